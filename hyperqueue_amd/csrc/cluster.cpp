// hqcluster::WorkerSet and hqcluster::Retracting — the host side of the resident worker set (cluster.h; kernels: kernels.hip).
#include "cluster.h"
#include "clock_core.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace hqcluster {

#define HQ_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(HQTICK_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

// ---------------------------------------------------------------------------------------------- the table layout
TabLayout table_layout(uint32_t W, uint32_t R, uint32_t nv, uint32_t ne) {
    TabLayout L{};
    L.nv = nv; L.ne = ne;
    L.o_tot = 0; L.o_free = L.o_tot + (size_t)W * R * 8; L.o_rem = L.o_free + (size_t)W * R * 8; L.o_amt = L.o_rem + (size_t)W * 8; L.o_time = L.o_amt + (size_t)L.ne * 8;
    L.o_off = L.o_time + (size_t)L.nv * 8; L.o_res = L.o_off + (size_t)(L.nv + 1) * 4; L.o_kind = L.o_res + (size_t)L.ne * 4; L.bytes = L.o_kind + L.ne + 64;
    return L;
}
TabLayout table_layout(const hqtick_snapshot *s, uint32_t W) {
    const uint32_t nv = s->n_requests ? s->rq_variant_off[s->n_requests] : 0;
    return table_layout(W, s->n_resources, nv, nv ? s->variant_entry_off[nv] : 0);
}
void pack_worker_rows(unsigned char *h, const TabLayout &L, uint32_t W, uint32_t R, const uint64_t *total, const uint64_t *free_, const int64_t *rem) {
    if (W && R) { memcpy(h + L.o_tot, total, (size_t)W * R * 8); memcpy(h + L.o_free, free_, (size_t)W * R * 8); }
    int64_t *hr = reinterpret_cast<int64_t *>(h + L.o_rem);
    if (rem) memcpy(hr, rem, (size_t)W * 8); else for (uint32_t w = 0; w < W; w++) hr[w] = HQ_NO_TIME_LIMIT;
}
void pack_request_tables(unsigned char *h, const TabLayout &L, const hqtick_snapshot *s) {
    if (!L.nv) return;
    memcpy(h + L.o_amt, s->entry_amount, (size_t)L.ne * 8);
    if (s->variant_min_time_ns) memcpy(h + L.o_time, s->variant_min_time_ns, (size_t)L.nv * 8); else memset(h + L.o_time, 0, (size_t)L.nv * 8);
    memcpy(h + L.o_off, s->variant_entry_off, (size_t)(L.nv + 1) * 4);
    memcpy(h + L.o_res, s->entry_resource, (size_t)L.ne * 4);
    memcpy(h + L.o_kind, s->entry_kind, L.ne);
}
void view_tables(unsigned char *d, const TabLayout &L, UpView *uv) {
    uv->total = (const uint64_t *)(d + L.o_tot); uv->free_ = (const uint64_t *)(d + L.o_free); uv->rem = (const int64_t *)(d + L.o_rem);
    uv->rt.entry_amount = (const uint64_t *)(d + L.o_amt); uv->rt.variant_min_time_ns = (const uint64_t *)(d + L.o_time);
    uv->rt.variant_entry_off = (const uint32_t *)(d + L.o_off); uv->rt.entry_resource = (const uint32_t *)(d + L.o_res);
    uv->rt.entry_kind = (const uint8_t *)(d + L.o_kind); uv->rt.n_variants = L.nv; uv->n_entries = L.ne;
}

// ---------------------------------------------------------------------------------------------- WorkerSet
int WorkerSet::init() {
    if (const char *e = getenv("HQTICK_CHECK_CLUSTER")) check = atoi(e) != 0;
    HQ_HIP(hipEventCreate(&ev));
    return 0;
}
void WorkerSet::release() {
    d_tab.release(); d_next.release(); h_tab.release(); h_delta.release(); d_deadline.release(); h_deadline.release();
    if (ev) hipEventDestroy(ev);
    ev = nullptr; pending = false; valid_ = false; clock_mode_ = false;
}
int WorkerSet::wait() {
    if (pending) { HQ_HIP(hipEventSynchronize(ev)); pending = false; }
    return 0;
}
int WorkerSet::staged(hipStream_t st) {
    HQ_HIP(hipEventRecord(ev, st)); pending = true;
    return 0;
}

int WorkerSet::upload(hipStream_t st, const hqtick_snapshot *s) {
    const uint32_t W = s->n_workers, R = s->n_resources;
    const TabLayout L = table_layout(s, W);
    if (int rc = wait()) return rc;
    HQ_HIP(hipStreamSynchronize(st));
    if (!h_tab.ensure(L.bytes) || !d_tab.ensure(L.bytes + 65536)) return fail(HQTICK_E_DEVICE, "allocating cluster tables");
    unsigned char *h = h_tab.as<unsigned char>();
    memset(h, 0, L.bytes);
    pack_worker_rows(h, L, W, R, s->worker_total, s->worker_free, s->worker_remaining_ns);
    pack_request_tables(h, L, s);
    HQ_HIP(hipMemcpyAsync(d_tab.p, h, L.bytes, hipMemcpyHostToDevice, st));
    HQ_HIP(hipStreamSynchronize(st));
    rt.assign(h + L.o_amt, h + L.bytes);
    W_ = W; R_ = R; valid_ = true; clock_mode_ = false;
    id.assign(s->worker_id, s->worker_id + W);
    wmap_ = hqhb::U32Map(); for (uint32_t w = 0; w < W; w++) wmap_.insert(id[w], 0); rank_dirty = true;  // (WorkerIds are minted ascending: a fresh map filled in that order)
    total.assign(s->worker_total, s->worker_total + (size_t)W * R); free_.assign(s->worker_free, s->worker_free + (size_t)W * R);
    rem.assign(W, HQ_NO_TIME_LIMIT); if (s->worker_remaining_ns) rem.assign(s->worker_remaining_ns, s->worker_remaining_ns + W);
    min_util.assign(W, 0.0f); if (s->worker_min_utilization) min_util.assign(s->worker_min_utilization, s->worker_min_utilization + W);
    flags_.assign(W, HQ_WORKER_SN); if (s->worker_flags) flags_.assign(s->worker_flags, s->worker_flags + W);
    group.assign(W, 0); if (s->worker_group) group.assign(s->worker_group, s->worker_group + W);
    n_groups = s->n_groups ? s->n_groups : 1;
    blocked.clear();
    for (uint32_t i = 0; i < s->n_blocked; i++) blocked[s->worker_id[s->blocked_worker[i]]].push_back({s->blocked_rq[i], s->blocked_variant[i]});
    blk_dirty = true;
    return 0;
}

int WorkerSet::update_rows(hipStream_t st, uint32_t n, const uint32_t *worker_index, const uint64_t *free_rows, const int64_t *remaining_ns) {
    const uint32_t R = R_;
    for (uint32_t i = 0; i < n; i++) if (worker_index[i] >= W_) return fail(HQTICK_E_INVALID, "hqtick_cluster_update_workers: worker index out of range");
    // staging: [free n*R u64][rem n i64][index n u32]; the scatter kernel reads it in place (pinned, device-mapped) — wait for the previous one first
    if (int rc = wait()) return rc;
    const size_t o_rem = (size_t)n * R * 8, o_idx = o_rem + (size_t)n * 8, bytes = o_idx + (size_t)n * 4 + 16;
    if (!h_delta.ensure(bytes)) return fail(HQTICK_E_DEVICE, "allocating delta staging");
    unsigned char *h = h_delta.as<unsigned char>(), *d = h_delta.dev<unsigned char>();
    memcpy(h, free_rows, o_rem);
    const bool to_deadline = remaining_ns && clock_mode_;  // clock mode: a remaining lifetime is one at the current clock and moves the row's deadline, not the column
    if (remaining_ns) memcpy(h + o_rem, remaining_ns, (size_t)n * 8);
    memcpy(h + o_idx, worker_index, (size_t)n * 4);
    for (uint32_t i = 0; i < n; i++) {  // the host mirror follows
        memcpy(free_.data() + (size_t)worker_index[i] * R, free_rows + (size_t)i * R, (size_t)R * 8);
        if (to_deadline) deadline[worker_index[i]] = hqclock::deadline_of(now_, remaining_ns[i]);
        else if (remaining_ns) rem[worker_index[i]] = remaining_ns[i];
    }
    if (to_deadline) dl_dirty = rem_dirty = true;
    const TabLayout L = table_layout(W_, R, 0, 0);
    HQ_HIP(hqk::scatter_worker_rows(reinterpret_cast<uint64_t *>(rows() + L.o_free), reinterpret_cast<int64_t *>(rows() + L.o_rem), R, n, reinterpret_cast<const uint32_t *>(d + o_idx),
                                    reinterpret_cast<const uint64_t *>(d), remaining_ns && !to_deadline ? reinterpret_cast<const int64_t *>(d + o_rem) : nullptr, st));
    return staged(st);
}

int WorkerSet::rows_of(const char *fn, uint32_t n, const uint32_t *worker_id, std::vector<uint32_t> *row, const std::function<int(uint32_t, uint32_t)> &also) {
    std::vector<uint8_t> seen(W_, 0);
    row->resize(n);
    for (uint32_t i = 0; i < n; i++) {
        auto it = std::lower_bound(id.begin(), id.end(), worker_id[i]);
        if (it == id.end() || *it != worker_id[i] || seen[it - id.begin()]) return fail(HQTICK_E_INVALID, std::string(fn) + ": unknown (or repeated) worker id");
        (*row)[i] = (uint32_t)(it - id.begin()); seen[(*row)[i]] = 1;
        if (also) { if (int rc = also(i, (*row)[i])) return rc; }
    }
    return 0;
}

int WorkerSet::plan_add(uint32_t n, const uint32_t *worker_id, const uint32_t *grp, std::vector<uint32_t> *src) {
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t prev = i ? worker_id[i - 1] : (W_ ? id[W_ - 1] : 0u);
        if ((i || W_) && worker_id[i] <= prev) return fail(HQTICK_E_INVALID, "hqtick_cluster_add_workers: ids must ascend above every id present");
        if (grp && grp[i] >= 65536) return fail(HQTICK_E_INVALID, "hqtick_cluster_add_workers: group index");
    }
    src->resize(W_ + n);
    for (uint32_t i = 0; i < W_ + n; i++) (*src)[i] = i;
    return 0;
}

int WorkerSet::plan_remove(uint32_t n, const uint32_t *worker_id, std::vector<uint32_t> *src) {
    std::vector<uint32_t> row;
    if (int rc = rows_of("hqtick_cluster_remove_workers", n, worker_id, &row)) return rc;
    std::vector<uint8_t> gone(W_, 0);
    for (uint32_t r : row) gone[r] = 1;
    src->clear(); src->reserve(W_ - n);
    for (uint32_t w = 0; w < W_; w++) if (!gone[w]) src->push_back(w);
    return 0;
}

// One re-pack kernel, request tables copied device to device.  The staging of the new workers' rows sits behind the row map in the pinned delta buffer.
int WorkerSet::repack(hipStream_t st, const std::vector<uint32_t> &src, uint32_t n_add, const uint64_t *add_total, const uint64_t *add_free, const int64_t *add_rem) {
    const uint32_t W_old = W_, R = R_, W_new = (uint32_t)src.size();
    if (int rc = wait()) return rc;
    const TabLayout Lo = table_layout(W_old, R, 0, 0), Ln = table_layout(W_new, R, 0, 0);
    if (!d_next.ensure(Ln.o_amt + rt.size() + 65536)) return fail(HQTICK_E_DEVICE, "allocating cluster tables");
    const size_t o_tot = ((size_t)W_new * 4 + 15) & ~(size_t)15, o_fr = o_tot + (size_t)n_add * R * 8, o_rem = o_fr + (size_t)n_add * R * 8, bytes = o_rem + (size_t)n_add * 8 + 64;
    if (!h_delta.ensure(bytes)) return fail(HQTICK_E_DEVICE, "allocating delta staging");
    unsigned char *h = h_delta.as<unsigned char>(), *d = h_delta.dev<unsigned char>();
    memcpy(h, src.data(), (size_t)W_new * 4);
    if (n_add) {
        memcpy(h + o_tot, add_total, (size_t)n_add * R * 8); memcpy(h + o_fr, add_free, (size_t)n_add * R * 8);
        if (add_rem) memcpy(h + o_rem, add_rem, (size_t)n_add * 8); else std::fill_n(reinterpret_cast<int64_t *>(h + o_rem), n_add, (int64_t)HQ_NO_TIME_LIMIT);
    }
    unsigned char *ob = d_tab.as<unsigned char>(), *nb = d_next.as<unsigned char>();
    HQ_HIP(hqk::repack_worker_rows(reinterpret_cast<const uint64_t *>(ob + Lo.o_tot), reinterpret_cast<const uint64_t *>(ob + Lo.o_free), reinterpret_cast<const int64_t *>(ob + Lo.o_rem), W_old, R, W_new,
                                   reinterpret_cast<const uint32_t *>(d), reinterpret_cast<const uint64_t *>(d + o_tot), reinterpret_cast<const uint64_t *>(d + o_fr), reinterpret_cast<const int64_t *>(d + o_rem),
                                   reinterpret_cast<uint64_t *>(nb + Ln.o_tot), reinterpret_cast<uint64_t *>(nb + Ln.o_free), reinterpret_cast<int64_t *>(nb + Ln.o_rem), st));
    if (!rt.empty()) HQ_HIP(hipMemcpyAsync(nb + Ln.o_amt, ob + Lo.o_amt, rt.size(), hipMemcpyDeviceToDevice, st));
    if (int rc = staged(st)) return rc;
    std::swap(d_tab, d_next);
    W_ = W_new;
    return 0;
}

void WorkerSet::add_rows(uint32_t n, const uint32_t *worker_id, const uint64_t *tot, const uint64_t *free_rows, const int64_t *rem_ns, const float *mu, const uint8_t *fl, const uint32_t *grp) {
    const uint32_t R = R_;
    id.insert(id.end(), worker_id, worker_id + n);
    for (uint32_t i = 0; i < n; i++) wmap_.insert(worker_id[i], 0);
    rank_dirty = true;
    total.insert(total.end(), tot, tot + (size_t)n * R); free_.insert(free_.end(), free_rows, free_rows + (size_t)n * R);
    for (uint32_t i = 0; i < n; i++) {
        rem.push_back(rem_ns ? rem_ns[i] : (int64_t)HQ_NO_TIME_LIMIT); min_util.push_back(mu ? mu[i] : 0.0f); flags_.push_back(fl ? fl[i] : (uint8_t)HQ_WORKER_SN);
        group.push_back(grp ? grp[i] : 0u); if (grp && grp[i] + 1 > n_groups) n_groups = grp[i] + 1;
        if (clock_mode_) deadline.push_back(hqclock::deadline_of(now_, rem.back()));  // (the re-pack wrote the plain lifetime into the column: the next tick's k_clock_rows replaces it)
    }
    if (clock_mode_) dl_dirty = rem_dirty = true;
    blk_dirty = true;
}

void WorkerSet::keep_rows(const std::vector<uint32_t> &src) {
    const uint32_t R = R_, W_old = (uint32_t)id.size();
    uint32_t k = 0;
    for (uint32_t w = 0; w < W_old; w++) {
        if (k == src.size() || src[k] != w) { blocked.erase(id[w]); wmap_.remove(id[w]); rank_dirty = true; continue; }
        if (k != w) {
            id[k] = id[w]; rem[k] = rem[w]; min_util[k] = min_util[w]; flags_[k] = flags_[w]; group[k] = group[w];
            if (clock_mode_) deadline[k] = deadline[w];
            memmove(total.data() + (size_t)k * R, total.data() + (size_t)w * R, (size_t)R * 8); memmove(free_.data() + (size_t)k * R, free_.data() + (size_t)w * R, (size_t)R * 8);
        }
        k++;
    }
    id.resize(k); rem.resize(k); min_util.resize(k); flags_.resize(k); group.resize(k); total.resize((size_t)k * R); free_.resize((size_t)k * R);
    if (clock_mode_) { deadline.resize(k); dl_dirty = rem_dirty = true; }
    blk_dirty = true;
}

int WorkerSet::set_clock(int64_t now_ns) {
    if (!clock_mode_) {  // a host that uploaded lifetimes taken at now_ns loses nothing
        deadline.resize(W_);
        for (uint32_t w = 0; w < W_; w++) deadline[w] = hqclock::deadline_of(now_ns, rem[w]);
        thr_src.clear(); thr.clear();
        clock_mode_ = true; dl_dirty = rem_dirty = true;
    } else if (now_ns != now_) rem_dirty = true;
    now_ = now_ns;
    return 0;
}

int WorkerSet::set_blocked(uint32_t worker_id, uint32_t n, const uint32_t *rq, const uint8_t *variant) {
    if (!std::binary_search(id.begin(), id.end(), worker_id)) return fail(HQTICK_E_INVALID, "hqtick_cluster_set_blocked: unknown worker id");
    if (n && (!rq || !variant)) return fail(HQTICK_E_INVALID, "hqtick_cluster_set_blocked: null array");
    if (n == 0) blocked.erase(worker_id);
    else { auto &v = blocked[worker_id]; v.clear(); for (uint32_t i = 0; i < n; i++) v.push_back({rq[i], variant[i]}); }
    blk_dirty = true;
    return 0;
}
int WorkerSet::block(uint32_t worker_id, uint32_t rq, uint8_t variant) {
    if (!std::binary_search(id.begin(), id.end(), worker_id)) return 0;
    auto &v = blocked[worker_id];
    if (std::find(v.begin(), v.end(), std::make_pair(rq, variant)) != v.end()) return 0;
    v.push_back({rq, variant}); blk_dirty = true;
    return 1;
}
int WorkerSet::enable_request(uint32_t worker_id, uint32_t rq, uint8_t variant) {
    if (!std::binary_search(id.begin(), id.end(), worker_id)) return fail(HQTICK_E_INVALID, "hqtick_cluster_enable_request: unknown worker id");
    const auto it = blocked.find(worker_id);
    if (it == blocked.end()) return 0;
    const auto p = std::find(it->second.begin(), it->second.end(), std::make_pair(rq, variant));
    if (p == it->second.end()) return 0;
    it->second.erase(p);
    if (it->second.empty()) blocked.erase(it);
    blk_dirty = true;
    return 1;
}
int WorkerSet::blocked_of(uint32_t worker_id, uint32_t *n, const uint32_t **rq, const uint8_t **variant) {
    if (!std::binary_search(id.begin(), id.end(), worker_id)) return fail(HQTICK_E_INVALID, "hqtick_cluster_blocked: unknown worker id");
    bo_rq.clear(); bo_variant.clear();
    const auto it = blocked.find(worker_id);
    if (it != blocked.end()) for (const auto &p : it->second) { bo_rq.push_back(p.first); bo_variant.push_back(p.second); }
    if (n) *n = (uint32_t)bo_rq.size();
    if (rq) *rq = bo_rq.data();
    if (variant) *variant = bo_variant.data();
    return 0;
}

int WorkerSet::set_flags(uint32_t n, const uint32_t *worker_id, const uint8_t *fl, bool sn_is_the_ledgers) {
    std::vector<uint32_t> row;
    auto flag_ok = [&](uint32_t i, uint32_t r) {
        if (fl[i] & ~(uint8_t)(HQ_WORKER_SN | HQ_WORKER_STOPPING)) return fail(HQTICK_E_INVALID, "hqtick_cluster_set_flags: undefined flag bits");
        if (sn_is_the_ledgers && ((fl[i] ^ flags_[r]) & HQ_WORKER_SN))
            return fail(HQTICK_E_INVALID, "hqtick_cluster_set_flags: with the assignment ledger on, HQ_WORKER_SN follows the ledger's multi-node tasks");
        return 0;
    };
    if (int rc = rows_of("hqtick_cluster_set_flags", n, worker_id, &row, flag_ok)) return rc;
    for (uint32_t i = 0; i < n; i++) flags_[row[i]] = fl[i];
    return 0;
}

int WorkerSet::complete(const hqtick_snapshot *s, hqtick_snapshot *full) {
    *full = *s;
    const bool mine = s->worker_id == nullptr && valid_;
    if (s->n_workers == HQ_WORKERS_RESIDENT && !mine)
        return fail(HQTICK_E_INVALID, s->worker_id ? "n_workers == HQ_WORKERS_RESIDENT with worker arrays in the snapshot"
                                                   : "n_workers == HQ_WORKERS_RESIDENT without a resident worker set (hqtick_cluster_upload; dropped by hqtick_cluster_drop)");
    if (clock_mode_ && valid_ && !mine) return fail(HQTICK_E_INVALID, "clock mode (hqtick_cluster_set_clock): the tick runs on the resident worker set, the snapshot must not carry worker arrays as well");
    if (!mine) return 0;
    const uint32_t W = W_;
    if (s->n_workers != 0 && s->n_workers != HQ_WORKERS_RESIDENT && s->n_workers != W) return fail(HQTICK_E_INVALID, "snapshot without worker arrays: n_workers must be HQ_WORKERS_RESIDENT, 0 or the resident worker count");
    if (s->n_resources != R_) return fail(HQTICK_E_INVALID, "snapshot without worker arrays: n_resources differs from the resident tables");
    if (blk_dirty) {
        blk_worker.clear(); blk_rq.clear(); blk_variant.clear();
        for (uint32_t w = 0; w < W; w++) { auto it = blocked.find(id[w]); if (it == blocked.end()) continue; for (auto &p : it->second) { blk_worker.push_back(w); blk_rq.push_back(p.first); blk_variant.push_back(p.second); } }
        blk_dirty = false;
    }
    if (clock_mode_) {  // the mirror's remaining lifetimes against this snapshot's thresholds: what k_clock_rows writes into the column (tables(), behind the request tables)
        const uint32_t nv = s->n_requests ? s->rq_variant_off[s->n_requests] : 0;
        const bool zeros = !s->variant_min_time_ns;  // (packed as zeros)
        bool same_thr = thr_src.size() == nv;
        for (uint32_t v = 0; same_thr && v < nv; v++) same_thr = thr_src[v] == (zeros ? 0 : s->variant_min_time_ns[v]);
        if (!same_thr) {
            thr_src.resize(nv);
            for (uint32_t v = 0; v < nv; v++) thr_src[v] = zeros ? 0 : s->variant_min_time_ns[v];
            thr = thr_src; std::sort(thr.begin(), thr.end()); thr.erase(std::unique(thr.begin(), thr.end()), thr.end());
            rem_dirty = true;
        }
        if (rem_dirty) {
            for (uint32_t w = 0; w < W; w++) rem[w] = hqclock::canonical_sorted(deadline[w], now_, thr.data(), (uint32_t)thr.size());
            rem_dirty = false; kernel_due = true;
        }
    }
    full->n_workers = W; full->worker_id = id.data(); full->worker_total = total.data(); full->worker_free = free_.data(); full->worker_remaining_ns = rem.data();
    full->worker_min_utilization = min_util.data(); full->worker_flags = flags_.data(); full->worker_group = group.data(); full->n_groups = n_groups;
    if (rank_dirty) {
        rank_.assign(W, 0); uint32_t pos = 0;
        wmap_.for_each([&](uint32_t key, uint32_t) { const auto it = std::lower_bound(id.begin(), id.end(), key); if (it != id.end() && *it == key) rank_[it - id.begin()] = pos++; });
        rank_dirty = false;
    }
    full->worker_map_rank = rank_.data();
    full->n_blocked = (uint32_t)blk_worker.size(); full->blocked_worker = blk_worker.data(); full->blocked_rq = blk_rq.data(); full->blocked_variant = blk_variant.data();
    return 0;
}

int WorkerSet::tables(hipStream_t st, const hqtick_snapshot *s, uint32_t W, UpView *uv) {
    const uint32_t R = s->n_resources;
    if (W != W_ || R != R_) return fail(HQTICK_E_INVALID, "cluster tables in HBM were uploaded for another worker set (hqtick_cluster_upload after workers join or leave)");
    const TabLayout L = table_layout(s, W);
    if (hqk::worker_eval_lds(R, L.nv, L.ne) > 150 * 1024) return fail(HQTICK_E_CAPACITY, "request table + 32 worker rows exceed the 150 KiB the worker-evaluation kernel stages in LDS");
    const size_t rt_bytes = L.bytes - L.o_amt;
    if (int rc = wait()) return rc;  // h_tab is the staging of the previous request-table upload
    if (L.bytes > d_tab.cap) {  // the request tables outgrew the allocation: move the worker rows over
        hqbuf::DevBuf nb;
        if (!nb.ensure(L.bytes * 2)) return fail(HQTICK_E_DEVICE, "allocating cluster tables");
        HQ_HIP(hipStreamSynchronize(st));
        HQ_HIP(hipMemcpy(nb.p, d_tab.p, L.o_amt, hipMemcpyDeviceToDevice));
        d_tab.release(); d_tab = nb;
    }
    if (!h_tab.ensure(L.bytes)) return fail(HQTICK_E_DEVICE, "allocating cluster tables");
    unsigned char *h = h_tab.as<unsigned char>();
    memset(h + L.o_amt, 0, rt_bytes);
    pack_request_tables(h, L, s);
    if (rt.size() != rt_bytes || memcmp(rt.data(), h + L.o_amt, rt_bytes) != 0) {  // new request classes: a few hundred bytes, stream-ordered before K2
        HQ_HIP(hipMemcpyAsync(rows() + L.o_amt, h + L.o_amt, rt_bytes, hipMemcpyHostToDevice, st));
        if (int rc = staged(st)) return rc;
        rt.assign(h + L.o_amt, h + L.o_amt + rt_bytes);
    }
    if (clock_mode_ && kernel_due) {  // something k_clock_rows reads changed since its last run: the clock, a deadline, the membership or the thresholds (complete())
        if (dl_dirty) {
            if (!h_deadline.ensure((size_t)W * 8 + 64) || !d_deadline.ensure((size_t)W * 8 + 64)) return fail(HQTICK_E_DEVICE, "allocating the deadline column");
            if (W) { memcpy(h_deadline.p, deadline.data(), (size_t)W * 8); HQ_HIP(hipMemcpyAsync(d_deadline.p, h_deadline.p, (size_t)W * 8, hipMemcpyHostToDevice, st)); }
            dl_dirty = false;
        }
        HQ_HIP(hqk::clock_rows(d_deadline.as<int64_t>(), now_, reinterpret_cast<const uint64_t *>(rows() + L.o_time), L.nv, W, reinterpret_cast<int64_t *>(rows() + L.o_rem), st));
        if (int rc = staged(st)) return rc;
        kernel_due = false; n_clock_launches++;
    }
    if (check) {  // HQTICK_CHECK_CLUSTER=1 (tests): the rows in HBM must be the rows of the snapshot
        std::vector<unsigned char> dev(L.o_amt);
        HQ_HIP(hipMemcpyAsync(dev.data(), d_tab.p, L.o_amt, hipMemcpyDeviceToHost, st));
        HQ_HIP(hipStreamSynchronize(st));
        std::vector<unsigned char> want(L.o_amt);
        pack_worker_rows(want.data(), L, W, R, s->worker_total, s->worker_free, s->worker_remaining_ns);
        if (memcmp(dev.data(), want.data(), L.o_amt) != 0) return fail(HQTICK_E_INVALID, "cluster tables in HBM differ from the snapshot's worker rows (a missed hqtick_cluster_update_workers)");
    }
    view_tables(rows(), L, uv);
    return 0;
}

// ---------------------------------------------------------------------------------------------- Retracting
void Retracting::add(uint32_t n, const uint64_t *task_id, const uint32_t *worker_id) {
    for (uint32_t i = 0; i < n; i++) tab[task_id[i]] = Entry{worker_id[i], true, false, 0, 0};
}

int Retracting::response(uint32_t worker_id, uint32_t n, const uint64_t *task_id) {
    last.clear();
    int left = 0;
    for (uint32_t i = 0; i < n; i++) left += take(worker_id, task_id[i], &last) ? 1 : 0;
    return left;
}

bool Retracting::take(uint32_t worker_id, uint64_t task_id, Reassigned *out, bool *redirected) {
    auto it = tab.find(task_id);
    if (it == tab.end() || it->second.old_id != worker_id) return false;  // "retracted task is in invalid state"  reactor.rs:476-481
    if (it->second.has_redirect) out->push(task_id, it->second.target_id, it->second.variant);
    if (redirected) *redirected = it->second.has_redirect;
    tab.erase(it);
    return true;
}

void Retracting::sources(std::vector<uint64_t> *task_id, std::vector<uint32_t> *worker_id) const {
    task_id->clear(); worker_id->clear();
    for (const auto &kv : tab) { task_id->push_back(kv.first); worker_id->push_back(kv.second.old_id); }  // (std::map: ascending task id)
}

// on_remove_worker's two passes over the Retracting tasks (server/reactor.rs:86-147), one pass over the table however many workers are lost
void Retracting::workers_removed(uint32_t n, const uint32_t *worker_id) {
    last.clear();
    if (tab.empty()) return;
    std::vector<uint32_t> lost(worker_id, worker_id + n);
    std::sort(lost.begin(), lost.end());
    auto is_lost = [&](uint32_t id) { return std::binary_search(lost.begin(), lost.end(), id); };
    for (auto it = tab.begin(); it != tab.end();) {
        Entry &e = it->second;
        if (is_lost(e.old_id)) {
            // the worker it was retracting from is gone: with a redirect (to a worker that stays) the task is Assigned{target} now and the host sends its
            // ComputeTasks message (reactor.rs:131-141) — reported through hqtick_cluster_last_reassigned; without one it is a Waiting task of its queue
            if (e.has_redirect && !is_lost(e.target_id)) last.push(it->first, e.target_id, e.variant);
            it = tab.erase(it);
            continue;
        }
        // the redirect TARGET is gone: the redirect is dropped and the task goes back into its queue, still Retracting{old} (reactor.rs:89-94: redirects.remove +
        // add_ready_task) — the host re-adds it to the resident ready set with the other tasks of the lost worker; the next tick sees it as Retracting again
        if (e.has_redirect && is_lost(e.target_id)) { e.has_redirect = false; e.in_queue = true; }
        ++it;
    }
}

int Retracting::to_snapshot(const uint32_t *worker_id, uint32_t W, hqtick_snapshot *full) {
    if (!worker_id) { err = "resident retracting table without worker ids (hqtick_cluster_upload, or worker arrays in the snapshot)"; return HQTICK_E_INVALID; }
    auto index_of = [&](uint32_t id) -> uint32_t { const uint32_t *e = worker_id + W, *it = std::lower_bound(worker_id, e, id); return (it != e && *it == id) ? (uint32_t)(it - worker_id) : HQ_NO_WORKER; };
    s_task.clear(); s_worker.clear(); s_red_worker.clear(); s_red_variant.clear();
    for (auto &kv : tab) {  // (std::map: ascending task id, as the snapshot wants it)
        if (!kv.second.in_queue) continue;
        const uint32_t oi = index_of(kv.second.old_id);
        if (oi == HQ_NO_WORKER) { err = "a Retracting task's worker is not in the worker set"; return HQTICK_E_INVALID; }
        s_task.push_back(kv.first); s_worker.push_back(oi);
        s_red_worker.push_back(kv.second.has_redirect ? index_of(kv.second.target_id) : HQ_NO_WORKER); s_red_variant.push_back(kv.second.variant);
    }
    full->n_retracting = (uint32_t)s_task.size();
    full->retracting_task = s_task.data(); full->retracting_worker = s_worker.data();
    full->retracting_redirect_worker = s_red_worker.data(); full->retracting_redirect_variant = s_red_variant.data();
    return 0;
}

void Retracting::apply_tick(const uint32_t *worker_id, uint32_t W, const std::vector<uint32_t> &retract_off, const std::vector<uint64_t> &retract_task, const std::vector<uint64_t> &red_task,
                            const std::vector<uint32_t> &red_worker, const std::vector<uint8_t> &red_variant, const std::vector<uint8_t> &red_kind) {
    for (uint32_t w = 0; w < W && w + 1 < retract_off.size(); w++)   // Prefilled{old} -> Retracting{old}: out of a prefill set, not in a queue
        for (uint32_t i = retract_off[w]; i < retract_off[w + 1]; i++) tab[retract_task[i]] = Entry{worker_id[w], false, false, 0, 0};
    for (size_t i = 0; i < red_task.size(); i++) {
        auto it = tab.find(red_task[i]);
        if (it == tab.end()) continue;
        Entry &e = it->second;
        const uint8_t kind = i < red_kind.size() ? red_kind[i] : (uint8_t)HQ_REDIRECT_FROM_PREFILL;
        e.in_queue = false;  // take_tasks removed it from its queue (or it came out of a prefill set)
        if (kind == HQ_REDIRECT_SAME_WORKER) continue;  // back on the worker it is retracting from: insert_sn_task(old) only, the redirect table is untouched (mapping.rs:66-80)
        if (red_worker[i] < W) { e.has_redirect = true; e.target_id = worker_id[red_worker[i]]; e.variant = red_variant[i]; }
    }
}

}  // namespace hqcluster

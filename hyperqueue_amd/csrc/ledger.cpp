// hqasg::Ledger — the host side of the assignment ledger (ledger.h; kernels: assigned.hip).
#include "ledger.h"

#include "graph.h"
#include "lose_core.h"

namespace hqasg {

#define HQ_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(HQTICK_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

void Ledger::release_all() {
    tab.release(); tab2.release(); for (RowPair *r : {&counts, &mn, &pf}) r->release();
    for (DevBuf &b : buf) b.release();
    h_ctr.release(); h_in.release(); h_cancel.release(); h_finish.release(); h_fail.release(); h_start.release(); h_reject.release(); h_lose.release();
}
void Ledger::take_requests(const hqtick_snapshot *s) {
    const uint32_t Q = s->n_requests;
    if (Q && (!s->rq_variant_off || !s->variant_entry_off)) return;  // (validate() reports it)
    const uint32_t nv = Q ? s->rq_variant_off[Q] : 0, ne = nv ? s->variant_entry_off[nv] : 0;
    if (ne && (!s->entry_resource || !s->entry_kind || !s->entry_amount)) return;
    std::vector<uint32_t> vn(nv, 0); if (s->variant_n_nodes) vn.assign(s->variant_n_nodes, s->variant_n_nodes + nv);
    if (rq_off.size() == (size_t)Q + 1 && vent_off.size() == (size_t)nv + 1 && ent_res.size() == ne && var_nodes == vn && std::equal(rq_off.begin(), rq_off.end(), s->rq_variant_off ? s->rq_variant_off : rq_off.data()) &&
        (nv == 0 || std::equal(vent_off.begin(), vent_off.end(), s->variant_entry_off)) && (ne == 0 || (std::equal(ent_res.begin(), ent_res.end(), s->entry_resource) &&
        std::equal(ent_kind.begin(), ent_kind.end(), s->entry_kind) && std::equal(ent_amt.begin(), ent_amt.end(), s->entry_amount))))
        return;
    rq_off.assign(1, 0); if (Q) rq_off.assign(s->rq_variant_off, s->rq_variant_off + Q + 1);
    vent_off.assign(1, 0); if (nv) vent_off.assign(s->variant_entry_off, s->variant_entry_off + nv + 1);
    ent_res.assign(s->entry_resource, s->entry_resource + ne); ent_kind.assign(s->entry_kind, s->entry_kind + ne); ent_amt.assign(s->entry_amount, s->entry_amount + ne);
    var_nodes.swap(vn);
    req_dirty = true;
}

// the request tables on the device: [rq_off Q + 1 u32][vent_off nv + 1 u32][ent_res ne u32][ent_amt ne u64][ent_kind ne u8]
Req Ledger::req(unsigned char *h) const {
    Pack pk{h, buf[B_REQ].as<unsigned char>()};
    Req r{};
    r.rq_off = pk.put(rq_off.data(), rq_off.size()); r.ventry_off = pk.put(vent_off.data(), vent_off.size()); r.ent_res = pk.put(ent_res.data(), ent_res.size());
    r.ent_amount = pk.put(ent_amt.data(), ent_amt.size(), 8); r.ent_kind = pk.put(ent_kind.data(), ent_kind.size()); r.Q = (uint32_t)rq_off.size() - 1;
    return r;
}
// a row table grows to `cols` columns (rounded up): zeroed, the rows copied over
int Ledger::widen(const Env &e, RowPair &t, uint32_t &t_stride, size_t cols, const char *what) {
    const uint32_t ns = row_stride(cols);
    const size_t bytes = (size_t)e.W * ns * 4 + 64;
    if (!t.next.ensure(bytes)) return fail(HQTICK_E_DEVICE, what);
    HQ_HIP(hipMemsetAsync(t.next.p, 0, bytes, e.stream));
    if (t_stride) HQ_HIP(repack_counts(t.cur.as<uint32_t>(), t_stride, e.W, nullptr, e.W, t.next.as<uint32_t>(), ns, t_stride, MnRows{}, MnRows{}, nullptr, e.stream));
    t.swap(); t_stride = ns; dirty_ = true;
    return 0;
}
// request tables + row-table widths on the device, as the host has them
int Ledger::sync_req(const Env &e) {
    const size_t Q = rq_off.size() - 1, nv = vent_off.size() - 1;
    if (nv > stride) { if (int rc = widen(e, counts, stride, nv, "hipMalloc assignment counts")) return rc; }  // new variant slots
    if (pf_on && Q > pf_stride) {  // new requests (Q <= variant slots: never wider than the count rows)
        if (int rc = widen(e, pf, pf_stride, Q, "hipMalloc prefilled counts")) return rc;
        pf_dirty = true;
    }
    if (!req_dirty) return 0;
    std::vector<unsigned char> h(req_bytes(), 0);
    HQ_HIP(hipStreamSynchronize(e.stream));  // (the previous tables may still be read by a queued kernel)
    if (!buf[B_REQ].ensure(h.size())) return fail(HQTICK_E_DEVICE, "hipMalloc ledger request tables");
    req(h.data());
    HQ_HIP(hipMemcpy(buf[B_REQ].p, h.data(), h.size(), hipMemcpyHostToDevice));
    req_dirty = false;
    return 0;
}
int Ledger::upload_wids(const Env &e) {
    if (!buf[B_WIDS].ensure(e.id->size() * 4 + 16)) return fail(HQTICK_E_DEVICE, "hipMalloc ledger worker ids");
    if (!e.id->empty()) HQ_HIP(hipMemcpyAsync(buf[B_WIDS].p, e.id->data(), e.id->size() * 4, hipMemcpyHostToDevice, e.stream));
    HQ_HIP(hipStreamSynchronize(e.stream));  // (pageable source)
    return 0;
}
// the flags column from the mirror (enable, hqtick_cluster_set_flags: the host is the writer, the mirror is current)
int Ledger::upload_flags(const Env &e) {
    if (e.W) HQ_HIP(hipMemcpyAsync(mn_rows(mn.cur, e.W, 0).flags, e.flags->data(), e.W, hipMemcpyHostToDevice, e.stream));
    HQ_HIP(hipStreamSynchronize(e.stream));  // (pageable source)
    return 0;
}
// room for `more` entries: live + tombstones + more stay under half the capacity; otherwise the live entries move to a fresh table
int Ledger::reserve(const Env &e, uint64_t more) {
    const uint64_t live = n_live + mn_live + (pf_on ? pf_live : 0);
    if (cap && (live + n_tomb + more) * 2 <= cap) return 0;
    uint64_t want = 1024; while (want < (live + more) * 4) want <<= 1;
    if (want > (1ull << 31)) return fail(HQTICK_E_CAPACITY, "assignment ledger: more than 2^29 entries");
    const uint32_t nc = (uint32_t)want;
    if (!tab2.ensure(nc)) return fail(HQTICK_E_DEVICE, "hipMalloc assignment ledger");
    const Table to = tab2.view(nc - 1);
    HQ_HIP(clear(to, e.stream));
    if (int rc = counted(e.stream, "hqasg::rehash", [&](uint32_t *ctr) { return cap ? rehash(table(), to, ctr, e.stream) : hipSuccess; })) return rc;
    if (cap && (c[C_FULL] || c[C_DONE] != live)) return fail(HQTICK_E_DEVICE, "assignment ledger: rebuild lost entries");
    std::swap(tab, tab2); cap = nc; n_tomb = 0;
    return 0;
}
// an insert batch (n > 0) from host columns, staged in pinned memory and read in place; c[C_OUT] entered, c[C_BAD] / c[C_DUP] refused
int Ledger::insert_host(const Env &e, uint32_t n, const uint64_t *id, const uint32_t *wid, const uint32_t *rq, const uint8_t *var, const uint64_t *prio, int upsert, int apply_free, const uint32_t *col_rq, int running) {
    if (int rc = reserve(e, n)) return rc;
    if (int rc = sync_req(e)) return rc;
    Pack pk;
    if (int rc = stage_in((size_t)n * 25, &pk)) return rc;
    Items it{};
    it.n = n; it.id = pk.put(id, n); it.wid = pk.put(wid, n); it.rq = pk.put(rq, n); it.prio = pk.put(prio, n, 8); it.variant = pk.put(var, n);
    if (!rq) std::fill_n(pk.host(it.rq), n, RQ_LOOKUP);  if (!prio) std::fill_n(pk.host(it.prio), n, (uint64_t)0);
    it.col_id = e.col_id; it.col_prio = e.col_prio; it.col_rq = col_rq ? col_rq : e.col_rq; it.col_n = e.col_n; it.run = running ? 1 : 0;
    if (int rc = counted(e.stream, "hqasg::insert", [&](uint32_t *ctr) { return insert(table(), req(), rows(e), it, upsert, apply_free, ctr, e.stream); })) return rc;
    if (c[C_FULL]) return fail(HQTICK_E_DEVICE, "assignment ledger: table full");
    n_live += c[C_OUT]; dirty_ = true;
    if (const uint32_t from_pf = std::min<uint64_t>(c[C_PF], pf_live)) { pf_live -= from_pf; n_live += from_pf; pf_dirty = true; }  // FROM_PREFILL redirects: prefilled entries that are assigned entries now
    return 0;
}

// multi-node placements (n > 0; task i on the workers wid[off[i] .. off[i + 1]), root first) enter table and rows; prio == nullptr: looked up in the ready-set columns.
// Few per call and built on the host, like the redirects: they are staged in pinned memory and read in place.  c[C_OUT] entered, c[C_BAD] + c[C_DUP] refused.
int Ledger::mn_enter(const Env &e, uint32_t n, const uint64_t *id, const uint32_t *rq, const uint64_t *prio, const uint32_t *off, const uint32_t *wid, int check) {
    const uint32_t W = e.W, n_wid = off[n];
    if (int rc = reserve(e, n)) return rc;
    if (int rc = sync_req(e)) return rc;
    Pack pk;
    if (int rc = stage_in((size_t)n * 24 + 4 + (size_t)n_wid * 4, &pk)) return rc;
    if (!buf[B_SCRATCH].ensure((size_t)W * 4 + 16)) return fail(HQTICK_E_DEVICE, "hipMalloc ledger scratch");
    MnItems it{};
    it.n = n; it.n_wid = n_wid; it.id = pk.put(id, n); it.prio = pk.put(prio, n); it.rq = pk.put(rq, n); it.off = pk.put(off, (size_t)n + 1); it.wid = pk.put(wid, n_wid);
    if (!prio) it.prio = nullptr;
    it.col_id = e.col_id; it.col_prio = e.col_prio; it.col_n = e.col_n;
    HQ_HIP(hipMemsetAsync(buf[B_SCRATCH].p, 0xFF, (size_t)W * 4 + 16, e.stream));
    if (int rc = counted(e.stream, "hqasg::mn_enter", [&](uint32_t *ctr) { return hqasg::mn_enter(table(), rows(e), mn_rows(mn.cur, W, mn_live), it, buf[B_SCRATCH].as<uint32_t>(), check, ctr, e.stream); })) return rc;
    if (c[C_FULL]) return fail(HQTICK_E_DEVICE, "assignment ledger: table full");
    mn_live += c[C_OUT];
    if (c[C_OUT]) { dirty_ = true; flags_dirty = true; }
    return 0;
}
bool Ledger::stage_for(uint32_t n_rec, bool ordered, uint32_t L, StageCols *c) {
    if (!buf[B_STAGE].ensure((size_t)n_rec * 22 + 64)) return false;
    Pack pk{nullptr, buf[B_STAGE].as<unsigned char>()}; const size_t n = n_rec;
    *c = stage_c = StageCols{pk.put<uint64_t>(nullptr, n), pk.put<uint32_t>(nullptr, n), pk.put<uint32_t>(nullptr, n), pk.put<uint32_t>(nullptr, n), pk.put<uint16_t>(nullptr, n)};
    stage_n = n_rec; stage_ordered = ordered; stage_L = L;
    return true;
}
void Ledger::collect_tick(const hqtick_snapshot *s, const hqtick_result *out, const std::vector<uint64_t> &new_free, const std::vector<uint32_t> &mn_rq, bool saved) {
    const uint32_t W = s->n_workers;
    pend_W = W; pend_free = new_free;
    red_id.clear(); red_wid.clear(); red_rq.clear(); red_var.clear(); red_prio.clear();
    for (uint32_t i = 0; i < out->n_redirects; i++) {
        uint32_t rq = RQ_LOOKUP; uint64_t pr = 0;
        if (out->redirect_kind[i] == HQ_REDIRECT_FROM_PREFILL && s->prefill_off && !pf_on)  // (with tracking on the task's prefilled entry knows both)  out of a prefill set: not in the ready set, the snapshot's prefill sets know it
            for (uint32_t q = 0; q < s->n_requests && rq == RQ_LOOKUP; q++)
                for (uint32_t j = s->prefill_off[q]; j < s->prefill_off[q + 1]; j++) if (s->prefill_task[j] == out->redirect_task[i]) { rq = q; pr = s->prefill_priority[q]; break; }
        red_id.push_back(out->redirect_task[i]); red_wid.push_back(out->redirect_worker[i] < W ? s->worker_id[out->redirect_worker[i]] : HQ_NO_WORKER);
        red_rq.push_back(rq); red_var.push_back(out->redirect_variant[i]); red_prio.push_back(pr);
    }
    pmn_id.clear(); pmn_rq.clear(); pmn_off.assign(1, 0); pmn_wid.clear();
    for (uint32_t i = 0; i < out->n_mn && i < mn_rq.size(); i++) {
        pmn_id.push_back(out->mn_task[i]); pmn_rq.push_back(mn_rq[i]);
        for (uint32_t j = out->mn_worker_off[i]; j < out->mn_worker_off[i + 1]; j++) pmn_wid.push_back(out->mn_worker[j] < W ? s->worker_id[out->mn_worker[j]] : HQ_NO_WORKER);
        pmn_off.push_back((uint32_t)pmn_wid.size());
    }
    pend_saved = saved; pending = true;
}

// a tick's placement becomes ledger state: its ASSIGN records and its redirects (upserts: a re-targeted task moves), free rows = the tick's new_free
int Ledger::apply_tick(const Env &e) {
    pending = false;
    const uint32_t W = e.W, n_rec = stage_n;
    const uint32_t *col_rq = pend_saved ? buf[B_SAVED_RQ].as<uint32_t>() : e.col_rq;
    stage_n = 0; last_host_bytes = 0;  // (no record data crosses from the host: the entries are where K5b staged them)
    if (pend_W != W || pend_free.size() != (size_t)W * e.R) return fail(HQTICK_E_INVALID, "assignment ledger: the worker set changed under a pending tick");
    if (n_rec) {
        if (int rc = reserve(e, n_rec)) return rc;
        if (int rc = sync_req(e)) return rc;
        const StageCols &sc = stage_c;  // (where stage_for put them for K5b)
        Staged st{};
        st.n = n_rec; st.task = sc.task; st.rq = sc.rq; st.row = sc.row; st.level = sc.level; st.meta = sc.meta;
        if (stage_ordered) { st.col_id = e.col_id; st.col_prio = e.col_prio; st.col_n = e.col_n; }  // the view's run table is in host memory
        else { st.levels = e.levels; st.n_levels = stage_L; }
        if (int rc = counted(e.stream, "hqasg::insert_staged", [&](uint32_t *ctr) { return insert_staged(table(), req(), rows(e), st, ctr, e.stream); })) return rc;
        if (c[C_FULL] || c[C_BAD] || (pf_on && c[C_DUP])) return fail(HQTICK_E_DEVICE, "assignment ledger: a record of the tick could not be entered");
        n_live += c[C_OUT];
        if (pf_on && c[C_PF]) { pf_live += c[C_PF]; pf_dirty = true; }  // its PREFILL records
    }
    if (!red_id.empty()) {
        if (int rc = insert_host(e, (uint32_t)red_id.size(), red_id.data(), red_wid.data(), red_rq.data(), red_var.data(), red_prio.data(), 1, 0, col_rq)) return rc;
        if (c[C_BAD]) return fail(HQTICK_E_DEVICE, "assignment ledger: a redirect of the tick could not be entered");
    }
    if (!pmn_id.empty()) {  // the multi-node placements (mapping.rs:133-154): the solver took free workers, so nothing is checked twice
        if (int rc = mn_enter(e, (uint32_t)pmn_id.size(), pmn_id.data(), pmn_rq.data(), nullptr, pmn_off.data(), pmn_wid.data(), 0)) return rc;
        if (c[C_BAD] + c[C_DUP] || c[C_OUT] != pmn_id.size()) return fail(HQTICK_E_DEVICE, "assignment ledger: a multi-node placement of the tick could not be entered");
        pmn_id.clear();
    }
    // free rows: the tick's new_free (Worker::insert_sn_task / remove_sn_task of mapping.rs, computed by the tick itself)
    if (W && e.R) {
        HQ_HIP(hipMemcpyAsync(e.cluster + (size_t)W * e.R * 8, pend_free.data(), (size_t)W * e.R * 8, hipMemcpyHostToDevice, e.stream));
        HQ_HIP(hipStreamSynchronize(e.stream));
        *e.free_ = pend_free;
    }
    dirty_ = true;
    return 0;
}

// the count rows follow a membership change: row w of the new set = old row src[w] (>= W_old: a new worker, zero)
// The multi-node columns move in the same launch; add_flags: the HQ_WORKER_* bytes of the new workers (nullptr: fresh single-node workers)
int Ledger::repack(const Env &e, const std::vector<uint32_t> &src, uint32_t W_old, const uint8_t *add_flags) {
    const uint32_t W_new = (uint32_t)src.size();
    if (!counts.next.ensure((size_t)W_new * stride * 4 + 64) || !buf[B_BATCH].ensure((size_t)W_new * 5 + 16) || !mn.next.ensure((size_t)W_new * 10 + 64)) return fail(HQTICK_E_DEVICE, "hipMalloc assignment counts");
    PfMove pfm{};
    if (pf_on) {  // the prefilled counts move in the same launch (pf_stride <= stride: both are the request tables' sizes rounded up alike)
        if (pf_stride > stride) return fail(HQTICK_E_DEVICE, "assignment ledger: prefilled table wider than the count rows");
        if (!pf.next.ensure((size_t)W_new * pf_stride * 4 + 64)) return fail(HQTICK_E_DEVICE, "hipMalloc prefilled counts");
        pfm = PfMove{pf.cur.as<uint32_t>(), pf_stride, pf.next.as<uint32_t>(), pf_stride, pf_stride};
    }
    std::vector<unsigned char> hb((size_t)W_new * 5 + 16, 0);  // [src row u32 W_new][flags of the new rows u8 W_new]: one copy
    if (W_new) memcpy(hb.data(), src.data(), (size_t)W_new * 4);
    for (uint32_t w = 0; w < W_new; w++) hb[(size_t)W_new * 4 + w] = src[w] >= W_old ? (add_flags ? add_flags[src[w] - W_old] : (uint8_t)HQ_WORKER_SN) : (uint8_t)0;
    HQ_HIP(hipMemcpyAsync(buf[B_BATCH].p, hb.data(), hb.size(), hipMemcpyHostToDevice, e.stream));
    HQ_HIP(repack_counts(counts.cur.as<uint32_t>(), stride, W_old, buf[B_BATCH].as<uint32_t>(), W_new, counts.next.as<uint32_t>(), stride, stride,
                         mn_rows(mn.cur, W_old, mn_live), mn_rows(mn.next, W_new, mn_live), buf[B_BATCH].as<uint8_t>() + (size_t)W_new * 4, e.stream, pfm));
    HQ_HIP(hipStreamSynchronize(e.stream));  // (pageable source)
    counts.swap(); mn.swap();
    if (pf_on) { pf.swap(); pf_dirty = true; }
    dirty_ = true;
    return 0;
}
// every entry of the lost workers leaves the ledger; (id, rq, priority) come back ascending by id (hqtick_cluster_last_requeued)
int Ledger::evict(const Env &e, uint32_t n, const uint32_t *worker_id) {
    std::vector<uint32_t> lost(worker_id, worker_id + n); std::sort(lost.begin(), lost.end());
    const uint64_t pf_now = pf_on ? pf_live : 0, cap_out = n_live + mn_live + pf_now + 1;
    if (!buf[B_SCRATCH].ensure((((size_t)n * 4 + 7) & ~(size_t)7) + cap_out * 22 + 16)) return fail(HQTICK_E_DEVICE, "hipMalloc ledger scratch");
    Pack pk{nullptr, buf[B_SCRATCH].as<unsigned char>()};  // [lost n u32][id u64][priority u64][rq u32][variant u8][running u8], cap_out each
    uint32_t *d_lost = pk.put<uint32_t>(nullptr, n); uint64_t *d_id = pk.put<uint64_t>(nullptr, cap_out, 8), *d_pr = pk.put<uint64_t>(nullptr, cap_out);
    uint32_t *d_rq = pk.put<uint32_t>(nullptr, cap_out); uint8_t *d_var = pk.put<uint8_t>(nullptr, cap_out), *d_run = pk.put<uint8_t>(nullptr, cap_out);
    HQ_HIP(hipMemcpyAsync(d_lost, lost.data(), (size_t)n * 4, hipMemcpyHostToDevice, e.stream));
    if (int rc = counted(e.stream, "hqasg::evict", [&](uint32_t *ctr) { return hqasg::evict(table(), n, d_lost, d_id, d_rq, d_pr, d_var, d_run, (uint32_t)cap_out, ctr, e.stream); })) return rc;
    const uint32_t k = c[C_OUT], k_mn = c[C_MN], k_pf = c[C_PF];
    if (k >= cap_out || (uint64_t)k_mn + k_pf > k || k_mn > mn_live || k_pf > pf_now || k - k_mn - k_pf > n_live) return fail(HQTICK_E_DEVICE, "assignment ledger: eviction count out of sync");
    if (k_mn) {  // a lost ROOT (reactor.rs:107-128): the task's other rows are free single-node workers again, before the rows are re-packed
        HQ_HIP(mn_reset_rows(table(), rows(e), mn_rows(mn.cur, e.W, mn_live), e.stream));
        flags_dirty = true;
    }
    std::vector<uint64_t> id(k), pr(k); std::vector<uint32_t> rq(k); std::vector<uint8_t> var(k ? cap_out + k : 0);  // [variant cap_out][running k]
    if (k) HQ_HIP(hipMemcpy(var.data(), d_var, (size_t)k * 2 + (cap_out - k), hipMemcpyDeviceToHost));  // (variant and running bytes lie one behind the other: one copy)
    if (k) {
        HQ_HIP(hipMemcpy(id.data(), d_id, (size_t)k * 8, hipMemcpyDeviceToHost));
        HQ_HIP(hipMemcpy(pr.data(), d_pr, (size_t)k * 8, hipMemcpyDeviceToHost));
        HQ_HIP(hipMemcpy(rq.data(), d_rq, (size_t)k * 4, hipMemcpyDeviceToHost));
    }
    std::vector<uint32_t> ord(k); for (uint32_t i = 0; i < k; i++) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return id[x] < id[y]; });
    for (uint32_t i : ord) {
        rq_task.push_back(id[i]); rq_prio.push_back(pr[i]); rq_rq.push_back(rq[i]);
        if (k_pf && var[i] == PF_VARIANT) rq_pf_task.push_back(id[i]);  // move_prefilled_task_to_ready: the subset the host takes out of its prefill sets
        else if (var[i] == MN_VARIANT || (var[i] != PF_VARIANT && var[cap_out + i])) rq_run_task.push_back(id[i]);  // running_tasks (reactor.rs:72-120): reported running, or multi-node
    }
    n_live -= k - k_mn - k_pf; mn_live -= k_mn; n_tomb += k; dirty_ = true;
    if (k_pf) { pf_live -= k_pf; pf_dirty = true; }
    return 0;
}

// evict() for hqtick_lose_workers: the same pass over the table, but a hit leaves (id, bucket) and everything that follows the count stays on the
// device -- hqgraph::sort_pairs by id, the gather of the buckets' columns (three dense columns for the merge, the same stores into pinned memory, kind and worker
// index), hqcancel::sort_rows by worker index with lose_core.h's offsets and CSR columns, the non-root members of the lost rows.  Nothing of it is read here.
int Ledger::lose_ensure(const Env &e, uint32_t n) {
    (void)e;
    const uint64_t cap_out = lose_bound() + 1;
    if (cap_out > 0x7FFFFFFFull) return fail(HQTICK_E_CAPACITY, "assignment ledger: more than 2^31 - 2 entries");
    const hqlose::DevLayout D = hqlose::dev_layout(cap_out, hqgraph::sort_capacity(cap_out), n);
    const hqlose::PinLayout P = hqlose::pin_layout(cap_out, n);
    if (!buf[B_LOSE].ensure(D.bytes) || !buf[B_CTR].ensure(64)) return fail(HQTICK_E_DEVICE, "hipMalloc ledger scratch");
    if (!h_lose.ensure(P.bytes) || !h_ctr.ensure(64)) return fail(HQTICK_E_DEVICE, "hipHostMalloc lost-worker lists");
    return 0;
}
int Ledger::lose(const Env &e, uint32_t n, const uint32_t *worker_id) {
    lose_out = LoseOut{};
    if (int rc = lose_ensure(e, n)) return rc;
    const uint64_t pf_now = pf_on ? pf_live : 0, cap_out = lose_bound() + 1;
    const hqlose::DevLayout D = hqlose::dev_layout(cap_out, hqgraph::sort_capacity(cap_out), n);
    const hqlose::PinLayout P = hqlose::pin_layout(cap_out, n);
    unsigned char *d = buf[B_LOSE].as<unsigned char>(), *h = h_lose.as<unsigned char>(), *hd = h_lose.dev<unsigned char>();
    auto dev = [&](size_t o) { return d + o; };
    // in: the lost ids sorted, the index of each in the caller's list, the caller's list -- one copy
    uint32_t *in = reinterpret_cast<uint32_t *>(h + P.in);
    std::vector<uint32_t> ord(n); for (uint32_t i = 0; i < n; i++) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return worker_id[x] < worker_id[y]; });
    for (uint32_t i = 0; i < n; i++) { in[i] = worker_id[ord[i]]; in[n + i] = ord[i]; in[2 * (size_t)n + i] = worker_id[i]; }
    uint64_t *h_mn_task = reinterpret_cast<uint64_t *>(h + P.m_task); uint32_t *h_mn_root = reinterpret_cast<uint32_t *>(h + P.m_root), *h_off = reinterpret_cast<uint32_t *>(h + P.off);
    std::fill_n(h_mn_task, (size_t)n, HT_EMPTY); std::fill_n(h_mn_root, (size_t)n, NONE); std::fill_n(h_off, (size_t)n + 1, 0u);
    HQ_HIP(hipMemcpyAsync(dev(D.lost), in, (size_t)n * 12, hipMemcpyHostToDevice, e.stream));
    LoseCols lc{};
    lc.n_lost = n; lc.lost = reinterpret_cast<uint32_t *>(dev(D.lost)); lc.lost_idx = reinterpret_cast<uint32_t *>(dev(D.lost_idx)); lc.call = reinterpret_cast<uint32_t *>(dev(D.call));
    lc.skey = reinterpret_cast<uint64_t *>(dev(D.skey)); lc.sval = reinterpret_cast<uint32_t *>(dev(D.sval));
    lc.id = reinterpret_cast<uint64_t *>(dev(D.id)); lc.prio = reinterpret_cast<uint64_t *>(dev(D.prio)); lc.rq = reinterpret_cast<uint32_t *>(dev(D.rq));
    lc.widx = reinterpret_cast<uint32_t *>(dev(D.widx)); lc.kind = dev(D.kind); lc.scratch = reinterpret_cast<uint32_t *>(dev(D.scratch));
    lc.o_id = reinterpret_cast<uint64_t *>(hd + P.f_id); lc.o_prio = reinterpret_cast<uint64_t *>(hd + P.f_prio); lc.o_rq = reinterpret_cast<uint32_t *>(hd + P.f_rq);
    lc.c_off = reinterpret_cast<uint32_t *>(hd + P.off); lc.c_id = reinterpret_cast<uint64_t *>(hd + P.c_id); lc.c_prio = reinterpret_cast<uint64_t *>(hd + P.c_prio);
    lc.c_rq = reinterpret_cast<uint32_t *>(hd + P.c_rq); lc.c_kind = hd + P.c_kind;
    lc.mn_task = reinterpret_cast<uint64_t *>(hd + P.m_task); lc.mn_root = reinterpret_cast<uint32_t *>(hd + P.m_root);
    if (int rc = counted(e.stream, "hqasg::lose_evict", [&](uint32_t *ctr) { return lose_evict(table(), rows(e), mn_rows(mn.cur, e.W, mn_live), lc, (uint32_t)cap_out, ctr, e.stream); })) return rc;
    const uint32_t k = c[C_OUT], k_mn = c[C_MN], k_pf = c[C_PF];
    if (k >= cap_out || (uint64_t)k_mn + k_pf > k || k_mn > mn_live || k_pf > pf_now || k - k_mn - k_pf > n_live) return fail(HQTICK_E_DEVICE, "assignment ledger: eviction count out of sync");
    n_live -= k - k_mn - k_pf; mn_live -= k_mn; n_tomb += k; dirty_ = true;  // (the entries are gone whatever happens below)
    if (k_pf) { pf_live -= k_pf; pf_dirty = true; }
    if (k) {
        HQ_HIP(hqgraph::sort_pairs(lc.skey, lc.sval, k, e.stream));
        HQ_HIP(lose_gather(table(), lc, k, e.stream));
    }
    HQ_HIP(lose_group(lc, k, e.stream));
    if (k_mn) {  // a lost ROOT (reactor.rs:107-128): the task's other rows are free single-node workers again, before the rows are re-packed
        HQ_HIP(mn_reset_rows(table(), rows(e), mn_rows(mn.cur, e.W, mn_live + k_mn), e.stream));
        flags_dirty = true;
    }
    lose_out = LoseOut{n, k, h_off, reinterpret_cast<uint64_t *>(h + P.c_id), reinterpret_cast<uint64_t *>(h + P.c_prio), reinterpret_cast<uint32_t *>(h + P.c_rq), h + P.c_kind,
                       reinterpret_cast<uint64_t *>(h + P.f_id), reinterpret_cast<uint64_t *>(h + P.f_prio), reinterpret_cast<uint32_t *>(h + P.f_rq), h_mn_task, h_mn_root, lc.id, lc.prio, lc.rq};
    return (int)k;
}

// the host mirror (free rows, counts) from the device tables: one synchronisation, two copies; then the assigned CSR of the host stages
int Ledger::sync_mirror(const Env &e) {
    const uint32_t W = e.W, R = e.R;
    if (int rc = sync_req(e)) return rc;
    if (dirty_) {
        e.free_->resize((size_t)W * R); h_counts.resize((size_t)W * stride);
        if (W && R) HQ_HIP(hipMemcpyAsync(e.free_->data(), e.cluster + (size_t)W * R * 8, (size_t)W * R * 8, hipMemcpyDeviceToHost, e.stream));
        if (W && stride) HQ_HIP(hipMemcpyAsync(h_counts.data(), counts.cur.p, (size_t)W * stride * 4, hipMemcpyDeviceToHost, e.stream));
        if (W && flags_dirty) {  // a ledger call moved SN bits (set_mn_task / reset_mn_task): the tick reads worker_flags from the mirror
            e.flags->resize(W);
            HQ_HIP(hipMemcpyAsync(e.flags->data(), mn_rows(mn.cur, W, 0).flags, W, hipMemcpyDeviceToHost, e.stream));
        }
        if (pf_on && pf_dirty) {  // a ledger call changed the prefilled counts: what the tick's has_pf is filled from
            h_pf.resize((size_t)W * pf_stride);
            if (W) HQ_HIP(hipMemcpyAsync(h_pf.data(), pf.cur.p, (size_t)W * pf_stride * 4, hipMemcpyDeviceToHost, e.stream));
        }
        HQ_HIP(hipStreamSynchronize(e.stream));
        dirty_ = false; agg_dirty = true; flags_dirty = false; pf_dirty = false;
    }
    if (!agg_dirty) return 0;
    // O(W x variant slots), not O(running tasks): the count table is what GapCache and Worker::is_free need
    const uint32_t Q = (uint32_t)rq_off.size() - 1;
    agg_off.assign((size_t)W + 1, 0); agg_rq.clear(); agg_cnt.clear(); agg_var.clear();
    for (uint32_t w = 0; w < W; w++) {
        const uint32_t *row = h_counts.data() + (size_t)w * stride;
        for (uint32_t q = 0; q < Q; q++)
            for (uint32_t v = rq_off[q]; v < rq_off[q + 1]; v++)
                if (row[v]) { agg_rq.push_back(q); agg_var.push_back((uint8_t)(v - rq_off[q])); agg_cnt.push_back(row[v]); }
        agg_off[w + 1] = (uint32_t)agg_rq.size();
    }
    agg_dirty = false;
    return 0;
}

// ---------------------------------------------------------------------------------------------- the C ABI's operations
int Ledger::enable(const Env &e, uint32_t n, const uint64_t *id, const uint32_t *wid, const uint32_t *rq, const uint8_t *var, const uint64_t *prio) {
    on = false; pending = false; cap = 0; n_live = 0; n_tomb = 0; last_unknown = 0; stride = 0; stage_n = 0; last_host_bytes = 0;
    clear_requeued();
    pf_on = false; pf_live = 0; pf_stride = 0; pf_dirty = false;  // (tracking is asked for again on the new ledger)
    if (int rc = reserve(e, n)) return rc;
    HQ_HIP(clear(table(), e.stream));
    req_dirty = true;
    if (int rc = sync_req(e)) return rc;
    const uint32_t W = e.W; if (!counts.cur.ensure((size_t)W * stride * 4 + 64)) return fail(HQTICK_E_DEVICE, "hipMalloc assignment counts");
    HQ_HIP(hipMemsetAsync(counts.cur.p, 0, (size_t)W * stride * 4 + 64, e.stream));
    // the multi-node columns: no row holds a task, the flags byte is the mirror's (a worker uploaded without its SN bit waits for hqtick_assigned_add_mn)
    mn_live = 0; flags_dirty = false; pmn_id.clear();
    if (!mn.cur.ensure((size_t)W * 10 + 64)) return fail(HQTICK_E_DEVICE, "hipMalloc assignment rows");
    HQ_HIP(hipMemsetAsync(mn.cur.p, 0xFF, (size_t)W * 8, e.stream));
    HQ_HIP(hipMemsetAsync(mn.cur.as<unsigned char>() + (size_t)W * 8, 0, (size_t)W * 2 + 64, e.stream));
    if (int rc = upload_flags(e)) return rc;
    if (int rc = upload_wids(e)) return rc;
    if (n) { if (int rc = insert_host(e, n, id, wid, rq, var, prio, 0, 0, nullptr)) return rc; }
    if (n && (c[C_BAD] || c[C_DUP])) return fail(HQTICK_E_INVALID, "hqtick_assigned_enable: an entry names an unknown worker, request or variant, or a task twice");
    on = true; dirty_ = true;
    return 0;
}
int Ledger::add(const Env &e, uint32_t n, const uint64_t *id, const uint32_t *wid, const uint32_t *rq, const uint8_t *var, const uint64_t *prio, int running) {
    last_unknown = 0; if (!n) return 0;
    if (int rc = insert_host(e, n, id, wid, rq, var, prio, 0, 1, nullptr, running)) return rc;
    last_unknown = (uint64_t)c[C_BAD] + c[C_DUP];
    return (int)c[C_OUT];
}
int Ledger::release(const Env &e, uint32_t n, const uint64_t *id) {
    last_unknown = 0; if (!n) return 0;
    if (int rc = sync_req(e)) return rc;
    const size_t WR = (size_t)e.W * e.R;
    if (!buf[B_SCRATCH].ensure((size_t)n * 12 + WR * 12 + 16)) return fail(HQTICK_E_DEVICE, "hipMalloc ledger scratch");
    Pack pk{nullptr, buf[B_SCRATCH].as<unsigned char>()};  // [ids n u64][delta W*R u64][pos n u32][last_all W*R u32]
    uint64_t *d_id = pk.put<uint64_t>(nullptr, n), *d_delta = pk.put<uint64_t>(nullptr, WR); uint32_t *d_pos = pk.put<uint32_t>(nullptr, n), *d_la = pk.put<uint32_t>(nullptr, WR);
    HQ_HIP(hipMemsetAsync(d_delta, 0, WR * 8, e.stream));
    HQ_HIP(hipMemsetAsync(d_la, 0, WR * 4, e.stream));
    Pack in;
    if (int rc = stage_in((size_t)n * 8, &in)) return rc;
    in.put(id, n);
    HQ_HIP(hipMemcpyAsync(d_id, in.h, (size_t)n * 8, hipMemcpyHostToDevice, e.stream));
    if (int rc = counted(e.stream, "hqasg::release", [&](uint32_t *ctr) { return hqasg::release(table(), req(), rows(e), mn_rows(mn.cur, e.W, mn_live), n, d_id, d_pos, d_la, d_delta, ctr, e.stream); })) return rc;
    const uint32_t done = c[C_DONE], done_mn = std::min(c[C_MN], done);  // (a multi-node task counts once, its rows were reset by the row pass)
    if (done_mn) flags_dirty = true;
    n_live -= done - done_mn; mn_live -= std::min<uint64_t>(done_mn, mn_live); n_tomb += done; last_unknown = (uint64_t)c[C_UNKNOWN] + c[C_DUP]; dirty_ = true;  // (the others of the batch are released either way)
    if (c[C_BAD]) return fail(HQTICK_E_DEVICE, "assignment ledger: an entry names a worker that is not in the resident set");
    return (int)done;
}
// on_cancel_tasks on the ledger (hqtick_cancel_tasks): the release's four passes in their cancel mode, then the grouping of the routes (cancel.h), all behind one
// set of counters and ONE synchronisation.  The ids are read where the caller staged them on the device; the lists and routes are written into pinned memory.
int Ledger::cancel(const Env &e, uint32_t n, const uint64_t *d_id, uint32_t n_retr, const uint64_t *retr_id, const uint32_t *retr_wid, const uint32_t **retr_hit) {
    last_unknown = 0; cancel_out = CancelOut{}; if (retr_hit) *retr_hit = nullptr;
    if (!n) return 0;
    if (int rc = sync_req(e)) return rc;
    const uint32_t W = e.W; const size_t WR = (size_t)W * e.R, nr = n_retr;
    const hqcancel::Scratch sc = hqcancel::scratch_of(n, W);
    if (!buf[B_SCRATCH].ensure((size_t)n * 4 + WR * 12 + 16) || !buf[B_CANCEL].ensure(nr * 16 + sc.total * 4 + (size_t)n * 5 + 64)) return fail(HQTICK_E_DEVICE, "hipMalloc ledger scratch");
    if (!h_cancel.ensure(nr * 16 + (size_t)n * 13 + (size_t)W * 8 + 64)) return fail(HQTICK_E_DEVICE, "hipHostMalloc cancel lists");
    Pack pk{nullptr, buf[B_SCRATCH].as<unsigned char>()};  // [delta W*R u64][pos n u32][last_all W*R u32]
    uint64_t *d_delta = pk.put<uint64_t>(nullptr, WR); uint32_t *d_pos = pk.put<uint32_t>(nullptr, n), *d_la = pk.put<uint32_t>(nullptr, WR);
    Pack dk{nullptr, buf[B_CANCEL].as<unsigned char>()};   // [override ids u64][override workers u32] (one copy) [sort scratch u32][route n u32][hit u32][kind n u8]
    uint64_t *d_rid = dk.put<uint64_t>(nullptr, nr); uint32_t *d_rwid = dk.put<uint32_t>(nullptr, nr), *d_sort = dk.put<uint32_t>(nullptr, sc.total, 8);
    uint32_t *d_route = dk.put<uint32_t>(nullptr, n), *d_hit = dk.put<uint32_t>(nullptr, nr); uint8_t *d_kind = dk.put<uint8_t>(nullptr, n);
    Pack hk{h_cancel.as<unsigned char>(), h_cancel.dev<unsigned char>()};  // in: the overrides; out: [ids n u64][hdr 2][workers W][offsets W + 1][route worker n][hit] u32 [kind n u8]
    const uint64_t *h_rid = hk.put(retr_id, nr); hk.put(retr_wid, nr);
    uint64_t *o_id = hk.put<uint64_t>(nullptr, n, 8); uint32_t *o_hdr = hk.put<uint32_t>(nullptr, 2), *o_wid = hk.put<uint32_t>(nullptr, W), *o_off = hk.put<uint32_t>(nullptr, (size_t)W + 1);
    uint32_t *o_rwid = hk.put<uint32_t>(nullptr, n), *o_hit = hk.put<uint32_t>(nullptr, nr); uint8_t *o_kind = hk.put<uint8_t>(nullptr, n);
    hk.host(o_hdr)[0] = hk.host(o_hdr)[1] = 0; hk.host(o_off)[0] = 0;
    HQ_HIP(hipMemsetAsync(d_delta, 0, WR * 8, e.stream));
    HQ_HIP(hipMemsetAsync(d_la, 0, WR * 4, e.stream));
    if (W) HQ_HIP(hipMemsetAsync(d_sort + sc.start, 0xFF, (size_t)W * 4, e.stream));
    if (nr) {
        HQ_HIP(hipMemsetAsync(d_hit, 0xFF, nr * 4, e.stream));
        HQ_HIP(hipMemcpyAsync(d_rid, hk.host(h_rid), nr * 12, hipMemcpyHostToDevice, e.stream));
    }
    const CancelCols cc{d_route, d_kind, d_rid, d_rwid, d_hit, n_retr};
    const hqcancel::Group g{n, W, d_route, d_kind, d_id, buf[B_WIDS].as<uint32_t>(), d_sort, o_id, o_wid, o_off, o_hdr, o_rwid, o_kind, HQ_NO_WORKER};
    if (int rc = counted(e.stream, "hqasg::cancel", [&](uint32_t *ctr) {
            hipError_t r = hqasg::cancel(table(), req(), rows(e), mn_rows(mn.cur, W, mn_live), n, d_id, d_pos, d_la, d_delta, cc, ctr, e.stream);
            if (r == hipSuccess) r = hqcancel::group(g, e.stream);
            if (r == hipSuccess && nr) r = hipMemcpyAsync(hk.host(o_hit), d_hit, nr * 4, hipMemcpyDeviceToHost, e.stream);
            return r; })) return rc;
    const uint32_t done = c[C_DONE], done_mn = std::min(c[C_MN], done), done_pf = (uint32_t)std::min<uint64_t>(std::min(c[C_PF], done - done_mn), pf_live);
    if (done_mn) flags_dirty = true;
    if (done_pf) { pf_live -= done_pf; pf_dirty = true; }
    n_live -= done - done_mn - done_pf; mn_live -= std::min<uint64_t>(done_mn, mn_live); n_tomb += done; last_unknown = (uint64_t)c[C_UNKNOWN] + c[C_DUP]; dirty_ = true;
    if (c[C_BAD]) return fail(HQTICK_E_DEVICE, "assignment ledger: an entry names a worker that is not in the resident set");
    const uint32_t *hdr = hk.host(o_hdr);
    if (hdr[0] > W || hdr[1] > n) return fail(HQTICK_E_DEVICE, "assignment ledger: the cancel lists are out of range");
    cancel_out = CancelOut{n, hdr[0], hdr[1], hk.host(o_wid), hk.host(o_off), hk.host(o_id), hk.host(o_rwid), hk.host(o_kind)};
    if (retr_hit) *retr_hit = hk.host(o_hit);
    return (int)hdr[1];
}
// task_finished on the ledger (hqtick_finish_tasks): the release's four passes in their finish mode behind one set of counters and ONE
// synchronisation.  Ids and reporters are read where the caller staged them on the device; the kinds and the override hits come back into pinned memory behind
// the passes, and the kinds stay on the device for the graph's skip input.
// task_failed (hqtick_fail_tasks) is the same step in the passes' fail mode with pinned memory of its own (a fail leaves the last finish's kinds
// alone): prefilled entries leave too, and the graph step behind it may still refuse _WAITING positions, so fail_out's kinds are final only after that.
int Ledger::finish(const Env &e, uint32_t n, const uint64_t *d_id, const uint32_t *d_reporter, uint32_t n_retr, const uint64_t *retr_id, const uint32_t *retr_wid, const uint32_t **retr_hit) {
    return reported(e, false, n, d_id, d_reporter, n_retr, retr_id, retr_wid, retr_hit);
}
int Ledger::fail_tasks(const Env &e, uint32_t n, const uint64_t *d_id, const uint32_t *d_reporter, uint32_t n_retr, const uint64_t *retr_id, const uint32_t *retr_wid, const uint32_t **retr_hit) {
    return reported(e, true, n, d_id, d_reporter, n_retr, retr_id, retr_wid, retr_hit);
}
int Ledger::reported(const Env &e, bool failing, uint32_t n, const uint64_t *d_id, const uint32_t *d_reporter, uint32_t n_retr, const uint64_t *retr_id, const uint32_t *retr_wid, const uint32_t **retr_hit) {
    FinishOut &out = failing ? fail_out : finish_out;
    hqbuf::PinBuf &h_out = failing ? h_fail : h_finish;
    last_unknown = 0; out = FinishOut{}; if (retr_hit) *retr_hit = nullptr;
    if (!n) return 0;
    if (int rc = sync_req(e)) return rc;
    const size_t WR = (size_t)e.W * e.R, nr = n_retr;
    if (!buf[B_SCRATCH].ensure((size_t)n * 4 + WR * 12 + 16) || !buf[B_CANCEL].ensure(nr * 16 + (size_t)n + 64)) return fail(HQTICK_E_DEVICE, "hipMalloc ledger scratch");
    if (!h_out.ensure(nr * 16 + (size_t)n + 64)) return fail(HQTICK_E_DEVICE, "hipHostMalloc finish kinds");
    Pack pk{nullptr, buf[B_SCRATCH].as<unsigned char>()};  // [delta W*R u64][pos n u32][last_all W*R u32]
    uint64_t *d_delta = pk.put<uint64_t>(nullptr, WR); uint32_t *d_pos = pk.put<uint32_t>(nullptr, n), *d_la = pk.put<uint32_t>(nullptr, WR);
    Pack dk{nullptr, buf[B_CANCEL].as<unsigned char>()};   // [override ids u64][override workers u32] (one copy) [hit u32][kind n u8]
    uint64_t *d_rid = dk.put<uint64_t>(nullptr, nr); uint32_t *d_rwid = dk.put<uint32_t>(nullptr, nr), *d_hit = dk.put<uint32_t>(nullptr, nr); uint8_t *d_kind = dk.put<uint8_t>(nullptr, n);
    Pack hk{h_out.as<unsigned char>(), h_out.dev<unsigned char>()};  // in: the overrides; out: [hit u32][kind n u8]
    const uint64_t *h_rid = hk.put(retr_id, nr); hk.put(retr_wid, nr);
    uint32_t *o_hit = hk.put<uint32_t>(nullptr, nr); uint8_t *o_kind = hk.put<uint8_t>(nullptr, n);
    HQ_HIP(hipMemsetAsync(d_delta, 0, WR * 8, e.stream));
    HQ_HIP(hipMemsetAsync(d_la, 0, WR * 4, e.stream));
    if (nr) {
        HQ_HIP(hipMemsetAsync(d_hit, 0xFF, nr * 4, e.stream));
        HQ_HIP(hipMemcpyAsync(d_rid, hk.host(h_rid), nr * 12, hipMemcpyHostToDevice, e.stream));
    }
    const CancelCols cc{nullptr, d_kind, d_rid, d_rwid, d_hit, n_retr, d_reporter};
    if (int rc = counted(e.stream, failing ? "hqasg::fail" : "hqasg::finish", [&](uint32_t *ctr) {
            hipError_t r = (failing ? hqasg::fail : hqasg::finish)(table(), req(), rows(e), mn_rows(mn.cur, e.W, mn_live), n, d_id, d_pos, d_la, d_delta, cc, ctr, e.stream);
            if (r == hipSuccess) r = hipMemcpyAsync(hk.host(o_kind), d_kind, n, hipMemcpyDeviceToHost, e.stream);
            if (r == hipSuccess && nr) r = hipMemcpyAsync(hk.host(o_hit), d_hit, nr * 4, hipMemcpyDeviceToHost, e.stream);
            return r; })) return rc;
    const uint32_t done = c[C_DONE], done_mn = std::min(c[C_MN], done), accepted = std::min(c[C_OUT], n);
    const uint32_t done_pf = failing ? (uint32_t)std::min<uint64_t>(std::min(c[C_PF], done - done_mn), pf_live) : 0u;
    if (done_mn) flags_dirty = true;
    if (done_pf) { pf_live -= done_pf; pf_dirty = true; }
    n_live -= done - done_mn - done_pf; mn_live -= std::min<uint64_t>(done_mn, mn_live); n_tomb += done; last_unknown = n - accepted; dirty_ = true;
    if (c[C_BAD]) return fail(HQTICK_E_DEVICE, "assignment ledger: an entry names a worker that is not in the resident set");
    out = FinishOut{n, accepted, hk.host(o_kind), d_kind, o_kind};
    if (retr_hit) *retr_hit = hk.host(o_hit);
    return (int)accepted;
}
// task_reject on the ledger (hqtick_reject_tasks): reported()'s step in the passes' reject mode with the requeue's compaction behind it, still one
// set of counters and one synchronisation.  The requeued columns stay in buf[B_REJECT] for the ready set's merge and are written into pinned memory by the same
// kernel; nothing of them is read on the host before the merge.
namespace {
struct RejectSizes { size_t scratch, cancel, reject, pinned; };
RejectSizes reject_sizes(uint32_t n, uint32_t n_retr, size_t WR) {
    const size_t nr = n_retr, slices = (((size_t)n + 255) / 256 + 15) & ~(size_t)15;
    return RejectSizes{(size_t)n * 4 + WR * 12 + 16, nr * 16 + (size_t)n + 64, (size_t)n * 37 + slices * 4 + 128, nr * 16 + (size_t)n * 25 + 128};
}
}  // namespace
int Ledger::reject_ensure(const Env &e, uint32_t n, uint32_t n_retr) {
    const RejectSizes z = reject_sizes(n, n_retr, (size_t)e.W * e.R);
    if (!buf[B_SCRATCH].ensure(z.scratch) || !buf[B_CANCEL].ensure(z.cancel) || !buf[B_REJECT].ensure(z.reject)) return fail(HQTICK_E_DEVICE, "hipMalloc ledger scratch");
    if (!h_reject.ensure(z.pinned) || !h_ctr.ensure(64) || !buf[B_CTR].ensure(64)) return fail(HQTICK_E_DEVICE, "hipHostMalloc reject lists");
    return 0;
}
int Ledger::reject(const Env &e, uint32_t n, const uint64_t *d_id, const uint32_t *d_reporter, const uint8_t *d_variant, const uint32_t *d_rq, const uint32_t *d_perm, uint32_t n_retr,
                   const uint64_t *retr_id, const uint32_t *retr_wid, const uint32_t **retr_hit) {
    last_unknown = 0; reject_out = RejectOut{}; if (retr_hit) *retr_hit = nullptr;
    if (!n) return 0;
    if (int rc = reject_ensure(e, n, n_retr)) return rc;
    if (int rc = sync_req(e)) return rc;
    const size_t WR = (size_t)e.W * e.R, nr = n_retr, slices = (((size_t)n + 255) / 256 + 15) & ~(size_t)15;
    Pack pk{nullptr, buf[B_SCRATCH].as<unsigned char>()};  // [delta W*R u64][pos n u32][last_all W*R u32]
    uint64_t *d_delta = pk.put<uint64_t>(nullptr, WR); uint32_t *d_pos = pk.put<uint32_t>(nullptr, n), *d_la = pk.put<uint32_t>(nullptr, WR);
    Pack dk{nullptr, buf[B_CANCEL].as<unsigned char>()};   // [override ids u64][override workers u32] (one copy) [hit u32][kind n u8]
    uint64_t *d_rid = dk.put<uint64_t>(nullptr, nr); uint32_t *d_rwid = dk.put<uint32_t>(nullptr, nr), *d_hit = dk.put<uint32_t>(nullptr, nr); uint8_t *d_kind = dk.put<uint8_t>(nullptr, n);
    Pack rk{nullptr, buf[B_REJECT].as<unsigned char>()};   // [record priority n u64][out id n u64][out priority n u64][blocks n u32][record rq n u32][out rq n u32][slices u32][flag n u8]
    uint64_t *d_rprio = rk.put<uint64_t>(nullptr, n, 8), *d_oid = rk.put<uint64_t>(nullptr, n), *d_oprio = rk.put<uint64_t>(nullptr, n);
    uint32_t *d_blk = rk.put<uint32_t>(nullptr, n), *d_rrq = rk.put<uint32_t>(nullptr, n), *d_orq = rk.put<uint32_t>(nullptr, n), *d_slices = rk.put<uint32_t>(nullptr, slices, 16);  // (the scan reads the table in 16-byte groups)
    uint8_t *d_flag = rk.put<uint8_t>(nullptr, n);
    Pack hk{h_reject.as<unsigned char>(), h_reject.dev<unsigned char>()};  // in: the overrides; out: [requeued id n u64][priority n u64][rq n u32][blocks n u32][hit u32][total u32][kind n u8]
    const uint64_t *h_rid = hk.put(retr_id, nr); hk.put(retr_wid, nr);
    uint64_t *o_id = hk.put<uint64_t>(nullptr, n, 8), *o_prio = hk.put<uint64_t>(nullptr, n);
    uint32_t *o_rq = hk.put<uint32_t>(nullptr, n), *o_blk = hk.put<uint32_t>(nullptr, n), *o_hit = hk.put<uint32_t>(nullptr, nr), *o_total = hk.put<uint32_t>(nullptr, 1);
    uint8_t *o_kind = hk.put<uint8_t>(nullptr, n);
    *hk.host(o_total) = 0;
    HQ_HIP(hipMemsetAsync(d_delta, 0, WR * 8, e.stream));
    HQ_HIP(hipMemsetAsync(d_la, 0, WR * 4, e.stream));
    if (nr) {
        HQ_HIP(hipMemsetAsync(d_hit, 0xFF, nr * 4, e.stream));
        HQ_HIP(hipMemcpyAsync(d_rid, hk.host(h_rid), nr * 12, hipMemcpyHostToDevice, e.stream));
    }
    const CancelCols cc{nullptr, d_kind, d_rid, d_rwid, d_hit, n_retr, d_reporter};
    const RejectCols rj{d_variant, d_rq, d_perm, d_blk, d_flag, d_rprio, d_rrq, d_slices, o_total, d_oid, d_oprio, d_orq, o_id, o_prio, o_rq};
    if (int rc = counted(e.stream, "hqasg::reject", [&](uint32_t *ctr) {
            hipError_t r = hqasg::reject(table(), req(), rows(e), mn_rows(mn.cur, e.W, mn_live), n, d_id, d_pos, d_la, d_delta, cc, rj, ctr, e.stream);
            if (r == hipSuccess) r = hipMemcpyAsync(hk.host(o_kind), d_kind, n, hipMemcpyDeviceToHost, e.stream);
            if (r == hipSuccess) r = hipMemcpyAsync(hk.host(o_blk), d_blk, (size_t)n * 4, hipMemcpyDeviceToHost, e.stream);
            if (r == hipSuccess && nr) r = hipMemcpyAsync(hk.host(o_hit), d_hit, nr * 4, hipMemcpyDeviceToHost, e.stream);
            return r; })) return rc;
    const uint32_t done = c[C_DONE], accepted = std::min(c[C_OUT], n), done_pf = (uint32_t)std::min<uint64_t>(std::min(c[C_PF], done), pf_live);
    if (done_pf) { pf_live -= done_pf; pf_dirty = true; }
    n_live -= done - done_pf; n_tomb += done; last_unknown = n - accepted; dirty_ = true;
    if (c[C_BAD]) return fail(HQTICK_E_DEVICE, "assignment ledger: an entry names a worker that is not in the resident set");
    if (*hk.host(o_total) != done) return fail(HQTICK_E_DEVICE, "assignment ledger: the requeued columns are out of sync with the entries that left");
    reject_out = RejectOut{n, accepted, done, hk.host(o_kind), hk.host(o_blk), hk.host(o_id), hk.host(o_prio), hk.host(o_rq), d_oid, d_oprio, d_orq};
    if (retr_hit) *retr_hit = hk.host(o_hit);
    return (int)accepted;
}
// task_running on the ledger (hqtick_start_tasks).  The claim pass runs once over the whole batch: a kind follows from the tables before the batch
// and the claims, and the caller's own positions between the segments (ids of the Retracting table, masked here) touch no entry a device position names.  What they
// do touch is the free rows, with saturating arithmetic, so the apply pass runs segment by segment in batch order around them.
int Ledger::start_begin(const Env &e, uint32_t n, const uint64_t *d_id, const uint32_t *d_reporter, const uint8_t *d_variant, const uint8_t *mask, uint32_t n_host) {
    last_unknown = 0; start_out = StartOut{}; start_n = 0; std::fill_n(start_acc, (size_t)C_N, 0u);
    if (!n) return 0;
    if (int rc = sync_req(e)) return rc;
    if (n_host) { if (int rc = reserve(e, 2 * (uint64_t)n_host)) return rc; }  // (each of them leaves a tombstone and enters an entry)
    if (!buf[B_START].ensure((size_t)n * 6 + 16) || !h_start.ensure((size_t)n * 2 + 16)) return fail(HQTICK_E_DEVICE, "hipMalloc start scratch");
    Pack dk{nullptr, buf[B_START].as<unsigned char>()};  // [pos n u32][kind n u8][mask n u8]
    uint32_t *d_pos = dk.put<uint32_t>(nullptr, n); uint8_t *d_kind = dk.put<uint8_t>(nullptr, n), *d_mask = dk.put<uint8_t>(nullptr, n);
    if (mask) {
        memcpy(h_start.as<unsigned char>() + n, mask, n);
        HQ_HIP(hipMemcpyAsync(d_mask, h_start.as<unsigned char>() + n, n, hipMemcpyHostToDevice, e.stream));
    }
    start_c = StartCols{d_id, d_reporter, d_variant, mask ? d_mask : nullptr, d_pos, d_kind}; start_n = n;
    HQ_HIP(start_claim(table(), req(), rows(e), start_c, 0, n, e.stream));
    return 0;
}
int Ledger::start_segment(const Env &e, uint32_t lo, uint32_t hi, bool last) {
    if (!start_n || (lo >= hi && !last)) return 0;
    const uint32_t n = start_n;
    if (int rc = counted(e.stream, "hqasg::start", [&](uint32_t *ctr) {
            hipError_t r = start_apply(table(), req(), rows(e), start_c, lo, hi, ctr, e.stream);
            if (r == hipSuccess && last) r = hipMemcpyAsync(h_start.p, start_c.kind, n, hipMemcpyDeviceToHost, e.stream);
            return r; })) return rc;
    for (uint32_t k = 0; k < C_N; k++) start_acc[k] += c[k];
    if (const uint32_t pf_now = (uint32_t)std::min<uint64_t>(c[C_PF], pf_live)) { pf_live -= pf_now; n_live += pf_now; pf_dirty = true; }  // started prefills are assigned entries now
    if (c[C_OUT]) dirty_ = true;
    if (last) { start_out = StartOut{n, std::min(start_acc[C_OUT], n), h_start.as<uint8_t>()}; start_n = 0; }
    return 0;
}
void Ledger::start_abort(const Env &e, uint32_t lo) {
    if (start_n && cap && start_unclaim(table(), start_c, lo, start_n, e.stream) == hipSuccess) hipStreamSynchronize(e.stream);
    start_n = 0; start_out = StartOut{};
}
int Ledger::running(const Env &e, uint32_t n, const uint64_t *task_id, uint8_t *run) {
    Pack pk;
    if (int rc = stage_in((size_t)n * 9, &pk)) return rc;
    const uint64_t *d_id = pk.put(task_id, n); uint8_t *d_r = pk.put<uint8_t>(nullptr, n);
    HQ_HIP(hqasg::running(table(), n, d_id, d_r, e.stream));
    HQ_HIP(hipStreamSynchronize(e.stream));
    memcpy(run, pk.host(d_r), n);
    int found = 0; for (uint32_t i = 0; i < n; i++) found += run[i] != 0xFF;
    return found;
}
int Ledger::add_mn(const Env &e, uint32_t n, const uint64_t *task_id, const uint32_t *rq, const uint64_t *priority, const uint32_t *worker_off, const uint32_t *worker_id) {
    last_unknown = 0; if (!n) return 0;
    if (worker_off[0] != 0) return fail(HQTICK_E_INVALID, "hqtick_assigned_add_mn: worker_off[0] must be 0");
    for (uint32_t i = 0; i < n; i++) if (worker_off[i + 1] < worker_off[i]) return fail(HQTICK_E_INVALID, "hqtick_assigned_add_mn: worker_off must not descend");
    if (worker_off[n] && !worker_id) return fail(HQTICK_E_INVALID, "hqtick_assigned_add_mn: null array");
    // a task whose request is not a multi-node one (n_nodes == 0, or unknown) never reaches the device
    std::vector<uint64_t> id, pr; std::vector<uint32_t> q, off{0}, wid;
    uint64_t skipped = 0;
    for (uint32_t i = 0; i < n; i++) {
        const bool mn_rq = (size_t)rq[i] + 1 < rq_off.size() && rq_off[rq[i]] < rq_off[rq[i] + 1] && rq_off[rq[i]] < var_nodes.size() && var_nodes[rq_off[rq[i]]] > 0;
        if (!mn_rq || worker_off[i] == worker_off[i + 1]) { skipped++; continue; }
        id.push_back(task_id[i]); pr.push_back(priority[i]); q.push_back(rq[i]);
        wid.insert(wid.end(), worker_id + worker_off[i], worker_id + worker_off[i + 1]); off.push_back((uint32_t)wid.size());
    }
    last_unknown = skipped;
    if (id.empty()) return 0;
    if (int rc = mn_enter(e, (uint32_t)id.size(), id.data(), q.data(), pr.data(), off.data(), wid.data(), 1)) return rc;
    last_unknown = skipped + c[C_BAD] + c[C_DUP];
    return (int)c[C_OUT];
}
int Ledger::mn_workers(const Env &e, uint64_t task_id, uint32_t *n, const uint32_t **worker_id) {
    mnw_out.clear();
    const uint32_t W = e.W;
    if (mn_live && W && task_id < HT_TOMB) {  // an accessor for tests and restore: the two columns come back, 9 B per row
        HQ_HIP(hipSetDevice(e.device));
        mnw_cols.resize((size_t)W * 9);
        HQ_HIP(hipMemcpyAsync(mnw_cols.data(), mn.cur.p, (size_t)W * 9, hipMemcpyDeviceToHost, e.stream));
        HQ_HIP(hipStreamSynchronize(e.stream));
        const unsigned char *root = mnw_cols.data() + (size_t)W * 8;
        for (int pass = 0; pass < 2; pass++)  // the root first, the others in ascending id (= row) order
            for (uint32_t w = 0; w < W; w++) {
                uint64_t t; memcpy(&t, mnw_cols.data() + (size_t)w * 8, 8);
                if (t == task_id && (root[w] != 0) == (pass == 0)) mnw_out.push_back((*e.id)[w]);
            }
    }
    if (n) *n = (uint32_t)mnw_out.size();  if (worker_id) *worker_id = mnw_out.data();
    return 0;
}
int Ledger::lookup(const Env &e, uint32_t n, const uint64_t *task_id, uint32_t *worker_id, uint8_t *variant) {
    Pack pk;
    if (int rc = stage_in((size_t)n * 13, &pk)) return rc;
    const uint64_t *d_id = pk.put(task_id, n); uint32_t *d_w = pk.put<uint32_t>(nullptr, n); uint8_t *d_v = pk.put<uint8_t>(nullptr, n);
    HQ_HIP(hqasg::lookup(table(), n, d_id, d_w, d_v, e.stream));
    HQ_HIP(hipStreamSynchronize(e.stream));
    memcpy(worker_id, pk.host(d_w), (size_t)n * 4); memcpy(variant, pk.host(d_v), n);
    int found = 0; for (uint32_t i = 0; i < n; i++) found += worker_id[i] != HQ_NO_WORKER;
    return found;
}

// ---- prefilled tasks (SingleNodeTaskAssignment::prefilled_tasks): one batch of ids (+ optional columns) staged in pinned memory and read in place
int Ledger::track_prefilled(const Env &e, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id, const uint32_t *rq, const uint64_t *priority) {
    if (max_variants() >= PF_VARIANT) return fail(HQTICK_E_UNSUPPORTED, "hqtick_assigned_track_prefilled: a request has 254 or more variants");
    last_unknown = 0; const uint32_t W = e.W;
    if (pf_on && pf_live) {  // a second call replaces the prefilled entries
        if (int rc = counted(e.stream, "hqasg::pf_drop_all", [&](uint32_t *ctr) { return pf_drop_all(table(), ctr, e.stream); })) return rc;
        n_tomb += c[C_DONE]; pf_live = 0;
    }
    pf_on = false;  // (until the table below stands: sync_req must not widen a table that is being replaced)
    if (int rc = reserve(e, n)) return rc;
    if (int rc = sync_req(e)) return rc;
    const uint32_t ns = row_stride(rq_off.size() - 1);
    if (!pf.cur.ensure((size_t)W * ns * 4 + 64)) return fail(HQTICK_E_DEVICE, "hipMalloc prefilled counts");
    HQ_HIP(hipMemsetAsync(pf.cur.p, 0, (size_t)W * ns * 4 + 64, e.stream));
    pf_stride = ns; pf_on = true; pf_live = 0; pf_dirty = true; dirty_ = true;
    if (!n) { HQ_HIP(hipStreamSynchronize(e.stream)); return 0; }
    Pack pk;
    if (int rc = stage_in((size_t)n * 24, &pk)) return rc;
    const uint64_t *d_id = pk.put(task_id, n), *d_pr = pk.put(priority, n); const uint32_t *d_w = pk.put(worker_id, n), *d_q = pk.put(rq, n);
    if (int rc = counted(e.stream, "hqasg::pf_seed", [&](uint32_t *ctr) { return pf_seed(table(), req(), rows(e), mn_rows(mn.cur, W, mn_live), n, d_id, d_w, d_q, d_pr, ctr, e.stream); })) return rc;
    if (c[C_FULL]) return fail(HQTICK_E_DEVICE, "assignment ledger: table full");
    pf_live = c[C_PF]; last_unknown = (uint64_t)c[C_BAD] + c[C_DUP];
    return (int)c[C_PF];
}

// task_from_prefilled_to_started (var: the variants the tasks start with) or remove_prefill_task (var == nullptr) for a batch of ids
int Ledger::pf_leave(const Env &e, uint32_t n, const uint64_t *task_id, const uint8_t *var) {
    last_unknown = 0; if (!n) return 0;
    if (var) { if (int rc = sync_req(e)) return rc; }
    Pack pk;
    if (int rc = stage_in((size_t)n * (var ? 9 : 8), &pk)) return rc;
    const uint64_t *d_id = pk.put(task_id, n); const uint8_t *d_v = pk.put(var, n);
    if (int rc = counted(e.stream, var ? "hqasg::pf_start" : "hqasg::pf_remove", [&](uint32_t *ctr) {
            return var ? pf_start(table(), req(), rows(e), n, d_id, d_v, ctr, e.stream) : pf_remove(table(), rows(e), n, d_id, ctr, e.stream); })) return rc;
    const uint32_t done = (uint32_t)std::min<uint64_t>(c[C_DONE], pf_live);
    pf_live -= done; (var ? n_live : n_tomb) += done; last_unknown = var ? (uint64_t)c[C_UNKNOWN] + c[C_BAD] : c[C_UNKNOWN];  // (started: an assigned entry; removed: a tombstone)
    if (done) { dirty_ = true; pf_dirty = true; }
    return (int)done;
}

}  // namespace hqasg

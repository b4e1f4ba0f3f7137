// hqready::ReadySet (ready.h): the resident ready set's columns, deltas and selection state.
#include "ready.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "kernels.h"

namespace hqready {

#define HQ_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(HQTICK_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
// The launch carries e.done as its stop event (hqk::time_next_launch: the dispatch's own completion signal, seen 2.8 us after the kernel is done where
// hipStreamSynchronize returns after 5.6 us).  `launched` = the wrapper really launched (it consumed the pending timer) and waiting on the kernel is not switched off.
#define HQ_HIP_LAST(call, launched) do { hipError_t e_ = (call); (launched) = hqk::take_launch_timer().stop == nullptr && e.wait_on_kernel; if (e_ != hipSuccess) return fail(HQTICK_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

namespace {
double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
bool append_enabled() { static const bool on = !(getenv("HQTICK_APPEND") && atoi(getenv("HQTICK_APPEND")) == 0); return on; }
size_t al16(size_t v) { return (v + 15) & ~(size_t)15; }
// a staged batch, in pinned memory and in d_add alike: [ids n u64][priorities n u64][request ids n u32], the columns 16-byte aligned
struct AddLayout { size_t o_p, o_q, bytes; };
AddLayout add_layout(uint64_t n) { AddLayout L; L.o_p = al16(n * 8); L.o_q = L.o_p * 2; L.bytes = L.o_q + n * 4 + 16; return L; }
// a packed batch in pinned memory: [id run starts u64][id run offsets n_id_runs + 1 u32][priority run values u64][priority run offsets n_prio_runs + 1 u32][id offsets n u32, optional][request ids n u16]
struct PackedLayout { size_t o_is, o_if, o_pv, o_pf, o_off, o_rq, bytes; };
PackedLayout packed_layout(uint64_t n, uint32_t n_id_runs, uint32_t n_prio_runs, bool with_off) {
    PackedLayout P; P.o_is = 0; P.o_if = al16(P.o_is + (size_t)n_id_runs * 8); P.o_pv = al16(P.o_if + (size_t)(n_id_runs + 1) * 4); P.o_pf = al16(P.o_pv + (size_t)n_prio_runs * 8);
    P.o_off = al16(P.o_pf + (size_t)(n_prio_runs + 1) * 4); P.o_rq = al16(P.o_off + (with_off ? (size_t)n * 4 : 0)); P.bytes = al16(P.o_rq + (size_t)n * 2);
    return P;
}
}  // namespace

void ReadySet::release() {
    for (hqbuf::DevBuf *b : {&d_id, &d_prio, &d_rq, &d_id2, &d_prio2, &d_rq2, &d_slice, &d_add, &d_pre8}) b->release();
    h_add.release(); h_addp.release(); h_flag.release();
}

// ---------------------------------------------------------------------------------------------- the set as a whole
int ReadySet::upload(const Env &e, uint64_t n, const uint64_t *id, const uint64_t *prio, const uint32_t *rq, bool sorted) {
    resident_ = false;  // whatever was resident is being overwritten: only a complete upload makes the set usable again
    uint64_t n_pow2 = 1; while (n_pow2 < n) n_pow2 <<= 1;
    const uint64_t cap = sorted ? n : n_pow2;
    if (!d_id.ensure(cap * 8 + 8) || !d_prio.ensure(cap * 8 + 8) || !d_rq.ensure(cap * 4 + 8)) return fail(HQTICK_E_DEVICE, "hipMalloc ready set");
    if (n) {
        // blocking copies: the caller's columns are pageable memory, and this is the one call whose result every later tick trusts (a level table built from
        // a column that was still arriving would list whatever the buffer held before; seen once under rocprofv3 with the asynchronous form)
        HQ_HIP(hipMemcpy(d_id.p, id, n * 8, hipMemcpyHostToDevice));
        HQ_HIP(hipMemcpy(d_prio.p, prio, n * 8, hipMemcpyHostToDevice));
        HQ_HIP(hipMemcpy(d_rq.p, rq, n * 4, hipMemcpyHostToDevice));
        if (!sorted) {  // the host handed over its queues in whatever order it walked them: sort by id on the device, once
            if (!h_flag.ensure(64)) return fail(HQTICK_E_DEVICE, "hipHostMalloc");
            uint32_t *flag = h_flag.as<uint32_t>(); flag[0] = 0;
            HQ_HIP(hqk::sort_ready(d_id.as<uint64_t>(), d_prio.as<uint64_t>(), d_rq.as<uint32_t>(), n, n_pow2, h_flag.dev<uint32_t>(), e.stream));
            HQ_HIP(hipStreamSynchronize(e.stream));
            if (flag[0]) return fail(HQTICK_E_INVALID, "ready set holds a task id twice (or the id 2^64 - 1)");
        } else {
            HQ_HIP(hipStreamSynchronize(e.stream));
        }
    }
    n_ = n; live_ = n; resident_ = true; abandon_selection();
    max_id = 0; max_id_valid = true;
    if (sorted) { if (n) max_id = id[n - 1]; } else for (uint64_t i = 0; i < n; i++) max_id = std::max(max_id, id[i]);
    return 0;
}

int ReadySet::load(hipStream_t st, const hqtick_snapshot *s, bool with_ids) {
    const uint64_t N = s->n_ready;
    if (!d_id.ensure(N * 8 + 8) || !d_prio.ensure(N * 8 + 8) || !d_rq.ensure(N * 4 + 8)) return fail(HQTICK_E_DEVICE, "hipMalloc ready set");
    if (N) {
        if (with_ids) HQ_HIP(hipMemcpyAsync(d_id.p, s->task_id, N * 8, hipMemcpyHostToDevice, st));
        HQ_HIP(hipMemcpyAsync(d_prio.p, s->task_priority, N * 8, hipMemcpyHostToDevice, st));
        HQ_HIP(hipMemcpyAsync(d_rq.p, s->task_rq, N * 4, hipMemcpyHostToDevice, st));
    }
    n_ = N; resident_ = false;
    return 0;
}

// ---------------------------------------------------------------------------------------------- adding
// Fresh ids behind everything resident, and room at the tail: ONE kernel writes the batch where it belongs and validates it, instead of the four of a merge (the
// columns are not re-written; what the ticks consumed stays as tombstones until a compaction is due).  The steady loop's add: 136 -> ~50 us.
bool ReadySet::can_append(uint64_t n_add, uint64_t first_id, uint64_t last_id) const {
    return append_enabled() && n_ > 0 && n_add > 0 && last_id >= first_id && first_id > 0 && max_id_valid && first_id > max_id &&
           d_id.cap >= (n_ + n_add) * 8 + 8 && d_prio.cap >= (n_ + n_add) * 8 + 8 && d_rq.cap >= (n_ + n_add) * 4 + 8;
}

int ReadySet::refused(uint32_t flag_word) {
    if (flag_word & 4u) return fail(HQTICK_E_INVALID, "hqtick_ready_add: a task id is already in the ready set");
    if (flag_word & 8u) return fail(HQTICK_E_INVALID, "hqtick_ready_add: ids not strictly ascending");
    if (flag_word & 16u) return fail(HQTICK_E_INVALID, "hqtick_ready_add: request id 0xFFFFFFFF is reserved");
    return 0;
}

// (nothing is bumped before the flag word has been read: a refused batch leaves rows behind the columns' end that nothing counts)
int ReadySet::appended(const Env &e, bool waits_on_kernel, uint64_t n_add, uint64_t last_id, const double *trace) {
    if (waits_on_kernel) HQ_HIP(hipEventSynchronize(e.done)); else HQ_HIP(hipStreamSynchronize(e.stream));
    if (trace) fprintf(stderr, "hqtick add (append, packed): n %llu prepare %.1f us, launch %.1f us, wait %.1f us\n", (unsigned long long)n_add, trace[1] - trace[0], trace[2] - trace[1], now_us() - trace[2]);
    if (int rc = refused(h_flag.as<uint32_t>()[0])) return rc;
    n_ += n_add; live_ += n_add; max_id = last_id; n_appends++; abandon_selection();
    return compact_due() ? rebuild(e, nullptr, nullptr, nullptr, 0) : 0;  // (a host that never calls hqtick_ready_consume_last — HQTICK_FLAG_CONSUME_IN_TICK — compacts here)
}

// a batch in device columns whose id range [first_id, last_id] the host knows: appended where that is possible, merged otherwise
int ReadySet::add_columns(const Env &e, const uint64_t *id, const uint64_t *prio, const uint32_t *rq, uint32_t n, uint64_t first_id, uint64_t last_id) {
    if (!can_append(n, first_id, last_id)) return rebuild(e, id, prio, rq, n);
    if (!h_flag.ensure(64)) return fail(HQTICK_E_DEVICE, "hipHostMalloc");
    h_flag.as<uint32_t>()[0] = 0;
    bool waits_on_kernel = false;
    hqk::time_next_launch(nullptr, e.done);
    HQ_HIP_LAST(hqk::ready_append(id, prio, rq, n, max_id, d_id.as<uint64_t>() + n_, d_prio.as<uint64_t>() + n_, d_rq.as<uint32_t>() + n_, h_flag.dev<uint32_t>(), e.stream), waits_on_kernel);
    return appended(e, waits_on_kernel, n, last_id);
}

// Drops the tombstones and merges `n_add` new tasks (device arrays, ids ascending; none: a compaction) into the alternate columns; swaps them in.
int ReadySet::ensure_add(uint64_t n_add) {  // (rebuild's own sizes, for the largest batch the caller may bring)
    const uint64_t N = n_, new_n = live_ + n_add, room = new_n + std::max<uint64_t>(new_n, 4096);
    if (!d_id2.ensure(room * 8 + 8) || !d_prio2.ensure(room * 8 + 8) || !d_rq2.ensure(room * 4 + 8) || !h_flag.ensure(64)) return fail(HQTICK_E_DEVICE, "hipMalloc ready set (rebuild)");
    const uint32_t n_slices = (uint32_t)((N + 255) / 256), stride = (n_slices + 15u) & ~15u;
    if (N && (!d_slice.ensure((size_t)stride * 4 + 64) || !d_pre8.ensure(N + 16))) return fail(HQTICK_E_DEVICE, "hipMalloc slice table");
    return 0;
}

int ReadySet::rebuild(const Env &e, const uint64_t *aid, const uint64_t *aprio, const uint32_t *arq, uint32_t n_add) {
    const uint64_t N = n_, new_n = live_ + n_add;
    // (a rebuild leaves room behind the columns: the next fresh batches are appended)
    const uint64_t room = new_n + std::max<uint64_t>(new_n, 4096);
    if (!d_id2.ensure(room * 8 + 8) || !d_prio2.ensure(room * 8 + 8) || !d_rq2.ensure(room * 4 + 8)) return fail(HQTICK_E_DEVICE, "hipMalloc ready set (rebuild)");
    if (N == 0) {  // nothing resident: the batch becomes the ready set — through the same validation as an appended one (ascending ids, no reserved request id:
                   // a refused batch leaves the set as it was, here: empty), written by the kernel that checks it
        if (n_add) {
            if (!h_flag.ensure(64)) return fail(HQTICK_E_DEVICE, "hipHostMalloc");
            h_flag.as<uint32_t>()[0] = 0;
            HQ_HIP(hqk::ready_append(aid, aprio, arq, n_add, 0xFFFFFFFFFFFFFFFFull, d_id2.as<uint64_t>(), d_prio2.as<uint64_t>(), d_rq2.as<uint32_t>(), h_flag.dev<uint32_t>(), e.stream));
        }
    } else {
        const uint32_t n_slices = (uint32_t)((N + 255) / 256), stride = (n_slices + 15u) & ~15u;
        if (!d_slice.ensure((size_t)stride * 4 + 64) || !h_flag.ensure(64) || !d_pre8.ensure(N + 16)) return fail(HQTICK_E_DEVICE, "hipMalloc slice table");
        uint32_t *flag = h_flag.as<uint32_t>(); flag[0] = 0; flag[1] = 0;
        hqk::WaveGeom g{256, n_slices, 4, stride};
        HQ_HIP(hqk::ready_live_count(d_rq.as<uint32_t>(), N, d_slice.as<uint32_t>(), e.stream));
        HQ_HIP(hqk::scan_waves(d_slice.as<uint32_t>(), g, 1, h_flag.dev<uint32_t>() + 1, nullptr, nullptr, e.stream));
        HQ_HIP(hqk::ready_rebuild(d_id.as<uint64_t>(), d_prio.as<uint64_t>(), d_rq.as<uint32_t>(), N, (uint32_t)live_, d_slice.as<uint32_t>(), aid, aprio, arq, n_add,
                                  d_id2.as<uint64_t>(), d_prio2.as<uint64_t>(), d_rq2.as<uint32_t>(), d_pre8.as<uint8_t>(), h_flag.dev<uint32_t>(), e.stream));
    }
    // the new last id comes back with the flags: the bound later appends are decided by (only of columns that are swapped in: a refused batch leaves the bound as it was)
    if (N || n_add) {  // (N = 0 means nothing live either: new_n = n_add)
        uint64_t *last_back = reinterpret_cast<uint64_t *>(h_flag.as<unsigned char>() + 16);
        if (new_n) HQ_HIP(hipMemcpyAsync(last_back, d_id2.as<uint64_t>() + (new_n - 1), 8, hipMemcpyDeviceToHost, e.stream));
        // (the batch came through a pinned staging buffer the caller may fill again as soon as this call returns: the kernels must be over by then)
        HQ_HIP(hipStreamSynchronize(e.stream));
        const uint32_t *flag = h_flag.as<uint32_t>();
        if (N && flag[1] != live_) return fail(HQTICK_E_DEVICE, "resident ready set: live-task count out of sync");
        if (int rc = refused(flag[0])) return rc;
        if (new_n) { max_id = *last_back; max_id_valid = true; }
    }
    std::swap(d_id, d_id2); std::swap(d_prio, d_prio2); std::swap(d_rq, d_rq2);
    n_ = new_n; live_ = new_n; abandon_selection();
    return 0;
}

int ReadySet::stage(uint64_t n, uint64_t **id, uint64_t **prio, uint32_t **rq) {
    const AddLayout L = add_layout(n);
    if (!h_add.ensure(L.bytes)) return fail(HQTICK_E_DEVICE, "hipHostMalloc delta staging");
    unsigned char *h = h_add.as<unsigned char>();
    *id = reinterpret_cast<uint64_t *>(h); *prio = reinterpret_cast<uint64_t *>(h + L.o_p); *rq = reinterpret_cast<uint32_t *>(h + L.o_q);
    staged_n = n;
    return 0;
}

int ReadySet::add_staged(const Env &e, uint64_t n) {
    if (n > staged_n) return fail(HQTICK_E_INVALID, "hqtick_ready_add_staged: more tasks than hqtick_ready_add_stage made room for");
    const AddLayout L = add_layout(staged_n);  // the layout the pointers were handed out for
    staged_n = 0;
    if (n == 0) return 0;
    const unsigned char *h = h_add.as<unsigned char>();
    const uint64_t *id = reinterpret_cast<const uint64_t *>(h); const uint32_t *rq = reinterpret_cast<const uint32_t *>(h + L.o_q);
    if (n_ == 0) {  // nothing resident: refused here, before anything is copied; otherwise the append / merge kernel validates the batch
        for (uint64_t i = 1; i < n; i++) if (id[i - 1] >= id[i]) return refused(8u);
        for (uint64_t i = 0; i < n; i++) if (rq[i] == hqk::RQ_TOMBSTONE) return refused(16u);
    }
    HQ_HIP(hipSetDevice(e.device));
    if (!d_add.ensure(L.bytes)) return fail(HQTICK_E_DEVICE, "hipMalloc delta staging");
    unsigned char *d = d_add.as<unsigned char>();
    HQ_HIP(hipMemcpyAsync(d, h, L.o_q + n * 4, hipMemcpyHostToDevice, e.stream));
    return add_columns(e, reinterpret_cast<const uint64_t *>(d), reinterpret_cast<const uint64_t *>(d + L.o_p), reinterpret_cast<const uint32_t *>(d + L.o_q), (uint32_t)n, id[0], id[n - 1]);
}

int ReadySet::add_packed(const Env &e, uint64_t n, uint32_t n_id_runs, const uint64_t *id_run_start, const uint32_t *id_run_len, const uint32_t *id_off, uint32_t n_prio_runs,
                         const uint64_t *prio_run_value, const uint32_t *prio_run_len, const uint16_t *task_rq) {
    const PackedLayout P = packed_layout(n, n_id_runs, n_prio_runs, id_off != nullptr);
    static const bool trace_add = getenv("HQTICK_TRACE_ADD") != nullptr;  // (experiments: where the microseconds of an add go, one line per call on stderr)
    double trace[3] = {trace_add ? now_us() : 0.0, 0.0, 0.0};
    if (!h_addp.ensure(P.bytes)) return fail(HQTICK_E_DEVICE, "hipHostMalloc packed delta staging");
    const AddLayout L = add_layout(n);
    if (!d_add.ensure(L.bytes)) return fail(HQTICK_E_DEVICE, "hipMalloc delta staging");
    unsigned char *h = h_addp.as<unsigned char>(), *hd = h_addp.dev<unsigned char>(), *d = d_add.as<unsigned char>();
    memcpy(h + P.o_is, id_run_start, (size_t)n_id_runs * 8); memcpy(h + P.o_pv, prio_run_value, (size_t)n_prio_runs * 8);
    uint32_t *idf = reinterpret_cast<uint32_t *>(h + P.o_if), *pf = reinterpret_cast<uint32_t *>(h + P.o_pf);
    idf[0] = 0; for (uint32_t r = 0; r < n_id_runs; r++) idf[r + 1] = idf[r] + id_run_len[r];
    pf[0] = 0; for (uint32_t r = 0; r < n_prio_runs; r++) pf[r + 1] = pf[r] + prio_run_len[r];
    if (id_off) memcpy(h + P.o_off, id_off, (size_t)n * 4);
    memcpy(h + P.o_rq, task_rq, (size_t)n * 2);
    // the batch's id range, from the run tables: what decides between appending and merging
    const uint64_t first_id = id_run_start[0] + (id_off ? id_off[0] : 0u);
    const uint64_t last_id = id_run_start[n_id_runs - 1] + (id_off ? id_off[n - 1] : id_run_len[n_id_runs - 1] - 1u);
    // the expansion kernel reads the packed batch in place (pinned, device-mapped): what crosses PCIe is the packed form.  It writes the batch behind the columns
    // and validates it — the whole add is this one launch — or into d_add for the merge, which validates it.
    const bool append = can_append(n, first_id, last_id);
    uint64_t *o_id = append ? d_id.as<uint64_t>() + n_ : reinterpret_cast<uint64_t *>(d), *o_prio = append ? d_prio.as<uint64_t>() + n_ : reinterpret_cast<uint64_t *>(d + L.o_p);
    uint32_t *o_rq = append ? d_rq.as<uint32_t>() + n_ : reinterpret_cast<uint32_t *>(d + L.o_q);
    bool waits_on_kernel = false;
    if (append) {
        trace[1] = trace_add ? now_us() : 0.0;
        if (!h_flag.ensure(64)) return fail(HQTICK_E_DEVICE, "hipHostMalloc");
        h_flag.as<uint32_t>()[0] = 0;
        hqk::time_next_launch(nullptr, e.done);
    }
    HQ_HIP_LAST(hqk::ready_unpack_adds((uint32_t)n, n_id_runs, reinterpret_cast<const uint64_t *>(hd + P.o_is), reinterpret_cast<const uint32_t *>(hd + P.o_if), id_off ? reinterpret_cast<const uint32_t *>(hd + P.o_off) : nullptr,
                                       n_prio_runs, reinterpret_cast<const uint64_t *>(hd + P.o_pv), reinterpret_cast<const uint32_t *>(hd + P.o_pf), reinterpret_cast<const uint16_t *>(hd + P.o_rq),
                                       o_id, o_prio, o_rq, append ? max_id : 0, append ? h_flag.dev<uint32_t>() : nullptr, e.stream), waits_on_kernel);
    if (!append) return rebuild(e, o_id, o_prio, o_rq, (uint32_t)n);
    trace[2] = trace_add ? now_us() : 0.0;
    return appended(e, waits_on_kernel, n, last_id, trace_add ? trace : nullptr);
}

// ---------------------------------------------------------------------------------------------- removing
int ReadySet::mark_removed(const Env &e, const uint64_t *dev_ids, uint32_t n) {
    uint32_t *cnt = h_flag.as<uint32_t>(); cnt[0] = 0;
    HQ_HIP(hqk::ready_mark_removed(d_id.as<uint64_t>(), d_rq.as<uint32_t>(), n_, dev_ids, n, h_flag.dev<uint32_t>(), e.stream));
    HQ_HIP(hipStreamSynchronize(e.stream));
    live_ -= cnt[0]; abandon_selection();
    return (int)cnt[0];  // number of tasks that were in the set
}

int ReadySet::remove(const Env &e, uint64_t n, const uint64_t *host_ids) {
    if (!d_add.ensure(n * 8 + 8) || !h_flag.ensure(64)) return fail(HQTICK_E_DEVICE, "hipMalloc delta staging");
    if (!h_add.ensure(n * 8 + 8)) return fail(HQTICK_E_DEVICE, "hipHostMalloc delta staging");
    memcpy(h_add.p, host_ids, n * 8);
    HQ_HIP(hipMemcpyAsync(d_add.p, h_add.p, n * 8, hipMemcpyHostToDevice, e.stream));
    return mark_removed(e, d_add.as<uint64_t>(), (uint32_t)n);
}

int ReadySet::remove_device(const Env &e, const uint64_t *dev_ids, uint32_t n) {
    if (!h_flag.ensure(64)) return fail(HQTICK_E_DEVICE, "hipHostMalloc");
    return mark_removed(e, dev_ids, n);
}

// ---------------------------------------------------------------------------------------------- the last tick's selection
int ReadySet::consumed(const Env &e) {
    live_ -= n_sel_; abandon_selection();  // (nothing is left of it to consume)
    return compact_due() ? rebuild(e, nullptr, nullptr, nullptr, 0) : 0;  // more tombstones than tasks: compact
}

}  // namespace hqready

// Kernels of hqtick_resident_check (audit.h, audit_core.h).  gfx950 only.
//
// Read-only passes over the resident tables, one item per thread, ordered by kernel boundaries on the context's stream: nothing is handed from one workgroup to
// another inside a kernel.  The invariants themselves are audit_core.h's item functions; what is here is how the items are spread over the lanes and how the
// findings leave the wavefront:
//   counters   one atomic add per wavefront and invariant (a ballot over the lanes' finding masks), and none at all in a wavefront that found nothing;
//   witnesses  a 64-bit atomic min, issued only by a lane that found a violation;
//   census     the live rows / live slots are counted the same way, one add per wavefront.
// Sums of integers and minima: the report does not depend on the order in which the wavefronts run.
// This is integer work bound by HBM latency (two dependent hash probes per live ready row); the streams themselves are coalesced, one row or slot per lane.
#include "audit.h"

namespace hqaudit {

namespace {

constexpr uint32_t TPB = 256;
inline unsigned nblk(uint64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

struct DevRep {
    Out o; uint32_t mask;
    __device__ void hit(uint32_t inv, uint64_t key) { mask |= 1u << inv; atomicMin(&o.first[inv], (unsigned long long)key); }
    // every lane of the wavefront must call: one add per invariant some lane found violated
    __device__ void flush() const {
        if (__ballot(mask != 0) == 0) return;
        for (uint32_t inv = 0; inv < HQ_INV_N; inv++) {
            const uint64_t m = __ballot((mask >> inv) & 1u);
            if (m && __lane_id() == (uint32_t)__ffsll((long long)m) - 1u) atomicAdd(&o.count[inv], (unsigned long long)__popcll(m));
        }
    }
};
// one atomic per wavefront for a per-lane flag (every lane of the wave must call)
__device__ __forceinline__ void wave_count(unsigned long long *c, bool v) {
    const uint64_t m = __ballot(v);
    if (m && __lane_id() == (uint32_t)__ffsll((long long)m) - 1u) atomicAdd(c, (unsigned long long)__popcll(m));
}

// the ready columns: neighbour compare (the row before a workgroup's first is read from HBM like any other), liveness, the hash probes of a live row
__global__ void __launch_bounds__(TPB) k_audit_ready(State S, Out o) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    DevRep rep{o, 0u};
    bool live = false;
    if (i < S.ready.n) live = ready_row(S, i, rep);
    wave_count(&o.live[0], live);
    rep.flush();
}
// the graph's slots, first pass: liveness and the way back through the hash table
__global__ void __launch_bounds__(TPB) k_audit_slots(State S, Out o) {
    const uint32_t sl = blockIdx.x * TPB + threadIdx.x;
    DevRep rep{o, 0u};
    bool live = false;
    if (sl < S.graph.n_slots) live = graph_slot_hash(S, sl, rep);
    wave_count(&o.live[1], live);
    rep.flush();
}
// the run chains: a wavefront takes 64 slots, reads their heads with one coalesced load, and walks the chain of every slot that has one with all 64 lanes
// on the run's edges (a hub's run of thousands of edges is a coalesced stream; a task without consumers costs its 4 bytes)
__global__ void __launch_bounds__(TPB) k_audit_edges(State S, uint32_t *__restrict__ cnt) {
    const uint32_t sl = blockIdx.x * TPB + threadIdx.x, lane = threadIdx.x & 63u;
    const bool has = sl < S.graph.n_slots && S.graph.unfinished[sl] != ST_FREE && S.graph.head[sl] != NONE;
    uint64_t m = __ballot(has);
    while (m) {
        const uint32_t src = (uint32_t)__ffsll((long long)m) - 1u;
        m &= m - 1;
        graph_edges(S.graph, sl - lane + src, lane, 64u, cnt, [](uint32_t *p) { atomicAdd(p, 1u); });
    }
}
// the graph's slots, second pass: the counter against the census of the edges; a released task that is nowhere (STRICT)
__global__ void __launch_bounds__(TPB) k_audit_counters(State S, const uint32_t *__restrict__ cnt, Out o) {
    const uint32_t sl = blockIdx.x * TPB + threadIdx.x;
    DevRep rep{o, 0u};
    if (sl < S.graph.n_slots) graph_slot_counter(S, sl, cnt, rep);
    rep.flush();
}
// the ledger.  Rows first (the multi-node columns: a root row counts on its task's bucket), then the buckets (self-probe, validity, the census into the audit's own
// tables, the totals), then the three row tables against the census, one (row, column) per lane.
__global__ void __launch_bounds__(TPB) k_audit_mn_rows(State S, LedgerScratch x, Out o) {
    const uint32_t w = blockIdx.x * TPB + threadIdx.x;
    DevRep rep{o, 0u};
    if (w < S.ledger.W) ledger_mn_row(S, w, x, rep, [](uint32_t *p) { atomicAdd(p, 1u); });
    rep.flush();
}
__global__ void __launch_bounds__(TPB) k_audit_ledger(State S, LedgerScratch x, Out o) {
    const uint64_t b = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    DevRep rep{o, 0u};
    uint32_t cls = CLS_NONE;
    if (b <= S.ledger.mask) cls = ledger_entry(S, (uint32_t)b, x, rep, [](uint32_t *p) { atomicAdd(p, 1u); });
    wave_count(&o.live[2], cls == CLS_SN); wave_count(&o.live[3], cls == CLS_MN); wave_count(&o.live[4], cls == CLS_PF);
    rep.flush();
}
// which: 0 the count table, 1 the prefilled table, 2 the free rows; n items
__global__ void __launch_bounds__(TPB) k_audit_ledger_rows(State S, LedgerScratch x, int which, uint64_t n, Out o) {
    const uint64_t i = (uint64_t)blockIdx.x * TPB + threadIdx.x;
    DevRep rep{o, 0u};
    if (i < n) {
        if (which == 0) ledger_count_item(S, i, x, rep);
        else if (which == 1) ledger_pf_item(S, i, x, rep);
        else ledger_free_item(S, i, rep);
    }
    rep.flush();
}
__global__ void __launch_bounds__(TPB) k_audit_retr(State S, Out o) {
    const uint32_t j = blockIdx.x * TPB + threadIdx.x;
    DevRep rep{o, 0u};
    if (j < S.retr.n) retr_entry(S, j, rep);
    rep.flush();
}

}  // namespace

size_t ledger_scratch_bytes(const State &S) {
    const Ledger &l = S.ledger;
    return ((size_t)l.W * l.stride + (size_t)l.W * l.pf_stride + (size_t)l.mask + 1) * 4;
}

hipError_t launch(const State &S, Out o, uint32_t *cnt, LedgerScratch x, hipStream_t s) {
    if (wants_ready_pass(S)) hipLaunchKernelGGL(k_audit_ready, dim3(nblk(S.ready.n)), dim3(TPB), 0, s, S, o);
    if (wants_graph_pass(S)) {
        const uint32_t n = S.graph.n_slots;
        const bool counters = (S.parts & HQ_CHECK_GRAPH) != 0;
        hipLaunchKernelGGL(k_audit_slots, dim3(nblk(n)), dim3(TPB), 0, s, S, o);
        if (counters) {
            if (hipError_t rc = hipMemsetAsync(cnt, 0, (size_t)n * 4, s)) return rc;
            hipLaunchKernelGGL(k_audit_edges, dim3(nblk(n)), dim3(TPB), 0, s, S, cnt);
        }
        hipLaunchKernelGGL(k_audit_counters, dim3(nblk(n)), dim3(TPB), 0, s, S, counters ? cnt : nullptr, o);
    }
    if (wants_ledger_pass(S)) {
        const Ledger &l = S.ledger;
        const bool part = wants_ledger_part(S);
        if (part) {
            if (hipError_t rc = hipMemsetAsync(x.cen_counts, 0, ledger_scratch_bytes(S), s)) return rc;
            if (l.W) hipLaunchKernelGGL(k_audit_mn_rows, dim3(nblk(l.W)), dim3(TPB), 0, s, S, x, o);
        }
        hipLaunchKernelGGL(k_audit_ledger, dim3(nblk((uint64_t)l.mask + 1)), dim3(TPB), 0, s, S, x, o);
        if (part) {
            const uint64_t nc = (uint64_t)l.W * l.stride, np = (S.have & HAVE_TRACKING) && l.pf ? (uint64_t)l.W * l.pf_stride : 0, nf = (uint64_t)l.W * l.R;
            if (nc) hipLaunchKernelGGL(k_audit_ledger_rows, dim3(nblk(nc)), dim3(TPB), 0, s, S, x, 0, nc, o);
            if (np) hipLaunchKernelGGL(k_audit_ledger_rows, dim3(nblk(np)), dim3(TPB), 0, s, S, x, 1, np, o);
            if (nf) hipLaunchKernelGGL(k_audit_ledger_rows, dim3(nblk(nf)), dim3(TPB), 0, s, S, x, 2, nf, o);
        }
    }
    if (wants_retr_pass(S)) hipLaunchKernelGGL(k_audit_retr, dim3(nblk(S.retr.n)), dim3(TPB), 0, s, S, o);
    return hipGetLastError();
}

}  // namespace hqaudit

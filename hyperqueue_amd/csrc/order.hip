// The ordered view of the ready set: the general path of phase A for ready sets whose (level, request) table does not fit the dense
// scan (more than MAX_LEVELS distinct priorities, or more than MAX_GROUPS groups).
//
// The view is a permutation of the LIVE slots of the id-sorted columns ordered by (request ascending, priority descending, slot ascending) — within one
// priority the slot order is the id order: TaskQueue::take_tasks' order (taskqueue.rs:320-355) — plus a run table with one row per nonempty (request,
// priority) pair.  It is built by a stable LSD radix sort with 8-bit digits over the key (rq, ~priority): digits 0-7 are the bytes of ~priority, 8-11 the
// bytes of rq.  One read pass histograms every digit at once; a digit that is constant over the live set needs no pass.  Each pass is three kernels —
// per-tile digit counts, a per-digit scan of those counts, a stable scatter — with a kernel boundary between them (no hand-off between workgroups of one
// launch).  Inside a tile (one wavefront, ORDER_TILE slots) ranks come from wave-private LDS counters plus the __ballot match-any of K4: no output position
// depends on the order in which atomics arrive, so replicas of a sharded scheduler build the same view byte for byte.
#include "kernels.h"
#include <hip/hip_ext.h>

// a measured launch: bracketed by the pending timer's events (if any) at the dispatch (kernels.hip: HQK_TIMED_LAUNCH)
#define HQK_ORDER_LAUNCH(kern, grid, block, lds, s, ...)                                                  \
    do {                                                                                                  \
        hqk::LaunchTimer t_ = hqk::take_launch_timer();                                                   \
        hipExtLaunchKernelGGL(kern, grid, block, lds, s, t_.start, t_.stop, 0, __VA_ARGS__);              \
    } while (0)

namespace hqk {

namespace {

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// lanes (among `active`) holding the same key as this lane: one __ballot per key bit
__device__ __forceinline__ uint64_t match_any(uint32_t key, int nbits, bool active) {
    uint64_t m = __ballot(active);
    for (int b = 0; b < nbits; b++) {
        bool bit = (key >> b) & 1u;
        uint64_t bal = __ballot(active && bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

// digit dg of the sort key of `slot`: bytes 0-7 of ~priority (descending priority = ascending key), then bytes 0-3 of the request id
__device__ __forceinline__ uint32_t digit_of(const uint64_t *prio, const uint32_t *rq, uint32_t slot, uint32_t dg) {
    return dg < 8 ? (uint32_t)((~prio[slot]) >> (dg * 8)) & 0xFFu : (rq[slot] >> ((dg - 8) * 8)) & 0xFFu;
}

constexpr uint32_t WPB = 4;  // wavefronts (tiles) per workgroup

// one read pass: the histogram of every digit over the live slots, and the request-id check
__global__ void __launch_bounds__(256) k_order_digits(const uint64_t *__restrict__ prio, const uint32_t *__restrict__ rq, uint64_t n, uint32_t Q,
                                                      uint32_t *__restrict__ ghist) {
    __shared__ uint32_t h[ORDER_DIGITS * 256];
    for (uint32_t i = threadIdx.x; i < ORDER_DIGITS * 256; i += blockDim.x) h[i] = 0;
    __syncthreads();
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = rq[i];
        if (r == RQ_TOMBSTONE) continue;
        bad = bad || r >= Q;
        const uint64_t k = ~prio[i];
#pragma unroll
        for (uint32_t dg = 0; dg < 8; dg++) atomicAdd(&h[dg * 256 + ((uint32_t)(k >> (dg * 8)) & 0xFFu)], 1u);
#pragma unroll
        for (uint32_t dg = 0; dg < 4; dg++) atomicAdd(&h[(8 + dg) * 256 + ((r >> (dg * 8)) & 0xFFu)], 1u);
    }
    if (bad) atomicOr(&ghist[ORDER_DIGITS * 256], 1u);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < ORDER_DIGITS * 256; i += blockDim.x) if (h[i]) atomicAdd(&ghist[i], h[i]);  // (sums: the result does not depend on the order)
}

// pass, kernel 1: digit counts of every tile -> tab[d * n_tiles + tile].  first: the input is the column itself (slot = index, tombstones skipped)
__global__ void __launch_bounds__(256) k_radix_count(const uint64_t *__restrict__ prio, const uint32_t *__restrict__ rq, uint64_t n_in, uint32_t first,
                                                     const uint32_t *__restrict__ in, uint32_t dg, uint32_t n_tiles, uint32_t *__restrict__ tab) {
    __shared__ uint32_t s_cnt[WPB * 256];
    const uint32_t wv = threadIdx.x >> 6, lane = lane_id(), tile = blockIdx.x * WPB + wv;
    uint32_t *cnt = s_cnt + wv * 256;
    for (uint32_t d = lane; d < 256; d += 64) cnt[d] = 0;
    if (tile >= n_tiles) return;
    const uint64_t b = (uint64_t)tile * ORDER_TILE, e = b + ORDER_TILE < n_in ? b + ORDER_TILE : n_in;
    for (uint64_t i = b + lane; i < e; i += 64) {
        const uint32_t slot = first ? (uint32_t)i : in[i];
        if (first && rq[slot] == RQ_TOMBSTONE) continue;
        atomicAdd(&cnt[digit_of(prio, rq, slot, dg)], 1u);  // (wave-private counters: a count, not a position)
    }
    for (uint32_t d = lane; d < 256; d += 64) tab[(size_t)d * n_tiles + tile] = cnt[d];
}

// pass, kernel 2: one workgroup per digit d: exclusive scan of row d of tab, offset by the number of live slots with a smaller digit (ghist)
__global__ void __launch_bounds__(256) k_radix_offsets(const uint32_t *__restrict__ ghist, uint32_t dg, uint32_t n_tiles, uint32_t *__restrict__ tab) {
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_carry;
    const uint32_t d = blockIdx.x, lane = lane_id(), wv = threadIdx.x >> 6;
    uint32_t below = threadIdx.x < d ? ghist[dg * 256 + threadIdx.x] : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) below += __shfl_xor(below, off, 64);
    if (lane == 0) s_w[wv] = below;
    __syncthreads();
    if (threadIdx.x == 0) s_carry = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    uint32_t *row = tab + (size_t)d * n_tiles;
    for (uint32_t base = 0; base < n_tiles; base += 256) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t c = i < n_tiles ? row[i] : 0u;
        uint32_t incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { uint32_t t = __shfl_up(incl, off, 64); if ((int)lane >= off) incl += t; }
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        uint32_t before = s_carry;
        for (uint32_t w = 0; w < wv; w++) before += s_w[w];
        if (i < n_tiles) row[i] = before + incl - c;
        __syncthreads();
        if (threadIdx.x == 0) s_carry += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
}

// pass, kernel 3: stable scatter.  The tile's wavefront walks its slots in order, 64 at a time; a slot's output position = its digit's running counter +
// the lanes of the same digit before it (match-any).  Positions are checked against n_out: a count that disagrees with the histogram sets err.
__global__ void __launch_bounds__(256) k_radix_scatter(const uint64_t *__restrict__ prio, const uint32_t *__restrict__ rq, uint64_t n_in, uint32_t first,
                                                       const uint32_t *__restrict__ in, uint32_t dg, uint32_t n_tiles, const uint32_t *__restrict__ tab,
                                                       uint32_t *__restrict__ out, uint32_t n_out, uint32_t *__restrict__ err) {
    __shared__ uint32_t s_cnt[WPB * 256];
    const uint32_t wv = threadIdx.x >> 6, lane = lane_id(), tile = blockIdx.x * WPB + wv;
    if (tile >= n_tiles) return;
    uint32_t *cnt = s_cnt + wv * 256;
    for (uint32_t d = lane; d < 256; d += 64) cnt[d] = tab[(size_t)d * n_tiles + tile];
    const uint64_t b = (uint64_t)tile * ORDER_TILE, e = b + ORDER_TILE < n_in ? b + ORDER_TILE : n_in;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    for (uint64_t c = b; c < e; c += 64) {  // (wave-uniform loop: every lane takes part in the ballots)
        const uint64_t i = c + lane;
        uint32_t slot = 0, d = 0;
        bool active = i < e;
        if (active) { slot = first ? (uint32_t)i : in[i]; active = !first || rq[slot] != RQ_TOMBSTONE; }
        if (active) d = digit_of(prio, rq, slot, dg);
        const uint64_t peers = match_any(d, 8, active);
        if (active) {
            const uint32_t before = (uint32_t)__popcll(peers & lt_mask), cur = cnt[d], pos = cur + before;
            if (pos < n_out) out[pos] = slot; else atomicOr(err, 1u);
            if (before == 0) cnt[d] = cur + (uint32_t)__popcll(peers);
        }
    }
}

// boundaries: position i of a sorted permutation opens a run when its (rq, priority) differs from position i - 1's (rq == NULL: its priority — a level of
// the priority-sorted permutation)
__device__ __forceinline__ bool opens_run(const uint64_t *prio, const uint32_t *rq, const uint32_t *perm, uint64_t i) {
    if (i == 0) return true;
    const uint32_t a = perm[i], b = perm[i - 1];
    return (rq && rq[a] != rq[b]) || prio[a] != prio[b];
}

__global__ void __launch_bounds__(256) k_run_count(const uint64_t *__restrict__ prio, const uint32_t *__restrict__ rq, const uint32_t *__restrict__ perm,
                                                   uint64_t n, uint32_t n_tiles, uint32_t *__restrict__ tile_cnt) {
    const uint32_t wv = threadIdx.x >> 6, lane = lane_id(), tile = blockIdx.x * WPB + wv;
    if (tile >= n_tiles) return;
    const uint64_t b = (uint64_t)tile * ORDER_TILE, e = b + ORDER_TILE < n ? b + ORDER_TILE : n;
    uint32_t cnt = 0;
    for (uint64_t c = b; c < e; c += 64) cnt += (uint32_t)__popcll(__ballot(c + lane < e && opens_run(prio, rq, perm, c + lane)));
    if (lane == 0) tile_cnt[tile] = cnt;
}

// exclusive scan of the per-tile run counts (one workgroup); tile_cnt[n_tiles] = number of runs
__global__ void __launch_bounds__(1024) k_run_scan(uint32_t *__restrict__ tile_cnt, uint32_t n_tiles, uint32_t *__restrict__ n_runs_out) {
    __shared__ uint32_t s_w[16];
    __shared__ uint32_t s_carry;
    const uint32_t lane = lane_id(), wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n_tiles; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t c = i < n_tiles ? tile_cnt[i] : 0u;
        uint32_t incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { uint32_t t = __shfl_up(incl, off, 64); if ((int)lane >= off) incl += t; }
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        uint32_t before = s_carry;
        for (uint32_t w = 0; w < wv; w++) before += s_w[w];
        if (i < n_tiles) tile_cnt[i] = before + incl - c;
        __syncthreads();
        if (threadIdx.x == 0) { uint32_t t = 0; for (uint32_t w = 0; w < 16; w++) t += s_w[w]; s_carry += t; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { tile_cnt[n_tiles] = s_carry; n_runs_out[0] = s_carry; }
}

// the global level rank of every live slot, from the priority-sorted permutation: lrank[slot] = number of distinct priorities above the slot's
__global__ void __launch_bounds__(256) k_level_write(const uint64_t *__restrict__ prio, const uint32_t *__restrict__ perm, uint64_t n, uint32_t n_tiles,
                                                     const uint32_t *__restrict__ tile_off, uint32_t *__restrict__ lrank) {
    const uint32_t wv = threadIdx.x >> 6, lane = lane_id(), tile = blockIdx.x * WPB + wv;
    if (tile >= n_tiles) return;
    const uint64_t b = (uint64_t)tile * ORDER_TILE, e = b + ORDER_TILE < n ? b + ORDER_TILE : n;
    const uint64_t le_mask = lane == 63 ? ~0ull : (2ull << lane) - 1ull;
    uint32_t r = tile_off[tile];
    for (uint64_t c = b; c < e; c += 64) {
        const uint64_t i = c + lane;
        const uint64_t bal = __ballot(i < e && opens_run(prio, nullptr, perm, i));
        if (i < e) lrank[perm[i]] = r + (uint32_t)__popcll(bal & le_mask) - 1u;  // (position 0 opens a level: r + popcount >= 1)
        r += (uint32_t)__popcll(bal);
    }
}

// the run table (rq, start, priority, level rank per run) and the inverse permutation inv[slot] = position in the view
__global__ void __launch_bounds__(256) k_run_write(const uint64_t *__restrict__ prio, const uint32_t *__restrict__ rq, const uint32_t *__restrict__ perm,
                                                   uint64_t n, uint32_t n_tiles, const uint32_t *__restrict__ tile_off, const uint32_t *__restrict__ lrank,
                                                   uint32_t *__restrict__ inv, uint32_t *__restrict__ run_rq, uint32_t *__restrict__ run_start,
                                                   uint32_t *__restrict__ run_rank, uint64_t *__restrict__ run_prio) {
    const uint32_t wv = threadIdx.x >> 6, lane = lane_id(), tile = blockIdx.x * WPB + wv;
    if (tile >= n_tiles) return;
    const uint64_t b = (uint64_t)tile * ORDER_TILE, e = b + ORDER_TILE < n ? b + ORDER_TILE : n;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    uint32_t r = tile_off[tile];
    for (uint64_t c = b; c < e; c += 64) {
        const uint64_t i = c + lane;
        const bool open = i < e && opens_run(prio, rq, perm, i);
        const uint64_t bal = __ballot(open);
        if (i < e) inv[perm[i]] = (uint32_t)i;
        if (open) {
            const uint32_t k = r + (uint32_t)__popcll(bal & lt_mask), slot = perm[i];
            run_rq[k] = rq[slot]; run_start[k] = (uint32_t)i; run_rank[k] = lrank[slot]; run_prio[k] = prio[slot];
        }
        r += (uint32_t)__popcll(bal);
    }
}

// K4 on the view: selected task j of request q (rq_sel_base[q] <= j < rq_sel_base[q + 1]) is the task at position p = j - rq_sel_base[q] of q's segment
__global__ void __launch_bounds__(256) k_order_select(OrderSelect os, uint32_t n_sel) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_sel) return;
    uint32_t lo = 0, hi = os.Q;  // last request with rq_sel_base[q] <= j (requests that take nothing share their base with the next one)
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (os.rq_sel_base[mid] <= j) lo = mid; else hi = mid; }
    const uint32_t q = lo, p = j - os.rq_sel_base[q];
    const uint32_t r0 = os.run_off[q], r1 = os.run_off[q + 1];
    if (r0 >= r1) { atomicOr(os.err, 1u); return; }
    const uint32_t pos = os.run_start[r0] + p;
    const uint32_t seg_end = r1 < os.n_runs ? os.run_start[r1] : os.n_live;
    if (pos >= seg_end) { atomicOr(os.err, 1u); return; }  // (the plan never takes more than the queue holds: a guard, not a path)
    uint32_t a = r0, z = r1;  // the run of that position: last run of q with start <= pos
    while (z - a > 1) { const uint32_t mid = (a + z) >> 1; if (os.run_start[mid] <= pos) a = mid; else z = mid; }
    const uint32_t slot = os.perm[pos];
    if (os.mark_rq) os.mark_rq[slot] = os.mark_value == RQ_TOMBSTONE ? RQ_TOMBSTONE : q;  // consume (tombstone) or restore (the request id back)
    if (os.mark_rq && !os.mark_and_select) return;
    uint32_t dst = j;
    const uint32_t nc = os.q_tnc[q];
    if (nc) {  // worker-major (kernels.hip: k_select): position p of the queue -> (worker p % n, its task p / n)
        const uint32_t nw = nc >> 16, c = nc & 0xFFFFu;
        if (p < nw * c) { const uint32_t sw = p / nw; dst = os.rq_sel_base[q] + (p - sw * nw) * c + sw; }
    }
    os.sel_task[dst] = os.task_id[slot];
    os.sel_rank[dst] = os.run_rank[a];
}

// where the Retracting tasks sit: (request, position in the view) of every wanted id, 0xFFFFFFFF = not a live task of the set
__global__ void __launch_bounds__(256) k_order_rank_of(const uint64_t *__restrict__ ids, const uint32_t *__restrict__ rq, uint64_t n, const uint32_t *__restrict__ inv,
                                                       const uint64_t *__restrict__ want, uint32_t n_want, uint32_t *__restrict__ out_rq, uint32_t *__restrict__ out_pos) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_want) return;
    const uint64_t id = want[k];
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (ids[mid] < id) lo = mid + 1; else hi = mid; }
    const bool found = lo < n && ids[lo] == id && rq[lo] != RQ_TOMBSTONE;
    out_rq[k] = found ? rq[lo] : 0xFFFFFFFFu;
    out_pos[k] = found ? inv[lo] : 0xFFFFFFFFu;
}

}  // namespace

hipError_t order_digits(const uint64_t *prio, const uint32_t *rq, uint64_t n, uint32_t Q, uint32_t *ghist, hipStream_t s) {
    hipError_t e;
    if ((e = hipMemsetAsync(ghist, 0, (ORDER_DIGITS * 256 + 4) * 4, s)) != hipSuccess) return e;
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_order_digits, dim3((uint32_t)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, prio, rq, n, Q, ghist);
    return hipGetLastError();
}

hipError_t order_pass(const uint64_t *prio, const uint32_t *rq, uint64_t n_in, bool first, const uint32_t *in, uint32_t dg, const uint32_t *ghist, uint32_t *tab,
                      uint32_t *out, uint32_t n_out, uint32_t *err, hipStream_t s) {
    const uint32_t n_tiles = order_tiles(n_in);
    if (n_tiles == 0) return hipSuccess;
    const dim3 grid((n_tiles + WPB - 1) / WPB);
    hipLaunchKernelGGL(k_radix_count, grid, dim3(256), 0, s, prio, rq, n_in, first ? 1u : 0u, in, dg, n_tiles, tab);
    hipLaunchKernelGGL(k_radix_offsets, dim3(256), dim3(256), 0, s, ghist, dg, n_tiles, tab);
    hipLaunchKernelGGL(k_radix_scatter, grid, dim3(256), 0, s, prio, rq, n_in, first ? 1u : 0u, in, dg, n_tiles, (const uint32_t *)tab, out, n_out, err);
    return hipGetLastError();
}

hipError_t order_levels(const uint64_t *prio, const uint32_t *perm, uint32_t n, uint32_t *tile_cnt, uint32_t *lrank, uint32_t *n_levels, hipStream_t s) {
    const uint32_t n_tiles = order_tiles(n);
    if (n_tiles == 0) return hipSuccess;
    const dim3 grid((n_tiles + WPB - 1) / WPB);
    hipLaunchKernelGGL(k_run_count, grid, dim3(256), 0, s, prio, (const uint32_t *)nullptr, perm, (uint64_t)n, n_tiles, tile_cnt);
    hipLaunchKernelGGL(k_run_scan, dim3(1), dim3(1024), 0, s, tile_cnt, n_tiles, n_levels);
    hipLaunchKernelGGL(k_level_write, grid, dim3(256), 0, s, prio, perm, (uint64_t)n, n_tiles, (const uint32_t *)tile_cnt, lrank);
    return hipGetLastError();
}

hipError_t order_runs(const uint64_t *prio, const uint32_t *rq, const uint32_t *perm, uint32_t n, uint32_t *tile_cnt, const uint32_t *lrank, uint32_t *inv,
                      uint32_t *n_runs, uint32_t *run_rq, uint32_t *run_start, uint32_t *run_rank, uint64_t *run_prio, hipStream_t s) {
    const uint32_t n_tiles = order_tiles(n);
    if (n_tiles == 0) return hipSuccess;
    const dim3 grid((n_tiles + WPB - 1) / WPB);
    hipLaunchKernelGGL(k_run_count, grid, dim3(256), 0, s, prio, rq, perm, (uint64_t)n, n_tiles, tile_cnt);
    hipLaunchKernelGGL(k_run_scan, dim3(1), dim3(1024), 0, s, tile_cnt, n_tiles, n_runs);
    hipLaunchKernelGGL(k_run_write, grid, dim3(256), 0, s, prio, rq, perm, (uint64_t)n, n_tiles, (const uint32_t *)tile_cnt, lrank, inv, run_rq, run_start, run_rank, run_prio);
    return hipGetLastError();
}

hipError_t order_select(const OrderSelect &os, uint32_t n_sel, hipStream_t s) {
    if (n_sel == 0) return hipSuccess;
    HQK_ORDER_LAUNCH(k_order_select, dim3((n_sel + 255) / 256), dim3(256), 0, s, os, n_sel);
    return hipGetLastError();
}

hipError_t order_rank_of(const uint64_t *ids, const uint32_t *rq, uint64_t n, const uint32_t *inv, const uint64_t *want, uint32_t n_want, uint32_t *out_rq, uint32_t *out_pos,
                         hipStream_t s) {
    if (n_want == 0) return hipSuccess;
    hipLaunchKernelGGL(k_order_rank_of, dim3((n_want + 255) / 256), dim3(256), 0, s, ids, rq, n, inv, want, n_want, out_rq, out_pos);
    return hipGetLastError();
}

}  // namespace hqk

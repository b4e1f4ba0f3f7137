// gfx950 census of the resident ready set: live tasks per (priority level, request id), for hqtick_query_resident (include/hqtick.h).
//
// Read-only on the context: it streams the priority (8 B) and request-id (4 B) columns of the resident set and writes nothing but the
// caller's count table.  K1 (k_level_hist, kernels.hip) counts the same groups but also leaves a group key per task behind, which
// hqtick_ready_consume_last replays the last selection from; a query between two ticks must not touch those keys, hence this kernel.
// The level table comes from K0 / K0b (distinct_priorities / sort_levels) run into buffers of the query's own: its length and values
// are read from HBM here, so discovery, sort and census follow each other on the stream with no host round trip between them.
#include "kernels.h"

namespace hqk {

namespace {

static const uint32_t CENSUS_LDS_BINS = 4096;   // L x Q up to this: one LDS histogram per workgroup; above it every add goes to the global table
static const uint32_t CENSUS_LDS_LEVELS = 512;  // level tables up to this are staged in LDS; a longer one is searched in place (L2-resident, read-only)
static const uint32_t CENSUS_TILE = 2048;       // tasks per workgroup step: 256 lanes x 8 consecutive tasks (four dwordx4 of priorities, two of request ids)

// lanes (among `active`) holding the same key as this lane: one __ballot per key bit (the match-any of kernels.hip)
__device__ __forceinline__ uint64_t census_match_any(uint32_t key, int nbits, bool active) {
    uint64_t m = __ballot(active);
    for (int b = 0; b < nbits; b++) {
        const bool bit = (key >> b) & 1u;
        const uint64_t bal = __ballot(active && bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

// out = [err u32 x 4][count u32 x L*Q]  (zeroed by the caller), count index = level * Q + rq.
// err[0] bit 0: a priority missing from the level table, bit 1: a request id >= Q, bit 2: the level table is unusable (more than MAX_LEVELS
// levels, or L * Q > MAX_GROUPS); no count is written then.
__global__ void __launch_bounds__(256) k_census(const uint64_t *__restrict__ prio, const uint32_t *__restrict__ rq, uint64_t n, uint32_t Q,
                                                const uint64_t *__restrict__ levels, const uint32_t *__restrict__ n_levels, uint32_t *__restrict__ out) {
    __shared__ uint64_t s_lv[CENSUS_LDS_LEVELS];
    __shared__ uint32_t s_hist[CENSUS_LDS_BINS];
    // The first tile's loads go out before anything that needs the level table (the table is one more round trip to HBM, written a moment ago by k_sort_levels)
    uint64_t p[8];
    uint32_t q[8];
    auto load_tile = [&](uint64_t i) {   // i is a multiple of 8: 64-byte aligned priorities, 32-byte aligned request ids
        if (i + 7 < n) {
#pragma unroll
            for (int u = 0; u < 4; u++) { const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(prio + i + 2 * u); p[2 * u] = a.x; p[2 * u + 1] = a.y; }
#pragma unroll
            for (int u = 0; u < 2; u++) { const uint4 r = *reinterpret_cast<const uint4 *>(rq + i + 4 * u); q[4 * u] = r.x; q[4 * u + 1] = r.y; q[4 * u + 2] = r.z; q[4 * u + 3] = r.w; }
        } else {
#pragma unroll
            for (int u = 0; u < 8; u++) { const bool in = i + u < n; p[u] = in ? prio[i + u] : 0; q[u] = in ? rq[i + u] : RQ_TOMBSTONE; }
        }
    };
    const uint64_t first = (uint64_t)blockIdx.x * CENSUS_TILE, step = (uint64_t)gridDim.x * CENSUS_TILE;
    if (first < n) load_tile(first + 8u * threadIdx.x);
    const uint32_t L = n_levels[0];   // (written by k_sort_levels ahead of this launch on the same stream; 0xFFFFFFFF = too many levels)
    if (L == 0) return;               // every slot is a tombstone: nothing to count
    if (L > MAX_LEVELS || (uint64_t)L * Q > MAX_GROUPS) { if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&out[0], 4u); return; }
    const uint32_t G = L * Q;
    const bool in_lds = G <= CENSUS_LDS_BINS;
    const int nbits = G > 1 ? 32 - __clz(G - 1) : 0;
    const bool lv_lds = L <= CENSUS_LDS_LEVELS;
    const uint64_t *lv = lv_lds ? s_lv : levels;
    if (lv_lds) for (uint32_t i = threadIdx.x; i < L; i += blockDim.x) s_lv[i] = levels[i];
    if (in_lds) for (uint32_t g = threadIdx.x; g < G; g += blockDim.x) s_hist[g] = 0;
    __syncthreads();
    uint32_t *__restrict__ table = out + 4;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t err = 0;
    for (uint64_t base = first; base < n; base += step) {   // (base is uniform: every lane reaches every ballot)
#pragma unroll
        for (int u = 0; u < 8; u++) {
            bool active = q[u] != RQ_TOMBSTONE;   // a tombstone left the set (handed out / removed) and counts nowhere
            uint32_t key = 0;
            if (active) {
                if (q[u] >= Q) { err |= 2u; active = false; }
                else {
                    uint32_t lo = 0, hi = L;   // first index of the descending table with lv[idx] <= p
                    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (lv[mid] > p[u]) lo = mid + 1; else hi = mid; }
                    if (lo >= L || lv[lo] != p[u]) { err |= 1u; active = false; }
                    else key = lo * Q + q[u];
                }
            }
            // wave-aggregated: the lowest lane of every run of equal keys adds the run's length, one add per distinct key of the wave
            const uint64_t m = census_match_any(key, nbits, active);
            if (active && lane == (uint32_t)(__ffsll((long long)m) - 1)) {
                const uint32_t c = (uint32_t)__popcll(m);
                if (in_lds) atomicAdd(&s_hist[key], c); else atomicAdd(&table[key], c);
            }
        }
        if (base + step < n) load_tile(base + step + 8u * threadIdx.x);
    }
    if (err) atomicOr(&out[0], err);
    if (!in_lds) return;
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < G; g += blockDim.x) { const uint32_t c = s_hist[g]; if (c) atomicAdd(&table[g], c); }
}

}  // namespace

hipError_t ready_census(const uint64_t *prio, const uint32_t *rq, uint64_t n, uint32_t Q, const uint64_t *levels, const uint32_t *n_levels, uint32_t *out, hipStream_t s) {
    if (n == 0 || Q == 0) return hipSuccess;
    const uint64_t tiles = (n + CENSUS_TILE - 1) / CENSUS_TILE;
    const unsigned blocks = (unsigned)(tiles < 2048 ? tiles : 2048);   // (20 KB of LDS: eight workgroups per CU; beyond 2048 tiles the workgroups stride)
    hipLaunchKernelGGL(k_census, dim3(blocks), dim3(256), 0, s, prio, rq, n, Q, levels, n_levels, out);
    return hipGetLastError();
}

}  // namespace hqk

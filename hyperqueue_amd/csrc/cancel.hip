// Kernels of a cancel batch's grouping (cancel.h, cancel_core.h).  gfx950 only: wave64, 256-thread workgroups.
#include "cancel.h"

namespace hqcancel {

namespace {

// the lanes of the calling wavefront whose digit equals its own: one __ballot per bit (8 digit bits + the bit that tells NO_DIGIT from 0xFF).  Every lane calls it.
struct DevMatch {
    HQC_HD static uint64_t match(const SortLds &, uint32_t, uint32_t d) {
#if defined(__HIP_DEVICE_COMPILE__)
        uint64_t m = ~0ull;
#pragma unroll
        for (int b = 0; b < 9; b++) {
            const bool bit = (d >> b) & 1u;
            const uint64_t bal = __ballot(bit);
            m &= bit ? bal : ~bal;
        }
        return m;
#else
        (void)d;
        return 0;
#endif
    }
};

__global__ void __launch_bounds__(BLOCK) k_cancel_count(SortArgs a) {
    __shared__ SortLds l;
    const int tid = (int)threadIdx.x;
    sort_p_zero(l, tid); sort_p_digits(a, l, blockIdx.x, tid);
    __syncthreads();
    sort_p_hist<DevMatch>(l, tid);
    __syncthreads();
    count_p_out(a, l, blockIdx.x, tid);
}
__global__ void __launch_bounds__(BLOCK) k_cancel_scan(SortArgs a) {
    __shared__ ScanLds l;
    const int tid = (int)threadIdx.x;
    scan_p1(a, l, tid);
    __syncthreads();
    scan_p2(l, tid);
    __syncthreads();
    scan_p3(a, l, tid);
}
__global__ void __launch_bounds__(BLOCK) k_cancel_scatter(SortArgs a) {
    __shared__ SortLds l;
    const int tid = (int)threadIdx.x;
    sort_p_zero(l, tid); sort_p_digits(a, l, blockIdx.x, tid);
    __syncthreads();
    sort_p_hist<DevMatch>(l, tid);
    __syncthreads();
    scatter_p_base(a, l, blockIdx.x, tid);
    __syncthreads();
    scatter_p_move<DevMatch>(a, l, blockIdx.x, tid);
}
__global__ void __launch_bounds__(BLOCK) k_cancel_mark(FinArgs a) { fin_mark(a, (uint64_t)blockIdx.x * BLOCK + threadIdx.x); }
__global__ void __launch_bounds__(BLOCK) k_cancel_lists(FinArgs a) {
    __shared__ FinLds l;
    const int tid = (int)threadIdx.x;
    fin_p1(a, l, tid);
    __syncthreads();
    fin_p2(a, l, tid);
    __syncthreads();
    fin_p3(a, l, tid);
}

}  // namespace

hipError_t sort_rows(uint32_t n, uint32_t W, const uint32_t *route, uint32_t *scratch, const uint32_t **key_out, const uint32_t **pos_out, hipStream_t s) {
    const Scratch sc = scratch_of(n, W);
    uint32_t *key[2] = {scratch + sc.key0, scratch + sc.key1}, *pos[2] = {scratch + sc.pos0, scratch + sc.pos1};
    const uint32_t nt = n_tiles_of(n), passes = passes_of(W);
    int cur = 0;
    for (uint32_t p = 0; p < passes && nt; p++) {
        SortArgs a{};
        a.n = n; a.W = W; a.shift = p * 8; a.n_tiles = nt; a.cnt = scratch + sc.cnt;
        if (p == 0) a.route = route; else { a.key_in = key[cur]; a.pos_in = pos[cur]; }
        const int nxt = p == 0 ? 0 : cur ^ 1;
        a.key_out = key[nxt]; a.pos_out = pos[nxt];
        hipLaunchKernelGGL(k_cancel_count, dim3(nt), dim3(BLOCK), 0, s, a);
        hipLaunchKernelGGL(k_cancel_scan, dim3(1), dim3(BLOCK), 0, s, a);
        hipLaunchKernelGGL(k_cancel_scatter, dim3(nt), dim3(BLOCK), 0, s, a);
        cur = nxt;
    }
    *key_out = key[cur]; *pos_out = pos[cur];
    return hipGetLastError();
}

hipError_t group(const Group &g, hipStream_t s) {
    const Scratch sc = scratch_of(g.n, g.W);
    const uint32_t *key = nullptr, *pos = nullptr;
    if (hipError_t r = sort_rows(g.n, g.W, g.route, g.scratch, &key, &pos, s); r != hipSuccess) return r;
    FinArgs f{};
    f.n = g.n; f.W = g.W; f.key = key; f.pos = pos; f.id = g.id; f.wid = g.wid; f.route = g.route; f.kind = g.kind; f.start = g.scratch + sc.start;
    f.out_id = g.out_id; f.out_wid = g.out_wid; f.out_off = g.out_off; f.hdr = g.hdr; f.route_wid = g.route_wid; f.route_kind = g.route_kind; f.no_worker = g.no_worker;
    if (g.n) hipLaunchKernelGGL(k_cancel_mark, dim3((g.n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, f);
    hipLaunchKernelGGL(k_cancel_lists, dim3(1), dim3(BLOCK), 0, s, f);
    return hipGetLastError();
}

}  // namespace hqcancel

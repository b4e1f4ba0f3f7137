// hqwire_table_* (include/hqwire.h): the resident task-attribute table of the wire encoder -- its kernels, the HIP backend of hqwtab::Table and the C ABI.
// The phases and the host side live in wire_table_core.h; the CPU debug hook (include/hqtick_debug.h) puts the same Table on host memory.
//
// Launch shapes (wave64, 256-thread workgroups, integer work bound by HBM bandwidth or by dependent-load latency, no MFMA):
//   k_wtab_append / _check / _remove / _setinst   one thread per batch row (id); append adds workgroups for a long blob range
//   k_wtab_count / _move                          one workgroup per tile of HQWIRE_TABLE_TILE rows; k_wtab_scan one workgroup over the tiles
//   k_wtab_merge                                  one thread per row of the old table and of the batch
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/hqtick.h"
#ifdef HQTICK_TEST_HOOKS
#include "../../include/hqtick_debug.h"
#endif
#include "wire_table_core.h"

using namespace hqwtab;

namespace {

__global__ __launch_bounds__(BLOCK) void k_wtab_append(TArgs a) {
    const uint64_t g = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    append_p(a, g);
    append_blob(a, g, (uint64_t)gridDim.x * BLOCK);
}
__global__ __launch_bounds__(BLOCK) void k_wtab_check(TArgs a) { check_p(a, (uint64_t)blockIdx.x * BLOCK + threadIdx.x); }
__global__ __launch_bounds__(BLOCK) void k_wtab_remove(TArgs a) { remove_p(a, (uint64_t)blockIdx.x * BLOCK + threadIdx.x); }
__global__ __launch_bounds__(BLOCK) void k_wtab_setinst(TArgs a) { setinst_p(a, (uint64_t)blockIdx.x * BLOCK + threadIdx.x); }

__global__ __launch_bounds__(BLOCK) void k_wtab_count(TArgs a) {
    __shared__ MoveLds lds;
    const uint32_t t = blockIdx.x;
    const int tid = (int)threadIdx.x;
    tile_p1(a, lds, t, tid);
    __syncthreads();
    tile_p2a(a, lds, t, tid);
    __syncthreads();
    count_p3(a, lds, t, tid);
}
__global__ __launch_bounds__(BLOCK) void k_wtab_scan(TArgs a) {
    __shared__ ScanLds lds;
    const int tid = (int)threadIdx.x;
    scan_p1(a, lds, tid);
    __syncthreads();
    scan_p2a(a, lds, tid);
    __syncthreads();
    scan_p2b(a, lds, tid);
    __syncthreads();
    scan_p2c(a, lds, tid);
    __syncthreads();
    scan_p3(a, lds, tid);
}
__global__ __launch_bounds__(BLOCK) void k_wtab_move(TArgs a) {
    __shared__ MoveLds lds;
    const uint32_t t = blockIdx.x;
    const int tid = (int)threadIdx.x;
    tile_p1(a, lds, t, tid);
    __syncthreads();
    tile_p2a(a, lds, t, tid);
    __syncthreads();
    move_p2b(a, lds, t, tid);
    __syncthreads();
    move_p3(a, lds, t, tid);
    __syncthreads();
    move_p4(a, lds, t, tid);
}
__global__ __launch_bounds__(BLOCK) void k_wtab_merge(TArgs a) {
    __shared__ MoveLds lds;
    const int tid = (int)threadIdx.x;
    merge_p1(a, lds, blockIdx.x, tid);
    __syncthreads();
    blob_p(lds, tid);
}

struct HipBackend : Backend {
    hipStream_t st;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool timing = false;
    explicit HipBackend(hipStream_t s) : st(s) {
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) e0 = e1 = nullptr;
    }
    ~HipBackend() override {
        if (e0) hipEventDestroy(e0);
        if (e1) hipEventDestroy(e1);
    }
    void *alloc(size_t bytes) override {
        void *p = nullptr;
        return hipMalloc(&p, bytes ? bytes : 1) == hipSuccess ? p : nullptr;
    }
    void release(void *p) override { hipFree(p); }
    void *alloc_staging(size_t bytes) override {
        void *p = nullptr;
        return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : nullptr;
    }
    void release_staging(void *p) override { hipHostFree(p); }
    bool upload(void *dev, const void *staging, size_t bytes) override { return !bytes || hipMemcpyAsync(dev, staging, bytes, hipMemcpyHostToDevice, st) == hipSuccess; }
    bool download(void *host, const void *dev, size_t bytes) override {
        if (bytes && hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st) != hipSuccess) return false;
        return hipStreamSynchronize(st) == hipSuccess;
    }
    bool fill(void *dev, int byte, size_t bytes) override { return !bytes || hipMemsetAsync(dev, byte, bytes, st) == hipSuccess; }
    bool launch(int kernel, const TArgs &a, uint32_t blocks) override {
        if (!blocks) return true;
        const dim3 g(blocks), b(BLOCK);
        switch (kernel) {
        case K_APPEND: hipLaunchKernelGGL(k_wtab_append, g, b, 0, st, a); break;
        case K_CHECK: hipLaunchKernelGGL(k_wtab_check, g, b, 0, st, a); break;
        case K_REMOVE: hipLaunchKernelGGL(k_wtab_remove, g, b, 0, st, a); break;
        case K_SETINST: hipLaunchKernelGGL(k_wtab_setinst, g, b, 0, st, a); break;
        case K_COUNT: hipLaunchKernelGGL(k_wtab_count, g, b, 0, st, a); break;
        case K_SCAN: hipLaunchKernelGGL(k_wtab_scan, g, b, 0, st, a); break;
        case K_MOVE: hipLaunchKernelGGL(k_wtab_move, g, b, 0, st, a); break;
        case K_MERGE: hipLaunchKernelGGL(k_wtab_merge, g, b, 0, st, a); break;
        default: return false;
        }
        return hipGetLastError() == hipSuccess;
    }
    bool sync() override { return hipStreamSynchronize(st) == hipSuccess; }
    void time_begin() override { timing = e0 && hipEventRecord(e0, st) == hipSuccess; }
    double time_end_us() override {  // called behind a drained stream
        float ms = 0;
        if (!timing || hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return 0;
        return 1000.0 * ms;
    }
};

}  // namespace

struct hqwire_table {
    Table t;
    hqwire_table(Backend *be, const hqwire_table_config *cfg) : t(be, cfg) {}
};

namespace {
int finish_create(hqwire_table **out, Backend *be, const hqwire_table_config *cfg) {
    hqwire_table *h = be ? new (std::nothrow) hqwire_table(be, cfg) : nullptr;
    if (!h) { delete be; return HQTICK_E_DEVICE; }
    if (!h->t.init()) { delete h; return HQTICK_E_DEVICE; }
    *out = h;
    return 0;
}
}  // namespace

extern "C" {

int hqwire_table_create(hqwire_table **out, const hqwire_table_config *cfg, void *hip_stream) {
    if (!out) return HQTICK_E_INVALID;
    *out = nullptr;
    if (cfg && cfg->initial_rows >= MAX_ROWS) return HQTICK_E_INVALID;
    int n_dev = 0, dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return HQTICK_E_NO_DEVICE;  // no CPU path in the product
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return HQTICK_E_NO_DEVICE;
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) return HQTICK_E_NO_DEVICE;  // the kernels are built for gfx950 only
    return finish_create(out, new (std::nothrow) HipBackend((hipStream_t)hip_stream), cfg);
}

void hqwire_table_destroy(hqwire_table *t) { delete t; }

int64_t hqwire_table_add_configs(hqwire_table *t, uint32_t n, const uint8_t *time_some, const uint64_t *time_secs, const uint32_t *time_nanos,
                                 const uint64_t *body_off, const uint8_t *body_blob) {
    return t ? t->t.add_configs(n, time_some, time_secs, time_nanos, body_off, body_blob) : HQTICK_E_INVALID;
}
int64_t hqwire_table_add_tasks(hqwire_table *t, uint64_t n, const uint64_t *task_id, const uint32_t *task_rq, const uint32_t *task_instance,
                               const uint64_t *task_priority, const uint32_t *task_config, const uint8_t *entry_some, const uint64_t *entry_off,
                               const uint8_t *entry_blob) {
    return t ? t->t.add_tasks(n, task_id, task_rq, task_instance, task_priority, task_config, entry_some, entry_off, entry_blob) : HQTICK_E_INVALID;
}
int64_t hqwire_table_remove_tasks(hqwire_table *t, uint64_t n, const uint64_t *task_id) { return t ? t->t.remove_tasks(n, task_id) : HQTICK_E_INVALID; }
int64_t hqwire_table_set_instance(hqwire_table *t, uint64_t n, const uint64_t *task_id, const uint32_t *values) {
    return t ? t->t.set_instance(n, task_id, values) : HQTICK_E_INVALID;
}
int hqwire_table_compact(hqwire_table *t) { return t ? t->t.compact() : HQTICK_E_INVALID; }
int hqwire_table_view(const hqwire_table *t, hqwire_tables *out) {
    if (!t || !out) return HQTICK_E_INVALID;
    t->t.view(out);
    return 0;
}
int hqwire_table_copy_out(const hqwire_table *t, hqwire_tables *host) {
    if (!t || !host) return HQTICK_E_INVALID;
    return const_cast<hqwire_table *>(t)->t.copy_out(host);
}
int hqwire_table_get_stats(const hqwire_table *t, hqwire_table_stats *out) {
    if (!t || !out) return HQTICK_E_INVALID;
    t->t.stats(out);
    return 0;
}
uint64_t hqwire_table_last_unknown(const hqwire_table *t) { return t ? t->t.last_unknown() : 0; }
const char *hqwire_table_last_error(const hqwire_table *t) { return t ? t->t.last_error() : "no table"; }

#ifdef HQTICK_TEST_HOOKS  // libhqtick_test.so only
// The table on HOST memory with the kernels' phases emulated (`order`: sequence of the emulated threads, as in hqwire_debug_encode_host_order): every
// other hqwire_table_* call works on it, its view holds host pointers for hqwire_debug_encode_host.
int hqwire_debug_table_create_host(hqwire_table **out, const hqwire_table_config *cfg, int order) {
    if (!out || order < 0 || order > 2) return HQTICK_E_INVALID;
    *out = nullptr;
    if (cfg && cfg->initial_rows >= MAX_ROWS) return HQTICK_E_INVALID;
    return finish_create(out, new (std::nothrow) HostBackend(order), cfg);
}
#endif

}  // extern "C"

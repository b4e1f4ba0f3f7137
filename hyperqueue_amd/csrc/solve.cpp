// hqsolve::Solver (solve.h): the block-solve launcher, the wiring of a placement solve, the RCCL communicator.
#include "solve.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "block_solve.h"
#include "kernels.h"

namespace hqsolve {

#define HQ_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(HQTICK_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)

namespace {
// duration between two dispatch events in us, or -1 when the pair was not recorded by a launch of this tick (the runtime's error state is
// cleared: an unrecorded event must not surface as the "last error" of the next launch)
double elapsed_us(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, a, b) == hipSuccess) return (double)ms * 1000.0;
    (void)hipGetLastError();
    return -1.0;
}

// librccl is loaded on first use (dlopen), so that a single-GPU host needs no RCCL at all and a process that already carries one (e.g. PyTorch's) shares it.
// north_star: "workers hash-partitioned across the GPUs of one node with a single RCCL allgather over xGMI to merge the assignment vector".
struct Rccl {
    void *h = nullptr;
    decltype(&ncclGetUniqueId) get_id = nullptr;
    decltype(&ncclCommInitRank) init_rank = nullptr;
    decltype(&ncclAllGather) all_gather = nullptr;
    decltype(&ncclCommDestroy) destroy = nullptr;
    decltype(&ncclGetErrorString) err = nullptr;
    bool ok() const { return h && get_id && init_rank && all_gather && destroy && err; }
};
Rccl &rccl() {
    static Rccl r;
    if (!r.h) {
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { r.h = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (r.h) break; }
        if (r.h) {
            r.get_id = (decltype(r.get_id))dlsym(r.h, "ncclGetUniqueId"); r.init_rank = (decltype(r.init_rank))dlsym(r.h, "ncclCommInitRank");
            r.all_gather = (decltype(r.all_gather))dlsym(r.h, "ncclAllGather"); r.destroy = (decltype(r.destroy))dlsym(r.h, "ncclCommDestroy");
            r.err = (decltype(r.err))dlsym(r.h, "ncclGetErrorString");
        }
    }
    return r;
}
}  // namespace

// The per-class blocks of the separable placement on the device (csrc/block_solve.hip): tables staged in ONE pinned, device-mapped buffer
// that the kernel reads in place (a few dozen bytes per class) and writes its answers into; one launch, one synchronisation.
struct Solver::DeviceBlocks : hqhost::BlockSolver {
    Solver &s; const Env &e; Stats *st;
    DeviceBlocks(Solver &solver, const Env &env, Stats *stats) : s(solver), e(env), st(stats) {}
    bool solve(const hqblock::ColTable &ct, const hqblock::ClassTable &cl, const hqblock::Output &out) override { return begin(ct, cl, out) && finish(); }
    bool overlaps() const override { return true; }
    // state between begin() and finish()
    hqblock::Output p_out{}; BlockLayout L; uint32_t p_nd = 0, p_nc = 0; bool p_launched = false, p_pending = false;
    bool begin(const hqblock::ColTable &ct, const hqblock::ClassTable &cl, const hqblock::Output &out) override {
        p_pending = false;
        const uint32_t NC = ct.n_cols, R = ct.R, nd = cl.n_classes;
        L = block_layout(NC, R, ct.ent_off[NC], nd);
        if (!s.h_blk.ensure(L.pinned_bytes())) return false;
        if (!s.d_blk.ensure(L.device_bytes())) return false;
        unsigned char *h = s.h_blk.as<unsigned char>(), *d = s.d_blk.as<unsigned char>(), *dpin = s.h_blk.dev<unsigned char>();
        pack_cols(h, ct, L); pack_classes(h, cl, R, L);
        // inputs: one copy into HBM (929 wavefronts reading the same table through PCIe reads would queue behind each other); outputs: written by the
        // kernel straight into pinned memory
        if (hqk::copy_pinned_to_hbm(dpin, d, L.o_x, e.stream) != hipSuccess) return false;  // (a copy kernel, not the copy engine: ~10 us less per launch)
        const hqblock::ColTable dct = cols_view(d, NC, R, L);  // [0, o_free) = the column table: staged into LDS by the kernel
        const hqblock::ClassTable dcl = classes_view(d, nd, L);
        uint64_t *dprof = nullptr;
        if (s.block_profile) {  // HQTICK_BLOCK_PROFILE=1: per-class stage timestamps (tools/block_profile.py)
            if (!s.h_blkprof.ensure((size_t)nd * 64 + 64)) return false;
            memset(s.h_blkprof.p, 0, (size_t)nd * 64);
            dprof = s.h_blkprof.dev<uint64_t>(); s.n_blkprof = nd;
        }
        hqblock::Output dout{(uint32_t *)(dpin + L.o_x), (uint32_t *)(dpin + L.o_st), (uint32_t *)(dpin + L.o_steps), dprof};
        hqk::time_next_launch(e.timing ? e.blk_start : nullptr, e.blk_stop);
        const hipError_t be = hqblock::block_solve(dct, dcl, dout, s.block_budget, e.stream);
        const bool launched = hqk::take_launch_timer().stop == nullptr && e.wait_on_kernel;
        if (be != hipSuccess) return false;
        p_out = out; p_nd = nd; p_nc = NC; p_launched = launched; p_pending = true;
        return true;
    }
    bool finish() override {
        if (!p_pending) return false;
        p_pending = false;
        if ((p_launched ? hipEventSynchronize(e.blk_stop) : hipStreamSynchronize(e.stream)) != hipSuccess) return false;  // the kernel's own completion signal
        const unsigned char *h = s.h_blk.as<unsigned char>();
        memcpy(p_out.x, h + L.o_x, (size_t)p_nd * p_nc * 4); memcpy(p_out.status, h + L.o_st, (size_t)p_nd * 4); memcpy(p_out.steps, h + L.o_steps, (size_t)p_nd * 4);
        if (st) {
            if (e.timing) { const double us_ = elapsed_us(e.blk_start, e.blk_stop); if (us_ >= 0) st->block_solve_us = us_; }
            st->blocks_finished = true; st->n_classes_launched = p_nd;
        }
        return true;
    }
};

// The ranks' exchange through the library's RCCL communicator (the callback's: solve_core.h, FnExchange)
struct Solver::CommExchange : hqprice::Exchange {
    Solver &s; const Env &e;
    CommExchange(Solver &solver, const Env &env) : s(solver), e(env) { rank = env.shard_index; world = env.shard_count; }
    bool allgather(const void *send, void *recv, size_t bytes) override { return s.allgather_host(e, send, recv, bytes); }
};

int Solver::init(int device, hipStream_t stream) {
    (void)device;
    if (const char *v = getenv("HQTICK_BLOCK_PROFILE")) block_profile = atoi(v) != 0;
    if (const char *v = getenv("HQTICK_BLOCK_BUDGET")) { long n = atol(v); if (n >= 1 && n <= (1 << 24)) block_budget = (uint32_t)n; }
    if (const char *v = getenv("HQTICK_BLOCK_MIN_CLASSES")) { long n = atol(v); if (n >= 0) block_min_classes = (uint32_t)n; }
    {
        bool price = true; uint32_t min_cols = 0;
        if (const char *v = getenv("HQTICK_PRICE")) price = atoi(v) != 0;
        if (const char *v = getenv("HQTICK_PRICE_MIN_COLS")) { long n = atol(v); if (n > 0) min_cols = (uint32_t)n; }
        if (price) { pricer = new hqprice::DeviceSweeper(stream); pricer->budget = block_budget; if (min_cols) pricer->min_cols = min_cols; }
    }
    if (const char *v = getenv("HQTICK_BLOCK_VERIFY")) block_verify = strcmp(v, "all") == 0 ? 0xFFFFFFFFu : (uint32_t)std::max(0L, atol(v));
    if (const char *v = getenv("HQTICK_SHARD_SOLVE")) shard_solve = atoi(v) != 0;
    if (const char *v = getenv("HQTICK_SHARD_MIN_BLOCKS")) { long n = atol(v); if (n >= 0) shard_min_blocks = (uint32_t)n; }
    if (const char *v = getenv("HQTICK_SHARD_MIN_CLASSES")) { long n = atol(v); if (n >= 0) shard_min_classes = (uint32_t)n; }
    return 0;
}

void Solver::release() {
    delete pricer; pricer = nullptr;
    d_blk.release(); h_blk.release(); h_blkprof.release();
    d_xsend.release(); d_xrecv.release(); h_xsend.release(); h_xrecv.release();
}

hqhost::Counts Solver::solve(const Env &e, hqhost::Problem &pb, const std::vector<hqhost::TaskBatch> &batches, const Opts &o, Stats *st) {
    DeviceBlocks dev_blocks(*this, e, st);
    wire(pb, Wiring{&dev_blocks, block_min_classes, pricer, block_verify, o.tick_seq, o.use_memo ? &block_memo : nullptr});
    pb.defer_row_check = o.defer_row_check; pb.no_fast_path = o.no_fast_path;
    FnExchange fn_x(xfn, xuser, e.shard_index, e.shard_count); CommExchange comm_x(*this, e);
    hqprice::Exchange &xch = xfn ? static_cast<hqprice::Exchange &>(fn_x) : comm_x;  // the host's callback if one is set, else the library's communicator
    double shard_sweep_us = -1.0;
    hqhost::Counts cnt = run_solver(pb, batches, sharded(e) ? &xch : nullptr, shard_min_classes, shard_min_blocks, &shard_sweep_us);
    unwire(pb);
    if (st) {
        st->price_sweep_us = shard_sweep_us >= 0.0 ? shard_sweep_us : (pricer ? pricer->stat_sweep_us : 0.0);
        st->exchange_calls = (uint32_t)xch.n_calls; st->exchange_bytes = xch.n_bytes; st->exchange_us = xch.us;
    }
    return cnt;
}

const uint64_t *Solver::block_profile_last(uint32_t *n_classes) const {
    if (!block_profile || !n_blkprof) { if (n_classes) *n_classes = 0; return nullptr; }
    if (n_classes) *n_classes = n_blkprof;
    return h_blkprof.as<uint64_t>();
}

// ---------------------------------------------------------------------------------------------- the RCCL communicator
int Solver::comm_unique_id(void *id_out) {
    Rccl &r = rccl();
    if (!r.ok()) return HQTICK_E_NO_DEVICE;
    ncclUniqueId id;
    if (r.get_id(&id) != ncclSuccess) return HQTICK_E_DEVICE;
    static_assert(sizeof(id) == HQTICK_COMM_ID_BYTES, "ncclUniqueId size");
    memcpy(id_out, &id, sizeof(id));
    return 0;
}

int Solver::comm_init(int device, const void *id, uint32_t rank, uint32_t world) {
    Rccl &r = rccl();
    if (!r.ok()) return fail(HQTICK_E_NO_DEVICE, "librccl.so could not be loaded");
    HQ_HIP(hipSetDevice(device));
    if (comm) { r.destroy((ncclComm_t)comm); comm = nullptr; }
    ncclUniqueId uid; memcpy(&uid, id, sizeof(uid));
    ncclComm_t c = nullptr;
    ncclResult_t rc = r.init_rank(&c, (int)world, uid, (int)rank);
    if (rc != ncclSuccess) { comm = nullptr; return fail(HQTICK_E_DEVICE, std::string("ncclCommInitRank: ") + r.err(rc)); }
    comm = c; comm_rank = rank; comm_world_ = world;
    return 0;
}

void Solver::comm_destroy(int device) {
    if (comm) { hipSetDevice(device); rccl().destroy((ncclComm_t)comm); comm = nullptr; }
    comm_world_ = 0; comm_rank = 0;
}

int Solver::allgather_device(const Env &e, const void *send, void *recv, size_t bytes) {
    HQ_HIP(hipSetDevice(e.device));
    ncclResult_t rc = rccl().all_gather(send, recv, bytes, ncclUint8, (ncclComm_t)comm, e.stream);
    if (rc != ncclSuccess) return fail(HQTICK_E_DEVICE, std::string("ncclAllGather: ") + rccl().err(rc));
    HQ_HIP(hipStreamSynchronize(e.stream));
    return 0;
}

// all-gather of a small HOST buffer through the RCCL communicator: staged through HBM (ncclAllGather wants device memory on both sides)
bool Solver::allgather_host(const Env &e, const void *send, void *recv, size_t bytes) {
    if (!comm || bytes == 0) return false;
    const size_t total = bytes * comm_world_;
    if (!h_xsend.ensure(bytes) || !h_xrecv.ensure(total) || !d_xsend.ensure(bytes) || !d_xrecv.ensure(total)) return false;
    if (hipSetDevice(e.device) != hipSuccess) return false;
    memcpy(h_xsend.p, send, bytes);
    if (hipMemcpyAsync(d_xsend.p, h_xsend.p, bytes, hipMemcpyHostToDevice, e.stream) != hipSuccess) return false;
    if (rccl().all_gather(d_xsend.p, d_xrecv.p, bytes, ncclUint8, (ncclComm_t)comm, e.stream) != ncclSuccess) return false;
    if (hipMemcpyAsync(h_xrecv.p, d_xrecv.p, total, hipMemcpyDeviceToHost, e.stream) != hipSuccess) return false;
    if (hipStreamSynchronize(e.stream) != hipSuccess) return false;
    memcpy(recv, h_xrecv.p, total);
    return true;
}

}  // namespace hqsolve

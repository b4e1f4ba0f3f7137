// The placement's device side: phase B of a tick.  A Solver owns the staging of the k_block_solve launches and their knobs, the price sweeper
// (k_price_sweep), the memo of host-solved class blocks, the ranks' exchange — the host's callback or the library's own RCCL communicator, with its staging — and the
// knobs of the sharded solve:
//   solve()               wires the block solver, the sweeper and the memo onto the Problem, wraps them for a sharded scheduler where sharded() holds, runs
//                         run_scheduling_solver once, and takes the wiring off again
//   replica() / sharded() whether others read this context's placement / whether the ranks split the solve
//   comm_*, allgather_*   the RCCL communicator (librccl is loaded on first use) and its two all-gathers: of device memory, and of a small host buffer
// What needs no HIP — the launch's layout, the emulated and the sharded block solver, the callback exchange — is solve_core.h's.  Like hqmap::Mapper, a method that
// returns int returns an HQTICK_E_* code (negative) with `err` set.  A failed block-solve launch is no error: the launcher returns false and the host solver takes
// the classes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/hqtick.h"
#include "devbuf.h"
#include "host_model.h"
#include "price_dev.h"
#include "solve_core.h"

namespace hqsolve {

// What the solver uses of its context.  blk_start is recorded only where `timing` asks for it; blk_stop is carried by k_block_solve's dispatch in any case — it is
// what the host waits on.
struct Env {
    int device; hipStream_t stream;
    hipEvent_t blk_start, blk_stop;
    bool timing, wait_on_kernel;
    uint32_t shard_index, shard_count;  // hqtick_set_shard
};
struct Opts { bool defer_row_check, no_fast_path; uint32_t tick_seq; bool use_memo; };
// of the last solve(); block_solve_us < 0: not measured; blocks_finished: a block-solve launch was waited for, n_classes_launched classes in it
struct Stats {
    double block_solve_us = -1; bool blocks_finished = false; uint32_t n_classes_launched = 0;
    uint32_t exchange_calls = 0; uint64_t exchange_bytes = 0; double exchange_us = 0, price_sweep_us = 0;
};

class Solver {
  public:
    std::string err;
    int init(int device, hipStream_t stream);  // the environment's knobs (HQTICK_BLOCK_*, HQTICK_PRICE*, HQTICK_SHARD_*), the sweeper
    void release();
    hqhost::Counts solve(const Env &e, hqhost::Problem &pb, const std::vector<hqhost::TaskBatch> &batches, const Opts &o, Stats *st);
    // others read this context's sweeps or records: a shard of several, a host's exchange, a communicator (a record sink alone is one scheduler's output path)
    bool replica(const Env &e) const { return e.shard_count > 1 || xfn || comm; }
    bool sharded(const Env &e) const { return shard_solve && e.shard_count > 1 && (xfn || (comm && comm_world_ == e.shard_count)); }
    void set_exchange(hqtick_exchange_fn fn, void *user) { xfn = fn; xuser = fn ? user : nullptr; }
    static int comm_unique_id(void *id_out);  // [HQTICK_COMM_ID_BYTES]
    int comm_init(int device, const void *id, uint32_t rank, uint32_t world);
    void comm_destroy(int device);
    bool has_comm() const { return comm != nullptr; }
    uint32_t comm_world() const { return comm_world_; }
    int allgather_device(const Env &e, const void *send, void *recv, size_t bytes);   // device memory on both sides; waits
    bool allgather_host(const Env &e, const void *send, void *recv, size_t bytes);    // a small host buffer, staged through HBM
    const uint64_t *block_profile_last(uint32_t *n_classes) const;  // HQTICK_BLOCK_PROFILE=1: the last launch's per-class stage timestamps

  private:
    struct DeviceBlocks;
    struct CommExchange;
    int fail(int code, const std::string &m) { err = m; return code; }

    hqbuf::PinBuf h_blk; hqbuf::DevBuf d_blk;  // one launch's staged image (solve_core.h: BlockLayout) and the copy of its inputs in HBM
    hqbuf::PinBuf h_blkprof; uint32_t n_blkprof = 0; bool block_profile = false;
    uint32_t block_budget = 4096, block_min_classes = 12;  // k_block_solve: search steps per class before the host solver takes it; classes below which the host solves alone
    uint32_t block_verify = 2;  // HQTICK_BLOCK_VERIFY: classes of a k_block_solve launch the host re-solves while the kernel runs (host_model.h: Problem::block_verify)
    hqhost::BlockMemo block_memo;  // host class blocks of earlier ticks (host_model.h)
    hqprice::DeviceSweeper *pricer = nullptr;  // k_price_sweep: the block sweeps of the coupled placement (csrc/price.hip); HQTICK_PRICE=0 keeps coupled ticks on the host search
    // sharded placement solve: the ranks split the coupled solve's price sweeps and the separable solve's class blocks, one small all-gather of host
    // buffers per sweep / per launch — through the host's callback (hqtick_set_exchange) or the library's own RCCL communicator
    uint32_t shard_min_blocks = 1025, shard_min_classes = 1025; bool shard_solve = true;
    hqtick_exchange_fn xfn = nullptr; void *xuser = nullptr;
    void *comm = nullptr; uint32_t comm_rank = 0, comm_world_ = 0;  // hqtick_comm_init (an ncclComm_t)
    hqbuf::DevBuf d_xsend, d_xrecv; hqbuf::PinBuf h_xsend, h_xrecv;
};

}  // namespace hqsolve

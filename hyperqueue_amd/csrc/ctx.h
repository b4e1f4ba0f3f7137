// The context behind the C ABI (include/hqtick.h: hqtick_ctx), for the two sources that see its layout: hqtick.cpp, which runs the ticks and checks the ABI's
// arguments, and debug_tick.cpp, the test library's hooks on a context.  Besides the struct: the HQ_HIP* macros and fail(), which leave an error's text in the
// context, and per module what it is given of the context (its Env) and how its errors come back (*_fail).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/hqtick.h"
#include "audit.h"
#include "cluster.h"
#include "devbuf.h"
#include "graph.h"
#include "host_model.h"
#include "kernels.h"
#include "ledger.h"
#include "map.h"
#include "ready.h"
#include "scan.h"
#include "solve.h"
#include "tick_core.h"

// The ordered view by itself (debug_tick.cpp: hqtick_debug_order_view and the two hooks that run on the view it built): a scanner of its own, so that the context
// keeps its permutation, its pending selection and its cached level table; what is known of that view; the hooks' scratch in HBM.
struct ViewHooks {
    hqscan::Scanner scan;
    bool valid = false; const void *ids = nullptr; uint64_t N = 0; uint32_t Q = 0, n_live = 0; bool rq_copy = false; std::vector<uint32_t> run_off, run_start, run_rank;
    hqbuf::DevBuf d_map, d_sel_task, d_sel_rank, d_rq, d_want;  // the selection's tables and output, the copy of the request column hqtick_debug_order_select marks, the ids hqtick_debug_order_rank_of looks up
    void release() { scan.release(); d_map.release(); d_sel_task.release(); d_sel_rank.release(); d_rq.release(); d_want.release(); }
};

struct hqtick_ctx {
    hqtick_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // K2 (worker evaluation: PCIe-latency-bound reads of the worker tables) runs here, next to K1 + K1b on `stream`
    bool k2_on_hist = false;       // HQTICK_K2_RIDE_ALONG=1: K2 rides along K1's launch (round 1 / first half of round 2); default: along K1b's
    bool k2_own_stream = false;    // HQTICK_K2_RIDE_ALONG=0: K2 as its own launch on stream2.  Measured (profiles/r02/README.md): K1 alone then takes 4.8 us instead of
                                   // 8.2 us (0.31 vs 0.18 of the HBM roofline), but the second stream's launch + synchronisation make phase A 36 us instead of 28 us:
                                   // the ride-along layout stays the default because the TICK is what counts
    hipEvent_t ev[14] = {};  // (ev[12] / ev[13]: around the kernels of the ordered view)
    std::string err = "";
    hqready::ReadySet ready;       // hqtick_upload_ready, hqtick_ready_* (ready.h): the ready set's columns in HBM (resident, or a tick's own), their deltas, the last selection's state
    hqscan::Scanner scan;          // GPU phase A (scan.h): the dense scan with its cached level table, the ordered view, the census — on the query sub-context, a query's
    hqsolve::Solver solver;        // the placement (solve.h): the block solvers' staging and knobs, the price sweeper, the block memo, the ranks' exchange and communicator
    hqmap::Mapper map;             // the mapping plan and GPU phase C (map.h): the plan's buffers, the records, the result's host part, the last selection's launch state
    bool timing = true, timing_k1 = false;  // (timing_k1: events around K1 alone, hqtick_set_kernel_timing(ctx, 2))
    hqbuf::PinBuf h_up, h_up2, h_q;
    hqcluster::WorkerSet ws;      // hqtick_cluster_* (ABI 5 and 7; cluster.h): the worker / request tables resident in HBM and their host mirror
    hqcluster::Retracting retr;   // hqtick_retracting_* (ABI 7): the table of Retracting tasks
    uint32_t last_row_groups = 0; // hqtick_cluster_last_row_groups
    bool wait_on_kernel = true;   // HQ_HIP_LAST; HQTICK_WAIT_ON_KERNEL=0: hipStreamSynchronize at every wait (A/B)
    bool defer_row_check = true;  // the coupled fast path's row check runs while phase C's kernels do; HQTICK_DEFER_ROW_CHECK=0: inside the solve (A/B)
    hqhost::Problem pb;
    // results (host)
    hqstages::BatchExport batches;
    std::vector<uint8_t> q_loaded;
    hqtick_kernel_stats stats{};
    uint32_t tpw_hint = 0;                            // HQTICK_TPW (tuning knob): tasks per wavefront slice
    uint32_t shard_index = 0, shard_count = 1;       // hqtick_set_shard
    void *sink = nullptr; size_t sink_bytes = 0;      // hqtick_set_record_sink (device memory)
    hqgraph::Graph graph;  // hqtick_graph_*: dependency counters + consumer lists in HBM
    hqasg::Ledger asg;     // hqtick_assigned_* (ABI 12; ledger.h)
    hqbuf::PinBuf h_cancel_ids; hqbuf::DevBuf d_cancel_ids; uint64_t cancel_ready_removed = 0;  // hqtick_cancel_tasks: the ids' staging and their one device copy; hqtick_cancel_last_ready_removed
    hqbuf::PinBuf h_fail_in; hqbuf::DevBuf d_fail_in;      // hqtick_fail_tasks: the same staging of its own
    hqbuf::PinBuf h_start_in; hqbuf::DevBuf d_start_in;    // hqtick_start_tasks: ids, reporting workers and variants, 13 B per position, staged once and copied to the device once
    hqbuf::PinBuf h_reject_in; hqbuf::DevBuf d_reject_in;  // hqtick_reject_tasks: ids, reporting workers, the order by (id, position), requests (only with Retracting tasks) and variants, staged once
    hqcluster::Reassigned reject_reassigned;               // hqtick_reject_last_reassigned
    hqcluster::Reassigned lose_reassigned;                 // hqtick_lose_last_reassigned
    std::vector<uint64_t> lose_mn_task; std::vector<uint32_t> lose_mn_lost, lose_mn_root;  // hqtick_lose_last_mn_left
    hqbuf::PinBuf h_finish_in; hqbuf::DevBuf d_finish_in;  // hqtick_finish_tasks: ids and reporting workers, 12 B per position, staged once and copied to the device once
    hqtick_ctx *qctx = nullptr;  // hqtick_query's private sub-context
    ViewHooks *view_hooks = nullptr;  // hqtick_debug_order_view's scanner and scratch (test library only), allocated on first use; nothing of it is touched on a tick's path
    uint32_t tick_seq = 0;  // the tick counter: moves the block solvers' sample window from tick to tick (host_model.h: Problem::tick_seq)
    double tl[32] = {}; int ntl = 0;  // debug timeline (us since tick start), hqtick_timeline()
    hqaudit::Auditor audit;  // hqtick_resident_check (audit.h): nothing of it exists until the first call
    bool check_resident = false; int audit_depth = 0;  // HQTICK_CHECK_RESIDENT=1: the audit behind every call that changes resident state (audit_depth: inside such a call)
};

#define HQ_HIP(call)                                                                                          \
    do {                                                                                                      \
        hipError_t e_ = (call);                                                                               \
        if (e_ != hipSuccess) { ctx->err = std::string(#call) + ": " + hipGetErrorString(e_); return HQTICK_E_DEVICE; } \
    } while (0)

// a launch wrapper that was handed a timer (hqk::time_next_launch) but returned without launching must not leave it to the next launch
#define HQ_HIP_TIMED(call)                                                                                    \
    do {                                                                                                      \
        hipError_t e_ = (call);                                                                               \
        hqk::take_launch_timer();                                                                             \
        if (e_ != hipSuccess) { ctx->err = std::string(#call) + ": " + hipGetErrorString(e_); return HQTICK_E_DEVICE; } \
    } while (0)

// The last launch of a phase carries a stop event (hipExtLaunchKernel: the dispatch's own completion signal), and the host waits on THAT instead of
// hipStreamSynchronize, which submits a marker packet of its own and returns 5.6 us after the kernel is done where the kernel's signal is seen after 2.8 us
// (tools/exp/launch_latency.hip, MI355X / ROCm 7.2).  `launched` = the wrapper really launched (it consumed the pending timer); otherwise the
// caller falls back to the stream.
#define HQ_HIP_LAST(call, launched)                                                                           \
    do {                                                                                                      \
        hipError_t e_ = (call);                                                                               \
        (launched) = hqk::take_launch_timer().stop == nullptr && ctx->wait_on_kernel;                        \
        if (e_ != hipSuccess) { ctx->err = std::string(#call) + ": " + hipGetErrorString(e_); return HQTICK_E_DEVICE; } \
    } while (0)

inline int fail(hqtick_ctx *ctx, int code, const std::string &msg) { ctx->err = msg; return code; }

// the worker set (hqcluster::WorkerSet, cluster.h)
inline int cluster_fail(hqtick_ctx *ctx, int rc) { if (rc < 0) ctx->err = ctx->ws.err; return rc; }

// the ready set (hqready::ReadySet, ready.h): what it is given of the context (ev[11]: the completion event an append's dispatch carries), and its errors
inline hqready::Env ready_env(hqtick_ctx *ctx) { return hqready::Env{ctx->device, ctx->stream, ctx->ev[11], ctx->wait_on_kernel}; }
inline int ready_fail(hqtick_ctx *ctx, int rc) { if (rc < 0) ctx->err = ctx->ready.err; return rc; }

// GPU phase A (hqscan::Scanner, scan.h): what it is given of the context (ev[0] / ev[1] around K0, ev[2] / ev[3] around K1, ev[8] K1b's completion, ev[12] / ev[13]
// around the kernels of the ordered view), and its errors
inline hqscan::Env scan_env(hqtick_ctx *ctx) {
    return hqscan::Env{ctx->stream, ctx->stream2, ctx->ev[0], ctx->ev[1], ctx->ev[2], ctx->ev[3], ctx->ev[8], ctx->ev[12], ctx->ev[13],
                       ctx->timing, ctx->timing_k1, ctx->wait_on_kernel, ctx->k2_on_hist, ctx->k2_own_stream, ctx->tpw_hint};
}
inline int scan_fail(hqtick_ctx *ctx, int rc) { if (rc < 0) ctx->err = ctx->scan.err; return rc; }

// The placement (hqsolve::Solver, solve.h): what it is given of the context (ev[9] / ev[10] around k_block_solve — ev[10] is its completion, which the host waits
// on), and its errors
inline hqsolve::Env solve_env(hqtick_ctx *ctx) { return hqsolve::Env{ctx->device, ctx->stream, ctx->ev[9], ctx->ev[10], ctx->timing, ctx->wait_on_kernel, ctx->shard_index, ctx->shard_count}; }
inline int solver_fail(hqtick_ctx *ctx, int rc) { if (rc < 0) ctx->err = ctx->solver.err; return rc; }

// The mapping (hqmap::Mapper, map.h): what it is given of the context (ev[4] / ev[5] around K4, ev[1] / ev[6] around K5a, ev[7] / ev[11] around K5b — ev[11] is K5b's
// completion, which the host waits on), and its errors
inline hqmap::Env map_env(hqtick_ctx *ctx, double t0 = 0) {
    return hqmap::Env{ctx->stream, ctx->ev[4], ctx->ev[5], ctx->ev[1], ctx->ev[6], ctx->ev[7], ctx->ev[11], ctx->timing, ctx->wait_on_kernel, ctx->cfg.flags,
                      ctx->sink, ctx->sink_bytes, ctx->shard_index, ctx->shard_count, hqmap::Timeline{t0, ctx->tl, &ctx->ntl}};
}
inline int map_fail(hqtick_ctx *ctx, int rc) { if (rc < 0) ctx->err = ctx->map.err; return rc; }

// The assignment ledger (hqasg::Ledger, ledger.h; ABI 12): what it is given of the context, and its errors
inline hqasg::Env ledger_env(hqtick_ctx *ctx) {
    const hqready::Cols c = ctx->ready.cols();
    return hqasg::Env{ctx->device, ctx->stream, ctx->ws.rows(), ctx->ws.W(), ctx->ws.R(), c.id, c.prio, c.rq, c.n,
                      ctx->scan.levels_dev(), &ctx->ws.ids(), ctx->ws.flags(), ctx->ws.free_rows()};
}
inline int ledger_fail(hqtick_ctx *ctx, int rc) { if (rc < 0) ctx->err = ctx->asg.err; return rc; }

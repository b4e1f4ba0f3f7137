// libhqtick.so — the C ABI of include/hqtick.h: one scheduling tick of tako on an MI355X.
//
// Data flow of hqtick_run():
//   H2D   ready-set columns (unless resident), worker/request tables
//   GPU   K0 distinct priorities -> K0b sorted level table -> K1 (level, rq) histogram per wave slice -> K1b scan
//         K2 per-(worker, variant) capability flags + task_max_count
//   D2H   level table, histogram, flags                                   (small)
//   HOST  batches (batches.rs) -> MILP (solver.rs) via the exact solver -> counts; selection plan
//   H2D   take/base per group, round-robin tables                         (small)
//   GPU   K4 select+scatter the taken tasks in queue order -> K5 expand to per-worker records
//   D2H   assignment records
// The stages live in modules of their own, each behind a class that owns its buffers and takes a small Env: the ready set (ready.h), phase A (scan.h), the worker
// set (cluster.h), the ledger (ledger.h), the placement's solvers and the ranks' exchange (solve.h; what needs no HIP in solve_core.h), the mapping plan and phase C
// (map.h; the plan itself, free of HIP, in map_core.h).  This file keeps the context, the sequence of a tick (TickRun::run) and the C ABI's argument checks.
// There is no CPU implementation of the scans or of the selection and the records: without a HIP device every entry point fails.
#include "../../include/hqtick.h"
#ifdef HQTICK_TEST_HOOKS
#include "../../include/hqtick_debug.h"
#endif

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "audit.h"
#include "cluster.h"
#include "ready.h"
#include "scan.h"
#include "solve.h"
#ifdef HQTICK_TEST_HOOKS
#include "price_emul.h"
#endif
#include "devbuf.h"
#include "graph.h"
#include "ledger.h"
#include "map.h"
#include "host_model.h"
#include "kernels.h"

using hqbuf::DevBuf;
using hqbuf::PinBuf;
using hqcluster::UpView;
using hqscan::Scan;
using hqscan::WorkerEval;

namespace {

double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

namespace {
// The ordered view by itself (hqtick_debug_order_view and the two hooks that run on the view it built): a scanner of its own, so that the context keeps its
// permutation, its pending selection and its cached level table; what is known of that view; the hooks' scratch in HBM.
struct ViewHooks {
    hqscan::Scanner scan;
    bool valid = false; const void *ids = nullptr; uint64_t N = 0; uint32_t Q = 0, n_live = 0; bool rq_copy = false; std::vector<uint32_t> run_off, run_start, run_rank;
    DevBuf d_map, d_sel_task, d_sel_rank, d_rq, d_want;  // the selection's tables and output, the copy of the request column hqtick_debug_order_select marks, the ids hqtick_debug_order_rank_of looks up
    void release() { scan.release(); d_map.release(); d_sel_task.release(); d_sel_rank.release(); d_rq.release(); d_want.release(); }
};
}  // namespace

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
    PinBuf h_up, h_up2, h_q;
    hqcluster::WorkerSet ws;      // hqtick_cluster_* (ABI 5 and 7; cluster.h): the worker / request tables resident in HBM and their host mirror
    hqcluster::Retracting retr;   // hqtick_retracting_* (ABI 7): the table of Retracting tasks
    uint32_t last_row_groups = 0; // hqtick_cluster_last_row_groups
    bool wait_on_kernel = true;   // HQ_HIP_LAST; HQTICK_WAIT_ON_KERNEL=0: hipStreamSynchronize at every wait (A/B)
    bool defer_row_check = true;  // the coupled fast path's row check runs while phase C's kernels do; HQTICK_DEFER_ROW_CHECK=0: inside the solve (A/B)
    hqhost::Problem pb;
    // results (host)
    std::vector<uint32_t> b_rq, b_size, b_limit, b_cut_off, c_size, c_bl_off, bl_rq, bl_size; std::vector<uint8_t> b_lr, b_blk;
    std::vector<uint8_t> q_loaded;
    hqtick_kernel_stats stats{};
    uint32_t tpw_hint = 0;                            // HQTICK_TPW (tuning knob): tasks per wavefront slice
    uint32_t shard_index = 0, shard_count = 1;       // hqtick_set_shard
    void *sink = nullptr; size_t sink_bytes = 0;      // hqtick_set_record_sink (device memory)
    hqgraph::Graph graph;  // hqtick_graph_*: dependency counters + consumer lists in HBM
    hqasg::Ledger asg;     // hqtick_assigned_* (ABI 12; ledger.h)
    PinBuf h_cancel_ids; DevBuf d_cancel_ids; uint64_t cancel_ready_removed = 0;  // hqtick_cancel_tasks: the ids' staging and their one device copy; hqtick_cancel_last_ready_removed
    PinBuf h_finish_in; DevBuf d_finish_in;  // hqtick_finish_tasks: ids and reporting workers, 12 B per position, staged once and copied to the device once
    hqtick_ctx *qctx = nullptr;  // hqtick_query's private sub-context
    ViewHooks *view_hooks = nullptr;  // hqtick_debug_order_view's scanner and scratch (test library only), allocated on first use; nothing of it is touched on a tick's path
    uint32_t tick_seq = 0;  // the tick counter: moves the block solvers' sample window from tick to tick (host_model.h: Problem::tick_seq)
    double tl[32] = {}; int ntl = 0;  // debug timeline (us since tick start), hqtick_timeline()
    hqaudit::Auditor audit;  // hqtick_resident_check (audit.h): nothing of it exists until the first call
    bool check_resident = false; int audit_depth = 0;  // HQTICK_CHECK_RESIDENT=1: the audit behind every call that changes resident state (audit_depth: inside such a call)
};

namespace {

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

int fail(hqtick_ctx *ctx, int code, const std::string &msg) { ctx->err = msg; return code; }

#ifdef HQTICK_TEST_HOOKS
// duration between two dispatch events in us, or -1 when the pair was not recorded (hqtick_time_kernel's calibration; the runtime's error state is cleared)
double elapsed_us(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, a, b) == hipSuccess) return (double)ms * 1000.0;
    (void)hipGetLastError();
    return -1.0;
}
#endif

int validate(hqtick_ctx *ctx, const hqtick_snapshot *s, bool need_tasks) {
    if (!s) return fail(ctx, HQTICK_E_INVALID, "null snapshot");
    if (s->n_workers && (!s->worker_id || !s->worker_total || !s->worker_free)) return fail(ctx, HQTICK_E_INVALID, "worker arrays missing");
    for (uint32_t w = 1; w < s->n_workers; w++) if (s->worker_id[w - 1] >= s->worker_id[w]) return fail(ctx, HQTICK_E_INVALID, "worker ids not ascending");
    if (s->n_requests && (!s->rq_variant_off || !s->variant_entry_off)) return fail(ctx, HQTICK_E_INVALID, "request arrays missing");
    for (uint32_t q = 0; q < s->n_requests; q++) {
        if (s->rq_variant_off[q + 1] <= s->rq_variant_off[q]) return fail(ctx, HQTICK_E_INVALID, "request without variants");
        if (s->rq_variant_off[q + 1] - s->rq_variant_off[q] > 32) return fail(ctx, HQTICK_E_INVALID, "more than 32 variants");
    }
    uint32_t nv = s->n_requests ? s->rq_variant_off[s->n_requests] : 0;
    for (uint32_t e = 0; e < (nv ? s->variant_entry_off[nv] : 0); e++) {
        if (s->entry_resource[e] >= s->n_resources) return fail(ctx, HQTICK_E_INVALID, "entry resource id out of range");
        if (s->entry_kind[e] == HQ_ENTRY_AMOUNT && s->entry_amount[e] == 0) return fail(ctx, HQTICK_E_INVALID, "zero amount request");
    }
    if (need_tasks && s->n_ready) {
        if (!s->task_id || !s->task_priority || !s->task_rq) return fail(ctx, HQTICK_E_INVALID, "ready-set columns missing");
        for (uint64_t i = 1; i < s->n_ready; i++) if (s->task_id[i - 1] >= s->task_id[i]) return fail(ctx, HQTICK_E_INVALID, "ready set not sorted by task id");
    }
    if (s->n_blocked && (!s->blocked_worker || !s->blocked_rq || !s->blocked_variant)) return fail(ctx, HQTICK_E_INVALID, "blocked arrays missing");
    for (uint32_t k = 0; k < s->n_blocked; k++) {
        if (s->blocked_worker[k] >= s->n_workers) return fail(ctx, HQTICK_E_INVALID, "blocked worker index");
        if (s->blocked_rq[k] >= s->n_requests) return fail(ctx, HQTICK_E_INVALID, "blocked request id out of range");
        if (s->blocked_variant[k] >= s->rq_variant_off[s->blocked_rq[k] + 1] - s->rq_variant_off[s->blocked_rq[k]]) return fail(ctx, HQTICK_E_INVALID, "blocked variant out of range");
    }
    if (s->worker_group) for (uint32_t w = 0; w < s->n_workers; w++) if (s->worker_group[w] >= (s->n_groups ? s->n_groups : 1)) return fail(ctx, HQTICK_E_INVALID, "worker_group >= n_groups");
    // CSR offsets: monotone, and their arrays present.  (The ENTRIES of assigned_* are checked where they are dereferenced — the gap rows of a
    // tick with priority cuts, host_model.cpp — so that the common tick does not pay a pass over every running task.)
    if (s->assigned_off) {
        for (uint32_t w = 0; w < s->n_workers; w++) if (s->assigned_off[w] > s->assigned_off[w + 1]) return fail(ctx, HQTICK_E_INVALID, "assigned_off not monotone");
        if (s->n_workers && s->assigned_off[s->n_workers] && (!s->assigned_rq || !s->assigned_variant)) return fail(ctx, HQTICK_E_INVALID, "assigned arrays missing");
    }
    if (s->prefilled_off) {
        for (uint32_t w = 0; w < s->n_workers; w++) if (s->prefilled_off[w] > s->prefilled_off[w + 1]) return fail(ctx, HQTICK_E_INVALID, "prefilled_off not monotone");
        if (s->n_workers && s->prefilled_off[s->n_workers] && !s->prefilled_rq) return fail(ctx, HQTICK_E_INVALID, "prefilled_rq missing");
    }
    if (s->prefill_off) {
        for (uint32_t q = 0; q < s->n_requests; q++) if (s->prefill_off[q] > s->prefill_off[q + 1]) return fail(ctx, HQTICK_E_INVALID, "prefill_off not monotone");
        const uint32_t np = s->n_requests ? s->prefill_off[s->n_requests] : 0;
        if (np && (!s->prefill_priority || !s->prefill_task || !s->prefill_worker)) return fail(ctx, HQTICK_E_INVALID, "prefill arrays missing");
        for (uint32_t i = 0; i < np; i++) if (s->prefill_worker[i] >= s->n_workers) return fail(ctx, HQTICK_E_INVALID, "prefill worker index");
    }
    if (s->n_retracting && (!s->retracting_task || !s->retracting_worker)) return fail(ctx, HQTICK_E_INVALID, "retracting arrays missing");
    for (uint32_t k = 0; k < s->n_retracting; k++) {
        if (s->retracting_worker[k] >= s->n_workers) return fail(ctx, HQTICK_E_INVALID, "retracting worker index");
        if (k && s->retracting_task[k - 1] >= s->retracting_task[k]) return fail(ctx, HQTICK_E_INVALID, "retracting tasks not ascending");
        if (s->retracting_redirect_worker && s->retracting_redirect_worker[k] != HQ_NO_WORKER && s->retracting_redirect_worker[k] >= s->n_workers) return fail(ctx, HQTICK_E_INVALID, "retracting redirect worker index");
    }
    return 0;
}

// Packs worker tables + request tables (cluster.h: TabLayout) into ONE pinned, device-mapped staging buffer that K2 reads in place (every byte
// crosses PCIe once per workgroup; no H2D copy command).
int upload_tables(hqtick_ctx *ctx, const hqtick_snapshot *s, uint32_t W, const uint64_t *total, const uint64_t *free_, const int64_t *rem, PinBuf &buf, UpView *uv) {
    const uint32_t R = s->n_resources;
    const hqcluster::TabLayout L = hqcluster::table_layout(s, W);
    if (hqk::worker_eval_lds(R, L.nv, L.ne) > 150 * 1024) return fail(ctx, HQTICK_E_CAPACITY, "request table + 32 worker rows exceed the 150 KiB the worker-evaluation kernel stages in LDS");
    if (!buf.ensure(L.bytes)) return fail(ctx, HQTICK_E_DEVICE, "allocating upload staging");
    unsigned char *h = buf.as<unsigned char>();
    hqcluster::pack_worker_rows(h, L, W, R, total, free_, rem);
    hqcluster::pack_request_tables(h, L, s);
    hqcluster::view_tables(buf.dev<unsigned char>(), L, uv);
    return 0;
}

// ... or from HBM, where a worker set is resident (hqcluster::WorkerSet::tables)
int cluster_fail(hqtick_ctx *ctx, int rc) { if (rc < 0) ctx->err = ctx->ws.err; return rc; }

// the ready set (hqready::ReadySet, ready.h): what it is given of the context (ev[11]: the completion event an append's dispatch carries), and its errors
hqready::Env ready_env(hqtick_ctx *ctx) { return hqready::Env{ctx->device, ctx->stream, ctx->ev[11], ctx->wait_on_kernel}; }
int ready_fail(hqtick_ctx *ctx, int rc) { if (rc < 0) ctx->err = ctx->ready.err; return rc; }

// K2 on a worker set, synchronous (used for the fake workers of hqtick_query); results land in pinned memory
int eval_workers_sync(hqtick_ctx *ctx, const hqtick_snapshot *s, uint32_t W, const uint64_t *total, const uint64_t *free_, const int64_t *rem, WorkerEval *out) {
    UpView uv; int rc;
    if ((rc = upload_tables(ctx, s, W, total, free_, rem, ctx->h_up2, &uv))) return rc;
    size_t n = (size_t)W * uv.rt.n_variants;
    if (!ctx->h_q.ensure(n * 5 + 64)) return fail(ctx, HQTICK_E_DEVICE, "hipHostMalloc query eval");
    out->tmc = ctx->h_q.as<uint32_t>(); out->flags = ctx->h_q.as<uint8_t>() + n * 4;
    if (n == 0) return 0;
    HQ_HIP(hqk::worker_eval(uv.total, uv.free_, uv.rem, W, s->n_resources, uv.rt, uv.n_entries, ctx->h_q.dev<uint8_t>() + n * 4, ctx->h_q.dev<uint32_t>(), ctx->stream));
    HQ_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

void fill_problem(hqhost::Problem &pb, const hqtick_snapshot *s, const hqtick_config &cfg, const WorkerEval &ev) {
    pb.R = s->n_resources; pb.n_groups = s->n_groups ? s->n_groups : 1; pb.time_limit_s = cfg.mip_time_limit_s; pb.certificate_only = (cfg.flags & HQTICK_FLAG_CERTIFICATE_ONLY) != 0;
    uint32_t nv = s->n_requests ? s->rq_variant_off[s->n_requests] : 0;
    pb.rqs.resize(s->n_requests); pb.variants.resize(nv);
    for (uint32_t q = 0; q < s->n_requests; q++) pb.rqs[q] = {s->rq_variant_off[q], s->rq_variant_off[q + 1] - s->rq_variant_off[q]};
    for (uint32_t v = 0; v < nv; v++) {
        uint32_t e0 = s->variant_entry_off[v];
        pb.variants[v] = {s->entry_resource + e0, s->entry_kind + e0, s->entry_amount + e0, s->variant_entry_off[v + 1] - e0,
                          s->variant_n_nodes ? s->variant_n_nodes[v] : 0, s->variant_weight ? s->variant_weight[v] : 10000,
                          s->variant_min_time_ns ? s->variant_min_time_ns[v] : 0};
    }
    hqhost::WorkerSet &ws = pb.real;
    ws.n = s->n_workers; ws.R = s->n_resources; ws.id = s->worker_id; ws.total = s->worker_total; ws.free_ = s->worker_free;
    ws.remaining_ns = s->worker_remaining_ns; ws.min_util = s->worker_min_utilization; ws.flags = s->worker_flags; ws.group = s->worker_group;
    ws.vflags = ev.flags; ws.vtmc = ev.tmc; ws.n_variant_slots = nv;
    if (ws.blocked.size() != ws.n || ws.n_blocked_lists) { ws.blocked.assign(ws.n, {}); ws.n_blocked_lists = 0; }  // (4096 empty lists re-made per tick cost more than the batches stage)
    ws.assigned_off = s->assigned_off; ws.assigned_rq = s->assigned_rq; ws.assigned_variant = s->assigned_variant;
    ws.agg_off = nullptr; ws.agg_rq = nullptr; ws.agg_cnt = nullptr; ws.agg_variant = nullptr;
    for (uint32_t k = 0; k < s->n_blocked; k++) ws.blocked[s->blocked_worker[k]].push_back({s->blocked_rq[k], s->blocked_variant[k]});
    ws.n_blocked_lists = s->n_blocked;
    hqhost::group_equal_rows(ws, false);  // needs nothing of K2's output: in a tick this runs while the GPU works on phase A
}

void export_batches(hqtick_ctx *ctx, const std::vector<hqhost::TaskBatch> &batches, hqtick_result *out) {
    ctx->b_rq.clear(); ctx->b_size.clear(); ctx->b_limit.clear(); ctx->b_lr.clear(); ctx->b_blk.clear();
    ctx->b_cut_off.assign(1, 0); ctx->c_size.clear(); ctx->c_bl_off.assign(1, 0); ctx->bl_rq.clear(); ctx->bl_size.clear();
    for (auto &b : batches) {
        ctx->b_rq.push_back(b.rq); ctx->b_size.push_back(b.size); ctx->b_limit.push_back(b.limit); ctx->b_lr.push_back(b.limit_reached); ctx->b_blk.push_back(b.is_blocker);
        for (auto &c : b.cuts) {
            ctx->c_size.push_back(c.size);
            for (auto &bl : c.blockers) { ctx->bl_rq.push_back(bl.first); ctx->bl_size.push_back(bl.second); }
            ctx->c_bl_off.push_back((uint32_t)ctx->bl_rq.size());
        }
        ctx->b_cut_off.push_back((uint32_t)ctx->c_size.size());
    }
    out->n_batches = (uint32_t)ctx->b_rq.size(); out->batch_rq = ctx->b_rq.data(); out->batch_size = ctx->b_size.data(); out->batch_limit = ctx->b_limit.data();
    out->batch_limit_reached = ctx->b_lr.data(); out->batch_is_blocker = ctx->b_blk.data(); out->batch_cut_off = ctx->b_cut_off.data();
    out->cut_size = ctx->c_size.data(); out->cut_blocker_off = ctx->c_bl_off.data(); out->blocker_rq = ctx->bl_rq.data(); out->blocker_size = ctx->bl_size.data();
}

// GPU phase A (hqscan::Scanner, scan.h): what it is given of the context (ev[0] / ev[1] around K0, ev[2] / ev[3] around K1, ev[8] K1b's completion, ev[12] / ev[13]
// around the kernels of the ordered view), and its errors
hqscan::Env scan_env(hqtick_ctx *ctx) {
    return hqscan::Env{ctx->stream, ctx->stream2, ctx->ev[0], ctx->ev[1], ctx->ev[2], ctx->ev[3], ctx->ev[8], ctx->ev[12], ctx->ev[13],
                       ctx->timing, ctx->timing_k1, ctx->wait_on_kernel, ctx->k2_on_hist, ctx->k2_own_stream, ctx->tpw_hint};
}
int scan_fail(hqtick_ctx *ctx, int rc) { if (rc < 0) ctx->err = ctx->scan.err; return rc; }

// K2's tables for the scanner: from HBM where a worker set is resident, else packed from the snapshot
struct TablesOf { hqtick_ctx *ctx; const hqtick_snapshot *s; };
int worker_tables(void *user, UpView *uv, std::string *err) {
    hqtick_ctx *ctx = static_cast<TablesOf *>(user)->ctx; const hqtick_snapshot *s = static_cast<TablesOf *>(user)->s;
    const int rc = ctx->ws.valid() ? cluster_fail(ctx, ctx->ws.tables(ctx->stream, s, s->n_workers, uv))
                                   : upload_tables(ctx, s, s->n_workers, s->worker_total, s->worker_free, s->worker_remaining_ns, ctx->h_up, uv);
    if (rc) *err = ctx->err;
    return rc;
}

// K2 on the real workers and the scan of ctx->ready's columns; `while_gpu_runs` (may be null): hqscan::Scanner::scan
int phase_a(hqtick_ctx *ctx, const hqtick_snapshot *s, WorkerEval *ev, Scan *sc, const std::function<void()> *while_gpu_runs = nullptr) {
    TablesOf t{ctx, s};
    const uint32_t W = s->n_workers, Q = s->n_requests;
    const int rc = ctx->scan.scan(scan_env(ctx), ctx->ready.cols(), hqscan::Shape{Q, s->n_retracting, s->retracting_task},
                                  hqscan::Workers{W, s->n_resources, (size_t)W * (Q ? s->rq_variant_off[Q] : 0), worker_tables, &t}, ev, sc, while_gpu_runs);
    const hqscan::Timings &tm = ctx->scan.timings();
    if (tm.distinct_us >= 0) ctx->stats.distinct_us = tm.distinct_us;
    if (tm.level_hist_us >= 0) ctx->stats.level_hist_us = tm.level_hist_us;
    if (tm.scan_us >= 0) ctx->stats.scan_us = tm.scan_us;
    return scan_fail(ctx, rc);
}

// TaskQueue::iter_priority_sizes (taskqueue.rs:273-302) for every request, from the histogram and the prefill sets
std::vector<hqhost::QueueLevels> queue_levels(const Scan &sc, const hqtick_snapshot *s) {
    std::vector<hqhost::QueueLevels> qs(s->n_requests);
    for (uint32_t q = 0; q < s->n_requests; q++) {
        auto &lv = qs[q].levels;
        for (uint32_t r = sc.run_off[q]; r < sc.run_off[q + 1]; r++) lv.push_back({sc.run_prio[r], sc.run_cnt[r]});
        uint32_t pfn = s->prefill_off ? s->prefill_off[q + 1] - s->prefill_off[q] : 0;
        if (pfn) {
            uint64_t pp = s->prefill_priority[q];
            if (!lv.empty() && lv[0].first == pp) lv[0].second += pfn; else lv.insert(lv.begin(), {pp, pfn});
        }
    }
    return qs;
}

// The placement (hqsolve::Solver, solve.h): what it is given of the context (ev[9] / ev[10] around k_block_solve — ev[10] is its completion, which the host waits
// on), and its errors
hqsolve::Env solve_env(hqtick_ctx *ctx) { return hqsolve::Env{ctx->device, ctx->stream, ctx->ev[9], ctx->ev[10], ctx->timing, ctx->wait_on_kernel, ctx->shard_index, ctx->shard_count}; }
int solver_fail(hqtick_ctx *ctx, int rc) { if (rc < 0) ctx->err = ctx->solver.err; return rc; }
bool is_replica(hqtick_ctx *ctx) { return ctx->solver.replica(solve_env(ctx)); }  // others read this context's sweeps or records (a record sink alone is one scheduler's output path)

// The mapping (hqmap::Mapper, map.h): what it is given of the context (ev[4] / ev[5] around K4, ev[1] / ev[6] around K5a, ev[7] / ev[11] around K5b — ev[11] is K5b's
// completion, which the host waits on), and its errors
hqmap::Env map_env(hqtick_ctx *ctx, double t0 = 0) {
    return hqmap::Env{ctx->stream, ctx->ev[4], ctx->ev[5], ctx->ev[1], ctx->ev[6], ctx->ev[7], ctx->ev[11], ctx->timing, ctx->wait_on_kernel, ctx->cfg.flags,
                      ctx->sink, ctx->sink_bytes, ctx->shard_index, ctx->shard_count, hqmap::Timeline{t0, ctx->tl, &ctx->ntl}};
}
int map_fail(hqtick_ctx *ctx, int rc) { if (rc < 0) ctx->err = ctx->map.err; return rc; }
bool transpose_enabled() { const char *e = getenv("HQTICK_TRANSPOSE"); return !(e && atoi(e) == 0); }

// One tick, stage by stage: run() is the only entry point and mirrors run_scheduling_inner (scheduler/main.rs:50-72).  The plan's stages are map_core.h's, on the
// mapper's plan (no per-tick allocation in the steady state); phase C is the mapper's.
struct TickRun {
    hqtick_ctx *ctx; const hqtick_snapshot *s; hqtick_result *out; const bool use_resident;
    hqmap::Plan &ps; hqhost::Problem &pb;
    const uint32_t W, R, Q;
    WorkerEval ev; Scan sc; hqhost::Counts cnt;
    uint64_t N = 0; int status = HQTICK_DONE;
    double t0 = 0;

    TickRun(hqtick_ctx *c, const hqtick_snapshot *snap, hqtick_result *o, bool resident)
        : ctx(c), s(snap), out(o), use_resident(resident), ps(c->map.plan), pb(c->pb), W(snap->n_workers), R(snap->n_resources), Q(snap->n_requests) {}

    void mark() { hqmap::Timeline{t0, ctx->tl, &ctx->ntl}.mark(); }
    int plan_fail(int rc, const char *why) { if (rc) ctx->err = why; return rc; }

    // the ready set: uploaded with the snapshot, or already resident
    int load_ready_set() {
        if (!use_resident) {
            if (int rc = ready_fail(ctx, ctx->ready.load(ctx->stream, s, true))) return rc;
            ctx->scan.columns_changed();
        } else if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "hqtick_run_resident without hqtick_upload_ready");
        N = ctx->ready.cols().n;
        return 0;
    }

    // what the plan reads (map_core.h): the scan, the counts, the snapshot, and of the context plain values
    hqmap::PlanIn plan_in() {
        hqmap::PlanIn in{};
        in.sc = &sc; in.cnt = &cnt; in.s = s; in.rqs = pb.rqs.data(); in.variants = pb.variants.data();
        in.proactive_filling_reserve = ctx->cfg.proactive_filling_reserve; in.proactive_filling_max = ctx->cfg.proactive_filling_max; in.flags = ctx->cfg.flags;
        in.sink = ctx->sink != nullptr; in.shard_index = ctx->shard_index; in.shard_count = ctx->shard_count;
        in.N = N; in.retr_key = ctx->scan.retracting_keys(); in.retr_rank = ctx->scan.retracting_ranks();
        if (ctx->asg.on && ctx->asg.tracking()) {  // the ledger's prefilled counts (its sync_mirror brought them back; a snapshot with prefilled_off was refused)
            uint32_t pf_stride = 0;
            const std::vector<uint32_t> &h_pf = ctx->asg.prefilled_host(&pf_stride);
            if (h_pf.size() >= (size_t)W * pf_stride) { in.ledger_pf = h_pf.data(); in.ledger_pf_stride = pf_stride; }
        }
        in.transpose_on = transpose_enabled();
        in.storage = hqmap::Mapper::plan_storage; in.user = &ctx->map;  // the big tables are built in the pinned buffer K4's ride-along workgroups copy from
        return in;
    }

    // GPU phase C (hqmap::Mapper::phase_c), with what the assignment ledger needs of it
    int phase_c(const hqmap::Env &me, const hqmap::PlanIn &in, const std::function<void()> *while_gpu_runs) {
        hqmap::PhaseC pc{};
        pc.sc = &sc; pc.scan = &ctx->scan; pc.ready = &ctx->ready; pc.in = &in; pc.while_gpu_runs = while_gpu_runs;
        pc.consume_in_tick = use_resident && (ctx->cfg.flags & HQTICK_FLAG_CONSUME_IN_TICK) != 0;
        pc.ledger_pfq_rq = ctx->asg.on;
        if (ps.n_sel && pc.consume_in_tick && ctx->asg.on && s->n_retracting) {  // the redirects of Retracting tasks look their request id up after K4 has tombstoned it
            pc.saved_rq = ctx->asg.saved_rq(N);
            if (!pc.saved_rq) return fail(ctx, HQTICK_E_DEVICE, "hipMalloc ledger request ids");
        }
        if (ps.n_sel && ctx->asg.on && ps.n_rec) {  // the ledger's copy of the placement stays in HBM, whatever form the records leave in
            hqasg::StageCols c{};
            if (!ctx->asg.stage_for(ps.n_rec, sc.ordered, sc.L, &c)) return fail(ctx, HQTICK_E_DEVICE, "hipMalloc ledger staging");
            pc.stage = hqk::Stage{c.task, c.rq, c.row, c.level, c.meta};
        }
        const int rc = map_fail(ctx, ctx->map.phase_c(me, pc));
        const hqmap::Timings &tm = ctx->map.timings();
        if (tm.select_us >= 0) ctx->stats.select_us = tm.select_us;
        if (tm.sweep_us >= 0) ctx->stats.sweep_us = tm.sweep_us;
        if (tm.other_us >= 0) ctx->stats.other_us = tm.other_us;
        return rc;
    }

    // The fast path's row check may move into phase C's window only where a discarded phase C leaves no trace: no tombstones written by K4, no
    // ledger staging, no record sink, no replica whose sweeps or records others read, no Retracting task whose redirect is planned from the selection.
    bool may_defer_row_check() const {
        const int sw = hqmilp::g_check_hook ? hqmilp::g_check_hook->allow : -1;
        if (!(sw < 0 ? ctx->defer_row_check : sw != 0)) return false;
        if (use_resident && (ctx->cfg.flags & HQTICK_FLAG_CONSUME_IN_TICK)) return false;
        if (ctx->asg.on || ctx->sink || is_replica(ctx)) return false;
        return s->n_retracting == 0;
    }

    void finish(const hqmap::Env &me, double t1, double t2, double t3) {
        out->status = status;
        ctx->map.export_result(me, cnt, out);
        mark();  // 9: result assembled
        double t5 = now_us();
        out->t_total_us = t5 - t0; out->t_scan_us = t1 - t0; out->t_batches_us = t2 - t1; out->t_solve_us = t3 - t2; out->t_mapping_us = t5 - t3;
        uint64_t n_pref = 0; for (uint32_t q = 0; q < Q; q++) n_pref += ps.new_pf_total[q];
        uint64_t n_asg = 0; for (uint32_t w = 0; w < W; w++) n_asg += ps.n_assign[w];
        uint32_t nv = Q ? s->rq_variant_off[Q] : 0;
        ctx->stats.n_assigned = n_asg; ctx->stats.n_prefilled = n_pref;
        ctx->stats.algorithmic_bytes = N * 20 + (uint64_t)W * R * 16 + (uint64_t)nv * R * 9 + n_asg * 13 + n_pref * 12;
        ctx->stats.tick_gpu_us = ctx->stats.distinct_us + ctx->stats.level_hist_us + ctx->stats.scan_us + ctx->stats.block_solve_us + ctx->stats.select_us + ctx->stats.sweep_us + ctx->stats.other_us;
    }

    int run() {
        t0 = now_us();
        ctx->ntl = 0;
        if (ctx->cfg.flags & HQTICK_FLAG_NO_TICK_CACHES) { ctx->scan.columns_changed(); hqhost::flush_tick_caches(); }  // nothing derived survives from the last tick
        memset(out, 0, sizeof(*out));
        ctx->stats = hqtick_kernel_stats{};
        int rc = validate(ctx, s, !use_resident);
        if (rc) return rc;
        HQ_HIP(hipSetDevice(ctx->device));
        if ((rc = load_ready_set())) return rc;
        // ---------------- GPU phase A ----------------
        const std::function<void()> prep = [&]() {   // request/worker views: no GPU output needed yet
            fill_problem(pb, s, ctx->cfg, ev);
            ctx->last_row_groups = (uint32_t)pb.real.rows.rep.size();
            if (ctx->asg.on && !s->assigned_off) {  // the ledger's per-worker (rq, variant) counts
                const hqasg::Agg g = ctx->asg.agg();
                pb.real.agg_off = g.off; pb.real.agg_rq = g.rq; pb.real.agg_cnt = g.cnt; pb.real.agg_variant = g.var;
            }
            // HQTICK_FLAG_CERTIFICATE_ONLY is for ONE scheduler: replicas (a shard of several, a record sink that is merged with others', an exchange) must return the
            // canonical point — what the merge compares byte for byte — so the flag is ignored there (include/hqtick.h).
            if (pb.certificate_only && (is_replica(ctx) || ctx->sink)) pb.certificate_only = false;
        };
        if ((rc = phase_a(ctx, s, &ev, &sc, &prep))) return rc;
        mark();  // 0: phase A done
        const double t1 = now_us();
        // ---------------- host: batches + placement ----------------
        std::vector<hqhost::QueueLevels> qlv = queue_levels(sc, s);
        std::vector<hqhost::TaskBatch> batches = hqhost::create_task_batches(pb, qlv);
        export_batches(ctx, batches, out);
        mark();  // 1: batches
        const double t2 = now_us();
        // Solve, plan and phase C.  They run twice in one case only: the placement came from the fast path with its row check deferred into phase C's window (below)
        // and the check failed — then once more with the fast path off, which is what the inline check's failure leads to.
        const hqmap::Env me = map_env(ctx, t0);
        const uint32_t tick_seq = ctx->tick_seq++;
        const int ntl_solve = ctx->ntl;
        double t3 = t2;
        bool check_ok = true;
        const std::function<void()> check = [&]() { if (cnt.row_check_pending()) check_ok = cnt.settle_row_check(); };
        auto solve_plan_map = [&](bool defer, bool classic) -> int {
            int rc;
            hqsolve::Stats st;
            const bool use_memo = !(ctx->cfg.flags & (HQTICK_FLAG_NO_BLOCK_MEMO | HQTICK_FLAG_NO_TICK_CACHES));
            cnt = ctx->solver.solve(solve_env(ctx), pb, batches, hqsolve::Opts{defer, classic, tick_seq, use_memo}, &st);
            if (st.block_solve_us >= 0) ctx->stats.block_solve_us = st.block_solve_us;
            if (st.blocks_finished) ctx->stats.n_classes_device = st.n_classes_launched;
            ctx->stats.price_sweeps = (uint32_t)cnt.price_sweeps; ctx->stats.price_rounds = (uint32_t)cnt.price_rounds; ctx->stats.price_us = cnt.price_us; ctx->stats.milp_us = cnt.milp_us; ctx->stats.model_us = cnt.model_us; ctx->stats.solve_pre_us = cnt.pre_us;
            ctx->stats.price_sweep_us = st.price_sweep_us; ctx->stats.milp_cols = (uint32_t)cnt.milp_cols; ctx->stats.milp_rows = (uint32_t)cnt.milp_rows;
            ctx->stats.n_classes_verified = cnt.blocks_verified; ctx->stats.n_classes_mismatch = cnt.blocks_mismatch; ctx->stats.n_classes_rejected = cnt.blocks_rejected; ctx->stats.n_classes_memo = cnt.blocks_memo;
            ctx->stats.exchange_calls = st.exchange_calls; ctx->stats.exchange_bytes = st.exchange_bytes; ctx->stats.exchange_us = st.exchange_us;
            if (cnt.error) return fail(ctx, cnt.error, cnt.errmsg);
            ctx->stats.n_classes_device = cnt.blocks_device; ctx->stats.n_classes_host = cnt.blocks_host; ctx->stats.block_steps_max = cnt.block_steps_max; ctx->stats.n_classes = cnt.n_classes;
            ctx->stats.solve_classify_us = cnt.t_classify_us; ctx->stats.solve_blocks_us = cnt.t_blocks_us; ctx->stats.solve_decode_us = cnt.t_decode_us;
            mark();  // 2: solve
            t3 = now_us();
            out->is_optimal = cnt.is_optimal;
            out->is_canonical = cnt.is_canonical && cnt.is_optimal;
            status = hqsolve::tick_status(cnt);
            // ---------------- host: mapping plan ----------------
            const hqmap::PlanIn in = plan_in();
            hqmap::HostResult &hr = ctx->map.res;
            const char *why = nullptr;
            ctx->ready.selection_void();  // the previous tick's plan is overwritten from here on: hqtick_ready_consume_last refers to THIS tick or to none (if it fails)
            if ((rc = plan_fail(hqmap::plan_keys(ps, hr, in, &why), why))) return rc;
            if ((rc = map_fail(ctx, ctx->map.launch_sweep_early(me)))) return rc;
            if ((rc = plan_fail(hqmap::plan_redirects(ps, hr, in, &why), why))) return rc;
            mark();  // 3: key tables + retracts
            if ((rc = plan_fail(hqmap::plan_prefill(ps, hr, in, &why), why))) return rc;
            mark();  // 4: prefill plan
            if ((rc = plan_fail(hqmap::plan_outputs(ps, hr, in, &why), why))) return rc;
            if ((rc = map_fail(ctx, ctx->map.check_capacity(sc.ordered)))) return rc;
            mark();  // 5: K5 tables
            // ---------------- GPU phase C ----------------
            return phase_c(me, in, defer && cnt.row_check_pending() ? &check : nullptr);
        };
        rc = solve_plan_map(may_defer_row_check(), false);
        check();  // (a pass that did not reach phase C's window: the check decides all the same whether its result, an error included, stands)
        if (!check_ok) {
            // What the inline check's failure leads to: the classic path's placement.  The discarded pass has left nothing but buffers the second one overwrites
            // (may_defer_row_check: no tombstones, no ledger staging, no sink) and the selection's launch state, which goes.
            HQ_HIP(hipStreamSynchronize(ctx->stream));
            ctx->ready.selection_void(); ctx->map.forget_selection();
            ctx->ntl = ntl_solve; cnt = hqhost::Counts();
            rc = solve_plan_map(false, true);
        }
        if (rc) return rc;
        mark();  // 8: phase C synced
        finish(me, t1, t2, t3);
        return status;
    }
};

// ---------------------------------------------------------------------------------------------- assignment ledger (ABI 12): what hqasg::Ledger (ledger.h) is given of the context
hqasg::Env ledger_env(hqtick_ctx *ctx) {
    const hqready::Cols c = ctx->ready.cols();
    return hqasg::Env{ctx->device, ctx->stream, ctx->ws.rows(), ctx->ws.W(), ctx->ws.R(), c.id, c.prio, c.rq, c.n,
                      ctx->scan.levels_dev(), &ctx->ws.ids(), ctx->ws.flags(), ctx->ws.free_rows()};
}
int ledger_fail(hqtick_ctx *ctx, int rc) { if (rc < 0) ctx->err = ctx->asg.err; return rc; }
// a placement waiting for hqtick_ready_consume_last is still live only while the tick's selection is: every ready-set delta that abandons the selection
// (an add, a remove, a compaction, a graph call, an upload) ends ready.selection_live() — and with it the placement is dropped too: Ledger::pending is read nowhere
// but here, so the ready set need not know the ledger to clear it
bool ledger_pending_live(hqtick_ctx *ctx) { return ctx->asg.pending_live(ctx->ready.selection_live()); }
int ledger_guard(hqtick_ctx *ctx) {
    if (ctx->asg.on && ledger_pending_live(ctx)) return fail(ctx, HQTICK_E_INVALID, "assignment ledger: the last tick's placement is pending (hqtick_ready_consume_last first)");
    return 0;
}

int run_tick(hqtick_ctx *ctx, const hqtick_snapshot *s, hqtick_result *out, bool use_resident) {
    hqtick_snapshot full;
    if (ctx->asg.on && s) {  // the assignment ledger (ABI 12) is the tick's only source of the running tasks
        if (is_replica(ctx)) return fail(ctx, HQTICK_E_UNSUPPORTED, "assignment ledger on a sharded or replica context");
        if (s->worker_id || !ctx->ws.valid()) return fail(ctx, HQTICK_E_INVALID, "assignment ledger on: the tick runs on the resident worker set (HQ_WORKERS_RESIDENT, no worker arrays)");
        if (s->assigned_off) return fail(ctx, HQTICK_E_INVALID, "assignment ledger on: the snapshot must not carry an assigned CSR as well");
        if (ctx->asg.tracking() && s->prefilled_off) return fail(ctx, HQTICK_E_INVALID, "prefilled tracking on: the snapshot must not carry a prefilled CSR as well");
        HQ_HIP(hipSetDevice(ctx->device));
        ctx->asg.abandon_tick();
        ctx->asg.take_requests(s);
        if (ctx->asg.tracking() && ctx->asg.max_variants() >= hqasg::PF_VARIANT) return fail(ctx, HQTICK_E_UNSUPPORTED, "prefilled tracking: a request has 254 or more variants");
        if (int rc = ctx->asg.sync_mirror(ledger_env(ctx))) return ledger_fail(ctx, rc);
    }
    if (s) {  // the worker side may live in the library (hqtick_cluster_*, ABI 7), and so may the Retracting tasks of the queues (hqtick_retracting_*)
        if (int rc = cluster_fail(ctx, ctx->ws.complete(s, &full))) return rc;
        s = &full;
    }
    const bool retr_resident = s && s->n_retracting == HQ_RETRACTING_RESIDENT;
    if (retr_resident) { if (int rc = ctx->retr.to_snapshot(s->worker_id, s->n_workers, &full)) return fail(ctx, rc, ctx->retr.err); }
    int rc;
    {
        TickRun run(ctx, s, out, use_resident);
        rc = run.run();
    }
    if (ctx->ready.unconfirmed()) {  // HQTICK_FLAG_CONSUME_IN_TICK: the selection has written its tombstones
        ctx->ready.confirm();
        if (rc < 0) {
            // ... and the tick did not come back (a record sink too small, a mapping capacity exceeded, a failed exchange: errors a host can recover from).  What it took
            // goes back.  Only if THAT fails is the set dropped and the host uploads it again.
            const std::string why = ctx->err;
            bool restored = false;
            const bool synced = hipStreamSynchronize(ctx->stream) == hipSuccess;
            if (synced && ctx->ready.selection_valid())  // the selection once more, giving the request ids back (hqmap::Mapper::replay_selection)
                restored = ctx->map.replay_selection(ctx->stream, hqmap::REPLAY_RESTORE, ctx->ready.cols(), ctx->scan, ctx->ready.selected_count(), &ctx->h_q) == 0;
            // nothing of this tick is left to consume; a restore gives the count back what the tick had subtracted when it launched the selection (the kernel may have run for any part of it)
            if (restored) ctx->ready.put_back(); else ctx->ready.lost();
            ctx->err = why;
            if (restored) ctx->err += " (HQTICK_FLAG_CONSUME_IN_TICK: what the tick had taken is back in the resident ready set)";
            else { ctx->err += " (HQTICK_FLAG_CONSUME_IN_TICK: the tick had already taken its tasks and they could not be put back; the resident ready set is dropped, upload it again)"; }
        }
    }
    if (rc >= 0 && retr_resident) ctx->retr.apply_tick(s->worker_id, s->n_workers, ctx->map.res.retract_off, ctx->map.res.retract_task, ctx->map.res.red_task, ctx->map.res.red_worker, ctx->map.res.red_variant, ctx->map.res.red_kind);
    if (rc >= 0 && ctx->asg.on) {  // the placement enters the ledger when it becomes state: now, or at hqtick_ready_consume_last in the two-call form
        const bool in_tick = use_resident && (ctx->cfg.flags & HQTICK_FLAG_CONSUME_IN_TICK) != 0;
        ctx->asg.collect_tick(s, out, ctx->map.res.new_free, ctx->map.res.mn_rq, in_tick && s->n_retracting != 0);  // (the column copy is taken only for the redirects of Retracting tasks)
        if (!use_resident || in_tick) {
            if (int r2 = ledger_fail(ctx, ctx->asg.apply_tick(ledger_env(ctx)))) {  // (the tick's tasks have left the ready set: without the placement the ledger is no longer the truth)
                ctx->asg.on = false; ctx->asg.pending = false;
                ctx->err += " (the assignment ledger is switched off: upload the worker set and enable it again)";
                return r2;
            }
        }
    }
    return rc;
}

}  // namespace

// HQTICK_CHECK_RESIDENT=1 (debug; read at hqtick_create like HQTICK_CHECK_CLUSTER): every successful call that changes resident state -- ready set, graph, ledger,
// cluster upload / drop and membership, b-levels, consume, a tick -- ends with the audit of READY | LEDGER | GRAPH, the parts that must hold after every single call (CROSS and STRICT hold only between
// whole handlers and are never run here).  A violation turns the call's answer into HQTICK_E_INVALID, with the invariant's name and witness in hqtick_last_error;
// what the call did stays done.  Calls the library makes on itself (a delta that ends in another) are audited once, when the outermost returns.
// Not audited: hqtick_cluster_update_workers (it stays asynchronous: the next audited call finds what it broke), hqtick_cluster_set_clock / _set_blocked and the
// hqtick_retracting_* calls (the deadlines, the blocked pairs and the Retracting table are in none of the three parts).
namespace {
struct AuditScope {  // inside a call that changes resident state
    hqtick_ctx *c;
    explicit AuditScope(hqtick_ctx *ctx) : c(ctx) { if (c) c->audit_depth++; }
    ~AuditScope() { if (c) c->audit_depth--; }
};
int audited(hqtick_ctx *ctx, int rc) {
    static const char *const names[HQ_INV_N] = {"HQ_INV_READY_ORDER", "HQ_INV_READY_COUNT", "HQ_INV_LEDGER_HASH", "HQ_INV_LEDGER_ENTRY", "HQ_INV_LEDGER_TOTALS", "HQ_INV_LEDGER_COUNTS",
                                                "HQ_INV_LEDGER_PREFILLED", "HQ_INV_LEDGER_FREE", "HQ_INV_LEDGER_MN", "HQ_INV_GRAPH_HASH", "HQ_INV_GRAPH_TOTALS", "HQ_INV_GRAPH_COUNTER",
                                                "HQ_INV_X_READY_ASSIGNED", "HQ_INV_X_READY_WAITING", "HQ_INV_X_RETRACTING", "HQ_INV_S_READY_UNKNOWN", "HQ_INV_S_ASSIGNED_WAITING",
                                                "HQ_INV_S_RELEASED_NOWHERE"};
    if (!ctx || !ctx->check_resident || ctx->audit_depth || rc < 0) return rc;
    hqtick_check_report rep;
    const int arc = hqtick_resident_check(ctx, HQ_CHECK_READY | HQ_CHECK_LEDGER | HQ_CHECK_GRAPH, &rep);
    if (arc <= 0) return arc < 0 ? arc : rc;
    std::string m = "HQTICK_CHECK_RESIDENT: the resident state is inconsistent after this call:";
    for (uint32_t k = 0; k < HQ_INV_N; k++)
        if (rep.count[k]) m += std::string(" ") + names[k] + " (" + std::to_string(rep.count[k]) + " violations, first key " + std::to_string(rep.first[k]) + ")";
    return fail(ctx, HQTICK_E_INVALID, m);
}
// the body of such a call: `return with_audit(ctx, [&]() -> int { ... });`
template <class F> int with_audit(hqtick_ctx *ctx, F &&body) {
    int rc;
    { AuditScope scope(ctx); rc = body(); }
    return audited(ctx, rc);
}
}  // namespace

// ================================================================================================ C ABI
extern "C" {

uint32_t hqtick_abi_version(void) { return HQTICK_ABI_VERSION; }
const char *hqtick_build_arch(void) { return "gfx950"; }

int hqtick_create(const hqtick_config *config, hqtick_ctx **out_ctx) {
    if (!config || !out_ctx || (config->abi_version != HQTICK_ABI_VERSION && config->abi_version != 10u && config->abi_version != 11u)) return HQTICK_E_INVALID;  // (11 and 12 added functions only: a config written for 10 is the same struct)
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || config->device_index < 0 || config->device_index >= n) return HQTICK_E_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, config->device_index) != hipSuccess) return HQTICK_E_NO_DEVICE;
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) return HQTICK_E_NO_DEVICE;  // kernels are built for gfx950 only
    if (hipSetDevice(config->device_index) != hipSuccess) return HQTICK_E_NO_DEVICE;
    hqtick_ctx *ctx = new hqtick_ctx();
    ctx->cfg = *config; ctx->device = config->device_index;
    ctx->timing = (config->flags & HQTICK_FLAG_NO_KERNEL_TIMING) == 0;
    if (const char *e = getenv("HQTICK_TPW")) { long v = atol(e); if (v >= 256 && v <= (1 << 20) && v % 256 == 0) ctx->tpw_hint = (uint32_t)v; }
    if (const char *e = getenv("HQTICK_CHECK_RESIDENT")) ctx->check_resident = atoi(e) != 0;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return HQTICK_E_DEVICE; }
    if (hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking) != hipSuccess) { hipStreamDestroy(ctx->stream); delete ctx; return HQTICK_E_DEVICE; }
    if (const char *e = getenv("HQTICK_K2_RIDE_ALONG")) { ctx->k2_own_stream = atoi(e) == 0; ctx->k2_on_hist = atoi(e) == 1; }
    if (const char *e = getenv("HQTICK_WAIT_ON_KERNEL")) ctx->wait_on_kernel = atoi(e) != 0;
    if (const char *e = getenv("HQTICK_DEFER_ROW_CHECK")) ctx->defer_row_check = atoi(e) != 0;
    if (ctx->solver.init(ctx->device, ctx->stream)) { delete ctx; return HQTICK_E_DEVICE; }
    if (ctx->ws.init()) { delete ctx; return HQTICK_E_DEVICE; }
    for (auto &e : ctx->ev) if (hipEventCreate(&e) != hipSuccess) { delete ctx; return HQTICK_E_DEVICE; }
    if (ctx->scan.init()) { delete ctx; return HQTICK_E_DEVICE; }
    *out_ctx = ctx;
    return 0;
}

void hqtick_destroy(hqtick_ctx *ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    if (ctx->stream2) hipStreamSynchronize(ctx->stream2);
    ctx->map.release();
    ctx->scan.release();
    ctx->ready.release();
    ctx->ws.release();
    if (ctx->qctx) { hqtick_destroy(ctx->qctx); ctx->qctx = nullptr; }
    if (ctx->view_hooks) { ctx->view_hooks->release(); delete ctx->view_hooks; ctx->view_hooks = nullptr; }
    hipSetDevice(ctx->device);
    ctx->solver.comm_destroy(ctx->device);
    ctx->solver.release();
    ctx->graph.release();
    ctx->asg.release_all();
    ctx->audit.release();
    ctx->h_up.release(); ctx->h_up2.release(); ctx->h_q.release();
    ctx->h_cancel_ids.release(); ctx->d_cancel_ids.release();
    ctx->h_finish_in.release(); ctx->d_finish_in.release();
    for (auto &e : ctx->ev) if (e) hipEventDestroy(e);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    if (ctx->stream2) hipStreamDestroy(ctx->stream2);
    delete ctx;
}

const char *hqtick_last_error(const hqtick_ctx *ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

int hqtick_run(hqtick_ctx *ctx, const hqtick_snapshot *snapshot, hqtick_result *out) { return with_audit(ctx, [&]() -> int {
    if (!ctx || !out) return HQTICK_E_INVALID;
    return run_tick(ctx, snapshot, out, false);
}); }

int hqtick_upload_ready(hqtick_ctx *ctx, uint64_t n, const uint64_t *task_id, const uint64_t *task_priority, const uint32_t *task_rq, int sorted) { return with_audit(ctx, [&]() -> int {
    if (!ctx) return HQTICK_E_INVALID;
    if (n && (!task_id || !task_priority || !task_rq)) return fail(ctx, HQTICK_E_INVALID, "null ready-set column");
    if (sorted) for (uint64_t i = 1; i < n; i++) if (task_id[i - 1] >= task_id[i]) return fail(ctx, HQTICK_E_INVALID, "ready set not sorted by task id");
    for (uint64_t i = 0; i < n; i++) if (task_rq[i] == 0xFFFFFFFFu) return fail(ctx, HQTICK_E_INVALID, "request id 0xFFFFFFFF is reserved");
    HQ_HIP(hipSetDevice(ctx->device));
    if (int rc = ready_fail(ctx, ctx->ready.upload(ready_env(ctx), n, task_id, task_priority, task_rq, sorted != 0))) return rc;
    ctx->scan.columns_changed();
    return 0;
}); }

int hqtick_run_resident(hqtick_ctx *ctx, const hqtick_snapshot *snapshot, hqtick_result *out) { return with_audit(ctx, [&]() -> int {
    if (!ctx || !out) return HQTICK_E_INVALID;
    return run_tick(ctx, snapshot, out, true);
}); }

// ---- the resident ready set's deltas (f1): arguments validated here, the operations are hqready::ReadySet's (ready.h) ----
uint64_t hqtick_ready_count(const hqtick_ctx *ctx) { return ctx && ctx->ready.resident() ? ctx->ready.live() : 0; }

int hqtick_ready_consume_last(hqtick_ctx *ctx) { return with_audit(ctx, [&]() -> int {
    if (!ctx) return HQTICK_E_INVALID;
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set");
    if (ledger_pending_live(ctx)) {  // the last tick's placement enters the assignment ledger (before the selection's request ids become tombstones)
        HQ_HIP(hipSetDevice(ctx->device));
        if (int rc = ledger_fail(ctx, ctx->asg.apply_tick(ledger_env(ctx)))) {
            ctx->asg.on = false;
            ctx->err += " (the assignment ledger is switched off: upload the worker set and enable it again)";
            return rc;
        }
    }
    if (!ctx->ready.selection_pending()) {  // nothing handed out since the last consume (or the tick consumed it itself: HQTICK_FLAG_CONSUME_IN_TICK)
        if (!ctx->ready.compact_due()) return 0;
        HQ_HIP(hipSetDevice(ctx->device));
        return ready_fail(ctx, ctx->ready.compact(ready_env(ctx)));
    }
    if (!ctx->ready.selection_valid()) return fail(ctx, HQTICK_E_INVALID, "hqtick_ready_consume_last needs a preceding hqtick_run_resident");
    HQ_HIP(hipSetDevice(ctx->device));
    // the selection of the last tick once more, writing tombstones instead of the selected ids (hqmap::Mapper::replay_selection)
    if (int rc = map_fail(ctx, ctx->map.replay_selection(ctx->stream, hqmap::REPLAY_TOMBSTONE, ctx->ready.cols(), ctx->scan, ctx->ready.selected_count()))) return rc;
    return ready_fail(ctx, ctx->ready.consumed(ready_env(ctx)));
}); }

int hqtick_ready_remove(hqtick_ctx *ctx, uint64_t n, const uint64_t *task_id) { return with_audit(ctx, [&]() -> int {
    if (!ctx || (n && !task_id)) return HQTICK_E_INVALID;
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set");
    if (n == 0 || ctx->ready.cols().n == 0) return 0;
    if (n > 0x7FFFFFFFull) return fail(ctx, HQTICK_E_CAPACITY, "more than 2^31 - 1 ids in one delta (the count of removed tasks is the int return value)");
    HQ_HIP(hipSetDevice(ctx->device));
    return ready_fail(ctx, ctx->ready.remove(ready_env(ctx), n, task_id));
}); }

// The batch of new ready tasks is staged in pinned memory (a pageable hipMemcpy of a few MB costs ~1 ms in page pinning).  The caller can write it there
// directly: hqtick_ready_add_stage hands out the three column pointers for n tasks, hqtick_ready_add_staged merges what was written (no copy on the host);
// hqtick_ready_add = stage + memcpy + merge for callers that have the columns elsewhere.
int hqtick_ready_add_stage(hqtick_ctx *ctx, uint64_t n, uint64_t **task_id, uint64_t **task_priority, uint32_t **task_rq) {
    if (!ctx || !task_id || !task_priority || !task_rq) return HQTICK_E_INVALID;
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set (hqtick_upload_ready with n = 0 creates an empty one)");
    if (n > 0xFFFFFFFFull) return fail(ctx, HQTICK_E_CAPACITY, "more than 2^32 ids in one delta");
    HQ_HIP(hipSetDevice(ctx->device));
    return ready_fail(ctx, ctx->ready.stage(n, task_id, task_priority, task_rq));
}

int hqtick_ready_add_staged(hqtick_ctx *ctx, uint64_t n) { return with_audit(ctx, [&]() -> int {
    if (!ctx) return HQTICK_E_INVALID;
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set (hqtick_upload_ready with n = 0 creates an empty one)");
    return ready_fail(ctx, ctx->ready.add_staged(ready_env(ctx), n));
}); }

int hqtick_ready_add_packed(hqtick_ctx *ctx, uint64_t n, uint32_t n_id_runs, const uint64_t *id_run_start, const uint32_t *id_run_len, const uint32_t *id_off, uint32_t n_prio_runs, const uint64_t *prio_run_value, const uint32_t *prio_run_len, const uint16_t *task_rq) { return with_audit(ctx, [&]() -> int {
    if (!ctx) return HQTICK_E_INVALID;
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set (hqtick_upload_ready with n = 0 creates an empty one)");
    if (n == 0) return 0;
    if (n > 0xFFFFFFFFull) return fail(ctx, HQTICK_E_CAPACITY, "more than 2^32 ids in one delta");
    if (!n_id_runs || !n_prio_runs || !id_run_start || !id_run_len || !prio_run_value || !prio_run_len || !task_rq) return fail(ctx, HQTICK_E_INVALID, "hqtick_ready_add_packed: null array");
    // the small run tables are checked here (a handful of entries); ids ascending across the whole batch, duplicates against the resident set and the reserved
    // request id are checked by the append / merge kernel, as for hqtick_ready_add
    uint64_t tot = 0; for (uint32_t r = 0; r < n_id_runs; r++) { if (!id_run_len[r]) return fail(ctx, HQTICK_E_INVALID, "hqtick_ready_add_packed: empty id run"); tot += id_run_len[r]; }
    if (tot != n) return fail(ctx, HQTICK_E_INVALID, "hqtick_ready_add_packed: the id runs do not add up to n");
    tot = 0; for (uint32_t r = 0; r < n_prio_runs; r++) { if (!prio_run_len[r]) return fail(ctx, HQTICK_E_INVALID, "hqtick_ready_add_packed: empty priority run"); tot += prio_run_len[r]; }
    if (tot != n) return fail(ctx, HQTICK_E_INVALID, "hqtick_ready_add_packed: the priority runs do not add up to n");
    HQ_HIP(hipSetDevice(ctx->device));
    return ready_fail(ctx, ctx->ready.add_packed(ready_env(ctx), n, n_id_runs, id_run_start, id_run_len, id_off, n_prio_runs, prio_run_value, prio_run_len, task_rq));
}); }

int hqtick_ready_add(hqtick_ctx *ctx, uint64_t n, const uint64_t *task_id, const uint64_t *task_priority, const uint32_t *task_rq) { return with_audit(ctx, [&]() -> int {
    if (!ctx || (n && (!task_id || !task_priority || !task_rq))) return HQTICK_E_INVALID;
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set (hqtick_upload_ready with n = 0 creates an empty one)");
    if (n == 0) return 0;
    uint64_t *hi = nullptr, *hp = nullptr; uint32_t *hq = nullptr;
    if (int rc = hqtick_ready_add_stage(ctx, n, &hi, &hp, &hq)) return rc;
    memcpy(hi, task_id, n * 8); memcpy(hp, task_priority, n * 8); memcpy(hq, task_rq, n * 4);
    return hqtick_ready_add_staged(ctx, n);
}); }

// ---------------------------------------------------------------------------------------------- dependency graph (f1)
namespace {
int graph_fail(hqtick_ctx *ctx, int rc) { ctx->err = ctx->graph.err; return rc; }
int graph_pre(hqtick_ctx *ctx) {
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set (hqtick_upload_ready with n = 0 creates an empty one)");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, HQTICK_E_DEVICE, "hipSetDevice");
    return 0;
}
}  // namespace

int hqtick_graph_add_tasks(hqtick_ctx *ctx, uint64_t n, const uint64_t *task_id, const uint64_t *task_priority, const uint32_t *task_rq, const uint32_t *dep_off, const uint64_t *dep_task_id) { return with_audit(ctx, [&]() -> int {
    if (!ctx || (n && (!task_id || !task_priority || !task_rq))) return HQTICK_E_INVALID;
    if (n && dep_off && dep_off[n] && !dep_task_id) return HQTICK_E_INVALID;
    if (int rc = graph_pre(ctx)) return rc;
    int r = ctx->graph.add(n, task_id, task_priority, task_rq, dep_off, dep_task_id, ctx->stream);
    if (r < 0) return graph_fail(ctx, r);
    if (r > 0) { if (int rc = ready_fail(ctx, ctx->ready.add_device(ready_env(ctx), ctx->graph.out_id(), ctx->graph.out_prio(), ctx->graph.out_rq(), (uint32_t)r))) return rc; }
    return r;
}); }

int hqtick_graph_finish(hqtick_ctx *ctx, uint64_t n, const uint64_t *task_id) { return with_audit(ctx, [&]() -> int {
    if (!ctx || (n && !task_id)) return HQTICK_E_INVALID;
    if (int rc = graph_pre(ctx)) return rc;
    int r = ctx->graph.finish(n, task_id, ctx->stream);
    // released consumers join the ready set even when the call reports ERR_NOT_READY: the graph itself is consistent
    const uint32_t rel = ctx->graph.n_out();
    if (rel) { if (int rc = ready_fail(ctx, ctx->ready.add_device(ready_env(ctx), ctx->graph.out_id(), ctx->graph.out_prio(), ctx->graph.out_rq(), rel))) return rc; }
    if (r < 0) return graph_fail(ctx, r);
    return r;
}); }

int hqtick_graph_remove(hqtick_ctx *ctx, uint64_t n, const uint64_t *task_id, int recursive) { return with_audit(ctx, [&]() -> int {
    if (!ctx || (n && !task_id)) return HQTICK_E_INVALID;
    if (int rc = graph_pre(ctx)) return rc;
    int r = ctx->graph.remove(n, task_id, recursive != 0, ctx->stream);
    if (r < 0) return graph_fail(ctx, r);
    if (r > 0 && ctx->ready.cols().n) {  // TaskQueue::remove for the ones that were ready  core.rs:227-231
        if (int rc = ready_fail(ctx, ctx->ready.remove_device(ready_env(ctx), ctx->graph.out_id(), (uint32_t)r)); rc < 0) return rc;
    }
    return r;
}); }

const uint64_t *hqtick_graph_last_ids(const hqtick_ctx *ctx, uint64_t *n) {
    if (!ctx) { if (n) *n = 0; return nullptr; }
    if (n) *n = ctx->graph.n_out();
    return ctx->graph.n_out() ? ctx->graph.out_id_host() : nullptr;
}

uint64_t hqtick_graph_last_unknown(const hqtick_ctx *ctx) { return ctx ? ctx->graph.n_unknown() : 0; }

int hqtick_graph_unfinished(hqtick_ctx *ctx, uint64_t n, const uint64_t *task_id, uint32_t *out) {
    if (!ctx || (n && (!task_id || !out))) return HQTICK_E_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, HQTICK_E_DEVICE, "hipSetDevice");
    int r = ctx->graph.unfinished(n, task_id, out, ctx->stream);
    return r < 0 ? graph_fail(ctx, r) : 0;
}

int hqtick_graph_blevel(hqtick_ctx *ctx, uint32_t flags, uint32_t *max_level, uint32_t *n_ready_updated) { return with_audit(ctx, [&]() -> int {
    if (!ctx) return HQTICK_E_INVALID;
    if (flags & ~(uint32_t)HQTICK_BLEVEL_UPDATE_READY) return fail(ctx, HQTICK_E_INVALID, "hqtick_graph_blevel: unknown flag");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, HQTICK_E_DEVICE, "hipSetDevice");
    const hqready::Cols cols = ctx->ready.cols();
    const bool upd = (flags & HQTICK_BLEVEL_UPDATE_READY) && ctx->ready.resident() && cols.n;
    int r = ctx->graph.blevel(max_level, upd ? cols.id : nullptr, upd ? cols.rq : nullptr, upd ? cols.prio : nullptr, upd ? cols.n : 0,
                              n_ready_updated, ctx->stream);
    if (r < 0) return graph_fail(ctx, r);
    // the ready set's priorities changed: the next tick rediscovers its levels.  A pending hqtick_ready_consume_last is left alone — its replay reads the group keys, the
    // per-slice counters and the plan of the last tick, none of which the priority rewrite touches.
    if (upd) ctx->scan.columns_changed();
    return r;
}); }

int hqtick_graph_priorities(hqtick_ctx *ctx, uint64_t n, const uint64_t *task_id, uint64_t *out) {
    if (!ctx || (n && (!task_id || !out))) return HQTICK_E_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, HQTICK_E_DEVICE, "hipSetDevice");
    int r = ctx->graph.priorities(n, task_id, out, ctx->stream);
    return r < 0 ? graph_fail(ctx, r) : 0;
}

int hqtick_graph_get_stats(const hqtick_ctx *ctx, hqtick_graph_stats *out) {
    if (!ctx || !out) return HQTICK_E_INVALID;
    hqgraph::Stats st = ctx->graph.stats();
    out->n_tasks = st.n_tasks; out->n_slots = st.n_slots; out->n_edges_live = st.n_edges_live; out->n_edges_pool = st.n_edges_pool; out->n_runs = st.n_runs;
    out->hash_capacity = st.hash_capacity; out->hash_tombstones = st.hash_tombstones; out->bytes_hbm = st.bytes_hbm; out->last_kernel_us = ctx->graph.last_kernel_us();
    return 0;
}

// ---- the resident worker set (row f1: the reactor's worker bookkeeping as deltas): arguments validated here, the operations are hqcluster::WorkerSet's
// and hqcluster::Retracting's (cluster.h), the ledger's steps (ledger.h) interleaved ----
int hqtick_cluster_upload(hqtick_ctx *ctx, const hqtick_snapshot *s) { return with_audit(ctx, [&]() -> int {
    if (!ctx || !s) return HQTICK_E_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, HQTICK_E_NO_DEVICE, "hipSetDevice failed");
    if (int rc = validate(ctx, s, false)) return rc;
    if (int rc = cluster_fail(ctx, ctx->ws.upload(ctx->stream, s))) return rc;
    ctx->asg.on = false; ctx->asg.pending = false;  // a new worker set: the ledger is enabled (seeded) again for it
    ctx->asg.take_requests(s);
    return 0;
}); }

// what opens every delta of the worker set: there is one
static int cluster_open(hqtick_ctx *ctx, const char *fn) {
    if (!ctx) return HQTICK_E_INVALID;
    if (!ctx->ws.valid()) return fail(ctx, HQTICK_E_INVALID, std::string(fn) + " without hqtick_cluster_upload");
    return 0;
}

int hqtick_cluster_update_workers(hqtick_ctx *ctx, uint32_t n, const uint32_t *worker_index, const uint64_t *free_rows, const int64_t *remaining_ns) {
    if (int rc = cluster_open(ctx, "hqtick_cluster_update_workers")) return rc;
    if (int rc = ledger_guard(ctx)) return rc;
    if (n == 0) return 0;
    if (!worker_index || !free_rows) return fail(ctx, HQTICK_E_INVALID, "hqtick_cluster_update_workers: null array");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, HQTICK_E_NO_DEVICE, "hipSetDevice failed");
    return cluster_fail(ctx, ctx->ws.update_rows(ctx->stream, n, worker_index, free_rows, remaining_ns));
}

int hqtick_cluster_drop(hqtick_ctx *ctx) { return with_audit(ctx, [&]() -> int {
    if (!ctx) return HQTICK_E_INVALID;
    ctx->ws.drop(); ctx->asg.on = false; ctx->asg.pending = false;
    return 0;
}); }

// Clock mode: the termination times stay with the worker set and a tick takes only the clock (hqcluster::WorkerSet::set_clock)
int hqtick_cluster_set_clock(hqtick_ctx *ctx, int64_t now_ns) {
    if (!ctx) return HQTICK_E_INVALID;
    if (is_replica(ctx)) return fail(ctx, HQTICK_E_UNSUPPORTED, "hqtick_cluster_set_clock: not on a sharded or replica context");
    if (int rc = cluster_open(ctx, "hqtick_cluster_set_clock")) return rc;
    if (int rc = ledger_guard(ctx)) return rc;
    return cluster_fail(ctx, ctx->ws.set_clock(now_ns));
}

int hqtick_cluster_deadlines(const hqtick_ctx *ctx, uint32_t *n_workers, const int64_t **deadline_ns) {
    if (!ctx || !ctx->ws.valid() || !ctx->ws.clock_mode()) return HQTICK_E_INVALID;
    if (n_workers) *n_workers = (uint32_t)ctx->ws.deadlines().size();
    if (deadline_ns) *deadline_ns = ctx->ws.deadlines().data();
    return 0;
}

uint32_t hqtick_cluster_last_row_groups(const hqtick_ctx *ctx) { return ctx ? ctx->last_row_groups : 0u; }

// Membership changes.  The order of the steps is load-bearing: the ledger's re-pack runs on an Env that already has the new worker count and still has the old mirror.
int hqtick_cluster_add_workers(hqtick_ctx *ctx, uint32_t n, const uint32_t *worker_id, const uint64_t *total_rows, const uint64_t *free_rows, const int64_t *remaining_ns, const float *min_utilization, const uint8_t *flags, const uint32_t *group) { return with_audit(ctx, [&]() -> int {
    if (int rc = cluster_open(ctx, "hqtick_cluster_add_workers")) return rc;
    if (n == 0) return 0;
    if (!worker_id || !total_rows || !free_rows) return fail(ctx, HQTICK_E_INVALID, "hqtick_cluster_add_workers: null array");
    const uint32_t W = ctx->ws.W();
    std::vector<uint32_t> src;
    if (int rc = cluster_fail(ctx, ctx->ws.plan_add(n, worker_id, group, &src))) return rc;
    if (int rc = ledger_guard(ctx)) return rc;
    HQ_HIP(hipSetDevice(ctx->device));
    if (int rc = cluster_fail(ctx, ctx->ws.repack(ctx->stream, src, n, total_rows, free_rows, remaining_ns))) return rc;
    if (ctx->asg.on) { if (int rc = ctx->asg.repack(ledger_env(ctx), src, W, flags)) return ledger_fail(ctx, rc); }
    ctx->ws.add_rows(n, worker_id, total_rows, free_rows, remaining_ns, min_utilization, flags, group);
    if (ctx->asg.on) return ledger_fail(ctx, ctx->asg.upload_wids(ledger_env(ctx)));
    return 0;
}); }

int hqtick_cluster_remove_workers(hqtick_ctx *ctx, uint32_t n, const uint32_t *worker_id) { return with_audit(ctx, [&]() -> int {
    if (int rc = cluster_open(ctx, "hqtick_cluster_remove_workers")) return rc;
    if (n == 0) return 0;
    if (!worker_id) return fail(ctx, HQTICK_E_INVALID, "hqtick_cluster_remove_workers: null array");
    const uint32_t W = ctx->ws.W();
    std::vector<uint32_t> src;
    if (int rc = cluster_fail(ctx, ctx->ws.plan_remove(n, worker_id, &src))) return rc;
    if (int rc = ledger_guard(ctx)) return rc;
    ctx->asg.clear_requeued();
    if (ctx->asg.on) { if (int rc = ctx->asg.evict(ledger_env(ctx), n, worker_id)) return ledger_fail(ctx, rc); }  // on_remove_worker: the lost workers' tasks leave the ledger (reactor.rs:64-147)
    HQ_HIP(hipSetDevice(ctx->device));
    if (int rc = cluster_fail(ctx, ctx->ws.repack(ctx->stream, src, 0, nullptr, nullptr, nullptr))) return rc;
    if (ctx->asg.on) { if (int rc = ctx->asg.repack(ledger_env(ctx), src, W, nullptr)) return ledger_fail(ctx, rc); }
    ctx->ws.keep_rows(src);
    ctx->retr.workers_removed(n, worker_id);
    if (ctx->asg.on) {
        if (int rc = ctx->asg.upload_wids(ledger_env(ctx))) return ledger_fail(ctx, rc);
        // ... and go back into the resident ready set with their priority and request (add_ready_task), ids ascending
        const hqasg::Ledger &a = ctx->asg;
        if (!a.rq_task.empty() && ctx->ready.resident()) {
            if (int rc = hqtick_ready_add(ctx, a.rq_task.size(), a.rq_task.data(), a.rq_prio.data(), a.rq_rq.data())) return rc;
        }
    }
    return 0;
}); }

int hqtick_cluster_last_reassigned(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id, const uint32_t **worker_id, const uint8_t **variant) {
    if (!ctx) return HQTICK_E_INVALID;
    ctx->retr.last.get(n, task_id, worker_id, variant);
    return 0;
}

int hqtick_cluster_set_blocked(hqtick_ctx *ctx, uint32_t worker_id, uint32_t n, const uint32_t *rq, const uint8_t *variant) {
    if (int rc = cluster_open(ctx, "hqtick_cluster_set_blocked")) return rc;
    return cluster_fail(ctx, ctx->ws.set_blocked(worker_id, n, rq, variant));
}

int hqtick_cluster_workers(const hqtick_ctx *ctx, uint32_t *n_workers, const uint32_t **worker_id) {
    if (!ctx || !ctx->ws.valid()) return HQTICK_E_INVALID;
    if (n_workers) *n_workers = ctx->ws.W();
    if (worker_id) *worker_id = ctx->ws.ids().data();
    return 0;
}

int hqtick_cluster_set_flags(hqtick_ctx *ctx, uint32_t n, const uint32_t *worker_id, const uint8_t *flags) { return with_audit(ctx, [&]() -> int {
    if (int rc = cluster_open(ctx, "hqtick_cluster_set_flags")) return rc;
    if (int rc = ledger_guard(ctx)) return rc;
    if (n == 0) return 0;
    if (!worker_id || !flags) return fail(ctx, HQTICK_E_INVALID, "hqtick_cluster_set_flags: null array");
    if (ctx->asg.on) {  // the ledger may have moved SN bits since the mirror was read
        if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, HQTICK_E_NO_DEVICE, "hipSetDevice failed");
        if (int rc = ctx->asg.sync_mirror(ledger_env(ctx))) return ledger_fail(ctx, rc);
    }
    if (int rc = cluster_fail(ctx, ctx->ws.set_flags(n, worker_id, flags, ctx->asg.on))) return rc;
    if (ctx->asg.on) return ledger_fail(ctx, ctx->asg.upload_flags(ledger_env(ctx)));
    return 0;
}); }

int hqtick_cluster_worker_flags(const hqtick_ctx *cctx, uint32_t *n_workers, const uint8_t **flags) {
    if (!cctx || !cctx->ws.valid()) return HQTICK_E_INVALID;
    hqtick_ctx *ctx = const_cast<hqtick_ctx *>(cctx);  // (the mirror is a cache of the ledger's column: reading it may refresh it)
    if (ctx->asg.on && ctx->asg.dirty()) {
        if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, HQTICK_E_NO_DEVICE, "hipSetDevice failed");
        if (int rc = ctx->asg.sync_mirror(ledger_env(ctx))) return ledger_fail(ctx, rc);
    }
    if (n_workers) *n_workers = ctx->ws.W();
    if (flags) *flags = ctx->ws.flags()->data();
    return 0;
}

int hqtick_retracting_add(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id) {
    if (!ctx) return HQTICK_E_INVALID;
    if (n && (!task_id || !worker_id)) return fail(ctx, HQTICK_E_INVALID, "hqtick_retracting_add: null array");
    ctx->retr.add(n, task_id, worker_id);
    return 0;
}

int hqtick_retract_response(hqtick_ctx *ctx, uint32_t worker_id, uint32_t n, const uint64_t *task_id, uint32_t *n_assigned, const uint64_t **assigned_task,
                            const uint32_t **assigned_worker_id, const uint8_t **assigned_variant) {
    if (!ctx) return HQTICK_E_INVALID;
    if (n && !task_id) return fail(ctx, HQTICK_E_INVALID, "hqtick_retract_response: null array");
    const int left = ctx->retr.response(worker_id, n, task_id);
    ctx->retr.last.get(n_assigned, assigned_task, assigned_worker_id, assigned_variant);
    return left;
}

uint32_t hqtick_retracting_count(const hqtick_ctx *ctx) { return ctx ? ctx->retr.count() : 0u; }

// ---- assignment ledger (ABI 12; include/hqtick.h): arguments validated here, the operations are hqasg::Ledger's (ledger.h) ----
int hqtick_assigned_enable(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id, const uint32_t *rq, const uint8_t *variant, const uint64_t *priority) { return with_audit(ctx, [&]() -> int {
    if (!ctx) return HQTICK_E_INVALID;
    if (is_replica(ctx)) return fail(ctx, HQTICK_E_UNSUPPORTED, "hqtick_assigned_enable: not on a sharded or replica context");
    if (!ctx->ws.valid()) return fail(ctx, HQTICK_E_INVALID, "hqtick_assigned_enable without a resident worker set (hqtick_cluster_upload)");
    if (n && (!task_id || !worker_id || !rq || !variant || !priority)) return fail(ctx, HQTICK_E_INVALID, "hqtick_assigned_enable: null array");
    HQ_HIP(hipSetDevice(ctx->device));
    return ledger_fail(ctx, ctx->asg.enable(ledger_env(ctx), n, task_id, worker_id, rq, variant, priority));
}); }

int hqtick_assigned_disable(hqtick_ctx *ctx) { return with_audit(ctx, [&]() -> int {
    if (!ctx) return HQTICK_E_INVALID;
    ctx->asg.on = false; ctx->asg.pending = false;
    return 0;
}); }

// what opens every ledger delta: the ledger is on (prefilled: and not a replica's; tracked: and tracks prefilled tasks), no placement is pending, the device is set,
// the arrays of a batch are there and the batch is one the kernels can index
static int ledger_open(hqtick_ctx *ctx, const char *fn, uint32_t n, bool arrays, bool prefilled = false, bool tracked = false) {
    if (!ctx) return HQTICK_E_INVALID;
    if (prefilled && is_replica(ctx)) return fail(ctx, HQTICK_E_UNSUPPORTED, std::string(fn) + ": not on a sharded or replica context");
    if (!ctx->asg.on) return fail(ctx, HQTICK_E_INVALID, "assignment ledger not enabled (hqtick_assigned_enable)");
    if (int rc = ledger_guard(ctx)) return rc;
    HQ_HIP(hipSetDevice(ctx->device));
    if (tracked && !ctx->asg.tracking()) return fail(ctx, HQTICK_E_INVALID, "prefilled tasks are not tracked (hqtick_assigned_track_prefilled)");
    if (n && !arrays) return fail(ctx, HQTICK_E_INVALID, std::string(fn) + ": null array");
    if (n > 0x7FFFFFFFu) return fail(ctx, HQTICK_E_CAPACITY, "more than 2^31 - 1 ids in one delta");
    return 0;
}

int hqtick_assigned_add(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id, const uint32_t *rq, const uint8_t *variant, const uint64_t *priority) { return with_audit(ctx, [&]() -> int {
    if (int rc = ledger_open(ctx, "hqtick_assigned_add", n, task_id && worker_id && rq && variant && priority)) return rc;
    return ledger_fail(ctx, ctx->asg.add(ledger_env(ctx), n, task_id, worker_id, rq, variant, priority));
}); }

int hqtick_assigned_release(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id) { return with_audit(ctx, [&]() -> int {
    if (int rc = ledger_open(ctx, "hqtick_assigned_release", n, task_id)) return rc;
    return ledger_fail(ctx, ctx->asg.release(ledger_env(ctx), n, task_id));
}); }

int hqtick_assigned_add_mn(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *rq, const uint64_t *priority, const uint32_t *worker_off, const uint32_t *worker_id) { return with_audit(ctx, [&]() -> int {
    if (int rc = ledger_open(ctx, "hqtick_assigned_add_mn", n, task_id && rq && priority && worker_off)) return rc;
    return ledger_fail(ctx, ctx->asg.add_mn(ledger_env(ctx), n, task_id, rq, priority, worker_off, worker_id));
}); }

uint64_t hqtick_assigned_mn_count(const hqtick_ctx *ctx) { return ctx && ctx->asg.on ? ctx->asg.mn_live : 0; }

int hqtick_assigned_mn_workers(hqtick_ctx *ctx, uint64_t task_id, uint32_t *n, const uint32_t **worker_id) {
    if (!ctx) return HQTICK_E_INVALID;
    if (!ctx->asg.on) return fail(ctx, HQTICK_E_INVALID, "assignment ledger not enabled (hqtick_assigned_enable)");
    return ledger_fail(ctx, ctx->asg.mn_workers(ledger_env(ctx), task_id, n, worker_id));
}

uint64_t hqtick_assigned_last_unknown(const hqtick_ctx *ctx) { return ctx ? ctx->asg.last_unknown : 0; }
uint64_t hqtick_assigned_last_host_bytes(const hqtick_ctx *ctx) { return ctx ? ctx->asg.last_host_bytes : 0; }
uint64_t hqtick_assigned_count(const hqtick_ctx *ctx) { return ctx && ctx->asg.on ? ctx->asg.n_live : 0; }

int hqtick_assigned_lookup(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, uint32_t *worker_id, uint8_t *variant) {
    if (!ctx) return HQTICK_E_INVALID;
    if (!ctx->asg.on) return fail(ctx, HQTICK_E_INVALID, "assignment ledger not enabled (hqtick_assigned_enable)");
    if (n && (!task_id || !worker_id || !variant)) return fail(ctx, HQTICK_E_INVALID, "hqtick_assigned_lookup: null array");
    if (!n) return 0;
    HQ_HIP(hipSetDevice(ctx->device));
    return ledger_fail(ctx, ctx->asg.lookup(ledger_env(ctx), n, task_id, worker_id, variant));
}

int hqtick_assigned_free_rows(hqtick_ctx *ctx, uint32_t *n_workers, const uint64_t **free_rows) {
    if (!ctx) return HQTICK_E_INVALID;
    if (!ctx->asg.on) return fail(ctx, HQTICK_E_INVALID, "assignment ledger not enabled (hqtick_assigned_enable)");
    HQ_HIP(hipSetDevice(ctx->device));
    if (int rc = ctx->asg.sync_mirror(ledger_env(ctx))) return ledger_fail(ctx, rc);
    if (n_workers) *n_workers = ctx->ws.W();
    if (free_rows) *free_rows = ctx->ws.free_rows()->data();
    return 0;
}

int hqtick_cluster_last_requeued(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id, const uint32_t **rq, const uint64_t **priority) {
    if (!ctx) return HQTICK_E_INVALID;
    if (n) *n = (uint32_t)ctx->asg.rq_task.size();
    if (task_id) *task_id = ctx->asg.rq_task.data();
    if (rq) *rq = ctx->asg.rq_rq.data();
    if (priority) *priority = ctx->asg.rq_prio.data();
    return 0;
}

int hqtick_cluster_last_requeued_prefilled(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id) {
    if (!ctx) return HQTICK_E_INVALID;
    if (n) *n = (uint32_t)ctx->asg.rq_pf_task.size();
    if (task_id) *task_id = ctx->asg.rq_pf_task.data();
    return 0;
}

// ---- prefilled tasks in the ledger (SingleNodeTaskAssignment::prefilled_tasks) ----
int hqtick_assigned_track_prefilled(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id, const uint32_t *rq, const uint64_t *priority) { return with_audit(ctx, [&]() -> int {
    if (int rc = ledger_open(ctx, "hqtick_assigned_track_prefilled", n, task_id && worker_id && rq && priority, true)) return rc;
    return ledger_fail(ctx, ctx->asg.track_prefilled(ledger_env(ctx), n, task_id, worker_id, rq, priority));
}); }

int hqtick_assigned_start_prefilled(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint8_t *variant) { return with_audit(ctx, [&]() -> int {
    if (int rc = ledger_open(ctx, "hqtick_assigned_start_prefilled", n, task_id && variant, true, true)) return rc;
    return ledger_fail(ctx, ctx->asg.start_prefilled(ledger_env(ctx), n, task_id, variant));
}); }

int hqtick_assigned_unprefill(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id) { return with_audit(ctx, [&]() -> int {
    if (int rc = ledger_open(ctx, "hqtick_assigned_unprefill", n, task_id, true, true)) return rc;
    return ledger_fail(ctx, ctx->asg.unprefill(ledger_env(ctx), n, task_id));
}); }

uint64_t hqtick_assigned_prefilled_count(const hqtick_ctx *ctx) { return ctx && ctx->asg.on && ctx->asg.tracking() ? ctx->asg.pf_live : 0; }

// ---- on_cancel_tasks in one call: the checks and the order of the steps are here, the steps are the graph's, the ready set's, the ledger's and the
// Retracting table's.  The ids are staged once in pinned memory and copied to the device once; every step reads that copy.
// What is left when a later step fails after an earlier one succeeded: the earlier ones stay done, as in hqtick_cluster_remove_workers.  After a failed ready-set
// step the closure has left the graph (hqtick_graph_last_ids names it) and hqtick_ready_remove of those ids finishes that part; after a failed ledger step the graph
// and the ready set are done and hqtick_assigned_release + hqtick_assigned_unprefill of the ids finish the ledger's (a failure behind the ledger's kernels has
// already taken the entries out and switched nothing off); the Retracting table is touched last and only after the ledger succeeded, so it never runs ahead of
// the ledger.  The lists of hqtick_cancel_last_* are empty after any failure.
int hqtick_cancel_tasks(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id) { return with_audit(ctx, [&]() -> int {
    if (!ctx) return HQTICK_E_INVALID;
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set");
    if (int rc = ledger_open(ctx, "hqtick_cancel_tasks", n, task_id)) return rc;  // (the guard comes before any step: a refused call changes nothing)
    ctx->asg.cancel_out = hqasg::Ledger::CancelOut{}; ctx->cancel_ready_removed = 0;
    if (n == 0) return 0;
    if (!ctx->h_cancel_ids.ensure((size_t)n * 8 + 8) || !ctx->d_cancel_ids.ensure((size_t)n * 8 + 8)) return fail(ctx, HQTICK_E_DEVICE, "hipMalloc cancel staging");
    memcpy(ctx->h_cancel_ids.p, task_id, (size_t)n * 8);
    HQ_HIP(hipMemcpyAsync(ctx->d_cancel_ids.p, ctx->h_cancel_ids.p, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    const uint64_t *d_ids = ctx->d_cancel_ids.as<uint64_t>();
    // 1 / 2: the graph's closure (remove_tasks_batched) and the ready set
    if (ctx->graph.resident()) {
        const int r = ctx->graph.remove_device(n, d_ids, true, ctx->stream);
        if (r < 0) return graph_fail(ctx, r);
        if (r > 0 && ctx->ready.cols().n) {
            const int k = ready_fail(ctx, ctx->ready.remove_device(ready_env(ctx), ctx->graph.out_id(), (uint32_t)r));
            if (k < 0) return k;
            ctx->cancel_ready_removed = (uint64_t)k;
        }
    } else if (ctx->ready.cols().n) {
        const int k = ready_fail(ctx, ctx->ready.remove_device(ready_env(ctx), d_ids, n));
        if (k < 0) return k;
        ctx->cancel_ready_removed = (uint64_t)k;
    }
    // 3: the ledger's entries, the routes and the messages; the Retracting table's (task, worker it is retracting from) pairs ride along as overrides
    std::vector<uint64_t> retr_id; std::vector<uint32_t> retr_wid;
    ctx->retr.sources(&retr_id, &retr_wid);
    const uint32_t *hit = nullptr;
    const int m = ledger_fail(ctx, ctx->asg.cancel(ledger_env(ctx), n, d_ids, (uint32_t)retr_id.size(), retr_id.data(), retr_wid.data(), &hit));
    if (m < 0) { ctx->asg.cancel_out = hqasg::Ledger::CancelOut{}; return m; }
    // 4: try_remove_redirection's other half: the listed tasks leave the Retracting table
    for (size_t k = 0; hit && k < retr_id.size(); k++) if (hit[k] != hqasg::NONE) ctx->retr.cancel(retr_id[k]);
    return m;
}); }

int hqtick_cancel_last_messages(const hqtick_ctx *ctx, uint32_t *n_workers, const uint32_t **worker_id, const uint32_t **task_off, const uint64_t **task_id) {
    static const uint32_t zero_off[1] = {0};
    if (!ctx) { if (n_workers) *n_workers = 0; if (worker_id) *worker_id = nullptr; if (task_off) *task_off = nullptr; if (task_id) *task_id = nullptr; return HQTICK_E_INVALID; }
    const hqasg::Ledger::CancelOut &o = ctx->asg.cancel_out;
    if (n_workers) *n_workers = o.n_workers;
    if (worker_id) *worker_id = o.worker_id;
    if (task_off) *task_off = o.task_off ? o.task_off : zero_off;
    if (task_id) *task_id = o.task_id;
    return 0;
}

int hqtick_cancel_last_routes(const hqtick_ctx *ctx, uint32_t *n, const uint32_t **worker_id, const uint8_t **kind) {
    if (!ctx) { if (n) *n = 0; if (worker_id) *worker_id = nullptr; if (kind) *kind = nullptr; return HQTICK_E_INVALID; }
    const hqasg::Ledger::CancelOut &o = ctx->asg.cancel_out;
    if (n) *n = o.n;
    if (worker_id) *worker_id = o.route_wid;
    if (kind) *kind = o.route_kind;
    return 0;
}

uint64_t hqtick_cancel_last_ready_removed(const hqtick_ctx *ctx) { return ctx ? ctx->cancel_ready_removed : 0; }

// ---- task_finished in one call: the checks and the order of the steps are here, the steps are the ledger's, the Retracting table's, the graph's and
// the ready set's.  Ids and reporting workers are staged once in pinned memory (12 B per position) and copied to the device once; every step reads that copy.
// What is left when a later step fails after an earlier one succeeded: the earlier ones stay done.  After a failed ledger step behind its kernels the accepted
// entries have left the table and hqtick_finish_last_routes is empty; nothing else was touched, and hqtick_assigned_release of the ids + hqtick_graph_finish finish
// the job for the ids a host knows to be rightly reported.  After a failed ready-set removal of an in-queue Retracting id (the table step) the ledger and the table
// are done: hqtick_ready_remove of those ids and hqtick_graph_finish of the accepted ids (hqtick_finish_last_routes names them) finish it.  After a failed graph
// step the ledger and the table are done and hqtick_graph_finish of the accepted ids finishes it; after a failed ready-set add the graph has released the
// consumers (hqtick_graph_last_ids names them) and hqtick_ready_add of those finishes it.  A finished task that still had dependencies (HQTICK_E_INVALID from
// the graph) leaves every step done, its consumers in the ready set included, as hqtick_graph_finish does.
int hqtick_finish_tasks(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id) { return with_audit(ctx, [&]() -> int {
    if (!ctx) return HQTICK_E_INVALID;
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set");
    if (int rc = ledger_open(ctx, "hqtick_finish_tasks", n, task_id && worker_id)) return rc;  // (the guard comes before any step: a refused call changes nothing)
    if (n > 0x03FFFFFFu) return fail(ctx, HQTICK_E_CAPACITY, "more than 2^26 finished tasks in one batch");
    ctx->asg.finish_out = hqasg::Ledger::FinishOut{}; ctx->asg.last_unknown = 0;
    if (n == 0) return 0;
    const size_t o_wid = (size_t)n * 8;
    if (!ctx->h_finish_in.ensure((size_t)n * 12 + 16) || !ctx->d_finish_in.ensure((size_t)n * 12 + 16)) return fail(ctx, HQTICK_E_DEVICE, "hipMalloc finish staging");
    memcpy(ctx->h_finish_in.p, task_id, (size_t)n * 8); memcpy(ctx->h_finish_in.as<unsigned char>() + o_wid, worker_id, (size_t)n * 4);
    HQ_HIP(hipMemcpyAsync(ctx->d_finish_in.p, ctx->h_finish_in.p, (size_t)n * 12, hipMemcpyHostToDevice, ctx->stream));
    const uint64_t *d_ids = ctx->d_finish_in.as<uint64_t>();
    const uint32_t *d_wid = reinterpret_cast<const uint32_t *>(ctx->d_finish_in.as<unsigned char>() + o_wid);
    // 1: the ledger's entries and the kinds; the Retracting table's (task, worker it is retracting from) pairs ride along as overrides
    std::vector<uint64_t> retr_id; std::vector<uint32_t> retr_wid;
    ctx->retr.sources(&retr_id, &retr_wid);
    const uint32_t *hit = nullptr;
    const int accepted = ledger_fail(ctx, ctx->asg.finish(ledger_env(ctx), n, d_ids, d_wid, (uint32_t)retr_id.size(), retr_id.data(), retr_wid.data(), &hit));
    if (accepted < 0) { ctx->asg.finish_out = hqasg::Ledger::FinishOut{}; return accepted; }
    // 2: try_remove_redirection's other half: the accepted Retracting tasks leave the table, and the resident ready set if they still sat in their queue
    std::vector<uint64_t> queued;
    for (size_t k = 0; hit && k < retr_id.size(); k++) {
        if (hit[k] == hqasg::NONE) continue;
        uint32_t old_id = 0; bool in_queue = false;
        if (ctx->retr.find(retr_id[k], &old_id, &in_queue) && in_queue) queued.push_back(retr_id[k]);
        ctx->retr.cancel(retr_id[k]);
    }
    if (!queued.empty() && ctx->ready.cols().n) { if (int rc = ready_fail(ctx, ctx->ready.remove(ready_env(ctx), queued.size(), queued.data())); rc < 0) return rc; }
    // 3 / 4: the graph (task_finished's consumers, reactor.rs:570-580) sees the accepted positions alone; the released consumers join the ready set
    if (accepted > 0 && ctx->graph.resident()) {
        const int r = ctx->graph.finish_device(n, d_ids, ctx->asg.finish_out.d_kind, ctx->stream);
        const uint32_t rel = ctx->graph.n_out();  // (also when the call reports ERR_NOT_READY: the graph itself is consistent)
        if (rel) { if (int rc = ready_fail(ctx, ctx->ready.add_device(ready_env(ctx), ctx->graph.out_id(), ctx->graph.out_prio(), ctx->graph.out_rq(), rel))) return rc; }
        if (r < 0) return graph_fail(ctx, r);
    } else if (ctx->graph.resident()) {
        ctx->graph.finish_device(0, nullptr, nullptr, ctx->stream);  // (nothing accepted: hqtick_graph_last_ids / _last_unknown answer as after an empty hqtick_graph_finish)
    }
    return accepted;
}); }

int hqtick_finish_last_routes(const hqtick_ctx *ctx, uint32_t *n, const uint8_t **kind) {
    if (!ctx) { if (n) *n = 0; if (kind) *kind = nullptr; return HQTICK_E_INVALID; }
    if (n) *n = ctx->asg.finish_out.n;
    if (kind) *kind = ctx->asg.finish_out.kind;
    return 0;
}

// task_running's Retracting arm (reactor.rs:311-335): host glue over Ledger::release, Retracting::cancel and Ledger::add, in the reference's order -- the
// redirect's entry leaves first, so a task the tick had put back on the worker it is retracting from (the dummy redirect) can be entered again.
int hqtick_retracting_started(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id, const uint32_t *rq, const uint8_t *variant, const uint64_t *priority) { return with_audit(ctx, [&]() -> int {
    if (!ctx) return HQTICK_E_INVALID;
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set");
    if (int rc = ledger_open(ctx, "hqtick_retracting_started", n, task_id && worker_id && rq && variant && priority)) return rc;
    ctx->asg.last_unknown = 0;
    if (n == 0) return 0;
    std::vector<uint64_t> s_id, s_prio, queued; std::vector<uint32_t> s_wid, s_rq; std::vector<uint8_t> s_var;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t old_id = 0; bool in_queue = false;
        if (!ctx->retr.find(task_id[i], &old_id, &in_queue) || old_id != worker_id[i]) continue;
        if (std::find(s_id.begin(), s_id.end(), task_id[i]) != s_id.end()) continue;  // (a later position of a started id: the entry is gone by then)
        s_id.push_back(task_id[i]); s_wid.push_back(worker_id[i]); s_rq.push_back(rq[i]); s_var.push_back(variant[i]); s_prio.push_back(priority[i]);
        if (in_queue) queued.push_back(task_id[i]);
    }
    const uint32_t m = (uint32_t)s_id.size();
    if (m) {
        if (int rc = ledger_fail(ctx, ctx->asg.release(ledger_env(ctx), m, s_id.data())); rc < 0) return rc;  // try_remove_redirection (an id without a redirect has no entry: unknown to the release)
        for (uint64_t t : s_id) ctx->retr.cancel(t);
        if (!queued.empty() && ctx->ready.cols().n) { if (int rc = ready_fail(ctx, ctx->ready.remove(ready_env(ctx), queued.size(), queued.data())); rc < 0) return rc; }
        const int k = ledger_fail(ctx, ctx->asg.add(ledger_env(ctx), m, s_id.data(), s_wid.data(), s_rq.data(), s_var.data(), s_prio.data()));  // insert_sn_task on the old worker
        if (k < 0) return k;
        if (ctx->asg.last_unknown) return fail(ctx, HQTICK_E_INVALID, "hqtick_retracting_started: an entry names an unknown worker, request or variant");
    }
    ctx->asg.last_unknown = n - m;
    return (int)m;
}); }

// The audit of the resident state (audit.h): the views of what this context holds, read through const accessors, handed to hqaudit::Auditor.  Nothing here changes
// the context: no selection or placement is abandoned, no mirror is synchronised, ctx->err is written only when the call itself fails.
int hqtick_resident_check(hqtick_ctx *ctx, uint32_t parts, hqtick_check_report *out) {
    if (!ctx || !out) return HQTICK_E_INVALID;
    if (parts & ~(HQ_CHECK_ALL | HQ_CHECK_STRICT)) return fail(ctx, HQTICK_E_INVALID, "hqtick_resident_check: undefined bit in parts");
    HQ_HIP(hipSetDevice(ctx->device));
    hqaudit::State S{};
    hqaudit::Totals t{};
    S.parts = parts;
    if (ctx->ready.resident()) {
        const hqready::Cols c = ctx->ready.cols();
        S.ready = hqaudit::Ready{c.id, c.rq, c.n};
        S.have |= hqaudit::HAVE_READY;
        t.ready_live = ctx->ready.live();
    }
    if (ctx->graph.resident()) {
        const hqgraph::View v = ctx->graph.audit_view();
        const hqgraph::Stats st = ctx->graph.stats();
        S.graph = hqaudit::Graph{v.id, v.unfinished, v.gen, v.head, v.ht_key, v.ht_val, v.ht_mask, v.run_next, v.run_off, v.run_len, reinterpret_cast<const uint32_t *>(v.edge),
                                 (uint32_t)st.n_slots, (uint32_t)st.n_runs, (uint32_t)st.n_edges_pool, st.n_tasks};
        S.have |= hqaudit::HAVE_GRAPH;
        t.graph_tasks = st.n_tasks; t.graph_slots = st.n_slots; t.graph_free = ctx->graph.free_slots();
    }
    hqasg::Ledger::AuditView lv{};
    hqaudit::ReqHost req{};
    if (ctx->asg.on && ctx->ws.valid() && ctx->asg.audit_view(ledger_env(ctx), &lv)) {
        hqaudit::Ledger &l = S.ledger;
        l.key = lv.t.key; l.worker = lv.t.worker; l.rq = lv.t.rq; l.variant = lv.t.variant; l.mask = lv.t.mask;
        l.wid = lv.r.wid; l.W = lv.r.W; l.R = lv.r.R; l.total = lv.r.total; l.free_ = lv.r.free_; l.counts = lv.r.counts; l.stride = lv.r.stride; l.pf = lv.r.pf; l.pf_stride = lv.r.pf_stride;
        l.mn_task = lv.m.task; l.mn_root = lv.m.root; l.flags = lv.m.flags;
        l.n_live = ctx->asg.n_live; l.mn_live = ctx->asg.mn_live; l.pf_live = ctx->asg.pf_live;
        req = hqaudit::ReqHost{lv.rq_off, lv.vent_off, lv.ent_res, lv.var_nodes, lv.ent_kind, lv.ent_amt};
        S.have |= hqaudit::HAVE_LEDGER;
        if (!(ctx->asg.pending && ctx->ready.selection_live())) S.have |= hqaudit::HAVE_LEDGER_SETTLED;  // (a placement waiting for its consume: the Retracting table is already that tick's)
        if (ctx->asg.tracking()) S.have |= hqaudit::HAVE_TRACKING;
    }
    hqaudit::RetrHost retr;
    if ((parts & HQ_CHECK_CROSS) && ctx->retr.count())
        ctx->retr.for_each([&](uint64_t task, bool in_queue, bool has_redirect, uint32_t target, uint8_t variant) {
            retr.task.push_back(task); retr.target.push_back(target); retr.variant.push_back(variant);
            retr.flags.push_back((uint8_t)((in_queue ? hqaudit::RETR_IN_QUEUE : 0) | (has_redirect ? hqaudit::RETR_REDIRECT : 0)));
        });
    const int rc = ctx->audit.run(ctx->stream, S, t, retr, req, out);
    if (rc < 0) ctx->err = ctx->audit.err;
    return rc;
}

int hqtick_ready_compact(hqtick_ctx *ctx) { return with_audit(ctx, [&]() -> int {
    if (!ctx) return HQTICK_E_INVALID;
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set");
    if (ctx->ready.live() == ctx->ready.cols().n) return 0;  // no tombstone
    HQ_HIP(hipSetDevice(ctx->device));
    return ready_fail(ctx, ctx->ready.compact(ready_env(ctx)));
}); }

}  // extern "C"

extern "C" {

// The tail of both queries, on the sub-context: the model over the fake workers K2 has evaluated (fresh: free == total), batches from the scan's runs, the solve, and
// which of the fake workers it loaded  (query.rs:73-81)
static int solve_on_fake_workers(hqtick_ctx *ctx, const hqtick_snapshot *s, const hqtick_query_workers *fake, const WorkerEval &ev_real, const WorkerEval &ev_fake, const Scan &sc,
                                 hqtick_query_result *out) {
    const uint32_t Q = s->n_requests;
    hqhost::Problem pb;
    fill_problem(pb, s, ctx->cfg, ev_real);
    hqhost::WorkerSet fw;
    hqsolve::fake_worker_set(fw, fake, s->n_resources, ev_fake.flags, ev_fake.tmc, Q ? s->rq_variant_off[Q] : 0);
    hqhost::group_equal_rows(fw, true);
    pb.custom = &fw;
    std::vector<hqhost::QueueLevels> qlv = queue_levels(sc, s);
    std::vector<hqhost::TaskBatch> batches = hqhost::create_task_batches(pb, qlv);
    hqhost::Counts cnt = ctx->solver.solve(solve_env(ctx), pb, batches, hqsolve::Opts{false, false, 0, false}, nullptr);
    if (cnt.error) return fail(ctx, cnt.error, cnt.errmsg);
    hqsolve::loaded_flags(cnt, fake->n_workers, ctx->q_loaded);
    out->n_workers = fake->n_workers; out->is_loaded = ctx->q_loaded.data(); out->is_optimal = cnt.is_optimal;
    return 0;
}

// The what-if query runs on the live Core between two ticks (crates/tako/src/control.rs:125-155): it must not disturb what the ctx keeps
// resident (ready-set columns, level table, the last tick's selection that hqtick_ready_consume_last replays, the dependency graph).  It
// therefore runs on a private sub-context — same device, own stream and buffers — created on first use.
static int query_ctx(hqtick_ctx *ctx) {
    if (ctx->qctx) return 0;
    hqtick_config cfg = ctx->cfg; cfg.flags |= HQTICK_FLAG_NO_KERNEL_TIMING;
    int rc = hqtick_create(&cfg, &ctx->qctx);
    if (rc) { ctx->qctx = nullptr; return fail(ctx, rc, "creating the query sub-context failed"); }
    return 0;
}
static int query_on(hqtick_ctx *ctx, const hqtick_snapshot *s, const hqtick_query_workers *fake, hqtick_query_result *out);
int hqtick_query(hqtick_ctx *ctx, const hqtick_snapshot *s, const hqtick_query_workers *fake, hqtick_query_result *out) {
    if (!ctx || !out || !fake) return HQTICK_E_INVALID;
    if (int rc = query_ctx(ctx)) return rc;
    int rc = query_on(ctx->qctx, s, fake, out);
    if (rc < 0) ctx->err = ctx->qctx->err;
    return rc;
}
static int query_on(hqtick_ctx *ctx, const hqtick_snapshot *s, const hqtick_query_workers *fake, hqtick_query_result *out) {
    int rc = validate(ctx, s, true);
    if (rc) return rc;
    HQ_HIP(hipSetDevice(ctx->device));
    if ((rc = ready_fail(ctx, ctx->ready.load(ctx->stream, s, false)))) return rc;  // (the query reads no task id)
    ctx->scan.columns_changed();
    WorkerEval ev_real, ev_fake;
    if ((rc = eval_workers_sync(ctx, s, fake->n_workers, fake->worker_total, fake->worker_total, fake->worker_remaining_ns, &ev_fake))) return rc;  // fresh fake workers: free == total
    Scan sc;
    if ((rc = phase_a(ctx, s, &ev_real, &sc))) return rc;
    return solve_on_fake_workers(ctx, s, fake, ev_real, ev_fake, sc, out);
}


int hqtick_query_resident(hqtick_ctx *ctx, const hqtick_snapshot *s, const hqtick_query_workers *fake, hqtick_query_result *out, uint64_t *rq_ready) {
    if (!ctx || !out || !fake) return HQTICK_E_INVALID;
    if (!s) return fail(ctx, HQTICK_E_INVALID, "null snapshot");
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set (hqtick_upload_ready)");
    if (ctx->ready.selection_pending()) return fail(ctx, HQTICK_E_INVALID, "a selection of hqtick_run_resident is pending: call hqtick_ready_consume_last before hqtick_query_resident");
    if (fake->n_workers && (!fake->worker_id || !fake->worker_total || !fake->worker_remaining_ns)) return fail(ctx, HQTICK_E_INVALID, "fake worker arrays missing");
    // What the query reads of the snapshot: resources, requests, the prefill sets' sizes and priorities.  The real workers and everything indexed by them
    // (blocked pairs, assignments, the prefill sets' workers, Retracting entries) are dropped, so W = 0, HQ_WORKERS_RESIDENT and a worker list answer alike.
    hqtick_snapshot sub = *s;
    sub.n_workers = 0; sub.worker_id = nullptr; sub.worker_total = nullptr; sub.worker_free = nullptr; sub.worker_remaining_ns = nullptr; sub.worker_min_utilization = nullptr;
    sub.worker_flags = nullptr; sub.worker_group = nullptr; sub.worker_map_rank = nullptr;
    sub.n_blocked = 0; sub.blocked_worker = nullptr; sub.blocked_rq = nullptr; sub.blocked_variant = nullptr;
    sub.assigned_off = nullptr; sub.assigned_rq = nullptr; sub.assigned_variant = nullptr; sub.prefilled_off = nullptr; sub.prefilled_rq = nullptr;
    sub.n_ready = 0; sub.task_id = nullptr; sub.task_priority = nullptr; sub.task_rq = nullptr;
    sub.prefill_off = nullptr; sub.prefill_priority = nullptr; sub.prefill_task = nullptr; sub.prefill_worker = nullptr;
    sub.n_retracting = 0; sub.retracting_task = nullptr; sub.retracting_worker = nullptr; sub.retracting_redirect_worker = nullptr; sub.retracting_redirect_variant = nullptr;
    if (int rc = validate(ctx, &sub, false)) return rc;
    const uint32_t Q = s->n_requests;
    if (s->prefill_off) {   // (queue_levels reads the sizes and priorities of the prefill sets)
        for (uint32_t q = 0; q < Q; q++) if (s->prefill_off[q] > s->prefill_off[q + 1]) return fail(ctx, HQTICK_E_INVALID, "prefill_off not monotone");
        if ((Q ? s->prefill_off[Q] : 0) && !s->prefill_priority) return fail(ctx, HQTICK_E_INVALID, "prefill arrays missing");
        sub.prefill_off = s->prefill_off; sub.prefill_priority = s->prefill_priority;
    }
    HQ_HIP(hipSetDevice(ctx->device));
    if (int rc = query_ctx(ctx)) return rc;
    hqtick_ctx *q = ctx->qctx;
    // the census reads ctx's columns on ctx's stream — behind every add, remove, append and compaction queued there — and writes only the sub-context's scanner
    Scan sc;
    if (int rc = q->scan.census(ctx->stream, ctx->ready.cols(), ctx->ready.live(), Q, &sc)) return fail(ctx, rc, q->scan.err);
    if (rq_ready) {
        for (uint32_t r = 0; r < Q; r++) rq_ready[r] = 0;
        for (uint32_t r = 0; r < Q; r++) for (uint32_t k = sc.run_off[r]; k < sc.run_off[r + 1]; k++) rq_ready[r] += sc.run_cnt[k];
    }
    // batches, model and solve on the sub-context, as hqtick_query
    WorkerEval ev_real, ev_fake;
    int rc = eval_workers_sync(q, &sub, fake->n_workers, fake->worker_total, fake->worker_total, fake->worker_remaining_ns, &ev_fake);
    if (!rc) rc = solve_on_fake_workers(q, &sub, fake, ev_real, ev_fake, sc, out);
    if (rc < 0) ctx->err = q->err;
    return rc;
}

#ifdef HQTICK_TEST_HOOKS
// ---- libhqtick_test.so only (include/hqtick_debug.h): CPU hooks for the test suite.  Not compiled into libhqtick.so. ----
namespace {
thread_local int g_block_emulation = 0, g_price_emulation = 0; thread_local uint32_t g_price_min_cols = 0, g_last_price_sweeps = 0, g_last_price_rounds = 0;
thread_local uint32_t g_block_budget = 4096, g_last_blocks_device = 0, g_last_blocks_host = 0;
thread_local uint32_t g_block_verify = 2, g_tick_seq = 0, g_last_guard[3] = {0, 0, 0}; thread_local int g_corrupt_mode = 0; thread_local uint32_t g_corrupt_class = 0, g_corrupt_fill = 0;
thread_local double g_last_stage_us[3] = {0, 0, 0};
}  // namespace

void hqtick_debug_set_block_guard(uint32_t verify, uint32_t tick_seq, int corrupt_mode, uint32_t corrupt_class, uint32_t corrupt_fill) {
    g_block_verify = verify; g_tick_seq = tick_seq; g_corrupt_mode = corrupt_mode; g_corrupt_class = corrupt_class; g_corrupt_fill = corrupt_fill;
}
void hqtick_debug_last_block_guard(uint32_t *verified, uint32_t *mismatch, uint32_t *rejected) {
    if (verified) *verified = g_last_guard[0]; if (mismatch) *mismatch = g_last_guard[1]; if (rejected) *rejected = g_last_guard[2];
}
thread_local hqhost::BlockMemo *g_memo = nullptr; thread_local uint32_t g_last_memo = 0;
void hqtick_debug_set_block_memo(int on) { if (on && !g_memo) g_memo = new hqhost::BlockMemo(); if (!on) { delete g_memo; g_memo = nullptr; } }
uint32_t hqtick_debug_last_block_memo(void) { return g_last_memo; }
void hqtick_debug_set_price_emulation(int on, uint32_t min_cols) { g_price_emulation = on; g_price_min_cols = min_cols; }
void hqtick_debug_set_fast_path(int on) { hqmilp::set_fast_path(on); }
void hqtick_debug_check_model_hints(int on) { hqprice::set_check_hints(on != 0); }
int hqtick_debug_model_hint_mismatches(void) { return hqprice::hint_mismatches(); }
thread_local int g_price_fault = -1;
void hqtick_debug_set_price_fault(int fail_at) { g_price_fault = fail_at; }
// the host stages as ONE RANK of a sharded scheduler: emulated sweeps / class blocks over this rank's share, completed through `fn` (tests/test_sharded.py: gloo)
thread_local hqtick_exchange_fn g_xfn = nullptr; thread_local void *g_xuser = nullptr; thread_local uint32_t g_xrank = 0, g_xworld = 1, g_xmin_blocks = 1, g_xmin_classes = 1, g_xcalls = 0;
void hqtick_debug_set_exchange(hqtick_exchange_fn fn, void *user, uint32_t rank, uint32_t world, uint32_t min_blocks, uint32_t min_classes) {
    g_xfn = fn; g_xuser = user; g_xrank = rank; g_xworld = world ? world : 1; g_xmin_blocks = min_blocks; g_xmin_classes = min_classes;
}
uint32_t hqtick_debug_last_exchange_calls(void) { return g_xcalls; }
void hqtick_debug_last_stage_us(double *out3) { if (out3) for (int i = 0; i < 3; i++) out3[i] = g_last_stage_us[i]; }
void hqtick_debug_last_price(uint32_t *sweeps, uint32_t *rounds) { if (sweeps) *sweeps = g_last_price_sweeps; if (rounds) *rounds = g_last_price_rounds; }
static thread_local std::vector<uint32_t> g_last_mn_rq, g_last_mn_off{0}, g_last_mn_worker;
uint32_t hqtick_debug_last_mn(const uint32_t **rq, const uint32_t **off, const uint32_t **worker) {
    if (rq) *rq = g_last_mn_rq.data();
    if (off) *off = g_last_mn_off.data();
    if (worker) *worker = g_last_mn_worker.data();
    return (uint32_t)g_last_mn_rq.size();
}
uint32_t hqtick_debug_clock_launches(const hqtick_ctx *ctx) { return ctx ? ctx->ws.clock_launches() : 0u; }
int hqtick_debug_last_order(const hqtick_ctx *ctx, uint32_t *n_runs, uint32_t *n_levels, double *order_us) {
    if (!ctx) return HQTICK_E_INVALID;
    const hqscan::Scanner::View &v = ctx->scan.last_view();
    if (n_runs) *n_runs = v.valid ? v.runs : 0;
    if (n_levels) *n_levels = v.valid ? v.levels : 0;
    if (order_us) *order_us = v.valid ? v.us : 0.0;
    return v.valid ? 1 : 0;
}
int hqtick_debug_last_scan(const hqtick_ctx *ctx, int which, uint32_t *n_levels, uint32_t *n_groups, uint32_t shape[4], uint64_t *levels, uint32_t cap_levels, uint32_t *hist,
                           uint32_t cap_groups) {
    if (!ctx || (which != 0 && which != 1)) return HQTICK_E_INVALID;
    if (which == 1 && !ctx->qctx) return 0;
    const hqscan::Scanner::Dense d = which == 0 ? ctx->scan.last_dense() : ctx->qctx->scan.last_census();  // what the last dense scan / the last census (on the query sub-context) left
    if (!d.valid) return 0;
    if (n_levels) *n_levels = d.L;
    if (n_groups) *n_groups = d.G;
    if (shape) for (int i = 0; i < 4; i++) shape[i] = d.shape[i];
    if (levels) for (uint32_t i = 0; i < d.L && i < cap_levels; i++) levels[i] = d.levels[i];
    if (hist) for (uint32_t i = 0; i < d.G && i < cap_groups; i++) hist[i] = d.hist[i];
    return 1;
}
// The ordered view by itself ("The view hooks"): built by a scanner of its own (ViewHooks), so that ctx keeps its permutation, its pending selection, its
// sticky flag and its level table; every device array comes back by one copy, here and nowhere on a tick's path.
int hqtick_debug_order_view(hqtick_ctx *ctx, uint32_t n_requests, uint32_t counts[4], uint32_t *perm, uint32_t *inv, uint32_t *lrank, uint64_t cap_slots, uint32_t *run_rq,
                            uint32_t *run_start, uint32_t *run_rank, uint64_t *run_prio, uint32_t cap_runs) {
    if (!ctx || !counts) return HQTICK_E_INVALID;
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set (hqtick_upload_ready)");
    HQ_HIP(hipSetDevice(ctx->device));
    if (!ctx->view_hooks) {
        ctx->view_hooks = new ViewHooks();
        if (int rc = ctx->view_hooks->scan.init()) { delete ctx->view_hooks; ctx->view_hooks = nullptr; return fail(ctx, rc, "creating the view sub-context failed"); }
    }
    ViewHooks *v = ctx->view_hooks;
    const hqready::Cols cols = ctx->ready.cols(); const uint64_t N = cols.n;
    v->valid = false; v->rq_copy = false;
    for (int i = 0; i < 4; i++) counts[i] = 0;
    Scan sc;
    hqscan::Env env{}; env.stream = ctx->stream;  // (untimed)
    if (int rc = v->scan.view(env, cols, n_requests, &sc)) return fail(ctx, rc, v->scan.err);
    const uint32_t nr = (uint32_t)sc.run_cnt.size(), n = nr ? sc.run_start.back() + sc.run_cnt.back() : 0u;
    if ((nr != 0) != v->scan.last_view().valid) return fail(ctx, HQTICK_E_DEVICE, "ordered view: the run table and the debug record disagree");
    counts[0] = n; counts[1] = nr; counts[2] = sc.L; counts[3] = v->scan.last_view().passes;
    if (n > cap_slots || N > cap_slots || nr > cap_runs) return fail(ctx, HQTICK_E_CAPACITY, "hqtick_debug_order_view: output arrays too small");
    if (n) {
        if (perm) HQ_HIP(hipMemcpy(perm, v->scan.perm(), (size_t)n * 4, hipMemcpyDeviceToHost));
        if (inv) HQ_HIP(hipMemcpy(inv, v->scan.inv(), (size_t)N * 4, hipMemcpyDeviceToHost));
        if (lrank) HQ_HIP(hipMemcpy(lrank, v->scan.level_ranks(N), (size_t)N * 4, hipMemcpyDeviceToHost));
        const hqscan::OrderTabLayout tl = hqscan::order_tab_layout(n);  // (the run table is in pinned host memory already: the view has synchronised)
        const uint8_t *hh = v->scan.run_table();
        if (run_rq) memcpy(run_rq, hh + tl.o_rq, (size_t)nr * 4);
        if (run_start) memcpy(run_start, hh + tl.o_st, (size_t)nr * 4);
        if (run_rank) memcpy(run_rank, hh + tl.o_rk, (size_t)nr * 4);
        if (run_prio) memcpy(run_prio, hh + tl.o_pr, (size_t)nr * 8);
    }
    v->ids = cols.id; v->N = N; v->Q = n_requests; v->n_live = n;
    v->run_off = std::move(sc.run_off); v->run_start = std::move(sc.run_start); v->run_rank = std::move(sc.run_level);
    v->valid = true;
    return 0;
}

namespace {
// the view hqtick_debug_order_view last built, if ctx's columns are still the ones it was built on
ViewHooks *debug_view_of(hqtick_ctx *ctx) {
    ViewHooks *v = ctx->view_hooks;
    if (!v || !v->valid || !ctx->ready.resident() || v->ids != ctx->ready.cols().id || v->N != ctx->ready.cols().n) return nullptr;
    return v;
}
}  // namespace

// k_order_select on that view.  mark_mode 0: select; 1: consume (RQ_TOMBSTONE at the selected slots, nothing selected); 2: restore (the request ids back, nothing
// selected); 3: consume and select in one launch (HQTICK_FLAG_CONSUME_IN_TICK).  The marks go to a copy of the rq column — a fresh one for modes 0, 1 and 3, the copy as the
// previous call left it for mode 2 — never to ctx's column.  The plan is checked on the host before the launch: no destination outside its request's range.
int hqtick_debug_order_select(hqtick_ctx *ctx, const uint32_t *rq_sel_base, const uint32_t *q_tnc, uint32_t n_sel, int mark_mode, uint64_t *sel_task, uint32_t *sel_rank,
                              uint32_t *rq_after, uint32_t *err) {
    if (!ctx || !rq_sel_base || !q_tnc || !sel_task || !sel_rank || !err || mark_mode < 0 || mark_mode > 3) return HQTICK_E_INVALID;
    ViewHooks *v = debug_view_of(ctx);
    if (!v) return fail(ctx, HQTICK_E_INVALID, "hqtick_debug_order_select: no view of the current ready set (hqtick_debug_order_view)");
    const uint32_t Q = v->Q, n = v->n_live, nr = (uint32_t)v->run_start.size();
    const uint64_t N = v->N;
    if (Q == 0 || n_sel == 0 || n == 0) return fail(ctx, HQTICK_E_INVALID, "hqtick_debug_order_select: nothing to select from");
    if (rq_sel_base[0] != 0 || rq_sel_base[Q] != n_sel) return fail(ctx, HQTICK_E_INVALID, "hqtick_debug_order_select: rq_sel_base does not span [0, n_sel]");
    for (uint32_t q = 0; q < Q; q++) {
        if (rq_sel_base[q] > rq_sel_base[q + 1]) return fail(ctx, HQTICK_E_INVALID, "hqtick_debug_order_select: rq_sel_base not monotone");
        const uint32_t take = rq_sel_base[q + 1] - rq_sel_base[q], nw = q_tnc[q] >> 16, c = q_tnc[q] & 0xFFFFu;
        if (!q_tnc[q]) continue;
        if (nw == 0) return fail(ctx, HQTICK_E_INVALID, "hqtick_debug_order_select: worker-major form without workers");
        for (uint32_t p = 0; p < take && p < nw * c; p++)
            if ((uint64_t)(p % nw) * c + p / nw >= take) return fail(ctx, HQTICK_E_INVALID, "hqtick_debug_order_select: a worker-major destination leaves its request's range");
    }
    if (mark_mode == 2 && !v->rq_copy) return fail(ctx, HQTICK_E_INVALID, "hqtick_debug_order_select: restore needs the copy a consume left");
    HQ_HIP(hipSetDevice(ctx->device));
    // the tables in HBM, as a tick's plan carries them: [rq_sel_base Q + 1][run_off Q + 1][q_tnc Q][run_start nr][run_rank nr]
    std::vector<uint32_t> tab;
    tab.insert(tab.end(), rq_sel_base, rq_sel_base + Q + 1);
    tab.insert(tab.end(), v->run_off.begin(), v->run_off.end());
    tab.insert(tab.end(), q_tnc, q_tnc + Q);
    tab.insert(tab.end(), v->run_start.begin(), v->run_start.end());
    tab.insert(tab.end(), v->run_rank.begin(), v->run_rank.end());
    if (!v->d_map.ensure(tab.size() * 4 + 16) || !v->d_sel_task.ensure((size_t)n_sel * 8 + 16) || !v->d_sel_rank.ensure((size_t)n_sel * 4 + 16) || !v->d_rq.ensure(N * 4 + 8))
        return fail(ctx, HQTICK_E_DEVICE, "hipMalloc view selection");
    HQ_HIP(hipMemcpy(v->d_map.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    uint32_t *derr = v->scan.select_err_dev();
    HQ_HIP(hipMemsetAsync(derr, 0, 4, ctx->stream));
    HQ_HIP(hipMemsetAsync(v->d_sel_task.p, 0xFF, (size_t)n_sel * 8, ctx->stream));   // the sentinel: a j the kernel did not write stays 0xFF..FF
    HQ_HIP(hipMemsetAsync(v->d_sel_rank.p, 0xFF, (size_t)n_sel * 4, ctx->stream));
    if (mark_mode != 2) { HQ_HIP(hipMemcpyAsync(v->d_rq.p, ctx->ready.cols().rq, N * 4, hipMemcpyDeviceToDevice, ctx->stream)); v->rq_copy = true; }
    const uint32_t *d = v->d_map.as<uint32_t>();
    hqk::OrderSelect os{};
    os.task_id = ctx->ready.cols().id; os.perm = v->scan.perm(); os.n_live = n; os.Q = Q; os.n_runs = nr;
    os.rq_sel_base = d; os.run_off = d + (Q + 1); os.q_tnc = d + 2 * (size_t)(Q + 1); os.run_start = os.q_tnc + Q; os.run_rank = os.run_start + nr;
    os.sel_task = v->d_sel_task.as<uint64_t>(); os.sel_rank = v->d_sel_rank.as<uint32_t>(); os.err = derr;
    if (mark_mode) { os.mark_rq = v->d_rq.as<uint32_t>(); os.mark_value = mark_mode == 2 ? 0u : hqk::RQ_TOMBSTONE; os.mark_and_select = mark_mode == 3 ? 1u : 0u; }
    HQ_HIP(hqk::order_select(os, n_sel, ctx->stream));
    HQ_HIP(hipStreamSynchronize(ctx->stream));
    HQ_HIP(hipMemcpy(sel_task, v->d_sel_task.p, (size_t)n_sel * 8, hipMemcpyDeviceToHost));
    HQ_HIP(hipMemcpy(sel_rank, v->d_sel_rank.p, (size_t)n_sel * 4, hipMemcpyDeviceToHost));
    if (rq_after) HQ_HIP(hipMemcpy(rq_after, v->d_rq.p, N * 4, hipMemcpyDeviceToHost));
    HQ_HIP(hipMemcpy(err, derr, 4, hipMemcpyDeviceToHost));
    return 0;
}

// k_order_rank_of on that view: (request, position in the view) of the wanted ids against ctx's id and rq columns; 0xFFFFFFFF twice = not a live task of the set
int hqtick_debug_order_rank_of(hqtick_ctx *ctx, const uint64_t *want, uint32_t n_want, uint32_t *out_rq, uint32_t *out_pos) {
    if (!ctx || (n_want && (!want || !out_rq || !out_pos))) return HQTICK_E_INVALID;
    ViewHooks *v = debug_view_of(ctx);
    if (!v) return fail(ctx, HQTICK_E_INVALID, "hqtick_debug_order_rank_of: no view of the current ready set (hqtick_debug_order_view)");
    if (n_want == 0) return 0;
    if (v->n_live == 0) { for (uint32_t i = 0; i < n_want; i++) out_rq[i] = out_pos[i] = 0xFFFFFFFFu; return 0; }  // (as phase A: no view, no launch)
    HQ_HIP(hipSetDevice(ctx->device));
    if (!v->d_want.ensure((size_t)n_want * 16 + 16)) return fail(ctx, HQTICK_E_DEVICE, "hipMalloc wanted ids");
    uint8_t *dw = v->d_want.as<uint8_t>();
    HQ_HIP(hipMemcpy(dw, want, (size_t)n_want * 8, hipMemcpyHostToDevice));
    HQ_HIP(hqk::order_rank_of(ctx->ready.cols().id, ctx->ready.cols().rq, v->N, v->scan.inv(), reinterpret_cast<const uint64_t *>(dw), n_want,
                              reinterpret_cast<uint32_t *>(dw + (size_t)n_want * 8), reinterpret_cast<uint32_t *>(dw + (size_t)n_want * 12), ctx->stream));
    HQ_HIP(hipStreamSynchronize(ctx->stream));
    HQ_HIP(hipMemcpy(out_rq, dw + (size_t)n_want * 8, (size_t)n_want * 4, hipMemcpyDeviceToHost));
    HQ_HIP(hipMemcpy(out_pos, dw + (size_t)n_want * 12, (size_t)n_want * 4, hipMemcpyDeviceToHost));
    return 0;
}

void hqtick_debug_set_block_emulation(int on, uint32_t budget) { g_block_emulation = on; if (budget) g_block_budget = budget; }
void hqtick_debug_last_blocks(uint32_t *n_emulated, uint32_t *n_host) { if (n_emulated) *n_emulated = g_last_blocks_device; if (n_host) *n_host = g_last_blocks_host; }

int hqtick_debug_block_solve_host(uint32_t n_cols, uint32_t n_resources, const uint32_t *ent_off, const uint32_t *ent_res, const uint8_t *ent_kind, const uint64_t *ent_amount,
                                  const uint32_t *weight, const double *pool, uint32_t n_classes, const uint64_t *free_, const uint64_t *total, const uint64_t *elig,
                                  uint32_t budget, uint32_t *x, uint32_t *status, uint32_t *steps) {
    hqblock::ColTable ct{n_cols, n_resources, ent_off, ent_res, ent_kind, ent_amount, weight, pool, nullptr, 0};
    hqblock::ClassTable cl{n_classes, free_, total, elig};
    hqblock::Output out{x, status, steps, nullptr};
    hqsolve::EmulatedBlocks emu(budget ? budget : 4096);
    return emu.solve(ct, cl, out) ? 0 : HQTICK_E_DEVICE;
}

// Test hooks (include/hqtick_debug.h): the host stages on caller-supplied scan outputs.  No device is touched.  with_plan: the five stages of the mapping plan
// (map_core.h) behind the solver, on the Retracting tasks' (key, rank) arrays of the dense form, the plan's big tables in a heap block.
static uint32_t *heap_storage(void *vec, size_t words) { auto *v = static_cast<std::vector<uint32_t> *>(vec); v->assign(words, 0); return v->data(); }
static int host_stages(const hqtick_config *config, const hqtick_snapshot *s, const uint8_t *vflags, const uint32_t *vtmc, uint32_t n_levels, const uint64_t *levels,
                       const uint32_t *hist, bool with_plan, const uint32_t *retr_key, const uint32_t *retr_rank, hqtick_result *out, std::string *err) {
    if (!config || !s || !out) return HQTICK_E_INVALID;
    struct KeepError { hqtick_ctx *c; std::string *e; ~KeepError() { if (e) *e = c->err; } };  // the refusal's text, for the hook that hands it out
    static thread_local hqtick_ctx *holder = nullptr;  // owns the result arrays; never creates a stream or a buffer
    if (!holder) holder = new hqtick_ctx();
    hqtick_ctx *ctx = holder;
    KeepError keep{ctx, err};
    ctx->cfg = *config; ctx->err.clear();
    if (int rc = validate(ctx, s, false)) return rc;
    WorkerEval ev; ev.flags = vflags; ev.tmc = vtmc;
    hqhost::Problem pb;
    fill_problem(pb, s, ctx->cfg, ev);
    Scan sc; sc.Q = s->n_requests; sc.L = n_levels; sc.G = n_levels * s->n_requests;
    sc.levels.assign(levels, levels + n_levels); sc.hist.assign(hist, hist + (size_t)n_levels * s->n_requests);
    runs_from_hist(sc);
    std::vector<hqhost::QueueLevels> qlv = queue_levels(sc, s);
    std::vector<hqhost::TaskBatch> batches = hqhost::create_task_batches(pb, qlv);
    memset(out, 0, sizeof(*out));
    g_last_mn_rq.clear(); g_last_mn_off.assign(1, 0); g_last_mn_worker.clear();
    export_batches(ctx, batches, out);
    hqsolve::EmulatedBlocks emu(g_block_budget);
    emu.corrupt_mode = g_corrupt_mode; emu.corrupt_class = g_corrupt_class; emu.corrupt_fill = g_corrupt_fill;
    hqprice::EmulatedSweeper pemu;
    if (g_price_emulation) { pemu.fail_at = g_price_fault; pemu.budget = g_block_budget; if (g_price_min_cols) pemu.min_cols = g_price_min_cols; }
    hqsolve::wire(pb, hqsolve::Wiring{g_block_emulation ? &emu : nullptr, 1, g_price_emulation ? &pemu : nullptr, g_block_verify, g_tick_seq, g_memo});
    hqhost::Counts cnt;
    auto solve = [&]() {
        if (g_xfn && g_xworld > 1) {  // this call is one rank of a sharded scheduler
            hqsolve::FnExchange xch(g_xfn, g_xuser, g_xrank, g_xworld);
            cnt = hqsolve::run_solver(pb, batches, &xch, g_xmin_classes, g_xmin_blocks);
            g_xcalls = (uint32_t)xch.n_calls;
        } else cnt = hqsolve::run_solver(pb, batches, nullptr, 0, 0);
    };
    // hqtick_debug_set_defer_row_check(1): the row check of a fast-path placement is this caller's, as in a tick (TickRun::run) — run behind the solver, and a failure
    // sends the model down the classic path in a second call.  Never as a rank of a sharded scheduler, like the tick.
    pb.defer_row_check = hqmilp::g_check_hook && hqmilp::g_check_hook->allow == 1 && !(g_xfn && g_xworld > 1);
    solve();
    if (cnt.row_check_pending() && !cnt.settle_row_check()) { pb.defer_row_check = false; pb.no_fast_path = true; solve(); }
    if (cnt.error) return fail(ctx, cnt.error, cnt.errmsg);
    g_last_guard[0] = cnt.blocks_verified; g_last_guard[1] = cnt.blocks_mismatch; g_last_guard[2] = cnt.blocks_rejected;
    g_last_memo = cnt.blocks_memo;
    g_last_blocks_device = cnt.blocks_device; g_last_blocks_host = cnt.blocks_host; g_last_price_sweeps = (uint32_t)cnt.price_sweeps; g_last_price_rounds = (uint32_t)cnt.price_rounds;
    g_last_stage_us[0] = cnt.t_classify_us; g_last_stage_us[1] = cnt.t_blocks_us; g_last_stage_us[2] = cnt.t_decode_us;
    for (size_t i = 0; i < cnt.mn_rq.size(); i++)
        for (auto &set : cnt.mn_sets[i]) { g_last_mn_rq.push_back(cnt.mn_rq[i]); g_last_mn_worker.insert(g_last_mn_worker.end(), set.begin(), set.end()); g_last_mn_off.push_back((uint32_t)g_last_mn_worker.size()); }
    hqmap::HostResult &hr = ctx->map.res;
    hr.cnt_rq.clear(); hr.cnt_variant.clear(); hr.cnt_worker.clear(); hr.cnt_value.clear();
    cnt.pairs();
    for (size_t k = 0; k < cnt.keys.size(); k++)
        for (auto &wc : cnt.per_key[k]) { hr.cnt_rq.push_back(cnt.keys[k].first); hr.cnt_variant.push_back(cnt.keys[k].second); hr.cnt_worker.push_back(wc.first); hr.cnt_value.push_back(wc.second); }
    out->is_optimal = cnt.is_optimal; out->is_canonical = cnt.is_canonical && cnt.is_optimal;
    out->status = hqsolve::tick_status(cnt);
    if (with_plan) {  // (plan_keys writes the counts itself: the same rows, in the same order)
        static thread_local std::vector<uint32_t> tables;
        hqmap::Plan &ps = ctx->map.plan;
        hqmap::PlanIn in{};
        in.sc = &sc; in.cnt = &cnt; in.s = s; in.rqs = pb.rqs.data(); in.variants = pb.variants.data();
        in.proactive_filling_reserve = config->proactive_filling_reserve; in.proactive_filling_max = config->proactive_filling_max; in.flags = config->flags;
        in.shard_count = 1; in.retr_key = retr_key; in.retr_rank = retr_rank; in.transpose_on = transpose_enabled();
        for (size_t g = 0; g < sc.hist.size(); g++) in.N += sc.hist[g];
        in.storage = heap_storage; in.user = &tables;
        const char *why = nullptr; int rc;
        if ((rc = hqmap::plan_keys(ps, hr, in, &why)) || (rc = hqmap::plan_redirects(ps, hr, in, &why)) || (rc = hqmap::plan_prefill(ps, hr, in, &why)) ||
            (rc = hqmap::plan_outputs(ps, hr, in, &why)))
            return fail(ctx, rc, why);
        hqmap::assemble_host_part(ps, hr, in);
        out->rec_off = hr.rec_off.data(); out->retract_off = hr.retract_off.data(); out->retract_task = hr.retract_task.data();
        out->n_redirects = (uint32_t)hr.red_task.size(); out->redirect_task = hr.red_task.data(); out->redirect_worker = hr.red_worker.data();
        out->redirect_variant = hr.red_variant.data(); out->redirect_kind = hr.red_kind.data(); out->new_free = hr.new_free.data();
    }
    out->n_counts = (uint32_t)hr.cnt_rq.size(); out->count_rq = hr.cnt_rq.data(); out->count_variant = hr.cnt_variant.data();
    out->count_worker = hr.cnt_worker.data(); out->count_value = hr.cnt_value.data();
    return out->status;
}
int hqtick_debug_host_stages(const hqtick_config *config, const hqtick_snapshot *s, const uint8_t *vflags, const uint32_t *vtmc, uint32_t n_levels,
                             const uint64_t *levels, const uint32_t *hist, hqtick_result *out) {
    return host_stages(config, s, vflags, vtmc, n_levels, levels, hist, false, nullptr, nullptr, out, nullptr);
}
int hqtick_debug_host_plan(const hqtick_config *config, const hqtick_snapshot *s, const uint8_t *vflags, const uint32_t *vtmc, uint32_t n_levels, const uint64_t *levels,
                           const uint32_t *hist, const uint32_t *retracting_key, const uint32_t *retracting_rank, hqtick_result *out, const char **error) {
    static thread_local std::string text;
    if (error) *error = "";
    if (s && s->n_retracting && (!retracting_key || !retracting_rank)) return HQTICK_E_INVALID;
    const int rc = host_stages(config, s, vflags, vtmc, n_levels, levels, hist, true, retracting_key, retracting_rank, out, &text);
    if (rc < 0 && error) *error = text.c_str();
    return rc;
}

int hqtick_debug_host_query(const hqtick_config *config, const hqtick_snapshot *s, const hqtick_query_workers *fake, const uint8_t *vflags, const uint32_t *vtmc,
                            const uint8_t *fake_vflags, const uint32_t *fake_vtmc, uint32_t n_levels, const uint64_t *levels, const uint32_t *hist,
                            hqtick_query_result *out) {
    if (!config || !s || !fake || !out) return HQTICK_E_INVALID;
    static thread_local hqtick_ctx *holder = nullptr;
    if (!holder) holder = new hqtick_ctx();
    hqtick_ctx *ctx = holder;
    ctx->cfg = *config;
    if (int rc = validate(ctx, s, false)) return rc;
    const uint32_t R = s->n_resources, Q = s->n_requests;
    WorkerEval ev; ev.flags = vflags; ev.tmc = vtmc;
    hqhost::Problem pb;
    fill_problem(pb, s, ctx->cfg, ev);
    hqhost::WorkerSet fw;  // as in hqtick_query
    hqsolve::fake_worker_set(fw, fake, R, fake_vflags, fake_vtmc, Q ? s->rq_variant_off[Q] : 0);
    hqhost::group_equal_rows(fw, true);
    pb.custom = &fw;
    Scan sc; sc.Q = Q; sc.L = n_levels; sc.G = n_levels * Q;
    sc.levels.assign(levels, levels + n_levels); sc.hist.assign(hist, hist + (size_t)n_levels * Q);
    runs_from_hist(sc);
    std::vector<hqhost::QueueLevels> qlv = queue_levels(sc, s);
    std::vector<hqhost::TaskBatch> batches = hqhost::create_task_batches(pb, qlv);
    hqsolve::EmulatedBlocks emu(g_block_budget);
    if (g_block_emulation) { pb.blocks = &emu; pb.block_min_classes = 1; }
    hqhost::Counts cnt = hqhost::run_scheduling_solver(pb, batches);
    if (cnt.error) return fail(ctx, cnt.error, cnt.errmsg);
    hqsolve::loaded_flags(cnt, fake->n_workers, ctx->q_loaded);  // query.rs:73-81
    out->n_workers = fake->n_workers; out->is_loaded = ctx->q_loaded.data(); out->is_optimal = cnt.is_optimal;
    return 0;
}

#endif  // HQTICK_TEST_HOOKS

int hqtick_set_shard(hqtick_ctx *ctx, uint32_t shard_index, uint32_t shard_count) {
    if (!ctx) return HQTICK_E_INVALID;
    if (shard_count > 1 && shard_index >= shard_count) return fail(ctx, HQTICK_E_INVALID, "shard_index >= shard_count");
    if (shard_count > 1 && ctx->asg.on) return fail(ctx, HQTICK_E_UNSUPPORTED, "hqtick_set_shard: the assignment ledger is on (hqtick_assigned_disable first)");
    ctx->shard_index = shard_count > 1 ? shard_index : 0; ctx->shard_count = shard_count > 1 ? shard_count : 1;
    return 0;
}

int hqtick_set_exchange(hqtick_ctx *ctx, hqtick_exchange_fn fn, void *user) {
    if (!ctx) return HQTICK_E_INVALID;
    ctx->solver.set_exchange(fn, user);
    return 0;
}

size_t hqtick_sink_bytes(uint32_t n_workers, uint32_t capacity_records) {
    size_t o_task = (16 + (size_t)(n_workers + 1) * 4 + 7) & ~(size_t)7;
    return (o_task + (size_t)capacity_records * 10 + 15) & ~(size_t)15;
}

uint32_t hqtick_sink_capacity_records(uint32_t n_workers, size_t capacity_bytes) {
    size_t fixed = hqtick_sink_bytes(n_workers, 0);
    if (capacity_bytes < fixed) return 0;
    size_t cap = (capacity_bytes - fixed) / 10;
    while (cap && hqtick_sink_bytes(n_workers, (uint32_t)cap) > capacity_bytes) cap--;
    return cap > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cap;
}

int hqtick_set_record_sink(hqtick_ctx *ctx, void *device_ptr, size_t capacity_bytes) {
    if (!ctx) return HQTICK_E_INVALID;
    if (device_ptr && (reinterpret_cast<uintptr_t>(device_ptr) & 15)) return fail(ctx, HQTICK_E_INVALID, "record sink must be 16-byte aligned");
    ctx->sink = device_ptr; ctx->sink_bytes = device_ptr ? capacity_bytes : 0;
    return 0;
}

#ifdef HQTICK_TEST_HOOKS  // measurement hooks of the tools (include/hqtick_debug.h): libhqtick_test.so only
int hqtick_time_kernel(hqtick_ctx *ctx, int which, int iters, double *avg_us) {
    if (!ctx || !avg_us || iters <= 0) return HQTICK_E_INVALID;
    if (!ctx->ready.selection_valid() || !ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "hqtick_time_kernel needs a preceding hqtick_run_resident tick that placed tasks");
    const hqmap::Mapper::Last last = ctx->map.last_selection();
    if (last.ordered) return fail(ctx, HQTICK_E_INVALID, "hqtick_time_kernel times the dense scan: the last tick took the ordered view");
    HQ_HIP(hipSetDevice(ctx->device));
    const hqready::Cols cols = ctx->ready.cols(); const hqk::WaveGeom g = last.geom;
    if (which == 2) {  // calibration: an EMPTY kernel of K1's grid, each launch bracketed by its own start / stop events like the stats pass of a tick
        double sum = 0.0; int cnt = 0;
        for (int i = 0; i < iters; i++) {
            hqk::time_next_launch(ctx->ev[2], ctx->ev[3]);
            HQ_HIP(hqk::empty_like_level_hist(g, ctx->stream));
            HQ_HIP(hipStreamSynchronize(ctx->stream));
            const double us_ = elapsed_us(ctx->ev[2], ctx->ev[3]);
            if (us_ >= 0) { sum += us_; cnt++; }
        }
        *avg_us = cnt ? sum / cnt : 0.0;
        return 0;
    }
    // HQTICK_KTIME_GRAPH: the launches captured into one graph and replayed — no host launch cost between them (a launch call with K1's argument block takes
    // longer than the kernel runs at 1 M tasks), so (graph duration) / iters is what the GPU spends per launch, kernel boundary included
    const bool as_graph = getenv("HQTICK_KTIME_GRAPH") != nullptr;
    if (as_graph) HQ_HIP(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    else HQ_HIP(hipEventRecord(ctx->ev[10], ctx->stream));
    for (int i = 0; i < iters; i++) {
        if (which == 0) { if (int rc = scan_fail(ctx, ctx->scan.relaunch_level_hist(ctx->stream, cols, last.L, last.Q, g))) return rc; }
        else if (which == 1) { if (int rc = map_fail(ctx, ctx->map.replay_selection(ctx->stream, hqmap::REPLAY_TIMED, cols, ctx->scan, ctx->ready.selected_count()))) return rc; }
        else return fail(ctx, HQTICK_E_INVALID, "which: 0 = level_hist, 1 = select_scatter, 2 = empty kernel of level_hist's grid");
    }
    if (as_graph) {
        hipGraph_t gr = nullptr; hipGraphExec_t ge = nullptr;
        HQ_HIP(hipStreamEndCapture(ctx->stream, &gr));
        HQ_HIP(hipGraphInstantiate(&ge, gr, nullptr, nullptr, 0));
        HQ_HIP(hipGraphLaunch(ge, ctx->stream));  // once untimed
        HQ_HIP(hipEventRecord(ctx->ev[10], ctx->stream));
        HQ_HIP(hipGraphLaunch(ge, ctx->stream));
        HQ_HIP(hipEventRecord(ctx->ev[11], ctx->stream));
        HQ_HIP(hipStreamSynchronize(ctx->stream));
        hipGraphExecDestroy(ge); hipGraphDestroy(gr);
    } else HQ_HIP(hipEventRecord(ctx->ev[11], ctx->stream));
    if (which == 0)  // K1 left raw counts in the slice table: turn them back into offsets
        if (int rc = scan_fail(ctx, ctx->scan.relaunch_scan_waves(ctx->stream, g, last.G))) return rc;
    HQ_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    HQ_HIP(hipEventElapsedTime(&ms, ctx->ev[10], ctx->ev[11]));
    *avg_us = (double)ms * 1000.0 / iters;
    return 0;
}

int hqtick_timeline(const hqtick_ctx *ctx, double *out, int cap) {
    if (!ctx || !out) return 0;
    int n = ctx->ntl < cap ? ctx->ntl : cap;
    for (int i = 0; i < n; i++) out[i] = ctx->tl[i];
    return n;
}

const uint64_t *hqtick_block_profile_last(const hqtick_ctx *ctx, uint32_t *n_classes) {
    if (!ctx) { if (n_classes) *n_classes = 0; return nullptr; }
    return ctx->solver.block_profile_last(n_classes);
}
#endif

int hqtick_set_kernel_timing(hqtick_ctx *ctx, int on) {
    if (!ctx) return HQTICK_E_INVALID;
    ctx->timing = on != 0 && on != 2; ctx->timing_k1 = on == 2;  // (any non-zero value but 2 = every measured kernel, as before ABI 9)
    return 0;
}

int hqtick_kernel_stats_last(const hqtick_ctx *ctx, hqtick_kernel_stats *out) {
    if (!ctx || !out) return HQTICK_E_INVALID;
    *out = ctx->stats;
    out->ready_appends = ctx->ready.appends();
    return 0;
}

// ---- the library's own RCCL communicator (hqsolve::Solver, solve.h): arguments validated here ----
int hqtick_comm_unique_id(void *id_out) {
    if (!id_out) return HQTICK_E_INVALID;
    return hqsolve::Solver::comm_unique_id(id_out);
}

int hqtick_comm_init(hqtick_ctx *ctx, const void *id, uint32_t rank, uint32_t world) {
    if (!ctx || !id || world == 0 || rank >= world) return HQTICK_E_INVALID;
    if (int rc = solver_fail(ctx, ctx->solver.comm_init(ctx->device, id, rank, world))) return rc;
    return hqtick_set_shard(ctx, rank, world);
}

int hqtick_shard_allgather(hqtick_ctx *ctx, void *recv_device, size_t recv_bytes) {
    if (!ctx || !recv_device) return HQTICK_E_INVALID;
    if (!ctx->solver.has_comm()) return fail(ctx, HQTICK_E_INVALID, "hqtick_shard_allgather without hqtick_comm_init");
    if (!ctx->sink || !ctx->sink_bytes) return fail(ctx, HQTICK_E_INVALID, "hqtick_shard_allgather without a record sink (hqtick_set_record_sink)");
    if (recv_bytes < (size_t)ctx->solver.comm_world() * ctx->sink_bytes) return fail(ctx, HQTICK_E_CAPACITY, "receive buffer smaller than world x sink bytes");
    return solver_fail(ctx, ctx->solver.allgather_device(solve_env(ctx), ctx->sink, recv_device, ctx->sink_bytes));
}

#ifdef HQTICK_TEST_HOOKS
// libhqtick_test.so: one all-gather of a host buffer through the library's RCCL communicator, as the sharded solve issues it per sweep — for the single-rank
// round trip of the GPU suite (recv == send) and for timing the exchange's fixed cost (H2D + ncclAllGather + D2H + one stream synchronisation)
int hqtick_debug_exchange(hqtick_ctx *ctx, const void *send, void *recv, size_t bytes_per_rank) {
    if (!ctx || !send || !recv) return HQTICK_E_INVALID;
    if (!ctx->solver.has_comm()) return fail(ctx, HQTICK_E_INVALID, "hqtick_debug_exchange without hqtick_comm_init");
    return ctx->solver.allgather_host(solve_env(ctx), send, recv, bytes_per_rank) ? 0 : fail(ctx, HQTICK_E_DEVICE, "the RCCL exchange failed");
}
#endif

int hqtick_comm_destroy(hqtick_ctx *ctx) {
    if (!ctx) return HQTICK_E_INVALID;
    ctx->solver.comm_destroy(ctx->device);
    return 0;
}

}  // extern "C"

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
// (map.h; the plan itself, free of HIP, in map_core.h).  The host stages between them — the snapshot's checks, the Problem, the queue levels, the batches' export,
// the plan's input and stage sequence, the row check's retry, a query's tail — are tick_core.h's, free of HIP and shared with the test hooks.  The context's layout
// is ctx.h's.  This file keeps the sequence of a tick (TickRun::run), the two queries and the C ABI's argument checks; the test library's hooks on a context live
// in debug_tick.cpp, so that both libraries link this file's one object.
// There is no CPU implementation of the scans or of the selection and the records: without a HIP device every entry point fails.
#include "../../include/hqtick.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "ctx.h"
#include "lose_core.h"
#include "reject_core.h"
#include "start_core.h"

using hqbuf::PinBuf;
using hqcluster::UpView;
using hqscan::Scan;
using hqscan::WorkerEval;

namespace {

double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

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
    hqready::Cols cols = ctx->ready.cols();
    // a resident set that holds only tombstones (every task handed out, cancelled or removed since the last compaction) is the empty set: nothing to discover a
    // level from, nothing to scan -- and still a tick: it may take tasks out of the prefill sets for a worker that has room (mapping.rs:82-104)
    if (ctx->ready.resident() && ctx->ready.live() == 0) cols.n = 0;
    const int rc = ctx->scan.scan(scan_env(ctx), cols, hqscan::Shape{Q, s->n_retracting, s->retracting_task},
                                  hqscan::Workers{W, s->n_resources, (size_t)W * (Q ? s->rq_variant_off[Q] : 0), worker_tables, &t}, ev, sc, while_gpu_runs);
    const hqscan::Timings &tm = ctx->scan.timings();
    if (tm.distinct_us >= 0) ctx->stats.distinct_us = tm.distinct_us;
    if (tm.level_hist_us >= 0) ctx->stats.level_hist_us = tm.level_hist_us;
    if (tm.scan_us >= 0) ctx->stats.scan_us = tm.scan_us;
    return scan_fail(ctx, rc);
}

bool is_replica(hqtick_ctx *ctx) { return ctx->solver.replica(solve_env(ctx)); }  // others read this context's sweeps or records (a record sink alone is one scheduler's output path)

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

    // the ready set: uploaded with the snapshot, or already resident
    int load_ready_set() {
        if (!use_resident) {
            if (int rc = ready_fail(ctx, ctx->ready.load(ctx->stream, s, true))) return rc;
            ctx->scan.columns_changed();
        } else if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "hqtick_run_resident without hqtick_upload_ready");
        N = ctx->ready.cols().n;
        if (ctx->ready.resident() && ctx->ready.live() == 0) N = 0;  // (only tombstones: phase_a)
        return 0;
    }

    // what the plan reads (map_core.h): hqstages::plan_in, and of the context the sink, the shard, the ledger's prefilled counts and the plan's storage
    hqmap::PlanIn plan_in() {
        hqmap::PlanIn in = hqstages::plan_in(sc, cnt, s, pb, ctx->cfg, N, ctx->scan.retracting_keys(), ctx->scan.retracting_ranks());
        in.sink = ctx->sink != nullptr; in.shard_index = ctx->shard_index; in.shard_count = ctx->shard_count;
        if (ctx->asg.on && ctx->asg.tracking()) {  // the ledger's prefilled counts (its sync_mirror brought them back; a snapshot with prefilled_off was refused)
            uint32_t pf_stride = 0;
            const std::vector<uint32_t> &h_pf = ctx->asg.prefilled_host(&pf_stride);
            if (h_pf.size() >= (size_t)W * pf_stride) { in.ledger_pf = h_pf.data(); in.ledger_pf_stride = pf_stride; }
        }
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
        int rc = hqstages::validate(s, !use_resident, ctx->err);
        if (rc) return rc;
        HQ_HIP(hipSetDevice(ctx->device));
        if ((rc = load_ready_set())) return rc;
        // ---------------- GPU phase A ----------------
        const std::function<void()> prep = [&]() {   // request/worker views: no GPU output needed yet
            hqstages::fill_problem(pb, s, ctx->cfg, ev);
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
        std::vector<hqhost::QueueLevels> qlv = hqstages::queue_levels(sc, s);
        std::vector<hqhost::TaskBatch> batches = hqhost::create_task_batches(pb, qlv);
        hqstages::export_batches(batches, ctx->batches, out);
        mark();  // 1: batches
        const double t2 = now_us();
        // Solve, plan and phase C.  They run twice in one case only (hqstages::with_row_check): the placement came from the fast path with its row check deferred into
        // phase C's window (below) and the check failed — then once more with the fast path off, which is what the inline check's failure leads to.
        const hqmap::Env me = map_env(ctx, t0);
        const uint32_t tick_seq = ctx->tick_seq++;
        const int ntl_solve = ctx->ntl;
        double t3 = t2;
        const std::function<void()> check = [&]() { if (cnt.row_check_pending()) cnt.settle_row_check(); };  // (the verdict stays with the counts)
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
            rc = hqstages::plan_stages(ps, hr, in, &why, [&](int stage) -> int {
                if (stage == 0) return map_fail(ctx, ctx->map.launch_sweep_early(me));  // K5a's sweep over the key tables, while the host plans on
                if (stage == 3) { if (int crc = map_fail(ctx, ctx->map.check_capacity(sc.ordered))) return crc; }
                mark();  // 3: key tables + retracts, 4: prefill plan, 5: K5 tables
                return 0;
            });
            if (rc) { if (why) ctx->err = why; return rc; }  // (a stage's refusal carries its text; the mapper has left its own)
            // ---------------- GPU phase C ----------------
            return phase_c(me, in, defer && cnt.row_check_pending() ? &check : nullptr);
        };
        // What a failed check leads to is what the inline check's failure does: the classic path's placement.  The discarded pass has left nothing but buffers the
        // second one overwrites (may_defer_row_check: no tombstones, no ledger staging, no sink) and the selection's launch state, which goes.
        rc = hqstages::with_row_check(cnt, may_defer_row_check(), solve_plan_map, [&]() -> int {
            HQ_HIP(hipStreamSynchronize(ctx->stream));
            ctx->ready.selection_void(); ctx->map.forget_selection();
            ctx->ntl = ntl_solve;
            return 0;
        });
        if (rc) return rc;
        mark();  // 8: phase C synced
        finish(me, t1, t2, t3);
        return status;
    }
};

// a placement waiting for hqtick_ready_consume_last is still live only while the tick's selection is: every ready-set delta that abandons the selection
// (an add, a remove, a compaction, a graph call, an upload) ends ready.selection_live() -- and with it the placement is dropped too, so the ready set need not
// know the ledger to clear it.  Whether a placement is LIVE is asked here alone; run_tick reads Ledger::pending right after it has set it (hold or apply the
// Retracting table's part) and hqtick_resident_check reads it together with selection_live()
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
        ctx->asg.abandon_tick(); ctx->retr.drop_tick();
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
    const bool in_tick = use_resident && (ctx->cfg.flags & HQTICK_FLAG_CONSUME_IN_TICK) != 0;
    // what create_task_mapping did to the Retracting tasks becomes state with the placement: at once, or -- a two-call tick of a ledger context, which a delta may
    // still abandon -- with the ledger's part at hqtick_ready_consume_last (an abandoned tick then leaves table and ledger agreeing, both as before it)
    const bool retr_waits = rc >= 0 && retr_resident && ctx->asg.on && use_resident && !in_tick;
    auto retr_tick = [&](bool hold) {
        const hqmap::HostResult &r = ctx->map.res;
        if (hold) ctx->retr.hold_tick(s->worker_id, s->n_workers, r.retract_off, r.retract_task, r.red_task, r.red_worker, r.red_variant, r.red_kind);
        else ctx->retr.apply_tick(s->worker_id, s->n_workers, r.retract_off, r.retract_task, r.red_task, r.red_worker, r.red_variant, r.red_kind);
    };
    if (rc >= 0 && retr_resident && !retr_waits) retr_tick(false);
    if (rc >= 0 && ctx->asg.on) {  // the placement enters the ledger when it becomes state: now, or at hqtick_ready_consume_last in the two-call form
        ctx->asg.collect_tick(s, out, ctx->map.res.new_free, ctx->map.res.mn_rq, in_tick && s->n_retracting != 0);  // (the column copy is taken only for the redirects of Retracting tasks)
        if (!use_resident || in_tick) {
            if (int r2 = ledger_fail(ctx, ctx->asg.apply_tick(ledger_env(ctx)))) {  // (the tick's tasks have left the ready set: without the placement the ledger is no longer the truth)
                ctx->asg.on = false; ctx->asg.pending = false;
                ctx->err += " (the assignment ledger is switched off: upload the worker set and enable it again)";
                return r2;
            }
        } else if (!ctx->ready.selection_live()) {
            // two-call form and the tick handed out no ready task: there is no selection to keep the placement pending.  One that has something to enter (a redirect of a
            // prefilled or Retracting task, a changed free row) holds the empty selection until the consume; one with nothing at all is dropped here, as cheaply as before
            if (ctx->asg.tick_enters(ledger_env(ctx))) ctx->ready.hold_empty(); else ctx->asg.pending = false;
        }
        if (retr_waits) retr_tick(ctx->asg.pending);
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
    ctx->h_fail_in.release(); ctx->d_fail_in.release();
    ctx->h_start_in.release(); ctx->d_start_in.release();
    ctx->h_reject_in.release(); ctx->d_reject_in.release();
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
            ctx->asg.on = false; ctx->ready.entered();
            ctx->err += " (the assignment ledger is switched off: upload the worker set and enable it again)";
            return rc;
        }
        ctx->ready.entered();  // (a held empty selection has nothing to replay: the branch below ends the call)
        ctx->retr.commit_tick();
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
    if (int rc = hqstages::validate(s, false, ctx->err)) return rc;
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
    if (int rc = ledger_guard(ctx)) return rc;  // (a pending placement holds that tick's changes of this table: they are applied to the table as the tick saw it)
    ctx->retr.add(n, task_id, worker_id);
    return 0;
}

int hqtick_retract_response(hqtick_ctx *ctx, uint32_t worker_id, uint32_t n, const uint64_t *task_id, uint32_t *n_assigned, const uint64_t **assigned_task,
                            const uint32_t **assigned_worker_id, const uint8_t **assigned_variant) {
    if (!ctx) return HQTICK_E_INVALID;
    if (n && !task_id) return fail(ctx, HQTICK_E_INVALID, "hqtick_retract_response: null array");
    if (int rc = ledger_guard(ctx)) return rc;
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

// ---- task_failed in one call: composed like hqtick_finish_tasks -- ids and reporting workers staged once, the ledger's passes in their fail mode,
// the Retracting table, then the graph's closure with its owners and the ready set.  What is left when a later step fails after an earlier one succeeded: the
// earlier ones stay done (ledger, then table, then graph and ready set), the consumer lists are empty, and hqtick_graph_remove(accepted ids, 1) finishes the job
// (with hqtick_ready_remove of hqtick_graph_last_ids if it was the ready set's removal that failed).
int hqtick_fail_tasks(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id) { return with_audit(ctx, [&]() -> int {
    if (!ctx) return HQTICK_E_INVALID;
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set");
    if (int rc = ledger_open(ctx, "hqtick_fail_tasks", n, task_id && worker_id)) return rc;  // (the guard comes before any step: a refused call changes nothing)
    if (n > 0x03FFFFFFu) return fail(ctx, HQTICK_E_CAPACITY, "more than 2^26 failed tasks in one batch");
    ctx->asg.fail_out = hqasg::Ledger::FinishOut{}; ctx->asg.last_unknown = 0;
    if (int rc = ctx->graph.fail_empty(n)) return graph_fail(ctx, rc);
    if (n == 0) return 0;
    const size_t o_wid = (size_t)n * 8;
    if (!ctx->h_fail_in.ensure((size_t)n * 12 + 16) || !ctx->d_fail_in.ensure((size_t)n * 12 + 16)) return fail(ctx, HQTICK_E_DEVICE, "hipMalloc fail staging");
    memcpy(ctx->h_fail_in.p, task_id, (size_t)n * 8); memcpy(ctx->h_fail_in.as<unsigned char>() + o_wid, worker_id, (size_t)n * 4);
    HQ_HIP(hipMemcpyAsync(ctx->d_fail_in.p, ctx->h_fail_in.p, (size_t)n * 12, hipMemcpyHostToDevice, ctx->stream));
    const uint64_t *d_ids = ctx->d_fail_in.as<uint64_t>();
    const uint32_t *d_wid = reinterpret_cast<const uint32_t *>(ctx->d_fail_in.as<unsigned char>() + o_wid);
    // 1: the ledger's entries and the kinds; the Retracting table's (task, worker it is retracting from) pairs ride along as overrides
    std::vector<uint64_t> retr_id; std::vector<uint32_t> retr_wid;
    ctx->retr.sources(&retr_id, &retr_wid);
    const uint32_t *hit = nullptr;
    int accepted = ledger_fail(ctx, ctx->asg.fail_tasks(ledger_env(ctx), n, d_ids, d_wid, (uint32_t)retr_id.size(), retr_id.data(), retr_wid.data(), &hit));
    if (accepted < 0) { ctx->asg.fail_out = hqasg::Ledger::FinishOut{}; return accepted; }
    hqasg::Ledger::FinishOut &out = ctx->asg.fail_out;
    uint8_t *kinds = const_cast<uint8_t *>(out.kind);  // (the ledger's pinned block; the graph step's refusals are written into it)
    // 2: try_remove_redirection's other half: the accepted Retracting tasks leave the table, and the resident ready set if they still sat in their queue
    std::vector<uint64_t> queued;
    for (size_t k = 0; hit && k < retr_id.size(); k++) {
        if (hit[k] == hqasg::NONE) continue;
        uint32_t old_id = 0; bool in_queue = false;
        if (ctx->retr.find(retr_id[k], &old_id, &in_queue) && in_queue) queued.push_back(retr_id[k]);
        ctx->retr.cancel(retr_id[k]);
    }
    if (!queued.empty() && ctx->ready.cols().n) { if (int rc = ready_fail(ctx, ctx->ready.remove(ready_env(ctx), queued.size(), queued.data())); rc < 0) return rc; }
    // 3 / 4: the accepted ids and their transitive consumers leave graph and ready set; every consumer goes to the smallest accepted position that reaches it
    if (ctx->graph.resident()) {
        uint32_t refused = 0, bad = hqasg::NONE;
        const int r = accepted > 0 ? ctx->graph.fail_device(n, d_ids, const_cast<uint8_t *>(out.d_kind), out.kind_dev, &refused, &bad, ctx->stream)
                                   : ctx->graph.remove_device(0, nullptr, true, ctx->stream);  // (nothing accepted: hqtick_graph_last_ids / _last_unknown answer as after an empty hqtick_graph_remove)
        if (r < 0) { ctx->graph.fail_empty(n); return graph_fail(ctx, r); }
        accepted -= (int)std::min<uint32_t>(refused, (uint32_t)accepted);
        out.accepted = (uint32_t)accepted; ctx->asg.last_unknown = n - (uint32_t)accepted;
        if (r > 0 && ctx->ready.cols().n) {
            if (int rc = ready_fail(ctx, ctx->ready.remove_device(ready_env(ctx), ctx->graph.out_id(), (uint32_t)r)); rc < 0) { ctx->graph.fail_empty(n); return rc; }
        }
        if (bad != hqasg::NONE)
            return fail(ctx, HQTICK_E_INVALID, "hqtick_fail_tasks: task " + std::to_string(task_id[bad]) + " holds a worker and is a transitive consumer of an earlier failed task of the batch");
    } else {
        // no graph: a _WAITING id is failed once (a later position is a repeat) and, like a Retracting one, just leaves the ready set if it sits there
        std::vector<uint64_t> waiting;
        for (uint32_t i = 0; i < n; i++) {
            if (kinds[i] != HQ_FAIL_WAITING) continue;
            if (std::find(waiting.begin(), waiting.end(), task_id[i]) != waiting.end()) { kinds[i] = HQ_FAIL_REPEAT; accepted--; continue; }
            waiting.push_back(task_id[i]);
        }
        out.accepted = (uint32_t)accepted; ctx->asg.last_unknown = n - (uint32_t)accepted;
        if (!waiting.empty() && ctx->ready.cols().n) { if (int rc = ready_fail(ctx, ctx->ready.remove(ready_env(ctx), waiting.size(), waiting.data())); rc < 0) return rc; }
    }
    return accepted;
}); }

int hqtick_fail_last_routes(const hqtick_ctx *ctx, uint32_t *n, const uint8_t **kind) {
    if (!ctx) { if (n) *n = 0; if (kind) *kind = nullptr; return HQTICK_E_INVALID; }
    if (n) *n = ctx->asg.fail_out.n;
    if (kind) *kind = ctx->asg.fail_out.kind;
    return 0;
}

int hqtick_fail_last_consumers(const hqtick_ctx *ctx, uint32_t *n, const uint32_t **consumer_off, const uint64_t **consumer_id) {
    static const uint32_t zero_off[1] = {0};
    if (!ctx) { if (n) *n = 0; if (consumer_off) *consumer_off = nullptr; if (consumer_id) *consumer_id = nullptr; return HQTICK_E_INVALID; }
    const bool have = ctx->graph.fail_off() != nullptr;
    if (n) *n = have ? ctx->graph.fail_n() : 0;
    if (consumer_off) *consumer_off = have ? ctx->graph.fail_off() : zero_off;
    if (consumer_id) *consumer_id = have ? ctx->graph.fail_ids() : nullptr;
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
        const int k = ledger_fail(ctx, ctx->asg.add(ledger_env(ctx), m, s_id.data(), s_wid.data(), s_rq.data(), s_var.data(), s_prio.data(), 1));  // insert_sn_task on the old worker; the task runs there
        if (k < 0) return k;
        if (ctx->asg.last_unknown) return fail(ctx, HQTICK_E_INVALID, "hqtick_retracting_started: an entry names an unknown worker, request or variant");
    }
    ctx->asg.last_unknown = n - m;
    return (int)m;
}); }

// ---- task_running in one call: the checks and the order of the steps are here.  Ids, reporting workers and variants are staged once in pinned memory
// (13 B per position) and copied to the device once.  The Retracting table is the host's, so the positions it decides are known before any launch: per id of the
// table the lowest rightly reported position with a variant of the request is the _RETRACTING candidate, later such positions are _REPEAT, wrong reporters
// _WRONG_WORKER; all of them are masked out for the device.  The claim pass runs once over the whole batch (a kind follows from the tables before the batch and the
// claims; a candidate's steps touch no entry a device position names); the apply pass is cut at each candidate, because a Retracting start releases the redirect
// target's entry and enters the task on the old worker, which does not commute with a saturating start on the same row.  The usual batch has no candidate: one
// segment, one synchronisation.  If a candidate's step fails, the segments and candidates before it stay done and hqtick_start_last_routes is empty.
int hqtick_start_tasks(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id, const uint8_t *variant, const uint32_t *rq, const uint64_t *priority) {
    return with_audit(ctx, [&]() -> int {
    if (!ctx) return HQTICK_E_INVALID;
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set");
    if (int rc = ledger_open(ctx, "hqtick_start_tasks", n, task_id && worker_id && variant)) return rc;  // (the guard comes before any step: a refused call changes nothing)
    if (n > 0x03FFFFFFu) return fail(ctx, HQTICK_E_CAPACITY, "more than 2^26 started tasks in one batch");
    if (n && ctx->retr.count() && (!rq || !priority)) return fail(ctx, HQTICK_E_INVALID, "hqtick_start_tasks: rq and priority are needed while the Retracting table holds a task");
    hqasg::Ledger &asg = ctx->asg;
    asg.start_out = hqasg::Ledger::StartOut{}; asg.last_unknown = 0;
    if (n == 0) return 0;
    const size_t o_wid = (size_t)n * 8, o_var = (size_t)n * 12;
    if (!ctx->h_start_in.ensure((size_t)n * 13 + 16) || !ctx->d_start_in.ensure((size_t)n * 13 + 16)) return fail(ctx, HQTICK_E_DEVICE, "hipMalloc start staging");
    unsigned char *h = ctx->h_start_in.as<unsigned char>(), *d = ctx->d_start_in.as<unsigned char>();
    memcpy(h, task_id, (size_t)n * 8); memcpy(h + o_wid, worker_id, (size_t)n * 4); memcpy(h + o_var, variant, n);
    HQ_HIP(hipMemcpyAsync(d, h, (size_t)n * 13, hipMemcpyHostToDevice, ctx->stream));
    // the positions the Retracting table decides (the mask byte of such a position is its kind; none of the kinds it can take is 0)
    std::vector<uint8_t> mask; std::vector<uint32_t> cand;
    if (ctx->retr.count()) {
        mask.assign(n, 0);
        std::vector<uint64_t> claimed;
        for (uint32_t i = 0; i < n; i++) {
            uint32_t old_id = 0; bool in_queue = false;
            const bool found = ctx->retr.find(task_id[i], &old_id, &in_queue);
            if (!found) continue;
            const bool earlier = std::find(claimed.begin(), claimed.end(), task_id[i]) != claimed.end();
            const uint32_t kind = hqstart::kind_of(false, hqstart::E_SN, false, false, false, asg.variant_exists(rq[i], variant[i]), true, old_id == worker_id[i], earlier);
            mask[i] = (uint8_t)kind;
            if (kind == HQ_START_RETRACTING) { claimed.push_back(task_id[i]); cand.push_back(i); }
        }
    }
    const hqasg::Env e0 = ledger_env(ctx);
    if (int rc = ledger_fail(ctx, asg.start_begin(e0, n, reinterpret_cast<const uint64_t *>(d), reinterpret_cast<const uint32_t *>(d + o_wid), d + o_var, mask.empty() ? nullptr : mask.data(),
                                                  (uint32_t)cand.size())); rc < 0) return rc;
    uint32_t lo = 0, started = 0;
    // (a failed step: the claims of the positions that were not applied are given back, so that the entries can be claimed by a later batch)
    auto failed = [&](int rc) { const std::string m = ctx->err; asg.start_abort(ledger_env(ctx), lo); ctx->err = m; return rc; };
    for (uint32_t c : cand) {
        if (int rc = ledger_fail(ctx, asg.start_segment(ledger_env(ctx), lo, c, false)); rc < 0) return failed(rc);
        lo = c + 1;
        // hqtick_retracting_started's steps for this one position: try_remove_redirection, the table entry, its place in the ready set, insert_sn_task running
        uint32_t old_id = 0; bool in_queue = false;
        ctx->retr.find(task_id[c], &old_id, &in_queue);
        if (int rc = ledger_fail(ctx, asg.release(ledger_env(ctx), 1, &task_id[c])); rc < 0) return failed(rc);
        ctx->retr.cancel(task_id[c]);
        if (in_queue && ctx->ready.cols().n) { if (int rc = ready_fail(ctx, ctx->ready.remove(ready_env(ctx), 1, &task_id[c])); rc < 0) return failed(rc); }
        const int k = ledger_fail(ctx, asg.add(ledger_env(ctx), 1, &task_id[c], &worker_id[c], &rq[c], &variant[c], &priority[c], 1));
        if (k < 0) return failed(k);
        if (asg.last_unknown) return failed(fail(ctx, HQTICK_E_INVALID, "hqtick_start_tasks: a Retracting task names an unknown worker, request or variant"));
        started++;
    }
    if (int rc = ledger_fail(ctx, asg.start_segment(ledger_env(ctx), lo, n, true)); rc < 0) { asg.start_out = hqasg::Ledger::StartOut{}; return failed(rc); }
    for (uint32_t i = 0; i < n && !mask.empty(); i++) if (mask[i]) asg.start_out.kind[i] = mask[i];
    asg.start_out.accepted = std::min(asg.start_out.accepted + started, n);
    asg.last_unknown = n - asg.start_out.accepted;
    return (int)asg.start_out.accepted;
}); }

int hqtick_start_last_routes(const hqtick_ctx *ctx, uint32_t *n, const uint8_t **kind) {
    if (!ctx) { if (n) *n = 0; if (kind) *kind = nullptr; return HQTICK_E_INVALID; }
    if (n) *n = ctx->asg.start_out.n;
    if (kind) *kind = ctx->asg.start_out.kind;
    return 0;
}

int hqtick_assigned_running(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, uint8_t *running) {
    if (!ctx) return HQTICK_E_INVALID;
    if (!ctx->asg.on) return fail(ctx, HQTICK_E_INVALID, "assignment ledger not enabled (hqtick_assigned_enable)");
    if (n && (!task_id || !running)) return fail(ctx, HQTICK_E_INVALID, "hqtick_assigned_running: null array");
    if (!n) return 0;
    HQ_HIP(hipSetDevice(ctx->device));
    return ledger_fail(ctx, ctx->asg.running(ledger_env(ctx), n, task_id, running));
}

int hqtick_cluster_last_requeued_running(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id) {
    if (!ctx) return HQTICK_E_INVALID;
    if (n) *n = (uint32_t)ctx->asg.rq_run_task.size();
    if (task_id) *task_id = ctx->asg.rq_run_task.data();
    return 0;
}

// ---- task_reject in one call: the checks and the order of the steps are here.  Ids, reporting workers, the permutation of the positions by
// ascending (id, position), the requests (only while the Retracting table holds a task) and the variants are staged once in pinned memory and copied to the device
// once.  1: the ledger's passes in their reject mode give every position its kind, take the _ASSIGNED and _PREFILLED entries out and leave the requeued tasks as
// three dense ascending columns on the device (one synchronisation).  2: the Retracting table's part on the host, as hqtick_retract_response does it for one id;
// with a redirect the kind becomes _REDIRECTED.  3: the blocks, in batch order.  4: the columns join the resident ready set (ReadySet::add_device, the graph's
// path; its own wait).  Host waits per call: one, two when something is requeued.  Every buffer of the four steps is ensured before the first change, the merge's
// included (ReadySet::ensure_add).  If the merge still fails (a device error), the entries have left the ledger and hqtick_ready_add of
// hqtick_reject_last_requeued finishes the job.
int hqtick_reject_tasks(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id, const uint8_t *variant, const uint32_t *rq) {
    return with_audit(ctx, [&]() -> int {
    if (!ctx) return HQTICK_E_INVALID;
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set");
    if (int rc = ledger_open(ctx, "hqtick_reject_tasks", n, task_id && worker_id && variant)) return rc;  // (the guard comes before any step: a refused call changes nothing)
    if (n > 0x03FFFFFFu) return fail(ctx, HQTICK_E_CAPACITY, "more than 2^26 rejected tasks in one batch");
    const bool with_rq = ctx->retr.count() != 0;
    if (n && with_rq && !rq) return fail(ctx, HQTICK_E_INVALID, "hqtick_reject_tasks: rq is needed while the Retracting table holds a task");
    hqasg::Ledger &asg = ctx->asg;
    asg.reject_out = hqasg::Ledger::RejectOut{}; asg.last_unknown = 0; ctx->reject_reassigned.clear();
    if (n == 0) return 0;
    const size_t o_wid = (size_t)n * 8, o_perm = (size_t)n * 12, o_rq = (size_t)n * 16, o_var = o_rq + (with_rq ? (size_t)n * 4 : 0), bytes = o_var + n;
    if (!ctx->h_reject_in.ensure(bytes + 16) || !ctx->d_reject_in.ensure(bytes + 16)) return fail(ctx, HQTICK_E_DEVICE, "hipMalloc reject staging");
    std::vector<uint64_t> retr_id; std::vector<uint32_t> retr_wid;
    ctx->retr.sources(&retr_id, &retr_wid);
    if (int rc = ledger_fail(ctx, asg.reject_ensure(ledger_env(ctx), n, (uint32_t)retr_id.size()))) return rc;
    if (int rc = ready_fail(ctx, ctx->ready.ensure_add(std::min<uint64_t>(n, asg.n_live + asg.pf_live)))) return rc;  // (at most every single-node and prefilled entry goes back)
    unsigned char *h = ctx->h_reject_in.as<unsigned char>(), *d = ctx->d_reject_in.as<unsigned char>();
    memcpy(h, task_id, (size_t)n * 8); memcpy(h + o_wid, worker_id, (size_t)n * 4); memcpy(h + o_var, variant, n);
    if (with_rq) memcpy(h + o_rq, rq, (size_t)n * 4);
    uint32_t *perm = reinterpret_cast<uint32_t *>(h + o_perm);  // the positions by ascending (id, position): the order the requeued columns come out in
    for (uint32_t i = 0; i < n; i++) perm[i] = i;
    std::stable_sort(perm, perm + n, [&](uint32_t a, uint32_t b) { return task_id[a] < task_id[b]; });
    HQ_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    // 1: the ledger
    const uint32_t *hit = nullptr;
    const int accepted = ledger_fail(ctx, asg.reject(ledger_env(ctx), n, reinterpret_cast<const uint64_t *>(d), reinterpret_cast<const uint32_t *>(d + o_wid), d + o_var,
                                                     with_rq ? reinterpret_cast<const uint32_t *>(d + o_rq) : nullptr, reinterpret_cast<const uint32_t *>(d + o_perm),
                                                     (uint32_t)retr_id.size(), retr_id.data(), retr_wid.data(), &hit));
    if (accepted < 0) { asg.reject_out = hqasg::Ledger::RejectOut{}; return accepted; }
    hqasg::Ledger::RejectOut &out = asg.reject_out;
    // 2: the Retracting tasks leave the table in batch order; one with a redirect is Assigned on its target (the target's ledger entry is already there)
    std::vector<uint32_t> hits;
    for (size_t k = 0; hit && k < retr_id.size(); k++) if (hit[k] != hqasg::NONE && hit[k] < n) hits.push_back(hit[k]);
    std::sort(hits.begin(), hits.end());
    for (uint32_t i : hits) {
        bool redirected = false;
        if (ctx->retr.take(worker_id[i], task_id[i], &ctx->reject_reassigned, &redirected) && redirected) out.kind[i] = HQ_REJECT_REDIRECTED;
    }
    // 3: worker.block_request per position (reactor.rs:389-391), in batch order; a position that lost its claim blocks nothing
    for (uint32_t i = 0; i < n; i++)
        if (out.blk_rq[i] != hqasg::NONE && hqreject::blocks_kind(out.kind[i])) ctx->ws.block(worker_id[i], out.blk_rq[i], variant[i]);
    // 4: add_ready_task for what left the ledger (reactor.rs:440-442), device columns into the device merge
    if (out.n_requeued) { if (int rc = ready_fail(ctx, ctx->ready.add_device(ready_env(ctx), out.d_id, out.d_prio, out.d_rq, out.n_requeued))) return rc; }
    return accepted;
}); }

int hqtick_reject_last_routes(const hqtick_ctx *ctx, uint32_t *n, const uint8_t **kind) {
    if (!ctx) { if (n) *n = 0; if (kind) *kind = nullptr; return HQTICK_E_INVALID; }
    if (n) *n = ctx->asg.reject_out.n;
    if (kind) *kind = ctx->asg.reject_out.kind;
    return 0;
}

int hqtick_reject_last_requeued(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id, const uint32_t **rq, const uint64_t **priority) {
    if (!ctx) return HQTICK_E_INVALID;
    const hqasg::Ledger::RejectOut &o = ctx->asg.reject_out;
    if (n) *n = o.n_requeued;
    if (task_id) *task_id = o.rq_id;
    if (rq) *rq = o.rq_rq;
    if (priority) *priority = o.rq_prio;
    return 0;
}

int hqtick_reject_last_reassigned(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id, const uint32_t **worker_id, const uint8_t **variant) {
    if (!ctx) return HQTICK_E_INVALID;
    ctx->reject_reassigned.get(n, task_id, worker_id, variant);
    return 0;
}

int hqtick_cluster_enable_request(hqtick_ctx *ctx, uint32_t worker_id, uint32_t rq, uint8_t variant) {
    if (int rc = cluster_open(ctx, "hqtick_cluster_enable_request")) return rc;
    return cluster_fail(ctx, ctx->ws.enable_request(worker_id, rq, variant));
}

int hqtick_cluster_blocked(const hqtick_ctx *cctx, uint32_t worker_id, uint32_t *n, const uint32_t **rq, const uint8_t **variant) {
    hqtick_ctx *ctx = const_cast<hqtick_ctx *>(cctx);  // (the answer's columns are the set's scratch)
    if (int rc = cluster_open(ctx, "hqtick_cluster_blocked")) return rc;
    return cluster_fail(ctx, ctx->ws.blocked_of(worker_id, n, rq, variant));
}

// ---- on_remove_worker in one call: hqtick_cluster_remove_workers' sequence, in the order that function documents as load-bearing, with the
// ledger's step replaced by Ledger::lose and the merge by ReadySet::add_device.  1: the eviction (one wait, for the count); the sort by id, the gather, the grouping
// by lost worker, the non-root members and the reset of lost roots' rows are enqueued behind it.  2: the two re-packs; the ledger's waits for everything enqueued
// so far, so the pinned lists are final behind it.  3: the host settles _REDIRECT from the Retracting table (which stays in host memory), orders the non-root
// members, and the table follows (Retracting::workers_removed).  4: the worker ids, then the merge of the three device columns (its own wait).  Every buffer of
// steps 1 and 4 is ensured before the first change.
int hqtick_lose_workers(hqtick_ctx *ctx, uint32_t n, const uint32_t *worker_id) { return with_audit(ctx, [&]() -> int {
    if (int rc = cluster_open(ctx, "hqtick_lose_workers")) return rc;
    if (!ctx->ready.resident()) return fail(ctx, HQTICK_E_INVALID, "no resident ready set");
    if (int rc = ledger_open(ctx, "hqtick_lose_workers", n, worker_id != nullptr)) return rc;
    hqasg::Ledger &asg = ctx->asg;
    const uint32_t W = ctx->ws.W();
    std::vector<uint32_t> src;
    if (n) { if (int rc = cluster_fail(ctx, ctx->ws.plan_remove(n, worker_id, &src))) return rc; }  // unknown or repeated ids: refused before anything changes
    asg.lose_out = hqasg::Ledger::LoseOut{}; ctx->lose_reassigned.clear(); ctx->lose_mn_task.clear(); ctx->lose_mn_lost.clear(); ctx->lose_mn_root.clear();
    if (n == 0) return 0;
    if (int rc = ledger_fail(ctx, asg.lose_ensure(ledger_env(ctx), n))) return rc;
    if (int rc = ready_fail(ctx, ctx->ready.ensure_add(asg.lose_bound()))) return rc;
    asg.clear_requeued();  // (the hqtick_cluster_last_requeued* lists answer for hqtick_cluster_remove_workers only: empty behind this call)
    // 1: the lost workers' entries leave the ledger
    const int k = ledger_fail(ctx, asg.lose(ledger_env(ctx), n, worker_id));
    if (k < 0) return k;
    const hqasg::Ledger::LoseOut out = asg.lose_out;
    asg.lose_out = hqasg::Ledger::LoseOut{};  // (until the lists are final)
    // 2: the rows leave the worker set and the ledger's row tables
    if (int rc = cluster_fail(ctx, ctx->ws.repack(ctx->stream, src, 0, nullptr, nullptr, nullptr))) return rc;
    if (int rc = asg.repack(ledger_env(ctx), src, W, nullptr)) return ledger_fail(ctx, rc);
    ctx->ws.keep_rows(src);
    // 3: the lists are final.  A single-node entry on the redirect TARGET of a Retracting task is the redirect's (reactor.rs:90-96)
    std::vector<std::pair<uint32_t, uint32_t>> index_of(n);  // (worker id, index in the caller's list), by id
    for (uint32_t i = 0; i < n; i++) index_of[i] = {worker_id[i], i};
    std::sort(index_of.begin(), index_of.end());
    if (out.off[n] != out.n) return fail(ctx, HQTICK_E_DEVICE, "assignment ledger: the lost workers' lists are out of sync with the entries that left");
    ctx->retr.for_each([&](uint64_t task, bool, bool has_redirect, uint32_t target, uint8_t) {
        if (!has_redirect) return;
        const auto it = std::lower_bound(index_of.begin(), index_of.end(), std::make_pair(target, 0u));
        if (it == index_of.end() || it->first != target) return;
        const uint64_t *lo = out.c_id + out.off[it->second], *hi = out.c_id + out.off[it->second + 1], *at = std::lower_bound(lo, hi, task);
        if (at != hi && *at == task) out.c_kind[at - out.c_id] = (uint8_t)hqlose::settle(out.c_kind[at - out.c_id], true);
    });
    std::vector<std::pair<uint64_t, uint32_t>> left;  // the non-root members: ascending task id, then the caller's order
    for (uint32_t i = 0; i < n; i++) if (out.mn_task[i] != hqasg::HT_EMPTY) left.push_back({out.mn_task[i], i});
    std::sort(left.begin(), left.end());
    for (const auto &m : left) { ctx->lose_mn_task.push_back(m.first); ctx->lose_mn_lost.push_back(worker_id[m.second]); ctx->lose_mn_root.push_back(out.mn_root[m.second]); }
    ctx->retr.workers_removed(n, worker_id);
    ctx->lose_reassigned = ctx->retr.last;
    asg.lose_out = out;
    // 4: the worker ids of the new rows; add_ready_task for what left the ledger, device columns into the device merge
    if (int rc = asg.upload_wids(ledger_env(ctx))) return ledger_fail(ctx, rc);
    if (out.n) { if (int rc = ready_fail(ctx, ctx->ready.add_device(ready_env(ctx), out.d_id, out.d_prio, out.d_rq, out.n))) return rc; }
    return k;
}); }

int hqtick_lose_last_tasks(const hqtick_ctx *ctx, uint32_t *n_workers, const uint32_t **task_off, const uint64_t **task_id, const uint32_t **rq, const uint64_t **priority, const uint8_t **kind) {
    if (!ctx) return HQTICK_E_INVALID;
    const hqasg::Ledger::LoseOut &o = ctx->asg.lose_out;
    if (n_workers) *n_workers = o.n_workers;
    if (task_off) *task_off = o.off;
    if (task_id) *task_id = o.c_id;
    if (rq) *rq = o.c_rq;
    if (priority) *priority = o.c_prio;
    if (kind) *kind = o.c_kind;
    return 0;
}

int hqtick_lose_last_requeued(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id, const uint32_t **rq, const uint64_t **priority) {
    if (!ctx) return HQTICK_E_INVALID;
    const hqasg::Ledger::LoseOut &o = ctx->asg.lose_out;
    if (n) *n = o.n;
    if (task_id) *task_id = o.f_id;
    if (rq) *rq = o.f_rq;
    if (priority) *priority = o.f_prio;
    return 0;
}

int hqtick_lose_last_reassigned(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id, const uint32_t **worker_id, const uint8_t **variant) {
    if (!ctx) return HQTICK_E_INVALID;
    ctx->lose_reassigned.get(n, task_id, worker_id, variant);
    return 0;
}

int hqtick_lose_last_mn_left(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id, const uint32_t **lost_worker_id, const uint32_t **root_worker_id) {
    if (!ctx) return HQTICK_E_INVALID;
    if (n) *n = (uint32_t)ctx->lose_mn_task.size();
    if (task_id) *task_id = ctx->lose_mn_task.data();
    if (lost_worker_id) *lost_worker_id = ctx->lose_mn_lost.data();
    if (root_worker_id) *root_worker_id = ctx->lose_mn_root.data();
    return 0;
}

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
        if (!(ctx->asg.pending && ctx->ready.selection_live())) S.have |= hqaudit::HAVE_LEDGER_SETTLED;  // (a placement waiting for its consume: a host between the two calls of a tick is half way through a handler)
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

// The tail of both queries, on the sub-context (hqstages::query_tail), with the sub-context's solver: no deferred check, no forced classic path, no memo
static int solve_on_fake_workers(hqtick_ctx *ctx, const hqtick_snapshot *s, const hqtick_query_workers *fake, const WorkerEval &ev_real, const WorkerEval &ev_fake, const Scan &sc,
                                 hqtick_query_result *out) {
    auto solve = [&](hqhost::Problem &pb, const std::vector<hqhost::TaskBatch> &batches) {
        return ctx->solver.solve(solve_env(ctx), pb, batches, hqsolve::Opts{false, false, 0, false}, nullptr);
    };
    return hqstages::query_tail(ctx->cfg, s, fake, ev_real, ev_fake, sc, solve, ctx->q_loaded, out, ctx->err);
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
    int rc = hqstages::validate(s, true, ctx->err);
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
    if (int rc = hqstages::validate(&sub, false, ctx->err)) return rc;
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

int hqtick_comm_destroy(hqtick_ctx *ctx) {
    if (!ctx) return HQTICK_E_INVALID;
    ctx->solver.comm_destroy(ctx->device);
    return 0;
}

}  // extern "C"

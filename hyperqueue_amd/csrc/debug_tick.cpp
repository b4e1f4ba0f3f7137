// libhqtick_test.so only (include/hqtick_debug.h): the hooks that need the context's layout (ctx.h) or the tick's host stages (tick_core.h).  Not compiled into
// libhqtick.so, which links the same hqtick.cpp object as the test library.
//   the host stages on caller-supplied scan outputs (hqtick_debug_host_stages, _host_plan, _host_query) and their per-thread knobs: no device is touched, no
//     context exists; the stages themselves are tick_core.h's, the ones a tick and a query run
//   what a context's last scan left (hqtick_debug_last_order, _last_scan, _clock_launches)
//   the ordered view by itself (hqtick_debug_order_view, _order_select, _order_rank_of)
//   the measurement hooks of the tools (hqtick_time_kernel, hqtick_timeline, hqtick_block_profile_last) and one exchange through the library's communicator
#include "../../include/hqtick.h"
#include "../../include/hqtick_debug.h"

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "price_emul.h"

using hqscan::Scan;
using hqscan::WorkerEval;

namespace {

// duration between two dispatch events in us, or -1 when the pair was not recorded (hqtick_time_kernel's calibration; the runtime's error state is cleared)
double elapsed_us(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, a, b) == hipSuccess) return (double)ms * 1000.0;
    (void)hipGetLastError();
    return -1.0;
}

thread_local int g_block_emulation = 0, g_price_emulation = 0; thread_local uint32_t g_price_min_cols = 0, g_last_price_sweeps = 0, g_last_price_rounds = 0;
thread_local uint32_t g_block_budget = 4096, g_last_blocks_device = 0, g_last_blocks_host = 0;
thread_local uint32_t g_block_verify = 2, g_tick_seq = 0, g_last_guard[3] = {0, 0, 0}; thread_local int g_corrupt_mode = 0; thread_local uint32_t g_corrupt_class = 0, g_corrupt_fill = 0;
thread_local double g_last_stage_us[3] = {0, 0, 0};
thread_local hqhost::BlockMemo *g_memo = nullptr; thread_local uint32_t g_last_memo = 0;
thread_local int g_price_fault = -1;
// the host stages as ONE RANK of a sharded scheduler: emulated sweeps / class blocks over this rank's share, completed through `fn` (tests/test_sharded.py: gloo)
thread_local hqtick_exchange_fn g_xfn = nullptr; thread_local void *g_xuser = nullptr; thread_local uint32_t g_xrank = 0, g_xworld = 1, g_xmin_blocks = 1, g_xmin_classes = 1, g_xcalls = 0;
thread_local std::vector<uint32_t> g_last_mn_rq, g_last_mn_off{0}, g_last_mn_worker;

// What the host hooks hand out pointers into, per thread, until the thread's next call: the batches' arrays, the plan and the result's host part, a query's
// loaded flags, a refusal's text.
struct HostHold { hqstages::BatchExport batches; hqmap::Plan plan; hqmap::HostResult res; std::vector<uint8_t> loaded; std::string err; };
thread_local HostHold g_hold;

uint32_t *heap_storage(void *vec, size_t words) { auto *v = static_cast<std::vector<uint32_t> *>(vec); v->assign(words, 0); return v->data(); }

// The host stages on caller-supplied scan outputs.  with_plan: the stages of the mapping plan (map_core.h) behind the solver, on the Retracting tasks' (key, rank)
// arrays of the dense form, the plan's big tables in a heap block.  A refusal's text is left in g_hold.err.
int host_stages(const hqtick_config *config, const hqtick_snapshot *s, const uint8_t *vflags, const uint32_t *vtmc, uint32_t n_levels, const uint64_t *levels,
                const uint32_t *hist, bool with_plan, const uint32_t *retr_key, const uint32_t *retr_rank, hqtick_result *out) {
    HostHold &h = g_hold;
    h.err.clear();
    if (!config || !s || !out) return HQTICK_E_INVALID;
    if (int rc = hqstages::validate(s, false, h.err)) return rc;
    WorkerEval ev; ev.flags = vflags; ev.tmc = vtmc;
    hqhost::Problem pb;
    hqstages::fill_problem(pb, s, *config, ev);
    const hqscan::Table sc = hqstages::table_from_hist(n_levels, levels, hist, s->n_requests);
    std::vector<hqhost::QueueLevels> qlv = hqstages::queue_levels(sc, s);
    std::vector<hqhost::TaskBatch> batches = hqhost::create_task_batches(pb, qlv);
    memset(out, 0, sizeof(*out));
    g_last_mn_rq.clear(); g_last_mn_off.assign(1, 0); g_last_mn_worker.clear();
    hqstages::export_batches(batches, h.batches, out);
    hqsolve::EmulatedBlocks emu(g_block_budget);
    emu.corrupt_mode = g_corrupt_mode; emu.corrupt_class = g_corrupt_class; emu.corrupt_fill = g_corrupt_fill;
    hqprice::EmulatedSweeper pemu;
    if (g_price_emulation) { pemu.fail_at = g_price_fault; pemu.budget = g_block_budget; if (g_price_min_cols) pemu.min_cols = g_price_min_cols; }
    hqsolve::wire(pb, hqsolve::Wiring{g_block_emulation ? &emu : nullptr, 1, g_price_emulation ? &pemu : nullptr, g_block_verify, g_tick_seq, g_memo});
    hqhost::Counts cnt;
    const bool one_rank = g_xfn && g_xworld > 1;  // this call is one rank of a sharded scheduler
    auto solve = [&](bool defer, bool classic) -> int {
        pb.defer_row_check = defer; pb.no_fast_path = classic;
        if (one_rank) {
            hqsolve::FnExchange xch(g_xfn, g_xuser, g_xrank, g_xworld);
            cnt = hqsolve::run_solver(pb, batches, &xch, g_xmin_classes, g_xmin_blocks);
            g_xcalls = (uint32_t)xch.n_calls;
        } else cnt = hqsolve::run_solver(pb, batches, nullptr, 0, 0);
        return 0;
    };
    // hqtick_debug_set_defer_row_check(1): the row check of a fast-path placement is this caller's, as in a tick (TickRun::run) — run behind the solver, and a failure
    // sends the model down the classic path in a second call.  Never as a rank of a sharded scheduler, like the tick.  Nothing but the counts rests on a pass here.
    hqstages::with_row_check(cnt, hqmilp::g_check_hook && hqmilp::g_check_hook->allow == 1 && !one_rank, solve, []() { return 0; });
    if (cnt.error) { h.err = cnt.errmsg; return cnt.error; }
    g_last_guard[0] = cnt.blocks_verified; g_last_guard[1] = cnt.blocks_mismatch; g_last_guard[2] = cnt.blocks_rejected;
    g_last_memo = cnt.blocks_memo;
    g_last_blocks_device = cnt.blocks_device; g_last_blocks_host = cnt.blocks_host; g_last_price_sweeps = (uint32_t)cnt.price_sweeps; g_last_price_rounds = (uint32_t)cnt.price_rounds;
    g_last_stage_us[0] = cnt.t_classify_us; g_last_stage_us[1] = cnt.t_blocks_us; g_last_stage_us[2] = cnt.t_decode_us;
    for (size_t i = 0; i < cnt.mn_rq.size(); i++)
        for (auto &set : cnt.mn_sets[i]) { g_last_mn_rq.push_back(cnt.mn_rq[i]); g_last_mn_worker.insert(g_last_mn_worker.end(), set.begin(), set.end()); g_last_mn_off.push_back((uint32_t)g_last_mn_worker.size()); }
    hqmap::HostResult &hr = h.res;
    hr.cnt_rq.clear(); hr.cnt_variant.clear(); hr.cnt_worker.clear(); hr.cnt_value.clear();
    cnt.pairs();
    for (size_t k = 0; k < cnt.keys.size(); k++)
        for (auto &wc : cnt.per_key[k]) { hr.cnt_rq.push_back(cnt.keys[k].first); hr.cnt_variant.push_back(cnt.keys[k].second); hr.cnt_worker.push_back(wc.first); hr.cnt_value.push_back(wc.second); }
    out->is_optimal = cnt.is_optimal; out->is_canonical = cnt.is_canonical && cnt.is_optimal;
    out->status = hqsolve::tick_status(cnt);
    if (with_plan) {  // (plan_keys writes the counts itself: the same rows, in the same order)
        static thread_local std::vector<uint32_t> tables;
        uint64_t N = 0;
        for (size_t g = 0; g < sc.hist.size(); g++) N += sc.hist[g];
        hqmap::PlanIn in = hqstages::plan_in(sc, cnt, s, pb, *config, N, retr_key, retr_rank);
        in.storage = heap_storage; in.user = &tables;
        const char *why = nullptr;
        if (int rc = hqstages::plan_stages(h.plan, hr, in, &why, [](int) { return 0; })) { h.err = why; return rc; }
        hqmap::assemble_host_part(h.plan, hr, in);
        out->rec_off = hr.rec_off.data(); out->retract_off = hr.retract_off.data(); out->retract_task = hr.retract_task.data();
        out->n_redirects = (uint32_t)hr.red_task.size(); out->redirect_task = hr.red_task.data(); out->redirect_worker = hr.red_worker.data();
        out->redirect_variant = hr.red_variant.data(); out->redirect_kind = hr.red_kind.data(); out->new_free = hr.new_free.data();
    }
    out->n_counts = (uint32_t)hr.cnt_rq.size(); out->count_rq = hr.cnt_rq.data(); out->count_variant = hr.cnt_variant.data();
    out->count_worker = hr.cnt_worker.data(); out->count_value = hr.cnt_value.data();
    return out->status;
}

// the view hqtick_debug_order_view last built, if ctx's columns are still the ones it was built on
ViewHooks *debug_view_of(hqtick_ctx *ctx) {
    ViewHooks *v = ctx->view_hooks;
    if (!v || !v->valid || !ctx->ready.resident() || v->ids != ctx->ready.cols().id || v->N != ctx->ready.cols().n) return nullptr;
    return v;
}

}  // namespace

extern "C" {

void hqtick_debug_set_block_guard(uint32_t verify, uint32_t tick_seq, int corrupt_mode, uint32_t corrupt_class, uint32_t corrupt_fill) {
    g_block_verify = verify; g_tick_seq = tick_seq; g_corrupt_mode = corrupt_mode; g_corrupt_class = corrupt_class; g_corrupt_fill = corrupt_fill;
}
void hqtick_debug_last_block_guard(uint32_t *verified, uint32_t *mismatch, uint32_t *rejected) {
    if (verified) *verified = g_last_guard[0]; if (mismatch) *mismatch = g_last_guard[1]; if (rejected) *rejected = g_last_guard[2];
}
void hqtick_debug_set_block_memo(int on) { if (on && !g_memo) g_memo = new hqhost::BlockMemo(); if (!on) { delete g_memo; g_memo = nullptr; } }
uint32_t hqtick_debug_last_block_memo(void) { return g_last_memo; }
void hqtick_debug_set_price_emulation(int on, uint32_t min_cols) { g_price_emulation = on; g_price_min_cols = min_cols; }
void hqtick_debug_set_fast_path(int on) { hqmilp::set_fast_path(on); }
void hqtick_debug_check_model_hints(int on) { hqprice::set_check_hints(on != 0); }
int hqtick_debug_model_hint_mismatches(void) { return hqprice::hint_mismatches(); }
void hqtick_debug_set_price_fault(int fail_at) { g_price_fault = fail_at; }
void hqtick_debug_set_exchange(hqtick_exchange_fn fn, void *user, uint32_t rank, uint32_t world, uint32_t min_blocks, uint32_t min_classes) {
    g_xfn = fn; g_xuser = user; g_xrank = rank; g_xworld = world ? world : 1; g_xmin_blocks = min_blocks; g_xmin_classes = min_classes;
}
uint32_t hqtick_debug_last_exchange_calls(void) { return g_xcalls; }
void hqtick_debug_last_stage_us(double *out3) { if (out3) for (int i = 0; i < 3; i++) out3[i] = g_last_stage_us[i]; }
void hqtick_debug_last_price(uint32_t *sweeps, uint32_t *rounds) { if (sweeps) *sweeps = g_last_price_sweeps; if (rounds) *rounds = g_last_price_rounds; }
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

int hqtick_debug_host_stages(const hqtick_config *config, const hqtick_snapshot *s, const uint8_t *vflags, const uint32_t *vtmc, uint32_t n_levels,
                             const uint64_t *levels, const uint32_t *hist, hqtick_result *out) {
    return host_stages(config, s, vflags, vtmc, n_levels, levels, hist, false, nullptr, nullptr, out);
}
int hqtick_debug_host_plan(const hqtick_config *config, const hqtick_snapshot *s, const uint8_t *vflags, const uint32_t *vtmc, uint32_t n_levels, const uint64_t *levels,
                           const uint32_t *hist, const uint32_t *retracting_key, const uint32_t *retracting_rank, hqtick_result *out, const char **error) {
    static thread_local std::string text;  // (the refusal's text outlives the thread's next host hook)
    if (error) *error = "";
    if (s && s->n_retracting && (!retracting_key || !retracting_rank)) return HQTICK_E_INVALID;
    const int rc = host_stages(config, s, vflags, vtmc, n_levels, levels, hist, true, retracting_key, retracting_rank, out);
    text = g_hold.err;
    if (rc < 0 && error) *error = text.c_str();
    return rc;
}

// The tail of a query on caller-supplied scan outputs, with the solver run_scheduling_solver and, under hqtick_debug_set_block_emulation, the emulated blocks from one
// class up: no sweeper, no memo, no verification knob (the product's query goes through Solver::solve's wiring).
int hqtick_debug_host_query(const hqtick_config *config, const hqtick_snapshot *s, const hqtick_query_workers *fake, const uint8_t *vflags, const uint32_t *vtmc,
                            const uint8_t *fake_vflags, const uint32_t *fake_vtmc, uint32_t n_levels, const uint64_t *levels, const uint32_t *hist,
                            hqtick_query_result *out) {
    if (!config || !s || !fake || !out) return HQTICK_E_INVALID;
    HostHold &h = g_hold;
    if (int rc = hqstages::validate(s, false, h.err)) return rc;
    WorkerEval ev; ev.flags = vflags; ev.tmc = vtmc;
    WorkerEval ev_fake; ev_fake.flags = fake_vflags; ev_fake.tmc = fake_vtmc;
    const hqscan::Table sc = hqstages::table_from_hist(n_levels, levels, hist, s->n_requests);
    auto solve = [&](hqhost::Problem &pb, const std::vector<hqhost::TaskBatch> &batches) {
        hqsolve::EmulatedBlocks emu(g_block_budget);
        if (g_block_emulation) { pb.blocks = &emu; pb.block_min_classes = 1; }
        return hqhost::run_scheduling_solver(pb, batches);
    };
    return hqstages::query_tail(*config, s, fake, ev, ev_fake, sc, solve, h.loaded, out, h.err);
}

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

// one all-gather of a host buffer through the library's RCCL communicator, as the sharded solve issues it per sweep — for the single-rank round trip of the GPU
// suite (recv == send) and for timing the exchange's fixed cost (H2D + ncclAllGather + D2H + one stream synchronisation)
int hqtick_debug_exchange(hqtick_ctx *ctx, const void *send, void *recv, size_t bytes_per_rank) {
    if (!ctx || !send || !recv) return HQTICK_E_INVALID;
    if (!ctx->solver.has_comm()) return fail(ctx, HQTICK_E_INVALID, "hqtick_debug_exchange without hqtick_comm_init");
    return ctx->solver.allgather_host(solve_env(ctx), send, recv, bytes_per_rank) ? 0 : fail(ctx, HQTICK_E_DEVICE, "the RCCL exchange failed");
}

}  // extern "C"

// The host stages of a tick with no HIP in sight: what the tick (hqtick.cpp: TickRun::run), the two queries and the CPU test hooks
// (debug_tick.cpp: hqtick_debug_host_stages, _host_plan, _host_query) all run — each piece defined here once — and what tools/tick_core_asan.cpp checks with no GPU
// and no Python.
//   validate         the snapshot's argument checks, with the refusal's text
//   fill_problem     snapshot + K2's output -> the solver's Problem
//   table_from_hist  a dense (level, request) histogram as the scan table the stages walk
//   queue_levels     TaskQueue::iter_priority_sizes per request, from the table and the prefill sets
//   export_batches   the batches as the result's flat arrays (BatchExport owns them)
//   plan_in          what the mapping plan reads, as far as every caller sets it alike
//   plan_stages      the four stages of the plan (map_core.h) in order, the caller's `after` behind each
//   with_row_check   the deferred row check's retry: a pass, the check if nobody has run it, and on its failure one classic pass
//   query_tail       the model over a query's fake workers, the caller's solve, and which of them it loaded
// Where two callers differ, the difference is an argument (a callable, a flag); nothing here asks who calls.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/hqtick.h"
#include "host_model.h"
#include "map_core.h"
#include "scan_core.h"
#include "solve_core.h"

namespace hqstages {

using hqscan::Table;
using hqscan::WorkerEval;

// 0, or HQTICK_E_INVALID with the reason in err.  need_tasks: the snapshot carries the ready set's columns (a tick on a resident set does not).
inline int validate(const hqtick_snapshot *s, bool need_tasks, std::string &err) {
    auto no = [&](const char *why) { err = why; return (int)HQTICK_E_INVALID; };
    if (!s) return no("null snapshot");
    if (s->n_workers && (!s->worker_id || !s->worker_total || !s->worker_free)) return no("worker arrays missing");
    for (uint32_t w = 1; w < s->n_workers; w++) if (s->worker_id[w - 1] >= s->worker_id[w]) return no("worker ids not ascending");
    if (s->n_requests && (!s->rq_variant_off || !s->variant_entry_off)) return no("request arrays missing");
    for (uint32_t q = 0; q < s->n_requests; q++) {
        if (s->rq_variant_off[q + 1] <= s->rq_variant_off[q]) return no("request without variants");
        if (s->rq_variant_off[q + 1] - s->rq_variant_off[q] > 32) return no("more than 32 variants");
    }
    uint32_t nv = s->n_requests ? s->rq_variant_off[s->n_requests] : 0;
    for (uint32_t e = 0; e < (nv ? s->variant_entry_off[nv] : 0); e++) {
        if (s->entry_resource[e] >= s->n_resources) return no("entry resource id out of range");
        if (s->entry_kind[e] == HQ_ENTRY_AMOUNT && s->entry_amount[e] == 0) return no("zero amount request");
    }
    if (need_tasks && s->n_ready) {
        if (!s->task_id || !s->task_priority || !s->task_rq) return no("ready-set columns missing");
        for (uint64_t i = 1; i < s->n_ready; i++) if (s->task_id[i - 1] >= s->task_id[i]) return no("ready set not sorted by task id");
    }
    if (s->n_blocked && (!s->blocked_worker || !s->blocked_rq || !s->blocked_variant)) return no("blocked arrays missing");
    for (uint32_t k = 0; k < s->n_blocked; k++) {
        if (s->blocked_worker[k] >= s->n_workers) return no("blocked worker index");
        if (s->blocked_rq[k] >= s->n_requests) return no("blocked request id out of range");
        if (s->blocked_variant[k] >= s->rq_variant_off[s->blocked_rq[k] + 1] - s->rq_variant_off[s->blocked_rq[k]]) return no("blocked variant out of range");
    }
    if (s->worker_group) for (uint32_t w = 0; w < s->n_workers; w++) if (s->worker_group[w] >= (s->n_groups ? s->n_groups : 1)) return no("worker_group >= n_groups");
    // CSR offsets: monotone, and their arrays present.  (The ENTRIES of assigned_* are checked where they are dereferenced — the gap rows of a
    // tick with priority cuts, host_model.cpp — so that the common tick does not pay a pass over every running task.)
    if (s->assigned_off) {
        for (uint32_t w = 0; w < s->n_workers; w++) if (s->assigned_off[w] > s->assigned_off[w + 1]) return no("assigned_off not monotone");
        if (s->n_workers && s->assigned_off[s->n_workers] && (!s->assigned_rq || !s->assigned_variant)) return no("assigned arrays missing");
    }
    if (s->prefilled_off) {
        for (uint32_t w = 0; w < s->n_workers; w++) if (s->prefilled_off[w] > s->prefilled_off[w + 1]) return no("prefilled_off not monotone");
        if (s->n_workers && s->prefilled_off[s->n_workers] && !s->prefilled_rq) return no("prefilled_rq missing");
    }
    if (s->prefill_off) {
        for (uint32_t q = 0; q < s->n_requests; q++) if (s->prefill_off[q] > s->prefill_off[q + 1]) return no("prefill_off not monotone");
        const uint32_t np = s->n_requests ? s->prefill_off[s->n_requests] : 0;
        if (np && (!s->prefill_priority || !s->prefill_task || !s->prefill_worker)) return no("prefill arrays missing");
        for (uint32_t i = 0; i < np; i++) if (s->prefill_worker[i] >= s->n_workers) return no("prefill worker index");
    }
    if (s->n_retracting && (!s->retracting_task || !s->retracting_worker)) return no("retracting arrays missing");
    for (uint32_t k = 0; k < s->n_retracting; k++) {
        if (s->retracting_worker[k] >= s->n_workers) return no("retracting worker index");
        if (k && s->retracting_task[k - 1] >= s->retracting_task[k]) return no("retracting tasks not ascending");
        if (s->retracting_redirect_worker && s->retracting_redirect_worker[k] != HQ_NO_WORKER && s->retracting_redirect_worker[k] >= s->n_workers) return no("retracting redirect worker index");
    }
    return 0;
}

inline void fill_problem(hqhost::Problem &pb, const hqtick_snapshot *s, const hqtick_config &cfg, const WorkerEval &ev) {
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

// the table of a dense histogram hist[level * Q + rq] over n_levels priorities (descending), as GPU phase A would have left it
inline Table table_from_hist(uint32_t n_levels, const uint64_t *levels, const uint32_t *hist, uint32_t Q) {
    Table sc;
    sc.Q = Q; sc.L = n_levels; sc.G = n_levels * Q;
    if (n_levels) sc.levels.assign(levels, levels + n_levels);
    if (sc.G) sc.hist.assign(hist, hist + (size_t)n_levels * Q);
    hqscan::runs_from_hist(sc);
    return sc;
}

// TaskQueue::iter_priority_sizes (taskqueue.rs:273-302) for every request, from the table's runs and the prefill sets
inline std::vector<hqhost::QueueLevels> queue_levels(const Table &sc, const hqtick_snapshot *s) {
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

// The batches as hqtick_result hands them out: per batch its columns and its cuts [b_cut_off], per cut its size and its blockers [c_bl_off].  The arrays live
// here; the result points into them until the next export.
struct BatchExport {
    std::vector<uint32_t> b_rq, b_size, b_limit, b_cut_off, c_size, c_bl_off, bl_rq, bl_size; std::vector<uint8_t> b_lr, b_blk;
};
inline void export_batches(const std::vector<hqhost::TaskBatch> &batches, BatchExport &x, hqtick_result *out) {
    x.b_rq.clear(); x.b_size.clear(); x.b_limit.clear(); x.b_lr.clear(); x.b_blk.clear();
    x.b_cut_off.assign(1, 0); x.c_size.clear(); x.c_bl_off.assign(1, 0); x.bl_rq.clear(); x.bl_size.clear();
    for (auto &b : batches) {
        x.b_rq.push_back(b.rq); x.b_size.push_back(b.size); x.b_limit.push_back(b.limit); x.b_lr.push_back(b.limit_reached); x.b_blk.push_back(b.is_blocker);
        for (auto &c : b.cuts) {
            x.c_size.push_back(c.size);
            for (auto &bl : c.blockers) { x.bl_rq.push_back(bl.first); x.bl_size.push_back(bl.second); }
            x.c_bl_off.push_back((uint32_t)x.bl_rq.size());
        }
        x.b_cut_off.push_back((uint32_t)x.c_size.size());
    }
    out->n_batches = (uint32_t)x.b_rq.size(); out->batch_rq = x.b_rq.data(); out->batch_size = x.b_size.data(); out->batch_limit = x.b_limit.data();
    out->batch_limit_reached = x.b_lr.data(); out->batch_is_blocker = x.b_blk.data(); out->batch_cut_off = x.b_cut_off.data();
    out->cut_size = x.c_size.data(); out->cut_blocker_off = x.c_bl_off.data(); out->blocker_rq = x.bl_rq.data(); out->blocker_size = x.bl_size.data();
}

inline bool transpose_enabled() { const char *e = getenv("HQTICK_TRANSPOSE"); return !(e && atoi(e) == 0); }

// What the plan reads (map_core.h) as every caller sets it: the table, the counts, the snapshot, the request views, the config's values, the ready set's slots and
// the Retracting tasks' (key, rank) arrays — one scheduler, no sink, no ledger.  The caller adds its storage, and the tick its sink, shard and ledger fields.
inline hqmap::PlanIn plan_in(const Table &sc, hqhost::Counts &cnt, const hqtick_snapshot *s, const hqhost::Problem &pb, const hqtick_config &cfg, uint64_t N,
                             const uint32_t *retr_key, const uint32_t *retr_rank) {
    hqmap::PlanIn in{};
    in.sc = &sc; in.cnt = &cnt; in.s = s; in.rqs = pb.rqs.data(); in.variants = pb.variants.data();
    in.proactive_filling_reserve = cfg.proactive_filling_reserve; in.proactive_filling_max = cfg.proactive_filling_max; in.flags = cfg.flags;
    in.shard_count = 1;
    in.N = N; in.retr_key = retr_key; in.retr_rank = retr_rank;
    in.transpose_on = transpose_enabled();
    return in;
}

// The plan's four stages in order: keys (0), redirects (1), prefill (2), outputs (3).  A stage that refuses ends the sequence with its code and *why set;
// after(i) runs behind stage i, and a non-zero answer of it ends the sequence with that code (*why is then left alone).
template <class After> inline int plan_stages(hqmap::Plan &ps, hqmap::HostResult &hr, const hqmap::PlanIn &in, const char **why, After &&after) {
    int rc;
    if ((rc = hqmap::plan_keys(ps, hr, in, why)) || (rc = after(0))) return rc;
    if ((rc = hqmap::plan_redirects(ps, hr, in, why)) || (rc = after(1))) return rc;
    if ((rc = hqmap::plan_prefill(ps, hr, in, why)) || (rc = after(2))) return rc;
    if ((rc = hqmap::plan_outputs(ps, hr, in, why)) || (rc = after(3))) return rc;
    return 0;
}

// The retry around a deferred row check.  pass(defer, classic) solves into cnt — with `defer`, a fast-path placement may come back with its
// check pending (Counts::row_check_pending) — and does whatever else rests on the counts; it may settle the check itself, or hand it to somebody who does.  A check
// still pending when the pass returns is settled here, whatever the pass returned: the check decides whether its result, an error included, stands.  A failed
// check voids the pass: discard() takes back what it left (non-zero: give up with that code), cnt is reset, and pass(false, true) runs once, on the classic path.
template <class Pass, class Discard> inline int with_row_check(hqhost::Counts &cnt, bool defer, Pass &&pass, Discard &&discard) {
    const int rc = pass(defer, false);
    if (cnt.row_check_pending()) cnt.settle_row_check();
    if (!cnt.row_check_failed()) return rc;
    if (const int drc = discard()) return drc;
    cnt = hqhost::Counts();
    return pass(false, true);
}

// The tail of a what-if query (query.rs:73-81): the model over the fake workers K2 has evaluated (fresh: free == total), batches from the table's runs,
// solve(pb, batches) — the caller's, with its own solver wiring — and which of the fake workers it loaded.  `loaded` owns what out->is_loaded points to.
template <class Solve>
inline int query_tail(const hqtick_config &cfg, const hqtick_snapshot *s, const hqtick_query_workers *fake, const WorkerEval &ev_real, const WorkerEval &ev_fake, const Table &sc,
                      Solve &&solve, std::vector<uint8_t> &loaded, hqtick_query_result *out, std::string &err) {
    const uint32_t Q = s->n_requests;
    hqhost::Problem pb;
    fill_problem(pb, s, cfg, ev_real);
    hqhost::WorkerSet fw;
    hqsolve::fake_worker_set(fw, fake, s->n_resources, ev_fake.flags, ev_fake.tmc, Q ? s->rq_variant_off[Q] : 0);
    hqhost::group_equal_rows(fw, true);
    pb.custom = &fw;
    std::vector<hqhost::QueueLevels> qlv = queue_levels(sc, s);
    std::vector<hqhost::TaskBatch> batches = hqhost::create_task_batches(pb, qlv);
    hqhost::Counts cnt = solve(pb, batches);
    if (cnt.error) { err = cnt.errmsg; return cnt.error; }
    hqsolve::loaded_flags(cnt, fake->n_workers, loaded);
    out->n_workers = fake->n_workers; out->is_loaded = loaded.data(); out->is_optimal = cnt.is_optimal;
    return 0;
}

}  // namespace hqstages

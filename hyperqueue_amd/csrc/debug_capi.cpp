// Test hooks declared in include/hqtick_debug.h: host-side building blocks that can be unit-tested without a GPU.
// They are NOT a CPU implementation of the tick (hqtick_run has none): only the exact MILP solver and the
// hashbrown-order helper are reachable here.
#include "../../include/hqtick_debug.h"

#include <algorithm>
#include <cstring>

#include "audit_core.h"
#include "cancel_core.h"
#include "clock_core.h"
#include "fail_core.h"
#include "finish_core.h"
#include "lose_core.h"
#include "start_core.h"
#include "reject_core.h"
#include "hb_order.h"
#include "milp.h"
#include "price_emul.h"

static thread_local int g_last_canonical = 0;
static thread_local long g_last_hull[2] = {0, 0};
extern "C" int hqtick_debug_milp_was_canonical(void) { return g_last_canonical; }
extern "C" void hqtick_debug_milp_last_hull(long *solves, long *nonpacking) {
    if (solves) *solves = g_last_hull[0];
    if (nonpacking) *nonpacking = g_last_hull[1];
}

extern "C" int hqtick_debug_milp_solve(int ncols, const double *obj, const uint8_t *col_kind, int nrows, const uint8_t *row_type,
                                       const double *rhs, const int *row_off, const int *row_col, const double *row_coef,
                                       double time_limit_s, int canonical, double *x_out, double *obj_out, int *is_optimal,
                                       long *nodes_out) {
    hqmilp::Model m;
    m.obj.assign(obj, obj + ncols);
    m.kind.assign(col_kind, col_kind + ncols);
    m.rtype.assign(row_type, row_type + nrows);
    m.rhs.assign(rhs, rhs + nrows);
    m.roff.assign(row_off, row_off + nrows + 1);
    int nnz = nrows ? row_off[nrows] : 0;
    m.rcol.assign(row_col, row_col + nnz);
    m.rcoef.assign(row_coef, row_coef + nnz);
    hqmilp::Result r = hqmilp::solve(m, time_limit_s, canonical != 0);
    g_last_canonical = r.canonical ? 1 : 0;
    g_last_hull[0] = r.hull_solves; g_last_hull[1] = r.hull_solves_nonpacking;
    if (nodes_out) *nodes_out = r.nodes;
    if (!r.feasible) return 0;
    for (int j = 0; j < ncols; j++) x_out[j] = r.x[j];
    *obj_out = r.objective;
    *is_optimal = r.optimal ? 1 : 0;
    return 1;
}

extern "C" void hqtick_debug_map_order_u32(const uint32_t *keys, uint32_t n, uint32_t *out_pos) {
    std::vector<uint32_t> order;
    hqhb::insertion_order_u32(keys, n, order);
    for (uint32_t i = 0; i < n; i++) out_pos[i] = order[i];
}

// The solver on a model that carries the builder's structure hints, with the price sweeps of the coupled solve run through the emulated wavefront
// (csrc/price_emul.cpp): the CPU tests' way into csrc/price.cpp + csrc/price_core.h.  col_group / row_implied may be null; min_cols = smallest
// component the sweeps take (0: the default).  stats_out[4] (optional): sweeps, rounds, certified-by-sweeps flag (sweeps > 0 and optimal), canonical.
extern "C" int hqtick_debug_milp_solve_priced(int ncols, const double *obj, const uint8_t *col_kind, const int32_t *col_group, int nrows, const uint8_t *row_type,
                                              const uint8_t *row_implied, const double *rhs, const int *row_off, const int *row_col, const double *row_coef,
                                              double time_limit_s, int use_sweeps, uint32_t min_cols, double *x_out, double *obj_out, int *is_optimal, double *stats_out) {
    hqmilp::Model m;
    m.obj.assign(obj, obj + ncols);
    m.kind.assign(col_kind, col_kind + ncols);
    m.rtype.assign(row_type, row_type + nrows);
    m.rhs.assign(rhs, rhs + nrows);
    m.roff.assign(row_off, row_off + nrows + 1);
    int nnz = nrows ? row_off[nrows] : 0;
    m.rcol.assign(row_col, row_col + nnz);
    m.rcoef.assign(row_coef, row_coef + nnz);
    if (col_group) m.col_group.assign(col_group, col_group + ncols);
    if (row_implied) m.row_implied.assign(row_implied, row_implied + nrows);
    hqprice::EmulatedSweeper emu;
    if (min_cols) emu.min_cols = min_cols;
    hqmilp::Result r = hqmilp::solve(m, time_limit_s, true, hqmilp::REFERENCE_MIP_REL_GAP, use_sweeps ? &emu : nullptr);
    g_last_canonical = r.canonical ? 1 : 0;
    g_last_hull[0] = r.hull_solves; g_last_hull[1] = r.hull_solves_nonpacking;
    if (stats_out) { stats_out[0] = r.price_sweeps; stats_out[1] = r.price_rounds; stats_out[2] = r.price_total_us; stats_out[3] = r.canonical ? 1.0 : 0.0; }
    if (!r.feasible) return 0;
    for (int j = 0; j < ncols; j++) x_out[j] = r.x[j];
    *obj_out = r.objective;
    *is_optimal = r.optimal ? 1 : 0;
    return 1;
}

// Equal-block runs of the coupled model (csrc/milp.h: Model::block_runs).  The probe the builder and the flattener write into is installed on this thread by
// hqtick_debug_set_block_runs(0 / 1) and taken away again by hqtick_debug_set_block_runs(-1).
static thread_local hqmilp::Probe g_block_run_probe;
extern "C" void hqtick_debug_set_block_runs(int on) {
    hqmilp::g_probe = on < 0 ? nullptr : &g_block_run_probe; hqmilp::set_block_runs(on);
    if (on >= 0) { g_block_run_probe.model = g_block_run_probe.tables = g_block_run_probe.runs = g_block_run_probe.covered = 0; }   // (a tick that builds no coupled model leaves zeros)
}
extern "C" void hqtick_debug_corrupt_block_runs(int on) { g_block_run_probe.corrupt_runs = on != 0; }
extern "C" void hqtick_debug_last_coupled_digest(uint64_t out[4]) {
    out[0] = g_block_run_probe.model; out[1] = g_block_run_probe.tables; out[2] = g_block_run_probe.runs; out[3] = g_block_run_probe.covered;
}
// The zero-price sweep launched from inside the flattening (csrc/price.h: set_early_sweep) and the first cut of this thread's coupled solves (capture_first_cut).
extern "C" void hqtick_debug_set_early_sweep(int on) { hqprice::set_early_sweep(on); }
extern "C" uint32_t hqtick_debug_early_sweeps(void) { return hqprice::early_sweeps(); }
extern "C" void hqtick_debug_capture_first_cut(int on) { hqprice::capture_first_cut(on != 0); }
extern "C" uint32_t hqtick_debug_first_cut(unsigned char *out, uint32_t cap) {
    const std::vector<unsigned char> &b = hqprice::first_cut_bytes();
    if (out && cap) memcpy(out, b.data(), std::min<size_t>(cap, b.size()));
    return (uint32_t)b.size();
}

// The fast path's row check deferred into phase C's window (csrc/milp.h: CheckHook).  Any of the three installs the hook on this thread; it stays.
static thread_local hqmilp::CheckHook g_row_check_hook;
static hqmilp::CheckHook &row_check_hook() { hqmilp::g_check_hook = &g_row_check_hook; return g_row_check_hook; }
extern "C" void hqtick_debug_set_defer_row_check(int on) { row_check_hook().allow = on; }
extern "C" uint32_t hqtick_debug_deferred_row_checks(int clear) { hqmilp::CheckHook &h = row_check_hook(); const uint32_t n = h.deferred; if (clear) h.deferred = 0; return n; }
extern "C" uint32_t hqtick_debug_fail_row_checks(uint32_t n) { hqmilp::CheckHook &h = row_check_hook(); const uint32_t left = h.fail_next; h.fail_next = n; return left; }

// clock mode: the phase function of k_clock_rows over arrays, in the linear form the kernel folds and in the sorted form of the host mirror
extern "C" int hqtick_debug_clock_rows(uint32_t n, const int64_t *deadline_ns, int64_t now_ns, uint32_t nv, const uint64_t *min_time_ns, int sorted_form, int64_t *remaining_out) {
    if ((n && (!deadline_ns || !remaining_out)) || (nv && !min_time_ns)) return HQTICK_E_INVALID;
    if (!sorted_form) {
        for (uint32_t w = 0; w < n; w++) {  // the table in chunks, as the kernel stages it
            if (deadline_ns[w] == hqclock::NO_LIMIT) { remaining_out[w] = hqclock::NO_LIMIT; continue; }
            const int64_t r = hqclock::sat_sub(deadline_ns[w], now_ns);
            uint64_t best = 0;
            for (uint32_t v0 = 0; r >= 0 && v0 < nv; v0 += hqclock::CHUNK) best = hqclock::fold_thresholds(best, r, min_time_ns + v0, std::min(hqclock::CHUNK, nv - v0));
            remaining_out[w] = r < 0 ? -1 : (int64_t)best;
        }
        return 0;
    }
    std::vector<uint64_t> thr(min_time_ns, min_time_ns + nv);
    std::sort(thr.begin(), thr.end()); thr.erase(std::unique(thr.begin(), thr.end()), thr.end());
    for (uint32_t w = 0; w < n; w++) remaining_out[w] = hqclock::canonical_sorted(deadline_ns[w], now_ns, thr.data(), (uint32_t)thr.size());
    return 0;
}
// the audit of the resident state on host arrays: audit_core.h's host backend
extern "C" int hqtick_debug_audit_host(const hqtick_debug_audit_tables *a, uint32_t parts, int order, hqtick_check_report *out) {
    if (!a || !out || (parts & ~(HQ_CHECK_ALL | HQ_CHECK_STRICT)) || order < 0 || order > 2 || (a->have & ~31u)) return HQTICK_E_INVALID;
    hqaudit::State S{};
    S.have = a->have; S.parts = parts;
    S.ready = hqaudit::Ready{a->ready_id, a->ready_rq, a->ready_n};
    S.graph = hqaudit::Graph{a->g_id, a->g_unfinished, a->g_gen, a->g_head, a->g_ht_key, a->g_ht_val, a->g_ht_mask, a->g_run_next, a->g_run_off, a->g_run_len, a->g_edge,
                             a->g_slots, a->g_runs, a->g_edges, a->g_tasks};
    S.ledger = hqaudit::Ledger{a->l_key, a->l_worker, a->l_rq, a->l_variant, a->l_mask, a->l_rq_off, a->l_ventry_off, a->l_ent_res, a->l_var_nodes, a->l_ent_kind, a->l_ent_amount,
                               a->l_Q, a->l_NV, a->l_wid, a->l_W, a->l_R, a->l_total, a->l_free, a->l_counts, a->l_stride, a->l_pf, a->l_pf_stride, a->l_mn_task, a->l_mn_root,
                               a->l_flags, a->l_n_live, a->l_mn_live, a->l_pf_live};
    S.retr = hqaudit::Retr{a->r_task, a->r_target, a->r_variant, a->r_flags, a->r_n};
    const hqaudit::Totals t{a->ready_live, a->g_tasks, a->g_free, a->g_slots};
    hqaudit::run_host(S, t, order, out);
    return (int)out->n_failed;
}
extern "C" int64_t hqtick_debug_clock_deadline(int64_t now_ns, int64_t remaining_ns) { return hqclock::deadline_of(now_ns, remaining_ns); }
extern "C" int64_t hqtick_debug_clock_remaining(int64_t deadline_ns, int64_t now_ns) { return hqclock::remaining_of(deadline_ns, now_ns); }
// the grouping of a cancel batch on host arrays: cancel_core.h's phases in the given thread order
extern "C" int hqtick_debug_cancel_group(uint32_t n, uint32_t W, const uint32_t *route_row, const uint64_t *task_id, const uint32_t *worker_id, int order, uint32_t *n_workers,
                                         uint32_t *out_worker, uint32_t *out_off, uint64_t *out_task) {
    if (!n_workers || !out_off || (n && (!route_row || !task_id || !out_task)) || (W && (!worker_id || !out_worker)) || order < 0 || order > 2 || n > 0x7FFFFFFFu) return HQTICK_E_INVALID;
    uint32_t n_ids = 0;
    if (!hqcancel::group_on_host(n, W, route_row, task_id, worker_id, order, n_workers, &n_ids, out_worker, out_off, out_task)) return HQTICK_E_DEVICE;
    return (int)n_ids;
}
// the rule of hqtick_finish_tasks on host arrays: finish_core.h's kind_of per position
extern "C" int hqtick_debug_finish_kind(uint32_t n, const uint8_t *entry_found, const uint8_t *entry_class, const uint8_t *entry_worker_match, const uint8_t *override_found,
                                        const uint8_t *override_worker_match, const uint8_t *earlier_accepted, uint8_t *kind) {
    if (n && (!entry_found || !entry_class || !entry_worker_match || !override_found || !override_worker_match || !earlier_accepted || !kind)) return HQTICK_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        if (entry_class[i] > hqfinish::E_PF) return HQTICK_E_INVALID;
        kind[i] = (uint8_t)hqfinish::kind_of(entry_found[i] != 0, entry_class[i], entry_worker_match[i] != 0, override_found[i] != 0, override_worker_match[i] != 0, earlier_accepted[i] != 0);
    }
    return (int)n;
}
// the rule of hqtick_fail_tasks on host arrays: fail_core.h's kind_of per position
extern "C" int hqtick_debug_fail_kind(uint32_t n, const uint8_t *entry_found, const uint8_t *entry_class, const uint8_t *entry_worker_match, const uint8_t *override_found,
                                      const uint8_t *override_worker_match, const uint8_t *reporter_none, const uint8_t *earlier_accepted, uint8_t *kind) {
    if (n && (!entry_found || !entry_class || !entry_worker_match || !override_found || !override_worker_match || !reporter_none || !earlier_accepted || !kind)) return HQTICK_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        if (entry_class[i] > hqfail::E_PF) return HQTICK_E_INVALID;
        kind[i] = (uint8_t)hqfail::kind_of(entry_found[i] != 0, entry_class[i], entry_worker_match[i] != 0, override_found[i] != 0, override_worker_match[i] != 0, reporter_none[i] != 0,
                                           earlier_accepted[i] != 0);
    }
    return (int)n;
}
// the rule of hqtick_start_tasks on host arrays: start_core.h's kind_of per position
extern "C" int hqtick_debug_start_kind(uint32_t n, const uint8_t *entry_found, const uint8_t *entry_class, const uint8_t *entry_worker_match, const uint8_t *entry_variant_match,
                                       const uint8_t *entry_run, const uint8_t *variant_exists, const uint8_t *override_found, const uint8_t *override_worker_match,
                                       const uint8_t *earlier_eligible, uint8_t *kind) {
    if (n && (!entry_found || !entry_class || !entry_worker_match || !entry_variant_match || !entry_run || !variant_exists || !override_found || !override_worker_match || !earlier_eligible || !kind))
        return HQTICK_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        if (entry_class[i] > hqstart::E_PF) return HQTICK_E_INVALID;
        kind[i] = (uint8_t)hqstart::kind_of(entry_found[i] != 0, entry_class[i], entry_worker_match[i] != 0, entry_variant_match[i] != 0, entry_run[i] != 0, variant_exists[i] != 0,
                                            override_found[i] != 0, override_worker_match[i] != 0, earlier_eligible[i] != 0);
    }
    return (int)n;
}
// the rule of hqtick_reject_tasks on host arrays: reject_core.h's kind_of and blocks per position
extern "C" int hqtick_debug_reject_kind(uint32_t n, const uint8_t *entry_found, const uint8_t *entry_class, const uint8_t *entry_worker_match, const uint8_t *entry_variant_match,
                                        const uint8_t *entry_run, const uint8_t *variant_none, const uint8_t *variant_exists, const uint8_t *override_found,
                                        const uint8_t *override_worker_match, const uint8_t *override_redirect, const uint8_t *earlier_eligible, const uint8_t *reporter_resident,
                                        uint8_t *kind, uint8_t *blocks) {
    if (n && (!entry_found || !entry_class || !entry_worker_match || !entry_variant_match || !entry_run || !variant_none || !variant_exists || !override_found || !override_worker_match ||
              !override_redirect || !earlier_eligible || !reporter_resident || !kind))
        return HQTICK_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        if (entry_class[i] > hqreject::E_PF) return HQTICK_E_INVALID;
        kind[i] = (uint8_t)hqreject::kind_of(entry_found[i] != 0, entry_class[i], entry_worker_match[i] != 0, entry_variant_match[i] != 0, entry_run[i] != 0, variant_none[i] != 0,
                                             variant_exists[i] != 0, override_found[i] != 0, override_worker_match[i] != 0, override_redirect[i] != 0, earlier_eligible[i] != 0);
        if (blocks) blocks[i] = hqreject::blocks(kind[i], variant_none[i] != 0, variant_exists[i] != 0, reporter_resident[i] != 0) ? 1 : 0;
    }
    return (int)n;
}
// the rule of hqtick_lose_workers on host arrays: lose_core.h's kind_of_entry and settle per evicted entry
extern "C" int hqtick_debug_lose_kind(uint32_t n, const uint8_t *entry_class, const uint8_t *entry_run, const uint8_t *redirect_target, uint8_t *kind, uint8_t *running) {
    if (n && (!entry_class || !entry_run || !redirect_target || !kind)) return HQTICK_E_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        if (entry_class[i] > hqlose::E_PF) return HQTICK_E_INVALID;
        kind[i] = (uint8_t)hqlose::settle(hqlose::kind_of_entry(entry_class[i], entry_run[i] != 0), redirect_target[i] != 0);
        if (running) running[i] = hqlose::is_running(kind[i]) ? 1 : 0;
    }
    return (int)n;
}
// the grouping of hqtick_lose_workers on host arrays: cancel_core.h's stable sort and lose_core.h's two phases in the given thread order
extern "C" int hqtick_debug_lose_group(uint32_t k, uint32_t n_workers, const uint64_t *task_id, const uint64_t *priority, const uint32_t *rq, const uint8_t *kind, const uint32_t *worker_index,
                                       int order, uint32_t *out_off, uint64_t *out_task, uint64_t *out_priority, uint32_t *out_rq, uint8_t *out_kind) {
    if (!n_workers || !out_off || order < 0 || order > 2 || k > 0x7FFFFFFFu || (k && (!task_id || !priority || !rq || !kind || !worker_index || !out_task || !out_priority || !out_rq || !out_kind)))
        return HQTICK_E_INVALID;
    for (uint32_t j = 0; j < k; j++) if (worker_index[j] >= n_workers || (j && task_id[j] <= task_id[j - 1])) return HQTICK_E_INVALID;
    if (!hqlose::group_on_host(k, n_workers, task_id, priority, rq, kind, worker_index, order, out_off, out_task, out_priority, out_rq, out_kind)) return HQTICK_E_DEVICE;
    return (int)k;
}

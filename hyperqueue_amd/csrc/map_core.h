// The mapping plan (map.h: hqmap::Mapper), with no HIP in sight: create_task_mapping and process_proactive_filling (scheduler/mapping.rs) restated as index
// arithmetic over the placement counts, so that tools/map_core_asan.cpp can run it under AddressSanitizer + UBSan on exact-size heap blocks (tests/test_map_core.py)
// and hqtick_debug_host_plan against the reference's mapping on a machine without a GPU (tests/test_host_stages.py).
//   plan_keys        the take sequence of every queue and the per-key tables                                  (mapping.rs:36-157)
//   plan_redirects   tasks that leave a prefill set or are Retracting in their queue: redirects, not records   (mapping.rs:66-101)
//   plan_prefill     process_proactive_filling                                                                  (mapping.rs:159-234)
//   plan_outputs     what K4 selects per (level, rq) group, where every worker's records go
//   assemble_host_part  everything of the result that needs no GPU output
//   small_words / pack_small, sweep_words / pack_sweep_keys   the packed small tables behind the big ones, and the key-table image of the early K5a launch
// Each stage returns 0 or an HQTICK_E_* code with *why set.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/hqtick.h"
#include "hb_order.h"
#include "host_model.h"
#include "scan_core.h"

namespace hqmap {

static constexpr uint32_t NONE = 0xFFFFFFFFu;

// The plan of one tick.  Reused across ticks: no per-tick allocation in the steady state.
struct Plan {
    std::vector<uint32_t> q_total, pf_n, pf_start, seq_taken, pf_drained, zq_taken, new_pf_total, pfl_size, rq_sel_base;
    std::vector<uint32_t> key_seg, key_sum, key_rq, key_var_w, key_ord_off, ord_cnt, key_t_off, key_bits_off;
    std::vector<uint32_t> key_tr;   // per key: c > 0 = stored worker-major by K4 (kernels.h: MapKeys::key_tr)
    std::vector<uint32_t> list_pos, pf_flag, pf_flag_prev, sn_ok, items, n_assign, asg_qw, has_pf, wm_order, pfq_src, pfq_size, out_off, take_base, mn_first, q_tnc;
    std::vector<uint8_t> now_mn;
    // the three per-(key | request, worker) tables of the plan are built IN the storage PlanIn::storage hands out — in a tick the pinned buffer K4's ride-along
    // workgroups copy from (a memcpy of ~100 KB per tick otherwise): [wpos nkeys * W][wcnt nkeys * W][pfl_j Q * W] at its head, the small tables behind them (pack_small)
    uint32_t *wpos = nullptr, *wcnt = nullptr, *pfl_j = nullptr; size_t pfl_rows = 0, plan_head_words = 0;
    std::vector<uint32_t> sink_hdr;
    std::vector<uint64_t> holes;                                 // (rq << 32 | logical position) of Retracting tasks taken this tick
    std::vector<std::pair<uint32_t, uint32_t>> freed;            // (worker, variant slot) given back by re-targeted redirects
    std::vector<std::pair<uint32_t, uint64_t>> retract_pairs;  // (old worker, task)
    // cached worker_map iteration order (emulated) for the last worker-id set
    std::vector<uint32_t> cached_ids, cached_order;
    // ---- the tick's sizes
    uint32_t nkeys = 0, max_count = 0, max_nk = 0, n_bit_words = 0, n_sel = 0, n_pfq = 0, n_rec = 0, max_items = 0, max_out = 0;
    uint32_t n_tr = 0;         // keys K4 stores worker-major (key_tr)
    bool may_reorder = false;  // the mapping kernel needs its stable sort: several priority levels, Retracting holes or prefilled tasks inside the queues
    bool compact = false;      // compact emission (HQTICK_FLAG_COMPACT_RECORDS / _DELTA16)
    std::vector<uint32_t> pfq_rq;                             // requests that prefill in this tick, ascending
    std::vector<std::pair<uint32_t, uint32_t>> retr_pos;      // (rq, queue position) of every Retracting task
    std::vector<std::vector<uint32_t>> key_T;                 // lazily built T_k(s) tables of worker_of()
};

// What of hqtick_result needs no GPU output (mn_*: filled once the multi-node task ids are back, Mapper::export_result).
struct HostResult {
    std::vector<uint32_t> cnt_rq, cnt_worker, cnt_value; std::vector<uint8_t> cnt_variant;
    std::vector<uint32_t> rec_off, retract_off, red_worker, mn_off, mn_worker, mn_rq; std::vector<uint64_t> retract_task, red_task, mn_task, new_free;
    std::vector<uint8_t> red_variant, red_kind;
};

struct PlanIn {
    const hqscan::Table *sc; hqhost::Counts *cnt;  // (Counts::pairs() builds the pairs of a by_class result on demand)
    const hqtick_snapshot *s;
    const hqhost::RequestView *rqs; const hqhost::VariantView *variants;
    uint32_t proactive_filling_reserve, proactive_filling_max, flags;  // of the config (flags: the record forms)
    bool sink;                                // a record sink is set: no compact emission
    uint32_t shard_index, shard_count;
    uint64_t N;                               // slots of the ready set
    const uint32_t *retr_key, *retr_rank;     // [s->n_retracting] dense: level * Q + rq and the rank among that group's tasks in ascending id; view: rq and the position in the permutation; key 0xFFFFFFFF = not in the set
    const uint32_t *ledger_pf; uint32_t ledger_pf_stride;  // the ledger's prefilled counts [W x stride], or null
    bool transpose_on;
    uint32_t *(*storage)(void *user, size_t words); void *user;  // room for the plan: the big tables at its head, small_words() behind them; null = none to be had
};

inline uint32_t n_groups(const hqscan::Table &sc) { return sc.ordered ? (uint32_t)sc.run_cnt.size() : sc.G; }  // entries of the selection plan

// ---- the packed small tables: their size, and the one place that writes them
// (an upper bound: every table below with one word where it is empty, the alignment word and the hole list)
inline size_t small_words(uint32_t nkeys, size_t n_cnt, uint32_t Q, uint32_t W, uint32_t n_groups_, uint32_t n_retracting, bool ordered) {
    return (size_t)9 * (nkeys + 4) + n_cnt + (size_t)7 * (Q + 2) + (W + 2) + (size_t)4 * n_groups_ + (size_t)2 * n_retracting + 64 +
           (ordered ? (size_t)3 * (Q + 2) + (size_t)2 * n_groups_ + 8 : 0);  // (the view's tables: run_off, q_tnc, run_start, run_rank)
}
struct Packer {
    uint32_t *hp; size_t cur;
    size_t put(const std::vector<uint32_t> &v) { const size_t o = cur; if (!v.empty()) memcpy(hp + cur, v.data(), v.size() * 4); cur += v.size(); if (v.empty()) hp[cur++] = 0; return o; }
};
struct SmallTables {  // word offsets from the start of the plan, as K4 / K5 are given them
    size_t o_rq, o_var, o_seg, o_ordoff, o_ord, o_toff, o_boff, o_tr, o_base, o_pfs, o_pfn, o_pqs, o_pqz, o_out, o_pqr, o_tb, o_roff, o_qtnc, o_rst, o_rrk, o_holes, words;
};
// hp: the plan's storage; the small tables go behind its plan_head_words.  with_pfq_rq: the ledger's staging names the request of a PREFILL record
inline SmallTables pack_small(uint32_t *hp, const Plan &ps, const hqscan::Table &sc, bool with_pfq_rq) {
    SmallTables t{};
    Packer pk{hp, ps.plan_head_words};
    t.o_rq = pk.put(ps.key_rq); t.o_var = pk.put(ps.key_var_w); t.o_seg = pk.put(ps.key_seg); t.o_ordoff = pk.put(ps.key_ord_off); t.o_ord = pk.put(ps.ord_cnt); t.o_toff = pk.put(ps.key_t_off);
    t.o_boff = pk.put(ps.key_bits_off); t.o_tr = pk.put(ps.key_tr); t.o_base = pk.put(ps.rq_sel_base); t.o_pfs = pk.put(ps.pf_start); t.o_pfn = pk.put(ps.pf_n);
    t.o_pqs = pk.put(ps.pfq_src); t.o_pqz = pk.put(ps.pfq_size); t.o_out = pk.put(ps.out_off);
    t.o_pqr = with_pfq_rq ? pk.put(ps.pfq_rq) : 0;
    t.o_tb = pk.put(ps.take_base);
    if (sc.ordered) { t.o_roff = pk.put(sc.run_off); t.o_qtnc = pk.put(ps.q_tnc); t.o_rst = pk.put(sc.run_start); t.o_rrk = pk.put(sc.run_level); }  // the view's tables (order.hip: k_order_select)
    if (pk.cur & 1) hp[pk.cur++] = 0;  // 8-byte alignment for the u64 hole list
    t.o_holes = pk.cur;
    for (uint64_t hk : ps.holes) { hp[pk.cur++] = (uint32_t)(hk & 0xFFFFFFFFu); hp[pk.cur++] = (uint32_t)(hk >> 32); }
    if (ps.holes.empty()) { hp[pk.cur++] = 0; hp[pk.cur++] = 0; }
    t.words = pk.cur;
    return t;
}
// ... and the key tables alone, as the early K5a launch reads them (counts in Map order per key)
inline size_t sweep_words(uint32_t nkeys, size_t n_ord) { return 4 * (size_t)(nkeys + 1) + n_ord; }
struct SweepTables { size_t o_toff, o_ordoff, o_boff, o_tr, o_ord, words; };
inline SweepTables pack_sweep_keys(uint32_t *hp, const Plan &ps) {
    SweepTables t{};
    Packer pk{hp, 0};
    t.o_toff = pk.put(ps.key_t_off); t.o_ordoff = pk.put(ps.key_ord_off); t.o_boff = pk.put(ps.key_bits_off); t.o_tr = pk.put(ps.key_tr); t.o_ord = pk.put(ps.ord_cnt);
    t.words = pk.cur;
    return t;
}

// host mirror of the K5 arithmetic: the worker that receives the task at index idx of key k's take_tasks() vector
inline uint32_t worker_of(Plan &ps, hqhost::Counts &cnt, uint32_t k, uint32_t idx) {
    cnt.pairs();  // (rare path: redirects)
    const auto &pk = cnt.per_key[k];
    std::vector<uint32_t> &T = ps.key_T[k];
    if (T.empty()) {
        uint32_t maxc = 0; for (auto &wc : pk) maxc = std::max(maxc, wc.second);
        std::vector<uint32_t> ge(maxc + 2, 0);
        for (auto &wc : pk) ge[wc.second]++;
        uint32_t more = (uint32_t)pk.size(), acc = 0;
        for (uint32_t sw = 0; sw <= maxc; sw++) { T.push_back(acc); more -= ge[sw]; acc += more; }
    }
    uint32_t sw = (uint32_t)(std::upper_bound(T.begin(), T.end(), idx) - T.begin()) - 1, nth = idx - T[sw];
    for (auto &wc : pk) if (wc.second > sw) { if (nth == 0) return wc.first; nth--; }
    return HQ_NO_WORKER;
}

// create_task_mapping as index arithmetic, part 1: the take sequence of every queue and the per-key tables  (mapping.rs:36-157)
inline int plan_keys(Plan &ps, HostResult &hr, const PlanIn &in, const char **why) {
    const hqscan::Table &sc = *in.sc; hqhost::Counts &cnt = *in.cnt; const hqtick_snapshot *s = in.s;
    const uint32_t W = s->n_workers, Q = s->n_requests;
    // per request: logical take sequence = [first level][prefilled][rest] when the prefill priority equals the top
    // priority of the queue, else [prefilled][all levels]   (taskqueue.rs:320-355)
    ps.q_total.assign(Q, 0); ps.pf_n.assign(Q, 0); ps.pf_start.assign(Q, 0); ps.seq_taken.assign(Q, 0);
    for (uint32_t q = 0; q < Q; q++) {
        const uint32_t r0 = sc.run_off[q], r1 = sc.run_off[q + 1];
        for (uint32_t r = r0; r < r1; r++) ps.q_total[q] += sc.run_cnt[r];
        ps.pf_n[q] = s->prefill_off ? s->prefill_off[q + 1] - s->prefill_off[q] : 0;
        if (ps.pf_n[q]) ps.pf_start[q] = (r0 < r1 && sc.run_prio[r0] == s->prefill_priority[q]) ? sc.run_cnt[r0] : 0;
    }
    const uint32_t nkeys = ps.nkeys = (uint32_t)cnt.keys.size();
    ps.key_seg.assign(nkeys, 0); ps.key_sum.assign(nkeys, 0); ps.key_rq.assign(nkeys, 0); ps.key_var_w.assign((nkeys + 3) / 4 + 1, 0);
    ps.key_ord_off.assign(nkeys + 1, 0); ps.key_t_off.assign(nkeys + 1, 0); ps.key_bits_off.assign(nkeys + 1, 0);
    const bool by_class = cnt.by_class && cnt.wclass.size() == W && cnt.key_col.size() == nkeys;
    size_t n_cnt = 0; for (uint32_t k = 0; k < nkeys; k++) n_cnt += cnt.key_size(k);
    {   // the big tables live at the head of the plan's storage; everything else of the plan (pack_small) is a few KB behind them
        ps.plan_head_words = (size_t)nkeys * W * 2 + (size_t)Q * W;
        ps.wpos = in.storage(in.user, ps.plan_head_words + small_words(nkeys, n_cnt, Q, W, n_groups(sc), s->n_retracting, sc.ordered));
        if (!ps.wpos) { *why = "hipHostMalloc plan"; return HQTICK_E_DEVICE; }
        ps.wcnt = ps.wpos + (size_t)nkeys * W; ps.pfl_j = ps.wcnt + (size_t)nkeys * W; ps.pfl_rows = 0;
    }
    if (!by_class) { std::fill(ps.wpos, ps.wpos + (size_t)nkeys * W, NONE); std::fill(ps.wcnt, ps.wcnt + (size_t)nkeys * W, 0u); }  // (by class: every row is written in full below)
    ps.items.assign(W, 0); ps.n_assign.assign(W, 0); ps.asg_qw.assign((size_t)Q * W, 0);
    hr.cnt_rq.resize(n_cnt); hr.cnt_variant.resize(n_cnt); hr.cnt_worker.resize(n_cnt); hr.cnt_value.resize(n_cnt); ps.ord_cnt.resize(n_cnt);
    uint32_t *c_rq = hr.cnt_rq.data(), *c_w = hr.cnt_worker.data(), *c_v = hr.cnt_value.data(), *c_ord = ps.ord_cnt.data(); uint8_t *c_var = hr.cnt_variant.data();
    size_t ci = 0;
    ps.max_count = 0; ps.max_nk = 0;
    if (by_class) {  // position of every worker in each distinct worker list (Map order), built once per list
        ps.list_pos.assign(cnt.lists.size() * (size_t)W, NONE);
        for (size_t l = 0; l < cnt.lists.size(); l++) {
            uint32_t *lp = ps.list_pos.data() + l * W; const std::vector<uint32_t> &wi = cnt.lists[l].widx;
            for (uint32_t i = 0; i < wi.size(); i++) lp[wi[i]] = i;
        }
    }
    for (uint32_t k = 0; k < nkeys; k++) {
        const uint32_t q = cnt.keys[k].first; const uint8_t v = cnt.keys[k].second;
        ps.key_rq[k] = q; reinterpret_cast<uint8_t *>(ps.key_var_w.data())[k] = v;
        uint32_t sum = 0, maxc = 0, pos = 0;
        uint32_t *wp = ps.wpos + (size_t)k * W, *wcn = ps.wcnt + (size_t)k * W, *aq = ps.asg_qw.data() + (size_t)q * W, *items = ps.items.data(), *nas = ps.n_assign.data();
        if (by_class) {  // separable tick: the count of a worker is its class's; sequential passes instead of scattering (worker, count) pairs
            const uint32_t *xg = cnt.class_x.data() + cnt.key_col[k], *wcl = cnt.wclass.data(); const uint32_t NCc = cnt.n_cols;
            const std::vector<uint32_t> &wi = cnt.lists[cnt.key_list[k]].widx;
            if (cnt.one_class) { const uint32_t c = xg[0]; for (uint32_t w = 0; w < W; w++) { wcn[w] = c; items[w] += c; aq[w] += c; } }  // a cold tick on identical workers (vectorises)
            else for (uint32_t w = 0; w < W; w++) { const uint32_t c = xg[(size_t)wcl[w] * NCc]; wcn[w] = c; items[w] += c; aq[w] += c; }
            memcpy(wp, ps.list_pos.data() + (size_t)cnt.key_list[k] * W, (size_t)W * 4);
            pos = (uint32_t)wi.size();
            if (pos) { std::fill(c_rq + ci, c_rq + ci + pos, q); memset(c_var + ci, v, pos); memcpy(c_w + ci, wi.data(), (size_t)pos * 4); }
            if (cnt.one_class) { const uint32_t c = xg[0]; std::fill(c_v + ci, c_v + ci + pos, c); std::fill(c_ord + ci, c_ord + ci + pos, c); sum = c * pos; maxc = c; }
            else for (uint32_t i = 0; i < pos; i++) { const uint32_t c = wcn[wi[i]]; c_v[ci + i] = c; c_ord[ci + i] = c; sum += c; maxc = std::max(maxc, c); }
            ci += pos;
        } else for (auto &wc : (cnt.pairs(), cnt.per_key[k])) {  // (worker, count) in the Map's iteration order
            const uint32_t w = wc.first, c = wc.second;
            sum += c; maxc = std::max(maxc, c);
            c_rq[ci] = q; c_var[ci] = v; c_w[ci] = w; c_v[ci] = c; c_ord[ci] = c; ci++;
            wp[w] = pos++; wcn[w] = c; items[w] += c; nas[w] += c; aq[w] += c;
        }
        ps.key_ord_off[k + 1] = (uint32_t)ci;
        ps.key_t_off[k + 1] = ps.key_t_off[k] + maxc + 1;  // sweeps 0..maxc
        ps.key_bits_off[k + 1] = ps.key_bits_off[k] + (maxc + 1) * ((pos + 63) / 64);
        ps.max_count = std::max(ps.max_count, maxc); ps.max_nk = std::max(ps.max_nk, pos);
        ps.key_seg[k] = ps.seq_taken[q]; ps.key_sum[k] = sum; ps.seq_taken[q] += sum;
        if (ps.seq_taken[q] > ps.q_total[q] + ps.pf_n[q]) { *why = "solver placed more tasks than the queue holds (reference panics, taskqueue.rs:327)"; return HQTICK_E_QUEUE_UNDERFLOW; }
    }
    if (by_class && W) memcpy(ps.n_assign.data(), ps.items.data(), (size_t)W * 4);  // equal until the redirects are taken off
    ps.n_bit_words = ps.key_bits_off[nkeys];
    // Worker-major selection (kernels.hip: SelPlanN): a request served by ONE key that starts at the head of its queue and gives every one of its workers the same
    // count — the cold tick on identical workers, and every saturated class of a homogeneous cluster — is written by K4 so that each worker's ids are contiguous.
    // Only plain queues: no prefill set in front of the request, no Retracting task anywhere in this tick (holes are positions of the queue order).
    ps.key_tr.assign(nkeys, 0);
    ps.n_tr = 0;
    if (in.transpose_on && s->n_retracting == 0) {
        std::vector<uint32_t> &nk = ps.pf_drained;  // (scratch: keys per request; plan_redirects re-assigns it)
        nk.assign(Q, 0);
        for (uint32_t k = 0; k < nkeys; k++) nk[ps.key_rq[k]]++;
        for (uint32_t k = 0; k < nkeys; k++) {
            const uint32_t q = ps.key_rq[k], n = ps.key_ord_off[k + 1] - ps.key_ord_off[k], c = ps.key_t_off[k + 1] - ps.key_t_off[k] - 1;
            if (nk[q] != 1 || ps.key_seg[k] != 0 || ps.pf_n[q] != 0 || n == 0 || c == 0 || c > 0xFFFFu || n > 0xFFFFu || (uint64_t)n * c != ps.key_sum[k]) continue;
            ps.key_tr[k] = c; ps.n_tr++;
        }
    }
    // multi-node placements take one task each from the head of their queue (mapping.rs:133-154)
    ps.mn_first.assign(cnt.mn_rq.size(), 0);
    for (size_t i = 0; i < cnt.mn_rq.size(); i++) {
        uint32_t q = cnt.mn_rq[i];
        ps.mn_first[i] = ps.seq_taken[q]; ps.seq_taken[q] += (uint32_t)cnt.mn_sets[i].size();
        if (ps.pf_n[q]) { *why = "multi-node queue with a prefill set"; return HQTICK_E_UNSUPPORTED; }
        if (ps.seq_taken[q] > ps.q_total[q]) { *why = "multi-node placement exceeds its queue"; return HQTICK_E_QUEUE_UNDERFLOW; }
    }
    return 0;
}

// part 2: tasks that leave a prefill set or are Retracting in their queue — redirects instead of records  (mapping.rs:66-101)
inline int plan_redirects(Plan &ps, HostResult &hr, const PlanIn &in, const char **why) {
    const hqscan::Table &sc = *in.sc; hqhost::Counts &cnt = *in.cnt; const hqtick_snapshot *s = in.s;
    const uint32_t W = s->n_workers, Q = s->n_requests, nkeys = ps.nkeys;
    // already-prefilled tasks that this tick hands out: Prefilled{old} -> retract + redirect  (mapping.rs:81-101)
    ps.retract_pairs.clear();
    hr.red_task.clear(); hr.red_worker.clear(); hr.red_variant.clear();
    ps.pf_drained.assign(Q, 0);
    ps.has_pf.assign((size_t)Q * W, 0);  // SingleNodeTaskAssignment::prefilled_tasks as per-(rq, worker) counts
    if (s->prefilled_off) for (uint32_t w = 0; w < W; w++) for (uint32_t i = s->prefilled_off[w]; i < s->prefilled_off[w + 1]; i++) if (s->prefilled_rq[i] < Q) ps.has_pf[(size_t)s->prefilled_rq[i] * W + w]++;
    if (in.ledger_pf) {  // the ledger's prefilled counts (its sync_mirror brought them back; a snapshot with prefilled_off was refused)
        const uint32_t pf_stride = in.ledger_pf_stride, nq = std::min(Q, pf_stride);
        for (uint32_t w = 0; w < W; w++) for (uint32_t q = 0; q < nq; q++) ps.has_pf[(size_t)q * W + w] = in.ledger_pf[(size_t)w * pf_stride + q];
    }
    ps.key_T.assign(nkeys, {});
    hr.red_kind.clear();
    for (uint32_t k = 0; k < nkeys; k++) {
        const uint32_t q = cnt.keys[k].first;
        if (!ps.pf_n[q]) continue;
        uint32_t a = std::max(ps.key_seg[k], ps.pf_start[q]), b = std::min(ps.key_seg[k] + ps.key_sum[k], ps.pf_start[q] + ps.pf_n[q]);
        for (uint32_t p = a; p < b; p++) {
            uint32_t slot = s->prefill_off[q] + (p - ps.pf_start[q]);
            uint64_t task = s->prefill_task[slot]; uint32_t oldw = s->prefill_worker[slot];
            uint32_t neww = worker_of(ps, cnt, k, p - ps.key_seg[k]);
            ps.retract_pairs.push_back({oldw, task});
            if (oldw < W && ps.has_pf[(size_t)q * W + oldw]) ps.has_pf[(size_t)q * W + oldw]--;
            hr.red_task.push_back(task); hr.red_worker.push_back(neww); hr.red_variant.push_back(cnt.keys[k].second); hr.red_kind.push_back(HQ_REDIRECT_FROM_PREFILL);
            if (neww < W) { ps.asg_qw[(size_t)q * W + neww]--; ps.n_assign[neww]--; }  // a redirect is not a new `assigned` record
            ps.pf_drained[q]++;
        }
    }
    // ready tasks in state Retracting{old} that this tick takes (mapping.rs:66-80): no `assigned` record, a redirect instead
    ps.holes.clear(); ps.freed.clear();
    ps.retr_pos.clear();  // (rq, queue position) of every Retracting task, for the prefill check
    if (s->n_retracting) {
        if (in.N == 0) { *why = "retracting tasks without a ready set"; return HQTICK_E_INVALID; }
        const uint32_t nr = s->n_retracting;
        const uint32_t *rkey = in.retr_key, *rrank = in.retr_rank;
        for (uint32_t i = 0; i < nr; i++) {
            if (rkey[i] == 0xFFFFFFFFu || Q == 0) { *why = "a retracting task is not in the ready set"; return HQTICK_E_INVALID; }
            uint32_t q, z;                                                                        // request and position in its queue (levels, then id)
            if (sc.ordered) {  // the view: rkey = rq, rrank = position in the permutation, whose segment of q starts at its first run
                q = rkey[i];
                if (q >= Q || sc.run_off[q] == sc.run_off[q + 1]) { *why = "a retracting task is not in the ready set"; return HQTICK_E_INVALID; }
                z = rrank[i] - sc.run_start[sc.run_off[q]];
            } else {
                const uint32_t l = rkey[i] / Q; q = rkey[i] % Q;
                z = rrank[i]; for (uint32_t r = sc.run_off[q]; r < sc.run_off[q + 1] && sc.run_level[r] < l; r++) z += sc.run_cnt[r];
            }
            const uint32_t p = z < ps.pf_start[q] ? z : z + ps.pf_n[q];                             // position in the logical take sequence
            ps.retr_pos.push_back({q, z});
            if (p >= ps.seq_taken[q]) continue;                                                   // stays in its queue
            uint32_t k = nkeys;
            for (uint32_t kk = 0; kk < nkeys; kk++) if (ps.key_rq[kk] == q && p >= ps.key_seg[kk] && p < ps.key_seg[kk] + ps.key_sum[kk]) { k = kk; break; }
            if (k == nkeys) { *why = "a Retracting task was taken by a multi-node placement"; return HQTICK_E_UNSUPPORTED; }
            const uint32_t neww = worker_of(ps, cnt, k, p - ps.key_seg[k]), oldw = s->retracting_worker[i];
            const uint8_t v = cnt.keys[k].second;
            ps.holes.push_back(((uint64_t)q << 32) | p);
            if (neww < W) { ps.asg_qw[(size_t)q * W + neww]--; ps.n_assign[neww]--; }
            hr.red_task.push_back(s->retracting_task[i]); hr.red_worker.push_back(neww); hr.red_variant.push_back(v);
            if (oldw != neww) {
                hr.red_kind.push_back(HQ_REDIRECT_RETARGET);
                const uint32_t tw = s->retracting_redirect_worker ? s->retracting_redirect_worker[i] : HQ_NO_WORKER;
                if (tw != HQ_NO_WORKER) ps.freed.push_back({tw, in.rqs[q].first_variant + (s->retracting_redirect_variant ? s->retracting_redirect_variant[i] : 0)});  // remove_sn_task(previous target)
            } else {
                hr.red_kind.push_back(HQ_REDIRECT_SAME_WORKER);
            }
        }
        std::sort(ps.holes.begin(), ps.holes.end());
    }
    // queue tasks taken per request (excluding the prefilled block)
    ps.zq_taken.assign(Q, 0);
    for (uint32_t q = 0; q < Q; q++) ps.zq_taken[q] = ps.seq_taken[q] - ps.pf_drained[q];
    // workers that received a multi-node task are no longer SN (set_mn_task)
    ps.now_mn.assign(W, 0);
    for (auto &sets : cnt.mn_sets) for (auto &set : sets) for (uint32_t w : set) ps.now_mn[w] = 1;
    return 0;
}

// part 3: process_proactive_filling  (mapping.rs:159-234)
inline int plan_prefill(Plan &ps, HostResult &, const PlanIn &in, const char **why) {
    const hqscan::Table &sc = *in.sc; const hqtick_snapshot *s = in.s;
    const uint32_t W = s->n_workers, Q = s->n_requests;
    if (s->worker_map_rank) { ps.wm_order.assign(W, 0); for (uint32_t w = 0; w < W; w++) ps.wm_order[s->worker_map_rank[w]] = w; }
    else {
        if (ps.cached_ids.size() != W || (W && memcmp(ps.cached_ids.data(), s->worker_id, (size_t)W * 4) != 0)) {
            ps.cached_ids.assign(s->worker_id, s->worker_id + W);
            hqhb::insertion_order_u32(s->worker_id, W, ps.cached_order);
        }
    }
    const std::vector<uint32_t> &wm_order = s->worker_map_rank ? ps.wm_order : ps.cached_order;  // (no copy of the cached order)
    ps.sn_ok.resize(W);  // per worker: still a single-node worker after this tick's multi-node placements
    for (uint32_t w = 0; w < W; w++) ps.sn_ok[w] = ((s->worker_flags ? (s->worker_flags[w] & HQ_WORKER_SN) != 0 : true) && !ps.now_mn[w]) ? 1u : 0u;
    ps.new_pf_total.assign(Q, 0); ps.pfl_size.assign(Q, 0);
    ps.pfq_src.clear(); ps.pfq_size.clear(); ps.pfl_rows = 0;
    ps.pfq_rq.clear();
    {
        // state of every queue after the takes: first level that still has tasks
        std::vector<int64_t> top_run(Q, -1); std::vector<uint32_t> top_left(Q, 0);  // (the run that is the queue's top after the takes)
        uint64_t global_top = 0;
        for (uint32_t q = 0; q < Q; q++) {
            uint32_t left = ps.zq_taken[q];
            for (uint32_t r = sc.run_off[q]; r < sc.run_off[q + 1]; r++) { uint32_t h = sc.run_cnt[r]; if (h > left) { top_run[q] = r; top_left[q] = h - left; break; } left -= h; }
            if (top_run[q] >= 0) global_top = std::max(global_top, sc.run_prio[top_run[q]]);  // TaskQueues::top_priority  taskqueue.rs:62-68
        }
        size_t prev_row = SIZE_MAX;  // the pfl_j row that belongs to pf_flag_prev
        for (uint32_t q = 0; q < Q; q++) {
            if (top_run[q] < 0 || sc.run_prio[top_run[q]] != global_top) continue;
            bool pf_left = ps.pf_n[q] > ps.pf_drained[q];
            uint32_t tsz = (pf_left && s->prefill_priority[q] != global_top) ? 0 : top_left[q];  // top_size_no_prefill  taskqueue.rs:241-253
            uint32_t size = tsz > in.proactive_filling_reserve ? tsz - in.proactive_filling_reserve : 0;
            if (!size) continue;
            // eligible workers: flags in index order (a branch-free pass), their ranks in worker_map order only when the set differs from the
            // previous request's (on a saturated tick every worker serves every class: one walk of the order for all requests)
            const uint32_t *aq = ps.asg_qw.data() + (size_t)q * W, *hp = ps.has_pf.data() + (size_t)q * W;
            ps.pf_flag.resize(W);
            uint32_t n_elig = 0;
            {
                uint32_t *fl = ps.pf_flag.data(); const uint32_t *sn = ps.sn_ok.data();
                for (uint32_t w = 0; w < W; w++) { const uint32_t f = sn[w] & (aq[w] != 0 ? 1u : 0u) & (hp[w] == 0 ? 1u : 0u); fl[w] = f; n_elig += f; }  // (vectorises)
            }
            if (!n_elig) continue;
            uint32_t psz = std::min(size / n_elig, in.proactive_filling_max);
            if (!psz) continue;
            ps.pfl_size[q] = psz;
            ps.pfq_rq.push_back(q);
            const size_t o = ps.pfl_rows++ * W;  // (at most Q rows: one per request)
            if (prev_row != SIZE_MAX && memcmp(ps.pf_flag.data(), ps.pf_flag_prev.data(), (size_t)W * 4) == 0) memcpy(ps.pfl_j + o, ps.pfl_j + prev_row, (size_t)W * 4);
            else {
                uint32_t *row = ps.pfl_j + o; const uint32_t *fl = ps.pf_flag.data();
                uint32_t j = 0;
                for (uint32_t w : wm_order) { const uint32_t f = fl[w]; row[w] = f ? j : NONE; j += f; }
                ps.pf_flag_prev.swap(ps.pf_flag);
            }
            prev_row = o;
            ps.new_pf_total[q] = psz * n_elig;
        }
    }
    for (auto &rp : ps.retr_pos) {  // take_tasks_for_prefill on a Retracting task: the reference asserts task.is_waiting()  (mapping.rs:221)
        const uint32_t q = rp.first, z = rp.second;
        if (ps.new_pf_total[q] && z >= ps.zq_taken[q] && z < ps.zq_taken[q] + ps.new_pf_total[q]) {
            *why = "a Retracting task reached take_tasks_for_prefill: the reference asserts task.is_waiting() (mapping.rs:221)"; return HQTICK_E_UNSUPPORTED;
        }
    }
    return 0;
}

// part 4: what K4 selects per (level, rq) group, where every worker's records go.  (The two capacity checks against the kernels' LDS staging follow directly
// behind it on the HIP side: Mapper::check_capacity.)
inline int plan_outputs(Plan &ps, HostResult &, const PlanIn &in, const char **why) {
    const hqscan::Table &sc = *in.sc; const hqtick_snapshot *s = in.s;
    const uint32_t W = s->n_workers, Q = s->n_requests, nkeys = ps.nkeys;
    // ---- selection plan per (level, rq) group ----
    ps.rq_sel_base.assign(Q + 1, 0);
    for (uint32_t q = 0; q < Q; q++) ps.rq_sel_base[q + 1] = ps.rq_sel_base[q] + ps.zq_taken[q] + ps.new_pf_total[q];
    ps.n_sel = ps.rq_sel_base[Q];
    // (the view selects per request from rq_sel_base alone — order.hip: k_order_select — and needs only the worker-major form per request)
    const size_t G = sc.ordered ? 0 : sc.G;
    ps.take_base.assign((size_t)4 * G, 0);  // [take][base][tnc][tsb] per (level, rq) group (kernels.hip: SelPlanN)
    ps.q_tnc.assign(sc.ordered ? Q : 0, 0);
    if (!sc.ordered) for (uint32_t q = 0; q < Q; q++) {
        uint32_t want = ps.zq_taken[q] + ps.new_pf_total[q], cum = 0;
        for (uint32_t r = sc.run_off[q]; r < sc.run_off[q + 1]; r++) {
            const uint32_t h = sc.run_cnt[r], t = want > cum ? std::min(h, want - cum) : 0, g = sc.run_group[r];
            ps.take_base[g] = t; ps.take_base[G + g] = ps.rq_sel_base[q] + cum;
            cum += h;
        }
    }
    if (ps.n_tr) {
        if (!ps.holes.empty()) { *why = "internal: worker-major selection on a tick with holes"; return HQTICK_E_UNSUPPORTED; }  // (cannot happen: no Retracting task, no hole)
        for (uint32_t k = 0; k < nkeys; k++) {
            if (!ps.key_tr[k]) continue;
            const uint32_t q = ps.key_rq[k], n = ps.key_ord_off[k + 1] - ps.key_ord_off[k];
            if (sc.ordered) { ps.q_tnc[q] = (n << 16) | ps.key_tr[k]; continue; }
            for (uint32_t r = sc.run_off[q]; r < sc.run_off[q + 1]; r++) { ps.take_base[2 * G + sc.run_group[r]] = (n << 16) | ps.key_tr[k]; ps.take_base[3 * G + sc.run_group[r]] = ps.rq_sel_base[q]; }
        }
    }
    for (uint32_t q : ps.pfq_rq) { ps.pfq_src.push_back(ps.rq_sel_base[q] + ps.zq_taken[q]); ps.pfq_size.push_back(ps.pfl_size[q]); }
    ps.n_pfq = (uint32_t)ps.pfq_rq.size();
    // ---- output offsets ----
    ps.out_off.assign(W + 1, 0);
    ps.max_items = 0; ps.max_out = 0;
    ps.compact = (in.flags & (HQTICK_FLAG_COMPACT_RECORDS | HQTICK_FLAG_COMPACT_DELTA16)) != 0 && !in.sink;
    for (uint32_t w = 0; w < W; w++) {
        if (in.shard_count > 1 && hqhb::hash_worker_id(s->worker_id[w]) % in.shard_count != in.shard_index) { ps.out_off[w + 1] = ps.out_off[w]; continue; }  // another rank's worker
        uint32_t npf = 0;
        for (uint32_t pi = 0; pi < ps.n_pfq; pi++) if (ps.pfl_j[(size_t)pi * W + w] != NONE) npf += ps.pfq_size[pi];
        ps.out_off[w + 1] = ps.out_off[w] + npf + ps.n_assign[w];
        ps.max_items = std::max(ps.max_items, ps.items[w]);
        ps.max_out = std::max(ps.max_out, npf + ps.n_assign[w]);
    }
    ps.n_rec = ps.out_off[W];
    ps.may_reorder = sc.L > 1 || !ps.holes.empty() || (s->prefill_off && s->prefill_off[Q] > 0);
    return 0;
}

// everything of the result that needs no GPU output: in a tick it runs while the GPU works on phase C
inline void assemble_host_part(const Plan &ps, HostResult &hr, const PlanIn &in) {
    const hqhost::Counts &cnt = *in.cnt; const hqtick_snapshot *s = in.s;
    const uint32_t W = s->n_workers, R = s->n_resources;
    hr.rec_off = ps.out_off;
    hr.retract_off.assign(W + 1, 0); hr.retract_task.assign(ps.retract_pairs.size(), 0);
    {
        for (auto &rp : ps.retract_pairs) if (rp.first < W) hr.retract_off[rp.first + 1]++;
        for (uint32_t w = 0; w < W; w++) hr.retract_off[w + 1] += hr.retract_off[w];
        std::vector<uint32_t> cur(hr.retract_off.begin(), hr.retract_off.end() - 1);
        for (auto &rp : ps.retract_pairs) if (rp.first < W) hr.retract_task[cur[rp.first]++] = rp.second;  // stable: per worker in emission order
    }
    // Worker::insert_sn_task for every placed task (server/worker.rs:188-196 -> workerload.rs:156-165)
    hr.new_free.assign(s->worker_free, s->worker_free + (size_t)W * R);
    for (uint32_t k = 0; k < ps.nkeys; k++) {
        const hqhost::VariantView &vv = in.variants[in.rqs[cnt.keys[k].first].first_variant + cnt.keys[k].second];
        const uint32_t *wcn = ps.wcnt + (size_t)k * W;  // this key's count per worker (0 = none): the plan's own row
        for (uint32_t w = 0; w < W; w++) {
            const uint32_t c = wcn[w];
            if (!c) continue;
            for (uint32_t e = 0; e < vv.n_entries; e++) {
                uint64_t &f = hr.new_free[(size_t)w * R + vv.res[e]];
                if (vv.kind[e] == HQ_ENTRY_ALL) f = 0; else { uint64_t d = vv.amount[e] * (uint64_t)c; f = f > d ? f - d : 0; }
            }
        }
    }
    for (auto &fr : ps.freed) {  // remove_sn_task on the previous target of a re-targeted redirect  (worker.rs:223-234 -> workerload.rs:194-202)
        const hqhost::VariantView &vv = in.variants[fr.second];
        for (uint32_t e = 0; e < vv.n_entries; e++) {
            uint64_t &f = hr.new_free[(size_t)fr.first * R + vv.res[e]];
            f = vv.kind[e] == HQ_ENTRY_ALL ? s->worker_total[(size_t)fr.first * R + vv.res[e]] : f + vv.amount[e];
        }
    }
}

}  // namespace hqmap

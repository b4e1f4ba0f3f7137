// The audit of the resident state (hqtick_resident_check): the invariants as plain functions of ONE item each — a row of the ready columns, a
// slot of the graph, a bucket of the ledger, an entry of the Retracting table — compiled for the device (the kernels of audit.hip) and for the host
// (run_host below: the debug hook of include/hqtick_debug.h and tools/audit_core_asan.cpp run the same functions on host arrays, one emulated thread after the
// other, in three orders).  They read through const views and write nothing but the reporter they are handed and, for the edge pass, the audit's own scratch.
//
// Reference (crates/tako/src/internal): Core::sanity_check server/core.rs:280-436 — the counter check :353-367, the redirects loop :325-347 — and
// Worker::sanity_check server/worker.rs:236-271.
//
// Every index read from a table is checked before it is used (a slot from the hash table, a run from a chain, an edge range, a consumer slot): the audit must
// stay inside the arrays on the very states it exists to find.  A chain walk gives up after n_runs steps or n_edges edges.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/hqtick.h"

#if defined(__HIPCC__)
#define HQA_HD __host__ __device__ inline
#else
#define HQA_HD inline
#endif

namespace hqaudit {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t ST_FREE = 0xFFFFFFFFu;       // graph.h: unfinished of a free slot
constexpr uint32_t RQ_TOMBSTONE = 0xFFFFFFFFu;  // the request id of a ready-set row whose task left
constexpr uint64_t HT_EMPTY = ~0ull, HT_TOMB = ~0ull - 1;  // both hash tables (graph.h, assigned.h)
constexpr uint8_t PF_VARIANT = 0xFE, MN_VARIANT = 0xFF;  // assigned.h: the variant column of a prefilled / a multi-node entry

// what is resident (State::have)
enum : uint32_t {
    HAVE_READY = 1u,           // the ready columns
    HAVE_GRAPH = 2u,           // the graph's tables (possibly without a task)
    HAVE_LEDGER = 4u,          // the ledger: its hash table, the worker rows, the count tables, the request tables
    HAVE_LEDGER_SETTLED = 8u,  // ... and no placement of a tick waits to enter it (the Retracting table already shows that tick's redirects)
    HAVE_TRACKING = 16u,       // ... with prefilled tracking on
};
enum : uint8_t { RETR_IN_QUEUE = 1, RETR_REDIRECT = 2 };  // Retr::flags

struct Ready { const uint64_t *id; const uint32_t *rq; uint64_t n; };  // n: physical rows, tombstones included
struct Graph {
    const uint64_t *id; const uint32_t *unfinished, *gen, *head;       // per slot
    const uint64_t *ht_key; const uint32_t *ht_val; uint32_t ht_mask;  // id -> slot
    const uint32_t *run_next, *run_off, *run_len; const uint32_t *edge;  // edge: (consumer slot, consumer gen) pairs
    uint32_t n_slots, n_runs, n_edges;  // slots ever used, run records and edge pool entries in use
    uint64_t n_tasks;                   // the host's count of live slots
};
struct Ledger {
    const uint64_t *key; const uint32_t *worker, *rq; const uint8_t *variant; uint32_t mask;  // the hash table's columns (assigned.h: Table), mask + 1 buckets
    // the request tables as the HOST has them (staged for the call: ResourceRqMap only grows, so every slot the device knows is the same there), NV variant slots
    const uint32_t *rq_off, *ventry_off, *ent_res, *var_nodes; const uint8_t *ent_kind; const uint64_t *ent_amount; uint32_t Q, NV;
    // the worker rows (assigned.h: Rows, MnRows)
    const uint32_t *wid; uint32_t W, R; const uint64_t *total, *free_; const uint32_t *counts; uint32_t stride; const uint32_t *pf; uint32_t pf_stride;
    const uint64_t *mn_task; const uint8_t *mn_root, *flags;
    uint64_t n_live, mn_live, pf_live;  // the host's counts of single-node, multi-node and prefilled entries
};
// the audit's own census of the ledger, zero on entry: single-node entries per (row, slot) [W x stride], prefilled entries per (row, request) [W x pf_stride],
// root rows per bucket [mask + 1]
struct LedgerScratch { uint32_t *cen_counts, *cen_pf, *roots; };
struct Retr { const uint64_t *task; const uint32_t *target; const uint8_t *variant; const uint8_t *flags; uint32_t n; };  // target: worker id of the redirect
struct State { Ready ready; Graph graph; Ledger ledger; Retr retr; uint32_t have, parts; };
// the host's own counts, compared with the device's census once the kernels are done
struct Totals { uint64_t ready_live, graph_tasks, graph_free, graph_slots; };
enum : uint32_t { CLS_NONE = 0, CLS_SN = 1, CLS_MN = 2, CLS_PF = 3 };  // what a bucket of the ledger holds

HQA_HD uint32_t ht_hash(uint64_t k) {  // murmur3 finaliser (graph.hip's and assigned.hip's)
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (uint32_t)k;
}
// bucket of `id` by linear probing, NONE if an EMPTY bucket comes first (or after a whole round)
HQA_HD uint32_t ht_find(const uint64_t *key, uint32_t mask, uint64_t id) {
    if (id >= HT_TOMB) return NONE;
    uint32_t h = ht_hash(id) & mask;
    for (uint32_t probe = 0; probe <= mask; probe++) {
        const uint64_t k = key[h];
        if (k == id) return h;
        if (k == HT_EMPTY) return NONE;
        h = (h + 1) & mask;
    }
    return NONE;
}
HQA_HD bool graph_nonempty(const State &S) { return (S.have & HAVE_GRAPH) && S.graph.n_tasks != 0; }
// the live slot the graph holds `id` in, NONE if it holds none
HQA_HD uint32_t graph_slot(const Graph &g, uint64_t id) {
    const uint32_t p = ht_find(g.ht_key, g.ht_mask, id);
    if (p == NONE) return NONE;
    const uint32_t sl = g.ht_val[p];
    return (sl < g.n_slots && g.unfinished[sl] != ST_FREE) ? sl : NONE;
}
// is `id` a live row of the ready columns (ids ascending: a binary search)
HQA_HD bool ready_live(const Ready &r, uint64_t id) {
    uint64_t lo = 0, hi = r.n;
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (r.id[mid] < id) lo = mid + 1; else hi = mid; }
    return lo < r.n && r.id[lo] == id && r.rq[lo] != RQ_TOMBSTONE;
}

// The parts of `S.parts` that S.have lets the audit evaluate (hqtick_check_report.checked).
HQA_HD uint32_t parts_present(const State &S) {
    const bool rd = (S.have & HAVE_READY) != 0, lg = (S.have & HAVE_LEDGER) != 0, gr = graph_nonempty(S);
    uint32_t c = 0;
    if (rd) c |= HQ_CHECK_READY;
    if (lg) c |= HQ_CHECK_LEDGER;
    if (S.have & HAVE_GRAPH) c |= HQ_CHECK_GRAPH;
    if ((rd && lg) || (rd && gr) || (S.retr.n && (rd || lg))) c |= HQ_CHECK_CROSS;
    if (gr && (rd || lg)) c |= HQ_CHECK_STRICT;
    return c & S.parts;
}

// ---- the items.  Rep: hit(invariant, key) — each item reports an invariant at most once.
// Row i of the ready columns.  Returns whether it is live.
template <class Rep> HQA_HD bool ready_row(const State &S, uint64_t i, Rep &rep) {
    const uint64_t id = S.ready.id[i];
    if ((S.parts & HQ_CHECK_READY) && i > 0 && S.ready.id[i - 1] >= id) rep.hit(HQ_INV_READY_ORDER, id);
    if (S.ready.rq[i] == RQ_TOMBSTONE) return false;
    if ((S.parts & HQ_CHECK_CROSS) && (S.have & HAVE_LEDGER) && ht_find(S.ledger.key, S.ledger.mask, id) != NONE) rep.hit(HQ_INV_X_READY_ASSIGNED, id);
    if ((S.parts & (HQ_CHECK_CROSS | HQ_CHECK_STRICT)) && graph_nonempty(S)) {
        const uint32_t sl = graph_slot(S.graph, id);
        if (sl == NONE) { if (S.parts & HQ_CHECK_STRICT) rep.hit(HQ_INV_S_READY_UNKNOWN, id); }
        else if ((S.parts & HQ_CHECK_CROSS) && S.graph.unfinished[sl] != 0) rep.hit(HQ_INV_X_READY_WAITING, id);
    }
    return true;
}
// Slot sl of the graph, first pass.  Returns whether it is live.
template <class Rep> HQA_HD bool graph_slot_hash(const State &S, uint32_t sl, Rep &rep) {
    const Graph &g = S.graph;
    if (g.unfinished[sl] == ST_FREE) return false;
    if (S.parts & HQ_CHECK_GRAPH) {
        const uint32_t p = ht_find(g.ht_key, g.ht_mask, g.id[sl]);
        if (p == NONE || g.ht_val[p] != sl) rep.hit(HQ_INV_GRAPH_HASH, g.id[sl]);
    }
    return true;
}
// The run chain of the live producer in slot sl: every edge whose generation matches counts on its consumer in the audit's scratch cnt [n_slots].
// Edges lane, lane + stride, ... of every run (a wavefront: 64 lanes; the host: one); add(&cnt[c]) is an atomic increment on the device.
template <class Add> HQA_HD void graph_edges(const Graph &g, uint32_t sl, uint32_t lane, uint32_t stride, uint32_t *cnt, Add add) {
    if (g.unfinished[sl] == ST_FREE) return;
    uint32_t steps = 0; uint64_t walked = 0;  // a chain holds every run and every edge at most once: one that goes on past either count is a cycle, and the walk ends
    for (uint32_t r = g.head[sl]; r != NONE && r < g.n_runs && steps < g.n_runs; r = g.run_next[r], steps++) {
        const uint32_t off = g.run_off[r], len = g.run_len[r];
        if (off > g.n_edges || len > g.n_edges - off) return;
        walked += len;
        if (walked > g.n_edges) return;
        for (uint32_t e = lane; e < len; e += stride) {
            const uint32_t c = g.edge[2 * (size_t)(off + e)], gn = g.edge[2 * (size_t)(off + e) + 1];
            if (c < g.n_slots && g.gen[c] == gn) add(&cnt[c]);
        }
    }
}
// Slot sl of the graph, second pass (cnt complete; nullptr when the GRAPH part was not asked for).
template <class Rep> HQA_HD void graph_slot_counter(const State &S, uint32_t sl, const uint32_t *cnt, Rep &rep) {
    const Graph &g = S.graph;
    const uint32_t unf = g.unfinished[sl];
    if (unf == ST_FREE) return;
    const uint64_t id = g.id[sl];
    if ((S.parts & HQ_CHECK_GRAPH) && cnt && unf != cnt[sl]) rep.hit(HQ_INV_GRAPH_COUNTER, id);
    const uint32_t need = HAVE_READY | HAVE_LEDGER | HAVE_TRACKING;
    if ((S.parts & HQ_CHECK_STRICT) && (S.have & need) == need && unf == 0 && !ready_live(S.ready, id) && ht_find(S.ledger.key, S.ledger.mask, id) == NONE)
        rep.hit(HQ_INV_S_RELEASED_NOWHERE, id);
}
// ---- the ledger (Worker::sanity_check server/worker.rs:236-271 and the multi-node arm of Core::sanity_check)
HQA_HD uint32_t row_of(const Ledger &l, uint32_t wid) {  // ids ascend in row order
    uint32_t lo = 0, hi = l.W;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (l.wid[mid] < wid) lo = mid + 1; else hi = mid; }
    return (lo < l.W && l.wid[lo] == wid) ? lo : NONE;
}
HQA_HD uint64_t sat_add(uint64_t a, uint64_t b) { uint64_t r; return __builtin_add_overflow(a, b, &r) ? UINT64_MAX : r; }
HQA_HD uint64_t sat_mul(uint64_t a, uint64_t b) { uint64_t r; return __builtin_mul_overflow(a, b, &r) ? UINT64_MAX : r; }
// Row w, first pass (before the buckets): its multi-node columns.  A root row counts on its task's bucket in x.roots.
template <class Rep, class Add> HQA_HD void ledger_mn_row(const State &S, uint32_t w, const LedgerScratch &x, Rep &rep, Add add) {
    const Ledger &l = S.ledger;
    const uint64_t task = l.mn_task[w];
    if (task == HT_EMPTY) { if (l.mn_root[w]) rep.hit(HQ_INV_LEDGER_MN, l.wid[w]); return; }  // (SN clear and no task is allowed: hqtick_assigned_add_mn documents it)
    bool bad = false;
    const uint32_t b = ht_find(l.key, l.mask, task);
    if (b == NONE || l.variant[b] != MN_VARIANT) bad = true;
    else if (l.mn_root[w]) { if (l.worker[b] == l.wid[w]) add(&x.roots[b]); else bad = true; }
    if (l.flags[w] & HQ_WORKER_SN) bad = true;
    for (uint32_t s = 0; s < l.stride && !bad; s++) if (l.counts[(size_t)w * l.stride + s]) bad = true;
    if (bad) rep.hit(HQ_INV_LEDGER_MN, task);
}
// Bucket b (x.roots complete).  Returns what the bucket holds, for the census of the totals.
template <class Rep, class Add> HQA_HD uint32_t ledger_entry(const State &S, uint32_t b, const LedgerScratch &x, Rep &rep, Add add) {
    const Ledger &l = S.ledger;
    const uint64_t k = l.key[b];
    if (k >= HT_TOMB) return CLS_NONE;
    const uint32_t v = l.variant[b], cls = v == MN_VARIANT ? CLS_MN : v == PF_VARIANT ? CLS_PF : CLS_SN;
    if ((S.parts & HQ_CHECK_STRICT) && graph_nonempty(S)) {
        const uint32_t sl = graph_slot(S.graph, k);
        if (sl == NONE || S.graph.unfinished[sl] != 0) rep.hit(HQ_INV_S_ASSIGNED_WAITING, k);
    }
    if (!(S.parts & HQ_CHECK_LEDGER)) return cls;
    if (ht_find(l.key, l.mask, k) != b) rep.hit(HQ_INV_LEDGER_HASH, k);
    const uint32_t row = row_of(l, l.worker[b]), rq = l.rq[b];
    bool ok = row != NONE && rq < l.Q;
    if (ok) {
        const uint32_t s0 = l.rq_off[rq], nvar = l.rq_off[rq + 1] - s0;
        if (cls == CLS_SN) {  // an entry the count table has no column for cannot be counted anywhere: not a valid entry either
            ok = v < nvar && s0 + v < l.stride;
            if (ok) add(&x.cen_counts[(size_t)row * l.stride + s0 + v]);
        } else if (cls == CLS_MN) {
            ok = s0 < l.NV && l.var_nodes[s0] > 0;
            if (ok && x.roots[b] != 1) rep.hit(HQ_INV_LEDGER_MN, k);  // exactly one root row, and it is the entry's worker
        } else {
            ok = (S.have & HAVE_TRACKING) && l.pf && rq < l.pf_stride;
            if (ok) add(&x.cen_pf[(size_t)row * l.pf_stride + rq]);
        }
    }
    if (!ok) rep.hit(HQ_INV_LEDGER_ENTRY, k);
    return cls;
}
// Item i = (row, slot) of the count table / (row, request) of the prefilled table / (row, resource) of the free rows (the census complete)
template <class Rep> HQA_HD void ledger_count_item(const State &S, uint64_t i, const LedgerScratch &x, Rep &rep) {
    const Ledger &l = S.ledger;
    if (l.counts[i] != x.cen_counts[i]) rep.hit(HQ_INV_LEDGER_COUNTS, (uint64_t)l.wid[i / l.stride] << 32 | (uint32_t)(i % l.stride));
}
template <class Rep> HQA_HD void ledger_pf_item(const State &S, uint64_t i, const LedgerScratch &x, Rep &rep) {
    const Ledger &l = S.ledger;
    if (l.pf[i] != x.cen_pf[i]) rep.hit(HQ_INV_LEDGER_PREFILLED, (uint64_t)l.wid[i / l.pf_stride] << 32 | (uint32_t)(i % l.pf_stride));
}
// free[row][r] == what resources.clone() followed by remove(rq) per assigned task leaves (workerload.rs:156-166): 0 if a running (rq, variant) has an ALL entry
// on r, else total - sum of count * amount, saturating at 0.  The removes commute, so the value follows from the count table and the request tables alone — and
// a release batch applied as "B (ALL), then A (AMOUNT)", which leaves total + amount(A), IS reported: the reference's own check would assert on it.
template <class Rep> HQA_HD void ledger_free_item(const State &S, uint64_t i, Rep &rep) {
    const Ledger &l = S.ledger;
    const uint32_t w = (uint32_t)(i / l.R), r = (uint32_t)(i % l.R);
    if (!(l.flags[w] & HQ_WORKER_SN)) return;  // (a worker on a multi-node task: its free row stays as it was)
    bool all = false; uint64_t sum = 0;
    const uint32_t ns = l.NV < l.stride ? l.NV : l.stride;
    for (uint32_t s = 0; s < ns; s++) {
        const uint32_t c = l.counts[(size_t)w * l.stride + s];
        if (!c) continue;
        for (uint32_t e = l.ventry_off[s]; e < l.ventry_off[s + 1]; e++) {
            if (l.ent_res[e] != r) continue;
            if (l.ent_kind[e] == HQ_ENTRY_ALL) all = true; else sum = sat_add(sum, sat_mul(c, l.ent_amount[e]));
        }
    }
    const uint64_t total = l.total[i], want = all ? 0 : (total > sum ? total - sum : 0);
    if (l.free_[i] != want) rep.hit(HQ_INV_LEDGER_FREE, (uint64_t)l.wid[w] << 32 | r);
}
// Entry j of the Retracting table (CROSS)
template <class Rep> HQA_HD void retr_entry(const State &S, uint32_t j, Rep &rep) {
    const uint64_t id = S.retr.task[j];
    const uint8_t f = S.retr.flags[j];
    bool bad = false;
    if ((f & RETR_IN_QUEUE) && (S.have & HAVE_READY) && !ready_live(S.ready, id)) bad = true;
    if ((f & RETR_REDIRECT) && (S.have & HAVE_LEDGER_SETTLED)) {
        const uint32_t b = ht_find(S.ledger.key, S.ledger.mask, id);
        if (b == NONE || S.ledger.worker[b] != S.retr.target[j] || S.ledger.variant[b] != S.retr.variant[j] || S.ledger.variant[b] >= PF_VARIANT) bad = true;
    }
    if (bad) rep.hit(HQ_INV_X_RETRACTING, id);
}
// which passes a State needs
HQA_HD bool wants_ready_pass(const State &S) { return (S.have & HAVE_READY) && S.ready.n && (parts_present(S) & (HQ_CHECK_READY | HQ_CHECK_CROSS | HQ_CHECK_STRICT)); }
HQA_HD bool wants_graph_pass(const State &S) { return (S.have & HAVE_GRAPH) && S.graph.n_slots && (parts_present(S) & (HQ_CHECK_GRAPH | HQ_CHECK_STRICT)); }
HQA_HD bool wants_ledger_part(const State &S) { return (parts_present(S) & HQ_CHECK_LEDGER) != 0; }  // all of the ledger's passes
HQA_HD bool wants_ledger_pass(const State &S) { return (S.have & HAVE_LEDGER) && (wants_ledger_part(S) || (graph_nonempty(S) && (parts_present(S) & HQ_CHECK_STRICT))); }  // the bucket pass
HQA_HD bool wants_retr_pass(const State &S) { return S.retr.n && (parts_present(S) & HQ_CHECK_CROSS); }

// ---- the end of an audit, on the host: the censuses against the host's counts, then the report's summary
inline void hit_host(uint64_t *count, uint64_t *first, uint32_t inv, uint64_t key) { count[inv]++; if (key < first[inv]) first[inv] = key; }
inline void finish_report(const State &S, const Totals &t, uint64_t ready_live_seen, uint64_t graph_live_seen, const uint64_t *ledger_seen, uint64_t *count, uint64_t *first,
                          hqtick_check_report *out) {
    const uint32_t present = parts_present(S);
    if ((present & HQ_CHECK_LEDGER) && (ledger_seen[0] != S.ledger.n_live || ledger_seen[1] != S.ledger.mn_live || ledger_seen[2] != ((S.have & HAVE_TRACKING) ? S.ledger.pf_live : 0))) {
        const uint64_t cap = (1ull << 21) - 1;  // sn | mn << 21 | pf << 42 of the census, each field saturated
        auto f = [&](uint64_t v) { return v < cap ? v : cap; };
        hit_host(count, first, HQ_INV_LEDGER_TOTALS, f(ledger_seen[0]) | f(ledger_seen[1]) << 21 | f(ledger_seen[2]) << 42);
    }
    if ((present & HQ_CHECK_READY) && ready_live_seen != t.ready_live) hit_host(count, first, HQ_INV_READY_COUNT, ready_live_seen);
    if ((present & HQ_CHECK_GRAPH) && (graph_live_seen != t.graph_tasks || graph_live_seen + t.graph_free != t.graph_slots)) hit_host(count, first, HQ_INV_GRAPH_TOTALS, graph_live_seen);
    out->checked = present; out->n_failed = 0;
    for (uint32_t k = 0; k < HQ_INV_N; k++) { out->count[k] = count[k]; out->first[k] = first[k]; out->n_failed += count[k] != 0; }
}

// ---- the host backend: every pass with one emulated thread per item, the threads of a pass in the given order (0 ascending, 1 descending, 2 a fixed
// permutation).  The report must not depend on it: a pass whose result did would be a data race on the GPU.
struct HostRep { uint64_t *count, *first; void hit(uint32_t inv, uint64_t key) { hit_host(count, first, inv, key); } };
inline uint64_t emu_index(uint64_t i, uint64_t n, int order) {
    if (order == 1) return n - 1 - i;
    if (order == 2) { const uint64_t p = n % 7919 ? 7919 : 7927; return (i * p + n / 3) % n; }  // p is prime and does not divide n: a bijection of [0, n)
    return i;
}
inline void run_host(const State &S, const Totals &t, int order, hqtick_check_report *out) {
    uint64_t count[HQ_INV_N], first[HQ_INV_N];
    for (uint32_t k = 0; k < HQ_INV_N; k++) { count[k] = 0; first[k] = UINT64_MAX; }
    HostRep rep{count, first};
    uint64_t ready_seen = 0, graph_seen = 0, ledger_seen[3] = {0, 0, 0};
    if (wants_ready_pass(S)) for (uint64_t i = 0; i < S.ready.n; i++) ready_seen += ready_row(S, emu_index(i, S.ready.n, order), rep);
    if (wants_graph_pass(S)) {
        const uint32_t n = S.graph.n_slots;
        const bool counters = (S.parts & HQ_CHECK_GRAPH) != 0;
        std::vector<uint32_t> cnt(counters ? n : 0, 0u);
        for (uint32_t i = 0; i < n; i++) graph_seen += graph_slot_hash(S, (uint32_t)emu_index(i, n, order), rep);
        if (counters) for (uint32_t i = 0; i < n; i++) graph_edges(S.graph, (uint32_t)emu_index(i, n, order), 0, 1, cnt.data(), [](uint32_t *p) { ++*p; });
        for (uint32_t i = 0; i < n; i++) graph_slot_counter(S, (uint32_t)emu_index(i, n, order), counters ? cnt.data() : nullptr, rep);
    }
    if (wants_ledger_pass(S)) {
        const Ledger &l = S.ledger;
        const uint64_t nb = (uint64_t)l.mask + 1, nc = (uint64_t)l.W * l.stride, np = (S.have & HAVE_TRACKING) && l.pf ? (uint64_t)l.W * l.pf_stride : 0, nf = (uint64_t)l.W * l.R;
        const bool part = wants_ledger_part(S);
        std::vector<uint32_t> cen_counts(part ? nc : 0, 0u), cen_pf(part ? np : 0, 0u), roots(part ? nb : 0, 0u);
        const LedgerScratch x{cen_counts.data(), cen_pf.data(), roots.data()};
        auto inc = [](uint32_t *p) { ++*p; };
        if (part) for (uint32_t w = 0; w < l.W; w++) ledger_mn_row(S, (uint32_t)emu_index(w, l.W, order), x, rep, inc);
        for (uint64_t b = 0; b < nb; b++) { const uint32_t cls = ledger_entry(S, (uint32_t)emu_index(b, nb, order), x, rep, inc); if (cls) ledger_seen[cls - 1]++; }
        if (part) {
            for (uint64_t i = 0; i < nc; i++) ledger_count_item(S, emu_index(i, nc, order), x, rep);
            for (uint64_t i = 0; i < np; i++) ledger_pf_item(S, emu_index(i, np, order), x, rep);
            for (uint64_t i = 0; i < nf; i++) ledger_free_item(S, emu_index(i, nf, order), rep);
        }
    }
    if (wants_retr_pass(S)) for (uint32_t j = 0; j < S.retr.n; j++) retr_entry(S, (uint32_t)emu_index(j, S.retr.n, order), rep);
    finish_report(S, t, ready_seen, graph_seen, ledger_seen, count, first, out);
    out->kernel_us = 0.0;
}

}  // namespace hqaudit

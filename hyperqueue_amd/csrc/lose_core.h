// hqtick_lose_workers (include/hqtick.h): the rule that names what a lost worker's ledger entry was, the layouts of the call's buffers and the
// phases of its grouping.  Plain host + device code without a HIP include: assigned.hip's gather kernel calls the rule per evicted entry, its group kernel runs the
// two grouping phases, ledger.cpp sizes its buffers by the layouts, and hqtick_debug_lose_kind / hqtick_debug_lose_group run the same functions on host arrays
// so that the CPU suite pins them.
//
// The grouping turns the evicted entries -- ids ascending, each with the index of its worker in the caller's list -- into a CSR over that list.  The stable sort
// by worker index is hqcancel::sort_rows (cancel_core.h: no output position depends on the order anything arrives in); a stable sort of id-ascending positions
// leaves the ids ascending inside a worker.  Behind it every output element is a function of the sorted arrays alone: offset g is the first sorted position whose
// key is not below g (a binary search per worker), element j is the gathered record of position pos[j].
#pragma once

#include <cstddef>
#include <cstdint>
#include <new>

#include "../../include/hqtick.h"
#include "cancel_core.h"

#if defined(__HIPCC__)
#define HQ_LOSE_HD __host__ __device__ inline
#else
#define HQ_LOSE_HD inline
#endif

namespace hqlose {

// the variant class of a ledger entry (finish_core.h's values)
enum EntryClass : uint32_t { E_SN = 0, E_MN = 1, E_PF = 2 };

// What an entry of a lost worker was, from its variant column and running byte (on_remove_worker, server/reactor.rs:64-147).  A multi-node entry is its ROOT's
// (its worker column names the root), so one that is hit was lost with its root; the running byte of multi-node and prefilled entries is always 0 and is not read.
HQ_LOSE_HD uint32_t kind_of_entry(uint32_t entry_class, bool entry_run) {
    return entry_class == E_MN ? HQ_LOSE_MN_ROOT : entry_class == E_PF ? HQ_LOSE_PREFILLED : entry_run ? HQ_LOSE_RUNNING : HQ_LOSE_ASSIGNED;
}
// ... and what the host makes of it once it has looked the id up in the Retracting table: a single-node entry on the worker that is the task's redirect TARGET is
// the redirect's entry (reactor.rs:90-96), whatever its running byte says; multi-node and prefilled tasks are never in that table
HQ_LOSE_HD uint32_t settle(uint32_t kind, bool redirect_target) {
    return redirect_target && (kind == HQ_LOSE_ASSIGNED || kind == HQ_LOSE_RUNNING) ? (uint32_t)HQ_LOSE_REDIRECT : kind;
}
// on_remove_worker's running_tasks: what client.on_worker_lost is told and what gets a crash counter
HQ_LOSE_HD bool is_running(uint32_t kind) { return kind == HQ_LOSE_RUNNING || kind == HQ_LOSE_MN_ROOT; }

// ---- the grouping's phases.  key / pos [k]: the worker indices sorted (stable) and the id-ascending positions in that order ----
struct GroupArgs {
    uint32_t k, n_workers;
    const uint32_t *key, *pos;
    const uint64_t *id, *prio; const uint32_t *rq; const uint8_t *kind;        // [k], ids ascending: what the gather wrote
    uint32_t *off; uint64_t *out_id, *out_prio; uint32_t *out_rq; uint8_t *out_kind;  // off [n_workers + 1], the columns [k]
};
// thread g <= n_workers: where worker g's tasks begin (g == n_workers: k)
HQ_LOSE_HD void grp_p_offset(const GroupArgs &a, uint32_t g) {
    if (g > a.n_workers) return;
    uint32_t lo = 0, hi = a.k;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (a.key[mid] < g) lo = mid + 1; else hi = mid; }
    a.off[g] = lo;
}
// thread j < k: the record of sorted position j
HQ_LOSE_HD void grp_p_gather(const GroupArgs &a, uint32_t j) {
    if (j >= a.k) return;
    const uint32_t p = a.pos[j];
    a.out_id[j] = a.id[p]; a.out_prio[j] = a.prio[p]; a.out_rq[j] = a.rq[p]; a.out_kind[j] = a.kind[p];
}

// ---- layouts: where the call's columns sit in its two buffers, for at most `cap` evicted entries of n lost workers (sort_cap: hqgraph::sort_capacity(cap)) ----
HQ_LOSE_HD size_t al8(size_t x) { return (x + 7) & ~(size_t)7; }
// device: [sort key u64 sort_cap][id u64 cap][priority u64 cap][sort value u32 sort_cap][rq u32 cap][worker index u32 cap][lost sorted u32 n][their indices u32 n]
//         [lost in the caller's order u32 n][the grouping's sort scratch u32][kind u8 cap]
struct DevLayout { size_t skey, id, prio, sval, rq, widx, lost, lost_idx, call, scratch, kind, bytes; };
HQ_LOSE_HD DevLayout dev_layout(size_t cap, size_t sort_cap, uint32_t n) {
    DevLayout L{};
    size_t o = 0;
    L.skey = o; o += sort_cap * 8; L.id = o; o += cap * 8; L.prio = o; o += cap * 8;
    L.sval = o; o += sort_cap * 4; L.rq = o; o += cap * 4; L.widx = o; o += cap * 4;
    L.lost = o; o += (size_t)n * 4; L.lost_idx = o; o += (size_t)n * 4; L.call = o; o += (size_t)n * 4;
    o = al8(o); L.scratch = o; o += hqcancel::scratch_of((uint32_t)cap, n).total * 4;
    L.kind = o; o += cap;
    L.bytes = al8(o) + 64;
    return L;
}
// pinned: in [lost sorted n][indices n][caller's order n] u32 (one copy to the device); out: the flat list [id u64 cap][priority u64 cap][rq u32 cap], the CSR
// [id u64 cap][priority u64 cap][rq u32 cap][offsets u32 n + 1][kind u8 cap], per lost worker [multi-node task u64 n][its root's worker id u32 n]
struct PinLayout { size_t in, f_id, f_prio, c_id, c_prio, m_task, f_rq, c_rq, off, m_root, c_kind, bytes; };
HQ_LOSE_HD PinLayout pin_layout(size_t cap, uint32_t n) {
    PinLayout L{};
    size_t o = 0;
    L.in = o; o = al8(o + (size_t)n * 12);
    L.f_id = o; o += cap * 8; L.f_prio = o; o += cap * 8; L.c_id = o; o += cap * 8; L.c_prio = o; o += cap * 8; L.m_task = o; o += (size_t)n * 8;
    L.f_rq = o; o += cap * 4; L.c_rq = o; o += cap * 4; L.off = o; o += ((size_t)n + 1) * 4; L.m_root = o; o += (size_t)n * 4;
    L.c_kind = o; o += cap;
    L.bytes = al8(o) + 64;
    return L;
}

// ---- host execution (debug hook, sanitizer program): the stable sort is cancel_core.h's own host execution (its compact lists of the positions 0 .. k - 1 by
// "row" = worker index), the two phases above run one emulated thread after the other in the given order (0 ascending, 1 descending, 2 scattered).  Every array
// is a heap block of its exact size.  widx [k] must be below n_workers.  Out: off [n_workers + 1], the columns [k]. ----
inline bool group_on_host(uint32_t k, uint32_t n_workers, const uint64_t *id, const uint64_t *prio, const uint32_t *rq, const uint8_t *kind, const uint32_t *widx, int order,
                          uint32_t *off, uint64_t *out_id, uint64_t *out_prio, uint32_t *out_rq, uint8_t *out_kind) {
    uint64_t *ident = new (std::nothrow) uint64_t[k], *sorted = new (std::nothrow) uint64_t[k];
    uint32_t *rows = new (std::nothrow) uint32_t[n_workers], *s_wid = new (std::nothrow) uint32_t[n_workers], *s_off = new (std::nothrow) uint32_t[(size_t)n_workers + 1];
    uint32_t *key = new (std::nothrow) uint32_t[k], *pos = new (std::nothrow) uint32_t[k];
    bool ok = ident && sorted && rows && s_wid && s_off && key && pos;
    if (ok) {
        for (uint32_t j = 0; j < k; j++) ident[j] = j;
        for (uint32_t w = 0; w < n_workers; w++) rows[w] = w;
        uint32_t n_rows = 0, n_ids = 0;
        ok = hqcancel::group_on_host(k, n_workers, widx, ident, rows, order, &n_rows, &n_ids, s_wid, s_off, sorted) && n_ids == k;
        if (ok) {
            for (uint32_t j = 0; j < k; j++) { pos[j] = (uint32_t)sorted[j]; key[j] = widx[pos[j]]; }
            const GroupArgs a{k, n_workers, key, pos, id, prio, rq, kind, off, out_id, out_prio, out_rq, out_kind};
            const uint32_t threads = k > n_workers + 1 ? k : n_workers + 1;
            for (uint32_t q = 0; q < threads; q++) {
                const uint32_t g = order == 1 ? threads - 1 - q : order == 2 ? (uint32_t)(((uint64_t)q * 77 + 13) % threads) : q;  // (order 2 may visit a thread twice: the phases are idempotent)
                grp_p_offset(a, g); grp_p_gather(a, g);
            }
            if (order == 2) for (uint32_t g = 0; g < threads; g++) { grp_p_offset(a, g); grp_p_gather(a, g); }  // ... and every thread at least once
        }
    }
    delete[] ident; delete[] sorted; delete[] rows; delete[] s_wid; delete[] s_off; delete[] key; delete[] pos;
    return ok;
}

}  // namespace hqlose

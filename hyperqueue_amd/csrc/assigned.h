// Assignment ledger: every single-node task in state Assigned / Running — and every Retracting task counted on its
// redirect target (server/worker.rs:249-252) — with the worker it runs on, kept in HBM between ticks, together with the per-worker
// (rq, variant) counts that GapCache and Worker::is_free read and the free rows of the resident worker set.
//
// Layout:
//   id -> entry: open-addressing hash table (linear probing, tombstones, rebuilt at half load), SoA columns indexed by bucket:
//     key u64 (HT_EMPTY / HT_TOMB) | worker id u32 | rq u32 | variant u8 | priority u64 | claim u32 (batch position of a release, else NONE)
//     | run u8 (1: the task was reported running; 0 on every entry that enters, and always on multi-node and prefilled entries)
//   counts u32 [W x stride]: running tasks per (worker row, variant slot); slot = rq_variant_off[rq] + variant
//   free / total rows: the resident worker set's own rows in HBM (hqtick_cluster_*), updated in place
//   multi-node tasks (Worker::mn_task, server/worker.rs:134-175): three more columns per worker row, 10 B per row, re-packed with the count rows
//     mn task u64 [W] (HT_EMPTY: the row holds none) | mn root u8 [W] (1: the row is its task's root) | flags u8 [W] (HQ_WORKER_* bits, the mirror's byte)
//   and one table entry per task: key = task id, worker = the ROOT's worker id, rq, priority, variant = MN_VARIANT (0xFF: no single-node entry carries
//   it — a request has fewer than 255 variants).  It counts in no (row, slot) and touches no free row while it runs.
//   Invariant: a row's mn task is a live MN_VARIANT entry of the table.  Release and eviction tombstone the entry first; the row pass that follows resets
//   every row whose task is no longer found (reset_mn_task: SN bit set, free row = total row, columns cleared).
//   prefilled tasks (SingleNodeTaskAssignment::prefilled_tasks, opt-in: hqtick_assigned_track_prefilled): one table entry per task, key = task id, worker = the
//   worker it is prefilled on, rq, priority, variant = PF_VARIANT (0xFE: with tracking on a request has fewer than 254 variants).  It counts in no (row, slot)
//   and touches no free row.  pf u32 [W x pf_stride]: prefilled tasks per (worker row, request), a second table re-packed by the count rows' launch.
//   Invariant: pf[w][q] = live PF_VARIANT entries of worker w and request q.  Rows::pf == nullptr (tracking off): no kernel reads or writes the table and a
//   PREFILL record of the staging is skipped, as before.
// Everything here is integer work bound by HBM latency; no MFMA.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hqasg {

constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint64_t HT_EMPTY = ~0ull, HT_TOMB = ~0ull - 1;  // task ids must be below HT_TOMB
constexpr uint32_t RQ_LOOKUP = 0xFFFFFFFFu;              // insert item whose rq / priority come from the ready-set columns
constexpr uint8_t MN_VARIANT = 0xFF;                     // variant column of a multi-node task's entry
constexpr uint8_t PF_VARIANT = 0xFE;                     // variant column of a prefilled task's entry

struct Table {
    uint64_t *key; uint32_t *worker; uint32_t *rq; uint8_t *variant; uint64_t *prio; uint32_t *claim; uint8_t *run;
    uint32_t mask;  // capacity - 1 (a power of two)
};
// the request tables (ResourceRqMap) as the ledger needs them: rq -> variant slots -> entries
struct Req {
    const uint32_t *rq_off; const uint32_t *ventry_off; const uint32_t *ent_res; const uint8_t *ent_kind; const uint64_t *ent_amount;
    uint32_t Q;
};
// the resident worker set: ids in row order, total / free rows, the count table
struct Rows {
    const uint32_t *wid; uint32_t W, R;
    const uint64_t *total; uint64_t *free_;
    uint32_t *counts; uint32_t stride;
    uint32_t *pf; uint32_t pf_stride;  // prefilled tasks per (row, request); nullptr: not tracked (a uniform argument)
};
// the multi-node columns of the worker rows (all nullptr: a caller without them); live = multi-node entries in the table as the host counts them — a
// uniform argument: with live == 0 no kernel reads the columns
struct MnRows {
    uint64_t *task; uint8_t *root; uint8_t *flags;
    uint32_t live;
};
// multi-node placements: task i runs on the workers wid[off[i] .. off[i + 1]), root first.  prio == nullptr: the priority is looked up by id in the
// ready-set columns col_id / col_prio (a consumed task keeps its id and priority)
struct MnItems {
    uint32_t n, n_wid;
    const uint64_t *id; const uint32_t *rq; const uint64_t *prio; const uint32_t *off; const uint32_t *wid;
    const uint64_t *col_id; const uint64_t *col_prio; uint64_t col_n;
};
// an insert batch from explicit columns (wid: worker ids)
struct Items {
    uint32_t n;
    const uint64_t *id; const uint32_t *wid; const uint32_t *rq; const uint8_t *variant; const uint64_t *prio;
    // rq / priority of an item with rq == RQ_LOOKUP: the ready-set columns, ids ascending
    const uint64_t *col_id; const uint64_t *col_prio; const uint32_t *col_rq; uint64_t col_n;
    uint8_t run;  // the running byte every entry of the batch enters with (hqtick_retracting_started: 1)
};
// a tick's placement as the mapping kernel staged it in HBM (kernels.h: hqk::Stage), one entry per record; meta = variant | kind << 8, entries whose kind
// is HQ_REC_PREFILL enter as PF_VARIANT entries when the prefilled tasks are tracked (Rows::pf) and are skipped otherwise.  The priority is levels[level] (the dense scan's level table, n_levels entries); levels == nullptr (the ordered view,
// whose run table lives in host memory): the priority alone is looked up by id in the ready-set columns col_id / col_prio.
struct Staged {
    uint32_t n;
    const uint64_t *task; const uint32_t *rq; const uint32_t *row; const uint32_t *level; const uint16_t *meta;
    const uint64_t *levels; uint32_t n_levels;
    const uint64_t *col_id; const uint64_t *col_prio; uint64_t col_n;
};
// counters of one operation, in device memory, one atomic per wavefront (insert: C_OUT = entries that were not there before; evict: entries gathered)
// (C_MN: the multi-node entries among C_DONE of a release / C_OUT of an eviction)
// (C_PF: prefilled entries — entered by the staged placement or a seed, turned into assigned entries by an upsert, gathered by an eviction)
enum Ctr : uint32_t { C_DONE = 0, C_UNKNOWN = 1, C_DUP = 2, C_FULL = 3, C_BAD = 4, C_OUT = 5, C_MN = 6, C_PF = 7, C_N = 8 };

hipError_t clear(Table t, hipStream_t s);
// insert (upsert != 0: an id already present moves to the new worker / variant, its old count is given back; else it is counted as a duplicate).
// apply_free != 0: Worker::insert_sn_task's free.remove on the worker's row (AMOUNT subtracts with saturation, ALL sets 0; these commute).
// An id that is a prefilled entry (a FROM_PREFILL redirect): rq and priority are the entry's own, the old worker's prefilled count drops and the entry becomes
// the assigned entry on the new worker (counted in C_DONE and C_PF, not in C_OUT); without upsert it is a duplicate like any other.
hipError_t insert(Table t, Req q, Rows r, Items it, int upsert, int apply_free, uint32_t *ctr, hipStream_t s);
// the staged placement of a tick as upserts, free rows untouched (they become the tick's new_free); with r.pf its PREFILL entries enter too (C_PF)
hipError_t insert_staged(Table t, Req q, Rows r, Staged st, uint32_t *ctr, hipStream_t s);
// release in batch order with the last-ALL rule; scratch: pos [n] u32, last_all [W * R] u32, delta [W * R] u64 (zero on entry and on return).
// A multi-node id of the batch leaves the table like the others (counted in C_DONE and C_MN); with m.live != 0 the W x R row pass resets its rows.
// A prefilled id is not the release's: it is counted as unknown and stays.
hipError_t release(Table t, Req q, Rows r, MnRows m, uint32_t n, const uint64_t *id, uint32_t *pos, uint32_t *last_all, uint64_t *delta, uint32_t *ctr, hipStream_t s);
// hqtick_cancel_tasks: the release's four passes in their cancel mode.  A prefilled id of the batch leaves too, as pf_remove takes it (prefilled count
// down, no free row; counted in C_DONE and C_PF), so the tables end as after release(ids) + pf_remove(ids).  Per batch position the passes write the worker ROW the
// CancelTasks message goes to (NONE: none) and an HQ_CANCEL_* kind: the entry's worker, the root of a multi-node task; REPEAT for a later position of an id that
// has an entry.  The Retracting overrides (ids ascending, the worker id each task is retracting FROM; retr_hit [n_retr] NONE on entry) are matched on the device:
// the first position of such an id is routed to that worker whatever the ledger names, and retr_hit[k] is that position (NONE: the id is not in the batch).
struct CancelCols { uint32_t *route; uint8_t *kind; const uint64_t *retr_id; const uint32_t *retr_wid; uint32_t *retr_hit; uint32_t n_retr; const uint32_t *reporter; };
hipError_t cancel(Table t, Req q, Rows r, MnRows m, uint32_t n, const uint64_t *id, uint32_t *pos, uint32_t *last_all, uint64_t *delta, CancelCols cc, uint32_t *ctr, hipStream_t s);
// hqtick_finish_tasks: the four passes in their finish mode.  cc.reporter [n] is the worker id every position was reported by (cc.route is not
// used: nobody is told).  finish_core.h's rule gives every position an HQ_FINISH_* kind in cc.kind; only the positions whose reporter is the entry's worker (the
// root of a multi-node task; for an id of the Retracting overrides the worker it is retracting FROM, whatever the ledger names) may claim, the lowest of them
// wins, and the tables end as after release(the accepted ids in batch order).  A prefilled entry is never claimed.  retr_hit[k]: the position that claimed
// override k (NONE: none did).  ctr[C_OUT]: the accepted positions (C_DONE of them left the table; the others are Retracting ids without an entry).
hipError_t finish(Table t, Req q, Rows r, MnRows m, uint32_t n, const uint64_t *id, uint32_t *pos, uint32_t *last_all, uint64_t *delta, CancelCols cc, uint32_t *ctr, hipStream_t s);
// hqtick_fail_tasks: the four passes in their fail mode, the finish mode with fail_core.h's rule and HQ_FAIL_* kinds.  A reporter of HQ_NO_WORKER
// makes a position _WAITING (accepted, nothing here to claim) or _NOT_WAITING; a prefilled entry reported by its worker is claimed and leaves as pf_remove takes it
// (prefilled count down, no free row; counted in C_DONE and C_PF), so the tables end as after release(accepted ids in batch order) + pf_remove(those ids).
hipError_t fail(Table t, Req q, Rows r, MnRows m, uint32_t n, const uint64_t *id, uint32_t *pos, uint32_t *last_all, uint64_t *delta, CancelCols cc, uint32_t *ctr, hipStream_t s);
// hqtick_reject_tasks: the four passes in their reject mode, the fail mode with reject_core.h's rule and HQ_REJECT_* kinds, then the requeue's
// compaction.  variant [n] is the rejected variant per position (0xFF: None), rq_in [n] (nullptr with n_retr == 0) the request of a position the Retracting
// overrides decide.  An override position never claims a ledger entry (a redirect target's entry stays); its kind comes back as _RETRACTING and the host settles it
// against _REDIRECTED.  An _ASSIGNED entry leaves as by release, a _PREFILLED one as by pf_remove (C_DONE / C_PF); before its key becomes a tombstone the apply pass
// records (priority, request) at its position and sets flag[i].  blk_rq [n]: the request whose (request, variant[i]) pair the position adds to its reporter's
// blocked set by the kind pass 1 gave it (NONE: none; the host drops those of positions that ended as _REPEAT).
// The compaction reads the flags through perm [n] -- the positions by ascending (id, position), staged by the host -- so the output order is that of the ids and
// does not depend on the order atomics arrive in: a count per 256-position slice, hqk::scan_waves over the slice table (slices [>= n_slices rounded up to 16], the
// total lands in *total), a write of the three dense columns into out_* (device, for the merge) and o_* (pinned, for the host).  Claims make every id accepted at
// most once, so the ids come out strictly ascending.  ctr[C_OUT]: the accepted positions.
struct RejectCols {
    const uint8_t *variant; const uint32_t *rq_in; const uint32_t *perm;
    uint32_t *blk_rq; uint8_t *flag; uint64_t *rec_prio; uint32_t *rec_rq;
    uint32_t *slices; uint32_t *total;
    uint64_t *out_id; uint64_t *out_prio; uint32_t *out_rq;
    uint64_t *o_id; uint64_t *o_prio; uint32_t *o_rq;
};
hipError_t reject(Table t, Req q, Rows r, MnRows m, uint32_t n, const uint64_t *id, uint32_t *pos, uint32_t *last_all, uint64_t *delta, CancelCols cc, RejectCols rj, uint32_t *ctr,
                  hipStream_t s);
// every entry of the workers `lost` (sorted ids) leaves the table; (id, rq, priority) appended to out_* [cap_out] (order undefined), count in ctr[C_OUT].
// A multi-node entry is its ROOT's (on_remove_worker, reactor.rs:107-128): a lost root evicts the task, a lost non-root leaves the entry alone.
// out_var [cap_out]: the entry's variant column (PF_VARIANT: it was prefilled; counted in C_PF); out_run [cap_out]: its running byte
hipError_t evict(Table t, uint32_t n_lost, const uint32_t *lost, uint64_t *out_id, uint32_t *out_rq, uint64_t *out_prio, uint8_t *out_var, uint8_t *out_run, uint32_t cap_out, uint32_t *ctr,
                 hipStream_t s);
// hqtick_lose_workers: the eviction with outputs whose order does not depend on the order atomics arrive in.  All pointers are device memory
// unless said otherwise; lose_core.h has the rule and the phases.
//   lose_evict   evict()'s pass over the table: a hit appends (id, bucket) to skey / sval [cap_out] (order undefined) and becomes a tombstone; its other columns
//                stay where they are for the gather.  Counts as evict() (C_OUT, C_MN, C_PF).  With m.live, behind it on the stream: per lost worker i of the
//                caller's order `call` [n_lost], mn_task[i] / mn_root[i] (pinned) = the multi-node task its row holds as a NON-root and that task's root worker id,
//                if the task is still in the table (its root stays); HT_EMPTY otherwise.  mn_reset_rows comes after it.
//   lose_sort    hqgraph::sort_pairs over the k pairs is the caller's (graph.h); lose_gather reads them sorted: position j takes the columns of bucket sval[j] --
//                the three dense columns of the merge (id, prio, rq: device) and, through the same stores, the flat list (o_*: pinned), the kind by
//                hqlose::kind_of_entry and the index of the entry's worker in the caller's list (lost [n_lost] sorted ids, lost_idx [n_lost] their indices).
//   lose_group   hqcancel::sort_rows of the worker indices (scratch: hqcancel::scratch_of(k, n_lost).total u32), then offsets and CSR columns (pinned).
struct LoseCols {
    uint32_t n_lost; const uint32_t *lost, *lost_idx, *call;
    uint64_t *skey; uint32_t *sval;
    uint64_t *id, *prio; uint32_t *rq, *widx; uint8_t *kind;
    uint64_t *o_id, *o_prio; uint32_t *o_rq;
    uint32_t *scratch;
    uint32_t *c_off; uint64_t *c_id, *c_prio; uint32_t *c_rq; uint8_t *c_kind;
    uint64_t *mn_task; uint32_t *mn_root;
};
hipError_t lose_evict(Table t, Rows r, MnRows m, LoseCols lc, uint32_t cap_out, uint32_t *ctr, hipStream_t s);
hipError_t lose_gather(Table t, LoseCols lc, uint32_t k, hipStream_t s);
hipError_t lose_group(LoseCols lc, uint32_t k, hipStream_t s);
// prefilled tasks (r.pf != nullptr in all four).  seed: item i (id, worker id, rq, priority) enters as a PF_VARIANT entry if the worker is resident and has its SN
// bit, the request exists and the id is new (C_DONE entered; C_BAD / C_DUP refused).  start: the entry of id[i] takes variant[i]: pf count down, (row, slot)
// count up, free.remove — all commuting atomics, one pass (C_DONE started; C_UNKNOWN not a prefilled entry, C_BAD no such variant).  remove: the entry leaves,
// pf count down (C_DONE removed, C_UNKNOWN not a prefilled entry).  drop_all: every PF_VARIANT entry leaves (C_DONE); the host clears the pf table.
hipError_t pf_seed(Table t, Req q, Rows r, MnRows m, uint32_t n, const uint64_t *id, const uint32_t *wid, const uint32_t *rq, const uint64_t *prio, uint32_t *ctr, hipStream_t s);
hipError_t pf_start(Table t, Req q, Rows r, uint32_t n, const uint64_t *id, const uint8_t *variant, uint32_t *ctr, hipStream_t s);
hipError_t pf_remove(Table t, Rows r, uint32_t n, const uint64_t *id, uint32_t *ctr, hipStream_t s);
hipError_t pf_drop_all(Table t, uint32_t *ctr, hipStream_t s);
// multi-node placements enter: owner is scratch [W] u32.  Task i enters only if every listed worker is resident, listed once, claimed by no task earlier in
// the batch and holds no multi-node task, and the id is new; check != 0 (hqtick_assigned_add_mn) also wants every worker free of single-node tasks and
// not STOPPING.  Then each row loses its SN bit and records the task (first row: root); free rows stay.  C_DONE entered, C_BAD / C_DUP refused.
hipError_t mn_enter(Table t, Rows r, MnRows m, MnItems it, uint32_t *owner, int check, uint32_t *ctr, hipStream_t s);
// reset_mn_task on every row whose multi-node task is no longer in the table (after an eviction; the release has this inside its own row pass)
hipError_t mn_reset_rows(Table t, Rows r, MnRows m, hipStream_t s);
// live entries of `from` re-inserted into the (cleared) table `to`
hipError_t rehash(Table from, Table to, uint32_t *ctr, hipStream_t s);
// dst row w = src row src_row[w] (NONE or >= W_src: a zero row), columns [0, n_cols).  With ms.task the multi-node columns move in the same launch
// (md: the destination; a new row holds no task and takes its flags byte from new_flags [W_dst]).  With pf.dst the prefilled counts move in the same launch too:
// columns [0, pf.n_cols), pf.n_cols <= n_cols
struct PfMove { const uint32_t *src; uint32_t src_stride; uint32_t *dst; uint32_t dst_stride; uint32_t n_cols; };
hipError_t repack_counts(const uint32_t *src, uint32_t src_stride, uint32_t W_src, const uint32_t *src_row, uint32_t W_dst, uint32_t *dst, uint32_t dst_stride,
                         uint32_t n_cols, MnRows ms, MnRows md, const uint8_t *new_flags, hipStream_t s, PfMove pf = PfMove{});
hipError_t lookup(Table t, uint32_t n, const uint64_t *id, uint32_t *out_wid, uint8_t *out_variant, hipStream_t s);
hipError_t running(Table t, uint32_t n, const uint64_t *id, uint8_t *out_run, hipStream_t s);  // the running byte per id (0xFF: no entry)
// hqtick_start_tasks: two passes over the staged positions [lo, hi) of a batch, one thread per position.  id / reporter / variant [n] are the
// staged columns; mask [n] (nullptr: no position is left out) is nonzero for a position the host decides itself (an id of the Retracting table); pos [n] and kind
// [n] are the passes' own.  start_claim evaluates start_core.h's rule on the tables as they are, writes the provisional kind and lets every _ASSIGNED /
// _PREFILLED position claim its entry (atomicMin on the claim word).  start_apply: the winner sets the running byte, a prefilled entry also takes the winner's
// variant with pf_start's arithmetic (all commuting atomics), and the claim word goes back to NONE -- the entry stays in the table, and a word left behind would
// beat the next batch's claims; a loser becomes _REPEAT.  ctr: C_OUT accepted positions, C_PF started prefills, C_MN multi-node positions.
struct StartCols { const uint64_t *id; const uint32_t *reporter; const uint8_t *variant; const uint8_t *mask; uint32_t *pos; uint8_t *kind; };
hipError_t start_claim(Table t, Req q, Rows r, StartCols sc, uint32_t lo, uint32_t hi, hipStream_t s);
hipError_t start_apply(Table t, Req q, Rows r, StartCols sc, uint32_t lo, uint32_t hi, uint32_t *ctr, hipStream_t s);
hipError_t start_unclaim(Table t, StartCols sc, uint32_t lo, uint32_t hi, hipStream_t s);  // a start that ends early: the claims of [lo, hi) go back to NONE, nothing starts

}  // namespace hqasg

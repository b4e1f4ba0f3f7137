// The host side of the assignment ledger (hqtick_assigned_*, ABI 12): the buffers of csrc/assigned.h's tables, the host's counts of what they
// hold, and one method per ledger operation.  The kernels are assigned.hip's; hqtick.cpp validates the arguments of the C ABI, builds an Env and forwards.
// Like hqgraph::Graph, a method returns an HQTICK_E_* code (negative) with `err` set; it enqueues on the Env's stream and has synchronised it when it returns.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hqtick.h"
#include "assigned.h"
#include "cancel.h"
#include "devbuf.h"

namespace hqasg {

// What a ledger call reads of the context it belongs to, built by hqtick.cpp for the call (by value: the cluster tables move at a membership change).
struct Env {
    int device; hipStream_t stream;
    unsigned char *cluster; uint32_t W, R;  // the resident worker rows in HBM: [total W x R u64][free W x R u64] ...
    const uint64_t *col_id, *col_prio; const uint32_t *col_rq; uint64_t col_n;  // the resident ready-set columns (physical length)
    const uint64_t *levels;                 // the dense scan's level table
    const std::vector<uint32_t> *id; std::vector<uint8_t> *flags; std::vector<uint64_t> *free_;  // the host mirror of the worker set: ids in row order, flags, free rows
};

// the placement staging K5b writes beside a tick's records and insert_staged reads: [task u64 | rq u32 | row u32 | level u32 | meta u16] x n_rec
struct StageCols { uint64_t *task; uint32_t *rq, *row, *level; uint16_t *meta; };
// per worker its distinct (rq, variant) pairs with counts, as a CSR over the workers
struct Agg { const uint32_t *off, *rq, *cnt; const uint8_t *var; };

class Ledger {
  public:
    // Plain state hqtick.cpp reads (and, for `on` and `pending`, sets); the buffers and whatever an operation keeps consistent with them are private.
    bool on = false;       // hqtick_assigned_enable .. _disable / a new worker set / a tick's placement that could not be entered
    bool pending = false;  // a tick's placement waits for hqtick_ready_consume_last (two-call form)
    std::string err;
    uint64_t n_live = 0, mn_live = 0, pf_live = 0;  // single-node, multi-node and (with tracking()) prefilled entries of the table
    uint64_t last_unknown = 0, last_host_bytes = 0;
    std::vector<uint64_t> rq_task, rq_prio, rq_pf_task; std::vector<uint32_t> rq_rq;  // hqtick_cluster_last_requeued(_prefilled): what the last evict() took out
    std::vector<uint64_t> rq_run_task;  // hqtick_cluster_last_requeued_running: its running single-node entries and its multi-node tasks (on_remove_worker's running_tasks)
    // hqtick_cancel_last_*: what the last cancel() wrote into pinned memory (n positions; n_workers messages holding n_ids ids)
    struct CancelOut { uint32_t n = 0, n_workers = 0, n_ids = 0; const uint32_t *worker_id = nullptr, *task_off = nullptr; const uint64_t *task_id = nullptr; const uint32_t *route_wid = nullptr; const uint8_t *route_kind = nullptr; };
    CancelOut cancel_out;
    // hqtick_finish_last_routes: the kinds the last finish() wrote into pinned memory (n positions, `accepted` of them with an accepted kind); d_kind: the same
    // kinds where the passes left them on the device (the graph's skip input; valid until the next cancel() or finish())
    // (kind_dev: the pinned kinds as the device sees them -- the graph step of hqtick_fail_tasks writes the final kinds there)
    struct FinishOut { uint32_t n = 0, accepted = 0; const uint8_t *kind = nullptr; const uint8_t *d_kind = nullptr; uint8_t *kind_dev = nullptr; };
    FinishOut finish_out;
    FinishOut fail_out;  // hqtick_fail_last_routes: the same of the last fail_tasks(); `accepted` and the kinds are final after the graph step
    // hqtick_start_last_routes: the kinds of the last start (pinned, n positions); `accepted` counts the device's accepted positions, the caller adds its own
    struct StartOut { uint32_t n = 0, accepted = 0; uint8_t *kind = nullptr; };
    StartOut start_out;
    // hqtick_reject_last_routes / _last_requeued: the kinds of the last reject (pinned, n positions; the caller settles _REDIRECTED in them), per position the request
    // whose pair it blocks (NONE: none), and what went back into the ready set: n_requeued ids ascending with request and priority, pinned for the host and in
    // device memory (d_*) for the merge
    struct RejectOut { uint32_t n = 0, accepted = 0, n_requeued = 0; uint8_t *kind = nullptr; const uint32_t *blk_rq = nullptr; const uint64_t *rq_id = nullptr, *rq_prio = nullptr;
                       const uint32_t *rq_rq = nullptr; const uint64_t *d_id = nullptr, *d_prio = nullptr; const uint32_t *d_rq = nullptr; };
    RejectOut reject_out;
    // hqtick_lose_last_tasks / _last_requeued / _last_mn_left: what the last lose() wrote into pinned memory -- the CSR over the n_workers lost workers in the
    // caller's order (the caller settles _REDIRECT in c_kind), the n evicted tasks as one ascending list (f_*), per lost worker the multi-node task it left as a
    // non-root and that task's root (HT_EMPTY: none) -- and the same three columns in device memory (d_*) for the merge
    struct LoseOut { uint32_t n_workers = 0, n = 0; const uint32_t *off = nullptr; const uint64_t *c_id = nullptr, *c_prio = nullptr; const uint32_t *c_rq = nullptr; uint8_t *c_kind = nullptr;
                     const uint64_t *f_id = nullptr, *f_prio = nullptr; const uint32_t *f_rq = nullptr; const uint64_t *mn_task = nullptr; const uint32_t *mn_root = nullptr;
                     const uint64_t *d_id = nullptr, *d_prio = nullptr; const uint32_t *d_rq = nullptr; };
    LoseOut lose_out;

    // ---- the C ABI's operations (arguments validated by the caller)
    int enable(const Env &e, uint32_t n, const uint64_t *id, const uint32_t *wid, const uint32_t *rq, const uint8_t *var, const uint64_t *prio);
    int add(const Env &e, uint32_t n, const uint64_t *id, const uint32_t *wid, const uint32_t *rq, const uint8_t *var, const uint64_t *prio, int running = 0);  // running: the entries' running byte
    int release(const Env &e, uint32_t n, const uint64_t *id);
    // hqtick_cancel_tasks' ledger step: d_id [n] is DEVICE memory (the call's one copy of the ids); the Retracting overrides are host arrays, ids
    // ascending.  The tables end as after release(ids) + unprefill(ids); cancel_out holds the messages and routes; *retr_hit [n_retr] (pinned, valid until the next
    // cancel): the batch position that claimed override k, NONE if the id is not listed.  Returns the number of ids in the messages.
    int cancel(const Env &e, uint32_t n, const uint64_t *d_id, uint32_t n_retr, const uint64_t *retr_id, const uint32_t *retr_wid, const uint32_t **retr_hit);
    // hqtick_finish_tasks' ledger step: d_id / d_reporter [n] are DEVICE memory (the call's one copy of ids and reporting workers); the Retracting
    // overrides are host arrays, ids ascending.  The tables end as after release(the accepted ids, batch order); finish_out holds the kinds; *retr_hit [n_retr]
    // (pinned, valid until the next finish): the batch position that was accepted for override k, NONE if none was.  Returns the number of accepted positions;
    // last_unknown is the number of refused ones.
    int finish(const Env &e, uint32_t n, const uint64_t *d_id, const uint32_t *d_reporter, uint32_t n_retr, const uint64_t *retr_id, const uint32_t *retr_wid, const uint32_t **retr_hit);
    // hqtick_fail_tasks' ledger step: finish() in the passes' fail mode.  The tables end as after release(accepted ids, batch order) +
    // unprefill(accepted ids); fail_out holds the kinds as the ledger sees them (a _WAITING position is accepted here).  Returns the accepted positions.
    int fail_tasks(const Env &e, uint32_t n, const uint64_t *d_id, const uint32_t *d_reporter, uint32_t n_retr, const uint64_t *retr_id, const uint32_t *retr_wid, const uint32_t **retr_hit);
    // hqtick_start_tasks' ledger steps.  start_begin: d_id / d_reporter / d_variant [n] are DEVICE memory (the call's one copy), mask [n] a host
    // array or nullptr (nonzero: a position the caller decides itself; it is uploaded only then), n_host the number of such positions the caller will start through
    // release() + add() -- room for them is made first, so that the table is not rebuilt between the claim pass, which runs here over the whole batch, and the
    // apply passes.  start_segment: the apply pass over [lo, hi) behind one set of counters and one synchronisation; last: the kinds come back with it and
    // start_out is set (the caller writes the kinds of its own positions into start_out.kind afterwards).  An empty range with !last does nothing.
    int start_begin(const Env &e, uint32_t n, const uint64_t *d_id, const uint32_t *d_reporter, const uint8_t *d_variant, const uint8_t *mask, uint32_t n_host);
    int start_segment(const Env &e, uint32_t lo, uint32_t hi, bool last);
    void start_abort(const Env &e, uint32_t lo);  // a start that ends early: the claims of the positions [lo, n) are given back
    // hqtick_reject_tasks' ledger step: the release's passes in their reject mode and the requeue's compaction behind one set of counters and ONE
    // synchronisation.  d_id / d_reporter / d_variant / d_perm [n] are DEVICE memory (the call's one copy; d_perm: the positions by ascending (id, position)),
    // d_rq [n] too, or nullptr with n_retr == 0.  The tables end as after release(_ASSIGNED ids, batch order) + unprefill(_PREFILLED ids); reject_out holds the
    // kinds as the ledger sees them, the blocks and the requeued columns.  reject_ensure makes every buffer first, so that a failed allocation changes nothing.
    int reject_ensure(const Env &e, uint32_t n, uint32_t n_retr);
    int reject(const Env &e, uint32_t n, const uint64_t *d_id, const uint32_t *d_reporter, const uint8_t *d_variant, const uint32_t *d_rq, const uint32_t *d_perm, uint32_t n_retr,
               const uint64_t *retr_id, const uint32_t *retr_wid, const uint32_t **retr_hit);
    bool variant_exists(uint32_t rq, uint32_t v) const { return (size_t)rq + 1 < rq_off.size() && v < rq_off[rq + 1] - rq_off[rq] && v < PF_VARIANT; }
    int running(const Env &e, uint32_t n, const uint64_t *id, uint8_t *run);  // hqtick_assigned_running
    int add_mn(const Env &e, uint32_t n, const uint64_t *id, const uint32_t *rq, const uint64_t *prio, const uint32_t *off, const uint32_t *wid);
    int mn_workers(const Env &e, uint64_t id, uint32_t *n, const uint32_t **wid);
    int lookup(const Env &e, uint32_t n, const uint64_t *id, uint32_t *wid, uint8_t *var);
    int track_prefilled(const Env &e, uint32_t n, const uint64_t *id, const uint32_t *wid, const uint32_t *rq, const uint64_t *prio);
    int start_prefilled(const Env &e, uint32_t n, const uint64_t *id, const uint8_t *var) { return pf_leave(e, n, id, var); }
    int unprefill(const Env &e, uint32_t n, const uint64_t *id) { return pf_leave(e, n, id, nullptr); }
    // ---- the worker set changes (hqtick_cluster_*)
    void take_requests(const hqtick_snapshot *s);  // the request tables of a snapshot, kept when they differ from the ones the ledger has
    int upload_wids(const Env &e);
    int upload_flags(const Env &e);
    int repack(const Env &e, const std::vector<uint32_t> &src, uint32_t W_old, const uint8_t *add_flags);
    int evict(const Env &e, uint32_t n, const uint32_t *worker_id);
    // hqtick_lose_workers' ledger step: evict() with everything behind the count on the device.  One synchronisation, for the count; the sort by
    // id, the gather, the grouping by lost worker and the reset of lost roots' rows are enqueued behind it and NOT waited for -- lose_out's pinned columns are
    // final after the next synchronisation of the stream, which is the row tables' re-pack (repack() below) in the caller's sequence.  The tables end as after
    // evict(); returns the number of evicted entries.  lose_ensure makes every buffer first (sized by the entries the ledger holds), so that a failed allocation
    // changes nothing.
    int lose_ensure(const Env &e, uint32_t n);
    int lose(const Env &e, uint32_t n, const uint32_t *worker_id);
    uint64_t lose_bound() const { return n_live + mn_live + (pf_on ? pf_live : 0); }  // at most this many entries leave
    void clear_requeued() { rq_task.clear(); rq_rq.clear(); rq_prio.clear(); rq_pf_task.clear(); rq_run_task.clear(); }
    // ---- a tick
    void abandon_tick() { pending = false; stage_n = 0; }  // (a tick that was never consumed is abandoned, as its selection is; its staging is never read)
    int sync_mirror(const Env &e);  // free rows, flags and counts back on the host; then agg()
    // the staging of n_rec records for K5b (false: no memory); ordered / L: how insert_staged will find their priorities
    bool stage_for(uint32_t n_rec, bool ordered, uint32_t L, StageCols *c);
    uint32_t *saved_rq(size_t n) { return buf[B_SAVED_RQ].ensure(n * 4 + 16) ? buf[B_SAVED_RQ].as<uint32_t>() : nullptr; }  // the request-id column as it was before K4's tombstones
    // the tick's redirects and multi-node placements (worker ids) and its new_free wait with its staged records; saved: their request ids are in saved_rq()
    void collect_tick(const hqtick_snapshot *s, const hqtick_result *out, const std::vector<uint64_t> &new_free, const std::vector<uint32_t> &mn_rq, bool saved);
    int apply_tick(const Env &e);  // ... and become ledger state
    // what collect_tick() took has something to enter: staged records, redirects, multi-node placements, or free rows that differ from the mirror's (sync_mirror read them for this tick)
    bool tick_enters(const Env &e) const { return stage_n || !red_id.empty() || !pmn_id.empty() || pend_free != *e.free_; }
    // a waiting placement is live only while the tick's selection is (selection: ReadySet::selection_live(): a selection not yet consumed, or an empty one held for its placement)
    bool pending_live(bool selection) { if (pending && !selection) pending = false; return pending; }
    uint32_t max_variants() const { uint32_t m = 0; for (size_t q = 0; q + 1 < rq_off.size(); q++) m = std::max(m, rq_off[q + 1] - rq_off[q]); return m; }
    bool tracking() const { return pf_on; }
    bool dirty() const { return dirty_; }
    const std::vector<uint32_t> &prefilled_host(uint32_t *stride) const { *stride = pf_stride; return h_pf; }  // pf [W x stride] as sync_mirror read it
    Agg agg() const { return Agg{agg_off.data(), agg_rq.data(), agg_cnt.data(), agg_var.data()}; }
    // what the audit (audit.h) reads: the device tables as they are and the host's request tables; false: no table yet
    struct AuditView { Table t; Rows r; MnRows m; const std::vector<uint32_t> *rq_off, *vent_off, *ent_res, *var_nodes; const std::vector<uint8_t> *ent_kind; const std::vector<uint64_t> *ent_amt; };
    bool audit_view(const Env &e, AuditView *v) const {
        if (!cap || !mn.cur.p || !buf[B_WIDS].p) return false;
        *v = AuditView{table(), rows(e), mn_rows(mn.cur, e.W, mn_live), &rq_off, &vent_off, &ent_res, &var_nodes, &ent_kind, &ent_amt};
        return true;
    }
    void release_all();

  private:
    using DevBuf = hqbuf::DevBuf;
    struct TableCols {  // the hash table's columns (assigned.h: Table), `cap` buckets
        DevBuf key, wid, rq, var, prio, claim, run;
        bool ensure(size_t cap) { return key.ensure(cap * 8) && wid.ensure(cap * 4) && rq.ensure(cap * 4) && var.ensure(cap) && prio.ensure(cap * 8) && claim.ensure(cap * 4) && run.ensure(cap); }
        Table view(uint32_t mask) const { return Table{key.as<uint64_t>(), wid.as<uint32_t>(), rq.as<uint32_t>(), var.as<uint8_t>(), prio.as<uint64_t>(), claim.as<uint32_t>(), run.as<uint8_t>(), mask}; }
        void release() { for (DevBuf *b : {&key, &wid, &rq, &var, &prio, &claim, &run}) b->release(); }
    };
    struct RowPair { DevBuf cur, next; void swap() { std::swap(cur, next); } void release() { cur.release(); next.release(); } };  // a per-worker-row table and the target of its next re-pack
    // Columns one behind the other in a buffer that has the room (h: its host side, nullptr for device memory; dv: the same bytes as the device sees them).
    // put() copies a column there (src == nullptr: left as it is) and returns where the device finds it.
    struct Pack {
        unsigned char *h = nullptr, *dv = nullptr; size_t end = 0;
        template <typename T> T *put(const T *src, size_t n, size_t align = 1) {
            end = (end + align - 1) & ~(align - 1);
            if (h && src) memcpy(h + end, src, n * sizeof(T));
            T *p = reinterpret_cast<T *>(dv + end); end += n * sizeof(T); return p;
        }
        template <typename T> T *host(const T *p) const { return reinterpret_cast<T *>(h + (reinterpret_cast<const unsigned char *>(p) - dv)); }
    };
    static uint32_t row_stride(size_t cols) { return std::max<uint32_t>(16, ((uint32_t)cols + 15) & ~15u); }
    int fail(int code, const std::string &m) { err = m; return code; }
    Table table() const { return tab.view(cap - 1); }
    Rows rows(const Env &e) const {
        return Rows{buf[B_WIDS].as<uint32_t>(), e.W, e.R, reinterpret_cast<const uint64_t *>(e.cluster), reinterpret_cast<uint64_t *>(e.cluster + (size_t)e.W * e.R * 8), counts.cur.as<uint32_t>(), stride,
                    pf_on ? pf.cur.as<uint32_t>() : nullptr, pf_on ? pf_stride : 0u};
    }
    // the multi-node columns of W rows in `b`; live: the uniform argument of the kernels that may skip them
    MnRows mn_rows(const DevBuf &b, uint32_t W, uint64_t live) const { return MnRows{b.as<uint64_t>(), b.as<uint8_t>() + (size_t)W * 8, b.as<uint8_t>() + (size_t)W * 9, (uint32_t)std::min<uint64_t>(live, 0xFFFFFFFFu)}; }
    size_t req_bytes() const { return (((rq_off.size() + vent_off.size() + ent_res.size()) * 4 + 7) & ~(size_t)7) + ent_res.size() * 9 + 64; }
    Req req(unsigned char *h = nullptr) const;  // the request tables in buf[B_REQ] (h: packed there as well)
    int stage_in(size_t bytes, Pack *pk) { if (!h_in.ensure(bytes + 16)) return fail(HQTICK_E_DEVICE, "hipHostMalloc ledger staging"); *pk = Pack{h_in.as<unsigned char>(), h_in.dev<unsigned char>()}; return 0; }
    // One operation's counters: zeroed on the stream, `launch` (given the device counters), 32 B copied back behind it, one synchronisation -> c (pinned).
    // c is the LAST operation's: insert_host and mn_enter end with theirs, and their callers read it before anything else runs.
    template <class F> int counted(hipStream_t s, const char *what, F &&launch) {
        if (!h_ctr.ensure(64) || !buf[B_CTR].ensure(64) || hipMemsetAsync(buf[B_CTR].p, 0, 64, s) != hipSuccess) return fail(HQTICK_E_DEVICE, "hipHostMalloc");
        c = h_ctr.as<uint32_t>(); std::fill_n(h_ctr.as<uint32_t>(), (size_t)C_N, 0u);
        hipError_t rc = launch(buf[B_CTR].as<uint32_t>());
        if (rc == hipSuccess) rc = hipMemcpyAsync(h_ctr.p, buf[B_CTR].p, 32, hipMemcpyDeviceToHost, s);
        if (rc == hipSuccess) rc = hipStreamSynchronize(s);
        return rc == hipSuccess ? 0 : fail(HQTICK_E_DEVICE, std::string(what) + ": " + hipGetErrorString(rc));
    }
    int widen(const Env &e, RowPair &t, uint32_t &stride, size_t cols, const char *what);
    int sync_req(const Env &e);
    int reserve(const Env &e, uint64_t more);
    int insert_host(const Env &e, uint32_t n, const uint64_t *id, const uint32_t *wid, const uint32_t *rq, const uint8_t *var, const uint64_t *prio, int upsert, int apply_free, const uint32_t *col_rq,
                    int running = 0);
    int mn_enter(const Env &e, uint32_t n, const uint64_t *id, const uint32_t *rq, const uint64_t *prio, const uint32_t *off, const uint32_t *wid, int check);
    int pf_leave(const Env &e, uint32_t n, const uint64_t *id, const uint8_t *var);
    int reported(const Env &e, bool failing, uint32_t n, const uint64_t *d_id, const uint32_t *d_reporter, uint32_t n_retr, const uint64_t *retr_id, const uint32_t *retr_wid, const uint32_t **retr_hit);  // finish() / fail_tasks()

    TableCols tab, tab2;      // the hash table; the target of a rebuild
    RowPair counts, mn, pf;   // counts u32 [W x stride]; [mn task u64 W][mn root u8 W][flags u8 W]; pf u32 [W x pf_stride]
    // request tables, worker ids in row order, kernel scratch, the request ids before K4, a re-pack's row map, K5b's staging, counters of one operation,
    // a cancel's routes, overrides and sort scratch, a start's positions, kinds and mask (the host steps between its segments use B_SCRATCH)
    // a reject's blocks, records, slice table and requeued columns; a lost-worker call's pairs, columns and sort scratch (lose_core.h: DevLayout)
    enum { B_REQ, B_WIDS, B_SCRATCH, B_SAVED_RQ, B_BATCH, B_STAGE, B_CTR, B_CANCEL, B_START, B_REJECT, B_LOSE, B_N }; DevBuf buf[B_N];
    StartCols start_c{}; uint32_t start_n = 0, start_acc[C_N] = {};  // a start between start_begin and its last segment: its columns, the counters summed over the segments
    hqbuf::PinBuf h_start;  // a start's mask in, its kinds out
    hqbuf::PinBuf h_reject;  // a reject's overrides in; its hits, kinds, blocks, requeued count and columns out
    hqbuf::PinBuf h_lose;    // a lost-worker call's worker lists in; its flat list, CSR and non-root members out (lose_core.h: PinLayout)
    hqbuf::PinBuf h_ctr, h_in, h_cancel, h_finish, h_fail;  // (h_cancel: a cancel's overrides in, its lists and routes out; h_finish / h_fail: a finish's / fail's overrides in, its kinds out)
    const uint32_t *c = nullptr;              // the last operation's counters (h_ctr)
    uint32_t cap = 0; uint64_t n_tomb = 0;    // buckets (a power of two), tombstones
    uint32_t stride = 0; bool flags_dirty = false;  // (flags_dirty: a ledger call changed the flags column since the mirror read it)
    bool pf_on = false; uint32_t pf_stride = 0; std::vector<uint32_t> h_pf; bool pf_dirty = false;  // (pf_dirty: ... the prefilled table since h_pf was read)
    std::vector<uint32_t> var_nodes;          // n_nodes per variant slot of the request tables
    // the request tables of the last snapshot (ResourceRqMap only grows: a slot keeps its number)
    std::vector<uint32_t> rq_off{0}, vent_off{0}, ent_res; std::vector<uint8_t> ent_kind; std::vector<uint64_t> ent_amt; bool req_dirty = true;
    std::vector<uint32_t> h_counts; bool dirty_ = false;  // the device tables changed since the host mirror (free rows, counts) was read
    std::vector<uint32_t> agg_off, agg_rq, agg_cnt; std::vector<uint8_t> agg_var; bool agg_dirty = true;
    // a tick's placement until it is applied
    uint32_t stage_n = 0; bool stage_ordered = false; uint32_t stage_L = 0; StageCols stage_c{};
    bool pend_saved = false; uint32_t pend_W = 0; std::vector<uint64_t> pend_free;
    std::vector<uint64_t> red_id, red_prio; std::vector<uint32_t> red_wid, red_rq; std::vector<uint8_t> red_var;
    std::vector<uint64_t> pmn_id; std::vector<uint32_t> pmn_rq, pmn_off{0}, pmn_wid;  // (worker ids, root first)
    std::vector<uint32_t> mnw_out; std::vector<unsigned char> mnw_cols;              // hqtick_assigned_mn_workers
};

}  // namespace hqasg

// The host side of the resident worker set (hqtick_cluster_*, hqtick_retracting_*, ABI 5 and 7): the layout of the worker / request tables that
// the worker evaluation reads, WorkerSet (the tables in HBM, their staging and their host mirror) and Retracting (the table of Retracting tasks, host only).
// The kernels are kernels.hip's; hqtick.cpp validates the arguments of the C ABI, interleaves the ledger's steps (ledger.h) and forwards.
// Like hqasg::Ledger, a method returns an HQTICK_E_* code (negative) with `err` set and enqueues on the stream it is given.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/hqtick.h"
#include "devbuf.h"
#include "hb_table.h"
#include "kernels.h"

namespace hqcluster {

// Worker tables + request tables in ONE buffer: [total W x R u64][free W x R u64][remaining W i64][entry amount ne u64][variant min time nv u64]
// [variant entry offset nv + 1 u32][entry resource ne u32][entry kind ne u8], 64 bytes of slack.  The request tables start at o_amt.
struct TabLayout { size_t o_tot, o_free, o_rem, o_amt, o_time, o_off, o_res, o_kind, bytes; uint32_t nv, ne; };
TabLayout table_layout(uint32_t W, uint32_t R, uint32_t nv, uint32_t ne);
TabLayout table_layout(const hqtick_snapshot *s, uint32_t W);
void pack_worker_rows(unsigned char *h, const TabLayout &L, uint32_t W, uint32_t R, const uint64_t *total, const uint64_t *free_, const int64_t *rem);
void pack_request_tables(unsigned char *h, const TabLayout &L, const hqtick_snapshot *s);
// the tables at `d` as the worker evaluation takes them
struct UpView { const uint64_t *total, *free_; const int64_t *rem; hqk::RequestTable rt; uint32_t n_entries; };
void view_tables(unsigned char *d, const TabLayout &L, UpView *uv);

class WorkerSet {
  public:
    std::string err;
    int init();      // after the device has been set: the staging event; HQTICK_CHECK_CLUSTER
    void release();
    // ---- what the ledger's Env and the C ABI's readers are given
    bool valid() const { return valid_; }
    uint32_t W() const { return W_; }
    uint32_t R() const { return R_; }
    unsigned char *rows() const { return d_tab.as<unsigned char>(); }
    const std::vector<uint32_t> &ids() const { return id; }
    std::vector<uint8_t> *flags() { return &flags_; }       // (the ledger moves HQ_WORKER_SN bits and free rows: its sync_mirror writes them here)
    std::vector<uint64_t> *free_rows() { return &free_; }
    // ---- the set as a whole
    int upload(hipStream_t st, const hqtick_snapshot *s);  // (validated by the caller)
    void drop() { valid_ = false; clock_mode_ = false; }
    // ---- clock mode (hqtick_cluster_set_clock): the termination times are resident and a tick takes only the clock.  The first call turns every row's remaining
    // lifetime into a deadline at `now_ns`; from then on `rem` and the column in HBM hold the canonical value of clock_core.h, rewritten (complete() on the host,
    // k_clock_rows from tables()) when the clock, a deadline, the membership or the request table's min_time thresholds changed.  upload() and drop() leave the mode.
    int set_clock(int64_t now_ns);
    bool clock_mode() const { return clock_mode_; }
    const std::vector<int64_t> &deadlines() const { return deadline; }
    uint32_t clock_launches() const { return n_clock_launches; }  // k_clock_rows launches of this set so far (test hook)
    // ---- deltas
    int update_rows(hipStream_t st, uint32_t n, const uint32_t *worker_index, const uint64_t *free_rows, const int64_t *remaining_ns);
    // A membership change in three steps, between which hqtick.cpp runs the ledger's: the row map `src` of the new table (old row index, or W + k for the k-th new
    // worker) from the checked arguments; the device step, after which W() is the new count while the mirror still has the old rows; the mirror's step.
    int plan_add(uint32_t n, const uint32_t *worker_id, const uint32_t *group, std::vector<uint32_t> *src);
    int plan_remove(uint32_t n, const uint32_t *worker_id, std::vector<uint32_t> *src);
    int repack(hipStream_t st, const std::vector<uint32_t> &src, uint32_t n_add, const uint64_t *add_total, const uint64_t *add_free, const int64_t *add_rem);
    void add_rows(uint32_t n, const uint32_t *worker_id, const uint64_t *total, const uint64_t *free_rows, const int64_t *rem, const float *min_util, const uint8_t *flags, const uint32_t *group);
    void keep_rows(const std::vector<uint32_t> &src);
    int set_blocked(uint32_t worker_id, uint32_t n, const uint32_t *rq, const uint8_t *variant);
    // one pair of one worker's blocked set (hqtick_reject_tasks, hqtick_cluster_enable_request / _blocked): block() adds it unless it is there (1: added, 0: it was
    // there or the worker is unknown), enable_request() removes it (1 / 0; unknown worker: HQTICK_E_INVALID), blocked_of() reads the set in the order it was added
    int block(uint32_t worker_id, uint32_t rq, uint8_t variant);
    int enable_request(uint32_t worker_id, uint32_t rq, uint8_t variant);
    int blocked_of(uint32_t worker_id, uint32_t *n, const uint32_t **rq, const uint8_t **variant);
    int set_flags(uint32_t n, const uint32_t *worker_id, const uint8_t *flags, bool sn_is_the_ledgers);  // the host part
    // ---- a tick
    // *full = *s; a snapshot without worker arrays gets the worker side and the blocked triples of a valid set
    int complete(const hqtick_snapshot *s, hqtick_snapshot *full);
    // the tables in HBM for the worker evaluation: the request tables of `s` are compared with what was uploaded and re-sent when the snapshot brings new request
    // classes; the worker rows are the caller's responsibility (update_rows), checked against the snapshot's under HQTICK_CHECK_CLUSTER=1
    int tables(hipStream_t st, const hqtick_snapshot *s, uint32_t W, UpView *uv);

  private:
    int fail(int code, const std::string &m) { err = m; return code; }
    int wait();                // the staging buffers are free again: the last copy or kernel that read them is done
    int staged(hipStream_t st);  // ... and are read by what was just enqueued
    // ids -> rows; unknown or repeated ids refused, and whatever `also` (list index, row) refuses of an id that passed
    int rows_of(const char *fn, uint32_t n, const uint32_t *worker_id, std::vector<uint32_t> *row, const std::function<int(uint32_t, uint32_t)> &also = {});

    hqbuf::DevBuf d_tab, d_next;  // the tables; the target of the next re-pack (swapped)
    hqbuf::PinBuf h_tab, h_delta;  // staging of whole tables / of a delta's rows (read in place by its kernel)
    hipEvent_t ev = nullptr; bool pending = false;
    bool valid_ = false, check = false; uint32_t W_ = 0, R_ = 0;
    std::vector<unsigned char> rt;  // host copy of the request-table part as uploaded (compared per tick: a few hundred bytes)
    // the host mirror (ABI 7): what a snapshot without worker arrays is completed from, kept current by the deltas
    uint32_t n_groups = 1;
    std::vector<uint32_t> id, group; std::vector<uint64_t> total, free_; std::vector<int64_t> rem; std::vector<float> min_util; std::vector<uint8_t> flags_;
    // clock mode: the clock, the deadline mirror and its column in HBM, the thresholds as the last tick's request table had them and sorted without duplicates
    bool clock_mode_ = false, dl_dirty = false, rem_dirty = false, kernel_due = false; int64_t now_ = 0; uint32_t n_clock_launches = 0;
    std::vector<int64_t> deadline; hqbuf::DevBuf d_deadline; hqbuf::PinBuf h_deadline;
    std::vector<uint64_t> thr_src, thr;
    std::map<uint32_t, std::vector<std::pair<uint32_t, uint8_t>>> blocked;   // worker id -> (rq, variant)
    // core.worker_map as the reference's map type keeps it: inserts and removals in the order they happened (a removal leaves the table's size and the other
    // workers' buckets as they were, so the iteration order is NOT that of the remaining ids inserted afresh); rank_[row] = position in its iteration order
    hqhb::U32Map wmap_; std::vector<uint32_t> rank_; bool rank_dirty = true;
    std::vector<uint32_t> blk_worker, blk_rq; std::vector<uint8_t> blk_variant; bool blk_dirty = true;  // the same as (worker index, rq, variant) triples
    std::vector<uint32_t> bo_rq; std::vector<uint8_t> bo_variant;  // blocked_of's columns
};

// Tasks a tick or a lost worker made Assigned{redirect target}: the host sends their ComputeTasks messages (hqtick_retract_response, hqtick_cluster_last_reassigned)
struct Reassigned {
    std::vector<uint64_t> task; std::vector<uint32_t> worker; std::vector<uint8_t> variant;
    void clear() { task.clear(); worker.clear(); variant.clear(); }
    void push(uint64_t t, uint32_t w, uint8_t v) { task.push_back(t); worker.push_back(w); variant.push_back(v); }
    void get(uint32_t *n, const uint64_t **t, const uint32_t **w, const uint8_t **v) const {
        if (n) *n = (uint32_t)task.size();
        if (t) *t = task.data();
        if (w) *w = worker.data();
        if (v) *v = variant.data();
    }
};

// The Retracting tasks (ABI 7): task -> (worker id it is retracting from, still in its queue?, redirect target id / variant).  Host logic only, after
// server/reactor.rs and scheduler/mapping.rs; not a part of the worker set (an upload or a drop leaves it as it is).
class Retracting {
  public:
    std::string err;
    Reassigned last;  // what the last response() / workers_removed() reassigned
    uint32_t count() const { return (uint32_t)tab.size(); }
    // every entry, ascending task id, as f(task, in_queue, has_redirect, target worker id, variant): what the audit (audit.h) uploads for its call
    template <class F> void for_each(F &&f) const { for (const auto &kv : tab) f(kv.first, kv.second.in_queue, kv.second.has_redirect, kv.second.target_id, kv.second.variant); }
    void add(uint32_t n, const uint64_t *task_id, const uint32_t *worker_id);  // process_retracted outside a tick: back in their queue
    int response(uint32_t worker_id, uint32_t n, const uint64_t *task_id);     // on_retract_response -> tasks that left the table
    // what response() does for one id, also task_reject's Retracting arm (reactor.rs:412-436; hqtick_reject_tasks): the task leaves the table if it is retracting from
    // `worker_id`; a redirect is appended to `out` (the task is Assigned on the target).  *redirected: whether it had one.  false: not in the table / another worker
    bool take(uint32_t worker_id, uint64_t task_id, Reassigned *out, bool *redirected = nullptr);
    // on_cancel_tasks (reactor.rs:751-761): sources() lists every entry as (task, worker id it is retracting FROM), ascending task id — what hqtick_cancel_tasks hands
    // the ledger as route overrides; cancel() erases one listed task's entry, redirect included (the ledger has released the target's entry: try_remove_redirection)
    void sources(std::vector<uint64_t> *task_id, std::vector<uint32_t> *worker_id) const;
    bool cancel(uint64_t task_id) { return tab.erase(task_id) != 0; }
    // task_finished / task_running of a Retracting task (reactor.rs:547-556, :311-335; hqtick_finish_tasks, hqtick_retracting_started): what the table holds for
    // one task -- the worker id it is retracting FROM, and whether it still sits in its queue.  The entry itself leaves through cancel().
    bool find(uint64_t task_id, uint32_t *old_id, bool *in_queue) const {
        const auto it = tab.find(task_id);
        if (it == tab.end()) return false;
        *old_id = it->second.old_id; *in_queue = it->second.in_queue;
        return true;
    }
    void workers_removed(uint32_t n, const uint32_t *worker_id);               // on_remove_worker (ids in any order: sorted here, and only if the table holds a task)
    // the tasks still in a queue as the retracting arrays of a snapshot whose workers are worker_id[0..W)
    int to_snapshot(const uint32_t *worker_id, uint32_t W, hqtick_snapshot *full);
    // what create_task_mapping did to task states and redirects (mapping.rs:66-101), from the tick's result
    void apply_tick(const uint32_t *worker_id, uint32_t W, const std::vector<uint32_t> &retract_off, const std::vector<uint64_t> &retract_task, const std::vector<uint64_t> &red_task,
                    const std::vector<uint32_t> &red_worker, const std::vector<uint8_t> &red_variant, const std::vector<uint8_t> &red_kind);
    // A two-call tick of a ledger context becomes state at hqtick_ready_consume_last, and the table with it: hold_tick() keeps apply_tick()'s arguments (copies),
    // commit_tick() applies them when the placement enters the ledger, drop_tick() forgets them (the tick was abandoned, or another tick begins)
    void hold_tick(const uint32_t *worker_id, uint32_t W, const std::vector<uint32_t> &retract_off, const std::vector<uint64_t> &retract_task, const std::vector<uint64_t> &red_task,
                   const std::vector<uint32_t> &red_worker, const std::vector<uint8_t> &red_variant, const std::vector<uint8_t> &red_kind) {
        held = Held{std::vector<uint32_t>(worker_id, worker_id + W), retract_off, retract_task, red_task, red_worker, red_variant, red_kind}; has_held = true;
    }
    void commit_tick() {
        if (has_held) apply_tick(held.wid.data(), (uint32_t)held.wid.size(), held.retract_off, held.retract_task, held.red_task, held.red_worker, held.red_variant, held.red_kind);
        drop_tick();
    }
    void drop_tick() { has_held = false; held = Held{}; }

  private:
    struct Held { std::vector<uint32_t> wid, retract_off; std::vector<uint64_t> retract_task, red_task; std::vector<uint32_t> red_worker; std::vector<uint8_t> red_variant, red_kind; };
    Held held; bool has_held = false;
    struct Entry { uint32_t old_id; bool in_queue; bool has_redirect; uint32_t target_id; uint8_t variant; };
    std::map<uint64_t, Entry> tab;
    std::vector<uint64_t> s_task; std::vector<uint32_t> s_worker, s_red_worker; std::vector<uint8_t> s_red_variant;  // to_snapshot's arrays
};

}  // namespace hqcluster

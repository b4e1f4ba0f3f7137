/*
 * hqtick.h — C ABI of the MI355X-native tako scheduling tick (libhqtick.so).
 *
 * This is the drop-in boundary for ONE hot path of It4innovations/hyperqueue: the server-side
 * scheduling tick of the `tako` crate.  The reference has no FFI seam today; the seam this ABI
 * replaces is (all paths relative to /root/reference/crates/tako/src/internal/):
 *
 *   run_scheduling_inner(core, comm, now)            scheduler/main.rs:50-72
 *     = create_task_batches(core, now, None)         scheduler/batches.rs:42-181
 *     + run_scheduling_solver(core, now, batches,..) scheduler/solver.rs:36-483
 *     + create_task_mapping(core, solution)          scheduler/mapping.rs:23-157
 *     + WorkerTaskMapping::send_messages order       scheduler/mapping.rs:259-292
 *   compute_new_worker_query (stages 1-2 only)       scheduler/query.rs:12-131
 *
 * The Rust host (tako) keeps `Core`, `Comm` and the wire layer; it flattens `Core` into the
 * SoA snapshot below, calls hqtick_run(), and applies the returned assignment vector exactly the way
 * create_task_mapping()/send_messages() would (see INTEGRATION.md for the extern "C" binding).
 *
 * Conventions
 *   - plain C, no torch / HIP types in any signature; all pointers are HOST pointers unless the
 *     function name says `_device`.
 *   - amounts are tako `ResourceAmount`: u64 fixed point, 10 000 fractions per unit,
 *     UINT64_MAX = ResourceAmount::MAX ("unknown / unbounded")   common/resources/amount.rs:7,26-31
 *   - task ids are packed `(job_id << 32) | job_task_id` which preserves `TaskId: Ord`  common/ids.rs:17-21
 *   - priorities are the raw `Priority(u64)`                       common/priority.rs:43-47
 *   - one hqtick_ctx per thread; a ctx owns its device buffers, streams and result storage;
 *     no global state; the library never aborts the host: every failure is a negative return code.
 */
#ifndef HQTICK_H
#define HQTICK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: what this header declares is its whole dynamic symbol table. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define HQTICK_ABI_VERSION 12u  /* 12: the assignment ledger, hqtick_assigned_* and hqtick_cluster_last_requeued (hqtick_create still accepts configs written for 10 and 11); 11: hqtick_query_resident (hqtick_create still accepts configs written for 10: the config struct is unchanged); 10: HQTICK_FLAG_NO_TICK_CACHES, hqtick_set_kernel_timing takes any non-zero value but 2 as 1, hqtick_graph_blevel leaves a pending hqtick_ready_consume_last alone; 9: hqtick_graph_blevel / _priorities (extension), hqtick_set_kernel_timing(ctx, 2), a failed CONSUME_IN_TICK tick restores its tasks; 8: HQ_WORKERS_RESIDENT, hqtick_cluster_last_reassigned; 7: hqtick_kernel_stats carries the price-sweep figures of coupled ticks; cluster membership deltas */

/* ResourceAmount::MAX                                    common/resources/amount.rs:31 */
#define HQ_AMOUNT_MAX UINT64_MAX
/* FRACTIONS_PER_UNIT                                     common/resources/amount.rs:7 */
#define HQ_FRACTIONS_PER_UNIT 10000u
/* MAX_TASK_PER_WORKER                                    server/workerload.rs:12 */
#define HQ_MAX_TASK_PER_WORKER 1024u
/* Worker without termination_time                        server/worker.rs:320-326 */
#define HQ_NO_TIME_LIMIT INT64_MAX
/* PriorityCut blocker size == None                       scheduler/batches.rs:15 */
#define HQ_BLOCKER_UNBOUNDED UINT32_MAX
/* "no worker" in records                                 */
#define HQ_NO_WORKER UINT32_MAX

/* AllocationRequest kinds; only Amount-vs-All matters to the tick   common/resources/request.rs:14-21 */
enum { HQ_ENTRY_AMOUNT = 0, HQ_ENTRY_ALL = 1 };

/* worker_flags bits */
enum {
    HQ_WORKER_SN = 1u,       /* WorkerAssignment::Sn (not holding a multi-node task)  server/worker.rs:48-51 */
    HQ_WORKER_STOPPING = 2u  /* stop_reason.is_some()                                 server/worker.rs:312-314 */
};

/* hqtick_run return codes == SchedulerResult              scheduler/main.rs:44-48 */
enum { HQTICK_DONE = 0, HQTICK_NEED_MORE_COMPUTE = 1, HQTICK_NO_PROGRESS = 2 };

/* error codes (negative) */
enum {
    HQTICK_E_INVALID = -1,      /* malformed snapshot (NULL pointer, unsorted ids, bad index)         */
    HQTICK_E_NO_DEVICE = -2,    /* HIP runtime / gfx950 device / kernels not available: NO CPU fallback */
    HQTICK_E_DEVICE = -3,       /* a HIP call failed; hqtick_last_error() has the text                */
    HQTICK_E_CAPACITY = -4,     /* a documented capacity limit was exceeded (levels, groups, ...)     */
    HQTICK_E_QUEUE_UNDERFLOW = -5, /* solver asked for more tasks than a queue holds: the reference
                                      panics here (taskqueue.rs:327 unwrap)                          */
    HQTICK_E_UNSUPPORTED = -6
};

/* assignment record kinds, in the order WorkerTaskMapping::send_messages emits them per worker
 * (prefills first with variant None, then assigned)          scheduler/mapping.rs:268-279 */
enum { HQ_REC_PREFILL = 0, HQ_REC_ASSIGN = 1 };

/* hqtick_config.flags: skip the HIP events that feed hqtick_kernel_stats_last() (saves ~6 API calls per tick) */
#define HQTICK_FLAG_NO_KERNEL_TIMING 1u
/* hqtick_config.flags: compact record emission.  The records of a tick cross PCIe as 4 bytes each (rec_task_lo = job_task_id, the low half of the
 * packed task id) plus one 10-byte RUN per maximal stretch of a worker's records that share (job_id, variant, kind) — instead of 10 bytes per
 * record.  result.rec_task / rec_variant / rec_kind are NULL then; see the run_* fields of hqtick_result.  (Ignored while a device record sink is
 * set: the sink keeps its own layout.) */
#define HQTICK_FLAG_COMPACT_RECORDS 2u
/* hqtick_config.flags, on top of COMPACT_RECORDS (ABI 6): the low halves travel as 16-bit DIFFERENCES.  The records of one (worker, request) come in
 * ascending id order, a few thousand ids apart on a large cluster, so a record that does not open a run is one 16-bit unit — its job_task_id minus its
 * predecessor's — or three units (0xFFFF, low 16 bits, high 16 bits of its job_task_id) when that difference is negative or above 0xFFFE; the record
 * that opens a run has its job_task_id in the run record (hqtick_rec_run16.first_lo).  2 bytes per record instead of 4: the mapping kernel's launch is
 * bound by these bytes crossing PCIe (C3: 25.6 -> ~20 us).  result.rec_task_lo / runs are NULL then; see rec_delta16 / runs16. */
#define HQTICK_FLAG_COMPACT_DELTA16 4u
/* hqtick_config.flags (ABI 8): do not keep class-block answers from tick to tick.  By default a context remembers the last 64 class blocks its HOST solver
 * answered with a certified canonical optimum, keyed by the block's whole model (every coefficient, byte for byte), and answers an identical block from that
 * table: between two ticks of a steady cluster the blocks rarely change while the code that solves them has gone cold.  The answer is the one the solver would
 * give again; kernel_stats.n_classes_memo counts the hits.  bench.py's headline sets this flag (nothing cached inside its timed region). */
#define HQTICK_FLAG_NO_BLOCK_MEMO 8u
/* hqtick_config.flags (ABI 8): hqtick_run_resident takes what it hands out out of the resident ready set ITSELF — as take_tasks / take_tasks_for_prefill / take_one do
 * inside the reference's tick (scheduler/taskqueue.rs:304-373): the selection kernel writes the tombstones while it selects, one kernel and one call per tick less
 * than hqtick_run_resident + hqtick_ready_consume_last (which is a no-op then).  A tick that FAILS after its selection was launched (a record sink too small, a
 * capacity exceeded, a failed exchange) puts back what it took — the group keys its scan left behind tell which tombstones are its own — and the set is as it
 * was before the call; only if that restore itself fails (a device error) does the context drop the resident set (hqtick_last_error says which happened) and the
 * host uploads it again.  Without the flag a tick changes nothing until hqtick_ready_consume_last says so: the two-call form stays the default and is what a
 * drop-in should start from; the flag is for a host whose ticks are short enough for one kernel and one call to matter (bench.py's add -> tick loops). */
#define HQTICK_FLAG_CONSUME_IN_TICK 16u
/* hqtick_config.flags (ABI 9): stop the coupled model's solve where the reference's solver stops — at the certificate.  HiGHS under solve_bounded returns as soon as
 * its incumbent is within mip_rel_gap = 1e-4 of the dual bound (solver/highs.rs:65-88); this library by default goes on to the EXACT optimum and then to the canonical
 * one among the tied optima (result.is_canonical = 1: the answer is a function of the snapshot alone, what parity tier T1 and replicas of a sharded scheduler compare
 * byte for byte).  That proof is most of a small coupled tick (an 80-column model of a few dozen ready tasks: certified after 0.1 ms, canonical after 0.8 ms; a
 * 128-column one: 0.3 ms against 26 ms).  With the flag the tick returns the certified point: is_optimal = 1, is_canonical = 0, the objective within 1e-4 of the
 * optimum exactly as the reference's — for a single scheduler whose ticks must be short.  (Ticks the class blocks or the price sweeps settle are not affected:
 * separable placements stay exact and canonical, swept ones were certificates already.)  IGNORED (ABI 10) on a context that is one of several replicas — after
 * hqtick_set_shard with more than one shard, with a record sink, an exchange callback or a communicator set — whose answers are compared and merged byte for byte. */
#define HQTICK_FLAG_CERTIFICATE_ONLY 32u
/* hqtick_config.flags (ABI 10): nothing DERIVED survives from one tick to the next.  By default a context keeps, next to the resident inputs (ready set, cluster
 * tables), three things it worked out in earlier ticks: the table of host-solved class blocks (NO_BLOCK_MEMO above), the priority-level table of the resident ready
 * set (re-validated by the scan kernel of every tick, rebuilt when a new priority shows up) and the hashbrown iteration orders of the worker-id lists it has seen
 * (Map<WorkerId, _> of scheduler/mapping.rs:36-43, memoised on the whole id list).  All three are pure functions of the tick's inputs, so the results do not change;
 * with this flag every tick works them out again.  For measurements: a loop that repeats one identical tick would otherwise hit all three on every iteration
 * (bench.py's headline sets the flag and says so in its line).  Implies HQTICK_FLAG_NO_BLOCK_MEMO. */
#define HQTICK_FLAG_NO_TICK_CACHES 64u

/* redirect_kind of a result entry (scheduler/mapping.rs:66-101):
 *   FROM_PREFILL  the task sat in a prefill set: Prefilled{old} -> Retracting{old}, retract sent to `old`, redirects.insert(task, (worker, v))
 *   RETARGET      the task was already Retracting{old} in its queue and goes to another worker: redirects.insert(task, (worker, v)); a
 *                 previous target, if any, gets its resources back (remove_sn_task)
 *   SAME_WORKER   the task was Retracting{old} and the tick put it on `old` itself: insert_sn_task(old) only, the redirect table is untouched
 */
enum { HQ_REDIRECT_FROM_PREFILL = 0, HQ_REDIRECT_RETARGET = 1, HQ_REDIRECT_SAME_WORKER = 2 };

/* SchedulerConfig                                           scheduler/state.rs:5-27 */
typedef struct hqtick_config {
    uint32_t abi_version;               /* HQTICK_ABI_VERSION */
    uint32_t proactive_filling_reserve; /* default 16 */
    uint32_t proactive_filling_max;     /* default 40 */
    double mip_time_limit_s;            /* default 5.0 (60.0 under the reference's cfg(test)) */
    int32_t device_index;               /* HIP device ordinal of this ctx */
    uint32_t flags;                     /* HQTICK_FLAG_* */
} hqtick_config;

/*
 * Snapshot of `Core` as the tick reads it.  Caller-owned, read-only during the call.
 *
 * Workers (W): ALL workers of core.worker_map, sorted by ascending WorkerId.  Per-worker resource
 * vectors are padded with zeros to R = n_resources (server/workerload.rs:25-31: missing => 0).
 * Ready set (N): every task sitting in a TaskQueue's `queue` (not its `prefill` set), as SoA,
 * sorted by ascending task id (the order TaskIds are minted in; hqtick_upload_ready() can sort
 * an unsorted set on the device once, outside the tick).
 */
typedef struct hqtick_snapshot {
    /* --- resources ------------------------------------------------------------------------- */
    uint32_t n_resources; /* R = GlobalResourceMapping::n_resources()   common/resources/map.rs:76 */

    /* --- workers --------------------------------------------------------------------------- */
    uint32_t n_workers;                 /* W */
    const uint32_t *worker_id;          /* [W] ascending                                         */
    const uint64_t *worker_total;       /* [W*R] row-major, Worker::resources    server/worker.rs:69 */
    const uint64_t *worker_free;        /* [W*R] SingleNodeTaskAssignment::free_resources   :44  */
    const int64_t *worker_remaining_ns; /* [W] termination_time - now (may be negative) or HQ_NO_TIME_LIMIT */
    const float *worker_min_utilization; /* [W] configuration.min_utilization                   */
    const uint8_t *worker_flags;        /* [W] HQ_WORKER_* bits                                  */
    const uint32_t *worker_group;       /* [W] dense group index in [0, n_groups)  (configuration.group) */
    uint32_t n_groups;
    const uint32_t *worker_map_rank;    /* [W] position of the worker in core.worker_map iteration
                                           (hashbrown order; the Rust shim reads it off `values()`),
                                           or NULL => emulate a map built by inserting ascending ids */

    /* Worker::blocked_requests as (worker index, rq, variant) triples   server/worker.rs:70 */
    uint32_t n_blocked;
    const uint32_t *blocked_worker; /* index into worker arrays */
    const uint32_t *blocked_rq;
    const uint8_t *blocked_variant;

    /* SingleNodeTaskAssignment::assigned_tasks as CSR of (rq, variant) per worker — what
     * GapCache::get_gap subtracts (scheduler/solver.rs:296-303) and what Worker::is_free tests */
    const uint32_t *assigned_off; /* [W+1] */
    const uint32_t *assigned_rq;
    const uint8_t *assigned_variant;

    /* SingleNodeTaskAssignment::prefilled_tasks as CSR of rq per worker (mapping.rs:199-205) */
    const uint32_t *prefilled_off; /* [W+1] */
    const uint32_t *prefilled_rq;

    /* --- resource requests: ResourceRqMap as CSR rq -> variants -> entries ------------------ */
    uint32_t n_requests;              /* Q (= number of TaskQueues, taskqueue.rs:32-35)       */
    const uint32_t *rq_variant_off;   /* [Q+1] into variant_* arrays                           */
    const uint32_t *variant_entry_off; /* [NV+1] into entry_* arrays; entries sorted by resource id */
    const uint32_t *variant_n_nodes;  /* [NV] 0 = single node                                  */
    const uint64_t *variant_min_time_ns; /* [NV]                                                */
    const uint32_t *variant_weight;   /* [NV] ResourceWeight(u32), 10 000 = 1.0                */
    const uint32_t *entry_resource;   /* [NE] */
    const uint8_t *entry_kind;        /* [NE] HQ_ENTRY_* */
    const uint64_t *entry_amount;     /* [NE] (ignored for HQ_ENTRY_ALL) */

    /* --- ready set SoA (TaskQueue::queue of every rq, flattened) ----------------------------- */
    uint64_t n_ready;            /* N */
    const uint64_t *task_id;     /* [N] ascending */
    const uint64_t *task_priority; /* [N] */
    const uint32_t *task_rq;     /* [N] */

    /* --- TaskQueue::prefill of every rq (taskqueue.rs:118) ------------------------------------ */
    const uint32_t *prefill_off;     /* [Q+1] */
    const uint64_t *prefill_priority; /* [Q] valid when the rq's prefill set is non-empty        */
    const uint64_t *prefill_task;    /* ids in the Set<TaskId>'s iteration order                  */
    const uint32_t *prefill_worker;  /* worker INDEX holding the prefilled task                   */

    /* --- ready tasks in state Retracting{worker}: put back into their queue when a higher-priority arrival dissolved the
     * prefill set (check_dispose_prefill, scheduler/taskqueue.rs:148-154).  They are ordinary members of the ready set (they appear in
     * the task_* columns / the resident set), but create_task_mapping treats them differently (scheduler/mapping.rs:66-80): no
     * `assigned` record, a redirect instead.  Ascending task id. */
    uint32_t n_retracting;
    const uint64_t *retracting_task;
    const uint32_t *retracting_worker;           /* worker INDEX the task is being retracted from                         */
    const uint32_t *retracting_redirect_worker;  /* current scheduler_state.redirects target (worker INDEX) or HQ_NO_WORKER */
    const uint8_t *retracting_redirect_variant;  /* its variant (ignored when there is no redirect)                       */
} hqtick_snapshot;

/* What-if query input: fake workers appended after the real ones (scheduler/query.rs:20-56).
 * Same layout as the worker arrays above; ids must be above every real id. */
typedef struct hqtick_query_workers {
    uint32_t n_workers;
    const uint32_t *worker_id;
    const uint64_t *worker_total; /* [n*R]; free == total for a fresh fake worker */
    const int64_t *worker_remaining_ns;
    const float *worker_min_utilization;
} hqtick_query_workers;

/* Compact emission (HQTICK_FLAG_COMPACT_RECORDS): one run = a maximal stretch of a worker's records that share (job id, variant, kind) */
typedef struct hqtick_rec_run {
    uint32_t first; /* index of the run's first record inside its worker's range */
    uint32_t job;   /* high 32 bits of the task ids of the run (the job id of HyperQueue's TaskId packing) */
    uint32_t meta;  /* variant | kind << 8 (low 16 bits; the rest is zero) */
} hqtick_rec_run;
typedef struct hqtick_run_span { uint32_t start, count; } hqtick_run_span;
/* HQTICK_FLAG_COMPACT_DELTA16: the run record also carries the low half of its first record's task id */
typedef struct hqtick_rec_run16 { uint32_t first, job, meta, first_lo; } hqtick_rec_run16;

/*
 * Result view.  All pointers are owned by the ctx and stay valid until the next call on it.
 */
typedef struct hqtick_result {
    int32_t status;     /* HQTICK_DONE / NEED_MORE_COMPUTE / NO_PROGRESS */
    uint8_t is_optimal; /* SchedulingSolution::is_optimal  scheduler/solver.rs:14-16 — with the reference's meaning: solve_bounded sets only
                           `time_limit` (solver/highs.rs:65-68), so HiGHS reports Optimal once the incumbent is within its default
                           mip_rel_gap = 1e-4 of the dual bound.  1 here = certified within that same 1e-4 (or proven exact). */
    uint8_t is_canonical; /* 1: the placement is the EXACT optimum and, among the optimal placements, the canonical one — the answer
                             is a function of the snapshot alone.  0: certified-optimal (or an incumbent) but the exact pass / the tie-break phase
                             was skipped or ran out of its work budget: only the objective value can be compared with another solver's answer.
                             (ABI 3; uses former padding.) */

    /* TaskBatch list (scheduler/batches.rs:18-27) — exposed so parity tier T1 is testable */
    uint32_t n_batches;
    const uint32_t *batch_rq;
    const uint32_t *batch_size;
    const uint32_t *batch_limit;
    const uint8_t *batch_limit_reached;
    const uint8_t *batch_is_blocker;
    const uint32_t *batch_cut_off;     /* [n_batches+1] */
    const uint32_t *cut_size;          /* [n_cuts] */
    const uint32_t *cut_blocker_off;   /* [n_cuts+1] */
    const uint32_t *blocker_rq;
    const uint32_t *blocker_size;      /* HQ_BLOCKER_UNBOUNDED = None */

    /* SchedulingSolution::sn_counts (solver.rs:12) flattened in the reference's iteration order:
     * outer = sn_counts.into_iter() order, inner = counts.iter() order (mapping.rs:36,43) */
    uint32_t n_counts;
    const uint32_t *count_rq;
    const uint8_t *count_variant;
    const uint32_t *count_worker; /* worker INDEX */
    const uint32_t *count_value;

    /* WorkerTaskMapping (mapping.rs:11-21) as CSR over worker index.  Per worker the records are in
     * the exact order send_messages() walks them: prefills, then assigned sorted by priority desc
     * (stable).  Retracts are a separate CSR (they are sent first, as one RetractTasks message). */
    const uint32_t *rec_off;    /* [W+1] */
    const uint64_t *rec_task;
    const uint8_t *rec_variant; /* 0xFF for prefills (variant None) */
    const uint8_t *rec_kind;    /* HQ_REC_* */
    const uint32_t *retract_off; /* [W+1] */
    const uint64_t *retract_task;
    /* Compact emission (HQTICK_FLAG_COMPACT_RECORDS; NULL otherwise).  Worker w's records are rec_off[w] .. rec_off[w + 1] as before; record i of
     * that range has task id (run.job << 32) | rec_task_lo[rec_off[w] + i], variant run.meta & 0xFF (0xFF = None: a prefill) and kind run.meta >> 8,
     * where `run` is the one of runs[run_span[w].start .. + run_span[w].count) with the largest run.first <= i (runs ascend by `first`; the first one
     * starts at 0).  run_span is defined only for workers with records; a worker's runs sit in the run slots of its own records (run_span[w].start ==
     * rec_off[w]: at most one run per record, so no allocation is needed on the device).  (ABI 5: the runs are 12-byte records and the span one 8-byte pair — every
     * store of the mapping kernel crosses PCIe as a write of its own, and three arrays of 4 + 4 + 2 bytes per run cost a third of the launch.) */
    const uint32_t *rec_task_lo;        /* [n_records] */
    const struct hqtick_run_span *run_span; /* [W] */
    const struct hqtick_rec_run *runs;
    /* HQTICK_FLAG_COMPACT_DELTA16 (ABI 6; NULL otherwise, and rec_task_lo / runs are NULL then).  run_span as above, indexing runs16.  Worker w's unit
     * stream starts at rec_delta16[4 * rec_off[w]] (at most 3 units per record; the slack keeps every stream 8-byte aligned).  Decoding the records of w
     * in order: a record that opens a run (i == run.first) has job_task_id = run.first_lo and consumes no unit; any other record reads one unit u:
     * u != 0xFFFF -> job_task_id = previous job_task_id + u;  u == 0xFFFF -> job_task_id = next unit | next-but-one unit << 16 (three units consumed). */
    const uint16_t *rec_delta16;
    const struct hqtick_rec_run16 *runs16;

    /* scheduler_state.redirects insertions made by this tick (mapping.rs:78-100) */
    uint32_t n_redirects;
    const uint64_t *redirect_task;
    const uint32_t *redirect_worker; /* worker INDEX of the new target */
    const uint8_t *redirect_variant;
    const uint8_t *redirect_kind;    /* HQ_REDIRECT_* */

    /* multi-node placements (solver.rs:442-464, mapping.rs:133-154): task + its workers, root first */
    uint32_t n_mn;
    const uint64_t *mn_task;
    const uint32_t *mn_worker_off; /* [n_mn+1] */
    const uint32_t *mn_worker;     /* worker INDEX */

    /* free resources of every worker after the tick (Worker::insert_sn_task, server/worker.rs:188-196) */
    const uint64_t *new_free; /* [W*R] */

    /* timing of the last call, microseconds (host wall clock around each stage) */
    double t_total_us, t_scan_us, t_batches_us, t_solve_us, t_mapping_us;
} hqtick_result;

/* compute_new_worker_query result: for every fake worker, 1 if it received any count
 * (query.rs:73-95), plus the batches for inspection */
typedef struct hqtick_query_result {
    uint32_t n_workers;
    const uint8_t *is_loaded; /* [n_workers] */
    uint8_t is_optimal;
} hqtick_query_result;

typedef struct hqtick_ctx hqtick_ctx;

/* Create a context bound to one HIP device.  Fails with HQTICK_E_NO_DEVICE when no gfx950
 * device / runtime is usable — there is deliberately no CPU implementation behind this ABI. */
int hqtick_create(const hqtick_config *config, hqtick_ctx **out_ctx);
void hqtick_destroy(hqtick_ctx *ctx);

/* One scheduling tick == run_scheduling_inner().  Copies the snapshot's columns to the device,
 * runs the tick, fills `out`.  Returns HQTICK_DONE/NEED_MORE_COMPUTE/NO_PROGRESS or a negative error. */
int hqtick_run(hqtick_ctx *ctx, const hqtick_snapshot *snapshot, hqtick_result *out);

/* Device-resident variant: keep the ready-set columns in HBM across ticks.
 * hqtick_upload_ready() copies (and, when `sorted`==0, sorts by task id on the device: bitonic, once per upload) the ready
 * set into ctx-owned HBM buffers; hqtick_run_resident() then runs ticks against them, taking every
 * other field (workers, requests, prefill sets) from `snapshot` and ignoring its task_* pointers. */
int hqtick_upload_ready(hqtick_ctx *ctx, uint64_t n_ready, const uint64_t *task_id,
                        const uint64_t *task_priority, const uint32_t *task_rq, int sorted);
int hqtick_run_resident(hqtick_ctx *ctx, const hqtick_snapshot *snapshot, hqtick_result *out);

/*
 * Resident ready-set deltas: what the reactor's event handlers do to TaskQueues between two ticks, applied to
 * the HBM-resident columns instead of re-uploading them.
 *   hqtick_ready_consume_last  every task the last hqtick_run_resident handed out (assigned, newly prefilled, multi-node)
 *                              leaves the set — take_tasks / take_tasks_for_prefill / take_one   scheduler/taskqueue.rs:304-373
 *   hqtick_ready_remove        ids (any order) leave the set — TaskQueue::remove on cancel        scheduler/taskqueue.rs:146-217
 *                              returns how many of them were present
 *   hqtick_ready_add           new ready tasks, ids strictly ascending — TaskQueues::add_ready_task scheduler/taskqueue.rs:37-43
 *   hqtick_ready_add_stage /   the same without a copy on the host (ABI 6): _stage hands out the three columns of the library's pinned staging buffer for
 *   hqtick_ready_add_staged    n tasks (valid until the next ready_add* call), the reactor writes the new tasks there, _staged(n' <= n) merges the first n'
 *   hqtick_ready_compact       drop the tombstones now (done automatically when they outnumber the live tasks, and by every add that merges)
 *   hqtick_ready_count         live tasks in the set
 * Removal writes a tombstone into the rq column (4 B per task).  An add whose first id lies behind every resident id (freshly minted ids: the usual batch) and
 * that finds room behind the columns is APPENDED there by one kernel, which also validates it (ABI 8; hqtick_kernel_stats.ready_appends counts); any other add, and
 * compact, stream the columns once (20 B read + 20 B written per live task) through a merge kernel and leave room for as many tasks again.  A refused batch
 * (ids not ascending, an id already resident, a reserved request id) leaves the set as it was.  Request id 0xFFFFFFFF is reserved for the tombstone.
 */
int hqtick_ready_consume_last(hqtick_ctx *ctx);
int hqtick_ready_remove(hqtick_ctx *ctx, uint64_t n, const uint64_t *task_id);
int hqtick_ready_add(hqtick_ctx *ctx, uint64_t n, const uint64_t *task_id, const uint64_t *task_priority, const uint32_t *task_rq);
int hqtick_ready_add_stage(hqtick_ctx *ctx, uint64_t n, uint64_t **task_id, uint64_t **task_priority, uint32_t **task_rq);
/* The same delta in the form a batch of newly ready tasks has anyway (ABI 8): 2-6 bytes per task over PCIe instead of 20 — at 188 k arrivals per tick the
 * transfer is what hqtick_ready_add costs (3.8 MB: ~70 us of a 134 us call).
 *   ids         n_id_runs runs of ascending ids: run r starts at id_run_start[r] and holds id_run_len[r] tasks; id_off[j] (u32, per task, in batch order) is the task's
 *               offset from its run's start — or id_off = NULL: the ids of a run are consecutive (a submit's array, a finished wave of one job).  The batch as a
 *               whole must ascend strictly, like hqtick_ready_add's.
 *   priorities  n_prio_runs runs over the same batch order: prio_run_value[r] for the next prio_run_len[r] tasks
 *   requests    task_rq u16 per task (request ids >= 65535: use hqtick_ready_add)
 * Expanded on the device into the columns hqtick_ready_add would have sent; everything else (merge, validation, errors) is hqtick_ready_add's. */
int hqtick_ready_add_packed(hqtick_ctx *ctx, uint64_t n, uint32_t n_id_runs, const uint64_t *id_run_start, const uint32_t *id_run_len, const uint32_t *id_off,
                            uint32_t n_prio_runs, const uint64_t *prio_run_value, const uint32_t *prio_run_len, const uint16_t *task_rq);
int hqtick_ready_add_staged(hqtick_ctx *ctx, uint64_t n);
int hqtick_ready_compact(hqtick_ctx *ctx);
uint64_t hqtick_ready_count(const hqtick_ctx *ctx);

/*
 * Cluster tables resident in HBM (ABI 5): the worker rows (total, free, remaining lifetime) and the request tables K2 reads every
 * tick stay on the device, and the reactor sends what its event handlers change instead of the library re-packing W rows per tick:
 *   hqtick_cluster_upload          the snapshot's worker_total / worker_free / worker_remaining_ns and request tables -> HBM.  Again whenever
 *                                  workers join or leave (on_new_worker / on_remove_worker, server/reactor.rs:20-186: the row count changes).
 *   hqtick_cluster_update_workers  n rows whose free resources (and, with remaining_ns != NULL, remaining lifetime) changed since the last call —
 *                                  tasks started (the previous tick's assignments, Worker::insert_sn_task) or finished (on_task_finished),
 *                                  time limits running down.  worker_index[n] are row numbers of the uploaded set, free_rows[n * n_resources].
 *                                  Applied in stream order before the next tick; returns without synchronising.
 *   hqtick_cluster_drop            back to per-tick packing.
 * While the tables are resident, hqtick_run / hqtick_run_resident read the worker rows from HBM (the snapshot's worker arrays still feed the host-side
 * model build and MUST hold the same values: the caller owns that invariant; HQTICK_CHECK_CLUSTER=1 in the environment makes every tick verify it and
 * fail with HQTICK_E_INVALID).  New request classes in a snapshot are detected and re-sent by the tick itself (a few hundred bytes).  A snapshot with
 * another n_workers / n_resources than the uploaded set is refused (HQTICK_E_INVALID).
 */
int hqtick_cluster_upload(hqtick_ctx *ctx, const hqtick_snapshot *snapshot);
int hqtick_cluster_update_workers(hqtick_ctx *ctx, uint32_t n, const uint32_t *worker_index, const uint64_t *free_rows, const int64_t *remaining_ns);
int hqtick_cluster_drop(hqtick_ctx *ctx);
/*
 * Cluster MEMBERSHIP and blocked requests as deltas (ABI 7): the worker set itself lives in the library between ticks — rows in HBM for the scans, a
 * mirror in host memory for the host stages — and the reactor forwards what its handlers do:
 *   hqtick_cluster_add_workers     on_new_worker  server/reactor.rs:20-32 (Core::new_worker): n workers with ids ascending and above every id present
 *                                  (WorkerIds are minted ascending), their total / free rows [n * R], and (NULL = the defaults of a fresh single-node
 *                                  worker) remaining lifetime, min_utilization, HQ_WORKER_* flags, group.  They take the row indices W .. W + n - 1.
 *   hqtick_cluster_remove_workers  on_remove_worker  server/reactor.rs:64-186: the rows of these ids leave; later rows move up (the row index of a
 *                                  worker is its position in ascending id order, as in a snapshot).  Unknown ids are an error (HQTICK_E_INVALID).
 *   hqtick_cluster_set_blocked     Worker::blocked_requests  server/worker.rs:70 of ONE worker, replaced by the n given (rq, variant) pairs:
 *                                  task_reject adds a pair (reactor.rs:365-445), EnableRequest removes it (request_enabled, reactor.rs:447-460),
 *                                  n = 0 clears.
 *   hqtick_cluster_workers         the current ids in row order (valid until the next membership call).
 *   hqtick_cluster_set_flags       the HQ_WORKER_SN and HQ_WORKER_STOPPING bits of the listed resident workers, replaced: Worker::set_stop
 *                                  (server/worker.rs:312-314) and, for a host without the assignment ledger, set_mn_task / reset_mn_task (:160-175).
 *                                  Unknown ids, an id listed twice or a bit outside the two defined ones are HQTICK_E_INVALID and change nothing.  With the
 *                                  assignment ledger on the SN bit belongs to the ledger (it follows the multi-node tasks): a call that would change a
 *                                  worker's SN bit is HQTICK_E_INVALID; STOPPING may still change.  Refused while a placement waits for its consume, like the
 *                                  other membership calls.  Works on sharded and replica contexts: every replica receives the same call.
 *   hqtick_cluster_worker_flags    the flags in row order (valid until the next call on the context).
 * One re-pack kernel per membership call (rows read from HBM, new rows from pinned staging); nothing is re-uploaded.
 * A tick whose snapshot has worker_id == NULL takes the WHOLE worker side from the library: ids, total / free rows (as kept current by
 * hqtick_cluster_update_workers), remaining lifetime, min_utilization, flags, groups and the blocked pairs.  Say so with n_workers = HQ_WORKERS_RESIDENT: such a
 * tick FAILS (HQTICK_E_INVALID) when the library holds no worker set (never uploaded, or hqtick_cluster_drop) instead of running as a legitimate tick of
 * zero workers, which is what n_workers = 0 with NULL arrays means without a resident set (with one, 0 and the current count are accepted as before).
 * worker_map_rank is emulated (the map is filled in id order at hqtick_cluster_upload and then follows hqtick_cluster_add_workers / _remove_workers as
 * core.worker_map follows on_new_worker / on_remove_worker: a removal leaves the map's size and the other workers' places as they were), and the per-worker CSRs assigned_off / prefilled_off (if given) must have current-count + 1 entries.  The reactor then
 * no longer flattens W x R worker arrays per tick.
 */
int hqtick_cluster_add_workers(hqtick_ctx *ctx, uint32_t n, const uint32_t *worker_id, const uint64_t *total_rows, const uint64_t *free_rows,
                               const int64_t *remaining_ns, const float *min_utilization, const uint8_t *flags, const uint32_t *group);
int hqtick_cluster_remove_workers(hqtick_ctx *ctx, uint32_t n, const uint32_t *worker_id);
int hqtick_cluster_set_blocked(hqtick_ctx *ctx, uint32_t worker_id, uint32_t n, const uint32_t *rq, const uint8_t *variant);
int hqtick_cluster_workers(const hqtick_ctx *ctx, uint32_t *n_workers, const uint32_t **worker_id);
int hqtick_cluster_set_flags(hqtick_ctx *ctx, uint32_t n, const uint32_t *worker_id, const uint8_t *flags);
int hqtick_cluster_worker_flags(const hqtick_ctx *ctx, uint32_t *n_workers, const uint8_t **flags);
/*
 * Workers with a time limit: CLOCK MODE (functions added under ABI 12).  worker_remaining_ns is termination time - now: it changes on every tick for every such
 * worker, and workers that connected microseconds apart never have equal rows.  Instead the library keeps each worker's termination time and is told the time:
 *   hqtick_cluster_set_clock       the clock of the resident worker set (any int64 nanosecond count; it may move in either direction).  The FIRST call switches
 *                                  the set to clock mode: every row gets the deadline now_ns + its remaining lifetime (saturating; HQ_NO_TIME_LIMIT stays), so a
 *                                  host that uploaded lifetimes taken at now_ns loses nothing.  Needs a resident worker set (HQTICK_E_INVALID); refused while a
 *                                  placement waits for its consume, like the other cluster calls; HQTICK_E_UNSUPPORTED on sharded and replica contexts.
 *   hqtick_cluster_deadlines       the termination times in row order (valid until the next call on the context); HQTICK_E_INVALID outside clock mode.
 *   hqtick_cluster_last_row_groups test accessor: the groups of equal worker rows the host stages of the last tick found.
 * In clock mode the other calls keep their meaning relative to the clock: remaining_ns of hqtick_cluster_add_workers and of hqtick_cluster_update_workers
 * (a correction) is the remaining lifetime at the current clock and sets the row's deadline to clock + remaining_ns.  hqtick_cluster_upload and
 * hqtick_cluster_drop leave clock mode, like everything else about a worker set.  A tick runs on the resident worker set (n_workers = HQ_WORKERS_RESIDENT,
 * worker_id = NULL); a snapshot that brings worker arrays is HQTICK_E_INVALID (the tick must not see two truths).
 * What a tick reads as a worker's remaining lifetime is then CANONICAL: HQ_NO_TIME_LIMIT without a limit, -1 past the deadline, else the largest
 * variant_min_time_ns of the snapshot's request table that deadline - clock still covers (0 if none).  Every variant's time test answers as for the true value,
 * and workers that pass the same tests are equal rows whatever their exact deadlines.  One small kernel (k_clock_rows) rewrites the column in HBM, and only when
 * the clock, a deadline, the membership or the request table changed since its last run; nothing is uploaded per tick.  A context that never sets the clock
 * launches nothing new.
 */
int hqtick_cluster_set_clock(hqtick_ctx *ctx, int64_t now_ns);
int hqtick_cluster_deadlines(const hqtick_ctx *ctx, uint32_t *n_workers, const int64_t **deadline_ns);
uint32_t hqtick_cluster_last_row_groups(const hqtick_ctx *ctx);
/*
 * Retracting tasks as deltas (ABI 7; on_retract_response, process_retracted — server/reactor.rs:34-62,462-508).  The table of tasks in state
 * Retracting{worker} — with their scheduler_state.redirects entry — can live in the library instead of travelling in every snapshot:
 *   hqtick_retracting_add      process_retracted outside a tick: a higher-priority arrival dissolved a prefill set (check_dispose_prefill,
 *                              scheduler/taskqueue.rs:148-154) and these tasks went back into their queue as Retracting{worker}.  worker = worker id.
 *   (the tick itself)          a tick run with snapshot->n_retracting == HQ_RETRACTING_RESIDENT takes the in-queue entries of the table as its
 *                              retracting_* arrays (worker ids -> row indices of the resident worker set: needs hqtick_cluster_upload) and, when it
 *                              succeeds, applies to the table what create_task_mapping does to task states and redirects (scheduler/mapping.rs:66-101):
 *                              a prefilled task it hands to another worker enters as Retracting{old} with a redirect, a Retracting task it takes gets its
 *                              redirect (re)targeted, or none when it lands on the worker it is retracting from.
 *   hqtick_retract_response    on_retract_response for one worker: every listed task that is Retracting{that worker} leaves the table — with a redirect
 *                              it is now Assigned to the target (reported in the three output arrays, valid until the next call: the host sends the
 *                              ComputeTasks message), without one it is an ordinary Waiting task of its queue again.  Other ids are ignored, as in the
 *                              reference ("retracted task in invalid state").  Returns the number of tasks that left the table.
 *   hqtick_retracting_count    entries in the table.
 * hqtick_cluster_remove_workers applies on_remove_worker (server/reactor.rs:86-147) to the table: an entry whose OLD worker is removed leaves it — with a
 * redirect to a worker that stays the task is Assigned{target} from now on and the host owes the target its ComputeTasks message: those (task, target id,
 * variant) triples are read with hqtick_cluster_last_reassigned (valid until the next hqtick_cluster_remove_workers / hqtick_retract_response call); without
 * one it is an ordinary Waiting task of its queue.  An entry whose redirect TARGET is removed loses the redirect and is in its queue again, still
 * Retracting{old} (redirects.remove + add_ready_task): the host re-adds the task to the resident ready set (hqtick_ready_add) with the lost worker's other tasks.
 */
#define HQ_RETRACTING_RESIDENT 0xFFFFFFFFu
/* hqtick_snapshot.n_workers of a tick whose worker side is the library's resident worker set (worker_id == NULL) */
#define HQ_WORKERS_RESIDENT 0xFFFFFFFFu
int hqtick_retracting_add(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id);
int hqtick_retract_response(hqtick_ctx *ctx, uint32_t worker_id, uint32_t n, const uint64_t *task_id, uint32_t *n_assigned, const uint64_t **assigned_task,
                            const uint32_t **assigned_worker_id, const uint8_t **assigned_variant);
uint32_t hqtick_retracting_count(const hqtick_ctx *ctx);
int hqtick_cluster_last_reassigned(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id, const uint32_t **worker_id, const uint8_t **variant);

/*
 * Assignment ledger (ABI 12): each worker's SingleNodeTaskAssignment (server/worker.rs:40-46) — its assigned / running single-node tasks
 * and its free_resources — kept by the library on the resident worker set, so that the host no longer sends free rows for task starts and finishes
 * (hqtick_cluster_update_workers) nor flattens the assigned CSR every tick.  OFF unless enabled; with it off every call behaves as in ABI 11.
 *   hqtick_assigned_enable     seed: n tasks (ids, worker ids, rq, variant, priority) in state Assigned / Running, or Retracting and counted on their redirect
 *                              target (worker.rs:249-252).  Needs a resident worker set (hqtick_cluster_upload), whose free rows already account for
 *                              these tasks: the seed does not change them.  n = 0: an empty ledger.  A second call replaces the ledger.
 *                              hqtick_cluster_upload (a new worker set) and hqtick_cluster_drop switch it off; hqtick_assigned_disable drops it.
 *   hqtick_assigned_add        tasks that start outside a tick (task_from_prefilled_to_started, worker.rs:212-221; a Retracting task that starts on the
 *                              worker it was retracting from, reactor.rs:296-333): insert + free.remove (AMOUNT subtracts with saturation, ALL sets 0,
 *                              workerload.rs:156-166).  rq and priority come from the caller.  Returns the number entered; ids already in the ledger and
 *                              entries naming an unknown worker / request / variant are counted (hqtick_assigned_last_unknown) and change nothing.
 *   hqtick_assigned_release    tasks that finished, failed, were cancelled or rejected while Assigned, or a Retracting task's redirect target after
 *                              try_remove_redirection: remove_sn_task (worker.rs:223-234), free.add — AMOUNT adds, ALL sets the resource back to the
 *                              worker's TOTAL (workerload.rs:194-202).  The batch is applied IN ITS ORDER: on one worker "A (AMOUNT), then B (ALL)" leaves
 *                              the total, "B, then A" the total + amount(A).  Unknown ids and repeats of an id within the batch are counted
 *                              (hqtick_assigned_last_unknown) and change nothing (the reference's tolerance of stale task updates).  Returns the number released.
 *   hqtick_assigned_count      entries in the ledger.
 *   hqtick_assigned_lookup     per id the worker id holding it (HQ_NO_WORKER: not in the ledger) and its variant (0xFF then).  Returns the number found.
 *   hqtick_assigned_free_rows  the resident worker set's free rows [W x R] as the ledger keeps them (valid until the next call on ctx).
 *   hqtick_cluster_last_requeued  the tasks the last hqtick_cluster_remove_workers took out of the ledger (on_remove_worker, reactor.rs:64-147) and put
 *                              back into the resident ready set with their priority and request (add_ready_task), ascending ids — if the context holds
 *                              one (hqtick_upload_ready); without it they are only reported and the host puts them wherever its queues are.  The merge
 *                              comes after the membership change: if it fails, the worker is gone and the tasks are out of the ledger, and the host
 *                              re-adds the reported tasks itself (hqtick_ready_add).  The host still owes
 *                              their instance-id bumps, crash counters (a task over its limit leaves with hqtick_ready_remove), prefill disposal and client
 *                              events; it no longer re-adds them.  A Retracting task whose redirect target was lost is among them (the Retracting table drops
 *                              the redirect, as before).  The lost worker's PREFILLED tasks are the host's to re-add unless prefilled tracking is on
 *                              (hqtick_assigned_track_prefilled below): then they are among the reported tasks.
 * The tick: with the ledger on, a tick runs on the resident worker set (n_workers = HQ_WORKERS_RESIDENT, worker_id = NULL) and assigned_off = NULL; it takes
 * the per-worker (rq, variant) counts and the free rows from the ledger.  An assigned CSR in the snapshot is HQTICK_E_INVALID (the tick must not see two
 * truths).  The tick's placement — its ASSIGN records and its redirects (FROM_PREFILL / SAME_WORKER insert on the target, RETARGET moves the task from its
 * old target) with the free rows of result.new_free — enters the ledger when it becomes state: at hqtick_ready_consume_last in the two-call form, inside the
 * tick under HQTICK_FLAG_CONSUME_IN_TICK (a tick that fails leaves ledger and free rows as they were), at once after hqtick_run.  Until a pending placement
 * is consumed, ledger and membership calls are HQTICK_E_INVALID; a tick that is not consumed (any ready-set or graph delta, another tick) is abandoned with
 * its selection and never enters.  A placement is pending whenever it has something to enter -- records, redirects, multi-node placements or a free row that
 * changed -- also when the tick handed out no ready task at all (its only output the redirect of a prefilled task to a worker with room): that tick, too, waits
 * for hqtick_ready_consume_last, which then enters it without replaying a selection, and a delta abandons it like any other.  A two-call tick that has nothing
 * to enter leaves nothing pending.  With a resident Retracting table (HQ_RETRACTING_RESIDENT) what the tick did to Retracting tasks becomes state at the same
 * moment as the placement, so an abandoned tick leaves the table, too, as it was; hqtick_retracting_add and hqtick_retract_response are refused in between
 * like the ledger calls.  A resident ready set that holds only tombstones is the empty set: the tick
 * runs (it may still redirect prefilled tasks).  If entering the placement itself fails (a device allocation), the ledger is switched off and the call says so: the
 * tasks have left the ready set, so the host uploads the worker set and enables the ledger again from its own view.
 * Remaining lifetimes: hqtick_cluster_update_workers needs the free rows of every row it lists, which a ledger host no longer holds, so time limits running
 * down go through the clock instead (hqtick_cluster_set_clock above: 8 bytes per tick, no rows).  hqtick_cluster_update_workers remains for corrections by a host
 * that does hold the rows.
 * Prefilled tasks (SingleNodeTaskAssignment::prefilled_tasks, server/worker.rs:40-46) are the ledger's too once tracking is switched on; with it off
 * every call and every launch is as described above and the host sends prefilled_off / prefilled_rq with each snapshot.  A prefilled task is an entry
 * of the same table with variant 0xFE (its worker: the one it is prefilled on; request and priority as for any entry); it counts in no (row, variant)
 * slot and touches no free row, and raises a count of its own per (worker row, request) — what process_proactive_filling reads (mapping.rs:197-203).
 *   hqtick_assigned_track_prefilled  tracking on, seeded with n prefilled tasks (ids, worker ids, rq, priority); n = 0 seeds nothing.  Needs an enabled
 *                              ledger; a second call replaces the prefilled entries; whatever switches the ledger off switches tracking off.  Entries
 *                              naming an unknown worker or request, an id already in the ledger or a worker without HQ_WORKER_SN are counted
 *                              (hqtick_assigned_last_unknown) and enter nothing.  HQTICK_E_UNSUPPORTED if a request has 254 or more variants.  Returns the
 *                              number entered.
 *   hqtick_assigned_start_prefilled  task_from_prefilled_to_started (worker.rs:212-221) for n (id, variant) pairs: the entry takes the variant, the
 *                              prefilled count drops, the (row, slot) count rises, free.remove is applied.  Request and priority are the entry's own.
 *                              Ids that are not prefilled entries and variants the request does not have are counted and change nothing.  Returns the
 *                              number started.
 *   hqtick_assigned_unprefill  remove_prefill_task (mapping.rs:85-88) outside a tick: process_retracted of a dissolved prefill set (reactor.rs:34-62), cancel
 *                              (:762-766), reject (:406-413), failed dependencies (:645-652).  The entry leaves, the prefilled count drops.  Ids that are
 *                              not prefilled entries are counted and change nothing (an assigned entry is never touched).  Returns the number removed.  Where
 *                              the task becomes Retracting the host calls hqtick_retracting_add as before.
 *   hqtick_assigned_prefilled_count  prefilled entries (hqtick_assigned_count stays the number of assigned single-node entries).
 *   hqtick_assigned_lookup     answers a prefilled id with its worker and variant 0xFE.
 *   hqtick_assigned_release    of a prefilled id counts it as unknown; hqtick_assigned_add of one counts it as a duplicate.  Neither changes anything.
 *   hqtick_cluster_remove_workers  the lost workers' prefilled entries leave with their other entries and are among hqtick_cluster_last_requeued, back in the
 *                              resident ready set with their request and stored priority (move_prefilled_task_to_ready: a plain add).
 *   hqtick_cluster_last_requeued_prefilled  the subset of the last hqtick_cluster_last_requeued that was prefilled, ascending: the host takes these out of
 *                              its queue-side prefill sets and skips their crash counters.
 * The tick with tracking on: a snapshot that carries prefilled_off is HQTICK_E_INVALID (two truths); the tick reads the per-(request, worker) prefilled counts
 * from the ledger.  Its PREFILL records enter as prefilled entries with its ASSIGN records, at the same moment (an abandoned or failed tick enters nothing);
 * a FROM_PREFILL redirect turns the task's prefilled entry into the assigned entry on the target, with the entry's own request and priority.
 * Not covered by tracking: the queue-side prefill sets (prefill_off / _priority / _task / _worker stay in the snapshot, in the Set's iteration order);
 * sharded contexts; integration/shim.rs.
 * Multi-node tasks (n_nodes > 0; Worker::mn_task, server/worker.rs:134-175) are the ledger's as well: per worker row the task it holds and whether it is
 * the root, per task one entry (root worker id, rq, priority).  A tick's multi-node placements (result.mn_*) enter with its ASSIGN records, at the same
 * moment (an abandoned or failed tick enters nothing): every listed worker loses HQ_WORKER_SN and records the task, the first as root (mapping.rs:133-154);
 * free rows stay as they are.  The next tick sees those workers as the reference does: no single-node placement on them.
 *   hqtick_assigned_add_mn     seed multi-node tasks after hqtick_assigned_enable (restore, tests): task i runs on worker_id[worker_off[i] .. worker_off[i + 1]),
 *                              root first.  A listed worker is either free (SN bit, nothing in the ledger, not STOPPING: Worker::is_free) or was uploaded
 *                              with the SN bit clear and holds no task yet.  A task that names an unknown worker, a busy or stopping one, a worker twice or
 *                              one an earlier task of the call took, whose id is in the ledger already or whose rq is not a multi-node request, is counted
 *                              (hqtick_assigned_last_unknown) and enters nothing.  Returns the number of tasks entered.
 *   hqtick_assigned_release    takes multi-node ids in the same batch: every row still holding the task gets reset_mn_task (worker.rs:172-175,
 *                              reactor.rs:357-363: SN bit set, free row = total row), the entry leaves, the return value counts the task once.
 *   hqtick_cluster_remove_workers  on_remove_worker (reactor.rs:107-128): a lost ROOT resets the task's other rows and the task is among
 *                              hqtick_cluster_last_requeued (and back in the resident ready set); a lost NON-ROOT just leaves, the task keeps its
 *                              remaining workers.  The outcome does not depend on the order of the ids within the call.
 *   hqtick_assigned_mn_count   multi-node tasks in the ledger (hqtick_assigned_count stays the number of single-node entries).
 *   hqtick_assigned_mn_workers the task's current workers, root first, the others by ascending id (valid until the next call on ctx); *n = 0: not a
 *                              multi-node task of the ledger.  hqtick_assigned_lookup of such an id answers with the root's worker id and variant 0xFF.
 * Not covered: a worker that takes a multi-node task while it still holds prefilled tasks (set_mn_task drops the set in the reference; the ledger leaves
 * its prefilled entries as they are).
 * The ledger does not depend on the form in which the records leave the device: the mapping kernel stages, beside every record it emits, the entry the
 * ledger stores (task, request, variant, worker row, priority level) in HBM, and the placement enters from there.  So the ledger works with plain records,
 * with HQTICK_FLAG_COMPACT_RECORDS / _DELTA16, and with a record sink (hqtick_set_record_sink, set before or after hqtick_assigned_enable, removed again
 * between ticks) on a context that is not sharded: with a sink the tick's records stay in HBM, hqwire_encode_device turns them into message bytes, and no
 * task record crosses PCIe in either direction.  A sink too small for a tick is HQTICK_E_CAPACITY as without the ledger; ledger, counts and free rows stay
 * as they were.
 *   hqtick_assigned_last_host_bytes  bytes of record data (offsets, task ids, variants, kinds, in any form) that the last placement's entry into the ledger
 *                              copied from host memory to the device: 0 in every form (redirects and the new_free rows are not counted).
 * HQTICK_E_UNSUPPORTED on a sharded or replica context (hqtick_set_shard with more than one shard, an exchange or a communicator).
 */
int hqtick_assigned_enable(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id, const uint32_t *rq, const uint8_t *variant, const uint64_t *priority);
int hqtick_assigned_disable(hqtick_ctx *ctx);
int hqtick_assigned_add(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id, const uint32_t *rq, const uint8_t *variant, const uint64_t *priority);
int hqtick_assigned_release(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id);
uint64_t hqtick_assigned_last_unknown(const hqtick_ctx *ctx);
uint64_t hqtick_assigned_count(const hqtick_ctx *ctx);
uint64_t hqtick_assigned_last_host_bytes(const hqtick_ctx *ctx);
int hqtick_assigned_lookup(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, uint32_t *worker_id, uint8_t *variant);
int hqtick_assigned_free_rows(hqtick_ctx *ctx, uint32_t *n_workers, const uint64_t **free_rows);
int hqtick_cluster_last_requeued(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id, const uint32_t **rq, const uint64_t **priority);
int hqtick_assigned_add_mn(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *rq, const uint64_t *priority, const uint32_t *worker_off,
                           const uint32_t *worker_id);
uint64_t hqtick_assigned_mn_count(const hqtick_ctx *ctx);
int hqtick_assigned_mn_workers(hqtick_ctx *ctx, uint64_t task_id, uint32_t *n, const uint32_t **worker_id);
int hqtick_assigned_track_prefilled(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id, const uint32_t *rq, const uint64_t *priority);
int hqtick_assigned_start_prefilled(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint8_t *variant);
int hqtick_assigned_unprefill(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id);
uint64_t hqtick_assigned_prefilled_count(const hqtick_ctx *ctx);
int hqtick_cluster_last_requeued_prefilled(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id);

/*
 * Cancelling tasks on the resident state in one call (functions added under ABI 12): on_cancel_tasks (server/reactor.rs:706-780) for the listed
 * ids, in the caller's order, on everything the context keeps resident.  The ids are staged once; the graph, the ready set and the ledger read that one copy.
 *   hqtick_cancel_tasks   needs a resident ready set and an enabled ledger; the graph and the prefilled tracking are optional.  The state afterwards:
 *       graph       with a graph (one that has held a task): as hqtick_graph_remove(ids, 1) leaves it -- the closure leaves the graph and the ready set, and
 *                   hqtick_graph_last_ids / _last_unknown answer as after that call.  Without one the listed ids leave the ready set as by hqtick_ready_remove.
 *       ledger      as hqtick_assigned_release(ids) followed by hqtick_assigned_unprefill(ids) leave it: single-node entries give their resources back in batch
 *                   order with the last-ALL rule, multi-node entries reset their rows, prefilled entries leave and lower their worker's prefilled count;
 *                   unknown ids and repeats change nothing.  hqtick_assigned_last_unknown: the positions that found no entry or repeated one.
 *       Retracting  a listed id leaves the table of hqtick_retracting_* (try_remove_redirection, reactor.rs:751-761: the ledger step has released its redirect
 *                   target's entry): a later hqtick_retract_response for it reassigns nothing.
 *     Only the listed ids are routed: a consumer in the closure is Waiting with unfinished dependencies and sits nowhere else.
 *     Returns the number of ids in the messages below; HQTICK_E_INVALID without a resident ready set, with the ledger off or with a two-call tick's placement
 *     pending (nothing changes then); HQTICK_E_CAPACITY for n > 2^31 - 1; n = 0 returns 0 and leaves empty lists.
 *     If a step fails after an earlier one succeeded the earlier ones stay done (graph and ready set first, then the ledger, then the table): the ledger calls
 *     named above finish the job, the lists below are empty.
 *   hqtick_cancel_last_messages   the CancelTasks lists (running_ids: Map<WorkerId, Vec<TaskId>>) as a CSR: the workers that get a message in ascending worker
 *       id, task_off[n_workers + 1], and per worker the ids in ascending batch position (the order the reference's Vec was pushed in).  An assigned, running
 *       or prefilled task goes to its worker, a multi-node task to its root, a Retracting task to the worker it is retracting FROM.
 *   hqtick_cancel_last_routes     per batch position the worker id (HQ_NO_WORKER: none) and an HQ_CANCEL_* kind.  HQ_CANCEL_REPEAT marks a later position of an
 *       id that has a ledger entry or is in the Retracting table (an id that sits in neither is HQ_CANCEL_NONE at every position).  A host needs _PREFILLED to take
 *       the task out of its queue-side prefill sets and _RETRACTING for its own task states.
 *   hqtick_cancel_last_ready_removed   tasks that left the resident ready set.
 * The arrays are pinned memory owned by the context, valid until the next hqtick_cancel_tasks.
 */
#define HQ_CANCEL_NONE       0
#define HQ_CANCEL_ASSIGNED   1
#define HQ_CANCEL_PREFILLED  2
#define HQ_CANCEL_MN         3
#define HQ_CANCEL_RETRACTING 4
#define HQ_CANCEL_REPEAT     5
int hqtick_cancel_tasks(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id);
int hqtick_cancel_last_messages(const hqtick_ctx *ctx, uint32_t *n_workers, const uint32_t **worker_id, const uint32_t **task_off, const uint64_t **task_id);
int hqtick_cancel_last_routes(const hqtick_ctx *ctx, uint32_t *n, const uint32_t **worker_id, const uint8_t **kind);
uint64_t hqtick_cancel_last_ready_removed(const hqtick_ctx *ctx);

/*
 * Finishing tasks on the resident state in one call (functions added under ABI 12): task_finished (server/reactor.rs:510-590) for a batch of
 * WorkerTaskUpdate::Finished, in the order the reactor saw them, on everything the context keeps resident.  Ids and reporting workers are staged once (12 B per
 * position); the ledger and the graph read that one copy.
 *   hqtick_finish_tasks   worker_id[i] is the worker whose TaskUpdates carried the finish of task_id[i]; a batch may mix workers.  It needs a resident ready set
 *       and an enabled ledger; the graph and the prefilled tracking are optional.  Every position gets an HQ_FINISH_* kind.  _ASSIGNED, _MN and _RETRACTING are
 *       ACCEPTED: the reporter is the worker of the single-node entry, the root of the multi-node entry, or -- for an id in the table of hqtick_retracting_* -- the
 *       worker the task is retracting FROM (the table decides, whatever the ledger names: its entry is the redirect target's).  Every other kind is REFUSED and
 *       changes nothing anywhere: _NONE (no entry and not in the table: "Unknown task finished"), _WRONG_WORKER (the reference's assert_eq!(*w_id, worker_id)),
 *       _PREFILLED (unreachable! in the reference), _REPEAT (a later position of an id an earlier position was accepted for).  A refused position claims
 *       nothing: a later position of the same id with the right worker is still accepted.  The state afterwards, for the accepted positions in batch order:
 *       ledger      as hqtick_assigned_release(accepted ids) leaves it: the last-ALL rule, multi-node rows reset, SN bits back.  For a Retracting id with a
 *                   redirect this releases the entry on the redirect target (try_remove_redirection, reactor.rs:592-604); one the tick had put back on the
 *                   worker it is retracting from gives that entry back.
 *       Retracting  accepted _RETRACTING ids leave the table of hqtick_retracting_*; one that still sat in its queue leaves the resident ready set too.
 *       graph       with a graph (one that has held a task): as hqtick_graph_finish(accepted ids) leaves it -- released consumers join the resident ready set, and
 *                   hqtick_graph_last_ids / _last_unknown answer as after that call.  A refused position is not shown to the graph.  An accepted task that still
 *                   had dependencies is HQTICK_E_INVALID as there: its consumers still join the ready set and the ledger step stays done.
 *     Returns the number of accepted positions (the handler's need_scheduling); hqtick_assigned_last_unknown is the number of refused ones.  HQTICK_E_INVALID
 *     without a resident ready set, with the ledger off, with a two-call tick's placement pending or with a NULL array (nothing changes then); HQTICK_E_CAPACITY
 *     for n > 2^26; n = 0 returns 0 and leaves an empty kind list.  If a step fails after an earlier one succeeded the earlier ones stay done (the ledger first,
 *     then the table, then graph and ready set): hqtick_graph_finish of the accepted ids finishes the job.
 *   hqtick_finish_last_routes   per batch position its HQ_FINISH_* kind: pinned memory owned by the context, valid until the next hqtick_finish_tasks.  Nobody
 *       is told about a finish, so there are no worker lists; a host needs the kinds for its own task objects and to log what the reference asserts.
 *   hqtick_retracting_started   task_running's Retracting arm (reactor.rs:311-335): for every id that is in the table with worker_id[i] the worker it is retracting
 *       FROM, the redirect target's ledger entry is released if there is one, the table entry is erased (with the id's place in the resident ready set, if it
 *       still sat in its queue), and the task is entered on worker_id[i] with (rq, variant, priority) as by hqtick_assigned_add -- in this order, so a task the
 *       tick had put back on that very worker can be entered again.  Other ids are refused, change nothing and are counted in hqtick_assigned_last_unknown.
 *       Returns the number started; the guards are those of hqtick_finish_tasks.
 */
#define HQ_FINISH_NONE         0
#define HQ_FINISH_ASSIGNED     1
#define HQ_FINISH_MN           2
#define HQ_FINISH_RETRACTING   3
#define HQ_FINISH_REPEAT       4
#define HQ_FINISH_WRONG_WORKER 5
#define HQ_FINISH_PREFILLED    6
int hqtick_finish_tasks(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id);
int hqtick_finish_last_routes(const hqtick_ctx *ctx, uint32_t *n, const uint8_t **kind);
int hqtick_retracting_started(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id, const uint32_t *rq, const uint8_t *variant,
                              const uint64_t *priority);

/*
 * Failing tasks on the resident state in one call (functions added under ABI 12): task_failed (server/reactor.rs:606-704) for a batch of
 * WorkerTaskUpdate::Failed and of the server's own task_failed(None, ..) (tasks that crashed on lost workers, reactor.rs:164-183), in the order the reactor saw
 * them, on everything the context keeps resident.  Ids and reporting workers are staged once (12 B per position); the ledger and the graph read that one copy.
 *   hqtick_fail_tasks   worker_id[i] is the worker whose TaskUpdates carried the failure of task_id[i], or HQ_NO_WORKER for the server's own call; a batch may mix
 *       workers.  It needs a resident ready set and an enabled ledger; the graph and the prefilled tracking are optional.  Every position gets an HQ_FAIL_* kind.
 *       _ASSIGNED, _MN, _PREFILLED, _RETRACTING and _WAITING are ACCEPTED: the reporter is the worker of the single-node or prefilled entry, the root of the
 *       multi-node entry, the worker a task in the table of hqtick_retracting_* is retracting FROM (the table decides first, whatever the ledger names), or
 *       HQ_NO_WORKER for an id with neither.  Every other kind is REFUSED and changes nothing anywhere: _NONE ("Unknown task failed"), _WRONG_WORKER (the
 *       reference's assert_eq!(worker_id, *w)), _NOT_WAITING (assert!(task.is_waiting())), _REPEAT (an earlier position was accepted for the id), _GONE (a
 *       _WAITING position whose task an earlier accepted position's closure has removed).  A refused position claims nothing: a later position of the same id with
 *       the right reporter is still accepted.  The kinds follow from the state before the batch and the claims of its positions; the state afterwards is that of
 *       the handler applied to the accepted positions in batch order:
 *       ledger      as hqtick_assigned_release(accepted ids) leaves it (the last-ALL rule, multi-node rows reset, SN bits back; for a Retracting id with a redirect
 *                   the redirect target's entry is released), and a _PREFILLED entry leaves as by hqtick_assigned_unprefill: the prefilled count drops, no free
 *                   row is touched.  Without prefilled tracking a failing Prefilled task has no entry and is _NONE: the host holds those sets and routes it
 *                   itself (task_queues.remove_prefilled + hqtick_graph_remove).
 *       Retracting  accepted _RETRACTING ids leave the table; one that still sat in its queue leaves the resident ready set too.
 *       graph       with a graph (one that has held a task): the accepted ids and their transitive consumers leave graph and ready set as after
 *                   hqtick_graph_remove(accepted ids, 1); hqtick_graph_last_ids / _last_unknown answer as after that call.  A _WAITING position whose id the graph
 *                   does not hold becomes _NONE.  Without a graph _WAITING and _RETRACTING ids just leave the ready set if they sit there.
 *     Returns the number of accepted positions after the graph step; hqtick_assigned_last_unknown is the number of refused ones.  HQTICK_E_INVALID without a
 *     resident ready set, with the ledger off, with a two-call tick's placement pending or with a NULL array (nothing changes then); HQTICK_E_CAPACITY for
 *     n > 2^26; n = 0 returns 0 and leaves empty lists.  If a step fails after an earlier one succeeded the earlier ones stay done (the ledger first, then the
 *     table, then graph and ready set): hqtick_graph_remove(accepted ids, 1) finishes the job and the consumer lists are empty.  An accepted position of a
 *     ledger or table kind whose task an earlier accepted position reaches cannot occur on a state hqtick_resident_check accepts: every step completes by the same
 *     rule and the call returns HQTICK_E_INVALID, naming the task.
 *   hqtick_fail_last_routes      per batch position its HQ_FAIL_* kind: pinned memory owned by the context, valid until the next hqtick_fail_tasks.
 *   hqtick_fail_last_consumers   what client.on_task_error wants per failed task: consumer_off [n + 1] by batch position, consumer_id ascending inside a position.
 *       Task c belongs to the SMALLEST accepted position whose closure holds it -- what the handler applied position by position gives.  A refused position has
 *       an empty range; the failed task itself is never in its own list; a _GONE position's task is in the list of the position that removed it.  The accepted
 *       ids and all lists together are hqtick_graph_last_ids.  Pinned memory owned by the context, valid until the next hqtick_fail_tasks; without a graph every
 *       range is empty.
 */
#define HQ_FAIL_NONE         0   /* refused: reporter given, no entry, not in the table */
#define HQ_FAIL_ASSIGNED     1   /* accepted: single-node entry (Assigned or Running), reporter is its worker */
#define HQ_FAIL_MN           2   /* accepted: multi-node entry, reporter is its root */
#define HQ_FAIL_PREFILLED    3   /* accepted: prefilled entry (tracking on), reporter is its worker */
#define HQ_FAIL_RETRACTING   4   /* accepted: in the Retracting table, reporter is the worker it retracts FROM */
#define HQ_FAIL_WAITING      5   /* accepted: reporter HQ_NO_WORKER, no entry, not in the table */
#define HQ_FAIL_REPEAT       6   /* refused: an earlier position was accepted for this id */
#define HQ_FAIL_WRONG_WORKER 7   /* refused: the reference's assert_eq!(worker_id, *w) */
#define HQ_FAIL_NOT_WAITING  8   /* refused: reporter HQ_NO_WORKER but the id has an entry or is in the table (assert!(task.is_waiting())) */
#define HQ_FAIL_GONE         9   /* refused by the graph step: a WAITING position whose id an earlier accepted position's closure removed ("Unknown task failed") */
int hqtick_fail_tasks(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id);
int hqtick_fail_last_routes(const hqtick_ctx *ctx, uint32_t *n, const uint8_t **kind);
int hqtick_fail_last_consumers(const hqtick_ctx *ctx, uint32_t *n, const uint32_t **consumer_off, const uint64_t **consumer_id);

/*
 * Starting tasks on the resident state in one call (functions added under ABI 12): task_running (server/reactor.rs:264-355) for a batch of
 * WorkerTaskUpdate::Running / RunningPrefilled, in the order the reactor saw them.  Ids, reporting workers and started variants are staged once (13 B per
 * position).  Every ledger entry carries a RUNNING byte: 0 when it enters (a tick's placement, hqtick_assigned_enable / _add / _add_mn, a prefilled seed, an
 * upsert that moves the id), 1 once the task was reported running (this call, hqtick_assigned_start_prefilled, hqtick_retracting_started).  Multi-node entries
 * keep 0: the reference has no Assigned state for them.
 *   hqtick_start_tasks   worker_id[i] reported task_id[i] running with variant[i]; a batch may mix workers.  rq[i] / priority[i] are the task's own request and
 *       priority, read only for accepted _RETRACTING positions (as hqtick_retracting_started takes them); both may be NULL while the table of hqtick_retracting_*
 *       is empty.  It needs a resident ready set and an enabled ledger.  Every position gets an HQ_START_* kind from the state BEFORE the batch:
 *         id in the Retracting table   reported by the worker it is retracting FROM: _RETRACTING (accepted; the table decides whatever the ledger names);
 *                                      _BAD_VARIANT if rq[i] has no variant[i]; reported by anyone else: _WRONG_WORKER
 *         no entry                     _NONE (the task is unknown or Waiting)
 *         prefilled entry              its worker: _PREFILLED (accepted), _BAD_VARIANT if its request has no such variant; another worker: _WRONG_WORKER
 *         single-node entry            another worker: _WRONG_WORKER (assert_eq!(*w_id, worker_id)); its worker, another variant: _WRONG_VARIANT
 *                                      (assert_eq!(*assigned_rv_id, rv_id)); its worker and variant: _RUNNING if it already runs (unreachable! in the reference),
 *                                      else _ASSIGNED (accepted)
 *         multi-node entry             the root: _MN (accepted; nothing changes, so every such position is _MN); another worker: _WRONG_WORKER
 *       Only _ASSIGNED, _PREFILLED and _RETRACTING positions claim their id: the lowest such position wins, the others become _REPEAT.  A refused position
 *       claims nothing and changes nothing.  The state afterwards is that of the handler applied to the accepted positions in batch order:
 *         _ASSIGNED    the entry's running byte is set; nothing else changes
 *         _PREFILLED   as hqtick_assigned_start_prefilled(id, the WINNING position's variant), and the running byte is set
 *         _RETRACTING  as hqtick_retracting_started for that one position, entered with the running byte set.  Such a start does not commute with a saturating
 *                      start on the same worker row, so the batch is cut at each of these positions: what comes before it is applied first.
 *     Returns the number of accepted positions; hqtick_assigned_last_unknown is the number of refused ones.  The handler asks for scheduling
 *     (ask_for_scheduling(), reactor.rs:313) iff some kind is _RETRACTING.  HQTICK_E_INVALID without a resident ready set, with the ledger off, with a two-call
 *     tick's placement pending, with a NULL id / worker / variant array, or with rq or priority NULL while the Retracting table holds a task (nothing changes
 *     then); HQTICK_E_CAPACITY for n > 2^26; n = 0 returns 0 and leaves an empty kind list.  If a step of a _RETRACTING position fails, the positions before it
 *     stay started and the kind list is empty.
 *   hqtick_start_last_routes   per batch position its HQ_START_* kind: pinned memory owned by the context, valid until the next hqtick_start_tasks.
 *   hqtick_assigned_running    per id the running byte of its entry (0 / 1; 0xFF: not in the ledger).  Returns the number found.
 *   hqtick_cluster_last_requeued_running   the subset of the last hqtick_cluster_last_requeued that is on_remove_worker's running_tasks (reactor.rs:72-120), ids
 *       ascending: single-node entries whose running byte was set and multi-node tasks whose root was lost -- what client.on_worker_lost is told and what gets a
 *       crash counter.  Prefilled and merely assigned entries, and a Retracting task's entry on a lost redirect target, are not in it.
 */
#define HQ_START_NONE          0   /* refused: no entry, not in the table */
#define HQ_START_ASSIGNED      1   /* accepted: single-node entry, its worker and variant, not yet running */
#define HQ_START_MN            2   /* accepted: multi-node entry, reporter is its root; claims nothing */
#define HQ_START_PREFILLED     3   /* accepted: prefilled entry (tracking on), reporter is its worker */
#define HQ_START_RETRACTING    4   /* accepted: in the Retracting table, reporter is the worker it retracts FROM */
#define HQ_START_REPEAT        5   /* refused: an earlier eligible position claimed this id */
#define HQ_START_WRONG_WORKER  6   /* refused: the reference's assert_eq!(*w_id, worker_id) / assert_eq!(ws[0], worker_id) */
#define HQ_START_WRONG_VARIANT 7   /* refused: the reference's assert_eq!(*assigned_rv_id, rv_id) */
#define HQ_START_RUNNING       8   /* refused: the single-node entry already runs (unreachable! in the reference) */
#define HQ_START_BAD_VARIANT   9   /* refused: the request of a prefilled or Retracting task has no such variant */
int hqtick_start_tasks(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id, const uint8_t *variant, const uint32_t *rq,
                       const uint64_t *priority);
int hqtick_start_last_routes(const hqtick_ctx *ctx, uint32_t *n, const uint8_t **kind);
int hqtick_assigned_running(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, uint8_t *running);
int hqtick_cluster_last_requeued_running(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id);

/*
 * Rejecting tasks on the resident state in one call (functions added under ABI 12): task_reject and request_enabled (server/reactor.rs:365-460) for a
 * batch of WorkerTaskUpdate::RejectRequest, in the order the reactor saw them.  Ids, reporting workers, rejected variants and the order of the positions by
 * ascending (id, position) are staged once (17 B per position, 21 B while the Retracting table holds a task).
 *   hqtick_reject_tasks   worker_id[i] rejected task_id[i] with variant[i] (0xFF: None, as in the records); a batch may mix workers and arms.  rq[i] is the task's
 *       own request, read only for the positions the Retracting table decides (the table holds no request, and a Retracting task without a redirect has no ledger
 *       entry); it may be NULL while that table is empty.  No priority is passed: a requeued task's request and priority are its ledger entry's own.  It needs a
 *       resident ready set and an enabled ledger.  Every position gets an HQ_REJECT_* kind from the state BEFORE the batch:
 *         id in the Retracting table   reported by the worker it is retracting FROM: _REDIRECTED if the table holds a redirect (accepted: the task is Assigned on the
 *                                      target, reactor.rs:420-431; it leaves the table, the target's ledger entry stays, and the triple is in
 *                                      hqtick_reject_last_reassigned for the ComputeTasks message), else _RETRACTING (accepted: it leaves the table; the task is
 *                                      already a member of the ready set and is not added again); _BAD_VARIANT if a variant is named that rq[i] does not have;
 *                                      reported by anyone else: _WRONG_WORKER
 *         no entry                     _NONE (the task is unknown, Waiting or Ready)
 *         multi-node entry             _MN (refused: unreachable! in the reference)
 *         entry of another worker      _WRONG_WORKER
 *         a variant is named that the entry's request does not have   _BAD_VARIANT
 *         prefilled entry              its worker, any variant, None included: _PREFILLED (accepted)
 *         single-node entry            _RUNNING if it already runs (refused: unreachable! in the reference); None or a variant that is not the entry's:
 *                                      _WRONG_VARIANT (resource_rq_variant != Some(*rv_id)); its worker and variant: _ASSIGNED (accepted)
 *       Only the four accepted kinds claim their id: the lowest such position wins, the others become _REPEAT.  The state afterwards is that of the handler applied
 *       to the accepted positions in batch order:
 *         _ASSIGNED    the entry leaves as by hqtick_assigned_release (count, free row and the last-ALL arithmetic in batch order)
 *         _PREFILLED   the entry leaves as by hqtick_assigned_unprefill
 *         both         go back into the resident ready set with the entry's request and priority (add_ready_task, :440-442), merged on the device; the last tick's
 *                      selection is abandoned, as by any delta.  The graph is not touched: the task is still in the task map.
 *       Blocks (worker.block_request, :389-391, runs before the state is looked at): the pair (request of the task, variant[i]) joins worker_id[i]'s blocked set for
 *       every position of kind _ASSIGNED, _PREFILLED, _RETRACTING, _REDIRECTED, _WRONG_WORKER or _WRONG_VARIANT whose variant is not None, whose request has that
 *       variant and whose reporter is a resident worker; a pair already blocked is not added twice.  _NONE, _REPEAT, _MN, _RUNNING and _BAD_VARIANT change nothing.
 *       Two deliberate deviations: an Assigned or Prefilled task reported by the wrong worker is refused after its block (the reference requeues it without
 *       releasing it, a state its own sanity_check rejects); a reporter that is not a resident worker is _WRONG_WORKER and blocks nothing.
 *     Returns the number of accepted positions; hqtick_assigned_last_unknown is the number of refused ones.  The handler asks for scheduling (task_reject returns
 *     true) iff some kind is _ASSIGNED, _PREFILLED or _RETRACTING.  HQTICK_E_INVALID without a resident ready set, with the ledger off, with a two-call tick's
 *     placement pending, with a NULL id / worker / variant array, or with rq NULL while the Retracting table holds a task (nothing changes then);
 *     HQTICK_E_CAPACITY for n > 2^26; n = 0 returns 0 and leaves an empty kind list.  Every buffer is ensured before the first change.
 *     A WorkerTaskUpdate batch that interleaves EnableRequest with rejects is cut by the host at each EnableRequest.
 *   hqtick_reject_last_routes      per batch position its HQ_REJECT_* kind: pinned memory owned by the context, valid until the next hqtick_reject_tasks.
 *   hqtick_reject_last_requeued    what went back into the ready set: ids ascending with request and priority, pinned memory, valid until the next
 *       hqtick_reject_tasks.  The host needs it for check_dispose_prefill / process_retracted of its queue-side prefill sets and for its Task objects.
 *   hqtick_reject_last_reassigned  the _REDIRECTED tasks as (task, redirect target, variant) in batch order: the ComputeTasks messages the host sends.
 *   hqtick_cluster_enable_request  request_enabled (:447-460): the pair leaves the worker's blocked set.  Returns 1 if it was there, 0 if not (nothing changes);
 *       HQTICK_E_INVALID for an unknown worker.  Works without the ledger.
 *   hqtick_cluster_blocked         one worker's blocked pairs in the order they were added (valid until the next change of that worker's set); without the ledger too.
 *       hqtick_cluster_set_blocked keeps its meaning: it replaces the worker's whole set.
 */
#define HQ_REJECT_NONE          0   /* refused: no entry, not in the table */
#define HQ_REJECT_ASSIGNED      1   /* accepted: single-node entry, its worker and variant, not running: released and requeued */
#define HQ_REJECT_PREFILLED     2   /* accepted: prefilled entry reported by its worker: unprefilled and requeued */
#define HQ_REJECT_RETRACTING    3   /* accepted: in the Retracting table without a redirect, reporter is the worker it retracts FROM */
#define HQ_REJECT_REDIRECTED    4   /* accepted: in the Retracting table with a redirect: Assigned on the target */
#define HQ_REJECT_REPEAT        5   /* refused: an earlier accepted position claimed this id */
#define HQ_REJECT_WRONG_WORKER  6   /* refused after its block: the entry / the table names another worker, or the reporter is not resident */
#define HQ_REJECT_WRONG_VARIANT 7   /* refused after its block: None, or not the variant the single-node entry was assigned with */
#define HQ_REJECT_RUNNING       8   /* refused: the single-node entry already runs (unreachable! in the reference) */
#define HQ_REJECT_BAD_VARIANT   9   /* refused: the task's request has no such variant */
#define HQ_REJECT_MN           10   /* refused: multi-node entry (unreachable! in the reference) */
int hqtick_reject_tasks(hqtick_ctx *ctx, uint32_t n, const uint64_t *task_id, const uint32_t *worker_id, const uint8_t *variant, const uint32_t *rq);
int hqtick_reject_last_routes(const hqtick_ctx *ctx, uint32_t *n, const uint8_t **kind);
int hqtick_reject_last_requeued(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id, const uint32_t **rq, const uint64_t **priority);
int hqtick_reject_last_reassigned(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id, const uint32_t **worker_id, const uint8_t **variant);
int hqtick_cluster_enable_request(hqtick_ctx *ctx, uint32_t worker_id, uint32_t rq, uint8_t variant);
int hqtick_cluster_blocked(const hqtick_ctx *ctx, uint32_t worker_id, uint32_t *n, const uint32_t **rq, const uint8_t **variant);

/*
 * Losing workers on the resident state in one call (functions added under ABI 12): on_remove_worker (server/reactor.rs:64-186) for a batch of lost
 * workers, with what the handler needs per worker.  hqtick_cluster_remove_workers stays as it is; this call leaves the same resident state and reports more.
 *   hqtick_lose_workers   the workers worker_id[0 .. n) are lost.  It needs a resident worker set, a resident ready set and an enabled ledger.  Every ledger entry
 *       of a lost worker leaves the ledger (a multi-node entry is its ROOT's: a lost root evicts the task and frees the task's other rows, a lost non-root only
 *       leaves), the rows leave the worker set and the ledger's row tables, the Retracting table follows (an entry retracting FROM a lost worker leaves -- with a
 *       redirect to a worker that stays the task is Assigned there and reported by hqtick_lose_last_reassigned; an entry whose redirect TARGET is lost loses the
 *       redirect and is back in its queue), and the evicted tasks go back into the resident ready set with their entries' own request and priority, merged on
 *       the device: ready set, ledger entries, counts, free rows, prefilled counts, multi-node rows and flags, worker rows, blocked sets and Retracting table are
 *       those hqtick_cluster_remove_workers leaves for the same list.  The evicted entries are sorted, classified and grouped on the device; no column of a
 *       requeued task crosses PCIe as input to the merge.
 *       Returns the number of tasks that went back into the ready set.  HQTICK_E_INVALID without a worker set, without a resident ready set, with the ledger off,
 *       with a two-call tick's placement pending, with a NULL array, or with an unknown or repeated worker id (nothing changes then); n = 0 returns 0 and leaves
 *       every list empty.  Every buffer of the eviction, the grouping and the merge is ensured before the first change.  If a later step still fails, what the
 *       lists hold says how far the call came: a failure of the eviction or of a re-pack (a device error) leaves all five lists EMPTY, and the host uploads the
 *       worker set and enables the ledger again from its own view; a failure of the last step -- the worker ids of the new rows, or the merge, which also refuses a
 *       requeued id the host had put into the ready set itself (HQTICK_E_INVALID) -- leaves the five lists FILLED: the workers are gone, the entries have left the
 *       ledger, the Retracting table has followed, the ready set is as it was, and hqtick_ready_add of hqtick_lose_last_requeued finishes the job.
 *       The host keeps these jobs: instance ids, crash counters, hqtick_fail_tasks(id, HQ_NO_WORKER) for a task over its crash limit, the prefill disposal an
 *       arrival triggers (check_dispose_prefill / process_retracted), the messages.
 *   hqtick_lose_last_tasks   a CSR over the lost workers in the CALLER'S order: worker i held task_id[task_off[i] .. task_off[i + 1]), ids ascending inside a
 *       worker, each with its entry's request and priority and an HQ_LOSE_* kind.  The union of the lists is exactly hqtick_lose_last_requeued.
 *   hqtick_lose_last_requeued    the same tasks as one list, ids strictly ascending, with request and priority.
 *   hqtick_lose_last_reassigned  (task, redirect target, variant) of the Retracting tasks that are Assigned on their target now: the ComputeTasks messages.
 *   hqtick_lose_last_mn_left     one (task, lost worker, root worker) triple per lost worker that was a NON-root member of a multi-node task whose root stays
 *       (the reference's ws.retain(|x| x != worker_id)): ascending by task id, then in the caller's order of the lost workers.  A task whose root is lost in the
 *       same batch is not listed: it is _MN_ROOT in its root's list.
 *   All five lists are memory owned by the context (the columns of the first two pinned), valid until the next hqtick_lose_workers; no other call touches them.
 *   After hqtick_lose_workers the hqtick_cluster_last_requeued / _prefilled / _running accessors are EMPTY (they answer for hqtick_cluster_remove_workers only);
 *   hqtick_cluster_last_reassigned reads the Retracting table's own last list and therefore repeats hqtick_lose_last_reassigned until the next
 *   hqtick_cluster_remove_workers / hqtick_retract_response.
 */
#define HQ_LOSE_ASSIGNED   0   /* single-node entry, not running: task object Waiting, instance id bumped */
#define HQ_LOSE_RUNNING    1   /* single-node entry, running: as above, and one of the worker's running_tasks (on_worker_lost, crash counter) */
#define HQ_LOSE_PREFILLED  2   /* prefilled entry (tracking on): move_prefilled_task_to_ready, leaves the queue-side prefill set, no crash counter */
#define HQ_LOSE_MN_ROOT    3   /* multi-node entry whose root this worker is: one of running_tasks; the other workers' rows are free single-node rows again */
#define HQ_LOSE_REDIRECT   4   /* single-node entry of a Retracting task whose redirect TARGET this worker is: the redirect is dropped, the task is back in its
                                  queue and stays Retracting{old} (reactor.rs:90-96), or is Waiting if `old` is lost in the same batch */
int hqtick_lose_workers(hqtick_ctx *ctx, uint32_t n, const uint32_t *worker_id);
int hqtick_lose_last_tasks(const hqtick_ctx *ctx, uint32_t *n_workers, const uint32_t **task_off, const uint64_t **task_id, const uint32_t **rq, const uint64_t **priority,
                           const uint8_t **kind);
int hqtick_lose_last_requeued(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id, const uint32_t **rq, const uint64_t **priority);
int hqtick_lose_last_reassigned(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id, const uint32_t **worker_id, const uint8_t **variant);
int hqtick_lose_last_mn_left(const hqtick_ctx *ctx, uint32_t *n, const uint64_t **task_id, const uint32_t **lost_worker_id, const uint32_t **root_worker_id);

/*
 * Audit of the resident state (function added under ABI 12): the counterpart of Core::sanity_check (server/core.rs:280-436) for what the
 * library holds in HBM.  The host that could compare the structures with a second copy no longer keeps one, so the comparison runs on the device, where the
 * state is: read-only kernels on the context's stream, behind every queued delta, reporting per invariant how many keys violate it and the smallest one.
 *   parts     HQ_CHECK_* bits.  A part whose structure is not resident is skipped (it is missing from report.checked); that is not an error.
 *   returns   report.n_failed (>= 0); HQTICK_E_INVALID for a NULL argument or an undefined bit in parts; HQTICK_E_DEVICE as everywhere else.
 * The call may come between any two calls on the context, also between hqtick_run_resident and hqtick_ready_consume_last (the state then is the one before the
 * tick's placement: the selected tasks are still in the ready set and not yet in the ledger).  It changes no resident byte, abandons no pending selection or
 * placement, and leaves the "valid until the next call" pointers of the other accessors alone.  Works on sharded and replica contexts, for the parts they can hold.
 * Its scratch (4 B per graph slot, ledger bucket and count-table cell) is allocated at the first call and freed by hqtick_destroy; a context that never calls it
 * launches and allocates nothing new.
 * count[] and first[] are integer sums and 64-bit minima: they do not depend on the order in which the device's threads run.
 *
 * The invariants, with the key reported in first[]:
 *   READY   HQ_INV_READY_ORDER       the physical id column ascends strictly (tombstones keep their ids)                 [the id at the first bad position]
 *           HQ_INV_READY_COUNT       the rows whose request id is not the tombstone number hqtick_ready_count            [the device's count]
 *   GRAPH   HQ_INV_GRAPH_HASH        every live slot's id is found at that slot through the hash table                    [task id]
 *           HQ_INV_GRAPH_TOTALS      live slots == n_tasks, and live slots + free stack == slots ever used                [the device's live count]
 *           HQ_INV_GRAPH_COUNTER     unfinished[c] == the edges into c whose generation matches, over the run chains of live producers — the
 *                                    assert_eq!(*unfinished_deps, count) of core.rs:353-367; stale edges and producers that left do not count     [task id]
 *   CROSS   (each evaluated when both of its sides are resident; what must hold whenever no handler is half done)
 *           HQ_INV_X_READY_ASSIGNED  no live ready id is a live entry of the assignment ledger, of any kind                [task id]
 *           HQ_INV_X_READY_WAITING   with a non-empty graph: no live ready id is in the graph with a non-zero counter      [task id]
 *           HQ_INV_X_RETRACTING      per entry of the Retracting table (core.rs:325-347): in_queue => live in the ready set; a redirect, with the ledger
 *                                    on => a single-node (not prefilled) ledger entry on the target worker with that variant                     [task id]
 *   STRICT  (opt-in: holds only for a host that keeps EVERY task in the graph; needs a non-empty graph and the ready set or the ledger)
 *           HQ_INV_S_READY_UNKNOWN     a live ready id that the graph does not hold                                        [task id]
 *           HQ_INV_S_ASSIGNED_WAITING  a ledger id that the graph does not hold, or holds with a non-zero counter           [task id]
 *           HQ_INV_S_RELEASED_NOWHERE  a graph task with counter 0 that is neither live in the ready set nor in the ledger; evaluated only with the ledger
 *                                      and its prefilled tracking on (else skipped: STRICT stays in checked)                                                        [task id]
 *   LEDGER  (needs the ledger on; Worker::sanity_check server/worker.rs:236-271 and the multi-node arm of Core::sanity_check)
 *           HQ_INV_LEDGER_HASH       probing for a live bucket's key finds that bucket: catches a duplicate key and an entry cut off by an EMPTY     [task id]
 *           HQ_INV_LEDGER_ENTRY      a live entry names a resident worker id and a known request; its variant is below the request's variant count (and has
 *                                    a column in the count table), or 0xFF on a multi-node request, or 0xFE with prefilled tracking on               [task id]
 *           HQ_INV_LEDGER_TOTALS     the device's census of single-node / multi-node / prefilled entries equals the host's counts
 *                                                                                                  [sn | mn << 21 | pf << 42 of the census, each saturated]
 *           HQ_INV_LEDGER_COUNTS     counts[row][slot] == the live single-node entries of that worker and (rq, variant)          [worker id << 32 | slot]
 *           HQ_INV_LEDGER_PREFILLED  pf[row][rq] == the live prefilled entries of that worker and request, with tracking on        [worker id << 32 | rq]
 *           HQ_INV_LEDGER_FREE       for every row with HQ_WORKER_SN: free[row][r] == what resources.clone() followed by remove(rq) per assigned task leaves:
 *                                    0 if a running (rq, variant) has an ALL entry on r, else total - sum of count x amount, saturating at 0 (the product and
 *                                    the sum saturate, they never wrap).  Computed from the count table and the request tables.  A release batch in the
 *                                    "B (ALL), then A (AMOUNT)" order (hqtick_assigned_release above) IS reported: the reference's own check asserts on it;
 *                                    so is a worker over-committed by hqtick_assigned_start_prefilled once its tasks are released   [worker id << 32 | r]
 *           HQ_INV_LEDGER_MN         a row's multi-node task is a live 0xFF entry; such a row has the SN bit clear and all-zero counts; every multi-node entry
 *                                    has exactly one root row, whose worker is the entry's.  (SN clear and no task is allowed: hqtick_assigned_add_mn.)
 *                                                                                                                         [task id, else worker id]
 * HQTICK_CHECK_RESIDENT=1 in the environment at hqtick_create (debug, like HQTICK_CHECK_CLUSTER): every successful call that changes resident state -- the ready-set,
 * graph, ledger, cluster and membership calls, the consume, a tick -- ends with the audit of READY | LEDGER | GRAPH, the parts that must hold after every single call (CROSS
 * and STRICT hold only between whole handlers and are never run in this mode).  A violation makes that call return HQTICK_E_INVALID with the invariant's name
 * and witness in hqtick_last_error; what the call did stays done.  hqtick_cluster_update_workers stays asynchronous and is not audited itself; nor are
 * hqtick_cluster_set_clock, hqtick_cluster_set_blocked and the hqtick_retracting_* calls, which change none of the three parts.
 */
#define HQ_CHECK_READY   1u    /* the ready set by itself                                   */
#define HQ_CHECK_LEDGER  2u    /* the ledger with the worker rows and request tables        */
#define HQ_CHECK_GRAPH   4u    /* the dependency graph by itself                            */
#define HQ_CHECK_CROSS   8u    /* between structures: what must hold whenever no handler is half done */
#define HQ_CHECK_STRICT  16u   /* what holds only for a host that keeps EVERY task in the graph and runs ledger + prefilled tracking */
#define HQ_CHECK_ALL     15u   /* (STRICT is opt-in) */
enum {
    HQ_INV_READY_ORDER = 0, HQ_INV_READY_COUNT = 1,
    HQ_INV_LEDGER_HASH = 2, HQ_INV_LEDGER_ENTRY = 3, HQ_INV_LEDGER_TOTALS = 4, HQ_INV_LEDGER_COUNTS = 5, HQ_INV_LEDGER_PREFILLED = 6, HQ_INV_LEDGER_FREE = 7, HQ_INV_LEDGER_MN = 8,
    HQ_INV_GRAPH_HASH = 9, HQ_INV_GRAPH_TOTALS = 10, HQ_INV_GRAPH_COUNTER = 11,
    HQ_INV_X_READY_ASSIGNED = 12, HQ_INV_X_READY_WAITING = 13, HQ_INV_X_RETRACTING = 14,
    HQ_INV_S_READY_UNKNOWN = 15, HQ_INV_S_ASSIGNED_WAITING = 16, HQ_INV_S_RELEASED_NOWHERE = 17,
    HQ_INV_N = 18
};
typedef struct hqtick_check_report {
    uint32_t checked;              /* HQ_CHECK_* parts that were asked for AND present */
    uint32_t n_failed;             /* invariants with count != 0 */
    uint64_t count[18];            /* [HQ_INV_N] violations per invariant */
    uint64_t first[18];            /* [HQ_INV_N] the SMALLEST offending key (above), UINT64_MAX when count == 0 */
    double   kernel_us;            /* HIP-event time of the audit's device work */
} hqtick_check_report;
int hqtick_resident_check(hqtick_ctx *ctx, uint32_t parts, hqtick_check_report *out);

/*
 * Device-resident dependency graph (BASELINE config 5): the `Waiting{unfinished_deps}` counters and the consumer
 * sets of tako's task map live in HBM next to the ready set, so a batch of `Finished` updates releases its consumers into the
 * resident ready set on the device.  A resident ready set must exist (hqtick_upload_ready with n = 0 creates an empty one).
 *   hqtick_graph_add_tasks   on_new_tasks  server/reactor.rs:188-220.  Tasks in submission order; dep_off[n + 1] / dep_task_id is
 *                            the CSR of Task::task_deps (each list free of duplicates, as hyperqueue's submit guarantees,
 *                            crates/hyperqueue/src/server/client/submit.rs:446).  A dependency is kept only if the task map holds
 *                            it when the consumer is processed: ids that are not in the graph (finished tasks), the task itself and
 *                            tasks LATER in the same batch are dropped, exactly as `find_task_mut` misses them.  Tasks with no kept
 *                            dependency are merged into the ready set (Core::add_task, server/core.rs:213-218).
 *                            Returns how many tasks of the batch are ready now.  HQTICK_E_INVALID (graph unchanged) if an id is
 *                            already in the graph or listed twice (the reference asserts, core.rs:217).
 *   hqtick_graph_finish      task_finished  server/reactor.rs:510-590: every consumer's counter is decremented
 *                            (Task::decrease_unfinished_deps, server/task.rs:207-216); consumers reaching 0 are merged into the ready
 *                            set (add_ready_task); the finished tasks leave the graph (Core::remove_task).  Ids that are not in the
 *                            graph are counted (hqtick_graph_last_unknown; "Unknown task finished", reactor.rs:565-567).  The tasks
 *                            must not be in the ready set any more (they were handed out by a tick).  Returns the number of
 *                            released tasks.
 *   hqtick_graph_remove      Core::remove_task  server/core.rs:222-240 for cancel (on_cancel_tasks, reactor.rs:706-780) and failed
 *                            dependencies (task_failed, reactor.rs:606-704): the tasks leave the graph and, if they are there, the
 *                            ready set.  recursive != 0 also removes their transitive consumers
 *                            (Task::collect_recursive_consumers, server/task.rs:235-250).  Returns the number of removed tasks.
 *   hqtick_graph_last_ids    ids the last graph call produced (ready-now / released / removed tasks), ASCENDING, in pinned host
 *                            memory owned by the ctx; valid until the next graph call.  The host shim uses them to keep its Task
 *                            objects in step (state Waiting{0}, client notifications).
 *   hqtick_graph_unfinished  Task::get_unfinished_deps for each id; 0xFFFFFFFF for ids that are not in the graph (test accessor).
 * Task ids >= 0xFFFFFFFFFFFFFFFE are reserved.  Memory: 52 B per task slot + 24 B per hash bucket (2-4 buckets per task) + 20 B per
 * dependency edge; pools grow on demand and are compacted when the dead edges of finished producers fill them.
 */
typedef struct hqtick_graph_stats {
    uint64_t n_tasks;          /* tasks in the graph (waiting, ready, assigned, running)   */
    uint64_t n_slots;          /* task slots ever used (high-water mark)                    */
    uint64_t n_edges_live, n_edges_pool, n_runs;
    uint64_t hash_capacity, hash_tombstones;
    uint64_t bytes_hbm;
    double last_kernel_us;     /* HIP-event time of the dominant kernel(s) of the last graph call */
} hqtick_graph_stats;
int hqtick_graph_add_tasks(hqtick_ctx *ctx, uint64_t n, const uint64_t *task_id, const uint64_t *task_priority,
                           const uint32_t *task_rq, const uint32_t *dep_off, const uint64_t *dep_task_id);
int hqtick_graph_finish(hqtick_ctx *ctx, uint64_t n, const uint64_t *task_id);
int hqtick_graph_remove(hqtick_ctx *ctx, uint64_t n, const uint64_t *task_id, int recursive);
const uint64_t *hqtick_graph_last_ids(const hqtick_ctx *ctx, uint64_t *n);
uint64_t hqtick_graph_last_unknown(const hqtick_ctx *ctx);
int hqtick_graph_unfinished(hqtick_ctx *ctx, uint64_t n, const uint64_t *task_id, uint32_t *out);
int hqtick_graph_get_stats(const hqtick_ctx *ctx, hqtick_graph_stats *out);
/* EXTENSION — no reference counterpart, parity unpinned, OFF unless called (BASELINE.json configs[4] names a "dynamic b-level recompute"; the reference has none:
 * the low 32 bits of Priority, "scheduler priority", are never written — common/priority.rs:43-66, server/task.rs:175-177).
 * hqtick_graph_blevel: b-level(t) = 0 for a task no task still in the graph depends on, else 1 + the largest b-level among its consumers — the longest path
 * from t to a sink — for every task of the device-resident graph, by level-synchronous sweeps over its consumer lists; the value REPLACES the low 32 bits of the
 * task's priority (what Priority::add_priority_u32 would add to a priority whose low bits are zero), so that tasks released by later hqtick_graph_finish calls
 * carry it into the ready set.  HQTICK_BLEVEL_UPDATE_READY: the tasks already in the resident ready set get their graph priorities too (one pass over the ready
 * columns, ids -> graph slots through the hash table; *n_ready_updated = how many).  Returns the number of sweeps (>= 0) or a negative error; *max_level = the
 * largest b-level (the depth of the graph).  A host that wants the reference's behaviour never calls it; no parity test does.  It may be called between
 * hqtick_run_resident and hqtick_ready_consume_last: the pending consume is not disturbed (it replays the last tick's selection, which does not read priorities).
 * hqtick_graph_priorities: the priorities the graph holds for the given ids (0 for an id it does not hold): test accessor. */
#define HQTICK_BLEVEL_UPDATE_READY 1u
int hqtick_graph_blevel(hqtick_ctx *ctx, uint32_t flags, uint32_t *max_level, uint32_t *n_ready_updated);
int hqtick_graph_priorities(hqtick_ctx *ctx, uint64_t n, const uint64_t *task_id, uint64_t *out);

/*
 * Multi-GPU: worker sharding.  Every rank (one ctx per GPU) runs the tick on the SAME snapshot — scans, batches and the
 * placement are replicated and deterministic — but expands and emits records only for the workers it owns:
 *     FxHash(worker_id) % shard_count == shard_index       (FxHash = fxhash 0.2.1 of the u32 id, as tako's Map uses)
 * rec_off[] of the result then holds zero-length ranges for the other workers.  shard_count <= 1 switches sharding off.
 */
int hqtick_set_shard(hqtick_ctx *ctx, uint32_t shard_index, uint32_t shard_count);

/*
 * Record sink in DEVICE memory (for the RCCL all-gather that merges the shards' assignment vectors).  While a sink is set,
 * the records of a tick are written into it instead of host memory (result.rec_task/rec_variant/rec_kind are NULL;
 * result.rec_off stays valid).  Layout, all little-endian, with cap = hqtick_sink_capacity_records(W, capacity_bytes):
 *     u32 header[4] = { n_records, placement_checksum, HQTICK_SINK_MAGIC, cap }
 *         placement_checksum: FNV-1a over the tick's counts (rq, variant, worker, count), multi-node sets and is_optimal — the same on
 *         every rank unless their replicated placements diverged (only a tick that ran into its time limit can do that: its incumbent
 *         depends on the clock); the merging side compares the values and falls back to one rank's placement if they differ.
 *     u32 rec_off[W + 1]        (+ 4 bytes of padding when W is even, so that the next array is 8-byte aligned)
 *     u64 task[cap]   u8 variant[cap]   u8 kind[cap]
 * A tick whose records do not fit returns HQTICK_E_CAPACITY.  device_ptr == NULL removes the sink.
 */
#define HQTICK_SINK_MAGIC 0x48515354u
int hqtick_set_record_sink(hqtick_ctx *ctx, void *device_ptr, size_t capacity_bytes);
size_t hqtick_sink_bytes(uint32_t n_workers, uint32_t capacity_records);
uint32_t hqtick_sink_capacity_records(uint32_t n_workers, size_t capacity_bytes);

/*
 * The merge of the shards inside the boundary: one RCCL all-gather (over xGMI on one node) of every rank's record sink, so that a host
 * that loads this library needs nothing else for the multi-GPU path.  librccl is loaded on first use (dlopen).
 *   hqtick_comm_unique_id   rank 0 creates the 128-byte communicator id; the host carries it to the other ranks by its own means
 *   hqtick_comm_init        every rank, collectively: ncclCommInitRank on the ctx's device; also hqtick_set_shard(rank, world)
 *   hqtick_shard_allgather  after a tick with a record sink set: recv_device (device memory, >= world x sink capacity_bytes) receives the
 *                           sinks of ranks 0..world-1 back to back, each in the layout documented above; returns when the data is there
 *                           (ncclAllGather on the ctx's stream + one synchronisation).  Every rank must use the same capacity_bytes.
 *   hqtick_comm_destroy     ncclCommDestroy (also done by hqtick_destroy)
 */
#define HQTICK_COMM_ID_BYTES 128
/*
 * The placement itself over the ranks (ABI 8; SURVEY.md §8e: the per-worker blocks are independent, what couples them stays replicated).  With
 * shard_count > 1 and an exchange — the library's RCCL communicator (hqtick_comm_init with world == shard_count) or a callback of the host — every rank
 *   * runs only ITS worker range of a coupled tick's price sweeps (k_price_sweep over its share of the master's 16 worker ranges) and completes each sweep
 *     with one small all-gather: per block (c.x, reduced value, bound, steps), per range the wide rows' activities, and the rank's reading of the clock, so
 *     that every replica sees bit-identical cuts and leaves the sweeps at the same sweep; the patterns cross once, when the master asks for them;
 *   * solves only every shard_count-th class block of a separable tick (k_block_solve) and completes the launch with one all-gather of the answers.
 * Results are the unsharded tick's, bit for bit (tests/test_sharded.py, tests/test_gpu_multi.py).  Models under HQTICK_SHARD_MIN_BLOCKS blocks / launches
 * under HQTICK_SHARD_MIN_CLASSES classes (default 1025 both: what one MI355X holds resident at once) are solved whole by every rank, without an exchange;
 * HQTICK_SHARD_SOLVE=0 switches the split off.  EVERY rank must run the same ticks: a rank that stops calling leaves the others in the collective.
 *   hqtick_exchange_fn    all-gather of host memory: this rank contributes bytes_per_rank bytes at `send`; on return `recv` holds shard_count x bytes_per_rank
 *                         bytes, rank-major.  0 = ok.  Called from inside hqtick_run* on the calling thread, a few KB per call.
 *   hqtick_set_exchange   install (fn != NULL) or remove the callback; it takes precedence over the RCCL communicator.  rank / world are those of
 *                         hqtick_set_shard.
 */
typedef int (*hqtick_exchange_fn)(void *user, const void *send, void *recv, size_t bytes_per_rank);
int hqtick_set_exchange(hqtick_ctx *ctx, hqtick_exchange_fn fn, void *user);
int hqtick_comm_unique_id(void *id_out);
int hqtick_comm_init(hqtick_ctx *ctx, const void *id, uint32_t rank, uint32_t world);
int hqtick_shard_allgather(hqtick_ctx *ctx, void *recv_device, size_t recv_bytes);
int hqtick_comm_destroy(hqtick_ctx *ctx);

/* compute_new_worker_query(): batches + solver on fake workers, no mapping  scheduler/query.rs:70-71.  Takes its ready set from the
 * snapshot's task_* columns and runs on a private sub-context: a resident ready set, the last tick's selection (hqtick_ready_consume_last)
 * and the dependency graph of `ctx` are left untouched, so a query may be issued between any two resident ticks. */
int hqtick_query(hqtick_ctx *ctx, const hqtick_snapshot *snapshot, const hqtick_query_workers *fake,
                 hqtick_query_result *out);

/* compute_new_worker_query() on the RESIDENT ready set (ABI 11): what hqtick_query answers, with the ready set taken from HBM instead of the snapshot.
 *   Ready set   the context's resident set (hqtick_upload_ready and the hqtick_ready_* / hqtick_graph_* deltas).  Every other field — resources,
 *               requests, prefill sets — comes from `snapshot`, as for hqtick_run_resident; its task pointers and n_ready are ignored, and so are its
 *               Retracting entries (they sit in the queues, so the resident set already counts them).
 *   Workers     query.rs hands create_task_batches and run_scheduling_solver Some(fake_workers) (batches.rs:80-82, solver.rs:57): the real workers
 *               are not read.  n_workers may be 0, HQ_WORKERS_RESIDENT or a worker list; the answer is the same in all three cases.  (The reference
 *               does read them in one place: the limit of a multi-node batch counts the free real workers (batches.rs:65-78), and where that limit is
 *               not 0 its solver panics on the fake workers' groups (solver.rs:104-106).  It answers only where every such limit is 0 — here it is 0 always.)
 *   Result      `out` exactly as hqtick_query fills it (is_loaded per fake worker, is_optimal; valid until the next call on ctx).  rq_ready (may be
 *               NULL) [snapshot->n_requests]: the live resident tasks of every request, queue.size() of query.rs:97-124 (multi_node_allocations).
 *   Device      one read-only census kernel over the priority and request-id columns (12 B per physical slot, tombstones skipped) on the ctx's
 *               stream, behind every queued delta (beyond the census's caps: the ordered view's radix passes, read-only on the columns too); its level
 *               table and counts go to buffers of the private sub-context that hqtick_query uses,
 *               where batches, model and solve run.  Nothing of ctx changes: columns, group keys, level table, wave table, the selection that
 *               hqtick_ready_consume_last replays, the live count, the graph, the Retracting table.
 *   Errors      HQTICK_E_INVALID without a resident set, and while a selection is pending (a hqtick_run_resident that placed tasks and no
 *               hqtick_ready_consume_last after it: consume first; under HQTICK_FLAG_CONSUME_IN_TICK nothing is pending).  Any number of
 *               distinct priorities: beyond 4096 levels or 16384 (level, request) groups the census gives way to the run table of the ordered view
 *               (DESIGN.md §8f), built on the same sub-context's buffers, as the tick does.
 *   Shards      a replica of hqtick_set_shard answers as a single context would, with no exchange. */
int hqtick_query_resident(hqtick_ctx *ctx, const hqtick_snapshot *snapshot, const hqtick_query_workers *fake,
                          hqtick_query_result *out, uint64_t *rq_ready);

/* Text of the last error on this ctx (never NULL). */
const char *hqtick_last_error(const hqtick_ctx *ctx);

/* Library/ABI version and the gfx arch the kernels were built for ("gfx950"). */
uint32_t hqtick_abi_version(void);
const char *hqtick_build_arch(void);

/*
 * Measurement hooks (used by bench.py; not part of the reference surface).
 * hqtick_kernel_stats(): HIP-event time of the ready-set streaming kernels of the last tick,
 * measured on the ctx's own stream, and the algorithmic bytes they moved.
 */
typedef struct hqtick_kernel_stats {
    double level_hist_us;   /* K1: per-(rq,priority) histogram over the ready set   */
    double select_us;       /* K4: selection + scatter of the taken tasks            */
    double distinct_us;     /* K0: distinct-priority discovery                       */
    double other_us;        /* K5b: per-worker expansion into records               */
    double scan_us;         /* K1b: scan of the per-slice counts                     */
    double sweep_us;        /* K5a: round-robin bit rows                             */
    double tick_gpu_us;     /* first kernel start -> last kernel end                 */
    uint64_t algorithmic_bytes; /* N*20 + W*R*16 + Q*V*R*9 + A*13 + P*12 */
    uint64_t n_assigned, n_prefilled;
    double block_solve_us;  /* k_block_solve: the per-worker-class blocks of the separable placement (one wavefront per class) */
    uint32_t n_classes_device, n_classes_host; /* worker classes solved by k_block_solve / by the host solver in the last tick */
    uint32_t block_steps_max, n_classes;       /* most search steps any class took; worker classes of the separable placement  */
    double solve_classify_us, solve_blocks_us, solve_decode_us; /* host wall clock inside the placement stage: worker classes, block solves
                                                  (launch + wait included), counts into the reference's Map iteration order */
    /* coupled ticks (priority cuts, unsaturated batches): the placement by price sweeps (k_price_sweep, csrc/price.hip) */
    uint32_t price_sweeps, price_rounds;   /* sweeps over all worker blocks / flag configurations of the last tick (0: the host search ran alone)   */
    uint32_t milp_cols, milp_rows;         /* size of the coupled model                                                                              */
    double price_us, price_sweep_us;       /* host wall clock inside the price solve / inside the sweeps (launch -> totals visible in pinned memory) */
    double milp_us, model_us;              /* host wall clock of the whole solve of the coupled model / of building it (solver.rs:95-430)            */
    double solve_pre_us;                   /* ... and of what the placement stage did before it (worker classes, the separable attempt)               */
    /* the guard on k_block_solve's answers: classes of the launch the host solved itself while the kernel ran (HQTICK_BLOCK_VERIFY, default 2 per launch, a window that
     * moves with the tick count) / of those: answers that differed (any: the whole launch is re-solved on the host) / answers thrown out by the per-class checks
     * (fits the rows, no room left for another task) and re-solved on the host */
    uint32_t n_classes_verified, n_classes_mismatch, n_classes_rejected;
    uint32_t n_classes_memo;               /* host class blocks of the last tick answered from the context's table of earlier identical blocks (HQTICK_FLAG_NO_BLOCK_MEMO: 0) */
    /* sharded placement solve (hqtick_set_exchange / hqtick_comm_init): the ranks' exchanges inside the last tick */
    uint32_t exchange_calls;               /* all-gathers of host buffers (one per sharded sweep, one per pattern fetch, one per class-block launch)          */
    uint32_t ready_appends;                /* NOT per tick: hqtick_ready_add* batches of this context that were appended behind the resident columns (fresh ids,
                                            * room at the tail: one kernel) instead of merged into new ones (HQTICK_APPEND=0: never)                       */
    uint64_t exchange_bytes;               /* bytes received by this rank in them                                                                              */
    double exchange_us;                    /* host wall clock inside them                                                                                      */
} hqtick_kernel_stats;
int hqtick_kernel_stats_last(const hqtick_ctx *ctx, hqtick_kernel_stats *out);
/* Switch the per-kernel timing on / off at run time (HQTICK_FLAG_NO_KERNEL_TIMING sets the initial state).  When on, the measured kernels are
 * bracketed by start / stop events AT THE DISPATCH (hipExtLaunchKernel): the duration is the kernel's own, the figure rocprofv3's kernel trace
 * reports, without the latency of markers queued around it.  on = 2: the events go around K1 alone (k_level_hist, the launch that streams the ready
 * set: the kernel the roofline figure is quoted on) — what bench.py's timed region runs with, so that every K1 launch of the run is measured the same
 * way and the live figure and a rocprofv3 kernel trace of the same command describe the same launches.  0 = off; any other value = every measured kernel. */
int hqtick_set_kernel_timing(hqtick_ctx *ctx, int on);
#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* HQTICK_H */

/*
 * hqtick_debug.h — test hooks exported by libhqtick_test.so ONLY (the product library libhqtick.so exports include/hqtick.h and
 * include/hqwire.h and nothing else; the hooks below are compiled under -DHQTICK_TEST_HOOKS, hyperqueue_amd/build.py::build_test).
 *
 * These expose HOST-side building blocks of the tick so they can be unit-tested on a machine without a GPU.
 * They are not part of the reference's surface and are not a CPU path of the tick: hqtick_run() has no CPU
 * implementation and fails with HQTICK_E_NO_DEVICE when no gfx950 device is present — in either library.
 */
#ifndef HQTICK_DEBUG_H
#define HQTICK_DEBUG_H
#include <stdint.h>
#include "hqtick.h"
#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: what this header declares is its whole dynamic symbol table. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* The exact MILP solver standing where the reference calls HiGHS (solver/highs.rs:51-88).  Maximise obj.x,
 * col_kind 0 = nat (0..), 1 = bool (0..=1); row_type 0 = Min (>=), 1 = Max (<=), 2 = Eq.  Returns 1 when a solution
 * was written (0 == the reference's `None`). */
int hqtick_debug_milp_solve(int ncols, const double *obj, const uint8_t *col_kind, int nrows, const uint8_t *row_type,
                            const double *rhs, const int *row_off, const int *row_col, const double *row_coef,
                            double time_limit_s, int canonical, double *x_out, double *obj_out, int *is_optimal,
                            long *nodes_out);

/* Which form of phase A the last tick of ctx took (hqtick_query and hqtick_query_resident run on a private sub-context and are not reported here): 1 = the ordered view of the ready set (more distinct priorities or
 * (level, request) groups than the dense scan holds, or HQTICK_ORDERED_VIEW=1), 0 = the dense scan.  On the view: n_runs = nonempty (request, priority)
 * pairs, n_levels = distinct priorities, order_us = event time of the view's kernels (0 under HQTICK_FLAG_NO_KERNEL_TIMING); all 0 otherwise. */
int hqtick_debug_last_order(const hqtick_ctx *ctx, uint32_t *n_runs, uint32_t *n_levels, double *order_us);

/* What the dense (level, request) scan left in host memory, read back without a copy, a launch or a synchronisation.  GPU only.
 * which = 0: the dense scan of the context's last tick.  which = 1: the census of its last hqtick_query_resident.
 * Returns 1 and fills the outputs if that call ran the dense table, 0 (nothing written) if it took the ordered view or scanned nothing.
 * levels: up to cap_levels values, descending; hist: up to cap_groups counts, index level * Q + rq; either may be NULL.
 * shape[4] (which = 0): waves_per_block, tasks_per_wave, n_waves, 1 if the level table was staged in LDS (or, with at most four levels, travelled in the
 * kernel arguments) and 0 if K1 searched it in HBM; zeros for which = 1. */
int hqtick_debug_last_scan(const hqtick_ctx *ctx, int which, uint32_t *n_levels, uint32_t *n_groups, uint32_t shape[4],
                           uint64_t *levels, uint32_t cap_levels, uint32_t *hist, uint32_t cap_groups);

/* The ordered view (csrc/order.hip) by itself, so that tests can compare ALL of it with a plain sort.  GPU only.  None of the three touches a tick:
 * the view is built on a sub-context of its own, every device array comes back by one copy made here.
 * _order_view builds the view of ctx's resident ready set (its priority and rq columns as they are, tombstones included) for n_requests requests, through the same
 * build_view a tick calls.  counts[4] = n_live, n_runs, n_levels, a mask with bit dg set for every digit that got a radix pass (0-7: bytes of ~priority, 8-11: bytes
 * of rq).  perm[n_live]: the live slots by (rq ascending, priority descending, slot ascending); inv[N] / lrank[N] (N = physical slots; defined at live slots only):
 * position of the slot in perm / number of distinct priorities above the slot's; run_*[n_runs]: one row per nonempty (rq, priority) pair in perm's order — its request, first
 * position in perm, level rank, priority.  cap_slots >= N and cap_runs >= n_runs, else HQTICK_E_CAPACITY (counts are filled all the same); any array may be NULL.
 * Errors are build_view's: a live rq >= n_requests is HQTICK_E_INVALID.  A set without a live slot gives counts of 0 and writes nothing. */
int hqtick_debug_order_view(hqtick_ctx *ctx, uint32_t n_requests, uint32_t counts[4], uint32_t *perm, uint32_t *inv, uint32_t *lrank, uint64_t cap_slots, uint32_t *run_rq,
                            uint32_t *run_start, uint32_t *run_rank, uint64_t *run_prio, uint32_t cap_runs);
/* k_order_select on the view _order_view last built (HQTICK_E_INVALID if ctx's columns were rebuilt since).  rq_sel_base[Q + 1] (0 first, n_sel last, monotone) and
 * q_tnc[Q] (n_workers << 16 | tasks per worker, 0 = off) are the plan; a worker-major destination outside its request's range is refused before the launch.
 * mark_mode 0: select only; 1: consume — RQ_TOMBSTONE at the selected slots, nothing selected; 2: restore — the request ids back, nothing selected; 3: consume and select
 * in one launch.  The marks go to a COPY of the rq column (fresh for modes 0, 1, 3; as the previous call left it for mode 2): the resident column and the live count stay.
 * sel_task[n_sel] / sel_rank[n_sel] are pre-filled with all-ones bytes, so a j the kernel left alone reads 2^64 - 1 / 2^32 - 1; rq_after[N] (may be NULL) = the copy
 * after the launch; err = the kernel's guard word (1: a position outside its request's segment, or a request without runs — that j is not written). */
int hqtick_debug_order_select(hqtick_ctx *ctx, const uint32_t *rq_sel_base, const uint32_t *q_tnc, uint32_t n_sel, int mark_mode, uint64_t *sel_task, uint32_t *sel_rank,
                              uint32_t *rq_after, uint32_t *err);
/* k_order_rank_of on that view: out_rq[k] / out_pos[k] = request and position in perm of want[k]; 2^32 - 1 twice for an id that is absent or tombstoned. */
int hqtick_debug_order_rank_of(hqtick_ctx *ctx, const uint64_t *want, uint32_t n_want, uint32_t *out_rq, uint32_t *out_pos);

/* The HOST stages of a tick — create_task_batches + run_scheduling_solver (scheduler/batches.rs:42-181, scheduler/solver.rs:36-483) — on
 * caller-supplied outputs of the GPU scans, so that this logic can be unit-tested on a machine without a GPU.  This is not a tick: the scans
 * (K0/K1/K2), the selection and the mapping have no CPU implementation, and nothing in the product calls this.
 *   vflags[W * NV], vtmc[W * NV]   what K2 (k_worker_eval) writes per (worker, variant slot): bit 0 fits the free resources now, bit 1 fits the
 *                                  total resources, bit 2 the worker's remaining time covers min_time; task_max_count_for_request
 *   levels[L] (descending), hist[L * Q]   what K0/K1/K1b produce: the distinct priorities of the ready set and the task count per (level, rq)
 * Fills status, is_optimal, is_canonical, the batch arrays and the count arrays of `out` (valid until the next call on this thread). */
int hqtick_debug_host_stages(const hqtick_config *config, const hqtick_snapshot *snapshot, const uint8_t *vflags, const uint32_t *vtmc,
                             uint32_t n_levels, const uint64_t *levels, const uint32_t *hist, hqtick_result *out);

/* The same, and behind the solver the host part of the mapping (csrc/map_core.h: create_task_mapping and process_proactive_filling as index arithmetic, the five
 * stages of the plan).  retracting_key / retracting_rank [snapshot->n_retracting]: what the dense scan reports of every Retracting task — key = level * Q + rq
 * (0xFFFFFFFF: not in the ready set), rank = its position among the tasks of that (level, rq) in ascending id.  Fills, beyond what hqtick_debug_host_stages
 * fills, rec_off, retract_off / retract_task, the redirects with their kinds and new_free; the records stay empty (they are K4's and K5's).  A refusal returns
 * its HQTICK_E_* code and leaves its text in *error (may be NULL; valid until the next call on this thread). */
int hqtick_debug_host_plan(const hqtick_config *config, const hqtick_snapshot *snapshot, const uint8_t *vflags, const uint32_t *vtmc,
                           uint32_t n_levels, const uint64_t *levels, const uint32_t *hist, const uint32_t *retracting_key,
                           const uint32_t *retracting_rank, hqtick_result *out, const char **error);

/* The host stages of hqtick_query (compute_new_worker_query, scheduler/query.rs:12-131) on caller-supplied scan outputs: as above, plus
 * fake_vflags / fake_vtmc [fake->n_workers * NV] = what K2 writes for the fake workers (free == total).  Fills `out` (valid until the next call
 * on this thread). */
int hqtick_debug_host_query(const hqtick_config *config, const hqtick_snapshot *snapshot, const hqtick_query_workers *fake,
                            const uint8_t *vflags, const uint32_t *vtmc, const uint8_t *fake_vflags, const uint32_t *fake_vtmc,
                            uint32_t n_levels, const uint64_t *levels, const uint32_t *hist, hqtick_query_result *out);

/* 1 if the last hqtick_debug_milp_solve on this thread completed its tie-break phase (Result::canonical, milp.h). */
int hqtick_debug_milp_was_canonical(void);
/* block solves of the root's block-hull cut rounds in the last hqtick_debug_milp_solve / _solve_priced call on this thread, and how many of them were on
 * blocks that are not packings (a row other than `<= hi` with hi >= 0 and coefficients >= 0, or a lower bound other than 0) */
void hqtick_debug_milp_last_hull(long *solves, long *nonpacking);

/* Iteration order of a hashbrown Map<WorkerId,_> built by inserting `keys` (distinct u32) in the given order:
 * out_pos[i] = index into `keys` of the i-th element visited (scheduler/mapping.rs:43). */
void hqtick_debug_map_order_u32(const uint32_t *keys, uint32_t n, uint32_t *out_pos);

/* The per-worker-class block solver of the separable placement (csrc/block_core.h = the algorithm of k_block_solve) with the wavefront
 * emulated on the CPU: the 64 lanes of every lane-parallel step run in a loop.  Arguments = the kernel's tables (hqblock::ColTable /
 * ClassTable / Output) as host arrays: the tick's (batch, variant) columns as a CSR of request entries + weight + resource pool sums, per class
 * free[R] / total[R] / eligibility mask; out: x[n_classes * n_cols], status[n_classes] (0 ok, 1 step budget exhausted, 2 block shape not
 * supported), steps[n_classes]. */
int hqtick_debug_block_solve_host(uint32_t n_cols, uint32_t n_resources, const uint32_t *ent_off, const uint32_t *ent_res, const uint8_t *ent_kind,
                                  const uint64_t *ent_amount, const uint32_t *weight, const double *pool, uint32_t n_classes, const uint64_t *free_,
                                  const uint64_t *total, const uint64_t *elig, uint32_t budget, uint32_t *x, uint32_t *status, uint32_t *steps);
/* on != 0: hqtick_debug_host_stages / _host_query (this thread) solve the class blocks of the separable path with that emulation instead
 * of the host MILP solver — the code path of a GPU tick, minus the hardware.  budget = search steps per class (0 keeps the current one). */
void hqtick_debug_set_block_emulation(int on, uint32_t budget);
/* host wall clock of the separable placement's stages in the last hqtick_debug_host_stages call: worker classes, block solves, counts into Map order (us) */
void hqtick_debug_last_stage_us(double *out3);
/* classes the last hqtick_debug_host_stages call solved through the emulation / with the host solver */
void hqtick_debug_last_blocks(uint32_t *n_emulated, uint32_t *n_host);

/* Measurement hooks of the tools under tools/ (round 3: moved here from the product's header; libhqtick_test.so is the same objects + these).  GPU only. */
/* Re-launches one streaming kernel of the last resident tick `iters` times back to back between two HIP events on the ctx's
 * stream and returns the average launch duration (which: 0 = K1 level_hist, 1 = K4 select_scatter).  which = 2: an EMPTY kernel of K1's grid, every launch
 * bracketed by its own dispatch events as in hqtick_set_kernel_timing — what that measure records for a kernel that does nothing.  GPU only. */
int hqtick_time_kernel(hqtick_ctx *ctx, int which, int iters, double *avg_us);
/* Host wall-clock marks (microseconds since the start of the last tick) at the internal stage boundaries of the last tick;
 * returns the number of marks written (bench tooling). */
int hqtick_timeline(const hqtick_ctx *ctx, double *out, int cap);
/* With HQTICK_BLOCK_PROFILE=1 in the environment at hqtick_create: 8 u64 per class of the last k_block_solve launch — 100 MHz timestamps
 * at start / block built / duals / greedy / phase 1 / phase 2 done, then phase-1 steps and dual-pool size.  NULL when off. */
const uint64_t *hqtick_block_profile_last(const hqtick_ctx *ctx, uint32_t *n_classes);


/* The coupled placement by price sweeps (csrc/price.cpp; k_price_sweep's algorithm in csrc/price_core.h) with the wavefront emulated on the CPU.
 * on != 0: hqtick_debug_host_stages (this thread) hands coupled models of at least min_cols columns (0: the default) to the sweeps — the code path
 * of a GPU tick, minus the hardware. */
void hqtick_debug_set_price_emulation(int on, uint32_t min_cols);
/* fault injection into this thread's emulated sweeps: fail_at = 0: the sweeper refuses the model at begin(); k >= 1: its k-th sweep fails; -1: off.  (A rank of a
 * sharded solve whose device fails must still take part in the exchange the others wait in: tests/test_shard_solve.py) */
void hqtick_debug_set_price_fault(int fail_at);
/* The coupled tick's fast path (csrc/milp.cpp, solve(): a large model with the builder's structure hints goes to the sweeps as it is) for this thread:
 * 1 on, 0 off (every model takes the classic path: presolve, components, scaled row copy), -1 the default. */
void hqtick_debug_set_fast_path(int on);
/* The fast path reads the model builder's structure hints (csrc/milp.h: Model::col_group / row_lhs / row_block / col_ub).  Shared lists and row_block rows are
 * always checked against the rows themselves (a wrong hint sends the model down the classic path); on != 0 makes this thread also recompute every hinted column bound
 * from the rows it stands for.  _mismatches: models refused for that reason since the check was switched on. */
void hqtick_debug_check_model_hints(int on);
int hqtick_debug_model_hint_mismatches(void);
/* The builder's equal-block runs (csrc/milp.h: Model::block_runs: consecutive worker blocks that differ in their costs only, built and flattened once per run) for
 * this thread: 1 recorded, 0 not — the model and every table must come out the same byte for byte —, -1 the default (on unless HQMILP_BLOCK_RUNS=0).  While it is 0 or 1
 * the thread's coupled models are also digested (below), and one that is too small for the fast path is flattened all the same, for its digest alone. */
void hqtick_debug_set_block_runs(int on);
/* Of the last coupled model hqtick_debug_host_stages built on this thread while hqtick_debug_set_block_runs was 0 or 1: out[0] = 64-bit FNV-1a over every array of
 * the model, out[1] = the same over what the fast path flattened it into (the problem and its sweep tables; 0: the model did not get there), out[2] = runs the builder
 * recorded, out[3] = blocks covered by the runs that passed the flattener's comparison. */
void hqtick_debug_last_coupled_digest(uint64_t out[4]);
/* The first sweep of a coupled solve (zero prices) launched from inside the flattening, as soon as the block tables are final (csrc/price.h: Sweeper::begin_blocks),
 * for this thread: 1 on, 0 off (the sweeper gets the complete tables, then the first launch), -1 the default (on unless HQPRICE_EARLY_SWEEP=0).  Both orders must
 * give the same tables, cuts and answers in every byte. */
void hqtick_debug_set_early_sweep(int on);
uint32_t hqtick_debug_early_sweeps(void);   /* sweeps launched that way on this thread since the last hqtick_debug_set_early_sweep */
/* The fast path's last step — the certified point against every row and bound of the model — run by the tick while phase C's kernels do, for this
 * thread: 1 on, 0 off (inside the solve, before the decode), -1 the default (the context's own: on unless HQTICK_DEFER_ROW_CHECK=0 at hqtick_create).  Where a discarded
 * phase C would leave a trace (HQTICK_FLAG_CONSUME_IN_TICK, the assignment ledger, a record sink, a shard or exchange, Retracting tasks) a tick never defers.
 * hqtick_debug_host_stages / _host_plan defer only while this is 1, and then run the check right behind the solver.
 * _deferred_row_checks: placements that left the solver with their check pending on this thread since the count was last cleared (clear != 0 clears it).
 * _fail_row_checks(n): the next n deferred checks on this thread return false without looking at the point — the caller must come back with what the same call gives
 * with the fast path off.  Returns how many of the failures armed before were still unused. */
void hqtick_debug_set_defer_row_check(int on);
uint32_t hqtick_debug_deferred_row_checks(int clear);
uint32_t hqtick_debug_fail_row_checks(uint32_t n);
/* on != 0: this thread's fast-path solves keep their first cut; hqtick_debug_first_cut copies up to cap bytes of the last one to out and returns its size —
 * act [K] and part_act [16 * K] as int64, then c.x, the bound and part_cx [16] as f64 (0: no solve got to its first cut). */
void hqtick_debug_capture_first_cut(int on);
uint32_t hqtick_debug_first_cut(unsigned char *out, uint32_t cap);
/* fault injection: on != 0 makes the builder merge its first two runs into one false claim (the flattener must refuse it and flatten those blocks one by one). */
void hqtick_debug_corrupt_block_runs(int on);
/* sweeps over all blocks / flag configurations of the last hqtick_debug_host_stages call (0: the host search ran alone) */
void hqtick_debug_last_price(uint32_t *sweeps, uint32_t *rounds);
/* the multi-node placements of the last hqtick_debug_host_stages call on this thread (the counts carry single-node placements only): returns the number of
 * placed multi-node tasks; task i is of request rq[i] and runs on the worker indices worker[off[i] .. off[i + 1]).  Valid until the next call. */
uint32_t hqtick_debug_last_mn(const uint32_t **rq, const uint32_t **off, const uint32_t **worker);
/* hqtick_debug_milp_solve on a model that carries the builder's structure hints (col_group: block of every column, -1 = a column of the whole model;
 * row_implied: rows implied for integer points by their block's other rows; both may be NULL), with the price sweeps run through the emulated
 * wavefront when use_sweeps != 0.  stats_out (optional, 4 doubles): sweeps, rounds, microseconds inside the price solve, canonical flag. */
int hqtick_debug_milp_solve_priced(int ncols, const double *obj, const uint8_t *col_kind, const int32_t *col_group, int nrows, const uint8_t *row_type,
                                   const uint8_t *row_implied, const double *rhs, const int *row_off, const int *row_col, const double *row_coef,
                                   double time_limit_s, int use_sweeps, uint32_t min_cols, double *x_out, double *obj_out, int *is_optimal, double *stats_out);

/* The wire encoding of include/hqwire.h on HOST memory: the same phase functions the three kernels run (csrc/wire_core.h), executed for
 * thread 0..255 in turn with a loop end standing in for each workgroup barrier.  Same arguments as hqwire_encode_device, all pointers host
 * pointers.  Lets the CPU test suite execute the encoder's logic; it is not a product path (hqwire_encode_device has no CPU fallback). */
struct hqwire_tables;
struct hqwire_records;
struct hqwire_output;
int hqwire_debug_encode_host(const struct hqwire_tables *tables, const struct hqwire_records *records, const struct hqwire_output *out);
/* As above with the emulated threads of every phase run in another sequence (0 ascending, 1 descending, 2 a fixed permutation): the bytes
 * must not depend on it -- a phase that did would be a data race on the GPU. */
int hqwire_debug_encode_host_order(const struct hqwire_tables *tables, const struct hqwire_records *records, const struct hqwire_output *out, int order);
/* The resident attribute table of include/hqwire.h (hqwire_table_*) on HOST memory: the same class on a backend whose buffers are heap blocks and whose
 * launches run the kernels' phase functions (csrc/wire_table_core.h) one emulated thread after the other, in the given order (0, 1 or 2 as above).  Every
 * other hqwire_table_* call then works on the table; its view holds host pointers that hqwire_debug_encode_host accepts. */
struct hqwire_table;
struct hqwire_table_config;
int hqwire_debug_table_create_host(struct hqwire_table **out, const struct hqwire_table_config *cfg, int order);

/* The guard on the class blocks' answers (csrc/host_model.cpp; hqtick_kernel_stats.n_classes_verified / _mismatch / _rejected) under fault injection: `verify` classes
 * of the launch are re-solved by the host (window starting at tick_seq * verify; UINT32_MAX = all), and the emulated blocks corrupt the answer of launch position
 * corrupt_class: mode 1 = one task short (feasible, not maximal), 2 = does not fit the rows, 3 = everything on ONE column, corrupt_fill = column << 16 | count (a count that
 * exactly fills a row every column needs is feasible and maximal, yet not the optimum), 0 = off. */
void hqtick_debug_set_block_guard(uint32_t verify, uint32_t tick_seq, int corrupt_mode, uint32_t corrupt_class, uint32_t corrupt_fill);
void hqtick_debug_last_block_guard(uint32_t *verified, uint32_t *mismatch, uint32_t *rejected);
/* The table of earlier class-block answers (hqtick.h: HQTICK_FLAG_NO_BLOCK_MEMO) for hqtick_debug_host_stages: on = 1 keeps one per thread from call to call,
 * 0 drops it (the default: every block is solved).  _last_block_memo: host blocks of the last call answered from it. */
void hqtick_debug_set_block_memo(int on);
uint32_t hqtick_debug_last_block_memo(void);
/* hqtick_debug_host_stages as ONE RANK of a sharded scheduler (include/hqtick.h: hqtick_set_exchange): the emulated sweeps / class blocks run over this rank's
 * share and are completed through `fn`; min_blocks / min_classes = the thresholds below which every rank solves the whole model.  fn = NULL: off. */
void hqtick_debug_set_exchange(hqtick_exchange_fn fn, void *user, uint32_t rank, uint32_t world, uint32_t min_blocks, uint32_t min_classes);
uint32_t hqtick_debug_last_exchange_calls(void);
/* one exchange of the sharded solve through the library's RCCL communicator (hqtick_comm_init): recv gets world x bytes_per_rank bytes */
int hqtick_debug_exchange(hqtick_ctx *ctx, const void *send, void *recv, size_t bytes_per_rank);

/* Clock mode (hqtick_cluster_set_clock; csrc/clock_core.h).  hqtick_debug_clock_rows runs the phase function of k_clock_rows on the CPU: remaining_out[w] = the
 * canonical remaining lifetime of deadline_ns[w] at now_ns against min_time_ns[0..nv) — sorted_form = 0: the linear fold over the table in the kernel's chunks,
 * 1: the binary search over a sorted copy without duplicates that the host mirror runs.  _clock_deadline / _clock_remaining: now + remaining and deadline - now as
 * the library computes them (saturating, HQ_NO_TIME_LIMIT kept).  _clock_launches: k_clock_rows launches of the context's worker set so far (GPU only). */
int hqtick_debug_clock_rows(uint32_t n, const int64_t *deadline_ns, int64_t now_ns, uint32_t nv, const uint64_t *min_time_ns, int sorted_form, int64_t *remaining_out);
int64_t hqtick_debug_clock_deadline(int64_t now_ns, int64_t remaining_ns);
int64_t hqtick_debug_clock_remaining(int64_t deadline_ns, int64_t now_ns);
uint32_t hqtick_debug_clock_launches(const hqtick_ctx *ctx);

/* The audit of the resident state (hqtick_resident_check; csrc/audit_core.h) on HOST arrays: the same per-item functions the kernels of csrc/audit.hip run, one
 * emulated thread after the other, the threads of every pass in the given order (0 ascending, 1 descending, 2 a fixed permutation) -- the report must not depend
 * on it.  `tables` holds what hqtick.cpp hands the auditor of a context, as host pointers with exactly the lengths named; `have`: bit 0 the ready columns, 1 the
 * graph, 2 the ledger, 3 no placement waits to enter the ledger, 4 prefilled tracking.  kernel_us of the report is 0.  Returns n_failed, or HQTICK_E_INVALID for a
 * NULL argument, an undefined bit or an order outside 0..2.  Not a product path: hqtick_resident_check has no CPU implementation. */
typedef struct hqtick_debug_audit_tables {
    uint32_t have;
    /* ready set: ready_n physical rows; ready_live = the host's count (hqtick_ready_count) */
    uint64_t ready_n, ready_live; const uint64_t *ready_id; const uint32_t *ready_rq;
    /* graph: g_slots slots ever used, g_runs run records, g_edges edge pool entries (g_edge: 2 u32 each), g_free entries on the free stack, g_tasks live tasks (host) */
    uint32_t g_slots, g_runs, g_edges, g_free, g_ht_mask; uint64_t g_tasks;
    const uint64_t *g_id; const uint32_t *g_unfinished, *g_gen, *g_head; const uint64_t *g_ht_key; const uint32_t *g_ht_val, *g_run_next, *g_run_off, *g_run_len, *g_edge;
    /* ledger: table of l_mask + 1 buckets; request tables (Q requests, NV variant slots, entries); W worker rows of R resources; counts [W x l_stride], pf [W x l_pf_stride]
     * (NULL without tracking); multi-node columns; the host's counts */
    uint32_t l_mask, l_Q, l_NV, l_W, l_R, l_stride, l_pf_stride; uint64_t l_n_live, l_mn_live, l_pf_live;
    const uint64_t *l_key; const uint32_t *l_worker, *l_rq; const uint8_t *l_variant;
    const uint32_t *l_rq_off, *l_ventry_off, *l_ent_res, *l_var_nodes; const uint8_t *l_ent_kind; const uint64_t *l_ent_amount;
    const uint32_t *l_wid; const uint64_t *l_total, *l_free; const uint32_t *l_counts, *l_pf; const uint64_t *l_mn_task; const uint8_t *l_mn_root, *l_flags;
    /* Retracting table: r_flags bit 0 in_queue, bit 1 has a redirect (r_target: worker id, r_variant) */
    uint32_t r_n; const uint64_t *r_task; const uint32_t *r_target; const uint8_t *r_variant, *r_flags;
} hqtick_debug_audit_tables;
int hqtick_debug_audit_host(const hqtick_debug_audit_tables *tables, uint32_t parts, int order, hqtick_check_report *out);

/* The grouping of a cancel batch (hqtick_cancel_tasks; csrc/cancel_core.h) on HOST arrays: the phase functions of csrc/cancel.hip's kernels, one emulated thread
 * after the other in the given order (0 ascending, 1 descending with the workgroups descending too, 2 a fixed permutation) -- the lists must not depend on it.
 * route_row [n]: the worker row of every batch position (anything not below W: no message); task_id [n]; worker_id [W]: the ids of the rows.  Out, caller-sized:
 * out_worker [W], out_off [W + 1], out_task [n], of which the first *n_workers (+ 1) / out_off[*n_workers] are written.  Returns the number of ids in the lists,
 * HQTICK_E_INVALID for a NULL argument or an order outside 0..2.  Not a product path. */
int hqtick_debug_cancel_group(uint32_t n, uint32_t W, const uint32_t *route_row, const uint64_t *task_id, const uint32_t *worker_id, int order, uint32_t *n_workers,
                              uint32_t *out_worker, uint32_t *out_off, uint64_t *out_task);

/* The decision rule of hqtick_finish_tasks (csrc/finish_core.h, the function the finish mode of the ledger's release passes calls per position) on HOST arrays,
 * one entry per evaluated position: entry_found (the ledger has an entry for the id), entry_class (0 single-node, 1 multi-node, 2 prefilled), entry_worker_match
 * (the reporter is the entry's worker / root), override_found (the id is in the Retracting table), override_worker_match (the reporter is the worker it is
 * retracting from), earlier_accepted (an earlier position of the batch was accepted for the id).  kind [n]: the HQ_FINISH_* kinds.  Returns n, HQTICK_E_INVALID
 * for a NULL array or a class above 2.  Not a product path. */
int hqtick_debug_finish_kind(uint32_t n, const uint8_t *entry_found, const uint8_t *entry_class, const uint8_t *entry_worker_match, const uint8_t *override_found,
                             const uint8_t *override_worker_match, const uint8_t *earlier_accepted, uint8_t *kind);

/* The decision rule of hqtick_fail_tasks (csrc/fail_core.h, the function the fail mode of the ledger's release passes calls per position) on HOST arrays, one
 * entry per evaluated position: the inputs of hqtick_debug_finish_kind and reporter_none (the position was reported by HQ_NO_WORKER).  kind [n]: the HQ_FAIL_*
 * kinds before the graph step.  Returns n, HQTICK_E_INVALID for a NULL array or a class above 2.  Not a product path. */
int hqtick_debug_fail_kind(uint32_t n, const uint8_t *entry_found, const uint8_t *entry_class, const uint8_t *entry_worker_match, const uint8_t *override_found,
                           const uint8_t *override_worker_match, const uint8_t *reporter_none, const uint8_t *earlier_accepted, uint8_t *kind);

/* The decision rule of hqtick_start_tasks (csrc/start_core.h, the function the claim pass of the ledger's start calls per position and the host calls for the ids of
 * the Retracting table) on HOST arrays, one entry per evaluated position: entry_found, entry_class (0 single-node, 1 multi-node, 2 prefilled), entry_worker_match
 * (the reporter is the entry's worker / root), entry_variant_match (the reported variant is the entry's), entry_run (the entry's running byte), variant_exists (the
 * request of the entry, or of a Retracting task, has the reported variant), override_found (the id is in the Retracting table), override_worker_match (the reporter
 * is the worker it is retracting from), earlier_eligible (an earlier eligible position of the batch claimed the id).  kind [n]: the HQ_START_* kinds.  Returns n,
 * HQTICK_E_INVALID for a NULL array or a class above 2.  Not a product path. */
int hqtick_debug_start_kind(uint32_t n, const uint8_t *entry_found, const uint8_t *entry_class, const uint8_t *entry_worker_match, const uint8_t *entry_variant_match,
                            const uint8_t *entry_run, const uint8_t *variant_exists, const uint8_t *override_found, const uint8_t *override_worker_match,
                            const uint8_t *earlier_eligible, uint8_t *kind);

/* The decision rule of hqtick_reject_tasks (csrc/reject_core.h, the function the claim pass of the ledger's reject calls per position and the host settles the
 * Retracting table's positions with) on HOST arrays, one entry per evaluated position: entry_found, entry_class (0 single-node, 1 multi-node, 2 prefilled),
 * entry_worker_match (the reporter is the entry's worker), entry_variant_match (the rejected variant is the entry's), entry_run (the entry's running byte),
 * variant_none (the position names no variant), variant_exists (the request of the entry, or of a Retracting task, has the named variant), override_found (the id is
 * in the Retracting table), override_worker_match (the reporter is the worker it is retracting from), override_redirect (the table holds a redirect),
 * earlier_eligible (an earlier accepted position of the batch claimed the id), reporter_resident.  kind [n]: the HQ_REJECT_* kinds; blocks [n] (may be NULL): 1 if
 * the position adds its pair to the reporter's blocked set.  Returns n, HQTICK_E_INVALID for a NULL array or a class above 2.  Not a product path. */
int hqtick_debug_reject_kind(uint32_t n, const uint8_t *entry_found, const uint8_t *entry_class, const uint8_t *entry_worker_match, const uint8_t *entry_variant_match,
                             const uint8_t *entry_run, const uint8_t *variant_none, const uint8_t *variant_exists, const uint8_t *override_found,
                             const uint8_t *override_worker_match, const uint8_t *override_redirect, const uint8_t *earlier_eligible, const uint8_t *reporter_resident,
                             uint8_t *kind, uint8_t *blocks);

/* The rule of hqtick_lose_workers (csrc/lose_core.h: the function the gather kernel calls per evicted entry, and the one the host settles the Retracting table's
 * redirect targets with) on HOST arrays, one entry per evicted ledger entry: entry_class (0 single-node, 1 multi-node, 2 prefilled), entry_run (the entry's running
 * byte), redirect_target (the id is in the Retracting table with the lost worker as its redirect target).  kind [n]: the HQ_LOSE_* kinds; running [n] (may be
 * NULL): 1 if the task is one of on_remove_worker's running_tasks.  Returns n, HQTICK_E_INVALID for a NULL array or a class above 2.  Not a product path. */
int hqtick_debug_lose_kind(uint32_t n, const uint8_t *entry_class, const uint8_t *entry_run, const uint8_t *redirect_target, uint8_t *kind, uint8_t *running);

/* The grouping of hqtick_lose_workers (csrc/lose_core.h) on HOST arrays: the evicted entries as the gather leaves them -- task_id [k] strictly ascending with
 * priority, rq, kind and worker_index [k] (the index of the entry's worker in the caller's list, below n_workers) -- through the stable sort of csrc/cancel_core.h
 * and the two phases of the group kernel, one emulated thread after the other in the given order (0 ascending, 1 descending, 2 a fixed permutation): the CSR must
 * not depend on it.  Out, caller-sized: out_off [n_workers + 1], the four columns [k].  Returns k, HQTICK_E_INVALID for a NULL argument, n_workers == 0, an index
 * not below n_workers, ids that do not ascend or an order outside 0..2.  Not a product path. */
int hqtick_debug_lose_group(uint32_t k, uint32_t n_workers, const uint64_t *task_id, const uint64_t *priority, const uint32_t *rq, const uint8_t *kind, const uint32_t *worker_index,
                            int order, uint32_t *out_off, uint64_t *out_task, uint64_t *out_priority, uint32_t *out_rq, uint8_t *out_kind);
#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif

/* hqwire.h -- worker-message wire encoding on the device, part of libhqtick.so.
 *
 * Replaces, for the messages one scheduling tick emits, what the reference does on the host between
 * `WorkerTaskMapping::send_messages` and the socket:
 *   /root/reference/crates/tako/src/internal/scheduler/mapping.rs:259-292   per worker RetractTasks + ComputeTasks, per multi-node task
 *                                                                          a single-task message with its node list
 *   .../server/task.rs:315-445       ComputeTasksBuilder (shared data deduplicated per message, size estimate, 32 MiB cut)
 *   .../messages/worker.rs:27-57,76-88   the serde structs
 *   .../transfer/auth.rs:253-263     bincode DefaultOptions + fixint: little endian, u64 lengths, u32 enum tags, u8 Option tags
 * Input: the tick's records where they already are -- in HBM (the record sink of hqtick_set_record_sink, include/hqtick.h) -- plus a
 * task-attribute table and a configuration table the host keeps resident in HBM (it knows both at submit time).  Output: one byte
 * buffer in HBM holding every message of the tick back to back, and per message slot its byte range; the host (or a NIC) reads ranges,
 * it never touches a task.  Sealing (orion AEAD) and length-delimited framing stay the reference's (network layer, out of scope).
 *
 * Message slots: slot w < n_workers = worker index w (its RetractTasks message, then its ComputeTasks message);
 * slot n_workers + k = multi-node task k (one ComputeTasks message for worker_id[mn_worker[mn_worker_off[k]]], the root).
 *
 * Fragmentation (ABI 2).  ComputeTasksBuilder cuts a worker's message whenever its size estimate passes MAX_TASK_MSG_SIZE = 32 MiB
 * (create_message_on_overflow, task.rs:388-400): the message so far is sent, the configuration index starts afresh.  With
 * hqwire_output.slot_nfrag / frag_end set the device does the same: the ComputeTasks range of a slot then holds slot_nfrag[s] messages back to
 * back, message f ending at frag_end[s * HQWIRE_MAX_FRAGMENTS + f] (absolute offset; message 0 starts at slot_off[2s + 1]), each with its own
 * shared-data list and shared_index numbering.
 *
 * Not covered on the device, reported per slot so the host builds the slot's ComputeTasks messages itself (they are rare).  The slot's
 * RetractTasks message IS emitted in every case — only the ComputeTasks part falls back:
 *   HQWIRE_SLOT_OVERSIZE  more than HQWIRE_MAX_FRAGMENTS messages for one slot (> 512 MiB for one worker in one tick), or an estimate above the
 *                         limit while the caller passed no fragment arrays
 *   HQWIRE_SLOT_TOO_MANY  more than HQWIRE_MAX_RECORDS records for one worker in one tick (device-side dedup table)
 *   HQWIRE_SLOT_UNKNOWN   a record names a task id that is not in the attribute table
 * No CPU implementation behind this entry point: without a gfx950 device it returns HQTICK_E_NO_DEVICE.
 *
 * The resident attribute table (ABI 3).  hqwire_table is the task-attribute table of `hqwire_tables` owned by the library, kept in HBM and changed by
 * the reactor events that feed the other resident structures: on_new_tasks -> hqwire_table_add_tasks; a task finished, failed or cancelled ->
 * hqwire_table_remove_tasks; a lost worker's tasks (what hqtick_cluster_last_requeued reports; increment_instance_id, server/reactor.rs:95,100,119) ->
 * hqwire_table_set_instance with values == NULL; a client's assignment (server/client.rs:53-60) -> the same call with values.  hqwire_table_view hands
 * the encoder a plain hqwire_tables; the encoder does not know the difference.
 *   Dead rows.  A removed row STAYS IN PLACE with its id until the next compaction, so the id column stays ascending and the encoder's row search is
 *   undisturbed; liveness is a bitmap kept outside the view.  Hence A DEAD ID STAYS FINDABLE BY THE ENCODER UNTIL THE NEXT COMPACTION: a record that names
 *   a removed task is encoded with the attributes the task had, not reported HQWIRE_SLOT_UNKNOWN.  A tick never names a finished task, which is what makes
 *   this lazy drop sound.  For records that name live tasks an encode on the view gives the bytes of an encode on a table built from the live tasks alone;
 *   after hqwire_table_compact every array of the view is byte for byte that table.
 *   Compaction runs by itself at the end of a remove that leaves more dead rows than live rows or more dead blob bytes than live blob bytes, and inside
 *   every add that has to merge (below).
 *   Ordering.  Every operation of a table is enqueued on the stream given at hqwire_table_create, and every mutating call returns after that stream has
 *   drained.  An encode enqueued on the table's stream is ordered behind the deltas by the stream itself.  An encode on ANOTHER stream is the caller's to
 *   order: it must have finished before the next mutating call on the table, which may move the arrays of the view and release the old ones.
 *   Calls on one table are not thread safe.  Errors are the negative HQTICK_E_* codes (include/hqtick.h); hqwire_table_last_error has the text.
 */
#ifndef HQWIRE_H
#define HQWIRE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: what this header declares is its whole dynamic symbol table. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define HQWIRE_ABI_VERSION 3u
#define HQWIRE_MAX_RECORDS 2048u                 /* records per worker message handled on the device */
#define HQWIRE_MAX_TASK_MSG_SIZE (32u << 20)     /* MAX_FRAME_SIZE / 4 (crates/tako/src/lib.rs:31, server/task.rs:315) */
#define HQWIRE_MAX_FRAGMENTS 16u                 /* ComputeTasks messages one slot may be cut into on the device */

enum { HQWIRE_SLOT_OK = 0, HQWIRE_SLOT_OVERSIZE = 1, HQWIRE_SLOT_UNKNOWN = 2, HQWIRE_SLOT_TOO_MANY = 3 };
enum { HQWIRE_OK = 0, HQWIRE_CAPACITY = 1 };     /* header[0] */

/* Task attributes (what ComputeTaskSeparateData takes from `Task`, messages/worker.rs:27-39) and the interned
 * `TaskConfiguration`s (server/task.rs:95-101; equal configurations share one index: the builder's `configuration_index` key). */
typedef struct hqwire_tables {
    uint64_t n_tasks;
    const uint64_t *task_id;       /* ascending; job_id << 32 | job_task_id                      */
    const uint32_t *task_rq;       /* ResourceRqId                                               */
    const uint32_t *task_instance; /* InstanceId                                                 */
    const uint64_t *task_priority; /* Task::priority() raw                                       */
    const uint32_t *task_config;   /* index into the configuration table                         */
    const uint8_t *entry_some;     /* 1 = Some(entry)                                            */
    const uint64_t *entry_off;     /* [n_tasks + 1] into entry_blob                              */
    const uint8_t *entry_blob;
    uint32_t n_configs;
    const uint8_t *config_time_some;  /* time_limit: Option<Duration>                            */
    const uint64_t *config_time_secs;
    const uint32_t *config_time_nanos;
    const uint64_t *body_off;      /* [n_configs + 1] into body_blob                             */
    const uint8_t *body_blob;
} hqwire_tables;

/* The tick's mapping (hqtick_result / record sink layout, include/hqtick.h). */
typedef struct hqwire_records {
    uint32_t n_workers;
    uint32_t n_records;          /* rec_off[n_workers] (known on the host: result.rec_off stays valid in sink mode) */
    const uint32_t *worker_id;   /* [n_workers]                                                 */
    const uint32_t *rec_off;     /* [n_workers + 1]                                             */
    const uint64_t *rec_task;
    const uint8_t *rec_variant;
    const uint8_t *rec_kind;     /* HQ_REC_PREFILL = 0 -> variant None, HQ_REC_ASSIGN = 1 -> Some(rec_variant) */
    const uint32_t *retract_off; /* [n_workers + 1] or NULL                                     */
    const uint64_t *retract_task;
    uint32_t n_mn;
    const uint64_t *mn_task;
    const uint32_t *mn_worker_off; /* [n_mn + 1] */
    const uint32_t *mn_worker;     /* worker INDEX, root first */
} hqwire_records;

typedef struct hqwire_output {
    uint8_t *bytes;        /* message bytes, back to back                                                          */
    uint64_t capacity;     /* of `bytes`                                                                           */
    uint64_t *slot_off;    /* [2 * n_slots + 1]: RetractTasks of slot s = [off[2s], off[2s+1]), ComputeTasks = [off[2s+1], off[2s+2]) */
    uint8_t *slot_status;  /* [n_slots] HQWIRE_SLOT_*                                                               */
    uint32_t *header;      /* [4] = { HQWIRE_OK / HQWIRE_CAPACITY, n_slots, total bytes low, total bytes high }     */
    void *scratch;         /* hqwire_scratch_bytes(n_records + n_mn, n_slots); 8-byte aligned                       */
    uint64_t scratch_bytes;
    /* ABI 2: fragmentation.  Both NULL = off (an estimate above the limit then marks the slot HQWIRE_SLOT_OVERSIZE). */
    uint32_t *slot_nfrag;  /* [n_slots] ComputeTasks messages of the slot (0 = none)                                */
    uint64_t *frag_end;    /* [n_slots * HQWIRE_MAX_FRAGMENTS] absolute end offset of message f of slot s           */
    uint64_t msg_size_limit; /* 0 = HQWIRE_MAX_TASK_MSG_SIZE; the builder's estimate limit (tests use small values)  */
} hqwire_output;

uint64_t hqwire_scratch_bytes(uint64_t n_records_incl_mn, uint64_t n_slots);

/* Encodes every message of one tick.  ALL pointers of the three structs are DEVICE pointers (HBM); the three kernels are enqueued on
 * `hip_stream` (a hipStream_t, NULL = the null stream) and the call returns without synchronising: header[0] / slot_status / slot_off are
 * valid once the stream has drained.  On HQWIRE_CAPACITY nothing is written to `bytes` (header[2..3] still hold the size needed).
 * Returns 0, HQTICK_E_INVALID (-1), HQTICK_E_NO_DEVICE (-2) or HQTICK_E_DEVICE (-3) (include/hqtick.h). */
int hqwire_encode_device(const hqwire_tables *tables, const hqwire_records *records, const hqwire_output *out, void *hip_stream);

/* ---- the resident attribute table (ABI 3) ------------------------------------------------------------------------------------------------ */
#define HQWIRE_TABLE_TILE 256u  /* rows per compaction tile (one workgroup) */

typedef struct hqwire_table hqwire_table;

/* Initial allocations, 0 = the default (65536 rows, 1 MiB of entries, 64 configurations, 64 KiB of bodies).  Buffers double when a call needs more;
 * tests use tiny values to reach the growth paths. */
typedef struct hqwire_table_config {
    uint64_t initial_rows;
    uint64_t initial_blob_bytes;
    uint64_t initial_configs;
    uint64_t initial_body_bytes;
} hqwire_table_config;

typedef struct hqwire_table_stats {
    uint64_t live_rows;        /* tasks in the table                                                                  */
    uint64_t physical_rows;    /* rows of the view = live + dead                                                      */
    uint64_t blob_bytes;       /* entry bytes of the view = entry_off[physical_rows]                                  */
    uint64_t dead_blob_bytes;  /* of which belong to dead rows                                                        */
    uint64_t n_configs;
    uint64_t body_bytes;
    uint64_t appends;          /* add_tasks calls that took the append path                                           */
    uint64_t merges;           /* ... the merge path                                                                  */
    uint64_t compactions;      /* forced, automatic and those inside a merge, each counted when it dropped dead rows  */
    uint64_t growths;          /* calls that had to enlarge the row / entry / configuration buffers                   */
    uint64_t hbm_bytes;        /* device memory held now                                                              */
    double last_kernel_us;     /* event time of the last mutating call's device work (0 on the host debug backend)    */
} hqwire_table_stats;

/* cfg may be NULL.  hip_stream: a hipStream_t, NULL = the null stream.  HQTICK_E_NO_DEVICE without a gfx950 device: no CPU path in the product. */
int hqwire_table_create(hqwire_table **out, const hqwire_table_config *cfg, void *hip_stream);
void hqwire_table_destroy(hqwire_table *t);

/* Appends n interned TaskConfigurations (append-only) and returns the index of the first one, or a negative error.  body_off has n + 1 entries into
 * body_blob (any base); time_secs / time_nanos are read where time_some is set. */
int64_t hqwire_table_add_configs(hqwire_table *t, uint32_t n, const uint8_t *time_some, const uint64_t *time_secs, const uint32_t *time_nanos,
                                 const uint64_t *body_off, const uint8_t *body_blob);

/* on_new_tasks.  task_id ascends strictly inside the batch; task_instance == NULL: zeros; entry_some == NULL: every entry is None (entry_off / entry_blob may
 * then be NULL too); entry_off has n + 1 entries into entry_blob (any base).  Returns n.  The batch is refused as a whole (HQTICK_E_INVALID, table unchanged) when
 * the ids do not ascend, an id equals a live row's id, a configuration index is >= the number of configurations, entry_off is not monotone, a row has
 * entry_some == 0 and a non-zero length, an id is reserved (>= 0xFFFFFFFFFFFFFFFE) or the physical row count would reach 0xFFFFFFFF.
 * A batch whose first id lies above every resident id (dead rows included) is appended behind the columns; any other batch is merged: dead rows are dropped
 * first, then the two sorted tables are merged into the second set of buffers.  A merged id whose row is dead is accepted: the new attributes stand. */
int64_t hqwire_table_add_tasks(hqwire_table *t, uint64_t n, const uint64_t *task_id, const uint32_t *task_rq, const uint32_t *task_instance,
                               const uint64_t *task_priority, const uint32_t *task_config, const uint8_t *entry_some, const uint64_t *entry_off,
                               const uint8_t *entry_blob);

/* Finished, failed and cancelled tasks.  Returns the number of live rows removed; ids that are unknown, already removed or repeated inside the batch
 * change nothing and are counted in hqwire_table_last_unknown. */
int64_t hqwire_table_remove_tasks(hqwire_table *t, uint64_t n, const uint64_t *task_id);

/* values == NULL: instance id + 1 for every listed id, an id listed twice rising by two.  With values: task_instance = values[i]; an id listed twice
 * with different values keeps either.  Returns the number of live rows found; unknown and dead ids are counted in hqwire_table_last_unknown. */
int64_t hqwire_table_set_instance(hqwire_table *t, uint64_t n, const uint64_t *task_id, const uint32_t *values);

/* Drops the dead rows now (nothing happens without any). */
int hqwire_table_compact(hqwire_table *t);

/* DEVICE pointers and counts to hand to hqwire_encode_device; valid until the next mutating call on the table.  Launches nothing, waits for nothing. */
int hqwire_table_view(const hqwire_table *t, hqwire_tables *out);

/* The arrays of the view copied to HOST buffers the caller sized from hqwire_table_get_stats (physical_rows rows, physical_rows + 1 offsets, blob_bytes,
 * n_configs, n_configs + 1 offsets, body_bytes); n_tasks and n_configs are filled in.  NULL pointers are skipped.  Tests, journalling, restore. */
int hqwire_table_copy_out(const hqwire_table *t, hqwire_tables *host);

int hqwire_table_get_stats(const hqwire_table *t, hqwire_table_stats *out);
uint64_t hqwire_table_last_unknown(const hqwire_table *t);
const char *hqwire_table_last_error(const hqwire_table *t);

uint32_t hqwire_abi_version(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif

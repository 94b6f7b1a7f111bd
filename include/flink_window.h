/*
 * flink_window.h — C-ABI of the MI355X keyed event-time window operator ("fw_").
 *
 * Drop-in boundary for Flink's WindowOperator + heap keyed state backend + event-time
 * timer service (paths relative to /root/reference/flink-streaming-java/src/main/java/
 * org/apache/flink/streaming/ unless they start with flink-*).  Plain pointers and sizes,
 * no C++ or torch types; every call returns an int status (FW_OK = 0, < 0 error) and
 * fw_last_error() gives the message (the Java shim throws IOException(message), as
 * HeapAggregatingState.java:90-92 wraps state errors).  Calls on one handle are serialised
 * by the caller (one handle per subtask, as one task thread owns one operator:
 * runtime/io/StreamInputProcessor.java:211-222); handles on different GPUs may be driven
 * concurrently.
 *
 * Micro-batch contract: records handed to one fw_push_* call are processed against the
 * current watermark exactly as WindowOperator.processElement would process them one by one
 * (WindowOperator.java:291-421); fw_advance_watermark is processWatermark
 * (api/operators/AbstractStreamOperator.java:735-740 -> HeapInternalTimerService.java:276-290).
 * The host therefore cuts batches at watermarks.
 */
#ifndef FLINK_WINDOW_H
#define FLINK_WINDOW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---- */
#define FW_OK 0
#define FW_ERR_ARG (-1)          /* invalid argument (IllegalArgumentException in the reference) */
#define FW_ERR_HIP (-2)          /* HIP runtime failure */
#define FW_ERR_NO_TIMESTAMP (-3) /* Long.MIN_VALUE timestamp: TumblingEventTimeWindows.java:69-71 */
#define FW_ERR_KEY_GROUP (-4)    /* key outside the handle's KeyGroupRange (KeyGroupRangeOffsets / StateTable) */
#define FW_ERR_CAPACITY (-5)     /* state could not be stored (HBM exhausted) */
#define FW_ERR_UNSUPPORTED (-6)  /* configuration not offered on the GPU path */
#define FW_ERR_STATE (-7)        /* corrupted / inconsistent handle state */
#define FW_ERR_DISPLACED (-8)    /* sliding windows kept as panes: the push holds a record with ts - offset + slide < 0
                                    off the slide grid, to which the reference assigns size / slide + 1 windows
                                    (Java's truncating % in TimeWindow.getWindowStartWithOffset).  The whole push is
                                    refused and nothing changed; fw_config::no_panes keeps windows, which take it */
#define FW_ERR_TIME_RANGE (-9)   /* a timestamp at an end of the long range that the operator does not take.  Timestamps
                                    and window bounds are Java longs and wrap as the reference's do; refused are
                                    (a) by every sliding operator, a timestamp just above Long.MIN_VALUE + size on
                                    which SlidingEventTimeWindows.assignWindows' walk wraps below Long.MIN_VALUE (the
                                    reference itself does not return on it); (b) by sliding windows kept as panes, a
                                    record whose window end wraps past Long.MAX_VALUE or that lies within
                                    size + 2 slide of Long.MIN_VALUE (fw_config::no_panes takes them); (c) by sliding
                                    t-digest windows, a record with several windows of which one's end wraps; (d) by
                                    fw_combine_extract_device of a tumbling combiner, every extraction once the
                                    combiner took a record at or above its window's end (the end, or
                                    ts - offset + size, wrapped).  Host columns, and every push of the window-contents (list)
                                    operator: the whole push is refused and nothing changed.  Device columns of
                                    fw_push_batch_device: those records are left out, the others taken, and the next
                                    call that ends by settling the operator (fw_synchronize, fw_advance_watermark with
                                    a count, fw_pending, a drain, ...) returns the code once, for every push since
                                    the last report; a push queued behind a refused one is taken in full.  The operator goes on */

/* ---- assigner, value and key kinds ---- */
#define FW_TUMBLING 0 /* api/windowing/assigners/TumblingEventTimeWindows.java:53-73 */
#define FW_SLIDING 1  /* api/windowing/assigners/SlidingEventTimeWindows.java:57-81   */
#define FW_SESSION 2  /* api/windowing/assigners/EventTimeSessionWindows.java:59-61  */
#define FW_COUNT 3    /* count windows: KeyedStream.countWindow(size, slide) = GlobalWindows + CountTrigger.of(slide) +
                         CountEvictor.of(size) (api/datastream/KeyedStream.java:383-397; EvictingWindowOperator.java
                         :102-239,334-366; CountTrigger.java:47-55; CountEvictor.java:63-78), and countWindow(size) =
                         PurgingTrigger.of(CountTrigger.of(size)) with slide = size.  Every slide-th element of a key
                         fires the key's last min(size, elements) elements, reduced in arrival order, while the
                         element is processed (no timers; watermarks only delimit the output).  Rows: start =
                         Long.MIN_VALUE, end = Long.MAX_VALUE (GlobalWindow, timestamp Long.MAX_VALUE), count, sum,
                         min, and max = the arrival ordinal of the window's first element (the passthrough fields of
                         sum(pos)); aggregate must be FW_AGG_FIRST.  expected_entries bounds the distinct keys. */

#define FW_VAL_I64 0 /* Long field: sum wraps at 64 bits (SumFunction.LongSum)            */
#define FW_VAL_I32 1 /* Integer field: sum wraps at 32 bits (SumFunction.IntSum)          */
#define FW_VAL_F64 2 /* Double field: min/max by Double.compare, sum within 1e-6 relative */
#define FW_VAL_I16 3 /* Short field: sum wraps at 16 bits (SumFunction.ShortSum); values sign-extended */
#define FW_VAL_I8 4  /* Byte field: sum wraps at 8 bits (SumFunction.ByteSum); values sign-extended   */
#define FW_VAL_F32 5 /* Float field passed as the double of the float: min/max by Float.compare, sum
                        rounded to float (SumFunction.FloatSum adds in float: within 1e-5 relative)  */

/* the AggregateFunction (fw_config.aggregate) */
#define FW_AGG_COUNT_SUM_MIN_MAX 0 /* built-in {count, sum, min, max} accumulator                        */
#define FW_AGG_HLL 1               /* HyperLogLog distinct count of the value column read as a u64 item
                                      (definition in DESIGN.md §HLL): fired rows carry
                                      count, sum = estimate (f64 bits), min = zero registers, max = the
                                      low 64 bits of sum_j 2^(65-p-M[j]); the accumulator is the registers
                                      and the count (a snapshot row's sum / min / max are 0 / Long.MAX_VALUE
                                      / Long.MIN_VALUE, not value statistics).  Tumbling and sliding windows
                                      (one register block per window), any allowed lateness (a window fires
                                      at maxTimestamp and keeps its registers until its cleanup time), and
                                      session windows (merged sessions take the register max of their blocks,
                                      AbstractHeapMergingState.mergeNamespaces; not with PurgingTrigger:
                                      FW_ERR_UNSUPPORTED); expected_entries sizes the register pool
                                      (2^p B/entry). */
#define FW_AGG_FIRST 2             /* the reduce aggregations sum(pos) / min(pos) of DataStream / WindowedStream
                                      (SumAggregator.java:66-76, ComparableAggregator.java:72-94 over
                                      HeapReducingState.add, HeapReducingState.java:72-84): the result is a
                                      copy of the FIRST element of the window with the field replaced.  Rows
                                      carry count, sum, min as usual and max = the arrival ordinal of that
                                      first element (0-based index of the record among all records pushed
                                      into the handle), from which the caller takes the passthrough fields.
                                      Merged sessions keep the smaller ordinal.  At most 65535 windows per
                                      record. */
#define FW_AGG_MINBY 3             /* minBy(pos) / maxBy(pos) with the first-tie rule (ComparableAggregator.java
                                      :72-94, Comparator.java MinBy/MaxBy): the whole element with the smallest
                                      (largest) field, the earlier one among equal fields; Integer, Long or
                                      Double (Double.compare order) fields.  Rows carry count, sum, min = the
                                      selected field value and max = the arrival ordinal of the selected element
                                      (exact: (field, ordinal) pairs compare in full).  Sliding windows keep
                                      panes like the other aggregates: a window's element is the smallest
                                      (field, ordinal) pair over its panes. */
#define FW_AGG_MAXBY 4
#define FW_AGG_TDIGEST 6           /* t-digest quantiles of a Double field (definition in DESIGN.md
                                      §t-digest and oracle/window_oracle.h): a merging t-digest with the k1 scale
                                      function, compression tdigest_compression (delta), at most delta/2
                                      centroids; add buffers, and every push compresses the values it added.
                                      Rows carry count = elements and sum / min / max = the estimated quantiles
                                      tdigest_quantiles[0..2] (f64 bits).  Tumbling and sliding windows (one
                                      digest per window; allowed lateness without PurgingTrigger: a late firing
                                      reports the digest with the push's values so far) and session windows
                                      (merged sessions' digests merge: the union of their centroids, compressed
                                      with the push's values; AbstractHeapMergingState.mergeNamespaces; with
                                      allowed lateness, no PurgingTrigger), FW_VAL_F64; expected_entries sizes
                                      the digest pool.  Keyed-state snapshots
                                      carry the digest as an accumulator block (fw_snapshot_key_group_blocks). */
#define FW_AGG_FIRST_MAX 5         /* max(pos) (ComparableAggregator.java:72-94, Comparator.MaxComparator): as
                                      FW_AGG_FIRST, but the min column holds the field's MAXIMUM (the first
                                      element with the field replaced by the max) */

#define FW_AGG_ROW 7               /* the Table API's group-window aggregation (flink-libraries/flink-table
                                      DataStreamGroupWindowAggregate.scala:197-294 -> WindowedStream.aggregate of
                                      one accumulator Row): several built-in aggregates over up to 8 nullable value
                                      columns (row_columns, row_column_type[], row_aggregate[] = FW_ROW_* << 8 |
                                      column), pushed with fw_push_row_batch(_device).  Semantics of the Table
                                      functions (.../table/functions/aggfunctions/ *AggFunction.scala; oracle/window_oracle.h
                                      OR_AGG_ROW): COUNT(col) counts non-null values; SUM / MIN / MAX / AVG are
                                      NULL when the column had none; integral SUM wraps to the column's width;
                                      integral AVG = the Long sum / count (Java division; Long: the exact sum)
                                      narrowed to the type; Double / Float AVG = the double sum / count.  Tumbling,
                                      sliding and session windows (merged sessions merge every aggregate), allowed
                                      lateness 0, EventTimeTrigger, no side output (the Table planner sets none).
                                      Rows carry count = COUNT(*) (sum / min / max 0); fw_drain_row_results gives
                                      each row's aggregates and their NULL mask.  Keyed-state snapshots carry the
                                      accumulator as a block (fw_snapshot_key_group_blocks): per column its
                                      non-null count, the sum's low and high words (floating: the f64 sum, 0),
                                      min and max (the column's value; 0 when the count is 0), int64 each. */
#define FW_ROW_COUNT_STAR 0 /* COUNT(*) / COUNT(1): every record (CountAggFunction.accumulate(acc))           */
#define FW_ROW_COUNT 1      /* COUNT(col): the non-null values (CountAggFunction.scala:51-55)                   */
#define FW_ROW_SUM 2        /* SUM(col) (SumAggFunction.scala)                                                  */
#define FW_ROW_MIN 3        /* MIN(col) (MinAggFunction.scala; Double / Float by their compare)                 */
#define FW_ROW_MAX 4        /* MAX(col) (MaxAggFunction.scala)                                                  */
#define FW_ROW_AVG 5        /* AVG(col) (AvgAggFunction.scala: Integral / BigIntegral / Floating)               */

#define FW_KEY_LONG 0   /* key is a Long: hashCode = (int)(v ^ (v >>> 32))               */
#define FW_KEY_INT 1    /* key is an Integer: hashCode = value                              */
#define FW_KEY_HASHED 2 /* caller passes key.hashCode() per record (String, Tuple, POJO);
                           the i64 key column is then the caller's dictionary id of the key */

/* Operator configuration: the arguments of the WindowOperator constructor
 * (runtime/operators/windowing/WindowOperator.java:179-212) restricted to the GPU-eligible
 * shapes (event-time assigner above, EventTimeTrigger or PurgingTrigger.of(EventTimeTrigger),
 * AggregatingStateDescriptor/ReducingStateDescriptor with the built-in count/sum/min/max
 * accumulator), plus the keyed-backend arguments of
 * flink-runtime/.../state/StateBackend.java:130 (numberOfKeyGroups, keyGroupRange). */
typedef struct fw_config {
  int32_t assigner;            /* FW_TUMBLING / FW_SLIDING / FW_SESSION                      */
  int32_t value_type;          /* FW_VAL_*                                                   */
  int32_t key_kind;            /* FW_KEY_*                                                   */
  int32_t purging;             /* 1 = PurgingTrigger.of(EventTimeTrigger.create())           */
  int32_t side_output;         /* 1 = late records go to the side output (lateDataOutputTag) */
  int32_t max_parallelism;     /* number of key groups (0 -> 128, ExecutionJobVertex.java:176) */
  int32_t key_group_start;     /* KeyGroupRange owned by this handle, inclusive             */
  int32_t key_group_end;       /*   (-1/-1 -> the whole range [0, max_parallelism-1])        */
  int32_t device;              /* HIP device ordinal                                         */
  int32_t sub_partitions;      /* state partitions per key group, power of two (0 = auto)   */
  int64_t size;                /* window size (tumbling, sliding)                            */
  int64_t slide;               /* slide (sliding)                                            */
  int64_t offset;              /* window offset (tumbling, sliding)                          */
  int64_t gap;                 /* session gap (session)                                      */
  int64_t allowed_lateness;    /* WindowedStream.allowedLateness, >= 0                       */
  int64_t expected_entries;    /* sizing hint: live (key, window) pairs (0 = default)        */
  int64_t max_batch;           /* largest n passed to one push (0 = 1 << 24)                */
  int32_t aggregate;           /* FW_AGG_* (0 = count/sum/min/max)                           */
  int32_t hll_precision;       /* FW_AGG_HLL: p in [4, 16], m = 2^p registers (0 -> 14)       */
  int32_t tdigest_compression; /* FW_AGG_TDIGEST: delta, even, in [10, 500] (0 -> 100)         */
  int32_t tdigest_export;      /* FW_AGG_TDIGEST: 1 = fired rows also keep their centroids for
                                  fw_drain_digests                                             */
  double tdigest_quantiles[3]; /* FW_AGG_TDIGEST: the quantiles of a row (all 0 -> .5 .95 .99) */
  int32_t count_evict_after;   /* FW_COUNT: 1 = CountEvictor.of(size, true): evict after the window function
                                  (the fired window is the last min(elements, size + slide)) */
  int32_t pad0;
  int32_t row_columns;         /* FW_AGG_ROW: value columns per record, 1 .. 8                   */
  int32_t row_aggregates;      /* FW_AGG_ROW: aggregates of a row, 1 .. 16                       */
  int32_t row_column_type[8];  /* FW_AGG_ROW: FW_VAL_* of each column                            */
  int32_t row_aggregate[16];   /* FW_AGG_ROW: FW_ROW_* << 8 | column                             */
  int32_t no_panes;            /* FW_SLIDING: 1 = keep windows, not panes, also where size % slide == 0 and the
                                  lateness is 0.  Panes refuse a displaced record (a pre-epoch timestamp with
                                  ts - offset + slide < 0 off the slide grid, which the reference assigns
                                  size / slide + 1 windows; FW_ERR_DISPLACED); windows take it exactly.  Appended:
                                  no earlier offset moved */
  int32_t trigger;             /* FW_TRIGGER_EVENT_TIME (0, a zeroed field: EventTimeTrigger.java:37-73, the window's
                                  default trigger) or FW_TRIGGER_CONTINUOUS_EVENT_TIME: the trigger argument of the
                                  WindowOperator constructor (WindowOperator.java:179-212) set by
                                  WindowedStream.trigger(ContinuousEventTimeTrigger.of(interval)); `purging` wraps
                                  either in PurgingTrigger.  The constants are the list operator's, below.  (In the
                                  former pad1 slot: no offset moved.) */
  int64_t trigger_interval;    /* FW_TRIGGER_CONTINUOUS_EVENT_TIME: ContinuousEventTimeTrigger's interval in ms
                                  (ContinuousEventTimeTrigger.java:42-50), > 0 (FW_ERR_ARG).  Appended. */
} fw_config;

/* ContinuousEventTimeTrigger on the aggregating operator (early firings: a window emits its running aggregate every
 * `interval` of event time, ContinuousEventTimeTrigger.java:39-151).  Offered for FW_AGG_COUNT_SUM_MIN_MAX over every
 * value type and key kind, FW_TUMBLING and FW_SLIDING, with allowed lateness, purging and side output, host and
 * device pushes.  Such a handle keeps windows: no panes, dense regions, compact records or single pass.
 *   Refused by fw_create (FW_ERR_UNSUPPORTED, before the GPU is touched): FW_SESSION (a merged session's fire time is
 *   the minimum over its founders in arrival order: fw_list_create takes sessions under this trigger), FW_COUNT,
 *   every other aggregate (the window-contents operator, fw_list_create, runs any function under this trigger), and
 *   size + allowed_lateness + 2 * trigger_interval > 2^60 (the fire time rides in the entry as an offset from the
 *   window's start).
 *   fw_advance_watermark refuses an advance over which one window would fire more than 2^20 times
 *   (FW_ERR_UNSUPPORTED, "2^20 trigger intervals"; nothing changed: advance in smaller steps).
 *   A record with ts > Long.MAX_VALUE - interval (its first fire time ts - ts % interval + interval, or the timer
 *   after it, wraps past Long.MAX_VALUE) is refused with FW_ERR_TIME_RANGE as the other timestamps at the ends of the long range are (host columns: the whole push, state
 *   untouched; device columns: the record is left out and the settling call reports it).
 *   The pre-shuffle combiner entry points refuse the handle (a combiner's partials carry no arrival order), and
 *   fw_snapshot_key_group / fw_restore_key_group point to fw_snapshot_key_group_fire / fw_restore_key_group_fire.
 *   fw_stats: keyed_state_entries counts the windows with contents (a purged window keeps its trigger state until its
 *   cleanup time), event_time_timers the timers at maxTimestamp, at the fire time and at the cleanup time, coinciding
 *   times once (HeapInternalTimerService keeps a set). */

typedef struct fw_op fw_op;

/* Fired window rows (struct of arrays).  One row per emitted window result:
 * the built-in AggregateFunction.getResult {count, sum, min, max} plus the key and the
 * TimeWindow; the record timestamp of the row is end - 1 = TimeWindow.maxTimestamp()
 * (TimestampedCollector.setAbsoluteTimestamp, WindowOperator.java:544-548).  For
 * FW_VAL_F64 / FW_VAL_F32, sum/min/max hold IEEE-754 double bit patterns. */
typedef struct fw_rows {
  int64_t* key;
  int64_t* start;
  int64_t* end;
  int64_t* count;
  int64_t* sum;
  int64_t* min;
  int64_t* max;
} fw_rows;

/* Late records routed to the side output (WindowOperator.sideOutput, :556-558). */
typedef struct fw_side_rows {
  int64_t* key;
  int64_t* ts;
  int64_t* val;
} fw_side_rows;

typedef struct fw_stats {
  int64_t records_in;             /* numRecordsIn                                            */
  int64_t late_records_dropped;   /* numLateRecordsDropped (WindowOperator.java:138-140,418) */
  int64_t keyed_state_entries;    /* numKeyedStateEntries of "window-contents"               */
  int64_t event_time_timers;      /* numEventTimeTimers                                      */
  int64_t current_watermark;      /* InternalTimerService.currentWatermark()                 */
  int64_t fired_rows_total;       /* all rows emitted since creation                         */
  int64_t pending_rows;           /* rows emitted and not yet drained                        */
  int64_t pending_side_rows;      /* side-output rows not yet drained                        */
  int64_t table_capacity;         /* slots in the HBM state table                            */
  int64_t table_grows;            /* times the table was resized                             */
  int64_t slow_path_records;      /* records replayed in arrival order (late firing / drop)  */
  int64_t state_merges;           /* pre-aggregated (key, window) deltas merged into HBM       */
  int64_t digest_centroids_fired; /* FW_AGG_TDIGEST: centroids of all digests fired so far      */
  int64_t single_pass_batches;    /* device batches partitioned in one pass (dense tumbling)    */
  int64_t single_pass_redone;     /* ... of which went through classify / scan / scatter after  */
  int64_t narrow_pass_batches;    /* ... of which wrote 8-byte records (key, window, int32 value) */
  int64_t narrow_pass_redone;     /* ... of which had a record without that form (then 16 bytes) */
  int64_t push_resumptions;       /* suspended sequences resumed after the host grew the table / row buffer */
} fw_stats;

/* Lifecycle — StreamOperator.setup/open/close/dispose (api/operators/StreamOperator.java:57-127). */
int fw_create(const fw_config* cfg, fw_op** out);
void fw_destroy(fw_op* op);
const char* fw_last_error(const fw_op* op);

/* processElement for a micro-batch (WindowOperator.java:291-421).
 *   fw_push_batch:        host buffers (a Java DirectByteBuffer in native byte order); the
 *                         batch is processed completely before the call returns, and errors
 *                         (FW_ERR_KEY_GROUP, FW_ERR_NO_TIMESTAMP, ...) are returned by it.
 *   fw_push_batch_device: device pointers already resident in HBM on the handle's device;
 *                         enqueued on the handle's stream and returns without waiting.  The
 *                         buffers must stay valid until the stream has passed the push (the
 *                         next fw_* call that returns a count, or fw_synchronize).  Errors the
 *                         batch raised are returned by that next call.
 * The state table grows on demand: a kernel that finds a region (or the fired-row buffer) short
 * of room stops before changing anything it could not keep, and the next synchronising call
 * grows the table and resumes it where it stopped, so no batch size is too large for the state.
 * key_hash may be NULL unless key_kind == FW_KEY_HASHED.  val points to n int64 (FW_VAL_I64 /
 * FW_VAL_I32, the latter already sign-extended) or n doubles (FW_VAL_F64). */
int fw_push_batch(fw_op* op, const int64_t* key, const int64_t* ts, const void* val, const int32_t* key_hash,
                  int64_t n);
int fw_push_batch_device(fw_op* op, const int64_t* key, const int64_t* ts, const void* val, const int32_t* key_hash,
                         int64_t n);

/* processWatermark: fires every (key, window) whose event-time timer is <= wm, clears state
 * whose cleanup time (maxTimestamp + allowedLateness, WindowOperator.java:637-644) is <= wm,
 * and returns the number of rows now pending (emitted since the last drain, including
 * late firings emitted while processing elements).  Rows pending at this point all precede
 * the watermark in the operator's output (AbstractStreamOperator.java:735-740). */
int fw_advance_watermark(fw_op* op, int64_t wm, int64_t* n_pending_rows);

/* Pending output.  *_host copy into caller-owned arrays of capacity cap and clear the pending
 * set (fw_drain_rows: host or device memory, a NULL column is skipped); fw_rows_device exposes the pending rows in HBM without copying (valid until the
 * next fw_* call) and fw_clear_pending drops them.  Each of these first settles an unsettled
 * device push. */
int fw_pending(fw_op* op, int64_t* n_rows, int64_t* n_side_rows);
int fw_drain_rows(fw_op* op, const fw_rows* host_dst, int64_t cap, int64_t* n);
int fw_drain_side(fw_op* op, const fw_side_rows* host_dst, int64_t cap, int64_t* n);
int fw_rows_device(fw_op* op, fw_rows* dev_view, int64_t* n);
/* FW_AGG_TDIGEST with tdigest_export: the centroids of the pending rows (the AggregateFunction's accumulator at
 * getResult), without draining them: for pending row i, n_centroids[i] and the centroids' sums (f64) and
 * weights at [i * delta/2 + k], k < n_centroids[i].  Call before fw_drain_rows. */
int fw_drain_digests(fw_op* op, int64_t* n_centroids, double* sum, int64_t* weight, int64_t cap_rows, int64_t* n);
int fw_clear_pending(fw_op* op);
/* FW_AGG_ROW: processElement for n records of the Table API's input rows (DataStreamGroupWindowAggregate's
 * WindowedStream.aggregate): row_columns value columns, column-major (cols + j * n = column j: int64 values
 * sign-extended, Double / Float as f64 bits), and per record a NULL mask (bit j = column j is NULL; nulls = NULL:
 * no NULLs).  Host buffers (processed before return) or HBM (_device, stream-ordered as fw_push_batch_device). */
int fw_push_row_batch(fw_op* op, const int64_t* key, const int64_t* ts, const int64_t* cols, const uint8_t* nulls,
                      const int32_t* key_hash, int64_t n);
int fw_push_row_batch_device(fw_op* op, const int64_t* key, const int64_t* ts, const int64_t* cols,
                             const uint8_t* nulls, const int32_t* key_hash, int64_t n);
/* FW_AGG_ROW: the aggregates of the pending rows (the generated AggregateFunction's getValue per aggregate:
 * values[i * row_aggregates + s], integers sign-extended, floating results as f64 bits, a Float result as the
 * double of the float) and null_mask[i] (bit s = aggregate s is NULL), without draining them: call before
 * fw_drain_rows.  Either output may be NULL. */
int fw_drain_row_results(fw_op* op, int64_t* values, uint32_t* null_mask, int64_t cap_rows, int64_t* n);

int fw_get_stats(fw_op* op, fw_stats* out);

/* Per-kernel timing with HIP events recorded around every launch on the handle's stream
 * (rocprofv3 --kernel-trace measures the same launches from outside).  Kernel kinds, in order:
 * classify_hist, scan, scatter, aggregate, slow, fire, tdigest (the t-digest compression of a push).  fw_profile_read returns accumulated
 * milliseconds and launch counts per kind (arrays of FW_NUM_KERNELS) and optionally resets them.
 * enable: 0 = off, 1 = every kind, FW_PROFILE_KINDS | (1 << kind) | ... = only those kinds (each timed launch
 * adds two event markers to its stream, so a measurement that needs one kernel's duration times only that one).
 * A handle of fw_create_count_trigger has no aggregate or ordered path of that form: it reports its slot lookup under
 * k_aggregate and its sort, scan and fold under k_slow; classify_hist, scan and scatter stay 0. */
#define FW_NUM_KERNELS 7
#define FW_PROFILE_KINDS 0x100
int fw_profile(fw_op* op, int enable);
int fw_profile_read(fw_op* op, double* ms, int64_t* launches, int reset);
const char* fw_kernel_name(int kind);
/* wait for every queued push / watermark and return the error any of them raised */
int fw_synchronize(fw_op* op);
void* fw_stream(fw_op* op); /* the hipStream_t the handle enqueues on */
/* Async input (StreamInputProcessor hands the next buffer over while the operator still works on the previous
 * one, StreamInputProcessor.java:211-223).  Enabled, fw_push_batch_device reads its columns on
 * fw_input_stream(op) — the caller orders the columns' producer before that stream (not before fw_stream) —
 * and the batch's partitioning kernels run there, beside the previous batch's aggregation and firing on
 * fw_stream.  Disabled (the default), or with side output or count windows, fw_input_stream(op) ==
 * fw_stream(op).  fw_keyby_push_device reads its columns and runs its exchange on fw_input_stream(op) too; host
 * pushes read theirs in fw_stream order. */
int fw_set_async_input(fw_op* op, int enable);
void* fw_input_stream(fw_op* op);

/* Pre-shuffle combining for the keyBy exchange: partial accumulators instead of records cross the
 * network when the aggregate is decomposable (AggregateFunction.merge, flink-core/.../AggregateFunction.java:160).
 * Eligible: tumbling windows or sliding windows kept as panes (size a multiple of slide; a partial is then one
 * (key, pane) accumulator), FW_AGG_COUNT_SUM_MIN_MAX, allowed lateness 0, no side output, Long or Integer keys.
 * A combiner is an ordinary handle over the subtask's whole input (any KeyGroupRange covering it; its watermark is
 * never advanced) into which the subtask pushes its batch; fw_combine_extract_device then drains the combiner's
 * state into the partials (device columns, the accumulators in the handle's own representation: only
 * fw_push_partials_device of a handle with the same configuration reads them) in key-group order, so destination
 * d of `world` subtasks (KeyGroupRangeAssignment.computeOperatorIndexForKeyGroup, :115-117) owns the contiguous
 * slice counts[d]; it empties the combiner.  When the partials exceed cap, *n is set, nothing is drained and
 * FW_ERR_CAPACITY is returned.  fw_push_partials_device is processElement for the partials of the receiving
 * subtask's KeyGroupRange: a partial whose window is late is dropped and its count added to the late records
 * (WindowOperator.java:402-418; with allowed lateness 0 every record of a late window is late). */
typedef struct {
  int64_t *key, *start, *cnt, *sum, *min, *max;
  /* the producing combiner's configuration tag (written by fw_combine_extract_device): assigner, size, slide,
     offset, value type, key kind, max parallelism and aggregate.  fw_push_partials_device refuses partials whose tag is
     not its own (FW_ERR_ARG): the accumulators are in the handle's internal representation (f64 min/max in
     sortable form, window starts of its own size and offset), so a differently configured receiver would
     misread them. */
  uint64_t config;
} fw_partials;
int fw_combine_extract_device(fw_op* combiner, int32_t world, fw_partials* out, int64_t cap, int64_t* counts,
                              int64_t* n);
int fw_push_partials_device(fw_op* op, const fw_partials* in, int64_t n);

/* Keyed-state snapshot and restore, one key group at a time: the heap backend writes its state per
 * key group (flink-runtime/.../state/heap/HeapKeyedStateBackend.java:289-399, offsets per key group
 * :370-381) and the timers likewise (api/operators/InternalTimeServiceManager.java:114), which is
 * what lets a restore re-shard the key groups over a different parallelism.  One row per live
 * (key, window) accumulator of "window-contents"; `timer` = 1 when the window's event-time trigger
 * timer (maxTimestamp) is registered, 0 when only its cleanup timer is pending (the cleanup timer is
 * implied by the window: cleanupTime, WindowOperator.java:637-644).  sum/min/max are in the form of
 * the fired rows (fw_rows).  Rows come out in no particular order.
 *   fw_snapshot_key_group: copies the key group's rows into caller-owned host arrays of capacity cap;
 *     with cap too small (or dst NULL) it only returns the row count in *n.
 *   fw_restore_key_group: inserts rows into the handle (which must own the key group); a row whose
 *     (key, window) is already present is merged into it (AggregateFunction.merge).  Long/Integer
 *     keys outside the key group are refused with FW_ERR_KEY_GROUP.  First-element reduces (FW_AGG_FIRST,
 *     FW_AGG_FIRST_MAX, FW_AGG_MINBY, FW_AGG_MAXBY): `max` is the element's ordinal, and later pushes are
 *     numbered after the largest restored one.  Rows of one call that restore the same (key, window) are merged
 *     in order.  HyperLogLog and t-digest handles keep their accumulator beside the row: these two calls
 *     refuse them (FW_ERR_UNSUPPORTED) and the _blocks variants below carry it. */
typedef struct fw_state_rows {
  int64_t* key;
  int64_t* start;
  int64_t* end;
  int64_t* count;
  int64_t* sum;
  int64_t* min;
  int64_t* max;
  int64_t* timer;
} fw_state_rows;
int fw_snapshot_key_group(fw_op* op, int32_t key_group, const fw_state_rows* host_dst, int64_t cap, int64_t* n);
int fw_restore_key_group(fw_op* op, int32_t key_group, const fw_state_rows* host_src, int64_t n);

/* The same with each row's accumulator block, for the aggregates whose accumulator is not in the row
 * (FW_AGG_HLL, FW_AGG_TDIGEST; any other handle takes them with blocks NULL).  The heap backend stores the
 * accumulator in the state's value column through the AggregateFunction's accumulator serializer
 * (HeapAggregatingState.java:73-93 keeps the ACC object; its TypeSerializer writes it per mapping at snapshot,
 * HeapKeyedStateBackend.java:370-381); this build's accumulators are fixed-size blocks of
 * fw_state_block_bytes(op) bytes, row i's at blocks + i * fw_state_block_bytes(op):
 *   FW_AGG_HLL      the 2^p registers M[0..m), one byte each (the rank, 0 = untouched);
 *   FW_AGG_TDIGEST  int64 little-endian words: n, then (sum as f64 bits, weight) of centroids 0..n-1 in
 *                   mean order, zero-padded to 1 + 2 * floor(delta / 2) words (the fw_rows.digests layout).
 * fw_snapshot_key_group_blocks: rows as fw_snapshot_key_group plus the blocks (host buffer of cap rows; NULL
 *   with cap 0 only counts).
 * fw_restore_key_group_blocks: rows as fw_restore_key_group; a new (key, window) takes a pool block holding the
 *   imported accumulator.  A HyperLogLog row whose (key, window) is already present merges by register max
 *   (AggregateFunction.merge); a t-digest one is refused with FW_ERR_STATE (the digest is not re-compressed).
 *   Rows must fit the pool (expected_entries): FW_ERR_CAPACITY otherwise, before anything changes. */
int64_t fw_state_block_bytes(fw_op* op);
int fw_snapshot_key_group_blocks(fw_op* op, int32_t key_group, const fw_state_rows* host_dst, uint8_t* host_blocks,
                                 int64_t cap, int64_t* n);
int fw_restore_key_group_blocks(fw_op* op, int32_t key_group, const fw_state_rows* host_src,
                                const uint8_t* host_blocks, int64_t n);

/* The same for a FW_TRIGGER_CONTINUOUS_EVENT_TIME handle, whose windows carry the trigger's partitioned state: the
 * "fire-time" ReducingState (ContinuousEventTimeTrigger.java:44-46, Min) and its timer (the heap backend snapshots both
 * per key group, HeapKeyedStateBackend.java:370-381, InternalTimeServiceManager.java:114).  fire_time[i] is row i's
 * fire time, Long.MIN_VALUE = null (as in the list operator's snapshots); in the `timer` column bit 0 is
 * maxTimestamp's timer and bit 1 "the timer at the fire time is registered".  A window purged by PurgingTrigger is a
 * row too (count 0) until its cleanup time: its fire time and timers are state.  Restore into any KeyGroupRange
 * (rescaling) works as for the plain rows; a row whose (key, window) is present merges, the fire times by Min.
 * fw_snapshot_key_group / fw_restore_key_group (and the _blocks forms) refuse such a handle with
 * FW_ERR_UNSUPPORTED, and these two refuse every other handle.  (The heap-format bridge does not carry the
 * trigger's state: DESIGN.md §7.) */
int fw_snapshot_key_group_fire(fw_op* op, int32_t key_group, const fw_state_rows* host_dst, int64_t* host_fire_time,
                               int64_t cap, int64_t* n);
int fw_restore_key_group_fire(fw_op* op, int32_t key_group, const fw_state_rows* host_src,
                              const int64_t* host_fire_time, int64_t n);

/* CountTrigger on the aggregating operator: WindowedStream.trigger(CountTrigger.of(max_count)) over the aggregating
 * state (WindowOperator.java:379-407 with HeapAggregatingState; CountTrigger.java:47-85), `cfg->purging` wrapping it
 * in PurgingTrigger.  A second constructor, as fw_list_create_join is: fw_config does not grow, cfg->trigger must be 0
 * (FW_ERR_ARG), and fw_create goes on refusing FW_TRIGGER_COUNT.
 *   Per element and window that is not late (cleanupTime > watermark; a window behind the watermark but within the
 *   allowed lateness counts like any other -- this trigger has no late firing of its own): add the element, count += 1,
 *   and at count >= max_count clear the count and emit one row {count, sum, min, max} of the accumulator as of that
 *   element; under PurgingTrigger the accumulator is cleared behind the row.  The comparison is >=: a restored or merged
 *   count of max_count or more fires at the next element.  A watermark fires nothing (onEventTime: CONTINUE); at the
 *   cleanup time the accumulator and the count are dropped, so a window's last < max_count elements are never emitted.
 *   Late records (all windows late): side output / late_records_dropped as on every handle.
 *   Offered for FW_AGG_COUNT_SUM_MIN_MAX over every value type and key kind, FW_TUMBLING and FW_SLIDING, with allowed
 *   lateness, purging and side output, host and device pushes.  The handle keeps windows (no panes, dense regions,
 *   compact or narrow records, single pass); the count rides in the window's entry.  A push, device columns included,
 *   is complete when the call returns (the host reads the push's row bound in the middle of it), and
 *   fw_input_stream(op) == fw_stream(op) whatever fw_set_async_input says.
 *   Refused before the GPU is touched: max_count outside [1, 2^31) and cfg->trigger != 0 (FW_ERR_ARG); FW_SESSION
 *   (fw_list_create with merging_state takes CountTrigger over sessions), FW_COUNT and every other aggregate
 *   (FW_ERR_UNSUPPORTED; each message names fw_list_create).
 *   Every entry point takes such a handle except the pre-shuffle combiner ones (a combiner's partials carry no arrival
 *   order) and the other snapshot / restore calls, which name the pair below (FW_ERR_UNSUPPORTED).
 *   fw_stats: keyed_state_entries counts the windows with contents (a purged window keeps its emptied entry and its
 *   cleanup timer until the cleanup time), event_time_timers one cleanup timer per window in flight.
 * fw_snapshot_key_group_trigger_count / fw_restore_key_group_trigger_count: the rows of fw_snapshot_key_group plus
 *   trigger_count[i], row i's count state (CountTrigger's "count" ReducingState, Sum; in [0, 2^48)); `timer` is 0 (no
 *   timer at maxTimestamp).  A purged, empty window is a row of count 0 until its cleanup time.  Restore into any
 *   KeyGroupRange works as for the plain rows; rows of one (key, window) merge and their trigger counts add without
 *   firing (CountTrigger.onMerge).  These two refuse every other handle.  (The heap-format bridge does not carry this
 *   state: DESIGN.md §7.) */
int fw_create_count_trigger(const fw_config* cfg, int64_t max_count, fw_op** out);
int fw_snapshot_key_group_trigger_count(fw_op* op, int32_t key_group, const fw_state_rows* host_dst,
                                        int64_t* host_trigger_count, int64_t cap, int64_t* n);
int fw_restore_key_group_trigger_count(fw_op* op, int32_t key_group, const fw_state_rows* host_src,
                                       const int64_t* host_trigger_count, int64_t n);

/* Key routing (both sides of keyBy).
 *   fw_key_groups_device: kg[i] = KeyGroupRangeAssignment.assignToKeyGroup(key_i, maxParallelism)
 *     (flink-runtime/.../state/KeyGroupRangeAssignment.java:58-71, MathUtils.java:134-154).
 *   fw_route_device: KeyGroupStreamPartitioner.selectChannels (runtime/partitioner/
 *     KeyGroupStreamPartitioner.java:53-65): groups the batch by destination operator index
 *     computeOperatorIndexForKeyGroup(maxPar, parallelism, kg) (KeyGroupRangeAssignment.java:115-117),
 *     keeping arrival order inside each destination; writes the reordered columns and
 *     counts[parallelism] (int64, device).  All pointers are device pointers on `device`;
 *     the call is asynchronous on `stream` (a hipStream_t, NULL = default stream). */
int fw_key_groups_device(const int64_t* key, const int32_t* key_hash, int32_t key_kind, int64_t n,
                         int32_t max_parallelism, int32_t* kg_out, void* stream);
int fw_route_device(const int64_t* key, const int64_t* ts, const int64_t* val, const int32_t* key_hash,
                    int32_t key_kind, int64_t n, int32_t max_parallelism, int32_t parallelism, int64_t* key_out,
                    int64_t* ts_out, int64_t* val_out, int32_t* hash_out, int64_t* counts, void* scratch,
                    int64_t scratch_bytes, void* stream);
int64_t fw_route_scratch_bytes(int64_t n, int32_t parallelism);

/* Pre-shuffle combining of HyperLogLog ("combining is results-equal for count/sum/min/max/HLL"): a
 * combiner's windows cross the exchange as partial rows plus their non-zero registers, the receiver merges them
 * with AggregateFunction.merge = register max (flink-core/.../AggregateFunction.java:160).  Tumbling windows, no
 * allowed lateness, Long or Integer keys (FW_ERR_UNSUPPORTED otherwise).
 *   fw_combine_extract_hll_device: drains the combiner like fw_combine_extract_device; a row's sum = how many of
 *     its window's registers are non-zero (min holds an opaque block id until the registers are taken),
 *     reg_counts[d] = the registers of destination d's partials (in partial order), *nregs their total.
 *   fw_combine_hll_registers_device: then writes the n rows' registers into regs[0, nregs) as u32
 *     (register index << 8 | rank), in row order, and releases the combiner's blocks (FW_ERR_CAPACITY, with
 *     nothing taken, when regs_cap < nregs; FW_ERR_STATE without a preceding extraction of n rows).
 *   fw_push_hll_partials_device: merges received partial rows (counts) and raises their registers (regs: the rows'
 *     register lists concatenated in row order) into this operator's windows; late rows are dropped with their
 *     records, as fw_push_partials_device does. */
int fw_combine_extract_hll_device(fw_op* op, int32_t world, fw_partials* out, int64_t cap, int64_t* counts,
                                  int64_t* reg_counts, int64_t* n, int64_t* nregs);
int fw_combine_hll_registers_device(fw_op* op, const fw_partials* out, int64_t n, uint32_t* regs, int64_t regs_cap);
int fw_push_hll_partials_device(fw_op* op, const fw_partials* in, int64_t n, const uint32_t* regs, int64_t nregs);

/* keyBy across the GPUs of one node behind the C-ABI (the RecordWriter -> KeyGroupStreamPartitioner ->
 * network -> input gate path: flink-runtime/.../io/network/api/writer/RecordWriter.java:88-115,
 * runtime/partitioner/KeyGroupStreamPartitioner.java:53-65; watermark valve runtime/streamstatus/
 * StatusWatermarkValve.java:173-191), over RCCL.  One communicator per subtask / GPU:
 *   fw_comm_unique_id: rank 0 creates the id (128 bytes) and hands it to the other subtasks (e.g. through the
 *     JobManager); fw_comm_init: every subtask joins with its rank (= its operator index) on its device.
 *   fw_keyby_push_device: this subtask's device batch is grouped by destination subtask
 *     (computeOperatorIndexForKeyGroup), the per-peer counts are exchanged (all-to-all of one int64 each, then
 *     read by the host: the receive sizes), the key / timestamp / value (/ key hash) columns go peer to peer
 *     (grouped ncclSend / ncclRecv, one pair per peer), and the records received from subtasks 0 .. world-1, each
 *     source's arrival order kept, are pushed into `op` (fw_push_batch_device), whose KeyGroupRange must be
 *     computeKeyGroupRangeForOperatorIndex(maxParallelism, world, rank).  *combined_wm = min over the subtasks of
 *     local_wm (the operator's input watermark), for the caller's fw_advance_watermark.  Collective: every
 *     subtask calls it once per batch.  Enqueued on fw_input_stream(op); the host waits once per batch, for the
 *     route and the count exchange on that stream (with async input not for the previous batch's aggregation). */
typedef struct fw_comm fw_comm;
int fw_comm_unique_id(void* id128);
int fw_comm_init(const void* id128, int32_t world, int32_t rank, int32_t device, fw_comm** out);
void fw_comm_destroy(fw_comm* comm);
int fw_keyby_push_device(fw_comm* comm, fw_op* op, const int64_t* key, const int64_t* ts, const void* val,
                         const int32_t* key_hash, int64_t n, int64_t local_wm, int64_t* combined_wm);
/* The same with pre-shuffle combining (see fw_combine_extract_device): the batch goes into `combiner` (this
 * subtask's combiner handle, same configuration -- FW_ERR_ARG otherwise --, never given a watermark), which is
 * drained into partials; the
 * partials' per-peer counts and six columns cross the exchange instead of the records, and the received ones are
 * merged into `op` (fw_push_partials_device).  Eligible configurations only. */
int fw_keyby_combine_push_device(fw_comm* comm, fw_op* combiner, fw_op* op, const int64_t* key, const int64_t* ts,
                                 const void* val, int64_t n, int64_t local_wm, int64_t* combined_wm);
/* The exchange's counters (the sending side of RecordWriter's numBytesOut / numRecordsOut,
 * flink-runtime/.../io/network/api/writer/RecordWriter.java:88-115): world / rank as the RCCL communicator reports
 * them (ncclCommCount / ncclCommUserRank), batches exchanged, items (records, or partials when combining) and
 * bytes sent to and received from the OTHER subtasks (a subtask's own share never leaves the GPU), how often the
 * receive columns were reallocated and what they hold. */
typedef struct fw_comm_stats {
  int32_t world, rank;
  int64_t batches, items_sent, items_received, bytes_sent, bytes_received, recv_reallocs, recv_capacity;
} fw_comm_stats;
int fw_comm_get_stats(fw_comm* comm, fw_comm_stats* out);
/* The host arithmetic of one exchange round, from the counts round's int64[2 world + 4] (send counts per peer,
 * receive counts per peer, watermark in / min, batch size in / sum over subtasks): send and receive offsets
 * ([world + 1] each, prefix sums: records from subtask 0 first, then 1, ..., as the input gate's channels) and
 * the totals.  recv_bound = the sum of every subtask's batch: no subtask can receive more, so the receive columns
 * are sized for it once.  FW_ERR_STATE when the counts contradict themselves (negative, more received than the
 * whole batch, the own share sent != received). */
typedef struct fw_exchange_plan_t {
  int64_t send_total, recv_total, items_sent, items_received, recv_bound;
} fw_exchange_plan_t;
int fw_exchange_plan(int32_t world, int32_t rank, const int64_t* counts, int64_t* send_off, int64_t* recv_off,
                     fw_exchange_plan_t* out);

/* ---- f2: Flink's wire format for one input channel <-> device columns.
 * The byte stream of a channel is its network buffers in order: SpanningRecordSerializer.addRecord writes each
 * StreamElement as a 4-byte big-endian length and then its bytes (flink-runtime/.../io/network/api/serialization/
 * SpanningRecordSerializer.java:76-98), StreamElementSerializer (SJ/runtime/streamrecord/StreamElementSerializer
 * .java:54-58, 167-221) writes a tag byte then
 *   0 record with timestamp: BE i64 timestamp, the value      1 record without timestamp: the value
 *   2 watermark: BE i64       3 latency marker: BE i64 marked time, BE i64 x 2 operator id, BE i32 subtask
 *   4 stream status: BE i32   (any other tag: "Corrupt stream, found tag: X")
 * and the value is a Tuple (TupleSerializer: fields in order, no null mask) of fixed-size fields, or one bare
 * field: Long / Integer / Short / Byte / Boolean (BE two's complement) and Double / Float (BE
 * doubleToLongBits / floatToIntBits), or String (StringSerializer -> StringValue.writeString, StringValue.java:
 * 789-817: length + 1 as a base-128 varint, 0 = null, then each UTF-16 char as a base-128 varint).  A String
 * field is the key (FW_ROLE_KEY) or skipped: the key column then holds the chars' 64-bit id (FNV-1a 64 over the
 * UTF-16 chars, then fmix64 of it ^ the length) and the key_hash column String.hashCode, the two columns
 * FW_KEY_HASHED takes; a null String key is a corrupt element (KeyGroupStreamPartitioner cannot hash it).  A
 * record with String fields is decoded when it is at most 64 bytes with its length prefix (WindowWordCount's
 * Tuple2<String, Integer> with a timestamp: words of up to 46 ASCII chars); a longer one is refused as a corrupt
 * element, and so is a String varint whose fifth byte still continues (writeString never writes one).  That limit,
 * the integer narrowing below and the String key's id are this build's own; everything else is pinned against an
 * independent restatement of the cited serializers (tests/wire_ref.py).
 *   fw_wire_decode_device: a device byte stream -> key / ts / val columns in arrival order (records without a
 *     timestamp get Long.MIN_VALUE, StreamRecord.getTimestamp), ready for fw_push_batch_device.  The field whose
 *     role is FW_ROLE_KEY becomes the key (an integer kind), FW_ROLE_VALUE the value (integers sign-extended,
 *     Double as its bits, Float widened to double bits); other fields are skipped.  stats: the frames of each
 *     kind, the last watermark (Long.MIN_VALUE if none: the caller's processWatermark), the last stream status
 *     (StreamStatus ACTIVE 0 / IDLE -1; 0 if none), and `consumed` = the bytes up to the end of the last complete element (a trailing partial element is
 *     the start of the next call's stream, SpillingAdaptiveSpanningRecordDeserializer's role).  The last watermark
 *     is found by presence: Watermark(Long.MIN_VALUE) is a watermark like any other.  At a corrupt element the
 *     call returns FW_ERR_STATE and still fills `stats` (the frames before that element, `consumed` = its byte
 *     position) and the columns' leading `stats->records` records, as the reference's deserializer has handed
 *     those on before it throws.  Frames are
 *     found in parallel: every 2 KiB chunk is parsed from each of its 64 possible first-frame offsets, and the
 *     chunks' transfer functions are composed (a decoded element is at most 64 bytes with its length prefix:
 *     value fields of at most 51 bytes).
 *   fw_wire_encode_device: fired rows -> elements of one output channel: tag 0, timestamp = end - 1 (the
 *     window's maxTimestamp, WindowOperator.emitWindowContents' TimestampedCollector), a Tuple of the row
 *     fields the layout's roles name (FW_ROLE_KEY / START / END / COUNT / SUM / MIN / MAX).  end - 1 is Java's
 *     long arithmetic (Long.MIN_VALUE - 1 wraps to Long.MAX_VALUE); a row whose end is Long.MAX_VALUE is a
 *     GlobalWindow's and keeps Long.MAX_VALUE (GlobalWindow.java:45-46).  Double and Float fields are written as
 *     DataOutputSerializer does (doubleToLongBits / floatToIntBits, DataOutputSerializer.java:173-180): every NaN,
 *     whatever its sign and payload, becomes 0x7ff8000000000000 / 0x7fc00000, and (float) rounds to nearest even.
 *     An integer row field written into a Double / Float field is (double) v, then (float) of that.  An f64 row
 *     field (sum / min / max of an FW_VAL_F64 aggregate) written into an integer field is Java's (long) d (NaN 0,
 *     saturating, toward zero) and then the field's low bytes, as (int) / (short) / (byte) of that long.
 * Both return FW_ERR_ARG for an unsupported layout and FW_ERR_STATE for a corrupt stream (message in
 * fw_wire_last_error) or too small an output; they run on the codec's own stream and return when done. */
#define FW_WIRE_LONG 0
#define FW_WIRE_INT 1
#define FW_WIRE_DOUBLE 2
#define FW_WIRE_SHORT 3
#define FW_WIRE_BYTE 4
#define FW_WIRE_FLOAT 5
#define FW_WIRE_BOOL 6
#define FW_WIRE_STRING 7
#define FW_ROLE_SKIP 0
#define FW_ROLE_KEY 1
#define FW_ROLE_VALUE 2
#define FW_ROLE_START 3
#define FW_ROLE_END 4
#define FW_ROLE_COUNT 5
#define FW_ROLE_SUM 6
#define FW_ROLE_MIN 7
#define FW_ROLE_MAX 8
#define FW_WIRE_MAX_FIELDS 8
typedef struct {
  int32_t nfields;                     /* 1 = a bare field, > 1 = a Tuple of that arity */
  int32_t kind[FW_WIRE_MAX_FIELDS];    /* FW_WIRE_* */
  int32_t role[FW_WIRE_MAX_FIELDS];    /* FW_ROLE_* */
} fw_wire_layout;
typedef struct {
  int64_t records, watermarks, latency_markers, statuses;
  int64_t consumed;                    /* bytes of complete elements */
  int64_t watermark;                   /* the last watermark, Long.MIN_VALUE if none */
  int32_t status;                      /* the last stream status (0 ACTIVE, -1 IDLE), 0 if none */
  int32_t pad;
} fw_wire_stats;
typedef struct fw_wire fw_wire;
/* max_bytes: the largest stream of one decode call; device: the HIP device of the buffers */
int fw_wire_create(const fw_wire_layout* layout, int64_t max_bytes, int32_t device, fw_wire** out);
void fw_wire_destroy(fw_wire* w);
const char* fw_wire_last_error(const fw_wire* w);
int fw_wire_decode_device(fw_wire* w, const uint8_t* bytes, int64_t nbytes, int64_t* key, int64_t* ts, int64_t* val,
                          int64_t cap, fw_wire_stats* stats);
/* the same with the key_hash column (int32, the key's Java hashCode: String.hashCode of a String key, 0 for the
 * other kinds, whose hash the operator derives itself); required when the key field is a String */
int fw_wire_decode_keyed_device(fw_wire* w, const uint8_t* bytes, int64_t nbytes, int64_t* key, int32_t* key_hash,
                                int64_t* ts, int64_t* val, int64_t cap, fw_wire_stats* stats);
/* rows: a device view (fw_rows_device); f64 = the rows' sum/min/max are double bits (FW_VAL_F64 aggregates);
 * out: device bytes of capacity cap; *written = n * element size */
int fw_wire_encode_device(fw_wire* w, const fw_rows* rows, int64_t n, int32_t f64, uint8_t* out, int64_t cap,
                          int64_t* written);

/* ---- f4: window contents (ListState) — WindowedStream.apply / process with an Iterable window function, and
 * evictors (SJ/api/datastream/WindowedStream.java:1080-1123 builds a WindowOperator over a ListStateDescriptor, or an
 * EvictingWindowOperator when an evictor is set).  The handle keeps every (key, window)'s list of elements in HBM
 * and applies, element by element, EvictingWindowOperator.processElement / onEventTime / emitWindowContents
 * (runtime/operators/windowing/EvictingWindowOperator.java:102-366; without an evictor WindowOperator.java:291-469):
 *   assigners  FW_TUMBLING, FW_SLIDING (every window of a record holds a copy), FW_GLOBAL (GlobalWindows: never
 *              late, never cleaned up; rows have start = Long.MIN_VALUE, end = Long.MAX_VALUE = their timestamp);
 *   triggers   FW_TRIGGER_EVENT_TIME (EventTimeTrigger.java:37-73), FW_TRIGGER_COUNT (CountTrigger.of(n),
 *              CountTrigger.java:47-70) or FW_TRIGGER_CONTINUOUS_EVENT_TIME (ContinuousEventTimeTrigger.of(interval),
 *              ContinuousEventTimeTrigger.java:39-151: early firings every trigger_interval ms of event time until
 *              the window's maxTimestamp, over time, global and session windows), each wrapped in PurgingTrigger
 *              (purging = 1) or not.  With the continuous trigger one watermark can fire a window several times: its
 *              due timers run in ascending time, every firing a row of its own (an evictor runs per firing; a timer
 *              that finds no contents does not reach the trigger, so it is not re-armed: WindowOperator.java:446-459).
 *              More than 2^20 firings of one window in one advance are refused (FW_ERR_UNSUPPORTED, nothing changed);
 *              FW_TRIGGER_DELTA (DeltaTrigger.of(trigger_threshold, f, serializer), DeltaTrigger.java:38-99, with the
 *              built-in f(old, new) = new.field - old.field over the value field, in the field's Java arithmetic and
 *              then widened to double: the mirror of the built-in DeltaEvictor function): per (key, window) the
 *              ValueState "last-element".  onElement (:53-64): no state -> the element is stored, nothing fires;
 *              f(last, element) > threshold (strict; a NaN delta never fires) -> the element is stored and the window
 *              FIREs over the list up to it; else nothing.  onEventTime is CONTINUE and the trigger registers no timer:
 *              a time window never fires at its maxTimestamp and has only the operator's cleanup timer; GlobalWindows
 *              have none.  clear() drops the state at the window's cleanup (clearAllState); a purge (purging = 1)
 *              or an evictor that empties the list leaves it.  Over tumbling, sliding (the state is per window) and
 *              global windows.  Refused before the device is touched: FW_SESSION, with or without merging_state
 *              (FW_ERR_ARG, "A merging window assigner cannot be used with a trigger that does not support merging.",
 *              WindowedStream.trigger: DeltaTrigger does not override canMerge), a NaN threshold (FW_ERR_ARG), and a
 *              join handle (FW_ERR_UNSUPPORTED: a DeltaFunction over the tagged union is user code).
 *              fw_stats, as for CountTrigger's count: keyed_state_entries counts the windows with contents only (a
 *              purged or emptied window keeps its last element, uncounted, until its cleanup), event_time_timers the
 *              cleanup timers only;
 *   evictors   CountEvictor.of(n[, after]) (CountEvictor.java:50-78), TimeEvictor.of(ms[, after]) (TimeEvictor.java
 *              :54-104; a timestamp of Long.MIN_VALUE is "no timestamp": nothing is evicted when the first element
 *              has none), DeltaEvictor.of(threshold, f[, after]) with the built-in f(e, last) = last.field - e.field
 *              in the field's Java arithmetic (DeltaEvictor.java:59-80).
 * Every firing emits one row: the window, count = elements the function sees (after evictBefore), the built-in
 * reduce over them in list order (sum wrapped to the field width, min, max; Double / Float fields by compare
 * order, sums in list order, so f64 sums are exact), first = the arrival ordinal of the first element (-1 if none;
 * the passthrough fields of reduce / sum(pos)), and with emit_contents the elements themselves in list order
 * (timestamp, value, ordinal) for the host's Iterable function (InternalIterableWindowFunction).  A push is
 * processed completely before the call returns (late firings and count triggers are ordered per (key, window)). */
#define FW_GLOBAL 4
#define FW_TRIGGER_EVENT_TIME 0
#define FW_TRIGGER_COUNT 1
#define FW_TRIGGER_CONTINUOUS_EVENT_TIME 2
#define FW_TRIGGER_DELTA 3
#define FW_EVICT_NONE 0
#define FW_EVICT_COUNT 1
#define FW_EVICT_TIME 2
#define FW_EVICT_DELTA 3
typedef struct fw_list_config {
  int32_t assigner;          /* FW_TUMBLING / FW_SLIDING / FW_GLOBAL / FW_SESSION (size = the gap)  */
  int32_t value_type;        /* FW_VAL_*                                                          */
  int32_t key_kind;          /* FW_KEY_*                                                          */
  int32_t trigger;           /* FW_TRIGGER_*                                                      */
  int32_t purging;           /* PurgingTrigger.of(trigger)                                        */
  int32_t evictor;           /* FW_EVICT_*                                                        */
  int32_t evict_after;       /* doEvictAfter                                                      */
  int32_t side_output;       /* late records to the side output instead of numLateRecordsDropped */
  int32_t emit_contents;     /* 1 = fired rows carry their elements                               */
  int32_t max_parallelism;   /* as fw_config                                                      */
  int32_t key_group_start;
  int32_t key_group_end;
  int32_t device;
  int32_t merging_state;     /* FW_SESSION only (FW_ERR_ARG otherwise): 1 = the handle keeps the full
                                MergingWindowSet form per in-flight window (its state window, the trigger's
                                count), takes FW_TRIGGER_COUNT and offers fw_list_snapshot_sessions /
                                fw_list_restore_sessions.  0 (the slot was padding): nothing of it         */
  int64_t size, slide, offset, allowed_lateness;
  int64_t trigger_count;     /* CountTrigger.of(n)                                                */
  int64_t evict_count;       /* CountEvictor maxCount, TimeEvictor windowSize (ms)                */
  double delta_threshold;    /* DeltaEvictor threshold                                            */
  int64_t expected_elements; /* sizing hint: elements held at once (0 = default)                  */
  int64_t max_batch;         /* largest n of one push (0 = 1 << 24)                               */
  union {                    /* the last slot: the parameter of the trigger that has one of its own          */
    int64_t trigger_interval;  /* ContinuousEventTimeTrigger.of(interval), ms (> 0 for that trigger)    */
    double trigger_threshold;  /* FW_TRIGGER_DELTA: DeltaTrigger's threshold (not NaN), apart from the
                                  DeltaEvictor's delta_threshold: a handle may use both                  */
  };
} fw_list_config;
typedef struct fw_list_rows {
  int64_t *key, *start, *end, *count, *sum, *min, *max;
  int64_t* first;            /* arrival ordinal of the row's first element, -1 if none          */
  int64_t* elem_off;         /* index of the row's first element among the drained elements     */
} fw_list_rows;
typedef struct fw_list_elems {
  int64_t *ts, *val, *ordinal;
} fw_list_elems;
/* A key group's list state, for snapshot / restore (the heap backend writes "window-contents" per key group:
 * HeapKeyedStateBackend.java:370-381): per (key, window) its list, CountTrigger's count and whether its
 * EventTimeTrigger timer is registered; the elements of all lists concatenated in list order.
 * With FW_TRIGGER_CONTINUOUS_EVENT_TIME the trigger_count column carries the trigger's "fire-time" state instead
 * (the next early firing; Long.MIN_VALUE = null), and timer is a bit set: 1 = the maxTimestamp timer is registered,
 * 2 = the timer at the fire time is registered (it is not once a firing at maxTimestamp or a timer over empty
 * contents has consumed it).
 * With FW_TRIGGER_DELTA the trigger_count column carries the value bits of the trigger's "last-element" state (as the
 * val column carries an element's) and timer bit 4 says that the state is present (0 otherwise: trigger_count is then
 * 0); bits 1 and 2 are never set, the trigger has no timer.  A window whose list is empty (purged or evicted) but
 * whose state is present is written with n_elems 0.  fw_list_restore_key_group refuses, with the handle unchanged, bit
 * 4 on a handle of another trigger and any other bit on a FW_TRIGGER_DELTA handle (FW_ERR_ARG). */
typedef struct fw_list_state {
  int64_t *key, *start, *end, *trigger_count, *timer, *n_elems;  /* per list   */
  int64_t *ts, *val, *ordinal;                                   /* elements   */
} fw_list_state;
typedef struct fw_list fw_list;
/* as fw_create: on an error *out may hold a handle that carries the message (fw_list_last_error); destroy it */
int fw_list_create(const fw_list_config* cfg, fw_list** out);
void fw_list_destroy(fw_list* op);
const char* fw_list_last_error(const fw_list* op);
/* processElement for a batch: host buffers, or device buffers on the handle's device (key_hash as fw_push_batch) */
int fw_list_push_batch(fw_list* op, const int64_t* key, const int64_t* ts, const void* val, const int32_t* key_hash,
                       int64_t n);
int fw_list_push_batch_device(fw_list* op, const int64_t* key, const int64_t* ts, const void* val,
                              const int32_t* key_hash, int64_t n);
/* processWatermark: the trigger's event-time timers <= wm fire their lists (a ContinuousEventTimeTrigger window once
 * per due timer), cleanup timers drop them */
int fw_list_advance_watermark(fw_list* op, int64_t wm, int64_t* n_pending_rows);
int fw_list_pending(fw_list* op, int64_t* n_rows, int64_t* n_elems, int64_t* n_side_rows);
/* copies the pending rows (and elements: elem_off counts from the first drained element) into host arrays and
 * clears them; FW_ERR_CAPACITY (nothing drained) when either capacity is too small */
int fw_list_drain(fw_list* op, const fw_list_rows* rows, int64_t cap_rows, const fw_list_elems* elems,
                  int64_t cap_elems, int64_t* n_rows, int64_t* n_elems);
int fw_list_drain_side(fw_list* op, const fw_side_rows* host_dst, int64_t cap, int64_t* n);
/* drops the pending rows and elements without copying them (a discarding sink) */
int fw_list_clear_pending(fw_list* op);
int fw_list_get_stats(fw_list* op, fw_stats* out);
/* per key group: the lists (dst NULL or a capacity too small: only the counts) / restored into the handle, appended
 * to a list already present */
int fw_list_snapshot_key_group(fw_list* op, int32_t key_group, const fw_list_state* dst, int64_t cap_lists,
                               int64_t cap_elems, int64_t* n_lists, int64_t* n_elems);
int fw_list_restore_key_group(fw_list* op, int32_t key_group, const fw_list_state* src, int64_t n_lists,
                              int64_t n_elems);

/* Session windows (FW_SESSION handles created with merging_state = 1): a key group's keyed state in the form the
 * merging WindowOperator keeps it (MergingWindowSet.java:150-225, WindowOperator.java:297-370): per in-flight window
 * the window itself (the namespace of the trigger's state and of the timers), its state window (the namespace its
 * "window-contents" list is kept under: the window the session started as, or the one a merge chose), the trigger's
 * state (CountTrigger's count, CountTrigger.java:47-85; ContinuousEventTimeTrigger's fire time, Long.MIN_VALUE =
 * null; 0 under EventTimeTrigger), timer with the bits of fw_list_state, and its list: the elements of all windows
 * concatenated in list order (the order the window function sees, not arrival order).  A purged window is a row with
 * n_elems 0: it stays in the MergingWindowSet until its cleanup time.
 * CountTrigger over sessions (merging_state handles only): a merge sums the merged windows' counts into the result
 * and does not fire; the element then counts, and at n the count is cleared and the window's whole list fires
 * (evictors as for every firing; PurgingTrigger clears the list); no timer is registered, and the window, its list
 * and its count are dropped at its cleanup time without a firing.
 * fw_list_snapshot_sessions follows fw_list_snapshot_key_group: dst NULL or a capacity too small returns only the
 * counts; windows come out in no particular order.  fw_list_restore_sessions refuses, with the handle untouched:
 * lengths that do not add up, a window shorter than the gap, two windows of a key that intersect
 * (TimeWindow.intersects) or share a state window, timer bits or a count that the handle's trigger cannot have
 * (FW_ERR_ARG); a FW_KEY_LONG / FW_KEY_INT key outside key_group (FW_ERR_KEY_GROUP); a key that already has an
 * in-flight window in the handle (FW_ERR_STATE).  Later pushes are numbered after the largest restored ordinal;
 * windows that are already due fire or leave with the next fw_list_advance_watermark.  The watermark is not part of
 * the state: a restored handle starts at Long.MIN_VALUE, as the reference's operator does, until it is advanced.  A
 * device failure after the restore began to apply leaves the handle unusable (FW_ERR_STATE from then on).  Both return
 * FW_ERR_UNSUPPORTED on a handle without merging_state. */
typedef struct fw_session_state {
  int64_t *key, *start, *end, *state_start, *state_end, *trigger_state, *timer, *n_elems; /* per window */
  int64_t *ts, *val, *ordinal;                                                            /* elements   */
} fw_session_state;
int fw_list_snapshot_sessions(fw_list* op, int32_t key_group, const fw_session_state* dst, int64_t cap_windows,
                              int64_t cap_elems, int64_t* n_windows, int64_t* n_elems);
int fw_list_restore_sessions(fw_list* op, int32_t key_group, const fw_session_state* src, int64_t n_windows,
                             int64_t n_elems);

/* ---- window joins: DataStream.join(other).where().equalTo().window().apply(JoinFunction) and coGroup(...).
 * In the reference a window join is not an operator of its own.  CoGroupedStreams.WithWindow.apply
 * (flink-streaming-java .../api/datastream/CoGroupedStreams.java:273-304) tags both inputs (Input1Tagger /
 * Input2Tagger, TaggedUnion), unions and keys them, and builds the ordinary WindowOperator / EvictingWindowOperator
 * over a ListState with the user's assigner, trigger and evictor.  CoGroupWindowFunction.apply (:657-685) splits every
 * firing's contents by tag into two lists, each in list order, and JoinedStreams' JoinCoGroupFunction.coGroup
 * (JoinedStreams.java:387-404) collects join(val1, val2) for every val1 of the first list and, inside, every val2 of
 * the second.  WithWindow passes no allowed lateness.
 *
 * A handle created by fw_list_create_join with fw_join_config::join != 0 is that operator: every assigner, trigger, evictor, lateness,
 * side-output and merging_state combination of the list operator, and emit_contents = 1 (FW_ERR_ARG otherwise: the
 * join reads the contents).  Its elements carry their input as bit 62 of the arrival ordinal (FW_ORD_SIDE: set = input
 * 2).  Every ordinal column that leaves the handle carries the bit -- the elements of fw_list_drain and
 * fw_list_drain_join, fw_list_state and fw_session_state snapshots -- and a restore takes it back in (later pushes are
 * numbered after the largest restored ordinal with the bit cleared); the rows' `first` column is the plain ordinal,
 * bit cleared.  fw_list_push_batch_side(_device) push a batch of one input (side 0 = input 1, 1 = input 2; one batch
 * comes from one input, as the union delivers buffers); fw_list_push_batch(_device) on a join handle mean input 1.  A
 * side push on a handle without a join, or a side outside {0, 1}, is FW_ERR_ARG.  The side output of a join handle
 * carries key, ts and val as on every handle: the side of a late record is not reported (the reference's side output
 * would carry the TaggedUnion).
 *
 * The join stage is a function of the pending output alone (the fired rows and their elements); it runs when one of the
 * three calls below asks for it and never touches the operator's state, so a refusal leaves everything as it was.
 *   split   per fired row n_first = its elements of input 1, and a partitioned copy of its elements: those of input 1
 *           in list order, then those of input 2 in list order (CoGroupWindowFunction's two lists), at the row's
 *           elem_off.  fw_list_drain keeps returning the unpartitioned list order.
 *   count   pairs of a row = n_first * (count - n_first) (64 bits), 0 on a FW_JOIN_COGROUP handle.
 *   emit    (FW_JOIN_INNER) pair q of a row is (i, j) = (q / n2, q % n2), i-major -- JoinCoGroupFunction's order --,
 *           a row's pairs contiguous and rows in row order; SoA int64 columns: row = the index of the fired row among
 *           the drained rows, idx1 / idx2 = the indices of the two elements among the drained partitioned elements
 *           (a consumer gathers ts, value or ordinal through them: a JoinFunction other than the projection is the
 *           host's), val1 / val2 = the two value fields, the built-in join(a, b) = (a.field, b.field) (double bits
 *           for FW_VAL_F64 / FW_VAL_F32).
 * fw_list_join_pending runs split and count: the pending rows, elements and (exactly, also beyond what any buffer
 * holds) pairs.  fw_list_drain_join copies all pending rows, n_first, the partitioned elements and the pairs to the
 * host and clears them, or drains nothing: FW_ERR_CAPACITY with the three counts set when a capacity is too small; a
 * NULL column is skipped; pairs == NULL drains the coGroup form alone and materialises no pair.  More pending pairs
 * than max_join_pairs are not materialised (FW_ERR_CAPACITY, nothing changed; drain with pairs == NULL, or drain more
 * often).  fw_list_join_device fills the structs with device pointers, valid until the next call on the handle, and
 * clears nothing (fw_list_clear_pending does; pairs == NULL: no pairs).  All three return FW_ERR_ARG on a handle
 * without a join, which allocates and launches nothing of this. */
#define FW_JOIN_NONE 0
#define FW_JOIN_COGROUP 1
#define FW_JOIN_INNER 2
#define FW_ORD_SIDE (1LL << 62)
/* the join of a handle, given to fw_list_create_join beside the list operator's configuration (fw_list_config keeps its
 * layout: a handle made by fw_list_create has no join) */
typedef struct fw_join_config {
  int32_t join;              /* FW_JOIN_COGROUP or FW_JOIN_INNER; FW_JOIN_NONE = what fw_list_create makes            */
  int32_t pad;
  int64_t max_join_pairs;    /* FW_JOIN_INNER: the most pending pairs fw_list_drain_join / fw_list_join_device
                                materialise (0 = 2^30, 40 GB of columns); >= 0                                     */
} fw_join_config;
typedef struct fw_join_pairs {
  int64_t *row, *idx1, *idx2, *val1, *val2;
} fw_join_pairs;
/* fw_list_create with a join.  Refused before the device is touched, beside fw_list_create's own refusals: join outside
 * 0..2, join != 0 with emit_contents == 0, max_join_pairs < 0 (FW_ERR_ARG).  join NULL or join->join == 0: fw_list_create */
int fw_list_create_join(const fw_list_config* cfg, const fw_join_config* join, fw_list** out);
int fw_list_push_batch_side(fw_list* op, int32_t side, const int64_t* key, const int64_t* ts, const void* val,
                            const int32_t* key_hash, int64_t n);
int fw_list_push_batch_side_device(fw_list* op, int32_t side, const int64_t* key, const int64_t* ts, const void* val,
                                   const int32_t* key_hash, int64_t n);
int fw_list_join_pending(fw_list* op, int64_t* n_rows, int64_t* n_elems, int64_t* n_pairs);
int fw_list_drain_join(fw_list* op, const fw_list_rows* rows, int64_t* n_first, int64_t cap_rows,
                       const fw_list_elems* elems, int64_t cap_elems, const fw_join_pairs* pairs, int64_t cap_pairs,
                       int64_t* n_rows, int64_t* n_elems, int64_t* n_pairs);
int fw_list_join_device(fw_list* op, fw_list_rows* rows, int64_t** n_first, fw_list_elems* elems, fw_join_pairs* pairs,
                        int64_t* n_rows, int64_t* n_elems, int64_t* n_pairs);

/* Count windows (an fw_op with FW_COUNT): the keyed state of one key group, in the logical form of the list operator
 * above, so it moves between count handles of any parallelism and to and from the equivalent fw_list handle
 * (FW_GLOBAL, FW_TRIGGER_COUNT with trigger_count = slide, FW_EVICT_COUNT with evict_count = size and the same
 * evict_after).  Conventions as fw_list_snapshot_key_group / fw_list_restore_key_group: dst NULL or too small a
 * capacity returns only the counts; the elements of all lists are concatenated in list order; lists come out in no
 * particular order; both calls settle an unsettled device push first.  A handle that is not FW_COUNT returns
 * FW_ERR_UNSUPPORTED, a key group outside the handle's KeyGroupRange FW_ERR_KEY_GROUP.  A key's key group is the one
 * of its first record (of its key_hash with FW_KEY_HASHED); count pushes do not check the KeyGroupRange, and a key
 * outside it appears in no snapshot.
 *
 * A snapshot row is the state EvictingWindowOperator holds for the key after its k elements, reduced to what a later
 * firing can still read (EvictingWindowOperator.java:334-366, CountTrigger.java:47-70, CountEvictor.java:63-78):
 *   start = Long.MIN_VALUE, end = Long.MAX_VALUE, timer = 0 (GlobalWindows have no timers);
 *   trigger_count = k % slide (CountTrigger clears its count at each firing);
 *   the reference's list has L_ref = k elements while nothing has fired (f = k - k % slide == 0), else
 *   min(size, f) + (k - f); the row carries its last m = min(L_ref, wl - 1) elements, oldest first, with their values
 *   and arrival ordinals (wl = size, or size + slide when evicting after).  Older elements of the list are ones the
 *   next firing evicts before the function sees them.  Every ts is Long.MIN_VALUE: count handles keep no timestamps,
 *   and CountEvictor and GlobalWindow rows read none;
 *   a key with m == 0 and trigger_count == 0 is omitted; with m == 0 and trigger_count != 0 its list is empty.
 * A restore takes lists in this form, or the full lists of the equivalent list operator's snapshot.  A list of L
 * elements with trigger count t becomes a key of cnt = L + ((t - L) mod slide) elements (non-negative mod: L when the
 * residues agree), whose ring takes the list's last min(L, wl - 1) elements: element i from the end is element number
 * cnt - i.  Refused before anything changes: t outside [0, slide), a negative n_elems, a window that is not the
 * GlobalWindow or list lengths that do not add up to n_elems (FW_ERR_ARG); a key of FW_KEY_LONG / FW_KEY_INT that is
 * not in key_group (FW_ERR_KEY_GROUP); a key that occurs twice or already has state in the handle (FW_ERR_STATE);
 * more new keys than the handle's key slots have left (FW_ERR_CAPACITY).  Later pushes are numbered after the largest
 * restored ordinal.  fw_snapshot_key_group(_blocks) / fw_restore_key_group(_blocks) keep refusing count handles. */
int fw_count_snapshot_key_group(fw_op* op, int32_t key_group, const fw_list_state* dst, int64_t cap_lists,
                                int64_t cap_elems, int64_t* n_lists, int64_t* n_elems);
int fw_count_restore_key_group(fw_op* op, int32_t key_group, const fw_list_state* src, int64_t n_lists,
                               int64_t n_elems);

/* Synthetic source used by the benchmarks (the same counter-based generator as the CPU
 * baseline and the tests): record i of stream `seed` has
 *   key = splitmix64(seed ^ 4i) mod num_keys  (uniform)  or Zipf(zipf_s) over num_keys,
 *   val = (int32) splitmix64(seed ^ (4i+1)),
 *   ts  = ts_base + floor(i * 1000 / rate) - (splitmix64(seed ^ (4i+2)) mod jitter).
 * Writes records [first, first + n) to device buffers; returns max(ts) over them in *max_ts
 * (device int64, may be NULL).  zipf_cdf (device, num_keys doubles) is used when non-NULL. */
int fw_generate_device(uint64_t seed, int64_t first, int64_t n, int64_t num_keys, const double* zipf_cdf,
                       int64_t ts_base, int64_t rate, int64_t jitter, int64_t* key, int64_t* ts, int64_t* val,
                       int64_t* max_ts, void* stream);

/* ---- Table API OVER windows on row time (fw_over.hip) ----
 * Paths below are relative to flink-libraries/flink-table/src/main/scala/org/apache/flink/table/ ("FT/").  The handle
 * replaces the four ProcessFunctions that FT/plan/nodes/datastream/DataStreamOverAggregate.scala:252-275 builds for
 * `agg OVER (PARTITION BY k ORDER BY rowtime ROWS | RANGE BETWEEN x PRECEDING AND CURRENT ROW)`: one output row per
 * input row, carrying the row's key, row time and arrival ordinal (the host re-attaches the forwarded fields by
 * ordinal) and the aggregates over the row's frame. */
#define FW_OVER_BOUNDED_ROWS 0    /* ROWS BETWEEN preceding PRECEDING AND CURRENT ROW (RowTimeBoundedRowsOver)      */
#define FW_OVER_BOUNDED_RANGE 1   /* RANGE BETWEEN preceding (ms) PRECEDING AND CURRENT ROW (RowTimeBoundedRangeOver) */
#define FW_OVER_UNBOUNDED_ROWS 2  /* ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW (RowTimeUnboundedRowsOver)    */
#define FW_OVER_UNBOUNDED_RANGE 3 /* RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW (RowTimeUnboundedRangeOver)  */

typedef struct fw_over fw_over;
typedef struct fw_over_config {
  int32_t kind;                /* FW_OVER_* */
  int32_t key_kind;            /* FW_KEY_* */
  int32_t max_parallelism;
  int32_t key_group_start;     /* the handle's KeyGroupRange, inclusive */
  int32_t key_group_end;
  int32_t device;
  int32_t row_columns;         /* value columns per row, 1 .. 8 (FW_AGG_ROW's encoding)            */
  int32_t row_aggregates;      /* aggregates per output row, 1 .. 16                                */
  int32_t row_column_type[8];  /* FW_VAL_* of each column                                           */
  int32_t row_aggregate[16];   /* FW_ROW_* << 8 | column                                            */
  int64_t preceding;           /* ROWS: N in [0, 2^31); RANGE: t >= 0 ms; ignored by unbounded kinds */
  int64_t expected_keys;       /* sizes the key map at creation (it grows); 0 = default             */
  int64_t max_batch;           /* largest push; 0 = default                                         */
} fw_over_config;

/* output rows: values[i * row_aggregates + s] (integers sign-extended, Double results as f64 bits), null_mask[i]
 * bit s = aggregate s is NULL */
typedef struct fw_over_rows {
  int64_t* key;
  int64_t* rowtime;
  int64_t* ordinal;
  int64_t* values;
  uint32_t* null_mask;
} fw_over_rows;

typedef struct fw_over_stats {
  int64_t rows_kept;          /* pushed rows stored                                                  */
  int64_t late_rows_dropped;  /* pushed rows dropped as late (no side output in the reference)       */
  int64_t keys;               /* keys with state                                                     */
  int64_t retained_rows;      /* fired rows kept for later frames (bounded kinds)                    */
  int64_t pending_rows;       /* stored rows that have not fired                                     */
  int64_t current_watermark;
  int64_t fired_rows_total;
  int64_t pending_output_rows;
} fw_over_stats;

/* keyed state of one key group.  Per key: last_ts = lastTriggeringTs (bounded kinds; 0 otherwise), acc = the unbounded
 * kinds' accumulator Row as FW_OVER_ACC_WORDS(row_columns) words: the rows accumulated, then per column its non-null
 * count, the sum's low and high words (Double: the f64 sum, 0), min and max (0 when the count is 0).  The
 * bounded kinds' accumulators are functions of the retained rows: their words are zero, but for the sum word of a
 * Double column with a SUM / AVG while the key's last emitted sum is NaN or infinite (it holds that sum, which the
 * reference's retracting accumulator never loses again); a snapshot of all zeros restores as it always did.  n_rows[i] rows of key i follow each other in
 * the row columns (retained and pending rows in arrival order): cols[r * row_columns + j], nulls[r] bit j. */
#define FW_OVER_ACC_WORDS(columns) (1 + 5 * (columns))
typedef struct fw_over_state {
  int64_t* key;
  int64_t* last_ts;
  int64_t* acc;
  int64_t* n_rows;
  int64_t* ts;
  int64_t* ordinal;
  int64_t* cols;
  uint8_t* nulls;
} fw_over_state;

/* open() of the ProcessFunction.  Refused before the GPU is touched: an unknown kind, ROWS preceding outside
 * [0, 2^31), RANGE preceding < 0, zero or too many columns / aggregates, a bad key group range (FW_ERR_ARG); Float
 * SUM / AVG (FW_ERR_UNSUPPORTED: the reference rounds to float after every accumulate and retract).  A failed create
 * returns a handle that carries the message (fw_over_last_error) and must be destroyed. */
int fw_over_create(const fw_over_config* cfg, fw_over** out);
void fw_over_destroy(fw_over* op);
/* the handle's last message.  fw_last_error takes an fw_op and does not serve an fw_over (as fw_list_last_error) */
const char* fw_over_last_error(const fw_over* op);
/* processElement (RowTimeBoundedRangeOver.scala:109-138, RowTimeBoundedRowsOver.scala:118-147,
 * RowTimeUnboundedOver.scala:103-129) for n rows: a bounded kind keeps a row iff rowtime > the key's
 * lastTriggeringTs (0 for a fresh key), an unbounded kind iff rowtime > the current watermark; other rows are dropped
 * and counted.  Row i of the push gets arrival ordinal (rows pushed so far) + i, dropped rows included.  cols:
 * column-major (cols + j * n = column j), nulls: bit j of nulls[i] = column j is NULL (NULL = none).  A
 * Long.MIN_VALUE row time: FW_ERR_NO_TIMESTAMP; a key outside the KeyGroupRange: FW_ERR_KEY_GROUP; rows that cannot
 * be stored: FW_ERR_CAPACITY; in each case the whole push is refused and nothing changed. */
int fw_over_push_batch(fw_over* op, const int64_t* key, const int64_t* rowtime, const int64_t* cols,
                       const uint8_t* nulls, const int32_t* key_hash, int64_t n);
int fw_over_push_batch_device(fw_over* op, const int64_t* key, const int64_t* rowtime, const int64_t* cols,
                              const uint8_t* nulls, const int32_t* key_hash, int64_t n);
/* onTimer for every registered row time <= wm (RowTimeBoundedRangeOver.scala:140-247, RowTimeBoundedRowsOver.scala
 * :149-267, RowTimeUnboundedOver.scala:140-211 and :267-335): the rows that fire are appended to the pending output,
 * a key's rows in (row time, arrival) order; *n_rows (may be NULL) = rows this call emitted.  A watermark lower than
 * the current one: FW_ERR_ARG. */
int fw_over_advance_watermark(fw_over* op, int64_t wm, int64_t* n_rows);
/* copies up to cap pending output rows to host buffers and removes them; epoch[i] (may be NULL) = the number of the
 * fw_over_advance_watermark call that emitted row i (0-based) */
int fw_over_drain(fw_over* op, const fw_over_rows* dst, int64_t* epoch, int64_t cap, int64_t* n);
/* the pending output rows in HBM (valid until the next call on the handle); they stay pending */
int fw_over_rows_device(fw_over* op, fw_over_rows* rows, int64_t* n);
/* discards the pending output rows (a sink that read them through fw_over_rows_device) */
int fw_over_clear_pending(fw_over* op);
int fw_over_get_stats(fw_over* op, fw_over_stats* out);
/* snapshotState / initializeState of the keyed state (lastTriggeringTs, the accumulator Row, the MapState of rows).
 * Snapshot: *n_keys / *n_rows = the key group's totals; the columns are written when dst is non-NULL and both
 * capacities suffice.  Restore works into any parallelism; refused with nothing changed: key_group outside the
 * handle's range or a Long / Integer key that is not in key_group (FW_ERR_KEY_GROUP); a key that occurs twice or
 * already has state (FW_ERR_STATE).  Later pushes are numbered after the largest restored ordinal.  The watermark is
 * not keyed state: a restored handle starts at Long.MIN_VALUE, as the reference's timer service does, and the host
 * advances it to the job's watermark again before it pushes on (the unbounded kinds test rows against it). */
int fw_over_snapshot_key_group(fw_over* op, int32_t key_group, const fw_over_state* dst, int64_t cap_keys,
                               int64_t cap_rows, int64_t* n_keys, int64_t* n_rows);
int fw_over_restore_key_group(fw_over* op, int32_t key_group, const fw_over_state* src, int64_t n_keys,
                              int64_t n_rows);

/* ---- Table API time-windowed (interval) join on row time (fw_tjoin.hip) ----
 * `l JOIN r ON l.k = r.k AND l.rowtime BETWEEN r.rowtime + lower AND r.rowtime + upper`, INNER or outer: the handle
 * replaces FT/runtime/join/RowTimeBoundedStreamJoin.scala (TimeBoundedStreamJoin.scala:55-494) inside
 * FT/runtime/operators/KeyedCoProcessOperatorWithWatermarkDelay.scala, as
 * FT/plan/nodes/datastream/DataStreamWindowJoin.scala:279-330 plans it.  It joins on key and row time only; an
 * operator with a further (non-equi) predicate stays on the CPU.  Both inputs are pushed in one tagged batch whose
 * index order is the arrival order across both sides. */
#define FW_TJOIN_INNER 0
#define FW_TJOIN_LEFT 1  /* LEFT OUTER: an unjoined left row leaves null-padded  */
#define FW_TJOIN_RIGHT 2 /* RIGHT OUTER                                          */
#define FW_TJOIN_FULL 3  /* FULL OUTER                                           */

typedef struct fw_tjoin fw_tjoin;
typedef struct fw_tjoin_config {
  int32_t join_type;        /* FW_TJOIN_* */
  int32_t key_kind;         /* FW_KEY_* */
  int32_t max_parallelism;
  int32_t key_group_start;  /* the handle's KeyGroupRange, inclusive */
  int32_t key_group_end;
  int32_t device;
  int64_t lower;            /* leftLowerBound: l.rowtime >= r.rowtime + lower                  */
  int64_t upper;            /* leftUpperBound: l.rowtime <= r.rowtime + upper; lower <= upper   */
  int64_t allowed_lateness; /* >= 0 (the planner passes 0)                                      */
  int64_t expected_keys;    /* sizes the key map at creation (it grows); 0 = default            */
  int64_t max_batch;        /* largest push the scratch is sized for (it grows); 0 = default    */
  int64_t max_pairs;        /* most pending output rows; 0 = 2^30 (as fw_join_config)           */
} fw_tjoin_config;

/* output rows.  left_ord / right_ord: the arrival ordinals of the joined input rows, from one counter over both
 * sides; -1 marks the null-padded side (its rowtime and val are 0).  cause_ord: the input row whose processElement
 * emitted the row, -1 for a clean-up timer; timer_ts: that timer's time (the record's timestamp), -1 otherwise. */
typedef struct fw_tjoin_rows {
  int64_t* key;
  int64_t* left_ord;
  int64_t* right_ord;
  int64_t* left_rowtime;
  int64_t* right_rowtime;
  int64_t* left_val;
  int64_t* right_val;
  int64_t* cause_ord;
  int64_t* timer_ts;
} fw_tjoin_rows;

typedef struct fw_tjoin_stats {
  int64_t rows_in;
  int64_t cached_rows;             /* pushed rows put into a cache                                         */
  int64_t rows_not_cached;         /* pushed rows whose window the operator time had already passed        */
  int64_t pairs;                   /* joined rows emitted                                                  */
  int64_t padded_at_arrival;       /* null-padded rows: an uncached, unjoined row                          */
  int64_t padded_at_scan;          /* ... an expired, unjoined cached row met by a scanning row            */
  int64_t padded_at_timer;         /* ... an expired, unjoined cached row at a clean-up timer              */
  int64_t pairs_with_expired_rows; /* joined rows whose cached partner had expired (it left in that scan)  */
  int64_t gate_skips;              /* pushed rows that did not scan the other cache                        */
  int64_t timers_set;              /* clean-up timer registrations (arrivals and re-registrations)         */
  int64_t store_rows;              /* rows in the two caches now                                           */
  int64_t active_timers;           /* timer states that are set now                                        */
  int64_t current_watermark;
  int64_t pending_output_rows;
} fw_tjoin_stats;

/* keyed state of one key group.  Per key: left_timer / right_timer = leftTimerState / rightTimerState (0 = unset);
 * n_rows[i] rows of key i follow each other in the row columns: side (0 = left cache, 1 = right cache), rowtime,
 * ordinal, val, emitted (the cached tuple's flag). */
typedef struct fw_tjoin_state {
  int64_t* key;
  int64_t* left_timer;
  int64_t* right_timer;
  int64_t* n_rows;
  uint8_t* side;
  int64_t* rowtime;
  int64_t* ordinal;
  int64_t* val;
  uint8_t* emitted;
} fw_tjoin_state;

/* open().  Refused before the GPU is touched (FW_ERR_ARG): an unknown join type, lower > upper (the planner's
 * negative-window-size branch uses no join operator), allowed_lateness < 0, |lower|, |upper| or the lateness >= 2^60,
 * max_pairs < 0, a bad key kind or key group range.  A failed create returns a handle that carries the message
 * (fw_tjoin_last_error) and must be destroyed. */
int fw_tjoin_create(const fw_tjoin_config* cfg, fw_tjoin** out);
void fw_tjoin_destroy(fw_tjoin* op);
const char* fw_tjoin_last_error(const fw_tjoin* op);
/* processElement1 / processElement2 for n tagged rows: side[i] 0 = left, 1 = right; row i gets arrival ordinal (rows
 * pushed so far) + i; val: one carried int64 per row (NULL = zeros).  Joined rows and the null-padded rows that the
 * reference emits from processElement are appended to the pending output.  Refused with nothing changed: a row time
 * < 0 or >= 2^62 (FW_ERR_TIME_RANGE: the reference's behaviour there depends on hash-map iteration order; a row that
 * is cached has rowtime + relativeSize > operator time >= 0, so the clean-up timer it registers is never <= 0 and is
 * never read as unset); a key outside the KeyGroupRange (FW_ERR_KEY_GROUP); a side outside {0, 1} (FW_ERR_ARG);
 * pending rows plus this push's rows above max_pairs (FW_ERR_CAPACITY). */
int fw_tjoin_push_batch(fw_tjoin* op, const uint8_t* side, const int64_t* key, const int64_t* rowtime,
                        const int64_t* val, const int32_t* key_hash, int64_t n);
int fw_tjoin_push_batch_device(fw_tjoin* op, const uint8_t* side, const int64_t* key, const int64_t* rowtime,
                               const int64_t* val, const int32_t* key_hash, int64_t n);
/* onTimer for every clean-up timer <= wm, then the watermark the operator forwards: *forwarded_wm = wm -
 * (max(leftRelativeSize, rightRelativeSize) + allowed_lateness); *n_rows = rows this call emitted (both may be NULL).
 * A watermark lower than the current one: FW_ERR_ARG. */
int fw_tjoin_advance_watermark(fw_tjoin* op, int64_t wm, int64_t* n_rows, int64_t* forwarded_wm);
/* copies up to cap pending output rows to host buffers and removes them; epoch[i] (may be NULL) = the number of
 * fw_tjoin_advance_watermark calls made before row i was emitted (a timer's rows count their own call as not made) */
int fw_tjoin_drain(fw_tjoin* op, const fw_tjoin_rows* dst, int64_t* epoch, int64_t cap, int64_t* n);
/* the pending output rows in HBM (valid until the next call on the handle); they stay pending */
int fw_tjoin_rows_device(fw_tjoin* op, fw_tjoin_rows* rows, int64_t* n);
int fw_tjoin_clear_pending(fw_tjoin* op);
int fw_tjoin_get_stats(fw_tjoin* op, fw_tjoin_stats* out);
/* snapshotState / initializeState of the keyed state (the two MapState caches, the two timer states).  Snapshot:
 * *n_keys / *n_rows = the key group's totals; the columns are written when dst is non-NULL and both capacities
 * suffice.  Restore works into any parallelism; refused with nothing changed: key_group outside the handle's range or
 * a Long / Integer key that is not in key_group (FW_ERR_KEY_GROUP); a key that occurs twice or already has state
 * (FW_ERR_STATE); a key with rows in a cache whose timer is 0 (FW_ERR_ARG: left cache rows come with right_timer,
 * right cache rows with left_timer).  Later pushes are numbered after the largest restored ordinal.  leftExpirationTime,
 * rightExpirationTime and the watermark are not keyed state: a restored handle starts them at 0, 0 and
 * Long.MIN_VALUE, as the reference does. */
int fw_tjoin_snapshot_key_group(fw_tjoin* op, int32_t key_group, const fw_tjoin_state* dst, int64_t cap_keys,
                                int64_t cap_rows, int64_t* n_keys, int64_t* n_rows);
int fw_tjoin_restore_key_group(fw_tjoin* op, int32_t key_group, const fw_tjoin_state* src, int64_t n_keys,
                               int64_t n_rows);

#ifdef __cplusplus
}
#endif
#endif /* FLINK_WINDOW_H */

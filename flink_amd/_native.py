"""ctypes binding of include/flink_window.h (libflinkwin.so, built for gfx950 by
flink_amd/csrc/Makefile).  There is no fallback: if the library is missing the import fails."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FW_LIB selects a diagnostic build variant (tools/variants.sh); the product build is _lib/libflinkwin.so
LIB_PATH = os.environ.get("FW_LIB") or os.path.join(_HERE, "_lib", "libflinkwin.so")
CSRC = os.path.join(_HERE, "csrc")

FW_OK = 0
FW_ERR_ARG = -1
FW_ERR_HIP = -2
FW_ERR_NO_TIMESTAMP = -3
FW_ERR_KEY_GROUP = -4
FW_ERR_CAPACITY = -5
FW_ERR_UNSUPPORTED = -6
FW_ERR_STATE = -7
FW_ERR_DISPLACED = -8
FW_ERR_TIME_RANGE = -9

FW_TUMBLING, FW_SLIDING, FW_SESSION, FW_COUNT = 0, 1, 2, 3
FW_VAL_I64, FW_VAL_I32, FW_VAL_F64, FW_VAL_I16, FW_VAL_I8, FW_VAL_F32 = 0, 1, 2, 3, 4, 5
FW_KEY_LONG, FW_KEY_INT, FW_KEY_HASHED = 0, 1, 2
FW_AGG_COUNT_SUM_MIN_MAX, FW_AGG_HLL, FW_AGG_FIRST, FW_AGG_MINBY, FW_AGG_MAXBY, FW_AGG_FIRST_MAX = 0, 1, 2, 3, 4, 5
FW_AGG_TDIGEST = 6
FW_AGG_ROW = 7
FW_ROW_COUNT_STAR, FW_ROW_COUNT, FW_ROW_SUM, FW_ROW_MIN, FW_ROW_MAX, FW_ROW_AVG = 0, 1, 2, 3, 4, 5
FW_NUM_KERNELS = 7
FW_PROFILE_KINDS = 0x100  # fw_profile(op, FW_PROFILE_KINDS | 1 << kind): time only those kinds

I64P = ctypes.POINTER(ctypes.c_int64)
I32P = ctypes.POINTER(ctypes.c_int32)
VP = ctypes.c_void_p


class FwConfig(ctypes.Structure):
    _fields_ = [("assigner", ctypes.c_int32), ("value_type", ctypes.c_int32), ("key_kind", ctypes.c_int32),
                ("purging", ctypes.c_int32), ("side_output", ctypes.c_int32), ("max_parallelism", ctypes.c_int32),
                ("key_group_start", ctypes.c_int32), ("key_group_end", ctypes.c_int32), ("device", ctypes.c_int32),
                ("sub_partitions", ctypes.c_int32), ("size", ctypes.c_int64), ("slide", ctypes.c_int64),
                ("offset", ctypes.c_int64), ("gap", ctypes.c_int64), ("allowed_lateness", ctypes.c_int64),
                ("expected_entries", ctypes.c_int64), ("max_batch", ctypes.c_int64),
                ("aggregate", ctypes.c_int32), ("hll_precision", ctypes.c_int32),
                ("tdigest_compression", ctypes.c_int32), ("tdigest_export", ctypes.c_int32),
                ("tdigest_quantiles", ctypes.c_double * 3), ("count_evict_after", ctypes.c_int32),
                ("pad0", ctypes.c_int32), ("row_columns", ctypes.c_int32), ("row_aggregates", ctypes.c_int32),
                ("row_column_type", ctypes.c_int32 * 8), ("row_aggregate", ctypes.c_int32 * 16),
                ("no_panes", ctypes.c_int32), ("trigger", ctypes.c_int32), ("trigger_interval", ctypes.c_int64)]


class FwRows(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("key", "start", "end", "count", "sum", "min", "max")]


class FwPartials(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("key", "start", "cnt", "sum", "min", "max")] + [("config", ctypes.c_uint64)]


class FwSideRows(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("key", "ts", "val")]


class FwStateRows(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("key", "start", "end", "count", "sum", "min", "max", "timer")]


class FwStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        "records_in", "late_records_dropped", "keyed_state_entries", "event_time_timers", "current_watermark",
        "fired_rows_total", "pending_rows", "pending_side_rows", "table_capacity", "table_grows",
        "slow_path_records", "state_merges", "digest_centroids_fired", "single_pass_batches",
        "single_pass_redone", "narrow_pass_batches", "narrow_pass_redone", "push_resumptions")]


FW_WIRE_LONG, FW_WIRE_INT, FW_WIRE_DOUBLE, FW_WIRE_SHORT, FW_WIRE_BYTE, FW_WIRE_FLOAT, FW_WIRE_BOOL, FW_WIRE_STRING = range(8)
(FW_ROLE_SKIP, FW_ROLE_KEY, FW_ROLE_VALUE, FW_ROLE_START, FW_ROLE_END, FW_ROLE_COUNT, FW_ROLE_SUM, FW_ROLE_MIN,
 FW_ROLE_MAX) = range(9)


class FwCommStats(ctypes.Structure):
    _fields_ = [("world", ctypes.c_int32), ("rank", ctypes.c_int32)] + [(n, ctypes.c_int64) for n in (
        "batches", "items_sent", "items_received", "bytes_sent", "bytes_received", "recv_reallocs", "recv_capacity")]


class FwExchangePlan(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ("send_total", "recv_total", "items_sent", "items_received",
                                               "recv_bound")]


class FwWireLayout(ctypes.Structure):
    _fields_ = [("nfields", ctypes.c_int32), ("kind", ctypes.c_int32 * 8), ("role", ctypes.c_int32 * 8)]


class FwWireStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ("records", "watermarks", "latency_markers", "statuses", "consumed",
                                               "watermark")] + [("status", ctypes.c_int32), ("pad", ctypes.c_int32)]


FW_GLOBAL = 4
FW_TRIGGER_EVENT_TIME, FW_TRIGGER_COUNT, FW_TRIGGER_CONTINUOUS_EVENT_TIME, FW_TRIGGER_DELTA = 0, 1, 2, 3
FW_EVICT_NONE, FW_EVICT_COUNT, FW_EVICT_TIME, FW_EVICT_DELTA = 0, 1, 2, 3


class FwListConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "assigner", "value_type", "key_kind", "trigger", "purging", "evictor", "evict_after", "side_output",
        "emit_contents", "max_parallelism", "key_group_start", "key_group_end", "device", "merging_state")] + \
        [(n, ctypes.c_int64) for n in ("size", "slide", "offset", "allowed_lateness", "trigger_count",
                                       "evict_count")] + \
        [("delta_threshold", ctypes.c_double), ("expected_elements", ctypes.c_int64), ("max_batch", ctypes.c_int64),
         ("trigger_interval", ctypes.c_int64)]

    # fw_list_config's last slot is a union: ContinuousEventTimeTrigger's trigger_interval or, for FW_TRIGGER_DELTA,
    # DeltaTrigger's trigger_threshold (a double in the same eight bytes)
    @property
    def trigger_threshold(self):
        return ctypes.c_double.from_buffer_copy(ctypes.c_int64(self.trigger_interval)).value

    @trigger_threshold.setter
    def trigger_threshold(self, x):
        self.trigger_interval = ctypes.c_int64.from_buffer_copy(ctypes.c_double(x)).value


FW_JOIN_NONE, FW_JOIN_COGROUP, FW_JOIN_INNER = 0, 1, 2
FW_ORD_SIDE = 1 << 62  # an element's input on a join handle: bit 62 of its arrival ordinal (set = input 2)


class FwJoinConfig(ctypes.Structure):
    _fields_ = [("join", ctypes.c_int32), ("pad", ctypes.c_int32), ("max_join_pairs", ctypes.c_int64)]


class FwJoinPairs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("row", "idx1", "idx2", "val1", "val2")]


class FwListRows(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("key", "start", "end", "count", "sum", "min", "max", "first",
                                               "elem_off")]


class FwListElems(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("ts", "val", "ordinal")]


class FwListState(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("key", "start", "end", "trigger_count", "timer", "n_elems", "ts", "val",
                                               "ordinal")]


class FwSessionState(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("key", "start", "end", "state_start", "state_end", "trigger_state",
                                               "timer", "n_elems", "ts", "val", "ordinal")]


FW_OVER_BOUNDED_ROWS, FW_OVER_BOUNDED_RANGE, FW_OVER_UNBOUNDED_ROWS, FW_OVER_UNBOUNDED_RANGE = 0, 1, 2, 3


class FwOverConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("kind", "key_kind", "max_parallelism", "key_group_start",
                                              "key_group_end", "device", "row_columns", "row_aggregates")] + \
        [("row_column_type", ctypes.c_int32 * 8), ("row_aggregate", ctypes.c_int32 * 16)] + \
        [(n, ctypes.c_int64) for n in ("preceding", "expected_keys", "max_batch")]


class FwOverRows(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("key", "rowtime", "ordinal", "values", "null_mask")]


class FwOverStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ("rows_kept", "late_rows_dropped", "keys", "retained_rows",
                                              "pending_rows", "current_watermark", "fired_rows_total",
                                              "pending_output_rows")]


class FwOverState(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("key", "last_ts", "acc", "n_rows", "ts", "ordinal", "cols", "nulls")]


def fw_over_acc_words(columns):
    return 1 + 5 * columns


FW_TJOIN_INNER, FW_TJOIN_LEFT, FW_TJOIN_RIGHT, FW_TJOIN_FULL = 0, 1, 2, 3


class FwTjoinConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("join_type", "key_kind", "max_parallelism", "key_group_start",
                                              "key_group_end", "device")] + \
        [(n, ctypes.c_int64) for n in ("lower", "upper", "allowed_lateness", "expected_keys", "max_batch",
                                       "max_pairs")]


class FwTjoinRows(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("key", "left_ord", "right_ord", "left_rowtime", "right_rowtime",
                                               "left_val", "right_val", "cause_ord", "timer_ts")]


class FwTjoinStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in (
        "rows_in", "cached_rows", "rows_not_cached", "pairs", "padded_at_arrival", "padded_at_scan",
        "padded_at_timer", "pairs_with_expired_rows", "gate_skips", "timers_set", "store_rows", "active_timers",
        "current_watermark", "pending_output_rows")]


class FwTjoinState(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("key", "left_timer", "right_timer", "n_rows", "side", "rowtime",
                                               "ordinal", "val", "emitted")]


# every exported symbol with its ctypes signature (restype, argtypes); mirrors include/flink_window.h
SIGNATURES = {
    "fw_create": (ctypes.c_int, [ctypes.POINTER(FwConfig), ctypes.POINTER(VP)]),
    "fw_destroy": (None, [VP]),
    "fw_last_error": (ctypes.c_char_p, [VP]),
    "fw_push_batch": (ctypes.c_int, [VP, VP, VP, VP, VP, ctypes.c_int64]),
    "fw_push_batch_device": (ctypes.c_int, [VP, VP, VP, VP, VP, ctypes.c_int64]),
    "fw_advance_watermark": (ctypes.c_int, [VP, ctypes.c_int64, I64P]),
    "fw_pending": (ctypes.c_int, [VP, I64P, I64P]),
    "fw_drain_rows": (ctypes.c_int, [VP, ctypes.POINTER(FwRows), ctypes.c_int64, I64P]),
    "fw_drain_side": (ctypes.c_int, [VP, ctypes.POINTER(FwSideRows), ctypes.c_int64, I64P]),
    "fw_rows_device": (ctypes.c_int, [VP, ctypes.POINTER(FwRows), I64P]),
    "fw_clear_pending": (ctypes.c_int, [VP]),
    "fw_drain_digests": (ctypes.c_int, [VP, VP, VP, VP, ctypes.c_int64, I64P]),
    "fw_push_row_batch": (ctypes.c_int, [VP, VP, VP, VP, VP, VP, ctypes.c_int64]),
    "fw_push_row_batch_device": (ctypes.c_int, [VP, VP, VP, VP, VP, VP, ctypes.c_int64]),
    "fw_drain_row_results": (ctypes.c_int, [VP, VP, VP, ctypes.c_int64, I64P]),
    "fw_get_stats": (ctypes.c_int, [VP, ctypes.POINTER(FwStats)]),
    "fw_synchronize": (ctypes.c_int, [VP]),
    "fw_profile": (ctypes.c_int, [VP, ctypes.c_int]),
    "fw_profile_read": (ctypes.c_int, [VP, ctypes.POINTER(ctypes.c_double), I64P, ctypes.c_int]),
    "fw_kernel_name": (ctypes.c_char_p, [ctypes.c_int]),
    "fw_stream": (VP, [VP]),
    "fw_set_async_input": (ctypes.c_int, [VP, ctypes.c_int]),
    "fw_input_stream": (VP, [VP]),
    "fw_combine_extract_device": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwPartials), ctypes.c_int64, I64P,
                                                 I64P]),
    "fw_push_partials_device": (ctypes.c_int, [VP, ctypes.POINTER(FwPartials), ctypes.c_int64]),
    "fw_combine_extract_hll_device": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwPartials), ctypes.c_int64,
                                                     I64P, I64P, I64P, I64P]),
    "fw_combine_hll_registers_device": (ctypes.c_int, [VP, ctypes.POINTER(FwPartials), ctypes.c_int64, VP,
                                                       ctypes.c_int64]),
    "fw_push_hll_partials_device": (ctypes.c_int, [VP, ctypes.POINTER(FwPartials), ctypes.c_int64, VP, ctypes.c_int64]),
    "fw_keyby_combine_push_device": (ctypes.c_int, [VP, VP, VP, VP, VP, VP, ctypes.c_int64, ctypes.c_int64, I64P]),
    "fw_snapshot_key_group": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwStateRows), ctypes.c_int64, I64P]),
    "fw_restore_key_group": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwStateRows), ctypes.c_int64]),
    "fw_state_block_bytes": (ctypes.c_int64, [VP]),
    "fw_snapshot_key_group_blocks": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwStateRows), VP,
                                                    ctypes.c_int64, I64P]),
    "fw_restore_key_group_blocks": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwStateRows), VP,
                                                   ctypes.c_int64]),
    "fw_snapshot_key_group_fire": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwStateRows), VP,
                                                  ctypes.c_int64, I64P]),
    "fw_restore_key_group_fire": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwStateRows), VP,
                                                 ctypes.c_int64]),
    "fw_create_count_trigger": (ctypes.c_int, [ctypes.POINTER(FwConfig), ctypes.c_int64, ctypes.POINTER(VP)]),
    "fw_snapshot_key_group_trigger_count": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwStateRows), VP,
                                                           ctypes.c_int64, I64P]),
    "fw_restore_key_group_trigger_count": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwStateRows), VP,
                                                          ctypes.c_int64]),
    "fw_key_groups_device": (ctypes.c_int, [VP, VP, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, VP, VP]),
    "fw_route_device": (ctypes.c_int, [VP, VP, VP, VP, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                       ctypes.c_int32, VP, VP, VP, VP, VP, VP, ctypes.c_int64, VP]),
    "fw_route_scratch_bytes": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    "fw_comm_unique_id": (ctypes.c_int, [VP]),
    "fw_comm_init": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(VP)]),
    "fw_comm_destroy": (None, [VP]),
    "fw_keyby_push_device": (ctypes.c_int, [VP, VP, VP, VP, VP, VP, ctypes.c_int64, ctypes.c_int64, I64P]),
    "fw_comm_get_stats": (ctypes.c_int, [VP, ctypes.POINTER(FwCommStats)]),
    "fw_exchange_plan": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, I64P, I64P, I64P,
                                        ctypes.POINTER(FwExchangePlan)]),
    "fw_wire_create": (ctypes.c_int, [ctypes.POINTER(FwWireLayout), ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(VP)]),
    "fw_wire_destroy": (None, [VP]),
    "fw_wire_last_error": (ctypes.c_char_p, [VP]),
    "fw_wire_decode_device": (ctypes.c_int, [VP, VP, ctypes.c_int64, VP, VP, VP, ctypes.c_int64,
                                             ctypes.POINTER(FwWireStats)]),
    "fw_wire_decode_keyed_device": (ctypes.c_int, [VP, VP, ctypes.c_int64, VP, VP, VP, VP, ctypes.c_int64,
                                             ctypes.POINTER(FwWireStats)]),
    "fw_wire_encode_device": (ctypes.c_int, [VP, ctypes.POINTER(FwRows), ctypes.c_int64, ctypes.c_int32, VP,
                                             ctypes.c_int64, I64P]),
    "fw_list_create": (ctypes.c_int, [ctypes.POINTER(FwListConfig), ctypes.POINTER(VP)]),
    "fw_list_create_join": (ctypes.c_int, [ctypes.POINTER(FwListConfig), ctypes.POINTER(FwJoinConfig),
                                           ctypes.POINTER(VP)]),
    "fw_list_destroy": (None, [VP]),
    "fw_list_last_error": (ctypes.c_char_p, [VP]),
    "fw_list_push_batch": (ctypes.c_int, [VP, VP, VP, VP, VP, ctypes.c_int64]),
    "fw_list_push_batch_device": (ctypes.c_int, [VP, VP, VP, VP, VP, ctypes.c_int64]),
    "fw_list_push_batch_side": (ctypes.c_int, [VP, ctypes.c_int32, VP, VP, VP, VP, ctypes.c_int64]),
    "fw_list_push_batch_side_device": (ctypes.c_int, [VP, ctypes.c_int32, VP, VP, VP, VP, ctypes.c_int64]),
    "fw_list_join_pending": (ctypes.c_int, [VP, I64P, I64P, I64P]),
    "fw_list_drain_join": (ctypes.c_int, [VP, ctypes.POINTER(FwListRows), VP, ctypes.c_int64,
                                          ctypes.POINTER(FwListElems), ctypes.c_int64, ctypes.POINTER(FwJoinPairs),
                                          ctypes.c_int64, I64P, I64P, I64P]),
    "fw_list_join_device": (ctypes.c_int, [VP, ctypes.POINTER(FwListRows), ctypes.POINTER(VP),
                                           ctypes.POINTER(FwListElems), ctypes.POINTER(FwJoinPairs), I64P, I64P, I64P]),
    "fw_list_advance_watermark": (ctypes.c_int, [VP, ctypes.c_int64, I64P]),
    "fw_list_pending": (ctypes.c_int, [VP, I64P, I64P, I64P]),
    "fw_list_drain": (ctypes.c_int, [VP, ctypes.POINTER(FwListRows), ctypes.c_int64, ctypes.POINTER(FwListElems),
                                     ctypes.c_int64, I64P, I64P]),
    "fw_list_clear_pending": (ctypes.c_int, [VP]),
    "fw_list_drain_side": (ctypes.c_int, [VP, ctypes.POINTER(FwSideRows), ctypes.c_int64, I64P]),
    "fw_list_get_stats": (ctypes.c_int, [VP, ctypes.POINTER(FwStats)]),
    "fw_list_snapshot_key_group": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwListState), ctypes.c_int64,
                                                  ctypes.c_int64, I64P, I64P]),
    "fw_list_restore_key_group": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwListState), ctypes.c_int64,
                                                 ctypes.c_int64]),
    "fw_list_snapshot_sessions": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwSessionState), ctypes.c_int64,
                                                 ctypes.c_int64, I64P, I64P]),
    "fw_list_restore_sessions": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwSessionState), ctypes.c_int64,
                                                ctypes.c_int64]),
    "fw_count_snapshot_key_group": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwListState), ctypes.c_int64,
                                                   ctypes.c_int64, I64P, I64P]),
    "fw_count_restore_key_group": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwListState), ctypes.c_int64,
                                                  ctypes.c_int64]),
    "fw_over_create": (ctypes.c_int, [ctypes.POINTER(FwOverConfig), ctypes.POINTER(VP)]),
    "fw_over_destroy": (None, [VP]),
    "fw_over_last_error": (ctypes.c_char_p, [VP]),
    "fw_over_push_batch": (ctypes.c_int, [VP, VP, VP, VP, VP, VP, ctypes.c_int64]),
    "fw_over_push_batch_device": (ctypes.c_int, [VP, VP, VP, VP, VP, VP, ctypes.c_int64]),
    "fw_over_advance_watermark": (ctypes.c_int, [VP, ctypes.c_int64, I64P]),
    "fw_over_drain": (ctypes.c_int, [VP, ctypes.POINTER(FwOverRows), VP, ctypes.c_int64, I64P]),
    "fw_over_rows_device": (ctypes.c_int, [VP, ctypes.POINTER(FwOverRows), I64P]),
    "fw_over_clear_pending": (ctypes.c_int, [VP]),
    "fw_over_get_stats": (ctypes.c_int, [VP, ctypes.POINTER(FwOverStats)]),
    "fw_over_snapshot_key_group": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwOverState), ctypes.c_int64,
                                                  ctypes.c_int64, I64P, I64P]),
    "fw_over_restore_key_group": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwOverState), ctypes.c_int64,
                                                 ctypes.c_int64]),
    "fw_tjoin_create": (ctypes.c_int, [ctypes.POINTER(FwTjoinConfig), ctypes.POINTER(VP)]),
    "fw_tjoin_destroy": (None, [VP]),
    "fw_tjoin_last_error": (ctypes.c_char_p, [VP]),
    "fw_tjoin_push_batch": (ctypes.c_int, [VP, VP, VP, VP, VP, VP, ctypes.c_int64]),
    "fw_tjoin_push_batch_device": (ctypes.c_int, [VP, VP, VP, VP, VP, VP, ctypes.c_int64]),
    "fw_tjoin_advance_watermark": (ctypes.c_int, [VP, ctypes.c_int64, I64P, I64P]),
    "fw_tjoin_drain": (ctypes.c_int, [VP, ctypes.POINTER(FwTjoinRows), VP, ctypes.c_int64, I64P]),
    "fw_tjoin_rows_device": (ctypes.c_int, [VP, ctypes.POINTER(FwTjoinRows), I64P]),
    "fw_tjoin_clear_pending": (ctypes.c_int, [VP]),
    "fw_tjoin_get_stats": (ctypes.c_int, [VP, ctypes.POINTER(FwTjoinStats)]),
    "fw_tjoin_snapshot_key_group": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwTjoinState), ctypes.c_int64,
                                                   ctypes.c_int64, I64P, I64P]),
    "fw_tjoin_restore_key_group": (ctypes.c_int, [VP, ctypes.c_int32, ctypes.POINTER(FwTjoinState), ctypes.c_int64,
                                                  ctypes.c_int64]),
    "fw_generate_device": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, VP,
                                          ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, VP, VP, VP, VP, VP]),
}

_lib = None


class NativeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


def lib():
    """Load libflinkwin.so.  Raises if it was not built — the GPU path has no CPU fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `make -C {CSRC}` "
                              "(or __graft_entry__.build()); flink_amd has no CPU fallback")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, handle=None):
    if rc != FW_OK:
        msg = lib().fw_last_error(handle).decode() if handle else "error"
        raise NativeError(rc, msg)
    return rc

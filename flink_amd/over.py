"""Table API OVER windows on row time on the GPU path -- the host mirror of the four ProcessFunctions that
flink-libraries/flink-table/src/main/scala/org/apache/flink/table/plan/nodes/datastream/DataStreamOverAggregate.scala
:252-275 builds (runtime/aggregate/RowTimeBounded{Rows,Range}Over.scala, RowTimeUnboundedOver.scala):
`agg OVER (PARTITION BY key ORDER BY rowtime ROWS | RANGE BETWEEN x PRECEDING AND CURRENT ROW)`.  One output row per
input row: (key, rowtime, arrival ordinal, aggregates over the row's frame); the host re-attaches the row's forwarded
fields by ordinal.  The planner's rewrite needs the JVM and is not rebuilt; a host that has planned a query hands the
frame and the select list to OverAggregate.
"""
import ctypes

import numpy as np

from . import _native as N
from ._handle import _TableHandle
from .table import _decode
from .windowing import FLOAT_TYPES, ROW_FUNCTIONS, VALUE_TYPES, _ms

_KEY_KINDS = {"long": N.FW_KEY_LONG, "int": N.FW_KEY_INT, "hashed": N.FW_KEY_HASHED}


class Over:
    """The frame: Over.rows(n) = ROWS BETWEEN n PRECEDING AND CURRENT ROW, Over.range(ms) = RANGE BETWEEN INTERVAL ms
    PRECEDING AND CURRENT ROW, Over.unbounded_rows() / Over.unbounded_range() = ... UNBOUNDED PRECEDING ..."""

    def __init__(self, kind, preceding=0):
        self.kind, self.preceding = kind, preceding

    @staticmethod
    def rows(n):
        return Over(N.FW_OVER_BOUNDED_ROWS, int(n))

    @staticmethod
    def range(ms):
        return Over(N.FW_OVER_BOUNDED_RANGE, _ms(ms))

    @staticmethod
    def unbounded_rows():
        return Over(N.FW_OVER_UNBOUNDED_ROWS)

    @staticmethod
    def unbounded_range():
        return Over(N.FW_OVER_UNBOUNDED_RANGE)


def over_config(frame, column_types, aggregates, key_type="long", max_parallelism=128, key_group_range=None, device=0,
                expected_keys=0, max_batch=0):
    c = N.FwOverConfig()
    c.kind, c.preceding = frame.kind, frame.preceding
    c.key_kind = _KEY_KINDS[key_type]
    c.max_parallelism = max_parallelism
    c.key_group_start, c.key_group_end = key_group_range if key_group_range is not None else (0, max_parallelism - 1)
    c.device = device
    c.row_columns, c.row_aggregates = len(column_types), len(aggregates)
    for j, t in enumerate(column_types[:8]):
        c.row_column_type[j] = VALUE_TYPES[t]
    for q, (f, col) in enumerate(aggregates[:16]):
        c.row_aggregate[q] = (ROW_FUNCTIONS[f] << 8) | int(col)
    c.expected_keys, c.max_batch = expected_keys, max_batch
    return c


class OverAggregate(_TableHandle):
    """One keyed row-time OVER aggregation.  `column_types`: the aggregated columns' types ("long", "int", "short",
    "byte", "double"; "float" for COUNT / MIN / MAX only); `aggregates`: [(function, column index)], function one of
    count_star, count, sum, min, max, avg.  process(keys, rowtimes, columns, nulls[, key_hash]) takes numpy arrays or
    CUDA tensors; watermark(wm) returns the rows it emits as [(key, rowtime, ordinal, [values, None = NULL])], a key's
    rows in (rowtime, arrival) order."""
    _prefix, _Rows, _Stats = "fw_over", N.FwOverRows, N.FwOverStats

    def __init__(self, frame, column_types, aggregates, key_type="long", **kw):
        self.column_types = tuple(column_types)
        self.aggregates = tuple((f, int(c)) for f, c in aggregates)
        self.frame = frame
        cfg = over_config(frame, self.column_types, self.aggregates, key_type=key_type, **kw)
        self._create(cfg)
        self.epoch = 0

    def process(self, keys, rowtimes, columns, nulls=None, key_hash=None):
        L = N.lib()
        nc = len(self.column_types)
        if hasattr(keys, "data_ptr"):
            import torch
            n = keys.numel()
            mat = columns if hasattr(columns, "data_ptr") else torch.stack(
                [c.view(torch.int64) if c.dtype == torch.float64 else c for c in columns])
            if mat.dtype == torch.float64:
                mat = mat.view(torch.int64)
            mat = mat.contiguous()
            if tuple(mat.shape) != (nc, n) or mat.dtype != torch.int64 or not mat.is_cuda:
                raise ValueError(f"columns must be {nc} int64 / float64 CUDA columns of {n} values")
            if nulls is not None and (nulls.dtype != torch.uint8 or nulls.numel() != n or not nulls.is_cuda):
                raise ValueError("nulls must be a uint8 CUDA tensor, one mask per row")
            for t in (keys, rowtimes) + ((key_hash,) if key_hash is not None else ()):
                if not t.is_cuda or not t.is_contiguous() or t.numel() != n:
                    raise ValueError("device columns must be contiguous CUDA tensors of equal length")
            torch.cuda.current_stream(keys.device).synchronize()  # the columns' producers; the push settles its own
            self._check(L.fw_over_push_batch_device(self._h, keys.data_ptr(), rowtimes.data_ptr(), mat.data_ptr(),
                                                    nulls.data_ptr() if nulls is not None else None,
                                                    key_hash.data_ptr() if key_hash is not None else None, n))
            return
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        rowtimes = np.ascontiguousarray(rowtimes, dtype=np.int64)
        n = len(keys)
        if len(columns) != nc:
            raise ValueError(f"columns must be {nc} columns of {n} values")
        # a "double" / "float" column travels as f64 bits (a Float as the double of the float), the others as int64
        mat = np.ascontiguousarray(np.stack([
            np.ascontiguousarray(c, dtype=np.float64).view(np.int64) if t in FLOAT_TYPES else np.asarray(c, dtype=np.int64)
            for c, t in zip(columns, self.column_types)])) if n else np.zeros((nc, 0), dtype=np.int64)
        if mat.shape != (nc, n) or len(rowtimes) != n:
            raise ValueError(f"columns must be {nc} columns of {n} values")
        nm = kh = None
        if nulls is not None:
            nulls = np.ascontiguousarray(nulls, dtype=np.uint8)
            nm = nulls.ctypes.data
        if key_hash is not None:
            key_hash = np.ascontiguousarray(key_hash, dtype=np.int32)
            kh = key_hash.ctypes.data
        self._check(L.fw_over_push_batch(self._h, keys.ctypes.data, rowtimes.ctypes.data, mat.ctypes.data, nm, kh, n))

    def advance_watermark(self, wm):
        n = ctypes.c_int64()
        self._check(N.lib().fw_over_advance_watermark(self._h, int(wm), ctypes.byref(n)))
        self.epoch += 1
        return n.value

    def rows_device(self):
        """The pending output rows where they are, in HBM: (FwOverRows of device pointers, rows).  Valid until the
        next call on the handle; the rows stay pending (clear_pending() discards them)."""
        return self._rows_device()

    def drain_arrays(self):
        """The pending output rows as arrays: key, rowtime, ordinal, values [rows, aggregates], null_mask, epoch."""
        st = self.stats()
        n = st["pending_output_rows"]
        ns = len(self.aggregates)
        out = {"key": np.empty(n, np.int64), "rowtime": np.empty(n, np.int64), "ordinal": np.empty(n, np.int64),
               "values": np.empty((n, ns), np.int64), "null_mask": np.empty(n, np.uint32),
               "epoch": np.empty(n, np.int64)}
        dst = N.FwOverRows(*(out[f].ctypes.data for f in ("key", "rowtime", "ordinal", "values", "null_mask")))
        got = ctypes.c_int64()
        self._check(N.lib().fw_over_drain(self._h, ctypes.byref(dst), out["epoch"].ctypes.data, n, ctypes.byref(got)))
        assert got.value == n
        return out

    def watermark(self, wm):
        self.advance_watermark(wm)
        a = self.drain_arrays()
        out = []
        for i in range(len(a["key"])):
            nm = int(a["null_mask"][i])
            v = [None if (nm >> q) & 1 else _decode(f, self.column_types[c], a["values"][i][q])
                 for q, (f, c) in enumerate(self.aggregates)]
            out.append((int(a["key"][i]), int(a["rowtime"][i]), int(a["ordinal"][i]), v))
        return out

    def snapshot(self, kg):
        """The keyed state of key group kg: {"key", "last_ts", "acc" [keys, words], "n_rows", "ts", "ordinal",
        "cols" [rows, columns], "nulls"} (numpy)."""
        L = N.lib()
        nk, nr = ctypes.c_int64(), ctypes.c_int64()
        self._check(L.fw_over_snapshot_key_group(self._h, kg, None, 0, 0, ctypes.byref(nk), ctypes.byref(nr)))
        k, r, nc = nk.value, nr.value, len(self.column_types)
        w = N.fw_over_acc_words(nc)
        st = {"key": np.zeros(k, np.int64), "last_ts": np.zeros(k, np.int64), "acc": np.zeros((k, w), np.int64),
              "n_rows": np.zeros(k, np.int64), "ts": np.zeros(r, np.int64), "ordinal": np.zeros(r, np.int64),
              "cols": np.zeros((r, nc), np.int64), "nulls": np.zeros(r, np.uint8)}
        dst = N.FwOverState(*(st[f].ctypes.data for f, _ in N.FwOverState._fields_))
        self._check(L.fw_over_snapshot_key_group(self._h, kg, ctypes.byref(dst), k, r, ctypes.byref(nk),
                                                 ctypes.byref(nr)))
        return st

    def restore(self, kg, state):
        st = {f: np.ascontiguousarray(state[f], dtype=np.uint8 if f == "nulls" else np.int64)
              for f, _ in N.FwOverState._fields_}
        src = N.FwOverState(*(st[f].ctypes.data for f, _ in N.FwOverState._fields_))
        self._check(N.lib().fw_over_restore_key_group(self._h, kg, ctypes.byref(src), len(st["key"]), len(st["ts"])))

"""Table API time-windowed (interval) join on row time on the GPU path -- the host mirror of
flink-libraries/flink-table/src/main/scala/org/apache/flink/table/runtime/join/RowTimeBoundedStreamJoin.scala inside
runtime/operators/KeyedCoProcessOperatorWithWatermarkDelay.scala, as plan/nodes/datastream/DataStreamWindowJoin.scala
:279-330 plans `l JOIN r ON l.k = r.k AND l.rowtime BETWEEN r.rowtime + lower AND r.rowtime + upper`.  The handle joins
on key and row time only; output rows carry the joined rows' arrival ordinals (one counter over both sides, -1 on the
null-padded side) and the host re-attaches the forwarded fields by ordinal.  The planner's rewrite is not rebuilt.
"""
import ctypes

import numpy as np

from . import _native as N
from ._handle import _TableHandle

_KEY_KINDS = {"long": N.FW_KEY_LONG, "int": N.FW_KEY_INT, "hashed": N.FW_KEY_HASHED}
JOIN_TYPES = {"inner": N.FW_TJOIN_INNER, "left": N.FW_TJOIN_LEFT, "right": N.FW_TJOIN_RIGHT, "full": N.FW_TJOIN_FULL}

_ROW_FIELDS = [f for f, _ in N.FwTjoinRows._fields_]
TJOIN_ROW_DTYPE = np.dtype([(f, np.int64) for f in _ROW_FIELDS] + [("epoch", np.int64)])
_STATE_U8 = ("side", "emitted")
_KEY_COLS = ("key", "left_timer", "right_timer", "n_rows")


def tjoin_config(join_type, lower, upper, allowed_lateness=0, key_type="long", max_parallelism=128,
                 key_group_range=None, device=0, expected_keys=0, max_batch=0, max_pairs=0):
    c = N.FwTjoinConfig()
    c.join_type = JOIN_TYPES[join_type] if isinstance(join_type, str) else int(join_type)
    c.lower, c.upper, c.allowed_lateness = int(lower), int(upper), int(allowed_lateness)
    c.key_kind = _KEY_KINDS[key_type]
    c.max_parallelism = max_parallelism
    c.key_group_start, c.key_group_end = key_group_range if key_group_range is not None else (0, max_parallelism - 1)
    c.device = device
    c.expected_keys, c.max_batch, c.max_pairs = expected_keys, max_batch, max_pairs
    return c


class TimeBoundedJoin(_TableHandle):
    """One keyed row-time interval join.  join_type: "inner", "left", "right" or "full"; lower / upper: the bounds of
    l.rowtime - r.rowtime in ms.  process(side, keys, rowtimes[, vals, key_hash]) takes numpy arrays or CUDA tensors,
    side[i] 0 = left / 1 = right, index order = arrival order; watermark(wm) returns (rows, forwarded watermark), the
    rows emitted since the last call as a TJOIN_ROW_DTYPE array."""
    _prefix, _Rows, _Stats = "fw_tjoin", N.FwTjoinRows, N.FwTjoinStats

    def __init__(self, join_type, lower, upper, allowed_lateness=0, key_type="long", **kw):
        cfg = tjoin_config(join_type, lower, upper, allowed_lateness, key_type=key_type, **kw)
        self._create(cfg)

    def process(self, side, keys, rowtimes, vals=None, key_hash=None):
        L = N.lib()
        if hasattr(keys, "data_ptr"):
            import torch
            n = keys.numel()
            if not hasattr(side, "data_ptr"):
                side = torch.full((n,), int(side), dtype=torch.uint8, device=keys.device)
            cols = [(side, torch.uint8), (keys, torch.int64), (rowtimes, torch.int64)]
            if vals is not None:
                cols.append((vals, torch.int64))
            if key_hash is not None:
                cols.append((key_hash, torch.int32))
            for t, dt in cols:
                if not t.is_cuda or not t.is_contiguous() or t.numel() != n or t.dtype != dt:
                    raise ValueError("device columns must be contiguous CUDA tensors of equal length: side uint8, "
                                     "keys / rowtimes / vals int64, key_hash int32")
            torch.cuda.current_stream(keys.device).synchronize()  # the columns' producers; the push settles its own
            self._check(L.fw_tjoin_push_batch_device(
                self._h, side.data_ptr(), keys.data_ptr(), rowtimes.data_ptr(),
                vals.data_ptr() if vals is not None else None,
                key_hash.data_ptr() if key_hash is not None else None, n))
            return
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        rowtimes = np.ascontiguousarray(rowtimes, dtype=np.int64)
        n = len(keys)
        side = np.full(n, side, np.uint8) if np.isscalar(side) else np.ascontiguousarray(side, dtype=np.uint8)
        if len(rowtimes) != n or len(side) != n:
            raise ValueError("side, keys and rowtimes must have equal length")
        vp = kp = None
        if vals is not None:
            vals = np.ascontiguousarray(vals, dtype=np.int64)
            vp = vals.ctypes.data
        if key_hash is not None:
            key_hash = np.ascontiguousarray(key_hash, dtype=np.int32)
            kp = key_hash.ctypes.data
        self._check(L.fw_tjoin_push_batch(self._h, side.ctypes.data, keys.ctypes.data, rowtimes.ctypes.data, vp, kp, n))

    def process_left(self, keys, rowtimes, vals=None, key_hash=None):
        self.process(0, keys, rowtimes, vals, key_hash)

    def process_right(self, keys, rowtimes, vals=None, key_hash=None):
        self.process(1, keys, rowtimes, vals, key_hash)

    def advance_watermark(self, wm):
        """(rows the timers emitted, forwarded watermark)"""
        n, fw = ctypes.c_int64(), ctypes.c_int64()
        self._check(N.lib().fw_tjoin_advance_watermark(self._h, int(wm), ctypes.byref(n), ctypes.byref(fw)))
        return n.value, fw.value

    def rows_device(self):
        """The pending output rows where they are, in HBM: (FwTjoinRows of device pointers, rows).  Valid until the
        next call on the handle; the rows stay pending (clear_pending() discards them)."""
        return self._rows_device()

    def drain(self):
        """The pending output rows (TJOIN_ROW_DTYPE), removed from the handle."""
        n = self.stats()["pending_output_rows"]
        cols = {f: np.empty(n, np.int64) for f in _ROW_FIELDS + ["epoch"]}
        dst = N.FwTjoinRows(*(cols[f].ctypes.data for f in _ROW_FIELDS))
        got = ctypes.c_int64()
        self._check(N.lib().fw_tjoin_drain(self._h, ctypes.byref(dst), cols["epoch"].ctypes.data, n, ctypes.byref(got)))
        assert got.value == n
        out = np.empty(n, TJOIN_ROW_DTYPE)
        for f in cols:
            out[f] = cols[f]
        return out

    def watermark(self, wm):
        _, fw = self.advance_watermark(wm)
        return self.drain(), fw

    def snapshot(self, kg):
        """The keyed state of key group kg: {"key", "left_timer", "right_timer", "n_rows"} per key and {"side",
        "rowtime", "ordinal", "val", "emitted"} per cached row (numpy)."""
        L = N.lib()
        nk, nr = ctypes.c_int64(), ctypes.c_int64()
        self._check(L.fw_tjoin_snapshot_key_group(self._h, kg, None, 0, 0, ctypes.byref(nk), ctypes.byref(nr)))
        k, r = nk.value, nr.value
        st = {f: np.zeros(k if f in _KEY_COLS else r, np.uint8 if f in _STATE_U8 else np.int64)
              for f, _ in N.FwTjoinState._fields_}
        dst = N.FwTjoinState(*(st[f].ctypes.data for f, _ in N.FwTjoinState._fields_))
        self._check(L.fw_tjoin_snapshot_key_group(self._h, kg, ctypes.byref(dst), k, r, ctypes.byref(nk),
                                                  ctypes.byref(nr)))
        return st

    def restore(self, kg, state):
        st = {f: np.ascontiguousarray(state[f], dtype=np.uint8 if f in _STATE_U8 else np.int64)
              for f, _ in N.FwTjoinState._fields_}
        src = N.FwTjoinState(*(st[f].ctypes.data for f, _ in N.FwTjoinState._fields_))
        self._check(N.lib().fw_tjoin_restore_key_group(self._h, kg, ctypes.byref(src), len(st["key"]),
                                                       len(st["rowtime"])))

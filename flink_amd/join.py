"""GpuWindowJoin: DataStream.join(other).where().equalTo().window(...).apply(JoinFunction) and coGroup(...) on one
MI355X (include/flink_window.h "window joins").

In the reference a window join is the ordinary window-contents operator over the tagged union of both inputs
(CoGroupedStreams.WithWindow.apply, CoGroupedStreams.java:273-304); CoGroupWindowFunction.apply (:657-685) splits every
firing by input, and JoinCoGroupFunction.coGroup (JoinedStreams.java:387-404) collects join(val1, val2) for every val1
of the first list and, inside, every val2 of the second.  So this class holds a GpuListWindowOperator created with a
join -- the same operator, state, timers and evictors -- pushes each input with its side, and takes every firing
through the join stage of libflinkwin.so: the split by input, the pair counts and the pairs are made on the GPU.

  process1 / process2      processElement1 / processElement2 for a batch of one input (host or device columns)
  watermark1 / watermark2  the input's watermark; the operator sees the minimum of both, forwarded only when it rises
                           (the union's StatusWatermarkValve); watermark(wm) sets both inputs
  pairs()                  PAIR_DTYPE (epoch, key, start, end, val1, val2, ord1, ord2), a row's pairs first-input-major
                           as JoinCoGroupFunction collects them; ord1 / ord2 are the elements' plain arrival ordinals
  cogroups()               [(row, elements of input 1, elements of input 2)] of every firing, each in list order (the
                           elements' ordinals carry the input in FW_ORD_SIDE)
  outputs()                [(epoch, result)] of join_function(val1, val2) per pair / cogroup_function(key, window,
                           first, second) per firing, applied on drain as the list operator's window_function is

The allowed lateness defaults to 0: the reference's builder (WithWindow) passes none.
"""
import ctypes

import numpy as np

from . import _native as N
from .listwindow import LIST_ROW_DTYPE, LIST_ROW_FIELDS, GpuListWindowOperator
from .operator import ELEM_DTYPE
from .windowing import DeltaTrigger

PAIR_FIELDS = ("row", "idx1", "idx2", "val1", "val2")
PAIR_DTYPE = np.dtype([(f, "<i8") for f in ("epoch", "key", "start", "end", "val1", "val2", "ord1", "ord2")])
ORD_MASK = ~N.FW_ORD_SIDE
_MODES = {"join": N.FW_JOIN_INNER, "cogroup": N.FW_JOIN_COGROUP}
LONG_MIN = -(1 << 63)


class _DeviceColumn:
    """n int64 at a raw device pointer, for torch.as_tensor"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (ptr or 0, False), "version": 2}


class GpuWindowJoin:
    def __init__(self, assigner, trigger=None, evictor=None, mode="join", join_function=None, cogroup_function=None,
                 **list_operator_keywords):
        if mode not in _MODES:
            raise ValueError('mode is "join" or "cogroup"')
        if isinstance(getattr(trigger, "nested", trigger), DeltaTrigger):
            raise ValueError("a window join does not take DeltaTrigger: a DeltaFunction over the tagged union of the "
                             "two inputs is user code")
        kw = dict(list_operator_keywords)
        kw.setdefault("allowed_lateness", 0)
        self.mode = mode
        self.join_function, self.cogroup_function = join_function, cogroup_function
        self.op = GpuListWindowOperator(assigner, trigger, evictor, join=_MODES[mode], emit_contents=True, **kw)
        self._max_pairs = int(kw.get("max_join_pairs", 0)) or 1 << 30
        self._in_wm = [LONG_MIN, LONG_MIN]
        self._out_wm = LONG_MIN
        self._rows, self._nfirst, self._elems, self._pairs, self._outputs, self._side = [], [], [], [], [], []
        self._n_elems = 0

    def close(self):
        self.op.close()

    dispose = close

    @property
    def epoch(self):
        return self.op.epoch

    # ------------------------------------------------------------------ input
    def process1(self, keys, ts, vals, key_hash=None):
        self.op.process_batch(keys, ts, vals, key_hash, side=0)
        self._collect(self.op.epoch)

    def process2(self, keys, ts, vals, key_hash=None):
        self.op.process_batch(keys, ts, vals, key_hash, side=1)
        self._collect(self.op.epoch)

    def _input_watermark(self, side, wm):
        self._in_wm[side] = max(self._in_wm[side], int(wm))
        m = min(self._in_wm)
        if m > self._out_wm:
            self._out_wm = m
            self.op.advance_watermark(m)
            self._collect(self.op.epoch - 1)

    def watermark1(self, wm):
        self._input_watermark(0, wm)

    def watermark2(self, wm):
        self._input_watermark(1, wm)

    def watermark(self, wm):
        self._in_wm[0] = max(self._in_wm[0], int(wm))
        self._input_watermark(1, wm)

    # ------------------------------------------------------------------ the join stage
    def join_pending(self):
        """(rows, elements, pairs) pending in HBM; the pairs are counted, not made"""
        nr, ne, np_ = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self.op._check(N.lib().fw_list_join_pending(self.op._h, ctypes.byref(nr), ctypes.byref(ne), ctypes.byref(np_)))
        return nr.value, ne.value, np_.value

    def drain_join(self, epoch=-1, pairs=True, cap_pairs=None):
        """(rows LIST_ROW_DTYPE, n_first, partitioned elements ELEM_DTYPE, pair columns {row, idx1, idx2, val1, val2} or
        None) pending, cleared from HBM.  pairs=False takes the coGroup form alone: no pair is materialised."""
        L = N.lib()
        nr, ne, npairs = self.join_pending()
        pairs = bool(pairs) and self.mode == "join"
        cap_p = npairs if cap_pairs is None else int(cap_pairs)
        refused = pairs and npairs > self._max_pairs  # the call reports it; no host columns are made for it
        cols = {f: np.zeros(nr, dtype=np.int64) for f in LIST_ROW_FIELDS}
        nfirst = np.zeros(nr, dtype=np.int64)
        ecols = {f: np.zeros(ne, dtype=np.int64) for f in ELEM_DTYPE.names}
        pcols = {f: np.zeros(0 if refused else max(cap_p, 0), dtype=np.int64) for f in PAIR_FIELDS} if pairs else None
        rows = N.FwListRows(**{f: cols[f].ctypes.data for f in LIST_ROW_FIELDS})
        elems = N.FwListElems(**{f: ecols[f].ctypes.data for f in ecols})
        pv = N.FwJoinPairs(**{f: pcols[f].ctypes.data for f in PAIR_FIELDS}) if pairs else None
        gr, ge, gp = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self.op._check(L.fw_list_drain_join(self.op._h, ctypes.byref(rows), nfirst.ctypes.data, nr, ctypes.byref(elems),
                                            ne, ctypes.byref(pv) if pairs else None, cap_p, ctypes.byref(gr),
                                            ctypes.byref(ge), ctypes.byref(gp)))
        out = np.zeros(gr.value, dtype=LIST_ROW_DTYPE)
        for f in LIST_ROW_FIELDS:
            out[f] = cols[f][:gr.value]
        out["epoch"] = epoch
        el = np.zeros(ge.value, dtype=ELEM_DTYPE)
        for f in ecols:
            el[f] = ecols[f][:ge.value]
        if pairs:
            pcols = {f: pcols[f][:gp.value] for f in PAIR_FIELDS}
        return out, nfirst[:gr.value], el, pcols

    def join_device(self, pairs=True):
        """Device view of the pending output, valid until the next call on the handle and not cleared: (rows, n_first,
        partitioned elements, pairs or None) as dicts of int64 CUDA tensors over the handle's own buffers."""
        import torch
        rows, elems, pv = N.FwListRows(), N.FwListElems(), N.FwJoinPairs()
        nfirst = ctypes.c_void_p()
        nr, ne, npairs = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        pairs = bool(pairs) and self.mode == "join"
        self.op._check(N.lib().fw_list_join_device(self.op._h, ctypes.byref(rows), ctypes.byref(nfirst),
                                                   ctypes.byref(elems), ctypes.byref(pv) if pairs else None,
                                                   ctypes.byref(nr), ctypes.byref(ne), ctypes.byref(npairs)))
        dev = f"cuda:{self.op._cfg.device}"

        def view(ptr, n):
            return torch.as_tensor(_DeviceColumn(ptr, n), device=dev) if n else torch.zeros(0, dtype=torch.int64,
                                                                                          device=dev)
        return ({f: view(getattr(rows, f), nr.value) for f in LIST_ROW_FIELDS}, view(nfirst.value, nr.value),
                {f: view(getattr(elems, f), ne.value) for f in ELEM_DTYPE.names},
                {f: view(getattr(pv, f), npairs.value) for f in PAIR_FIELDS} if pairs else None)

    def _collect(self, epoch):
        rows, nfirst, el, pc = self.drain_join(epoch)
        if len(rows):
            rows["elem_off"] += self._n_elems
            self._rows.append(rows)
            self._nfirst.append(nfirst)
            self._elems.append(el)
            if pc is not None:
                r = pc["row"]
                out = np.zeros(len(r), dtype=PAIR_DTYPE)
                for f in ("epoch", "key", "start", "end"):
                    out[f] = rows[f][r]
                out["val1"], out["val2"] = pc["val1"], pc["val2"]
                out["ord1"], out["ord2"] = el["ordinal"][pc["idx1"]] & ORD_MASK, el["ordinal"][pc["idx2"]] & ORD_MASK
                self._pairs.append(out)
                if self.join_function is not None:
                    self._outputs.extend((epoch, self.join_function(int(a), int(b)))
                                         for a, b in zip(pc["val1"].tolist(), pc["val2"].tolist()))
            if self.cogroup_function is not None:
                for x, n1 in zip(rows, nfirst):
                    o = int(x["elem_off"]) - self._n_elems
                    self._outputs.append((epoch, self.cogroup_function(int(x["key"]), (int(x["start"]), int(x["end"])),
                                                                       el[o:o + n1], el[o + n1:o + int(x["count"])])))
            self._n_elems += len(el)
        if self.op.side_output_enabled:
            self._side.append(self.op.drain_side(epoch))
        return rows

    # ------------------------------------------------------------------ output
    def rows(self):
        return np.concatenate(self._rows) if self._rows else np.zeros(0, dtype=LIST_ROW_DTYPE)

    def n_first(self):
        return np.concatenate(self._nfirst) if self._nfirst else np.zeros(0, dtype=np.int64)

    def elems(self):
        return np.concatenate(self._elems) if self._elems else np.zeros(0, dtype=ELEM_DTYPE)

    def pairs(self):
        return np.concatenate(self._pairs) if self._pairs else np.zeros(0, dtype=PAIR_DTYPE)

    def cogroups(self):
        e = self.elems()
        return [(r, e[r["elem_off"]:r["elem_off"] + n1], e[r["elem_off"] + n1:r["elem_off"] + r["count"]])
                for r, n1 in zip(self.rows(), self.n_first().tolist())]

    def outputs(self):
        return list(self._outputs)

    def side_rows(self):
        """late records: key, ts, val (the input a late record came from is not reported)"""
        from .listwindow import SIDE_DTYPE
        return np.concatenate(self._side) if self._side else np.zeros(0, dtype=SIDE_DTYPE)

    # ------------------------------------------------------------------ state and metrics: the list operator's
    def snapshot_state(self):
        return self.op.snapshot_state()

    def initialize_state(self, snapshot):
        self.op.initialize_state(snapshot)

    snapshotState, initializeState = snapshot_state, initialize_state

    def stats(self):
        return self.op.stats()

    @property
    def late_dropped(self):
        return self.op.late_dropped

    @property
    def num_keyed_state_entries(self):
        return self.op.num_keyed_state_entries

    @property
    def num_event_time_timers(self):
        return self.op.num_event_time_timers

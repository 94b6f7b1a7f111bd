"""CountTrigger on the aggregating operator, GpuWindowOperator(trigger=CountTrigger.of(n)) (fw_create_count_trigger),
against the pinned ListWindowOracle(trigger="count", evictor="none"), whose row over a firing's list is the accumulator
at that element.  Bar: rows as sorted multisets per watermark epoch, integers bit for bit (the double streams are
dyadic: every partial sum is exact, so bit for bit too), and after every step numKeyedStateEntries, numEventTimeTimers,
numLateRecordsDropped and the side rows.  The streams and configurations are vetted on the CPU by
tests/test_agg_count_trigger_abi.py."""
import ctypes

import numpy as np
import pytest

from flink_amd import _native as N
from flink_amd import (CountSumMinMax, CountTrigger, KeyGroupRange, PurgingTrigger, SlidingEventTimeWindows,
                       TumblingEventTimeWindows)
from flink_amd.operator import GpuWindowOperator
from oracle import oracle as orc
from tests import agg_count_trigger_util as U
from tests import time_edges_util as TE
from tests.continuous_ref import LMAX, drive, seeded_stream
from tests.count_trigger_ref import CountTriggerRef

pytestmark = pytest.mark.gpu


class _Gpu:
    """the operator in the harness shape drive() uses; device=True pushes torch columns (fw_push_batch_device)"""

    def __init__(self, value_type="long", assigner="tumbling", size=0, slide=0, offset=0, lateness=0, n=1,
                 purging=False, side_output=False, device=False, **kw):
        asg = TumblingEventTimeWindows.of(size, offset) if assigner == "tumbling" else \
            SlidingEventTimeWindows.of(size, slide, offset)
        trig = CountTrigger.of(n)
        self.op = GpuWindowOperator(asg, CountSumMinMax(value_type), PurgingTrigger.of(trig) if purging else trig,
                                    allowed_lateness=lateness, side_output=side_output, **kw)
        self.value_type, self.device = value_type, device

    def process(self, k, t, v):
        v = U.values_of(np.asarray(v), self.value_type)[0]
        if self.device:
            import torch
            k, t, v = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (k, t, v))
        self.op.process(k, t, v)
        # rows fired inside the push belong to the epoch the operator's next watermark() closes
        self.op._rows.append(self.op.drain_rows(self.op.epoch))

    def watermark(self, wm):
        self.op.watermark(wm)

    def row_tuples(self):
        r = self.op.rows()
        return sorted(zip(*[r[f].tolist() for f in ("epoch", "key", "start", "end", "count", "sum", "min", "max")]))

    def side_tuples(self):
        s = self.op.side_rows()
        return sorted(zip(*[s[f].tolist() for f in ("epoch", "key", "ts", "val")]))

    def close(self):
        self.op.close()


def _assert_rows(gpu, ref, nonempty=True):
    a, b = gpu.row_tuples(), ref.row_tuples()
    assert len(a) == len(b) and (len(a) > 0 or not nonempty), (len(a), len(b))
    assert a == b, [x for x in zip(a, b) if x[0] != x[1]][:3]


def _stats_checker(gpu, ref, side=False):
    def check():
        st = gpu.op.stats()
        assert st["keyed_state_entries"] == ref.num_state_entries
        assert st["event_time_timers"] == ref.num_timers
        assert st["late_records_dropped"] == ref.late_dropped
        if side:  # (the operator hands the side rows out with the watermark that closes their epoch)
            assert gpu.side_tuples() == [r for r in ref.side_tuples() if r[0] < ref.epoch]
    return check


@pytest.mark.parametrize("cfg", U.CONFIGS, ids=U.IDS)
@pytest.mark.parametrize("value_type", U.VALUE_TYPES)
def test_gpu_agg_count_trigger_parity(cfg, value_type):
    gpu, ref = _Gpu(value_type, **cfg), U.Oracle(value_type, **cfg)
    k, t, v = U.stream_of(cfg)
    drive([gpu, ref], k, t, v, each=_stats_checker(gpu, ref, side=cfg["side_output"]))
    _assert_rows(gpu, ref, nonempty=cfg["n"] != U.BIG)
    _stats_checker(gpu, ref)()
    assert gpu.op.stats()["keyed_state_entries"] == 0  # (Long.MAX_VALUE cleaned every window up)
    if cfg["side_output"]:
        assert gpu.side_tuples() == ref.side_tuples()
    gpu.close()


@pytest.mark.parametrize("cfg", [U.CONFIGS[1], U.CONFIGS[11]], ids=[U.IDS[1], U.IDS[11]])
@pytest.mark.parametrize("value_type", U.NARROW_TYPES)
def test_gpu_agg_count_trigger_float_short_byte(cfg, value_type):
    """Float (the sum is rounded once, when the row is written; the stream's sums are exact in float, so the bits are
    the oracle's), Short and Byte (sums wrap to 16 / 8 bits)"""
    gpu, ref = _Gpu(value_type, **cfg), U.Oracle(value_type, **cfg)
    k, t, v = U.stream_of(cfg)
    drive([gpu, ref], k, t, v, each=_stats_checker(gpu, ref, side=cfg["side_output"]))
    _assert_rows(gpu, ref)
    gpu.close()


@pytest.mark.parametrize("cfg", [U.CONFIGS[4], U.CONFIGS[9]], ids=[U.IDS[4], U.IDS[9]])
def test_gpu_agg_count_trigger_host_push_without_async_input(cfg):
    gpu, ref = _Gpu("long", async_input=False, **cfg), U.Oracle("long", **cfg)
    k, t, v = U.stream_of(cfg)
    drive([gpu, ref], k, t, v, each=_stats_checker(gpu, ref, side=cfg["side_output"]))
    _assert_rows(gpu, ref)
    assert gpu.side_tuples() == ref.side_tuples()
    gpu.close()


def _state_args(n=0):
    cols = [np.zeros(max(n, 1), dtype=np.int64) for _ in range(9)]
    return cols, N.FwStateRows(*[c.ctypes.data for c in cols[:8]])


def test_gpu_agg_count_trigger_entry_points_that_refuse():
    """the combiner entry points refuse such a handle (partials carry no arrival order); the other snapshot / restore
    pairs refuse it and name the new pair; the new pair refuses every other handle"""
    L = N.lib()
    ct = _Gpu("long", **U.CONFIGS[0])
    plain = GpuWindowOperator(TumblingEventTimeWindows.of(100), CountSumMinMax("long"))
    h, n = ct.op._h, ctypes.c_int64()
    cols, rows = _state_args()
    part = N.FwPartials()

    def refused(rc, handle, *fragments):
        assert rc == N.FW_ERR_UNSUPPORTED, rc
        msg = L.fw_last_error(handle).decode()
        assert all(f in msg for f in fragments), msg

    refused(L.fw_combine_extract_device(h, 1, ctypes.byref(part), 0, None, ctypes.byref(n)), h, "CountTrigger",
            "arrival order")
    refused(L.fw_push_partials_device(h, ctypes.byref(part), 0), h, "CountTrigger", "arrival order")
    refused(L.fw_snapshot_key_group(h, 0, None, 0, ctypes.byref(n)), h, "fw_snapshot_key_group_trigger_count")
    refused(L.fw_snapshot_key_group_blocks(h, 0, None, None, 0, ctypes.byref(n)), h,
            "fw_snapshot_key_group_trigger_count")
    refused(L.fw_snapshot_key_group_fire(h, 0, None, None, 0, ctypes.byref(n)), h, "fw_snapshot_key_group")
    refused(L.fw_restore_key_group(h, 0, ctypes.byref(rows), 0), h, "fw_restore_key_group_trigger_count")
    refused(L.fw_restore_key_group_blocks(h, 0, ctypes.byref(rows), None, 0), h, "fw_restore_key_group_trigger_count")
    refused(L.fw_restore_key_group_fire(h, 0, ctypes.byref(rows), cols[8].ctypes.data, 0), h, "fw_restore_key_group")
    refused(L.fw_snapshot_key_group_trigger_count(plain._h, 0, None, None, 0, ctypes.byref(n)), plain._h,
            "fw_create_count_trigger")
    refused(L.fw_restore_key_group_trigger_count(plain._h, 0, ctypes.byref(rows), cols[8].ctypes.data, 0), plain._h,
            "fw_create_count_trigger")
    # ... and the handles go on working
    one = np.ones(2, dtype=np.int64)
    ct.process(one, 10 * one, one)
    assert len(ct.row_tuples()) == 2
    plain.close()
    ct.close()


@pytest.mark.parametrize("async_input", [True, False], ids=["async", "sync"])
@pytest.mark.parametrize("cfg", U.DEVICE_CONFIGS, ids=[U.cfg_id(c) for c in U.DEVICE_CONFIGS])
def test_gpu_agg_count_trigger_device_push(cfg, async_input):
    gpu, ref = _Gpu("long", device=True, async_input=async_input, **cfg), U.Oracle("long", **cfg)
    k, t, v = U.stream_of(cfg)
    drive([gpu, ref], k, t, v, each=_stats_checker(gpu, ref, side=cfg["side_output"]))
    _assert_rows(gpu, ref)
    if cfg["side_output"]:
        assert gpu.side_tuples() == ref.side_tuples()
    gpu.close()


@pytest.mark.parametrize("purging", [False, True], ids=["keep", "purge"])
def test_gpu_agg_count_trigger_batch_geometry(purging):
    """the same stream in pushes of 1, 7, 64 records and all at once: the counts carry across pushes"""
    cfg = dict(assigner="sliding", size=300, slide=100, offset=0, lateness=0, n=3, purging=purging, side_output=False)
    k, t, v = seeded_stream(3, 640, 5, 400, 50)
    ref = U.Oracle("long", **cfg)
    ref.process(k, t, v)
    exp = ref.row_tuples()
    assert len(exp) > 100
    for batch in (1, 7, 64, len(k)):
        gpu = _Gpu("long", **cfg)
        for b in range(0, len(k), batch):
            gpu.process(k[b:b + batch], t[b:b + batch], v[b:b + batch])
        assert gpu.row_tuples() == exp, batch
        gpu.close()


def test_gpu_agg_count_trigger_exact_group():
    """a push whose group has exactly n - c0 records: it fires at the push's last record and leaves count 0"""
    cfg = dict(assigner="tumbling", size=100, slide=0, offset=0, lateness=0, n=5, purging=False, side_output=False)
    gpu = _Gpu("long", **cfg)
    one = np.ones(8, dtype=np.int64)
    gpu.process(one[:2], 10 * one[:2], np.array([4, 5]))  # c0 = 2
    assert gpu.row_tuples() == []
    gpu.process(one[:3], 20 * one[:3], np.array([-7, 9, 1]))  # exactly n - c0
    assert gpu.row_tuples() == [(0, 1, 0, 100, 5, 12, -7, 9)]
    snap = np.concatenate(list(gpu.op.snapshot_state().values()))
    assert snap["trigger_count"].tolist() == [0] and snap["count"].tolist() == [5]
    gpu.process(one[:4], 30 * one[:4], np.array([1, 1, 1, 1]))  # c0 = 0 again: no row yet
    assert len(gpu.row_tuples()) == 1
    gpu.close()


@pytest.mark.parametrize("keys", [1, 2], ids=["one-key", "two-keys"])
@pytest.mark.parametrize("purging", [False, True], ids=["keep", "purge"])
def test_gpu_agg_count_trigger_hot_key(keys, purging):
    """3 * 32768 + 17 records of one key (two alternating keys) in one window, one push: the scan crosses its chunks;
    every row's count is exact and the sums are the closed form"""
    cfg = dict(assigner="tumbling", size=1000000, slide=0, offset=0, lateness=0, n=5, purging=purging,
               side_output=False)
    gpu = _Gpu("long", **cfg)
    k, t, v = U.hot_stream(keys)
    gpu.process(k, t, v)
    exp = U.hot_expected(k, v, 5, purging)
    assert len(exp) == sum(int((k == key).sum()) // 5 for key in np.unique(k))
    assert gpu.row_tuples() == exp
    gpu.close()


def test_gpu_agg_count_trigger_row_growth():
    """n = 1 over sliding 300/100: one push of 2^17 records gives 3 * 2^17 rows from a handle sized for far fewer"""
    n = 1 << 17
    op = GpuWindowOperator(SlidingEventTimeWindows.of(300, 100), CountSumMinMax("long"), CountTrigger.of(1),
                           max_batch=n, expected_entries=1024)
    k = np.arange(n, dtype=np.int64) % 5000
    t = 1000 + (np.arange(n, dtype=np.int64) * 31) % 700
    v = np.arange(n, dtype=np.int64)
    op.process(k, t, v)
    rows = op.drain_rows(0)
    assert len(rows) == 3 * n
    # every (key, window)'s rows count 1 .. its elements, and the last one holds the sum of them all
    order = np.lexsort((rows["count"], rows["start"], rows["key"]))
    r = rows[order]
    first = np.r_[True, (r["key"][1:] != r["key"][:-1]) | (r["start"][1:] != r["start"][:-1])]
    assert np.all(r["count"][first] == 1) and np.all(np.diff(r["count"])[~first[1:]] == 1)
    last = np.r_[first[1:], True]
    assert int(r["sum"][last].sum()) == 3 * int(v.sum())
    op.close()


def test_gpu_agg_count_trigger_many_records_per_new_window_do_not_grow_the_table():
    """512 windows opened by 128 records each in one push: the records that race for a new window's slot are not
    counted against the regions' load limit (a handle sized for 16384 windows keeps its table)"""
    n = 1 << 16
    op = GpuWindowOperator(TumblingEventTimeWindows.of(1000), CountSumMinMax("long"), CountTrigger.of(128),
                           max_batch=n, expected_entries=16384)
    k = np.arange(n, dtype=np.int64) % 512
    op.process(k, np.full(n, 5, dtype=np.int64), np.ones(n, dtype=np.int64))
    rows = op.drain_rows(0)
    assert len(rows) == 512 and np.all(rows["count"] == 128) and np.all(rows["sum"] == 128)
    st = op.stats()
    assert st["table_grows"] == 0 and st["keyed_state_entries"] == 512
    op.close()


@pytest.mark.parametrize("cfg", [TE.PRE_TUMBLING[1], TE.PRE_SLIDING[1], TE.PRE_SLIDING[3]],
                         ids=["tumbling-o999", "sliding-o999", "sliding-late-purging-side"])
def test_gpu_agg_count_trigger_pre_epoch(cfg):
    """time_edges_util's pre-epoch class: negative timestamps, displaced records (whose extra window counts too)"""
    full = dict(assigner=cfg["assigner"], size=cfg["size"], slide=cfg.get("slide", 0), offset=cfg.get("offset", 0),
                lateness=cfg.get("lateness", 0), n=3, purging=cfg.get("purging", False),
                side_output=cfg.get("side_output", False))
    batches, wms = TE.pre_epoch_stream(cfg, n=8000, batch=1000)
    if cfg["assigner"] == "sliding":
        assert TE.coverage(cfg, batches)["extra"] > 0
    gpu, ref = _Gpu("long", **full), U.Oracle("long", **full)
    check = _stats_checker(gpu, ref, side=full["side_output"])
    for (k, t, v), wm in zip(batches, wms):
        for h in (gpu, ref):
            h.process(k, t, v)
            h.watermark(wm)
        check()
    for h in (gpu, ref):
        h.watermark(LMAX)
    _assert_rows(gpu, ref)
    assert any(r[2] < 0 for r in gpu.row_tuples())
    if full["side_output"]:
        assert gpu.side_tuples() == ref.side_tuples()
    gpu.close()


@pytest.mark.parametrize("name", U.WRAP_NAMES)
def test_gpu_agg_count_trigger_long_range_ends(name):
    """one WRAP_CASES configuration at each end of the long range under the warm schedule: the windows path's
    treatment (wrapping longs, exact; the sliding assigner's runaway set is not in these streams)"""
    cfg, batches, wms = TE.wrap_case(name)
    full = U.wrap_cfg(cfg)
    gpu, ref = _Gpu("long", **full), U.Oracle("long", **full)
    check = _stats_checker(gpu, ref)
    for (k, t, v), wm in zip(batches, wms):
        for h in (gpu, ref):
            h.process(k, t, v)
            h.watermark(wm)
        check()
    _assert_rows(gpu, ref)
    gpu.close()


def _halves(k, t, v, cfg):
    h = len(k) // 2
    return h, int(t[:h].max()) - 70


@pytest.mark.parametrize("cfg", U.SNAPSHOT_CONFIGS, ids=[U.cfg_id(c) for c in U.SNAPSHOT_CONFIGS])
@pytest.mark.parametrize("split", [1, 2], ids=["whole", "two-halves"])
def test_gpu_agg_count_trigger_snapshot_restore(cfg, split):
    """a mid-stream snapshot of all key groups into a fresh handle, or into two handles of half the key-group range
    each: the continued stream gives the uninterrupted run's rows"""
    k, t, v = seeded_stream(21, 20000, 200, 2000, 60)
    h, wm = _halves(k, t, v, cfg)
    whole, ref = _Gpu("long", **cfg), U.Oracle("long", **cfg)
    for x in (whole, ref):
        x.process(k[:h], t[:h], v[:h])
        x.watermark(wm)
    snap = whole.op.snapshot_state()
    assert whole.op.state_dtype().names[-1] == "trigger_count"
    rows = np.concatenate(list(snap.values()))
    assert len(rows) > 0 and int((rows["trigger_count"] > 0).sum()) > 0 and np.all(rows["timer"] == 0)
    if cfg["purging"]:  # a purged-and-empty window survives as a row of count 0 with its timer
        assert int(((rows["count"] == 0) & (rows["trigger_count"] == 0)).sum()) > 0
    st = whole.op.stats()
    assert st["event_time_timers"] == len(rows) and st["keyed_state_entries"] == int((rows["count"] > 0).sum())
    ranges = [KeyGroupRange(0, 127)] if split == 1 else [KeyGroupRange(0, 63), KeyGroupRange(64, 127)]
    parts = [_Gpu("long", key_group_range=r, **cfg) for r in ranges]
    from oracle.oracle import key_groups_long
    kg = key_groups_long(k, 128)
    for p, r in zip(parts, ranges):
        p.op.initialize_state(snap)
        p.op.watermark(wm)
        p.op.epoch = 1
        p.op._rows.clear()
        m = (kg[h:] >= r.start_key_group) & (kg[h:] <= r.end_key_group)
        p.process(k[h:][m], t[h:][m], v[h:][m])
        p.watermark(LMAX)
    ref.process(k[h:], t[h:], v[h:])
    ref.watermark(LMAX)
    got = sorted(sum((p.row_tuples() for p in parts), []))
    exp = [r for r in ref.row_tuples() if r[0] >= 1]
    assert len(exp) > 0 and got == exp
    assert sum(p.op.stats()["event_time_timers"] for p in parts) == 0
    for p in parts + [whole]:
        p.close()


def test_gpu_agg_count_trigger_restored_count_above_n():
    """a restored trigger_count of n + 2 fires at the next element with the whole accumulator, then every n; duplicate
    rows of one window merge and their counts add without firing (against CountTriggerRef)"""
    n = 4
    cfg = dict(assigner="tumbling", size=100, slide=0, offset=0, lateness=0, n=n, purging=False, side_output=False)
    gpu = _Gpu("long", **cfg)
    ref = CountTriggerRef(**cfg)
    rows = np.zeros(3, dtype=gpu.op.state_dtype())
    # window (key 1, [0, 100)) twice: counts 3 + 3 = n + 2; window (key 2, [0, 100)) below n
    for i, (key, cnt, sm, mn, mx, tc) in enumerate([(1, 5, 50, 2, 30, 3), (1, 4, -8, -9, 3, 3), (2, 2, 7, 3, 4, 2)]):
        rows[i] = (key, 0, 100, cnt, sm, mn, mx, 0, tc)
        ref.restore(key, 0, cnt, sm, mn, mx, tc)
    from oracle.oracle import key_groups_long
    kgs = key_groups_long(rows["key"], 128)
    for g in np.unique(kgs):
        gpu.op.restore_key_group(int(g), rows[kgs == g])
    back = np.concatenate(list(gpu.op.snapshot_state().values()))
    back = back[np.argsort(back["key"])]
    assert back["trigger_count"].tolist() == [n + 2, 2] and back["count"].tolist() == [9, 2]
    assert back["sum"].tolist() == [42, 7] and back["min"].tolist() == [-9, 3] and back["max"].tolist() == [30, 4]
    assert gpu.row_tuples() == []  # (merging fires nothing)
    k = np.array([1, 2, 1, 1, 1, 1, 2, 1, 1, 1], dtype=np.int64)
    t = np.full(10, 50, dtype=np.int64)
    v = np.arange(10, dtype=np.int64) * 3 - 5
    gpu.process(k, t, v)
    ref.process(k, t, v)
    exp = ref.rows()
    assert [r[4] for r in exp if r[1] == 1] == [10, 14] and [r[4] for r in exp if r[1] == 2] == [4]
    assert gpu.row_tuples() == exp
    gpu.close()


def test_gpu_agg_count_trigger_restored_empty_duplicate():
    """a duplicate row of an emptied window (count 0, junk in sum / min / max) leaves the accumulator as it is and
    adds its trigger count, whether it is the row that is inserted (key 1) or the one that merges (key 2)"""
    cfg = dict(assigner="tumbling", size=100, slide=0, offset=0, lateness=0, n=4, purging=True, side_output=False)
    gpu = _Gpu("long", **cfg)
    rows = np.zeros(4, dtype=gpu.op.state_dtype())
    for i, (key, cnt, sm, mn, mx, tc) in enumerate([(1, 0, 999, -777, 888, 1), (1, 5, 50, 2, 30, 2),
                                                    (2, 3, -8, -9, 3, 1), (2, 0, 999, -777, 888, 2)]):
        rows[i] = (key, 0, 100, cnt, sm, mn, mx, 0, tc)
    from oracle.oracle import key_groups_long
    kgs = key_groups_long(rows["key"], 128)
    for g in np.unique(kgs):
        gpu.op.restore_key_group(int(g), rows[kgs == g])
    back = np.concatenate(list(gpu.op.snapshot_state().values()))
    back = back[np.argsort(back["key"])]
    assert back["key"].tolist() == [1, 2] and back["trigger_count"].tolist() == [3, 3]
    assert back["count"].tolist() == [5, 3] and back["sum"].tolist() == [50, -8]
    assert back["min"].tolist() == [2, -9] and back["max"].tolist() == [30, 3]
    assert gpu.op.stats()["keyed_state_entries"] == 2
    gpu.close()


def test_gpu_agg_count_trigger_neighbours_unchanged():
    """a tumbling and a sliding handle of plain fw_create still give the oracle's rows beside a CountTrigger handle"""
    ct = _Gpu("long", **U.CONFIGS[1])
    k, t, v = seeded_stream(9, 20000, 37, 2000, 150)
    t = t + 1000  # (no pre-epoch timestamp: the sliding neighbour keeps panes, which refuse displaced records)
    ct.process(k, t, v)
    for asg, ocfg in ((TumblingEventTimeWindows.of(100), dict(assigner="tumbling", size=100)),
                      (SlidingEventTimeWindows.of(300, 100), dict(assigner="sliding", size=300, slide=100))):
        op, ref = GpuWindowOperator(asg, CountSumMinMax("long")), orc.WindowOperatorOracle(**ocfg)
        for h in (op, ref):
            h.process(k[:10000], t[:10000], v[:10000])
            h.watermark(int(t[:10000].max()) - 100)
            h.process(k[10000:], t[10000:], v[10000:])
            h.watermark(LMAX)
        g, r = op.rows(), ref.rows()
        key = lambda a: a[np.lexsort((a["start"], a["key"], a["epoch"]))]  # noqa: E731
        g, r = key(g), key(r)
        assert len(g) == len(r) > 0
        for f in ("epoch", "key", "start", "end", "count", "sum", "min", "max"):
            assert np.array_equal(g[f], r[f]), f
        op.close()
    ct.close()

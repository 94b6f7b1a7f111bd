"""ContinuousEventTimeTrigger (early firings) on the aggregating operator, GpuWindowOperator(trigger=
ContinuousEventTimeTrigger.of(interval)), against tests/continuous_ref.ContinuousRef(trigger="continuous",
evictor="none"), whose rows' (key, start, end, count, sum, min, max) are what an aggregating state holds.  Bar: rows
as sorted multisets per epoch, bit for bit -- duplicates matter, a window that fires three times in one advance gives
three equal rows -- and after every step numKeyedStateEntries, numEventTimeTimers, numLateRecordsDropped and the side
rows.  The streams and configurations are vetted on the CPU by tests/test_agg_continuous_abi.py."""
import ctypes

import numpy as np
import pytest

from flink_amd import (ContinuousEventTimeTrigger, CountSumMinMax, KeyGroupRange, PurgingTrigger,
                       SlidingEventTimeWindows, TumblingEventTimeWindows)
from flink_amd import _native as N
from flink_amd.operator import FIRE_NULL, GpuWindowOperator
from tests import agg_continuous_util as U
from tests.continuous_ref import LMAX, drive, load_continuous_kats, replay_kat, seeded_stream

pytestmark = pytest.mark.gpu

KATS = [c for c in load_continuous_kats() if c["derived"] and c["cfg"]["assigner"] in ("tumbling", "sliding")]


class _Gpu:
    """the operator in the harness shape drive() and replay_kat() use: process / watermark / rows, values of the
    field's type"""

    def __init__(self, value_type="long", assigner="tumbling", size=0, slide=0, offset=0, lateness=0, interval=0,
                 purging=False, side_output=False, **kw):
        asg = TumblingEventTimeWindows.of(size, offset) if assigner == "tumbling" else \
            SlidingEventTimeWindows.of(size, slide, offset)
        trig = ContinuousEventTimeTrigger.of(interval)
        self.op = GpuWindowOperator(asg, CountSumMinMax(value_type), PurgingTrigger.of(trig) if purging else trig,
                                    allowed_lateness=lateness, side_output=side_output, **kw)
        self.value_type = value_type

    def process(self, k, t, v):
        self.op.process(k, t, U.values_of(np.asarray(v), self.value_type)[0])
        # late firings, visible step by step (replay_kat): drained with the epoch they belong to, the one the
        # operator's own watermark() would have given them
        self.op._rows.append(self.op.drain_rows(self.op.epoch))

    def watermark(self, wm):
        self.op.watermark(wm)

    def rows(self):
        return self.op.rows()

    def row_tuples(self):
        r = self.op.rows()
        return sorted(zip(*[r[f].tolist() for f in ("epoch", "key", "start", "end", "count", "sum", "min", "max")]))

    def side_tuples(self):
        s = self.op.side_rows()
        return sorted(zip(*[s[f].tolist() for f in ("epoch", "key", "ts", "val")]))

    def close(self):
        self.op.close()


class _Ref:
    """ContinuousRef pushed the same stream (the values in the form it takes)"""

    def __init__(self, value_type="long", **cfg):
        self.ref = U.ref_of(value_type, **cfg)
        self.value_type = value_type

    def process(self, k, t, v):
        self.ref.process(k, t, U.values_of(np.asarray(v), self.value_type)[1])

    def watermark(self, wm):
        self.ref.watermark(wm)

    def rows(self):
        return self.ref.rows()

    def row_tuples(self):
        return U.ref_rows(self.ref, self.value_type)

    def side_tuples(self):
        return sorted(zip(*[c.tolist() for c in self.ref.side_rows()]))


def _pair(value_type="long", gpu_kw=None, **cfg):
    return _Gpu(value_type, **cfg, **(gpu_kw or {})), _Ref(value_type, **cfg)


def _assert_rows(gpu, ref):
    a, b = gpu.row_tuples(), ref.row_tuples()
    assert len(a) == len(b) > 0, (len(a), len(b))
    assert a == b, [x for x in zip(a, b) if x[0] != x[1]][:3]


def _stats_checker(gpu, ref, side=False):
    def check():
        st = gpu.op.stats()
        assert st["keyed_state_entries"] == ref.ref.num_state_entries
        assert st["event_time_timers"] == ref.ref.num_timers
        assert st["late_records_dropped"] == ref.ref.late_dropped
        if side:  # (the operator hands the side rows out with the watermark that closes their epoch)
            assert gpu.side_tuples() == [r for r in ref.side_tuples() if r[0] < ref.ref.epoch]
    return check


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_gpu_agg_continuous_kats(case):
    assert len(KATS) >= 7
    gpu = _Gpu(**case["cfg"])
    for i, (got, exp) in enumerate(replay_kat(case, gpu)):
        assert got == exp, (case["name"], i, got, exp)
    ref = _Ref(**case["cfg"])
    replay_kat(case, ref)
    _assert_rows(gpu, ref)
    gpu.close()


@pytest.mark.parametrize("cfg", U.SEEDED_CONFIGS, ids=U.SEEDED_IDS)
@pytest.mark.parametrize("value_type", U.VALUE_TYPES)
def test_gpu_agg_continuous_vs_restatement(cfg, value_type):
    gpu, ref = _pair(value_type, **cfg)
    k, t, v = seeded_stream(U.seed_of(cfg), 20000, 37, 2000, 150)
    drive([gpu, ref], k, t, v, each=_stats_checker(gpu, ref, side=bool(cfg.get("side_output"))))
    _assert_rows(gpu, ref)
    _stats_checker(gpu, ref)()
    if cfg.get("side_output"):
        assert gpu.side_tuples() == ref.side_tuples()
    gpu.close()


def test_gpu_agg_continuous_arrival_order_across_split_partition():
    # one (key, window) of more than 3 * FW_AGG_CHUNK records in one push: its partition is split over several
    # aggregate workgroups; the window is armed from record 0, which lies several intervals later than most
    cfg = dict(assigner="tumbling", size=100000, interval=250)
    gpu, ref = _pair(**cfg)
    k, t, v = U.split_stream(cfg["interval"], cfg["size"])
    for h in (gpu, ref):
        h.process(k, t, v)
    for wm in (1000, 1500, 2499, 2500, 2750, 3100, 99998, 99999):
        for h in (gpu, ref):
            h.watermark(wm)
    # key 1 is armed from record 0 (fire time 10 intervals = 2500: first row at the fourth watermark), key 2 from its
    # own first record (6 intervals = 1500: the second); the minimum timestamp would have fired both at the first
    first = {}
    for e, key, *_ in gpu.row_tuples():
        first[key] = min(first.get(key, e), e)
    assert first == {1: 3, 2: 1}
    _assert_rows(gpu, ref)
    gpu.close()


def test_gpu_agg_continuous_device_columns():
    # the stream as torch tensors: two pushes back to back with async input and no synchronisation between them,
    # then the watermark; rows equal those of the host-column run
    import torch
    cfg = dict(assigner="sliding", size=100, slide=25, lateness=40, interval=33)
    (a, b, wm) = U.device_stream()
    host = _Gpu(**cfg)
    dev = _Gpu(**cfg)
    ref = _Ref(**cfg)
    for part in (a, b):
        host.process(*part)
        ref.process(*part)
    cols = [[torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in part] for part in (a, b)]
    for c in cols:
        dev.op.process_batch(*c)  # asynchronous: no synchronize between the pushes
    for h in (host, dev, ref):
        h.watermark(wm)
        h.watermark(wm + 300)
        h.watermark(LMAX)
    _assert_rows(host, ref)
    assert dev.row_tuples() == host.row_tuples()
    host.close()
    dev.close()


def test_gpu_agg_continuous_growth():
    # a table far smaller than the stream: fire times survive rehash, and row-buffer growth inside a firing
    gpu, ref = _pair(gpu_kw=U.GROWTH_GPU_KW, **U.GROWTH_CONFIG)
    k, t, v = U.growth_stream()
    drive([gpu, ref], k, t, v, bound=50, each=_stats_checker(gpu, ref))
    _assert_rows(gpu, ref)
    assert gpu.op.stats()["table_grows"] > 0
    gpu.close()


def test_gpu_agg_continuous_firings_limit():
    gpu, ref = _pair(**U.LIMIT_CONFIG)
    for h in (gpu, ref):
        h.process(np.array([1]), np.array([5]), np.array([3]))
    with pytest.raises(N.NativeError) as e:
        gpu.op.advance_watermark(1 << 30)
    assert e.value.code == N.FW_ERR_UNSUPPORTED
    assert "2^20 trigger intervals" in str(e.value)
    for h in (gpu, ref):  # nothing was changed: a smaller advance works, from the same state
        h.watermark(1000)
    assert len(gpu.rows()) == 1000 - 5
    _assert_rows(gpu, ref)
    gpu.close()


def test_gpu_agg_continuous_time_range():
    cfg = U.RANGE_CONFIG
    gpu, ref = _pair(**cfg)
    k, t, v = seeded_stream(3, 2000, 20, 1000, 50)
    for h in (gpu, ref):
        h.process(k[:1000], t[:1000], v[:1000])
    bad_t = t[1000:1010].copy()
    bad_t[4] = LMAX - cfg["interval"] + 1  # ts > Long.MAX_VALUE - interval: the first fire time wraps
    with pytest.raises(N.NativeError) as e:
        gpu.process(k[1000:1010], bad_t, v[1000:1010])
    assert e.value.code == N.FW_ERR_TIME_RANGE
    for h in (gpu, ref):  # the refused push left nothing behind
        h.process(k[1000:], t[1000:], v[1000:])
        h.watermark(int(t.max()) - 60)
        h.watermark(LMAX)
    _assert_rows(gpu, ref)
    assert gpu.op.stats()["records_in"] == 2000
    gpu.close()


@pytest.mark.parametrize("cfg", U.SNAPSHOT_CONFIGS, ids=["keeping", "purging"])
def test_gpu_agg_continuous_snapshot_restore(cfg):
    gpu, ref = _pair(**cfg)
    k, t, v, h, wm = U.snapshot_stream()
    for o in (gpu, ref):
        o.process(k[:h], t[:h], v[:h])
        o.watermark(wm)
    # the plain pair refuses the handle and names the new one
    n = ctypes.c_int64()
    rc = N.lib().fw_snapshot_key_group(gpu.op._h, 0, None, 0, ctypes.byref(n))
    assert rc == N.FW_ERR_UNSUPPORTED and b"fw_snapshot_key_group_fire" in N.lib().fw_last_error(gpu.op._h)
    snap = gpu.op.snapshot_state()
    rows = np.concatenate(list(snap.values()))
    assert "fire_time" in rows.dtype.names
    fires = {(int(r["key"]), (int(r["start"]), int(r["end"]))): int(r["fire_time"]) for r in rows
             if r["fire_time"] != FIRE_NULL}
    assert fires == ref.ref.fire and len(fires) > 0
    assert int((rows["count"] > 0).sum()) == ref.ref.num_state_entries
    # bit 1 of the timer column: the timer at the fire time is registered (where that time is neither maxTimestamp
    # nor the cleanup time, whose own timers the reference's set does not tell apart)
    lat = cfg.get("lateness", 0)
    regd = {(int(r["key"]), (int(r["start"]), int(r["end"]))) for r in rows
            if r["timer"] & 2 and r["fire_time"] not in (r["end"] - 1, r["end"] - 1 + lat)}
    assert regd == {(key, w) for (key, w), f in ref.ref.fire.items()
                    if (f, key, w) in ref.ref.timers and f not in (w[1] - 1, w[1] - 1 + lat)}
    if cfg.get("purging"):  # dead chains: a fire time with no timer behind it, over purged contents
        assert any((r["timer"] & 2) == 0 and r["fire_time"] != FIRE_NULL and r["count"] == 0 for r in rows)
    else:  # stuck chains (fire == maxTimestamp, fired) beside live ones
        assert any(r["fire_time"] == r["end"] - 1 and (r["timer"] & 2) == 0 for r in rows)
    assert any(r["timer"] & 2 for r in rows)
    halves = [_Gpu(key_group_range=KeyGroupRange(0, 63), **cfg), _Gpu(key_group_range=KeyGroupRange(64, 127), **cfg)]
    for op in halves:
        op.op.initialize_state(snap)
        op.op.epoch = gpu.op.epoch
        op.op.advance_watermark(wm)
        op.op.epoch -= 1
    st = [op.op.stats() for op in halves]
    assert sum(s["keyed_state_entries"] for s in st) == ref.ref.num_state_entries
    assert sum(s["event_time_timers"] for s in st) == ref.ref.num_timers
    kgs = np.array([_kg(int(x)) for x in k[h:]])
    for o in (gpu, ref):
        o.process(k[h:], t[h:], v[h:])
    for op, (lo, hi) in zip(halves, ((0, 63), (64, 127))):
        m = (kgs >= lo) & (kgs <= hi)
        op.process(k[h:][m], t[h:][m], v[h:][m])
    for o in [gpu, ref] + halves:
        o.watermark(int(t.max()) - 70)
        o.watermark(LMAX)
    _assert_rows(gpu, ref)
    later = [r for r in ref.row_tuples() if r[0] > 0]
    assert sorted(halves[0].row_tuples() + halves[1].row_tuples()) == later and len(later) > 0
    for op in halves:
        op.close()
    gpu.close()


def _kg(key, max_par=128):
    from flink_amd.keygroups import assign_to_key_group, long_hash_code
    return assign_to_key_group(long_hash_code(key), max_par)


# rows of one window [0, 100) as (count, sum, min, max, timer, fire_time); the first one is an emptied window whose
# sum / min / max are junk a restore must not read
_MERGE_ROWS = [(0, 999, -777, 888, 0b10, 30), (3, 60, 10, 30, 0b01, 20), (2, -5, -7, 2, 0b10, 20),
               (4, 100, 1, 50, 0b01, FIRE_NULL)]
_NULL_ROWS = [(1, 8, 8, 8, 0b01, FIRE_NULL), (2, 11, 5, 6, 0b00, FIRE_NULL)]


def _merged(rows):
    """what the rows of one (key, window) restore to: AggregateFunction.merge of the rows with contents, the fire time
    by Min over the non-null ones, maxTimestamp's timer if any row has it, the fire timer of the rows at that Min"""
    full = [r for r in rows if r[0] > 0]
    fires = [r[5] for r in rows if r[5] != FIRE_NULL]
    fire = min(fires) if fires else FIRE_NULL
    timer = int(any(r[4] & 1 for r in rows)) | 2 * int(any(r[4] & 2 for r in rows if fires and r[5] == fire))
    return (sum(r[0] for r in full), sum(r[1] for r in full), min((r[2] for r in full), default=None),
            max((r[3] for r in full), default=None), timer, fire)


@pytest.mark.parametrize("lateness", [0, 30])
def test_gpu_agg_continuous_restore_merges_repeated_rows(lateness):
    """rows of one (key, window) merge on restore, within one call (a round per repetition) and onto a window an
    earlier call restored: key 1 in one call with the emptied row first (it is the one inserted), key 2 in two calls
    with the emptied row merging, key 3 with null fire times only, key 4 an emptied window alone"""
    gpu = _Gpu("long", assigner="tumbling", size=100, interval=10, lateness=lateness)
    calls = [(1, _MERGE_ROWS), (2, _MERGE_ROWS[2:]), (2, _MERGE_ROWS[:2]), (3, _NULL_ROWS), (4, _MERGE_ROWS[:1])]
    for key, rows in calls:
        a = np.zeros(len(rows), dtype=gpu.op.state_dtype())
        for i, (cnt, sm, mn, mx, timer, fire) in enumerate(rows):
            a[i] = (key, 0, 100, cnt, sm, mn, mx, timer, fire)
        gpu.op.restore_key_group(_kg(key), a)
    exp = {1: _merged(_MERGE_ROWS), 2: _merged(_MERGE_ROWS), 3: _merged(_NULL_ROWS), 4: _merged(_MERGE_ROWS[:1])}
    assert exp[1] == (9, 155, -7, 50, 0b11, 20) and exp[3][4:] == (0b01, FIRE_NULL) and exp[4][0] == 0
    back = np.concatenate(list(gpu.op.snapshot_state().values()))
    back = back[np.argsort(back["key"])]
    assert back["key"].tolist() == [1, 2, 3, 4]  # one row per (key, window)
    assert back["start"].tolist() == [0] * 4 and back["end"].tolist() == [100] * 4
    for r in back:
        cnt, sm, mn, mx, timer, fire = exp[int(r["key"])]
        assert (int(r["count"]), int(r["timer"]), int(r["fire_time"])) == (cnt, timer, fire), int(r["key"])
        if cnt:  # (an emptied window's sum / min / max are not state)
            assert (int(r["sum"]), int(r["min"]), int(r["max"])) == (sm, mn, mx), int(r["key"])
    assert gpu.op.stats()["keyed_state_entries"] == sum(1 for e in exp.values() if e[0] > 0) == 3
    gpu.close()


def test_gpu_agg_continuous_combiner_refused():
    gpu = _Gpu(assigner="tumbling", size=100, interval=10)
    with pytest.raises(N.NativeError) as e:
        gpu.op.combine_extract(1)
    assert e.value.code == N.FW_ERR_UNSUPPORTED and "no arrival order" in str(e.value)
    import torch
    z = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(6)]
    with pytest.raises(N.NativeError) as e:
        gpu.op.push_partials(*z, config=1)
    assert e.value.code == N.FW_ERR_UNSUPPORTED and "no arrival order" in str(e.value)
    gpu.close()

"""DeltaTrigger on the GPU window-contents operator (fw_list_*, FW_TRIGGER_DELTA) against the TopSpeedWindowing
example's own expected output and, on seeded streams, against the plain-Python restatement (tests/delta_ref.py).  Bar:
every firing's row (key, window, count, sum, min, max as integer / f64 bit patterns, first ordinal) and its contents
in list order are equal per watermark epoch, as multisets (TestHarnessUtil's rule)."""
from collections import Counter

import numpy as np
import pytest

from flink_amd import (CountEvictor, DeltaEvictor, DeltaTrigger, EventTimeTrigger, GlobalWindows, KeyGroupRange,
                       PurgingTrigger, SlidingEventTimeWindows, TimeEvictor, TumblingEventTimeWindows,
                       assign_to_key_group, long_hash_code)
from flink_amd import _native as N
from tests import delta_util as U
from tests.delta_ref import DeltaRef, max_by_speed

pytestmark = pytest.mark.gpu

LMAX = U.LMAX
_VT = {"i64": "long", "i32": "int", "f64": "double", "i16": "short", "i8": "byte", "f32": "float"}
CARS, TOP_SPEEDS, THRESHOLD, EVICTOR_MS = U.load_topspeed()


def _gpu(assigner="tumbling", size=0, slide=0, offset=0, lateness=0, threshold=0.0, purging=False, evictor="none",
         evict_after=False, evict_arg=0, evict_threshold=0.0, side_output=False, value_type="i64", **gpu_kw):
    from flink_amd.listwindow import GpuListWindowOperator
    asg = {"global": GlobalWindows.create, "tumbling": lambda: TumblingEventTimeWindows.of(size, offset),
           "sliding": lambda: SlidingEventTimeWindows.of(size, slide, offset)}[assigner]()
    trig = DeltaTrigger.of(threshold)
    ev = {"none": lambda: None, "count": lambda: CountEvictor.of(evict_arg, evict_after),
          "time": lambda: TimeEvictor.of(evict_arg, evict_after),
          "delta": lambda: DeltaEvictor.of(evict_threshold, evict_after)}[evictor]()
    op = GpuListWindowOperator(asg, PurgingTrigger.of(trig) if purging else trig, ev, allowed_lateness=lateness,
                               side_output=side_output, value_type=_VT[value_type], **gpu_kw)
    op.wants_f64 = value_type in U.FLOATS
    return op


def _pair(gpu_kw=None, **cfg):
    return _gpu(**cfg, **(gpu_kw or {})), DeltaRef(**cfg)


def _registry_cfg(cfg):
    c = {k: v for k, v in cfg.items() if k not in ("keys", "n")}
    unit = U.UNIT[c["value_type"]]
    return dict(c, threshold=U.TRIGGER_UNITS * unit, evict_threshold=U.EVICT_UNITS * unit)


def _assert_side(gpu, ref):
    gs = sorted(map(tuple, np.stack([gpu.side_rows()[f] for f in ("epoch", "key", "ts", "val")], 1).tolist()))
    assert gs == sorted(zip(*[c.tolist() for c in ref.side_rows()]))


def _stats_equal(gpu, ref):
    st = gpu.stats()
    assert st["keyed_state_entries"] == ref.num_state_entries
    assert st["event_time_timers"] == ref.num_timers
    assert st["late_records_dropped"] == ref.late_dropped


# ---------------------------------------------------------------- the example
@pytest.mark.parametrize("chunk", [200, 1, 7, 64])
def test_gpu_top_speed_windowing(chunk):
    # keyBy(0).window(GlobalWindows).evictor(TimeEvictor.of(10 s)).trigger(DeltaTrigger.of(50, new.f2 - old.f2)): the
    # handle's value field is f2, the distance; maxBy(1) is the host's, over each firing's contents
    cfg = dict(assigner="global", threshold=THRESHOLD, evictor="time", evict_arg=EVICTOR_MS, value_type="f64")
    gpu, ref = _pair(**cfg)
    k = np.array([c[0] for c in CARS], dtype=np.int64)
    t = np.array([c[3] for c in CARS], dtype=np.int64)
    v = np.array([c[2] for c in CARS], dtype=np.float64)
    for a in range(0, len(CARS), chunk):
        gpu.process(k[a:a + chunk], t[a:a + chunk], v[a:a + chunk])
    ref.process(k, t, v)
    assert sorted(max_by_speed(CARS, gpu.contents())) == sorted(TOP_SPEEDS)
    U.assert_same(gpu, ref, "f64")
    # row for row: a key's firings come out in the order of its elements
    for car in (0, 1):
        assert [r for r in max_by_speed(CARS, gpu.contents()) if r[0] == car] == \
            [r for r in max_by_speed(CARS, ref.contents()) if r[0] == car]
    gpu.close()


# ---------------------------------------------------------------- seeded parity
@pytest.mark.parametrize("i", range(len(U.CONFIGS)), ids=[U.config_id(c) for c in U.CONFIGS])
def test_gpu_delta_vs_restatement(i):
    cfg = U.CONFIGS[i]
    vt = cfg["value_type"]
    gpu, ref = _pair(**_registry_cfg(cfg))
    k, t, v = U.stream_of(i, cfg)
    U.drive([gpu, ref], k, t, v, seed=i, each=lambda: _stats_equal(gpu, ref))
    U.assert_same(gpu, ref, vt)
    assert len(gpu.rows()) > 0
    if cfg.get("side_output"):
        _assert_side(gpu, ref)
    else:
        assert gpu.late_dropped == ref.late_dropped
    gpu.close()


# ---------------------------------------------------------------- long lists
@pytest.mark.parametrize("evictor", ["none", "count"])
def test_gpu_delta_long_list(evictor):
    # one list of 4096 new elements, every 16th fires: 255 firings, where one firing per new element would be sized
    # 4096 * 4096 elements
    n = 4096
    cfg = dict(assigner="global", threshold=15.0, evictor=evictor, evict_arg=8)
    gpu, ref = _pair(**cfg)
    k, t, v = np.full(n, 42, dtype=np.int64), np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)
    gpu.process_batch(k, t, v)
    ref.process(k, t, v)
    rows, elems, _ = gpu.pending()
    assert rows == len(ref.rows()) == n // 16 - 1
    assert elems == int(ref.rows()["count"].sum())  # the element buffer holds exactly the firings' contents
    assert elems == (8 * rows if evictor == "count" else sum(16 * f + 1 for f in range(1, n // 16)))
    gpu._collect(gpu.epoch)
    U.assert_same(gpu, ref, "i64")
    gpu.close()


# ---------------------------------------------------------------- no firing at the watermark
def test_gpu_delta_never_fires_on_time():
    cfg = dict(assigner="tumbling", size=1000, lateness=500, threshold=1e9)
    gpu, ref = _pair(**cfg)
    k, t, v = U.delta_stream(5, 6000, ("uniform", 256), "i64")
    U.drive([gpu, ref], k, t, v, batches=5, seed=5, each=lambda: _stats_equal(gpu, ref))
    assert len(gpu.rows()) == 0 == len(ref.rows()) and gpu.pending()[:2] == (0, 0)
    st = gpu.stats()
    assert st["keyed_state_entries"] == 0 and st["event_time_timers"] == 0 and st["current_watermark"] == LMAX
    assert all(len(lists) == 0 for lists, _ in gpu.snapshot_state().values())  # the trigger's state went with the windows
    assert not ref.last
    gpu.close()


# ---------------------------------------------------------------- compaction
def test_gpu_delta_state_survives_compaction():
    # fw_list.hip maybe_compact: dead elements > 2^16 and the majority of the log.  Every second element of a key fires
    # and purges its list, so the dead elements follow the records: the second push of 36000 passes 2^16.  The lists are
    # then empty and only the last elements remain, in the rebuilt map: the later pushes' firings need them.
    cfg = dict(assigner="global", threshold=15.0, purging=True)
    gpu, ref = _pair(**cfg)
    n, keys, pushes = 144000, 1000, 4
    k = np.arange(n, dtype=np.int64) % keys
    v = (np.arange(n, dtype=np.int64) // keys) * 10
    t = np.arange(n, dtype=np.int64)
    grows = []
    for p in range(pushes):
        sl = slice(p * n // pushes, (p + 1) * n // pushes)
        gpu.process(k[sl], t[sl], v[sl])
        ref.process(k[sl], t[sl], v[sl])
        grows.append(gpu.stats()["table_grows"])
    assert grows[0] == 0 and grows[1] > 0, grows  # compacted after the second push, with pushes still to come
    assert len(gpu.rows()) == len(ref.rows()) == keys * ((n // keys - 1) // 2)
    U.assert_same(gpu, ref, "i64")
    gpu.close()


# ---------------------------------------------------------------- snapshot / restore / rescale
SNAP_CFG = dict(assigner="tumbling", size=1000, lateness=500, threshold=8.0, purging=True)


def _first_half():
    gpu, ref = _pair(**SNAP_CFG)
    k, t, v = U.delta_stream(77, 12000, ("uniform", 256), "i64", span=6000)
    h = 6000
    wm = int(t[:h].max()) - 100
    for o in (gpu, ref):
        o.process(k[:h // 2], t[:h // 2], v[:h // 2])
        o.process(k[h // 2:h], t[h // 2:h], v[h // 2:h])
        o.watermark(wm)
    return gpu, ref, (k, t, v), h, wm


def _finish(ops, k, t, v):
    for o, sel in ops:
        o.process(k[sel], t[sel], v[sel])
        o.watermark(int(t.max()) - 100)
        o.watermark(LMAX)


def _later(ref):
    exp = U.firings(ref, "i64", ordinals=False)
    for f in [f for f in exp if f[0] == 0]:  # (a restored operator starts after the first epoch)
        del exp[f]
    return exp


@pytest.mark.parametrize("parts", [1, 2])
def test_gpu_delta_snapshot_restore(parts):
    gpu, ref, (k, t, v), h, wm = _first_half()
    snap = gpu.snapshot_state()
    lists = np.concatenate([s[0] for s in snap.values()])
    # the trigger_count column holds the last elements' value bits, timer 4 = present; purged windows are empty lists
    last = {(int(r["key"]), (int(r["start"]), int(r["end"]))): int(r["trigger_count"]) for r in lists if r["timer"] == 4}
    assert last == ref.last and len(last) > 0
    assert set(lists["timer"].tolist()) == {4}
    assert int(((lists["n_elems"] == 0) & (lists["timer"] == 4)).sum()) > 0
    assert int((lists["n_elems"] > 0).sum()) == ref.num_state_entries
    ranges = [KeyGroupRange(0, 127)] if parts == 1 else [KeyGroupRange(0, 63), KeyGroupRange(64, 127)]
    ops = []
    for r in ranges:
        op = _gpu(key_group_range=r, **SNAP_CFG)
        op.initialize_state(snap)
        op.epoch = gpu.epoch
        op.advance_watermark(wm)
        op.epoch -= 1
        ops.append(op)
    st = [op.stats() for op in ops]
    assert sum(s["keyed_state_entries"] for s in st) == ref.num_state_entries
    assert sum(s["event_time_timers"] for s in st) == ref.num_timers
    kg = np.array([assign_to_key_group(long_hash_code(int(x)), 128) for x in k[h:]])
    sels = [np.flatnonzero((kg >= r.start_key_group) & (kg <= r.end_key_group)) + h for r in ranges]
    _finish([(gpu, slice(h, None)), (ref, slice(h, None))] + list(zip(ops, sels)), k, t, v)
    U.assert_same(gpu, ref, "i64")  # the uninterrupted run
    got = sum((U.firings(op, "i64", ordinals=False) for op in ops), Counter())
    assert got == _later(ref) and sum(got.values()) > 0
    for op in ops + [gpu]:
        op.close()


def test_gpu_delta_restore_refusals():
    from flink_amd.listwindow import GpuListWindowOperator
    gpu, ref, (k, t, v), h, wm = _first_half()
    snap = gpu.snapshot_state()
    kg, (lists, elems) = next((g, s) for g, s in snap.items() if len(s[0]) > 1)
    before = (gpu.stats(), gpu.snapshot_key_group(kg))

    def same_as_before(op, was):
        st, (l2, e2) = op.stats(), op.snapshot_key_group(kg)
        assert st == was[0] and l2.tolist() == was[1][0].tolist() and e2.tolist() == was[1][1].tolist()

    for bits in (1, 2, 5, 8):  # a delta handle has no trigger timer, and knows no other bit
        bad = lists.copy()
        bad["timer"][-1] = bits
        with pytest.raises(N.NativeError) as e:
            gpu.restore_key_group(kg, bad, elems)
        assert e.value.code == N.FW_ERR_ARG and "timer bits" in str(e.value)
        same_as_before(gpu, before)
    other = GpuListWindowOperator(TumblingEventTimeWindows.of(1000), EventTimeTrigger.create(), allowed_lateness=500)
    was = (other.stats(), other.snapshot_key_group(kg))
    with pytest.raises(N.NativeError) as e:  # the last-element bit on a handle of another trigger
        other.restore_key_group(kg, lists, elems)
    assert e.value.code == N.FW_ERR_ARG and "timer bits" in str(e.value)
    same_as_before(other, was)
    # untouched: the stream goes on as if nothing had been tried
    _finish([(gpu, slice(h, None)), (ref, slice(h, None))], k, t, v)
    U.assert_same(gpu, ref, "i64")
    other.close()
    gpu.close()

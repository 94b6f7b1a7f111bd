"""ContinuousEventTimeTrigger on the GPU window-contents operator (fw_list_*, libflinkwin.so) against the reference's
known-answer sequences and the plain-Python restatement (tests/continuous_ref.py) on seeded streams.  Bar: every
firing's row (key, window, count, sum, min, max as integer / f64 bit patterns, first ordinal) and its contents in list
order are equal, epoch by epoch."""
import numpy as np
import pytest

from flink_amd import (ContinuousEventTimeTrigger, CountEvictor, EventTimeSessionWindows, GlobalWindows,
                       KeyGroupRange, PurgingTrigger, SlidingEventTimeWindows, TimeEvictor, TumblingEventTimeWindows)
from tests.continuous_ref import (LMIN, NONMERGING_CONFIGS, SESSION_CONFIGS, ContinuousRef, drive,
                                  load_continuous_kats, replay_kat, seeded_stream, zipf_stream)
from tests.test_gpu_list import _assert_same, _firings, _pair

pytestmark = pytest.mark.gpu

KATS = load_continuous_kats()
_VT = {"i64": "long", "f64": "double"}


def _gpu(assigner="tumbling", size=0, slide=0, offset=0, gap=0, lateness=0, interval=0, purging=False, evictor="none",
         evict_after=False, evict_arg=0, side_output=False, value_type="i64", **gpu_kw):
    from flink_amd.listwindow import GpuListWindowOperator
    asg = {"global": GlobalWindows.create, "session": lambda: EventTimeSessionWindows.with_gap(gap),
           "tumbling": lambda: TumblingEventTimeWindows.of(size, offset),
           "sliding": lambda: SlidingEventTimeWindows.of(size, slide, offset)}[assigner]()
    trig = ContinuousEventTimeTrigger.of(interval)
    ev = {"none": None, "count": CountEvictor.of(evict_arg, evict_after), "time": TimeEvictor.of(evict_arg, evict_after)}
    op = GpuListWindowOperator(asg, PurgingTrigger.of(trig) if purging else trig, ev[evictor],
                               allowed_lateness=lateness, side_output=side_output, value_type=_VT[value_type], **gpu_kw)
    op.wants_f64 = value_type == "f64"
    return op


def _pair_c(value_type="i64", gpu_kw=None, **cfg):
    return _gpu(value_type=value_type, **cfg, **(gpu_kw or {})), \
        ContinuousRef(trigger="continuous", value_type=value_type, **cfg)


def _values(v, value_type):
    return (v.astype(np.float64) * 0.37).view(np.int64) if value_type == "f64" else v


def _assert_side(gpu, ref):
    gs = sorted(map(tuple, np.stack([gpu.side_rows()[f] for f in ("epoch", "key", "ts", "val")], 1).tolist()))
    assert gs == sorted(zip(*[c.tolist() for c in ref.side_rows()]))


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_gpu_continuous_kats(case):
    gpu, ref = _pair_c(**case["cfg"])
    for i, (got, exp) in enumerate(replay_kat(case, gpu)):
        assert got == exp, (case["name"], i)
    replay_kat(case, ref)
    _assert_same(gpu, ref)  # and the contents of every firing
    gpu.close()


@pytest.mark.parametrize("cfg", NONMERGING_CONFIGS, ids=[str(i) for i in range(len(NONMERGING_CONFIGS))])
@pytest.mark.parametrize("value_type", ["i64", "f64"])
def test_gpu_continuous_vs_restatement(cfg, value_type):
    gpu, ref = _pair_c(value_type, **cfg)
    k, t, v = seeded_stream(7 + len(str(cfg)), 20000, 37, 2000, 150)

    def stats():  # numKeyedStateEntries / numEventTimeTimers while windows are open
        st = gpu.stats()
        assert st["keyed_state_entries"] == ref.num_state_entries
        assert st["event_time_timers"] == ref.num_timers

    drive([gpu, ref], k, t, _values(v, value_type), final=(500, "bounded" if cfg["assigner"] == "global" else "max"),
          each=stats)
    _assert_same(gpu, ref)
    assert gpu.late_dropped == ref.late_dropped
    if cfg.get("side_output"):
        _assert_side(gpu, ref)
    stats()
    gpu.close()


@pytest.mark.parametrize("cfg", SESSION_CONFIGS, ids=[str(i) for i in range(len(SESSION_CONFIGS))])
@pytest.mark.parametrize("value_type,zipf", [("i64", False), ("f64", True)], ids=["i64-uniform", "f64-zipf"])
def test_gpu_continuous_sessions_vs_restatement(cfg, value_type, zipf):
    gpu, ref = _pair_c(value_type, **cfg)
    k, t, v = (zipf_stream if zipf else seeded_stream)(23 + len(str(cfg)), 20000, 300 if zipf else 400, 20000, 150)
    drive([gpu, ref], k, t, _values(v, value_type))
    _assert_same(gpu, ref)
    assert gpu.late_dropped == ref.late_dropped
    if cfg.get("side_output"):
        _assert_side(gpu, ref)
    rows = gpu.rows()
    assert (rows["end"] - rows["start"] > cfg["gap"]).any() and ref.merges > 0  # sessions merged
    assert ref.fire_from_other > 0  # and a merged window took its fire time from a window that was not the target
    gpu.close()


@pytest.mark.parametrize("cfg", [dict(assigner="tumbling", size=50, lateness=20, interval=20),
                                 dict(assigner="session", gap=25, lateness=100, interval=40)],
                         ids=["tumbling", "session"])
def test_gpu_continuous_growth_and_compaction(cfg):
    # a log and a map far smaller than the stream: the fire times survive map rebuilds and log compactions
    gpu, ref = _pair_c(gpu_kw=dict(expected_elements=1024), **cfg)
    k, t, v = seeded_stream(31, 100000, 3000, 50000, 60)
    drive([gpu, ref], k, t, v, bound=50)
    _assert_same(gpu, ref)
    assert gpu.stats()["table_grows"] > 0
    gpu.close()


def test_gpu_continuous_firings_limit():
    from flink_amd import _native as N
    gpu, ref = _pair_c(assigner="global", interval=1)
    for h in (gpu, ref):
        h.process(np.array([1]), np.array([5]), np.array([3]))
    with pytest.raises(N.NativeError) as e:
        gpu.advance_watermark(1 << 40)
    assert e.value.code == N.FW_ERR_UNSUPPORTED
    assert "2^20 trigger intervals" in str(e.value)
    for h in (gpu, ref):  # nothing was changed: a smaller advance works, from the same state
        h.watermark(1000)
    assert len(gpu.rows()) == 1000 - 5
    _assert_same(gpu, ref)
    gpu.close()


def test_gpu_continuous_snapshot_restore():
    # every key group moved into a fresh operator mid-stream: its later firings equal an unsnapshotted twin's, and
    # the snapshot's trigger_count column holds the fire times
    cfg = dict(assigner="tumbling", size=100, lateness=50, interval=30)
    gpu, ref = _pair_c(**cfg)
    k, t, v = seeded_stream(21, 20000, 200, 2000, 60)
    h = 10000
    wm = int(t[:h].max()) - 70
    for o in (gpu, ref):
        o.process(k[:h], t[:h], v[:h])
        o.watermark(wm)
    snap = gpu.snapshot_state()
    lists = np.concatenate([s[0] for s in snap.values()])
    fires = {(int(r["key"]), (int(r["start"]), int(r["end"]))): int(r["trigger_count"]) for r in lists
             if r["trigger_count"] != LMIN}
    assert fires == ref.fire and len(fires) > 0
    assert sum(int((s[0]["n_elems"] > 0).sum()) for s in snap.values()) == ref.num_state_entries
    op = _gpu(key_group_range=KeyGroupRange(0, 127), **cfg)
    op.initialize_state(snap)
    st = op.stats()
    assert st["keyed_state_entries"] == ref.num_state_entries and st["event_time_timers"] == ref.num_timers
    op.epoch = gpu.epoch
    op.advance_watermark(wm)
    op.epoch -= 1
    for o in (op, gpu, ref):
        o.process(k[h:], t[h:], v[h:])
        o.watermark(int(t.max()) - 70)
        o.watermark((1 << 63) - 1)
    _assert_same(gpu, ref)
    assert (gpu.rows()["epoch"] == 0).any() and (gpu.rows()["epoch"] > 0).any()
    got = _firings(op, ordinals=False)
    exp = _firings(ref, ordinals=False)
    for f in [f for f in exp if f[0] == 0]:  # (the restored operator starts after the first epoch)
        del exp[f]
    assert got == exp
    op.close()
    gpu.close()


@pytest.mark.parametrize("cfg", [dict(assigner="tumbling", size=100, lateness=60),
                                 dict(assigner="tumbling", size=100, trigger="count", trigger_count=3)],
                         ids=["event_time", "count"])
def test_gpu_list_other_triggers_unchanged(cfg):
    # the kernels this trigger shares with EventTimeTrigger and CountTrigger operators still give the oracle's rows
    gpu, ref = _pair(**cfg)
    k, t, v = seeded_stream(7, 20000, 37, 2000, 150)
    drive([gpu, ref], k, t, v)
    _assert_same(gpu, ref)
    gpu.close()

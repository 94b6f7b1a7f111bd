"""ContinuousEventTimeTrigger on the aggregating operator, without a GPU: what fw_create refuses (before it touches
the device), through ctypes and through GpuWindowOperator, and a vetting of every configuration and stream the GPU
tests use (tests/test_gpu_agg_continuous.py): ContinuousRef alone runs them and the classes of behaviour the GPU tests
mean to cover are asserted to occur."""
import ctypes

import numpy as np
import pytest

from flink_amd import (ContinuousEventTimeTrigger, CountSumMinMax, CountWindows, EventTimeSessionWindows,
                       FirstElementReduce, PurgingTrigger, TumblingEventTimeWindows)
from flink_amd import _native as N
from flink_amd.operator import GpuWindowOperator
from tests import agg_continuous_util as U
from tests.continuous_ref import LMAX, TimerRunaway, drive, load_continuous_kats, replay_kat, seeded_stream

CONT = N.FW_TRIGGER_CONTINUOUS_EVENT_TIME


def _create(**kw):
    c = N.FwConfig()
    c.key_group_start = c.key_group_end = -1
    for k, v in kw.items():
        setattr(c, k, v)
    h = ctypes.c_void_p()
    rc = N.lib().fw_create(ctypes.byref(c), ctypes.byref(h))
    msg = N.lib().fw_last_error(h).decode()
    N.lib().fw_destroy(h)
    return rc, msg


def _row_config(**kw):
    c = dict(aggregate=N.FW_AGG_ROW, row_columns=1, row_aggregates=1, **kw)
    return c


# every aggregate other than count/sum/min/max, each in a configuration fw_create takes under EventTimeTrigger
OTHER_AGGREGATES = {
    "hll": dict(aggregate=N.FW_AGG_HLL),
    "first": dict(aggregate=N.FW_AGG_FIRST),
    "first_max": dict(aggregate=N.FW_AGG_FIRST_MAX),
    "minby": dict(aggregate=N.FW_AGG_MINBY),
    "maxby": dict(aggregate=N.FW_AGG_MAXBY),
    "tdigest": dict(aggregate=N.FW_AGG_TDIGEST, value_type=N.FW_VAL_F64),
    "row": _row_config(),
}


@pytest.mark.parametrize("kw,code,fragment", [
    (dict(assigner=N.FW_SESSION, gap=30), N.FW_ERR_UNSUPPORTED, "session windows is not offered on the aggregating"),
    (dict(assigner=N.FW_COUNT, size=10, slide=5, aggregate=N.FW_AGG_FIRST), N.FW_ERR_UNSUPPORTED,
     "count windows is not offered"),
    (dict(assigner=N.FW_TUMBLING, size=100, trigger_interval=0), N.FW_ERR_ARG,
     "ContinuousEventTimeTrigger interval must be > 0"),
    (dict(assigner=N.FW_TUMBLING, size=100, trigger_interval=-1), N.FW_ERR_ARG,
     "ContinuousEventTimeTrigger interval must be > 0"),
    (dict(assigner=N.FW_SLIDING, size=100, slide=20, trigger_interval=-1), N.FW_ERR_ARG,
     "ContinuousEventTimeTrigger interval must be > 0"),
    (dict(assigner=N.FW_TUMBLING, size=1 << 59, trigger_interval=1 << 59), N.FW_ERR_UNSUPPORTED, "may not exceed 2^60"),
] + [(dict(assigner=N.FW_TUMBLING, size=100, **a), N.FW_ERR_UNSUPPORTED,
      "is offered for the count/sum/min/max aggregate") for a in OTHER_AGGREGATES.values()],
    ids=["session", "count", "interval-0", "interval-neg", "interval-neg-sliding", "span"] + list(OTHER_AGGREGATES))
def test_create_refuses(kw, code, fragment):
    kw = dict(kw)
    kw.setdefault("trigger_interval", 10)
    rc, msg = _create(trigger=CONT, **kw)
    assert rc == code, msg
    assert fragment in msg
    if code == N.FW_ERR_UNSUPPORTED and "2^60" not in fragment:  # the message names where the job runs instead
        assert "fw_list_create" in msg


def test_create_refuses_unknown_trigger():
    rc, msg = _create(assigner=N.FW_TUMBLING, size=100, trigger=N.FW_TRIGGER_COUNT)
    assert rc == N.FW_ERR_ARG and "unknown trigger" in msg


@pytest.mark.parametrize("name", list(OTHER_AGGREGATES))
def test_other_aggregates_still_pass_the_checks_without_the_trigger(name):
    # (the configurations above are refused for the trigger, not for something else: with EventTimeTrigger the checks
    # pass and fw_create goes on to the device, which this machine may not have)
    rc, msg = _create(assigner=N.FW_TUMBLING, size=100, device=1 << 20, **OTHER_AGGREGATES[name])
    assert rc == N.FW_ERR_HIP, (rc, msg)


def _trigger(interval):
    t = ContinuousEventTimeTrigger.of(5)
    t.interval = interval  # (of() itself refuses a non-positive interval: the operator's own check is what is tested)
    return t


@pytest.mark.parametrize("make,code,fragment", [
    (lambda: GpuWindowOperator(EventTimeSessionWindows.with_gap(30), trigger=_trigger(10)), N.FW_ERR_UNSUPPORTED,
     "session windows is not offered"),
    (lambda: GpuWindowOperator(CountWindows.of(10, 5), FirstElementReduce("long"), trigger=_trigger(10)),
     N.FW_ERR_UNSUPPORTED, "count windows is not offered"),
    (lambda: GpuWindowOperator(TumblingEventTimeWindows.of(100), FirstElementReduce("long"),
                               trigger=PurgingTrigger.of(_trigger(10))), N.FW_ERR_UNSUPPORTED,
     "is offered for the count/sum/min/max aggregate"),
    (lambda: GpuWindowOperator(TumblingEventTimeWindows.of(100), trigger=_trigger(0)), N.FW_ERR_ARG,
     "interval must be > 0"),
    (lambda: GpuWindowOperator(TumblingEventTimeWindows.of(100), CountSumMinMax("double"),
                               trigger=PurgingTrigger.of(_trigger(-1))), N.FW_ERR_ARG, "interval must be > 0"),
], ids=["session", "count", "first", "interval-0", "interval-neg"])
def test_operator_refuses(make, code, fragment):
    with pytest.raises(N.NativeError) as e:
        make()
    assert e.value.code == code and fragment in str(e.value)


def test_config_fields_and_snapshot_dtype():
    from flink_amd.operator import FIRE_STATE_DTYPE
    fields = [f for f, _ in N.FwConfig._fields_]
    assert fields[-2:] == ["trigger", "trigger_interval"] and fields[-3] == "no_panes"  # pad1's slot, then appended
    assert N.FwConfig.trigger_interval.offset == N.FwConfig.trigger.offset + 4 == ctypes.sizeof(N.FwConfig) - 8
    assert N.FW_TRIGGER_EVENT_TIME == 0  # a zeroed field: the existing behaviour
    assert FIRE_STATE_DTYPE.names[-1] == "fire_time" and FIRE_STATE_DTYPE.names[-2] == "timer"


# ---------------------------------------------------------------- the GPU tests' streams, vetted with ContinuousRef
def _run_seeded(cfg):
    ref = U.ref_of(**cfg)
    k, t, v = seeded_stream(U.seed_of(cfg), 20000, 37, 2000, 150)
    during = []

    def each():
        during.append(len(ref._rows))
    drive([ref], k, t, v, each=each)
    return ref, k, t


def _armed_off_minimum(ref, k, t, batches=10):
    """windows whose fire time is not the one their minimum-timestamp element of the first push that reached them
    would have set: armed by an element that is not the minimum"""
    # replay the arming rule push by push on the first push each window appears in
    n = len(k) // batches
    seen, off = set(), 0
    cfg = ref
    for b in range(batches):
        first, mn = {}, {}
        for key, ts in zip(k[b * n:(b + 1) * n].tolist(), t[b * n:(b + 1) * n].tolist()):
            for w in cfg._assign(ts):
                kw = (key, w)
                if kw in seen:
                    continue
                first.setdefault(kw, ts)
                mn[kw] = min(mn.get(kw, ts), ts)
        for kw in first:
            seen.add(kw)
            iv = cfg.interval
            if first[kw] - first[kw] % iv != mn[kw] - mn[kw] % iv:
                off += 1
    return off


@pytest.mark.parametrize("cfg", U.SEEDED_CONFIGS, ids=U.SEEDED_IDS)
def test_seeded_configurations_cover_what_the_gpu_tests_mean(cfg):
    try:
        ref, k, t = _run_seeded(cfg)
    except TimerRunaway:
        pytest.fail("TimerRunaway")
    assert len(ref.early_by_window) > 0  # early firings
    if cfg == U.SEEDED_CONFIGS[0]:
        assert len(ref.stuck_windows) > 0  # the interval-11 tumbling windows that meet maxTimestamp
    rows = ref.rows()
    assert len(rows) > 0 and (t < 0).any()  # negative timestamps
    assert _armed_off_minimum(ref, k, t) > 0  # armed by an element that is not the window's minimum
    # duplicates: some window fires more than once in one advance
    tup = [tuple(r)[:8] + (int(r["epoch"]),) for r in rows]
    assert len(set(tup)) < len(tup) or cfg.get("purging")


def test_seeded_configurations_have_late_firings():
    # a row emitted during process (an element of a window whose maxTimestamp the watermark has passed)
    late = 0
    for cfg in U.SEEDED_CONFIGS:
        ref = U.ref_of(**cfg)
        k, t, v = seeded_stream(U.seed_of(cfg), 20000, 37, 2000, 150)
        n = len(k) // 10
        wm = -10**9
        for b in range(10):
            before = len(ref._rows)
            ref.process(k[b * n:(b + 1) * n], t[b * n:(b + 1) * n], v[b * n:(b + 1) * n])
            fired = len(ref._rows) - before
            late += fired
            assert fired == 0 or cfg.get("lateness", 0) > 0  # (only allowed lateness keeps such a window)
            wm = max(wm, int(t[b * n:(b + 1) * n].max()) - 100)
            if b % 3 != 1:
                ref.watermark(wm)
    assert late > 0


def test_value_columns():
    _, _, v = seeded_stream(7, 20000, 37, 2000, 150)
    w, wr = U.values_of(v, "int")
    assert (np.abs(w) >= 1 << 30).all() and (np.abs(w) < 1 << 31).all() and (w > 0).any() and (w < 0).any()
    assert U.wrap32((1 << 31) + 5) == -(1 << 31) + 5
    d, bits = U.values_of(v, "double")
    assert (d != 0).all() and (d * 8 == np.round(d * 8)).all() and (np.abs(d * 8) <= 1000).all()
    assert bits.dtype == np.int64
    # the sums of the int field do leave 32 bits in the seeded windows
    ref = U.ref_of("int", **U.SEEDED_CONFIGS[0])
    k, t, _ = seeded_stream(U.seed_of(U.SEEDED_CONFIGS[0]), 20000, 37, 2000, 150)
    drive([ref], k, t, wr)
    assert any(U.wrap32(r["sum"]) != int(r["sum"]) for r in ref.rows())


def test_kats_for_the_aggregating_operator():
    kats = [c for c in load_continuous_kats() if c["derived"] and c["cfg"]["assigner"] in ("tumbling", "sliding")]
    assert len(kats) == 7 and all(c["name"].startswith("derived_") for c in kats)
    for c in kats:
        ref = U.ref_of(**c["cfg"])
        for i, (got, exp) in enumerate(replay_kat(c, ref)):
            assert got == exp, (c["name"], i)


def test_split_stream():
    k, t, v = U.split_stream()
    assert k[0] == 1 and t[0] > 8 * 250 and np.median(t[k == 1]) < 3 * 250 and t.argmin() == 1
    ref = U.ref_of(assigner="tumbling", size=100000, interval=250)
    ref.process(k, t, v)
    assert ref.fire == {(1, (0, 100000)): 2500, (2, (0, 100000)): 1500}
    for wm in (1000, 1500, 2499, 2500, 2750, 3100, 99998, 99999):
        ref.watermark(wm)
    first = {}
    for r in ref.rows():
        first[int(r["key"])] = min(first.get(int(r["key"]), 99), int(r["epoch"]))
    assert first == {1: 3, 2: 1}


def test_growth_limit_range_and_snapshot_streams():
    ref = U.ref_of(**U.GROWTH_CONFIG)
    drive([ref], *U.growth_stream(), bound=50)
    assert len(ref.early_by_window) > 1024 and len(ref.rows()) > 0
    ref = U.ref_of(**U.LIMIT_CONFIG)
    ref.process(np.array([1]), np.array([5]), np.array([3]))
    ref.watermark(1000)
    assert len(ref.rows()) == 995
    for cfg in U.SNAPSHOT_CONFIGS:
        ref = U.ref_of(**cfg)
        k, t, v, h, wm = U.snapshot_stream()
        ref.process(k[:h], t[:h], v[:h])
        ref.watermark(wm)
        live = sum(1 for (key, w), f in ref.fire.items() if (f, key, w) in ref.timers and f != w[1] - 1)
        stuck = sum(1 for (key, w), f in ref.fire.items() if f == w[1] - 1 and (f, key, w) not in ref.timers)
        dead = sum(1 for (key, w), f in ref.fire.items()
                   if (f, key, w) not in ref.timers and f != w[1] - 1 and (key, w) not in ref.state)
        assert live > 0 and stuck > 0
        assert dead > 0 or not cfg.get("purging")
        ref.process(k[h:], t[h:], v[h:])
        ref.watermark(int(t.max()) - 70)
        ref.watermark(LMAX)
        assert (ref.rows()["epoch"] > 0).any()

"""DeltaTrigger, the part that needs no GPU: the TopSpeedWindowing example's own input and expected output through the
plain-Python restatement (tests/delta_ref.py), the mutations that fixture is said to catch, what the seeded streams of
tests/test_gpu_delta_trigger.py exercise, and the C-ABI's refusals, which come before the device is touched."""
import ctypes
import os
import subprocess

import pytest

from flink_amd import _native as N
from tests import delta_util as U
from tests.delta_ref import DeltaRef, top_speeds

CARS, TOP_SPEEDS, THRESHOLD, EVICTOR_MS = U.load_topspeed()
MERGING_MESSAGE = "A merging window assigner cannot be used with a trigger that does not support merging."


# ---------------------------------------------------------------- (a), (b) the example
def test_fixture_shape():
    assert len(CARS) == 200 and len(TOP_SPEEDS) == 71 and {c[0] for c in CARS} == {0, 1}
    assert THRESHOLD == 50.0 and EVICTOR_MS == 10000


def test_restatement_reproduces_top_speeds():
    # TopSpeedWindowingExampleITCase.java:50-62 compares sorted lines
    assert sorted(top_speeds(CARS, THRESHOLD, EVICTOR_MS)) == sorted(TOP_SPEEDS)


@pytest.mark.parametrize("name,kw", [
    ("no eviction", dict(ref_kw=dict(evictor="none"))),
    ("evictor 9 s", dict(evictor_ms=9000)),
    ("evictor 11 s", dict(evictor_ms=11000)),
    ("later element on ties", dict(later_on_ties=True)),
    ("last updated on every element", dict(ref_kw=dict(update_always=True))),
])
def test_fixture_catches_mutation(name, kw):
    args = dict(threshold=THRESHOLD, evictor_ms=EVICTOR_MS)
    args.update(kw)
    assert sorted(top_speeds(CARS, **args)) != sorted(TOP_SPEEDS), name


def test_fixture_does_not_pin_the_strict_comparison():
    # no example record has a delta equal to the threshold (the seeded streams do: below)
    assert sorted(top_speeds(CARS, THRESHOLD, EVICTOR_MS, ref_kw=dict(greater_equal=True))) == sorted(TOP_SPEEDS)


# ---------------------------------------------------------------- (c) what the seeded streams exercise
@pytest.fixture(scope="module")
def registry_hits():
    total, per_type = {}, {}
    for i, cfg in enumerate(U.CONFIGS):
        ref = U.ref_of(cfg)
        k, t, v = U.stream_of(i, cfg)
        U.drive([ref], k, t, v, seed=i)
        assert len(ref.rows()) > 0, U.config_id(cfg)
        ref.hits["late"], ref.hits["side"] = ref.late_dropped, len(ref._side)
        for name, n in ref.hits.items():
            total[name] = total.get(name, 0) + n
            per_type[(cfg["value_type"], name)] = per_type.get((cfg["value_type"], name), 0) + n
    return total, per_type


def test_seeded_streams_hit_the_edges(registry_hits):
    total, per_type = registry_hits
    assert total["equal"] > 0            # deltas exactly equal to the threshold: > and >= differ
    assert total["time_cutoff"] > 0      # a timestamp exactly at a TimeEvictor cutoff: <= and < differ
    assert per_type[("f64", "nan")] > 0  # NaN deltas (a NaN value, or Infinity - Infinity)
    assert per_type[("i32", "wrapped")] > 0  # an Integer delta that wraps
    assert total["after_purge"] > 0      # a window that receives elements after a purge emptied it
    assert total["reopened"] > 0         # a window cleaned up whose key later opens a new one
    assert total["first_of_push"] > 0    # firings on the first element of a push: the state crossed pushes
    assert total["late"] > 0 and total["side"] > 0  # numLateRecordsDropped and the side output
    for vt in ("i64", "i32", "f64", "i16", "i8", "f32"):
        assert per_type[(vt, "equal")] > 0, vt


def test_registry_covers_every_axis():
    for shape in ("tumbling", "sliding", "global"):
        cs = [c for c in U.CONFIGS if c["assigner"] == shape]
        assert {c.get("evictor", "none") for c in cs} == {"none", "count", "time", "delta"}, shape
        assert {bool(c.get("purging")) for c in cs} == {False, True}, shape
        assert {c["value_type"] for c in cs} >= {"i64", "i32", "f64"}, shape
        assert {c["keys"][0] for c in cs} == {"uniform", "zipf"}, shape
    for ev in ("count", "time", "delta"):
        assert {bool(c.get("evict_after")) for c in U.CONFIGS if c.get("evictor") == ev} == {False, True}, ev
    assert {c.get("lateness", 0) for c in U.CONFIGS} == {0, 500} and any(c.get("side_output") for c in U.CONFIGS)


def test_strict_comparisons_matter_on_the_seeded_streams():
    cfg = U.CONFIGS[0]
    k, t, v = U.stream_of(0, cfg)
    a, b = U.ref_of(cfg), U.ref_of(cfg)
    b.greater_equal = True
    U.drive([a, b], k, t, v, seed=0)
    assert U.firings(a, "i64") != U.firings(b, "i64")


def test_delta_trigger_never_fires_on_time():
    ref = DeltaRef(assigner="tumbling", size=100, threshold=1000.0)
    ref.process([1, 1, 2], [5, 50, 60], [1, 2, 3])
    assert ref.num_timers == 2 and ref.num_state_entries == 2 and len(ref.last) == 2  # cleanup timers only
    ref.watermark(U.LMAX)
    assert len(ref.rows()) == 0 and ref.num_timers == 0 and ref.num_state_entries == 0 and not ref.last


# ---------------------------------------------------------------- (d) the C-ABI before the device
def _create(join=0, **kw):
    c = N.FwListConfig()
    c.assigner, c.size, c.emit_contents = N.FW_TUMBLING, 100, 1
    c.key_group_start = c.key_group_end = -1
    c.trigger = N.FW_TRIGGER_DELTA
    for k, v in kw.items():
        setattr(c, k, v)
    h = ctypes.c_void_p()
    if join:
        jc = N.FwJoinConfig(join=join, max_join_pairs=0)
        rc = N.lib().fw_list_create_join(ctypes.byref(c), ctypes.byref(jc), ctypes.byref(h))
    else:
        rc = N.lib().fw_list_create(ctypes.byref(c), ctypes.byref(h))
    msg = N.lib().fw_list_last_error(h).decode() if h else ""
    N.lib().fw_list_destroy(h)
    return rc, msg


@pytest.mark.parametrize("merging_state", [0, 1])
def test_create_refuses_a_merging_assigner(merging_state):
    rc, msg = _create(assigner=N.FW_SESSION, merging_state=merging_state, trigger_threshold=1.0)
    assert rc == N.FW_ERR_ARG and msg == MERGING_MESSAGE, (rc, msg)


def test_create_refuses_a_nan_threshold():
    rc, msg = _create(trigger_threshold=float("nan"))
    assert rc == N.FW_ERR_ARG and "NaN" in msg, (rc, msg)


@pytest.mark.parametrize("join", [N.FW_JOIN_COGROUP, N.FW_JOIN_INNER])
def test_create_refuses_a_join(join):
    rc, msg = _create(join=join, trigger_threshold=1.0)
    assert rc == N.FW_ERR_UNSUPPORTED and "DeltaTrigger" in msg, (rc, msg)


def test_config_layout_is_unchanged(tmp_path):
    # the threshold shares the struct's last slot with trigger_interval (a trigger has one parameter): the size and
    # every existing offset stay
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in N.FwListConfig._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flink_window.h"\nint main(void) {\n'
                   '  printf("%d\\n", FW_TRIGGER_DELTA);\n'
                   '  printf("%zu\\n", sizeof(fw_list_config));\n'
                   '  printf("%zu\\n", offsetof(fw_list_config, trigger_threshold));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(fw_list_config, {f}));\n' for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == N.FW_TRIGGER_DELTA == 3
    assert out[1] == ctypes.sizeof(N.FwListConfig) == 136
    assert out[2] == N.FwListConfig.trigger_interval.offset == 128
    assert out[3:] == [getattr(N.FwListConfig, f).offset for f in fields]
    expected = dict(assigner=0, trigger=12, merging_state=52, size=56, trigger_count=88, evict_count=96,
                    delta_threshold=104, expected_elements=112, max_batch=120, trigger_interval=128)
    assert {f: getattr(N.FwListConfig, f).offset for f in expected} == expected
    c = N.FwListConfig()
    c.trigger_threshold = 50.0
    assert c.trigger_threshold == 50.0 and c.trigger_interval == 0x4049000000000000


# ---------------------------------------------------------------- the Python surface
def test_trigger_is_exported_and_purgeable():
    import flink_amd
    from flink_amd import DeltaTrigger, PurgingTrigger
    assert flink_amd.DeltaTrigger is DeltaTrigger and DeltaTrigger.of(50).threshold == 50.0
    p = PurgingTrigger.of(DeltaTrigger.of(2.5))
    assert p.purging and p.nested.threshold == 2.5
    with pytest.raises(ValueError):
        DeltaTrigger.of(float("nan"))


def test_operators_refuse_before_the_library():
    from flink_amd import DeltaTrigger, EventTimeSessionWindows, PurgingTrigger, TumblingEventTimeWindows
    from flink_amd.join import GpuWindowJoin
    from flink_amd.listwindow import GpuListWindowOperator
    for trig in (DeltaTrigger.of(1), PurgingTrigger.of(DeltaTrigger.of(1))):
        for ms in (False, True):
            with pytest.raises(ValueError) as e:
                GpuListWindowOperator(EventTimeSessionWindows.with_gap(10), trig, merging_state=ms)
            assert str(e.value) == MERGING_MESSAGE
        with pytest.raises(ValueError) as e:
            GpuWindowJoin(TumblingEventTimeWindows.of(100), trig)
        assert "DeltaTrigger" in str(e.value)

"""ContinuousEventTimeTrigger on the window-contents operator, the part that needs no GPU: the plain-Python
restatement (tests/continuous_ref.py) against the reference's known-answer sequences and, under EventTimeTrigger,
against the ListState oracle firing for firing; the C-ABI's new field, constant and refusal; the heap-state helper
and the export."""
import ctypes
from collections import Counter

import numpy as np
import pytest

from flink_amd import _native as N
from oracle import oracle as orc
from tests.continuous_ref import (LMIN, NONMERGING_CONFIGS, ContinuousRef, drive, hashset_order, load_continuous_kats,
                                  replay_kat, seeded_stream)

KATS = load_continuous_kats()


def _firings(op):
    out = Counter()
    for r, el in op.contents():
        ords = "ordinal" if "ordinal" in el.dtype.names else "ord"
        out[(int(r["epoch"]), int(r["key"]), int(r["start"]), int(r["end"]), int(r["count"]), int(r["sum"]),
             int(r["min"]), int(r["max"]), int(r["first"]),
             tuple(zip(el["ts"].tolist(), el["val"].tolist(), el[ords].tolist())))] += 1
    return out


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_restatement_reproduces_kats(case):
    ref = ContinuousRef(trigger="continuous", **case["cfg"])
    for i, (got, exp) in enumerate(replay_kat(case, ref)):
        assert got == exp, (case["name"], i)


def test_kat_file_names_its_sources():
    assert len(KATS) >= 8
    for c in KATS:
        assert ".java:" in c["source"]
        assert c["derived"] == c["source"].startswith("derived")


def _stream(seed, n, keys, span, jitter):  # (the seeded streams of tests/test_gpu_list.py)
    rng = np.random.default_rng(seed)
    k = rng.integers(0, keys, n, dtype=np.int64)
    t = np.arange(n, dtype=np.int64) * span // n - rng.integers(0, jitter, n, dtype=np.int64)
    v = rng.integers(-1000, 1000, n, dtype=np.int64)
    return k, t, v


def _zipf_stream(seed, n, keys, span, jitter, s=1.1):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, keys + 1) ** s
    k = rng.choice(keys, n, p=w / w.sum()).astype(np.int64) * 7919 + 13
    t = np.arange(n, dtype=np.int64) * span // n - rng.integers(0, jitter, n, dtype=np.int64)
    v = rng.integers(-1000, 1000, n, dtype=np.int64)
    return k, t, v


EVENT_TIME_CONFIGS = [
    dict(assigner="tumbling", size=100),
    dict(assigner="tumbling", size=100, purging=True, lateness=50, side_output=True),
    dict(assigner="tumbling", size=100, lateness=60),
    dict(assigner="sliding", size=100, slide=25),
    dict(assigner="sliding", size=90, slide=30, lateness=40),
    dict(assigner="tumbling", size=100, evictor="count", evict_arg=3),
    dict(assigner="tumbling", size=100, evictor="count", evict_arg=2, evict_after=True, lateness=30),
    dict(assigner="tumbling", size=200, evictor="time", evict_arg=50),
    dict(assigner="sliding", size=100, slide=50, evictor="time", evict_arg=20, evict_after=True),
    dict(assigner="session", gap=30),
    dict(assigner="session", gap=30, lateness=200),
    dict(assigner="session", gap=30, lateness=200, purging=True, side_output=True),
    dict(assigner="session", gap=50, purging=True),
    dict(assigner="session", gap=30, evictor="count", evict_arg=3),
    dict(assigner="session", gap=30, lateness=150, evictor="count", evict_arg=2, evict_after=True),
    dict(assigner="session", gap=40, evictor="time", evict_arg=25),
    dict(assigner="session", gap=40, lateness=100, evictor="time", evict_arg=10, evict_after=True, purging=True),
]


@pytest.mark.parametrize("cfg", EVENT_TIME_CONFIGS, ids=[str(i) for i in range(len(EVENT_TIME_CONFIGS))])
@pytest.mark.parametrize("value_type,zipf", [("i64", False), ("f64", True)], ids=["i64-uniform", "f64-zipf"])
def test_restatement_equals_oracle_under_event_time_trigger(cfg, value_type, zipf):
    # everything of the restatement but the trigger: assigners, merging in HashSet order, lateness, side output,
    # purging, the evictors, the timers' bookkeeping
    session = cfg["assigner"] == "session"
    ref = ContinuousRef(trigger="event_time", value_type=value_type, **cfg)
    okw = {k: v for k, v in cfg.items() if k != "assigner"}
    oracle = orc.ListWindowOracle(assigner=cfg["assigner"], trigger="event_time", value_type=value_type, **okw)
    gen = _zipf_stream if zipf else _stream
    k, t, v = gen(23 + len(str(cfg)), 6000, 300 if zipf else 400, 6000, 150) if session else \
        gen(7 + len(str(cfg)), 6000, 37, 600, 150)
    if value_type == "f64":
        v = (v.astype(np.float64) * 0.37).view(np.int64)
    wm = -10**9
    for b in range(10):
        sl = slice(b * 600, (b + 1) * 600)
        for h in (ref, oracle):
            h.process(k[sl], t[sl], v[sl])
        wm = max(wm, int(t[sl].max()) - 100)
        if b % 3 != 1:
            for h in (ref, oracle):
                h.watermark(wm)
        if not session:
            assert ref.num_state_entries == oracle.num_state_entries
            assert ref.num_timers == oracle.num_timers
    for w in (wm + 500, (1 << 63) - 1):
        for h in (ref, oracle):
            h.watermark(w)
    a, b = _firings(ref), _firings(oracle)
    assert sum(a.values()) == sum(b.values()) > 0
    assert a == b, (list((a - b).items())[:2], list((b - a).items())[:2])
    assert ref.late_dropped == oracle.late_dropped
    if cfg.get("side_output"):
        assert sorted(zip(*[c.tolist() for c in ref.side_rows()])) == \
            sorted(zip(*[c.tolist() for c in oracle.side_rows()]))
    if session:
        assert ref.merges > 0


def test_seeded_windows_cover_every_firing_class():
    # over the GPU tests' non-merging configurations (tests/test_gpu_continuous_trigger.py) some windows never fire early, some fire early many
    # times, and some meet their maxTimestamp with a fire time and stop there
    zero = many = stuck = 0
    for cfg in NONMERGING_CONFIGS[:5]:
        ref = ContinuousRef(trigger="continuous", **cfg)
        k, t, v = seeded_stream(7 + len(str(cfg)), 20000, 37, 2000, 150)
        drive([ref], k, t, v)
        wins = {(int(r["key"]), (int(r["start"]), int(r["end"]))) for r in ref.rows()}
        zero += sum(1 for w in wins if ref.early_by_window.get(w, 0) == 0)
        many += sum(1 for w in wins if ref.early_by_window.get(w, 0) >= 3)
        stuck += len(ref.stuck_windows)
    assert zero > 0 and many > 0 and stuck > 0, (zero, many, stuck)


def test_hashset_order_is_by_bucket_then_insertion():
    wins = [(a, a + 11) for a in range(0, 200, 20)]
    got = hashset_order(wins)
    assert sorted(got) == sorted(wins) and got != wins  # (some pair of these is out of insertion order)


# ---------------------------------------------------------------- the C-ABI and the Python surface
def _list_create(**kw):
    c = N.FwListConfig()
    c.key_group_start = c.key_group_end = -1
    for k, v in kw.items():
        setattr(c, k, v)
    h = ctypes.c_void_p()
    rc = N.lib().fw_list_create(ctypes.byref(c), ctypes.byref(h))
    msg = N.lib().fw_list_last_error(h).decode() if h else ""
    N.lib().fw_list_destroy(h)
    return rc, msg


@pytest.mark.parametrize("interval", [0, -5])
@pytest.mark.parametrize("assigner", ["tumbling", "session"])
def test_list_create_rejects_non_positive_interval(interval, assigner):
    rc, msg = _list_create(assigner=N.FW_TUMBLING if assigner == "tumbling" else N.FW_SESSION, size=100,
                           trigger=N.FW_TRIGGER_CONTINUOUS_EVENT_TIME, trigger_interval=interval)
    assert rc == N.FW_ERR_ARG
    assert "ContinuousEventTimeTrigger interval must be > 0" in msg


def test_trigger_constant_and_config_layout(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in N.FwListConfig._fields_]
    assert fields[-1] == "trigger_interval" and fields[-2] == "max_batch"  # appended: no earlier offset moved
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flink_window.h"\nint main(void) {\n'
                   '  printf("%d\\n", FW_TRIGGER_CONTINUOUS_EVENT_TIME);\n'
                   '  printf("%zu\\n", sizeof(fw_list_config));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(fw_list_config, {f}));\n' for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == N.FW_TRIGGER_CONTINUOUS_EVENT_TIME == 2
    assert out[1] == ctypes.sizeof(N.FwListConfig)
    assert out[2:] == [getattr(N.FwListConfig, f).offset for f in fields]
    assert N.FwListConfig.trigger_interval.offset == N.FwListConfig.max_batch.offset + 8


def test_fire_times_from_heap():
    from flink_amd import heapstate as H
    fires = H.fire_times_from_heap([((0, 3000), "key1", 2000), ((3000, 6000), "key2", 4000)])
    assert fires == {("key1", (0, 3000)): 2000, ("key2", (3000, 6000)): 4000}
    timers = {("key1", (0, 3000), 2999), ("key1", (0, 3000), 2000)}
    lists, elems = H.list_state_from_heap([((0, 3000), "key1", [5, 6]), ((3000, 6000), "key3", [7])], timers,
                                          key_id=lambda k: int(k[3:]), value_of=int, fire_times=fires)
    assert [(r["trigger_count"], r["timer"], r["n_elems"]) for r in lists] == [(2000, 3, 2), (LMIN, 0, 1)]
    assert [e[1] for e in elems] == [5, 6, 7]


def test_trigger_is_exported_and_purgeable():
    import flink_amd
    from flink_amd import ContinuousEventTimeTrigger, PurgingTrigger, Time
    assert flink_amd.ContinuousEventTimeTrigger is ContinuousEventTimeTrigger
    assert ContinuousEventTimeTrigger.of(250).interval == 250
    assert ContinuousEventTimeTrigger.of(Time.seconds(2)).interval == 2000
    p = PurgingTrigger.of(ContinuousEventTimeTrigger.of(3))
    assert p.purging and p.nested.interval == 3
    with pytest.raises(ValueError):
        ContinuousEventTimeTrigger.of(0)

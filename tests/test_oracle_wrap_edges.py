"""Timestamps at both ends of the long range, on the CPU: the oracle against the independent restatement
tests/window_ref.py where Java's longs wrap, the vetting of every registry entry of tests/time_edges_util.WRAP_CASES
(the only streams tests/test_gpu_wrap_edges.py may send to a GPU), and the coverage conditions that keep those GPU
tests from passing vacuously (asserted on the oracle and the restatement alone).  Exact integers throughout.

Three things the reference does not compute are kept out of the class and pinned here: the sliding assigner's runaway
set (the oracle returns OR_ERR_RUNAWAY, window_ref raises Runaway), ContinuousEventTimeTrigger chains that walk from the
bottom of the range to the watermark (tests/continuous_ref.py raises TimerRunaway at its timer cap), and sessions under
allowed lateness at the top (a merged window's maxTimestamp + lateness wraps and the merge function throws).

Two coverage conditions of the issue cannot hold and are replaced by what the arithmetic gives (test_bottom_windows_
never_wrap): with 0 <= offset < slide no window of a timestamp in the bottom range wraps or starts near
Long.MAX_VALUE, so "at least 200 rows with end < start" and "at least 50 rows whose start lies near Long.MAX_VALUE"
are asserted for top streams only (a top stream's rows near the other end start near Long.MIN_VALUE).  What the bottom
holds instead: records with no window (ts - size wraps), ts - offset wrapping inside getWindowStartWithOffset,
watermarks and cleanup times next to Long.MIN_VALUE, and the runaway set next to them."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import time_edges_util as T
from tests import window_ref as W
from tests.continuous_ref import ContinuousRef, TimerRunaway

MIN, MAX = W.LONG_MIN, W.LONG_MAX
CFGS = T.WRAP_CONFIGS
TIME_CFGS = {k: c for k, c in CFGS.items() if c["assigner"] != "session"}


def _end_timestamps(cfg, span=6000):
    """every timestamp within `span` of either end that is in the class (Long.MIN_VALUE itself and the runaway set left out)"""
    out = list(range(MAX - span, MAX + 1)) + list(range(MIN + 1, MIN + span + 1))
    if cfg["assigner"] == "sliding":
        out = [t for t in out if not W.is_runaway(t, cfg["size"], cfg["slide"], cfg.get("offset", 0))]
    return out


def test_window_start_sweep_at_both_ends():
    # oracle_window_start == TimeWindow.getWindowStartWithOffset restated, wherever ts - offset or + size wraps
    L = orc.lib()
    n = 0
    for size, offsets in [(1000, (0, 1, 999, 808, 308)), (2500, (0, 808)), (500, (0, 308)), (700, (0, 1))]:
        for off in offsets:
            for base in (MAX - 1500, MIN + 1):
                for ts in range(base, base + 1500):
                    assert L.oracle_window_start(ts, off, size) == W.window_start(ts, off, size), (ts, off, size)
                    n += 1
    assert n >= 20_000
    # the facts the class is built on: 2^63 mod 1000 = 808 puts Long.MIN_VALUE on the grid of offset 808
    assert (1 << 63) % 1000 == 808 and W.window_start(MAX - 192, 808, 1000) == MAX - 999
    assert W.tumbling_windows(MAX - 192, 1000, 808) == [(MAX - 999, MIN)] and W.max_timestamp(MIN) == MAX
    # ts - offset + size past Long.MAX_VALUE: a negative remainder, the start lands above ts and wraps to the bottom
    assert W.window_start(MAX, 808, 1000) == MIN + 616


def _assigned(cfg, ts):
    ref = orc.WindowOperatorOracle(**cfg)
    ts = np.array(ts, dtype=np.int64)
    ref.process(np.arange(len(ts)), ts, np.ones(len(ts), dtype=np.int64))
    ref.watermark(MAX)
    out = [[] for _ in ts]
    for r in ref.rows():
        out[int(r["key"])].append((int(r["start"]), int(r["end"])))
    return out


def test_assigners_sweep_at_both_ends():
    # one record per key, no watermark before Long.MAX_VALUE: the oracle's windows == the restatement's, per record
    n = wrapped = none = 0
    for name, cfg in CFGS.items():
        if cfg.get("lateness"):
            continue
        ts = _end_timestamps(cfg, 2000 if cfg["assigner"] == "session" else 4 * cfg["size"])
        for t, g in zip(ts, _assigned(cfg, ts)):
            # (a window that ends at Long.MIN_VALUE + 1 has maxTimestamp Long.MIN_VALUE, the initial watermark: late)
            want = [w for w in W.windows_of(cfg, t) if not W.is_window_late(w[1], 0, MIN)]
            assert sorted(g) == sorted(set(want)), (cfg, t, g, want)
            wrapped += any(e < s for s, e in want)
            none += not want
            n += 1
    assert n >= 20_000 and wrapped >= 2_000 and none >= 2_000


def test_bottom_windows_never_wrap():
    # with 0 <= offset < slide: no window of a bottom timestamp has end < start or a start above 0 (the module docstring)
    for cfg in TIME_CFGS.values():
        for t in range(MIN + 1, MIN + 4 * cfg["size"] + 1):
            if cfg["assigner"] == "sliding" and W.is_runaway(t, cfg["size"], cfg["slide"], cfg.get("offset", 0)):
                continue
            assert all(s < e < 0 for s, e in W.windows_of(cfg, t)), (cfg, t)


@pytest.mark.parametrize("lateness", [0, 500, MAX])
@pytest.mark.parametrize("wm", [MIN + 2000, 0, MAX - 3000, MAX - 1000, MAX - 1])
def test_lateness_arithmetic_at_both_ends(lateness, wm):
    # cleanupTime (clamped to Long.MAX_VALUE when maxTimestamp + lateness wraps), isWindowLate, isElementLate with
    # ts + lateness wrapping, and the late-drop count: after one watermark, one record per key is kept in exactly its
    # windows that are not late, and dropped when it has none and is late itself
    for cfg in (CFGS["tumbling-o808"], CFGS["tumbling-o1"], CFGS["sliding-2500-o308"], CFGS["sliding-2500-o0"],
                CFGS["sliding-700-1000"]):
        cfg = dict(cfg, lateness=lateness)
        ts = _end_timestamps(cfg, 4000)[::3]
        ref = orc.WindowOperatorOracle(**cfg)
        ref.watermark(wm)
        ref.process(np.arange(len(ts)), np.array(ts, dtype=np.int64), np.ones(len(ts), dtype=np.int64))
        ref.watermark(MAX)
        got = sorted((int(r["key"]), int(r["start"])) for r in ref.rows())
        want, dropped = [], 0
        for i, t in enumerate(ts):
            live = [s for s, e in W.windows_of(cfg, t) if not W.is_window_late(e, lateness, wm)]
            want += [(i, s) for s in live]
            dropped += (not live) and W.is_element_late(t, lateness, wm)
        assert got == sorted(want) and ref.late_dropped == dropped, (cfg, wm)
    assert W.cleanup_time(MIN, 0) == MAX and W.cleanup_time(MAX - 10, 500) == MAX and W.cleanup_time(MIN + 5, 500) == MIN + 504
    assert W.is_element_late(MAX, 500, MIN + 499) and not W.is_element_late(MAX, 500, MIN + 498)


def test_runaway_set_is_refused_by_both():
    # sliding 2500 / 1000, offset 0: ts - Long.MIN_VALUE in [2500, 3307] -- ts - size does not wrap, the walk down does
    run = [d for d in range(1, 6000) if W.is_runaway(MIN + d, 2500, 1000)]
    assert run == list(range(2500, 3308))
    with pytest.raises(W.Runaway):
        W.sliding_windows(MIN + 2500, 2500, 1000)
    assert W.sliding_windows(MIN + 2499, 2500, 1000) == [] and len(W.sliding_windows(MIN + 3308, 2500, 1000)) == 3
    for mk in (lambda: orc.WindowOperatorOracle(assigner="sliding", size=2500, slide=1000),
               lambda: orc.ListWindowOracle(assigner="sliding", size=2500, slide=1000)):
        for d in (2500, 3307):
            ref = mk()
            with pytest.raises(orc.OracleError) as e:
                ref.process(np.array([1]), np.array([MIN + d], dtype=np.int64), np.array([1]))
            assert e.value.code == -4  # OR_ERR_RUNAWAY
        ref = mk()
        ref.process(np.array([1, 2]), np.array([MIN + 2499, MIN + 3308], dtype=np.int64), np.array([1, 1]))
        ref.watermark(MAX)
        assert sorted(int(s) for s in ref.rows()["start"]) == [MIN + 808 + j * 1000 for j in (1, 2, 3)]
    with pytest.raises(TimerRunaway):
        ContinuousRef(assigner="sliding", size=2500, slide=1000)._assign(MIN + 2500)


def test_sessions_under_lateness_at_the_top_throw_in_the_reference():
    # a merged session that ends within the lateness of Long.MAX_VALUE: maxTimestamp + allowedLateness wraps below
    # every watermark and the merge function throws; those streams are not in the registry
    ref = orc.WindowOperatorOracle(assigner="session", gap=300, lateness=200)
    ref.watermark(0)
    with pytest.raises(orc.OracleError) as e:
        ref.process(np.array([1, 1]), np.array([MAX - 500, MAX - 400], dtype=np.int64), np.array([1, 1]))
    assert e.value.code == -2  # OR_ERR_MERGE_LATE
    assert not any(n.startswith("session-late-side-top") for n in T.WRAP_CASES)


def _restated_rows(cfg, batches, wms):
    ref = ContinuousRef(**cfg)
    for (k, t, v), wm in zip(batches, wms):
        ref.process(k, t, v)
        ref.watermark(wm)
    return ref


@pytest.mark.parametrize("name", [n for n in T.WRAP_CASES if n.startswith("session")])
def test_sessions_with_several_records_per_key(name):
    # MergingWindowSet.addWindow restated incrementally (tests/continuous_ref.py _add_window: per key,
    # TimeWindow.mergeWindows over the kept windows and the new one, in arrival order) against the oracle, row for row
    cfg, batches, wms = T.wrap_case(name)
    ref = orc.WindowOperatorOracle(**cfg)
    for (k, t, v), wm in zip(batches, wms):
        ref.process(k, t, v)
        ref.watermark(wm)
    py = _restated_rows({k: v for k, v in cfg.items()}, batches, wms)
    f = ("epoch", "key", "start", "end", "count", "sum", "min", "max")
    a, b = ref.rows(), py.rows()
    assert sorted(zip(*(a[x].tolist() for x in f))) == sorted(zip(*(b[x].tolist() for x in f)))
    assert ref.late_dropped == py.late_dropped and len(ref.side_rows()) == len(py.side_rows()[0])
    if T.WRAP_CASES[name]["end"] == "top":
        # two equal wrapped windows do not intersect each other, yet share one state (the mapping is keyed by the
        # window): one row with count 2, where a merge of the batch's sorted windows would give two rows
        w = a[a["end"] < a["start"]]
        # (a warm stream opens wrapped sessions only before its first watermark: too few for an equal pair)
        assert T.WRAP_CASES[name]["schedule"] == T.WARM or (w["count"] >= 2).sum() >= 10
        keys = list(zip(w["epoch"].tolist(), w["key"].tolist(), w["start"].tolist()))
        assert len(set(keys)) == len(keys)


def test_equal_wrapped_sessions_share_one_state():
    ref = orc.WindowOperatorOracle(assigner="session", gap=300)
    t = MAX - 100
    assert not (t <= W.wrap64(t + 300) and W.wrap64(t + 300) >= t)  # TimeWindow.intersects with itself
    ref.process(np.array([7, 7, 7]), np.array([t, t, t - 250], dtype=np.int64), np.array([1, 2, 4]))
    ref.watermark(MAX)
    rows = sorted((int(r["start"]), int(r["end"]), int(r["count"]), int(r["sum"])) for r in ref.rows())
    assert rows == [(t - 250, t + 50, 1, 4), (t, MIN + 199, 2, 3)]  # ([t - 250, t + 50) ends above the other's start)


# ---- the registry: vetting and coverage
def _true_windows(cfg, t):
    """the windows of t on unbounded ints: grid points at or below t, nothing wraps"""
    off, size = cfg.get("offset", 0), T.extent(cfg)
    if cfg["assigner"] == "session":
        return [(t, t + size)]
    step = T.step(cfg)
    s = t - (t - off) % step
    out = []
    while s > t - size:
        out.append((s, s + size))
        s -= step
    return out


def _caused_by_wrap(cfg, t, wm):
    """the record (arriving under watermark wm) is dropped as late -- none of its windows is kept and it is late
    itself -- although on unbounded ints one of its windows would not be late: the drop comes from a long that wrapped
    (a window's end past Long.MAX_VALUE, or ts - offset + size, which leaves a start above ts or no window at all)"""
    lat = cfg.get("lateness", 0)
    if any(not W.is_window_late(e, lat, wm) for _, e in W.windows_of(cfg, t)) or not W.is_element_late(t, lat, wm):
        return False
    return any(e - 1 + lat > wm for _, e in _true_windows(cfg, t))


@pytest.mark.parametrize("name", list(T.WRAP_CASES))
def test_registry_entry_is_in_the_class_and_covers_it(name):
    case = T.WRAP_CASES[name]
    cfg, batches, wms = T.wrap_case(name)
    end, warm, top = case["end"], case["schedule"] == T.WARM, case["end"] == "top"
    n = sum(len(b[0]) for b in batches)
    ext = T.extent(cfg)
    assert 4000 <= n <= 8000 and 4 <= len(batches) <= 6 and wms[-1] == MAX
    near = case["schedule"] == T.NEAR
    assert wms == (T.warm_watermarks(cfg) if warm else [MAX - ext - ext // 2] * 4 + [MAX - 1, MAX] if near else [MIN] * 5 + [MAX])
    all_ts = [t for _, ts, _ in batches for t in ts.tolist()]
    lo, hi = (MAX - 4 * ext, MAX) if top else (MIN + 1, MIN + 4 * ext)
    assert all(lo <= t <= hi for t in all_ts) and MIN not in all_ts
    assert ({MAX, MAX - 1} <= set(all_ts)) if top else (MIN + 1 in all_ts)
    # 1. nothing of the runaway set
    if cfg["assigner"] == "sliding":
        assert not any(W.is_runaway(t, cfg["size"], cfg["slide"], cfg.get("offset", 0)) for t in set(all_ts))
    # 2. the reference completes under its cap
    most = W.sliding_cap(cfg["size"], cfg["slide"]) if cfg["assigner"] == "sliding" else 2
    row_cap = 8 * n * most
    if "interval" in case:
        ref = ContinuousRef(trigger="continuous", interval=case["interval"], timer_cap=row_cap, **cfg)
    else:
        ref = orc.WindowOperatorOracle(**cfg)
    cur, by_wrap = MIN, 0
    for (k, t, v), wm in zip(batches, wms):
        ref.process(k, t, v)
        if warm and "interval" not in case:
            by_wrap += sum(_caused_by_wrap(cfg, x, cur) for x in t.tolist())
        ref.watermark(wm)
        cur = max(cur, wm)
    rows = ref.rows()
    # 3. the fired rows are bounded
    assert 0 < len(rows) <= row_cap
    c = T.wrap_row_classes(rows, end)
    # ---- coverage
    recs = [W.windows_of(cfg, t) for t in all_ts]
    wrapped = sum(any(e < s for s, e in ws) for ws in recs) / n
    none = sum(not ws for ws in recs) / n
    if top:
        assert c["wrapped"] >= 200, c
        if cfg["assigner"] == "sliding" and cfg["size"] == 2500:
            assert wrapped >= 0.30 and none >= 0.03, (wrapped, none)
        if cfg["assigner"] == "tumbling" and cfg.get("offset") == 808:
            assert wrapped >= 0.15, wrapped
        # (700 / 1000: above MAX - 1000 the start lands above ts and the walk gives the record a second window one slide
        # below, which is late only when the record truly is; no drop there comes from a wrap)
        if warm and "interval" not in case and name != "sliding-700-1000-top-warm":
            side = len(ref.side_rows())
            assert by_wrap >= 100 and ref.late_dropped + side >= by_wrap, (by_wrap, ref.late_dropped, side)
    else:
        assert c["wrapped"] == 0 and c["far"] == 0  # (test_bottom_windows_never_wrap)
        if cfg["assigner"] == "sliding":
            assert none >= 0.10, none  # ts - size wraps: no window
        if warm:
            side = ref.side_rows()
            assert (rows["epoch"] < len(wms) - 1).any()
            assert ref.late_dropped + len(side[0] if "interval" in case else side) >= 1000
    # a window that ends at Long.MIN_VALUE (maxTimestamp Long.MAX_VALUE) fires by the last watermark and by no earlier
    # one, in every configuration that has one: the grid of offset 808 (size 1000) / 308 (2500 / 1000), and sessions
    has_min_end = top and (cfg["assigner"] == "session" or
                           any(e == MIN for t in range(MAX - ext, MAX + 1) for _, e in W.windows_of(cfg, t)))
    if has_min_end:
        last = rows[rows["end"] == MIN]
        assert len(last) >= 1 and (last["epoch"] == len(wms) - 1).all()
        if cfg.get("lateness", 0) == 0:
            assert c["end_min"] == len(last)
    else:
        assert c["end_min"] == 0


def test_continuous_chain_from_the_bottom_of_the_range_is_excluded():
    # offset 808's window [MAX - 999, Long.MIN_VALUE) has its cleanup timer at Long.MAX_VALUE: a first timer that wraps
    # starts a chain that walks up the whole range; the restatement stops at its cap instead of not returning
    cfg = dict(assigner="tumbling", size=1000, offset=808)
    batches, wms = T.wrap_stream(cfg, "top", T.COLD, n=4000, num_keys=32)
    ref = ContinuousRef(trigger="continuous", interval=33, timer_cap=64 * 4000, **cfg)
    with pytest.raises(TimerRunaway):
        for (k, t, v), wm in zip(batches, wms):
            ref.process(k, t, v)
            ref.watermark(wm)
    assert W.continuous_next_fire(MAX - 5, 33) < MIN + 40

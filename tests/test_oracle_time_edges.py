"""The event-time arithmetic on the CPU: the oracle against the independent restatement tests/window_ref.py on
pre-epoch timestamps and odd window sizes, and the coverage conditions that keep tests/test_gpu_time_edges.py from
passing vacuously (asserted on the oracle and the restatement alone).  Exact integers throughout."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import time_edges_util as T
from tests import window_ref as W
from tests.continuous_ref import jrem, jwrap

H8, H24 = T.H8, T.H24


def _mix(x):
    x = (x + 0x9E3779B97F4A7C15) & ((1 << 64) - 1)
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & ((1 << 64) - 1)
    return x ^ (x >> 31)


def _offsets(step):
    return [0, step - 1, -(step - 1), -H8 if step == H24 else step // 2]


def _timestamps(step, offset, extent, count, seed):
    """every boundary offset + j step + {-1, 0, 1} for j in -3 .. 3, then `count` seeded timestamps over
    [-60 extent, 20 extent], inside the range that does not wrap"""
    room = W.LONG_MAX - 2 * extent - step - abs(offset) - 2
    out = [offset + j * step + e for j in range(-3, 4) for e in (-1, 0, 1)]
    lo, hi = max(-60 * extent, -room), min(20 * extent, room)
    out += [lo + _mix(seed * 1_000_003 + i) % (hi - lo + 1) for i in range(count)]
    return [t for t in out if -room <= t <= room]


SIZES = [1000, H24] + T.ODD_SIZES


def test_window_start_sweep():
    # oracle_window_start == TimeWindow.getWindowStartWithOffset restated, on > 10^5 (ts, offset, size) triples
    L = orc.lib()
    n = 0
    for size in SIZES:
        for off in _offsets(size):
            for ts in _timestamps(size, off, size, 2000, size):
                want = W.window_start(ts, off, size)
                assert L.oracle_window_start(ts, off, size) == want, (ts, off, size)
                # (the start the reference computes: on the grid, within a size of ts, above ts exactly when displaced)
                assert (want - off) % size == 0 and abs(want - ts) < size
                assert (want > ts) == W.is_displaced(ts, off, size)
                n += 1
    assert n >= 100_000


def test_time_window_test_vectors_in_the_restatement():
    # TimeWindowTest.testGetWindowStartWithOffset (flink-streaming-java/src/test/java/.../windows/TimeWindowTest.java)
    assert [W.window_start(t, 0, 7) for t in (1, 6, 7, 8)] == [0, 0, 7, 7]
    assert [W.window_start(t, 3, 7) for t in (1, 2, 3, 9, 10)] == [-4, -4, 3, 3, 10]
    assert [W.window_start(t, -2, 7) for t in (1, -2, 3, 4, 7, 12)] == [-2, -2, -2, -2, 5, 12]
    assert W.window_start(1470902048450, -H8, H24) == 1470844800000
    assert W.window_start(1, -H8, H24) == -H8 and W.window_start(-H8 - 1, -H8, H24) == -H8 - H24
    # the issue's hand-worked table: size 3000, slide 1000
    assert [s for s, _ in W.sliding_windows(1500, 3000, 1000)] == [1000, 0, -1000]
    assert [s for s, _ in W.sliding_windows(-1000, 3000, 1000)] == [-1000, -2000, -3000]
    assert [s for s, _ in W.sliding_windows(-1500, 3000, 1000)] == [-1000, -2000, -3000, -4000]
    assert len(W.sliding_windows(-1600, 2500, 1000)) == 4


def _assigned(cfg, ts):
    """the windows the oracle's operator assigns to each timestamp: one record per key, everything fired at the end"""
    ref = orc.WindowOperatorOracle(**cfg)
    ts = np.array(ts, dtype=np.int64)
    ref.process(np.arange(len(ts)), ts, np.ones(len(ts), dtype=np.int64))
    ref.watermark(W.LONG_MAX)
    rows = ref.rows()
    out = [[] for _ in ts]
    for r in rows:
        out[int(r["key"])].append((int(r["start"]), int(r["end"])))
    return out


ASSIGNER_CFGS = ([dict(assigner="tumbling", size=s, offset=o) for s in SIZES for o in _offsets(s)]
                 + [dict(assigner="sliding", size=s, slide=sl, offset=o)
                    for s, sl in [(2500, 1000), (3000, 1000), (2000, 500), (1000, 1000), (700, 1000), (7, 3),
                                  (1_000_003, (1 << 17) - 1), (3 * ((1 << 20) + 1), (1 << 20) + 1),
                                  ((1 << 61) + 1, (1 << 60) + 3), (H24, H8)]
                    for o in _offsets(sl)]
                 + [dict(assigner="session", gap=g) for g in (1, 300, (1 << 40) + 15)])


def test_assigners_sweep():
    # the oracle's tumbling / sliding / session assignWindows == the restatement's, per record
    n = extra = 0
    for cfg in ASSIGNER_CFGS:
        step, extent = T._step(cfg), T._extent(cfg)
        ts = _timestamps(step, cfg.get("offset", 0), extent, 1200, extent + step)
        got = _assigned(cfg, ts)
        for t, g in zip(ts, got):
            want = W.windows_of(cfg, t)
            assert sorted(g) == sorted(want), (cfg, t, g, want)
            if cfg["assigner"] == "sliding":
                most = -(-cfg["size"] // cfg["slide"])
                assert len(want) <= most + 1
                # the extra window is the displaced records', and every one of them has it when slide <= size
                assert (len(want) == most + 1) <= W.is_displaced(t, cfg.get("offset", 0), step)
                extra += len(want) == most + 1
            n += 1
    assert n >= 100_000 and extra >= 10_000


def test_sessions_merge_across_zero():
    # EventTimeSessionWindows + TimeWindow.mergeWindows: per key, the oracle's sessions == the restatement's covers
    cfg = T.PRE_SESSIONS[0]
    batches, _ = T.pre_epoch_stream(cfg, n=20_000, num_keys=64)
    ref = orc.WindowOperatorOracle(**cfg)
    wins = {}
    for k, t, v in batches:
        ref.process(k, t, v)
        for key, ts in zip(k.tolist(), t.tolist()):
            wins.setdefault(key, []).extend(W.session_window(ts, cfg["gap"]))
    ref.watermark(W.LONG_MAX)
    want = sorted((key, s, e) for key, w in wins.items() for s, e in W.merge_sessions(w))
    rows = ref.rows()
    assert sorted((int(r["key"]), int(r["start"]), int(r["end"])) for r in rows) == want
    assert any(s < 0 < e for _, s, e in want)


@pytest.mark.parametrize("lateness", [0, 300, W.LONG_MAX])
def test_lateness_arithmetic(lateness):
    # maxTimestamp, cleanupTime (its overflow to Long.MAX_VALUE included), isWindowLate, isElementLate: after a
    # watermark, one record per key is kept in exactly its windows that are not late and dropped when it has none
    for cfg, wm in [(dict(assigner="tumbling", size=1000, offset=-999), -4200),
                    (dict(assigner="sliding", size=2500, slide=1000), -3700),
                    (dict(assigner="sliding", size=2500, slide=1000, offset=999), 1)]:
        cfg = dict(cfg, lateness=lateness)
        ts = list(range(wm - 6000, wm + 3000, 7))
        ref = orc.WindowOperatorOracle(**cfg)
        ref.watermark(wm)
        ref.process(np.arange(len(ts)), np.array(ts), np.ones(len(ts), dtype=np.int64))
        ref.watermark(W.LONG_MAX)
        got = sorted((int(r["key"]), int(r["start"])) for r in ref.rows())
        want, dropped = [], 0
        for i, t in enumerate(ts):
            live = [s for s, e in W.windows_of(cfg, t) if not W.is_window_late(e, lateness, wm)]
            want += [(i, s) for s in live]
            dropped += (not live) and W.is_element_late(t, lateness, wm)
        assert got == sorted(want) and ref.late_dropped == dropped
        assert lateness or dropped > 100
    assert W.cleanup_time(W.LONG_MAX, 5) == W.LONG_MAX and W.cleanup_time(10, 5) == 14 and W.max_timestamp(0) == -1


def test_continuous_next_fire_restated_twice():
    # ContinuousEventTimeTrigger's first timer: tests/continuous_ref.py (the list operator's reference) and
    # window_ref agree, and a pre-epoch timestamp off the interval's grid gets the grid point above it + interval
    for interval in (1, 11, 33, 250, (1 << 32) + 1):
        for i in range(3000):
            ts = _mix(i * 31 + interval) % (80 * interval) - 60 * interval
            assert W.continuous_next_fire(ts, interval) == jwrap(jwrap(ts - jrem(ts, interval)) + interval)
    assert W.continuous_next_fire(-5, 11) == 11 and W.continuous_next_fire(-11, 11) == 0 and W.continuous_next_fire(5, 11) == 11


# ---- coverage: what the GPU tests' streams hold, by the oracle and the restatement alone
def _fired(cfg, batches, wms):
    ref = orc.WindowOperatorOracle(**cfg)
    for (k, t, v), wm in zip(batches, wms):
        ref.process(k, t, v)
        ref.watermark(wm)
    return ref.rows()


@pytest.mark.parametrize("cfg", T.PRE_ALL, ids=[str(i) for i in range(len(T.PRE_ALL))])
def test_pre_epoch_streams_cover_their_class(cfg):
    batches, wms = T.pre_epoch_stream(cfg)
    T.assert_no_wrap(cfg, batches)
    assert 20_000 <= sum(len(b[0]) for b in batches) <= 60_000 and 4 <= len(batches) - 1 <= 8
    c = T.coverage(cfg, batches)
    assert c["displaced"] >= 0.30 and c["negative"] >= 0.10 and c["nonneg"] >= 0.20, c
    if cfg["assigner"] == "sliding":
        assert c["extra"] >= 0.20, c
    assert sum(w < 0 for w in wms) >= 2 and any(0 <= w < W.LONG_MAX for w in wms) and wms[-1] == W.LONG_MAX
    rows = _fired(cfg, batches, wms)
    if cfg["assigner"] == "tumbling" and cfg.get("offset", 0) % cfg["size"] == 0:
        # (0 is on a tumbling grid: no window has start < 0 < end; the two windows that meet at 0 fire)
        assert (rows["end"] == 0).any() and (rows["start"] == 0).any()
    else:
        assert ((rows["start"] < 0) & (rows["end"] > 0)).any()
    assert len(np.unique(rows["start"][rows["start"] < 0])) >= 50
    assert T.row_classes(cfg, rows, batches)["from_displaced"] >= 1000


@pytest.mark.parametrize("cfg", T.PRE_SESSIONS, ids=["plain", "lateness"])
def test_pre_epoch_sessions_cover_their_class(cfg):
    batches, wms = T.pre_epoch_stream(cfg, num_keys=300)
    rows = _fired(cfg, batches, wms)
    assert ((rows["start"] < 0) & (rows["end"] > 0)).sum() >= 5  # sessions that merged across 0
    assert (rows["count"] > 1).sum() >= 1000 and (rows["start"] < 0).sum() >= 1000


ODD_ALL = T.ODD_TUMBLING + [T.ODD_PANE_PAIR] + T.ODD_NONPANE_PAIRS


@pytest.mark.parametrize("cfg", ODD_ALL, ids=[f"{c['assigner']}-{c['size']}" for c in ODD_ALL])
def test_odd_size_streams_cover_their_class(cfg):
    batches, wms = T.odd_stream(cfg, floor=T.odd_floor(cfg))
    T.assert_no_wrap(cfg, batches)
    rows = _fired(cfg, batches, wms)
    starts = np.unique(rows["start"])
    huge = cfg["size"] == (1 << 62) + 1
    assert len(starts) >= (2 if huge else 3), starts
    assert (starts < 0).any() and (starts >= 0).any()
    if cfg == T.ODD_PANE_PAIR:  # nothing a pane operator would refuse
        assert T.coverage(cfg, batches)["displaced"] == 0
    # the reciprocal's shift for the two largest sizes (flink_amd/csrc/fw_internal.h make_div_inv: l = ceil(log2 d))
    assert (1 << 61).bit_length() == 62 and (1 << 62).bit_length() == 63  # ((d - 1).bit_length() = ceil(log2 d))

"""tests/over_ref.py against the reference's own OVER window tests (tests/golden/over_kats.json) and the edge
semantics of the four ProcessFunctions that no reference test pins.  No GPU."""
import pytest

from tests.over_ref import LMAX, LMIN, OverRef
from tests.over_util import check_kat, load_kats, replay_kat

KATS = load_kats()


class _Ref:
    def __init__(self, case):
        self.r = OverRef(case["kind"], case["preceding"], case["column_types"], case["aggregates"])

    def process(self, keys, rowtimes, columns, nulls):
        self.r.process(keys, rowtimes, columns, nulls)

    def watermark(self, wm):
        return self.r.watermark(wm)


def test_fixture_is_complete():
    names = {c["name"] for c in KATS}
    assert len(KATS) == 9 and len(names) == 9
    assert {c["kind"] for c in KATS if c["name"].startswith("harness")} == {
        "bounded_rows", "bounded_range", "unbounded_rows", "unbounded_range"}
    for c in KATS:
        assert ":" in c["source"] and c["expected"]


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_reference_kats(case):
    check_kat(case, replay_kat(case, _Ref(case)))


def _one(kind, preceding=1000):
    return OverRef(kind, preceding, ["long"], [("count_star", 0), ("sum", 0)])


@pytest.mark.parametrize("kind", ["bounded_rows", "bounded_range"])
def test_fresh_bounded_key_drops_row_times_up_to_zero(kind):
    # lastTriggeringTsState.value of an unset ValueState[Long] is 0L (RowTimeBoundedRangeOver.scala:122)
    r = _one(kind)
    r.process([7, 7, 7, 8], [-5, 0, 1, 0], [[1, 2, 3, 4]])
    assert r.stats()["late_rows_dropped"] == 3 and r.stats()["rows_kept"] == 1
    assert r.watermark(10) == [(7, 1, 2, [1, 3])]


@pytest.mark.parametrize("kind", ["bounded_rows", "bounded_range"])
def test_bounded_key_drops_its_last_fired_row_time(kind):
    r = _one(kind)
    r.process([7], [100], [[1]])
    assert len(r.watermark(500)) == 1
    r.process([7, 7], [100, 101], [[2, 3]])          # == lastTriggeringTs: dropped; + 1: kept
    assert r.stats()["late_rows_dropped"] == 1
    assert r.watermark(600) == [(7, 101, 2, [2, 4])]


@pytest.mark.parametrize("kind", ["bounded_rows", "bounded_range"])
def test_bounded_key_keeps_a_row_behind_the_watermark(kind):
    # the test is against the key's lastTriggeringTs, not the watermark: the row fires at the next watermark call
    r = _one(kind)
    r.process([7], [100], [[1]])
    assert len(r.watermark(500)) == 1
    r.process([7], [300], [[5]])                      # 100 < 300 <= 500
    assert r.stats()["late_rows_dropped"] == 0 and r.stats()["pending_rows"] == 1
    assert r.watermark(500) == [(7, 300, 1, [2, 6])]


@pytest.mark.parametrize("kind", ["unbounded_rows", "unbounded_range"])
def test_unbounded_drops_at_the_watermark(kind):
    r = _one(kind)
    assert r.watermark(500) == []
    r.process([7, 7], [500, 501], [[1, 2]])
    assert r.stats()["late_rows_dropped"] == 1
    assert r.watermark(LMAX) == [(7, 501, 1, [1, 2])]


@pytest.mark.parametrize("kind", ["unbounded_rows", "unbounded_range"])
def test_unbounded_accepts_negative_row_times_at_first(kind):
    r = _one(kind)                                   # a fresh handle's watermark is Long.MIN_VALUE
    r.process([7, 7], [-10, LMIN + 1], [[1, 2]])
    assert r.stats()["late_rows_dropped"] == 0
    assert r.watermark(0) == [(7, LMIN + 1, 1, [1, 2]), (7, -10, 0, [2, 3])]


def test_nulls_and_width_wrap():
    r = OverRef("bounded_rows", 1, ["int", "long"], [("sum", 0), ("avg", 0), ("min", 1), ("count", 1), ("avg", 1)])
    big = (1 << 31) - 1
    r.process([1, 1, 1], [1, 2, 3], [[big, big, 5], [0, 0, LMAX]], nulls=[2, 2, 0])
    got = r.watermark(10)
    assert got[0][3] == [big, big, None, 0, None]
    assert got[1][3] == [-2, big, None, 0, None]      # Int SUM wraps; the Integral AVG divides a Long sum
    assert got[2][3] == [-(1 << 31) + 4, ((big + 5) // 2), LMAX, 1, LMAX]


@pytest.mark.parametrize("kind,preceding", [("bounded_rows", 0), ("bounded_rows", 7), ("bounded_range", 0),
                                            ("bounded_range", 13), ("unbounded_rows", 0), ("unbounded_range", 0)])
def test_direct_frame_evaluation_agrees(kind, preceding):
    # tests/over_util.brute_frames (the GPU boundary tests' reference for long runs) against the restatement
    import numpy as np
    from tests.over_util import assert_same_rows, brute_frames
    rng = np.random.default_rng(5)
    n = 600
    keys = rng.integers(1, 6, size=n, dtype=np.int64)
    ts = rng.integers(1, 120, size=n, dtype=np.int64)
    cols = [rng.integers(-(1 << 62), 1 << 62, size=n, dtype=np.int64), rng.integers(-50, 50, size=n, dtype=np.int64)]
    nulls = (rng.random(n) < 0.3).astype(np.uint8) * 2
    aggs = [("count_star", 0), ("count", 1), ("sum", 0), ("avg", 0), ("min", 1), ("max", 1), ("sum", 1)]
    r = OverRef(kind, preceding, ["long", "long"], aggs)
    r.process(keys, ts, cols, nulls)
    assert_same_rows(brute_frames(kind, preceding, keys, ts, cols, nulls, aggs), r.watermark(LMAX), 0.0)


@pytest.mark.parametrize("kind", ["bounded_rows", "bounded_range", "unbounded_rows", "unbounded_range"])
@pytest.mark.parametrize("zipf", [0.0, 1.1])
def test_seeded_streams_are_not_vacuous(kind, zipf):
    # the GPU parity test's streams, on the reference's output alone: >= 60 % of the rows emitted, >= 1 % late
    from tests.over_util import AGGS16, TYPES5, run_steps, seeded_stream
    steps = seeded_stream(11, nkeys=500 if zipf else 97, zipf=zipf)
    r = OverRef(kind, {"bounded_rows": 5, "bounded_range": 50}.get(kind, 0), TYPES5, AGGS16)
    emitted = sum(len(w) for w in run_steps(_Wrap(r), steps))
    pushed = sum(len(s[1]) for s in steps if s[0] == "p")
    assert emitted >= 0.6 * pushed and r.stats()["late_rows_dropped"] >= 0.01 * pushed, (emitted, r.stats(), pushed)
    assert emitted + r.stats()["late_rows_dropped"] == pushed


class _Wrap:
    def __init__(self, r):
        self.r = r

    def process(self, keys, rowtimes, columns, nulls):
        self.r.process(keys, rowtimes, columns, nulls)

    def watermark(self, wm):
        return self.r.watermark(wm)

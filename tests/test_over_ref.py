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


# ---------------------------------------------------------------- Double specials, zero signs (answers by hand from the Scala)
import struct  # noqa: E402

NAN, INF, DBL_MAX = float("nan"), float("inf"), 1.7976931348623157e308
ALL_KINDS = ["bounded_rows", "bounded_range", "unbounded_rows", "unbounded_range"]


def _b(v):
    """a result as comparable bits: None, or the 64 bits with every NaN the canonical one"""
    if v is None:
        return None
    return "nan" if v != v else struct.unpack("<q", struct.pack("<d", v))[0]


PZ, NZ = _b(0.0), _b(-0.0)


def _doubles(kind, preceding, values, fns=("sum", "min", "max", "avg"), wms=None):
    """one key, row times 1, 2, ..; per function the emitted results as bits, over all watermarks"""
    r = OverRef(kind, preceding, ["double"], [(f, 0) for f in fns])
    n = len(values)
    r.process([1] * n, list(range(1, n + 1)), [[0.0 if v is None else v for v in values]],
              [1 if v is None else 0 for v in values])
    rows = [row for wm in (wms or [LMAX]) for row in r.watermark(wm)]
    assert [row[1] for row in rows] == list(range(1, n + 1))
    return {f: [_b(row[3][q]) for row in rows] for q, f in enumerate(fns)}


def test_double_compare_order():
    from tests.over_ref import _compare, double_bits
    assert PZ == 0 and NZ == -(1 << 63) and double_bits(-NAN) == double_bits(NAN) == 0x7FF8000000000000
    order = [-INF, -1.5, -0.0, 0.0, 1.5, DBL_MAX, INF, NAN]
    for i, a in enumerate(order):
        for j, b in enumerate(order):
            assert _compare(a, b) == (i > j) - (i < j), (a, b)
    assert _compare(3, 3) == 0 and _compare(-2, 5) == -1


def test_bounded_max_keeps_a_stale_nan_after_its_retraction():
    # MaxAggFunctionWithRetract.scala:84: `v == acc.f0` is false for NaN, so the map is not rescanned when the NaN
    # leaves: ROWS 1 PRECEDING over NaN, 1, 2, 3 -- the frames {1, 2} and {2, 3} hold no NaN and still give NaN
    for wms in (None, [3, LMAX], [1, 2, 3, 4]):
        got = _doubles("bounded_rows", 1, [NAN, 1.0, 2.0, 3.0], wms=wms)
        assert got["max"] == ["nan"] * 4
        assert got["min"] == ["nan", _b(1.0), _b(1.0), _b(2.0)]      # MIN: NaN is the greatest value, never stale
        assert got["sum"] == ["nan"] * 4 and got["avg"] == ["nan"] * 4
    # ... until the map empties (:78-80 resets f0): frames {NaN}, {NaN, 1}, {1, NULL}, {NULL, NULL}, {NULL, 5}
    got = _doubles("bounded_rows", 1, [NAN, 1.0, None, None, 5.0], fns=("max", "min"))
    assert got["max"] == ["nan", "nan", "nan", None, _b(5.0)]
    assert got["min"] == ["nan", _b(1.0), _b(1.0), None, _b(5.0)]
    # RANGE 1 ms PRECEDING, row times 1 .. 4: the same frames
    got = _doubles("bounded_range", 1, [NAN, 1.0, 2.0, 3.0])
    assert got["max"] == ["nan"] * 4 and got["min"] == ["nan", _b(1.0), _b(1.0), _b(2.0)]


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_min_ignores_nan_and_max_takes_it(kind):
    # a frame that grows only (ROWS / RANGE 10 over 3 rows, or unbounded): compare(NaN, x) > 0 for every x
    neg_nan = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]     # Inf - Inf on x86: the sign bit set
    for nan in (NAN, neg_nan):
        got = _doubles(kind, 10, [nan, -INF, 1.0], fns=("min", "max"))
        assert got["min"] == ["nan", _b(-INF), _b(-INF)] and got["max"] == ["nan"] * 3
        got = _doubles(kind, 10, [1.0, nan, INF], fns=("min", "max"))
        assert got["min"] == [_b(1.0)] * 3 and got["max"] == [_b(1.0), "nan", "nan"]


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_zero_signs_in_min_and_max_in_both_arrival_orders(kind):
    # Double.compare(-0.0, 0.0) < 0: MIN takes -0.0, MAX takes +0.0, whichever came first
    got = _doubles(kind, 10, [0.0, -0.0], fns=("min", "max"))
    assert got["min"] == [PZ, NZ] and got["max"] == [PZ, PZ]
    got = _doubles(kind, 10, [-0.0, 0.0], fns=("min", "max"))
    assert got["min"] == [NZ, NZ] and got["max"] == [NZ, PZ]


def test_retracting_a_zero_rescans_by_numeric_equality():
    # ROWS 1 PRECEDING over -0.0, 0.0, 0.0: the third row retracts -0.0; -0.0 == f0 (numeric), the map {0.0} is
    # rescanned.  Over 0.0, -0.0, -0.0 the MAX 0.0 leaves the same way.
    assert _doubles("bounded_rows", 1, [-0.0, 0.0, 0.0], fns=("min", "max")) == {"min": [NZ, NZ, PZ], "max": [NZ, PZ, PZ]}
    assert _doubles("bounded_rows", 1, [0.0, -0.0, -0.0], fns=("min", "max")) == {"min": [PZ, NZ, NZ], "max": [PZ, PZ, NZ]}


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_sum_of_negative_zeros_is_positive_zero(kind):
    # numeric.zero is +0.0 and 0.0 + -0.0 = +0.0 (SumWithRetractAggFunction.scala:43-52, SumAggFunction.scala:39-50)
    got = _doubles(kind, 1, [-0.0, -0.0, None, -0.0], fns=("sum", "avg", "min"))
    assert got["sum"] == [PZ] * 4 and got["avg"] == [PZ] * 4 and got["min"] == [NZ] * 4


def test_a_retracted_infinity_leaves_a_sticky_nan():
    # ROWS 1 PRECEDING over Inf, 1, 2, 3: Inf, Inf + 1, then (Inf - Inf) + 2 = NaN, and NaN from there on
    for wms in (None, [2, LMAX], [3, LMAX]):
        got = _doubles("bounded_rows", 1, [INF, 1.0, 2.0, 3.0, 4.0], wms=wms)
        assert got["sum"] == [_b(INF), _b(INF), "nan", "nan", "nan"]
        assert got["max"] == [_b(INF), _b(INF), _b(2.0), _b(3.0), _b(4.0)]
    got = _doubles("bounded_range", 0, [INF, 1.0, 2.0])     # RANGE 0: each row alone
    assert got["sum"] == [_b(INF), "nan", "nan"]
    got = _doubles("bounded_rows", 1, [INF, -INF, 2.0], fns=("sum",))   # Inf + -Inf
    assert got["sum"] == [_b(INF), "nan", "nan"]
    got = _doubles("bounded_rows", 1, [-INF, 1.0, 2.0], fns=("sum",))
    assert got["sum"] == [_b(-INF), _b(-INF), "nan"]
    for kind in ("unbounded_rows", "unbounded_range"):      # nothing is retracted
        assert _doubles(kind, 0, [INF, 1.0, 2.0], fns=("sum",))["sum"] == [_b(INF)] * 3


def test_an_overflowed_sum_is_a_sticky_infinity():
    # ROWS 1 PRECEDING over MAX, MAX, 1, 2: MAX, MAX + MAX = Inf, (Inf - MAX) + 1 = Inf, and Inf from there on
    for wms in (None, [2, LMAX], [3, LMAX]):
        got = _doubles("bounded_rows", 1, [DBL_MAX, DBL_MAX, 1.0, 2.0, 3.0], wms=wms)
        assert got["sum"] == [_b(DBL_MAX), _b(INF), _b(INF), _b(INF), _b(INF)]
        assert got["avg"] == [_b(DBL_MAX), _b(INF), _b(INF), _b(INF), _b(INF)]
        assert got["max"] == [_b(DBL_MAX), _b(DBL_MAX), _b(DBL_MAX), _b(2.0), _b(3.0)]
    got = _doubles("bounded_rows", 1, [DBL_MAX, DBL_MAX, 1.0, -INF, 3.0], fns=("sum",))
    assert got["sum"] == [_b(DBL_MAX), _b(INF), _b(INF), "nan", "nan"]

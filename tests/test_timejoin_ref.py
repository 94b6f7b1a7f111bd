"""The time-windowed join's restatement against the reference's own harness sequences (tests/golden/
timejoin_kats.json), hand-derived edge cases, and the non-vacuity of the seeded streams the GPU parity test uses."""
import numpy as np
import pytest

from .timejoin_ref import LMAX, LMIN, TimeBoundedJoinRef
from .timejoin_util import (BOUNDS, JOIN_TYPES, PER_PUSH, PUSHES, RefEngine, brute_force_pairs, load_kats, make_stream,
                            ref_run, replay_kat, segments, single_key_rows)

KATS = load_kats()


def test_fixture_is_complete():
    assert len(KATS) == 5
    assert sorted({c["join_type"] for c in KATS}) == ["full", "inner", "left", "right"]
    for c in KATS:
        assert "JoinHarnessTest.scala:" in c["source"] and c["steps"] and c["expected"] and c["asserts"]
    assert [c["name"] for c in KATS] == [
        "row_time_inner_join_with_common_bounds", "row_time_inner_join_with_negative_bounds",
        "row_time_left_outer_join", "row_time_right_outer_join", "row_time_full_outer_join"]


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_kat_through_the_restatement(case):
    eng = RefEngine(case["join_type"], case["lower"], case["upper"], case["allowed_lateness"])
    seen = []

    def check(n, what, value):
        got = eng.ref.num_event_time_timers() if what == "timers" else eng.ref.num_keyed_state_entries()
        seen.append(1)
        assert got == value, (n, what, got, value)

    got = replay_kat(case, eng, check)
    assert len(seen) == len(case["asserts"])
    gs, gw = segments(got)
    es, ew = segments(case["expected"])
    assert gw == ew
    assert gs == es


# ---- hand-derived edge cases (expected values worked out from the semantics, not from the restatement)
def gate_scenario(engine):
    """INNER (-10, 20): leftRelativeSize 10, rightRelativeSize 20.  Returns the rows of the last push."""
    engine.watermark(50)
    # left row C@45 passes the gate (0 < 55): rightExpirationTime := 50 - 20 - 1 = 29
    assert engine.push([0], [3], [45], [0]) == []
    # right rows A@100 and B@100 are cached (50 < 120); their clean-up timers are 100 + 20 + 15 + 1 = 136
    assert engine.push([1, 1], [1, 2], [100, 100], [7, 8]) == []
    engine.watermark(130)  # C's timer (71) fires and cleans the left cache; 136 is not due
    # rightExpirationTime is still 29 (stale), the expiration time of this epoch is 130 - 20 - 1 = 109:
    #   A@125 (upper bound 135 > 29) is the first to pass the gate: it scans, A's right row 100 is outside
    #         [105, 135] and <= 109: removed
    #   B@95  (upper bound 105 <= 109) does not scan although B's right row 100 is inside [75, 105]: no pair
    #   B@101 (111 > 109) scans: the expired row 100 is inside [81, 111]: one pair, then the row is gone
    #   B@102 (112 > 109) scans an empty cache
    return engine.push([0, 0, 0, 0], [1, 2, 2, 2], [125, 95, 101, 102], [1, 2, 3, 4])


def test_gate_first_scanner_with_a_stale_expiration_time_and_an_expired_row_joined_once():
    eng = RefEngine("inner", -10, 20)
    rows = gate_scenario(eng)
    # ordinals: C = 0, A = 1, B = 2 (right rows), then 3, 4, 5, 6
    assert rows == [(2, 5, 2, 101, 100, 3, 8, 5, -1)]
    st = eng.ref.stats()
    assert st["pairs"] == 1 and st["pairs_with_expired_rows"] == 1 and st["gate_skips"] == 1
    assert eng.ref.X == [119, 109]  # the left cache's from C's timer at 130, the right cache's from A's scan


def test_remaining_row_at_time_zero_clears_the_cache_without_padding():
    # reachable through restored state only: a timer that fires while its cache's expiration time is negative
    ref = TimeBoundedJoinRef("full", -5, 9)
    ref.restore({"key": [1], "left_timer": [0], "right_timer": [3], "n_rows": [2], "side": [0, 0], "rowtime": [0, 4],
                 "ordinal": [0, 1], "val": [5, 6], "emitted": [0, 0]})
    rows, fw = ref.watermark(3)  # expiration 3 - 5 - 1 = -3: nothing expired, the earliest remaining row is at 0
    assert rows == [] and fw == 3 - 9
    assert ref.stats()["store_rows"] == 0 and ref.stats()["active_timers"] == 0
    assert ref.num_keyed_state_entries() == 0 and ref.watermark(LMAX)[0] == []


def test_allowed_lateness_moves_the_timer_the_expiration_and_the_forwarded_watermark():
    ref = TimeBoundedJoinRef("left", -5, 9, allowed_lateness=4)
    assert ref.push([0], [1], [1], [11]) == []
    assert ref.watermark(17) == ([], 17 - 13)
    rows, fw = ref.watermark(18)  # 1 + 5 + 7 + 4 + 1
    assert rows == [(1, 0, -1, 1, 0, 11, 0, -1, 18)] and fw == 5


@pytest.mark.parametrize("lower,upper,first,second,miss", [
    (0, 0, (0, 5), (1, 5), (1, 6)),        # l.rowtime = r.rowtime
    (3, 3, (1, 10), (0, 13), (0, 12)),     # both bounds positive: l = r + 3
    (-3, -3, (0, 10), (1, 13), (1, 12)),   # both negative: l = r - 3
    (2, 5, (1, 10), (0, 15), (0, 16)),
    (-5, -2, (0, 10), (1, 15), (1, 16)),
])
def test_one_sided_bounds(lower, upper, first, second, miss):
    ref = TimeBoundedJoinRef("inner", lower, upper)
    assert ref.process(first[0], 1, first[1]) == []
    rows = ref.process(second[0], 1, second[1])
    lt, rt = (first[1], second[1]) if first[0] == 0 else (second[1], first[1])
    lo, ro = (0, 1) if first[0] == 0 else (1, 0)
    assert rows == [(1, lo, ro, lt, rt, 0, 0, 1, -1)]
    assert ref.process(miss[0], 1, miss[1]) == []


def test_long_max_watermark_ends_the_stream():
    ref = TimeBoundedJoinRef("full", -5, 9)
    ref.push([0, 1], [1, 2], [100, 200], [1, 2])
    rows, fw = ref.watermark(LMAX)
    assert sorted(rows) == [(1, 0, -1, 100, 0, 1, 0, -1, 113), (2, -1, 1, 0, 200, 0, 2, -1, 217)]
    assert fw == LMAX - 9 and ref.X == [LMAX, LMAX]
    # afterwards nothing scans and nothing is cached: an arriving row is padded at once
    assert ref.push([0], [2], [300], [3]) == [(2, 2, -1, 300, 0, 3, 0, 2, -1)]
    assert ref.stats()["gate_skips"] == 1 and ref.stats()["store_rows"] == 0


def test_forwarded_watermark_wraps_like_the_reference():
    ref = TimeBoundedJoinRef("inner", -10, 20)
    assert ref.watermark(LMIN + 3)[1] == LMAX - 16


# ---- the seeded streams exercise every path (the GPU parity test proves nothing about them otherwise)
@pytest.mark.parametrize("kind", ["uniform", "zipf"])
@pytest.mark.parametrize("join_type", JOIN_TYPES)
def test_seeded_streams_are_not_vacuous(join_type, kind):
    calls, fws, st = ref_run(join_type, kind)
    n = PUSHES * PER_PUSH
    assert st["rows_in"] == n and len(calls) == len(fws) == PUSHES
    assert st["pairs"] >= n
    assert st["rows_not_cached"] * 100 >= n
    assert st["pairs_with_expired_rows"] > 0
    assert st["gate_skips"] > 0
    if join_type != "inner":
        assert st["padded_at_timer"] > 0 and st["padded_at_arrival"] > 0 and st["padded_at_scan"] > 0
    else:
        assert st["padded_at_timer"] == st["padded_at_arrival"] == st["padded_at_scan"] == 0
    assert st["cached_rows"] + st["rows_not_cached"] == n and st["store_rows"] == 0
    assert make_stream(kind)[0][2].min() >= 0 and BOUNDS == (-50, 30)


@pytest.mark.parametrize("lower,upper", [(-10000, 10000), (-6, 6)])
def test_brute_force_matches_the_restatement_for_one_key(lower, upper):
    sides, keys, ts, vals = single_key_rows(300)  # 600 rows
    ref = TimeBoundedJoinRef("inner", lower, upper)
    rows = ref.push(sides, keys, ts, vals)
    got = np.array(sorted((r[1], r[2]) for r in rows), dtype=np.int64).reshape(-1, 2)
    exp = brute_force_pairs(sides, ts, lower, upper)
    assert len(exp) > 0 and np.array_equal(got, exp)
    for r in rows:  # the later of the two emitted the pair
        assert r[7] == max(r[1], r[2])

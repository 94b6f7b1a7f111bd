"""Writes timejoin_kats.json: the five row-time sequences of the reference's JoinHarnessTest, transcribed as data.
Run from the repository root: python tests/golden/make_timejoin_kats.py"""
import json
import os

SRC = "flink-libraries/flink-table/src/test/scala/org/apache/flink/table/runtime/harness/JoinHarnessTest.scala"
L, R = 0, 1
N = None  # the null-padded side


def case(name, lines, join_type, lower, upper, script, expected):
    steps, asserts = [], []
    for s in script:
        if s[0] in ("timers", "entries"):
            asserts.append([len(steps), s[0], s[1]])  # holds after the first len(steps) steps
        else:
            steps.append(list(s))
    return {"name": name, "source": f"{SRC}:{lines}", "join_type": join_type, "lower": lower, "upper": upper,
            "allowed_lateness": 0, "steps": steps, "asserts": asserts, "expected": expected}


def e(side, key, t):
    return ("e", side, key, t)


def w(wm):
    return ("w", wm)


def row(lt, lk, rt, rk, ts=0):
    return ["row", lt, lk, rt, rk, ts]


def wm(v):
    return ["wm", v]


K1, K2 = "k1", "k2"
OUTER_SCRIPT = [
    e(L, K1, 1), e(R, K2, 1), ("timers", 2), ("entries", 4),
    w(14), ("timers", 1), ("entries", 2),
    w(18), ("timers", 0), ("entries", 0),
    e(L, K1, 2), e(R, K2, 2), ("entries", 0), ("timers", 0),
    e(L, K1, 19), e(L, K1, 20), e(R, K1, 26), e(R, K1, 25), e(L, K1, 21),
    e(R, K2, 39), e(R, K2, 40), e(L, K2, 50), e(L, K2, 49), e(R, K2, 41),
    w(100)]
OUTER_PAIRS = [row(20, K1, 25, K1), row(21, K1, 25, K1), row(21, K1, 26, K1),
               row(49, K2, 40, K2), row(49, K2, 41, K2), row(50, K2, 41, K2)]

CASES = [
    case("row_time_inner_join_with_common_bounds", "259-354", "inner", -10, 20, [
        w(1), e(L, K1, 1), ("timers", 1), e(L, K1, 2), e(R, K1, 2), ("timers", 2), ("entries", 4),
        e(L, K1, 5), e(R, K1, 15), w(20), ("entries", 4), e(L, K1, 35), w(38),
        e(L, K2, 40), e(R, K2, 39), ("entries", 6), w(61), ("entries", 4)],
        [wm(-19), row(1, K1, 2, K1), row(2, K1, 2, K1), row(5, K1, 2, K1), row(5, K1, 15, K1), wm(0),
         row(35, K1, 15, K1), wm(18), row(40, K2, 39, K2), wm(41)]),
    case("row_time_inner_join_with_negative_bounds", "358-436", "inner", -10, -7, [
        w(1), e(R, K1, 2), ("entries", 0), w(2), e(L, K1, 3), e(R, K1, 3), e(R, K1, 13), e(L, K1, 6),
        ("entries", 4), w(10), ("entries", 2), w(18), ("entries", 0)],
        [wm(-9), wm(-8), row(3, K1, 13, K1), row(6, K1, 13, K1), wm(0), wm(8)]),
    case("row_time_left_outer_join", "440-550", "left", -5, 9, OUTER_SCRIPT,
         [row(1, K1, N, N, 14), wm(5), wm(9), row(2, K1, N, N)] + OUTER_PAIRS + [row(19, K1, N, N, 32), wm(91)]),
    case("row_time_right_outer_join", "554-663", "right", -5, 9, OUTER_SCRIPT,
         [wm(5), row(N, N, 1, K2, 18), wm(9), row(N, N, 2, K2)] + OUTER_PAIRS + [row(N, N, 39, K2, 56), wm(91)]),
    case("row_time_full_outer_join", "667-784", "full", -5, 9, OUTER_SCRIPT,
         [row(1, K1, N, N, 14), wm(5), row(N, N, 1, K2, 18), wm(9), row(2, K1, N, N), row(N, N, 2, K2)] + OUTER_PAIRS +
         [row(19, K1, N, N, 32), row(N, N, 39, K2, 56), wm(91)]),
]

ABOUT = ("Row-time time-windowed join known answers, transcribed as data from the reference's JoinHarnessTest (paths "
         "relative to the reference root). steps: [\"w\", watermark] (processWatermark1 and processWatermark2 with the "
         "same value) or [\"e\", side (0 = processElement1, 1 = processElement2), key, rowtime]; every element's record "
         "timestamp is 0. asserts: [n, \"timers\" | \"entries\", value] = numEventTimeTimers / numKeyedStateEntries "
         "after the first n steps. expected, in position: [\"wm\", forwarded watermark] or [\"row\", left rowtime, "
         "left key, right rowtime, right key, record timestamp] (null = the padded side); the harness sorts the "
         "records between two watermarks before it compares. String keys are mapped to ids by the test.")

if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "timejoin_kats.json")
    with open(path, "w") as f:
        json.dump({"about": ABOUT, "cases": CASES}, f, indent=1)
        f.write("\n")

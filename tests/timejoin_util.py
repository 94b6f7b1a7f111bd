"""Shared by the time-windowed join tests: the JoinHarnessTest fixture and its replay through any engine, the seeded
tagged streams of the parity tests, and a numpy brute force for one key."""
import json
import os

import numpy as np

from .timejoin_ref import LMAX, TimeBoundedJoinRef

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "timejoin_kats.json")
KEY_IDS = {"k1": 1, "k2": 2}
KEY_NAMES = {v: k for k, v in KEY_IDS.items()}
JOIN_TYPES = ("inner", "left", "right", "full")
ROW_FIELDS = ("key", "left_ord", "right_ord", "left_rowtime", "right_rowtime", "left_val", "right_val", "cause_ord",
              "timer_ts")


def load_kats():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


class RefEngine:
    """TimeBoundedJoinRef behind the interface the replays use: push() and watermark() return row tuples."""

    def __init__(self, join_type, lower, upper, allowed_lateness=0, **_):
        self.ref = TimeBoundedJoinRef(join_type, lower, upper, allowed_lateness)

    def push(self, sides, keys, rowtimes, vals=None):
        return self.ref.push(sides, keys, rowtimes, vals)

    def watermark(self, wm):
        return self.ref.watermark(wm)


def replay_kat(case, engine, check_counts=None):
    """The case's steps through `engine`; returns the output in the fixture's `expected` form.  check_counts(n, what,
    value) is called for every recorded assert (the restatement answers them; the GPU handle has no such view)."""
    out = []
    asserts = {}
    for n, what, value in case["asserts"]:
        asserts.setdefault(n, []).append((what, value))

    def rows_of(rows):
        for r in sorted(rows):
            key, lo, ro, lt, rt, _, _, cause, tts = r
            name = KEY_NAMES[key]
            out.append(["row", lt if lo >= 0 else None, name if lo >= 0 else None, rt if ro >= 0 else None,
                        name if ro >= 0 else None, tts if cause < 0 else 0])

    for i, s in enumerate(case["steps"]):
        if s[0] == "w":
            rows, fw = engine.watermark(s[1])
            rows_of(rows)
            out.append(["wm", fw])
        else:
            rows_of(engine.push([s[1]], [KEY_IDS[s[2]]], [s[3]], [0]))
        if check_counts:
            for what, value in asserts.get(i + 1, ()):
                check_counts(i + 1, what, value)
    return out


def segments(stream):
    """(sorted rows between watermarks, watermarks by position): what the harness's comparator compares"""
    segs, wms, cur = [], [], []
    for x in stream:
        if x[0] == "wm":
            segs.append(sorted(cur, key=repr))
            cur = []
            wms.append(x[1])
        else:
            cur.append(x)
    segs.append(sorted(cur, key=repr))
    return segs, wms


# ---- seeded streams: pushes of tagged rows with jitter and a tail of very late rows, a watermark after each
PUSHES, PER_PUSH, SPAN, JITTER, TAIL = 24, 2000, 200, 120, 0.03
BOUNDS = (-50, 30)
STREAMS = {"uniform": (97, None), "zipf": (500, 1.1)}


def make_stream(kind, seed=0x7101, pushes=PUSHES, per_push=PER_PUSH):
    """[(sides, keys, rowtimes, vals, watermark)]; the last watermark is Long.MAX_VALUE"""
    nkeys, zipf_s = STREAMS[kind]
    rng = np.random.default_rng(seed)
    p = None
    if zipf_s is not None:
        p = 1.0 / np.arange(1, nkeys + 1) ** zipf_s
        p /= p.sum()
    out = []
    for q in range(pushes):
        base = 1000 + q * SPAN
        keys = rng.choice(nkeys, per_push, p=p).astype(np.int64) * 7919 - 300
        sides = rng.integers(0, 2, per_push).astype(np.uint8)
        ts = base + rng.integers(0, SPAN, per_push) - rng.integers(0, JITTER, per_push)
        late = rng.random(per_push) < TAIL
        ts = np.where(late, base - rng.integers(150, 400, per_push), ts).astype(np.int64)
        vals = rng.integers(-(1 << 40), 1 << 40, per_push).astype(np.int64)
        out.append((sides, keys, ts, vals, base + SPAN - 40 if q < pushes - 1 else LMAX))
    return out


_REF_RUNS = {}


def ref_run(join_type, kind):
    """The restatement over make_stream(kind), computed once: ([sorted rows per push + watermark call], [forwarded
    watermarks], stats)"""
    if (join_type, kind) not in _REF_RUNS:
        ref = TimeBoundedJoinRef(join_type, *BOUNDS)
        calls, fws = [], []
        for sides, keys, ts, vals, wm in make_stream(kind):
            rows = ref.push(sides, keys, ts, vals)
            more, fw = ref.watermark(wm)
            calls.append(sorted(rows + more))
            fws.append(fw)
        _REF_RUNS[(join_type, kind)] = (calls, fws, ref.stats())
    return _REF_RUNS[(join_type, kind)]


def rows_as_tuples(a):
    """a TJOIN_ROW_DTYPE array as the restatement's row tuples"""
    cols = [a[f].tolist() for f in ROW_FIELDS]
    return list(zip(*cols))


# ---- one key holds every row
def single_key_rows(n_each=1500, seed=0x51):
    """n_each left and n_each right rows of one key, interleaved; row times in [0, 4 * n_each)"""
    rng = np.random.default_rng(seed)
    n = 2 * n_each
    sides = (np.arange(n) % 2).astype(np.uint8)
    ts = rng.integers(0, 4 * n_each, n).astype(np.int64)
    keys = np.full(n, 42, np.int64)
    vals = np.arange(n, dtype=np.int64) * 3 + 1
    return sides, keys, ts, vals


def brute_force_pairs(sides, ts, lower, upper):
    """With no watermark every row is cached and scans (bounds with t - lower > 0 and t + upper > 0 for every row): the
    pairs are all (l, r) with lower <= l.rowtime - r.rowtime <= upper.  Returns sorted (left_ord, right_ord) rows."""
    li, ri = np.nonzero(sides == 0)[0], np.nonzero(sides == 1)[0]
    d = ts[li][:, None] - ts[ri][None, :]
    a, b = np.nonzero((d >= lower) & (d <= upper))
    pairs = np.stack([li[a], ri[b]], axis=1)
    return pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]

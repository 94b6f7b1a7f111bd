"""Window joins (flink_amd.join.GpuWindowJoin, fw_list_*_join): streams, the reference and the comparison shared by
tests/test_join_abi.py (CPU: the reference alone) and tests/test_gpu_join.py.

The reference is the window-contents oracle (oracle.ListWindowOracle; tests.continuous_ref.ContinuousRef, which has its
interface, for ContinuousEventTimeTrigger, which the oracle does not have) driven with the union stream, exactly as
CoGroupedStreams.WithWindow.apply builds the operator (CoGroupedStreams.java:273-304).  Its contents() are each firing's
elements with arrival ordinals; the driver keeps the side of every ordinal it pushed, splits each firing by side
(CoGroupWindowFunction.apply, :657-685) and forms the cross product first-input-major (JoinCoGroupFunction.coGroup,
JoinedStreams.java:387-404).

A stream is a list of steps ("push", side, keys, ts, vals) and ("wm", side or None, watermark): one batch comes from one
input; a watermark of one input reaches the operator as the minimum of both when that rises."""
import json
import os
from collections import Counter

import numpy as np

LMIN, LMAX = -(1 << 63), (1 << 63) - 1
SIDE = 1 << 62
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cogroup_join_kats.json")


def load_kats():
    with open(FIXTURE) as f:
        return json.load(f)


# ---------------------------------------------------------------- streams
def kat_stream(case, interleave, delta):
    """the case's two sources as steps; interleave "first" = all of input 1, then input 2; "alternate" = element by
    element.  Every element is followed by its input's punctuated watermark ts + delta, a finished source by
    Long.MAX_VALUE.  A self-join (source2 null) pushes each batch on both sides."""
    def steps(side, recs):
        out = []
        for r in recs:
            out.append([("push", side, [r["key"]], [r["ts"]], [r["val"]]), ("wm", side, r["ts"] + delta)])
        return out
    s1 = steps(0, case["source1"])
    s2 = steps(1, case["source2"] if case["source2"] is not None else case["source1"])
    if case["source2"] is None:  # each element arrives on both inputs
        return [x for a, b in zip(s1, s2) for x in a + b] + [("wm", None, LMAX)]
    if interleave == "first":
        return [x for a in s1 for x in a] + [("wm", 0, LMAX)] + [x for b in s2 for x in b] + [("wm", 1, LMAX)]
    out = []
    for i in range(max(len(s1), len(s2))):
        for s in (s1, s2):
            if i < len(s):
                out += s[i]
    return out + [("wm", 0, LMAX), ("wm", 1, LMAX)]


def seeded_stream(seed=11, n=4000, keys=40, span=2000, jitter=300, wm_lag=60, wm_every=3, f64=False):
    """n records in batches of one side each (sides uniform), timestamps in [0, span) rising with a jitter, a watermark
    for both inputs after every wm_every batches, wm_lag behind the largest timestamp so far"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, keys, n, dtype=np.int64)
    t = np.clip(np.arange(n, dtype=np.int64) * span // n + jitter // 2 - rng.integers(0, jitter, n, dtype=np.int64), 0,
                span - 1)
    v = rng.integers(-1000, 1000, n, dtype=np.int64)
    if f64:
        v = v.astype(np.float64) * 0.37
    out, i, b = [], 0, 0
    while i < n:
        m = int(rng.integers(1, 60))
        out.append(("push", int(rng.integers(0, 2)), k[i:i + m], t[i:i + m], v[i:i + m]))
        i += m
        b += 1
        if b % wm_every == 0:
            out.append(("wm", None, int(t[:i].max()) - wm_lag))
    return out + [("wm", None, LMAX)]


def hot_stream():
    """one (key 7, window [0, 1000)) of 1500 x 1100 elements (1.65M pairs: hundreds of emit chunks, more than 2^16
    pairs in a row) pushed in batches of alternating side, among small rows: keys with one input only, rows with a
    single element of input 2, small two-sided rows -- rows are laid out by the hash of (key, window), so the hot row
    lies among them"""
    rng = np.random.default_rng(5)
    out = []

    def push(side, key, n):
        out.append(("push", side, np.full(n, key, dtype=np.int64), rng.integers(0, 1000, n, dtype=np.int64),
                    rng.integers(-10 ** 6, 10 ** 6, n, dtype=np.int64)))
    for key in range(100, 110):
        push(0, key, 3)          # input 1 only
        push(1, key + 100, 2)    # input 2 only
        push(0, key + 200, 4)    # n2 == 1
        push(1, key + 200, 1)
        push(1, key + 300, 3)    # small two-sided rows
        push(0, key + 300, 2)
    for _ in range(5):
        push(0, 7, 300)
        push(1, 7, 220)
    for key in range(110, 120):
        push(0, key, 1)
        push(1, key + 100, 5)
    return out + [("wm", None, 999)]


def count_stream():
    """one row of 70000 x 70000 elements: 4.9e9 pairs, past 2^32, that no test materialises"""
    n = 70000
    k = np.full(n, 3, dtype=np.int64)
    t = np.arange(n, dtype=np.int64) % 1000
    return [("push", 0, k, t, np.arange(n, dtype=np.int64)), ("push", 1, k, t, -np.arange(n, dtype=np.int64)),
            ("wm", None, 999)]


# the configurations of the seeded parity test: (id, reference keywords, stream keywords)
SEEDED = [
    ("sliding", dict(assigner="sliding", size=100, slide=25, lateness=40), {}),
    ("tumbling", dict(assigner="tumbling", size=100, lateness=40), {}),
    ("tumbling-purging-count3", dict(assigner="tumbling", size=100, lateness=40, trigger="count", trigger_count=3,
                                     purging=True), {}),
    ("tumbling-evict4-before", dict(assigner="tumbling", size=100, lateness=40, evictor="count", evict_arg=4), {}),
    ("tumbling-evict4-after", dict(assigner="tumbling", size=100, lateness=40, evictor="count", evict_arg=4,
                                   evict_after=True), {}),
    ("tumbling-continuous33", dict(assigner="tumbling", size=100, lateness=40, trigger="continuous", interval=33), {}),
    ("session30", dict(assigner="session", gap=30, lateness=40), {}),
    ("session30-merging-state", dict(assigner="session", gap=30, lateness=40, merging_state=True), {}),
    ("sliding-double", dict(assigner="sliding", size=100, slide=25, lateness=40, value_type="f64"), dict(f64=True)),
    ("tumbling-device-columns", dict(assigner="tumbling", size=100, lateness=40, device_columns=True), {}),
]


def make_ref(assigner="tumbling", merging_state=False, device_columns=False, **kw):
    """the reference operator of a configuration"""
    if kw.get("trigger") == "continuous":
        from tests.continuous_ref import ContinuousRef
        return ContinuousRef(assigner=assigner, **kw)
    from oracle import oracle as orc
    return orc.ListWindowOracle(assigner=assigner, **kw)


def make_gpu(assigner="tumbling", size=0, slide=0, offset=0, gap=0, lateness=0, trigger="event_time", trigger_count=0,
             interval=0, purging=False, evictor="none", evict_after=False, evict_arg=0, value_type="i64",
             merging_state=False, device_columns=False, mode="join", **kw):
    from flink_amd import (ContinuousEventTimeTrigger, CountEvictor, CountTrigger, EventTimeSessionWindows,
                           EventTimeTrigger, PurgingTrigger, SlidingEventTimeWindows, TumblingEventTimeWindows)
    from flink_amd.join import GpuWindowJoin
    a = (EventTimeSessionWindows.with_gap(gap) if assigner == "session"
         else TumblingEventTimeWindows.of(size, offset) if assigner == "tumbling"
         else SlidingEventTimeWindows.of(size, slide, offset))
    trig = (CountTrigger.of(trigger_count) if trigger == "count"
            else ContinuousEventTimeTrigger.of(interval) if trigger == "continuous" else EventTimeTrigger.create())
    if purging:
        trig = PurgingTrigger.of(trig)
    ev = CountEvictor.of(evict_arg, evict_after) if evictor == "count" else None
    return GpuWindowJoin(a, trig, ev, mode=mode, allowed_lateness=lateness,
                         value_type={"i64": "long", "f64": "double"}[value_type], merging_state=merging_state, **kw)


# ---------------------------------------------------------------- the reference driver
def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.int64) if v.dtype == np.float64 else v.astype(np.int64)


class RefJoin:
    """the oracle over the union stream, the side of every ordinal, and the union's watermark valve"""

    def __init__(self, ref):
        self.ref, self.sides, self.in_wm, self.out_wm = ref, [], [LMIN, LMIN], LMIN

    def step(self, st):
        """True when the step reached the operator (a watermark that does not raise the minimum does not)"""
        if st[0] == "push":
            _, side, k, t, v = st
            self.ref.process(np.asarray(k, dtype=np.int64), np.asarray(t, dtype=np.int64), np.asarray(v))
            self.sides += [side] * len(k)
            return True
        _, side, wm = st
        for s in ((0, 1) if side is None else (side,)):
            self.in_wm[s] = max(self.in_wm[s], wm)
        m = min(self.in_wm)
        if m <= self.out_wm:
            return False
        self.out_wm = m
        self.ref.watermark(m)
        return True

    def firings(self, start=0, ordinals=True):
        """[(row tuple, first list, second list)] of the firings from index `start` on: the row is (epoch, key, start,
        end, count, sum, min, max[, first ordinal]), a list holds (ts, value bits[, ordinal]) in list order"""
        sides = np.asarray(self.sides, dtype=np.int64)
        out = []
        for r, el in self.ref.contents()[start:]:
            o = np.asarray(el["ordinal" if "ordinal" in el.dtype.names else "ord"], dtype=np.int64)
            s = sides[o] if len(o) else o
            out.append(_firing(r, el["ts"], el["val"], o, s, ordinals))
        return out


def _firing(r, ts, val, o, s, ordinals):
    row = tuple(int(r[f]) for f in ("epoch", "key", "start", "end", "count", "sum", "min", "max"))
    if ordinals:
        row += (int(r["first"]),)
    cols = (ts, val, o) if ordinals else (ts, val)
    lists = tuple(tuple(zip(*(np.asarray(c)[s == x].tolist() for c in cols))) for x in (0, 1))
    return row, lists[0], lists[1]


def gpu_firings(j, start=0, ordinals=True):
    """the same of a GpuWindowJoin from row `start` on, from its partitioned elements; asserts on the way that a row's
    first n_first elements are of input 1 and the others of input 2"""
    out = []
    rows, nf, el = j.rows(), j.n_first(), j.elems()
    for r, n1 in list(zip(rows, nf.tolist()))[start:]:
        e = el[r["elem_off"]:r["elem_off"] + r["count"]]
        s = (e["ordinal"] & SIDE != 0).astype(np.int64)
        assert not s[:n1].any() and s[n1:].all(), (r, n1)
        out.append(_firing(r, e["ts"], e["val"], e["ordinal"] & ~SIDE, s, ordinals))
    return out


def expected_pairs(first, second):
    """JoinCoGroupFunction.coGroup over two lists of (ts, val, ord): columns val1, val2, ord1, ord2"""
    n1, n2 = len(first), len(second)
    if not n1 or not n2:
        return tuple(np.zeros(0, dtype=np.int64) for _ in range(4))
    a, b = np.asarray(first, dtype=np.int64), np.asarray(second, dtype=np.int64)
    return np.repeat(a[:, 1], n2), np.tile(b[:, 1], n1), np.repeat(a[:, 2], n2), np.tile(b[:, 2], n1)


def check_pairs(j, firings, start_row=0, start_pair=0):
    """the pairs of the rows from start_row on are, row by row and in order, the cross product of the row's lists;
    returns the number of pairs checked"""
    p = j.pairs()
    rows = j.rows()[start_row:]
    assert len(rows) == len(firings)
    q = start_pair
    for r, (_, first, second) in zip(rows, firings):
        v1, v2, o1, o2 = expected_pairs(first, second)
        s = p[q:q + len(v1)]
        assert len(s) == len(v1), (len(p), q, len(v1))
        for f in ("epoch", "key", "start", "end"):
            assert (s[f] == r[f]).all(), f
        assert np.array_equal(s["val1"], v1) and np.array_equal(s["val2"], v2)
        assert np.array_equal(s["ord1"], o1) and np.array_equal(s["ord2"], o2)
        q += len(v1)
    return q - start_pair


def count_pairs(firings):
    return sum(len(a) * len(b) for _, a, b in firings)


def same_firings(got, exp):
    g, e = Counter(got), Counter(exp)
    assert sum(g.values()) == sum(e.values()), (sum(g.values()), sum(e.values()))
    assert g == e, (list((g - e).items())[:2], list((e - g).items())[:2])


def gpu_step(j, st):
    if st[0] == "push":
        _, side, k, t, v = st
        (j.process2 if side else j.process1)(k, t, v)
    else:
        _, side, wm = st
        (j.watermark if side is None else j.watermark2 if side else j.watermark1)(wm)


def run_both(j, ref, stream, ordinals=True, device=False):
    """drives both with the stream; after every step the new firings (their split and their pairs), the late count
    and the operator's state and timer counts are compared.  Returns the reference's firings."""
    rj = RefJoin(ref)
    nrows = npairs = 0
    for st in stream:
        if st[0] == "push" and device:
            import torch
            st = st[:2] + tuple(torch.as_tensor(np.ascontiguousarray(c)).cuda() for c in st[2:])
            gpu_step(j, st)
            st = st[:2] + tuple(c.cpu().numpy() for c in st[2:])
        else:
            gpu_step(j, st)
        rj.step(st)
        exp = rj.firings(nrows, ordinals)
        got = gpu_firings(j, nrows, ordinals)
        same_firings(got, exp)
        if j.mode == "join":
            npairs += check_pairs(j, got, nrows, npairs)
        nrows += len(got)
        s = j.stats()
        assert s["late_records_dropped"] == ref.late_dropped
        assert s["keyed_state_entries"] == ref.num_state_entries
        assert s["event_time_timers"] == ref.num_timers
    assert len(j.pairs()) == (npairs if j.mode == "join" else 0)
    return rj.firings(0, ordinals)


def classes(firings):
    """what a set of firings exercises"""
    c = Counter()
    seen = Counter()
    for row, a, b in firings:
        n1, n2 = len(a), len(b)
        c["rows"] += 1
        c["pairs"] += n1 * n2
        c["largest"] = max(c["largest"], n1 * n2)
        c["only_first"] += n1 > 0 and n2 == 0
        c["only_second"] += n1 == 0 and n2 > 0
        c["empty"] += n1 == 0 and n2 == 0
        c["both"] += n1 > 0 and n2 > 0
        c["n2_is_1"] += n1 > 1 and n2 == 1
        c["n1_is_1"] += n1 == 1 and n2 > 1
        seen[row[1:4]] += 1
        c["refired"] += seen[row[1:4]] == 2
    return c

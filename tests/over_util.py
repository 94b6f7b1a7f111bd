"""Helpers of the OVER window tests: the known answers of tests/golden/over_kats.json replayed through anything with
process(keys, rowtimes, columns, nulls) / watermark(wm) -> [(key, rowtime, ordinal, [values])] (the restatement
tests/over_ref.py and the GPU operator alike), and seeded streams."""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "over_kats.json")
LMAX = (1 << 63) - 1
KINDS = ("bounded_rows", "bounded_range", "unbounded_rows", "unbounded_range")


def load_kats():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def key_ids(case):
    """String keys -> ids (1, 2, ... in order of appearance); integer keys stay."""
    ids = {}
    for s in case["steps"]:
        if s[0] == "e" and isinstance(s[1], str) and s[1] not in ids:
            ids[s[1]] = len(ids) + 1
    return ids


def replay_kat(case, op):
    """Consecutive elements go in as one push.  Returns the emitted rows as (key, forwarded fields, values), the
    forwarded fields re-attached by ordinal, in emission order."""
    ids = key_ids(case)
    kid = lambda k: ids[k] if isinstance(k, str) else int(k)  # noqa: E731
    fwd, out, pend = [], [], []

    def flush():
        if pend:
            nc = len(pend[0][3])
            op.process(np.array([kid(p[1]) for p in pend], dtype=np.int64),
                       np.array([p[2] for p in pend], dtype=np.int64),
                       [np.array([p[3][j] for p in pend], dtype=np.int64) for j in range(nc)], None)
            pend.clear()

    def emit(rows):
        for key, _rowtime, ordinal, vals in rows:
            out.append((key, tuple(fwd[ordinal]), tuple(vals)))

    for s in case["steps"]:
        if s[0] == "e":
            fwd.append(s[4])
            pend.append(s)
        else:
            flush()
            emit(op.watermark(s[1]))
    flush()
    if case["final_max_watermark"]:
        emit(op.watermark(LMAX))
    return out


def expected_rows(case):
    ids = key_ids(case)
    return [(ids[k] if isinstance(k, str) else int(k), tuple(f), tuple(v)) for k, f, v in case["expected"]]


def check_kat(case, got):
    """Per key in order with keys sorted (`ordered`), or as sorted lists (the ITCases compare sorted strings)."""
    exp = expected_rows(case)
    if case["ordered"]:
        for k in sorted({r[0] for r in exp} | {r[0] for r in got}):
            assert [r for r in got if r[0] == k] == [r for r in exp if r[0] == k], (case["name"], k)
    else:
        assert sorted(got, key=repr) == sorted(exp, key=repr), case["name"]


# ---------------------------------------------------------------- seeded streams (test_gpu_over.py)
TYPES5 = ["long", "int", "short", "byte", "double"]
AGGS16 = [("count_star", 0), ("count", 1), ("sum", 0), ("avg", 0), ("min", 0), ("max", 0), ("sum", 1), ("avg", 1),
          ("sum", 2), ("avg", 2), ("sum", 3), ("avg", 3), ("sum", 4), ("avg", 4), ("min", 4), ("max", 4)]


def seeded_stream(seed, n=12000, pushes=6, nkeys=97, zipf=0.0, jitter=400, lag=100):
    """Steps ("p", keys, rowtimes, columns, nulls) / ("w", wm): row i's nominal time is 1000 + i // 2, pulled back by
    up to `jitter` ms (out of order within and across pushes); after each push the watermark goes to the largest row
    time so far - lag, so the head of the next push is late; a final Long.MAX_VALUE watermark.  Columns TYPES5: Long
    values whose sums wrap at 64 bits, Int values whose sums wrap at 32, Short, Byte, Double in [1, 1000); about a
    fifth of every column NULL, and the Int column NULL in every row of the keys divisible by 5."""
    rng = np.random.default_rng(seed)
    if zipf:
        w = 1.0 / np.arange(1, nkeys + 1) ** zipf
        keys = rng.choice(nkeys, size=n, p=w / w.sum()).astype(np.int64) + 1
    else:
        keys = rng.integers(1, nkeys + 1, size=n, dtype=np.int64)
    ts = 1000 + np.arange(n, dtype=np.int64) // 2 - rng.integers(0, jitter, size=n, dtype=np.int64)
    cols = [rng.integers(-(1 << 62), 1 << 62, size=n, dtype=np.int64),
            rng.integers((1 << 31) - 4096, 1 << 31, size=n, dtype=np.int64) * rng.choice([-1, 1], size=n),
            rng.integers(-(1 << 15), 1 << 15, size=n, dtype=np.int64),
            rng.integers(-128, 128, size=n, dtype=np.int64),
            rng.uniform(1.0, 1000.0, size=n)]
    cols[1] = np.clip(cols[1], -(1 << 31), (1 << 31) - 1)
    nulls = np.zeros(n, dtype=np.uint8)
    for j in range(5):
        nulls |= (rng.random(n) < 0.2).astype(np.uint8) << j
    nulls[keys % 5 == 0] |= 2
    steps, hi = [], -(1 << 62)
    for p in range(pushes):
        a, b = p * n // pushes, (p + 1) * n // pushes
        steps.append(("p", keys[a:b], ts[a:b], [c[a:b] for c in cols], nulls[a:b]))
        hi = max(hi, int(ts[a:b].max()))
        steps.append(("w", hi - lag))
    steps.append(("w", LMAX))
    return steps


def run_steps(op, steps):
    """Every watermark's rows: [[(key, rowtime, ordinal, [values])]]."""
    out = []
    for s in steps:
        if s[0] == "p":
            op.process(s[1], s[2], s[3], s[4])
        else:
            out.append(op.watermark(s[1]))
    return out


def by_key(rows):
    d = {}
    for key, rowtime, ordinal, vals in rows:
        d.setdefault(key, []).append((rowtime, ordinal, vals))
    return d


def assert_same_rows(got, exp, rtol, ordinals=True):
    """Per key in (rowtime, arrival) order; integers and NULLs exact, floats within rtol.  Finite float
    expectations only: a relative tolerance cannot match a NaN or an infinity (and does not see a zero's sign); such
    values are compared by bits, tests/over_edges_util.py::same_rows_bits."""
    g, e = by_key(got), by_key(exp)
    assert sorted(g) == sorted(e), (len(g), len(e))
    for k in e:
        assert len(g[k]) == len(e[k]), (k, len(g[k]), len(e[k]))
        for (gt, go, gv), (et, eo, ev) in zip(g[k], e[k]):
            assert gt == et and (go == eo or not ordinals), (k, gt, go, et, eo)
            for q, (a, b) in enumerate(zip(gv, ev)):
                if isinstance(b, float) and a is not None:
                    assert math.isfinite(b), ("assert_same_rows cannot judge a non-finite expectation", k, gt, q, a, b)
                    assert abs(a - b) <= rtol * abs(b), (k, gt, q, a, b)
                else:
                    assert a == b and type(a) is type(b), (k, gt, q, a, b)


# ---------------------------------------------------------------- frames evaluated directly (one firing, fresh keys)
def brute_frames(kind, preceding, keys, ts, cols, nulls, aggregates):
    """The frames of a stream pushed into fresh keys and fired by one watermark above every row time (bounded kinds:
    every row time > 0), evaluated per row from its frame's bounds (sums from prefix differences in Python integers, extremes from
    two overlapping power-of-two spans): Long columns only.  Returns [(key, rowtime,
    ordinal, [values])], a key's rows in (rowtime, arrival) order.  Independent of tests/over_ref.py (which
    test_over_ref.py holds it against) and fast enough for frames of thousands of rows."""
    n = len(keys)
    order = np.lexsort((np.arange(n), ts, keys))
    out = []
    k_s, t_s = keys[order], ts[order]
    starts = np.flatnonzero(np.r_[True, k_s[1:] != k_s[:-1]])
    ends = np.r_[starts[1:], n]
    for a, b in zip(starts, ends):
        idx = order[a:b]
        t = t_s[a:b]
        m = b - a
        pos = np.arange(m)
        if kind.endswith("rows"):
            hi = pos
            lo = np.maximum(0, pos - preceding) if kind.startswith("bounded") else np.zeros(m, dtype=np.int64)
        else:
            hi = np.searchsorted(t, t, "right") - 1
            lo = np.searchsorted(t, t - preceding, "left") if kind.startswith("bounded") else np.zeros(m, dtype=np.int64)
        res = []
        for fn, j in aggregates:
            if fn == "count_star":
                res.append([int(x) for x in hi - lo + 1])
                continue
            v = cols[j][idx]
            ok = ((nulls[idx] >> j) & 1) == 0 if nulls is not None else np.ones(m, dtype=bool)
            cnt = np.r_[0, np.cumsum(ok)]
            nn = cnt[hi + 1] - cnt[lo]
            if fn == "count":
                res.append([int(x) for x in nn])
            elif fn in ("sum", "avg"):
                ps = [0]
                for x, o in zip(v.tolist(), ok.tolist()):
                    ps.append(ps[-1] + (x if o else 0))
                col = []
                for i in range(m):
                    s = ps[hi[i] + 1] - ps[lo[i]]
                    if nn[i] == 0:
                        col.append(None)
                    elif fn == "sum":
                        s &= (1 << 64) - 1
                        col.append(s - (1 << 64) if s >> 63 else s)
                    else:
                        q = abs(s) // int(nn[i])
                        col.append(-q if s < 0 else q)
                res.append(col)
            else:
                ident = np.iinfo(np.int64).max if fn == "min" else np.iinfo(np.int64).min
                w = np.where(ok, v, ident)
                red = np.minimum if fn == "min" else np.maximum
                # every span 2^k from every row (clipped at the run's end); a frame is two overlapping spans
                tab = [w]
                while (1 << len(tab)) <= m:
                    h = 1 << (len(tab) - 1)
                    p = tab[-1]
                    tab.append(np.r_[red(p[:-h], p[h:]), p[m - h:]])
                k = np.floor(np.log2(hi - lo + 1)).astype(np.int64)
                val = np.empty(m, dtype=np.int64)
                for q in range(len(tab)):
                    sel = np.flatnonzero(k == q)
                    val[sel] = red(tab[q][lo[sel]], tab[q][hi[sel] + 1 - (1 << q)])
                res.append([None if nn[i] == 0 else int(val[i]) for i in range(m)])
        for i in range(m):
            out.append((int(k_s[a]), int(t[i]), int(idx[i]), [r[i] for r in res]))
    return out

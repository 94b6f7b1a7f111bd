"""Double specials, zero signs and firing cadence on the row-time OVER handle: the streams, the expectation and the
bit-exact comparison of tests/test_over_float_edges.py (CPU: the streams are not vacuous) and
tests/test_gpu_over_edges.py (GPU).

The values come from the palettes of tests/float_edges_util.py, so every finite partial sum is exact and a result is
comparable by its 64 bits whatever the evaluation order.  Two things differ from the keyed-window streams:

* DBL_MAX.  A retracting sum absorbs: (x + DBL_MAX) - DBL_MAX has lost x, in the reference's order and in any other
  in a different way, so a lone DBL_MAX among dyadics is not comparable.  Here DBL_MAX comes only as two peers (one
  row time, consecutive arrivals): DBL_MAX + DBL_MAX = +Inf, which a bounded key then keeps for good.
* NaNs with the sign bit set, as `np.inf - np.inf` gives them on x86 (0xfff8000000000000): a class of their own, and
  never canonicalised on the host.

Stream (`stream(variant)`, 16273 rows, time-ordered across its 8 pushes so that no cadence makes a row late):
* key 0 holds 2 * 4096 + 17 rows, row times 1 + position // 2 (peer pairs), so a run fired by one watermark starts at
  row 0 of the gathered rows and crosses the scan's 8-row, 512-row and 4096-row boundaries and the range minima's
  64-row blocks and 2048-row workgroups.  `variant` puts a special at the run positions SPECIAL_AT.
* 384 short keys (8 .. 391) of 21 rows: 7 peer groups of 3 rows, 20 ms apart.  Classes by key % 8 as in
  float_edges_util.specials, except 5 (dyadics >= 0 and one DBL_MAX peer pair), 6 (sign-set NaN among dyadics) and
  key % 16 == 7 (every value -0.0).  About a fifth of the values NULL; keys with key % 32 == 9 wholly NULL.
* columns: Double, Float (as float32; COUNT / MIN / MAX only), Long.
"""
import functools
import struct

import numpy as np

from tests.float_edges_util import DBL_MAX, NAN_BITS, NEG_ZERO_BITS, dyadic, specials
from tests.over_ref import OverRef, double_bits

LMAX = (1 << 63) - 1
NEG_NAN_BITS = 0xFFF8000000000000 - (1 << 64)     # as int64
NEG_NAN = np.array([NEG_NAN_BITS], dtype=np.int64).view(np.float64)[0]
INF_BITS = 0x7FF0000000000000

TYPES = ["double", "float", "long"]
AGGS = [("sum", 0), ("avg", 0), ("min", 0), ("max", 0), ("count", 0), ("min", 1), ("max", 1), ("count", 1),
        ("count_star", 0), ("sum", 2)]
Q_SUM, Q_AVG, Q_MIN, Q_MAX, Q_CNT, Q_FMIN, Q_FMAX = 0, 1, 2, 3, 4, 5, 6
FLOAT_SUMS, FLOAT_EXTREMES = (Q_SUM, Q_AVG), (Q_MIN, Q_MAX, Q_FMIN, Q_FMAX)
MAX_OF = {Q_MAX: 0, Q_FMAX: 1}          # aggregate -> column

FRAMES = [("bounded_rows", 1), ("bounded_rows", 5), ("bounded_rows", 200), ("bounded_range", 0), ("bounded_range", 50),
          ("unbounded_rows", 0), ("unbounded_range", 0)]
FRAME_IDS = [f"{k}-{p}" for k, p in FRAMES]
VARIANTS = ["nan", "neg_nan", "pinf", "pinf_ninf", "dbl_max_twice", "neg_zero"]

LONG_KEY, LONG_ROWS = 0, 2 * 4096 + 17
SPECIAL_AT = [0, 7, 8, 511, 512, 4095, 4096, 4097, LONG_ROWS - 1]
SHORT_KEYS, GROUPS, PEERS = 384, 7, 3
PUSHES = 8


def _long_specials(variant):
    """{run position: value} of key 0"""
    if variant == "pinf_ninf":       # +Inf, then -Inf, alternating along the positions (7 and 8 share a frame)
        return {p: (np.inf if q % 2 == 0 else -np.inf) for q, p in enumerate(SPECIAL_AT)}
    if variant == "dbl_max_twice":   # the position and its successor; (0, 1) and the other even positions are peers
        return {p + d: DBL_MAX for p in SPECIAL_AT for d in (0, 1) if p + d < LONG_ROWS}
    v = {"nan": np.nan, "neg_nan": NEG_NAN, "pinf": np.inf, "neg_zero": -0.0}[variant]
    return {p: v for p in SPECIAL_AT}


@functools.lru_cache(maxsize=None)
def stream(variant):
    """(keys, ts, [double f64, float f32, long i64], nulls, push bounds): rows in arrival order"""
    rng = np.random.default_rng(0x0E5)
    # key 0
    lk = np.full(LONG_ROWS, LONG_KEY, dtype=np.int64)
    lt = 1 + np.arange(LONG_ROWS, dtype=np.int64) // 2
    lv = rng.integers(0, 1 << 32, LONG_ROWS, dtype=np.int64)
    ld = dyadic(lk, lv, "f64")
    lf = dyadic(lk, lv >> 3, "f32")
    lnull = ((rng.random(LONG_ROWS) < 0.2).astype(np.uint8)) | ((rng.random(LONG_ROWS) < 0.2).astype(np.uint8) << 1)
    for p, v in _long_specials(variant).items():
        ld[p] = v
        lf[p] = v if abs(v) != DBL_MAX else np.finfo(np.float32).max
        lnull[p] = 0
    # the short keys
    ids = np.arange(8, 8 + SHORT_KEYS, dtype=np.int64)
    per = GROUPS * PEERS
    sk = np.repeat(ids, per)
    base = 1 + (ids * 2477) % (int(lt.max()) - 20 * GROUPS)
    st = np.repeat(base, per) + np.tile(np.repeat(np.arange(GROUPS, dtype=np.int64) * 20, PEERS), SHORT_KEYS)
    sv = rng.integers(0, 1 << 32, len(sk), dtype=np.int64)
    sd, sf = specials(sk, sv, "f64").copy(), specials(sk, sv >> 3, "f32").copy()
    snull = ((rng.random(len(sk)) < 0.2).astype(np.uint8)) | ((rng.random(len(sk)) < 0.2).astype(np.uint8) << 1)
    g = sk % 8
    row = np.tile(np.arange(per), SHORT_KEYS)
    sd[g == 5] = np.abs(dyadic(sk, sv, "f64"))[g == 5]
    pair = (g == 5) & ((row == 7) | (row == 8))        # the second and third peer of the third group
    sd[pair] = DBL_MAX
    snull[pair] &= 2
    for col, bit in ((sd, 0), (sf, 1)):
        nn = (g == 6) & (((sv >> (21 + 3 * bit)) & 7) < 2)
        col.view(np.int64)[nn] = NEG_NAN_BITS
    sd[sk % 16 == 7] = -0.0
    sf[sk % 16 == 7] = -0.0
    snull[sk % 32 == 9] |= 3
    keys, ts = np.concatenate([lk, sk]), np.concatenate([lt, st])
    d, f, nulls = np.concatenate([ld, sd]), np.concatenate([lf, sf]), np.concatenate([lnull, snull])
    # arrival: time-ordered across the pushes, the row times of a push in a shuffled order, peers in their order
    tmax = int(ts.max())
    edges = [tmax * q // PUSHES for q in range(PUSHES + 1)]
    rank = np.empty(tmax + 1, dtype=np.int64)
    for a, b in zip(edges[:-1], edges[1:]):
        rank[a + 1:b + 1] = a + 1 + rng.permutation(b - a)
    order = np.argsort(rank[ts], kind="stable")
    keys, ts, d, f, nulls = keys[order], ts[order], d[order], f[order], nulls[order]
    longs = ((np.arange(len(keys), dtype=np.int64) * 2654435761) % 2001) - 1000
    bounds = [int(np.searchsorted(rank[ts], e + 1)) for e in edges]
    bounds[0] = 0
    assert bounds[-1] == len(keys) <= 1 << 14
    return keys, ts, [d, f.astype(np.float32), longs], nulls, bounds


def pushes(variant):
    keys, ts, cols, nulls, bounds = stream(variant)
    return [(keys[a:b], ts[a:b], [c[a:b] for c in cols], nulls[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]


def cadence_watermarks(variant, cadence):
    """per push the watermarks that follow it; no row of a later push is at or below any of them"""
    ps = pushes(variant)
    out, done = [], 0
    for q, p in enumerate(ps):
        top = int(p[1].max())
        if cadence == "final":
            w = []
        elif cadence == "every_push":
            w = [top]
        else:  # every 37th row time
            w = list(range(done + 37, top + 1, 37))
            done = w[-1] if w else done
        out.append(w + ([LMAX] if q == len(ps) - 1 else []))
    return out


# ---------------------------------------------------------------- rows as arrays of raw words
def value_bits(v):
    if isinstance(v, float):
        return struct.unpack("<q", struct.pack("<d", v))[0]
    return 0 if v is None else int(v)


def rows_to_arrays(rows, aggs=AGGS):
    """[(key, rowtime, ordinal, [values])] -> drain_arrays()' fields; a Double as its raw bits"""
    n, ns = len(rows), len(aggs)
    out = {"key": np.empty(n, np.int64), "rowtime": np.empty(n, np.int64), "ordinal": np.empty(n, np.int64),
           "values": np.zeros((n, ns), np.int64), "null_mask": np.zeros(n, np.uint32)}
    for i, (k, t, o, vals) in enumerate(rows):
        out["key"][i], out["rowtime"][i], out["ordinal"][i] = k, t, o
        for q, v in enumerate(vals):
            if v is None:
                out["null_mask"][i] |= np.uint32(1 << q)
            else:
                out["values"][i, q] = value_bits(v)
    return out


def concat(parts):
    return {f: np.concatenate([p[f] for p in parts]) for f in ("key", "rowtime", "ordinal", "values", "null_mask")}


def _is_nan(bits):
    return ((bits & INF_BITS) == INF_BITS) & ((bits & 0x000FFFFFFFFFFFFF) != 0)


def same_rows_bits(got, exp, aggs=AGGS, types=TYPES):
    """Keys, row times, ordinals, NULLs and integer results exact; a key's rows emitted in (row time, arrival) order;
    Doubles by their 64 bits, except that a SUM / AVG that is NaN matches any NaN (DESIGN "NaN sum matches as a
    class"); a MIN / MAX that is NaN must be exactly 0x7ff8000000000000 (the expectation's is canonicalised, as
    Double.doubleToLongBits does)."""
    assert len(got["key"]) == len(exp["key"]) > 0, (len(got["key"]), len(exp["key"]))
    go = np.argsort(got["key"], kind="stable")
    k, t, o = got["key"][go], got["rowtime"][go], got["ordinal"][go]
    same = k[1:] == k[:-1]
    assert (~same | (t[1:] > t[:-1]) | ((t[1:] == t[:-1]) & (o[1:] > o[:-1]))).all(), "a key's rows out of order"
    eo = np.lexsort((exp["ordinal"], exp["rowtime"], exp["key"]))
    for f in ("key", "rowtime", "ordinal", "null_mask"):
        bad = np.flatnonzero(got[f][go] != exp[f][eo])
        assert bad.size == 0, (f, bad.size, got[f][go][bad[:3]], exp[f][eo][bad[:3]], k[bad[:3]], t[bad[:3]])
    gv, ev = got["values"][go], exp["values"][eo]
    for q, (fn, c) in enumerate(aggs):
        a, b = gv[:, q].copy(), ev[:, q].copy()
        live = (exp["null_mask"][eo] >> q) & 1 == 0
        floating = types[c] in ("double", "float") and fn in ("sum", "avg", "min", "max")
        if floating and fn in ("sum", "avg"):
            both = _is_nan(a) & _is_nan(b)
            a[both] = b[both] = NAN_BITS
        elif floating:
            b[_is_nan(b)] = NAN_BITS
        bad = np.flatnonzero((a != b) & live)
        assert bad.size == 0, (f"aggregate {q} {fn}({c}) differs in {bad.size} of {int(live.sum())} rows; first: key "
                               f"{k[bad[:4]].tolist()} rowtime {t[bad[:4]].tolist()} got "
                               f"{[hex(int(x) & (2 ** 64 - 1)) for x in a[bad[:4]]]} expected "
                               f"{[hex(int(x) & (2 ** 64 - 1)) for x in b[bad[:4]]]}")


# ---------------------------------------------------------------- the expectation
def order_key(bits):
    """Double.compare order of f64 bits as a signed integer order, NaN canonical"""
    b = np.where(_is_nan(bits), NAN_BITS, bits).astype(np.int64)
    return np.where(b < 0, b ^ LMAX, b)


def frames_of(kind, preceding, keys, ts):
    """every row's frame as positions in `order` (rows by key, row time, arrival): (order, lo, hi)"""
    n = len(keys)
    order = np.lexsort((np.arange(n), ts, keys))
    k, t = keys[order], ts[order]
    pos = np.arange(n)
    start = np.maximum.accumulate(np.where(np.r_[True, k[1:] != k[:-1]], pos, 0))
    comp = k.astype(np.float64) * 2.0 ** 40 + t     # (key, row time) as one sortable number: keys < 2^12, ts < 2^40
    if kind.endswith("rows"):
        hi = pos
        lo = np.maximum(start, pos - preceding) if kind.startswith("bounded") else start
    else:
        hi = np.searchsorted(comp, comp, "right") - 1
        lo = np.searchsorted(comp, comp - preceding, "left") if kind.startswith("bounded") else start
        lo = np.maximum(lo, start)
    return order, lo, hi


def frame_true_max(kind, preceding, keys, ts, col_f64, null):
    """{ordinal: the frame's maximum in Double.compare order as bits (canonical NaN), None over no non-null value}:
    a brute force over every row's frame (one firing, no late rows: the ordinal is the arrival index)"""
    order, lo, hi = frames_of(kind, preceding, keys, ts)
    bits = np.ascontiguousarray(col_f64, dtype=np.float64).view(np.int64)[order]
    ok = ~null[order]
    ks = np.where(ok, order_key(bits), -(1 << 63))
    out = {}
    for i in range(len(order)):
        a, b = lo[i], hi[i] + 1
        if not ok[a:b].any():
            out[int(order[i])] = None
            continue
        m = int(ks[a:b].max())
        out[int(order[i])] = m if m >= 0 else m ^ LMAX
    return out


@functools.lru_cache(maxsize=None)
def restated(variant, kind, preceding):
    """the restatement's rows (tests/over_ref.py, one final watermark) and its statistics"""
    ref = OverRef(kind, preceding, TYPES, AGGS)
    for p in pushes(variant):
        ref.process(*p)
    rows = ref.watermark(LMAX)
    return rows, ref.stats()


@functools.lru_cache(maxsize=None)
def expected(variant, kind, preceding):
    """drain_arrays()-shaped expectation: the restatement, bounded MAX replaced by the frame's true maximum (the one
    documented deviation, DESIGN 3f / 7: the reference's MAX keeps a NaN that has left the frame)"""
    rows, _ = restated(variant, kind, preceding)
    exp = rows_to_arrays(rows)
    for q in FLOAT_EXTREMES:    # a MIN / MAX that is NaN: the canonical one (Double.doubleToLongBits)
        exp["values"][_is_nan(exp["values"][:, q]), q] = NAN_BITS
    if kind.startswith("bounded"):
        keys, ts, cols, nulls, _ = stream(variant)
        for q, c in MAX_OF.items():
            true = frame_true_max(kind, preceding, keys, ts, cols[c], (nulls >> c) & 1 == 1)
            for i, o in enumerate(exp["ordinal"]):
                v = true[int(o)]
                assert (v is None) == bool((exp["null_mask"][i] >> q) & 1)
                if v is not None:
                    exp["values"][i, q] = v
    return exp


# ---------------------------------------------------------------- classes (on the restatement's output alone)
def classes(variant, kind, preceding, short_only=True):
    """How many emitted rows carry each class the stream exists for; the frames' contents come from frames_of."""
    keys, ts, cols, nulls, _ = stream(variant)
    rows, _ = restated(variant, kind, preceding)
    order, lo, hi = frames_of(kind, preceding, keys, ts)
    at = np.empty(len(order), dtype=np.int64)
    at[order] = np.arange(len(order))
    d = np.ascontiguousarray(cols[0], dtype=np.float64)
    bits = d.view(np.int64)[order]
    ok = ((nulls >> 0) & 1 == 0)[order]

    def pref(mask):
        return np.r_[0, np.cumsum(mask & ok)]
    p_nan, p_neg_nan = pref(_is_nan(bits)), pref(bits == NEG_NAN_BITS)
    p_nonfin = pref((bits & INF_BITS) == INF_BITS)
    p_pz, p_nz, p_ok = pref(bits == 0), pref(bits == NEG_ZERO_BITS), pref(np.ones(len(bits), dtype=bool))
    p_fin = pref(((bits & INF_BITS) != INF_BITS))
    out = dict.fromkeys(["sum_nan", "sum_pinf", "max_nan", "min_nz_with_pz", "max_pz_with_nz", "sum_pz_of_nz",
                         "neg_nan_in_min_frame_with_finite", "poison_outlives_row", "stale_max_nan"], 0)
    for key, _t, ordinal, vals in rows:
        if short_only and key == LONG_KEY:
            continue
        i = at[ordinal]
        a, b = lo[i], hi[i] + 1
        cnt = lambda p: int(p[b] - p[a])  # noqa: E731
        s, mn, mx = vals[Q_SUM], vals[Q_MIN], vals[Q_MAX]
        if s is None:
            continue
        out["sum_nan"] += s != s
        out["sum_pinf"] += s == np.inf
        out["max_nan"] += mx != mx
        out["min_nz_with_pz"] += double_bits(mn) == NEG_ZERO_BITS and cnt(p_pz) > 0
        out["max_pz_with_nz"] += double_bits(mx) == 0 and cnt(p_nz) > 0
        out["sum_pz_of_nz"] += double_bits(s) == 0 and cnt(p_nz) == cnt(p_ok)
        out["neg_nan_in_min_frame_with_finite"] += cnt(p_neg_nan) > 0 and cnt(p_fin) > 0
        out["poison_outlives_row"] += s != s and cnt(p_nonfin) == 0
        out["stale_max_nan"] += mx != mx and cnt(p_nan) == 0
    return {k: int(v) for k, v in out.items()}


COMMON_CLASSES = ("sum_nan", "sum_pinf", "max_nan", "min_nz_with_pz", "max_pz_with_nz", "sum_pz_of_nz",
                  "neg_nan_in_min_frame_with_finite")
BOUNDED_CLASSES = ("poison_outlives_row", "stale_max_nan")

"""What the DeltaTrigger tests share: the TopSpeedWindowing fixture, the seeded streams and configurations (a registry:
the CPU test counts what they exercise, the GPU test runs them), the schedule, and the comparison of firings."""
import json
import os
from collections import Counter

import numpy as np

from tests.delta_ref import NAN_BITS, DeltaRef

LMAX = (1 << 63) - 1
FLOATS = ("f64", "f32")
# trigger and DeltaEvictor thresholds in units of the value grid: values are m units, a unit is 2^-3 for the floating
# types (dyadic: sums and differences are exact, so a delta can equal the threshold) and 1 for the integer types
UNIT = {"i64": 1.0, "i32": 1.0, "i16": 1.0, "i8": 1.0, "f64": 0.125, "f32": 0.125}
TRIGGER_UNITS, EVICT_UNITS = 8, 12


def load_topspeed():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topspeed_windowing.json")) as f:
        d = json.load(f)
    return [tuple(r) for r in d["CAR_DATA"]], [tuple(r) for r in d["TOP_SPEEDS"]], d["threshold"], d["evictor_ms"]


def delta_stream(seed, n, keys, value_type, span=10000, jitter=700):
    """(keys, timestamps, value bits): `keys` = ("uniform", 256) or ("zipf", 64); timestamps ascend with a jitter
    (records up to 700 ms behind: late for a tumbling window even with an allowed lateness of 500); values m units
    with m in [-16, 16]; f64 streams carry NaN and +-Infinity, i32 streams values at both ends of the int range (their
    differences wrap)"""
    rng = np.random.default_rng(seed)
    kind, nk = keys
    if kind == "zipf":
        w = 1.0 / np.arange(1, nk + 1) ** 1.1
        k = rng.choice(nk, n, p=w / w.sum()).astype(np.int64) * 7919 + 13
    else:
        k = rng.integers(0, nk, n, dtype=np.int64)
    t = np.arange(n, dtype=np.int64) * span // n - rng.integers(0, jitter, n, dtype=np.int64)
    m = rng.integers(-16, 17, n, dtype=np.int64)
    if value_type in FLOATS:
        v = m.astype(np.float64) * UNIT[value_type]
        if value_type == "f64":
            r = rng.random(n)
            v[r < 0.004] = np.nan
            v[(r >= 0.004) & (r < 0.007)] = np.inf
            v[(r >= 0.007) & (r < 0.010)] = -np.inf
        return k, t, v.view(np.int64)
    if value_type == "i32":
        r = rng.random(n)
        m = np.where(r < 0.05, (1 << 31) - 1 - (m + 16), np.where(r < 0.10, -(1 << 31) + (m + 16), m))
    return k, t, m.astype(np.int64)


def ragged_cuts(seed, n, batches):
    rng = np.random.default_rng(seed + 1000)
    cuts = np.sort(rng.choice(np.arange(1, n), batches - 1, replace=False))
    return [0] + cuts.tolist() + [n]


def drive(ops, k, t, v, batches=10, bound=50, seed=0, each=None, final=(700, LMAX)):
    """ragged pushes, a watermark `bound` behind the newest timestamp after two of every three, then a jump and
    Long.MAX_VALUE"""
    cuts = ragged_cuts(seed, len(k), batches)
    wm = -10**9
    for b in range(batches):
        sl = slice(cuts[b], cuts[b + 1])
        for h in ops:
            h.process(k[sl], t[sl], v[sl].view(np.float64) if getattr(h, "wants_f64", False) else v[sl])
        wm = max(wm, int(t[sl].max()) - bound)
        if b % 3 != 1:
            for h in ops:
                h.watermark(wm)
        if each:
            each()
    for w in (wm + final[0], final[1]):
        for h in ops:
            h.watermark(w)
        if each:
            each()


def ref_of(cfg):
    """the DeltaRef of a registry configuration (thresholds in units of the value type's grid)"""
    c = dict(cfg)
    vt = c.get("value_type", "i64")
    c.pop("keys", None)
    c.pop("n", None)
    return DeltaRef(threshold=TRIGGER_UNITS * UNIT[vt], evict_threshold=EVICT_UNITS * UNIT[vt], **c)


def stream_of(i, cfg):
    return delta_stream(100 + i, cfg.get("n", 20000), cfg.get("keys", ("uniform", 256)), cfg.get("value_type", "i64"))


_T, _S, _G = dict(assigner="tumbling", size=1000), dict(assigner="sliding", size=3000, slide=1000), dict(assigner="global")
_Z, _U = ("zipf", 64), ("uniform", 256)
# shapes x lateness x purging x evictors (none, CountEvictor(4), TimeEvictor(300), DeltaEvictor; before and after) x
# value types x key distributions, every value of every axis with every shape
CONFIGS = [
    dict(_T, value_type="i64", keys=_U),
    dict(_T, value_type="i32", keys=_Z, lateness=500, purging=True, side_output=True),
    dict(_S, value_type="f64", keys=_U, lateness=500),
    dict(_S, value_type="i64", keys=_Z, purging=True, evictor="count", evict_arg=4),
    dict(_G, value_type="f64", keys=_Z),
    dict(_G, value_type="i32", keys=_U, purging=True, evictor="time", evict_arg=300),
    dict(_T, value_type="f64", keys=_U, lateness=500, side_output=True, evictor="count", evict_arg=4, evict_after=True),
    dict(_T, value_type="i64", keys=_Z, evictor="time", evict_arg=300),
    dict(_T, value_type="i32", keys=_U, lateness=500, evictor="time", evict_arg=300, evict_after=True),
    dict(_S, value_type="f64", keys=_Z, evictor="delta"),
    dict(_G, value_type="i64", keys=_U, evictor="delta", evict_after=True),
    dict(_T, value_type="i32", keys=_Z, purging=True, evictor="delta", side_output=True),
    dict(_G, value_type="f64", keys=_U, purging=True, evictor="count", evict_arg=4),
    dict(_S, value_type="i64", keys=_U, lateness=500, side_output=True, evictor="time", evict_arg=300, evict_after=True),
    dict(_T, value_type="f64", keys=_Z, lateness=500, purging=True, evictor="delta", evict_after=True),
    dict(_G, value_type="i32", keys=_Z, evictor="count", evict_arg=4, evict_after=True),
    dict(_S, value_type="i32", keys=_U, lateness=500, purging=True, side_output=True),
    # the narrow field types, smaller
    dict(_T, value_type="i16", keys=_U, n=4000, lateness=500, evictor="count", evict_arg=4),
    dict(_S, value_type="i8", keys=_Z, n=4000, purging=True),
    dict(_G, value_type="f32", keys=_U, n=4000, evictor="delta"),
]


def config_id(cfg):
    ev = cfg.get("evictor", "none") + ("-after" if cfg.get("evict_after") else "")
    return "-".join([cfg["assigner"], cfg["value_type"], cfg["keys"][0], ev] + (["purging"] if cfg.get("purging") else [])
                    + ([f"late{cfg['lateness']}"] if cfg.get("lateness") else []))


def firings(op, value_type, ordinals=True):
    """Counter of every firing: (epoch, key, start, end, count, sum, min, max[, first], contents), all as integers or
    bit patterns.  The sum of a floating field is compared as Double.doubleToLongBits gives it (every NaN the canonical
    one: the sign of the NaN that Infinity - Infinity makes is the adder's, not the program's)."""
    out = Counter()
    for r, el in op.contents():
        name = "ordinal" if "ordinal" in el.dtype.names else "ord"
        cont = (tuple(zip(el["ts"].tolist(), el["val"].tolist(), el[name].tolist())) if ordinals
                else tuple(zip(el["ts"].tolist(), el["val"].tolist())))
        s = int(r["sum"])
        if value_type in FLOATS and np.array([s], dtype=np.int64).view(np.float64)[0] != \
                np.array([s], dtype=np.int64).view(np.float64)[0]:
            s = NAN_BITS
        out[(int(r["epoch"]), int(r["key"]), int(r["start"]), int(r["end"]), int(r["count"]), s, int(r["min"]),
             int(r["max"])) + ((int(r["first"]),) if ordinals else ()) + (cont,)] += 1
    return out


def assert_same(gpu, ref, value_type, ordinals=True):
    g, r = firings(gpu, value_type, ordinals), firings(ref, value_type, ordinals)
    assert sum(g.values()) == sum(r.values()), (sum(g.values()), sum(r.values()))
    assert g == r, (list((g - r).items())[:3], list((r - g).items())[:3])

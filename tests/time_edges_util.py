"""Input classes for the event-time arithmetic (DESIGN.md "Event-time arithmetic"): streams of generate_host moved in
time, with the watermarks that go with them.  tests/test_oracle_time_edges.py guards them on the CPU (the oracle
against tests/window_ref.py, and the coverage conditions below), tests/test_gpu_time_edges.py drives them through the
GPU's paths.  Everything is compared as exact integers: values are the generator's integers (int32 range), or the
dyadic palette of tests/float_edges_util.py where a path takes a Double field, so every sum is free of its order.

* pre-epoch: timestamps from -60 size to +20 size, on and off the grid.  45 % of the records lie below
  offset - step (step = the slide, or the size of a tumbling window): displaced when off the grid, i.e.
  ts - offset + step < 0 with a negative Java remainder, where TimeWindow.getWindowStartWithOffset lands above ts and a
  sliding record gets ceil(size / slide) + 1 windows.  20 % lie in [offset - step, offset) (negative, not displaced), the
  rest from offset up.  Every 8th record is put on the grid and every 16th one next to it.  Watermarks: the largest
  timestamp so far - bound after every batch (negative, then crossing zero), then Long.MAX_VALUE.
* odd sizes: sizes 1, 3, 7, 2^k - 1, 2^k + 1, 1_000_003, 2^32 + 1, the prime 2^40 + 15, 2^61 + 1 and 2^62 + 1 (the last two
  give the reciprocal's shift l = 62 and 63), timestamps scaled to the size so that every configuration fills at least
  three windows (2^62 + 1: the two windows on either side of 0).  A pane pair keeps its timestamps at or above
  offset - slide (panes refuse displaced records).

Out of scope: timestamps, window ends or `ts - offset + size` that wrap past Long.MAX_VALUE / Long.MIN_VALUE.  No stream
here holds one (assert_no_wrap), and none is sent to the GPU.
"""
import numpy as np

from tests import window_ref as W

MAX_WM = W.LONG_MAX
H8, H24 = 8 * 3_600_000, 24 * 3_600_000
P40 = (1 << 40) + 15  # prime


def _step(cfg):
    return cfg["slide"] if cfg["assigner"] == "sliding" else cfg["gap"] if cfg["assigner"] == "session" else cfg["size"]


def _extent(cfg):
    return cfg["gap"] if cfg["assigner"] == "session" else cfg["size"]


def _raw(n, num_keys, seed):
    """keys, values and a per-record disorder in [0, 1000) from generate_host (its jitter draw)"""
    from flink_amd.datagen import generate_host
    keys, t, vals = generate_host(seed, 0, n, num_keys, ts_base=0, rate=1000 * n, jitter=1000)
    return keys, -t, vals


def _batches(keys, ts, vals, batch, bound):
    n = len(keys)
    batches, wms, mx = [], [], W.LONG_MIN
    for b in range(0, n, batch):
        sl = slice(b, min(n, b + batch))
        batches.append((keys[sl], ts[sl], vals[sl]))
        mx = max(mx, int(ts[sl].max()))
        wms.append(mx - bound)
    batches.append((keys[:0], ts[:0], vals[:0]))
    wms.append(MAX_WM)
    return batches, wms


def _snap(ts, offset, step, every=8):
    """every 8th record onto the grid at or below it, every 16th one 1 ms next to the grid (alternating sides)"""
    i = np.arange(len(ts))
    on = i % every == 0
    g = ts - np.mod(ts - offset, step)  # (floor: numpy's mod has the divisor's sign)
    near = on & (i % (2 * every) == 0)
    side = np.where(i % (4 * every) == 0, -1, 1)
    return np.where(near, g + side, np.where(on, g, ts))


def pre_epoch_stream(cfg, n=40_000, batch=5_000, num_keys=200, seed=0x7E90, disorder=1.5, bound=0.4, span=(-60, 20)):
    """[(keys, ts, values)] and watermarks of the pre-epoch class for an oracle configuration.  `disorder` and `bound`
    are in units of the size (session: the gap): records arrive up to `disorder` sizes behind the front of the stream
    and the watermark trails it by `bound` sizes, so late drops, late firings and partially late records occur; span:
    the first and last timestamp in sizes (the dense paths take a narrower one: a batch's windows must fit 8)."""
    size, step, off = _extent(cfg), _step(cfg), cfg.get("offset", 0)
    keys, dis, vals = _raw(n, num_keys, seed)
    i = np.arange(n, dtype=np.int64)
    a, b = (45 * n) // 100, (65 * n) // 100
    lo, mid0, mid1, hi = span[0] * size, off - step, off, span[1] * size
    ts = np.where(i < a, lo + (i * (mid0 - lo)) // a,
                  np.where(i < b, mid0 + ((i - a) * (mid1 - mid0)) // (b - a), mid1 + ((i - b) * (hi - mid1)) // (n - b)))
    ts = ts - (dis * np.where((i >= a) & (i < b), step // 2, int(disorder * size))) // 1000  # (the band keeps most of its own)
    ts = _snap(ts, off, step)
    return _batches(keys, ts.astype(np.int64), vals, batch, int(bound * size))


def odd_stream(cfg, n=24_000, batch=4_000, num_keys=64, seed=0x0DD5, floor=None):
    """the odd-sizes class: timestamps over [-8 size, 8 size) (narrower where that would wrap: 2^61 + 1 fills windows
    -2 .. 2, 2^62 + 1 the windows [-size, 0) and [0, size)), records up to half a size out of order, the watermark
    0.3 sizes behind.  floor = the smallest timestamp (a pane pair: offset - slide)."""
    size, step, off = _extent(cfg), _step(cfg), cfg.get("offset", 0)
    keys, dis, vals = _raw(n, num_keys, seed)
    room = W.LONG_MAX - size - (cfg["slide"] if cfg["assigner"] == "sliding" else 0) - abs(off) - 2
    lo, hi = max(-8 * size, -room), min(8 * size, room)
    if floor is not None:
        lo = max(lo, floor)
    stepn = (hi - lo) // n
    ts = [lo + i * stepn + (i * ((hi - lo) % n)) // n - (int(d) * (size // 2)) // 1000 for i, d in enumerate(dis.tolist())]
    ts = [max(t, lo) for t in ts]
    ts = np.array(ts, dtype=np.int64)
    if step < (1 << 40):
        ts = np.maximum(_snap(ts, off, step), lo)
    return _batches(keys, ts, vals, batch, (3 * size) // 10)


# ---- configurations (oracle keyword dictionaries)
# Offsets: the reference's assigners take 0 <= offset < size (slide) only (TumblingEventTimeWindows.java:53-56,
# SlidingEventTimeWindows.java:56-59), and so do the operators here.  size - 1 and 1 (the grid of -(size - 1)) are the
# extremes; TimeWindowTest's -8 h of a 24 h window has the grid of +16 h.  getWindowStartWithOffset itself is swept
# with negative offsets on the CPU (tests/test_oracle_time_edges.py).
PRE_TUMBLING = [dict(assigner="tumbling", size=1000),
                dict(assigner="tumbling", size=1000, offset=999),
                dict(assigner="tumbling", size=1000, offset=1),
                dict(assigner="tumbling", size=H24, offset=H24 - H8)]
PRE_SLIDING = [dict(assigner="sliding", size=2500, slide=1000),
               dict(assigner="sliding", size=2500, slide=1000, offset=999),
               dict(assigner="sliding", size=2500, slide=1000, offset=1),
               dict(assigner="sliding", size=2000, slide=500, lateness=300, purging=True, side_output=True)]
PRE_PANES = [dict(assigner="sliding", size=3000, slide=1000),
             dict(assigner="sliding", size=3000, slide=500, offset=1)]
PRE_SESSIONS = [dict(assigner="session", gap=300), dict(assigner="session", gap=300, lateness=200, side_output=True)]
PRE_ALL = PRE_TUMBLING + PRE_SLIDING + PRE_PANES

ODD_SIZES = [1, 3, 7, (1 << 10) - 1, (1 << 10) + 1, (1 << 20) - 1, (1 << 31) + 1, 1_000_003, (1 << 32) + 1, P40,
             (1 << 61) + 1, (1 << 62) + 1]
ODD_TUMBLING = [dict(assigner="tumbling", size=s) for s in ODD_SIZES]
ODD_PANE_PAIR = dict(assigner="sliding", size=3 * ((1 << 20) + 1), slide=(1 << 20) + 1)
ODD_NONPANE_PAIRS = [dict(assigner="sliding", size=7, slide=3), dict(assigner="sliding", size=1_000_003, slide=(1 << 17) - 1),
                     dict(assigner="sliding", size=(1 << 61) + 1, slide=(1 << 60) + 3)]


def odd_floor(cfg):
    """the pane pair's smallest timestamp: nothing displaced"""
    return cfg.get("offset", 0) - cfg["slide"] if cfg == ODD_PANE_PAIR else None


def assert_no_wrap(cfg, batches):
    """the out-of-scope class stays out: no timestamp whose ts - offset + size, ts - size or start + size wraps"""
    size, off = _extent(cfg), cfg.get("offset", 0)
    step = _step(cfg)
    slide = step if cfg["assigner"] == "sliding" else 0
    for _, ts, _ in batches:
        if len(ts) == 0:
            continue
        lo, hi = int(ts.min()), int(ts.max())
        assert W.LONG_MIN < lo - size - abs(off) and hi + size + slide + abs(off) < W.LONG_MAX, (cfg, lo, hi)


# ---- what a stream covers, by the reference arithmetic alone
def coverage(cfg, batches):
    """fractions of the records: displaced, negative but not displaced, non-negative, with the extra window"""
    step, off, size = _step(cfg), cfg.get("offset", 0), _extent(cfg)
    n = disp = neg = nonneg = extra = 0
    most = -(-size // step)
    for _, ts, _ in batches:
        for t in ts.tolist():
            n += 1
            d = W.is_displaced(t, off, step)
            disp += d
            neg += (not d) and off - step <= t < off
            nonneg += t >= 0 and t >= off
            if cfg["assigner"] == "sliding":
                extra += len(W.sliding_windows(t, size, step, off)) == most + 1
    return dict(displaced=disp / n, negative=neg / n, nonneg=nonneg / n, extra=extra / n)


def row_classes(cfg, rows, batches=None):
    """rows with a negative start, rows that straddle 0, and (with the batches) rows of windows that hold a displaced
    record -- for sliding windows: a record with the extra window"""
    out = dict(rows=len(rows), negative_start=int((rows["start"] < 0).sum()),
               straddle=int(((rows["start"] < 0) & (rows["end"] > 0)).sum()))
    if batches is not None and cfg["assigner"] != "session":
        step, off = _step(cfg), cfg.get("offset", 0)
        hit = set()
        for k, ts, _ in batches:
            for key, t in zip(k.tolist(), ts.tolist()):
                if W.is_displaced(t, off, step):
                    for s, _ in W.windows_of(cfg, t):
                        hit.add((key, s))
        out["from_displaced"] = sum((int(r["key"]), int(r["start"])) in hit for r in rows)
    return out

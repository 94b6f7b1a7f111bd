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

* the ends of the long range (WRAP_CASES, the registry tests/test_gpu_wrap_edges.py takes every stream from, vetted by
  tests/test_oracle_wrap_edges.py): 8000 records evenly over the last four steps or the first four extents of the
  range, Long.MAX_VALUE, MAX - 1, MAX - extent + 1 and MIN + 1 among them, every 8th on the grid and every 16th next to
  it, 256 keys (a tumbling assigner has one wrapped window per key; the coverage conditions ask for 200 wrapped rows),
  six batches each spread over the whole range, under a cold schedule (no watermark before Long.MAX_VALUE) and a warm
  one (MIN + 2 extents, 0, MAX - 3 extents, MAX - extent, MAX - 1, MAX); one dense stream also under a *near*
  schedule (the watermark 1.5 extents below the top from the first batch on, wrap_stream).  All arithmetic on Python
  ints.

Out of the classes: the pre-epoch and odd-size streams hold no timestamp, window end or `ts - offset + size` that wraps
(assert_no_wrap stays in force for them).  The long-range class leaves out what the reference itself does not compute:
the sliding assigner's runaway set just above Long.MIN_VALUE + size (window_ref.is_runaway), ContinuousEventTimeTrigger
streams whose timer chain would walk from the bottom of the range to the watermark (tests/continuous_ref.py
TimerRunaway), and sessions under allowed lateness at the top, whose merge function throws.  None of them is sent to
a GPU, except the runaway timestamps of the refusal test (host columns, refused before anything is queued).
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


# ---- the ends of the long range (the module docstring's third class)
MIN_TS = W.LONG_MIN
WARM = "warm"
COLD = "cold"
NEAR = "near"


def _stride(n):
    """an odd stride coprime with n: record j of the arrival order is record (j * stride) % n of the time order"""
    from math import gcd
    p = (2654435761 % n) | 1
    while gcd(p, n) != 1:
        p += 2
    return p


def wrap_timestamps(cfg, end, n):
    """n Python ints, evenly over the last (end == "top") or first (end == "bottom") four extents of the long range, in
    time order; every 8th on the grid, every 16th 1 ms next to it; the extreme timestamps themselves; no timestamp of
    the sliding assigner's runaway set (moved out of it instead)"""
    ext, step, off = _extent(cfg), _step(cfg), cfg.get("offset", 0)
    # (the top of a sliding stream: four slides, the span of the coverage conditions' uniform baseline -- 40 % of the
    # records with a wrapped window, 4.8 % with none; over four sizes of 2500 / 1000 they would be 18 % and 1.7 %)
    lo, hi = (W.LONG_MAX - 4 * min(ext, step), W.LONG_MAX) if end == "top" else (MIN_TS + 1, MIN_TS + 4 * ext)
    out = []
    for i in range(n):
        t = lo + (i * (hi - lo)) // (n - 1)
        if i % 8 == 0:
            t -= (t - off) % step  # (Python ints: the grid point at or below t)
            if i % 16 == 0:
                t += -1 if i % 32 == 0 else 1
        out.append(min(max(t, lo), hi))
    if end == "top":
        out[-1], out[-2], out[-3] = W.LONG_MAX, W.LONG_MAX - 1, W.LONG_MAX - ext + 1  # ([MAX - ext + 1, Long.MIN_VALUE))
    else:
        out[0] = MIN_TS + 1
    if cfg["assigner"] == "sliding":
        run = lambda t: W.is_runaway(t, cfg["size"], cfg["slide"], off)  # noqa: E731
        for i, t in enumerate(out):
            if run(t):  # moved above the set, or (where that leaves the range) below it, where a record has no window
                up = t + cfg["size"] + cfg["slide"]
                while up > hi or run(up):
                    up = max(lo, (t if up > t else up) - cfg["size"])
                out[i] = up
    return out


def warm_watermarks(cfg):
    ext = _extent(cfg)
    return [MIN_TS + 2 * ext, 0, W.LONG_MAX - 3 * ext, W.LONG_MAX - ext, W.LONG_MAX - 1, MAX_WM]


def wrap_stream(cfg, end, schedule, n=8000, num_keys=256, seed=0x3A9, key_base=0):
    """[(keys, ts, values)] and watermarks of the long-range class: six batches, each spread over the whole four
    extents (the arrival order is a stride permutation of the time order), so every batch meets every watermark's
    side.  The first batch, the only one a warm stream pushes before its first watermark, and the last one, which arrives
    under Long.MAX_VALUE - 1, are 3/8 of the stream each: a tumbling assigner has one wrapped window per key, which under
    a warm schedule only the first batch fills, and where that window ends at Long.MIN_VALUE only the last batch's
    records above it are late because of a wrap.
    cold: no watermark before Long.MAX_VALUE (the batches' watermark is Long.MIN_VALUE, which advances nothing: it is
    the operator's initial one).
    warm: after the batches, in turn, Long.MIN_VALUE + 2 extents, 0, Long.MAX_VALUE - 3 extents, - 1 extent, - 1,
    Long.MAX_VALUE.
    near (the dense single pass): Long.MAX_VALUE - 1.5 extents after each of the first four batches (the timestamps
    above it that the next batches keep lie in the watermark's own window: a compact window delta counts from
    2^(log_s - 1) windows below the watermark's to as many above, which is one for log_s = 1), then MAX - 1 and MAX;
    batches 2 to 5 keep only their timestamps below MAX - extent (the others arrive with the last batch), whose windows neither wrap nor lie at the other end
    of the range, so those batches are ones a narrow single pass can keep.
    All arithmetic on Python ints (numpy wraps silently)."""
    keys, _, vals = _raw(n, num_keys, seed)
    ts = wrap_timestamps(cfg, end, n)
    p = _stride(n)
    order = [(j * p) % n for j in range(n)]
    keys, vals = keys[order] + key_base, vals[order]
    ts = np.array([ts[i] for i in order], dtype=np.int64)
    nb = 6
    cuts = [0] + [(3 * n) // 8 + (n * j) // 16 for j in range(nb - 1)] + [n]
    batches = [(keys[a:b], ts[a:b], vals[a:b]) for a, b in zip(cuts, cuts[1:])]
    if schedule == NEAR:
        ext = _extent(cfg)
        for b in range(1, 5):  # (what they give up arrives with the last batch)
            k, t, v = batches[b]
            m = t < W.LONG_MAX - ext
            batches[b] = (k[m], t[m], v[m])
            batches[5] = tuple(np.concatenate([x, y[~m]]) for x, y in zip(batches[5], (k, t, v)))
        return batches, [W.LONG_MAX - ext - ext // 2] * 4 + [W.LONG_MAX - 1, MAX_WM]
    wms = warm_watermarks(cfg) if schedule == WARM else [MIN_TS] * (nb - 1) + [MAX_WM]
    return batches, wms


_W_TUMBLING = [("tumbling-o%d" % o, dict(assigner="tumbling", size=1000, offset=o)) for o in (0, 1, 999, 808)]
_W_SLIDING = [("sliding-2500-o%d" % o, dict(assigner="sliding", size=2500, slide=1000, offset=o)) for o in (0, 808, 308)]
_W_PANES = [("panes-3000-1000", dict(assigner="sliding", size=3000, slide=1000)),
            ("panes-3000-500", dict(assigner="sliding", size=3000, slide=500))]
_W_OTHER = [("sliding-700-1000", dict(assigner="sliding", size=700, slide=1000)),
            ("session", dict(assigner="session", gap=300)),
            ("session-late-side", dict(assigner="session", gap=300, lateness=200, side_output=True)),
            ("tumbling-late", dict(assigner="tumbling", size=1000, offset=808, lateness=500)),
            ("tumbling-late-purge-side", dict(assigner="tumbling", size=1000, lateness=500, purging=True, side_output=True)),
            ("sliding-late-purge-side", dict(assigner="sliding", size=2500, slide=1000, offset=308, lateness=500,
                                             purging=True, side_output=True)),
            ("tumbling-late-max", dict(assigner="tumbling", size=1000, offset=808, lateness=W.LONG_MAX)),
            ("sliding-late-max", dict(assigner="sliding", size=2500, slide=1000, lateness=W.LONG_MAX))]

# the registry: every stream of the class that a GPU test may send, by name.  tests/test_oracle_wrap_edges.py vets each
# entry on the CPU (nothing of the runaway set, the reference completes under its cap, the fired rows are bounded).
WRAP_CASES = {}
for _name, _cfg in _W_TUMBLING + _W_SLIDING + _W_PANES + _W_OTHER:
    for _end in ("top", "bottom"):
        for _sched in (COLD, WARM):
            if _name == "session-late-side" and _end == "top":
                # TimeWindow.maxTimestamp + allowedLateness wraps for a merged session that ends within the lateness of
                # Long.MAX_VALUE, and the reference's merge function then throws ("The end timestamp of an event-time
                # window cannot become earlier than the current watermark by merging"): not a stream it computes
                continue
            WRAP_CASES[f"{_name}-{_end}-{_sched}"] = dict(cfg=_cfg, end=_end, schedule=_sched, args={})
# dense tumbling regions want many keys per window (tests/test_gpu_wrap_edges.py: the single pass)
for _sched in (COLD, WARM):
    WRAP_CASES[f"dense-tumbling-top-{_sched}"] = dict(cfg=dict(assigner="tumbling", size=1000, offset=808), end="top",
                                                      schedule=_sched, args={})
WRAP_CASES["dense-tumbling-top-near"] = dict(cfg=dict(assigner="tumbling", size=1000, offset=808), end="top", schedule=NEAR,
                                            args={})
# the list operator's ContinuousEventTimeTrigger: a top stream on the grid of offset 0, whose wrapped first timers
# (ts - ts % interval + interval past Long.MAX_VALUE) belong to the window that ends at Long.MIN_VALUE + 192 and are
# followed by its cleanup timer after 6 steps; offset 808's window [MAX - 999, Long.MIN_VALUE) would walk the chain
# from the bottom of the range to Long.MAX_VALUE (excluded set 2)
WRAP_CASES["continuous-tumbling-top-cold"] = dict(cfg=dict(assigner="tumbling", size=1000), end="top", schedule=COLD,
                                                  args={}, interval=33)
WRAP_CASES["continuous-tumbling-bottom-warm"] = dict(cfg=dict(assigner="tumbling", size=1000, offset=1), end="bottom",
                                                     schedule=WARM, args={}, interval=33)


# the configurations of the class by name (the registry's entries are these at an end under a schedule), and the two
# lengths a stream is built from
WRAP_CONFIGS = dict(_W_TUMBLING + _W_SLIDING + _W_PANES + _W_OTHER)
extent, step = _extent, _step


def wrap_case(name):
    """(cfg, batches, watermarks) of a registry entry"""
    c = WRAP_CASES[name]
    batches, wms = wrap_stream(c["cfg"], c["end"], c["schedule"], **c["args"])
    return c["cfg"], batches, wms


def wrap_row_classes(rows, end):
    """rows, rows of a wrapped window (end < start), rows that end at Long.MIN_VALUE, and rows that reach the other
    end of the range from their stream's (a top stream's rows that end below 0, a bottom stream's that start above it)"""
    s, e = rows["start"], rows["end"]
    return dict(rows=len(rows), wrapped=int((e < s).sum()), end_min=int((e == MIN_TS).sum()),
                far=int((e < 0).sum() if end == "top" else (s > 0).sum()))


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

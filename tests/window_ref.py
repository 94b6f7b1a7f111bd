"""An independent restatement of the reference's event-time arithmetic, on Python's unbounded ints with one explicit
wrap to Java's long (`wrap64`).  No numpy inside the arithmetic and no call into oracle/: tests/test_oracle_time_edges.py
holds the oracle against it, tests/test_gpu_time_edges.py uses it to count what the GPU rows cover.

Paths are relative to flink-streaming-java/src/main/java/org/apache/flink/streaming/.
"""

LONG_MIN = -(1 << 63)
LONG_MAX = (1 << 63) - 1


def wrap64(x):
    """a Java long: the low 64 bits of x, two's complement"""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def jmod(a, b):
    """Java's `a % b` for longs: truncating division, the result has the dividend's sign (JLS 15.17.3)"""
    r = abs(a) % abs(b)
    return -r if a < 0 else r


def window_start(ts, offset, size):
    """TimeWindow.getWindowStartWithOffset (api/windowing/windows/TimeWindow.java:254-256)"""
    return wrap64(ts - jmod(wrap64(wrap64(ts - offset) + size), size))


def tumbling_windows(ts, size, offset=0):
    """TumblingEventTimeWindows.assignWindows (api/windowing/assigners/TumblingEventTimeWindows.java:63-75):
    [(start, end)]; Long.MIN_VALUE raises as there"""
    if ts <= LONG_MIN:
        raise ValueError("Record has Long.MIN_VALUE timestamp (= no timestamp marker).")
    s = window_start(ts, offset, size)
    return [(s, wrap64(s + size))]


class Runaway(ValueError):
    """a timestamp on which the reference's own loop does not return (sliding_windows)"""


def sliding_cap(size, slide):
    """the most windows a sliding record has, a displaced record's extra one included: ceil(size / slide) + 1"""
    return -(-size // slide) + 1


def sliding_windows(ts, size, slide, offset=0, cap=None):
    """SlidingEventTimeWindows.assignWindows (api/windowing/assigners/SlidingEventTimeWindows.java:67-81), newest first.
    The loop is evaluated for at most `cap` windows (default sliding_cap): for a timestamp just above
    Long.MIN_VALUE + size, `ts - size` does not wrap but the walk down does, past Long.MIN_VALUE to the top of the
    range, and the reference runs for about 2^64 / slide steps.  Such a timestamp is in the runaway set: Runaway."""
    if ts <= LONG_MIN:
        raise ValueError("Record has Long.MIN_VALUE timestamp (= no timestamp marker).")
    cap = sliding_cap(size, slide) if cap is None else cap
    out = []
    start = window_start(ts, offset, slide)
    lo = wrap64(ts - size)
    while start > lo:
        if len(out) == cap:
            raise Runaway(f"sliding walk of ts {ts} (size {size}, slide {slide}, offset {offset}) passes {cap} windows")
        out.append((start, wrap64(start + size)))
        start = wrap64(start - slide)
    return out


def is_runaway(ts, size, slide, offset=0):
    """ts is in the runaway set of the sliding assigner (size, slide, offset)"""
    try:
        sliding_windows(ts, size, slide, offset)
    except Runaway:
        return True
    return False


def session_window(ts, gap):
    """EventTimeSessionWindows.assignWindows (api/windowing/assigners/EventTimeSessionWindows.java:59-61)"""
    return [(ts, wrap64(ts + gap))]


def merge_sessions(windows):
    """TimeWindow.mergeWindows (api/windowing/windows/TimeWindow.java:201-245): the windows sorted by start, each
    merged into the current one while they intersect (start <= other.end and end >= other.start, :117-119) -> the
    covers (:124-126)"""
    out = []
    for s, e in sorted(windows):
        if out and out[-1][0] <= e and out[-1][1] >= s:
            out[-1] = (min(out[-1][0], s), max(out[-1][1], e))
        else:
            out.append((s, e))
    return out


def max_timestamp(end):
    """TimeWindow.maxTimestamp (api/windowing/windows/TimeWindow.java:83-85)"""
    return wrap64(end - 1)


def cleanup_time(end, lateness):
    """WindowOperator.cleanupTime (runtime/operators/windowing/WindowOperator.java:637-644), event time"""
    mx = max_timestamp(end)
    c = wrap64(mx + lateness)
    return c if c >= mx else LONG_MAX


def is_window_late(end, lateness, watermark):
    """WindowOperator.isWindowLate (runtime/operators/windowing/WindowOperator.java:576-578)"""
    return cleanup_time(end, lateness) <= watermark


def is_element_late(ts, lateness, watermark):
    """WindowOperator.isElementLate (runtime/operators/windowing/WindowOperator.java:586-589)"""
    return wrap64(ts + lateness) <= watermark


def continuous_next_fire(ts, interval):
    """ContinuousEventTimeTrigger.onElement's first timer (api/windowing/triggers/ContinuousEventTimeTrigger.java:64-65):
    timestamp - (timestamp % interval) + interval"""
    return wrap64(wrap64(ts - jmod(ts, interval)) + interval)


# ---- the classes the time-edge tests count (DESIGN.md "Event-time arithmetic")
def is_displaced(ts, offset, step):
    """ts - offset + step < 0 off the grid: Java's % leaves a negative remainder, the start lands above ts"""
    t = ts - offset + step
    return t < 0 and t % step != 0


def windows_of(cfg, ts):
    """[(start, end)] of a record under an oracle configuration dict (assigner, size, slide, offset, gap)"""
    a = cfg["assigner"]
    if a == "tumbling":
        return tumbling_windows(ts, cfg["size"], cfg.get("offset", 0))
    if a == "sliding":
        return sliding_windows(ts, cfg["size"], cfg["slide"], cfg.get("offset", 0))
    return session_window(ts, cfg["gap"])

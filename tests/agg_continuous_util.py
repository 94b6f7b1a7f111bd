"""Configurations and streams of the ContinuousEventTimeTrigger tests of the aggregating operator
(tests/test_gpu_agg_continuous.py runs them on the GPU, tests/test_agg_continuous_abi.py vets them with ContinuousRef
alone).  The checker is tests/continuous_ref.ContinuousRef(trigger="continuous", evictor="none"): its rows'
(key, start, end, count, sum, min, max) are what an aggregating state holds."""
import numpy as np

from tests.continuous_ref import ContinuousRef, seeded_stream

LMAX = (1 << 63) - 1

# seeded parity, over seeded_stream(seed, 20000, 37, 2000, 150) driven by continuous_ref.drive
SEEDED_CONFIGS = [
    dict(assigner="tumbling", size=100, interval=11),  # the windows k = 0, 11 meet maxTimestamp and stop there
    dict(assigner="tumbling", size=100, lateness=50, purging=True, side_output=True, interval=33),
    dict(assigner="sliding", size=100, slide=25, lateness=40, interval=33),
    dict(assigner="sliding", size=100, slide=25, lateness=0, interval=33),  # (the shape that would be panes)
    dict(assigner="sliding", size=100, slide=30, offset=7, interval=13),
    dict(assigner="tumbling", size=100, offset=41, interval=250),  # the interval exceeds the size
    dict(assigner="tumbling", size=50, interval=1),
]
SEEDED_IDS = ["tumbling-i11", "tumbling-late-purging-side-i33", "sliding-late-i33", "sliding-panes-shape-i33",
              "sliding-offset-i13", "tumbling-offset-i250", "tumbling-i1"]
VALUE_TYPES = ["long", "int", "double"]
GROWTH_CONFIG = dict(assigner="tumbling", size=50, lateness=20, interval=20)
# (8 key groups of one region each: 8 regions of 256 slots for about 10^4 live windows, so the table grows, by
# suspended pushes among other ways)
GROWTH_GPU_KW = dict(expected_entries=1024, max_parallelism=8, sub_partitions=1)
# (interval 11: the window [0, 100) meets its maxTimestamp with a fire time and stops there; the allowed lateness
# keeps it, stuck, past the snapshot's watermark)
SNAPSHOT_CONFIGS = [dict(assigner="tumbling", size=100, lateness=1000, interval=11),
                    dict(assigner="tumbling", size=100, lateness=1000, purging=True, interval=11)]
LIMIT_CONFIG = dict(assigner="tumbling", size=1 << 40, interval=1)
RANGE_CONFIG = dict(assigner="tumbling", size=100, interval=40)


def seed_of(cfg):
    return 7 + len(str(cfg))


def values_of(v, value_type):
    """the value column of a stream for a field type (what the GPU operator is pushed), and the same as the int64 /
    f64-bit column ContinuousRef takes:
      long    the stream's values;
      int     values around +-2^30, so a window's sum leaves 32 bits (the GPU sum wraps, SumFunction.IntSum);
      double  non-zero dyadic values m * 2^-3, |m| <= 1000: every partial sum is exact, so the sum's bits are the same
              whatever order they are added in"""
    if value_type == "int":
        w = np.where(v % 2 == 0, 1, -1).astype(np.int64) * ((1 << 30) + np.abs(v))
        return w, w
    if value_type == "double":
        m = np.where(v == 0, 1000, v).astype(np.float64) / 8.0
        return m, m.view(np.int64)
    return v, v


def ref_of(value_type="long", **cfg):
    return ContinuousRef(trigger="continuous", evictor="none", value_type="f64" if value_type == "double" else "i64",
                         **cfg)


def wrap32(x):
    """a Java int's value of the low 32 bits"""
    return (int(x) + (1 << 31)) % (1 << 32) - (1 << 31)


def ref_rows(ref, value_type="long"):
    """ContinuousRef's rows as (epoch, key, start, end, count, sum, min, max), the sum in the field's width"""
    out = []
    for r in ref.rows():
        s = wrap32(r["sum"]) if value_type == "int" else int(r["sum"])
        out.append((int(r["epoch"]), int(r["key"]), int(r["start"]), int(r["end"]), int(r["count"]), s, int(r["min"]),
                    int(r["max"])))
    return sorted(out)


def split_stream(interval=250, size=100000):
    """One push, two keys.  (key 1, window [0, size)) receives more than three times FW_AGG_CHUNK = 32768 records, so
    its partition is split over several aggregate workgroups; record 0 of the push belongs to it and lies several
    intervals later than most of the others, and the smallest timestamp is not at the front either: arming from any
    record but the first arrived gives other fire times."""
    n = 120000
    rng = np.random.default_rng(5)
    k = np.where(np.arange(n) % 12 == 11, 2, 1).astype(np.int64)
    t = rng.integers(10, 3 * interval, n, dtype=np.int64)
    t[0] = 9 * interval + 17  # the arming element of (1, [0, size)): fire = 10 * interval
    t[1] = 3  # the smallest timestamp, second to arrive
    k[0] = k[1] = 1
    first2 = int(np.flatnonzero(k == 2)[0])
    t[first2] = 5 * interval + 1  # key 2 is armed from its own first record: fire = 6 * interval
    v = rng.integers(-1000, 1000, n, dtype=np.int64)
    assert size > 10 * interval and int((k == 1).sum()) > 3 * 32768
    return k, t, v


def device_stream():
    """two pushes of the seeded stream, for the device-column test"""
    k, t, v = seeded_stream(11, 20000, 37, 2000, 150)
    h = 10000
    return (k[:h], t[:h], v[:h]), (k[h:], t[h:], v[h:]), int(t.max()) - 100


def growth_stream():
    return seeded_stream(31, 100000, 3000, 50000, 60)


def snapshot_stream():
    k, t, v = seeded_stream(21, 20000, 200, 2000, 60)
    h = 10000
    return k, t, v, h, int(t[:h].max()) - 70

"""Configurations, streams and checkers of the CountTrigger tests of the aggregating operator
(tests/test_gpu_agg_count_trigger.py runs them on the GPU, tests/test_agg_count_trigger_abi.py vets them on the CPU).
The reference is the pinned ListWindowOracle(trigger="count", evictor="none"): with no evictor its row over a firing's
list is the accumulator at that element.  tests/count_trigger_ref.CountTriggerRef restates the rules for what the oracle
cannot express (restored counts) and is itself held to the oracle on every stream used here."""
import numpy as np

from oracle import oracle as orc
from tests.continuous_ref import seeded_stream, zipf_stream
from tests.count_trigger_ref import CountTriggerRef

BIG = 10 ** 6  # no row ever; the state is still cleaned


def _c(assigner, size, slide=0, offset=0, lateness=0, n=1, purging=False, side_output=False):
    return dict(assigner=assigner, size=size, slide=slide, offset=offset, lateness=lateness, n=n, purging=purging,
                side_output=side_output)


# over seeded_stream(seed, 20000, 37, 2000, 150) driven by continuous_ref.drive: tumbling 100 and 97 with offset 13,
# sliding 300/100 and 250/100 (size % slide != 0, 4 windows per record with the displaced one); n in {1, 2, 3, 7, 10^6};
# lateness 0 and 150; purging and side output on and off
CONFIGS = [
    _c("tumbling", 100, n=1, side_output=True),
    _c("tumbling", 100, n=2, lateness=150, purging=True, side_output=True),
    _c("tumbling", 100, n=3, purging=True),
    _c("tumbling", 100, n=7, lateness=150),
    _c("tumbling", 97, offset=13, n=2, lateness=150, side_output=True),
    _c("tumbling", 97, offset=13, n=7, purging=True),
    _c("tumbling", 100, n=BIG, lateness=150),
    _c("sliding", 300, 100, n=1),
    _c("sliding", 300, 100, n=2, purging=True),
    _c("sliding", 300, 100, n=3, lateness=150, purging=True, side_output=True),
    _c("sliding", 300, 100, n=7),
    _c("sliding", 250, 100, n=2, lateness=150),
    _c("sliding", 250, 100, n=7, lateness=150, purging=True, side_output=True),
    _c("sliding", 250, 100, n=BIG),
]


def cfg_id(c):
    return (f"{c['assigner'][:4]}{c['size']}" + (f"-{c['slide']}" if c["slide"] else "") +
            (f"+{c['offset']}" if c["offset"] else "") + f"-n{c['n']}-l{c['lateness']}" +
            ("-purge" if c["purging"] else "") + ("-side" if c["side_output"] else ""))


IDS = [cfg_id(c) for c in CONFIGS]
VALUE_TYPES = ["long", "int", "double"]
DEVICE_CONFIGS = [CONFIGS[1], CONFIGS[9], CONFIGS[11]]
SNAPSHOT_CONFIGS = [_c("tumbling", 100, n=3, lateness=1000), _c("tumbling", 100, n=3, lateness=1000, purging=True),
                    _c("sliding", 250, 100, n=2, lateness=1000, purging=True)]


# timestamps at the ends of the long range: one time_edges_util.WRAP_CASES configuration at each end, warm schedule
WRAP_NAMES = ["tumbling-o999-top-warm", "sliding-2500-o808-bottom-warm"]


def wrap_cfg(cfg, n=3):
    return dict(assigner=cfg["assigner"], size=cfg["size"], slide=cfg.get("slide", 0), offset=cfg.get("offset", 0),
                lateness=cfg.get("lateness", 0), n=n, purging=cfg.get("purging", False),
                side_output=cfg.get("side_output", False))


SEED = 33  # (a seed whose disorder reaches every class: late records at lateness 0, firings behind the watermark)


def stream_of(cfg):
    """the configuration's stream: the seeded one, Zipf keys for every third configuration"""
    if cfg in CONFIGS and CONFIGS.index(cfg) % 3 == 2:
        return zipf_stream(SEED, 20000, 37, 2000, 150)
    return seeded_stream(SEED, 20000, 37, 2000, 150)


def values_of(v, value_type):
    """the value column for a field type as the GPU operator is pushed it, and as the int64 / f64-bit column the
    references take:
      long    the stream's values;
      int     values near +-2^31 / 2, so two elements' sum leaves 32 bits (the sum wraps, SumFunction.IntSum);
      double  non-zero dyadic values m / 8, |m| <= 1000: every partial sum is exact, so the sum's bits do not depend on
              the order of the additions (DESIGN §2's bar, at its exact end), and no window is made of -0.0 alone"""
    if value_type == "int":
        w = np.where(v % 2 == 0, 1, -1).astype(np.int64) * ((1 << 30) + np.abs(v))
        return w, w
    if value_type in ("double", "float"):  # (float: |sums| * 8 stay below 2^24, so FloatSum's roundings are exact too)
        m = np.where(v == 0, 1000, v).astype(np.float64) / 8.0
        return m, m.view(np.int64)
    if value_type == "short":  # near +-2^15 / 2: two elements' sum leaves 16 bits (ShortSum)
        w = np.where(v % 2 == 0, 1, -1).astype(np.int64) * ((1 << 14) + np.abs(v))
        return w, w
    if value_type == "byte":  # near +-2^7 / 2 (ByteSum)
        w = np.where(v % 2 == 0, 1, -1).astype(np.int64) * ((1 << 6) + np.abs(v) % 60)
        return w, w
    return v, v


_OVT = {"long": "i64", "int": "i32", "double": "f64", "short": "i16", "byte": "i8", "float": "f32"}
_WRAP = {"int": 32, "short": 16, "byte": 8}
NARROW_TYPES = ["float", "short", "byte"]


def wrap_bits(x, bits):
    """a Java int / short / byte's value of the low bits"""
    return (int(x) + (1 << (bits - 1))) % (1 << bits) - (1 << (bits - 1))


class Oracle:
    """ListWindowOracle under CountTrigger in the harness shape of continuous_ref.drive"""

    def __init__(self, value_type="long", **cfg):
        self.ref = orc.ListWindowOracle(assigner=cfg["assigner"], size=cfg["size"], slide=cfg["slide"],
                                        offset=cfg["offset"], lateness=cfg["lateness"], trigger="count",
                                        trigger_count=cfg["n"], purging=cfg["purging"], evictor="none",
                                        side_output=cfg["side_output"], value_type=_OVT[value_type])
        self.value_type = value_type
        self.epoch = 0

    def process(self, k, t, v):
        self.ref.process(k, t, values_of(np.asarray(v), self.value_type)[1])

    def watermark(self, wm):
        self.ref.watermark(wm)
        self.epoch += 1

    def row_tuples(self):
        out = []
        for r in self.ref.rows():
            s = wrap_bits(r["sum"], _WRAP[self.value_type]) if self.value_type in _WRAP else int(r["sum"])
            out.append((int(r["epoch"]), int(r["key"]), int(r["start"]), int(r["end"]), int(r["count"]), s,
                        int(r["min"]), int(r["max"])))
        return sorted(out)

    def side_tuples(self):
        k, t, v, e = self.ref.side_rows()  # (oracle_list_get_side_rows: key, ts, val, epoch)
        return sorted(zip(e.tolist(), k.tolist(), t.tolist(), v.tolist()))

    @property
    def late_dropped(self):
        return self.ref.late_dropped

    @property
    def num_state_entries(self):
        return self.ref.num_state_entries

    @property
    def num_timers(self):
        return self.ref.num_timers


class Restated:
    """CountTriggerRef in the same shape; it also counts the classes of the vetting: firings from a carried count,
    windows cleaned up with 0 < count < n, firings of windows behind the watermark, side-output records"""

    def __init__(self, value_type="long", **cfg):
        self.ref = CountTriggerRef(value_type=value_type, **cfg)
        self.value_type = value_type
        self.carried = self.leftover = self.behind = 0

    def process(self, k, t, v):
        r = self.ref
        before = {kw: a[4] for kw, a in r.state.items()}
        n0 = len(r._rows)
        r.process(np.asarray(k), np.asarray(t), values_of(np.asarray(v), self.value_type)[1])
        seen = set()
        for row in r._rows[n0:]:
            kw = (row[1], row[2])
            if kw not in seen and before.get(kw, 0) > 0:
                self.carried += 1
            seen.add(kw)
            if row[3] - 1 <= r.wm:
                self.behind += 1

    def watermark(self, wm):
        r = self.ref
        self.leftover += sum(1 for kw, a in r.state.items() if r._cleanup(kw[1]) <= wm and 0 < a[4] < r.n)
        r.watermark(wm)

    @property
    def epoch(self):
        return self.ref.epoch

    def row_tuples(self):
        return self.ref.rows()

    def side_tuples(self):
        return self.ref.side_rows()

    @property
    def late_dropped(self):
        return self.ref.late_dropped

    @property
    def num_state_entries(self):
        return self.ref.num_state_entries

    @property
    def num_timers(self):
        return self.ref.num_timers


def hot_stream(keys=1):
    """3 * 32768 + 17 records of `keys` alternating keys in one tumbling window [0, 10^6), one push: a group longer than
    a scan chunk, a workgroup's step and a hot partition's 32768-record chunk"""
    n = 3 * 32768 + 17
    k = (np.arange(n, dtype=np.int64) % keys) * 1009 + 7
    t = (np.arange(n, dtype=np.int64) * 7919) % 1000000
    v = np.arange(n, dtype=np.int64) % 2001 - 1000
    return k, t, v


def hot_expected(k, v, n_fire, purging, size=1000000):
    """the closed form of hot_stream's rows: per key its values in arrival order, a row at every n-th; prefix sums,
    running min / max (restarted behind each row under purging)"""
    rows = []
    for key in np.unique(k):
        x = v[k == key]
        rs = np.arange(n_fire, len(x) + 1, n_fire)
        if purging:
            b = x[:len(rs) * n_fire].reshape(-1, n_fire)
            cnt, sm, mn, mx = np.full(len(rs), n_fire), b.sum(1), b.min(1), b.max(1)
        else:
            cnt, sm = rs, np.cumsum(x)[rs - 1]
            mn, mx = np.minimum.accumulate(x)[rs - 1], np.maximum.accumulate(x)[rs - 1]
        rows += [(0, int(key), 0, size, int(c), int(a), int(lo), int(hi)) for c, a, lo, hi in zip(cnt, sm, mn, mx)]
    return sorted(rows)

"""Streams for the narrow-keyed dense table (k_dn_aggregate, fw_device.hip) and a host mirror of what each of them
puts into every region: plain numpy, no GPU.  tests/test_dn_streams.py pins the builders' premises on the CPU;
tests/test_gpu_dn_edges.py runs the streams on the GPU and asserts rows and the exact push_resumptions of every push.

The configuration the streams share ("P16"): one key group (max_parallelism=1), sub_partitions=16 (log_s = 4, so
ndn0 = 8 and the narrow deltas 0..7 are the compact deltas 8..15: all eight exist, delta 0 is the watermark's
window), expected_entries=65536 (R = 8192 entries a region), max_batch=2^19 (a narrow run holds 2 rcap = 131072
records).  "P32" is the same with sub_partitions=32 (log_s = 5, ndn0 = 16: narrow deltas 8..15 have a compact form)."""
import re
import os
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_WM = (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
KEY_MIN, KEY_MAX = -(1 << 28), (1 << 28) - 1  # narrow keys
SIZE = 1000
WM0 = 10 * SIZE + 10  # the lone first watermark: its window, [10000, 11000), is narrow delta 0
NW_DBITS = 3
DN_EMPTY = 0xFFFFFFFF
SUB_SALT = 0x5851F42D4C957F2D
MAX_BATCH = 1 << 19
BOUNDS = {"long": (I32_MIN, I32_MAX), "int": (I32_MIN, I32_MAX), "short": (-(1 << 15), (1 << 15) - 1),
          "byte": (-128, 127)}  # (a narrow value is an int32, whatever the field)
BITS = {"long": 64, "int": 32, "short": 16, "byte": 8}
ORACLE_VT = {"long": "i64", "int": "i32", "short": "i16", "byte": "i8"}
STATE_DTYPE = np.dtype([(f, "<i8") for f in ("key", "start", "end", "count", "sum", "min", "max", "timer")])
ROW_DTYPE = np.dtype([(f, "<i8") for f in ("key", "start", "end", "count", "sum", "min", "max", "epoch")])


def kernel_shape():
    """(NT, NS, RPT, EPT, ND) of the k_dn_aggregate instantiation that launch_aggregate starts, read from the
    sources so that the lengths and limits below follow a retune."""
    with open(os.path.join(ROOT, "flink_amd", "csrc", "fw_device.hip")) as f:
        m = re.search(r"FW_LAUNCH_MAIN\(\(k_dn_aggregate<(\d+), (\d+), (\d+), (\d+), \d+>\)", f.read())
    with open(os.path.join(ROOT, "flink_amd", "csrc", "fw_internal.h")) as f:
        d = re.search(r"#define FW_DT_NDEPTH (\d+)", f.read())
    nt, ns, rpt, ept = (int(x) for x in m.groups())
    return nt, ns, rpt, ept, max(1, int(d.group(1)))


NT, NS, RPT, EPT, ND = kernel_shape()
RS = NT * RPT          # records of a round
ENTRY_MAX = EPT * NT   # entries the threads' registers hold
LIMIT = NS * 15 // 16  # fill limit of the LDS table
RUN_MAX = 65535        # the packed accumulator's count field


# ---------------------------------------------------------------- the region mirror
def fmix64(x):
    x = np.asarray(x, dtype=np.uint64).copy()
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xFF51AFD7ED558CCD)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xC4CEB9FE1A85EC53)
    x ^= x >> np.uint64(33)
    return x


def region_of(keys, log_s=4):
    """partition_of for one key group: the top log_s bits of fmix64(key ^ SUB_SALT)."""
    k = np.asarray(keys, dtype=np.int64).view(np.uint64)
    with np.errstate(over="ignore"):
        return (fmix64(k ^ np.uint64(SUB_SALT)) >> np.uint64(64 - log_s)).astype(np.int64)


def keys_in(r, n, log_s=4, first=1, inside=True):
    """the first n keys >= first whose region is r (inside=False: is not r)"""
    c = np.arange(first, first + (n + 64) * (1 << log_s) * 4, dtype=np.int64)
    hit = region_of(c, log_s) == r
    out = c[hit if inside else ~hit][:n]
    assert len(out) == n
    return out


def narrow_id(keys, dn):
    return ((np.asarray(keys, dtype=np.int64) << NW_DBITS) | np.asarray(dn, dtype=np.int64)).astype(np.uint32)


def ts_in(dn, wm=WM0, size=SIZE):
    """a timestamp inside the window dn windows after the watermark's, varied inside the window"""
    dn = np.asarray(dn, dtype=np.int64)
    return (wm // size + dn) * size + 100 + (np.arange(dn.size, dtype=np.int64).reshape(dn.shape) * 37) % 800


@dataclass
class Stream:
    name: str
    steps: list            # (keys, ts, values, watermark); keys None = the watermark alone
    deltas: list           # expected push_resumptions delta of every step
    vt: str = "long"
    sub_partitions: int = 16
    expected_entries: int = 65536
    r: int = -1            # the region the stream aims at
    premises: dict = field(default_factory=dict)  # step -> {"run": , "new": , "live": } of region r
    ids: tuple = ()        # narrow ids that must occur among the stream's records
    wide: dict = field(default_factory=dict)      # step -> records that are meant to have no narrow form
    pre: list = None       # restored streams: the steps of the operator whose snapshot is edited ...
    edit: object = None    # ... and the edit, rows -> rows (sorted by key, start beforehand)

    @property
    def log_s(self):
        return self.sub_partitions.bit_length() - 1

    @property
    def P(self):
        return self.sub_partitions

    def op_kwargs(self):
        return dict(max_parallelism=1, sub_partitions=self.sub_partitions, expected_entries=self.expected_entries,
                    max_batch=MAX_BATCH)


def _wrap(x, bits):
    x = int(x) & ((1 << bits) - 1)
    return x - (1 << bits) if x >> (bits - 1) else x


class Exact:
    """Running (count, sum, min, max) of every live (key, window) in Python ints; fired rows' sums wrap at the
    field's width (SumFunction's IntSum / ShortSum / ByteSum), state sums at 64 bits."""

    def __init__(self, size=SIZE, bits=64):
        self.size, self.bits, self.wm, self.g = size, bits, -(1 << 63), {}

    def restore(self, rows):
        for x in rows:
            self.g[(int(x["key"]), int(x["start"]))] = [int(x["count"]), int(x["sum"]), int(x["min"]), int(x["max"])]

    def push(self, k, t, v):
        k, t, v = (np.asarray(x, dtype=np.int64) for x in (k, t, v))
        st = t - t % self.size  # (floor: numpy's % takes the divisor's sign)
        keep = st + self.size - 1 > self.wm  # WindowOperator.isWindowLate, lateness 0
        k, st, v = k[keep], st[keep], v[keep]
        grp, inv = np.unique(np.stack([k, st], axis=1), axis=0, return_inverse=True)
        inv = inv.ravel()
        n = len(grp)
        cnt, sm = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        mn, mx = np.full(n, MAX_WM, dtype=np.int64), np.full(n, -MAX_WM - 1, dtype=np.int64)
        np.add.at(cnt, inv, 1)
        np.add.at(sm, inv, v)  # (exact: a push's |sum| < 2^19 2^31)
        np.minimum.at(mn, inv, v)
        np.maximum.at(mx, inv, v)
        for i in range(n):
            a = self.g.setdefault((int(grp[i, 0]), int(grp[i, 1])), [0, 0, MAX_WM, -MAX_WM - 1])
            a[0] += int(cnt[i])
            a[1] += int(sm[i])
            a[2], a[3] = min(a[2], int(mn[i])), max(a[3], int(mx[i]))

    def watermark(self, wm, epoch):
        self.wm = max(self.wm, wm)
        due = sorted(kw for kw in self.g if kw[1] + self.size - 1 <= self.wm)
        out = np.zeros(len(due), dtype=ROW_DTYPE)
        for i, kw in enumerate(due):
            c, s, mn, mx = self.g.pop(kw)
            out[i] = (kw[0], kw[1], kw[1] + self.size, c, _wrap(_wrap(s, 64), self.bits), mn, mx, epoch)
        return out

    def live(self):
        out = np.zeros(len(self.g), dtype=STATE_DTYPE)
        for i, kw in enumerate(sorted(self.g)):
            c, s, mn, mx = self.g[kw]
            out[i] = (kw[0], kw[1], kw[1] + self.size, c, _wrap(s, 64), mn, mx, 1)  # (timer: EventTimeTrigger's is set)
        return out


def exact_rows(s, restored=None):
    ex = Exact(SIZE, BITS[s.vt])
    if restored is not None:
        ex.restore(restored)
    out = []
    for e, (k, t, v, wm) in enumerate(s.steps):
        if k is not None:
            ex.push(k, t, v)
        out.append(ex.watermark(wm, e))
    return np.concatenate(out)


def sort_state(rows):
    return rows[np.lexsort((rows["start"], rows["key"]))]


def mirror(s, restored=None):
    """What every step of the stream puts into every region: per step {"run": records of each region's run, "new":
    (key, window) groups the push adds to each region, "live": each region's entries after the push, "narrow":
    whether each record has a narrow form against the watermark in effect, "ids": the records' narrow ids (of the
    narrow ones), "entry_ids": ids of the entries each region held before the push (None: no narrow id)}."""
    P, log_s, ndn0 = s.P, s.log_s, s.P // 2
    wm, live, out = -(1 << 63), [set() for _ in range(P)], []
    if restored is not None:
        for x in restored:
            live[int(region_of([x["key"]], log_s)[0])].add((int(x["key"]), int(x["start"])))
    lo, hi = BOUNDS[s.vt]
    for k, t, v, w in s.steps:
        m = None
        if k is not None:
            k, t, v = (np.asarray(x, dtype=np.int64) for x in (k, t, v))
            assert len(k) <= MAX_BATCH and v.min() >= lo and v.max() <= hi
            st = t - t % SIZE
            ontime = st + SIZE - 1 > wm
            assert ontime.all(), "the streams carry no late record"
            dn = st // SIZE - wm // SIZE if wm > -(1 << 62) else np.full(len(k), -1, dtype=np.int64)
            compact = (dn + ndn0 >= 0) & (dn + ndn0 < P)
            nar = (dn >= 0) & (dn < 8) & (k >= KEY_MIN) & (k <= KEY_MAX) & (v >= I32_MIN) & (v <= I32_MAX)
            reg = region_of(k, log_s)
            m = {"run": np.bincount(reg, minlength=P), "narrow": nar, "compact": compact,
                 "ids": narrow_id(k[nar], dn[nar]), "new": np.zeros(P, dtype=np.int64), "entry_ids": []}
            for p in range(P):
                ids = []
                for (ek, es) in live[p]:
                    d = es // SIZE - wm // SIZE
                    ids.append(int(narrow_id([ek], [d])[0]) if 0 <= d < 8 and KEY_MIN <= ek <= KEY_MAX else None)
                m["entry_ids"].append(ids)
            for p, kk, ss in zip(reg.tolist(), k.tolist(), st.tolist()):
                if (kk, ss) not in live[p]:
                    live[p].add((kk, ss))
                    m["new"][p] += 1
            m["live"] = np.array([len(x) for x in live])
        wm = max(wm, w)
        for p in range(P):
            live[p] = {kw for kw in live[p] if kw[1] + SIZE - 1 > wm}
        out.append(m)
    return out


# ---------------------------------------------------------------- builders
def _shuffled(rng, *cols):
    o = rng.permutation(len(cols[0]))
    return tuple(c[o] for c in cols)


def _records(keys, dn, vals, wm=WM0):
    keys, dn, vals = (np.ascontiguousarray(x, dtype=np.int64) for x in (keys, dn, vals))
    return keys, ts_in(dn, wm), vals


def _grid(keys, n=None):
    """(keys, dn) of the first n (key, window) pairs, window-minor: keys x the eight narrow windows"""
    k = np.repeat(np.asarray(keys, dtype=np.int64), 8)
    d = np.tile(np.arange(8, dtype=np.int64), len(keys))
    return (k, d) if n is None else (k[:n], d[:n])


def _vals(rng, n, vt="long"):
    lo, hi = BOUNDS[vt]
    return rng.integers(lo, hi, n, endpoint=True).astype(np.int64)


def _filler(rng, r, n, log_s=4, pool=60):
    """n records for the regions other than r"""
    ks = keys_in(r, pool, log_s, first=1000, inside=False)
    return _records(ks[rng.integers(0, pool, n)], rng.integers(0, 8, n), _vals(rng, n))


def _cat(a, b):
    return tuple(np.concatenate([x, y]) for x, y in zip(a, b))


def round_lengths():
    return [1, 2, 3, RS - 1, RS, RS + 1, ND * RS - 1, ND * RS, ND * RS + 1, 3 * RS + 1, 2 * ND * RS,
            RUN_MAX - 1, RUN_MAX, RUN_MAX + 1]


def stream_rounds(r=5):
    """(a) region r's run lengths around the ring's rounds and the count field, 64 ids with independent random
    int32 values, the watermark unchanged; every second push also carries 300 records for the other regions."""
    rng = np.random.default_rng(0xA11CE)
    K = keys_in(r, 8)
    steps, deltas, prem, seen = [(None, None, None, WM0)], [0], {}, set()
    for i, n in enumerate(round_lengths()):
        rec = _records(K[rng.integers(0, 8, n)], rng.integers(0, 8, n), _vals(rng, n))
        before = len(seen)
        seen |= set(zip(rec[0].tolist(), (rec[1] // SIZE).tolist()))
        if i % 2:
            rec = _shuffled(rng, *_cat(rec, _filler(rng, r, 300)))
        steps.append(rec + (WM0,))
        deltas.append(1 if n > RUN_MAX else 0)
        prem[i + 1] = {"run": n, "new": len(seen) - before, "live": len(seen)}
    steps.append((None, None, None, MAX_WM))
    deltas.append(0)
    assert len(seen) == 64
    return Stream("rounds", steps, deltas, r=r, premises=prem)


def stream_claims(r=9):
    """(b) 3000 new ids of region r in one push into an empty table, each three times in adjacent records, so that
    lanes of one wave lose the CAS to the same id.  (Tickets in flight: at most three per unclaimed id and one per
    thread, so fill stays below c + min(NT, 3 (3000 - c)) <= 3683 < LIMIT with c ids claimed: no spurious refusal.)"""
    rng = np.random.default_rng(0xB0B)
    k, d = _grid(keys_in(r, 375))
    k, d = np.repeat(k, 3), np.repeat(d, 3)
    steps = [(None, None, None, WM0), _records(k, d, _vals(rng, len(k))) + (WM0 + 1,), (None, None, None, MAX_WM)]
    return Stream("claims", steps, [0, 0, 0], r=r, premises={1: {"run": 9000, "new": 3000, "live": 3000}})


def stream_entries(r=3):
    """(c) live = EPT NT is taken, one more is refused: EPT NT new groups, the same ids again, one new id (the
    read-in holds exactly EPT NT entries), then a record for an existing id (EPT NT + 1 entries: refused)."""
    rng = np.random.default_rng(0xC0)
    k, d = _grid(keys_in(r, ENTRY_MAX // 8 + 1))
    n = ENTRY_MAX
    steps = [(None, None, None, WM0),
             _records(k[:n], d[:n], _vals(rng, n)) + (WM0 + 1,),
             _records(k[:n], d[:n], _vals(rng, n)) + (WM0 + 2,),
             _records(k[n:n + 1], d[n:n + 1], _vals(rng, 1)) + (WM0 + 3,),
             _records(k[:1], d[:1], _vals(rng, 1)) + (WM0 + 4,),
             (None, None, None, MAX_WM)]
    prem = {1: {"run": n, "new": n, "live": n}, 2: {"run": n, "new": 0, "live": n},
            3: {"run": 1, "new": 1, "live": n + 1}, 4: {"run": 1, "new": 0, "live": n + 1}}
    return Stream("entries", steps, [0, 0, 0, 0, 1, 0], r=r, premises=prem)


def stream_fill(n, r=12):
    """(c) n new groups, one record each, into an empty region r: LIMIT are taken, LIMIT + 1 are refused (unique
    ids: a ticket is only ever held for an unclaimed id, so fill never exceeds the number of ids)."""
    rng = np.random.default_rng(0xF1 + n)
    k, d = _grid(keys_in(r, n // 8 + 1), n)
    steps = [(None, None, None, WM0), _records(k, d, _vals(rng, n)) + (WM0 + 1,), (None, None, None, MAX_WM)]
    return Stream(f"fill{n}", steps, [0, 1 if n > LIMIT else 0, 0], r=r,
                  premises={1: {"run": n, "new": n, "live": n}})


def stream_passes(r=7):
    """(c) a region in passes.  LIMIT + 1 new groups in two windows are refused and go to k_dt_aggregate, whose
    compact table (3630 groups) takes them in two passes and leaves passes[r] = 1 (it decays only when a push ends
    below 3/4 of that table).  The watermark then fires the older window, so live drops to half, below EPT NT; the
    next narrow push meets passes[r] != 0 alone and is refused; k_dt_aggregate's resumed launch ends with few
    groups, clears passes[r], and the push after that is taken."""
    rng = np.random.default_rng(0x9A55)
    n = LIMIT + 1
    K = keys_in(r, (n + 1) // 2)
    k, d = np.repeat(K, 2)[:n], np.tile(np.arange(2, dtype=np.int64), len(K))[:n]
    fire0 = (WM0 // SIZE + 1) * SIZE - 1  # maxTimestamp of the watermark's window: delta 0 fires, the base stays
    steps = [(None, None, None, WM0),
             _records(k, d, _vals(rng, n)) + (fire0,),
             _records(K[:1], [1], _vals(rng, 1), fire0) + (fire0,),
             _records(K[1:2], [1], _vals(rng, 1), fire0) + (fire0,),
             (None, None, None, MAX_WM)]
    half = n // 2
    prem = {1: {"run": n, "new": n, "live": n}, 2: {"run": 1, "new": 0, "live": half},
            3: {"run": 1, "new": 0, "live": half}}
    return Stream("passes", steps, [0, 1, 1, 0, 0], r=r, premises=prem)


def stream_marker_refused():
    """(d) key -1 in narrow window 7 has the id 0xFFFFFFFF, the table's EMPTY marker: refused as a record, and, once
    its group is an entry of the region, refused again; a push for other regions is taken."""
    rng = np.random.default_rng(0xD1)
    r = int(region_of([-1])[0])
    inr, out = keys_in(r, 20), keys_in(r, 40, inside=False)
    a = _cat(_records([-1], [7], [-123]), _records(inr, rng.integers(0, 8, 20), _vals(rng, 20)))
    a = _shuffled(rng, *_cat(a, _records(out, rng.integers(0, 8, 40), _vals(rng, 40))))
    b = _records(inr[:10], rng.integers(0, 7, 10), _vals(rng, 10))
    c = _records(out, rng.integers(0, 8, 40), _vals(rng, 40))
    steps = [(None, None, None, WM0), a + (WM0 + 1,), b + (WM0 + 2,), c + (WM0 + 3,), (None, None, None, MAX_WM)]
    prem = {1: {"run": 21, "new": 21, "live": 21}, 2: {"run": 10, "new": None, "live": None},
            3: {"run": 0, "new": 0, "live": None}}
    return Stream("marker_refused", steps, [0, 1, 1, 0, 0], r=r, premises=prem, ids=(0xFFFFFFFF,))


MARKER_NEIGHBOURS = (0xFFFFFFF7,) + tuple(range(0xFFFFFFF8, 0xFFFFFFFF)) + (0x80000000, 0x80000007, 0x7FFFFFF8,
                                                                           0x7FFFFFFF, 0)


def stream_marker_neighbours():
    """(d) the ids next to the marker and at the ends of the id range are taken: key -1 in windows 0..6, key -2 in
    window 7, keys -2^28 and 2^28 - 1 in windows 0 and 7, key 0 in window 0, and key 12345 in all eight windows;
    the second push meets them as entries."""
    rng = np.random.default_rng(0xD2)
    k = [-1] * 7 + [-2, KEY_MIN, KEY_MIN, KEY_MAX, KEY_MAX, 0] + [12345] * 8
    d = list(range(7)) + [7, 0, 7, 0, 7, 0] + list(range(8))
    push = lambda: _records(np.repeat(k, 2), np.repeat(d, 2), _vals(rng, 2 * len(k)))  # noqa: E731
    steps = [(None, None, None, WM0), push() + (WM0 + 1,), push() + (WM0 + 2,), (None, None, None, MAX_WM)]
    return Stream("marker_neighbours", steps, [0, 0, 0, 0], ids=MARKER_NEIGHBOURS)


def stream_width(vt):
    """(f) int / short / byte fields on all eight windows: values at the type's bounds, so that the sums of the
    all-maximum and all-minimum groups of every window wrap at the field's width.  Three records a group in every
    push: an odd count, so that an error of count 2^30 or count 2^31 in the bias does not vanish modulo 2^32."""
    rng = np.random.default_rng(0xF00 + BITS[vt])
    lo, hi = BOUNDS[vt]
    k, d = _grid(np.arange(1, 41, dtype=np.int64))
    k, d = np.repeat(k, 3), np.repeat(d, 3)
    steps = [(None, None, None, WM0)]
    for b in range(3):
        v = _vals(rng, len(k), vt)
        v[rng.integers(0, len(k), 50)] = hi
        v[rng.integers(0, len(k), 50)] = lo
        v = np.where(k % 3 == 0, hi, np.where(k % 3 == 1, lo, v))
        steps.append(_shuffled(rng, *_records(k, d, v)) + (WM0 + 1 + b,))
    steps.append((None, None, None, MAX_WM))
    return Stream(f"width_{vt}", steps, [0] * 5, vt=vt)


def stream_grow(n, r=2):
    """(g) expected_entries=0, so R = 1024 entries a region: n new groups of region r in one push.  2000 (above R,
    at most LIMIT): the write-back runs out of the region's buffer (capover), nothing is committed, the host grows
    the table and resumes the push once.  800 (above 3R/4, at most R): the push commits, and the table grows at the
    settle (need_grow) without a resumption."""
    rng = np.random.default_rng(0x6 + n)
    k, d = _grid(keys_in(r, n // 8), n)
    steps = [(None, None, None, WM0), _records(k, d, _vals(rng, n)) + (WM0 + 1,),
             _records(k[:50], d[:50], _vals(rng, 50)) + (WM0 + 2,), (None, None, None, MAX_WM)]
    return Stream(f"grow{n}", steps, [0, 1 if n > 1024 else 0, 0, 0], expected_entries=0, r=r,
                  premises={1: {"run": n, "new": n, "live": n}, 2: {"run": 50, "new": 0, "live": n}})


def stream_sticky(r=6):
    """(h) the switch and its reset: a push with a 70000-record hot key (R) is refused for its run length, a push
    without it (clean) is taken.  R, R, clean, R, R, R, R, R: the clean push resets the count of refusing pushes in
    a row, so the three after it are resumed and only then does the compact table's kernel lead."""
    rng = np.random.default_rng(0x57)
    hot = keys_in(r, 1)[0]
    pool = np.arange(2000, 2400, dtype=np.int64)
    steps, deltas, prem = [(None, None, None, WM0)], [0], {}
    for i, kind in enumerate("RRCRRRRR"):
        rec = _records(pool[rng.integers(0, len(pool), 2000)], rng.integers(0, 8, 2000), _vals(rng, 2000))
        base = int((region_of(rec[0]) == r).sum())
        if kind == "R":
            rec = _shuffled(rng, *_cat(rec, _records(np.full(70_000, hot), rng.integers(0, 8, 70_000),
                                                     _vals(rng, 70_000))))
        steps.append(rec + (WM0,))
        prem[i + 1] = {"run": base + (70_000 if kind == "R" else 0), "new": None, "live": None}
    steps.append((None, None, None, MAX_WM))
    return Stream("sticky", steps, [0, 1, 1, 0, 1, 1, 1, 0, 0, 0], r=r, premises=prem)


def stream_uncounted(sub_partitions):
    """(k) a batch the single pass could not take: k_dn_aggregate refuses every region without counting it.
    P32: one record at narrow delta 8 (a compact form, no narrow one) in the middle of a stream: the batch is redone
    with 16-byte records (narrow_pass_redone), resumed once, and the operator keeps 16-byte records from then on.
    P16: one record 16 windows ahead has no compact form either: the batch is redone through the offset path
    (single_pass_redone, not narrow_pass_redone) and resumed once; the operator stays narrow, so a later narrow push
    for the far entry's region is refused (the entry has no narrow id: compact_delta < 0), others are taken."""
    rng = np.random.default_rng(0xCC + sub_partitions)
    log_s = sub_partitions.bit_length() - 1
    far_dn = 8 if sub_partitions == 32 else 16
    far = np.int64(777)
    r = int(region_of([far], log_s)[0])
    pool = keys_in(r, 300, log_s, first=1000, inside=False)
    inr = keys_in(r, 20, log_s, first=1000)

    def clean(n=1000, keys=pool):
        return _records(keys[rng.integers(0, len(keys), n)], rng.integers(0, 8, n), _vals(rng, n))
    c0, c1 = clean(), clean()
    mid = tuple(np.concatenate([x[:500], y, x[500:]]) for x, y in zip(c1, _records([far], [far_dn], [42])))
    steps = [(None, None, None, WM0), c0 + (WM0 + 1,), mid + (WM0 + 2,), clean() + (WM0 + 3,),
             clean(100, inr) + (WM0 + 4,), (None, None, None, MAX_WM)]
    deltas = [0, 0, 1, 0, 0 if sub_partitions == 32 else 1, 0]
    return Stream(f"uncounted_p{sub_partitions}", steps, deltas, sub_partitions=sub_partitions, r=r, wide={2: 1},
                  premises={4: {"run": 100, "new": None, "live": None}})


# ---- (e) restored entries: `pre` runs on a first operator, `edit` changes its snapshot, `steps` follow the restore
def _restored(name, edit, targets, sub_partitions=16, deltas=None):
    """pre: keys 101, 102, 103 with one record each in narrow window 3.  steps: one narrow push for the region of
    every target key (refused: delta 1 each), then one for the regions that hold none of them (taken)."""
    rng = np.random.default_rng(0xE0 + len(name))
    log_s = sub_partitions.bit_length() - 1
    pre = [(None, None, None, WM0), _records([101, 102, 103], [3, 3, 3], [11, -22, 33]) + (WM0 + 1,)]
    regs = [int(region_of([t], log_s)[0]) for t in targets]
    assert len(set(regs)) == len(regs)
    steps, prem = [(None, None, None, WM0 + 1)], {}
    for i, (t, rg) in enumerate(zip(targets, regs)):
        ks = keys_in(rg, 30, log_s, first=1000)
        steps.append(_records(ks, rng.integers(0, 8, 30), _vals(rng, 30), WM0 + 1) + (WM0 + 2 + i,))
        prem[i + 1] = {"region": rg, "run": 30}
    c = np.arange(5000, 5400, dtype=np.int64)
    c = c[~np.isin(region_of(c, log_s), regs)]
    steps.append(_records(c, rng.integers(0, 8, len(c)), _vals(rng, len(c)), WM0 + 1) + (WM0 + 9,))
    steps.append((None, None, None, MAX_WM))
    deltas = deltas or [0] + [1] * len(targets) + [0, 0]
    return Stream(name, steps, deltas, sub_partitions=sub_partitions, premises=prem, pre=pre, edit=edit)


def _edit_keys(rows):
    rows = rows.copy()
    rows["key"][0], rows["key"][1] = 1 << 28, -(1 << 28) - 1
    return rows


def _edit_start(dn):
    def edit(rows):
        rows = rows.copy()
        rows["start"][0] = (WM0 // SIZE + dn) * SIZE
        rows["end"][0] = rows["start"][0] + SIZE  # (timer is a flag: the trigger's timer at maxTimestamp is set)
        return rows
    return edit


def stream_restored_keys():
    """(e) restored keys 2^28 and -2^28 - 1: one past each end of the narrow key range"""
    return _restored("restored_keys", _edit_keys, [1 << 28, -(1 << 28) - 1])


def stream_restored_far():
    """(e) P16: a restored window 9 windows after the watermark's has no compact form (compact_delta < 0: `d < 0`)"""
    return _restored("restored_far", _edit_start(9), [101])


def stream_restored_dn8():
    """(e) P32: a restored window at narrow delta 10 has a compact form (26 < 32) and no narrow one (`dn >= 8`)"""
    return _restored("restored_dn8", _edit_start(10), [101], sub_partitions=32)


def _edit_minmax(rows):
    rows = rows.copy()
    rows["min"][0], rows["max"][1] = I32_MIN - 1, I32_MAX + 1
    return rows


def stream_restored_minmax():
    """(e) a restored minimum one below int32 (key 101) and a restored maximum one above it (key 102)"""
    return _restored("restored_minmax", _edit_minmax, [101, 102])


def _edit_sums(rows):
    rows = rows.copy()
    rows["sum"][0], rows["sum"][1] = (1 << 63) - 5, -(1 << 63) + 5
    return rows


def stream_restored_sums():
    """(e) restored sums five below 2^63 and five above -2^63, narrow min / max: a narrow push carries each across
    its bound (+10 and -10), and the region is taken: esum + ds wraps at 64 bits"""
    pre = [(None, None, None, WM0), _records([101, 102, 103], [3, 3, 3], [11, -22, 33]) + (WM0 + 1,)]
    steps = [(None, None, None, WM0 + 1),
             _records([101, 101, 102, 102, 103], [3] * 5, [7, 3, -4, -6, 1], WM0 + 1) + (WM0 + 2,),
             (None, None, None, MAX_WM)]
    return Stream("restored_sums", steps, [0, 0, 0], pre=pre, edit=_edit_sums)


def restored_rows(s, snapshot_rows):
    """the edited snapshot of a restored stream"""
    return s.edit(sort_state(snapshot_rows))


def pre_state(s):
    """what the first operator's snapshot holds, from the exact aggregates (the CPU test's stand-in)"""
    ex = Exact()
    for e, (k, t, v, wm) in enumerate(s.pre):
        if k is not None:
            ex.push(k, t, v)
        ex.watermark(wm, e)
    return ex.live()


STREAMS = {
    "rounds": stream_rounds, "claims": stream_claims, "entries": stream_entries,
    "fill_at": lambda: stream_fill(LIMIT), "fill_over": lambda: stream_fill(LIMIT + 1), "passes": stream_passes,
    "marker_refused": stream_marker_refused, "marker_neighbours": stream_marker_neighbours,
    "width_int": lambda: stream_width("int"), "width_short": lambda: stream_width("short"),
    "width_byte": lambda: stream_width("byte"), "grow_over": lambda: stream_grow(2000),
    "grow_after": lambda: stream_grow(800), "sticky": stream_sticky,
    "uncounted_p32": lambda: stream_uncounted(32), "uncounted_p16": lambda: stream_uncounted(16),
    "restored_keys": stream_restored_keys, "restored_far": stream_restored_far,
    "restored_dn8": stream_restored_dn8, "restored_minmax": stream_restored_minmax,
    "restored_sums": stream_restored_sums,
}
_CACHE = {}


def stream(name):
    """the named stream, built once (its arrays are shared: leave them unchanged)"""
    if name not in _CACHE:
        _CACHE[name] = STREAMS[name]()
    return _CACHE[name]

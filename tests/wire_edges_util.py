"""The wire codec's edge cases, built once with tests/wire_ref.py and used by test_oracle_wire_edges.py (the oracle
against wire_ref, on the CPU) and test_gpu_wire_edges.py (the kernels against wire_ref).  The registry checks on the
CPU, from wire_ref's element starts, that every case still reaches the edge it is named for (assert_coverage)."""
import functools

import numpy as np

from tests import wire_ref as W

WCH, WE = 2048, 64  # fw_wire.hip: chunk bytes; first-element offsets per chunk = the largest element with its prefix
LONG_MIN, LONG_MAX = W.LONG_MIN, W.LONG_MAX
INT_MIN = -(1 << 31)

F3 = [("long", "key"), ("long", "skip"), ("int", "value")]
WIDEST = [("long", "key"), ("long", "value"), ("long", "skip"), ("long", "skip"), ("long", "skip"), ("long", "skip"),
          ("short", "skip"), ("byte", "skip")]  # F = 51: an element of 64 bytes with its timestamp and prefix
TOO_WIDE = WIDEST[:-1] + [("short", "skip")]  # F = 52
S2 = [("string", "key"), ("int", "value")]
S4 = [("long", "skip"), ("string", "key"), ("string", "skip"), ("int", "value")]


class Case:
    def __init__(self, name, fields, data, string_limit=W.STRING_LIMIT):
        self.name, self.fields, self.data, self.string_limit = name, fields, bytes(data), string_limit
        self._ref = None

    @property
    def keyed(self):
        return any(k == "string" and r == "key" for k, r in self.fields)

    @property
    def ref(self):  # computed once, shared
        if self._ref is None:
            self._ref = W.decode(self.data, self.fields, self.string_limit)
        return self._ref

    def __repr__(self):
        return self.name


def value_kind(fields):
    return next((k for k, r in fields if r == "value"), None)


def assert_decoded(case, key, kh, ts, val, stats, ref=None):
    """Columns and stats against wire_ref, exactly; a NaN of a Float value field by class (its widened payload is
    build-defined)."""
    ref = case.ref if ref is None else ref
    np.testing.assert_array_equal(np.asarray(key, dtype=np.int64), ref.key, err_msg=f"{case}: key")
    np.testing.assert_array_equal(np.asarray(ts, dtype=np.int64), ref.ts, err_msg=f"{case}: ts")
    if kh is not None:
        np.testing.assert_array_equal(np.asarray(kh, dtype=np.int32), ref.key_hash, err_msg=f"{case}: key_hash")
    val = np.asarray(val, dtype=np.int64)
    assert val.shape == ref.val.shape, f"{case}: val"
    if value_kind(case.fields) == "float":
        nan = np.array([W.is_nan64(int(x)) for x in ref.val], dtype=bool)
        got_nan = np.array([W.is_nan64(int(x)) for x in val], dtype=bool)
        np.testing.assert_array_equal(got_nan, nan, err_msg=f"{case}: NaN class")
        np.testing.assert_array_equal(val[~nan], ref.val[~nan], err_msg=f"{case}: val")
    else:
        np.testing.assert_array_equal(val, ref.val, err_msg=f"{case}: val")
    for f in ("records", "watermarks", "latency_markers", "statuses", "consumed", "watermark", "status"):
        assert stats[f] == ref.stats[f], f"{case}: {f}: {stats[f]} != {ref.stats[f]}"


# ---- building blocks ----------------------------------------------------------------------------------------------
def _f3_element(rng, kind):
    if kind == 0:
        return W.put_record(F3, [int(x) for x in rng.integers(-(1 << 40), 1 << 40, 3)], ts=int(rng.integers(0, 1 << 40)))
    if kind == 1:
        return W.put_record(F3, [int(x) for x in rng.integers(-(1 << 31), 1 << 31, 3)])
    if kind == 2:
        return W.put_watermark(int(rng.integers(-(1 << 40), 1 << 40)))
    if kind == 3:
        return W.put_latency(int(rng.integers(0, 1 << 40)), int(rng.integers(-(1 << 62), 1 << 62)), 7,
                             int(rng.integers(0, 64)))
    return W.put_status(int(rng.integers(-1, 1)))


_F3_SIZE = {0: 33, 1: 25, 2: 13, 3: 33, 4: 9}


def fill_exact(total, seed):
    """Mixed F3 elements of exactly `total` bytes (0, or any total that 9 a + 13 b reaches: every total >= 96)."""
    rng = np.random.default_rng(seed)
    parts, left = [], total
    while left >= 233:
        kind = int(rng.choice([0, 0, 0, 1, 2, 3, 4]))
        parts.append(_f3_element(rng, kind))
        left -= _F3_SIZE[kind]
    for b in range(left // 13 + 1):
        if (left - 13 * b) % 9 == 0:
            parts += [_f3_element(rng, 2) for _ in range(b)] + [_f3_element(rng, 4) for _ in range((left - 13 * b) // 9)]
            break
    else:
        raise ValueError(f"no filler of {total} bytes")
    out = b"".join(parts)
    assert len(out) == total
    return out


_BLOCK = np.dtype([("l0", ">u4"), ("t0", "u1"), ("ts0", ">i8"), ("k0", ">i8"), ("s0", ">i8"), ("v0", ">i4"),
                   ("l1", ">u4"), ("t1", "u1"), ("k1", ">i8"), ("s1", ">i8"), ("v1", ">i4"),
                   ("l2", ">u4"), ("t2", "u1"), ("wm", ">i8"),
                   ("l3", ">u4"), ("t3", "u1"), ("st", ">i4"),
                   ("l4", ">u4"), ("t4", "u1"), ("m", ">i8"), ("lo", ">i8"), ("hi", ">i8"), ("sub", ">i4"),
                   ("l5", ">u4"), ("t5", "u1"), ("ts5", ">i8"), ("k5", ">i8"), ("s5", ">i8"), ("v5", ">i4")])
assert _BLOCK.itemsize == 146


def mixed_bytes(total, seed):
    """A mixed F3 stream of exactly `total` bytes: blocks of six elements (every kind) built as one structured
    array, then an exact filler."""
    nb = max(0, (total - 250) // _BLOCK.itemsize)
    rng = np.random.default_rng(seed)
    a = np.zeros(nb, dtype=_BLOCK)
    for i, (ln, tag) in enumerate([(29, 0), (21, 1), (9, 2), (5, 4), (29, 3), (29, 0)]):
        a[f"l{i}"], a[f"t{i}"] = ln, tag
    for f in ("ts0", "ts5", "m", "wm"):
        a[f] = rng.integers(-(1 << 50), 1 << 50, nb)
    for f in ("k0", "k1", "k5", "s0", "s1", "s5", "lo", "hi"):
        a[f] = rng.integers(LONG_MIN, LONG_MAX, nb)
    for f in ("v0", "v1", "v5", "sub"):
        a[f] = rng.integers(INT_MIN, 1 << 31, nb)
    a["st"] = rng.integers(-1, 1, nb)
    return a.tobytes() + fill_exact(total - nb * _BLOCK.itemsize, seed + 1)


def element_sizes(data, ref):
    ends = ref.starts[1:] + [ref.stats["consumed"] if ref.bad_pos is None else ref.bad_pos]
    return [e - s for s, e in zip(ref.starts, ends)]


def level_vector(nbytes):
    v, m = [], (nbytes + WCH - 1) // WCH
    while True:
        v.append(m)
        if m == 1:
            return v
        m = (m + WE - 1) // WE


# ---- decode, fixed layouts ------------------------------------------------------------------------------------------
def _widest_record(i, ts=None):
    x = i * 0x9E3779B97F4A7C15
    return W.put_record(WIDEST, [x + 1, -x, x ^ 5, x >> 3, ~x, x * 3, i, -i], ts=i * 7 - 3 if ts is None else ts)


@functools.lru_cache(None)
def entry_offset_cases():
    """p status frames (9 bytes), then 200 widest records: every chunk's first element starts 9 p mod 64 into it."""
    return [Case(f"entry_p{p}", WIDEST, b"".join([W.put_status(-(i & 1)) for i in range(p)] +
                                                 [_widest_record(i + p) for i in range(200)])) for p in range(64)]


LEVEL_CHUNKS = (1, 2, 63, 64, 65, 4095, 4096, 4097)


@functools.lru_cache(None)
def level_case(nchunks, exact):
    """A mixed stream of exactly `nchunks` chunks that ends on the chunk boundary (exact), or 777 bytes short of it
    with an element across the last boundary."""
    total = nchunks * WCH - (0 if exact else 777)
    return Case(f"level_{nchunks}_{'exact' if exact else 'straddle'}", F3, mixed_bytes(total, 100 + nchunks))


def level_cases(sizes=LEVEL_CHUNKS):
    return [level_case(n, e) for n in sizes for e in (False, True)]


def reuse_sequence():
    return [level_case(4097, False), Case("reuse_3_chunks", F3, mixed_bytes(3 * WCH - 100, 7)), level_case(65, False)]


@functools.lru_cache(None)
def range_end_cases():
    rec = lambda k, ts: W.put_record(F3, [k, 0, k], ts=ts)  # noqa: E731
    pad = fill_exact(3 * WCH, 31)  # three mixed chunks, whose own watermarks precede the one under test
    out = [Case("ts_ends", F3, rec(1, LONG_MAX) + rec(2, LONG_MIN) + rec(3, -1) + rec(4, 0) + W.put_record(F3, [5, 0, 5])),
           Case("wm_max", F3, rec(1, 5) + W.put_watermark(7) + W.put_watermark(LONG_MAX) + rec(2, 6)),
           Case("wm_min_same_chunk", F3, rec(1, 5) + W.put_watermark(500) + rec(2, 6) + W.put_watermark(LONG_MIN) + rec(3, 7)),
           Case("wm_min_three_chunks_later", F3, rec(1, 5) + W.put_watermark(500) + b"".join(
               rec(i, i) for i in range(3 * WCH // 33 + 2)) + W.put_watermark(LONG_MIN) + rec(3, 7)),
           Case("wm_min_only", F3, rec(1, 5) + W.put_watermark(LONG_MIN) + rec(3, 7)),
           Case("wm_min_then_more_chunks", F3, W.put_watermark(LONG_MIN) + b"".join(rec(i, i) for i in range(200))),
           Case("wm_after_mixed", F3, pad + W.put_watermark(LONG_MIN))]
    for s in (0, -1, INT_MIN, (1 << 31) - 1):
        out.append(Case(f"status_last_{s}", F3, W.put_status(-1 if s == 0 else 0) + rec(1, 1) + W.put_status(s) + rec(2, 2)))
        out.append(Case(f"status_last_{s}_chunks_later", F3, W.put_status(-1 if s == 0 else 0) + W.put_status(s) +
                        b"".join(rec(i, i) for i in range(200))))
    return out


FLOAT_BITS = [0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x007fffff, 0x00800000, 0x7f7fffff, 0xff7fffff,
              0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffbfffff,
              0x3f800000, 0x3f800001]
DOUBLE_BITS = [0, 1 << 63, 1, 0x000fffffffffffff, 0x800fffffffffffff, 0x0010000000000000, 0x7fefffffffffffff,
               0xffefffffffffffff, 0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000000, 0xfff8000000000000,
               0x7ff0000000000001, 0xfff0000000000001, 0xffffffffffffffff, 0x3ff0000000000000]


@functools.lru_cache(None)
def float_cases():
    rng = np.random.default_rng(77)
    fb = FLOAT_BITS + [int(x) for x in rng.integers(0, 1 << 32, 1000)]
    db = DOUBLE_BITS + [int(x) for x in rng.integers(0, 1 << 63, 500)] + [int(x) | (1 << 63) for x in rng.integers(0, 1 << 63, 500)]
    ff, fd = [("long", "key"), ("float", "value")], [("double", "skip"), ("long", "key"), ("double", "value")]
    return [Case("float_values", ff, b"".join(W.put_record(ff, [i, b], ts=i if i % 3 else None) for i, b in enumerate(fb))),
            Case("double_values", fd, b"".join(W.put_record(fd, [b ^ 1, i, b], ts=i if i % 5 else None) for i, b in enumerate(db)))]


INT_RANGE = {"byte": 8, "short": 16, "int": 32, "long": 64}


@functools.lru_cache(None)
def integer_cases():
    out = []
    for kind, bits in INT_RANGE.items():
        vals = [-(1 << (bits - 1)), (1 << (bits - 1)) - 1, -1, 0]
        for role in ("key", "value"):
            other = ("long", "value" if role == "key" else "key")
            fields = [("byte", "skip"), (kind, role), other]
            out.append(Case(f"int_{kind}_{role}", fields, b"".join(
                W.put_record(fields, [i, v, 1000 + i], ts=i if i & 1 else None) for i, v in enumerate(vals))))
    fb = [("boolean", "value"), ("long", "key")]
    out.append(Case("boolean_bytes", fb, b"".join(W.put_record(fb, [b, i], ts=i) for i, b in enumerate([0, 1, 0x80, 0xff, 2]))))
    fb = [("boolean", "key"), ("boolean", "value")]
    out.append(Case("boolean_key", fb, b"".join(W.put_record(fb, [b, b ^ 0x80]) for b in [0, 1, 0x80])))
    return out


def capacity_case():
    return Case("capacity", F3, mixed_bytes(3 * WCH + 5, 55))


# ---- decode, corrupt elements ---------------------------------------------------------------------------------------
def _valid_body(tag):
    el = _f3_element(np.random.default_rng(900 + tag), tag)
    return el[4:]


def corrupt_kinds():
    """name -> (the element's bytes, wire_ref's code)"""
    kinds = {}
    for t in (5, 9, 0x7f, 0x80, 0xff):
        kinds[f"tag_{t:#x}"] = (W.frame(bytes([t]) + bytes(range(1, 9))), t - 256 if t >= 128 else t)
    kinds["empty"] = (W.frame(b""), -3)
    for tag in range(5):
        body = _valid_body(tag)
        kinds[f"tag{tag}_short"] = (W.frame(body[:-1]), -2)
        kinds[f"tag{tag}_long"] = (W.frame(body + b"\x2a"), -2)
    return kinds


PLACEMENTS = ("first", "last", "chunk_first_byte", "chunk_last_byte", "straddle", "chunk_64", "second_later")


def _place(x, placement, other):
    """-> (bytes, the byte position x must be refused at)"""
    tail = fill_exact(3000, 12)
    if placement == "first":
        return x + tail, 0
    if placement == "last":
        return fill_exact(3 * WCH + 300, 13) + x, 3 * WCH + 300
    at = {"chunk_first_byte": 2 * WCH, "chunk_last_byte": 3 * WCH - 1, "straddle": 2 * WCH - 2, "chunk_64": 64 * WCH + 100,
          "second_later": 3000}[placement]
    if placement == "second_later":
        return fill_exact(at, 14) + x + fill_exact(5000, 15) + other + tail, at  # the other corruption comes later
    return fill_exact(at, 16) + x + tail, at


@functools.lru_cache(None)
def corrupt_cases():
    """-> {(kind, placement): (Case, position, code)}"""
    kinds = corrupt_kinds()
    names = list(kinds)
    out = {}
    for i, name in enumerate(names):
        x, code = kinds[name]
        other = kinds[names[(i + 3) % len(names)]][0]
        for pl in PLACEMENTS:
            data, at = _place(x, pl, other)
            out[(name, pl)] = (Case(f"corrupt_{name}_{pl}", F3, data), at, code)
    return out


@functools.lru_cache(None)
def partial_tail_cases():
    """A length prefix that promises more bytes than remain is the next call's element, whatever its tag."""
    head = fill_exact(WCH + 500, 21)
    out = [Case(f"partial_tag{t}", F3, head + _f3_element(np.random.default_rng(t), t)[:-1]) for t in range(5)]
    out.append(Case("partial_unknown_tag", F3, head + W._be(9, 4) + b"\x09123"))
    out.append(Case("partial_huge_prefix", F3, head + b"\xff\xff\xff\xff\x00" + fill_exact(500, 22)))
    out.append(Case("partial_prefix_cut", F3, head + b"\x00\x00"))
    return out


# ---- decode, String layouts -----------------------------------------------------------------------------------------
STRINGS = ["a", "", "w\u00f6rd", "\u65e5\u672c\u8a9e", "\x7f", "\x80", "\u3fff", "\u4000", "\uffff", "\U0001f600x",
           "x" * 20, "\u20acuro", "\x00", "key1"]


def _s_record(fields, i, key, skip, ts):
    if fields is S2:
        return W.put_record(S2, [key, i * 10 - 7], ts=ts)
    return W.put_record(S4, [i * 0x0101010101, key, skip, -i], ts=ts)


@functools.lru_cache(None)
def string_stream(which, n=40):
    fields = S2 if which == "S2" else S4
    parts = []
    for i in range(n):
        s = STRINGS[i % len(STRINGS)]
        parts.append(_s_record(fields, i, s, [None, "", "sk\u00efp"][i % 3], None if i % 4 == 1 else i * 1000 - 5))
        if i % 7 == 3:
            parts.append(W.put_watermark(i))
        if i % 11 == 5:
            parts.append(W.put_status(-(i & 1)))
    return Case(f"strings_{which}", fields, b"".join(parts))


@functools.lru_cache(None)
def string_size_limit_cases():
    """-> [(Case, refused position or None)]: S2 records of exactly 64 and of 65 bytes, with and without timestamp."""
    lead = W.put_record(S2, ["lead", 1], ts=1)
    out = []
    for ts, fits in ((5, 46), (None, 54)):
        ok, over = W.put_record(S2, ["y" * fits, 2], ts=ts), W.put_record(S2, ["y" * (fits + 1), 3], ts=ts)
        assert len(ok) == 64 and len(over) == 65
        out.append((Case(f"string_64_ts{ts}", S2, lead + ok + lead), None))
        out.append((Case(f"string_65_ts{ts}", S2, lead + ok + over + lead), len(lead) + 64))
    return out


@functools.lru_cache(None)
def string_boundary_stream():
    c = string_stream("S4", 120)
    assert len(c.data) > WCH + 70
    return c


def string_boundary_cuts():
    return list(range(WCH - 30, WCH + 71))


@functools.lru_cache(None)
def string_corrupt_cases():
    """-> [(Case, position, code)]"""
    good = [W.put_record(S2, [s, i], ts=i) for i, s in enumerate(["one", "tw\u00f6", "\u65e5"])]
    lead = b"".join(good)
    rec = lambda body: W.frame(b"\x00" + W._be(9, 8) + body)  # noqa: E731
    bad = {
        "varint_past_element": rec(b"\x03a\xe5"),                                   # a char's varint continues into nothing
        "length_varint_past_element": rec(b"\x83"),
        "string_ends_before_element": rec(W.write_string("ab") + W._be(7, 4) + b"\x00"),
        "string_ends_after_element": rec(b"\x06ab"),                                 # five chars promised, two there
        "value_cut_short": rec(W.write_string("ab") + b"\x00\x00"),
        "five_byte_varint_continues": rec(b"\x02\x81\x80\x80\x80\x80\x00" + W._be(7, 4)),
        "five_byte_length_continues": rec(b"\x82\x80\x80\x80\x80\x00a" + W._be(7, 4)),
        "huge_length": rec(b"\xff\xff\xff\xff\x0fab" + W._be(7, 4)),
        "no_timestamp_bytes": W.frame(b"\x00\x01\x02"),
    }
    out = [(Case(f"string_{k}", S2, lead + x + good[0]), len(lead), -2) for k, x in bad.items()]
    null = W.put_record(S2, [None, 4], ts=4)
    out.append((Case("null_key_first", S2, null + lead), 0, -4))
    out.append((Case("null_key_second", S2, good[0] + null + lead), len(good[0]), -4))
    out.append((Case("null_key_last", S2, lead * 30 + null), 30 * len(lead), -4))
    out.append((Case("null_key_no_timestamp", S2, lead + W.put_record(S2, [None, 4]) + lead), len(lead), -4))
    big = string_stream("S2", 200).data  # a null key beyond the first chunk
    out.append((Case("null_key_third_chunk", S2, big + null + lead), len(big), -4))
    # a five-byte varint whose last byte ends it is read (its high bits fall off the char)
    fine = rec(b"\x02\xc1\x80\x80\x80\x01" + W._be(7, 4))
    out.append((Case("string_five_byte_varint_ok", S2, lead + fine + good[0]), None, None))
    return out


# ---- encode ---------------------------------------------------------------------------------------------------------
ENC_KINDS = ("long", "int", "double", "short", "byte", "float", "boolean")
ENC_ROLES = ("key", "start", "end", "count", "sum", "min", "max")


def encode_layouts():
    """Seven layouts of seven fields, a Latin square: every kind meets every role once."""
    return [[(ENC_KINDS[j], ENC_ROLES[(i + j) % 7]) for j in range(7)] for i in range(7)]


def _d(x):
    return W.bits_from_double(x)


FLT_MAX = float(np.finfo(np.float32).max)
ENC_DOUBLE_BITS = ([_d(x) for x in (0.0, -0.0, 0.5, -0.5, 0.99, -0.99, 1.5, -1.5, 2.0 ** -149, 2.0 ** -150, -(2.0 ** -150),
                                    3 * 2.0 ** -150, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, FLT_MAX * (1 + 2.0 ** -25),
                                    2.0 ** 128 - 2.0 ** 103, -(2.0 ** 128 - 2.0 ** 103), float("inf"), float("-inf"),
                                    2.0 ** 63, -(2.0 ** 63), 1e300, -1e300, 2.0 ** 31, -(2.0 ** 31) - 1.5, 255.9)] +
                   [1, 0x000fffffffffffff, 0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001,
                    0xffffffffffffffff, _d(2.0 ** 63) - 1, _d(-(2.0 ** 63)) + 1, _d(-(2.0 ** 63)) - 1])
ENC_INTS = [0, 1, -1, (1 << 53) + 1, -((1 << 53) + 1), (1 << 54) + 2, LONG_MAX, LONG_MIN, 1 << 31, (1 << 31) + 5,
            -(1 << 31) - 1, 1 << 15, 1 << 7, (1 << 24) + 1, 0x0102030405060708, -0x0102030405060708]
ENC_ENDS = [3000, LONG_MAX, LONG_MIN, 0, LONG_MIN + 1, -1]
ENC_ROWS = 257


def _s64(v):
    return W._signed(v, 64)


@functools.lru_cache(None)
def encode_rows(f64):
    """257 rows in which every listed value stands in every column it belongs to (coprime strides)."""
    rows = {f: np.zeros(ENC_ROWS, dtype=np.int64) for f in W.ROW_FIELDS}
    agg = ENC_DOUBLE_BITS if f64 else ENC_INTS
    for i in range(ENC_ROWS):
        rows["key"][i] = ENC_INTS[i % len(ENC_INTS)]
        rows["start"][i] = ENC_INTS[(i + 3) % len(ENC_INTS)]
        rows["count"][i] = ENC_INTS[(i + 5) % len(ENC_INTS)]
        rows["end"][i] = (ENC_ENDS + ENC_INTS)[i % (len(ENC_ENDS) + len(ENC_INTS))]
        rows["sum"][i] = _s64(agg[i % len(agg)])
        rows["min"][i] = _s64(agg[(i + 7) % len(agg)])
        rows["max"][i] = _s64(agg[(i + 13) % len(agg)])
    return rows


def rows_slice(rows, n):
    return {f: rows[f][:n].copy() for f in W.ROW_FIELDS}


ENC_SIZES = (0, 1, 255, 256, 257)


# ---- what the registry promises, checked from wire_ref's element starts -------------------------------------------
def assert_coverage():
    # all 64 entry offsets, and exit offset 63 (an element that ends in the last byte before a chunk's offset 63)
    entries, exits = set(), set()
    for c in entry_offset_cases():
        r = c.ref
        assert r.bad_pos is None and r.stats["records"] == 200 and r.stats["consumed"] == len(c.data)
        firsts = {}
        for s, sz in zip(r.starts, element_sizes(c.data, r)):
            firsts.setdefault(s // WCH, s % WCH)
            if (s + sz) // WCH > s // WCH:
                exits.add((s + sz) % WCH)
            if sz == 64:
                assert len(c.data[s:s + sz]) == 64
        entries |= set(firsts.values())
    assert entries == set(range(64)), sorted(set(range(64)) - entries)
    assert 63 in exits and max(exits) == 63
    # the four level vectors, an element across the last boundary, a stream that ends on one
    vectors = []
    for n in LEVEL_CHUNKS:
        for exact in (False, True):
            c = level_case(n, exact)
            r = c.ref
            assert r.bad_pos is None and r.stats["consumed"] == len(c.data), c
            assert min(r.stats[f] for f in ("records", "watermarks", "latency_markers", "statuses")) > 0
            assert level_vector(len(c.data))[0] == n
            vectors.append(level_vector(len(c.data)))
            if exact:
                assert len(c.data) == n * WCH
            elif n > 1:
                b = (n - 1) * WCH
                assert any(s < b < s + sz for s, sz in zip(r.starts, element_sizes(c.data, r))), c
    for v in ([1], [2, 1], [65, 2, 1], [4097, 65, 2, 1]):
        assert v in vectors, v
    assert [level_vector(len(c.data)) for c in reuse_sequence()] == [[4097, 65, 2, 1], [3, 1], [65, 2, 1]]
    # every corrupt kind at every placement, refused where and how it was built to be
    cc = corrupt_cases()
    assert set(cc) == {(k, p) for k in corrupt_kinds() for p in PLACEMENTS} and len(corrupt_kinds()) == 16
    for (kind, pl), (c, at, code) in cc.items():
        r = c.ref
        assert (r.bad_pos, r.bad_tag) == (at, code), (c, r.bad_pos, r.bad_tag)
        n = len(corrupt_kinds()[kind][0])
        if pl == "last":
            assert at + n == len(c.data)
        if pl == "chunk_first_byte":
            assert at % WCH == 0 and at > 0
        if pl == "chunk_last_byte":
            assert at % WCH == WCH - 1
        if pl == "straddle":
            assert at // WCH < (at + n - 1) // WCH
        if pl == "chunk_64":
            assert at // WCH == 64
        if pl == "second_later":
            later = W.decode(c.data[at + n:], F3)
            assert later.bad_pos is not None and later.bad_pos + n >= 5000
    for c in partial_tail_cases():
        assert c.ref.bad_pos is None and c.ref.stats["consumed"] == WCH + 500, c
    # String layouts
    for which in ("S2", "S4"):
        r = string_stream(which).ref
        assert r.bad_pos is None and r.stats["records"] == 40 and LONG_MIN in r.ts and 900 < len(string_stream(which).data) < WCH
    for c, at in string_size_limit_cases():
        assert c.ref.bad_pos == at and (at is None or c.ref.bad_tag == -2), c
        assert W.decode(c.data, c.fields, string_limit=None).bad_pos is None  # the reference itself has no such limit
    for c, at, code in string_corrupt_cases():
        assert (c.ref.bad_pos, c.ref.bad_tag) == (at, code), (c, c.ref.bad_pos, c.ref.bad_tag)
    # encode: every kind x role, every listed value in its columns
    pairs = {p for L in encode_layouts() for p in L}
    assert pairs == {(k, r) for k in ENC_KINDS for r in ENC_ROLES} and all(len(L) <= 8 for L in encode_layouts())
    for f64 in (False, True):
        rows = encode_rows(f64)
        for f in ("sum", "min", "max"):
            assert {int(x) for x in rows[f]} == {_s64(v) for v in (ENC_DOUBLE_BITS if f64 else ENC_INTS)}
        for f in ("key", "start", "count"):
            assert {int(x) for x in rows[f]} == set(ENC_INTS)
        assert set(ENC_ENDS) <= {int(x) for x in rows["end"]}

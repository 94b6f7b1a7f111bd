"""Input palettes on which floating sums are exactly comparable, and the bit-exact row comparison that goes
with them (tests/test_oracle_float_edges.py guards the inputs on the CPU, tests/test_gpu_float_edges.py drives
them through the GPU's floating-point sites).

GPU atomics add in arbitrary order, so a floating sum is comparable bit for bit only when every partial sum of
the window's elements, in any order, is exactly representable: then every order gives the same bits.

* dyadic: Double fields m * 2^-10 with integer |m| <= 2^20 (keys with key % 2 == 1: m * 2^-3, |m| <= 64, so that
  windows whose sum is exactly zero occur), Float fields m * 2^-3 with |m| <= 64 (as the double of the float).
  A partial sum of fewer than 2^18 such values is an integer multiple of the scale below 2^38 (Double) / 2^24
  (Float): exact in the format, so FloatSum's per-step rounding (SumFunction.java:92-99), the GPU's f64 sum
  rounded once and the exact sum coincide.
* specials, by key % 8, each group's result independent of the order:
    0  canonical NaN among dyadics       sum NaN, max NaN (Double.compare: NaN is largest), min the finite minimum
    1  +Inf among dyadics                sum = max = +Inf
    2  +Inf and -Inf among dyadics       sum NaN once both occur, else the infinity
    3  only -0.0 and +0.0                min = -0.0 if any, max = +0.0 if any, zero sum (sign: see DESIGN "Float sums")
    4  subnormals m * 2^-1074, |m| <= 64 (Float: m * 2^-149)   exact subnormal sums (no flush to zero anywhere)
    5  DBL_MAX (Float: FLT_MAX) among non-negative dyadics     Inf exactly when the window holds two or more
    6, 7  plain dyadic
"""
import numpy as np

NAN_BITS = 0x7FF8000000000000  # Double.doubleToLongBits' canonical NaN
NEG_ZERO_BITS = -(1 << 63)
DBL_MAX = float(np.finfo(np.float64).max)
FLT_MAX = float(np.finfo(np.float32).max)
MAX_WM = (1 << 63) - 1
MAX_WINDOW_COUNT = 1 << 18


def _u32(vals):
    return np.asarray(vals, dtype=np.int64) & 0xFFFFFFFF


def dyadic(keys, vals, value_type):
    """float64 values (of a Float field: the doubles of floats), a deterministic function of (keys, vals)"""
    u = _u32(vals)
    narrow = ((u & 0x7F) - 64).astype(np.float64) * 2.0 ** -3
    if value_type == "f32":
        return narrow
    wide = ((u & 0x1FFFFF) - (1 << 20)).astype(np.float64) * 2.0 ** -10
    return np.where(np.asarray(keys) % 2 == 1, narrow, wide)


def specials(keys, vals, value_type):
    u = _u32(vals)
    g = np.asarray(keys) % 8
    sel = (u >> 21) & 7
    d = dyadic(keys, vals, value_type)
    big = FLT_MAX if value_type == "f32" else DBL_MAX
    sub = 2.0 ** (-149 if value_type == "f32" else -1074)
    out = d.copy()
    out[(g == 0) & (sel == 0)] = np.nan
    out[(g == 1) & (sel == 0)] = np.inf
    out[(g == 2) & (sel == 0)] = np.inf
    out[(g == 2) & (sel == 1)] = -np.inf
    out = np.where(g == 3, np.where(sel & 1, -0.0, 0.0), out)
    out = np.where(g == 4, ((u & 0x7F) - 64).astype(np.float64) * sub, out)
    out = np.where(g == 5, np.where(sel == 0, big, np.abs(d)), out)
    # (every NaN is the canonical one)
    bits = out.view(np.int64).copy()
    bits[np.isnan(out)] = NAN_BITS
    return bits.view(np.float64)


def cancelling(vals):
    """Part 3: +-(v & 0xFFFFF) / 7.0, the sign from another bit of v: sums that cancel and are not exact"""
    u = _u32(vals)
    return np.where((u >> 21) & 1, -1.0, 1.0) * ((u & 0xFFFFF).astype(np.float64) / 7.0)


PALETTES = {"dyadic": dyadic, "specials": specials}


def stream(n, batch, num_keys, bound, jitter, rate, palette, value_type, seed=0x5EED, zipf=None, final=True):
    """[(keys, ts, float64 values)] batches and the watermark after each (max timestamp so far - bound, then
    Long.MAX_VALUE), the shape of tests/test_gpu_parity.py's _stream with the field drawn from a palette."""
    from flink_amd.datagen import generate_host
    keys, ts, vals = generate_host(seed, 0, n, num_keys, ts_base=1_000_000, rate=rate, jitter=jitter, zipf_s=zipf)
    vals = palette(keys, vals, value_type) if callable(palette) else PALETTES[palette](keys, vals, value_type)
    batches, wms, mx = [], [], -(1 << 63)
    for b in range(0, n, batch):
        sl = slice(b, min(n, b + batch))
        batches.append((keys[sl], ts[sl], vals[sl]))
        mx = max(mx, int(ts[sl].max()))
        wms.append(mx - bound)
    if final:
        batches.append((keys[:0], ts[:0], vals[:0]))
        wms.append(MAX_WM)
    return batches, wms


# Every stream of tests/test_gpu_float_edges.py that feeds a keyed window operator, with the oracle configurations
# it is run under there; tests/test_oracle_float_edges.py checks each on the CPU.
ORDERED = dict(n=1 << 17, batch=1 << 13, num_keys=5000, bound=400, jitter=1500, rate=100_000, zipf=1.1)
DENSE = dict(n=1 << 17, batch=1 << 14, num_keys=50_000, bound=20, jitter=30, rate=1_000_000)
HOT = dict(n=1 << 20, batch=1 << 19, num_keys=10_000, bound=50, jitter=50, rate=1_000_000, zipf=1.1)
RESTORE = dict(n=1 << 16, batch=1 << 13, num_keys=3000, bound=50, jitter=80, rate=200_000)
COMBINE = dict(n=1 << 17, batch=1 << 14, num_keys=2000, bound=300, jitter=900, rate=200_000)
COMBINE_PANES = dict(n=1 << 17, batch=1 << 14, num_keys=2000, bound=300, jitter=9000, rate=100_000)

ORDERED_CFG = dict(assigner="tumbling", size=1000, lateness=700)
DENSE_CFG = dict(assigner="tumbling", size=100)
PANES_CFGS = [dict(assigner="sliding", size=3000, slide=1000), dict(assigner="sliding", size=2500, slide=1000, offset=300)]
SESSION_CFG = dict(assigner="session", gap=300, lateness=400)
HOT_CFGS = [dict(assigner="tumbling", size=100), dict(assigner="session", gap=20),
            dict(assigner="sliding", size=400, slide=100)]
RESTORE_CFGS = [dict(assigner="tumbling", size=100), dict(assigner="session", gap=40)]
COMBINE_CFG = dict(assigner="tumbling", size=1000)
COMBINE_PANES_CFG = dict(assigner="sliding", size=6000, slide=1000)

# (name, stream, [(oracle configuration, needs the first-element classes)])
STREAMS = [
    ("ordered", ORDERED, [(ORDERED_CFG, False), (dict(ORDERED_CFG, first=True), True), (SESSION_CFG, False)]
     + [(c, False) for c in PANES_CFGS]),
    ("dense", DENSE, [(DENSE_CFG, False)]),
    ("hot", HOT, [(dict(c, first=True), True) for c in HOT_CFGS]),
    ("restore", RESTORE, [(c, False) for c in RESTORE_CFGS]),
    ("combine", COMBINE, [(COMBINE_CFG, False)]),
    ("combine-panes", COMBINE_PANES, [(COMBINE_PANES_CFG, False)]),
]


# ---- the other inputs of tests/test_gpu_float_edges.py (count windows, the list operator, Table rows)
def count_stream(palette, value_type):
    """tests/test_gpu_parity.py's count-window stream (Zipf 1.05 over 700 keys) with the field from a palette"""
    from flink_amd.datagen import generate_host
    keys, _, vals = generate_host(0xC0DE, 0, 60_000, 700, ts_base=0, rate=1_000_000, jitter=0, zipf_s=1.05)
    return keys, PALETTES[palette](keys, vals, value_type)


def list_stream(palette, value_type, keys=37, span=2000, n=20_000):
    """tests/test_gpu_list.py's seeded stream shape (out of order by up to 150 ms) with the field from a palette"""
    rng = np.random.default_rng(0xF10A7)
    k = rng.integers(0, keys, n, dtype=np.int64)
    t = np.arange(n, dtype=np.int64) * span // n - rng.integers(0, 150, n, dtype=np.int64)
    return k, t, PALETTES[palette](k, rng.integers(0, 1 << 32, n, dtype=np.int64), value_type)


TABLE_TYPES = ["f64", "f32", "i32"]
TABLE_SPECS = ([("count_star", 0)] + [(fn, c) for c in (0, 1) for fn in ("count", "sum", "avg", "min", "max")]
               + [("sum", 2)])
TABLE_CFGS = [dict(assigner="tumbling", size=1000), dict(assigner="sliding", size=3000, slide=1000),
              dict(assigner="sliding", size=2500, slide=1000, offset=300), dict(assigner="session", gap=400)]


def table_columns(palette):
    """a Double and a Float column carrying the palette (from different bits of the generator's value), an Int column"""
    pal = PALETTES[palette]
    return lambda k, v: [pal(k, v, "f64"), pal(k, v >> 3, "f32"), v % 100_003]


def table_steps(cols_of, n=1 << 17, batch=1 << 14, keys=20_000, bound=300, jitter=900, rate=200_000, seed=0x5EED):
    """tests/test_gpu_table.py's stream (Zipf 1.1 keys, 15 % NULLs per column) with the columns from cols_of(k, v)"""
    from flink_amd.datagen import generate_host
    k, t, v = generate_host(seed, 0, n, keys, ts_base=1_000_000, rate=rate, jitter=jitter, zipf_s=1.1)
    rng = np.random.default_rng(seed)
    cols = cols_of(k, v)
    nulls = np.zeros(n, dtype=np.uint8)
    for j in range(len(cols)):
        nulls |= ((rng.random(n) < 0.15).astype(np.uint8) << j)
    out, mx = [], -(1 << 63)
    for b in range(0, n, batch):
        sl = slice(b, min(n, b + batch))
        mx = max(mx, int(t[sl].max()))
        out.append((k[sl], t[sl], [c[sl] for c in cols], nulls[sl], mx - bound))
    out.append((k[:0], t[:0], [c[:0] for c in cols], nulls[:0], MAX_WM))
    return out



def table_column_view(rows, vals, nulls, c):
    """(count, sum, min, max) of value column c (0: Double, 1: Float) of TABLE_SPECS results as rows for classes(),
    for the result rows where the column has a non-NULL value"""
    q0 = 1 + 5 * c
    live = (nulls >> (q0 + 1)) & 1 == 0
    from oracle.oracle import ROW_DTYPE
    view = np.zeros(int(live.sum()), dtype=ROW_DTYPE)
    view["key"], view["count"] = rows["key"][live], vals[live, q0]
    view["sum"], view["min"], view["max"] = vals[live, q0 + 1], vals[live, q0 + 3], vals[live, q0 + 4]
    return view


def f64(bits):
    return np.asarray(bits, dtype=np.int64).view(np.float64)


def classes(rows, value_type, first=False):
    """How many rows carry each class the palettes exist for (count / sum / min / max rows of a keyed operator; with
    first=True the rows' max is an arrival ordinal, so the zero pair is not visible and the -0.0 sum is counted)."""
    s, n, g = f64(rows["sum"]), rows["count"], rows["key"] % 8
    big = FLT_MAX if value_type == "f32" else DBL_MAX
    tiny = float(np.finfo(np.float32 if value_type == "f32" else np.float64).tiny)
    with np.errstate(invalid="ignore"):
        out = {
            "negative_sum": int((s < 0).sum()),
            "zero_sum_n2": int(((s == 0) & (n >= 2)).sum()),
            "nan_sum": int(np.isnan(s).sum()),
            "pinf_sum": int(((s == np.inf) & (g != 5)).sum()),
            "ninf_sum": int((s == -np.inf).sum()),
            "subnormal_sum": int(((s != 0) & (np.abs(s) < tiny)).sum()),
            "max_sum": int((s == big).sum()),
            "overflow_sum": int(((s == np.inf) & (g == 5)).sum()),
        }
    if first:
        out["neg_zero_sum"] = int((rows["sum"] == NEG_ZERO_BITS).sum())
    else:
        out["zero_pair"] = int(((rows["min"] == NEG_ZERO_BITS) & (rows["max"] == 0)).sum())
    return out


DYADIC_CLASSES = ("negative_sum", "zero_sum_n2")
SPECIAL_CLASSES = ("negative_sum", "zero_sum_n2", "nan_sum", "pinf_sum", "ninf_sum", "subnormal_sum", "max_sum",
                   "overflow_sum")


def required_classes(palette, first=False):
    if palette == "dyadic":
        return DYADIC_CLASSES
    return SPECIAL_CLASSES + (("neg_zero_sum",) if first else ("zero_pair",))


def _order(rows, epoch):
    cols = [rows["max"], rows["min"], rows["count"], rows["end"], rows["start"], rows["key"]]
    return np.lexsort(cols + [rows["epoch"]] if epoch else cols)


def assert_rows_bit_equal(gpu, ref, epoch=True):
    """Stricter than parity_util.assert_rows_equal: epoch, key, start, end, count equal; min and max equal as
    int64 bits (both sides canonicalise NaN); the sum equal as int64 bits, so the sign of a zero counts -- except
    that a NaN sum matches any NaN (Inf - Inf is 0xfff8... on x86 and 0x7ff8... on the GPU, and the oracle keeps
    raw sum bits).  epoch=False for count windows (GlobalWindows rows are not tied to watermarks)."""
    assert len(gpu) == len(ref), f"row count {len(gpu)} != {len(ref)}"
    assert len(gpu) > 0
    g, r = gpu[_order(gpu, epoch)], ref[_order(ref, epoch)]
    for f in (("epoch",) if epoch else ()) + ("key", "start", "end", "count", "min", "max"):
        bad = np.nonzero(g[f] != r[f])[0]
        assert bad.size == 0, f"field {f} differs in {bad.size} rows, first: gpu={g[bad[:3]]} ref={r[bad[:3]]}"
    assert_bits_or_nan(g["sum"], r["sum"], "sum", g, r)


def assert_bits_or_nan(a, b, what, ga=None, rb=None):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    same = (a == b) | (np.isnan(f64(a)) & np.isnan(f64(b)))
    bad = np.nonzero(~same)[0]
    ctx = "" if ga is None else f" gpu={ga[bad[:3]]} ref={rb[bad[:3]]}"
    assert bad.size == 0, (f"{what} differs in {bad.size} of {len(a)}, first: {[hex(int(x) & (2**64 - 1)) for x in a[bad[:3]]]} vs "
                           f"{[hex(int(x) & (2**64 - 1)) for x in b[bad[:3]]]}{ctx}")


def java_double_compare(a, b):
    """Double.compare(a, b) restated: numeric order first, then doubleToLongBits (so -0.0 < 0.0, and NaN, whose
    bits are canonical, equals itself and is larger than +Inf)."""
    if a < b:
        return -1
    if a > b:
        return 1
    x = NAN_BITS if a != a else int(np.float64(a).view(np.int64))
    y = NAN_BITS if b != b else int(np.float64(b).view(np.int64))
    return 0 if x == y else -1 if x < y else 1


DOUBLE_COMPARE_LIST = [float("-inf"), -DBL_MAX, -1.5, -2.0 ** -1022, -2.0 ** -1074, -0.0, 0.0, 2.0 ** -1074,
                       2.0 ** -1022, 1.5, FLT_MAX, DBL_MAX, float("inf"), float("nan")]

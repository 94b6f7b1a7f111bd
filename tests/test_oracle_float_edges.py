"""CPU guard of the inputs of tests/test_gpu_float_edges.py, on the oracle alone: the palettes of
tests/float_edges_util.py must make floating sums independent of the summation order (or the GPU comparison could
not be bit-exact), keep every window below 2^18 elements (the Float palette's exactness bound), and produce every
class of row the GPU tests rely on.  These are conditions on the inputs: if one fails, the stream is wrong.
Also: the oracle's Double.compare order over the special values, and the sign of a zero sum per aggregate."""
import functools
import itertools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import float_edges_util as fe

VTS = ["f64", "f32"]
PALS = ["dyadic", "specials"]


def _freeze(cfg):
    return tuple(sorted(cfg.items()))


@functools.lru_cache(maxsize=None)
def _stream(name, palette, vt):
    spec = next(s for n, s, _ in fe.STREAMS if n == name)
    return fe.stream(palette=palette, value_type=vt, **spec)


def _oracle_rows(name, palette, vt, cfg, reverse=False):
    batches, wms = _stream(name, palette, vt)
    ref = orc.WindowOperatorOracle(**dict(cfg), value_type=vt)
    for (k, t, v), wm in zip(batches, wms):
        if reverse:
            k, t, v = k[::-1], t[::-1], v[::-1]
        ref.process(k, t, v)
        ref.watermark(wm)
    rows = ref.rows()
    ref.close()
    return rows


CASES = [(n, c, first) for n, _, cfgs in fe.STREAMS for c, first in cfgs]
IDS = [f"{n}-{c['assigner']}{c.get('size', c.get('gap'))}{'-first' if first else ''}" for n, c, first in CASES]


@pytest.mark.parametrize("vt", VTS)
@pytest.mark.parametrize("palette", PALS)
@pytest.mark.parametrize("name,cfg,first", CASES, ids=IDS)
def test_stream_has_every_class_and_short_windows(name, cfg, first, palette, vt):
    rows = _oracle_rows(name, palette, vt, _freeze(cfg))
    assert 0 < int(rows["count"].max()) < fe.MAX_WINDOW_COUNT
    got = fe.classes(rows, vt, first)
    for c in fe.required_classes(palette, first):
        assert got[c] > 0, (c, got)


ASSIGNERS = []
for _n, _, _cfgs in fe.STREAMS:
    for _c, _ in _cfgs:
        _a = {k: v for k, v in _c.items() if k in ("assigner", "size", "slide", "offset")}
        if _a["assigner"] != "session" and (_n, _a) not in ASSIGNERS:
            ASSIGNERS.append((_n, _a))


@pytest.mark.parametrize("vt", VTS)
@pytest.mark.parametrize("palette", PALS)
@pytest.mark.parametrize("name,cfg", ASSIGNERS, ids=[f"{n}-{c['assigner']}{c['size']}" for n, c in ASSIGNERS])
def test_rows_do_not_depend_on_the_order_inside_a_batch(name, cfg, palette, vt):
    """Every batch fed in reversed internal order: the same rows, bit for bit (NaN sums as a class).  On the
    stream's assigner alone: with allowed lateness every late element fires its window again with the partial sum
    so far, and a first-element row carries an arrival ordinal, which both legitimately depend on the order (as
    session lateness does); the sums of whole windows, which is what the palettes promise, do not."""
    a = _oracle_rows(name, palette, vt, _freeze(cfg))
    b = _oracle_rows(name, palette, vt, _freeze(cfg), reverse=True)
    fe.assert_rows_bit_equal(a, b)


def test_palette_values_are_what_the_docstring_says():
    keys = np.repeat(np.arange(16, dtype=np.int64), 4096)
    vals = (np.arange(len(keys), dtype=np.int64) * 2654435761) & 0xFFFFFFFF
    for vt, scale, big, sub in (("f64", 2.0 ** -10, fe.DBL_MAX, 2.0 ** -1074), ("f32", 2.0 ** -3, fe.FLT_MAX, 2.0 ** -149)):
        d = fe.dyadic(keys, vals, vt)
        assert np.array_equal(d, np.round(d / scale) * scale) and np.abs(d).max() <= (2.0 ** 10 if vt == "f64" else 8.0)
        assert np.array_equal(d[keys % 2 == 1] * 8, np.round(d[keys % 2 == 1] * 8)) and np.abs(d[keys % 2 == 1]).max() <= 8
        assert (d < 0).any() and (d > 0).any()
        s = fe.specials(keys, vals, vt)
        g = keys % 8
        if vt == "f32":
            assert np.array_equal(s[~np.isnan(s)], s[~np.isnan(s)].astype(np.float32).astype(np.float64))
        assert np.isnan(s[g == 0]).any() and set(s[np.isnan(s)].view(np.int64).tolist()) == {fe.NAN_BITS}
        assert not np.isnan(s[g != 0]).any()
        assert (s[g == 1] == np.inf).any() and not (s[g == 1] == -np.inf).any()
        assert (s[g == 2] == np.inf).any() and (s[g == 2] == -np.inf).any()
        assert set(s[g == 3].view(np.int64).tolist()) == {0, fe.NEG_ZERO_BITS}
        assert np.array_equal(s[g == 4], np.round(s[g == 4] / sub) * sub) and np.abs(s[g == 4]).max() <= 64 * sub
        assert (s[g == 4] != 0).any()
        assert (s[g == 5] == big).any() and (s[g == 5] >= 0).all()
        assert np.array_equal(s[g >= 6], d[g >= 6])


def test_oracle_double_compare_order():
    """min / max of every ordered pair of the special values through a window of two elements, against a plain
    restatement of Double.compare (numeric order, then doubleToLongBits: -0.0 < 0.0, NaN canonical and largest);
    minBy / maxBy select by the same order."""
    xs = fe.DOUBLE_COMPARE_LIST
    assert all(fe.java_double_compare(a, b) < 0 for a, b in zip(xs, xs[1:]))  # (the list is in Double.compare order)
    assert fe.java_double_compare(float("nan"), float("nan")) == 0 and fe.java_double_compare(-0.0, 0.0) < 0
    pairs = list(itertools.product(range(len(xs)), repeat=2))
    keys = np.repeat(np.arange(len(pairs), dtype=np.int64), 2)
    vals = np.array([xs[i] for p in pairs for i in p], dtype=np.float64)
    ts = np.full(len(keys), 5, dtype=np.int64)
    bits = lambda x: fe.NAN_BITS if x != x else int(np.float64(x).view(np.int64))  # noqa: E731
    for kw, col in ((dict(), None), (dict(by="min"), "min"), (dict(by="max"), "max")):
        ref = orc.WindowOperatorOracle(assigner="tumbling", size=10, value_type="f64", **kw)
        ref.process(keys, ts, vals)
        ref.watermark(fe.MAX_WM)
        rows = ref.rows()
        rows = rows[np.argsort(rows["key"])]
        assert len(rows) == len(pairs)
        for r, (i, j) in zip(rows, pairs):
            a, b = xs[i], xs[j]
            lo, hi = (a, b) if fe.java_double_compare(a, b) <= 0 else (b, a)
            if col is None:
                assert (int(r["min"]), int(r["max"])) == (bits(lo), bits(hi)), (a, b)
            else:  # the selected field, and on a tie the earlier element (ordinal 2 * pair)
                assert int(r["min"]) == bits(lo if col == "min" else hi), (a, b, col)
                first_wins = fe.java_double_compare(a, b) <= 0 if col == "min" else fe.java_double_compare(a, b) >= 0
                assert int(r["max"]) == 2 * int(r["key"]) + (0 if first_wins else 1), (a, b, col)


@pytest.mark.parametrize("vt", VTS)
@pytest.mark.parametrize("assigner", [dict(assigner="tumbling", size=10), dict(assigner="session", gap=10)],
                         ids=["tumbling", "session"])
def test_oracle_sign_of_a_zero_sum(assigner, vt):
    """sum(pos) / max(pos) / minBy / maxBy keep a ReducingState: the first element is the state and later ones are
    added to it (HeapReducingState.java:72-84, SumAggregator.java:66-76), so a window of -0.0 alone sums to -0.0 and
    any +0.0 makes it +0.0.  CountSumMinMax adds to createAccumulator's +0.0: always +0.0."""
    keys = np.array([1, 1, 2, 2, 3, 3, 4], dtype=np.int64)
    vals = np.array([-0.0, -0.0, -0.0, 0.0, 0.0, -0.0, -0.0])
    ts = np.array([1, 2, 1, 2, 1, 2, 1], dtype=np.int64)
    want_reduce = {1: fe.NEG_ZERO_BITS, 2: 0, 3: 0, 4: fe.NEG_ZERO_BITS}
    for kw in (dict(), dict(first=True), dict(first="max"), dict(by="min"), dict(by="max")):
        ref = orc.WindowOperatorOracle(**assigner, value_type=vt, **kw)
        ref.process(keys, ts, vals)
        ref.watermark(fe.MAX_WM)
        got = {int(r["key"]): int(r["sum"]) for r in ref.rows()}
        assert got == (want_reduce if kw else {k: 0 for k in want_reduce}), kw
    cw = orc.CountWindowOracle(2, 2, value_type=vt)
    cw.process(keys, vals.view(np.int64))
    assert {int(r["key"]): int(r["sum"]) for r in cw.rows()} == {1: fe.NEG_ZERO_BITS, 2: 0, 3: 0}


def _table_oracle(cfg, palette, reverse=False):
    ref = orc.WindowOperatorOracle(**cfg, row=(fe.TABLE_TYPES, fe.TABLE_SPECS))
    for k, t, cols, nulls, wm in fe.table_steps(fe.table_columns(palette)):
        if reverse:
            k, t, cols, nulls = k[::-1], t[::-1], [c[::-1] for c in cols], nulls[::-1]
        ref.process_rows(k, t, cols, nulls)
        ref.watermark(wm)
    rows, (vals, nm) = ref.rows(), ref.row_results()
    o = np.lexsort((rows["count"], rows["start"], rows["key"], rows["epoch"]))
    return rows[o], vals[o], nm[o]


@pytest.mark.parametrize("palette", PALS)
@pytest.mark.parametrize("cfg", fe.TABLE_CFGS, ids=["tumbling", "sliding", "sliding-split", "session"])
def test_table_stream(cfg, palette):
    """The Table rows' inputs: every class in the Double and the Float column's SUM / MIN / MAX, windows below 2^18
    elements, and (non-session assigners) every aggregate bit-identical with each batch reversed."""
    rows, vals, nm = _table_oracle(cfg, palette)
    assert 0 < int(rows["count"].max()) < fe.MAX_WINDOW_COUNT
    for c, vt in ((0, "f64"), (1, "f32")):
        got = fe.classes(fe.table_column_view(rows, vals, nm, c), vt)
        for cl in fe.required_classes(palette):
            assert got[cl] > 0, (vt, cl, got)
    if cfg["assigner"] != "session":
        rows2, vals2, nm2 = _table_oracle(cfg, palette, reverse=True)
        for f in ("epoch", "key", "start", "end", "count"):
            assert np.array_equal(rows[f], rows2[f]), f
        assert np.array_equal(nm, nm2)
        fe.assert_bits_or_nan(vals.ravel(), vals2.ravel(), "table aggregates")


@pytest.mark.parametrize("vt", VTS)
def test_count_and_list_streams_have_every_class(vt):
    """count windows (at most 10 elements, summed in list order on both sides) and the list operator's windows"""
    keys, vals = fe.count_stream("specials", vt)
    ref = orc.CountWindowOracle(10, 5, value_type=vt)
    ref.process(keys, vals.view(np.int64))
    got = fe.classes(ref.rows(), vt, first=True)
    for cl in fe.required_classes("specials", first=True):
        assert got[cl] > 0, (cl, got)
    for cfg, shape in ((dict(assigner="tumbling", size=100), {}), (dict(assigner="session", gap=30), dict(keys=400, span=20_000))):
        k, t, v = fe.list_stream("specials", vt, **shape)
        ref = orc.ListWindowOracle(value_type=vt, **cfg)
        ref.process(k, t, v)
        ref.watermark(fe.MAX_WM)
        r = ref.rows()
        view = np.zeros(len(r), dtype=orc.ROW_DTYPE)
        for f in ("key", "count", "sum", "min", "max"):
            view[f] = r[f]
        assert 0 < int(r["count"].max()) < fe.MAX_WINDOW_COUNT
        got = fe.classes(view, vt)
        for cl in fe.required_classes("specials"):
            assert got[cl] > 0, (cfg, cl, got)

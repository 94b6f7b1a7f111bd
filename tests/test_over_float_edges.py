"""The OVER edge streams of tests/over_edges_util.py on the CPU: their shape, and -- on the restatement's output
alone -- that every class of result tests/test_gpu_over_edges.py exists for does occur under every frame.  No GPU."""
import numpy as np
import pytest

from tests import over_edges_util as E
from tests.float_edges_util import DBL_MAX, NAN_BITS, NEG_ZERO_BITS

MIN_ROWS = 8


@pytest.mark.parametrize("variant", E.VARIANTS)
def test_stream_shape(variant):
    keys, ts, cols, nulls, bounds = E.stream(variant)
    n = len(keys)
    assert n <= 1 << 14 and len(bounds) == E.PUSHES + 1
    assert cols[0].dtype == np.float64 and cols[1].dtype == np.float32 and cols[2].dtype == np.int64
    # time-ordered across the pushes (no cadence makes a row late), out of order within one
    tops = [int(ts[a:b].max()) for a, b in zip(bounds[:-1], bounds[1:])]
    lows = [int(ts[a:b].min()) for a, b in zip(bounds[:-1], bounds[1:])]
    assert all(lo > top for lo, top in zip(lows[1:], tops[:-1])) and lows[0] == 1
    assert all((np.diff(ts[a:b]) < 0).any() for a, b in zip(bounds[:-1], bounds[1:]))
    for cadence in ("final", "every_push", "every_37"):
        wms = E.cadence_watermarks(variant, cadence)
        flat = [w for ws in wms for w in ws]
        assert flat == sorted(flat) and flat[-1] == E.LMAX
        for q, ws in enumerate(wms[:-1]):
            assert all(w < lows[q + 1] for w in ws)
    assert len([w for ws in E.cadence_watermarks(variant, "every_37") for w in ws]) == tops[-1] // 37 + 1
    # key 0 is the smallest key (its run starts the gathered rows) and holds 2 * 4096 + 17 rows in peer pairs
    assert keys.min() == E.LONG_KEY and int((keys == E.LONG_KEY).sum()) == E.LONG_ROWS == 8209
    run = np.flatnonzero(keys == E.LONG_KEY)
    run = run[np.argsort(ts[run], kind="stable")]            # (row time, arrival)
    assert (ts[run] == 1 + np.arange(E.LONG_ROWS) // 2).all()
    d = cols[0].view(np.int64)[run]
    f = cols[1].astype(np.float64).view(np.int64)[run]       # as the handle widens it
    want = {"nan": NAN_BITS, "neg_nan": E.NEG_NAN_BITS, "pinf": E.INF_BITS, "neg_zero": NEG_ZERO_BITS}
    for q, p in enumerate(E.SPECIAL_AT):
        assert nulls[run[p]] == 0
        if variant in want:
            assert d[p] == want[variant] and f[p] == want[variant], (p, hex(d[p]), hex(f[p]))
        elif variant == "pinf_ninf":
            assert cols[0][run[p]] == (np.inf if q % 2 == 0 else -np.inf)
        else:
            assert cols[0][run[p]] == DBL_MAX and cols[0][run[min(p + 1, E.LONG_ROWS - 1)]] == DBL_MAX
    special = set(E._long_specials(variant))
    plain = np.array([p not in special for p in range(E.LONG_ROWS)])
    assert np.isfinite(cols[0][run][plain]).all() and (np.abs(cols[0][run][plain]) <= 1024).all()
    # the short keys: NULLs, wholly NULL keys, the all -0.0 keys, sign-set NaNs kept as they are
    short = keys != E.LONG_KEY
    assert len(np.unique(keys[short])) == E.SHORT_KEYS
    for c in (0, 1):
        frac = float(((nulls[short] >> c) & 1).mean())
        assert 0.15 < frac < 0.3, frac
    assert ((nulls[keys % 32 == 9] & 3) == 3).all() and (keys % 32 == 9).sum() >= 200
    assert (cols[0].view(np.int64)[keys % 16 == 7] == NEG_ZERO_BITS).all()
    bits = cols[0].view(np.int64)[short]
    assert (bits[keys[short] % 8 == 6] == E.NEG_NAN_BITS).sum() >= 100 and (bits[keys[short] % 8 == 0] == NAN_BITS).sum() >= 50
    assert (cols[1].astype(np.float64).view(np.int64)[short] == E.NEG_NAN_BITS).sum() >= 100
    # DBL_MAX only as one pair of consecutive peers per key % 8 == 5 key
    for k in np.unique(keys[short & (keys % 8 == 5)]):
        r = np.flatnonzero(keys == k)
        r = r[np.argsort(ts[r], kind="stable")]
        big = np.flatnonzero(cols[0][r] == DBL_MAX)
        assert len(big) == 2 and big[1] == big[0] + 1 and ts[r[big[0]]] == ts[r[big[1]]] and (nulls[r[big]] & 1 == 0).all()
        assert (cols[0][r] >= 0).all()


@pytest.mark.parametrize("kind,preceding", E.FRAMES, ids=E.FRAME_IDS)
def test_every_class_occurs(kind, preceding, capsys):
    """Counted on the short keys, which every variant shares.  Two places where a class cannot come from them:
    RANGE 0 retracts every earlier row before it accumulates a row time's rows, so the map of the retracting MAX empties
    (MaxAggFunctionWithRetract.scala:78-80) and no NaN is ever stale: the count must be 0; under ROWS 200 no row leaves a
    21-row key's frame, so the two bounded classes are counted over the whole "nan" stream (key 0 included)."""
    got = E.classes("nan", kind, preceding)
    with capsys.disabled():
        print(f"\n  {kind} {preceding}: {got}")
    for c in E.COMMON_CLASSES:
        assert got[c] >= MIN_ROWS, (c, got)
    if not kind.startswith("bounded"):
        assert all(got[c] == 0 for c in E.BOUNDED_CLASSES)
        return
    if preceding == 200:
        got = E.classes("nan", kind, preceding, short_only=False)
        with capsys.disabled():
            print(f"  {kind} {preceding}, with key 0: {got}")
    assert got["poison_outlives_row"] >= MIN_ROWS, got
    if (kind, preceding) == ("bounded_range", 0):
        assert got["stale_max_nan"] == 0
    else:
        assert got["stale_max_nan"] >= MIN_ROWS, got


@pytest.mark.parametrize("kind,preceding", [f for f in E.FRAMES if f[0].startswith("bounded")],
                         ids=[i for i in E.FRAME_IDS if i.startswith("bounded")])
def test_frame_true_max_differs_from_the_restatement_in_the_stale_nans_only(kind, preceding):
    rows, _ = E.restated("neg_nan", kind, preceding)
    raw, exp = E.rows_to_arrays(rows), E.expected("neg_nan", kind, preceding)
    stale = E.classes("neg_nan", kind, preceding, short_only=False)["stale_max_nan"]
    for q in E.MAX_OF:
        a, b = raw["values"][:, q], exp["values"][:, q]
        live = (raw["null_mask"] >> q) & 1 == 0
        differ = live & (np.where(E._is_nan(a), NAN_BITS, a) != b)
        assert (E._is_nan(a[differ])).all() and not E._is_nan(b[differ]).any()
        if q == E.Q_MAX:
            assert int(differ.sum()) == stale
    for f in ("key", "rowtime", "ordinal", "null_mask"):
        assert np.array_equal(raw[f], exp[f])


def test_the_comparison_sees_zero_signs_and_nan_bits():
    exp = E.expected("nan", "bounded_rows", 1)
    E.same_rows_bits({f: a.copy() for f, a in exp.items()}, exp)

    def changed(q, pick, new):
        got = {f: a.copy() for f, a in exp.items()}
        i = int(np.flatnonzero(pick(exp["values"][:, q]) & ((exp["null_mask"] >> q) & 1 == 0))[0])
        got["values"][i, q] = new
        return got
    E.same_rows_bits(changed(E.Q_SUM, E._is_nan, E.NEG_NAN_BITS), exp)          # a NaN sum matches any NaN
    for q, pick, new in ((E.Q_SUM, lambda v: v == 0, NEG_ZERO_BITS), (E.Q_MIN, lambda v: v == NEG_ZERO_BITS, 0),
                         (E.Q_MAX, E._is_nan, E.NEG_NAN_BITS), (E.Q_FMAX, E._is_nan, E.INF_BITS),
                         (E.Q_SUM, E._is_nan, E.INF_BITS), (E.Q_CNT, lambda v: v == 1, 2)):
        with pytest.raises(AssertionError):
            E.same_rows_bits(changed(q, pick, new), exp)
    got = {f: a[::-1].copy() for f, a in exp.items()}                              # a key's rows out of order
    with pytest.raises(AssertionError):
        E.same_rows_bits(got, exp)

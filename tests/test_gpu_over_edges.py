"""Row-time OVER windows on the GPU (fw_over.hip) on Double specials, zero signs, firing cadences, restored state
and the ends of the row-time range, bit for bit against the restatement (tests/over_ref.py through
tests/over_edges_util.py; tests/test_over_float_edges.py shows on the CPU that the streams are not vacuous).
No tolerance anywhere: the inputs make every finite sum exact."""
import numpy as np
import pytest

from flink_amd.over import Over, OverAggregate
from tests import over_edges_util as E
from tests.float_edges_util import DBL_MAX, NEG_ZERO_BITS
from tests.over_ref import LMAX, LMIN, OverRef

pytestmark = pytest.mark.gpu

MAX_PAR = 16
FIELDS = ("key", "rowtime", "ordinal", "values", "null_mask")


def gpu_op(kind, preceding, types=E.TYPES, aggs=E.AGGS, **kw):
    frame = {"bounded_rows": lambda: Over.rows(preceding), "bounded_range": lambda: Over.range(preceding),
             "unbounded_rows": Over.unbounded_rows, "unbounded_range": Over.unbounded_range}[kind]()
    return OverAggregate(frame, types, aggs, **kw)


def push(op, p, device=False):
    keys, ts, cols, nulls = p
    if not device:
        op.process(keys, ts, cols, nulls)   # the Float column as a float32 array
        return
    import torch
    words = [np.ascontiguousarray(c, dtype=np.float64).view(np.int64) if c.dtype.kind == "f" else c.astype(np.int64)
             for c in cols]
    op.process(torch.from_numpy(keys.copy()).cuda(), torch.from_numpy(ts.copy()).cuda(),
               torch.from_numpy(np.stack(words)).cuda(), torch.from_numpy(nulls.copy()).cuda())


def fire(op, wms):
    parts = []
    for w in wms:
        op.advance_watermark(w)
        parts.append(op.drain_arrays())
    return parts


def run(op, variant, cadence, device=False, first=0, last=None):
    """the rows of pushes first .. last - 1 under a cadence, concatenated over the watermarks"""
    parts = []
    for p, wms in list(zip(E.pushes(variant), E.cadence_watermarks(variant, cadence)))[first:last]:
        push(op, p, device)
        parts += fire(op, wms)
    return E.concat(parts) if parts else None


def per_key(a):
    """rows grouped by key, each key's rows in the order they were emitted"""
    o = np.argsort(a["key"], kind="stable")
    return {f: a[f][o] for f in FIELDS}


# ---------------------------------------------------------------- 1. parity on the specials streams
@pytest.mark.parametrize("kind,preceding", E.FRAMES, ids=E.FRAME_IDS)
@pytest.mark.parametrize("variant", E.VARIANTS)
def test_gpu_over_edges_parity(variant, kind, preceding):
    """Host push and device push, one final watermark.  Bounded MAX is held to the frame's true maximum in
    Double.compare order (the documented deviation: the reference keeps a NaN that has left the frame,
    tests/test_over_ref.py::test_bounded_max_keeps_a_stale_nan_after_its_retraction); everything else to the
    restatement."""
    exp = E.expected(variant, kind, preceding)
    _, rstats = E.restated(variant, kind, preceding)
    for device in (False, True):
        op = gpu_op(kind, preceding)
        got = run(op, variant, "final", device=device)
        st = op.stats()
        op.close()
        E.same_rows_bits(got, exp)
        for f in ("rows_kept", "late_rows_dropped", "keys", "retained_rows", "pending_rows"):
            assert st[f] == rstats[f], (f, st[f], rstats[f])


# ---------------------------------------------------------------- 2. cadence independence
@pytest.mark.parametrize("kind,preceding", E.FRAMES, ids=E.FRAME_IDS)
@pytest.mark.parametrize("variant", E.VARIANTS)
def test_gpu_over_edges_cadence_independence(variant, kind, preceding):
    """The same pushes fired by one final watermark, by a watermark after every push and by a watermark at every 37th
    row time: a key's rows, concatenated over the watermarks, are the same bits, and the restatement's."""
    exp = E.expected(variant, kind, preceding)
    runs = []
    for cadence in ("final", "every_push", "every_37"):
        op = gpu_op(kind, preceding)
        runs.append(per_key(run(op, variant, cadence)))
        op.close()
    # against the expectation first (a NaN sum matches as a class), then bit for bit among themselves
    for r in runs:
        E.same_rows_bits(r, exp)
    for r in runs[1:]:
        for f in ("key", "rowtime", "ordinal", "null_mask"):
            assert np.array_equal(r[f], runs[0][f]), f
        live = ((runs[0]["null_mask"][:, None] >> np.arange(len(E.AGGS))[None, :]) & 1) == 0
        assert np.array_equal(r["values"][live], runs[0]["values"][live])


def _one_key(kind, preceding, values, wms, fns=("sum", "avg", "min", "max")):
    op = gpu_op(kind, preceding, ["double"], [(f, 0) for f in fns])
    n = len(values)
    op.process(np.ones(n, np.int64), np.arange(1, n + 1, dtype=np.int64), [np.array(values, dtype=np.float64)])
    got = E.concat(fire(op, wms))
    op.close()
    assert got["rowtime"].tolist() == list(range(1, n + 1)) and not got["null_mask"].any()
    return {f: ["nan" if E._is_nan(np.int64(v)) else int(v) for v in got["values"][:, q]] for q, f in enumerate(fns)}


def _bits(v):
    return int(np.float64(v).view(np.int64))


CADENCES4 = [[LMAX], [3, LMAX], [1, 2, 3, LMAX], [2, 4]]


@pytest.mark.parametrize("wms", CADENCES4, ids=["one", "after-third", "every-row", "pairs"])
def test_gpu_over_rows_1_preceding_over_nan_1_2_3(wms):
    """The sum is NaN in all four rows however the watermarks batch the timers (the answers:
    tests/test_over_ref.py::test_bounded_max_keeps_a_stale_nan_after_its_retraction); MAX is the frame's own."""
    got = _one_key("bounded_rows", 1, [np.nan, 1.0, 2.0, 3.0], wms)
    assert got["sum"] == ["nan"] * 4 and got["avg"] == ["nan"] * 4
    assert got["min"] == ["nan", _bits(1.0), _bits(1.0), _bits(2.0)]
    assert got["max"] == ["nan", "nan", _bits(2.0), _bits(3.0)]
    raw = _one_key("bounded_rows", 1, [E.NEG_NAN, 1.0, 2.0, 3.0], wms, fns=("min", "max"))
    assert raw == {"min": got["min"], "max": got["max"]}


@pytest.mark.parametrize("wms", [[LMAX], [2, LMAX], [3, LMAX], [1, 2, 3, 4, 5]], ids=["one", "2", "3", "every-row"])
def test_gpu_over_sticky_sums_of_one_key(wms):
    """tests/test_over_ref.py::test_a_retracted_infinity_leaves_a_sticky_nan and
    ::test_an_overflowed_sum_is_a_sticky_infinity on the GPU, under every cadence"""
    inf, pinf = np.inf, _bits(np.inf)
    assert _one_key("bounded_rows", 1, [inf, 1.0, 2.0, 3.0, 4.0], wms)["sum"] == [pinf, pinf, "nan", "nan", "nan"]
    assert _one_key("bounded_range", 0, [inf, 1.0, 2.0, 3.0, 4.0], wms)["sum"] == [pinf] + ["nan"] * 4
    assert _one_key("bounded_rows", 1, [inf, -inf, 2.0, 3.0, 4.0], wms)["sum"] == [pinf] + ["nan"] * 4
    assert _one_key("bounded_rows", 1, [-inf, 1.0, 2.0, 3.0, 4.0], wms)["sum"] == [_bits(-inf)] * 2 + ["nan"] * 3
    got = _one_key("bounded_rows", 1, [DBL_MAX, DBL_MAX, 1.0, 2.0, 3.0], wms)
    assert got["sum"] == [_bits(DBL_MAX)] + [pinf] * 4 and got["avg"] == got["sum"]
    assert got["max"] == [_bits(DBL_MAX)] * 3 + [_bits(2.0), _bits(3.0)]
    assert _one_key("bounded_rows", 1, [DBL_MAX, DBL_MAX, 1.0, -inf, 3.0], wms)["sum"] == [_bits(DBL_MAX), pinf, pinf, "nan", "nan"]
    for kind in ("unbounded_rows", "unbounded_range"):
        assert _one_key(kind, 0, [inf, 1.0, 2.0, 3.0, 4.0], wms)["sum"] == [pinf] * 5
    # zero signs: a sum is 0.0 + ..., never -0.0; MIN takes -0.0 and MAX +0.0 in either arrival order
    for kind in ("bounded_rows", "bounded_range", "unbounded_rows", "unbounded_range"):
        got = _one_key(kind, 1, [-0.0, -0.0, -0.0, 0.0, -0.0], wms)
        assert got["sum"] == [0] * 5 and got["avg"] == [0] * 5, (kind, got)
        if kind != "bounded_range":
            assert got["min"] == [NEG_ZERO_BITS] * 5 and got["max"][3:] == [0, 0] and got["max"][:3] == [NEG_ZERO_BITS] * 3


# ---------------------------------------------------------------- 3. state
@pytest.mark.parametrize("kind,preceding", E.FRAMES, ids=E.FRAME_IDS)
@pytest.mark.parametrize("variant", ["nan", "dbl_max_twice"])
def test_gpu_over_edges_snapshot_restore(variant, kind, preceding):
    """Five pushes, a snapshot of every key group, a restore into a fresh handle that is handed the watermark again,
    three more pushes: the continuation is the uninterrupted run's, bit for bit.  By then key 0's sum has been NaN
    ("nan") or +Inf ("dbl_max_twice") since its first rows, and the last special before the cut (run position 4097,
    4098) has left a bounded key's retained rows (row 5100 or so is the last one fired)."""
    cut = 5
    whole = gpu_op(kind, preceding, max_parallelism=MAX_PAR)
    run(whole, variant, "every_push", last=cut)
    exp = run(whole, variant, "every_push", first=cut)
    whole.close()
    src = gpu_op(kind, preceding, max_parallelism=MAX_PAR)
    run(src, variant, "every_push", last=cut)
    snaps = {kg: src.snapshot(kg) for kg in range(MAX_PAR)}
    assert sum(len(s["key"]) for s in snaps.values()) == src.stats()["keys"]
    src.close()
    # key 0's state: the words of its Double column (rows, then per column count, sum, .., min, max)
    s0 = next(s for s in snaps.values() if E.LONG_KEY in s["key"])
    i = int(np.flatnonzero(s0["key"] == E.LONG_KEY)[0])
    word = np.int64(s0["acc"][i, 2])
    if variant == "nan":
        assert E._is_nan(word)
    else:
        assert int(word) == E.INF_BITS
    if kind.startswith("bounded"):
        a = int(s0["n_rows"][:i].sum())
        kept = s0["cols"][a:a + int(s0["n_rows"][i]), 0]
        assert len(kept) > 0 and ((kept & E.INF_BITS) != E.INF_BITS).all() and (np.abs(kept.view(np.float64)) <= 1024).all()
        # a key whose sum is finite carries nothing: its words are the zeros the handle wrote before it kept a carry
        for s in snaps.values():
            sums = s["acc"][:, 2]
            assert ((sums == 0) | ((sums & E.INF_BITS) == E.INF_BITS)).all()
            assert (np.delete(s["acc"], 2, axis=1) == 0).all()
    dst = gpu_op(kind, preceding, max_parallelism=MAX_PAR)
    for kg, s in snaps.items():
        dst.restore(kg, s)
    assert dst.advance_watermark(E.cadence_watermarks(variant, "every_push")[cut - 1][-1]) == 0
    got = run(dst, variant, "every_push", first=cut)
    dst.close()
    assert len(got["key"]) > 4000
    # ordinals restart after the largest restored one; everything else is the same bits
    for f in ("key", "rowtime", "null_mask"):
        assert np.array_equal(got[f], exp[f]), f
    live = ((exp["null_mask"][:, None] >> np.arange(len(E.AGGS))[None, :]) & 1) == 0
    assert np.array_equal(got["values"][live], exp["values"][live])
    full = E.expected(variant, kind, preceding)
    tail = np.isin(full["ordinal"], exp["ordinal"])
    E.same_rows_bits(exp, {f: full[f][tail] for f in FIELDS})


@pytest.mark.parametrize("kind,preceding", [("bounded_rows", 5), ("bounded_range", 50)])
def test_gpu_over_a_snapshot_without_a_carry_restores_as_before(kind, preceding):
    """The layout did not change: a bounded key's accumulator words of a snapshot taken over finite sums are all zero,
    as every snapshot written before the carry was (the restore then set them to zero itself), and restoring such a
    snapshot continues the uninterrupted run bit for bit."""
    from tests.over_util import seeded_stream
    steps = [(s[0], s[1], s[2], [s[3][4]], (s[4] >> 4) & 1) if s[0] == "p" else s
             for s in seeded_stream(61, n=4000, pushes=4, nkeys=37)]
    types, aggs = ["double"], [("sum", 0), ("avg", 0), ("min", 0), ("max", 0), ("count_star", 0)]

    def play(op, part):
        out = []
        for s in part:
            if s[0] == "p":
                op.process(s[1], s[2], s[3], s[4])
            else:
                op.advance_watermark(s[1])
                out.append(op.drain_arrays())
        return E.concat(out) if out else None
    whole = gpu_op(kind, preceding, types, aggs, max_parallelism=MAX_PAR)
    play(whole, steps[:4])
    exp = play(whole, steps[4:])
    whole.close()
    src = gpu_op(kind, preceding, types, aggs, max_parallelism=MAX_PAR)
    play(src, steps[:4])
    snaps = {kg: src.snapshot(kg) for kg in range(MAX_PAR)}
    src.close()
    assert sum(len(s["key"]) for s in snaps.values()) == 37 and all((s["acc"] == 0).all() for s in snaps.values())
    dst = gpu_op(kind, preceding, types, aggs, max_parallelism=MAX_PAR)
    for kg, s in snaps.items():
        dst.restore(kg, s)
    lead = E.concat(fire(dst, [steps[3][1]]))    # a bounded key's rows behind the watermark fire here
    got = play(dst, steps[4:])
    dst.close()
    got = per_key(E.concat([lead, got]))
    exp = per_key(exp)
    assert len(exp["key"]) > 1000
    for f in ("key", "rowtime", "values", "null_mask"):
        assert np.array_equal(got[f], exp[f]), f


# ---------------------------------------------------------------- 4. the ends of the row-time range
def _replay(kind, preceding, steps, types=E.TYPES, aggs=E.AGGS):
    """steps ("p", keys, ts) / ("w", wm) through the handle and the restatement; values from the rows' index"""
    op, ref = gpu_op(kind, preceding, types, aggs), OverRef(kind, preceding, types, aggs)
    got, exp, base = [], [], 0
    for s in steps:
        if s[0] == "p":
            keys, ts = np.array(s[1], dtype=np.int64), np.array(s[2], dtype=np.int64)
            i = base + np.arange(len(keys), dtype=np.int64)
            base += len(keys)
            cols = [((i * 37) % 129 - 64) / 8.0, (((i * 11) % 65 - 32) / 4.0).astype(np.float32), (i * 7919) % 2001 - 1000]
            nulls = ((i % 5 == 0).astype(np.uint8)) | ((i % 7 == 0).astype(np.uint8) << 1)
            op.process(keys, ts, cols, nulls)
            ref.process(keys, ts, cols, nulls)
        else:
            got += fire(op, [s[1]])
            exp += ref.watermark(s[1])
    st = op.stats()
    op.close()
    return E.concat(got), E.rows_to_arrays(exp, aggs), st, ref.stats()


@pytest.mark.parametrize("kind", ["unbounded_rows", "unbounded_range"])
def test_gpu_over_unbounded_negative_row_times(kind):
    """tests/test_over_ref.py::test_unbounded_accepts_negative_row_times_at_first on the GPU: row times down to
    Long.MIN_VALUE + 1, watermarks from Long.MIN_VALUE + 1 through 0 to Long.MAX_VALUE, rows exactly at the watermark
    (late) and one above it (kept)."""
    lo = LMIN + 1
    ks = [3, 4, 3, 5, 4, 3]
    steps = [("p", ks * 2, [lo, lo, lo + 1, lo + 2, -(1 << 62), -5] + [-1, 0, 1, 1 << 62, LMAX - 1, LMAX])]
    for wm in (lo, lo + 1, -(1 << 62), -1, 0, 1 << 62, LMAX - 1):
        steps += [("w", wm), ("p", [3, 4, 5, 3, 4, 5], [wm, wm, wm, wm + 1, wm + 1, wm + 1])]
    steps += [("w", LMAX)]
    got, exp, st, rs = _replay(kind, 0, steps)
    E.same_rows_bits(got, exp)
    assert st["late_rows_dropped"] == rs["late_rows_dropped"] >= 18 and st["rows_kept"] == rs["rows_kept"] >= 30
    assert st["keys"] == rs["keys"] == 3 and st["pending_rows"] == 0
    assert (got["rowtime"] < 0).sum() >= 12 and got["rowtime"].min() == lo and got["rowtime"].max() == LMAX


@pytest.mark.parametrize("kind,preceding", [("bounded_rows", 2), ("bounded_range", 2), ("bounded_range", LMAX)])
def test_gpu_over_bounded_row_time_ends(kind, preceding):
    """Row times <= 0 are late for a fresh bounded key and claim no key; RANGE frames within 3 ms of Long.MAX_VALUE
    with `preceding` 2 and Long.MAX_VALUE (the unsigned distance in the frame search)."""
    steps = [("p", [1, 1, 2, 2, 2, 3, 4, 4], [0, -1, LMIN + 1, -(1 << 62), 5, 0, 1, -7]),   # keys 1, 3: late rows only
             ("w", 4),
             ("p", [2, 4, 2, 4, 2, 4, 2, 4, 2, 2], [1, 1, LMAX - 3, LMAX - 3, LMAX - 2, LMAX - 1, LMAX - 1, LMAX, LMAX, LMAX]),
             ("w", LMAX - 2),
             ("p", [2, 4, 2, 5], [LMAX - 2, LMAX - 1, LMAX, LMAX]),       # key 2's LMAX - 2: at its last fired row time
             ("w", LMAX)]
    got, exp, st, rs = _replay(kind, preceding, steps)
    E.same_rows_bits(got, exp)
    for f in ("rows_kept", "late_rows_dropped", "keys", "retained_rows", "pending_rows"):
        assert st[f] == rs[f], (f, st[f], rs[f])
    assert st["keys"] == 3 and st["late_rows_dropped"] >= 7   # keys 1 and 3 claimed nothing
    assert (got["rowtime"] >= LMAX - 3).sum() >= 9
    star = [q for q, (f, _) in enumerate(E.AGGS) if f == "count_star"][0]
    if preceding == LMAX:   # a frame from row time 1 to Long.MAX_VALUE
        assert got["values"][(got["key"] == 2) & (got["rowtime"] == LMAX), star].max() >= 8

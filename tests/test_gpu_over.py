"""Row-time OVER windows on the GPU (flink_amd/over.py -> fw_over.hip) against the reference's own tests, the
sequential restatement tests/over_ref.py and, for long runs, frames evaluated directly (tests/over_util.py)."""
import functools

import numpy as np
import pytest

from flink_amd import _native as N
from flink_amd.keygroups import (assign_to_key_group, compute_key_group_range_for_operator_index, long_hash_code)
from flink_amd.over import Over, OverAggregate
from tests.over_ref import LMAX, OverRef
from tests.over_util import (AGGS16, KINDS, TYPES5, assert_same_rows, brute_frames, check_kat, load_kats, replay_kat,
                             run_steps, seeded_stream)
from tests.parity_util import F64_RTOL

pytestmark = pytest.mark.gpu

KATS = load_kats()
PREC = {"bounded_rows": 5, "bounded_range": 50, "unbounded_rows": 0, "unbounded_range": 0}


def frame_of(kind, preceding):
    return {"bounded_rows": lambda: Over.rows(preceding), "bounded_range": lambda: Over.range(preceding),
            "unbounded_rows": Over.unbounded_rows, "unbounded_range": Over.unbounded_range}[kind]()


def gpu_op(kind, preceding, types, aggs, **kw):
    return OverAggregate(frame_of(kind, preceding), types, aggs, **kw)


class _Ref:
    def __init__(self, kind, preceding, types, aggs):
        self.r = OverRef(kind, preceding, types, aggs)

    def process(self, keys, rowtimes, columns, nulls=None):
        self.r.process(keys, rowtimes, columns, nulls)

    def watermark(self, wm):
        return self.r.watermark(wm)


# ---------------------------------------------------------------- 1. the reference's own tests
@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_gpu_over_kats(case):
    op = gpu_op(case["kind"], case["preceding"], case["column_types"], case["aggregates"], key_type=case["key_type"])
    check_kat(case, replay_kat(case, op))
    op.close()


# ---------------------------------------------------------------- 2. seeded parity
@functools.lru_cache(maxsize=None)
def _seeded(kind, zipf):
    steps = seeded_stream(11, nkeys=500 if zipf else 97, zipf=zipf)
    ref = _Ref(kind, PREC[kind], TYPES5, AGGS16)
    return steps, run_steps(ref, steps), ref.r.stats()


@pytest.mark.parametrize("zipf", [0.0, 1.1], ids=["uniform", "zipf"])
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_over_seeded_parity(kind, zipf):
    steps, exp, rstats = _seeded(kind, zipf)
    pushed = sum(len(s[1]) for s in steps if s[0] == "p")
    # on the reference's output alone: the configuration is not vacuous
    assert sum(len(w) for w in exp) >= 0.6 * pushed and rstats["late_rows_dropped"] >= 0.01 * pushed
    runs = []
    for _ in range(2):
        op = gpu_op(kind, PREC[kind], TYPES5, AGGS16)
        raw = []
        for s in steps:
            if s[0] == "p":
                op.process(s[1], s[2], s[3], s[4])
            else:
                op.advance_watermark(s[1])
                raw.append(op.drain_arrays())
        st = op.stats()
        op.close()
        runs.append(raw)
    for a, b in zip(*runs):  # the same input gives bit-identical output, Double sums included
        for f in ("key", "rowtime", "ordinal", "values", "null_mask", "epoch"):
            assert np.array_equal(a[f], b[f]), f
    for f in ("rows_kept", "late_rows_dropped", "keys", "retained_rows", "pending_rows"):
        assert st[f] == rstats[f], (f, st[f], rstats[f])
    op = gpu_op(kind, PREC[kind], TYPES5, AGGS16)
    got = run_steps(op, steps)
    op.close()
    assert len(got) == len(exp)
    for w, (g, e) in enumerate(zip(got, exp)):
        assert_same_rows(g, e, F64_RTOL)
    for w, a in enumerate(runs[0]):
        assert (a["epoch"] == w).all()


# ---------------------------------------------------------------- 3. run lengths and frames at the tile boundaries
RUNS = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 4096 + 1]
B_TYPES = ["long", "long", "long", "long"]
B_AGGS = [("count_star", 0), ("sum", 3), ("avg", 3), ("count", 3), ("min", 0), ("max", 0), ("min", 1), ("max", 1),
          ("min", 2), ("max", 2), ("min", 3), ("max", 3)]


@functools.lru_cache(maxsize=None)
def _boundary_stream():
    """One key per run length.  Row times: distinct in the even keys, peer groups of 3 in the odd ones, and in the
    longest key one peer group of 5000 rows; arrival order shuffled.  Columns: strictly increasing and strictly
    decreasing in (rowtime, arrival) order, constant, and random with NULLs."""
    rng = np.random.default_rng(3)
    keys, ts = [], []
    for k, m in enumerate(RUNS):
        keys.append(np.full(m, k + 1, dtype=np.int64))
        t = 1 + (np.arange(m, dtype=np.int64) if k % 2 == 0 else np.arange(m, dtype=np.int64) // 3)
        if m == RUNS[-1]:
            t = np.r_[np.arange(1, 3001), np.full(5000, 3001), np.arange(3002, 3002 + m - 8000)].astype(np.int64)
        ts.append(t)
    keys, ts = np.concatenate(keys), np.concatenate(ts)
    p = rng.permutation(len(keys))
    keys, ts = keys[p], ts[p]
    n = len(keys)
    inc = ts * 100000 + np.arange(n, dtype=np.int64)
    cols = [inc, -inc, np.full(n, 7, dtype=np.int64), rng.integers(-(1 << 62), 1 << 62, size=n, dtype=np.int64)]
    nulls = (rng.random(n) < 0.3).astype(np.uint8) << 3
    return keys, ts, cols, nulls


@functools.lru_cache(maxsize=None)
def _boundary_expected(kind, preceding):
    keys, ts, cols, nulls = _boundary_stream()
    return brute_frames(kind, preceding, keys, ts, cols, nulls, B_AGGS)


@pytest.mark.parametrize("kind,preceding", [("bounded_rows", n) for n in (0, 1, 2, 63, 64, 4095, 4096, 4097, 10000)] +
                         [("bounded_range", t) for t in (0, 1, 9000)] + [("unbounded_rows", 0), ("unbounded_range", 0)])
def test_gpu_over_tile_boundaries(kind, preceding):
    keys, ts, cols, nulls = _boundary_stream()
    assert len(keys) <= 1 << 16
    op = gpu_op(kind, preceding, B_TYPES, B_AGGS)
    op.process(keys, ts, cols, nulls)
    got = op.watermark(LMAX)
    op.close()
    assert_same_rows(got, _boundary_expected(kind, preceding), 0.0)


@pytest.mark.parametrize("kind", KINDS)
def test_gpu_over_one_row_per_key(kind):
    n = 1 << 16
    rng = np.random.default_rng(8)
    keys = rng.permutation(n).astype(np.int64) * 7919 - 12345
    ts = rng.integers(1, 1000, size=n, dtype=np.int64)
    v = rng.integers(-(1 << 62), 1 << 62, size=n, dtype=np.int64)
    op = gpu_op(kind, 3, ["long"], [("count_star", 0), ("sum", 0), ("avg", 0), ("min", 0), ("max", 0)],
                expected_keys=n)
    op.process(keys, ts, [v])
    op.advance_watermark(LMAX)
    a = op.drain_arrays()
    assert op.stats()["keys"] == n
    op.close()
    assert len(a["key"]) == n and not a["null_mask"].any()
    o = np.argsort(a["ordinal"])
    assert np.array_equal(a["ordinal"][o], np.arange(n)) and np.array_equal(a["key"][o], keys)
    assert np.array_equal(a["rowtime"][o], ts)
    assert (a["values"][o][:, 0] == 1).all()
    for q in range(1, 5):
        assert np.array_equal(a["values"][o][:, q], v), q


@pytest.mark.parametrize("kind,preceding", [("bounded_rows", 100), ("bounded_rows", 5000), ("bounded_rows", 40000),
                                            ("bounded_range", 300), ("bounded_range", 20000),
                                            ("unbounded_rows", 0), ("unbounded_range", 0)])
def test_gpu_over_one_key_holds_every_row(kind, preceding):
    """The non-partitioned OVER: 2^16 rows of one key, half fired (and retained / accumulated) by an earlier
    watermark.  ROWS 40000 and RANGE 20000 (row times 1 .. 32768, two rows each) retain the whole first half: the
    second watermark's run is all 2^16 rows, the retained / firing boundary in its middle."""
    n, half = 1 << 16, 1 << 15
    rng = np.random.default_rng(9)
    ts = 1 + np.arange(n, dtype=np.int64) // 2          # peer pairs
    ts[:half] = ts[:half][rng.permutation(half)]
    ts[half:] = ts[half:][rng.permutation(half)]
    keys = np.full(n, 42, dtype=np.int64)
    cols = [ts * 100000 + np.arange(n), rng.integers(-(1 << 62), 1 << 62, size=n, dtype=np.int64)]
    cols[0] = cols[0].astype(np.int64)
    nulls = (rng.random(n) < 0.3).astype(np.uint8) << 1
    aggs = [("count_star", 0), ("sum", 1), ("avg", 1), ("min", 0), ("max", 0), ("min", 1), ("max", 1)]
    op = gpu_op(kind, preceding, ["long", "long"], aggs)
    op.process(keys[:half], ts[:half], [c[:half] for c in cols], nulls[:half])
    first = op.watermark(int(ts[:half].max()))
    mid = op.stats()
    op.process(keys[half:], ts[half:], [c[half:] for c in cols], nulls[half:])
    second = op.watermark(LMAX)
    st = op.stats()
    op.close()
    exp = brute_frames(kind, preceding, keys, ts, cols, nulls, aggs)
    cut = int(ts[:half].max())
    assert_same_rows(first, [r for r in exp if r[1] <= cut], 0.0)
    assert_same_rows(second, [r for r in exp if r[1] > cut], 0.0)
    assert st["late_rows_dropped"] == 0 and st["pending_rows"] == 0 and st["keys"] == 1
    # retained: ROWS the key's last N + 1 fired rows; RANGE the rows within t of the last fired row time (two rows
    # per row time; the first watermark's is 16384, the last one's 32768); the unbounded kinds keep the accumulator
    if kind == "bounded_rows":
        assert mid["retained_rows"] == min(half, preceding + 1) and st["retained_rows"] == preceding + 1
    elif kind == "bounded_range":
        assert mid["retained_rows"] == 2 * min(16384, preceding + 1) and st["retained_rows"] == 2 * (preceding + 1)
    else:
        assert mid["retained_rows"] == 0 and st["retained_rows"] == 0
    if preceding >= 20000:
        assert mid["retained_rows"] == half


# ---------------------------------------------------------------- 4. state
S_TYPES = ["long", "int", "double"]
S_AGGS = [("count_star", 0), ("sum", 0), ("avg", 0), ("min", 0), ("max", 1), ("sum", 1), ("count", 1), ("sum", 2),
          ("max", 2)]
MAX_PAR = 16


def _state_steps():
    steps = seeded_stream(21, n=6000, pushes=6, nkeys=61)
    return [(s[0], s[1], s[2], [s[3][0], s[3][1], s[3][4]], (s[4] & 3) | ((s[4] >> 2) & 4)) if s[0] == "p" else s
            for s in steps]


@pytest.mark.parametrize("par", [1, 2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_over_snapshot_restore_rescale(kind, par):
    steps = _state_steps()
    cut = 6  # three pushes and watermarks in
    whole = gpu_op(kind, PREC[kind], S_TYPES, S_AGGS, max_parallelism=MAX_PAR)
    exp = run_steps(whole, steps)
    whole.close()
    src = gpu_op(kind, PREC[kind], S_TYPES, S_AGGS, max_parallelism=MAX_PAR)
    run_steps(src, steps[:cut])
    snaps = {kg: src.snapshot(kg) for kg in range(MAX_PAR)}
    assert sum(len(s["key"]) for s in snaps.values()) == src.stats()["keys"]
    assert sum(len(s["ts"]) for s in snaps.values()) == src.stats()["retained_rows"] + src.stats()["pending_rows"]
    src.close()
    ops, owner = [], {}
    for i in range(par):
        r = compute_key_group_range_for_operator_index(MAX_PAR, par, i)
        lo, hi = r.start_key_group, r.end_key_group
        op = gpu_op(kind, PREC[kind], S_TYPES, S_AGGS, max_parallelism=MAX_PAR, key_group_range=(lo, hi))
        for kg in range(lo, hi + 1):
            op.restore(kg, snaps[kg])
            owner[kg] = i
        ops.append(op)
    # the watermark is not keyed state: a restored operator starts at Long.MIN_VALUE, as the reference's timer service
    # does, and the host hands it the job's watermark again before the stream continues.  Rows this fires (a bounded
    # key's rows behind the watermark) lead the next watermark's, where the uninterrupted run emits them.
    carry = [r for op in ops for r in op.watermark(steps[cut - 1][1])]
    kg_of = {}
    got = []
    for s in steps[cut:]:
        if s[0] == "p":
            for k in np.unique(s[1]):
                kg_of.setdefault(int(k), assign_to_key_group(long_hash_code(int(k)), MAX_PAR))
            dest = np.array([owner[kg_of[int(k)]] for k in s[1]])
            for i, op in enumerate(ops):
                m = dest == i
                op.process(s[1][m], s[2][m], [c[m] for c in s[3]], s[4][m])
        else:
            got.append(carry + [r for op in ops for r in op.watermark(s[1])])
            carry = []
    restored_max = max((int(s["ordinal"].max()) for s in snaps.values() if len(s["ordinal"])), default=-1)
    for g, e in zip(got, exp[cut // 2:]):
        assert_same_rows(g, e, F64_RTOL, ordinals=False)
    assert len(got) == len(exp) - cut // 2 and sum(len(g) for g in got) > 1000
    # later pushes are numbered after the largest restored ordinal
    seen = set()
    for sn in snaps.values():
        seen |= set(zip(np.repeat(sn["key"], sn["n_rows"]).tolist(), sn["ts"].tolist(), sn["ordinal"].tolist()))
    if par == 1:
        for g in got:
            for key, rowtime, ordinal, _ in g:
                assert (key, rowtime, ordinal) in seen or ordinal > restored_max
    for op in ops:
        op.close()


def test_gpu_over_restore_refuses_a_key_with_state():
    steps = _state_steps()
    src = gpu_op("bounded_range", 50, S_TYPES, S_AGGS, max_parallelism=MAX_PAR)
    run_steps(src, steps[:4])
    kg = next(k for k in range(MAX_PAR) if len(src.snapshot(k)["key"]))
    snap = src.snapshot(kg)
    dst = gpu_op("bounded_range", 50, S_TYPES, S_AGGS, max_parallelism=MAX_PAR)
    dst.restore(kg, snap)
    before = dst.stats()
    with pytest.raises(N.NativeError) as e:
        dst.restore(kg, snap)
    assert e.value.code == N.FW_ERR_STATE and "already has state" in str(e.value)
    assert dst.stats() == before
    with pytest.raises(N.NativeError) as e:  # and a live handle refuses its own keys
        src.restore(kg, snap)
    assert e.value.code == N.FW_ERR_STATE
    other = (kg + 1) % MAX_PAR
    with pytest.raises(N.NativeError) as e:  # a Long key restored into a key group that is not its own
        dst.restore(other, snap)
    assert e.value.code == N.FW_ERR_KEY_GROUP
    src.close()
    dst.close()


@pytest.mark.parametrize("kind", KINDS)
def test_gpu_over_watermark_below_every_pending_row(kind):
    op = gpu_op(kind, PREC[kind], ["long"], [("sum", 0)])
    op.process(np.array([1, 2, 1]), np.array([500, 700, 600]), [np.array([1, 2, 3])])
    before = op.stats()
    assert op.watermark(499) == []
    after = op.stats()
    assert {**after, "current_watermark": 0} == {**before, "current_watermark": 0} and after["pending_rows"] == 3
    assert [r[:3] for r in op.watermark(500)] == [(1, 500, 0)]
    with pytest.raises(N.NativeError) as e:
        op.watermark(10)
    assert e.value.code == N.FW_ERR_ARG and "lower than" in str(e.value)
    with pytest.raises(N.NativeError) as e:
        op.process(np.array([1, 1]), np.array([900, -(1 << 63)]), [np.array([1, 2])])
    assert e.value.code == N.FW_ERR_NO_TIMESTAMP
    assert op.stats()["pending_rows"] == 2 and op.stats()["rows_kept"] == 3  # the refused push changed nothing
    assert sorted(r[:3] for r in op.watermark(LMAX)) == [(1, 600, 2), (2, 700, 1)]
    op.close()


@pytest.mark.parametrize("kind", KINDS)
def test_gpu_over_growth_keeps_parity(kind):
    # a store of 1024 rows and a key map of 1024 keys at creation; the stream holds 3000 keys and 9000 rows
    steps = seeded_stream(31, n=9000, pushes=3, nkeys=3000, jitter=1200, lag=200)
    ref = _Ref(kind, PREC[kind], TYPES5, AGGS16)
    exp = run_steps(ref, steps)
    op = gpu_op(kind, PREC[kind], TYPES5, AGGS16, expected_keys=1, max_batch=1024)
    got = run_steps(op, steps)
    st = op.stats()
    op.close()
    for g, e in zip(got, exp):
        assert_same_rows(g, e, F64_RTOL)
    rs = ref.r.stats()
    assert st["keys"] == rs["keys"] > 1024 and st["late_rows_dropped"] == rs["late_rows_dropped"] > 0
    assert st["rows_kept"] == rs["rows_kept"] > 1024


def test_gpu_over_key_group_range_is_enforced():
    op = gpu_op("unbounded_rows", 0, ["long"], [("sum", 0)], max_parallelism=MAX_PAR, key_group_range=(0, 3))
    ks = np.arange(1, 200, dtype=np.int64)
    inside = np.array([assign_to_key_group(long_hash_code(int(k)), MAX_PAR) <= 3 for k in ks])
    op.process(ks[inside], np.full(int(inside.sum()), 5), [ks[inside]])
    with pytest.raises(N.NativeError) as e:
        op.process(ks, np.full(len(ks), 5), [ks])
    assert e.value.code == N.FW_ERR_KEY_GROUP
    assert op.stats()["rows_kept"] == int(inside.sum())
    assert len(op.watermark(LMAX)) == int(inside.sum())
    op.close()


@pytest.mark.parametrize("kind", KINDS)
def test_gpu_over_device_push_matches_host_push(kind):
    # fw_over_push_batch_device (columns in HBM) against fw_over_push_batch: the same rows, bit for bit
    import torch
    steps = seeded_stream(41, n=4000, pushes=4, nkeys=53)
    host = gpu_op(kind, PREC[kind], TYPES5, AGGS16)
    exp = run_steps(host, steps)
    host.close()
    dev = gpu_op(kind, PREC[kind], TYPES5, AGGS16)
    got = []
    for s in steps:
        if s[0] == "p":
            cols = torch.stack([torch.from_numpy(np.ascontiguousarray(c).view(np.int64).copy()) for c in s[3]]).cuda()
            dev.process(torch.from_numpy(s[1].copy()).cuda(), torch.from_numpy(s[2].copy()).cuda(), cols,
                        torch.from_numpy(s[4].copy()).cuda())
        else:
            got.append(dev.watermark(s[1]))
    dev.close()
    assert got == exp and sum(len(w) for w in got) > 2400


# ---------------------------------------------------------------- 5. floating order keys, the device view
F_TYPES = ["double", "float", "long"]
F_AGGS = [("min", 0), ("max", 0), ("sum", 0), ("avg", 0), ("count", 0), ("min", 1), ("max", 1), ("count", 1),
          ("count_star", 0), ("sum", 2)]


@pytest.mark.parametrize("kind", KINDS)
def test_gpu_over_mixed_sign_doubles_and_floats(kind):
    """Double and Float MIN / MAX over values of both signs (the order key's negative branch, and its complement for
    MAX); the Float column goes in as a float32 array.  Mixed-sign sums cancel, so a tolerance relative to the result
    would measure the cancellation, not the code: SUM / AVG are held to the forward error bound of a summation,
    |got - exp| <= rtol * (the same aggregate over |x|), which a second run of the reference over |x| supplies."""
    rng = np.random.default_rng(17)
    n = 4000
    keys = rng.integers(1, 30, size=n, dtype=np.int64)
    ts = 1 + np.arange(n, dtype=np.int64) // 3 - rng.integers(0, 40, size=n, dtype=np.int64)
    ts = np.maximum(ts, 1)
    d = rng.uniform(-1000.0, 1000.0, size=n)
    f = rng.uniform(-1000.0, 1000.0, size=n).astype(np.float32)
    v = rng.integers(-1000, 1000, size=n, dtype=np.int64)
    nulls = ((rng.random(n) < 0.2).astype(np.uint8)) | ((rng.random(n) < 0.2).astype(np.uint8) << 1)
    half = n // 2
    steps = [("p", keys[:half], ts[:half], [d[:half], f[:half], v[:half]], nulls[:half]), ("w", int(ts[:half].max()) - 20),
             ("p", keys[half:], ts[half:], [d[half:], f[half:], v[half:]], nulls[half:]), ("w", LMAX)]
    ref = _Ref(kind, PREC[kind], F_TYPES, F_AGGS)
    exp = run_steps(ref, steps)
    mag = _Ref(kind, PREC[kind], F_TYPES, F_AGGS)
    mags = run_steps(mag, [(s[0], s[1], s[2], [np.abs(s[3][0]), s[3][1], s[3][2]], s[4]) if s[0] == "p" else s
                           for s in steps])
    op = gpu_op(kind, PREC[kind], F_TYPES, F_AGGS)
    got = run_steps(op, steps)
    op.close()
    assert sum(len(w) for w in exp) > 0.6 * n
    negative = {0: False, 1: False, 5: False, 6: False}  # a negative Double / Float MIN and MAX each occur
    for g, e, m in zip(got, exp, mags):
        eg, ee, em = (sorted(x, key=lambda r: (r[0], r[1], r[2])) for x in (g, e, m))
        assert [r[:3] for r in eg] == [r[:3] for r in ee]
        for (_, _, _, gv), (_, _, _, ev), (_, _, _, mv) in zip(eg, ee, em):
            for q in (0, 1, 4, 5, 6, 7, 8, 9):  # MIN / MAX of both columns and the counts: exact
                assert gv[q] == ev[q] and type(gv[q]) is type(ev[q]), (q, gv, ev)
            for q in (2, 3):                    # SUM / AVG of the Double column
                if ev[q] is None:
                    assert gv[q] is None
                else:
                    assert abs(gv[q] - ev[q]) <= F64_RTOL * mv[q], (q, gv[q], ev[q], mv[q])
            for q in negative:
                negative[q] |= ev[q] is not None and ev[q] < 0
    assert all(negative.values()), negative


def test_gpu_over_device_view_and_clear_pending():
    """fw_over_rows_device hands out the pending rows where they are; fw_over_clear_pending drops them and their
    epoch tags."""
    import torch
    steps = seeded_stream(51, n=3000, pushes=3, nkeys=41)
    a = gpu_op("bounded_rows", 5, TYPES5, AGGS16)
    b = gpu_op("bounded_rows", 5, TYPES5, AGGS16)
    for s in steps[:4]:
        for op in (a, b):
            op.process(s[1], s[2], s[3], s[4]) if s[0] == "p" else op.advance_watermark(s[1])
    exp = b.drain_arrays()
    rows, n = a.rows_device()
    assert n == len(exp["key"]) > 500 and a.stats()["pending_output_rows"] == n
    class _View:  # a device column as torch reads it
        def __init__(self, ptr, shape, typestr):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}

    ns = len(AGGS16)
    for f, shape, typestr in (("key", (n,), "<i8"), ("rowtime", (n,), "<i8"), ("ordinal", (n,), "<i8"),
                              ("values", (n, ns), "<i8"), ("null_mask", (n,), "<i4")):
        host = torch.as_tensor(_View(getattr(rows, f), shape, typestr), device="cuda").cpu().numpy()
        assert np.array_equal(host.view(exp[f].dtype), exp[f]), f
    assert a.rows_device()[1] == n  # the view leaves the rows pending
    a.clear_pending()
    assert a.stats()["pending_output_rows"] == 0 and a.rows_device()[1] == 0
    for op in (a, b):
        op.process(*steps[4][1:])
        op.advance_watermark(steps[5][1])
    ga, gb = a.drain_arrays(), b.drain_arrays()
    for f in ("key", "rowtime", "ordinal", "values", "null_mask", "epoch"):
        assert np.array_equal(ga[f], gb[f]), f
    assert len(ga["key"]) > 0 and (ga["epoch"] == 2).all()  # only the third watermark call's rows, tagged as such
    a.close()
    b.close()


def _drain_some(op, cap):
    """fw_over_drain with room for `cap` rows: the rows it hands out (drain_arrays' fields)"""
    import ctypes
    ns = len(op.aggregates)
    out = {"key": np.full(cap, -7, np.int64), "rowtime": np.full(cap, -7, np.int64), "ordinal": np.full(cap, -7, np.int64),
           "values": np.full((cap, ns), -7, np.int64), "null_mask": np.full(cap, 7, np.uint32),
           "epoch": np.full(cap, -7, np.int64)}
    dst = N.FwOverRows(*(out[f].ctypes.data for f in ("key", "rowtime", "ordinal", "values", "null_mask")))
    got = ctypes.c_int64()
    op._check(N.lib().fw_over_drain(op._h, ctypes.byref(dst), out["epoch"].ctypes.data, cap, ctypes.byref(got)))
    assert 0 <= got.value <= cap
    return {f: a[:got.value] for f, a in out.items()}


def test_gpu_over_partial_drains_hand_out_the_rows_and_epochs_of_one_drain():
    """Three drains (less than the first watermark's rows, to the middle of the second's, the rest) return what one
    drain returns, epochs included.  13 rows of three keys fire in watermark calls of 4, 5 and 4 rows; three aggregates,
    so a row of `values` is wider than the other columns, and two rows whose SUM is NULL."""
    keys = np.array([5, -3, 9] * 4 + [5], np.int64)
    ts = np.arange(1, 14, dtype=np.int64)
    col = np.arange(100, 113, dtype=np.int64)
    nulls = np.zeros(13, np.uint8)
    nulls[[0, 3]] = 1  # key 5's first two rows
    aggs = [("sum", 0), ("count_star", 0), ("max", 0)]
    a, b = gpu_op("bounded_rows", 1, ["long"], aggs), gpu_op("bounded_rows", 1, ["long"], aggs)
    for op in (a, b):
        op.process(keys, ts, [col], nulls)
        assert [op.advance_watermark(wm) for wm in (4, 9, 13)] == [4, 5, 4]
    one = b.drain_arrays()
    assert one["epoch"].tolist() == [0] * 4 + [1] * 5 + [2] * 4
    assert sorted(one["rowtime"].tolist()) == ts.tolist() and np.count_nonzero(one["null_mask"]) == 2
    assert a.stats()["pending_output_rows"] == 13
    parts = []
    for cap, left in ((3, 10), (4, 6), (100, 0)):
        parts.append(_drain_some(a, cap))
        assert a.stats()["pending_output_rows"] == left
    assert [len(p["key"]) for p in parts] == [3, 4, 6]
    for f in one:
        assert np.array_equal(np.concatenate([p[f] for p in parts]), one[f]), f
    assert len(_drain_some(a, 5)["key"]) == 0 and len(b.drain_arrays()["key"]) == 0
    a.close()
    b.close()

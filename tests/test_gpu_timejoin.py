"""The time-windowed (interval) join on the GPU against the reference's harness sequences, the sequential restatement
(tests/timejoin_ref.py) and a numpy brute force.  Everything is integers and ordinals: comparisons are exact, rows as
sorted multisets per call, forwarded watermarks by position."""
import numpy as np
import pytest

from flink_amd import _native as N
from flink_amd.keygroups import assign_to_key_group, compute_key_group_range_for_operator_index, long_hash_code
from flink_amd.timejoin import TimeBoundedJoin

from .timejoin_ref import COUNTERS, LMAX
from .timejoin_util import (BOUNDS, JOIN_TYPES, RefEngine, brute_force_pairs, load_kats, make_stream, ref_run, replay_kat,
                            rows_as_tuples, segments, single_key_rows)

pytestmark = pytest.mark.gpu

KATS = load_kats()
SHARED_STATS = COUNTERS + ("store_rows", "active_timers", "current_watermark")
# fw_tjoin.hip TJ_CHUNK = TJ_THREADS * TJ_ITEMS: the candidates a workgroup of the pair pass takes per step
TJ_CHUNK = 256 * 4


class GpuEngine:
    """TimeBoundedJoin behind the interface of RefEngine: push() and watermark() return row tuples."""

    def __init__(self, join_type, lower, upper, allowed_lateness=0, device_push=False, **kw):
        self.op = TimeBoundedJoin(join_type, lower, upper, allowed_lateness, **kw)
        self.device_push = device_push

    def process(self, sides, keys, rowtimes, vals=None):
        sides = np.asarray(sides, np.uint8)
        keys = np.asarray(keys, np.int64)
        rowtimes = np.asarray(rowtimes, np.int64)
        vals = None if vals is None else np.asarray(vals, np.int64)
        if self.device_push:
            import torch
            dev = [None if a is None else torch.from_numpy(a).cuda() for a in (sides, keys, rowtimes, vals)]
            self.op.process(*dev)
        else:
            self.op.process(sides, keys, rowtimes, vals)

    def push(self, sides, keys, rowtimes, vals=None):
        self.process(sides, keys, rowtimes, vals)
        return rows_as_tuples(self.op.drain())

    def watermark(self, wm):
        rows, fw = self.op.watermark(wm)
        return rows_as_tuples(rows), fw

    def shared_stats(self):
        st = self.op.stats()
        return {f: st[f] for f in SHARED_STATS}


def ref_shared(ref):
    st = ref.stats()
    return {f: st[f] for f in SHARED_STATS}


def state_of(op, key_groups):
    """everything a refused call must leave alone"""
    snaps = [{f: a.tolist() for f, a in op.snapshot(kg).items()} for kg in key_groups]
    return op.stats(), snaps


def norm_state(st):
    """a snapshot as {key: (left_timer, right_timer, sorted rows)}"""
    out, r = {}, 0
    for i, key in enumerate(st["key"]):
        n = int(st["n_rows"][i])
        rows = sorted((int(st["side"][q]), int(st["rowtime"][q]), int(st["ordinal"][q]), int(st["val"][q]),
                       int(st["emitted"][q])) for q in range(r, r + n))
        r += n
        out[int(key)] = (int(st["left_timer"][i]), int(st["right_timer"][i]), rows)
    return out


# ---- the reference's harness sequences
@pytest.mark.parametrize("device_push", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_kat(case, device_push):
    eng = GpuEngine(case["join_type"], case["lower"], case["upper"], case["allowed_lateness"], device_push=device_push)
    gs, gw = segments(replay_kat(case, eng))
    es, ew = segments(case["expected"])
    assert gw == ew
    assert gs == es
    eng.op.close()


# ---- seeded parity
@pytest.mark.parametrize("kind", ["uniform", "zipf"])
@pytest.mark.parametrize("join_type", JOIN_TYPES)
def test_seeded_parity_with_the_restatement(join_type, kind):
    calls, fws, ref_stats = ref_run(join_type, kind)
    runs = []
    for device_push in (False, True):
        eng = GpuEngine(join_type, *BOUNDS, device_push=device_push)
        got, gfw = [], []
        for sides, keys, ts, vals, wm in make_stream(kind):
            eng.process(sides, keys, ts, vals)
            rows, fw = eng.watermark(wm)
            got.append(sorted(rows))
            gfw.append(fw)
        assert gfw == fws
        for q, (g, e) in enumerate(zip(got, calls)):
            assert g == e, f"call {q}: {len(g)} rows, expected {len(e)}"
        assert eng.shared_stats() == {f: ref_stats[f] for f in SHARED_STATS}
        runs.append(got)
        eng.op.close()
    assert runs[0] == runs[1]


# ---- one key holds every row
def check_pairs_against_brute_force(a, sides, ts, vals, lower, upper):
    exp = brute_force_pairs(sides, ts, lower, upper)
    assert len(a) == len(exp)
    o = np.lexsort((a["right_ord"], a["left_ord"]))
    assert np.array_equal(a["left_ord"][o], exp[:, 0]) and np.array_equal(a["right_ord"][o], exp[:, 1])
    assert (a["key"] == 42).all() and (a["timer_ts"] == -1).all()
    assert np.array_equal(a["cause_ord"], np.maximum(a["left_ord"], a["right_ord"]))
    for s in ("left", "right"):
        assert np.array_equal(a[s + "_rowtime"], ts[a[s + "_ord"]]) and np.array_equal(a[s + "_val"], vals[a[s + "_ord"]])
    return len(exp)


def test_one_key_holds_every_row_all_pairs():
    sides, keys, ts, vals = single_key_rows(1500)
    op = TimeBoundedJoin("inner", -10000, 10000)
    op.process(sides, keys, ts, vals)
    n = check_pairs_against_brute_force(op.drain(), sides, ts, vals, -10000, 10000)
    assert n == 1500 * 1500 and n > 1000 * TJ_CHUNK  # many steps of the pair pass
    op.close()


@pytest.mark.parametrize("split", [1, 2, 7])
def test_one_key_holds_every_row_few_partners(split):
    sides, keys, ts, vals = single_key_rows(1500)
    op = TimeBoundedJoin("inner", -6, 6)
    cuts = np.linspace(0, len(keys), split + 1).astype(int)
    for a, b in zip(cuts[:-1], cuts[1:]):
        op.process(sides[a:b], keys[a:b], ts[a:b], vals[a:b])
    n = check_pairs_against_brute_force(op.drain(), sides, ts, vals, -6, 6)
    assert 2 * 1500 < n < 5 * 1500  # 1500 * 1500 * 13 / 6000 = 4875 expected: about 3 partners per row
    op.close()


# ---- boundaries
def parity_one_push(join_type, lower, upper, sides, keys, ts, vals, **kw):
    eng = GpuEngine(join_type, lower, upper, **kw)
    ref = RefEngine(join_type, lower, upper)
    for e in (eng, ref):
        e.watermark(40)
    g = sorted(eng.push(sides, keys, ts, vals))
    assert g == sorted(ref.push(sides, keys, ts, vals))
    gr, gf = eng.watermark(LMAX)
    rr, rf = ref.watermark(LMAX)
    assert sorted(gr) == sorted(rr) and gf == rf
    assert eng.shared_stats() == ref_shared(ref.ref)
    eng.op.close()
    return len(g) + len(gr)


@pytest.mark.parametrize("one_key", [True, False], ids=["single_key", "one_row_per_key"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097])
def test_batch_size_boundaries(n, one_key):
    rng = np.random.default_rng(n)
    sides = rng.integers(0, 2, n).astype(np.uint8)
    keys = np.full(n, 9, np.int64) if one_key else np.arange(n, dtype=np.int64) * 31 - 7
    ts = rng.integers(0, min(max(n, 100), 600), n).astype(np.int64)  # some rows are late at watermark 40
    vals = rng.integers(-99, 99, n).astype(np.int64)
    # a small key map and store: 4097 keys and rows grow both
    assert parity_one_push("full", -2, 2, sides, keys, ts, vals, expected_keys=1, max_batch=1) >= n // 2


@pytest.mark.parametrize("new_vs_new", [False, True], ids=["store", "batch"])
@pytest.mark.parametrize("pairs", [TJ_CHUNK - 1, TJ_CHUNK, TJ_CHUNK + 1, 2 * TJ_CHUNK, 2 * TJ_CHUNK + 1])
def test_pair_total_at_the_emit_chunk(pairs, new_vs_new):
    """`pairs` right rows at one row time, then one left row that joins them all: the pair pass has exactly `pairs`
    candidates, from the store or from the same push"""
    op = TimeBoundedJoin("inner", 0, 0)
    k = np.full(pairs + 1, 3, np.int64)
    t = np.full(pairs + 1, 5, np.int64)
    s = np.array([1] * pairs + [0], np.uint8)
    v = np.arange(pairs + 1, dtype=np.int64)
    if new_vs_new:
        op.process(s, k, t, v)
    else:
        op.process(s[:-1], k[:-1], t[:-1], v[:-1])
        assert op.stats()["pending_output_rows"] == 0
        op.process(s[-1:], k[-1:], t[-1:], v[-1:])
    a = op.drain()
    assert len(a) == pairs and (a["left_ord"] == pairs).all() and (a["cause_ord"] == pairs).all()
    assert np.array_equal(np.sort(a["right_ord"]), np.arange(pairs)) and np.array_equal(a["right_val"], a["right_ord"])
    op.close()


def test_one_sided_and_empty_pushes():
    eng, ref = GpuEngine("full", -5, 9), RefEngine("full", -5, 9)
    rng = np.random.default_rng(5)
    z = np.zeros(0, np.int64)
    assert eng.push(np.zeros(0, np.uint8), z, z, z) == []
    for side in (0, 1, 0):  # only left rows, only right rows, left again
        keys = rng.integers(0, 20, 300).astype(np.int64)
        ts = rng.integers(0, 60, 300).astype(np.int64)
        s = np.full(300, side, np.uint8)
        assert sorted(eng.push(s, keys, ts, keys)) == sorted(ref.push(s, keys, ts, keys))
    assert eng.op.stats()["rows_in"] == 900
    g, r = eng.watermark(LMAX), ref.watermark(LMAX)
    assert sorted(g[0]) == sorted(r[0]) and g[1] == r[1] and eng.shared_stats() == ref_shared(ref.ref)
    eng.op.close()


# ---- refusals leave the state unchanged
def test_max_pairs():
    op = TimeBoundedJoin("inner", 0, 0, max_pairs=10, max_parallelism=4)
    rows = lambda n, side, t: (np.full(n, side, np.uint8), np.full(n, 1, np.int64), np.full(n, t, np.int64), None)  # noqa: E731
    op.process(*rows(5, 1, 7))
    op.process(*rows(1, 0, 7))       # 5 pairs pending
    op.process(*rows(6, 1, 8))
    before = state_of(op, range(4))
    with pytest.raises(N.NativeError) as e:
        op.process(*rows(1, 0, 8))   # 6 more: one over the limit
    assert e.value.code == N.FW_ERR_CAPACITY and "max_pairs" in str(e.value)
    assert state_of(op, range(4)) == before and before[0]["pending_output_rows"] == 5
    assert len(op.drain()) == 5
    op.process(*rows(1, 0, 8))       # the same push
    a = op.drain()
    assert len(a) == 6 and (a["left_ord"] == 12).all()  # the refused push took no ordinal
    op.close()


def test_per_push_refusals_leave_the_state_unchanged():
    kgr = (0, 1)
    op = TimeBoundedJoin("full", -10, 20, max_parallelism=4, key_group_range=kgr)
    inside = [k for k in range(200) if assign_to_key_group(long_hash_code(k), 4) in (0, 1)]
    outside = [k for k in range(200) if assign_to_key_group(long_hash_code(k), 4) in (2, 3)]
    rng = np.random.default_rng(3)
    keys = rng.choice(inside, 400).astype(np.int64)
    op.process(rng.integers(0, 2, 400).astype(np.uint8), keys, rng.integers(0, 200, 400).astype(np.int64), keys)
    op.advance_watermark(60)
    before = state_of(op, kgr)
    assert before[0]["store_rows"] > 0 and before[0]["pending_output_rows"] > 0
    good = ([0, 1, 0], [inside[0], inside[1], inside[2]], [100, 101, 102])
    for code, fragment, (i, column, value) in [
            (N.FW_ERR_TIME_RANGE, "[0, 2^62)", (1, 2, -1)),
            (N.FW_ERR_TIME_RANGE, "[0, 2^62)", (2, 2, 1 << 62)),
            (N.FW_ERR_KEY_GROUP, "KeyGroupRange", (0, 1, outside[0])),
            (N.FW_ERR_ARG, "side", (1, 0, 2))]:
        for device_push in (False, True):
            cols = [list(c) for c in good]
            cols[column][i] = value
            cols = [np.array(cols[0], np.uint8), np.array(cols[1], np.int64), np.array(cols[2], np.int64)]
            if device_push:
                import torch
                cols = [torch.from_numpy(c).cuda() for c in cols]
            with pytest.raises(N.NativeError) as e:
                op.process(*cols)
            assert e.value.code == code and fragment in str(e.value), str(e.value)
            assert state_of(op, kgr) == before
    op.process(np.array(good[0], np.uint8), np.array(good[1], np.int64), np.array(good[2], np.int64))
    assert op.stats()["rows_in"] == 403
    op.close()


def test_a_row_with_a_non_positive_clean_up_time_is_processed_as_the_reference_does():
    """With bounds (-10, -7) a right row at 2 has 2 - 7 + 1 + 0 + 1 <= 0; the reference's own harness sequence pushes
    such rows (testRowTimeInnerJoinWithNegativeBounds).  They are never cached, so no timer is registered for them."""
    eng, ref = GpuEngine("full", -10, -7), RefEngine("full", -10, -7)
    for e in (eng, ref):
        e.watermark(1)
    s, k, t = [1, 1, 0, 1, 0], [1, 1, 1, 1, 1], [2, 3, 3, 13, 6]
    assert sorted(eng.push(s, k, t, t)) == sorted(ref.push(s, k, t, t))
    assert eng.shared_stats() == ref_shared(ref.ref) and eng.op.stats()["rows_not_cached"] == 2
    g, r = eng.watermark(LMAX), ref.watermark(LMAX)
    assert sorted(g[0]) == sorted(r[0]) and g[1] == r[1]
    eng.op.close()


def test_watermarks_below_the_earliest_timer_and_lower_watermarks():
    op = TimeBoundedJoin("full", -5, 9, max_parallelism=4)
    op.process([0, 1], [1, 2], [100, 200], [1, 2])  # timers 113 and 217
    before = state_of(op, range(4))
    n, fw = op.advance_watermark(112)
    assert (n, fw) == (0, 103)
    after = state_of(op, range(4))
    assert after[1] == before[1] and after[0]["current_watermark"] == 112
    assert {**after[0], "current_watermark": 0} == {**before[0], "current_watermark": 0}
    with pytest.raises(N.NativeError) as e:
        op.advance_watermark(111)
    assert e.value.code == N.FW_ERR_ARG and "lower" in str(e.value)
    rows, fw = op.watermark(113)
    assert rows_as_tuples(rows) == [(1, 0, -1, 100, 0, 1, 0, -1, 113)] and fw == 104 and rows["epoch"].tolist() == [1]
    assert op.stats()["active_timers"] == 1
    op.close()


def test_gate_and_expired_row_scenario_in_one_batch_and_row_by_row():
    from .test_timejoin_ref import gate_scenario
    exp = gate_scenario(RefEngine("inner", -10, 20))
    assert len(exp) == 1
    for device_push in (False, True):
        eng = GpuEngine("inner", -10, 20, device_push=device_push)
        assert gate_scenario(eng) == exp
        st = eng.op.stats()
        assert st["pairs"] == 1 and st["pairs_with_expired_rows"] == 1 and st["gate_skips"] == 1
        eng.op.close()
    # the same rows one push each: the operator-wide expiration times carry over between pushes
    eng = GpuEngine("inner", -10, 20)
    eng.watermark(50)
    eng.push([0], [3], [45], [0])
    eng.push([1], [1], [100], [7])
    eng.push([1], [2], [100], [8])
    eng.watermark(130)
    got = []
    for k, t, v in ((1, 125, 1), (2, 95, 2), (2, 101, 3), (2, 102, 4)):
        got += eng.push([0], [k], [t], [v])
    assert got == exp and eng.op.stats()["gate_skips"] == 1
    eng.op.close()


# ---- growth
def test_key_map_and_store_growth_keep_parity():
    eng = GpuEngine("left", -20, 20, expected_keys=1, max_batch=1)
    ref = RefEngine("left", -20, 20)
    rng = np.random.default_rng(11)
    for q in range(4):  # 1500 new keys per push and 500 old ones: the map (1024 keys) and the store (1024 rows) grow
        keys = np.concatenate([np.arange(1500) + 1500 * q, rng.integers(0, 1500 * (q + 1), 500)]).astype(np.int64)
        rng.shuffle(keys)
        sides = rng.integers(0, 2, 2000).astype(np.uint8)
        ts = (100 * q + rng.integers(0, 150, 2000)).astype(np.int64)
        assert sorted(eng.push(sides, keys, ts, ts)) == sorted(ref.push(sides, keys, ts, ts))
        g, r = eng.watermark(100 * q + 30), ref.watermark(100 * q + 30)
        assert sorted(g[0]) == sorted(r[0]) and g[1] == r[1]
    assert eng.shared_stats() == ref_shared(ref.ref) and eng.op.stats()["store_rows"] > 1024
    eng.op.close()


# ---- keyed state
MAXPAR = 8


def kg_of(key):
    return assign_to_key_group(long_hash_code(int(key)), MAXPAR)


@pytest.mark.parametrize("parts", [1, 2, 3])
@pytest.mark.parametrize("join_type", ["inner", "full"])
def test_snapshot_restore_and_rescale(join_type, parts):
    stream = make_stream("uniform", pushes=14)
    eng = GpuEngine(join_type, *BOUNDS, max_parallelism=MAXPAR)
    ref = RefEngine(join_type, *BOUNDS)
    for sides, keys, ts, vals, wm in stream[:8]:
        for e in (eng, ref):
            e.push(sides, keys, ts, vals)
            e.watermark(wm)
    wm0 = stream[7][4]
    snaps = {kg: eng.op.snapshot(kg) for kg in range(MAXPAR)}
    for kg in range(MAXPAR):  # the handle's keyed state is the restatement's
        assert norm_state(snaps[kg]) == norm_state(ref.ref.snapshot(lambda k: kg_of(k) == kg))
    assert sum(len(s["rowtime"]) for s in snaps.values()) == eng.op.stats()["store_rows"] > 0
    with pytest.raises(N.NativeError) as e:  # restoring onto a key that has state
        kg = next(kg for kg in range(MAXPAR) if len(snaps[kg]["key"]))
        eng.op.restore(kg, snaps[kg])
    assert e.value.code == N.FW_ERR_STATE and "already has state" in str(e.value)
    eng.op.close()
    for idx in range(parts):
        r = compute_key_group_range_for_operator_index(MAXPAR, parts, idx)
        lo, hi = r.start_key_group, r.end_key_group
        sub = GpuEngine(join_type, *BOUNDS, max_parallelism=MAXPAR, key_group_range=(lo, hi), expected_keys=1, max_batch=1)
        sref = RefEngine(join_type, *BOUNDS)
        for kg in range(lo, hi + 1):
            sub.op.restore(kg, snaps[kg])
            sref.ref.restore(ref.ref.snapshot(lambda k: kg_of(k) == kg))
        # the expiration times restart at 0 and the watermark at Long.MIN_VALUE on both sides
        for e in (sub, sref):
            assert e.watermark(wm0) == ([], wm0 - 50)
        for sides, keys, ts, vals, wm in stream[8:]:
            mine = np.array([lo <= kg_of(k) <= hi for k in keys])
            a = (sides[mine], keys[mine], ts[mine], vals[mine])
            assert sorted(sub.push(*a)) == sorted(sref.push(*a))
            g, x = sub.watermark(wm), sref.watermark(wm)
            assert sorted(g[0]) == sorted(x[0]) and g[1] == x[1]
        assert sub.op.stats()["rows_in"] == int(sum(
            np.count_nonzero([lo <= kg_of(k) <= hi for k in s[1]]) for s in stream[8:])) > 0
        sub.op.close()


def test_restored_timer_with_a_remaining_row_at_time_zero_clears_without_padding():
    st = {"key": [1], "left_timer": [0], "right_timer": [3], "n_rows": [2], "side": [0, 0], "rowtime": [0, 4],
          "ordinal": [0, 1], "val": [5, 6], "emitted": [0, 0]}
    op = TimeBoundedJoin("full", -5, 9, max_parallelism=4)
    kg = assign_to_key_group(long_hash_code(1), 4)
    op.restore(kg, st)
    assert norm_state(op.snapshot(kg)) == norm_state(st) and op.stats()["store_rows"] == 2
    rows, fw = op.watermark(3)
    assert len(rows) == 0 and fw == -6
    s = op.stats()
    assert s["store_rows"] == 0 and s["active_timers"] == 0 and len(op.snapshot(kg)["key"]) == 0
    op.process([1], [1], [2], [9])  # numbered after the largest restored ordinal
    assert op.snapshot(kg)["ordinal"].tolist() == [2]
    op.close()


def test_restored_rows_without_their_timer_are_refused():
    """a cache's rows come with the timer that cleans them: without it no timer would remove them and a snapshot,
    which picks the keys with a timer set, would drop them"""
    op = TimeBoundedJoin("full", -5, 9, max_parallelism=4)
    kg = assign_to_key_group(long_hash_code(1), 4)
    base = {"key": [1], "n_rows": [1], "rowtime": [4], "ordinal": [0], "val": [5], "emitted": [0]}
    for side, timers, fragment in ((0, {"left_timer": [0], "right_timer": [0]}, "right_timer"),
                                   (0, {"left_timer": [30], "right_timer": [0]}, "right_timer"),
                                   (1, {"left_timer": [0], "right_timer": [30]}, "left_timer")):
        with pytest.raises(N.NativeError) as e:
            op.restore(kg, {**base, **timers, "side": [side]})
        assert e.value.code == N.FW_ERR_ARG and fragment in str(e.value)
        assert op.stats()["store_rows"] == 0 and op.stats()["active_timers"] == 0 and len(op.snapshot(kg)["key"]) == 0
    op.restore(kg, {**base, "left_timer": [0], "right_timer": [30], "side": [0]})
    assert op.stats()["store_rows"] == 1 and op.snapshot(kg)["right_timer"].tolist() == [30]
    op.close()


def test_rows_device_then_clear_pending_equals_drain():
    import torch
    a, b = GpuEngine("full", *BOUNDS), GpuEngine("full", *BOUNDS)
    for sides, keys, ts, vals, wm in make_stream("uniform", pushes=2):
        for e in (a, b):
            e.process(sides, keys, ts, vals)
            e.op.advance_watermark(wm)
    exp = b.op.drain()
    rows, n = a.op.rows_device()
    assert n == len(exp) > 2000 and a.op.stats()["pending_output_rows"] == n

    class _View:  # a device column as torch reads it
        def __init__(self, ptr):
            self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (ptr, False), "version": 2}

    # (the order inside a call follows the key slots, which two handles hand out in the order their claims land)
    view = {f: torch.as_tensor(_View(getattr(rows, f)), device="cuda").cpu().numpy() for f, _ in N.FwTjoinRows._fields_}
    assert sorted(zip(*(view[f].tolist() for f in view))) == sorted(rows_as_tuples(exp))
    assert set(exp["epoch"].tolist()) == {0, 1} and exp["timer_ts"].max() > 0
    a.op.clear_pending()
    assert a.op.stats()["pending_output_rows"] == 0 and len(a.op.drain()) == 0
    for e in (a, b):
        e.op.close()


def _drain_some(op, cap):
    """fw_tjoin_drain with room for `cap` rows: the rows it hands out (TJOIN_ROW_DTYPE fields as lists)"""
    import ctypes
    fields = [f for f, _ in N.FwTjoinRows._fields_]
    cols = {f: np.full(cap, -7, np.int64) for f in fields + ["epoch"]}
    dst = N.FwTjoinRows(*(cols[f].ctypes.data for f in fields))
    got = ctypes.c_int64()
    op._check(N.lib().fw_tjoin_drain(op._h, ctypes.byref(dst), cols["epoch"].ctypes.data, cap, ctypes.byref(got)))
    assert 0 <= got.value <= cap
    return {f: cols[f][:got.value].tolist() for f in cols}


def test_partial_drains_hand_out_the_rows_and_epochs_of_one_drain():
    """Three drains (less than the first call's rows, to the middle of the second call's, the rest) return what one
    drain returns, epochs included.  A full join: pushes append pairs and arrival padding, watermarks timer padding,
    four rows per watermark call.  Every push brings at most one new key, so both handles number the key slots alike
    and emit in the same order."""
    steps = [("p", [(0, 1, 100, 11)]),
             ("p", [(1, 1, 105, 12), (0, 2, 100, 21)]),
             ("p", [(1, 2, 95, 22), (1, 1, 108, 13), (0, 3, 100, 31)]),
             ("w", 121),
             ("p", [(0, 1, 200, 14), (0, 4, 200, 41), (0, 3, 201, 32)]),
             ("p", [(1, 1, 195, 15), (1, 4, 205, 42), (1, 2, 50, 23)]),
             ("w", 222),
             ("p", [(0, 2, 300, 24), (1, 3, 300, 33), (0, 4, 301, 43)]),
             ("p", [(1, 2, 305, 25), (1, 2, 295, 26)]),
             ("w", 322)]
    a, b, ref = TimeBoundedJoin("full", -10, 10), TimeBoundedJoin("full", -10, 10), RefEngine("full", -10, 10)
    exp_rows, from_timers = [], 0
    for kind, arg in steps:
        if kind == "p":
            cols = [list(c) for c in zip(*arg)]
            exp_rows += ref.push(*cols)
            for op in (a, b):
                op.process(*cols)
        else:
            rows, _ = ref.watermark(arg)
            exp_rows += rows
            from_timers += len(rows)
            for op in (a, b):
                op.advance_watermark(arg)
    one = b.drain()
    assert one["epoch"].tolist() == [0] * 4 + [1] * 4 + [2] * 4 and from_timers == 4
    assert sorted(rows_as_tuples(one)) == sorted(exp_rows)
    assert a.stats()["pending_output_rows"] == 12
    parts = []
    for cap, left in ((3, 9), (3, 6), (100, 0)):
        parts.append(_drain_some(a, cap))
        assert a.stats()["pending_output_rows"] == left
    assert [len(p["key"]) for p in parts] == [3, 3, 6]
    for f in one.dtype.names:
        assert sum((p[f] for p in parts), []) == one[f].tolist(), f
    assert _drain_some(a, 5)["key"] == [] and len(b.drain()) == 0
    a.close()
    b.close()

"""Window joins on the GPU: GpuWindowJoin (fw_list_push_batch_side, fw_list_join_pending, fw_list_drain_join,
fw_list_join_device; libflinkwin.so) against CoGroupJoinITCase's results and against the window-contents oracle over
the union stream with the split by input and the cross product formed in Python (tests/join_util.py).
Bar: per fired row n_first, the partitioned elements and the pair sequence (val1, val2, ord1, ord2) exact and in
JoinCoGroupFunction's order; rows as multisets per epoch; late counts, state entries and timers equal after every step."""
import ctypes

import numpy as np
import pytest

from flink_amd import _native as N
from tests import join_util as J
from tests.test_join_abi import KATS, kat_expected, kat_results

pytestmark = pytest.mark.gpu


def _oracle(**kw):
    from oracle import oracle as orc
    return orc.ListWindowOracle(**kw)


# ---------------------------------------------------------------- 1. CoGroupJoinITCase
@pytest.mark.parametrize("interleave", ["first", "alternate"])
@pytest.mark.parametrize("name", sorted(KATS["cases"]))
def test_gpu_join_kats(name, interleave):
    case = KATS["cases"][name]
    j = J.make_gpu(assigner="tumbling", size=KATS["window"]["size"], mode=case["mode"])
    stream = J.kat_stream(case, interleave, KATS["watermarks"]["delta"])
    J.run_both(j, _oracle(assigner="tumbling", size=KATS["window"]["size"]), stream)
    pushed = [(k, t) for st in stream if st[0] == "push" for k, t in zip(st[2], st[3])]
    got = J.gpu_firings(j)
    assert kat_results(case, got, pushed) == kat_expected(case)
    if case["mode"] == "join":  # and through pairs(): key, the two value fields, the ordinals' timestamps
        p = j.pairs()
        res = sorted(([int(x["key"]), int(x["val1"]), pushed[x["ord1"]][1]],
                      [int(x["key"]), int(x["val2"]), pushed[x["ord2"]][1]]) for x in p)
        assert res == kat_expected(case)
    else:
        assert len(j.pairs()) == 0 and j.join_pending()[2] == 0
    j.close()


def test_gpu_join_functions_are_applied_on_drain():
    case = KATS["cases"]["testJoin"]
    names = KATS["names"]
    j = J.make_gpu(assigner="tumbling", size=3, join_function=lambda a, b: names[a] + ":" + names[b],
                   cogroup_function=lambda key, w, first, second: (key, w, len(first), len(second)))
    for st in J.kat_stream(case, "alternate", -1):
        J.gpu_step(j, st)
    out = [o for _, o in j.outputs()]
    assert sorted(o for o in out if isinstance(o, str)) == sorted(names[a[1]] + ":" + names[b[1]]
                                                                 for a, b in case["expected"])
    assert sorted(o for o in out if not isinstance(o, str)) == [(1, (0, 3), 3, 2), (1, (6, 9), 3, 2), (2, (3, 6), 2, 2)]
    assert [(len(a), len(b)) for _, a, b in j.cogroups()] == [(int(n), int(r["count"] - n))
                                                              for r, n in zip(j.rows(), j.n_first())]
    j.close()


# ---------------------------------------------------------------- 2. seeded parity
@pytest.mark.parametrize("name,cfg,skw", J.SEEDED, ids=[s[0] for s in J.SEEDED])
def test_gpu_join_vs_oracle(name, cfg, skw):
    j = J.make_gpu(**cfg)
    exp = J.run_both(j, J.make_ref(**cfg), J.seeded_stream(**skw), device=cfg.get("device_columns", False))
    assert len(j.pairs()) == J.count_pairs(exp) > 400
    j.close()


def test_gpu_cogroup_mode_vs_oracle():
    cfg = dict(assigner="tumbling", size=100, lateness=40)
    j = J.make_gpu(mode="cogroup", **cfg)
    exp = J.run_both(j, J.make_ref(**cfg), J.seeded_stream(n=1500))
    assert len(exp) == len(j.cogroups()) > 100 and len(j.pairs()) == 0
    j.close()


# ---------------------------------------------------------------- 3. one hot row among small ones
def test_gpu_join_hot_row():
    j = J.make_gpu(assigner="tumbling", size=1000)
    exp = J.run_both(j, _oracle(assigner="tumbling", size=1000), J.hot_stream())
    assert max(len(a) * len(b) for _, a, b in exp) == 1500 * 1100 > 1 << 16
    assert len(j.pairs()) == J.count_pairs(exp)
    j.close()


# ---------------------------------------------------------------- 4. count without materialising
def test_gpu_join_counts_what_it_cannot_materialise():
    j = J.make_gpu(assigner="tumbling", size=1000)
    stream = J.count_stream()
    for _, side, k, t, v in stream[:2]:
        j.op.process_batch(k, t, v, side=side)
    j.op.advance_watermark(stream[2][2])
    assert j.join_pending() == (1, 140000, 4900000000)
    before = j.op.pending()
    with pytest.raises(N.NativeError) as e:
        j.drain_join()
    assert e.value.code == N.FW_ERR_CAPACITY and "pairs == NULL" in str(e.value) and "max_join_pairs" in str(e.value)
    assert j.op.pending() == before == (1, 140000, 0) and j.join_pending() == (1, 140000, 4900000000)
    rows, nf, el, pairs = j.drain_join(pairs=False)
    assert pairs is None and nf.tolist() == [70000] and rows["count"].tolist() == [140000]
    assert rows["first"].tolist() == [0] and rows["elem_off"].tolist() == [0]
    assert np.array_equal(el["val"], np.concatenate([stream[0][4], stream[1][4]]))
    assert np.array_equal(el["ordinal"], np.concatenate([np.arange(70000), np.arange(70000, 140000) | J.SIDE]))
    assert np.array_equal(el["ts"], np.concatenate([stream[0][3], stream[1][3]]))
    assert j.op.pending() == (0, 0, 0) and j.join_pending() == (0, 0, 0)
    j.close()


def test_gpu_join_max_join_pairs_is_a_setting():
    j = J.make_gpu(assigner="tumbling", size=100, max_join_pairs=5)
    j.op.process_batch([1, 1, 1], [1, 2, 3], [10, 11, 12], side=0)
    j.op.process_batch([1, 1], [4, 5], [20, 21], side=1)
    j.op.advance_watermark(99)
    assert j.join_pending() == (1, 5, 6)
    with pytest.raises(N.NativeError) as e:
        j.join_device()
    assert e.value.code == N.FW_ERR_CAPACITY
    j.op.process_batch([2, 2], [101, 102], [1, 2], side=1)  # a refusal left the handle as it was
    rows, nf, el, pairs = j.drain_join(pairs=False)
    assert nf.tolist() == [3] and el["val"].tolist() == [10, 11, 12, 20, 21]
    j.close()


# ---------------------------------------------------------------- 5. the capacity convention
def test_gpu_join_capacity_convention():
    cfg = dict(assigner="tumbling", size=100)
    j, rj = J.make_gpu(**cfg), J.RefJoin(_oracle(**cfg))
    stream = [s for s in J.seeded_stream(n=600, span=300) if s[0] == "push"]  # (dense: rows of both inputs)
    for st in stream:
        j.op.process_batch(*st[2:], side=st[1])
        rj.step(st)
    j.op.advance_watermark(J.LMAX)
    rj.step(("wm", None, J.LMAX))
    exp = rj.firings()
    nr, ne, npairs = j.join_pending()
    assert (nr, npairs) == (len(exp), J.count_pairs(exp)) and npairs > 100
    with pytest.raises(N.NativeError) as e:
        j.drain_join(cap_pairs=npairs - 1)
    assert e.value.code == N.FW_ERR_CAPACITY
    assert j.join_pending() == (nr, ne, npairs) and j.op.pending() == (nr, ne, 0)
    j.op.epoch = 1
    j._collect(0)
    got = J.gpu_firings(j)
    J.same_firings(got, exp)
    assert J.check_pairs(j, got) == npairs
    j.close()


# ---------------------------------------------------------------- 6. incremental, and the device view
def test_gpu_join_incremental_and_device_view():
    cfg = dict(assigner="tumbling", size=100, lateness=1000)
    j, rj = J.make_gpu(**cfg), J.RefJoin(_oracle(**cfg))
    stream = [s for s in J.seeded_stream(n=900, seed=3, span=500) if s[0] == "push"]
    half = len(stream) // 2
    for st in stream[:half]:
        j.op.process_batch(*st[2:], side=st[1])
        rj.step(st)
    wm = int(max(st[3].max() for st in stream[:half]))
    j.op.advance_watermark(wm)
    rj.step(("wm", None, wm))
    first = j.join_pending()
    assert first[0] == len(rj.firings()) > 0 and first[2] == J.count_pairs(rj.firings())
    for st in stream[half:]:  # late elements within the lateness fire their windows at once: more rows, more pairs
        j.op.process_batch(*st[2:], side=st[1])
        rj.step(st)
    exp = rj.firings()
    second = j.join_pending()
    assert second[0] == len(exp) > first[0] and second[2] == J.count_pairs(exp) > first[2]
    drows, dnf, del_, dpairs = j.join_device()
    dev = ({f: c.cpu().numpy() for f, c in drows.items()}, dnf.cpu().numpy(), {f: c.cpu().numpy() for f, c in del_.items()},
           {f: c.cpu().numpy() for f, c in dpairs.items()})
    assert j.join_pending() == second  # a view clears nothing
    rows, nf, el, pairs = j.drain_join(epoch=1)
    assert all(np.array_equal(dev[0][f], rows[f]) for f in dev[0]) and np.array_equal(dev[1], nf)
    assert all(np.array_equal(dev[2][f], el[f]) for f in dev[2])
    assert all(np.array_equal(dev[3][f], pairs[f]) for f in dev[3]) and len(pairs["row"]) == second[2]
    # rows keep row order: the pairs' row column is non-decreasing, old rows before the new ones
    assert (np.diff(pairs["row"]) >= 0).all() and pairs["row"][0] < first[0] <= pairs["row"][-1]
    rows["epoch"][:first[0]] = 0
    j._rows, j._nfirst, j._elems = [rows], [nf], [el]
    got = J.gpu_firings(j)
    J.same_firings(got, exp)
    for r, (_, a, b) in enumerate(got):
        v1, v2, o1, o2 = J.expected_pairs(a, b)
        m = pairs["row"] == r
        assert np.array_equal(pairs["val1"][m], v1) and np.array_equal(pairs["val2"][m], v2)
        assert np.array_equal(el["ordinal"][pairs["idx1"][m]] & ~J.SIDE, o1)
        assert np.array_equal(el["ordinal"][pairs["idx2"][m]] & ~J.SIDE, o2)
    j.close()


# ---------------------------------------------------------------- 7. state
def test_gpu_join_snapshot_restore_rescale():
    from flink_amd import KeyGroupRange
    from oracle import oracle as orc
    cfg = dict(assigner="tumbling", size=100, lateness=40)
    stream = J.seeded_stream()
    cut = len(stream) // 2
    while stream[cut - 1][0] != "wm":
        cut += 1
    j, rj = J.make_gpu(**cfg), J.RefJoin(J.make_ref(**cfg))
    for st in stream[:cut]:
        J.gpu_step(j, st)
        rj.step(st)
    snap = j.snapshot_state()
    ords = np.concatenate([s[1]["ordinal"] for s in snap.values()])
    sides = np.asarray(rj.sides)
    assert len(ords) > 50 and ((ords & J.SIDE != 0) == (sides[ords & ~J.SIDE] == 1)).all()
    assert 0 < int((ords & J.SIDE != 0).sum()) < len(ords)
    got = J.gpu_firings(j, ordinals=False)
    npairs = len(j.pairs())
    parts = []
    for r in (KeyGroupRange(0, 63), KeyGroupRange(64, 127)):
        p = J.make_gpu(key_group_range=r, **cfg)
        p.initialize_state(snap)
        p.op.epoch = j.epoch - 1
        p.watermark(rj.out_wm)  # the watermark is not part of the state
        assert len(p.rows()) == 0
        for st in stream[cut:]:
            if st[0] == "push":
                kg = orc.key_groups_long(st[2], 128)
                mine = (kg >= r.start_key_group) & (kg <= r.end_key_group)
                st = st[:2] + tuple(c[mine] for c in st[2:])
            J.gpu_step(p, st)
        # ordinals number each handle's own records from the largest restored one on: plain, and beyond it
        assert (p.rows()["first"] >= 0).all() and (p.rows()["first"] < J.SIDE).all()
        assert (p.elems()["ordinal"] & ~J.SIDE).max() > (ords & ~J.SIDE).max()
        f = J.gpu_firings(p, ordinals=False)
        got += f
        npairs += len(p.pairs())
        parts.append(p)
    for st in stream[cut:]:
        rj.step(st)
    exp = rj.firings(ordinals=False)
    J.same_firings(got, exp)
    assert npairs == J.count_pairs(exp)
    for p in parts:
        # a restored handle's pairs are its rows' cross products too (values; its ordinals are its own)
        q = 0
        pr = p.pairs()
        for _, a, b in J.gpu_firings(p, ordinals=False):
            n = len(a) * len(b)
            if n:
                assert np.array_equal(pr["val1"][q:q + n], np.repeat([x[1] for x in a], len(b)))
                assert np.array_equal(pr["val2"][q:q + n], np.tile([x[1] for x in b], len(a)))
            q += n
        assert q == len(pr)
        p.close()
    j.close()


# ---------------------------------------------------------------- 8. the plain drain is unchanged
def test_gpu_join_plain_drain_is_list_order_with_tagged_ordinals():
    j, ref = J.make_gpu(assigner="tumbling", size=100), _oracle(assigner="tumbling", size=100)
    rj = J.RefJoin(ref)
    for st in [s for s in J.seeded_stream(n=500) if s[0] == "push"]:
        j.op.process_batch(*st[2:], side=st[1])
        rj.step(st)
    j.op.process_batch([5], [7], [1])  # the plain push on a join handle is input 1
    rj.step(("push", 0, [5], [7], [1]))
    j.op.advance_watermark(J.LMAX)
    ref.watermark(J.LMAX)
    j.join_pending()  # (the split lives beside the pending elements)
    rows, el = j.op.drain()
    sides = np.asarray(rj.sides)
    exp = {(int(r["key"]), int(r["start"])): (int(r["first"]), e) for r, e in ref.contents()}
    assert len(rows) == len(exp) > 20
    mixed = 0
    for r in rows:
        first, e = exp[(int(r["key"]), int(r["start"]))]
        g = el[r["elem_off"]:r["elem_off"] + r["count"]]
        assert int(r["first"]) == first  # the plain ordinal
        assert np.array_equal(g["ordinal"], e["ord"] | (sides[e["ord"]] * J.SIDE))  # list order, tagged
        assert np.array_equal(g["ts"], e["ts"]) and np.array_equal(g["val"], e["val"])
        s = sides[e["ord"]]
        mixed += bool((np.diff(s) < 0).any())  # an element of input 2 before one of input 1: not partitioned
    assert mixed > 5
    j.close()


# ---------------------------------------------------------------- 9. handles without a join
def test_gpu_joinless_handle_refuses():
    from flink_amd import TumblingEventTimeWindows
    from flink_amd.listwindow import GpuListWindowOperator
    op = GpuListWindowOperator(TumblingEventTimeWindows.of(100))
    L = N.lib()
    n = ctypes.c_int64()
    k = np.zeros(1, dtype=np.int64)
    assert L.fw_list_join_pending(op._h, ctypes.byref(n), None, None) == N.FW_ERR_ARG
    assert L.fw_list_drain_join(op._h, None, None, 0, None, 0, None, 0, None, None, None) == N.FW_ERR_ARG
    assert L.fw_list_join_device(op._h, None, None, None, None, None, None, None) == N.FW_ERR_ARG
    for side in (0, 1):
        assert L.fw_list_push_batch_side(op._h, side, k.ctypes.data, k.ctypes.data, k.ctypes.data, None, 1) == N.FW_ERR_ARG
        assert L.fw_list_push_batch_side_device(op._h, side, None, None, None, None, 0) == N.FW_ERR_ARG
    assert "without a join" in L.fw_list_last_error(op._h).decode() or "join" in L.fw_list_last_error(op._h).decode()
    op.process([1], [5], [3])
    op.watermark(J.LMAX)
    assert op.rows()["first"].tolist() == [0] and op.stats()["records_in"] == 1
    op.close()
    j = J.make_gpu(assigner="tumbling", size=100)
    for side in (-1, 2):
        assert L.fw_list_push_batch_side(j.op._h, side, k.ctypes.data, k.ctypes.data, k.ctypes.data, None, 1) == N.FW_ERR_ARG
    assert j.op.stats()["records_in"] == 0
    j.close()

"""Count windows (countWindow(size, slide).sum(pos), FW_COUNT): keyed-state snapshot, restore and rescaling on the GPU
(fw_count_snapshot_key_group / fw_count_restore_key_group), in the list operator's logical form.

The judge is oracle.CountWindowOracle run over the whole stream without interruption: whatever is snapshotted at a
cut, restored (into count handles of any parallelism, or into the equivalent GpuListWindowOperator) and continued
must fire exactly the oracle's rows after the cut.  Rows are compared exactly (f64 sums are list-order sums on both
sides, so bit-exact).  `max` is the arrival ordinal of a row's first element: a restored handle numbers its pushes
after the largest restored ordinal, so its ordinals are translated back to the stream's before they are compared."""
import ctypes

import numpy as np
import pytest

from flink_amd import CountEvictor, CountTrigger, CountWindows, GlobalWindows, KeyGroupRange, TumblingEventTimeWindows
from flink_amd import _native as N
from flink_amd.datagen import generate_host
from flink_amd.keygroups import (assign_to_key_group, compute_key_group_range_for_operator_index, long_hash_code)
from flink_amd.windowing import FirstElementReduce
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

LMIN, LMAX = -(1 << 63), (1 << 63) - 1
_VT = {"i64": "long", "f64": "double"}
FIELDS = ("key", "start", "end", "count", "sum", "min", "max")
MAXPAR = 16


def _count_op(size, slide, after=False, value_type="i64", **kw):
    from flink_amd.operator import GpuWindowOperator
    kw.setdefault("max_parallelism", MAXPAR)
    return GpuWindowOperator(CountWindows.of(size, slide, after), FirstElementReduce(_VT[value_type], "sum"), **kw)


def _list_op(size, slide, after, **kw):
    from flink_amd.listwindow import GpuListWindowOperator
    kw.setdefault("max_parallelism", MAXPAR)
    return GpuListWindowOperator(GlobalWindows.create(), CountTrigger.of(slide), CountEvictor.of(size, after),
                                 emit_contents=False, **kw)


def _kg_of_long(key, max_par=MAXPAR):
    return assign_to_key_group(long_hash_code(int(key)), max_par)


def _bits(vals):
    return vals.view(np.int64) if vals.dtype == np.float64 else vals


def _rowset(rows, first="max"):
    return sorted(tuple(int(r[f]) for f in FIELDS[:6]) + (int(r[first]),) for r in rows)


def _oracle_after_cut(size, slide, after, vt, keys, vals, cut):
    """rows the uninterrupted oracle fires for records [cut, n) of the stream (ordinals = stream indices)"""
    ref = orc.CountWindowOracle(size, slide, after, value_type=vt)
    ref.process(keys[:cut], _bits(vals[:cut]))
    n0 = len(ref.rows())
    ref.process(keys[cut:], _bits(vals[cut:]))
    rows = ref.rows()[n0:].copy()
    ref.close()
    return rows


def _largest_ordinal(snap):
    return max([int(e["ordinal"].max()) for _, e in snap.values() if len(e)], default=-1)


def _translate(rows, base, index, field="max"):
    """ordinals of a restored handle back to the stream's: an ordinal below `base` (= the largest restored ordinal
    + 1) is a restored element's and is the stream's already; base + i is the i-th record the handle was pushed,
    stream record index[i]"""
    rows = rows.copy()
    o = rows[field]
    new = o >= base
    rows[field][new] = np.asarray(index, dtype=np.int64)[o[new] - base]
    return rows


def _expected_list(size, slide, after, k):
    """(n_elems, trigger_count) of a key's snapshot row after its k elements; None = the key is omitted"""
    wl = size + slide if after else size
    f = k - k % slide
    l_ref = k if f == 0 else min(size, f) + (k - f)
    m = min(l_ref, wl - 1)
    t = k % slide
    return None if m == 0 and t == 0 else (m, t)


def _cut_stream(size, slide, vt, seed=7):
    """key j = 0 .. 3 (size + slide) + 1 gets j elements, shuffled; then 2 (size + slide) more for every key"""
    nk = 3 * (size + slide) + 2
    rng = np.random.default_rng(seed)
    k1 = rng.permutation(np.repeat(np.arange(nk, dtype=np.int64), np.arange(nk)))
    k2 = rng.permutation(np.repeat(np.arange(nk, dtype=np.int64), 2 * (size + slide)))
    keys = np.concatenate([k1, k2])
    if vt == "f64":  # sums whose order matters: magnitudes spread over many binades, both signs
        vals = rng.standard_normal(len(keys)) * np.exp2(rng.integers(-30, 30, len(keys)).astype(np.float64))
    else:
        vals = rng.integers(-(1 << 40), 1 << 40, len(keys), dtype=np.int64)
    return nk, keys, vals, len(k1)


CONFIGS = [(10, 5, False), (10, 10, False), (7, 3, False), (4, 6, False), (1, 1, False), (1, 3, False), (4, 2, True),
           (5, 3, True)]


@pytest.mark.parametrize("vt", ["i64", "f64"])
@pytest.mark.parametrize("size,slide,after", CONFIGS, ids=[f"{a}_{b}_{c}" for a, b, c in CONFIGS])
def test_every_cut_point_in_one_snapshot(size, slide, after, vt):
    nk, keys, vals, cut = _cut_stream(size, slide, vt)
    zeros = np.zeros(len(keys), dtype=np.int64)
    a = _count_op(size, slide, after, vt, expected_entries=2 * nk)
    ragged = cut * 2 // 5 + 1  # a key's elements straddle the two pushes: its ring is read across them
    a.process(keys[:ragged], zeros[:ragged], vals[:ragged])
    a.process(keys[ragged:cut], zeros[ragged:cut], vals[ragged:cut])
    snap = a.snapshot_state()
    a.close()
    assert sorted(snap) == list(range(MAXPAR))
    # every key's list against the closed form
    seen = {}
    for kg, (lists, elems) in snap.items():
        assert int(lists["n_elems"].sum()) == len(elems)
        off = 0
        for r in lists:
            assert _kg_of_long(r["key"]) == kg
            assert int(r["key"]) not in seen
            seen[int(r["key"])] = (r, elems[off:off + int(r["n_elems"])])
            off += int(r["n_elems"])
    bits = _bits(vals)
    for j in range(nk):
        exp = _expected_list(size, slide, after, j)
        if exp is None:
            assert j not in seen, j
            continue
        m, t = exp
        r, el = seen.pop(j)
        assert (int(r["n_elems"]), int(r["trigger_count"])) == (m, t), j
        assert (int(r["start"]), int(r["end"]), int(r["timer"])) == (LMIN, LMAX, 0), j
        mine = np.flatnonzero(keys[:cut] == j)[j - m:]  # its last m elements, oldest first
        assert np.array_equal(el["ordinal"], mine), j
        assert np.array_equal(el["val"], bits[mine]), j
        assert np.all(el["ts"] == LMIN), j
    assert not seen
    # restored into a fresh handle, the stream goes on exactly as if it had never been cut
    b = _count_op(size, slide, after, vt, expected_entries=2 * nk)
    b.initialize_state(snap)
    base = _largest_ordinal(snap) + 1
    mid = cut + (len(keys) - cut) // 3
    b.process(keys[cut:mid], zeros[cut:mid], vals[cut:mid])
    b.process(keys[mid:], zeros[mid:], vals[mid:])
    got = _translate(b.rows(), base, np.arange(cut, len(keys)))
    b.close()
    exp = _oracle_after_cut(size, slide, after, vt, keys, vals, cut)
    assert len(exp) > 0
    assert _rowset(got) == _rowset(exp)


@pytest.mark.parametrize("hashed", [False, True], ids=["long_keys", "hashed_keys"])
def test_rescaling_one_handle_to_three(hashed):
    n, cut = 20_000, 9_001
    keys, _, vals = generate_host(0xC0FFEE, 0, n, 300, ts_base=0, rate=1_000_000, jitter=0, zipf_s=1.05)
    zeros = np.zeros(n, dtype=np.int64)
    if hashed:  # the caller's hashes disagree with the keys' own: the stored key group must follow the hash
        kh = ((keys * 2654435761 + 12345) & 0x7FFFFFFF).astype(np.int32)
        kg = np.array([assign_to_key_group(int(h), MAXPAR) for h in kh])
        assert np.any(kg != np.array([_kg_of_long(k) for k in keys]))
    else:
        kh = None
        kg = np.array([_kg_of_long(k) for k in keys])
    kw = dict(key_type="hashed") if hashed else {}
    one = _count_op(10, 5, expected_entries=512, **kw)
    for a, b in ((0, 4_097), (4_097, cut)):
        one.process(keys[a:b], zeros[a:b], vals[a:b], None if kh is None else kh[a:b])
    snap = one.snapshot_state()
    one.close()
    kg_of_key = dict(zip(keys.tolist(), kg.tolist()))
    for g, (lists, elems) in snap.items():
        assert all(kg_of_key[int(k)] == g for k in lists["key"]), g
    assert sum(len(l) for l, _ in snap.values()) == len(set(keys[:cut].tolist()))  # (every key has elements: size > 1)
    got = []
    for i in range(3):
        r = compute_key_group_range_for_operator_index(MAXPAR, 3, i)
        mine = {g: s for g, s in snap.items() if g in r}
        op = _count_op(10, 5, expected_entries=512, key_group_range=r, **kw)
        op.initialize_state(snap)  # (takes the key groups of its own range)
        base = _largest_ordinal(mine) + 1
        idx = cut + np.flatnonzero((kg[cut:] >= r.start_key_group) & (kg[cut:] <= r.end_key_group))
        assert len(idx) > 0
        h = len(idx) // 2 + 1
        for part in (idx[:h], idx[h:]):
            op.process(keys[part], zeros[part], vals[part], None if kh is None else kh[part])
        got.append(_translate(op.rows(), base, idx))
        # what this handle holds now is again state of its own key groups only
        again = op.snapshot_state()
        assert sorted(again) == list(r)
        for g, (lists, _) in again.items():
            assert all(kg_of_key[int(k)] == g for k in lists["key"]), g
        op.close()
    exp = _oracle_after_cut(10, 5, False, "i64", keys, vals, cut)
    assert len(exp) > 1000
    assert _rowset(np.concatenate(got)) == _rowset(exp)


@pytest.mark.parametrize("size,slide,after", [(10, 5, False), (5, 3, True)], ids=["10_5_before", "5_3_after"])
def test_count_handle_to_list_operator_and_back(size, slide, after):
    nk, keys, vals, cut = _cut_stream(size, slide, "i64", seed=11)
    zeros = np.zeros(len(keys), dtype=np.int64)
    exp = _oracle_after_cut(size, slide, after, "i64", keys, vals, cut)
    mid = cut + (len(keys) - cut) // 3
    index = np.arange(cut, len(keys))
    # count handle -> list operator
    a = _count_op(size, slide, after, expected_entries=2 * nk)
    a.process(keys[:cut], zeros[:cut], vals[:cut])
    snap = a.snapshot_state()
    a.close()
    lo = _list_op(size, slide, after)
    lo.initialize_state(snap)
    lo.process(keys[cut:mid], zeros[cut:mid], vals[cut:mid])
    lo.process(keys[mid:], zeros[mid:], vals[mid:])
    got = _translate(lo.rows(), _largest_ordinal(snap) + 1, index, field="first")
    lo.close()
    assert _rowset(got, first="first") == _rowset(exp)
    # list operator -> count handle: the full lists of the reference's state
    lo = _list_op(size, slide, after)
    lo.process(keys[:cut], zeros[:cut], vals[:cut])
    snap = lo.snapshot_state()
    lo.close()
    if not after:  # (evicting before: the reference's lists are longer than the ring, the count handle takes their tails)
        assert any(int(l["n_elems"].max(initial=0)) > size - 1 for l, _ in snap.values())
    b = _count_op(size, slide, after, expected_entries=2 * nk)
    b.initialize_state(snap)
    b.process(keys[cut:mid], zeros[cut:mid], vals[cut:mid])
    b.process(keys[mid:], zeros[mid:], vals[mid:])
    got = _translate(b.rows(), _largest_ordinal(snap) + 1, index)
    b.close()
    assert _rowset(got) == _rowset(exp)


def _lists(rows):
    out = np.zeros(len(rows), dtype=[(f, "<i8") for f in ("key", "start", "end", "trigger_count", "timer", "n_elems")])
    for i, (key, t, n) in enumerate(rows):
        out[i] = (key, LMIN, LMAX, t, 0, n)
    return out


def _elems(vals, first_ordinal=0):
    out = np.zeros(len(vals), dtype=[("ts", "<i8"), ("val", "<i8"), ("ordinal", "<i8")])
    out["ts"], out["val"], out["ordinal"] = LMIN, vals, np.arange(first_ordinal, first_ordinal + len(vals))
    return out


def _keys_of_group(g, n, start=1000):
    out, k = [], start
    while len(out) < n:
        if _kg_of_long(k) == g:
            out.append(k)
        k += 1
    return out


def _snap_set(op):
    return sorted((kg, l.tobytes(), e.tobytes()) for kg, (l, e) in op.snapshot_state().items())


def test_refusals_leave_the_handle_unchanged_and_usable():
    k3 = _keys_of_group(3, 4)
    op = _count_op(10, 5, expected_entries=64)
    pushed = np.array([k3[0]] * 3, dtype=np.int64)
    op.process(pushed, np.zeros(3, dtype=np.int64), np.array([5, 6, 7], dtype=np.int64))
    before = _snap_set(op)

    def refused(code, kg, lists, elems):
        with pytest.raises(N.NativeError) as ei:
            op.restore_key_group(kg, lists, elems)
        assert ei.value.code == code, ei.value
        assert _snap_set(op) == before

    # CountTrigger.of(5) never holds a count of 5: it clears it when it fires
    refused(N.FW_ERR_ARG, 3, _lists([(k3[1], 5, 1)]), _elems([1]))
    refused(N.FW_ERR_ARG, 3, _lists([(k3[1], -1, 1)]), _elems([1]))
    refused(N.FW_ERR_ARG, 3, _lists([(k3[1], 0, -1)]), _elems([]))
    refused(N.FW_ERR_ARG, 3, _lists([(k3[1], 0, 2)]), _elems([1]))  # lengths do not add up
    # a valid list first, so a refusal after a partial restore would show
    refused(N.FW_ERR_STATE, 3, _lists([(k3[1], 1, 1), (k3[2], 2, 1), (k3[2], 2, 1)]), _elems([1, 2, 3]))
    refused(N.FW_ERR_STATE, 3, _lists([(k3[1], 1, 1), (k3[0], 2, 1)]), _elems([1, 2]))  # k3[0] was pushed
    # the handle still works: a valid restore, then both keys go on
    op.restore_key_group(3, _lists([(k3[1], 4, 4)]), _elems([100, 200, 300, 400], first_ordinal=50))
    more = np.array([k3[0], k3[0], k3[1]], dtype=np.int64)
    op.process(more, np.zeros(3, dtype=np.int64), np.array([8, 9, 500], dtype=np.int64))
    # the 5th element of each key fires: k3[0] from its own first element, k3[1] from its first restored one
    rows = {int(r["key"]): tuple(int(r[f]) for f in ("count", "sum", "min", "max")) for r in op.rows()}
    assert rows == {k3[0]: (5, 35, 5, 0), k3[1]: (5, 1500, 100, 50)}
    op.close()


def test_restore_capacity_refused_before_anything_changes():
    op = _count_op(10, 5, expected_entries=8)
    ks = _keys_of_group(5, 9)
    lists = _lists([(k, 1, 1) for k in ks])
    with pytest.raises(N.NativeError) as ei:
        op.restore_key_group(5, lists, _elems(list(range(9))))
    assert ei.value.code == N.FW_ERR_CAPACITY
    assert all(len(l) == 0 and len(e) == 0 for l, e in op.snapshot_state().values())
    op.restore_key_group(5, lists[:8], _elems(list(range(8))))  # eight fit
    assert len(op.snapshot_key_group(5)[0]) == 8
    with pytest.raises(N.NativeError) as ei:
        op.restore_key_group(5, lists[8:], _elems([8]))
    assert ei.value.code == N.FW_ERR_CAPACITY
    assert len(op.snapshot_key_group(5)[0]) == 8
    op.close()


def test_other_handles_and_key_groups_refused():
    from flink_amd.operator import GpuWindowOperator
    L = N.lib()
    nl, ne = ctypes.c_int64(), ctypes.c_int64()
    tw = GpuWindowOperator(TumblingEventTimeWindows.of(100), max_parallelism=MAXPAR)
    assert L.fw_count_snapshot_key_group(tw._h, 0, None, 0, 0, ctypes.byref(nl), ctypes.byref(ne)) == N.FW_ERR_UNSUPPORTED
    assert L.fw_count_restore_key_group(tw._h, 0, None, 0, 0) == N.FW_ERR_UNSUPPORTED
    tw.close()
    op = _count_op(10, 5, expected_entries=64, key_group_range=KeyGroupRange(0, 7))
    with pytest.raises(N.NativeError) as ei:
        op.snapshot_key_group(12)
    assert ei.value.code == N.FW_ERR_KEY_GROUP
    with pytest.raises(N.NativeError) as ei:
        op.restore_key_group(12, _lists([(_keys_of_group(12, 1)[0], 1, 1)]), _elems([1]))
    assert ei.value.code == N.FW_ERR_KEY_GROUP
    with pytest.raises(N.NativeError) as ei:  # a long key that is not of the key group it is restored under
        op.restore_key_group(3, _lists([(_keys_of_group(4, 1)[0], 1, 1)]), _elems([1]))
    assert ei.value.code == N.FW_ERR_KEY_GROUP
    # the row-state calls keep refusing count handles
    n = ctypes.c_int64()
    assert L.fw_snapshot_key_group_blocks(op._h, 0, None, None, 0, ctypes.byref(n)) == N.FW_ERR_UNSUPPORTED
    assert L.fw_snapshot_key_group(op._h, 0, None, 0, ctypes.byref(n)) == N.FW_ERR_UNSUPPORTED
    assert L.fw_restore_key_group(op._h, 0, None, 0) == N.FW_ERR_UNSUPPORTED
    # a key pushed outside the handle's KeyGroupRange appears in no snapshot of an owned key group
    k = np.array(_keys_of_group(12, 1) * 3, dtype=np.int64)
    op.process(k, np.zeros(3, dtype=np.int64), k)
    assert all(len(l) == 0 for l, _ in op.snapshot_state().values())
    op.close()

"""The premises of the streams that tests/test_gpu_dn_edges.py runs against k_dn_aggregate (tests/dn_util.py), checked
on the CPU: what each push puts into each region is what its GPU test means to put there, the records meant to be
narrow are, the ids meant to occur do, and the oracle's rows are the exact Python-int aggregates.  If one of these
failed, the GPU test of that stream would be testing nothing."""
import numpy as np
import pytest

from tests import dn_util as D
from tests.parity_util import assert_rows_equal


def _restored(s):
    return D.restored_rows(s, D.pre_state(s)) if s.pre else None


def test_kernel_shape_and_limits():
    # the figures the issue's thresholds are written in; a retune moves the streams with them
    assert D.RS == D.NT * D.RPT and D.ND >= 1 and D.LIMIT == D.NS * 15 // 16
    # live > LIMIT cannot be the first refusal: the entries' registers run out before the table's fill limit
    assert D.ENTRY_MAX < D.LIMIT
    # P16: a narrow run holds 2 rcap = 4 max_batch / P records, so a run of RUN_MAX + 1 reaches the kernel
    assert 2 * ((2 * D.MAX_BATCH // 16) & ~7) > D.RUN_MAX + 1
    ls = D.round_lengths()
    assert ls == sorted(ls) and len(set(ls)) == len(ls) and 200_000 < sum(ls) < 300_000
    assert {1, 2, 3, D.RS, D.ND * D.RS, D.ND * D.RS + 1, D.RUN_MAX, D.RUN_MAX + 1} <= set(ls)
    assert sum(n % 2 for n in ls) >= 5  # odd lengths: the last pair of a run is clamped


def test_region_mirror_restates_partition_of():
    # fmix64 is murmur3's finaliser: known values, and a bijection's spread over the 16 regions
    assert int(D.fmix64([0])[0]) == 0 and int(D.fmix64([1])[0]) == 0xB456BCFC34C2CB2C
    reg = D.region_of(np.arange(-50_000, 50_000))
    assert reg.min() == 0 and reg.max() == 15 and np.bincount(reg).min() > 5000
    assert np.array_equal(D.region_of(np.arange(1000), 5) >> 1, D.region_of(np.arange(1000), 4))
    for r in (0, 7, 15):
        assert (D.region_of(D.keys_in(r, 100)) == r).all() and (D.region_of(D.keys_in(r, 100, inside=False)) != r).all()


@pytest.mark.parametrize("name", sorted(D.STREAMS))
def test_stream_premises(name):
    s = D.stream(name)
    steps, M = s.steps, D.mirror(s, _restored(s))
    assert len(s.deltas) == len(steps)
    # a lone watermark first, so that the first batch is already narrow; the last step fires everything
    assert steps[0][0] is None and steps[0][3] >= D.WM0 and steps[-1][0] is None and steps[-1][3] == D.MAX_WM
    ids = set()
    for e, ((k, t, v, wm), m) in enumerate(zip(steps, M)):
        if k is None:
            assert s.deltas[e] == 0
            continue
        # every record meant to be narrow is: key, window delta and value (narrow_encode's three conditions)
        assert int((~m["narrow"]).sum()) == s.wide.get(e, 0), (e, np.nonzero(~m["narrow"])[0][:5])
        ids |= set(m["ids"].tolist())
        p = s.premises.get(e)
        if p:
            r = p.get("region", s.r)
            for f in ("run", "new", "live"):
                if p.get(f) is not None:
                    assert int(m[f][r]) == p[f], (e, f, int(m[f][r]), p[f])
    assert set(s.ids) <= ids, [hex(i) for i in set(s.ids) - ids]
    # no three refusing pushes in a row by accident (the sticky stream means them)
    if name != "sticky":
        d = s.deltas
        assert not any(d[i] and d[i + 1] and d[i + 2] for i in range(len(d) - 2))


def test_rounds_premises():
    s, ls = D.stream("rounds"), D.round_lengths()
    M = D.mirror(s)
    assert [int(m["run"][s.r]) for m in M[1:-1]] == ls
    # every second push leaves the other 15 regions empty (the kernel's begin == end path), the others fill them
    for i, m in enumerate(M[1:-1]):
        others = np.delete(m["run"], s.r)
        assert (others.sum() == 300 and (others > 0).sum() >= 12) if i % 2 else others.sum() == 0
    assert int(M[-2]["live"][s.r]) == 64 and s.deltas[1:-1] == [0] * (len(ls) - 1) + [1]
    # values are distinguishable: a round read twice or skipped changes the sums
    for k, t, v, wm in s.steps[4:-1]:
        assert len(np.unique(v)) > len(v) * 0.99


def test_claims_premises():
    s = D.stream("claims")
    k, t, v, _ = s.steps[1]
    ids = D.narrow_id(k, t // D.SIZE - D.WM0 // D.SIZE)
    assert (D.region_of(k) == s.r).all() and len(np.unique(ids)) == 3000 < D.LIMIT
    # each id three times, in adjacent records
    assert (ids[0::3] == ids[1::3]).all() and (ids[0::3] == ids[2::3]).all() and len(np.unique(ids[0::3])) == 3000


def test_limit_premises():
    e, at, over = D.stream("entries"), D.stream("fill_at"), D.stream("fill_over")
    assert [e.premises[i]["live"] for i in (1, 2, 3, 4)] == [D.ENTRY_MAX, D.ENTRY_MAX, D.ENTRY_MAX + 1, D.ENTRY_MAX + 1]
    assert at.premises[1]["new"] == D.LIMIT and at.deltas[1] == 0
    assert over.premises[1]["new"] == D.LIMIT + 1 and over.deltas[1] == 1
    for s in (at, over):  # unique ids, so no two tickets are ever held for one id
        k, t, _, _ = s.steps[1]
        assert len(np.unique(D.narrow_id(k, t // D.SIZE - D.WM0 // D.SIZE))) == len(k)
    p = D.stream("passes")
    M = D.mirror(p)
    # refused for its groups alone (not for run length or entries), then live is below every entry limit
    assert int(M[1]["run"][p.r]) <= D.RUN_MAX and int(M[1]["new"][p.r]) == D.LIMIT + 1 > 3630
    assert int(M[2]["live"][p.r]) <= D.ENTRY_MAX and int(M[2]["live"][p.r]) < 3630 * 3 // 4
    assert all(i is not None and i != D.DN_EMPTY for i in M[2]["entry_ids"][p.r])


def test_marker_premises():
    s = D.stream("marker_refused")
    M = D.mirror(s)
    assert D.DN_EMPTY in M[1]["ids"].tolist() and D.DN_EMPTY not in M[2]["ids"].tolist()
    assert D.DN_EMPTY in M[2]["entry_ids"][s.r]        # the id now sits in an entry
    assert M[3]["run"][s.r] == 0 and M[3]["run"].sum() > 0
    n = D.stream("marker_neighbours")
    N = D.mirror(n)
    assert D.DN_EMPTY not in N[1]["ids"].tolist()
    ent = {i for p in range(16) for i in N[2]["entry_ids"][p]}
    assert set(D.MARKER_NEIGHBOURS) <= ent and None not in ent
    k, t = n.steps[1][0], n.steps[1][1]
    assert set(((t[k == 12345]) // D.SIZE - D.WM0 // D.SIZE).tolist()) == set(range(8))


def test_restored_premises():
    keys, far, dn8, sums = (D.stream("restored_" + x) for x in ("keys", "far", "dn8", "sums"))
    for s, n_bad in ((keys, 2), (far, 1), (dn8, 1)):
        rows = _restored(s)
        M = D.mirror(s, rows)
        bad = [p for p in range(s.P) if None in M[1]["entry_ids"][p]]
        assert len(bad) == n_bad
        # one push for each such region, then one that avoids them all
        for i in range(n_bad):
            rg = s.premises[i + 1]["region"]
            assert rg in bad and M[i + 1]["run"][rg] == 30 and M[i + 1]["run"].sum() == 30
        assert all(M[n_bad + 1]["run"][p] == 0 for p in bad) and M[n_bad + 1]["run"].sum() > 100
    mm = D.stream("restored_minmax")
    rows, M = _restored(mm), D.mirror(mm, _restored(mm))
    assert rows["min"][0] == D.I32_MIN - 1 and rows["max"][1] == D.I32_MAX + 1
    for i in (0, 1):  # one push for the region of each such entry (the entries' ids are narrow: min / max alone)
        rg = int(D.region_of([rows["key"][i]])[0])
        assert mm.premises[i + 1]["region"] == rg and M[i + 1]["run"][rg] == 30 == M[i + 1]["run"].sum()
        assert None not in M[i + 1]["entry_ids"][rg] and M[3]["run"][rg] == 0
    r = _restored(far)[0]
    d = r["start"] // D.SIZE - D.WM0 // D.SIZE
    assert d + 8 >= 16  # P16: no compact delta (compact_delta < 0)
    r = _restored(dn8)[0]
    d = r["start"] // D.SIZE - D.WM0 // D.SIZE
    assert 8 <= d < 16 and d + 16 < 32  # P32: a compact delta, no narrow one
    rows = _restored(sums)
    assert rows["sum"].tolist()[:2] == [(1 << 63) - 5, -(1 << 63) + 5]
    assert (rows["min"] >= D.I32_MIN).all() and (rows["max"] <= D.I32_MAX).all()
    out = D.exact_rows(sums, rows)
    by = {int(x["key"]): int(x["sum"]) for x in out}
    assert by[101] == -(1 << 63) + 5 and by[102] == (1 << 63) - 5  # closed form: +10 and -10 across the bounds


def test_width_premises():
    for vt in ("int", "short", "byte"):
        s = D.stream("width_" + vt)
        lo, hi = D.BOUNDS[vt]
        full = D.Stream("x", s.steps, s.deltas, vt="long")
        exact, wrapped = D.exact_rows(full), D.exact_rows(s)
        assert len(exact) == len(wrapped) == 40 * 8 and (wrapped["count"] == 9).all()  # (3 a push: odd)
        for w in np.unique(exact["start"]):  # every window has sums that wrap, upwards and downwards
            e = exact[exact["start"] == w]["sum"]
            assert (e > hi).any() and (e < lo).any()
        assert (wrapped["sum"] >= lo).all() and (wrapped["sum"] <= hi).all()
        assert int(wrapped["max"].max()) == hi and int(wrapped["min"].min()) == lo


def test_sticky_and_uncounted_premises():
    s = D.stream("sticky")
    runs = [s.premises[i]["run"] for i in range(1, 9)]
    assert [n > D.RUN_MAX for n in runs] == [c == "R" for c in "RRCRRRRR"]
    for name, log_s in (("uncounted_p32", 5), ("uncounted_p16", 4)):
        u = D.stream(name)
        M = D.mirror(u)
        bad = np.nonzero(~M[2]["narrow"])[0]
        assert len(bad) == 1 and 400 < bad[0] < 600  # in the middle of the batch
        assert bool(M[2]["compact"][bad[0]]) == (log_s == 5)
        assert M[3]["run"][u.r] == 0 and M[4]["run"][u.r] == 100 == M[4]["run"].sum()


# ---------------------------------------------------------------- the oracle agrees with the exact aggregates
@pytest.mark.parametrize("name", sorted(n for n in D.STREAMS if not n.startswith("restored")))
def test_oracle_rows_are_the_exact_aggregates(name):
    from oracle import oracle as orc
    s = D.stream(name)
    ref = orc.WindowOperatorOracle(assigner="tumbling", size=D.SIZE, value_type=D.ORACLE_VT[s.vt])
    for k, t, v, wm in s.steps:
        if k is not None:
            ref.process(k, t, v)
        ref.watermark(wm)
    assert_rows_equal(ref.rows(), D.exact_rows(s))

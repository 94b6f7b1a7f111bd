"""Every refusal and round boundary of the narrow-keyed dense table (k_dn_aggregate, fw_device.hip), on the streams of
tests/dn_util.py, whose premises tests/test_dn_streams.py proves on the CPU.  Rows are bit-exact against the oracle
(restored state: against exact Python-int aggregates), and every push's push_resumptions delta is asserted with ==:
it is the only observable that says whether k_dn_aggregate committed the push's regions (0) or left some to the
resumed k_dt_aggregate sequence (1)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from flink_amd import KeyGroupRange, TumblingEventTimeWindows
from flink_amd.windowing import CountSumMinMax
from tests import dn_util as D
from tests.parity_util import _sorted, assert_rows_equal
from tests.test_gpu_dense_narrow_table import ROOT, _drive

pytestmark = pytest.mark.gpu

_ROWS, _REF, _SNAP = {}, {}, {}  # in-process rows of the host-push runs, references, edited snapshots: made once


def _op(s, device=False):
    from flink_amd.operator import GpuWindowOperator
    return GpuWindowOperator(TumblingEventTimeWindows.of(D.SIZE), CountSumMinMax(s.vt),
                             key_group_range=KeyGroupRange(0, 0), async_input=device, **s.op_kwargs())


def _restored(s):
    """snapshot_state() of an operator that ran s.pre, edited (the recipe of test_gpu_dn_entry_without_narrow_form)"""
    if s.pre is None:
        return None
    if s.name not in _SNAP:
        a = _op(s)
        _drive(a, s.pre)
        snap = a.snapshot_state()
        a.close()
        assert list(snap) == [0] and len(snap[0]) == 3
        _SNAP[s.name] = D.restored_rows(s, snap[0])
    return _SNAP[s.name]


def _ref(s):
    if s.name not in _REF:
        if s.pre is not None:
            _REF[s.name] = D.exact_rows(s, _restored(s))
        else:
            from oracle import oracle as orc
            ref = orc.WindowOperatorOracle(assigner="tumbling", size=D.SIZE, value_type=D.ORACLE_VT[s.vt])
            for k, t, v, wm in s.steps:
                if k is not None:
                    ref.process(k, t, v)
                ref.watermark(wm)
            _REF[s.name] = ref.rows()
    return _REF[s.name]


def run_stream(s, device=False, each=None):
    """-> rows, push_resumptions delta of every step (host pushes), stats, the stream's whole delta.
    each(e, op): called after step e (host pushes)."""
    op = _op(s, device)
    rs = _restored(s)
    if rs is not None:
        op.initialize_state({0: rs})
    base = prev = op.stats()["push_resumptions"]
    deltas = None
    if device:
        rows = _drive(op, s.steps, True)
    else:
        deltas = []
        for e, step in enumerate(s.steps):
            rows = _drive(op, [step])
            now = op.stats()["push_resumptions"]
            deltas.append(now - prev)
            prev = now
            if each:
                each(e, op)
    st = op.stats()
    op.close()
    if not device:
        _ROWS[s.name] = rows
    return rows, deltas, st, st["push_resumptions"] - base


def _check(name, redone=0):
    s = D.stream(name)
    rows, deltas, st, total = run_stream(s)
    assert_rows_equal(rows, _ref(s), s.vt)
    assert deltas == s.deltas, (deltas, s.deltas)
    assert st["narrow_pass_redone"] == redone
    return s, rows, st


# ---------------------------------------------------------------- (a) round boundaries
def test_gpu_dn_round_boundaries():
    """Region r's run lengths 1, 2, 3, RS - 1, RS, RS + 1, ND RS - 1, ND RS, ND RS + 1, 3 RS + 1, 2 ND RS, 65534,
    65535 and 65536 on one operator with the watermark unchanged, 64 ids with random int32 values.  After every push
    the live state equals the running exact aggregates, so a failure names its run length; only 65536 is refused."""
    s, ls = D.stream("rounds"), D.round_lengths()
    ex = D.Exact()

    def each(e, op):
        k, t, v, wm = s.steps[e]
        if k is not None:
            ex.push(k, t, v)
        want = ex.live()
        ex.watermark(wm, e)
        if k is None:
            return
        got = D.sort_state(op.snapshot_state()[0])
        assert len(got) == len(want), f"run length {ls[e - 1]}: {len(got)} entries, {len(want)} expected"
        for f in want.dtype.names:
            bad = np.nonzero(got[f] != want[f])[0]
            assert bad.size == 0, f"run length {ls[e - 1]}: {f} differs: {got[bad[:3]]} expected {want[bad[:3]]}"

    rows, deltas, st, _ = run_stream(s, each=each)
    assert_rows_equal(rows, _ref(s))
    assert deltas == s.deltas == [0] * len(ls) + [1, 0], deltas
    assert st["narrow_pass_redone"] == 0 and st["narrow_pass_batches"] == len(ls)


# ---------------------------------------------------------------- (b) claim races
def test_gpu_dn_claim_races():
    s, rows, st = _check("claims")
    assert len(rows) == 3000 and (rows["count"] == 3).all()


# ---------------------------------------------------------------- (c) entry and fill limits
def test_gpu_dn_entry_limit():
    """live = EPT NT = 3072 entries are read in (delta 0, also with one claim on top), 3073 are refused.
    `live > LIMIT` (3825) cannot be the first refusal with this instantiation: EPT NT < LIMIT, so `live > EPT NT`
    refuses first (tests/test_dn_streams.py asserts the inequality)."""
    _check("entries")


@pytest.mark.parametrize("name", ["fill_at", "fill_over"])
def test_gpu_dn_fill_limit(name):
    # LIMIT = 3825 new groups fill the table to its limit and are taken; the 3826th claim gets no ticket
    s, rows, st = _check(name)
    assert len(rows) == s.premises[1]["new"]


def test_gpu_dn_region_in_passes():
    """k_dt_aggregate leaves tb.passes[p] != 0 when a region's groups exceed its LDS table and clears it when a push
    ends below 3/4 of that table; nothing else writes it.  A narrow push can meet it: after the refused 3826-group
    push, firing the older window halves the region's entries, and the next one-record push is refused for the
    passes alone (run 1, 1913 narrow entries); the resumed k_dt_aggregate clears them, so the push after is taken."""
    _check("passes")


# ---------------------------------------------------------------- (d) the empty marker
def test_gpu_dn_empty_marker_refused():
    # id 0xFFFFFFFF as a record (M.over), then as an entry of the region (M.refuse); a push elsewhere is taken
    s, rows, st = _check("marker_refused")
    hit = rows[(rows["key"] == -1)]
    assert len(hit) == 1 and hit["start"][0] == (D.WM0 // D.SIZE + 7) * D.SIZE and hit["sum"][0] == -123


def test_gpu_dn_marker_neighbours_taken():
    s, rows, st = _check("marker_neighbours")
    w0 = D.WM0 // D.SIZE * D.SIZE
    got = {(int(x["key"]), int(x["start"] - w0) // D.SIZE) for x in rows}
    want = {(-1, d) for d in range(7)} | {(-2, 7), (D.KEY_MIN, 0), (D.KEY_MIN, 7), (D.KEY_MAX, 0), (D.KEY_MAX, 7),
                                          (0, 0)} | {(12345, d) for d in range(8)}
    assert got == want and (rows["count"] == 4).all() and (rows["end"] == rows["start"] + D.SIZE).all()


# ---------------------------------------------------------------- (e) restored entries without a narrow id
@pytest.mark.parametrize("name", ["restored_keys", "restored_far", "restored_dn8", "restored_minmax"])
def test_gpu_dn_restored_entry_refused(name):
    # keys 2^28 and -2^28 - 1; P16, a window with no compact delta (d < 0); P32, narrow delta 10 (dn >= 8); a minimum
    # of -2^31 - 1 and a maximum of 2^31
    _check(name)


def test_gpu_dn_restored_sums_wrap():
    s, rows, st = _check("restored_sums")
    by = {int(x["key"]): int(x["sum"]) for x in rows}
    assert by[101] == -(1 << 63) + 5 and by[102] == (1 << 63) - 5 and by[103] == 34


# ---------------------------------------------------------------- (f) field widths
@pytest.mark.parametrize("vt", ["int", "short", "byte"])
def test_gpu_dn_field_widths(vt):
    s, rows, st = _check("width_" + vt)
    lo, hi = D.BOUNDS[vt]
    assert st["narrow_pass_batches"] == 3 and len(np.unique(rows["start"])) == 8
    assert (rows["sum"] >= lo).all() and (rows["sum"] <= hi).all()


# ---------------------------------------------------------------- (g) capover and growth
def test_gpu_dn_capover_grows_and_resumes():
    # 2000 new groups, R = 1024: the write-back stops at the buffer's end, nothing is committed; one resumption
    s, rows, st = _check("grow_over")
    assert st["table_grows"] >= 1 and len(rows) == 2000


def test_gpu_dn_commit_then_grow():
    # 800 new groups fit R = 1024: committed by the first launch (no resumption); above 3R/4 sets need_grow, and
    # settle grows the table after the push without suspending anything
    s, rows, st = _check("grow_after")
    assert st["table_grows"] >= 1 and len(rows) == 800


# ---------------------------------------------------------------- (h) the sticky switch and its reset
def test_gpu_dn_sticky_switch_resets():
    s, rows, st = _check("sticky")
    assert st["narrow_pass_batches"] == 8


# ---------------------------------------------------------------- (i) async device pushes
@pytest.mark.parametrize("name", ["entries", "fill_at", "fill_over", "passes", "marker_refused", "marker_neighbours",
                                  "restored_keys", "restored_far", "restored_dn8", "restored_minmax", "restored_sums"])
def test_gpu_dn_async_device_push(name):
    # the resumed sequence behind an async device push with a watermark queued after it (advance_watermark(wait=False))
    s = D.stream(name)
    rows, _, st, total = run_stream(s, device=True)
    assert_rows_equal(rows, _ref(s), s.vt)
    assert total == sum(s.deltas) and st["narrow_pass_redone"] == 0


# ---------------------------------------------------------------- (j) the same rows with the old kernel first
NO_DN = ["rounds", "claims", "marker_refused", "marker_neighbours", "width_int", "width_short", "width_byte"]


@pytest.fixture(scope="module")
def no_dn_rows(tmp_path_factory):
    # FW_NO_DN=1 is read once by the library: one fresh child runs all the streams
    out = tmp_path_factory.mktemp("no_dn") / "rows.npz"
    script = os.path.join(ROOT, "tests", "test_gpu_dense_narrow_table.py")
    p = subprocess.run([sys.executable, script, str(out)] + NO_DN, env=dict(os.environ, FW_NO_DN="1"), cwd=ROOT,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-4000:]
    return np.load(out)


@pytest.mark.parametrize("name", NO_DN)
def test_gpu_dn_same_rows_with_the_compact_table_first(name, no_dn_rows):
    s = D.stream(name)
    if name not in _ROWS:
        run_stream(s)
    assert_rows_equal(no_dn_rows[name], _ref(s), s.vt)
    assert no_dn_rows[name + ".resumptions"] == 0  # (the compact table's kernel refuses none of these)
    assert np.array_equal(_sorted(no_dn_rows[name]), _sorted(_ROWS[name]))


# ---------------------------------------------------------------- (k) the uncounted refusal
def test_gpu_dn_uncounted_refusal_narrow_miss():
    """P32, one record at narrow delta 8 in the middle of a stream: the scatter finds no narrow form, the batch is
    redone with 16-byte records, and k_dn_aggregate, launched first, refuses every region uncounted: one resumption.
    The operator keeps 16-byte records from then on (narrow_pass_batches stops at 2), so no later push is resumed."""
    s, rows, st = _check("uncounted_p32", redone=1)
    assert st["narrow_pass_batches"] == 2 and st["single_pass_redone"] == 0


def test_gpu_dn_uncounted_refusal_no_compact_form():
    """P16, one record 16 windows ahead.  It has no compact form, which k_scatter_rsv checks before the narrow one: the
    batch counts as a redone single pass (single_pass_redone == 1, narrow_pass_redone == 0: RSV_OVER without the
    narrow flag) and takes the offset path with wide records; k_dn_aggregate refuses it uncounted: one resumption.
    Nothing turns narrow records off, so the later batches are narrow again (narrow_pass_batches == 4); the one for
    the far entry's region is refused by the read-in (compact_delta < 0) and resumed, the other is taken."""
    s, rows, st = _check("uncounted_p16", redone=0)
    assert st["narrow_pass_batches"] == 4 and st["single_pass_redone"] == 1

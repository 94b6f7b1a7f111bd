"""Pre-epoch timestamps and odd window sizes through every operator path on the GPU, against the oracle, exactly
(tests/time_edges_util.py builds the inputs, tests/test_oracle_time_edges.py guards them on the CPU and holds the
oracle against the independent restatement tests/window_ref.py).  No tolerance anywhere: keys, window bounds, counts,
sums, minima, maxima, side rows and late counts are compared as integers (t-digest centroids and quantiles as f64
bits; HyperLogLog estimates, an f64 computed from bit-exact registers, as in tests/test_gpu_parity.py).

Sliding windows kept as panes refuse a displaced record (FW_ERR_DISPLACED, DESIGN.md "Event-time arithmetic"): the pane
and combine tests pin the refusal (nothing of the push is taken, the operator goes on exactly), and the same stream
matches the oracle on an operator created with no_panes.

Rows compared on the MI355X run (rows / with a negative start / with start < 0 < end / of windows that hold a displaced
record -- for sliding windows a record with ceil(size / slide) + 1 windows):

  path (cases)                               rows  negative start  start < 0 < end  displaced
  ---------------------------------------  ------  --------------  ---------------  ---------
  general tumbling i64 (5)                  66249           47285              800      45792
  general sliding i64 (6)                  191333          142023             2200     139547
  general tumbling i32 (1)                  13179            9528              200       9225
  general sliding i32 (1)                   36186           26804              400      26295
  panes (displaced refused) host (2)        45550           11901             1600          0
  panes (displaced refused) device (2)      45550           11901             1600          0
  sliding size % slide == 0, no_panes (2)  125747           92098             1600      90188
  dense single pass narrow (2)              21926           13804             1024      13568
  dense single pass compact (2)             21926           13804             1024      13568
  first tumbling (1)                        13179            9528              200       9225
  first sliding (1)                         36186           26804              400      26295
  minBy tumbling (1)                        13211            9412              200       9118
  maxBy sliding (1)                         36125           26891              600      26382
  HyperLogLog tumbling (1)                  13179            9528              200       9225
  HyperLogLog sliding (2)                   78997           58371              800      57316
  t-digest tumbling (1)                      7373            5412              100       5302
  t-digest sliding (1)                      19492           14740              300      14602
  t-digest sliding lateness (1)             31057           23150              300      22907
  Table rows tumbling (1)                   11752            8288              200       7975
  Table rows sliding (1)                    33116           24251              400      23651
  list tumbling (1)                          4760            3552               64       3475
  list sliding (2)                          34766           26024              384      25665
  list tumbling continuous (1)              20943           16645              256      16441
  list sliding continuous (1)               52156           36495              493      36004
  sessions (aggregate) (2)                  15933           13324              616          -
  sessions (list) (1)                        7553            5589              300          -
  combine tumbling (1)                      13179            9528              200       9225
  combine panes (displaced refused) (1)     15182            3938              400          0
  snapshot / restore / continue (1)         13179            9528              200       9225
  heap-format round trip (1)                 1100            1000               50          -
  odd size general tumbling (12)            10510            5222                0       4160
  odd size general sliding (3)              11402            6016              640       6012
  odd size dense (24)                      346644          174210                0     131860
  odd size panes (1)                         1728             192              128          0
  odd size list tumbling (4)                16549           10233                0          -
  odd size list sliding (1)                  2484            1280              128          -
  odd size t-digest tumbling (2)             1342             638                0          -
  odd size t-digest sliding (1)              2484            1280              128          -

("-": sessions have no grid; the odd-size list and t-digest rows were not classified.  A tumbling window has no
extra window: its displaced records go into the window above them.)
"""
import numpy as np
import pytest

from flink_amd import (ContinuousEventTimeTrigger, CountEvictor, EventTimeSessionWindows, EventTimeTrigger,
                       HyperLogLog, PurgingTrigger, SlidingEventTimeWindows, TDigest, TumblingEventTimeWindows)
from flink_amd import _native as N
from flink_amd.windowing import CountSumMinMax, ExtremalElementReduce, FirstElementReduce, RowAggregate
from oracle import oracle as orc
from tests import time_edges_util as T
from tests import window_ref as W
from tests.float_edges_util import dyadic
from tests.parity_util import assert_rows_equal, assert_side_equal

pytestmark = pytest.mark.gpu

_VT = {"i64": "long", "i32": "int", "f64": "double"}
MAX_WM = W.LONG_MAX


def _assigner(cfg):
    a = cfg["assigner"]
    if a == "tumbling":
        return TumblingEventTimeWindows.of(cfg["size"], cfg.get("offset", 0))
    if a == "sliding":
        return SlidingEventTimeWindows.of(cfg["size"], cfg["slide"], cfg.get("offset", 0))
    return EventTimeSessionWindows.with_gap(cfg["gap"])


def _gpu_op(cfg, **kw):
    from flink_amd.operator import GpuWindowOperator
    vt = _VT[cfg.get("value_type", "i64")]
    agg = (FirstElementReduce(vt, "sum") if cfg.get("first") else ExtremalElementReduce(cfg["by"], vt) if cfg.get("by")
           else CountSumMinMax(vt))
    trig = PurgingTrigger.of(EventTimeTrigger.create()) if cfg.get("purging") else EventTimeTrigger.create()
    return GpuWindowOperator(_assigner(cfg), agg, trig, allowed_lateness=cfg.get("lateness", 0),
                             side_output=cfg.get("side_output", False), **kw)


def _report(path, cfg, rows, batches=None):
    c = T.row_classes(cfg, rows, batches)
    print(f"TIME_EDGES | {path} | {c['rows']} | {c['negative_start']} | {c['straddle']} | {c.get('from_displaced', '-')} |")
    return c


def _run_both(cfg, batches, wms, path, device=False, **gpu_kw):
    """the GPU operator and the oracle over the same batches and watermarks; rows, side rows and late counts equal"""
    gpu = _gpu_op(cfg, **gpu_kw)
    ref = orc.WindowOperatorOracle(**cfg)
    for (k, t, v), wm in zip(batches, wms):
        if device and len(k):
            import torch
            gpu.process(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (k, t, v)))
        else:
            gpu.process(k, t, v)
        ref.process(k, t, v)
        gpu.watermark(wm)
        ref.watermark(wm)
    g, r = gpu.rows(), ref.rows()
    assert_rows_equal(g, r, _VT[cfg.get("value_type", "i64")])
    assert_side_equal(gpu.side_rows(), ref.side_rows())
    assert gpu.late_dropped == ref.late_dropped
    st = gpu.stats()
    gpu.close()
    assert len(g) > 0
    return g, st, _report(path, cfg, g, batches), ref.late_dropped


# ---------------------------------------------------------------- general aggregate, ordered path
GENERAL = ([(c, "i64") for c in T.PRE_TUMBLING + T.PRE_SLIDING] + [(T.PRE_TUMBLING[1], "i32"), (T.PRE_SLIDING[0], "i32")]
           + [(dict(assigner="tumbling", size=1000, offset=1, lateness=700), "i64"),
              (dict(assigner="sliding", size=1000, slide=1000), "i64"),   # (size == slide: a displaced record has two windows)
              (dict(assigner="sliding", size=700, slide=1000, offset=999), "i64")])


@pytest.mark.parametrize("cfg,vt", GENERAL, ids=[f"{i}-{v}" for i, (_, v) in enumerate(GENERAL)])
def test_gpu_pre_epoch_general_aggregate(cfg, vt):
    # count / sum / min / max through classify, scatter, k_aggregate and -- records arrive up to 1.5 sizes late against
    # a bound of 0.4 -- the ordered replay (late firings, partially late displaced records, side output, purging).
    # expected_entries below 65536 keeps tumbling windows off the dense path (its own test below).
    cfg = dict(cfg, value_type=vt)
    batches, wms = T.pre_epoch_stream(cfg)
    g, st, c, late = _run_both(cfg, batches, wms, f"general {cfg['assigner']} {vt}", expected_entries=20_000)
    assert c["negative_start"] >= 1000 and c["from_displaced"] >= 1000
    assert late > 0 or cfg.get("side_output")
    if cfg.get("lateness") or cfg["assigner"] == "sliding":
        assert st["slow_path_records"] > 0


# ---------------------------------------------------------------- panes: the refusal, and windows instead
def _not_displaced(cfg, batches):
    off, step = cfg.get("offset", 0), cfg["slide"]
    out = []
    for k, t, v in batches:
        m = np.array([not W.is_displaced(x, off, step) for x in t.tolist()], dtype=bool)
        out.append((k[m], t[m], v[m]))
    return out


@pytest.mark.parametrize("device", [False, True], ids=["host-push", "device-push"])
@pytest.mark.parametrize("cfg", T.PRE_PANES, ids=["3s-1s", "3s-500ms-offset"])
def test_gpu_pre_epoch_panes_refuse_displaced_records(cfg, device):
    # a pane operator refuses a push that holds a displaced record -- error code, message, nothing taken: no state
    # entry, no record counted, no late drop -- and then runs the stream's other records (pre-epoch ones on the grid and
    # in [offset - slide, offset) among them) exactly as the oracle does.  Refusals recur while the watermark is below
    # offset + size - slide - 1; after that a displaced record is late in every window and is dropped as in the oracle.
    batches, wms = T.pre_epoch_stream(cfg)
    kept = _not_displaced(cfg, batches)
    gpu = _gpu_op(cfg)
    ref = orc.WindowOperatorOracle(**cfg)

    def push(k, t, v):
        if device and len(k):
            import torch
            gpu.process(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (k, t, v)))
        else:
            gpu.process(k, t, v)

    refused, prev_wm = 0, W.LONG_MIN
    for (k, t, v), (kk, kt, kv), wm in zip(batches, kept, wms):
        if len(kk) < len(k) and prev_wm < cfg.get("offset", 0) + cfg["size"] - cfg["slide"] - 1:
            before = gpu.stats()
            with pytest.raises(N.NativeError, match="size / slide \\+ 1 windows") as e:
                push(k, t, v)
            assert e.value.code == N.FW_ERR_DISPLACED
            after = gpu.stats()
            assert all(after[f] == before[f] for f in ("records_in", "keyed_state_entries", "late_records_dropped",
                                                       "pending_rows"))
            refused += 1
            k, t, v = kk, kt, kv
        push(k, t, v)
        ref.process(k, t, v)
        gpu.watermark(wm)
        ref.watermark(wm)
        prev_wm = wm
    assert refused >= 2
    # the watermark is past 0 now: displaced records are late in all their windows, and dropped as the oracle drops them
    k, t, v = batches[0]
    push(k, t, v)
    ref.process(k, t, v)
    gpu.watermark(MAX_WM)
    ref.watermark(MAX_WM)
    g = gpu.rows()
    assert_rows_equal(g, ref.rows())
    assert gpu.late_dropped == ref.late_dropped >= len(k)
    gpu.close()
    c = _report(f"panes (displaced refused) {'device' if device else 'host'}", cfg, g, kept)
    assert c["negative_start"] >= 500 and c["straddle"] >= 100 and c["from_displaced"] == 0


@pytest.mark.parametrize("cfg", T.PRE_PANES, ids=["3s-1s", "3s-500ms-offset"])
def test_gpu_pre_epoch_no_panes_takes_displaced_records(cfg):
    # the same streams, whole, on an operator created with no_panes: windows, size / slide + 1 of them for a displaced
    # record, exactly the oracle's rows
    batches, wms = T.pre_epoch_stream(cfg)
    g, st, c, late = _run_both(cfg, batches, wms, "sliding size % slide == 0, no_panes", no_panes=True,
                               expected_entries=20_000)
    assert c["from_displaced"] >= 1000 and c["straddle"] >= 100


# ---------------------------------------------------------------- dense single pass: narrow and compact records
@pytest.mark.parametrize("device", [False, True], ids=["host-push", "async-device-push"])
@pytest.mark.parametrize("wide_keys", [False, True], ids=["narrow", "compact"])
def test_gpu_pre_epoch_dense_single_pass(wide_keys, device):
    # the recipe of test_gpu_narrow_records_and_fallback: dense tumbling regions, single-pass batches whose records are
    # narrow (8 bytes: 29-bit key, 3-bit window delta from the watermark's window, int32 value) or, with keys beyond
    # 2^28, compact (16 bytes, the delta counted from 2^(log_s - 1) windows before the watermark's).  The base is
    # negative, crosses zero inside a batch, and the first batch (no watermark yet) has no base at all.
    cfg = dict(assigner="tumbling", size=100, offset=1)
    batches, wms = T.pre_epoch_stream(cfg, n=60_000, batch=7_500, num_keys=512, disorder=0.3, bound=0.2, span=(-14, 8))
    if wide_keys:
        batches = [(k + (1 << 30), t, v) for k, t, v in batches]
    assert sum(w < 0 for w in wms) >= 2
    assert any(len(t) and t.min() < -50 and t.max() > 101 for _, t, _ in batches)  # a batch with windows on both sides of 0
    g, st, c, late = _run_both(cfg, batches, wms, f"dense single pass {'compact' if wide_keys else 'narrow'}", device=device,
                               max_batch=1 << 15)
    assert st["single_pass_batches"] >= 4
    assert (st["narrow_pass_batches"] >= 2) == (not wide_keys)
    assert c["negative_start"] >= 1000 and c["from_displaced"] >= 1000


# ---------------------------------------------------------------- first element, minBy / maxBy
@pytest.mark.parametrize("cfg", [dict(T.PRE_TUMBLING[1], first=True), dict(T.PRE_SLIDING[0], first=True),
                                 dict(T.PRE_TUMBLING[2], by="min"), dict(T.PRE_SLIDING[1], by="max")],
                         ids=["first-tumbling", "first-sliding", "minby-tumbling", "maxby-sliding"])
def test_gpu_pre_epoch_first_element_and_extremal(cfg):
    # the arrival ordinal rides above the window count in a partitioned record (nwin < 2^16, the extra window included)
    batches, wms = T.pre_epoch_stream(cfg)
    if cfg.get("by"):
        batches = [(k, t, v % 5) for k, t, v in batches]  # ties: broken by arrival order
    g, st, c, _ = _run_both(cfg, batches, wms, f"{'first' if cfg.get('first') else cfg['by'] + 'By'} {cfg['assigner']}",
                            expected_entries=20_000)
    assert c["from_displaced"] >= 1000


# ---------------------------------------------------------------- HyperLogLog
def _hll_rows_equal(g, r):
    ks = lambda a: a[np.lexsort((a["start"], a["key"], a["epoch"]))]  # noqa: E731
    g, r = ks(g), ks(r)
    assert len(g) == len(r) > 0
    for f in ("epoch", "key", "start", "end", "count", "min", "max"):
        assert np.array_equal(g[f], r[f]), f
    np.testing.assert_allclose(g["sum"].view(np.float64), r["sum"].view(np.float64), rtol=1e-9)


@pytest.mark.parametrize("cfg", [T.PRE_TUMBLING[1], T.PRE_SLIDING[0], T.PRE_PANES[0]],
                         ids=["tumbling", "sliding-2500-1000", "sliding-3000-1000"])
def test_gpu_pre_epoch_hll(cfg):
    # a record raises its register in every one of its windows (the fan-out loops take the extra window's block too)
    from flink_amd.operator import GpuWindowOperator
    batches, wms = T.pre_epoch_stream(cfg)
    gpu = GpuWindowOperator(_assigner(cfg), HyperLogLog(8), expected_entries=30_000)
    ref = orc.WindowOperatorOracle(**cfg, hll_p=8)
    for (k, t, v), wm in zip(batches, wms):
        gpu.process(k, t, v)
        ref.process(k, t, v)
        gpu.watermark(wm)
        ref.watermark(wm)
    assert gpu.late_dropped == ref.late_dropped
    g = gpu.rows()
    _hll_rows_equal(g, ref.rows())
    gpu.close()
    assert _report(f"HyperLogLog {cfg['assigner']}", cfg, g, batches)["from_displaced"] >= 1000


# ---------------------------------------------------------------- t-digest
def _run_tdigest(cfg, batches, wms, delta=40, **kw):
    from flink_amd.operator import GpuWindowOperator
    q = (0.5, 0.95, 0.99)
    trig = PurgingTrigger.of(EventTimeTrigger.create()) if cfg.get("purging") else EventTimeTrigger.create()
    gpu = GpuWindowOperator(_assigner(cfg), TDigest(delta, q, export=True), trig, allowed_lateness=cfg.get("lateness", 0), **kw)
    ref = orc.WindowOperatorOracle(**cfg, tdigest=delta, quantiles=q)
    g_rows, g_dig = [], []
    for epoch, ((k, t, v), wm) in enumerate(zip(batches, wms)):
        if len(k):
            gpu.process(k, t, v)
            ref.process(k, t, v)
        gpu.advance_watermark(wm)
        g_dig += gpu.drain_digests()
        g_rows.append(gpu.drain_rows(epoch))
        ref.watermark(wm)
    assert gpu.late_dropped == ref.late_dropped
    gpu.close()
    g_rows, r_rows = np.concatenate(g_rows), ref.rows()
    assert len(g_rows) == len(r_rows) > 0
    go = np.lexsort((g_rows["count"], g_rows["start"], g_rows["key"], g_rows["epoch"]))
    ro = np.lexsort((r_rows["count"], r_rows["start"], r_rows["key"], r_rows["epoch"]))
    for f in ("epoch", "key", "start", "end", "count", "sum", "min", "max"):  # (quantiles as f64 bits)
        bad = np.nonzero(g_rows[f][go] != r_rows[f][ro])[0]
        assert bad.size == 0, f"{f} differs at {bad[:5]}: {g_rows[go][bad[:3]]} vs {r_rows[ro][bad[:3]]}"
    for a, b in zip(go, ro):
        (gs, gw), (rs, rw) = g_dig[a], ref.digest(int(b))
        assert np.array_equal(gw, rw) and np.array_equal(gs.view(np.int64), rs.view(np.int64))
    return g_rows


TD_CFGS = [T.PRE_TUMBLING[2], T.PRE_SLIDING[1], dict(assigner="sliding", size=2000, slide=500, lateness=300)]


@pytest.mark.parametrize("cfg", TD_CFGS, ids=["tumbling", "sliding", "sliding-lateness"])
def test_gpu_pre_epoch_tdigest(cfg):
    # one item per (record, window) into the compression (mb x wpr items), and under allowed lateness the ordered
    # path's chains td_olink[element * wpr + window]: the extra window is window wpr - 1 of its element
    batches, wms = T.pre_epoch_stream(cfg, n=30_000, batch=5_000, num_keys=100)
    batches = [(k, t, dyadic(k, v, "f64")) for k, t, v in batches]
    g = _run_tdigest(cfg, batches, wms, expected_entries=30_000)
    assert _report(f"t-digest {cfg['assigner']}{' lateness' if cfg.get('lateness') else ''}", cfg, g, batches)["from_displaced"] >= 1000
    if cfg.get("lateness"):
        keys = np.stack([g["key"], g["start"]], axis=1)
        assert len(np.unique(keys, axis=0)) < len(keys)  # windows fired more than once


# ---------------------------------------------------------------- Table API rows (FW_AGG_ROW)
ROW_TYPES = ["i64", "i32"]
ROW_SPECS = [("count_star", 0), ("count", 0), ("sum", 0), ("avg", 0), ("min", 0), ("max", 0), ("sum", 1), ("min", 1)]


@pytest.mark.parametrize("cfg", [T.PRE_TUMBLING[1], dict(assigner="sliding", size=2500, slide=1000, offset=300)],
                         ids=["tumbling", "sliding-split"])
def test_gpu_pre_epoch_table_rows(cfg):
    from flink_amd.operator import GpuWindowOperator
    batches, wms = T.pre_epoch_stream(cfg, n=30_000, batch=5_000)
    rng = np.random.default_rng(0x7AB1E)
    gpu = GpuWindowOperator(_assigner(cfg), RowAggregate(("long", "int"), tuple(ROW_SPECS)), max_batch=1 << 13)
    ref = orc.WindowOperatorOracle(**cfg, row=(ROW_TYPES, ROW_SPECS))
    for (k, t, v), wm in zip(batches, wms):
        cols = [v << 31, v % 100_003]
        nulls = (rng.random(len(k)) < 0.15).astype(np.uint8) | ((rng.random(len(k)) < 0.15).astype(np.uint8) << 1)
        gpu.process_row_batch(k, t, cols, nulls)
        ref.process_rows(k, t, cols, nulls)
        gpu.watermark(wm)
        ref.watermark(wm)
    g, r = gpu.rows(), ref.rows()
    (gv, gn), (rv, rn) = gpu.row_results(), ref.row_results()
    gi = np.lexsort((g["start"], g["key"], g["epoch"]))
    ri = np.lexsort((r["start"], r["key"], r["epoch"]))
    assert len(gi) == len(ri) > 0
    for f in ("epoch", "key", "start", "end", "count"):
        assert np.array_equal(g[f][gi], r[f][ri]), f
    assert np.array_equal(gn[gi], rn[ri])
    live = (gn[gi, None] >> np.arange(len(ROW_SPECS))[None, :]) & 1 == 0
    assert np.array_equal(np.where(live, gv[gi], 0), np.where(live, rv[ri], 0))
    assert gpu.stats()["late_records_dropped"] == ref.late_dropped
    gpu.close()
    assert _report(f"Table rows {cfg['assigner']}", cfg, g, batches)["from_displaced"] >= 1000


# ---------------------------------------------------------------- the list operator
def _list_pair(cfg, interval=0, evict=0):
    from flink_amd.listwindow import GpuListWindowOperator
    from tests.continuous_ref import ContinuousRef
    trig = ContinuousEventTimeTrigger.of(interval) if interval else EventTimeTrigger.create()
    gpu = GpuListWindowOperator(_assigner(cfg), trig, CountEvictor.of(evict, False) if evict else None,
                                allowed_lateness=cfg.get("lateness", 0), value_type="long")
    if interval:
        ref = ContinuousRef(trigger="continuous", interval=interval, evictor="count" if evict else "none", evict_arg=evict,
                            **cfg)
    elif cfg["assigner"] == "session":
        ref = orc.ListWindowOracle(assigner="session", gap=cfg["gap"], lateness=cfg.get("lateness", 0),
                                   evictor="count" if evict else "none", evict_arg=evict)
    else:
        ref = orc.ListWindowOracle(evictor="count" if evict else "none", evict_arg=evict, **cfg)
    return gpu, ref


LIST_CFGS = [(dict(assigner="tumbling", size=100, offset=99), 0, 3), (dict(assigner="sliding", size=90, slide=30, offset=1), 0, 3),
             (dict(assigner="sliding", size=100, slide=25, lateness=40), 0, 0),
             (dict(assigner="tumbling", size=100, offset=1), 33, 0), (dict(assigner="sliding", size=100, slide=25), 33, 0)]


@pytest.mark.parametrize("cfg,interval,evict", LIST_CFGS,
                         ids=["tumbling-evictor", "sliding-evictor", "sliding-lateness", "continuous-tumbling", "continuous-sliding"])
def test_gpu_pre_epoch_list_operator(cfg, interval, evict):
    # window contents with CountEvictor, and ContinuousEventTimeTrigger with an interval (33) that does not divide the
    # size: its first timer ts - ts % interval + interval lands one interval above a pre-epoch element's grid point.
    # The list operator counts a record's windows before it appends (no per-record bound), so the extra window fits.
    from tests.test_gpu_list import _assert_same
    gpu, ref = _list_pair(cfg, interval, evict)
    batches, wms = T.pre_epoch_stream(cfg, n=20_000, batch=2_500, num_keys=64, disorder=1.2, bound=0.8)
    for (k, t, v), wm in zip(batches, wms):
        gpu.process(k, t, v)
        ref.process(k, t, v)
        gpu.watermark(wm)
        ref.watermark(wm)
    _assert_same(gpu, ref)
    assert gpu.late_dropped == ref.late_dropped
    g = gpu.rows()
    gpu.close()
    c = _report(f"list {cfg['assigner']}{' continuous' if interval else ''}", cfg, g, batches)
    assert c["from_displaced"] >= 1000 and c["straddle"] >= 1


# ---------------------------------------------------------------- sessions that merge across 0
@pytest.mark.parametrize("cfg", T.PRE_SESSIONS, ids=["plain", "lateness-side-output"])
def test_gpu_pre_epoch_sessions_aggregate(cfg):
    batches, wms = T.pre_epoch_stream(cfg, num_keys=300)
    g, st, c, _ = _run_both(cfg, batches, wms, "sessions (aggregate)")
    assert c["straddle"] >= 5 and (g["end"] - g["start"] > cfg["gap"]).any() and st["state_merges"] > 0


def test_gpu_pre_epoch_sessions_list():
    from tests.test_gpu_list import _assert_same
    cfg = dict(assigner="session", gap=30)
    gpu, ref = _list_pair(cfg)
    batches, wms = T.pre_epoch_stream(cfg, n=20_000, batch=2_500, num_keys=300, disorder=1.2, bound=0.8)
    for (k, t, v), wm in zip(batches, wms):
        gpu.process(k, t, v)
        ref.process(k, t, v)
        gpu.watermark(wm)
        ref.watermark(wm)
    _assert_same(gpu, ref)
    assert gpu.late_dropped == ref.late_dropped
    g = gpu.rows()
    gpu.close()
    c = _report("sessions (list)", cfg, g)
    assert c["straddle"] >= 1 and (g["end"] - g["start"] > 30).any()


# ---------------------------------------------------------------- pre-shuffle combine, world 1
def _combine(cfg, pushes, wms):
    """comb -> partials -> op for every (k, t, v) of `pushes`; returns the receiving operator's rows"""
    import torch
    comb, op = _gpu_op(cfg), _gpu_op(cfg)
    ref = orc.WindowOperatorOracle(**cfg)
    rows = []
    for (k, t, v), wm in zip(pushes, wms):
        if len(k):
            comb.process_batch(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (k, t, v)))
            parts, _ = comb.combine_extract(1)
            op.push_partials(*(c.clone() for c in parts), config=parts.config)
            ref.process(k, t, v)
        rows.append(op.process_watermark(wm))
        ref.watermark(wm)
    g = np.concatenate(rows)
    assert_rows_equal(g, ref.rows())
    assert op.late_dropped == ref.late_dropped
    comb.close()
    op.close()
    return g


def test_gpu_pre_epoch_combine_tumbling():
    cfg = T.PRE_TUMBLING[1]
    batches, wms = T.pre_epoch_stream(cfg)
    g = _combine(cfg, batches, wms)
    assert _report("combine tumbling", cfg, g, batches)["from_displaced"] >= 1000


def test_gpu_pre_epoch_combine_panes_refuses_displaced_records():
    # the combiner is a pane operator whose watermark never moves: it refuses every push that holds a displaced record
    # (nothing taken: the next extraction carries only what was accepted), and combining the others is exact
    import torch
    cfg = T.PRE_PANES[0]
    batches, wms = T.pre_epoch_stream(cfg)
    kept = _not_displaced(cfg, batches)
    comb = _gpu_op(cfg)
    with pytest.raises(N.NativeError, match="size / slide \\+ 1 windows") as e:
        comb.process_batch(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in batches[0]))
    assert e.value.code == N.FW_ERR_DISPLACED and comb.stats()["records_in"] == 0
    parts, counts = comb.combine_extract(1)
    assert counts == [0]
    comb.close()
    g = _combine(cfg, kept, wms)
    c = _report("combine panes (displaced refused)", cfg, g, kept)
    assert c["negative_start"] >= 500 and c["straddle"] >= 100
    with pytest.raises(N.NativeError) as e:  # windows instead of panes are not combinable
        _gpu_op(cfg, no_panes=True).combine_extract(1)
    assert e.value.code == N.FW_ERR_UNSUPPORTED


# ---------------------------------------------------------------- snapshot -> restore -> continue
def test_gpu_pre_epoch_snapshot_restore_continue():
    # the cut falls while the watermark is negative: the in-flight windows of the snapshot have negative starts
    from flink_amd.keygroups import compute_key_group_range_for_operator_index
    cfg = T.PRE_TUMBLING[1]
    batches, wms = T.pre_epoch_stream(cfg)
    ref = orc.WindowOperatorOracle(**cfg)
    for (k, t, v), wm in zip(batches, wms):
        ref.process(k, t, v)
        ref.watermark(wm)
    cut = 2
    assert wms[cut - 1] < -10 * cfg["size"]
    a = _gpu_op(cfg, max_parallelism=128, expected_entries=20_000)
    for (k, t, v), wm in zip(batches[:cut], wms[:cut]):
        a.process(k, t, v)
        a.watermark(wm)
    got = [a.rows()]
    snap = a.snapshot_state()
    live = np.concatenate([r for r in snap.values() if len(r)])
    assert len(live) > 100 and (live["start"] < 0).all()
    a.close()
    from flink_amd.keygroups import assign_to_key_group, long_hash_code
    parts = []
    for idx in range(2):
        kgr = compute_key_group_range_for_operator_index(128, 2, idx)
        op = _gpu_op(cfg, max_parallelism=128, key_group_range=kgr, expected_entries=20_000)
        op.initialize_state(snap)
        parts.append((kgr, op))
    for (k, t, v), wm in zip(batches[cut:], wms[cut:]):
        kg = np.array([assign_to_key_group(long_hash_code(int(x)), 128) for x in k], dtype=np.int64)
        for kgr, op in parts:
            m = (kg >= kgr.start_key_group) & (kg <= kgr.end_key_group)
            op.process(k[m], t[m], v[m])
            op.watermark(wm)
    for _, op in parts:
        r = op.rows()
        r["epoch"] += cut
        got.append(r)
        op.close()
    g = np.concatenate(got)
    assert_rows_equal(g, ref.rows())
    _report("snapshot / restore / continue", cfg, g, batches)


def test_gpu_pre_epoch_heap_format_round_trip():
    # the GPU's state rows with negative window starts through the heap backend's key-group section format
    # (flink_amd/heapstate.py: TimeWindowSerializer's two longs, the state table's iteration order by
    # TimeWindow.hashCode) and back into a fresh operator, which then fires them as the oracle does
    from flink_amd import heapstate as H
    from flink_amd.operator import STATE_DTYPE, GpuWindowOperator
    cfg = dict(assigner="tumbling", size=1000, offset=999)
    n = 4000
    k = np.arange(n, dtype=np.int64) % 50
    t = -20_000 + (np.arange(n, dtype=np.int64) * 23_000) // n
    v = (np.arange(n, dtype=np.int64) * 7919) % 1000 - 500
    names = [f"key{i}" for i in range(50)]
    ids = {s: i for i, s in enumerate(names)}
    mk = lambda: GpuWindowOperator(_assigner(cfg), FirstElementReduce("int"), key_type="hashed", max_parallelism=1)  # noqa: E731
    from flink_amd.keygroups import string_hash_code
    kh = np.array([string_hash_code(names[i]) for i in k], dtype=np.int32)
    a = mk()
    a.process(k, t, v, key_hash=kh)
    a.watermark(-10_500)
    first = a.rows()
    rows = a.snapshot_key_group(0)
    a.close()
    assert len(rows) > 100 and (rows["start"] < 0).any() and ((rows["start"] < 0) & (rows["end"] > 0)).any()
    passthrough = {int(r["max"]): (names[int(r["key"])], 0) for r in rows}
    mappings = H.heap_from_reduce_rows(rows, names.__getitem__, passthrough, 1)
    timers = set(H.rows_to_timers(rows, names.__getitem__))
    tup = H.TupleSer(H.StringSer(), H.IntSer())
    ser = {"window-contents": (H.TimeWindowSer(), H.StringSer(), tup)}
    sec = H.write_key_group_section(0, [(0, "window-contents", H.heap_section_order(mappings, string_hash_code,
                                                                                    H.time_window_hash))], ser)
    back = H.read_key_group_section(H.DataInput(sec), 0, ["window-contents"], ser)["window-contents"]
    assert sorted(back) == sorted(mappings)
    rows2, _ = H.reduce_rows_from_heap(back, timers, ids.__getitem__, 1, ordinal_base=n)
    arr = np.zeros(len(rows2), dtype=STATE_DTYPE)
    for i, r in enumerate(rows2):
        for f in STATE_DTYPE.names:
            arr[i][f] = r[f]
    b = mk()
    b.restore_key_group(0, arr)
    b.watermark(MAX_WM)
    g = np.concatenate([first, b.rows()])
    b.close()
    ref = orc.WindowOperatorOracle(**cfg, first=True, value_type="i32")
    ref.process(k, t, v)
    ref.watermark(-10_500)
    ref.watermark(MAX_WM)
    r = ref.rows()
    # (the heap state of a reduce keeps no element count and no ordinal: window bounds, keys and sums are what returns)
    key = lambda x: sorted(zip(x["key"].tolist(), x["start"].tolist(), x["end"].tolist(), x["sum"].tolist()))  # noqa: E731
    assert key(g) == key(r)
    _report("heap-format round trip", cfg, g)


# ---------------------------------------------------------------- odd sizes
@pytest.mark.parametrize("cfg", T.ODD_TUMBLING + T.ODD_NONPANE_PAIRS,
                         ids=[f"{c['assigner']}-{c['size']}" for c in T.ODD_TUMBLING + T.ODD_NONPANE_PAIRS])
def test_gpu_odd_sizes_general_aggregate(cfg):
    # the reciprocal remainder on the device (jrem: |t|, the dividend's sign, l == 0 for size 1, l = 62 / 63 for
    # 2^61 + 1 / 2^62 + 1) through classify and the ordered replay
    batches, wms = T.odd_stream(cfg)
    g, st, c, _ = _run_both(cfg, batches, wms, f"odd size general {cfg['assigner']}", expected_entries=20_000)
    assert c["negative_start"] >= 1 and (g["start"] >= 0).any()


@pytest.mark.parametrize("device", [False, True], ids=["host-push", "async-device-push"])
@pytest.mark.parametrize("size", T.ODD_SIZES)
def test_gpu_odd_sizes_dense_single_pass(size, device):
    # dense regions: compact and narrow window deltas through div_inv(start - cbase); sizes for which no base is
    # representable (2^62 + 1: 2^(log_s - 1) windows below the watermark's leave the long range) take the wide form
    cfg = dict(assigner="tumbling", size=size)
    batches, wms = T.odd_stream(cfg, num_keys=2048)
    g, st, c, _ = _run_both(cfg, batches, wms, "odd size dense", device=device, max_batch=1 << 15)
    assert c["negative_start"] >= 1 and (g["start"] >= 0).any()
    assert st["single_pass_batches"] >= 1 or size > (1 << 60)


def test_gpu_odd_sizes_panes():
    cfg = T.ODD_PANE_PAIR
    batches, wms = T.odd_stream(cfg, floor=T.odd_floor(cfg))
    g, st, c, _ = _run_both(cfg, batches, wms, "odd size panes")
    assert c["straddle"] >= 1 and c["from_displaced"] == 0


@pytest.mark.parametrize("cfg,interval", [(dict(assigner="tumbling", size=7), 0), (dict(assigner="sliding", size=7, slide=3), 0),
                                          (dict(assigner="tumbling", size=1023), 100),
                                          (dict(assigner="tumbling", size=(1 << 32) + 1), 0),
                                          (dict(assigner="tumbling", size=(1 << 61) + 1), 0)],
                         ids=["7", "7-3", "1023-continuous", "2^32+1", "2^61+1"])
def test_gpu_odd_sizes_list_operator(cfg, interval):
    # the list operator takes window starts with a plain % (fw_list.hip w_start_of): the two operators agree with the
    # oracle, so with each other
    from tests.test_gpu_list import _assert_same
    gpu, ref = _list_pair(cfg, interval)
    batches, wms = T.odd_stream(cfg, n=12_000, batch=2_000)
    for (k, t, v), wm in zip(batches, wms):
        gpu.process(k, t, v)
        ref.process(k, t, v)
        gpu.watermark(wm)
        ref.watermark(wm)
    _assert_same(gpu, ref)
    assert gpu.late_dropped == ref.late_dropped
    g = gpu.rows()
    gpu.close()
    assert _report(f"odd size list {cfg['assigner']}", cfg, g)["negative_start"] >= 1


@pytest.mark.parametrize("cfg", [dict(assigner="tumbling", size=1023), dict(assigner="sliding", size=7, slide=3),
                                 dict(assigner="tumbling", size=(1 << 61) + 1)], ids=["1023", "7-3", "2^61+1"])
def test_gpu_odd_sizes_tdigest(cfg):
    batches, wms = T.odd_stream(cfg, n=12_000, batch=2_000)
    batches = [(k, t, dyadic(k, v, "f64")) for k, t, v in batches]
    g = _run_tdigest(cfg, batches, wms, expected_entries=30_000)
    assert _report(f"odd size t-digest {cfg['assigner']}", cfg, g)["negative_start"] >= 1

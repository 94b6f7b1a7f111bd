"""Timestamps at both ends of the long range through the operator paths on the GPU, against the oracle, exactly.  The
streams come from the registry tests/time_edges_util.WRAP_CASES only; tests/test_oracle_wrap_edges.py vets every entry
on the CPU (nothing of the runaway set, the reference completes under its cap, bounded rows) and asserts what the
streams cover.  Rows are compared per watermark epoch, with no tolerance, as in tests/test_gpu_time_edges.py.

Java longs wrap and the operators follow them: a window whose end wraps past Long.MAX_VALUE is late from the first
watermark on, one that ends at Long.MIN_VALUE has maxTimestamp Long.MAX_VALUE and fires at the final watermark only,
and ts - offset + size past Long.MAX_VALUE leaves a start above ts that wraps to the bottom of the range.  Refusals
(FW_ERR_TIME_RANGE, DESIGN.md "Event-time arithmetic") are pinned here: sliding windows kept as panes and the combiner
(the same stream is exact with no_panes; a tumbling combiner refuses its extraction once it took a record at or above
its window's end), the sliding assigner's runaway set on every sliding operator, and a sliding t-digest.

Rows compared on the MI355X run (rows / of a wrapped window, end < start / that end at Long.MIN_VALUE / that reach the
other end of the range from their stream's: a top stream's rows that end below 0; no window of a bottom stream wraps,
tests/test_oracle_wrap_edges.py test_bottom_windows_never_wrap); per case in profiles/wrap_edges/rows.txt:

  path (cases)                                      rows end < start end == MIN other end
  ---------------------------------------------- ------- ----------- ---------- ---------
  general i64 (52)                                 89652       11726       2560     13502
  general i32 host push (4)                         5858         745        512       846
  general i64 device push (4)                       5858         745        512       846
  dense single pass host (3)                        3533         768        768      1153
  dense single pass device (3)                      3533         768        768      1153
  panes (refused records left out) (8)              5324           0          0         0
  panes device columns (1)                           924           0          0         0
  panes device columns, pipelined (2)               1340           0          0         0
  sliding size % slide == 0, no_panes (8)          29276        7794          0      7794
  combine panes (refused records left out) (1)       924           0          0         0
  combine tumbling (1)                              1096           0          0         0
  sessions (aggregate) (6)                          4142        2386         14      2386
  sessions (list) (4)                               3518        2386         14      2386
  list (15)                                        27000        3657       1536      4302
  list continuous (2)                              65930         256          0       869
  first (2)                                         2466         745        512       846
  minBy (2)                                         3661         256          0       437
  maxBy (1)                                         2167         931          0       931
  HyperLogLog (3)                                   4857         745        512       846
  t-digest (5)                                      7680         512        512       735
  Table rows (2)                                    2466         745        512       846
  snapshot / restore / continue (2)                 2466         745        512       846
  heap-format round trip (2)                         450         100         50       200

(panes, combine: the rows of the records that are not refused.)
"""
import numpy as np
import pytest

from flink_amd import HyperLogLog, _native as N
from flink_amd.windowing import RowAggregate
from oracle import oracle as orc
from tests import time_edges_util as T
from tests import window_ref as W
from tests.float_edges_util import dyadic
from tests.parity_util import assert_rows_equal
from tests.test_gpu_time_edges import (ROW_SPECS, ROW_TYPES, _assigner, _combine, _gpu_op, _hll_rows_equal, _list_pair,
                                       _run_both, _run_tdigest)

pytestmark = pytest.mark.gpu
MIN, MAX = W.LONG_MIN, W.LONG_MAX


def _report(path, name, rows):
    c = T.wrap_row_classes(rows, T.WRAP_CASES[name]["end"])
    print(f"WRAP_EDGES | {path} | {name} | {c['rows']} | {c['wrapped']} | {c['end_min']} | {c['far']} |")
    return c


def _names(*prefixes, ends=("top", "bottom"), schedules=(T.COLD, T.WARM)):
    return [f"{p}-{e}-{s}" for p in prefixes for e in ends for s in schedules if f"{p}-{e}-{s}" in T.WRAP_CASES]


def _covered(name, c):
    """what the CPU test asserts of the oracle's rows holds of the GPU's (they are equal), restated for the reader"""
    if T.WRAP_CASES[name]["end"] == "top":
        assert c["wrapped"] >= 200
    else:
        assert c["wrapped"] == 0


# ---------------------------------------------------------------- general aggregate: classify, scatter, ordered replay
GENERAL = (_names("tumbling-o0", "tumbling-o1", "tumbling-o999", "tumbling-o808", "sliding-2500-o0", "sliding-2500-o808",
                  "sliding-2500-o308", "sliding-700-1000", "tumbling-late", "tumbling-late-purge-side",
                  "sliding-late-purge-side", "tumbling-late-max", "sliding-late-max"))


@pytest.mark.parametrize("name", GENERAL)
def test_gpu_wrap_general_aggregate(name):
    # expected_entries below 65536 keeps tumbling windows off the dense path (its own test below).  A sliding record of
    # which one window's end wraps goes to the ordered replay, which tests every window by itself: under a warm
    # schedule its wrapped windows are late and the others are not.
    cfg, batches, wms = T.wrap_case(name)
    g, st, _, late = _run_both(cfg, batches, wms, f"wrap general {name}", expected_entries=20_000)
    _covered(name, _report("general i64", name, g))
    if cfg["assigner"] == "sliding" and cfg["size"] > cfg["slide"] and T.WRAP_CASES[name]["end"] == "top":
        assert st["slow_path_records"] >= 1000


@pytest.mark.parametrize("name", ["tumbling-o808-top-warm", "sliding-2500-o308-top-warm", "sliding-2500-o0-bottom-warm",
                                  "tumbling-o999-bottom-cold"])
@pytest.mark.parametrize("vt,device", [("i32", False), ("i64", True)], ids=["i32-host", "i64-device"])
def test_gpu_wrap_general_aggregate_i32_and_device_push(name, vt, device):
    cfg, batches, wms = T.wrap_case(name)
    cfg = dict(cfg, value_type=vt)
    g, _, _, _ = _run_both(cfg, batches, wms, f"wrap general {name} {vt}", device=device, expected_entries=20_000)
    _covered(name, _report(f"general {vt} {'device' if device else 'host'} push", name, g))


# ---------------------------------------------------------------- dense single pass
@pytest.mark.parametrize("device", [False, True], ids=["host-push", "async-device-push"])
@pytest.mark.parametrize("name", ["dense-tumbling-top-cold", "dense-tumbling-top-warm", "dense-tumbling-top-near"])
def test_gpu_wrap_dense_single_pass(name, device):
    # dense tumbling regions (expected_entries >= 65536).  While the watermark is Long.MIN_VALUE, or within
    # 2^(log_s - 1) sizes of it, a batch has no compact base at all and takes the classify / scan / scatter sequence with
    # wide records; with a base, the records at the top of the range have no window delta from it (their windows lie
    # 2^63 / size windows above the watermark's) and the single pass is redone.  Once the watermark is near the top, a
    # narrow batch runs there: the wrapped windows are late by then and classify drops their records.
    cfg, batches, wms = T.wrap_case(name)
    gpu = _gpu_op(cfg, max_batch=1 << 15)
    ref = orc.WindowOperatorOracle(**cfg)
    deltas = []
    for (k, t, v), wm in zip(batches, wms):
        before = gpu.stats()
        if device:
            import torch
            gpu.process(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (k, t, v)))
        else:
            gpu.process(k, t, v)
        after = gpu.stats()
        deltas.append({f: after[f] - before[f] for f in ("single_pass_batches", "single_pass_redone",
                                                         "narrow_pass_batches", "narrow_pass_redone")})
        ref.process(k, t, v)
        gpu.watermark(wm)
        ref.watermark(wm)
    g = gpu.rows()
    assert_rows_equal(g, ref.rows())
    assert gpu.late_dropped == ref.late_dropped
    gpu.close()
    # the deltas of every batch, exactly (single_pass_batches, single_pass_redone, narrow_pass_batches,
    # narrow_pass_redone; a narrow pass is a single pass, and one redone for a record it cannot take, not for a record
    # without a narrow form, counts under single_pass_redone):
    none, redone, kept = (0, 0, 0, 0), (1, 1, 1, 0), (1, 0, 1, 0)
    want = {
        # no watermark: no compact base, so the single pass is not tried and the batch takes classify / scan / scatter
        T.COLD: [none] * 6,
        # Long.MIN_VALUE + 2 sizes: still no base.  0: a base, but the records at the top have no window delta from it.
        # MAX - 3 sizes, MAX - size, MAX - 1: deltas fit, but every batch holds records of [MAX - 999, Long.MIN_VALUE),
        # which lie at or above their window's end: redone, so that the classify pass notes them (above_window)
        T.WARM: [none, none, redone, redone, redone, redone],
        # MAX - 1.5 sizes from the first batch on: batches 2 to 5 hold only records below MAX - size and are kept as
        # narrow passes; the last batch brings the records of [MAX - 999, Long.MIN_VALUE) under MAX - 1 and is redone
        T.NEAR: [none, kept, kept, kept, kept, redone],
    }[T.WRAP_CASES[name]["schedule"]]
    got = [(d["single_pass_batches"], d["single_pass_redone"], d["narrow_pass_batches"], d["narrow_pass_redone"])
           for d in deltas]
    print("WRAP_EDGES_DENSE", name, device, got)
    assert got == want, (got, want)
    _covered(name, _report(f"dense single pass {'device' if device else 'host'}", name, g))


# ---------------------------------------------------------------- panes and the combiner: the refusal
def _pane_refuses(cfg, t):
    """the refusal of sliding windows kept as panes: the newest window's end wraps, or ts - offset + slide does, or ts
    lies within size + 2 slide of Long.MIN_VALUE"""
    last = W.window_start(t, cfg.get("offset", 0), cfg["slide"])
    return (W.wrap64(last + cfg["size"]) < last or t - cfg.get("offset", 0) + cfg["slide"] > MAX
            or t < MIN + cfg["size"] + 2 * cfg["slide"])


def _kept(cfg, batches):
    out = []
    for k, t, v in batches:
        # (and not displaced: all but the grid points of a bottom stream, which panes refuse with FW_ERR_DISPLACED)
        m = np.array([not _pane_refuses(cfg, x) and not W.is_displaced(x, cfg.get("offset", 0), cfg["slide"])
                      for x in t.tolist()], dtype=bool)
        out.append((k[m], t[m], v[m]))
    return out


@pytest.mark.parametrize("name", _names("panes-3000-1000", "panes-3000-500"))
def test_gpu_wrap_panes_refuse(name):
    # host columns: the push is refused whole under any watermark -- error code, nothing taken: no state entry, no record
    # counted, no late drop, no pending row -- and the operator goes on with the stream's other records exactly
    cfg, batches, wms = T.wrap_case(name)
    kept = _kept(cfg, batches)
    gpu, ref = _gpu_op(cfg), orc.WindowOperatorOracle(**cfg)
    refused = 0
    for (k, t, v), (kk, kt, kv), wm in zip(batches, kept, wms):
        if len(kk) < len(k):
            before = gpu.stats()
            with pytest.raises(N.NativeError, match="kept as panes") as e:
                gpu.process(k, t, v)
            assert e.value.code == N.FW_ERR_TIME_RANGE
            after = gpu.stats()
            assert all(after[f] == before[f] for f in ("records_in", "keyed_state_entries", "late_records_dropped",
                                                       "pending_rows"))
            refused += 1
        gpu.process(kk, kt, kv)
        ref.process(kk, kt, kv)
        gpu.watermark(wm)
        ref.watermark(wm)
    assert refused == len(batches)  # (every batch is spread over the whole range)
    g = gpu.rows()
    assert_rows_equal(g, ref.rows())
    assert gpu.late_dropped == ref.late_dropped
    gpu.close()
    c = _report("panes (refused records left out)", name, g)
    # (3000 / 500 at the top: the stream spans four slides, every record of it has a window whose end wraps)
    least = 50 if T.WRAP_CASES[name]["end"] == "bottom" else 500 if cfg["slide"] == 1000 else 0
    assert c["rows"] >= least and c["wrapped"] == 0


def test_gpu_wrap_panes_refuse_device_columns():
    # device columns are not read by the host: classify leaves the refused records out, the others are taken, and the
    # call that settles the push returns the code; the operator goes on
    import torch
    name = "panes-3000-1000-top-warm"
    cfg, batches, wms = T.wrap_case(name)
    kept = _kept(cfg, batches)
    gpu, ref = _gpu_op(cfg), orc.WindowOperatorOracle(**cfg)
    for (k, t, v), (kk, kt, kv), wm in zip(batches, kept, wms):
        with pytest.raises(N.NativeError, match=f"{len(k) - len(kk)} record") as e:
            gpu.process(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (k, t, v)))
        assert e.value.code == N.FW_ERR_TIME_RANGE
        ref.process(kk, kt, kv)
        gpu.watermark(wm)
        ref.watermark(wm)
    g = gpu.rows()
    assert_rows_equal(g, ref.rows())
    assert gpu.late_dropped == ref.late_dropped
    gpu.close()
    _report("panes device columns", name, g)


@pytest.mark.parametrize("both", [False, True], ids=["first-refused", "both-refused"])
def test_gpu_wrap_panes_refuse_pipelined_device_pushes(both):
    # two device pushes back to back, nothing settled between them: the second one's batch-only kernels are queued
    # (and may run) before the first is settled.  The refused records of both are counted -- the device only ever adds
    # to the count --, the error is returned once, by the call that settles, after both pushes' other records were
    # taken, and the operator goes on exactly
    import torch
    name = "panes-3000-1000-top-cold"
    cfg, batches, _ = T.wrap_case(name)
    kept = _kept(cfg, batches)
    gpu, ref = _gpu_op(cfg), orc.WindowOperatorOracle(**cfg)
    dev = lambda b: tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in b)  # noqa: E731
    first, second = batches[1], (batches[2] if both else kept[2])
    want = (len(batches[1][0]) - len(kept[1][0])) + (len(batches[2][0]) - len(kept[2][0]) if both else 0)
    assert len(kept[1][0]) >= 100 and len(kept[2][0]) >= 100 and want >= 100
    a, b = dev(first), dev(second)
    gpu.process_batch(*a)
    gpu.process_batch(*b)
    with pytest.raises(N.NativeError, match=f"^\\[-9\\] {want} record") as e:
        gpu.synchronize()
    assert e.value.code == N.FW_ERR_TIME_RANGE
    gpu.synchronize()  # reported once
    for kb in (kept[1], kept[2]):
        ref.process(*kb)
    assert gpu.stats()["records_in"] >= len(kept[1][0]) + len(kept[2][0])
    gpu.process(*kept[3])  # the operator goes on
    ref.process(*kept[3])
    gpu.watermark(MAX)
    ref.watermark(MAX)
    g = gpu.rows()
    assert_rows_equal(g, ref.rows())
    assert gpu.late_dropped == ref.late_dropped
    gpu.close()
    assert _report("panes device columns, pipelined", name, g)["rows"] >= 500


@pytest.mark.parametrize("name", _names("panes-3000-1000", "panes-3000-500"))
def test_gpu_wrap_no_panes_is_exact(name):
    cfg, batches, wms = T.wrap_case(name)
    g, _, _, _ = _run_both(cfg, batches, wms, f"wrap no_panes {name}", no_panes=True, expected_entries=20_000)
    _covered(name, _report("sliding size % slide == 0, no_panes", name, g))


def test_gpu_wrap_combiner_refuses():
    # the combiner is a pane operator whose watermark never moves: it refuses the same records, and combining the others
    # is exact
    import torch
    name = "panes-3000-1000-top-warm"
    cfg, batches, wms = T.wrap_case(name)
    comb = _gpu_op(cfg)
    with pytest.raises(N.NativeError) as e:
        comb.process_batch(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in batches[0]))
        comb.synchronize()
    assert e.value.code == N.FW_ERR_TIME_RANGE
    comb.close()
    g = _combine(cfg, _kept(cfg, batches), wms)
    assert _report("combine panes (refused records left out)", name, g)["rows"] >= 500
    # tumbling windows: the receiver counts a late partial's records by the window's start, which is right while a
    # window's records lie below its end; a combiner that took a record at or above its window's end (the end wrapped,
    # or the start did) refuses its extractions, and a bottom stream combines exactly
    for name in ("tumbling-o808-top-cold", "tumbling-o0-top-cold"):
        cfg, batches, _ = T.wrap_case(name)
        comb = _gpu_op(cfg)
        comb.process_batch(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in batches[0]))
        with pytest.raises(N.NativeError, match="at or above its window's end") as e:
            comb.combine_extract(1)
        assert e.value.code == N.FW_ERR_TIME_RANGE
        comb.close()
    cfg, batches, wms = T.wrap_case("tumbling-o999-bottom-warm")
    _covered("tumbling-o999-bottom-warm", _report("combine tumbling", "tumbling-o999-bottom-warm", _combine(cfg, batches, wms)))


# ---------------------------------------------------------------- the runaway set
def test_gpu_wrap_runaway_timestamps_are_refused():
    # sliding 2500 / 1000: ts - Long.MIN_VALUE in [2500, 3307].  Host columns only: the whole push is refused, and the
    # operators go on (the list operator's walk is bounded by ceil(size / slide) + 1 like the aggregate's)
    from flink_amd.listwindow import GpuListWindowOperator
    from flink_amd import EventTimeTrigger
    cfg = dict(assigner="sliding", size=2500, slide=1000)
    k = np.arange(4, dtype=np.int64)
    ok = np.array([MIN + 2499, MIN + 3308, MIN + 5000, MIN + 1], dtype=np.int64)
    v = np.ones(4, dtype=np.int64)
    ref = orc.WindowOperatorOracle(**cfg)
    ref.process(k, ok, v)
    ref.watermark(MAX)
    makers = [(2500, lambda: _gpu_op(cfg, expected_entries=20_000)), (3000, lambda: _gpu_op(dict(cfg, size=3000))),
              (2500, lambda: GpuListWindowOperator(_assigner(cfg), EventTimeTrigger.create(), None, value_type="long"))]
    for size, mk in makers:  # (size 3000: kept as panes, which refuse the whole bottom range)
        gpu = mk()
        for d in (size, size + 807):
            assert W.is_runaway(MIN + d, size, 1000) and not W.is_runaway(MIN + d + 1 if d > size else MIN + d - 1, size, 1000)
            bad = ok.copy()
            bad[2] = MIN + d
            with pytest.raises(N.NativeError) as e:
                gpu.process(k, bad, v)
            assert e.value.code == N.FW_ERR_TIME_RANGE
        if size == 2500:
            gpu.process(k, ok, v)
            gpu.watermark(MAX)
            f = ("key", "start", "end", "count", "sum")
            assert sorted(zip(*(gpu.rows()[x].tolist() for x in f))) == sorted(zip(*(ref.rows()[x].tolist() for x in f)))
        gpu.close()
    # host-column Table rows are refused whole as well
    from flink_amd.operator import GpuWindowOperator
    gpu = GpuWindowOperator(_assigner(cfg), RowAggregate(("long", "int"), tuple(ROW_SPECS)), max_batch=1 << 13)
    bad = ok.copy()
    bad[2] = MIN + 2500
    with pytest.raises(N.NativeError) as e:
        gpu.process_row_batch(k, bad, [v, v], None)
    assert e.value.code == N.FW_ERR_TIME_RANGE and gpu.stats()["records_in"] == 0
    gpu.process_row_batch(k, ok, [v, v], None)
    assert gpu.stats()["records_in"] == 4
    gpu.close()


# ---------------------------------------------------------------- sessions
@pytest.mark.parametrize("name", _names("session", "session-late-side"))
def test_gpu_wrap_sessions_aggregate(name):
    # several records per key.  A session [ts, ts + gap) that wraps takes the ordered path (TimeWindow.intersects does
    # not hold between it and its neighbours by start), and two equal wrapped windows share one state
    cfg, batches, wms = T.wrap_case(name)
    g, st, _, _ = _run_both(cfg, batches, wms, f"wrap sessions {name}")
    c = _report("sessions (aggregate)", name, g)
    _covered(name, c)
    if T.WRAP_CASES[name]["end"] == "top" and T.WRAP_CASES[name]["schedule"] == T.COLD:
        w = g[g["end"] < g["start"]]
        assert (w["count"] >= 2).sum() >= 10 and st["slow_path_records"] >= 1000


def _run_list(name, cfg, batches, wms, interval=0, evict=0, path="list"):
    from flink_amd import CountEvictor, EventTimeTrigger, PurgingTrigger
    from flink_amd.listwindow import GpuListWindowOperator
    from tests.test_gpu_list import _assert_same
    gpu, ref = _list_pair(cfg, interval, evict)
    if cfg.get("purging"):  # (_list_pair's operator takes no PurgingTrigger)
        gpu.close()
        gpu = GpuListWindowOperator(_assigner(cfg), PurgingTrigger.of(EventTimeTrigger.create()),
                                    CountEvictor.of(evict, False) if evict else None,
                                    allowed_lateness=cfg.get("lateness", 0), value_type="long")
    for (k, t, v), wm in zip(batches, wms):
        gpu.process(k, t, v)
        ref.process(k, t, v)
        gpu.watermark(wm)
        ref.watermark(wm)
    _assert_same(gpu, ref)
    assert gpu.late_dropped == ref.late_dropped
    g = gpu.rows()
    gpu.close()
    return _report(path, name, g)


@pytest.mark.parametrize("name", _names("session"))
def test_gpu_wrap_sessions_list(name):
    cfg, batches, wms = T.wrap_case(name)
    _covered(name, _run_list(name, cfg, batches, wms, path="sessions (list)"))


# ---------------------------------------------------------------- the list operator
LIST = ([(n, 0, 0) for n in _names("tumbling-o808", "sliding-2500-o308")]
        + [(n, 0, 3) for n in ("tumbling-o0-top-warm", "sliding-2500-o0-top-warm", "sliding-2500-o808-bottom-warm")]
        + [(n, 0, 0) for n in ("tumbling-late-purge-side-top-warm", "sliding-late-purge-side-top-warm",
                               "tumbling-late-max-top-warm", "sliding-late-purge-side-bottom-warm")]
        + [("continuous-tumbling-top-cold", 33, 0), ("continuous-tumbling-bottom-warm", 33, 0)])


@pytest.mark.parametrize("name,interval,evict", LIST, ids=[f"{n}{'-evictor' if e else ''}" for n, _, e in LIST])
def test_gpu_wrap_list_operator(name, interval, evict):
    # window contents, with CountEvictor, with purging and lateness, and the two vetted ContinuousEventTimeTrigger streams
    # (a first timer ts - ts % interval + interval that wraps starts its chain at the bottom of the range, where the
    # wrapped window's cleanup timer follows after six steps)
    cfg, batches, wms = T.wrap_case(name)
    assert interval == T.WRAP_CASES[name].get("interval", 0)
    if cfg.get("side_output"):
        cfg = {k: v for k, v in cfg.items() if k != "side_output"}
    c = _run_list(name, cfg, batches, wms, interval, evict, path=f"list{' continuous' if interval else ''}")
    if not interval:
        _covered(name, c)


# ---------------------------------------------------------------- other aggregates (they share classify, scatter, replay)
@pytest.mark.parametrize("name,extra", [("tumbling-o808-top-warm", dict(first=True)), ("sliding-2500-o308-top-warm", dict(first=True)),
                                        ("tumbling-o0-top-cold", dict(by="min")), ("sliding-2500-o0-top-warm", dict(by="max")),
                                        ("sliding-2500-o808-bottom-warm", dict(by="min"))],
                         ids=["first-tumbling", "first-sliding", "minby-tumbling", "maxby-sliding", "minby-sliding-bottom"])
def test_gpu_wrap_first_element_and_extremal(name, extra):
    cfg, batches, wms = T.wrap_case(name)
    cfg = dict(cfg, **extra)
    if cfg.get("by"):
        batches = [(k, t, v % 5) for k, t, v in batches]  # ties: broken by arrival order
    g, _, _, _ = _run_both(cfg, batches, wms, f"wrap {extra} {name}", expected_entries=20_000)
    _covered(name, _report("first" if extra.get("first") else extra["by"] + "By", name, g))


@pytest.mark.parametrize("name", ["tumbling-o808-top-warm", "sliding-2500-o308-top-warm", "sliding-2500-o0-bottom-cold"])
def test_gpu_wrap_hll(name):
    from flink_amd.operator import GpuWindowOperator
    cfg, batches, wms = T.wrap_case(name)
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
    _covered(name, _report("HyperLogLog", name, g))


@pytest.mark.parametrize("name", ["tumbling-o808-top-warm", "tumbling-late-top-warm", "sliding-late-purge-side-bottom-warm",
                                  "sliding-2500-o0-bottom-warm", "sliding-700-1000-bottom-warm"])
def test_gpu_wrap_tdigest(name):
    cfg, batches, wms = T.wrap_case(name)
    cfg = {k: v for k, v in cfg.items() if k != "side_output"}
    batches = [(k, t, dyadic(k, v, "f64")) for k, t, v in batches]
    g = _run_tdigest(cfg, batches, wms, expected_entries=30_000)
    _covered(name, _report("t-digest", name, g))


@pytest.mark.parametrize("lateness", [0, 500])
def test_gpu_wrap_tdigest_sliding_refuses(lateness):
    # the t-digest takes a record's windows that are not late as its newest ones, which a wrapped newest end breaks: a
    # sliding record with several windows of which one's end wraps is refused (host columns: the whole push), with and
    # without allowed lateness; bottom streams, tumbling windows and 700 / 1000 (one window) are taken, above
    from flink_amd import TDigest
    from flink_amd.operator import GpuWindowOperator
    cfg, batches, _ = T.wrap_case("sliding-2500-o0-top-cold")
    gpu = GpuWindowOperator(_assigner(cfg), TDigest(40, (0.5,)), allowed_lateness=lateness, expected_entries=30_000)
    k, t, v = batches[0]
    before = gpu.stats()
    with pytest.raises(N.NativeError) as e:
        gpu.process(k, t, dyadic(k, v, "f64"))
    assert e.value.code == N.FW_ERR_TIME_RANGE
    after = gpu.stats()
    assert all(after[f] == before[f] for f in ("records_in", "keyed_state_entries", "late_records_dropped"))
    gpu.close()


@pytest.mark.parametrize("name", ["tumbling-o808-top-warm", "sliding-2500-o308-top-warm"])
def test_gpu_wrap_table_rows(name):
    from flink_amd.operator import GpuWindowOperator
    cfg, batches, wms = T.wrap_case(name)
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
    _covered(name, _report("Table rows", name, g))


# ---------------------------------------------------------------- state handoff
@pytest.mark.parametrize("name", ["tumbling-o808-top-warm", "sliding-2500-o308-top-warm"])
def test_gpu_wrap_snapshot_restore_continue(name):
    # the cut falls before the first warm watermark: the snapshot holds wrapped windows, which that watermark makes late
    # in the restored operators, and windows that end at Long.MIN_VALUE, which stay to the end
    from flink_amd.keygroups import (assign_to_key_group, compute_key_group_range_for_operator_index, long_hash_code)
    cfg, batches, wms = T.wrap_case(name)
    ref = orc.WindowOperatorOracle(**cfg)
    for (k, t, v), wm in zip(batches, wms):
        ref.process(k, t, v)
        ref.watermark(wm)
    a = _gpu_op(cfg, max_parallelism=128, expected_entries=20_000)
    a.process(*batches[0])
    snap = a.snapshot_state()
    live = np.concatenate([r for r in snap.values() if len(r)])
    assert (live["end"] < live["start"]).sum() >= 200 and (live["end"] == MIN).sum() >= 100
    a.close()
    parts = []
    for idx in range(2):
        kgr = compute_key_group_range_for_operator_index(128, 2, idx)
        op = _gpu_op(cfg, max_parallelism=128, key_group_range=kgr, expected_entries=20_000)
        op.initialize_state(snap)
        parts.append((kgr, op))
    for _, op in parts:
        op.watermark(wms[0])
    for (k, t, v), wm in zip(batches[1:], wms[1:]):
        kg = np.array([assign_to_key_group(long_hash_code(int(x)), 128) for x in k], dtype=np.int64)
        for kgr, op in parts:
            m = (kg >= kgr.start_key_group) & (kg <= kgr.end_key_group)
            op.process(k[m], t[m], v[m])
            op.watermark(wm)
    got = []
    for _, op in parts:
        got.append(op.rows())
        op.close()
    g = np.concatenate(got)
    assert_rows_equal(g, ref.rows())
    _covered(name, _report("snapshot / restore / continue", name, g))


def test_gpu_wrap_heap_format_round_trip():
    # state rows of wrapped windows, and of a window that ends at Long.MIN_VALUE, through the heap backend's key-group
    # section format (TimeWindowSerializer's two longs, the state table's order by TimeWindow.hashCode of start + end,
    # which wraps) and back into a fresh operator, which fires them as the oracle does
    from flink_amd import heapstate as H
    from flink_amd.keygroups import string_hash_code
    from flink_amd.operator import STATE_DTYPE, GpuWindowOperator
    from flink_amd.windowing import FirstElementReduce
    n = 4000
    k = np.arange(n, dtype=np.int64) % 50
    v = (np.arange(n, dtype=np.int64) * 7919) % 1000 - 500
    names = [f"key{i}" for i in range(50)]
    ids = {s: i for i, s in enumerate(names)}
    kh = np.array([string_hash_code(names[i]) for i in k], dtype=np.int32)
    for cfg in (dict(assigner="tumbling", size=1000, offset=808), dict(assigner="tumbling", size=1000, offset=1)):
        t = np.array([MAX - 2999 + (i * 2999) // (n - 1) for i in range(n)], dtype=np.int64)
        mk = lambda: GpuWindowOperator(_assigner(cfg), FirstElementReduce("int"), key_type="hashed", max_parallelism=1)  # noqa: E731
        a = mk()
        a.process(k, t, v, key_hash=kh)
        # (offset 808: [MAX - 999, Long.MIN_VALUE) outlives every watermark but the last; offset 1: the wrapped window
        # [MAX - 806, MIN + 193) fires at any watermark, so the cut comes before the first)
        cut = MAX - 2500 if cfg["offset"] == 808 else MIN
        a.watermark(cut)
        first = a.rows()
        rows = a.snapshot_key_group(0)
        a.close()
        assert (rows["end"] < rows["start"]).sum() >= 50
        assert ((rows["end"] == MIN).sum() >= 50) == (cfg["offset"] == 808)
        passthrough = {int(r["max"]): (names[int(r["key"])], 0) for r in rows}
        mappings = H.heap_from_reduce_rows(rows, names.__getitem__, passthrough, 1)
        timers = set(H.rows_to_timers(rows, names.__getitem__))
        ser = {"window-contents": (H.TimeWindowSer(), H.StringSer(), H.TupleSer(H.StringSer(), H.IntSer()))}
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
        b.watermark(MAX)
        g = np.concatenate([first, b.rows()])
        b.close()
        ref = orc.WindowOperatorOracle(**cfg, first=True, value_type="i32")
        ref.process(k, t, v)
        ref.watermark(cut)
        ref.watermark(MAX)
        r = ref.rows()
        key = lambda x: sorted(zip(x["key"].tolist(), x["start"].tolist(), x["end"].tolist(), x["sum"].tolist()))  # noqa: E731
        assert key(g) == key(r)
        print(f"WRAP_EDGES | heap-format round trip | offset {cfg['offset']} | {len(g)} | {int((g['end'] < g['start']).sum())} | "
              f"{int((g['end'] == MIN).sum())} | {int((g['end'] < 0).sum())} |")

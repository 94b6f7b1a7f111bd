"""Signed, special and cancelling floating-point fields on every floating-point site of the GPU operators, bit for
bit against the oracle (tests/float_edges_util.py: the palettes make every partial sum exactly representable, so
the order in which the GPU's atomics add does not show; tests/test_oracle_float_edges.py guards the inputs).
Bar: keys, windows, counts, min and max as bits (canonical NaN), sums as bits including the sign of a zero, a NaN
sum matching any NaN.  Each test prints the rows it compared and how many carried each special class.

Recorded on an MI355X, summed over the Double / Float and dyadic / specials cases of each path (rows compared; rows
whose sum is negative, zero with two or more elements, NaN, +Inf, -Inf, a nonzero subnormal, DBL_MAX / FLT_MAX, an
overflow to Inf; rows with min = -0.0 and max = +0.0; reduce-aggregate rows whose sum is -0.0):

    path                           rows      neg     zero      NaN     +Inf     -Inf     subn      MAX     ovfl    -0/+0   -0 sum
    lds+ordered                  182924    72585     9268    25126    11364      928     9594     1270     5250     8538        -
    sliding-panes                 73844    30551     3591     2854     2648      898     4570     1188      750     2810        -
    sliding-split                 62796    25973     2973     2352     2144      760     3900     1018      606     2330        -
    sessions                      69716    29243     2717     1750     2118      852     4290      942      314     1932        -
    table-growth                  34260    14326     1296      976     1000      396     2120      436      208      964        -
    dense-single-pass            560168   238484    17992     8440    13476     6316    35016     6640      776    11020        -
    hot-keys-tumbling            325920   135616    13483     9916    10026     3554    20306     4450     2256        -     5242
    hot-keys-session             425116   180481    10470     7280     9752     4106    26492     4668     1030        -     9836
    hot-keys-sliding             518184   210206    28756    25880    21694     6154    32362     8802     7532        -     4300
    reduce-tumbling              731696   290340    37072   100504    45456     3712    38376     5080    21000        -     3648
    reduce-session               278864   116972    10868     7000     8472     3408    17160     3768     1256        -     4760
    count-windows                406160   167514     9408    20036    14790     4414    20074     4400     1680        -     6616
    snapshot-restore-tumbling     50280    20383     2940     2118     2242      772     3116     1014      466     2486        -
    snapshot-restore-session      31596    12545     1729     1732     1434      392     1954      502      520     1472        -
    combiner-tumbling             16000     5848     1024     1854      996       58      996      134      812     1000        -
    combiner-sliding             116236    45906     6854     7348     5596     1228     7148     1916     2466     5952        -
    table-tumbling               105536    44332     2742     2062     2648     1108     6506     1130      376     1842        -
    table-sliding                512812   215078    16206    11522    13786     5554    31606     5968     2302    11168        -
    table-session                100256    42054     2460     1994     2474     1028     6118     1040      408     1698        -
    list-tumbling                  3108     1116      211      402      204        4      210       26      132      210        -
    list-session                  74196    31663      315      632     1180      584     4610      612        6      150        -
    list-delta-evictor             1554      167      210      228      378        0      210       26      132      210        -
    total                       4681222  1931383   182585   242006   173878    46226   276734    55030    50278    53782    34402

Every case matched the oracle on its first run with the kernels' reduce-aggregate sums starting from -0.0
(sum_zero, fw_device.hip).  With the sums starting from +0.0 bits as before, test_reduce_aggregates[*-specials-*]
(16 cases) and test_hot_key_chunk_deltas[*-specials-*] (6 cases) fail, every mismatch a window of -0.0 alone whose
sum came out +0.0 (2621 of 81480 rows in hot-keys-tumbling); no other site disagreed.  With the oracle's sums
starting from +0.0 as before, tests/test_oracle_float_edges.py::test_oracle_sign_of_a_zero_sum and
test_stream_has_every_class_and_short_windows[*-first-specials-*] fail on the CPU.  The cancelling sums (part 3) stayed within
0.99 of the bound against math.fsum (CountSumMinMax: 8565 rows) and 0.97 (Table SUM / AVG: 13189 rows)."""
import math

import numpy as np
import pytest

from flink_amd import (CountWindows, DeltaEvictor, EventTimeSessionWindows, EventTimeTrigger,
                       SlidingEventTimeWindows, TumblingEventTimeWindows)
from flink_amd.windowing import CountSumMinMax, ExtremalElementReduce, FirstElementReduce, RowAggregate
from oracle import oracle as orc
from tests import float_edges_util as fe

pytestmark = pytest.mark.gpu

_VT = {"f64": "double", "f32": "float"}
VTS = ["f64", "f32"]
PALS = ["dyadic", "specials"]
both = lambda f: pytest.mark.parametrize("vt", VTS)(pytest.mark.parametrize("palette", PALS)(f))  # noqa: E731


def _assigner(assigner, size=0, slide=0, offset=0, gap=0):
    if assigner == "tumbling":
        return TumblingEventTimeWindows.of(size, offset)
    if assigner == "sliding":
        return SlidingEventTimeWindows.of(size, slide, offset)
    return EventTimeSessionWindows.with_gap(gap)


def _gpu_op(vt, assigner, size=0, slide=0, offset=0, gap=0, lateness=0, first=False, by=None, **kw):
    from flink_amd.operator import GpuWindowOperator
    agg = (FirstElementReduce(_VT[vt], "max" if first == "max" else "sum") if first
           else ExtremalElementReduce(by, _VT[vt]) if by else CountSumMinMax(_VT[vt]))
    return GpuWindowOperator(_assigner(assigner, size, slide, offset, gap), agg, EventTimeTrigger.create(),
                             allowed_lateness=lateness, **kw)


def _report(path, rows, vt, first=False):
    print(f"FLOAT_EDGES {path} {vt} rows={len(rows)} {fe.classes(rows, vt, first)}")


def _run_both(path, cfg, spec, palette, vt, **gpu_kw):
    """host pushes of the stream into the GPU operator and the oracle; rows compared bit for bit -> GPU stats"""
    batches, wms = fe.stream(palette=palette, value_type=vt, **spec)
    gpu = _gpu_op(vt, **cfg, **gpu_kw)
    ref = orc.WindowOperatorOracle(**cfg, value_type=vt)
    for (k, t, v), wm in zip(batches, wms):
        gpu.process(k, t, v)
        ref.process(k, t, v)
        gpu.watermark(wm)
        ref.watermark(wm)
    g, r, st = gpu.rows(), ref.rows(), gpu.stats()
    assert gpu.late_dropped == ref.late_dropped
    gpu.close()
    fe.assert_rows_bit_equal(g, r)
    _report(path, g, vt, bool(cfg.get("first") or cfg.get("by")))
    return st


@both
def test_lds_and_ordered_path(palette, vt):
    # lds_acc + acc_add: jitter 1.5 s against a 0.4 s bound with lateness 0.7 s sends late elements of live windows
    # down the ordered path, the rest through the LDS pre-aggregation
    st = _run_both("lds+ordered", fe.ORDERED_CFG, fe.ORDERED, palette, vt)
    assert st["slow_path_records"] > 0


@both
@pytest.mark.parametrize("cfg", fe.PANES_CFGS, ids=["panes", "split"])
def test_panes_and_split_sliding(cfg, palette, vt):
    # k_fire_panes sums a window's panes (3000 / 1000); 2500 / 1000 is not kept as panes: every element is split
    _run_both("sliding-" + ("panes" if cfg["size"] == 3000 else "split"), cfg, fe.ORDERED, palette, vt)


@both
def test_sessions_merge(palette, vt):
    st = _run_both("sessions", fe.SESSION_CFG, fe.ORDERED, palette, vt)
    assert st["state_merges"] > 0


@both
def test_table_growth_mid_push(palette, vt):
    st = _run_both("table-growth", fe.COMBINE_CFG, fe.ORDERED, palette, vt, expected_entries=2000, max_parallelism=4,
                   sub_partitions=1)
    assert st["table_grows"] > 0


@both
@pytest.mark.parametrize("async_input", [False, True], ids=["host-push", "async-device-push"])
def test_dense_single_pass(async_input, palette, vt):
    # dt_add / dt_merge: dense tumbling windows take the single-pass scatter into the compact table; a record whose
    # window is too far ahead for a compact word (batch 2) sends that batch through the wide records
    batches, wms = fe.stream(palette=palette, value_type=vt, **fe.DENSE)
    k, t, v = batches[2]
    t = t.copy()
    t[17] += 10 ** 12
    batches[2] = (k, t, v)
    gpu = _gpu_op(vt, **fe.DENSE_CFG, max_batch=1 << 14, async_input=async_input)
    ref = orc.WindowOperatorOracle(**fe.DENSE_CFG, value_type=vt)
    drained = []
    for e, ((k, t, v), wm) in enumerate(zip(batches, wms)):
        if async_input:
            import torch
            gpu.process_batch(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (k, t, v)))
            gpu.advance_watermark(wm, wait=False)
            drained.append(gpu.drain_rows(e))
        else:
            gpu.process(k, t, v)
            gpu.watermark(wm)
        ref.process(k, t, v)
        ref.watermark(wm)
    g = np.concatenate(drained) if async_input else gpu.rows()
    st = gpu.stats()
    assert gpu.late_dropped == ref.late_dropped
    gpu.close()
    fe.assert_rows_bit_equal(g, ref.rows())
    _report("dense-single-pass", g, vt)
    assert st["single_pass_batches"] > 0


@both
@pytest.mark.parametrize("cfg", fe.HOT_CFGS, ids=["tumbling", "session", "panes"])
def test_hot_key_chunk_deltas(cfg, palette, vt):
    # lds_acc_delta: Zipf keys over 2^19-record pushes split hot partitions into chunks whose deltas are merged
    _run_both("hot-keys-" + cfg["assigner"], dict(cfg, first=True), fe.HOT, palette, vt)


@both
@pytest.mark.parametrize("agg", [dict(first=True), dict(first="max"), dict(by="min"), dict(by="max")],
                         ids=["sum", "max", "minBy", "maxBy"])
@pytest.mark.parametrize("cfg", [fe.ORDERED_CFG, fe.SESSION_CFG], ids=["tumbling", "session"])
def test_reduce_aggregates(cfg, agg, palette, vt):
    # sum(pos) / max(pos) / minBy / maxBy: the sum starts from the window's first element (a window of -0.0 alone
    # sums to -0.0), the selected field follows Double.compare
    _run_both("reduce-" + cfg["assigner"], dict(cfg, **agg), fe.ORDERED, palette, vt)


@both
@pytest.mark.parametrize("size,slide,after", [(10, 5, False), (4, 2, True), (1, 1, False)], ids=["10_5", "4_2_after", "1_1"])
def test_count_windows(size, slide, after, palette, vt):
    from flink_amd.operator import GpuWindowOperator
    keys, vals = fe.count_stream(palette, vt)
    gpu = GpuWindowOperator(CountWindows.of(size, slide, after), FirstElementReduce(_VT[vt], "sum"), expected_entries=1024)
    ref = orc.CountWindowOracle(size, slide, after, value_type=vt)
    cuts = [0, 1, 17, 4096, 4097, 20_000, 20_001, 45_000, 60_000]
    for a, b in zip(cuts, cuts[1:]):
        gpu.process(keys[a:b], np.zeros(b - a, dtype=np.int64), vals[a:b])
        ref.process(keys[a:b], vals[a:b].view(np.int64))
        gpu.watermark(b)
    g, r = gpu.rows(), ref.rows()
    gpu.close()
    fe.assert_rows_bit_equal(g, r, epoch=False)
    _report("count-windows", g, vt, True)


@both
@pytest.mark.parametrize("cfg", fe.RESTORE_CFGS, ids=["tumbling", "session"])
def test_snapshot_restore(cfg, palette, vt):
    # the stream cut in half: every key group's rows into a fresh operator, which continues; one uninterrupted oracle
    batches, wms = fe.stream(palette=palette, value_type=vt, **fe.RESTORE)
    half = len(batches) // 2
    ref = orc.WindowOperatorOracle(**cfg, value_type=vt)
    for (k, t, v), wm in zip(batches, wms):
        ref.process(k, t, v)
        ref.watermark(wm)
    a = _gpu_op(vt, **cfg, max_parallelism=128)
    for (k, t, v), wm in zip(batches[:half], wms[:half]):
        a.process(k, t, v)
        a.watermark(wm)
    rows0 = a.rows()
    snap = {kg: a.snapshot_key_group(kg) for kg in range(128)}
    assert sum(len(s) for s in snap.values()) == a.num_keyed_state_entries > 0
    a.close()
    b = _gpu_op(vt, **cfg, max_parallelism=128)
    for kg, s in snap.items():
        if len(s):
            b.restore_key_group(kg, s)
    b.advance_watermark(wms[half - 1])  # the restored operator's watermark (no window is due at it)
    b.clear_pending()
    for (k, t, v), wm in zip(batches[half:], wms[half:]):
        b.process(k, t, v)
        b.watermark(wm)
    rows1 = b.rows()
    rows1["epoch"] += half - 1  # (b's first watermark was the restore's)
    b.close()
    g = np.concatenate([rows0, rows1])
    fe.assert_rows_bit_equal(g, ref.rows())
    _report("snapshot-restore-" + cfg["assigner"], g, vt)


@both
@pytest.mark.parametrize("cfg,spec", [(fe.COMBINE_CFG, fe.COMBINE), (fe.COMBINE_PANES_CFG, fe.COMBINE_PANES)],
                         ids=["tumbling", "panes"])
def test_combiner_world1(cfg, spec, palette, vt):
    # a combiner's partial accumulators (f64 min / max in sortable form) merged by the receiving operator
    import torch
    from flink_amd.operator import GpuWindowOperator
    batches, wms = fe.stream(palette=palette, value_type=vt, final=False, **spec)
    agg = CountSumMinMax(_VT[vt])
    comb = GpuWindowOperator(_assigner(**cfg), agg, device=0)
    op = GpuWindowOperator(_assigner(**cfg), agg, device=0)
    ref = orc.WindowOperatorOracle(**cfg, value_type=vt)
    rows = []
    for (k, t, v), wm in zip(batches, wms):
        comb.process_batch(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (k, t, v)))
        parts, _ = comb.combine_extract(1)
        op.push_partials(*(c.clone() for c in parts), config=parts.config)
        ref.process(k, t, v)
        rows.append(op.process_watermark(wm))
        ref.watermark(wm)
    rows.append(op.process_watermark(fe.MAX_WM))
    ref.watermark(fe.MAX_WM)
    assert op.late_dropped == ref.late_dropped > 0
    comb.close()
    op.close()
    g = np.concatenate(rows)
    fe.assert_rows_bit_equal(g, ref.rows())
    _report("combiner-" + cfg["assigner"], g, vt)


# ---------------------------------------------------------------- Table Row aggregates
T_TYPES, T_SPECS, T_CFGS = fe.TABLE_TYPES, fe.TABLE_SPECS, fe.TABLE_CFGS


def _table_run(cfg, types, specs, steps, **gpu_kw):
    from flink_amd.operator import GpuWindowOperator
    gpu = GpuWindowOperator(_assigner(**cfg), RowAggregate(tuple({**_VT, "i32": "int"}[t] for t in types),
                                                           tuple(specs)), max_batch=1 << 14, **gpu_kw)
    ref = orc.WindowOperatorOracle(**cfg, row=(types, specs))
    for k, t, cols, nulls, wm in steps:
        gpu.process_row_batch(k, t, cols, nulls)
        ref.process_rows(k, t, cols, nulls)
        gpu.watermark(wm)
        ref.watermark(wm)
    g_rows, (g_vals, g_nm), st = gpu.rows(), gpu.row_results(), gpu.stats()
    r_rows, (r_vals, r_nm) = ref.rows(), ref.row_results()
    assert st["late_records_dropped"] == ref.late_dropped
    gpu.close()
    order = lambda rows: np.lexsort((rows["count"], rows["start"], rows["key"], rows["epoch"]))  # noqa: E731
    gi, ri = order(g_rows), order(r_rows)
    assert len(gi) == len(ri) > 0
    for f in ("epoch", "key", "start", "end", "count"):
        assert np.array_equal(g_rows[f][gi], r_rows[f][ri]), f
    assert np.array_equal(g_nm[gi], r_nm[ri])
    return g_rows[gi], g_vals[gi], g_nm[gi], r_vals[ri], st


@pytest.mark.parametrize("palette", PALS)
@pytest.mark.parametrize("small_table", [False, True], ids=["sized", "grows"])
@pytest.mark.parametrize("cfg", T_CFGS, ids=["tumbling", "sliding", "sliding-split", "session"])
def test_table_row_aggregates(cfg, small_table, palette):
    # row_add / row_merge_blocks / row_value: a Double and a Float column carrying the palette, NULLs in every column;
    # a dyadic sum is exact and the average then a single division of identical operands, so COUNT, SUM, AVG, MIN and
    # MAX are all asked bit for bit (a NaN SUM / AVG matches any NaN)
    steps = fe.table_steps(fe.table_columns(palette))
    small = dict(expected_entries=2000, max_parallelism=4, sub_partitions=1) if small_table else {}
    rows, gv, nm, rv, st = _table_run(cfg, T_TYPES, T_SPECS, steps, **small)
    if small_table:
        assert st["table_grows"] > 0
    for q, (fn, c) in enumerate(T_SPECS):
        live = (nm >> q) & 1 == 0
        if fn in ("sum", "avg") and c < 2:
            fe.assert_bits_or_nan(gv[live, q], rv[live, q], f"{fn}({T_TYPES[c]})")
        else:
            bad = np.flatnonzero(gv[live, q] != rv[live, q])
            assert bad.size == 0, (fn, c, bad[:5], gv[live, q][bad[:5]], rv[live, q][bad[:5]])
    for c, vt in ((0, "f64"), (1, "f32")):
        _report(f"table-{cfg['assigner']}{cfg.get('size', '')}", fe.table_column_view(rows, gv, nm, c), vt)


# ---------------------------------------------------------------- list operator
def _list_pair(vt, assigner, size=0, gap=0, evictor=None, threshold=0.0):
    from flink_amd.listwindow import GpuListWindowOperator
    gpu = GpuListWindowOperator(_assigner(assigner, size, gap=gap), EventTimeTrigger.create(),
                                DeltaEvictor.of(threshold, False) if evictor else None, value_type=_VT[vt])
    kw = dict(gap=gap) if assigner == "session" else dict(size=size)
    ref = orc.ListWindowOracle(assigner=assigner, evictor="delta" if evictor else "none", threshold=threshold,
                               value_type=vt, **kw)
    return gpu, ref


def _list_firings(op):
    out = []
    for r, el in op.contents():
        ords = "ordinal" if "ordinal" in el.dtype.names else "ord"
        out.append(((int(r["epoch"]), int(r["key"]), int(r["start"]), int(r["end"]), int(r["count"]), int(r["first"]),
                     int(r["min"]), int(r["max"]), tuple(zip(el["ts"].tolist(), el["val"].tolist(), el[ords].tolist()))),
                    int(r["sum"])))
    out.sort()
    return out


def _list_run(path, gpu, ref, palette, vt, keys=37, span=2000):
    k, t, v = fe.list_stream(palette, vt, keys, span)
    n = len(k)
    wm = -10 ** 9
    for b in range(10):
        sl = slice(b * 2000, (b + 1) * 2000)
        gpu.process(k[sl], t[sl], v[sl])
        ref.process(k[sl], t[sl], v[sl])
        wm = max(wm, int(t[sl].max()) - 100)
        gpu.watermark(wm)
        ref.watermark(wm)
    gpu.watermark(fe.MAX_WM)
    ref.watermark(fe.MAX_WM)
    g, r = _list_firings(gpu), _list_firings(ref)
    late = ref.late_dropped
    assert gpu.late_dropped == late
    gpu.close()
    assert len(g) == len(r) > 0
    assert [x for x, _ in g] == [x for x, _ in r]  # rows (min / max as bits) and the contents of every firing
    gs, rs = np.array([s for _, s in g], dtype=np.int64), np.array([s for _, s in r], dtype=np.int64)
    fe.assert_bits_or_nan(gs, rs, "sum")
    view = np.zeros(len(g), dtype=orc.ROW_DTYPE)
    view["key"], view["count"] = [x[1] for x, _ in g], [x[4] for x, _ in g]
    view["sum"], view["min"], view["max"] = gs, [x[6] for x, _ in g], [x[7] for x, _ in g]
    _report(path, view, vt)
    return view, n - late


@both
@pytest.mark.parametrize("cfg", [dict(assigner="tumbling", size=100), dict(assigner="session", gap=30)],
                         ids=["tumbling", "session"])
def test_list_apply(cfg, palette, vt):
    # fkey / canon of fw_list.hip: apply over ListState, the rows' sum (in list order on both sides), min and max;
    # the stream shapes of tests/test_gpu_list.py (37 keys over 2 s; sessions: 400 keys over 20 s, gap 30 ms)
    gpu, ref = _list_pair(vt, **cfg)
    shape = dict(keys=400, span=20_000) if cfg["assigner"] == "session" else {}
    view, _ = _list_run("list-" + cfg["assigner"], gpu, ref, palette, vt, **shape)
    if cfg["assigner"] == "session":
        assert (view["count"] > 1).any()


@pytest.mark.parametrize("vt", VTS)
def test_list_delta_evictor_specials(vt):
    # delta_of: DeltaEvictor's last - element over the specials; Inf - Inf and NaN deltas are never evicted (the
    # comparison with the threshold is false), finite ones beyond the threshold are
    gpu, ref = _list_pair(vt, "tumbling", size=100, evictor=True, threshold=4.0)
    view, fed = _list_run("list-delta-evictor", gpu, ref, "specials", vt)
    # (tumbling, no lateness: every element that is not late is in exactly one firing unless it was evicted)
    assert np.isnan(fe.f64(view["sum"])).any() and 0 < int(view["count"].sum()) < fed


# ---------------------------------------------------------------- cancelling sums that are not exact
def _window_groups(keys, ts, wm_prev, size, live=None):
    """{(key, tumbling window start): indices of its elements} of the elements that are not late (allowed lateness
    0: a window is late when its maxTimestamp <= the watermark, WindowOperator.isWindowLate)"""
    start = ts - ts % size
    keep = start + size - 1 > wm_prev
    if live is not None:
        keep &= live
    out = {}
    for i in np.flatnonzero(keep):
        out.setdefault((int(keys[i]), int(start[i])), []).append(i)
    return out


def _check_cancelling(rows_key_start_count, s_gpu, s_ref, groups, x, avg=None):
    """|S_gpu - S_oracle| <= 2 (n - 1) 2^-53 sum|x_i|: neither side's order is pinned and each is a recursive
    summation of the window's n elements, whose error is at most (n - 1) 2^-53 sum|x_i| whatever the order; and
    against math.fsum (the exactly rounded sum) within (n - 1) 2^-53 sum|x_i|, so a wrong element cannot hide behind
    the oracle.  avg = (gpu, oracle) averages: each is one correctly rounded division of its sum by n, so they
    differ by at most the sums' bound over n plus 2^-53 (|S_gpu| + |S_oracle|) / n."""
    u = 2.0 ** -53
    worst, cancel = 0.0, 0
    for j, (key, start, cnt) in enumerate(rows_key_start_count):
        idx = groups[(key, start)]
        n = len(idx)
        assert n == cnt, (key, start, n, cnt)
        el = x[idx]
        absum, exact = math.fsum(np.abs(el).tolist()), math.fsum(el.tolist())
        b = (n - 1) * u * absum
        assert abs(s_gpu[j] - s_ref[j]) <= 2 * b, (key, start, n, s_gpu[j], s_ref[j], b)
        assert abs(s_gpu[j] - exact) <= b, (key, start, n, s_gpu[j], exact, b)
        if avg is not None:
            assert abs(avg[0][j] - avg[1][j]) <= (2 * b + u * (abs(s_gpu[j]) + abs(s_ref[j]))) / n
        if b:
            worst = max(worst, abs(s_gpu[j] - exact) / b)
        cancel += n >= 2 and abs(exact) < 1e-3 * absum
    print(f"FLOAT_EDGES cancelling rows={len(rows_key_start_count)} cancelling_windows={cancel} worst_error/bound={worst:.3g}")
    assert cancel > 0


def _wm_prev(steps_len, wms):
    return np.concatenate([np.full(n, wms[i - 1] if i else -(1 << 63), dtype=np.int64) for i, n in enumerate(steps_len)])


def test_cancelling_sums_count_sum_min_max():
    cfg = dict(assigner="tumbling", size=1000)
    batches, wms = fe.stream(palette=lambda k, v, vt: fe.cancelling(v), value_type="f64", **fe.ORDERED)
    gpu = _gpu_op("f64", **cfg)
    ref = orc.WindowOperatorOracle(**cfg, value_type="f64")
    for (k, t, v), wm in zip(batches, wms):
        gpu.process(k, t, v)
        ref.process(k, t, v)
        gpu.watermark(wm)
        ref.watermark(wm)
    g, r = gpu.rows(), ref.rows()
    gpu.close()
    order = lambda a: a[np.lexsort((a["start"], a["key"]))]  # noqa: E731 (lateness 0: one row per (key, window))
    g, r = order(g), order(r)
    for f in ("epoch", "key", "start", "end", "count", "min", "max"):
        assert np.array_equal(g[f], r[f]), f
    keys, ts, x = (np.concatenate(c) for c in zip(*batches))
    groups = _window_groups(keys, ts, _wm_prev([len(b[0]) for b in batches], wms), 1000)
    assert len(groups) == len(g)
    _check_cancelling(list(zip(g["key"].tolist(), g["start"].tolist(), g["count"].tolist())), fe.f64(g["sum"]),
                      fe.f64(r["sum"]), groups, x)
    assert (fe.f64(g["sum"]) < 0).any() and (fe.f64(g["min"]) < 0).any()


def test_cancelling_sums_table_sum_avg():
    cfg = dict(assigner="tumbling", size=1000)
    specs = [("count", 0), ("sum", 0), ("avg", 0)]
    steps = fe.table_steps(lambda k, v: [fe.cancelling(v)])
    rows, gv, nm, rv, _ = _table_run(cfg, ["f64"], specs, steps)
    live = (nm & 2) == 0  # (rows with at least one non-NULL value)
    assert np.array_equal(gv[:, 0], rv[:, 0]) and live.any()
    keys, ts, x = (np.concatenate(c) for c in zip(*((s[0], s[1], s[2][0]) for s in steps)))
    nulls = np.concatenate([s[3] for s in steps])
    groups = _window_groups(keys, ts, _wm_prev([len(s[0]) for s in steps], [s[4] for s in steps]), 1000,
                            live=(nulls & 1) == 0)
    _check_cancelling(list(zip(rows["key"][live].tolist(), rows["start"][live].tolist(), gv[live, 0].tolist())),
                      fe.f64(gv[live, 1]), fe.f64(rv[live, 1]), groups, x,
                      avg=(fe.f64(gv[live, 2]), fe.f64(rv[live, 2])))

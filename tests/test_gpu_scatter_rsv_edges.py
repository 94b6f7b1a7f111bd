"""The single-pass scatter (k_scatter_rsv) at the edges of its pipeline: persistent workgroups walk the batch in
rounds of RR records, with the next round's loads in flight while the current one is ranked, staged and reserved
and the previous one is copied out.  Every case: rows bit-exact against the oracle (f64 sums within 1e-6), the
late count equal to the oracle's, every record fired or late, and the single-pass statistics what the case means.

Partitions P = key groups << log2(sub_partitions) (fw_runtime.cpp fw_create: `c.P = c.n_kg << c.log_s`); the
launcher takes rounds of 8192 records up to 1024 partitions and of 4096 up to 2048 (launch_scatter_rsv).  The
statistics expose no region count, so the two legs are chosen by that derivation:
  rr8192: 128 key groups x 8 sub-partitions = 1024 partitions,
  rr4096: 128 key groups x 16 sub-partitions = 2048 partitions.
A compact record holds a window delta below sub_partitions, counted from sub_partitions / 2 windows before the
watermark's; an operator's first batch has no watermark to count from and goes through the offset path."""
import os
import re

import numpy as np
import pytest

from flink_amd import KeyGroupRange
from flink_amd.datagen import generate_host
from oracle import oracle as orc
from tests.parity_util import assert_rows_equal
from tests.test_gpu_parity import _VT, _gpu_op

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {"rr8192": dict(max_parallelism=128, sub_partitions=8), "rr4096": dict(max_parallelism=128, sub_partitions=16)}
SIZE = 100
LMIN = -(1 << 63)


def scatter_shape():
    """(FW_TILE, {leg: RR}) as the sources have them."""
    with open(os.path.join(ROOT, "flink_amd", "csrc", "fw_internal.h")) as f:
        tile = int(re.search(r"#define FW_TILE (\d+)", f.read()).group(1))
    with open(os.path.join(ROOT, "flink_amd", "csrc", "fw_device.hip")) as f:
        src = f.read()
    body = src[src.index("void launch_scatter_rsv("):]
    m = re.search(r"const int rr = big \? (\d+) : (\d+);", body)
    rr = {"rr8192": int(m.group(1)), "rr4096": int(m.group(2))}
    for leg, r in rr.items():
        assert f"k_scatter_rsv<{r}, true>" in body and f"k_scatter_rsv<{r}, false>" in body and tile % r == 0
    return tile, rr


FW_TILE, RR = scatter_shape()


def _values(vals, value_type):
    return (vals & 0xFFFFF).astype(np.float64) / 7.0 if value_type == "f64" else vals


def _split(keys, ts, vals, lengths, bound):
    """Batches of the given lengths, a watermark `bound` behind the largest timestamp after each, a final flush."""
    batches, wms, b, mx = [], [], 0, LMIN
    for n in lengths:
        sl = slice(b, b + n)
        batches.append((keys[sl], ts[sl], vals[sl]))
        mx = max(mx, int(ts[sl].max()))
        wms.append(mx - bound)
        b += n
    assert b == len(keys)
    batches.append((keys[:0], ts[:0], vals[:0]))
    wms.append((1 << 63) - 1)
    return batches, wms


_REF = {}


def _oracle(name, value_type, batches, wms):
    """The oracle's rows and late count of a case's stream: computed once, shared by its parametrisations."""
    if (name, value_type) not in _REF:
        ref = orc.WindowOperatorOracle(assigner="tumbling", size=SIZE, value_type=value_type)
        for (k, t, v), wm in zip(batches, wms):
            ref.process(k, t, v)
            ref.watermark(wm)
        rows = ref.rows()
        rows.setflags(write=False)
        _REF[name, value_type] = rows, ref.late_dropped
    return _REF[name, value_type]


def _gpu(batches, wms, value_type, leg, device, offset_views=False, **kw):
    import torch
    kw = dict(LEGS[leg], **kw)
    kw.setdefault("max_batch", 1 << 17)
    gpu = _gpu_op("tumbling", SIZE, value_type=value_type, async_input=device, **kw)
    drained = []
    for e, ((k, t, v), wm) in enumerate(zip(batches, wms)):
        if device:
            cols = []
            for x in (k, t, v):
                x = torch.from_numpy(np.ascontiguousarray(x))
                if offset_views and len(x):  # one element behind a 16-byte-aligned allocation: no 16-byte loads of the column
                    buf = torch.empty(len(x) + 2, dtype=x.dtype, device="cuda")
                    assert buf.data_ptr() % 16 == 0
                    buf[1:1 + len(x)].copy_(x)
                    x = buf[1:1 + len(x)]
                    assert x.data_ptr() % 16 == 8 and x.is_contiguous()
                else:
                    x = x.cuda()
                cols.append(x)
            gpu.process_batch(*cols)
            gpu.advance_watermark(wm, wait=False)
            drained.append(gpu.drain_rows(e))
        else:
            gpu.process(k, t, v)
            gpu.watermark(wm)
    rows = np.concatenate(drained) if device else gpu.rows()
    st = gpu.stats()
    gpu.close()
    return rows, st


def _check(rows, st, ref_rows, ref_late, pushed, value_type):
    assert_rows_equal(rows, ref_rows, _VT[value_type])
    assert st["late_records_dropped"] == ref_late
    assert int(rows["count"].sum()) + st["late_records_dropped"] == pushed


PUSH = pytest.mark.parametrize("device", [False, True], ids=["host-push", "async-device-push"])
VALUE = pytest.mark.parametrize("value_type", ["i64", "f64"])
LEG = pytest.mark.parametrize("leg", list(LEGS))


def _lengths(leg):
    r = RR[leg]
    return [50_000, 1, 2, 3, r - 1, r, r + 1, 2 * r + 1, FW_TILE - 1, FW_TILE, FW_TILE + 1, 3 * FW_TILE + 5]


def _length_stream(leg, value_type):
    lengths = _lengths(leg)
    k, t, v = generate_host(0x5EED, 0, sum(lengths), 50_000, ts_base=1_000_000, rate=1_000_000, jitter=0)
    return lengths, _split(k, t, _values(v, value_type), lengths, bound=20)


@PUSH
@VALUE
@LEG
def test_gpu_scatter_rsv_batch_lengths(leg, value_type, device):
    # the empty prefetched round (a workgroup's only round), the odd-length pair clamp, a last round shorter than a
    # wave, one record more or fewer than a round and than a tile
    lengths, (batches, wms) = _length_stream(leg, value_type)
    ref_rows, ref_late = _oracle("lengths-" + leg, value_type, batches, wms)
    rows, st = _gpu(batches, wms, value_type, leg, device)
    _check(rows, st, ref_rows, ref_late, sum(lengths), value_type)
    assert ref_late == 0
    # every batch behind the first took the single pass, none was redone
    assert st["single_pass_batches"] == len(lengths) - 1
    assert st["single_pass_redone"] == 0 and st["narrow_pass_redone"] == 0
    assert st["narrow_pass_batches"] == (len(lengths) - 1 if value_type == "i64" else 0)


def test_gpu_scatter_rsv_more_tiles_than_workgroups():
    # every workgroup walks several rounds and the last stride is ragged: 2 x CUs x 2 + 3 tiles and 5 records in one
    # push (all of it inside the two windows behind the watermark: 2e8 records per second of event time)
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (2 * cus * 2 + 3) * FW_TILE + 5
    lengths = [50_000, n]
    k, t, v = generate_host(0xBEEF, 0, sum(lengths), 50_000, ts_base=1_000_000, rate=200_000_000, jitter=0)
    batches, wms = _split(k, t, v, lengths, bound=0)
    ref_rows, ref_late = _oracle("tiles", "i64", batches, wms)
    rows, st = _gpu(batches, wms, "i64", "rr8192", True, max_batch=n)
    _check(rows, st, ref_rows, ref_late, sum(lengths), "i64")
    assert st["single_pass_batches"] == 1 and st["narrow_pass_batches"] == 1
    assert st["single_pass_redone"] == 0 and st["narrow_pass_redone"] == 0


@VALUE
@LEG
def test_gpu_scatter_rsv_unaligned_columns(leg, value_type):
    # device columns one element behind a 16-byte boundary, odd lengths: every load takes the clamped 8-byte path
    lengths = [50_001, FW_TILE + RR[leg] + 7, 3]
    k, t, v = generate_host(0xA11, 0, sum(lengths), 50_000, ts_base=1_000_000, rate=1_000_000, jitter=0)
    batches, wms = _split(k, t, _values(v, value_type), lengths, bound=20)
    ref_rows, ref_late = _oracle("unaligned-" + leg, value_type, batches, wms)
    rows, st = _gpu(batches, wms, value_type, leg, True, offset_views=True)
    _check(rows, st, ref_rows, ref_late, sum(lengths), value_type)
    assert st["single_pass_batches"] == 2 and st["single_pass_redone"] == 0 and st["narrow_pass_redone"] == 0


def _edge_rounds(leg, tiles):
    """Indices in the first and in the last round of the second and of the last of `tiles` tiles: the rounds that are
    prefetched while another one is processed."""
    r = RR[leg]
    last = (tiles - 1) * FW_TILE
    return np.array([FW_TILE, FW_TILE + r - 1, 2 * FW_TILE - r, 2 * FW_TILE - 1, last + 1, last + FW_TILE - 2])


@PUSH
@VALUE
@LEG
def test_gpu_scatter_rsv_late_counted_once(leg, value_type, device):
    lengths = [50_000, 3 * FW_TILE]
    k, t, v = generate_host(0x1A7E, 0, sum(lengths), 50_000, ts_base=1_000_000, rate=1_000_000, jitter=0)
    t = t.copy()
    at = lengths[0] + _edge_rounds(leg, 3)
    t[at] = 1_000_000 - 500  # (windows long fired by the first batch's watermark)
    batches, wms = _split(k, t, _values(v, value_type), lengths, bound=20)
    ref_rows, ref_late = _oracle("late-" + leg, value_type, batches, wms)
    rows, st = _gpu(batches, wms, value_type, leg, device)
    _check(rows, st, ref_rows, ref_late, sum(lengths), value_type)
    assert ref_late == len(at)  # (jitter 0: no other record is late)
    assert st["single_pass_batches"] == 1 and st["single_pass_redone"] == 0 and st["narrow_pass_redone"] == 0


@VALUE
@LEG
def test_gpu_scatter_rsv_errors_counted_once(leg, value_type):
    from flink_amd import _native as N
    # records outside the KeyGroupRange: the error names their number.  64 key groups x 16 (32) sub-partitions are
    # the 1024 (2048) partitions of the leg
    sub = 2 * LEGS[leg]["sub_partitions"]
    lengths = [50_000, 3 * FW_TILE]
    k, t, v = generate_host(0xE44, 0, 4 * sum(lengths), 50_000, ts_base=1_000_000, rate=1_000_000, jitter=0)
    kg = orc.key_groups_long(k, 128)
    inside = k[kg < 64][:sum(lengths)].copy()
    outside = k[kg >= 64]
    t, v = t[:sum(lengths)], _values(v[:sum(lengths)], value_type)
    at = lengths[0] + _edge_rounds(leg, 3)
    bad = inside.copy()
    bad[at] = outside[:len(at)]
    for keys, ts, what in ((bad, t, f"{len(at)} record\\(s\\) outside KeyGroupRange"),
                           (inside, np.where(np.isin(np.arange(len(t)), at), LMIN, t), "Long.MIN_VALUE")):
        gpu = _gpu_op("tumbling", SIZE, value_type=value_type, max_parallelism=128, sub_partitions=sub,
                      key_group_range=KeyGroupRange(0, 63), max_batch=1 << 17, async_input=False)
        n0 = lengths[0]
        gpu.process(keys[:n0], ts[:n0], v[:n0])
        gpu.watermark(int(ts[:n0].max()) - 20)
        with pytest.raises(N.NativeError, match=what):
            gpu.process(keys[n0:], ts[n0:], v[n0:])
            gpu.watermark(int(t.max()) - 20)
        gpu.close()


@PUSH
@VALUE
@LEG
def test_gpu_scatter_rsv_fallbacks_inside_pipeline(leg, value_type, device):
    # three batches the single pass cannot take, each between two it can: a record 16 windows ahead (no compact
    # form) in the last round of the batch's last tile, a key of 2^28 (no narrow form) in the batch's very last
    # record, a hot key in three quarters of the batch (its run passes rcap).  Each is redone exactly, and the batch
    # behind it finds the reservation words zeroed and takes the single pass again.
    lengths = [50_000, 4 * FW_TILE, 20_000, 2 * FW_TILE + 1, 20_000, 4 * FW_TILE, 20_000]
    k, t, v = generate_host(0xFA11, 0, sum(lengths), 50_000, ts_base=1_000_000, rate=1_000_000, jitter=0)
    starts = np.cumsum([0] + lengths)
    batches, wms = _split(k, t, _values(v, value_type), lengths, bound=20)  # (the watermarks of the plain stream)
    kk, tt, vv = (x.copy() for x in batches[1])
    tt[len(tt) - 2] += 16 * SIZE
    batches[1] = (kk, tt, vv)
    kk, tt, vv = (x.copy() for x in batches[3])
    kk[-1] = 1 << 28
    batches[3] = (kk, tt, vv)
    kk, tt, vv = (x.copy() for x in batches[5])
    kk[: len(kk) * 3 // 4] = 7
    batches[5] = (kk, tt, vv)
    assert starts[-1] == sum(lengths)
    ref_rows, ref_late = _oracle("fallbacks-" + leg, value_type, batches, wms)
    rows, st = _gpu(batches, wms, value_type, leg, device)
    _check(rows, st, ref_rows, ref_late, sum(lengths), value_type)
    assert ref_late == 0
    assert st["single_pass_batches"] == len(lengths) - 1
    if value_type == "i64":  # the wide key costs the narrow form, for good; the other two the single pass
        assert st["narrow_pass_redone"] == 1 and st["single_pass_redone"] == 2
        assert st["narrow_pass_batches"] == 3
    else:  # (a key of 2^28 is any other key in a 16-byte record)
        assert st["narrow_pass_redone"] == 0 and st["single_pass_redone"] == 2
        assert st["narrow_pass_batches"] == 0

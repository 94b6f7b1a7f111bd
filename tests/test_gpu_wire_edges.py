"""f2 on the GPU: the kernels of fw_wire.hip (through flink_amd.wire.WireCodec) against tests/wire_ref.py, the
independent byte-level restatement of the reference's serializers, on every case of tests/wire_edges_util.py (which
test_oracle_wire_edges.py runs through the oracle, so the three agree).  Every comparison is exact; the only
class-level one is a decoded Float NaN, whose widened payload is build-defined."""
import ctypes

import numpy as np
import pytest

from tests import wire_edges_util as U
from tests import wire_ref as W

pytestmark = pytest.mark.gpu

_codecs = {}


def _codec(fields, max_bytes=1 << 20):
    """One codec per layout for the whole module (decodes of different lengths through one codec are part of what is
    tested: every case must equal wire_ref whatever the codec decoded before)."""
    from flink_amd.wire import WireCodec, WireLayout
    key = (tuple(fields), max_bytes)
    if key not in _codecs:
        _codecs[key] = WireCodec(WireLayout(fields), max_bytes)
    return _codecs[key]


@pytest.fixture(scope="module", autouse=True)
def _close_codecs():
    yield
    for c in _codecs.values():
        c.close()
    _codecs.clear()


def _dev(data):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def _cols(cols):
    cols = [c.cpu().numpy() for c in cols]
    return cols[0], (cols[3] if len(cols) > 3 else None), cols[1], cols[2]


def _clean(case, ref=None, data=None, codec=None, cap=None):
    codec = codec or _codec(case.fields)
    cols, st = codec.decode(_dev(case.data if data is None else data), cap)
    k, kh, t, v = _cols(cols)
    U.assert_decoded(case, k, kh, t, v, st, ref)


def _corrupt(case, at, code, ref=None):
    from flink_amd import _native as N
    with pytest.raises(N.NativeError) as ei:
        _codec(case.fields).decode(_dev(case.data))
    e = ei.value
    assert e.code == N.FW_ERR_STATE, (case, str(e))
    if code in (-2, -4):  # a known tag whose element is not one of this layout (or a null String key)
        assert "does not match the layout" in str(e) and str(e).endswith(f"at byte {at}"), (case, str(e))
        if code == -4:
            assert "null String key" in str(e)
    else:
        assert str(e).endswith(f"Corrupt stream, found tag: {code}"), (case, str(e))
    assert e.stats["consumed"] == at, (case, e.stats)
    k, kh, t, v = _cols(e.columns)
    U.assert_decoded(case, k, kh, t, v, e.stats, ref)


def test_gpu_wire_widest_layout_and_every_entry_offset():
    from flink_amd import _native as N
    for c in U.entry_offset_cases():
        _clean(c)
    wide = _codec(U.TOO_WIDE)
    with pytest.raises(N.NativeError) as ei:
        wide.decode(_dev(U.entry_offset_cases()[0].data))
    assert ei.value.code == N.FW_ERR_ARG


@pytest.mark.parametrize("nchunks", U.LEVEL_CHUNKS)
def test_gpu_wire_level_boundaries(nchunks):
    for exact in (False, True):
        c = U.level_case(nchunks, exact)
        _clean(c, codec=_codec(U.F3, 4097 * U.WCH))
        _clean(c, codec=_codec(U.F3, len(c.data)))  # a codec whose tree is exactly this stream's


def test_gpu_wire_codec_reused_for_shorter_streams():
    from flink_amd.wire import WireCodec, WireLayout
    one = WireCodec(WireLayout(U.F3), 4097 * U.WCH)
    for c in U.reuse_sequence():
        _clean(c, codec=one)
        fresh = WireCodec(WireLayout(U.F3), 4097 * U.WCH)
        _clean(c, codec=fresh)
        fresh.close()
    one.close()


def test_gpu_wire_range_ends():
    for c in U.range_end_cases():
        _clean(c)


def test_gpu_wire_float_and_double_value_fields():
    for c in U.float_cases():
        _clean(c)


def test_gpu_wire_every_integer_kind_at_both_ends():
    for c in U.integer_cases():
        _clean(c)


def test_gpu_wire_capacity():
    from flink_amd import _native as N
    c = U.capacity_case()
    n = c.ref.stats["records"]
    _clean(c, cap=n)
    with pytest.raises(N.NativeError) as ei:
        _codec(c.fields).decode(_dev(c.data), n - 1)
    assert ei.value.code == N.FW_ERR_STATE and "capacity" in str(ei.value)


@pytest.mark.parametrize("placement", U.PLACEMENTS)
@pytest.mark.parametrize("kind", list(U.corrupt_kinds()))
def test_gpu_wire_corrupt_elements(kind, placement):
    c, at, code = U.corrupt_cases()[(kind, placement)]
    _corrupt(c, at, code)


def test_gpu_wire_partial_tails():
    for c in U.partial_tail_cases():
        _clean(c)


@pytest.mark.parametrize("which", ["S2", "S4"])
def test_gpu_wire_string_layouts_and_every_cut(which):
    c = U.string_stream(which)
    _clean(c)
    for end in range(len(c.data) + 1):
        _clean(c, W.decode(c.data[:end], c.fields), c.data[:end])


def test_gpu_wire_string_cuts_around_a_chunk_boundary():
    c = U.string_boundary_stream()
    for end in U.string_boundary_cuts():
        _clean(c, W.decode(c.data[:end], c.fields), c.data[:end])


def test_gpu_wire_string_size_limit():
    for c, at in U.string_size_limit_cases():
        if at is None:
            _clean(c)
        else:
            _corrupt(c, at, -2)


def test_gpu_wire_corrupt_string_records():
    for c, at, code in U.string_corrupt_cases():
        if at is None:
            _clean(c)
        else:
            _corrupt(c, at, code)


def _device_rows(rows):
    import torch
    t = {f: torch.from_numpy(np.ascontiguousarray(rows[f])).cuda() for f in W.ROW_FIELDS}
    return t, {f: t[f].data_ptr() for f in W.ROW_FIELDS}


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("layout", range(7))
def test_gpu_wire_encode_every_kind_and_role(layout, f64):
    fields = U.encode_layouts()[layout]
    rows = U.encode_rows(f64)
    keep, view = _device_rows(rows)
    got = _codec(fields).encode(view, U.ENC_ROWS, f64).cpu().numpy().tobytes()
    want = W.encode(rows, fields, f64)
    size = len(want) // U.ENC_ROWS
    for r in range(U.ENC_ROWS):  # (row by row, so that a failure names the row)
        assert got[r * size:(r + 1) * size] == want[r * size:(r + 1) * size], (r, {f: hex(int(rows[f][r]) & (1 << 64) - 1) for f in rows})
    assert got == want


@pytest.mark.parametrize("f64", [False, True])
def test_gpu_wire_encode_sizes_and_refusals(f64):
    import torch
    from flink_amd import _native as N
    fields = U.encode_layouts()[2]
    codec = _codec(fields)
    for n in U.ENC_SIZES:
        rows = U.rows_slice(U.encode_rows(f64), n)
        keep, view = _device_rows(rows)
        assert codec.encode(view, n, f64).cpu().numpy().tobytes() == W.encode(rows, fields, f64)
    # an output one byte too small: refused, nothing written
    keep, view = _device_rows(U.encode_rows(f64))
    size = 13 + sum(W.SIZE[k] for k, _ in fields)
    out = torch.zeros(U.ENC_ROWS * size, dtype=torch.uint8, device="cuda")
    written = ctypes.c_int64(99)
    rc = N.lib().fw_wire_encode_device(codec._h, ctypes.byref(N.FwRows(**view)), U.ENC_ROWS, int(f64), out.data_ptr(),
                                       U.ENC_ROWS * size - 1, ctypes.byref(written))
    assert rc == N.FW_ERR_STATE and written.value == 0 and not bool(out.any().item())
    # a decode layout is no output layout
    for bad in ([("long", "key"), ("long", "value")], U.S2):
        with pytest.raises(N.NativeError) as ei:
            _codec(bad).encode(view, U.ENC_ROWS, f64)
        assert ei.value.code == N.FW_ERR_ARG

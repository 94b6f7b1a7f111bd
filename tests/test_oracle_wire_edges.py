"""f2 on the CPU: oracle/wire_oracle.cpp against tests/wire_ref.py, the independent byte-level restatement written
from the reference's sources, on every case of tests/wire_edges_util.py -- byte for byte and column for column.  This
vets the oracle before test_gpu_wire_edges.py looks at a kernel, and asserts the registry's coverage conditions (all
64 entry offsets, exit offset 63, the four level vectors, every corrupt kind at every placement, every kind x role
on encode).  The only class-level comparison is a decoded Float NaN (its widened payload is build-defined)."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as orc
from tests import wire_edges_util as U
from tests import wire_ref as W


def _decode(case, data=None, cap=None):
    data = case.data if data is None else data
    cap = len(data) // 5 + 1 if cap is None else cap
    (k, kh, t, v), st, rc = orc.wire_decode_keyed(data, case.fields, cap=cap)
    return (k, kh, t, v), st, rc


def _clean(case, ref=None, data=None):
    (k, kh, t, v), st, rc = _decode(case, data)
    assert rc == 0, (case, rc, st)
    U.assert_decoded(case, k, kh, t, v, st, ref)


def _corrupt(case, at, code, ref=None):
    (k, kh, t, v), st, rc = _decode(case)
    assert (rc, st["bad_tag"], st["consumed"]) == (-1, code, at), (case, rc, st)
    U.assert_decoded(case, k, kh, t, v, st, ref)


def test_registry_reaches_its_edges():
    U.assert_coverage()


def test_entry_offsets_and_widest_element():
    for c in U.entry_offset_cases():
        _clean(c)


@pytest.mark.parametrize("nchunks", U.LEVEL_CHUNKS)
def test_level_boundaries(nchunks):
    for exact in (False, True):
        _clean(U.level_case(nchunks, exact))


def test_range_ends():
    cases = {c.name: c for c in U.range_end_cases()}
    for c in cases.values():
        _clean(c)
    # (the reference values themselves, so that a shared slip in building the cases cannot hide)
    assert list(cases["ts_ends"].ref.ts) == [U.LONG_MAX, U.LONG_MIN, -1, 0, U.LONG_MIN]
    assert cases["wm_max"].ref.stats["watermark"] == U.LONG_MAX
    for name in ("wm_min_same_chunk", "wm_min_three_chunks_later", "wm_min_only", "wm_min_then_more_chunks", "wm_after_mixed"):
        assert cases[name].ref.stats["watermark"] == U.LONG_MIN and cases[name].ref.stats["watermarks"] >= 1
    assert cases["status_last_-2147483648"].ref.stats["status"] == U.INT_MIN


def test_float_and_double_value_fields():
    for c in U.float_cases():
        _clean(c)


def test_every_integer_kind_at_both_ends():
    for c in U.integer_cases():
        _clean(c)
    byname = {c.name: c for c in U.integer_cases()}
    assert list(byname["int_short_key"].ref.key) == [-32768, 32767, -1, 0]
    assert list(byname["int_byte_value"].ref.val) == [-128, 127, -1, 0]
    assert list(byname["boolean_bytes"].ref.val) == [0, 1, 1, 1, 1]


def test_capacity():
    c = U.capacity_case()
    n = c.ref.stats["records"]
    (k, kh, t, v), st, rc = _decode(c, cap=n)
    assert rc == 0
    U.assert_decoded(c, k, kh, t, v, st)
    assert _decode(c, cap=n - 1)[2] == -2


@pytest.mark.parametrize("placement", U.PLACEMENTS)
@pytest.mark.parametrize("kind", list(U.corrupt_kinds()))
def test_corrupt_elements(kind, placement):
    c, at, code = U.corrupt_cases()[(kind, placement)]
    _corrupt(c, at, code)


def test_partial_tails():
    for c in U.partial_tail_cases():
        _clean(c)


@pytest.mark.parametrize("which", ["S2", "S4"])
def test_string_layouts_and_every_cut(which):
    c = U.string_stream(which)
    _clean(c)
    for end in range(len(c.data) + 1):
        _clean(c, W.decode(c.data[:end], c.fields), c.data[:end])


def test_string_cuts_around_a_chunk_boundary():
    c = U.string_boundary_stream()
    for end in U.string_boundary_cuts():
        _clean(c, W.decode(c.data[:end], c.fields), c.data[:end])


def test_string_size_limit_is_this_builds_not_the_references():
    # the oracle restates the reference, which reads a String record of any length: it equals wire_ref without the limit
    for c, at in U.string_size_limit_cases():
        _clean(c, W.decode(c.data, c.fields, string_limit=None))


def test_corrupt_string_records():
    for c, at, code in U.string_corrupt_cases():
        if at is None:
            _clean(c)
        else:
            _corrupt(c, at, code)


def _rows_array(rows):
    a = np.zeros(len(rows["key"]), dtype=orc.ROW_DTYPE)
    for f in W.ROW_FIELDS:
        a[f] = rows[f]
    return a


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("layout", range(7))
def test_encode_every_kind_and_role(layout, f64):
    fields = U.encode_layouts()[layout]
    rows = U.encode_rows(f64)
    got, want = orc.wire_encode(_rows_array(rows), fields, f64), W.encode(rows, fields, f64)
    size = len(want) // U.ENC_ROWS
    for r in range(U.ENC_ROWS):  # (row by row, so that a failure names the row)
        assert got[r * size:(r + 1) * size] == want[r * size:(r + 1) * size], (r, {f: hex(int(rows[f][r]) & (1 << 64) - 1) for f in rows})
    assert got == want


def test_encode_known_bytes():
    # wire_ref's own encode, by hand: canonical NaNs, (long) d, ties to even, end - 1 at both ends
    rows = {f: np.zeros(4, dtype=np.int64) for f in W.ROW_FIELDS}
    rows["end"][:] = [3000, U.LONG_MAX, U.LONG_MIN, 0]
    rows["sum"][:] = [W._signed(x, 64) for x in (0xfff8000000000000, 0x7ff0000000000001, W.bits_from_double(1 + 2.0 ** -24),
                                                 W.bits_from_double(-1e300))]
    b = W.encode(rows, [("double", "sum"), ("float", "sum"), ("long", "sum"), ("int", "sum")], f64=True)
    el = [b[i * 37:(i + 1) * 37] for i in range(4)]
    assert [e[5:13].hex() for e in el] == ["0000000000000bb7", "7fffffffffffffff", "7fffffffffffffff", "ffffffffffffffff"]
    assert el[0][13:].hex() == "7ff8000000000000" + "7fc00000" + "0000000000000000" + "00000000"
    assert el[1][13:].hex() == "7ff8000000000000" + "7fc00000" + "0000000000000000" + "00000000"
    assert el[2][13:].hex() == "3ff0000010000000" + "3f800000" + "0000000000000001" + "00000001"
    assert el[3][13:].hex() == "fe37e43c8800759c" + "ff800000" + "8000000000000000" + "00000000"


@pytest.mark.parametrize("f64", [False, True])
def test_encode_sizes_and_too_small_an_output(f64):
    fields = U.encode_layouts()[2]
    for n in U.ENC_SIZES:
        rows = U.rows_slice(U.encode_rows(f64), n)
        assert orc.wire_encode(_rows_array(rows), fields, f64) == W.encode(rows, fields, f64)
    a = _rows_array(U.encode_rows(f64))
    L = orc.wire_layout(fields)
    out = np.zeros(len(a) * 41, dtype=np.uint8)
    assert orc._wire_lib().oracle_wire_encode(ctypes.byref(L), a.ctypes.data, len(a), int(f64), out.ctypes.data,
                                              len(a) * 41 - 1) == -1
    assert not out.any()

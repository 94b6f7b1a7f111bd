"""The OVER window C-ABI without a GPU: every refusal that fw_over_create makes before it touches the device, with
its code and a message, and the new structs' layouts against the ctypes mirror."""
import ctypes
import os
import subprocess

import pytest

from flink_amd import _native as N
from flink_amd.over import Over, over_config

HEADER_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def _create(frame, column_types=("long",), aggregates=(("sum", 0),), patch=None, **kw):
    c = over_config(frame, list(column_types), list(aggregates), **kw)
    if patch:
        patch(c)
    h = ctypes.c_void_p()
    rc = N.lib().fw_over_create(ctypes.byref(c), ctypes.byref(h))
    msg = N.lib().fw_over_last_error(h).decode() if h else ""
    N.lib().fw_over_destroy(h)
    return rc, msg


def _set(**fields):
    def patch(c):
        for f, v in fields.items():
            setattr(c, f, v)
    return patch


@pytest.mark.parametrize("frame,fragment", [
    (Over.rows(-1), "[0, 2^31)"),
    (Over.rows(1 << 31), "[0, 2^31)"),
    (Over.range(-1), "t must be >= 0"),
    (Over(4), "kind must be"),
    (Over(-1), "kind must be"),
])
def test_frames_refused_before_the_device(frame, fragment):
    rc, msg = _create(frame)
    assert rc == N.FW_ERR_ARG and fragment in msg, (rc, msg)


@pytest.mark.parametrize("patch,fragment", [
    (_set(row_columns=0), "row_columns"),
    (_set(row_columns=9), "row_columns"),
    (_set(row_aggregates=0), "row_aggregates"),
    (_set(row_aggregates=17), "row_aggregates"),
])
def test_select_lists_refused_before_the_device(patch, fragment):
    for frame in (Over.rows(2), Over.range(5), Over.unbounded_rows(), Over.unbounded_range()):
        rc, msg = _create(frame, patch=patch)
        assert rc == N.FW_ERR_ARG and fragment in msg, (rc, msg)


@pytest.mark.parametrize("fn", ["sum", "avg"])
def test_float_sum_and_avg_are_unsupported(fn):
    for frame in (Over.rows(2), Over.range(5), Over.unbounded_rows(), Over.unbounded_range()):
        rc, msg = _create(frame, column_types=("long", "float"), aggregates=(("count", 0), (fn, 1)))
        assert rc == N.FW_ERR_UNSUPPORTED and "Float" in msg, (rc, msg)


def test_null_handles_and_null_config():
    L = N.lib()
    n = ctypes.c_int64()
    h = ctypes.c_void_p()
    assert L.fw_over_create(None, ctypes.byref(h)) == N.FW_ERR_ARG
    assert L.fw_over_push_batch(None, None, None, None, None, None, 0) == N.FW_ERR_ARG
    assert L.fw_over_push_batch_device(None, None, None, None, None, None, 0) == N.FW_ERR_ARG
    assert L.fw_over_advance_watermark(None, 0, ctypes.byref(n)) == N.FW_ERR_ARG
    assert L.fw_over_drain(None, None, None, 0, ctypes.byref(n)) == N.FW_ERR_ARG
    assert L.fw_over_rows_device(None, None, ctypes.byref(n)) == N.FW_ERR_ARG
    assert L.fw_over_get_stats(None, None) == N.FW_ERR_ARG
    assert L.fw_over_clear_pending(None) == N.FW_ERR_ARG
    assert L.fw_over_snapshot_key_group(None, 0, None, 0, 0, ctypes.byref(n), ctypes.byref(n)) == N.FW_ERR_ARG
    assert L.fw_over_restore_key_group(None, 0, None, 0, 0) == N.FW_ERR_ARG
    assert L.fw_over_last_error(None) == b"null handle"
    L.fw_over_destroy(None)


def test_constants_match_the_header():
    src = open(os.path.join(HEADER_DIR, "flink_window.h")).read()
    for name in ("FW_OVER_BOUNDED_ROWS", "FW_OVER_BOUNDED_RANGE", "FW_OVER_UNBOUNDED_ROWS", "FW_OVER_UNBOUNDED_RANGE"):
        assert f"#define {name} {getattr(N, name)} " in src
    assert "#define FW_OVER_ACC_WORDS(columns) (1 + 5 * (columns))" in src and N.fw_over_acc_words(8) == 41


def test_struct_layouts_match_header(tmp_path):
    src = tmp_path / "layout.c"
    structs = {"fw_over_config": N.FwOverConfig, "fw_over_rows": N.FwOverRows, "fw_over_stats": N.FwOverStats,
               "fw_over_state": N.FwOverState}
    body = '  printf("%zu\\n%zu\\n", sizeof(fw_config), sizeof(fw_list_config));\n'
    for name, cls in structs.items():
        body += f'  printf("%zu\\n", sizeof({name}));\n'
        body += "".join(f'  printf("%zu\\n", offsetof({name}, {f}));\n' for f, _ in cls._fields_)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "flink_window.h"\nint main(void) {\n' + body +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", HEADER_DIR, "-o", str(exe), str(src)])
    out = iter(int(x) for x in subprocess.check_output([str(exe)]).split())
    # fw_config and fw_list_config do not grow: the OVER operator's configuration is a struct of its own
    assert ctypes.sizeof(N.FwConfig) == next(out)
    assert ctypes.sizeof(N.FwListConfig) == next(out) == 136
    sizes = {"fw_over_config": 152, "fw_over_rows": 40, "fw_over_stats": 64, "fw_over_state": 64}
    for name, cls in structs.items():
        assert ctypes.sizeof(cls) == next(out) == sizes[name], name
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == next(out), (name, f)

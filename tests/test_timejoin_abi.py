"""The time-windowed join C-ABI without a GPU: every refusal that fw_tjoin_create makes before it touches the device,
with its code and a message, and the new structs' layouts and prototypes against the ctypes mirror."""
import ctypes
import os
import re
import subprocess

import pytest

from flink_amd import _native as N
from flink_amd.timejoin import JOIN_TYPES, tjoin_config

HEADER_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
B60 = 1 << 60


def _create(join_type="inner", lower=-10, upper=20, patch=None, **kw):
    c = tjoin_config(join_type, lower, upper, **kw)
    if patch:
        patch(c)
    h = ctypes.c_void_p()
    rc = N.lib().fw_tjoin_create(ctypes.byref(c), ctypes.byref(h))
    msg = N.lib().fw_tjoin_last_error(h).decode() if h else ""
    N.lib().fw_tjoin_destroy(h)
    return rc, msg


def _set(**fields):
    def patch(c):
        for f, v in fields.items():
            setattr(c, f, v)
    return patch


@pytest.mark.parametrize("kw,fragment", [
    (dict(join_type=4), "join_type must be"),
    (dict(join_type=-1), "join_type must be"),
    (dict(lower=5, upper=4), "lower > upper"),
    (dict(lower=0, upper=-1), "lower > upper"),
    (dict(allowed_lateness=-1), "allowed lateness must be non-negative"),
    (dict(allowed_lateness=B60), "below 2^60"),
    (dict(lower=-B60, upper=0), "(-2^60, 2^60)"),
    (dict(lower=0, upper=B60), "(-2^60, 2^60)"),
    (dict(lower=B60, upper=B60), "(-2^60, 2^60)"),
    (dict(max_pairs=-1), "max_pairs"),
    (dict(max_parallelism=0), "KeyGroupRange"),
    (dict(max_parallelism=128, key_group_range=(5, 4)), "KeyGroupRange"),
    (dict(max_parallelism=128, key_group_range=(0, 128)), "KeyGroupRange"),
    (dict(max_parallelism=128, key_group_range=(-1, 3)), "KeyGroupRange"),
    (dict(patch=_set(key_kind=7)), "key_kind"),
    (dict(expected_keys=-1), "expected_keys"),
    (dict(max_batch=-1), "expected_keys and max_batch"),
])
def test_configurations_refused_before_the_device(kw, fragment):
    for jt in ("inner", "full") if "join_type" not in kw else (kw["join_type"],):
        rc, msg = _create(**{**kw, "join_type": jt})
        assert rc == N.FW_ERR_ARG and fragment in msg, (rc, msg)


def test_null_handles_and_null_config():
    L = N.lib()
    n = ctypes.c_int64()
    h = ctypes.c_void_p()
    assert L.fw_tjoin_create(None, ctypes.byref(h)) == N.FW_ERR_ARG
    assert L.fw_tjoin_push_batch(None, None, None, None, None, None, 0) == N.FW_ERR_ARG
    assert L.fw_tjoin_push_batch_device(None, None, None, None, None, None, 0) == N.FW_ERR_ARG
    assert L.fw_tjoin_advance_watermark(None, 0, ctypes.byref(n), ctypes.byref(n)) == N.FW_ERR_ARG
    assert L.fw_tjoin_drain(None, None, None, 0, ctypes.byref(n)) == N.FW_ERR_ARG
    assert L.fw_tjoin_rows_device(None, None, ctypes.byref(n)) == N.FW_ERR_ARG
    assert L.fw_tjoin_get_stats(None, None) == N.FW_ERR_ARG
    assert L.fw_tjoin_clear_pending(None) == N.FW_ERR_ARG
    assert L.fw_tjoin_snapshot_key_group(None, 0, None, 0, 0, ctypes.byref(n), ctypes.byref(n)) == N.FW_ERR_ARG
    assert L.fw_tjoin_restore_key_group(None, 0, None, 0, 0) == N.FW_ERR_ARG
    assert L.fw_tjoin_last_error(None) == b"null handle"
    L.fw_tjoin_destroy(None)


def test_constants_match_the_header():
    src = open(os.path.join(HEADER_DIR, "flink_window.h")).read()
    for name in ("FW_TJOIN_INNER", "FW_TJOIN_LEFT", "FW_TJOIN_RIGHT", "FW_TJOIN_FULL"):
        assert re.search(rf"#define {name} {getattr(N, name)}\b", src), name
    assert JOIN_TYPES == {"inner": 0, "left": 1, "right": 2, "full": 3}


def test_prototypes_match_the_ctypes_mirror():
    """every fw_tjoin_ prototype of the header is bound, with as many arguments as the header declares"""
    src = open(os.path.join(HEADER_DIR, "flink_window.h")).read()
    protos = re.findall(r"^(?:int|void|const char\*) (fw_tjoin_\w+)\(([^;]*)\);", src, re.M | re.S)
    names = {n for n, _ in protos}
    assert names == {n for n in N.SIGNATURES if n.startswith("fw_tjoin_")} and len(names) == 12
    for name, args in protos:
        assert len(N.SIGNATURES[name][1]) == len(args.split(",")), name
        assert hasattr(N.lib(), name)


def test_struct_layouts_match_header(tmp_path):
    src = tmp_path / "layout.c"
    structs = {"fw_tjoin_config": N.FwTjoinConfig, "fw_tjoin_rows": N.FwTjoinRows, "fw_tjoin_stats": N.FwTjoinStats,
               "fw_tjoin_state": N.FwTjoinState}
    body = '  printf("%zu\\n%zu\\n%zu\\n", sizeof(fw_config), sizeof(fw_list_config), sizeof(fw_over_config));\n'
    for name, cls in structs.items():
        body += f'  printf("%zu\\n", sizeof({name}));\n'
        body += "".join(f'  printf("%zu\\n", offsetof({name}, {f}));\n' for f, _ in cls._fields_)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "flink_window.h"\nint main(void) {\n' + body +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", HEADER_DIR, "-o", str(exe), str(src)])
    out = iter(int(x) for x in subprocess.check_output([str(exe)]).split())
    # the existing configurations do not grow: the join's is a struct of its own
    assert ctypes.sizeof(N.FwConfig) == next(out)
    assert ctypes.sizeof(N.FwListConfig) == next(out) == 136
    assert ctypes.sizeof(N.FwOverConfig) == next(out) == 152
    sizes = {"fw_tjoin_config": 72, "fw_tjoin_rows": 72, "fw_tjoin_stats": 112, "fw_tjoin_state": 72}
    for name, cls in structs.items():
        assert ctypes.sizeof(cls) == next(out) == sizes[name], name
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == next(out), (name, f)

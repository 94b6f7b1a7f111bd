"""Window joins, the part that needs no GPU: fw_list_create's refusals for the join fields, the argument checks of the
new entry points that come before the device, the new struct layouts against the header, and the reference side of
tests/test_gpu_join.py on its own -- the CoGroupJoinITCase fixture and every seeded stream through the oracle and the
Python split / cross product of tests/join_util.py -- with the classes of rows the GPU tests mean to exercise."""
import ctypes
import os
import subprocess

import pytest

from flink_amd import _native as N
from tests import join_util as J

HEADER_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
KATS = J.load_kats()


def _cfg(**kw):
    c = N.FwListConfig()
    c.assigner, c.size, c.emit_contents = N.FW_TUMBLING, 100, 1
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _create(join=0, max_join_pairs=0, **kw):
    c = _cfg(**kw)
    jc = N.FwJoinConfig(join=join, max_join_pairs=max_join_pairs)
    h = ctypes.c_void_p()
    rc = N.lib().fw_list_create_join(ctypes.byref(c), ctypes.byref(jc), ctypes.byref(h))
    msg = N.lib().fw_list_last_error(h).decode() if h else ""
    N.lib().fw_list_destroy(h)
    return rc, msg


@pytest.mark.parametrize("kw,fragment", [
    (dict(join=3), "join must be"),
    (dict(join=-1), "join must be"),
    (dict(join=N.FW_JOIN_INNER, emit_contents=0), "emit_contents must be 1"),
    (dict(join=N.FW_JOIN_COGROUP, emit_contents=0), "emit_contents must be 1"),
    (dict(join=N.FW_JOIN_INNER, max_join_pairs=-1), "max_join_pairs"),
])
def test_create_refuses_before_the_device(kw, fragment):
    rc, msg = _create(**kw)
    assert rc == N.FW_ERR_ARG and fragment in msg, (rc, msg)


def test_new_entry_points_refuse_a_null_handle():
    L = N.lib()
    n = ctypes.c_int64()
    assert L.fw_list_push_batch_side(None, 0, None, None, None, None, 0) == N.FW_ERR_ARG
    assert L.fw_list_push_batch_side_device(None, 1, None, None, None, None, 0) == N.FW_ERR_ARG
    assert L.fw_list_join_pending(None, ctypes.byref(n), None, None) == N.FW_ERR_ARG
    assert L.fw_list_drain_join(None, None, None, 0, None, 0, None, 0, None, None, None) == N.FW_ERR_ARG
    assert L.fw_list_join_device(None, None, None, None, None, None, None, None) == N.FW_ERR_ARG


def test_constants_match_the_header():
    src = open(os.path.join(HEADER_DIR, "flink_window.h")).read()
    for name in ("FW_JOIN_NONE", "FW_JOIN_COGROUP", "FW_JOIN_INNER"):
        assert f"#define {name} {getattr(N, name)}\n" in src
    assert "#define FW_ORD_SIDE (1LL << 62)" in src and N.FW_ORD_SIDE == 1 << 62 == J.SIDE


def test_struct_layouts_match_header(tmp_path):
    src = tmp_path / "layout.c"
    structs = {"fw_join_config": N.FwJoinConfig, "fw_join_pairs": N.FwJoinPairs}
    body = '  printf("%zu\\n", sizeof(fw_list_config));\n'
    for name, cls in structs.items():
        body += f'  printf("%zu\\n", sizeof({name}));\n'
        body += "".join(f'  printf("%zu\\n", offsetof({name}, {f}));\n' for f, _ in cls._fields_)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "flink_window.h"\nint main(void) {\n' + body +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", HEADER_DIR, "-o", str(exe), str(src)])
    out = iter(int(x) for x in subprocess.check_output([str(exe)]).split())
    # the list operator's configuration keeps its layout: the join travels in a struct of its own
    assert ctypes.sizeof(N.FwListConfig) == next(out) == 136
    for name, cls in structs.items():
        assert ctypes.sizeof(cls) == next(out) == {"fw_join_config": 16, "fw_join_pairs": 40}[name]
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == next(out), (name, f)


def test_a_null_or_zeroed_join_is_fw_list_create():
    # (before the device: the same refusal as fw_list_create's for the same bad configuration, join or not)
    for jc in (None, N.FwJoinConfig()):
        c = _cfg(size=-1)
        h = ctypes.c_void_p()
        rc = N.lib().fw_list_create_join(ctypes.byref(c), ctypes.byref(jc) if jc is not None else None, ctypes.byref(h))
        assert rc == N.FW_ERR_ARG and "TumblingEventTimeWindows" in N.lib().fw_list_last_error(h).decode()
        N.lib().fw_list_destroy(h)


# ---------------------------------------------------------------- the reference alone
def _ref_results(case, interleave):
    from oracle import oracle as orc
    rj = J.RefJoin(orc.ListWindowOracle(assigner="tumbling", size=KATS["window"]["size"]))
    stream = J.kat_stream(case, interleave, KATS["watermarks"]["delta"])
    for st in stream:
        rj.step(st)
    pushed = [(k, t) for st in stream if st[0] == "push" for k, t in zip(st[2], st[3])]
    return rj.firings(), pushed


def kat_results(case, firings, pushed):
    """the case's results in the fixture's form, from firings (row, first, second)"""
    if case["mode"] == "cogroup":
        return sorted(([[row[1], v] for _, v, _ in a], [[row[1], v] for _, v, _ in b]) for row, a, b in firings)
    out = []
    for row, a, b in firings:
        v1, v2, o1, o2 = J.expected_pairs(a, b)
        out += [([row[1], int(x), pushed[p][1]], [row[1], int(y), pushed[q][1]]) for x, y, p, q in zip(v1, v2, o1, o2)]
    return sorted(out)


def kat_expected(case):
    if case["mode"] == "cogroup":
        return sorted((e["first"], e["second"]) for e in case["expected"])
    return sorted((a, b) for a, b in case["expected"])


@pytest.mark.parametrize("interleave", ["first", "alternate"])
@pytest.mark.parametrize("name", sorted(KATS["cases"]))
def test_reference_reproduces_the_kats(name, interleave):
    case = KATS["cases"][name]
    firings, pushed = _ref_results(case, interleave)
    assert kat_results(case, firings, pushed) == kat_expected(case)
    assert len(case["expected"]) == {"testCoGroup": 4, "testJoin": 16, "testSelfJoin": 22}[name]


@pytest.mark.parametrize("name,cfg,skw", J.SEEDED, ids=[s[0] for s in J.SEEDED])
def test_seeded_streams_cover_what_the_gpu_tests_mean(name, cfg, skw):
    rj = J.RefJoin(J.make_ref(**cfg))
    for st in J.seeded_stream(**skw):
        rj.step(st)
    c = J.classes(rj.firings())
    assert c["rows"] > 300 and c["both"] > 50 and c["pairs"] > 400, c
    assert c["only_first"] > 10 and c["only_second"] > 10 and c["n2_is_1"] > 0 and c["n1_is_1"] > 0, c
    assert rj.ref.late_dropped > 0, "records beyond the allowed lateness"
    if cfg.get("trigger", "event_time") == "event_time" and not cfg.get("purging"):
        assert c["refired"] > 0, "late firings within the allowed lateness"
    if cfg.get("purging"):
        assert c["largest"] <= 2  # three elements per firing
    if cfg["assigner"] == "sliding":
        assert c["largest"] >= 16 and c["rows"] > 2000, c


def test_hot_and_count_streams():
    from tests.join_util import count_stream, hot_stream
    from oracle import oracle as orc
    rj = J.RefJoin(orc.ListWindowOracle(assigner="tumbling", size=1000))
    for st in hot_stream():
        rj.step(st)
    f = rj.firings()
    c = J.classes(f)
    hot = [(len(a), len(b)) for _, a, b in f if len(a) * len(b) > 1 << 16]
    assert hot == [(1500, 1100)] and c["only_first"] >= 5 and c["only_second"] >= 5 and c["n2_is_1"] >= 1, (hot, c)
    assert sum(st[0] == "push" and st[2][0] == 7 for st in hot_stream()) >= 6  # the hot key's alternating batches
    n = sum(len(st[2]) for st in count_stream() if st[0] == "push")
    assert n == 140000 and 70000 * 70000 > 1 << 32


def test_heap_bridge_carries_the_side_in_the_ordinal():
    from flink_amd import heapstate as H
    assert H.FW_ORD_SIDE == N.FW_ORD_SIDE
    # TaggedUnion values as (side, value): one window of key "a" with elements of both inputs, one of input 2 only
    mappings = [((0, 3), "a", [(0, 10), (1, 20), (0, 11)]), ((3, 6), "a", [(1, 21)])]
    kw = dict(key_id=lambda k: 1, value_of=lambda v: v[1], ordinal_base=5, side_of=lambda v: v[0])
    lists, elems = H.list_state_from_heap(mappings, {("a", (0, 3), 2)}, **kw)
    assert [e[2] for e in elems] == [5, 6 | J.SIDE, 7, 8 | J.SIDE] and [e[1] for e in elems] == [10, 20, 11, 21]
    assert [x["timer"] for x in lists] == [1, 0]
    back = H.heap_from_list_state(lists, elems, lambda k: "a", lambda e: (int(e[2] & J.SIDE != 0), e[1]))
    assert back == mappings
    plain, pe = H.list_state_from_heap(mappings, set(), **{**kw, "side_of": None})
    assert [e[2] for e in pe] == [5, 6, 7, 8]  # without side_of: as before
    wins, se = H.session_state_from_heap([((0, 3), "a", mappings[0][2])], [(None, "a", [((0, 3), (0, 3))])], set(), **kw)
    assert [e[2] for e in se] == [5, 6 | J.SIDE, 7] and wins[0]["n_elems"] == 3

"""Session windows with merging_state (CountTrigger over sessions, session snapshots), the host side: the Python
reference (tests/session_ref.py) against the reference's known answers (tests/golden/session_count_kats.json) and,
on EventTimeTrigger streams, against the reference-pinned ListState oracle; the C ABI of the new struct and entry
points.  The GPU side is tests/test_gpu_session_state.py."""
import ctypes
from collections import Counter

import numpy as np
import pytest

from flink_amd import _native as N
from flink_amd import heapstate as H
from oracle import oracle as orc
from tests import session_heap_util as SH
from tests.session_ref import SessionRef, load_session_kats, session_stream

KATS = load_session_kats()
CFG = dict(gap=3000, trigger="count", trigger_count=4, purging=True)


def kat_rows(op, seen):
    rows = op.rows()
    return sorted([int(r[f]) for f in ("key", "start", "end", "count", "sum")] for r in rows[seen:]), len(rows)


def kat_state(st):
    """session_state() reduced to the KAT file's form (values only: the savepoint's lists hold no timestamps)"""
    return sorted([k, s, e, ss, se, c, [v for _, v, _ in lst]] for k, rows in st.items()
                  for s, e, ss, se, c, _, lst in rows)


@pytest.mark.parametrize("case", KATS, ids=[c["name"] for c in KATS])
def test_reference_reproduces_kats(case):
    ref = SessionRef(**CFG)
    if case.get("initial_state"):
        ref.load_state([tuple(r) for r in case["initial_state"]])
    seen = 0
    for step in case["steps"]:
        if step.get("restore"):  # the restatement's restore is its own state handed to a fresh operator
            st, ref = kat_state(ref.session_state()), SessionRef(**CFG)
            ref.load_state([tuple(r) for r in st])
            seen = 0
            continue
        k, t, v = (np.array(c, dtype=np.int64) for c in zip(*step["elements"]))
        ref.process(k, t, v)
        got, seen = kat_rows(ref, seen)
        assert got == sorted(step["rows"])
        if "state" in step:
            assert kat_state(ref.session_state()) == sorted(step["state"])
    assert ref.late_dropped == 0


def _firings(op):
    out = Counter()
    for r, el in op.contents():
        ords = "ordinal" if "ordinal" in el.dtype.names else "ord"
        out[tuple(int(r[f]) for f in ("epoch", "key", "start", "end", "count", "sum", "min", "max", "first")) +
            (tuple(zip(el["ts"].tolist(), el["val"].tolist(), el[ords].tolist())),)] += 1
    return out


@pytest.mark.parametrize("cfg", [dict(gap=30), dict(gap=30, lateness=200, purging=True, side_output=True),
                                 dict(gap=25, lateness=120, evictor="count", evict_arg=3),
                                 dict(gap=40, evictor="count", evict_arg=2, evict_after=True, purging=True)],
                         ids=["plain", "late-purging-side", "late-evict-before", "evict-after-purging"])
@pytest.mark.parametrize("zipf", [False, True], ids=["uniform", "zipf"])
def test_reference_equals_list_oracle_on_event_time_sessions(cfg, zipf):
    # the merge, HashSet-order and list-order machinery the count trigger rides on, against oracle/list_oracle.cpp
    ref = SessionRef(**cfg)
    orc_ref = orc.ListWindowOracle(assigner="session", **cfg)
    k, t, v = session_stream(7 + len(str(cfg)), 6000, 120, 6000, 150, zipf=zipf)
    wm = -10**9
    for b in range(6):
        sl = slice(b * 1000, (b + 1) * 1000)
        for h in (ref, orc_ref):
            h.process(k[sl], t[sl], v[sl])
        wm = max(wm, int(t[sl].max()) - 100)
        if b % 3 != 1:
            for h in (ref, orc_ref):
                h.watermark(wm)
    for h in (ref, orc_ref):
        h.watermark((1 << 63) - 1)
    assert _firings(ref) == _firings(orc_ref)
    assert ref.merges > 0 and ref.late_dropped == orc_ref.late_dropped
    if cfg.get("side_output"):
        assert sorted(zip(*[c.tolist() for c in ref.side_rows()])) == sorted(zip(*[c.tolist() for c in
                                                                                  orc_ref.side_rows()]))


def test_session_state_abi(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in N.FwSessionState._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flink_window.h"\nint main(void) {\n'
                   '  printf("%zu\\n%zu\\n%zu\\n", sizeof(fw_session_state), sizeof(fw_list_config), '
                   'offsetof(fw_list_config, merging_state));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(fw_session_state, {f}));\n' for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(N.FwSessionState) == 11 * 8
    assert out[1] == ctypes.sizeof(N.FwListConfig) == 136  # unchanged: the flag took the padding slot
    assert out[2] == N.FwListConfig.merging_state.offset == 52
    assert out[3:] == [getattr(N.FwSessionState, f).offset for f in fields]
    lib = ctypes.CDLL(N.LIB_PATH)
    assert lib.fw_list_snapshot_sessions and lib.fw_list_restore_sessions


@pytest.mark.parametrize("kw", [dict(assigner=N.FW_TUMBLING, size=100), dict(assigner=N.FW_GLOBAL),
                                dict(assigner=N.FW_SESSION, size=100, merging_state=2)])
def test_merging_state_is_for_sessions_only(kw):
    c = N.FwListConfig()
    c.key_group_start = c.key_group_end = -1
    c.merging_state = 1
    for k, v in kw.items():
        setattr(c, k, v)
    h = ctypes.c_void_p()
    rc = N.lib().fw_list_create(ctypes.byref(c), ctypes.byref(h))
    msg = N.lib().fw_list_last_error(h).decode() if h else ""
    N.lib().fw_list_destroy(h)
    assert rc == N.FW_ERR_ARG and "merging_state" in msg


# ---------------------------------------------------------------- the reference's session savepoints
@pytest.mark.parametrize("version", ["1.3", "1.4"])
def test_session_fixture_content(version):
    _, mk, rk, meta, states, tmeta, timers = SH.read(SH.load(version, mint=False))
    assert list(mk.key_groups()) == [0] and list(rk.key_groups()) == [0]
    assert meta["states"] == [("REDUCING", "count"), ("LIST", "window-contents"), ("LIST", "merging-window-set")]
    assert states["count"] == [((10, 4000), "key1", 2)]                                  # under the actual window
    assert states["window-contents"] == [((10, 3010), "key1", [("key1", 1), ("key1", 2)])]  # under the state window
    assert sorted(states["merging-window-set"]) == [                      # key2's purged window: in the mapping only
        (H.VOID_NAMESPACE, "key1", [((10, 4000), (10, 3010))]), (H.VOID_NAMESPACE, "key2", [((0, 6500), (0, 3000))])]
    assert sorted(timers) == [("key1", (10, 4000), 3999), ("key2", (0, 6500), 6499)]    # two cleanup timers
    assert tmeta["versioned"] is False
    _, _, _, meta, states, _, timers = SH.read(SH.load(version, mint=True))
    assert meta["states"] == [("LIST", "window-contents"), ("LIST", "merging-window-set")]
    assert states == {"window-contents": [], "merging-window-set": []} and timers == []


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("mint", [False, True], ids=["written", "mint"])
@pytest.mark.parametrize("version", ["1.3", "1.4"])
def test_session_fixture_rewritten_byte_exact(version, mint, seed):
    # three registered states in the host's registration order with their ids, the VoidNamespace state among them,
    # each in its table's iteration order (1.3 NestedMapsStateTable, 1.4 CopyOnWriteStateTable), the timers in theirs
    data = SH.load(version, mint)
    assert SH.rewrite_shuffled(data, version, seed) == data


def test_session_heap_bridges_round_trip():
    _, _, _, _, states, _, timers = SH.read(SH.load("1.4", mint=False))
    wins, elems = H.session_state_from_heap(states["window-contents"], states["merging-window-set"], set(timers),
                                            SH.KEY_IDS.__getitem__, lambda v: v[1],
                                            counts=H.trigger_counts_from_heap(states["count"]))
    assert sorted((w["key"], w["start"], w["end"], w["state_start"], w["state_end"], w["trigger_state"], w["timer"],
                   w["n_elems"]) for w in wins) == [(1, 10, 4000, 10, 3010, 2, 0, 2), (2, 0, 6500, 0, 3000, 0, 0, 0)]
    assert [e[1] for e in elems] == [1, 2]
    back, tm = H.heap_from_session_state(wins, elems, SH.KEY_NAMES.__getitem__,
                                         lambda key, e: (key, int(e[1])), count_trigger=True)
    assert {n: sorted(m) for n, m in back.items()} == {n: sorted(m) for n, m in states.items()}
    assert tm == set(timers)
    # the aggregating operator: rows keyed by the actual window, the state window resolved through the mapping
    rows = H.session_rows_from_heap([((10, 3010), "key1", 7)], states["merging-window-set"], set(timers),
                                    SH.KEY_IDS.__getitem__, lambda a: dict(count=1, sum=a, min=a, max=a))
    # (timer 1: with lateness 0 the cleanup timer at 3999 is also an EventTimeTrigger's maxTimestamp timer)
    assert rows == [dict(key=1, start=10, end=4000, timer=1, count=1, sum=7, min=7, max=7)]
    out = H.heap_from_session_rows(rows, SH.KEY_NAMES.__getitem__, lambda r: r["sum"])
    assert out == {"window-contents": [((10, 4000), "key1", 7)],
                   "merging-window-set": [(H.VOID_NAMESPACE, "key1", [((10, 4000), (10, 4000))])]}

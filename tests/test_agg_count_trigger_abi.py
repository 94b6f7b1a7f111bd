"""CountTrigger on the aggregating operator, without a GPU: the three entry points' prototypes, what
fw_create_count_trigger refuses before it touches the device (through ctypes and through GpuWindowOperator), and a
vetting of every configuration and stream the GPU tests use (tests/test_gpu_agg_count_trigger.py): the restatement
tests/count_trigger_ref.py equals the pinned ListWindowOracle on them, and the classes of behaviour the GPU tests mean
to cover are asserted to occur."""
import ctypes
import os
import re

import numpy as np
import pytest

from flink_amd import (CountSumMinMax, CountTrigger, CountWindows, EventTimeSessionWindows, FirstElementReduce,
                       PurgingTrigger, SlidingEventTimeWindows, TumblingEventTimeWindows)
from flink_amd import _native as N
from flink_amd.operator import COUNT_STATE_DTYPE, GpuWindowOperator
from tests import agg_count_trigger_util as U
from tests import time_edges_util as TE
from tests.continuous_ref import drive, seeded_stream

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flink_window.h")
NEW = ["fw_create_count_trigger", "fw_snapshot_key_group_trigger_count", "fw_restore_key_group_trigger_count"]


def _create(max_count=3, **kw):
    c = N.FwConfig()
    c.key_group_start = c.key_group_end = -1
    for k, v in kw.items():
        setattr(c, k, v)
    h = ctypes.c_void_p()
    rc = N.lib().fw_create_count_trigger(ctypes.byref(c), max_count, ctypes.byref(h))
    msg = N.lib().fw_last_error(h).decode()
    N.lib().fw_destroy(h)
    return rc, msg


def _kind(ctype):
    if ctype in (ctypes.c_int64, ctypes.c_int32, ctypes.c_int):
        return ctype
    return "pointer"


@pytest.mark.parametrize("name", NEW)
def test_header_and_ctypes_agree(name):
    text = open(HEADER).read()
    m = re.search(r"\bint " + name + r"\(([^)]*)\);", text)
    assert m, name
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    want = []
    for p in params:
        ty = p.rsplit(" ", 1)[0] if not p.endswith("*") else p
        want.append("pointer" if "*" in p else {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}[ty])
    res, args = N.SIGNATURES[name]
    assert res is ctypes.c_int
    assert [_kind(a) for a in args] == want, (params, args)
    assert hasattr(N.lib(), name)


OTHER_AGGREGATES = {
    "hll": dict(aggregate=N.FW_AGG_HLL),
    "first": dict(aggregate=N.FW_AGG_FIRST),
    "first_max": dict(aggregate=N.FW_AGG_FIRST_MAX),
    "minby": dict(aggregate=N.FW_AGG_MINBY),
    "maxby": dict(aggregate=N.FW_AGG_MAXBY),
    "tdigest": dict(aggregate=N.FW_AGG_TDIGEST, value_type=N.FW_VAL_F64),
    "row": dict(aggregate=N.FW_AGG_ROW, row_columns=1, row_aggregates=1),
}


@pytest.mark.parametrize("kw,code,fragment", [
    (dict(assigner=N.FW_SESSION, gap=30), N.FW_ERR_UNSUPPORTED, "session windows is not offered on the aggregating"),
    (dict(assigner=N.FW_COUNT, size=10, slide=5, aggregate=N.FW_AGG_FIRST), N.FW_ERR_UNSUPPORTED,
     "CountTrigger over count windows"),
    (dict(assigner=N.FW_TUMBLING, size=100, max_count=0), N.FW_ERR_ARG, "maxCount must be in [1, 2^31)"),
    (dict(assigner=N.FW_TUMBLING, size=100, max_count=-4), N.FW_ERR_ARG, "maxCount must be in [1, 2^31)"),
    (dict(assigner=N.FW_SLIDING, size=100, slide=20, max_count=1 << 31), N.FW_ERR_ARG, "maxCount must be in [1, 2^31)"),
    (dict(assigner=N.FW_TUMBLING, size=100, trigger=N.FW_TRIGGER_COUNT), N.FW_ERR_ARG, "fw_config.trigger must be 0"),
    (dict(assigner=N.FW_TUMBLING, size=100, trigger=N.FW_TRIGGER_CONTINUOUS_EVENT_TIME, trigger_interval=5),
     N.FW_ERR_ARG, "fw_config.trigger must be 0"),
] + [(dict(assigner=N.FW_TUMBLING, size=100, **a), N.FW_ERR_UNSUPPORTED,
      "is offered for the count/sum/min/max aggregate") for a in OTHER_AGGREGATES.values()],
    ids=["session", "count", "n-0", "n-neg", "n-2^31", "trigger-count", "trigger-continuous"] + list(OTHER_AGGREGATES))
def test_create_refuses(kw, code, fragment):
    kw = dict(kw)
    rc, msg = _create(kw.pop("max_count", 3), device=1 << 20, **kw)  # (refused before the device is touched)
    assert rc == code, msg
    assert fragment in msg
    if code == N.FW_ERR_UNSUPPORTED:  # the message names where the job runs instead
        assert "fw_list_create" in msg


def test_fw_create_still_refuses_the_count_trigger():
    c = N.FwConfig()
    c.key_group_start = c.key_group_end = -1
    c.assigner, c.size, c.trigger = N.FW_TUMBLING, 100, N.FW_TRIGGER_COUNT
    h = ctypes.c_void_p()
    rc = N.lib().fw_create(ctypes.byref(c), ctypes.byref(h))
    msg = N.lib().fw_last_error(h).decode()
    N.lib().fw_destroy(h)
    assert rc == N.FW_ERR_ARG and "unknown trigger" in msg


@pytest.mark.parametrize("kw", [
    dict(assigner=N.FW_TUMBLING, size=100, value_type=vt, key_kind=kk)
    for vt in (N.FW_VAL_I64, N.FW_VAL_I32, N.FW_VAL_F64, N.FW_VAL_I16, N.FW_VAL_I8, N.FW_VAL_F32)
    for kk in (N.FW_KEY_LONG, N.FW_KEY_INT, N.FW_KEY_HASHED)
] + [
    dict(assigner=N.FW_SLIDING, size=300, slide=100),
    dict(assigner=N.FW_SLIDING, size=250, slide=100, allowed_lateness=150, purging=1, side_output=1),
    dict(assigner=N.FW_TUMBLING, size=97, offset=13, allowed_lateness=150, purging=1),
    dict(assigner=N.FW_TUMBLING, size=100, side_output=1, max_count=(1 << 31) - 1),
    dict(assigner=N.FW_TUMBLING, size=100, max_count=1),
])
def test_offered_configurations_reach_the_device(kw):
    kw = dict(kw)
    rc, msg = _create(kw.pop("max_count", 3), device=1 << 20, **kw)
    assert rc == N.FW_ERR_HIP, (rc, msg)


@pytest.mark.parametrize("make,code,fragment", [
    (lambda: GpuWindowOperator(EventTimeSessionWindows.with_gap(30), trigger=CountTrigger.of(3), device=1 << 20),
     N.FW_ERR_UNSUPPORTED, "session windows is not offered"),
    (lambda: GpuWindowOperator(CountWindows.of(10, 5), FirstElementReduce("long"), trigger=CountTrigger.of(3),
                               device=1 << 20), N.FW_ERR_UNSUPPORTED, "CountTrigger over count windows"),
    (lambda: GpuWindowOperator(TumblingEventTimeWindows.of(100), FirstElementReduce("long"),
                               trigger=PurgingTrigger.of(CountTrigger.of(3)), device=1 << 20), N.FW_ERR_UNSUPPORTED,
     "is offered for the count/sum/min/max aggregate"),
    (lambda: GpuWindowOperator(SlidingEventTimeWindows.of(300, 100), CountSumMinMax("double"),
                               trigger=PurgingTrigger.of(CountTrigger.of(3)), device=1 << 20), N.FW_ERR_HIP, ""),
], ids=["session", "count", "first", "offered"])
def test_operator_goes_through_the_new_constructor(make, code, fragment):
    with pytest.raises(N.NativeError) as e:
        make()
    assert e.value.code == code and fragment in str(e.value)


def test_state_dtype_ends_with_the_trigger_count():
    assert COUNT_STATE_DTYPE.names[-1] == "trigger_count" and COUNT_STATE_DTYPE.names[-2] == "timer"


# ------------------------------------------------ the GPU tests' streams: restatement == oracle, classes vetted
def _run(cfg, value_type):
    o, r = U.Oracle(value_type, **cfg), U.Restated(value_type, **cfg)
    k, t, v = U.stream_of(cfg)

    def each():
        assert (o.num_state_entries, o.num_timers, o.late_dropped) == (r.num_state_entries, r.num_timers, r.late_dropped)
    drive([o, r], k, t, v, each=each)
    assert o.row_tuples() == r.row_tuples() and o.side_tuples() == r.side_tuples()
    return o, r


@pytest.fixture(scope="module")
def runs():
    return {(U.cfg_id(c), vt): _run(c, vt) for c in U.CONFIGS for vt in U.VALUE_TYPES}


def test_restatement_equals_oracle_and_rows_exist(runs):
    for c in U.CONFIGS:
        o, _ = runs[(U.cfg_id(c), "long")]
        assert (len(o.row_tuples()) > 1000) == (c["n"] != U.BIG), U.cfg_id(c)
    # the int streams leave 32 bits: some emitted sum differs from the long stream's
    o32, o64 = runs[(U.IDS[3], "int")], runs[(U.IDS[3], "long")]
    assert any(abs(r[5]) > (1 << 30) for r in o32[0].row_tuples()) and len(o32[0].row_tuples()) == len(o64[0].row_tuples())


def test_streams_hold_every_class(runs):
    """a condition on the inputs: a class none of the streams reaches fails here"""
    for c in U.CONFIGS:
        _, r = runs[(U.cfg_id(c), "long")]
        if 1 < c["n"] < U.BIG:
            assert r.carried > 100, U.cfg_id(c)   # windows that fire from a carried count
            assert r.leftover > 100, U.cfg_id(c)  # windows cleaned up with 0 < count < n left
        if c["n"] == U.BIG:
            assert r.leftover > 100 and r.row_tuples() == []
    late = [c for c in U.CONFIGS if c["lateness"] and c["assigner"] == "tumbling" and c["n"] < U.BIG]
    # firings of windows already behind the watermark but within the allowed lateness
    assert sum(runs[(U.cfg_id(c), "long")][1].behind for c in late) > 100
    side = [c for c in U.CONFIGS if c["side_output"]]
    assert sum(len(runs[(U.cfg_id(c), "long")][1].side_tuples()) for c in side) > 50  # side-output records
    drop = [c for c in U.CONFIGS if not c["side_output"] and not c["lateness"] and c["assigner"] == "tumbling"]
    assert sum(runs[(U.cfg_id(c), "long")][1].late_dropped for c in drop) > 50


def test_snapshot_streams_hold_their_classes():
    k, t, v = seeded_stream(21, 20000, 200, 2000, 60)
    h = len(k) // 2
    for c in U.SNAPSHOT_CONFIGS:
        r = U.Restated("long", **c)
        r.process(k[:h], t[:h], v[:h])
        r.watermark(int(t[:h].max()) - 70)
        st = r.ref.state
        assert sum(1 for a in st.values() if a[4] > 0) > 50  # counts that the restored handles must carry on from
        if c["purging"]:
            assert sum(1 for a in st.values() if a[0] == 0 and a[4] == 0) > 10  # purged-and-empty windows in flight
        n0 = len(r.ref._rows)
        r.process(k[h:], t[h:], v[h:])
        assert r.carried > 50 and len(r.ref._rows) > n0


@pytest.mark.parametrize("cfg", [TE.PRE_TUMBLING[1], TE.PRE_SLIDING[1], TE.PRE_SLIDING[3]])
def test_pre_epoch_streams_restatement_equals_oracle(cfg):
    full = dict(assigner=cfg["assigner"], size=cfg["size"], slide=cfg.get("slide", 0), offset=cfg.get("offset", 0),
                lateness=cfg.get("lateness", 0), n=3, purging=cfg.get("purging", False),
                side_output=cfg.get("side_output", False))
    batches, wms = TE.pre_epoch_stream(cfg, n=8000, batch=1000)
    o, r = U.Oracle("long", **full), U.Restated("long", **full)
    for (k, t, v), wm in zip(batches, wms):
        for h in (o, r):
            h.process(k, t, v)
            h.watermark(wm)
        assert (o.num_state_entries, o.num_timers, o.late_dropped) == (r.num_state_entries, r.num_timers, r.late_dropped)
    assert o.row_tuples() == r.row_tuples() and len(o.row_tuples()) > 500
    assert any(x[2] < 0 for x in o.row_tuples())
    assert o.side_tuples() == r.side_tuples()


@pytest.mark.parametrize("name", U.WRAP_NAMES)
def test_long_range_streams_fire_in_the_oracle(name):
    cfg, batches, wms = TE.wrap_case(name)
    o = U.Oracle("long", **U.wrap_cfg(cfg))
    for (k, t, v), wm in zip(batches, wms):
        o.process(k, t, v)
        o.watermark(wm)
    rows = o.row_tuples()
    top = name.split("-")[-2] == "top"
    assert len(rows) > 200 and any((r[2] > (1 << 62)) if top else (r[2] < -(1 << 62)) for r in rows)


def test_hot_stream_closed_form_is_the_oracles():
    for keys in (1, 2):
        for purging in (False, True):
            k, t, v = U.hot_stream(keys)
            cfg = dict(assigner="tumbling", size=1000000, slide=0, offset=0, lateness=0, n=5, purging=purging,
                       side_output=False)
            o = U.Oracle("long", **cfg)
            o.process(k[:20000], t[:20000], v[:20000])  # (the oracle keeps lists: a prefix of the push is enough)
            exp = U.hot_expected(k[:20000], v[:20000], 5, purging)
            assert o.row_tuples() == exp and len(exp) == 4000

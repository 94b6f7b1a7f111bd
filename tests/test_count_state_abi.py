"""CPU-side checks of the count-window state calls: no handle is created, nothing touches the GPU."""
import ctypes

from flink_amd import _native as N


def test_count_state_calls_refuse_a_null_handle():
    L = N.lib()
    nl, ne = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert L.fw_count_snapshot_key_group(None, 0, None, 0, 0, ctypes.byref(nl), ctypes.byref(ne)) == N.FW_ERR_ARG
    assert (nl.value, ne.value) == (-1, -1)
    assert L.fw_count_restore_key_group(None, 0, None, 0, 0) == N.FW_ERR_ARG
    st = N.FwListState()
    assert L.fw_count_restore_key_group(None, 0, ctypes.byref(st), 1, 0) == N.FW_ERR_ARG


def test_count_state_signatures_mirror_the_list_operator():
    for mine, theirs in (("fw_count_snapshot_key_group", "fw_list_snapshot_key_group"),
                         ("fw_count_restore_key_group", "fw_list_restore_key_group")):
        assert N.SIGNATURES[mine] == N.SIGNATURES[theirs]


def test_list_state_dtypes_are_shared_by_both_operator_modules():
    from flink_amd import listwindow, operator
    assert listwindow.LIST_STATE_DTYPE is operator.LIST_STATE_DTYPE
    assert listwindow.ELEM_DTYPE is operator.ELEM_DTYPE
    assert operator.LIST_STATE_DTYPE.names == ("key", "start", "end", "trigger_count", "timer", "n_elems")
    assert operator.ELEM_DTYPE.names == ("ts", "val", "ordinal")
    assert operator.LIST_STATE_DTYPE.itemsize == 48 and operator.ELEM_DTYPE.itemsize == 24

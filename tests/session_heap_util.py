"""The reference's session savepoints (tests/golden/heap/win-op-migration-test-session-with-stateful-trigger{,-mint}-
flink1.{3,4}-snapshot, written by WindowOperatorMigrationTest.java:110-152 and :213-246): read to their content and
rewritten from content, for the CPU and the GPU tests."""
import os
import random

from flink_amd import heapstate as H

HEAP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "heap")
TUP = H.TupleSer(H.StringSer(), H.IntSer())
TW = H.TimeWindowSer()
SERIALIZERS = {"count": (TW, H.StringSer(), H.LongSer()),
               "window-contents": (TW, H.StringSer(), H.ListSer(TUP)),
               "merging-window-set": (H.VoidNamespaceSer(), H.StringSer(), H.ListSer(H.TupleSer(TW, TW)))}
NS_HASHES = {"merging-window-set": H.void_namespace_hash}
KEY_IDS = {"key1": 1, "key2": 2}
KEY_NAMES = {v: k for k, v in KEY_IDS.items()}


def load(version, mint):
    name = f"win-op-migration-test-session-with-stateful-trigger{'-mint' if mint else ''}-flink{version}-snapshot"
    with open(os.path.join(HEAP, name), "rb") as f:
        return f.read()


def read(data):
    """(operator snapshot, managed handle, raw handle, meta, {state: mappings} of key group 0, timer meta, timers)"""
    snap = H.read_operator_snapshot(data)
    mk, rk = snap["managed_keyed"][0], snap["raw_keyed"][0]
    meta, groups = H.read_heap_keyed_state(mk, SERIALIZERS)
    tmeta = {}
    timers = H.read_timers(rk, H.StringSer(), TW, meta=tmeta)
    return snap, mk, rk, meta, groups[0], tmeta[0], list(timers[0]["window-timers"][0])


def write(template, version, states, timers):
    """a savepoint file from content, with the serializer blocks and handle names of `template` (the host's)"""
    snap, mk, rk, meta, _, tmeta, _ = read(template)
    return H.write_savepoint_key_group_0_states(meta, tmeta, states, list(timers), SERIALIZERS, snap["chain_index"],
                                                mk.name, rk.name, ns_hashes=NS_HASHES,
                                                table="nested_maps" if version == "1.3" else "copy_on_write")


def rewrite_shuffled(data, version, seed):
    _, _, _, _, states, _, timers = read(data)
    rnd = random.Random(seed)
    states = {n: list(m) for n, m in states.items()}
    for m in states.values():
        rnd.shuffle(m)
    rnd.shuffle(timers)
    return write(data, version, states, timers)

#!/usr/bin/env python3
"""Benchmark of the window join (flink_amd.join.GpuWindowJoin; fw_list_push_batch_side_device, fw_list_join_device) on
one MI355X: two inputs of 2^23 records per step, 1 s tumbling event-time windows, uniform Long keys, bounded
out-of-orderness 200 ms, 2^24 records per event-second over both inputs (a step is one window's worth), a watermark
after every step.  A step pushes both inputs, advances the watermark, runs the join stage over what fired -- split,
count, and the pairs (row, idx1, idx2, val1, val2) materialised in HBM -- and discards it (the sink).

A (key, window) holds 2^23 / keys elements of each input, so the mean number of pairs per input record is
2^22 / keys: --keys 4194304 gives about 1, --keys 262144 about 16.

Reported, all for information: input records/s and pairs/s over the whole step; the join stage's own time split into
split + count (fw_list_join_pending) and emit (fw_list_join_device with the split done), and the emit kernel's store
bandwidth 40 B x pairs / emit time beside the project's measured copy rate.  `--host-sample N` forms the
same pairs the way a host has to without the stage, on N steps: drain the contents (fw_list_drain) and split and cross
them with numpy.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 6.3e12  # the device copy rate this project measured, B/s


def host_pairs(np, rows, el):
    """CoGroupWindowFunction + JoinCoGroupFunction with numpy over a plain drain: the five pair columns"""
    nr = len(rows)
    order = np.argsort(rows["elem_off"], kind="stable")  # the rows' elements tile the drained elements in this order
    blk = np.repeat(np.arange(nr, dtype=np.int64), rows["count"][order])
    side = (el["ordinal"] >> 62) & 1
    pval = el["val"][np.argsort(blk * 2 + side, kind="stable")]  # a stable partition inside every row's range
    n1 = np.zeros(nr, dtype=np.int64)
    n1[order] = np.bincount(blk[side == 0], minlength=nr)
    n2 = rows["count"] - n1
    npairs = n1 * n2
    total = int(npairs.sum())
    prow = np.repeat(np.arange(nr, dtype=np.int64), npairs)
    q = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(npairs) - npairs, npairs)
    i, j = np.divmod(q, n2[prow])
    idx1 = rows["elem_off"][prow] + i
    idx2 = rows["elem_off"][prow] + n1[prow] + j
    return prow, idx1, idx2, pval[idx1], pval[idx2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1 << 23, help="records per input per step")
    ap.add_argument("--keys", type=int, default=1 << 22)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--host-sample", type=int, default=0, help="steps on which the host baseline is timed too")
    args = ap.parse_args()

    import numpy as np
    import torch
    from flink_amd import TumblingEventTimeWindows
    from flink_amd.datagen import generate_device
    from flink_amd.join import GpuWindowJoin

    rate = args.batch * 1000 // args.window  # per input: a step is one window of event time
    j = GpuWindowJoin(TumblingEventTimeWindows.of(args.window), max_batch=args.batch,
                      expected_elements=int(2 * args.batch * 1.5))
    inputs, wms, m = [], [], -(1 << 63)
    for s in range(args.warmup + args.steps + args.host_sample):
        both = []
        for side, seed in ((0, 0x5EED), (1, 0xC0FFEE)):
            k, t, v, mx = generate_device(seed, s * args.batch, args.batch, args.keys, ts_base=0, rate=rate, jitter=200,
                                          device=0)
            both.append((k, t, v))
            m = max(m, int(mx.item()))
        inputs.append(both)
        wms.append(m - 200)
    torch.cuda.synchronize()
    rows = elems = pairs = 0
    t_split = t_emit = 0.0

    def step(s, host=False):
        nonlocal rows, elems, pairs, t_split, t_emit
        for side in (0, 1):
            j.op.process_batch(*inputs[s][side], side=side)
        j.op.advance_watermark(wms[s])
        if host:
            r, e = j.op.drain()
            return host_pairs(np, r, e)
        a = time.perf_counter()
        nr, ne, npairs = j.join_pending()
        b = time.perf_counter()
        j.join_device()  # (synchronises: the pairs are in HBM when it returns)
        c = time.perf_counter()
        t_split += b - a
        t_emit += c - b
        rows, elems, pairs = rows + nr, elems + ne, pairs + npairs
        j.op.clear_pending()

    for s in range(args.warmup):
        step(s)
    rows = elems = pairs = 0
    t_split = t_emit = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(args.warmup, args.warmup + args.steps):
        step(s)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n_in = 2 * args.batch * args.steps
    host = None
    if args.host_sample:
        h0 = time.perf_counter()
        hp = 0
        for s in range(args.warmup + args.steps, args.warmup + args.steps + args.host_sample):
            hp += len(step(s, host=True)[0])
        hdt = time.perf_counter() - h0
        host = {"steps": args.host_sample, "pairs": hp, "ms_per_step": round(hdt / args.host_sample * 1e3, 1),
                "records_per_s": round(2 * args.batch * args.host_sample / hdt, 1),
                "gpu_over_host": round((n_in / dt) / (2 * args.batch * args.host_sample / hdt), 2),
                "kind": "the same pushes and watermark, then fw_list_drain and the split and cross product with numpy "
                        "on the host (what a join job has to do without the stage), 1 thread"}
    line = {
        "metric": "input records/sec, keyed window join (both inputs), 1 GPU", "value": round(n_in / dt, 1),
        "unit": "records/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "dtype": "int64",
        "data": "synthetic (splitmix64 counter stream)", "informational": True,
        "pairs_per_s": round(pairs / dt, 1), "pairs_per_input_record": round(pairs / max(n_in, 1), 3),
        "config": {"workload": f"window join, tumbling {args.window} ms, {args.keys} uniform Long keys, 2 x {args.batch} "
                               "records per step, pairs materialised in HBM and discarded",
                   "fired_rows": rows, "fired_elements": elems, "pairs": pairs},
        "join_stage": {"split_count_ms_per_step": round(t_split / args.steps * 1e3, 3),
                       "emit_ms_per_step": round(t_emit / args.steps * 1e3, 3),
                       "emit_store_bytes_per_s": round(40 * pairs / t_emit, 1) if t_emit else None,
                       "emit_store_over_copy_rate": round(40 * pairs / t_emit / COPY_RATE, 4) if t_emit else None,
                       "basis": "40 B per pair / (fw_list_join_device wall time with the split done, launch and "
                                "synchronisation included); copy rate 6.3 TB/s (DESIGN.md §4)"},
        "host_baseline": host,
    }
    print(json.dumps(line), flush=True)
    j.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Benchmark of the Table API time-windowed (interval) join (flink_amd.timejoin.TimeBoundedJoin;
fw_tjoin_push_batch_device, fw_tjoin_advance_watermark) on one MI355X.  Device-resident splitmix64 stream (the
generator of bench.py): a row's side is the low bit of its value, bounded out-of-orderness 200 ms, a punctuated
watermark max ts - 200 after every batch; a step pushes one tagged batch, advances the watermark and discards the
emitted rows, which stay in HBM (the sink).

Legs, one JSON line each, every leg in a child process of its own under its own time limit (a leg that fails or runs
out of time ends the run; the legs after it are not started):
  inner_1, full_1     1M uniform keys, 1e8 rows per event-second, bounds (-10, 9): about 1 partner per row
  inner_8, full_8     the same stream, bounds (-80, 79): about 8 partners per row
  zipf_inner          Zipf(1.1) over 1M keys, 1e6 rows per event-second, bounds (0, 0): the hottest key holds 7 % of
                      the rows and most of the pairs
  single_key_65536    one key, 65536 rows a step, two rows per ms, bounds (-4, 3)
  window_join         for orientation only: the tumbling window join (GpuWindowJoin, 20 ms windows) on inner_1's two
                      streams; it loses the pairs that straddle a window edge
  restatement         for orientation only: tests/timejoin_ref.py (sequential Python) on a 2^16-row slice of inner_1
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = ["inner_1", "full_1", "inner_8", "full_8", "zipf_inner", "single_key_65536", "window_join", "restatement"]
BOUNDS = {"1": (-10, 9), "8": (-80, 79)}


def make_inputs(args, leg, total):
    import torch
    from flink_amd.datagen import generate_device, zipf_cdf
    inputs, wms, m = [], [], -(1 << 63)
    single = leg.startswith("single_key")
    zipf = leg.startswith("zipf")
    batch = int(leg.rsplit("_", 1)[1]) if single else args.batch // 2 if zipf else args.batch
    cdf = torch.from_numpy(zipf_cdf(args.keys, 1.1)).cuda() if zipf else None
    for s in range(total):
        if single:
            i = torch.arange(s * batch, (s + 1) * batch, dtype=torch.int64, device="cuda")
            k, t, v = torch.full((batch,), 42, dtype=torch.int64, device="cuda"), i // 2 + 1, i * 2654435761 % 1000003
            side = (i & 1).to(torch.uint8)
            m = int(t[-1].item())
            wms.append(m)
        else:
            k, t, v, mx = generate_device(0x5EED, s * batch, batch, args.keys, ts_base=1000,
                                          rate=args.rate // 100 if zipf else args.rate, jitter=200, cdf_dev=cdf, device=0)
            side = (v & 1).to(torch.uint8)
            m = max(m, int(mx.item()))
            wms.append(m - 200)
        inputs.append((side, k, t, v))
    torch.cuda.synchronize()
    return inputs, wms, batch


def run_leg(args):
    import torch
    leg = args.leg
    total = args.warmup + args.steps
    line = {"metric": "input rows/sec, row-time interval join, 1 GPU", "leg": leg, "unit": "records/s", "n_gpus": 1,
            "steps": args.steps, "warmup": args.warmup, "higher_is_better": True, "informational": True}
    if leg == "restatement":
        from tests.timejoin_ref import TimeBoundedJoinRef
        inputs, wms, batch = make_inputs(args, "inner_1", 1)
        n = 1 << 16
        side, k, t, v = (x[:n].cpu().numpy() for x in inputs[0])
        ref = TimeBoundedJoinRef("inner", *BOUNDS["1"])
        t0 = time.perf_counter()
        rows = len(ref.push(side, k, t, v)) + len(ref.watermark(int(t.max()) - 200)[0])
        dt = time.perf_counter() - t0
        line.update(value=round(n / dt, 1), emitted_rows=rows, steps=1, warmup=0,
                    config={"what": "TimeBoundedJoinRef, INNER (-10, 9), one push of 2^16 rows and a watermark"})
        print(json.dumps(line), flush=True)
        return
    inputs, wms, batch = make_inputs(args, "inner_1" if leg == "window_join" else leg, total)
    if leg == "window_join":
        from flink_amd import TumblingEventTimeWindows
        from flink_amd.join import GpuWindowJoin
        split = [[tuple(x[side == sd].contiguous() for x in (k, t, v)) for sd in (0, 1)] for side, k, t, v in inputs]
        j = GpuWindowJoin(TumblingEventTimeWindows.of(20), max_batch=batch, expected_elements=int(batch * 3))

        def step(s):
            for sd in (0, 1):
                j.op.process_batch(*split[s][sd], side=sd)
            j.op.advance_watermark(wms[s])
            npairs = j.join_pending()[2]
            j.join_device()
            j.op.clear_pending()
            return npairs
        what, stats = "GpuWindowJoin, tumbling 20 ms windows, for orientation", None
    else:
        from flink_amd.timejoin import TimeBoundedJoin
        if leg.startswith("single_key"):
            jt, b, keys = "inner", (-4, 3), 1024
        elif leg.startswith("zipf"):
            jt, b, keys = "inner", (0, 0), int(args.keys * 1.25)
        else:
            jt, b, keys = leg.split("_")[0], BOUNDS[leg.split("_")[1]], int(args.keys * 1.25)
        op = TimeBoundedJoin(jt, b[0], b[1], expected_keys=keys, max_batch=batch)

        def step(s):
            op.process(*inputs[s])
            op.advance_watermark(wms[s])
            n = op.rows_device()[1]
            op.clear_pending()
            return n
        what = f"{jt.upper()} JOIN, l.rowtime BETWEEN r.rowtime + {b[0]} AND r.rowtime + {b[1]}"
        stats = op.stats
    for s in range(args.warmup):
        step(s)
    torch.cuda.synchronize()
    rows = 0
    t0 = time.perf_counter()
    for s in range(args.warmup, total):
        rows += step(s)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n_in = batch * args.steps
    line.update(value=round(n_in / dt, 1), emitted_rows_per_s=round(rows / dt, 1), emitted_rows=int(rows),
                ms_per_step=round(dt / args.steps * 1e3, 3), ns_per_row=round(dt / n_in * 1e9, 3),
                config={"join": what, "batch": batch, "keys": 1 if leg.startswith("single_key") else args.keys,
                        "bound_ms": 200})
    if stats:
        line["stats"] = stats()
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=6, help="6 batches of 2^22 are 250 ms of event time: the caches are full")
    ap.add_argument("--batch", type=int, default=1 << 22)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--rate", type=int, default=100_000_000)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--leg", default=None, help="(internal) run this one leg in this process")
    ap.add_argument("--leg-timeout", type=int, default=120, help="seconds per leg")
    args = ap.parse_args()
    if args.leg:
        run_leg(args)
        return 0
    for leg in args.legs.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--steps", str(args.steps), "--warmup",
               str(args.warmup), "--batch", str(args.batch), "--keys", str(args.keys), "--rate", str(args.rate)]
        try:
            rc = subprocess.run(cmd, timeout=args.leg_timeout).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"leg": leg, "error": f"no result within {args.leg_timeout} s"}), flush=True)
            return 124
        if rc != 0:
            print(json.dumps({"leg": leg, "error": f"exit status {rc}"}), flush=True)
            return rc if rc > 0 else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

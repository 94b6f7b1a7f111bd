#!/usr/bin/env python3
"""Benchmark of the row-time OVER windows (flink_amd.over.OverAggregate; fw_over_push_batch_device,
fw_over_advance_watermark) on one MI355X.  Device-resident C2-shaped stream (bench.py's preset: 1M uniform Long keys,
1e8 records per event-second, bounded out-of-orderness 200 ms, a punctuated watermark max ts - 200 after every batch),
select list SUM + MIN + COUNT over one Long column; a step pushes one batch, advances the watermark and discards the
emitted rows, which stay in HBM (the sink).

Legs, one JSON line each, every leg in a child process of its own under its own time limit (a leg that fails or
runs out of time ends the run; the legs after it are not started):
  rows, range, unbounded_rows, unbounded_range   the four kinds, ROWS 8 PRECEDING / RANGE 1 s PRECEDING
  count_window                                   for orientation only: countWindow(9, 1).sum on the same stream
                                                 (FW_COUNT), the nearest existing per-element output
  single_key_65536, single_key_262144            one constant key (the non-partitioned OVER), ROWS 8 PRECEDING, a step
                                                 = that many rows in row-time order; ns per row must not rise with
                                                 the run's length (linear work)
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = ["rows", "range", "unbounded_rows", "unbounded_range", "count_window", "single_key_65536", "single_key_262144"]
AGGS = [("sum", 0), ("min", 0), ("count", 0)]


def frame_of(leg):
    from flink_amd.over import Over
    return {"rows": lambda: Over.rows(8), "range": lambda: Over.range(1000), "unbounded_rows": Over.unbounded_rows,
            "unbounded_range": Over.unbounded_range}[leg]()


def run_leg(args):
    import torch
    from flink_amd.datagen import generate_device
    from flink_amd.over import Over, OverAggregate
    leg = args.leg
    total = args.warmup + args.steps
    single = leg.startswith("single_key")
    batch = int(leg.rsplit("_", 1)[1]) if single else args.batch
    inputs, wms, m = [], [], -(1 << 63)
    for s in range(total):
        if single:
            t = torch.arange(s * batch, (s + 1) * batch, dtype=torch.int64, device="cuda") // 2 + 1
            k = torch.full((batch,), 42, dtype=torch.int64, device="cuda")
            v = (t * 2654435761) % 1000003
            m = int(t[-1].item())
            wms.append(m)
        else:
            k, t, v, mx = generate_device(0x5EED, s * batch, batch, args.keys, ts_base=1, rate=args.rate, jitter=200,
                                          device=0)
            m = max(m, int(mx.item()))
            wms.append(m - 200)
        inputs.append((k, t, v))
    torch.cuda.synchronize()
    rows = 0
    if leg == "count_window":
        from flink_amd import CountWindows
        from flink_amd.operator import GpuWindowOperator
        from flink_amd.windowing import FirstElementReduce
        op = GpuWindowOperator(CountWindows.of(9, 1), FirstElementReduce("long", "sum"), device=0,
                               expected_entries=int(args.keys * 1.25), max_batch=batch)

        def step(s):
            k, t, v = inputs[s]
            op.process_batch(k, t, v)
            n = op.advance_watermark(0)
            op.clear_pending()
            return n
        what = "countWindow(9, 1).sum (FW_COUNT), for orientation"
    else:
        op = OverAggregate(Over.rows(8) if single else frame_of(leg), ["long"], AGGS,
                           expected_keys=1024 if single else int(args.keys * 1.25), max_batch=batch)

        def step(s):
            k, t, v = inputs[s]
            op.process(k, t, v.unsqueeze(0))
            n = op.advance_watermark(wms[s])
            op.clear_pending()
            return n
        what = ("one key, ROWS BETWEEN 8 PRECEDING AND CURRENT ROW" if single else
                {"rows": "ROWS BETWEEN 8 PRECEDING AND CURRENT ROW", "range": "RANGE BETWEEN 1 s PRECEDING AND CURRENT ROW",
                 "unbounded_rows": "ROWS UNBOUNDED PRECEDING", "unbounded_range": "RANGE UNBOUNDED PRECEDING"}[leg])
    for s in range(args.warmup):
        step(s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(args.warmup, total):
        rows += step(s)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n_in = batch * args.steps
    line = {"metric": "input rows/sec, row-time OVER window, 1 GPU", "leg": leg, "value": round(n_in / dt, 1),
            "unit": "records/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3), "ns_per_row": round(dt / n_in * 1e9, 3),
            "higher_is_better": True, "informational": True, "emitted_rows": int(rows),
            "data": "synthetic (splitmix64 counter stream)" if not single else "one key, two rows per row time",
            "config": {"frame": what, "select": "SUM, MIN, COUNT of one Long column", "batch": batch,
                       "keys": 1 if single else args.keys, "rate": None if single else args.rate, "bound_ms": 200}}
    if leg != "count_window":
        line["stats"] = op.stats()
    print(json.dumps(line), flush=True)
    op.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=7, help="7 batches of 2^24 are 1.17 s of event time: RANGE 1 s is full")
    ap.add_argument("--batch", type=int, default=1 << 24)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--rate", type=int, default=100_000_000)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--leg", default=None, help="(internal) run this one leg in this process")
    ap.add_argument("--leg-timeout", type=int, default=150, help="seconds per leg")
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

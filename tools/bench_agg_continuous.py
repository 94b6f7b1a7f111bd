#!/usr/bin/env python3
"""ContinuousEventTimeTrigger on the aggregating operator against the window-contents operator under the same trigger,
on the C2-shaped stream: tumbling 1 s windows, 1M uniform Long keys, 2^24 records per step generated in HBM, one
watermark per step, ContinuousEventTimeTrigger.of(250 ms).  Two legs in one job, one after the other: this operator
(GpuWindowOperator), then tools/bench_list.py --trigger continuous --interval 250 in a fresh child process (the list
operator keeps every element, 28 B each, and walks a window's list at every firing).  Prints one JSON line: records/s,
fired rows per step and ms per step of both legs, and their ratio.

    python tools/bench_agg_continuous.py [--steps 12 --warmup 6 --interval 250] [--no-list-leg]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--batch", type=int, default=1 << 24)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--rate", type=int, default=100_000_000)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--interval", type=int, default=250)
    ap.add_argument("--no-list-leg", action="store_true")
    args = ap.parse_args()

    import torch
    from flink_amd import ContinuousEventTimeTrigger, TumblingEventTimeWindows
    from flink_amd.datagen import generate_device
    from flink_amd.operator import GpuWindowOperator

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    op = GpuWindowOperator(TumblingEventTimeWindows.of(args.window),
                           trigger=ContinuousEventTimeTrigger.of(args.interval), max_batch=args.batch,
                           expected_entries=2 * args.keys)
    batches, wms, m = [], [], -(1 << 63)
    for s in range(args.warmup + args.steps):
        k, t, v, mx = generate_device(0x5EED, s * args.batch, args.batch, args.keys, ts_base=0, rate=args.rate,
                                      jitter=200, device=0)
        batches.append((k, t, v))
        m = max(m, int(mx.item()))
        wms.append(m - 200)
    torch.cuda.synchronize()
    fired = 0

    def step(s):
        nonlocal fired
        op.process_batch(*batches[s])
        fired += op.advance_watermark(wms[s])
        op.clear_pending()  # discarding sink: the fired rows were materialised in HBM

    for s in range(args.warmup):
        step(s)
    fired = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(args.warmup, args.warmup + args.steps):
        step(s)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = op.stats()
    op.close()
    agg = {"records_per_s": round(args.steps * args.batch / dt, 1), "ms_per_step": round(dt / args.steps * 1e3, 4),
           "fired_rows_per_step": round(fired / args.steps, 1), "table_grows": st["table_grows"],
           "push_resumptions": st["push_resumptions"]}
    lst = None
    if not args.no_list_leg:
        del batches
        torch.cuda.empty_cache()
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_list.py"), "--trigger", "continuous",
                              "--interval", str(args.interval), "--steps", str(args.steps), "--warmup",
                              str(args.warmup), "--batch", str(args.batch), "--keys", str(args.keys), "--rate",
                              str(args.rate), "--window", str(args.window)], capture_output=True, text=True, check=True)
        j = json.loads(out.stdout.strip().splitlines()[-1])
        lst = {"records_per_s": j["value"], "ms_per_step": j["ms_per_step"],
               "fired_rows_per_step": round(j["config"]["fired_rows"] / args.steps, 1)}
    line = {"metric": "records/sec, ContinuousEventTimeTrigger on the C2-shaped stream, 1 GPU",
            "value": agg["records_per_s"], "unit": "records/s", "higher_is_better": True, "steps": args.steps,
            "warmup": args.warmup,
            "config": {"workload": f"tumbling {args.window} ms, ContinuousEventTimeTrigger({args.interval} ms), "
                                   f"{args.keys} uniform Long keys, {args.rate} records per event-second, "
                                   f"{args.batch} per step"},
            "aggregate_leg": agg, "list_leg": lst,
            "aggregate_over_list": round(agg["records_per_s"] / lst["records_per_s"], 3) if lst else None}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""CountTrigger on the aggregating operator against the window-contents operator under the same trigger, on the
C2-shaped stream: tumbling 1 s windows, 1M uniform Long keys, 2^24 records per step generated in HBM, one watermark per
step, CountTrigger.of(4), optionally inside PurgingTrigger.  Both legs alternate twice in one job (A, B, A, B), each run
in a fresh child process: A = this operator (GpuWindowOperator over fw_create_count_trigger), B = tools/bench_list.py
--trigger count:N (the list operator keeps every element, 28 B each, and walks a window's whole list at every firing).
Prints one JSON line: records/s, fired rows per step and ms per step of all four runs, the lower A over the higher B,
and whether A's lower run lies above B's higher one.  Every leg has a time limit of its own (--leg-timeout): a leg
that misses it ends the job, and the line then says which one and gives no ratio.

Without --purging the B legs are started only with --list-leg: there the list operator's push bounds its fired
elements by firings x list length per window (fw_list.hip k_walk_bound), about 4 x 100 x 10^6 in the later steps of a
window, above FW_LIST_ROOM = 2^28; beyond that bound its walk reserves every firing's elements with a compare-and-swap
loop on one counter (emit_firing), some 4 x 10^6 firings per step one after the other, and a leg takes many minutes
(DESIGN.md 3e).  Give such a run --leg-timeout accordingly.  With --purging the lists stay short and B runs as A does.

    python tools/bench_agg_count_trigger.py [--steps 12 --warmup 6 --count 4] [--purging | --list-leg]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def agg_leg(args):
    import torch
    from flink_amd import CountTrigger, PurgingTrigger, TumblingEventTimeWindows
    from flink_amd.datagen import generate_device
    from flink_amd.operator import GpuWindowOperator

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    trig = CountTrigger.of(args.count)
    op = GpuWindowOperator(TumblingEventTimeWindows.of(args.window),
                           trigger=PurgingTrigger.of(trig) if args.purging else trig, max_batch=args.batch,
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
        fired += op.advance_watermark(wms[s])  # (the rows of the push: the watermark itself fires none)
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
    print(json.dumps({"records_per_s": round(args.steps * args.batch / dt, 1),
                      "ms_per_step": round(dt / args.steps * 1e3, 4),
                      "fired_rows_per_step": round(fired / args.steps, 1), "table_grows": st["table_grows"]}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--batch", type=int, default=1 << 24)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--rate", type=int, default=100_000_000)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--count", type=int, default=4)
    ap.add_argument("--purging", action="store_true")
    ap.add_argument("--list-leg", action="store_true",
                    help="without --purging: also run the list operator's legs (minutes each, see above)")
    ap.add_argument("--leg-timeout", type=int, default=180, help="seconds one leg's child process may take")
    ap.add_argument("--leg", default="", help="agg: run this operator's leg alone (what the job starts as a child)")
    args = ap.parse_args()
    if args.leg == "agg":
        agg_leg(args)
        return 0
    common = ["--steps", str(args.steps), "--warmup", str(args.warmup), "--batch", str(args.batch), "--keys",
              str(args.keys), "--rate", str(args.rate), "--window", str(args.window)]
    purge = ["--purging"] if args.purging else []

    def child(cmd):
        return subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=args.leg_timeout)

    def run_agg():
        out = child([sys.executable, os.path.abspath(__file__), "--leg", "agg", "--count", str(args.count)] + common +
                    purge)
        return json.loads(out.stdout.strip().splitlines()[-1])

    def run_list():
        out = child([sys.executable, os.path.join(ROOT, "tools", "bench_list.py"), "--trigger", f"count:{args.count}",
                     "--no-cpu-baseline"] + common + purge)
        j = json.loads(out.stdout.strip().splitlines()[-1])
        return {"records_per_s": j["value"], "ms_per_step": j["ms_per_step"],
                "fired_rows_per_step": round(j["config"]["fired_rows"] / args.steps, 1)}

    runs = []
    with_list = args.purging or args.list_leg
    for name, leg in (("aggregate", run_agg), ("list", run_list), ("aggregate", run_agg), ("list", run_list)):
        if name == "list" and not with_list:
            continue
        try:
            runs.append((name, leg()))
        except subprocess.TimeoutExpired:
            # a leg that does not finish ends the job: nothing more is started on the GPU, no ratio is claimed
            print(json.dumps({"metric": "records/sec, CountTrigger on the C2-shaped stream, 1 GPU", "value": None,
                              "runs": [{"leg": n, **r} for n, r in runs],
                              "unfinished": f"the {name} leg did not finish within {args.leg_timeout} s"}), flush=True)
            return 1
    a = [r["records_per_s"] for n, r in runs if n == "aggregate"]
    b = [r["records_per_s"] for n, r in runs if n == "list"]
    if not b:  # this operator's legs alone: no ratio
        print(json.dumps({"metric": "records/sec, CountTrigger on the C2-shaped stream, 1 GPU", "value": min(a),
                          "unit": "records/s", "steps": args.steps, "warmup": args.warmup,
                          "runs": [{"leg": n, **r} for n, r in runs],
                          "list_leg": "not run (--list-leg)"}), flush=True)
        return 0
    line = {"metric": "records/sec, CountTrigger on the C2-shaped stream, 1 GPU", "value": min(a),
            "unit": "records/s", "higher_is_better": True, "steps": args.steps, "warmup": args.warmup,
            "config": {"workload": f"tumbling {args.window} ms, {'PurgingTrigger(' if args.purging else ''}"
                                   f"CountTrigger({args.count}){')' if args.purging else ''}, {args.keys} uniform Long "
                                   f"keys, {args.rate} records per event-second, {args.batch} per step"},
            "runs": [{"leg": n, **r} for n, r in runs],
            "aggregate_lower_over_list_higher": round(min(a) / max(b), 3),
            "aggregate_lower_above_list_higher": min(a) > max(b)}
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

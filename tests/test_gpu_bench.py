"""bench.py end to end on the GPU at a tiny size: a plain run times its steps and prints the line without the legs
that take runs of their own, `--dump-outputs` writes what the timed path computed (checked against numpy over the
same counter-based stream), and `--full` brings the other legs back."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from flink_amd.datagen import generate_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
B, KEYS, STEPS, WARMUP = 1 << 16, 1000, 3, 1
# 10 ms of event time per step and no jitter: step s holds exactly the records of window [10 s, 10 s + 10); with a
# 5 ms bound the watermark after step s is 10 s + 4, which fires step s - 1's window and leaves step s's live
SHAPE = ["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--batch", str(B), "--keys", str(KEYS),
         "--rate", str(B * 100), "--window", "10", "--bound", "5", "--jitter", "0"]
FIELDS = ("key", "start", "end", "count", "sum", "min", "max")


def run(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH] + SHAPE + args, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def expected_rows(step):
    """count/sum/min/max per key of step `step`'s batch (one window), sorted by key"""
    k, t, v = generate_host(0x5EED, step * B, B, KEYS, ts_base=0, rate=B * 100, jitter=0)
    assert t.min() == 10 * step and t.max() == 10 * step + 9
    keys, inv, cnt = np.unique(k, return_inverse=True, return_counts=True)
    s = np.zeros(len(keys), dtype=np.int64)
    np.add.at(s, inv, v)
    mn = np.full(len(keys), np.iinfo(np.int64).max)
    np.minimum.at(mn, inv, v)
    mx = np.full(len(keys), np.iinfo(np.int64).min)
    np.maximum.at(mx, inv, v)
    n = len(keys)
    return {"key": keys, "start": np.full(n, 10 * step), "end": np.full(n, 10 * step + 10), "count": cnt, "sum": s,
            "min": mn, "max": mx}


@pytest.mark.gpu
@pytest.mark.parametrize("stage", [[], ["--stage-gib", "0.002"]], ids=["one-chunk", "chunks-of-1"])
def test_plain_run_is_lean_and_dumps_what_the_timed_path_computed(tmp_path, stage):
    # a batch is 1.5 MiB: 0.002 GiB stage one step at a time, the clock stopped between them; the results are the same
    out = tmp_path / "dump"
    d = run(["--dump-outputs", str(out)] + stage)
    assert d["steps"] == STEPS and d["n_gpus"] == 1 and d["unit"] == "records/s" and d["higher_is_better"] is True
    assert d["dtype"] == "int64" and d["metric"].startswith("records/sec keyed windowed aggregation")
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(B / (d["ms_per_step"] * 1e-3), rel=1e-2)  # (ms_per_step is rounded to 1e-4 ms)
    assert d["cpu_baseline"] is None and d["host_fed"] is None and "kernels_isolated" not in d
    assert d["path_roofline"]["fired_rows"] > 0
    last = WARMUP + STEPS - 1
    total = 0
    for name, step in (("fired", last - 1), ("final", last)):
        exp = expected_rows(step)
        for f in FIELDS:
            path = out / f"{name}_{f}.npy"
            got = np.load(path)
            total += os.path.getsize(path)
            assert got.dtype == np.float64
            assert np.array_equal(got, exp[f].astype(np.float64)), (name, f)
        assert d["outputs"][name] == {"rows": len(exp["key"]), "rows_written": len(exp["key"])}
    assert sorted(p.name for p in out.iterdir()) == sorted(f"{n}_{f}.npy" for n in ("fired", "final") for f in FIELDS)
    assert total < 64 * 1000 * 1000


@pytest.mark.gpu
def test_full_run_brings_the_other_legs():
    d = run(["--full", "--cpu-sample", str(4 * B), "--stage-gib", "0.004"])  # (chunks of 2 steps)
    assert d["steps"] == STEPS and d["ms_per_step"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["kind"] == "port"
    assert d["host_fed"]["value"] > 0 and d["host_fed"]["fired_rows"] > 0
    assert d["kernels_isolated"] and d["roofline"]["isolated"]["avg_ms"] > 0
    assert "outputs" not in d


def test_dump_outputs_sample_is_fixed_and_within_budget(tmp_path, monkeypatch):
    """CPU: a group over its share of the budget keeps the same rows whatever order the table gave them in."""
    import importlib.util
    from flink_amd.operator import ROW_DTYPE
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(mod, "DUMP_BUDGET", 64_000)
    rng = np.random.default_rng(7)
    rows = np.zeros(5000, dtype=ROW_DTYPE)
    rows["key"] = np.repeat(np.arange(2500), 2)
    rows["start"] = np.tile([0, 10], 2500)
    rows["sum"] = rng.integers(-1 << 40, 1 << 40, 5000)
    rows["max"] = rng.integers(-1 << 63, (1 << 63) - 1, 5000)
    a, b = tmp_path / "a", tmp_path / "b"
    ia = mod.dump_outputs(str(a), {"final": rows}, (), ("max",), 0, 1)
    ib = mod.dump_outputs(str(b), {"final": rows[rng.permutation(5000)]}, (), ("max",), 0, 1)
    assert ia == ib and 0 < ia["final"]["rows_written"] < ia["final"]["rows"] == 5000
    names = sorted(p.name for p in a.iterdir())
    assert names == sorted(p.name for p in b.iterdir()) and "final_max_hi.npy" in names and "final_max_lo.npy" in names
    assert sum(np.load(a / n).nbytes for n in names) <= 64_000
    for n in names:
        assert np.load(a / n).dtype == np.float64 and np.array_equal(np.load(a / n), np.load(b / n)), n
    key, start = np.load(a / "final_key.npy"), np.load(a / "final_start.npy")
    assert np.array_equal(np.lexsort((start, key)), np.arange(len(key)))
    pick = (2 * key + start // 10).astype(np.int64)  # rows[] holds (key, start) in this order
    hi, lo = np.load(a / "final_max_hi.npy"), np.load(a / "final_max_lo.npy")
    assert np.array_equal(hi.astype(np.int64) * (1 << 32) + lo.astype(np.int64), rows["max"][pick])

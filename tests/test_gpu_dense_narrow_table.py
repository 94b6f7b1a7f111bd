"""The narrow-keyed LDS table of the dense aggregate (k_dn_aggregate, fw_device.hip): the first launch of a narrow
single-pass batch.  Integers bit-exact against the oracle; push_resumptions tells whether that launch committed every
region (0) or left some to the resumed sequence's kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from flink_amd import KeyGroupRange, TumblingEventTimeWindows  # noqa: E402
from flink_amd.datagen import generate_host  # noqa: E402
from flink_amd.keygroups import assign_to_key_group, long_hash_code  # noqa: E402
from flink_amd.windowing import CountSumMinMax  # noqa: E402
from tests.parity_util import assert_rows_equal  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_WM = (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
KG = 77  # the key group of the tests that keep one key group in four regions (sub_partitions=4: compact records need
#          two bits of sub-partition, so this is the smallest P), whose runs may then hold 2^16 records and more


def _op(size, **kw):
    from flink_amd.operator import GpuWindowOperator
    return GpuWindowOperator(TumblingEventTimeWindows.of(size), CountSumMinMax("long"), **kw)


def _oracle(size, steps):
    from oracle import oracle as orc
    ref = orc.WindowOperatorOracle(assigner="tumbling", size=size)
    for k, t, v, wm in steps:
        if k is not None:
            ref.process(k, t, v)
        ref.watermark(wm)
    return ref.rows()


def _drive(op, steps, device=False):
    """steps: (keys, ts, values, watermark), keys None = the watermark alone.  device: async device pushes."""
    drained = []
    for e, (k, t, v, wm) in enumerate(steps):
        if device:
            import torch
            if k is not None:
                op.process_batch(*(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (k, t, v)))
            op.advance_watermark(wm, wait=False)
            drained.append(op.drain_rows(e))
        else:
            if k is not None:
                op.process(k, t, v)
            op.watermark(wm)
    return np.concatenate(drained) if device else op.rows()


# ---------------------------------------------------------------- the stream every region of which the kernel takes
def _all_regions_steps():
    """Tumbling 100, 50K keys, 8 batches of 75K records at 1000 records per time unit: a batch spans 75 units, so the
    batches cover windows opening (batch 0, after a first watermark: every claim comes from a record), steady batches
    and batches that straddle a window end.  Batch 1 carries values at both int32 bounds and the keys -2^28 and
    2^28 - 1."""
    n, b = 600_000, 75_000
    keys, ts, vals = generate_host(0x5EED, 0, n, 50_000, ts_base=1_000_000, rate=1_000_000, jitter=30)
    keys, vals = keys.copy(), vals.copy()
    vals[b + 5], vals[b + 6], vals[b + 7] = I32_MIN, I32_MAX, 0
    keys[b + 8], keys[b + 9] = -(1 << 28), (1 << 28) - 1
    steps, mx = [(None, None, None, int(ts[:b].min()) - 1)], -(1 << 63)
    for s in range(0, n, b):
        sl = slice(s, s + b)
        mx = max(mx, int(ts[sl].max()))
        steps.append((keys[sl], ts[sl], vals[sl], mx - 20))
    steps.append((None, None, None, MAX_WM))
    return steps


_REF = {}


def _all_regions_ref():
    if "rows" not in _REF:
        _REF["steps"] = _all_regions_steps()
        _REF["rows"] = _oracle(100, _REF["steps"])
    return _REF["steps"], _REF["rows"]


@pytest.mark.parametrize("device", [False, True], ids=["host-push", "async-device-push"])
def test_gpu_dn_takes_every_region(device):
    steps, r = _all_regions_ref()
    op = _op(100, max_batch=1 << 17, async_input=device)
    g = _drive(op, steps, device)
    st = op.stats()
    op.close()
    assert_rows_equal(g, r)
    assert int(g["max"].max()) == I32_MAX and int(g["min"].min()) == I32_MIN
    assert {-(1 << 28), (1 << 28) - 1} <= set(g["key"].tolist())
    # every batch was narrow and the first launch committed every region: nothing was resumed
    assert st["narrow_pass_batches"] >= 6 and st["narrow_pass_redone"] == 0
    assert st["push_resumptions"] == 0


def test_gpu_dn_env_knob_same_rows(tmp_path):
    # FW_NO_DN=1 (read once by the library: a fresh child) puts the compact table's kernel first again
    steps, r = _all_regions_ref()
    out = tmp_path / "rows.npy"
    env = dict(os.environ, FW_NO_DN="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-4000:]
    g = np.load(out)
    assert_rows_equal(g, r)
    op = _op(100, max_batch=1 << 17)
    here = _drive(op, steps)
    op.close()
    from tests.parity_util import _sorted
    assert np.array_equal(_sorted(g), _sorted(here))


# ---------------------------------------------------------------- the packed accumulator's fields
def test_gpu_dn_bias_and_carry():
    # one key, so one region's run; 65535 records (the longest run the packed accumulator takes), all -2^31 in one
    # batch and all 2^31 - 1 in the next: the count field is full, the biased sum is 0 in the first batch and at its
    # maximum 65535 (2^32 - 1) in the second.  (One key group in four regions: a region's run may then hold the batch.)
    n, size = 65535, 1_000_000
    key = next(x for x in range(1, 10_000) if assign_to_key_group(long_hash_code(x), 128) == KG)
    k = np.full(n, key, dtype=np.int64)
    t = size + 1000 + np.arange(n, dtype=np.int64) % 1000
    lo, hi = np.full(n, I32_MIN, dtype=np.int64), np.full(n, I32_MAX, dtype=np.int64)
    steps = [(None, None, None, size + 10), (k, t, lo, size + 20), (k, t, hi, size + 30), (None, None, None, MAX_WM)]
    op = _op(size, max_batch=1 << 16, key_group_range=KeyGroupRange(KG, KG), sub_partitions=4)
    g = _drive(op, steps)
    st = op.stats()
    op.close()
    assert_rows_equal(g, _oracle(size, steps))
    assert len(g) == 1 and g["count"][0] == 2 * n and g["sum"][0] == -n
    assert g["min"][0] == I32_MIN and g["max"][0] == I32_MAX
    assert st["narrow_pass_batches"] == 2 and st["push_resumptions"] == 0


# ---------------------------------------------------------------- refusals
def test_gpu_dn_run_length_refusal_and_sticky_switch():
    # One key group and sub_partitions=4 (P = 4 regions, the fewest that take compact records).  A key's records all
    # land in one region, so a key with 70000 of a batch's 2^17 records puts more than 65535 into its region's run,
    # whatever the other keys' regions are (counted below), and the kernel refuses that region.  Every such push is
    # resumed once; after three in a row the compact table's kernel leads again.
    kg, size, n = KG, 1_000_000, 1 << 17
    cand = np.arange(1, 40_000, dtype=np.int64)
    keys = np.array([x for x in cand if assign_to_key_group(long_hash_code(int(x)), 128) == kg][:300], dtype=np.int64)
    assert len(keys) >= 200
    rng = np.random.default_rng(7)
    steps = [(None, None, None, size + 10)]
    for b in range(5):
        k = keys[rng.integers(0, len(keys), n)]
        k[rng.permutation(n)[:70_000]] = keys[0]
        assert int((k == keys[0]).sum()) >= 65536
        t = size + 100 + rng.integers(0, 1000, n).astype(np.int64)
        v = rng.integers(I32_MIN, I32_MAX, n, endpoint=True).astype(np.int64)
        steps.append((k, t, v, size + 20 + b))
    steps.append((None, None, None, MAX_WM))
    op = _op(size, max_batch=n, key_group_range=KeyGroupRange(kg, kg), sub_partitions=4)
    g = _drive(op, steps)
    st = op.stats()
    op.close()
    assert_rows_equal(g, _oracle(size, steps))
    assert st["narrow_pass_batches"] == 5 and st["narrow_pass_redone"] == 0
    assert st["push_resumptions"] == 3


def test_gpu_dn_entry_without_narrow_form():
    # restored entries whose min / max lie outside int32 (their batch was not narrow), then narrow batches onto the
    # same keys: the regions that hold such an entry are refused and taken by the resumed sequence
    steps, r = _all_regions_ref()
    k0, t0, v0, wm0 = steps[1]
    v0 = v0.copy()
    newest = np.argsort(t0)[-2:]  # (their windows end after the watermark: live in the snapshot)
    v0[newest[0]], v0[newest[1]] = 1 << 40, -(1 << 40)
    steps = [steps[0], (k0, t0, v0, wm0)] + steps[2:]
    a = _op(100, max_batch=1 << 17)
    first = _drive(a, steps[:2])
    snap = a.snapshot_state()
    a.close()
    live = np.concatenate([x for x in snap.values() if len(x)])
    assert (live["max"] > I32_MAX).any() and (live["min"] < I32_MIN).any()
    b = _op(100, max_batch=1 << 17)
    b.initialize_state(snap)
    before = b.stats()["push_resumptions"]
    rest = _drive(b, [(None, None, None, steps[0][3]), (None, None, None, wm0)] + steps[2:])
    st = b.stats()
    b.close()
    assert_rows_equal(np.concatenate([first, rest]), _oracle(100, steps))
    assert st["narrow_pass_batches"] >= 1
    assert st["push_resumptions"] - before >= 1


if __name__ == "__main__":  # the FW_NO_DN child: <out> (the all-regions stream), or <out.npz> <dn_util stream> ...
    if len(sys.argv) > 2:  # (tests/test_gpu_dn_edges.py: every named stream's rows and whole push_resumptions)
        from tests import dn_util
        from tests.test_gpu_dn_edges import run_stream
        res = {}
        for name in sys.argv[2:]:
            rows_, _, _, total_ = run_stream(dn_util.stream(name))
            res[name], res[name + ".resumptions"] = rows_, np.int64(total_)
        np.savez(sys.argv[1], **res)
    else:
        _op_ = _op(100, max_batch=1 << 17)
        np.save(sys.argv[1], _drive(_op_, _all_regions_steps()))
        _op_.close()

"""bench.py --dump-outputs: what the last timed step returned, as float64 .npy files of bounded size, on one rank and
gathered over several; a plain run (no --full) prints the headline line without the legs that take runs of their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

FULL_ONLY = ("pipelined", "warm_start", "batch_sweep", "seeds", "wbc_qp", "cpu_baseline")


def _step_output(B, nsol, cols=55, seed=0):
    g = torch.Generator().manual_seed(seed)
    XU = torch.rand((B, nsol), generator=g, dtype=torch.float64)
    full = torch.rand((B, cols), generator=g, dtype=torch.float64)
    return XU, full


def test_dump_one_rank_writes_every_array_as_float64(tmp_path):
    B, nsol = 300, 1060
    XU, full = _step_output(B, nsol)
    arrays = bench.dump_outputs(str(tmp_path), full, XU, np.arange(B), B)
    names = {"x1_u0", "kkt", "status", "iterations", "instances", "solution", "solution_instances"}
    assert {f[:-4] for f in os.listdir(tmp_path)} == names
    for name in names:
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, arrays[name])
    assert np.array_equal(np.load(tmp_path / "x1_u0.npy"), full[:, :-3].numpy())
    assert np.array_equal(np.load(tmp_path / "status.npy"), full[:, -2].numpy())
    assert np.array_equal(np.load(tmp_path / "solution.npy"), XU.numpy())             # small batch: every instance


def test_dump_sample_is_fixed_and_bounded(tmp_path):
    B, nsol = 65536, 1060
    a, b = bench.dump_sample(B, nsol), bench.dump_sample(B, nsol)
    assert np.array_equal(a, b) and np.all(np.diff(a) > 0) and a[-1] < B
    assert a.shape[0] * nsol * 8 <= bench.DUMP_SOLUTION_BYTES
    XU, full = _step_output(B, 64)
    bench.dump_outputs(str(tmp_path), full, XU, np.arange(B), B)
    total = sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path))
    assert total <= 64 << 20
    inst = np.load(tmp_path / "instances.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "kkt.npy"), full[inst, -3].numpy())
    rows = np.load(tmp_path / "solution_instances.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "solution.npy"), XU[rows].numpy())


def test_dump_over_dealt_ranks_matches_one_rank(tmp_path):
    """Each rank holds the solution rows of its deal (a permutation); the sum over the ranks rebuilds the sample."""
    B, nsol, world = 5000, 1060, 3
    XU, full = _step_output(B, nsol)
    order = np.random.default_rng(1).permutation(B)
    parts = []
    for r in range(world):
        rows = order[r::world]
        bench.dump_outputs(None, full, XU[rows], rows, B, reduce_sum=lambda t: parts.append(t.clone()))
    total = sum(parts)
    sample = bench.dump_sample(B, nsol)
    assert np.array_equal(total.numpy(), XU[sample].numpy())


@pytest.mark.gpu
def test_plain_bench_run_is_lean_and_dumps_the_same_outputs_twice(tmp_path):
    def run(d):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--batch", "256", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        return json.loads(lines[0])
    a, b = run(tmp_path / "a"), run(tmp_path / "b")
    for d in (a, b):
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["roofline"]["kernel_launches_timed"] == 3
        assert d["unit"] == "solves/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert not any(k in d for k in FULL_ONLY)
    st = np.load(tmp_path / "a" / "status.npy")
    assert st.shape == (256,) and np.isin(st, (0, 1, 2, 3)).all()
    assert np.load(tmp_path / "a" / "solution.npy").shape[0] == 256
    for name in sorted(os.listdir(tmp_path / "a")):                          # same inputs, same computation, same bits
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name), equal_nan=True), name

"""GPU tier: the Newton step applied where the next matrix sweep loads the iterate (the one-wave 4-vertex kernel,
Solver::STEP_FUSED in csrc/cmpc_kernel.hpp) against the step applied in a pass of its own.  The pair kernel keeps that pass
(apply_step) and is bit for bit the one-wave kernel by tests/test_gpu_parity.py, so the one-wave handle (spec.kernel = 1) is
compared with the pair handle (spec.kernel = 2): XU, status, iterations, KKT error and the solver state, every bit.

Cases: B = 48 `randomized` at N = 20 (retried factorisations: stages visited twice in an iteration) and the rows of a larger
draw that end with status 2 (the regularisation exhausted, the step collapsed), N = 1 and N = 3 (the first and the terminal node next to each other), a solve resumed from `state_out`
(a failed resumed attempt is followed by a plain one whose first iteration has no step), a primal warm start, max_iter = 3
(the last sweep applies the last step and the iterate it leaves is what is returned)."""
import dataclasses

import numpy as np
import pytest
import torch

from cmpc_amd import workloads as wl

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 48


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _handles(spec):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device: the HIP extension must run, there is no fallback")
    from cmpc_amd.solver import BatchedCentroidalMPC
    return tuple(BatchedCentroidalMPC(dataclasses.replace(spec, kernel=k), device=DEV) for k in (1, 2))


def _solve(s, want, rec, warm=None, state=None):
    so = s.new_state(rec.shape[0])
    r = s.solve(_t(rec), warm=_t(warm), state=_t(state), state_out=so)
    torch.cuda.synchronize()
    assert s.last_kernel_name() == want, s.last_kernel_name()
    return tuple(x.cpu().numpy() for x in r) + (so.cpu().numpy(),)


def _pair_of_solves(spec, rec, **kw):
    one, pair = _handles(spec)
    try:
        a = _solve(one, "cmpc_solve_kernel<4, 1>", rec, **kw)
        b = _solve(pair, "cmpc_solve_pair_kernel<4, 2>", rec, **kw)
    finally:
        one.close()
        pair.close()
    return a, b


def _same(a, b, label):
    for name, x, y in zip(("XU", "status", "iters", "kkt", "state"), a, b):
        assert np.array_equal(x, y, equal_nan=True), (label, name)


@pytest.fixture(scope="module")
def cold():
    spec, rec = wl.make_workload("randomized", B=B)
    assert spec.N == 20 and spec.nv == 4
    return spec, rec, _pair_of_solves(spec, rec)


def test_randomized_batch_with_retries_and_status_2(cold):
    _, _, (a, b) = cold
    print("status counts", np.bincount(a[1], minlength=4).tolist(), "iterations", int(a[2].sum()))
    assert np.isin(a[1], (0, 3)).mean() > 0.5
    _same(a, b, "randomized")


NO_POINT = [21, 26, 46, 56, 57, 80]          # rows of a draw of 256 that the C oracle ends with status 2 (46, 57, 80: after retries)


def test_instances_that_end_without_a_usable_point():
    spec, rec = wl.make_workload("randomized", B=256)
    a, b = _pair_of_solves(spec, rec[NO_POINT])
    print("status", a[1].tolist(), "iterations", a[2].tolist())
    assert (a[1] == 2).any()
    _same(a, b, "status 2")


@pytest.mark.parametrize("N", [1, 3])
def test_short_horizons(N):
    spec, rec = wl.make_workload("randomized", B=B, N=N, seed=2)
    a, b = _pair_of_solves(spec, rec)
    assert np.isin(a[1], (0, 3)).mean() > 0.5
    _same(a, b, f"N = {N}")


def test_resumed_from_state_out(cold):
    spec, _, (first, _) = cold
    _, rec2 = wl.make_workload("randomized", B=B, seed=777)
    a, b = _pair_of_solves(spec, rec2, state=first[4])
    print("resumed: status counts", np.bincount(a[1], minlength=4).tolist(), "iterations", int(a[2].sum()))
    _same(a, b, "resumed")


def test_primal_warm_start(cold):
    spec, rec, (first, _) = cold
    warm = np.where(np.isfinite(first[0]), first[0], 0.0)
    a, b = _pair_of_solves(spec, rec, warm=warm)
    _same(a, b, "warm start")


def test_max_iter_3(cold):
    spec, rec, _ = cold
    a, b = _pair_of_solves(dataclasses.replace(spec, max_iter=3), rec)
    assert (a[2] == 3).all()
    _same(a, b, "max_iter = 3")

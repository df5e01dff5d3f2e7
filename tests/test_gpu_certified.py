"""Every kind of HIP solver verdict certified from the outside: answers of the library (cmpc_amd.solver, the C ABI), a sample of
each launch, checked on the CPU by oracle/kkt_certificate.py at the levels of tests/test_kkt_certificate.py (status 0 within
C_CONVERGED * max(kkt, tol), status 3 within C_ACCEPTABLE * max(kkt, tol) and kkt <= acc_tol), and every status-2 answer of
a cold sample proved infeasible by oracle/stage0_feasibility.py.  The certificates run in a pool of CPU-only workers.

CMPC_CERT_REPORT=<file> appends one JSON line per case: sample size, largest kappa_ind / max(kkt, tol), status-2 answers
certified infeasible."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from conftest import oracle_spec
from cmpc_amd import workloads as wl
from cmpc_amd.problem import ProblemSpec
from test_kkt_certificate import check_certified, _mismatched_state_batch

pytestmark = pytest.mark.gpu

KERNELS = {"single": 1, "pair": 2}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device: the HIP extension must run, there is no fallback")
    from cmpc_amd.solver import BatchedCentroidalMPC
    return BatchedCentroidalMPC


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _solve(gpu, spec, rec, warm=None, state=None, state_out=False):
    s = gpu(spec, device="cuda:0")
    so = s.new_state(rec.shape[0]) if state_out else None
    out, st, it, kkt = s.solve(_dev(rec), warm=_dev(warm), state=_dev(state), state_out=so)
    torch.cuda.synchronize()
    r = (out.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy(), kkt.cpu().numpy())
    return r + ((so.cpu().numpy(),) if state_out else ())


def _report(case, n, worst, n_inf=0, n_st2=0):
    path = os.environ.get("CMPC_CERT_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(case=case, sample=int(n), worst_ratio=float(worst), status2=int(n_st2),
                                    status2_certified_infeasible=int(n_inf))) + "\n")


def _certify_sample(spec, rec, out, st, kkt, idx, case, u_prox=None, cold=True):
    idx = np.asarray(idx)
    worst = check_certified(spec, rec[idx], out[idx], st[idx], kkt[idx], None if u_prox is None else u_prox[idx], what=case)
    n_inf, two = 0, idx[st[idx] == 2]
    if cold and two.size:
        from oracle import nlp_reference as nlp, stage0_feasibility as s0
        ns = nlp.Spec(N=spec.N, nv=spec.nv, k1=spec.k1, k2=spec.k2, delta=spec.delta, w_rate=spec.w_rate)
        for i in two:
            ok, bound = s0.certify(ns, rec[i])
            assert ok, (case, int(i), bound)
            n_inf += 1
    _report(case, int(np.isin(st[idx], (0, 3)).sum()), worst, n_inf, two.size)
    return worst


def _sample(B, n, seed=0):
    return np.sort(np.random.default_rng(seed).choice(B, size=min(n, B), replace=False))


@pytest.mark.parametrize("name", ["perturbed", "payload", "randomized"])
@pytest.mark.parametrize("kernel", ["single", "pair"])
def test_cold_nominal_answers_certify(gpu, name, kernel):
    spec, rec = wl.make_workload(name, B=128, N=20)
    spec = dataclasses.replace(spec, kernel=KERNELS[kernel])
    out, st, it, kkt = _solve(gpu, spec, rec)
    assert np.isin(st, (0, 3)).mean() > 0.85
    _certify_sample(spec, rec, out, st, kkt, _sample(128, 24), "%s N=20 %s" % (name, kernel))


@pytest.mark.parametrize("name,B,N,n", [("perturbed", 32, 3, 16), ("perturbed", 32, 40, 12), ("long_horizon", 16, 40, 6)])
def test_short_and_long_horizons_certify(gpu, name, B, N, n):
    spec, rec = wl.make_workload(name, B=B, N=N)
    if N > 20:
        spec.max_iter = 150                                   # (as tests/test_gpu_parity.py: long horizons take more iterations)
    out, st, it, kkt = _solve(gpu, spec, rec)
    assert np.isin(st, (0, 3)).mean() > 0.8
    _certify_sample(spec, rec, out, st, kkt, _sample(B, n), "%s N=%d nv=%d" % (name, N, spec.nv))


def test_rate_ten_answers_certify(gpu):
    spec, rec = wl.make_workload("perturbed", B=64, N=10, rate=10)
    out, st, it, kkt = _solve(gpu, spec, rec)
    assert np.isin(st, (0, 3)).mean() > 0.7
    _certify_sample(spec, rec, out, st, kkt, _sample(64, 20), "perturbed N=10 rate 10")


@pytest.mark.parametrize("B", [1, 63, 65])
def test_ragged_batches_certify(gpu, B):
    spec, rec = wl.make_workload("randomized", B=B, N=20)
    out, st, it, kkt = _solve(gpu, spec, rec)
    _certify_sample(spec, rec, out, st, kkt, np.unique([0, B // 2, B - 1]), "randomized N=20 B=%d" % B)


def test_launch_beyond_the_pair_threshold_certifies(gpu):
    """The library's own choice at B = 8192 (the one-wavefront kernel, ticket queue well past the resident grid): early and
    late queue positions."""
    spec, rec = wl.make_workload("randomized", B=8192, N=20)
    s = gpu(spec, device="cuda:0")
    out, st, it, kkt = s.solve(_dev(rec))
    torch.cuda.synchronize()
    assert s.last_kernel_name() == "cmpc_solve_kernel<4, 1>"
    out, st, kkt = out.cpu().numpy(), st.cpu().numpy(), kkt.cpu().numpy()
    idx = np.concatenate([np.arange(0, 8192, 512), np.arange(8176, 8192)])
    _certify_sample(spec, rec, out, st, kkt, idx, "randomized N=20 B=8192 auto")


@pytest.mark.parametrize("kernel", ["single", "pair"])
def test_warm_started_answers_certify_around_the_warm_centre(gpu, oracle, kernel):
    spec, rec = wl.make_workload("perturbed", B=32, N=20, scale=0.5)
    cold, st0, _, _ = oracle.solve_batch(oracle_spec(oracle, spec), rec)
    spec = dataclasses.replace(spec, kernel=KERNELS[kernel])
    out, st, it, kkt = _solve(gpu, spec, rec, warm=cold)
    assert np.isin(st, (0, 3)).mean() > 0.9
    _certify_sample(spec, rec, out, st, kkt, _sample(32, 12), "warm start %s" % kernel, u_prox=cold, cold=False)


def test_walk_resumed_from_the_solver_state_certifies(gpu):
    """Closed loop (tests/test_warm_state.py::_loop): every tick resumed from the previous tick's solver state, its proximal
    centre the previous tick's answer."""
    from test_warm_state import _loop
    N = 10
    spec = ProblemSpec(N=N)
    solver = gpu(spec, device="cuda:0")

    def gpu_solve(rec, warm, state):
        s_out = solver.new_state(1)
        out, st, it, kk = solver.solve(_dev(rec), warm=_dev(warm), state=_dev(state), state_out=s_out)
        gpu_solve.kkt.append(float(kk.cpu()[0]))
        return out.cpu().numpy(), s_out.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()
    gpu_solve.kkt = []
    recs, sols, its = _loop(gpu_solve, N, 240, 10, use_state=True)
    st, kkt = _loop.last_status, np.array(gpu_solve.kkt)
    assert its[1:].mean() < its[0]
    warm = np.concatenate([sols[:1] * 0.0, sols[:-1]])             # (tick 0: cold, centre 0)
    _certify_sample(spec, recs, sols, st, kkt, np.arange(len(st)), "walk N=10 resumed", u_prox=warm, cold=False)


def test_foreign_state_batch_status_three_is_the_saved_point(gpu, oracle):
    """512 instances resumed from another instance's state with a budget of 30 iterations: every "acceptable" answer must be
    a point of that quality -- on the device, `out` holds the saved point, not a half-written or later iterate."""
    spec, cs, rec, state = _mismatched_state_batch(oracle)
    out, st, it, kkt, _ = _solve(gpu, spec, rec, state=state, state_out=True)
    three = np.flatnonzero(st == 3)
    zero = np.flatnonzero(st == 0)
    assert three.size >= 3
    idx = np.unique(np.concatenate([three, zero[_sample(zero.size, 16)]])) if zero.size else three
    _certify_sample(spec, rec, out, st, kkt, idx, "foreign state cap 30", cold=False)

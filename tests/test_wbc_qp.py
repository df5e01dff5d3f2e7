"""Whole-body inverse-dynamics QP (reference code/inverse_dynamics.py:92-134, code/utils.py:40-92).
CPU tier: the numpy oracle against the KKT conditions of the reference's own 72-variable statement (the QP is convex:
a KKT point IS the solution, whatever found it), the host-side cost assembly against a literal loop, the C ABI exports.
GPU tier: the HIP kernel against the oracle through the C ABI -- over the parameter matrix (contact phase x foot size x
friction), past the launch's resident grid, at the iteration cap, on a side stream, and on the instances whose wrench
pivots are lost to cancellation ("Whole-body QP": the F_REG floor)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from cmpc_amd import capi, wbc, workloads as wl
from oracle import wbc_qp_oracle as wq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("contact", ["ds", "lfoot", "rfoot"])
def test_oracle_solution_satisfies_the_reference_statement(contact):
    Hq, Fq, M, h, Jc = wl.wbc_synthetic(6, seed=3, contact=contact)
    for b in range(6):
        r = wq.solve(Hq[b], Fq[b], M[b], h[b], Jc[b], 0.05, 0.5)
        assert r["status"] == 0 and r["iters"] <= 40
        k = wq.kkt_full(Hq[b], Fq[b], M[b], h[b], Jc[b], 0.05, 0.5, r["qdd"], r["tau"], r["f"])
        assert k["stationarity"] < 1e-6 and k["equality"] < 1e-8 and k["ineq_violation"] < 1e-9
        # the statement's rows, literally: CoP inside the foot, friction pyramid, unilateral normal force
        for w in (r["f"][0:6], r["f"][6:12]):
            assert abs(w[0]) <= 0.05 * w[5] + 1e-8 and abs(w[1]) <= 0.05 * w[5] + 1e-8
            assert abs(w[3]) <= 0.5 * w[5] + 1e-8 and abs(w[4]) <= 0.5 * w[5] + 1e-8 and w[5] >= -1e-9
        assert np.all(r["tau"][:6] == 0.0)
    # a foot in the air carries (next to) nothing: its Jacobian rows are zero, only the 1e-6 regulariser sees it
    if contact != "ds":
        air = slice(6, 12) if contact == "lfoot" else slice(0, 6)
        assert np.abs(r["f"][air]).max() < 1.0


def test_solution_is_the_minimiser_among_feasible_perturbations():
    """Independent of the KKT algebra: no feasible point nearby has a lower cost."""
    Hq, Fq, M, h, Jc = wl.wbc_synthetic(1, seed=11)
    r = wq.solve(Hq[0], Fq[0], M[0], h[0], Jc[0], 0.05, 0.5)
    cost = lambda q, f: 0.5 * q @ Hq[0] @ q + Fq[0] @ q + 0.5 * wq.F_REG * f @ f
    base = cost(r["qdd"], r["f"])
    Ae = np.hstack([M[0][:6, :], -Jc[0][:, :6].T])
    Ai = wq.ineq_matrix(0.05, 0.5)
    N_ = np.linalg.svd(Ae)[2][6:].T                        # null space of the floating-base rows
    rng = np.random.default_rng(0)
    for _ in range(200):
        dx = N_ @ rng.normal(0, 1e-2, size=N_.shape[1])
        q, f = r["qdd"] + dx[:30], r["f"] + dx[30:]
        if (Ai @ f <= 0).all():
            assert cost(q, f) >= base - 1e-9 * abs(base)


def test_cost_assembly_matches_the_literal_loop():
    rng = np.random.default_rng(5)
    B, rows = 3, {'lfoot': 6, 'rfoot': 6, 'com': 3, 'torso': 3, 'base': 3, 'joints': 30}
    J = {k: rng.normal(size=(B, r, 30)) for k, r in rows.items()}
    Jd = {k: rng.normal(size=(B, r, 30)) for k, r in rows.items()}
    ff, pe, ve = ({k: rng.normal(size=(B, r)) for k, r in rows.items()} for _ in range(3))
    qd = rng.normal(size=(B, 30))
    t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}
    Hq, Fq = wbc.assemble_task_cost(t(J), t(Jd), t(ff), t(pe), t(ve), torch.from_numpy(qd))
    for b in range(B):
        H, F = np.zeros((30, 30)), np.zeros(30)
        for task in wbc.TASKS:                                # code/inverse_dynamics.py:92-103
            H += wbc.WEIGHTS[task] * J[task][b].T @ J[task][b]
            F += -wbc.WEIGHTS[task] * J[task][b].T @ (ff[task][b] + wbc.VEL_GAINS[task] * ve[task][b]
                                                      + wbc.POS_GAINS[task] * pe[task][b] - Jd[task][b] @ qd[b])
        assert np.allclose(Hq[b].numpy(), H, rtol=1e-12, atol=1e-12) and np.allclose(Fq[b].numpy(), F, rtol=1e-12, atol=1e-12)


def test_header_symbols_are_exported():
    text = open(os.path.join(ROOT, "include", "cmpc_wbc.h")).read()
    names = sorted(set(re.findall(r"\b(cmpc_wbc_[a-z_]+)\s*\(", text)))
    assert set(names) == set(capi.WBC_SYMBOLS)
    raw = ctypes.CDLL(capi.LIB_PATH)
    for n in names:
        assert hasattr(raw, n)


# ---- the wrench-block pivot floor.  Instance b of wbc_synthetic(32, seed, contact) at half foot size d and
# friction mu: the fz pivot of a foot's 6 x 6 block (column 35 or 41) comes out <= 0 one or two Newton steps before
# convergence -- a difference of barrier terms of size z / s ~ 1e10 whose exact value is >= F_REG = 1e-6.
LOST_PIVOT = [("ds", 3, 0.02, 0.5, 31), ("lfoot", 21, 0.05, 0.3, 3), ("lfoot", 21, 0.05, 0.7, 10), ("rfoot", 21, 0.1, 0.9, 30)]
CONTACTS = ("ds", "lfoot", "rfoot")
FOOT_MU = ((0.1, 0.5), (0.1, 0.3), (0.1, 0.7), (0.2, 0.9), (0.04, 0.5))          # (foot_size, mu); d = foot_size / 2
MATRIX_SEED, MATRIX_B, N_ORACLE = 21, 1024, 16


@functools.lru_cache(maxsize=None)
def _instances(contact, seed, B):
    """Read-only (instance b does not depend on B: wbc_synthetic draws instance after instance from one stream)."""
    mats = wl.wbc_synthetic(B, seed=seed, contact=contact)
    for a in mats:
        a.setflags(write=False)
    return mats


@functools.lru_cache(maxsize=None)
def _oracle(contact, seed, B, b, d, mu, tol=wq.TOL, max_iter=wq.MAX_ITER):
    return wq.solve(*(a[b] for a in _instances(contact, seed, B)), d, mu, tol=tol, max_iter=max_iter)


def _kkt_ok(mats, b, d, mu, qdd, tau30, f, eq=1e-8, ineq=1e-9):
    """The file's thresholds on the reference statement's KKT conditions (CPU tier 1e-6 / 1e-8 / 1e-9, GPU tier 1e-6 /
    1e-7 / 1e-8), with the active band that does not mistake a weakly active row (s ~ z ~ 1e-5: one double-support
    instance in six has one) for a stationarity error (kkt_full), and therefore with the complementarity of the
    multipliers it finds: the solvers stop at s z <= 1e-9 sd, sd = max(1, sum |multipliers| / 2200) -- 1e-8 covers
    multipliers summing to 22 000, twenty times the robot's weight."""
    k = wq.kkt_full(*(a[b] for a in mats), d, mu, qdd, tau30, f, act_tol=1e-4)
    assert k["stationarity"] < 1e-6 and k["equality"] < eq and k["ineq_violation"] < ineq and k["comp"] < 1e-8, (b, k)


@pytest.mark.parametrize("contact,seed,d,mu,b", LOST_PIVOT)
def test_oracle_floors_a_wrench_pivot_lost_to_cancellation(contact, seed, d, mu, b):
    r = _oracle(contact, seed, 32, b, d, mu)
    assert r["status"] == 0 and r["floored"] >= 1 and r["iters"] <= 40
    _kkt_ok(_instances(contact, seed, 32), b, d, mu, r["qdd"], r["tau"], r["f"])


def test_oracle_returns_status_2_and_zeros_on_an_indefinite_hessian():
    Hq, Fq, M, h, Jc = wl.wbc_synthetic(1, seed=5)
    r = wq.solve(-Hq[0], Fq[0], M[0], h[0], Jc[0], 0.05, 0.5)          # the first pivot is negative: no exception
    assert r["status"] == 2 and r["iters"] == 0 and r["floored"] == 0
    assert not r["qdd"].any() and not r["tau"].any() and not r["f"].any()


def test_solve_batch_argument_checks_return_before_any_hip_call():
    """Every rejected call returns 1 with the check's own message (a call that got as far as the HIP runtime would name a
    HIP error instead, with or without a GPU); B == 0 is a valid empty batch whatever the buffers."""
    lib = capi.load()
    bufs = [np.zeros(n) for n in (900, 30, 900, 30, 360, 30, 30, 12)] + [np.zeros(1, dtype=np.int32) for _ in range(2)]
    ptr = [b.ctypes.data for b in bufs]

    def call(B=1, d=0.05, mu=0.5, tol=1e-9, max_iter=60, null=None):
        p = [None if i == null else v for i, v in enumerate(ptr)]
        return lib.cmpc_wbc_qp_solve_batch(0, B, *p[:5], d, mu, tol, max_iter, *p[5:], None)

    assert lib.cmpc_wbc_qp_solve_batch(0, 0, *([None] * 5), 0.05, 0.5, 1e-9, 60, *([None] * 5), None) == 0
    cases = [(dict(B=-1), b"negative batch")] + [(dict(null=i), b"null buffer") for i in range(10)]
    cases += [(kw, b"bad argument") for kw in (dict(tol=0.0), dict(tol=-1e-9), dict(tol=float("nan")), dict(max_iter=0),
                                               dict(max_iter=-3), dict(d=0.0), dict(d=-0.05), dict(d=float("nan")),
                                               dict(mu=0.0), dict(mu=-0.5), dict(mu=float("nan")))]
    for kw, msg in cases:
        assert call(**kw) == 1, kw
        err = lib.cmpc_wbc_last_error()
        assert err and msg in err, (kw, err)


@pytest.mark.gpu
@pytest.mark.parametrize("contact,B", [("ds", 300), ("lfoot", 64), ("rfoot", 64)])
def test_hip_kernel_matches_the_oracle(contact, B):
    Hq, Fq, M, h, Jc = wl.wbc_synthetic(B, seed=21, contact=contact)
    ref = wq.solve_batch(Hq[:48], Fq[:48], M[:48], h[:48], Jc[:48], 0.05, 0.5)
    qp = wbc.BatchedInverseDynamicsQP(foot_size=0.1, mu=0.5, device="cuda:0")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tau, qdd, f, st, it = qp.solve(dev(Hq), dev(Fq), dev(M), dev(h), dev(Jc))
    torch.cuda.synchronize()
    assert (st == 0).all() and int(it.max()) <= 45
    tau, qdd, f = tau.cpu().numpy(), qdd.cpu().numpy(), f.cpu().numpy()
    assert (ref["status"] == 0).all()
    scale = lambda a: np.maximum(np.abs(a).max(axis=1, keepdims=True), 1.0)
    assert (np.abs(tau[:48] - ref["tau"][:, 6:]) / scale(ref["tau"])).max() < 1e-6
    assert (np.abs(qdd[:48] - ref["qdd"]) / scale(ref["qdd"])).max() < 1e-6
    assert (np.abs(f[:48] - ref["f"]) / scale(ref["f"])).max() < 1e-6
    assert np.abs(it.cpu().numpy()[:48] - ref["iters"]).max() <= 2
    # every instance of the batch (beyond the oracle's sample): KKT conditions of the reference statement
    for b in (48, B // 2, B - 1):
        t30 = np.concatenate([np.zeros(6), tau[b]])
        k = wq.kkt_full(Hq[b], Fq[b], M[b], h[b], Jc[b], 0.05, 0.5, qdd[b], t30, f[b])
        assert k["stationarity"] < 1e-6 and k["equality"] < 1e-7 and k["ineq_violation"] < 1e-8
    # batch composition does not matter (instances are independent)
    t2 = qp.solve(dev(Hq[7:9]), dev(Fq[7:9]), dev(M[7:9]), dev(h[7:9]), dev(Jc[7:9]))[0].cpu().numpy()
    assert np.array_equal(t2, tau[7:9])


@pytest.mark.gpu
def test_hip_kernel_failure_path_returns_zeros_like_the_reference():
    """code/utils.py:85-92: QPSolver.solve returns zeros when the solver fails.  An indefinite task Hessian (wrong-inertia
    pivot) and a NaN input (non-finite KKT error) must end with status 2 and finite, zero outputs; the good instances
    of the same batch are untouched."""
    Hq, Fq, M, h, Jc = wl.wbc_synthetic(4, seed=5)
    Hq[1] = -Hq[1]                                  # indefinite: the first pivot is negative
    Fq[2, 3] = np.nan                               # non-finite residual
    qp = wbc.BatchedInverseDynamicsQP(foot_size=0.1, mu=0.5, device="cuda:0")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tau, qdd, f, st, it = qp.solve(dev(Hq), dev(Fq), dev(M), dev(h), dev(Jc))
    torch.cuda.synchronize()
    assert st.tolist() == [0, 2, 2, 0]
    for b in (1, 2):
        assert float(tau[b].abs().max()) == 0.0 and float(qdd[b].abs().max()) == 0.0 and float(f[b].abs().max()) == 0.0
    assert torch.isfinite(tau).all() and torch.isfinite(qdd).all() and torch.isfinite(f).all()
    bad = wq.solve(Hq[2], Fq[2], M[2], h[2], Jc[2], 0.05, 0.5)               # the oracle takes the same exit
    assert bad["status"] == 2 and not bad["qdd"].any() and not bad["tau"].any()
    ref = wq.solve(Hq[3], Fq[3], M[3], h[3], Jc[3], 0.05, 0.5)
    assert np.abs(qdd[3].cpu().numpy() - ref["qdd"]).max() < 1e-6 * max(1.0, np.abs(ref["qdd"]).max())


# ---- GPU tier beyond one parameter set

def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()            # (a writable copy: the cached instances are read-only)


def _launch(mats, foot_size, mu, **kw):
    """One launch on cuda:0; numpy (tau (B,30) with the zero base rows in front, qdd, f, status, iters)."""
    qp = wbc.BatchedInverseDynamicsQP(foot_size=foot_size, mu=mu, device="cuda:0", **kw)
    tau, qdd, f, st, it = qp.solve(*(m if torch.is_tensor(m) else _dev(m) for m in mats))
    torch.cuda.synchronize()
    tau30 = np.concatenate([np.zeros((tau.shape[0], 6)), tau.cpu().numpy()], axis=1)
    return tau30, qdd.cpu().numpy(), f.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()


def _assert_parity(out, idx, refs, iters=True):
    """The parity rule of test_hip_kernel_matches_the_oracle: 1e-6 of the largest entry (at least 1) on tau, qdd and f,
    iteration counts within 2; rows `idx` of the launch `out` against the oracle's results `refs`."""
    tau, qdd, f, st, it = out
    assert all(r["status"] == 0 for r in refs) and (st[idx] == 0).all()
    for got, key in ((tau, "tau"), (qdd, "qdd"), (f, "f")):
        ref = np.array([r[key] for r in refs])
        err = np.abs(got[idx] - ref) / np.maximum(np.abs(ref).max(axis=1, keepdims=True), 1.0)
        assert err.max() < 1e-6, (key, err.max(axis=1))
    if iters:
        assert np.abs(it[idx] - np.array([r["iters"] for r in refs])).max() <= 2


def _sample(contact, d, mu, **kw):
    """The oracle's sample of a class of the parameter matrix: instances 0 .. 15, where the oracle floored no pivot (a
    floored step is a different step: kernel and oracle need not floor in the same one, and the iteration counts are
    compared only where neither the rule nor the rounding decides them).  At most one instance gives way to the next
    one after the sample."""
    idx = list(range(N_ORACLE))
    refs = [_oracle(contact, MATRIX_SEED, MATRIX_B, b, d, mu, **kw) for b in idx]
    swapped = [k for k, r in enumerate(refs) if r["floored"]]
    assert len(swapped) <= 1
    for k in swapped:
        idx[k] = N_ORACLE
        refs[k] = _oracle(contact, MATRIX_SEED, MATRIX_B, N_ORACLE, d, mu, **kw)
        assert refs[k]["floored"] == 0
    return np.array(idx), refs


@pytest.mark.gpu
@pytest.mark.parametrize("foot_size,mu", FOOT_MU)
@pytest.mark.parametrize("contact", CONTACTS)
def test_hip_kernel_over_the_parameter_matrix(contact, foot_size, mu):
    """1024 instances per class: every one converges to finite outputs (before the pivot floor: profiles/
    wbc_pivot_floor.json); sixteen against the oracle, four more against the reference statement's KKT conditions."""
    d = foot_size / 2
    mats = _instances(contact, MATRIX_SEED, MATRIX_B)
    out = _launch(mats, foot_size, mu)
    tau, qdd, f, st, it = out
    assert (st == 0).all(), np.flatnonzero(st != 0)
    assert np.isfinite(tau).all() and np.isfinite(qdd).all() and np.isfinite(f).all() and int(it.max()) <= 45
    idx, refs = _sample(contact, d, mu)
    _assert_parity(out, idx, refs)
    for b in (17, 300, 777, MATRIX_B - 1):
        _kkt_ok(mats, b, d, mu, qdd[b], tau[b], f[b], eq=1e-7, ineq=1e-8)      # (the GPU tier's thresholds, as above)
    # what the sample covers, from the oracle's multipliers: a row with z > 1e-3 has s < 1e-6 at tol 1e-9 -- active
    act = np.array([r["z"] for r in refs]) > 1e-3
    feet = {"ds": (0, 1), "lfoot": (0,), "rfoot": (1,)}[contact]              # (a foot in the air: f ~ 0, every row degenerate)
    cop = [act[:, 8 * k: 8 * k + 4].any(axis=1) for k in feet]
    fric = [act[:, 8 * k + 4: 8 * k + 8].any(axis=1) for k in feet]
    assert np.any(cop) and np.any(fric)
    if contact == "ds":
        assert (act[:, :8].any(axis=1) & act[:, 8:].any(axis=1)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("contact,seed,d,mu,b", LOST_PIVOT)
def test_hip_kernel_solves_the_lost_pivot_instances(contact, seed, d, mu, b):
    """The QP is strictly convex: one solution, whichever steps kernel and oracle floor in (no iteration parity)."""
    mats = _instances(contact, seed, 32)
    out = _launch(mats, 2 * d, mu)
    tau, qdd, f, st, it = out
    assert st[b] == 0 and (st == 0).all()
    _assert_parity(out, np.array([b]), [_oracle(contact, seed, 32, b, d, mu)], iters=False)
    _kkt_ok(mats, b, d, mu, qdd[b], tau[b], f[b], eq=1e-7, ineq=1e-8)


@pytest.mark.gpu
def test_hip_kernel_past_the_resident_grid():
    """The launch's grid is 7 workgroups per CU; a longer batch goes round the instance loop.  B > 2 grids, tiled from 257
    distinct instances (257 is prime to the grid: the copies of an instance land in different workgroups, at different
    turns of the loop, behind different predecessors), the three contact phases interleaved, an indefinite Hessian and
    a NaN planted among them -- below the grid and above it, each followed by good instances in its workgroup.  Nothing
    an instance leaves in LDS (x, the packed factor, the constant Schur complement) or in registers may reach the
    next: every row is bit for bit the row of a launch of the 257 alone, one instance per workgroup."""
    grid = torch.cuda.get_device_properties(0).multi_processor_count * 7
    B, U = 2 * grid + 515, 257
    assert B > 2 * grid and grid % U != 0 and U < grid
    per = [_instances(c, MATRIX_SEED, MATRIX_B) for c in CONTACTS]
    base = [np.stack([per[i % 3][k][i // 3] for i in range(U)]) for k in range(5)]
    bad_h, bad_f = (5, 100, 256), (50, 200)
    for i in bad_h:
        base[0][i] = -base[0][i]
    for i in bad_f:
        base[1][i, 3] = np.nan
    ref = _launch(base, 0.1, 0.5)
    rows = np.arange(B) % U
    got = _launch([_dev(a)[torch.from_numpy(rows).cuda()].contiguous() for a in base], 0.1, 0.5)
    planted = np.isin(rows, bad_h + bad_f)
    assert planted[:grid].sum() >= 5 and planted[grid:].sum() >= 5
    assert (ref[3][list(bad_h + bad_f)] == 2).all() and (np.delete(ref[3], bad_h + bad_f) == 0).all()
    for i in bad_h + bad_f:
        assert not ref[0][i].any() and not ref[1][i].any() and not ref[2][i].any()
    for g, r, name in zip(got, ref, ("tau", "qdd", "f", "status", "iters")):
        assert g.dtype == r.dtype and np.array_equal(g.view(np.uint8), r[rows].view(np.uint8)), name


@pytest.mark.gpu
def test_hip_kernel_iteration_cap_and_looser_tolerance():
    """status 1 = out of iterations, zeros out (the reference's QPSolver returns zeros when OSQP fails): an instance the
    oracle solves in k iterations converges under max_iter = k and does not under k - 1, in kernel and oracle alike."""
    mats = _instances("ds", MATRIX_SEED, MATRIX_B)
    for b in range(4):
        one = [a[b:b + 1] for a in mats]
        k = _oracle("ds", MATRIX_SEED, MATRIX_B, b, 0.05, 0.5)["iters"]
        tau, qdd, f, st, it = _launch(one, 0.1, 0.5, max_iter=k)
        assert st[0] == 0 and it[0] == k and qdd.any()
        tau, qdd, f, st, it = _launch(one, 0.1, 0.5, max_iter=k - 1)
        assert st[0] == 1 and it[0] == k - 1
        assert not tau.any() and not qdd.any() and not f.any()
        capped = wq.solve(*(a[0] for a in one), 0.05, 0.5, max_iter=k - 1)
        assert capped["status"] == 1 and capped["iters"] == k - 1 and not capped["qdd"].any() and not capped["tau"].any()
    idx, refs = _sample("ds", 0.05, 0.5, tol=1e-6)
    tight = [_oracle("ds", MATRIX_SEED, MATRIX_B, b, 0.05, 0.5)["iters"] for b in idx]
    assert sum(r["iters"] for r in refs) <= sum(tight) - N_ORACLE // 2          # (the tolerance did reach the solver)
    _assert_parity(_launch([a[:N_ORACLE + 1] for a in mats], 0.1, 0.5, tol=1e-6), idx, refs)


@pytest.mark.gpu
def test_hip_kernel_on_a_side_stream():
    mats = [_dev(a[:64]) for a in _instances("ds", MATRIX_SEED, MATRIX_B)]
    qp = wbc.BatchedInverseDynamicsQP(foot_size=0.1, mu=0.5, device="cuda:0")
    want = [t.cpu().numpy() for t in qp.solve(*mats)]
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = qp.solve(*mats)
    side.synchronize()
    assert int(want[3].max()) == 0
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy().view(np.uint8), w.view(np.uint8))

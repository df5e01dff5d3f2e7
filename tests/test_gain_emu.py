"""CPU tier: the first-stage gain of the device source (host emulation, tests/emu/cmpc_emu_gain.cpp) against the
independent reference of tests/gain_reference.py (literal restatement, autograd, implicit-function theorem)."""
import ctypes
import os

import numpy as np
import pytest

import build as _b
import gain_reference as gr
from cmpc_amd import workloads as wl
from cmpc_amd.problem import to_cspec

#: max|G - G_ref| / max(1, max|G_ref|) per row group at a status-0 point.  Measured on the emulation: <= 1e-5 at
#: mpc_rate 1; at mpc_rate 10, 4.6e-4 on the foot rows of an instance whose landing foot is pinned through swing stages
#: (the precision floor of a capped-penalty sweep there: cmpc_kernel.hpp, GAIN_SIG_CAP_BOX)
LEVEL = {1: 1e-4, 10: 1e-3}


@pytest.fixture(scope="module")
def emu():
    return ctypes.CDLL(_b.build_emu_gain())


@pytest.fixture(scope="module")
def plain():
    return ctypes.CDLL(_b.build_emu())


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _solve(lib, spec, rec, gain=True, pair=False, fail_iter=None):
    os.environ["CMPC_EMU_PAIR"] = "1" if pair else "0"
    if fail_iter is None:
        os.environ.pop("CMPC_EMU_FAIL_ITER", None)
    else:
        os.environ["CMPC_EMU_FAIL_ITER"] = str(fail_iter)
    try:
        cs = to_cspec(spec)
        rec = np.ascontiguousarray(rec, dtype=np.float64)
        B = rec.shape[0]
        out = np.zeros((B, spec.nsol))
        st, it, kk = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B)
        so = np.zeros((B, spec.nstate))
        if gain:
            G = np.full((B, 20 + spec.nu, 20), 7.0)
            assert lib.cmpc_emu_solve_batch_gain(ctypes.byref(cs), B, _p(rec), None, None, _p(out), _p(so), _p(st), _p(it),
                                                 _p(kk), _p(G)) == 0
            return out, st, it, kk, so, G
        assert lib.cmpc_emu_solve_batch_state(ctypes.byref(cs), B, _p(rec), None, None, _p(out), _p(so), _p(st), _p(it),
                                              _p(kk)) == 0
        return out, st, it, kk, so, None
    finally:
        os.environ.pop("CMPC_EMU_PAIR", None)
        os.environ.pop("CMPC_EMU_FAIL_ITER", None)


def _compare(spec, rec, out, st, G, level):
    cs = to_cspec(spec)
    worst, skipped, n = 0.0, 0, 0
    for b in range(rec.shape[0]):
        if st[b] != 0:
            continue
        n += 1
        assert np.isfinite(G[b]).all(), f"instance {b}: status 0 without a finite gain"
        Gr, weak, _ = gr.gain(cs, rec[b], out[b])
        if weak:
            skipped += 1
            continue
        e = gr.rel_err_groups(G[b], Gr, spec.nv)
        worst = max(worst, max(e.values()))
        assert max(e.values()) <= level, f"instance {b}: {e}"
    assert n > 0
    return worst, skipped, n


@pytest.mark.parametrize("name,N,B,rate", [("randomized", 3, 3, 1), ("randomized", 10, 3, 1), ("perturbed", 10, 3, 1),
                                           ("payload", 10, 3, 1), ("randomized", 10, 3, 10), ("long_horizon", 2, 2, 1)])
def test_gain_matches_reference(emu, name, N, B, rate):
    spec, rec = wl.make_workload(name, B=B, N=N, rate=rate, scale=0.25 if name == "perturbed" else 1.0)
    out, st, _, _, _, G = _solve(emu, spec, rec)
    worst, skipped, n = _compare(spec, rec, out, st, G, LEVEL[rate])
    print(f"{name} N={N} rate={rate}: worst {worst:.2e}, skipped {skipped}/{n}")
    assert n - skipped >= 1                    # (the skipped share is held to a level on a large batch: test_gpu_gain.py)


def test_gain_launch_leaves_the_solve_alone(emu, plain):
    spec, rec = wl.make_workload("randomized", B=3, N=3)
    a = _solve(emu, spec, rec)
    b = _solve(plain, spec, rec, gain=False)
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(x, y)


def test_single_wave_and_pair_bit_identical(emu):
    spec, rec = wl.make_workload("randomized", B=3, N=3)
    a = _solve(emu, spec, rec, pair=False)
    b = _solve(emu, spec, rec, pair=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[5], b[5], equal_nan=True)
    assert np.isfinite(a[5][a[1] == 0]).all()


def test_saved_point_and_failed_instances(emu):
    """A failed factorisation late in the solve returns the saved acceptable point (status 3): the gain is formed there,
    through the saved copy of the iterate; a failure before any point was saved is status 2 and a NaN gain."""
    spec, rec = wl.make_workload("randomized", B=2, N=3)
    out0, st0, it0, _, _, _ = _solve(emu, spec, rec)
    assert (st0 == 0).all()
    # the last iteration fails: the point saved the iteration before is returned
    out, st, it, kk, _, G = _solve(emu, spec, rec[:1], fail_iter=int(it0[0]) - 1)
    assert st[0] == 3, (st, it)
    assert np.isfinite(G[0]).all()
    Gr, weak, _ = gr.gain(to_cspec(spec), rec[0], out[0])
    e = gr.rel_err_groups(G[0], Gr, spec.nv)
    print("saved point", e, "kkt", kk[0])
    assert not weak and max(e.values()) <= LEVEL[1], e
    # the first iteration fails: nothing saved, status 2, NaN
    out, st, it, kk, _, G = _solve(emu, spec, rec[:1], fail_iter=0)
    assert st[0] == 2 and np.isnan(G[0]).all()


@pytest.mark.parametrize("rate,b,cols", [(10, 2, (6, 12, 16, 17, 18)), (1, 1, (0, 4, 7, 10, 12, 16))])
def test_gain_against_finite_differences_of_the_solver(emu, rate, b, cols):
    """Central differences of the emulated solver itself (eps = 1e-4, every perturbed solve status 0), column by column,
    foot columns included: the kernel's G and the reference within LEVEL of them (the differences carry the solver's
    tolerance over eps, ~1e-4).  (At rate 10 the CoM columns of this instance are not smooth at this eps: a Lyapunov row
    changes activity; kernel and reference agree there, the differences do not.)"""
    spec, rec = wl.make_workload("randomized", B=3, N=10, rate=rate)
    out, st, _, _, _, G = _solve(emu, spec, rec[b:b + 1])
    assert st[0] == 0
    Gr, weak, _ = gr.gain(to_cspec(spec), rec[b], out[0])
    eps, nx = 1e-4, 20
    u0 = slice(nx * (spec.N + 1), nx * (spec.N + 1) + spec.nu)
    recs = []
    for c in cols:
        for sgn in (1, -1):
            r = rec[b].copy()
            r[c] += sgn * eps
            recs.append(r)
    o, s, _, _, _, _ = _solve(emu, spec, np.array(recs), gain=False)
    assert (s == 0).all(), s
    for i, c in enumerate(cols):
        d = o[2 * i] - o[2 * i + 1]
        fd = np.concatenate([d[nx:2 * nx], d[u0]]) / (2 * eps)
        sc = max(1.0, np.abs(fd).max())
        e_k, e_r = np.abs(G[0][:, c] - fd).max() / sc, np.abs(Gr[:, c] - fd).max() / sc
        print(f"rate {rate} column {c}: |G - fd| {e_k:.1e}, |G_ref - fd| {e_r:.1e}")
        assert e_k <= LEVEL[rate] and e_r <= LEVEL[rate], (c, e_k, e_r)

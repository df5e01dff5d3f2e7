"""CPU tier: the solver with per-instance constants (Solver<..., CONSTS>, cmpc_solve_batch_consts) as the host emulation
of the device source runs it (tests/emu/cmpc_emu_consts.cpp): bit for bit the plain solver where the rows say what the
spec says, every instance of a mixed batch its own homogeneous solve, the C oracle on each instance's own spec, and the
refusal of a row the solver cannot use.  Small cases: the harness runs 64 OS threads per instance."""
import ctypes
import os

import numpy as np
import pytest

import build as _b
from conftest import oracle_spec, rel_inf
from consts_common import drawn_specs, uniform_rows
from cmpc_amd import problem, workloads as wl
from cmpc_amd.problem import to_cspec


@pytest.fixture(scope="module")
def emu():
    return ctypes.CDLL(_b.build_emu_consts())


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _solve(lib, spec, rec, rows=None, pair=False):
    """(out, status, iters, kkt, state_out) of the emulated solve: the plain solver (rows None) or the CONSTS variant."""
    os.environ["CMPC_EMU_PAIR"] = "1" if pair else "0"
    try:
        cs = to_cspec(spec)
        rec = np.ascontiguousarray(rec, dtype=np.float64)
        B = rec.shape[0]
        out, so = np.full((B, spec.nsol), 7.0), np.full((B, spec.nstate), 7.0)
        st, it, kk = np.full(B, -1, np.int32), np.full(B, -1, np.int32), np.full(B, 7.0)
        if rows is None:
            rc = lib.cmpc_emu_solve_batch_state(ctypes.byref(cs), B, _p(rec), None, None, _p(out), _p(so), _p(st), _p(it), _p(kk))
        else:
            rows = np.ascontiguousarray(rows, dtype=np.float64)
            assert rows.shape == (B, problem.NCONST)
            rc = lib.cmpc_emu_solve_batch_consts(ctypes.byref(cs), B, _p(rec), _p(rows), None, None, _p(out), _p(so), _p(st),
                                                 _p(it), _p(kk))
        assert rc == 0
        return out, st, it, kk, so
    finally:
        os.environ.pop("CMPC_EMU_PAIR", None)


def _same(a, b, idx_a=slice(None), idx_b=slice(None)):
    for x, y in zip(a, b):
        assert np.array_equal(x[idx_a], y[idx_b], equal_nan=True)


@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
@pytest.mark.parametrize("name,N,B", [("perturbed", 10, 2), ("payload", 3, 2), ("randomized", 20, 2)])
def test_rows_of_the_spec_are_bitwise_the_plain_solve(emu, name, N, B, pair):
    spec, rec = wl.make_workload(name, B=B, N=N)
    plain = _solve(emu, spec, rec, pair=pair)
    assert np.isin(plain[1], (0, 3)).all()
    _same(plain, _solve(emu, spec, rec, rows=uniform_rows(spec, B), pair=pair))


@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
def test_mixed_batch_is_bitwise_the_homogeneous_solves(emu, pair):
    """Nominal (4 / 0.1, delta 0.01), mpc_rate 10 (5 / 0.2, delta 0.1, no force-rate cost) and payload (7 / 1) instances
    interleaved in one batch, each with its own row: every instance is its group's own solve."""
    groups = [wl.make_workload("perturbed", B=2, N=10, rate=1), wl.make_workload("perturbed", B=2, N=10, rate=10),
              wl.make_workload("payload", B=2, N=10)]
    s1, s10, sp = (g[0] for g in groups)
    assert (s1.delta, s1.k1, s1.k2, s1.w_rate) != (s10.delta, s10.k1, s10.k2, s10.w_rate) and (sp.k1, sp.k2) == (7.0, 1.0)
    homog = [_solve(emu, s, r, pair=pair) for s, r in groups]
    order = [(0, 0), (1, 0), (2, 0), (1, 1), (0, 1), (2, 1)]                   # (group, instance of the group)
    rec = np.stack([groups[g][1][i] for g, i in order])
    rows = problem.consts_rows([groups[g][0] for g, _ in order])
    # the handle's own constants are none of the groups': only the rows count
    handle = wl.make_workload("perturbed", B=1, N=10)[0]
    handle.k1, handle.k2, handle.w_hw = 6.0, 0.5, 500.0
    mixed = _solve(emu, handle, rec, rows=rows, pair=pair)
    for j, (g, i) in enumerate(order):
        _same(mixed, homog[g], j, i)


@pytest.mark.parametrize("name,N,B", [("perturbed", 10, 3), ("randomized", 20, 2)])
def test_drawn_rows_match_the_oracle_on_each_instances_own_spec(emu, oracle, name, N, B):
    """Levels: tests/test_emu_kernel.py::test_kernel_source_matches_oracle for the same N at rate 1 (same usable verdict,
    every instance usable, rel-inf < 1e-5)."""
    spec, rec = wl.make_workload(name, B=B, N=N)
    over, specs = drawn_specs(spec, B)
    got, st, it, kk, _ = _solve(emu, spec, rec, rows=problem.consts_rows(specs))
    for b in range(B):
        cs = oracle_spec(oracle, spec, **over[b])
        ref, st_ref, it_ref, _ = oracle.solve(cs, rec[b])
        err = rel_inf(got[b], ref)[0]
        print(f"{name} N={N} instance {b}: status {st[b]} / {st_ref}, iterations {it[b]} / {it_ref}, rel-inf {err:.2e}")
        assert (st[b] in (0, 3)) == (st_ref in (0, 3)) and st[b] in (0, 3)
        assert err < 1e-5
    # the rows matter: the shared spec's answer is another one
    base = _solve(emu, spec, rec[:1])
    assert rel_inf(got[0], base[0][0])[0] > 1e-6


@pytest.mark.parametrize("field,value", [("k2", float("nan")), ("delta", 0.0), ("w_foot", -1.0)])
def test_a_bad_row_is_refused_and_its_neighbours_are_untouched(emu, field, value):
    spec, rec = wl.make_workload("perturbed", B=3, N=10)
    rows = uniform_rows(spec, 3)
    good = _solve(emu, spec, rec, rows=rows)
    rows[1, problem.CONST_FIELDS.index(field)] = value
    for pair in (False, True):
        out, st, it, kk, so = _solve(emu, spec, rec, rows=rows, pair=pair)
        assert st[1] == 2 and it[1] == 0 and kk[1] == np.inf and np.isnan(out[1]).all()
        mu_word = spec.nstate - 8 - 2 * (spec.N + 1)
        assert so[1, mu_word] == 0.0                                           # no solver state
        for j in (0, 2):
            _same((out, st, it, kk, so), good, j, j)

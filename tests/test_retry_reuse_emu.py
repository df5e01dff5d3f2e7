"""CPU tier: the reuse path of a retried factorisation (Solver::EVAL_REUSE, csrc/cmpc_kernel.hpp) on the host emulation of
the kernel source.  tests/emu/cmpc_emu_reuse.cpp is built twice, with the reuse path and with -DCMPC_NO_EVAL_REUSE (every
stage of a retry pass evaluated again): every output of the two must agree bit for bit, and the harness counters must show
that the reuse path really ran.

Batches (chosen on the CPU, with the C oracle's own retry counts):
  cold     `randomized`, B = 4, N = 20, the configuration's own seed: the oracle reports 42 retried factorisations over the four
           instances (13, 0, 0, 29), 10.5 per instance -- above the 3 per instance of DESIGN.md section 4.  The emulation and
           the oracle run the same algorithm but part in the last bits, and the end game -- where the retries are -- is a few
           iterations longer or shorter for it (28 against 31 on the last instance, a tenth): the emulation's count has to
           lie within a quarter of the oracle's, not on it.
  resumed  the same four records of seed 777 resumed from the states the cold batch wrote (`state` / `state_out`): 53 retry
           passes, 21 of which fail again -- the case of two failed passes in one iteration (k_done is lowered to the
           minimum; the error measures stay the failed passes').
  N = 3, N = 40: short and long horizons (the stage index arithmetic of the reuse words, the terminal node's reload, the
           k_done = N + 1 sentinel), on records the oracle says retry, picked from a draw of 32: N = 3, seed 2, instances
           7, 18, 20, 23 (the oracle: 5, 4, 4, 4 retries); N = 40, the configuration's own seed, instances 3 and 8 (10 and 13).
           The reuse path has to run on both (retry passes > 0, stages reused > 0).  Each of these instances retries in a
           handful of iterations only, and an escalation chain (reg x 100, then x 8, until the inertia is right) is one or
           two passes longer or shorter where the kernel's blocked factorisation and the oracle's plain one judge a
           borderline pivot differently; at N = 40 the trajectories also part (30 and 31 iterations against 36 and 26).  With
           counts this small that is a large share, so here the emulation's count has to lie within a factor of two of the
           oracle's."""
import ctypes
import os

import numpy as np
import pytest

import build as _b
from cmpc_amd import workloads as wl
from cmpc_amd.problem import to_cspec


@pytest.fixture(scope="module")
def libs():
    a, b = ctypes.CDLL(_b.build_emu_reuse()), ctypes.CDLL(_b.build_emu_reuse(reuse=False))
    assert a.cmpc_emu_eval_reuse() == 1 and b.cmpc_emu_eval_reuse() == 0
    return a, b


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _solve(lib, spec, rec, state=None):
    """((out, status, iters, kkt, state_out), [retry passes, stages the failed passes had evaluated, stages reused, retry
    passes that failed again]) of the emulated single-wave solve."""
    os.environ.pop("CMPC_EMU_PAIR", None)
    os.environ.pop("CMPC_EMU_FAIL_ITER", None)
    cs = to_cspec(spec)
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    B = rec.shape[0]
    out, so = np.full((B, spec.nsol), 7.0), np.full((B, spec.nstate), 7.0)
    st, it, kk = np.full(B, -1, np.int32), np.full(B, -1, np.int32), np.full(B, 7.0)
    stats = (ctypes.c_longlong * 4)()
    lib.cmpc_emu_retry_stats(stats)                                    # (reset)
    assert lib.cmpc_emu_solve_batch_state(ctypes.byref(cs), B, _p(rec), None, _p(state), _p(out), _p(so), _p(st), _p(it), _p(kk)) == 0
    lib.cmpc_emu_retry_stats(stats)
    return (out, st, it, kk, so), list(stats)


def _same(a, b):
    for name, x, y in zip(("XU", "status", "iters", "kkt", "state"), a, b):
        assert np.array_equal(x, y, equal_nan=True), name


def _oracle_retries(oracle, spec, rec):
    cs = oracle.default_spec(N=spec.N, nv=spec.nv, tol=spec.tol, max_iter=spec.max_iter, k1=spec.k1, k2=spec.k2, prox=spec.prox,
                             acc_tol=spec.acc_tol)
    B = rec.shape[0]
    out = np.zeros((B, oracle.nsol(cs)))
    st, it, nreg = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    kkt, waste = np.zeros(B), np.zeros(B)
    assert oracle.lib().cmpc_oracle_solve_batch_stats(ctypes.byref(cs), B, _p(rec), None, _p(out), _p(st), _p(it), _p(kkt), _p(nreg),
                                                      _p(waste), 0) == 0
    return nreg


COLD_B, RESUME_SEED = 4, 777          # cold batch: `randomized`, the configuration's own seed; resumed on the records of seed 777


@pytest.fixture(scope="module")
def cold(libs):
    spec, rec = wl.make_workload("randomized", B=COLD_B)
    assert spec.N == 20 and spec.nv == 4
    return spec, rec, _solve(libs[0], spec, rec), _solve(libs[1], spec, rec)


def test_cold_batch_that_retries_is_bitwise_the_full_evaluation(cold, oracle):
    spec, rec, (new, stats), (old, stats_old) = cold
    nreg = _oracle_retries(oracle, spec, rec)
    print(f"oracle retries {nreg.tolist()}, emulation: {stats[0]} retry passes, {stats[1]} stages evaluated by failed passes, "
          f"{stats[2]} stages reused, {stats[3]} retry passes failed again; iterations {new[2].tolist()}")
    assert nreg.mean() >= 3.0                                          # the batch retries at the level DESIGN.md section 4 records
    _same(new, old)
    assert stats[0] > 0 and stats[2] > 0                               # the reuse path ran
    assert stats_old[2] == 0
    assert 0.75 * nreg.sum() <= stats[0] <= 1.25 * nreg.sum()          # ... as often as the oracle retries (docstring)
    # every stage a failed pass had evaluated is reused by the pass that follows it (and by no other)
    assert stats[2] >= stats[1] - (spec.N + 1) * stats[3] and stats[2] <= (spec.N + 1) * stats[0]


def test_resumed_batch_with_two_failed_passes_in_one_iteration(cold, libs):
    spec, _, (first, _), _ = cold
    _, rec2 = wl.make_workload("randomized", B=COLD_B, seed=RESUME_SEED)
    state = np.ascontiguousarray(first[4])
    new, stats = _solve(libs[0], spec, rec2, state=state)
    old, _ = _solve(libs[1], spec, rec2, state=state)
    print(f"resumed: status {new[1].tolist()} iterations {new[2].tolist()}, {stats[0]} retry passes, {stats[2]} stages reused, "
          f"{stats[3]} retry passes failed again")
    _same(new, old)
    assert stats[0] > 0 and stats[2] > 0
    assert stats[3] > 0                                                # a second failed pass in one iteration


HORIZONS = {3: (2, [7, 18, 20, 23]), 40: (None, [3, 8])}          # N: (seed, instances of a draw of 32 that retry)


@pytest.mark.parametrize("N", sorted(HORIZONS))
def test_short_and_long_horizons_that_retry(libs, oracle, N):
    seed, idx = HORIZONS[N]
    spec, rec = wl.make_workload("randomized", B=32, N=N, seed=seed)
    if N > 20:
        spec.max_iter = 150
    rec = np.ascontiguousarray(rec[idx])
    nreg = _oracle_retries(oracle, spec, rec)
    new, stats = _solve(libs[0], spec, rec)
    old, _ = _solve(libs[1], spec, rec)
    print(f"N = {N}: oracle retries {nreg.tolist()}; status {new[1].tolist()} iterations {new[2].tolist()}, retry passes {stats[0]}, "
          f"stages reused {stats[2]}, retry passes failed again {stats[3]}")
    assert (nreg > 0).all()                                            # every instance retries
    assert np.isin(new[1], (0, 3)).all()
    _same(new, old)
    assert stats[0] > 0 and stats[2] > 0                               # the reuse path ran at this horizon
    assert 0.5 * nreg.sum() <= stats[0] <= 2.0 * nreg.sum()
    assert stats[2] <= (N + 1) * stats[0]

"""GPU tier: batches with per-instance gains, weights and foot geometry (cmpc_solve_batch_consts,
BatchedCentroidalMPC.solve_with_consts).  Rows that say what the spec says give the plain launch bit for bit; every
instance of a mixed fleet is its group's homogeneous launch bit for bit; drawn rows agree with the C oracle run per
instance on its own spec, by the rule of tests/test_gpu_parity.py::test_parity_with_oracle; a bad row costs its own
instance only."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from conftest import oracle_spec, rel_inf
from consts_common import drawn_specs, uniform_rows
from cmpc_amd import problem, workloads as wl
import nlp_batch
from test_gpu_parity import LEVELS, REL_TOL, FLAT_TIGHT, _explain_outliers

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KERNELS = {"single": 1, "pair": 2}
PLAIN_NAMES = {("single", 4): "cmpc_solve_kernel<4, 1>", ("pair", 4): "cmpc_solve_pair_kernel<4, 2>",
               ("single", 8): "cmpc_solve_kernel<8, 2>"}
CONSTS_NAMES = {("single", 4): "cmpc_solve_consts_kernel<4, 1>", ("pair", 4): "cmpc_solve_pair_consts_kernel<4, 2>",
                ("single", 8): "cmpc_solve_consts_kernel<8, 2>"}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device: the HIP extension must run, there is no fallback")
    from cmpc_amd.solver import BatchedCentroidalMPC
    return BatchedCentroidalMPC


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(solver, rec, rows=None, warm=None, state=None, want_state=False):
    """(out, status, iters, kkt[, state_out]) as numpy; rows None = the plain launch."""
    B = rec.shape[0]
    so = solver.new_state(B) if want_state else None
    kw = dict(warm=None if warm is None else _t(warm), state=None if state is None else _t(state), state_out=so)
    r = solver.solve(_t(rec), **kw) if rows is None else solver.solve_with_consts(_t(rec), _t(rows), **kw)
    torch.cuda.synchronize()
    res = tuple(x.cpu().numpy() for x in r)
    return res + (so.cpu().numpy(),) if want_state else res


def _same(a, b, ia=slice(None), ib=slice(None)):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x[ia], y[ib], equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,name,N,B", [("single", "randomized", 20, 512), ("pair", "randomized", 20, 512),
                                             ("single", "long_horizon", 40, 64)])
def test_rows_of_the_spec_are_bitwise_the_plain_launch(gpu, kernel, name, N, B):
    spec, rec = wl.make_workload(name, B=B, N=N)
    spec = dataclasses.replace(spec, kernel=KERNELS[kernel])
    if N > 20:
        spec.max_iter = 150
    s = gpu(spec, device=DEV)
    plain = _run(s, rec, want_state=True)
    assert s.last_kernel_name() == PLAIN_NAMES[(kernel, spec.nv)]
    got = _run(s, rec, rows=uniform_rows(spec, B), want_state=True)
    assert s.last_kernel_name() == CONSTS_NAMES[(kernel, spec.nv)], s.last_kernel_name()
    assert np.isin(plain[1], (0, 3)).mean() > 0.85
    _same(got, plain)
    s.close()


@pytest.mark.parametrize("kernel", ["single", "pair"])
def test_mixed_fleet_is_bitwise_the_homogeneous_launches(gpu, kernel):
    """Nominal perturbed (4 / 0.1), payload (7 / 1) and mpc_rate-10 perturbed (5 / 0.2, delta 0.1, no force-rate cost):
    128 instances each, shuffled into one launch with their own rows."""
    groups = [wl.make_workload("perturbed", B=128, N=20), wl.make_workload("payload", B=128, N=20),
              wl.make_workload("perturbed", B=128, N=20, rate=10)]
    homog = []
    for spec, rec in groups:
        s = gpu(dataclasses.replace(spec, kernel=KERNELS[kernel]), device=DEV)
        homog.append(_run(s, rec, want_state=True))
        assert s.last_kernel_name() == PLAIN_NAMES[(kernel, 4)]
        s.close()
    rng = np.random.default_rng(11)
    order = rng.permutation(3 * 128)
    g_of, i_of = order // 128, order % 128
    rec = np.stack([groups[g][1][i] for g, i in zip(g_of, i_of)])
    rows = problem.consts_rows([groups[g][0] for g in g_of])
    assert len({tuple(r) for r in rows}) == 3
    s = gpu(dataclasses.replace(groups[0][0], kernel=KERNELS[kernel]), device=DEV)
    mixed = _run(s, rec, rows=rows, want_state=True)
    assert s.last_kernel_name() == CONSTS_NAMES[(kernel, 4)]
    s.close()
    for g in range(3):
        sel = np.flatnonzero(g_of == g)
        _same(mixed, homog[g], sel, i_of[sel])
        assert np.isin(homog[g][1], (0, 3)).mean() > 0.7


def test_drawn_rows_against_the_oracle_per_instance(gpu, oracle):
    """The rule of test_gpu_parity.py::test_parity_with_oracle for the `nominal` class, with the oracle run per instance on
    that instance's own spec."""
    B, N = 512, 20
    spec, rec = wl.make_workload("randomized", B=B, N=N)
    med_all, med_tight, q90_tight, share, obj_tol = LEVELS["nominal"]
    over, specs = drawn_specs(spec, B)
    s = gpu(spec, device=DEV)
    got, st, it, kkt = _run(s, rec, rows=problem.consts_rows(specs))
    s.close()
    css = [oracle_spec(oracle, spec, **o) for o in over]
    ref, st_ref, kkt_ref = np.zeros_like(got), np.zeros(B, np.int32), np.zeros(B)
    for b in range(B):
        ref[b], st_ref[b], _, kkt_ref[b] = oracle.solve(css[b], rec[b])
    ok_g, ok_r = np.isin(st, (0, 3)), np.isin(st_ref, (0, 3))
    both = ok_g & ok_r
    err = rel_inf(got[both], ref[both])
    tight = (st == 0) & (st_ref == 0)
    err_t = rel_inf(got[tight], ref[tight])
    out = np.where(both)[0][err >= REL_TOL]
    print(f"verdicts differ on {(ok_g != ok_r).sum()} of {B}; both usable {both.mean():.3f}; oracle usable {ok_r.mean():.3f}; "
          f"median {np.median(err):.2e}, tight median {np.median(err_t):.2e}, tight q90 {np.quantile(err_t, 0.9):.2e}, "
          f"tight max {err_t.max():.2e}; beyond 1e-4: {len(out)} of {int(both.sum())}; mean iterations {it[ok_g].mean():.1f}")
    assert (ok_g != ok_r).sum() <= max(2, 0.03 * B)
    assert both.mean() >= 0.85
    assert np.median(err) < med_all and np.median(err_t) < med_tight and np.quantile(err_t, 0.9) < q90_tight
    assert err_t.max() <= FLAT_TIGHT
    assert len(out) <= share * both.sum(), (len(out), int(both.sum()))
    for i in out:                                                 # every one of them explained, on its own spec
        _explain_outliers(oracle, css[i], spec, rec, got, ref, [i], st, st_ref, kkt, kkt_ref, obj_tol=obj_tol)


def test_closed_loop_ticks_with_state_and_drawn_rows(gpu):
    """Three ticks with state / state_out: with drawn rows the second tick takes fewer iterations than a cold solve of the
    same records; with uniform rows every tick is bit for bit the plain closed loop."""
    B, N = 256, 20
    spec, _ = wl.make_workload("perturbed", B=B, N=N)
    sc = wl.scene()
    rng = np.random.default_rng(5)
    t0 = rng.integers(200, 1200, size=B)

    def records(tick):
        t = t0 + tick
        com, dcom = sc.nominal_state(t)
        com = com + np.random.default_rng(7).uniform(-0.01, 0.01, size=(B, 3))
        com[:, 2] = np.minimum(com[:, 2], 0.755)
        z = np.zeros((B, 3))
        return sc.build_records(spec, t, com, dcom, z, z, np.zeros(B), np.zeros(B), np.full(B, wl.HRP4_MASS), np.full(B, 0.5))

    recs = [records(k) for k in range(3)]
    s = gpu(spec, device=DEV)
    drawn = problem.consts_rows(drawn_specs(spec, B)[1])
    for rows, check_plain in ((uniform_rows(spec, B), True), (drawn, False)):
        warm, state, warm_p, state_p = None, None, None, None
        for k in range(3):
            got = _run(s, recs[k], rows=rows, warm=warm, state=state, want_state=True)
            if check_plain:
                plain = _run(s, recs[k], warm=warm_p, state=state_p, want_state=True)
                _same(got, plain)
                warm_p, state_p = plain[0], plain[4]
            ok = np.isin(got[1], (0, 3))
            assert ok.mean() > 0.85
            if k == 1:
                cold = _run(s, recs[k], rows=rows)
                both = ok & np.isin(cold[1], (0, 3))
                print(f"tick 1 ({'uniform' if check_plain else 'drawn'} rows): {got[2][both].mean():.1f} iterations resumed, "
                      f"{cold[2][both].mean():.1f} cold")
                assert got[2][both].mean() < cold[2][both].mean()
            warm, state = got[0], got[4]
    s.close()


def test_sizes_empty_single_and_ragged_full_size(gpu):
    spec, rec = wl.make_workload("randomized", B=8192 + 37, N=20)
    s = gpu(spec, device=DEV)
    e = s.solve_with_consts(_t(rec[:0]), _t(np.zeros((0, 18))))
    assert e[0].shape == (0, spec.nsol) and e[1].shape == (0,)
    one = _run(s, rec[:1], rows=uniform_rows(spec, 1))
    _same(one, _run(s, rec[:1]))
    # four drawn specs dealt round the ragged batch: the properties of test_full_size_properties_domain_randomised, each
    # instance against its own constants
    B = rec.shape[0]
    over, pal = drawn_specs(spec, 4)
    rows = problem.consts_rows([pal[b % 4] for b in range(B)])
    got, st, it, kkt = _run(s, rec, rows=rows)
    assert s.last_kernel_name() == CONSTS_NAMES[("single", 4)]
    s.close()
    conv = np.isin(st, (0, 3))
    assert conv.mean() > 0.9
    assert np.isfinite(got).all()
    for j in range(4):
        sel = conv & (np.arange(B) % 4 == j)
        r = nlp_batch.residuals(pal[j], rec[sel], got[sel])
        assert r["x0"].max() == 0.0
        assert r["defect"].max() < 1e-7
        assert r["cone"].max() < 1e-5 and r["unilateral"].max() < 1e-5
        assert r["height"].max() < 1e-6 and r["box"].max() < 1e-6
        assert r["lyapunov"].max() < 1e-5 and r["contraction"].max() < 1e-6
        assert r["swing_force"].max() < 1e-6
    assert (kkt[st == 0] <= 100 * spec.tol).all() and (kkt[st == 3] <= spec.acc_tol).all() and (it[conv] <= spec.max_iter).all()


def test_misuse_is_refused(gpu):
    spec, rec = wl.make_workload("perturbed", B=4, N=10)
    s = gpu(spec, device=DEV)
    r, rows = _t(rec), _t(uniform_rows(spec, 4))
    out = torch.empty((4, spec.nsol), dtype=torch.float64, device=DEV)
    st, it = torch.empty(4, dtype=torch.int32, device=DEV), torch.empty(4, dtype=torch.int32, device=DEV)
    kk = torch.empty(4, dtype=torch.float64, device=DEV)
    rc = s._lib.cmpc_solve_batch_consts(s._h, 4, r.data_ptr(), None, None, None, out.data_ptr(), None, st.data_ptr(),
                                        it.data_ptr(), kk.data_ptr(), ctypes.c_void_p(0))
    assert rc != 0 and b"consts" in s._lib.cmpc_last_error(s._h)
    for bad in (rows[:3], rows[:, :17].contiguous(), rows.float(), rows.cpu(), rows.t().contiguous().t(), rows.cpu().numpy()):
        with pytest.raises(ValueError):
            s.solve_with_consts(r, bad)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            s.solve_with_consts(r, rows.to("cuda:1"))
    got = s.solve_with_consts(r, rows)                            # the handle is still good
    torch.cuda.synchronize()
    assert np.isin(got[1].cpu().numpy(), (0, 3)).all()
    s.close()


@pytest.mark.parametrize("kernel", ["single", "pair"])
def test_one_bad_row_changes_nothing_else(gpu, kernel):
    B = 512
    spec, rec = wl.make_workload("randomized", B=B, N=20)
    s = gpu(dataclasses.replace(spec, kernel=KERNELS[kernel]), device=DEV)
    rows = problem.consts_rows(drawn_specs(spec, B)[1])
    good = _run(s, rec, rows=rows, want_state=True)
    keep = np.ones(B, bool)
    for b, (field, value) in ((17, ("g", float("nan"))), (200, ("delta", 0.0)), (511, ("w_force", -1.0)), (300, ("box[1]", float("inf")))):
        rows[b, problem.CONST_FIELDS.index(field)] = value
        keep[b] = False
    got = _run(s, rec, rows=rows, want_state=True)
    s.close()
    bad = np.flatnonzero(~keep)
    assert (got[1][bad] == 2).all() and (got[2][bad] == 0).all() and np.isinf(got[3][bad]).all() and np.isnan(got[0][bad]).all()
    assert (got[4][bad, spec.nstate - 8 - 2 * (spec.N + 1)] == 0.0).all()
    _same(got, good, keep, keep)

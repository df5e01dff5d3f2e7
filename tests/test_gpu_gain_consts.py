"""GPU tier: gains for batches with per-instance constants (cmpc_solve_batch_gain_consts), the fourth row of the launch table,
and the rollout that asks for them.  On the shapes of tests/test_gpu_instance_loop.py: the reported kernel, the launch with
uniform rows bit for bit the gain launch (six outputs) and the consts launch (five), a batch larger than the resident grid --
the slots' saved iterates are reused -- against a small one, the refusal of one row.  A mixed fleet of nine against three
handles of one spec each, the refusal of null arguments, and BatchedRollout(gains=True) against gains=False."""
import dataclasses

import numpy as np
import pytest
import torch

from consts_common import drawn_specs, uniform_rows
from scenes_common import scene_set
from cmpc_amd import capi, problem, workloads as wl
from cmpc_amd.problem import ProblemSpec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 3
B_BIG = 2048                 # more than the 1792 resident one-wave workgroups of an MI355X (256 CUs x 7)
KERNELS = {"single": 1, "pair": 2}
# case -> (workload, kernel, batch sizes, reported name of the gain-consts launch)
CASES = {
    "nv4-single": ("perturbed", "single", (1, 3, B_BIG), "cmpc_solve_gain_consts_kernel<4, 1>"),
    "nv4-pair": ("perturbed", "pair", (1, 3), "cmpc_solve_pair_gain_consts_kernel<4, 2>"),
    "nv8": ("long_horizon", "single", (1, 3), "cmpc_solve_gain_consts_kernel<8, 2>"),
}
VARIANTS = ("gain", "consts", "both")
_cache = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(x):
    x = x.detach().cpu().contiguous()
    return x.view(torch.int64).numpy() if x.dtype == torch.float64 else x.numpy()


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device: the HIP extension must run, there is no fallback")


def _launch(s, variant, rec, rows=None):
    """(kernel name, (out, status, iters, kkt, state[, G])) of one launch, as numpy."""
    B = rec.shape[0]
    so = s.new_state(B)
    rows = _t(uniform_rows(s.spec, B) if rows is None else rows)
    G = None
    if variant == "gain":
        *r, G = s.solve_with_gain(_t(rec), state_out=so)
    elif variant == "consts":
        r = s.solve_with_consts(_t(rec), rows, state_out=so)
    else:
        *r, G = s.solve_with_gain(_t(rec), state_out=so, consts=rows)
    torch.cuda.synchronize()
    return s.last_kernel_name(), tuple(x.cpu().numpy() for x in r) + (so.cpu().numpy(),) + (() if G is None else (G.cpu().numpy(),))


def _case(case):
    """Every launch of a case, once: {(variant, B): (name, arrays)}, plus ("nan", 3): the gain-consts launch with a NaN in row 1."""
    if case not in _cache:
        _need_gpu()
        from cmpc_amd.solver import BatchedCentroidalMPC
        name, kernel, sizes, _ = CASES[case]
        spec, rec = wl.make_workload(name, B=max(sizes), N=N)
        s = BatchedCentroidalMPC(dataclasses.replace(spec, kernel=KERNELS[kernel]), device=DEV)
        res = {(v, B): _launch(s, v, rec[:B]) for B in sizes for v in VARIANTS}
        rows = uniform_rows(s.spec, 3)
        rows[1, 1] = float("nan")
        res[("nan", 3)] = _launch(s, "both", rec[:3], rows)
        s.close()
        _cache[case] = (spec, res)
    return _cache[case]


def _same(a, b, ia=slice(None), ib=slice(None), n=None):
    n = len(a) if n is None else n
    assert len(a) >= n and len(b) >= n
    for x, y in zip(a[:n], b[:n]):
        assert np.array_equal(x[ia], y[ib], equal_nan=True)


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_fourth_row_of_the_table_reports_its_kernel(case):
    spec, res = _case(case)
    assert spec.nv == (8 if case == "nv8" else 4)
    for B in CASES[case][2]:
        assert res[("both", B)][0] == CASES[case][3], (B, res[("both", B)][0])
        assert "consts" not in res[("gain", B)][0] and "gain" not in res[("consts", B)][0]


@pytest.mark.parametrize("case", sorted(CASES))
def test_uniform_rows_are_bitwise_the_gain_launch_and_the_consts_launch(case):
    _, res = _case(case)
    for B in CASES[case][2]:
        both, gain, consts = (res[(v, B)][1] for v in ("both", "gain", "consts"))
        assert len(both) == len(gain) == 6 and len(consts) == 5
        ok = gain[1] == 0
        if B >= 3:                              # (the comparisons are not between refusals or gains of NaN only)
            assert ok.mean() > 0.5 and np.isfinite(gain[5][ok]).all()
        _same(both, gain)                       # solution, status, iterations, KKT error, state, gain
        _same(both, consts, n=5)


def test_small_batches_are_rows_of_the_batch_whose_slots_draw_second_tickets():
    """B = 2048 on 1792 resident slots: the saved iterate of a slot serves more than one instance."""
    _, res = _case("nv4-single")
    big = res[("both", B_BIG)][1]
    _same(res[("both", 3)][1], big, slice(None), slice(0, 3))
    _same(res[("both", 1)][1], big, slice(None), slice(0, 1))


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_nan_row_is_refused_without_a_gain_and_the_others_are_unchanged(case):
    _, res = _case(case)
    got, good = res[("nan", 3)][1], res[("both", 3)][1]
    assert res[("nan", 3)][0] == CASES[case][3]
    assert got[1][1] == 2 and got[2][1] == 0 and np.isinf(got[3][1]) and np.isnan(got[0][1]).all()
    assert np.isnan(got[5][1]).all()                                           # every word of the gain block
    _same(got, good, [0, 2], [0, 2])


def test_mixed_fleet_of_nine_equals_three_handles_of_one_spec_each():
    """Nominal, payload and mpc_rate 10 instances interleaved in one launch at N = 10 (the inputs of the CPU tier), each with
    its own row on a handle whose own constants are none of theirs: every instance is its own spec's solve_with_gain."""
    _need_gpu()
    from cmpc_amd.solver import BatchedCentroidalMPC
    groups = [wl.make_workload("perturbed", B=3, N=10, scale=0.25), wl.make_workload("payload", B=3, N=10),
              wl.make_workload("randomized", B=3, N=10, rate=10)]
    assert len({(s.delta, s.k1, s.k2) for s, _ in groups}) == 3
    ref = []
    for spec, rec in groups:
        s = BatchedCentroidalMPC(spec, device=DEV)
        ref.append(_launch(s, "gain", rec)[1])
        s.close()
    order = [(g, i) for i in range(3) for g in range(3)]
    rec = np.stack([groups[g][1][i] for g, i in order])
    rows = problem.consts_rows([groups[g][0] for g, _ in order])
    handle = dataclasses.replace(groups[0][0], k1=6.0, k2=0.5, w_hw=500.0)
    s = BatchedCentroidalMPC(handle, device=DEV)
    name, mixed = _launch(s, "both", rec, rows)
    s.close()
    assert "gain_consts" in name
    n_gain = 0
    for j, (g, i) in enumerate(order):
        _same(mixed, ref[g], j, i)
        n_gain += int(np.isfinite(mixed[5][j]).all())
    assert n_gain >= 3


def test_null_gain_and_null_consts_are_refused_with_a_message():
    _need_gpu()
    from cmpc_amd.solver import BatchedCentroidalMPC
    spec, rec = wl.make_workload("perturbed", B=1, N=N)
    s = BatchedCentroidalMPC(spec, device=DEV)
    lib = capi.load()
    r, rows = _t(rec), _t(uniform_rows(spec, 1))
    out, G = torch.empty((1, spec.nsol), dtype=torch.float64, device=DEV), torch.empty((1, 20 + spec.nu, 20), dtype=torch.float64, device=DEV)
    st, it = torch.empty(1, dtype=torch.int32, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)
    kk = torch.empty(1, dtype=torch.float64, device=DEV)
    call = lambda c, g: lib.cmpc_solve_batch_gain_consts(s._h, 1, r.data_ptr(), c, None, None, out.data_ptr(), None, st.data_ptr(),
                                                         it.data_ptr(), kk.data_ptr(), g, None)
    assert call(rows.data_ptr(), None) != 0
    msg = lib.cmpc_last_error(s._h).decode()
    assert "null gain" in msg and "use cmpc_solve_batch_consts for" in msg, msg
    assert call(None, G.data_ptr()) != 0
    msg = lib.cmpc_last_error(s._h).decode()
    assert "null consts" in msg and "use cmpc_solve_batch_gain for" in msg, msg
    assert call(rows.data_ptr(), G.data_ptr()) == 0
    torch.cuda.synchronize()
    assert st.item() in (0, 3)
    with pytest.raises(ValueError):
        s.solve_with_gain(r, consts=rows[:, :17])
    s.close()


def test_rollout_with_gains_walks_the_same_trajectory_and_keeps_the_gains():
    """A fleet of six over the five walks with drawn constants, three ticks: gains=True changes nothing of the walk; the gains
    it keeps are those of each instance's own spec on the tick's records, warm start and solver state; tracking the state the
    records were built at returns the tick's x_1 and u_0."""
    _need_gpu()
    from cmpc_amd.rollout import BatchedRollout
    from cmpc_amd.solver import BatchedCentroidalMPC
    ss, spec, B, t0 = scene_set(), ProblemSpec(N=N), 6, 240
    sid = np.array([0, 1, 2, 3, 4, 0], dtype=np.int32)
    _, specs = drawn_specs(spec, B)
    rows = problem.consts_rows(specs)
    com, dcom = ss.nominal_state(np.full(B, t0), sid)
    a = BatchedRollout(ss, spec, B, device=DEV, scene_id=sid, consts=rows, gains=True)
    b = BatchedRollout(ss, spec, B, device=DEV, scene_id=sid, consts=rows, gains=False)
    for ro in (a, b):
        ro.reset(t0, com, dcom)
    assert b.last_gain is None
    for tick in range(3):
        warm = None if a.warm is None else a.warm.clone()
        s_in = a._state[0].clone()
        ra, rb = a.step(), b.step()
        for x, y in zip(ra, rb):
            assert np.array_equal(_bits(x), _bits(y))
        for k in ("state", "last_XU", "last_status", "last_iters", "plan_pos", "t", "alive", "warm"):
            assert np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k))), (tick, k)
    assert "gain_consts" in a.solver.last_kernel_name() and "gain" not in b.solver.last_kernel_name()
    assert b.last_gain is None and tuple(a.last_gain.shape) == (B, 20 + spec.nu, 20)
    status = a.last_status.cpu().numpy()
    n_gain = 0
    for i in range(B):                               # the last tick again, instance by instance on a handle of its own spec
        s = BatchedCentroidalMPC(specs[i], device=DEV)
        XU, st, it, _, G = s.solve_with_gain(a.last_records[i:i + 1], warm=warm[i:i + 1].contiguous(), state=s_in[i:i + 1].contiguous())
        torch.cuda.synchronize()
        assert np.array_equal(_bits(XU), _bits(a.last_XU[i:i + 1])) and st.item() == status[i]
        assert np.array_equal(_bits(G), _bits(a.last_gain[i:i + 1])), i
        n_gain += int(torch.isfinite(G).all().item())
        s.close()
    assert n_gain >= 1
    x1, u0, used = a.track(a.last_records[:, :20].contiguous())
    torch.cuda.synchronize()
    n1 = 20 * (N + 1)
    assert np.array_equal(x1.cpu().numpy(), a.last_XU[:, 20:40].cpu().numpy())
    assert np.array_equal(u0.cpu().numpy(), a.last_XU[:, n1:n1 + spec.nu].cpu().numpy())
    assert np.array_equal(used.cpu().numpy(), torch.isfinite(a.last_gain).all(dim=2).all(dim=1).cpu().numpy())
    with pytest.raises(RuntimeError):
        b.track(a.last_records[:, :20].contiguous())


def test_rollout_on_a_single_scene_keeps_a_gain():
    _need_gpu()
    from cmpc_amd.rollout import BatchedRollout
    sc, spec, B, t0 = wl.scene(), ProblemSpec(N=N), 2, 240
    com, dcom = sc.nominal_state(np.full(B, t0))
    a = BatchedRollout(sc, spec, B, device=DEV, gains=True)
    b = BatchedRollout(sc, spec, B, device=DEV)
    for ro in (a, b):
        ro.reset(t0, com, dcom)
        ro.step()
    assert a.solver.last_kernel_name() == "cmpc_solve_pair_gain_kernel<4, 2>"
    assert np.array_equal(_bits(a.state), _bits(b.state)) and np.array_equal(_bits(a.last_XU), _bits(b.last_XU))
    st = a.last_status.cpu().numpy()
    assert (st == 0).any() and torch.isfinite(a.last_gain[torch.from_numpy(st == 0).to(DEV)]).all().item()

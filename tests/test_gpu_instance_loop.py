"""GPU tier: the one instance loop and the launch table behind cmpc_solve_batch_state, _gain and _consts.  Every row of
the table (plain, gain, consts x pair, one-wave 4-vertex, 8-vertex) on the smallest shapes that exercise the loop: the
reported kernel, the gain and the consts launch bit for bit the plain one, a batch larger than the resident grid (workgroups
draw a second ticket) against a small one, and the refusal of one row of constants."""
import dataclasses

import numpy as np
import pytest
import torch

from consts_common import uniform_rows
from cmpc_amd import workloads as wl

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 3
B_BIG = 2048                 # more than the 1792 resident one-wave workgroups of an MI355X (256 CUs x 7)
KERNELS = {"single": 1, "pair": 2}
# case -> (workload, kernel, batch sizes, reported names of the plain / gain / consts launch)
CASES = {
    "nv4-single": ("perturbed", "single", (1, 3, B_BIG),
                   ("cmpc_solve_kernel<4, 1>", "cmpc_solve_gain_kernel<4, 1>", "cmpc_solve_consts_kernel<4, 1>")),
    "nv4-pair": ("perturbed", "pair", (1, 3),
                 ("cmpc_solve_pair_kernel<4, 2>", "cmpc_solve_pair_gain_kernel<4, 2>", "cmpc_solve_pair_consts_kernel<4, 2>")),
    "nv8": ("long_horizon", "single", (1, 3),
            ("cmpc_solve_kernel<8, 2>", "cmpc_solve_gain_kernel<8, 2>", "cmpc_solve_consts_kernel<8, 2>")),
}
VARIANTS = ("plain", "gain", "consts")
_cache = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _launch(s, variant, rec, rows=None):
    """(kernel name, (out, status, iters, kkt, state)) of one launch, as numpy."""
    B = rec.shape[0]
    so = s.new_state(B)
    if variant == "plain":
        r = s.solve(_t(rec), state_out=so)
    elif variant == "gain":
        r = s.solve_with_gain(_t(rec), state_out=so)[:4]
    else:
        r = s.solve_with_consts(_t(rec), _t(uniform_rows(s.spec, B) if rows is None else rows), state_out=so)
    torch.cuda.synchronize()
    return s.last_kernel_name(), tuple(x.cpu().numpy() for x in r) + (so.cpu().numpy(),)


def _case(case):
    """Every launch of a case, once: {(variant, B): (name, arrays)}, plus ("nan", 3): the consts launch with a NaN in row 1."""
    if case not in _cache:
        if not torch.cuda.is_available():
            pytest.fail("GPU tests need a ROCm device: the HIP extension must run, there is no fallback")
        from cmpc_amd.solver import BatchedCentroidalMPC
        name, kernel, sizes, _ = CASES[case]
        spec, rec = wl.make_workload(name, B=max(sizes), N=N)
        s = BatchedCentroidalMPC(dataclasses.replace(spec, kernel=KERNELS[kernel]), device=DEV)
        res = {(v, B): _launch(s, v, rec[:B]) for B in sizes for v in VARIANTS}
        rows = uniform_rows(s.spec, 3)
        rows[1, 1] = float("nan")
        res[("nan", 3)] = _launch(s, "consts", rec[:3], rows)
        s.close()
        _cache[case] = (spec, res)
    return _cache[case]


def _same(a, b, ia=slice(None), ib=slice(None)):
    assert len(a) == len(b) == 5
    for x, y in zip(a, b):
        assert np.array_equal(x[ia], y[ib], equal_nan=True)


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_row_of_the_table_reports_its_kernel(case):
    spec, res = _case(case)
    assert spec.nv == (8 if case == "nv8" else 4)
    for B in CASES[case][2]:
        for v, name in zip(VARIANTS, CASES[case][3]):
            assert res[(v, B)][0] == name, (v, B, res[(v, B)][0])


@pytest.mark.parametrize("case", sorted(CASES))
def test_gain_and_consts_launches_are_bitwise_the_plain_launch(case):
    _, res = _case(case)
    for B in CASES[case][2]:
        plain = res[("plain", B)][1]
        if B == B_BIG:                  # (most of the batch is solved: the comparisons below are not between refusals)
            assert np.isin(plain[1], (0, 3)).mean() > 0.5
        _same(res[("gain", B)][1], plain)
        _same(res[("consts", B)][1], plain)


@pytest.mark.parametrize("variant", VARIANTS)
def test_small_batches_are_rows_of_the_batch_that_takes_second_tickets(variant):
    _, res = _case("nv4-single")
    big = res[(variant, B_BIG)][1]
    _same(res[(variant, 3)][1], big, slice(None), slice(0, 3))
    _same(res[(variant, 1)][1], big, slice(None), slice(0, 1))


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_nan_row_is_refused_and_the_others_are_unchanged(case):
    spec, res = _case(case)
    got, good = res[("nan", 3)][1], res[("consts", 3)][1]
    assert res[("nan", 3)][0] == CASES[case][3][2]
    assert got[1][1] == 2 and got[2][1] == 0 and np.isinf(got[3][1]) and np.isnan(got[0][1]).all()
    _same(got, good, [0, 2], [0, 2])

"""CPU tier: the whole-body QP on HRP-4's own matrices for the first time.  The emulated kernel's J, M, h of the robot
standing at the shipped initial configuration (v = 0, zero errors and feed-forward, the reference's weights) go through
oracle.wbc_qp_oracle with d = 0.05, mu = 0.5; the known answer: the feet share the weight."""
import functools

import numpy as np
import pytest

import rbd_common as rc
from cmpc_amd import rbd
from oracle import wbc_qp_oracle as wq
from wbc_tasks_common import FLAGS, literal_cost

D, MU = 0.05, 0.5


@functools.lru_cache(maxsize=None)
def standing_matrices():
    q = rc.standing()[None, :]
    e = rc.emulate("hrp4", q, np.zeros_like(q))
    sel = rc.model("hrp4").joint_selection(rbd.HRP4_REDUNDANT_DOFS)
    zeros = np.zeros(51)
    assert np.abs(e.jdqd).max() == 0.0                                     # at rest: nothing to fold into the feed-forward
    Hq, Fq = literal_cost(e.J[0], None, zeros, zeros, zeros, None, sel)
    return e.J[0], e.M[0], e.h[0], Hq, Fq


def solve_standing(contact):
    J, M, h, Hq, Fq = standing_matrices()
    fl, fr = FLAGS[contact]
    return wq.solve(Hq, Fq, M, h, np.vstack([fl * J[0:6], fr * J[6:12]]), D, MU)


def test_double_support_shares_the_weight_between_the_feet():
    r = solve_standing("ds")
    m = rc.model("hrp4").total_mass
    fz_l, fz_r = r["f"][5], r["f"][11]                                     # wrench rows: moment 3, force 3, as J's
    print("status", r["status"], "iters", r["iters"], "fz", fz_l, fz_r, "sum - mg", fz_l + fz_r - m * rc.G,
          "max|qdd|", np.abs(r["qdd"]).max())
    assert r["status"] == 0
    assert abs(fz_l + fz_r - m * rc.G) < 1.0
    assert abs(fz_l - fz_r) < 0.1
    assert np.abs(r["qdd"]).max() < 0.1


@pytest.mark.parametrize("contact", ["lfoot", "rfoot"])
def test_single_support_is_solved(contact):
    r = solve_standing(contact)
    print(contact, "status", r["status"], "iters", r["iters"])
    assert r["status"] == 0

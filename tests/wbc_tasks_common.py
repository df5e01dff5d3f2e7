"""What the tests of the task-form whole-body QP share (CPU and GPU tiers): the literal numpy loop of code/
inverse_dynamics.py:98-106 over the stacked task form, and the mixed sample -- instance b of
``wbc_synthetic_tasks(64, seed=21)`` with contact ``CONTACTS[b % 3]`` and (foot_size, mu) = ``FOOT_MU[b % 5]`` -- with the
oracle's answer for each of its instances, computed once and never modified."""
import functools

import numpy as np

from cmpc_amd import wbc, workloads as wl
from oracle import wbc_qp_oracle as wq
from test_wbc_qp import CONTACTS, FOOT_MU

SEED, N_SRC, B_MIXED = 21, 64, 60
ROWS = (6, 6, 3, 3, 3)                                       # lfoot, rfoot, com, torso, base
FLAGS = {"ds": (1.0, 1.0), "lfoot": (1.0, 0.0), "rfoot": (0.0, 1.0)}


def literal_cost(J, Jdot, ff, pe, ve, qd, sel, weights=None, pos_gains=None, vel_gains=None):
    """Hq (30,30), Fq (30,) of one instance: the reference's loop over the six tasks, the joint task with its Jacobian
    diag(sel) and a zero derivative (:52, :65).  Jdot None: no -Jdot qd term."""
    w, kp, kv = (dict(d, **(g or {})) for d, g in ((wbc.WEIGHTS, weights), (wbc.POS_GAINS, pos_gains), (wbc.VEL_GAINS, vel_gains)))
    H, F, r0 = np.zeros((30, 30)), np.zeros(30), 0
    for task, n in zip(wbc.TASKS, ROWS + (30,)):
        rows = slice(r0, r0 + n)
        Jt = J[rows] if task != 'joints' else np.diag(sel)
        acc = ff[rows] + kv[task] * ve[rows] + kp[task] * pe[rows]
        if task != 'joints' and Jdot is not None:
            acc = acc - Jdot[rows] @ qd
        H += w[task] * Jt.T @ Jt
        F += -w[task] * Jt.T @ acc
        r0 += n
    return H, F


@functools.lru_cache(maxsize=None)
def task_instances(B=N_SRC, seed=SEED):
    """(J, Jdot, ff, pe, ve, qd, sel, M, h), read-only (instance b does not depend on B)."""
    arrs = wl.wbc_synthetic_tasks(B, seed=seed)
    for a in arrs:
        a.setflags(write=False)
    return arrs


def params_of(b):
    """(contact name, (flag_l, flag_r), d, mu) of instance b of the mixed sample."""
    c = CONTACTS[b % 3]
    foot_size, mu = FOOT_MU[b % 5]
    return c, FLAGS[c], foot_size / 2, mu


def matrices_of(b, flags, B=N_SRC, **gains):
    """(Hq, Fq, M, h, Jc) of task instance b as the oracle takes them: the literal loop and Jc = flags x J[:12]."""
    J, Jdot, ff, pe, ve, qd, sel, M, h = task_instances(B)
    Hq, Fq = literal_cost(J[b], Jdot[b], ff[b], pe[b], ve[b], qd[b], sel, **gains)
    Jc = np.vstack([flags[0] * J[b, 0:6], flags[1] * J[b, 6:12]])
    return Hq, Fq, M[b], h[b], Jc


@functools.lru_cache(maxsize=None)
def mixed_oracle(b, tol=wq.TOL, max_iter=wq.MAX_ITER):
    _, flags, d, mu = params_of(b)
    return wq.solve(*matrices_of(b, flags), d, mu, tol=tol, max_iter=max_iter)


def kkt_ok(mats, d, mu, qdd, tau30, f):
    """test_wbc_qp._kkt_ok at the GPU tier's thresholds, for one instance given as its matrices."""
    k = wq.kkt_full(*mats, d, mu, qdd, tau30, f, act_tol=1e-4)
    assert k["stationarity"] < 1e-6 and k["equality"] < 1e-7 and k["ineq_violation"] < 1e-8 and k["comp"] < 1e-8, k

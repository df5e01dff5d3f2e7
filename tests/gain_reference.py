"""TEST INFRASTRUCTURE ONLY -- an independent reference of the first-stage gain G = d(x_1, u_0)/dx0.

At a returned point w of an instance (the solution layout of `out_XU`), the multipliers of the literal restatement
oracle/nlp_reference.py are fitted by the bounded least squares of oracle/kkt_certificate.certify (same candidate rows,
same column scaling), the Hessian of its Lagrangian (proximal term at its centre included) comes from torch autograd, and
the strictly active inequality rows are taken as equalities.  The implicit-function system

    [ H   Jc'  Ja' ] [dw ]   [ 0 ]
    [ Jc  0    0   ] [dl ] = [ E ]      E: d/dx0 of -(X[:,0] - x0) = the first 20 equality rows, +I
    [ Ja  0    0   ] [dz ]   [ 0 ]

gives dw/dx0, whose X[:,1] and U[:,0] rows are G.  Nothing here is shared with the C oracle or the kernel: no stage
structure, no Riccati factor, no barrier.

Rows are classified by the fitted multiplier z, the slack -g and the weight of the row as a barrier penalty,
eff = (z / -g) |grad g|^2 / h  against the curvature of the problem (h: the largest diagonal entry of the Hessian):
  strictly active   z >= ZETA * sd, -g <= SLACK and eff >= EFF_HI   (equality in the system)
  inactive          z <  ZETA * sd and -g >  SLACK                  (dropped)
  soft              z >= ZETA * sd and eff < EFF_HI                 (kept as the penalty (z / s) Jg' Jg in H: see below)
  near              z <  ZETA * sd and SOFT_SLACK < -g <= SLACK     (active with a vanishing multiplier in the NLP; in the
                    barrier problem the gain is defined for, a penalty with z = mu / -g, i.e. weight mu / g^2)
  weakly active     z <  ZETA * sd and -g <= SOFT_SLACK             (neither the multiplier nor the slack is resolved:
                    `weak` = True, the instance is not compared; so is an instance whose strictly active rows are not
                    independent of the equalities: there the active-set derivative does not exist)
The slack s of a soft row is -g where the primal point resolves it (-g > SOFT_SLACK); below that, -g is rounding of the
solver's primal residual, and s is the central-path slack mu / z at the barrier value the gain is defined at
(mu = tol / 10, the solver's final barrier value).
The solver's gain is the derivative of its barrier problem, in which every row is a penalty (z/s) |grad g|^2: away from
weakly active rows that is the active-set sensitivity, except for the rows whose penalty is neither large nor small
against h (at the solver's final barrier value, 1e-9, a row needs z |grad g| of order sqrt(1e-3 h) to be hard).  The
last Lyapunov rows of a horizon are typically such rows; they enter the reference as the same penalty, with s = -g and z
from the fit -- still nothing taken from the solver but its primal point.
"""
import numpy as np
import scipy.optimize as so
import torch

from oracle import kkt_certificate as kc
from oracle import nlp_reference as nlp

ZETA = 1e-6
SLACK = 1e-6
EFF_HI = 1e6
SOFT_SLACK = 1e-8


def _multipliers(gradf, Jc, g, Jg):
    """kkt_certificate.certify's bounded least squares: (lam, z over all rows, sd)."""
    nw, ne = gradf.size, Jc.shape[0]
    gn = np.maximum(1.0, np.abs(Jg).max(axis=1))
    act = np.flatnonzero(-g <= kc.ACTIVE_DIST * gn)
    na = act.size
    A = np.zeros((nw + na, ne + na))
    A[:nw, :ne] = Jc.T
    A[:nw, ne:] = Jg[act].T
    A[nw + np.arange(na), ne + np.arange(na)] = np.abs(g[act])
    b = np.concatenate([-gradf, np.zeros(na)])
    lo = np.concatenate([np.full(ne, -np.inf), np.zeros(na)])
    cs = np.maximum(np.sqrt((A * A).sum(axis=0)), 1e-300)
    r = so.lsq_linear(A / cs, b, bounds=(lo, np.full(ne + na, np.inf)), method="bvls", tol=1e-14, lsmr_tol=None,
                      max_iter=None)
    y = r.x / cs
    lam = y[:ne]
    z = np.zeros(g.size)
    z[act] = np.maximum(y[ne:], 0.0)
    mult = np.concatenate([np.abs(lam), z])
    sd = max(100.0, mult.mean()) / 100.0
    return lam, z, sd


def gain(spec, rec, w, u_prox=None):
    """(G (20 + nu, 20), weak, info) at the point w of the instance with record rec; u_prox = the proximal centre
    (the warm XU of the solve, or None for a cold one)."""
    s = kc.nlp_spec(spec)
    par = nlp.unpack_record(s, rec)
    up = kc._uprox(s, u_prox)
    gradf, c, Jc, g, Jg = kc.derivatives(s, rec, w, u_prox)
    lam, z, sd = _multipliers(gradf, Jc, g, Jg)
    lam_t, z_t = torch.tensor(lam), torch.tensor(z)

    def lagr(v):
        return (nlp.cost(s, par, v, up) + lam_t @ nlp.equalities(s, par, v) + z_t @ nlp.inequalities(s, par, v))

    w0 = torch.tensor(np.asarray(w, dtype=np.float64).copy())
    H = torch.autograd.functional.hessian(lagr, w0, vectorize=True).numpy()
    slack = -g
    h = np.abs(np.diag(H)).max()
    eff = z / np.maximum(slack, 1e-300) * (Jg * Jg).sum(axis=1) / h
    big = z >= ZETA * sd
    strict = big & (slack <= SLACK) & (eff >= EFF_HI)
    soft = big & ~strict
    near = ~big & (slack <= SLACK) & (slack > SOFT_SLACK)
    weak_rows = ~big & (slack <= SOFT_SLACK)
    mu = float(getattr(spec, "tol", 1e-8)) / 10
    ss = np.where(slack > SOFT_SLACK, slack, mu / np.maximum(z, 1e-300))
    wgt = np.where(soft, z / ss, 0.0) + np.where(near, mu / np.maximum(slack, 1e-300) ** 2, 0.0)
    pen = soft | near
    H = H + Jg[pen].T @ (wgt[pen][:, None] * Jg[pen])
    Ja = Jg[strict]
    nw, ne, na = w0.numel(), Jc.shape[0], Ja.shape[0]
    K = np.zeros((nw + ne + na, nw + ne + na))
    K[:nw, :nw] = H
    K[:nw, nw:nw + ne] = Jc.T
    K[nw:nw + ne, :nw] = Jc
    K[:nw, nw + ne:] = Ja.T
    K[nw + ne:, :nw] = Ja
    rhs = np.zeros((nw + ne + na, nlp.NX))
    rhs[nw:nw + nlp.NX, :] = np.eye(nlp.NX)           # c_0 = X[:,0] - x0: d/dx0 = -I, moved to the right
    try:
        sol = np.linalg.solve(K, rhs)
    except np.linalg.LinAlgError:             # the strictly active rows are not independent of the equalities (LICQ fails,
        sol = np.full((K.shape[0], nlp.NX), np.nan)    # e.g. a box row on a stance foot that x0 pins): no active-set derivative
    dw = sol[:nw]
    NX = nlp.NX
    G = np.concatenate([dw[NX:2 * NX], dw[NX * (s.N + 1):NX * (s.N + 1) + s.nu]], axis=0)
    info = dict(sd=sd, n_strict=int(strict.sum()), n_soft=int(soft.sum()), n_near=int(near.sum()),
                n_weak=int(weak_rows.sum()))
    return G, bool(weak_rows.any()) or not np.isfinite(G).all(), info


def rel_err_groups(G, Gref, nv):
    """max|G - Gref| / max(1, max|Gref|) per row group: x_1, forces, foot velocities."""
    nf = 6 * nv
    groups = dict(x1=slice(0, 20), forces=slice(20, 20 + nf), feet=slice(20 + nf, 20 + nf + 8))
    return {k: float(np.abs(G[sl] - Gref[sl]).max() / max(1.0, np.abs(Gref[sl]).max())) for k, sl in groups.items()}

"""TEST INFRASTRUCTURE ONLY -- an independent KKT certificate of a primal point.

Given a point w of the NLP in the solution layout (X (20 x (N+1)) then U (nu x N), what `out_XU` holds), `certify` measures
how well w meets the first-order optimality conditions of the literal restatement oracle/nlp_reference.py (autograd
derivatives, no stage structure).  It shares no code with the C oracle or the HIP solver: neither its derivatives, nor its
multipliers, nor its error measure.  The solvers report a scaled KKT error `kkt` for their answer; this module checks that
number from the outside.

  primal         max(|c(w)|_inf, max_i g_i(w)+)         equalities c = 0 and inequalities g <= 0 as the restatement states
                                                         them, with IPOPT's bound_relax_factor (spec.relax) applied
  multipliers    (lam, z) = argmin |grad f + Jc' lam + Jg' z|^2 + |diag(g) z|^2   over lam free, z >= 0
                 (scipy.optimize.lsq_linear, bounded least squares).  z is a free variable only on the rows whose bound is
                 within ACTIVE_DIST of w, measured along the row's own gradient (-g_i <= ACTIVE_DIST * max(1, |grad g_i|_inf));
                 the other rows get z = 0.  Their true multipliers are small: s_i z_i <= e_c at the solver's point, so a
                 dropped row moves the stationarity residual by at most e_c / ACTIVE_DIST.
  stationarity   |grad f + Jc' lam + Jg' z|_inf / sd
  complementarity max_i z_i |g_i| / sd
  kappa_ind      max of the three

sd is the solvers' own scale of the dual error (oracle/cmpc_oracle.c, `sd = fmax(100.0, sum_mult / n_mult) / 100.0`, the
kernel's copy in csrc/cmpc_kernel.hpp; oracle/ipm_dense.py uses the same rule): the mean absolute multiplier over the
multipliers of the problem, floored at 100, over 100.  Here the mean runs over the fitted (lam, z).

The cost includes the proximal term 0.5 * rho * |U - u_prox|^2 around the solver's proximal centre: the caller's warm
U, or 0 for a cold solve.  u_prox is given as (nu, N) or in the layout of U inside w (nu * N values, stage-major).
"""
import numpy as np
import scipy.optimize as so
import torch

from . import nlp_reference as nlp

#: rows whose bound lies within this distance of the point (in units of the row's gradient) carry a multiplier
ACTIVE_DIST = 1.0

_SPEC_FIELDS = ("delta", "g", "k1", "k2", "w_rate", "prox", "relax", "w_hw", "w_cxy", "w_foot", "w_force", "w_cz_const",
                "cz_max")


def nlp_spec(spec):
    """nlp_reference.Spec with the constants of `spec` (a ProblemSpec, a ctypes cmpc_spec or an nlp_reference.Spec)."""
    if isinstance(spec, nlp.Spec):
        return spec
    fl, fw = getattr(spec, "foot_length", 0.25), getattr(spec, "foot_width", 0.13)
    s = nlp.Spec(N=int(spec.N), nv=int(spec.nv), foot_length=float(fl), foot_width=float(fw))
    for f in _SPEC_FIELDS:
        if hasattr(spec, f):
            setattr(s, f, float(getattr(spec, f)))
    if hasattr(spec, "box"):
        s.box = tuple(float(b) for b in spec.box)
    return s


def _uprox(s, u_prox):
    if u_prox is None:
        return None
    up = np.asarray(u_prox, dtype=np.float64)
    if up.shape == (s.nu, s.N):
        return up
    up = up.reshape(-1)
    if up.size == nlp.NX * (s.N + 1) + s.nu * s.N:      # a whole warm start: its U part
        up = up[nlp.NX * (s.N + 1):]
    return up.reshape(s.N, s.nu).T.copy()


def derivatives(spec, rec, w, u_prox=None):
    """(grad f, c, Jc, g, Jg) of the restatement at w (torch autograd, fp64)."""
    s = nlp_spec(spec)
    par = nlp.unpack_record(s, rec)
    up = _uprox(s, u_prox)
    wt = torch.tensor(np.asarray(w, dtype=np.float64).copy(), requires_grad=True)
    f = nlp.cost(s, par, wt, up)
    gradf = torch.autograd.grad(f, wt)[0].numpy()
    w0 = wt.detach()
    c = nlp.equalities(s, par, w0).numpy()
    g = nlp.inequalities(s, par, w0).numpy()
    Jc = torch.autograd.functional.jacobian(lambda v: nlp.equalities(s, par, v), w0, vectorize=True).numpy()
    Jg = torch.autograd.functional.jacobian(lambda v: nlp.inequalities(s, par, v), w0, vectorize=True).numpy()
    return gradf, c, Jc, g, Jg


def certify(spec, rec, w, u_prox=None):
    """dict(primal, stationarity, complementarity, kappa_ind, sd, n_active) of the point w (see the module docstring)."""
    gradf, c, Jc, g, Jg = derivatives(spec, rec, w, u_prox)
    nw, ne = gradf.size, c.size
    primal = max(np.abs(c).max(), max(0.0, g.max()))
    gn = np.maximum(1.0, np.abs(Jg).max(axis=1))
    act = np.flatnonzero(-g <= ACTIVE_DIST * gn)
    na = act.size
    # columns: lam (ne, free), z (na, >= 0);  rows: stationarity (nw), complementarity (na)
    A = np.zeros((nw + na, ne + na))
    A[:nw, :ne] = Jc.T
    A[:nw, ne:] = Jg[act].T
    A[nw + np.arange(na), ne + np.arange(na)] = np.abs(g[act])
    b = np.concatenate([-gradf, np.zeros(na)])
    lo = np.concatenate([np.full(ne, -np.inf), np.zeros(na)])
    # (column scaling: the multipliers of the dynamics reach 1e3 .. 1e4, those of the box rows 1e5; lsq_linear converges on
    # the scaled problem and the residual is formed again from the unscaled data below)
    cs = np.maximum(np.sqrt((A * A).sum(axis=0)), 1e-300)
    r = so.lsq_linear(A / cs, b, bounds=(lo, np.full(ne + na, np.inf)), method="bvls", tol=1e-14, lsmr_tol=None,
                      max_iter=None)
    y = r.x / cs
    lam, z = y[:ne], np.maximum(y[ne:], 0.0)
    rd = gradf + Jc.T @ lam + Jg[act].T @ z
    mult = np.concatenate([np.abs(lam), z, np.zeros(g.size - na)])   # (every row of the problem counts, as in the solvers)
    sd = max(100.0, mult.mean()) / 100.0
    stat = np.abs(rd).max() / sd
    comp = (z * np.abs(g[act])).max() / sd if na else 0.0
    return dict(primal=float(primal), stationarity=float(stat), complementarity=float(comp),
                kappa_ind=float(max(primal, stat, comp)), sd=float(sd), n_active=int(na))


# ---------------------------------------------------------------------------------------------------------------------
# Many points at once: a `spawn` pool of CPU-only workers (no GPU runtime in them: HIP_VISIBLE_DEVICES is empty when they
# start, and they import this module, numpy, scipy and torch alone).  One autograd Jacobian of an N = 20 instance takes
# about a second on one core.

MAX_WORKERS = 8


def _worker_init():
    torch.set_num_threads(1)


def _job(args):
    return certify(*args)


def certify_many(spec, recs, ws, u_prox=None, workers=None):
    """[certify(spec, recs[i], ws[i], u_prox[i])] over a process pool of at most MAX_WORKERS workers."""
    import multiprocessing as mp
    import os
    s = nlp_spec(spec)                          # (a plain class of oracle/: what the workers unpickle)
    n = len(ws)
    ups = [None] * n if u_prox is None else [None if u is None else np.asarray(u) for u in u_prox]
    jobs = [(s, np.asarray(recs[i]), np.asarray(ws[i]), ups[i]) for i in range(n)]
    if workers is None:
        ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        workers = min(MAX_WORKERS, ncpu, n)
    workers = max(1, min(MAX_WORKERS, workers))
    if workers == 1 or n <= 1:
        return [_job(j) for j in jobs]
    saved = {k: os.environ.get(k) for k in ("HIP_VISIBLE_DEVICES", "OMP_NUM_THREADS")}
    os.environ["HIP_VISIBLE_DEVICES"], os.environ["OMP_NUM_THREADS"] = "", "1"
    try:
        with mp.get_context("spawn").Pool(workers, initializer=_worker_init) as pool:
            return pool.map(_job, jobs, chunksize=1)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

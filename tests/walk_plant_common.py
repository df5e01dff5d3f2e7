"""What the tests of the contact plant share (cmpc_walk_plant_step; CPU and GPU tiers): the emulated device source
(tests/emu/walk_plant_emu.cpp through ctypes), a dense numpy restatement of the step written from include/cmpc_walk.h
(``numpy.linalg.solve``, plain loops, scipy's rotations -- nothing of the kernel's), the 16-robot mix the two are compared
on, the standing robot with the torques that hold it still, and the batch of rows that must not move.  Built once and never
modified."""
import collections
import ctypes
import functools

import numpy as np
from scipy.spatial.transform import Rotation

import build as _build
import rbd_common as rc

Stepped = collections.namedtuple("Stepped", "q v impulse status residual")
FILL = 12345.0
DT, HALF = 0.01, 0.05
#: corner k of a foot: the signs of (x, y)
CORNERS = ((1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0))


class Params(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("sweeps", ctypes.c_int32), ("dt", ctypes.c_double), ("ground_z", ctypes.c_double),
                ("erp", ctypes.c_double), ("cfm", ctypes.c_double)]


def params(sweeps=50, dt=DT, ground_z=0.0, erp=0.2, cfm=0.0, struct_size=None):
    return Params(ctypes.sizeof(Params) if struct_size is None else struct_size, sweeps, dt, ground_z, erp, cfm)


@functools.lru_cache(maxsize=None)
def emu_lib():
    lib = ctypes.CDLL(_build.build_emu_walk_plant())
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.cmpc_emu_walk_plant_step.argtypes = [i32] + [vp] * 7 + [i32, vp, vp, vp, ctypes.POINTER(Params)] + [vp] * 5
    lib.cmpc_emu_walk_plant_step.restype = ctypes.c_int
    lib.cmpc_emu_walk_plant_last_error.restype = ctypes.c_char_p
    return lib


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def emulate_plant(case, prm, in_place=False, tau_ld=24, outputs=("impulse", "status", "residual"), null=()):
    """The emulated ``cmpc_walk_plant_step`` on copies of the case's arrays -> ``Stepped`` of numpy (None where not asked
    for; status and residual are pre-filled); raises ValueError with the validation's message.  case: a dict of q, v, M,
    h, J, pose, foot_mu and optionally tau (B,24), ext, hold, impulse (the warm start); ``null``: names passed as NULL."""
    B = np.shape(case["q"])[0]
    a = {k: (None if k in null or case.get(k) is None else np.array(case[k], dtype=np.uint8 if k == "hold" else np.float64, order="C"))
         for k in ("q", "v", "M", "h", "J", "pose", "tau", "ext", "foot_mu", "hold", "impulse")}
    if a["tau"] is not None and tau_ld > 24:
        wide = np.full((B, tau_ld), FILL)
        wide[:, :24] = a["tau"]
        a["tau"] = wide
    if "impulse" not in outputs:
        a["impulse"] = None
    elif a["impulse"] is None:
        a["impulse"] = np.zeros((B, 24))
    q_out, v_out = (a["q"], a["v"]) if in_place else (np.full((B, 30), FILL), np.full((B, 30), FILL))
    if "q_out" in null:
        q_out = None
    status = np.full(B, -7, np.int32) if "status" in outputs else None
    residual = np.full(B, FILL) if "residual" in outputs else None
    ptr = lambda x: None if x is None else x.ctypes.data
    r = emu_lib().cmpc_emu_walk_plant_step(B, ptr(a["q"]), ptr(a["v"]), ptr(a["M"]), ptr(a["h"]), ptr(a["J"]), ptr(a["pose"]),
                                           ptr(a["tau"]), tau_ld, ptr(a["ext"]), ptr(a["foot_mu"]), ptr(a["hold"]),
                                           None if prm is None else ctypes.byref(prm), ptr(a["impulse"]), ptr(q_out), ptr(v_out),
                                           ptr(status), ptr(residual))
    if r != 0:
        raise ValueError(emu_lib().cmpc_emu_walk_plant_last_error().decode())
    return Stepped(q_out, v_out, a["impulse"], status, residual)


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def skew(r):
    return np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]])


def contact_rows(J, pose, half, ground_z=0.0):
    """(Jc (24,30), phi (8,)) of one robot: the world-frame linear Jacobians and heights of the eight sole vertices."""
    Jc, phi = np.zeros((24, 30)), np.zeros(8)
    for f in range(2):
        Rf, pf = Rotation.from_rotvec(np.array(pose[6 * f:6 * f + 3])).as_matrix(), pose[6 * f + 3:6 * f + 6]
        for k, (sx, sy) in enumerate(CORNERS):
            i = 4 * f + k
            r = Rf @ np.array([sx * half, sy * half, 0.0])
            Jc[3 * i:3 * i + 3] = J[6 * f + 3:6 * f + 6] - skew(r) @ J[6 * f:6 * f + 3]
            phi[i] = (pf + r)[2] - ground_z
    return Jc, phi


def admissible(p, mu):
    p = np.array(p, dtype=np.float64)
    for i in range(8):
        p[3 * i + 2] = max(0.0, p[3 * i + 2])
        hyp, lim = np.hypot(p[3 * i], p[3 * i + 1]), mu * p[3 * i + 2]
        if hyp > lim:
            p[3 * i:3 * i + 2] *= (lim / hyp if lim > 0.0 else 0.0)
    return p


def restate_one(q, v, M, h, J, pose, tau, ext, half, mu, warm, sweeps, dt=DT, ground_z=0.0, erp=0.2, cfm=0.0):
    """One robot's step, dense -> (q+, v+, p, residual, margins), margins = the smallest |p_n| among the p_n updates that
    landed off zero and the smallest |hypot - mu p_n| / (mu p_n): how far the run stayed from a tie of its branches."""
    R = Rotation.from_rotvec(np.array(q[0:3])).as_matrix()
    g = np.concatenate([R.T @ ext[0:3], R.T @ ext[3:6], tau]) - h
    v_free = v + dt * np.linalg.solve(M, g)
    Jc, phi = contact_rows(J, pose, half, ground_z)
    Y = np.linalg.solve(M, Jc.T)
    W = Jc @ Y + cfm * np.eye(24)
    c = Jc @ v_free
    c[2::3] += np.where(phi >= 0.0, phi, erp * phi) / dt
    p = admissible(warm, mu)
    tie_n, tie_cone = np.inf, np.inf
    for _ in range(sweeps):
        for i in range(8):
            n = 3 * i + 2
            t = p[n] - (W[n] @ p + c[n]) / W[n, n]
            tie_n = min(tie_n, abs(t))
            p[n] = max(0.0, t)
            for a in (3 * i, 3 * i + 1):
                p[a] = p[a] - (W[a] @ p + c[a]) / W[a, a]
            hyp, lim = np.hypot(p[3 * i], p[3 * i + 1]), mu * p[n]
            if lim > 0.0:
                tie_cone = min(tie_cone, abs(hyp - lim) / lim)
            if hyp > lim:
                p[3 * i:3 * i + 2] *= (lim / hyp if lim > 0.0 else 0.0)
    u = W @ p + c
    residual = max(0.0, float(np.max(-u[2::3])))
    vn = v_free + Y @ p
    Rn = Rotation.from_matrix(R) * Rotation.from_rotvec(dt * vn[0:3])
    qn = np.concatenate([Rn.as_rotvec(), q[3:6] + dt * R @ vn[3:6], q[6:] + dt * vn[6:]])
    return qn, vn, p, residual, (tie_n, tie_cone)


def restate(case, sweeps, **kw):
    B = case["q"].shape[0]
    out = [restate_one(case["q"][b], case["v"][b], case["M"][b], case["h"][b], case["J"][b], case["pose"][b],
                       np.zeros(24) if case.get("tau") is None else case["tau"][b],
                       np.zeros(6) if case.get("ext") is None else case["ext"][b], case["foot_mu"][b, 0], case["foot_mu"][b, 1],
                       np.zeros(24) if case.get("impulse") is None else case["impulse"][b], sweeps, **kw) for b in range(B)]
    return (Stepped(np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out]), np.zeros(B, np.int32),
                    np.array([o[3] for o in out])), np.array([o[4] for o in out]))


# ---- cases --------------------------------------------------------------------------------------------------------------------
def evaluated(q, v, **more):
    """The case dict of robots at (q, v): the emulated ``rbd_eval`` of HRP-4 there, and what ``more`` adds."""
    ev = rc.emulate("hrp4", q, v, outputs=("J", "M", "h", "pose"))
    case = dict(q=np.array(q), v=np.array(v), M=ev.M, h=ev.h, J=ev.J, pose=ev.pose)
    case.update(more)
    case.setdefault("foot_mu", np.tile([HALF, 0.5], (np.shape(q)[0], 1)))
    return case


def lowest_vertex(q):
    """Height of the lowest sole vertex of every robot at q (B,30)."""
    pose = rc.emulate("hrp4", q, np.zeros_like(q), outputs=("pose",)).pose
    return np.array([contact_rows(np.zeros((21, 30)), p, HALF)[1].min() for p in pose])


def frozen(case):
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def mix_case(seed=0):
    """16 robots, read-only: eight draws of ``rc.sample('hrp4')`` lowered so that their lowest sole vertex is within +-1 cm
    of the floor, four at ``rc.standing()`` with random v, four in free flight; random tau, ext, mu in [0.3, 0.9] and a
    random (not yet admissible) warm start."""
    rng = np.random.default_rng([71, seed])
    qs, vs = rc.sample("hrp4", 8)
    q, v = np.zeros((16, 30)), np.zeros((16, 30))
    q[0:8], v[0:8] = qs, vs
    q[0:8, 5] -= lowest_vertex(q[0:8]) - rng.uniform(-0.01, 0.01, size=8)
    q[8:12] = rc.standing()
    v[8:12] = 0.3 * rng.normal(size=(4, 30))
    q[12:16] = qs[3:7]
    q[12:16, 5] += 1.0 - np.minimum(lowest_vertex(q[12:16]), 0.0)
    v[12:16] = vs[3:7]
    foot_mu = np.stack([np.full(16, HALF), rng.uniform(0.3, 0.9, size=16)], axis=1)
    return frozen(evaluated(q, v, tau=5.0 * rng.normal(size=(16, 24)), ext=10.0 * rng.normal(size=(16, 6)), foot_mu=foot_mu,
                            impulse=0.05 * rng.normal(size=(16, 24))))


def total_mass():
    return rc.model("hrp4").total_mass


@functools.lru_cache(maxsize=None)
def static_case(lift=0.0):
    """One robot at ``rc.standing()`` (raised by ``lift``) at rest, with the torques that hold it still on the floor: f the
    least-squares solution of Jc'[:6] f = h[:6], tau = (h - Jc' f)[6:].  Read-only; the forces are kept under 'f'."""
    q = np.array(rc.standing())[None]
    q[0, 5] += lift
    case = evaluated(q, np.zeros((1, 30)))
    Jc, _ = contact_rows(case["J"][0], case["pose"][0], HALF)
    f = np.linalg.lstsq(Jc.T[:6], case["h"][0, :6], rcond=None)[0]
    case["tau"] = (case["h"][0] - Jc.T @ f)[None, 6:]
    case["f"] = f
    return frozen(case)


def tile(case, idx):
    return {k: (a[idx] if isinstance(a, np.ndarray) and a.shape[0] == case["q"].shape[0] and k != "f" else a) for k, a in case.items()}


BAD_KINDS = ("hold", "NaN in q", "NaN in v", "NaN in M", "NaN in h", "NaN in J", "NaN in pose", "NaN in tau", "NaN in ext",
             "NaN in impulse", "foot_mu 0", "foot_mu -1", "negative pivot")
BAD_ROW = 5


@functools.lru_cache(maxsize=None)
def bad_case(kind):
    """(clean, bad): eight robots of the mix (contact, standing and flying ones), and the same with ``kind`` at row BAD_ROW.
    'negative pivot': every entry of row 7 and of column 7 of M negated once, the diagonal with them (negating the row and
    then the column would put the diagonal back and leave M positive definite)."""
    clean = tile(mix_case(), np.array([0, 1, 8, 12, 2, 3, 9, 13]))
    clean["hold"] = np.zeros(8, np.uint8)
    bad = {k: np.array(a) for k, a in clean.items()}
    b = BAD_ROW
    if kind == "hold":
        bad["hold"][b] = 1
    elif kind.startswith("NaN in "):
        a = bad[kind[7:]][b]
        a.reshape(-1)[a.size - 1 if kind[7:] in ("M", "J", "pose") else a.size // 2] = np.nan
    elif kind == "foot_mu 0":
        bad["foot_mu"][b, 1] = 0.0
    elif kind == "foot_mu -1":
        bad["foot_mu"][b, 0] = -1.0
    elif kind == "negative pivot":
        d = bad["M"][b, 7, 7]
        bad["M"][b, 7, :] *= -1.0
        bad["M"][b, :, 7] *= -1.0
        bad["M"][b, 7, 7] = -d
    else:
        raise ValueError(kind)
    return frozen(clean), frozen(bad)


def check_bad_row(kind, run):
    """The rules of include/cmpc_walk.h on ``bad_case(kind)``; run(case) -> ``Stepped`` (the GPU tier runs it too)."""
    clean, bad = bad_case(kind)
    want, got = run(clean), run(bad)
    b = BAD_ROW
    assert (want.status == 0).all()
    assert got.status[b] == (1 if kind == "hold" else 2), (kind, got.status)
    assert bits_equal(got.q[b], bad["q"][b]) and bits_equal(got.v[b], bad["v"][b]), kind
    if kind == "hold":
        assert bits_equal(got.impulse[b], bad["impulse"][b])
    else:
        assert bits_equal(got.impulse[b], np.zeros(24))
    rest = np.delete(np.arange(8), b)
    assert (got.status[rest] == 0).all()
    for k in ("q", "v", "impulse", "residual"):
        assert bits_equal(getattr(got, k)[rest], getattr(want, k)[rest]), (kind, k)
    return got


def cone_ok(impulse, mu):
    """Every vertex: p_n >= 0 and hypot(p_x, p_y) <= mu p_n (1 + 1e-12)."""
    p = np.asarray(impulse).reshape(-1, 8, 3)
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64).reshape(-1, 1), p.shape[:2])
    return bool((p[..., 2] >= 0.0).all() and (np.hypot(p[..., 0], p[..., 1]) <= mu * p[..., 2] * (1 + 1e-12)).all())

"""What the tests of the measurement that closes the walking loop share (cmpc_walk_measure; CPU and GPU tiers): the emulated
device source (tests/emu/walk_measure_emu.cpp through ctypes), its numpy restatement, the batch with rows that must not be
fed back, and the standing robots and start tick at which the closed loop is started.  Built once and never modified."""
import collections
import ctypes
import functools

import numpy as np

import build as _build
import rbd_common as rc
from cmpc_amd import workloads as wl
from scenes_common import five_scenes

Measured = collections.namedtuple("Measured", "state alive x_meas innovation")
FILL = 12345.0
#: the guards of the bad-row batch: CoM height, and the base's tilt from the vertical in radians
Z_MIN, TILT_MAX = 0.4, 0.5
#: the closed-loop cases: six robots, N = 10, started one tick before the plan write-back of the first step may fire
B_LOOP, N_LOOP, RATE_SCALE = 6, 10, 0.1


@functools.lru_cache(maxsize=None)
def emu_lib():
    lib = ctypes.CDLL(_build.build_emu_walk_measure())
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    lib.cmpc_emu_walk_measure.argtypes, lib.cmpc_emu_walk_measure.restype = [i32, vp, vp, f64, f64, vp, vp, vp, vp], ctypes.c_int
    lib.cmpc_emu_walk_measure_last_error.restype = ctypes.c_char_p
    return lib


def emulate_measure(centroid, pose, state, alive=None, z_min=-np.inf, cos_tilt_min=-np.inf, outputs=("x_meas", "innovation")):
    """The emulated ``cmpc_walk_measure`` on copies of state and alive -> ``Measured`` of numpy (None where not asked for;
    the outputs are pre-filled with FILL); raises ValueError with the validation's message.  state=None passes NULL."""
    B = np.shape(centroid)[0]
    cen, pose = (np.ascontiguousarray(a, dtype=np.float64) for a in (centroid, pose))
    state = None if state is None else np.array(state, dtype=np.float64, order="C")
    alive = None if alive is None else np.array(alive, dtype=np.uint8, order="C")
    xm = np.full((B, 20), FILL) if "x_meas" in outputs else None
    inn = np.full((B, 9), FILL) if "innovation" in outputs else None
    ptr = lambda a: None if a is None else a.ctypes.data
    r = emu_lib().cmpc_emu_walk_measure(B, ptr(cen), ptr(pose), z_min, cos_tilt_min, ptr(state), ptr(alive), ptr(xm), ptr(inn))
    if r != 0:
        raise ValueError(emu_lib().cmpc_emu_walk_measure_last_error().decode())
    return Measured(state, alive, xm, inn)


def mirror_measure(centroid, pose, state):
    """The rows of a robot that is fed back, by numpy: the reference's ``current_state`` (its 20 words before the plan
    overwrites the foot positions: CoM, its velocity, the momentum, the MPC's own theta_hat, and per foot the third angle,
    x, y of its pose and a 0), the state with the measured words in it, and measured minus predicted."""
    s = np.array(state)
    x = np.zeros((s.shape[0], 20))
    x[:, 0:9], x[:, 9:12] = centroid, s[:, 9:12]
    x[:, 12:15], x[:, 16:19] = pose[:, 2:5], pose[:, 8:11]
    inn = centroid - s[:, 0:9]
    s[:, 0:9], s[:, 12], s[:, 13] = centroid, pose[:, 2], pose[:, 8]
    return Measured(s, None, x, inn)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@functools.lru_cache(maxsize=None)
def mirror_case(name, B):
    """(centroid, pose, state) on the evaluations of ``rc.emulated(name, B)`` with a random state.  Read-only."""
    ev = rc.emulated(name, B)
    state = np.random.default_rng([rc.MODELS.index(name), 41, B]).normal(size=(B, 16))
    state.setflags(write=False)
    return ev.centroid, ev.pose, state


BAD_KINDS = ("alive = 0", "NaN in centroid", "Inf in pose", "CoM below z_min", "tilted past tilt_max")


@functools.lru_cache(maxsize=None)
def bad_case(kind, B=18):
    """A batch in which every robot would be fed back (CoM 0.6..0.9 high, base within 0.2 rad of upright), and the same with
    one of the BAD_KINDS at rows 0, B // 2 and B - 1: (clean, bad, rows), the first two dicts of centroid, pose, state,
    alive.  Read-only."""
    rng = np.random.default_rng([43, B])
    cen, pose, state = rng.normal(size=(B, 9)), rng.normal(size=(B, 21)), rng.normal(size=(B, 16))
    cen[:, 2] = rng.uniform(0.6, 0.9, size=B)
    w = rng.normal(size=(B, 3))
    pose[:, 18:21] = w / np.linalg.norm(w, axis=1)[:, None] * rng.uniform(0.0, 0.2, size=(B, 1))
    clean = dict(centroid=cen, pose=pose, state=state, alive=np.ones(B, np.uint8))
    bad = {k: a.copy() for k, a in clean.items()}
    rows = (0, B // 2, B - 1)
    for i, b in enumerate(rows):
        if kind == "alive = 0":
            bad["alive"][b] = 0
        elif kind == "NaN in centroid":
            bad["centroid"][b, (0, 4, 8)[i]] = np.nan
        elif kind == "Inf in pose":
            bad["pose"][b, (0, 13, 20)[i]] = (np.inf, -np.inf, np.inf)[i]
        elif kind == "CoM below z_min":
            bad["centroid"][b, 2] = (Z_MIN - 1e-3, Z_MIN, -1.0)[i]          # (at z_min is not above it)
        elif kind == "tilted past tilt_max":
            bad["pose"][b, 18:21] = ((TILT_MAX + 0.05, 0.0, 0.3), (0.0, -2.0, 0.0), (1.0, 1.0, 1.0))[i]
        else:
            raise ValueError(kind)
    for d in (clean, bad):
        for a in d.values():
            a.setflags(write=False)
    return clean, bad, rows


# ---- the closed loop ----------------------------------------------------------------------------------------------------------
def start_tick(scene, N=N_LOOP):
    """One tick before the first tick at which the plan write-back may fire (``rollout_schedule``'s cond): late in the
    first single support (tick 260 of the shipped walk)."""
    return int(np.nonzero(wl.rollout_schedule(scene, N)[0])[0][0]) - 1


@functools.lru_cache(maxsize=None)
def standing_robots(B=B_LOOP):
    """(q, v) (B,30), read-only: HRP-4 standing (``rc.standing()``), every robot its own arms, and small joint rates of its
    own so that the momentum about the CoM is not zero (a resting robot in late single support is an
    infeasible MPC instance)."""
    rng = np.random.default_rng(9)
    q = np.tile(rc.standing(), (B, 1))
    q[:, 22:30] += rng.uniform(-0.05, 0.05, size=(B, 8))
    v = np.zeros_like(q)
    v[:, 6:] = RATE_SCALE * rng.normal(size=(B, 24))
    q.setflags(write=False)
    v.setflags(write=False)
    return q, v


def loop_mass():
    return rc.model("hrp4").total_mass


def loop_mu(B=B_LOOP):
    return np.array([0.3, 0.3, 0.5, 0.5, 0.9, 0.9])[:B]


def shipped():
    return five_scenes()[0]

"""What the tests of the batched rigid-body model share (CPU and GPU tiers): the three models -- HRP-4 from
tests/golden/hrp4.urdf, a 24-joint serial chain (depth 24, the worst case for the kernel's level loops) and a star with 24
joints on the base, the last two authored here with random axes, placements and inertias --, the drawn instances, the
emulated device source (tests/emu/rbd_emu.cpp through ctypes) and the reference's answers, computed once per model and
never modified."""
import ctypes
import functools
import os

import numpy as np
from scipy.spatial.transform import Rotation

import build as _build
import rbd_reference as ref
from cmpc_amd import rbd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
URDF = os.path.join(ROOT, "tests", "golden", "hrp4.urdf")
MODELS = ("hrp4", "chain", "star")
G = 9.81
FIELDS = rbd.Evaluation._fields
SHAPES = dict(J=(21, 30), jdqd=(21,), M=(30, 30), h=(30,), pose=(21,), vel=(21,), centroid=(9,))
#: the level every output is held to: 1e-9 x max(1, largest |entry| of that output).  fp64 rounding of <~1e3 chained
#: operations is <~1e-12: three orders of margin, no measurement behind it.
LEVEL = 1e-9


def _authored(topology, seed):
    rng = np.random.default_rng(seed)
    parent = np.array([-1] + [(i - 1 if topology == "chain" else 0) for i in range(1, 25)], dtype=np.int32)
    joint_R = np.stack([np.eye(3)] + [Rotation.from_rotvec(rng.normal(size=3)).as_matrix() for _ in range(24)])
    joint_p = rng.uniform(-0.2, 0.2, size=(25, 3))
    axis = rng.normal(size=(25, 3))
    mass = rng.uniform(0.3, 2.0, size=25)
    com = rng.uniform(-0.1, 0.1, size=(25, 3))
    inertia = np.zeros((25, 6))
    for i in range(25):
        A = rng.normal(size=(3, 3))
        I = 0.01 * (A @ A.T + 0.5 * np.eye(3))
        inertia[i] = (I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2])
    frame_body = np.array([24, 12, 6, 0], dtype=np.int32)
    frame_R = np.stack([Rotation.from_rotvec(0.3 * rng.normal(size=3)).as_matrix() for _ in range(4)])
    frame_p = rng.uniform(-0.1, 0.1, size=(4, 3))
    return rbd.RobotModel(parent, joint_R, joint_p, axis, mass, com, inertia, frame_body, frame_R, frame_p)


@functools.lru_cache(maxsize=None)
def model(name):
    if name == "hrp4":
        return rbd.RobotModel.from_urdf(URDF)
    return _authored(name, seed={"chain": 101, "star": 202}[name])


@functools.lru_cache(maxsize=None)
def raw_tree(name):
    """The tree the reference works on: for HRP-4 the raw URDF, all 55 links."""
    if name == "hrp4":
        return ref.tree_from_urdf(URDF, rbd.DEFAULT_FRAMES)
    return ref.tree_from_model(model(name))


@functools.lru_cache(maxsize=None)
def standing():
    """HRP-4 at the shipped initial configuration (code/simulation.py:63-77), soles' midpoint at the world origin."""
    m = model("hrp4")
    q = m.place_on_ground(m.configuration(rbd.HRP4_INITIAL_DEG, degrees=True))
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def sample(name, B=8):
    """(q, v) (B,30), read-only; instance b does not depend on B.  Joint angles within 0.5 rad of a nominal, base rotation
    angle up to 1 rad -- instance 1 at exactly 0, instance 2 at 1e-10 --, v ~ N(0, 0.5)."""
    nominal = standing() if name == "hrp4" else np.zeros(30)
    q, v = np.zeros((B, 30)), np.zeros((B, 30))
    for b in range(B):
        rng = np.random.default_rng([MODELS.index(name), 7, b])
        d = rng.normal(size=3)
        angle = 0.0 if b == 1 else 1e-10 if b == 2 else rng.uniform(0.05, 1.0)
        q[b, 0:3] = angle * d / np.linalg.norm(d)
        q[b, 3:6] = nominal[3:6] + rng.uniform(-0.5, 0.5, size=3)
        q[b, 6:] = nominal[6:] + rng.uniform(-0.5, 0.5, size=24)
        v[b] = rng.normal(scale=0.5, size=30)
    q.setflags(write=False)
    v.setflags(write=False)
    return q, v


@functools.lru_cache(maxsize=None)
def reference(name, B=8):
    q, v = sample(name, B)
    out = ref.evaluate_batch(raw_tree(name), q, v, G)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def emu_lib():
    lib = ctypes.CDLL(_build.build_emu_rbd())
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.cmpc_emu_rbd_eval.argtypes = [vp] * 10 + [i32, vp, vp, ctypes.c_double] + [vp] * 7
    lib.cmpc_emu_rbd_eval.restype = ctypes.c_int
    lib.cmpc_emu_rbd_last_error.restype = ctypes.c_char_p
    for f in (lib.cmpc_emu_rbd_log, lib.cmpc_emu_rbd_exp):
        f.argtypes, f.restype = [i32, vp, vp], None
    lib.cmpc_emu_rbd_sincos.argtypes, lib.cmpc_emu_rbd_sincos.restype = [i32, vp, vp, vp], None
    return lib


def emulate_tables(tables, q, v, g=G, outputs=FIELDS):
    """The emulated device source on host tables (the argument order of ``cmpc_rbd_model_create``) -> ``rbd.Evaluation`` of
    numpy arrays (None where not asked for); raises ValueError with the validation's message."""
    q, v = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(v, dtype=np.float64)
    B = q.shape[0]
    out = {k: (np.full((B,) + SHAPES[k], 12345.0) if k in outputs else None) for k in FIELDS}
    rc = emu_lib().cmpc_emu_rbd_eval(*(a.ctypes.data for a in tables), B, q.ctypes.data, v.ctypes.data, g,
                                     *(None if out[k] is None else out[k].ctypes.data for k in FIELDS))
    if rc != 0:
        raise ValueError(emu_lib().cmpc_emu_rbd_last_error().decode())
    return rbd.Evaluation(**out)


def emulate(name, q, v, g=G, outputs=FIELDS):
    return emulate_tables(model(name).tables(), q, v, g, outputs)


@functools.lru_cache(maxsize=None)
def emulated(name, B=8):
    out = emulate(name, *sample(name, B))
    for a in out:
        a.setflags(write=False)
    return out


def worst(got, want):
    """Largest error of every output over the level it is held to (<= 1 passes), by field."""
    return {k: float(np.abs(getattr(got, k) - getattr(want, k)).max() / (LEVEL * max(1.0, np.abs(getattr(want, k)).max())))
            for k in FIELDS}

"""What the tests of the rigid-body model with per-robot inertial parameters share (cmpc_rbd_eval_inertial; CPU and GPU
tiers): the emulated per-instance device source (tests/emu/rbd_inertial_emu.cpp through ctypes), the drawn tables -- eight
robots per model, each with its own link masses, centres of mass and inertias --, the models built from single rows and the
payload cases.  On top of ``rbd_common``; built once and never modified."""
import ctypes
import functools

import numpy as np

import build as _build
import rbd_common as rc
import rbd_reference as ref
from cmpc_amd import rbd

FILL = 12345.0
#: the reference's payload experiment: box.urdf's masses in kg (its commented sweep) on the torso, in front of the chest
PAYLOADS = (0.7, 1.0, 1.5, 2.0, 2.5)
PAYLOAD_AT = (0.15, 0.0, 0.1)


@functools.lru_cache(maxsize=None)
def emu_lib():
    lib = ctypes.CDLL(_build.build_emu_rbd_inertial())
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.cmpc_emu_rbd_eval_inertial.argtypes = [vp] * 10 + [i32, vp, vp, vp, ctypes.c_double] + [vp] * 7
    lib.cmpc_emu_rbd_eval_inertial.restype = ctypes.c_int
    lib.cmpc_emu_rbd_inertial_last_error.restype = ctypes.c_char_p
    lib.cmpc_emu_rbd_inertial_lds_bytes.restype = ctypes.c_int
    return lib


def emulate(name, q, v, inertial, g=rc.G, outputs=rc.FIELDS):
    """The emulated per-instance source on model ``name`` with robot b on row b of ``inertial`` (B,25,10) ->
    ``rbd.Evaluation`` of numpy arrays (None where not asked for)."""
    q, v = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(v, dtype=np.float64)
    tab = np.ascontiguousarray(inertial, dtype=np.float64)
    B = q.shape[0]
    assert tab.shape == (B, 25, 10), tab.shape
    out = {k: (np.full((B,) + rc.SHAPES[k], FILL) if k in outputs else None) for k in rc.FIELDS}
    r = emu_lib().cmpc_emu_rbd_eval_inertial(*(a.ctypes.data for a in rc.model(name).tables()), B, q.ctypes.data, v.ctypes.data,
                                             tab.ctypes.data, g, *(None if out[k] is None else out[k].ctypes.data for k in rc.FIELDS))
    if r != 0:
        raise ValueError(emu_lib().cmpc_emu_rbd_inertial_last_error().decode())
    return rbd.Evaluation(**out)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@functools.lru_cache(maxsize=None)
def rows(name, B=8):
    """(B,25,10), read-only; row b does not depend on B.  Row 0 is the model's own; in the others every body's mass is
    scaled by a factor drawn in [0.7, 1.4], its centre of mass shifted by up to 2 cm per axis and its inertia replaced by a
    drawn symmetric positive definite one."""
    tab = np.tile(rc.model(name).inertial(), (B, 1, 1))
    for b in range(1, B):
        rng = np.random.default_rng([rc.MODELS.index(name), 31, b])
        tab[b, :, 0] *= rng.uniform(0.7, 1.4, size=25)
        tab[b, :, 1:4] += rng.uniform(-0.02, 0.02, size=(25, 3))
        for i in range(25):
            A = rng.normal(size=(3, 3))
            I = 0.01 * (A @ A.T + 0.5 * np.eye(3))
            tab[b, i, 4:] = (I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2])
    tab.setflags(write=False)
    return tab


def model_from_row(name, row):
    """The ``RobotModel`` of ``name`` with the inertial words of ``row`` (25,10): what a robot on that row is."""
    m = rc.model(name)
    new = rbd.RobotModel(m.parent, m.joint_R, m.joint_p, m.axis, row[:, 0], row[:, 1:4], row[:, 4:10], m.frame_body, m.frame_R,
                         m.frame_p, joint_names=m.joint_names)
    new.axis = m.axis                        # (the constructor normalises once more, which may move a last bit: same kinematics)
    return new


@functools.lru_cache(maxsize=None)
def emulated(name, B=8):
    """The per-instance source on ``rc.sample(name)`` with ``rows(name)``; read-only."""
    out = emulate(name, *rc.sample(name, B), rows(name, B))
    for a in out:
        a.setflags(write=False)
    return out


def torso():
    return rc.model("hrp4").body_of("torso")


def payload_rows(masses, at=PAYLOAD_AT):
    """(len(masses),25,10): HRP-4 with one payload per robot on the torso body at ``at``."""
    return rbd.attach_payload(rc.model("hrp4").inertial(), torso(), np.asarray(masses, dtype=np.float64), np.asarray(at, dtype=np.float64))


def tree_with_payload(mass, at):
    """The reference's tree of the nominal HRP-4 model plus ONE extra link, fixed to the torso body at ``at``, that carries
    the payload as a point mass: no parallel-axis rule anywhere."""
    t = ref.tree_from_model(rc.model("hrp4"))
    extra = dict(parent=torso(), R0=np.eye(3), p0=np.asarray(at, dtype=np.float64), axis=None, dof=None, mass=float(mass),
                 c=np.zeros(3), I=np.zeros((3, 3)))
    return ref.Tree(list(t.links) + [extra], t.frames)


def sequential_total(row):
    """A row's masses summed in body order 0 .. 24: the kernel's total, bit for bit."""
    total = 0.0
    for i in range(25):
        total += float(row[i, 0])
    return total

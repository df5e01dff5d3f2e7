"""What the tests of the walking loop share (CPU and GPU tiers): the emulated device source (tests/emu/rbd_walk_emu.cpp through
ctypes), the gait tables of the five walks of tests/scenes_common.py, drawn batches of task-reference inputs on the
evaluations of tests/rbd_common.py, and the scipy restatement of the integrator.  Built once and never modified."""
import copy
import ctypes
import functools

import numpy as np
from scipy.spatial.transform import Rotation

import build as _build
import rbd_common as rc
from cmpc_amd import rbd, workloads as wl
from cmpc_amd.foot_trajectory_generator import FootTrajectoryGenerator
from scenes_common import NAMES, five_scenes, scene_set

REF_FIELDS = rbd.REFERENCE_FIELDS
WIDTH = dict(ff=51, pos_err=51, vel_err=51, feet_des=36)
INPUTS = ("plan_pos", "pose", "vel", "jdqd", "com_des", "q", "v")


@functools.lru_cache(maxsize=None)
def emu_lib():
    lib = ctypes.CDLL(_build.build_emu_rbd_walk())
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    gait = [i32, i32, i32] + [vp] * 8 + [f64, f64]
    lib.cmpc_emu_walk_gait_check.argtypes, lib.cmpc_emu_walk_gait_check.restype = gait, ctypes.c_int
    lib.cmpc_emu_walk_task_refs.argtypes, lib.cmpc_emu_walk_task_refs.restype = gait + [i32] + [vp] * 14, ctypes.c_int
    lib.cmpc_emu_walk_integrate.argtypes, lib.cmpc_emu_walk_integrate.restype = [i32, vp, vp, vp, f64, vp, vp, vp], ctypes.c_int
    lib.cmpc_emu_walk_last_error.restype = ctypes.c_char_p
    return lib


@functools.lru_cache(maxsize=None)
def walks(pick=NAMES):
    """The ``SceneSet`` of the walks named (all five: the set of tests/scenes_common.py)."""
    return scene_set() if pick == NAMES else wl.SceneSet([five_scenes()[NAMES.index(n)] for n in pick])


@functools.lru_cache(maxsize=None)
def tables(pick=NAMES):
    """The gait tables of the walks named, as one set (read-only)."""
    tab = walks(pick).gait_tables()
    for a in tab.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return tab


def editable(tab):
    return {k: (np.array(a) if isinstance(a, np.ndarray) else a) for k, a in tab.items()}


def gait_refusal(tab):
    """None, or the native validation's message."""
    keep = rbd.gait_arguments(tab)
    rc_ = emu_lib().cmpc_emu_walk_gait_check(*(a.ctypes.data if isinstance(a, np.ndarray) else a for a in keep))
    return emu_lib().cmpc_emu_walk_last_error().decode() if rc_ else None


def emulate_refs(tab, case, q_ref=None, outputs=REF_FIELDS):
    """The emulated ``cmpc_walk_task_refs`` on a case (dict of t, scene_id and the INPUTS) -> ``rbd.References`` of numpy."""
    B = case["t"].shape[0]
    keep = rbd.gait_arguments(tab)
    f = lambda k, dt=np.float64: None if case.get(k) is None else np.ascontiguousarray(case[k], dtype=dt)
    arrs = [f("t", np.int32), f("scene_id", np.int32)] + [f(k) for k in INPUTS] + [None if q_ref is None else np.ascontiguousarray(q_ref)]
    out = {k: (np.full((B, WIDTH[k]), 12345.0) if k in outputs else None) for k in REF_FIELDS}
    r = emu_lib().cmpc_emu_walk_task_refs(*(a.ctypes.data if isinstance(a, np.ndarray) else a for a in keep), B,
                                          *(None if a is None else a.ctypes.data for a in arrs),
                                          *(None if out[k] is None else out[k].ctypes.data for k in REF_FIELDS))
    if r != 0:
        raise ValueError(emu_lib().cmpc_emu_walk_last_error().decode())
    return rbd.References(**out)


def emulate_integrate(q, v, qdd, dt, hold=None, in_place=False):
    q, v, qdd = (np.array(a, dtype=np.float64, order="C") for a in (q, v, qdd))
    hold = None if hold is None else np.ascontiguousarray(hold, dtype=np.uint8)
    qo, vo = (q, v) if in_place else (np.full_like(q, 12345.0), np.full_like(v, 12345.0))
    r = emu_lib().cmpc_emu_walk_integrate(q.shape[0], q.ctypes.data, v.ctypes.data, qdd.ctypes.data, dt,
                                          None if hold is None else hold.ctypes.data, qo.ctypes.data, vo.ctypes.data)
    if r != 0:
        raise ValueError(emu_lib().cmpc_emu_walk_last_error().decode())
    return qo, vo


def interesting_ticks(s, pick=NAMES):
    """Ticks of scene s that take every branch of the swing-foot generator: t = 0, one tick inside step 0, and for a
    left-support and a right-support step the first, middle and last tick of the single support, the first and the middle
    tick of the double support; the last tick of the scene."""
    tab = tables(pick)
    ticks = [0, 1]
    for idx in (1, 2, 3, 4):
        st, ss = int(tab["step_start"][s, idx]), int(tab["ss_dur"][s, idx])
        ds = int(tab["step_start"][s, idx + 1]) - st - ss
        ticks += [st, st + ss // 2, st + ss - 1, st + ss, st + ss + ds // 2]
    return ticks + [int(tab["T"][s]) - 1]


def mixed_plan(scene_id, seed, pick=NAMES):
    """(B, n_steps_max, 3): every robot's own plan, x and y of every entry moved by up to 3 cm (the padding stays NaN)."""
    rng = np.random.default_rng(seed)
    plan = walks(pick).plan_pos[scene_id].copy()
    plan[:, :, :2] += rng.uniform(-0.03, 0.03, size=plan[:, :, :2].shape)
    return plan


def generator_feet(s, t, plan_pos, pick=NAMES):
    """feet_des (36,) from the package's own FootTrajectoryGenerator on a copy of scene s's planner with the robot's plan."""
    sc = five_scenes()[NAMES.index(pick[s])]
    pl = copy.deepcopy(sc.planner)
    for i, step in enumerate(pl.plan):
        step['pos'] = np.array(plan_pos[i])
    now = FootTrajectoryGenerator(sc.initial, pl, sc.params).generate_feet_trajectories_at_time(int(t))
    return np.hstack([np.hstack([now[f][k] for k in ('pos', 'vel', 'acc')]) for f in ('lfoot', 'rfoot')])


@functools.lru_cache(maxsize=None)
def refs_case(name, B, pick=NAMES):
    """A batch of task-reference inputs on the evaluations of ``rc.sample(name, B)``: scenes and ticks mixed over the batch
    (robots 1 and 2, the bases at angle 0 and 1e-10, on the straight `shipped` walk at a tick of step 0, where the desired
    base rotation is the identity to 1e-16), every robot its own plan and CoM reference.  The rotation of a task frame is
    the evaluation's, except where it is more than 2 rad from the desired one: there it is moved onto 1.8 rad from it
    along the same axis (Log is held to the level only away from pi).  Read-only."""
    ev = rc.emulated(name, B)
    q, v = rc.sample(name, B)
    rng = np.random.default_rng([rc.MODELS.index(name), 31, B])
    sid = (np.arange(B) % len(pick)).astype(np.int32)
    t = np.array([interesting_ticks(s, pick)[(3 * b) % 23] for b, s in enumerate(sid)], dtype=np.int32)   # (23 ticks each)
    if "shipped" in pick:
        sid[1:3], t[1:3] = pick.index("shipped"), (0, 1)
    case = dict(t=t, scene_id=sid, plan_pos=mixed_plan(sid, [5, B], pick), pose=ev.pose.copy(), vel=ev.vel.copy(), jdqd=ev.jdqd.copy(),
                com_des=rng.normal(size=(B, 9)), q=q.copy(), v=v.copy())
    for b in range(B):
        feet = generator_feet(sid[b], t[b], case["plan_pos"][b], pick)
        want = (feet[0:3], feet[18:21], (feet[0:3] + feet[18:21]) / 2., (feet[0:3] + feet[18:21]) / 2.)
        for r0, wd in zip((0, 6, 15, 18), want):
            Rd = Rotation.from_rotvec(wd)
            rel = (Rd * Rotation.from_rotvec(case["pose"][b, r0:r0 + 3]).inv()).as_rotvec()
            if np.linalg.norm(rel) > 2.0:
                rel *= 1.8 / np.linalg.norm(rel)
                case["pose"][b, r0:r0 + 3] = (Rotation.from_rotvec(rel).inv() * Rd).as_rotvec()
    for a in case.values():
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def q_ref():
    a = np.array(rc.standing())
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def emulated_refs(name, B, pick=NAMES):
    out = emulate_refs(tables(pick), refs_case(name, B, pick), q_ref())
    for a in out:
        a.setflags(write=False)
    return out


def mirror_refs(case, q_ref, pick=NAMES):
    """``rbd.References`` by numpy and scipy: the generator's feet, the mean of their first three entries for torso and
    base, Log(R_des R_cur') by ``Rotation``."""
    B = case["t"].shape[0]
    ff, pe, ve, fd = np.zeros((B, 51)), np.zeros((B, 51)), np.zeros((B, 51)), np.zeros((B, 36))
    for b in range(B):
        feet = generator_feet(case["scene_id"][b], case["t"][b], case["plan_pos"][b], pick)
        fd[b] = feet
        l, r = feet[:18].reshape(3, 6), feet[18:].reshape(3, 6)          # rows pos, vel, acc
        mean = (l[:, :3] + r[:, :3]) / 2.
        des = np.zeros((3, 21))
        des[:, 0:6], des[:, 6:12], des[:, 12:15] = l, r, case["com_des"][b].reshape(3, 3)
        des[:, 15:18], des[:, 18:21] = mean, mean
        ff[b, :21] = des[2] - case["jdqd"][b]
        pe[b, :21] = des[0] - case["pose"][b]
        ve[b, :21] = des[1] - case["vel"][b]
        for r0 in (0, 6, 15, 18):
            Rd, Rc = Rotation.from_rotvec(des[0, r0:r0 + 3]), Rotation.from_rotvec(np.array(case["pose"][b, r0:r0 + 3]))
            pe[b, r0:r0 + 3] = (Rd * Rc.inv()).as_rotvec()
        pe[b, 27:] = q_ref[6:] - case["q"][b, 6:]
        ve[b, 27:] = -case["v"][b, 6:]
    return rbd.References(ff, pe, ve, fd)


def mirror_integrate(q, v, qdd, dt):
    """(v+, p+, joints+, R+ (B,3,3)) of the explicit body-twist step, by scipy."""
    R = Rotation.from_rotvec(q[:, 0:3])
    vn = v + dt * qdd
    Rn = R * Rotation.from_rotvec(dt * vn[:, 0:3])
    return vn, q[:, 3:6] + dt * R.apply(vn[:, 3:6]), q[:, 6:] + dt * vn[:, 6:], Rn.as_matrix()


def same_bits(got, want, rows=slice(None), fields=REF_FIELDS):
    for k in fields:
        g, w = np.ascontiguousarray(getattr(got, k)), np.ascontiguousarray(getattr(want, k)[rows])
        assert g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)), k

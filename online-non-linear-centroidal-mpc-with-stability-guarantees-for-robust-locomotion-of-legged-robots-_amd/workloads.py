"""Synthetic workloads of BASELINE.json and the vectorised parameter builder.

``Scene`` holds the flat-ground walk of the reference driver (code/simulation.py:24-39,
:97-130): the shipped velocity commands, planner, swing generator and CoM reference, plus
per-tick tables that make the front half of ``centroidal_mpc.solve``
(code/centroidal_mpc_vertices.py:482-600) a pure gather, so a whole batch of parameter
records is built with numpy fancy indexing instead of the reference's Python loops.
"""
import numpy as np

from .footstep_planner_vertices import FootstepPlanner
from .foot_trajectory_generator import FootTrajectoryGenerator
from .functions import references
from .problem import ProblemSpec, current_contacts, contact_flags

HRP4_MASS = 40.05487735          # sum of link masses of code/urdf/hrp4.urdf

# initial sole poses of the DART model, code/Debug/contact_trj_from_centroidal_MPC line 1
LFOOT0 = np.array([0.0, -1.3870180197464853e-16, -4.639952657811354e-18,
                   1.0310923973763693e-17, 0.10163857612916291, -1.3877787807814457e-17])
RFOOT0 = np.array([0.0, -1.3870180197464853e-16, 4.639952657811354e-18,
                   1.0310923973763693e-17, -0.10163857612916291, -1.3877787807814457e-17])

# code/simulation.py:97
VREF = ([(0.15, 0., 0)] * 5 + [(0.15, 0.0, 0)] * 3 + [(0.15, 0.0, 0)] * 3 +
        [(0.13, 0, 0)] * 4 + [(0.1, 0., 0)] * 2 + [(0., 0, 0)] * 3)


def default_params(N=10, mpc_rate=1):
    """The params dict of code/simulation.py:24-44 (mass from the URDF)."""
    p = {'g': 9.81, 'h': 0.72, 'foot_size': 0.1, 'step_height': 0.02, 'world_time_step': 0.01,
         'ss_duration': 70, 'ds_duration': 30, 'first_swing': 'rfoot', 'µ': 0.5, 'N': N, 'dof': 30,
         'mass': HRP4_MASS, 'update_contact': 'YES', 'mpc_rate': mpc_rate}
    p['eta'] = np.sqrt(p['g'] / p['h'])
    return p


class Scene:
    """Planner + references of one walk and per-tick gather tables.  vref: the velocity commands handed to
    ``FootstepPlanner`` (None = the shipped walk ``VREF``); ``params['first_swing']`` names the foot that swings first."""

    def __init__(self, params=None, vref=None):
        self.params = default_params() if params is None else params
        self.vref = VREF if vref is None else list(vref)
        self.initial = {'lfoot': {'pos': LFOOT0.copy()}, 'rfoot': {'pos': RFOOT0.copy()},
                        'com': {'pos': np.array([0., 0., 0.72]), 'vel': np.zeros(3)},
                        'hw': {'val': np.zeros(3)}}
        self.planner = FootstepPlanner(self.vref, LFOOT0, RFOOT0, self.params)
        self.ftg = FootTrajectoryGenerator(self.initial, self.planner, self.params)
        self.com_ref = references(self.ftg, self.planner)
        self.refresh_tables()

    def refresh_tables(self):
        """(Re)build per-tick tables from the planner (call again after a plan write-back)."""
        pl, first = self.planner, self.params['first_swing']
        keys = ('pos_x', 'pos_y', 'pos_z', 'vel_x', 'vel_y', 'vel_z', 'acc_x', 'acc_y', 'acc_z')
        T = min(len(self.com_ref[k]) for k in keys)
        self.T = T
        self.com_tab = np.stack([np.asarray(self.com_ref[k], dtype=np.float64)[:T] for k in keys], axis=1)
        pose_l = pl.position_contacts_ref['contact_left']
        pose_r = pl.position_contacts_ref['contact_right']
        self.pose_l, self.pose_r = pose_l, pose_r
        gl, gr = np.ones(T), np.ones(T)
        cur_l, cur_r = np.zeros((T, 3)), np.zeros((T, 3))
        # schedule tables for per-instance plans (rollout.BatchedRollout): plan entries behind the x0 foot
        # positions (:493-509), phase and step index of every tick, support foot of the step
        self.slot_l, self.slot_r = np.full(T, -1, np.int32), np.full(T, -1, np.int32)
        self.is_ss, self.step_idx = np.zeros(T, bool), np.zeros(T, np.int32)
        self.support_is_l = np.zeros(T, bool)
        for t in range(T):
            idx = pl.get_step_index_at_time(t)
            self.step_idx[t] = idx
            self.support_is_l[t] = pl.plan[idx]['foot_id'] == 'lfoot'
            if pl.get_phase_at_time(t) != 'ds':
                self.is_ss[t] = True
                if pl.plan[idx]['foot_id'] == 'lfoot':
                    gr[t] = 0.
                else:
                    gl[t] = 0.
            cur_l[t], cur_r[t] = current_contacts(pl, pose_l[:, 3:6], pose_r[:, 3:6], t, first)
            if t >= 200:
                index = pl.get_step_index_at_time(t - 70)
                a, b = index + (index % 2), index + (index - 1) % 2
                self.slot_l[t], self.slot_r[t] = (a, b) if first == 'lfoot' else (b, a)
        self.plan_pos = np.stack([np.asarray(p['pos'], dtype=np.float64) for p in pl.plan])
        self.gl_tab, self.gr_tab, self.cur_l, self.cur_r = gl, gr, cur_l, cur_r

    def t_max(self, N, rate=1):
        return self.T - 1 - (N + 1) * rate

    def gait_tables(self):
        """The host tables of ``cmpc_walk_gait_create`` (include/cmpc_walk.h) for this walk, S = 1: what the swing-foot
        generator reads from the planner at a tick, except the plan positions, which every robot of a rollout owns."""
        return _gait_tables([self])

    def build_records(self, spec, t, com, dcom, hw, theta_hat, yaw_l, yaw_r, mass, mu, rate=1):
        """Vectorised front half of ``solve`` for B instances.  All inputs have leading dim B."""
        t = np.asarray(t, dtype=np.int64)
        B, N = t.shape[0], spec.N
        rec = np.zeros((B, spec.nrec))
        rec[:, 0:3], rec[:, 3:6], rec[:, 6:9], rec[:, 9:12] = com, dcom, hw, theta_hat
        rec[:, 12], rec[:, 13:16] = yaw_l, self.cur_l[t]
        rec[:, 16], rec[:, 17:20] = yaw_r, self.cur_r[t]
        rec[:, 20], rec[:, 21] = mass, mu
        rec[:, 22], rec[:, 23] = self.gl_tab[t + N * rate], self.gr_tab[t + N * rate]
        st = rec[:, 24:].reshape(B, N, 19)
        tt = t[:, None] + (1 + np.arange(N))[None, :] * rate          # (B, N): ticks t+(1+i)*rate
        tn = t[:, None] + np.arange(N)[None, :] * rate                # contact flags at t+i*rate
        st[:, :, 0:9] = self.com_tab[tt]
        st[:, :, 9:12] = self.pose_l[tt, 3:6]
        st[:, :, 12:15] = self.pose_r[tt, 3:6]
        st[:, :, 15] = self.pose_l[tt, 2]
        st[:, :, 16] = self.pose_r[tt, 2]
        st[:, :, 17] = self.gl_tab[tn]
        st[:, :, 18] = self.gr_tab[tn]
        return rec

    def nominal_state(self, t):
        t = np.asarray(t, dtype=np.int64)
        com = np.stack([self.com_tab[t, 0], self.com_tab[t, 1], np.full(t.shape, 0.72)], axis=1)
        dcom = np.stack([self.com_tab[t, 3], self.com_tab[t, 4], np.zeros(t.shape)], axis=1)
        return com, dcom


def _gait_tables(scenes):
    """dict of the gait tables of S scenes, padded per scene (-1 for the integers, 0 for support_l, NaN for ang): T (S,),
    step_idx (S, T_max) int32, n_steps (S,), step_start / ss_dur (S, n_steps_max) int32 ticks, support_l (S, n_steps_max)
    uint8, ang (S, n_steps_max, 3), init_feet (S, 12) = [lfoot ang, pos, rfoot ang, pos], step_height, delta."""
    S = len(scenes)
    for k in ('step_height', 'world_time_step'):
        if any(sc.params[k] != scenes[0].params[k] for sc in scenes):
            raise ValueError(f"all scenes of a gait must share params[{k!r}]")
    T = np.array([sc.T for sc in scenes], dtype=np.int32)
    n = np.array([len(sc.planner.plan) for sc in scenes], dtype=np.int32)
    Tm, nm = int(T.max()), int(n.max())
    tab = dict(T=T, n_steps=n, step_idx=np.full((S, Tm), -1, np.int32), step_start=np.full((S, nm), -1, np.int32),
               ss_dur=np.full((S, nm), -1, np.int32), support_l=np.zeros((S, nm), np.uint8), ang=np.full((S, nm, 3), np.nan),
               init_feet=np.zeros((S, 12)), step_height=float(scenes[0].params['step_height']),
               delta=float(scenes[0].params['world_time_step']))
    for s, sc in enumerate(scenes):
        pl = sc.planner
        tab['step_idx'][s, :T[s]] = sc.step_idx[:T[s]]
        tab['step_start'][s, :n[s]] = pl.step_end_times() - np.array([p['ss_duration'] + p['ds_duration'] for p in pl.plan])
        tab['ss_dur'][s, :n[s]] = pl.ss_durations()
        tab['support_l'][s, :n[s]] = pl.support_is_left()
        tab['ang'][s, :n[s]] = np.array([p['ang'] for p in pl.plan], dtype=np.float64)
        tab['init_feet'][s] = np.hstack((sc.initial['lfoot']['pos'], sc.initial['rfoot']['pos']))
    return tab


def rollout_schedule(sc, N, rate=1):
    """Per-tick tables of the contact-plan write-back (code/centroidal_mpc_vertices.py:656-675) for one ``Scene`` and a
    horizon of N stages `rate` ticks apart, T entries each:
      cond     now single support, horizon end double support: the write-back may fire
      is_ds    double support: the update flag is cleared
      wb_slot  plan entry the landing point goes to (the step after the current one)
      wb_row   rows of x_N holding it: support = lfoot -> the swing foot is the right one -> 17:20, else 13:16"""
    T = sc.T
    end = np.minimum(np.arange(T) + N * rate - 1, T - 1)
    cond = sc.is_ss & ~sc.is_ss[end]
    wb_slot = np.minimum(sc.step_idx + 1, sc.plan_pos.shape[0] - 1).astype(np.int64)
    wb_row = np.where(sc.support_is_l, 17, 13).astype(np.int64)
    return cond, ~sc.is_ss, wb_slot, wb_row


class SceneSet:
    """S walks with their per-tick tables stacked: ``com_tab`` (S, T_max, 9), ``pose_l`` / ``pose_r`` (S, T_max, 6),
    ``gl_tab`` / ``gr_tab`` (S, T_max), ``cur_l`` / ``cur_r`` (S, T_max, 3), ``slot_l`` / ``slot_r`` (S, T_max),
    ``plan_pos`` (S, n_steps_max, 3), ``is_ss`` / ``step_idx`` / ``support_is_l`` (S, T_max).  Every instance of a batch
    names its walk by a scene index.  Rows beyond a scene's own ``T[s]`` / ``n_steps[s]`` are padding: NaN for doubles,
    -1 for slots and step indices, False for flags -- a read of padding shows.  The scenes may differ in the velocity
    commands, ``first_swing`` and the phase durations; the tick length, the default mass and ``mpc_rate`` are shared
    (one batch advances by one ``rate``)."""

    SHARED = ('world_time_step', 'mass', 'mpc_rate')

    def __init__(self, scenes):
        scenes = list(scenes)
        if not scenes:
            raise ValueError("a SceneSet needs at least one Scene")
        for k in self.SHARED:
            if any(sc.params[k] != scenes[0].params[k] for sc in scenes):
                raise ValueError(f"all scenes of a set must share params[{k!r}]")
        self.scenes, self.params = scenes, scenes[0].params
        self.S = S = len(scenes)
        self.T = np.array([sc.T for sc in scenes], dtype=np.int32)
        self.n_steps = np.array([sc.plan_pos.shape[0] for sc in scenes], dtype=np.int32)
        self.T_max, self.n_steps_max = int(self.T.max()), int(self.n_steps.max())

        def stack(name, fill, dtype, rows=self.T_max, lens=self.T):
            first = np.asarray(getattr(scenes[0], name))
            out = np.full((S, rows) + first.shape[1:], fill, dtype=dtype)
            for s, sc in enumerate(scenes):
                out[s, :lens[s]] = np.asarray(getattr(sc, name))[:lens[s]]
            return out
        for name in ('com_tab', 'pose_l', 'pose_r', 'gl_tab', 'gr_tab', 'cur_l', 'cur_r'):
            setattr(self, name, stack(name, np.nan, np.float64))
        for name in ('slot_l', 'slot_r', 'step_idx'):
            setattr(self, name, stack(name, -1, np.int32))
        for name in ('is_ss', 'support_is_l'):
            setattr(self, name, stack(name, False, bool))
        self.plan_pos = stack('plan_pos', np.nan, np.float64, rows=self.n_steps_max, lens=self.n_steps)

    def t_max(self, N, rate=1):
        """Last valid tick of every scene, (S,)."""
        return self.T - 1 - (N + 1) * rate

    def gait_tables(self):
        """The host tables of ``cmpc_walk_gait_create`` for the S walks, padded per scene (``Scene.gait_tables``)."""
        return _gait_tables(self.scenes)

    def build_records(self, spec, t, scene_id, com, dcom, hw, theta_hat, yaw_l, yaw_r, mass, mu, rate=1):
        """``Scene.build_records`` for a mixed batch: instance b is tick t[b] of scene scene_id[b]."""
        t, s = np.asarray(t, dtype=np.int64), np.asarray(scene_id, dtype=np.int64)
        B, N = t.shape[0], spec.N
        if s.shape != (B,) or (s < 0).any() or (s >= self.S).any():
            raise ValueError(f"scene_id must hold B indices in [0, {self.S})")
        if (t < 0).any() or (t + (N + 1) * rate >= self.T[s]).any():
            raise ValueError("tick outside its scene: need 0 <= t and t + (N+1)*rate < T[scene_id]")
        rec = np.zeros((B, spec.nrec))
        rec[:, 0:3], rec[:, 3:6], rec[:, 6:9], rec[:, 9:12] = com, dcom, hw, theta_hat
        rec[:, 12], rec[:, 13:16] = yaw_l, self.cur_l[s, t]
        rec[:, 16], rec[:, 17:20] = yaw_r, self.cur_r[s, t]
        rec[:, 20], rec[:, 21] = mass, mu
        rec[:, 22], rec[:, 23] = self.gl_tab[s, t + N * rate], self.gr_tab[s, t + N * rate]
        st = rec[:, 24:].reshape(B, N, 19)
        tt = t[:, None] + (1 + np.arange(N))[None, :] * rate
        tn = t[:, None] + np.arange(N)[None, :] * rate
        ss = s[:, None]
        st[:, :, 0:9] = self.com_tab[ss, tt]
        st[:, :, 9:12] = self.pose_l[ss, tt, 3:6]
        st[:, :, 12:15] = self.pose_r[ss, tt, 3:6]
        st[:, :, 15] = self.pose_l[ss, tt, 2]
        st[:, :, 16] = self.pose_r[ss, tt, 2]
        st[:, :, 17] = self.gl_tab[ss, tn]
        st[:, :, 18] = self.gr_tab[ss, tn]
        return rec

    def schedule(self, N, rate=1):
        """``rollout_schedule`` of every scene, stacked: (cond, is_ds, wb_slot, wb_row), each (S, T_max); padding is
        False / False / -1 / -1."""
        S, Tm = self.S, self.T_max
        cond, is_ds = np.zeros((S, Tm), bool), np.zeros((S, Tm), bool)
        wb_slot, wb_row = np.full((S, Tm), -1, np.int64), np.full((S, Tm), -1, np.int64)
        for s, sc in enumerate(self.scenes):
            c, d, sl, ro = rollout_schedule(sc, N, rate)
            cond[s, :sc.T], is_ds[s, :sc.T], wb_slot[s, :sc.T], wb_row[s, :sc.T] = c, d, sl, ro
        return cond, is_ds, wb_slot, wb_row

    def nominal_state(self, t, scene_id):
        t, s = np.asarray(t, dtype=np.int64), np.asarray(scene_id, dtype=np.int64)
        com = np.stack([self.com_tab[s, t, 0], self.com_tab[s, t, 1], np.full(t.shape, 0.72)], axis=1)
        dcom = np.stack([self.com_tab[s, t, 3], self.com_tab[s, t, 4], np.zeros(t.shape)], axis=1)
        return com, dcom


_SCENE = None


def scene():
    global _SCENE
    if _SCENE is None:
        _SCENE = Scene()
    return _SCENE


CONFIGS = {
    # name: (seed, N, nv, payload gains, default batch)
    "perturbed": (20250711, 20, 4, False, 256),          # BASELINE config 2
    "payload": (20250712, 20, 4, True, 4096),            # config 3
    "randomized": (20250713, 20, 4, False, 65536),       # config 4
    "long_horizon": (20250714, 40, 8, False, 16384),     # config 5
}


def make_workload(name, B=None, N=None, scale=1.0, rate=1, seed=None):
    """(spec, records (B, nrec) numpy) for one of the BASELINE synthetic configs.
    seed = None: the configuration's own seed; another value draws a fresh batch of the same distribution.
    rate = 10 is the reference's ``mpc_rate == 10`` variant: delta = 0.1 s, k1, k2 = 5, 0.2, no force-rate
    cost (:11, :27-31, :339-341), references sampled every tenth tick (:548-600)."""
    seed0, N0, nv, payload, B0 = CONFIGS[name]
    seed = seed0 if seed is None else seed
    B = B0 if B is None else B
    N = N0 if N is None else N
    sc = scene()
    spec = ProblemSpec.from_params(default_params(N=N, mpc_rate=rate), payload=payload, nv=nv)
    rng = np.random.default_rng(seed)
    t = rng.integers(200, min(1700, sc.t_max(N, rate)) + 1, size=B)
    com, dcom = sc.nominal_state(t)
    com = com + scale * rng.uniform(-0.02, 0.02, size=(B, 3))
    com[:, 2] = np.minimum(com[:, 2], 0.755)
    dcom = dcom + scale * rng.normal(0, 0.05, size=(B, 3))
    hw = scale * rng.normal(0, 0.3, size=(B, 3))
    theta = np.zeros((B, 3))
    mass = np.full(B, HRP4_MASS)
    mu = np.full(B, 0.5)
    if name == "payload":
        theta = rng.uniform(-25, 25, size=(B, 3))
        com[:, 2] -= rng.uniform(0, 0.02, size=B)
    if name == "randomized":
        mass = HRP4_MASS * rng.uniform(0.8, 1.2, size=B)
        mu = rng.uniform(0.3, 0.9, size=B)
        F = rng.uniform(0, 100, size=B)
        ang = rng.uniform(0, 2 * np.pi, size=B)
        arm = rng.uniform(0, 0.4, size=B)
        Fv = np.stack([F * np.cos(ang), F * np.sin(ang), np.zeros(B)], axis=1)
        dcom = dcom + Fv * 0.1 / mass[:, None]
        r = np.stack([np.zeros(B), np.zeros(B), arm], axis=1)
        hw = hw + np.cross(r, Fv) * 0.1
    rec = sc.build_records(spec, t, com, dcom, hw, theta, np.zeros(B), np.zeros(B), mass, mu, rate=rate)
    return spec, rec


def walk_records(spec, ticks, hw=None, theta_hat=None):
    """Config 1 sampled open loop: records of the nominal flat-ground walk at `ticks` (x0 on the CoM
    reference, measured angular momentum `hw` (len(ticks), 3) -- zero if None, which puts late single support
    at the edge of feasibility)."""
    sc = scene()
    t = np.asarray(ticks, dtype=np.int64)
    com, dcom = sc.nominal_state(t)
    B = t.shape[0]
    hw = np.zeros((B, 3)) if hw is None else np.asarray(hw, dtype=np.float64)
    th = np.zeros((B, 3)) if theta_hat is None else np.asarray(theta_hat, dtype=np.float64)
    return sc.build_records(spec, t, com, dcom, hw, th, np.zeros(B), np.zeros(B),
                            np.full(B, HRP4_MASS), np.full(B, 0.5))


WBC_ND, WBC_NC = 30, 12           # dofs and contact-wrench dimensions of the whole-body QP (code/inverse_dynamics.py:30-66)


WBC_TASK_ROWS = {'lfoot': 6, 'rfoot': 6, 'com': 3, 'torso': 3, 'base': 3}     # the task Jacobians of :46-51
# position and velocity gains of code/inverse_dynamics.py:43-44 by task (wbc.POS_GAINS / VEL_GAINS: kept here as well, this
# module is numpy only)
WBC_POS_GAINS = {'lfoot': 10., 'rfoot': 10., 'com': 5., 'torso': 10., 'base': 10., 'joints': 10.}
WBC_VEL_GAINS = {'lfoot': 5., 'rfoot': 5., 'com': 10., 'torso': 5., 'base': 3., 'joints': 5.}


def _wbc_joint_selection():
    sel = np.zeros(WBC_ND); sel[18:30] = 1.0                         # "redundant dofs" of the joint task
    return sel


def _wbc_draw(rng, mass, g):
    """One synthetic robot from `rng`: task Jacobians, target accelerations of the tasks and of the joints, M, h."""
    Jt = {k: rng.normal(0, 0.4, size=(r, WBC_ND)) for k, r in WBC_TASK_ROWS.items()}
    for k in ('lfoot', 'rfoot'):
        Jt[k][:, :6] += np.eye(6)                             # feet move with the floating base
    Jt['com'][:, 3:6] += np.eye(3)
    acc = {k: rng.normal(0, 1.0, size=r) for k, r in WBC_TASK_ROWS.items()}
    acc_joints = rng.normal(0, 1.0, size=WBC_ND)
    L = rng.normal(0, 0.15, size=(WBC_ND, WBC_ND))
    Mb = L @ L.T + np.diag(np.concatenate([np.full(3, 2.0), np.full(3, mass), rng.uniform(0.05, 1.0, WBC_ND - 6)]))
    hb = rng.normal(0, 2.0, size=WBC_ND); hb[5] += mass * g      # gravity on the base translation (z)
    return Jt, acc, acc_joints, Mb, hb


def wbc_synthetic(B, seed=0, contact="ds", mass=HRP4_MASS, g=9.81):
    """Synthetic instances of the size and structure of the reference's QP for HRP-4 (30 dofs): task Jacobians of the
    shapes of :46-51 with random entries, a positive definite mass matrix with the robot's total mass on the base
    translation, gravity on the base, contact Jacobians [.. foot wrench ..] scaled by the contact flags (:109)."""
    rng = np.random.default_rng(seed)
    Hq = np.zeros((B, WBC_ND, WBC_ND)); Fq = np.zeros((B, WBC_ND)); M = np.zeros((B, WBC_ND, WBC_ND)); h = np.zeros((B, WBC_ND)); Jc = np.zeros((B, WBC_NC, WBC_ND))
    sel = _wbc_joint_selection()
    weights = {'lfoot': 1.0, 'rfoot': 1.0, 'com': 1.0, 'torso': 1.0, 'base': 1.0}
    rows = WBC_TASK_ROWS
    for b in range(B):
        Jt, acc, acc_joints, Mb, hb = _wbc_draw(rng, mass, g)
        Hb = sum(weights[k] * Jt[k].T @ Jt[k] for k in rows) + 0.1 * np.diag(sel)
        Fb = -sum(weights[k] * Jt[k].T @ acc[k] for k in rows) - 0.1 * sel * acc_joints
        cl, cr = contact in ("ds", "lfoot"), contact in ("ds", "rfoot")
        Jcb = np.vstack([cl * Jt['lfoot'], cr * Jt['rfoot']])
        Hq[b], Fq[b], M[b], h[b], Jc[b] = Hb, Fb, Mb, hb, Jcb
    return Hq, Fq, M, h, Jc


def wbc_synthetic_tasks(B, seed=0, mass=HRP4_MASS, g=9.81):
    """The instances of ``wbc_synthetic(B, seed)`` in the task form of code/inverse_dynamics.py:46-103: J, Jdot (B,21,30),
    ff, pos_err, vel_err (B,51), qd (B,30), joint_sel (30,), M, h.  The Jacobians, the target accelerations, M and h are
    wbc_synthetic's own draws (same stream: J[:, :12] is its double-support Jc, bit for bit); Jdot, qd and the errors
    come from a second generator, and ff = target - k_v e_v - k_p e_p + Jdot qd, so that the commanded accelerations --
    and with them Hq, Fq -- are wbc_synthetic's up to rounding.  Instance b does not depend on B."""
    rng, rng2 = np.random.default_rng(seed), np.random.default_rng([seed, 1])
    NR = sum(WBC_TASK_ROWS.values())
    J = np.zeros((B, NR, WBC_ND)); Jdot = np.zeros((B, NR, WBC_ND)); qd = np.zeros((B, WBC_ND))
    ff, pe, ve = (np.zeros((B, NR + WBC_ND)) for _ in range(3))
    M = np.zeros((B, WBC_ND, WBC_ND)); h = np.zeros((B, WBC_ND))
    kp = np.concatenate([np.full(r, WBC_POS_GAINS[k]) for k, r in WBC_TASK_ROWS.items()] + [np.full(WBC_ND, WBC_POS_GAINS['joints'])])
    kv = np.concatenate([np.full(r, WBC_VEL_GAINS[k]) for k, r in WBC_TASK_ROWS.items()] + [np.full(WBC_ND, WBC_VEL_GAINS['joints'])])
    for b in range(B):
        Jt, acc, acc_joints, M[b], h[b] = _wbc_draw(rng, mass, g)
        J[b] = np.vstack([Jt[k] for k in WBC_TASK_ROWS])
        target = np.concatenate([acc[k] for k in WBC_TASK_ROWS] + [acc_joints])
        Jdot[b] = rng2.normal(0, 0.4, size=(NR, WBC_ND))
        qd[b] = rng2.normal(0, 0.5, size=WBC_ND)
        pe[b] = rng2.normal(0, 0.02, size=NR + WBC_ND)
        ve[b] = rng2.normal(0, 0.1, size=NR + WBC_ND)
        ff[b] = target - kv * ve[b] - kp * pe[b] + np.concatenate([Jdot[b] @ qd[b], np.zeros(WBC_ND)])
    return J, Jdot, ff, pe, ve, qd, _wbc_joint_selection(), M, h

"""Closed-loop batched rollout: B independent copies of the controller loop, entirely on the GPU.

Per tick (the reference's ``customPreStep``, code/simulation.py:193-212, without DART; the single-instance
twin of this loop is ``walk.WalkHarness`` around the drop-in class):
  1. parameter records from the per-tick tables, the current centroidal state and the instance's OWN contact
     plan (``DeviceRecordBuilder`` = front half of ``centroidal_mpc.solve``, :482-600);
  2. batched solve, warm-started from the previous tick's solution, unshifted (:630-631);
  3. back half of ``solve`` (:614-683): theta_hat is carried from x_1 (:485, :644); the contact-plan
     write-back (:656-675) scatters the predicted landing point x_N of the swing foot into the instance's plan
     (``update_contact = 'YES'``), guarded by the per-instance ``update_contact_flag``; the state is advanced
     to the MPC's own prediction x_1 (perfect-tracking centroidal model standing in for simulator +
     whole-body controller), optionally disturbed by a velocity push.  The angular momentum is either the MPC's
     prediction or an exogenous measured signal ``hw_measured[t] (+ per-instance offset)`` (see walk.py).
  4. optionally the consumer of the tick, the whole-body inverse-dynamics QP (code/inverse_dynamics.py:30-134, called
     from code/simulation.py:214-232 with ``desired['com']`` = the MPC's CoM position / velocity / acceleration): a
     batched ``wbc.BatchedInverseDynamicsQP`` fed by the caller's rigid-body model (``attach_whole_body``, or from the task
     Jacobians with every instance's own contact flags and friction: ``attach_whole_body_tasks``), so that the
     whole tick -- records, MPC solve, write-back, QP -- stays on the device.
Everything after the solve is index arithmetic and copies in torch (device memory plumbing); the schedule
(phases, step indices) is shared by the batch, the plan positions are per instance.

A fleet: with a ``workloads.SceneSet`` every instance walks the command of its own scene (``scene_id``): the records come
from ``cmpc_build_records_scenes`` and step 3 is one launch, ``cmpc_rollout_advance``, indexed by (scene, tick); only the
momentum lookup stays a torch gather.  With ``consts`` every instance is solved with its own 18 problem constants
(``solve_with_consts``), with one scene or with a set.  With ``gains=True`` every tick also returns the first-stage gains
(``solve_with_gain``, with the instances' own constants when there are any; the trajectory is the same bit for bit) and
``track`` applies them to a measured state between two solves.

With ``feedback=True`` the loop is closed around the robot of the attached ``BatchedRobot.walking_model``: every tick begins
with ``model.measure(self)`` (``cmpc_walk_measure``), which puts the robot's own centroid -- CoM, its velocity, the angular
momentum about it -- and foot angles into the state the records are built from, as the reference's ``retrieve_state`` does
first in ``customPreStep`` (code/simulation.py:201-204).  The order of the tick is then: measure, records from the measured
state, MPC solve, task references and QP on the same evaluation, integrate.  Step 3 is unchanged: words 0..11 of the state
are the MPC's prediction x_1 until the next measurement replaces words 0..8 (``last_measurement.innovation`` is their
difference); theta_hat carries over from x_1.  A robot whose evaluation is not finite or that has fallen stops exactly as
one whose solve failed.
"""
import numpy as np
import torch

from .problem import CONST_FIELDS, NCONST
from .solver import BatchedCentroidalMPC, DeviceRecordBuilder, usable
from .workloads import SceneSet, rollout_schedule


def _checked_consts(consts, spec, B):
    """(B, 18) host copy of the per-instance constants, refused unless every row steps by the spec's delta: the schedule
    advances by `rate` ticks for the whole batch."""
    c = consts.detach().cpu().numpy() if isinstance(consts, torch.Tensor) else np.asarray(consts)
    c = np.ascontiguousarray(c, dtype=np.float64)
    if c.shape != (B, NCONST):
        raise ValueError(f"consts must have shape (B, {NCONST}) = ({B}, {NCONST})")
    bad = np.nonzero(c[:, CONST_FIELDS.index("delta")] != spec.delta)[0]
    if bad.size:
        raise ValueError(f"consts rows {bad[:8].tolist()} have a delta other than the spec's {spec.delta}: one batch "
                         f"advances by one tick length")
    return c


class BatchedRollout:
    def __init__(self, scene, spec, B, device="cuda:0", mass=None, mu=0.5, update_contact=True,
                 hw_measured=None, hw_offset=None, rate=1, scene_id=None, consts=None, gains=False, feedback=False):
        """scene: a ``workloads.Scene`` (one walk for the batch) or a ``workloads.SceneSet`` with ``scene_id`` (B,) naming
        every instance's walk (optional for a set of one).  hw_measured: one recording (ticks, 3), or with a set one per
        scene.  consts (B, 18): per-instance problem constants, every row with the spec's delta.
        gains: every tick solves through ``solve_with_gain`` and keeps ``last_gain`` (B, 20 + nu, 20) next to
        ``last_records`` and ``last_XU`` (``track``); it is one buffer, overwritten by the next tick.
        feedback: every tick begins with the attached model's ``measure`` (the module's docstring) and keeps
        ``last_measurement`` next to ``last_records``; the robot's own momentum is the signal, so ``hw_measured`` and
        ``hw_offset`` are refused with it, and so is a ``push_dv``."""
        if feedback and (hw_measured is not None or hw_offset is not None):
            raise ValueError("feedback=True takes the angular momentum from the robot itself: hw_measured and hw_offset do not go with it")
        self.feedback, self.last_measurement = bool(feedback), None
        consts = None if consts is None else _checked_consts(consts, spec, B)
        self._set = scene if isinstance(scene, SceneSet) else None
        if self._set is None and scene_id is not None:
            raise ValueError("scene_id goes with a SceneSet")
        if self._set is not None:
            if scene_id is None and scene.S > 1:
                raise ValueError("a SceneSet of several scenes needs scene_id")
            sid = np.zeros(B, np.int32) if scene_id is None else np.asarray(
                scene_id.cpu() if isinstance(scene_id, torch.Tensor) else scene_id)
            if sid.shape != (B,) or (sid < 0).any() or (sid >= scene.S).any():
                raise ValueError(f"scene_id must hold B indices in [0, {scene.S})")
            sid = sid.astype(np.int32)
        self.scene, self.spec, self.B, self.rate = scene, spec, B, rate
        self.solver = BatchedCentroidalMPC(spec, device=device)
        self.device = self.solver.device
        self.builder = DeviceRecordBuilder(scene, device=self.device)
        dev, f64 = self.device, torch.float64
        self.consts = None if consts is None else torch.from_numpy(consts).to(dev)
        self.gains, self.last_gain = bool(gains), None
        self.state = torch.zeros((B, 16), dtype=f64, device=dev)
        self.state[:, 14] = scene.params['mass'] if mass is None else torch.as_tensor(mass, dtype=f64, device=dev)
        self.state[:, 15] = torch.as_tensor(mu, dtype=f64, device=dev)
        self.t = torch.zeros(B, dtype=torch.int32, device=dev)
        self.warm = None
        # solver states of the previous / this tick (cmpc_solve_batch_state), swapped every tick
        self._state = [self.solver.new_state(B), self.solver.new_state(B)]
        self.alive = torch.ones(B, dtype=torch.bool, device=dev)
        # per-instance plans and the shared schedule (:656-675)
        self.update_contact = update_contact
        self.flag = torch.zeros(B, dtype=torch.bool, device=dev)             # update_contact_flag
        self.counter = torch.zeros(B, dtype=torch.bool, device=dev)          # model_state['counter'] of the last tick
        self.hw_offset = None if hw_offset is None else torch.as_tensor(np.asarray(hw_offset), dtype=f64, device=dev)
        self._gl = torch.from_numpy(np.ascontiguousarray(scene.gl_tab)).to(dev)
        self._gr = torch.from_numpy(np.ascontiguousarray(scene.gr_tab)).to(dev)
        self._wbc = None
        if self._set is not None:
            self._init_set(sid, hw_measured)
            return
        self.plan_pos = torch.from_numpy(scene.plan_pos).to(dev).repeat(B, 1, 1).contiguous()
        cond, is_ds, wb_slot, wb_row = rollout_schedule(scene, spec.N, rate)
        self._cond = torch.from_numpy(cond).to(dev)
        self._is_ds = torch.from_numpy(is_ds).to(dev)
        self._wb_slot = torch.from_numpy(wb_slot).to(dev)
        self._wb_row = torch.from_numpy(wb_row).to(dev)
        self.hw_measured = None if hw_measured is None else torch.as_tensor(np.asarray(hw_measured), dtype=f64, device=dev)

    def _init_set(self, sid, hw_measured):
        """The per-instance side of a scene set: scene indices, plans (padded to n_steps_max) and momentum recordings."""
        sset, dev, f64 = self._set, self.device, torch.float64
        self.scene_id = torch.from_numpy(sid).to(dev)
        self._sid = self.scene_id.long()
        self._t_last = torch.from_numpy(sset.T.astype(np.int64) - 1).to(dev)[self._sid]      # last tick of the instance's scene
        self.plan_pos = torch.from_numpy(sset.plan_pos).to(dev)[self._sid].contiguous()
        self._warm_buf = torch.empty((self.B, self.spec.nsol), dtype=f64, device=dev)
        if self.update_contact:
            self.builder.set_schedule(sset, self.spec.N, self.rate)
        # one recording for every scene, or one per scene (rows of different length padded with NaN, never read)
        self.hw_measured = None
        if hw_measured is not None:
            one = not isinstance(hw_measured, (list, tuple))
            recs = [np.asarray(h, dtype=np.float64) for h in ([hw_measured] if one else hw_measured)]
            if not one and len(recs) != sset.S:
                raise ValueError(f"hw_measured: one recording, or a list of one per scene ({sset.S})")
            pad = np.full((len(recs), max(len(h) for h in recs), 3), np.nan)
            for i, h in enumerate(recs):
                pad[i, :len(h)] = h
            self.hw_measured = torch.from_numpy(pad).to(dev)
            self._hw_sid = torch.zeros(self.B, dtype=torch.int64, device=dev) if one else self._sid
            self._hw_last = torch.tensor([len(h) - 1 for h in recs], dtype=torch.int64, device=dev)[self._hw_sid]

    def attach_whole_body(self, qp, model):
        """Run the whole-body QP inside every tick.  ``qp``: a ``wbc.BatchedInverseDynamicsQP``; ``model(rollout, desired)``
        returns the device tensors (Hq, Fq, M, h, Jc) of its ``solve`` from the caller's rigid-body library (DART in the
        reference, code/inverse_dynamics.py:46-66, :107-111) and ``desired`` = dict(com_pos, com_vel, com_acc (B,3),
        gamma_l, gamma_r (B,)) -- what code/simulation.py:214-232 hands over from the MPC's ``model_state``.  The
        result of the last tick is kept in ``last_wbc`` = (tau (B,24), qdd, f_c, status, iters)."""
        self._wbc = (qp, model, None)
        self.last_wbc = None

    def attach_whole_body_tasks(self, qp, model, mu=None, foot_size=None):
        """``attach_whole_body`` from the task form: ``model(rollout, desired)`` returns the task inputs of
        ``qp.solve_tasks`` -- (J, Jdot, ff, pos_error, vel_error, qd, M, h[, joint_selection[, gains]]) -- and the rollout
        supplies the rest per instance: contact = (gamma_l, gamma_r) of the instance's own scene and tick, mu = the
        friction the MPC runs with (``state[:, 15]``) unless given here, foot_size (default: the qp's)."""
        self._wbc = (qp, model, dict(mu=mu, foot_size=foot_size))
        self.last_wbc = None

    def _whole_body(self, x1, u0):
        """The consumer of the tick: whole-body QP on the same stream, no host hop."""
        if self._wbc is None:
            return
        qp, model, tasks = self._wbc
        desired = self.desired_com(x1, u0, self.t)
        if tasks is None:
            self.last_wbc = qp.solve(*model(self, desired))
            return
        args = tuple(model(self, desired))
        contact = torch.stack([desired["gamma_l"], desired["gamma_r"]], dim=1).to(torch.float64).contiguous()
        mu = self.state[:, 15].contiguous() if tasks["mu"] is None else tasks["mu"]
        self.last_wbc = qp.solve_tasks(*args[:8], contact, mu, tasks["foot_size"], *args[8:])
        if hasattr(model, "advance"):                      # (``BatchedRobot.walking_model``: q, v move by the QP's acceleration)
            model.advance(self, self.last_wbc)

    def desired_com(self, x1, u0, t):
        """``model_state['com']`` of the reference's back half (:633-649) for the batch: position and velocity of x_1 and
        CoM_acc = (gamma_l sum F_l + gamma_r sum F_r) / m + (0, 0, -g) from u_0 and the contact flags at tick t."""
        nv = self.spec.nv
        if self._set is None:
            tl = torch.clamp(t.long(), max=self._gl.shape[0] - 1)
            gl, gr = self._gl[tl], self._gr[tl]
        else:                                                                 # the flags of the instance's own scene
            tl = torch.minimum(t.long(), self._t_last)
            gl, gr = self._gl[self._sid, tl], self._gr[self._sid, tl]
        F = u0[:, :6 * nv].reshape(-1, 2, nv, 3).sum(dim=2)                  # (B, foot, 3)
        acc = (gl[:, None] * F[:, 0] + gr[:, None] * F[:, 1]) / self.state[:, 14:15]
        acc = acc + torch.tensor([0.0, 0.0, -self.spec.g], dtype=torch.float64, device=self.device)
        return {"com_pos": x1[:, 0:3], "com_vel": x1[:, 3:6], "com_acc": acc, "gamma_l": gl, "gamma_r": gr}

    def _hw_at(self, t):
        if self._set is not None:
            h = self.hw_measured[self._hw_sid, torch.minimum(t.long(), self._hw_last)]
            return h if self.hw_offset is None else h + self.hw_offset
        h = self.hw_measured[torch.clamp(t.long(), max=self.hw_measured.shape[0] - 1)]
        return h if self.hw_offset is None else h + self.hw_offset

    def _measure(self, push_dv):
        """The head of a tick with ``feedback``: the attached model's measurement into ``state`` and ``alive``."""
        if push_dv is not None:
            raise ValueError("push_dv does not go with feedback=True: the next measurement would overwrite it; disturb the robot "
                             "through its own q, v")
        model = None if self._wbc is None else self._wbc[1]
        if not hasattr(model, "measure"):
            raise RuntimeError("feedback=True needs an attached model with a measure(rollout), such as BatchedRobot.walking_model "
                               "(attach_whole_body_tasks)")
        self.last_measurement = model.measure(self)

    def reset(self, t0, com, dcom, hw=None, theta_hat=None):
        """Every instance at tick t0 with the given centroidal state, the scene's plan, no warm start, alive.  With
        ``feedback`` the first measurement replaces com, dcom and hw by the robot's own."""
        dev, f64 = self.device, torch.float64
        self.t[:] = torch.as_tensor(t0, dtype=torch.int32, device=dev)
        self.state[:, 0:3] = torch.as_tensor(com, dtype=f64, device=dev)
        self.state[:, 3:6] = torch.as_tensor(dcom, dtype=f64, device=dev)
        if hw is not None:
            self.state[:, 6:9] = torch.as_tensor(hw, dtype=f64, device=dev)
        elif self.hw_measured is not None:
            self.state[:, 6:9] = self._hw_at(self.t)
        else:
            self.state[:, 6:9] = 0.0
        self.state[:, 9:12] = 0.0 if theta_hat is None else torch.as_tensor(theta_hat, dtype=f64, device=dev)
        self.state[:, 12:14] = 0.0
        self.warm = None
        self._state[0].zero_()
        self.alive[:] = True
        self.flag[:] = False
        if self._set is not None:
            self.plan_pos = torch.from_numpy(self._set.plan_pos).to(dev)[self._sid].contiguous()
        else:
            self.plan_pos = torch.from_numpy(self.scene.plan_pos).to(dev).repeat(self.B, 1, 1).contiguous()

    def _solve_tick(self, rec, s_in, s_out):
        if self.gains:
            # (one gain buffer for the rollout: every tick writes all of it)
            *res, self.last_gain = self.solver.solve_with_gain(rec, warm=self.warm, state=s_in, state_out=s_out, gain=self.last_gain,
                                                               consts=self.consts)
            return tuple(res)
        if self.consts is not None:
            return self.solver.solve_with_consts(rec, self.consts, warm=self.warm, state=s_in, state_out=s_out)
        return self.solver.solve(rec, warm=self.warm, state=s_in, state_out=s_out)

    def track(self, x_meas, columns=0xFFF):
        """The last tick's gain applied to a measured state x_meas (B, 20), in the layout of x0: (x1, u0, used) of
        ``BatchedCentroidalMPC.track`` on ``last_records``, ``last_XU`` and ``last_gain``.  Needs ``gains=True`` and a tick."""
        if self.last_gain is None:
            raise RuntimeError("track needs a rollout built with gains=True that has made a step")
        return self.solver.track(self.last_records, self.last_XU, self.last_gain, x_meas, columns=columns)

    def _step_set(self, push_dv):
        """``step`` of a fleet: records by (scene, tick), the solve, then the back half in one launch."""
        sp, N, dev = self.spec, self.spec.N, self.device
        if self.feedback:
            self._measure(push_dv)
        rec = self.builder.build(sp, self.t, self.state, rate=self.rate, scene_id=self.scene_id,
                                 plan_pos=self.plan_pos if self.update_contact else None)
        s_in, s_out = self._state
        XU, status, iters, kkt = self._solve_tick(rec, s_in, s_out)
        self._state = [s_out, s_in]
        x1 = XU[:, 20:40]
        u0 = XU[:, 20 * (N + 1):20 * (N + 1) + sp.nu]
        self.last_records, self.last_XU, self.last_status, self.last_iters = rec, XU, status, iters
        self._whole_body(x1, u0)
        hw_next = None if self.hw_measured is None else self._hw_at(self.t + self.rate)
        if push_dv is not None:
            push_dv = torch.as_tensor(push_dv, dtype=torch.float64, device=dev).expand(self.B, 3).contiguous()
        self.builder.advance(sp, self.rate, self.scene_id, XU, status, self.t, self.state, self.alive, self._warm_buf,
                             flag=self.flag, counter=self.counter, plan_pos=self.plan_pos, hw_next=hw_next, push_dv=push_dv,
                             update_contact=self.update_contact, copy_all_warm=self.warm is None)
        self.warm = self._warm_buf
        return x1, u0, status

    def step(self, push_dv=None):
        """One control tick for every instance.  Returns (x1 (B,20), u0 (B,nu), status (B,))."""
        if self._set is not None:
            return self._step_set(push_dv)
        sp, N = self.spec, self.spec.N
        if self.feedback:
            self._measure(push_dv)
        rec = self.builder.build(sp, self.t, self.state, rate=self.rate,
                                 plan_pos=self.plan_pos if self.update_contact else None)
        s_in, s_out = self._state
        XU, status, iters, kkt = self._solve_tick(rec, s_in, s_out)
        ok = usable(status) & self.alive
        self._state = [s_out, s_in]              # (an instance whose solve failed stops for good, see `alive`)
        x1 = XU[:, 20:40]
        u0 = XU[:, 20 * (N + 1):20 * (N + 1) + sp.nu]
        self.last_records, self.last_XU, self.last_status, self.last_iters = rec, XU, status, iters
        self._whole_body(x1, u0)
        # plan write-back (:656-675), per instance
        tl = self.t.long()
        if self.update_contact:
            fire = self._cond[tl] & ~self.flag & ok
            rows = self._wb_row[tl]
            cols = 20 * N + rows[:, None] + torch.arange(3, device=self.device)[None, :]
            landing = torch.gather(XU, 1, cols)                               # x_collect[17:20 or 13:16, N]
            b = torch.nonzero(fire, as_tuple=True)[0]
            self.plan_pos[b, self._wb_slot[tl][b]] = landing[b]
            self.flag = (self.flag | fire) & ~(self._is_ds[tl] & ok)
            self.counter = fire
        # instances whose solve failed stop moving (the reference raises, :605-614); the rest advance
        self.alive = ok
        nxt = self.state.clone()
        nxt[:, 0:12] = x1[:, 0:12]
        if self.hw_measured is not None:
            nxt[:, 6:9] = self._hw_at(self.t + self.rate)
        if push_dv is not None:
            nxt[:, 3:6] += torch.as_tensor(push_dv, dtype=torch.float64, device=self.device)
        self.state = torch.where(ok[:, None], nxt, self.state)
        # x_1 is the state delta = rate * world_time_step ahead, and the reference solves every `rate`-th tick
        # (code/simulation.py:203): schedule time moves with the state
        self.t = torch.where(ok, self.t + self.rate, self.t).to(torch.int32)
        self.warm = XU if self.warm is None else torch.where(ok[:, None], XU, self.warm)
        return x1, u0, status

    def run(self, ticks, push=None):
        """`ticks` control steps; push = (first_tick, last_tick, dv(3)) velocity disturbance per tick.
        Returns the CoM history (ticks+1, B, 3) and the final alive mask."""
        if self.feedback and push is not None:
            raise ValueError("push does not go with feedback=True: disturb the robot through its own q, v")
        hist = [self.state[:, 0:3].clone()]
        for i in range(ticks):
            dv = push[2] if (push is not None and push[0] <= i <= push[1]) else None
            self.step(dv)
            hist.append(self.state[:, 0:3].clone())
        return torch.stack(hist), self.alive

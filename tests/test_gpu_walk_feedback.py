"""GPU tier of the measurement that closes the walking loop (cmpc_walk_measure; one wavefront -- one workgroup -- per robot)
and of ``BatchedRollout(feedback=True)``: every row of a launch bit for bit the emulated source's
(tests/emu/walk_measure_emu.cpp), past the resident grid, on a side stream with NULL outputs, on the rows that must not be
fed back; and inside the closed-loop rollout, where every tick equals the by-hand sequence evaluate -> measure -> build ->
solve -> desired_com -> task_references -> solve_tasks -> integrate bit for bit, through the tick of the plan write-back, for
one scene and for a fleet.  Whether the robots stay upright is not asserted anywhere: it is unmeasured.

Shapes: B = 1, B = 257 (a workgroup holds one robot, so there is no per-workgroup edge; 257 is odd and more than one block),
one batch longer than the resident grid, and six robots in the closed loops, started at the tick that
tests/test_walk_measure_emu.py shows the C oracle to solve from the measured state."""
import functools

import numpy as np
import pytest
import torch

import rbd_common as rc
import walk_measure_common as mc
from cmpc_amd import rbd, wbc, workloads as wl
from cmpc_amd.problem import ProblemSpec
from cmpc_amd.rollout import BatchedRollout
from cmpc_amd.solver import usable
from scenes_common import NAMES, five_scenes
from test_walk import measured_hw
from test_walk_measure_emu import check_bad_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_BIG = 257
Z_MIN, TILT_MAX = 0.5, 0.6                                    # of the launch tests: some of the drawn robots are below / past them
FALL = (0.4, 0.5)                                             # of the closed loops


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # (a writable copy: the cached instances are read-only)


@functools.lru_cache(maxsize=None)
def robot():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device: the HIP extension must run, there is no fallback")
    return rbd.BatchedRobot(rc.model("hrp4"), device=DEV, g=rc.G)


@functools.lru_cache(maxsize=None)
def launch_case():
    """(centroid, pose, state, alive) of 257 robots, read-only: the evaluations of ``rc.sample``, one robot in ten dead."""
    cen, pose, state = mc.mirror_case("hrp4", B_BIG)
    alive = (np.random.default_rng(93).uniform(size=B_BIG) >= 0.1).astype(np.uint8)
    alive[B_BIG - 1] = 0
    alive.setflags(write=False)
    return cen, pose, state, alive


@functools.lru_cache(maxsize=None)
def emulated_launch():
    out = mc.emulate_measure(*launch_case(), Z_MIN, np.cos(TILT_MAX))
    for a in out:
        a.setflags(write=False)
    return out


def launch(cen, pose, state, alive, z_min=Z_MIN, tilt_max=TILT_MAX, outputs=("x_meas", "innovation"), as_bool=False):
    ev = rbd.Evaluation(None, None, None, None, dev(pose), None, dev(cen))
    s = dev(state)
    a = None if alive is None else (dev(alive).bool() if as_bool else dev(alive))
    m = robot().measure(ev, s, a, z_min=z_min, tilt_max=tilt_max, outputs=outputs)
    torch.cuda.synchronize()
    return mc.Measured(s.cpu().numpy(), None if a is None else a.cpu().numpy().astype(np.uint8),
                       *(None if t is None else t.cpu().numpy() for t in m))


def same(got, want, rows=slice(None)):
    for k in mc.Measured._fields:
        g, w = getattr(got, k), getattr(want, k)
        assert (g is None) == (w is None) and (g is None or mc.bits_equal(g, w[rows])), k


@pytest.mark.parametrize("B", [1, B_BIG])
def test_launch_matches_the_emulated_source_bit_for_bit(B):
    want = emulated_launch()
    fed = want.alive == 1
    assert 20 < fed.sum() < B_BIG - 40 and (launch_case()[3] == 1).sum() - fed.sum() > 20      # fed back, dead, and fallen ones
    same(launch(*(a[:B] for a in launch_case()), as_bool=B > 1), want, slice(0, B))


def test_past_the_resident_grid():
    """More robots than workgroups are resident at once: the kernel's instance loop takes its second turn."""
    B = torch.cuda.get_device_properties(DEV).multi_processor_count * 32 + 65
    idx = np.arange(B) % B_BIG
    same(launch(*(a[idx] for a in launch_case())), emulated_launch(), idx)


def test_on_a_side_stream_with_null_outputs_and_null_alive():
    cen, pose, state, alive = launch_case()
    want = mc.emulate_measure(cen, pose, state, None, Z_MIN, np.cos(TILT_MAX), outputs=())
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ev = rbd.Evaluation(None, None, None, None, dev(pose), None, dev(cen))
        s, s2, a2 = dev(state), dev(state), dev(alive)
        none = robot().measure(ev, s, None, z_min=Z_MIN, tilt_max=TILT_MAX, outputs=())
        part = robot().measure(ev, s2, a2, z_min=Z_MIN, tilt_max=TILT_MAX, outputs=("innovation",))
    side.synchronize()
    assert none.x_meas is None and none.innovation is None and part.x_meas is None
    assert mc.bits_equal(s.cpu().numpy(), want.state)
    full = emulated_launch()
    assert mc.bits_equal(s2.cpu().numpy(), full.state) and mc.bits_equal(a2.cpu().numpy(), full.alive)
    assert mc.bits_equal(part.innovation.cpu().numpy(), full.innovation)


@pytest.mark.parametrize("kind", mc.BAD_KINDS)
def test_rows_that_must_not_be_fed_back(kind):
    run = lambda case: launch(case["centroid"], case["pose"], case["state"], case["alive"], mc.Z_MIN, mc.TILT_MAX)
    got = check_bad_rows(kind, run)
    bad = mc.bad_case(kind)[1]
    same(got, mc.emulate_measure(bad["centroid"], bad["pose"], bad["state"], bad["alive"], mc.Z_MIN, np.cos(mc.TILT_MAX)))


def test_bad_arguments_are_refused():
    r = robot()
    cen, pose, state, alive = (dev(a[:4]) for a in launch_case())
    ev = rbd.Evaluation(None, None, None, None, pose, None, cen)
    with pytest.raises(ValueError, match="state"):
        r.measure(ev, state[:, :15].contiguous())
    with pytest.raises(ValueError, match="alive"):
        r.measure(ev, state, alive.to(torch.int32))
    with pytest.raises(ValueError, match="ev.pose"):
        r.measure(rbd.Evaluation(None, None, None, None, pose.float(), None, cen), state)
    with pytest.raises(ValueError, match="unknown outputs"):
        r.measure(ev, state, outputs=("x_meas", "nope"))
    with pytest.raises(RuntimeError, match="NaN"):
        r.measure(ev, state, z_min=float("nan"))
    torch.cuda.synchronize()
    assert torch.equal(state, dev(launch_case()[2][:4]))


# ---- inside the rollout -------------------------------------------------------------------------------------------------------
class Counted:
    """``robot().evaluate`` and ``.measure`` with their calls counted and their results kept (put in place by monkeypatch)."""

    def __init__(self, monkeypatch):
        r = robot()
        self.evaluations, self.measurements = [], []
        ev0, me0 = r.evaluate, r.measure

        def evaluate(*a, **k):
            self.evaluations.append(ev0(*a, **k))
            return self.evaluations[-1]

        def measure(*a, **k):
            self.measurements.append(me0(*a, **k))
            return self.measurements[-1]

        monkeypatch.setattr(r, "evaluate", evaluate)
        monkeypatch.setattr(r, "measure", measure)


def _loop(scene, sid=None, feedback=True, q0=None, nan_mu=True):
    """A rollout of the six standing robots of ``mc.standing_robots`` on ``scene`` at the start tick, with
    ``walking_model`` attached: (rollout, model, q, v, pieces for the by-hand tick)."""
    B, spec = mc.B_LOOP, ProblemSpec(N=mc.N_LOOP)
    scenes = [scene] if sid is None else scene.scenes
    t0 = {mc.start_tick(sc) for sc in scenes}
    assert len(t0) == 1                                       # (the walks share their phase durations)
    t0 = t0.pop()
    ro = BatchedRollout(scene, spec, B, device=DEV, mass=mc.loop_mass(), mu=mc.loop_mu(), scene_id=sid, feedback=feedback)
    qs, vs = mc.standing_robots()
    q, v = dev(qs if q0 is None else q0), dev(vs)
    r, g = robot(), rbd.Gait(scene, device=DEV)
    q_ref = dev(rc.standing())
    model = r.walking_model(q, v, g, q_ref=q_ref, fall=FALL)
    qp = wbc.BatchedInverseDynamicsQP(foot_size=0.1, mu=0.5, device=DEV)
    foot_mu = mc.loop_mu().copy()
    if nan_mu:
        foot_mu[4] = np.nan                                   # this robot's QP fails every tick: it holds
    foot_mu = dev(foot_mu)
    ro.attach_whole_body_tasks(qp, model, mu=foot_mu)
    com, dcom = scene.nominal_state(np.full(B, t0)) if sid is None else scene.nominal_state(np.full(B, t0), sid)
    ro.reset(t0, com, dcom)                                   # (with feedback the first measurement replaces com, dcom, hw)
    return ro, model, q, v, dict(spec=spec, t0=t0, gait=g, q_ref=q_ref, qp=qp, foot_mu=foot_mu, com=com, dcom=dcom)


def _feedback_case(scene, sid, monkeypatch):
    """Three ticks with feedback, the second of which is the tick of the plan write-back.  The twin is a rollout without
    feedback and without a whole-body model: its ``step`` is the unchanged rest of the MPC's tick (build, solve, back half),
    so measure + twin.step() + the whole-body calls by hand is the sequence the tick is held to."""
    B, NANQ, NANMU = mc.B_LOOP, 1, 4
    q0 = np.array(mc.standing_robots()[0])
    q0[NANQ, 10] = np.nan
    ro, model, q, v, p = _loop(scene, sid, q0=q0)
    spec, g, q_ref, qp, foot_mu = p["spec"], p["gait"], p["q_ref"], p["qp"], p["foot_mu"]
    twin = BatchedRollout(scene, spec, B, device=DEV, mass=mc.loop_mass(), mu=mc.loop_mu(), scene_id=sid)
    twin.reset(p["t0"], p["com"], p["dcom"])
    clean, _, qc, vc, _ = _loop(scene, sid)                   # the same without the NaN in q: the neighbours' yardstick
    r, counted = robot(), Counted(monkeypatch)
    s = np.zeros(B, np.int32) if sid is None else sid
    sid_dev = None if sid is None else dev(sid)
    gl, gr = np.atleast_2d(scene.gl_tab), np.atleast_2d(scene.gr_tab)
    sel = dev(rc.model("hrp4").joint_selection(rbd.HRP4_REDUNDANT_DOFS))
    wrote = False
    for i in range(3):
        t_tick, plan, q_in, v_in = ro.t.clone(), ro.plan_pos.clone(), q.clone(), v.clone()
        del counted.evaluations[:], counted.measurements[:]
        x1, u0, status = ro.step()
        # the launch count: one evaluation, made by measure, and the model's references and QP ran on that very tensor set
        assert len(counted.evaluations) == 1 and len(counted.measurements) == 1
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(model.last_evaluation, counted.evaluations[0]))
        assert ro.last_measurement is counted.measurements[0] and model.last_measurement is ro.last_measurement
        got_wbc = [t.clone() for t in ro.last_wbc]
        # by hand
        ev = r.evaluate(q_in, v_in)
        m = r.measure(ev, twin.state, twin.alive, z_min=FALL[0], tilt_max=FALL[1])
        alive_m = twin.alive.clone()
        hx1, hu0, hstatus = twin.step()
        tt = t_tick.cpu().numpy()
        flags = np.stack([gl[s, tt], gr[s, tt]], axis=1).astype(np.float64)
        desired = twin.desired_com(hx1, hu0, t_tick)
        com_des = torch.cat([desired["com_pos"], desired["com_vel"], desired["com_acc"]], dim=1).contiguous()
        refs = r.task_references(g, t_tick, sid_dev, plan, ev, com_des, q_in, v_in, q_ref)
        direct = qp.solve_tasks(ev.J, None, refs.ff, refs.pos_err, refs.vel_err, None, ev.M, ev.h, dev(flags), foot_mu, None, sel)
        hold = (direct[3] != 0) | ~alive_m
        q_hand, v_hand = r.integrate(q_in, v_in, direct[1], spec.delta, hold=hold)
        clean.step()
        torch.cuda.synchronize()
        eq = lambda a, b: mc.bits_equal(a.cpu().numpy(), b.cpu().numpy())
        assert eq(ro.last_records, twin.last_records) and eq(ro.last_XU, twin.last_XU) and eq(status, hstatus), i
        assert eq(ro.state, twin.state) and eq(ro.alive, twin.alive) and eq(ro.t, twin.t) and eq(ro.plan_pos, twin.plan_pos), i
        assert eq(ro.last_measurement.x_meas, m.x_meas) and eq(ro.last_measurement.innovation, m.innovation), i
        for a, d, name in zip(got_wbc, direct, ("tau", "qdd", "f", "status", "iters")):
            assert a.dtype == d.dtype and torch.equal(a, d), (name, i)
        assert eq(q, q_hand) and eq(v, v_hand), i
        # the records are built from the robot: its centroid in words 0..8, its foot angles in words 12 and 16
        fed = alive_m.cpu().numpy()
        rec, cen, pose = ro.last_records.cpu().numpy(), ev.centroid.cpu().numpy(), ev.pose.cpu().numpy()
        assert fed.tolist() == [b != NANQ for b in range(B)] or i > 0
        assert not fed[NANQ] and mc.bits_equal(rec[fed, 0:9], cen[fed])
        assert np.array_equal(rec[fed, 12], pose[fed, 2]) and np.array_equal(rec[fed, 16], pose[fed, 8])
        inn = m.innovation.cpu().numpy()
        assert np.isnan(inn[~fed]).all() and np.isfinite(inn[fed]).all()
        # the robot with a NaN in q is dead from the first measurement on and holds; the one whose QP fails holds q, v
        qp_status, mpc_ok = direct[3].cpu().numpy(), usable(hstatus).cpu().numpy()
        print("tick", int(tt[0]), "fed back", fed.tolist(), "mpc status", hstatus.tolist(), "qp status", qp_status.tolist(),
              "worst |innovation|", float(np.abs(inn[fed]).max()) if fed.any() else None)
        assert not ro.alive[NANQ] and eq(q[NANQ], q_in[NANQ]) and eq(v[NANQ], v_in[NANQ]) and int(ro.t[NANQ]) == p["t0"]
        assert qp_status[NANMU] != 0 and eq(q[NANMU], q_in[NANMU]) and eq(v[NANMU], v_in[NANMU])
        moved = (qp_status == 0) & fed
        assert moved.any() and all(not torch.equal(q[b], q_in[b]) for b in np.nonzero(moved)[0])
        assert (ro.alive.cpu().numpy() & mpc_ok).any()
        # the neighbours: what they do does not depend on the dead robot (the QP-failing one is the same in both runs)
        rest = [b for b in range(B) if b != NANQ]
        assert eq(q[rest], qc[rest]) and eq(v[rest], vc[rest]) and eq(ro.state[rest], clean.state[rest]), i
        if not eq(ro.plan_pos, plan):
            assert i == 1
            wrote = True
    assert wrote, "no robot's plan was rewritten in these ticks"


def test_single_scene_with_feedback_equals_the_by_hand_sequence_every_tick(monkeypatch):
    _feedback_case(five_scenes()[0], None, monkeypatch)


def test_fleet_with_feedback_equals_the_by_hand_sequence_every_tick(monkeypatch):
    scs = five_scenes()
    sset = wl.SceneSet([scs[NAMES.index(n)] for n in ("shipped", "lfirst")])
    _feedback_case(sset, np.array([0, 1, 0, 1, 0, 1], np.int32), monkeypatch)


def test_feedback_makes_the_mpc_see_where_the_robot_is():
    """Robot 0's base 2 cm further along x.  Without feedback the MPC's record and forces are the unshifted run's bit for
    bit; with it the record's CoM moves by the shift and the forces differ."""
    scene, shift = five_scenes()[0], 0.02
    q0 = np.array(mc.standing_robots()[0])
    q0[0, 3] += shift
    out = {}
    for feedback in (False, True):
        for shifted in (False, True):
            ro, _, _, _, _ = _loop(scene, feedback=feedback, q0=q0 if shifted else None, nan_mu=False)
            _, u0, status = ro.step()
            torch.cuda.synchronize()
            out[feedback, shifted] = (ro.last_records.cpu().numpy(), u0.cpu().numpy(), status.cpu().numpy())
    assert mc.bits_equal(out[False, False][0], out[False, True][0]) and mc.bits_equal(out[False, False][1], out[False, True][1])
    rec0, rec1 = out[True, False][0], out[True, True][0]
    print("record com_x of robot 0:", rec0[0, 0], "->", rec1[0, 0], "status", out[True, False][2].tolist(), out[True, True][2].tolist())
    assert abs((rec1[0, 0] - rec0[0, 0]) - shift) < 1e-12 and mc.bits_equal(rec1[1:], rec0[1:])
    assert not np.array_equal(out[True, True][1][0], out[True, False][1][0])
    assert mc.bits_equal(out[True, True][1][1:], out[True, False][1][1:])
    assert not mc.bits_equal(rec0[:, 0:9], out[False, False][0][:, 0:9])


def test_what_does_not_go_with_feedback_is_refused():
    scene, spec, B = five_scenes()[0], ProblemSpec(N=mc.N_LOOP), mc.B_LOOP
    with pytest.raises(ValueError, match="hw_measured"):
        BatchedRollout(scene, spec, B, device=DEV, hw_measured=np.zeros((10, 3)), feedback=True)
    with pytest.raises(ValueError, match="hw_offset"):
        BatchedRollout(scene, spec, B, device=DEV, hw_offset=np.zeros((B, 3)), feedback=True)
    ro, _, q, v, p = _loop(scene)
    state = ro.state.clone()
    with pytest.raises(ValueError, match="push_dv"):
        ro.step(push_dv=[0.1, 0.0, 0.0])
    with pytest.raises(ValueError, match="push"):
        ro.run(2, push=(0, 1, [0.1, 0.0, 0.0]))
    assert torch.equal(ro.state, state) and int(ro.t[0]) == p["t0"]
    bare = BatchedRollout(scene, spec, B, device=DEV, mass=mc.loop_mass(), feedback=True)
    bare.reset(p["t0"], p["com"], p["dcom"])
    with pytest.raises(RuntimeError, match="measure"):
        bare.step()
    bare.attach_whole_body_tasks(p["qp"], robot().task_model(q, v))        # a model that cannot measure
    with pytest.raises(RuntimeError, match="measure"):
        bare.step()


def test_without_feedback_nothing_is_measured(monkeypatch):
    ro, model, q, v, p = _loop(five_scenes()[0], feedback=False, nan_mu=False)
    counted = Counted(monkeypatch)
    ro.reset(p["t0"], p["com"], p["dcom"], hw=measured_hw()[p["t0"]])      # (a nominal state at rest is infeasible at this tick)
    state = ro.state.clone()
    x1, u0, status = ro.step()
    torch.cuda.synchronize()
    assert len(counted.measurements) == 0 and len(counted.evaluations) == 1
    assert model.last_measurement is None and ro.last_measurement is None
    assert mc.bits_equal(ro.last_records[:, 0:9].cpu().numpy(), state[:, 0:9].cpu().numpy())
    ok = usable(status).cpu().numpy()
    print("status", status.tolist())
    assert ok.any()
    assert mc.bits_equal(ro.state[:, 0:12].cpu().numpy()[ok], x1[:, 0:12].cpu().numpy()[ok])
    assert mc.bits_equal(ro.state.cpu().numpy()[~ok], state.cpu().numpy()[~ok])

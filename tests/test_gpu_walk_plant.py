"""GPU tier of the contact plant (cmpc_walk_plant_step; one wavefront -- one workgroup -- per robot) and of
``walking_model(plant=...)``: every row of a launch bit for bit the emulated source's (tests/emu/walk_plant_emu.cpp), past
the resident grid, on a side stream with the optional arguments left out and a strided tau, on the rows that must not move;
and inside the closed-loop rollout with feedback, where every tick equals the by-hand sequence evaluate -> measure -> build
-> solve -> desired_com -> task_references -> solve_tasks -> simulate bit for bit, for one scene and for a fleet, and where
a rollout without a plant is still the integrate path.  Whether the robots stay upright is not asserted anywhere.

Shapes: B = 1 and B = 67 (a workgroup holds one robot, so there is no per-workgroup edge; 67 is odd and more than one block,
and small because the harness runs each robot's lanes as threads), one batch longer than the kernel's resident grid (six
robots per CU), and six robots in the closed loops, started at the tick tests/test_gpu_walk_feedback.py starts from."""
import functools

import numpy as np
import pytest
import torch

import rbd_common as rc
import walk_measure_common as mc
import walk_plant_common as pc
from cmpc_amd import rbd, wbc, workloads as wl
from cmpc_amd.problem import ProblemSpec
from cmpc_amd.rollout import BatchedRollout
from scenes_common import NAMES, five_scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_BIG, SWEEPS = 67, 20
FALL = (0.4, 0.5)
TICKS = 12


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # (a writable copy: the cached instances are read-only)


@functools.lru_cache(maxsize=None)
def robot():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device: the HIP extension must run, there is no fallback")
    return rbd.BatchedRobot(rc.model("hrp4"), device=DEV, g=rc.G)


@functools.lru_cache(maxsize=None)
def launch_case():
    """67 robots, read-only: the 16-robot mix of the CPU tier tiled, one robot in eleven held."""
    case = pc.tile(pc.mix_case(), np.arange(B_BIG) % 16)
    case["hold"] = (np.arange(B_BIG) % 11 == 3).astype(np.uint8)
    return pc.frozen(case)


@functools.lru_cache(maxsize=None)
def emulated_launch():
    out = pc.emulate_plant(launch_case(), pc.params(sweeps=SWEEPS))
    for a in out:
        a.setflags(write=False)
    return out


def launch(case, sweeps=SWEEPS, in_place=False, as_bool=False, outputs=rbd.PLANT_OUTPUTS):
    """``BatchedRobot.simulate`` on the case -> ``pc.Stepped`` of numpy; status and residual are pre-filled as the harness's."""
    B = case["q"].shape[0]
    ev = rbd.Evaluation(dev(case["J"]), None, dev(case["M"]), dev(case["h"]), dev(case["pose"]), None, None)
    q, v = dev(case["q"]), dev(case["v"])
    opt = lambda k: None if case.get(k) is None else dev(case[k])
    hold = opt("hold")
    if hold is not None and as_bool:
        hold = hold.bool()
    s = robot().simulate(q, v, ev, opt("tau"), dev(case["foot_mu"]), rbd.Plant(pc.DT, sweeps=sweeps), ext=opt("ext"), hold=hold,
                         impulse=opt("impulse"), out=(q, v) if in_place else None, outputs=outputs)
    torch.cuda.synchronize()
    assert tuple(s.q.shape) == (B, 30) and (not in_place or (s.q is q and s.v is v))
    return pc.Stepped(*(None if t is None else t.cpu().numpy() for t in s))


def same(got, want, rows=slice(None), held=None):
    for k in pc.Stepped._fields:
        g, w = getattr(got, k), getattr(want, k)[rows]
        if k == "residual" and held is not None:                 # a held row's residual is not touched: whatever was there
            g, w = g[~held], w[~held]
        assert pc.bits_equal(g, w), k


@pytest.mark.parametrize("B", [1, B_BIG])
def test_launch_matches_the_emulated_source_bit_for_bit(B):
    want = emulated_launch()
    held = launch_case()["hold"] != 0
    assert (want.status[held] == 1).all() and (want.status[~held] == 0).all() and 3 < held.sum() < 10
    assert (want.impulse.reshape(B_BIG, 8, 3)[:, :, 2] > 0).any(axis=1).sum() > 20
    same(launch(pc.tile(launch_case(), np.arange(B)), in_place=B > 1, as_bool=B > 1), want, slice(0, B), held[:B])


def test_past_the_resident_grid():
    """More robots than workgroups are resident at once: the kernel's instance loop takes its second turn."""
    B = torch.cuda.get_device_properties(DEV).multi_processor_count * pc.emu_lib().cmpc_emu_walk_plant_per_cu() + 65
    idx = np.arange(B) % B_BIG
    same(launch(pc.tile(launch_case(), idx)), emulated_launch(), idx, launch_case()["hold"][idx] != 0)


def test_on_a_side_stream_with_the_optional_arguments_left_out_and_a_strided_tau():
    case = launch_case()
    bare = dict(case, ext=None, hold=None, impulse=None)
    want = pc.emulate_plant(bare, pc.params(sweeps=SWEEPS), outputs=())
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ev = rbd.Evaluation(dev(case["J"]), None, dev(case["M"]), dev(case["h"]), dev(case["pose"]), None, None)
        wide = torch.full((B_BIG, 30), float("nan"), dtype=torch.float64, device=DEV)
        wide[:, 6:] = dev(case["tau"])
        tau = wide[:, 6:]
        assert not tau.is_contiguous()
        got = robot().simulate(dev(case["q"]), dev(case["v"]), ev, tau, dev(case["foot_mu"]), rbd.Plant(pc.DT, sweeps=SWEEPS), outputs=())
        none = robot().simulate(dev(case["q"]), dev(case["v"]), ev, None, dev(case["foot_mu"]), rbd.Plant(pc.DT, sweeps=SWEEPS),
                                outputs=("residual",))
    side.synchronize()
    assert got.impulse is None and got.status is None and got.residual is None
    assert pc.bits_equal(got.q.cpu().numpy(), want.q) and pc.bits_equal(got.v.cpu().numpy(), want.v)
    limp = pc.emulate_plant(dict(bare, tau=None), pc.params(sweeps=SWEEPS), outputs=("residual",))
    assert pc.bits_equal(none.v.cpu().numpy(), limp.v) and pc.bits_equal(none.residual.cpu().numpy(), limp.residual)
    assert none.impulse is None and none.status is None


@pytest.mark.parametrize("kind", pc.BAD_KINDS)
def test_rows_that_must_not_move(kind):
    got = pc.check_bad_row(kind, lambda case: launch(case, sweeps=5))
    want = pc.emulate_plant(pc.bad_case(kind)[1], pc.params(sweeps=5))
    same(got, want, held=pc.bad_case(kind)[1]["hold"] != 0)


def test_bad_arguments_are_refused():
    r, case = robot(), pc.tile(launch_case(), np.arange(4))
    ev = rbd.Evaluation(dev(case["J"]), None, dev(case["M"]), dev(case["h"]), dev(case["pose"]), None, None)
    q, v, tau, fm = dev(case["q"]), dev(case["v"]), dev(case["tau"]), dev(case["foot_mu"])
    plant = rbd.Plant(pc.DT)
    with pytest.raises(ValueError, match="rbd.Plant"):
        r.simulate(q, v, ev, tau, fm, 0.01)
    with pytest.raises(ValueError, match="ev.M"):
        r.simulate(q, v, rbd.Evaluation(ev.J, None, ev.M[:, :29].contiguous(), ev.h, ev.pose, None, None), tau, fm, plant)
    with pytest.raises(ValueError, match="tau"):
        r.simulate(q, v, ev, dev(np.zeros((4, 48)))[:, ::2], fm, plant)
    with pytest.raises(ValueError, match="tau"):
        r.simulate(q, v, ev, tau.float(), fm, plant)
    with pytest.raises(ValueError, match="foot_mu"):
        r.simulate(q, v, ev, tau, fm[:, :1].contiguous(), plant)
    with pytest.raises(ValueError, match="hold"):
        r.simulate(q, v, ev, tau, fm, plant, hold=torch.zeros(4, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="impulse"):
        r.simulate(q, v, ev, tau, fm, plant, impulse=torch.zeros((4, 8), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="unknown outputs"):
        r.simulate(q, v, ev, tau, fm, plant, outputs=("nope",))
    for name, value in (("sweeps", -1), ("dt", 0.0), ("erp", 2.0), ("cfm", -1.0), ("ground_z", float("inf"))):
        broken = rbd.Plant(pc.DT)
        setattr(broken, name, value)                             # past the checks of Plant: the native validation's turn
        with pytest.raises(RuntimeError, match=name):
            r.simulate(q, v, ev, tau, fm, broken, out=(q, v))
    torch.cuda.synchronize()
    assert torch.equal(q, dev(case["q"])) and torch.equal(v, dev(case["v"]))


# ---- inside the rollout -------------------------------------------------------------------------------------------------------
def _loop(scene, sid, plant, ext=None, feedback=True):
    """A rollout of the six standing robots of ``mc.standing_robots`` on ``scene`` at the start tick of
    tests/test_gpu_walk_feedback.py with ``walking_model(plant=plant)`` attached; robot 4's QP fails every tick."""
    B, spec = mc.B_LOOP, ProblemSpec(N=mc.N_LOOP)
    t0 = {mc.start_tick(sc) for sc in ([scene] if sid is None else scene.scenes)}
    assert len(t0) == 1
    t0 = t0.pop()
    ro = BatchedRollout(scene, spec, B, device=DEV, mass=mc.loop_mass(), mu=mc.loop_mu(), scene_id=sid, feedback=feedback)
    qs, vs = mc.standing_robots()
    q, v = dev(qs), dev(vs)
    r, g = robot(), rbd.Gait(scene, device=DEV)
    q_ref = dev(rc.standing())
    model = r.walking_model(q, v, g, q_ref=q_ref, fall=FALL, plant=plant, ext=ext)
    qp = wbc.BatchedInverseDynamicsQP(foot_size=0.1, mu=0.5, device=DEV)
    foot_mu = mc.loop_mu().copy()
    foot_mu[4] = np.nan
    foot_mu = dev(foot_mu)
    ro.attach_whole_body_tasks(qp, model, mu=foot_mu)
    com, dcom = scene.nominal_state(np.full(B, t0)) if sid is None else scene.nominal_state(np.full(B, t0), sid)
    ro.reset(t0, com, dcom)
    return ro, model, q, v, dict(spec=spec, t0=t0, gait=g, q_ref=q_ref, qp=qp, foot_mu=foot_mu, com=com, dcom=dcom)


def _plant_case(scene, sid):
    B, plant = mc.B_LOOP, rbd.Plant(ProblemSpec(N=mc.N_LOOP).delta, sweeps=SWEEPS)
    push = np.zeros((B, 6))
    push[2, 4] = push[3, 4] = 6.0                                # the reference's 3 N on base and torso, summed onto the base
    ext = dev(push)
    ro, model, q, v, p = _loop(scene, sid, plant, ext)
    spec, g, q_ref, qp, foot_mu = p["spec"], p["gait"], p["q_ref"], p["qp"], p["foot_mu"]
    twin = BatchedRollout(scene, spec, B, device=DEV, mass=mc.loop_mass(), mu=mc.loop_mu(), scene_id=sid)
    twin.reset(p["t0"], p["com"], p["dcom"])
    r = robot()
    s = np.zeros(B, np.int32) if sid is None else sid
    sid_dev = None if sid is None else dev(sid)
    gl, gr = np.atleast_2d(scene.gl_tab), np.atleast_2d(scene.gr_tab)
    sel = dev(rc.model("hrp4").joint_selection(rbd.HRP4_REDUNDANT_DOFS))
    floor = dev(np.stack([np.full(B, 0.05), mc.loop_mu()], axis=1))
    imp_hand = torch.zeros((B, 24), dtype=torch.float64, device=DEV)
    eq = lambda a, b: pc.bits_equal(a.cpu().numpy(), b.cpu().numpy())
    touched = False
    for i in range(TICKS):
        t_tick, plan, q_in, v_in = ro.t.clone(), ro.plan_pos.clone(), q.clone(), v.clone()
        ro.step()
        ev = r.evaluate(q_in, v_in)
        r.measure(ev, twin.state, twin.alive, z_min=FALL[0], tilt_max=FALL[1])
        alive_m = twin.alive.clone()
        hx1, hu0, hstatus = twin.step()
        tt = np.minimum(t_tick.cpu().numpy(), gl.shape[1] - 1)
        flags = np.stack([gl[s, tt], gr[s, tt]], axis=1).astype(np.float64)
        desired = twin.desired_com(hx1, hu0, t_tick)
        com_des = torch.cat([desired["com_pos"], desired["com_vel"], desired["com_acc"]], dim=1).contiguous()
        refs = r.task_references(g, t_tick, sid_dev, plan, ev, com_des, q_in, v_in, q_ref)
        direct = qp.solve_tasks(ev.J, None, refs.ff, refs.pos_err, refs.vel_err, None, ev.M, ev.h, dev(flags), foot_mu, None, sel)
        hand = r.simulate(q_in, v_in, ev, direct[0], floor, plant, ext=ext, hold=~alive_m, impulse=imp_hand)
        torch.cuda.synchronize()
        assert eq(q, hand.q) and eq(v, hand.v) and eq(model.impulse, imp_hand), i
        assert eq(ro.state, twin.state) and eq(ro.alive, twin.alive) and eq(ro.t, twin.t), i
        assert eq(model.last_plant.status, hand.status) and eq(model.last_plant.residual, hand.residual), i
        assert model.last_plant.q is q and model.last_plant.impulse is model.impulse
        status = hand.status.cpu().numpy()
        fed = alive_m.cpu().numpy()
        print("tick", int(tt[0]), "alive", fed.tolist(), "plant status", status.tolist(), "qp status", direct[3].tolist(),
              "largest residual", float(np.nanmax(hand.residual.cpu().numpy()[status == 0], initial=0.0)))
        assert (status[~fed] == 1).all() and (status[fed] == 0).all()
        # the robot whose QP fails is not held: it moves, limp
        assert direct[3][4] != 0 and (not fed[4] or not eq(q[4], q_in[4]))
        touched = touched or bool((imp_hand.reshape(B, 8, 3)[:, :, 2] > 0).any())
    assert touched, "no robot ever touched the floor"


def test_single_scene_with_the_plant_equals_the_by_hand_sequence_every_tick():
    _plant_case(five_scenes()[0], None)


def test_fleet_with_the_plant_equals_the_by_hand_sequence_every_tick():
    scs = five_scenes()
    sset = wl.SceneSet([scs[NAMES.index(n)] for n in ("shipped", "lfirst")])
    _plant_case(sset, np.array([0, 1, 0, 1, 0, 1], np.int32))


def test_without_a_plant_the_rollout_is_the_integrate_path_bit_for_bit():
    """The same rollout with plant=None: every tick's (q, v) are ``integrate`` of the tick's own QP acceleration with hold =
    QP failed or not alive, and the model carries nothing of the plant's."""
    ro, model, q, v, p = _loop(five_scenes()[0], None, None)
    assert not hasattr(model, "impulse") and not hasattr(model, "last_plant")
    r = robot()
    for i in range(3):
        q_in, v_in, alive_in = q.clone(), v.clone(), ro.alive.clone()
        ro.step()
        alive_m = alive_in & torch.isfinite(ro.last_measurement.x_meas).all(dim=1)
        hold = (ro.last_wbc[3] != 0) | ~alive_m
        q_hand, v_hand = r.integrate(q_in, v_in, ro.last_wbc[1], p["spec"].delta, hold=hold)
        torch.cuda.synchronize()
        assert torch.equal(q, q_hand) and torch.equal(v, v_hand), i
        assert torch.equal(q[4], q_in[4]) and not torch.equal(q[0], q_in[0])

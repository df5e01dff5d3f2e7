"""GPU tier of the rigid-body model with per-robot inertial parameters (cmpc_rbd_eval_inertial, rbd_eval_inertial_kernel; one
wavefront -- one workgroup -- per robot): every row of a launch bit for bit the emulated source's
(tests/emu/rbd_inertial_emu.cpp) for HRP-4, the 24-joint chain and the 24-joint star, past the resident grid; a table of the
model's own rows against the plain ``evaluate``; bad rows at both ends of a batch; refusals, ``set_inertial(None)`` and a side
stream; evaluate -> solve_tasks on standing robots that carry a box; and inside the closed-loop rollout with feedback on the
contact plant, where every tick equals the by-hand sequence bit for bit, the robots without a payload equal the same rollout
on a robot without a table, and a row rewritten between two ticks changes that robot alone.  Whether a payload makes a
robot fall is not asserted anywhere.

Shapes: B = 1 and B = 67 (a workgroup holds one robot, so there is no per-workgroup edge; 67 is odd and more than one
block), one batch longer than the kernel's resident grid (six robots per CU), all three tiled from the CPU tier's eight
(q, v, row) triples, and six robots in the closed loop."""
import functools

import numpy as np
import pytest
import torch

import rbd_common as rc
import rbd_inertial_common as ic
import walk_measure_common as mc
from cmpc_amd import rbd, wbc
from cmpc_amd.problem import ProblemSpec
from cmpc_amd.rollout import BatchedRollout
from scenes_common import five_scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_BIG, SWEEPS = 67, 20
FALL = (0.4, 0.5)
LOOP_PAYLOADS = (0.0, 0.0, 0.7, 2.0, 2.5, 2.5)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # (a writable copy: the cached instances are read-only)


def robot(name, inertial=None):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device: the HIP extension must run, there is no fallback")
    return rbd.BatchedRobot(rc.model(name), device=DEV, g=rc.G, inertial=inertial)


def host(ev):
    return rbd.Evaluation(*(None if t is None else t.cpu().numpy() for t in ev))


def launch(name, q, v, tab, outputs=rc.FIELDS):
    out = robot(name, dev(tab)).evaluate(dev(q), dev(v), outputs=outputs)
    torch.cuda.synchronize()
    return host(out)


def same_bits(got, want, rows=slice(None)):
    for k in rc.FIELDS:
        assert ic.bits_equal(getattr(got, k), getattr(want, k)[rows]), k


def resident_plus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count * 6 + 65     # (25.4 KB of LDS per workgroup: six per CU)


@pytest.mark.parametrize("B", [1, B_BIG, "past the resident grid"])
@pytest.mark.parametrize("name", rc.MODELS)
def test_every_row_is_the_emulated_sources_bit_for_bit(name, B):
    """The CPU tier's eight robots, every one its own model, tiled; the longest batch takes the kernel's instance loop into
    its second turn."""
    B = resident_plus() if isinstance(B, str) else B
    idx = np.arange(B) % 8
    (q, v), tab = rc.sample(name), ic.rows(name)
    got = launch(name, q[idx], v[idx], tab[idx])
    same_bits(got, ic.emulated(name), idx)
    assert np.array_equal(got.M, np.swapaxes(got.M, 1, 2)) and all(np.isfinite(getattr(got, k)).all() for k in rc.FIELDS)


def test_a_table_of_the_models_own_rows_equals_the_plain_evaluate_bit_for_bit():
    idx = np.arange(B_BIG) % 8
    q, v = (a[idx] for a in rc.sample("hrp4"))
    r = robot("hrp4")
    plain = r.evaluate(dev(q), dev(v))
    assert r.inertial is None and r.total_mass == rc.model("hrp4").total_mass
    r.set_inertial(dev(np.tile(rc.model("hrp4").inertial(), (B_BIG, 1, 1))))
    own = r.evaluate(dev(q), dev(v))
    torch.cuda.synchronize()
    same_bits(host(own), host(plain))
    same_bits(host(own), rc.emulated("hrp4"), idx)


def test_bad_rows_at_both_ends_leave_their_neighbours_untouched():
    idx = np.arange(B_BIG) % 8
    (q, v), tab = rc.sample("hrp4"), np.array(ic.rows("hrp4")[idx])
    tab[0, 24, 9] = np.nan                                    # the row's last word
    tab[B_BIG - 1, 0, 0] = -1.0                               # a negative mass, the row's first
    got = launch("hrp4", q[idx], v[idx], tab)
    for k in rc.FIELDS:
        a = getattr(got, k)
        assert np.isnan(a[0]).all() and np.isnan(a[B_BIG - 1]).all(), k
    same_bits(rbd.Evaluation(*(a[1:B_BIG - 1] for a in got)), ic.emulated("hrp4"), idx[1:B_BIG - 1])
    # a robot without any mass, and one whose total overflows, in the middle
    tab = np.array(ic.rows("hrp4")[idx])
    tab[30, :, 0] = 0.0
    tab[31, :, 0] = 1e308
    got = launch("hrp4", q[idx], v[idx], tab)
    keep = np.delete(np.arange(B_BIG), (30, 31))
    assert all(np.isnan(getattr(got, k)[30:32]).all() for k in rc.FIELDS)
    same_bits(rbd.Evaluation(*(a[keep] for a in got)), ic.emulated("hrp4"), idx[keep])


def test_refusals_the_shared_path_again_and_a_side_stream():
    (q, v), tab = rc.sample("star"), ic.rows("star")
    qd, vd, good = dev(q), dev(v), dev(tab)
    r = robot("star")
    for bad in (dev(tab[:, :24]), dev(tab[:, :, :9]), dev(tab[0]), good.float(), torch.from_numpy(np.array(tab)),
                dev(np.tile(tab, (1, 1, 2)))[:, :, ::2], np.array(tab)):
        with pytest.raises(ValueError, match="inertial"):
            r.set_inertial(bad)
        with pytest.raises(ValueError, match="inertial"):
            rbd.BatchedRobot(rc.model("star"), device=DEV, g=rc.G, inertial=bad)
    assert r.inertial is None
    r.set_inertial(good)
    with pytest.raises(ValueError, match="8 robots"):
        r.evaluate(qd[:5], vd[:5])
    # the ABI refuses a null table with a message
    assert r._lib.cmpc_rbd_eval_inertial(r._handle, 8, qd.data_ptr(), vd.data_ptr(), None, rc.G, *([None] * 7), None) != 0
    assert b"null inertial" in r._lib.cmpc_rbd_last_error()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = r.evaluate(qd, vd)
        part = r.evaluate(qd, vd, outputs=("h", "centroid"))
        none = r.evaluate(qd, vd, outputs=())
    side.synchronize()
    same_bits(host(got), ic.emulated("star"))
    assert all(t is None for t in none) and part.M is None and part.J is None
    assert ic.bits_equal(part.h.cpu().numpy(), ic.emulated("star").h) and ic.bits_equal(part.centroid.cpu().numpy(), ic.emulated("star").centroid)
    total = r.total_mass.cpu().numpy()
    assert total.shape == (8,) and all(total[b] == ic.sequential_total(tab[b]) for b in range(8))
    r.set_inertial(None)
    back = r.evaluate(qd, vd)
    torch.cuda.synchronize()
    same_bits(host(back), rc.emulated("star"))
    assert r.total_mass == rc.model("star").total_mass


def test_standing_robots_with_a_box_through_the_qp_carry_its_weight():
    """evaluate -> solve_tasks, double support: the feet carry every robot's own total; the bounds of
    tests/test_rbd_wbc_host.py."""
    masses = (0.0, 2.0, 2.5)
    q = np.tile(rc.standing(), (3, 1))
    qd, vd = dev(q), dev(np.zeros_like(q))
    r = robot("hrp4", dev(ic.payload_rows(masses)))
    ev = r.evaluate(qd, vd)
    qp = wbc.BatchedInverseDynamicsQP(foot_size=0.1, mu=0.5, device=DEV)
    sel = dev(rc.model("hrp4").joint_selection(rbd.HRP4_REDUNDANT_DOFS))
    zeros = torch.zeros((3, 51), dtype=torch.float64, device=DEV)
    ff = zeros.clone()
    ff[:, :21] = -ev.jdqd
    tau, qdd, f, st, it = qp.solve_tasks(ev.J, None, ff, zeros, zeros, None, ev.M, ev.h, dev(np.ones((3, 2))), joint_selection=sel)
    torch.cuda.synchronize()
    f, qdd, st, total = f.cpu().numpy(), qdd.cpu().numpy(), st.cpu().numpy(), r.total_mass.cpu().numpy()
    fz = f[:, 5] + f[:, 11]
    print("status", st, "sum fz - total g", fz - total * rc.G, "if the payload were ignored", fz - rc.model("hrp4").total_mass * rc.G,
          "max|qdd|", np.abs(qdd).max(axis=1))
    assert np.abs(total - (rc.model("hrp4").total_mass + np.array(masses))).max() < 1e-12
    assert (st == 0).all()
    assert (np.abs(fz - total * rc.G) < 1.0).all() and (np.abs(qdd).max(axis=1) < 0.1).all()


# ---- inside the rollout -------------------------------------------------------------------------------------------------------
def _loop(r, scene, plant):
    """A rollout (feedback on, the MPC told the scene's mass: it does not know of the payloads) of the six standing robots of
    ``mc.standing_robots`` on ``scene`` at the start tick of tests/test_gpu_walk_feedback.py, with ``r``'s walking model on
    the plant attached."""
    B, spec = mc.B_LOOP, ProblemSpec(N=mc.N_LOOP)
    t0 = mc.start_tick(scene)
    ro = BatchedRollout(scene, spec, B, device=DEV, mass=mc.loop_mass(), mu=mc.loop_mu(), feedback=True)
    qs, vs = mc.standing_robots()
    q, v = dev(qs), dev(vs)
    g, q_ref = rbd.Gait(scene, device=DEV), dev(rc.standing())
    model = r.walking_model(q, v, g, q_ref=q_ref, fall=FALL, plant=plant)
    qp = wbc.BatchedInverseDynamicsQP(foot_size=0.1, mu=0.5, device=DEV)
    foot_mu = dev(mc.loop_mu())
    ro.attach_whole_body_tasks(qp, model, mu=foot_mu)
    com, dcom = scene.nominal_state(np.full(B, t0))
    ro.reset(t0, com, dcom)
    return ro, model, q, v, dict(spec=spec, t0=t0, gait=g, q_ref=q_ref, qp=qp, foot_mu=foot_mu, com=com, dcom=dcom)


def test_closed_loop_with_payloads_equals_the_by_hand_sequence_every_tick():
    scene, B = five_scenes()[0], mc.B_LOOP
    assert B == len(LOOP_PAYLOADS)
    plant = rbd.Plant(ProblemSpec(N=mc.N_LOOP).delta, sweeps=SWEEPS)
    table = dev(ic.payload_rows(LOOP_PAYLOADS))
    r = robot("hrp4", table)
    ro, model, q, v, p = _loop(r, scene, plant)
    spec, g, q_ref, qp, foot_mu = p["spec"], p["gait"], p["q_ref"], p["qp"], p["foot_mu"]
    twin = BatchedRollout(scene, spec, B, device=DEV, mass=mc.loop_mass(), mu=mc.loop_mu())
    twin.reset(p["t0"], p["com"], p["dcom"])
    # the same rollout on a robot without a table: rows 0 and 1 carry nothing
    bare = robot("hrp4")
    ro0, model0, q0, v0, _ = _loop(bare, scene, plant)
    gl, gr = np.atleast_2d(scene.gl_tab), np.atleast_2d(scene.gr_tab)
    sel = dev(rc.model("hrp4").joint_selection(rbd.HRP4_REDUNDANT_DOFS))
    floor = dev(np.stack([np.full(B, 0.05), mc.loop_mu()], axis=1))
    imp_hand = torch.zeros((B, 24), dtype=torch.float64, device=DEV)
    eq = lambda a, b: ic.bits_equal(a.cpu().numpy(), b.cpu().numpy())
    for i in range(3):
        if i == 2:                                              # between ticks 1 and 2 robot 3 drops its box
            before = r.evaluate(q, v)
            table[3] = dev(rc.model("hrp4").inertial())
        t_tick, plan, q_in, v_in = ro.t.clone(), ro.plan_pos.clone(), q.clone(), v.clone()
        ro.step()
        ro0.step()
        ev = r.evaluate(q_in, v_in)
        r.measure(ev, twin.state, twin.alive, z_min=FALL[0], tilt_max=FALL[1])
        alive_m = twin.alive.clone()
        hx1, hu0, hstatus = twin.step()
        tt = np.minimum(t_tick.cpu().numpy(), gl.shape[1] - 1)
        flags = np.stack([gl[0, tt], gr[0, tt]], axis=1).astype(np.float64)
        desired = twin.desired_com(hx1, hu0, t_tick)
        com_des = torch.cat([desired["com_pos"], desired["com_vel"], desired["com_acc"]], dim=1).contiguous()
        refs = r.task_references(g, t_tick, None, plan, ev, com_des, q_in, v_in, q_ref)
        direct = qp.solve_tasks(ev.J, None, refs.ff, refs.pos_err, refs.vel_err, None, ev.M, ev.h, dev(flags), foot_mu, None, sel)
        hand = r.simulate(q_in, v_in, ev, direct[0], floor, plant, hold=~alive_m, impulse=imp_hand)
        torch.cuda.synchronize()
        assert eq(q, hand.q) and eq(v, hand.v) and eq(model.impulse, imp_hand), i
        assert eq(ro.state, twin.state) and eq(ro.alive, twin.alive) and eq(ro.t, twin.t), i
        assert all(eq(a, b) for a, b in zip(model.last_evaluation, ev)), i
        assert all(eq(a, b) for a, b in zip(ro.last_wbc, direct)), i
        assert eq(q[:2], q0[:2]) and eq(v[:2], v0[:2]) and eq(ro.state[:2], ro0.state[:2]), i
        assert not eq(q[2:], q0[2:]), i                          # (and the loaded robots are not the bare ones)
        print("tick", int(tt[0]), "alive", alive_m.tolist(), "qp status", direct[3].tolist(), "plant status", hand.status.tolist(),
              "sum fz", (direct[2][:, 5] + direct[2][:, 11]).tolist())
        if i == 2:
            rest = [0, 1, 2, 4, 5]
            for k in rc.FIELDS:
                a, b = getattr(ev, k), getattr(before, k)
                assert eq(a[rest], b[rest]), k
            assert not eq(ev.M[3], before.M[3]) and not eq(ev.centroid[3], before.centroid[3])
            # robot 3 is now the nominal robot at its (q, v)
            nominal = bare.evaluate(q_in, v_in)
            assert all(eq(getattr(ev, k)[3], getattr(nominal, k)[3]) for k in rc.FIELDS)

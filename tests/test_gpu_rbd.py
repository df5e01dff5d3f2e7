"""GPU tier of the batched rigid-body model (cmpc_rbd_eval, rbd_eval_kernel; one wavefront -- one workgroup -- per robot):
the launch against the independent CPU reference (tests/rbd_reference.py) at the 1e-9 level of tests/rbd_common.py, every
row bit for bit the row of a launch of that instance alone and of the emulated source, for HRP-4, the 24-joint chain and
the 24-joint star; NaN rows planted at both ends of a batch; past the resident grid (the kernel's instance loop); a side
stream; NULL outputs; evaluate -> solve_tasks on the standing HRP-4; and inside the closed-loop rollout.

Shapes: B = 1, B = 257 (a workgroup holds one robot, so there is no per-workgroup edge; 257 is odd and more than one
block), and one batch longer than the resident grid."""
import functools

import numpy as np
import pytest
import torch

import rbd_common as rc
from cmpc_amd import rbd, wbc, workloads as wl
from cmpc_amd.problem import ProblemSpec
from cmpc_amd.rollout import BatchedRollout
from scenes_common import NAMES, five_scenes, hw_for
from test_walk import measured_hw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_BIG = 257


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)              # (a writable copy: the cached instances are read-only)


@functools.lru_cache(maxsize=None)
def robot(name):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device: the HIP extension must run, there is no fallback")
    return rbd.BatchedRobot(rc.model(name), device=DEV, g=rc.G)


def launch(name, q, v, outputs=rc.FIELDS):
    out = robot(name).evaluate(dev(q), dev(v), outputs=outputs)
    torch.cuda.synchronize()
    return rbd.Evaluation(*(None if t is None else t.cpu().numpy() for t in out))


def same_bits(got, want, rows=slice(None)):
    for k in rc.FIELDS:
        g, w = getattr(got, k), np.ascontiguousarray(getattr(want, k)[rows])
        assert g.shape == w.shape and np.array_equal(np.ascontiguousarray(g).view(np.uint8), w.view(np.uint8)), k


@pytest.mark.parametrize("B", [1, B_BIG])
@pytest.mark.parametrize("name", rc.MODELS)
def test_batch_matches_the_reference_and_the_emulated_source_bit_for_bit(name, B):
    q, v = rc.sample(name, B_BIG)
    got = launch(name, q[:B], v[:B])
    want = rbd.Evaluation(*(a[:B] for a in rc.reference(name, B_BIG)))
    w = rc.worst(got, want)
    print(name, B, "error / level:", w)
    assert max(w.values()) <= 1.0, w
    same_bits(got, rc.emulated(name, B_BIG), slice(0, B))
    for b in range(B):
        assert np.array_equal(got.M[b], got.M[b].T)


@pytest.mark.parametrize("name", rc.MODELS)
def test_every_row_is_the_row_of_a_launch_of_that_instance_alone(name):
    q, v = rc.sample(name, B_BIG)
    r, qd, vd = robot(name), dev(q), dev(v)
    alone = [r.evaluate(qd[b:b + 1], vd[b:b + 1]) for b in range(B_BIG)]
    torch.cuda.synchronize()
    got = rbd.Evaluation(*(torch.cat([getattr(a, k) for a in alone]).cpu().numpy() for k in rc.FIELDS))
    same_bits(got, rc.emulated(name, B_BIG))


@pytest.mark.parametrize("name", rc.MODELS)
def test_nan_rows_at_both_ends_leave_their_neighbours_untouched(name):
    q, v = (a.copy() for a in rc.sample(name, B_BIG))
    q[0, 29], v[B_BIG - 1, 0] = np.nan, np.inf
    got, clean = launch(name, q, v), rc.emulated(name, B_BIG)
    for k in rc.FIELDS:
        a = getattr(got, k)
        assert np.isnan(a[0]).all() and np.isnan(a[B_BIG - 1]).all(), k
    same_bits(rbd.Evaluation(*(a[1:B_BIG - 1] for a in got)), clean, slice(1, B_BIG - 1))


def test_a_base_rotation_vector_whose_square_overflows_is_a_nan_row():
    q, v = (a.copy() for a in rc.sample("chain", B_BIG))
    q[100, 2] = 1e200
    got, clean = launch("chain", q, v), rc.emulated("chain", B_BIG)
    keep = np.delete(np.arange(B_BIG), 100)
    assert all(np.isnan(getattr(got, k)[100]).all() for k in rc.FIELDS)
    same_bits(rbd.Evaluation(*(a[keep] for a in got)), clean, keep)


def test_past_the_resident_grid():
    """More robots than workgroups are resident at once: the kernel's instance loop takes its second turn."""
    props = torch.cuda.get_device_properties(DEV)
    B = props.multi_processor_count * 6 + 65                  # (160 KB of LDS per CU, 23.4 KB per workgroup: six per CU)
    idx = np.arange(B) % B_BIG
    q, v = rc.sample("hrp4", B_BIG)
    same_bits(launch("hrp4", q[idx], v[idx]), rc.emulated("hrp4", B_BIG), idx)


def test_on_a_side_stream_and_with_null_outputs():
    q, v = rc.sample("star", B_BIG)
    r, qd, vd = robot("star"), dev(q), dev(v)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = r.evaluate(qd, vd)
        part = r.evaluate(qd, vd, outputs=("h", "centroid"))
        none = r.evaluate(qd, vd, outputs=())
    side.synchronize()
    same_bits(rbd.Evaluation(*(t.cpu().numpy() for t in got)), rc.emulated("star", B_BIG))
    assert all(t is None for t in none) and part.M is None and part.J is None
    assert np.array_equal(part.h.cpu().numpy(), rc.emulated("star", B_BIG).h)
    assert np.array_equal(part.centroid.cpu().numpy(), rc.emulated("star", B_BIG).centroid)


def test_bad_arguments_are_refused():
    r = robot("hrp4")
    q, v = (dev(a[:2]) for a in rc.sample("hrp4"))
    with pytest.raises(ValueError):
        r.evaluate(q, v[:, :29].contiguous())
    with pytest.raises(ValueError):
        r.evaluate(q.float(), v)
    with pytest.raises(ValueError):
        r.evaluate(q, v, outputs=("J", "nope"))
    bad = rc.model("hrp4")
    tables = [a.copy() for a in bad.tables()]
    tables[0][4] = 9                                          # the native validation, in front of the device tables
    import ctypes
    h = ctypes.c_void_p()
    assert r._lib.cmpc_rbd_model_create(0, *(a.ctypes.data for a in tables), ctypes.byref(h)) != 0 and not h
    assert b"parent" in r._lib.cmpc_rbd_last_error()


def _standing(B):
    q = np.tile(rc.standing(), (B, 1))
    return q, np.zeros_like(q)


def test_standing_hrp4_through_the_qp_shares_the_weight_between_the_feet():
    """q, qd -> torques in two launches, on the robot's own matrices; the bounds of tests/test_rbd_wbc_host.py."""
    q, v = (dev(a) for a in _standing(3))
    ev = robot("hrp4").evaluate(q, v)
    qp = wbc.BatchedInverseDynamicsQP(foot_size=0.1, mu=0.5, device=DEV)
    sel = dev(rc.model("hrp4").joint_selection(rbd.HRP4_REDUNDANT_DOFS))
    zeros = torch.zeros((3, 51), dtype=torch.float64, device=DEV)
    ff = zeros.clone()
    ff[:, :21] = -ev.jdqd
    contact = dev([[1.0, 1.0], [1.0, 0.0], [0.0, 1.0]])
    tau, qdd, f, st, it = qp.solve_tasks(ev.J, None, ff, zeros, zeros, None, ev.M, ev.h, contact, joint_selection=sel)
    torch.cuda.synchronize()
    f, qdd, st = f.cpu().numpy(), qdd.cpu().numpy(), st.cpu().numpy()
    mg = rc.model("hrp4").total_mass * rc.G
    print("status", st, "iters", it.cpu().numpy(), "fz", f[0, 5], f[0, 11], "sum - mg", f[0, 5] + f[0, 11] - mg, "max|qdd|", np.abs(qdd[0]).max())
    assert (st == 0).all()
    assert abs(f[0, 5] + f[0, 11] - mg) < 1.0 and abs(f[0, 5] - f[0, 11]) < 0.1 and np.abs(qdd[0]).max() < 0.1
    assert tau.shape == (3, 24)


def _rollout_case(scene, B, ticks, sid=None, hw=None):
    spec = ProblemSpec(N=10)
    mu = np.array([0.3, 0.3, 0.5, 0.5, 0.9, 0.9])[:B]
    rng = np.random.default_rng(9)
    ro = BatchedRollout(scene, spec, B, device=DEV, mu=mu, hw_measured=hw, hw_offset=rng.normal(0, 0.05, size=(B, 3)), scene_id=sid,
                        gains=True)
    q0, v0 = _standing(B)
    q0[:, 22:30] += rng.uniform(-0.05, 0.05, size=(B, 8))     # every robot its own arms
    q, v = dev(q0), dev(v0)
    r = robot("hrp4")
    model = r.task_model(q, v)
    qp = wbc.BatchedInverseDynamicsQP(foot_size=0.1, mu=0.5, device=DEV)
    ro.attach_whole_body_tasks(qp, model)
    t0 = 255
    s = np.zeros(B, np.int32) if sid is None else sid
    com, dcom = (scene.nominal_state(np.full(B, t0)) if sid is None else scene.nominal_state(np.full(B, t0), sid))
    ro.reset(t0, com + rng.uniform(-0.003, 0.003, size=(B, 3)), dcom)
    gl, gr = np.atleast_2d(scene.gl_tab), np.atleast_2d(scene.gr_tab)
    sel = dev(rc.model("hrp4").joint_selection(rbd.HRP4_REDUNDANT_DOFS))
    for i in range(ticks):
        t_tick = ro.t.clone()
        x1, u0, _ = ro.step()
        got = [t.clone() for t in ro.last_wbc]
        # the same tick by hand: evaluate, the CoM rows from the MPC's desired, solve_tasks with this tick's flags and mu
        flags = np.stack([gl[s, t0 + i], gr[s, t0 + i]], axis=1).astype(np.float64)
        desired = ro.desired_com(x1, u0, t_tick)
        ev = r.evaluate(q, v)
        ff = torch.zeros((B, 51), dtype=torch.float64, device=DEV)
        pe, ve = torch.zeros_like(ff), torch.zeros_like(ff)
        ff[:, :21] = -ev.jdqd
        ff[:, 12:15] += desired["com_acc"]
        pe[:, 12:15] = desired["com_pos"] - ev.pose[:, 12:15]
        ve[:, 12:15] = desired["com_vel"] - ev.vel[:, 12:15]
        direct = qp.solve_tasks(ev.J, None, ff, pe, ve, None, ev.M, ev.h, dev(flags), dev(mu), None, sel)
        torch.cuda.synchronize()
        for g, d, name in zip(got, direct, ("tau", "qdd", "f", "status", "iters")):
            assert g.dtype == d.dtype and torch.equal(g, d), (name, i)
        same_bits(rbd.Evaluation(*(t.cpu().numpy() for t in model.last_evaluation)), rbd.Evaluation(*(t.cpu().numpy() for t in ev)))
        assert got[0].shape == (B, 24) and got[3].shape == (B,)
        # the measured centroidal state, padded to the 20 columns of x0, through the gain of the tick
        x_meas = torch.cat([ev.centroid, ro.last_records[:, 9:20]], dim=1).contiguous()
        y1, w0, used = ro.track(x_meas, columns=0x1FF)
        torch.cuda.synchronize()
        assert y1.shape == (B, 20) and torch.isfinite(y1).all() and torch.isfinite(w0).all()
        q[:, 25] += 0.01                                       # the caller moves the robots in place between ticks
        v[:, 25] = 0.1


def test_rollout_of_a_single_scene_runs_the_robot_every_tick():
    _rollout_case(five_scenes()[0], 6, 3, hw=measured_hw())


def test_rollout_of_a_fleet_runs_the_robot_every_tick():
    scs, hwm = five_scenes(), measured_hw()
    pick = (NAMES.index("shipped"), NAMES.index("lfirst"))
    sset = wl.SceneSet([scs[k] for k in pick])
    _rollout_case(sset, 6, 3, sid=np.array([0, 1, 0, 1, 0, 1], np.int32), hw=[hw_for(NAMES[k], hwm) for k in pick])

"""Scene sets on the GPU: closed-loop batches in which every robot walks its own command.  The record builder with a
scene index (``cmpc_build_records_scenes``) against the single-scene kernel and the host builder, its refusals on the
device, the fused back half of the tick (``cmpc_rollout_advance``) against the torch path it replaces, a mixed fleet
against per-scene rollouts, the nominal fleet of all five walks, and per-instance constants in the loop.  All comparisons
are bit for bit: the new kernels copy, and add once."""
import ctypes

import numpy as np
import pytest
import torch

from cmpc_amd import capi, workloads as wl
from cmpc_amd.footstep_planner_vertices import FootstepPlanner
from cmpc_amd.problem import ProblemSpec, build_record, to_cspec
from cmpc_amd.rollout import BatchedRollout
from cmpc_amd.solver import DeviceRecordBuilder
from scenes_common import NAMES, WALKS, five_scenes, hw_for, scene_set, walk_params
from test_walk import measured_hw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 10


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device: the HIP extension must run, there is no fallback")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(x):
    """Host copy for bit-for-bit comparison (NaN rows of a refused solve included)."""
    x = x.detach().cpu().contiguous()
    return x.view(torch.int64).numpy() if x.dtype == torch.float64 else x.numpy()


@pytest.fixture(scope="module")
def mixed_batch(gpu):
    """B = 257 instances over the five scenes: random ticks (the edge ticks of the plan lookup and every scene's last valid
    tick included), random states, per-instance plans perturbed by 1e-3; the records of the set builder, computed once."""
    scs, ss = five_scenes(), scene_set()
    rng = np.random.default_rng(41)
    B = 257
    sid = rng.integers(0, 5, size=B).astype(np.int32)
    sid[:10] = np.repeat(np.arange(5), 2)
    t = np.array([rng.integers(0, scs[s].t_max(N) + 1) for s in sid], dtype=np.int32)
    t[0:10:2] = [scs[s].t_max(N) for s in range(5)]
    t[10:14] = [199, 200, 269, 270]
    state = rng.normal(size=(B, 16))
    plans = ss.plan_pos[sid] + rng.normal(scale=1e-3, size=(B, ss.n_steps_max, 3))      # (padding stays NaN)
    bld = DeviceRecordBuilder(ss, device=DEV)
    spec = ProblemSpec(N=N)
    got = bld.build(spec, dev(t), dev(state), plan_pos=dev(plans), scene_id=dev(sid)).cpu().numpy()
    return dict(spec=spec, B=B, sid=sid, t=t, state=state, plans=plans, bld=bld, got=got)


def test_set_builder_equals_the_single_scene_kernel_and_the_host_builder(mixed_batch):
    mb, scs = mixed_batch, five_scenes()
    spec, sid, t, state, plans, got = (mb[k] for k in ("spec", "sid", "t", "state", "plans", "got"))
    assert not np.isnan(got).any()                                    # no padding row or plan entry was read
    for s, sc in enumerate(scs):
        m = np.nonzero(sid == s)[0]
        n = sc.plan_pos.shape[0]
        one = DeviceRecordBuilder(sc, device=DEV)
        want = one.build(spec, dev(t[m]), dev(state[m]), plan_pos=dev(plans[m, :n])).cpu().numpy()
        assert np.array_equal(got[m], want), NAMES[s]
    for b in range(0, mb["B"], 8):
        sc, name = scs[sid[b]], NAMES[sid[b]]
        planner = FootstepPlanner(sc.vref, wl.LFOOT0, wl.RFOOT0, walk_params(name))
        for i, p in enumerate(planner.plan):
            p['pos'] = plans[b, i].copy()
        x = state[b]
        want = build_record(spec, planner, sc.com_ref, int(t[b]), x[0:3], x[3:6], x[6:9], x[9:12], x[12], x[13], x[14], x[15],
                            first_swing=WALKS[name][1], contacts_ref=sc.planner.position_contacts_ref)
        assert np.array_equal(got[b], want), (b, name)


def test_set_of_one_scene_equals_the_existing_builder(gpu, scene):
    rng = np.random.default_rng(42)
    spec, B = ProblemSpec(N=N), 257
    t = rng.integers(0, scene.t_max(N) + 1, size=B).astype(np.int32)
    t[:5] = [199, 200, 269, 270, scene.t_max(N)]
    state = rng.normal(size=(B, 16))
    plans = np.repeat(scene.plan_pos[None], B, axis=0) + rng.normal(scale=1e-3, size=(B,) + scene.plan_pos.shape)
    want = DeviceRecordBuilder(scene, device=DEV).build(spec, dev(t), dev(state), plan_pos=dev(plans)).cpu().numpy()
    bld = DeviceRecordBuilder(wl.SceneSet([scene]), device=DEV)
    got = bld.build(spec, dev(t), dev(state), plan_pos=dev(plans), scene_id=torch.zeros(B, dtype=torch.int32, device=DEV))
    assert np.array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError, match="scene_id"):
        bld.build(spec, dev(t), dev(state), plan_pos=dev(plans))
    with pytest.raises(ValueError, match="scene_id"):
        DeviceRecordBuilder(scene, device=DEV).build(spec, dev(t), dev(state), scene_id=torch.zeros(B, dtype=torch.int32, device=DEV))


def test_set_builder_refuses_on_the_device(mixed_batch):
    """scene_id = -1, scene_id = S, the first tick past a short scene's own end (valid for the longest scene) and a negative
    tick: an all-NaN record each, every other record as before."""
    mb, ss = mixed_batch, scene_set()
    sid, t = mb["sid"].copy(), mb["t"].copy()
    short = int(np.nonzero(mb["sid"] == NAMES.index("lateral"))[0][-1])
    refused = [20, 21, short, 23]
    assert short not in (20, 21, 23)
    sid[20], sid[21] = -1, ss.S
    t[short] = ss.T[sid[short]] - (N + 1)
    assert t[short] + (N + 1) < ss.T.max() and t[short] == five_scenes()[sid[short]].t_max(N) + 1
    t[23] = -1
    got = mb["bld"].build(mb["spec"], dev(t), dev(mb["state"]), plan_pos=dev(mb["plans"]), scene_id=dev(sid)).cpu().numpy()
    assert np.isnan(got[refused]).all()
    keep = np.setdiff1d(np.arange(mb["B"]), refused)
    assert np.array_equal(got[keep], mb["got"][keep])


def test_c_entry_points_refuse_bad_arguments(gpu):
    lib, ss = capi.load(), scene_set()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    err = lambda: lib.cmpc_last_error(None).decode()
    T = np.ascontiguousarray(ss.T, dtype=np.int32)
    tabs = [np.ascontiguousarray(a, dtype=np.float64) for a in (ss.com_tab, ss.pose_l, ss.pose_r, ss.gl_tab, ss.gr_tab, ss.cur_l, ss.cur_r)]
    sl, sr = (np.ascontiguousarray(a, dtype=np.int32) for a in (ss.slot_l, ss.slot_r))
    h = ctypes.c_void_p()
    assert lib.cmpc_scenes_create(0, 0, ss.T_max, p(T), *[p(a) for a in tabs], ss.n_steps_max, p(sl), p(sr), ctypes.byref(h)) != 0
    assert "S must be at least 1" in err()
    assert lib.cmpc_scenes_create(0, ss.S, ss.T_max, p(T), *[p(a) for a in tabs], 0, p(sl), p(sr), ctypes.byref(h)) != 0
    assert "n_steps_max" in err()
    assert lib.cmpc_scenes_create(0, ss.S, ss.T_max, p(T), None, *[p(a) for a in tabs[1:]], ss.n_steps_max, p(sl), p(sr), ctypes.byref(h)) != 0
    assert "null table" in err()
    assert lib.cmpc_tables_create(0, 0, *[p(a) for a in tabs], ctypes.byref(h)) != 0 and err() == "cmpc_tables_create: bad argument"
    assert lib.cmpc_scenes_create(0, ss.S, ss.T_max, p(T), *[p(a) for a in tabs], ss.n_steps_max, p(sl), p(sr), ctypes.byref(h)) == 0
    try:
        B = 4
        z32 = torch.zeros(B, dtype=torch.int32, device=DEV)
        st, rec = torch.zeros((B, 16), dtype=torch.float64, device=DEV), torch.zeros((B, 24 + 19 * N), dtype=torch.float64, device=DEV)
        assert lib.cmpc_build_records_scenes(h, N, 1, B, z32.data_ptr(), None, st.data_ptr(), None, rec.data_ptr(), None) != 0
        assert "null buffer" in err()
        # the single-scene entry point does not serve a set of five
        assert lib.cmpc_build_records_planned(h, N, 1, B, z32.data_ptr(), st.data_ptr(), None, rec.data_ptr(), None) != 0
        assert "several scenes" in err()
        spec = ProblemSpec(N=N)
        XU, warm = (torch.zeros((B, spec.nsol), dtype=torch.float64, device=DEV) for _ in range(2))
        u8 = [torch.zeros(B, dtype=torch.uint8, device=DEV) for _ in range(3)]
        plan = torch.zeros((B, ss.n_steps_max, 3), dtype=torch.float64, device=DEV)
        adv = lambda xu, w: lib.cmpc_rollout_advance(h, N, spec.nv, 1, B, z32.data_ptr(), xu, z32.data_ptr(), None, None, 1, 0,
                                                      z32.data_ptr(), st.data_ptr(), *[u.data_ptr() for u in u8], plan.data_ptr(), w, None)
        assert adv(XU.data_ptr(), warm.data_ptr()) != 0 and "schedule" in err()          # no schedule yet
        sched = ss.schedule(N, 1)
        arrs = [np.ascontiguousarray(sched[0], dtype=np.uint8), np.ascontiguousarray(sched[1], dtype=np.uint8),
                np.ascontiguousarray(sched[2], dtype=np.int32), np.ascontiguousarray(sched[3], dtype=np.int32)]
        assert lib.cmpc_scenes_set_schedule(h, N, 1, p(arrs[0]), p(arrs[1]), None, p(arrs[3])) != 0 and "null buffer" in err()
        assert lib.cmpc_scenes_set_schedule(h, N, 1, *[p(a) for a in arrs]) == 0
        assert adv(None, warm.data_ptr()) != 0 and "null buffer" in err()
        assert adv(XU.data_ptr(), XU.data_ptr()) != 0 and "overlaps" in err()
    finally:
        lib.cmpc_tables_destroy(h)


STATE_KEYS = ("state", "t", "alive", "flag", "counter", "plan_pos", "warm")


def test_fused_back_half_equals_the_torch_path_tick_by_tick(gpu, scene):
    """A set of one scene (the shipped walk) against today's rollout after every one of 75 ticks from t0 = 240: through the
    write-back (261) and the touch-down (270), with a velocity push on ticks 10-12, and with a sixth instance started at
    t0 = 255 with zero momentum -- the certified-infeasible late-single-support corner, which ends
    status 2 on its first tick and stops for good on both sides."""
    hwm, spec = measured_hw(), ProblemSpec(N=N)
    B, ticks = 6, 75
    t0 = np.array([240] * 5 + [255])
    rng = np.random.default_rng(21)
    com, dcom = scene.nominal_state(t0)
    com = com + rng.uniform(-0.004, 0.004, size=(B, 3))
    off = rng.normal(0, 0.05, size=(B, 3))
    com[5] = scene.nominal_state(t0[5:])[0][0]                      # the corner is x0 on the reference, hw = 0
    hw0 = hwm[t0] + off
    hw0[5] = 0.0
    a = BatchedRollout(scene, spec, B, device=DEV, hw_measured=hwm, hw_offset=off)
    b = BatchedRollout(wl.SceneSet([scene]), spec, B, device=DEV, hw_measured=hwm, hw_offset=off)
    for ro in (a, b):
        ro.reset(t0, com, dcom, hw=hw0)
    push = np.array([0.01, -0.006, 0.0])
    for i in range(ticks):
        dv = push if 10 <= i <= 12 else None
        _, _, sa = a.step(dv)
        _, _, sb = b.step(dv)
        assert np.array_equal(sa.cpu().numpy(), sb.cpu().numpy()), i
        if i == 0:
            assert int(sa[5]) == 2, sa.tolist()
        for k in STATE_KEYS:
            assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), (i, k)
        assert not bool(b.alive[5])
    assert b.alive.dtype == torch.bool and b.alive[:5].all().item() and int(b.t[5]) == 255
    assert (b.t[:5] == 240 + ticks).all().item()
    assert not np.array_equal(b.plan_pos[:5].cpu().numpy(), np.repeat(scene.plan_pos[None], 5, axis=0))   # the write-back fired


def test_set_rollout_without_plan_write_back_equals_the_torch_path(gpu, scene):
    """update_contact=False on a set of one scene against today's rollout in that mode: the nominal plan is kept, flag and
    counter are left alone, everything else advances as before -- after every one of 40 ticks through t = 261 and 270."""
    hwm, spec = measured_hw(), ProblemSpec(N=N)
    B, t0 = 4, 240
    rng = np.random.default_rng(25)
    com, dcom = scene.nominal_state(np.full(B, t0))
    com = com + rng.uniform(-0.004, 0.004, size=(B, 3))
    off = rng.normal(0, 0.05, size=(B, 3))
    a = BatchedRollout(scene, spec, B, device=DEV, hw_measured=hwm, hw_offset=off, update_contact=False)
    b = BatchedRollout(wl.SceneSet([scene]), spec, B, device=DEV, hw_measured=hwm, hw_offset=off, update_contact=False)
    for ro in (a, b):
        ro.reset(t0, com, dcom)
    for i in range(40):
        a.step()
        b.step()
        for k in STATE_KEYS:
            assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), (i, k)
    assert b.alive.all().item() and not b.counter.any().item() and not b.flag.any().item()
    assert np.array_equal(b.plan_pos.cpu().numpy(), np.repeat(scene.plan_pos[None], B, axis=0))
    # the C contract: without the write-back the three buffers may be absent
    XU, status = b.last_XU, b.last_status
    t_before = b.t.clone()
    b.builder.advance(spec, 1, b.scene_id, XU, status, b.t, b.state, b.alive, b._warm_buf, update_contact=False)
    assert np.array_equal((b.t - t_before).cpu().numpy(), np.ones(B, np.int32))


def run_fleet(ro, ticks):
    fired = np.zeros((ticks, ro.B), bool)
    hist = [ro.state[:, 0:3].clone()]
    for i in range(ticks):
        ro.step()
        fired[i] = ro.counter.cpu().numpy()
        hist.append(ro.state[:, 0:3].clone())
    return fired, torch.stack(hist).cpu().numpy()


def test_mixed_fleet_equals_per_scene_rollouts(gpu):
    """Two instances per walk in one batch against the same instances in today's single-scene rollout of their own scene."""
    scs, ss, hwm, spec = five_scenes(), scene_set(), measured_hw(), ProblemSpec(N=N)
    B, t0, ticks = 10, 240, 75
    sid = np.repeat(np.arange(5), 2).astype(np.int32)
    rng = np.random.default_rng(23)
    com, dcom = ss.nominal_state(np.full(B, t0), sid)
    com = com + rng.uniform(-0.004, 0.004, size=(B, 3))
    off = rng.normal(0, 0.05, size=(B, 3))
    fleet = BatchedRollout(ss, spec, B, device=DEV, scene_id=sid, hw_measured=[hw_for(n, hwm) for n in NAMES], hw_offset=off)
    fleet.reset(t0, com, dcom)
    fired, _ = run_fleet(fleet, ticks)
    assert fleet.alive.all().item() and fired.any(axis=0).all()
    state, plan = fleet.state.cpu().numpy(), fleet.plan_pos.cpu().numpy()
    for s, (name, sc) in enumerate(zip(NAMES, scs)):
        m = np.nonzero(sid == s)[0]
        one = BatchedRollout(sc, spec, len(m), device=DEV, hw_measured=hw_for(name, hwm), hw_offset=off[m])
        one.reset(t0, com[m], dcom[m])
        fired_one, _ = run_fleet(one, ticks)
        n = sc.plan_pos.shape[0]
        assert np.array_equal(state[m], one.state.cpu().numpy()), name
        assert np.array_equal(plan[m, :n], one.plan_pos.cpu().numpy()) and np.isnan(plan[m, n:]).all(), name
        assert np.array_equal(fired[:, m], fired_one), name
        assert not np.array_equal(plan[m[0], :n], sc.plan_pos), name


def test_nominal_fleet_of_all_five_walks(gpu):
    """One unperturbed instance per walk from t = 0 for 380 ticks: all alive, write-backs at t = 261 and 361 each, the CoM
    within 3 cm (x, y) and 1 cm (z) of its own scene's reference (the bounds of test_walk.check_walk_log).  The C oracle
    walks all five for 480 ticks in the CPU-tier harness."""
    scs, ss, hwm, spec = five_scenes(), scene_set(), measured_hw(), ProblemSpec(N=N)
    B, ticks = 5, 380
    sid = np.arange(5, dtype=np.int32)
    fleet = BatchedRollout(ss, spec, B, device=DEV, scene_id=sid, hw_measured=[hw_for(n, hwm) for n in NAMES])
    com, dcom = ss.nominal_state(np.zeros(B, int), sid)
    fleet.reset(0, com, dcom)
    fired = np.zeros((ticks, B), bool)
    com_hist, status_hist = [], []
    for i in range(ticks):
        x1, _, status = fleet.step()
        fired[i] = fleet.counter.cpu().numpy()
        com_hist.append(x1[:, 0:3].cpu().numpy())
        status_hist.append(status.cpu().numpy())
    status_hist, com_hist = np.array(status_hist), np.array(com_hist)
    lost = []
    for s in range(B):
        bad = np.nonzero(~np.isin(status_hist[:, s], (0, 3)))[0]
        if bad.size:
            lost.append((NAMES[s], int(bad[0]), int(status_hist[bad[0], s])))
    print("nominal fleet: (walk, first lost tick, status):", lost)
    assert not lost and fleet.alive.all().item()
    for s, sc in enumerate(scs):
        assert np.nonzero(fired[:, s])[0].tolist() == [261, 361], NAMES[s]
        err = np.abs(com_hist[:, s] - sc.com_tab[1:ticks + 1, 0:3])            # x_1 of tick t against the reference at t + 1
        print(f"nominal fleet {NAMES[s]}: max |CoM - ref| = {err.max(axis=0)}")
        assert err[:, 0].max() < 0.03 and err[:, 1].max() < 0.03 and err[:, 2].max() < 0.01, NAMES[s]


def consts_rollout(scene_or_set, spec, B, t0, com, dcom, off, ticks, consts=None):
    ro = BatchedRollout(scene_or_set, spec, B, device=DEV, hw_measured=measured_hw(), hw_offset=off, consts=consts)
    ro.reset(t0, com, dcom)
    fired, _ = run_fleet(ro, ticks)
    return ro, fired


def test_per_instance_constants_in_the_loop(gpu, scene):
    params = wl.default_params(N=N)
    nominal, payload = ProblemSpec.from_params(params), ProblemSpec.from_params(params, payload=True)
    assert (payload.k1, payload.k2) == (7.0, 1.0) and payload.delta == nominal.delta
    B, t0, ticks = 8, 240, 60
    rng = np.random.default_rng(24)
    com, dcom = scene.nominal_state(np.full(B, t0))
    com = com + rng.uniform(-0.004, 0.004, size=(B, 3))
    off = rng.normal(0, 0.05, size=(B, 3))
    args = (B, t0, com, dcom, off, ticks)
    row = np.zeros(18)
    capi.load().cmpc_spec_consts(ctypes.byref(to_cspec(nominal)), row.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert np.array_equal(row, nominal.consts_row())
    plain, fired_plain = consts_rollout(scene, nominal, *args)
    assert plain.alive.all().item() and fired_plain.any(axis=0).all()
    # eight copies of the spec's own row: the rollout without consts, through a consts kernel (one Scene, the torch back half)
    same, fired_same = consts_rollout(scene, nominal, *args, consts=np.repeat(row[None], B, axis=0))
    assert "consts" in same.solver.last_kernel_name() and "consts" not in plain.solver.last_kernel_name()
    for k in STATE_KEYS:
        assert np.array_equal(bits(getattr(same, k)), bits(getattr(plain, k))), k
    assert np.array_equal(fired_same, fired_plain)
    # four nominal and four payload rows (a scene set, the fused back half) against the two homogeneous rollouts
    heavy, fired_heavy = consts_rollout(scene, payload, *args)
    rows = np.stack([nominal.consts_row()] * 4 + [payload.consts_row()] * 4)
    mixed, fired_mixed = consts_rollout(wl.SceneSet([scene]), nominal, *args, consts=rows)
    assert "consts" in mixed.solver.last_kernel_name()
    for k in ("state", "plan_pos", "warm", "alive", "t"):
        got = bits(getattr(mixed, k))
        assert np.array_equal(got[:4], bits(getattr(plain, k))[:4]) and np.array_equal(got[4:], bits(getattr(heavy, k))[4:]), k
    assert np.array_equal(fired_mixed[:, :4], fired_plain[:, :4]) and np.array_equal(fired_mixed[:, 4:], fired_heavy[:, 4:])
    assert not np.array_equal(bits(plain.state)[4:], bits(heavy.state)[4:])       # the gains do change the walk
    rows[5, 0] = 2 * nominal.delta
    with pytest.raises(ValueError, match="delta"):
        BatchedRollout(scene, nominal, B, device=DEV, consts=rows)

"""Scene sets on the CPU tier: ``workloads.Scene(vref=...)``, ``workloads.SceneSet`` (stacked tables, the numpy record
builder, the write-back schedule), two non-shipped walks in closed loop through the drop-in class with the C oracle
standing in for the HIP solver, and the host-side refusal of per-instance constants with a foreign delta."""
import numpy as np
import pytest

from cmpc_amd import workloads as wl
from cmpc_amd.foot_trajectory_generator import FootTrajectoryGenerator
from cmpc_amd.footstep_planner_vertices import FootstepPlanner
from cmpc_amd.problem import ProblemSpec
from cmpc_amd.walk import WalkHarness
from scenes_common import NAMES, WALKS, five_scenes, hw_for, scene_set, walk_params
from test_walk import make_oracle_backed, measured_hw

TABLES = ('com_tab', 'pose_l', 'pose_r', 'gl_tab', 'gr_tab', 'cur_l', 'cur_r', 'slot_l', 'slot_r', 'plan_pos', 'is_ss',
          'step_idx', 'support_is_l')


def test_default_vref_reproduces_the_shipped_scene_and_the_five_walks_have_their_lengths(scene):
    for sc in (wl.Scene(vref=None), wl.Scene(vref=wl.VREF)):
        assert sc.T == scene.T
        for k in TABLES:
            a, b = np.asarray(getattr(sc, k)), np.asarray(getattr(scene, k))
            assert a.dtype == b.dtype and np.array_equal(a, b), k
    assert wl.scene() is scene
    for name, sc in zip(NAMES, five_scenes()):
        assert (sc.T, sc.plan_pos.shape[0]) == WALKS[name][2:], name
    turn = five_scenes()[NAMES.index("turn")]
    assert 1.4 < np.abs(turn.pose_l[:turn.T, 0:3]).max() <= 1.5 + 1e-9          # the turning walk does turn (yaw up to 1.5 rad)


def test_scene_set_stacks_and_pads():
    scs, ss = five_scenes(), scene_set()
    assert ss.S == 5 and ss.T.tolist() == [WALKS[n][2] for n in NAMES] and ss.T_max == 1971 and ss.n_steps_max == 20
    for s, sc in enumerate(scs):
        for k in TABLES:
            full, own = getattr(ss, k)[s], np.asarray(getattr(sc, k))
            n = sc.plan_pos.shape[0] if k == 'plan_pos' else sc.T
            assert np.array_equal(full[:n], own[:n]), (s, k)
            pad = full[n:]
            if full.dtype == np.float64:
                assert np.isnan(pad).all(), (s, k)
            elif full.dtype == bool:
                assert not pad.any(), (s, k)
            else:
                assert (pad == -1).all(), (s, k)
    p = wl.default_params(); p['mpc_rate'] = 10
    with pytest.raises(ValueError, match="mpc_rate"):
        wl.SceneSet([scs[0], wl.Scene(p)])
    with pytest.raises(ValueError):
        wl.SceneSet([])


def test_scene_set_records_equal_each_scenes_own_bit_for_bit():
    scs, ss = five_scenes(), scene_set()
    spec, B = ProblemSpec(N=10), 64
    rng = np.random.default_rng(31)
    sid = rng.integers(0, 5, size=B)
    sid[:10] = np.repeat(np.arange(5), 2)                                        # every scene, at its edge ticks
    t = np.array([rng.integers(0, scs[s].t_max(10) + 1) for s in sid])
    t[0:10:2] = [scs[s].t_max(10) for s in range(5)]
    t[10:14] = [199, 200, 269, 270]
    x = rng.normal(size=(B, 16))
    args = lambda m: (x[m, 0:3], x[m, 3:6], x[m, 6:9], x[m, 9:12], x[m, 12], x[m, 13], x[m, 14], x[m, 15])
    got = ss.build_records(spec, t, sid, *args(slice(None)))
    assert got.shape == (B, spec.nrec) and not np.isnan(got).any()               # no padding in a valid tick's record
    for s, sc in enumerate(scs):
        m = sid == s
        assert m.any() and np.array_equal(got[m], sc.build_records(spec, t[m], *args(m))), s
    # a tick that is valid for the longest scene only, and a scene index out of range
    with pytest.raises(ValueError, match="tick outside"):
        ss.build_records(spec, np.array([scs[2].t_max(10) + 1]), np.array([2]), *args(slice(0, 1)))
    with pytest.raises(ValueError, match="scene_id"):
        ss.build_records(spec, np.array([0]), np.array([5]), *args(slice(0, 1)))


def test_schedule_of_a_set_is_every_scenes_own():
    """What ``BatchedRollout.__init__`` computed for its one scene before the helper was lifted out, restated."""
    N, rate = 10, 1
    sched = scene_set().schedule(N, rate)
    assert all(a.shape == (5, 1971) for a in sched)
    for s, sc in enumerate(five_scenes()):
        T = sc.T
        end = np.minimum(np.arange(T) + N * rate - 1, T - 1)
        want = (sc.is_ss & ~sc.is_ss[end], ~sc.is_ss,
                np.minimum(sc.step_idx + 1, sc.plan_pos.shape[0] - 1).astype(np.int64),
                np.where(sc.support_is_l, 17, 13).astype(np.int64))
        for got, w, h in zip(sched, want, wl.rollout_schedule(sc, N, rate)):
            assert np.array_equal(got[s, :T], w) and np.array_equal(h, w), s
        assert sched[0][s, 261] and not sched[0][s, 260]                        # the write-back tick of the first step
    # the left-first walk lands its left foot first: rows 13:16 of x_N, where the others take 17:20
    assert sched[3][NAMES.index("lfirst"), 261] == 13 and sched[3][0, 261] == 17


@pytest.mark.parametrize("name", ["turn", "lfirst"])
def test_closed_loop_of_a_non_shipped_walk(oracle, name):
    """The closed loop of tests/test_walk.py on another command: 300 ticks, N = 10, the oracle-backed drop-in class; the
    left-first walk with the mirrored momentum recording.  Every tick is usable and the write-back fires at t = 261."""
    sc = five_scenes()[NAMES.index(name)]
    params = walk_params(name)
    planner = FootstepPlanner(sc.vref, wl.LFOOT0, wl.RFOOT0, params)            # a fresh plan: the MPC rewrites it
    ftg = FootTrajectoryGenerator(sc.initial, planner, params)
    mpc = make_oracle_backed(oracle)(sc.initial, planner, params, sc.com_ref, None, None)
    nominal = [p['pos'].copy() for p in planner.plan]
    log = WalkHarness(mpc, planner, ftg, params, sc.initial, hw_measured=hw_for(name, measured_hw())).run(300)
    assert np.isin(log['status'], (0, 3)).all(), log['t'][~np.isin(log['status'], (0, 3))]
    assert log['t'][log['counter'] == 1].tolist() == [261]
    idx = planner.get_step_index_at_time(261)
    assert np.array_equal(planner.plan[idx + 1]['pos'], log['mpc_new_contact'][261])
    assert not np.array_equal(planner.plan[idx + 1]['pos'], nominal[idx + 1])


def test_rollout_refuses_constants_with_a_foreign_delta_before_touching_the_device(scene):
    """Checked on the host at construction: the schedule advances by `rate` ticks for the whole batch."""
    from cmpc_amd.rollout import BatchedRollout
    spec = ProblemSpec(N=10)
    rows = np.repeat(spec.consts_row()[None], 4, axis=0)
    rows[2, 0] = 2 * spec.delta
    with pytest.raises(ValueError, match="delta"):
        BatchedRollout(scene, spec, 4, consts=rows)
    with pytest.raises(ValueError, match="shape"):
        BatchedRollout(scene, spec, 4, consts=rows[:3])

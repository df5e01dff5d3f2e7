"""CPU tier of the contact plant (cmpc_walk_plant_step of include/cmpc_walk.h) on the emulated device source
(tests/emu/walk_plant_emu.cpp): the step against a dense numpy restatement, the standing robot that must stay still, free
flight, a push, a landing, sliding on the cone, the rows that must not move, NULL arguments, every refusal, the argument
checks of ``rbd.Plant`` and the call path of ``walking_model`` with and without a plant, and the stand-alone program under
the sanitizers.  Whether HRP-4 stays upright on this plant is not asserted anywhere."""
import os
import subprocess

import numpy as np
import pytest

import rbd_common as rc
import rbd_walk_common as wc
import walk_plant_common as pc
from cmpc_amd import rbd

#: largest relative difference of v_out, q_out and impulse between the emulated source and the restatement on the 16-robot
#: mix at 20 sweeps, measured on the CPU: 5.2e-15 (v_out 8.3e-16, q_out 5.0e-16, impulse 5.2e-15).  100 x that is far below
#: 1e-7, the loosest the level may be, and the level is 100 x the measurement.
RESTATEMENT_MEASURED = 5.2e-15
RESTATEMENT_LEVEL = min(100 * RESTATEMENT_MEASURED, 1e-7)
SWEEPS_MIX = 20


def rel(got, want):
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------
def test_the_step_is_the_dense_numpy_restatement():
    case = pc.mix_case()
    got = pc.emulate_plant(case, pc.params(sweeps=SWEEPS_MIX))
    want, margins = pc.restate(case, SWEEPS_MIX)
    # no draw sits on a tie of the sweeps' branches (a draw that did would be replaced, not the level widened)
    assert margins.min() > 1e-9, margins
    assert (got.status == 0).all()
    phi = np.array([pc.contact_rows(case["J"][b], case["pose"][b], pc.HALF)[1].min() for b in range(16)])
    assert (np.abs(phi[:8]) <= 0.01 + 1e-12).all() and (phi[12:] >= 1.0 - 1e-12).all()
    touching = (got.impulse.reshape(16, 8, 3)[:, :, 2] > 0).any(axis=1)
    assert touching[:12].sum() >= 6 and not touching[12:].any()
    err = {k: rel(getattr(got, k), getattr(want, k)) for k in ("v", "q", "impulse")}
    print("largest relative difference:", err, "residual", rel(got.residual, want.residual))
    assert max(err.values()) <= RESTATEMENT_LEVEL
    assert np.abs(got.residual - want.residual).max() <= RESTATEMENT_LEVEL
    assert pc.cone_ok(got.impulse, case["foot_mu"][:, 1])


# ---- 2. static equilibrium ----------------------------------------------------------------------------------------------------
def test_a_standing_robot_with_the_torques_that_hold_it_stays_still():
    case = pc.static_case()
    f = case["f"].reshape(8, 3)
    print("normal forces", f[:, 2].min(), "...", f[:, 2].max(), "largest tangential", np.abs(f[:, :2]).max())
    assert f[:, 2].min() > 40.0 and np.abs(f[:, :2]).max() < 1e-10
    got = pc.emulate_plant(case, pc.params(sweeps=300))
    pn = got.impulse.reshape(8, 3)[:, 2].sum()
    share = pn / (pc.DT * pc.total_mass() * rc.G)
    print("max |v+|", np.abs(got.v).max(), "sum p_n / (dt m g) - 1", share - 1.0, "residual", got.residual[0])
    assert got.status[0] == 0
    assert np.abs(got.v).max() <= 1e-6
    assert abs(share - 1.0) <= 1e-6
    assert got.residual[0] <= 1e-9
    assert pc.cone_ok(got.impulse, 0.5)


# ---- 3. free flight, 4. push --------------------------------------------------------------------------------------------------
def flying_case():
    rng = np.random.default_rng(5)
    q = np.array(rc.standing())[None]
    q[0, 5] += 1.0
    return pc.evaluated(q, 0.5 * rng.normal(size=(1, 30)), tau=3.0 * rng.normal(size=(1, 24)))


def test_free_flight_has_no_impulse_and_is_the_integrator():
    case = flying_case()
    got = pc.emulate_plant(case, pc.params(sweeps=20))
    assert got.status[0] == 0 and pc.bits_equal(got.impulse, np.zeros((1, 24))) and got.residual[0] == 0.0
    qdd = np.linalg.solve(case["M"][0], np.concatenate([np.zeros(6), case["tau"][0]]) - case["h"][0])[None]
    vn, pn, jn, Rn = wc.mirror_integrate(case["q"], case["v"], qdd, pc.DT)
    assert np.abs(got.v - vn).max() <= 1e-12
    assert np.abs(got.q[:, 3:6] - pn).max() <= 1e-12 and np.abs(got.q[:, 6:] - jn).max() <= 1e-12
    from scipy.spatial.transform import Rotation
    assert np.abs(Rotation.from_rotvec(got.q[:, 0:3]).as_matrix() - Rn).max() <= 1e-12


def test_a_push_changes_the_centroid_velocity_by_force_dt_over_mass():
    case = flying_case()
    force = np.array([10.0, -5.0, 3.0])
    pushed = dict(case, ext=np.concatenate([np.zeros(3), force])[None])
    prm = pc.params(sweeps=20)
    without, with_ = pc.emulate_plant(case, prm), pc.emulate_plant(pushed, prm)
    J_com = case["J"][0, 12:15]                                  # of the input evaluation
    got = pc.total_mass() * J_com @ (with_.v[0] - without.v[0]) / pc.DT
    print("force felt by the centroid", got)
    assert np.abs(got - force).max() <= 1e-9
    assert pc.bits_equal(with_.impulse, np.zeros((1, 24)))


# ---- 5. landing ---------------------------------------------------------------------------------------------------------------
def test_landing_from_one_centimetre_does_not_sink_into_the_floor():
    base = pc.static_case(lift=0.01)
    prm = pc.params(sweeps=100)
    q, v, imp = base["q"], base["v"], np.zeros((1, 24))
    lowest, pn, touched = [], [], None
    for tick in range(15):
        case = pc.evaluated(q, v, tau=base["tau"], impulse=imp)
        got = pc.emulate_plant(case, prm)
        assert got.status[0] == 0 and pc.cone_ok(got.impulse, 0.5)
        q, v, imp = got.q, got.v, got.impulse
        lowest.append(float(pc.lowest_vertex(q)[0]))
        pn.append(float(imp.reshape(8, 3)[:, 2].sum()))
        if touched is None and pn[-1] > 0:
            touched = tick
    print("lowest vertex", min(lowest), "touch-down at tick", touched, "sum p_n", pn)
    assert min(lowest) >= -1e-5
    assert touched is not None and all(x > 0 for x in pn[touched:])


# ---- 6. sliding ---------------------------------------------------------------------------------------------------------------
def test_a_sliding_robot_has_its_impulses_on_the_cone_against_the_motion():
    base = pc.static_case()
    from scipy.spatial.transform import Rotation
    v = np.zeros((1, 30))
    v[0, 3:6] = Rotation.from_rotvec(np.array(base["q"][0, 0:3])).as_matrix().T @ np.array([1.0, 0.0, 0.0])
    case = pc.evaluated(base["q"], v, tau=base["tau"])
    got = pc.emulate_plant(case, pc.params(sweeps=100))
    p = got.impulse.reshape(8, 3)
    on = p[:, 2] > 0
    assert got.status[0] == 0 and on.sum() >= 4 and pc.cone_ok(got.impulse, 0.5)
    hyp = np.hypot(p[on, 0], p[on, 1])
    print("vertices in contact", int(on.sum()), "largest |hypot / (mu p_n) - 1|", np.abs(hyp / (0.5 * p[on, 2]) - 1.0).max())
    assert (np.abs(hyp - 0.5 * p[on, 2]) <= 1e-12 * 0.5 * p[on, 2]).all() and (p[on, 0] < 0).all()


# ---- 7. rows that must not move -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pc.BAD_KINDS)
def test_rows_that_must_not_move_keep_their_bits_and_leave_their_neighbours_untouched(kind):
    got = pc.check_bad_row(kind, lambda case: pc.emulate_plant(case, pc.params(sweeps=5)))
    if kind != "hold":
        assert np.isnan(got.residual[pc.BAD_ROW])
    else:
        assert got.residual[pc.BAD_ROW] == pc.FILL                   # not touched


def test_in_place_null_optional_pointers_and_the_leading_dimension_of_tau():
    case, prm = pc.mix_case(), pc.params(sweeps=5)
    full = pc.emulate_plant(case, prm)
    same = lambda a, b, ks: all(pc.bits_equal(getattr(a, k), getattr(b, k)) for k in ks)
    assert same(pc.emulate_plant(case, prm, in_place=True), full, pc.Stepped._fields)
    assert same(pc.emulate_plant(case, prm, tau_ld=30), full, pc.Stepped._fields)
    for outputs in ((), ("status",), ("residual",)):
        got = pc.emulate_plant(dict(case, impulse=None), prm, outputs=outputs)
        cold = pc.emulate_plant(dict(case, impulse=None), prm)
        assert got.impulse is None and same(got, cold, ("q", "v") + outputs)
        assert (got.status is None) == ("status" not in outputs) and (got.residual is None) == ("residual" not in outputs)
    assert not pc.bits_equal(cold.v, full.v)                         # the warm start matters at five sweeps
    zero = dict(case, tau=np.zeros((16, 24)), ext=np.zeros((16, 6)), hold=np.zeros(16, np.uint8))
    assert same(pc.emulate_plant(case, prm, null=("tau", "ext", "hold")), pc.emulate_plant(zero, prm), pc.Stepped._fields)
    empty = pc.emulate_plant({k: a[:0] for k, a in case.items()}, prm)
    assert empty.q.shape == (0, 30)
    # zero sweeps: the admissible warm start is what is applied and returned
    got = pc.emulate_plant(case, pc.params(sweeps=0))
    assert pc.cone_ok(got.impulse, case["foot_mu"][:, 1])
    assert np.abs(got.impulse - np.array([pc.admissible(case["impulse"][b], case["foot_mu"][b, 1]) for b in range(16)])).max() < 1e-15


# ---- 8. bad arguments ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change, message", [
    (dict(sweeps=-1), "sweeps"), (dict(dt=0.0), "dt"), (dict(dt=np.inf), "dt"), (dict(dt=np.nan), "dt"), (dict(erp=-0.1), "erp"),
    (dict(erp=1.5), "erp"), (dict(erp=np.nan), "erp"), (dict(cfm=-1e-9), "cfm"), (dict(ground_z=np.nan), "ground_z"),
    (dict(ground_z=np.inf), "ground_z"), (dict(struct_size=8), "struct_size")])
def test_bad_parameters_are_refused(change, message):
    with pytest.raises(ValueError, match=message):
        pc.emulate_plant(pc.mix_case(), pc.params(**change))


def test_bad_pointers_and_sizes_are_refused():
    case, prm = pc.mix_case(), pc.params()
    for name in ("q", "v", "M", "h", "J", "pose", "foot_mu", "q_out"):
        with pytest.raises(ValueError, match="null q, v, M, h, J, pose, foot_mu, q_out or v_out"):
            pc.emulate_plant(case, prm, null=(name,))
    with pytest.raises(ValueError, match="null params"):
        pc.emulate_plant(case, None)
    with pytest.raises(ValueError, match="tau_ld"):
        pc.emulate_plant(case, prm, tau_ld=23)
    lib = pc.emu_lib()
    assert lib.cmpc_emu_walk_plant_step(-1, *([None] * 7), 24, None, None, None, prm, *([None] * 5)) == 1
    assert b"negative" in lib.cmpc_emu_walk_plant_last_error()


# ---- 11. the host API without a GPU -------------------------------------------------------------------------------------------
def test_plant_checks_its_arguments_without_a_device():
    p = rbd.Plant(0.01)
    assert (p.dt, p.sweeps, p.erp, p.cfm, p.ground_z) == (0.01, 50, 0.2, 0.0, 0.0)
    prm = rbd.Plant(0.005, sweeps=30, erp=0.1, cfm=1e-9, ground_z=-0.2).params()
    assert (prm.struct_size, prm.sweeps, prm.dt, prm.ground_z, prm.erp, prm.cfm) == (40, 30, 0.005, -0.2, 0.1, 1e-9)
    for kw, message in ((dict(dt=0.0), "dt"), (dict(dt=np.nan), "dt"), (dict(dt=0.01, sweeps=-1), "sweeps"),
                        (dict(dt=0.01, sweeps=2.5), "sweeps"), (dict(dt=0.01, erp=1.1), "erp"), (dict(dt=0.01, cfm=-1.0), "cfm"),
                        (dict(dt=0.01, ground_z=np.inf), "ground_z")):
        with pytest.raises(ValueError, match=message):
            rbd.Plant(**kw)
    assert rbd.PlantStep._fields == ("q", "v", "impulse", "status", "residual")


class _Stub:
    """A ``BatchedRobot`` that never touches a device: records which of integrate / simulate ``advance`` calls."""
    walking_model = rbd.BatchedRobot.walking_model
    _checked = staticmethod(lambda name, t, shape, dtype=None: t)

    def __init__(self):
        import torch
        self.model, self.device, self.calls = rc.model("hrp4"), torch.device("cpu"), []

    def integrate(self, *a, **k):
        self.calls.append(("integrate", a, k))

    def simulate(self, *a, **k):
        self.calls.append(("simulate", a, k))
        return "stepped"


def test_walking_model_takes_the_integrate_path_without_a_plant_and_simulate_with_one():
    import torch
    import types
    B = 3
    q, v = torch.zeros((B, 30), dtype=torch.float64), torch.zeros((B, 30), dtype=torch.float64)
    ro = types.SimpleNamespace(alive=torch.tensor([True, False, True]), spec=types.SimpleNamespace(delta=0.01),
                               state=torch.arange(B * 16, dtype=torch.float64).reshape(B, 16))
    wbc = (torch.ones((B, 24), dtype=torch.float64), torch.ones((B, 30), dtype=torch.float64), None, torch.tensor([0, 0, 3]), None)
    stub = _Stub()
    model = stub.walking_model(q, v, gait=None)
    assert not hasattr(model, "impulse") and not hasattr(model, "last_plant")
    model.advance(ro, wbc)
    (name, a, k), = stub.calls
    assert name == "integrate" and a[2] is wbc[1] and k["hold"].tolist() == [False, True, True] and k["out"][0] is q
    with pytest.raises(ValueError, match="go with a plant"):
        stub.walking_model(q, v, gait=None, ext=torch.zeros((B, 6), dtype=torch.float64))
    with pytest.raises(ValueError, match="rbd.Plant"):
        stub.walking_model(q, v, gait=None, plant=0.01)
    del stub.calls[:]
    plant, ext = rbd.Plant(0.01, sweeps=20), torch.zeros((B, 6), dtype=torch.float64)
    model = stub.walking_model(q, v, gait=None, plant=plant, ext=ext)
    assert tuple(model.impulse.shape) == (B, 24) and model.last_plant is None and model.ext is ext
    model.last_evaluation = "ev"
    model.advance(ro, wbc)
    (name, a, k), = stub.calls
    assert name == "simulate" and a[0] is q and a[1] is v and a[2] == "ev" and a[3] is wbc[0] and a[5] is plant
    assert a[4][:, 0].tolist() == [0.05] * B and torch.equal(a[4][:, 1], ro.state[:, 15])
    # a robot whose QP failed is not held; a dead one is
    assert k["hold"].tolist() == [False, True, False] and k["ext"] is ext and k["impulse"] is model.impulse and k["out"][1] is v
    assert model.last_plant == "stepped"
    assert not hasattr(stub.walking_model(q, v, gait=None, plant=plant, integrate=False), "advance")


# ---- 10. the stand-alone program under the sanitizers -------------------------------------------------------------------------
def test_stand_alone_program_is_clean_under_asan_ubsan(tmp_path):
    """tests/emu/walk_plant_emu_main.cpp (its own main) built with -fsanitize=address,undefined and run as a child process:
    exit status 0, no report.  The sanitizers' runtimes are linked into the program."""
    exe = str(tmp_path / "walk_plant_emu_main")
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-mfma", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined",
                           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(rc.ROOT, "tests", "emu", "walk_plant_emu_main.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    log = r.stdout + r.stderr
    assert "Sanitizer" not in log and "runtime error" not in log, log[-4000:]
    assert r.returncode == 0 and "ok B=16" in r.stdout, log[-4000:]

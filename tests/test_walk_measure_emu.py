"""CPU tier of the measurement that closes the walking loop (cmpc_walk_measure of include/cmpc_walk.h) on the emulated device
source (tests/emu/walk_measure_emu.cpp): the measured state, x_meas and innovation against the numpy restatement bit for
bit, the rows that must not be fed back, the tilt guard against scipy, NULL arguments and refusals, the MPC record of the
measured standing robots solved by the C oracle at the tick the GPU tier starts its closed loops, the kernel's resources and
the stand-alone program under the sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import rbd_common as rc
import walk_measure_common as mc
from cmpc_amd.problem import ProblemSpec
from oracle import oracle_lib as ol


# ---- 1. the mirror ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.MODELS)
def test_measured_state_x_meas_and_innovation_are_the_numpy_restatement_bit_for_bit(name):
    B = 18
    cen, pose, state = mc.mirror_case(name, B)
    got = mc.emulate_measure(cen, pose, state, np.ones(B, np.uint8))
    want = mc.mirror_measure(cen, pose, state)
    assert np.isfinite(cen).all() and np.isfinite(pose).all()
    for k in ("state", "x_meas", "innovation"):
        assert mc.bits_equal(getattr(got, k), getattr(want, k)), k
    assert (got.alive == 1).all()
    assert mc.bits_equal(got.state[:, 9:12], state[:, 9:12]) and mc.bits_equal(got.state[:, 14:16], state[:, 14:16])
    assert not np.array_equal(got.state[:, 0:9], state[:, 0:9]) and (got.x_meas[:, (15, 19)] == 0).all()
    assert np.array_equal(got.state[:, 12], pose[:, 2]) and np.array_equal(got.state[:, 13], pose[:, 8])


# ---- 2. rows that must not be fed back ----------------------------------------------------------------------------------------
def check_bad_rows(kind, run):
    """The rules of include/cmpc_walk.h on ``mc.bad_case(kind)``; run(case) -> ``mc.Measured`` (the GPU tier runs it too)."""
    clean, bad, rows = mc.bad_case(kind)
    B = clean["state"].shape[0]
    want, got = run(clean), run(bad)
    assert (want.alive == 1).all() and np.isfinite(want.x_meas).all() and np.isfinite(want.innovation).all()
    for b in rows:
        assert mc.bits_equal(got.state[b], bad["state"][b]), (kind, b)
        assert np.isnan(got.x_meas[b]).all() and np.isnan(got.innovation[b]).all(), (kind, b)
        assert got.alive[b] == 0, (kind, b)
    rest = np.delete(np.arange(B), rows)
    assert (got.alive[rest] == 1).all()
    for k in ("state", "x_meas", "innovation"):
        assert mc.bits_equal(getattr(got, k)[rest], getattr(want, k)[rest]), (kind, k)
    return got


def emulated_case(case, **kw):
    return mc.emulate_measure(case["centroid"], case["pose"], case["state"], case["alive"], mc.Z_MIN, np.cos(mc.TILT_MAX), **kw)


@pytest.mark.parametrize("kind", mc.BAD_KINDS)
def test_rows_that_must_not_be_fed_back_keep_their_state_and_leave_their_neighbours_untouched(kind):
    check_bad_rows(kind, emulated_case)
    if kind != "alive = 0":
        # without alive nothing is written in its place; the rows are refused all the same
        clean, bad, rows = mc.bad_case(kind)
        got = mc.emulate_measure(bad["centroid"], bad["pose"], bad["state"], None, mc.Z_MIN, np.cos(mc.TILT_MAX))
        assert got.alive is None and all(np.isnan(got.x_meas[b]).all() and mc.bits_equal(got.state[b], bad["state"][b]) for b in rows)


# ---- 3. the tilt guard --------------------------------------------------------------------------------------------------------
def test_tilt_guard_against_scipy():
    tilt_max, eps = 0.35, 1e-6
    rng = np.random.default_rng(47)
    w = []
    for sign in (-1.0, 1.0):                            # tilt_max -/+ eps about a horizontal axis, after a yaw
        for yaw in (0.0, 0.7, -2.0):
            a = rng.uniform(0, 2 * np.pi)
            tilt = Rotation.from_rotvec((tilt_max + sign * eps) * np.array([np.cos(a), np.sin(a), 0.0]))
            w.append((Rotation.from_rotvec([0.0, 0.0, yaw]) * tilt).as_rotvec())
    w += [np.array([0.0, 0.0, 3.1]), np.zeros(3)]       # a pure yaw has tilt 0; so has the zero vector
    w = np.array(w)
    B = w.shape[0]
    tilt = np.arccos(np.clip(Rotation.from_rotvec(w).as_matrix()[:, 2, 2], -1.0, 1.0))
    assert np.abs(np.abs(tilt[:6] - tilt_max) - eps).max() < 1e-9 and (tilt[6:] < 1e-7).all()
    cen, pose, state = (rng.normal(size=(B, n)) for n in (9, 21, 16))
    pose[:, 18:21] = w
    got = mc.emulate_measure(cen, pose, state, np.ones(B, np.uint8), -np.inf, np.cos(tilt_max))
    assert got.alive.tolist() == [1, 1, 1, 0, 0, 0, 1, 1]
    assert (np.isnan(got.x_meas).all(axis=1) == (got.alive == 0)).all()
    # both guards disabled: every finite row is fed back, whatever its height and tilt
    cen[:, 2] = -5.0
    pose[0, 18:21] = (3.0, 0.0, 0.0)
    off = mc.emulate_measure(cen, pose, state, np.ones(B, np.uint8), -np.inf, -np.inf)
    assert (off.alive == 1).all() and mc.bits_equal(off.state, mc.mirror_measure(cen, pose, state).state)
    # +inf: nothing is above it
    assert (mc.emulate_measure(cen, pose, state, np.ones(B, np.uint8), np.inf, -np.inf).alive == 0).all()


# ---- 4. NULL arguments and refusals -------------------------------------------------------------------------------------------
def test_null_alive_null_outputs_the_empty_batch_and_refusals():
    B = 18
    cen, pose, state = mc.mirror_case("hrp4", B)
    full = mc.emulate_measure(cen, pose, state, np.ones(B, np.uint8))
    for outputs in ((), ("x_meas",), ("innovation",)):
        got = mc.emulate_measure(cen, pose, state, None, outputs=outputs)
        assert got.alive is None and mc.bits_equal(got.state, full.state)
        assert (got.x_meas is None) == ("x_meas" not in outputs) and (got.innovation is None) == ("innovation" not in outputs)
        for k in outputs:
            assert mc.bits_equal(getattr(got, k), getattr(full, k))
    empty = mc.emulate_measure(np.zeros((0, 9)), np.zeros((0, 21)), np.zeros((0, 16)))
    assert empty.state.shape == (0, 16)
    lib = mc.emu_lib()
    assert lib.cmpc_emu_walk_measure(0, None, None, 0.0, 0.0, None, None, None, None) == 0
    with pytest.raises(ValueError, match="NaN"):
        mc.emulate_measure(cen, pose, state, z_min=np.nan)
    with pytest.raises(ValueError, match="NaN"):
        mc.emulate_measure(cen, pose, state, cos_tilt_min=np.nan)
    with pytest.raises(ValueError, match="null"):
        mc.emulate_measure(cen, pose, None)
    s = np.array(state)
    assert lib.cmpc_emu_walk_measure(-1, cen.ctypes.data, pose.ctypes.data, 0.0, 0.0, s.ctypes.data, None, None, None) == 1
    assert b"negative" in lib.cmpc_emu_walk_measure_last_error() and mc.bits_equal(s, state)


# ---- 5. the loop can close at the tick the GPU tier starts from --------------------------------------------------------------
def test_the_record_of_the_measured_standing_robots_is_solved_by_the_oracle_at_the_start_tick():
    """The standing robots of the GPU tier's closed loops, their emulated centroid through the emulated measurement into a
    state with mass = the model's, the host record builder at the start tick, the C oracle: status 0 or 3 on at least 4 of
    the 6 (this build: 6 of 6 at tick 260, |hw| up to 0.92; with the robots at rest the same tick solves too, but tick 360
    does not)."""
    B, scene, spec = mc.B_LOOP, mc.shipped(), ProblemSpec(N=mc.N_LOOP)
    q, v = mc.standing_robots()
    ev = rc.emulate("hrp4", q, v, outputs=("centroid", "pose"))
    assert np.abs(ev.centroid[:, 6:9]).max(axis=1).min() > 1e-2          # no robot's momentum is zero
    state = np.zeros((B, 16))
    state[:, 14], state[:, 15] = mc.loop_mass(), mc.loop_mu()
    s = mc.emulate_measure(ev.centroid, ev.pose, state, np.ones(B, np.uint8), 0.4, np.cos(0.5))
    assert (s.alive == 1).all() and mc.bits_equal(s.state[:, 0:9], ev.centroid)
    t0 = mc.start_tick(scene)
    assert scene.is_ss[t0] and not scene.is_ss[t0 + spec.N]
    s = s.state
    rec = scene.build_records(spec, np.full(B, t0), s[:, 0:3], s[:, 3:6], s[:, 6:9], s[:, 9:12], s[:, 12], s[:, 13], s[:, 14], s[:, 15])
    assert mc.bits_equal(rec[:, 0:9], ev.centroid) and np.array_equal(rec[:, 12], ev.pose[:, 2]) and np.array_equal(rec[:, 16], ev.pose[:, 8])
    cs = ol.default_spec(N=spec.N, nv=spec.nv, tol=spec.tol, max_iter=spec.max_iter, k1=spec.k1, k2=spec.k2, prox=spec.prox,
                         acc_tol=spec.acc_tol)
    _, status, iters, _ = ol.solve_batch(cs, rec)
    print("start tick", t0, "oracle status", status.tolist(), "iterations", iters.tolist(),
          "largest |hw|", float(np.abs(ev.centroid[:, 6:9]).max()), "solved", int(np.isin(status, (0, 3)).sum()), "of", B)
    assert np.isin(status, (0, 3)).sum() >= 4


# ---- 6. resources -------------------------------------------------------------------------------------------------------------
def test_the_unit_has_one_kernel_with_no_scratch_and_the_lds_the_harness_reports():
    pkg = os.path.join(rc.ROOT, "online-non-linear-centroidal-mpc-with-stability-guarantees-for-robust-locomotion-of-legged-robots-_amd")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, os.path.join(pkg, "csrc", "walk_measure.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, cur = {}, None
    for ln in r.stderr.splitlines():                     # (the remarks only)
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur:
            res[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    print(res)
    assert len(res) == 1 and "walk_measure_kernel" in next(iter(res)), sorted(res)
    (one,) = res.values()
    assert one["ScratchSize"] == 0 and one["LDS Size"] == mc.emu_lib().cmpc_emu_walk_measure_lds_bytes() == 1024


# ---- 7. the stand-alone program under the sanitizers --------------------------------------------------------------------------
def test_stand_alone_program_is_clean_under_asan_ubsan(tmp_path):
    """tests/emu/walk_measure_emu_main.cpp (its own main) built with -fsanitize=address,undefined and run as a child
    process: exit status 0, no report.  The sanitizers' runtimes are linked into the program."""
    exe = str(tmp_path / "walk_measure_emu_main")
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-mfma", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined",
                           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(rc.ROOT, "tests", "emu", "walk_measure_emu_main.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    log = r.stdout + r.stderr
    assert "Sanitizer" not in log and "runtime error" not in log, log[-4000:]
    assert r.returncode == 0 and "ok B=12" in r.stdout, log[-4000:]

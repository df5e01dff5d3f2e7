"""CPU tier: the device source of the batched rigid-body model (csrc/rbd_kernel.hpp) run on the CPU through
tests/emu/rbd_emu.cpp, against the independent reference of tests/rbd_reference.py (torch float64, automatic
differentiation of plain forward kinematics on the raw link tree) -- HRP-4, a 24-joint chain and a 24-joint star, 8
instances each, every output within 1e-9 x max(1, largest |entry|) --, and the structural facts that need no reference."""
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import rbd_common as rc
from cmpc_amd import rbd


@pytest.mark.parametrize("name", rc.MODELS)
def test_every_output_matches_the_reference(name):
    got, want = rc.emulated(name), rc.reference(name)
    w = rc.worst(got, want)
    print(name, "error / level:", w)
    assert all(np.isfinite(getattr(got, k)).all() for k in rc.FIELDS)
    assert max(w.values()) <= 1.0, w


@pytest.mark.parametrize("name", rc.MODELS)
def test_structure_of_the_mass_matrix(name):
    e, m = rc.emulated(name), rc.model(name)
    for b in range(8):
        M = e.M[b]
        assert np.array_equal(M, M.T)                                       # bit for bit
        assert np.abs(M[3:6, 3:6] - m.total_mass * np.eye(3)).max() <= 1e-10
        np.linalg.cholesky(M)


@pytest.mark.parametrize("name", rc.MODELS)
def test_at_rest_h_is_gravity_and_the_bias_accelerations_vanish(name):
    q, _ = rc.sample(name)
    e, m = rc.emulate(name, q, np.zeros_like(q)), rc.model(name)
    for b in range(8):
        Rb = Rotation.from_rotvec(np.array(q[b, 0:3])).as_matrix()
        assert np.abs(e.h[b, 3:6] - Rb.T @ np.array([0.0, 0.0, m.total_mass * rc.G])).max() <= 1e-9 * m.total_mass * rc.G
    assert np.abs(e.jdqd).max() == 0.0 and np.abs(e.vel).max() == 0.0 and np.abs(e.centroid[:, 3:]).max() == 0.0


@pytest.mark.parametrize("name", rc.MODELS)
def test_com_velocity_is_the_com_jacobian_times_v(name):
    e = rc.emulated(name)
    _, v = rc.sample(name)
    Jv = np.einsum('brn,bn->br', e.J, v)
    assert np.abs(e.centroid[:, 3:6] - Jv[:, 12:15]).max() <= 1e-12
    assert np.abs(e.vel - Jv).max() <= 1e-12 * max(1.0, np.abs(Jv).max())
    assert np.array_equal(e.centroid[:, 0:3], e.pose[:, 12:15]) and np.array_equal(e.centroid[:, 3:6], e.vel[:, 12:15])


def test_log_agrees_with_scipy_up_to_pi_minus_a_tenth():
    rng = np.random.default_rng(5)
    axes = rng.normal(size=(100, 3))
    angles = np.concatenate([rng.uniform(0.0, np.pi - 0.1, size=96), [np.pi - 0.1, 1e-9, 1e-5, 1e-3]])
    R = Rotation.from_rotvec(axes / np.linalg.norm(axes, axis=1, keepdims=True) * angles[:, None]).as_matrix()
    w = np.zeros((100, 3))
    rc.emu_lib().cmpc_emu_rbd_log(100, np.ascontiguousarray(R).ctypes.data, w.ctypes.data)
    want = Rotation.from_matrix(R).as_rotvec()
    err = np.abs(w - want).max()
    print("Log vs scipy:", err)
    assert err <= 1e-12                                                     # (|s| >= sin 0.1: fp64 rounding over sin t, ~1e-15)


def test_log_of_the_identity_is_exactly_zero_and_finite_near_pi():
    lib = rc.emu_lib()
    w = np.ones(3)
    lib.cmpc_emu_rbd_log(1, np.eye(3).ctypes.data, w.ctypes.data)
    assert np.array_equal(w, np.zeros(3)) and not np.signbit(w).any()
    axes = np.random.default_rng(6).normal(size=(40, 3))
    angles = np.concatenate([np.pi - np.logspace(-16, -1, 39), [np.pi]])
    R = np.ascontiguousarray(Rotation.from_rotvec(axes / np.linalg.norm(axes, axis=1, keepdims=True) * angles[:, None]).as_matrix())
    w = np.zeros((40, 3))
    lib.cmpc_emu_rbd_log(40, R.ctypes.data, w.ctypes.data)
    assert np.isfinite(w).all() and np.abs(np.linalg.norm(w, axis=1) - angles).max() <= 1e-6


def test_exp_takes_its_series_branch_and_the_kernels_sine_is_good():
    lib = rc.emu_lib()
    rng = np.random.default_rng(8)
    d = rng.normal(size=(60, 3))
    angles = np.concatenate([[0.0], np.logspace(-12, 0.49, 59)])             # across the branch at |w|^2 = 1e-6
    w = np.ascontiguousarray(d / np.linalg.norm(d, axis=1, keepdims=True) * angles[:, None])
    R = np.zeros((60, 3, 3))
    lib.cmpc_emu_rbd_exp(60, w.ctypes.data, R.ctypes.data)
    assert np.array_equal(R[0], np.eye(3))
    assert np.abs(R - Rotation.from_rotvec(w).as_matrix()).max() <= 1e-15 * 8
    x = np.concatenate([rng.uniform(-10.0, 10.0, size=2000), np.arange(-8, 9) * (np.pi / 4), [0.0]])
    s, c = np.zeros_like(x), np.zeros_like(x)
    lib.cmpc_emu_rbd_sincos(len(x), x.ctypes.data, s.ctypes.data, c.ctypes.data)
    assert max(np.abs(s - np.sin(x)).max(), np.abs(c - np.cos(x)).max()) <= 4e-16


@pytest.mark.parametrize("word", [0, 17, 29])
@pytest.mark.parametrize("where", ["q", "v"])
def test_a_planted_nan_row_is_nan_and_its_neighbours_are_untouched(where, word):
    q, v = (a.copy() for a in rc.sample("hrp4"))
    (q if where == "q" else v)[3, word] = np.nan if word else np.inf
    got, clean = rc.emulate("hrp4", q, v), rc.emulated("hrp4")
    for k in rc.FIELDS:
        a = getattr(got, k)
        assert np.isnan(a[3]).all(), k
        assert np.array_equal(np.delete(a, 3, axis=0), np.delete(getattr(clean, k), 3, axis=0)), k


def test_null_outputs_are_skipped_and_rows_do_not_depend_on_the_batch():
    q, v = rc.sample("chain")
    part = rc.emulate("chain", q, v, outputs=("M", "centroid"))
    assert part.J is None and part.h is None
    assert np.array_equal(part.M, rc.emulated("chain").M) and np.array_equal(part.centroid, rc.emulated("chain").centroid)
    alone = rc.emulate("chain", q[5:6], v[5:6])
    assert all(np.array_equal(getattr(alone, k)[0], getattr(rc.emulated("chain"), k)[5]) for k in rc.FIELDS)


def write_case(path, name, B=3):
    """The input file of tests/emu/rbd_emu_main.cpp: the model's tables, then B instances."""
    q, v = rc.sample(name)
    with open(path, "w") as f:
        for a in rc.model(name).tables():
            f.write(" ".join(repr(x) for x in a.ravel().tolist()) + "\n")
        f.write(f"{B} {rc.G!r}\n")
        for a in (q[:B], v[:B]):
            f.write(" ".join(repr(x) for x in a.ravel().tolist()) + "\n")


def test_stand_alone_program_is_clean_under_asan_ubsan(tmp_path):
    """tests/emu/rbd_emu_main.cpp (its own main) built with -fsanitize=address,undefined and run as a child process on three
    instances of each model: exit status 0, no report.  The sanitizers' runtimes are linked into the program, so it does not
    depend on what else the environment loads; the environment is passed on as it is."""
    exe = str(tmp_path / "rbd_emu_main")
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-mfma", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined",
                           "-static-libasan", "-static-libubsan",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(rc.ROOT, "tests", "emu", "rbd_emu_main.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for name in rc.MODELS:
        case = str(tmp_path / f"{name}.txt")
        write_case(case, name)
        r = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=300)
        log = r.stdout + r.stderr
        assert "Sanitizer" not in log and "runtime error" not in log, log[-4000:]
        assert r.returncode == 0 and "ok B=3" in r.stdout, log[-4000:]


def test_a_base_rotation_vector_whose_square_overflows_is_a_nan_row():
    """Finite words, but |q[0:3]|^2 is not: the row takes the NaN exit as well (no angle is formed from it)."""
    q, v = (a.copy() for a in rc.sample("star"))
    q[5, 1] = 1e200
    got, clean = rc.emulate("star", q, v), rc.emulated("star")
    for k in rc.FIELDS:
        a = getattr(got, k)
        assert np.isnan(a[5]).all(), k
        assert np.array_equal(np.delete(a, 5, axis=0), np.delete(getattr(clean, k), 5, axis=0)), k
    s, c = np.zeros(3), np.zeros(3)
    x = np.array([np.inf, -np.inf, np.nan])
    rc.emu_lib().cmpc_emu_rbd_sincos(3, x.ctypes.data, s.ctypes.data, c.ctypes.data)
    assert np.isnan(s).all() and np.isnan(c).all()

"""CPU tier: the per-instance path of the rigid-body model's device source (csrc/rbd_kernel.hpp, run_instance<true>, what
csrc/rbd_inertial.hip launches) run on the CPU through tests/emu/rbd_inertial_emu.cpp.  With every row the model's own it is
the existing kernel bit for bit; with drawn rows every robot is bit for bit the existing kernel on a model built from its
row, and within the project's level of the independent reference (tests/rbd_reference.py) on that model's tree; a bad row is
a NaN robot and nobody else's business."""
import os
import subprocess

import numpy as np
import pytest

import rbd_common as rc
import rbd_inertial_common as ic

B = 8


@pytest.mark.parametrize("name", rc.MODELS)
def test_uniform_rows_are_the_existing_kernel_bit_for_bit(name):
    tab = np.tile(rc.model(name).inertial(), (B, 1, 1))
    got, want = ic.emulate(name, *rc.sample(name), tab), rc.emulated(name)
    for k in rc.FIELDS:
        assert np.array_equal(getattr(got, k), getattr(want, k)), k


@pytest.mark.parametrize("name", rc.MODELS)
def test_every_robot_is_the_existing_kernel_on_a_model_built_from_its_row(name):
    q, v = rc.sample(name)
    got, tab = ic.emulated(name), ic.rows(name)
    assert np.array_equal(tab[0], rc.model(name).inertial()) and not np.array_equal(tab[1], tab[0])
    for b in range(B):
        want = rc.emulate_tables(ic.model_from_row(name, tab[b]).tables(), q[b:b + 1], v[b:b + 1])
        for k in rc.FIELDS:
            assert ic.bits_equal(getattr(got, k)[b], getattr(want, k)[0]), (b, k)
    # and the rows matter: robot 1 is not the nominal robot at the same (q, v)
    nominal = rc.emulate(name, q[1:2], v[1:2])
    assert not np.array_equal(got.M[1], nominal.M[0]) and not np.array_equal(got.centroid[1], nominal.centroid[0])


@pytest.mark.parametrize("name", rc.MODELS)
def test_every_robot_matches_the_reference_on_its_own_tree(name):
    import rbd_reference as ref
    from cmpc_amd import rbd
    q, v = rc.sample(name)
    got, tab = ic.emulated(name), ic.rows(name)
    worst = {}
    for b in range(B):
        want = ref.evaluate_batch(ref.tree_from_model(ic.model_from_row(name, tab[b])), q[b:b + 1], v[b:b + 1], rc.G)
        w = rc.worst(rbd.Evaluation(*(getattr(got, k)[b:b + 1] for k in rc.FIELDS)), want)
        worst = {k: max(w[k], worst.get(k, 0.0)) for k in w}
    print(name, "error / level:", worst)
    assert all(np.isfinite(getattr(got, k)).all() for k in rc.FIELDS)
    assert max(worst.values()) <= 1.0, worst


BAD = {"NaN": (3, 117, np.nan), "inf": (3, 249, np.inf), "negative mass": (3, 10 * 7, -0.25), "inf mass": (3, 0, np.inf)}


@pytest.mark.parametrize("kind", sorted(BAD) + ["no mass at all"])
def test_a_bad_row_is_a_nan_robot_and_its_neighbours_are_untouched(kind):
    q, v = rc.sample("hrp4")
    tab = np.array(ic.rows("hrp4"))
    if kind == "no mass at all":
        b = 5
        tab[b, :, 0] = 0.0
    else:
        b, word, value = BAD[kind]
        tab[b].reshape(-1)[word] = value
    got, clean = ic.emulate("hrp4", q, v, tab), ic.emulated("hrp4")
    for k in rc.FIELDS:
        a = getattr(got, k)
        assert np.isnan(a[b]).all(), k
        assert ic.bits_equal(np.delete(a, b, axis=0), np.delete(getattr(clean, k), b, axis=0)), k


def test_a_zero_mass_on_one_body_is_not_a_bad_row():
    """>= 0, as on the host: a massless link is a legitimate model."""
    q, v = rc.sample("star")
    tab = np.array(ic.rows("star"))
    tab[2, 9, 0] = 0.0
    got = ic.emulate("star", q, v, tab)
    want = rc.emulate_tables(ic.model_from_row("star", tab[2]).tables(), q[2:3], v[2:3])
    assert all(ic.bits_equal(getattr(got, k)[2], getattr(want, k)[0]) for k in rc.FIELDS)


def test_null_outputs_are_skipped_and_rows_do_not_depend_on_the_batch():
    q, v = rc.sample("chain")
    tab, full = ic.rows("chain"), ic.emulated("chain")
    part = ic.emulate("chain", q, v, tab, outputs=("M", "centroid"))
    assert part.J is None and part.h is None
    assert np.array_equal(part.M, full.M) and np.array_equal(part.centroid, full.centroid)
    alone = ic.emulate("chain", q[5:6], v[5:6], tab[5:6])
    assert all(np.array_equal(getattr(alone, k)[0], getattr(full, k)[5]) for k in rc.FIELDS)
    # a bad row takes its exit with every output skipped, too
    bad = np.array(tab)
    bad[4, 3, 2] = np.nan
    none = ic.emulate("chain", q, v, bad, outputs=())
    assert all(x is None for x in none)


def write_case(path, name, B=3):
    """The input file of tests/emu/rbd_inertial_emu_main.cpp: the model's tables, B instances, their rows."""
    q, v = rc.sample(name)
    with open(path, "w") as f:
        for a in rc.model(name).tables():
            f.write(" ".join(repr(x) for x in a.ravel().tolist()) + "\n")
        f.write(f"{B} {rc.G!r}\n")
        for a in (q[:B], v[:B], ic.rows(name)[:B]):
            f.write(" ".join(repr(x) for x in a.ravel().tolist()) + "\n")


def test_stand_alone_program_is_clean_under_asan_ubsan(tmp_path):
    """tests/emu/rbd_inertial_emu_main.cpp (its own main) built with -fsanitize=address,undefined and run as a child process
    on three robots of each model, their own rows, and once more with a bad row: exit status 0, no report.  The
    sanitizers' runtimes are linked into the program; nothing is loaded into this process."""
    exe = str(tmp_path / "rbd_inertial_emu_main")
    subprocess.check_call(["g++", "-std=c++17", "-pthread", "-mfma", "-ffp-contract=off", "-O1", "-g", "-fsanitize=address,undefined",
                           "-static-libasan", "-static-libubsan",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(rc.ROOT, "tests", "emu", "rbd_inertial_emu_main.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for name in rc.MODELS:
        case = str(tmp_path / f"{name}.txt")
        write_case(case, name)
        r = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=300)
        log = r.stdout + r.stderr
        assert "Sanitizer" not in log and "runtime error" not in log, log[-4000:]
        assert r.returncode == 0 and "ok B=3" in r.stdout, log[-4000:]

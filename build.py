"""Build every native artefact in-tree (HIP library for gfx950, C oracle, host-emulation harness)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "online-non-linear-centroidal-mpc-with-stability-guarantees-for-robust-locomotion-of-legged-robots-_amd")


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


CSRC = os.path.join(PKG, "csrc")
# the solver's device source, which the host emulation and the device unit harness compile as well
KERNEL_DEPS = [os.path.join(CSRC, "cmpc_kernel.hpp"), os.path.join(CSRC, "cmpc_lds_asm.hpp"), os.path.join(CSRC, "cmpc_wave.hpp"),
               os.path.join(ROOT, "include", "cmpc.h")]
# everything the HIP library (and each of its diagnostic variants) is built from; DEVICE_UNITS are the translation units:
# the solver, the batched whole-body QP (include/cmpc_wbc.h) and the batched rigid-body model (include/cmpc_rbd.h), same library
# the device source of the batched rigid-body model (include/cmpc_rbd.h), which tests/emu/rbd_emu.cpp compiles as well
RBD_DEPS = [os.path.join(CSRC, "rbd_kernel.hpp"), os.path.join(ROOT, "include", "cmpc_rbd.h")]
# (rbd_inertial.hip, cmpc_rbd_eval_inertial, is that source's per-instance path: tests/emu/rbd_inertial_emu.cpp compiles it too)
# the device source of the walking loop around it (include/cmpc_walk.h), which tests/emu/rbd_walk_emu.cpp compiles as well
WALK_DEPS = [os.path.join(CSRC, "rbd_walk_kernel.hpp"), os.path.join(ROOT, "include", "cmpc_walk.h")]
# the device source of the measurement that closes that loop (cmpc_walk_measure), which tests/emu/walk_measure_emu.cpp compiles as well
MEASURE_DEPS = [os.path.join(CSRC, "walk_measure_kernel.hpp"), os.path.join(ROOT, "include", "cmpc_walk.h")]
# the device source of the contact plant (cmpc_walk_plant_step), which tests/emu/walk_plant_emu.cpp compiles as well
PLANT_DEPS = [os.path.join(CSRC, "walk_plant_kernel.hpp"), os.path.join(CSRC, "rbd_walk_kernel.hpp"),
              os.path.join(ROOT, "include", "cmpc_walk.h")]
DEVICE_UNITS = [os.path.join(CSRC, "cmpc_hip.hip"), os.path.join(CSRC, "wbc_qp.hip"), os.path.join(CSRC, "rbd.hip"),
                os.path.join(CSRC, "rbd_walk.hip"), os.path.join(CSRC, "walk_measure.hip"), os.path.join(CSRC, "walk_plant.hip"),
                os.path.join(CSRC, "rbd_inertial.hip")]
DEVICE_DEPS = DEVICE_UNITS + KERNEL_DEPS + RBD_DEPS + WALK_DEPS + MEASURE_DEPS + PLANT_DEPS + [
    os.path.join(CSRC, "cmpc_order_fit.h"), os.path.join(CSRC, "rbd_model.h"), os.path.join(ROOT, "include", "cmpc_wbc.h")]
EMU_DIR = os.path.join(ROOT, "tests", "emu")


def _hipcc_lib(out, defines=(), force=False, verbose=False):
    if force or _newer(out, DEVICE_DEPS):
        subprocess.check_call(["hipcc"] + (["-Rpass-analysis=kernel-resource-usage"] if verbose else [])
                              + ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared"]
                              + ["-D" + d for d in defines] + ["-o", out] + DEVICE_UNITS)
    return out


def _emu_lib(src, out, defines=(), force=False):
    src, out = os.path.join(EMU_DIR, src), os.path.join(EMU_DIR, out)
    if force or _newer(out, [src, os.path.join(EMU_DIR, "cmpc_emu.cpp")] + KERNEL_DEPS):
        # (-mfma -ffp-contract=off: the kernel's explicit CMPC_FMA are single instructions, and nothing else is fused)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-pthread"]
                              + ["-D" + d for d in defines] + ["-o", out, src])
    return out


def build_hip(force=False, verbose=False):
    return _hipcc_lib(os.path.join(PKG, "libcmpc_amd.so"), force=force, verbose=verbose)


def build_hip_profile(force=False):
    """Diagnostic variant with in-kernel phase timers (tools/ only; never loaded by the package)."""
    return _hipcc_lib(os.path.join(ROOT, "tools", "libcmpc_amd_prof.so"), ["CMPC_PROFILE"], force)


def build_hip_dev(force=False):
    """Developer variant (tools/ only; never loaded by the package unless CMPC_LIB_PATH names it): -DCMPC_DEV_KNOBS compiles
    in the environment knobs of the occupancy / kernel-choice studies (CMPC_WG_PER_CU, CMPC_PAIR, CMPC_PAIR_PER_CU), which
    the shipped library does not read."""
    return _hipcc_lib(os.path.join(ROOT, "tools", "libcmpc_amd_dev.so"), ["CMPC_DEV_KNOBS"], force)


def build_hip_no_reuse(force=False, profile=False):
    """Diagnostic variant (tools/ only; loaded through CMPC_LIB_PATH): -DCMPC_NO_EVAL_REUSE, the one-wave 4-vertex kernel that
    evaluates every stage of a retry pass again -- the third leg of the A/B runs, and with profile=True the `before` of
    tools/phase_profile.py's retry figures.  Built with -DCMPC_SEPARATE_STEP as well: the step applied in the stage load
    makes a kernel track its failed passes whether it reuses their evaluations or not (it parks and restores the error
    measures), so without it this would no longer be the kernel that profiles/retry_reuse_* measured as `before`."""
    return _hipcc_lib(os.path.join(ROOT, "tools", "libcmpc_amd_noreuse_prof.so" if profile else "libcmpc_amd_noreuse.so"),
                      ["CMPC_NO_EVAL_REUSE", "CMPC_SEPARATE_STEP"] + (["CMPC_PROFILE"] if profile else []), force)


def build_hip_separate_step(force=False, profile=False):
    """Diagnostic variant (tools/ only; loaded through CMPC_LIB_PATH): -DCMPC_SEPARATE_STEP, the one-wave 4-vertex kernels that
    apply the Newton step in a pass of their own (apply_step) instead of where the next matrix sweep loads the iterate -- the
    other leg of the A/B runs, and with profile=True the `before` of tools/phase_profile.py's step figures."""
    return _hipcc_lib(os.path.join(ROOT, "tools", "libcmpc_amd_sepstep_prof.so" if profile else "libcmpc_amd_sepstep.so"),
                      ["CMPC_SEPARATE_STEP"] + (["CMPC_PROFILE"] if profile else []), force)


def build_oracle(force=False):
    out = os.path.join(ROOT, "oracle", "libcmpc_oracle.so")
    deps = [os.path.join(ROOT, "oracle", "cmpc_oracle.c"), os.path.join(ROOT, "include", "cmpc.h")]
    if force or _newer(out, deps):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-B", "libcmpc_oracle.so"],
                              stdout=subprocess.DEVNULL)
    return out


def build_emu(force=False):
    return _emu_lib("cmpc_emu.cpp", "libcmpc_emu.so", force=force)


def build_emu_gain(force=False):
    """Host emulation of the gain variant of the solver (tests/emu/cmpc_emu_gain.cpp): test harness only."""
    return _emu_lib("cmpc_emu_gain.cpp", "libcmpc_emu_gain.so", force=force)


def build_emu_consts(force=False):
    """Host emulation of the solver with per-instance constants (tests/emu/cmpc_emu_consts.cpp): test harness only."""
    return _emu_lib("cmpc_emu_consts.cpp", "libcmpc_emu_consts.so", force=force)


def build_emu_gain_consts(force=False):
    """Host emulation of the gain variant with per-instance constants (tests/emu/cmpc_emu_gain_consts.cpp): test harness only."""
    return _emu_lib("cmpc_emu_gain_consts.cpp", "libcmpc_emu_gain_consts.so", force=force)


def build_emu_reuse(force=False, reuse=True):
    """Host emulation with counters on the retried factorisations (tests/emu/cmpc_emu_reuse.cpp): test harness only.
    reuse=False builds the kernel source with -DCMPC_NO_EVAL_REUSE, the path that evaluates every stage of a retry pass again."""
    return _emu_lib("cmpc_emu_reuse.cpp", "libcmpc_emu_reuse.so" if reuse else "libcmpc_emu_noreuse.so",
                    [] if reuse else ["CMPC_NO_EVAL_REUSE"], force)


def build_emu_step(force=False, fused=True):
    """Host emulation with counters on the step application (tests/emu/cmpc_emu_step.cpp): test harness only.
    fused=False builds the kernel source with -DCMPC_SEPARATE_STEP, the path that applies the step in a pass of its own."""
    return _emu_lib("cmpc_emu_step.cpp", "libcmpc_emu_step.so" if fused else "libcmpc_emu_sepstep.so",
                    [] if fused else ["CMPC_SEPARATE_STEP"], force)


def build_emu_rbd(force=False):
    """Host emulation of the batched rigid-body model (tests/emu/rbd_emu.cpp): test harness only."""
    src, out = os.path.join(EMU_DIR, "rbd_emu.cpp"), os.path.join(EMU_DIR, "librbd_emu.so")
    if force or _newer(out, [src] + RBD_DEPS):
        # (-ffp-contract=off: the kernel source forms every product and sum as written, in both of its builds)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                               "-o", out, src])
    return out


def build_emu_rbd_inertial(force=False):
    """Host emulation of the rigid-body model with per-robot inertial parameters (tests/emu/rbd_inertial_emu.cpp, on the
    harness of rbd_emu.cpp): test harness only."""
    src, out = os.path.join(EMU_DIR, "rbd_inertial_emu.cpp"), os.path.join(EMU_DIR, "librbd_inertial_emu.so")
    if force or _newer(out, [src, os.path.join(EMU_DIR, "rbd_emu.cpp")] + RBD_DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                               "-o", out, src])
    return out


def build_emu_rbd_walk(force=False):
    """Host emulation of the walking loop (tests/emu/rbd_walk_emu.cpp, with the rigid-body model's in it): test harness only."""
    src, out = os.path.join(EMU_DIR, "rbd_walk_emu.cpp"), os.path.join(EMU_DIR, "librbd_walk_emu.so")
    if force or _newer(out, [src, os.path.join(EMU_DIR, "rbd_emu.cpp")] + RBD_DEPS + WALK_DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                               "-o", out, src])
    return out


def build_emu_walk_measure(force=False):
    """Host emulation of the measurement (tests/emu/walk_measure_emu.cpp, on the harness of rbd_emu.cpp): test harness only."""
    src, out = os.path.join(EMU_DIR, "walk_measure_emu.cpp"), os.path.join(EMU_DIR, "libwalk_measure_emu.so")
    if force or _newer(out, [src, os.path.join(EMU_DIR, "rbd_emu.cpp")] + RBD_DEPS + MEASURE_DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                               "-o", out, src])
    return out


def build_emu_walk_plant(force=False):
    """Host emulation of the contact plant (tests/emu/walk_plant_emu.cpp, on the harness of rbd_emu.cpp): test harness only."""
    src, out = os.path.join(EMU_DIR, "walk_plant_emu.cpp"), os.path.join(EMU_DIR, "libwalk_plant_emu.so")
    if force or _newer(out, [src, os.path.join(EMU_DIR, "rbd_emu.cpp")] + RBD_DEPS + PLANT_DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                               "-o", out, src])
    return out


def build_device_unit(force=False):
    """GPU-tier unit harness for the device-only primitives (tests/gpu_unit): never loaded by the package."""
    src = os.path.join(ROOT, "tests", "gpu_unit", "cmpc_device_unit.hip")
    out = os.path.join(ROOT, "tests", "gpu_unit", "libcmpc_device_unit.so")
    if force or _newer(out, [src] + KERNEL_DEPS):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-o", out, src])
    return out


def build_tools(force=False):
    """Small stand-alone HIP programs the profiling scripts use (tools/ubench): the HBM counter calibration of
    tools/profile_round.sh and the LDS b128 repro.  Not part of the product library."""
    outs = []
    for name in ("hbm_calib", "lds_b128_repro"):
        src = os.path.join(ROOT, "tools", "ubench", name + ".hip")
        out = os.path.join(ROOT, "tools", "ubench", name)
        if force or _newer(out, [src]):
            r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-o", out, src], capture_output=True, text=True)
            if r.returncode != 0:                        # profiling helpers only: report, do not fail the product build
                print(f"build_tools: {name} failed to compile (profiling scripts that need it will not run)\n{r.stderr}",
                      file=sys.stderr)
                continue
        outs.append(out)
    return outs


if __name__ == "__main__":
    force = "--force" in sys.argv
    print(build_hip(force, verbose="-v" in sys.argv))
    print(build_oracle(force))
    print(build_emu(force))
    print(build_emu_gain(force))
    print(build_emu_consts(force))
    print(build_emu_gain_consts(force))
    print(build_emu_reuse(force))
    print(build_emu_reuse(force, reuse=False))
    print(build_emu_step(force))
    print(build_emu_step(force, fused=False))
    print(build_emu_rbd(force))
    print(build_emu_rbd_inertial(force))
    print(build_emu_rbd_walk(force))
    print(build_emu_walk_measure(force))
    print(build_emu_walk_plant(force))
    print(build_device_unit(force))
    print(build_tools(force))

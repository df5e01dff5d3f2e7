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


def build_hip(force=False, verbose=False):
    src = os.path.join(PKG, "csrc", "cmpc_hip.hip")
    wbc = os.path.join(PKG, "csrc", "wbc_qp.hip")          # batched whole-body QP (include/cmpc_wbc.h), same library
    deps = [src, wbc, os.path.join(PKG, "csrc", "cmpc_kernel.hpp"), os.path.join(PKG, "csrc", "cmpc_lds_asm.hpp"), os.path.join(PKG, "csrc", "cmpc_wave.hpp"), os.path.join(PKG, "csrc", "cmpc_order_fit.h"),
            os.path.join(ROOT, "include", "cmpc.h"), os.path.join(ROOT, "include", "cmpc_wbc.h")]
    out = os.path.join(PKG, "libcmpc_amd.so")
    if force or _newer(out, deps):
        cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-o", out, src, wbc]
        if verbose:
            cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
        subprocess.check_call(cmd)
    return out


def build_hip_profile(force=False):
    """Diagnostic variant with in-kernel phase timers (tools/ only; never loaded by the package)."""
    src = os.path.join(PKG, "csrc", "cmpc_hip.hip")
    deps = [src, os.path.join(PKG, "csrc", "cmpc_kernel.hpp"), os.path.join(PKG, "csrc", "cmpc_lds_asm.hpp"), os.path.join(PKG, "csrc", "cmpc_wave.hpp"),
            os.path.join(ROOT, "include", "cmpc.h")]
    out = os.path.join(ROOT, "tools", "libcmpc_amd_prof.so")
    if force or _newer(out, deps):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                               "-DCMPC_PROFILE", "-o", out, src, os.path.join(PKG, "csrc", "wbc_qp.hip")])
    return out


def build_hip_dev(force=False):
    """Developer variant (tools/ only; never loaded by the package unless CMPC_LIB_PATH names it): -DCMPC_DEV_KNOBS compiles
    in the environment knobs of the occupancy / kernel-choice studies (CMPC_WG_PER_CU, CMPC_PAIR, CMPC_PAIR_PER_CU), which
    the shipped library does not read."""
    src = os.path.join(PKG, "csrc", "cmpc_hip.hip")
    deps = [src, os.path.join(PKG, "csrc", "cmpc_kernel.hpp"), os.path.join(PKG, "csrc", "cmpc_lds_asm.hpp"), os.path.join(PKG, "csrc", "cmpc_wave.hpp"),
            os.path.join(ROOT, "include", "cmpc.h")]
    out = os.path.join(ROOT, "tools", "libcmpc_amd_dev.so")
    if force or _newer(out, deps):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                               "-DCMPC_DEV_KNOBS", "-o", out, src, os.path.join(PKG, "csrc", "wbc_qp.hip")])
    return out


def build_oracle(force=False):
    out = os.path.join(ROOT, "oracle", "libcmpc_oracle.so")
    deps = [os.path.join(ROOT, "oracle", "cmpc_oracle.c"), os.path.join(ROOT, "include", "cmpc.h")]
    if force or _newer(out, deps):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-B", "libcmpc_oracle.so"],
                              stdout=subprocess.DEVNULL)
    return out


def build_emu(force=False):
    src = os.path.join(ROOT, "tests", "emu", "cmpc_emu.cpp")
    out = os.path.join(ROOT, "tests", "emu", "libcmpc_emu.so")
    deps = [src, os.path.join(PKG, "csrc", "cmpc_kernel.hpp"), os.path.join(PKG, "csrc", "cmpc_lds_asm.hpp"), os.path.join(PKG, "csrc", "cmpc_wave.hpp"),
            os.path.join(ROOT, "include", "cmpc.h")]
    if force or _newer(out, deps):
        # (-mfma -ffp-contract=off: the kernel's explicit CMPC_FMA are single instructions, and nothing else is fused)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-o", out, src])
    return out


def build_emu_gain(force=False):
    """Host emulation of the gain variant of the solver (tests/emu/cmpc_emu_gain.cpp): test harness only."""
    src = os.path.join(ROOT, "tests", "emu", "cmpc_emu_gain.cpp")
    out = os.path.join(ROOT, "tests", "emu", "libcmpc_emu_gain.so")
    deps = [src, os.path.join(ROOT, "tests", "emu", "cmpc_emu.cpp"), os.path.join(PKG, "csrc", "cmpc_kernel.hpp"),
            os.path.join(PKG, "csrc", "cmpc_lds_asm.hpp"), os.path.join(PKG, "csrc", "cmpc_wave.hpp"),
            os.path.join(ROOT, "include", "cmpc.h")]
    if force or _newer(out, deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-o", out, src])
    return out


def build_emu_consts(force=False):
    """Host emulation of the solver with per-instance constants (tests/emu/cmpc_emu_consts.cpp): test harness only."""
    src = os.path.join(ROOT, "tests", "emu", "cmpc_emu_consts.cpp")
    out = os.path.join(ROOT, "tests", "emu", "libcmpc_emu_consts.so")
    deps = [src, os.path.join(ROOT, "tests", "emu", "cmpc_emu.cpp"), os.path.join(PKG, "csrc", "cmpc_kernel.hpp"),
            os.path.join(PKG, "csrc", "cmpc_lds_asm.hpp"), os.path.join(PKG, "csrc", "cmpc_wave.hpp"),
            os.path.join(ROOT, "include", "cmpc.h")]
    if force or _newer(out, deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-o", out, src])
    return out


def build_emu_reuse(force=False, reuse=True):
    """Host emulation with counters on the retried factorisations (tests/emu/cmpc_emu_reuse.cpp): test harness only.
    reuse=False builds the kernel source with -DCMPC_NO_EVAL_REUSE, the path that evaluates every stage of a retry pass again."""
    src = os.path.join(ROOT, "tests", "emu", "cmpc_emu_reuse.cpp")
    out = os.path.join(ROOT, "tests", "emu", "libcmpc_emu_reuse.so" if reuse else "libcmpc_emu_noreuse.so")
    deps = [src, os.path.join(ROOT, "tests", "emu", "cmpc_emu.cpp"), os.path.join(PKG, "csrc", "cmpc_kernel.hpp"),
            os.path.join(PKG, "csrc", "cmpc_lds_asm.hpp"), os.path.join(PKG, "csrc", "cmpc_wave.hpp"),
            os.path.join(ROOT, "include", "cmpc.h")]
    if force or _newer(out, deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-pthread"]
                              + ([] if reuse else ["-DCMPC_NO_EVAL_REUSE"]) + ["-o", out, src])
    return out


def build_hip_no_reuse(force=False, profile=False):
    """Diagnostic variant (tools/ only; loaded through CMPC_LIB_PATH): -DCMPC_NO_EVAL_REUSE, the one-wave 4-vertex kernel that
    evaluates every stage of a retry pass again -- the third leg of the A/B runs, and with profile=True the `before` of
    tools/phase_profile.py's retry figures."""
    src = os.path.join(PKG, "csrc", "cmpc_hip.hip")
    deps = [src, os.path.join(PKG, "csrc", "cmpc_kernel.hpp"), os.path.join(PKG, "csrc", "cmpc_lds_asm.hpp"), os.path.join(PKG, "csrc", "cmpc_wave.hpp"),
            os.path.join(ROOT, "include", "cmpc.h")]
    out = os.path.join(ROOT, "tools", "libcmpc_amd_noreuse_prof.so" if profile else "libcmpc_amd_noreuse.so")
    if force or _newer(out, deps):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-DCMPC_NO_EVAL_REUSE"]
                              + (["-DCMPC_PROFILE"] if profile else []) + ["-o", out, src, os.path.join(PKG, "csrc", "wbc_qp.hip")])
    return out


def build_device_unit(force=False):
    """GPU-tier unit harness for the device-only primitives (tests/gpu_unit): never loaded by the package."""
    src = os.path.join(ROOT, "tests", "gpu_unit", "cmpc_device_unit.hip")
    out = os.path.join(ROOT, "tests", "gpu_unit", "libcmpc_device_unit.so")
    deps = [src, os.path.join(PKG, "csrc", "cmpc_kernel.hpp"), os.path.join(PKG, "csrc", "cmpc_lds_asm.hpp"), os.path.join(PKG, "csrc", "cmpc_wave.hpp")]
    if force or _newer(out, deps):
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
    print(build_emu_reuse(force))
    print(build_emu_reuse(force, reuse=False))
    print(build_device_unit(force))
    print(build_tools(force))

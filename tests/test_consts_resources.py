"""CPU tier: resources and ISA of the kernels with per-instance constants (cross-compiled for gfx950, as
tests/test_gain_resources.py does): same LDS as the default kernels, no scratch, the default and gain kernels where they
were, and the row of constants arriving through SCALAR loads."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "online-non-linear-centroidal-mpc-with-stability-guarantees-for-robust-locomotion-of-legged-robots-_amd")

PAIRS = [("cmpc_solve_consts_kernel<4, 1>", "cmpc_solve_kernel<4, 1>"),
         ("cmpc_solve_pair_consts_kernel<4, 2>", "cmpc_solve_pair_kernel<4, 2>"),
         ("cmpc_solve_consts_kernel<8, 2>", "cmpc_solve_kernel<8, 2>")]


def _demangle(name):
    cur = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    return re.sub(r"\(anonymous namespace\)::|\(.*|^void ", "", cur)


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    """(resources, isa): the resource remarks and the instruction text of every kernel of csrc/cmpc_hip.hip."""
    asm = str(tmp_path_factory.mktemp("consts_isa") / "cmpc_hip.s")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", asm, os.path.join(PKG, "csrc", "cmpc_hip.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = _demangle(m.group(1))
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur:
            res[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    isa = {}
    text = open(asm).read()
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        body = [re.sub(r"\s*;.*", "", ln).strip() for ln in m.group(2).splitlines()]
        isa[_demangle(m.group(1))] = [ln for ln in body if ln and not ln.startswith((".", ";"))]
    return res, isa


def _count(lines, prefix):
    return sum(1 for ln in lines if ln.startswith(prefix))


@pytest.mark.parametrize("consts,plain", PAIRS)
def test_consts_kernels_exist_with_the_default_lds_and_no_scratch(build, consts, plain):
    res, _ = build
    assert consts in res and plain in res, sorted(res)
    print(consts, res[consts], "|", plain, res[plain])
    assert res[consts]["LDS Size"] == res[plain]["LDS Size"]           # the feature uses no LDS
    assert res[consts]["VGPRs"] <= 256
    # the final build: no scratch in any of the three (the default kernels: 0 / 12 / 0 bytes per lane)
    assert res[consts]["ScratchSize"] == 0


def test_default_and_gain_kernels_keep_their_resource_lines(build):
    res, _ = build
    want = {"cmpc_solve_kernel<4, 1>": dict(VGPRs=256, AGPRs=0, ScratchSize=0, LDS=22936),
            "cmpc_solve_pair_kernel<4, 2>": dict(VGPRs=256, AGPRs=0, ScratchSize=12, LDS=53672),
            "cmpc_solve_kernel<8, 2>": dict(VGPRs=256, AGPRs=203, ScratchSize=0, LDS=59944),
            "cmpc_solve_gain_kernel<4, 1>": dict(VGPRs=256, AGPRs=0, ScratchSize=288, LDS=22936),
            "cmpc_solve_pair_gain_kernel<4, 2>": dict(VGPRs=256, AGPRs=0, ScratchSize=240, LDS=53672),
            "cmpc_solve_gain_kernel<8, 2>": dict(VGPRs=256, AGPRs=220, ScratchSize=176, LDS=59944)}
    for k, v in want.items():
        got = dict(res[k], LDS=res[k]["LDS Size"])
        for f, x in v.items():
            assert got[f] == x, (k, f, res[k])


@pytest.mark.parametrize("consts,plain", PAIRS)
def test_the_row_arrives_through_scalar_loads(build, consts, plain):
    """The constants of the default kernels are kernel arguments (scalar loads of the argument segment); the new kernels
    read the eighteen of the row from memory instead.  Read by scalar loads, that shows as MORE s_load instructions and
    not one more vector load from global memory; read through vector loads it would be the other way round."""
    _, isa = build
    a, b = isa[consts], isa[plain]
    s_a, s_b = _count(a, "s_load_"), _count(b, "s_load_")
    g_a, g_b = _count(a, "global_load_") + _count(a, "flat_load_") + _count(a, "buffer_load_"), \
        _count(b, "global_load_") + _count(b, "flat_load_") + _count(b, "buffer_load_")
    print(f"{consts}: s_load {s_a} (default {s_b}), vector loads from memory {g_a} (default {g_b}), "
          f"scratch {_count(a, 'scratch_')} (default {_count(b, 'scratch_')})")
    assert s_a >= s_b + 18, (s_a, s_b)                 # at least one load per entry of the row on top of the default's
    assert g_a <= g_b, (g_a, g_b)

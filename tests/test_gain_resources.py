"""CPU tier: resources of the gain kernels (cross-compiled ISA, as tests/test_capi.py does): each gain kernel's LDS is at
most its default kernel's, so that residency per CU stays the same."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "online-non-linear-centroidal-mpc-with-stability-guarantees-for-robust-locomotion-of-legged-robots-_amd")


@pytest.fixture(scope="module")
def resources():
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, os.path.join(PKG, "csrc", "cmpc_hip.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            cur = re.sub(r"\(anonymous namespace\)::|\(.*|^void ", "", cur)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur:
            res[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return res


@pytest.mark.parametrize("gain,plain", [("cmpc_solve_gain_kernel<4, 1>", "cmpc_solve_kernel<4, 1>"),
                                        ("cmpc_solve_pair_gain_kernel<4, 2>", "cmpc_solve_pair_kernel<4, 2>"),
                                        ("cmpc_solve_gain_kernel<8, 2>", "cmpc_solve_kernel<8, 2>")])
def test_gain_kernel_lds_within_default(resources, gain, plain):
    assert gain in resources and plain in resources, sorted(resources)
    print(gain, resources[gain], plain, resources[plain])
    assert resources[gain]["LDS Size"] <= resources[plain]["LDS Size"]


def test_default_kernels_resources_unchanged(resources):
    # the resource lines of the default kernels as they were before the gain variants existed
    want = {"cmpc_solve_kernel<4, 1>": dict(VGPRs=256, AGPRs=0, ScratchSize=0),
            "cmpc_solve_pair_kernel<4, 2>": dict(VGPRs=256, AGPRs=0, ScratchSize=12),
            "cmpc_solve_kernel<8, 2>": dict(VGPRs=256, AGPRs=203, ScratchSize=0)}
    lds = {"cmpc_solve_kernel<4, 1>": 22936, "cmpc_solve_pair_kernel<4, 2>": 53672, "cmpc_solve_kernel<8, 2>": 59944}
    for k, v in want.items():
        for f, x in v.items():
            assert resources[k][f] == x, (k, f, resources[k])
        assert resources[k]["LDS Size"] == lds[k]

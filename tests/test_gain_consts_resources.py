"""CPU tier: resources of the kernels with a gain AND per-instance constants, and of the gain-tracking kernel (cross-compiled
for gfx950, as tests/test_gain_resources.py does): the LDS of the default kernels, so that residency per CU is unchanged; the
256 registers of two waves per SIMD; the scratch of each pinned at what this build reports (DESIGN.md section 5 quotes it next
to the gain kernels' 288 / 240 / 176 bytes); no scratch and no spill in the tracking kernel."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "online-non-linear-centroidal-mpc-with-stability-guarantees-for-robust-locomotion-of-legged-robots-_amd")

#: kernel -> (LDS bytes per workgroup = the default kernel's, scratch bytes per lane of this build)
WANT = {"cmpc_solve_gain_consts_kernel<4, 1>": (22936, 192),
        "cmpc_solve_pair_gain_consts_kernel<4, 2>": (53672, 176),
        "cmpc_solve_gain_consts_kernel<8, 2>": (59944, 176)}
FIELDS = r"VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|SGPRs Spill|VGPRs Spill"


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
        m = re.search(r"remark:\s+(" + FIELDS + r"): (\d+)", ln)
        if m and cur:
            res[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    return res


@pytest.mark.parametrize("kernel", sorted(WANT))
def test_gain_consts_kernels_keep_the_default_lds_and_their_pinned_scratch(resources, kernel):
    assert kernel in resources, sorted(resources)
    print(kernel, resources[kernel])
    lds, scratch = WANT[kernel]
    plain = kernel.replace("_gain_consts", "")
    assert resources[kernel]["LDS Size"] == lds == resources[plain]["LDS Size"]
    assert resources[kernel]["VGPRs"] <= 256
    assert resources[kernel]["ScratchSize"] == scratch


@pytest.mark.parametrize("kernel", ["cmpc_gain_track_kernel<4>", "cmpc_gain_track_kernel<8>"])
def test_track_kernel_has_no_scratch_and_no_spill(resources, kernel):
    assert kernel in resources, sorted(resources)
    print(kernel, resources[kernel])
    r = resources[kernel]
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0

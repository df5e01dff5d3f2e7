"""Resources of the contact plant's kernel (csrc/walk_plant.hip), read from hipcc's remarks of a cross-compile for gfx950 as
tests/test_rbd_resources.py reads the model's: one kernel in the unit, no scratch and no spilled vector register, the LDS the
harness reports, and six robots per CU by the rule of that file."""
import os
import re
import subprocess

import rbd_common as rc
import walk_plant_common as pc

#: what the kernel has (hipcc's remarks for gfx950)
VGPRS, LDS_BYTES = 255, 24712


def test_the_unit_has_one_kernel_with_no_scratch_the_lds_the_harness_reports_and_six_robots_per_cu():
    pkg = os.path.join(rc.ROOT, "online-non-linear-centroidal-mpc-with-stability-guarantees-for-robust-locomotion-of-legged-robots-_amd")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, os.path.join(pkg, "csrc", "walk_plant.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, cur = {}, None
    for ln in r.stderr.splitlines():                     # (the remarks only)
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|VGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and cur:
            res[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    print(res)
    assert len(res) == 1 and "walk_plant_kernel" in next(iter(res)), sorted(res)
    (one,) = res.values()
    lib = pc.emu_lib()
    assert one["ScratchSize"] == 0 and one["VGPRs Spill"] == 0
    assert one["LDS Size"] == lib.cmpc_emu_walk_plant_lds_bytes() == LDS_BYTES
    assert lib.cmpc_emu_walk_plant_per_cu() == 6
    assert 6 * -(-(one["LDS Size"] + 64) // 1280) * 1280 <= 160 * 1024
    assert one["VGPRs"] == VGPRS and one["AGPRs"] == 0

"""CPU tier, cross-compiled ISA: the reuse path of a retried factorisation in the plain and the per-instance-constants
one-wave 4-vertex kernels.  No scratch instruction inside a stage loop (loop depth read as tests/test_capi.py reads it: the
stage loops are at depth 4 and deeper), no scratch at all, and the reuse path's global loads are there: the kernels built
with -DCMPC_NO_EVAL_REUSE have fewer load instructions, by at most the nine words a lane reloads and by no fewer than seven (the compiler may merge
two neighbouring words into one load or serve one from a load the stage issues anyway; a reload dropped altogether shows)."""
import os
import re
import subprocess

import pytest

import build as _b

KERNELS = {"plain": "cmpc_solve_kernelILi4ELi1EEEvN4cmpc5KArgsEPiPKi", "consts": "cmpc_solve_consts_kernelILi4ELi1EEEvN4cmpc5KArgsEPKdPiPKi"}
RELOADS = 9          # dense rows (3), b, R'v_j with the yaw curvatures and pi, Lyapunov gradient, sigma, h0, h1: eval_stage


def _isa(tmp_path_factory, flags):
    out = tmp_path_factory.mktemp("isa") / "cmpc.s"
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", *flags, "-o", str(out),
                           os.path.join(_b.PKG, "csrc", "cmpc_hip.hip")])
    return out.read_text()


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return _isa(tmp_path_factory, []), _isa(tmp_path_factory, ["-DCMPC_NO_EVAL_REUSE"])


def _body(isa, mangled):
    name = next(m for m in re.findall(r"^(\S*" + mangled + r"):", isa, flags=re.M))
    body = isa[isa.index(name + ":"):]
    return body[:body.index("s_endpgm")]


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_no_scratch_in_the_stage_loops_and_the_reloads_are_there(isa, which):
    new, old = (_body(x, KERNELS[which]) for x in isa)
    depth, at = 0, []
    for ln in new.splitlines():
        m = re.match(r"^\.LBB\d+_\d+:(.*)$", ln)
        if m:
            d = re.search(r"Depth=(\d+)", m.group(1))
            depth = int(d.group(1)) if d else 0
        elif "This Inner Loop Header: Depth=" in ln or "This Loop Header: Depth=" in ln:
            depth = int(re.search(r"Depth=(\d+)", ln).group(1))
        elif ln.strip().startswith("scratch_"):
            at.append(depth)
    print(which, "scratch instructions at loop depths", at)
    assert not [d for d in at if d > 3], at                             # none inside a stage loop
    assert not at                                                       # (and none at all: the kernels' resource lines say 0)
    n_new, n_old = (sum(ln.strip().startswith("global_load") for ln in b.splitlines()) for b in (new, old))
    print(which, "global loads", n_new, "without the reuse path", n_old)
    assert RELOADS - 2 <= n_new - n_old <= RELOADS

"""What gains for per-instance constants cost, and what applying a gain in one launch saves.

Solver legs: randomized N = 20, cold start, B = 8192 and 65 536, ms per launch (HIP events, median of K launches after W
warm-up launches each).  The PARENT commit's cmpc_solve_batch_gain against this tree's gain launch (the same instructions) and
this tree's gain-consts launch with uniform rows (the same work: the tool asserts identical iteration counts); this tree's
plain and consts launches in the same session give the yardstick, the ratio consts : plain.

The parent's tree is checked out and built somewhere else first, e.g.
    mkdir /tmp/parent && git archive HEAD~1 | tar -x -C /tmp/parent && (cd /tmp/parent && python build.py)
and named with --parent-tree.  Every leg runs in a fresh child process (a library is chosen when the package is first
imported): the parent's gain launch first and last (the difference between the two is the run-to-run spread a difference has
to exceed), this tree's legs alternated in between.

Track leg: B = 65 536, nu = 32, a finite G, columns = 0xFFF: cmpc_gain_track against the three-launch torch expression of
INTEGRATION.md section 3a on the same tensors (torch events around R launches back to back, so that the queue is never empty
and the host's launch cost is not in the figure; per launch, median of K), and the kernel's bytes per second over its
algorithmic traffic -- per instance it reads G, x0, x_meas, x_1, u_0 and writes x1_out, u0_out, used.

--legs track measures the track leg alone and replaces that entry of an existing --out file.

usage: python tools/gain_consts_cost.py --parent-tree DIR [--steps K] [--warmup W] [--sizes 8192,65536] [--legs solver,track]
                                        [--out profiles/gain_consts_cost.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_NAME = "online-non-linear-centroidal-mpc-with-stability-guarantees-for-robust-locomotion-of-legged-robots-_amd"

# the measuring child: the parent's tree runs the gain leg only
CHILD = r"""
import json, sys
import numpy as np, torch
tree, leg, sizes, steps, warmup = sys.argv[1], sys.argv[2], [int(x) for x in sys.argv[3].split(",")], int(sys.argv[4]), int(sys.argv[5])
sys.path.insert(0, tree)
import cmpc_amd
from cmpc_amd import capi, workloads as wl
from cmpc_amd.solver import BatchedCentroidalMPC
res = dict(lib=capi.LIB_PATH, sizes={})
for B in sizes:
    spec, rec = wl.make_workload("randomized", B=B, N=20)
    s = BatchedCentroidalMPC(spec, device="cuda:0")
    r = torch.from_numpy(rec).to("cuda:0")
    rows = torch.from_numpy(np.ascontiguousarray(np.tile(spec.consts_row(), (B, 1)))).to("cuda:0") if "consts" in leg else None
    G = torch.empty((B, 20 + spec.nu, 20), dtype=torch.float64, device="cuda:0") if "gain" in leg else None
    ms = []
    for i in range(warmup + steps):
        if leg == "plain":
            o = s.solve(r)
        elif leg == "consts":
            o = s.solve_with_consts(r, rows)
        elif leg == "gain":
            o = s.solve_with_gain(r, gain=G)
        else:
            o = s.solve_with_gain(r, gain=G, consts=rows)
        t = s.last_kernel_ms()
        if i >= warmup:
            ms.append(t)
    st = o[1].cpu().numpy()
    res["sizes"][str(B)] = dict(ms=float(np.median(ms)), all_ms=[round(x, 3) for x in ms], kernel=s.last_kernel_name(),
                                usable=int(np.isin(st, (0, 3)).sum()), iters=int(o[2].sum().item()),
                                gains=None if G is None else int(torch.isfinite(G).all(dim=2).all(dim=1).sum().item()))
    s.close()
print("RESULT " + json.dumps(res))
"""

TRACK = r"""
import json, sys
import numpy as np, torch
tree, B, steps, warmup, reps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
sys.path.insert(0, tree)
import cmpc_amd
from cmpc_amd.problem import ProblemSpec
from cmpc_amd.solver import BatchedCentroidalMPC
dev, N = "cuda:0", 20
spec = ProblemSpec(N=N, nv=4)
nu = spec.nu
s = BatchedCentroidalMPC(spec, device=dev)
g = torch.Generator(device=dev).manual_seed(7)
rec = torch.randn((B, spec.nrec), dtype=torch.float64, device=dev, generator=g)
XU = torch.randn((B, spec.nsol), dtype=torch.float64, device=dev, generator=g)
G = torch.randn((B, 20 + nu, 20), dtype=torch.float64, device=dev, generator=g)
xm = (rec[:, :20] + 0.05 * torch.randn((B, 20), dtype=torch.float64, device=dev, generator=g)).contiguous()
x1o, u0o = torch.empty((B, 20), dtype=torch.float64, device=dev), torch.empty((B, nu), dtype=torch.float64, device=dev)
x0, u0, Gu = rec[:, :20], XU[:, 20 * (N + 1):20 * (N + 1) + nu], G[:, 20:, :]

def kernel():
    return s.track(rec, XU, G, xm, columns=0xFFF, x1_out=x1o, u0_out=u0o)

def expression():                                                  # INTEGRATION.md section 3a, as it stood: u only
    ok = torch.isfinite(G).all(dim=2).all(dim=1)
    return u0 + torch.where(ok[:, None], (Gu @ (xm - x0)[:, :, None])[:, :, 0], torch.zeros_like(u0))

def timed(f):
    ms = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            f()
        b.record(); b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b) / reps)
    return float(np.median(ms)), [round(x, 4) for x in ms]

k_ms, k_all = timed(kernel)
e_ms, e_all = timed(expression)
k2_ms, k2_all = timed(kernel)
dx = torch.zeros_like(xm); dx[:, :12] = (xm - x0)[:, :12]
u_ref = u0 + (Gu @ dx[:, :, None])[:, :, 0]
err = float((u0o - u_ref).abs().max().item())
bytes_per = 8 * ((20 + nu) * 20 + 20 + 20 + 20 + nu + 20 + nu) + 1   # reads G, x0, x_meas, x_1, u_0; writes x1_out, u0_out, used
print("RESULT " + json.dumps(dict(B=B, nu=nu, launches_per_sample=reps, kernel_ms=min(k_ms, k2_ms), kernel_first_ms=k_ms, kernel_last_ms=k2_ms, torch_ms=e_ms,
                                  kernel_all_ms=k_all + k2_all, torch_all_ms=e_all, bytes_per_instance=bytes_per,
                                  kernel_bytes_per_s=B * bytes_per / (min(k_ms, k2_ms) * 1e-3), max_abs_diff_u=err,
                                  note="torch_ms: isfinite(G).all, bmm over the u rows, where -- u only, as INTEGRATION.md 3a had it; "
                                       "kernel_ms: x_1 and u_0 both")))
"""


def run_child(code, tree, args, timeout):
    env = dict(os.environ, CMPC_LIB_PATH=os.path.join(tree, PKG_NAME, "libcmpc_amd.so"))
    r = subprocess.run([sys.executable, "-c", code, tree] + [str(x) for x in args], env=env, cwd=tree, capture_output=True, text=True,
                       timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"child {args} in {tree} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", required=True, help="checkout of the parent commit with its library built")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="8192,65536")
    ap.add_argument("--track-batch", type=int, default=65536)
    ap.add_argument("--track-reps", type=int, default=20, help="launches back to back per timed sample of the track leg")
    ap.add_argument("--legs", default="solver,track")
    ap.add_argument("--leg-timeout", type=int, default=280)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.steps < 5:
        raise SystemExit("--steps: the median of at least five launches per leg")
    parent = os.path.abspath(a.parent_tree)
    if not os.path.exists(os.path.join(parent, PKG_NAME, "libcmpc_amd.so")):
        raise SystemExit(f"{parent}: no built library (python build.py in that tree first)")
    legs = [("parent_first", parent, "gain"), ("gain", ROOT, "gain"), ("plain", ROOT, "plain"), ("gain_consts", ROOT, "gain_consts"),
            ("consts", ROOT, "consts"), ("parent_last", parent, "gain")]
    got = {}
    for name, tree, leg in (legs if "solver" in a.legs else []):
        got[name] = run_child(CHILD, tree, [leg, a.sizes, a.steps, a.warmup], a.leg_timeout)
        print(name, json.dumps(got[name]), flush=True)
    rows = []
    for B in (a.sizes.split(",") if "solver" in a.legs else []):
        p0, p1 = got["parent_first"]["sizes"][B], got["parent_last"]["sizes"][B]
        ga, gc, pl, co = (got[k]["sizes"][B] for k in ("gain", "gain_consts", "plain", "consts"))
        # the same work in every leg: uniform rows, and the gain is taken after the verdict
        assert p0["iters"] == p1["iters"] == ga["iters"] == gc["iters"] == pl["iters"] == co["iters"], (B, "iteration counts differ")
        assert p0["usable"] == ga["usable"] == gc["usable"] and p0["gains"] == ga["gains"] == gc["gains"], (B, "verdicts differ")
        parent_ms = 0.5 * (p0["ms"] + p1["ms"])
        every = p0["all_ms"] + p1["all_ms"]
        rows.append(dict(B=int(B), parent_gain_ms=parent_ms, parent_first_ms=p0["ms"], parent_last_ms=p1["ms"],
                         parent_spread=abs(p0["ms"] - p1["ms"]) / parent_ms,                  # between two runs of the same code
                         parent_launch_spread=(max(every) - min(every)) / parent_ms,         # between its single launches
                         gain_ms=ga["ms"], gain_consts_ms=gc["ms"], plain_ms=pl["ms"], consts_ms=co["ms"],
                         gain_vs_parent=ga["ms"] / parent_ms - 1.0, gain_consts_vs_parent=gc["ms"] / parent_ms - 1.0,
                         gain_consts_vs_gain=gc["ms"] / ga["ms"] - 1.0, consts_vs_plain=co["ms"] / pl["ms"] - 1.0,
                         parent_kernel=p0["kernel"], gain_kernel=ga["kernel"], gain_consts_kernel=gc["kernel"],
                         iters=p0["iters"], usable=p0["usable"], gains=p0["gains"],
                         launches=dict(parent_first=p0["all_ms"], gain=ga["all_ms"], plain=pl["all_ms"], gain_consts=gc["all_ms"],
                                       consts=co["all_ms"], parent_last=p1["all_ms"])))
        print(json.dumps(rows[-1]), flush=True)
    doc = dict(workload="randomized N=20 cold, uniform rows", steps=a.steps, warmup=a.warmup, rows=rows)
    if "solver" not in a.legs and a.out and os.path.exists(a.out):
        doc = json.load(open(a.out))
    if "track" in a.legs:
        doc["track"] = run_child(TRACK, ROOT, [a.track_batch, a.steps, a.warmup, a.track_reps], a.leg_timeout)
        print("track", json.dumps(doc["track"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()

"""What per-instance constants cost: launches of cmpc_solve_batch_consts with uniform rows (the work is identical) against
the plain launch of the PARENT commit's library, on the benchmark's workload (randomized, N = 20, cold start), B = 8192 and
65 536, ms per launch (HIP events, median of K launches after W warm-up launches each).

The parent's tree is checked out and built somewhere else first, e.g.
    mkdir /tmp/parent && git archive HEAD~1 | tar -x -C /tmp/parent && (cd /tmp/parent && python build.py)
and named with --parent-tree.  Every leg runs in a fresh child process (a library is chosen when the package is first
imported): the parent's package with the parent's library twice (first and last: the difference between the two is the
run-to-run spread a difference has to exceed), this tree's plain launch and this tree's consts launch in between.

usage: python tools/consts_cost.py --parent-tree DIR [--steps K] [--warmup W] [--sizes 8192,65536] [--out profiles/consts_cost.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_NAME = "online-non-linear-centroidal-mpc-with-stability-guarantees-for-robust-locomotion-of-legged-robots-_amd"

# the measuring child: only calls both trees have, except for the consts leg
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
    rows = torch.from_numpy(np.ascontiguousarray(np.tile(spec.consts_row(), (B, 1)))).to("cuda:0") if leg == "consts" else None
    ms = []
    for i in range(warmup + steps):
        o = s.solve_with_consts(r, rows) if leg == "consts" else s.solve(r)
        t = s.last_kernel_ms()
        if i >= warmup:
            ms.append(t)
    st = o[1].cpu().numpy()
    res["sizes"][str(B)] = dict(ms=float(np.median(ms)), all_ms=[round(x, 3) for x in ms], kernel=s.last_kernel_name(),
                                usable=int(np.isin(st, (0, 3)).sum()), iters=int(o[2].sum().item()))
    s.close()
print("RESULT " + json.dumps(res))
"""


def run_leg(tree, leg, a):
    env = dict(os.environ, CMPC_LIB_PATH=os.path.join(tree, PKG_NAME, "libcmpc_amd.so"))
    r = subprocess.run([sys.executable, "-c", CHILD, tree, leg, a.sizes, str(a.steps), str(a.warmup)], env=env, cwd=tree,
                       capture_output=True, text=True, timeout=a.leg_timeout)
    if r.returncode != 0:
        raise SystemExit(f"leg {leg} in {tree} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", required=True, help="checkout of the parent commit with its library built")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="8192,65536")
    ap.add_argument("--leg-timeout", type=int, default=280)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    parent = os.path.abspath(a.parent_tree)
    if not os.path.exists(os.path.join(parent, PKG_NAME, "libcmpc_amd.so")):
        raise SystemExit(f"{parent}: no built library (python build.py in that tree first)")
    legs = [("parent_first", parent, "plain"), ("plain", ROOT, "plain"), ("consts", ROOT, "consts"), ("parent_last", parent, "plain")]
    got = {}
    for name, tree, leg in legs:
        got[name] = run_leg(tree, leg, a)
        print(name, json.dumps(got[name]), flush=True)
    rows = []
    for B in a.sizes.split(","):
        p0, p1 = got["parent_first"]["sizes"][B], got["parent_last"]["sizes"][B]
        pl, co = got["plain"]["sizes"][B], got["consts"]["sizes"][B]
        parent_ms = 0.5 * (p0["ms"] + p1["ms"])
        every = p0["all_ms"] + p1["all_ms"]
        rows.append(dict(B=int(B), parent_ms=parent_ms, parent_first_ms=p0["ms"], parent_last_ms=p1["ms"],
                         parent_spread=abs(p0["ms"] - p1["ms"]) / parent_ms,                   # between two runs of the same code
                         parent_launch_spread=(max(every) - min(every)) / parent_ms,          # between its single launches
                         plain_ms=pl["ms"], consts_ms=co["ms"], consts_vs_parent=co["ms"] / parent_ms - 1.0,
                         plain_vs_parent=pl["ms"] / parent_ms - 1.0, parent_kernel=p0["kernel"], consts_kernel=co["kernel"],
                         same_work=(p0["iters"] == co["iters"] and p0["usable"] == co["usable"]),
                         launches=dict(parent_first=p0["all_ms"], plain=pl["all_ms"], consts=co["all_ms"], parent_last=p1["all_ms"])))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(workload="randomized N=20 cold, uniform rows", steps=a.steps, warmup=a.warmup, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()

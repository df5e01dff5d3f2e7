"""What a scene set costs per closed-loop tick: `BatchedRollout` on one `Scene` (builder, solve, some thirty torch launches
for the back half) against the set-based rollout (`cmpc_build_records_scenes`, the same solve, `cmpc_rollout_advance`) with
S = 1 (the shipped walk: the same solves, so the difference is builder plus back half) and with S = 5 (the five walks of the
scene-set tests dealt round robin: other solves, so its figure stands beside its own iteration count).  One MI355X,
B = 4096, N = 10, perturbed initial states and per-instance momentum offsets from t0 = 150 (tools/walk_demo.py, leg b),
K ticks timed after W, ms per tick = host clock around the K ticks between two device synchronisations.

The single-scene leg runs the PARENT commit when its tree is named (checked out and built somewhere else first, e.g.
    mkdir /tmp/parent && git archive HEAD~1 | tar -x -C /tmp/parent && (cd /tmp/parent && python build.py)
); without --parent-tree it runs this tree's single-scene path, which is the parent's code.  Every run is a fresh child
process; the three legs are alternated R times in one session, the figure of a leg is the median of its R runs, and the
parent's own run-to-run spread (max - min over its R runs) is what a difference has to exceed.

usage: python tools/scenes_cost.py [--parent-tree DIR] [--batch 4096] [--ticks 300] [--warmup 20] [--runs 5] [--out profiles/scenes_cost.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_NAME = "online-non-linear-centroidal-mpc-with-stability-guarantees-for-robust-locomotion-of-legged-robots-_amd"

CHILD = r"""
import json, sys, time
import numpy as np, torch
tree, leg, B, ticks, warmup, hw_path = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[6]
sys.path.insert(0, tree)
import cmpc_amd
from cmpc_amd import capi, workloads as wl
from cmpc_amd.problem import ProblemSpec
from cmpc_amd.rollout import BatchedRollout
hw = np.loadtxt(hw_path)
spec, start = ProblemSpec(N=10), 150
rng = np.random.default_rng(7)
if leg == "single":
    sc = wl.scene()
    com, dcom = sc.nominal_state(np.full(B, start))
    kw = dict(hw_measured=hw)
else:
    walks = [(None, "rfoot"), ([(0.08, 0, 0)] * 10 + [(0, 0, 0)] * 3, "rfoot"), ([(0.1, 0.03, 0)] * 8 + [(0, 0, 0)] * 3, "rfoot"),
             ([(0.1, 0, 0.15)] * 12 + [(0, 0, 0)] * 3, "rfoot"), ([(0.12, 0, 0)] * 9 + [(0, 0, 0)] * 3, "lfoot")]
    scenes = []
    for vref, first in walks[:1 if leg == "set1" else 5]:
        p = wl.default_params(); p['first_swing'] = first
        scenes.append(wl.Scene(p, vref=vref))
    sc = wl.SceneSet(scenes)
    sid = (np.arange(B) % sc.S).astype(np.int32)
    com, dcom = sc.nominal_state(np.full(B, start), sid)
    kw = dict(scene_id=sid, hw_measured=[hw * np.array([-1.0, 1.0, -1.0]) if s.params['first_swing'] == 'lfoot' else hw for s in scenes])
com = com + rng.uniform(-0.003, 0.003, size=(B, 3)); dcom = dcom + rng.normal(0, 0.01, size=(B, 3))
ro = BatchedRollout(sc, spec, B, device="cuda:0", hw_offset=rng.normal(0, 0.05, size=(B, 3)), **kw)
ro.reset(start, com, dcom)
iters = 0
for i in range(warmup):
    ro.step()
torch.cuda.synchronize(); t0 = time.perf_counter()
for i in range(ticks):
    ro.step()
    iters = iters + ro.last_iters.sum()
torch.cuda.synchronize(); dt = time.perf_counter() - t0
print("RESULT " + json.dumps(dict(lib=capi.LIB_PATH, ms_per_tick=1e3 * dt / ticks, alive=int(ro.alive.sum().item()),
                                  mean_iters=float(iters.item()) / (ticks * B), kernel=ro.solver.last_kernel_name())))
"""


def run_leg(tree, leg, a):
    env = dict(os.environ, CMPC_LIB_PATH=os.path.join(tree, PKG_NAME, "libcmpc_amd.so"))
    hw = os.path.join(ROOT, "tests", "golden", "measured_hw_cuhw.txt")
    r = subprocess.run([sys.executable, "-c", CHILD, tree, leg, str(a.batch), str(a.ticks), str(a.warmup), hw], env=env, cwd=tree,
                       capture_output=True, text=True, timeout=a.leg_timeout)
    if r.returncode != 0:
        raise SystemExit(f"leg {leg} in {tree} failed ({r.returncode}):\n{r.stderr[-2000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default="", help="checkout of the parent commit with its library built")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--leg-timeout", type=int, default=170)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    parent = os.path.abspath(a.parent_tree) if a.parent_tree else ROOT
    if not os.path.exists(os.path.join(parent, PKG_NAME, "libcmpc_amd.so")):
        raise SystemExit(f"{parent}: no built library (python build.py in that tree first)")
    legs = [("parent", parent, "single"), ("set_S1", ROOT, "set1"), ("set_S5", ROOT, "set5")]
    runs = {name: [] for name, _, _ in legs}
    for r in range(a.runs):
        for name, tree, leg in legs:
            runs[name].append(run_leg(tree, leg, a))
            print(r, name, json.dumps(runs[name][-1]), flush=True)
    ms = {name: [x["ms_per_tick"] for x in v] for name, v in runs.items()}
    base = median(ms["parent"])
    res = dict(workload=f"closed loop, B = {a.batch}, N = 10, t0 = 150, {a.ticks} ticks after {a.warmup}", runs=a.runs,
               parent_is="the parent commit's tree" if a.parent_tree else "this tree's single-scene path (the parent's code)",
               parent_ms_per_tick=base, parent_spread_ms=max(ms["parent"]) - min(ms["parent"]),
               parent_spread=(max(ms["parent"]) - min(ms["parent"])) / base)
    for name in ("set_S1", "set_S5"):
        res[name + "_ms_per_tick"] = median(ms[name])
        res[name + "_vs_parent"] = median(ms[name]) / base - 1.0
    res["same_work_S1"] = all(x["mean_iters"] == runs["parent"][0]["mean_iters"] and x["alive"] == runs["parent"][0]["alive"]
                              for x in runs["set_S1"])
    res["legs"] = runs
    print(json.dumps({k: v for k, v in res.items() if k != "legs"}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

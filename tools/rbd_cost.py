"""What the batched rigid-body model costs: ms per launch of `BatchedRobot.evaluate` (HIP events, median of K launches after W
warm-up launches) at B = 8192 and 65 536 HRP-4 robots around the shipped initial configuration, the bytes the launch writes
and the resulting GB/s, and -- in the same session, on the launch's own outputs -- the `solve_tasks` launch it feeds (double
support, zero errors, -jdqd as feed-forward).  One session's numbers.

usage: python tools/rbd_cost.py [--steps K] [--warmup W] [--sizes 8192,65536] [--out profiles/rbd_cost.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
UNIQ, SEED = 1024, 20251019


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="8192,65536")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rbd_cost.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import cmpc_amd  # noqa: F401
    from cmpc_amd import rbd, wbc

    dev = "cuda:0"
    model = rbd.RobotModel.from_urdf(os.path.join(ROOT, "tests", "golden", "hrp4.urdf"))
    robot = rbd.BatchedRobot(model, device=dev)
    qp = wbc.BatchedInverseDynamicsQP(foot_size=0.1, mu=0.5, device=dev)
    sel = torch.from_numpy(model.joint_selection(rbd.HRP4_REDUNDANT_DOFS)).to(dev)
    rng = np.random.default_rng(SEED)
    q0 = model.place_on_ground(model.configuration(rbd.HRP4_INITIAL_DEG, degrees=True))
    qu = np.tile(q0, (UNIQ, 1))
    qu[:, 0:3] += rng.normal(scale=0.02, size=(UNIQ, 3))
    qu[:, 22:30] += rng.uniform(-0.2, 0.2, size=(UNIQ, 8))               # arms: the feet stay flat on the ground
    vu = rng.normal(scale=0.05, size=(UNIQ, 30))

    def timed(call):
        ms = []
        for i in range(args.warmup + args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = call()
            b.record()
            b.synchronize()
            if i >= args.warmup:
                ms.append(a.elapsed_time(b))
        return out, ms

    rows = []
    for B in (int(x) for x in args.sizes.split(",")):
        q = torch.from_numpy(np.ascontiguousarray(np.tile(qu, (B // UNIQ, 1)))).to(dev)
        v = torch.from_numpy(np.ascontiguousarray(np.tile(vu, (B // UNIQ, 1)))).to(dev)
        ev, ms = timed(lambda: robot.evaluate(q, v))
        written = sum(t.numel() * t.element_size() for t in ev)
        zeros = torch.zeros((B, 51), dtype=torch.float64, device=dev)
        ff = zeros.clone()
        ff[:, :21] = -ev.jdqd
        contact = torch.ones((B, 2), dtype=torch.float64, device=dev)
        out, qms = timed(lambda: qp.solve_tasks(ev.J, None, ff, zeros, zeros, None, ev.M, ev.h, contact, joint_selection=sel))
        st = out[3].cpu().numpy()
        med, qmed = statistics.median(ms), statistics.median(qms)
        rows.append(dict(B=B, evaluate_ms=med, bytes_written=written, write_GBps=written / med / 1e6,
                         us_per_robot=1e3 * med / B, solve_tasks_ms=qmed, solve_tasks_status0=int((st == 0).sum()),
                         evaluate_over_solve_tasks=med / qmed, launches=dict(evaluate=[round(x, 4) for x in ms],
                                                                              solve_tasks=[round(x, 4) for x in qms]),
                         finite=bool(all(torch.isfinite(t).all() for t in ev))))
        print(json.dumps(rows[-1]))
    res = dict(workload=f"HRP-4, {UNIQ} seeded instances around the initial configuration, tiled", steps=args.steps,
               warmup=args.warmup, rows=rows)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

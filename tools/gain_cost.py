"""What the first-stage gain costs: plain (cmpc_solve_batch_state) against gain launches (cmpc_solve_batch_gain) on the
benchmark's workload (randomized, N = 20, cold start), B = 8192 and 65 536, ms per launch (HIP events, median of K
launches after W warm-up launches each), and the share of status-0 / status-3 instances with a finite gain.
usage: python tools/gain_cost.py [--steps K] [--warmup W] [--out profiles/gain_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmpc_amd  # noqa: E402,F401
from cmpc_amd import workloads as wl  # noqa: E402
from cmpc_amd.solver import BatchedCentroidalMPC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="8192,65536")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    for B in [int(x) for x in a.sizes.split(",")]:
        spec, rec = wl.make_workload("randomized", B=B, N=20)
        s = BatchedCentroidalMPC(spec, device="cuda:0")
        r = torch.from_numpy(rec).to("cuda:0")
        res = {}
        for leg in ("plain", "gain"):
            ms = []
            for i in range(a.warmup + a.steps):
                o = s.solve(r) if leg == "plain" else s.solve_with_gain(r)
                t = s.last_kernel_ms()
                if i >= a.warmup:
                    ms.append(t)
            res[leg] = dict(ms=float(np.median(ms)), all_ms=[round(x, 3) for x in ms], kernel=s.last_kernel_name())
        st = o[1].cpu().numpy()
        fin = torch.isfinite(o[4]).all(dim=2).all(dim=1).cpu().numpy()
        row = dict(B=B, plain_ms=res["plain"]["ms"], gain_ms=res["gain"]["ms"],
                   overhead=res["gain"]["ms"] / res["plain"]["ms"] - 1.0,
                   plain_kernel=res["plain"]["kernel"], gain_kernel=res["gain"]["kernel"],
                   status0=int((st == 0).sum()), status0_finite=int(fin[st == 0].sum()),
                   status3=int((st == 3).sum()), status3_finite=int(fin[st == 3].sum()),
                   status12=int(((st == 1) | (st == 2)).sum()), launches=dict(plain=res["plain"]["all_ms"], gain=res["gain"]["all_ms"]))
        print(json.dumps(row), flush=True)
        rows.append(row)
        s.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(workload="randomized N=20 cold", steps=a.steps, warmup=a.warmup, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()

"""Status counts of the whole-body QP kernel over the parameter matrix of tests/test_wbc_qp.py: the three contact phases x
five (foot_size, mu) pairs, 1024 synthetic instances each (15 360 QPs).  Prints one JSON object; profiles/
wbc_pivot_floor.json holds the output of the library before and after the wrench-block pivot floor.

    python tools/wbc_status_counts.py [--seed 21] [--batch 1024] [--label NAME]

CMPC_LIB_PATH (capi.py) selects the build of the library."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cmpc_amd  # noqa: E402,F401
from cmpc_amd import wbc, workloads as wl  # noqa: E402

CONTACTS = ("ds", "lfoot", "rfoot")
FOOT_MU = ((0.1, 0.5), (0.1, 0.3), (0.1, 0.7), (0.2, 0.9), (0.04, 0.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a ROCm GPU")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    classes = []
    for contact in CONTACTS:
        mats = [dev(a) for a in wl.wbc_synthetic(args.batch, seed=args.seed, contact=contact)]
        for foot_size, mu in FOOT_MU:
            qp = wbc.BatchedInverseDynamicsQP(foot_size=foot_size, mu=mu, device="cuda:0")
            tau, qdd, f, st, it = qp.solve(*mats)
            torch.cuda.synchronize()
            st, it = st.cpu().numpy(), it.cpu().numpy()
            classes.append({"contact": contact, "foot_size": foot_size, "mu": mu,
                            "status": [int((st == s).sum()) for s in (0, 1, 2)],
                            "status2_instances": np.flatnonzero(st == 2).tolist(),
                            "status2_iters": it[st == 2].tolist(),
                            "mean_iterations": float(it.mean()), "max_iterations": int(it.max()),
                            "finite": bool(torch.isfinite(tau).all() and torch.isfinite(qdd).all() and torch.isfinite(f).all())})
    print(json.dumps({"label": args.label, "seed": args.seed, "batch": args.batch, "qps": args.batch * len(classes),
                      "status2_total": sum(c["status"][2] for c in classes),
                      "status1_total": sum(c["status"][1] for c in classes), "classes": classes}))


if __name__ == "__main__":
    main()

"""Developer script (CPU only): what a cheaper retry pass of the matrix sweep is worth to a launch.  The C oracle's iteration and
retry counts per instance (cmpc_oracle_solve_batch_stats: retries, wasted sweeps) are replayed through the shipped queue
order on 1792 slots, as tools/launch_model.py does, with cost per instance = 100 x iterations + w x wasted sweeps, for
w = 75 (a wasted sweep evaluated in full) down to 50.  About 80 s per seed on 16 cores.
usage: python tools/retry_reuse_model.py"""
import ctypes
import heapq
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import cmpc_amd  # noqa: F401
from cmpc_amd import workloads as wl, queue_order as qo
from oracle import oracle_lib as ol

B, SLOTS = 8192, 1792


def makespan(cost, order):
    """End of the launch when the instances are dealt in `order` to SLOTS slots, each to the slot that is free first."""
    free = [0] * SLOTS
    heapq.heapify(free)
    end = 0
    for i in order:
        t = heapq.heappop(free) + cost[i]
        end = max(end, t)
        heapq.heappush(free, t)
    return end


def main():
    lib = ol.lib()                               # (the oracle as the tests build it: oracle/Makefile, OpenMP)
    for seed in (None, 777, 31337):
        spec, rec = wl.make_workload("randomized", B=B, seed=seed)
        order = np.argsort(-qo.bucket_of(qo.predicted_iterations(rec, spec)), kind="stable")
        cs = ol.default_spec(N=spec.N, nv=spec.nv, tol=spec.tol, max_iter=spec.max_iter, k1=spec.k1, k2=spec.k2, prox=spec.prox,
                             acc_tol=spec.acc_tol)
        out = np.zeros((B, ol.nsol(cs)))
        st, it, nreg = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
        kkt, waste = np.zeros(B), np.zeros(B)
        t0 = time.time()
        lib.cmpc_oracle_solve_batch_stats(ctypes.byref(cs), B, ol._p(rec), None, ol._p(out), ol._p(st), ol._p(it), ol._p(kkt),
                                          ol._p(nreg), ol._p(waste), 0)
        iters = np.maximum(it.astype(np.int64), 1) * 100
        res = {}
        for w in (75, 60, 55, 50):
            cost = iters + np.round(w * waste).astype(np.int64)
            res[w] = (makespan(cost, order), cost.sum() / SLOTS)
        by_status = {s: (round(float(waste[st == s].mean()), 2), round(float(nreg[st == s].mean()), 2)) for s in (0, 2, 3) if (st == s).any()}
        print(f"seed {seed}: {time.time() - t0:.1f} s, retries / solve {nreg.mean():.2f}, wasted sweeps / solve {waste.mean():.2f}, "
              f"iterations {it.mean():.2f}, (wasted sweeps, retries) by status {by_status}")
        for w, (m, bal) in res.items():
            print(f"  w {w}: makespan {m}, balanced {bal:.0f}, makespan / w75 {m / res[75][0]:.4f}, work / w75 {bal / res[75][1]:.4f}")


if __name__ == "__main__":
    main()

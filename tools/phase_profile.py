"""Developer script: per-phase share of the solve kernel's cycles (diagnostic build with in-kernel s_memtime ticks,
build.build_hip_profile()), and the retried factorisations: retry passes, how far the failed passes got, and the ticks a
retry pass spends inside stages a failed pass of the iteration had evaluated (build.build_hip_no_reuse(profile=True) for
the kernel without the reuse path: CMPC_PROF_LIB).  usage (GPU box): python tools/phase_profile.py [workload] [B]"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["CMPC_LIB_PATH"] = os.environ.get("CMPC_PROF_LIB") or os.path.join(ROOT, "tools", "libcmpc_amd_prof.so")
import numpy as np, torch
import cmpc_amd
from cmpc_amd import workloads as wl, capi
from cmpc_amd.solver import BatchedCentroidalMPC
name = sys.argv[1] if len(sys.argv) > 1 else "randomized"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
spec, rec = wl.make_workload(name, B=B)
if spec.N > 20:
    spec.max_iter = 150
s = BatchedCentroidalMPC(spec, device="cuda:0")
d = torch.from_numpy(rec).to("cuda:0")
s.solve(d); torch.cuda.synchronize()
lib = capi.load()
import re
_hdr = open(os.path.join(os.path.dirname(cmpc_amd.__file__), "csrc", "cmpc_kernel.hpp")).read()
NPROF = int(re.search(r"#define CMPC_NPROF (\d+)", _hdr).group(1))          # (one home: the kernel header)
# retry slots (cmpc_retry_class in the kernel header): ticks of retry passes inside stages a failed pass had evaluated, by phase slot
RETRY_CLASS = {31: (11, 12, 26, 0), 32: (24, 25), 34: (27,)}                 # 33: every other phase slot
buf = (ctypes.c_longlong * NPROF)()
lib.cmpc_profile_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
assert lib.cmpc_profile_read(s._h, buf) == 0
_, _, iters, _ = s.solve(d); torch.cuda.synchronize()
assert lib.cmpc_profile_read(s._h, buf) == 0
n_it = float(iters.sum().item())
v = np.array(list(buf), dtype=np.float64)
names = {27: "reuse path: reloads + LDS commit", 24: "stage iterates: load + LDS commit", 11: "geometry", 12: "inequality rows", 25: "barrier weights", 26: "gradient / residual",
         0: "slab stores of the evaluation", 1: "Hessian rows: diagonal", 9: "Hessian rows: row roles and coefficients", 15: "Hessian rows: force columns", 23: "Hessian rows: velocity and state columns", 13: "P b", 10: "G'PG: T = P[B A]", 14: "G'PG: M += [B A]'T", 
         19: "Cholesky: trailing write-back of the previous block + block load", 20: "Cholesky: pivot chain + in-block updates", 21: "Cholesky: block store", 22: "MFMA trailing update",  8: "(factor tail)",
         2: "backward vectors: m", 3: "backward vectors: l", 5: "backward vectors: p", 4: "factor store",
         16: "forward sweep: loads", 17: "forward sweep: du, slack directions", 18: "forward sweep: dx", 6: "(forward tail + reductions)", 7: "step application"}
tot = v[:28].sum()
B_, iters_np = len(iters), iters.cpu().numpy()
print(f"cycles per instance-iteration (s_memtime ticks): {tot / n_it:.0f}   kernel {s.last_kernel_ms():.1f} ms")
for i in np.argsort(-v[:28]):
    if v[i] > 0:
        print(f"{100 * v[i] / tot:5.1f} %  {v[i] / n_it:8.0f} cyc/it  tick {i:2d}  {names.get(int(i), '')}")
retries, evaluated, reused, again = v[28], v[29], v[30], v[35]
spec_N = spec.N
print(f"retried factorisations: {retries / B_:.2f} retry passes per solve ({again / B_:.2f} of them fail again), the failed passes had "
      f"evaluated {evaluated / max(retries, 1):.1f} of {spec_N + 1} stages on average = {evaluated / (spec_N + 1) / B_:.2f} sweeps per solve; "
      f"{reused / B_:.1f} stages per solve taken from the slab")
inside = v[31] + v[32] + v[33] + v[34]
print(f"ticks of retry passes inside stages a failed pass had evaluated: {100 * inside / tot:.2f} % of the launch's ticks")
print(f"  {100 * v[31] / tot:5.2f} %  geometry, inequality rows, gradient / residual, evaluation stores (independent of the regularisation)")
print(f"  {100 * v[32] / tot:5.2f} %  stage loads, barrier weights")
print(f"  {100 * v[34] / tot:5.2f} %  reuse path: reloads")
print(f"  {100 * v[33] / tot:5.2f} %  the rest (column lists, P b, G'PG, Hessian rows, factorisation, backward vectors, factor store)")

"""CPU tier of the whole-body QP from task Jacobians (cmpc_wbc_qp_solve_tasks): the synthetic task instances against
wbc_synthetic, the stacked form against assemble_task_cost, the C ABI's symbols, default gains and argument checks, and
the oracle alone on the sample the GPU tier compares against."""
import ctypes
import hashlib
import os
import re

import numpy as np
import torch

from cmpc_amd import capi, wbc, workloads as wl
from wbc_tasks_common import B_MIXED, literal_cost, mixed_oracle, task_instances

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# sha256 over the five arrays of wbc_synthetic(**kw), recorded before wbc_synthetic_tasks shared its draws
SYNTHETIC_HASHES = [(dict(B=8, seed=21), "399be8449672480ddeed8df0696088c05daf654256c5515f96ab6b3aaedba660"),
                    (dict(B=5, seed=3, contact="lfoot"), "2b25e5bedf240a23c3f9b28c3213d74a954cc51c6f119db89d90767a51fa06de"),
                    (dict(B=3, seed=5, contact="rfoot", mass=40.0, g=9.0), "ca974f9cf65bea4f555f7bbdc8dcdaf08cd8eddb99a631db6636635b66a3f29c")]


def test_wbc_synthetic_is_unchanged():
    for kw, want in SYNTHETIC_HASHES:
        h = hashlib.sha256()
        for a in wl.wbc_synthetic(**kw):
            h.update(np.ascontiguousarray(a).tobytes())
        assert h.hexdigest() == want, kw


def test_synthetic_tasks_are_the_instances_of_wbc_synthetic():
    """M, h and the feet's Jacobians bit for bit; Hq, Fq of the literal loop over the task form to 1e-10 (about 150 terms
    of size O(1) at 2e-16 each: 1e-13 at most, three orders of margin)."""
    Hq, Fq, M, h, Jc = wl.wbc_synthetic(8, seed=21)
    J, Jdot, ff, pe, ve, qd, sel, Mt, ht = task_instances()
    assert J.shape == (64, 21, 30) and Jdot.shape == J.shape and ff.shape == pe.shape == ve.shape == (64, 51)
    assert qd.shape == (64, 30) and sel.shape == (30,)
    assert np.array_equal(Mt[:8], M) and np.array_equal(ht[:8], h) and np.array_equal(J[:8, :12], Jc)
    worst = 0.0
    for b in range(8):
        H, F = literal_cost(J[b], Jdot[b], ff[b], pe[b], ve[b], qd[b], sel)
        worst = max(worst, np.abs(H - Hq[b]).max(), np.abs(F - Fq[b]).max())
        assert np.allclose(H, Hq[b], rtol=1e-10, atol=1e-10) and np.allclose(F, Fq[b], rtol=1e-10, atol=1e-10)
    print(f"literal loop over the task form against wbc_synthetic: max abs deviation {worst:.2e}")
    # the second stream is in use: a Jdot qd term of the size of the targets, errors that the gains amplify
    assert np.abs(np.einsum("brn,bn->br", Jdot, qd)).mean() > 0.3 and np.abs(pe).mean() > 0.01 and np.abs(ve).mean() > 0.05
    # instance b does not depend on B
    assert all(np.array_equal(a[:5], c) for a, c in zip(task_instances(), wl.wbc_synthetic_tasks(5, seed=21)) if a.ndim > 1)


def test_stack_tasks_and_the_literal_loop_reproduce_assemble_task_cost():
    """The inputs of test_wbc_qp.test_cost_assembly_matches_the_literal_loop (same generator, same draws), with the joint
    task as the task form has it: Jacobian diag(sel), zero derivative."""
    rng = np.random.default_rng(5)
    B, rows = 3, {'lfoot': 6, 'rfoot': 6, 'com': 3, 'torso': 3, 'base': 3, 'joints': 30}
    J = {k: rng.normal(size=(B, r, 30)) for k, r in rows.items()}
    Jd = {k: rng.normal(size=(B, r, 30)) for k, r in rows.items()}
    ff, pe, ve = ({k: rng.normal(size=(B, r)) for k, r in rows.items()} for _ in range(3))
    qd = rng.normal(size=(B, 30))
    sel = np.diagonal(J['joints'][0]).copy()
    J['joints'] = np.tile(np.diag(sel), (B, 1, 1))
    Jd['joints'] = np.zeros((B, 30, 30))
    t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}
    Hq, Fq = wbc.assemble_task_cost(t(J), t(Jd), t(ff), t(pe), t(ve), torch.from_numpy(qd))
    Js, Jds, ffs, pes, ves = (a.numpy() for a in wbc.stack_tasks(t(J), t(Jd), t(ff), t(pe), t(ve)))
    assert Js.shape == Jds.shape == (B, 21, 30) and ffs.shape == pes.shape == ves.shape == (B, 51)
    assert np.array_equal(Js[:, 12:15], J['com']) and np.array_equal(ffs[:, 21:], ff['joints'])
    for b in range(B):
        H, F = literal_cost(Js[b], Jds[b], ffs[b], pes[b], ves[b], qd[b], sel)
        assert np.allclose(Hq[b].numpy(), H, rtol=1e-12, atol=1e-12) and np.allclose(Fq[b].numpy(), F, rtol=1e-12, atol=1e-12)
    assert wbc.stack_tasks(t(J), None, t(ff), t(pe), t(ve))[1] is None


def test_header_symbols_and_default_gains():
    text = open(os.path.join(ROOT, "include", "cmpc_wbc.h")).read()
    names = set(re.findall(r"\b(cmpc_wbc_[a-z_]+)\s*\(", text))
    assert {"cmpc_wbc_qp_solve_tasks", "cmpc_wbc_default_gains"} <= names and names == set(capi.WBC_SYMBOLS)
    assert int(re.search(r"#define CMPC_WBC_TASK_ROWS (\d+)", text).group(1)) == wbc.TASK_ROWS == 21 and wbc.NACC == 51
    lib = capi.load()
    g = capi.WbcGains()
    lib.cmpc_wbc_default_gains(ctypes.byref(g))
    assert g.struct_size == ctypes.sizeof(capi.WbcGains) == 8 + 18 * 8 and g.reserved == 0
    for i, task in enumerate(wbc.TASKS):
        assert (g.weight[i], g.pos_gain[i], g.vel_gain[i]) == (wbc.WEIGHTS[task], wbc.POS_GAINS[task], wbc.VEL_GAINS[task])
    assert wl.WBC_POS_GAINS == wbc.POS_GAINS and wl.WBC_VEL_GAINS == wbc.VEL_GAINS and tuple(wl.WBC_TASK_ROWS) == wbc.TASKS[:-1]
    mine = wbc.make_gains()
    assert bytes(mine) == bytes(g)
    other = wbc.make_gains(weights={'com': 2.0}, vel_gains={'joints': 6.0})
    assert other.weight[2] == 2.0 and other.vel_gain[5] == 6.0 and other.weight[5] == 0.1 and other.pos_gain[2] == 5.0


def test_solve_tasks_argument_checks_return_before_any_hip_call():
    """Every rejected call returns 1 with the check's own message (a call that got as far as the HIP runtime would name a
    HIP error instead, with or without a GPU); B == 0 is a valid empty batch whatever the buffers."""
    lib = capi.load()
    # J, Jdot, acc_ff, pos_err, vel_err, qd, joint_sel, M, h, contact, foot_mu | tau, qdd, f_c, status, iters
    bufs = [np.zeros(n) for n in (630, 630, 51, 51, 51, 30, 30, 900, 30, 2, 2, 30, 30, 12)] + [np.zeros(1, dtype=np.int32) for _ in range(2)]
    ptr = [b.ctypes.data for b in bufs]
    gains = wbc.make_gains()

    def call(B=1, tol=1e-9, max_iter=60, null=(), g=gains):
        p = [None if i in null else v for i, v in enumerate(ptr)]
        return lib.cmpc_wbc_qp_solve_tasks(0, B, *p[:11], None if g is None else ctypes.byref(g), tol, max_iter, *p[11:], None)

    assert lib.cmpc_wbc_qp_solve_tasks(0, 0, *([None] * 12), 1e-9, 60, *([None] * 6)) == 0
    small = wbc.make_gains()
    small.struct_size -= 8
    cases = [(dict(B=-1), b"negative batch")]
    cases += [(dict(null=(i,)), b"null buffer") for i in range(16) if i not in (1, 5)]       # (Jdot and qd: below)
    cases += [(dict(null=(5,)), b"null buffer"), (dict(g=None), b"null buffer")]             # qd missing next to a Jdot
    cases += [(kw, b"bad argument") for kw in (dict(tol=0.0), dict(tol=-1e-9), dict(tol=float("nan")), dict(max_iter=0),
                                               dict(max_iter=-3))]
    cases += [(dict(g=small), b"struct_size"), (dict(g=capi.WbcGains()), b"struct_size")]
    for kw, msg in cases:
        assert call(**kw) == 1, kw
        err = lib.cmpc_wbc_last_error()
        assert err and b"cmpc_wbc_qp_solve_tasks" in err and msg in err, (kw, err)


def test_the_oracle_solves_the_whole_gpu_sample():
    """The sixty instances the GPU tier holds the kernel against: the oracle converges on every one, in at most 27
    iterations, and floors no pivot (a floored step is a different step: iteration counts are compared where none is)."""
    refs = [mixed_oracle(b) for b in range(B_MIXED)]
    assert [r["status"] for r in refs] == [0] * B_MIXED
    print("iterations:", [r["iters"] for r in refs])
    assert max(r["iters"] for r in refs) <= 27
    assert sum(r["floored"] for r in refs) == 0

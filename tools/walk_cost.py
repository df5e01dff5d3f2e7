"""What the walking loop around the rigid-body model costs: ms per launch of `BatchedRobot.task_references` and
`BatchedRobot.integrate` (HIP events, median of K launches after W warm-up launches) at B = 8192 and 65 536 HRP-4 robots on
the shipped walk, the bytes each launch moves and the resulting GB/s; the same references formed by torch expressions (the
vectorised form of the test mirror), for comparison; and the share of a whole rollout tick (MPC + evaluate + references + QP
+ integrate) the two launches take.  A report-only leg walks 6 robots for 200 ticks through `walking_model` and records the
per-tick swing-foot and CoM tracking error and the QP failures.  One session's numbers.

usage: python tools/walk_cost.py [--steps K] [--warmup W] [--sizes 8192,65536] [--out profiles/walk_cost.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
UNIQ, SEED = 1024, 20261020


def torch_references(tab, t, plan, ev, com_des, q, v, q_ref):
    """The references of `cmpc_walk_task_refs` for one scene as torch expressions on the device: (ff, pos_err, vel_err)."""
    import torch
    B, ar = t.shape[0], torch.arange(t.shape[0], device=t.device)
    idx = tab["step_idx"][t.long()].long()
    tt, ss = (t - tab["step_start"][idx]).double()[:, None], tab["ss_dur"][idx].double()[:, None]
    prev, nxt = torch.clamp(idx - 1, min=0), idx + 1
    T = torch.clamp(ss, min=1.0)
    A, Bc, d = -2 / T**3, 3 / T**2, tab["delta"]
    s0, s1, s2 = A * tt**3 + Bc * tt**2, (3 * A * tt**2 + 2 * Bc * tt) / d, (6 * A * tt + 2 * Bc) / d**2
    p0, p1 = torch.cat([tab["ang"][prev], plan[ar, prev]], 1), torch.cat([tab["ang"][nxt], plan[ar, nxt]], 1)
    pos, vel, acc = p0 + (p1 - p0) * s0, (p1 - p0) * s1, (p1 - p0) * s2
    h = tab["step_height"]
    Az, Bz, Cz = 16 * h / T**4, -32 * h / T**3, 16 * h / T**2
    pos[:, 5:6] = Az * tt**4 + Bz * tt**3 + Cz * tt**2
    vel[:, 5:6] = (4 * Az * tt**3 + 3 * Bz * tt**2 + 2 * Cz * tt) / d
    acc[:, 5:6] = (12 * Az * tt**2 + 6 * Bz * tt + 2 * Cz) / d**2
    single = tt < ss
    zero = torch.zeros_like(pos)
    swing = [torch.where(single, a, b) for a, b in ((pos, p1), (vel, zero), (acc, zero))]
    support = [torch.cat([tab["ang"][idx], plan[ar, idx]], 1), zero, zero]
    sup_l, first = tab["support_l"][idx].bool()[:, None], (idx == 0)[:, None]
    feet = []
    for f, left in enumerate((True, False)):
        mine = sup_l if left else ~sup_l
        now = [torch.where(mine, a, b) for a, b in zip(support, swing)]
        now[0] = torch.where(first, tab["init_feet"][6 * f:6 * f + 6].expand(B, 6), now[0])
        feet.append([now[0]] + [torch.where(first, zero, x) for x in now[1:]])
    mean = [(feet[0][k][:, :3] + feet[1][k][:, :3]) / 2. for k in range(3)]
    com = com_des.reshape(B, 3, 3)
    des = [torch.cat([feet[0][k], feet[1][k], com[:, k], mean[k], mean[k]], 1) for k in range(3)]
    ff, pe, ve = (torch.zeros((B, 51), dtype=torch.float64, device=t.device) for _ in range(3))
    ff[:, :21] = des[2] - ev.jdqd
    pe[:, :21] = des[0] - ev.pose
    ve[:, :21] = des[1] - ev.vel

    def exp(w):
        th = torch.linalg.norm(w, dim=1).clamp(min=1e-12)[:, None, None]
        K = torch.zeros((B, 3, 3), dtype=torch.float64, device=w.device)
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
        return torch.eye(3, dtype=torch.float64, device=w.device) + torch.sin(th) / th * K + (1 - torch.cos(th)) / th**2 * (K @ K)

    for r0 in (0, 6, 15, 18):
        E = exp(des[0][:, r0:r0 + 3]) @ exp(ev.pose[:, r0:r0 + 3]).transpose(1, 2)
        s = 0.5 * torch.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], 1)
        sn = torch.linalg.norm(s, dim=1)
        th = torch.atan2(sn, 0.5 * (E[:, 0, 0] + E[:, 1, 1] + E[:, 2, 2] - 1))
        pe[:, r0:r0 + 3] = s * torch.where(sn > 1e-9, th / sn.clamp(min=1e-300), torch.ones_like(sn))[:, None]
    pe[:, 27:], ve[:, 27:] = q_ref[6:] - q[:, 6:], -v[:, 6:]
    return ff, pe, ve


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="8192,65536")
    ap.add_argument("--walk-ticks", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk_cost.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import cmpc_amd  # noqa: F401
    from cmpc_amd import rbd, wbc, workloads as wl
    from cmpc_amd.problem import ProblemSpec
    from cmpc_amd.rollout import BatchedRollout

    dev = "cuda:0"
    model = rbd.RobotModel.from_urdf(os.path.join(ROOT, "tests", "golden", "hrp4.urdf"))
    robot = rbd.BatchedRobot(model, device=dev)
    scene = wl.Scene()
    gait = rbd.Gait(scene, device=dev)
    host = scene.gait_tables()
    tab = {k: (torch.from_numpy(np.ascontiguousarray(a[0])).to(dev) if isinstance(a, np.ndarray) else a) for k, a in host.items()}
    qp = wbc.BatchedInverseDynamicsQP(foot_size=0.1, mu=0.5, device=dev)
    rng = np.random.default_rng(SEED)
    q0 = model.place_on_ground(model.configuration(rbd.HRP4_INITIAL_DEG, degrees=True))
    q_ref = torch.from_numpy(q0).to(dev)
    qu = np.tile(q0, (UNIQ, 1))
    qu[:, 0:3] += rng.normal(scale=0.02, size=(UNIQ, 3))
    qu[:, 22:30] += rng.uniform(-0.2, 0.2, size=(UNIQ, 8))
    vu = rng.normal(scale=0.05, size=(UNIQ, 30))
    last = int(host["step_start"][0, -1]) - 1                 # ticks with a next plan entry
    tu = rng.integers(0, min(last, scene.T - 1), size=UNIQ).astype(np.int32)
    pu = np.tile(scene.plan_pos, (UNIQ, 1, 1))
    pu[:, :, :2] += rng.uniform(-0.03, 0.03, size=(UNIQ, pu.shape[1], 2))
    cu = np.concatenate([scene.com_tab[tu, 0:3], scene.com_tab[tu, 3:6], scene.com_tab[tu, 6:9]], axis=1)

    def timed(call, steps=args.steps, warmup=args.warmup):
        ms = []
        for i in range(warmup + steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = call()
            b.record()
            b.synchronize()
            if i >= warmup:
                ms.append(a.elapsed_time(b))
        return out, ms

    rows = []
    for B in (int(x) for x in args.sizes.split(",")):
        tile = lambda a: torch.from_numpy(np.ascontiguousarray(np.tile(a, (B // UNIQ,) + (1,) * (a.ndim - 1)))).to(dev)
        q, v, t, plan, com_des = tile(qu), tile(vu), tile(tu), tile(pu), tile(cu)
        ev, ems = timed(lambda: robot.evaluate(q, v))
        refs, rms = timed(lambda: robot.task_references(gait, t, None, plan, ev, com_des, q, v, q_ref))
        mirror, tms = timed(lambda: torch_references(tab, t, plan, ev, com_des, q, v, q_ref))
        diff = max(float((a - b).abs().max()) for a, b in zip(refs[:3], mirror))
        contact = torch.ones((B, 2), dtype=torch.float64, device=dev)
        sel = torch.from_numpy(model.joint_selection(rbd.HRP4_REDUNDANT_DOFS)).to(dev)
        out, qms = timed(lambda: qp.solve_tasks(ev.J, None, refs.ff, refs.pos_err, refs.vel_err, None, ev.M, ev.h, contact,
                                                joint_selection=sel))
        hold = out[3] != 0
        _, ims = timed(lambda: robot.integrate(q, v, out[1], 0.01, hold=hold))
        # bytes per robot: t, three plan rows, pose / vel / jdqd, com_des, q, v in; ff, pos_err, vel_err, feet_des out
        refs_bytes = B * (4 + 8 * (9 + 3 * 21 + 9 + 60) + 8 * (3 * 51 + 36))
        int_bytes = B * (8 * 90 + 1 + 8 * 60)
        # the whole tick, through the rollout (N = 10, one scene, the robots' own q, v integrated in place)
        ro = BatchedRollout(scene, ProblemSpec(N=10), B, device=dev, mu=0.5)
        qr, vr = q.clone(), torch.zeros_like(v)
        ro.attach_whole_body_tasks(qp, robot.walking_model(qr, vr, gait, q_ref=q_ref))
        com, dcom = scene.nominal_state(np.full(B, 255))
        ro.reset(255, com, dcom)
        _, kms = timed(ro.step, steps=min(args.steps, 5), warmup=2)
        med = {k: statistics.median(x) for k, x in dict(evaluate=ems, refs=rms, torch_refs=tms, solve_tasks=qms, integrate=ims, tick=kms).items()}
        rows.append(dict(B=B, task_refs_ms=med["refs"], task_refs_bytes=refs_bytes, task_refs_GBps=refs_bytes / med["refs"] / 1e6,
                         integrate_ms=med["integrate"], integrate_bytes=int_bytes, integrate_GBps=int_bytes / med["integrate"] / 1e6,
                         torch_refs_ms=med["torch_refs"], torch_over_kernel=med["torch_refs"] / med["refs"],
                         torch_vs_kernel_max_abs_diff=diff, evaluate_ms=med["evaluate"], solve_tasks_ms=med["solve_tasks"],
                         solve_tasks_status0=int((out[3] == 0).sum()), tick_ms=med["tick"],
                         new_launches_share_of_tick=(med["refs"] + med["integrate"]) / med["tick"],
                         launches={k: [round(x, 4) for x in xs] for k, xs in dict(task_refs=rms, integrate=ims, torch_refs=tms,
                                                                                  tick=kms).items()}))
        print(json.dumps(rows[-1]))
        del ro, ev, refs, mirror, out

    # report only: 6 robots, the shipped walk from the end of its initial double support
    B, t0 = 6, 150
    q = torch.from_numpy(np.tile(q0, (B, 1))).to(dev)
    v = torch.zeros_like(q)
    # (the MPC's angular momentum is the reference's recording, as in tools/walk_demo.py: the robots' own is not fed back)
    hw = np.loadtxt(os.path.join(ROOT, "tests", "golden", "measured_hw_cuhw.txt"))
    ro = BatchedRollout(scene, ProblemSpec(N=10), B, device=dev, mu=0.5, hw_measured=hw)
    wm = robot.walking_model(q, v, gait, q_ref=q_ref)
    ro.attach_whole_body_tasks(qp, wm)
    com, dcom = scene.nominal_state(np.full(B, t0))
    ro.reset(t0, com, dcom)
    swing, comerr, fails, alive = [], [], [], []
    for i in range(args.walk_ticks):
        tk = ro.t.clone()
        ro.step()
        r, e = wm.last_references, wm.last_evaluation
        idx = tab["step_idx"][tk.long()].long()
        left_swings = ~tab["support_l"][idx].bool()
        err_l = (r.feet_des[:, 3:6] - e.pose[:, 3:6]).norm(dim=1)
        err_r = (r.feet_des[:, 21:24] - e.pose[:, 9:12]).norm(dim=1)
        swing.append(float(torch.where(left_swings, err_l, err_r).max()))
        comerr.append(float(r.pos_err[:, 12:15].norm(dim=1).max()))
        fails.append(int((ro.last_wbc[3] != 0).sum()))
        alive.append(int(ro.alive.sum()))
    walk = dict(B=B, t0=t0, ticks=args.walk_ticks, qp_failures=int(sum(fails)), qp_failures_per_tick=fails, mpc_alive_per_tick=alive,
                swing_foot_error_m=[round(x, 5) for x in swing], com_error_m=[round(x, 5) for x in comerr],
                finite_state=bool(torch.isfinite(q).all() and torch.isfinite(v).all()),
                base_height_end_m=[round(float(x), 4) for x in q[:, 5]],
                note="report only: worst robot per tick; swing_foot_error is of the foot that is not the step's support foot; "
                     "whether HRP-4 stays upright in this loop is not asserted anywhere")
    print(json.dumps({k: walk[k] for k in ("qp_failures", "finite_state", "base_height_end_m")}))
    res = dict(workload=f"HRP-4, {UNIQ} seeded instances around the initial configuration on the shipped walk, tiled; one session",
               method="HIP events around one launch (tick: around one BatchedRollout.step, N = 10, one scene, walking_model "
                      "attached), median of `steps` after `warmup`",
               steps=args.steps, warmup=args.warmup, rows=rows, walk=walk)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

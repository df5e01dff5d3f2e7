"""What the contact plant costs, and what HRP-4 does on it: ms per launch of `BatchedRobot.simulate` (HIP events, median of K
launches after W warm-up launches) at B = 8192 and 65 536 HRP-4 robots with 30 and 100 sweeps, next to
`BatchedRobot.integrate` -- the launch the plant replaces -- timed in the same session, next to the same step written as
batched torch expressions (`torch.linalg.cholesky`, `cholesky_solve`, the sweeps as a Python loop of torch operations), the
bytes a launch moves and its share of a whole rollout tick.  No number is fixed in advance and nothing is tuned to the outcome.
A report-only leg walks 6 robots for 200 ticks from t = 150 with `feedback=True` on the plant, with 30 and 100 sweeps, without
a push and with 6 N in y on the base (the reference's 3 N on base and torso summed onto the base; the reference pushes for
100 ticks from tick 800, here the 100 ticks begin 50 ticks into the run), and lists per robot the ticks until `alive` first
clears, and per run the largest residual, the lowest vertex height, the swing-foot error and the CoM error against the MPC.
Whether the robots stay up is not asserted anywhere.  One session's numbers.

usage: python tools/walk_plant_cost.py [--steps K] [--warmup W] [--sizes 8192,65536] [--out profiles/walk_plant_cost.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
UNIQ, SEED = 1024, 20261021
# bytes per robot, every word once (what a stepped robot moves):
#   plant      in: q, v, h 90, M 900, J 630, pose 21, tau 24, ext 6, foot_mu 2, impulse 24 words and hold;
#              out: q, v 60, impulse 24, residual 1 words and status
#   integrate  in: q, v, qdd 90 words and hold; out: q, v 60 words
PLANT_BYTES = 8 * (90 + 900 + 630 + 21 + 24 + 6 + 2 + 24) + 1 + 8 * (60 + 24 + 1) + 4       # 14261
INTEGRATE_BYTES = 8 * 90 + 1 + 8 * 60                                                          # 1201
FALL = (0.3, 1.0)                                                  # of the report-only walk: CoM height, base tilt in rad
CORNERS = ((1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0))


def exp_so3(w):
    """Rotation matrices (B,3,3) of rotation vectors (B,3), by Rodrigues' formula."""
    import torch
    t = w.norm(dim=1).clamp_min(1e-300)
    a = (w / t[:, None])
    K = torch.zeros((w.shape[0], 3, 3), dtype=w.dtype, device=w.device)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -a[:, 2], a[:, 1], a[:, 2], -a[:, 0], -a[:, 1], a[:, 0]
    eye = torch.eye(3, dtype=w.dtype, device=w.device)
    return eye + torch.sin(t)[:, None, None] * K + (1.0 - torch.cos(t))[:, None, None] * (K @ K)


def log_so3(R):
    """Rotation vectors of rotation matrices, the arccos form (angles well below pi)."""
    import torch
    c = ((R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1.0) / 2.0).clamp(-1.0, 1.0)
    t = torch.arccos(c)
    s = torch.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], dim=1) / 2.0
    k = torch.where(t > 1e-8, t / torch.sin(t).clamp_min(1e-300), torch.ones_like(t))
    return s * k[:, None]


def vertex_arms(pose, half):
    """(arms (B,8,3), heights (B,8)) of the sole vertices from the task poses (B,21) and the half foot size (B,)."""
    import torch
    arms, heights = [], []
    for f in range(2):
        Rf = exp_so3(pose[:, 6 * f:6 * f + 3])
        for sx, sy in CORNERS:
            s = torch.stack([sx * half, sy * half, torch.zeros_like(half)], dim=1)
            r = (Rf @ s[:, :, None])[:, :, 0]
            arms.append(r)
            heights.append(pose[:, 6 * f + 5] + r[:, 2])
    return torch.stack(arms, dim=1), torch.stack(heights, dim=1)


def torch_step(q, v, ev, tau, ext, foot_mu, impulse, sweeps, dt, erp=0.2, ground_z=0.0):
    """The step of include/cmpc_walk.h (cmpc_walk_plant_step) as batched torch expressions -> (q+, v+, p)."""
    import torch
    B = q.shape[0]
    half, mu = foot_mu[:, 0], foot_mu[:, 1]
    R = exp_so3(q[:, 0:3])
    Rt = R.transpose(1, 2)
    g = torch.cat([(Rt @ ext[:, 0:3, None])[:, :, 0], (Rt @ ext[:, 3:6, None])[:, :, 0], tau], dim=1) - ev.h
    L = torch.linalg.cholesky(ev.M)
    v_free = v + dt * torch.cholesky_solve(g[:, :, None], L)[:, :, 0]
    arms, heights = vertex_arms(ev.pose, half)
    rows = []
    for i in range(8):
        f = i // 4
        r = arms[:, i, :, None].expand(B, 3, 30)
        rows.append(ev.J[:, 6 * f + 3:6 * f + 6] - torch.cross(r, ev.J[:, 6 * f:6 * f + 3], dim=1))
    Jc = torch.cat(rows, dim=1)
    Y = torch.cholesky_solve(Jc.transpose(1, 2), L)
    W = Jc @ Y
    c = (Jc @ v_free[:, :, None])[:, :, 0]
    phi = heights - ground_z
    c[:, 2::3] += torch.where(phi >= 0.0, phi, erp * phi) / dt
    p = impulse.clone()

    def cone(i):
        n = 3 * i + 2
        hyp, lim = torch.hypot(p[:, 3 * i], p[:, 3 * i + 1]), mu * p[:, n]
        scale = torch.where(hyp > lim, torch.where(lim > 0.0, lim / hyp.clamp_min(1e-300), torch.zeros_like(lim)), torch.ones_like(lim))
        p[:, 3 * i:3 * i + 2] *= scale[:, None]

    for i in range(8):
        p[:, 3 * i + 2].clamp_(min=0.0)
        cone(i)
    for _ in range(sweeps):
        for i in range(8):
            n = 3 * i + 2
            p[:, n] = (p[:, n] - ((W[:, n] * p).sum(dim=1) + c[:, n]) / W[:, n, n]).clamp_min(0.0)
            for a in (3 * i, 3 * i + 1):
                p[:, a] = p[:, a] - ((W[:, a] * p).sum(dim=1) + c[:, a]) / W[:, a, a]
            cone(i)
    vn = v_free + (Y @ p[:, :, None])[:, :, 0]
    qn = torch.cat([log_so3(R @ exp_so3(dt * vn[:, 0:3])), q[:, 3:6] + dt * (R @ vn[:, 3:6, None])[:, :, 0], q[:, 6:] + dt * vn[:, 6:]], dim=1)
    return qn, vn, p


def finite_max(x):
    x = x[x.isfinite()]
    return round(float(x.max()), 6) if x.numel() else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="8192,65536")
    ap.add_argument("--sweeps", default="30,100")
    ap.add_argument("--walk-ticks", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk_plant_cost.json"))
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
    tu = rng.normal(scale=5.0, size=(UNIQ, 24))
    sweeps_list = [int(x) for x in args.sweeps.split(",")]
    delta = ProblemSpec(N=10).delta

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
        q, v, tau = tile(qu), tile(vu), tile(tu)
        ev = robot.evaluate(q, v)
        foot_mu = torch.tensor([0.05, 0.5], dtype=torch.float64, device=dev).repeat(B, 1)
        ext = torch.zeros((B, 6), dtype=torch.float64, device=dev)
        hold = torch.zeros(B, dtype=torch.bool, device=dev)
        qdd = tile(rng.normal(scale=5.0, size=(UNIQ, 30)))
        _, ims = timed(lambda: robot.integrate(q, v, qdd, delta, hold=hold))
        integrate_ms = statistics.median(ims)
        for sweeps in sweeps_list:
            plant = rbd.Plant(delta, sweeps=sweeps)
            # (every launch of the series starts cold from the same robots: out of place, the warm start zero)
            cold = lambda: torch.zeros((B, 24), dtype=torch.float64, device=dev)
            imp = cold()
            step, pms = timed(lambda: robot.simulate(q, v, ev, tau, foot_mu, plant, ext=ext, hold=hold, impulse=imp.zero_()))
            (tq, tv, tp), tms = timed(lambda: torch_step(q, v, ev, tau, ext, foot_mu, cold(), sweeps, delta), steps=min(args.steps, 3), warmup=1)
            agree = dict(v=float((tv - step.v).abs().max()), q=float((tq - step.q).abs().max()), impulse=float((tp - step.impulse).abs().max()))
            # the batch is UNIQ robots tiled: every tile of an output must be the first one, bit for bit
            tiles = lambda x: bool((x.view(B // UNIQ, UNIQ, -1) == x[:UNIQ]).all())
            tiled = dict(kernel=tiles(step.v) and tiles(step.impulse), torch=tiles(tv) and tiles(tp))
            ro = BatchedRollout(scene, ProblemSpec(N=10), B, device=dev, mu=0.5, feedback=True, mass=model.total_mass)
            qr, vr = q.clone(), torch.zeros_like(v)
            ro.attach_whole_body_tasks(qp, robot.walking_model(qr, vr, gait, q_ref=q_ref, plant=plant))
            com, dcom = scene.nominal_state(np.full(B, 255))
            ro.reset(255, com, dcom)
            _, kms = timed(ro.step, steps=min(args.steps, 5), warmup=2)
            del ro
            med = dict(plant=statistics.median(pms), torch=statistics.median(tms), tick=statistics.median(kms))
            rows.append(dict(B=B, sweeps=sweeps, plant_ms=med["plant"], plant_bytes=B * PLANT_BYTES,
                             plant_GBps=B * PLANT_BYTES / med["plant"] / 1e6, integrate_ms=integrate_ms,
                             plant_over_integrate_ms=med["plant"] / integrate_ms, torch_ms=med["torch"],
                             torch_over_plant=med["torch"] / med["plant"], kernel_beats_torch=bool(med["plant"] < med["torch"]),
                             torch_minus_kernel_abs_max=agree, tiles_identical=tiled, residual_max=finite_max(step.residual),
                             stepped=int((step.status == 0).sum()), tick_with_plant_ms=med["tick"],
                             plant_share_of_tick=med["plant"] / med["tick"],
                             launches={k: [round(x, 4) for x in xs] for k, xs in dict(plant=pms, integrate=ims, torch=tms, tick=kms).items()}))
            print(json.dumps({k: rows[-1][k] for k in rows[-1] if k != "launches"}))
        del ev

    # report only: 6 robots on the plant, the shipped walk from the end of its initial double support, with feedback
    B, t0 = 6, 150
    push_from, push_ticks = 50, 100
    walks = {}
    for sweeps in sweeps_list:
        for push in (0.0, 6.0):
            q = torch.from_numpy(np.tile(q0, (B, 1))).to(dev)
            v = torch.zeros_like(q)
            ext = torch.zeros((B, 6), dtype=torch.float64, device=dev)
            ro = BatchedRollout(scene, ProblemSpec(N=10), B, device=dev, mu=0.5, feedback=True, mass=model.total_mass)
            wm = robot.walking_model(q, v, gait, q_ref=q_ref, fall=FALL, plant=rbd.Plant(delta, sweeps=sweeps), ext=ext)
            ro.attach_whole_body_tasks(qp, wm)
            com, dcom = scene.nominal_state(np.full(B, t0))
            ro.reset(t0, com, dcom)
            swing, comerr, resid, lowest, alive, fails = [], [], [], [], [], []
            first_dead = [None] * B
            half = torch.full((B,), 0.05, dtype=torch.float64, device=dev)
            for i in range(args.walk_ticks):
                ext[:, 4] = push if push_from <= i < push_from + push_ticks else 0.0
                tk = ro.t.clone()
                ro.step()
                r, e, ps = wm.last_references, wm.last_evaluation, wm.last_plant
                idx = tab["step_idx"][tk.long().clamp(max=tab["step_idx"].shape[0] - 1)].long()
                left_swings = ~tab["support_l"][idx].bool()
                err_l = (r.feet_des[:, 3:6] - e.pose[:, 3:6]).norm(dim=1)
                err_r = (r.feet_des[:, 21:24] - e.pose[:, 9:12]).norm(dim=1)
                swing.append(finite_max(torch.where(left_swings, err_l, err_r)))
                comerr.append(finite_max(r.pos_err[:, 12:15].norm(dim=1)))
                resid.append(finite_max(ps.residual[ps.status == 0]))
                h = vertex_arms(e.pose, half)[1]
                h = h[h.isfinite()]
                lowest.append(round(float(h.min()), 6) if h.numel() else None)
                fails.append(int((ro.last_wbc[3] != 0).sum()))
                now = ro.alive.tolist()
                alive.append(int(sum(now)))
                for b in range(B):
                    if not now[b] and first_dead[b] is None:
                        first_dead[b] = i + 1
            top = lambda xs: max((x for x in xs if x is not None), default=None)
            name = f"sweeps_{sweeps}_push_{push:g}N"
            walks[name] = dict(sweeps=sweeps, push_y_N=push, push_ticks=[push_from, push_from + push_ticks] if push else None,
                               ticks_until_alive_first_clears=first_dead, alive_at_the_end=alive[-1], alive_per_tick=alive,
                               qp_failures=int(sum(fails)), residual_max_m_per_s=top(resid),
                               lowest_vertex_m=min((x for x in lowest if x is not None), default=None),
                               swing_foot_error_max_m=top(swing), com_error_max_m=top(comerr),
                               residual_per_tick=resid, lowest_vertex_per_tick=lowest, swing_foot_error_m=swing, com_error_m=comerr,
                               base_height_end_m=[round(float(x), 4) if bool(torch.isfinite(x)) else None for x in q[:, 5]],
                               finite_state=bool(torch.isfinite(q).all() and torch.isfinite(v).all()))
            print(name, json.dumps({k: walks[name][k] for k in ("ticks_until_alive_first_clears", "alive_at_the_end", "qp_failures",
                                                                "residual_max_m_per_s", "lowest_vertex_m", "swing_foot_error_max_m",
                                                                "com_error_max_m", "base_height_end_m")}))
            del ro
    res = dict(workload=f"HRP-4, {UNIQ} seeded instances around the initial configuration (soles on the floor), tiled; one session",
               method="HIP events around one launch (tick: around one BatchedRollout.step with feedback, N = 10, one scene, "
                      "walking_model(plant=...) attached, from t = 255), median of `steps` after `warmup`; every plant launch starts "
                      "cold.  integrate is the launch the plant replaces, timed in the same session.  torch: the same step as "
                      "batched torch expressions, timed the same way (3 launches after 1); torch_minus_kernel_abs_max says that "
                      "the two computed the same step",
               bytes_per_robot=dict(plant=PLANT_BYTES, integrate=INTEGRATE_BYTES), steps=args.steps, warmup=args.warmup, rows=rows,
               walk=dict(B=B, t0=t0, ticks=args.walk_ticks, fall_guards=dict(z_min=FALL[0], tilt_max=FALL[1]), runs=walks,
                         note="report only: worst robot per tick (null where no robot has a finite value); a robot leaves `alive` "
                              "when its MPC solve fails or the measurement's guards find it fallen; residual is of the robots the "
                              "plant stepped; whether HRP-4 stays upright is not asserted anywhere"))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

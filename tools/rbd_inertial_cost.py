"""What per-robot inertial parameters cost: ms per launch of `BatchedRobot.evaluate` with an inertial table
(`rbd_eval_inertial_kernel`) whose rows are all the model's own, alternated launch by launch with the shared-model kernel
(`rbd_eval_kernel`, the baseline: this kernel's code is the one `profiles/rbd_cost.json` measured) on the same (q, v): HIP
events around one launch, median of K pairs after W warm-up pairs, at B = 8192 and 65 536 HRP-4 robots around the shipped
initial configuration; ns per robot and GB/s over the bytes the launch moves (q, v and every output, and for the new kernel
the 2000 bytes of the robot's row).  The two launches must return the same bits.

Report only, same session: the closed loop with `feedback=True` on the contact plant, 200 ticks of the shipped walk from
t = 150, one robot per payload of 0, 0.7, 1.0, 1.5, 2.0 and 2.5 kg welded to the torso body at (0.15, 0, 0.1), the MPC not
told (it plans for the scene's mass): ticks alive, distance of the robot's CoM to the MPC's, largest |theta_hat| and largest
|innovation| per robot.  Nothing here is asserted anywhere.

usage: python tools/rbd_inertial_cost.py [--steps K] [--warmup W] [--sizes 8192,65536] [--walk-ticks 200]
                                         [--out profiles/rbd_inertial_cost.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
UNIQ, SEED = 1024, 20251019
PAYLOADS, AT = (0.0, 0.7, 1.0, 1.5, 2.0, 2.5), (0.15, 0.0, 0.1)
FALL = (0.4, 0.5)
IO_BYTES = 8 * (30 + 30 + 21 * 30 + 21 + 30 * 30 + 30 + 21 + 21 + 9)      # q, v and the seven outputs of one robot
ROW_BYTES = 8 * 25 * 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="8192,65536")
    ap.add_argument("--walk-ticks", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rbd_inertial_cost.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import cmpc_amd  # noqa: F401
    from cmpc_amd import rbd, wbc, workloads as wl
    from cmpc_amd.problem import ProblemSpec
    from cmpc_amd.rollout import BatchedRollout

    dev = "cuda:0"
    model = rbd.RobotModel.from_urdf(os.path.join(ROOT, "tests", "golden", "hrp4.urdf"))
    shared = rbd.BatchedRobot(model, device=dev)
    rng = np.random.default_rng(SEED)
    q0 = model.place_on_ground(model.configuration(rbd.HRP4_INITIAL_DEG, degrees=True))
    qu = np.tile(q0, (UNIQ, 1))
    qu[:, 0:3] += rng.normal(scale=0.02, size=(UNIQ, 3))
    qu[:, 22:30] += rng.uniform(-0.2, 0.2, size=(UNIQ, 8))               # arms: the feet stay flat on the ground
    vu = rng.normal(scale=0.05, size=(UNIQ, 30))

    def event_ms(call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = call()
        b.record()
        b.synchronize()
        return out, a.elapsed_time(b)

    rows = []
    for B in (int(x) for x in args.sizes.split(",")):
        q = torch.from_numpy(np.ascontiguousarray(np.tile(qu, (B // UNIQ, 1)))).to(dev)
        v = torch.from_numpy(np.ascontiguousarray(np.tile(vu, (B // UNIQ, 1)))).to(dev)
        table = torch.from_numpy(np.ascontiguousarray(np.tile(model.inertial(), (B, 1, 1)))).to(dev)
        own = rbd.BatchedRobot(model, device=dev, inertial=table)
        ms = dict(shared=[], inertial=[])
        for i in range(args.warmup + args.steps):                       # alternated: both see the same clocks and the same cache
            ev_s, t_s = event_ms(lambda: shared.evaluate(q, v))
            ev_i, t_i = event_ms(lambda: own.evaluate(q, v))
            if i >= args.warmup:
                ms["shared"].append(t_s)
                ms["inertial"].append(t_i)
        same = bool(all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(ev_s, ev_i)))
        med = {k: statistics.median(x) for k, x in ms.items()}
        moved = dict(shared=B * IO_BYTES, inertial=B * (IO_BYTES + ROW_BYTES))
        rows.append(dict(B=B, shared_ms=med["shared"], inertial_ms=med["inertial"], inertial_over_shared=med["inertial"] / med["shared"],
                         ns_per_robot={k: 1e6 * med[k] / B for k in med}, bytes_moved=moved,
                         GBps={k: moved[k] / med[k] / 1e6 for k in med}, same_bits=same,
                         finite=bool(all(torch.isfinite(t).all() for t in ev_i)),
                         launches={k: [round(x, 4) for x in xs] for k, xs in ms.items()}))
        print(json.dumps({k: rows[-1][k] for k in rows[-1] if k != "launches"}))
        del own, table, ev_s, ev_i

    # report only: one robot per payload on the plant, the shipped walk from the end of its initial double support
    B, t0, spec = len(PAYLOADS), 150, ProblemSpec(N=10)
    scene = wl.Scene()
    gait = rbd.Gait(scene, device=dev)
    qp = wbc.BatchedInverseDynamicsQP(foot_size=0.1, mu=0.5, device=dev)
    table = torch.from_numpy(rbd.attach_payload(model.inertial(), model.body_of("torso"), np.array(PAYLOADS), np.array(AT))).to(dev)
    loaded = rbd.BatchedRobot(model, device=dev, inertial=table)
    q = torch.from_numpy(np.tile(q0, (B, 1))).to(dev)
    v = torch.zeros_like(q)
    ro = BatchedRollout(scene, spec, B, device=dev, mu=0.5, feedback=True, mass=model.total_mass)      # (the MPC is not told)
    wm = loaded.walking_model(q, v, gait, q_ref=torch.from_numpy(q0).to(dev), fall=FALL, plant=rbd.Plant(spec.delta, sweeps=30))
    ro.attach_whole_body_tasks(qp, wm)
    com, dcom = scene.nominal_state(np.full(B, t0))
    ro.reset(t0, com, dcom)
    alive_ticks, com_dist, theta, innov, qp_fail = [0] * B, [0.0] * B, [0.0] * B, [0.0] * B, [0] * B
    com_dist_per_tick = []
    for i in range(args.walk_ticks):
        ro.step()
        now = ro.alive.tolist()
        d = wm.last_references.pos_err[:, 12:15].norm(dim=1).tolist()           # the MPC's desired CoM minus the robot's
        th = ro.state[:, 9:12].abs().amax(dim=1).tolist()
        inn = ro.last_measurement.innovation.abs().amax(dim=1).tolist()
        st = ro.last_wbc[3].tolist()
        for b in range(B):
            if now[b]:
                alive_ticks[b] = i + 1
            finite = lambda x: x == x and abs(x) != float("inf")
            if finite(d[b]):
                com_dist[b] = max(com_dist[b], d[b])
            if finite(th[b]):
                theta[b] = max(theta[b], th[b])
            if finite(inn[b]):
                innov[b] = max(innov[b], inn[b])
            qp_fail[b] += int(st[b] != 0 and now[b])
        com_dist_per_tick.append([round(x, 5) if x == x else None for x in d])
    walk = dict(B=B, t0=t0, ticks=args.walk_ticks, payload_kg=list(PAYLOADS), on="torso body", at=list(AT), sweeps=30,
                mpc_mass_kg=model.total_mass, total_mass_kg=loaded.total_mass.tolist(),
                fall_guards=dict(z_min=FALL[0], tilt_max=FALL[1]), ticks_alive=alive_ticks, com_distance_to_mpc_max_m=com_dist,
                theta_hat_abs_max=theta, innovation_abs_max=innov, qp_failures_while_alive=qp_fail,
                base_height_end_m=[round(float(x), 4) if bool(torch.isfinite(x)) else None for x in q[:, 5]],
                com_distance_per_tick_m=com_dist_per_tick,
                note="report only: one robot per payload, welded to the torso body (the reference's box lies loose on the forearms); "
                     "a robot leaves `alive` when its MPC solve ends unusable or the measurement's guards find it fallen; maxima are "
                     "over the ticks with a finite value; whether a payload makes a robot fall sooner is not asserted anywhere")
    print(json.dumps({k: walk[k] for k in walk if k not in ("com_distance_per_tick_m", "note")}))
    res = dict(workload=f"HRP-4, {UNIQ} seeded instances around the initial configuration, tiled; every row of the table the model's own; "
                        "one session",
               method="HIP events around one launch, the shared-model kernel and the per-instance kernel alternated on the same (q, v), "
                      "median of `steps` pairs after `warmup`; bytes_moved: q, v, the seven outputs and, for the per-instance kernel, the "
                      "robot's 2000-byte row", steps=args.steps, warmup=args.warmup,
               bytes_per_robot=dict(shared=IO_BYTES, inertial=IO_BYTES + ROW_BYTES), rows=rows, walk=walk)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

"""What feeding each robot's measured centroidal state back to its MPC costs: ms per launch of `BatchedRobot.measure` (HIP
events, median of K launches after W warm-up launches) at B = 8192 and 65 536 HRP-4 robots, next to `BatchedRobot.integrate`
timed in the same session -- unchanged code, so the yardstick of the commit before --, the bytes each launch moves, and a
whole rollout tick (MPC + evaluate + references + QP + integrate) with and without `feedback=True`: one launch more and none
fewer.  The expectation is that the measure launch is no slower than the integrate launch of the session; the outcome is
recorded either way and nothing is tuned to it.  A report-only leg walks 6 robots for 200 ticks from t = 150 twice -- the MPC
on the recorded momentum, as `tools/walk_cost.py` does, and with `feedback=True` and the model's total mass -- and lists per
tick the MPC instances alive, the robots fed back, the QP failures, the worst CoM error, the worst |innovation| and the
swing-foot error.  Whether the robots stay up is not asserted anywhere.  One session's numbers.

usage: python tools/walk_feedback_cost.py [--steps K] [--warmup W] [--sizes 8192,65536] [--out profiles/walk_feedback_cost.json]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
UNIQ, SEED = 1024, 20261021
# bytes per robot, counted as tools/walk_cost.py counts them (every word once, what a fed-back robot moves):
#   measure    in: centroid 9, pose 21, state 16 words and alive; out: x_meas 20, innovation 9, 11 words of the state
#   integrate  in: q, v, qdd 90 words and hold; out: q, v 60 words
MEASURE_BYTES = 8 * (9 + 21 + 16) + 1 + 8 * (20 + 9 + 11)         # 689
INTEGRATE_BYTES = 8 * 90 + 1 + 8 * 60                              # 1201: the measure launch moves 0.57 of it
FALL = (0.3, 1.0)                                                  # of the report-only walk: CoM height, base tilt in rad


def finite_max(x):
    """Largest finite entry of a tensor as a float, or None (the rows of robots that were not measured are NaN)."""
    x = x[x.isfinite()]
    return round(float(x.max()), 5) if x.numel() else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="8192,65536")
    ap.add_argument("--walk-ticks", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "walk_feedback_cost.json"))
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
    su = rng.normal(size=(UNIQ, 16))

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
        q, v, state = tile(qu), tile(vu), tile(su)
        alive = torch.ones(B, dtype=torch.bool, device=dev)
        ev = robot.evaluate(q, v)
        qdd = tile(rng.normal(scale=5.0, size=(UNIQ, 30)))
        hold = torch.zeros(B, dtype=torch.bool, device=dev)
        # (every launch of the series measures the same robots: the state it rewrites is not an input of the next one's verdict)
        _, mms = timed(lambda: robot.measure(ev, state, alive))
        _, ims = timed(lambda: robot.integrate(q, v, qdd, 0.01, hold=hold))
        fed = int(alive.sum())
        ticks = {}
        for feedback in (False, True):
            ro = BatchedRollout(scene, ProblemSpec(N=10), B, device=dev, mu=0.5, feedback=feedback,
                                mass=model.total_mass if feedback else None)
            qr, vr = q.clone(), torch.zeros_like(v)
            ro.attach_whole_body_tasks(qp, robot.walking_model(qr, vr, gait, q_ref=q_ref))
            com, dcom = scene.nominal_state(np.full(B, 255))
            ro.reset(255, com, dcom)
            _, kms = timed(ro.step, steps=min(args.steps, 5), warmup=2)
            ticks[feedback] = (kms, int(ro.alive.sum()))
            del ro
        med = {k: statistics.median(x) for k, x in dict(measure=mms, integrate=ims, tick=ticks[False][0], tick_fb=ticks[True][0]).items()}
        rows.append(dict(B=B, measure_ms=med["measure"], measure_bytes=B * MEASURE_BYTES, measure_GBps=B * MEASURE_BYTES / med["measure"] / 1e6,
                         integrate_ms=med["integrate"], integrate_bytes=B * INTEGRATE_BYTES,
                         integrate_GBps=B * INTEGRATE_BYTES / med["integrate"] / 1e6,
                         measure_over_integrate_ms=med["measure"] / med["integrate"],
                         measure_over_integrate_bytes=MEASURE_BYTES / INTEGRATE_BYTES,
                         measure_no_slower_than_integrate=bool(med["measure"] <= med["integrate"]), robots_fed_back=fed,
                         tick_ms=med["tick"], tick_feedback_ms=med["tick_fb"], tick_feedback_over_tick=med["tick_fb"] / med["tick"],
                         mpc_alive_after_ticks=dict(without=ticks[False][1], feedback=ticks[True][1]),
                         launches={k: [round(x, 4) for x in xs] for k, xs in dict(measure=mms, integrate=ims, tick=ticks[False][0],
                                                                                  tick_feedback=ticks[True][0]).items()}))
        print(json.dumps(rows[-1]))
        del ev

    # report only: 6 robots, the shipped walk from the end of its initial double support, as today and with feedback
    B, t0 = 6, 150
    hw = np.loadtxt(os.path.join(ROOT, "tests", "golden", "measured_hw_cuhw.txt"))
    walks = {}
    for name, feedback in (("recorded_hw", False), ("feedback", True)):
        q = torch.from_numpy(np.tile(q0, (B, 1))).to(dev)
        v = torch.zeros_like(q)
        ro = BatchedRollout(scene, ProblemSpec(N=10), B, device=dev, mu=0.5, hw_measured=None if feedback else hw, feedback=feedback,
                            mass=model.total_mass if feedback else None)
        wm = robot.walking_model(q, v, gait, q_ref=q_ref, fall=FALL)
        ro.attach_whole_body_tasks(qp, wm)
        com, dcom = scene.nominal_state(np.full(B, t0))
        ro.reset(t0, com, dcom)
        swing, comerr, innov, fails, alive, fed = [], [], [], [], [], []
        for i in range(args.walk_ticks):
            tk = ro.t.clone()
            ro.step()
            r, e = wm.last_references, wm.last_evaluation
            idx = tab["step_idx"][tk.long()].long()
            left_swings = ~tab["support_l"][idx].bool()
            err_l = (r.feet_des[:, 3:6] - e.pose[:, 3:6]).norm(dim=1)
            err_r = (r.feet_des[:, 21:24] - e.pose[:, 9:12]).norm(dim=1)
            swing.append(finite_max(torch.where(left_swings, err_l, err_r)))
            comerr.append(finite_max(r.pos_err[:, 12:15].norm(dim=1)))
            innov.append(finite_max(ro.last_measurement.innovation.abs()) if feedback else None)
            fed.append(int(ro.last_measurement.x_meas.isfinite().all(dim=1).sum()) if feedback else None)
            fails.append(int((ro.last_wbc[3] != 0).sum()))
            alive.append(int(ro.alive.sum()))
        height = [float(x) for x in q[:, 5]]
        walks[name] = dict(feedback=feedback, mass=float(ro.state[0, 14]), qp_failures=int(sum(fails)), qp_failures_per_tick=fails,
                           mpc_alive_per_tick=alive, fed_back_per_tick=fed, swing_foot_error_m=swing, com_error_m=comerr, innovation_abs_max=innov,
                           finite_state=bool(torch.isfinite(q).all() and torch.isfinite(v).all()),
                           base_height_end_m=[round(x, 4) if math.isfinite(x) else None for x in height])
        print(json.dumps({k: walks[name][k] for k in ("feedback", "qp_failures", "finite_state", "base_height_end_m")}),
              "alive at the end:", alive[-1])
        del ro
    res = dict(workload=f"HRP-4, {UNIQ} seeded instances around the initial configuration, tiled; one session",
               method="HIP events around one launch (tick: around one BatchedRollout.step, N = 10, one scene, walking_model "
                      "attached, from t = 255), median of `steps` after `warmup`; integrate is unchanged code timed in the same "
                      "session, the yardstick for the measure launch.  The two tick figures are not the price of the launch: "
                      "the MPC instances differ (without feedback the nominal state at rest, with it the robot's own state and "
                      "the model's mass), and so do their iteration counts; mpc_alive_after_ticks says how they ended",
               bytes_per_robot=dict(measure=MEASURE_BYTES, integrate=INTEGRATE_BYTES),
               steps=args.steps, warmup=args.warmup, rows=rows,
               walk=dict(B=B, t0=t0, ticks=args.walk_ticks, fall_guards=dict(z_min=FALL[0], tilt_max=FALL[1]), runs=walks,
                         note="report only: worst robot per tick (null where no robot has a finite value); swing_foot_error is of "
                              "the foot that is not the step's support foot; innovation is measured minus the MPC's prediction, "
                              "all nine words; fed_back counts the robots the measurement accepted, so a robot that leaves "
                              "mpc_alive while it was fed back was stopped by its MPC solve, not by a guard; whether HRP-4 stays upright in either loop is not asserted anywhere"))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

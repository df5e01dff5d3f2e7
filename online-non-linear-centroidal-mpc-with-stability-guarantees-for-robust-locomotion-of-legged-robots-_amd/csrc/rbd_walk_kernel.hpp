// rbd_walk_kernel.hpp -- device code of the walking loop around the batched rigid-body model (include/cmpc_walk.h),
// gfx950 / CDNA4: the whole-body task references of every robot from its own adapted plan, and the step that turns the
// whole-body QP's acceleration into the next tick's (q, v).
//
// One wavefront (one 64-thread workgroup) owns one robot at a time, as in rbd_kernel.hpp; both routines are a handful of
// flops per robot, so the layout is chosen for the memory side: every input word is loaded once, lane i word i, and every
// output word is stored by the lane of the same index -- consecutive lanes, consecutive words.
//   refs_instance       0. schedule lookup (bounds first), inputs to LDS, one finiteness flag per lane
//                       1. lanes 0, 1: the desired pose, velocity and acceleration of the left and the right foot
//                       2. lanes 0..3: Log(R_des R_cur') of lfoot, rfoot, torso, base
//                       3. lane i < 51: word i of ff, pos_err, vel_err; lane i < 36: word i of feet_des
//   integrate_instance  0. q, v, qdd to LDS, flags   1. lane 0: the base; lanes 6..29: the joints   2. out
//
// Written on the macro layer of cmpc_kernel.hpp (CMPC_DEV, CMPC_LANE, CMPC_SYNC, CMPC_FMA), with the rotation maps and the
// sine / cosine of rbd_kernel.hpp: hipcc compiles it for the product library (csrc/rbd_walk.hip), g++ for the CPU test
// harness (tests/emu/rbd_walk_emu.cpp).  No contraction and no libm trigonometry: the two builds agree bit for bit.
#pragma once
#include "../../include/cmpc_walk.h"
#include "rbd_kernel.hpp"
#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace cmpc_walk {

enum { ND = CMPC_RBD_DOFS, ROWS = CMPC_RBD_ROWS, NACC = CMPC_WALK_ROWS, NFEET = CMPC_WALK_FEET_WORDS };

// The validated gait tables (check_gait); the pointers are device memory in the product library, host arrays in the harness.
struct Gait {
  int32_t S, T_max, n_max;
  const int32_t *T, *step_idx, *n_steps, *step_start, *ss_dur;
  const uint8_t *support_l;
  const double *ang, *init_feet;
  double step_height, delta;
};

// LDS of one robot, in doubles.  refs: the inputs in the order pose, vel, jdqd, com_des, q, v, then the three plan rows
// idx-1, idx, idx+1, one flag word per lane, the desired feet and the four rotation errors.
enum {
  W_POSE = 0, W_VEL = W_POSE + ROWS, W_JDQD = W_VEL + ROWS, W_COM = W_JDQD + ROWS, W_Q = W_COM + 9, W_V = W_Q + ND,
  W_PLAN = W_V + ND, W_IN_END = W_PLAN + 9, W_FLAG = 144, W_FEET = W_FLAG + 64, W_AERR = W_FEET + NFEET,
  REFS_LDS_DOUBLES = W_AERR + 12,
  I_Q = 0, I_V = 32, I_A = 64, I_FLAG = 96, I_QOUT = 160, I_VOUT = 192, INTEGRATE_LDS_DOUBLES = 224
};
static_assert(W_IN_END <= W_FLAG, "the inputs of a robot end before its flag words");

// ---------------------------------------------------------------------------------------------------------------------
// Host: validation.  Returns NULL, or what is wrong.  After it no entry can index outside an array: for every tick of
// a scene 0 <= step_idx < n_steps and step_start[step_idx] <= tick, and every single-support duration a cubic divides
// by is > 0 (entry 0 is the initial double support: the reference gives it 0 and never divides by it).
inline const char *check_gait(int32_t S, int32_t T_max, int32_t n_max, const int32_t *T, const int32_t *step_idx,
                              const int32_t *n_steps, const int32_t *step_start, const int32_t *ss_dur, const uint8_t *support_l,
                              const double *ang, const double *init_feet, double step_height, double delta) {
  if (!T || !step_idx || !n_steps || !step_start || !ss_dur || !support_l || !ang || !init_feet) return "null table";
  if (S < 1 || T_max < 1 || n_max < 1) return "S, T_max and n_steps_max must be >= 1";
  if (!cmpc_rbd::host_finite(delta) || !(delta > 0.0)) return "delta must be finite and > 0";
  if (!cmpc_rbd::host_finite(step_height)) return "step_height must be finite";
  for (int32_t s = 0; s < S; ++s) {
    if (T[s] < 1 || T[s] > T_max) return "T[s] must be in [1, T_max]";
    if (n_steps[s] < 1 || n_steps[s] > n_max) return "n_steps[s] must be in [1, n_steps_max]";
    for (int32_t i = 0; i < n_steps[s]; ++i) {
      const size_t e = (size_t)s * n_max + i;
      if (step_start[e] < 0) return "step_start must be >= 0";
      if (ss_dur[e] < 0 || (i > 0 && ss_dur[e] == 0)) return "ss_dur must be > 0 (>= 0 for entry 0, the initial double support)";
      if (support_l[e] > 1) return "support_l must be 0 or 1";
      for (int k = 0; k < 3; ++k)
        if (!cmpc_rbd::host_finite(ang[3 * e + k])) return "ang must be finite";
    }
    for (int k = 0; k < 12; ++k)
      if (!cmpc_rbd::host_finite(init_feet[12 * (size_t)s + k])) return "init_feet must be finite";
    for (int32_t t = 0; t < T[s]; ++t) {
      const int32_t idx = step_idx[(size_t)s * T_max + t];
      if (idx < 0 || idx >= n_steps[s]) return "step_idx out of range: every tick needs 0 <= step_idx < n_steps[s]";
      if (step_start[(size_t)s * n_max + idx] > t) return "step_start[step_idx[t]] must be <= t";
    }
  }
  return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------
// Device.  One foot's desired [ang, pos], velocity and acceleration (18 words): generate_feet_trajectories_at_time of the
// package's FootTrajectoryGenerator.  plan: the rows idx-1, idx, idx+1 of the robot's own plan (LDS; unused rows are 0).
CMPC_DEV void desired_foot(const Gait &G, int s, int idx, int tt, bool left, const double *plan, double *out) {
#pragma unroll
  for (int k = 0; k < 18; ++k) out[k] = 0.0;
  if (idx == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = G.init_feet[12 * (size_t)s + (left ? 0 : 6) + k];
    return;
  }
  const size_t e = (size_t)s * G.n_max + idx;
  const bool support = (G.support_l[e] != 0) == left;
  const int ss = G.ss_dur[e];
  if (support || tt >= ss) {                                     // pinned to its plan entry: this step's, or the next one's
    const int row = support ? 1 : 2;
    const double *a = G.ang + 3 * (support ? e : e + 1);
#pragma unroll
    for (int k = 0; k < 3; ++k) { out[k] = a[k]; out[3 + k] = plan[3 * row + k]; }
    return;
  }
  // single support: cubic in the plane and the angles, quartic bump in z; t and T in ticks, the rates per second
  const double T = (double)ss, t = (double)tt, T2 = T * T, t2 = t * t, d = G.delta, d2 = d * d;
  const double A = -2.0 / (T2 * T), B = 3.0 / T2;
  const double s0 = A * (t2 * t) + B * t2;
  const double s1 = (3.0 * A * t2 + 2.0 * B * t) / d;
  const double s2 = (6.0 * A * t + 2.0 * B) / d2;
  const double *a0 = G.ang + 3 * (e - 1), *a1 = G.ang + 3 * (e + 1);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double da = a1[k] - a0[k], dp = plan[6 + k] - plan[k];
    out[k] = a0[k] + da * s0;       out[6 + k] = da * s1;  out[12 + k] = da * s2;
    out[3 + k] = plan[k] + dp * s0; out[9 + k] = dp * s1;  out[15 + k] = dp * s2;
  }
  const double h = G.step_height;
  const double Az = 16.0 * h / (T2 * T2), Bz = -32.0 * h / (T2 * T), Cz = 16.0 * h / T2;
  out[5] = Az * (t2 * t2) + Bz * (t2 * t) + Cz * t2;
  out[11] = (4.0 * Az * (t2 * t) + 3.0 * Bz * t2 + 2.0 * Cz * t) / d;
  out[17] = (12.0 * Az * t2 + 6.0 * Bz * t + 2.0 * Cz) / d2;
}

// first row of the task frames lfoot, rfoot, torso, base in the 21 task rows
CMPC_DEV int frame_row(int f) { return f == 0 ? 0 : f == 1 ? 6 : f == 2 ? 15 : 18; }

// One robot.  b: its index; the inputs and outputs are the batch's arrays (outputs may be null); lds: REFS_LDS_DOUBLES.
CMPC_DEV void refs_instance(const Gait &G, size_t b, const int32_t *t_all, const int32_t *scene_id, const double *plan_pos,
                            const double *pose, const double *vel, const double *jdqd, const double *com_des, const double *q,
                            const double *v, const double *q_ref, double *ff, double *pos_err, double *vel_err, double *feet_des,
                            double *lds) {
  const int lane = CMPC_LANE;
  double *IN = lds, *PL = lds + W_PLAN, *FL = lds + W_FLAG, *FD = lds + W_FEET, *AE = lds + W_AERR;

  // 0. the schedule: every index is checked before the table it reads (the same words in every lane)
  const int s = scene_id ? scene_id[b] : 0;
  const int t = t_all[b];
  bool ok = s >= 0 && s < G.S;
  int idx = 0, tt = 0, ss = 0;
  if (ok) ok = t >= 0 && t < G.T[s];
  if (ok) {
    idx = G.step_idx[(size_t)s * G.T_max + t];
    ok = idx + 1 < G.n_steps[s];
  }
  if (ok) {
    tt = t - G.step_start[(size_t)s * G.n_max + idx];
    ss = G.ss_dur[(size_t)s * G.n_max + idx];
  }
  const bool single = ok && idx > 0 && tt < ss;
  bool mine = true;                                              // this lane's words are finite
  for (int i = lane; i < W_IN_END; i += 64) {
    double x = 0.0;
    if (i < W_VEL) x = pose[b * ROWS + i];
    else if (i < W_JDQD) x = vel[b * ROWS + (i - W_VEL)];
    else if (i < W_COM) x = jdqd[b * ROWS + (i - W_JDQD)];
    else if (i < W_Q) x = com_des[b * 9 + (i - W_COM)];
    else if (i < W_V) x = q[b * ND + (i - W_Q)];
    else if (i < W_PLAN) x = v[b * ND + (i - W_V)];
    else if (ok && idx > 0) {                                     // the plan rows in use: idx, idx+1, and idx-1 for the cubic
      const int r = (i - W_PLAN) / 3;
      if (r > 0 || single) x = plan_pos[(b * G.n_max + (size_t)(idx - 1 + r)) * 3 + (i - W_PLAN) % 3];
    }
    IN[i] = x;
    mine = mine && cmpc_rbd::dev_finite(x);
  }
  FL[lane] = mine ? 0.0 : 1.0;
  CMPC_SYNC();
  bool bad = !ok;
  for (int k = 0; k < 64; ++k) bad = bad || FL[k] != 0.0;
  if (bad) {
    const double nan = __builtin_nan("");
    if (lane < NACC) {
      if (ff) ff[b * NACC + lane] = nan;
      if (pos_err) pos_err[b * NACC + lane] = nan;
      if (vel_err) vel_err[b * NACC + lane] = nan;
    }
    if (lane < NFEET && feet_des) feet_des[b * NFEET + lane] = nan;
    CMPC_SYNC();
    return;
  }

  // 1. the desired feet
  if (lane < 2) {
    double out[18];
    desired_foot(G, s, idx, tt, lane == 0, PL, out);
#pragma unroll
    for (int k = 0; k < 18; ++k) FD[18 * lane + k] = out[k];
  }
  CMPC_SYNC();

  // 2. world-frame rotation errors Log(R_des R_cur'); torso and base want the mean of the feet's angle triples
  if (lane < 4) {
    const int r0 = frame_row(lane);
    double wd[3], wc[3], Rd[9], Rc[9], E[9], w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      wd[k] = lane < 2 ? FD[18 * lane + k] : (FD[k] + FD[18 + k]) / 2.0;
      wc[k] = IN[W_POSE + r0 + k];
    }
    cmpc_rbd::exp_so3(wd, Rd);
    cmpc_rbd::exp_so3(wc, Rc);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) E[3 * i + j] = Rd[3 * i] * Rc[3 * j] + Rd[3 * i + 1] * Rc[3 * j + 1] + Rd[3 * i + 2] * Rc[3 * j + 2];
    cmpc_rbd::log_so3(E, w);
#pragma unroll
    for (int k = 0; k < 3; ++k) AE[3 * lane + k] = w[k];
  }
  CMPC_SYNC();

  // 3. out: lane i owns word i of every row
  if (lane < NACC) {
    double a = 0.0, pe = 0.0, ve = 0.0;
    if (lane < ROWS) {
      const int f = lane < 6 ? 0 : lane < 12 ? 1 : lane < 15 ? -1 : lane < 18 ? 2 : 3;
      double dp, dv, da;
      if (f < 0) {                                               // centre of mass
        const int k = lane - 12;
        dp = IN[W_COM + k]; dv = IN[W_COM + 3 + k]; da = IN[W_COM + 6 + k];
      } else if (f < 2) {
        const int k = lane - 6 * f;
        dp = FD[18 * f + k]; dv = FD[18 * f + 6 + k]; da = FD[18 * f + 12 + k];
      } else {
        const int k = lane - frame_row(f);
        dp = 0.0; dv = (FD[6 + k] + FD[24 + k]) / 2.0; da = (FD[12 + k] + FD[30 + k]) / 2.0;
      }
      const bool angular = f >= 0 && lane - frame_row(f) < 3;
      a = da - IN[W_JDQD + lane];
      pe = angular ? AE[3 * f + (lane - frame_row(f))] : dp - IN[W_POSE + lane];
      ve = dv - IN[W_VEL + lane];
    } else if (lane >= ROWS + 6) {                               // the joints hold q_ref; the base dofs have no task
      const int d = lane - ROWS;
      pe = (q_ref ? q_ref[d] : 0.0) - IN[W_Q + d];
      ve = -IN[W_V + d];
    }
    if (ff) ff[b * NACC + lane] = a;
    if (pos_err) pos_err[b * NACC + lane] = pe;
    if (vel_err) vel_err[b * NACC + lane] = ve;
  }
  if (lane < NFEET && feet_des) feet_des[b * NFEET + lane] = FD[lane];
  CMPC_SYNC();
}

// q+ (QO) from q (Q) and the new velocity (VO), all LDS: lane 0 the base, lanes 6..29 the joints (include/cmpc_walk.h).
CMPC_DEV void integrate_pose(const double *Q, const double *VO, double dt, double *QO, int lane) {
  if (lane == 0) {
    const double w[3] = {Q[0], Q[1], Q[2]};
    const double dw[3] = {dt * VO[0], dt * VO[1], dt * VO[2]}, vb[3] = {VO[3], VO[4], VO[5]};
    double R[9], dR[9], Rn[9], wn[3], vw[3];
    cmpc_rbd::exp_so3(w, R);
    cmpc_rbd::exp_so3(dw, dR);
    cmpc_rbd::matmul3(R, dR, Rn);
    cmpc_rbd::log_so3(Rn, wn);
    cmpc_rbd::matvec3(R, vb, vw);
#pragma unroll
    for (int k = 0; k < 3; ++k) { QO[k] = wn[k]; QO[3 + k] = Q[3 + k] + dt * vw[k]; }
  } else if (lane >= 6 && lane < ND) {
    QO[lane] = Q[lane] + dt * VO[lane];
  }
}

// One robot's explicit step in the body-twist convention of include/cmpc_rbd.h; in place is allowed (every word is in LDS
// before the first store).  lds: INTEGRATE_LDS_DOUBLES.
CMPC_DEV void integrate_instance(size_t b, const double *q, const double *v, const double *qdd, double dt, const uint8_t *hold,
                                 double *q_out, double *v_out, double *lds) {
  const int lane = CMPC_LANE;
  double *Q = lds + I_Q, *V = lds + I_V, *A = lds + I_A, *FL = lds + I_FLAG, *QO = lds + I_QOUT, *VO = lds + I_VOUT;
  bool mine = true;
  if (lane < ND) {
    const double qi = q[b * ND + lane], vi = v[b * ND + lane], ai = qdd[b * ND + lane];
    Q[lane] = qi; V[lane] = vi; A[lane] = ai;
    mine = cmpc_rbd::dev_finite(qi) && cmpc_rbd::dev_finite(vi) && cmpc_rbd::dev_finite(ai);
  }
  FL[lane] = mine ? 0.0 : 1.0;
  CMPC_SYNC();
  bool keep = hold && hold[b] != 0;
  for (int k = 0; k < 64; ++k) keep = keep || FL[k] != 0.0;
  if (keep) {
    if (lane < ND) { q_out[b * ND + lane] = Q[lane]; v_out[b * ND + lane] = V[lane]; }
    CMPC_SYNC();
    return;
  }
  if (lane < ND) VO[lane] = V[lane] + dt * A[lane];
  CMPC_SYNC();
  integrate_pose(Q, VO, dt, QO, lane);
  CMPC_SYNC();
  if (lane < ND) { q_out[b * ND + lane] = QO[lane]; v_out[b * ND + lane] = VO[lane]; }
  CMPC_SYNC();
}

}  // namespace cmpc_walk

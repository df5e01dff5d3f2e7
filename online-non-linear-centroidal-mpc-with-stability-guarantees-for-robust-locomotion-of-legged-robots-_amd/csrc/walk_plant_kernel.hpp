// walk_plant_kernel.hpp -- device code of the contact plant of the walking loop (cmpc_walk_plant_step of
// include/cmpc_walk.h), gfx950 / CDNA4: joint torques, an external wrench on the base and a flat frictional floor under the
// eight sole vertices move the robot one tick.  A velocity-level time-stepping scheme, the contact impulses by projected
// Gauss-Seidel on the circular friction cone.
//
// One wavefront (one 64-thread workgroup) owns one robot at a time, as in rbd_walk_kernel.hpp.
//   plant_instance  0. every input word to LDS, lane-strided (M and J: consecutive lanes, consecutive words), one flag word
//                      per lane; hold, foot_mu -- every word is read before the first store
//                   1. lane i < 8: vertex i's arm r_i and height phi_i; lane 8: [R'm; R'f] of the wrench
//                   2. Jc (24 rows) from J and the arms, row 24 = generalised force - h; lane k < 24: Jc[k].v
//                   3. M = L L' in place, row i by lane i; a pivot that is not finite and > 0 refuses the robot
//                   4. lane k < 25: Z[k] = L^-1 (row k), in place        (forward substitution, one lane per right-hand side)
//                   5. W = Z Z' + cfm I (= Jc M^-1 Jc'),  c[k] = Jc[k].v + dt Z[k].Z[24] (= Jc v_free), + the height term
//                   6. lane k < 25: Y[k] = L^-T Z[k], in place           (back substitution);  v_free = v + dt Y[24]
//                   7. warm start made admissible by lane i < 8;  lane j < 24: u_j = (W p + c)_j
//                   8. the sweeps: per vertex the three lanes publish their u, every lane forms the vertex's three new
//                      impulses (the same words in every lane), lane j adds the three changes into u_j -- one LDS hand-off
//                      per vertex, no reduction
//                   9. residual; v+ = v_free + Y p by lane d < 30; q+ by integrate_pose of rbd_walk_kernel.hpp; out
// Every sum runs in the order written here.  The rows of Jc / Z / Y and of M have a stride of 31 words, so that the lanes
// that each walk a row of their own fall on different LDS banks.
//
// Written on the macro layer of cmpc_kernel.hpp (CMPC_DEV, CMPC_LANE, CMPC_SYNC, CMPC_FMA), with the Exp and Log of
// rbd_kernel.hpp: hipcc compiles it for the product library (csrc/walk_plant.hip), g++ for the CPU test harness
// (tests/emu/walk_plant_emu.cpp).  No contraction and no libm: the two builds agree bit for bit.
#pragma once
#include "../../include/cmpc_walk.h"
#include "rbd_walk_kernel.hpp"
#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace cmpc_walk {

enum { NC = 24, NVERT = 8, JROWS = 12, LD = 31, TAU_WORDS = CMPC_RBD_DOFS - 6, PLANT_PER_CU = 6 };

// LDS of one robot, in doubles.
enum {
  P_M = 0,                          // M, then its factor L (lower triangle), rows of LD words
  P_J = P_M + ND * LD,              // the twelve foot rows of J, packed
  P_Z = P_J + JROWS * ND,           // Jc, then Z, then Y: 24 rows and the force row, LD words each
  P_W = P_Z + (NC + 1) * LD,
  P_Q = P_W + NC * NC, P_V = P_Q + 32, P_H = P_V + 32, P_VO = P_H + 32, P_QO = P_VO + 32,
  P_C = P_QO + 32, P_P = P_C + NC, P_U = P_P + 2 * NC, P_POSE = P_U + NC, P_EXT = P_POSE + 24, P_E6 = P_EXT + 8, P_TAU = P_E6 + 8,
  P_ARM = P_TAU + NC, P_PHI = P_ARM + 3 * NVERT, P_JV = P_PHI + NVERT, P_US = P_JV + NC, P_FLAG = P_US + 8,
  PLANT_LDS_DOUBLES = P_FLAG + 64
};
static_assert(PLANT_PER_CU * ((PLANT_LDS_DOUBLES * 8 + 64 + 1279) / 1280) * 1280 <= 160 * 1024, "six robots per CU");

// Host: what is wrong with the arguments of a launch, or NULL.
inline const char *check_plant(int32_t B, const double *q, const double *v, const double *M, const double *h, const double *J,
                               const double *pose, int32_t tau_ld, const double *foot_mu, const cmpc_walk_plant_params *prm,
                               const double *q_out, const double *v_out) {
  if (B < 0) return "negative batch";
  if (!prm) return "null params";
  if (prm->struct_size != (int32_t)sizeof(cmpc_walk_plant_params)) return "params.struct_size is not sizeof(cmpc_walk_plant_params)";
  if (B > 0 && (!q || !v || !M || !h || !J || !pose || !foot_mu || !q_out || !v_out)) return "null q, v, M, h, J, pose, foot_mu, q_out or v_out";
  if (tau_ld < TAU_WORDS) return "tau_ld must be >= 24";
  if (prm->sweeps < 0) return "sweeps must be >= 0";
  if (!cmpc_rbd::host_finite(prm->dt) || !(prm->dt > 0.0)) return "dt must be finite and > 0";
  if (!(prm->erp >= 0.0 && prm->erp <= 1.0)) return "erp must be in [0, 1]";
  if (!cmpc_rbd::host_finite(prm->cfm) || !(prm->cfm >= 0.0)) return "cfm must be finite and >= 0";
  if (!cmpc_rbd::host_finite(prm->ground_z)) return "ground_z must be finite";
  return nullptr;
}

// (x, y) scaled onto the disk of radius mu pn (to 0 when pn = 0); pn >= 0
CMPC_DEV void plant_cone(double mu, double pn, double &px, double &py) {
  const double hyp = __builtin_sqrt(px * px + py * py), lim = mu * pn;
  if (hyp > lim) {
    if (pn > 0.0) {
      const double s = lim / hyp;
      px = px * s; py = py * s;
    } else {
      px = 0.0; py = 0.0;
    }
  }
}

// One robot.  b: its index; the arrays are the batch's (tau, ext, hold, impulse, status, residual may be null);
// lds: PLANT_LDS_DOUBLES.
CMPC_DEV void plant_instance(size_t b, const double *q, const double *v, const double *M, const double *h, const double *J,
                             const double *pose, const double *tau, int tau_ld, const double *ext, const double *foot_mu,
                             const uint8_t *hold, int sweeps, double dt, double ground_z, double erp, double cfm, double *impulse,
                             double *q_out, double *v_out, int32_t *status, double *residual, double *lds) {
  const int lane = CMPC_LANE;
  double *Mm = lds + P_M, *Jm = lds + P_J, *Z = lds + P_Z, *W = lds + P_W, *Q = lds + P_Q, *V = lds + P_V, *H = lds + P_H;
  double *VO = lds + P_VO, *QO = lds + P_QO, *C = lds + P_C, *P = lds + P_P, *U = lds + P_U, *PO = lds + P_POSE, *EX = lds + P_EXT;
  double *E6 = lds + P_E6, *TA = lds + P_TAU, *ARM = lds + P_ARM, *PHI = lds + P_PHI, *JV = lds + P_JV, *US = lds + P_US;
  double *FL = lds + P_FLAG;

  // 0. in: every word this robot's stores could overwrite is read here
  bool mine = true;
  for (int e = lane; e < ND * ND; e += 64) {
    const double x = M[b * (ND * ND) + e];
    Mm[(e / ND) * LD + e % ND] = x;
    mine = mine && cmpc_rbd::dev_finite(x);
  }
  for (int e = lane; e < ROWS * ND; e += 64) {
    const double x = J[b * (ROWS * ND) + e];
    if (e < JROWS * ND) Jm[e] = x;
    mine = mine && cmpc_rbd::dev_finite(x);
  }
  if (lane < ND) {
    const double qi = q[b * ND + lane], vi = v[b * ND + lane], hi = h[b * ND + lane];
    Q[lane] = qi; V[lane] = vi; H[lane] = hi;
    mine = mine && cmpc_rbd::dev_finite(qi) && cmpc_rbd::dev_finite(vi) && cmpc_rbd::dev_finite(hi);
  } else if (lane >= 32 && lane < 32 + ROWS) {
    const double x = pose[b * ROWS + (lane - 32)];
    PO[lane - 32] = x;
    mine = mine && cmpc_rbd::dev_finite(x);
  } else if (lane >= 56 && lane < 62) {
    const double x = ext ? ext[b * 6 + (lane - 56)] : 0.0;
    EX[lane - 56] = x;
    mine = mine && cmpc_rbd::dev_finite(x);
  }
  if (lane < NC) {
    const double t = tau ? tau[b * (size_t)tau_ld + lane] : 0.0, p = impulse ? impulse[b * NC + lane] : 0.0;
    TA[lane] = t; P[lane] = p;
    mine = mine && cmpc_rbd::dev_finite(t) && cmpc_rbd::dev_finite(p);
  }
  const double half = foot_mu[b * 2], mu = foot_mu[b * 2 + 1];
  const bool held = hold && hold[b] != 0;
  FL[lane] = mine ? 0.0 : 1.0;
  CMPC_SYNC();
  if (held) {                                                    // (q, v) keep their bits; the impulse row is not touched
    if (lane < ND) { q_out[b * ND + lane] = Q[lane]; v_out[b * ND + lane] = V[lane]; }
    if (lane == 0 && status) status[b] = 1;
    CMPC_SYNC();
    return;
  }
  bool bad = !(cmpc_rbd::dev_finite(half) && half > 0.0 && cmpc_rbd::dev_finite(mu) && mu > 0.0);
  for (int k = 0; k < 64; ++k) bad = bad || FL[k] != 0.0;

  if (!bad) {
    // 1. the arms and heights of the vertices; the wrench in the base frame
    if (lane <= NVERT) {
      const bool vertex = lane < NVERT;
      const int f = (lane >> 2) & 1;
      const double w[3] = {vertex ? PO[6 * f] : Q[0], vertex ? PO[6 * f + 1] : Q[1], vertex ? PO[6 * f + 2] : Q[2]};
      double R[9];
      cmpc_rbd::exp_so3(w, R);
      if (vertex) {
        const double s[3] = {(lane & 2) ? -half : half, (lane & 1) ? -half : half, 0.0};
        double r[3];
        cmpc_rbd::matvec3(R, s, r);
        ARM[3 * lane] = r[0]; ARM[3 * lane + 1] = r[1]; ARM[3 * lane + 2] = r[2];
        PHI[lane] = (PO[6 * f + 5] + r[2]) - ground_z;
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {                            // R' m, R' f
          E6[k] = R[k] * EX[0] + R[3 + k] * EX[1] + R[6 + k] * EX[2];
          E6[3 + k] = R[k] * EX[3] + R[3 + k] * EX[4] + R[6 + k] * EX[5];
        }
      }
    }
    CMPC_SYNC();

    // 2. Jc[3i + r] = J_lin[r] - (r_i x J_ang)[r]; row 24 = [R'm; R'f; tau] - h
    for (int e = lane; e < NC * ND; e += 64) {
      const int row = e / ND, d = e % ND, i = row / 3, r = row % 3, f = i >> 2;
      const double *a = Jm + (6 * f) * ND + d, *arm = ARM + 3 * i;
      const double a0 = a[0], a1 = a[ND], a2 = a[2 * ND];
      const double cr = r == 0 ? arm[1] * a2 - arm[2] * a1 : r == 1 ? arm[2] * a0 - arm[0] * a2 : arm[0] * a1 - arm[1] * a0;
      Z[row * LD + d] = a[(3 + r) * ND] - cr;
    }
    if (lane < ND) Z[NC * LD + lane] = (lane < 6 ? E6[lane] : TA[lane - 6]) - H[lane];
    CMPC_SYNC();
    if (lane < NC) {
      double s = 0.0;
      for (int d = 0; d < ND; ++d) s = CMPC_FMA(Z[lane * LD + d], V[d], s);
      JV[lane] = s;
    }

    // 3. M = L L', right-looking: row i by lane i
    for (int k = 0; k < ND && !bad; ++k) {
      const double piv = Mm[k * LD + k];                           // the same word in every lane
      if (!(cmpc_rbd::dev_finite(piv) && piv > 0.0)) { bad = true; break; }
      const double lkk = __builtin_sqrt(piv);
      CMPC_SYNC();                                               // every lane has the pivot before lane k overwrites it
      if (lane == k) Mm[k * LD + k] = lkk;
      else if (lane > k && lane < ND) Mm[lane * LD + k] = Mm[lane * LD + k] / lkk;
      CMPC_SYNC();
      if (lane > k && lane < ND) {
        const double lik = Mm[lane * LD + k];
        for (int j = k + 1; j <= lane; ++j) Mm[lane * LD + j] = CMPC_FMA(-lik, Mm[j * LD + k], Mm[lane * LD + j]);
      }
      CMPC_SYNC();
    }
  }

  if (bad) {                                                     // refused: (q, v) keep their bits, the impulse row is zeros
    CMPC_SYNC();
    if (lane < ND) { q_out[b * ND + lane] = Q[lane]; v_out[b * ND + lane] = V[lane]; }
    if (lane < NC && impulse) impulse[b * NC + lane] = 0.0;
    if (lane == 0 && status) status[b] = 2;
    if (lane == 0 && residual) residual[b] = __builtin_nan("");
    CMPC_SYNC();
    return;
  }

  // 4. forward substitution, one lane per right-hand side
  if (lane <= NC) {
    double *x = Z + lane * LD;
    for (int i = 0; i < ND; ++i) {
      double s = x[i];
      for (int j = 0; j < i; ++j) s = CMPC_FMA(-Mm[i * LD + j], x[j], s);
      x[i] = s / Mm[i * LD + i];
    }
  }
  CMPC_SYNC();

  // 5. W and c
  for (int e = lane; e < NC * NC; e += 64) {
    const int a = e / NC, c = e % NC;
    double s = 0.0;
    for (int d = 0; d < ND; ++d) s = CMPC_FMA(Z[a * LD + d], Z[c * LD + d], s);
    W[e] = a == c ? s + cfm : s;
  }
  if (lane < NC) {
    double s = 0.0;
    for (int d = 0; d < ND; ++d) s = CMPC_FMA(Z[lane * LD + d], Z[NC * LD + d], s);
    double c = JV[lane] + dt * s;
    if (lane % 3 == 2) {
      const double phi = PHI[lane / 3];
      c = c + (phi >= 0.0 ? phi : erp * phi) / dt;
    }
    C[lane] = c;
  }
  CMPC_SYNC();

  // 6. back substitution: Y[k] = L^-T Z[k];  v_free
  if (lane <= NC) {
    double *x = Z + lane * LD;
    for (int i = ND - 1; i >= 0; --i) {
      double s = x[i];
      for (int j = i + 1; j < ND; ++j) s = CMPC_FMA(-Mm[j * LD + i], x[j], s);
      x[i] = s / Mm[i * LD + i];
    }
  }
  // 7. the warm start, made admissible
  if (lane < NVERT) {
    const double p2 = P[3 * lane + 2], pn = p2 > 0.0 ? p2 : 0.0;
    double px = P[3 * lane], py = P[3 * lane + 1];
    plant_cone(mu, pn, px, py);
    P[3 * lane] = px; P[3 * lane + 1] = py; P[3 * lane + 2] = pn;
  }
  CMPC_SYNC();
  if (lane < ND) VO[lane] = V[lane] + dt * Z[NC * LD + lane];    // v_free
  double u = 0.0;
  if (lane < NC) {
    u = C[lane];
    for (int k = 0; k < NC; ++k) u = CMPC_FMA(W[k * NC + lane], P[k], u);       // (W is symmetric bit for bit)
  }

  // 8. the sweeps; the impulses alternate between two rows, so that no lane can meet a word of the sweep in progress
  for (int s = 0; s < sweeps; ++s) {
    const double *Pr = P + (s & 1) * NC;
    double *Pw = P + ((s + 1) & 1) * NC;
    for (int i = 0; i < NVERT; ++i) {
      const int x = 3 * i, y = x + 1, n = x + 2;
      double *us = US + 3 * (i & 1);
      if (lane >= x && lane <= n) us[lane - x] = u;
      CMPC_SYNC();
      const double px0 = Pr[x], py0 = Pr[y], pn0 = Pr[n];            // the same words in every lane from here
      const double t = pn0 - us[2] / W[n * NC + n], pn = t > 0.0 ? t : 0.0, dn = pn - pn0;
      const double ux = CMPC_FMA(W[x * NC + n], dn, us[0]);
      double px = px0 - ux / W[x * NC + x];
      const double uy = CMPC_FMA(W[y * NC + x], px - px0, CMPC_FMA(W[y * NC + n], dn, us[1]));
      double py = py0 - uy / W[y * NC + y];
      plant_cone(mu, pn, px, py);
      if (lane < NC)
        u = CMPC_FMA(W[y * NC + lane], py - py0, CMPC_FMA(W[x * NC + lane], px - px0, CMPC_FMA(W[n * NC + lane], dn, u)));
      if (lane == 0) { Pw[x] = px; Pw[y] = py; Pw[n] = pn; }      // read a sweep, eight hand-offs, later
    }
  }
  if (lane < NC) U[lane] = u;
  CMPC_SYNC();
  const double *PF = P + (sweeps & 1) * NC;

  // 9. out
  if (lane < ND) {
    double s = VO[lane];
    for (int k = 0; k < NC; ++k) s = CMPC_FMA(Z[k * LD + lane], PF[k], s);
    VO[lane] = s;
  }
  CMPC_SYNC();
  integrate_pose(Q, VO, dt, QO, lane);
  CMPC_SYNC();
  if (lane < ND) { q_out[b * ND + lane] = QO[lane]; v_out[b * ND + lane] = VO[lane]; }
  if (lane < NC && impulse) impulse[b * NC + lane] = PF[lane];
  if (lane == 0) {
    if (status) status[b] = 0;
    if (residual) {
      double r = 0.0;
      for (int i = 0; i < NVERT; ++i) {
        const double m = -U[3 * i + 2];
        r = m > r ? m : r;
      }
      residual[b] = r;
    }
  }
  CMPC_SYNC();
}

}  // namespace cmpc_walk

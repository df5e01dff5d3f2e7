// rbd_kernel.hpp -- device code of the batched rigid-body model (include/cmpc_rbd.h), gfx950 / CDNA4.
//
// One wavefront (one 64-thread workgroup) owns one robot at a time.  Everything is expressed in WORLD coordinates with the
// world origin as the reference point of every spatial vector ([angular; linear of the point at the origin]), so composite
// quantities are plain sums:
//   1. lane 0: base pose Exp(q[0:3]), its six motion vectors and its twist; lanes 1..24: the joints' local rotations
//   2. by tree level: body poses, joint motion vectors S, body twists V, bias accelerations A (vdot = 0, no gravity)
//   3. one lane per body: spatial inertia about the origin, momentum I V, bias force I A + V x* I V (gravity joins in 5:
//      a subtree's weight is its composite inertia times the acceleration +g, so the bias terms stay exact zeros at rest)
//   4. one lane per component: inertias, forces and momenta summed towards the root (parent[i] < i: one descending loop)
//   5. one lane per dof: F = Ic S; h = S . f; its entries of M by walking the ancestor chain (each value written to both
//      triangles: M is symmetric bit for bit); its column of the task Jacobian.  Lanes 32..36: frame poses, velocities,
//      bias accelerations, and the centroidal state
//   6. M and J leave LDS with unit stride
// The model's tables (cmpc_rbd::Tables) are read from global memory: they are the same for every robot of the launch.
// run_instance<true> (csrc/rbd_inertial.hip, cmpc_rbd_eval_inertial) is the same routine for a fleet whose robots carry their
// own inertial parameters: mass, centre of mass and inertia of every body come from the robot's own row of a device table
// inertial[B][25][10], copied with unit stride into LDS words of its own behind J; kinematics, frames and topology stay in the
// shared Tables.  run_instance<false> is the code it was: the switch is resolved at compile time.
//
// Written on the macro layer of cmpc_kernel.hpp (CMPC_DEV, CMPC_LANE, CMPC_SYNC, CMPC_FMA): hipcc compiles it for the product
// library (csrc/rbd.hip), g++ for the CPU test harness (tests/emu/rbd_emu.cpp), where the lanes are threads and CMPC_SYNC is
// a barrier -- so every cross-lane LDS hand-off carries one.  Both builds form every sum and product in the order written,
// with no contraction (the pragma below; the harness is built with -ffp-contract=off), and sine, cosine and the arc
// tangent are spelled out here from +, *, /, sqrt and rint: the two builds agree bit for bit.
#pragma once
#include "../../include/cmpc_rbd.h"
#include <math.h>
#include <stdint.h>
#ifdef __clang__
#pragma clang fp contract(off)
#endif
#ifndef CMPC_FMA
#define CMPC_FMA(x, y, z) __builtin_fma((x), (y), (z))
#endif

namespace cmpc_rbd {

enum { NB = CMPC_RBD_BODIES, ND = CMPC_RBD_DOFS, NF = CMPC_RBD_FRAMES, ROWS = CMPC_RBD_ROWS };

// The validated model (fill_tables): plain data, copied to the device once.
struct Tables {
  int32_t parent[NB];        // parent[0] = -1
  int32_t depth[NB];         // depth[0] = 0
  int32_t max_depth;
  int32_t frame_body[NF];
  uint32_t moved_by[NB];     // bit d: dof d moves the body (bits 0..5, the base, always)
  double E[NB][9], r[NB][3], axis[NB][3];
  double mass[NB], com[NB][3], inertia[NB][6];
  double fR[NF][9], fp[NF][3];
  double total_mass;
};

// LDS of one robot, in doubles
enum {
  L_Q = 0, L_V = 32, L_R = 64, L_P = L_R + 9 * NB, L_S = L_P + 3 * NB, L_VEL = L_S + 6 * ND,
  L_ACC = L_VEL + 6 * NB, L_I = L_ACC + 6 * NB, L_MOM = L_I + 10 * NB, L_F = L_MOM + 6 * NB, L_M = L_F + 6 * NB,
  L_J = L_M + ND * ND, LDS_DOUBLES = L_J + ROWS * ND,
  // the per-instance kernel: the robot's own row behind J, which nothing else writes (phase 3's zeroing ends at J's end)
  IW = CMPC_RBD_INERTIAL_WORDS, L_IR = LDS_DOUBLES, LDS_DOUBLES_INERTIAL = L_IR + IW * NB
};

// ---------------------------------------------------------------------------------------------------------------------
// Host: validation.  Returns NULL, or what is wrong.
inline bool host_finite(double x) { return __builtin_fabs(x) <= 1.7976931348623157e308; }

inline bool orthonormal(const double *R) {                     // R'R = I to 1e-9 (false for a non-finite entry)
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double d = 0.0;
      for (int k = 0; k < 3; ++k) d += R[3 * k + a] * R[3 * k + b];
      if (!(__builtin_fabs(d - (a == b ? 1.0 : 0.0)) < 1e-9)) return false;
    }
  return true;
}

inline const char *fill_tables(Tables &T, const int32_t *parent, const double *joint_R, const double *joint_p, const double *axis,
                               const double *mass, const double *com, const double *inertia, const int32_t *frame_body,
                               const double *frame_R, const double *frame_p) {
  if (!parent || !joint_R || !joint_p || !axis || !mass || !com || !inertia || !frame_body || !frame_R || !frame_p)
    return "null table";
  T = Tables();
  if (parent[0] != -1) return "parent[0] must be -1 (the floating base)";
  T.parent[0] = -1; T.depth[0] = 0; T.max_depth = 0; T.moved_by[0] = 0x3Fu;
  double total = 0.0;
  for (int i = 0; i < NB; ++i) {
    if (i > 0) {
      if (parent[i] < 0 || parent[i] >= i) return "parents must satisfy 0 <= parent[i] < i";
      T.parent[i] = parent[i];
      T.depth[i] = T.depth[parent[i]] + 1;
      if (T.depth[i] > T.max_depth) T.max_depth = T.depth[i];
      T.moved_by[i] = T.moved_by[parent[i]] | (1u << (5 + i));
      double n2 = 0.0;
      for (int k = 0; k < 3; ++k) {
        if (!host_finite(axis[3 * i + k]) || !host_finite(joint_p[3 * i + k])) return "joint axes and origins must be finite";
        n2 += axis[3 * i + k] * axis[3 * i + k];
      }
      if (!host_finite(n2) || !(n2 > 1e-24)) return "joint axes must be non-zero";
      const double n = __builtin_sqrt(n2);
      for (int k = 0; k < 3; ++k) { T.axis[i][k] = axis[3 * i + k] / n; T.r[i][k] = joint_p[3 * i + k]; }
      if (!orthonormal(joint_R + 9 * i)) return "joint rotations must be orthonormal";
      for (int k = 0; k < 9; ++k) T.E[i][k] = joint_R[9 * i + k];
    } else {
      T.E[0][0] = T.E[0][4] = T.E[0][8] = 1.0;
      T.axis[0][2] = 1.0;
    }
    if (!host_finite(mass[i]) || !(mass[i] >= 0.0)) return "masses must be finite and >= 0";
    T.mass[i] = mass[i];
    total += mass[i];
    for (int k = 0; k < 3; ++k) {
      if (!host_finite(com[3 * i + k])) return "centres of mass must be finite";
      T.com[i][k] = com[3 * i + k];
    }
    for (int k = 0; k < 6; ++k) {
      if (!host_finite(inertia[6 * i + k])) return "inertias must be finite";
      T.inertia[i][k] = inertia[6 * i + k];
    }
  }
  if (!host_finite(total) || !(total > 0.0)) return "the total mass must be > 0";
  T.total_mass = total;
  for (int f = 0; f < NF; ++f) {
    if (frame_body[f] < 0 || frame_body[f] >= NB) return "frame bodies must be in range";
    T.frame_body[f] = frame_body[f];
    for (int k = 0; k < 9; ++k) {
      if (!host_finite(frame_R[9 * f + k])) return "frame placements must be finite";
      T.fR[f][k] = frame_R[9 * f + k];
    }
    for (int k = 0; k < 3; ++k) {
      if (!host_finite(frame_p[3 * f + k])) return "frame placements must be finite";
      T.fp[f][k] = frame_p[3 * f + k];
    }
    if (!orthonormal(frame_R + 9 * f)) return "frame rotations must be orthonormal";
  }
  return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------
// Device: small algebra
CMPC_DEV void cross3(const double *a, const double *b, double *c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
CMPC_DEV double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
CMPC_DEV double dot6(const double *a, const double *b) { return dot3(a, b) + dot3(a + 3, b + 3); }
// c = A b, c = A B (row-major 3x3)
CMPC_DEV void matvec3(const double *A, const double *b, double *c) {
#pragma unroll
  for (int i = 0; i < 3; ++i) c[i] = A[3 * i] * b[0] + A[3 * i + 1] * b[1] + A[3 * i + 2] * b[2];
}
CMPC_DEV void matmul3(const double *A, const double *B, double *C) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
// symmetric 3x3 (xx xy xz yy yz zz) times vector
CMPC_DEV void symvec3(const double *s, const double *b, double *c) {
  c[0] = s[0] * b[0] + s[1] * b[1] + s[2] * b[2];
  c[1] = s[1] * b[0] + s[3] * b[1] + s[4] * b[2];
  c[2] = s[2] * b[0] + s[4] * b[1] + s[5] * b[2];
}
// spatial inertia about the origin (m, h = m c, I_O: 10 words) times a motion vector [w; v]: [I_O w + h x v; m v - h x w]
CMPC_DEV void inertia_apply(const double *I, const double *V, double *F) {
  double a[3], b[3];
  symvec3(I + 4, V, a);
  cross3(I + 1, V + 3, b);
  F[0] = a[0] + b[0]; F[1] = a[1] + b[1]; F[2] = a[2] + b[2];
  cross3(I + 1, V, b);
  F[3] = I[0] * V[3] - b[0]; F[4] = I[0] * V[4] - b[1]; F[5] = I[0] * V[5] - b[2];
}

CMPC_DEV bool dev_finite(double x) { return __builtin_fabs(x) <= 1.7976931348623157e308; }

// sine and cosine from + and * alone (Cody-Waite reduction by pi/2 in two parts, minimax kernels on [-pi/4, pi/4]): about
// 1 ulp for the |x| of joint angles, and the same bits from both builds of this source.  NaN for a non-finite x.
CMPC_DEV void sincos_d(double x, double *sn, double *cs) {
  if (!dev_finite(x)) { *sn = *cs = x - x; return; }            // (no integer is formed from a NaN below)
  const double kf = __builtin_rint(x * 6.36619772367581382433e-01);
  double r = CMPC_FMA(-kf, 1.57079632673412561417e+00, x);
  r = CMPC_FMA(-kf, 6.07710050650619224932e-11, r);
  const double z = r * r;
  const double ps = -1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04
                    + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10))));
  const double pc = 4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05
                    + z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))));
  const double s = r + r * z * ps;
  const double c = 1.0 - 0.5 * z + z * z * pc;
  const int n = (int)(kf - 4.0 * __builtin_floor(kf * 0.25));     // 0..3 for every finite x
  const double s1 = (n & 1) ? c : s, c1 = (n & 1) ? s : c;
  *sn = (n & 2) ? -s1 : s1;
  *cs = ((n + 1) & 2) ? -c1 : c1;
}

// R = Exp(w^): series for small angles
CMPC_DEV void exp_so3(const double *w, double *R) {
  const double t2 = dot3(w, w);
  double A, B;
  if (t2 < 1e-6) {
    A = 1.0 - t2 * (1.0 / 6.0 - t2 * (1.0 / 120.0 - t2 * (1.0 / 5040.0)));
    B = 0.5 - t2 * (1.0 / 24.0 - t2 * (1.0 / 720.0 - t2 * (1.0 / 40320.0)));
  } else {
    const double t = __builtin_sqrt(t2);
    double s, c;
    sincos_d(t, &s, &c);
    A = s / t;
    B = (1.0 - c) / t2;
  }
  R[0] = 1.0 + B * (w[0] * w[0] - t2); R[1] = B * (w[0] * w[1]) - A * w[2];  R[2] = B * (w[0] * w[2]) + A * w[1];
  R[3] = B * (w[0] * w[1]) + A * w[2]; R[4] = 1.0 + B * (w[1] * w[1] - t2);  R[5] = B * (w[1] * w[2]) - A * w[0];
  R[6] = B * (w[0] * w[2]) - A * w[1]; R[7] = B * (w[1] * w[2]) + A * w[0];  R[8] = 1.0 + B * (w[2] * w[2] - t2);
}

// rotation by angle q about the unit axis a
CMPC_DEV void rot_axis(const double *a, double q, double *R) {
  double s, c;
  sincos_d(q, &s, &c);
  const double B = 1.0 - c;
  R[0] = 1.0 + B * (a[0] * a[0] - 1.0); R[1] = B * (a[0] * a[1]) - s * a[2];  R[2] = B * (a[0] * a[2]) + s * a[1];
  R[3] = B * (a[0] * a[1]) + s * a[2];  R[4] = 1.0 + B * (a[1] * a[1] - 1.0); R[5] = B * (a[1] * a[2]) - s * a[0];
  R[6] = B * (a[0] * a[2]) - s * a[1];  R[7] = B * (a[1] * a[2]) + s * a[0];  R[8] = 1.0 + B * (a[2] * a[2] - 1.0);
}

// w = Log(R): the rotation vector.  s = vee(R - R')/2 = sin(t) axis, c = (tr R - 1)/2 = cos(t); t = atan2(|s|, c) by a
// coarse estimate (error < 4e-3) and three Newton steps t += asin(sin(t* - t)), each of fifth order.  R = I gives exact
// zeros.  Within 1e-7 of pi the axis comes from the diagonal (sign not fixed: only finiteness is promised there).
CMPC_DEV void log_so3(const double *R, double *w) {
  const double s[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
  const double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
  const double s2 = dot3(s, s);
  if (s2 < 1e-8 && c > 0.0) {                                  // asin(x)/x = 1 + x^2/6 + 3 x^4/40 + ...
    const double f = 1.0 + s2 * (1.0 / 6.0 + s2 * (3.0 / 40.0 + s2 * (15.0 / 336.0)));
    w[0] = s[0] * f; w[1] = s[1] * f; w[2] = s[2] * f;
    return;
  }
  const double sn = __builtin_sqrt(s2);
  const double PI = 3.14159265358979323846;
  if (!(sn > 1e-7)) {
    const double d = 1.0 - c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double e = (R[4 * k] - c) / d;
      w[k] = PI * __builtin_sqrt(e > 0.0 ? e : 0.0);
    }
    return;
  }
  const double nrm = __builtin_sqrt(s2 + c * c);
  const double y = sn / nrm, x = c / nrm, ax = __builtin_fabs(x);
  const double t = (ax < y ? ax : y) / (ax < y ? y : ax);
  double a = t * (0.78539816339744830962 + 0.273 * (1.0 - t));
  if (y > ax) a = 0.5 * PI - a;
  if (x < 0.0) a = PI - a;
#pragma unroll 1
  for (int it = 0; it < 3; ++it) {
    double sa, ca;
    sincos_d(a, &sa, &ca);
    const double d = y * ca - x * sa;
    a = a + (d + d * d * d * (1.0 / 6.0));
  }
  const double f = a / sn;
  w[0] = s[0] * f; w[1] = s[1] * f; w[2] = s[2] * f;
}

// ---------------------------------------------------------------------------------------------------------------------
// One robot.  q, v and the outputs point at the instance's own rows (outputs may be null); lds: LDS_DOUBLES doubles.
// INERTIAL: irow is the robot's own [25][10] row (mass, com xyz, inertia xx xy xz yy yz zz per body) and lds has
// LDS_DOUBLES_INERTIAL doubles; T's mass, com, inertia and total_mass are not read.
template <bool INERTIAL = false>
CMPC_DEV void run_instance(const Tables *T, const double *q, const double *v, double g, double *J, double *jdqd, double *M,
                           double *h, double *pose, double *vel, double *centroid, double *lds, const double *irow = nullptr) {
  const int lane = CMPC_LANE;
  double *Q = lds + L_Q, *Vq = lds + L_V, *Rw = lds + L_R, *Pw = lds + L_P, *S = lds + L_S, *VEL = lds + L_VEL;
  double *ACC = lds + L_ACC, *IN = lds + L_I, *MOM = lds + L_MOM, *FRC = lds + L_F, *Ml = lds + L_M, *Jl = lds + L_J;

  // 0. the instance's row; a non-finite word anywhere in it -- or a base rotation vector whose squared norm is not finite --
  // makes every output NaN.  Every lane writes a flag word of its own (in M's window, idle until phase 3) and all of them
  // read the thirty (INERTIAL: the sixty-four): no word has two writers.
  double *IR = lds + L_IR;                                        // (INERTIAL only: the end of lds otherwise)
  double mtot_own = 0.0;
  if constexpr (INERTIAL) {
    // the robot's own row as well, with unit stride: lane l copies words l, l + 64, ... and judges the words it copied (a
    // non-finite word, or a mass < 0: word 0 of a body's ten), so here every one of the 64 lanes writes a flag word
    double flag = 0.0;
    if (lane < ND) {
      const double qi = q[lane], vi = v[lane];
      Q[lane] = qi; Vq[lane] = vi;
      if (!(dev_finite(qi) && dev_finite(vi))) flag = 1.0;
    }
    for (int i = lane; i < IW * NB; i += 64) {
      const double w = irow[i];
      IR[i] = w;
      if (!dev_finite(w) || (i % IW == 0 && !(w >= 0.0))) flag = 1.0;
    }
    Ml[lane] = flag;
  } else if (lane < ND) {
    const double qi = q[lane], vi = v[lane];
    Q[lane] = qi; Vq[lane] = vi;
    Ml[lane] = (dev_finite(qi) && dev_finite(vi)) ? 0.0 : 1.0;
  }
  CMPC_SYNC();
  bool bad = !dev_finite(Q[0] * Q[0] + Q[1] * Q[1] + Q[2] * Q[2]);
  for (int k = 0; k < ND; ++k) bad = bad || Ml[k] != 0.0;
  if constexpr (INERTIAL) {
    for (int k = ND; k < 64; ++k) bad = bad || Ml[k] != 0.0;
    // the total in fill_tables' order, bodies 0 .. 24, by every lane for itself: the same bits in all of them
    for (int i = 0; i < NB; ++i) mtot_own += IR[IW * i];
    bad = bad || !dev_finite(mtot_own) || !(mtot_own > 0.0);
  }
  if (bad) {
    const double nan = __builtin_nan("");
    if (J) for (int i = lane; i < ROWS * ND; i += 64) J[i] = nan;
    if (M) for (int i = lane; i < ND * ND; i += 64) M[i] = nan;
    if (lane < ND && h) h[lane] = nan;
    if (lane < ROWS) {
      if (jdqd) jdqd[lane] = nan;
      if (pose) pose[lane] = nan;
      if (vel) vel[lane] = nan;
    }
    if (lane < 9 && centroid) centroid[lane] = nan;
    CMPC_SYNC();
    return;
  }

  // 1. base pose, motion vectors and twist (lane 0); the joints' rotations parent <- child (lanes 1..24, in registers)
  double El[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) El[k] = 0.0;
  if (lane == 0) {
    const double w[3] = {Q[0], Q[1], Q[2]}, p[3] = {Q[3], Q[4], Q[5]};
    double R[9];
    exp_so3(w, R);
#pragma unroll
    for (int k = 0; k < 9; ++k) Rw[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) Pw[k] = p[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double col[3] = {R[k], R[3 + k], R[6 + k]};
      double pc[3];
      cross3(p, col, pc);
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        S[6 * k + e] = col[e]; S[6 * k + 3 + e] = pc[e];
        S[6 * (3 + k) + e] = 0.0; S[6 * (3 + k) + 3 + e] = col[e];
      }
    }
    const double wb[3] = {Vq[0], Vq[1], Vq[2]}, vb[3] = {Vq[3], Vq[4], Vq[5]};
    double om[3], vl[3], po[3];
    matvec3(R, wb, om);
    matvec3(R, vb, vl);
    cross3(p, om, po);
#pragma unroll
    for (int e = 0; e < 3; ++e) { VEL[e] = om[e]; VEL[3 + e] = vl[e] + po[e]; ACC[e] = 0.0; ACC[3 + e] = 0.0; }
  } else if (lane < NB) {
    double Rq[9];
    rot_axis(T->axis[lane], Q[5 + lane], Rq);
    matmul3(T->E[lane], Rq, El);
  }
  CMPC_SYNC();

  // 2. down the tree, one level per step
  const int max_depth = T->max_depth;
  const int my_depth = lane < NB ? T->depth[lane] : -1;
  const int par = (lane > 0 && lane < NB) ? T->parent[lane] : 0;
  for (int lev = 1; lev <= max_depth; ++lev) {
    if (my_depth == lev) {
      double Rp[9], pp[3], R[9], p[3], a[3], pa[3];
#pragma unroll
      for (int k = 0; k < 9; ++k) Rp[k] = Rw[9 * par + k];
#pragma unroll
      for (int k = 0; k < 3; ++k) pp[k] = Pw[3 * par + k];
      matmul3(Rp, El, R);
      matvec3(Rp, T->r[lane], p);
#pragma unroll
      for (int k = 0; k < 3; ++k) p[k] = pp[k] + p[k];
      matvec3(R, T->axis[lane], a);
      cross3(p, a, pa);
#pragma unroll
      for (int k = 0; k < 9; ++k) Rw[9 * lane + k] = R[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) { Pw[3 * lane + k] = p[k]; S[6 * (5 + lane) + k] = a[k]; S[6 * (5 + lane) + 3 + k] = pa[k]; }
      const double qd = Vq[5 + lane];
      double Vp[6], c1[3], c2[3], c3[3];
#pragma unroll
      for (int k = 0; k < 6; ++k) Vp[k] = VEL[6 * par + k];
      cross3(Vp, a, c1);                    // the parent's twist x S (S x S = 0: the body's own gives the same)
      cross3(Vp, pa, c2);
      cross3(Vp + 3, a, c3);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        VEL[6 * lane + k] = Vp[k] + a[k] * qd;
        VEL[6 * lane + 3 + k] = Vp[3 + k] + pa[k] * qd;
        ACC[6 * lane + k] = ACC[6 * par + k] + c1[k] * qd;
        ACC[6 * lane + 3 + k] = ACC[6 * par + 3 + k] + (c2[k] + c3[k]) * qd;
      }
    }
    CMPC_SYNC();
  }

  // 3. per body: spatial inertia about the world origin, momentum, bias force
  if (lane < NB) {
    double R[9], c[3], t[9], Ic[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = Rw[9 * lane + k];
    const double *ir = INERTIAL ? IR + IW * lane : nullptr;      // the body's own ten words
    matvec3(R, INERTIAL ? ir + 1 : T->com[lane], c);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = Pw[3 * lane + k] + c[k];
    const double *ib = INERTIAL ? ir + 4 : T->inertia[lane];
    const double Ib[9] = {ib[0], ib[1], ib[2], ib[1], ib[3], ib[4], ib[2], ib[4], ib[5]};
    matmul3(R, Ib, t);
    // Ic = t R' (its upper triangle is used)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Ic[3 * i + j] = t[3 * i] * R[3 * j] + t[3 * i + 1] * R[3 * j + 1] + t[3 * i + 2] * R[3 * j + 2];
    const double m = INERTIAL ? ir[0] : T->mass[lane], cc = dot3(c, c);
    double I[10];
    I[0] = m; I[1] = m * c[0]; I[2] = m * c[1]; I[3] = m * c[2];
    I[4] = Ic[0] + m * (cc - c[0] * c[0]); I[5] = 0.5 * (Ic[1] + Ic[3]) - m * (c[0] * c[1]); I[6] = 0.5 * (Ic[2] + Ic[6]) - m * (c[0] * c[2]);
    I[7] = Ic[4] + m * (cc - c[1] * c[1]); I[8] = 0.5 * (Ic[5] + Ic[7]) - m * (c[1] * c[2]);
    I[9] = Ic[8] + m * (cc - c[2] * c[2]);
    double V[6], A[6], P[6], F[6], x1[3], x2[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) { V[k] = VEL[6 * lane + k]; A[k] = ACC[6 * lane + k]; }
    inertia_apply(I, V, P);
    inertia_apply(I, A, F);
    cross3(V, P, x1);                       // V x* P = [w x n + v x f; w x f]
    cross3(V + 3, P + 3, x2);
#pragma unroll
    for (int k = 0; k < 3; ++k) F[k] = F[k] + (x1[k] + x2[k]);
    cross3(V, P + 3, x1);
#pragma unroll
    for (int k = 0; k < 3; ++k) F[3 + k] = F[3 + k] + x1[k];
#pragma unroll
    for (int k = 0; k < 10; ++k) IN[10 * lane + k] = I[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) { MOM[6 * lane + k] = P[k]; FRC[6 * lane + k] = F[k]; }
  }
  for (int i = lane; i < ND * ND + ROWS * ND; i += 64) Ml[i] = 0.0;       // (M and J are adjacent)
  CMPC_SYNC();

  // 4. towards the root: composite inertias, subtree forces and momenta; one lane per component, so no hand-off inside
  if (lane < 22) {
    double *X = lane < 10 ? IN + lane : lane < 16 ? FRC + (lane - 10) : MOM + (lane - 16);
    const int stride = lane < 10 ? 10 : 6;
    for (int i = NB - 1; i > 0; --i) {
      const int pi = T->parent[i];
      X[stride * pi] = X[stride * pi] + X[stride * i];
    }
  }
  CMPC_SYNC();

  // 5. one lane per dof; lanes 32..35 the task frames, lane 36 the centroidal state
  const double mtot = INERTIAL ? mtot_own : T->total_mass;
  if (lane < ND) {
    const int b = lane < 6 ? 0 : lane - 5;
    double Sj[6], Ic[10], F[6], Fb[6], W[6];
    const double G[6] = {0.0, 0.0, 0.0, 0.0, 0.0, g};             // gravity (0, 0, -g) as an acceleration +g of every body
#pragma unroll
    for (int k = 0; k < 6; ++k) { Sj[k] = S[6 * lane + k]; Fb[k] = FRC[6 * b + k]; }
#pragma unroll
    for (int k = 0; k < 10; ++k) Ic[k] = IN[10 * b + k];
    inertia_apply(Ic, Sj, F);
    inertia_apply(Ic, G, W);
#pragma unroll
    for (int k = 0; k < 6; ++k) Fb[k] = Fb[k] + W[k];
    if (h) h[lane] = dot6(Sj, Fb);
    if (lane >= 6) {
      for (int k = b; k > 0; k = T->parent[k]) {
        const double val = dot6(S + 6 * (5 + k), F);
        Ml[ND * lane + 5 + k] = val;
        Ml[ND * (5 + k) + lane] = val;
      }
    }
    const int nbase = lane < 6 ? lane + 1 : 6;
    for (int d = 0; d < nbase; ++d) {
      const double val = dot6(S + 6 * d, F);
      Ml[ND * lane + d] = val;
      Ml[ND * d + lane] = val;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) Jl[ND * (12 + k) + lane] = F[3 + k] / mtot;
    for (int f = 0; f < NF; ++f) {
      const int fb = T->frame_body[f];
      if ((T->moved_by[fb] >> lane) & 1u) {
        const int r0 = f == 0 ? 0 : f == 1 ? 6 : f == 2 ? 15 : 18;
#pragma unroll
        for (int k = 0; k < 3; ++k) Jl[ND * (r0 + k) + lane] = Sj[k];
        if (f < 2) {
          double x[3], wx[3];
          matvec3(Rw + 9 * fb, T->fp[f], x);
#pragma unroll
          for (int k = 0; k < 3; ++k) x[k] = Pw[3 * fb + k] + x[k];
          cross3(Sj, x, wx);
#pragma unroll
          for (int k = 0; k < 3; ++k) Jl[ND * (r0 + 3 + k) + lane] = Sj[3 + k] + wx[k];
        }
      }
    }
  } else if (lane >= 32 && lane < 32 + NF) {
    const int f = lane - 32, fb = T->frame_body[f];
    const int r0 = f == 0 ? 0 : f == 1 ? 6 : f == 2 ? 15 : 18;
    double Rf[9], w[3], V[6], A[6];
    matmul3(Rw + 9 * fb, T->fR[f], Rf);
    log_so3(Rf, w);
#pragma unroll
    for (int k = 0; k < 6; ++k) { V[k] = VEL[6 * fb + k]; A[k] = ACC[6 * fb + k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (pose) pose[r0 + k] = w[k];
      if (vel) vel[r0 + k] = V[k];
      if (jdqd) jdqd[r0 + k] = A[k];
    }
    if (f < 2) {
      double x[3], vx[3], ax[3], wv[3];
      matvec3(Rw + 9 * fb, T->fp[f], x);
#pragma unroll
      for (int k = 0; k < 3; ++k) x[k] = Pw[3 * fb + k] + x[k];
      cross3(V, x, vx);
#pragma unroll
      for (int k = 0; k < 3; ++k) vx[k] = V[3 + k] + vx[k];
      cross3(A, x, ax);
      cross3(V, vx, wv);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (pose) pose[r0 + 3 + k] = x[k];
        if (vel) vel[r0 + 3 + k] = vx[k];
        if (jdqd) jdqd[r0 + 3 + k] = A[3 + k] + ax[k] + wv[k];
      }
    }
  } else if (lane == 32 + NF) {
    double c[3], cd[3], P[6], cp[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) P[k] = MOM[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) { c[k] = IN[1 + k] / mtot; cd[k] = P[3 + k] / mtot; }
    cross3(c, P + 3, cp);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (pose) pose[12 + k] = c[k];
      if (vel) vel[12 + k] = cd[k];
      if (jdqd) jdqd[12 + k] = FRC[3 + k] / mtot;
      if (centroid) { centroid[k] = c[k]; centroid[3 + k] = cd[k]; centroid[6 + k] = P[k] - cp[k]; }
    }
  }
  CMPC_SYNC();

  // 6. out, with unit stride
  if (M) for (int i = lane; i < ND * ND; i += 64) M[i] = Ml[i];
  if (J) for (int i = lane; i < ROWS * ND; i += 64) J[i] = Jl[i];
  CMPC_SYNC();
}

}  // namespace cmpc_rbd

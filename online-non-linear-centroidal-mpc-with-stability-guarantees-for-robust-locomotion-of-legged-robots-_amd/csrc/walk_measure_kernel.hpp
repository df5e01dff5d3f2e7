// walk_measure_kernel.hpp -- device code of the measurement that closes the walking loop (cmpc_walk_measure of
// include/cmpc_walk.h), gfx950 / CDNA4: the robot's own centroid and foot angles become the state the MPC's next record is
// built from, unless the robot is dead, its evaluation is not finite, or it has fallen.
//
// One wavefront (one 64-thread workgroup) owns one robot at a time, as in rbd_walk_kernel.hpp; the routine is a copy, one
// subtraction per word and one Exp, so the layout is chosen for the memory side: every input word is loaded once, lane i
// word i, and every output word is stored by the lane of its index.
//   measure_instance  0. lanes 0..29: centroid and pose to LDS, one finiteness flag per lane; lanes 32..47: the state;
//                        alive[b] -- every word is read before the first store
//                     1. every lane: the flags, the height and the tilt of the base (the same words in every lane)
//                     2. out: lane i < 20 word i of x_meas, lane i < 9 word i of innovation and of the state,
//                        lanes 12, 13 the two foot angles, lane 0 alive[b]
//
// Written on the macro layer of cmpc_kernel.hpp (CMPC_DEV, CMPC_LANE, CMPC_SYNC), with the Exp of rbd_kernel.hpp: hipcc
// compiles it for the product library (csrc/walk_measure.hip), g++ for the CPU test harness
// (tests/emu/walk_measure_emu.cpp).  No contraction and no libm trigonometry: the two builds agree bit for bit.
#pragma once
#include "../../include/cmpc_walk.h"
#include "rbd_kernel.hpp"
#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace cmpc_walk {

// LDS of one robot, in doubles: centroid 9 and pose 21 in one row, the state, one flag word per lane.
enum {
  MS_CEN = 0, MS_POSE = 9, MS_IN_END = MS_POSE + CMPC_RBD_ROWS, MS_STATE = 32, MS_STATE_END = MS_STATE + 16, MS_FLAG = 64,
  MEASURE_LDS_DOUBLES = MS_FLAG + 64,
  MS_XMEAS = 20, MS_INNOV = 9
};
static_assert(MS_IN_END <= MS_STATE && MS_STATE_END <= MS_FLAG, "a robot's inputs, its state and its flag words do not overlap");

// Host: what is wrong with the arguments of a launch, or NULL.
inline const char *check_measure(int32_t B, const double *centroid, const double *pose, double z_min, double cos_tilt_min,
                                 const double *state) {
  if (B < 0) return "negative batch";
  if (z_min != z_min || cos_tilt_min != cos_tilt_min) return "z_min and cos_tilt_min must not be NaN (-INFINITY disables a guard)";
  if (B > 0 && (!centroid || !pose || !state)) return "null centroid, pose or state";
  return nullptr;
}

// One robot.  b: its index; the arrays are the batch's (alive, x_meas and innovation may be null); lds: MEASURE_LDS_DOUBLES.
CMPC_DEV void measure_instance(size_t b, const double *centroid, const double *pose, double z_min, double cos_tilt_min,
                               double *state, uint8_t *alive, double *x_meas, double *innovation, double *lds) {
  const int lane = CMPC_LANE;
  double *IN = lds, *PO = lds + MS_POSE, *ST = lds + MS_STATE, *FL = lds + MS_FLAG;

  // 0. in: every word this robot's stores could overwrite is read here
  bool mine = true;
  if (lane < MS_IN_END) {
    const double x = lane < MS_POSE ? centroid[b * 9 + lane] : pose[b * CMPC_RBD_ROWS + (lane - MS_POSE)];
    IN[lane] = x;
    mine = cmpc_rbd::dev_finite(x);
  } else if (lane >= MS_STATE && lane < MS_STATE_END) {
    ST[lane - MS_STATE] = state[b * 16 + (lane - MS_STATE)];
  }
  FL[lane] = mine ? 0.0 : 1.0;
  const bool dead = alive && alive[b] == 0;
  CMPC_SYNC();

  // 1. the verdict, the same in every lane
  bool bad = false;
  for (int k = 0; k < MS_IN_END; ++k) bad = bad || FL[k] != 0.0;
  bool stop = dead || bad;
  if (!stop) {
    const double w[3] = {PO[18], PO[19], PO[20]};
    double R[9];
    cmpc_rbd::exp_so3(w, R);
    stop = !(IN[MS_CEN + 2] > z_min) || !(R[8] > cos_tilt_min);
  }
  if (stop) {
    const double nan = __builtin_nan("");
    if (lane < MS_XMEAS && x_meas) x_meas[b * MS_XMEAS + lane] = nan;
    if (lane < MS_INNOV && innovation) innovation[b * MS_INNOV + lane] = nan;
    if (lane == 0 && alive && !dead) alive[b] = 0;
    CMPC_SYNC();
    return;
  }

  // 2. out
  if (lane < MS_XMEAS && x_meas) {
    double x = 0.0;                                               // words 15 and 19
    if (lane < 9) x = IN[lane];
    else if (lane < 12) x = ST[lane];                             // theta_hat: the MPC's own
    else if (lane < 15) x = PO[2 + (lane - 12)];                  // lfoot: third angle, then x, y
    else if (lane >= 16 && lane < 19) x = PO[8 + (lane - 16)];    // rfoot
    x_meas[b * MS_XMEAS + lane] = x;
  }
  if (lane < 9) {
    if (innovation) innovation[b * MS_INNOV + lane] = IN[lane] - ST[lane];
    state[b * 16 + lane] = IN[lane];
  } else if (lane == 12 || lane == 13) {
    state[b * 16 + lane] = PO[lane == 12 ? 2 : 8];
  }
  CMPC_SYNC();
}

}  // namespace cmpc_walk

// walk_plant_emu_main.cpp -- TEST HARNESS ONLY.  A stand-alone program around walk_plant_emu.cpp for sanitizer builds
// (-fsanitize=address,undefined): runs the device source of cmpc_walk_plant_step on a small batch authored here -- three
// ordinary robots, a held one, a NaN in each input array, a foot_mu of 0 and of -1, a mass matrix with a negative pivot --
// in place and out of place, with and without the optional pointers, and checks the rules of include/cmpc_walk.h on it.
// The inputs are synthetic (a random positive definite M, random J): the step needs no more.  Usage: walk_plant_emu_main
#include "walk_plant_emu.cpp"

#include <cmath>
#include <cstdio>
#include <cstring>

enum Kind { PLAIN, HOLD, NAN_Q, NAN_V, NAN_M, NAN_H, NAN_J, NAN_POSE, NAN_TAU, NAN_EXT, NAN_IMP, MU_ZERO, MU_NEG, PIVOT };
static const int B = 16;
static const Kind kind[B] = {NAN_Q, PLAIN, HOLD, NAN_V, NAN_M, PLAIN, NAN_H, NAN_J, NAN_POSE, NAN_TAU, PLAIN, NAN_EXT, NAN_IMP,
                             MU_ZERO, MU_NEG, PIVOT};

struct Batch {
  std::vector<double> q, v, M, h, J, pose, tau, ext, mu, imp;
  std::vector<uint8_t> hold;
};

static Batch make(bool with_bad) {
  Batch a;
  a.q.resize(B * 30); a.v.resize(B * 30); a.M.resize(B * 900); a.h.resize(B * 30); a.J.resize(B * 630); a.pose.resize(B * 21);
  a.tau.resize(B * 30); a.ext.resize(B * 6); a.mu.resize(B * 2); a.imp.resize(B * 24); a.hold.assign(B, 0);
  unsigned r = 97531u;
  auto rnd = [&]() { r = r * 1664525u + 1013904223u; return ((r >> 8) & 0xFFFF) / 65536.0 - 0.5; };
  for (auto *x : {&a.q, &a.v, &a.h, &a.J, &a.pose, &a.tau, &a.ext, &a.imp})
    for (double &y : *x) y = rnd();
  for (int b = 0; b < B; ++b) {
    std::vector<double> A(900);
    for (double &y : A) y = rnd();
    for (int i = 0; i < 30; ++i)
      for (int j = 0; j < 30; ++j) {
        double s = i == j ? 2.0 : 0.0;
        for (int k = 0; k < 30; ++k) s += A[30 * i + k] * A[30 * j + k];
        a.M[900 * b + 30 * i + j] = s;
      }
    a.pose[21 * b + 5] = 0.02 * rnd();                           // the soles near the floor
    a.pose[21 * b + 11] = 0.02 * rnd();
    a.mu[2 * b] = 0.05; a.mu[2 * b + 1] = 0.5 + 0.3 * rnd();
    if (!with_bad) continue;
    switch (kind[b]) {
      case HOLD: a.hold[b] = 1; break;
      case NAN_Q: a.q[30 * b + 29] = NAN; break;
      case NAN_V: a.v[30 * b] = NAN; break;
      case NAN_M: a.M[900 * b + 899] = NAN; break;
      case NAN_H: a.h[30 * b + 7] = INFINITY; break;
      case NAN_J: a.J[630 * b + 629] = NAN; break;
      case NAN_POSE: a.pose[21 * b + 20] = NAN; break;
      case NAN_TAU: a.tau[30 * b + 23] = NAN; break;
      case NAN_EXT: a.ext[6 * b + 5] = -INFINITY; break;
      case NAN_IMP: a.imp[24 * b + 11] = NAN; break;
      case MU_ZERO: a.mu[2 * b + 1] = 0.0; break;
      case MU_NEG: a.mu[2 * b] = -1.0; break;
      case PIVOT:
        for (int k = 0; k < 30; ++k) {                           // every entry of row 7 and of column 7 once, the diagonal too
          a.M[900 * b + 30 * 7 + k] = -a.M[900 * b + 30 * 7 + k];
          if (k != 7) a.M[900 * b + 30 * k + 7] = -a.M[900 * b + 30 * k + 7];
        }
        break;
      default: break;
    }
  }
  return a;
}

struct Out {
  std::vector<double> q, v, imp, res;
  std::vector<int32_t> st;
};

static int run(const Batch &a, const cmpc_walk_plant_params &prm, Out &o) {
  o.q.assign(B * 30, 7.0); o.v.assign(B * 30, 7.0); o.imp = a.imp; o.res.assign(B, 7.0); o.st.assign(B, -1);
  return cmpc_emu_walk_plant_step(B, a.q.data(), a.v.data(), a.M.data(), a.h.data(), a.J.data(), a.pose.data(), a.tau.data(), 30,
                                  a.ext.data(), a.mu.data(), a.hold.data(), &prm, o.imp.data(), o.q.data(), o.v.data(), o.st.data(),
                                  o.res.data());
}

int main() {
  cmpc_walk_plant_params prm;
  prm.struct_size = (int32_t)sizeof(prm); prm.sweeps = 7; prm.dt = 0.01; prm.ground_z = 0.0; prm.erp = 0.2; prm.cfm = 0.0;
  const Batch clean = make(false), bad = make(true);
  Out oc, ob;
  if (run(clean, prm, oc) != 0 || run(bad, prm, ob) != 0) { fprintf(stderr, "refused: %s\n", cmpc_emu_walk_plant_last_error()); return 3; }
  double sum = 0.0;
  for (int b = 0; b < B; ++b) {
    if (oc.st[b] != 0) { fprintf(stderr, "clean row %d: status %d\n", b, oc.st[b]); return 4; }
    for (int i = 0; i < 8; ++i) {
      const double *p = &oc.imp[24 * b + 3 * i];
      if (!(p[2] >= 0.0) || !(std::hypot(p[0], p[1]) <= clean.mu[2 * b + 1] * p[2] * (1 + 1e-12))) { fprintf(stderr, "row %d: cone\n", b); return 4; }
    }
    if (kind[b] == PLAIN) {
      if (ob.st[b] != 0 || memcmp(&ob.q[30 * b], &oc.q[30 * b], 240) || memcmp(&ob.v[30 * b], &oc.v[30 * b], 240)
          || memcmp(&ob.imp[24 * b], &oc.imp[24 * b], 192) || memcmp(&ob.res[b], &oc.res[b], 8)) { fprintf(stderr, "neighbour %d moved\n", b); return 5; }
      for (int k = 0; k < 30; ++k) sum += oc.v[30 * b + k];
      continue;
    }
    const int want = kind[b] == HOLD ? 1 : 2;
    if (ob.st[b] != want || memcmp(&ob.q[30 * b], &bad.q[30 * b], 240) || memcmp(&ob.v[30 * b], &bad.v[30 * b], 240)) {
      fprintf(stderr, "row %d: status %d, or (q, v) moved\n", b, ob.st[b]);
      return 6;
    }
    for (int k = 0; k < 24; ++k) {
      const double got = ob.imp[24 * b + k], held = bad.imp[24 * b + k];
      if (want == 1 ? memcmp(&got, &held, 8) != 0 : !(got == 0.0 && !std::signbit(got))) { fprintf(stderr, "row %d: impulse\n", b); return 6; }
    }
  }
  // in place, the optional pointers NULL, packed torques: (q, v) as above
  Batch c = clean;
  std::vector<double> tau24(B * 24);
  for (int b = 0; b < B; ++b) memcpy(&tau24[24 * b], &clean.tau[30 * b], 192);
  std::vector<double> imp = clean.imp;
  if (cmpc_emu_walk_plant_step(B, c.q.data(), c.v.data(), c.M.data(), c.h.data(), c.J.data(), c.pose.data(), tau24.data(), 24,
                               c.ext.data(), c.mu.data(), nullptr, &prm, imp.data(), c.q.data(), c.v.data(), nullptr, nullptr) != 0) return 7;
  if (memcmp(c.q.data(), oc.q.data(), B * 240) || memcmp(c.v.data(), oc.v.data(), B * 240) || memcmp(imp.data(), oc.imp.data(), B * 192)) {
    fprintf(stderr, "in place differs\n");
    return 7;
  }
  Out on;
  on.q.assign(B * 30, 7.0); on.v.assign(B * 30, 7.0);
  if (cmpc_emu_walk_plant_step(B, clean.q.data(), clean.v.data(), clean.M.data(), clean.h.data(), clean.J.data(), clean.pose.data(),
                               nullptr, 24, nullptr, clean.mu.data(), nullptr, &prm, nullptr, on.q.data(), on.v.data(), nullptr, nullptr) != 0) return 8;
  for (double x : on.v)
    if (!std::isfinite(x)) return 8;
  // refusals, and the empty batch
  cmpc_walk_plant_params p2 = prm;
  p2.sweeps = -1;
  if (run(clean, p2, on) == 0) return 9;
  p2 = prm; p2.dt = 0.0;
  if (run(clean, p2, on) == 0) return 9;
  p2 = prm; p2.struct_size = 8;
  if (run(clean, p2, on) == 0) return 9;
  if (cmpc_emu_walk_plant_step(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 24, nullptr, nullptr, nullptr, &prm,
                               nullptr, nullptr, nullptr, nullptr, nullptr) != 0) return 9;
  printf("ok B=%d checksum %.17g\n", B, sum);
  return 0;
}

// rbd_walk_emu_main.cpp -- TEST HARNESS ONLY.  A stand-alone program around rbd_walk_emu.cpp for sanitizer builds
// (-fsanitize=address,undefined): runs the device source of both walking-loop kernels on a small two-scene gait authored
// here -- every branch of the foot generator, NaN rows, rows outside their scene, hold rows, NULL outputs, in place -- and
// checks that bad rows are NaN, held rows unchanged and everything else finite.  Usage: rbd_walk_emu_main
#include "rbd_walk_emu.cpp"

#include <cmath>
#include <cstdio>
#include <cstring>

int main() {
  // two scenes, padded: scene 0 has 4 steps over 50 ticks, scene 1 has 3 steps over 30 ticks and swings the other foot
  const int S = 2, T_max = 50, n_max = 4;
  const int32_t T[S] = {50, 30}, n_steps[S] = {4, 3};
  const int32_t step_start[S * n_max] = {0, 20, 30, 40, 0, 10, 20, -1};
  const int32_t ss_dur[S * n_max] = {0, 7, 7, 7, 0, 6, 6, -1};
  const uint8_t support_l[S * n_max] = {1, 0, 1, 0, 0, 1, 0, 0};
  std::vector<int32_t> step_idx(S * T_max, -1);
  for (int t = 0; t < 50; ++t) step_idx[t] = t < 20 ? 0 : t < 30 ? 1 : t < 40 ? 2 : 3;
  for (int t = 0; t < 30; ++t) step_idx[T_max + t] = t / 10;
  std::vector<double> ang(S * n_max * 3, NAN), init_feet(S * 12, 0.0);
  for (int s = 0; s < S; ++s)
    for (int i = 0; i < n_steps[s]; ++i) { ang[3 * (s * n_max + i)] = 0.0; ang[3 * (s * n_max + i) + 1] = 0.0; ang[3 * (s * n_max + i) + 2] = 0.1 * i; }
  for (int s = 0; s < S; ++s) { init_feet[12 * s + 4] = 0.1; init_feet[12 * s + 10] = -0.1; }

  // rows: every branch, then the bad ones
  struct Row { int t, s; };
  const Row rows[] = {{0, 0}, {5, 0}, {20, 0}, {23, 0}, {26, 0}, {27, 0}, {35, 0}, {12, 1}, {17, 1},
                      {-1, 0}, {50, 0}, {30, 1}, {3, -1}, {3, 2}, {45, 0}, {25, 1}, {22, 0}, {22, 0}};
  const int B = (int)(sizeof(rows) / sizeof(rows[0])), first_bad = 9, nan_pose = B - 2, nan_plan = B - 1;
  std::vector<int32_t> t(B), sid(B);
  std::vector<double> plan(B * n_max * 3), pose(B * 21), vel(B * 21), jd(B * 21), com(B * 9), q(B * 30), v(B * 30), qref(30, 0.1);
  unsigned r = 12345u;
  auto rnd = [&]() { r = r * 1664525u + 1013904223u; return ((r >> 8) & 0xFFFF) / 65536.0 - 0.5; };
  for (int b = 0; b < B; ++b) { t[b] = rows[b].t; sid[b] = rows[b].s; }
  for (auto *a : {&plan, &pose, &vel, &jd, &com, &q, &v})
    for (double &x : *a) x = rnd();
  pose[21 * nan_pose + 7] = NAN;
  plan[(nan_plan * n_max + 2) * 3 + 1] = INFINITY;              // plan[idx + 1] of a single-support row
  std::vector<double> ff(B * 51), pe(B * 51), ve(B * 51), fd(B * 36);
  for (int pass = 0; pass < 2; ++pass)                          // (the second pass with every output skipped: the NULL branches)
    if (cmpc_emu_walk_task_refs(S, T_max, n_max, T, step_idx.data(), n_steps, step_start, ss_dur, support_l, ang.data(),
                                init_feet.data(), 0.02, 0.01, B, t.data(), pass ? nullptr : sid.data(), plan.data(), pose.data(),
                                vel.data(), jd.data(), com.data(), q.data(), v.data(), pass ? nullptr : qref.data(),
                                pass ? nullptr : ff.data(), pass ? nullptr : pe.data(), pass ? nullptr : ve.data(),
                                pass ? nullptr : fd.data()) != 0) {
      fprintf(stderr, "refused: %s\n", cmpc_emu_walk_last_error());
      return 3;
    }
  double sum = 0.0;
  for (int b = 0; b < B; ++b) {
    const bool bad = b >= first_bad;
    for (int k = 0; k < 51 + 51 + 51 + 36; ++k) {
      const double x = k < 51 ? ff[51 * b + k] : k < 102 ? pe[51 * b + k - 51] : k < 153 ? ve[51 * b + k - 102] : fd[36 * b + k - 153];
      if (bad ? !std::isnan(x) : !std::isfinite(x)) { fprintf(stderr, "row %d word %d: %g\n", b, k, x); return 4; }
      if (!bad) sum += x;
    }
  }

  // the integrator: plain rows, a held row, a NaN acceleration, then the same in place
  const int Bi = 6;
  std::vector<double> qi(Bi * 30), vi(Bi * 30), ai(Bi * 30), qo(Bi * 30), vo(Bi * 30);
  for (auto *a : {&qi, &vi, &ai})
    for (double &x : *a) x = rnd();
  for (int k = 0; k < 3; ++k) qi[30 + k] = 0.0;                  // a base at the identity
  ai[30 * 4 + 17] = NAN;
  const uint8_t hold[Bi] = {0, 0, 0, 1, 0, 0};
  if (cmpc_emu_walk_integrate(Bi, qi.data(), vi.data(), ai.data(), 0.01, hold, qo.data(), vo.data()) != 0) return 3;
  for (int b = 0; b < Bi; ++b) {
    const bool held = b == 3 || b == 4;
    if (held && (memcmp(&qo[30 * b], &qi[30 * b], 240) != 0 || memcmp(&vo[30 * b], &vi[30 * b], 240) != 0)) {
      fprintf(stderr, "held row %d changed\n", b);
      return 5;
    }
    for (int k = 0; k < 30; ++k) {
      if (!std::isfinite(qo[30 * b + k]) || !std::isfinite(vo[30 * b + k])) { fprintf(stderr, "integrator row %d not finite\n", b); return 5; }
      sum += qo[30 * b + k] + vo[30 * b + k];
    }
  }
  std::vector<double> q2 = qi, v2 = vi;
  if (cmpc_emu_walk_integrate(Bi, q2.data(), v2.data(), ai.data(), 0.01, nullptr, q2.data(), v2.data()) != 0) return 3;
  for (int b = 0; b < Bi; ++b)
    if (b != 3 && (memcmp(&q2[30 * b], &qo[30 * b], 240) != 0 || memcmp(&v2[30 * b], &vo[30 * b], 240) != 0)) {
      fprintf(stderr, "in place differs in row %d\n", b);
      return 6;
    }
  printf("ok B=%d+%d checksum %.17g\n", B, Bi, sum);
  return 0;
}

// walk_measure_emu_main.cpp -- TEST HARNESS ONLY.  A stand-alone program around walk_measure_emu.cpp for sanitizer builds
// (-fsanitize=address,undefined): runs the device source of cmpc_walk_measure on a small batch authored here -- plain rows, a
// dead row, NaN and Inf rows, a row below z_min, a tilted base, at both ends of the batch -- with and without alive and the
// outputs, and checks every rule of include/cmpc_walk.h on it.  Usage: walk_measure_emu_main
#include "walk_measure_emu.cpp"

#include <cmath>
#include <cstdio>
#include <cstring>

int main() {
  const int B = 12;
  enum Kind { PLAIN, DEAD, NAN_CEN, INF_POSE, LOW, TILTED };
  const Kind kind[B] = {DEAD, PLAIN, NAN_CEN, PLAIN, PLAIN, INF_POSE, LOW, PLAIN, TILTED, PLAIN, PLAIN, NAN_CEN};
  std::vector<double> cen(B * 9), pose(B * 21), state(B * 16);
  std::vector<uint8_t> alive(B, 1);
  unsigned r = 4321u;
  auto rnd = [&]() { r = r * 1664525u + 1013904223u; return ((r >> 8) & 0xFFFF) / 65536.0 - 0.5; };
  for (auto *a : {&cen, &pose, &state})
    for (double &x : *a) x = rnd();
  for (int b = 0; b < B; ++b) {
    cen[9 * b + 2] = 0.8 + 0.1 * rnd();
    for (int k = 18; k < 21; ++k) pose[21 * b + k] *= 0.2;       // bases within 0.2 rad of upright
    if (kind[b] == DEAD) alive[b] = 0;
    if (kind[b] == NAN_CEN) cen[9 * b + 8] = NAN;
    if (kind[b] == INF_POSE) pose[21 * b + 13] = -INFINITY;
    if (kind[b] == LOW) cen[9 * b + 2] = 0.3;
    if (kind[b] == TILTED) { pose[21 * b + 18] = 1.0; pose[21 * b + 19] = 0.0; pose[21 * b + 20] = 0.5; }
  }
  const double z_min = 0.5, cos_tilt_min = std::cos(0.6);
  const std::vector<double> state0 = state;
  std::vector<double> xm(B * 20, 12345.0), inn(B * 9, 12345.0);
  if (cmpc_emu_walk_measure(B, cen.data(), pose.data(), z_min, cos_tilt_min, state.data(), alive.data(), xm.data(), inn.data()) != 0) {
    fprintf(stderr, "refused: %s\n", cmpc_emu_walk_measure_last_error());
    return 3;
  }
  double sum = 0.0;
  for (int b = 0; b < B; ++b) {
    const double *s0 = &state0[16 * b], *s = &state[16 * b], *c = &cen[9 * b], *p = &pose[21 * b];
    if (kind[b] != PLAIN) {
      if (memcmp(s, s0, 128) != 0 || alive[b] != 0) { fprintf(stderr, "row %d: state or alive\n", b); return 4; }
      for (int k = 0; k < 29; ++k)
        if (!std::isnan(k < 20 ? xm[20 * b + k] : inn[9 * b + k - 20])) { fprintf(stderr, "row %d word %d is not NaN\n", b, k); return 4; }
      continue;
    }
    const double want[20] = {c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], s0[9], s0[10], s0[11],
                             p[2], p[3], p[4], 0.0, p[8], p[9], p[10], 0.0};
    if (alive[b] != 1 || memcmp(&xm[20 * b], want, 160) != 0 || memcmp(s, c, 72) != 0 || memcmp(s + 9, s0 + 9, 24) != 0
        || s[12] != p[2] || s[13] != p[8] || memcmp(s + 14, s0 + 14, 16) != 0) {
      fprintf(stderr, "row %d: x_meas or state\n", b);
      return 5;
    }
    for (int k = 0; k < 9; ++k) {
      if (inn[9 * b + k] != c[k] - s0[k]) { fprintf(stderr, "row %d: innovation %d\n", b, k); return 5; }
      sum += inn[9 * b + k];
    }
  }
  // no alive, no outputs, both guards off: the rows that were dead, low or tilted are measured, the non-finite ones are not
  std::vector<double> s2 = state0;
  if (cmpc_emu_walk_measure(B, cen.data(), pose.data(), -INFINITY, -INFINITY, s2.data(), nullptr, nullptr, nullptr) != 0) return 3;
  for (int b = 0; b < B; ++b) {
    const bool kept = kind[b] == NAN_CEN || kind[b] == INF_POSE;
    if (memcmp(&s2[16 * b], kept ? &state0[16 * b] : &cen[9 * b], kept ? 128 : 72) != 0) { fprintf(stderr, "second pass, row %d\n", b); return 6; }
  }
  // refusals, and the empty batch
  if (cmpc_emu_walk_measure(-1, cen.data(), pose.data(), 0.0, 0.0, s2.data(), nullptr, nullptr, nullptr) == 0) return 7;
  if (cmpc_emu_walk_measure(B, cen.data(), pose.data(), NAN, 0.0, s2.data(), nullptr, nullptr, nullptr) == 0) return 7;
  if (cmpc_emu_walk_measure(B, cen.data(), pose.data(), 0.0, 0.0, nullptr, nullptr, nullptr, nullptr) == 0) return 7;
  if (cmpc_emu_walk_measure(0, nullptr, nullptr, 0.0, 0.0, nullptr, nullptr, nullptr, nullptr) != 0) return 7;
  printf("ok B=%d checksum %.17g\n", B, sum);
  return 0;
}

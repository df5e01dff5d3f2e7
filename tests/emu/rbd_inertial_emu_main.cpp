// rbd_inertial_emu_main.cpp -- TEST HARNESS ONLY.  A stand-alone program around rbd_inertial_emu.cpp for sanitizer builds
// (-fsanitize=address,undefined): reads a model's tables, a batch and every robot's own inertial row from a text file of
// numbers, runs the per-instance path of the rigid-body model's device source on it and checks that M is symmetric and
// everything finite; then once more with a NaN planted in the last robot's row, whose outputs must all be NaN (the exit of
// a bad row) and the other robots' unchanged.  Usage: rbd_inertial_emu_main FILE
//   parent[25] joint_R[225] joint_p[75] axis[75] mass[25] com[75] inertia[150] frame_body[4] frame_R[36] frame_p[12] B g
//   q[B][30] v[B][30] inertial[B][25][10]
#include "rbd_inertial_emu.cpp"

#include <cmath>
#include <cstdio>

static bool read_d(FILE *f, std::vector<double> &a, size_t n) {
  a.resize(n);
  for (size_t i = 0; i < n; ++i)
    if (fscanf(f, "%lf", &a[i]) != 1) return false;
  return true;
}
static bool read_i(FILE *f, std::vector<int32_t> &a, size_t n) {
  a.resize(n);
  for (size_t i = 0; i < n; ++i) {
    int v;
    if (fscanf(f, "%d", &v) != 1) return false;
    a[i] = v;
  }
  return true;
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<int32_t> parent, frame_body, nb;
  std::vector<double> jR, jp, axis, mass, com, inertia, fR, fp, g, q, v, rows;
  bool ok = read_i(f, parent, 25) && read_d(f, jR, 225) && read_d(f, jp, 75) && read_d(f, axis, 75) && read_d(f, mass, 25) &&
            read_d(f, com, 75) && read_d(f, inertia, 150) && read_i(f, frame_body, 4) && read_d(f, fR, 36) && read_d(f, fp, 12) &&
            read_i(f, nb, 1) && read_d(f, g, 1);
  ok = ok && nb[0] >= 1 && nb[0] <= 64 && read_d(f, q, 30 * (size_t)nb[0]) && read_d(f, v, 30 * (size_t)nb[0]) &&
       read_d(f, rows, 250 * (size_t)nb[0]);
  fclose(f);
  if (!ok) { fprintf(stderr, "short or malformed input\n"); return 2; }
  const int B = nb[0];
  std::vector<double> J(630 * B), jd(21 * B), M(900 * B), h(30 * B), pose(21 * B), vel(21 * B), cen(9 * B);
  auto run = [&](const std::vector<double> &tab, bool outputs) {
    return cmpc_emu_rbd_eval_inertial(parent.data(), jR.data(), jp.data(), axis.data(), mass.data(), com.data(), inertia.data(),
                                      frame_body.data(), fR.data(), fp.data(), B, q.data(), v.data(), tab.data(), g[0],
                                      outputs ? J.data() : nullptr, outputs ? jd.data() : nullptr, outputs ? M.data() : nullptr,
                                      outputs ? h.data() : nullptr, outputs ? pose.data() : nullptr, outputs ? vel.data() : nullptr,
                                      outputs ? cen.data() : nullptr);
  };
  if (run(rows, true) != 0) { fprintf(stderr, "refused: %s\n", cmpc_emu_rbd_inertial_last_error()); return 3; }
  if (run(rows, false) != 0) return 3;               // (every output skipped: the NULL branches)
  double sum = 0.0;
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < 30; ++i)
      for (int j = 0; j < 30; ++j)
        if (M[900 * b + 30 * i + j] != M[900 * b + 30 * j + i]) { fprintf(stderr, "M not symmetric\n"); return 4; }
  for (const auto *a : {&J, &jd, &M, &h, &pose, &vel, &cen})
    for (double x : *a) {
      if (!std::isfinite(x)) { fprintf(stderr, "non-finite output\n"); return 5; }
      sum += x;
    }
  // a bad row: the last robot's last word
  const std::vector<double> M0 = M, cen0 = cen;
  std::vector<double> bad = rows;
  bad[250 * (size_t)B - 1] = std::nan("");
  if (run(bad, true) != 0) return 3;
  for (int b = 0; b < B; ++b) {
    const bool last = b == B - 1;
    for (int i = 0; i < 900; ++i)
      if (last ? !std::isnan(M[900 * b + i]) : M[900 * b + i] != M0[900 * b + i]) { fprintf(stderr, "bad row: M of robot %d\n", b); return 6; }
    for (int i = 0; i < 9; ++i)
      if (last ? !std::isnan(cen[9 * b + i]) : cen[9 * b + i] != cen0[9 * b + i]) { fprintf(stderr, "bad row: centroid of robot %d\n", b); return 6; }
  }
  if (run(bad, false) != 0) return 3;
  printf("ok B=%d checksum %.17g\n", B, sum);
  return 0;
}

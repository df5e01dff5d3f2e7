// rbd_emu_main.cpp -- TEST HARNESS ONLY.  A stand-alone program around rbd_emu.cpp for sanitizer builds
// (-fsanitize=address,undefined): reads a model's tables and a batch from a text file of numbers, runs the device source of
// the rigid-body model on it and checks that M is symmetric and everything finite.  Usage: rbd_emu_main FILE
//   parent[25] joint_R[225] joint_p[75] axis[75] mass[25] com[75] inertia[150] frame_body[4] frame_R[36] frame_p[12] B g
//   q[B][30] v[B][30]
#include "rbd_emu.cpp"

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
  std::vector<double> jR, jp, axis, mass, com, inertia, fR, fp, g, q, v;
  bool ok = read_i(f, parent, 25) && read_d(f, jR, 225) && read_d(f, jp, 75) && read_d(f, axis, 75) && read_d(f, mass, 25) &&
            read_d(f, com, 75) && read_d(f, inertia, 150) && read_i(f, frame_body, 4) && read_d(f, fR, 36) && read_d(f, fp, 12) &&
            read_i(f, nb, 1) && read_d(f, g, 1);
  ok = ok && nb[0] >= 0 && nb[0] <= 64 && read_d(f, q, 30 * (size_t)nb[0]) && read_d(f, v, 30 * (size_t)nb[0]);
  fclose(f);
  if (!ok) { fprintf(stderr, "short or malformed input\n"); return 2; }
  const int B = nb[0];
  std::vector<double> J(630 * B), jd(21 * B), M(900 * B), h(30 * B), pose(21 * B), vel(21 * B), cen(9 * B);
  if (cmpc_emu_rbd_eval(parent.data(), jR.data(), jp.data(), axis.data(), mass.data(), com.data(), inertia.data(),
                        frame_body.data(), fR.data(), fp.data(), B, q.data(), v.data(), g[0], J.data(), jd.data(), M.data(),
                        h.data(), pose.data(), vel.data(), cen.data()) != 0) {
    fprintf(stderr, "refused: %s\n", cmpc_emu_rbd_last_error());
    return 3;
  }
  // (a second pass with every output skipped: the NULL branches)
  if (cmpc_emu_rbd_eval(parent.data(), jR.data(), jp.data(), axis.data(), mass.data(), com.data(), inertia.data(),
                        frame_body.data(), fR.data(), fp.data(), B, q.data(), v.data(), g[0], nullptr, nullptr, nullptr, nullptr,
                        nullptr, nullptr, nullptr) != 0)
    return 3;
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
  printf("ok B=%d checksum %.17g\n", B, sum);
  return 0;
}

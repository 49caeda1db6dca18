// disc_noise_harness.cpp -- test-only shim: the PRODUCT's host-side functions for uncertain discs (csrc/pocs_collide.h:
// pocs_disc_noise_factor, pocs_disc_noise_grow on the record pocs_prepare_disc forms, pocs_disc_displaced and
// pocs_pose_collides_noisy) through a C ABI, so that tests/test_disc_noise.py can check them against the specification restated in
// Python on the CPU.  Built by that file with the flags tests/conftest.py uses for host_harness.cpp; never part of libpocs.so.
// With DISC_NOISE_HARNESS_MAIN it is a stand-alone program (its own main) for a sanitizer build: it reads one binary file of cases
// and writes one answer per case to standard output.
#include "../probability-of-collision-for-safe-planning_amd/csrc/pocs_collide.h"

#include <cstdio>
#include <cstring>
#include <vector>

static const pocs_tables* tabs() {
  static pocs_tables T;
  static bool ready = false;
  if (!ready) { pocs_tables_init(&T); ready = true; }
  return &T;
}

// records and rows of D discs as upload_world composes them under covariances (no boxes in front); -1 for a bad covariance
static int compose(const pocs_footprint* fp, const double* discs, const double* cov, int D, double* rec, double* rows) {
  for (int d = 0; d < D; ++d) {
    pocs_prepare_disc(discs + 3 * d, fp, rec + d * POCS_OBS_STRIDE);
    if (pocs_disc_noise_factor(cov + 3 * d, rows + d * POCS_NOISE_STRIDE) < 0) return -1;
    rows[d * POCS_NOISE_STRIDE + 3] = (double)d;
    pocs_disc_noise_grow(rows + d * POCS_NOISE_STRIDE, rec + d * POCS_OBS_STRIDE);
  }
  return 0;
}

extern "C" {
// the factorisation: 0 = a row was written, 1 = zeros (a certain disc), -1 = not a covariance
int nh_factor(const double* cov3, double* row3) { return pocs_disc_noise_factor(cov3, row3); }
// the record of one disc, grown for its covariance (8 doubles)
int nh_record(const double* fp4, const double* disc3, const double* cov3, double* rec8) {
  const pocs_footprint fp = {fp4[0], fp4[1], fp4[2], fp4[3]};
  double row[POCS_NOISE_STRIDE];
  return compose(&fp, disc3, cov3, 1, rec8, row);
}
// the displaced centre of a disc at (cx, cy) with index d for pose index `index`
int nh_displaced(const double* centre2, const double* cov3, unsigned long long seed, unsigned long long index, unsigned v, int d, double* out2) {
  double row[POCS_NOISE_STRIDE];
  const int k = pocs_disc_noise_factor(cov3, row);
  if (k < 0) return -1;
  row[3] = (double)d;
  out2[0] = centre2[0]; out2[1] = centre2[1];
  if (k == 0) pocs_disc_displaced(centre2[0], centre2[1], row, seed, index, v, tabs(), &out2[0], &out2[1]);
  return 0;
}
// One table of D <= 16 discs, n poses of indices idx[i]: out[i] bit d = pose i touches displaced disc d; bit 31 should the function's
// own answer ever differ from (bits != 0)
int nh_flags(const double* fp4, const double* discs, const double* cov, int D, unsigned long long seed, unsigned v, int n,
             const double* poses_xyt, const unsigned long long* idx, unsigned* out) {
  if (D < 0 || D > 16) return -1;
  const pocs_footprint fp = {fp4[0], fp4[1], fp4[2], fp4[3]};
  double rec[16 * POCS_OBS_STRIDE], rows[16 * POCS_NOISE_STRIDE];
  if (compose(&fp, discs, cov, D, rec, rows) != 0) return -1;
  for (int i = 0; i < n; ++i) {
    const double* p = poses_xyt + 3 * i;
    unsigned bits = 0u;
    const bool any = pocs_pose_collides_noisy(p[0], p[1], p[2], &fp, rec, rows, D, seed, idx[i], v, tabs(), &bits);
    out[i] = bits | (any != (bits != 0u) ? 0x80000000u : 0u);
  }
  return 0;
}
// the largest |z| of pocs_normal_pair_w2 over nr radius words x na angle words
double nh_max_abs_z(const unsigned* wr, int nr, const unsigned* wa, int na) {
  double worst = 0.0;
  for (int i = 0; i < nr; ++i)
    for (int j = 0; j < na; ++j) {
      double z0, z1;
      pocs_normal_pair_w2(wr[i], wa[j], tabs(), &z0, &z1);
      worst = fmax(worst, fmax(fabs(z0), fabs(z1)));
    }
  return worst;
}
// n cases of their own: case i is one pose, one disc of index dnum[i], its covariance, a pose index, a seed and a waypoint word.
// out[i]: 1 = touches, 0 = does not; -1 returned for a bad covariance
int nh_cases(const double* fp4, int n, const double* poses_xyt, const double* discs, const double* cov, const unsigned long long* seeds,
             const unsigned long long* idx, const unsigned* v, const int* dnum, int* out) {
  const pocs_footprint fp = {fp4[0], fp4[1], fp4[2], fp4[3]};
  for (int i = 0; i < n; ++i) {
    double rec[POCS_OBS_STRIDE], row[POCS_NOISE_STRIDE];
    if (compose(&fp, discs + 3 * i, cov + 3 * i, 1, rec, row) != 0) return -1;
    row[3] = (double)dnum[i];
    const double* p = poses_xyt + 3 * i;
    out[i] = pocs_pose_collides_noisy(p[0], p[1], p[2], &fp, rec, row, 1, seeds[i], idx[i], v[i], tabs()) ? 1 : 0;
  }
  return 0;
}
}

#ifdef DISC_NOISE_HARNESS_MAIN
// file: int32 n, pad; double fp[4]; poses[3 n]; discs[3 n]; cov[3 n]; u64 seeds[n]; u64 idx[n]; u32 v[n]; i32 dnum[n].  stdout: n lines.
int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int head[2];
  double fp4[4];
  if (fread(head, sizeof(int), 2, f) != 2 || fread(fp4, sizeof(double), 4, f) != 4) { fclose(f); return 2; }
  const int n = head[0];
  if (n < 0 || n > (1 << 20)) { fclose(f); return 2; }
  const size_t N = (size_t)n;
  std::vector<double> poses(3 * N + 1), discs(3 * N + 1), cov(3 * N + 1);
  std::vector<unsigned long long> seeds(N + 1), idx(N + 1);
  std::vector<unsigned> v(N + 1);
  std::vector<int> dnum(N + 1), out(N + 1, -1);
  const bool ok = fread(poses.data(), sizeof(double), 3 * N, f) == 3 * N && fread(discs.data(), sizeof(double), 3 * N, f) == 3 * N &&
                  fread(cov.data(), sizeof(double), 3 * N, f) == 3 * N && fread(seeds.data(), 8, N, f) == N && fread(idx.data(), 8, N, f) == N &&
                  fread(v.data(), 4, N, f) == N && fread(dnum.data(), 4, N, f) == N;
  fclose(f);
  if (!ok) return 2;
  if (nh_cases(fp4, n, poses.data(), discs.data(), cov.data(), seeds.data(), idx.data(), v.data(), dnum.data(), out.data()) != 0) return 2;
  for (int i = 0; i < n; ++i) printf("%d\n", out[i]);
  return 0;
}
#endif

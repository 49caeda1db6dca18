// pocs_world.h -- the cull decisions of a large collision world (pocs_set_world with more than POCS_MAX_OBSTACLES boxes; product
// code, host + device, no HIP type).
//
// A large world is a table of up to POCS_MAX_WORLD_BOXES records (pocs_prepare_obstacle) in device memory.  Nothing spatial
// is built over it: the records that can matter are found by brute force, and every decision below only ever drops a record
// that the broad phase of pocs_box_hit rejects for every pose in question -- so the flags are those of the full loop over M.
//
//   GMM  per (run, waypoint) one block of k_world_cull tests all M records against the box of every pose the run's mixture
//        can draw (pocs_world_reach_box, pocs_world_extents, pocs_world_keep: the arithmetic of k_gmm_step's own cull, which
//        calls the same functions) and hands the sampling launch the kept records, at most POCS_MAX_OBSTACLES of them;
//   MC   per wave and particle iteration the 64 lanes' footprint centres are reduced to their bounding box, and a record the
//        box cannot reach (pocs_world_wave_rejects) is skipped by the whole wave.
//
// tests/large_world_harness.cpp compiles these for the host; tests/test_large_world_host.py checks them against the oracle.
#pragma once
#include "pocs_collide.h"
#include "pocs_model.h"

// Every pose (base x, y and heading) a mixture of K components can draw, from its sampler parameters par[K][POCS_PARAM_STRIDE]
// (mean[3], then L00 L10 L11 L20 L21 L22 of the lower Cholesky factor).  A Box-Muller normal is bounded: u >= 2^-32 gives
// |z| <= sqrt(64 ln 2) < 6.661 (pocs_normal_pair_w2; 6.67 leaves 0.1 % for the rounding of radius * cos), so every pose lies
// within mean_k +- 6.67 (|L00|, |L10|+|L11|, |L20|+|L21|+|L22|) of some component.  The position box is then grown by the
// distance between the base and the footprint's centre, the heading range by a relative 1e-9.
struct pocs_reach { double xlo, xhi, ylo, yhi, tlo, thi; };
POCS_HD void pocs_world_reach_box(const double* par, const int K, const pocs_footprint& fp, pocs_reach& r) {
  double xlo = 1e300, xhi = -1e300, ylo = 1e300, yhi = -1e300, tlo = 1e300, thi = -1e300;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < K; ++k) {
    const double* p = &par[k * POCS_PARAM_STRIDE];
    const double ex = 6.67 * fabs(p[3]), ey = 6.67 * (fabs(p[4]) + fabs(p[5])), et = 6.67 * (fabs(p[6]) + fabs(p[7]) + fabs(p[8]));
    xlo = fmin(xlo, p[0] - ex); xhi = fmax(xhi, p[0] + ex);
    ylo = fmin(ylo, p[1] - ey); yhi = fmax(yhi, p[1] + ey);
    tlo = fmin(tlo, p[2] - et); thi = fmax(thi, p[2] + et);
  }
  const double pad = sqrt(fp.dx * fp.dx + fp.dy * fp.dy) + 1e-6;   // footprint centre vs base
  xlo -= pad; xhi += pad; ylo -= pad; yhi += pad;
  tlo -= 1e-9 * (1.0 + fabs(tlo)); thi += 1e-9 * (1.0 + fabs(thi));
  r.xlo = xlo; r.xhi = xhi; r.ylo = ylo; r.yhi = yhi; r.tlo = tlo; r.thi = thi;
}

// The footprint's largest half-extent along world x and along world y over the headings [tlo, thi] (pocs_footprint_extent_pre:
// rr the bounding radius, phi = atan2(hy, hx)).  The kernels evaluate the four end values side by side in four lanes; these are
// the same functions of the same arguments.
POCS_HD void pocs_world_extents(const pocs_footprint& fp, const double rr, const double phi, const pocs_reach& r, double& ext_x, double& ext_y) {
  const double HALF_PI = 1.57079632679489661923;
  ext_x = pocs_footprint_extent_pre(fp.hx, fp.hy, rr, phi, r.tlo, r.thi);
  ext_y = pocs_footprint_extent_pre(fp.hx, fp.hy, rr, phi, r.tlo - HALF_PI, r.thi - HALF_PI);
}

// Does record o (POCS_OBS_STRIDE doubles) stay in the run's table?  bx, by: the record's broad phase tightened to the run's
// headings -- the obstacle's own world box (as pocs_prepare_obstacle) + the footprint's extents for this run, never more than
// the table's o[6], o[7].  A record whose tightened box misses the pose box is rejected by the broad phase for every sample.
POCS_HD bool pocs_world_keep(const double* o, const pocs_reach& r, const double ext_x, const double ext_y, double& bx, double& by) {
  bx = fmin(o[6], fma(o[4], fabs(o[2]), o[5] * fabs(o[3])) * (1.0 + 1e-12) + ext_x);
  by = fmin(o[7], fma(o[4], fabs(o[3]), o[5] * fabs(o[2])) * (1.0 + 1e-12) + ext_y);
  return !(o[0] - bx > r.xhi || o[0] + bx < r.xlo || o[1] - by > r.yhi || o[1] + by < r.ylo);
}

// MC: may a wave whose footprint centres all lie in [xlo, xhi] x [ylo, yhi] skip the record with centre (cx, cy) and broad
// phase (bx, by) = (o[6], o[7])?  Rounding is monotone: px <= xhi gives fl(cx - px) >= fl(cx - xhi), so cx - xhi > bx means
// |cx - px| > bx for every lane -- the broad phase of pocs_box_hit rejects the record for each of them; likewise on the other
// three sides.
POCS_HD bool pocs_world_wave_rejects(const double cx, const double cy, const double bx, const double by,
                                     const double xlo, const double xhi, const double ylo, const double yhi) {
  return cx - xhi > bx || xlo - cx > bx || cy - yhi > by || ylo - cy > by;
}

// A pose's footprint centre and heading sine / cosine, exactly as pocs_pose_collides forms them.
POCS_HD void pocs_world_pose(double x, double y, double th, const pocs_footprint* fp, const pocs_tables* T,
                             double* px, double* py, double* sn, double* cs) {
  pocs_sincos_tab(th, T, sn, cs, nullptr);
  *px = x; *py = y;
  if (!(fp->dx == 0.0 && fp->dy == 0.0)) {
    *px = x + fma(*cs, fp->dx, -(*sn * fp->dy));
    *py = y + fma(*sn, fp->dx, *cs * fp->dy);
  }
}

// pocs_collide.h -- the collision predicate (product code, host + device).
//
// Stands in for MCSimulator::checkCollision (MCSimulator.h:257-285), i.e. for
// robot->SetActiveDOFValues + env->CheckCollision(robot) (:275,:279).  OpenRAVE, its ODE checker
// and the PR2 model are not part of the reference tree, so this is the build's own explicit 2-D
// model: one oriented footprint box carried by the base pose (x, y, theta) against M static
// oriented boxes, separating-axis test on the four face normals.  Touching counts as collision.
//
// Obstacle record (POCS_OBS_STRIDE doubles), prepared once on the host by pocs_prepare_obstacle:
//   cx cy   centre            ax ay   unit x-axis of the box (cos yaw, sin yaw)
//   hx hy   half extents      bx by   half extents of its world AABB grown by the footprint's
//                                     bounding radius (broad phase; purely conservative)
#pragma once
#include "pocs_math.h"
#include "pocs_model.h"      // pocs_wrap_angle: the segment checks' sub-poses are outputs of pocs_motion

#define POCS_OBS_STRIDE 8
#define POCS_MAX_OBSTACLES 64

struct pocs_footprint { double dx, dy, hx, hy; };   // offset in the base frame, half extents

POCS_HD void pocs_prepare_obstacle(const double box5[5], const pocs_footprint* fp, double* rec) {
  double sn, cs;
  pocs_sincos(box5[4], &sn, &cs);
  const double rr = sqrt(fp->hx * fp->hx + fp->hy * fp->hy);
  rec[0] = box5[0]; rec[1] = box5[1];
  rec[2] = cs; rec[3] = sn;
  rec[4] = box5[2]; rec[5] = box5[3];
  rec[6] = (box5[2] * fabs(cs) + box5[3] * fabs(sn)) + rr;
  rec[7] = (box5[2] * fabs(sn) + box5[3] * fabs(cs)) + rr;
}

// Narrow phase: footprint at (px, py) with heading (sn, cs) against one obstacle record that has
// passed the broad phase.  Separating axes = the four face normals; a > b <=> a - b > 0 exactly
// in IEEE arithmetic (gradual underflow), so each pair of tests folds into one compare of the larger
// margin.  An axis-aligned obstacle (axis exactly (1, 0)) takes a shorter path that produces the
// same values: fma(c, 1, s*0) == c, fma(dx, 1, dy*0) == dx.
// The margins of the four axes given the relative yaw (cr, sr: cosine and sine, signed) and the offset in the
// obstacle's frame (e1, e2).  Inlined into BOTH paths of pocs_box_narrow below instead of after their merge: merged,
// the compiler materialises |cos|, |sin| and copies of the offsets into fresh registers for the common tail (six
// vector moves per pose and record in the axis-aligned case); in place, the absolute values are operand modifiers.
POCS_HD bool pocs_box_margins(double dx, double dy, double sn, double cs, double rx, double ry, double hx, double hy,
                              double cr, double sr, double e1, double e2) {
  // The obstacle's own two axes first: they separate nearly every pose that is in reach but does not
  // touch (a wall and a robot driving past it), and a wave whose poses are all separated there skips
  // the footprint's axes.  (max of the four margins > 0  <=>  one of the two maxima > 0.)
  const double m3 = fabs(e1) - (hx + fma(rx, fabs(cr), ry * fabs(sr)));
  const double m4 = fabs(e2) - (hy + fma(rx, fabs(sr), ry * fabs(cr)));
  if (fmax(m3, m4) > 0.0) return false;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("; footprint axes");                                // keeps the early return a branch
#endif
  const double d1 = fma(dx, cs, dy * sn);                         // d in the footprint frame
  const double d2 = fma(dy, cs, -(dx * sn));
  const double m1 = fabs(d1) - (rx + fma(hx, fabs(cr), hy * fabs(sr)));
  const double m2 = fabs(d2) - (ry + fma(hx, fabs(sr), hy * fabs(cr)));
  return !(fmax(m1, m2) > 0.0);
}

POCS_HD bool pocs_box_narrow(double px, double py, double sn, double cs, double rx, double ry,
                             const double* o) {
  const double dx = o[0] - px;
  const double dy = o[1] - py;
  const double ax = o[2], ay = o[3], hx = o[4], hy = o[5];
  if (ax == 1.0 && ay == 0.0)                                     // wave-uniform: the relative yaw IS the heading, the offset as it is
    return pocs_box_margins(dx, dy, sn, cs, rx, ry, hx, hy, cs, sn, dx, dy);
  return pocs_box_margins(dx, dy, sn, cs, rx, ry, hx, hy,
                          fma(cs, ax, sn * ay),                   // cos of the relative yaw
                          fma(sn, ax, -(cs * ay)),                // sin of the relative yaw
                          fma(dx, ax, dy * ay),                   // d in the obstacle frame
                          fma(dy, ax, -(dx * ay)));
}

// Broad phase + narrow phase against one record (host-side convenience, same result).
POCS_HD bool pocs_box_hit(double px, double py, double sn, double cs, double rx, double ry,
                          const double* o) {
  if (fabs(o[0] - px) > o[6] || fabs(o[1] - py) > o[7]) return false;
  return pocs_box_narrow(px, py, sn, cs, rx, ry, o);
}

// ---- round obstacles (pocs_set_discs) ---------------------------------------------------------------------------------
// A disc {cx, cy, r} occupies one record of the table, behind the boxes, prepared as its bounding square -- centre, axis (1, 0),
// hx = hy = r, fields 6 and 7 exactly as pocs_prepare_obstacle forms them for that square -- with ONE difference: ay is -0.0, the
// marker.  -0.0 is arithmetic-neutral wherever a record is read (|ay| = 0, ay == 0.0, products with it are zeros), so the broad
// phase, gmm_cull's keep test and its heading-tightened box read the record as the square's and stay conservative (a disc lies
// inside its square), and the culls' copies of fields 0 .. 5 carry the marker into the kept lists.  A BOX record never holds
// ay = -0.0 in a table that may hold discs: pocs_prepare_box_beside_discs writes +0.0 for a zero sine (no result of the box test
// depends on the sign of a zero ay: it is read through ax == 1.0 && ay == 0.0, products and fabs).
// The test below is exact: the squared distance from the disc's centre to the footprint's box, in the footprint's frame, against
// r^2, touching included.  The flag is broad phase AND narrow phase, as pocs_box_hit is.
POCS_HD void pocs_prepare_disc(const double disc3[3], const pocs_footprint* fp, double* rec) {
  const double sq[5] = {disc3[0], disc3[1], disc3[2], disc3[2], 0.0};
  pocs_prepare_obstacle(sq, fp, rec);
  rec[2] = 1.0; rec[3] = -0.0;
}
POCS_HD void pocs_prepare_box_beside_discs(const double box5[5], const pocs_footprint* fp, double* rec) {
  pocs_prepare_obstacle(box5, fp, rec);
  // a yaw of -0.0 gives ay = -0.0: written as +0.0, so that the marker means a disc.  (fabs of a zero is +0.0 under any
  // floating-point flags; the nonzero values are kept as they are)
  rec[3] = rec[3] == 0.0 ? fabs(rec[3]) : rec[3];
}
POCS_HD bool pocs_record_is_disc(double ay) { return ay == 0.0 && __builtin_signbit(ay); }

// Narrow phase for a disc record that has passed the broad phase: the operations of the specification, in its order.
POCS_HD bool pocs_disc_narrow(double px, double py, double sn, double cs, double rx, double ry, const double* o) {
  const double dx = o[0] - px;
  const double dy = o[1] - py;
  const double r = o[4];
  const double d1 = fma(dx, cs, dy * sn);                         // d in the footprint frame (the box test's own d1, d2)
  const double d2 = fma(dy, cs, -(dx * sn));
  const double q1 = fmax(fabs(d1) - rx, 0.0);
  const double q2 = fmax(fabs(d2) - ry, 0.0);
  return !(fma(q1, q1, q2 * q2) > r * r);
}
// pocs_box_hit for a table that may hold discs: the record's kind is the same in every lane (a wave-uniform branch, as the
// ax == 1.0 && ay == 0.0 test of pocs_box_narrow is).
POCS_HD bool pocs_world_hit(double px, double py, double sn, double cs, double rx, double ry, const double* o) {
  if (fabs(o[0] - px) > o[6] || fabs(o[1] - py) > o[7]) return false;
  if (pocs_record_is_disc(o[3])) return pocs_disc_narrow(px, py, sn, cs, rx, ry, o);
  return pocs_box_narrow(px, py, sn, cs, rx, ry, o);
}

// checkCollision for one pose: true if the footprint touches any of the M obstacles.
// ROUND (pocs_set_discs with D > 0): the table may hold disc records (pocs_world_hit); ROUND = false is the function as it has
// always been.
template <bool ROUND = false>
POCS_HD bool pocs_pose_collides(double x, double y, double th, const pocs_footprint* fp,
                                const double* obs, int M, const pocs_tables* T, const pocs_vconst* V = nullptr) {
  if (M <= 0) return false;                     // nothing in reach (k_gmm_step: every obstacle culled): no heading needed
  double sn, cs;
  pocs_sincos_tab(th, T, &sn, &cs, V);
  double px = x, py = y;
  if (!(fp->dx == 0.0 && fp->dy == 0.0)) {      // a centred footprint skips x + (c*0 - s*0) == x
#if defined(__HIP_DEVICE_COMPILE__)
    // keeps this a (scalar) BRANCH: left alone the compiler computes both and selects, 10 vector
    // instructions per pose for a footprint that is centred in every scene of the reference
    asm volatile("; offset footprint");
#endif
    px = x + fma(cs, fp->dx, -(sn * fp->dy));
    py = y + fma(sn, fp->dx, cs * fp->dy);
  }
  bool hit = false;                             // (set under a condition, not or-ed in: see pocs_pair_collides)
  if constexpr (ROUND) {
    for (int m = 0; m < M; ++m)
      if (pocs_world_hit(px, py, sn, cs, fp->hx, fp->hy, obs + m * POCS_OBS_STRIDE)) hit = true;
  } else {
    for (int m = 0; m < M; ++m)
      if (pocs_box_hit(px, py, sn, cs, fp->hx, fp->hy, obs + m * POCS_OBS_STRIDE)) hit = true;
  }
  return hit;
}
// One pose against a table that may hold discs, the two kinds apart: bit 0 = touches some box, bit 1 = touches some disc (the
// flag of pocs_pose_collides<true> is kinds != 0).  The probe's and the host harness' way in.
POCS_HD unsigned pocs_pose_kinds_touched(double x, double y, double th, const pocs_footprint* fp,
                                         const double* obs, int M, const pocs_tables* T, const pocs_vconst* V = nullptr) {
  if (M <= 0) return 0u;
  double sn, cs;
  pocs_sincos_tab(th, T, &sn, &cs, V);
  double px = x, py = y;
  if (!(fp->dx == 0.0 && fp->dy == 0.0)) {
    px = x + fma(cs, fp->dx, -(sn * fp->dy));
    py = y + fma(sn, fp->dx, cs * fp->dy);
  }
  unsigned kinds = 0u;
  for (int m = 0; m < M; ++m) {
    const double* o = obs + m * POCS_OBS_STRIDE;
    if (pocs_world_hit(px, py, sn, cs, fp->hx, fp->hy, o)) kinds |= pocs_record_is_disc(o[3]) ? 2u : 1u;
  }
  return kinds;
}

// ---- uncertain discs (pocs_set_disc_covariances) ----------------------------------------------------------------------
// A disc's centre may carry a position covariance {sxx, sxy, syy}.  The host factorises it as the initial covariance is
// factorised (pocs_disc_noise_factor: l00 = sqrt(sxx), l10 = sxy / l00, l11 = sqrt(syy - l10 l10), double arithmetic in that
// order) into the record's ROW of the noise table, {l00, l10, l11, d} with d the disc's index in the caller's table; a row of
// zeros is a certain disc or a box and draws nothing (an uncertain row has l00 > 0).  A pose is one possible world: for pose
// index i, the run's seed, disc d and waypoint word v
//   words = Philox4x32-7((lo32(i >> 1), hi32(i >> 1), v, 5 << 16 | d), seed)        (pocs_draw, POCS_STREAM_DISC)
//   (z0, z1) = pocs_normal_pair_w2(words[2 h], words[2 h + 1]),  h = i & 1          (one draw serves poses 2 j and 2 j + 1)
//   cx' = fma(l00, z0, cx)     cy' = fma(l11, z1, fma(l10, z0, cy))
// and the flag is the broad phase on the NOMINAL centre AND pocs_disc_narrow's operations on (cx', cy').
// Why the culls stay exact: |z| <= sqrt(64 ln 2) < 6.661 (pocs_normal_pair_w2), so |cx' - cx| <= 6.661 |l00| and
// |cy' - cy| <= 6.661 (|l10| + |l11|) up to the rounding of two fmas (relative 2^-52, far inside the 0.1 % that 6.67 leaves).
// The record's fields 6 and 7 are grown on the host by gx = 6.67 |l00| and gy = 6.67 (|l10| + |l11|) (pocs_disc_noise_grow):
// the displaced disc lies inside the nominal bounding square moved by at most (gx, gy), so a pose that the grown broad phase
// rejects is further than the footprint's bounding radius from every displaced square and cannot touch.  gmm_cull tightens a
// kept record's box to the record's own extents plus the footprint's extents over the run's headings; with + gx, + gy
// (gmm_cull<.., RN>) the same argument holds for the tightened box, and its keep test reads the grown fields: no flag changes.
#define POCS_NOISE_STRIDE 4
// 0: a row was written (uncertain, l00 > 0), 1: all zeros, a certain disc (the row is zeros), -1: not a covariance
POCS_HD int pocs_disc_noise_factor(const double cov3[3], double row3[3]) {
  row3[0] = row3[1] = row3[2] = 0.0;
  for (int j = 0; j < 3; ++j)
    if (!__builtin_isfinite(cov3[j])) return -1;
  if (cov3[0] == 0.0 && cov3[1] == 0.0 && cov3[2] == 0.0) return 1;
  if (!(cov3[0] > 0.0)) return -1;
  const double l00 = sqrt(cov3[0]);
  const double l10 = cov3[1] / l00;
  const double t = cov3[2] - l10 * l10;
  if (!(t > 0.0) || !__builtin_isfinite(l10)) return -1;
  row3[0] = l00; row3[1] = l10; row3[2] = sqrt(t);
  return 0;
}
// the growth of a prepared disc record's fields 6 and 7 (pocs_prepare_disc forms them first, unchanged)
POCS_HD void pocs_disc_noise_grow(const double row3[3], double* rec) {
  rec[6] += 6.67 * fabs(row3[0]);
  rec[7] += 6.67 * (fabs(row3[1]) + fabs(row3[2]));
}
// the displaced centre of the disc of row `row` (l00 != 0) for pose index `index`
POCS_HD void pocs_disc_displaced(double cx, double cy, const double* row, uint64_t seed, uint64_t index, uint32_t v,
                                 const pocs_tables* T, double* cxp, double* cyp, const pocs_vconst* V = nullptr) {
  const pocs_u32x4 w = pocs_draw(seed, index >> 1, v, POCS_STREAM_DISC, (uint32_t)row[3]);
  double z0, z1;
  if (index & 1ull) pocs_normal_pair_w2(w.z, w.w, T, &z0, &z1, V);
  else              pocs_normal_pair_w2(w.x, w.y, T, &z0, &z1, V);
  *cxp = fma(row[0], z0, cx);
  *cyp = fma(row[2], z1, fma(row[1], z0, cy));
}
// pocs_world_hit for a table whose disc records may be uncertain: `row` is the record's row of the noise table
POCS_HD bool pocs_world_hit_noisy(double px, double py, double sn, double cs, double rx, double ry, const double* o, const double* row,
                                  uint64_t seed, uint64_t index, uint32_t v, const pocs_tables* T) {
  if (fabs(o[0] - px) > o[6] || fabs(o[1] - py) > o[7]) return false;
  if (pocs_record_is_disc(o[3])) {
    if (row[0] != 0.0) {                                             // (wave-uniform) an uncertain disc: the test on the displaced centre
      double d[5];
      pocs_disc_displaced(o[0], o[1], row, seed, index, v, T, &d[0], &d[1]);
      d[4] = o[4];
      return pocs_disc_narrow(px, py, sn, cs, rx, ry, d);
    }
    return pocs_disc_narrow(px, py, sn, cs, rx, ry, o);
  }
  return pocs_box_narrow(px, py, sn, cs, rx, ry, o);
}
// pocs_pose_collides<true> under disc covariances, beside it: `rows` holds POCS_NOISE_STRIDE doubles per record of `obs`.
// `discs_touched`, where given, receives bit (row[3]) per touched DISC record (the probe's and the harness' way in; D <= 32 there).
// T: ALL the tables -- the heading reads the sector table, the draw the log tables of the radius too (on the device: the staged
// copy, whose even log entries stage_tables has doubled).
POCS_HD bool pocs_pose_collides_noisy(double x, double y, double th, const pocs_footprint* fp, const double* obs, const double* rows, int M,
                                      uint64_t seed, uint64_t index, uint32_t v, const pocs_tables* T, unsigned* discs_touched = nullptr) {
  if (discs_touched) *discs_touched = 0u;
  if (M <= 0) return false;
  double sn, cs;
  pocs_sincos_tab(th, T, &sn, &cs);
  double px = x, py = y;
  if (!(fp->dx == 0.0 && fp->dy == 0.0)) {
    px = x + fma(cs, fp->dx, -(sn * fp->dy));
    py = y + fma(sn, fp->dx, cs * fp->dy);
  }
  bool hit = false;
  for (int m = 0; m < M; ++m) {
    const double* o = obs + m * POCS_OBS_STRIDE;
    const double* row = rows + m * POCS_NOISE_STRIDE;
    if (pocs_world_hit_noisy(px, py, sn, cs, fp->hx, fp->hy, o, row, seed, index, v, T)) {
      hit = true;
      if (discs_touched && pocs_record_is_disc(o[3])) *discs_touched |= 1u << ((unsigned)row[3] & 31u);
    }
  }
  return hit;
}

// ---- prediction hypotheses (pocs_set_disc_hypotheses) ------------------------------------------------------------------
// A disc may be one ALTERNATIVE of a group: the alternatives of a group exclude each other, for one pose at most one of them
// exists.  The host forms exact integer thresholds (pocs_hyp_thresholds): n_d = floor(weight_d 2^32) -- the product is exact --,
// and within a group in ascending d, lo_d = the sum of n_e over the earlier discs e < d of the group, hi_d = lo_d + n_d <= 2^32.
// A pose is one possible world: for pose index i, the run's seed, group g and waypoint word v
//   words = Philox4x32-7((lo32(i >> 1), hi32(i >> 1), v, 6 << 16 | g), seed)        (pocs_draw, POCS_STREAM_HYP)
//   u = words[2 h],  h = i & 1                                                      (one draw serves poses 2 j and 2 j + 1)
// and disc d exists for the pose iff lo_d <= u < hi_d: integers, nothing is floating point.  The record's GATE is four 32-bit
// words {lo, hi - 1, g, on} (hi - 1 fits: n_d >= 1); on = 0 is a box or a disc that is always there, and draws nothing.
// The flag of a gated record is "exists" AND the record's test as it is without this (the broad phase on the nominal centre with
// the grown fields, the narrow phase, on the displaced centre for an uncertain disc); streams 5 and 6 are independent.
// Why the culls stay exact: removing a disc for a pose can only remove hits.  Every cull keeps a record when SOME pose in reach
// could touch it; a record that is dropped touches no pose whether it exists or not, and a record that is kept is tested pose
// by pose with its gate.  So the table's fields 6 and 7, gmm_cull's keep test and its tightened box stand with no change to any
// record, as they stood under the growth (the block above pocs_disc_noise_factor).
#define POCS_GATE_STRIDE 4
// The thresholds of a table of D alternatives; lo, hi: D entries each.  0: formed; otherwise what the setter refuses, 1: a group
// outside [-1, D), 2: a weight that is not finite or outside (0, 1], 3: n_d = 0, 4: a group whose last hi exceeds 2^32 -- and
// *bad is the disc.  A disc of group -1 has lo = 0, hi = 2^32 and its weight is not read.
POCS_HD int pocs_hyp_thresholds(const int* group, const double* weight, int D, unsigned long long* lo, unsigned long long* hi, int* bad) {
  for (int d = 0; d < D; ++d) {
    *bad = d;
    if (group[d] < -1 || group[d] >= D) return 1;
    if (group[d] < 0) { lo[d] = 0ull; hi[d] = 1ull << 32; continue; }
    if (!__builtin_isfinite(weight[d]) || !(weight[d] > 0.0) || !(weight[d] <= 1.0)) return 2;
    const unsigned long long n = (unsigned long long)floor(weight[d] * 4294967296.0);
    if (n == 0ull) return 3;
    unsigned long long l = 0ull;
    for (int e = 0; e < d; ++e)
      if (group[e] == group[d]) l = hi[e];                           // (ascending e: the last earlier one's hi is the sum so far)
    lo[d] = l; hi[d] = l + n;
    if (hi[d] > (1ull << 32)) return 4;
  }
  return 0;
}
POCS_HD void pocs_hyp_gate(int group, unsigned long long lo, unsigned long long hi, uint32_t* gate) {
  gate[0] = group < 0 ? 0u : (uint32_t)lo;
  gate[1] = group < 0 ? 0xFFFFFFFFu : (uint32_t)(hi - 1ull);
  gate[2] = group < 0 ? 0u : (uint32_t)group;
  gate[3] = group < 0 ? 0u : 1u;
}
// the existence word of group g for pose index `index`
POCS_HD uint32_t pocs_hyp_word(uint64_t seed, uint64_t index, uint32_t v, uint32_t g) {
  const pocs_u32x4 w = pocs_draw(seed, index >> 1, v, POCS_STREAM_HYP, g);
  return (index & 1ull) ? w.z : w.x;
}
// does the record of gate `gate` exist for the pose?  (on = 0: always)
POCS_HD bool pocs_hyp_exists(const uint32_t* gate, uint64_t seed, uint64_t index, uint32_t v) {
  if (gate[3] == 0u) return true;
  const uint32_t u = pocs_hyp_word(seed, index, v, gate[2]);
  return gate[0] <= u && u <= gate[1];
}
// pocs_world_hit_noisy for a table whose disc records may be gated: `gate` is the record's gate, `row` its row of the noise table
// (rows may be null: no covariances), v the deviations' waypoint word and vh the hypotheses'
POCS_HD bool pocs_world_hit_gated(double px, double py, double sn, double cs, double rx, double ry, const double* o, const double* row,
                                  const uint32_t* gate, uint64_t seed, uint64_t index, uint32_t v, uint32_t vh, const pocs_tables* T) {
  if (fabs(o[0] - px) > o[6] || fabs(o[1] - py) > o[7]) return false;
  if (pocs_record_is_disc(o[3])) {
    if (!pocs_hyp_exists(gate, seed, index, vh)) return false;       // (the gate is wave-uniform, the answer is the lane's)
    if (row && row[0] != 0.0) {
      double d[5];
      pocs_disc_displaced(o[0], o[1], row, seed, index, v, T, &d[0], &d[1]);
      d[4] = o[4];
      return pocs_disc_narrow(px, py, sn, cs, rx, ry, d);
    }
    return pocs_disc_narrow(px, py, sn, cs, rx, ry, o);
  }
  return pocs_box_narrow(px, py, sn, cs, rx, ry, o);
}
// pocs_pose_collides_noisy under hypotheses, beside it: `gates` holds POCS_GATE_STRIDE words per record of `obs`, `rows` (null: no
// covariances) POCS_NOISE_STRIDE doubles.  `exists` / `touched`, where given, receive bit m per DISC record m that exists for the
// pose / that the pose touches (the probe's and the harness' way in; M <= 32 there).
POCS_HD bool pocs_pose_collides_gated(double x, double y, double th, const pocs_footprint* fp, const double* obs, const double* rows,
                                      const uint32_t* gates, int M, uint64_t seed, uint64_t index, uint32_t v, uint32_t vh,
                                      const pocs_tables* T, unsigned* exists = nullptr, unsigned* touched = nullptr) {
  if (exists) *exists = 0u;
  if (touched) *touched = 0u;
  if (M <= 0) return false;
  double sn, cs;
  pocs_sincos_tab(th, T, &sn, &cs);
  double px = x, py = y;
  if (!(fp->dx == 0.0 && fp->dy == 0.0)) {
    px = x + fma(cs, fp->dx, -(sn * fp->dy));
    py = y + fma(sn, fp->dx, cs * fp->dy);
  }
  bool hit = false;
  for (int m = 0; m < M; ++m) {
    const double* o = obs + m * POCS_OBS_STRIDE;
    const uint32_t* gate = gates + m * POCS_GATE_STRIDE;
    if (exists && pocs_record_is_disc(o[3]) && pocs_hyp_exists(gate, seed, index, vh)) *exists |= 1u << ((unsigned)m & 31u);
    if (pocs_world_hit_gated(px, py, sn, cs, fp->hx, fp->hy, o, rows ? rows + m * POCS_NOISE_STRIDE : nullptr, gate, seed, index, v, vh, T)) {
      hit = true;
      if (touched && pocs_record_is_disc(o[3])) *touched |= 1u << ((unsigned)m & 31u);
    }
  }
  return hit;
}

// ---- a round footprint (pocs_set_footprint_disc) ------------------------------------------------------------------------
// The robot is a disc of radius rho >= 0 centred on the pose's reference point (rho = 0: a point).  It has no heading: theta is never
// read, and no sine or cosine appears anywhere below.  The records are the table's as it is under discs -- boxes by
// pocs_prepare_box_beside_discs' rule (a zero sine is +0.0), discs as their bounding squares with the ay = -0.0 marker, an uncertain
// disc's fields 6 and 7 grown by pocs_disc_noise_grow -- with ONE difference: the footprint's bounding radius in fields 6 and 7 is
// rho itself, pocs_prepare_obstacle's operations in their order with rho in place of sqrt(hx^2 + hy^2).  The flag is broad phase AND
// narrow phase, touching included:
//   box record    e = the offset in the obstacle's frame (pocs_box_narrow's e1, e2), q_i = fmax(|e_i| - h_i, 0), the squared distance
//                 from the pose to the box fma(q1, q1, q2 q2) against rho rho.  An axis-aligned record takes e = (dx, dy): the same bits
//                 (fma(dx, 1, dy * 0) is dx up to the sign of a zero, which the absolute value drops)
//   disc record   R = r + rho, fma(dx, dx, dy dy) against R R; an uncertain disc: the same on the displaced centre (pocs_disc_displaced)
POCS_HD void pocs_prepare_obstacle_round(const double box5[5], double rho, double* rec) {
  double sn, cs;
  pocs_sincos(box5[4], &sn, &cs);
  rec[0] = box5[0]; rec[1] = box5[1];
  rec[2] = cs; rec[3] = sn == 0.0 ? fabs(sn) : sn;                 // (pocs_prepare_box_beside_discs: the marker means a disc)
  rec[4] = box5[2]; rec[5] = box5[3];
  rec[6] = (box5[2] * fabs(cs) + box5[3] * fabs(sn)) + rho;
  rec[7] = (box5[2] * fabs(sn) + box5[3] * fabs(cs)) + rho;
}
POCS_HD void pocs_prepare_disc_round(const double disc3[3], double rho, double* rec) {
  const double sq[5] = {disc3[0], disc3[1], disc3[2], disc3[2], 0.0};
  pocs_prepare_obstacle_round(sq, rho, rec);
  rec[2] = 1.0; rec[3] = -0.0;
}
// The two narrow phases, for a record that has passed the broad phase: (dx, dy) = the record's centre minus the pose.
POCS_HD bool pocs_round_box_narrow(double dx, double dy, double rho, const double* o) {
  const double ax = o[2], ay = o[3];
  const double e1 = fma(dx, ax, dy * ay);
  const double e2 = fma(dy, ax, -(dx * ay));
  const double q1 = fmax(fabs(e1) - o[4], 0.0);
  const double q2 = fmax(fabs(e2) - o[5], 0.0);
  return !(fma(q1, q1, q2 * q2) > rho * rho);
}
POCS_HD bool pocs_round_disc_narrow(double dx, double dy, double rho, double r) {
  const double R = r + rho;
  return !(fma(dx, dx, dy * dy) > R * R);
}
// pocs_world_hit's twin
POCS_HD bool pocs_round_world_hit(double x, double y, double rho, const double* o) {
  const double dx = o[0] - x, dy = o[1] - y;
  if (fabs(dx) > o[6] || fabs(dy) > o[7]) return false;
  if (pocs_record_is_disc(o[3])) return pocs_round_disc_narrow(dx, dy, rho, o[4]);
  return pocs_round_box_narrow(dx, dy, rho, o);
}
// pocs_world_hit_noisy's twin: the broad phase on the nominal centre, an uncertain disc's narrow phase on the displaced one
POCS_HD bool pocs_round_world_hit_noisy(double x, double y, double rho, const double* o, const double* row, uint64_t seed, uint64_t index,
                                        uint32_t v, const pocs_tables* T) {
  const double dx = o[0] - x, dy = o[1] - y;
  if (fabs(dx) > o[6] || fabs(dy) > o[7]) return false;
  if (pocs_record_is_disc(o[3])) {
    if (row[0] != 0.0) {                                             // (wave-uniform) an uncertain disc
      double cxp, cyp;
      pocs_disc_displaced(o[0], o[1], row, seed, index, v, T, &cxp, &cyp);
      return pocs_round_disc_narrow(cxp - x, cyp - y, rho, o[4]);
    }
    return pocs_round_disc_narrow(dx, dy, rho, o[4]);
  }
  return pocs_round_box_narrow(dx, dy, rho, o);
}
// One pose against the table, the two kinds apart as pocs_pose_kinds_touched gives them: bit 0 = touches some box, bit 1 = touches
// some disc; the flag is kinds != 0.  `rows` (null: no covariances): POCS_NOISE_STRIDE doubles per record of `obs`, and then the
// pose's index, the seed, the waypoint word and ALL the tables (pocs_pose_collides_noisy) are read.
POCS_HD unsigned pocs_round_pose_kinds(double x, double y, double rho, const double* obs, int M, const double* rows = nullptr,
                                       uint64_t seed = 0, uint64_t index = 0, uint32_t v = 0, const pocs_tables* T = nullptr) {
  unsigned kinds = 0u;
  for (int m = 0; m < M; ++m) {
    const double* o = obs + m * POCS_OBS_STRIDE;
    const bool t = rows ? pocs_round_world_hit_noisy(x, y, rho, o, rows + m * POCS_NOISE_STRIDE, seed, index, v, T)
                        : pocs_round_world_hit(x, y, rho, o);
    if (t) kinds |= pocs_record_is_disc(o[3]) ? 2u : 1u;
  }
  return kinds;
}
// checkCollision for one pose under a round footprint, and its twin under disc covariances (the MC kernels' forms)
POCS_HD bool pocs_round_pose_collides(double x, double y, double rho, const double* obs, int M) {
  bool hit = false;                                                // (set under a condition, not or-ed in: see pocs_pair_collides)
  for (int m = 0; m < M; ++m)
    if (pocs_round_world_hit(x, y, rho, obs + m * POCS_OBS_STRIDE)) hit = true;
  return hit;
}
POCS_HD bool pocs_round_pose_collides_noisy(double x, double y, double rho, const double* obs, const double* rows, int M, uint64_t seed,
                                            uint64_t index, uint32_t v, const pocs_tables* T) {
  bool hit = false;
  for (int m = 0; m < M; ++m)
    if (pocs_round_world_hit_noisy(x, y, rho, obs + m * POCS_OBS_STRIDE, rows + m * POCS_NOISE_STRIDE, seed, index, v, T)) hit = true;
  return hit;
}

// The same predicate for the two poses a thread of k_gmm_step draws per iteration, with ONE pass over the obstacle
// table (it sits in LDS) and the loop's bookkeeping paid once.  Per pose exactly the operations of pocs_pose_collides, in
// the same order: the same flags.  On the device (pocs_pair_loop) the compiled loop
//   - fetches a record ONCE for both poses, as 16-byte reads from an address held in one vector register that advances
//     per record: (cx, cy) and (bx, by) for the broad phase, and (ax, ay), (hx, hy) where some lane of either pose is
//     inside the record's box (the compiler issues that second pair behind the scalar branch);
//   - computes the headings' sines and cosines once per call at most, the first time some lane of either pose passes a
//     record's broad phase (a wave-uniform branch), when the footprint is centred: x, y and the record decide the broad
//     phase alone then, and are used in place.  An offset footprint needs the heading for (px, py) and keeps it in front;
//   - hands back each pose's flag as a 64-bit LANE MASK in scalar registers: a record's answer is balloted where the
//     narrow phase has given it and or-ed in by a scalar instruction.  The mask is zero when M <= 0.
//   EAGER (k_gmm_step's lone form, whose sampling phase is latency): a record's eight doubles are all waited for at the
//   head of its iteration, once.
// The host path keeps the plain loop below.
#if defined(__HIPCC__)
typedef double pocs_v2d __attribute__((ext_vector_type(2)));
struct pocs_each_none { __device__ __forceinline__ void operator()(int, int, bool) const {} };

// pocs_box_margins for the lanes of `pm` (those inside the record's broad-phase box), the answer as a lane mask.  Every
// branch is wave-uniform: the wave computes with all its lanes -- a vector instruction costs the same under any exec mask
// -- and the lanes that count are picked by scalar ands of compare results, so no flag ever lives in a vector register.
// Per lane the operations of pocs_box_margins, in its order, with its early return after the obstacle's own axes.
__device__ __forceinline__ unsigned long long pocs_box_margins_mask(unsigned long long pm, double dx, double dy, double sn, double cs,
                                                                    double rx, double ry, double hx, double hy,
                                                                    double cr, double sr, double e1, double e2,
                                                                    double p3, double p4) {
  // p3, p4: the footprint's extents along the obstacle's axes, fma(rx, |cr|, ry * |sr|) and fma(rx, |sr|, ry * |cr|) -- the
  // caller's, because for an axis-aligned record they are functions of the heading alone, formed once with it
  const double m3 = fabs(e1) - (hx + p3);
  const double m4 = fabs(e2) - (hy + p4);
  const unsigned long long near = pm & __builtin_amdgcn_ballot_w64(!(fmax(m3, m4) > 0.0));
  if (near == 0ull) return 0ull;
  asm volatile("; footprint axes");                                // keeps the early return a branch
  const double d1 = fma(dx, cs, dy * sn);
  const double d2 = fma(dy, cs, -(dx * sn));
  const double m1 = fabs(d1) - (rx + fma(hx, fabs(cr), hy * fabs(sr)));
  const double m2 = fabs(d2) - (ry + fma(hx, fabs(sr), hy * fabs(cr)));
  return near & __builtin_amdgcn_ballot_w64(!(fmax(m1, m2) > 0.0));
}

// pocs_disc_narrow for the lanes of `pm`, the answer as a lane mask: per lane its operations in its order, balloted.
__device__ __forceinline__ unsigned long long pocs_disc_narrow_mask(unsigned long long pm, double dx, double dy, double sn, double cs,
                                                                    double rx, double ry, double r) {
  const double d1 = fma(dx, cs, dy * sn);
  const double d2 = fma(dy, cs, -(dx * sn));
  const double q1 = fmax(fabs(d1) - rx, 0.0);
  const double q2 = fmax(fabs(d2) - ry, 0.0);
  return pm & __builtin_amdgcn_ballot_w64(!(fma(q1, q1, q2 * q2) > r * r));
}

// What the pair loop needs for uncertain discs (pocs_set_disc_covariances; the block above pocs_disc_noise_factor): the rows of the
// list it runs over (LDS, POCS_NOISE_STRIDE doubles per record, in the list's order), the run's seed, the lane's PAIR index
// (poses 2 pair and 2 pair + 1) and the waypoint word.  pocs_noise_none: no such thing, and not one instruction of it.
struct pocs_noise_none { static constexpr bool on = false; };
struct pocs_noise_pair {
  static constexpr bool on = true;
  const double* rows;
  uint64_t seed, pair;
  uint32_t v;
};
// Hypotheses (pocs_set_disc_hypotheses; the block above pocs_hyp_thresholds) on top of that: the GATES of the list the loop runs over
// as well (LDS, POCS_GATE_STRIDE words per record, in the list's order) and the hypotheses' waypoint word.  The rows may all be zeros.
struct pocs_noise_gate_pair {
  static constexpr bool on = true;
  const double* rows;
  uint64_t seed, pair;
  uint32_t v;
  const uint32_t* gates;
  uint32_t vh;
};
template <class NZ> struct pocs_nz_gated { static constexpr bool value = false; };
template <> struct pocs_nz_gated<pocs_noise_gate_pair> { static constexpr bool value = true; };

// ROUND: the table may hold disc records; a record's kind is decided by a scalar branch on a ballot of its marker (every lane
// reads the same record), and `kinds`, where given, receives the two poses' masks for the disc records apart: kinds[h] is the part
// of mask[h] that discs contributed.
// NZ = pocs_noise_pair (ROUND only): behind the disc branch a second scalar branch on the record's row -- every lane reads the same
// one -- and for an uncertain disc ONE Philox call per pair, a Box-Muller pair per pose whose broad phase some lane passed, and
// pocs_disc_narrow's operations on the displaced centre.
// NZ = pocs_noise_gate_pair: in front of that a scalar branch on the record's gate -- every lane reads the same one -- and for a gated
// disc that some lane's broad phase passed ONE Philox call per pair and an integer range compare per pose, balloted and and-ed into
// the pose's broad-phase mask by a scalar instruction: a lane for whose pose the disc does not exist takes no part in the record's
// narrow phase; a record that exists for no lane inside its box still draws its deviation's Philox words (one call per pair) and
// skips the Box-Muller pairs and the narrow phase of both poses.
template <bool EAGER, bool CENTRED, class Each, bool ROUND = false, class NZ = pocs_noise_none>
__device__ __forceinline__ void pocs_pair_loop(const double x[2], const double y[2], const double th[2], const pocs_footprint* fp,
                                               const double* obs, int M, const pocs_tables* T, const pocs_vconst* V,
                                               unsigned long long mask[2], Each each, unsigned long long* kinds = nullptr, NZ nz = NZ()) {
  static_assert(!NZ::on || ROUND, "uncertain discs: the ROUND form");
  const double rx = fp->hx, ry = fp->hy;
  double sn[2], cs[2], px[2], py[2];
  [[maybe_unused]] unsigned long long k0 = 0ull, k1 = 0ull;
  double ex[2], ey[2];                                             // the footprint's extents along world x and y at the two headings
  bool heading = false;                                            // (wave-uniform) sn, cs, ex, ey hold the two headings' values
  // (until then they hold nothing: said to the compiler, which otherwise zeroes them in front of the loop)
  if (CENTRED) asm volatile("" : "=v"(sn[0]), "=v"(cs[0]), "=v"(sn[1]), "=v"(cs[1]), "=v"(ex[0]), "=v"(ey[0]), "=v"(ex[1]), "=v"(ey[1]));
  if (!CENTRED) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      pocs_sincos_tab(th[h], T, &sn[h], &cs[h], V);
      px[h] = x[h] + fma(cs[h], fp->dx, -(sn[h] * fp->dy));
      py[h] = y[h] + fma(sn[h], fp->dx, cs[h] * fp->dy);
      ex[h] = fma(rx, fabs(cs[h]), ry * fabs(sn[h]));
      ey[h] = fma(rx, fabs(sn[h]), ry * fabs(cs[h]));
    }
    heading = true;
  }
  unsigned long long m0 = 0ull, m1 = 0ull;
  // the record's address: LDS, one vector register, advanced per record (left to itself the compiler keeps it scalar and
  // moves it into a vector register in front of every read)
  const __attribute__((address_space(3))) pocs_v2d* o = (const __attribute__((address_space(3))) pocs_v2d*)obs;
  asm volatile("" : "+v"(o));
  for (int m = 0; m < M; ++m, o += POCS_OBS_STRIDE / 2) {
    pocs_v2d c = o[0], b = o[3], a = o[1], e = o[2];               // (cx, cy) (bx, by) | (ax, ay) (hx, hy)
    if (EAGER) asm volatile("" : "+v"(c), "+v"(b), "+v"(a), "+v"(e));
    double dx[2], dy[2];
    unsigned long long pm[2], bt[2] = {0ull, 0ull};
#pragma unroll
    for (int h = 0; h < 2; ++h) {                                  // pocs_box_hit's broad phase
      dx[h] = c.x - (CENTRED ? x[h] : px[h]);
      dy[h] = c.y - (CENTRED ? y[h] : py[h]);
      pm[h] = __builtin_amdgcn_ballot_w64(!(fabs(dx[h]) > b.x)) & __builtin_amdgcn_ballot_w64(!(fabs(dy[h]) > b.y));
    }
    if ((pm[0] | pm[1]) != 0ull) {                                 // pocs_box_narrow for the lanes inside the box
      if (CENTRED && !heading) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          double t = th[h];
          asm volatile("" : "+v"(t));                              // the argument reduction stays in here too: not hoisted in front of the loop
          pocs_sincos_tab(t, T, &sn[h], &cs[h], V);
          ex[h] = fma(rx, fabs(cs[h]), ry * fabs(sn[h]));
          ey[h] = fma(rx, fabs(sn[h]), ry * fabs(cs[h]));
        }
        heading = true;
      }
      // an axis-aligned record (every lane reads the same one): the relative yaw IS the heading, the offset as it is
      bool disc = false;                                             // (scalar) the record is a disc: ay is -0.0
      if constexpr (ROUND) {
        const double ay = a.y;                                       // (a copy: the bits of THIS element are compared)
        disc = __builtin_amdgcn_ballot_w64(__builtin_bit_cast(unsigned long long, ay) == 0x8000000000000000ull) != 0ull;
      }
      if (ROUND && disc) {
        if constexpr (pocs_nz_gated<NZ>::value) {
          const uint32_t* const gt = nz.gates + m * POCS_GATE_STRIDE;
          const uint32_t g_on = gt[3];
          if (__builtin_amdgcn_ballot_w64(g_on != 0u) != 0ull) {     // (scalar) the disc is an alternative of a group
            const pocs_u32x4 wh = pocs_draw(nz.seed, nz.pair, nz.vh, POCS_STREAM_HYP, gt[2]);
            const uint32_t g_lo = gt[0], g_him = gt[1];
            pm[0] &= __builtin_amdgcn_ballot_w64(g_lo <= wh.x && wh.x <= g_him);
            pm[1] &= __builtin_amdgcn_ballot_w64(g_lo <= wh.z && wh.z <= g_him);
          }
        }
        bool noisy = false;                                          // (scalar) the disc is uncertain: its row's l00 is not zero
        if constexpr (NZ::on) {
          const double* const row = nz.rows + m * POCS_NOISE_STRIDE;
          const double l00 = row[0];
          noisy = __builtin_amdgcn_ballot_w64(l00 != 0.0) != 0ull;
          if (noisy) {
            const pocs_u32x4 wd = pocs_draw(nz.seed, nz.pair, nz.v, POCS_STREAM_DISC, (uint32_t)row[3]);
            const double l10 = row[1], l11 = row[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              if (pm[h] == 0ull) continue;
              double z0, z1;
              pocs_normal_pair_w2(h ? wd.z : wd.x, h ? wd.w : wd.y, T, &z0, &z1, V);
              const double cxp = fma(l00, z0, c.x), cyp = fma(l11, z1, fma(l10, z0, c.y));
              bt[h] = pocs_disc_narrow_mask(pm[h], cxp - (CENTRED ? x[h] : px[h]), cyp - (CENTRED ? y[h] : py[h]), sn[h], cs[h], rx, ry, e.x);
            }
          }
        }
        if (!noisy) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (pm[h] == 0ull) continue;
          bt[h] = pocs_disc_narrow_mask(pm[h], dx[h], dy[h], sn[h], cs[h], rx, ry, e.x);
        }
        }
        if constexpr (ROUND) { k0 |= bt[0]; k1 |= bt[1]; }
      } else {
      const bool turned = (__builtin_amdgcn_ballot_w64(a.x != 1.0) | __builtin_amdgcn_ballot_w64(a.y != 0.0)) != 0ull;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (pm[h] == 0ull) continue;
        if (!turned)
          bt[h] = pocs_box_margins_mask(pm[h], dx[h], dy[h], sn[h], cs[h], rx, ry, e.x, e.y, cs[h], sn[h], dx[h], dy[h], ex[h], ey[h]);
        else {
          const double cr = fma(cs[h], a.x, sn[h] * a.y), sr = fma(sn[h], a.x, -(cs[h] * a.y));      // the relative yaw
          bt[h] = pocs_box_margins_mask(pm[h], dx[h], dy[h], sn[h], cs[h], rx, ry, e.x, e.y, cr, sr,
                                        fma(dx[h], a.x, dy[h] * a.y), fma(dy[h], a.x, -(dx[h] * a.y)),   // d in the obstacle frame
                                        fma(rx, fabs(cr), ry * fabs(sr)), fma(rx, fabs(sr), ry * fabs(cr)));
        }
      }
      }
      m0 |= bt[0]; m1 |= bt[1];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) each(m, h, __builtin_amdgcn_inverse_ballot_w64(bt[h]));
  }
  mask[0] = m0; mask[1] = m1;
  if constexpr (ROUND) { if (kinds) { kinds[0] = k0; kinds[1] = k1; } }
}

// The pair's flags as lane masks (bit l: lane l's pose h touches some record; lanes that do not run the call stay 0).
template <bool EAGER = false, class Each = pocs_each_none, bool ROUND = false, class NZ = pocs_noise_none>
__device__ __forceinline__ void pocs_pair_collides_masks(const double x[2], const double y[2], const double th[2], const pocs_footprint* fp,
                                                         const double* obs, int M, const pocs_tables* T, const pocs_vconst* V,
                                                         unsigned long long mask[2], Each each = Each(), unsigned long long* kinds = nullptr,
                                                         NZ nz = NZ()) {
  mask[0] = 0ull; mask[1] = 0ull;
  if constexpr (ROUND) { if (kinds) { kinds[0] = 0ull; kinds[1] = 0ull; } }
  if (M <= 0) return;
  // (scalar) the loop twice, not one loop behind a merge of (x, y) with (px, py): merged, the centred footprint pays four
  // 64-bit register copies per call for values it already holds
  if (fp->dx == 0.0 && fp->dy == 0.0) {
    if constexpr (NZ::on) {
      pocs_pair_loop<EAGER, true, Each, true, NZ>(x, y, th, fp, obs, M, T, V, mask, each, kinds, nz);
    } else if constexpr (ROUND) {
      pocs_pair_loop<EAGER, true, Each, true>(x, y, th, fp, obs, M, T, V, mask, each, kinds);
    } else {
      pocs_pair_loop<EAGER, true>(x, y, th, fp, obs, M, T, V, mask, each);
    }
  } else {
    asm volatile("; offset footprint");
    if constexpr (NZ::on) {
      pocs_pair_loop<EAGER, false, Each, true, NZ>(x, y, th, fp, obs, M, T, V, mask, each, kinds, nz);
    } else if constexpr (ROUND) {
      pocs_pair_loop<EAGER, false, Each, true>(x, y, th, fp, obs, M, T, V, mask, each, kinds);
    } else {
      pocs_pair_loop<EAGER, false>(x, y, th, fp, obs, M, T, V, mask, each);
    }
  }
}

// The pair form under a round footprint (pocs_set_footprint_disc), in the manner of pocs_pair_loop: one fetch per record serves both
// poses, the record's kind is decided by the scalar branch on its marker, every answer is balloted and or-ed into the pose's lane
// mask by a scalar instruction -- no flag lives in a vector register -- and there is no heading: per pose the operations of
// pocs_round_world_hit (NZ = pocs_noise_pair: of pocs_round_world_hit_noisy, one Philox call per pair and uncertain disc) in their
// order.  `kinds`, where given: the part of each mask that disc records contributed.  The masks are zero when M <= 0.
template <class NZ = pocs_noise_none>
__device__ __forceinline__ void pocs_pair_round_masks(const double x[2], const double y[2], const double rho, const double* obs, int M,
                                                      [[maybe_unused]] const pocs_tables* T, [[maybe_unused]] const pocs_vconst* V,
                                                      unsigned long long mask[2], unsigned long long* kinds = nullptr, [[maybe_unused]] NZ nz = NZ()) {
  unsigned long long m0 = 0ull, m1 = 0ull, k0 = 0ull, k1 = 0ull;
  const double rho2 = rho * rho;
  const __attribute__((address_space(3))) pocs_v2d* o = (const __attribute__((address_space(3))) pocs_v2d*)obs;
  asm volatile("" : "+v"(o));
  for (int m = 0; m < M; ++m, o += POCS_OBS_STRIDE / 2) {
    const pocs_v2d c = o[0], b = o[3], a = o[1], e = o[2];           // (cx, cy) (bx, by) | (ax, ay) (hx, hy)
    double dx[2], dy[2];
    unsigned long long pm[2], bt[2] = {0ull, 0ull};
#pragma unroll
    for (int h = 0; h < 2; ++h) {                                    // the broad phase
      dx[h] = c.x - x[h];
      dy[h] = c.y - y[h];
      pm[h] = __builtin_amdgcn_ballot_w64(!(fabs(dx[h]) > b.x)) & __builtin_amdgcn_ballot_w64(!(fabs(dy[h]) > b.y));
    }
    if ((pm[0] | pm[1]) == 0ull) continue;
    const double ay = a.y;                                           // (a copy: the bits of THIS element are compared)
    const bool disc = __builtin_amdgcn_ballot_w64(__builtin_bit_cast(unsigned long long, ay) == 0x8000000000000000ull) != 0ull;
    if (disc) {
      const double R = e.x + rho, R2 = R * R;
      bool noisy = false;                                            // (scalar) the disc is uncertain: its row's l00 is not zero
      if constexpr (NZ::on) {
        const double* const row = nz.rows + m * POCS_NOISE_STRIDE;
        const double l00 = row[0];
        noisy = __builtin_amdgcn_ballot_w64(l00 != 0.0) != 0ull;
        if (noisy) {
          const pocs_u32x4 wd = pocs_draw(nz.seed, nz.pair, nz.v, POCS_STREAM_DISC, (uint32_t)row[3]);
          const double l10 = row[1], l11 = row[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if (pm[h] == 0ull) continue;
            double z0, z1;
            pocs_normal_pair_w2(h ? wd.z : wd.x, h ? wd.w : wd.y, T, &z0, &z1, V);
            const double ex = fma(l00, z0, c.x) - x[h], ey = fma(l11, z1, fma(l10, z0, c.y)) - y[h];
            bt[h] = pm[h] & __builtin_amdgcn_ballot_w64(!(fma(ex, ex, ey * ey) > R2));
          }
        }
      }
      if (!noisy) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (pm[h] == 0ull) continue;
          bt[h] = pm[h] & __builtin_amdgcn_ballot_w64(!(fma(dx[h], dx[h], dy[h] * dy[h]) > R2));
        }
      }
      k0 |= bt[0]; k1 |= bt[1];
    } else {
      // an axis-aligned record (every lane reads the same one): the offset as it is
      const bool turned = (__builtin_amdgcn_ballot_w64(a.x != 1.0) | __builtin_amdgcn_ballot_w64(a.y != 0.0)) != 0ull;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (pm[h] == 0ull) continue;
        double e1 = dx[h], e2 = dy[h];
        if (turned) {
          e1 = fma(dx[h], a.x, dy[h] * a.y);
          e2 = fma(dy[h], a.x, -(dx[h] * a.y));
        }
        const double q1 = fmax(fabs(e1) - e.x, 0.0);
        const double q2 = fmax(fabs(e2) - e.y, 0.0);
        bt[h] = pm[h] & __builtin_amdgcn_ballot_w64(!(fma(q1, q1, q2 * q2) > rho2));
      }
    }
    m0 |= bt[0]; m1 |= bt[1];
  }
  mask[0] = m0; mask[1] = m1;
  if (kinds) { kinds[0] = k0; kinds[1] = k1; }
}
#endif

template <bool EAGER = false>
POCS_HD void pocs_pair_collides(const double x[2], const double y[2], const double th[2], const pocs_footprint* fp,
                                const double* obs, int M, const pocs_tables* T, const pocs_vconst* V, bool hit[2]) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned long long mask[2];
  pocs_pair_collides_masks<EAGER>(x, y, th, fp, obs, M, T, V, mask);
  hit[0] = __builtin_amdgcn_inverse_ballot_w64(mask[0]);
  hit[1] = __builtin_amdgcn_inverse_ballot_w64(mask[1]);
#else
  hit[0] = false; hit[1] = false;
  if (M <= 0) return;
  double sn[2], cs[2], px[2], py[2];
  for (int h = 0; h < 2; ++h) {
    pocs_sincos_tab(th[h], T, &sn[h], &cs[h], V);
    px[h] = x[h]; py[h] = y[h];
  }
  if (!(fp->dx == 0.0 && fp->dy == 0.0)) {
    for (int h = 0; h < 2; ++h) {
      px[h] = x[h] + fma(cs[h], fp->dx, -(sn[h] * fp->dy));
      py[h] = y[h] + fma(sn[h], fp->dx, cs[h] * fp->dy);
    }
  }
  for (int m = 0; m < M; ++m) {
    const double* o = obs + m * POCS_OBS_STRIDE;
    for (int h = 0; h < 2; ++h)
      if (pocs_box_hit(px[h], py[h], sn[h], cs[h], fp->hx, fp->hy, o)) hit[h] = true;
  }
#endif
}

// The two predicates above with every record's own answer kept (POCS_OPT_OBSTACLE_COUNTS: which box a collision comes
// from).  Per pose the same operations in the same order -- pocs_box_hit against record m, the flag set under the same
// condition -- and each answer handed to `each` before the next record is looked at: each(m, touched) for one pose,
// each(m, h, touched) for pose h of a pair, called by every lane that runs the loop, outside the test's own branches (a
// caller may ballot in it).  The flag is set exactly when some record's answer is.  The single-pose form is a function of
// its own: pocs_pose_collides stays, instruction for instruction, what it is.  On the device the pair's form is the one
// loop of pocs_pair_collides_masks with a callback: every lane's answer for record m comes from that record's lane mask.
template <class Each>
POCS_HD bool pocs_pose_collides_each(double x, double y, double th, const pocs_footprint* fp, const double* obs, int M,
                                     const pocs_tables* T, Each each, const pocs_vconst* V = nullptr) {
  if (M <= 0) return false;
  double sn, cs;
  pocs_sincos_tab(th, T, &sn, &cs, V);
  double px = x, py = y;
  if (!(fp->dx == 0.0 && fp->dy == 0.0)) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("; offset footprint");
#endif
    px = x + fma(cs, fp->dx, -(sn * fp->dy));
    py = y + fma(sn, fp->dx, cs * fp->dy);
  }
  bool hit = false;
  for (int m = 0; m < M; ++m) {
    const bool t = pocs_box_hit(px, py, sn, cs, fp->hx, fp->hy, obs + m * POCS_OBS_STRIDE);
    if (t) hit = true;
    each(m, t);
  }
  return hit;
}

template <bool EAGER = false, class Each>
POCS_HD void pocs_pair_collides_each(const double x[2], const double y[2], const double th[2], const pocs_footprint* fp,
                                     const double* obs, int M, const pocs_tables* T, const pocs_vconst* V, bool hit[2], Each each) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned long long mask[2];
  pocs_pair_collides_masks<EAGER>(x, y, th, fp, obs, M, T, V, mask, each);
  hit[0] = __builtin_amdgcn_inverse_ballot_w64(mask[0]);
  hit[1] = __builtin_amdgcn_inverse_ballot_w64(mask[1]);
#else
  hit[0] = false; hit[1] = false;
  if (M <= 0) return;
  double sn[2], cs[2], px[2], py[2];
  for (int h = 0; h < 2; ++h) {
    pocs_sincos_tab(th[h], T, &sn[h], &cs[h], V);
    px[h] = x[h]; py[h] = y[h];
  }
  if (!(fp->dx == 0.0 && fp->dy == 0.0)) {
    for (int h = 0; h < 2; ++h) {
      px[h] = x[h] + fma(cs[h], fp->dx, -(sn[h] * fp->dy));
      py[h] = y[h] + fma(sn[h], fp->dx, cs[h] * fp->dy);
    }
  }
  for (int m = 0; m < M; ++m) {
    const double* o = obs + m * POCS_OBS_STRIDE;
    for (int h = 0; h < 2; ++h) {
      const bool t = pocs_box_hit(px[h], py[h], sn[h], cs[h], fp->hx, fp->hy, o);
      if (t) hit[h] = true;
      each(m, h, t);
    }
  }
#endif
}

// The footprint's largest half-extent along world x over all headings in [lo, hi] (along world y: the
// same function of [lo - pi/2, hi - pi/2]): an upper bound, never more than the bounding radius.
//   f(t) = rx |cos t| + ry |sin t| is concave between the multiples of pi/2 and peaks with the bounding
//   radius at t = +-atan(ry / rx) + k pi: with no peak inside the range the maximum sits at an end.
// k_gmm_step's culling uses it to give the records it keeps a broad phase that fits the task's headings
// (gmm_cull); tests/test_product_host_vs_oracle.py scans f densely against it.
//   rr = the bounding radius sqrt(rx^2 + ry^2), phi = atan2(ry, rx): constants of the footprint, computed once on the
//   host for the kernels (every block of every launch culls: a square root, an arc tangent and four divisions less
//   in each of them)
// (in three steps, so that a wave can evaluate the end values of several ranges side by side, one per lane: gmm_cull)
//   is the bounding radius the answer without looking at the ends (a range of pi or more, a peak inside it)?
POCS_HD bool pocs_footprint_extent_is_radius(double phi, double lo, double hi) {
  const double PI = 3.14159265358979323846, INV_PI = 0.318309886183790671538;
  if (!(hi - lo < PI)) return true;
  for (int sgn = -1; sgn <= 1; sgn += 2) {
    const double s = sgn * phi;
    if (ceil((lo - s) * INV_PI) <= floor((hi - s) * INV_PI)) return true;   // a peak inside the range
  }
  return false;
}
//   f at one end of a range
POCS_HD double pocs_footprint_extent_end(double rx, double ry, double t) {
  double sn, cs;
  pocs_sincos(t, &sn, &cs);
  return fma(rx, fabs(cs), ry * fabs(sn));
}
//   the bound from the two end values
POCS_HD double pocs_footprint_extent_of_ends(double rr, double fa, double fb) {
  return fmin(rr, fmax(fa, fb) * (1.0 + 1e-9) + 1e-12);
}
POCS_HD double pocs_footprint_extent_pre(double rx, double ry, double rr, double phi, double lo, double hi) {
  if (pocs_footprint_extent_is_radius(phi, lo, hi)) return rr;
  const double fa = pocs_footprint_extent_end(rx, ry, lo);
  const double fb = pocs_footprint_extent_end(rx, ry, hi);
  return pocs_footprint_extent_of_ends(rr, fa, fb);
}
POCS_HD double pocs_footprint_extent(double rx, double ry, double lo, double hi) {
  return pocs_footprint_extent_pre(rx, ry, sqrt(rx * rx + ry * ry), atan2(ry, rx), lo, hi);
}

// ---- clearance levels (pocs_set_clearance_levels) -------------------------------------------------------------------
// For clearances d_0 < d_1 < ... < d_{L-1} a pose is WITHIN clearance d of the world exactly when the collision test above
// answers "touches" for the footprint grown by d -- {dx, dy, hx + d, hy + d}, one addition per half extent -- touching
// included.  Every margin of the narrow phase is a monotone function of the half extents, so a pose within d is within every
// larger d: the largest level is tested first and a smaller one only for a pose that touched.  The records are those prepared
// (pocs_prepare_obstacle) for the footprint grown by d_{L-1}: fields 0 .. 5 do not depend on the footprint, and a broad phase
// sized for the largest level is conservative for the smaller ones.  The functions above stay what they are.
#define POCS_MAX_CLEARANCE_LEVELS 4

POCS_HD pocs_footprint pocs_grown_footprint(const pocs_footprint* fp, double d) {
  pocs_footprint g = {fp->dx, fp->dy, fp->hx + d, fp->hy + d};
  return g;
}

// The smallest level l with the pose within clearance d[l]; L: within none.  (The footprint itself is not looked at: a caller
// that wants to know whether the pose collides asks pocs_pose_collides with the records of the footprint as it is.)
POCS_HD int pocs_pose_clearance_level(double x, double y, double th, const pocs_footprint* fp, const double* d, int L,
                                      const double* obs, int M, const pocs_tables* T, const pocs_vconst* V = nullptr) {
  int level = L;
  for (int l = L - 1; l >= 0; --l) {
    const pocs_footprint g = pocs_grown_footprint(fp, d[l]);
    if (!pocs_pose_collides(x, y, th, &g, obs, M, T, V)) break;
    level = l;
  }
  return level;
}

#if defined(__HIPCC__)
// The same for the pair of poses a thread of k_gmm_step draws, as lane masks per level in the manner of
// pocs_pair_collides_masks: each(l, m0, m1) is called once per level, from L - 1 down to 0, with the lanes whose pose 0 / pose 1
// is within d[l].  A level below one that no lane of either pose touched is not computed (both masks zero), and a lane counts
// for a level only if it counted for the one above: per lane the answer of pocs_pose_clearance_level, whatever the other lanes
// of its wave hold.  `obs` and `d` lie in LDS (the kept records of the grown footprint, the distances).
template <class Each>
__device__ __forceinline__ void pocs_pair_clearance_masks(const double x[2], const double y[2], const double th[2], const pocs_footprint* fp,
                                                          const double* d, int L, const double* obs, int M, const pocs_tables* T,
                                                          const pocs_vconst* V, Each each) {
  unsigned long long up0 = ~0ull, up1 = ~0ull;
#pragma unroll 1
  for (int l = L - 1; l >= 0; --l) {
    unsigned long long m[2] = {0ull, 0ull};
    if ((up0 | up1) != 0ull) {                                      // (scalar)
      const pocs_footprint g = pocs_grown_footprint(fp, d[l]);
      pocs_pair_collides_masks<false>(x, y, th, &g, obs, M, T, V, m);
      m[0] &= up0; m[1] &= up1;
    }
    each(l, m[0], m[1]);
    up0 = m[0]; up1 = m[1];
  }
}
#endif

// ---- compound footprints (pocs_set_footprint_parts) ------------------------------------------------------------------
// A compound footprint is F parts, each {dx, dy, hx, hy} exactly a pocs_footprint: an offset in the base frame and half
// extents, no yaw of its own.  A pose touches a world exactly when pocs_pose_collides answers "touches" for at least one
// part taken alone as the footprint: per part the same operations in the same order, the flag the OR of the parts' flags.
// A part as the kernels hold it is POCS_PART_STRIDE doubles: dx dy hx hy, then its bounding radius sqrt(hx^2 + hy^2) and
// corner angle atan2(hy, hx) (pocs_footprint_extent_pre), which only the GMM cull reads.  The records are those prepared
// (pocs_prepare_obstacle) for the part with the largest bounding radius: fields 0 .. 5 do not depend on the footprint, and
// a broad phase sized for the largest part is conservative for the others.  The functions above stay what they are.
#define POCS_MAX_FOOTPRINT_PARTS 4
#define POCS_PART_STRIDE 6

// Which of the parts (each a pocs_footprint) has the largest bounding radius: the one the records are prepared for.
POCS_HD int pocs_parts_cover(const pocs_footprint* parts, int F) {
  int best = 0;
  double rbest = -1.0;
  for (int f = 0; f < F; ++f) {
    const double rr = sqrt(parts[f].hx * parts[f].hx + parts[f].hy * parts[f].hy);
    if (rr > rbest) { rbest = rr; best = f; }
  }
  return best;
}
POCS_HD void pocs_prepare_part(const pocs_footprint* fp, double* rec) {
  rec[0] = fp->dx; rec[1] = fp->dy; rec[2] = fp->hx; rec[3] = fp->hy;
  rec[4] = sqrt(fp->hx * fp->hx + fp->hy * fp->hy);
  rec[5] = atan2(fp->hy, fp->hx);
}

// One pose: bit f of the answer is set when part f touches some record.  The heading's sine and cosine once per pose;
// (px, py) per part as pocs_pose_collides forms it, pocs_box_hit per part and record as there.
POCS_HD unsigned pocs_pose_parts_touched(double x, double y, double th, const double* parts, int F,
                                         const double* obs, int M, const pocs_tables* T, const pocs_vconst* V = nullptr) {
  if (M <= 0) return 0u;
  double sn, cs;
  pocs_sincos_tab(th, T, &sn, &cs, V);
  unsigned touched = 0u;
  for (int f = 0; f < F; ++f) {
    const double* q = parts + f * POCS_PART_STRIDE;
    const double dx = q[0], dy = q[1], rx = q[2], ry = q[3];
    double px = x, py = y;
    if (!(dx == 0.0 && dy == 0.0)) {
      px = x + fma(cs, dx, -(sn * dy));
      py = y + fma(sn, dx, cs * dy);
    }
    bool hit = false;
    for (int m = 0; m < M; ++m)
      if (pocs_box_hit(px, py, sn, cs, rx, ry, obs + m * POCS_OBS_STRIDE)) hit = true;
    if (hit) touched |= 1u << f;
  }
  return touched;
}
POCS_HD bool pocs_pose_collides_parts(double x, double y, double th, const double* parts, int F,
                                      const double* obs, int M, const pocs_tables* T, const pocs_vconst* V = nullptr) {
  return pocs_pose_parts_touched(x, y, th, parts, F, obs, M, T, V) != 0u;
}

#if defined(__HIPCC__)
// The same for the pair of poses a thread of k_gmm_step draws, as lane masks in the manner of pocs_pair_collides_masks:
// mask[h] bit l = lane l's pose h touches with some part; each(f, m0, m1) is called once per part with the part's own two
// masks.  The two headings' sines and cosines are computed once per call; per part the loop of pocs_pair_loop over the
// records -- one fetch per record for both poses, the narrow phase behind wave-uniform branches, every answer balloted.
// `parts` and `obs` lie in LDS.  F and M are wave-uniform.
struct pocs_each_part_none { __device__ __forceinline__ void operator()(int, unsigned long long, unsigned long long) const {} };

template <class Each = pocs_each_part_none>
__device__ __forceinline__ void pocs_pair_parts_masks(const double x[2], const double y[2], const double th[2], const double* parts, int F,
                                                      const double* obs, int M, const pocs_tables* T, const pocs_vconst* V,
                                                      unsigned long long mask[2], Each each = Each()) {
  unsigned long long all0 = 0ull, all1 = 0ull;
  double sn[2] = {0.0, 0.0}, cs[2] = {1.0, 1.0};
  if (M > 0) {                                                       // (scalar)
#pragma unroll
    for (int h = 0; h < 2; ++h) pocs_sincos_tab(th[h], T, &sn[h], &cs[h], V);
  }
#pragma unroll 1
  for (int f = 0; f < F; ++f) {
    unsigned long long m0 = 0ull, m1 = 0ull;
    if (M > 0) {
      const double* q = parts + f * POCS_PART_STRIDE;
      const double fdx = q[0], fdy = q[1], rx = q[2], ry = q[3];
      const bool offset = __builtin_amdgcn_ballot_w64(!(fdx == 0.0 && fdy == 0.0)) != 0ull;      // (scalar: every lane reads the same part)
      double px[2], py[2], ex[2], ey[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        px[h] = x[h]; py[h] = y[h];
        if (offset) {
          px[h] = x[h] + fma(cs[h], fdx, -(sn[h] * fdy));
          py[h] = y[h] + fma(sn[h], fdx, cs[h] * fdy);
        }
        ex[h] = fma(rx, fabs(cs[h]), ry * fabs(sn[h]));
        ey[h] = fma(rx, fabs(sn[h]), ry * fabs(cs[h]));
      }
      const __attribute__((address_space(3))) pocs_v2d* o = (const __attribute__((address_space(3))) pocs_v2d*)obs;
      asm volatile("" : "+v"(o));
      for (int m = 0; m < M; ++m, o += POCS_OBS_STRIDE / 2) {
        const pocs_v2d c = o[0], b = o[3], a = o[1], e = o[2];       // (cx, cy) (bx, by) | (ax, ay) (hx, hy)
        double dx[2], dy[2];
        unsigned long long pm[2], bt[2] = {0ull, 0ull};
#pragma unroll
        for (int h = 0; h < 2; ++h) {                                // pocs_box_hit's broad phase
          dx[h] = c.x - px[h];
          dy[h] = c.y - py[h];
          pm[h] = __builtin_amdgcn_ballot_w64(!(fabs(dx[h]) > b.x)) & __builtin_amdgcn_ballot_w64(!(fabs(dy[h]) > b.y));
        }
        if ((pm[0] | pm[1]) != 0ull) {                               // pocs_box_narrow for the lanes inside the box
          const bool turned = (__builtin_amdgcn_ballot_w64(a.x != 1.0) | __builtin_amdgcn_ballot_w64(a.y != 0.0)) != 0ull;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if (pm[h] == 0ull) continue;
            if (!turned)
              bt[h] = pocs_box_margins_mask(pm[h], dx[h], dy[h], sn[h], cs[h], rx, ry, e.x, e.y, cs[h], sn[h], dx[h], dy[h], ex[h], ey[h]);
            else {
              const double cr = fma(cs[h], a.x, sn[h] * a.y), sr = fma(sn[h], a.x, -(cs[h] * a.y));      // the relative yaw
              bt[h] = pocs_box_margins_mask(pm[h], dx[h], dy[h], sn[h], cs[h], rx, ry, e.x, e.y, cr, sr,
                                            fma(dx[h], a.x, dy[h] * a.y), fma(dy[h], a.x, -(dx[h] * a.y)),
                                            fma(rx, fabs(cr), ry * fabs(sr)), fma(rx, fabs(sr), ry * fabs(cr)));
            }
          }
          m0 |= bt[0]; m1 |= bt[1];
        }
      }
    }
    each(f, m0, m1);
    all0 |= m0; all1 |= m1;
  }
  mask[0] = all0; mask[1] = all1;
}
#endif

// ---- watched regions (pocs_set_regions) -----------------------------------------------------------------------------
// A region is a box of the obstacle layout that truncates nothing: a call counts the surviving poses that are in it.  A pose
// is IN region g exactly when pocs_pose_collides answers "touches" against the one-box table holding the region, for the
// region's own footprint -- the robot's (POCS_REGION_TOUCH) or the point {0, 0, 0, 0} (POCS_REGION_POINT: the pose's
// reference point lies in the box or on its boundary).  Record g (POCS_OBS_STRIDE doubles) is prepared by
// pocs_prepare_obstacle for footprint g (four doubles: dx dy hx hy).  The same operations in the same order as
// pocs_pose_collides, touching included; the functions above stay what they are.
#define POCS_MAX_REGIONS 4
#define POCS_REGION_TOUCH 0
#define POCS_REGION_POINT 1

// One pose: bit g of the answer = the pose is in region g.  The heading's sine and cosine are formed once.
POCS_HD unsigned pocs_pose_regions_mask(double x, double y, double th, const double* rec, const double* fps, int G,
                                        const pocs_tables* T, const pocs_vconst* V = nullptr) {
  if (G <= 0) return 0u;
  double sn, cs;
  pocs_sincos_tab(th, T, &sn, &cs, V);
  unsigned in = 0u;
  for (int g = 0; g < G; ++g) {
    const double* f = fps + 4 * g;
    double px = x, py = y;
    if (!(f[0] == 0.0 && f[1] == 0.0)) {          // (pocs_pose_collides: a centred footprint skips x + (c*0 - s*0) == x)
      px = x + fma(cs, f[0], -(sn * f[1]));
      py = y + fma(sn, f[0], cs * f[1]);
    }
    if (pocs_box_hit(px, py, sn, cs, f[2], f[3], rec + g * POCS_OBS_STRIDE)) in |= 1u << g;
  }
  return in;
}

#if defined(__HIPCC__)
// The same for the pair of poses a sampling thread holds, as lane masks per region: each(g, m0, m1) is called once per region
// of `keep` with the lanes whose pose 0 / pose 1 is in it.  Per region the one-record loop of pocs_pair_collides_masks with the region's
// footprint: every branch is wave-uniform, and a region whose broad phase no lane of either pose passes costs two ballots.
// `rec` and `fps` lie in LDS; a footprint's four values are the same in every lane and are moved to scalar registers, so
// that the centred / offset choice of pocs_pair_collides_masks stays a scalar branch.
__device__ __forceinline__ double pocs_wave_uniform_f64(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | (unsigned long long)lo);
}
template <class Each>
__device__ __forceinline__ void pocs_pair_regions_masks(const double x[2], const double y[2], const double th[2], const double* rec,
                                                        const double* fps, int G, unsigned keep, const pocs_tables* T, const pocs_vconst* V,
                                                        Each each) {
  // keep (wave-uniform): bit g clear = the caller knows that no pose of the wave can be in region g; it is not looked at
#pragma unroll 1
  for (int g = 0; g < G; ++g) {
    if (((keep >> g) & 1u) == 0u) continue;
    const pocs_footprint f = {pocs_wave_uniform_f64(fps[4 * g]), pocs_wave_uniform_f64(fps[4 * g + 1]),
                              pocs_wave_uniform_f64(fps[4 * g + 2]), pocs_wave_uniform_f64(fps[4 * g + 3])};
    unsigned long long m[2];
    pocs_pair_collides_masks<false>(x, y, th, &f, rec + g * POCS_OBS_STRIDE, 1, T, V, m);
    each(g, m[0], m[1]);
  }
}
#endif

// ---- segment checks (pocs_set_segment_checks) ------------------------------------------------------------------------
// With J >= 2 checks per segment a pose also "touches" at a waypoint when one of J - 1 sub-poses on the way into that waypoint
// touches.  The sub-poses are outputs of pocs_motion (pocs_model.h) as it is, on a control whose third entry is 0.0:
//   q_j = pocs_motion(p, {a0, d_j, 0.0}),  1 <= j <= J - 1,
//   forwards  (MC, from the particle at the segment's start, the step's noisy control u):   a0 = u[0],  d_j = f_j * u[1];
//   backwards (GMM, from the sample at the segment's end, the step's applied control u):    a0 = -u[2], d_j = -(f_{J-j} * u[1]);
//   f_j = (double)j / (double)J, one IEEE division (pocs_segment_fractions: formed once on the host, read by the kernels).
// The J - 1 sub-poses of a pose share one heading: one sine and cosine of the drive direction p.theta + a0 (pocs_sincos, as
// pocs_motion forms them -- the MC step holds them already), one of the wrapped heading as the collision test evaluates it
// (pocs_sincos_tab), and the rotated footprint offset once; only the centre moves, along a line.  Per sub-pose and record the
// operations of pocs_pose_collides in its order (pocs_box_hit): the flags are those of pocs_pose_collides(q_j).
//   The broad phase over the whole segment (single-pose form): fma(d, cs, x) is a monotone function of d, and so is the sum
//   with the offset and the difference to a record's centre, each being one rounded monotone operation; every d_j lies between
//   0 and d_end = +-u[1] (f < 1, a rounded product never passes its factor).  So per axis every sub-pose's offset to a record
//   lies between the offsets of the two ends d = 0 and d = d_end, and a record whose broad-phase box neither end's interval
//   reaches is failed by pocs_box_hit's broad phase for every sub-pose: it is skipped for all of them.  Exact, no margin.
#define POCS_MAX_SEGMENT_CHECKS 8

POCS_HD void pocs_segment_fractions(int J, double* f) {            // f[j] = j / J for j < J, 0 behind (f[0] = 0)
  for (int j = 0; j < POCS_MAX_SEGMENT_CHECKS; ++j) f[j] = j < J ? (double)j / (double)J : 0.0;
}
// the drive of sub-pose j
POCS_HD double pocs_segment_drive(const double* f, int J, int j, int backward, double u1) {
  return backward ? -(f[J - j] * u1) : f[j] * u1;
}

// One pose: bit j (1 <= j <= J - 1) of the answer is set when sub-pose j touches some record.  hd = p.theta + a0, the drive
// direction as pocs_motion forms it, (sn, cs) its sine and cosine by pocs_sincos.
POCS_HD unsigned pocs_segment_touched_dir(double x, double y, double hd, double sn, double cs, double u1, const double* f, int J, int backward,
                                          const pocs_footprint* fp, const double* obs, int M, const pocs_tables* T,
                                          const pocs_vconst* V = nullptr) {
  if (M <= 0 || J < 2) return 0u;
  const double qt = pocs_wrap_angle(hd + 0.0);                     // pocs_motion: x[2] + u[0] + u[2] with u[2] = 0.0
  double sh, ch;
  pocs_sincos_tab(qt, T, &sh, &ch, V);
  const bool offset = !(fp->dx == 0.0 && fp->dy == 0.0);
  double ox = 0.0, oy = 0.0;
  if (offset) {
    ox = fma(ch, fp->dx, -(sh * fp->dy));
    oy = fma(sh, fp->dx, ch * fp->dy);
  }
  // the two ends of the line the footprint's centre moves on
  const double dend = backward ? -u1 : u1;
  double ax = x, ay = y, bx = fma(dend, cs, x), by = fma(dend, sn, y);
  if (offset) { ax = x + ox; ay = y + oy; bx = bx + ox; by = by + oy; }
  const double xlo = fmin(ax, bx), xhi = fmax(ax, bx), ylo = fmin(ay, by), yhi = fmax(ay, by);
  static_assert(POCS_MAX_OBSTACLES <= 64, "the records in the segment's reach are a 64-bit mask");
  unsigned long long cand = 0ull;
  for (int m = 0; m < M; ++m) {
    const double* o = obs + m * POCS_OBS_STRIDE;
    // o[0] - px over px in [xlo, xhi] lies in [o[0] - xhi, o[0] - xlo]: all |.| > o[6] exactly when the interval misses [-o[6], o[6]]
    if (o[0] - xhi > o[6] || o[0] - xlo < -o[6] || o[1] - yhi > o[7] || o[1] - ylo < -o[7]) continue;
    cand |= 1ull << m;
  }
  if (cand == 0ull) return 0u;
  unsigned touched = 0u;
  for (int j = 1; j < J; ++j) {
    const double d = pocs_segment_drive(f, J, j, backward, u1);
    const double qx = fma(d, cs, x), qy = fma(d, sn, y);
    double px = qx, py = qy;
    if (offset) { px = qx + ox; py = qy + oy; }
    bool hit = false;
    for (unsigned long long b = cand; b != 0ull; b &= b - 1ull) {
      const int m = __builtin_ctzll(b);
      if (pocs_box_hit(px, py, sh, ch, fp->hx, fp->hy, obs + m * POCS_OBS_STRIDE)) hit = true;
    }
    if (hit) touched |= 1u << j;
  }
  return touched;
}
// ... with the drive direction's sine and cosine formed here (the GMM form's way in, the probe, the host harness)
POCS_HD unsigned pocs_segment_touched(double x, double y, double th, double a0, double u1, const double* f, int J, int backward,
                                      const pocs_footprint* fp, const double* obs, int M, const pocs_tables* T,
                                      const pocs_vconst* V = nullptr) {
  if (M <= 0 || J < 2) return 0u;
  double sn, cs;
  pocs_sincos(th + a0, &sn, &cs);
  return pocs_segment_touched_dir(x, y, th + a0, sn, cs, u1, f, J, backward, fp, obs, M, T, V);
}

#if defined(__HIPCC__)
// The same for the pair of poses a sampling thread holds, as lane masks in the manner of pocs_pair_parts_masks: mask[h] bit l =
// some sub-pose of lane l's pose h touches; each(j, m0, m1) is called once per sub-pose with its own two masks.  The two drive
// directions' and wrapped headings' sines and cosines and the rotated offsets once per call; per sub-pose the record loop of
// pocs_pair_parts_masks -- one fetch per record for both poses, the narrow phase behind wave-uniform branches, every answer
// balloted.  `obs` lies in LDS (the caller's kept list, culled for the whole segment); f, J, backward, a0, u1 and M are
// wave-uniform.
struct pocs_each_sub_none { __device__ __forceinline__ void operator()(int, unsigned long long, unsigned long long) const {} };

template <class Each = pocs_each_sub_none>
__device__ __forceinline__ void pocs_pair_segment_masks(const double x[2], const double y[2], const double th[2], double a0, double u1,
                                                        const double* f, int J, int backward, const pocs_footprint* fp,
                                                        const double* obs, int M, const pocs_tables* T, const pocs_vconst* V,
                                                        unsigned long long mask[2], Each each = Each()) {
  unsigned long long all0 = 0ull, all1 = 0ull;
  const double rx = fp->hx, ry = fp->hy;
  double sn[2] = {0.0, 0.0}, cs[2] = {1.0, 1.0}, sh[2] = {0.0, 0.0}, ch[2] = {1.0, 1.0}, ox[2] = {0.0, 0.0}, oy[2] = {0.0, 0.0}, ex[2], ey[2];
  const bool offset = __builtin_amdgcn_ballot_w64(!(fp->dx == 0.0 && fp->dy == 0.0)) != 0ull;      // (scalar: every lane reads the same footprint)
  if (M > 0) {                                                       // (scalar)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const double hd = th[h] + a0;
      pocs_sincos(hd, &sn[h], &cs[h]);
      pocs_sincos_tab(pocs_wrap_angle(hd + 0.0), T, &sh[h], &ch[h], V);
      if (offset) {
        ox[h] = fma(ch[h], fp->dx, -(sh[h] * fp->dy));
        oy[h] = fma(sh[h], fp->dx, ch[h] * fp->dy);
      }
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    ex[h] = fma(rx, fabs(ch[h]), ry * fabs(sh[h]));
    ey[h] = fma(rx, fabs(sh[h]), ry * fabs(ch[h]));
  }
#pragma unroll 1
  for (int j = 1; j < J; ++j) {
    unsigned long long m0 = 0ull, m1 = 0ull;
    if (M > 0) {
      const double d = pocs_segment_drive(f, J, j, backward, u1);
      double px[2], py[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        px[h] = fma(d, cs[h], x[h]); py[h] = fma(d, sn[h], y[h]);
        if (offset) { px[h] = px[h] + ox[h]; py[h] = py[h] + oy[h]; }
      }
      const __attribute__((address_space(3))) pocs_v2d* o = (const __attribute__((address_space(3))) pocs_v2d*)obs;
      asm volatile("" : "+v"(o));
      for (int m = 0; m < M; ++m, o += POCS_OBS_STRIDE / 2) {
        const pocs_v2d c = o[0], b = o[3], a = o[1], e = o[2];       // (cx, cy) (bx, by) | (ax, ay) (hx, hy)
        double dx[2], dy[2];
        unsigned long long pm[2], bt[2] = {0ull, 0ull};
#pragma unroll
        for (int h = 0; h < 2; ++h) {                                // pocs_box_hit's broad phase
          dx[h] = c.x - px[h];
          dy[h] = c.y - py[h];
          pm[h] = __builtin_amdgcn_ballot_w64(!(fabs(dx[h]) > b.x)) & __builtin_amdgcn_ballot_w64(!(fabs(dy[h]) > b.y));
        }
        if ((pm[0] | pm[1]) != 0ull) {                               // pocs_box_narrow for the lanes inside the box
          const bool turned = (__builtin_amdgcn_ballot_w64(a.x != 1.0) | __builtin_amdgcn_ballot_w64(a.y != 0.0)) != 0ull;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            if (pm[h] == 0ull) continue;
            if (!turned)
              bt[h] = pocs_box_margins_mask(pm[h], dx[h], dy[h], sh[h], ch[h], rx, ry, e.x, e.y, ch[h], sh[h], dx[h], dy[h], ex[h], ey[h]);
            else {
              const double cr = fma(ch[h], a.x, sh[h] * a.y), sr = fma(sh[h], a.x, -(ch[h] * a.y));      // the relative yaw
              bt[h] = pocs_box_margins_mask(pm[h], dx[h], dy[h], sh[h], ch[h], rx, ry, e.x, e.y, cr, sr,
                                            fma(dx[h], a.x, dy[h] * a.y), fma(dy[h], a.x, -(dx[h] * a.y)),
                                            fma(rx, fabs(cr), ry * fabs(sr)), fma(rx, fabs(sr), ry * fabs(cr)));
            }
          }
          m0 |= bt[0]; m1 |= bt[1];
        }
      }
    }
    each(j, m0, m1);
    all0 |= m0; all1 |= m1;
  }
  mask[0] = all0; mask[1] = all1;
}
#endif

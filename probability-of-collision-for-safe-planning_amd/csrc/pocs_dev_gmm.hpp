// pocs_dev_gmm.hpp -- the GMM sampling step, a part of pocs_kernels.hip (the only unit with device code; included there,
// inside its anonymous namespace).  Relies on pocs_dev_prims.hpp and, for its closers, on pocs_dev_advance.hpp.
//
//   k_gmm_step      S1+C1+T1  one waypoint of truncateGMM (MCSimulator.h:570-642) in ONE launch, for
//                             every run of a batch of independent estimations: the launch's units
//                             (run, virtual slice) dealt evenly to the blocks.  A block:
//                             head  log/sector tables, obstacle table and this waypoint's sampler
//                                   parameters -> LDS; exact culling of the obstacle table against
//                                   the mixture's bounding box, the kept records' broad phase
//                                   tightened to the run's range of headings;
//                             body  GM_Model::sampleNPoints (GM_Model.h:83-116) + checkMatrixCollisions
//                                   (:241-253) + the moment sums (:592-611), fused, one PAIR of
//                                   samples per thread-iteration: a sample is born, tested and folded
//                                   into its component's (n, sum x, sum x x^T) in registers; pose
//                                   and flag are streamed out once (24 B + 2 B).  A wave whose 128
//                                   samples lie in one component block (nearly always) runs the
//                                   iteration's scalar-component form in an inner loop of its own;
//                                   at the end of every virtual slice the wave's lane chains become a
//                                   wave sum in LDS (transposition, no barrier);
//                             tail  wave sums -> write-through rows per (run, virtual slice) -> ticket ->
//                                   the last block of a run to arrive adds the run's rows in a fixed
//                                   order and advances the mixture to the next waypoint: truncated
//                                   mean/cov, weights (:597-629), per-component EKF predict/update
//                                   (:766-771, :804-812), Cholesky -- on one GPU right away, sharded
//                                   after it has exchanged the run's moments with the other ranks (IPC
//                                   slots, one hop over xGMI) in the same tail.
//                             The waypoint loop never returns to the host.  (k_gmm_step_risk, k_gmm_step_tree: the same block
//                             under a risk bound / for one level of a tree of plans; k_gmm_close: the lone form's last rows;
//                             k_gmm_step_boxes, k_gmm_step_risk_boxes, k_gmm_step_tree_boxes: the counting forms of the three, which
//                             also count per obstacle box the samples that touch it, POCS_OPT_OBSTACLE_COUNTS; k_gmm_step_world,
//                             k_gmm_step_risk_world: the forms under a large collision world, pocs_set_world, whose heads fetch the
//                             records that k_world_cull -- one launch in front of each of theirs -- has left for their runs.)

// LDS of k_gmm_step.  A block works through a contiguous range of the launch's UNITS -- (run, virtual slice)
// pairs, pocs_kernels.h -- that may cross from one run into the next: everything per run is held twice.
//   tr     the wave's transpose scratch of flush_unit (5 rows of 64 lane values, pitch 66); before the first
//          flush the same bytes hold the full obstacle table the culling reads, after the last one the
//          closer's staging rows (gmm_close_sums)
//   slot   wave sums (survivors, nine sums) of the unit's FIRST component, per virtual slice held and wave;
//          once the rows are out, the mixture advance's scratch
//   xtra   ... of a component that STARTS inside the unit (a wave meets the start of a component once per run)
//   occ / oci  (the counting form only, POCS_OPT_OBSTACLE_COUNTS: an empty base otherwise, the layout below as it is) per run
//          buffer and KEPT record: the block's samples that touch it, and the record's index in the caller's table (gmm_cull
//          compacts): 1 KB
template <bool OC> struct gmm_oc_smem {};
template <> struct gmm_oc_smem<true> {
  unsigned occ[2][POCS_MAX_OBSTACLES];
  int oci[2][POCS_MAX_OBSTACLES];
};
//   keep2 / clh / clc  (the clearance form only, pocs_set_clearance_levels: an empty base otherwise again) per run buffer the obstacle
//          table culled against the footprint grown by the largest clearance (8 KB), the head of the waypoint's pocs_clear_dev
//          (grown footprint, its radius and corner angle, the distances) and per run buffer and level the block's samples within it
template <bool CL> struct gmm_cl_smem {};
template <> struct gmm_cl_smem<true> {
  alignas(16) double keep2[2][POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];
  double clh[6 + POCS_MAX_CLEARANCE_LEVELS];
  unsigned clc[2][POCS_MAX_CLEARANCE_LEVELS];
  int nkeep2[2];
};
static_assert(offsetof(pocs_clear_dev, fp_rr) == 32 && offsetof(pocs_clear_dev, d) == 48 && offsetof(pocs_clear_dev, obs) == 48 + 8 * POCS_MAX_CLEARANCE_LEVELS,
              "clh: the record's first doubles are footprint (4), radius, corner angle, distances");
//   fpp    (the parts form only, pocs_set_footprint_parts: an empty base otherwise again) the parts of the compound footprint, 192 B
template <bool FPN> struct gmm_fp_smem {};
template <> struct gmm_fp_smem<true> {
  double fpp[POCS_MAX_FOOTPRINT_PARTS * POCS_PART_STRIDE];
};
//   rgh / rgk / rgc  (the regions form only, pocs_set_regions: an empty base otherwise again) the regions' records and footprints
//          (pocs_regions_dev's head, 384 B), per run buffer the regions the run's mixture can reach (a bit each) and per run buffer and
//          region the block's collision-free samples in it: 432 B, so K = 8 holds 75 856 B against the twin's 75 424
template <bool RG> struct gmm_rg_smem {};
template <> struct gmm_rg_smem<true> {
  alignas(16) double rgh[POCS_REGIONS_HEAD];
  unsigned rgc[2][POCS_MAX_REGIONS];
  unsigned rgk[2];
};
//   keeps / sgf / sgu / sgc  (the segment form only, pocs_set_segment_checks: an empty base otherwise again) per run buffer the obstacle
//          table culled for the run's whole way in (8 KB), the fractions f_j, the run's applied control of step w - 1, the block's
//          samples whose own pose is free and some sub-pose touches, and J
template <bool SG> struct gmm_sg_smem {};
template <> struct gmm_sg_smem<true> {
  alignas(16) double keeps[2][POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];
  double sgf[2][POCS_MAX_SEGMENT_CHECKS];
  double sgu[2][4];
  unsigned sgc[2];
  int nkeeps[2];
  int sgJ[2];
};
//   (the noise form only, pocs_set_disc_covariances: LDS of its own beside gmm_smem, whose type and layout stay) per run buffer and KEPT
//          record its row {l00, l10, l11, disc index} of the noise table, in the kept list's order: 4 KB
//   (the hypotheses form, pocs_set_disc_hypotheses, on top of it: behind the two buffers' rows, per run buffer and KEPT record its gate
//          {lo, hi - 1, g, on}, four 32-bit words, in the kept list's order: 2 KB more -- gmm_gates finds them)
template <bool RN, bool RH = false> struct gmm_noise_rows { static __device__ __forceinline__ double* get() { return nullptr; } };
template <> struct gmm_noise_rows<true, false> {
  static __device__ __forceinline__ double* get() {
    __shared__ alignas(16) double rows[2 * POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE];
    return rows;
  }
};
template <> struct gmm_noise_rows<true, true> {
  static __device__ __forceinline__ double* get() {
    __shared__ alignas(16) double rows[2 * POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE + 2 * POCS_MAX_OBSTACLES * POCS_GATE_STRIDE / 2];
    return rows;
  }
};
__device__ __forceinline__ uint32_t* gmm_gates(double* nz, const int rb) {
  return reinterpret_cast<uint32_t*>(nz + 2 * POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE) + rb * (POCS_MAX_OBSTACLES * POCS_GATE_STRIDE);
}
template <int K, int TB, bool OC = false, bool CL = false, bool FPN = false, bool RG = false, bool SG = false>
struct gmm_smem : gmm_oc_smem<OC>, gmm_cl_smem<CL>, gmm_fp_smem<FPN>, gmm_rg_smem<RG>, gmm_sg_smem<SG> {
  static constexpr int NC = K * POCS_NMOM;
  static constexpr int NW = TB / 64;
  // (the clearance form holds 24 units at a time, not 32: with its second kept table K = 7 and K = 8 would otherwise pass the 80 KB
  // that let two blocks share a CU's 160 KB; the sums are defined per unit, so how many a block holds at a time changes no bit)
  static constexpr int SUB = (CL || SG) ? 24 : POCS_GMM_SUB;      // (the segment form's second kept table: as the clearance form)
  alignas(16) pocs_tables tab;                                       // 12 KB log / sector tables, staged once per block
  alignas(16) double keep[2][POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];  // obstacle table culled for the block's (up to) two runs
  alignas(16) double par[2][K * POCS_PARAM_STRIDE];                  // sampler parameters of (run, waypoint)
  alignas(16) double tr[NW][POCS_FLUSH_ROWS][POCS_FLUSH_PITCH];
  alignas(16) double slot[SUB][NW][POCS_UNIT_SUMS];
  double xtra[2][NW][K][POCS_UNIT_SUMS];
  int kf[SUB][NW];                                                   // the component slot[..] belongs to
  int xj[2][NW][K];                                                  // the held virtual slice xtra[..] belongs to (-1: none)
  unsigned long long seed[2];                                        // the two runs' seeds
  int nkeep[2];
  int last[2];                                                       // this block drew the last ticket of its run 0 / 1
  static_assert(sizeof(double) * NW * POCS_FLUSH_ROWS * POCS_FLUSH_PITCH >= sizeof(double) * POCS_MAX_OBSTACLES * POCS_OBS_STRIDE,
                "the obstacle table is staged in the transpose scratch");
  static_assert(NW * POCS_FLUSH_ROWS * POCS_FLUSH_PITCH >= 16 * NC, "the closer's staging rows live in the transpose scratch");
  static_assert(SUB * NW * POCS_UNIT_SUMS >= POCS_ADV_SCRATCH(K) + POCS_SPEC_SCRATCH(K), "the advance's scratch lives in the slots");
  __device__ __forceinline__ double* obs() { return &tr[0][0][0]; }
  static_assert(!CL || NW * POCS_FLUSH_ROWS * POCS_FLUSH_PITCH >= 2 * POCS_MAX_OBSTACLES * POCS_OBS_STRIDE, "... and the grown footprint's table behind it");
  __device__ __forceinline__ double* obs2() { return &tr[0][0][0] + POCS_MAX_OBSTACLES * POCS_OBS_STRIDE; }
  __device__ __forceinline__ double* stage() { return &tr[0][0][0]; }
  __device__ __forceinline__ double* adv() { return &slot[0][0][0]; }
  __device__ __forceinline__ double* spec() { return &slot[0][0][0] + POCS_ADV_SCRATCH(K); }
};

// ---------------------------------------------------------------------------------------------
// The moment sums have ONE fixed shape, whatever the launch looks like ("summation
// tree"; oracle/pocs_oracle.c restates it and the two agree bit for bit):
//   lane chain   a lane's samples of one component inside one UNIT-WAVE -- wave v (tid / 64) of virtual slice
//                j of the run, over the slice's chunks in order, sample 2 lp before 2 lp + 1 -- accumulated
//                sequentially: sums += x, fma(x, x, sum) ...; survivors counted as integers;
//   wave sum     the 64 lane chains: eight runs of eight lanes added in lane order, then
//                ((g0 + g1) + (g2 + g3)) + ((g4 + g5) + (g6 + g7))                         (flush_unit)
//   row          of (virtual slice, component): the eight wave sums in wave order          (gmm_emit_rows)
//   total        the run's VS rows as sixteen interleaved partial sums, then those in order (gmm_close_sums)
// A run always has the same VS virtual slices (a function of the shard's sample count only), so the
// result does not depend on how many runs share a launch, on the blocks a launch uses, or on which
// block or wave worked on which slice: a batch of R runs, run-ahead and R single calls give the same bits.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double oct_sum(double s) {     // lanes 8 j .. 8 j + 7 hold g0 .. g7 -> all hold the sum above
  s += dpp_f64<0xB1>(s);     // quad_perm [1,0,3,2]
  s += dpp_f64<0x4E>(s);     // quad_perm [2,3,0,1]
  s += dpp_f64<0x141>(s);    // row_half_mirror
  return s;
}

// A wave leaves component `k` of the unit it is working on (held virtual slice `tl`, run buffer `rb`): its
// lane chains -> the wave sum -> LDS (slot[tl][wave] if this is the unit's first component, otherwise the
// wave's xtra entry of k), and the chains restart.  By LDS transposition, five then four sums at a
// time: every lane writes its values, lane 8 j + q adds lanes 8 q .. 8 q + 7 of sum j, oct_sum adds the
// eight q.  One wave: the LDS executes a wave's instructions in order, nothing else synchronises.
template <int K, int TB, bool OC, bool CL, bool FPN, bool RG, bool SG>
__device__ __forceinline__ void flush_unit(gmm_smem<K, TB, OC, CL, FPN, RG, SG>& sm, const int wave, const int lane, const int rb, const int tl,
                                           const int k, bool& first, double (&acc)[9], int& nfree) {
  double* const T = &sm.tr[wave][0][0];
  double* const dst = first ? &sm.slot[tl][wave][0] : &sm.xtra[rb][wave][k][0];
  const int j = lane >> 3, q = lane & 7;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int nv = pass == 0 ? 5 : 4, v0 = pass == 0 ? 0 : 5;
#pragma unroll
    for (int i = 0; i < nv; ++i) T[i * POCS_FLUSH_PITCH + lane] = acc[v0 + i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    double s = 0.0;
    if (j < nv) {
      const double* p = &T[j * POCS_FLUSH_PITCH + 8 * q];
      s = p[0]; s += p[1]; s += p[2]; s += p[3]; s += p[4]; s += p[5]; s += p[6]; s += p[7];
    }
    s = oct_sum(s);
    if (j < nv && q == 0) dst[1 + v0 + j] = s;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0) {
    dst[0] = (double)nfree;
    if (first) sm.kf[tl][wave] = k; else sm.xj[rb][wave][k] = tl;
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) acc[i] = 0.0;
  nfree = 0;
  first = false;
}

// Cull the obstacle table against the bounding box of the mixture staged in par[rb] (ONE wave, all 64
// lanes).  A Box-Muller normal is bounded: u >= 2^-32 gives |z| <= sqrt(64 ln 2) < 6.661
// (pocs_normal_pair_w2; 6.67 leaves 0.1 % for the rounding of radius * cos), so every pose the run can
// draw lies within mean_k +- 6.67 (|L00|, |L10|+|L11|) of some component; an obstacle whose inflated
// box (the broad phase of pocs_box_hit) misses that region is rejected by the broad phase for every
// sample, so dropping it here changes no flag.
//
// The same bound on the heading makes the broad phase of the kept records tighter than the table's: the
// table inflates an obstacle's box by the footprint's bounding RADIUS (any heading); a run whose
// headings all lie in [t_lo, t_hi] needs only the footprint's largest half-extent along world x and
// along world y over that range (two convex sets that touch overlap in every projection).  Where the
// robot's heading is known to a fraction of a radian -- most of a plan -- far fewer poses reach the
// narrow phase, and none that could touch is lost: the flags do not change.
//   (pocs_footprint_extent, pocs_collide.h: host + device, checked on the CPU against a dense scan)
// The run's reach and the footprint's extents over its headings as ONE wave forms them (all 64 lanes), for k_world_cull: the
// arithmetic of gmm_cull below through the host + device functions of pocs_world.h, the four end values side by side in lanes
// 0 .. 3 as there.  (gmm_cull keeps its own text: built on top of this function it computed the same values with the
// instructions of every sampling kernel in another order -- profiles/large_world_isa.txt.)
template <int K>
__device__ __forceinline__ void gmm_reach(const pocs_footprint& fp, const double fp_rr, const double fp_phi, const int lane, const double* par,
                                          pocs_reach& rc, double& ext_x, double& ext_y) {
  pocs_world_reach_box(par, K, fp, rc);
  const double tlo = rc.tlo, thi = rc.thi;
  const double HALF_PI = 1.57079632679489661923;
  // pocs_footprint_extent_pre for world x (the range as it is) and world y (shifted by a quarter turn), with the four end
  // values -- a general sine and cosine each, ~70 dependent operations -- evaluated side by side in lanes 0 .. 3 instead of
  // one after the other in every lane: the same functions of the same arguments, a quarter of the wave's time
  const double end_t = ((lane & 1) ? thi : tlo) - ((lane & 2) ? HALF_PI : 0.0);      // tlo, thi, tlo - pi/2, thi - pi/2
  const double end_f = pocs_footprint_extent_end(fp.hx, fp.hy, end_t);
  ext_x = pocs_footprint_extent_is_radius(fp_phi, tlo, thi) ? fp_rr
        : pocs_footprint_extent_of_ends(fp_rr, lane_value(end_f, 0), lane_value(end_f, 1));
  ext_y = pocs_footprint_extent_is_radius(fp_phi, tlo - HALF_PI, thi - HALF_PI) ? fp_rr
        : pocs_footprint_extent_of_ends(fp_rr, lane_value(end_f, 2), lane_value(end_f, 3));
}
// RN (pocs_set_disc_covariances; `nz`: the block's kept rows, [2][POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE] in LDS): lane m also fetches
// record m's row of the launch's noise table; the tightened box gains the record's growth gx = 6.67 |l00|, gy = 6.67 (|l10| + |l11|)
// -- the host's own operations, so that the table's grown fields 6 and 7 and the tightened ones bound the same displaced disc
// (pocs_collide.h, the block above pocs_disc_noise_factor) -- and a kept record's row is written to the kept list's position.
// RH (pocs_set_disc_hypotheses, on top of RN; the rows may all be zeros): lane m also fetches record m's gate of the launch's gate table
// and a kept record's gate is written to the kept list's position behind the rows (gmm_gates).  No box changes: removing a disc for
// a pose can only remove hits (pocs_collide.h, the block above pocs_hyp_thresholds).
template <bool RN = false, bool RH = false, int K, int TB, bool OC, bool CL, bool FPN, bool RG, bool SG>
__device__ __forceinline__ void gmm_cull(const pocs_gmm_launch& a, gmm_smem<K, TB, OC, CL, FPN, RG, SG>& sm, const int rb, const int lane, const double* par,
                                         [[maybe_unused]] double* nz = nullptr) {
  const pocs_footprint fp = a.fp;
  const int M = a.M;
  const double* const obs = sm.obs();
  double xlo = 1e300, xhi = -1e300, ylo = 1e300, yhi = -1e300, tlo = 1e300, thi = -1e300;
#pragma unroll
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
  const double HALF_PI = 1.57079632679489661923;
  // pocs_footprint_extent_pre for world x (the range as it is) and world y (shifted by a quarter turn), with the four end
  // values -- a general sine and cosine each, ~70 dependent operations -- evaluated side by side in lanes 0 .. 3 instead of
  // one after the other in every lane: the same functions of the same arguments, a quarter of the wave's time
  const double end_t = ((lane & 1) ? thi : tlo) - ((lane & 2) ? HALF_PI : 0.0);      // tlo, thi, tlo - pi/2, thi - pi/2
  const double end_f = pocs_footprint_extent_end(fp.hx, fp.hy, end_t);
  const double ext_x = pocs_footprint_extent_is_radius(a.fp_phi, tlo, thi) ? a.fp_rr
                     : pocs_footprint_extent_of_ends(a.fp_rr, lane_value(end_f, 0), lane_value(end_f, 1));
  const double ext_y = pocs_footprint_extent_is_radius(a.fp_phi, tlo - HALF_PI, thi - HALF_PI) ? a.fp_rr
                     : pocs_footprint_extent_of_ends(a.fp_rr, lane_value(end_f, 2), lane_value(end_f, 3));
  bool keep = false;
  double bx = 0.0, by = 0.0;
  [[maybe_unused]] double row[POCS_NOISE_STRIDE] = {0.0, 0.0, 0.0, 0.0};
  if (lane < M) {
    const double* o = &obs[lane * POCS_OBS_STRIDE];
    if constexpr (RN) {
#pragma unroll
      for (int j = 0; j < POCS_NOISE_STRIDE; ++j) row[j] = a.noise[lane * POCS_NOISE_STRIDE + j];
      const double gx = 6.67 * fabs(row[0]), gy = 6.67 * (fabs(row[1]) + fabs(row[2]));
      bx = fmin(o[6], fma(o[4], fabs(o[2]), o[5] * fabs(o[3])) * (1.0 + 1e-12) + ext_x + gx);
      by = fmin(o[7], fma(o[4], fabs(o[3]), o[5] * fabs(o[2])) * (1.0 + 1e-12) + ext_y + gy);
    } else {
    // the obstacle's own world box (as pocs_prepare_obstacle) + the footprint's extents for this run
    bx = fmin(o[6], fma(o[4], fabs(o[2]), o[5] * fabs(o[3])) * (1.0 + 1e-12) + ext_x);
    by = fmin(o[7], fma(o[4], fabs(o[3]), o[5] * fabs(o[2])) * (1.0 + 1e-12) + ext_y);
    }
    keep = !(o[0] - bx > xhi || o[0] + bx < xlo || o[1] - by > yhi || o[1] + by < ylo);
  }
  const unsigned long long mask = __ballot(keep);
  if (keep) {
    const int pos = __popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
    for (int j = 0; j < 6; ++j) sm.keep[rb][pos * POCS_OBS_STRIDE + j] = obs[lane * POCS_OBS_STRIDE + j];
    sm.keep[rb][pos * POCS_OBS_STRIDE + 6] = bx;
    sm.keep[rb][pos * POCS_OBS_STRIDE + 7] = by;
    if constexpr (OC) sm.oci[rb][pos] = lane;      // the kept slot's index in the caller's table: its counter leaves under it
    if constexpr (RN) {
#pragma unroll
      for (int j = 0; j < POCS_NOISE_STRIDE; ++j) nz[(rb * POCS_MAX_OBSTACLES + pos) * POCS_NOISE_STRIDE + j] = row[j];
    }
    if constexpr (RH) {
      static_assert(!RH || RN, "hypotheses: on top of the noise form");
      uint32_t* const gz = gmm_gates(nz, rb) + pos * POCS_GATE_STRIDE;
#pragma unroll
      for (int j = 0; j < POCS_GATE_STRIDE; ++j) gz[j] = a.gates[lane * POCS_GATE_STRIDE + j];
    }
  }
  if constexpr (OC) sm.occ[rb][lane] = 0u;           // (one wave, POCS_MAX_OBSTACLES = 64 lanes: every counter of the buffer)
  if (lane == 0) sm.nkeep[rb] = __popcll(mask);
}

// The cull under a round footprint (pocs_set_footprint_disc; one wave, all 64 lanes): the footprint's extent is rho at every heading,
// so the table's fields 6 and 7 -- the record's own world box + rho, an uncertain disc's growth included -- are already tight and the
// kept list carries them as they are; the run's heading range, the four end values and fp_phi are not formed.  The keep test is
// gmm_cull's on those fields, with pad = 1e-6 (the footprint is centred): a record it drops is rejected by the broad phase for every
// pose the run can draw, and a kept record keeps its own broad phase, so the kept list's flags are the full table's, bit for bit.
// RN: a kept record's row of the launch's noise table is written to the kept list's position, as gmm_cull<true> does.
template <bool RN, int K, int TB, bool OC, bool CL, bool FPN, bool RG, bool SG>
__device__ __forceinline__ void gmm_cull_rfoot(const pocs_gmm_launch& a, gmm_smem<K, TB, OC, CL, FPN, RG, SG>& sm, const int rb, const int lane, const double* par,
                                               [[maybe_unused]] double* nz = nullptr) {
  const int M = a.M;
  const double* const obs = sm.obs();
  double xlo = 1e300, xhi = -1e300, ylo = 1e300, yhi = -1e300;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double* p = &par[k * POCS_PARAM_STRIDE];
    const double ex = 6.67 * fabs(p[3]), ey = 6.67 * (fabs(p[4]) + fabs(p[5]));
    xlo = fmin(xlo, p[0] - ex); xhi = fmax(xhi, p[0] + ex);
    ylo = fmin(ylo, p[1] - ey); yhi = fmax(yhi, p[1] + ey);
  }
  const double pad = 1e-6;
  xlo -= pad; xhi += pad; ylo -= pad; yhi += pad;
  bool keep = false;
  if (lane < M) {
    const double* o = &obs[lane * POCS_OBS_STRIDE];
    keep = !(o[0] - o[6] > xhi || o[0] + o[6] < xlo || o[1] - o[7] > yhi || o[1] + o[7] < ylo);
  }
  const unsigned long long mask = __ballot(keep);
  if (keep) {
    const int pos = __popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
    for (int j = 0; j < POCS_OBS_STRIDE; ++j) sm.keep[rb][pos * POCS_OBS_STRIDE + j] = obs[lane * POCS_OBS_STRIDE + j];
    if constexpr (RN) {
#pragma unroll
      for (int j = 0; j < POCS_NOISE_STRIDE; ++j) nz[(rb * POCS_MAX_OBSTACLES + pos) * POCS_NOISE_STRIDE + j] = a.noise[lane * POCS_NOISE_STRIDE + j];
    }
  }
  if (lane == 0) sm.nkeep[rb] = __popcll(mask);
}

// The clearance form's second list (one wave, all 64 lanes, beside the wave that runs gmm_cull for the same run buffer): the table
// prepared for the footprint grown by the largest clearance (sm.obs2()) culled against the same mixture with that footprint's
// extents -- gmm_cull's arithmetic with clh's footprint, radius and corner angle in place of the launch's -- into keep2[rb]; the
// level counters of the buffer start at zero.  Conservative for every smaller level: their footprints lie inside this one.
template <int K, int TB, bool OC>
__device__ __forceinline__ void gmm_cull_clear(const pocs_gmm_launch& a, gmm_smem<K, TB, OC, true>& sm, const int rb, const int lane, const double* par) {
  const pocs_footprint fp = {sm.clh[0], sm.clh[1], sm.clh[2], sm.clh[3]};
  const double fp_rr = sm.clh[4], fp_phi = sm.clh[5];
  const int M = a.M;
  const double* const obs = sm.obs2();
  double xlo = 1e300, xhi = -1e300, ylo = 1e300, yhi = -1e300, tlo = 1e300, thi = -1e300;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double* p = &par[k * POCS_PARAM_STRIDE];
    const double ex = 6.67 * fabs(p[3]), ey = 6.67 * (fabs(p[4]) + fabs(p[5])), et = 6.67 * (fabs(p[6]) + fabs(p[7]) + fabs(p[8]));
    xlo = fmin(xlo, p[0] - ex); xhi = fmax(xhi, p[0] + ex);
    ylo = fmin(ylo, p[1] - ey); yhi = fmax(yhi, p[1] + ey);
    tlo = fmin(tlo, p[2] - et); thi = fmax(thi, p[2] + et);
  }
  const double pad = sqrt(fp.dx * fp.dx + fp.dy * fp.dy) + 1e-6;
  xlo -= pad; xhi += pad; ylo -= pad; yhi += pad;
  tlo -= 1e-9 * (1.0 + fabs(tlo)); thi += 1e-9 * (1.0 + fabs(thi));
  const double HALF_PI = 1.57079632679489661923;
  const double end_t = ((lane & 1) ? thi : tlo) - ((lane & 2) ? HALF_PI : 0.0);
  const double end_f = pocs_footprint_extent_end(fp.hx, fp.hy, end_t);
  const double ext_x = pocs_footprint_extent_is_radius(fp_phi, tlo, thi) ? fp_rr
                     : pocs_footprint_extent_of_ends(fp_rr, lane_value(end_f, 0), lane_value(end_f, 1));
  const double ext_y = pocs_footprint_extent_is_radius(fp_phi, tlo - HALF_PI, thi - HALF_PI) ? fp_rr
                     : pocs_footprint_extent_of_ends(fp_rr, lane_value(end_f, 2), lane_value(end_f, 3));
  bool keep = false;
  double bx = 0.0, by = 0.0;
  if (lane < M) {
    const double* o = &obs[lane * POCS_OBS_STRIDE];
    bx = fmin(o[6], fma(o[4], fabs(o[2]), o[5] * fabs(o[3])) * (1.0 + 1e-12) + ext_x);
    by = fmin(o[7], fma(o[4], fabs(o[3]), o[5] * fabs(o[2])) * (1.0 + 1e-12) + ext_y);
    keep = !(o[0] - bx > xhi || o[0] + bx < xlo || o[1] - by > yhi || o[1] + by < ylo);
  }
  const unsigned long long mask = __ballot(keep);
  if (keep) {
    const int pos = __popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
    for (int j = 0; j < 6; ++j) sm.keep2[rb][pos * POCS_OBS_STRIDE + j] = obs[lane * POCS_OBS_STRIDE + j];
    sm.keep2[rb][pos * POCS_OBS_STRIDE + 6] = bx;
    sm.keep2[rb][pos * POCS_OBS_STRIDE + 7] = by;
  }
  if (lane < POCS_MAX_CLEARANCE_LEVELS) sm.clc[rb][lane] = 0u;
  if (lane == 0) sm.nkeep2[rb] = __popcll(mask);
}

// The parts form's cull (one wave, all 64 lanes, in place of gmm_cull): ONE kept list per run buffer for the compound footprint
// staged in sm.fpp.  Per part f gmm_cull's arithmetic with the part's offset, half extents, bounding radius and corner angle: the
// mixture's box padded by the part's own offset, the part's extents over the run's headings (the four end values of part f side
// by side in lanes 4 f .. 4 f + 3), the record's broad-phase box for that part (never more than the table's, which is sized for the
// largest part).  A record is kept if the keep test passes for ANY part; its fields 6 and 7 are the largest of the parts' boxes, so
// the broad phase of the sampling loop -- against each part's own centre -- is conservative for every part: no flag changes.
template <int K, int TB>
__device__ __forceinline__ void gmm_cull_parts(const pocs_gmm_launch& a, gmm_smem<K, TB, false, false, true>& sm, const int rb, const int lane, const double* par) {
  const int M = a.M, F = a.parts_F;
  const double* const obs = sm.obs();
  double xlo = 1e300, xhi = -1e300, ylo = 1e300, yhi = -1e300, tlo = 1e300, thi = -1e300;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double* p = &par[k * POCS_PARAM_STRIDE];
    const double ex = 6.67 * fabs(p[3]), ey = 6.67 * (fabs(p[4]) + fabs(p[5])), et = 6.67 * (fabs(p[6]) + fabs(p[7]) + fabs(p[8]));
    xlo = fmin(xlo, p[0] - ex); xhi = fmax(xhi, p[0] + ex);
    ylo = fmin(ylo, p[1] - ey); yhi = fmax(yhi, p[1] + ey);
    tlo = fmin(tlo, p[2] - et); thi = fmax(thi, p[2] + et);
  }
  tlo -= 1e-9 * (1.0 + fabs(tlo)); thi += 1e-9 * (1.0 + fabs(thi));
  const double HALF_PI = 1.57079632679489661923;
  static_assert(POCS_MAX_FOOTPRINT_PARTS == 4, "lanes 4 f + e");
  const int pf = ((lane >> 2) & 3) < F ? ((lane >> 2) & 3) : 0;      // (the lanes past 4 F repeat a part: their values are not read)
  const double end_t = ((lane & 1) ? thi : tlo) - ((lane & 2) ? HALF_PI : 0.0);      // tlo, thi, tlo - pi/2, thi - pi/2
  const double end_f = pocs_footprint_extent_end(sm.fpp[pf * POCS_PART_STRIDE + 2], sm.fpp[pf * POCS_PART_STRIDE + 3], end_t);
  const bool in = lane < M;
  const double* const o = &obs[(in ? lane : 0) * POCS_OBS_STRIDE];
  const double o0 = o[0], o1 = o[1], o6 = o[6], o7 = o[7];
  const double ax = fma(o[4], fabs(o[2]), o[5] * fabs(o[3])) * (1.0 + 1e-12), ay = fma(o[4], fabs(o[3]), o[5] * fabs(o[2])) * (1.0 + 1e-12);
  bool keep = false;
  double bx = 0.0, by = 0.0;
#pragma unroll 1
  for (int f = 0; f < F; ++f) {                      // (scalar)
    const double* q = &sm.fpp[f * POCS_PART_STRIDE];
    const double rr = q[4], phi = q[5];
    const double e0 = lane_value(end_f, 4 * f), e1 = lane_value(end_f, 4 * f + 1), e2 = lane_value(end_f, 4 * f + 2), e3 = lane_value(end_f, 4 * f + 3);
    const double ext_x = pocs_footprint_extent_is_radius(phi, tlo, thi) ? rr : pocs_footprint_extent_of_ends(rr, e0, e1);
    const double ext_y = pocs_footprint_extent_is_radius(phi, tlo - HALF_PI, thi - HALF_PI) ? rr : pocs_footprint_extent_of_ends(rr, e2, e3);
    const double pad = sqrt(q[0] * q[0] + q[1] * q[1]) + 1e-6;       // the part's centre vs the base
    const double bxf = fmin(o6, ax + ext_x), byf = fmin(o7, ay + ext_y);
    if (in && !(o0 - bxf > xhi + pad || o0 + bxf < xlo - pad || o1 - byf > yhi + pad || o1 + byf < ylo - pad)) keep = true;
    bx = fmax(bx, bxf); by = fmax(by, byf);
  }
  const unsigned long long mask = __ballot(keep);
  if (keep) {
    const int pos = __popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
    for (int j = 0; j < 6; ++j) sm.keep[rb][pos * POCS_OBS_STRIDE + j] = obs[lane * POCS_OBS_STRIDE + j];
    sm.keep[rb][pos * POCS_OBS_STRIDE + 6] = bx;
    sm.keep[rb][pos * POCS_OBS_STRIDE + 7] = by;
  }
  if (lane == 0) sm.nkeep[rb] = __popcll(mask);
}

// The regions form's reach (one wave, all 64 lanes, beside the wave that runs gmm_cull for the same run buffer): lane g decides
// whether the run's mixture can reach region g at all -- gmm_cull's conservative keep test against the mixture's bounding box (the
// same 6.67 sigma box, padded by the footprint's offset), with the region's own footprint: the record's broad-phase half extents
// are its AABB grown by that footprint's bounding radius (pocs_prepare_obstacle), which bounds the footprint's extent at every
// heading.  A region that fails it fails pocs_box_hit's broad phase for every sample of the run.  The answers are a bit each in
// rgk[rb]; the region counters of the buffer start at zero.
template <int K, int TB, bool OC, bool CL, bool FPN>
__device__ __forceinline__ void gmm_cull_regions(const pocs_gmm_launch& a, gmm_smem<K, TB, OC, CL, FPN, true>& sm, const int rb, const int lane, const double* par) {
  double xlo = 1e300, xhi = -1e300, ylo = 1e300, yhi = -1e300;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double* p = &par[k * POCS_PARAM_STRIDE];
    const double ex = 6.67 * fabs(p[3]), ey = 6.67 * (fabs(p[4]) + fabs(p[5]));
    xlo = fmin(xlo, p[0] - ex); xhi = fmax(xhi, p[0] + ex);
    ylo = fmin(ylo, p[1] - ey); yhi = fmax(yhi, p[1] + ey);
  }
  bool keep = false;
  if (lane < a.reg_G) {
    const double* o = &sm.rgh[lane * POCS_OBS_STRIDE];
    const double* f = &sm.rgh[POCS_MAX_REGIONS * POCS_OBS_STRIDE + 4 * lane];
    const double pad = sqrt(f[0] * f[0] + f[1] * f[1]) + 1e-6;
    keep = !(o[0] - o[6] > xhi + pad || o[0] + o[6] < xlo - pad || o[1] - o[7] > yhi + pad || o[1] + o[7] < ylo - pad);
  }
  const unsigned long long mask = __ballot(keep);
  if (lane < POCS_MAX_REGIONS) sm.rgc[rb][lane] = 0u;
  if (lane == 0) sm.rgk[rb] = (unsigned)mask;
}

// The segment form's second list (one wave, all 64 lanes, beside the wave that runs gmm_cull for the same run buffer; `r` is the run):
// the records some SUB-POSE of some sample of the run can touch.  A sub-pose's centre lies up to |u[1]| from its sample's (the drive
// of sub-pose j is a rounded fraction of u[1], and the drive direction is a unit vector up to rounding), and its heading is the
// sample's shifted by -u[2]: so the mixture's 6.67 sigma box is grown by |u[1]| (and the footprint's offset, and a margin for the
// rounding), and a record is tested with the table's own broad-phase box -- its AABB grown by the footprint's bounding radius, which
// bounds the footprint's extent at EVERY heading: no range of headings is assumed for the sub-poses.  A record that fails this is
// failed by pocs_box_hit's broad phase for every sub-pose of the run, so dropping it changes no flag; the kept records keep the
// table's fields 6 and 7.  At waypoint 0 there is no way in: the list is empty.  An empty list skips all sub-pose work of the run
// buffer by one scalar branch (gmm_units).  The wave also stages J, the fractions and the run's applied control of step w - 1 (chain
// record [0..2]), and zeroes the buffer's counter.
template <int K, int TB>
__device__ __forceinline__ void gmm_cull_seg(const pocs_gmm_launch& a, gmm_smem<K, TB, false, false, false, false, true>& sm, const int rb, const int lane,
                                             const double* par, const int r) {
  const int w = a.waypoint, M = a.M;
  const int J = a.seg->J;
  const double* const ch = a.chain + ((size_t)r * (a.W > 1 ? a.W - 1 : 1) + (w > 0 ? w - 1 : 0)) * POCS_CHAIN_STRIDE;
  const double u1 = w > 0 ? ch[1] : 0.0;
  if (lane < POCS_MAX_SEGMENT_CHECKS) sm.sgf[rb][lane] = a.seg->f[lane];
  if (lane < 3) sm.sgu[rb][lane] = w > 0 ? ch[lane] : 0.0;
  const pocs_footprint fp = a.fp;
  const double* const obs = sm.obs();
  double xlo = 1e300, xhi = -1e300, ylo = 1e300, yhi = -1e300;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double* p = &par[k * POCS_PARAM_STRIDE];
    const double ex = 6.67 * fabs(p[3]), ey = 6.67 * (fabs(p[4]) + fabs(p[5]));
    xlo = fmin(xlo, p[0] - ex); xhi = fmax(xhi, p[0] + ex);
    ylo = fmin(ylo, p[1] - ey); yhi = fmax(yhi, p[1] + ey);
  }
  const double pad = sqrt(fp.dx * fp.dx + fp.dy * fp.dy) + fabs(u1) * (1.0 + 1e-9) + 1e-6;   // footprint centre vs base, the drive
  xlo -= pad; xhi += pad; ylo -= pad; yhi += pad;
  bool keep = false;
  if (lane < M && w > 0 && J > 1) {
    const double* o = &obs[lane * POCS_OBS_STRIDE];
    keep = !(o[0] - o[6] > xhi || o[0] + o[6] < xlo || o[1] - o[7] > yhi || o[1] + o[7] < ylo);
  }
  const unsigned long long mask = __ballot(keep);
  if (keep) {
    const int pos = __popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
    for (int j = 0; j < POCS_OBS_STRIDE; ++j) sm.keeps[rb][pos * POCS_OBS_STRIDE + j] = obs[lane * POCS_OBS_STRIDE + j];
  }
  if (lane == 0) { sm.nkeeps[rb] = __popcll(mask); sm.sgc[rb] = 0u; sm.sgJ[rb] = J; }
}

// ---------------------------------------------------------------------------------------------
// THE BODY: units [ta, tb) of the launch (unit t = virtual slice t mod VS of run t / VS; at most
// POCS_GMM_SUB of them, of at most two runs r0 and r0 + 1 whose parameters and culled tables are staged
// in buffers 0 and 1), as every thread of the block runs them: GM_Model::sampleNPoints
// (GM_Model.h:83-116) + checkMatrixCollisions (MCSimulator.h:241-253) + the moment sums (:592-611),
// fused, one PAIR of samples per thread and iteration.  The waves of the block do not meet in here: each
// works through the units at its own pace and leaves its wave sums in LDS (flush_unit).  What a lane adds
// up, and in which order, depends on (run, virtual slice, wave, lane) only.
// ---------------------------------------------------------------------------------------------
//   zpre / npre (the lone form, LONE_PRE): the normals of the unit's first `npre` iterations, drawn in the block's head by
//   the waves that waited there ([iteration][sample of the pair x 3][thread]); the same function of the same arguments,
//   the same bits -- a call of one run then spends its sampling phase on what depends on the mixture only
//   OC (POCS_OPT_OBSTACLE_COUNTS): per kept record and pose of the pair, the lanes that touch it and whose sample exists are
//   balloted; hits are rare, so a zero ballot -- nearly all of them -- is skipped by a scalar branch, and otherwise one lane
//   adds the population count to the block's LDS counter of (run buffer, kept slot).  Nothing else differs: the same
//   pocs_pair_collides_masks, with every record's answer handed out.
//   CL (pocs_set_clearance_levels): behind the unchanged base test the level test runs on the second kept list
//   (pocs_pair_clearance_masks); per level the lanes whose sample exists are picked by scalar ands of the masks and one lane adds
//   the population count to the block's LDS counter of (run buffer, level).  The odd shard's unused twin does not count.
//   FPN (pocs_set_footprint_parts, F > 1): the collision test is pocs_pair_parts_masks over the parts staged in sm.fpp, on the one
//   kept list (gmm_cull_parts); the flag is the OR of the parts' flags and everything behind it is what it is.
//   RG (pocs_set_regions): behind the unchanged collision test the region test runs over the regions the run's mixture can reach
//   (sm.rgk[rb]: usually none, one scalar branch); per region the lanes whose sample exists, whose flag is 0 and which are in the
//   region are picked by scalar ands of the masks and lane 0 adds the population count to the block's LDS counter of (run buffer,
//   region).  The odd shard's unused twin does not count.
//   SG (pocs_set_segment_checks, J > 1): behind the unchanged collision test of the samples themselves, where the run's second kept list
//   is not empty (usually it is: one scalar branch), the J - 1 sub-poses on each sample's way in are tested on that list
//   (pocs_pair_segment_masks, backwards along the run's applied control); lane 0 adds the population count of the lanes whose sample
//   exists, whose own flag is 0 and some sub-pose of which touches to the block's LDS counter of the run buffer, and the sub-poses'
//   masks are or-ed into the flags: everything behind is formed from those.  The odd shard's unused twin does not count.
//   RD (pocs_set_discs, D > 0): the kept list may hold disc records; the collision test is pocs_pair_collides_masks' ROUND form, which
//   decides a record's kind by a scalar branch and ballots the disc's answer into the same masks.  Nothing else differs.
//   RN (pocs_set_disc_covariances, on top of RD; `nz`: the kept rows gmm_cull<true> left): the ROUND form is handed the run buffer's
//   rows, the run's seed, the lane's pair index pair0 + lp and the waypoint, and tests an uncertain disc on its displaced centre.
//   RF (pocs_set_footprint_disc, with or without RN, never with RD: the form serves worlds with and without discs): the collision test
//   is pocs_pair_round_masks on the kept list gmm_cull_rfoot left -- the radius is fp.hx, the headings are not looked at.
//   RH (pocs_set_disc_hypotheses, on top of RD and RN, never with RF): the ROUND form is handed the run buffer's gates as well
//   (gmm_gates) and the waypoint as the hypotheses' word too, and a gated disc counts for the poses for which it exists.
template <int K, bool STORE, int TB, bool LONE_PRE = false, bool OC = false, bool CL = false, bool FPN = false, bool RG = false, bool SG = false,
          bool RD = false, bool RN = false, bool RF = false, bool RH = false>
__device__ __forceinline__ void gmm_units(const pocs_gmm_launch& a, gmm_smem<K, TB, OC, CL, FPN, RG, SG>& sm, const int w, const int r0,
                                          const int ta, const int tb, const double* zpre = nullptr, const int npre = 0,
                                          [[maybe_unused]] const double* nz = nullptr) {
  static_assert(!RN || RD || RF, "uncertain discs: on top of the round form");
  static_assert(!(RF && (RD || LONE_PRE || OC || CL || FPN || RG || SG)), "a round footprint: a family of its own");
  static_assert(!RH || (RD && RN && !RF), "hypotheses: on top of the noise form, a footprint box");
  const pocs_tables* const s_tab = &sm.tab;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const pocs_footprint fp = a.fp;
  const int vs_mask = (1 << a.vs_shift) - 1;
  //   acc[0..8] = sums of x, y, t, xx, xy, xt, yy, yt, tt over the survivors of the component being
  //   accumulated (a wave works through the component blocks in order), nfree = their number (the wave's)
  double acc[9];
  int nfree = 0;
#pragma unroll
  for (int j = 0; j < 9; ++j) acc[j] = 0.0;
  // Positions inside the shard are 32-bit (the host refuses shards of 2^31 samples and more): LOCAL sample
  // i is global sample first + i, local pair lp holds local samples 2 lp, 2 lp + 1 (a.first is even,
  // checked by the host), and everything the unit loop decides -- chunk ranges, the end of a component
  // block, whole or general iteration -- is scalar integer arithmetic.
  const int count = (int)a.count;
  const int npairs = (count + 1) >> 1;
  const uint64_t pair0 = (uint64_t)(a.first >> 1);
  const double first_d = (double)a.first;
  const int wave_first = 128 * wave;                // the wave's first sample within a chunk
  // The (up to) four waves of a SIMD -- two of this block, two of the co-resident one -- are arbitrated
  // by priority, then AGE: left alone, the oldest wave of a SIMD runs ~1.7 x faster than the youngest for
  // the whole launch.  Rotating the priority with the iteration gives every wave the same share.
  // slot = which of the block's waves on this SIMD: wave v runs on SIMD v mod 4, so waves v and v + 4 share
  // one.  The second block of a CU is (observed, speed only) the one dispatched 256 blocks later.
  const int prio_slot = (TB >= 512 ? (wave >> 2) : 0) + (TB >= 512 ? 2 : 1) * (int)((blockIdx.x >> 8) & 3u);
  int prio_it = prio_slot;
  // per run (wave-uniform; reloaded when the block's range crosses into its second run)
  int rb = -1, nkeep = 0, kcur = 0, kw = 0;
  const double* s_par = nullptr;
  const double* s_keep = nullptr;
  [[maybe_unused]] const double* s_keep2 = nullptr;       // CL: the second kept list and its length
  [[maybe_unused]] int nkeep2 = 0;
  [[maybe_unused]] unsigned rgkeep = 0u;                  // RG: the regions in the run's reach, a bit each
  [[maybe_unused]] const double* s_keeps = nullptr;       // SG: the second kept list, its length, J, the fractions, the applied control
  [[maybe_unused]] int nkeeps = 0, sgJ = 1;
  [[maybe_unused]] const double* s_sgf = nullptr;
  [[maybe_unused]] double sg_u1 = 0.0, sg_u2 = 0.0;
  uint64_t seed = 0;
  double cumn[K > 1 ? K - 1 : 1];                   // cumulative component counts
  double *xr = nullptr, *yr = nullptr, *tr = nullptr;
  int16_t* fr = nullptr;
  int seg_end = 0;                                  // local sample index up to which (exclusive) the samples belong to component kw and exist
  POCS_VCONST(vc_);                                 // polynomial constants held in vector registers (pocs_math.h)
  const pocs_vconst* const vc = &vc_;

  // ONE iteration = 2 * TB samples, one pair per thread.  WHOLE (compile time): the wave's 128 samples lie
  // inside component block kw and inside the shard -- every lane live, both samples of its pair exist,
  // the component is the scalar kw == kcur.  Otherwise: the general case (a block boundary inside the
  // wave, the shard's last chunk), every decision per lane.  Same arithmetic per sample either way.
  int it_unit = 0;                                  // (lone form) the iteration's number within the unit
  auto iteration = [&](auto whole_tag, const int base, const int tl, bool& first) __attribute__((always_inline)) {
    constexpr bool WHOLE = decltype(whole_tag)::value;
    switch (prio_it++ & 3) {                       // s_setprio takes an immediate
      case 0: __builtin_amdgcn_s_setprio(0); break;
      case 1: __builtin_amdgcn_s_setprio(1); break;
      case 2: __builtin_amdgcn_s_setprio(2); break;
      default: __builtin_amdgcn_s_setprio(3); break;
    }
    const int lp = base + tid;
    const bool live = WHOLE || lp < npairs;        // a lane past the end computes, masked
    double zz[2][3];
    uint32_t spare[2];
    // The seed is made opaque once per iteration: otherwise the compiler hoists all 20 Philox round
    // keys (seed + r * Weyl constants) out of the loop and pins 20 SGPRs of a register file that is
    // already spilling; recomputing them costs 2 scalar adds per round.
    uint64_t seed_it = seed;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(seed_it));
#endif
    bool drawn = false;
    if constexpr (LONE_PRE) {
      if (it_unit < npre) {                          // (scalar)
        const double* z = zpre + (size_t)it_unit * 6 * TB + tid;
#pragma unroll
        for (int q = 0; q < 3; ++q) { zz[0][q] = z[q * TB]; zz[1][q] = z[(3 + q) * TB]; }
        drawn = true;
        ++it_unit;
      }
    }
    if (!drawn) {
      POCS_TUNE_NORMALS(pocs_normal3_pair(seed_it, pair0 + (uint64_t)(unsigned)lp, (uint32_t)w, POCS_STREAM_GMM, s_tab, zz[0], zz[1], &spare[0], &spare[1], vc));
    }
    const int i0 = 2 * lp;
    const bool two = WHOLE || (live && (i0 + 1) < count);  // false only for the last sample of an odd shard
    double xs[2], ys[2], ts[2];
    unsigned long long hits[2];                     // the two poses' flags as lane masks (pocs_pair_collides_masks)
    int ks[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      int k = kw;                                   // WHOLE: one LDS address for the wave, broadcast reads
      if (!WHOLE) {
        // component of the sample (GM_Model.h:87-107: counts[k] samples per component, one block
        // after the other): the first component whose cumulative count exceeds the global index
        const double gidx = (first_d + (double)i0) + (double)h;   // exact: < 2^53
        k = 0;
#pragma unroll
        for (int j = 0; j < K - 1; ++j) k += (cumn[j] <= gidx) ? 1 : 0;
      }
      const double* p = &s_par[k * POCS_PARAM_STRIDE];
      // mvnrnd (glue_mvnrnd_meat.hpp:134-145): chol_lower * z + mean
      xs[h] = fma(p[3], zz[h][0], p[0]);
      ys[h] = fma(p[5], zz[h][1], fma(p[4], zz[h][0], p[1]));
      ts[h] = fma(p[8], zz[h][2], fma(p[7], zz[h][1], fma(p[6], zz[h][0], p[2])));
      ks[h] = k;
    }
    POCS_TUNE_COLLIDE_STATS();
    if constexpr (FPN) {
      pocs_pair_parts_masks(xs, ys, ts, sm.fpp, a.parts_F, s_keep, nkeep, s_tab, vc, hits);
    } else
    if constexpr (OC) {
      unsigned* const occ = sm.occ[rb];
      pocs_pair_collides_masks<LONE_PRE>(xs, ys, ts, &fp, s_keep, nkeep, s_tab, vc, hits, [&](const int m, const int h, const bool t) {
        const unsigned long long b = __ballot(t && (h == 0 ? live : two));      // the odd shard's unused twin does not count
        if (b != 0ull && lane == (int)__builtin_ctzll(b))
          __hip_atomic_fetch_add(&occ[m], (unsigned)__popcll(b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      });
    } else
    if constexpr (RF) {
      if constexpr (RN) {
        const pocs_noise_pair np = {nz + rb * (POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE), seed_it, pair0 + (uint64_t)(unsigned)lp, (uint32_t)w};
        pocs_pair_round_masks<pocs_noise_pair>(xs, ys, fp.hx, s_keep, nkeep, s_tab, vc, hits, nullptr, np);
      } else {
        pocs_pair_round_masks(xs, ys, fp.hx, s_keep, nkeep, s_tab, vc, hits);
      }
    } else
    if constexpr (RH) {
      const pocs_noise_gate_pair np = {nz + rb * (POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE), seed_it, pair0 + (uint64_t)(unsigned)lp, (uint32_t)w,
                                       gmm_gates(const_cast<double*>(nz), rb), (uint32_t)w};
      pocs_pair_collides_masks<false, pocs_each_none, true, pocs_noise_gate_pair>(xs, ys, ts, &fp, s_keep, nkeep, s_tab, vc, hits, pocs_each_none(), nullptr, np);
    } else
    if constexpr (RN) {
      const pocs_noise_pair np = {nz + rb * (POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE), seed_it, pair0 + (uint64_t)(unsigned)lp, (uint32_t)w};
      pocs_pair_collides_masks<false, pocs_each_none, true, pocs_noise_pair>(xs, ys, ts, &fp, s_keep, nkeep, s_tab, vc, hits, pocs_each_none(), nullptr, np);
    } else
    if constexpr (RD) {
      pocs_pair_collides_masks<false, pocs_each_none, true>(xs, ys, ts, &fp, s_keep, nkeep, s_tab, vc, hits);
    } else {
    POCS_TUNE_COLLIDE(pocs_pair_collides_masks<LONE_PRE>(xs, ys, ts, &fp, s_keep, nkeep, s_tab, vc, hits));
    }
    if constexpr (CL) {
      const unsigned long long lm = WHOLE ? ~0ull : __ballot(live), tm = WHOLE ? ~0ull : __ballot(two);
      unsigned* const clc = sm.clc[rb];
      pocs_pair_clearance_masks(xs, ys, ts, &fp, &sm.clh[6], a.clr_L, s_keep2, nkeep2, s_tab, vc,
                                [&](const int l, const unsigned long long m0, const unsigned long long m1) {
        const unsigned n = (unsigned)__popcll(m0 & lm) + (unsigned)__popcll(m1 & tm);      // (scalar)
        if (n != 0u && lane == 0) __hip_atomic_fetch_add(&clc[l], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      });
    }
    if constexpr (RG) {
      if (rgkeep != 0u) {                                            // (scalar: nearly every waypoint's belief is near no region)
        const unsigned long long f0 = (WHOLE ? ~0ull : __ballot(live)) & ~hits[0], f1 = (WHOLE ? ~0ull : __ballot(two)) & ~hits[1];
        unsigned* const rgc = sm.rgc[rb];
        pocs_pair_regions_masks(xs, ys, ts, &sm.rgh[0], &sm.rgh[POCS_MAX_REGIONS * POCS_OBS_STRIDE], a.reg_G, rgkeep, s_tab, vc,
                                [&](const int g, const unsigned long long m0, const unsigned long long m1) {
          const unsigned n = (unsigned)__popcll(m0 & f0) + (unsigned)__popcll(m1 & f1);      // (scalar)
          if (n != 0u && lane == 0) __hip_atomic_fetch_add(&rgc[g], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        });
      }
    }
    if constexpr (SG) {
      if (nkeeps != 0) {                                             // (scalar: at most waypoints of a plan nothing is near the way in)
        unsigned long long sub[2];
        pocs_pair_segment_masks(xs, ys, ts, -sg_u2, sg_u1, s_sgf, sgJ, 1, &fp, s_keeps, nkeeps, s_tab, vc, sub);
        const unsigned long long lm = WHOLE ? ~0ull : __ballot(live), tm = WHOLE ? ~0ull : __ballot(two);
        const unsigned n = (unsigned)__popcll(sub[0] & ~hits[0] & lm) + (unsigned)__popcll(sub[1] & ~hits[1] & tm);      // (scalar)
        if (n != 0u && lane == 0) __hip_atomic_fetch_add(&sm.sgc[rb], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        hits[0] |= sub[0]; hits[1] |= sub[1];
      }
    }
    if constexpr (POCS_TUNE_SKIP_MOMENTS) { POCS_TUNE_MOMENTS_ALT(); } else {
    // T1 sums over the collision-free samples of the component being accumulated:
    //   (x, y, t, x x, x y, x t, y y, y t, t t) with the products inside the fma; survivors by population count.
    if (WHOLE) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        nfree += __popcll(~hits[h]);                // every lane is live: the survivors are the mask's zero bits
        if (!__builtin_amdgcn_inverse_ballot_w64(hits[h])) {      // the few lanes that collided sit this out: exec from the mask
          const double x = xs[h], y = ys[h], t = ts[h];
          acc[0] += x; acc[1] += y; acc[2] += t;
          acc[3] = fma(x, x, acc[3]); acc[4] = fma(x, y, acc[4]); acc[5] = fma(x, t, acc[5]);
          acc[6] = fma(y, y, acc[6]); acc[7] = fma(y, t, acc[7]); acc[8] = fma(t, t, acc[8]);
        }
      }
    } else {
      // The components present in the wave are visited in increasing order (scalar loop), the previous
      // component's chains being flushed first; with ind = 1.0 for a surviving sample of the component and
      // 0.0 otherwise, (xm, ym, tm) = ind * (x, y, t) enter the sums -- a sample that does not count adds +-0
      // to every one of them, which is why the WHOLE form above gives the same bits.
      // Sample indices grow with the lane: the wave's first LIVE lane holds its first component, lane 63 its last.
      const unsigned long long live_mask = __ballot(live);
      const int klo = live_mask ? __builtin_amdgcn_readlane(ks[0], (int)__builtin_ctzll(live_mask)) : K;
      const int khi = __ballot(two) == ~0ull ? __builtin_amdgcn_readlane(ks[1], 63) : K - 1;
#pragma unroll
      for (int kk = 0; kk < K; ++kk) {
        if (kk < klo || kk > khi) continue;                                 // scalar compares
        if (kk != kcur) { flush_unit(sm, wave, lane, rb, tl, kcur, first, acc, nfree); kcur = kk; }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const bool sel = (h == 0 ? live : two) && ks[h] == kk;
          const bool cnt = sel && !__builtin_amdgcn_inverse_ballot_w64(hits[h]);
          nfree += __popcll(__ballot(cnt));
          const double ind = cnt ? 1.0 : 0.0;
          const double xm = ind * xs[h], ym = ind * ys[h], tm = ind * ts[h];
          acc[0] += xm; acc[1] += ym; acc[2] += tm;
          acc[3] = fma(xm, xs[h], acc[3]); acc[4] = fma(xm, ys[h], acc[4]); acc[5] = fma(xm, ts[h], acc[5]);
          acc[6] = fma(ym, ys[h], acc[6]); acc[7] = fma(ym, ts[h], acc[7]); acc[8] = fma(tm, ts[h], acc[8]);
        }
      }
    }
    }
    // (RH: the hypotheses forms read the launch's own word -- a scalar branch per iteration -- so that the family is instantiated
    // once per K and not twice: the build's time, not the call's, is what that saves.  Every other form folds STORE as it did.)
    if ((RH ? a.store != 0 : STORE) && live) {
      // Both poses of the pair leave together.  For the last sample of an odd shard the second slot is
      // the pair's unused twin: it lands in the padding element of the run's slice (sample_stride >=
      // count + 1 then) and is never read back.  Written once, never re-read by the kernels: non-temporal,
      // past the caches.  The loop counter is wave-uniform (SGPRs) and the lane adds its tid: the store
      // addresses are a scalar base per iteration plus a constant 16*tid, no per-lane 64-bit arithmetic.
      const size_t ub = 2 * (size_t)(unsigned)base;
      const int fl = (__builtin_amdgcn_inverse_ballot_w64(hits[0]) ? 1 : 0) |
                     ((two && __builtin_amdgcn_inverse_ballot_w64(hits[1])) ? 0x10000 : 0);      // selects on the masks
      store16_nt(xr + ub, 16u * (unsigned)tid, (v2d){xs[0], xs[1]});
      store16_nt(yr + ub, 16u * (unsigned)tid, (v2d){ys[0], ys[1]});
      store16_nt(tr + ub, 16u * (unsigned)tid, (v2d){ts[0], ts[1]});
      store4_nt(fr + ub, 4u * (unsigned)tid, fl);
    }
  };

  // the component block the wave's local sample l0 lies in, and where whole waves of it end
  auto lookup = [&](const int l0) __attribute__((always_inline)) {
    const double g0 = first_d + (double)l0;
    int kk = 0;
#pragma unroll
    for (int q = 0; q < K - 1; ++q) kk += (cumn[q] <= g0) ? 1 : 0;
    kw = __builtin_amdgcn_readfirstlane(kk);
    double e = (double)count;
    if (kw < K - 1) e = fmin(e, s_par[kw * POCS_PARAM_STRIDE + 9] - first_d);      // exact: integers below 2^53
    seg_end = __builtin_amdgcn_readfirstlane((int)e);
  };
  for (int t = ta; t < tb; ++t) {
    const int tl = t - ta;
    const int r = t >> a.vs_shift, j = t & vs_mask;
    if (r - r0 != rb) {                              // (scalar) the block's first unit, or its range enters run r0 + 1
      rb = r - r0;
      s_par = sm.par[rb]; s_keep = sm.keep[rb];
      nkeep = __builtin_amdgcn_readfirstlane(sm.nkeep[rb]);
      if constexpr (CL) { s_keep2 = sm.keep2[rb]; nkeep2 = __builtin_amdgcn_readfirstlane(sm.nkeep2[rb]); }
      if constexpr (RG) rgkeep = (unsigned)__builtin_amdgcn_readfirstlane((int)sm.rgk[rb]);
      if constexpr (SG) {
        s_keeps = sm.keeps[rb]; s_sgf = sm.sgf[rb];
        nkeeps = __builtin_amdgcn_readfirstlane(sm.nkeeps[rb]); sgJ = __builtin_amdgcn_readfirstlane(sm.sgJ[rb]);
        sg_u1 = pocs_wave_uniform_f64(sm.sgu[rb][1]); sg_u2 = pocs_wave_uniform_f64(sm.sgu[rb][2]);
      }
      seed = (uint64_t)uniform64((long long)sm.seed[rb]);         // scalar registers, provably
#pragma unroll
      for (int q = 0; q < K - 1; ++q) cumn[q] = s_par[q * POCS_PARAM_STRIDE + 9];
      // (Keeping the wave's component parameters in scalar registers instead of reading them at one LDS
      // address spills scalar registers: measured 5 % slower at K = 3.)
      xr = a.x + (size_t)r * a.sample_stride;          // this run's slice (sample_stride is even)
      yr = a.y + (size_t)r * a.sample_stride;
      tr = a.th + (size_t)r * a.sample_stride;
      fr = a.flags + (size_t)r * a.sample_stride;
      seg_end = 0;                                     // nothing known about this run's component blocks yet
    }
    // chunks [c_begin, c_end) of virtual slice j: a fixed cut of the run's chunks into VS = 2^vs_shift ranges
    const int c_begin = (int)(((long long)j * a.chunks) >> a.vs_shift);
    const int c_end = (int)(((long long)(j + 1) * a.chunks) >> a.vs_shift);
    bool first = true;                               // (scalar) nothing of this unit has been flushed yet
    it_unit = (t == ta) ? 0 : npre;                  // (lone form) normals drawn ahead exist for the first unit held only
    // A wave's samples only move forward within a run, so the component block found for an earlier unit still
    // holds while the wave's 128 samples end before seg_end; it is looked up again (a few vector compares)
    // only when they do not: at a block boundary, at the shard's end.
    const int end = c_end * TB;
    int base = c_begin * TB;
    if (2 * base + wave_first + 128 > seg_end) lookup(2 * base + wave_first);
    kcur = kw;                                       // the component the wave's first sample of the unit belongs to
    // A wave's 128 samples of an iteration nearly always lie inside ONE component block and inside the shard:
    // those iterations run in the inner loop below, which knows nothing of the general case (no per-lane
    // index compares, no masks, no flush; the accumulators stay where they are).
    while (base < end) {
      int l0 = 2 * base + wave_first;                                        // local index of the wave's first sample
      if (l0 + 128 > seg_end) lookup(l0);
      if (l0 + 128 <= seg_end) {
        if (kw != kcur) { flush_unit(sm, wave, lane, rb, tl, kcur, first, acc, nfree); kcur = kw; }
        do {
          iteration(std::true_type{}, base, tl, first);
          base += TB;
          l0 += 2 * TB;
        } while (base < end && l0 + 128 <= seg_end);
      } else {
        iteration(std::false_type{}, base, tl, first);
        base += TB;
      }
    }
    __builtin_amdgcn_s_setprio(3);                   // flushes run at the top priority: other waves will wait for them
    flush_unit(sm, wave, lane, rb, tl, kcur, first, acc, nfree);      // the unit's last component
  }
}

// The rows of the held units [ta, tb): column c of (virtual slice, component) = the eight wave sums in wave
// order -- whichever of them the unit has: slot if the component was the wave's first there, xtra if it
// started inside the wave's share, +0 otherwise -- stored write-through to the run's partial rows.
// Column 1 (collisions) stays 0: a component's collisions are what is left of its block (gmm_close_sums).
template <int K, int TB, bool OC, bool CL, bool FPN, bool RG, bool SG>
__device__ __forceinline__ void gmm_emit_rows(const pocs_gmm_launch& a, gmm_smem<K, TB, OC, CL, FPN, RG, SG>& sm, const int r0, const int ta, const int tb) {
  constexpr int NC = K * POCS_NMOM, NW = TB / 64;
  for (int i = threadIdx.x; i < (tb - ta) * NC; i += TB) {
    const int tl = i / NC, c = i - tl * NC, k = c / POCS_NMOM, col = c - k * POCS_NMOM;
    const int rb = ((ta + tl) >> a.vs_shift) - r0;
    double v = 0.0;
    if (col != 1) {
      const int s = col == 0 ? 0 : col - 1;
      // the eight waves' terms are fetched side by side (both candidates of each: one LDS round trip), then added in wave order
      double ps[NW], px[NW];
      int kf[NW], xj[NW];
#pragma unroll
      for (int u = 0; u < NW; ++u) { kf[u] = sm.kf[tl][u]; xj[u] = sm.xj[rb][u][k]; ps[u] = sm.slot[tl][u][s]; px[u] = sm.xtra[rb][u][k][s]; }
#pragma unroll
      for (int u = 0; u < NW; ++u) {
        const double p = kf[u] == k ? ps[u] : (xj[u] == tl ? px[u] : 0.0);
        v = (u == 0) ? p : v + p;
      }
    }
    store_wt(&a.partial[(size_t)(ta + tl) * NC + c], v);        // [run][VS][NC] = [unit][NC]
  }
}

// The closer of (r, w) -- the block that drew the run's last ticket, behind its acquire -- adds the VS
// partial rows of the run in a FIXED order that does not depend on who adds them: sixteen interleaved
// partial sums per column, P_g = row g + row (g + 16) + row (g + 32) + ... in that order, then
// P_0 + P_1 + ... + P_15 in that order.  Every (g, column) is one work item: its loads are L1-bypassing
// and independent, so the block has the whole table in flight at once -- ONE memory round trip.
// `stage`: >= 16 * NC doubles of LDS.  The collisions of a component are what is left of its block of
// this shard's samples: nColl_k = n_k - nFree_k, with [cum_{k-1}, cum_k) the component's global sample
// range (par[k][9], cum_{K-1} = n_total).  Result: tot[c], and moments[w][r][c] in global memory (it
// leaves the launch at the kernel boundary).
// The rows of ONE batch of work items (two per thread, starting at item i0): request() issues every load, reduce() adds
// them in row order into the staging rows.  A caller with other requests to make (the lone form's heads; the closer, whose
// mixture advance wants state[w] and the chain record) issues the first batch itself, next to them.
template <int K, int NT>
struct close_rows {
  static constexpr int NC = K * POCS_NMOM, G = 16, ITEMS = G * NC, RPI = POCS_GMM_MAX_VS / G;
  double v[2][RPI];
  __device__ __forceinline__ void request(const double* src, const int S, const int i0) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int i = i0 + t * NT, g = i / NC, c = i - g * NC;
#pragma unroll
      for (int u = 0; u < RPI; ++u) {
        const int q = g + u * G;
        v[t][u] = (i < ITEMS && q < S) ? load_wt(&src[(size_t)q * NC + c]) : 0.0;
      }
    }
  }
  // every value passes through an (empty) asm statement: the additions of reduce() cannot rise above it into the branches
  // of the loads -- where the compiler, left to itself, puts an item's first one, with a wait for that load in front of
  // all the others
  __device__ __forceinline__ void pin() {
    static_assert(RPI % 4 == 0, "four values per statement");
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < RPI; u += 4) asm volatile("" : "+v"(v[t][u]), "+v"(v[t][u + 1]), "+v"(v[t][u + 2]), "+v"(v[t][u + 3]));
  }
  __device__ __forceinline__ void reduce(double* stage, const int S, const int i0) const {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int i = i0 + t * NT, g = i / NC;
      double sum = 0.0;
#pragma unroll
      for (int u = 0; u < RPI; ++u) if (g + u * G < S) sum += v[t][u];
      if (i < ITEMS) stage[i] = sum;
    }
  }
};
template <int K>
__device__ __forceinline__ const double* close_rows_of(const pocs_gmm_launch& a, const double* rows, const int r) {
  return rows + (size_t)r * (1 << a.vs_shift) * (K * POCS_NMOM);
}
//   REQUESTED: the caller has issued the first batch (items tid, tid + NT) into `cr` already
template <int K, int NT, bool REQUESTED = false>
__device__ __forceinline__ void gmm_close_sums(const pocs_gmm_launch& a, const int w, const int r, const double* s_par,
                                               double* stage, double* tot, const int tid,
                                               const double* rows, const bool store, close_rows<K, NT>& cr) {
  constexpr int NC = K * POCS_NMOM, G = 16, ITEMS = G * NC, nthreads = NT;
  const int S = 1 << a.vs_shift;
  const double* src = close_rows_of<K>(a, rows, r);
  // An item's (up to) sixteen rows g, g + 16, ... are all requested before the first is waited for, and so are the
  // rows of the thread's NEXT item where there are more items than threads (K = 3: 528 items on 512 threads --
  // taken one after the other, sixteen threads cost the whole block a second memory round trip): two items per
  // batch, ONE round trip per batch for the run's 256 rows.  Added in row order.  (requests_issued() between the two
  // steps: left to itself the compiler folds an item's first addition into the branch of its first load and waits
  // there -- three round trips per batch instead of one.)
  for (int i0 = tid; i0 < ITEMS; i0 += 2 * NT) {
    if (!(REQUESTED && i0 == tid)) cr.request(src, S, i0);
    requests_issued();
    cr.pin();
    cr.reduce(stage, S, i0);
  }
  __syncthreads();
  for (int c = tid; c < NC; c += nthreads) {
    double v = stage[c];
    const int ng = S < G ? S : G;
    for (int g = 1; g < ng; ++g) v += stage[g * NC + c];
    tot[c] = v;
  }
  __syncthreads();
  const double lo = (double)a.first, hi = (double)(a.first + a.count);
  for (int k = tid; k < K; k += nthreads) {
    const double c0 = (k == 0) ? 0.0 : s_par[(k - 1) * POCS_PARAM_STRIDE + 9];
    const double c1 = (k == K - 1) ? (double)a.n_total : s_par[k * POCS_PARAM_STRIDE + 9];
    const double n_k = fmax(0.0, fmin(c1, hi) - fmax(c0, lo));
    tot[k * POCS_NMOM + 1] = n_k - tot[k * POCS_NMOM];
  }
  __syncthreads();
  if (store) for (int c = tid; c < NC; c += nthreads) a.moments[((size_t)w * a.nruns + r) * NC + c] = tot[c];
}

// One waypoint of runs [run_lo, run_lo + run_cnt) of the call as ONE launch (the host issues a call's runs as
// one launch per waypoint, or as two half-batches on two streams whose launches overlap, pocs_host.hip).
// The launch's work is the flat list of UNITS t = r * VS + j (virtual slice j of run r); block b takes the
// b-th `upb` of them -- every block
// the same number, whatever the number of runs, which is what lets a launch of ANY number of runs fill
// the 512 resident blocks evenly.  A block's range may cross from one run into the next (never further:
// upb <= VS).
//   head  log / sector tables, the obstacle table, the sampler parameters of the block's (up to) two
//         runs -> LDS; exact culling of the obstacle table per run (waves 0 and 1);
//   body  gmm_units, POCS_GMM_SUB units at a time, each followed by the rows of those units -> the
//         write-through partial rows [run][VS];
//   tail  every storing wave drains -> the block meets -> one ticket per run it touched; the block that
//         draws a run's last ticket acquires, adds the run's VS rows and (one GPU) advances the mixture
//         to the next waypoint -- sharded: after exchanging the run's moments with the other ranks.
//
// LONE (one run per call, no batch, no run-ahead): nothing else is in flight to hide a closer behind, and the
// tickets' two round trips (drain the rows, draw the ticket) and the closer's acquire are pure latency.  The
// launch of waypoint w then closes waypoint w - 1 ITSELF, in the head of EVERY block: the rows of w - 1 (the
// other half of the row buffer: a fast block must not overwrite what a slow one still reads), state[w-1] and
// the chain record arrive in one round trip behind the kernel boundary; every block adds the rows in the
// fixed order, advances the mixture -- 256 times the same few microseconds of one wave, on CUs that would
// otherwise wait for one of them to do it -- and keeps param[w] in LDS; block 0 writes moments[w-1], state[w],
// param[w] out for the getters.  The tail is the rows' stores and nothing else; a one-block launch
// (k_gmm_close) adds the last waypoint's rows.  Same functions, same order of additions: the same bits.
//
// RISK (a call of plans under a risk bound, pocs_set_plan_risk_bound; the kernel k_gmm_step_risk, never LONE): a run whose
// running probability 1 - prod_{v <= w} (1 - p_v) has reached the bound is not worked on any further.
//   deciding  the closer of (r, w) has the run's collision counts in LDS the moment it has added the rows: one lane forms p_w
//             and the survival product exactly as the host's combine does (plain / and *, this file is built without
//             contraction), keeps the product in surv[r] and, at the bound, publishes stop[r] = w + 1 and does not advance
//             the mixture (as for a plan that ends at w);
//   obeying   a head asks for the stop words of its (at most two) runs with its other requests -- the same round trip -- and
//             a block whose runs have all stopped returns behind it (nothing staged, no cull, no rows, no ticket); a block
//             that straddles a stopped and a live run narrows its range to the live run's units and takes that run's ticket
//             only.  Which blocks meet a run (b_first, b_last) does not change: a stopped run's tickets are never drawn, so
//             nobody closes it and nobody waits for it.
// No fence of its own: stop[r] and surv[r] are written by a closer of waypoint w's launch and read by waypoint w + 1's launch
// of the SAME sub-batch -- a run never changes sub-batch (plan_layout) --, i.e. behind a kernel boundary on one stream, as
// state / param[w + 1] are; write-through stores and L1-bypassing loads like those.
//
// TREE (a tree of plans, pocs_set_plan_tree; the kernel k_gmm_step_tree, ticket form, never LONE, nothing stored): the launch's
// "runs" are nodes of ONE level of the tree.  a.waypoint is the level's depth and keys the random draws, as a plan's waypoint
// does; the rows a node owns -- param, ticket, moments, and under RISK its stop word and survival product -- are addressed by
// its slot alone (the host lays them out [slot], i.e. W = 1, row 0).  The mixtures were built by k_gmm_tree_advance, which
// under RISK has also handed the parent's stop and survival product down: the heads and closers below do what they do for
// waypoint `depth` of a plan.
//
// OC (POCS_OPT_OBSTACLE_COUNTS; the kernels k_gmm_step_boxes, k_gmm_step_risk_boxes, k_gmm_step_tree_boxes): the block also counts,
// per run buffer and kept obstacle record, its samples that touch the record (gmm_units), in LDS counters that gmm_cull zeroes;
// behind the units the nonzero ones leave with one integer atomic each to obs_counts[run][waypoint][the record's index in the
// caller's table] -- exact whatever the grid.  A stopped run's blocks add nothing; the table is the shard's, the exchange does
// not carry it.
//
// WORLD (a large collision world, pocs_set_world; the kernels k_gmm_step_world, k_gmm_step_risk_world: ticket form, never LONE, TREE
// or OC): there is no table to stage and to cull -- k_world_cull, the launch in front of this one, has left the records in reach of
// every run of the launch in a.kept and their number in a.reach.  The head asks for the (up to) two runs' records and counts with
// its other requests, the same single round trip, and commits min(reach, POCS_MAX_OBSTACLES) records to sm.keep[rb] -- what gmm_cull
// leaves there otherwise.  The body does not know the difference.
//
// CL (clearance levels, pocs_set_clearance_levels; the kernels k_gmm_step_clear, k_gmm_step_risk_clear: ticket form, never LONE, TREE,
// OC or WORLD): the head also stages the table prepared for the footprint grown by the largest clearance (behind the base table in
// the transpose scratch) and the head of the waypoint's pocs_clear_dev, with its other requests; waves 2 and 3 cull that table
// beside waves 0 and 1 (gmm_cull_clear); the body counts per level (gmm_units); behind the units the nonzero counters leave with
// one integer atomic each to clr_counts[run][waypoint][level], as occ does.  The base test, the moment sums, the tickets and the
// closers are what they are.  LDS: + 8 KB for the second kept table, + 0.1 KB, and 24 instead of 32 held units (- 5.25 KB): K = 3 holds
// 70 688 B against the twin's 67 744, K = 8 78 368 B against 75 424 -- two blocks per CU (160 KB) in every instantiation, as the twins.
//
// FPN (a compound footprint, pocs_set_footprint_parts with F > 1; the kernels k_gmm_step_parts, k_gmm_step_risk_parts: ticket form,
// never LONE, TREE, OC, WORLD or CL): the head also stages the parts (pocs_parts_dev) with its other requests; waves 0 and 1 cull with
// gmm_cull_parts in place of gmm_cull -- ONE kept list per run buffer, a record kept if any part's keep test passes, its broad-phase
// fields the largest of the parts' -- and the body asks pocs_pair_parts_masks.  The moment sums, the tickets and the closers are what
// they are.  LDS: + 192 B for the parts (K = 8: 75 616 B against the twin's 75 424): two blocks per CU in every instantiation.
//
// RG (watched regions, pocs_set_regions; the kernels k_gmm_step_regions, k_gmm_step_risk_regions: ticket form, never LONE, TREE, OC,
// WORLD, CL or FPN): the head also stages the regions' records and footprints (the head of pocs_regions_dev) with its other requests;
// waves 2 and 3 decide per run buffer which regions the run's mixture can reach (gmm_cull_regions) beside waves 0 and 1; the body
// counts per kept region the collision-free samples in it (gmm_units); behind the units the nonzero counters leave with one integer
// atomic each to reg_counts[run][waypoint][region], as clc does.  The collision test, the moment sums, the tickets and the closers
// are what they are.  LDS: + 432 B (K = 8: 75 856 B against the twin's 75 424): two blocks per CU in every instantiation.
//
// SG (segment checks, pocs_set_segment_checks with J > 1; the kernels k_gmm_step_seg, k_gmm_step_risk_seg: ticket form, never LONE, TREE,
// OC, WORLD, CL, FPN or RG): waves 2 and 3 build per run buffer the second kept list -- the records in reach of the run's whole way
// in (gmm_cull_seg, which also stages J, the fractions and the run's applied control) -- beside waves 0 and 1; the body tests the
// sub-poses of the samples where that list is not empty and ors their flags in (gmm_units); behind the units the nonzero counters
// leave with one integer atomic each to seg_counts[run][waypoint], as clc does.  The samples' own test, the moment sums (formed from
// the or-ed flags), the tickets and the closers are what they are.  LDS: + 8 KB for the second kept table, + 0.3 KB, and 24 instead of
// 32 held units, as the clearance form: two blocks per CU in every instantiation.
template <int K, bool STORE, int TB, bool LONE, bool RISK, bool TREE = false, bool OC = false, bool WORLD = false, bool CL = false, bool FPN = false,
          bool RG = false, bool SG = false, bool RD = false, bool RN = false, bool RF = false, bool RH = false>
__device__ __forceinline__ void gmm_step_block(const pocs_gmm_launch a) {      // (by value, as a kernel holds its argument)
  typedef gmm_smem<K, TB, OC, CL, FPN, RG, SG> smem_t;
  static_assert(!RN || RD || RF, "uncertain discs: on top of the round form");
  static_assert(!(RF && (RD || LONE || TREE || OC || WORLD || CL || FPN || RG || SG)), "a round footprint: the ticket form of a batch or of plans on a small world, no counts, no segment checks");
  static_assert(!(RD && (LONE || TREE || OC || WORLD || CL || FPN || RG || SG)), "round obstacles: the ticket form of a batch or of plans on a small world, a single footprint box, no counts, no segment checks");
  static_assert(!(SG && (LONE || TREE || OC || WORLD || CL || FPN || RG)), "segment checks: the ticket form of a batch or of plans on a small world, a single footprint box, no other counts");
  static_assert(!SG || TB >= 256, "waves 2 and 3 build the second kept list");
  static_assert(!(RG && (LONE || TREE || OC || WORLD || CL || FPN)), "watched regions: the ticket form of a batch or of plans on a small world, no other counts");
  static_assert(!RG || TB >= 256, "waves 2 and 3 decide the regions in reach");
  static_assert(!(FPN && (LONE || TREE || OC || WORLD || CL)), "a compound footprint: the ticket form of a batch or of plans on a small world, no counts per box or level");
  static_assert(!(CL && (LONE || TREE || OC || WORLD)), "clearance levels: the ticket form of a batch or of plans on a small world, no per-box counts");
  static_assert(!(WORLD && (LONE || TREE || OC)), "a large world: the ticket form of a batch or of plans, no per-box counts");
  static_assert(!WORLD || TB == POCS_MAX_OBSTACLES * POCS_OBS_STRIDE, "one element of a run's kept records per thread");
  static_assert(!(LONE && RISK), "the lone form closes in its heads: a call under a risk bound takes the ticket form");
  static_assert(!(TREE && (LONE || STORE)), "a tree's levels take the ticket form and store no samples");
  constexpr int SUB = smem_t::SUB, NW = smem_t::NW;
  // (the block's LDS, declared here and not handed in by the kernel: every instantiation is inlined into exactly one kernel,
  // and the accesses stay LDS accesses from the front end on)
  __shared__ smem_t sm;
  // (lone form: one block per CU, the whole LDS is its own) the normals of the unit's first POCS_LONE_PRE iterations
  __shared__ double s_zpre[LONE ? POCS_LONE_PRE * 6 * TB : 2];
  // (RN: the kept records' noise rows per run buffer, 4 KB next to the kept lists: with the _round form's 75 424 B, 79 520 B of the
  // 81 920 B that let two blocks share a CU, for every K.  No other form holds a byte of it.)
  // (RH: their gates behind them, 2 KB more: 81 568 B at K = 8, still under the 81 920 B)
  static_assert(!RH || (RD && RN && !RF), "hypotheses: on top of the noise form, a footprint box");
  double* const s_nz = gmm_noise_rows<RN, RH>::get();
  int npre = 0;
  const int tid = threadIdx.x;
  const int w = a.waypoint;
  const int wr = TREE ? 0 : w;                       // the row of (run, waypoint) in the run's [W] arrays; a tree: one row per node
  const int t_lo = a.run_lo << a.vs_shift, t_hi = (a.run_lo + a.run_cnt) << a.vs_shift;    // this launch's units
  const int bx = (int)blockIdx.x;
  const int t0_all = t_lo + bx * a.upb;
  const int t1_all = (t0_all + a.upb < t_hi) ? t0_all + a.upb : t_hi;
  const int r0_all = t0_all >> a.vs_shift, r1_all = (t1_all - 1) >> a.vs_shift;       // the block's first and last run (r1 <= r0 + 1)
  // (RISK: narrowed below to the block's live run where the other one has stopped; otherwise these ARE the block's range)
  int t0 = t0_all, t1 = t1_all, r0 = r0_all, r1 = r1_all;
  POCS_STAMP_BEGIN();
  // The head's inputs are all REQUESTED before the first of them is waited for: the tables (24 bytes per thread), and per
  // form what follows -- one memory round trip for the lot, then the stores to LDS.
  constexpr int PS = K * POCS_PARAM_STRIDE;
  static_assert(POCS_MAX_OBSTACLES * POCS_OBS_STRIDE <= TB, "one obstacle element per thread");
  static_assert(2 * PS <= TB, "one sampler parameter per thread (two runs)");
  static_assert(POCS_ADV_STAGE_MAX <= 4 * TB, "the advance's inputs in one batch");
  double tabv[table_regs<TB>::N];
  request_tables<TB>(a.tables, tid, tabv);
  double obs_elem = 0.0;
  if constexpr (!WORLD) obs_elem = tid < a.M * POCS_OBS_STRIDE ? a.env->obs[tid] : 0.0;
  [[maybe_unused]] double fpp_elem = 0.0;                       // FPN: the parts
  if constexpr (FPN) fpp_elem = tid < POCS_MAX_FOOTPRINT_PARTS * POCS_PART_STRIDE ? a.parts->part[tid] : 0.0;
  [[maybe_unused]] double obs2_elem = 0.0, clh_elem = 0.0;      // CL: the grown footprint's table, the head of the clearance record
  if constexpr (CL) {
    obs2_elem = tid < a.M * POCS_OBS_STRIDE ? a.clr->obs[tid] : 0.0;
    clh_elem = tid < 6 + POCS_MAX_CLEARANCE_LEVELS ? reinterpret_cast<const double*>(a.clr)[tid] : 0.0;
  }
  [[maybe_unused]] double rgh_elem = 0.0;                       // RG: the regions' records and footprints
  if constexpr (RG) rgh_elem = tid < POCS_REGIONS_HEAD ? reinterpret_cast<const double*>(a.regions)[tid] : 0.0;
  if (LONE && w > 0) {
    // close waypoint w - 1 and advance to w, here (r0 is the call's one run)
    const bool out = blockIdx.x == 0;
    const adv_ptrs ap = advance_ptrs(a, K, w, r0, sm.adv());
    double advv[4];
    advance_request(ap, false, tid, TB, advv);                                             // state[w-1], chain record, sensor (the moments come from the rows)
    const double parv = tid < PS ? a.param[((size_t)r0 * a.W + (w - 1)) * PS + tid] : 0.0;   // (the counts of w - 1)
    const unsigned long long seedv = a.hdr[r0].seed;
    close_rows<K, TB> cr;
    cr.request(close_rows_of<K>(a, a.partial_prev, r0), 1 << a.vs_shift, tid);             // the rows of w - 1
    requests_issued();
    commit_tables<TB>(&sm.tab, tid, tabv);
    advance_commit(ap, false, tid, TB, advv);
    if (tid < PS) sm.par[1][tid] = parv;
    for (int j = tid; j < 2 * NW * K; j += TB) (&sm.xj[0][0][0])[j] = -1;
    if (tid == 0) sm.seed[0] = seedv;
    double* const l_mom = ap.l_mom;
    // (the obstacle table, one element per thread, requested with everything else: it lands in the transpose scratch as soon
    // as the row sums are done with it, under the components' serial chain instead of in a round trip of its own behind it)
    gmm_close_sums<K, TB, true>(a, w - 1, r0, sm.par[1], sm.stage(), l_mom, tid, a.partial_prev, out, cr);
    POCS_STAMP(5);
    if (tid < a.M * POCS_OBS_STRIDE) sm.obs()[tid] = obs_elem;      // (every read of the staging rows lies behind a barrier of gmm_close_sums)
    // While wave 0 walks the components' serial chain and a lane of wave 1 draws the counts, the other six waves draw
    // the normals of the block's first unit -- they do not depend on the mixture -- for all 512 threads and the unit's
    // first iterations: (seed, pair index, waypoint) -> six normals, the arguments the sampling loop would use.
    const int j0 = t0 & ((1 << a.vs_shift) - 1);
    const int cb0 = (int)(((long long)j0 * a.chunks) >> a.vs_shift), ce0 = (int)(((long long)(j0 + 1) * a.chunks) >> a.vs_shift);
    npre = (ce0 - cb0) < POCS_LONE_PRE ? (ce0 - cb0) : POCS_LONE_PRE;
    auto draw_ahead = [&]() __attribute__((always_inline)) {
      POCS_VCONST(vc_);
      const uint64_t seed = seedv;                          // (requested with the head's other inputs)
      const uint64_t pair0 = (uint64_t)(a.first >> 1);
      for (int it = 0; it < npre; ++it)
        for (int l = tid - 128; l < TB; l += TB - 128) {
          double za[3], zb[3];
          uint32_t sa, sb;
          pocs_normal3_pair(seed, pair0 + (uint64_t)(unsigned)((cb0 + it) * TB + l), (uint32_t)w, POCS_STREAM_GMM, &sm.tab, za, zb, &sa, &sb, &vc_);
          double* z = s_zpre + (size_t)it * 6 * TB + l;
#pragma unroll
          for (int q = 0; q < 3; ++q) { z[q * TB] = za[q]; z[(3 + q) * TB] = zb[q]; }
        }
    };
    // (the cull of the obstacle table against the mixture of waypoint w -- means and factors only -- by wave 1, beside wave 0's
    // normalisation and publishing instead of behind them and a barrier)
    auto cull_early = [&]() __attribute__((always_inline)) { gmm_cull(a, sm, 0, tid - 64, ap.l_par); };
    if (tid < 128) __builtin_amdgcn_s_setprio(3);          // the components' chain and the count lane go first on their SIMDs; the drawing waves fill in
    advance_block(a, K, w, r0, sm.adv(), sm.spec(), true, tid, TB, true, out, draw_ahead, cull_early);
    if (tid < 128) __builtin_amdgcn_s_setprio(0);
    __syncthreads();
    POCS_STAMP(6);
    POCS_STAMP_COUNT(14);
    const double* const l_par = advance_ptrs(a, K, w, r0, sm.adv()).l_par;
    for (int j = tid; j < PS; j += TB) sm.par[0][j] = l_par[j];
  } else {
    // param[r][w][..]: the two runs' records are a.W records apart
    const int rp = tid / PS, jp = tid - rp * PS;
    const double parv = tid < (r1 - r0 + 1) * PS ? load_wt(&a.param[((size_t)(r0 + rp) * a.W + wr) * PS + jp]) : 0.0;
    const unsigned long long seedv = tid <= r1 - r0 ? a.hdr[r0 + tid].seed : 0ull;
    // WORLD: element `tid` of the kept records of the block's first and second run (a block of one run asks for its records twice)
    // and the two counts; `shift` as below: a live second run whose first has stopped lands in buffer 0
    double keptv[2] = {0.0, 0.0};
    int reachv[2] = {0, 0};
    if constexpr (WORLD) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int rq = r0_all + q <= r1_all ? r0_all + q : r1_all;
        keptv[q] = load_wt(&a.kept[(size_t)rq * (POCS_MAX_OBSTACLES * POCS_OBS_STRIDE) + tid]);
        reachv[q] = __hip_atomic_load(&a.reach[(size_t)rq * a.W + wr], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    auto commit_world = [&](const int shift) __attribute__((always_inline)) {
      if constexpr (WORLD) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int rb = q - shift;
          if (q <= r1_all - r0_all && rb >= 0 && rb <= r1 - r0) {
            const int n = reachv[q] < POCS_MAX_OBSTACLES ? reachv[q] : POCS_MAX_OBSTACLES;      // (an overflow fails the call on the host; nothing is read past the 64)
            if (tid < n * POCS_OBS_STRIDE) sm.keep[rb][tid] = keptv[q];
            if (tid == 0) sm.nkeep[rb] = n;
          }
        }
      }
    };
    if constexpr (RISK) {
      // the stop words of the block's runs, every lane the same two addresses, in flight with everything above (a stopped run's
      // param[w] was never built: what was requested of it is dropped below, unread)
      const unsigned s0 = __hip_atomic_load(&a.stop[r0_all], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned s1 = __hip_atomic_load(&a.stop[r1_all], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      requests_issued();
      const bool dead0 = __builtin_amdgcn_readfirstlane((int)s0) != 0, dead1 = __builtin_amdgcn_readfirstlane((int)s1) != 0;
      if (dead0 && dead1) return;                      // (one run: both words are its word) nothing left to do for this block
      int shift = 0;                                   // the live run's requests land in buffer 0
      if (dead0) { shift = 1; r0 = r1_all; t0 = r1_all << a.vs_shift; }
      else if (dead1) { r1 = r0_all; t1 = r1_all << a.vs_shift; }
      commit_tables<TB>(&sm.tab, tid, tabv);
      if (tid < a.M * POCS_OBS_STRIDE) sm.obs()[tid] = obs_elem;
      if constexpr (CL) { if (tid < a.M * POCS_OBS_STRIDE) sm.obs2()[tid] = obs2_elem; if (tid < 6 + POCS_MAX_CLEARANCE_LEVELS) sm.clh[tid] = clh_elem; }
      if constexpr (FPN) { if (tid < POCS_MAX_FOOTPRINT_PARTS * POCS_PART_STRIDE) sm.fpp[tid] = fpp_elem; }
      if constexpr (RG) { if (tid < POCS_REGIONS_HEAD) sm.rgh[tid] = rgh_elem; }
      if (tid < (r1_all - r0_all + 1) * PS && rp >= shift && rp - shift <= r1 - r0) sm.par[rp - shift][jp] = parv;
      for (int j = tid; j < 2 * NW * K; j += TB) (&sm.xj[0][0][0])[j] = -1;
      if (tid <= r1_all - r0_all && tid >= shift && tid - shift <= r1 - r0) sm.seed[tid - shift] = seedv;
      commit_world(shift);
    } else {
    requests_issued();
    commit_tables<TB>(&sm.tab, tid, tabv);
    if (tid < a.M * POCS_OBS_STRIDE) sm.obs()[tid] = obs_elem;
    if constexpr (CL) { if (tid < a.M * POCS_OBS_STRIDE) sm.obs2()[tid] = obs2_elem; if (tid < 6 + POCS_MAX_CLEARANCE_LEVELS) sm.clh[tid] = clh_elem; }
      if constexpr (FPN) { if (tid < POCS_MAX_FOOTPRINT_PARTS * POCS_PART_STRIDE) sm.fpp[tid] = fpp_elem; }
    if constexpr (RG) { if (tid < POCS_REGIONS_HEAD) sm.rgh[tid] = rgh_elem; }
    if (tid < (r1 - r0 + 1) * PS) sm.par[rp][jp] = parv;
    for (int j = tid; j < 2 * NW * K; j += TB) (&sm.xj[0][0][0])[j] = -1;
    if (tid <= r1 - r0) sm.seed[tid] = seedv;
    commit_world(0);
    }
  }
  __syncthreads();
  if constexpr (!WORLD) {
  if (!(LONE && w > 0)) {                            // (scalar; the lone form's heads have culled already, above)
    if constexpr (CL) {
      if (tid >= 128 && tid < 192) gmm_cull_clear(a, sm, 0, tid - 128, sm.par[0]);
      else if (tid >= 192 && tid < 256 && r1 > r0) gmm_cull_clear(a, sm, 1, tid - 192, sm.par[1]);
    }
    if constexpr (RG) {
      if (tid >= 128 && tid < 192) gmm_cull_regions(a, sm, 0, tid - 128, sm.par[0]);
      else if (tid >= 192 && tid < 256 && r1 > r0) gmm_cull_regions(a, sm, 1, tid - 192, sm.par[1]);
    }
    if constexpr (SG) {
      if (tid >= 128 && tid < 192) gmm_cull_seg(a, sm, 0, tid - 128, sm.par[0], r0);
      else if (tid >= 192 && tid < 256 && r1 > r0) gmm_cull_seg(a, sm, 1, tid - 192, sm.par[1], r0 + 1);
    }
    if constexpr (FPN) {
      if (tid < 64) gmm_cull_parts(a, sm, 0, tid, sm.par[0]);
      else if (tid < 128 && r1 > r0) gmm_cull_parts(a, sm, 1, tid - 64, sm.par[1]);
    } else if constexpr (RF) {
      if (tid < 64) gmm_cull_rfoot<RN>(a, sm, 0, tid, sm.par[0], s_nz);
      else if (tid < 128 && r1 > r0) gmm_cull_rfoot<RN>(a, sm, 1, tid - 64, sm.par[1], s_nz);
    } else if constexpr (RN) {
      if (tid < 64) gmm_cull<true, RH>(a, sm, 0, tid, sm.par[0], s_nz);
      else if (tid < 128 && r1 > r0) gmm_cull<true, RH>(a, sm, 1, tid - 64, sm.par[1], s_nz);
    } else {
    if (tid < 64) gmm_cull(a, sm, 0, tid, sm.par[0]);
    else if (tid < 128 && r1 > r0) gmm_cull(a, sm, 1, tid - 64, sm.par[1]);
    }
    __syncthreads();
  }                                                  // from here on the transpose scratch is the waves'
  }
  POCS_STAMP(0);
  for (int ta = t0; ta < t1; ta += SUB) {
    const int tb = (ta + SUB < t1) ? ta + SUB : t1;
    if constexpr (RF) gmm_units<K, STORE, TB, LONE, OC, CL, FPN, RG, SG, false, RN, true>(a, sm, w, r0, ta, tb, s_zpre, ta == t0 ? npre : 0, s_nz);
    else
    if constexpr (RN) gmm_units<K, STORE, TB, LONE, OC, CL, FPN, RG, SG, RD, true, false, RH>(a, sm, w, r0, ta, tb, s_zpre, ta == t0 ? npre : 0, s_nz);
    else
    gmm_units<K, STORE, TB, LONE, OC, CL, FPN, RG, SG, RD>(a, sm, w, r0, ta, tb, s_zpre, ta == t0 ? npre : 0);
    POCS_STAMP(1);
    __syncthreads();
    POCS_STAMP(2);
    gmm_emit_rows(a, sm, r0, ta, tb);
    if (tb < t1) {                                   // more units to come (only launches of > 64 runs): the slots start over
      __syncthreads();
      for (int j = tid; j < 2 * NW * K; j += TB) (&sm.xj[0][0][0])[j] = -1;
      __syncthreads();
    }
  }
  if constexpr (OC) {
    // (every wave's LDS additions lie in front of the barrier behind the last gmm_units; nkeep[] is reused by the closer's
    // exchange only, further down)
    const int rb = tid >> 6, j = tid & 63;
    if (rb <= r1 - r0 && j < sm.nkeep[rb]) {
      const unsigned n = sm.occ[rb][j];
      if (n) atomicAdd(&a.obs_counts[((size_t)(r0 + rb) * a.W + wr) * POCS_MAX_OBSTACLES + sm.oci[rb][j]], (unsigned long long)n);
    }
  }
  if constexpr (CL) {
    // (as occ above: every wave's LDS additions lie in front of the barrier behind the last gmm_units)
    const int rb = tid >> 2, l = tid & 3;
    static_assert(POCS_MAX_CLEARANCE_LEVELS == 4, "thread 4 rb + l");
    if (tid < 8 && rb <= r1 - r0 && l < a.clr_L) {
      const unsigned n = sm.clc[rb][l];
      if (n) atomicAdd(&a.clr_counts[((size_t)(r0 + rb) * a.W + wr) * POCS_MAX_CLEARANCE_LEVELS + l], (unsigned long long)n);
    }
  }
  if constexpr (RG) {
    // (as clc above: every wave's LDS additions lie in front of the barrier behind the last gmm_units)
    const int rb = tid >> 2, g = tid & 3;
    static_assert(POCS_MAX_REGIONS == 4, "thread 4 rb + g");
    if (tid < 8 && rb <= r1 - r0 && g < a.reg_G) {
      const unsigned n = sm.rgc[rb][g];
      if (n) atomicAdd(&a.reg_counts[((size_t)(r0 + rb) * a.W + wr) * POCS_MAX_REGIONS + g], (unsigned long long)n);
    }
  }
  if constexpr (SG) {
    // (as clc above: every wave's LDS additions lie in front of the barrier behind the last gmm_units)
    if (tid < 2 && tid <= r1 - r0) {
      const unsigned n = sm.sgc[tid];
      if (n) atomicAdd(&a.seg_counts[(size_t)(r0 + tid) * a.W + wr], (unsigned long long)n);
    }
  }
  if (LONE) return;                                  // the rows leave through the kernel boundary; the next launch's heads add them
  drain_stores();
  __syncthreads();
  POCS_STAMP(3);
  if (tid <= r1 - r0) {                              // one ticket per run touched: the blocks whose range meets [r VS, (r + 1) VS)
    const int r = r0 + tid;
    const int b_first = ((r << a.vs_shift) - t_lo) / a.upb, b_last_raw = ((((r + 1) << a.vs_shift) - 1) - t_lo) / a.upb;
    const int b_last = b_last_raw < (int)gridDim.x - 1 ? b_last_raw : (int)gridDim.x - 1;
    const unsigned t = __hip_atomic_fetch_add(&a.ticket[(size_t)r * a.W + wr], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sm.last[tid] = (t == (unsigned)(b_last - b_first)) ? 1 : 0;
  }
  if (tid == 0 && r1 == r0) sm.last[1] = 0;
  __syncthreads();
  POCS_STAMP(4);
  // The closer of a run, written out for the block's first run and -- when its range crosses into a second one --
  // once more, NOT as a loop over the two: the advance wants every vector register there is, and in a loop
  // whatever the compiler hoists out of the body (thread-dependent addresses) is live across it and spilled
  // (256 bytes of scratch per lane instead of 60).
  auto closer = [&](const int rb) __attribute__((always_inline)) -> bool {
    const int r = r0 + rb;
    // (a call of plans: a run whose plan ends at w has no waypoint w + 1 -- no chain record, no state / param rows to build;
    // those runs are the tail of the launch's, and advance_in_tail is where they begin)
    bool adv = r < a.advance_in_tail;
    if (tid == 0) acquire_agent();
    __syncthreads();
    // the run's rows and -- one GPU -- what the mixture advance wants besides their sums (state[w], the chain record, the
    // sensor: written by earlier launches), requested together: one round trip instead of one after the other
    const adv_ptrs ap = advance_ptrs(a, K, w + 1, r, sm.adv());
    double* const l_mom = ap.l_mom;
    double advv[4];
    advance_request<true>(ap, false, tid, TB, advv, adv);
    close_rows<K, TB> cr;
    cr.request(close_rows_of<K>(a, a.partial, r), 1 << a.vs_shift, tid);
    double survv = 1.0;                                // RISK: the run's survival product up to w - 1, requested with the rest
    if constexpr (RISK) if (tid == 0 && w > 0) survv = load_wt(&a.surv[r]);
    requests_issued();
    if (adv) advance_commit(ap, false, tid, TB, advv);
    gmm_close_sums<K, TB, true>(a, wr, r, sm.par[rb], sm.stage(), l_mom, tid, a.partial, true, cr);
    POCS_STAMP(5);
    if constexpr (RISK) {
      // p_w and the running probability as gmm_combine (pocs_host.hip) forms them from the same moments: the counts added in
      // component order from 0.0, one division, one multiplication, one subtraction, IEEE double -- the host recomputes the
      // stop from the moments it reads back and refuses the call if the two ever disagree
      if (tid == 0) {
        double coll = 0.0;
        for (int k = 0; k < K; ++k) coll += l_mom[k * POCS_NMOM + 1];
        const double p = coll / (1.0 * (double)a.n_total);
        const double prod = survv * (1.0 - p);
        store_wt(&a.surv[r], prod);
        const bool stop = (1.0 - prod) >= a.risk_bound;
        if (stop) __hip_atomic_store(&a.stop[r], (unsigned)(w + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sm.last[rb] = stop ? 2 : 1;                    // (last0 / last1 were read before the first closer)
      }
      __syncthreads();
      if (sm.last[rb] == 2) adv = false;               // a stopped run builds no state / param[w + 1], draws no component counts
    }
    if (a.exchange_in_tail) {
      // sharded: the run's closer is also its messenger -- this shard's moments go to every rank, the world's
      // come back summed in rank order, and the mixture advances here (no launch, no host, between waypoints)
      __syncthreads();
      if (__hip_atomic_load(&a.sync[POCS_SYNC_ABORT], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return false;
      // (a whole call replayed from a graph bakes its arguments in: the call's number -- part of every row's epoch and
      // of the choice between the two slot sets -- then travels in the run's header, uploaded per call like its seed)
      unsigned long long epoch = a.xchg.epoch;
      int parity = a.xchg.parity;
      if (a.xchg_epoch_from_header) {
        const unsigned long long calls = a.hdr[r].pad;
        epoch = (calls << 20) | (unsigned long long)(w + 1);
        parity = (int)((calls * (unsigned long long)a.W + (unsigned long long)w) & 1ull);
      }
      if (!gmm_exchange_rows(a, a.xchg, epoch, parity, K, w, r, l_mom, l_mom, tid, TB, &sm.nkeep[0] /* free by now */)) return false;
      __syncthreads();                                 // the world's sums are in l_mom for the advance (which no longer starts with a staging barrier)
    }
    if (adv) advance_block(a, K, w + 1, r, sm.adv(), sm.spec(), true, tid, TB, true);     // (staged above; gmm_close_sums' barriers lie between)
    __syncthreads();
    POCS_STAMP(6);
    POCS_STAMP_COUNT(14);
    return true;
  };
  const int last0 = __builtin_amdgcn_readfirstlane(sm.last[0]), last1 = __builtin_amdgcn_readfirstlane(sm.last[1]);
  if (last0 && !closer(0)) return;
  if (last1) (void)closer(1);
}

template <int K, bool STORE, int TB, bool LONE>
__global__ __launch_bounds__(TB, (LONE ? 1 : POCS_GMM_BLOCKS_PER_CU) * TB / 256) void k_gmm_step(pocs_gmm_launch a) {   // (lone: one block per CU, its LDS)
  gmm_step_block<K, STORE, TB, LONE, false>(a);
}
// The ticket form under a risk bound (RISK above).  A kernel of its own name: k_gmm_step is, instruction for instruction, what
// it is without the feature.
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_risk(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, true>(a);
}

// One level of a tree of plans (TREE above), with or without the risk bound.
template <int K, int TB, bool RISK>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_tree(pocs_gmm_launch a) {
  gmm_step_block<K, false, TB, false, RISK, true>(a);
}

// The counting forms (POCS_OPT_OBSTACLE_COUNTS): kernels of their own names, so that the ones above stay what they are.
template <int K, bool STORE, int TB, bool LONE>
__global__ __launch_bounds__(TB, (LONE ? 1 : POCS_GMM_BLOCKS_PER_CU) * TB / 256) void k_gmm_step_boxes(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, LONE, false, false, true>(a);
}
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_risk_boxes(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, true, false, true>(a);
}
template <int K, int TB, bool RISK>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_tree_boxes(pocs_gmm_launch a) {
  gmm_step_block<K, false, TB, false, RISK, true, true>(a);
}

// The clearance forms (CL above): kernels of their own names again.
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_clear(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, false, false, false, false, true>(a);
}
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_risk_clear(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, true, false, false, false, true>(a);
}

// The forms under a compound footprint (FPN above): kernels of their own names again.
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_parts(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, false, false, false, false, false, true>(a);
}
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_risk_parts(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, true, false, false, false, false, true>(a);
}

// The forms that count watched regions (RG above): kernels of their own names again.
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_regions(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, false, false, false, false, false, false, true>(a);
}
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_risk_regions(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, true, false, false, false, false, false, true>(a);
}

// The forms under segment checks (SG above): kernels of their own names again.
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_seg(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, false, false, false, false, false, false, false, true>(a);
}
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_risk_seg(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, true, false, false, false, false, false, false, true>(a);
}

// The forms under round obstacles (RD above; pocs_set_discs with D > 0): kernels of their own names again.  The head stages and culls
// the composed table with gmm_cull as it is -- a disc record reads as its bounding square there, marker copied -- and the shared memory
// is the twin's: the same LDS, two blocks per CU in every instantiation.
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_round(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, false, false, false, false, false, false, false, false, true>(a);
}
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_risk_round(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, true, false, false, false, false, false, false, false, true>(a);
}

// The forms under uncertain discs (RN above; pocs_set_disc_covariances with a nonzero row), on top of the _round forms: kernels of their
// own names again.  The head culls with gmm_cull<true>, which grows the tightened boxes and leaves each kept record's row beside the
// kept list; the sampling loop draws an uncertain disc's deviation per pair and tests the displaced disc.
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_noise(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, false, false, false, false, false, false, false, false, true, true>(a);
}
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_risk_noise(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, true, false, false, false, false, false, false, false, true, true>(a);
}

// The forms under prediction hypotheses (RH above; pocs_set_disc_hypotheses), on top of the _noise forms: kernels of their own names
// again.  The head culls with gmm_cull<true, true>, which leaves each kept record's gate beside its row; the sampling loop draws a
// gated disc's existence word per pair and and-s the poses for which it exists into the record's broad-phase masks.
// Whether samples are stored is the launch's word `store` here, read at run time (gmm_units): one kernel per K and risk setting.
template <int K, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_hyp(pocs_gmm_launch a) {
  gmm_step_block<K, true, TB, false, false, false, false, false, false, false, false, false, true, true, false, true>(a);
}
template <int K, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_risk_hyp(pocs_gmm_launch a) {
  gmm_step_block<K, true, TB, false, true, false, false, false, false, false, false, false, true, true, false, true>(a);
}

// The forms under a round footprint (RF above; pocs_set_footprint_disc): a family of its own names, for worlds with and without discs,
// and its noise twins under disc covariances.  The head culls with gmm_cull_rfoot -- no heading range -- and the sampling loop tests
// with pocs_pair_round_masks, which forms no sine or cosine.  The shared memory is the twin's (the noise twins: + the 4 KB of rows).
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_rfoot(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, false, false, false, false, false, false, false, false, false, false, true>(a);
}
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_risk_rfoot(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, true, false, false, false, false, false, false, false, false, false, true>(a);
}
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_rfoot_noise(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, false, false, false, false, false, false, false, false, false, true, true>(a);
}
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_risk_rfoot_noise(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, true, false, false, false, false, false, false, false, false, true, true>(a);
}

// The forms under a large collision world (WORLD above): kernels of their own names again.
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_world(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, false, false, false, true>(a);
}
template <int K, bool STORE, int TB>
__global__ __launch_bounds__(TB, POCS_GMM_BLOCKS_PER_CU * TB / 256) void k_gmm_step_risk_world(pocs_gmm_launch a) {
  gmm_step_block<K, STORE, TB, false, true, false, false, true>(a);
}

// The cull of a large world for one waypoint: one block per run of the launch's run range, in front of the waypoint's sampling
// launch on the same stream (a kernel node of the replayed graph like the others).  The block forms the run's reach from
// param[run][waypoint] as gmm_cull does (gmm_reach), tests all world_M records with gmm_cull's keep test (pocs_world_keep) and
// writes the kept ones in the caller's order: per pass of POCS_CULL_BLOCK records a ballot per wave, the (pass, wave) counts
// through LDS, one prefix over them by wave 0 -- no atomics, so the list is the same in every replay.  The first
// POCS_MAX_OBSTACLES kept records go to kept[run] (fields 6 and 7 tightened, as gmm_cull leaves them) with their indices, the full
// count to reach[run][waypoint].  A run stopped under the risk bound has no param[waypoint]: its reach is 0 (a NaN box would keep
// everything and report an overflow that is none).
template <int K>
__global__ __launch_bounds__(POCS_CULL_BLOCK) void k_world_cull(pocs_gmm_launch a) {
  constexpr int NT = POCS_CULL_BLOCK, NW = NT / 64, PS = K * POCS_PARAM_STRIDE, NIT = POCS_MAX_WORLD_RECORDS / NT;
  static_assert(NIT * NW == 64 && NIT <= 32, "the (pass, wave) counts are one wave's worth; a thread's keep bits fit a word");
  static_assert(PS <= NT, "one sampler parameter per thread");
  __shared__ double s_par[PS];
  __shared__ int s_cnt[NIT * NW];
  __shared__ int s_total;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = a.run_lo + (int)blockIdx.x, w = a.waypoint;
  const int M = a.world_M < POCS_MAX_WORLD_RECORDS ? a.world_M : POCS_MAX_WORLD_RECORDS;
  int* const reach = &a.reach[(size_t)r * a.W + w];
  unsigned stopw = 0u;
  if (a.stop) stopw = __hip_atomic_load(&a.stop[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const double parv = tid < PS ? load_wt(&a.param[((size_t)r * a.W + w) * PS + tid]) : 0.0;
  requests_issued();
  if (__builtin_amdgcn_readfirstlane((int)stopw) != 0) {      // (the same word in every thread of the block)
    if (tid == 0) __hip_atomic_store(reach, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  if (tid < PS) s_par[tid] = parv;
  if (tid < NIT * NW) s_cnt[tid] = 0;
  __syncthreads();
  pocs_reach rc;
  double ext_x, ext_y;
  gmm_reach<K>(a.fp, a.fp_rr, a.fp_phi, lane, s_par, rc, ext_x, ext_y);      // (every wave for itself: all 64 lanes)
  const int nit = (M + NT - 1) / NT;                  // (block-uniform: every lane of a wave is at every ballot)
  unsigned keepbits = 0u;
  for (int it = 0; it < nit; ++it) {
    const int m = it * NT + tid;
    bool keep = false;
    double bx, by;
    if (m < M) keep = pocs_world_keep(a.world + (size_t)m * POCS_OBS_STRIDE, rc, ext_x, ext_y, bx, by);
    const unsigned long long b = __ballot(keep);
    if (keep) keepbits |= 1u << it;
    if (lane == 0) s_cnt[it * NW + wave] = __popcll(b);
  }
  __syncthreads();
  if (tid < 64) {                                     // exclusive prefix of the 64 counts, which lie in record order
    const int v = s_cnt[tid];
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(inc, d);
      if (lane >= d) inc += t;
    }
    s_cnt[tid] = inc - v;
    if (tid == 63) s_total = inc;
  }
  __syncthreads();
  double* const kept = a.kept + (size_t)r * (POCS_MAX_OBSTACLES * POCS_OBS_STRIDE);
  int* const kept_idx = a.kept_idx + (size_t)r * POCS_MAX_OBSTACLES;
  for (int it = 0; it < nit; ++it) {
    const bool keep = ((keepbits >> it) & 1u) != 0u;
    const unsigned long long b = __ballot(keep);
    if (keep) {
      const int pos = s_cnt[it * NW + wave] + __popcll(b & ((1ull << lane) - 1ull));
      if (pos < POCS_MAX_OBSTACLES) {
        const int m = it * NT + tid;
        const double* o = a.world + (size_t)m * POCS_OBS_STRIDE;
        double bx, by;
        (void)pocs_world_keep(o, rc, ext_x, ext_y, bx, by);      // (the same function of the same arguments: the tightened broad phase)
#pragma unroll
        for (int j = 0; j < 6; ++j) store_wt(&kept[pos * POCS_OBS_STRIDE + j], o[j]);
        store_wt(&kept[pos * POCS_OBS_STRIDE + 6], bx);
        store_wt(&kept[pos * POCS_OBS_STRIDE + 7], by);
        __hip_atomic_store(&kept_idx[pos], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  if (tid == 0) __hip_atomic_store(reach, s_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Lone call, behind the last waypoint's launch: its rows -> moments[W-1] (one block).
template <int K>
__global__ __launch_bounds__(256) void k_gmm_close(pocs_gmm_launch a) {
  constexpr int NC = K * POCS_NMOM, PS = K * POCS_PARAM_STRIDE;
  __shared__ double s_par[PS];
  __shared__ double s_stage[16 * NC];
  __shared__ double s_tot[NC];
  const int w = a.waypoint, r = a.run_lo;
  for (int j = threadIdx.x; j < PS; j += 256) s_par[j] = a.param[((size_t)r * a.W + w) * PS + j];
  close_rows<K, 256> cr;
  gmm_close_sums<K, 256>(a, w, r, s_par, s_stage, s_tot, threadIdx.x, a.partial, true, cr);    // (first barrier: s_par is in)
}

// pocs_dev_probe.hpp -- the test hooks' kernels, a part of pocs_kernels.hip (the only unit with device code; included there last,
// inside its anonymous namespace).  Nothing of the hot path calls them: pocs_probe.hip launches them, through pocs_launch_probe_*
// in pocs_kernels.hip, on inputs a test picks.  Relies on pocs_dev_prims.hpp (stage_tables, request_tables, load_wt), on
// pocs_dev_gmm.hpp (gmm_smem, gmm_cull), on pocs_dev_mc.hpp (stage_mc_head, mc_move_dir) and on pocs_math.h / pocs_collide.h.
//
//   k_probe_math, k_probe_radius_roots   the sampler's table-driven functions and its two square roots
//   k_probe_collide, k_probe_counts      the collision test with k_gmm_step's cull; the component counts of a waypoint
//   k_probe_clearance, k_probe_parts, k_probe_regions, k_probe_segment, k_probe_discs, k_probe_disc_noise, k_probe_disc_hypotheses,
//   k_probe_footprint_disc
//                                        a mode's single-pose form beside its pair form, pose by pose: ONE block each, which stages
//                                        its tables with probe_stage and walks the poses with probe_pair_walk
//
// The two pieces the pair probes share exist once: the copy of a record table into LDS (probe_stage) and the walk over the pairs of
// poses (probe_pair_walk).

// `count` doubles of a table in device memory -> LDS, by the whole block: the records of an env->obs unless the caller says otherwise.
__device__ __forceinline__ void probe_stage(const double* __restrict__ src, double* dst, const int count = POCS_MAX_OBSTACLES * POCS_OBS_STRIDE) {
  for (int j = threadIdx.x; j < count; j += POCS_BLOCK) dst[j] = src[j];
}

// The walk of a one-block pair probe over n poses: pose 2 p with pose 2 p + 1 is pair p, an odd last pose is paired with itself
// (i1 == i0), and lane l of a wave takes the pairs p0 + l of the wave's trips p0 = first lane of the wave, + POCS_BLOCK, ...
// The pair forms ballot and turn their masks back into lane flags (__builtin_amdgcn_inverse_ballot_w64), so EVERY lane of a wave
// makes EVERY trip the wave makes: the trip count hangs on p0, which is the same in all 64 lanes, and a lane without a pair
// (!live) walks pose 0 beside itself and calls body like the others; body guards nothing but its writes with `live`.
//   body(xs, ys, ts, i0, i1, live): the pair's poses by column and their indices.  HEADING false: th is not read, ts is zeros.
template <bool HEADING = true, typename Body>
__device__ __forceinline__ void probe_pair_walk(const int n, const double* __restrict__ x, const double* __restrict__ y,
                                                const double* __restrict__ th, Body body) {
  const int npairs = (n + 1) / 2;
  for (int p0 = (int)threadIdx.x - (int)(threadIdx.x & 63); p0 < npairs; p0 += POCS_BLOCK) {
    const int p = p0 + (int)(threadIdx.x & 63);
    const bool live = p < npairs;
    const int i0 = live ? 2 * p : 0, i1 = live && i0 + 1 < n ? i0 + 1 : i0;
    const double xs[2] = {x[i0], x[i1]}, ys[2] = {y[i0], y[i1]};
    double ts[2] = {0.0, 0.0};
    if constexpr (HEADING) { ts[0] = th[i0]; ts[1] = th[i1]; }
    body(xs, ys, ts, i0, i1, live);
  }
}

// The hot path's table-driven sampler functions on words / angles the caller picks (pocs_probe_device_math: a test
// hook -- the words a free-running launch meets once in 2^32 draws, the cells' edges, a heading on a sector's tie):
// the same inline functions, the tables staged in LDS as k_gmm_step stages them, the constants pinned as there.
__global__ __launch_bounds__(POCS_BLOCK) void k_probe_math(const pocs_tables* __restrict__ tables, int n, const uint32_t* __restrict__ wr,
                                                          const uint32_t* __restrict__ wa, const double* __restrict__ x,
                                                          double* __restrict__ out) {
  __shared__ pocs_tables s_tab;
  stage_tables(tables, &s_tab);
  __syncthreads();
  POCS_VCONST(vc_);
  for (int i = threadIdx.x; i < n; i += POCS_BLOCK) {
    double z0, z1, sn, cs;
    pocs_normal_pair_w2(wr[i], wa[i], &s_tab, &z0, &z1, &vc_);
    pocs_sincos_tab(x[i], &s_tab, &sn, &cs, &vc_);
    out[i] = z0; out[n + i] = z1; out[2 * n + i] = sn; out[3 * n + i] = cs;
    out[4 * n + i] = pocs_radius2_unit32(wr[i], &s_tab);
  }
}
// The Box-Muller radius' two square roots on a range of words (pocs_probe_device_radius_roots: a test hook -- the sweep over
// all 2^32 words that pocs_sqrt_radius rests on): per word the argument t = |pocs_radius2_unit32(w)| through the tables
// staged in LDS as k_gmm_step stages them, the correctly rounded root and the short one; a wave adds the number of its lanes
// whose two roots differ in any bit to out[0], and the smallest such word goes to out[1].
__global__ __launch_bounds__(POCS_BLOCK) void k_probe_radius_roots(const pocs_tables* __restrict__ tables, uint32_t first, unsigned long long count,
                                                                  unsigned long long* __restrict__ out) {
  __shared__ pocs_tables s_tab;
  stage_tables(tables, &s_tab);
  __syncthreads();
  const unsigned long long stride = (unsigned long long)gridDim.x * POCS_BLOCK;
  // (every lane of a wave makes every trip: the count is balloted)
  for (unsigned long long i0 = (unsigned long long)blockIdx.x * POCS_BLOCK + (threadIdx.x & ~63u); i0 < count; i0 += stride) {
    const unsigned long long i = i0 + (threadIdx.x & 63u);
    const bool live = i < count;
    const uint32_t w = first + (uint32_t)(live ? i : 0ull);
    const double t = fabs(pocs_radius2_unit32(w, &s_tab));
    const double full = pocs_sqrt_normal(t), brief = pocs_sqrt_radius(t);
    const bool bad = live && __builtin_bit_cast(unsigned long long, full) != __builtin_bit_cast(unsigned long long, brief);
    const unsigned long long b = __ballot(bad);
    if (b != 0ull) {                                                 // (scalar)
      if ((threadIdx.x & 63u) == (unsigned)__builtin_ctzll(b)) {    // the wave's first such lane: its lowest such word
        atomicAdd(&out[0], (unsigned long long)__popcll(b));
        atomicMin(&out[1], (unsigned long long)w);
      }
    }
  }
}
// The hot paths' collision test and k_gmm_step's obstacle cull on poses, a mixture and a world the caller picks
// (pocs_probe_device_collide: a test hook -- a pose a few ulps from touching, a pose at the edge of what the mixture can
// draw, which no free-running launch meets): ONE block that does what the kernels' blocks do, through the same inline
// functions.  The head of gmm_step_block (ticket form, one run): tables, obstacle table and the mixture's parameters ->
// gmm_smem, wave 0 culls, barrier.  Then the head of an MC block (stage_mc_head: its loops are guarded by the arrays'
// sizes, so a block of TB >= POCS_BLOCK threads stages the same bytes).  Then per pose the three forms the kernels use:
//   flags[i]          pocs_pose_collides on the full table, as the MC kernels call it
//   flags[n + i]      pocs_pair_collides<false> on the culled table, as the batch form of k_gmm_step calls it
//   flags[2 n + i]    pocs_pair_collides<true> on the culled table, as its lone form does
// poses 2 p and 2 p + 1 one pair; an odd last pose is paired with itself, and 2 is added to its flag should the two
// slots of that pair ever disagree.
template <int K, int TB>
__global__ __launch_bounds__(TB) void k_probe_collide(pocs_gmm_launch a, int n, const double* __restrict__ x, const double* __restrict__ y,
                                                      const double* __restrict__ th, int* __restrict__ flags, int* __restrict__ nkeep_out,
                                                      double* __restrict__ kept) {
  typedef gmm_smem<K, TB> smem_t;
  __shared__ smem_t sm;
  constexpr int PS = K * POCS_PARAM_STRIDE;
  static_assert(POCS_MAX_OBSTACLES * POCS_OBS_STRIDE <= TB && PS <= TB, "one obstacle element, one sampler parameter per thread");
  const int tid = threadIdx.x;
  double tabv[table_regs<TB>::N];
  request_tables<TB>(a.tables, tid, tabv);
  const double obs_elem = tid < a.M * POCS_OBS_STRIDE ? a.env->obs[tid] : 0.0;
  const double parv = tid < PS ? load_wt(&a.param[tid]) : 0.0;
  requests_issued();
  commit_tables<TB>(&sm.tab, tid, tabv);
  if (tid < a.M * POCS_OBS_STRIDE) sm.obs()[tid] = obs_elem;
  if (tid < PS) sm.par[0][tid] = parv;
  __syncthreads();
  if (tid < 64) gmm_cull(a, sm, 0, tid, sm.par[0]);
  __syncthreads();
  const int nkeep = __builtin_amdgcn_readfirstlane(sm.nkeep[0]);
  if (tid == 0) *nkeep_out = nkeep;
  for (int j = tid; j < nkeep * POCS_OBS_STRIDE; j += TB) kept[j] = sm.keep[0][j];
  const mc_head hd = stage_mc_head(a.env, a.tables);
  const mc_world wd = hd.world();
  for (int i = tid; i < n; i += TB)
    flags[i] = pocs_pose_collides(x[i], y[i], th[i], &wd.fp, wd.obs, wd.M, wd.tab) ? 1 : 0;
  const pocs_footprint fp = a.fp;
  POCS_VCONST(vc_);
  for (int p = tid; 2 * p < n; p += TB) {
    const int i0 = 2 * p, i1 = i0 + 1 < n ? i0 + 1 : i0;
    const double xs[2] = {x[i0], x[i1]}, ys[2] = {y[i0], y[i1]}, ts[2] = {th[i0], th[i1]};
    bool hits[2];
    pocs_pair_collides<false>(xs, ys, ts, &fp, sm.keep[0], nkeep, &sm.tab, &vc_, hits);
    flags[n + i0] = (hits[0] ? 1 : 0) + (i1 == i0 && hits[1] != hits[0] ? 2 : 0);
    if (i1 != i0) flags[n + i1] = hits[1] ? 1 : 0;
    pocs_pair_collides<true>(xs, ys, ts, &fp, sm.keep[0], nkeep, &sm.tab, &vc_, hits);
    flags[2 * n + i0] = (hits[0] ? 1 : 0) + (i1 == i0 && hits[1] != hits[0] ? 2 : 0);
    if (i1 != i0) flags[2 * n + i1] = hits[1] ? 1 : 0;
  }
}
// The clearance level of poses, a footprint, distances and a world the caller picks (pocs_probe_device_clearance: a test hook beside
// k_probe_collide): ONE block stages the tables, the base records and the records of the footprint grown by the largest distance as
// the kernels' heads do and asks, per pose, the functions the kernels ask: pocs_pose_collides for the footprint itself (-1), then
// pocs_pose_clearance_level as the MC kernels call it; and pocs_pair_clearance_masks as k_gmm_step's clearance form calls it, pose
// 2 p with pose 2 p + 1 (an odd last pose with itself) -- 100 is added to a pose's answer should the two forms ever disagree.
__global__ __launch_bounds__(POCS_BLOCK) void k_probe_clearance(const pocs_env_dev* __restrict__ env, const pocs_clear_dev* __restrict__ clr, int L,
                                                                const pocs_tables* __restrict__ tables, int n, const double* __restrict__ x,
                                                                const double* __restrict__ y, const double* __restrict__ th, int* __restrict__ out) {
  __shared__ pocs_tables s_tab;
  __shared__ __attribute__((aligned(16))) double s_obs[POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];
  __shared__ __attribute__((aligned(16))) double s_obs2[POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];
  __shared__ double s_d[POCS_MAX_CLEARANCE_LEVELS];
  stage_tables(tables, &s_tab);
  probe_stage(env->obs, s_obs);
  probe_stage(clr->obs, s_obs2);
  if (threadIdx.x < POCS_MAX_CLEARANCE_LEVELS) s_d[threadIdx.x] = clr->d[threadIdx.x];
  __syncthreads();
  const pocs_footprint fp = env->fp;
  const int M = env->M;
  POCS_VCONST(vc_);
  probe_pair_walk(n, x, y, th, [&](const double* xs, const double* ys, const double* ts, const int i0, const int i1, const bool live) {
    int single[2], pair[2] = {L, L};
#pragma unroll
    for (int h = 0; h < 2; ++h)
      single[h] = pocs_pose_collides(xs[h], ys[h], ts[h], &fp, s_obs, M, &s_tab) ? -1
                : pocs_pose_clearance_level(xs[h], ys[h], ts[h], &fp, s_d, L, s_obs2, M, &s_tab);
    pocs_pair_clearance_masks(xs, ys, ts, &fp, s_d, L, s_obs2, M, &s_tab, &vc_, [&](const int l, const unsigned long long m0, const unsigned long long m1) {
      if (__builtin_amdgcn_inverse_ballot_w64(m0)) pair[0] = l;
      if (__builtin_amdgcn_inverse_ballot_w64(m1)) pair[1] = l;
    });
    if (live) {
      out[i0] = single[0] + ((single[0] >= 0 && pair[0] != single[0]) || (i1 == i0 && single[1] != single[0]) ? 100 : 0);
      if (i1 != i0) out[i1] = single[1] + (single[1] >= 0 && pair[1] != single[1] ? 100 : 0);
    }
  });
}
// Which parts of a compound footprint touch, on poses, parts and a world the caller picks (pocs_probe_device_footprint_parts: a test
// hook beside k_probe_clearance): ONE block stages the tables, the records (prepared for the covering part) and the parts as the
// kernels' heads do and asks, per pose, the functions the kernels ask: pocs_pose_parts_touched as the MC kernels' predicate forms
// its flag; and pocs_pair_parts_masks as k_gmm_step's parts form calls it, pose 2 p with pose 2 p + 1 (an odd last pose with
// itself) -- bit 8 is set in a pose's answer should the two forms ever disagree.
__global__ __launch_bounds__(POCS_BLOCK) void k_probe_parts(const pocs_env_dev* __restrict__ env, const pocs_parts_dev* __restrict__ parts, int F,
                                                            const pocs_tables* __restrict__ tables, int n, const double* __restrict__ x,
                                                            const double* __restrict__ y, const double* __restrict__ th, int* __restrict__ out) {
  __shared__ pocs_tables s_tab;
  __shared__ __attribute__((aligned(16))) double s_obs[POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];
  __shared__ double s_parts[POCS_MAX_FOOTPRINT_PARTS * POCS_PART_STRIDE];
  stage_tables(tables, &s_tab);
  probe_stage(env->obs, s_obs);
  if (threadIdx.x < POCS_MAX_FOOTPRINT_PARTS * POCS_PART_STRIDE) s_parts[threadIdx.x] = parts->part[threadIdx.x];
  __syncthreads();
  const int M = env->M;
  POCS_VCONST(vc_);
  probe_pair_walk(n, x, y, th, [&](const double* xs, const double* ys, const double* ts, const int i0, const int i1, const bool live) {
    unsigned single[2], pair[2] = {0u, 0u};
#pragma unroll
    for (int h = 0; h < 2; ++h) single[h] = pocs_pose_parts_touched(xs[h], ys[h], ts[h], s_parts, F, s_obs, M, &s_tab);
    unsigned long long all[2];
    pocs_pair_parts_masks(xs, ys, ts, s_parts, F, s_obs, M, &s_tab, &vc_, all, [&](const int f, const unsigned long long m0, const unsigned long long m1) {
      if (__builtin_amdgcn_inverse_ballot_w64(m0)) pair[0] |= 1u << f;
      if (__builtin_amdgcn_inverse_ballot_w64(m1)) pair[1] |= 1u << f;
    });
    const bool any0 = __builtin_amdgcn_inverse_ballot_w64(all[0]), any1 = __builtin_amdgcn_inverse_ballot_w64(all[1]);
    if (live) {
      out[i0] = (int)(single[0] | ((pair[0] != single[0] || any0 != (single[0] != 0u) || (i1 == i0 && single[1] != single[0])) ? 256u : 0u));
      if (i1 != i0) out[i1] = (int)(single[1] | ((pair[1] != single[1] || any1 != (single[1] != 0u)) ? 256u : 0u));
    }
  });
}
// Which watched regions poses are in, on poses and regions the caller picks (pocs_probe_device_regions: a test hook beside
// k_probe_parts): ONE block stages the tables and the regions' records and footprints as the kernels' heads do and asks, per pose,
// pocs_pose_regions_mask as the MC kernels call it, and pocs_pair_regions_masks, the sampling thread's pair form, pose 2 p with pose
// 2 p + 1 (an odd last pose with itself) -- bit 8 + g is set in a pose's answer should the two forms ever disagree on region g.
__global__ __launch_bounds__(POCS_BLOCK) void k_probe_regions(const pocs_regions_dev* __restrict__ regions, int G,
                                                              const pocs_tables* __restrict__ tables, int n, const double* __restrict__ x,
                                                              const double* __restrict__ y, const double* __restrict__ th, int* __restrict__ out) {
  __shared__ pocs_tables s_tab;
  __shared__ __attribute__((aligned(16))) double s_reg[POCS_REGIONS_HEAD];
  stage_tables(tables, &s_tab);
  if (threadIdx.x < POCS_REGIONS_HEAD) s_reg[threadIdx.x] = reinterpret_cast<const double*>(regions)[threadIdx.x];
  __syncthreads();
  const double* const s_rec = s_reg;
  const double* const s_fp = s_reg + POCS_MAX_REGIONS * POCS_OBS_STRIDE;
  POCS_VCONST(vc_);
  probe_pair_walk(n, x, y, th, [&](const double* xs, const double* ys, const double* ts, const int i0, const int i1, const bool live) {
    unsigned single[2], pair[2] = {0u, 0u};
#pragma unroll
    for (int h = 0; h < 2; ++h) single[h] = pocs_pose_regions_mask(xs[h], ys[h], ts[h], s_rec, s_fp, G, &s_tab);
    pocs_pair_regions_masks(xs, ys, ts, s_rec, s_fp, G, ~0u, &s_tab, &vc_, [&](const int g, const unsigned long long m0, const unsigned long long m1) {
      if (__builtin_amdgcn_inverse_ballot_w64(m0)) pair[0] |= 1u << g;
      if (__builtin_amdgcn_inverse_ballot_w64(m1)) pair[1] |= 1u << g;
    });
    if (live) {
      out[i0] = (int)(single[0] | ((pair[0] ^ single[0]) << 8) | (i1 == i0 ? (single[1] ^ single[0]) << 8 : 0u));
      if (i1 != i0) out[i1] = (int)(single[1] | ((pair[1] ^ single[1]) << 8));
    }
  });
}
// The segment checks' sub-poses on poses, a footprint, a world and a control the caller picks (pocs_probe_device_segment: a test hook
// beside k_probe_parts): ONE block stages the tables and the records as the kernels' heads do and asks, per pose, the functions the
// kernels ask.  backward 0, the MC form: the pose is a particle at the segment's start, the end pose is mc_move's (bit J: it touches,
// by pocs_pose_collides), the sub-poses pocs_segment_touched_dir with mc_move_dir's sine and cosine, as mc_step_body calls it.
// backward 1, the GMM form: the pose is a sample at the segment's end (bit J: it touches), the sub-poses pocs_segment_touched.  And
// both ways pocs_pair_segment_masks as k_gmm_step's segment form calls it, pose 2 p with pose 2 p + 1 (an odd last pose with itself):
// bit 16 is set in a pose's answer should the two forms ever disagree.
__global__ __launch_bounds__(POCS_BLOCK) void k_probe_segment(const pocs_env_dev* __restrict__ env, const pocs_seg_dev* __restrict__ seg,
                                                              const pocs_tables* __restrict__ tables, double u0, double u1, double u2, int backward, int n,
                                                              const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ th,
                                                              int* __restrict__ out) {
  __shared__ pocs_tables s_tab;
  __shared__ __attribute__((aligned(16))) double s_obs[POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];
  __shared__ double s_f[POCS_MAX_SEGMENT_CHECKS];
  stage_tables(tables, &s_tab);
  probe_stage(env->obs, s_obs);
  if (threadIdx.x < POCS_MAX_SEGMENT_CHECKS) s_f[threadIdx.x] = seg->f[threadIdx.x];
  __syncthreads();
  const int M = env->M, J = seg->J;
  const pocs_footprint fp = env->fp;
  POCS_VCONST(vc_);
  const double a0 = backward ? -u2 : u0;
  probe_pair_walk(n, x, y, th, [&](const double* xs, const double* ys, const double* ts, const int i0, const int i1, const bool live) {
    unsigned single[2], pair[2] = {0u, 0u};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (backward) {
        single[h] = pocs_segment_touched(xs[h], ys[h], ts[h], a0, u1, s_f, J, 1, &fp, s_obs, M, &s_tab);
        if (pocs_pose_collides(xs[h], ys[h], ts[h], &fp, s_obs, M, &s_tab)) single[h] |= 1u << J;
      } else {
        double nx, ny, nt, sn, cs;
        mc_move_dir(xs[h], ys[h], ts[h], u0, u1, u2, nx, ny, nt, sn, cs);
        single[h] = pocs_segment_touched_dir(xs[h], ys[h], ts[h] + u0, sn, cs, u1, s_f, J, 0, &fp, s_obs, M, &s_tab);
        if (pocs_pose_collides(nx, ny, nt, &fp, s_obs, M, &s_tab)) single[h] |= 1u << J;
      }
    }
    unsigned long long all[2];
    pocs_pair_segment_masks(xs, ys, ts, a0, u1, s_f, J, backward, &fp, s_obs, M, &s_tab, &vc_, all, [&](const int j, const unsigned long long m0, const unsigned long long m1) {
      if (__builtin_amdgcn_inverse_ballot_w64(m0)) pair[0] |= 1u << j;
      if (__builtin_amdgcn_inverse_ballot_w64(m1)) pair[1] |= 1u << j;
    });
    const bool any0 = __builtin_amdgcn_inverse_ballot_w64(all[0]), any1 = __builtin_amdgcn_inverse_ballot_w64(all[1]);
    const unsigned subs = (1u << J) - 1u;
    if (live) {
      out[i0] = (int)(single[0] | ((pair[0] != (single[0] & subs) || any0 != ((single[0] & subs) != 0u) || (i1 == i0 && single[1] != single[0])) ? 65536u : 0u));
      if (i1 != i0) out[i1] = (int)(single[1] | ((pair[1] != (single[1] & subs) || any1 != ((single[1] & subs) != 0u)) ? 65536u : 0u));
    }
  });
}
// The component counts of a waypoint on weights, alive flags, seeds, waypoints and sample totals the caller picks
// (pocs_probe_device_counts: a test hook -- a free-running call meets only the (n, p, seed) its own mixtures produce): one thread
// per case builds the K x POCS_STATE_STRIDE image of which only [12] (weight) and [13] (alive) matter, as speculate_counts does,
// and runs pocs_normalise_weights + pocs_component_counts -- the inline functions of advance_finish and speculate_counts.
// Kc / seeds / wp / n_total: n; w / alive / out: n rows of POCS_MAX_GAUSSIANS, of which case i uses the first Kc[i].
__global__ __launch_bounds__(POCS_BLOCK) void k_probe_counts(int n, const int* __restrict__ Kc, const double* __restrict__ w,
                                                            const double* __restrict__ alive, const unsigned long long* __restrict__ seeds,
                                                            const uint32_t* __restrict__ wp, const double* __restrict__ n_total,
                                                            double* __restrict__ out) {
  const int i = (int)blockIdx.x * POCS_BLOCK + (int)threadIdx.x;
  if (i >= n) return;
  const int K = min(max(Kc[i], 1), POCS_MAX_GAUSSIANS);              // (the host has checked the range)
  const size_t row = (size_t)i * POCS_MAX_GAUSSIANS;
  double st[POCS_MAX_GAUSSIANS * POCS_STATE_STRIDE];
  for (int k = 0; k < K; ++k) {
    st[k * POCS_STATE_STRIDE + 12] = w[row + k];
    st[k * POCS_STATE_STRIDE + 13] = alive[row + k];
  }
  const int last_alive = pocs_normalise_weights(K, 1, st);
  double cum[POCS_MAX_GAUSSIANS];
  pocs_component_counts(K, st, last_alive, (uint64_t)seeds[i], wp[i], n_total[i], cum, 1);
  for (int k = 0; k < POCS_MAX_GAUSSIANS; ++k) out[row + k] = k < K ? cum[k] : 0.0;
}
// The footprint-against-world test on poses, a footprint, boxes and discs the caller picks (pocs_probe_device_discs: a test hook beside
// k_probe_segment): ONE block stages the tables and the composed records as the kernels' heads do and asks, per pose, the functions
// the kernels ask.  Bit 0: the pose touches some box, bit 1: some disc -- pocs_pose_kinds_touched, the single-pose form's operations
// with the two kinds apart -- and pocs_pose_collides<true> as the MC kernels call it must say (bits != 0).  Then
// pocs_pair_collides_masks' ROUND form as k_gmm_step_round calls it, pose 2 p with pose 2 p + 1 (an odd last pose with itself), its
// disc masks handed out: bit 8 is set in a pose's answer should the two forms ever disagree.
__global__ __launch_bounds__(POCS_BLOCK) void k_probe_discs(const pocs_env_dev* __restrict__ env, const pocs_tables* __restrict__ tables, int n,
                                                            const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ th,
                                                            int* __restrict__ out) {
  __shared__ pocs_tables s_tab;
  __shared__ __attribute__((aligned(16))) double s_obs[POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];
  stage_tables(tables, &s_tab);
  probe_stage(env->obs, s_obs);
  __syncthreads();
  const int M = env->M < POCS_MAX_OBSTACLES ? env->M : POCS_MAX_OBSTACLES;
  const pocs_footprint fp = env->fp;
  POCS_VCONST(vc_);
  probe_pair_walk(n, x, y, th, [&](const double* xs, const double* ys, const double* ts, const int i0, const int i1, const bool live) {
    unsigned single[2];
    bool bad[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      single[h] = pocs_pose_kinds_touched(xs[h], ys[h], ts[h], &fp, s_obs, M, &s_tab);
      bad[h] = pocs_pose_collides<true>(xs[h], ys[h], ts[h], &fp, s_obs, M, &s_tab) != (single[h] != 0u);
    }
    unsigned long long all[2], disc[2];
    pocs_pair_collides_masks<false, pocs_each_none, true>(xs, ys, ts, &fp, s_obs, M, &s_tab, &vc_, all, pocs_each_none(), disc);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool any = __builtin_amdgcn_inverse_ballot_w64(all[h]), round = __builtin_amdgcn_inverse_ballot_w64(disc[h]);
      // (a pose that touches a box AND a disc: the pair form says "any" and "disc"; the box bit is not handed out apart)
      if (any != (single[h] != 0u) || round != ((single[h] & 2u) != 0u)) bad[h] = true;
    }
    if (live) {
      out[i0] = (int)(single[0] | ((bad[0] || (i1 == i0 && single[1] != single[0])) ? 256u : 0u));
      if (i1 != i0) out[i1] = (int)(single[1] | (bad[1] ? 256u : 0u));
    }
  });
}
// Uncertain discs on poses, a footprint, discs and factor rows the caller picks (pocs_probe_device_disc_noise: a test hook beside
// k_probe_discs): ONE block stages the tables, the D grown disc records and their rows and asks, per pose of index first + i, the
// functions the kernels ask.  The displaced centres are pocs_disc_displaced's, disc by disc; bit d of a pose's flags is "touches
// displaced disc d" by pocs_pose_collides_noisy, the MC kernels' single-pose form, whose own answer must be (bits != 0).  Then
// pocs_pair_collides_masks' noisy ROUND form as k_gmm_step_noise calls it, disc by disc on poses 2 p, 2 p + 1 of pair
// (first >> 1) + p = (first + i0) >> 1 (an odd last pose beside its own twin's index, which is then not read): bit 31 should the two
// forms ever disagree.
__global__ __launch_bounds__(POCS_BLOCK) void k_probe_disc_noise(const pocs_env_dev* __restrict__ env, const double* __restrict__ rows,
                                                                 const pocs_tables* __restrict__ tables, unsigned long long seed, unsigned v,
                                                                 unsigned long long first, int n, const double* __restrict__ x,
                                                                 const double* __restrict__ y, const double* __restrict__ th,
                                                                 double* __restrict__ centres, unsigned* __restrict__ flags) {
  __shared__ pocs_tables s_tab;
  __shared__ __attribute__((aligned(16))) double s_obs[POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];
  __shared__ __attribute__((aligned(16))) double s_rows[POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE];
  stage_tables(tables, &s_tab);
  probe_stage(env->obs, s_obs);
  probe_stage(rows, s_rows, POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE);
  __syncthreads();
  const int D = env->M < 16 ? env->M : 16;
  const pocs_footprint fp = env->fp;
  POCS_VCONST(vc_);
  probe_pair_walk(n, x, y, th, [&](const double* xs, const double* ys, const double* ts, const int i0, const int i1, const bool live) {
    const bool two = i1 != i0;
    const unsigned long long idx[2] = {first + (unsigned long long)i0, first + (unsigned long long)i0 + 1ull};
    unsigned single[2] = {0u, 0u}, pair[2] = {0u, 0u};
    bool bad[2] = {false, false};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool any = pocs_pose_collides_noisy(xs[h], ys[h], ts[h], &fp, s_obs, s_rows, D, seed, idx[h], v, &s_tab, &single[h]);
      if (any != (single[h] != 0u)) bad[h] = true;
      if (live && (h == 0 || two))
        for (int d = 0; d < D; ++d) {
          double cx = s_obs[d * POCS_OBS_STRIDE], cy = s_obs[d * POCS_OBS_STRIDE + 1];
          if (s_rows[d * POCS_NOISE_STRIDE] != 0.0)
            pocs_disc_displaced(cx, cy, &s_rows[d * POCS_NOISE_STRIDE], seed, idx[h], v, &s_tab, &cx, &cy);
          double* const out = centres + ((size_t)(h == 0 ? i0 : i1) * (size_t)D + (size_t)d) * 2;
          out[0] = cx; out[1] = cy;
        }
    }
    for (int d = 0; d < D; ++d) {                                      // (scalar) the pair form, one record at a time: a bit per disc
      unsigned long long all[2];
      const pocs_noise_pair np = {&s_rows[d * POCS_NOISE_STRIDE], seed, idx[0] >> 1, v};
      pocs_pair_collides_masks<false, pocs_each_none, true, pocs_noise_pair>(xs, ys, ts, &fp, &s_obs[d * POCS_OBS_STRIDE], 1, &s_tab, &vc_, all,
                                                                             pocs_each_none(), nullptr, np);
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (__builtin_amdgcn_inverse_ballot_w64(all[h])) pair[h] |= 1u << d;
    }
    if (live) {
      flags[i0] = single[0] | ((bad[0] || pair[0] != single[0]) ? 0x80000000u : 0u);
      if (two) flags[i1] = single[1] | ((bad[1] || pair[1] != single[1]) ? 0x80000000u : 0u);
    }
  });
}
// Prediction hypotheses on poses, a footprint, discs, factor rows and gates the caller picks (pocs_probe_device_disc_hypotheses: a test
// hook beside k_probe_disc_noise): ONE block stages the tables, the D <= 32 grown disc records, their rows (zeros: no covariances) and
// their gates and asks, per pose of index first + i, the functions the kernels ask.  pocs_pose_collides_gated, the MC kernels'
// single-pose form, hands out bit d of `exists` per disc that exists for the pose and bit d of `flags` per disc the pose touches;
// its own answer must be (flags != 0).  Then pocs_pair_collides_masks' gated ROUND form as k_gmm_step_hyp calls it, disc by disc on
// poses 2 p, 2 p + 1 of pair (first + i0) >> 1: should the two forms ever disagree, the pose's exists is 0 and its flags are all ones.  v is the waypoint word of the
// deviations and of the existence draws alike.
__global__ __launch_bounds__(POCS_BLOCK) void k_probe_disc_hypotheses(const pocs_env_dev* __restrict__ env, const double* __restrict__ rows,
                                                                      const uint32_t* __restrict__ gates, const pocs_tables* __restrict__ tables,
                                                                      unsigned long long seed, unsigned v, unsigned long long first, int n,
                                                                      const double* __restrict__ x, const double* __restrict__ y,
                                                                      const double* __restrict__ th, unsigned* __restrict__ exists,
                                                                      unsigned* __restrict__ flags) {
  __shared__ pocs_tables s_tab;
  __shared__ __attribute__((aligned(16))) double s_obs[POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];
  __shared__ __attribute__((aligned(16))) double s_rows[POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE];
  __shared__ __attribute__((aligned(16))) uint32_t s_gates[POCS_MAX_OBSTACLES * POCS_GATE_STRIDE];
  stage_tables(tables, &s_tab);
  probe_stage(env->obs, s_obs);
  probe_stage(rows, s_rows, POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE);
  for (int j = threadIdx.x; j < POCS_MAX_OBSTACLES * POCS_GATE_STRIDE; j += POCS_BLOCK) s_gates[j] = gates[j];
  __syncthreads();
  const int D = env->M < 32 ? env->M : 32;
  const pocs_footprint fp = env->fp;
  POCS_VCONST(vc_);
  probe_pair_walk(n, x, y, th, [&](const double* xs, const double* ys, const double* ts, const int i0, const int i1, const bool live) {
    const bool two = i1 != i0;
    const unsigned long long idx[2] = {first + (unsigned long long)i0, first + (unsigned long long)i0 + 1ull};
    unsigned ex[2] = {0u, 0u}, single[2] = {0u, 0u}, pair[2] = {0u, 0u};
    bool bad[2] = {false, false};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool any = pocs_pose_collides_gated(xs[h], ys[h], ts[h], &fp, s_obs, s_rows, s_gates, D, seed, idx[h], v, v, &s_tab, &ex[h], &single[h]);
      if (any != (single[h] != 0u) || (single[h] & ~ex[h]) != 0u) bad[h] = true;
    }
    for (int d = 0; d < D; ++d) {                                      // (scalar) the pair form, one record at a time: a bit per disc
      unsigned long long all[2];
      const pocs_noise_gate_pair np = {&s_rows[d * POCS_NOISE_STRIDE], seed, idx[0] >> 1, v, &s_gates[d * POCS_GATE_STRIDE], v};
      pocs_pair_collides_masks<false, pocs_each_none, true, pocs_noise_gate_pair>(xs, ys, ts, &fp, &s_obs[d * POCS_OBS_STRIDE], 1, &s_tab, &vc_, all,
                                                                                  pocs_each_none(), nullptr, np);
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (__builtin_amdgcn_inverse_ballot_w64(all[h])) pair[h] |= 1u << d;
    }
    if (live) {                                                        // (a disagreement: touched discs that do not exist, all of them)
      const bool b0 = bad[0] || pair[0] != single[0], b1 = bad[1] || pair[1] != single[1];
      exists[i0] = b0 ? 0u : ex[0];
      flags[i0] = b0 ? 0xFFFFFFFFu : single[0];
      if (two) {
        exists[i1] = b1 ? 0u : ex[1];
        flags[i1] = b1 ? 0xFFFFFFFFu : single[1];
      }
    }
  });
}
// The round footprint's test on poses, a radius, boxes, discs and factor rows the caller picks (pocs_probe_device_footprint_disc: a test
// hook beside k_probe_discs): ONE block stages the tables, the composed records and -- where given -- their rows and asks, per pose of
// index first + i, the functions the kernels ask.  Bit 0: the pose touches some box, bit 1: some disc, displaced where its row says so
// -- pocs_round_pose_kinds, the single-pose form on the full table, and the MC kernels' pocs_round_pose_collides[_noisy] must say
// (bits != 0).  Then pocs_pair_round_masks as the _rfoot kernels call it on poses 2 p, 2 p + 1 of pair (first >> 1) + p =
// (first + i0) >> 1 (an odd last pose beside its own twin's index, which is then not read), its disc masks handed out: bit 8 should
// the two forms ever disagree.  There is no heading column: the walk reads none.
__global__ __launch_bounds__(POCS_BLOCK) void k_probe_footprint_disc(const pocs_env_dev* __restrict__ env, const double* __restrict__ rows,
                                                                     const pocs_tables* __restrict__ tables, unsigned long long seed, unsigned v,
                                                                     unsigned long long first, int n, const double* __restrict__ x,
                                                                     const double* __restrict__ y, int* __restrict__ out) {
  __shared__ pocs_tables s_tab;
  __shared__ __attribute__((aligned(16))) double s_obs[POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];
  __shared__ __attribute__((aligned(16))) double s_rows[POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE];
  stage_tables(tables, &s_tab);
  probe_stage(env->obs, s_obs);
  for (int j = threadIdx.x; j < POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE; j += POCS_BLOCK) s_rows[j] = rows ? rows[j] : 0.0;
  __syncthreads();
  const int M = env->M < POCS_MAX_OBSTACLES ? env->M : POCS_MAX_OBSTACLES;
  const double rho = env->fp.hx;
  const bool noisy = rows != nullptr;                                  // (the same in every thread)
  POCS_VCONST(vc_);
  probe_pair_walk<false>(n, x, y, nullptr, [&](const double* xs, const double* ys, const double*, const int i0, const int i1, const bool live) {
    const unsigned long long idx[2] = {first + (unsigned long long)i0, first + (unsigned long long)i0 + 1ull};
    unsigned single[2];
    bool bad[2];
    unsigned long long all[2], disc[2];
    if (noisy) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        single[h] = pocs_round_pose_kinds(xs[h], ys[h], rho, s_obs, M, s_rows, seed, idx[h], v, &s_tab);
        bad[h] = pocs_round_pose_collides_noisy(xs[h], ys[h], rho, s_obs, s_rows, M, seed, idx[h], v, &s_tab) != (single[h] != 0u);
      }
      const pocs_noise_pair np = {s_rows, seed, idx[0] >> 1, v};
      pocs_pair_round_masks<pocs_noise_pair>(xs, ys, rho, s_obs, M, &s_tab, &vc_, all, disc, np);
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        single[h] = pocs_round_pose_kinds(xs[h], ys[h], rho, s_obs, M);
        bad[h] = pocs_round_pose_collides(xs[h], ys[h], rho, s_obs, M) != (single[h] != 0u);
      }
      pocs_pair_round_masks(xs, ys, rho, s_obs, M, &s_tab, &vc_, all, disc);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool any = __builtin_amdgcn_inverse_ballot_w64(all[h]), round = __builtin_amdgcn_inverse_ballot_w64(disc[h]);
      // (a pose that touches a box AND a disc: the pair form says "any" and "disc"; the box bit is not handed out apart)
      if (any != (single[h] != 0u) || round != ((single[h] & 2u) != 0u)) bad[h] = true;
    }
    if (live) {
      out[i0] = (int)(single[0] | (bad[0] ? 256u : 0u));
      if (i1 != i0) out[i1] = (int)(single[1] | (bad[1] ? 256u : 0u));
    }
  });
}

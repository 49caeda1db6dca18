// pocs_dev_mc.hpp -- the Monte-Carlo family, a part of pocs_kernels.hip (the only unit with device code; included there,
// inside its anonymous namespace).  Relies on pocs_dev_prims.hpp (wave_sum_u32, requests_issued) and on pocs_math.h /
// pocs_collide.h; nothing of the GMM parts.
//
//   k_mc_init       P2+P3     initParticles (MCSimulator.h:287-297) + first checkParticleCollisions (:333-347)
//   k_mc_step       P1+P3     moveParticles (:300-322) + checkParticleCollisions, one waypoint, particles streamed through
//                             HBM (SoA): 24 B in, 24 B out, u32 RMW; k_mc_step_counts: with first collisions / the stop
//   k_mc_fused      P1+P3     same arithmetic, whole roll-out in registers (the controls do not depend on the particles,
//                             SURVEY 3.2), 0 B per evaluation; k_mc_fused_counts; k_mc_fused_sched: under an obstacle schedule
//   k_mc_tree_step  P1+P3     one level of a tree of plans: the parent's particles moved into the node's place
//   k_mc_count      P3        getCollisionProportion (:324-330): |{hits > 0}|.
//   k_mc_init_world, k_mc_step_world: k_mc_init and k_mc_step against a large collision world (pocs_set_world), culled per wave
//                             and particle iteration (mc_world_collides)
//   MC_BOXES forms of k_mc_init / k_mc_step_counts / k_mc_fused_sched, k_mc_fused_boxes, k_mc_tree_step_boxes: ... with the first
//                             collisions split by obstacle box (POCS_OPT_OBSTACLE_COUNTS)
//
// Each of these exists once: the block head (stage_mc_head -> mc_head -> mc_world), the initial draw (mc_initial), the motion
// step (mc_move), the particle accessors (mc_load / mc_store) and the block sum of counts (mc_block_add).

// what a thread keeps of the head behind the barrier: footprint and M in registers, obstacle records and tables where they are
struct mc_world {
  const double* obs;
  const pocs_tables* tab;
  pocs_footprint fp;
  int M;
};
// Where the head lies in LDS.  world() -- the copies of footprint and M out of LDS -- is a step of its own, which the kernels
// take BEHIND their run's pointers (mc_view): taken in stage_mc_head, the same instructions come out in another order.
struct mc_head {
  const double* obs;
  const pocs_tables* tab;
  const pocs_footprint* fp;
  const int* M;
  __device__ __forceinline__ mc_world world() const { return {obs, tab, *fp, *M}; }
};
// The head of an MC block (POCS_BLOCK threads): the collision world (obstacle records, footprint, M) and the 4 KB sector table --
// the MC kernels only evaluate the footprint heading -- into LDS, ending in the block's barrier.  Every load is issued before
// the first is waited for: written as copy loops with the block size as their stride, the compiler kept them loops of load -
// wait - store, four dependent memory round trips in front of every block's first particle.  (The obstacle array has its
// full size whatever M is: all of it is requested, M need not be known first.)
__device__ __forceinline__ mc_head stage_mc_head(const pocs_env_dev* __restrict__ env, const pocs_tables* __restrict__ g) {
  __shared__ double s_obs[POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];
  __shared__ pocs_footprint s_fp;
  __shared__ int s_M;
  __shared__ pocs_tables s_tab;
  constexpr int NO = POCS_MAX_OBSTACLES * POCS_OBS_STRIDE, NS = (int)(sizeof(g->sc) / sizeof(double));
  constexpr int UO = (NO + POCS_BLOCK - 1) / POCS_BLOCK, US = (NS + POCS_BLOCK - 1) / POCS_BLOCK;
  const int tid = threadIdx.x;
  const double* src = &g->sc[0][0];
  double vo[UO], vs[US];
#pragma unroll
  for (int u = 0; u < UO; ++u) { const int i = tid + u * POCS_BLOCK; vo[u] = i < NO ? env->obs[i] : 0.0; }
#pragma unroll
  for (int u = 0; u < US; ++u) { const int i = tid + u * POCS_BLOCK; vs[u] = i < NS ? src[i] : 0.0; }
  const pocs_footprint fp = env->fp;
  const int M = env->M;
  requests_issued();
  double* dst = &s_tab.sc[0][0];
#pragma unroll
  for (int u = 0; u < UO; ++u) { const int i = tid + u * POCS_BLOCK; if (i < NO) s_obs[i] = vo[u]; }
#pragma unroll
  for (int u = 0; u < US; ++u) { const int i = tid + u * POCS_BLOCK; if (i < NS) dst[i] = vs[u]; }
  if (tid == 0) { s_fp = fp; s_M = M; }
  __syncthreads();
  return {s_obs, &s_tab, &s_fp, &s_M};
}

// MC_NOISE: the log tables of the Box-Muller radius into the head's table as well -- stage_tables' copy, the even entries doubled
// on their way in --, behind the head's barrier and ending in one of its own.  (The head has room for them: its table is whole.)
__device__ __forceinline__ void stage_mc_log_tables(const pocs_tables* __restrict__ g, const pocs_tables* s_tab) {
  constexpr int NLG = (int)(sizeof(g->lg) / sizeof(double));
  const double* src = &g->lg[0][0];
  double* dst = const_cast<double*>(&s_tab->lg[0][0]);
  for (int j = threadIdx.x; j < NLG; j += POCS_BLOCK) dst[j] = (j & 1) == 0 ? 2.0 * src[j] : src[j];
  __syncthreads();
}

// MC kernels: blockIdx.y = run of the batch (its own seed, its own noisy controls, its own slice
// of the particle arrays).
struct mc_run_view {
  uint64_t seed;
  const double* chain;
  double* x; double* y; double* th;
  uint32_t* hits;
};
__device__ __forceinline__ mc_run_view mc_view(const pocs_mc_launch& a) {
  const int r = blockIdx.y;
  const size_t o = (size_t)r * (size_t)a.stride;
  mc_run_view v;
  v.seed = a.hdr[r].seed;
  v.chain = a.chain + (size_t)r * (a.W > 1 ? a.W - 1 : 1) * POCS_CHAIN_STRIDE;
  v.x = a.x + o; v.y = a.y + o; v.th = a.th + o; v.hits = a.hits + o;
  return v;
}

// Where run blockIdx.y starts and how many controls it drives (k_mc_fused): the launch's mu0 / step, or -- a call of
// plans -- its own plan's start and length (pocs_mc_launch::run_plan).
struct mc_run_start {
  double mu[3];
  int steps;
};
__device__ __forceinline__ mc_run_start mc_start(const pocs_mc_launch& a) {
  mc_run_start s;
  if (a.run_plan) {
    const double* q = a.run_plan + 4 * (size_t)blockIdx.y;
    s.mu[0] = q[0]; s.mu[1] = q[1]; s.mu[2] = q[2];
    s.steps = (int)q[3];
  } else {
    s.mu[0] = a.mu0[0]; s.mu[1] = a.mu0[1]; s.mu[2] = a.mu0[2];
    s.steps = a.step;
  }
  return s;
}

// First collisions per waypoint (POCS_OPT_MC_WAYPOINT_COUNTS, POCS_OPT_MC_RISK_BOUND).  The MC kernels have one body each,
// instantiated by MODE: MC_PLAIN is the kernel as it has always been (k_mc_init, k_mc_step, k_mc_fused: not one instruction
// more), MC_COUNTS also adds to wp_counts[run][w] the particles that collide at waypoint w and at no waypoint before it,
// MC_STOP (k_mc_step only) also obeys the risk bound.  A particle's first collision is read off the hit counter the kernel
// holds anyway (old == 0).  Integer counts added with integer atomics: exact, whatever the grid and the shard partition.
//
// MC_BOXES (POCS_OPT_OBSTACLE_COUNTS), a flag on top of MC_COUNTS or MC_STOP: the first collisions are also split by obstacle
// box -- obs_counts[run][w][m], the particles whose first collision is at waypoint w and which touch box m there (a particle
// that touches two boxes counts for both).  The collision test is then pocs_pose_collides_each, which hands out every record's
// answer; a thread keeps them as a 64-bit mask (POCS_MAX_OBSTACLES = 64: box 63 is bit 63), and the mask matters only for a
// particle with old == 0 && hit.  The forms without the flag are the kernels as they are.
//
// MC_CLEAR (pocs_set_clearance_levels), a flag on top of MC_PLAIN, MC_COUNTS or MC_STOP, on k_mc_init and the per-step kernel: every
// particle keeps one byte, the smallest clearance level it has been within so far (L: none yet), and a particle counts for every
// level between its new smallest level and its old one -- clr_counts[run][w][l], the particles within clearance d_l at waypoint w and
// at no waypoint before: the first-collision profile as it would be for the grown footprint on the same cloud.  The level comes
// from pocs_pose_clearance_level on the table prepared for the footprint grown by the largest clearance, staged beside the world's;
// the collision test itself, the hit counters and the other counts are what they are without the flag.
//
// MC_PARTS (pocs_set_footprint_parts with F > 1), a flag on top of MC_PLAIN, MC_COUNTS or MC_STOP, on k_mc_init and the per-step
// kernel: the collision test is pocs_pose_collides_parts over the parts staged beside the world's records (which are prepared for
// the largest part); the hit counters and the counts are formed from that flag as they are from the single footprint's.
//
// MC_REGIONS (pocs_set_regions), a flag on top of MC_PLAIN, MC_COUNTS or MC_STOP, on k_mc_init and the per-step kernel, never with
// MC_BOXES, MC_CLEAR or MC_PARTS: reg_counts[run][w][g] also counts the particles that have collided at no waypoint <= w and are in
// region g at w (pocs_pose_regions_mask on the regions staged beside the world's records).  No per-particle state: "never
// collided" is the hit counter the kernel holds anyway -- !hit in k_mc_init, old == 0 && !hit in the per-step kernel, which reads the
// counter of a particle that does not collide only when the particle is in some region.  The collision test, the hit counters
// and the other counts are what they are without the flag.
//
// MC_SEG (pocs_set_segment_checks with J > 1), a flag on top of MC_COUNTS or MC_STOP on the per-step kernel alone (waypoint 0 is the
// initial cloud: k_mc_init is what it is), never with MC_BOXES, MC_CLEAR, MC_PARTS or MC_REGIONS: a particle touches at waypoint
// s + 1 when its end pose (mc_move, unchanged) or one of the J - 1 sub-poses q_j = pocs_motion(p, {u[0], f_j u[1], 0.0}) on the way
// there touches the world of waypoint s + 1.  The end pose is tested first and the sub-poses only for a particle whose end pose is
// free: the OR needs nothing more, and seg_counts[run][s + 1] counts exactly that case -- the particles whose first touching
// waypoint this is and whose end pose is free.  The sine and cosine of the drive direction are mc_move's own (mc_move_dir).  J and
// the fractions are read from pocs_seg_dev in device memory (wave-uniform loads); hit counters and counts are formed from the flag.
//
// MC_ROUND (pocs_set_discs with D > 0), a flag on top of MC_PLAIN, MC_COUNTS or MC_STOP on k_mc_init and the per-step kernel, never
// with MC_BOXES, MC_CLEAR, MC_PARTS, MC_REGIONS or MC_SEG: the staged table may hold disc records behind its boxes, and the
// collision test is pocs_pose_collides<true>, which decides a record's kind by a wave-uniform branch.  Nothing else differs.
//
// MC_NOISE (pocs_set_disc_covariances with a nonzero row), a flag on top of MC_ROUND: a disc record whose row of the launch's noise
// table is not zero is tested on its displaced centre (pocs_pose_collides_noisy) -- the deviation drawn for (seed, global particle
// index first + i, disc, waypoint word), the word 0 at every waypoint under POCS_DISC_NOISE_PERSISTENT and the launch's waypoint
// otherwise.  The rows are read where they lie (wave-uniform addresses).  The head stages the sector table alone and the Box-Muller
// radius needs the log tables: these forms stage them behind the head (stage_mc_log_tables).  Nothing else differs.
//
// MC_RFOOT (pocs_set_footprint_disc), a flag on top of MC_ROUND and of MC_ROUND | MC_NOISE, for worlds with and without discs: the
// footprint is the disc of radius fp.hx centred on the particle, the collision test pocs_round_pose_collides (MC_NOISE:
// pocs_round_pose_collides_noisy, the same index, seed and waypoint word).  The heading is not looked at.  Nothing else differs.
//
// MC_HYP (pocs_set_disc_hypotheses), a flag on top of MC_ROUND and of MC_ROUND | MC_NOISE, never with MC_RFOOT: a disc record whose
// gate of the launch's gate table is on counts for the particles for which it exists (pocs_pose_collides_gated) -- the existence word
// drawn for (seed, global particle index first + i, group, word 0): a particle's world keeps its alternative for the whole
// roll-out.  The gates are read where they lie (wave-uniform addresses); without MC_NOISE no row is read and no log table staged.
//
// The bits themselves (enum MC_*): pocs_launch_forms.hpp, where the host chooses a launch's word.
static_assert(POCS_MAX_OBSTACLES <= 64, "a particle's touched boxes are a 64-bit mask");

// pocs_pose_collides with the touched boxes as a mask (the flag: mask != 0, as the plain form's).
__device__ __forceinline__ bool mc_collides_mask(double x, double y, double t, const pocs_footprint* fp, const double* obs, int M,
                                                 const pocs_tables* tab, unsigned long long& mask) {
  mask = 0ull;
  return pocs_pose_collides_each(x, y, t, fp, obs, M, tab, [&](const int m, const bool touched) { if (touched) mask |= 1ull << m; });
}

// The lanes of a wave that are in the particle loop together, `first` = a first collision at this waypoint with touched boxes
// `mask`: per box that any of them touches one ballot, and the first lane of the ballot adds its population count to dst[m]
// (the block's LDS counters, or -- the fused kernels -- the run's row in global memory, as mc_wave_first_hits does).  No first
// collision in the wave (nearly always): one ballot and a scalar branch.
__device__ __forceinline__ void mc_wave_box_hits(bool first, unsigned long long mask, int M, unsigned long long* dst) {
  if (__ballot(first) == 0ull) return;
  for (int m = 0; m < M; ++m) {
    const unsigned long long b = __ballot(first && ((mask >> m) & 1ull) != 0ull);
    if (b != 0ull && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(b)) atomicAdd(&dst[m], (unsigned long long)__popcll(b));
  }
}
// The block's LDS counters of the kernels that meet a block boundary per waypoint (k_mc_init, k_mc_step, k_mc_tree_step):
// zeroed in front of the head's barrier, and behind the particle loop the nonzero ones leave with one atomic each, thread m
// box m.
struct mc_box_counters {
  unsigned long long* c;
  __device__ __forceinline__ void out(int M, unsigned long long* row) const {
    __syncthreads();
    const int m = threadIdx.x;
    if (m < M) { const unsigned long long n = c[m]; if (n) atomicAdd(&row[m], n); }
  }
};
__device__ __forceinline__ mc_box_counters mc_box_counters_zeroed() {
  __shared__ unsigned long long s_box[POCS_MAX_OBSTACLES];
  if (threadIdx.x < POCS_MAX_OBSTACLES) s_box[threadIdx.x] = 0ull;
  return {s_box};
}

// A block's sum of counts -> dst[at]: every thread's own count, one wave sum, one word per wave in LDS, one atomic per block
// (integer: order independent, exact) and none when the sum is 0.  Every thread of the block arrives (behind its particle
// loop).  dst[at] is addressed by thread 0 alone, behind the barrier.
__device__ __forceinline__ void mc_block_add(unsigned c, unsigned long long* dst, size_t at = 0) {
  __shared__ unsigned s_c[POCS_BLOCK / 64];
  c = wave_sum_u32(c);
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < POCS_BLOCK / 64; ++w) t += s_c[w];
    if (t) atomicAdd(&dst[at], t);
  }
}

// The lanes of a wave that are in the particle loop together: those with a first collision at this waypoint, counted by
// ballot, added by the first of them.
__device__ __forceinline__ void mc_wave_first_hits(bool first, unsigned long long* dst) {
  const unsigned long long m = __ballot(first);
  if (m != 0ull && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(m)) atomicAdd(dst, (unsigned long long)__popcll(m));
}

// MC_CLEAR: what a thread keeps of the clearance record behind the head's barrier, and its staging (in front of that barrier).
struct mc_clear {
  const double* obs;               // LDS: the table prepared for the footprint grown by d[L - 1]
  const double* d;                 // LDS: the distances
  int L;
};
__device__ __forceinline__ mc_clear stage_mc_clear(const pocs_mc_launch& a) {
  __shared__ double s_obs2[POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];
  __shared__ double s_d[POCS_MAX_CLEARANCE_LEVELS];
  constexpr int NO = POCS_MAX_OBSTACLES * POCS_OBS_STRIDE, UO = (NO + POCS_BLOCK - 1) / POCS_BLOCK;
  const int tid = threadIdx.x;
  double vo[UO];
#pragma unroll
  for (int u = 0; u < UO; ++u) { const int i = tid + u * POCS_BLOCK; vo[u] = i < NO ? a.clr->obs[i] : 0.0; }
  const double dv = tid < POCS_MAX_CLEARANCE_LEVELS ? a.clr->d[tid] : 0.0;
  requests_issued();
#pragma unroll
  for (int u = 0; u < UO; ++u) { const int i = tid + u * POCS_BLOCK; if (i < NO) s_obs2[i] = vo[u]; }
  if (tid < POCS_MAX_CLEARANCE_LEVELS) s_d[tid] = dv;
  return {s_obs2, s_d, a.clr_L};
}
// MC_PARTS: the parts of the compound footprint in LDS, staged in front of the head's barrier.
struct mc_parts {
  const double* p;                 // LDS: F x POCS_PART_STRIDE
  int F;
};
__device__ __forceinline__ mc_parts stage_mc_parts(const pocs_mc_launch& a) {
  __shared__ double s_parts[POCS_MAX_FOOTPRINT_PARTS * POCS_PART_STRIDE];
  const int tid = threadIdx.x;
  const double v = tid < POCS_MAX_FOOTPRINT_PARTS * POCS_PART_STRIDE ? a.parts->part[tid] : 0.0;
  requests_issued();
  if (tid < POCS_MAX_FOOTPRINT_PARTS * POCS_PART_STRIDE) s_parts[tid] = v;
  return {s_parts, a.parts_F};
}
// The lanes of a wave that are in the particle loop together, each with its particle's level at this waypoint and its smallest
// level before: per level that some particle reaches for the first time one ballot, and the first lane of the ballot adds the
// population count to the level's counter of (run, waypoint), as mc_wave_first_hits does.
__device__ __forceinline__ void mc_wave_level_hits(int now, int before, int L, unsigned long long* dst) {
  if (__ballot(now < before) == 0ull) return;
  for (int l = 0; l < L; ++l) {
    const unsigned long long b = __ballot(now <= l && l < before);
    if (b != 0ull && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(b)) atomicAdd(&dst[l], (unsigned long long)__popcll(b));
  }
}

// MC_REGIONS: the regions' records and footprints in LDS, staged in front of the head's barrier.
struct mc_regions {
  const double* rec;               // LDS: G x POCS_OBS_STRIDE
  const double* fp;                // LDS: G x 4
  int G;
};
__device__ __forceinline__ mc_regions stage_mc_regions(const pocs_mc_launch& a) {
  __shared__ double s_reg[POCS_REGIONS_HEAD];
  static_assert(POCS_REGIONS_HEAD <= POCS_BLOCK && offsetof(pocs_regions_dev, fp) == POCS_MAX_REGIONS * POCS_OBS_STRIDE * sizeof(double),
                "one double of rec | fp per thread");
  const int tid = threadIdx.x;
  const double v = tid < POCS_REGIONS_HEAD ? reinterpret_cast<const double*>(a.regions)[tid] : 0.0;
  requests_issued();
  if (tid < POCS_REGIONS_HEAD) s_reg[tid] = v;
  return {s_reg, s_reg + POCS_MAX_REGIONS * POCS_OBS_STRIDE, a.reg_G};
}
// The lanes of a wave that are in the particle loop together, each with the regions its never-collided particle is in (0: none,
// or collided): per region one ballot, and the first lane of the ballot adds the population count to the region's counter of
// (run, waypoint), as mc_wave_level_hits does.  No such particle in the wave: one ballot and a scalar branch.
__device__ __forceinline__ void mc_wave_region_hits(unsigned in, int G, unsigned long long* dst) {
  if (__ballot(in != 0u) == 0ull) return;
  for (int g = 0; g < G; ++g) {
    const unsigned long long b = __ballot(((in >> g) & 1u) != 0u);
    if (b != 0ull && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(b)) atomicAdd(&dst[g], (unsigned long long)__popcll(b));
  }
}

// MC_STOP, the head of every block of the launch of control s: is the run stopped?  The run stops at the FIRST waypoint s
// whose cumulative count C[s] = F[0] + ... + F[s] has (double)C[s] / (double)N >= bound.  F[0..s] were completed by the
// EARLIER launches of the graph (control s - 1 wrote F[s]); this launch adds to F[s + 1] only, which nobody reads here: all
// blocks of the run see the same numbers and decide alike.  A stopped run's particles stay where they are, so its later
// launches find F[s + 1 ...] = 0, the same C and the same answer -- no block reads a word that a block of its own launch
// writes.  Block 0 of the launch that finds the bound reached for the first time (C[s - 1] was below it) reports s + 1 in the
// run's stop word, which only the host reads.
__device__ __forceinline__ bool mc_run_stopped(const pocs_mc_launch& a) {
  __shared__ unsigned long long s_c[POCS_BLOCK / 64];
  const int r = blockIdx.y, s = a.step;
  const unsigned long long* F = a.wp_counts + (size_t)r * (size_t)a.W;
  unsigned long long part = 0;
  for (int w = threadIdx.x; w <= s; w += POCS_BLOCK) part += F[w];
  // (a wave sum of 64-bit counts out of 32-bit ones: three pieces of 22 bits, 64 of which cannot overflow)
  const unsigned long long c = (unsigned long long)wave_sum_u32((unsigned)(part & 0x3FFFFFull)) +
                               ((unsigned long long)wave_sum_u32((unsigned)((part >> 22) & 0x3FFFFFull)) << 22) +
                               ((unsigned long long)wave_sum_u32((unsigned)(part >> 44)) << 44);
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
  __syncthreads();
  unsigned long long C = 0;
  for (int w = 0; w < POCS_BLOCK / 64; ++w) C += s_c[w];
  const double n = (double)a.wp_n;
  const bool stopped = (double)C / n >= a.wp_bound;
  if (stopped && blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned long long before = C - F[s];          // C[s - 1] (0 for s = 0: waypoint 0 is always evaluated)
    if (!((double)before / n >= a.wp_bound)) a.wp_stop[r] = (unsigned)s + 1u;
  }
  return stopped;
}

// Particle i of a run at waypoint 0: mu + L0 z, z its own three normals (initParticles).  The pose comes back through
// references, as mc_move's does: returned as a record, the compiler ordered the callers' instructions differently.
__device__ __forceinline__ void mc_initial(const pocs_mc_launch& a, uint64_t seed, long long i, const mc_run_start& st,
                                           double& x, double& y, double& t) {
  double z[3];
  uint32_t spare;
  pocs_normal3(seed, (uint64_t)(a.first + i), 0u, POCS_STREAM_MCINIT, z, &spare);
  x = fma(a.L0[0], z[0], st.mu[0]);
  y = fma(a.L0[2], z[1], fma(a.L0[1], z[0], st.mu[1]));
  t = fma(a.L0[5], z[2], fma(a.L0[4], z[1], fma(a.L0[3], z[0], st.mu[2])));
}

// The motion model (moveParticles): the pose (x, y, t) driven by the noisy control (u0, u1, u2) -- turn, drive, turn.  The new
// pose may be written over the old one (k_mc_fused).
__device__ __forceinline__ void mc_move(const double x, const double y, const double t, const double u0, const double u1,
                                        const double u2, double& nx, double& ny, double& nt) {
  double sn, cs;
  pocs_sincos(t + u0, &sn, &cs);
  nx = fma(u1, cs, x);
  ny = fma(u1, sn, y);
  nt = pocs_wrap_angle(t + u0 + u2);
}
// MC_SEG: mc_move with the drive direction's sine and cosine handed out (the same operations: the same pose).
__device__ __forceinline__ void mc_move_dir(const double x, const double y, const double t, const double u0, const double u1,
                                            const double u2, double& nx, double& ny, double& nt, double& sn, double& cs) {
  pocs_sincos(t + u0, &sn, &cs);
  nx = fma(u1, cs, x);
  ny = fma(u1, sn, y);
  nt = pocs_wrap_angle(t + u0 + u2);
}

// ---- a large collision world (pocs_set_world with more than POCS_MAX_OBSTACLES boxes; k_mc_init_world, k_mc_step_world) ----
// The particles of a block are not bounded ahead of time, so the table is culled per wave and particle iteration, against the box
// of the wave's 64 footprint centres (mc_world_collides).  Nothing of the table is staged: the head is the sector table and the
// footprint.
__device__ __forceinline__ mc_world stage_mc_head_world(const pocs_mc_launch& a) {
  __shared__ pocs_tables s_tab;
  constexpr int NS = (int)(sizeof(a.tables->sc) / sizeof(double)), US = (NS + POCS_BLOCK - 1) / POCS_BLOCK;
  const int tid = threadIdx.x;
  const double* src = &a.tables->sc[0][0];
  double vs[US];
#pragma unroll
  for (int u = 0; u < US; ++u) { const int i = tid + u * POCS_BLOCK; vs[u] = i < NS ? src[i] : 0.0; }
  const pocs_footprint fp = a.env->fp;
  requests_issued();
  double* dst = &s_tab.sc[0][0];
#pragma unroll
  for (int u = 0; u < US; ++u) { const int i = tid + u * POCS_BLOCK; if (i < NS) dst[i] = vs[u]; }
  __syncthreads();
  return {a.world, &s_tab, fp, a.world_M};
}
// the wave's minimum / maximum of v, in every lane (all 64 lanes active): row steps by DPP, the four rows through scalar registers
__device__ __forceinline__ double wave_min_f64(double v) {
  v = fmin(v, dpp_f64<0xB1>(v)); v = fmin(v, dpp_f64<0x4E>(v)); v = fmin(v, dpp_f64<0x141>(v)); v = fmin(v, dpp_f64<0x140>(v));
  return fmin(fmin(lane_value(v, 0), lane_value(v, 16)), fmin(lane_value(v, 32), lane_value(v, 48)));
}
__device__ __forceinline__ double wave_max_f64(double v) {
  v = fmax(v, dpp_f64<0xB1>(v)); v = fmax(v, dpp_f64<0x4E>(v)); v = fmax(v, dpp_f64<0x141>(v)); v = fmax(v, dpp_f64<0x140>(v));
  return fmax(fmax(lane_value(v, 0), lane_value(v, 16)), fmax(lane_value(v, 32), lane_value(v, 48)));
}
// pocs_pose_collides against a table of any length, for the 64 poses of a wave at once -- ALL 64 lanes arrive (the callers' particle
// loops run on a wave-uniform bound; a lane without a particle, `live` false, carries a dead pose that adds +-infinity to the
// bounds below and whose flag is dropped).  Per lane the footprint centre and the heading's sine and cosine exactly as
// pocs_pose_collides forms them (pocs_world_pose); the wave's bounding box of the centres; then per 64 records: lane l looks at
// record base + l and rejects it if the box cannot reach it (pocs_world_wave_rejects: exact, pocs_world.h), one ballot, and for
// every record left -- a scalar loop over the ballot's bits -- all lanes run pocs_box_hit on it through a wave-uniform pointer.
// Every record that is not rejected for the whole wave goes through pocs_box_hit itself: the flags of the full loop over M.
__device__ __forceinline__ bool mc_world_collides(const bool live, const double x, const double y, const double t, const mc_world& wd) {
  const int lane = threadIdx.x & 63;
  double px, py, sn, cs;
  pocs_world_pose(x, y, t, &wd.fp, wd.tab, &px, &py, &sn, &cs);
  const double inf = __builtin_inf();
  const double xlo = wave_min_f64(live ? px : inf), xhi = wave_max_f64(live ? px : -inf);
  const double ylo = wave_min_f64(live ? py : inf), yhi = wave_max_f64(live ? py : -inf);
  bool hit = false;
  for (int base = 0; base < wd.M; base += 64) {        // (wave-uniform)
    const int m = base + lane;
    bool cand = false;
    if (m < wd.M) {
      const double* o = wd.obs + (size_t)m * POCS_OBS_STRIDE;
      cand = !pocs_world_wave_rejects(o[0], o[1], o[6], o[7], xlo, xhi, ylo, yhi);
    }
    unsigned long long b = __ballot(cand);
    while (b != 0ull) {                                // (scalar)
      const int j = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(b));
      b &= b - 1ull;
      const double* o = wd.obs + (size_t)(base + j) * POCS_OBS_STRIDE;
      if (pocs_box_hit(px, py, sn, cs, wd.fp.hx, wd.fp.hy, o)) hit = true;
    }
  }
  return hit && live;
}

// WORLD (k_mc_init_world): the same particle, the same stores, the collision test against the large world; the loop runs on the
// wave's first index, so that every lane of a wave is at the cross-lane steps of mc_world_collides.
template <int MODE, bool WORLD = false>
__device__ __forceinline__ void mc_init_body(const pocs_mc_launch& a) {
  static_assert(WORLD && (MODE & MC_BOXES) == 0, "the body of k_mc_init_world; k_mc_init keeps its own");
  const mc_world wd = stage_mc_head_world(a);
  const mc_run_view v = mc_view(a);
  const mc_run_start st = mc_start(a);
  unsigned first = 0;
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * POCS_BLOCK;
  for (long long i0 = (long long)blockIdx.x * POCS_BLOCK + (threadIdx.x - lane); i0 < a.count; i0 += stride) {      // (wave-uniform)
    const long long i = i0 + lane;
    const bool live = i < a.count;
    double x = 0.0, y = 0.0, t = 0.0;
    if (live) {
      mc_initial(a, v.seed, i, st, x, y, t);
      v.x[i] = x; v.y[i] = y; v.th[i] = t;
    }
    const unsigned h = mc_world_collides(live, x, y, t, wd) ? 1u : 0u;
    if (live) v.hits[i] = h;
    first += h;
  }
  if (MODE != MC_PLAIN) mc_block_add(first, a.wp_counts + (size_t)blockIdx.y * (size_t)a.W);      // waypoint 0
}
template <int MODE>
__global__ __launch_bounds__(POCS_BLOCK) void k_mc_init_world(pocs_mc_launch a) { mc_init_body<MODE, true>(a); }

template <int MODE>
__global__ __launch_bounds__(POCS_BLOCK) void k_mc_init(pocs_mc_launch a) {
  mc_box_counters box = {nullptr};
  if constexpr ((MODE & MC_BOXES) != 0) box = mc_box_counters_zeroed();      // (in front of the head's barrier)
  mc_clear cl = {nullptr, nullptr, 0};
  if constexpr ((MODE & MC_CLEAR) != 0) cl = stage_mc_clear(a);              // (in front of the head's barrier)
  mc_parts pt = {nullptr, 0};
  if constexpr ((MODE & MC_PARTS) != 0) pt = stage_mc_parts(a);              // (in front of the head's barrier)
  mc_regions rg = {nullptr, nullptr, 0};
  if constexpr ((MODE & MC_REGIONS) != 0) rg = stage_mc_regions(a);          // (in front of the head's barrier)
  const mc_head hd = stage_mc_head(a.env, a.tables);
  if constexpr ((MODE & MC_NOISE) != 0) stage_mc_log_tables(a.tables, hd.tab);
  const mc_run_view v = mc_view(a);
  const mc_world wd = hd.world();
  const mc_run_start st = mc_start(a);
  unsigned first = 0;                              // this thread's particles that collide at waypoint 0 (unused: MC_PLAIN)
  const long long stride = (long long)gridDim.x * POCS_BLOCK;
  for (long long i = (long long)blockIdx.x * POCS_BLOCK + threadIdx.x; i < a.count; i += stride) {
    double x, y, t;
    mc_initial(a, v.seed, i, st, x, y, t);
    v.x[i] = x; v.y[i] = y; v.th[i] = t;
    unsigned h;
    if constexpr ((MODE & MC_BOXES) != 0) {
      unsigned long long mask;
      h = mc_collides_mask(x, y, t, &wd.fp, wd.obs, wd.M, wd.tab, mask) ? 1u : 0u;
      mc_wave_box_hits(h != 0u, mask, wd.M, box.c);
    } else if constexpr ((MODE & MC_PARTS) != 0) {
      h = pocs_pose_collides_parts(x, y, t, pt.p, pt.F, wd.obs, wd.M, wd.tab) ? 1u : 0u;
    } else if constexpr ((MODE & MC_HYP) != 0) {
      static_assert((MODE & MC_HYP) == 0 || ((MODE & MC_ROUND) != 0 && (MODE & (MC_BOXES | MC_CLEAR | MC_PARTS | MC_REGIONS | MC_SEG | MC_RFOOT)) == 0), "hypotheses: on top of MC_ROUND, with or without MC_NOISE");
      h = pocs_pose_collides_gated(x, y, t, &wd.fp, wd.obs, (MODE & MC_NOISE) != 0 ? a.noise : nullptr, a.gates, wd.M, v.seed, (uint64_t)(a.first + i), 0u, 0u, wd.tab) ? 1u : 0u;      // waypoint 0
    } else if constexpr ((MODE & MC_RFOOT) != 0) {
      static_assert((MODE & MC_RFOOT) == 0 || ((MODE & MC_ROUND) != 0 && (MODE & (MC_BOXES | MC_CLEAR | MC_PARTS | MC_REGIONS | MC_SEG)) == 0), "a round footprint: on top of MC_ROUND, with or without MC_NOISE");
      if constexpr ((MODE & MC_NOISE) != 0)
        h = pocs_round_pose_collides_noisy(x, y, wd.fp.hx, wd.obs, a.noise, wd.M, v.seed, (uint64_t)(a.first + i), 0u, wd.tab) ? 1u : 0u;      // waypoint 0
      else
        h = pocs_round_pose_collides(x, y, wd.fp.hx, wd.obs, wd.M) ? 1u : 0u;
    } else if constexpr ((MODE & MC_NOISE) != 0) {
      static_assert((MODE & MC_NOISE) == 0 || ((MODE & MC_ROUND) != 0 && (MODE & (MC_BOXES | MC_CLEAR | MC_PARTS | MC_REGIONS | MC_SEG)) == 0), "uncertain discs: on top of MC_ROUND alone");
      h = pocs_pose_collides_noisy(x, y, t, &wd.fp, wd.obs, a.noise, wd.M, v.seed, (uint64_t)(a.first + i), 0u, wd.tab) ? 1u : 0u;      // waypoint 0
    } else if constexpr ((MODE & MC_ROUND) != 0) {
      static_assert((MODE & MC_ROUND) == 0 || (MODE & (MC_BOXES | MC_CLEAR | MC_PARTS | MC_REGIONS | MC_SEG)) == 0, "round obstacles: on top of the three plain modes alone");
      h = pocs_pose_collides<true>(x, y, t, &wd.fp, wd.obs, wd.M, wd.tab) ? 1u : 0u;
    } else {
      h = pocs_pose_collides(x, y, t, &wd.fp, wd.obs, wd.M, wd.tab) ? 1u : 0u;
    }
    v.hits[i] = h;
    first += h;
    if constexpr ((MODE & MC_CLEAR) != 0) {
      const int lv = pocs_pose_clearance_level(x, y, t, &wd.fp, cl.d, cl.L, cl.obs, wd.M, wd.tab);
      a.clr_level[(size_t)blockIdx.y * (size_t)a.stride + (size_t)i] = (unsigned char)lv;
      mc_wave_level_hits(lv, cl.L, cl.L, a.clr_counts + (size_t)blockIdx.y * (size_t)a.W * POCS_MAX_CLEARANCE_LEVELS);
    }
    if constexpr ((MODE & MC_REGIONS) != 0) {
      const unsigned in = h != 0u ? 0u : pocs_pose_regions_mask(x, y, t, rg.rec, rg.fp, rg.G, wd.tab);
      mc_wave_region_hits(in, rg.G, a.reg_counts + (size_t)blockIdx.y * (size_t)a.W * POCS_MAX_REGIONS);
    }
  }
  if ((MODE & 3) != MC_PLAIN) mc_block_add(first, a.wp_counts + (size_t)blockIdx.y * (size_t)a.W);      // waypoint 0
  if constexpr ((MODE & MC_BOXES) != 0) box.out(wd.M, a.obs_counts + (size_t)blockIdx.y * (size_t)a.W * POCS_MAX_OBSTACLES);
}

// A particle's words in HBM.  NT: non-temporal accesses, chosen by the host when the particle state of the batch does not
// fit the 256 MB Infinity Cache anyway (the stream then runs faster past the caches; when it does fit, plain accesses keep
// it there between waypoint launches).
template <bool NT, typename T> __device__ __forceinline__ T mc_load(const T* p) { return NT ? __builtin_nontemporal_load(p) : *p; }
template <bool NT, typename T> __device__ __forceinline__ void mc_store(const T v, T* p) { if (NT) __builtin_nontemporal_store(v, p); else *p = v; }

// One particle per thread and iteration: a two-particle version with 16-byte accesses measured 12 % slower in cache, 7 %
// faster out of it.
//   WORLD (k_mc_step_world): the collision test against a large world (mc_world_collides), the particle loop on the wave's first
//   index so that every lane of a wave is at its cross-lane steps; MC_BOXES is not served there
template <bool NT, int MODE, bool WORLD = false>
__device__ __forceinline__ void mc_step_body(const pocs_mc_launch& a) {
  if ((MODE & 3) == MC_STOP) { if (mc_run_stopped(a)) return; }      // (the same answer in every thread of the block)
  if constexpr (WORLD) {
    static_assert(!WORLD || (MODE & MC_BOXES) == 0, "no per-box counts under a large world");
    const mc_world wd = stage_mc_head_world(a);
    const mc_run_view v = mc_view(a);
    const double* u = v.chain + (size_t)a.step * POCS_CHAIN_STRIDE + 6;
    const double u0 = u[0], u1 = u[1], u2 = u[2];
    unsigned first = 0;
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * POCS_BLOCK;
    for (long long i0 = (long long)blockIdx.x * POCS_BLOCK + (threadIdx.x - lane); i0 < a.count; i0 += stride) {      // (wave-uniform)
      const long long i = i0 + lane;
      const bool live = i < a.count;
      double nx = 0.0, ny = 0.0, nt = 0.0;
      if (live) {
        const double x = mc_load<NT>(v.x + i), y = mc_load<NT>(v.y + i), t = mc_load<NT>(v.th + i);
        mc_move(x, y, t, u0, u1, u2, nx, ny, nt);
        mc_store<NT>(nx, v.x + i); mc_store<NT>(ny, v.y + i); mc_store<NT>(nt, v.th + i);
      }
      if (mc_world_collides(live, nx, ny, nt, wd)) {
        const uint32_t old = v.hits[i];
        v.hits[i] = old + 1u;
        first += old == 0u ? 1u : 0u;
      }
    }
    if (MODE != MC_PLAIN) mc_block_add(first, a.wp_counts + (size_t)blockIdx.y * (size_t)a.W + (size_t)a.step + 1);
    return;
  }
  mc_box_counters box = {nullptr};
  if constexpr ((MODE & MC_BOXES) != 0) box = mc_box_counters_zeroed();      // (in front of the head's barrier)
  mc_clear cl = {nullptr, nullptr, 0};
  if constexpr ((MODE & MC_CLEAR) != 0) cl = stage_mc_clear(a);              // (in front of the head's barrier)
  mc_parts pt = {nullptr, 0};
  if constexpr ((MODE & MC_PARTS) != 0) pt = stage_mc_parts(a);              // (in front of the head's barrier)
  mc_regions rg = {nullptr, nullptr, 0};
  if constexpr ((MODE & MC_REGIONS) != 0) rg = stage_mc_regions(a);          // (in front of the head's barrier)
  const mc_head hd = stage_mc_head(a.env, a.tables);
  if constexpr ((MODE & MC_NOISE) != 0) stage_mc_log_tables(a.tables, hd.tab);
  const mc_run_view v = mc_view(a);
  const mc_world wd = hd.world();
  const double* u = v.chain + (size_t)a.step * POCS_CHAIN_STRIDE + 6;
  const double u0 = u[0], u1 = u[1], u2 = u[2];
  unsigned first = 0;                              // this thread's particles whose first collision is this waypoint (unused: MC_PLAIN)
  const long long stride = (long long)gridDim.x * POCS_BLOCK;
  if constexpr ((MODE & MC_SEG) != 0) {
    static_assert((MODE & MC_SEG) == 0 || ((MODE & (MC_BOXES | MC_CLEAR | MC_PARTS | MC_REGIONS)) == 0 && (MODE & 3) != MC_PLAIN),
                  "segment checks: on top of MC_COUNTS or MC_STOP alone");
    const double* const sf = a.seg->f;             // (wave-uniform: J and the fractions come through the scalar cache)
    const int J = a.seg->J;
    unsigned between = 0;                          // ... whose first touching waypoint this is and whose end pose is free
    for (long long i = (long long)blockIdx.x * POCS_BLOCK + threadIdx.x; i < a.count; i += stride) {
      const double x = mc_load<NT>(v.x + i), y = mc_load<NT>(v.y + i), t = mc_load<NT>(v.th + i);
      double nx, ny, nt, sn, cs;
      mc_move_dir(x, y, t, u0, u1, u2, nx, ny, nt, sn, cs);
      mc_store<NT>(nx, v.x + i); mc_store<NT>(ny, v.y + i); mc_store<NT>(nt, v.th + i);
      const bool end = pocs_pose_collides(nx, ny, nt, &wd.fp, wd.obs, wd.M, wd.tab);
      bool sub = false;
      if (!end) sub = pocs_segment_touched_dir(x, y, t + u0, sn, cs, u1, sf, J, 0, &wd.fp, wd.obs, wd.M, wd.tab) != 0u;
      if (end || sub) {
        const uint32_t old = v.hits[i];
        v.hits[i] = old + 1u;
        first += old == 0u ? 1u : 0u;
        between += (old == 0u && sub) ? 1u : 0u;
      }
    }
    mc_block_add(first, a.wp_counts + (size_t)blockIdx.y * (size_t)a.W + (size_t)a.step + 1);
    __syncthreads();                                 // (mc_block_add's scratch is read by thread 0 of the call above)
    mc_block_add(between, a.seg_counts + (size_t)blockIdx.y * (size_t)a.W + (size_t)a.step + 1);
    return;
  }
  for (long long i = (long long)blockIdx.x * POCS_BLOCK + threadIdx.x; i < a.count; i += stride) {
    const double x = mc_load<NT>(v.x + i), y = mc_load<NT>(v.y + i), t = mc_load<NT>(v.th + i);
    double nx, ny, nt;
    mc_move(x, y, t, u0, u1, u2, nx, ny, nt);
    mc_store<NT>(nx, v.x + i); mc_store<NT>(ny, v.y + i); mc_store<NT>(nt, v.th + i);
    if constexpr ((MODE & MC_BOXES) != 0) {
      unsigned long long mask;
      bool fresh = false;
      if (mc_collides_mask(nx, ny, nt, &wd.fp, wd.obs, wd.M, wd.tab, mask)) {
        const uint32_t old = v.hits[i];
        v.hits[i] = old + 1u;
        fresh = old == 0u;
        first += fresh ? 1u : 0u;
      }
      mc_wave_box_hits(fresh, mask, wd.M, box.c);
    } else if constexpr ((MODE & MC_PARTS) != 0) {
      if (pocs_pose_collides_parts(nx, ny, nt, pt.p, pt.F, wd.obs, wd.M, wd.tab)) {
        const uint32_t old = v.hits[i];
        v.hits[i] = old + 1u;
        first += old == 0u ? 1u : 0u;
      }
    } else if constexpr ((MODE & MC_REGIONS) != 0) {
      unsigned in = 0u;
      if (pocs_pose_collides(nx, ny, nt, &wd.fp, wd.obs, wd.M, wd.tab)) {
        const uint32_t old = v.hits[i];
        v.hits[i] = old + 1u;
        first += old == 0u ? 1u : 0u;
      } else {
        in = pocs_pose_regions_mask(nx, ny, nt, rg.rec, rg.fp, rg.G, wd.tab);
        if (in != 0u && v.hits[i] != 0u) in = 0u;      // (in a region, but collided at an earlier waypoint)
      }
      mc_wave_region_hits(in, rg.G, a.reg_counts + ((size_t)blockIdx.y * (size_t)a.W + (size_t)a.step + 1) * POCS_MAX_REGIONS);
    } else if constexpr ((MODE & MC_HYP) != 0) {
      static_assert((MODE & MC_HYP) == 0 || ((MODE & MC_ROUND) != 0 && (MODE & (MC_BOXES | MC_CLEAR | MC_PARTS | MC_REGIONS | MC_SEG | MC_RFOOT)) == 0), "hypotheses: on top of MC_ROUND, with or without MC_NOISE");
      const uint32_t vw = a.noise_persistent ? 0u : (uint32_t)(a.step + 1);      // (the deviations' word; the existence draws' is 0)
      if (pocs_pose_collides_gated(nx, ny, nt, &wd.fp, wd.obs, (MODE & MC_NOISE) != 0 ? a.noise : nullptr, a.gates, wd.M, v.seed, (uint64_t)(a.first + i), vw, 0u, wd.tab)) {
        const uint32_t old = v.hits[i];
        v.hits[i] = old + 1u;
        first += old == 0u ? 1u : 0u;
      }
    } else if constexpr ((MODE & MC_RFOOT) != 0) {
      static_assert((MODE & MC_RFOOT) == 0 || ((MODE & MC_ROUND) != 0 && (MODE & (MC_BOXES | MC_CLEAR | MC_PARTS | MC_REGIONS | MC_SEG)) == 0), "a round footprint: on top of MC_ROUND, with or without MC_NOISE");
      bool touch;
      if constexpr ((MODE & MC_NOISE) != 0) {
        const uint32_t vw = a.noise_persistent ? 0u : (uint32_t)(a.step + 1);      // control s produces waypoint s + 1
        touch = pocs_round_pose_collides_noisy(nx, ny, wd.fp.hx, wd.obs, a.noise, wd.M, v.seed, (uint64_t)(a.first + i), vw, wd.tab);
      } else {
        touch = pocs_round_pose_collides(nx, ny, wd.fp.hx, wd.obs, wd.M);
      }
      if (touch) {
        const uint32_t old = v.hits[i];
        v.hits[i] = old + 1u;
        first += old == 0u ? 1u : 0u;
      }
    } else if constexpr ((MODE & MC_NOISE) != 0) {
      static_assert((MODE & MC_NOISE) == 0 || ((MODE & MC_ROUND) != 0 && (MODE & (MC_BOXES | MC_CLEAR | MC_PARTS | MC_REGIONS | MC_SEG)) == 0), "uncertain discs: on top of MC_ROUND alone");
      const uint32_t vw = a.noise_persistent ? 0u : (uint32_t)(a.step + 1);      // control s produces waypoint s + 1
      if (pocs_pose_collides_noisy(nx, ny, nt, &wd.fp, wd.obs, a.noise, wd.M, v.seed, (uint64_t)(a.first + i), vw, wd.tab)) {
        const uint32_t old = v.hits[i];
        v.hits[i] = old + 1u;
        first += old == 0u ? 1u : 0u;
      }
    } else if constexpr ((MODE & MC_ROUND) != 0) {
      static_assert((MODE & MC_ROUND) == 0 || (MODE & (MC_BOXES | MC_CLEAR | MC_PARTS | MC_REGIONS | MC_SEG)) == 0, "round obstacles: on top of the three plain modes alone");
      if (pocs_pose_collides<true>(nx, ny, nt, &wd.fp, wd.obs, wd.M, wd.tab)) {
        const uint32_t old = v.hits[i];
        v.hits[i] = old + 1u;
        first += old == 0u ? 1u : 0u;
      }
    } else {
    if (pocs_pose_collides(nx, ny, nt, &wd.fp, wd.obs, wd.M, wd.tab)) {
      const uint32_t old = v.hits[i];                // the counter is in hand exactly when the particle collides
      v.hits[i] = old + 1u;
      first += old == 0u ? 1u : 0u;
    }
    }
    if constexpr ((MODE & MC_CLEAR) != 0) {
      unsigned char* const lp = a.clr_level + (size_t)blockIdx.y * (size_t)a.stride + (size_t)i;
      const int before = (int)*lp;
      const int lv = pocs_pose_clearance_level(nx, ny, nt, &wd.fp, cl.d, cl.L, cl.obs, wd.M, wd.tab);
      if (lv < before) *lp = (unsigned char)lv;
      mc_wave_level_hits(lv, before, cl.L, a.clr_counts + ((size_t)blockIdx.y * (size_t)a.W + (size_t)a.step + 1) * POCS_MAX_CLEARANCE_LEVELS);
    }
  }
  if ((MODE & 3) != MC_PLAIN) mc_block_add(first, a.wp_counts + (size_t)blockIdx.y * (size_t)a.W + (size_t)a.step + 1);   // control s -> waypoint s + 1
  if constexpr ((MODE & MC_BOXES) != 0) box.out(wd.M, a.obs_counts + ((size_t)blockIdx.y * (size_t)a.W + (size_t)a.step + 1) * POCS_MAX_OBSTACLES);
}
template <bool NT>
__global__ __launch_bounds__(POCS_BLOCK) void k_mc_step(pocs_mc_launch a) { mc_step_body<NT, MC_PLAIN>(a); }
template <bool NT, int MODE>
__global__ __launch_bounds__(POCS_BLOCK) void k_mc_step_counts(pocs_mc_launch a) { mc_step_body<NT, MODE>(a); }
template <bool NT, int MODE>
__global__ __launch_bounds__(POCS_BLOCK) void k_mc_step_world(pocs_mc_launch a) { mc_step_body<NT, MODE, true>(a); }

// MC_COUNTS: a particle has at most one first collision, so per step a wave ballots them and one lane adds the wave's count,
// only when there is one (no block-level sum: the blocks of a fused launch never meet between steps).
template <int MODE>
__device__ __forceinline__ void mc_fused_body(const pocs_mc_launch& a) {
  const mc_head hd = stage_mc_head(a.env, a.tables);
  const mc_run_view v = mc_view(a);
  const mc_world wd = hd.world();
  const mc_run_start st = mc_start(a);             // (its steps: uniform per block, blockIdx.y being the run)
  unsigned long long* wp = MODE != MC_PLAIN ? a.wp_counts + (size_t)blockIdx.y * (size_t)a.W : nullptr;
  const long long stride = (long long)gridDim.x * POCS_BLOCK;
  for (long long i = (long long)blockIdx.x * POCS_BLOCK + threadIdx.x; i < a.count; i += stride) {
    double x, y, t;
    mc_initial(a, v.seed, i, st, x, y, t);
    unsigned long long* const bx = (MODE & MC_BOXES) != 0 ? a.obs_counts + (size_t)blockIdx.y * (size_t)a.W * POCS_MAX_OBSTACLES : nullptr;
    unsigned h;
    if constexpr ((MODE & MC_BOXES) != 0) {
      unsigned long long mask;
      h = mc_collides_mask(x, y, t, &wd.fp, wd.obs, wd.M, wd.tab, mask) ? 1u : 0u;
      mc_wave_box_hits(h != 0u, mask, wd.M, bx);
    } else {
      h = pocs_pose_collides(x, y, t, &wd.fp, wd.obs, wd.M, wd.tab) ? 1u : 0u;
    }
    if (MODE != MC_PLAIN) mc_wave_first_hits(h != 0u, wp);
    for (int s = 0; s < st.steps; ++s) {
      const double* u = v.chain + (size_t)s * POCS_CHAIN_STRIDE + 6;   // wave-uniform
      const double u0 = u[0], u1 = u[1], u2 = u[2];
      mc_move(x, y, t, u0, u1, u2, x, y, t);
      bool hit;
      if constexpr ((MODE & MC_BOXES) != 0) {
        unsigned long long mask;
        hit = mc_collides_mask(x, y, t, &wd.fp, wd.obs, wd.M, wd.tab, mask);
        mc_wave_box_hits(hit && h == 0u, mask, wd.M, bx + (size_t)(s + 1) * POCS_MAX_OBSTACLES);
      } else {
        hit = pocs_pose_collides(x, y, t, &wd.fp, wd.obs, wd.M, wd.tab);
      }
      if (MODE != MC_PLAIN) mc_wave_first_hits(hit && h == 0u, wp + s + 1);
      h += hit ? 1u : 0u;
    }
    v.x[i] = x; v.y[i] = y; v.th[i] = t;
    v.hits[i] = h;
  }
}
__global__ __launch_bounds__(POCS_BLOCK) void k_mc_fused(pocs_mc_launch a) { mc_fused_body<MC_PLAIN>(a); }
__global__ __launch_bounds__(POCS_BLOCK) void k_mc_fused_counts(pocs_mc_launch a) { mc_fused_body<MC_COUNTS>(a); }
__global__ __launch_bounds__(POCS_BLOCK) void k_mc_fused_boxes(pocs_mc_launch a) { mc_fused_body<MC_COUNTS | MC_BOXES>(a); }

// The fused roll-out under an obstacle schedule (pocs_set_obstacle_schedule, S = env_steps > 1): waypoint w is tested against
// record min(w, S - 1) of the env array, so a block cannot stage one world and keep it.  Step-outer per tile of POCS_BLOCK
// particles, one particle per thread in registers; the world of the current waypoint in one of TWO LDS buffers.  The M records
// of the next waypoint (the next tile's waypoint 0 behind a tile's last) are requested BEFORE the current waypoint's move and
// collision test and stored into the other buffer behind it: the requests are in flight while the step computes, and a step
// costs one block barrier, not a memory round trip.  The other buffer was last read one waypoint ago, in front of the previous
// barrier.  Every thread of a block makes the same trips through both loops (the tile loop runs on the block's first index,
// the steps are the run's: blockIdx.y); a thread without a particle only stages.  Footprint and M are the same in every
// record.  Per particle and waypoint the arithmetic of mc_fused_body through the same functions: the same bits.
template <int MODE>
__global__ __launch_bounds__(POCS_BLOCK) void k_mc_fused_sched(pocs_mc_launch a) {
  constexpr int NO = POCS_MAX_OBSTACLES * POCS_OBS_STRIDE, NS = (int)(sizeof(a.tables->sc) / sizeof(double));
  constexpr int UO = (NO + POCS_BLOCK - 1) / POCS_BLOCK, US = (NS + POCS_BLOCK - 1) / POCS_BLOCK;
  __shared__ double s_obs[2][NO];
  __shared__ pocs_tables s_tab;
  const int tid = threadIdx.x;
  {                                                    // the head: world 0 and the sector table, as stage_mc_head stages them
    const double* src = &a.tables->sc[0][0];
    double vo[UO], vs[US];
#pragma unroll
    for (int u = 0; u < UO; ++u) { const int j = tid + u * POCS_BLOCK; vo[u] = j < NO ? a.env->obs[j] : 0.0; }
#pragma unroll
    for (int u = 0; u < US; ++u) { const int j = tid + u * POCS_BLOCK; vs[u] = j < NS ? src[j] : 0.0; }
    requests_issued();
    double* dst = &s_tab.sc[0][0];
#pragma unroll
    for (int u = 0; u < UO; ++u) { const int j = tid + u * POCS_BLOCK; if (j < NO) s_obs[0][j] = vo[u]; }
#pragma unroll
    for (int u = 0; u < US; ++u) { const int j = tid + u * POCS_BLOCK; if (j < NS) dst[j] = vs[u]; }
  }
  const pocs_footprint fp = a.env->fp;
  const int M = a.env->M < POCS_MAX_OBSTACLES ? a.env->M : POCS_MAX_OBSTACLES, nrec = M * POCS_OBS_STRIDE;
  const int last = a.env_steps - 1;
  __syncthreads();
  const mc_run_view v = mc_view(a);
  const mc_run_start st = mc_start(a);             // (its steps: uniform per block, blockIdx.y being the run)
  unsigned long long* wp = MODE != MC_PLAIN ? a.wp_counts + (size_t)blockIdx.y * (size_t)a.W : nullptr;
  unsigned long long* const bx = (MODE & MC_BOXES) != 0 ? a.obs_counts + (size_t)blockIdx.y * (size_t)a.W * POCS_MAX_OBSTACLES : nullptr;
  int cur = 0;                                     // the buffer that holds the current waypoint's world
  const long long stride = (long long)gridDim.x * POCS_BLOCK;
  for (long long base = (long long)blockIdx.x * POCS_BLOCK; base < a.count; base += stride) {      // (block-uniform)
    const long long i = base + tid;
    const bool live = i < a.count;
    double x = 0.0, y = 0.0, t = 0.0, u0 = 0.0, u1 = 0.0, u2 = 0.0;
    unsigned h = 0;
    for (int w = 0; w <= st.steps; ++w) {
      // what the NEXT waypoint needs -- its control (control w produces waypoint w + 1) and its world's records -- is requested
      // here and first used behind this waypoint's test.  No request sits in a branch (a lane past the M records asks for
      // record 0 again, and a tile's last waypoint for control 0): the only wait of the step is the one in front of the stores
      const double* nu = v.chain + (size_t)(w < st.steps ? w : 0) * POCS_CHAIN_STRIDE + 6;   // wave-uniform
      const double n0 = nu[0], n1 = nu[1], n2 = nu[2];
      const int nw = w < st.steps ? w + 1 : 0;
      const double* nsrc = a.env[nw < last ? nw : last].obs;
      double vo[UO];
#pragma unroll
      for (int q = 0; q < UO; ++q) { const int j = tid + q * POCS_BLOCK; vo[q] = nsrc[j < nrec ? j : 0]; }
      requests_issued();
      if (live) {
        if (w == 0) mc_initial(a, v.seed, i, st, x, y, t);
        else mc_move(x, y, t, u0, u1, u2, x, y, t);
        bool hit;
        if constexpr ((MODE & MC_BOXES) != 0) {
          unsigned long long mask;
          hit = mc_collides_mask(x, y, t, &fp, s_obs[cur], M, &s_tab, mask);
          mc_wave_box_hits(hit && h == 0u, mask, M, bx + (size_t)w * POCS_MAX_OBSTACLES);
        } else {
          hit = pocs_pose_collides(x, y, t, &fp, s_obs[cur], M, &s_tab);
        }
        if (MODE != MC_PLAIN) mc_wave_first_hits(hit && h == 0u, wp + w);
        h += hit ? 1u : 0u;
      }
      requests_issued();
      u0 = n0; u1 = n1; u2 = n2;
#pragma unroll
      for (int q = 0; q < UO; ++q) { const int j = tid + q * POCS_BLOCK; if (j < nrec) s_obs[cur ^ 1][j] = vo[q]; }
      __syncthreads();
      cur ^= 1;
    }
    if (live) {
      v.x[i] = x; v.y[i] = y; v.th[i] = t;
      v.hits[i] = h;
    }
  }
}

// A tree of plans (pocs_set_plan_tree), one launch per level (at most 256 nodes per launch): blockIdx.y = node of the launch,
// slot r = tree_lo + blockIdx.y.  The node's particles are its PARENT's, moved by the noisy control of the edge into the node
// (chain[r], one record per node) -- mc_step_body's arithmetic -- read from the parent's place in the previous level's half of
// the particle buffers and written to the node's place in this level's half: source != destination, two levels live at a
// time.  Counted per node: the particles whose FIRST collision on the path root -> node is at the node (wp_counts[r]) and
// those that have collided at or before it (total[r]); integer atomics, exact whatever the grid.
//   BOXES (k_mc_tree_step_boxes, POCS_OPT_OBSTACLE_COUNTS): ... and the node's first collisions by obstacle box, obs_counts[r].
template <bool NT, bool BOXES>
__device__ __forceinline__ void mc_tree_step_body(const pocs_mc_launch& a) {
  mc_box_counters box = {nullptr};
  if constexpr (BOXES) box = mc_box_counters_zeroed();      // (in front of the head's barrier)
  const mc_head hd = stage_mc_head(a.env, a.tables);
  const int r = a.tree_lo + (int)blockIdx.y, pr = a.tree_parent[r];
  const size_t so = (size_t)(pr - a.tree_src_lo) * (size_t)a.stride, dso = (size_t)(r - a.tree_dst_lo) * (size_t)a.stride;
  const double* sx = a.tree_sx + so; const double* sy = a.tree_sy + so; const double* st = a.tree_sth + so;
  const uint32_t* sh = a.tree_shits + so;
  double* dx = a.x + dso; double* dy = a.y + dso; double* dt = a.th + dso;
  uint32_t* dh = a.hits + dso;
  const mc_world wd = hd.world();
  const double* u = a.chain + (size_t)r * POCS_CHAIN_STRIDE + 6;
  const double u0 = u[0], u1 = u[1], u2 = u[2];
  unsigned first = 0, coll = 0;
  const long long stride = (long long)gridDim.x * POCS_BLOCK;
  for (long long i = (long long)blockIdx.x * POCS_BLOCK + threadIdx.x; i < a.count; i += stride) {
    const double x = mc_load<NT>(sx + i), y = mc_load<NT>(sy + i), t = mc_load<NT>(st + i);
    const uint32_t old = mc_load<NT>(sh + i);
    double nx, ny, nt;
    mc_move(x, y, t, u0, u1, u2, nx, ny, nt);
    uint32_t h;
    if constexpr (BOXES) {
      unsigned long long mask;
      const bool hit = mc_collides_mask(nx, ny, nt, &wd.fp, wd.obs, wd.M, wd.tab, mask);
      h = old + (hit ? 1u : 0u);
      mc_wave_box_hits(hit && old == 0u, mask, wd.M, box.c);
    } else {
      h = old + (pocs_pose_collides(nx, ny, nt, &wd.fp, wd.obs, wd.M, wd.tab) ? 1u : 0u);
    }
    mc_store<NT>(nx, dx + i); mc_store<NT>(ny, dy + i); mc_store<NT>(nt, dt + i); mc_store<NT>(h, dh + i);
    first += (old == 0u && h != 0u) ? 1u : 0u;
    coll += h != 0u ? 1u : 0u;
  }
  mc_block_add(first, a.wp_counts + r);
  __syncthreads();                                   // (mc_block_add's scratch is read by thread 0 of the call above)
  mc_block_add(coll, a.total + r);
  if constexpr (BOXES) box.out(wd.M, a.obs_counts + (size_t)r * POCS_MAX_OBSTACLES);
}
template <bool NT>
__global__ __launch_bounds__(POCS_BLOCK) void k_mc_tree_step(pocs_mc_launch a) { mc_tree_step_body<NT, false>(a); }
template <bool NT>
__global__ __launch_bounds__(POCS_BLOCK) void k_mc_tree_step_boxes(pocs_mc_launch a) { mc_tree_step_body<NT, true>(a); }

__global__ __launch_bounds__(POCS_BLOCK) void k_mc_count(pocs_mc_launch a) {
  const mc_run_view v = mc_view(a);
  unsigned c = 0;
  const long long stride = (long long)gridDim.x * POCS_BLOCK;
  for (long long i = (long long)blockIdx.x * POCS_BLOCK + threadIdx.x; i < a.count; i += stride)
    c += v.hits[i] > 0u ? 1u : 0u;
  mc_block_add(c, a.total, blockIdx.y);
}

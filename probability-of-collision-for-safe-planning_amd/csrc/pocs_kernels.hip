// pocs_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the hot path: the ONE unit of the library that holds
// device code (one gfx950 code object).  The kernels live in its parts, by family, included below in this order; this
// file keeps what the host runtime calls (pocs_launch_*, pocs_kernels.h, the test hooks' pocs_launch_probe_* among them), k_zero_counts
// and the bandwidth kernels k_copy and k_fill.  A pocs_launch_* that has a choice of kernels -- the GMM sampling launch, the MC path's
// init, step and fused roll-out, the two tree steps -- does not make it here: it asks its chooser in pocs_launch_forms.hpp (host only;
// precedence of the features, what each needs, refuses and checks), looks the answer's kernel up in the tables below (gmm_kernel_of,
// mc_kernel_of: the list of the hot path's instantiations) and launches that.
//
//   pocs_dev_prims.hpp    wave sums, table staging, write-through / L1-bypassing / non-temporal accessors, the hand-off
//                         fences, the diagnostic hooks                                           (relies on nothing)
//   pocs_dev_advance.hpp  k_gmm_advance, k_gmm_tree_advance, k_gmm_exchange: the mixture advance and the one-hop
//                         exchange of a run's moments between the GPUs of a node                 (prims)
//   pocs_dev_gmm.hpp      k_gmm_step, k_gmm_step_risk, k_gmm_step_tree, k_gmm_close: one waypoint of truncateGMM in one
//                         launch -- sampling, collision test, moment sums, closer; k_world_cull, k_gmm_step_world,
//                         k_gmm_step_risk_world: the same under a large collision world          (prims, advance)
//   pocs_dev_mc.hpp       k_mc_init, k_mc_step, k_mc_fused, k_mc_fused_sched, k_mc_tree_step, k_mc_count, and k_mc_init_world,
//                         k_mc_step_world under a large collision world                          (prims)
//   pocs_dev_probe.hpp    the eleven k_probe_* kernels of the test hooks (pocs_probe.hip), with the one staging helper and the
//                         one pair walk that the seven pair probes share; nothing of the hot path   (prims, gmm, mc)
//
// Bound: these are FP64-VALU / HBM streaming kernels, no contraction => no MFMA.  Mixture
// parameters, the obstacle table and the 12 KB of log/sector tables are staged in LDS once per
// block (all lanes read the same obstacle record => LDS broadcast; the per-lane component and
// table lookups are 16-byte reads).  Reductions are DPP row sums followed by one LDS pass and a
// per-block partial row; partials are combined in a fixed order so results are bitwise
// reproducible run to run (no float atomics).
#include "pocs_kernels.h"
#include <type_traits>
#include <stdio.h>

namespace {
#include "pocs_dev_prims.hpp"
#include "pocs_dev_advance.hpp"
#include "pocs_dev_gmm.hpp"
#include "pocs_dev_mc.hpp"
#include "pocs_dev_probe.hpp"

// The number of Gaussians as a compile-time constant: f(std::integral_constant<int, K>) for K in 1 .. POCS_MAX_GAUSSIANS.
template <typename F>
hipError_t with_K(const int K, F f) {
  static_assert(POCS_MAX_GAUSSIANS == 8, "one case per K");
  switch (K) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    case 5: return f(std::integral_constant<int, 5>());
    case 6: return f(std::integral_constant<int, 6>());
    case 7: return f(std::integral_constant<int, 7>());
    case 8: return f(std::integral_constant<int, 8>());
    default: return hipErrorInvalidValue;
  }
}

// From a form (pocs_launch_forms.hpp: the chooser's answer) to its kernel.  The tables below ARE the list of the hot path's
// instantiations -- an address taken here is what emits one --, and a form that has no entry has no kernel: null, a refusal.
using gmm_kernel = void (*)(pocs_gmm_launch);
using mc_kernel = void (*)(pocs_mc_launch);
namespace pf = pocs_forms;
static_assert(pf::kMaxGaussians == POCS_MAX_GAUSSIANS && pf::kMaxObstacles == POCS_MAX_OBSTACLES && pf::kMaxClearanceLevels == POCS_MAX_CLEARANCE_LEVELS &&
              pf::kMaxFootprintParts == POCS_MAX_FOOTPRINT_PARTS && pf::kMaxRegions == POCS_MAX_REGIONS && pf::kMaxWorldRecords == POCS_MAX_WORLD_RECORDS,
              "the choosers check the library's limits");
template <int K>
gmm_kernel gmm_kernel_of(const pf::Form f) {
  constexpr int TB = POCS_GMM_BLOCK_OF(K);
  switch (f.fam) {
#define STORE_LONE(k) case pf::k: { static constexpr gmm_kernel t[] = {k<K, false, TB, false>, k<K, true, TB, false>, k<K, false, TB, true>, k<K, true, TB, true>}; return t[f.store + 2 * f.lone]; }
#define STORE(k) case pf::k: { static constexpr gmm_kernel t[] = {k<K, false, TB>, k<K, true, TB>}; return t[f.store]; }
#define RISK(k) case pf::k: { static constexpr gmm_kernel t[] = {k<K, TB, false>, k<K, TB, true>}; return t[f.risk]; }
    STORE_LONE(k_gmm_step) STORE(k_gmm_step_risk) STORE_LONE(k_gmm_step_boxes) STORE(k_gmm_step_risk_boxes)
    STORE(k_gmm_step_world) STORE(k_gmm_step_risk_world) STORE(k_gmm_step_clear) STORE(k_gmm_step_risk_clear)
    STORE(k_gmm_step_regions) STORE(k_gmm_step_risk_regions) STORE(k_gmm_step_parts) STORE(k_gmm_step_risk_parts)
    STORE(k_gmm_step_seg) STORE(k_gmm_step_risk_seg) STORE(k_gmm_step_round) STORE(k_gmm_step_risk_round)
    STORE(k_gmm_step_noise) STORE(k_gmm_step_risk_noise) STORE(k_gmm_step_rfoot) STORE(k_gmm_step_risk_rfoot)
    STORE(k_gmm_step_rfoot_noise) STORE(k_gmm_step_risk_rfoot_noise)
    RISK(k_gmm_step_tree) RISK(k_gmm_step_tree_boxes)
    case pf::k_gmm_step_hyp: return k_gmm_step_hyp<K, TB>;                 // (stored or not: the launch's word, read by the kernel)
    case pf::k_gmm_step_risk_hyp: return k_gmm_step_risk_hyp<K, TB>;
    default: return nullptr;
#undef STORE_LONE
#undef STORE
#undef RISK
  }
}
// The MC form words that have a kernel: every mode (k_mc_init: the two it has) under each word of FEATURE_WORDS; the counting modes
// alone, with and without MC_BOXES and (the per-step kernel) MC_SEG; the bare modes under a large world and an obstacle schedule.
#define FEATURE_WORDS(MODES, X, k)                                                                                                        \
  MODES(X, k, MC_CLEAR) MODES(X, k, MC_PARTS) MODES(X, k, MC_REGIONS) MODES(X, k, MC_ROUND) MODES(X, k, MC_ROUND | MC_NOISE)                \
  MODES(X, k, MC_ROUND | MC_RFOOT) MODES(X, k, MC_ROUND | MC_NOISE | MC_RFOOT) MODES(X, k, MC_ROUND | MC_HYP) MODES(X, k, MC_ROUND | MC_NOISE | MC_HYP)
#define MODES_2(X, k, w) X(k, MC_PLAIN | (w)) X(k, MC_COUNTS | (w))
#define MODES_3(X, k, w) MODES_2(X, k, w) X(k, MC_STOP | (w))
#define WORD(k, w) case (w): return k<(w)>;
#define NT_WORD(k, w) case (w): { static constexpr mc_kernel t[] = {k<false, (w)>, k<true, (w)>}; return t[f.nt]; }
#define NT(k) case pf::k: { static constexpr mc_kernel t[] = {k<false>, k<true>}; return t[f.nt]; }
mc_kernel mc_kernel_of(const pf::Form f) {
  switch (f.fam) {
    case pf::k_mc_init:
      switch (f.word) { MODES_2(WORD, k_mc_init, 0) WORD(k_mc_init, MC_COUNTS | MC_BOXES) FEATURE_WORDS(MODES_2, WORD, k_mc_init) default: return nullptr; }
    case pf::k_mc_init_world:
      switch (f.word) { MODES_2(WORD, k_mc_init_world, 0) default: return nullptr; }
    NT(k_mc_step)
    case pf::k_mc_step_counts:
      switch (f.word) {
        NT_WORD(k_mc_step_counts, MC_COUNTS) NT_WORD(k_mc_step_counts, MC_STOP) NT_WORD(k_mc_step_counts, MC_COUNTS | MC_BOXES) NT_WORD(k_mc_step_counts, MC_STOP | MC_BOXES)
        NT_WORD(k_mc_step_counts, MC_COUNTS | MC_SEG) NT_WORD(k_mc_step_counts, MC_STOP | MC_SEG) FEATURE_WORDS(MODES_3, NT_WORD, k_mc_step_counts)
        default: return nullptr;
      }
    case pf::k_mc_step_world:
      switch (f.word) { MODES_3(NT_WORD, k_mc_step_world, 0) default: return nullptr; }
    case pf::k_mc_fused: return k_mc_fused;
    case pf::k_mc_fused_counts: return k_mc_fused_counts;
    case pf::k_mc_fused_boxes: return k_mc_fused_boxes;
    case pf::k_mc_fused_sched:
      switch (f.word) { MODES_2(WORD, k_mc_fused_sched, 0) WORD(k_mc_fused_sched, MC_COUNTS | MC_BOXES) default: return nullptr; }
    NT(k_mc_tree_step) NT(k_mc_tree_step_boxes)
    default: return nullptr;
  }
}
#undef FEATURE_WORDS
#undef MODES_2
#undef MODES_3
#undef WORD
#undef NT_WORD
#undef NT
// The one launch of a chosen kernel.
template <typename L>
hipError_t launch_form(void (*const kernel)(L), const dim3 grid, const dim3 block, hipStream_t s, const L& a) {
  if (!kernel) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, grid, block, 0, s, a);
  return hipGetLastError();
}
}  // namespace

#ifdef POCS_TUNING
#define POCS_TUNING_REPORT
#include "pocs_tuning.h"
#endif

// One waypoint's sampling launch.  Which kernel, and which records are refused: pocs_forms::gmm_step_form.
hipError_t pocs_launch_gmm_step(int K, const pocs_gmm_launch& a, hipStream_t s) {
  const pf::Form f = pf::gmm_step_form(K, a);
  if (!f) return hipErrorInvalidValue;
  return with_K(K, [&](auto k) {
    constexpr int KK = decltype(k)::value, TB = POCS_GMM_BLOCK_OF(KK);
    return launch_form(gmm_kernel_of<KK>(f), dim3(a.blocks), dim3(TB), s, a);
  });
}
// The cull of a large world in front of a waypoint's sampling launch: one block per run of the launch's run range.
hipError_t pocs_launch_world_cull(int K, const pocs_gmm_launch& a, hipStream_t s) {
  if (!a.world || a.world_M < 1 || a.world_M > POCS_MAX_WORLD_RECORDS || !a.kept || !a.kept_idx || !a.reach || !a.param || a.run_cnt < 1 ||
      a.run_lo < 0 || a.run_lo + a.run_cnt > a.nruns || a.waypoint < 0 || a.waypoint >= a.W || (a.risk && !a.stop))
    return hipErrorInvalidValue;
  return with_K(K, [&](auto k) {
    pocs_gmm_launch c = a;
    if (!a.risk) c.stop = nullptr;                     // (the kernel reads the stop word where there is one)
    hipLaunchKernelGGL((k_world_cull<decltype(k)::value>), dim3(a.run_cnt), dim3(POCS_CULL_BLOCK), 0, s, c);
    return hipGetLastError();
  });
}
hipError_t pocs_launch_gmm_close(int K, const pocs_gmm_launch& a, hipStream_t s) {
  return with_K(K, [&](auto k) {
    hipLaunchKernelGGL((k_gmm_close<decltype(k)::value>), dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
  });
}
hipError_t pocs_launch_gmm_exchange(int K, const pocs_gmm_launch& a, const pocs_xchg_dev& x, hipStream_t s) {
  hipLaunchKernelGGL(k_gmm_exchange, dim3(a.nruns), dim3(128), 0, s, a, x, K);
  return hipGetLastError();
}
hipError_t pocs_launch_gmm_advance(int K, const pocs_gmm_launch& a, hipStream_t s) {
  hipLaunchKernelGGL(k_gmm_advance, dim3(a.nruns), dim3(128), 0, s, a, K);
  return hipGetLastError();
}

// One level of a tree of plans: the sampling launch over nodes [run_lo, run_lo + run_cnt) of depth a.waypoint.  The rows are
// one per node: the launch must address them with W = 1 (TREE, gmm_step_block), and nothing may ask its closers for more than
// the node's sums (no advance, no exchange, no stored samples).
hipError_t pocs_launch_gmm_tree_step(int K, const pocs_gmm_launch& a, hipStream_t s) {
  const pf::Form f = pf::gmm_tree_step_form(K, a);
  if (!f) return hipErrorInvalidValue;
  return with_K(K, [&](auto k) {
    constexpr int KK = decltype(k)::value, TB = POCS_GMM_BLOCK_OF(KK);
    return launch_form(gmm_kernel_of<KK>(f), dim3(a.blocks), dim3(TB), s, a);
  });
}
// ... and the launch that builds the level's mixtures ahead of it: one block per node, grid = a.run_cnt.
hipError_t pocs_launch_gmm_tree_advance(int K, const pocs_gmm_launch& a, hipStream_t s) {
  if (a.W != 1 || !a.tree_parent || a.run_cnt < 1 || a.run_lo < 0 || a.run_lo + a.run_cnt > a.nruns || (a.risk && (!a.stop || !a.surv)) ||
      K < 1 || K > POCS_MAX_GAUSSIANS)
    return hipErrorInvalidValue;
  if (a.risk) hipLaunchKernelGGL(k_gmm_tree_advance<true>, dim3(a.run_cnt), dim3(128), 0, s, a, K);
  else        hipLaunchKernelGGL(k_gmm_tree_advance<false>, dim3(a.run_cnt), dim3(128), 0, s, a, K);
  return hipGetLastError();
}
// One level of a tree of plans on the MC path: grid (nblk, a.nruns), a.nruns = the launch's nodes, slots tree_lo ...
hipError_t pocs_launch_mc_tree_step(int nblk, const pocs_mc_launch& a, hipStream_t s) {
  const pf::Form f = pf::mc_tree_step_form(a);
  return f ? launch_form(mc_kernel_of(f), dim3(nblk, a.nruns), dim3(POCS_BLOCK), s, a) : hipErrorInvalidValue;
}

// The MC path's launches, all on grid (nblk, a.nruns): the initial cloud, one control, the fused roll-out (pocs_forms::mc_*_form).
hipError_t pocs_launch_mc_init(int nblk, const pocs_mc_launch& a, hipStream_t s) {
  const pf::Form f = pf::mc_init_form(a);
  return f ? launch_form(mc_kernel_of(f), dim3(nblk, a.nruns), dim3(POCS_BLOCK), s, a) : hipErrorInvalidValue;
}
hipError_t pocs_launch_mc_step(int nblk, const pocs_mc_launch& a, hipStream_t s) {
  const pf::Form f = pf::mc_step_form(a);
  return f ? launch_form(mc_kernel_of(f), dim3(nblk, a.nruns), dim3(POCS_BLOCK), s, a) : hipErrorInvalidValue;
}
hipError_t pocs_launch_mc_fused(int nblk, const pocs_mc_launch& a, hipStream_t s) {
  const pf::Form f = pf::mc_fused_form(a);
  return f ? launch_form(mc_kernel_of(f), dim3(nblk, a.nruns), dim3(POCS_BLOCK), s, a) : hipErrorInvalidValue;
}
hipError_t pocs_launch_mc_count(int nblk, const pocs_mc_launch& a, hipStream_t s) {
  hipLaunchKernelGGL(k_mc_count, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
  return hipGetLastError();
}

// The per-obstacle counts of a call start at zero (POCS_OPT_OBSTACLE_COUNTS): a kernel, so that the replayed graph -- kernel
// nodes only -- zeroes them itself.
__global__ __launch_bounds__(POCS_BLOCK) void k_zero_counts(unsigned long long* __restrict__ p, size_t n) {
  const size_t stride = (size_t)gridDim.x * POCS_BLOCK;
  for (size_t i = (size_t)blockIdx.x * POCS_BLOCK + threadIdx.x; i < n; i += stride) p[i] = 0ull;
}
hipError_t pocs_launch_zero_counts(unsigned long long* p, size_t words, hipStream_t s) {
  if (!p) return hipErrorInvalidValue;
  if (words == 0) return hipSuccess;
  const size_t nb = (words + POCS_BLOCK - 1) / POCS_BLOCK;
  hipLaunchKernelGGL(k_zero_counts, dim3((unsigned)(nb < POCS_MAX_BLOCKS ? nb : POCS_MAX_BLOCKS)), dim3(POCS_BLOCK), 0, s, p, words);
  return hipGetLastError();
}

// Plain streaming copy: the measured HBM ceiling the streaming kernels are compared with next to
// the datasheet peak (bench.py "copy_GBps").  Four 16-byte non-temporal loads in flight per lane,
// 8192 blocks: the best of the variants in tools/ubench/copy_rates.hip (6.0-6.2 TB/s read + written;
// one plain load per lane on 2048 blocks stops at 4.9).
__global__ __launch_bounds__(POCS_BLOCK) void k_copy(const double2* __restrict__ src, double2* __restrict__ dst, long long n) {
  typedef double v2d __attribute__((ext_vector_type(2)));
  const v2d* s = reinterpret_cast<const v2d*>(src);
  v2d* d = reinterpret_cast<v2d*>(dst);
  const long long stride = (long long)gridDim.x * POCS_BLOCK * 4;
  for (long long i = (long long)blockIdx.x * POCS_BLOCK * 4 + threadIdx.x; i < n; i += stride) {
    v2d v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) if (i + u * POCS_BLOCK < n) v[u] = __builtin_nontemporal_load(s + i + u * POCS_BLOCK);
#pragma unroll
    for (int u = 0; u < 4; ++u) if (i + u * POCS_BLOCK < n) __builtin_nontemporal_store(v[u], d + i + u * POCS_BLOCK);
  }
}
// Plain streaming FILL: what a write-only stream reaches on this GPU -- the GMM kernels read nothing, so
// this, not the copy rate, is the bandwidth ceiling they could run into (bench.py "fill_GBps").
__global__ __launch_bounds__(POCS_BLOCK) void k_fill(double2* __restrict__ dst, long long n, double v) {
  typedef double v2d __attribute__((ext_vector_type(2)));
  v2d* d = reinterpret_cast<v2d*>(dst);
  const v2d x = {v, v};
  const long long stride = (long long)gridDim.x * POCS_BLOCK * 4;
  for (long long i = (long long)blockIdx.x * POCS_BLOCK * 4 + threadIdx.x; i < n; i += stride) {
#pragma unroll
    for (int u = 0; u < 4; ++u) if (i + u * POCS_BLOCK < n) __builtin_nontemporal_store(x, d + i + u * POCS_BLOCK);
  }
}
// The test hooks' launches (pocs_probe.hip calls them): the kernels are pocs_dev_probe.hpp's, one block each but for the sweep of
// the radius roots and the cases of the counts.
hipError_t pocs_launch_probe_math(const pocs_tables* tables, int n, const uint32_t* wr, const uint32_t* wa, const double* x, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_probe_math, dim3(1), dim3(POCS_BLOCK), 0, s, tables, n, wr, wa, x, out);
  return hipGetLastError();
}
hipError_t pocs_launch_probe_radius_roots(const pocs_tables* tables, uint32_t first, unsigned long long count, unsigned long long* out, hipStream_t s) {
  if (!tables || !out || count < 1 || (unsigned long long)first + count > (1ull << 32)) return hipErrorInvalidValue;
  const unsigned long long nb = (count + POCS_BLOCK - 1) / POCS_BLOCK;
  hipLaunchKernelGGL(k_probe_radius_roots, dim3((unsigned)(nb < POCS_MAX_BLOCKS ? nb : POCS_MAX_BLOCKS)), dim3(POCS_BLOCK), 0, s, tables, first, count, out);
  return hipGetLastError();
}
hipError_t pocs_launch_probe_collide(int K, const pocs_gmm_launch& a, int n, const double* x, const double* y, const double* th,
                                     int* flags, int* nkeep, double* kept, hipStream_t s) {
  if (n < 1 || a.M < 0 || a.M > POCS_MAX_OBSTACLES || !a.env || !a.tables || !a.param) return hipErrorInvalidValue;
  return with_K(K, [&](auto k) {
    constexpr int KK = decltype(k)::value, TB = POCS_GMM_BLOCK_OF(KK);
    hipLaunchKernelGGL((k_probe_collide<KK, TB>), dim3(1), dim3(TB), 0, s, a, n, x, y, th, flags, nkeep, kept);
    return hipGetLastError();
  });
}
hipError_t pocs_launch_probe_clearance(const pocs_env_dev* env, const pocs_clear_dev* clr, int L, const pocs_tables* tables, int n,
                                       const double* x, const double* y, const double* th, int* level_out, hipStream_t s) {
  if (!env || !clr || !tables || n < 1 || L < 0 || L > POCS_MAX_CLEARANCE_LEVELS || !x || !y || !th || !level_out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_clearance, dim3(1), dim3(POCS_BLOCK), 0, s, env, clr, L, tables, n, x, y, th, level_out);
  return hipGetLastError();
}
hipError_t pocs_launch_probe_parts(const pocs_env_dev* env, const pocs_parts_dev* parts, int F, const pocs_tables* tables, int n,
                                   const double* x, const double* y, const double* th, int* touched_out, hipStream_t s) {
  if (!env || !parts || !tables || n < 1 || F < 1 || F > POCS_MAX_FOOTPRINT_PARTS || !x || !y || !th || !touched_out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_parts, dim3(1), dim3(POCS_BLOCK), 0, s, env, parts, F, tables, n, x, y, th, touched_out);
  return hipGetLastError();
}
hipError_t pocs_launch_probe_regions(const pocs_regions_dev* regions, int G, const pocs_tables* tables, int n,
                                     const double* x, const double* y, const double* th, int* mask_out, hipStream_t s) {
  if (!regions || !tables || n < 1 || G < 0 || G > POCS_MAX_REGIONS || !x || !y || !th || !mask_out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_regions, dim3(1), dim3(POCS_BLOCK), 0, s, regions, G, tables, n, x, y, th, mask_out);
  return hipGetLastError();
}
hipError_t pocs_launch_probe_segment(const pocs_env_dev* env, const pocs_seg_dev* seg, const pocs_tables* tables, double u0, double u1,
                                     double u2, int backward, int n, const double* x, const double* y, const double* th, int* mask_out,
                                     hipStream_t s) {
  if (!env || !seg || !tables || n < 1 || !x || !y || !th || !mask_out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_segment, dim3(1), dim3(POCS_BLOCK), 0, s, env, seg, tables, u0, u1, u2, backward ? 1 : 0, n, x, y, th, mask_out);
  return hipGetLastError();
}
hipError_t pocs_launch_probe_counts(int n, const int* K, const double* w, const double* alive, const unsigned long long* seeds, const uint32_t* wp,
                                    const double* n_total, double* out, hipStream_t s) {
  if (n < 1 || n > (1 << 20) || !K || !w || !alive || !seeds || !wp || !n_total || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_counts, dim3((unsigned)((n + POCS_BLOCK - 1) / POCS_BLOCK)), dim3(POCS_BLOCK), 0, s, n, K, w, alive, seeds, wp, n_total, out);
  return hipGetLastError();
}
hipError_t pocs_launch_probe_discs(const pocs_env_dev* env, const pocs_tables* tables, int n, const double* x, const double* y,
                                   const double* th, int* out, hipStream_t s) {
  if (!env || !tables || n < 1 || !x || !y || !th || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_discs, dim3(1), dim3(POCS_BLOCK), 0, s, env, tables, n, x, y, th, out);
  return hipGetLastError();
}
hipError_t pocs_launch_probe_disc_noise(const pocs_env_dev* env, const double* rows, const pocs_tables* tables, unsigned long long seed,
                                        unsigned v, unsigned long long first, int n, const double* x, const double* y, const double* th,
                                        double* centres, unsigned* flags, hipStream_t s) {
  if (!env || !rows || !tables || n < 1 || (first & 1ull) || !x || !y || !th || !centres || !flags) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_disc_noise, dim3(1), dim3(POCS_BLOCK), 0, s, env, rows, tables, seed, v, first, n, x, y, th, centres, flags);
  return hipGetLastError();
}
hipError_t pocs_launch_probe_disc_hypotheses(const pocs_env_dev* env, const double* rows, const uint32_t* gates, const pocs_tables* tables,
                                             unsigned long long seed, unsigned v, unsigned long long first, int n, const double* x,
                                             const double* y, const double* th, unsigned* exists, unsigned* flags, hipStream_t s) {
  if (!env || !rows || !gates || !tables || n < 1 || (first & 1ull) || !x || !y || !th || !exists || !flags) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_disc_hypotheses, dim3(1), dim3(POCS_BLOCK), 0, s, env, rows, gates, tables, seed, v, first, n, x, y, th, exists, flags);
  return hipGetLastError();
}
hipError_t pocs_launch_probe_footprint_disc(const pocs_env_dev* env, const double* rows, const pocs_tables* tables, unsigned long long seed,
                                            unsigned v, unsigned long long first, int n, const double* x, const double* y, int* out,
                                            hipStream_t s) {
  if (!env || !tables || n < 1 || (first & 1ull) || !x || !y || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_footprint_disc, dim3(1), dim3(POCS_BLOCK), 0, s, env, rows, tables, seed, v, first, n, x, y, out);
  return hipGetLastError();
}
hipError_t pocs_launch_fill(void* dst, long long bytes, hipStream_t s) {
  hipLaunchKernelGGL(k_fill, dim3(8192), dim3(POCS_BLOCK), 0, s, (double2*)dst, bytes / 16, 1.5);
  return hipGetLastError();
}
hipError_t pocs_launch_copy(const void* src, void* dst, long long bytes, hipStream_t s) {
  hipLaunchKernelGGL(k_copy, dim3(8192), dim3(POCS_BLOCK), 0, s, (const double2*)src, (double2*)dst, bytes / 16);
  return hipGetLastError();
}

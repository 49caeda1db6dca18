// pocs_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the hot path: the ONE unit of the library that holds
// device code (one gfx950 code object).  The kernels live in its parts, by family, included below in this order; this
// file keeps what the host runtime calls (pocs_launch_*, pocs_kernels.h) and the test and bandwidth kernels.
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
}  // namespace

#ifdef POCS_TUNING
#define POCS_TUNING_REPORT
#include "pocs_tuning.h"
#endif

hipError_t pocs_launch_gmm_step(int K, const pocs_gmm_launch& a, hipStream_t s) {
  return with_K(K, [&](auto k) {
    constexpr int KK = decltype(k)::value, TB = POCS_GMM_BLOCK_OF(KK);
    if (a.rfoot) {                                     // a round footprint: a family of its own, with and without discs and covariances
      if (a.lone || a.obs_counts || a.world || a.tree_parent || a.exchange_in_tail || a.clr || a.parts || a.regions || a.seg ||
          a.M > POCS_MAX_OBSTACLES || (a.risk && (!a.stop || !a.surv)) || !(a.fp.dx == 0.0 && a.fp.dy == 0.0 && a.fp.hx == a.fp.hy && a.fp.hx >= 0.0))
        return hipErrorInvalidValue;
      if (a.noise) {
        if (a.risk) {
          if (a.store) hipLaunchKernelGGL((k_gmm_step_risk_rfoot_noise<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
          else         hipLaunchKernelGGL((k_gmm_step_risk_rfoot_noise<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        } else {
          if (a.store) hipLaunchKernelGGL((k_gmm_step_rfoot_noise<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
          else         hipLaunchKernelGGL((k_gmm_step_rfoot_noise<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        }
      } else if (a.risk) {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_risk_rfoot<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_risk_rfoot<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      } else {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_rfoot<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_rfoot<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      }
    } else
    if (a.noise) {                                     // uncertain discs: the _noise forms on top of the _round forms
      if (!a.round || a.lone || a.obs_counts || a.world || a.tree_parent || a.exchange_in_tail || a.clr || a.parts || a.regions || a.seg ||
          a.M > POCS_MAX_OBSTACLES || (a.risk && (!a.stop || !a.surv)))
        return hipErrorInvalidValue;
      if (a.risk) {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_risk_noise<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_risk_noise<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      } else {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_noise<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_noise<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      }
    } else
    if (a.round) {                                     // round obstacles: the ticket forms whose table may hold disc records
      if (a.lone || a.obs_counts || a.world || a.tree_parent || a.exchange_in_tail || a.clr || a.parts || a.regions || a.seg ||
          a.M > POCS_MAX_OBSTACLES || (a.risk && (!a.stop || !a.surv)))
        return hipErrorInvalidValue;
      if (a.risk) {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_risk_round<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_risk_round<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      } else {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_round<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_round<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      }
    } else
    if (a.seg) {                                       // segment checks: the ticket forms that also test the sub-poses on the way in
      if (a.lone || a.obs_counts || a.world || a.tree_parent || a.exchange_in_tail || a.clr || a.parts || a.regions || !a.seg_counts || !a.chain ||
          a.M > POCS_MAX_OBSTACLES || (a.risk && (!a.stop || !a.surv)))
        return hipErrorInvalidValue;
      if (a.risk) {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_risk_seg<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_risk_seg<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      } else {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_seg<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_seg<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      }
    } else
    if (a.parts) {                                     // a compound footprint: the ticket forms that test every part
      if (a.lone || a.obs_counts || a.world || a.tree_parent || a.exchange_in_tail || a.clr || a.parts_F < 2 || a.parts_F > POCS_MAX_FOOTPRINT_PARTS ||
          a.M > POCS_MAX_OBSTACLES || (a.risk && (!a.stop || !a.surv)))
        return hipErrorInvalidValue;
      if (a.risk) {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_risk_parts<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_risk_parts<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      } else {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_parts<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_parts<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      }
    } else
    if (a.regions) {                                   // watched regions: the ticket forms that also count per region
      if (a.lone || a.obs_counts || a.world || a.tree_parent || a.exchange_in_tail || a.clr || !a.reg_counts || a.reg_G < 1 || a.reg_G > POCS_MAX_REGIONS ||
          a.M > POCS_MAX_OBSTACLES || (a.risk && (!a.stop || !a.surv)))
        return hipErrorInvalidValue;
      if (a.risk) {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_risk_regions<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_risk_regions<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      } else {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_regions<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_regions<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      }
    } else
    if (a.clr) {                                       // clearance levels: the ticket forms that also count per level
      if (a.lone || a.obs_counts || a.world || a.tree_parent || a.exchange_in_tail || !a.clr_counts || a.clr_L < 1 || a.clr_L > POCS_MAX_CLEARANCE_LEVELS ||
          a.M > POCS_MAX_OBSTACLES || (a.risk && (!a.stop || !a.surv)))
        return hipErrorInvalidValue;
      if (a.risk) {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_risk_clear<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_risk_clear<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      } else {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_clear<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_clear<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      }
    } else
    if (a.world) {                                     // a large world: the ticket forms that fetch what k_world_cull has left
      if (a.lone || a.obs_counts || a.exchange_in_tail || a.tree_parent || !a.kept || !a.reach || a.M != 0 ||
          (a.risk && (!a.stop || !a.surv)))
        return hipErrorInvalidValue;
      if (a.risk) {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_risk_world<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_risk_world<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      } else {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_world<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_world<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      }
    } else
    if (a.obs_counts) {                                // POCS_OPT_OBSTACLE_COUNTS: the same choice among the counting forms
      if (a.M > POCS_MAX_OBSTACLES) return hipErrorInvalidValue;
      if (a.risk) {
        if (a.lone || a.exchange_in_tail || !a.stop || !a.surv) return hipErrorInvalidValue;
        if (a.store) hipLaunchKernelGGL((k_gmm_step_risk_boxes<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_risk_boxes<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      } else if (a.lone) {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_boxes<KK, true, TB, true>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_boxes<KK, false, TB, true>), dim3(a.blocks), dim3(TB), 0, s, a);
      } else {
        if (a.store) hipLaunchKernelGGL((k_gmm_step_boxes<KK, true, TB, false>), dim3(a.blocks), dim3(TB), 0, s, a);
        else         hipLaunchKernelGGL((k_gmm_step_boxes<KK, false, TB, false>), dim3(a.blocks), dim3(TB), 0, s, a);
      }
    } else if (a.risk) {
      if (a.lone || a.exchange_in_tail || !a.stop || !a.surv) return hipErrorInvalidValue;
      if (a.store) hipLaunchKernelGGL((k_gmm_step_risk<KK, true, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
      else         hipLaunchKernelGGL((k_gmm_step_risk<KK, false, TB>), dim3(a.blocks), dim3(TB), 0, s, a);
    } else if (a.lone) {
      if (a.store) hipLaunchKernelGGL((k_gmm_step<KK, true, TB, true>), dim3(a.blocks), dim3(TB), 0, s, a);
      else         hipLaunchKernelGGL((k_gmm_step<KK, false, TB, true>), dim3(a.blocks), dim3(TB), 0, s, a);
    } else {
      if (a.store) hipLaunchKernelGGL((k_gmm_step<KK, true, TB, false>), dim3(a.blocks), dim3(TB), 0, s, a);
      else         hipLaunchKernelGGL((k_gmm_step<KK, false, TB, false>), dim3(a.blocks), dim3(TB), 0, s, a);
    }
    return hipGetLastError();
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
  if (a.W != 1 || !a.tree_parent || a.lone || a.store || a.advance_in_tail || a.exchange_in_tail || a.run_cnt < 1 || a.run_cnt > 256 ||
      a.run_lo < 0 || a.run_lo + a.run_cnt > a.nruns || (a.risk && (!a.stop || !a.surv)))
    return hipErrorInvalidValue;
  return with_K(K, [&](auto k) {
    constexpr int KK = decltype(k)::value, TB = POCS_GMM_BLOCK_OF(KK);
    if (a.obs_counts) {
      if (a.risk) hipLaunchKernelGGL((k_gmm_step_tree_boxes<KK, TB, true>), dim3(a.blocks), dim3(TB), 0, s, a);
      else        hipLaunchKernelGGL((k_gmm_step_tree_boxes<KK, TB, false>), dim3(a.blocks), dim3(TB), 0, s, a);
    } else if (a.risk) hipLaunchKernelGGL((k_gmm_step_tree<KK, TB, true>), dim3(a.blocks), dim3(TB), 0, s, a);
    else               hipLaunchKernelGGL((k_gmm_step_tree<KK, TB, false>), dim3(a.blocks), dim3(TB), 0, s, a);
    return hipGetLastError();
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
  if (a.world) return hipErrorInvalidValue;
  if (!a.tree_parent || !a.tree_sx || !a.tree_sy || !a.tree_sth || !a.tree_shits || !a.wp_counts || !a.total || a.nruns < 1 || a.nruns > 256 ||
      a.tree_dst_lo < 1 || a.tree_lo < a.tree_dst_lo || a.tree_src_lo < 0 || a.tree_src_lo >= a.tree_dst_lo || a.tree_sx == a.x)
    return hipErrorInvalidValue;
  const dim3 grid(nblk, a.nruns), block(POCS_BLOCK);
  if (a.obs_counts) {
    if (a.nontemporal) hipLaunchKernelGGL(k_mc_tree_step_boxes<true>, grid, block, 0, s, a);
    else               hipLaunchKernelGGL(k_mc_tree_step_boxes<false>, grid, block, 0, s, a);
  } else if (a.nontemporal) hipLaunchKernelGGL(k_mc_tree_step<true>, grid, block, 0, s, a);
  else                      hipLaunchKernelGGL(k_mc_tree_step<false>, grid, block, 0, s, a);
  return hipGetLastError();
}

hipError_t pocs_launch_mc_init(int nblk, const pocs_mc_launch& a, hipStream_t s) {
  if ((a.wp_mode != 0 && !a.wp_counts) || (a.obs_counts && !a.wp_mode)) return hipErrorInvalidValue;
  if (a.rfoot) {                                      // a round footprint: MC_RFOOT on top of MC_ROUND, with or without MC_NOISE
    if (!a.round || a.world || a.obs_counts || a.clr || a.parts || a.regions || a.seg) return hipErrorInvalidValue;
    if (a.noise) {
      if (a.wp_mode) hipLaunchKernelGGL(k_mc_init<MC_COUNTS | MC_ROUND | MC_NOISE | MC_RFOOT>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
      else           hipLaunchKernelGGL(k_mc_init<MC_PLAIN | MC_ROUND | MC_NOISE | MC_RFOOT>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
    } else {
      if (a.wp_mode) hipLaunchKernelGGL(k_mc_init<MC_COUNTS | MC_ROUND | MC_RFOOT>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
      else           hipLaunchKernelGGL(k_mc_init<MC_PLAIN | MC_ROUND | MC_RFOOT>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
    }
  } else
  if (a.noise) {                                      // uncertain discs: the MC_NOISE forms on top of the MC_ROUND forms
    if (!a.round || a.world || a.obs_counts || a.clr || a.parts || a.regions || a.seg) return hipErrorInvalidValue;
    if (a.wp_mode) hipLaunchKernelGGL(k_mc_init<MC_COUNTS | MC_ROUND | MC_NOISE>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
    else           hipLaunchKernelGGL(k_mc_init<MC_PLAIN | MC_ROUND | MC_NOISE>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
  } else
  if (a.round) {                                      // round obstacles: the MC_ROUND forms (a small world, no counts per box, level or region, one footprint box)
    if (a.world || a.obs_counts || a.clr || a.parts || a.regions || a.seg) return hipErrorInvalidValue;
    if (a.wp_mode) hipLaunchKernelGGL(k_mc_init<MC_COUNTS | MC_ROUND>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
    else           hipLaunchKernelGGL(k_mc_init<MC_PLAIN | MC_ROUND>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
  } else
  if (a.parts) {                                      // a compound footprint: the MC_PARTS forms (a small world, no per-box counts, no levels)
    if (a.world || a.obs_counts || a.clr || a.parts_F < 2 || a.parts_F > POCS_MAX_FOOTPRINT_PARTS) return hipErrorInvalidValue;
    if (a.wp_mode) hipLaunchKernelGGL(k_mc_init<MC_COUNTS | MC_PARTS>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
    else           hipLaunchKernelGGL(k_mc_init<MC_PLAIN | MC_PARTS>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
  } else
  if (a.regions) {                                    // watched regions: the MC_REGIONS forms (a small world, no per-box counts, levels or parts)
    if (a.world || a.obs_counts || a.clr || !a.reg_counts || a.reg_G < 1 || a.reg_G > POCS_MAX_REGIONS) return hipErrorInvalidValue;
    if (a.wp_mode) hipLaunchKernelGGL(k_mc_init<MC_COUNTS | MC_REGIONS>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
    else           hipLaunchKernelGGL(k_mc_init<MC_PLAIN | MC_REGIONS>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
  } else
  if (a.clr) {                                        // clearance levels: the MC_CLEAR forms (a small world, no per-box counts)
    if (a.world || a.obs_counts || !a.clr_counts || !a.clr_level || a.clr_L < 1 || a.clr_L > POCS_MAX_CLEARANCE_LEVELS) return hipErrorInvalidValue;
    if (a.wp_mode) hipLaunchKernelGGL(k_mc_init<MC_COUNTS | MC_CLEAR>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
    else           hipLaunchKernelGGL(k_mc_init<MC_PLAIN | MC_CLEAR>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
  } else
  if (a.world) {                                      // a large world (no per-box counts there)
    if (a.obs_counts || a.world_M < 1 || a.world_M > POCS_MAX_WORLD_RECORDS) return hipErrorInvalidValue;
    if (a.wp_mode) hipLaunchKernelGGL(k_mc_init_world<MC_COUNTS>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
    else           hipLaunchKernelGGL(k_mc_init_world<MC_PLAIN>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
  } else
  if (a.obs_counts) hipLaunchKernelGGL(k_mc_init<MC_COUNTS | MC_BOXES>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
  else if (a.wp_mode) hipLaunchKernelGGL(k_mc_init<MC_COUNTS>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
  else           hipLaunchKernelGGL(k_mc_init<MC_PLAIN>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
  return hipGetLastError();
}
hipError_t pocs_launch_mc_step(int nblk, const pocs_mc_launch& a, hipStream_t s) {
  const dim3 grid(nblk, a.nruns), block(POCS_BLOCK);
  if ((a.wp_mode != 0 && !a.wp_counts) || (a.obs_counts && !a.wp_mode)) return hipErrorInvalidValue;
  if (a.rfoot) {                                      // a round footprint: the MC_RFOOT forms of the three modes, with or without MC_NOISE
    if (!a.round || a.world || a.obs_counts || a.clr || a.parts || a.regions || a.seg || a.step < 0 || a.step + 1 >= a.W ||
        (a.wp_mode == 2 && (!a.wp_stop || a.wp_n < 1)))
      return hipErrorInvalidValue;
    constexpr int RF = MC_ROUND | MC_RFOOT, RFN = MC_ROUND | MC_NOISE | MC_RFOOT;
    if (a.noise) {
      if (a.wp_mode == 2) {
        if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_STOP | RFN>), grid, block, 0, s, a);
        else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_STOP | RFN>), grid, block, 0, s, a);
      } else if (a.wp_mode == 1) {
        if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_COUNTS | RFN>), grid, block, 0, s, a);
        else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_COUNTS | RFN>), grid, block, 0, s, a);
      } else {
        if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_PLAIN | RFN>), grid, block, 0, s, a);
        else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_PLAIN | RFN>), grid, block, 0, s, a);
      }
    } else if (a.wp_mode == 2) {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_STOP | RF>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_STOP | RF>), grid, block, 0, s, a);
    } else if (a.wp_mode == 1) {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_COUNTS | RF>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_COUNTS | RF>), grid, block, 0, s, a);
    } else {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_PLAIN | RF>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_PLAIN | RF>), grid, block, 0, s, a);
    }
  } else
  if (a.noise) {                                      // uncertain discs: the MC_NOISE forms of the three modes
    if (!a.round || a.world || a.obs_counts || a.clr || a.parts || a.regions || a.seg || a.step < 0 || a.step + 1 >= a.W ||
        (a.wp_mode == 2 && (!a.wp_stop || a.wp_n < 1)))
      return hipErrorInvalidValue;
    if (a.wp_mode == 2) {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_STOP | MC_ROUND | MC_NOISE>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_STOP | MC_ROUND | MC_NOISE>), grid, block, 0, s, a);
    } else if (a.wp_mode == 1) {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_COUNTS | MC_ROUND | MC_NOISE>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_COUNTS | MC_ROUND | MC_NOISE>), grid, block, 0, s, a);
    } else {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_PLAIN | MC_ROUND | MC_NOISE>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_PLAIN | MC_ROUND | MC_NOISE>), grid, block, 0, s, a);
    }
  } else
  if (a.round) {                                      // round obstacles: the MC_ROUND forms of the three modes
    if (a.world || a.obs_counts || a.clr || a.parts || a.regions || a.seg || a.step < 0 || a.step + 1 >= a.W ||
        (a.wp_mode == 2 && (!a.wp_stop || a.wp_n < 1)))
      return hipErrorInvalidValue;
    if (a.wp_mode == 2) {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_STOP | MC_ROUND>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_STOP | MC_ROUND>), grid, block, 0, s, a);
    } else if (a.wp_mode == 1) {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_COUNTS | MC_ROUND>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_COUNTS | MC_ROUND>), grid, block, 0, s, a);
    } else {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_PLAIN | MC_ROUND>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_PLAIN | MC_ROUND>), grid, block, 0, s, a);
    }
  } else
  if (a.seg) {                                        // segment checks: the MC_SEG forms of the two counting modes
    if (a.world || a.obs_counts || a.clr || a.parts || a.regions || !a.seg_counts || a.wp_mode == 0 || a.step < 0 || a.step + 1 >= a.W ||
        (a.wp_mode == 2 && (!a.wp_stop || a.wp_n < 1)))
      return hipErrorInvalidValue;
    if (a.wp_mode == 2) {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_STOP | MC_SEG>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_STOP | MC_SEG>), grid, block, 0, s, a);
    } else {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_COUNTS | MC_SEG>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_COUNTS | MC_SEG>), grid, block, 0, s, a);
    }
  } else
  if (a.parts) {                                      // a compound footprint: the MC_PARTS forms of the three modes
    if (a.world || a.obs_counts || a.clr || a.parts_F < 2 || a.parts_F > POCS_MAX_FOOTPRINT_PARTS || a.step < 0 || a.step + 1 >= a.W ||
        (a.wp_mode == 2 && (!a.wp_stop || a.wp_n < 1)))
      return hipErrorInvalidValue;
    if (a.wp_mode == 2) {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_STOP | MC_PARTS>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_STOP | MC_PARTS>), grid, block, 0, s, a);
    } else if (a.wp_mode == 1) {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_COUNTS | MC_PARTS>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_COUNTS | MC_PARTS>), grid, block, 0, s, a);
    } else {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_PLAIN | MC_PARTS>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_PLAIN | MC_PARTS>), grid, block, 0, s, a);
    }
  } else
  if (a.regions) {                                    // watched regions: the MC_REGIONS forms of the three modes
    if (a.world || a.obs_counts || a.clr || !a.reg_counts || a.reg_G < 1 || a.reg_G > POCS_MAX_REGIONS || a.step < 0 || a.step + 1 >= a.W ||
        (a.wp_mode == 2 && (!a.wp_stop || a.wp_n < 1)))
      return hipErrorInvalidValue;
    if (a.wp_mode == 2) {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_STOP | MC_REGIONS>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_STOP | MC_REGIONS>), grid, block, 0, s, a);
    } else if (a.wp_mode == 1) {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_COUNTS | MC_REGIONS>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_COUNTS | MC_REGIONS>), grid, block, 0, s, a);
    } else {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_PLAIN | MC_REGIONS>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_PLAIN | MC_REGIONS>), grid, block, 0, s, a);
    }
  } else
  if (a.clr) {                                        // clearance levels: the MC_CLEAR forms of the three modes
    if (a.world || a.obs_counts || !a.clr_counts || !a.clr_level || a.clr_L < 1 || a.clr_L > POCS_MAX_CLEARANCE_LEVELS || a.step < 0 || a.step + 1 >= a.W ||
        (a.wp_mode == 2 && (!a.wp_stop || a.wp_n < 1)))
      return hipErrorInvalidValue;
    if (a.wp_mode == 2) {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_STOP | MC_CLEAR>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_STOP | MC_CLEAR>), grid, block, 0, s, a);
    } else if (a.wp_mode == 1) {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_COUNTS | MC_CLEAR>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_COUNTS | MC_CLEAR>), grid, block, 0, s, a);
    } else {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_PLAIN | MC_CLEAR>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_PLAIN | MC_CLEAR>), grid, block, 0, s, a);
    }
  } else
  if (a.world) {                                      // a large world: the same three modes, no per-box counts
    if (a.obs_counts || a.world_M < 1 || a.world_M > POCS_MAX_WORLD_RECORDS) return hipErrorInvalidValue;
    if (a.wp_mode != 0 && (a.step < 0 || a.step + 1 >= a.W || (a.wp_mode == 2 && (!a.wp_stop || a.wp_n < 1)))) return hipErrorInvalidValue;
    if (a.wp_mode == 2) {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_world<true, MC_STOP>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_world<false, MC_STOP>), grid, block, 0, s, a);
    } else if (a.wp_mode == 1) {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_world<true, MC_COUNTS>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_world<false, MC_COUNTS>), grid, block, 0, s, a);
    } else {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_world<true, MC_PLAIN>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_world<false, MC_PLAIN>), grid, block, 0, s, a);
    }
  } else
  if (a.obs_counts) {                                 // ... and per obstacle box: the MC_BOXES forms of the two below
    if (a.step < 0 || a.step + 1 >= a.W || (a.wp_mode == 2 && (!a.wp_stop || a.wp_n < 1))) return hipErrorInvalidValue;
    if (a.wp_mode == 2) {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_STOP | MC_BOXES>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_STOP | MC_BOXES>), grid, block, 0, s, a);
    } else {
      if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_COUNTS | MC_BOXES>), grid, block, 0, s, a);
      else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_COUNTS | MC_BOXES>), grid, block, 0, s, a);
    }
  } else if (a.wp_mode == 2) {                               // first collisions per waypoint, and the risk bound obeyed
    if (!a.wp_stop || a.wp_n < 1 || a.step < 0 || a.step + 1 >= a.W) return hipErrorInvalidValue;
    if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_STOP>), grid, block, 0, s, a);
    else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_STOP>), grid, block, 0, s, a);
  } else if (a.wp_mode == 1) {                        // first collisions per waypoint
    if (a.step < 0 || a.step + 1 >= a.W) return hipErrorInvalidValue;
    if (a.nontemporal) hipLaunchKernelGGL((k_mc_step_counts<true, MC_COUNTS>), grid, block, 0, s, a);
    else               hipLaunchKernelGGL((k_mc_step_counts<false, MC_COUNTS>), grid, block, 0, s, a);
  } else if (a.nontemporal) hipLaunchKernelGGL(k_mc_step<true>, grid, block, 0, s, a);
  else                      hipLaunchKernelGGL(k_mc_step<false>, grid, block, 0, s, a);
  return hipGetLastError();
}
hipError_t pocs_launch_mc_fused(int nblk, const pocs_mc_launch& a, hipStream_t s) {
  if (a.wp_mode == 2 || (a.wp_mode != 0 && !a.wp_counts) || (a.obs_counts && !a.wp_mode)) return hipErrorInvalidValue;      // (no stop without a launch boundary per step)
  if (a.clr) return hipErrorInvalidValue;             // (clearance levels: the per-step form)
  if (a.parts) return hipErrorInvalidValue;           // (a compound footprint: the per-step form)
  if (a.regions) return hipErrorInvalidValue;         // (watched regions: the per-step form)
  if (a.seg) return hipErrorInvalidValue;             // (segment checks: the per-step form)
  if (a.round) return hipErrorInvalidValue;           // (round obstacles: the per-step form)
  if (a.world) return hipErrorInvalidValue;           // (a large world is not staged: no fused form)
  if (a.obs_counts) {
    if (a.env_steps > 1) hipLaunchKernelGGL(k_mc_fused_sched<MC_COUNTS | MC_BOXES>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
    else                 hipLaunchKernelGGL(k_mc_fused_boxes, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
  } else if (a.env_steps > 1) {                              // an obstacle schedule: the world is restaged per step
    if (a.wp_mode) hipLaunchKernelGGL(k_mc_fused_sched<MC_COUNTS>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
    else           hipLaunchKernelGGL(k_mc_fused_sched<MC_PLAIN>, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
  } else if (a.wp_mode) hipLaunchKernelGGL(k_mc_fused_counts, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
  else                  hipLaunchKernelGGL(k_mc_fused, dim3(nblk, a.nruns), dim3(POCS_BLOCK), 0, s, a);
  return hipGetLastError();
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
hipError_t pocs_launch_probe_math(const pocs_tables* tables, int n, const uint32_t* wr, const uint32_t* wa, const double* x, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_probe_math, dim3(1), dim3(POCS_BLOCK), 0, s, tables, n, wr, wa, x, out);
  return hipGetLastError();
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
hipError_t pocs_launch_probe_radius_roots(const pocs_tables* tables, uint32_t first, unsigned long long count, unsigned long long* out, hipStream_t s) {
  if (!tables || !out || count < 1 || (unsigned long long)first + count > (1ull << 32)) return hipErrorInvalidValue;
  const unsigned long long nb = (count + POCS_BLOCK - 1) / POCS_BLOCK;
  hipLaunchKernelGGL(k_probe_radius_roots, dim3((unsigned)(nb < POCS_MAX_BLOCKS ? nb : POCS_MAX_BLOCKS)), dim3(POCS_BLOCK), 0, s, tables, first, count, out);
  return hipGetLastError();
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
hipError_t pocs_launch_probe_collide(int K, const pocs_gmm_launch& a, int n, const double* x, const double* y, const double* th,
                                     int* flags, int* nkeep, double* kept, hipStream_t s) {
  if (n < 1 || a.M < 0 || a.M > POCS_MAX_OBSTACLES || !a.env || !a.tables || !a.param) return hipErrorInvalidValue;
  return with_K(K, [&](auto k) {
    constexpr int KK = decltype(k)::value, TB = POCS_GMM_BLOCK_OF(KK);
    hipLaunchKernelGGL((k_probe_collide<KK, TB>), dim3(1), dim3(TB), 0, s, a, n, x, y, th, flags, nkeep, kept);
    return hipGetLastError();
  });
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
  for (int j = threadIdx.x; j < POCS_MAX_OBSTACLES * POCS_OBS_STRIDE; j += POCS_BLOCK) { s_obs[j] = env->obs[j]; s_obs2[j] = clr->obs[j]; }
  if (threadIdx.x < POCS_MAX_CLEARANCE_LEVELS) s_d[threadIdx.x] = clr->d[threadIdx.x];
  __syncthreads();
  const pocs_footprint fp = env->fp;
  const int M = env->M;
  POCS_VCONST(vc_);
  const int npairs = (n + 1) / 2;
  // (every lane of a wave makes every trip: the pair form ballots)
  for (int p0 = (int)threadIdx.x - (int)(threadIdx.x & 63); p0 < npairs; p0 += POCS_BLOCK) {
    const int p = p0 + (int)(threadIdx.x & 63);
    const bool live = p < npairs;
    const int i0 = live ? 2 * p : 0, i1 = live && i0 + 1 < n ? i0 + 1 : i0;
    const double xs[2] = {x[i0], x[i1]}, ys[2] = {y[i0], y[i1]}, ts[2] = {th[i0], th[i1]};
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
  }
}
hipError_t pocs_launch_probe_clearance(const pocs_env_dev* env, const pocs_clear_dev* clr, int L, const pocs_tables* tables, int n,
                                       const double* x, const double* y, const double* th, int* level_out, hipStream_t s) {
  if (!env || !clr || !tables || n < 1 || L < 0 || L > POCS_MAX_CLEARANCE_LEVELS || !x || !y || !th || !level_out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_clearance, dim3(1), dim3(POCS_BLOCK), 0, s, env, clr, L, tables, n, x, y, th, level_out);
  return hipGetLastError();
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
  for (int j = threadIdx.x; j < POCS_MAX_OBSTACLES * POCS_OBS_STRIDE; j += POCS_BLOCK) s_obs[j] = env->obs[j];
  if (threadIdx.x < POCS_MAX_FOOTPRINT_PARTS * POCS_PART_STRIDE) s_parts[threadIdx.x] = parts->part[threadIdx.x];
  __syncthreads();
  const int M = env->M;
  POCS_VCONST(vc_);
  const int npairs = (n + 1) / 2;
  // (every lane of a wave makes every trip: the pair form ballots)
  for (int p0 = (int)threadIdx.x - (int)(threadIdx.x & 63); p0 < npairs; p0 += POCS_BLOCK) {
    const int p = p0 + (int)(threadIdx.x & 63);
    const bool live = p < npairs;
    const int i0 = live ? 2 * p : 0, i1 = live && i0 + 1 < n ? i0 + 1 : i0;
    const double xs[2] = {x[i0], x[i1]}, ys[2] = {y[i0], y[i1]}, ts[2] = {th[i0], th[i1]};
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
  }
}
hipError_t pocs_launch_probe_parts(const pocs_env_dev* env, const pocs_parts_dev* parts, int F, const pocs_tables* tables, int n,
                                   const double* x, const double* y, const double* th, int* touched_out, hipStream_t s) {
  if (!env || !parts || !tables || n < 1 || F < 1 || F > POCS_MAX_FOOTPRINT_PARTS || !x || !y || !th || !touched_out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_parts, dim3(1), dim3(POCS_BLOCK), 0, s, env, parts, F, tables, n, x, y, th, touched_out);
  return hipGetLastError();
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
  const int npairs = (n + 1) / 2;
  // (every lane of a wave makes every trip: the pair form ballots)
  for (int p0 = (int)threadIdx.x - (int)(threadIdx.x & 63); p0 < npairs; p0 += POCS_BLOCK) {
    const int p = p0 + (int)(threadIdx.x & 63);
    const bool live = p < npairs;
    const int i0 = live ? 2 * p : 0, i1 = live && i0 + 1 < n ? i0 + 1 : i0;
    const double xs[2] = {x[i0], x[i1]}, ys[2] = {y[i0], y[i1]}, ts[2] = {th[i0], th[i1]};
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
  }
}
hipError_t pocs_launch_probe_regions(const pocs_regions_dev* regions, int G, const pocs_tables* tables, int n,
                                     const double* x, const double* y, const double* th, int* mask_out, hipStream_t s) {
  if (!regions || !tables || n < 1 || G < 0 || G > POCS_MAX_REGIONS || !x || !y || !th || !mask_out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_regions, dim3(1), dim3(POCS_BLOCK), 0, s, regions, G, tables, n, x, y, th, mask_out);
  return hipGetLastError();
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
  for (int j = threadIdx.x; j < POCS_MAX_OBSTACLES * POCS_OBS_STRIDE; j += POCS_BLOCK) s_obs[j] = env->obs[j];
  if (threadIdx.x < POCS_MAX_SEGMENT_CHECKS) s_f[threadIdx.x] = seg->f[threadIdx.x];
  __syncthreads();
  const int M = env->M, J = seg->J;
  const pocs_footprint fp = env->fp;
  POCS_VCONST(vc_);
  const double a0 = backward ? -u2 : u0;
  const int npairs = (n + 1) / 2;
  // (every lane of a wave makes every trip: the pair form ballots)
  for (int p0 = (int)threadIdx.x - (int)(threadIdx.x & 63); p0 < npairs; p0 += POCS_BLOCK) {
    const int p = p0 + (int)(threadIdx.x & 63);
    const bool live = p < npairs;
    const int i0 = live ? 2 * p : 0, i1 = live && i0 + 1 < n ? i0 + 1 : i0;
    const double xs[2] = {x[i0], x[i1]}, ys[2] = {y[i0], y[i1]}, ts[2] = {th[i0], th[i1]};
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
  }
}
hipError_t pocs_launch_probe_segment(const pocs_env_dev* env, const pocs_seg_dev* seg, const pocs_tables* tables, double u0, double u1,
                                     double u2, int backward, int n, const double* x, const double* y, const double* th, int* mask_out,
                                     hipStream_t s) {
  if (!env || !seg || !tables || n < 1 || !x || !y || !th || !mask_out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_segment, dim3(1), dim3(POCS_BLOCK), 0, s, env, seg, tables, u0, u1, u2, backward ? 1 : 0, n, x, y, th, mask_out);
  return hipGetLastError();
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
hipError_t pocs_launch_probe_counts(int n, const int* K, const double* w, const double* alive, const unsigned long long* seeds, const uint32_t* wp,
                                    const double* n_total, double* out, hipStream_t s) {
  if (n < 1 || n > (1 << 20) || !K || !w || !alive || !seeds || !wp || !n_total || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_counts, dim3((unsigned)((n + POCS_BLOCK - 1) / POCS_BLOCK)), dim3(POCS_BLOCK), 0, s, n, K, w, alive, seeds, wp, n_total, out);
  return hipGetLastError();
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
  for (int j = threadIdx.x; j < POCS_MAX_OBSTACLES * POCS_OBS_STRIDE; j += POCS_BLOCK) s_obs[j] = env->obs[j];
  __syncthreads();
  const int M = env->M < POCS_MAX_OBSTACLES ? env->M : POCS_MAX_OBSTACLES;
  const pocs_footprint fp = env->fp;
  POCS_VCONST(vc_);
  const int npairs = (n + 1) / 2;
  // (every lane of a wave makes every trip: the pair form ballots)
  for (int p0 = (int)threadIdx.x - (int)(threadIdx.x & 63); p0 < npairs; p0 += POCS_BLOCK) {
    const int p = p0 + (int)(threadIdx.x & 63);
    const bool live = p < npairs;
    const int i0 = live ? 2 * p : 0, i1 = live && i0 + 1 < n ? i0 + 1 : i0;
    const double xs[2] = {x[i0], x[i1]}, ys[2] = {y[i0], y[i1]}, ts[2] = {th[i0], th[i1]};
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
  }
}
hipError_t pocs_launch_probe_discs(const pocs_env_dev* env, const pocs_tables* tables, int n, const double* x, const double* y,
                                   const double* th, int* out, hipStream_t s) {
  if (!env || !tables || n < 1 || !x || !y || !th || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_discs, dim3(1), dim3(POCS_BLOCK), 0, s, env, tables, n, x, y, th, out);
  return hipGetLastError();
}
// Uncertain discs on poses, a footprint, discs and factor rows the caller picks (pocs_probe_device_disc_noise: a test hook beside
// k_probe_discs): ONE block stages the tables, the D grown disc records and their rows and asks, per pose of index first + i, the
// functions the kernels ask.  The displaced centres are pocs_disc_displaced's, disc by disc; bit d of a pose's flags is "touches
// displaced disc d" by pocs_pose_collides_noisy, the MC kernels' single-pose form, whose own answer must be (bits != 0).  Then
// pocs_pair_collides_masks' noisy ROUND form as k_gmm_step_noise calls it, disc by disc on poses 2 p, 2 p + 1 of pair
// (first >> 1) + p (an odd last pose beside its own twin's index, which is then not read): bit 31 should the two forms ever disagree.
__global__ __launch_bounds__(POCS_BLOCK) void k_probe_disc_noise(const pocs_env_dev* __restrict__ env, const double* __restrict__ rows,
                                                                 const pocs_tables* __restrict__ tables, unsigned long long seed, unsigned v,
                                                                 unsigned long long first, int n, const double* __restrict__ x,
                                                                 const double* __restrict__ y, const double* __restrict__ th,
                                                                 double* __restrict__ centres, unsigned* __restrict__ flags) {
  __shared__ pocs_tables s_tab;
  __shared__ __attribute__((aligned(16))) double s_obs[POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];
  __shared__ __attribute__((aligned(16))) double s_rows[POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE];
  stage_tables(tables, &s_tab);
  for (int j = threadIdx.x; j < POCS_MAX_OBSTACLES * POCS_OBS_STRIDE; j += POCS_BLOCK) s_obs[j] = env->obs[j];
  for (int j = threadIdx.x; j < POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE; j += POCS_BLOCK) s_rows[j] = rows[j];
  __syncthreads();
  const int D = env->M < 16 ? env->M : 16;
  const pocs_footprint fp = env->fp;
  POCS_VCONST(vc_);
  const int npairs = (n + 1) / 2;
  // (every lane of a wave makes every trip: the pair form ballots)
  for (int p0 = (int)threadIdx.x - (int)(threadIdx.x & 63); p0 < npairs; p0 += POCS_BLOCK) {
    const int p = p0 + (int)(threadIdx.x & 63);
    const bool live = p < npairs;
    const int i0 = live ? 2 * p : 0;
    const bool two = live && i0 + 1 < n;
    const int i1 = two ? i0 + 1 : i0;
    const double xs[2] = {x[i0], x[i1]}, ys[2] = {y[i0], y[i1]}, ts[2] = {th[i0], th[i1]};
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
  }
}
hipError_t pocs_launch_probe_disc_noise(const pocs_env_dev* env, const double* rows, const pocs_tables* tables, unsigned long long seed,
                                        unsigned v, unsigned long long first, int n, const double* x, const double* y, const double* th,
                                        double* centres, unsigned* flags, hipStream_t s) {
  if (!env || !rows || !tables || n < 1 || (first & 1ull) || !x || !y || !th || !centres || !flags) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_probe_disc_noise, dim3(1), dim3(POCS_BLOCK), 0, s, env, rows, tables, seed, v, first, n, x, y, th, centres, flags);
  return hipGetLastError();
}
// The round footprint's test on poses, a radius, boxes, discs and factor rows the caller picks (pocs_probe_device_footprint_disc: a test
// hook beside k_probe_discs): ONE block stages the tables, the composed records and -- where given -- their rows and asks, per pose of
// index first + i, the functions the kernels ask.  Bit 0: the pose touches some box, bit 1: some disc, displaced where its row says so
// -- pocs_round_pose_kinds, the single-pose form on the full table, and the MC kernels' pocs_round_pose_collides[_noisy] must say
// (bits != 0).  Then pocs_pair_round_masks as the _rfoot kernels call it on poses 2 p, 2 p + 1 of pair (first >> 1) + p (an odd last
// pose beside its own twin's index, which is then not read), its disc masks handed out: bit 8 should the two forms ever disagree.
__global__ __launch_bounds__(POCS_BLOCK) void k_probe_footprint_disc(const pocs_env_dev* __restrict__ env, const double* __restrict__ rows,
                                                                     const pocs_tables* __restrict__ tables, unsigned long long seed, unsigned v,
                                                                     unsigned long long first, int n, const double* __restrict__ x,
                                                                     const double* __restrict__ y, int* __restrict__ out) {
  __shared__ pocs_tables s_tab;
  __shared__ __attribute__((aligned(16))) double s_obs[POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];
  __shared__ __attribute__((aligned(16))) double s_rows[POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE];
  stage_tables(tables, &s_tab);
  for (int j = threadIdx.x; j < POCS_MAX_OBSTACLES * POCS_OBS_STRIDE; j += POCS_BLOCK) s_obs[j] = env->obs[j];
  for (int j = threadIdx.x; j < POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE; j += POCS_BLOCK) s_rows[j] = rows ? rows[j] : 0.0;
  __syncthreads();
  const int M = env->M < POCS_MAX_OBSTACLES ? env->M : POCS_MAX_OBSTACLES;
  const double rho = env->fp.hx;
  const bool noisy = rows != nullptr;                                  // (the same in every thread)
  POCS_VCONST(vc_);
  const int npairs = (n + 1) / 2;
  // (every lane of a wave makes every trip: the pair form ballots)
  for (int p0 = (int)threadIdx.x - (int)(threadIdx.x & 63); p0 < npairs; p0 += POCS_BLOCK) {
    const int p = p0 + (int)(threadIdx.x & 63);
    const bool live = p < npairs;
    const int i0 = live ? 2 * p : 0;
    const bool two = live && i0 + 1 < n;
    const int i1 = two ? i0 + 1 : i0;
    const double xs[2] = {x[i0], x[i1]}, ys[2] = {y[i0], y[i1]};
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
      if (two) out[i1] = (int)(single[1] | (bad[1] ? 256u : 0u));
    }
  }
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

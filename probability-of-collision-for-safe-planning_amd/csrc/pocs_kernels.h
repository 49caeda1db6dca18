// pocs_kernels.h -- launch interface between the host runtime (pocs_host.hip, pocs_ctx.hpp) and the gfx950
// kernels (pocs_kernels.hip: the pocs_launch_* functions; the kernels themselves in its parts pocs_dev_prims.hpp,
// pocs_dev_advance.hpp, pocs_dev_gmm.hpp, pocs_dev_mc.hpp, pocs_dev_probe.hpp).  Internal; the public boundary is include/pocs.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pocs_collide.h"
#include "pocs_launch_forms.hpp"   // the MC_* bits of the MC kernels' form word; which kernel a launch record asks for
#include "pocs_model.h"
#include "pocs_world.h"

#define POCS_BLOCK 256        // MC kernels
// GMM kernels: TWO blocks of 512 threads per CU = four waves per SIMD at <= 128 VGPRs.  The sampling body
// keeps one component's sums per thread whatever K is, so one shape serves every K (measured at K = 8,
// 10^7 samples, 16 runs: 2 x 512 0.39 of the HBM peak, 1 x 768 and 3 x 256 0.40, 2 x 384 0.31).  Two
// co-resident blocks instead of one fat one: while one block is in its head or tail (parameter
// staging, block reduction, the drain of its stores, ticket, mixture advance) the other block's waves
// have the CU's issue slots.
#define POCS_GMM_BLOCK_OF(K) 512
#define POCS_GMM_BLOCKS_PER_CU 2
#define POCS_NUM_CUS 256
#define POCS_MAX_BLOCKS 2048
// Task geometry of k_gmm_step.  A chunk = one iteration of a block = POCS_GMM_BLOCK_OF(K) pairs of samples.
// A run's chunks are cut into VS = 2^vs_shift VIRTUAL SLICES, slice j = chunks [j * chunks / VS,
// (j + 1) * chunks / VS): VS depends on the shard's sample count only (the largest power of two <= min(256,
// chunks)), never on how many runs share the launch -- the moment sums are defined on the virtual slices
// (pocs_dev_gmm.hpp, "summation tree"), which is what makes a run's result independent of the batch.
// The launch's work = the flat list of units t = r * VS + j; block b takes units [b * upb, (b + 1) * upb).
#define POCS_GMM_MAX_VS 256
// Block size and slice count are part of the NUMERICS (the summation tree is defined on chunks of 512 pairs, 64-lane
// waves and at most 256 virtual slices; oracle/pocs_oracle.c::tree_moments restates exactly these): a build with
// other values would produce other last bits under the same version string.
static_assert(POCS_GMM_BLOCK_OF(3) == 512 && POCS_GMM_MAX_VS == 256, "summation tree (numerics v7 and later): 512-pair chunks, 256 virtual slices");
#define POCS_LONE_PRE 3        // lone form: iterations of a unit whose normals the block's head draws ahead (72 KB of LDS at 512 threads)
#define POCS_GMM_SUB 32        // units whose wave sums a block holds in LDS at a time (64 runs x 256 slices / 512 blocks)
#define POCS_UNIT_SUMS 10      // survivors + the nine sums
#define POCS_FLUSH_ROWS 5      // flush_unit's transpose scratch per wave: 5 rows of 64 lane values,
#define POCS_FLUSH_PITCH 66    // pitch 66 doubles (16-byte aligned rows, off the bank stride)
// chain record (doubles), one per step i < W-1:
//   [0..2] applied control   [3..5] diag of M   [6..8] the noisy control actually driven (MC)
//   [9] unused               [10 .. 10+L) the L range observations of the step
#define POCS_CHAIN_Z 10
#define POCS_CHAIN_STRIDE 48
static_assert(POCS_CHAIN_Z + POCS_MAX_LANDMARKS <= POCS_CHAIN_STRIDE, "chain record too small");

struct pocs_env_dev {            // collision world as the kernels see it (in HBM one record per step of the obstacle schedule, staged to LDS)
  pocs_footprint fp;
  int M;
  int pad;
  double obs[POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];
};

// Clearance levels (pocs_set_clearance_levels) as the kernels see them, in HBM beside the collision world: one record per step of
// the obstacle schedule.  The distances and everything derived from them live HERE, not in launch arguments: a call's launches
// carry the array's address and L, so other distances with the same L replay the cached graph.
struct pocs_clear_dev {
  pocs_footprint fp;             // the footprint grown by d[L - 1]
  double fp_rr, fp_phi;          // its bounding radius and corner angle (pocs_footprint_extent_pre), for the cull
  double d[POCS_MAX_CLEARANCE_LEVELS];
  double obs[POCS_MAX_OBSTACLES * POCS_OBS_STRIDE];   // the step's boxes prepared (pocs_prepare_obstacle) for that footprint
};

// A compound footprint (pocs_set_footprint_parts, F > 1) as the kernels see it, in HBM beside the collision world: the parts'
// values live HERE, not in launch arguments -- a call's launches carry the address and F, so other values with the same F replay the
// cached graph.  Under a compound footprint the world's records (pocs_env_dev::obs) are prepared for the part with the largest
// bounding radius (pocs_parts_cover), and pocs_env_dev::fp is part 0.
struct pocs_parts_dev {
  double part[POCS_MAX_FOOTPRINT_PARTS * POCS_PART_STRIDE];   // per part dx dy hx hy, bounding radius, corner angle (pocs_prepare_part)
};

// Watched regions (pocs_set_regions) as the kernels see them, in HBM beside the collision world: ONE record, the regions are
// static.  The boxes and everything derived from them live HERE, not in launch arguments: a call's launches carry the address
// and G, so other boxes with the same G and kinds replay the cached graph.
struct pocs_regions_dev {
  double rec[POCS_MAX_REGIONS * POCS_OBS_STRIDE];   // region g prepared (pocs_prepare_obstacle) for ITS footprint
  double fp[POCS_MAX_REGIONS * 4];                  // that footprint, dx dy hx hy: the robot's (TOUCH) or {0, 0, 0, 0} (POINT)
  double fp_rr[POCS_MAX_REGIONS], fp_phi[POCS_MAX_REGIONS];   // its bounding radius and corner angle (pocs_footprint_extent_pre)
  int kind[POCS_MAX_REGIONS];
};
#define POCS_REGIONS_HEAD (POCS_MAX_REGIONS * (POCS_OBS_STRIDE + 4))   // the doubles a kernel's head stages: rec | fp

// Segment checks (pocs_set_segment_checks, J > 1) as the kernels see them, in HBM beside the collision world: J and the fractions
// f_j = j / J (pocs_segment_fractions) live HERE, not in launch arguments -- a call's launches carry the address, so another J > 1
// replays the cached graph.  The controls come from the run's chain record, which is on the device anyway.
struct pocs_seg_dev {
  double f[POCS_MAX_SEGMENT_CHECKS];
  int J;                         // 2 .. POCS_MAX_SEGMENT_CHECKS
  int pad;
};

struct pocs_run_header {         // per-run scalars read by every kernel (so a captured graph stays valid)
  uint64_t seed;
  uint64_t pad;                  // sharded whole calls: the context's count of exchange sequences (pocs_gmm_launch::xchg_epoch_from_header)
};

// One-hop exchange of the per-waypoint moments between the GPUs of a node: every rank
// owns a buffer that ALL ranks have mapped (hipIpc); rank q writes its rows into slot q of every
// buffer, then its flags; every rank adds the slots of its own buffer in rank order.
//   data  f64 [2 parities][POCS_XCHG_MAX_WORLD][POCS_XCHG_MAX_RUNS][POCS_XCHG_MAX_NC]
//   flags u64 [2 parities][POCS_XCHG_MAX_WORLD][POCS_XCHG_MAX_RUNS]      = epoch of the row in that slot
#define POCS_XCHG_MAX_WORLD 8
#define POCS_XCHG_MAX_RUNS 256
#define POCS_XCHG_MAX_NC (POCS_MAX_GAUSSIANS * POCS_NMOM)
#define POCS_XCHG_DATA_DOUBLES (2ull * POCS_XCHG_MAX_WORLD * POCS_XCHG_MAX_RUNS * POCS_XCHG_MAX_NC)
#define POCS_XCHG_FLAG_WORDS (2ull * POCS_XCHG_MAX_WORLD * POCS_XCHG_MAX_RUNS)
#define POCS_XCHG_BYTES ((POCS_XCHG_DATA_DOUBLES + POCS_XCHG_FLAG_WORDS + 2) * 8ull)
struct pocs_xchg_dev {
  double* buf[POCS_XCHG_MAX_WORLD];   // buffer of rank q as mapped in THIS process (own rank: the allocation itself)
  int world, rank;
  int parity;                         // which of the two slot sets: (exchanges so far) & 1, the same on every rank
  int pad;
  unsigned long long epoch;           // of this waypoint's rows: (call number << 20) | (waypoint + 1)
};

// Arrays carry a leading "run" dimension: a launch advances `nruns` independent estimations (the
// reference's driver performs 200 of them one after the other, MCSimulation.py:238-256) in lockstep.
// Where a field below says "non-null (nonzero) = the launch is the kernel's _x form", that is its part in a choice made in ONE place,
// pocs_forms::gmm_step_form / gmm_tree_step_form (pocs_launch_forms.hpp): which of several such words wins, what a form needs and
// refuses beside it ("never LONE, TREE, ...") and which of its values are checked is that header's rule for the feature, not this text.
struct pocs_gmm_launch {
  const pocs_run_header* hdr;    // [nruns] per-run seeds
  const pocs_env_dev* env;       // obstacle table (records only; M and the footprint travel below)
  const pocs_tables* tables;     // log / sector tables (pocs_math.h), staged to LDS
  const double* chain;           // [nruns][W-1][POCS_CHAIN_STRIDE]  (a call of plans: W = the longest plan's length)
  const pocs_sensor* sensor;
  double* state;                 // [nruns][W][K*POCS_STATE_STRIDE]  mixture sampled at each waypoint
  double* param;                 // [nruns][W][K*POCS_PARAM_STRIDE]  its sampler parameters (incl. the cumulative component counts)
  double* moments;               // [W][nruns][K*POCS_NMOM]          reduced moments of each waypoint
  double* partial;               // [nruns][VS][K*POCS_NMOM]         row of (run, virtual slice); rewritten every waypoint
  const double* partial_prev;    // lone call: the rows the PREVIOUS waypoint's launch left (the other half of the buffer)
  unsigned* sync;                // the call's synchronisation words, zeroed once per call:
                                 // [1] give-up code of a bounded wait (0 = none)
  unsigned* ticket;              // [nruns][W] arrival counters of the blocks of (run, waypoint); same zeroed block
  unsigned* xwait;               // [nruns][W] sharded: how long the closer of (run, waypoint) waited for the world's rows (10 ns ticks); same block
  double* x; double* y; double* th;   // SoA sample buffers [nruns][sample_stride] (unused when !store)
  int16_t* flags;
  long long n_total;             // samples of the whole mixture (all shards): what the component counts add up to
  long long first;               // global index of the shard's first sample
  long long count;               // samples in this shard
  long long sample_stride;       // even, >= count
  int nruns;
  int W;
  pocs_footprint fp;
  double fp_rr, fp_phi;          // its bounding radius and corner angle atan2(hy, hx) (pocs_footprint_extent_pre)
  int M;
  int waypoint;
  int store;
  int advance_in_tail;           // > 0: the last block of run r < advance_in_tail also builds state/param[waypoint+1] (single GPU;
                                 // run_lo + run_cnt, except in a call of plans: the runs whose plan ends at this waypoint are the
                                 // tail of the launch's runs and have no waypoint + 1); 0: none
  int exchange_in_tail;          // 1: ... after exchanging the run's moments with the other ranks through `xchg` (sharded)
  int xchg_epoch_from_header;    // 1: the exchange's call number comes from hdr[run].pad (whole calls replayed from a graph), not from xchg
  int lone;                      // 1: one run per call -- no tickets, no closer: every block of waypoint w's launch adds the
                                 //    rows of w-1 and advances the mixture itself, in its head (k_gmm_step, "lone call")
  pocs_xchg_dev xchg;
  // launch geometry (above)
  long long chunks;              // of the shard
  int vs_shift;                  // VS = 1 << vs_shift virtual slices per run
  int upb;                       // units per block (<= VS)
  int blocks;
  int run_lo, run_cnt;           // the runs of the batch this launch works on
  // a call of plans under a risk bound (pocs_set_plan_risk_bound; behind everything else: the other launches' argument offsets stay)
  int risk;                      // 1: the launch is k_gmm_step_risk, whose closers decide the stop of their run and whose heads obey it
  int risk_pad;
  unsigned* stop;                // [nruns] 0 = the run is live, w + 1 = its closer of waypoint w found the running probability at the
                                 // bound -- no later launch works on the run; part of the call's zeroed synchronisation block
  double* surv;                  // [nruns] the run's running survival product prod_{v <= w} (1 - p_v), kept by its closers (the closer
                                 // of waypoint 0 starts from 1.0: never read before it is written)
  double risk_bound;             // a run stops at the first waypoint w with 1 - surv >= risk_bound
  // a tree of plans (pocs_set_plan_tree; behind everything else again).  Its launches work on the nodes of ONE level: a "run" is a
  // node's slot, nruns the number of nodes, W = 1 (every [run][W] array holds one row per node), `waypoint` the level's depth.
  const int* tree_parent;        // [nruns] the slot of every slot's parent (slot 0, the root: 0); null: not a tree launch
  // per-obstacle collision counts (POCS_OPT_OBSTACLE_COUNTS; behind everything else again)
  unsigned long long* obs_counts; // [nruns][W][POCS_MAX_OBSTACLES] samples of the shard drawn at (run, waypoint) whose footprint touches box m of
                                 // the caller's table; non-null: the launch is the kernel's _boxes form.  Zeroed by pocs_launch_zero_counts
                                 // at the head of the call's launches
  // a large collision world (pocs_set_world with more than POCS_MAX_OBSTACLES boxes; behind everything else again).  `env` then holds
  // no record (M = 0 above); k_world_cull, one launch in front of every waypoint's sampling launch, leaves per run the records in
  // the run's reach, and the sampling launch is the kernel's _world form, whose heads fetch those instead of culling the table
  const double* world;           // [world_M][POCS_OBS_STRIDE] the prepared records; non-null: a large world
  int world_M;
  int world_pad;
  double* kept;                  // [nruns][POCS_MAX_OBSTACLES][POCS_OBS_STRIDE] the first POCS_MAX_OBSTACLES kept records of (run, this waypoint), in
                                 // the caller's order, fields 6 and 7 tightened to the run's headings
  int* kept_idx;                 // [nruns][POCS_MAX_OBSTACLES] their indices in the caller's table
  int* reach;                    // [nruns][W] how many records the cull kept at (run, waypoint), the overflow included; zeroed per call
  // clearance levels (pocs_set_clearance_levels; behind everything else again): non-null = the launch is the kernel's _clear form
  // (ticket form, with or without the risk bound; never LONE, TREE, OC or WORLD), which also counts per level the samples drawn at
  // (run, waypoint) that are within the level's clearance of the waypoint's world
  const pocs_clear_dev* clr;     // the record of the launch's waypoint (aimed with `env`)
  unsigned long long* clr_counts; // [nruns][W][POCS_MAX_CLEARANCE_LEVELS]; zeroed by pocs_launch_zero_counts at the head of the call's launches
  int clr_L;                     // 1 .. POCS_MAX_CLEARANCE_LEVELS
  int clr_pad;
  // a compound footprint (pocs_set_footprint_parts with F > 1; behind everything else again): non-null = the launch is the kernel's
  // _parts form (ticket form, with or without the risk bound; never LONE, TREE, OC, WORLD or CL), whose cull and collision test run
  // over the parts; `fp`, `fp_rr` and `fp_phi` above are zero then
  const pocs_parts_dev* parts;
  int parts_F;                   // 2 .. POCS_MAX_FOOTPRINT_PARTS
  int parts_pad;
  // watched regions (pocs_set_regions; behind everything else again): non-null = the launch is the kernel's _regions form (ticket
  // form, with or without the risk bound; never LONE, TREE, OC, WORLD, CL or parts), which also counts per region the samples drawn
  // at (run, waypoint) whose collision flag is 0 and which are in the region
  const pocs_regions_dev* regions;
  unsigned long long* reg_counts; // [nruns][W][POCS_MAX_REGIONS]; zeroed by pocs_launch_zero_counts at the head of the call's launches
  int reg_G;                     // 1 .. POCS_MAX_REGIONS
  int reg_pad;
  // segment checks (pocs_set_segment_checks with J > 1; behind everything else again): non-null = the launch is the kernel's _seg form
  // (ticket form, with or without the risk bound; never LONE, TREE, OC, WORLD, CL, parts or regions): a sample drawn at waypoint w >= 1
  // also touches when one of its J - 1 sub-poses on the way in does -- backwards along the applied control of step w - 1, chain record
  // [0..2] of the run -- and the samples whose own pose is free and some sub-pose touches are counted
  const pocs_seg_dev* seg;
  unsigned long long* seg_counts; // [nruns][W]; zeroed by pocs_launch_zero_counts at the head of the call's launches
  // round obstacles (pocs_set_discs with D > 0; behind everything else again): nonzero = the launch is the kernel's _round form (ticket
  // form, with or without the risk bound; never LONE, TREE, OC, WORLD, CL, parts, regions or segment checks): the table in `env` may
  // hold disc records behind its boxes (pocs_collide.h), M counts both
  int round;
  int round_pad;
  // uncertain discs (pocs_set_disc_covariances with a nonzero row; behind everything else again): non-null = the launch is the _noise
  // form on top of the _round form (`round` is nonzero too): the rows {l00, l10, l11, disc index} of the records of `env`, record by
  // record (POCS_NOISE_STRIDE doubles each, zeros for a box), for the launch's waypoint -- aimed with `env`.  The waypoint word of the
  // deviations is the launch's waypoint
  const double* noise;
  // a round footprint (pocs_set_footprint_disc; behind everything else again): nonzero = the launch is the _rfoot form (ticket form,
  // with or without the risk bound, `noise` non-null: its noise twin; never LONE, TREE, OC, WORLD, CL, parts, regions or segment
  // checks), whatever `round` says -- a world without discs takes the same family.  fp is {0, 0, rho, rho}: the radius is fp.hx
  int rfoot;
  int rfoot_pad;
  // prediction hypotheses (pocs_set_disc_hypotheses; behind everything else again): non-null = the launch is the _hyp form on top of the
  // _noise form (`round` is nonzero and `noise` non-null too -- rows of zeros where the context has no covariances --, never `rfoot`):
  // the gates {lo, hi - 1, g, on} of the records of `env`, record by record (POCS_GATE_STRIDE 32-bit words each, zeros for a box and
  // for a disc that is always there), the same at every waypoint.  The waypoint word of the existence draws is the launch's waypoint
  const uint32_t* gates;
};
#define POCS_MAX_WORLD_RECORDS 4096   // = POCS_MAX_WORLD_BOXES (include/pocs.h; pocs_ctx.hpp checks)
#define POCS_CULL_BLOCK 256           // k_world_cull
// a tree's stop words: 0 = live, depth + 1 = the node's own closer found the bound reached, this bit = below such a node
#define POCS_TREE_STOP_INHERITED 0x80000000u
#define POCS_SYNC_ABORT 1

// "non-null (nonzero) = the MC_X forms" below: the word's part in the choice of pocs_forms::mc_init_form / mc_step_form / mc_fused_form /
// mc_tree_step_form (pocs_launch_forms.hpp), which hold the precedence, the refusals and the checks as for pocs_gmm_launch.
struct pocs_mc_launch {               // blockIdx.y = run of the batch, like pocs_gmm_launch
  const pocs_run_header* hdr;          // [nruns]
  const pocs_env_dev* env;
  const pocs_tables* tables;
  const double* chain;                 // [nruns][W-1][STRIDE]: noisy control of step s at [..][s][6..8]
  double* x; double* y; double* th;    // SoA particle state [nruns][stride] of this shard
  uint32_t* hits;                      // particlecollisions [nruns][stride]
  unsigned long long* total;           // [nruns] particles with hits > 0
  long long first, count;
  long long stride;                    // >= count
  int W;
  double mu0[3];
  double L0[6];
  const double* run_plan;              // a call of plans: [nruns][4] = start mean (3) and number of steps of each run's plan
                                       // (k_mc_init, k_mc_fused); null: mu0 and `step` hold for every run
  int step;                            // k_mc_step: control index; k_mc_fused: number of steps
  int nruns;
  int nontemporal;                     // k_mc_step: the batch's state exceeds the Infinity Cache, stream past it
  // first collisions per waypoint (POCS_OPT_MC_WAYPOINT_COUNTS / POCS_OPT_MC_RISK_BOUND; behind everything else: the other
  // launches' argument offsets stay)
  int wp_mode;                         // 0: the kernels above as they are; 1: the _counts kernels also fill wp_counts; 2 (k_mc_step
                                       // only): ... and a run whose cumulative count has reached the bound moves no further
  unsigned long long* wp_counts;       // [nruns][W] particles of the shard whose FIRST collision is at waypoint w (0: k_mc_init,
                                       // s + 1: control s); zeroed with `total`, one allocation
  unsigned* wp_stop;                   // [nruns] 0 = never stopped, s + 1 = stopped at waypoint s; written once, read by the host only
  long long wp_n;                      // mode 2: N, the particles of a run
  double wp_bound;                     // mode 2: a run stops at the first waypoint s with (double)C[s] / (double)N >= wp_bound
  // a tree of plans (k_mc_tree_step; behind everything else again): the launch's nodes are slots tree_lo .. tree_lo + nruns of one
  // level; x / y / th / hits above are that level's half of the particle buffers (node r at (r - tree_dst_lo) * stride), tree_s* the
  // previous level's (the parent at (tree_parent[r] - tree_src_lo) * stride); chain, wp_counts and total hold one entry per slot
  const int* tree_parent;
  const double* tree_sx; const double* tree_sy; const double* tree_sth;
  const uint32_t* tree_shits;
  int tree_lo, tree_dst_lo, tree_src_lo, tree_pad;   // the launch's first slot, its level's, the previous level's
  // an obstacle schedule (pocs_set_obstacle_schedule; behind everything else again).  Every per-waypoint launch gets the record
  // of its own waypoint in `env` above; only the fused roll-out walks the array: env[min(w, env_steps - 1)] at waypoint w
  int env_steps;                       // pocs_launch_mc_fused: > 1 = k_mc_fused_sched over env[0 .. env_steps); 0 / 1: one world, k_mc_fused
  int env_pad;
  // per-obstacle collision counts (POCS_OPT_OBSTACLE_COUNTS; behind everything else again): needs wp_mode != 0
  unsigned long long* obs_counts;      // [nruns][W][POCS_MAX_OBSTACLES] particles of the shard whose FIRST collision is at waypoint w and which touch
                                       // box m there (a tree: one row per slot); non-null: the kernels' MC_BOXES forms
  // a large collision world (pocs_set_world; behind everything else again): k_mc_init_world / k_mc_step_world, which cull the table
  // per wave and particle iteration (mc_world_collides); `env` carries the footprint and no record
  const double* world;                 // [world_M][POCS_OBS_STRIDE]; non-null: a large world
  int world_M;
  int world_pad;
  // clearance levels (pocs_set_clearance_levels; behind everything else again): non-null = the MC_CLEAR forms of k_mc_init /
  // k_mc_step_counts (per-step launches only), which keep per particle the smallest level it has been within so far and count per
  // level the particles that are within it at waypoint w and at no waypoint before
  const pocs_clear_dev* clr;           // the record of the launch's waypoint (aimed with `env`)
  unsigned long long* clr_counts;      // [nruns][W][POCS_MAX_CLEARANCE_LEVELS]; zeroed inside the graph like obs_counts
  unsigned char* clr_level;            // [nruns][stride] the particle's smallest level so far (clr_L: none); written by k_mc_init
  int clr_L;
  int clr_pad;
  // a compound footprint (pocs_set_footprint_parts with F > 1): non-null = the MC_PARTS forms of k_mc_init and the per-step kernels
  const pocs_parts_dev* parts;
  int parts_F;
  int parts_pad;
  // watched regions (pocs_set_regions; behind everything else again): non-null = the MC_REGIONS forms of k_mc_init /
  // k_mc_step_counts (per-step launches only; never with a large world, per-box counts, levels or parts), which also count per
  // region the particles that have collided at no waypoint so far and are in the region at the launch's waypoint
  const pocs_regions_dev* regions;
  unsigned long long* reg_counts;      // [nruns][W][POCS_MAX_REGIONS]; zeroed inside the graph like obs_counts
  int reg_G;                           // 1 .. POCS_MAX_REGIONS
  int reg_pad;
  // segment checks (pocs_set_segment_checks with J > 1; behind everything else again): non-null = the MC_SEG forms of
  // k_mc_step_counts (per-step launches only, wp_mode 1 or 2; never with a large world, per-box counts, levels, parts or regions): a
  // particle also touches at waypoint step + 1 when one of its J - 1 sub-poses on the way there does, and the particles whose first
  // touching waypoint this is and whose end pose is free are counted
  const pocs_seg_dev* seg;
  unsigned long long* seg_counts;      // [nruns][W]; zeroed inside the graph like obs_counts
  // round obstacles (pocs_set_discs with D > 0; behind everything else again): nonzero = the MC_ROUND forms of k_mc_init and
  // k_mc_step_counts (per-step launches only, every wp_mode; never with a large world, per-box counts, levels, parts, regions or
  // segment checks): the table in `env` may hold disc records behind its boxes
  int round;
  int round_pad;
  // uncertain discs (pocs_set_disc_covariances with a nonzero row; behind everything else again): non-null = the MC_NOISE forms on top
  // of the MC_ROUND forms (`round` is nonzero too): the rows of the records of `env` for the launch's waypoint, aimed with `env`;
  // noise_persistent nonzero: the deviations' waypoint word is 0 at every waypoint (a particle's world keeps its deviation),
  // otherwise the launch's waypoint
  const double* noise;
  int noise_persistent;
  int noise_pad;
  // a round footprint (pocs_set_footprint_disc; behind everything else again): nonzero = the MC_RFOOT forms on top of the MC_ROUND
  // forms (`round` is nonzero too, with or without discs; `noise` non-null: on top of MC_NOISE as well).  The radius is env->fp.hx
  int rfoot;
  int rfoot_pad;
  // prediction hypotheses (pocs_set_disc_hypotheses; behind everything else again): non-null = the MC_HYP forms on top of the MC_ROUND
  // forms (`round` is nonzero too; `noise` non-null: on top of MC_NOISE as well; never `rfoot`): the gates of the records of `env`,
  // the same at every waypoint.  The waypoint word of the existence draws is 0 at every waypoint: a particle's world keeps its
  // alternative for the whole roll-out
  const uint32_t* gates;
};

// The launches.  hipErrorInvalidValue: the record is refused -- for the launches that choose among kernels (gmm_step, gmm_tree_step,
// mc_init, mc_step, mc_fused, mc_tree_step) by their chooser in pocs_launch_forms.hpp -- and nothing was launched.
hipError_t pocs_launch_gmm_step(int K, const pocs_gmm_launch& a, hipStream_t s);              // grid = a.blocks
hipError_t pocs_launch_world_cull(int K, const pocs_gmm_launch& a, hipStream_t s);            // grid = a.run_cnt: one block per run of the launch
hipError_t pocs_launch_gmm_advance(int K, const pocs_gmm_launch& a, hipStream_t s);
hipError_t pocs_launch_gmm_tree_advance(int K, const pocs_gmm_launch& a, hipStream_t s);    // grid = a.run_cnt: the nodes of one level
hipError_t pocs_launch_gmm_tree_step(int K, const pocs_gmm_launch& a, hipStream_t s);       // grid = a.blocks
hipError_t pocs_launch_gmm_close(int K, const pocs_gmm_launch& a, hipStream_t s);             // lone call: the last waypoint's rows -> moments
hipError_t pocs_launch_gmm_exchange(int K, const pocs_gmm_launch& a, const pocs_xchg_dev& x, hipStream_t s);   // grid = a.nruns
hipError_t pocs_launch_zero_counts(unsigned long long* p, size_t words, hipStream_t s);     // a kernel, not a memset: it sits inside the replayed graphs
hipError_t pocs_launch_copy(const void* src, void* dst, long long bytes, hipStream_t s);
hipError_t pocs_launch_fill(void* dst, long long bytes, hipStream_t s);
hipError_t pocs_launch_probe_math(const pocs_tables* tables, int n, const uint32_t* wr, const uint32_t* wa, const double* x, double* out, hipStream_t s);   // out: 5 x n
// words first .. first + count - 1 (inside 0 .. 2^32 - 1); out[0] += the words whose two radius roots differ, out[1] = min(out[1], the smallest)
hipError_t pocs_launch_probe_radius_roots(const pocs_tables* tables, uint32_t first, unsigned long long count, unsigned long long* out, hipStream_t s);
// one block; a: env, tables, param (the K records of ONE mixture: W = 1), fp, fp_rr, fp_phi, M -- nothing else is read.
// x / y / th: n poses; flags: 3 x n (full table, pair, pair EAGER); nkeep: 1; kept: POCS_MAX_OBSTACLES records
hipError_t pocs_launch_probe_collide(int K, const pocs_gmm_launch& a, int n, const double* x, const double* y, const double* th,
                                     int* flags, int* nkeep, double* kept, hipStream_t s);
// one block; poses n x (x, y, th) by component; level_out[i]: -1 the footprint itself touches, else the smallest level, L for none
// (+100 should the pair form ever disagree with the single-pose form).  env: base records of M boxes; clr: the grown ones
hipError_t pocs_launch_probe_clearance(const pocs_env_dev* env, const pocs_clear_dev* clr, int L, const pocs_tables* tables, int n,
                                       const double* x, const double* y, const double* th, int* level_out, hipStream_t s);
// one block; poses n x (x, y, th) by component; touched_out[i]: bit f = part f touches (bit 8 should the pair form ever disagree with
// the single-pose form).  env: records of M boxes prepared for the covering part; parts: F parts
hipError_t pocs_launch_probe_parts(const pocs_env_dev* env, const pocs_parts_dev* parts, int F, const pocs_tables* tables, int n,
                                   const double* x, const double* y, const double* th, int* touched_out, hipStream_t s);
// one block; poses n x (x, y, th) by component; mask_out[i]: bit g = pose i is in region g by the single-pose form (bit 8 + g should
// the pair form ever disagree with it)
hipError_t pocs_launch_probe_regions(const pocs_regions_dev* regions, int G, const pocs_tables* tables, int n,
                                     const double* x, const double* y, const double* th, int* mask_out, hipStream_t s);
// one block; poses n x (x, y, th) by component; env: records of M boxes and the footprint; seg: J and the fractions; u: the control;
// backward 0: the MC form from the start pose, 1: the GMM form from the sample.  mask_out[i]: bit j (1 <= j < J) = sub-pose j touches,
// bit J = the end pose (mc_move's, or the sample itself) touches, bit 16 should the pair form ever disagree with the single-pose form
hipError_t pocs_launch_probe_segment(const pocs_env_dev* env, const pocs_seg_dev* seg, const pocs_tables* tables, double u0, double u1,
                                     double u2, int backward, int n, const double* x, const double* y, const double* th, int* mask_out,
                                     hipStream_t s);
// one block; poses n x (x, y, th) by component; env: the composed records (boxes, then discs) and the footprint.  out[i]: bit 0 = pose
// i touches some box, bit 1 = some disc (the single-pose form on the full table), bit 8 should the pair form ever disagree with it
hipError_t pocs_launch_probe_discs(const pocs_env_dev* env, const pocs_tables* tables, int n, const double* x, const double* y,
                                   const double* th, int* out, hipStream_t s);
// one block; poses n x (x, y, th) by component, pose i has index first + i (first even); env: the D disc records alone, grown; rows:
// their noise rows.  centres[(i * D + d) * 2 ..]: disc d's displaced centre for pose i; flags[i]: bit d = pose i touches displaced disc
// d (the single-pose form), bit 31 should the pair form ever disagree with it
hipError_t pocs_launch_probe_disc_noise(const pocs_env_dev* env, const double* rows, const pocs_tables* tables, unsigned long long seed,
                                        unsigned v, unsigned long long first, int n, const double* x, const double* y, const double* th,
                                        double* centres, unsigned* flags, hipStream_t s);
// one block; poses n x (x, y, th) by component, pose i has index first + i (first even); env: the D <= 32 disc records alone, grown;
// rows: their noise rows (zeros: no covariances); gates: their gates; v: the waypoint word of deviations and existence draws alike.
// exists[i]: bit d = disc d exists for pose i; flags[i]: bit d = pose i touches disc d (the single-pose form; both); exists 0 and
// flags all ones should the pair form ever disagree with it
hipError_t pocs_launch_probe_disc_hypotheses(const pocs_env_dev* env, const double* rows, const uint32_t* gates, const pocs_tables* tables,
                                             unsigned long long seed, unsigned v, unsigned long long first, int n, const double* x,
                                             const double* y, const double* th, unsigned* exists, unsigned* flags, hipStream_t s);
// one block; poses n x (x, y, th) by component, pose i has index first + i (first even); env: the composed records (boxes, then discs)
// prepared for the round footprint of radius env->fp.hx; rows: null, or the records' noise rows.  out[i]: bit 0 = pose i touches some
// box, bit 1 = some disc, displaced where its row says so (the single-pose form on the full table), bit 8 should the pair form ever
// disagree with it
hipError_t pocs_launch_probe_footprint_disc(const pocs_env_dev* env, const double* rows, const pocs_tables* tables, unsigned long long seed,
                                            unsigned v, unsigned long long first, int n, const double* x, const double* y, int* out,
                                            hipStream_t s);
// one thread per case; K / seeds / wp / n_total: n; w / alive / out: n rows of POCS_MAX_GAUSSIANS (case i uses the first K[i]): raw weights
// and alive flags in, cumulative component counts out (pocs_normalise_weights + pocs_component_counts, as advance_finish and
// speculate_counts call them)
hipError_t pocs_launch_probe_counts(int n, const int* K, const double* w, const double* alive, const unsigned long long* seeds, const uint32_t* wp,
                                    const double* n_total, double* out, hipStream_t s);
hipError_t pocs_launch_mc_init(int nblk, const pocs_mc_launch& a, hipStream_t s);
hipError_t pocs_launch_mc_step(int nblk, const pocs_mc_launch& a, hipStream_t s);
hipError_t pocs_launch_mc_fused(int nblk, const pocs_mc_launch& a, hipStream_t s);
hipError_t pocs_launch_mc_count(int nblk, const pocs_mc_launch& a, hipStream_t s);
hipError_t pocs_launch_mc_tree_step(int nblk, const pocs_mc_launch& a, hipStream_t s);

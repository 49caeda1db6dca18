// pocs_ctx.hpp -- what the units of the host runtime share: the context behind the C ABI (include/pocs.h) with its
// sub-records, error reporting, device buffers, the graph cache's slots, and the functions one unit calls in another.
//
//   pocs_stage.hip   host chain, staging layout, run / tree images, look-ahead cache, upload of a call's runs
//   pocs_host.hip    the run paths: GMM and MC whole calls, their tree forms, the step and exchange API
//   pocs_api.hip     context life cycle, setters, getters, run-ahead front, text dispatcher
//   pocs_audit.hip   read-backs of device state for tests and audits, bandwidth measurements, timing getters
//   pocs_probe.hip   the test hooks pocs_probe_device_*
//   pocs_modes.hpp   the modes a context can be in and the table of the pairs that exclude each other (no HIP type)
//
// Host only: none of these units holds a kernel (pocs_kernels.hip does, with its parts pocs_dev_*.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/pocs.h"
#include "pocs_kernels.h"
#include "pocs_modes.hpp"

// Everything internal to the host runtime lives in this namespace and stays out of the library's dynamic symbols.
#define POCS_HIDDEN __attribute__((visibility("hidden")))

namespace pocs_rt POCS_HIDDEN {

// A device buffer the context owns: freed with the context (pocs_destroy selects the device first), grown by `ensure`.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
};

enum class Kind { None, Gmm, Mc };      // the estimator a call ran, a result belongs to, a cached run-ahead batch serves

// candidate plans (pocs_set_plans): n > 0 = every run* call evaluates n plans, one run each, in one batch.  The context's W is
// then the longest plan's length (the stride of every [run][W] array) and its batch = n; the single plan's length and
// the batch wait in single_W / single_batch (enter_multi) for pocs_set_plans(ctx, 0, ...).
struct PlanSet {
  int n = 0;
  std::vector<int> W;                             // [P]
  std::vector<size_t> toff, ooff;                 // [P] where plan p starts in traj (3 x W_p) / odom (3 x (W_p - 1))
  std::vector<double> traj, odom;
};

// a tree of candidate plans (pocs_set_plan_tree): n > 0 = every run* call evaluates the n nodes once each.  On the device a node
// is a SLOT: the nodes level by level (BFS), every level a contiguous range of slots, and every per-run array holds one row
// per slot -- while a tree is set the context's W = 1 and its batch = n (the single plan's length and batch wait in single_W /
// single_batch, as under pocs_set_plans; a tree and a set of plans exclude each other).
struct PlanTree {
  int n = 0;
  std::vector<int> parent, depth;                 // [T], the caller's node order
  std::vector<double> pose, odom;                 // 3 x T by component: the node's pose, the control of the edge into it
  std::vector<int> slot, node;                    // node -> slot, slot -> node
  std::vector<int> level;                         // [D + 2]: level d = slots [level[d], level[d + 1])
  std::vector<int> pslot;                         // [T] the slot of every slot's parent (slot 0: 0), as uploaded to d_tparent
  bool dirty = false;
};

// Everything that describes the last call: what the getters serve.  A new set of plans and a call that fails after its launches
// leave none of it (reset_results).
struct Results {
  Kind last_kind = Kind::None;           // what the last launch was (on a tree: what the last call on the tree was, tree_last)
  uint64_t batch_base = 0;               // run_index of run 0 of the last launch
  int batch_R = 1;                       // runs in the last launch
  int view = 0;                          // the run of the last launch the getters expose
  std::vector<double> h_chain;           // (W-1) x POCS_CHAIN_STRIDE
  std::vector<double> h_mu, h_cov;       // (W-1) x 3, (W-1) x 9 : main EKF after each step
  std::vector<double> probs;             // W (the selected run of the last batch)
  std::vector<double> batch_probs;       // final probability of every run of the last batch
  std::vector<unsigned long long> mc_counts;   // collided particles of every run of the last MC batch (this shard)
  std::vector<double> last_moments;      // W x K x 11 (the selected run)
  std::vector<double> batch_moments;     // [W][R][K*11] of the last GMM launch
  long long last_gmm_count = 0, last_mc_count = 0;
  int last_gmm_wp = -1;
  std::vector<int> plan_slot_[2];        // the batch slot of plan p in the last GMM / MC call of plans: through plan_slot(kind)
  std::vector<int>& plan_slot(Kind k) { return plan_slot_[k == Kind::Mc]; }
  const std::vector<int>& plan_slot(Kind k) const { return plan_slot_[k == Kind::Mc]; }
  std::vector<int> plan_E;               // [P] waypoints evaluated per plan in the last GMM call of plans (empty: there was none)
  std::vector<unsigned long long> mc_wp; // [R][mc_wp_W] first collisions per waypoint of the last MC call, in run / plan order (empty: the call ran without)
  int mc_wp_W = 0;
  std::vector<int> plan_E_mc;            // [P] waypoints evaluated per plan in the last MC call of plans under the bound (empty: every plan to its end)
  int tree_sel = 0;                      // the node the getters show (pocs_select_tree_node)
  std::vector<double> tree_probs;                 // [T] node order: running probability of the path root -> n
  std::vector<unsigned char> tree_eval;           // [T] 1 evaluated, 0 cut off below a stopped ancestor
  std::vector<unsigned long long> tree_F, tree_C; // [T] MC: first collisions at the node, collided at or before it
  size_t tree_mc_half = 0;                        // MC: elements of one level's half of the particle buffers
  // per-obstacle collision counts (POCS_OPT_OBSTACLE_COUNTS): the table stays on the device ([slot][oc_W][POCS_MAX_OBSTACLES], d_obsct)
  // and pocs_get_obstacle_counts reads the selected run's rows; this is what the last call left there
  Kind oc_kind = Kind::None;                      // None: the last call ran with the option off (or there was none)
  int oc_M = 0, oc_W = 0;                         // boxes of the call's world, rows per slot
  // clearance levels (pocs_set_clearance_levels): the table of the last call, read back with its results ([slot][cl_W][cl_L]), and
  // why there is none to serve (pocs_get_clearance_counts names it)
  enum ClearState { ClNoCall, ClOff, ClTouched, ClNotApplied, ClServed };
  ClearState cl_state = ClNoCall;
  Kind cl_kind = Kind::None;
  int cl_L = 0, cl_W = 0;
  long long cl_N = 0;                             // samples / particles per waypoint of the call: the probabilities' divisor
  std::vector<unsigned long long> cl_counts;
  // watched regions (pocs_set_regions): the table of the last call, read back with its results in slot order
  // ([slot][rg_W][POCS_MAX_REGIONS]), and why there is none to serve (pocs_get_region_counts names it)
  enum RegionState { RgNoCall, RgOff, RgTouched, RgNotApplied, RgServed };
  RegionState rg_state = RgNoCall;
  Kind rg_kind = Kind::None;
  int rg_G = 0, rg_W = 0;
  long long rg_N = 0;                             // samples / particles per waypoint of the call: the probabilities' divisor
  std::vector<unsigned long long> rg_counts;
  // segment checks (pocs_set_segment_checks): the segment counts B of the last call, read back with its results in slot order
  // ([slot][sg_W]), and why there are none to serve (pocs_get_segment_counts names it)
  enum SegState { SgNoCall, SgOff, SgTouched, SgNotServed, SgServed };
  SegState sg_state = SgNoCall;
  Kind sg_kind = Kind::None;
  int sg_J = 1, sg_W = 0;
  std::vector<unsigned long long> sg_counts;
};

// One cached graph and its signature: the bytes of its launches in issue order (Issuer, pocs_host.hip), compared before a replay.
struct GraphSlot { hipGraphExec_t exec = nullptr; std::vector<unsigned char> sig; long long captures = 0; };

// The synchronisation words of one GMM call (pocs_kernels.h), a block of d_ticket that ONE memset zeroes at the head of the call:
// [1] give-up code, [0], [2..3] pad, then -- under a risk bound -- the runs' stop words [R] (padded to 4: they travel back with the
// give-up word in one copy), the tickets [R][W], the closers' exchange waits [R][W].  Computed once per call (gmm_prepare) and
// kept as the layout of the LAST call: what its getters read with.
struct SyncLayout {
  size_t stop = 4, ticket = 4, xwait = 4, words = 0;      // word offsets; the block's words, a multiple of 4 (0: no GMM call yet)
  size_t cells = 0;                                        // R x W: tickets, and exchange waits
  size_t pin = 0, copy_words = 1;                          // the give-up word's place in pinned memory (doubles from h_pin) and the words
};                                                         // its copy moves: the stop words land stop - POCS_SYNC_ABORT behind it

}  // namespace pocs_rt

struct pocs_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr;
  // A call of many runs is issued as `groups` sub-batches on streams of their own (gmm_groups): while one
  // sub-batch is in the tail of a waypoint's launch (the last blocks' slower waves, the serial mixture
  // advance of its closers, the launch boundary) the others' sampling blocks have the SIMDs.
  hipStream_t side_stream[3] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr}, ev_seq[2] = {nullptr, nullptr};
  double seq_ms = 0.0;                   // POCS_OPT_PROFILE: first launch -> last launch's end of the last whole-run call
  int seq_groups = 1;
  std::string err;

  // ---- configuration (what MCSimulator holds, MCSimulator.h:94-136) ----
  double alphas[4] = {1, 1, 1, 1};      // ones, as the reference ctor leaves them (:143)
  bool have_alphas = false;
  pocs_sensor sensor;
  bool have_q = false, have_landmarks = false;
  int num_landmarks = -1;
  long long num_particles = -1;
  double cov0[9];
  bool have_cov0 = false;
  int W = -1;
  std::vector<double> traj, odom;        // by component: 3 x W, 3 x (W-1)
  bool have_traj = false, have_odom = false;
  int K = -1;
  long long num_gmm = -1;
  uint64_t seed = 0x5EED0001ull;
  uint64_t run_index = 0;
  pocs_footprint fp = {0.0, 0.0, 0.334, 0.334};
  std::vector<double> boxes;             // world_S x M x 5: world s is the collision world at waypoint s (the last one holds behind it)
  int world_S = 1;                       // steps of the obstacle schedule (pocs_set_obstacle_schedule); 1: a static world (pocs_set_obstacles)
  bool have_obstacles = false;           // pocs_set_obstacles / addObstacle / clearObstacles was called at least once
  // a large static world (pocs_set_world with more than POCS_MAX_OBSTACLES boxes): M x 5, and `boxes` above is empty -- the table
  // of at most POCS_MAX_OBSTACLES records that every kernel stages holds nothing then; empty: no large world
  std::vector<double> world;
  // how many records the cull of the last GMM call under a large world kept per waypoint (pocs_get_world_reach), in run / plan
  // order: [reach_R][reach_W], and the waypoints of each row that mean something.  Not part of `res`: it outlives a call that
  // failed on overflow
  std::vector<int> reach, reach_len;
  int reach_R = 0, reach_W = 0;
  long long shard_first = -1, shard_count = -1;
  long long opt_store = 1, opt_fused = 0, opt_graph = 1, opt_profile = 0, opt_lone = 1, opt_groups = 0, opt_mc_nt = -1;
  unsigned long long epoch = 0;          // bumped by every setter: the look-ahead image (`ahead`) is valid for one epoch
  int batch = 1;                         // independent GMM estimations advanced in lockstep per call
  // run-ahead (POCS_OPT_RUN_AHEAD): with batch == 1 a run* call evaluates the next `run_ahead` runs
  // of the context in one launch and the following calls are served from it (res.view: the one served last).
  int run_ahead = 1;
  int ra_have = 0;                       // runs of the last launch that may still be served (0: none)
  pocs_rt::Kind ra_kind = pocs_rt::Kind::None;
  bool ra_internal = false;              // the last launch was an internal run-ahead batch

  pocs_rt::PlanSet plans;
  pocs_rt::PlanTree tree;
  int single_W = -1, single_batch = 1;   // the single plan's W / batch while plans or a tree hold the context's (enter_multi)
  long long opt_plan_seeds = 0;          // POCS_OPT_PLAN_SEEDS
  // risk bound of calls of plans (pocs_set_plan_risk_bound): a plan whose running probability reaches it is not evaluated
  // any further (k_gmm_step_risk decides and obeys on the device; gmm_combine restates the rule on the moments read back)
  double risk_bound = 1.0;               // >= 1: off
  // first collisions per waypoint of MC calls (POCS_OPT_MC_WAYPOINT_COUNTS) and the risk bound obeyed by them
  // (POCS_OPT_MC_RISK_BOUND): k_mc_*_counts count, k_mc_step_counts<.., MC_STOP> decides and obeys; run_mc_local restates the
  // rule on the counts read back
  long long opt_mc_wp = 0, opt_mc_rb = 0;
  // per-obstacle collision counts (POCS_OPT_OBSTACLE_COUNTS): the launches are the kernels' _boxes / MC_BOXES forms
  long long opt_obs_counts = 0;
  // clearance levels (pocs_set_clearance_levels): L = 0 is off.  Applied to whole calls on one GPU over a small world (clearance_applied,
  // pocs_host.hip); everywhere else a call is the call it is with L = 0
  int clr_L = 0;
  double clr_d[POCS_MAX_CLEARANCE_LEVELS] = {0.0, 0.0, 0.0, 0.0};
  // watched regions (pocs_set_regions): G = 0 is off.  Applied where regions_applied (pocs_host.hip) says; everywhere else a call is
  // the call it is with G = 0
  int reg_G = 0;
  double reg_box[POCS_MAX_REGIONS * 5] = {};
  int reg_kind[POCS_MAX_REGIONS] = {};
  // a compound footprint (pocs_set_footprint_parts): F = 1 is the single box `fp`.  F > 1: `fp` is part 0, every call is served by the
  // kernels' _parts / MC_PARTS forms (parts_applied, pocs_host.hip) and the modes of pocs_modes::kPartsExcluded are refused
  int fp_F = 1;
  pocs_footprint fp_parts[POCS_MAX_FOOTPRINT_PARTS] = {};
  // segment checks (pocs_set_segment_checks): J = 1 is off -- every call is, launch for launch, what it is without this.  J > 1: every
  // call is served by the kernels' _seg / MC_SEG forms (seg_applied) and the modes of pocs_modes::kSegExcluded and a compound
  // footprint are refused
  int seg_J = 1;
  // round obstacles (pocs_set_discs): disc_D = 0 is off -- every call is, launch for launch, what it is without this.  D > 0: disc_S
  // tables of D discs {cx, cy, r}, table min(w, disc_S - 1) in force at waypoint w beside box step min(w, world_S - 1); upload_world
  // composes the two into the env records (boxes, then discs), every call is served by the kernels' _round / MC_ROUND forms
  // (discs_applied) and the modes of pocs_modes::kDiscExcluded, a compound footprint and segment checks are refused
  std::vector<double> discs;             // disc_S x disc_D x 3
  int disc_D = 0, disc_S = 1;
  // uncertain discs (pocs_set_disc_covariances): empty is off -- every call is, launch for launch, the discs call it is without this
  // (a table of zeros is stored as empty).  Otherwise disc_S x disc_D x {sxx, sxy, syy}, every row zeros or a covariance the setter
  // has factorised once already; upload_world factorises them again into d_noise ([env_steps][POCS_MAX_OBSTACLES] rows {l00, l10, l11,
  // disc index}, record by record beside d_env) and grows the disc records, and every call is served by the _noise / MC_NOISE forms
  std::vector<double> disc_cov;
  int disc_noise_persistent = 0;         // the MC path's waypoint word: 1 = 0 at every waypoint, 0 = the waypoint
  // prediction hypotheses (pocs_set_disc_hypotheses): empty is off -- every call is, launch for launch, the call it is without this (a
  // table whose groups are all -1 is stored as empty).  Otherwise disc_D groups and weights as the caller gave them, which the setter
  // has turned into thresholds once already; upload_world forms them again into d_gates ([POCS_MAX_OBSTACLES] gates {lo, hi - 1, g, on},
  // record by record, the same at every env step) and every call is served by the _hyp / MC_HYP forms
  std::vector<int> hyp_group;
  std::vector<double> hyp_weight;
  // a round footprint (pocs_set_footprint_disc): fp_round = false is off -- every call is, launch for launch, what it is without this.
  // On: the robot is the disc of radius fp_rho centred on the pose; `fp` is its bounding square {0, 0, rho, rho} and fp_F = 1 (what
  // pocs_get_footprint_parts reports), upload_world prepares every record with rho as the bounding radius, every call is served by
  // the kernels' _rfoot / MC_RFOOT forms (rfoot_applied) and the modes of pocs_modes::kRoundFpExcluded and segment checks are refused
  bool fp_round = false;
  double fp_rho = 0.0;

  // host image (headers | chains | initial mixtures) of the NEXT batch, computed while the GPU
  // works on the current one
  struct {
    bool valid = false;
    uint64_t seed = 0, run_index = 0;
    int R = 0;
    unsigned long long epoch = 0;
    std::vector<double> image, chain0, mu0, cov0;
    std::vector<int> slot_plan;          // a call of plans: the layout the image was built for
  } ahead;

  // ---- device state ----
  pocs_rt::DevBuf d_env, d_sensor, d_hdr, d_chain, d_state, d_param, d_moments, d_partial;
  pocs_rt::DevBuf d_sx, d_sy, d_st, d_flags, d_px, d_py, d_pt, d_hits, d_total, d_ticket, d_tables;
  pocs_rt::DevBuf d_runplan;             // a call of plans: [R][4] start mean and steps per run (the MC kernels)
  pocs_rt::DevBuf d_surv;                // a call of plans under a risk bound: [R] running survival product of every run
  pocs_rt::DevBuf d_tparent;             // a tree of plans: [T] int, the slot of every slot's parent
  // a large world: its prepared records [M][POCS_OBS_STRIDE]; per batch slot the records k_world_cull kept for the waypoint being
  // sampled [slots][POCS_MAX_OBSTACLES][POCS_OBS_STRIDE], their indices in the caller's table [slots][POCS_MAX_OBSTACLES] int, and the
  // kept counts [slots][W] int, zeroed at the head of every call
  pocs_rt::DevBuf d_world, d_kept, d_keptidx, d_reach;
  // clearance levels: [world_S] pocs_clear_dev beside d_env (upload_world), the counters [slots][W][POCS_MAX_CLEARANCE_LEVELS] u64 zeroed
  // by a kernel at the head of every call's launches, and the MC particles' smallest level so far [slots][stride] u8
  pocs_rt::DevBuf d_clr, d_clrct, d_clrlv;
  // watched regions: one pocs_regions_dev beside d_env (upload_world) and the counters [slots][W][POCS_MAX_REGIONS] u64, zeroed by a
  // kernel at the head of every call's launches
  pocs_rt::DevBuf d_reg, d_regct;
  pocs_rt::DevBuf d_parts;               // a compound footprint: one pocs_parts_dev beside d_env (upload_world)
  // segment checks: one pocs_seg_dev beside d_env (upload_world: J and the fractions live in device memory, so another J > 1 replays
  // the cached graph) and the segment counts [slots][W] u64, zeroed by a kernel at the head of every call's launches
  pocs_rt::DevBuf d_seg, d_segct;
  pocs_rt::DevBuf d_noise;               // uncertain discs: the noise rows, an allocation of its own (pocs_env_dev keeps its layout)
  pocs_rt::DevBuf d_gates;               // prediction hypotheses: the records' gates, POCS_MAX_OBSTACLES x POCS_GATE_STRIDE words (a fixed size: new weights replay the graph)
  pocs_rt::DevBuf d_obsct;               // POCS_OPT_OBSTACLE_COUNTS: [slots][W][POCS_MAX_OBSTACLES] u64, zeroed by a kernel at the head of every call's launches
  // one-hop exchange (pocs_xchg_*): this rank's buffer, the peers' buffers as mapped here
  void* xchg_own = nullptr;
  void* xchg_peer[POCS_XCHG_MAX_WORLD] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int xchg_world = 0, xchg_rank = -1;
  bool xchg_connected = false;
  unsigned long long xchg_calls = 0;     // begin/end sequences so far: part of every row's epoch
  double* ext_moments = nullptr;         // caller-owned moments buffer (multi-GPU), or null
  long long ext_moments_len = 0;
  void* h_pin = nullptr;                 // pinned staging: hdr | chain | state0 | moments | total
  size_t h_pin_cap = 0;
  void* h_copy = nullptr;                // pinned staging of the audit copies (pocs_copy_*, pocs_get_gmm_state): device data
                                         // reaches caller memory through it, in pieces of POCS_COPY_CHUNK bytes
  bool env_dirty = true, sensor_dirty = true;

  pocs_rt::GraphSlot graph_gmm, graph_mc;
  std::vector<unsigned char> sig;        // the signature of the call being made (kept for its capacity)
  pocs_rt::SyncLayout sync;              // of the last GMM call

  std::vector<hipEvent_t> events;
  double prof_ms = 0.0;
  long long prof_launches = 0;

  pocs_rt::Results res;                  // ---- results of the last run ----
  int last_gmm_adv = -1;                 // last waypoint whose mixture has been built (step API)
  bool gmm_open = false;
};

namespace pocs_rt POCS_HIDDEN {

inline int fail(pocs_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

#define HIPCHK(c, call)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail((c), POCS_E_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                  __FILE__, __LINE__);                                                    \
  } while (0)

inline void drop_graphs(pocs_ctx* c) {
  for (GraphSlot* g : {&c->graph_gmm, &c->graph_mc}) {
    if (g->exec) { hipGraphExecDestroy(g->exec); g->exec = nullptr; }
    g->sig.clear();
  }
}

// Grow a device buffer (its pointer is part of the signature of the launches that use it: the next call captures its graph again).
inline int ensure(pocs_ctx* c, DevBuf& b, size_t bytes) {
  if (bytes == 0) bytes = 16;
  if (b.cap >= bytes) return POCS_OK;
  if (b.p) {
    HIPCHK(c, hipStreamSynchronize(c->stream));      // nothing queued may still use the old buffer
    void* old = b.p;
    b.p = nullptr; b.cap = 0;                        // (before the free is checked: a DevBuf never keeps a pointer it does not own)
    HIPCHK(c, hipFree(old));
  }
  HIPCHK(c, hipMalloc(&b.p, bytes));
  b.cap = bytes;
  return POCS_OK;
}

// Run-ahead bookkeeping.  A setter (or any other launch) ends the serving of cached runs: the
// context's run counter goes back to just after the last run that was handed out, so the sequence
// of seeds the caller sees is the one it would have seen one run per launch.
inline void ra_drop(pocs_ctx* c) {
  if (c->ra_have > 0) c->run_index = c->res.batch_base + (uint64_t)c->res.view + 1;
  c->ra_have = 0;
}
inline void touch(pocs_ctx* c) { ra_drop(c); c->epoch++; }

// The one place that clears the results of the last call.  clear(), not = {}: a planner sets new plans before every call, and
// the calls' assign / resize then find their buffers still allocated.
inline void reset_results(pocs_ctx* c) {
  Results& r = c->res;
  r.last_kind = Kind::None; r.batch_base = 0; r.batch_R = c->batch; r.view = 0;
  r.h_chain.clear(); r.h_mu.clear(); r.h_cov.clear();
  r.probs.clear(); r.batch_probs.clear(); r.mc_counts.clear(); r.last_moments.clear(); r.batch_moments.clear();
  r.last_gmm_count = 0; r.last_mc_count = 0; r.last_gmm_wp = -1;
  r.plan_slot(Kind::Gmm).clear(); r.plan_slot(Kind::Mc).clear(); r.plan_E.clear();
  r.mc_wp.clear(); r.mc_wp_W = 0; r.plan_E_mc.clear();
  r.tree_sel = 0; r.tree_mc_half = 0;
  r.tree_probs.clear(); r.tree_eval.clear(); r.tree_F.clear(); r.tree_C.clear();
  r.oc_kind = Kind::None; r.oc_M = 0; r.oc_W = 0;
  r.cl_state = Results::ClNoCall; r.cl_kind = Kind::None; r.cl_L = 0; r.cl_W = 0; r.cl_N = 0; r.cl_counts.clear();
  r.rg_state = Results::RgNoCall; r.rg_kind = Kind::None; r.rg_G = 0; r.rg_W = 0; r.rg_N = 0; r.rg_counts.clear();
  r.sg_state = Results::SgNoCall; r.sg_kind = Kind::None; r.sg_J = 1; r.sg_W = 0; r.sg_counts.clear();
}

// The collision world: M boxes per step, and the record of the device's env array ([world_S] pocs_env_dev) that waypoint w --
// a launch's waypoint, a tree level's depth -- is tested against.
inline int world_boxes(const pocs_ctx* c) { return (int)(c->boxes.size() / 5 / (size_t)c->world_S); }
// Round obstacles are set (pocs_set_discs with D > 0).  The env array then holds max(world_S, disc_S) composed records of
// world_boxes + disc_D obstacle records each; without discs both are what they have always been.
inline bool discs_applied(const pocs_ctx* c) { return c->disc_D > 0; }
inline int env_steps(const pocs_ctx* c) { return discs_applied(c) && c->disc_S > c->world_S ? c->disc_S : c->world_S; }
inline int env_records(const pocs_ctx* c) { return world_boxes(c) + c->disc_D; }
// Disc covariances are set and some row is not zero (pocs_set_disc_covariances): the launches carry the rows of their waypoint.
inline bool noise_applied(const pocs_ctx* c) { return discs_applied(c) && !c->disc_cov.empty(); }
// Hypotheses are set and some disc is gated (pocs_set_disc_hypotheses): the launches carry the gate table, and rows of zeros where the
// context has no covariances (upload_world then fills d_noise with zeros).
inline bool hyp_applied(const pocs_ctx* c) { return discs_applied(c) && !c->hyp_group.empty(); }
inline bool noise_rows_held(const pocs_ctx* c) { return noise_applied(c) || hyp_applied(c); }
// what pocs_hyp_thresholds refuses, in words
inline const char* hyp_refusal(int k) {
  return k == 1 ? "a group is -1 (always there) or an index in [0, D)" : k == 2 ? "a weight is finite and in (0, 1]"
       : k == 3 ? "floor(weight * 2^32) is 0: the alternative would never exist" : "the weights of its group sum to more than 1";
}
inline const double* noise_at(const pocs_ctx* c, int w) {
  const int S = env_steps(c);
  return (const double*)c->d_noise.p + (size_t)(w < 0 ? 0 : w < S ? w : S - 1) * (POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE);
}
inline const pocs_env_dev* world_at(const pocs_ctx* c, int w) {
  const int S = env_steps(c);
  return (const pocs_env_dev*)c->d_env.p + (w < 0 ? 0 : w < S ? w : S - 1);
}

inline const pocs_clear_dev* clear_at(const pocs_ctx* c, int w) {
  return (const pocs_clear_dev*)c->d_clr.p + (w < 0 ? 0 : w < c->world_S ? w : c->world_S - 1);
}

// A large world is in force (pocs_set_world with more than POCS_MAX_OBSTACLES boxes), and its number of boxes.
static_assert(POCS_MAX_WORLD_RECORDS == POCS_MAX_WORLD_BOXES, "pocs_kernels.h restates the public limit");
inline int large_boxes(const pocs_ctx* c) { return (int)(c->world.size() / 5); }

// The modes a context is in (pocs_modes.hpp), as a bit word: the one place that says what "plans are set" and the others mean.
inline unsigned modes_of(const pocs_ctx* c) {
  using namespace pocs_modes;
  return (c->plans.n > 0 ? kPlans : 0u) | (c->tree.n > 0 ? kTree : 0u) | (c->shard_first >= 0 ? kShard : 0u) |
         (c->xchg_own ? kXchgCreated : 0u) | (c->xchg_connected ? kXchgConnected : 0u) | (c->ext_moments ? kMoments : 0u) |
         (!c->world.empty() ? kLargeWorld : 0u) | (c->opt_obs_counts ? kObsCounts : 0u) | (c->opt_fused ? kFused : 0u) |
         (c->gmm_open ? kSequence : 0u);
}
inline bool in_mode(const pocs_ctx* c, unsigned any_of) { return (modes_of(c) & any_of) != 0; }
inline bool large_world(const pocs_ctx* c) { return in_mode(c, pocs_modes::kLargeWorld); }

// A compound footprint is set (pocs_set_footprint_parts with F > 1): not a mode of the table -- one mask of the modes it excludes
// (pocs_modes::kPartsExcluded), asked here in front of the table and by the setter itself.
inline bool parts_applied(const pocs_ctx* c) { return c->fp_F > 1; }
inline int parts_refuse(pocs_ctx* c, const char* what, pocs_modes::Mode enter) {
  if (!parts_applied(c) || !(enter & pocs_modes::kPartsExcluded)) return POCS_OK;
  return fail(c, POCS_E_STATE, "%s: a compound footprint is set (pocs_set_footprint_parts); %s", what, pocs_modes::kPartsClause);
}

// Segment checks are set (pocs_set_segment_checks with J > 1): as a compound footprint, one mask (pocs_modes::kSegExcluded) asked in
// front of the table and by the setter itself.
inline bool seg_applied(const pocs_ctx* c) { return c->seg_J > 1; }
inline int seg_refuse(pocs_ctx* c, const char* what, pocs_modes::Mode enter) {
  if (!seg_applied(c) || !(enter & pocs_modes::kSegExcluded)) return POCS_OK;
  return fail(c, POCS_E_STATE, "%s: segment checks are set (pocs_set_segment_checks); %s", what, pocs_modes::kSegClause);
}

// Round obstacles are set: as segment checks, one mask (pocs_modes::kDiscExcluded) asked in front of the table and by the setter.
inline int discs_refuse(pocs_ctx* c, const char* what, pocs_modes::Mode enter) {
  if (!discs_applied(c) || !(enter & pocs_modes::kDiscExcluded)) return POCS_OK;
  return fail(c, POCS_E_STATE, "%s: discs are set (pocs_set_discs); %s", what, pocs_modes::kDiscClause);
}

// A round footprint is in force (pocs_set_footprint_disc): as discs, one mask (pocs_modes::kRoundFpExcluded) asked in front of the
// table, behind the discs' mask, and by the setter itself.
inline bool rfoot_applied(const pocs_ctx* c) { return c->fp_round; }
inline int rfoot_refuse(pocs_ctx* c, const char* what, pocs_modes::Mode enter) {
  if (!rfoot_applied(c) || !(enter & pocs_modes::kRoundFpExcluded)) return POCS_OK;
  return fail(c, POCS_E_STATE, "%s: a round footprint is set (pocs_set_footprint_disc); %s", what, pocs_modes::kRoundFpClause);
}

// May the context enter `enter`, as asked by the call `what`?  The one place that refuses a combination (pocs_modes.hpp).
inline int may_enter(pocs_ctx* c, const char* what, pocs_modes::Mode enter, unsigned among = pocs_modes::kAll) {
  if (among == pocs_modes::kAll) {                   // (a setter's staged asks in front of its argument checks enter nothing yet)
    if (int r = parts_refuse(c, what, enter)) return r;
    if (int r = seg_refuse(c, what, enter)) return r;
    if (int r = discs_refuse(c, what, enter)) return r;
    if (int r = rfoot_refuse(c, what, enter)) return r;
  }
  const pocs_modes::Refusal r = pocs_modes::refusal(modes_of(c), enter, among);
  if (r.code == POCS_OK) return POCS_OK;
  char clause[200];
  snprintf(clause, sizeof clause, r.clause, POCS_MAX_OBSTACLES);
  return fail(c, r.code, "%s: %s; %s", what, pocs_modes::name(r.by), clause);
}

// What the last call on the tree was: last_kind (a failed call, entering and leaving a tree all go through reset_results).
inline Kind tree_last(const pocs_ctx* c) { return c->tree.n ? c->res.last_kind : Kind::None; }

inline double* moments_dev(pocs_ctx* c) { return c->ext_moments ? c->ext_moments : (double*)c->d_moments.p; }
inline long long sample_stride_of(long long count) { return count > 0 ? ((count + 1) & ~1LL) : 2; }   // even
inline uint64_t seed_of_run(const pocs_ctx* c, uint64_t run) { return c->seed + 0x9E3779B97F4A7C15ull * run; }

// ---- pocs_stage.hip ----
// One plan as the host chain and the initial mixture read it: trajectory 3 x W and odometry 3 x (W-1), by component.
struct PlanView { const double* traj; const double* odom; int W; };
PlanView plan_view(const pocs_ctx* c, int p);          // p < 0: the single plan (pocs_set_trajectory / pocs_set_odometry)
void compute_chain(pocs_ctx* c, uint64_t seed, const PlanView& pv);
// pinned staging layout (doubles): [0 .. 2R) run headers, then R chains, then R initial mixtures, (a call of plans:
// then R rows of start mean and steps), then the moments [W][R][K*11], then the MC total
struct PinLayout { size_t chain, state0, runplan, moments, total, end; };
PinLayout pin_layout(const pocs_ctx* c);
int ensure_pin(pocs_ctx* c);
std::vector<int> plan_layout(const pocs_ctx* c, int G);
std::vector<int> slot_lengths(const pocs_ctx* c, const std::vector<int>& slot_plan);
int live_runs(const std::vector<int>& Ws, int lo, int hi, int w);
uint64_t plan_run(const pocs_ctx* c, int p);
void prefetch_next_batch(pocs_ctx* c, int groups);
int stage_and_upload_runs(pocs_ctx* c, int groups, Kind kind);

// ---- pocs_host.hip ----
int upload_tables(pocs_ctx* c);
int upload_world(pocs_ctx* c);
void fill_gmm_world(const pocs_ctx* c, pocs_gmm_launch* a, int w);
size_t obs_count_words(const pocs_ctx* c);
bool clearance_applied(const pocs_ctx* c);
bool regions_applied(const pocs_ctx* c);
double waypoint_probability(const double* row, int K, long long n);
void prepare_regions(const pocs_footprint& fp, const double* boxes, const int* kinds, int G, pocs_regions_dev* out);
void prepare_segment(int J, pocs_seg_dev* out);
void prepare_parts(const pocs_footprint* parts, int F, const double* boxes, int M, pocs_env_dev* env, pocs_parts_dev* out);
void prepare_clearance(const pocs_footprint& fp, const double* d, int L, const double* boxes, int M, pocs_clear_dev* out);
void gmm_select_view(pocs_ctx* c, int v);
void tree_select_gmm(pocs_ctx* c, int n);
int run_gmm_full(pocs_ctx* c, double* probability);
int run_mc_local(pocs_ctx* c);

}  // namespace pocs_rt

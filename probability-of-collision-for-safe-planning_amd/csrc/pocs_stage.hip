// pocs_stage.hip -- what the host prepares for a call before the GPU runs it: the per-waypoint host chain, the pinned
// staging layout, the host image of a batch of runs (or of a tree), the look-ahead cache and the upload of a call's runs.
//
// Mirrors the O(1) part of MCSimulator::EKF_GaussProp (mcsimplugin/MCSimulator.h:649-864).  Everything per particle /
// per sample runs in pocs_kernels.hip.
#include "pocs_ctx.hpp"

namespace pocs_rt POCS_HIDDEN {

// ---------------------------------------------------------------------------------------------
// Host chain: everything in EKF_GaussProp's loop body that does not touch particles/samples
// (MCSimulator.h:692-800): M (generateM_EKF :495-513), gain L and applied control (:714-726,
// generateL :532-553, inverseOdometry :434-449), EKFpredict on the main estimate (:746),
// sampleOdometry (:754, :391-410), the L noisy range observations (:786-789, :383-387) and
// EKFupdate (:797-800).  Noise comes from Philox stream POCS_STREAM_CHAIN, index = step,
// draw order r1, tr, r2, z_0 .. z_{L-1} as in the reference (:403-405, :786-789).
// ---------------------------------------------------------------------------------------------
void inverse_odometry(const double p1[3], const double p2[3], double out[3]) {
  double r1 = atan2(p2[1] - p1[1], p2[0] - p1[0]) - p1[2];
  r1 = pocs_wrap_angle(r1);
  const double ddx = p2[0] - p1[0], ddy = p2[1] - p1[1];
  const double tr = sqrt(ddx * ddx + ddy * ddy);
  double r2 = p2[2] - p1[2] - r1;
  r2 = pocs_wrap_angle(r2);
  out[0] = r1; out[1] = tr; out[2] = r2;
}

double chain_normal(uint64_t seed, int step, int draw) {
  const pocs_u32x4 w = pocs_draw(seed, (uint64_t)step, 0u, POCS_STREAM_CHAIN, (uint32_t)(draw >> 1));
  double n0, n1;
  pocs_normal_pair(w.x, w.y, w.z, &n0, &n1);
  return (draw & 1) ? n1 : n0;
}

PlanView plan_view(const pocs_ctx* c, int p) {          // p < 0: the single plan (pocs_set_trajectory / pocs_set_odometry)
  if (p < 0) return PlanView{c->traj.data(), c->odom.data(), c->W};
  return PlanView{c->plans.traj.data() + c->plans.toff[(size_t)p], c->plans.odom.data() + c->plans.ooff[(size_t)p], c->plans.W[(size_t)p]};
}

// Step i of the chain: from waypoint xs to waypoint xg under the nominal control us, with the normals of step i.  Carries the
// main EKF's mu / cov and the real state across the step and fills the step's record.  A plan applies it along its waypoints
// (compute_chain), a tree of plans from every parent to each of its children (build_tree_image).
void chain_step(const pocs_ctx* c, uint64_t seed, int i, const double us[3], const double xs[3], const double xg[3],
                double mu[3], double cov[9], double real[3], double* rec) {
  const int L = c->sensor.L;
  const double a1 = c->alphas[0], a2 = c->alphas[1], a3 = c->alphas[2], a4 = c->alphas[3];
  // generateM_EKF on the NOMINAL control
  rec[3] = a1 * (us[0] * us[0]) + a2 * (us[1] * us[1]);
  rec[4] = a3 * (us[1] * us[1]) + a4 * (us[0] * us[0]) + a4 * (us[2] * us[2]);
  rec[5] = a1 * (us[2] * us[2]) + a2 * (us[1] * us[1]);
  // generateL + applied control
  double ureq[3], applied[3];
  inverse_odometry(mu, xg, ureq);
  for (int j = 0; j < 3; ++j) {
    const double xhat = mu[j] - xs[j];
    const double ubar = ureq[j] - us[j];
    const double gain = ubar / (xhat != 0 ? xhat : 0.1);
    applied[j] = us[j] + gain * xhat;
    rec[j] = applied[j];
  }
  // EKFpredict on the main estimate
  double pmu[3], pcov[9];
  pocs_ekf_predict(mu, cov, applied, rec + 3, pmu, pcov);
  // sampleOdometry on the APPLIED control
  const double v0 = a1 * (applied[0] * applied[0]) + a2 * (applied[1] * applied[1]);
  const double v1 = a3 * (applied[1] * applied[1]) +
                    a4 * ((applied[0] * applied[0]) + (applied[2] * applied[2]));
  const double v2 = a1 * (applied[2] * applied[2]) + a2 * (applied[1] * applied[1]);
  double noisy[3];
  noisy[0] = applied[0] + chain_normal(seed, i, 0) * sqrt(v0);
  noisy[1] = applied[1] + chain_normal(seed, i, 1) * sqrt(v1);
  noisy[2] = applied[2] + chain_normal(seed, i, 2) * sqrt(v2);
  rec[6] = noisy[0]; rec[7] = noisy[1]; rec[8] = noisy[2];
  double next[3];
  pocs_motion(real, noisy, next);
  real[0] = next[0]; real[1] = next[1]; real[2] = next[2];
  // noisy range observations of the real state
  for (int l = 0; l < L; ++l) {
    const double dx = real[0] - c->sensor.lx[l], dy = real[1] - c->sensor.ly[l];
    const double dist = sqrt(dx * dx + dy * dy);
    rec[POCS_CHAIN_Z + l] = dist + (0.0 + chain_normal(seed, i, 3 + l) * sqrt(c->sensor.Q));
  }
  pocs_ekf_update(pmu, pcov, rec + POCS_CHAIN_Z, &c->sensor);
  memcpy(mu, pmu, 3 * sizeof(double));
  memcpy(cov, pcov, 9 * sizeof(double));
}

void compute_chain(pocs_ctx* c, uint64_t seed, const PlanView& pv) {
  const int W = pv.W;
  const double* traj = pv.traj;
  const double* odom = pv.odom;
  c->res.h_chain.assign((size_t)(W > 1 ? W - 1 : 1) * POCS_CHAIN_STRIDE, 0.0);
  c->res.h_mu.assign((size_t)(W > 1 ? W - 1 : 1) * 3, 0.0);
  c->res.h_cov.assign((size_t)(W > 1 ? W - 1 : 1) * 9, 0.0);
  double mu[3] = {traj[0], traj[W], traj[2 * W]};
  double cov[9];
  memcpy(cov, c->cov0, sizeof cov);
  double real[3] = {mu[0], mu[1], mu[2]};
  for (int i = 0; i < W - 1; ++i) {
    double* rec = &c->res.h_chain[(size_t)i * POCS_CHAIN_STRIDE];
    const double us[3] = {odom[i], odom[(W - 1) + i], odom[2 * (W - 1) + i]};
    const double xs[3] = {traj[i], traj[W + i], traj[2 * W + i]};
    const double xg[3] = {traj[i + 1], traj[W + i + 1], traj[2 * W + i + 1]};
    chain_step(c, seed, i, us, xs, xg, mu, cov, real, rec);
    memcpy(&c->res.h_mu[(size_t)i * 3], mu, sizeof mu);
    memcpy(&c->res.h_cov[(size_t)i * 9], cov, sizeof cov);
  }
}

PinLayout pin_layout(const pocs_ctx* c) {
  PinLayout p;
  const size_t W = (size_t)(c->W > 0 ? c->W : 1), K = (size_t)(c->K > 0 ? c->K : 1), R = (size_t)c->batch;
  p.chain = 2 * R;
  p.state0 = p.chain + R * (W > 1 ? W - 1 : 1) * POCS_CHAIN_STRIDE;
  p.runplan = p.state0 + R * K * POCS_STATE_STRIDE;
  p.moments = p.runplan + (c->plans.n ? 4 * R : 0);
  p.total = p.moments + W * R * K * POCS_NMOM;
  p.end = p.total + R + 2 + (R + 4) / 2 + 1;   // one u64 per run: MC totals; the call's give-up word and -- under a risk bound -- the R stop words behind it
  if (c->opt_mc_wp || c->opt_mc_rb || c->opt_obs_counts || seg_applied(c)) p.end += R * W + (R + 1) / 2;      // (mc_counts_active: the per-box counts bring the per-waypoint ones along)
  if (c->tree.n) p.end += R;                          // an MC call on a tree: [T] collided at or before the node, [T] first collisions   // MC calls with first collisions per waypoint: behind the totals, [R][W] u64 and the R stop words
  return p;
}

int ensure_pin(pocs_ctx* c) {
  const size_t bytes = pin_layout(c).end * sizeof(double);
  if (c->h_pin_cap >= bytes) return POCS_OK;
  if (c->h_pin) { HIPCHK(c, hipHostFree(c->h_pin)); c->h_pin = nullptr; c->h_pin_cap = 0; }
  HIPCHK(c, hipHostMalloc(&c->h_pin, bytes, hipHostMallocDefault));
  c->h_pin_cap = bytes;
  return POCS_OK;
}

uint64_t effective_seed(const pocs_ctx* c, uint64_t ahead = 0) {
  // every run of a context draws a fresh stream (the reference re-draws on each run*,
  // MCSimulator.h:656-679); setSeed rewinds run_index so (seed, run) is reproducible.
  return seed_of_run(c, c->run_index + ahead);
}

// A call of plans (pocs_set_plans): which plan each batch slot holds.  Slots in DESCENDING plan length (ties in plan
// order), so that the runs still live at any waypoint are a prefix of every sub-batch's slot range and the launch of
// waypoint w covers those only; with G sub-batches (gmm_groups) the plans of consecutive rank go to consecutive
// sub-batches, the larger ones first, so that all of them stay busy to the end.  Empty without plans.
std::vector<int> plan_layout(const pocs_ctx* c, int G) {
  std::vector<int> slot_plan;
  if (!c->plans.n) return slot_plan;
  const int R = c->plans.n;
  if (G < 1) G = 1;
  if (G > R) G = R;
  std::vector<int> rank(R);
  for (int p = 0; p < R; ++p) rank[p] = p;
  std::stable_sort(rank.begin(), rank.end(), [c](int x, int y) { return c->plans.W[(size_t)x] > c->plans.W[(size_t)y]; });
  std::vector<int> lo(G), n(G), fill(G, 0), order(G);
  for (int g = 0; g < G; ++g) {                      // sub-batch g = slots [g R / G, (g + 1) R / G), as enqueue_gmm_all cuts them
    lo[g] = (int)((long long)g * R / G);
    n[g] = (int)((long long)(g + 1) * R / G) - lo[g];
    order[g] = g;
  }
  std::stable_sort(order.begin(), order.end(), [&n](int x, int y) { return n[x] > n[y]; });
  slot_plan.assign(R, 0);
  for (int i = 0; i < R; ++i) {
    int k = i % G;
    while (fill[order[k]] == n[order[k]]) k = (k + 1) % G;
    const int g = order[k];
    slot_plan[(size_t)(lo[g] + fill[g]++)] = rank[i];
  }
  return slot_plan;
}
// the plan length of every slot of such a layout
std::vector<int> slot_lengths(const pocs_ctx* c, const std::vector<int>& slot_plan) {
  std::vector<int> Ws(slot_plan.size());
  for (size_t s = 0; s < slot_plan.size(); ++s) Ws[s] = c->plans.W[(size_t)slot_plan[s]];
  return Ws;
}
// runs of slots [lo, hi) whose plan is longer than w: a prefix of the range (plan_layout)
int live_runs(const std::vector<int>& Ws, int lo, int hi, int w) {
  int n = 0;
  while (lo + n < hi && Ws[(size_t)(lo + n)] > w) ++n;
  return n;
}
// The run number whose stream plan p draws, relative to the call's first: plan p draws run p's (the default), or --
// POCS_OPT_PLAN_SEEDS = 1, common random numbers -- every plan the call's first run's.
uint64_t plan_run(const pocs_ctx* c, int p) { return c->opt_plan_seeds ? 0 : (uint64_t)p; }

// The initial mixture of one run (initGMM, MCSimulator.h:350-352, GM_Model.h:57-77): K copies of (mu, cov0), weights 1 / K,
// all alive.  Nothing for K < 1 (an MC call of a context that was never given a K).
void write_initial_mixture(double* rows, const double mu[3], const double* cov0, int K) {
  for (int k = 0; k < K; ++k) {
    double* s = rows + (size_t)k * POCS_STATE_STRIDE;
    s[0] = mu[0]; s[1] = mu[1]; s[2] = mu[2];
    memcpy(s + 3, cov0, 9 * sizeof(double));
    s[12] = 1.0 / K; s[13] = 1.0; s[14] = 0.0; s[15] = 0.0;
  }
}

// Host image of one batch starting at run `base` (relative to c->run_index): per run the header
// (seed), the chain record and the initial mixture (initGMM, MCSimulator.h:350-352,
// GM_Model.h:57-77: K copies of (mu0, Sigma0), weights 1/K), laid out as the pinned staging area.
// A call of plans: slot r holds plan slot_plan[r] -- its own chain, start mean and seed (plan_run) -- and a row of
// start mean and steps.  Leaves slot 0's chain in c->res.h_chain / h_mu / h_cov.
// A tree of plans: every slot's header (ONE stream: the run `base`'s, as common random numbers give every plan of a call),
// the record of the edge into every node -- compute_chain unrolled over the tree: the main EKF's mu / cov and the real state
// travel from parent to child, a node of depth d is reached by step d - 1 and its normals -- and the root's initial mixture.
void build_tree_image(pocs_ctx* c, uint64_t base, double* img) {
  const PinLayout pl = pin_layout(c);
  const int T = c->tree.n;
  const uint64_t seed = effective_seed(c, base);
  std::vector<double> mu((size_t)T * 3), cov((size_t)T * 9), real((size_t)T * 3);
  for (int n = 0; n < T; ++n) {                       // (node order is topological: a parent comes before its children)
    const size_t slot = (size_t)c->tree.slot[(size_t)n];
    pocs_run_header hdr; hdr.seed = seed; hdr.pad = c->xchg_calls;
    memcpy(img + 2 * slot, &hdr, sizeof hdr);
    double* rec = img + pl.chain + slot * POCS_CHAIN_STRIDE;
    memset(rec, 0, POCS_CHAIN_STRIDE * sizeof(double));
    const double xg[3] = {c->tree.pose[(size_t)n], c->tree.pose[(size_t)T + n], c->tree.pose[2 * (size_t)T + n]};
    if (n == 0) {
      memcpy(&mu[0], xg, sizeof xg); memcpy(&real[0], xg, sizeof xg); memcpy(&cov[0], c->cov0, 9 * sizeof(double));
      continue;
    }
    const size_t p = (size_t)c->tree.parent[(size_t)n];
    const double xs[3] = {c->tree.pose[p], c->tree.pose[(size_t)T + p], c->tree.pose[2 * (size_t)T + p]};
    const double us[3] = {c->tree.odom[(size_t)n], c->tree.odom[(size_t)T + n], c->tree.odom[2 * (size_t)T + n]};
    memcpy(&mu[3 * (size_t)n], &mu[3 * p], 3 * sizeof(double));
    memcpy(&cov[9 * (size_t)n], &cov[9 * p], 9 * sizeof(double));
    memcpy(&real[3 * (size_t)n], &real[3 * p], 3 * sizeof(double));
    chain_step(c, seed, c->tree.depth[(size_t)n] - 1, us, xs, xg, &mu[3 * (size_t)n], &cov[9 * (size_t)n], &real[3 * (size_t)n], rec);
  }
  const double root[3] = {c->tree.pose[0], c->tree.pose[(size_t)T], c->tree.pose[2 * (size_t)T]};
  write_initial_mixture(img + pl.state0, root, c->cov0, c->K);      // the root's slot is 0
  c->res.h_chain.assign(POCS_CHAIN_STRIDE, 0.0); c->res.h_mu.assign(3, 0.0); c->res.h_cov.assign(9, 0.0);      // (the getters compute a path's chain when asked)
}

void build_run_image(pocs_ctx* c, uint64_t base, double* img, const std::vector<int>& slot_plan) {
  if (c->tree.n) { build_tree_image(c, base, img); return; }
  const PinLayout pl = pin_layout(c);
  const int W = c->W, R = c->batch;
  const size_t steps = (size_t)(W > 1 ? W - 1 : 1);
  for (int r = R - 1; r >= 0; --r) {          // run 0 last: c->res.h_chain / h_mu / h_cov keep ITS chain
    const int p = c->plans.n ? slot_plan[(size_t)r] : -1;
    const uint64_t seed = effective_seed(c, base + (p >= 0 ? plan_run(c, p) : (uint64_t)r));
    const PlanView pv = plan_view(c, p);
    compute_chain(c, seed, pv);
    pocs_run_header hdr; hdr.seed = seed; hdr.pad = c->xchg_calls;      // (sharded whole calls read their exchange epoch from here)
    memcpy(img + 2 * (size_t)r, &hdr, sizeof hdr);
    double* ch = img + pl.chain + (size_t)r * steps * POCS_CHAIN_STRIDE;
    memcpy(ch, c->res.h_chain.data(), c->res.h_chain.size() * sizeof(double));
    if (c->res.h_chain.size() < steps * POCS_CHAIN_STRIDE)                // (a shorter plan: records no kernel reads, zeroed)
      memset(ch + c->res.h_chain.size(), 0, (steps * POCS_CHAIN_STRIDE - c->res.h_chain.size()) * sizeof(double));
    const double start[3] = {pv.traj[0], pv.traj[pv.W], pv.traj[2 * pv.W]};
    write_initial_mixture(img + pl.state0 + (size_t)r * (c->K > 0 ? c->K : 0) * POCS_STATE_STRIDE, start, c->cov0, c->K);
    if (c->plans.n) {
      double* q = img + pl.runplan + 4 * (size_t)r;
      q[0] = start[0]; q[1] = start[1]; q[2] = start[2]; q[3] = (double)(pv.W - 1);
    }
  }
}

// While the GPU works on the current batch: the host chains of the next one (`groups`: the next call's sub-batches,
// which a call of plans lays its slots out by).
void prefetch_next_batch(pocs_ctx* c, int groups) {
  const PinLayout pl = pin_layout(c);
  auto& a = c->ahead;
  if (c->tree.n) { a.valid = false; return; }        // (a planner sets a new tree for its next call: nothing to look ahead to)
  std::vector<double> keep_chain = c->res.h_chain, keep_mu = c->res.h_mu, keep_cov = c->res.h_cov;
  a.image.resize(pl.moments);
  a.slot_plan = plan_layout(c, groups);
  build_run_image(c, 0, a.image.data(), a.slot_plan);       // c->run_index already points at the next batch
  a.chain0.swap(c->res.h_chain); a.mu0.swap(c->res.h_mu); a.cov0.swap(c->res.h_cov);
  c->res.h_chain.swap(keep_chain); c->res.h_mu.swap(keep_mu); c->res.h_cov.swap(keep_cov);
  a.seed = c->seed; a.run_index = c->run_index; a.R = c->batch; a.epoch = c->epoch;
  a.valid = true;
}

// Host image of this call's batch into the pinned staging area (from the look-ahead cache when it
// matches), run counter advanced; then the uploads every path needs: headers and chains (and, for a call of
// plans, the runs' start rows).  `groups`: the call's sub-batches; `kind`: the estimator whose plan layout it records.
int stage_and_upload_runs(pocs_ctx* c, int groups, Kind kind) {
  const PinLayout pl = pin_layout(c);
  double* pin = (double*)c->h_pin;
  const int W = c->W, R = c->batch;
  const size_t steps = (size_t)(W > 1 ? W - 1 : 1);
  const std::vector<int> slot_plan = plan_layout(c, groups);
  auto& a = c->ahead;
  if (a.valid && a.seed == c->seed && a.run_index == c->run_index && a.R == R && a.epoch == c->epoch &&
      a.image.size() == pl.moments && a.slot_plan == slot_plan) {
    memcpy(pin, a.image.data(), pl.moments * sizeof(double));
    c->res.h_chain = a.chain0; c->res.h_mu = a.mu0; c->res.h_cov = a.cov0;
  } else {
    build_run_image(c, 0, pin, slot_plan);
  }
  a.valid = false;
  for (int r = 0; r < R; ++r) ((uint64_t*)pin)[2 * (size_t)r + 1] = c->xchg_calls;      // (the image may have been built a call ago: the headers' exchange count is this call's)
  c->res.batch_base = c->run_index;
  c->res.batch_R = R;
  c->res.view = 0;
  c->run_index += (c->plans.n && c->opt_plan_seeds) || c->tree.n ? 1 : (uint64_t)R;      // (a tree: one stream for all its nodes)
  if (c->plans.n) {
    std::vector<int>& ps = c->res.plan_slot(kind);
    ps.assign((size_t)R, 0);
    for (int r = 0; r < R; ++r) ps[(size_t)slot_plan[(size_t)r]] = r;
    HIPCHK(c, hipMemcpyAsync(c->d_runplan.p, pin + pl.runplan, (size_t)R * 4 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipMemcpyAsync(c->d_hdr.p, pin, (size_t)R * sizeof(pocs_run_header), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_chain.p, pin + pl.chain, (size_t)R * steps * POCS_CHAIN_STRIDE * sizeof(double),
                           hipMemcpyHostToDevice, c->stream));
  return POCS_OK;
}

}  // namespace pocs_rt

// pocs_audit.hip -- looking into a context from outside the hot path: read-backs of device state for tests and audits
// (mixtures, samples, particles, the host chain, the obstacle counts), the bandwidth measurements, and the timing getters.  (The
// test hooks pocs_probe_device_* live in pocs_probe.hip.)
#include "pocs_ctx.hpp"

using namespace pocs_rt;

// The batch slot that holds the selected run's data in the device buffers: the run itself, or -- the last launch of that
// kind was a call of plans -- the selected plan's slot.
static size_t view_slot(const pocs_ctx* c, Kind kind) {
  const std::vector<int>& ps = c->res.plan_slot(kind);
  return (c->plans.n && (size_t)c->res.view < ps.size()) ? (size_t)ps[(size_t)c->res.view] : (size_t)c->res.view;
}

extern "C" {

// Device -> caller memory through the context's own pinned staging buffer, a piece at a time (the runtime
// would otherwise pin the caller's pageable pages on the fly for every call).
#define POCS_COPY_CHUNK (4u << 20)
static int copy_out(pocs_ctx* c, void* dst, const void* src_dev, size_t bytes, size_t elem, size_t dst_stride) {
#if defined(POCS_TUNING) && defined(POCS_PAGEABLE_GETTERS)      // diagnostic build: round 2's getters (the runtime pins the caller's pages per call)
  if (dst_stride == 0 || dst_stride == elem) { HIPCHK(c, hipMemcpy(dst, src_dev, bytes, hipMemcpyDeviceToHost)); return POCS_OK; }
#endif
  if (!c->h_copy) HIPCHK(c, hipHostMalloc(&c->h_copy, POCS_COPY_CHUNK, hipHostMallocDefault));
  for (size_t off = 0; off < bytes; off += POCS_COPY_CHUNK) {
    const size_t n = bytes - off < POCS_COPY_CHUNK ? bytes - off : POCS_COPY_CHUNK;
    HIPCHK(c, hipMemcpy(c->h_copy, (const char*)src_dev + off, n, hipMemcpyDeviceToHost));
    if (dst_stride == 0) memcpy((char*)dst + off, c->h_copy, n);
    else                                             // scatter elements of `elem` bytes `dst_stride` bytes apart
      for (size_t i = 0; i < n / elem; ++i) memcpy((char*)dst + (off / elem + i) * dst_stride, (const char*)c->h_copy + i * elem, elem);
  }
  return POCS_OK;
}
static long long copy_soa_as_aos(pocs_ctx* c, const DevBuf& bx, const DevBuf& by, const DevBuf& bt,
                                 size_t first, long long n, double* aos) {
  const DevBuf* src[3] = {&bx, &by, &bt};
  for (int j = 0; j < 3; ++j)
    if (copy_out(c, aos + j, (const double*)src[j]->p + first, (size_t)n * sizeof(double), sizeof(double), 3 * sizeof(double)) != POCS_OK) return -1;
  return n;
}

int pocs_get_gmm_state(pocs_ctx* c, int w, double* means3, double* covs9, double* weights, double* alive) {
  if (!c) return POCS_E_ARG;
  const size_t row = (size_t)c->K * POCS_STATE_STRIDE;
  const double* src = nullptr;                       // the mixture's K rows on the device
  if (c->tree.n) {                                   // the mixture of the selected node's ancestor of depth w
    if (tree_last(c) != Kind::Gmm || !c->d_state.p) return fail(c, POCS_E_ARG, "no mixture for waypoint %d: the last call was not a GMM call on the tree", w);
    const int depth = c->tree.depth[(size_t)c->res.tree_sel];
    if (w < 0 || w > depth) return fail(c, POCS_E_ARG, "no mixture for waypoint %d: node %d has depth %d", w, c->res.tree_sel, depth);
    int v = c->res.tree_sel;
    for (int d = depth; d > w; --d) v = c->tree.parent[(size_t)v];
    if (!c->res.tree_eval[(size_t)v]) return fail(c, POCS_E_ARG, "no mixture for waypoint %d: node %d lies below a node stopped by the risk bound", w, v);
    src = (double*)c->d_state.p + (size_t)c->tree.slot[(size_t)v] * row;
  } else {
    if (w < 0 || w > c->res.last_gmm_wp || !c->d_state.p) return fail(c, POCS_E_ARG, "no mixture for waypoint %d", w);
    if (c->plans.n && w >= pocs_get_path_length(c)) return fail(c, POCS_E_ARG, "no mixture for waypoint %d: plan %d has %d waypoints", w, c->res.view, pocs_get_path_length(c));
    if (c->plans.n && (size_t)c->res.view < c->res.plan_E.size() && w >= c->res.plan_E[(size_t)c->res.view])
      return fail(c, POCS_E_ARG, "no mixture for waypoint %d: plan %d was stopped by the risk bound after %d waypoints", w, c->res.view, c->res.plan_E[(size_t)c->res.view]);
    src = (double*)c->d_state.p + (view_slot(c, Kind::Gmm) * c->W + (size_t)w) * row;               // [run][W][K*16]
  }
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<double> s(row);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int r = copy_out(c, s.data(), src, row * sizeof(double), 1, 0)) return r;
  for (int k = 0; k < c->K; ++k) {
    if (means3) memcpy(means3 + 3 * k, &s[(size_t)k * POCS_STATE_STRIDE], 3 * sizeof(double));
    if (covs9) memcpy(covs9 + 9 * k, &s[(size_t)k * POCS_STATE_STRIDE + 3], 9 * sizeof(double));
    if (weights) weights[k] = s[(size_t)k * POCS_STATE_STRIDE + 12];
    if (alive) alive[k] = s[(size_t)k * POCS_STATE_STRIDE + 13];
  }
  return c->K;
}

int pocs_get_host_chain(pocs_ctx* c, double* applied3, double* noisy3, double* z, double* mu3, double* cov9) {
  if (!c) return POCS_E_ARG;
  const int steps = pocs_get_path_length(c) - 1, L = c->sensor.L;
  if (c->tree.n) {                                   // the chain of the path root -> the selected node, as a plan's
    if (tree_last(c) == Kind::None) return fail(c, POCS_E_STATE, "no run yet");
    const size_t W = (size_t)steps + 1, T = (size_t)c->tree.n;
    std::vector<double> traj(3 * W), odom(3 * (W > 1 ? W - 1 : 1));
    for (int v = c->res.tree_sel, w = steps; v >= 0; v = c->tree.parent[(size_t)v], --w)
      for (size_t j = 0; j < 3; ++j) {
        traj[j * W + (size_t)w] = c->tree.pose[j * T + (size_t)v];
        if (w > 0) odom[j * (W - 1) + (size_t)w - 1] = c->tree.odom[j * T + (size_t)v];
      }
    compute_chain(c, seed_of_run(c, c->res.batch_base), PlanView{traj.data(), odom.data(), (int)W});
  }
  if (c->plans.n) {                                   // the selected plan's chain (h_chain holds slot 0's)
    if (c->res.h_chain.empty()) return fail(c, POCS_E_STATE, "no run yet");
    compute_chain(c, seed_of_run(c, c->res.batch_base + plan_run(c, c->res.view)), plan_view(c, c->res.view));
  }
  if (steps < 0 || c->res.h_chain.size() < (size_t)(steps > 0 ? steps : 1) * POCS_CHAIN_STRIDE)
    return fail(c, POCS_E_STATE, "no run yet");
  if (c->res.view != 0 && !c->plans.n && !c->tree.n) compute_chain(c, seed_of_run(c, c->res.batch_base + (uint64_t)c->res.view), plan_view(c, -1));   // h_chain holds run 0's
  for (int i = 0; i < steps; ++i) {
    const double* rec = &c->res.h_chain[(size_t)i * POCS_CHAIN_STRIDE];
    if (applied3) memcpy(applied3 + 3 * i, rec, 3 * sizeof(double));
    if (noisy3) memcpy(noisy3 + 3 * i, rec + 6, 3 * sizeof(double));
    if (z) memcpy(z + (size_t)L * i, rec + POCS_CHAIN_Z, (size_t)L * sizeof(double));
    if (mu3) memcpy(mu3 + 3 * i, &c->res.h_mu[(size_t)3 * i], 3 * sizeof(double));
    if (cov9) memcpy(cov9 + 9 * i, &c->res.h_cov[(size_t)9 * i], 9 * sizeof(double));
  }
  return steps;
}

long long pocs_copy_gmm_samples(pocs_ctx* c, double* aos, int16_t* flags, long long cap) {
  if (!c) return POCS_E_ARG;
  const long long n = c->res.last_gmm_count;
  if (c->tree.n) return fail(c, POCS_E_STATE, "no stored samples: a call on a tree of plans stores none");
  if (!c->opt_store || !c->d_sx.p || c->res.last_gmm_wp < 0) return fail(c, POCS_E_STATE, "no stored samples");
  if (cap < n) return fail(c, POCS_E_BUFFER, "need room for %lld samples", n);
  if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
    return fail(c, POCS_E_DEVICE, "sync failed");
  const size_t off = view_slot(c, Kind::Gmm) * (size_t)sample_stride_of(n);          // this run's slice
  if (aos && copy_soa_as_aos(c, c->d_sx, c->d_sy, c->d_st, off, n, aos) < 0) return fail(c, POCS_E_DEVICE, "copy failed");
  if (flags && copy_out(c, flags, (const int16_t*)c->d_flags.p + off, (size_t)n * sizeof(int16_t), 1, 0) != POCS_OK)
    return fail(c, POCS_E_DEVICE, "copy failed");
  return n;
}

long long pocs_copy_particles(pocs_ctx* c, double* aos, uint32_t* hits, long long cap) {
  if (!c) return POCS_E_ARG;
  const long long n = c->res.last_mc_count;
  if (!c->d_px.p || n <= 0) return fail(c, POCS_E_STATE, "no particles");
  if (cap < n) return fail(c, POCS_E_BUFFER, "need room for %lld particles", n);
  if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
    return fail(c, POCS_E_DEVICE, "sync failed");
  size_t off = view_slot(c, Kind::Mc) * (size_t)sample_stride_of(n);                // this run's slice
  if (c->tree.n) {                                   // a tree: the last two levels' clouds are still there; the deepest level's are served
    const int D = (int)c->tree.level.size() - 2;
    if (tree_last(c) != Kind::Mc) return fail(c, POCS_E_STATE, "no particles: the last call was not an MC call on the tree");
    if (c->tree.depth[(size_t)c->res.tree_sel] != D)
      return fail(c, POCS_E_STATE, "particles of node %d (depth %d) are gone: an MC call on a tree keeps the clouds of its deepest level (%d)", c->res.tree_sel, c->tree.depth[(size_t)c->res.tree_sel], D);
    off = (size_t)(D & 1) * c->res.tree_mc_half + (size_t)(c->tree.slot[(size_t)c->res.tree_sel] - c->tree.level[(size_t)D]) * (size_t)sample_stride_of(n);
  }
  if (aos && copy_soa_as_aos(c, c->d_px, c->d_py, c->d_pt, off, n, aos) < 0) return fail(c, POCS_E_DEVICE, "copy failed");
  if (hits && copy_out(c, hits, (const uint32_t*)c->d_hits.p + off, (size_t)n * sizeof(uint32_t), 1, 0) != POCS_OK)
    return fail(c, POCS_E_DEVICE, "copy failed");
  return n;
}

// POCS_OPT_OBSTACLE_COUNTS: the table A[w][m] of the selected run, plan or tree path (include/pocs.h), read from the device's
// [slot][oc_W][POCS_MAX_OBSTACLES] array the last call filled: a run's or a plan's rows lie one behind the other, a path's one per
// node.  Row-major E x M, M = the boxes of the call's world.
int pocs_get_obstacle_counts(pocs_ctx* c, unsigned long long* out, int cap, int* boxes) {
  if (!c) return POCS_E_ARG;
  if (!out || !boxes) return fail(c, POCS_E_ARG, "pocs_get_obstacle_counts: null output");
  const Kind kind = c->res.oc_kind;
  if (kind == Kind::None || kind != c->res.last_kind || !c->d_obsct.p)
    return fail(c, POCS_E_STATE, "pocs_get_obstacle_counts: the last call ran without POCS_OPT_OBSTACLE_COUNTS (or there was none)");
  const size_t M = (size_t)c->res.oc_M, Wr = (size_t)c->res.oc_W, row = POCS_MAX_OBSTACLES;
  std::vector<size_t> rows;                          // the device rows ([slot * oc_W + w]) of the view's waypoints, in order
  if (c->tree.n) {
    if (tree_last(c) != kind) return fail(c, POCS_E_STATE, "pocs_get_obstacle_counts: the last call was not a call on the tree");
    for (int v = c->res.tree_sel; v >= 0; v = c->tree.parent[(size_t)v])
      if (kind == Kind::Mc || c->res.tree_eval[(size_t)v]) rows.push_back((size_t)c->tree.slot[(size_t)v]);      // (GMM under a bound: the evaluated part)
    std::reverse(rows.begin(), rows.end());
  } else {
    const size_t r = (size_t)c->res.view;
    int E = (int)Wr;                                   // a plan's own length, or the waypoints before its stop
    if (c->plans.n && r < c->res.plan_slot(kind).size()) {
      if (kind == Kind::Gmm) E = r < c->res.plan_E.size() ? c->res.plan_E[r] : c->plans.W[r];
      else E = c->res.plan_E_mc.empty() ? c->plans.W[r] : c->res.plan_E_mc[r];
    }
    if (r >= (size_t)c->res.batch_R && kind == Kind::Gmm) return fail(c, POCS_E_STATE, "pocs_get_obstacle_counts: no run %zu in the last call", r);
    const size_t slot = view_slot(c, kind);
    for (int w = 0; w < E; ++w) rows.push_back(slot * Wr + (size_t)w);
  }
  *boxes = (int)M;
  const size_t E = rows.size();
  if ((size_t)(cap < 0 ? 0 : cap) < E * M) return fail(c, POCS_E_BUFFER, "need %zu counters", E * M);
  if (M == 0 || E == 0) return (int)E;
  if ((rows.back() + 1) * row * sizeof(unsigned long long) > c->d_obsct.cap) return fail(c, POCS_E_STATE, "pocs_get_obstacle_counts: the table does not cover the selection");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<unsigned long long> h(E * row);
  const unsigned long long* dev = (const unsigned long long*)c->d_obsct.p;
  if (!c->tree.n) {                                  // one piece
    if (int r = copy_out(c, h.data(), dev + rows[0] * row, E * row * sizeof(unsigned long long), 1, 0)) return r;
  } else {
    for (size_t w = 0; w < E; ++w)
      if (int r = copy_out(c, &h[w * row], dev + rows[w] * row, row * sizeof(unsigned long long), 1, 0)) return r;
  }
  for (size_t w = 0; w < E; ++w) memcpy(out + w * M, &h[w * row], M * sizeof(unsigned long long));
  return (int)E;
}

// Measured streaming bandwidth of this GPU (GB/s), best of 5 timed with hipEvents on the context's stream: of a plain
// 16-B-per-lane copy of `bytes` (rounded down to 16; read + written bytes per second) -- the ceiling the streaming kernels are
// compared with next to the datasheet's 8 TB/s -- or, write-only, of a plain fill of `bytes` (bytes written per second).
static int measure_bandwidth(pocs_ctx* c, long long bytes, double* gbps, bool copy) {
  if (!c || !gbps) return POCS_E_ARG;
  if (bytes < 1024) return fail(c, POCS_E_ARG, copy ? "copy size too small" : "fill size too small");
  HIPCHK(c, hipSetDevice(c->device));
  bytes &= ~15LL;
  void *a = nullptr, *b = nullptr;
  HIPCHK(c, hipMalloc(&a, (size_t)bytes));
  if (copy && hipMalloc(&b, (size_t)bytes) != hipSuccess) { (void)hipFree(a); return fail(c, POCS_E_DEVICE, "hipMalloc failed"); }
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  if (copy) (void)hipMemsetAsync(a, 1, (size_t)bytes, c->stream);
  double best = 0.0;
  int rc = POCS_OK;
  for (int i = 0; i < 6 && rc == POCS_OK; ++i) {
    (void)hipEventRecord(e0, c->stream);
    if ((copy ? pocs_launch_copy(a, b, bytes, c->stream) : pocs_launch_fill(a, bytes, c->stream)) != hipSuccess) rc = fail(c, POCS_E_DEVICE, copy ? "copy launch failed" : "fill launch failed");
    (void)hipEventRecord(e1, c->stream);
    if (hipEventSynchronize(e1) != hipSuccess) rc = fail(c, POCS_E_DEVICE, copy ? "copy failed" : "fill failed");
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    if (i > 0 && ms > 0.f) { const double g = (copy ? 2.0 : 1.0) * (double)bytes / (ms * 1e-3) / 1e9; if (g > best) best = g; }
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  (void)hipFree(a);
  if (copy) (void)hipFree(b);
  *gbps = best;
  return rc;
}
int pocs_measure_copy_bandwidth(pocs_ctx* c, long long bytes, double* gbps) { return measure_bandwidth(c, bytes, gbps, true); }
int pocs_measure_fill_bandwidth(pocs_ctx* c, long long bytes, double* gbps) { return measure_bandwidth(c, bytes, gbps, false); }

int pocs_get_sequence_time(pocs_ctx* c, double* ms, int* concurrent) {
  if (!c) return POCS_E_ARG;
  if (ms) *ms = c->seq_ms;
  if (concurrent) *concurrent = c->seq_groups;
  return POCS_OK;
}

// Sharded GMM calls through the library's own exchange: how long the closers of the last begin..end sequence waited
// for the other ranks' moments, over its (run, waypoint) pairs: min, median, max in microseconds.
int pocs_get_exchange_wait(pocs_ctx* c, double* min_median_max_us) {
  if (!c || !min_median_max_us) return POCS_E_ARG;
  if (!c->sync.cells || !c->d_ticket.p) return fail(c, POCS_E_STATE, "no GMM call yet");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = c->sync.cells;                      // (the layout of the call that filled the block, whatever the setters have said since)
  std::vector<unsigned> v(n);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int r = copy_out(c, v.data(), (unsigned*)c->d_ticket.p + c->sync.xwait, n * sizeof(unsigned), sizeof(unsigned), sizeof(unsigned))) return r;
  std::sort(v.begin(), v.end());
  min_median_max_us[0] = 0.01 * v.front();
  min_median_max_us[1] = 0.01 * ((n & 1) ? v[n / 2] : 0.5 * ((double)v[n / 2 - 1] + (double)v[n / 2]));
  min_median_max_us[2] = 0.01 * v.back();
  return POCS_OK;
}

int pocs_get_graph_captures(pocs_ctx* c, long long* gmm, long long* mc) {      // captures of either graph since pocs_create
  if (!c) return POCS_E_ARG;
  if (gmm) *gmm = c->graph_gmm.captures;
  if (mc) *mc = c->graph_mc.captures;
  return POCS_OK;
}

int pocs_get_kernel_time(pocs_ctx* c, double* total_ms, long long* launches) {
  if (!c) return POCS_E_ARG;
  if (total_ms) *total_ms = c->prof_ms;
  if (launches) *launches = c->prof_launches;
  return POCS_OK;
}

}  // extern "C"

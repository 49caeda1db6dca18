// pocs_audit.hip -- looking into a context from outside the hot path: read-backs of device state for tests and audits
// (mixtures, samples, particles, the host chain), the bandwidth and device-math probes, and the timing getters.
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

// Test hook: the device's table-driven sampler functions on chosen inputs (include/pocs.h).
int pocs_probe_device_math(pocs_ctx* c, int n, const uint32_t* radius_words, const uint32_t* angle_words, const double* headings,
                           double* z0, double* z1, double* sn, double* cs, double* radius2) {
  if (!c || n < 1 || n > (1 << 20) || !radius_words || !angle_words || !headings || !z0 || !z1 || !sn || !cs || !radius2) return c ? fail(c, POCS_E_ARG, "pocs_probe_device_math: 1 <= n <= 2^20, no null pointers") : POCS_E_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (int r = upload_tables(c)) return r;
  const size_t nw = (size_t)n * sizeof(uint32_t), nd = (size_t)n * sizeof(double);
  char* buf = nullptr;                         // [wr | wa | x | out 5 n]
  HIPCHK(c, hipMalloc((void**)&buf, 2 * nw + 6 * nd + 64));
  uint32_t* d_wr = (uint32_t*)buf;
  uint32_t* d_wa = d_wr + n;
  double* d_x = (double*)(buf + ((2 * nw + 15) & ~(size_t)15));
  double* d_out = d_x + n;
  int rc = POCS_OK;
  if (hipMemcpy(d_wr, radius_words, nw, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_wa, angle_words, nw, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_x, headings, nd, hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe upload failed");
  if (rc == POCS_OK && pocs_launch_probe_math((const pocs_tables*)c->d_tables.p, n, d_wr, d_wa, d_x, d_out, c->stream) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe launch failed");
  if (rc == POCS_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, POCS_E_DEVICE, "probe kernel failed");
  double* dst[5] = {z0, z1, sn, cs, radius2};
  for (int j = 0; j < 5 && rc == POCS_OK; ++j)
    if (hipMemcpy(dst[j], d_out + (size_t)j * n, nd, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(c, POCS_E_DEVICE, "probe download failed");
  (void)hipFree(buf);
  return rc;
}

// Test hook: the two square roots of the Box-Muller radius on a range of words (include/pocs.h).
int pocs_probe_device_radius_roots(pocs_ctx* c, uint32_t first_word, unsigned long long count, unsigned long long* mismatches, uint32_t* first_bad) {
  if (!c) return POCS_E_ARG;
  if (!mismatches || !first_bad || count < 1 || (unsigned long long)first_word + count > (1ull << 32))
    return fail(c, POCS_E_ARG, "pocs_probe_device_radius_roots: count >= 1, first_word + count <= 2^32, no null pointers");
  HIPCHK(c, hipSetDevice(c->device));
  if (int r = upload_tables(c)) return r;
  unsigned long long* d_out = nullptr;               // [mismatches | smallest mismatching word]
  HIPCHK(c, hipMalloc((void**)&d_out, 2 * sizeof(unsigned long long)));
  unsigned long long h[2] = {0ull, ~0ull};
  int rc = POCS_OK;
  if (hipMemcpy(d_out, h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) rc = fail(c, POCS_E_DEVICE, "probe upload failed");
  if (rc == POCS_OK && pocs_launch_probe_radius_roots((const pocs_tables*)c->d_tables.p, first_word, count, d_out, c->stream) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe launch failed");
  if (rc == POCS_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, POCS_E_DEVICE, "probe kernel failed");
  if (rc == POCS_OK && hipMemcpy(h, d_out, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(c, POCS_E_DEVICE, "probe download failed");
  (void)hipFree(d_out);
  if (rc != POCS_OK) return rc;
  *mismatches = h[0];
  *first_bad = h[0] ? (uint32_t)h[1] : 0u;
  return POCS_OK;
}

// Test hook: the device's collision test and obstacle cull on chosen poses and a chosen mixture (include/pocs.h).
int pocs_probe_device_collide(pocs_ctx* c, int K, const double* params, int n, const double* poses, int* flag_full, int* flag_pair,
                              int* flag_pair_eager, int* nkeep, double* kept) {
  if (!c) return POCS_E_ARG;
  if (!params || !poses || !flag_full || !flag_pair || !flag_pair_eager || !nkeep || !kept || n < 1 || n > (1 << 20) || K < 1 || K > POCS_MAX_GAUSSIANS)
    return fail(c, POCS_E_ARG, "pocs_probe_device_collide: 1 <= n <= 2^20, 1 <= K <= %d, no null pointers", POCS_MAX_GAUSSIANS);
  if (!c->have_obstacles)
    return fail(c, POCS_E_STATE, "no collision world: pocs_set_obstacles / addObstacle / clearObstacles missing");
  if (int r = may_enter(c, "pocs_probe_device_collide", pocs_modes::kProbe)) return r;
  if (discs_applied(c))                              // (this probe's three forms test boxes: a world with discs is probed by pocs_probe_device_discs)
    return fail(c, POCS_E_STATE, "pocs_probe_device_collide: discs are set (pocs_set_discs); the probe tests boxes only, pocs_probe_device_discs probes a world with discs");
  // (a heading that is not a number has no sector: nothing of the kind reaches the device)
  const size_t PS = (size_t)K * POCS_PARAM_STRIDE;
  for (size_t j = 0; j < PS; ++j)
    if (!std::isfinite(params[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_collide: parameter %zu is not finite", j);
  for (size_t j = 0; j < 3 * (size_t)n; ++j)
    if (!std::isfinite(poses[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_collide: pose %zu is not finite", j / 3);
  HIPCHK(c, hipSetDevice(c->device));
  if (int r = upload_world(c)) return r;
  // [par | x | y | th | kept] doubles, then [flags 3 n | nkeep] ints
  const size_t nrec = (size_t)POCS_MAX_OBSTACLES * POCS_OBS_STRIDE, nd = PS + 3 * (size_t)n + nrec, ni = 3 * (size_t)n + 1;
  std::vector<double> h(nd, 0.0);
  memcpy(h.data(), params, PS * sizeof(double));
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 3; ++j) h[PS + (size_t)j * n + i] = poses[3 * (size_t)i + j];
  char* buf = nullptr;
  HIPCHK(c, hipMalloc((void**)&buf, nd * sizeof(double) + ni * sizeof(int)));
  double* d_par = (double*)buf;
  double *d_x = d_par + PS, *d_kept = d_x + 3 * (size_t)n;
  int* d_flags = (int*)(d_kept + nrec);
  pocs_gmm_launch a;
  memset(&a, 0, sizeof a);
  fill_gmm_world(c, &a, 0);                         // (under an obstacle schedule: world 0)
  a.param = d_par; a.W = 1; a.nruns = 1; a.run_cnt = 1;
  std::vector<int> f(ni, 0);
  int rc = POCS_OK;
  if (hipMemcpy(buf, h.data(), nd * sizeof(double), hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_flags, 0, ni * sizeof(int)) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe upload failed");
  if (rc == POCS_OK && pocs_launch_probe_collide(K, a, n, d_x, d_x + n, d_x + 2 * (size_t)n, d_flags, d_flags + 3 * (size_t)n, d_kept, c->stream) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe launch failed");
  if (rc == POCS_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, POCS_E_DEVICE, "probe kernel failed");
  if (rc == POCS_OK && (hipMemcpy(f.data(), d_flags, ni * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
                        hipMemcpy(kept, d_kept, nrec * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
    rc = fail(c, POCS_E_DEVICE, "probe download failed");
  (void)hipFree(buf);
  if (rc != POCS_OK) return rc;
  memcpy(flag_full, f.data(), (size_t)n * sizeof(int));
  memcpy(flag_pair, f.data() + n, (size_t)n * sizeof(int));
  memcpy(flag_pair_eager, f.data() + 2 * (size_t)n, (size_t)n * sizeof(int));
  *nkeep = f[3 * (size_t)n];
  return POCS_OK;
}

// Test hook: the device's clearance level on chosen poses, footprint, distances and boxes (include/pocs.h).  Nothing of the context's
// world, plans or modes is read: the two tables are prepared here, as upload_world prepares the context's.
int pocs_probe_device_clearance(pocs_ctx* c, const double* fp4, const double* d, int L, const double* boxes, int M, int n,
                                const double* poses, int* level_out) {
  if (!c) return POCS_E_ARG;
  if (!fp4 || !poses || !level_out || n < 1 || n > (1 << 20) || L < 0 || L > POCS_MAX_CLEARANCE_LEVELS || (L > 0 && !d) || M < 0 || M > POCS_MAX_OBSTACLES || (M > 0 && !boxes))
    return fail(c, POCS_E_ARG, "pocs_probe_device_clearance: 1 <= n <= 2^20, 0 <= L <= %d, 0 <= M <= %d, no null pointers", POCS_MAX_CLEARANCE_LEVELS, POCS_MAX_OBSTACLES);
  for (int j = 0; j < 4; ++j)
    if (!std::isfinite(fp4[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_clearance: footprint value %d is not finite", j);
  if (!(fp4[2] > 0) || !(fp4[3] > 0)) return fail(c, POCS_E_ARG, "pocs_probe_device_clearance: footprint half extents must be > 0");
  for (int l = 0; l < L; ++l)
    if (!std::isfinite(d[l]) || !(d[l] > (l ? d[l - 1] : 0.0)))
      return fail(c, POCS_E_ARG, "pocs_probe_device_clearance: distance %d: finite distances with 0 < d[0] < d[1] < ... are needed", l);
  for (size_t j = 0; j < 5 * (size_t)M; ++j)
    if (!std::isfinite(boxes[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_clearance: box %zu: value %zu is not finite", j / 5, j % 5);
  for (int m = 0; m < M; ++m)
    if (!(boxes[5 * (size_t)m + 2] > 0) || !(boxes[5 * (size_t)m + 3] > 0)) return fail(c, POCS_E_ARG, "pocs_probe_device_clearance: box %d: half extents must be > 0", m);
  for (size_t j = 0; j < 3 * (size_t)n; ++j)
    if (!std::isfinite(poses[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_clearance: pose %zu is not finite", j / 3);
  HIPCHK(c, hipSetDevice(c->device));
  if (int r = upload_tables(c)) return r;
  const pocs_footprint fp = {fp4[0], fp4[1], fp4[2], fp4[3]};
  std::vector<pocs_env_dev> env(1);
  std::vector<pocs_clear_dev> clr(1);
  memset(env.data(), 0, sizeof(pocs_env_dev));
  env[0].fp = fp; env[0].M = M;
  for (int m = 0; m < M; ++m) pocs_prepare_obstacle(boxes + 5 * (size_t)m, &fp, &env[0].obs[(size_t)m * POCS_OBS_STRIDE]);
  prepare_clearance(fp, d, L, boxes, M, clr.data());
  std::vector<double> h(3 * (size_t)n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 3; ++j) h[(size_t)j * n + i] = poses[3 * (size_t)i + j];
  // [env | clr | x | y | th] then [levels n] ints
  const size_t off_clr = sizeof(pocs_env_dev), off_x = off_clr + sizeof(pocs_clear_dev), off_out = off_x + 3 * (size_t)n * sizeof(double);
  static_assert(sizeof(pocs_env_dev) % 8 == 0 && sizeof(pocs_clear_dev) % 8 == 0, "the probe's buffer keeps its parts aligned");
  char* buf = nullptr;
  HIPCHK(c, hipMalloc((void**)&buf, off_out + (size_t)n * sizeof(int)));
  int rc = POCS_OK;
  if (hipMemcpy(buf, env.data(), sizeof(pocs_env_dev), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(buf + off_clr, clr.data(), sizeof(pocs_clear_dev), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(buf + off_x, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(buf + off_out, 0, (size_t)n * sizeof(int)) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe upload failed");
  const double* d_x = (const double*)(buf + off_x);
  if (rc == POCS_OK && pocs_launch_probe_clearance((const pocs_env_dev*)buf, (const pocs_clear_dev*)(buf + off_clr), L, (const pocs_tables*)c->d_tables.p, n,
                                                   d_x, d_x + n, d_x + 2 * (size_t)n, (int*)(buf + off_out), c->stream) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe launch failed");
  if (rc == POCS_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, POCS_E_DEVICE, "probe kernel failed");
  if (rc == POCS_OK && hipMemcpy(level_out, buf + off_out, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe download failed");
  (void)hipFree(buf);
  return rc;
}

// Test hook: which parts of a compound footprint touch, on the device, for chosen poses, parts and boxes (include/pocs.h).  Nothing of
// the context's world, plans or modes is read: the records and the parts are prepared here, as upload_world prepares the context's.
int pocs_probe_device_footprint_parts(pocs_ctx* c, const double* parts, int F, const double* boxes, int M, int n,
                                      const double* poses, int* touched_out) {
  if (!c) return POCS_E_ARG;
  if (!parts || !poses || !touched_out || n < 1 || n > (1 << 20) || F < 1 || F > POCS_MAX_FOOTPRINT_PARTS || M < 0 || M > POCS_MAX_OBSTACLES || (M > 0 && !boxes))
    return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_parts: 1 <= n <= 2^20, 1 <= F <= %d, 0 <= M <= %d, no null pointers", POCS_MAX_FOOTPRINT_PARTS, POCS_MAX_OBSTACLES);
  for (int j = 0; j < 4 * F; ++j)
    if (!std::isfinite(parts[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_parts: part %d: value %d is not finite", j / 4, j % 4);
  for (int f = 0; f < F; ++f)
    if (!(parts[4 * f + 2] > 0) || !(parts[4 * f + 3] > 0)) return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_parts: part %d: half extents must be > 0", f);
  for (size_t j = 0; j < 5 * (size_t)M; ++j)
    if (!std::isfinite(boxes[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_parts: box %zu: value %zu is not finite", j / 5, j % 5);
  for (int m = 0; m < M; ++m)
    if (!(boxes[5 * (size_t)m + 2] > 0) || !(boxes[5 * (size_t)m + 3] > 0)) return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_parts: box %d: half extents must be > 0", m);
  for (size_t j = 0; j < 3 * (size_t)n; ++j)
    if (!std::isfinite(poses[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_parts: pose %zu is not finite", j / 3);
  HIPCHK(c, hipSetDevice(c->device));
  if (int r = upload_tables(c)) return r;
  pocs_footprint fps[POCS_MAX_FOOTPRINT_PARTS];
  for (int f = 0; f < F; ++f) fps[f] = pocs_footprint{parts[4 * f], parts[4 * f + 1], parts[4 * f + 2], parts[4 * f + 3]};
  std::vector<pocs_env_dev> env(1);
  pocs_parts_dev pd;
  prepare_parts(fps, F, boxes, M, env.data(), &pd);
  std::vector<double> h(3 * (size_t)n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 3; ++j) h[(size_t)j * n + i] = poses[3 * (size_t)i + j];
  // [env | parts | x | y | th] then [touched n] ints
  const size_t off_parts = sizeof(pocs_env_dev), off_x = off_parts + sizeof(pocs_parts_dev), off_out = off_x + 3 * (size_t)n * sizeof(double);
  static_assert(sizeof(pocs_env_dev) % 8 == 0 && sizeof(pocs_parts_dev) % 8 == 0, "the probe's buffer keeps its parts aligned");
  char* buf = nullptr;
  HIPCHK(c, hipMalloc((void**)&buf, off_out + (size_t)n * sizeof(int)));
  int rc = POCS_OK;
  if (hipMemcpy(buf, env.data(), sizeof(pocs_env_dev), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(buf + off_parts, &pd, sizeof(pocs_parts_dev), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(buf + off_x, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(buf + off_out, 0, (size_t)n * sizeof(int)) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe upload failed");
  const double* d_x = (const double*)(buf + off_x);
  if (rc == POCS_OK && pocs_launch_probe_parts((const pocs_env_dev*)buf, (const pocs_parts_dev*)(buf + off_parts), F, (const pocs_tables*)c->d_tables.p, n,
                                               d_x, d_x + n, d_x + 2 * (size_t)n, (int*)(buf + off_out), c->stream) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe launch failed");
  if (rc == POCS_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, POCS_E_DEVICE, "probe kernel failed");
  if (rc == POCS_OK && hipMemcpy(touched_out, buf + off_out, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe download failed");
  (void)hipFree(buf);
  return rc;
}

// Test hook: which watched regions the device finds chosen poses in, for a footprint and regions of the caller's own
// (include/pocs.h).  Nothing of the context's world, plans, modes or regions is read: the record is prepared here, as upload_world
// prepares the context's.
int pocs_probe_device_regions(pocs_ctx* c, const double* fp4, const double* boxes, const int* kinds, int G, int n,
                              const double* poses, int* mask_out) {
  if (!c) return POCS_E_ARG;
  if (!fp4 || !poses || !mask_out || n < 1 || n > (1 << 20) || G < 0 || G > POCS_MAX_REGIONS || (G > 0 && (!boxes || !kinds)))
    return fail(c, POCS_E_ARG, "pocs_probe_device_regions: 1 <= n <= 2^20, 0 <= G <= %d, no null pointers", POCS_MAX_REGIONS);
  for (int j = 0; j < 4; ++j)
    if (!std::isfinite(fp4[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_regions: footprint value %d is not finite", j);
  if (!(fp4[2] > 0) || !(fp4[3] > 0)) return fail(c, POCS_E_ARG, "pocs_probe_device_regions: footprint half extents must be > 0");
  for (size_t j = 0; j < 5 * (size_t)G; ++j)
    if (!std::isfinite(boxes[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_regions: region %zu: value %zu is not finite", j / 5, j % 5);
  for (int g = 0; g < G; ++g) {
    if (!(boxes[5 * (size_t)g + 2] > 0) || !(boxes[5 * (size_t)g + 3] > 0)) return fail(c, POCS_E_ARG, "pocs_probe_device_regions: region %d: half extents must be > 0", g);
    if (kinds[g] != POCS_REGION_TOUCH && kinds[g] != POCS_REGION_POINT) return fail(c, POCS_E_ARG, "pocs_probe_device_regions: region %d: kind %d", g, kinds[g]);
  }
  for (size_t j = 0; j < 3 * (size_t)n; ++j)
    if (!std::isfinite(poses[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_regions: pose %zu is not finite", j / 3);
  HIPCHK(c, hipSetDevice(c->device));
  if (int r = upload_tables(c)) return r;
  const pocs_footprint fp = {fp4[0], fp4[1], fp4[2], fp4[3]};
  pocs_regions_dev reg;
  prepare_regions(fp, boxes, kinds, G, &reg);
  std::vector<double> h(3 * (size_t)n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 3; ++j) h[(size_t)j * n + i] = poses[3 * (size_t)i + j];
  // [regions | x | y | th] then [masks n] ints
  const size_t off_x = sizeof(pocs_regions_dev), off_out = off_x + 3 * (size_t)n * sizeof(double);
  static_assert(sizeof(pocs_regions_dev) % 8 == 0, "the probe's buffer keeps its parts aligned");
  char* buf = nullptr;
  HIPCHK(c, hipMalloc((void**)&buf, off_out + (size_t)n * sizeof(int)));
  int rc = POCS_OK;
  if (hipMemcpy(buf, &reg, sizeof reg, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(buf + off_x, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(buf + off_out, 0, (size_t)n * sizeof(int)) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe upload failed");
  const double* d_x = (const double*)(buf + off_x);
  if (rc == POCS_OK && pocs_launch_probe_regions((const pocs_regions_dev*)buf, G, (const pocs_tables*)c->d_tables.p, n,
                                                 d_x, d_x + n, d_x + 2 * (size_t)n, (int*)(buf + off_out), c->stream) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe launch failed");
  if (rc == POCS_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, POCS_E_DEVICE, "probe kernel failed");
  if (rc == POCS_OK && hipMemcpy(mask_out, buf + off_out, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe download failed");
  (void)hipFree(buf);
  return rc;
}

// Test hook: which sub-poses of a segment touch, on the device, for chosen poses, footprint, boxes, control and J (include/pocs.h).
// Nothing of the context's world, plans or modes is read: the records and the segment record are prepared here, as upload_world
// prepares the context's.
int pocs_probe_device_segment(pocs_ctx* c, const double* fp4, const double* boxes, int M, const double* u3, int J, int backward, int n,
                              const double* poses, int* mask_out) {
  if (!c) return POCS_E_ARG;
  if (!fp4 || !u3 || !poses || !mask_out || n < 1 || n > (1 << 20) || J < 1 || J > POCS_MAX_SEGMENT_CHECKS || M < 0 || M > POCS_MAX_OBSTACLES ||
      (M > 0 && !boxes) || (backward != 0 && backward != 1))
    return fail(c, POCS_E_ARG, "pocs_probe_device_segment: 1 <= n <= 2^20, 1 <= J <= %d, 0 <= M <= %d, backward 0 or 1, no null pointers", POCS_MAX_SEGMENT_CHECKS, POCS_MAX_OBSTACLES);
  for (int j = 0; j < 4; ++j)
    if (!std::isfinite(fp4[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_segment: footprint value %d is not finite", j);
  if (!(fp4[2] > 0) || !(fp4[3] > 0)) return fail(c, POCS_E_ARG, "pocs_probe_device_segment: footprint half extents must be > 0");
  for (int j = 0; j < 3; ++j)
    if (!std::isfinite(u3[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_segment: control value %d is not finite", j);
  for (size_t j = 0; j < 5 * (size_t)M; ++j)
    if (!std::isfinite(boxes[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_segment: box %zu: value %zu is not finite", j / 5, j % 5);
  for (int m = 0; m < M; ++m)
    if (!(boxes[5 * (size_t)m + 2] > 0) || !(boxes[5 * (size_t)m + 3] > 0)) return fail(c, POCS_E_ARG, "pocs_probe_device_segment: box %d: half extents must be > 0", m);
  for (size_t j = 0; j < 3 * (size_t)n; ++j)
    if (!std::isfinite(poses[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_segment: pose %zu is not finite", j / 3);
  HIPCHK(c, hipSetDevice(c->device));
  if (int r = upload_tables(c)) return r;
  const pocs_footprint fp = {fp4[0], fp4[1], fp4[2], fp4[3]};
  std::vector<pocs_env_dev> env(1);
  memset(env.data(), 0, sizeof(pocs_env_dev));
  env[0].fp = fp; env[0].M = M;
  for (int m = 0; m < M; ++m) pocs_prepare_obstacle(boxes + (size_t)m * 5, &fp, &env[0].obs[(size_t)m * POCS_OBS_STRIDE]);
  pocs_seg_dev sg;
  prepare_segment(J, &sg);
  std::vector<double> h(3 * (size_t)n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 3; ++j) h[(size_t)j * n + i] = poses[3 * (size_t)i + j];
  // [env | seg | x | y | th] then [masks n] ints
  const size_t off_seg = sizeof(pocs_env_dev), off_x = off_seg + sizeof(pocs_seg_dev), off_out = off_x + 3 * (size_t)n * sizeof(double);
  static_assert(sizeof(pocs_env_dev) % 8 == 0 && sizeof(pocs_seg_dev) % 8 == 0, "the probe's buffer keeps its parts aligned");
  char* buf = nullptr;
  HIPCHK(c, hipMalloc((void**)&buf, off_out + (size_t)n * sizeof(int)));
  int rc = POCS_OK;
  if (hipMemcpy(buf, env.data(), sizeof(pocs_env_dev), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(buf + off_seg, &sg, sizeof sg, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(buf + off_x, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(buf + off_out, 0, (size_t)n * sizeof(int)) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe upload failed");
  const double* d_x = (const double*)(buf + off_x);
  if (rc == POCS_OK && pocs_launch_probe_segment((const pocs_env_dev*)buf, (const pocs_seg_dev*)(buf + off_seg), (const pocs_tables*)c->d_tables.p,
                                                 u3[0], u3[1], u3[2], backward, n, d_x, d_x + n, d_x + 2 * (size_t)n, (int*)(buf + off_out),
                                                 c->stream) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe launch failed");
  if (rc == POCS_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, POCS_E_DEVICE, "probe kernel failed");
  if (rc == POCS_OK && hipMemcpy(mask_out, buf + off_out, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe download failed");
  (void)hipFree(buf);
  return rc;
}

// Test hook: the device's component counts on chosen weights, alive flags, seeds, waypoints and sample totals (include/pocs.h).
// Nothing of the context's world, plans or modes is read.
int pocs_probe_device_counts(pocs_ctx* c, int n, const int* K, const double* weights, const double* alive, const uint64_t* seeds,
                             const uint32_t* waypoints, const long long* n_total, double* counts_out) {
  if (!c) return POCS_E_ARG;
  if (!K || !weights || !alive || !seeds || !waypoints || !n_total || !counts_out || n < 1 || n > (1 << 20))
    return fail(c, POCS_E_ARG, "pocs_probe_device_counts: 1 <= n <= 2^20, no null pointers");
  constexpr size_t KM = POCS_MAX_GAUSSIANS;
  for (int i = 0; i < n; ++i) {
    if (K[i] < 1 || K[i] > POCS_MAX_GAUSSIANS) return fail(c, POCS_E_ARG, "pocs_probe_device_counts: case %d: 1 <= K <= %d", i, POCS_MAX_GAUSSIANS);
    if (n_total[i] < 1 || n_total[i] > (1LL << 53)) return fail(c, POCS_E_ARG, "pocs_probe_device_counts: case %d: 1 <= n_total <= 2^53", i);
    for (int k = 0; k < K[i]; ++k) {
      const double w = weights[(size_t)i * KM + k], a = alive[(size_t)i * KM + k];
      if (!std::isfinite(w) || w < 0.0) return fail(c, POCS_E_ARG, "pocs_probe_device_counts: case %d: weight %d is not a finite number >= 0", i, k);
      if (!std::isfinite(a)) return fail(c, POCS_E_ARG, "pocs_probe_device_counts: case %d: alive flag %d is not finite", i, k);
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  // [w | alive] n x KM doubles each, [n_total] n doubles, [out] n x KM doubles, [seeds] n 64-bit words, [waypoints | K] n 32-bit words each
  const size_t nk = (size_t)n * KM;
  std::vector<double> h(2 * nk + (size_t)n, 0.0);
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < K[i]; ++k) {                       // (what lies behind a case's K is not read, here or on the device)
      h[(size_t)i * KM + k] = weights[(size_t)i * KM + k];
      h[nk + (size_t)i * KM + k] = alive[(size_t)i * KM + k];
    }
    h[2 * nk + (size_t)i] = (double)n_total[i];
  }
  const size_t off_out = h.size() * sizeof(double), off_seed = off_out + nk * sizeof(double), off_wp = off_seed + (size_t)n * sizeof(uint64_t),
               off_k = off_wp + (size_t)n * sizeof(uint32_t);
  char* buf = nullptr;
  HIPCHK(c, hipMalloc((void**)&buf, off_k + (size_t)n * sizeof(int)));
  int rc = POCS_OK;
  if (hipMemcpy(buf, h.data(), off_out, hipMemcpyHostToDevice) != hipSuccess || hipMemset(buf + off_out, 0, nk * sizeof(double)) != hipSuccess ||
      hipMemcpy(buf + off_seed, seeds, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(buf + off_wp, waypoints, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(buf + off_k, K, (size_t)n * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe upload failed");
  const double* d_w = (const double*)buf;
  if (rc == POCS_OK && pocs_launch_probe_counts(n, (const int*)(buf + off_k), d_w, d_w + nk, (const unsigned long long*)(buf + off_seed),
                                                (const uint32_t*)(buf + off_wp), d_w + 2 * nk, (double*)(buf + off_out), c->stream) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe launch failed");
  if (rc == POCS_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, POCS_E_DEVICE, "probe kernel failed");
  if (rc == POCS_OK && hipMemcpy(counts_out, buf + off_out, nk * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe download failed");
  (void)hipFree(buf);
  return rc;
}

// Test hook: which kinds of obstacle a pose touches, on the device, for chosen poses, footprint, boxes and discs (include/pocs.h).
// Nothing of the context's world, plans or modes is read: the composed record (boxes, then discs) is prepared here, as upload_world
// prepares the context's.
int pocs_probe_device_discs(pocs_ctx* c, const double* fp4, const double* boxes, int M, const double* discs, int D, int n,
                            const double* poses, int* out) {
  if (!c) return POCS_E_ARG;
  if (!fp4 || !poses || !out || n < 1 || n > (1 << 20) || M < 0 || D < 0 || M + D > POCS_MAX_OBSTACLES || (M > 0 && !boxes) || (D > 0 && !discs))
    return fail(c, POCS_E_ARG, "pocs_probe_device_discs: 1 <= n <= 2^20, 0 <= M, 0 <= D, M + D <= %d, no null pointers", POCS_MAX_OBSTACLES);
  for (int j = 0; j < 4; ++j)
    if (!std::isfinite(fp4[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_discs: footprint value %d is not finite", j);
  if (!(fp4[2] > 0) || !(fp4[3] > 0)) return fail(c, POCS_E_ARG, "pocs_probe_device_discs: footprint half extents must be > 0");
  for (size_t j = 0; j < 5 * (size_t)M; ++j)
    if (!std::isfinite(boxes[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_discs: box %zu: value %zu is not finite", j / 5, j % 5);
  for (int m = 0; m < M; ++m)
    if (!(boxes[5 * (size_t)m + 2] > 0) || !(boxes[5 * (size_t)m + 3] > 0)) return fail(c, POCS_E_ARG, "pocs_probe_device_discs: box %d: half extents must be > 0", m);
  for (size_t j = 0; j < 3 * (size_t)D; ++j)
    if (!std::isfinite(discs[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_discs: disc %zu: value %zu is not finite", j / 3, j % 3);
  for (int d = 0; d < D; ++d)
    if (!(discs[3 * (size_t)d + 2] > 0)) return fail(c, POCS_E_ARG, "pocs_probe_device_discs: disc %d: the radius must be > 0", d);
  for (size_t j = 0; j < 3 * (size_t)n; ++j)
    if (!std::isfinite(poses[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_discs: pose %zu is not finite", j / 3);
  HIPCHK(c, hipSetDevice(c->device));
  if (int r = upload_tables(c)) return r;
  const pocs_footprint fp = {fp4[0], fp4[1], fp4[2], fp4[3]};
  std::vector<pocs_env_dev> env(1);
  memset(env.data(), 0, sizeof(pocs_env_dev));
  env[0].fp = fp; env[0].M = M + D;
  for (int m = 0; m < M; ++m) pocs_prepare_box_beside_discs(boxes + (size_t)m * 5, &fp, &env[0].obs[(size_t)m * POCS_OBS_STRIDE]);
  for (int d = 0; d < D; ++d) pocs_prepare_disc(discs + (size_t)d * 3, &fp, &env[0].obs[(size_t)(M + d) * POCS_OBS_STRIDE]);
  std::vector<double> h(3 * (size_t)n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 3; ++j) h[(size_t)j * n + i] = poses[3 * (size_t)i + j];
  // [env | x | y | th] then [out n] ints
  const size_t off_x = sizeof(pocs_env_dev), off_out = off_x + 3 * (size_t)n * sizeof(double);
  static_assert(sizeof(pocs_env_dev) % 8 == 0, "the probe's buffer keeps its parts aligned");
  char* buf = nullptr;
  HIPCHK(c, hipMalloc((void**)&buf, off_out + (size_t)n * sizeof(int)));
  int rc = POCS_OK;
  if (hipMemcpy(buf, env.data(), sizeof(pocs_env_dev), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(buf + off_x, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(buf + off_out, 0, (size_t)n * sizeof(int)) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe upload failed");
  const double* d_x = (const double*)(buf + off_x);
  if (rc == POCS_OK && pocs_launch_probe_discs((const pocs_env_dev*)buf, (const pocs_tables*)c->d_tables.p, n, d_x, d_x + n, d_x + 2 * (size_t)n,
                                               (int*)(buf + off_out), c->stream) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe launch failed");
  if (rc == POCS_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, POCS_E_DEVICE, "probe kernel failed");
  if (rc == POCS_OK && hipMemcpy(out, buf + off_out, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe download failed");
  (void)hipFree(buf);
  return rc;
}

// Test hook: which kinds of obstacle a pose touches under a ROUND footprint, on the device, for a chosen radius, boxes, discs and --
// where given -- disc covariances (include/pocs.h).  Nothing of the context's world, plans or modes is read: records and rows are
// prepared here, as upload_world prepares the context's under pocs_set_footprint_disc.
int pocs_probe_device_footprint_disc(pocs_ctx* c, double radius, const double* boxes, int M, const double* discs, int D, const double* cov,
                                     uint64_t seed, uint32_t waypoint_word, unsigned long long first, int n, const double* poses, int* out) {
  if (!c) return POCS_E_ARG;
  if (!poses || !out || n < 1 || n > (1 << 20) || M < 0 || D < 0 || M + D > POCS_MAX_OBSTACLES || (M > 0 && !boxes) || (D > 0 && !discs) ||
      (first & 1ull) || first > (1ull << 62))
    return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_disc: 1 <= n <= 2^20, 0 <= M, 0 <= D, M + D <= %d, first even and at most 2^62, no null pointers", POCS_MAX_OBSTACLES);
  if (!std::isfinite(radius) || radius < 0) return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_disc: the radius must be finite and >= 0");
  for (size_t j = 0; j < 5 * (size_t)M; ++j)
    if (!std::isfinite(boxes[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_disc: box %zu: value %zu is not finite", j / 5, j % 5);
  for (int m = 0; m < M; ++m)
    if (!(boxes[5 * (size_t)m + 2] > 0) || !(boxes[5 * (size_t)m + 3] > 0)) return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_disc: box %d: half extents must be > 0", m);
  for (size_t j = 0; j < 3 * (size_t)D; ++j)
    if (!std::isfinite(discs[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_disc: disc %zu: value %zu is not finite", j / 3, j % 3);
  for (int d = 0; d < D; ++d)
    if (!(discs[3 * (size_t)d + 2] > 0)) return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_disc: disc %d: the radius must be > 0", d);
  for (size_t j = 0; j < 3 * (size_t)n; ++j)
    if (!std::isfinite(poses[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_disc: pose %zu is not finite", j / 3);
  const double rho = radius == 0.0 ? 0.0 : radius;
  std::vector<pocs_env_dev> env(1);
  memset(env.data(), 0, sizeof(pocs_env_dev));
  env[0].fp = pocs_footprint{0.0, 0.0, rho, rho}; env[0].M = M + D;
  std::vector<double> rows(POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE, 0.0);
  for (int m = 0; m < M; ++m) pocs_prepare_obstacle_round(boxes + (size_t)m * 5, rho, &env[0].obs[(size_t)m * POCS_OBS_STRIDE]);
  for (int d = 0; d < D; ++d) {
    double* const rec = &env[0].obs[(size_t)(M + d) * POCS_OBS_STRIDE];
    pocs_prepare_disc_round(discs + (size_t)d * 3, rho, rec);
    if (cov) {
      double* const row = &rows[(size_t)(M + d) * POCS_NOISE_STRIDE];
      if (pocs_disc_noise_factor(cov + (size_t)d * 3, row) < 0)
        return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_disc: disc %d: neither zeros nor a finite covariance with sxx > 0 and syy - sxy^2 / sxx > 0", d);
      row[3] = (double)d;
      pocs_disc_noise_grow(row, rec);
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (int r = upload_tables(c)) return r;
  std::vector<double> h(2 * (size_t)n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 2; ++j) h[(size_t)j * n + i] = poses[3 * (size_t)i + j];      // (the heading is never read)
  // [env | rows | x | y] then [out n] ints
  static_assert(sizeof(pocs_env_dev) % 8 == 0, "the probe's buffer keeps its parts aligned");
  const size_t off_rows = sizeof(pocs_env_dev), off_x = off_rows + rows.size() * sizeof(double), off_out = off_x + 2 * (size_t)n * sizeof(double);
  char* buf = nullptr;
  HIPCHK(c, hipMalloc((void**)&buf, off_out + (size_t)n * sizeof(int)));
  int rc = POCS_OK;
  if (hipMemcpy(buf, env.data(), sizeof(pocs_env_dev), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(buf + off_rows, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(buf + off_x, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(buf + off_out, 0, (size_t)n * sizeof(int)) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe upload failed");
  const double* d_x = (const double*)(buf + off_x);
  if (rc == POCS_OK && pocs_launch_probe_footprint_disc((const pocs_env_dev*)buf, cov ? (const double*)(buf + off_rows) : nullptr,
                                                        (const pocs_tables*)c->d_tables.p, seed, waypoint_word, first, n, d_x, d_x + n,
                                                        (int*)(buf + off_out), c->stream) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe launch failed");
  if (rc == POCS_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, POCS_E_DEVICE, "probe kernel failed");
  if (rc == POCS_OK && hipMemcpy(out, buf + off_out, (size_t)n * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe download failed");
  (void)hipFree(buf);
  return rc;
}

// Test hook: the displaced centres and the touched displaced discs, on the device, for chosen poses, pose indices, footprint, discs and
// covariances (include/pocs.h).  Nothing of the context's world, plans or modes is read: records and rows are prepared here, as
// upload_world prepares the context's.
int pocs_probe_device_disc_noise(pocs_ctx* c, const double* fp4, const double* discs, const double* cov, int D, uint64_t seed,
                                 uint32_t waypoint_word, unsigned long long first, int n, const double* poses, double* centres_out,
                                 unsigned* flags_out) {
  if (!c) return POCS_E_ARG;
  if (!fp4 || !discs || !cov || !poses || !centres_out || !flags_out || D < 1 || D > 16 || n < 2 || n > (1 << 20) || (n & 1) || (first & 1ull) ||
      first > (1ull << 62))
    return fail(c, POCS_E_ARG, "pocs_probe_device_disc_noise: 1 <= D <= 16, 2 <= n <= 2^20 and even, first even and at most 2^62, no null pointers");
  for (int j = 0; j < 4; ++j)
    if (!std::isfinite(fp4[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_disc_noise: footprint value %d is not finite", j);
  if (!(fp4[2] > 0) || !(fp4[3] > 0)) return fail(c, POCS_E_ARG, "pocs_probe_device_disc_noise: footprint half extents must be > 0");
  for (size_t j = 0; j < 3 * (size_t)D; ++j)
    if (!std::isfinite(discs[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_disc_noise: disc %zu: value %zu is not finite", j / 3, j % 3);
  for (int d = 0; d < D; ++d)
    if (!(discs[3 * (size_t)d + 2] > 0)) return fail(c, POCS_E_ARG, "pocs_probe_device_disc_noise: disc %d: the radius must be > 0", d);
  for (size_t j = 0; j < 3 * (size_t)n; ++j)
    if (!std::isfinite(poses[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_disc_noise: pose %zu is not finite", j / 3);
  const pocs_footprint fp = {fp4[0], fp4[1], fp4[2], fp4[3]};
  std::vector<pocs_env_dev> env(1);
  memset(env.data(), 0, sizeof(pocs_env_dev));
  env[0].fp = fp; env[0].M = D;
  std::vector<double> rows(POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE, 0.0);
  for (int d = 0; d < D; ++d) {
    double* const rec = &env[0].obs[(size_t)d * POCS_OBS_STRIDE];
    pocs_prepare_disc(discs + (size_t)d * 3, &fp, rec);
    if (pocs_disc_noise_factor(cov + (size_t)d * 3, &rows[(size_t)d * POCS_NOISE_STRIDE]) < 0)
      return fail(c, POCS_E_ARG, "pocs_probe_device_disc_noise: disc %d: neither zeros nor a finite covariance with sxx > 0 and syy - sxy^2 / sxx > 0", d);
    rows[(size_t)d * POCS_NOISE_STRIDE + 3] = (double)d;
    pocs_disc_noise_grow(&rows[(size_t)d * POCS_NOISE_STRIDE], rec);
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (int r = upload_tables(c)) return r;
  std::vector<double> h(3 * (size_t)n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 3; ++j) h[(size_t)j * n + i] = poses[3 * (size_t)i + j];
  // [env | rows | x | y | th | centres n x D x 2] then [flags n] words
  static_assert(sizeof(pocs_env_dev) % 8 == 0, "the probe's buffer keeps its parts aligned");
  const size_t off_rows = sizeof(pocs_env_dev), off_x = off_rows + rows.size() * sizeof(double), off_c = off_x + 3 * (size_t)n * sizeof(double),
               nc = (size_t)n * (size_t)D * 2, off_f = off_c + nc * sizeof(double);
  char* buf = nullptr;
  HIPCHK(c, hipMalloc((void**)&buf, off_f + (size_t)n * sizeof(unsigned)));
  int rc = POCS_OK;
  if (hipMemcpy(buf, env.data(), sizeof(pocs_env_dev), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(buf + off_rows, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(buf + off_x, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(buf + off_c, 0, nc * sizeof(double) + (size_t)n * sizeof(unsigned)) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe upload failed");
  const double* d_x = (const double*)(buf + off_x);
  if (rc == POCS_OK && pocs_launch_probe_disc_noise((const pocs_env_dev*)buf, (const double*)(buf + off_rows), (const pocs_tables*)c->d_tables.p, seed,
                                                    waypoint_word, first, n, d_x, d_x + n, d_x + 2 * (size_t)n, (double*)(buf + off_c),
                                                    (unsigned*)(buf + off_f), c->stream) != hipSuccess)
    rc = fail(c, POCS_E_DEVICE, "probe launch failed");
  if (rc == POCS_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, POCS_E_DEVICE, "probe kernel failed");
  if (rc == POCS_OK && (hipMemcpy(centres_out, buf + off_c, nc * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
                        hipMemcpy(flags_out, buf + off_f, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess))
    rc = fail(c, POCS_E_DEVICE, "probe download failed");
  (void)hipFree(buf);
  return rc;
}

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

// pocs_probe.hip -- the test hooks of include/pocs.h: the eleven pocs_probe_device_* entries, which run the device's own inline
// functions on inputs a test picks (kernels: pocs_dev_probe.hpp, launched through pocs_launch_probe_* in pocs_kernels.hip).  Host
// code only.  An entry is its own range check, the shared argument checks, its own record preparation, and one Scratch: append the
// parts, launch, download.  But for pocs_probe_device_collide nothing of a context's world, plans or modes is read.
#include "pocs_ctx.hpp"

using namespace pocs_rt;

namespace {

// ---- argument checks: written once, with the entry's name and the item's noun; code POCS_E_ARG --------------------------------------
// all of count x width values finite
int all_finite(pocs_ctx* c, const char* entry, const char* noun, const double* v, int count, int width) {
  for (size_t j = 0; j < (size_t)count * (size_t)width; ++j)
    if (!std::isfinite(v[j])) return fail(c, POCS_E_ARG, "%s: %s %zu: value %zu is not finite", entry, noun, j / (size_t)width, j % (size_t)width);
  return POCS_OK;
}
// the half extents (columns 2 and 3) of `count` records > 0; the first record is reported as number `index0`
int extents_positive(pocs_ctx* c, const char* entry, const char* noun, const double* v, int count, int width, int index0 = 0) {
  for (int m = 0; m < count; ++m)
    if (!(v[(size_t)m * width + 2] > 0) || !(v[(size_t)m * width + 3] > 0)) return fail(c, POCS_E_ARG, "%s: %s %d: half extents must be > 0", entry, noun, index0 + m);
  return POCS_OK;
}
int boxes_ok(pocs_ctx* c, const char* entry, const double* boxes, int M) {
  if (int r = all_finite(c, entry, "box", boxes, M, 5)) return r;
  return extents_positive(c, entry, "box", boxes, M, 5);
}
int discs_ok(pocs_ctx* c, const char* entry, const double* discs, int D) {
  if (int r = all_finite(c, entry, "disc", discs, D, 3)) return r;
  for (int d = 0; d < D; ++d)
    if (!(discs[3 * (size_t)d + 2] > 0)) return fail(c, POCS_E_ARG, "%s: disc %d: the radius must be > 0", entry, d);
  return POCS_OK;
}
int footprint_ok(pocs_ctx* c, const char* entry, const double* fp4) {
  for (int j = 0; j < 4; ++j)
    if (!std::isfinite(fp4[j])) return fail(c, POCS_E_ARG, "%s: footprint value %d is not finite", entry, j);
  if (!(fp4[2] > 0) || !(fp4[3] > 0)) return fail(c, POCS_E_ARG, "%s: footprint half extents must be > 0", entry);
  return POCS_OK;
}
int poses_ok(pocs_ctx* c, const char* entry, const double* poses, int n) {
  for (size_t j = 0; j < 3 * (size_t)n; ++j)
    if (!std::isfinite(poses[j])) return fail(c, POCS_E_ARG, "%s: pose %zu is not finite", entry, j / 3);
  return POCS_OK;
}

// ---- record preparation ---------------------------------------------------------------------------------------------------------------
// n x 3 poses (x, y, theta) by column: x_0 .. x_{n-1}, y .., and -- cols 3 -- theta ..
std::vector<double> pose_columns(const double* poses, int n, int cols = 3) {
  std::vector<double> h((size_t)cols * (size_t)n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < cols; ++j) h[(size_t)j * n + i] = poses[3 * (size_t)i + j];
  return h;
}
// The bare record of M boxes, then D discs, for a footprint: prepared record by record as upload_world prepares the context's.
typedef void (*prepare_fn)(const double* item, const pocs_footprint* fp, double* rec);
void bare_env(pocs_env_dev* env, const pocs_footprint& fp, const double* boxes, int M, prepare_fn box, const double* discs = nullptr, int D = 0,
              prepare_fn disc = nullptr) {
  memset(env, 0, sizeof *env);
  env->fp = fp; env->M = M + D;
  for (int m = 0; m < M; ++m) box(boxes + (size_t)m * 5, &fp, &env->obs[(size_t)m * POCS_OBS_STRIDE]);
  for (int d = 0; d < D; ++d) disc(discs + (size_t)d * 3, &fp, &env->obs[(size_t)(M + d) * POCS_OBS_STRIDE]);
}
// The factor row {l00, l10, l11, disc index} of disc d's covariance, and its record grown by the row.
int noise_row(pocs_ctx* c, const char* entry, const double* cov3, int d, double* row, double* rec) {
  if (pocs_disc_noise_factor(cov3, row) < 0)
    return fail(c, POCS_E_ARG, "%s: disc %d: neither zeros nor a finite covariance with sxx > 0 and syy - sxy^2 / sxx > 0", entry, d);
  row[3] = (double)d;
  pocs_disc_noise_grow(row, rec);
  return POCS_OK;
}
int device_with_tables(pocs_ctx* c) {
  HIPCHK(c, hipSetDevice(c->device));
  return upload_tables(c);
}

// ---- one device allocation per probe call -----------------------------------------------------------------------------------------------
// The parts are appended in turn -- host bytes to upload, or a byte count to zero -- and lie 8-byte aligned one behind the other
// in ONE allocation, which the destructor frees: upload(), at<T>(part) for the launch, ran(launch), download(part, ..).
struct Scratch {
  struct Part { const void* src; size_t bytes, off; };
  pocs_ctx* c;
  std::vector<Part> parts;
  size_t total = 0;
  char* buf = nullptr;
  explicit Scratch(pocs_ctx* ctx) : c(ctx) {}
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() { (void)hipFree(buf); }
  int add(const void* src, size_t bytes) {             // -> the part's number
    parts.push_back(Part{src, bytes, total});
    total += (bytes + 7) & ~(size_t)7;
    return (int)parts.size() - 1;
  }
  int zeros(size_t bytes) { return add(nullptr, bytes); }
  template <typename T> T* at(int part) const { return reinterpret_cast<T*>(buf + parts[(size_t)part].off); }
  int upload() {
    HIPCHK(c, hipMalloc((void**)&buf, total));
    for (const Part& p : parts)
      if ((p.src ? hipMemcpy(buf + p.off, p.src, p.bytes, hipMemcpyHostToDevice) : hipMemset(buf + p.off, 0, p.bytes)) != hipSuccess)
        return fail(c, POCS_E_DEVICE, "probe upload failed");
    return POCS_OK;
  }
  int ran(hipError_t launch) {                         // the launch's own answer, then the kernel's
    if (launch != hipSuccess) return fail(c, POCS_E_DEVICE, "probe launch failed");
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, POCS_E_DEVICE, "probe kernel failed");
    return POCS_OK;
  }
  int download(int part, void* dst, size_t bytes, size_t from = 0) {
    if (hipMemcpy(dst, buf + parts[(size_t)part].off + from, bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(c, POCS_E_DEVICE, "probe download failed");
    return POCS_OK;
  }
};

}  // namespace

extern "C" {

// Test hook: the device's table-driven sampler functions on chosen inputs (include/pocs.h).
int pocs_probe_device_math(pocs_ctx* c, int n, const uint32_t* radius_words, const uint32_t* angle_words, const double* headings,
                           double* z0, double* z1, double* sn, double* cs, double* radius2) {
  if (!c || n < 1 || n > (1 << 20) || !radius_words || !angle_words || !headings || !z0 || !z1 || !sn || !cs || !radius2) return c ? fail(c, POCS_E_ARG, "pocs_probe_device_math: 1 <= n <= 2^20, no null pointers") : POCS_E_ARG;
  if (int r = device_with_tables(c)) return r;
  const size_t nw = (size_t)n * sizeof(uint32_t), nd = (size_t)n * sizeof(double);
  Scratch s(c);
  const int wr = s.add(radius_words, nw), wa = s.add(angle_words, nw), x = s.add(headings, nd), out = s.zeros(5 * nd);
  if (int r = s.upload()) return r;
  if (int r = s.ran(pocs_launch_probe_math((const pocs_tables*)c->d_tables.p, n, s.at<uint32_t>(wr), s.at<uint32_t>(wa), s.at<double>(x), s.at<double>(out), c->stream))) return r;
  double* dst[5] = {z0, z1, sn, cs, radius2};
  for (int j = 0; j < 5; ++j)
    if (int r = s.download(out, dst[j], nd, (size_t)j * nd)) return r;
  return POCS_OK;
}

// Test hook: the two square roots of the Box-Muller radius on a range of words (include/pocs.h).
int pocs_probe_device_radius_roots(pocs_ctx* c, uint32_t first_word, unsigned long long count, unsigned long long* mismatches, uint32_t* first_bad) {
  if (!c) return POCS_E_ARG;
  if (!mismatches || !first_bad || count < 1 || (unsigned long long)first_word + count > (1ull << 32))
    return fail(c, POCS_E_ARG, "pocs_probe_device_radius_roots: count >= 1, first_word + count <= 2^32, no null pointers");
  if (int r = device_with_tables(c)) return r;
  unsigned long long h[2] = {0ull, ~0ull};           // [mismatches | smallest mismatching word]
  Scratch s(c);
  const int out = s.add(h, sizeof h);
  if (int r = s.upload()) return r;
  if (int r = s.ran(pocs_launch_probe_radius_roots((const pocs_tables*)c->d_tables.p, first_word, count, s.at<unsigned long long>(out), c->stream))) return r;
  if (int r = s.download(out, h, sizeof h)) return r;
  *mismatches = h[0];
  *first_bad = h[0] ? (uint32_t)h[1] : 0u;
  return POCS_OK;
}

// Test hook: the device's collision test and obstacle cull on chosen poses and a chosen mixture (include/pocs.h): the one probe that
// reads the context's world.
int pocs_probe_device_collide(pocs_ctx* c, int K, const double* params, int n, const double* poses, int* flag_full, int* flag_pair,
                              int* flag_pair_eager, int* nkeep, double* kept) {
  static const char E[] = "pocs_probe_device_collide";
  if (!c) return POCS_E_ARG;
  if (!params || !poses || !flag_full || !flag_pair || !flag_pair_eager || !nkeep || !kept || n < 1 || n > (1 << 20) || K < 1 || K > POCS_MAX_GAUSSIANS)
    return fail(c, POCS_E_ARG, "pocs_probe_device_collide: 1 <= n <= 2^20, 1 <= K <= %d, no null pointers", POCS_MAX_GAUSSIANS);
  if (!c->have_obstacles)
    return fail(c, POCS_E_STATE, "no collision world: pocs_set_obstacles / addObstacle / clearObstacles missing");
  if (int r = may_enter(c, E, pocs_modes::kProbe)) return r;
  if (discs_applied(c))                              // (this probe's three forms test boxes: a world with discs is probed by pocs_probe_device_discs)
    return fail(c, POCS_E_STATE, "pocs_probe_device_collide: discs are set (pocs_set_discs); the probe tests boxes only, pocs_probe_device_discs probes a world with discs");
  // (a heading that is not a number has no sector: nothing of the kind reaches the device)
  const size_t PS = (size_t)K * POCS_PARAM_STRIDE;
  for (size_t j = 0; j < PS; ++j)
    if (!std::isfinite(params[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_collide: parameter %zu is not finite", j);
  if (int r = poses_ok(c, E, poses, n)) return r;
  HIPCHK(c, hipSetDevice(c->device));
  if (int r = upload_world(c)) return r;
  const std::vector<double> h = pose_columns(poses, n);
  const size_t nrec = (size_t)POCS_MAX_OBSTACLES * POCS_OBS_STRIDE, ni = 3 * (size_t)n + 1;      // flags 3 n, then nkeep
  Scratch s(c);
  const int par = s.add(params, PS * sizeof(double)), x = s.add(h.data(), h.size() * sizeof(double)), rec = s.zeros(nrec * sizeof(double)),
            flags = s.zeros(ni * sizeof(int));
  if (int r = s.upload()) return r;
  pocs_gmm_launch a;
  memset(&a, 0, sizeof a);
  fill_gmm_world(c, &a, 0);                         // (under an obstacle schedule: world 0)
  a.param = s.at<double>(par); a.W = 1; a.nruns = 1; a.run_cnt = 1;
  const double* d_x = s.at<double>(x);
  int* d_flags = s.at<int>(flags);
  if (int r = s.ran(pocs_launch_probe_collide(K, a, n, d_x, d_x + n, d_x + 2 * (size_t)n, d_flags, d_flags + 3 * (size_t)n, s.at<double>(rec), c->stream))) return r;
  std::vector<int> f(ni, 0);
  if (int r = s.download(flags, f.data(), ni * sizeof(int))) return r;
  if (int r = s.download(rec, kept, nrec * sizeof(double))) return r;
  memcpy(flag_full, f.data(), (size_t)n * sizeof(int));
  memcpy(flag_pair, f.data() + n, (size_t)n * sizeof(int));
  memcpy(flag_pair_eager, f.data() + 2 * (size_t)n, (size_t)n * sizeof(int));
  *nkeep = f[3 * (size_t)n];
  return POCS_OK;
}

// Test hook: the device's clearance level on chosen poses, footprint, distances and boxes (include/pocs.h).
int pocs_probe_device_clearance(pocs_ctx* c, const double* fp4, const double* d, int L, const double* boxes, int M, int n,
                                const double* poses, int* level_out) {
  static const char E[] = "pocs_probe_device_clearance";
  if (!c) return POCS_E_ARG;
  if (!fp4 || !poses || !level_out || n < 1 || n > (1 << 20) || L < 0 || L > POCS_MAX_CLEARANCE_LEVELS || (L > 0 && !d) || M < 0 || M > POCS_MAX_OBSTACLES || (M > 0 && !boxes))
    return fail(c, POCS_E_ARG, "pocs_probe_device_clearance: 1 <= n <= 2^20, 0 <= L <= %d, 0 <= M <= %d, no null pointers", POCS_MAX_CLEARANCE_LEVELS, POCS_MAX_OBSTACLES);
  if (int r = footprint_ok(c, E, fp4)) return r;
  for (int l = 0; l < L; ++l)
    if (!std::isfinite(d[l]) || !(d[l] > (l ? d[l - 1] : 0.0)))
      return fail(c, POCS_E_ARG, "pocs_probe_device_clearance: distance %d: finite distances with 0 < d[0] < d[1] < ... are needed", l);
  if (int r = boxes_ok(c, E, boxes, M)) return r;
  if (int r = poses_ok(c, E, poses, n)) return r;
  if (int r = device_with_tables(c)) return r;
  const pocs_footprint fp = {fp4[0], fp4[1], fp4[2], fp4[3]};
  pocs_env_dev env;
  bare_env(&env, fp, boxes, M, pocs_prepare_obstacle);
  std::vector<pocs_clear_dev> clr(1);
  prepare_clearance(fp, d, L, boxes, M, clr.data());
  const std::vector<double> h = pose_columns(poses, n);
  Scratch s(c);
  const int p_env = s.add(&env, sizeof env), p_clr = s.add(clr.data(), sizeof(pocs_clear_dev)), x = s.add(h.data(), h.size() * sizeof(double)),
            out = s.zeros((size_t)n * sizeof(int));
  if (int r = s.upload()) return r;
  const double* d_x = s.at<double>(x);
  if (int r = s.ran(pocs_launch_probe_clearance(s.at<pocs_env_dev>(p_env), s.at<pocs_clear_dev>(p_clr), L, (const pocs_tables*)c->d_tables.p, n,
                                                d_x, d_x + n, d_x + 2 * (size_t)n, s.at<int>(out), c->stream))) return r;
  return s.download(out, level_out, (size_t)n * sizeof(int));
}

// Test hook: which parts of a compound footprint touch, on the device, for chosen poses, parts and boxes (include/pocs.h).
int pocs_probe_device_footprint_parts(pocs_ctx* c, const double* parts, int F, const double* boxes, int M, int n,
                                      const double* poses, int* touched_out) {
  static const char E[] = "pocs_probe_device_footprint_parts";
  if (!c) return POCS_E_ARG;
  if (!parts || !poses || !touched_out || n < 1 || n > (1 << 20) || F < 1 || F > POCS_MAX_FOOTPRINT_PARTS || M < 0 || M > POCS_MAX_OBSTACLES || (M > 0 && !boxes))
    return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_parts: 1 <= n <= 2^20, 1 <= F <= %d, 0 <= M <= %d, no null pointers", POCS_MAX_FOOTPRINT_PARTS, POCS_MAX_OBSTACLES);
  if (int r = all_finite(c, E, "part", parts, F, 4)) return r;
  if (int r = extents_positive(c, E, "part", parts, F, 4)) return r;
  if (int r = boxes_ok(c, E, boxes, M)) return r;
  if (int r = poses_ok(c, E, poses, n)) return r;
  if (int r = device_with_tables(c)) return r;
  pocs_footprint fps[POCS_MAX_FOOTPRINT_PARTS];
  for (int f = 0; f < F; ++f) fps[f] = pocs_footprint{parts[4 * f], parts[4 * f + 1], parts[4 * f + 2], parts[4 * f + 3]};
  pocs_env_dev env;
  pocs_parts_dev pd;
  prepare_parts(fps, F, boxes, M, &env, &pd);
  const std::vector<double> h = pose_columns(poses, n);
  Scratch s(c);
  const int p_env = s.add(&env, sizeof env), p_parts = s.add(&pd, sizeof pd), x = s.add(h.data(), h.size() * sizeof(double)),
            out = s.zeros((size_t)n * sizeof(int));
  if (int r = s.upload()) return r;
  const double* d_x = s.at<double>(x);
  if (int r = s.ran(pocs_launch_probe_parts(s.at<pocs_env_dev>(p_env), s.at<pocs_parts_dev>(p_parts), F, (const pocs_tables*)c->d_tables.p, n,
                                            d_x, d_x + n, d_x + 2 * (size_t)n, s.at<int>(out), c->stream))) return r;
  return s.download(out, touched_out, (size_t)n * sizeof(int));
}

// Test hook: which watched regions the device finds chosen poses in, for a footprint and regions of the caller's own
// (include/pocs.h).
int pocs_probe_device_regions(pocs_ctx* c, const double* fp4, const double* boxes, const int* kinds, int G, int n,
                              const double* poses, int* mask_out) {
  static const char E[] = "pocs_probe_device_regions";
  if (!c) return POCS_E_ARG;
  if (!fp4 || !poses || !mask_out || n < 1 || n > (1 << 20) || G < 0 || G > POCS_MAX_REGIONS || (G > 0 && (!boxes || !kinds)))
    return fail(c, POCS_E_ARG, "pocs_probe_device_regions: 1 <= n <= 2^20, 0 <= G <= %d, no null pointers", POCS_MAX_REGIONS);
  if (int r = footprint_ok(c, E, fp4)) return r;
  if (int r = all_finite(c, E, "region", boxes, G, 5)) return r;
  for (int g = 0; g < G; ++g) {                      // (region by region: its extents, then its kind)
    if (int r = extents_positive(c, E, "region", boxes + 5 * (size_t)g, 1, 5, g)) return r;
    if (kinds[g] != POCS_REGION_TOUCH && kinds[g] != POCS_REGION_POINT) return fail(c, POCS_E_ARG, "pocs_probe_device_regions: region %d: kind %d", g, kinds[g]);
  }
  if (int r = poses_ok(c, E, poses, n)) return r;
  if (int r = device_with_tables(c)) return r;
  const pocs_footprint fp = {fp4[0], fp4[1], fp4[2], fp4[3]};
  pocs_regions_dev reg;
  prepare_regions(fp, boxes, kinds, G, &reg);
  const std::vector<double> h = pose_columns(poses, n);
  Scratch s(c);
  const int p_reg = s.add(&reg, sizeof reg), x = s.add(h.data(), h.size() * sizeof(double)), out = s.zeros((size_t)n * sizeof(int));
  if (int r = s.upload()) return r;
  const double* d_x = s.at<double>(x);
  if (int r = s.ran(pocs_launch_probe_regions(s.at<pocs_regions_dev>(p_reg), G, (const pocs_tables*)c->d_tables.p, n,
                                              d_x, d_x + n, d_x + 2 * (size_t)n, s.at<int>(out), c->stream))) return r;
  return s.download(out, mask_out, (size_t)n * sizeof(int));
}

// Test hook: which sub-poses of a segment touch, on the device, for chosen poses, footprint, boxes, control and J (include/pocs.h).
int pocs_probe_device_segment(pocs_ctx* c, const double* fp4, const double* boxes, int M, const double* u3, int J, int backward, int n,
                              const double* poses, int* mask_out) {
  static const char E[] = "pocs_probe_device_segment";
  if (!c) return POCS_E_ARG;
  if (!fp4 || !u3 || !poses || !mask_out || n < 1 || n > (1 << 20) || J < 1 || J > POCS_MAX_SEGMENT_CHECKS || M < 0 || M > POCS_MAX_OBSTACLES ||
      (M > 0 && !boxes) || (backward != 0 && backward != 1))
    return fail(c, POCS_E_ARG, "pocs_probe_device_segment: 1 <= n <= 2^20, 1 <= J <= %d, 0 <= M <= %d, backward 0 or 1, no null pointers", POCS_MAX_SEGMENT_CHECKS, POCS_MAX_OBSTACLES);
  if (int r = footprint_ok(c, E, fp4)) return r;
  for (int j = 0; j < 3; ++j)
    if (!std::isfinite(u3[j])) return fail(c, POCS_E_ARG, "pocs_probe_device_segment: control value %d is not finite", j);
  if (int r = boxes_ok(c, E, boxes, M)) return r;
  if (int r = poses_ok(c, E, poses, n)) return r;
  if (int r = device_with_tables(c)) return r;
  const pocs_footprint fp = {fp4[0], fp4[1], fp4[2], fp4[3]};
  pocs_env_dev env;
  bare_env(&env, fp, boxes, M, pocs_prepare_obstacle);
  pocs_seg_dev sg;
  prepare_segment(J, &sg);
  const std::vector<double> h = pose_columns(poses, n);
  Scratch s(c);
  const int p_env = s.add(&env, sizeof env), p_seg = s.add(&sg, sizeof sg), x = s.add(h.data(), h.size() * sizeof(double)),
            out = s.zeros((size_t)n * sizeof(int));
  if (int r = s.upload()) return r;
  const double* d_x = s.at<double>(x);
  if (int r = s.ran(pocs_launch_probe_segment(s.at<pocs_env_dev>(p_env), s.at<pocs_seg_dev>(p_seg), (const pocs_tables*)c->d_tables.p, u3[0], u3[1], u3[2],
                                              backward, n, d_x, d_x + n, d_x + 2 * (size_t)n, s.at<int>(out), c->stream))) return r;
  return s.download(out, mask_out, (size_t)n * sizeof(int));
}

// Test hook: the device's component counts on chosen weights, alive flags, seeds, waypoints and sample totals (include/pocs.h).
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
  const size_t nk = (size_t)n * KM;
  std::vector<double> h(2 * nk + (size_t)n, 0.0);    // [w | alive] n x KM doubles each, [n_total] n doubles
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < K[i]; ++k) {                       // (what lies behind a case's K is not read, here or on the device)
      h[(size_t)i * KM + k] = weights[(size_t)i * KM + k];
      h[nk + (size_t)i * KM + k] = alive[(size_t)i * KM + k];
    }
    h[2 * nk + (size_t)i] = (double)n_total[i];
  }
  Scratch s(c);
  const int in = s.add(h.data(), h.size() * sizeof(double)), out = s.zeros(nk * sizeof(double)), seed = s.add(seeds, (size_t)n * sizeof(uint64_t)),
            wp = s.add(waypoints, (size_t)n * sizeof(uint32_t)), Kc = s.add(K, (size_t)n * sizeof(int));
  if (int r = s.upload()) return r;
  const double* d_w = s.at<double>(in);
  if (int r = s.ran(pocs_launch_probe_counts(n, s.at<int>(Kc), d_w, d_w + nk, s.at<unsigned long long>(seed), s.at<uint32_t>(wp), d_w + 2 * nk,
                                             s.at<double>(out), c->stream))) return r;
  return s.download(out, counts_out, nk * sizeof(double));
}

// Test hook: which kinds of obstacle a pose touches, on the device, for chosen poses, footprint, boxes and discs (include/pocs.h): the
// composed record is boxes, then discs.
int pocs_probe_device_discs(pocs_ctx* c, const double* fp4, const double* boxes, int M, const double* discs, int D, int n,
                            const double* poses, int* out) {
  static const char E[] = "pocs_probe_device_discs";
  if (!c) return POCS_E_ARG;
  if (!fp4 || !poses || !out || n < 1 || n > (1 << 20) || M < 0 || D < 0 || M + D > POCS_MAX_OBSTACLES || (M > 0 && !boxes) || (D > 0 && !discs))
    return fail(c, POCS_E_ARG, "pocs_probe_device_discs: 1 <= n <= 2^20, 0 <= M, 0 <= D, M + D <= %d, no null pointers", POCS_MAX_OBSTACLES);
  if (int r = footprint_ok(c, E, fp4)) return r;
  if (int r = boxes_ok(c, E, boxes, M)) return r;
  if (int r = discs_ok(c, E, discs, D)) return r;
  if (int r = poses_ok(c, E, poses, n)) return r;
  if (int r = device_with_tables(c)) return r;
  pocs_env_dev env;
  bare_env(&env, pocs_footprint{fp4[0], fp4[1], fp4[2], fp4[3]}, boxes, M, pocs_prepare_box_beside_discs, discs, D, pocs_prepare_disc);
  const std::vector<double> h = pose_columns(poses, n);
  Scratch s(c);
  const int p_env = s.add(&env, sizeof env), x = s.add(h.data(), h.size() * sizeof(double)), flags = s.zeros((size_t)n * sizeof(int));
  if (int r = s.upload()) return r;
  const double* d_x = s.at<double>(x);
  if (int r = s.ran(pocs_launch_probe_discs(s.at<pocs_env_dev>(p_env), (const pocs_tables*)c->d_tables.p, n, d_x, d_x + n, d_x + 2 * (size_t)n,
                                            s.at<int>(flags), c->stream))) return r;
  return s.download(flags, out, (size_t)n * sizeof(int));
}

// Test hook: which kinds of obstacle a pose touches under a ROUND footprint, on the device, for a chosen radius, boxes, discs and --
// where given -- disc covariances (include/pocs.h): records and rows as upload_world prepares them under pocs_set_footprint_disc.
int pocs_probe_device_footprint_disc(pocs_ctx* c, double radius, const double* boxes, int M, const double* discs, int D, const double* cov,
                                     uint64_t seed, uint32_t waypoint_word, unsigned long long first, int n, const double* poses, int* out) {
  static const char E[] = "pocs_probe_device_footprint_disc";
  if (!c) return POCS_E_ARG;
  if (!poses || !out || n < 1 || n > (1 << 20) || M < 0 || D < 0 || M + D > POCS_MAX_OBSTACLES || (M > 0 && !boxes) || (D > 0 && !discs) ||
      (first & 1ull) || first > (1ull << 62))
    return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_disc: 1 <= n <= 2^20, 0 <= M, 0 <= D, M + D <= %d, first even and at most 2^62, no null pointers", POCS_MAX_OBSTACLES);
  if (!std::isfinite(radius) || radius < 0) return fail(c, POCS_E_ARG, "pocs_probe_device_footprint_disc: the radius must be finite and >= 0");
  if (int r = boxes_ok(c, E, boxes, M)) return r;
  if (int r = discs_ok(c, E, discs, D)) return r;
  if (int r = poses_ok(c, E, poses, n)) return r;
  const double rho = radius == 0.0 ? 0.0 : radius;
  pocs_env_dev env;                                  // (the footprint's half extents carry rho to the round preparations)
  bare_env(&env, pocs_footprint{0.0, 0.0, rho, rho}, boxes, M, [](const double* b, const pocs_footprint* fp, double* rec) { pocs_prepare_obstacle_round(b, fp->hx, rec); },
           discs, D, [](const double* d, const pocs_footprint* fp, double* rec) { pocs_prepare_disc_round(d, fp->hx, rec); });
  std::vector<double> rows(POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE, 0.0);
  for (int d = 0; cov && d < D; ++d)
    if (int r = noise_row(c, E, cov + (size_t)d * 3, d, &rows[(size_t)(M + d) * POCS_NOISE_STRIDE], &env.obs[(size_t)(M + d) * POCS_OBS_STRIDE])) return r;
  if (int r = device_with_tables(c)) return r;
  const std::vector<double> h = pose_columns(poses, n, 2);      // (the heading is never read)
  Scratch s(c);
  const int p_env = s.add(&env, sizeof env), p_rows = s.add(rows.data(), rows.size() * sizeof(double)), x = s.add(h.data(), h.size() * sizeof(double)),
            flags = s.zeros((size_t)n * sizeof(int));
  if (int r = s.upload()) return r;
  const double* d_x = s.at<double>(x);
  if (int r = s.ran(pocs_launch_probe_footprint_disc(s.at<pocs_env_dev>(p_env), cov ? s.at<double>(p_rows) : nullptr, (const pocs_tables*)c->d_tables.p, seed,
                                                     waypoint_word, first, n, d_x, d_x + n, s.at<int>(flags), c->stream))) return r;
  return s.download(flags, out, (size_t)n * sizeof(int));
}

// Test hook: the displaced centres and the touched displaced discs, on the device, for chosen poses, pose indices, footprint, discs and
// covariances (include/pocs.h): records and rows as upload_world prepares the context's.
int pocs_probe_device_disc_noise(pocs_ctx* c, const double* fp4, const double* discs, const double* cov, int D, uint64_t seed,
                                 uint32_t waypoint_word, unsigned long long first, int n, const double* poses, double* centres_out,
                                 unsigned* flags_out) {
  static const char E[] = "pocs_probe_device_disc_noise";
  if (!c) return POCS_E_ARG;
  if (!fp4 || !discs || !cov || !poses || !centres_out || !flags_out || D < 1 || D > 16 || n < 2 || n > (1 << 20) || (n & 1) || (first & 1ull) ||
      first > (1ull << 62))
    return fail(c, POCS_E_ARG, "pocs_probe_device_disc_noise: 1 <= D <= 16, 2 <= n <= 2^20 and even, first even and at most 2^62, no null pointers");
  if (int r = footprint_ok(c, E, fp4)) return r;
  if (int r = discs_ok(c, E, discs, D)) return r;
  if (int r = poses_ok(c, E, poses, n)) return r;
  pocs_env_dev env;
  bare_env(&env, pocs_footprint{fp4[0], fp4[1], fp4[2], fp4[3]}, nullptr, 0, nullptr, discs, D, pocs_prepare_disc);
  std::vector<double> rows(POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE, 0.0);
  for (int d = 0; d < D; ++d)
    if (int r = noise_row(c, E, cov + (size_t)d * 3, d, &rows[(size_t)d * POCS_NOISE_STRIDE], &env.obs[(size_t)d * POCS_OBS_STRIDE])) return r;
  if (int r = device_with_tables(c)) return r;
  const std::vector<double> h = pose_columns(poses, n);
  const size_t nc = (size_t)n * (size_t)D * 2;       // centres n x D x 2
  Scratch s(c);
  const int p_env = s.add(&env, sizeof env), p_rows = s.add(rows.data(), rows.size() * sizeof(double)), x = s.add(h.data(), h.size() * sizeof(double)),
            centres = s.zeros(nc * sizeof(double)), flags = s.zeros((size_t)n * sizeof(unsigned));
  if (int r = s.upload()) return r;
  const double* d_x = s.at<double>(x);
  if (int r = s.ran(pocs_launch_probe_disc_noise(s.at<pocs_env_dev>(p_env), s.at<double>(p_rows), (const pocs_tables*)c->d_tables.p, seed, waypoint_word, first, n,
                                                 d_x, d_x + n, d_x + 2 * (size_t)n, s.at<double>(centres), s.at<unsigned>(flags), c->stream))) return r;
  if (int r = s.download(centres, centres_out, nc * sizeof(double))) return r;
  return s.download(flags, flags_out, (size_t)n * sizeof(unsigned));
}

// Test hook: which discs exist for a pose and which it touches, on the device, for chosen poses, pose indices, footprint, discs,
// covariances (may be null: none) and hypotheses (include/pocs.h): records, rows and gates as upload_world prepares the context's.
int pocs_probe_device_disc_hypotheses(pocs_ctx* c, const double* fp4, const double* discs, const double* cov, const int* group,
                                      const double* weight, int D, uint64_t seed, uint32_t waypoint_word, unsigned long long first, int n,
                                      const double* poses, unsigned* exists_out, unsigned* flags_out) {
  static const char E[] = "pocs_probe_device_disc_hypotheses";
  if (!c) return POCS_E_ARG;
  if (!fp4 || !discs || !group || !weight || !poses || !exists_out || !flags_out || D < 1 || D > 32 || n < 2 || n > (1 << 20) || (n & 1) ||
      (first & 1ull) || first > (1ull << 62))
    return fail(c, POCS_E_ARG, "pocs_probe_device_disc_hypotheses: 1 <= D <= 32, 2 <= n <= 2^20 and even, first even and at most 2^62, no null pointers but the covariances");
  if (int r = footprint_ok(c, E, fp4)) return r;
  if (int r = discs_ok(c, E, discs, D)) return r;
  if (int r = poses_ok(c, E, poses, n)) return r;
  unsigned long long lo[32], hi[32];
  int bad = 0;
  if (const int k = pocs_hyp_thresholds(group, weight, D, lo, hi, &bad))
    return fail(c, POCS_E_ARG, "pocs_probe_device_disc_hypotheses: disc %d: %s", bad, hyp_refusal(k));
  pocs_env_dev env;
  bare_env(&env, pocs_footprint{fp4[0], fp4[1], fp4[2], fp4[3]}, nullptr, 0, nullptr, discs, D, pocs_prepare_disc);
  std::vector<double> rows(POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE, 0.0);
  std::vector<uint32_t> gates(POCS_MAX_OBSTACLES * POCS_GATE_STRIDE, 0u);
  for (int d = 0; d < D; ++d) {
    if (cov)
      if (int r = noise_row(c, E, cov + (size_t)d * 3, d, &rows[(size_t)d * POCS_NOISE_STRIDE], &env.obs[(size_t)d * POCS_OBS_STRIDE])) return r;
    pocs_hyp_gate(group[d], lo[d], hi[d], &gates[(size_t)d * POCS_GATE_STRIDE]);
  }
  if (int r = device_with_tables(c)) return r;
  const std::vector<double> h = pose_columns(poses, n);
  Scratch s(c);
  const int p_env = s.add(&env, sizeof env), p_rows = s.add(rows.data(), rows.size() * sizeof(double)),
            p_gates = s.add(gates.data(), gates.size() * sizeof(uint32_t)), x = s.add(h.data(), h.size() * sizeof(double)),
            exists = s.zeros((size_t)n * sizeof(unsigned)), flags = s.zeros((size_t)n * sizeof(unsigned));
  if (int r = s.upload()) return r;
  const double* d_x = s.at<double>(x);
  if (int r = s.ran(pocs_launch_probe_disc_hypotheses(s.at<pocs_env_dev>(p_env), s.at<double>(p_rows), s.at<uint32_t>(p_gates), (const pocs_tables*)c->d_tables.p,
                                                      seed, waypoint_word, first, n, d_x, d_x + n, d_x + 2 * (size_t)n, s.at<unsigned>(exists),
                                                      s.at<unsigned>(flags), c->stream))) return r;
  if (int r = s.download(exists, exists_out, (size_t)n * sizeof(unsigned))) return r;
  return s.download(flags, flags_out, (size_t)n * sizeof(unsigned));
}

}  // extern "C"

// pocs_api.hip -- the C ABI's front (include/pocs.h): context life cycle, the typed setters and getters, the run* calls with
// their run-ahead, and the MCModule-compatible text dispatcher (mirrors MCModule, mcsimplugin/mcsimplugin.cpp:7-232).
// Without a HIP device pocs_create fails: there is no CPU path.
#include <new>

#include "pocs_ctx.hpp"
#include "pocs_command.hpp"

#define POCS_VERSION_STRING "pocs-mi355x 0.4 (gfx950; numerics v9: summation tree of 512-pair chunks, 256 virtual slices)"

using namespace pocs_rt;

// ---- text dispatcher: replies and the help text ----
static int put(pocs_ctx* c, char* out, size_t cap, const char* text) {
  if (!out || cap == 0) return POCS_OK;
  const size_t n = strlen(text);
  if (n + 1 > cap) { out[0] = 0; return fail(c, POCS_E_BUFFER, "reply needs %zu bytes", n + 1); }
  memcpy(out, text, n + 1);
  return POCS_OK;
}

static const char* kHelp =
    "MyCommand        This is an example command\n"
    "ArmaCommand      kept for compatibility (no-op)\n"
    "setAlphas        a1 a2 a3 a4: squared odometry noise coefficients\n"
    "setQ             q: variance of the range sensor noise\n"
    "setNumLandmarks  n\n"
    "setLandmarks     x_0..x_{n-1} y_0..y_{n-1}\n"
    "setNumParticles  n: particles of the MC simulation\n"
    "setInitialCovariance  c00 c01 c02 c10 .. c22 (row major)\n"
    "setPathLength    W\n"
    "setTrajectory    x_0..x_{W-1} y_0..y_{W-1} theta_0..theta_{W-1}\n"
    "setOdometry      r1_0.. tr_0.. r2_0.. (W-1 each)\n"
    "runSimulation    run the MC simulation, replies the collision probability\n"
    "setNumGaussians  k: components of the mixture (1..8)\n"
    "runGMMEstimation sampling-based GMM estimate, replies the collision probability\n"
    "setNumGMMSamples n: samples per waypoint for the GMM estimate\n"
    "setSeed          s: 64-bit seed of the counter-based random streams (new)\n"
    "setFootprint     dx dy half_x half_y (new)\n"
    "addObstacle      cx cy half_x half_y yaw_rad (new)\n"
    "clearObstacles   (new)\n"
    "setBatch         r: independent GMM estimations advanced in lockstep per runGMMEstimation (new)\n"
    "setRunAhead      r: with one run per command, evaluate the next r runs in one launch and serve the following commands from it (new)\n"
    "help             this text\n";

// ---- the shapes every setter and getter shares ----
// A setter's prologue: false for a null context; otherwise it TOUCHES before it validates (a refused setter ends run-ahead serving too).
static bool setter(pocs_ctx* c) {
  if (c) touch(c);
  return c != nullptr;
}

// `rows` boxes of {cx, cy, half_x, half_y, yaw}, `per_step` of them per step of a schedule: half extents > 0 and -- where the
// setter asks for it (`finite`; pocs_set_obstacles never has) -- every value finite.
static int check_boxes(pocs_ctx* c, const char* what, const double* boxes, size_t rows, size_t per_step, bool finite) {
  for (size_t i = 0; i < rows; ++i) {
    const double* b = boxes + 5 * i;
    const int step = (int)(i / per_step), m = (int)(i % per_step);
    for (int j = 0; finite && j < 5; ++j)
      if (!std::isfinite(b[j])) return fail(c, POCS_E_ARG, "%s: step %d, box %d: value %d is not finite", what, step, m, j);
    if (!(b[2] > 0) || !(b[3] > 0)) return fail(c, POCS_E_ARG, "%s: step %d, box %d: half extents must be > 0", what, step, m);
  }
  return POCS_OK;
}

// A vector getter's tail: POCS_E_BUFFER when the caller's `cap` elements do not hold the `n` there are, else the copy and n.
template <class T>
static int copy_out(pocs_ctx* c, T* out, int cap, const T* src, size_t n, const char* unit) {
  if ((long long)n > (long long)cap) return fail(c, POCS_E_BUFFER, "need %zu %s", n, unit);
  if (n) memcpy(out, src, n * sizeof(T));
  return (int)n;
}
template <class T>
static int copy_out(pocs_ctx* c, T* out, int cap, const std::vector<T>& v, const char* unit) { return copy_out(c, out, cap, v.data(), v.size(), unit); }
// ... of the two per-run getters: after an internal run-ahead batch the caller asked for one run at a time, and gets that one.
template <class T>
static int batch_out(pocs_ctx* c, T* out, int cap, const std::vector<T>& v, const char* unit) {
  if (!c->ra_internal) return copy_out(c, out, cap, v, unit);
  if (cap < 1 || v.empty()) return fail(c, POCS_E_BUFFER, "need 1 %s", unit);
  out[0] = v[(size_t)c->res.view];
  return 1;
}

// The collision world in force: `steps` tables of `small` boxes each in the table every kernel stages, OR a large world of `large` boxes
// beside it (the staged table is then empty); each gives way to the other.
static int install_world(pocs_ctx* c, const double* boxes, size_t small, int steps, size_t large) {
  c->boxes.assign(boxes, boxes + (size_t)steps * small * 5);
  c->world.assign(boxes, boxes + large * 5);
  c->world_S = steps;
  c->have_obstacles = true;
  c->env_dirty = true;
  return POCS_OK;
}

// ---- the run-ahead front ----
// run* with run-ahead: serve the next cached run, or evaluate the next `run_ahead` runs at once.
static bool ra_can_serve(const pocs_ctx* c, Kind kind) {
  return c->ra_have > 0 && c->ra_kind == kind && c->batch == 1 && c->res.view + 1 < c->ra_have;
}
// Runs evaluated per launch when run-ahead is on.  0 (automatic): enough runs to keep the chip busy for the
// launch's fixed cost to fade -- 1.6 x 10^7 mixture samples or 8 x 10^6 particles (what stays in the
// Infinity Cache between two waypoint launches) per launch, at least 8, at most 64: the reference's
// own 200 runs of 10^4 samples go 64 at a time, a 10^6-sample estimation 16 at a time.
static int ra_depth(const pocs_ctx* c, Kind kind) {
  if (c->run_ahead != 0) return c->run_ahead;
  const long long n = kind == Kind::Gmm ? c->num_gmm : c->num_particles;
  const long long want = (kind == Kind::Gmm ? 16000000LL : 8000000LL) / (n > 0 ? n : 1);
  return (int)(want < 8 ? 8 : want > 64 ? 64 : want);
}
static bool ra_wanted(const pocs_ctx* c, Kind kind) {
  using namespace pocs_modes;
  return ra_depth(c, kind) > 1 && c->batch == 1 && !c->opt_profile && !in_mode(c, kPlans | kTree | kShard | kMoments | kSequence);
}
// The front of every run* call: serve the next cached run of `kind` (`ahead`: the call takes part in run-ahead), or drop what is
// cached, size the launch, make it (`run`) and remember what it left; res.view is then the run the call hands out.
template <class Run>
static int ra_front(pocs_ctx* c, Kind kind, bool ahead, Run run) {
  HIPCHK(c, hipSetDevice(c->device));
  if (ahead && ra_can_serve(c, kind)) {
    if (kind == Kind::Gmm) gmm_select_view(c, c->res.view + 1); else c->res.view += 1;
    return POCS_OK;
  }
  ra_drop(c);
  c->ra_internal = false;
  const int depth = ahead && ra_wanted(c, kind) ? ra_depth(c, kind) : 0;
  if (depth) c->batch = depth;
  const int rc = run();
  if (depth) c->batch = 1;
  if (rc == POCS_OK && depth) { c->ra_have = depth; c->ra_kind = kind; c->ra_internal = true; }
  return rc;
}
static void mc_fill_probs(pocs_ctx* c) {
  // getCollisionProportion, MCSimulator.h:324-330 (of the particles this context evaluated)
  const double den = (double)(c->res.last_mc_count > 0 ? c->res.last_mc_count : 1);
  c->res.batch_probs.assign(c->res.mc_counts.size(), 0.0);
  for (size_t r = 0; r < c->res.mc_counts.size(); ++r) c->res.batch_probs[r] = (double)c->res.mc_counts[r] / den;
}

extern "C" {

const char* pocs_version(void) { return POCS_VERSION_STRING; }

int pocs_create(pocs_ctx** out, int device) {
  if (!out) return POCS_E_ARG;
  *out = nullptr;
  pocs_ctx* c = new (std::nothrow) pocs_ctx();
  if (!c) return POCS_E_ARG;
  *out = c;        // returned even on failure so the caller can read pocs_last_error
  memset(&c->sensor, 0, sizeof c->sensor);
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(c, POCS_E_DEVICE, "no HIP device available (%s); libpocs has no CPU path",
                e != hipSuccess ? hipGetErrorString(e) : "device count 0");
  if (device < 0 || device >= n) return fail(c, POCS_E_ARG, "device %d out of range (0..%d)", device, n - 1);
  c->device = device;
  HIPCHK(c, hipSetDevice(device));
  HIPCHK(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
  c->stream = c->own_stream;
  for (int g = 0; g < 3; ++g) {
    HIPCHK(c, hipStreamCreateWithFlags(&c->side_stream[g], hipStreamNonBlocking));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_join[g], hipEventDisableTiming));
  }
  HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  HIPCHK(c, hipEventCreate(&c->ev_seq[0]));
  HIPCHK(c, hipEventCreate(&c->ev_seq[1]));
  return POCS_OK;
}

#if defined(POCS_TUNING) && defined(POCS_STAMPS)
void pocs_stamps_report();
#endif
void pocs_destroy(pocs_ctx* c) {
  if (!c) return;
#if defined(POCS_TUNING) && defined(POCS_STAMPS)
  if (c->own_stream) { hipSetDevice(c->device); hipStreamSynchronize(c->stream); pocs_stamps_report(); }
#endif
  if (c->own_stream) {
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    drop_graphs(c);
    for (hipEvent_t e : c->events) hipEventDestroy(e);
    for (int g = 0; g < 3; ++g) {
      if (c->side_stream[g]) { hipStreamSynchronize(c->side_stream[g]); hipStreamDestroy(c->side_stream[g]); }
      if (c->ev_join[g]) hipEventDestroy(c->ev_join[g]);
    }
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    if (c->ev_seq[0]) hipEventDestroy(c->ev_seq[0]);
    if (c->ev_seq[1]) hipEventDestroy(c->ev_seq[1]);
    if (c->h_pin) hipHostFree(c->h_pin);
    if (c->h_copy) hipHostFree(c->h_copy);
    for (int q = 0; q < POCS_XCHG_MAX_WORLD; ++q)
      if (c->xchg_peer[q] && c->xchg_peer[q] != c->xchg_own) (void)hipIpcCloseMemHandle(c->xchg_peer[q]);
    if (c->xchg_own) (void)hipFree(c->xchg_own);
    hipStreamDestroy(c->own_stream);
  }
  delete c;                                          // (every DevBuf frees itself: the device is selected above)
}

const char* pocs_last_error(const pocs_ctx* c) { return c ? c->err.c_str() : "null context"; }

int pocs_set_footprint(pocs_ctx* c, double dx, double dy, double hx, double hy) {
  if (!setter(c)) return POCS_E_ARG;
  if (!(hx > 0) || !(hy > 0)) return fail(c, POCS_E_ARG, "footprint half extents must be > 0");
  c->fp.dx = dx; c->fp.dy = dy; c->fp.hx = hx; c->fp.hy = hy;
  c->fp_F = 1; c->fp_parts[0] = c->fp;               // (a compound footprint is replaced by the single box)
  c->fp_round = false; c->fp_rho = 0.0;              // (and so is a round one)
  c->env_dirty = true;
  return POCS_OK;
}

// ---- a round footprint (include/pocs.h) ----
int pocs_set_footprint_disc(pocs_ctx* c, double radius) {
  if (!setter(c)) return POCS_E_ARG;
  if (!std::isfinite(radius) || radius < 0) return fail(c, POCS_E_ARG, "pocs_set_footprint_disc: the radius must be finite and >= 0");
  // (not a mode of the table: the one mask of what a round footprint excludes, pocs_modes.hpp, and segment checks beside it)
  unsigned in_the_way = modes_of(c) & pocs_modes::kRoundFpExcluded;
  if (in_the_way) {                                  // names ONE mode: the open sequence before all others, a connected exchange before its buffer
    const bool open = (in_the_way & pocs_modes::kSequence) != 0;
    if (open) in_the_way = pocs_modes::kSequence;
    if (in_the_way & pocs_modes::kXchgConnected) in_the_way &= ~(unsigned)pocs_modes::kXchgCreated;
    return fail(c, open ? POCS_E_ORDER : POCS_E_STATE, "pocs_set_footprint_disc: %s; %s",
                pocs_modes::name((pocs_modes::Mode)(in_the_way & (0u - in_the_way))), pocs_modes::kRoundFpClause);
  }
  if (seg_applied(c))
    return fail(c, POCS_E_STATE, "pocs_set_footprint_disc: segment checks are set (pocs_set_segment_checks); %s", pocs_modes::kRoundFpClause);
  if (hyp_applied(c))
    return fail(c, POCS_E_STATE, "pocs_set_footprint_disc: prediction hypotheses are set (pocs_set_disc_hypotheses); hypotheses are served under a footprint box");
  const double rho = radius == 0.0 ? 0.0 : radius;   // (a point robot: +0.0)
  c->fp = pocs_footprint{0.0, 0.0, rho, rho};        // the bounding square: what pocs_get_footprint_parts reports
  c->fp_F = 1; c->fp_parts[0] = c->fp;               // (a compound footprint is replaced)
  c->fp_round = true; c->fp_rho = rho;
  c->env_dirty = true;
  return POCS_OK;
}

int pocs_get_footprint_disc(const pocs_ctx* c, double* radius) {
  if (!c) return POCS_E_ARG;
  if (!rfoot_applied(c)) return 0;
  if (radius) *radius = c->fp_rho;
  return 1;
}

// ---- compound footprints (include/pocs.h) ----
int pocs_set_footprint_parts(pocs_ctx* c, const double* parts, int F) {
  if (!setter(c)) return POCS_E_ARG;
  if (!parts || F < 1 || F > POCS_MAX_FOOTPRINT_PARTS)
    return fail(c, POCS_E_ARG, "pocs_set_footprint_parts: %d parts outside 1..%d (or null parts)", F, POCS_MAX_FOOTPRINT_PARTS);
  for (int j = 0; j < 4 * F; ++j)
    if (!std::isfinite(parts[j])) return fail(c, POCS_E_ARG, "pocs_set_footprint_parts: part %d: value %d is not finite", j / 4, j % 4);
  for (int f = 0; f < F; ++f)
    if (!(parts[4 * f + 2] > 0) || !(parts[4 * f + 3] > 0)) return fail(c, POCS_E_ARG, "pocs_set_footprint_parts: part %d: half extents must be > 0", f);
  if (F == 1) return pocs_set_footprint(c, parts[0], parts[1], parts[2], parts[3]);
  // (not a mode of the table: the one mask of what a compound footprint excludes, pocs_modes.hpp)
  unsigned in_the_way = modes_of(c) & pocs_modes::kPartsExcluded;
  if (in_the_way) {                                  // names ONE mode: the open sequence before all others, a connected exchange before its buffer
    const bool open = (in_the_way & pocs_modes::kSequence) != 0;
    if (open) in_the_way = pocs_modes::kSequence;
    if (in_the_way & pocs_modes::kXchgConnected) in_the_way &= ~(unsigned)pocs_modes::kXchgCreated;
    return fail(c, open ? POCS_E_ORDER : POCS_E_STATE, "pocs_set_footprint_parts: %s; %s",
                pocs_modes::name((pocs_modes::Mode)(in_the_way & (0u - in_the_way))), pocs_modes::kPartsClause);
  }
  if (seg_applied(c))                                // (the segment forms test a single box: refused in both directions)
    return fail(c, POCS_E_STATE, "pocs_set_footprint_parts: segment checks are set (pocs_set_segment_checks); %s", pocs_modes::kSegClause);
  if (discs_applied(c))                              // (so do the round forms)
    return fail(c, POCS_E_STATE, "pocs_set_footprint_parts: discs are set (pocs_set_discs); %s", pocs_modes::kDiscClause);
  for (int f = 0; f < F; ++f) c->fp_parts[f] = pocs_footprint{parts[4 * f], parts[4 * f + 1], parts[4 * f + 2], parts[4 * f + 3]};
  c->fp_F = F;
  c->fp_round = false; c->fp_rho = 0.0;              // (a round footprint is replaced)
  c->fp = c->fp_parts[0];
  c->env_dirty = true;
  return POCS_OK;
}

int pocs_get_footprint_parts(const pocs_ctx* c, double* parts, int cap) {
  if (!c || !parts) return POCS_E_ARG;
  if (cap < c->fp_F) return POCS_E_BUFFER;
  for (int f = 0; f < c->fp_F; ++f) {
    const pocs_footprint& q = c->fp_F > 1 ? c->fp_parts[f] : c->fp;
    parts[4 * f] = q.dx; parts[4 * f + 1] = q.dy; parts[4 * f + 2] = q.hx; parts[4 * f + 3] = q.hy;
  }
  return c->fp_F;
}

int pocs_set_obstacles(pocs_ctx* c, const double* boxes, int M) {
  if (!setter(c)) return POCS_E_ARG;
  if (M < 0 || M > POCS_MAX_OBSTACLES || (M > 0 && !boxes))
    return fail(c, POCS_E_ARG, "obstacle count %d outside 0..%d", M, POCS_MAX_OBSTACLES);
  if (M + c->disc_D > POCS_MAX_OBSTACLES)            // (boxes and discs share the table of POCS_MAX_OBSTACLES records)
    return fail(c, POCS_E_ARG, "%d boxes beside %d discs (pocs_set_discs): more than %d records", M, c->disc_D, POCS_MAX_OBSTACLES);
  if (int r = check_boxes(c, "obstacles", boxes, (size_t)M, (size_t)M, false)) return r;
  return install_world(c, boxes, (size_t)M, 1, 0);
}

// The obstacle schedule: S worlds of M boxes each, world s the collision world at waypoint s (upload_world prepares one
// record per step; every launch takes the record of its waypoint: world_at).  S = 1 is pocs_set_obstacles.
int pocs_set_obstacle_schedule(pocs_ctx* c, const double* boxes, int M, int S) {
  if (!setter(c)) return POCS_E_ARG;
  if (M < 0 || M > POCS_MAX_OBSTACLES) return fail(c, POCS_E_ARG, "obstacle count %d outside 0..%d", M, POCS_MAX_OBSTACLES);
  if (S == 0 && M == 0) return pocs_set_obstacles(c, nullptr, 0);      // no schedule, an explicitly empty world
  if (S < 1 || S > POCS_MAX_WORLD_STEPS) return fail(c, POCS_E_ARG, "obstacle schedule of %d steps outside 1..%d", S, POCS_MAX_WORLD_STEPS);
  if (M > 0 && !boxes) return fail(c, POCS_E_ARG, "obstacle schedule: null boxes");
  if (M + c->disc_D > POCS_MAX_OBSTACLES)
    return fail(c, POCS_E_ARG, "obstacle schedule: %d boxes beside %d discs (pocs_set_discs): more than %d records", M, c->disc_D, POCS_MAX_OBSTACLES);
  if (int r = check_boxes(c, "obstacle schedule", boxes, (size_t)S * (size_t)M, (size_t)M, true)) return r;
  return install_world(c, boxes, (size_t)M, S, 0);
}

int pocs_get_world_steps(const pocs_ctx* c) { return (c && (c->have_obstacles || discs_applied(c))) ? env_steps(c) : 0; }      // (max(Sb, Sd) under discs)

// ---- round obstacles (include/pocs.h) ----
// S tables of D discs {cx, cy, r}; upload_world composes them with the boxes' steps into the env records.  D = 0 clears.
int pocs_set_discs(pocs_ctx* c, const double* discs, int D, int S) {
  if (!setter(c)) return POCS_E_ARG;
  if (D < 0 || D > POCS_MAX_OBSTACLES) return fail(c, POCS_E_ARG, "pocs_set_discs: %d discs outside 0..%d", D, POCS_MAX_OBSTACLES);
  if (D == 0 || (S == 0 && !discs)) {                // clears: every call is again what it is without discs
    if (c->disc_D > 0) c->env_dirty = true;
    c->discs.clear(); c->disc_D = 0; c->disc_S = 1;
    c->disc_cov.clear(); c->disc_noise_persistent = 0;      // (covariances need discs)
    c->hyp_group.clear(); c->hyp_weight.clear();            // (and so do hypotheses)
    return POCS_OK;
  }
  if (S < 1 || S > POCS_MAX_WORLD_STEPS) return fail(c, POCS_E_ARG, "pocs_set_discs: %d steps outside 1..%d", S, POCS_MAX_WORLD_STEPS);
  if (!discs) return fail(c, POCS_E_ARG, "pocs_set_discs: null discs");
  const int M = large_world(c) ? 0 : world_boxes(c);
  if (M + D > POCS_MAX_OBSTACLES)
    return fail(c, POCS_E_ARG, "pocs_set_discs: %d discs beside %d boxes: more than %d records", D, M, POCS_MAX_OBSTACLES);
  for (size_t i = 0; i < (size_t)S * (size_t)D; ++i) {
    const double* d = discs + 3 * i;
    for (int j = 0; j < 3; ++j)
      if (!std::isfinite(d[j])) return fail(c, POCS_E_ARG, "pocs_set_discs: step %d, disc %d: value %d is not finite", (int)(i / (size_t)D), (int)(i % (size_t)D), j);
    if (!(d[2] > 0)) return fail(c, POCS_E_ARG, "pocs_set_discs: step %d, disc %d: the radius must be > 0", (int)(i / (size_t)D), (int)(i % (size_t)D));
  }
  // (not a mode of the table: the one mask of what discs exclude, pocs_modes.hpp, and a compound footprint and segment checks beside it)
  unsigned in_the_way = modes_of(c) & pocs_modes::kDiscExcluded;
  if (in_the_way) {                                  // names ONE mode: the open sequence before all others, a connected exchange before its buffer
    const bool open = (in_the_way & pocs_modes::kSequence) != 0;
    if (open) in_the_way = pocs_modes::kSequence;
    if (in_the_way & pocs_modes::kXchgConnected) in_the_way &= ~(unsigned)pocs_modes::kXchgCreated;
    return fail(c, open ? POCS_E_ORDER : POCS_E_STATE, "pocs_set_discs: %s; %s",
                pocs_modes::name((pocs_modes::Mode)(in_the_way & (0u - in_the_way))), pocs_modes::kDiscClause);
  }
  if (parts_applied(c))
    return fail(c, POCS_E_STATE, "pocs_set_discs: a compound footprint is set (pocs_set_footprint_parts); %s", pocs_modes::kDiscClause);
  if (seg_applied(c))
    return fail(c, POCS_E_STATE, "pocs_set_discs: segment checks are set (pocs_set_segment_checks); %s", pocs_modes::kDiscClause);
  c->discs.assign(discs, discs + (size_t)S * (size_t)D * 3);
  if (D != c->disc_D || S != c->disc_S) { c->disc_cov.clear(); c->disc_noise_persistent = 0; }      // (the same D and S keep the covariances: new predictions, the same fan)
  if (D != c->disc_D) { c->hyp_group.clear(); c->hyp_weight.clear(); }      // (the same D keeps the hypotheses, whatever S is: an alternative is a whole track)
  c->disc_D = D; c->disc_S = S;
  c->env_dirty = true;                               // (same D and S: the records are overwritten in place and the cached graph replays)
  return POCS_OK;
}

// ---- prediction hypotheses (include/pocs.h) ----
// A group and a weight per disc in force; upload_world turns them into the records' gates.
int pocs_set_disc_hypotheses(pocs_ctx* c, const int* group, const double* weight, int D) {
  if (!setter(c)) return POCS_E_ARG;
  if (modes_of(c) & pocs_modes::kSequence)
    return fail(c, POCS_E_ORDER, "pocs_set_disc_hypotheses: %s; %s", pocs_modes::name(pocs_modes::kSequence), pocs_modes::kDiscClause);
  if ((!group || !weight) && D == 0) {               // clears: every call is again the call it is without hypotheses
    if (!c->hyp_group.empty()) c->env_dirty = true;
    c->hyp_group.clear(); c->hyp_weight.clear();
    return POCS_OK;
  }
  if (!discs_applied(c)) return fail(c, POCS_E_STATE, "pocs_set_disc_hypotheses: no discs are set (pocs_set_discs): hypotheses belong to discs");
  if (rfoot_applied(c))
    return fail(c, POCS_E_STATE, "pocs_set_disc_hypotheses: a round footprint is set (pocs_set_footprint_disc); hypotheses are served under a footprint box");
  if (D != c->disc_D) return fail(c, POCS_E_ARG, "pocs_set_disc_hypotheses: %d discs, the discs in force are %d", D, c->disc_D);
  if (!group || !weight) return fail(c, POCS_E_ARG, "pocs_set_disc_hypotheses: null %s", !group ? "groups" : "weights");
  std::vector<unsigned long long> lo((size_t)D), hi((size_t)D);
  int bad = 0;
  if (const int k = pocs_hyp_thresholds(group, weight, D, lo.data(), hi.data(), &bad))
    return fail(c, POCS_E_ARG, "pocs_set_disc_hypotheses: disc %d (group %d, weight %g): %s", bad, group[bad], weight[bad], hyp_refusal(k));
  bool any = false;
  for (int d = 0; d < D; ++d) any = any || group[d] >= 0;
  if (any) {
    c->hyp_group.assign(group, group + D);
    c->hyp_weight.assign(weight, weight + D);
    for (int d = 0; d < D; ++d)
      if (group[d] < 0) c->hyp_weight[(size_t)d] = 1.0;      // (not read: what the getter hands back for a disc that is always there)
  } else {                                           // (all groups -1 is the same as cleared)
    c->hyp_group.clear(); c->hyp_weight.clear();
  }
  c->env_dirty = true;                               // (the same D: the gates are overwritten in place and the cached graph replays)
  return POCS_OK;
}

int pocs_get_disc_hypotheses(const pocs_ctx* c, int* group, double* weight, unsigned long long* lo, unsigned long long* hi, int cap) {
  if (!c) return POCS_E_ARG;
  if (!hyp_applied(c)) return 0;
  const int D = c->disc_D;
  if (D > cap) return POCS_E_BUFFER;
  std::vector<unsigned long long> l((size_t)D), h((size_t)D);
  int bad = 0;
  pocs_hyp_thresholds(c->hyp_group.data(), c->hyp_weight.data(), D, l.data(), h.data(), &bad);
  for (int d = 0; d < D; ++d) {
    if (group) group[d] = c->hyp_group[(size_t)d];
    if (weight) weight[d] = c->hyp_weight[(size_t)d];
    if (lo) lo[d] = l[(size_t)d];
    if (hi) hi[d] = h[(size_t)d];
  }
  return D;
}

// ---- uncertain discs (include/pocs.h) ----
// S x D covariances {sxx, sxy, syy} for the discs in force; upload_world factorises them into the noise rows and grows the records.
int pocs_set_disc_covariances(pocs_ctx* c, const double* cov, int D, int S, int persistent) {
  if (!setter(c)) return POCS_E_ARG;
  if (modes_of(c) & pocs_modes::kSequence)
    return fail(c, POCS_E_ORDER, "pocs_set_disc_covariances: %s; %s", pocs_modes::name(pocs_modes::kSequence), pocs_modes::kDiscClause);
  if (!cov && D == 0) {                              // clears: every call is again the discs call it is without covariances
    if (!c->disc_cov.empty()) c->env_dirty = true;
    c->disc_cov.clear(); c->disc_noise_persistent = 0;
    return POCS_OK;
  }
  if (!discs_applied(c)) return fail(c, POCS_E_STATE, "pocs_set_disc_covariances: no discs are set (pocs_set_discs): covariances belong to discs");
  if (!cov) return fail(c, POCS_E_ARG, "pocs_set_disc_covariances: null covariances");
  if (D != c->disc_D || S != c->disc_S)
    return fail(c, POCS_E_ARG, "pocs_set_disc_covariances: %d discs over %d steps, the discs in force are %d over %d", D, S, c->disc_D, c->disc_S);
  if (persistent != POCS_DISC_NOISE_PER_WAYPOINT && persistent != POCS_DISC_NOISE_PERSISTENT)
    return fail(c, POCS_E_ARG, "pocs_set_disc_covariances: persistent is %d, POCS_DISC_NOISE_PER_WAYPOINT (0) or POCS_DISC_NOISE_PERSISTENT (1)", persistent);
  bool any = false;
  for (size_t i = 0; i < (size_t)S * (size_t)D; ++i) {
    double row[3];
    const int k = pocs_disc_noise_factor(cov + 3 * i, row);
    if (k < 0)
      return fail(c, POCS_E_ARG, "pocs_set_disc_covariances: step %d, disc %d: {%g, %g, %g} is neither zeros nor a finite covariance with sxx > 0 and syy - sxy^2 / sxx > 0",
                  (int)(i / (size_t)D), (int)(i % (size_t)D), cov[3 * i], cov[3 * i + 1], cov[3 * i + 2]);
    any = any || k == 0;
  }
  if (any) c->disc_cov.assign(cov, cov + (size_t)S * (size_t)D * 3);      // (all rows zero is the same as cleared)
  else c->disc_cov.clear();
  c->disc_noise_persistent = any ? persistent : 0;
  c->env_dirty = true;                               // (the same shape: rows and records are overwritten in place and the cached graph replays)
  return POCS_OK;
}

int pocs_get_disc_covariances(const pocs_ctx* c, double* out, int cap, int* persistent) {
  if (!c) return POCS_E_ARG;
  if (persistent) *persistent = c->disc_noise_persistent;
  const size_t n = noise_applied(c) ? c->disc_cov.size() : 0;
  if (n == 0) return 0;
  if (!out || (long long)n > (long long)cap) return POCS_E_BUFFER;
  memcpy(out, c->disc_cov.data(), n * sizeof(double));
  return (int)n;
}

int pocs_get_discs(const pocs_ctx* c, int* D, int* S) {
  if (!c) return POCS_E_ARG;
  if (D) *D = c->disc_D;
  if (S) *S = c->disc_D > 0 ? c->disc_S : 0;
  return POCS_OK;
}

// A static world of up to POCS_MAX_WORLD_BOXES boxes.  Up to POCS_MAX_OBSTACLES it IS pocs_set_obstacles; above, the boxes are kept
// apart from the staged table (which is then empty): upload_world prepares their records, the GMM launches get a cull launch in
// front of each waypoint and the _world forms of the sampling kernel, the MC launches the _world forms of theirs.
int pocs_set_world(pocs_ctx* c, const double* boxes, int M) {
  if (!setter(c)) return POCS_E_ARG;
  if (M < 0 || M > POCS_MAX_WORLD_BOXES || (M > 0 && !boxes))
    return fail(c, POCS_E_ARG, "world of %d boxes outside 0..%d (or null boxes)", M, POCS_MAX_WORLD_BOXES);
  if (M <= POCS_MAX_OBSTACLES) return pocs_set_obstacles(c, boxes, M);
  if (int r = check_boxes(c, "world", boxes, (size_t)M, (size_t)M, true)) return r;
  if (int r = may_enter(c, "pocs_set_world with more than 64 boxes", pocs_modes::kLargeWorld)) return r;
  return install_world(c, boxes, 0, 1, (size_t)M);
}

int pocs_get_world_boxes(const pocs_ctx* c) {
  if (!c || !c->have_obstacles) return 0;
  return large_world(c) ? large_boxes(c) : world_boxes(c);
}

int pocs_get_world_reach(pocs_ctx* c, int* out, int cap) {
  if (!c || !out) return POCS_E_ARG;
  if (c->reach_R < 1 || c->reach.empty())
    return fail(c, POCS_E_STATE, "pocs_get_world_reach: the last GMM call did not run under a large world (pocs_set_world with more than %d boxes)", POCS_MAX_OBSTACLES);
  const size_t r = c->res.view >= 0 && c->res.view < c->reach_R ? (size_t)c->res.view : 0;
  return copy_out(c, out, cap, &c->reach[r * (size_t)c->reach_W], (size_t)c->reach_len[r], "ints");
}

int pocs_set_alphas(pocs_ctx* c, const double* a, int n) {
  if (!setter(c)) return POCS_E_ARG;
  if (n < 1 || n > 4 || !a) return fail(c, POCS_E_ARG, "setAlphas takes 1..4 values (got %d)", n);
  for (int i = 0; i < n; ++i) c->alphas[i] = a[i];
  c->have_alphas = true;
  return POCS_OK;
}

int pocs_set_q(pocs_ctx* c, double q) {
  if (!setter(c)) return POCS_E_ARG;
  if (!(q >= 0)) return fail(c, POCS_E_ARG, "Q must be >= 0");
  c->sensor.Q = q; c->have_q = true; c->sensor_dirty = true;
  return POCS_OK;
}

int pocs_set_num_landmarks(pocs_ctx* c, int n) {
  if (!setter(c)) return POCS_E_ARG;
  if (n < 0 || n > POCS_MAX_LANDMARKS) return fail(c, POCS_E_ARG, "numLandmarks %d outside 0..%d", n, POCS_MAX_LANDMARKS);
  c->num_landmarks = n; c->have_landmarks = false;
  return POCS_OK;
}

int pocs_set_landmarks(pocs_ctx* c, const double* xy, int n) {
  if (!setter(c)) return POCS_E_ARG;
  if (c->num_landmarks < 0) return fail(c, POCS_E_ORDER, "setLandmarks before setNumLandmarks");
  if (n != c->num_landmarks || (n > 0 && !xy)) return fail(c, POCS_E_ARG, "setLandmarks needs 2*%d values", c->num_landmarks);
  c->sensor.L = n;
  for (int i = 0; i < n; ++i) { c->sensor.lx[i] = xy[i]; c->sensor.ly[i] = xy[n + i]; }
  c->have_landmarks = true; c->sensor_dirty = true;
  return POCS_OK;
}

int pocs_set_num_particles(pocs_ctx* c, long long n) {
  if (!setter(c)) return POCS_E_ARG;
  if (n < 1) return fail(c, POCS_E_ARG, "numParticles must be >= 1");
  c->num_particles = n;
  return POCS_OK;
}

int pocs_set_initial_covariance(pocs_ctx* c, const double* m9) {
  if (!setter(c) || !m9) return POCS_E_ARG;
  memcpy(c->cov0, m9, 9 * sizeof(double));
  c->have_cov0 = true;
  return POCS_OK;
}

int pocs_set_path_length(pocs_ctx* c, int W) {
  if (!setter(c)) return POCS_E_ARG;
  if (int r = may_enter(c, "pocs_set_path_length", pocs_modes::kSinglePlan)) return r;
  if (W < 1) return fail(c, POCS_E_ARG, "pathLength must be >= 1");
  if (W != c->W) { c->have_traj = false; c->have_odom = false; }
  c->W = W;
  return POCS_OK;
}

int pocs_set_trajectory(pocs_ctx* c, const double* v, int W) {
  if (!setter(c)) return POCS_E_ARG;
  if (int r = may_enter(c, "pocs_set_trajectory", pocs_modes::kSinglePlan)) return r;
  if (c->W < 1) return fail(c, POCS_E_ORDER, "setTrajectory before setPathLength");
  if (W != c->W || !v) return fail(c, POCS_E_ARG, "setTrajectory needs 3*%d values", c->W);
  c->traj.assign(v, v + (size_t)3 * W);
  c->have_traj = true;
  return POCS_OK;
}

int pocs_set_odometry(pocs_ctx* c, const double* v, int Wm1) {
  if (!setter(c)) return POCS_E_ARG;
  if (int r = may_enter(c, "pocs_set_odometry", pocs_modes::kSinglePlan)) return r;
  if (c->W < 1) return fail(c, POCS_E_ORDER, "setOdometry before setPathLength");
  if (Wm1 != c->W - 1 || (Wm1 > 0 && !v)) return fail(c, POCS_E_ARG, "setOdometry needs 3*%d values", c->W - 1);
  c->odom.assign(v, v + (size_t)3 * Wm1);
  c->have_odom = true;
  return POCS_OK;
}

int pocs_set_num_gaussians(pocs_ctx* c, int K) {
  if (!setter(c)) return POCS_E_ARG;
  if (K < 1 || K > POCS_MAX_GAUSSIANS) return fail(c, POCS_E_ARG, "numGaussians %d outside 1..%d", K, POCS_MAX_GAUSSIANS);
  c->K = K;
  return POCS_OK;
}

int pocs_set_num_gmm_samples(pocs_ctx* c, long long n) {
  if (!setter(c)) return POCS_E_ARG;
  if (n < 1) return fail(c, POCS_E_ARG, "numGMMSamples must be >= 1");
  c->num_gmm = n;
  return POCS_OK;
}

int pocs_set_seed(pocs_ctx* c, uint64_t seed) {
  if (!setter(c)) return POCS_E_ARG;
  c->seed = seed; c->run_index = 0;
  return POCS_OK;
}

int pocs_set_option(pocs_ctx* c, int option, long long value) {
  if (!setter(c)) return POCS_E_ARG;
  switch (option) {
    case POCS_OPT_STORE_SAMPLES: c->opt_store = value ? 1 : 0; break;
    case POCS_OPT_MC_FUSED:
      if (value) if (int r = may_enter(c, "POCS_OPT_MC_FUSED = 1", pocs_modes::kFused)) return r;
      c->opt_fused = value ? 1 : 0;
      break;
    case POCS_OPT_USE_GRAPH: c->opt_graph = value ? 1 : 0; break;
    case POCS_OPT_PROFILE:
      if (value < 0 || value > 2) return fail(c, POCS_E_ARG, "POCS_OPT_PROFILE takes 0, 1 or 2");
      c->opt_profile = value;
      break;
    case POCS_OPT_PERSISTENT:
      // the queue-driven whole-call kernel (k_gmm_run) of round 2 was retired in round 3: slower than one launch per
      // waypoint at every batch size measured, and not worth a second summation shape
      if (value) return fail(c, POCS_E_ARG, "POCS_OPT_PERSISTENT: the queue-driven kernel has been retired (DESIGN.md section 5)");
      break;
    case POCS_OPT_LONE_CALL: c->opt_lone = value ? 1 : 0; break;
    case POCS_OPT_SUB_BATCHES:
      if (value < 0 || value > 2) return fail(c, POCS_E_ARG, "sub-batches %lld outside 0..2 (0 = by the call's size; three lost, four gained less than two: DESIGN.md section 5)", value);
      c->opt_groups = value;
      break;
    case POCS_OPT_MC_NONTEMPORAL:
      if (value < -1 || value > 1) return fail(c, POCS_E_ARG, "POCS_OPT_MC_NONTEMPORAL takes -1 (by size), 0 or 1");
      c->opt_mc_nt = value;
      break;
    case POCS_OPT_PLAN_SEEDS:
      if (value < 0 || value > 1) return fail(c, POCS_E_ARG, "POCS_OPT_PLAN_SEEDS takes 0 (plan p draws run p's stream) or 1 (common random numbers)");
      c->opt_plan_seeds = value;
      break;
    case POCS_OPT_MC_WAYPOINT_COUNTS:
      if (value < 0 || value > 1) return fail(c, POCS_E_ARG, "POCS_OPT_MC_WAYPOINT_COUNTS takes 0 or 1");
      c->opt_mc_wp = value;
      break;
    case POCS_OPT_MC_RISK_BOUND:
      if (value < 0 || value > 1) return fail(c, POCS_E_ARG, "POCS_OPT_MC_RISK_BOUND takes 0 (MC calls ignore the risk bound) or 1");
      c->opt_mc_rb = value;
      break;
    case POCS_OPT_OBSTACLE_COUNTS:
      if (value < 0 || value > 1) return fail(c, POCS_E_ARG, "POCS_OPT_OBSTACLE_COUNTS takes 0 or 1");
      // (inside a sequence the option is not touched at all, whatever the value)
      if (int r = may_enter(c, "POCS_OPT_OBSTACLE_COUNTS", pocs_modes::kObsCounts, value ? pocs_modes::kAll : pocs_modes::kSequence)) return r;
      c->opt_obs_counts = value;
      c->res.oc_kind = Kind::None;                           // (a table is served until the option is touched or the next call)
      break;
    case POCS_OPT_RUN_AHEAD:
      if (value < 0 || value > 256) return fail(c, POCS_E_ARG, "run-ahead %lld outside 0..256", value);
      c->run_ahead = (int)value;                     // 0 = sized per call (ra_depth)
      break;
    default: return fail(c, POCS_E_ARG, "unknown option %d", option);
  }
  return POCS_OK;
}

int pocs_set_batch(pocs_ctx* c, int runs) {
  if (!setter(c)) return POCS_E_ARG;
  if (int r = may_enter(c, "pocs_set_batch", pocs_modes::kSinglePlan)) return r;
  if (runs < 1 || runs > 256) return fail(c, POCS_E_ARG, "batch %d outside 1..256", runs);
  if (int r = may_enter(c, "pocs_set_batch", pocs_modes::kBatch)) return r;
  c->batch = runs;
  return POCS_OK;
}

// A set of plans or a tree takes the context's W and batch over (W: the stride of every [run][W] array; batch: the plans or
// the nodes); the single plan's wait for leave_multi.  The results of the last launch refer to the plans (or the plan) it
// evaluated: entering and leaving drop them.
static void enter_multi(pocs_ctx* c, int W, int batch) {
  if (!in_mode(c, pocs_modes::kPlans | pocs_modes::kTree)) { c->single_W = c->W; c->single_batch = c->batch; }
  c->W = W; c->batch = batch;
  reset_results(c);
}
static void leave_multi(pocs_ctx* c) {
  c->W = c->single_W; c->batch = c->single_batch;
  reset_results(c);
}

int pocs_set_plans(pocs_ctx* c, int P, const int* W, const double* trajs, const double* odoms) {
  if (!setter(c)) return POCS_E_ARG;
  if (int r = may_enter(c, "pocs_set_plans", pocs_modes::kPlans, pocs_modes::kSequence)) return r;      // (P = 0 too)
  if (P < 0 || P > 256) return fail(c, POCS_E_ARG, "plans: P = %d outside 0..256", P);
  if (P == 0) {                                      // back to the single plan
    if (c->plans.n) { c->plans = PlanSet{}; leave_multi(c); }
    return POCS_OK;
  }
  if (int r = may_enter(c, "pocs_set_plans", pocs_modes::kPlans, pocs_modes::kTree)) return r;
  if (!W || !trajs) return fail(c, POCS_E_ARG, "plans: null lengths or trajectories");
  size_t nt = 0, no = 0;
  int Wmax = 0;
  for (int p = 0; p < P; ++p) {
    if (W[p] < 1) return fail(c, POCS_E_ARG, "plans: plan %d has length %d (>= 1 needed)", p, W[p]);
    nt += 3 * (size_t)W[p]; no += 3 * (size_t)(W[p] - 1);
    Wmax = W[p] > Wmax ? W[p] : Wmax;
  }
  if (no > 0 && !odoms) return fail(c, POCS_E_ARG, "plans: null odometry");
  if (int r = may_enter(c, "pocs_set_plans", pocs_modes::kPlans)) return r;
  c->plans.W.assign(W, W + P);
  c->plans.toff.assign((size_t)P, 0); c->plans.ooff.assign((size_t)P, 0);
  for (int p = 1; p < P; ++p) {
    c->plans.toff[(size_t)p] = c->plans.toff[(size_t)p - 1] + 3 * (size_t)W[p - 1];
    c->plans.ooff[(size_t)p] = c->plans.ooff[(size_t)p - 1] + 3 * (size_t)(W[p - 1] - 1);
  }
  c->plans.traj.assign(trajs, trajs + nt);
  if (no > 0) c->plans.odom.assign(odoms, odoms + no); else c->plans.odom.clear();
  c->plans.odom.push_back(0.0);                       // (never read: keeps .data() of a set of one-waypoint plans non-null)
  enter_multi(c, Wmax, P);
  c->plans.n = P;
  return POCS_OK;
}

int pocs_set_plan_risk_bound(pocs_ctx* c, double bound) {
  if (!setter(c)) return POCS_E_ARG;
  if (!(bound > 0.0)) return fail(c, POCS_E_ARG, "risk bound %g: a probability in (0, 1), or >= 1 for none", bound);     // (NaN too)
  if (int r = may_enter(c, "pocs_set_plan_risk_bound", pocs_modes::kRiskBound)) return r;
  c->risk_bound = bound < 1.0 ? bound : 1.0;
  return POCS_OK;
}

int pocs_get_plan_evaluated(pocs_ctx* c, int* out, int cap) {
  if (!c || !out) return POCS_E_ARG;
  const Kind kind = c->res.last_kind;                    // (an MC call by default ignores the bound: every plan is driven to its end)
  if (!c->plans.n || kind == Kind::None || c->res.plan_slot(kind).empty() || (kind == Kind::Gmm && c->res.plan_E.empty()))
    return fail(c, POCS_E_STATE, "pocs_get_plan_evaluated: the last call was not a call of plans");
  return copy_out(c, out, cap, kind == Kind::Gmm ? c->res.plan_E : c->res.plan_E_mc.empty() ? c->plans.W : c->res.plan_E_mc, "ints");
}

int pocs_set_plan_tree(pocs_ctx* c, int nodes, const int* parent, const double* poses, const double* odoms) {
  if (!setter(c)) return POCS_E_ARG;
  if (int r = may_enter(c, "pocs_set_plan_tree", pocs_modes::kTree, pocs_modes::kSequence)) return r;      // (nodes = 0 too)
  if (nodes < 0 || nodes > POCS_MAX_TREE_NODES) return fail(c, POCS_E_ARG, "tree: %d nodes outside 0..%d", nodes, POCS_MAX_TREE_NODES);
  if (nodes == 0) {                                  // back to the single plan
    if (c->tree.n) { c->tree = PlanTree{}; leave_multi(c); }
    return POCS_OK;
  }
  if (int r = may_enter(c, "pocs_set_plan_tree", pocs_modes::kTree, pocs_modes::kPlans | pocs_modes::kLargeWorld)) return r;
  if (!parent || !poses || (nodes > 1 && !odoms)) return fail(c, POCS_E_ARG, "tree: null parents, poses or controls");
  if (parent[0] != -1) return fail(c, POCS_E_ARG, "tree: node 0 is the root, its parent must be -1 (got %d)", parent[0]);
  for (int n = 1; n < nodes; ++n)
    if (parent[n] < 0 || parent[n] >= n)
      return fail(c, POCS_E_ARG, "tree: parent[%d] = %d; one root, and every other node's parent comes before it (0 <= parent[n] < n)", n, parent[n]);
  if (int r = may_enter(c, "pocs_set_plan_tree", pocs_modes::kTree)) return r;
  const size_t T = (size_t)nodes;
  std::vector<int> depth(T, 0);
  int D = 0;
  for (size_t n = 1; n < T; ++n) { depth[n] = depth[(size_t)parent[n]] + 1; D = depth[n] > D ? depth[n] : D; }
  c->tree.parent.assign(parent, parent + T);
  c->tree.depth = depth;
  c->tree.pose.assign(poses, poses + 3 * T);
  if (odoms) c->tree.odom.assign(odoms, odoms + 3 * T); else c->tree.odom.assign(3 * T, 0.0);
  // slots: level by level, every level a contiguous range, the nodes of a level in node order
  c->tree.level.assign((size_t)D + 2, 0);
  for (size_t n = 0; n < T; ++n) c->tree.level[(size_t)depth[n] + 1] += 1;
  for (size_t d = 0; d <= (size_t)D; ++d) c->tree.level[d + 1] += c->tree.level[d];
  std::vector<int> fill(c->tree.level.begin(), c->tree.level.end() - 1);
  c->tree.slot.assign(T, 0); c->tree.node.assign(T, 0); c->tree.pslot.assign(T, 0);
  for (size_t n = 0; n < T; ++n) { const int s = fill[(size_t)depth[n]]++; c->tree.slot[n] = s; c->tree.node[(size_t)s] = (int)n; }
  for (size_t n = 1; n < T; ++n) c->tree.pslot[(size_t)c->tree.slot[n]] = c->tree.slot[(size_t)parent[n]];
  c->tree.dirty = true;
  enter_multi(c, 1, nodes);                          // one row per node in every [run][W] array
  c->tree.n = nodes;
  return POCS_OK;
}

int pocs_get_tree_probabilities(pocs_ctx* c, double* out, int cap) {
  if (!c || !out) return POCS_E_ARG;
  if (tree_last(c) == Kind::None || c->res.tree_probs.empty()) return fail(c, POCS_E_STATE, "pocs_get_tree_probabilities: the last call was not a call on a tree of plans");
  return copy_out(c, out, cap, c->res.tree_probs, "doubles");
}

int pocs_get_tree_evaluated(pocs_ctx* c, unsigned char* out, int cap) {
  if (!c || !out) return POCS_E_ARG;
  if (tree_last(c) == Kind::None || c->res.tree_eval.empty()) return fail(c, POCS_E_STATE, "pocs_get_tree_evaluated: the last call was not a call on a tree of plans");
  return copy_out(c, out, cap, c->res.tree_eval, "bytes");
}

int pocs_mc_get_tree_counts(pocs_ctx* c, unsigned long long* out, int cap) {
  if (!c || !out) return POCS_E_ARG;
  if (tree_last(c) != Kind::Mc || c->res.tree_C.empty()) return fail(c, POCS_E_STATE, "pocs_mc_get_tree_counts: the last call was not an MC call on a tree of plans");
  return copy_out(c, out, cap, c->res.tree_C, "counters");
}

int pocs_select_tree_node(pocs_ctx* c, int node) {
  if (!c) return POCS_E_ARG;
  if (tree_last(c) == Kind::None) return fail(c, POCS_E_STATE, "pocs_select_tree_node: the last call was not a call on a tree of plans");
  if (node < 0 || node >= c->tree.n) return fail(c, POCS_E_ARG, "node %d outside the tree (0..%d)", node, c->tree.n - 1);
  if (tree_last(c) == Kind::Gmm) tree_select_gmm(c, node);
  c->res.tree_sel = node;
  return POCS_OK;
}

// ---- clearance levels (include/pocs.h) ----
static int check_clearance_levels(pocs_ctx* c, const char* what, const double* d, int L) {
  if (L < 0 || L > POCS_MAX_CLEARANCE_LEVELS || (L > 0 && !d)) return fail(c, POCS_E_ARG, "%s: %d levels outside 0..%d (or null distances)", what, L, POCS_MAX_CLEARANCE_LEVELS);
  for (int l = 0; l < L; ++l)
    if (!std::isfinite(d[l]) || !(d[l] > (l ? d[l - 1] : 0.0)))
      return fail(c, POCS_E_ARG, "%s: distance %d (%g): finite distances with 0 < d[0] < d[1] < ... are needed", what, l, d[l]);
  return POCS_OK;
}

int pocs_set_clearance_levels(pocs_ctx* c, const double* d, int L) {
  if (!setter(c)) return POCS_E_ARG;
  if (int r = check_clearance_levels(c, "pocs_set_clearance_levels", d, L)) return r;
  c->clr_L = L;
  for (int l = 0; l < POCS_MAX_CLEARANCE_LEVELS; ++l) c->clr_d[l] = l < L ? d[l] : 0.0;
  c->env_dirty = true;                               // (the second record set and the distances live beside the world on the device)
  if (c->res.cl_state != Results::ClNoCall) c->res.cl_state = Results::ClTouched;      // (a table is served until the levels are touched or the next call)
  return POCS_OK;
}

int pocs_get_clearance_levels(const pocs_ctx* c, double* d, int cap) {
  if (!c) return POCS_E_ARG;
  if (c->clr_L > 0 && (!d || cap < c->clr_L)) return POCS_E_BUFFER;
  for (int l = 0; l < c->clr_L; ++l) d[l] = c->clr_d[l];
  return c->clr_L;
}

// The table of the last call serves `what`?  POCS_E_STATE with the reason otherwise.
static int clearance_served(pocs_ctx* c, const char* what) {
  const Results& r = c->res;
  switch (r.cl_state) {
    case Results::ClServed: break;
    case Results::ClNoCall: return fail(c, POCS_E_STATE, "%s: there was no call yet", what);
    case Results::ClOff: return fail(c, POCS_E_STATE, "%s: the last call ran without clearance levels (L was 0)", what);
    case Results::ClTouched: return fail(c, POCS_E_STATE, "%s: pocs_set_clearance_levels touched the levels since the last call", what);
    default: return fail(c, POCS_E_STATE, "%s: the levels are not applied to the last call (a tree of plans, a large world, POCS_OPT_OBSTACLE_COUNTS, a shard, the step API, segment checks, discs -- or it failed)", what);
  }
  if (r.cl_kind == Kind::None || r.cl_kind != r.last_kind || r.cl_counts.empty()) return fail(c, POCS_E_STATE, "%s: there was no call yet", what);
  return POCS_OK;
}
// run / plan r of the last call: its batch slot and the waypoints its rows cover
static void clearance_rows(const pocs_ctx* c, size_t r, size_t* slot, int* E) {
  const Kind kind = c->res.cl_kind;
  *slot = r; *E = c->res.cl_W;
  if (c->plans.n && r < c->res.plan_slot(kind).size()) {
    *slot = (size_t)c->res.plan_slot(kind)[r];
    if (kind == Kind::Gmm) *E = r < c->res.plan_E.size() ? c->res.plan_E[r] : c->plans.W[r];
    else *E = c->res.plan_E_mc.empty() ? c->plans.W[r] : c->res.plan_E_mc[r];
  }
}

int pocs_get_clearance_counts(pocs_ctx* c, unsigned long long* out, int cap, int* levels) {
  if (!c) return POCS_E_ARG;
  if (!out || !levels) return fail(c, POCS_E_ARG, "pocs_get_clearance_counts: null output");
  if (int r = clearance_served(c, "pocs_get_clearance_counts")) return r;
  size_t slot; int E;
  clearance_rows(c, (size_t)c->res.view, &slot, &E);
  const size_t L = (size_t)c->res.cl_L, W = (size_t)c->res.cl_W;
  if ((slot + 1) * W * POCS_MAX_CLEARANCE_LEVELS > c->res.cl_counts.size() || (size_t)E > W)
    return fail(c, POCS_E_STATE, "pocs_get_clearance_counts: the table does not cover the selection");
  *levels = (int)L;
  if ((size_t)(cap < 0 ? 0 : cap) < (size_t)E * L) return fail(c, POCS_E_BUFFER, "need %zu counters", (size_t)E * L);
  for (size_t w = 0; w < (size_t)E; ++w)
    for (size_t l = 0; l < L; ++l) out[w * L + l] = c->res.cl_counts[(slot * W + w) * POCS_MAX_CLEARANCE_LEVELS + l];
  return E;
}

int pocs_get_batch_clearance_probabilities(pocs_ctx* c, int level, double* out, int cap) {
  if (!c) return POCS_E_ARG;
  if (!out) return fail(c, POCS_E_ARG, "pocs_get_batch_clearance_probabilities: null output");
  if (int r = clearance_served(c, "pocs_get_batch_clearance_probabilities")) return r;
  if (level < 0 || level >= c->res.cl_L) return fail(c, POCS_E_ARG, "pocs_get_batch_clearance_probabilities: level %d outside 0..%d", level, c->res.cl_L - 1);
  const size_t W = (size_t)c->res.cl_W, R = c->res.cl_counts.size() / (W * POCS_MAX_CLEARANCE_LEVELS);
  const size_t lo = c->ra_internal ? (size_t)c->res.view : 0, hi = c->ra_internal ? lo + 1 : R;
  if ((long long)(hi - lo) > (long long)cap) return fail(c, POCS_E_BUFFER, "need %zu doubles", hi - lo);
  const double n = (double)c->res.cl_N;
  for (size_t r = lo; r < hi; ++r) {
    size_t slot; int E;
    clearance_rows(c, r, &slot, &E);
    const unsigned long long* A = &c->res.cl_counts[slot * W * POCS_MAX_CLEARANCE_LEVELS + (size_t)level];
    if (c->res.cl_kind == Kind::Gmm) {               // as gmm_combine forms the final probability from the collision counts
      double prod = 1.0;
      for (int w = 0; w < E; ++w) prod *= (1.0 - (double)A[(size_t)w * POCS_MAX_CLEARANCE_LEVELS] / (1.0 * n));
      out[r - lo] = 1.0 - prod;
    } else {
      unsigned long long sum = 0;
      for (int w = 0; w < E; ++w) sum += A[(size_t)w * POCS_MAX_CLEARANCE_LEVELS];
      out[r - lo] = (double)sum / n;
    }
  }
  return (int)(hi - lo);
}

// ---- watched regions (include/pocs.h) ----
int pocs_set_regions(pocs_ctx* c, const double* boxes, const int* kinds, int G) {
  if (!setter(c)) return POCS_E_ARG;
  if (G < 0 || G > POCS_MAX_REGIONS || (G > 0 && (!boxes || !kinds)))
    return fail(c, POCS_E_ARG, "pocs_set_regions: %d regions outside 0..%d (or a null pointer)", G, POCS_MAX_REGIONS);
  if (int r = check_boxes(c, "pocs_set_regions", boxes, (size_t)G, (size_t)(G > 0 ? G : 1), true)) return r;
  for (int g = 0; g < G; ++g)
    if (kinds[g] != POCS_REGION_TOUCH && kinds[g] != POCS_REGION_POINT)
      return fail(c, POCS_E_ARG, "pocs_set_regions: region %d: kind %d is neither POCS_REGION_TOUCH (0) nor POCS_REGION_POINT (1)", g, kinds[g]);
  c->reg_G = G;
  for (int g = 0; g < POCS_MAX_REGIONS; ++g) {
    for (int j = 0; j < 5; ++j) c->reg_box[5 * g + j] = g < G ? boxes[5 * g + j] : 0.0;
    c->reg_kind[g] = g < G ? kinds[g] : 0;
  }
  c->env_dirty = true;                               // (the regions' record lives beside the world on the device)
  if (c->res.rg_state != Results::RgNoCall) c->res.rg_state = Results::RgTouched;      // (a table is served until the regions are touched or the next call)
  return POCS_OK;
}

int pocs_get_regions(const pocs_ctx* c, double* boxes, int* kinds, int cap) {
  if (!c) return POCS_E_ARG;
  if (c->reg_G > 0 && (!boxes || !kinds || cap < c->reg_G)) return POCS_E_BUFFER;
  for (int g = 0; g < c->reg_G; ++g) {
    for (int j = 0; j < 5; ++j) boxes[5 * g + j] = c->reg_box[5 * g + j];
    kinds[g] = c->reg_kind[g];
  }
  return c->reg_G;
}

// The table of the last call serves `what`?  POCS_E_STATE with the reason otherwise.
static int regions_served(pocs_ctx* c, const char* what) {
  const Results& r = c->res;
  switch (r.rg_state) {
    case Results::RgServed: break;
    case Results::RgNoCall: return fail(c, POCS_E_STATE, "%s: there was no call yet", what);
    case Results::RgOff: return fail(c, POCS_E_STATE, "%s: the last call ran without watched regions (G was 0)", what);
    case Results::RgTouched: return fail(c, POCS_E_STATE, "%s: pocs_set_regions touched the regions since the last call", what);
    default: return fail(c, POCS_E_STATE, "%s: the regions are not applied to the last call (a tree of plans, a large world, POCS_OPT_OBSTACLE_COUNTS, a shard, the step API, a compound footprint, clearance levels, segment checks, discs -- or it failed)", what);
  }
  if (r.rg_kind == Kind::None || r.rg_kind != r.last_kind || r.rg_counts.empty()) return fail(c, POCS_E_STATE, "%s: there was no call yet", what);
  return POCS_OK;
}
// run / plan r of the last call: its batch slot and the waypoints its rows cover
static void region_rows(const pocs_ctx* c, size_t r, size_t* slot, int* E) {
  const Kind kind = c->res.rg_kind;
  *slot = r; *E = c->res.rg_W;
  if (c->plans.n && r < c->res.plan_slot(kind).size()) {
    *slot = (size_t)c->res.plan_slot(kind)[r];
    if (kind == Kind::Gmm) *E = r < c->res.plan_E.size() ? c->res.plan_E[r] : c->plans.W[r];
    else *E = c->res.plan_E_mc.empty() ? c->plans.W[r] : c->res.plan_E_mc[r];
  }
}

int pocs_get_region_counts(pocs_ctx* c, unsigned long long* out, int cap, int* regions) {
  if (!c) return POCS_E_ARG;
  if (!out || !regions) return fail(c, POCS_E_ARG, "pocs_get_region_counts: null output");
  if (int r = regions_served(c, "pocs_get_region_counts")) return r;
  size_t slot; int E;
  region_rows(c, (size_t)c->res.view, &slot, &E);
  const size_t G = (size_t)c->res.rg_G, W = (size_t)c->res.rg_W;
  if ((slot + 1) * W * POCS_MAX_REGIONS > c->res.rg_counts.size() || (size_t)E > W)
    return fail(c, POCS_E_STATE, "pocs_get_region_counts: the table does not cover the selection");
  *regions = (int)G;
  if ((size_t)(cap < 0 ? 0 : cap) < (size_t)E * G) return fail(c, POCS_E_BUFFER, "need %zu counters", (size_t)E * G);
  for (size_t w = 0; w < (size_t)E; ++w)
    for (size_t g = 0; g < G; ++g) out[w * G + g] = c->res.rg_counts[(slot * W + w) * POCS_MAX_REGIONS + g];
  return E;
}

int pocs_get_batch_region_probabilities(pocs_ctx* c, int region, int waypoint, double* out, int cap) {
  if (!c) return POCS_E_ARG;
  if (!out) return fail(c, POCS_E_ARG, "pocs_get_batch_region_probabilities: null output");
  if (int r = regions_served(c, "pocs_get_batch_region_probabilities")) return r;
  if (region < 0 || region >= c->res.rg_G) return fail(c, POCS_E_ARG, "pocs_get_batch_region_probabilities: region %d outside 0..%d", region, c->res.rg_G - 1);
  if (waypoint < -1) return fail(c, POCS_E_ARG, "pocs_get_batch_region_probabilities: waypoint %d (-1: each plan's own last waypoint)", waypoint);
  const size_t W = (size_t)c->res.rg_W, R = c->res.rg_counts.size() / (W * POCS_MAX_REGIONS);
  const size_t lo = c->ra_internal ? (size_t)c->res.view : 0, hi = c->ra_internal ? lo + 1 : R;
  if ((long long)(hi - lo) > (long long)cap) return fail(c, POCS_E_BUFFER, "need %zu doubles", hi - lo);
  const double n = (double)c->res.rg_N;
  for (size_t r = lo; r < hi; ++r) {
    size_t slot; int E;
    region_rows(c, r, &slot, &E);
    // the run's / plan's own length (a stop shortens E, not the plan): -1 asks for its last waypoint
    const int Wr = c->plans.n && r < c->plans.W.size() ? c->plans.W[r] : (int)W;
    const int w = waypoint < 0 ? Wr - 1 : waypoint;
    if (w >= E || w >= Wr) { out[r - lo] = -1.0; continue; }      // (not evaluated there: behind a stop, or past the plan's end)
    const double share = (double)c->res.rg_counts[(slot * W + (size_t)w) * POCS_MAX_REGIONS + (size_t)region] / n;      // one division
    if (c->res.rg_kind == Kind::Mc) { out[r - lo] = share; continue; }      // the cloud's joint share "never collided and in the region at w"
    // GMM: the estimator's independence product for "free up to w", p_v formed as gmm_combine forms it, in waypoint order from 1.0
    const size_t Rb = (size_t)c->res.batch_R, NC = (size_t)c->K * POCS_NMOM;
    double prod = 1.0;
    for (int v = 0; v < w; ++v) prod *= (1.0 - waypoint_probability(&c->res.batch_moments[((size_t)v * Rb + slot) * NC], c->K, (long long)c->res.rg_N));
    out[r - lo] = prod * share;
  }
  return (int)(hi - lo);
}

// ---- segment checks (include/pocs.h) ----
int pocs_set_segment_checks(pocs_ctx* c, int J) {
  if (!setter(c)) return POCS_E_ARG;
  if (J < 1 || J > POCS_MAX_SEGMENT_CHECKS)
    return fail(c, POCS_E_ARG, "pocs_set_segment_checks: %d checks per segment outside 1..%d", J, POCS_MAX_SEGMENT_CHECKS);
  if (J > 1) {
    // (not a mode of the table: the one mask of what segment checks exclude, pocs_modes.hpp, and a compound footprint beside it)
    unsigned in_the_way = modes_of(c) & pocs_modes::kSegExcluded;
    if (in_the_way) {                                // names ONE mode: the open sequence before all others, a connected exchange before its buffer
      const bool open = (in_the_way & pocs_modes::kSequence) != 0;
      if (open) in_the_way = pocs_modes::kSequence;
      if (in_the_way & pocs_modes::kXchgConnected) in_the_way &= ~(unsigned)pocs_modes::kXchgCreated;
      return fail(c, open ? POCS_E_ORDER : POCS_E_STATE, "pocs_set_segment_checks: %s; %s",
                  pocs_modes::name((pocs_modes::Mode)(in_the_way & (0u - in_the_way))), pocs_modes::kSegClause);
    }
    if (parts_applied(c))
      return fail(c, POCS_E_STATE, "pocs_set_segment_checks: a compound footprint is set (pocs_set_footprint_parts); %s", pocs_modes::kSegClause);
    if (discs_applied(c))
      return fail(c, POCS_E_STATE, "pocs_set_segment_checks: discs are set (pocs_set_discs); %s", pocs_modes::kDiscClause);
    if (rfoot_applied(c))
      return fail(c, POCS_E_STATE, "pocs_set_segment_checks: a round footprint is set (pocs_set_footprint_disc); %s", pocs_modes::kRoundFpClause);
  }
  c->seg_J = J;
  c->env_dirty = true;                               // (J and the fractions live beside the world on the device)
  if (c->res.sg_state != Results::SgNoCall) c->res.sg_state = Results::SgTouched;      // (a table is served until the setter is touched or the next call)
  return POCS_OK;
}

int pocs_get_segment_checks(const pocs_ctx* c) { return c ? c->seg_J : POCS_E_ARG; }

int pocs_get_segment_counts(pocs_ctx* c, unsigned long long* out, int cap) {
  if (!c) return POCS_E_ARG;
  if (!out) return fail(c, POCS_E_ARG, "pocs_get_segment_counts: null output");
  const Results& r = c->res;
  const char* const what = "pocs_get_segment_counts";
  switch (r.sg_state) {
    case Results::SgServed: break;
    case Results::SgNoCall: return fail(c, POCS_E_STATE, "%s: there was no call yet", what);
    case Results::SgOff: return fail(c, POCS_E_STATE, "%s: the last call ran without segment checks (J was 1)", what);
    case Results::SgTouched: return fail(c, POCS_E_STATE, "%s: pocs_set_segment_checks was called since the last call", what);
    default: return fail(c, POCS_E_STATE, "%s: the last call is not a served shape (it failed, or was refused)", what);
  }
  if (r.sg_kind == Kind::None || r.sg_kind != r.last_kind || r.sg_counts.empty()) return fail(c, POCS_E_STATE, "%s: there was no call yet", what);
  // run / plan `view` of the last call: its batch slot and the waypoints its row covers
  size_t slot = (size_t)r.view;
  int E = r.sg_W;
  if (c->plans.n && (size_t)r.view < r.plan_slot(r.sg_kind).size()) {
    const size_t p = (size_t)r.view;
    slot = (size_t)r.plan_slot(r.sg_kind)[p];
    if (r.sg_kind == Kind::Gmm) E = p < r.plan_E.size() ? r.plan_E[p] : c->plans.W[p];
    else E = r.plan_E_mc.empty() ? c->plans.W[p] : r.plan_E_mc[p];
  }
  const size_t W = (size_t)r.sg_W;
  if ((slot + 1) * W > r.sg_counts.size() || (size_t)E > W) return fail(c, POCS_E_STATE, "%s: the table does not cover the selection", what);
  if (cap < E) return fail(c, POCS_E_BUFFER, "need %d counters", E);
  for (int w = 0; w < E; ++w) out[w] = r.sg_counts[slot * W + (size_t)w];
  return E;
}

int pocs_get_batch_probabilities(pocs_ctx* c, double* out, int cap) {
  if (!c || !out) return POCS_E_ARG;
  return batch_out(c, out, cap, c->res.batch_probs, "doubles");
}

int pocs_select_batch_run(pocs_ctx* c, int run) {
  if (!c) return POCS_E_ARG;
  if (c->ra_internal) return fail(c, POCS_E_ORDER, "pocs_select_batch_run: the last launch was a run-ahead batch (one run per command)");
  if (int r = may_enter(c, "pocs_select_batch_run", pocs_modes::kSelectRun)) return r;
  if (run < 0 || run >= c->res.batch_R || c->res.batch_probs.empty()) return fail(c, POCS_E_ARG, "run %d outside the last batch (0..%d)", run, c->res.batch_R - 1);
  if (c->res.last_kind == Kind::Gmm) gmm_select_view(c, run);       // per-waypoint probabilities and moments of that run
  c->res.view = run;
  return POCS_OK;
}

int pocs_set_shard(pocs_ctx* c, long long first, long long count) {
  if (!setter(c)) return POCS_E_ARG;
  if (first == -1 && count == -1) { c->shard_first = -1; c->shard_count = -1; return POCS_OK; }   // whole range
  if (int r = may_enter(c, "pocs_set_shard", pocs_modes::kShard)) return r;
  if (first < 0 || count < 0) return fail(c, POCS_E_ARG, "negative shard");
  c->shard_first = first; c->shard_count = count;
  return POCS_OK;
}

int pocs_set_stream(pocs_ctx* c, void* s) {
  if (!setter(c)) return POCS_E_ARG;
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return POCS_OK;
}

int pocs_gmm_bind_moments(pocs_ctx* c, void* dptr, long long len) {
  if (!setter(c)) return POCS_E_ARG;
  if (dptr) if (int r = may_enter(c, "pocs_gmm_bind_moments", pocs_modes::kMoments)) return r;
  c->ext_moments = (double*)dptr; c->ext_moments_len = dptr ? len : 0;
  return POCS_OK;
}

int pocs_run_gmm_estimation(pocs_ctx* c, double* probability) {
  if (!c) return POCS_E_ARG;
  if (!probability) return fail(c, POCS_E_ARG, "null output");
  if (int r = ra_front(c, Kind::Gmm, true, [&] { return run_gmm_full(c, probability); })) return r;
  *probability = c->res.batch_probs[(size_t)c->res.view];
  return POCS_OK;
}

int pocs_run_simulation(pocs_ctx* c, double* probability) {
  if (!c) return POCS_E_ARG;
  if (!probability) return fail(c, POCS_E_ARG, "null output");
  if (int r = ra_front(c, Kind::Mc, true, [&] { const int rc = run_mc_local(c); if (rc == POCS_OK) mc_fill_probs(c); return rc; })) return r;
  *probability = c->res.batch_probs[(size_t)c->res.view];
  return POCS_OK;
}

int pocs_mc_run_local(pocs_ctx* c, unsigned long long* collided) {
  if (!c) return POCS_E_ARG;
  if (!collided) return fail(c, POCS_E_ARG, "null output");
  if (int r = ra_front(c, Kind::Mc, false, [&] { return run_mc_local(c); })) return r;
  *collided = c->res.mc_counts[0];
  return POCS_OK;
}

int pocs_mc_get_batch_counts(pocs_ctx* c, unsigned long long* out, int cap) {
  if (!c || !out) return POCS_E_ARG;
  return batch_out(c, out, cap, c->res.mc_counts, "counters");
}

int pocs_mc_get_waypoint_counts(pocs_ctx* c, unsigned long long* out, int cap) {
  if (!c || !out) return POCS_E_ARG;
  const size_t W = (size_t)(c->res.mc_wp_W > 0 ? c->res.mc_wp_W : 1), r = (size_t)c->res.view;
  if (c->tree.n) {                                   // the selected node's path: the first collisions at each of its nodes
    if (tree_last(c) != Kind::Mc || c->res.tree_F.empty()) return fail(c, POCS_E_STATE, "pocs_mc_get_waypoint_counts: the last call was not an MC call on the tree");
    const int n = c->tree.depth[(size_t)c->res.tree_sel] + 1;
    if (n > cap) return fail(c, POCS_E_BUFFER, "need %d counters", n);
    for (int v = c->res.tree_sel, w = n - 1; v >= 0; v = c->tree.parent[(size_t)v], --w) out[w] = c->res.tree_F[(size_t)v];
    return n;
  }
  if (c->res.last_kind != Kind::Mc || c->res.mc_wp.empty() || (r + 1) * W > c->res.mc_wp.size())
    return fail(c, POCS_E_STATE, "pocs_mc_get_waypoint_counts: the last call was not an MC call under POCS_OPT_MC_WAYPOINT_COUNTS (or POCS_OPT_MC_RISK_BOUND with a bound)");
  int n = (int)W;                                    // the selected run's waypoints; a plan's own, or those before its stop
  if (c->plans.n && r < c->res.plan_slot(Kind::Mc).size()) n = c->res.plan_E_mc.empty() ? c->plans.W[r] : c->res.plan_E_mc[r];
  return copy_out(c, out, cap, &c->res.mc_wp[r * W], (size_t)n, "counters");
}

int pocs_xchg_create(pocs_ctx* c, int world, int rank, void* handle64) {
  if (!c || !handle64) return POCS_E_ARG;
  if (world < 1 || world > POCS_XCHG_MAX_WORLD || rank < 0 || rank >= world)
    return fail(c, POCS_E_ARG, "exchange: world %d / rank %d outside 1..%d", world, rank, POCS_XCHG_MAX_WORLD);
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "pocs.h promises a 64-byte handle");
  if (int r = may_enter(c, "pocs_xchg_create", pocs_modes::kXchgCreated)) return r;
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->xchg_own) {
    // FINE-GRAINED device memory: other GPUs write into it and this GPU polls it inside a running kernel.
    // Ordinary (coarse-grained) allocations are only coherent with other devices at kernel boundaries --
    // a flag once cached in an XCD's L2 could be read stale for ever.
    HIPCHK(c, hipExtMallocWithFlags(&c->xchg_own, POCS_XCHG_BYTES, hipDeviceMallocFinegrained));
    HIPCHK(c, hipMemset(c->xchg_own, 0, POCS_XCHG_BYTES));       // epoch 0 = nothing has landed
    HIPCHK(c, hipDeviceSynchronize());
  }
  c->xchg_world = world; c->xchg_rank = rank; c->xchg_connected = false;
  hipIpcMemHandle_t h;
  HIPCHK(c, hipIpcGetMemHandle(&h, c->xchg_own));
  memcpy(handle64, &h, sizeof h);
  return POCS_OK;
}

int pocs_xchg_connect(pocs_ctx* c, const void* handles, int world) {
  if (!c || !handles) return POCS_E_ARG;
  if (int r = may_enter(c, "pocs_xchg_connect", pocs_modes::kXchgConnected)) return r;
  if (!c->xchg_own || world != c->xchg_world) return fail(c, POCS_E_ORDER, "pocs_xchg_connect before pocs_xchg_create (or another world size)");
  HIPCHK(c, hipSetDevice(c->device));
  for (int q = 0; q < world; ++q) {
    if (q == c->xchg_rank) { c->xchg_peer[q] = c->xchg_own; continue; }
    hipIpcMemHandle_t h;
    memcpy(&h, (const char*)handles + 64 * (size_t)q, sizeof h);
    if (c->xchg_peer[q] && c->xchg_peer[q] != c->xchg_own) { (void)hipIpcCloseMemHandle(c->xchg_peer[q]); c->xchg_peer[q] = nullptr; }
    HIPCHK(c, hipIpcOpenMemHandle(&c->xchg_peer[q], h, hipIpcMemLazyEnablePeerAccess));
  }
  c->xchg_connected = true;
  return POCS_OK;
}

int pocs_get_path_length(const pocs_ctx* c) {
  if (!c) return POCS_E_ARG;
  if (c->plans.n) return c->plans.W[(size_t)(c->res.view < c->plans.n ? c->res.view : 0)];     // the selected plan's
  if (c->tree.n) return c->tree.depth[(size_t)c->res.tree_sel] + 1;                     // the path root -> the selected node
  return c->W;
}

int pocs_get_waypoint_probabilities(pocs_ctx* c, double* out, int cap) {
  if (!c || !out) return POCS_E_ARG;
  return copy_out(c, out, cap, c->res.probs, "doubles");
}

int pocs_get_moments(pocs_ctx* c, int w, double* out, int cap) {
  if (!c || !out) return POCS_E_ARG;
  const int n = c->K * POCS_NMOM;
  if (w < 0 || (size_t)(w + 1) * n > c->res.last_moments.size()) return fail(c, POCS_E_ARG, "no moments for waypoint %d", w);
  return copy_out(c, out, cap, &c->res.last_moments[(size_t)w * n], (size_t)n, "doubles");
}

// The text channel: the grammar (names, token counts, order rules) lives in pocs_command.hpp -- host only, fuzzed
// under sanitizers on the CPU -- and this is the dispatch of a parsed line to the typed setters above.
int pocs_send_command(pocs_ctx* c, const char* line, char* out, size_t cap) {
  if (!c || !line) return POCS_E_ARG;
  if (out && cap) out[0] = 0;
  const pocs_cmd::Shape shape = {c->num_landmarks, c->W};
  const pocs_cmd::Parsed p = pocs_cmd::parse(line, shape);
  if (p.err) return fail(c, p.err, "%s", p.msg.c_str());
  const std::vector<double>& v = p.v;
  switch (p.id) {
    case pocs_cmd::kMyCommand: return put(c, out, cap, "output");                   // mcsimplugin.cpp:225-231
    case pocs_cmd::kArmaCommand: return POCS_OK;                                     // :189-223 (Armadillo demo) -> no-op
    case pocs_cmd::kHelp: return put(c, out, cap, kHelp);
    case pocs_cmd::kSetAlphas: return pocs_set_alphas(c, v.data(), (int)v.size());   // :174-187
    case pocs_cmd::kSetQ: return pocs_set_q(c, v[0]);
    case pocs_cmd::kSetNumLandmarks: return pocs_set_num_landmarks(c, (int)p.n);
    case pocs_cmd::kSetLandmarks: return pocs_set_landmarks(c, v.data(), c->num_landmarks);
    case pocs_cmd::kSetNumParticles: return pocs_set_num_particles(c, p.n);
    case pocs_cmd::kSetInitialCovariance: return pocs_set_initial_covariance(c, v.data());
    case pocs_cmd::kSetPathLength: return pocs_set_path_length(c, (int)p.n);
    case pocs_cmd::kSetTrajectory: return pocs_set_trajectory(c, v.data(), c->W);
    case pocs_cmd::kSetOdometry: return pocs_set_odometry(c, v.data(), c->W - 1);
    case pocs_cmd::kSetNumGaussians: return pocs_set_num_gaussians(c, (int)p.n);
    case pocs_cmd::kSetNumGMMSamples: return pocs_set_num_gmm_samples(c, p.n);
    case pocs_cmd::kSetSeed: return pocs_set_seed(c, (uint64_t)p.seed);
    case pocs_cmd::kSetFootprint: return pocs_set_footprint(c, v[0], v[1], v[2], v[3]);
    case pocs_cmd::kAddObstacle: {
      if (int r = may_enter(c, "addObstacle", pocs_modes::kAddObstacle)) return r;
      std::vector<double> b(c->boxes.begin(), c->boxes.begin() + (size_t)world_boxes(c) * 5);   // (under a schedule: world 0)
      b.insert(b.end(), v.begin(), v.end());
      return pocs_set_obstacles(c, b.data(), (int)(b.size() / 5));
    }
    case pocs_cmd::kClearObstacles: return pocs_set_obstacles(c, nullptr, 0);
    case pocs_cmd::kSetBatch: return pocs_set_batch(c, (int)p.n);
    case pocs_cmd::kSetRunAhead: return pocs_set_option(c, POCS_OPT_RUN_AHEAD, p.n);
    case pocs_cmd::kRunSimulation: case pocs_cmd::kRunGMMEstimation: {               // :75-81, :66-72
      double prob = 0.0;
      const int r = (p.id == pocs_cmd::kRunSimulation) ? pocs_run_simulation(c, &prob) : pocs_run_gmm_estimation(c, &prob);
      if (r) return r;
      char buf[64];
      snprintf(buf, sizeof buf, "%.17g", prob);
      return put(c, out, cap, buf);
    }
    case pocs_cmd::kUnknown: break;
  }
  return fail(c, POCS_E_UNKNOWN_COMMAND, "unknown command '%s'", p.name.c_str());
}

}  // extern "C"

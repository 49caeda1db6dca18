// pocs_host.hip -- the run paths of the host runtime: what a GMM or an MC call prepares, enqueues (eagerly or as a
// replayed hipGraph), reads back and combines -- for a batch of runs, a set of plans or a tree of plans -- and the step and
// exchange API on top of the same launches.  Everything per particle / per sample runs in pocs_kernels.hip.  There is no
// CPU path for that work.
#include <chrono>

#include "pocs_ctx.hpp"

namespace pocs_rt POCS_HIDDEN {

int grid_blocks(long long count, int block, int bpc) {
  // One block per `block` evaluations up to `bpc` resident blocks per CU (256 CUs), grid-stride beyond that.
  long long nb = (count + block - 1) / block;
  if (nb < 1) nb = 1;
  if (nb > 256LL * bpc) nb = 256LL * bpc;
  if (nb > POCS_MAX_BLOCKS) nb = POCS_MAX_BLOCKS;
  return (int)nb;
}
// Task geometry of k_gmm_step (pocs_kernels.h): a chunk = one block iteration = TB pairs of samples; a
// run's `chunks` are cut into VS = 2^vs_shift virtual slices -- a function of the shard's sample count
// ONLY, the moment sums are defined on them -- and the launch's units (run, virtual slice) are dealt to
// the blocks `upb` at a time.  The chip takes blocks 256 at a time (one more per CU) and holds 512 of
// these: `upb` is the smallest number that fits the launch into 512 blocks (256 below 4 runs: fewer,
// fatter blocks amortise head and tail better when the launch is short anyway), so every block of a launch
// has the same amount of work whatever the number of runs (20 runs x 256 slices = 512 blocks x 10).
#define POCS_FULL_GRID_FROM_RUNS 4   // (round 4, measured after the heads got shorter: 512 blocks from 4 runs per launch on, +4 % at 4 runs, +6-7 % at 6 and 7; 2 and 3 runs lose 4 % with them -- profiles/r04_ab_full_grid_from_4_runs.txt; it was 8)
struct GmmGeometry { long long chunks; int vs_shift; int upb; int blocks; };
GmmGeometry gmm_geometry(long long count, int runs, int K, int groups = 1) {
  const int tb = POCS_GMM_BLOCK_OF(K);
  const long long npairs = (count + 1) / 2;
  GmmGeometry g;
  g.chunks = (npairs + tb - 1) / tb;
  if (g.chunks < 1) g.chunks = 1;
  g.vs_shift = 0;
  while ((2LL << g.vs_shift) <= g.chunks && (2 << g.vs_shift) <= POCS_GMM_MAX_VS) ++g.vs_shift;
  if (runs < 1) runs = 1;
  const long long units = (long long)runs << g.vs_shift;
  // (`groups` launches share the chip: each gets its share of the resident blocks)
  const long long budget = (runs * groups >= POCS_FULL_GRID_FROM_RUNS ? POCS_NUM_CUS * POCS_GMM_BLOCKS_PER_CU : POCS_NUM_CUS) / groups;
  g.upb = (int)((units + budget - 1) / budget);
  if (g.upb > (1 << g.vs_shift)) g.upb = 1 << g.vs_shift;           // a block's range touches at most two runs
  g.blocks = (int)((units + g.upb - 1) / g.upb);
  return g;
}
int grid_for_mc(long long count, int runs = 1) {                                      // MC kernels, per run
  // six 256-thread blocks per CU (69 VGPRs: plenty of room) keep enough loads in flight for the
  // stream: measured 0.78 of the HBM peak against 0.67 with three, 0.70 with eight
  const int one = grid_blocks(count, POCS_BLOCK, 6);
  if (runs <= 1) return one;
  int per = 1536 / runs;                             // the batch's launches share the chip's 6 x 256 resident blocks
  if (per < 1) per = 1;
  return per < one ? per : one;
}

int check_common(pocs_ctx* c) {
  if (!c->have_q || !c->have_landmarks) return fail(c, POCS_E_STATE, "setQ / setLandmarks missing");
  if (!c->have_cov0) return fail(c, POCS_E_STATE, "setInitialCovariance missing");
  if (!c->plans.n && !c->tree.n && (!c->have_traj || !c->have_odom)) return fail(c, POCS_E_STATE, "setTrajectory / setOdometry missing");
  if (c->W < 1) return fail(c, POCS_E_STATE, "setPathLength missing");
  // The reference receives its collision world through the module constructor (sim(penv),
  // mcsimplugin.cpp:12 -> MCSimulator.h:139-156).  A context that was never given one would answer
  // 0.0 for every run: refuse instead.  An explicitly empty world (clearObstacles) is allowed.
  if (!c->have_obstacles && !discs_applied(c))       // (a context given discs and never boxes has a world: M = 0)
    return fail(c, POCS_E_STATE, "no collision world: pocs_set_obstacles / addObstacle / clearObstacles missing");
  return POCS_OK;
}

int upload_tables(pocs_ctx* c) {               // log / sector tables of the numerics spec, once
  if (c->d_tables.p) return POCS_OK;
  pocs_tables T;
  pocs_tables_init(&T);
  if (int r = ensure(c, c->d_tables, sizeof T)) return r;
  HIPCHK(c, hipMemcpy(c->d_tables.p, &T, sizeof T, hipMemcpyHostToDevice));
  return POCS_OK;
}
// Clearance levels: the record of one world step as the kernels read it (pocs_clear_dev) -- the footprint grown by the largest
// distance, its radius and corner angle, the distances, and the step's boxes prepared for that footprint exactly as upload_world
// prepares them for the footprint itself.  (pocs_probe_device_clearance prepares its own table through this function too.)
void prepare_clearance(const pocs_footprint& fp, const double* d, int L, const double* boxes, int M, pocs_clear_dev* out) {
  memset(out, 0, sizeof *out);
  out->fp = L > 0 ? pocs_grown_footprint(&fp, d[L - 1]) : fp;
  out->fp_rr = sqrt(out->fp.hx * out->fp.hx + out->fp.hy * out->fp.hy);
  out->fp_phi = atan2(out->fp.hy, out->fp.hx);
  for (int l = 0; l < L; ++l) out->d[l] = d[l];
  for (int m = 0; m < M; ++m) pocs_prepare_obstacle(boxes + (size_t)m * 5, &out->fp, &out->obs[(size_t)m * POCS_OBS_STRIDE]);
}

// A compound footprint (F > 1) as the kernels read it: the parts (pocs_prepare_part), and one world step's record with the boxes
// prepared for the part with the largest bounding radius -- a broad phase that is conservative for every part -- and part 0 as its
// footprint.  (pocs_probe_device_footprint_parts prepares its own through this function too; env may be null.)
void prepare_parts(const pocs_footprint* parts, int F, const double* boxes, int M, pocs_env_dev* env, pocs_parts_dev* out) {
  if (out) {
    memset(out, 0, sizeof *out);
    for (int f = 0; f < F; ++f) pocs_prepare_part(&parts[f], &out->part[(size_t)f * POCS_PART_STRIDE]);
  }
  if (env) {
    const pocs_footprint* cover = &parts[pocs_parts_cover(parts, F)];
    memset(env, 0, sizeof *env);
    env->fp = parts[0]; env->M = M;
    for (int m = 0; m < M; ++m) pocs_prepare_obstacle(boxes + (size_t)m * 5, cover, &env->obs[(size_t)m * POCS_OBS_STRIDE]);
  }
}

// Where the levels are applied: whole calls on one GPU over a small world, static or scheduled -- single runs, batches, run-ahead,
// calls of plans with and without the risk bound, GMM and MC.  A tree of plans, a large world, per-box counts, a shard (and with it
// the exchange and a bound moments buffer) are the calls they are with L = 0; the step API never asks.
bool clearance_applied(const pocs_ctx* c) {
  using namespace pocs_modes;
  return c->clr_L > 0 && !parts_applied(c) && !seg_applied(c) && !discs_applied(c) && !rfoot_applied(c) && !in_mode(c, kTree | kLargeWorld | kObsCounts | kShard | kMoments);
}

// Watched regions: the record the kernels read (pocs_regions_dev) -- region g prepared as upload_world prepares an obstacle, for
// the region's own footprint: the robot's (POCS_REGION_TOUCH) or the point {0, 0, 0, 0} (POCS_REGION_POINT).
// (pocs_probe_device_regions prepares its own record through this function too.)
void prepare_regions(const pocs_footprint& fp, const double* boxes, const int* kinds, int G, pocs_regions_dev* out) {
  memset(out, 0, sizeof *out);
  for (int g = 0; g < G; ++g) {
    const pocs_footprint f = kinds[g] == POCS_REGION_POINT ? pocs_footprint{0.0, 0.0, 0.0, 0.0} : fp;
    out->kind[g] = kinds[g];
    out->fp[4 * g] = f.dx; out->fp[4 * g + 1] = f.dy; out->fp[4 * g + 2] = f.hx; out->fp[4 * g + 3] = f.hy;
    out->fp_rr[g] = sqrt(f.hx * f.hx + f.hy * f.hy);
    out->fp_phi[g] = atan2(f.hy, f.hx);
    pocs_prepare_obstacle(boxes + (size_t)g * 5, &f, &out->rec[(size_t)g * POCS_OBS_STRIDE]);
  }
}

// Where the regions are applied -- the ONE place that says so: whole calls on one GPU over a small world, static or scheduled --
// single runs, batches in both sub-batch forms, run-ahead, calls of plans with and without the risk bounds, GMM and MC.  A tree of
// plans, a large world, per-box counts, a shard (and with it the exchange and a bound moments buffer), a compound footprint and clearance levels with
// L > 0 are the calls they are with G = 0; the step API never asks.
bool regions_applied(const pocs_ctx* c) {
  using namespace pocs_modes;
  return c->reg_G > 0 && c->clr_L == 0 && !parts_applied(c) && !seg_applied(c) && !discs_applied(c) && !rfoot_applied(c) && !in_mode(c, kTree | kLargeWorld | kObsCounts | kShard | kMoments);
}

// Segment checks (J > 1) as the kernels read them (pocs_seg_dev): J and the fractions f_j = j / J.  (pocs_probe_device_segment
// prepares its own record through this function too.)  Clearance levels and watched regions are not applied while J > 1 (above):
// the call is the J > 1 call without them.
void prepare_segment(int J, pocs_seg_dev* out) {
  memset(out, 0, sizeof *out);
  out->J = J;
  pocs_segment_fractions(J, out->f);
}

int upload_world(pocs_ctx* c) {                // tables + the collision world: one record (obstacle records, footprint) per step of the schedule
  if (int r = upload_tables(c)) return r;
  if (c->env_dirty) {
    const size_t Sb = (size_t)c->world_S, S = (size_t)env_steps(c);
    const int M = world_boxes(c);
    std::vector<pocs_env_dev> env(S);
    memset(env.data(), 0, S * sizeof(pocs_env_dev));
    std::vector<double> noise(noise_rows_held(c) ? S * POCS_MAX_OBSTACLES * POCS_NOISE_STRIDE : 0, 0.0);      // uncertain discs: a row per record (hypotheses without covariances: rows of zeros)
    std::vector<uint32_t> gates(hyp_applied(c) ? POCS_MAX_OBSTACLES * POCS_GATE_STRIDE : 0, 0u);      // prediction hypotheses: a gate per record, the same at every step
    if (hyp_applied(c)) {
      std::vector<unsigned long long> lo((size_t)c->disc_D), hi((size_t)c->disc_D);
      int bad = 0;
      pocs_hyp_thresholds(c->hyp_group.data(), c->hyp_weight.data(), c->disc_D, lo.data(), hi.data(), &bad);      // (the setter has checked the table)
      for (int d = 0; d < c->disc_D; ++d) pocs_hyp_gate(c->hyp_group[(size_t)d], lo[(size_t)d], hi[(size_t)d], &gates[(size_t)(M + d) * POCS_GATE_STRIDE]);
    }
    pocs_parts_dev parts;
    for (size_t s = 0; s < S; ++s) {
      if (discs_applied(c) || rfoot_applied(c)) {    // round obstacles: record s is box step min(s, Sb - 1), then disc step min(s, Sd - 1)
        const bool rf = rfoot_applied(c);              // (a round footprint, with or without discs: the same records with rho as the bounding radius)
        const size_t sb = s < Sb ? s : Sb - 1, sd = s < (size_t)c->disc_S ? s : (size_t)c->disc_S - 1;
        const int D = c->disc_D;
        env[s].fp = c->fp;
        env[s].M = M + D;
        for (int m = 0; m < M; ++m) {
          const double* const box = &c->boxes[(sb * (size_t)M + (size_t)m) * 5];
          if (rf) pocs_prepare_obstacle_round(box, c->fp_rho, &env[s].obs[(size_t)m * POCS_OBS_STRIDE]);
          else pocs_prepare_box_beside_discs(box, &c->fp, &env[s].obs[(size_t)m * POCS_OBS_STRIDE]);
        }
        for (int d = 0; d < D; ++d) {
          double* const rec = &env[s].obs[(size_t)(M + d) * POCS_OBS_STRIDE];
          if (rf) pocs_prepare_disc_round(&c->discs[(sd * (size_t)D + (size_t)d) * 3], c->fp_rho, rec);
          else pocs_prepare_disc(&c->discs[(sd * (size_t)D + (size_t)d) * 3], &c->fp, rec);
          if (noise_applied(c)) {                      // the record's row (zeros: a certain disc) and the growth of its fields 6 and 7
            double* const row = &noise[(s * POCS_MAX_OBSTACLES + (size_t)(M + d)) * POCS_NOISE_STRIDE];
            pocs_disc_noise_factor(&c->disc_cov[(sd * (size_t)D + (size_t)d) * 3], row);      // (the setter has checked every row)
            row[3] = (double)d;
            pocs_disc_noise_grow(row, rec);
          }
        }
        continue;
      }
      if (parts_applied(c)) {                        // (a compound footprint: the records of the covering part; no large world then)
        prepare_parts(c->fp_parts, c->fp_F, c->boxes.data() + s * (size_t)M * 5, M, &env[s], s == 0 ? &parts : nullptr);
        continue;
      }
      env[s].fp = c->fp;
      env[s].M = M;
      for (int m = 0; m < M; ++m)
        pocs_prepare_obstacle(&c->boxes[(s * (size_t)M + (size_t)m) * 5], &c->fp, &env[s].obs[(size_t)m * POCS_OBS_STRIDE]);
    }
    if (int r = ensure(c, c->d_env, S * sizeof(pocs_env_dev))) return r;      // (a schedule that grows: the graphs go with the old table)
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (nothing queued may still read the last world's)
    HIPCHK(c, hipMemcpy(c->d_env.p, env.data(), S * sizeof(pocs_env_dev), hipMemcpyHostToDevice));
    if (!noise.empty()) {                            // (the same shape: overwritten in place, the cached graph replays)
      if (int r = ensure(c, c->d_noise, noise.size() * sizeof(double))) return r;
      HIPCHK(c, hipMemcpy(c->d_noise.p, noise.data(), noise.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    if (!gates.empty()) {                            // (a fixed size: other weights are overwritten in place, the cached graph replays)
      if (int r = ensure(c, c->d_gates, gates.size() * sizeof(uint32_t))) return r;
      HIPCHK(c, hipMemcpy(c->d_gates.p, gates.data(), gates.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (parts_applied(c)) {
      if (int r = ensure(c, c->d_parts, sizeof(pocs_parts_dev))) return r;
      HIPCHK(c, hipMemcpy(c->d_parts.p, &parts, sizeof parts, hipMemcpyHostToDevice));
    }
    if (c->clr_L > 0 && !large_world(c)) {           // the second record set, next to the first: the footprint grown by d_L
      std::vector<pocs_clear_dev> clr(Sb);             // (per step of the BOXES' schedule: the levels are not applied under discs)
      for (size_t s = 0; s < Sb; ++s) prepare_clearance(c->fp, c->clr_d, c->clr_L, c->boxes.data() + s * (size_t)M * 5, M, &clr[s]);
      if (int r = ensure(c, c->d_clr, Sb * sizeof(pocs_clear_dev))) return r;
      HIPCHK(c, hipMemcpy(c->d_clr.p, clr.data(), Sb * sizeof(pocs_clear_dev), hipMemcpyHostToDevice));
    }
    if (seg_applied(c)) {                            // the segment checks' record, next to the world
      pocs_seg_dev sg;
      prepare_segment(c->seg_J, &sg);
      if (int r = ensure(c, c->d_seg, sizeof sg)) return r;
      HIPCHK(c, hipMemcpy(c->d_seg.p, &sg, sizeof sg, hipMemcpyHostToDevice));
    }
    if (c->reg_G > 0 && !parts_applied(c)) {         // the watched regions, next to the world: TOUCH regions follow the footprint
      pocs_regions_dev reg;
      prepare_regions(c->fp, c->reg_box, c->reg_kind, c->reg_G, &reg);
      if (int r = ensure(c, c->d_reg, sizeof reg)) return r;
      HIPCHK(c, hipMemcpy(c->d_reg.p, &reg, sizeof reg, hipMemcpyHostToDevice));
    }
    if (large_world(c)) {                            // the large world's records (the env record above then holds the footprint and M = 0)
      const size_t LM = (size_t)large_boxes(c);
      std::vector<double> rec(LM * POCS_OBS_STRIDE);
      for (size_t m = 0; m < LM; ++m) pocs_prepare_obstacle(&c->world[m * 5], &c->fp, &rec[m * POCS_OBS_STRIDE]);
      if (int r = ensure(c, c->d_world, rec.size() * sizeof(double))) return r;
      HIPCHK(c, hipMemcpy(c->d_world.p, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    c->env_dirty = false;
  }
  return POCS_OK;
}
int upload_static(pocs_ctx* c) {
  if (int r = upload_world(c)) return r;
  if (c->sensor_dirty) {
    if (int r = ensure(c, c->d_sensor, sizeof(pocs_sensor))) return r;
    HIPCHK(c, hipMemcpy(c->d_sensor.p, &c->sensor, sizeof(pocs_sensor), hipMemcpyHostToDevice));
    c->sensor_dirty = false;
  }
  return POCS_OK;
}

int upload_tree(pocs_ctx* c) {                  // a tree of plans: the slots' parents, once per tree
  if (!c->tree.dirty && c->d_tparent.p) return POCS_OK;
  if (int r = ensure(c, c->d_tparent, c->tree.pslot.size() * sizeof(int))) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));      // (nothing queued may still read the last tree's)
  HIPCHK(c, hipMemcpy(c->d_tparent.p, c->tree.pslot.data(), c->tree.pslot.size() * sizeof(int), hipMemcpyHostToDevice));
  c->tree.dirty = false;
  return POCS_OK;
}

int prof_begin(pocs_ctx* c, size_t launches) {
  c->prof_ms = 0.0; c->prof_launches = 0;
  if (c->opt_profile != 1) return POCS_OK;
  while (c->events.size() < 2 * launches) {
    hipEvent_t e;
    HIPCHK(c, hipEventCreate(&e));
    c->events.push_back(e);
  }
  return POCS_OK;
}
int prof_collect(pocs_ctx* c, size_t launches) {
  if (c->opt_profile != 1) return POCS_OK;
  for (size_t i = 0; i < launches; ++i) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->events[2 * i], c->events[2 * i + 1]));
    c->prof_ms += ms;
  }
  c->prof_launches = (long long)launches;
  return POCS_OK;
}

// ------------------------------------------------------------------------------------------
// The issuer and the graph cache
// ------------------------------------------------------------------------------------------
// Every kernel launch of a call, the fork and join of its sub-batches and its profiling events go through an Issuer.  In Sign mode
// (`sig` set) it launches nothing and appends to `sig`, in issue order: per launch the launch function (its address is the tag),
// the stream's slot (0 = the call's stream, g = side stream g - 1) and the object bytes of every argument, scalar or struct; per
// fork / join a null tag and the two slots.  Those bytes determine every kernel node of the captured graph, so they are the
// graph's key: argument structs are zero-filled before they are filled in and copied with memcpy, padding included.
struct Issuer {
  pocs_ctx* c;
  std::vector<unsigned char>* sig;                   // Sign mode; null: Issue mode, which does the work
  hipStream_t stream(int slot) const { return slot ? c->side_stream[slot - 1] : c->stream; }
  void put(const void* p, size_t n) { sig->insert(sig->end(), (const unsigned char*)p, (const unsigned char*)p + n); }
  template <class Fn, class... Args>
  int launch(Fn* fn, int slot, const Args&... args) {      // fn(args..., stream)
    if (sig) { put(&fn, sizeof fn); put(&slot, sizeof slot); (put(&args, sizeof args), ...); return POCS_OK; }
    HIPCHK(c, fn(args..., stream(slot)));
    return POCS_OK;
  }
  int order(int from, int to, hipEvent_t e, bool record = true) {      // fork / join: stream `to` waits for `e`, recorded on stream `from`
    if (sig) { const void* none = nullptr; put(&none, sizeof none); put(&from, sizeof from); put(&to, sizeof to); return POCS_OK; }
    if (record) HIPCHK(c, hipEventRecord(e, stream(from)));
    HIPCHK(c, hipStreamWaitEvent(stream(to), e, 0));
    return POCS_OK;
  }
  int mark(hipEvent_t e, int slot = 0) { if (!sig) HIPCHK(c, hipEventRecord(e, stream(slot))); return POCS_OK; }      // a profiling event: not signed
};

// The graph cache: leaves in `slot.exec` the graph of `enqueue`'s launches.  `enqueue` runs in Sign mode first: behind the call's
// stream handle its launches are the call's signature, and the cached graph is good while its own is the same, byte for byte.
// Otherwise the same function runs in Issue mode under capture.  A setter that changes no launch keeps the graph; a buffer that
// moved, another stream, a reconnected peer do not -- and nobody has to say so.
template <class Enqueue>
int ensure_graph(pocs_ctx* c, GraphSlot& slot, Enqueue enqueue) {
  c->sig.clear();
  Issuer{c, &c->sig}.put(&c->stream, sizeof c->stream);
  if (int r = enqueue(Issuer{c, &c->sig})) return r;
  if (slot.exec && c->sig == slot.sig) return POCS_OK;
  if (slot.exec) { hipGraphExecDestroy(slot.exec); slot.exec = nullptr; }
  hipGraph_t g = nullptr;
  HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  const int r = enqueue(Issuer{c, nullptr});
  hipError_t e = hipStreamEndCapture(c->stream, &g);
  if (r) { if (g) hipGraphDestroy(g); return r; }
  HIPCHK(c, e);
  e = hipGraphInstantiate(&slot.exec, g, nullptr, nullptr, 0);
  hipGraphDestroy(g);
  HIPCHK(c, e);
  slot.sig = c->sig; slot.captures += 1;
  return POCS_OK;
}
// Run a call's launches: eagerly (POCS_OPT_GRAPH = 0, or POCS_OPT_PROFILE = 1, whose events sit between the launches), or as the
// replay of their graph -- `span`: between the ev_seq pair (POCS_OPT_PROFILE = 2).
template <class Enqueue>
int run_launches(pocs_ctx* c, GraphSlot& slot, bool span, Enqueue enqueue) {
  if (!c->opt_graph || c->opt_profile == 1) return enqueue(Issuer{c, nullptr});
  if (int r = ensure_graph(c, slot, enqueue)) return r;
  if (span) HIPCHK(c, hipEventRecord(c->ev_seq[0], c->stream));
  HIPCHK(c, hipGraphLaunch(slot.exec, c->stream));
  if (span) HIPCHK(c, hipEventRecord(c->ev_seq[1], c->stream));
  return POCS_OK;
}

// ------------------------------------------------------------------------------------------
// GMM path
// ------------------------------------------------------------------------------------------
int gmm_shard(pocs_ctx* c, long long* first, long long* count) {
  *first = c->shard_first >= 0 ? c->shard_first : 0;
  *count = c->shard_first >= 0 ? c->shard_count : c->num_gmm;
  if (*first < 0 || *count < 0 || *first + *count > c->num_gmm)
    return fail(c, POCS_E_ARG, "shard [%lld,+%lld) outside numGMMSamples=%lld", *first, *count, c->num_gmm);
  if (*count > 2147480000LL)        // the kernels' positions inside a shard are 32-bit
    return fail(c, POCS_E_ARG, "a GMM shard holds at most 2147480000 samples per run (got %lld): shard the run", *count);
  if ((*first & 1) && *count > 0)   // mixture samples 2j, 2j+1 share their random draws: a shard starts on a pair
    return fail(c, POCS_E_ARG, "GMM shard must start at an even sample index (got %lld)", *first);
  return POCS_OK;
}

// A call of plans on the GMM path under a risk bound: the launches are k_gmm_step_risk (and never the lone form: a call of
// ONE plan takes the ticket form then, which computes the same bits -- tests/test_gpu_parity.py::test_lone_call_changes_no_bit).
// Off (the default, bound >= 1) and without plans nothing of a call changes: the same launches of the same kernels, the same
// memset, the same copies.
bool risk_active(const pocs_ctx* c) { return (c->plans.n > 0 || c->tree.n > 0) && c->risk_bound < 1.0; }

// Per-obstacle collision counts (POCS_OPT_OBSTACLE_COUNTS): d_obsct holds [batch][W][POCS_MAX_OBSTACLES] u64 (a tree: W = 1, one row
// per slot).  It is zeroed by the first launch of every call -- a kernel, inside the replayed graph -- and read by the getter
// (pocs_audit.hip).  Off: no buffer, no launch, and every launch is the kernel it has always been.
size_t obs_count_words(const pocs_ctx* c) { return (size_t)c->batch * (size_t)(c->W > 0 ? c->W : 1) * POCS_MAX_OBSTACLES; }
int ensure_obs_counts(pocs_ctx* c) {
  return c->opt_obs_counts ? ensure(c, c->d_obsct, obs_count_words(c) * sizeof(unsigned long long)) : POCS_OK;
}
int enqueue_obs_counts_reset(Issuer is) {
  pocs_ctx* c = is.c;
  if (!c->opt_obs_counts) return POCS_OK;
  return is.launch(pocs_launch_zero_counts, 0, (unsigned long long*)c->d_obsct.p, obs_count_words(c));
}
// what the getter needs to know of the call that has just filled the table (None with the option off)
void note_obs_counts(pocs_ctx* c, Kind kind) {
  c->res.oc_kind = c->opt_obs_counts ? kind : Kind::None;
  c->res.oc_M = world_boxes(c);
  c->res.oc_W = c->W > 0 ? c->W : 1;
}

// Clearance levels: d_clrct holds [batch][W][POCS_MAX_CLEARANCE_LEVELS] u64, zeroed by the first launch of every call they are applied
// to (a kernel, inside the replayed graph, as d_obsct) and read back behind the call (read_clearance).  Not applied: no buffer, no
// launch, and every launch is the kernel it is with L = 0.
size_t clear_count_words(const pocs_ctx* c) { return (size_t)c->batch * (size_t)(c->W > 0 ? c->W : 1) * POCS_MAX_CLEARANCE_LEVELS; }
int ensure_clearance(pocs_ctx* c) {
  return clearance_applied(c) ? ensure(c, c->d_clrct, clear_count_words(c) * sizeof(unsigned long long)) : POCS_OK;
}
int enqueue_clearance_reset(Issuer is) {
  pocs_ctx* c = is.c;
  if (!clearance_applied(c)) return POCS_OK;
  return is.launch(pocs_launch_zero_counts, 0, (unsigned long long*)c->d_clrct.p, clear_count_words(c));
}
// the state a call leaves for pocs_get_clearance_counts while it runs (or fails) ...
void open_clearance(pocs_ctx* c) {
  Results& r = c->res;
  r.cl_state = c->clr_L == 0 ? Results::ClOff : Results::ClNotApplied;
  r.cl_kind = Kind::None; r.cl_L = 0; r.cl_W = 0; r.cl_N = 0; r.cl_counts.clear();
}
// ... and behind its results: the table in slot order, as the device holds it (the stream is idle)
int read_clearance(pocs_ctx* c, Kind kind, long long n) {
  if (!clearance_applied(c)) return POCS_OK;
  Results& r = c->res;
  r.cl_counts.assign(clear_count_words(c), 0ull);
  HIPCHK(c, hipMemcpy(r.cl_counts.data(), c->d_clrct.p, r.cl_counts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  r.cl_state = Results::ClServed; r.cl_kind = kind; r.cl_L = c->clr_L; r.cl_W = c->W > 0 ? c->W : 1; r.cl_N = n;
  return POCS_OK;
}

// Watched regions: d_regct holds [batch][W][POCS_MAX_REGIONS] u64, zeroed by the first launch of every call they are applied to (a
// kernel, inside the replayed graph, as d_clrct) and read back behind the call (read_regions).  Not applied: no buffer, no launch,
// and every launch is the kernel it is with G = 0.
size_t region_count_words(const pocs_ctx* c) { return (size_t)c->batch * (size_t)(c->W > 0 ? c->W : 1) * POCS_MAX_REGIONS; }
int ensure_regions(pocs_ctx* c) {
  return regions_applied(c) ? ensure(c, c->d_regct, region_count_words(c) * sizeof(unsigned long long)) : POCS_OK;
}
// the state a call leaves for pocs_get_region_counts while it runs (or fails) ...
void open_regions(pocs_ctx* c) {
  Results& r = c->res;
  r.rg_state = c->reg_G == 0 ? Results::RgOff : Results::RgNotApplied;
  r.rg_kind = Kind::None; r.rg_G = 0; r.rg_W = 0; r.rg_N = 0; r.rg_counts.clear();
}
// ... and behind its results: the table in slot order, as the device holds it (the stream is idle)
int read_regions(pocs_ctx* c, Kind kind, long long n) {
  if (!regions_applied(c)) return POCS_OK;
  Results& r = c->res;
  r.rg_counts.assign(region_count_words(c), 0ull);
  HIPCHK(c, hipMemcpy(r.rg_counts.data(), c->d_regct.p, r.rg_counts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  r.rg_state = Results::RgServed; r.rg_kind = kind; r.rg_G = c->reg_G; r.rg_W = c->W > 0 ? c->W : 1; r.rg_N = n;
  return POCS_OK;
}

// Segment checks: d_segct holds the segment counts [batch][W] u64, zeroed by the first launch of every call under J > 1 (a kernel,
// inside the replayed graph, as d_regct) and read back behind the call (read_segment).  J = 1: no buffer, no launch, and every
// launch is the kernel it has always been.
size_t seg_count_words(const pocs_ctx* c) { return (size_t)c->batch * (size_t)(c->W > 0 ? c->W : 1); }
int ensure_segment(pocs_ctx* c) {
  return seg_applied(c) ? ensure(c, c->d_segct, seg_count_words(c) * sizeof(unsigned long long)) : POCS_OK;
}
// the state a call leaves for pocs_get_segment_counts while it runs (or fails) ...
void open_segment(pocs_ctx* c) {
  Results& r = c->res;
  r.sg_state = seg_applied(c) ? Results::SgNotServed : Results::SgOff;
  r.sg_kind = Kind::None; r.sg_J = c->seg_J; r.sg_W = 0; r.sg_counts.clear();
}
// ... and behind its results: the table in slot order, as the device holds it (the stream is idle)
int read_segment(pocs_ctx* c, Kind kind) {
  if (!seg_applied(c)) return POCS_OK;
  Results& r = c->res;
  r.sg_counts.assign(seg_count_words(c), 0ull);
  HIPCHK(c, hipMemcpy(r.sg_counts.data(), c->d_segct.p, r.sg_counts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  r.sg_state = Results::SgServed; r.sg_kind = kind; r.sg_J = c->seg_J; r.sg_W = c->W > 0 ? c->W : 1;
  return POCS_OK;
}

// The call's synchronisation words (SyncLayout, pocs_ctx.hpp); the copy behind the launches starts at the give-up word and,
// under a risk bound, runs on through the pad and the stop words.
SyncLayout sync_layout(const pocs_ctx* c) {
  static_assert(POCS_SYNC_ABORT < 4, "the give-up word lies ahead of the stop words");
  SyncLayout s;
  const size_t R = (size_t)c->batch, stops = risk_active(c) ? R : 0;
  s.cells = R * (size_t)(c->W > 0 ? c->W : 1);
  s.ticket = s.stop + ((stops + 3) & ~(size_t)3);
  s.xwait = s.ticket + s.cells;
  s.words = (s.xwait + s.cells + 3) & ~(size_t)3;
  s.pin = pin_layout(c).total + R + 1;
  s.copy_words = stops ? s.stop - POCS_SYNC_ABORT + stops : 1;
  return s;
}

int gmm_prepare(pocs_ctx* c) {
  if (int r = check_common(c)) return r;
  if (c->K < 1) return fail(c, POCS_E_STATE, "setNumGaussians missing");
  if (c->num_gmm < 1) return fail(c, POCS_E_STATE, "setNumGMMSamples missing");
  long long first, count;
  if (int r = gmm_shard(c, &first, &count)) return r;
  if (int r = upload_static(c)) return r;
  const size_t W = (size_t)c->W, K = (size_t)c->K, R = (size_t)c->batch;
  const GmmGeometry geo = gmm_geometry(count, c->batch, c->K);
  if (int r = ensure(c, c->d_hdr, R * sizeof(pocs_run_header))) return r;
  if (int r = ensure(c, c->d_chain, R * (W > 1 ? W - 1 : 1) * POCS_CHAIN_STRIDE * sizeof(double))) return r;
  if (int r = ensure(c, c->d_state, R * W * K * POCS_STATE_STRIDE * sizeof(double))) return r;
  if (int r = ensure(c, c->d_param, R * W * K * POCS_PARAM_STRIDE * sizeof(double))) return r;
  if (!c->ext_moments)
    if (int r = ensure(c, c->d_moments, W * R * K * POCS_NMOM * sizeof(double))) return r;
  if (c->ext_moments && c->ext_moments_len < (long long)(W * R * K * POCS_NMOM))
    return fail(c, POCS_E_BUFFER, "bound moments buffer too small");
  // (x 2: a lone call alternates halves; a tree: its launches cover at most 256 nodes and use the rows one after the other)
  if (int r = ensure(c, c->d_partial, 2 * ((c->tree.n && R > 256 ? (size_t)256 : R) << geo.vs_shift) * K * POCS_NMOM * sizeof(double))) return r;
  c->sync = sync_layout(c);
  if (int r = ensure(c, c->d_ticket, c->sync.words * sizeof(unsigned))) return r;
  if (c->plans.n)
    if (int r = ensure(c, c->d_runplan, R * 4 * sizeof(double))) return r;
  if (risk_active(c))
    if (int r = ensure(c, c->d_surv, R * sizeof(double))) return r;
  if (c->tree.n)
    if (int r = upload_tree(c)) return r;
  if (int r = ensure_obs_counts(c)) return r;
  if (int r = ensure_clearance(c)) return r;
  if (int r = ensure_regions(c)) return r;
  if (int r = ensure_segment(c)) return r;
  if (large_world(c)) {
    if (int r = ensure(c, c->d_kept, R * POCS_MAX_OBSTACLES * POCS_OBS_STRIDE * sizeof(double))) return r;
    if (int r = ensure(c, c->d_keptidx, R * POCS_MAX_OBSTACLES * sizeof(int))) return r;
    if (int r = ensure(c, c->d_reach, R * W * sizeof(int))) return r;
  }
  if (c->opt_store && !c->tree.n) {                   // (a call on a tree stores no samples)
    const size_t n = R * (size_t)sample_stride_of(count);
    if (int r = ensure(c, c->d_sx, n * sizeof(double))) return r;
    if (int r = ensure(c, c->d_sy, n * sizeof(double))) return r;
    if (int r = ensure(c, c->d_st, n * sizeof(double))) return r;
    if (int r = ensure(c, c->d_flags, n * sizeof(int16_t))) return r;
  }
  return ensure_pin(c);
}

// Sub-batches of a whole-run call.  The moment sums do not depend on the launch shape (pocs_dev_gmm.hpp,
// "summation tree"), so a split changes no bit of any result.  TWO sub-batches on two streams by default where a call
// has the work for it (round 4, measured on MI355X with numerics v8, 10^6 samples, K = 3, one box, three alternations and
// a sweep, profiles/r04_sub_batches.txt): while one sub-batch is in the tail of its waypoint -- the slow end of its last
// blocks, the serial mixture advance of its last closer, the launch boundary, the next launch's heads -- the other's
// sampling blocks have the chip: +11 % at 8 runs per call, +7 % at 16 and 20, +6 % at 32, +4 % at 64; K = 8, 10^7
// samples, 16 runs: +4 %.  Below 8 runs per call a launch of half the runs does not fill the chip (-5 ... -23 % at 2 ... 6
// runs), and launches of less than ~6 x 10^5 evaluations are all dispatch (64 runs of 10^4 samples: -15 %): one launch
// for all then.  Three sub-batches lose everywhere, four gain less than two.  (Round 3 had measured +0.5 % at 20 runs
// for the same split and left it off: its closers were a third longer and it timed one pass, not a median.)
// POCS_OPT_SUB_BATCHES: 0 = this rule (default), 1, 2 (tests/test_gpu_parity.py checks the bits).
int gmm_groups(const pocs_ctx* c) {
  if (c->ext_moments) return 1;                      // the caller's all-reduce covers the whole batch at once
  if (c->tree.n) return 1;                           // a tree's levels depend on each other: one stream
  int g = (int)c->opt_groups;
  if (g == 0) {
    const double count = (double)(c->shard_first >= 0 ? c->shard_count : c->num_gmm);
    g = (c->batch >= 8 && (double)c->batch * count >= 1.2e6) ? 2 : 1;
  }
  if (g > c->batch) g = c->batch;
  return g < 1 ? 1 : g;
}

int gmm_upload_run(pocs_ctx* c) {
  if (int r = stage_and_upload_runs(c, gmm_groups(c), Kind::Gmm)) return r;
  const PinLayout pl = pin_layout(c);
  double* pin = (double*)c->h_pin;
  const int W = c->W, R = c->batch;
  // the initial mixture of run r goes to state[r][0]: R rows of K*16 doubles, pitch W*K*16
  const size_t row = (size_t)c->K * POCS_STATE_STRIDE * sizeof(double);
  HIPCHK(c, hipMemcpy2DAsync(c->d_state.p, (size_t)W * row, pin + pl.state0, row, row, (size_t)(c->tree.n ? 1 : R),     // (a tree: the root's)
                             hipMemcpyHostToDevice, c->stream));
  return POCS_OK;
}

// A whole-run call of a context that is CONNECTED to its peers (pocs_xchg_connect) and holds a shard exchanges every
// run's moments in the closing block of its launch (k_gmm_step, exchange_in_tail): the call is then the sharded
// estimation in ONE library call -- the same graph replay, the same two sub-batches as on one GPU, no host in the loop.
// Only the whole-run call (enqueue_gmm_all) asks enqueue_step for that exchange: the step API's sample launches
// (pocs_gmm_sample_local / pocs_gmm_step_local) leave the shard's sums to the caller's exchange, whatever the context.
bool whole_call_exchanges(const pocs_ctx* c) { return c->xchg_connected && c->shard_first >= 0 && !c->ext_moments; }

// The collision world as a GMM launch carries it (upload_world has put it on the device): what the obstacle cull and the
// collision test of k_gmm_step read -- and all that pocs_probe_device_collide's one-block launch reads besides its mixture.
// `w`: the launch's waypoint, which picks the step of an obstacle schedule (the probe: world 0).
void fill_gmm_world(const pocs_ctx* c, pocs_gmm_launch* a, int w) {
  a->env = world_at(c, w);
  a->tables = (const pocs_tables*)c->d_tables.p;
  a->M = env_records(c);                             // (the boxes, and behind them the discs in force)
  a->round = discs_applied(c) ? 1 : 0;               // (nonzero: the sampling launch is the _round form)
  a->noise = noise_rows_held(c) ? noise_at(c, w) : nullptr;      // (non-null: the _noise form on top of it)
  a->gates = hyp_applied(c) ? (const uint32_t*)c->d_gates.p : nullptr;      // (non-null: the _hyp form on top of that, rows of zeros where there are no covariances)
  a->rfoot = rfoot_applied(c) ? 1 : 0;               // (nonzero: the _rfoot family, with or without discs and covariances)
  if (!parts_applied(c)) {                           // (a compound footprint's values live in device memory: the launch carries none)
    a->fp = c->fp;
    a->fp_rr = sqrt(c->fp.hx * c->fp.hx + c->fp.hy * c->fp.hy); a->fp_phi = atan2(c->fp.hy, c->fp.hx);
  }
  if (large_world(c)) {                              // (M above is 0 then: the staged table is empty)
    a->world = (const double*)c->d_world.p; a->world_M = large_boxes(c);
    a->kept = (double*)c->d_kept.p; a->kept_idx = (int*)c->d_keptidx.p; a->reach = (int*)c->d_reach.p;
  }
}

// What the GMM launches of a call share: filled once per call, and every launch is a memcpy of it aimed at its waypoint and runs.
void fill_gmm_launch(pocs_ctx* c, pocs_gmm_launch* a, long long first, long long count) {
  memset(a, 0, sizeof *a);
  a->hdr = (const pocs_run_header*)c->d_hdr.p;
  fill_gmm_world(c, a, 0);
  a->chain = (const double*)c->d_chain.p;
  a->sensor = (const pocs_sensor*)c->d_sensor.p;
  a->state = (double*)c->d_state.p;
  a->param = (double*)c->d_param.p;
  a->moments = moments_dev(c);
  a->partial = (double*)c->d_partial.p;
  a->partial_prev = a->partial;
  a->sync = (unsigned*)c->d_ticket.p;
  a->ticket = a->sync + c->sync.ticket;
  a->xwait = a->sync + c->sync.xwait;
  a->x = (double*)c->d_sx.p; a->y = (double*)c->d_sy.p; a->th = (double*)c->d_st.p;
  a->flags = (int16_t*)c->d_flags.p;
  a->first = first; a->count = count; a->n_total = c->num_gmm;
  a->store = c->opt_store ? 1 : 0;
  a->sample_stride = sample_stride_of(count);
  a->nruns = c->batch; a->W = c->W;
  a->obs_counts = c->opt_obs_counts ? (unsigned long long*)c->d_obsct.p : nullptr;      // (non-null: the sampling launch is the counting form)
}
// `w`: the waypoint (a tree: the level's depth), which picks the step of an obstacle schedule; runs [run_lo, run_lo + run_cnt)
// (run_cnt < 0: the batch), with the geometry of a launch that shares the chip with `groups` - 1 others.
void aim_gmm_launch(const pocs_ctx* c, pocs_gmm_launch* a, int w, int run_lo = 0, int run_cnt = -1, int groups = 1) {
  if (run_cnt < 0) run_cnt = c->batch;
  a->env = world_at(c, w); a->waypoint = w;
  if (a->noise) a->noise = noise_at(c, w);           // (uncertain discs: the rows of the same step)
  if (a->clr) a->clr = clear_at(c, w);               // (the clearance form: the record of the same step)
  const GmmGeometry geo = gmm_geometry(a->count, run_cnt, c->K, groups);
  a->chunks = geo.chunks; a->vs_shift = geo.vs_shift; a->upb = geo.upb; a->blocks = geo.blocks;
  a->run_lo = run_lo; a->run_cnt = run_cnt;
}

// The exchange of waypoint w's moments with the connected peers.  `epoch_from_headers`: the kernel forms the rows' epoch and the
// slot set's parity itself, from the call number in the run headers (a whole call replayed from a graph bakes its arguments in).
void fill_xchg(const pocs_ctx* c, pocs_xchg_dev* x, int w, bool epoch_from_headers) {
  memset(x, 0, sizeof *x);
  for (int q = 0; q < c->xchg_world; ++q) x->buf[q] = (double*)c->xchg_peer[q];
  x->world = c->xchg_world; x->rank = c->xchg_rank;
  if (epoch_from_headers) return;
  x->epoch = (c->xchg_calls << 20) | (unsigned long long)(w + 1);
  x->parity = (int)((c->xchg_calls * (unsigned long long)c->W + (unsigned long long)w) & 1ull);
}

// state/param[w] from state/moments[w-1]: its own tiny launch for waypoint 0 and, when sharded,
// after the caller's all-reduce; on one GPU the last block of k_gmm_step(w-1) has done it already.
int enqueue_advance(Issuer is, int w) {
  pocs_gmm_launch a;
  fill_gmm_launch(is.c, &a, 0, 0);
  aim_gmm_launch(is.c, &a, w);
  return is.launch(pocs_launch_gmm_advance, 0, is.c->K, a);
}

// One run per call (no batch, no run-ahead) on one GPU: the launches close the previous waypoint in their heads
// (k_gmm_step, "LONE"): 30.6 -> 27.5 us per waypoint at 10^6 samples, K = 3 (MI355X).  POCS_OPT_LONE_CALL = 0
// keeps the ticket-and-closer form; the results are the same bits.
// (Under a large world the cull of waypoint w reads param[w] ahead of the sampling launch; the lone form builds param[w] in its own
// heads, so a call of one run takes the ticket form there: the same bits.)
// (Under clearance levels and watched regions too: the counting forms exist as the ticket form only.)
// (And under a compound footprint: the parts form exists as the ticket form only.  And under segment checks and discs: the same.)
bool lone_call(const pocs_ctx* c) { return c->opt_lone && !large_world(c) && !clearance_applied(c) && !regions_applied(c) && !parts_applied(c) && !seg_applied(c) && !discs_applied(c) && !rfoot_applied(c) && c->batch == 1 && !c->tree.n && !c->ext_moments && !(c->xchg_connected && c->shard_first >= 0) && !risk_active(c); }
void set_risk(pocs_ctx* c, pocs_gmm_launch* a) {      // under a risk bound the launch is k_gmm_step_risk (whole calls of plans or on a tree only)
  a->risk = 1;
  a->stop = a->sync + c->sync.stop;
  a->surv = (double*)c->d_surv.p;
  a->risk_bound = c->risk_bound;
}
void set_lone(pocs_ctx* c, pocs_gmm_launch* a, int w) {
  const size_t half = ((size_t)1 << a->vs_shift) * c->K * POCS_NMOM;      // one run's rows
  a->lone = 1;
  a->advance_in_tail = 0;
  a->partial = (double*)c->d_partial.p + (size_t)(w & 1) * half;
  a->partial_prev = (double*)c->d_partial.p + (size_t)((w + 1) & 1) * half;
}

// The launches of one waypoint for one sub-batch of a call, or for the step API's batch.
struct StepLaunch {
  int slot = 0;                                      // the stream: 0 = the call's, g = side stream g - 1
  int run_lo = 0, run_cnt = -1, groups = 1;          // the runs (run_cnt < 0: the batch), the launches that share the chip
  bool advance = false;                              // the closers build the next waypoint's mixture in the launch's tail ...
  int adv_cnt = -1;                                  // ... of the first adv_cnt runs only (a call of plans: the others end here); < 0: all
  enum { NONE, FROM_CONTEXT, FROM_HEADERS } exchange = NONE;      // ... behind the moments' exchange with the peers; the call's number from the
  bool lone = false, risk = false;                   // context (step API) or the run headers (the whole-run call ONLY, above).  The lone form;
  int prof_slot = -1;                                // k_gmm_step_risk (whole calls of plans only).  >= 0: profiling events around the sampling launch
};
int enqueue_step(Issuer is, const pocs_gmm_launch& base, int w, const StepLaunch& s) {
  pocs_ctx* c = is.c;
  pocs_gmm_launch a;
  memcpy(&a, &base, sizeof a);
  aim_gmm_launch(c, &a, w, s.run_lo, s.run_cnt, s.groups);
  a.advance_in_tail = (s.advance && w + 1 < c->W) ? a.run_lo + (s.adv_cnt >= 0 ? s.adv_cnt : a.run_cnt) : 0;   // (the runs below it advance)
  if (s.lone) set_lone(c, &a, w);
  if (s.risk) set_risk(c, &a);
  if (s.exchange != StepLaunch::NONE) {
    a.exchange_in_tail = 1;
    a.xchg_epoch_from_header = s.exchange == StepLaunch::FROM_HEADERS;
    fill_xchg(c, &a.xchg, w, a.xchg_epoch_from_header);
  }
  if (a.world) if (int r = is.launch(pocs_launch_world_cull, s.slot, c->K, a)) return r;      // a large world: cull(w) in front of step(w), same stream, same runs
  if (s.prof_slot >= 0) if (int r = is.mark(c->events[2 * s.prof_slot], s.slot)) return r;
  if (int r = is.launch(pocs_launch_gmm_step, s.slot, c->K, a)) return r;
  if (s.prof_slot >= 0) if (int r = is.mark(c->events[2 * s.prof_slot + 1], s.slot)) return r;
  return POCS_OK;
}

int enqueue_ticket_reset(pocs_ctx* c) {
  HIPCHK(c, hipMemsetAsync(c->d_ticket.p, 0, c->sync.words * sizeof(unsigned), c->stream));
  if (large_world(c))                                // (a waypoint that no cull launch covers -- a plan's end, a stop -- reports no reach)
    HIPCHK(c, hipMemsetAsync(c->d_reach.p, 0, (size_t)c->batch * (size_t)c->W * sizeof(int), c->stream));
  return POCS_OK;
}

// How many launches of the hot kernel one whole-run call makes (what POCS_OPT_PROFILE brackets).
size_t gmm_hot_launches(const pocs_ctx* c) { return (size_t)c->W; }

// The launches of a whole-run call: what the hipGraph holds.  KERNEL NODES ONLY -- the ticket reset ahead of
// them and the result copies behind them are plain stream operations (enqueue_gmm_results).  On ROCm 7.2 a
// captured graph that also held the memset and the two device-to-host copies went stale between replays: after
// a few dozen small synchronous copies plus a large one on the null stream (a caller reading mixture states
// and samples back between two runs), the next replay's memset no longer cleared the tickets and its kernels
// ran on garbage -- reproduced with round 2's library, gone with kernel-only graphs (tests/test_gpu_parity.py
// ::test_graph_replays_survive_readbacks).
// A call on a tree of plans: per level d an advance launch that builds the mixtures of the level's nodes from their parents'
// rows (k_gmm_tree_advance), then the sampling launch over those nodes -- the ticket-and-closer form without an advance in its
// tail, whose closers leave the nodes' moments (k_gmm_step_tree) -- a level wider than 256 nodes as several launches of at most
// 256.  The launches of a level read what the launches of the level above wrote: one stream, one after the other.  A launch's
// rows of partial sums start at the head of the row buffer whatever its first slot is (the kernels address them by slot).
int enqueue_gmm_tree(Issuer is, long long count) {
  pocs_ctx* c = is.c;
  const int D = (int)c->tree.level.size() - 2;
  if (int r = enqueue_obs_counts_reset(is)) return r;
  pocs_gmm_launch base, a;
  fill_gmm_launch(c, &base, 0, count);
  base.store = 0; base.tree_parent = (const int*)c->d_tparent.p;
  if (risk_active(c)) set_risk(c, &base);
  auto tree_launch = [&](int d, int lo, int cnt) {
    memcpy(&a, &base, sizeof a);
    aim_gmm_launch(c, &a, d, lo, cnt);
    a.partial = (double*)((uintptr_t)c->d_partial.p - (uintptr_t)(((size_t)lo << a.vs_shift) * (size_t)c->K * POCS_NMOM * sizeof(double)));
    a.partial_prev = a.partial;
  };
  for (int d = 0; d <= D; ++d) {
    const int lo = c->tree.level[(size_t)d], hi = c->tree.level[(size_t)d + 1];
    tree_launch(d, lo, hi - lo);
    if (int r = is.launch(pocs_launch_gmm_tree_advance, 0, c->K, a)) return r;
    for (int s = lo; s < hi; s += 256) {
      tree_launch(d, s, hi - s < 256 ? hi - s : 256);
      if (int r = is.launch(pocs_launch_gmm_tree_step, 0, c->K, a)) return r;
    }
  }
  return POCS_OK;
}

int enqueue_gmm_all(Issuer is, long long first, long long count, bool prof) {
  pocs_ctx* c = is.c;
  if (c->tree.n) return enqueue_gmm_tree(is, count);
  const int W = c->W, R = c->batch, G = gmm_groups(c);
  if (int r = enqueue_obs_counts_reset(is)) return r;    // (ahead of the fork: every sub-batch's launches lie behind it)
  if (int r = enqueue_clearance_reset(is)) return r;
  if (regions_applied(c)) if (int r = is.launch(pocs_launch_zero_counts, 0, (unsigned long long*)c->d_regct.p, region_count_words(c))) return r;
  if (seg_applied(c)) if (int r = is.launch(pocs_launch_zero_counts, 0, (unsigned long long*)c->d_segct.p, seg_count_words(c))) return r;
  if (int r = enqueue_advance(is, 0)) return r;
  if (prof) if (int r = is.mark(c->ev_seq[0])) return r;
  for (int g = 1; g < G; ++g) if (int r = is.order(0, g, c->ev_fork, g == 1)) return r;
  pocs_gmm_launch base;
  fill_gmm_launch(c, &base, first, count);
  if (parts_applied(c)) { base.parts = (const pocs_parts_dev*)c->d_parts.p; base.parts_F = c->fp_F; }
  if (clearance_applied(c)) {                        // (the whole call only: the step API's launches never carry the levels)
    base.clr = clear_at(c, 0); base.clr_counts = (unsigned long long*)c->d_clrct.p; base.clr_L = c->clr_L;
  }
  if (seg_applied(c)) {                              // (the whole call only: the step API is refused under J > 1)
    base.seg = (const pocs_seg_dev*)c->d_seg.p; base.seg_counts = (unsigned long long*)c->d_segct.p;
  }
  if (regions_applied(c)) {                          // (the whole call only, as the levels)
    base.regions = (const pocs_regions_dev*)c->d_reg.p; base.reg_counts = (unsigned long long*)c->d_regct.p; base.reg_G = c->reg_G;
  }
  StepLaunch s;
  s.groups = G; s.advance = true; s.lone = lone_call(c); s.risk = risk_active(c);
  if (whole_call_exchanges(c)) s.exchange = StepLaunch::FROM_HEADERS;
  // a call of plans: the launch of waypoint w covers the runs whose plan is longer than w -- a prefix of every
  // sub-batch's slots (plan_layout) -- and the closers of those whose plan ends at w do not advance
  const std::vector<int> Ws = slot_lengths(c, plan_layout(c, G));
  for (int w = 0; w < W; ++w)
    for (int g = 0; g < G; ++g) {                    // sub-batch g = runs [g R / G, (g + 1) R / G); events bracket sub-batch 0's launches
      const int lo = (int)((long long)g * R / G), hi = (int)((long long)(g + 1) * R / G);
      s.slot = g; s.run_lo = lo; s.run_cnt = hi - lo; s.adv_cnt = -1; s.prof_slot = (prof && g == 0) ? w : -1;
      if (c->plans.n) {
        s.run_cnt = live_runs(Ws, lo, hi, w);
        s.adv_cnt = live_runs(Ws, lo, hi, w + 1);
        if (s.run_cnt == 0) {                        // this sub-batch's plans have all ended
          if (s.prof_slot >= 0) { if (int r = is.mark(c->events[2 * w])) return r; if (int r = is.mark(c->events[2 * w + 1])) return r; }
          continue;
        }
      }
      if (int r = enqueue_step(is, base, w, s)) return r;
    }
  if (s.lone) {                                      // the last waypoint's rows -> moments[W-1]
    aim_gmm_launch(c, &base, W - 1, 0, 1, 1);
    set_lone(c, &base, W - 1);
    if (int r = is.launch(pocs_launch_gmm_close, 0, c->K, base)) return r;
  }
  for (int g = 1; g < G; ++g) if (int r = is.order(g, 0, c->ev_join[g - 1])) return r;
  if (prof) if (int r = is.mark(c->ev_seq[1])) return r;
  return POCS_OK;
}
int enqueue_gmm_results(pocs_ctx* c) {
  const int W = c->W;
  const PinLayout pl = pin_layout(c);
  HIPCHK(c, hipMemcpyAsync((double*)c->h_pin + pl.moments, moments_dev(c),
                           (size_t)W * c->batch * c->K * POCS_NMOM * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  // the call's give-up word travels back with the results -- and, under a risk bound, the runs' stop words behind it (SyncLayout)
  HIPCHK(c, hipMemcpyAsync((double*)c->h_pin + c->sync.pin, (unsigned*)c->d_ticket.p + POCS_SYNC_ABORT,
                           c->sync.copy_words * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  if (large_world(c)) {                              // the kept counts [R][W]: into the context's own table, slot order (gmm_read_reach sorts them)
    c->reach.assign((size_t)c->batch * (size_t)c->W, 0);
    HIPCHK(c, hipMemcpyAsync(c->reach.data(), c->d_reach.p, c->reach.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  }
  return POCS_OK;
}

// A bounded wait that expired on the device fails the call that has just synchronised (`what`: the caller's message, with %u).
int gmm_check_gave_up(pocs_ctx* c, const char* what) {
  unsigned gave_up = 0;
  memcpy(&gave_up, (double*)c->h_pin + c->sync.pin, sizeof gave_up);
  return gave_up ? fail(c, POCS_E_DEVICE, what, gave_up) : POCS_OK;
}

// The kept counts of a GMM call under a large world, as enqueue_gmm_results brought them back in slot order -> run / plan order
// (pocs_get_world_reach), and the overflow check: a (run, waypoint) whose cull kept more than POCS_MAX_OBSTACLES records was sampled
// against the first POCS_MAX_OBSTACLES of them only, so the call fails -- naming the lowest such waypoint and its count.  The table
// it leaves stays readable.
int gmm_read_reach(pocs_ctx* c) {
  const int R = c->batch, W = c->W;
  const bool plans = c->plans.n && !c->res.plan_slot(Kind::Gmm).empty();
  const std::vector<int> by_slot = c->reach;
  c->reach_R = R; c->reach_W = W;
  c->reach_len.assign((size_t)R, W);
  int bad_w = -1, bad_n = 0, bad_r = 0;
  for (int r = 0; r < R; ++r) {
    const int slot = plans ? c->res.plan_slot(Kind::Gmm)[(size_t)r] : r;
    if (plans) c->reach_len[(size_t)r] = c->plans.W[(size_t)r];
    for (int w = 0; w < W; ++w) {
      const int n = by_slot[(size_t)slot * W + w];
      c->reach[(size_t)r * W + w] = n;
      if (n > POCS_MAX_OBSTACLES && (bad_w < 0 || w < bad_w)) { bad_w = w; bad_n = n; bad_r = r; }
    }
  }
  if (bad_w >= 0)
    return fail(c, POCS_E_STATE, "large world: %d boxes are in reach of run %d at waypoint %d, more than the %d a run may meet at one waypoint; results discarded",
                bad_n, bad_r, bad_w, POCS_MAX_OBSTACLES);
  return POCS_OK;
}

// F1 (MCSimulator.h:848-856): p_w = colliding / numGMMSamples (:633-641), result = 1 - prod(1 - p_w)
// p_w from one waypoint's moments row [K][POCS_NMOM]: the components' colliding counts added in component order, then divided.
// The order of these operations is part of the numerics: k_gmm_step_risk restates it on the device.
double waypoint_probability(const double* row, int K, long long n) {
  double coll = 0.0;
  for (int k = 0; k < K; ++k) coll += row[(size_t)k * POCS_NMOM + 1];
  return coll / (1.0 * (double)n);
}

// The getters' view of the last GMM launch: per-waypoint probabilities and moments of run v.
// (a call of plans: v is the plan, which the moments hold in its batch slot, over its own W_p waypoints)
void gmm_select_view(pocs_ctx* c, int v) {
  const bool plans = c->plans.n && !c->res.plan_slot(Kind::Gmm).empty();
  // (a plan stopped by the risk bound: its E[v] evaluated waypoints -- what lies behind them is whatever an earlier call left)
  const int W = plans ? ((size_t)v < c->res.plan_E.size() ? c->res.plan_E[(size_t)v] : c->plans.W[(size_t)v]) : c->W, K = c->K, R = c->res.batch_R;
  const int slot = plans ? c->res.plan_slot(Kind::Gmm)[(size_t)v] : v;
  c->res.view = v;
  c->res.probs.assign(W, 0.0);
  c->res.last_moments.assign((size_t)W * K * POCS_NMOM, 0.0);
  for (int w = 0; w < W; ++w) {
    const double* m = &c->res.batch_moments[((size_t)w * R + slot) * K * POCS_NMOM];
    c->res.probs[w] = waypoint_probability(m, K, c->num_gmm);
    memcpy(&c->res.last_moments[(size_t)w * K * POCS_NMOM], m, (size_t)K * POCS_NMOM * sizeof(double));
  }
}

// `stop` (a whole call of plans under a risk bound, else null): the device's stop word of every batch slot -- 0, or s + 1 for
// a run whose closer of waypoint s found the running probability at the bound.  The rule is restated here on the moments read
// back: plan p stops at the FIRST waypoint s with c_s = 1 - prod_{v <= s} (1 - p_v) >= bound, E[p] = s + 1 waypoints were
// evaluated and its probability is c_s; the moments past E[p] - 1 are not read.  Device and host form c_s with the same
// operations in the same order; if the two stops ever differ the call fails instead of reporting either.
// The getters' view of a node of the last GMM call on a tree: the path root -> n as a plan of depth(n) + 1 waypoints (its
// evaluated part, where the risk bound has cut the path off above n).
void tree_select_gmm(pocs_ctx* c, int n) {
  const int K = c->K;
  std::vector<int> path;
  for (int v = n; v >= 0; v = c->tree.parent[(size_t)v]) if (c->res.tree_eval[(size_t)v]) path.push_back(v);
  std::reverse(path.begin(), path.end());
  c->res.tree_sel = n;
  c->res.probs.assign(path.size(), 0.0);
  c->res.last_moments.assign(path.size() * (size_t)K * POCS_NMOM, 0.0);
  for (size_t w = 0; w < path.size(); ++w) {
    const double* m = &c->res.batch_moments[(size_t)c->tree.slot[(size_t)path[w]] * K * POCS_NMOM];
    c->res.probs[w] = waypoint_probability(m, K, c->num_gmm);
    memcpy(&c->res.last_moments[w * (size_t)K * POCS_NMOM], m, (size_t)K * POCS_NMOM * sizeof(double));
  }
}

// A call on a tree: moments [T][K*11] and -- under a risk bound -- the stop words [T], both by slot.  Every node's running
// probability is its parent's survival product times its own (1 - p), formed as gmm_combine forms a plan's: the same operations
// in the same order as along the path root -> n.  The bound's rule is restated on what came back: a node is evaluated unless an
// ancestor's running probability has reached the bound; the device's word of every node must say the same (0, depth + 1 at
// the bound, the inherited mark below it), or the call fails.
int gmm_combine_tree(pocs_ctx* c, const double* moments, double* probability, const unsigned* stop) {
  const int T = c->tree.n, K = c->K;
  c->res.batch_R = T;
  c->res.last_kind = Kind::Gmm;
  c->res.batch_moments.assign(moments, moments + (size_t)T * K * POCS_NMOM);
  c->res.plan_E.clear();
  c->res.tree_probs.assign((size_t)T, 0.0);
  c->res.tree_eval.assign((size_t)T, 1);
  std::vector<double> prod((size_t)T, 1.0);
  std::vector<unsigned char> cut((size_t)T, 0);        // the node, or an ancestor, is at the bound: nothing below is evaluated
  for (int n = 0; n < T; ++n) {
    const size_t slot = (size_t)c->tree.slot[(size_t)n];
    const int p = c->tree.parent[(size_t)n], depth = c->tree.depth[(size_t)n];
    const unsigned dev = stop ? stop[slot] : 0u;
    if (p >= 0 && cut[(size_t)p]) {
      if (!(dev & POCS_TREE_STOP_INHERITED))
        return fail(c, POCS_E_DEVICE, "risk bound: node %d lies below a stopped node, the device's word for it is %u; results discarded", n, dev);
      c->res.tree_eval[(size_t)n] = 0; cut[(size_t)n] = 1;
      prod[(size_t)n] = prod[(size_t)p];
      c->res.tree_probs[(size_t)n] = c->res.tree_probs[(size_t)p];
      continue;
    }
    const double pw = waypoint_probability(moments + slot * K * POCS_NMOM, K, c->num_gmm);
    double pr = p >= 0 ? prod[(size_t)p] : 1.0;
    pr *= (1.0 - pw);
    prod[(size_t)n] = pr;
    const unsigned host = (stop && 1.0 - pr >= c->risk_bound) ? (unsigned)depth + 1u : 0u;
    if (host != dev)
      return fail(c, POCS_E_DEVICE, "risk bound: node %d (depth %d): stop word %u on the device, %u on the host; results discarded", n, depth, dev, host);
    cut[(size_t)n] = host != 0u;
    c->res.tree_probs[(size_t)n] = 1.0 - pr;
  }
  c->res.batch_probs.assign(1, c->res.tree_probs[0]);
  c->res.view = 0;
  tree_select_gmm(c, 0);
  *probability = c->res.tree_probs[0];
  return POCS_OK;
}

int gmm_combine(pocs_ctx* c, const double* moments, double* probability, const unsigned* stop = nullptr) {
  if (c->tree.n) return gmm_combine_tree(c, moments, probability, stop);
  const int W = c->W, K = c->K, R = c->batch;          // moments: [W][R][K*11]
  c->res.batch_R = R;
  c->res.last_kind = Kind::Gmm;
  c->res.batch_moments.assign(moments, moments + (size_t)W * R * K * POCS_NMOM);
  c->res.batch_probs.assign(R, 0.0);
  const bool plans = c->plans.n && !c->res.plan_slot(Kind::Gmm).empty();
  if (plans) c->res.plan_E = c->plans.W; else c->res.plan_E.clear();
  for (int r = 0; r < R; ++r) {                        // (a call of plans: r is the plan, in its slot, over its W_p waypoints)
    const int slot = plans ? c->res.plan_slot(Kind::Gmm)[(size_t)r] : r, Wr = plans ? c->plans.W[(size_t)r] : W;
    const int dev = stop ? (int)stop[(size_t)slot] : 0;
    if (dev < 0 || dev > Wr) return fail(c, POCS_E_DEVICE, "risk bound: the device stopped plan %d at waypoint %d of %d; results discarded", r, dev - 1, Wr);
    const int Er = dev ? dev : Wr;
    int host = 0;                                      // the host's stop word
    double prod = 1.0;
    for (int w = 0; w < Er; ++w) {
      const double p = waypoint_probability(moments + ((size_t)w * R + slot) * K * POCS_NMOM, K, c->num_gmm);
      prod *= (1.0 - p);
      if (stop && 1.0 - prod >= c->risk_bound) { host = w + 1; break; }
    }
    if (host != dev)
      return fail(c, POCS_E_DEVICE, "risk bound: plan %d stops at waypoint %d on the device and at %d on the host (-1: not at all); results discarded",
                  r, dev - 1, host - 1);
    c->res.batch_probs[r] = 1.0 - prod;
    if (plans) c->res.plan_E[(size_t)r] = Er;
  }
  gmm_select_view(c, 0);
  *probability = c->res.batch_probs[0];
  return POCS_OK;
}

int run_gmm_full(pocs_ctx* c, double* probability) {
  if (!probability) return fail(c, POCS_E_ARG, "null output");
#if defined(POCS_TUNING) && defined(POCS_CALL_TIMES)                          // tuning build: host-side phases of a call on stderr
  const auto t_in = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) { fprintf(stderr, "[call] %s +%.1f us\n", what,
      std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_in).count()); };
#else
  auto lap = [](const char*) {};
#endif
  c->res.oc_kind = Kind::None;                                  // (the per-obstacle table is rewritten from here on; noted again behind the combine)
  open_clearance(c);
  open_regions(c);
  open_segment(c);
  c->reach.clear(); c->reach_len.clear(); c->reach_R = 0; c->reach_W = 0;      // (pocs_get_world_reach covers the last GMM call)
  if (int r = gmm_prepare(c)) return r;
  long long first, count;
  if (int r = gmm_shard(c, &first, &count)) return r;
  lap("prepared");
  if (whole_call_exchanges(c)) {
    if (c->batch > POCS_XCHG_MAX_RUNS) return fail(c, POCS_E_ARG, "exchange: at most %d runs per call", POCS_XCHG_MAX_RUNS);
    c->xchg_calls += 1;                                // one exchange sequence: every connected rank makes the same calls in the same order
  }
  if (int r = gmm_upload_run(c)) return r;
  lap("upload enqueued");
  // POCS_OPT_PROFILE: 1 = events around every launch of the hot kernel (eager launches: an event between two kernels
  // keeps the command processor from preparing the next launch under the running one, which adds ~9 us to what it
  // brackets); 2 = the replayed graph as it runs in production between ONE pair of events outside it: span / W is the
  // mean launch PERIOD -- duration plus the gap to the next launch --, an upper bound of the mean duration.
  // (a call on a tree is not bracketed launch by launch: POCS_OPT_PROFILE = 1 runs it eagerly, untimed)
  const bool prof = c->opt_profile == 1 && !c->tree.n, span = c->opt_profile == 2 && c->opt_graph;
  if (int r = prof_begin(c, gmm_hot_launches(c))) return r;
  if (int r = enqueue_ticket_reset(c)) return r;
  if (int r = run_launches(c, c->graph_gmm, span, [&](Issuer is) { return enqueue_gmm_all(is, first, count, prof); })) return r;
  if (int r = enqueue_gmm_results(c)) return r;
  lap("launched");
  prefetch_next_batch(c, gmm_groups(c));          // host chains of the next batch, while the GPU works on this one
  lap("next batch prepared");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  lap("synchronised");
  if (prof) if (int r = prof_collect(c, gmm_hot_launches(c))) return r;
  if (prof || span) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev_seq[0], c->ev_seq[1]));
    c->seq_ms = ms; c->seq_groups = gmm_groups(c);
    if (span) { c->prof_ms = ms; c->prof_launches = (long long)gmm_hot_launches(c); }      // pocs_get_kernel_time: span / W
  }
  if (int r = gmm_check_gave_up(c, "a bounded wait expired on the device (code %u); results discarded")) return r;
  const unsigned* stop = risk_active(c) ? (const unsigned*)((double*)c->h_pin + c->sync.pin) + (c->sync.stop - POCS_SYNC_ABORT) : nullptr;
  if (large_world(c)) if (int r = gmm_read_reach(c)) { reset_results(c); return r; }
  if (int r = gmm_combine(c, (double*)c->h_pin + pin_layout(c).moments, probability, stop)) { reset_results(c); return r; }
  note_obs_counts(c, Kind::Gmm);
  if (int r = read_clearance(c, Kind::Gmm, c->num_gmm)) return r;
  if (int r = read_regions(c, Kind::Gmm, c->num_gmm)) return r;
  if (int r = read_segment(c, Kind::Gmm)) return r;
  c->res.last_gmm_count = count;
  c->res.last_gmm_wp = c->W - 1;
  lap("combined");
  return POCS_OK;
}

// ------------------------------------------------------------------------------------------
// MC path
// ------------------------------------------------------------------------------------------
int mc_shard(pocs_ctx* c, long long* first, long long* count) {
  *first = c->shard_first >= 0 ? c->shard_first : 0;
  *count = c->shard_first >= 0 ? c->shard_count : c->num_particles;
  if (*first < 0 || *count < 0 || *first + *count > c->num_particles)
    return fail(c, POCS_E_ARG, "shard [%lld,+%lld) outside numParticles=%lld", *first, *count, c->num_particles);
  return POCS_OK;
}

// An MC call of plans obeys the risk bound only when asked to (POCS_OPT_MC_RISK_BOUND; by default it ignores the bound); such a
// call, or any MC call under POCS_OPT_MC_WAYPOINT_COUNTS, counts the first collisions per waypoint.  Both off: the launches,
// the memset and the copies of an MC call are what they have always been.
bool mc_stop_active(const pocs_ctx* c) { return c->opt_mc_rb && risk_active(c) && !c->tree.n; }     // (an MC call on a tree ignores the bound)
bool mc_counts_active(const pocs_ctx* c) { return c->opt_mc_wp || c->opt_obs_counts || seg_applied(c) || mc_stop_active(c); }      // (the per-box counts split the per-waypoint ones; an MC call under segment checks counts as under POCS_OPT_MC_WAYPOINT_COUNTS)
// The fused kernel carries a particle through all its steps and meets no other block on the way: a call that stops on a count
// takes the per-step form.
// So does a call that counts clearance levels: the levels live in the per-step kernels (MC_CLEAR).
// And a call under a compound footprint: the parts live in the per-step kernels too (MC_PARTS).
// And a call that counts watched regions: they live in the per-step kernels as well (MC_REGIONS).
// And a call under segment checks: the sub-poses live in the per-step kernels (MC_SEG).
bool mc_fused_form(const pocs_ctx* c) { return c->opt_fused && !mc_stop_active(c) && !clearance_applied(c) && !parts_applied(c) && !regions_applied(c) && !seg_applied(c) && !discs_applied(c) && !rfoot_applied(c); }      // (and under discs and a round footprint: MC_ROUND and MC_RFOOT live in the per-step kernels)
// d_total, u64 words: [R] collided particles per run | counts active: [R][W] first collisions | [R] u32 stop words
size_t mc_total_words(const pocs_ctx* c) {
  const size_t R = (size_t)c->batch, W = (size_t)c->W;
  return mc_counts_active(c) ? R + R * W + (R + 1) / 2 : R;
}

// 28 B of state per particle.  Up to 8 x 10^6 particles (224 MB) the state of a batch stays in the
// 256 MB Infinity Cache between waypoint launches; past that the launches stream from HBM whatever
// they do, and non-temporal accesses then stream faster (16 x 10^6: 148 us instead of 189 us)
#define POCS_MC_CACHE_BYTES 232.0e6

// What every MC launch of a call shares: the per-run inputs, the counters, `count` particles per run, the Cholesky factor of
// the initial covariance, and the non-temporal rule on the `live_particles` whose state the call's launches go back to.
int mc_launch_base(pocs_ctx* c, long long count, double live_particles, pocs_mc_launch* a) {
  memset(a, 0, sizeof *a);
  a->hdr = (const pocs_run_header*)c->d_hdr.p;
  a->env = world_at(c, 0);                           // (k_mc_init: waypoint 0; the launches of later waypoints set their own)
  a->tables = (const pocs_tables*)c->d_tables.p;
  if (large_world(c)) { a->world = (const double*)c->d_world.p; a->world_M = large_boxes(c); }      // (k_mc_init_world, k_mc_step_world)
  a->chain = (const double*)c->d_chain.p;
  a->total = (unsigned long long*)c->d_total.p;
  a->count = count; a->stride = sample_stride_of(count);
  a->nontemporal = c->opt_mc_nt >= 0 ? (int)c->opt_mc_nt : ((live_particles * 28.0 > POCS_MC_CACHE_BYTES) ? 1 : 0);
  if (!pocs_chol3_lower(c->cov0, a->L0)) return fail(c, POCS_E_ARG, "initial covariance is not positive definite");
  return POCS_OK;
}

int enqueue_mc_all(Issuer is, long long first, long long count, bool prof) {
  pocs_ctx* c = is.c;
  const int W = c->W, R = c->batch, nblk = grid_for_mc(count, R);
  pocs_mc_launch a;
  if (int r = mc_launch_base(c, count, (double)R * (double)sample_stride_of(count), &a)) return r;
  a.x = (double*)c->d_px.p; a.y = (double*)c->d_py.p; a.th = (double*)c->d_pt.p;
  a.hits = (uint32_t*)c->d_hits.p;
  a.first = first; a.W = W; a.nruns = R;
  if (mc_counts_active(c)) {
    a.wp_mode = mc_stop_active(c) ? 2 : 1;
    a.wp_counts = a.total + R;
    a.wp_stop = (unsigned*)(a.wp_counts + (size_t)R * (size_t)W);
    a.wp_n = c->num_particles;                       // (a context with plans holds no shard: the run's particles)
    a.wp_bound = c->risk_bound;
  }
  if (c->opt_obs_counts) {
    a.obs_counts = (unsigned long long*)c->d_obsct.p;
    if (int r = enqueue_obs_counts_reset(is)) return r;
  }
  if (parts_applied(c)) { a.parts = (const pocs_parts_dev*)c->d_parts.p; a.parts_F = c->fp_F; }
  if (clearance_applied(c)) {
    a.clr = clear_at(c, 0); a.clr_counts = (unsigned long long*)c->d_clrct.p; a.clr_level = (unsigned char*)c->d_clrlv.p; a.clr_L = c->clr_L;
    if (int r = enqueue_clearance_reset(is)) return r;
  }
  if (regions_applied(c)) {
    a.regions = (const pocs_regions_dev*)c->d_reg.p; a.reg_counts = (unsigned long long*)c->d_regct.p; a.reg_G = c->reg_G;
    if (int r = is.launch(pocs_launch_zero_counts, 0, a.reg_counts, region_count_words(c))) return r;
  }
  if (seg_applied(c)) {
    a.seg = (const pocs_seg_dev*)c->d_seg.p; a.seg_counts = (unsigned long long*)c->d_segct.p;
    if (int r = is.launch(pocs_launch_zero_counts, 0, a.seg_counts, seg_count_words(c))) return r;
  }
  if (discs_applied(c)) a.round = 1;                 // (round obstacles: the MC_ROUND forms of k_mc_init and the per-step kernel)
  if (rfoot_applied(c)) { a.round = 1; a.rfoot = 1; }      // (a round footprint: MC_RFOOT on top, with or without discs)
  if (hyp_applied(c)) a.gates = (const uint32_t*)c->d_gates.p;      // (prediction hypotheses: MC_HYP on top of MC_ROUND, with or without MC_NOISE)
  if (noise_applied(c)) { a.noise = noise_at(c, 0); a.noise_persistent = c->disc_noise_persistent ? 1 : 0; }      // (uncertain discs: MC_NOISE on top)
  if (c->plans.n) {
    a.run_plan = (const double*)c->d_runplan.p;      // every run its own start mean and steps
  } else {
    a.mu0[0] = c->traj[0]; a.mu0[1] = c->traj[W]; a.mu0[2] = c->traj[2 * W];
  }
  // a call of plans: slots in descending plan length (plan_layout, one group), so the runs that still drive a control at
  // step s are a prefix -- the launch of step s covers those only
  const std::vector<int> Ws = slot_lengths(c, plan_layout(c, 1));
  if (mc_fused_form(c)) {
    a.step = W - 1;
    a.env_steps = c->world_S;                        // (> 1: k_mc_fused_sched, which restages the world per step)
    if (prof) if (int r = is.mark(c->events[0])) return r;
    if (int r = is.launch(pocs_launch_mc_fused, 0, nblk, a)) return r;
    if (prof) if (int r = is.mark(c->events[1])) return r;
  } else {
    a.step = 0;
    if (int r = is.launch(pocs_launch_mc_init, 0, nblk, a)) return r;
    for (int s = 0; s < W - 1; ++s) {
      a.step = s;
      pocs_mc_launch as;
      memcpy(&as, &a, sizeof as);
      as.env = world_at(c, s + 1);                   // control s produces waypoint s + 1
      if (as.noise) as.noise = noise_at(c, s + 1);
      if (as.clr) as.clr = clear_at(c, s + 1);
      int nb = nblk;
      if (c->plans.n) {
        as.nruns = live_runs(Ws, 0, R, s + 1);       // plans with a control at step s: W_p - 1 > s
        nb = grid_for_mc(count, as.nruns);
      }
      if (prof) if (int r = is.mark(c->events[2 * s])) return r;
      if (as.nruns > 0) if (int r = is.launch(pocs_launch_mc_step, 0, nb, as)) return r;
      if (prof) if (int r = is.mark(c->events[2 * s + 1])) return r;
    }
  }
  return is.launch(pocs_launch_mc_count, 0, nblk, a);
}

// The first collisions per waypoint as the call's copy brought them back (`words`: mc_total_words, slot order) -> c->res.mc_wp in
// run / plan order.  Every run's counts must add up to its collided particles (k_mc_count's own count of hits > 0).  Under an
// MC stop the rule is restated here on the counts read back: plan p stops at the FIRST waypoint s with
// (double)C[s] / (double)N >= bound, C[s] = F[0] + ... + F[s]; a stop at the last waypoint stops nothing.  The device's stop
// word must say the same and nothing may have been counted behind the stop, or the call fails instead of reporting either.
int mc_read_waypoint_counts(pocs_ctx* c, const unsigned long long* words) {
  const size_t R = (size_t)c->batch, W = (size_t)c->W;
  const unsigned long long* F = words + R;
  const unsigned* stopw = (const unsigned*)(F + R * W);
  const bool plans = c->plans.n > 0, stop = mc_stop_active(c);
  c->res.mc_wp.assign(R * W, 0ull);
  c->res.mc_wp_W = (int)W;
  if (stop) c->res.plan_E_mc = c->plans.W;
  const double n = (double)c->num_particles;
  for (size_t r = 0; r < R; ++r) {                     // (a call of plans: r is the plan, in its slot, over its W_p waypoints)
    const size_t slot = plans ? (size_t)c->res.plan_slot(Kind::Mc)[r] : r, Wr = plans ? (size_t)c->plans.W[r] : W;
    const unsigned long long* f = F + slot * W;
    unsigned long long C = 0;
    int host = 0;                                      // the host's stop word
    for (size_t w = 0; w < W; ++w) {
      C += f[w];
      if (w >= Wr && f[w]) return fail(c, POCS_E_DEVICE, "MC waypoint counts: run %zu has %llu first collisions at waypoint %zu of %zu; results discarded", r, f[w], w, Wr);
      if (stop && !host && w + 1 < Wr && (double)C / n >= c->risk_bound) host = (int)w + 1;
      if (host && (int)w >= host && f[w]) return fail(c, POCS_E_DEVICE, "MC risk bound: plan %zu moved behind its stop at waypoint %d; results discarded", r, host - 1);
    }
    if (C != c->res.mc_counts[r])
      return fail(c, POCS_E_DEVICE, "MC waypoint counts: the first collisions of run %zu add up to %llu, its collided particles are %llu; results discarded", r, C, c->res.mc_counts[r]);
    if (stop) {
      const int dev = (int)stopw[slot];
      if (dev != host)
        return fail(c, POCS_E_DEVICE, "MC risk bound: plan %zu stops at waypoint %d on the device and at %d on the host (-1: not at all); results discarded",
                    r, dev - 1, host - 1);
      if (host) c->res.plan_E_mc[r] = host;
    }
    memcpy(&c->res.mc_wp[r * W], f, W * sizeof(unsigned long long));
  }
  return POCS_OK;
}

// An MC call on a tree of plans.  The root's cloud is drawn by k_mc_init; per level one k_mc_tree_step launch (several for a
// level wider than 256 nodes) moves every node's particles from its parent's place in the previous level's half of the
// particle buffers to its own place in this level's half -- two levels of state are live at a time -- and counts the node's
// first collisions and its collided particles.  The fused form has no counterpart here: a node's cloud is its parent's, so
// POCS_OPT_MC_FUSED = 1 is served by these per-step launches (the same arithmetic, the same bits).  The risk bound is ignored,
// POCS_OPT_MC_RISK_BOUND or not.
size_t tree_max_width(const pocs_ctx* c) {
  size_t w = 1;
  for (size_t d = 0; d + 1 < c->tree.level.size(); ++d) w = std::max(w, (size_t)(c->tree.level[d + 1] - c->tree.level[d]));
  return w;
}
#define POCS_TREE_MC_MAX_BYTES (64ull << 30)      // both halves of the particle state of an MC call on a tree
int enqueue_mc_tree(Issuer is, long long count) {
  pocs_ctx* c = is.c;
  const int T = c->tree.n, D = (int)c->tree.level.size() - 2;
  const size_t half = c->res.tree_mc_half;
  pocs_mc_launch a;
  if (int r = mc_launch_base(c, count, 2.0 * (double)half, &a)) return r;      // (two levels of state are live at a time)
  a.wp_mode = 1;
  a.wp_counts = a.total + T;                         // [T] first collisions, by slot (W = 1: k_mc_init's row of run 0 is the root's)
  a.W = 1;
  a.mu0[0] = c->tree.pose[0]; a.mu0[1] = c->tree.pose[(size_t)T]; a.mu0[2] = c->tree.pose[2 * (size_t)T];
  if (c->opt_obs_counts) {
    a.obs_counts = (unsigned long long*)c->d_obsct.p;      // [T][64], by slot
    if (int r = enqueue_obs_counts_reset(is)) return r;
  }
  auto half_of = [&](pocs_mc_launch* l, int d) {
    const size_t o = (size_t)(d & 1) * half;
    l->x = (double*)c->d_px.p + o; l->y = (double*)c->d_py.p + o; l->th = (double*)c->d_pt.p + o; l->hits = (uint32_t*)c->d_hits.p + o;
  };
  half_of(&a, 0);
  a.nruns = 1;
  if (int r = is.launch(pocs_launch_mc_init, 0, grid_for_mc(count, 1), a)) return r;
  a.tree_parent = (const int*)c->d_tparent.p;
  for (int d = 1; d <= D; ++d) {
    const int lo = c->tree.level[(size_t)d], hi = c->tree.level[(size_t)d + 1];
    a.tree_sx = a.x; a.tree_sy = a.y; a.tree_sth = a.th; a.tree_shits = a.hits;      // (the previous level's half)
    half_of(&a, d);
    a.env = world_at(c, d);
    a.tree_dst_lo = lo; a.tree_src_lo = c->tree.level[(size_t)d - 1];
    for (int s = lo; s < hi; s += 256) {
      a.tree_lo = s;
      a.nruns = hi - s < 256 ? hi - s : 256;
      if (int r = is.launch(pocs_launch_mc_tree_step, 0, grid_for_mc(count, a.nruns), a)) return r;
    }
  }
  return POCS_OK;
}

// What both MC paths share behind run_mc_local's checks: the common buffers and the runs' upload (mc_prepare), and the call's
// tail (mc_run): counters zeroed, launches run, counters copied to the pin's `total` words (-> *tot), stream synchronised.  (The
// reset and the copy are plain stream operations: the captured graph holds kernel nodes only, like the GMM path's.)
int mc_prepare(pocs_ctx* c, size_t runs, size_t chain_rows, size_t elems, size_t total_bytes) {
  if (int r = ensure(c, c->d_hdr, runs * sizeof(pocs_run_header))) return r;
  if (int r = ensure(c, c->d_chain, chain_rows * POCS_CHAIN_STRIDE * sizeof(double))) return r;
  for (DevBuf* b : {&c->d_px, &c->d_py, &c->d_pt}) if (int r = ensure(c, *b, elems * sizeof(double))) return r;
  if (int r = ensure(c, c->d_hits, elems * sizeof(uint32_t))) return r;
  if (int r = ensure(c, c->d_total, total_bytes + 16)) return r;
  if (int r = ensure_obs_counts(c)) return r;
  if (int r = ensure_clearance(c)) return r;
  if (clearance_applied(c)) if (int r = ensure(c, c->d_clrlv, elems)) return r;
  if (int r = ensure_regions(c)) return r;
  if (int r = ensure_segment(c)) return r;
  if (int r = ensure_pin(c)) return r;
  return stage_and_upload_runs(c, 1, Kind::Mc);
}
template <class Enqueue>
int mc_run(pocs_ctx* c, size_t total_bytes, bool span, const unsigned long long** tot, Enqueue enqueue) {
  HIPCHK(c, hipMemsetAsync(c->d_total.p, 0, total_bytes, c->stream));
  if (int r = run_launches(c, c->graph_mc, span, enqueue)) return r;
  *tot = (const unsigned long long*)((double*)c->h_pin + pin_layout(c).total);
  HIPCHK(c, hipMemcpyAsync((void*)*tot, c->d_total.p, total_bytes, hipMemcpyDeviceToHost, c->stream));
  prefetch_next_batch(c, 1);       // host chains of the next batch, while the GPU works on this one
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return POCS_OK;
}

int run_mc_tree(pocs_ctx* c) {                      // (behind run_mc_local's checks)
  if (int r = upload_tree(c)) return r;
  const long long count = c->num_particles;
  const size_t T = (size_t)c->tree.n, stride = (size_t)sample_stride_of(count), half = tree_max_width(c) * stride;
  if ((double)half * 2.0 * 28.0 > (double)POCS_TREE_MC_MAX_BYTES)
    return fail(c, POCS_E_ARG, "MC on a tree: its widest level has %zu nodes; two levels of %lld particles each need %.1f GB of particle state, more than the %llu GB an MC call on a tree may hold",
                tree_max_width(c), count, (double)half * 2.0 * 28.0 / 1e9, (unsigned long long)(POCS_TREE_MC_MAX_BYTES >> 30));
  c->res.tree_mc_half = half;
  const size_t total_bytes = 2 * T * sizeof(unsigned long long);       // [T] collided at or before the node | [T] first collisions at it
  if (int r = mc_prepare(c, T, T, 2 * half, total_bytes)) return r;
  const unsigned long long* tot;
  if (int r = mc_run(c, total_bytes, false, &tot, [&](Issuer is) { return enqueue_mc_tree(is, count); })) return r;
  c->prof_ms = 0.0; c->prof_launches = 0;
  const unsigned long long* F = tot + T;
  c->res.tree_F.assign(T, 0ull); c->res.tree_C.assign(T, 0ull);
  c->res.tree_probs.assign(T, 0.0); c->res.tree_eval.assign(T, 1);
  c->res.mc_wp.clear(); c->res.plan_E_mc.clear();
  for (size_t n = 0; n < T; ++n) {
    const size_t slot = (size_t)c->tree.slot[n];
    const int p = c->tree.parent[n];
    c->res.tree_F[n] = F[slot];
    c->res.tree_C[n] = (p >= 0 ? c->res.tree_C[(size_t)p] : 0ull) + F[slot];
    // (the kernel's own count of the node's collided particles must be its path's first collisions added up)
    if (p >= 0 && tot[slot] != c->res.tree_C[n]) {
      const int r = fail(c, POCS_E_DEVICE, "MC on a tree: node %zu has %llu collided particles, the first collisions along its path add up to %llu; results discarded",
                         n, tot[slot], c->res.tree_C[n]);
      reset_results(c);
      return r;
    }
    c->res.tree_probs[n] = (double)c->res.tree_C[n] / (double)count;
  }
  c->res.mc_counts.assign(1, c->res.tree_C[0]);
  c->res.last_mc_count = count;
  c->res.last_kind = Kind::Mc;
  c->res.tree_sel = 0;
  note_obs_counts(c, Kind::Mc);
  return POCS_OK;
}

// One batch of MC roll-outs (runSimulation x batch) over this context's shard; fills c->res.mc_counts.
int run_mc_local(pocs_ctx* c) {
  c->res.oc_kind = Kind::None;
  open_clearance(c);
  open_regions(c);
  open_segment(c);
  if (int r = check_common(c)) return r;
  if (c->num_particles < 1) return fail(c, POCS_E_STATE, "setNumParticles missing");
  if (int r = upload_static(c)) return r;
  if (c->tree.n) return run_mc_tree(c);
  long long first, count;
  if (int r = mc_shard(c, &first, &count)) return r;
  const size_t W = (size_t)c->W, R = (size_t)c->batch;
  const size_t total_bytes = mc_total_words(c) * sizeof(unsigned long long);
  if (c->plans.n)
    if (int r = ensure(c, c->d_runplan, R * 4 * sizeof(double))) return r;
  if (int r = mc_prepare(c, R, R * (W > 1 ? W - 1 : 1), R * (size_t)sample_stride_of(count), total_bytes)) return r;
  const bool prof = c->opt_profile == 1, span = c->opt_profile == 2 && c->opt_graph;      // (as run_gmm_full)
  const size_t nprof = mc_fused_form(c) ? 1 : (W > 1 ? W - 1 : 0);
  if (int r = prof_begin(c, nprof > 0 ? nprof : 1)) return r;
  const unsigned long long* tot;
  if (int r = mc_run(c, total_bytes, span, &tot, [&](Issuer is) { return enqueue_mc_all(is, first, count, prof); })) return r;
  if (int r = prof_collect(c, nprof)) return r;
  if (span) {                                          // the graph's span over its W - 1 hot launches (+ the init and count launches: an upper bound)
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev_seq[0], c->ev_seq[1]));
    c->prof_ms = ms; c->prof_launches = (long long)(nprof > 0 ? nprof : 1);
  }
  c->res.mc_counts.resize(R);
  memcpy(c->res.mc_counts.data(), tot, R * sizeof(unsigned long long));
  if (c->plans.n) {                                     // slot order -> the caller's plan order
    const std::vector<unsigned long long> by_slot = c->res.mc_counts;
    for (size_t p = 0; p < R; ++p) c->res.mc_counts[p] = by_slot[(size_t)c->res.plan_slot(Kind::Mc)[p]];
  }
  c->res.last_mc_count = count;
  c->res.last_kind = Kind::Mc;
  c->res.mc_wp.clear(); c->res.plan_E_mc.clear();
  if (mc_counts_active(c))
    if (int r = mc_read_waypoint_counts(c, tot)) { reset_results(c); return r; }
  note_obs_counts(c, Kind::Mc);
  if (int r = read_clearance(c, Kind::Mc, count)) return r;
  if (int r = read_regions(c, Kind::Mc, count)) return r;
  return read_segment(c, Kind::Mc);
}

}  // namespace pocs_rt

using namespace pocs_rt;

extern "C" {

// The step API's sampling launch of waypoint w, eager -- `exchange`: with the moments' exchange and the advance in its tail.
static int step_api_sample(pocs_ctx* c, int w, bool exchange) {
  long long first, count;
  if (int r = gmm_shard(c, &first, &count)) return r;
  pocs_gmm_launch base;
  fill_gmm_launch(c, &base, first, count);
  StepLaunch s;
  s.prof_slot = c->opt_profile == 1 ? w : -1;
  if (exchange) { s.advance = true; s.exchange = StepLaunch::FROM_CONTEXT; }
  if (int r = enqueue_step({c, nullptr}, base, w, s)) return r;
  c->res.last_gmm_wp = w;
  c->res.last_gmm_count = count;
  if (exchange && w + 1 < c->W) c->last_gmm_adv = w + 1;
  return POCS_OK;
}

int pocs_gmm_begin(pocs_ctx* c) {
  if (!c) return POCS_E_ARG;
  if (int r = may_enter(c, "pocs_gmm_begin", pocs_modes::kSequence)) return r;
  HIPCHK(c, hipSetDevice(c->device));
  ra_drop(c);
  c->ra_internal = false;
  if (int r = gmm_prepare(c)) return r;
  if (int r = gmm_upload_run(c)) return r;
  if (int r = prof_begin(c, (size_t)c->W)) return r;
  if (int r = enqueue_ticket_reset(c)) return r;
  if (int r = enqueue_obs_counts_reset({c, nullptr})) return r;
  c->res.oc_kind = Kind::None;                                 // (the table is this sequence's from here on; served once pocs_gmm_end has closed it)
  open_clearance(c);                                           // (the step API: the levels are not applied)
  open_regions(c);                                             // (nor the watched regions)
  open_segment(c);                                             // (segment checks refuse the sequence: J is 1 here)
  c->xchg_calls += 1;
  c->gmm_open = true;
  c->res.last_gmm_wp = -1;
  c->last_gmm_adv = -1;
  return POCS_OK;
}

int pocs_gmm_advance_local(pocs_ctx* c, int w) {
  if (!c) return POCS_E_ARG;
  if (!c->gmm_open) return fail(c, POCS_E_ORDER, "pocs_gmm_advance_local before pocs_gmm_begin");
  if (w != c->res.last_gmm_wp + 1 || w != c->last_gmm_adv + 1 || w >= c->W)
    return fail(c, POCS_E_ORDER, "advance of waypoint %d out of sequence", w);
  if (int r = enqueue_advance({c, nullptr}, w)) return r;    // folds the (reduced) moments of w-1
  c->last_gmm_adv = w;
  return POCS_OK;
}

int pocs_gmm_sample_local(pocs_ctx* c, int w) {
  if (!c) return POCS_E_ARG;
  if (!c->gmm_open) return fail(c, POCS_E_ORDER, "pocs_gmm_sample_local before pocs_gmm_begin");
  if (w != c->res.last_gmm_wp + 1 || w >= c->W) return fail(c, POCS_E_ORDER, "waypoint %d out of sequence", w);
  if (w != c->last_gmm_adv) return fail(c, POCS_E_ORDER, "waypoint %d sampled before pocs_gmm_advance_local(%d)", w, w);
  return step_api_sample(c, w, false);
}

int pocs_gmm_step_local(pocs_ctx* c, int w) {
  if (int r = pocs_gmm_advance_local(c, w)) return r;
  return pocs_gmm_sample_local(c, w);
}

void* pocs_gmm_moments_ptr(pocs_ctx* c, int w) {
  if (!c || w < 0 || w >= c->W || c->K < 1) return nullptr;
  double* m = moments_dev(c);
  return m ? m + (size_t)w * c->batch * c->K * POCS_NMOM : nullptr;
}

int pocs_gmm_moments_len(const pocs_ctx* c) { return (c && c->K > 0) ? c->batch * c->K * POCS_NMOM : 0; }

int pocs_gmm_exchange_local(pocs_ctx* c, int w) {
  if (!c) return POCS_E_ARG;
  if (!c->gmm_open) return fail(c, POCS_E_ORDER, "pocs_gmm_exchange_local before pocs_gmm_begin");
  if (!c->xchg_connected) return fail(c, POCS_E_ORDER, "pocs_gmm_exchange_local before pocs_xchg_connect");
  if (w != c->res.last_gmm_wp || w != c->last_gmm_adv) return fail(c, POCS_E_ORDER, "exchange of waypoint %d out of sequence", w);
  if (c->batch > POCS_XCHG_MAX_RUNS) return fail(c, POCS_E_ARG, "exchange: at most %d runs per call", POCS_XCHG_MAX_RUNS);
  pocs_gmm_launch a;
  fill_gmm_launch(c, &a, 0, 0);
  aim_gmm_launch(c, &a, w);
  pocs_xchg_dev x;
  fill_xchg(c, &x, w, false);
  if (int r = Issuer{c, nullptr}.launch(pocs_launch_gmm_exchange, 0, c->K, a, x)) return r;
  if (w + 1 < c->W) c->last_gmm_adv = w + 1;          // the exchange launch has built the mixture of w + 1
  return POCS_OK;
}

// sample(w) + exchange(w) in ONE launch: the block that closes a run's waypoint exchanges its moments
// (k_gmm_step, exchange_in_tail) and advances the mixture -- what pocs_gmm_sample_local followed by
// pocs_gmm_exchange_local does with two launches, bit for bit.
int pocs_gmm_sample_exchange_local(pocs_ctx* c, int w) {
  if (!c) return POCS_E_ARG;
  if (!c->gmm_open) return fail(c, POCS_E_ORDER, "pocs_gmm_sample_exchange_local before pocs_gmm_begin");
  if (!c->xchg_connected) return fail(c, POCS_E_ORDER, "pocs_gmm_sample_exchange_local before pocs_xchg_connect");
  if (w != c->res.last_gmm_wp + 1 || w >= c->W) return fail(c, POCS_E_ORDER, "waypoint %d out of sequence", w);
  if (w != c->last_gmm_adv) return fail(c, POCS_E_ORDER, "waypoint %d sampled before its mixture exists", w);
  if (c->batch > POCS_XCHG_MAX_RUNS) return fail(c, POCS_E_ARG, "exchange: at most %d runs per call", POCS_XCHG_MAX_RUNS);
  return step_api_sample(c, w, true);
}

int pocs_gmm_end(pocs_ctx* c, double* probability) {
  if (!c) return POCS_E_ARG;
  if (!c->gmm_open) return fail(c, POCS_E_ORDER, "pocs_gmm_end before pocs_gmm_begin");
  if (c->res.last_gmm_wp != c->W - 1) return fail(c, POCS_E_ORDER, "pocs_gmm_end after %d of %d waypoints", c->res.last_gmm_wp + 1, c->W);
  if (!probability) return fail(c, POCS_E_ARG, "null output");
  if (int r = enqueue_gmm_results(c)) return r;   // (no plans, no tree here: the moments and the give-up word alone)
  prefetch_next_batch(c, gmm_groups(c));          // host chains of the next batch, while the queued work drains
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (int r = gmm_check_gave_up(c, "a bounded wait expired on the device (code %u: 4 = a peer's moments never arrived); results discarded")) { c->gmm_open = false; return r; }
  if (int r = prof_collect(c, (size_t)c->W)) return r;
  (void)gmm_combine(c, (double*)c->h_pin + pin_layout(c).moments, probability);      // (no risk bound in the step API: cannot fail)
  note_obs_counts(c, Kind::Gmm);
  c->gmm_open = false;
  return POCS_OK;
}

}  // extern "C"

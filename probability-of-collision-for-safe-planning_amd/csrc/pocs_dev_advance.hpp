// pocs_dev_advance.hpp -- the mixture advance and the exchange of moments between ranks, a part of pocs_kernels.hip (the
// only unit with device code; included there, inside its anonymous namespace).  Relies on pocs_dev_prims.hpp and on
// pocs_model.h (the arithmetic of one component).
//
//   k_gmm_advance       T1 tail  the mixture advance as its own launch (waypoint 0; after the caller's all-reduce when the
//                                shards exchange their moments that way)
//   k_gmm_tree_advance  T1 tail  the same for the nodes of one level of a tree of plans, from the PARENT's rows
//   k_gmm_exchange      T1 tail  exchange + advance as their own launch (the step API's two-launch form)
//   advance_block, gmm_exchange_rows: the same two steps as k_gmm_step's closers run them (pocs_dev_gmm.hpp)

// LDS scratch of the mixture advance (doubles): state[w-1], moments, chain record, sensor, state[w], param[w];
// and of the speculated component counts.
#define POCS_ADV_SCRATCH(K) ((K) * (2 * POCS_STATE_STRIDE + POCS_NMOM + POCS_PARAM_STRIDE) + POCS_CHAIN_STRIDE + \
                             (int)(sizeof(pocs_sensor) / sizeof(double)))
#define POCS_SPEC_SCRATCH(K) ((K) * (POCS_STATE_STRIDE + 2))

// Mixture bookkeeping of waypoint `w` (pocs_gmm_advance_component / pocs_gmm_normalise): every input
// (state[w-1], the reduced moments of w-1, the chain record of step w-1, the sensor) is first brought
// to LDS in ONE round trip, lanes < K of one wave then take one component each (truncated mean /
// covariance, EKF predict + update, Cholesky); lane 0 normalises, draws the component counts, and the
// wave writes state[w] / param[w] back write-through.  Run by a whole block (k_gmm_advance,
// k_gmm_step: a lane of a second wave draws the counts meanwhile, on the premise -- checked -- that
// no factorisation fails).
struct adv_ptrs {
  double *l_prev, *l_mom, *l_ch, *l_sen, *l_next, *l_par;
  double *g_state, *g_param;
  const double *g_prev, *g_mom, *g_ch, *g_sen;
  int ss, ps, NC;
};
// TREE (a tree of plans, pocs_set_plan_tree): the rows are one per NODE -- state / param / moments [slot], chain [slot] = the
// record of the edge into the node -- and the predecessor of slot r is its PARENT's row, not "the same run, one waypoint
// earlier"; w is the node's depth: it keys the random draws and tells the root (w = 0) from the rest, and addresses nothing.
template <bool TREE = false>
__device__ __forceinline__ adv_ptrs advance_ptrs(const pocs_gmm_launch& a, int K, int w, int r, double* scratch) {
  adv_ptrs p;
  constexpr int SEN = (int)(sizeof(pocs_sensor) / sizeof(double));
  p.ss = K * POCS_STATE_STRIDE; p.ps = K * POCS_PARAM_STRIDE; p.NC = K * POCS_NMOM;
  p.l_prev = scratch;
  p.l_mom = p.l_prev + p.ss;
  p.l_ch = p.l_mom + p.NC;
  p.l_sen = p.l_ch + POCS_CHAIN_STRIDE;
  p.l_next = p.l_sen + SEN;
  p.l_par = p.l_next + p.ss;
  if (TREE) {
    const int pr = w > 0 ? a.tree_parent[r] : r;     // (the root's initial mixture lies in its own row, as a run's in state[r][0])
    p.g_state = a.state + (size_t)r * p.ss;
    p.g_param = a.param + (size_t)r * p.ps;
    p.g_prev = a.state + (size_t)pr * p.ss;
    p.g_mom = a.moments + (size_t)pr * p.NC;
    p.g_ch = a.chain + (size_t)r * POCS_CHAIN_STRIDE;
    p.g_sen = reinterpret_cast<const double*>(a.sensor);
    return p;
  }
  // run r of the batch: state/param [r][W][..], moments [W][R][..] (one all-reduce per waypoint
  // covers every run), chain [r][W-1][..]
  p.g_state = a.state + (size_t)r * a.W * p.ss;
  p.g_param = a.param + (size_t)r * a.W * p.ps;
  p.g_prev = p.g_state + (size_t)(w > 0 ? w - 1 : 0) * p.ss;
  p.g_mom = a.moments + ((size_t)(w > 0 ? w - 1 : 0) * a.nruns + r) * p.NC;
  p.g_ch = a.chain + ((size_t)r * (a.W > 1 ? a.W - 1 : 1) + (w > 0 ? w - 1 : 0)) * POCS_CHAIN_STRIDE;
  p.g_sen = reinterpret_cast<const double*>(a.sensor);
  return p;
}

// `nthreads` threads (tid < nthreads).  mom_in_lds: l_mom already holds the moments of w-1 (the caller
// has just reduced them); otherwise they are read from a.moments (own launch: after the caller's
// all-reduce).  state[w-1] may have been written by another block of THIS launch: L1-bypassing loads.
// One batch of loads for everything (the scratch is laid out l_prev | l_mom | l_ch | l_sen).
// (request / commit: the batch of four loads per thread that starts at index i0, and their stores -- a caller with other
// requests to make puts them between the two, so that all of them share one round trip)
__device__ __forceinline__ int advance_stage_count(const adv_ptrs& p, const bool load_mom) {
  constexpr int SEN = (int)(sizeof(pocs_sensor) / sizeof(double));
  return p.ss + POCS_CHAIN_STRIDE + SEN + (load_mom ? p.NC : 0);
}
//   ONE_LOAD: one load per element, its address chosen by the element's range, L1-bypassing for all four sources (state[w-1]
//   needs it, the others do not mind) -- for the closer, where around four different loads in an if / else-if chain the compiler
//   put a wait behind each branch (three dependent round trips); the lone form's heads keep the chain (no waits there, and the
//   chain record and the sensor come through the caches: measured 0.17 us per waypoint)
template <bool ONE_LOAD = false>
__device__ __forceinline__ void advance_request(const adv_ptrs& p, const bool load_mom, const int i0, const int nthreads, double (&v)[4],
                                                const bool wanted = true) {
  constexpr int SEN = (int)(sizeof(pocs_sensor) / sizeof(double));
  const int ss = p.ss, n = wanted ? advance_stage_count(p, load_mom) : 0;     // (not wanted: no lane loads anything -- and no branch round the loads)
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = i0 + u * nthreads;
    if (ONE_LOAD) {
      const double* src = i < ss ? &p.g_prev[i]
                        : i < ss + POCS_CHAIN_STRIDE ? &p.g_ch[i - ss]
                        : i < ss + POCS_CHAIN_STRIDE + SEN ? &p.g_sen[i - ss - POCS_CHAIN_STRIDE]
                        : &p.g_mom[i - ss - POCS_CHAIN_STRIDE - SEN];
      v[u] = i < n ? load_wt(src) : 0.0;
    } else {
      v[u] = 0.0;
      if (i < ss) v[u] = load_wt(&p.g_prev[i]);
      else if (i < ss + POCS_CHAIN_STRIDE) v[u] = p.g_ch[i - ss];
      else if (i < ss + POCS_CHAIN_STRIDE + SEN) v[u] = p.g_sen[i - ss - POCS_CHAIN_STRIDE];
      else if (i < n) v[u] = p.g_mom[i - ss - POCS_CHAIN_STRIDE - SEN];
    }
  }
}
__device__ __forceinline__ void advance_commit(const adv_ptrs& p, const bool load_mom, const int i0, const int nthreads, const double (&v)[4]) {
  constexpr int SEN = (int)(sizeof(pocs_sensor) / sizeof(double));
  const int ss = p.ss, n = advance_stage_count(p, load_mom);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = i0 + u * nthreads;
    if (i < ss) p.l_prev[i] = v[u];
    else if (i < ss + POCS_CHAIN_STRIDE + SEN) p.l_ch[i - ss] = v[u];              // l_ch | l_sen are contiguous
    else if (i < n) p.l_mom[i - ss - POCS_CHAIN_STRIDE - SEN] = v[u];
  }
}
template <bool TREE = false>
__device__ __forceinline__ void advance_stage(const pocs_gmm_launch& a, int K, int w, int r, double* scratch,
                                              bool mom_in_lds, int tid, int nthreads) {
  const adv_ptrs p = advance_ptrs<TREE>(a, K, w, r, scratch);
  const bool load_mom = w > 0 && !mom_in_lds;
  // index space: [0, ss) state | [ss, ss + CH + SEN) chain record, sensor | then (only if wanted) the moments;
  // l_mom is NOT touched when the caller has put the moments there
  const int n = advance_stage_count(p, load_mom);
  for (int i0 = tid; i0 < n; i0 += nthreads * 4) {
    double v[4];
    advance_request(p, load_mom, i0, nthreads, v);
    requests_issued();
    advance_commit(p, load_mom, i0, nthreads, v);
  }
}
// the largest index space of advance_stage: a block of TB threads with 4 TB >= this stages it in ONE batch
#define POCS_ADV_STAGE_MAX (POCS_MAX_GAUSSIANS * (POCS_STATE_STRIDE + POCS_NMOM) + POCS_CHAIN_STRIDE + (int)(sizeof(pocs_sensor) / sizeof(double)))

// one wave, after advance_stage (+ barrier): one component per lane
template <bool TREE = false>
__device__ __forceinline__ void advance_components(const pocs_gmm_launch& a, int K, int w, int r, int lane, double* scratch) {
  const adv_ptrs p = advance_ptrs<TREE>(a, K, w, r, scratch);
  if (lane < K)
    pocs_gmm_advance_component(lane, p.l_prev, (w == 0) ? nullptr : p.l_mom, p.l_ch, p.l_ch + 3, p.l_ch + POCS_CHAIN_Z,
                               reinterpret_cast<const pocs_sensor*>(p.l_sen), p.l_next, p.l_par);
}

// one lane of ANOTHER wave, meanwhile: the component counts of waypoint w on the premise -- checked by
// advance_finish -- that no Cholesky factorisation fails.  spec = K cumulative counts, K alive flags assumed.
template <bool TREE = false>
__device__ __forceinline__ void speculate_counts(const pocs_gmm_launch& a, int K, int w, int r, double* scratch, double* spec) {
  const adv_ptrs p = advance_ptrs<TREE>(a, K, w, r, scratch);
  double* st = spec + 2 * K;                                   // a K x STATE_STRIDE image: only [12], [13] matter
  for (int k = 0; k < K; ++k) {
    const double alive_prev = p.l_prev[k * POCS_STATE_STRIDE + 13];
    const double n = p.l_mom[k * POCS_NMOM];
    const bool alive = alive_prev != 0.0 && n >= 2.0;          // pocs_gmm_advance_component / pocs_truncated_moments
    st[k * POCS_STATE_STRIDE + 12] = alive ? n : 0.0;
    st[k * POCS_STATE_STRIDE + 13] = alive ? alive_prev : 0.0;
    spec[K + k] = st[k * POCS_STATE_STRIDE + 13];
  }
  const int last_alive = pocs_normalise_weights(K, 1, st);
  pocs_component_counts(K, st, last_alive, a.hdr[r].seed, (uint32_t)w, (double)a.n_total, spec, 1);
}

// the wave of advance_components, after it (+ barrier): weights, component counts (the speculated ones
// if there are any and their premise held), write-through stores of state[w] / param[w].
template <bool TREE = false>
__device__ __forceinline__ void advance_finish(const pocs_gmm_launch& a, int K, int w, int r, int lane, double* scratch,
                                               const double* spec, const bool publish = true) {
  const adv_ptrs p = advance_ptrs<TREE>(a, K, w, r, scratch);
  if (lane == 0) {
    bool use_spec = spec != nullptr;
    if (use_spec) for (int k = 0; k < K; ++k) use_spec = use_spec && (p.l_next[k * POCS_STATE_STRIDE + 13] == spec[K + k]);
    if (use_spec) {
      (void)pocs_normalise_weights(K, 1, p.l_next);
      for (int k = 0; k < K; ++k) p.l_par[k * POCS_PARAM_STRIDE + 9] = spec[k];
    } else {
      pocs_gmm_normalise(K, w > 0, p.l_next, p.l_par, a.hdr[r].seed, (uint32_t)w, (double)a.n_total);
    }
  }
  __threadfence_block();
  __builtin_amdgcn_wave_barrier();
  if (!publish) return;                              // (lone call: one block of the launch writes the records out)
  const size_t row = TREE ? 0 : (size_t)w;           // (a tree: g_state / g_param are the node's own row)
  for (int j = lane; j < p.ss; j += 64) store_wt(&p.g_state[row * p.ss + j], p.l_next[j]);
  for (int j = lane; j < p.ps; j += 64) store_wt(&p.g_param[row * p.ps + j], p.l_par[j]);
  // (not drained: nothing inside this launch reads the records -- state[w] / param[w] are for the NEXT waypoint's launch, behind
  // the kernel boundary; waiting for the write-through stores here kept every closer 1.2 us longer in the launch's tail)
}

// The whole advance to waypoint w by a block of >= 128 threads (every thread calls it).
// staged: the caller has issued advance_stage already (and a barrier since); publish: state[w] / param[w] go out
// to global memory as well (always, except for all but one block of a lone call's launch).
struct advance_no_side_job { __device__ __forceinline__ void operator()() const {} };
// `side_job`: run by the threads tid >= 128 -- the waves that otherwise wait at the barrier below for the components'
// serial chain (wave 0) and the count lane (wave 1) -- with nothing of the advance's scratch in it (the lone form's
// heads draw the first iterations' normals there, k_gmm_step)
// `post_job`: run by wave 1 (64 <= tid < 128; its lane 0 has drawn the counts by then) beside advance_finish, with nothing in it
// that the normalisation still changes -- means and Cholesky factors of param[w] are final once the components are through
// (the lone form's heads cull the obstacle table there)
template <bool TREE = false, typename SideJob = advance_no_side_job, typename PostJob = advance_no_side_job>
__device__ __forceinline__ void advance_block(const pocs_gmm_launch& a, int K, int w, int r, double* adv, double* spec,
                                              bool mom_in_lds, int tid, int nthreads, const bool staged = false,
                                              const bool publish = true, SideJob side_job = SideJob(), PostJob post_job = PostJob()) {
  POCS_ADV_STAMP_BEGIN();
  if (!staged) {
    advance_stage<TREE>(a, K, w, r, adv, mom_in_lds, tid, nthreads);
    __syncthreads();
  }
  POCS_ADV_STAMP(8);
  if (tid < 64) advance_components<TREE>(a, K, w, r, tid, adv);
  else if (tid == 64 && w > 0) speculate_counts<TREE>(a, K, w, r, adv, spec);
  else if (tid >= 128) side_job();
  POCS_ADV_STAMP(9);
  __syncthreads();
  POCS_ADV_STAMP(10);
  if (tid < 64) advance_finish<TREE>(a, K, w, r, tid, adv, w > 0 ? spec : nullptr, publish);
  else if (tid < 128) post_job();
  POCS_ADV_STAMP(11);
}
__global__ __launch_bounds__(128) void k_gmm_advance(pocs_gmm_launch a, int K) {
  __shared__ double s_adv[POCS_ADV_SCRATCH(POCS_MAX_GAUSSIANS)];
  __shared__ double s_spec[POCS_SPEC_SCRATCH(POCS_MAX_GAUSSIANS)];
  advance_block(a, K, a.waypoint, blockIdx.x, s_adv, s_spec, false, threadIdx.x, 128);      // one block per run
}
// A tree of plans, level d = a.waypoint: one block per node of the level (slots run_lo .. run_lo + run_cnt), the mixture of
// the node from its PARENT's state and reduced moments and its own chain record -- the arithmetic of k_gmm_advance in the same
// order.  RISK (pocs_set_plan_risk_bound): a node whose parent has stopped -- at the bound itself, or below a node that has --
// inherits the stop (its word gets the inherited mark, no mixture is built, and the heads of the level's sampling launch
// return on it as they do on a plan's stop); a live parent hands its running survival product down, so that the node's
// closer starts from it exactly as a plan's closer of waypoint d starts from waypoint d - 1's.  stop / surv of the parent
// were written by the launches of level d - 1, behind a kernel boundary on the same stream.
template <bool RISK>
__global__ __launch_bounds__(128) void k_gmm_tree_advance(pocs_gmm_launch a, int K) {
  __shared__ double s_adv[POCS_ADV_SCRATCH(POCS_MAX_GAUSSIANS)];
  __shared__ double s_spec[POCS_SPEC_SCRATCH(POCS_MAX_GAUSSIANS)];
  const int r = a.run_lo + (int)blockIdx.x, w = a.waypoint;
  if (RISK && w > 0) {
    const int pr = a.tree_parent[r];
    const unsigned sp = __hip_atomic_load(&a.stop[pr], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__builtin_amdgcn_readfirstlane((int)sp) != 0) {
      if (threadIdx.x == 0) __hip_atomic_store(&a.stop[r], sp | POCS_TREE_STOP_INHERITED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
    if (threadIdx.x == 0) store_wt(&a.surv[r], load_wt(&a.surv[pr]));
  }
  advance_block<true>(a, K, w, r, s_adv, s_spec, false, threadIdx.x, 128);
}

// ---------------------------------------------------------------------------------------------
// Sharded over the GPUs of a node: the moments of waypoint w of this rank's samples (moments[w][r],
// left by k_gmm_step) -> the moments of the whole mixture, in ONE hop over xGMI instead of a ring
// (11 K doubles per run are latency, not bandwidth), and straight on to the mixture
// of waypoint w+1 -- exchange + advance in one small launch (one block per run) between two sampling
// launches.  Every rank owns a buffer that all ranks have mapped; rank q writes its row into slot q
// of EVERY buffer (system-scope stores: peers sit across xGMI), drains, meets, writes the slot's flag
// = this waypoint's epoch; then waits for the world's flags in its OWN buffer and adds the slots in
// rank order -- every rank the same sum, bit for bit, whatever the arrival order.  Slots alternate
// with the parity of a running count of exchanges that is the same on every rank (calls x W + waypoint,
// pocs_xchg_dev::parity -- NOT the waypoint's own parity: with an odd W the last exchange of a call and
// the first of the next would share a slot): a rank can only be one exchange ahead of another.  The wait is bounded
// (30 s, once per call: later exchanges of a call that has given up return at once): on expiry the
// call's give-up word is set and the host reports POCS_E_DEVICE.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double* xchg_row(double* buf, int parity, int src, int r) {
  return buf + (((size_t)parity * POCS_XCHG_MAX_WORLD + src) * POCS_XCHG_MAX_RUNS + r) * POCS_XCHG_MAX_NC;
}
__device__ __forceinline__ unsigned long long* xchg_flag(double* buf, int parity, int src, int r) {
  return reinterpret_cast<unsigned long long*>(buf + POCS_XCHG_DATA_DOUBLES) +
         ((size_t)parity * POCS_XCHG_MAX_WORLD + src) * POCS_XCHG_MAX_RUNS + r;
}
// The exchange itself, by the `nthreads` threads of one block for run r at waypoint w: `mine` (NC doubles,
// global or LDS) -> slot `rank` of every rank's buffer; wait for the world's rows; the sum in rank order
// -> a.moments[w][r] and l_mom (LDS; may be `mine`).  s_ok: one int of LDS.  false = gave up.
__device__ __forceinline__ bool gmm_exchange_rows(const pocs_gmm_launch& a, const pocs_xchg_dev& x, const unsigned long long epoch, const int parity,
                                                  const int K, const int w, const int r,
                                                  const double* mine, double* l_mom, const int tid, const int nthreads, int* s_ok) {
  const int NC = K * POCS_NMOM;
  for (int i = tid; i < NC * x.world; i += nthreads) {
    const int q = i / NC, c = i - q * NC;
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(xchg_row(x.buf[q], parity, x.rank, r) + c),
                       (unsigned long long)__double_as_longlong(mine[c]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  // the rows are out before the flags: they were stored write-through at system scope, and every storing
  // wave waits for its stores here.  (NOT a system-scope release fence: that writes back the whole L2, and
  // in the tail of a sampling launch the L2 is full of samples on their way out -- measured +45 us per
  // 64-run launch.)
  drain_stores();
  __syncthreads();
  if (tid < x.world)
    __hip_atomic_store(xchg_flag(x.buf[tid], parity, x.rank, r), epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  // every rank's row of this waypoint has landed in MY buffer?
  if (tid == 0) *s_ok = 1;
  __syncthreads();
  if (tid < x.world) {
    const unsigned long long* f = xchg_flag(x.buf[x.rank], parity, tid, r);
    const unsigned long long t0 = wall_clock64();
    unsigned polls = 0;
    while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != epoch) {
      __builtin_amdgcn_s_sleep(8);
      if ((++polls & 255u) == 0u && wall_clock64() - t0 > 3000000000ull) {      // 30 s: ranks of a cold node start seconds apart
        __hip_atomic_store(&a.sync[POCS_SYNC_ABORT], 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *s_ok = 0;
        break;
      }
    }
    // how long this closer waited for rank `tid`'s row (10 ns ticks; its own row: no time): the longest of them is
    // what the exchange cost this (run, waypoint) -- pocs_get_exchange_wait, for a scaling run that explains itself
    const unsigned long long dt = wall_clock64() - t0;
    __hip_atomic_fetch_max(&a.xwait[(size_t)r * a.W + w], (unsigned)(dt < 0xffffffffull ? dt : 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid < 64) {                                          // ONE wave, the one that polled: drop this XCD's stale lines
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");          // system scope
    drain_stores();                                        // the invalidate completes before the barrier releases the readers
  }
  __syncthreads();
  if (!*s_ok) return false;
  // the slots of my buffer, added in rank order -- every rank's value REQUESTED before the first is waited for (as a loop over
  // the world with the addition in it, the compiler waits for each system-scope load before it issues the next: eight
  // dependent round trips per waypoint on eight GPUs)
  for (int c = tid; c < NC; c += nthreads) {
    double v[POCS_XCHG_MAX_WORLD];
#pragma unroll
    for (int q = 0; q < POCS_XCHG_MAX_WORLD; ++q)
      v[q] = q < x.world ? __longlong_as_double((long long)__hip_atomic_load(
                 reinterpret_cast<const unsigned long long*>(xchg_row(x.buf[x.rank], parity, q, r) + c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM))
                         : 0.0;
    asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]));
    static_assert(POCS_XCHG_MAX_WORLD == 8, "eight values pinned");
    double tot = 0.0;
#pragma unroll
    for (int q = 0; q < POCS_XCHG_MAX_WORLD; ++q) if (q < x.world) tot += v[q];
    a.moments[((size_t)w * a.nruns + r) * NC + c] = tot;    // the mixture's moments replace this shard's
    l_mom[c] = tot;
  }
  return true;
}
__global__ __launch_bounds__(128) void k_gmm_exchange(pocs_gmm_launch a, pocs_xchg_dev x, int K) {
  __shared__ double s_adv[POCS_ADV_SCRATCH(POCS_MAX_GAUSSIANS)];
  __shared__ double s_spec[POCS_SPEC_SCRATCH(POCS_MAX_GAUSSIANS)];
  __shared__ int s_ok;
  const int tid = threadIdx.x, r = blockIdx.x, w = a.waypoint, NC = K * POCS_NMOM;
  // an earlier exchange of this call gave up: do not wait another 30 s per waypoint, the call is lost
  if (__hip_atomic_load(&a.sync[POCS_SYNC_ABORT], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;
  double* const l_mom = advance_ptrs(a, K, w + 1, r, s_adv).l_mom;
  if (!gmm_exchange_rows(a, x, x.epoch, x.parity, K, w, r, a.moments + ((size_t)w * a.nruns + r) * NC, l_mom, tid, 128, &s_ok)) return;
  if (w + 1 < a.W) advance_block(a, K, w + 1, r, s_adv, s_spec, true, tid, 128);     // starts with a barrier after staging
}

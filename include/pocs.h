/* pocs.h -- C ABI of libpocs.so, the MI355X-native collision-probability estimator.
 *
 * This is the drop-in boundary for the reference's OpenRAVE module `MCModule`
 * (mcsimplugin/mcsimplugin.cpp:7-255) and the estimator it owns (`MCSimulator`,
 * mcsimplugin/MCSimulator.h:93-930; `GM_Model`, mcsimplugin/GM_Model.h:34-126).
 * Plain C types only; no exceptions cross this boundary.  Every function that returns `int`
 * returns POCS_OK (0) or a negative POCS_E_* code; pocs_last_error() gives the text.
 *
 * One context = one GPU = one host thread at a time (the reference is single-threaded and takes
 * the environment mutex per query, MCSimulator.h:272,282).  Contexts are independent.
 * There is no CPU fallback: pocs_create fails when no HIP device is usable.
 */
#ifndef POCS_H
#define POCS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POCS_OK 0
#define POCS_E_ARG (-1)        /* bad argument / wrong token count                           */
#define POCS_E_ORDER (-2)      /* command sent before the one it depends on (see below)      */
#define POCS_E_STATE (-3)      /* run requested with incomplete configuration                */
#define POCS_E_DEVICE (-4)     /* HIP error (text holds hipGetErrorString)                   */
#define POCS_E_UNKNOWN_COMMAND (-5)
#define POCS_E_BUFFER (-6)     /* caller buffer too small                                    */

typedef struct pocs_ctx pocs_ctx;

/* ---- lifetime: replaces CreateInterfaceValidated / MCModule ctor / DestroyPlugin ----------
 * (mcsimplugin.cpp:12-45,236-255; MCSimulator ctor MCSimulator.h:139-156). `device` is the HIP
 * ordinal. */
int pocs_create(pocs_ctx** out, int device);
void pocs_destroy(pocs_ctx* ctx);
const char* pocs_last_error(const pocs_ctx* ctx);
const char* pocs_version(void);

/* ---- collision world: replaces the OpenRAVE environment + robot handed to the MCSimulator
 * ctor and queried at MCSimulator.h:275,279.  boxes = M x {cx, cy, half_x, half_y, yaw_rad}. */
int pocs_set_footprint(pocs_ctx* ctx, double dx, double dy, double half_x, double half_y);
int pocs_set_obstacles(pocs_ctx* ctx, const double* boxes, int M);

/* ---- moving obstacles: a collision world per waypoint (ours) --------------------------------
 * A planner with a prediction for a pedestrian, a door or a second robot hands over S worlds of M boxes each:
 *   boxes: S x M x {cx, cy, half_x, half_y, yaw_rad}, world s = boxes[s], 0 <= M <= 64 (the same M in every step),
 *   1 <= S <= POCS_MAX_WORLD_STEPS.  Centre, half extents and yaw may all change from step to step (a growing box is how a
 *   caller expresses the growing uncertainty of a prediction).
 * World s is the collision world AT WAYPOINT s; waypoints >= S see world S - 1 (the last world holds).  Waypoint 0 is the initial
 * cloud or mixture, waypoint s + 1 what control s produces: the indexing of pocs_mc_get_waypoint_counts.  The estimator tests
 * poses at waypoints only, as the reference does: nothing is interpolated between two worlds.
 * The time axis in every call shape: a single run, a batch, run-ahead, a shard, the step API (pocs_gmm_step_local,
 * pocs_gmm_sample_local, pocs_gmm_sample_exchange_local) and the whole-call exchange: the waypoint index; a call of plans: each
 * plan's own waypoint index (all plans start at time 0); a tree: a node's depth.  The risk bound (GMM and MC) works unchanged on
 * top: it reads counts, not worlds.
 * S = 1 is pocs_set_obstacles(boxes, M), bit for bit, in every result and getter (for every table this function accepts: it
 * also refuses values that are not finite, which pocs_set_obstacles, checking the half extents only, takes as it always has).  S = 0 with M = 0 clears the schedule and leaves
 * an explicitly empty static world, as clearObstacles does.  pocs_set_obstacles and clearObstacles replace the schedule with a
 * static world; addObstacle replaces it with world 0 plus the new box.  pocs_set_footprint re-prepares the records of every step.
 * POCS_E_ARG (the context keeps the world it had): a null `boxes` with M > 0, M or S out of range, any value that is not finite,
 * a half extent <= 0.
 * pocs_get_world_steps: S of the schedule in force; 1 for a static world; 0 for a context without a collision world.
 * Launches: every per-waypoint launch (all GMM forms, the tree's levels, the MC init and per-step launches) is handed the record
 * of its own waypoint and is otherwise what it is under a static world.  The fused MC roll-out (POCS_OPT_MC_FUSED = 1) under
 * S > 1 is a kernel of its own, which restages the world per step while the step computes (k_mc_fused_sched, DESIGN.md section
 * 5; kept because it is faster than the per-step form there: profiles/obstacle_schedule_vs_parent.txt); with S = 1 it is the
 * kernel it has always been.  Particles, hit counters and counts are the same bits in both MC forms.
 * pocs_probe_device_collide keeps probing world 0.  The text channel has no command for a schedule. */
#define POCS_MAX_WORLD_STEPS 4096
int pocs_set_obstacle_schedule(pocs_ctx* ctx, const double* boxes, int M, int S);  /* boxes: S x M x {cx, cy, half_x, half_y, yaw_rad} */
int pocs_get_world_steps(const pocs_ctx* ctx);                                      /* S of the schedule in force; 1 for a static world; 0 for none */

/* ---- large worlds: up to POCS_MAX_WORLD_BOXES boxes (ours) -----------------------------------
 * What a planner hands over is often an occupancy grid or a wall made of many small boxes: hundreds to thousands of boxes, almost
 * none of them near the robot at any one waypoint.  pocs_set_world takes such a table:
 *   boxes: M x {cx, cy, half_x, half_y, yaw_rad}, 0 <= M <= POCS_MAX_WORLD_BOXES.
 * With M <= 64 it IS pocs_set_obstacles(boxes, M): the same device state, the same kernels, the same bits.  With M > 64 it installs a
 * LARGE static world, and 64 (POCS_MAX_OBSTACLES) becomes the number of boxes that may be IN REACH of one run at one waypoint:
 *   - both estimators compute, bit for bit, what the full loop over all M boxes computes (what the CPU oracle computes).  Nothing
 *     spatial is built: the GMM path culls the table by brute force once per run and waypoint -- one small launch in front of every
 *     waypoint's sampling launch, inside the same replayed graph -- against the box of every pose the run's mixture can draw; the MC
 *     path culls it per wave and particle iteration against the box of the wave's 64 poses (DESIGN.md sections 1 and 5);
 *   - a GMM call in which some run has more than 64 boxes in reach at some waypoint fails with POCS_E_STATE (the message names the
 *     lowest such waypoint and its count), its results are discarded and the context stays usable; an MC call has no such limit;
 *   - pocs_get_world_reach: for the selected run (pocs_select_batch_run; plan p while plans are set; the run served last under
 *     run-ahead) of the last GMM call, per waypoint the number of boxes its cull kept; a waypoint that was not evaluated (behind a
 *     stop under the risk bound) gives 0.  Writes and returns the run's (the plan's) number of waypoints; stays readable after a
 *     call that failed on overflow; POCS_E_STATE when the last GMM call did not run under a large world, POCS_E_BUFFER for a short
 *     buffer;
 *   - batches, run-ahead, sub-batches, pocs_set_plans, the risk bound (GMM and MC), POCS_OPT_MC_WAYPOINT_COUNTS, POCS_OPT_STORE_SAMPLES,
 *     POCS_OPT_MC_NONTEMPORAL work as under a small world and give the bits a small world with the same boxes in reach gives.  A GMM
 *     call of ONE run takes the ticket form (the lone form builds a waypoint's mixture in its own heads, so nothing could cull ahead
 *     of it): POCS_OPT_LONE_CALL has no effect under a large world; the results are the same bits either way.
 * It replaces whatever world or schedule was set; pocs_set_obstacles, pocs_set_obstacle_schedule and clearObstacles replace a large
 * world.  pocs_set_footprint re-prepares its records.  pocs_get_world_steps answers 1.
 * What a large world does not combine with is refused, with a message that names the call and the mode in its way, the context left
 * as it was: the matrix of all mode combinations and their codes is DESIGN.md section 9 (from csrc/pocs_modes.hpp).  An obstacle
 * schedule keeps its limit of 64 boxes per step.
 * POCS_E_ARG (the world in force stays): M out of range, a null `boxes` with M > 0, a half extent <= 0, and for M > 64 any value that
 * is not finite.  The text channel has no command for it.
 * pocs_get_world_boxes: M of the world in force -- a large world's, a static world's, a schedule's boxes per step; 0 without one. */
#define POCS_MAX_WORLD_BOXES 4096
int pocs_set_world(pocs_ctx* ctx, const double* boxes, int M);          /* boxes: M x {cx, cy, half_x, half_y, yaw_rad} */
int pocs_get_world_boxes(const pocs_ctx* ctx);
int pocs_get_world_reach(pocs_ctx* ctx, int* out, int cap);             /* per waypoint: boxes in reach of the selected run in the last GMM call */

/* ---- typed twins of the setter commands (argument order = token order of the command) ---- */
int pocs_set_alphas(pocs_ctx* ctx, const double* alphas, int n);            /* mcsimplugin.cpp:174-187 -> MCSimulator.h:224-230; n must be 4 */
int pocs_set_q(pocs_ctx* ctx, double q);                                    /* :168-172 -> :232-235 */
int pocs_set_num_landmarks(pocs_ctx* ctx, int n);                           /* :142-146 -> :208-212 */
int pocs_set_landmarks(pocs_ctx* ctx, const double* xs_then_ys, int n);     /* :148-166 -> :214-218; needs set_num_landmarks first */
int pocs_set_num_particles(pocs_ctx* ctx, long long n);                     /* :136-140 -> :182-186 */
int pocs_set_initial_covariance(pocs_ctx* ctx, const double* row_major9);   /* :121-134 -> :176-180 */
int pocs_set_path_length(pocs_ctx* ctx, int W);                             /* :115-119 -> :200-202 */
int pocs_set_trajectory(pocs_ctx* ctx, const double* xs_ys_thetas, int W);  /* :83-97 -> :158-168 (also sets the initial mean); needs set_path_length first */
int pocs_set_odometry(pocs_ctx* ctx, const double* r1s_trs_r2s, int Wm1);   /* :99-113 -> :170-174 */
int pocs_set_num_gaussians(pocs_ctx* ctx, int K);                           /* :49-54 -> :188-192; 1..8 */
int pocs_set_num_gmm_samples(pocs_ctx* ctx, long long n);                   /* :56-61 -> :194-198 */
int pocs_set_seed(pocs_ctx* ctx, uint64_t seed);                            /* new: the reference seeds from the clock (MCSimulator.h:141, GM_Model.h:53-54) */

/* ---- the two estimators ---------------------------------------------------------------- */
int pocs_run_simulation(pocs_ctx* ctx, double* probability);       /* runSimulation,    mcsimplugin.cpp:75-81 -> MCSimulator.h:361-365 */
int pocs_run_gmm_estimation(pocs_ctx* ctx, double* probability);   /* runGMMEstimation, mcsimplugin.cpp:66-72 -> MCSimulator.h:354-358 */

/* ---- the text channel: same 15 command names and token grammar as MCModule's SendCommand
 * (mcsimplugin.cpp:13-44) plus `setSeed`, `setFootprint`, `addObstacle`, `clearObstacles`,
 * `help`.  `line` = "<name> <tokens...>".  The reply text (the probability for run*, "output"
 * for MyCommand) is written NUL-terminated into out[cap]. */
int pocs_send_command(pocs_ctx* ctx, const char* line, char* out, size_t cap);

/* ---- options (ours) -------------------------------------------------------------------- */
#define POCS_OPT_STORE_SAMPLES 1   /* 1 (default): GMM samples + flags are written to HBM (26 B/eval, auditable); 0: not stored */
#define POCS_OPT_MC_FUSED 2        /* 0 (default): one launch per waypoint, particles streamed through HBM (56 B/eval); 1: whole roll-out in registers */
#define POCS_OPT_USE_GRAPH 3       /* 1 (default): the per-run launch sequence is replayed from a hipGraph */
#define POCS_OPT_PROFILE 4         /* 1: bracket every launch of the hot kernel with hipEvents (eager launches; see pocs_get_kernel_time).  An event
                                      between two kernels costs the bracketed kernel ~9 us of dispatch that back-to-back launches overlap.
                                      2 (whole-run GMM calls): the replayed graph as it runs in production between one pair of events;
                                      pocs_get_kernel_time then returns the span and W, i.e. the mean launch PERIOD (duration + gap) */
#define POCS_OPT_RUN_AHEAD 5       /* R > 1, or 0 = R sized per call from the sample / particle count (8..64: the reference's 200 runs
                                      of 10^4 samples go 64 at a time, a 10^6-sample estimation 16 at a time); default 1 = off.
                                      With one run per call (batch 1), a run* call evaluates the NEXT R
                                      runs of the context in one launch and the following R-1 calls are served from it -- the
                                      reference driver's one-command-per-run loop (MCSimulation.py:238-256) at batch throughput.
                                      Same runs, same seeds, and -- the moment sums being defined on a run's virtual slices, not on
                                      the launch -- bit for bit the same results and getters as one launch per run
                                      (tests/test_gpu_parity.py::test_timed_launch_shapes_against_the_oracle); any setter ends the
                                      serving and the run counter resumes after the last run handed out.  Text: setRunAhead R */
#define POCS_OPT_PERSISTENT 6      /* retired (round 3): 0 is accepted, 1 returns POCS_E_ARG.  Round 2's queue-driven whole-call kernel
                                      (k_gmm_run) was slower than one launch per waypoint at every batch size measured and is gone
                                      (DESIGN.md section 5). */
#define POCS_OPT_LONE_CALL 7       /* 1 (default): a whole-run GMM call of ONE run (batch 1, no run-ahead, one GPU) uses launches that close
                                      the previous waypoint in every block's head instead of tickets and a closing block (no one else
                                      is in flight to hide a closer behind): 10 % less time per waypoint, the same bits
                                      (tests/test_gpu_parity.py::test_lone_call_changes_no_bit).  0: the ticket form always.  No effect under
                                      a large world (pocs_set_world with more than 64 boxes): the ticket form always, the same bits. */
#define POCS_OPT_SUB_BATCHES 8     /* 0 (default): a whole-run call of >= 8 runs and >= 1.2e6 evaluations per waypoint is issued as TWO sub-batches
                                      on two streams, so that one sub-batch's launch tail (its last blocks' slow end, the serial mixture advance
                                      of its last closer, the launch boundary) is covered by the other's sampling blocks: +4 ... +11 % measured;
                                      smaller calls as one launch per waypoint.  1 / 2 force one form.  The moment sums are defined on a run's
                                      virtual slices, not on the launch: no bit of any result changes. */
#define POCS_OPT_MC_NONTEMPORAL 9  /* -1 (default): k_mc_step streams past the caches when the batch's particle state (28 B per particle)
                                      exceeds the 256 MB Infinity Cache and uses plain accesses when it fits; 0 / 1 force one form.
                                      Same results either way. */
#define POCS_OPT_PLAN_SEEDS 10     /* a call of plans (pocs_set_plans): 0 (default): plan p draws the stream of run run_index + p, as run p
                                      of a batch does, and the run counter advances by P; 1, common random numbers: every plan draws the
                                      stream of run run_index and the counter advances by 1 -- the difference between two plans'
                                      probabilities, what a planner compares, then has a much smaller variance */
#define POCS_OPT_MC_WAYPOINT_COUNTS 11   /* 0 (default): an MC call is what it has always been.  1: MC calls also count, per run and waypoint w, the
                                      particles that collide at w and at no waypoint before it (pocs_mc_get_waypoint_counts), in both launch
                                      forms (POCS_OPT_MC_FUSED 0 and 1); no other result changes */
#define POCS_OPT_MC_RISK_BOUND 12  /* 0 (default): pocs_run_simulation ignores the risk bound.  1: an MC call of plans under a bound in (0, 1)
                                      stops a plan at the first waypoint where its share of collided particles reaches the bound
                                      (pocs_set_plan_risk_bound); such a call counts as under POCS_OPT_MC_WAYPOINT_COUNTS and takes the per-step
                                      launch form whatever POCS_OPT_MC_FUSED says.  No effect without plans or with the bound off */
#define POCS_OPT_OBSTACLE_COUNTS 13 /* 0 (default): every call is what it has always been.  1: every pocs_run_gmm_estimation, pocs_run_simulation and
                                      step-API sequence also fills, per run / plan / tree node, a table of collision counts per waypoint and
                                      obstacle box (pocs_get_obstacle_counts); the launches are then counting forms of the kernels, and an
                                      MC call counts as under POCS_OPT_MC_WAYPOINT_COUNTS.  No other result changes by a bit.  Not inside a
                                      begin/end sequence (POCS_E_ORDER) */
int pocs_set_option(pocs_ctx* ctx, int option, long long value);

/* ---- batches of independent runs (ours) --------------------------------------------------
 * The reference's driver performs its 200 estimations one after the other
 * (MCSimulation.py:238-256).  With a batch of R, one pocs_run_gmm_estimation / begin..end
 * sequence advances R independent estimations in lockstep (one launch per waypoint for all of
 * them); run i of the batch draws exactly what the i-th of R consecutive single runs would have
 * drawn -- and computes, bit for bit, what it would have computed: the launch shape changes no result.
 * pocs_run_gmm_estimation returns run 0's probability, pocs_get_batch_probabilities all
 * R.  The per-waypoint exchange of the step API then covers R x 11K doubles.  runSimulation is
 * batched the same way (pocs_mc_get_batch_counts: the shard's collided particles per run). */
int pocs_set_batch(pocs_ctx* ctx, int runs);
int pocs_get_batch_probabilities(pocs_ctx* ctx, double* out, int cap);
int pocs_select_batch_run(pocs_ctx* ctx, int run);   /* the getters below (waypoint probabilities, moments, mixture state, host chain,
                                                        samples / particles) expose run `run` of the last batch; a new launch selects run 0 */

/* ---- batches of candidate plans (ours) ---------------------------------------------------
 * A planner has many candidate plans and wants the collision probability of each.  With P plans set
 * (1 <= P <= 256), one pocs_run_gmm_estimation / pocs_run_simulation call evaluates every plan once, in
 * one batch, and each plan gets bit for bit what a context holding that plan alone computes for it.
 *   W[p] >= 1 is plan p's length.  trajs: plan p's trajectory, 3 x W[p] by component (x_0..x_{W-1}
 *   y_0.. theta_0..), as pocs_set_trajectory takes it, the plans' blocks concatenated in plan order;
 *   odoms: its odometry, 3 x (W[p] - 1) by component as pocs_set_odometry takes it, concatenated the
 *   same way (may be NULL if every plan has one waypoint).  P = 0 clears the plans: the context goes
 *   back to its single plan and batch.  Bad input: POCS_E_ARG.  Setting plans drops the last results.
 * While plans are set:
 *   - the batch is P; pocs_get_batch_probabilities / pocs_mc_get_batch_counts return the P results in
 *     plan order, pocs_run_* returns plan 0's;
 *   - pocs_select_batch_run(p) selects plan p for the getters: pocs_get_path_length returns W[p], the
 *     waypoint getters cover W[p] waypoints (a waypoint >= W[p] is POCS_E_ARG), samples and particles
 *     are plan p's;
 *   - seeds: POCS_OPT_PLAN_SEEDS;
 *   - pocs_set_batch, pocs_set_path_length, pocs_set_trajectory and pocs_set_odometry return
 *     POCS_E_ORDER (clear the plans with pocs_set_plans(ctx, 0, ...) first); a shard (pocs_set_shard
 *     other than (-1, -1)), the step API (pocs_gmm_begin) and the in-library exchange (pocs_xchg_*)
 *     return POCS_E_STATE: plan batches run on one GPU;
 *   - run-ahead (POCS_OPT_RUN_AHEAD) is not applied.
 * A launch covers only the plans still running: the slots of a batch are ordered by descending plan
 * length, and the launch of waypoint w covers the plans longer than w. */
int pocs_set_plans(pocs_ctx* ctx, int P, const int* W, const double* trajs, const double* odoms);

/* ---- a risk bound for calls of plans (ours) ------------------------------------------------
 * What a planner does with a plan's probability is a chance constraint: a candidate above the bound it plans under is
 * thrown away, however far above.  A plan's probability 1 - prod_w (1 - p_w) never decreases along the plan, so with a
 * bound in (0, 1) set, a GMM call of plans (pocs_run_gmm_estimation while plans are set) stops plan p at the FIRST waypoint
 * s whose running probability c_s = 1 - prod_{v <= s} (1 - p_v) is >= bound -- formed exactly as the final probability is
 * (p_v = collisions / numGMMSamples, the product in waypoint order, IEEE double) -- and evaluates nothing of it beyond:
 *   - pocs_get_batch_probabilities()[p] (pocs_run_gmm_estimation's value for plan 0) is c_s: a lower bound of the plan's
 *     full probability that is already >= bound.  A plan that never reaches the bound, or reaches it only at its last
 *     waypoint, gets its full probability as without a bound;
 *   - pocs_get_plan_evaluated: per plan, in plan order, the number of waypoints evaluated, 1 <= E[p] <= W[p]; E[p] < W[p]
 *     means the plan was stopped.  POCS_E_BUFFER for cap < P, POCS_E_STATE when the last call was not a call of plans;
 *     W[p] after a pocs_run_simulation call or with the bound off;
 *   - with plan p selected, pocs_get_waypoint_probabilities writes (and returns) E[p] values, pocs_get_moments and
 *     pocs_get_gmm_state cover waypoints 0 .. E[p] - 1 (POCS_E_ARG beyond), pocs_get_path_length stays W[p], and
 *     pocs_copy_gmm_samples returns the samples of waypoint E[p] - 1, the last one drawn for that plan;
 *   - everything computed before the stop is, bit for bit, what the same plan gets with the bound off; seeds and the run
 *     counter (POCS_OPT_PLAN_SEEDS) do not depend on who stopped.
 * bound >= 1.0 (the default is 1.0): off -- every call is what it is without this function.  bound <= 0 or NaN: POCS_E_ARG.
 * The bound belongs to the context: it survives pocs_set_plans, and has no effect while no plans are set (pocs_set_batch,
 * run-ahead, the step API; sharded contexts refuse plans).
 * The stop is decided and obeyed on the device, inside the call's one replayed graph; the host restates
 * the rule on the moments it reads back, and a call whose two stops differ returns POCS_E_DEVICE.
 * pocs_run_simulation ignores the bound BY DEFAULT.  With POCS_OPT_MC_RISK_BOUND = 1 an MC call of plans under a bound in (0, 1)
 * stops plan p at the FIRST waypoint s with (double)C[s] / (double)N >= bound -- C[s] = F[0] + ... + F[s] the particles that
 * have collided at waypoints 0 .. s (pocs_mc_get_waypoint_counts), N = numParticles, one IEEE division -- and moves its particles
 * no further:
 *   - pocs_mc_get_batch_counts()[p] is C[s], pocs_get_batch_probabilities()[p] (pocs_run_simulation's value for plan 0) is
 *     C[s] / N, pocs_get_plan_evaluated()[p] is s + 1, pocs_mc_get_waypoint_counts covers s + 1 waypoints, and
 *     pocs_copy_particles returns the cloud at waypoint s with its hit counters over waypoints 0 .. s.  A plan that never reaches
 *     the bound, or only at its last waypoint, gets what it gets without the option;
 *   - everything before the stop is bit for bit what the plan gets unstopped; seeds and the run counter do not depend on who
 *     stopped;
 *   - the stop is decided on the device from the counts that the earlier launches of the call's graph completed, one launch per
 *     waypoint: the fused kernel (POCS_OPT_MC_FUSED = 1) meets no launch boundary between steps, so a call with the MC stop active
 *     takes the per-step form whatever that option says.  The host restates the rule on the counts it reads back; a mismatch
 *     is POCS_E_DEVICE and the results are discarded;
 *   - stopped plans' blocks are still launched and return in their head. */
int pocs_set_plan_risk_bound(pocs_ctx* ctx, double bound);
int pocs_get_plan_evaluated(pocs_ctx* ctx, int* out, int cap);

/* ---- a tree of candidate plans (ours) ------------------------------------------------------
 * What a planner holds is a search tree: candidates that share long prefixes (RRT extensions, lattice expansions).  With a
 * tree of T nodes set (1 <= T <= POCS_MAX_TREE_NODES), one pocs_run_gmm_estimation / pocs_run_simulation call evaluates every
 * NODE once -- not every root-to-leaf path -- and returns the running probability of the path root -> n for every node n.
 *   parent[0] == -1 and 0 <= parent[n] < n otherwise: one root, nodes in topological order.  poses: the nodes' poses, 3 x T by
 *   component (x_0..x_{T-1} y_0.. theta_0..); odoms: the control of the edge parent[n] -> n, 3 x T by component (node 0's
 *   entry is ignored; may be NULL for T = 1).  A path's length, depth + 1, is bounded as pocs_set_path_length bounds it.
 *   Anything else: POCS_E_ARG.  nodes = 0 clears the tree: the context goes back to its single plan and batch.  Setting a
 *   tree drops the last results.
 * THE CONTRACT: for every node n, every value below is bit for bit what pocs_set_plans computes for the path root -> n alone
 * under POCS_OPT_PLAN_SEEDS = 1, on a context with the same configuration, seed and run counter -- GMM and MC, both MC launch
 * forms.  (The host chain is keyed by (seed, step), the mixture of a waypoint depends on the waypoints before it only, and
 * the moment sums do not depend on the launch they travel in: a shared prefix computes the same bits for every path.)
 * While a tree is set:
 *   - a call draws the stream of run run_index, as POCS_OPT_PLAN_SEEDS = 1 does for plans, and the run counter advances by 1;
 *     pocs_run_gmm_estimation / pocs_run_simulation return node 0's value;
 *   - pocs_get_tree_probabilities: per node, in node order, the running probability 1 - prod (1 - p_v) over the path root -> n
 *     (after an MC call: collided at or before n / numParticles); pocs_mc_get_tree_counts: after an MC call, per node, the
 *     particles that collided at or before n on its path; POCS_E_BUFFER for cap < T, POCS_E_STATE when the last call was not
 *     such a call;
 *   - pocs_select_tree_node(n) makes the getters show the path root -> n as a plan of depth(n) + 1 waypoints:
 *     pocs_get_path_length, pocs_get_waypoint_probabilities, pocs_get_moments, pocs_get_gmm_state, pocs_get_host_chain,
 *     pocs_mc_get_waypoint_counts (always counted on a tree, POCS_OPT_MC_WAYPOINT_COUNTS or not).  pocs_copy_particles serves
 *     the nodes of the DEEPEST level only (an MC call keeps two levels of particle state, not T clouds) and returns
 *     POCS_E_STATE for any other node.  A new call selects node 0;
 *   - samples are NOT stored, whatever POCS_OPT_STORE_SAMPLES says: pocs_copy_gmm_samples returns POCS_E_STATE;
 *   - what a tree does not combine with (a set of plans, the single plan's setters, a shard, the step API, the exchange, a large
 *     world) is refused: the matrix with its codes is DESIGN.md section 9; run-ahead is not applied; POCS_OPT_PROFILE = 1 runs
 *     the call eagerly without per-launch times.
 * Risk bound (pocs_set_plan_risk_bound in (0, 1)): a GMM call does not evaluate the descendants of a node whose running
 * probability has reached the bound.  The stop is decided on the device -- a node's launch reads its parent's stop word and
 * inherits it -- and the host restates the rule on what it reads back (a mismatch: POCS_E_DEVICE).  A stopped node's entry of
 * pocs_get_tree_probabilities is its own running probability; an unevaluated node's entry is its nearest evaluated ancestor's,
 * and its byte of pocs_get_tree_evaluated is 0 (1 for every evaluated node; all 1 with the bound off and after an MC call).
 * With an unevaluated node selected the getters cover the evaluated part of its path.  Everything evaluated is bit for bit
 * what it is with the bound off.  An MC call on a tree IGNORES the bound, POCS_OPT_MC_RISK_BOUND included.
 * Launches: the nodes are laid out level by level; per level a GMM call makes one small launch that builds the nodes'
 * mixtures from their parents' and one sampling launch (more for a level wider than 256 nodes); an MC call makes one launch
 * per level that moves every node's particles from its parent's cloud into its own -- this per-step form also serves
 * POCS_OPT_MC_FUSED = 1 (same arithmetic, same bits) -- and refuses (POCS_E_ARG) a tree whose two widest consecutive
 * levels' clouds would not fit (DESIGN.md sections 3 and 5). */
#define POCS_MAX_TREE_NODES 4096
int pocs_set_plan_tree(pocs_ctx* ctx, int nodes, const int* parent,
                       const double* poses,   /* 3 x nodes by component: x_0..x_{T-1} y_0.. theta_0.. */
                       const double* odoms);  /* 3 x nodes by component: the control of the edge parent[n] -> n (node 0's entry is ignored) */
int pocs_get_tree_probabilities(pocs_ctx* ctx, double* out, int cap);   /* per node, node order: running probability of the path root -> n */
int pocs_get_tree_evaluated(pocs_ctx* ctx, unsigned char* out, int cap);/* per node: 1 evaluated, 0 cut off below a stopped ancestor */
int pocs_mc_get_tree_counts(pocs_ctx* ctx, unsigned long long* out, int cap); /* MC: per node, particles that collided at or before n on its path */
int pocs_select_tree_node(pocs_ctx* ctx, int node);

/* ---- sharding over GPUs (one process per GPU; the caller owns the collective) -----------
 * A context evaluates global sample / particle indices [first, first+count) of the N configured;
 * random draws are keyed by the GLOBAL index, so every sample, flag, survivor count and hit counter is the same
 * whatever the partition.  The moment SUMS of the GMM path are another matter: each shard adds its samples in its own
 * summation tree (a function of the shard's sample count: 512-pair chunks, at most 256 virtual slices -- part of the
 * numerics version pocs_version() names) and the ranks' totals are added in rank order, so the sums of a sharded run
 * differ from the one-GPU run's in their last bits (a different order of the same additions): bit-equality of sums,
 * mixture states and probabilities holds PER SHARD SIZE -- the same world size and shards reproduce bit for bit --,
 * not across world sizes (8 shards of cfg3 against one GPU: all counts equal, final probability equal, sums within
 * 8e-10 of their scale). */
int pocs_set_shard(pocs_ctx* ctx, long long first, long long count);   /* (-1, -1) = the whole range again */
int pocs_set_stream(pocs_ctx* ctx, void* hip_stream);                 /* launch on this stream (e.g. a torch stream).  NULL = back to the context's
                                                                          own NON-BLOCKING stream -- not the null stream: a caller whose
                                                                          other work (collectives, copies) runs on the null stream -- torch's
                                                                          default "current stream" has handle 0 -- passes hipStreamLegacy
                                                                          ((hipStream_t)1), or the two are not ordered (parallel.GpuEngine does) */

/* GMM, one waypoint at a time: begin -> for w in 0..W-1 { step_local(w); <all-reduce SUM of
 * moments_ptr(w), moments_len doubles>; } -> end.  step_local(w) first folds the (already
 * reduced) moments of w-1 into the mixture, then samples + collides + reduces this shard. */
int pocs_gmm_begin(pocs_ctx* ctx);
int pocs_gmm_step_local(pocs_ctx* ctx, int waypoint);
/* The two halves of step_local, for a caller that interleaves two contexts on one GPU and wants
 * the small advance launch to overlap the other context's sampling kernel: advance_local(w) builds
 * the mixture of waypoint w from the reduced moments of w-1, sample_local(w) samples + collides +
 * reduces; both on the context's stream, in this order. */
int pocs_gmm_advance_local(pocs_ctx* ctx, int waypoint);
int pocs_gmm_sample_local(pocs_ctx* ctx, int waypoint);
void* pocs_gmm_moments_ptr(pocs_ctx* ctx, int waypoint);              /* device pointer, f64[moments_len] */
int pocs_gmm_moments_len(const pocs_ctx* ctx);                       /* batch x 11 x K: one exchange covers every run of the batch */
int pocs_gmm_bind_moments(pocs_ctx* ctx, void* device_ptr, long long len_doubles);  /* optional: keep the [W][batch][11K] moments in a caller-owned device buffer (e.g. a torch tensor handed to all_reduce); NULL unbinds */
int pocs_gmm_end(pocs_ctx* ctx, double* probability);
/* The exchange without a collective library, for the GPUs of ONE node (11 K doubles per
 * run and waypoint are latency, not bandwidth): every rank owns a small device buffer that all ranks map
 * (HIP IPC); pocs_gmm_exchange_local(w) -- one small launch, after pocs_gmm_sample_local(w) -- writes this
 * rank's moments of waypoint w into its slot of EVERY rank's buffer (one hop over xGMI), waits for the
 * world's slots in its own buffer, adds them in rank order (every rank the same bits) and builds the
 * mixture of waypoint w+1, so the sequence per waypoint is sample_local(w), exchange_local(w) -- no
 * advance_local, no all-reduce.  sample_local and step_local never exchange themselves, moments buffer bound
 * or not: their moments stay the shard's until the caller's exchange.  Setup, once: pocs_xchg_create on every rank (returns the 64-byte IPC
 * handle of its buffer), the caller gathers the handles (any host channel), pocs_xchg_connect(handles of
 * rank 0 .. world-1, 64 bytes each).  world <= 8, batch <= 256.
 * Two rules for connected contexts: (1) LOCK STEP -- every rank calls pocs_gmm_begin the same number of times
 * and exchanges the same waypoints in the same order: the count of begin..end sequences is part of every row's
 * epoch and of the choice between the two slot sets; (2) NOBODY LEAVES EARLY -- a rank must not destroy its
 * context (or exit) while a peer may still write into or read from its buffer: put a barrier of the host
 * channel between the last pocs_gmm_end and pocs_destroy, as bench.py and the tests do.
 * A peer that never arrives makes the kernel's bounded wait (30 s, once per call) give up: pocs_gmm_end then
 * returns POCS_E_DEVICE and the call's results are discarded. */
int pocs_xchg_create(pocs_ctx* ctx, int world, int rank, void* handle64_out);
int pocs_xchg_connect(pocs_ctx* ctx, const void* handles_world_x_64, int world);
int pocs_gmm_exchange_local(pocs_ctx* ctx, int waypoint);
/* THE WHOLE CALL IN ONE LIBRARY CALL (round 4; what bench.py uses for N > 1 by default, POCS_ONEHOP=2, after a probe of it on
 * the node): a context that holds a shard (pocs_set_shard) and is connected to its peers (pocs_xchg_create / pocs_xchg_connect),
 * with no caller-owned moments buffer bound, runs the SHARDED estimation when pocs_run_gmm_estimation (or the text command) is
 * called on it: the library replays the call from its hipGraph -- the same launches, the same two sub-batches as on one GPU -- and
 * the block that closes a run's waypoint exchanges the run's moments with the other ranks over one hop, adds them in rank order
 * and builds the next mixture (as pocs_gmm_sample_exchange_local below does per waypoint).  Every rank returns the same
 * probabilities; the getters show the whole mixture's moments and states.  The call's number -- part of every row's epoch --
 * travels in the run headers uploaded per call, so the replayed graph needs no re-capture.  Rules as below: lock step (every
 * connected rank makes the same calls in the same order), nobody leaves early; a peer that never arrives makes the call return
 * POCS_E_DEVICE after the kernel's bounded wait.  Only the whole call exchanges by itself: on the same context the step API
 * (pocs_gmm_sample_local / pocs_gmm_step_local) leaves the shard's sums for pocs_gmm_exchange_local or the caller's all-reduce.
 * The same exchange one waypoint at a time, launches issued by the caller (POCS_ONEHOP=3; round 3's default):
 * POCS_ONEHOP=1 is the two-launch form above, POCS_ONEHOP=0 one RCCL all-reduce per waypoint): the block that closes a run's
 * waypoint is also its messenger -- it sends the shard's moments, waits for the world's, adds them in rank
 * order and builds the next mixture, while the launch's finished blocks have already given their CUs to
 * whatever else is queued (a second context's sampling launch).  Per waypoint: sample_exchange_local(w);
 * before waypoint 0: advance_local(0).  Same results as sample_local + exchange_local, bit for bit. */
int pocs_gmm_sample_exchange_local(pocs_ctx* ctx, int waypoint);
/* MC: the shard's count of particles that collided at least once (device-synchronous). */
int pocs_mc_run_local(pocs_ctx* ctx, unsigned long long* collided);            /* run 0 of the batch */
int pocs_mc_get_batch_counts(pocs_ctx* ctx, unsigned long long* out, int cap);   /* every run of the last MC batch */
/* MC under POCS_OPT_MC_WAYPOINT_COUNTS: the first-collision profile of the selected run (pocs_select_batch_run; plan p while plans
 * are set; the run served last under run-ahead): out[w] = the shard's particles that collide at waypoint w and at no waypoint
 * before it -- waypoint 0 is the initial cloud, waypoint s + 1 what control s produces.  Their sum is the run's entry of
 * pocs_mc_get_batch_counts; out[0] + ... + out[s] over N particles is the MC counterpart of the GMM path's running probability;
 * the shards' profiles add up to the whole run's.  Integer counts: the same whatever the launch form, the grid and the
 * partition.  Writes and returns the number of waypoints covered (a plan's own length, or the waypoints before its stop).
 * POCS_E_BUFFER for a short buffer; POCS_E_STATE when the last call was not an MC call or ran with the option off. */
int pocs_mc_get_waypoint_counts(pocs_ctx* ctx, unsigned long long* out, int cap);
/* Under POCS_OPT_OBSTACLE_COUNTS: which box a plan's risk comes from.  The table A[w][m] of the selected run (pocs_select_batch_run;
 * plan p while plans are set; the path root -> n for pocs_select_tree_node(n); the run served last under run-ahead), m = the index
 * of the box in the table the caller handed over (pocs_set_obstacles, addObstacle order, world min(w, S - 1) of
 * pocs_set_obstacle_schedule):
 *   GMM  A[w][m] = the shard's samples drawn at waypoint w whose footprint touches box m;
 *   MC   A[w][m] = the shard's particles whose FIRST collision is at waypoint w and which touch box m there: the split of
 *        pocs_mc_get_waypoint_counts by box.
 * Not exclusive: a sample or particle that touches two boxes counts for both, so max_m A[w][m] <= collisions at w <= sum_m A[w][m].
 * "Touches" is the collision test's own answer for that box: a pose collides exactly when it touches at least one.  Integer counts:
 * the same whatever the launch form, the grid and the shard partition; the table is the shard's, the shards' tables add up to the
 * whole run's (the in-library exchange does not carry them).
 * Writes E x M values row-major (waypoint-major), *boxes = M, and returns E, the waypoints covered: a plan's own length, or the
 * waypoints before its stop under a risk bound, or depth + 1 for a tree node (the evaluated part under a GMM bound).  M = 0 writes
 * nothing and returns E.  POCS_E_BUFFER for cap < E * M; POCS_E_STATE when the last call ran with the option off (or the option was
 * touched since, or there was no call); POCS_E_ARG for null pointers.  Every call shape serves it: none is refused. */
int pocs_get_obstacle_counts(pocs_ctx* ctx, unsigned long long* out, int cap, int* boxes);

/* ---- clearance levels: near-miss counts per waypoint, for both estimators (ours) ----------------
 * How CLOSE a plan comes, out of the samples a call draws anyway.  For clearances 0 < d_0 < d_1 < ... (at most
 * POCS_MAX_CLEARANCE_LEVELS of them):
 *   grown footprint     the footprint grown by d is {dx, dy, half_x + d, half_y + d}: one IEEE addition per half extent;
 *   within clearance d  a pose is within clearance d of a world exactly when the collision test answers "touches" for the grown
 *                       footprint against that world, touching included.  (The grown box is the definition: no Euclidean distance.)
 *   nesting             every margin of the test is a monotone function of the half extents: a pose within d is within every
 *                       larger d, and a pose that collides is within every clearance.
 * pocs_set_clearance_levels: 0 <= L <= POCS_MAX_CLEARANCE_LEVELS finite distances, 0 < d[0] < d[1] < ...; L = 0 (the default) is
 * off.  POCS_E_ARG otherwise, and the levels in force stay.  The levels belong to the context: they survive pocs_set_plans and
 * pocs_set_footprint (which re-prepares what depends on the footprint).  Like every setter it ends run-ahead serving.  The text
 * channel has no command for it.
 *
 * Where the levels are APPLIED: whole calls on one GPU -- pocs_run_gmm_estimation, pocs_run_simulation (pocs_mc_run_local) -- as
 * single runs, batches in both sub-batch forms, run-ahead, calls of plans with and without the risk bound, over static worlds of up
 * to 64 boxes and obstacle schedules.  A GMM call of one run then takes the ticket form (POCS_OPT_LONE_CALL has no effect, as
 * under a large world), an MC call the per-step form whatever POCS_OPT_MC_FUSED says (as under the MC risk bound).  No other
 * result of any call changes by a bit.  NOT applied -- never refused: a tree of plans, a large world (pocs_set_world with more than
 * 64 boxes), POCS_OPT_OBSTACLE_COUNTS = 1, a shard (with it a bound moments buffer and the exchange) and the step API: there the call
 * is launch for launch and bit for bit the call it is with L = 0, and the two getters below answer POCS_E_STATE.  The same holds
 * while a compound footprint is set (pocs_set_footprint_parts with F > 1): the call is the call with L = 0 under that footprint.
 *
 * pocs_get_clearance_counts serves the selected run (pocs_select_batch_run; plan p while plans are set; the run served last under
 * run-ahead): writes the table A, E x L row-major, sets *levels = L and returns E, the waypoints covered -- a plan's own length, or
 * the waypoints before its stop under a risk bound (GMM, or MC with POCS_OPT_MC_RISK_BOUND).
 *   GMM  A[w][l] = the samples drawn at waypoint w that are within clearance d_l of the world at w (world min(w, S - 1) under a
 *        schedule).  The colliding samples are included: collisions at w <= A[w][0] <= ... <= A[w][L-1] <= N.
 *   MC   A[w][l] = the particles that are within clearance d_l at waypoint w and at no waypoint before it: the first-collision
 *        profile of pocs_mc_get_waypoint_counts as it would be for the grown footprint on the same cloud.
 * POCS_E_BUFFER for cap < E * L, POCS_E_ARG for null pointers, POCS_E_STATE -- the message says which -- when there was no call, L
 * was 0, a setter touched the levels since, or the last call is one the levels are not applied to.
 * pocs_get_batch_clearance_probabilities(level): per run / plan of the last call, in run / plan order (after a run-ahead batch:
 * the run served last),
 *   GMM  1 - prod_w (1 - A[w][level] / N), formed exactly as the final probability is formed from the collision counts: the
 *        division, the product in waypoint order, IEEE double.  NOTE what this number is: the samples of waypoint w are drawn
 *        from the mixture truncated by COLLISIONS before w, not by near misses -- it is the probability of the same estimator with
 *        "within d_level" counted in place of "collides" at every waypoint on the belief the collision estimate propagates, NOT
 *        the collision probability of the grown footprint (whose belief would be truncated differently);
 *   MC   (sum_w A[w][level]) / N, one IEEE division: exactly the collision probability of the grown footprint on this cloud. */
#define POCS_MAX_CLEARANCE_LEVELS 4
int pocs_set_clearance_levels(pocs_ctx* ctx, const double* d, int L);
int pocs_get_clearance_levels(const pocs_ctx* ctx, double* d, int cap);     /* writes and returns L */
int pocs_get_clearance_counts(pocs_ctx* ctx, unsigned long long* out, int cap, int* levels);
int pocs_get_batch_clearance_probabilities(pocs_ctx* ctx, int level, double* out, int cap);

/* ---- compound footprints: a robot of up to four boxes, for both estimators (ours) ----------------
 * A compound footprint is F parts, 1 <= F <= POCS_MAX_FOOTPRINT_PARTS.  Part f is {dx, dy, half_x, half_y}, exactly a
 * pocs_set_footprint footprint: an offset in the base frame and half extents, with no yaw of its own.
 *   touches   a pose touches a world exactly when the collision test (pocs_pose_collides) answers "touches" for at least one part
 *             taken alone as the footprint.  Per part the same operations run in the same order, so the flag is the OR of the parts'
 *             flags, touching included.
 * Everything downstream is what it is today, formed from that flag: the truncation, moment sums, nColl, probabilities and risk
 * bound on the GMM path; hit counters, first-collision profile, counts and the MC risk bound on the MC path.
 *
 * pocs_set_footprint_parts: F = 1 IS pocs_set_footprint(parts[0..3]) -- the same device state, the same kernels, the same bits (as
 * pocs_set_world with at most 64 boxes is pocs_set_obstacles).  POCS_E_ARG, with the footprint in force kept: F out of range, a null
 * pointer, a value that is not finite, a half extent <= 0.  pocs_set_footprint and the text channel's setFootprint replace a
 * compound footprint with the single box.  Like every setter it ends run-ahead serving; it re-prepares the records of every world
 * step, as pocs_set_footprint does.  The text channel has no command for it.  pocs_get_footprint_parts writes the parts in force and
 * returns F (1 after pocs_set_footprint); POCS_E_BUFFER for cap < F.
 *
 * SERVED (F > 1): whole calls on one GPU -- pocs_run_gmm_estimation, pocs_run_simulation, pocs_mc_run_local -- as single runs,
 * batches in both sub-batch forms, run-ahead, calls of plans with and without the risk bound (GMM, and MC with
 * POCS_OPT_MC_RISK_BOUND), POCS_OPT_MC_WAYPOINT_COUNTS, POCS_OPT_STORE_SAMPLES (stored flags are the compound flags), over static
 * worlds of up to 64 boxes and obstacle schedules.  A GMM call of one run takes the ticket form (POCS_OPT_LONE_CALL has no effect,
 * as under a large world), an MC call the per-step form whatever POCS_OPT_MC_FUSED says (as under the MC risk bound).  New values
 * with the same F replay the cached graph (the values live in device memory); a change of F may capture again.
 * REFUSED, never silently served with one box -- a compound footprint changes results: a tree of plans, a large world (more than
 * 64 boxes), a shard, the exchange (created or connected), a bound moments buffer, an open begin/end sequence and pocs_gmm_begin,
 * POCS_OPT_OBSTACLE_COUNTS = 1, pocs_probe_device_collide.  In both directions, with the context left as it was:
 * pocs_set_footprint_parts(F > 1) under any of these answers POCS_E_STATE (POCS_E_ORDER inside a begin/end sequence) and names what
 * is in the way; entering any of them while F > 1 answers POCS_E_STATE, and the message names the call and "a compound footprint
 * is set (pocs_set_footprint_parts)".  Clearance levels are not applied while F > 1 (see there). */
#define POCS_MAX_FOOTPRINT_PARTS 4
int pocs_set_footprint_parts(pocs_ctx* ctx, const double* parts /* F x {dx, dy, half_x, half_y} */, int F);
int pocs_get_footprint_parts(const pocs_ctx* ctx, double* parts, int cap /* in parts */);   /* writes and returns F (1 after pocs_set_footprint) */

/* ---- watched regions: arrival and pass-through counts per waypoint (ours) ------------------------
 * Whether a plan ARRIVES, out of the samples and particles a call draws anyway.  A region is a box {cx, cy, half_x, half_y, yaw_rad} in the
 * layout of pocs_set_obstacles plus a kind; at most POCS_MAX_REGIONS of them.  Regions truncate nothing, are static (they follow no
 * obstacle schedule) and change no other result of any call by a bit.
 *   POCS_REGION_TOUCH  a pose is IN the region exactly when pocs_pose_collides answers "touches" for the robot's footprint in force
 *                      against the one-box table holding the region: the same operations in the same order, touching counts;
 *   POCS_REGION_POINT  the same predicate with the footprint {0, 0, 0, 0}: the pose's reference point lies in the box or on its
 *                      boundary.  (pocs_set_footprint still refuses half extents <= 0: the point is internal to the regions.)
 * pocs_set_regions: 0 <= G <= POCS_MAX_REGIONS boxes and kinds; G = 0 (the default) clears.  POCS_E_ARG for G out of range, a null
 * pointer, a value that is not finite, a half extent <= 0 or a kind other than 0 or 1, and the table in force stays.  The regions
 * belong to the context: they survive pocs_set_plans and pocs_set_footprint (which re-prepares the TOUCH regions).  Like every
 * setter it ends run-ahead serving.  The text channel has no command for it.  pocs_get_regions writes and returns G.
 *
 * Where the regions are APPLIED: whole calls on one GPU -- pocs_run_gmm_estimation, pocs_run_simulation (pocs_mc_run_local) -- as
 * single runs, batches in both sub-batch forms, run-ahead, calls of plans with and without the risk bounds, over static worlds of up
 * to 64 boxes and obstacle schedules.  A GMM call of one run then takes the ticket form (POCS_OPT_LONE_CALL has no effect, as under
 * clearance levels), an MC call the per-step form whatever POCS_OPT_MC_FUSED says (as under the MC risk bound).  NOT applied --
 * never refused: a tree of plans, a large world, POCS_OPT_OBSTACLE_COUNTS = 1, a shard (with it a bound moments buffer and the
 * exchange), the step API, a compound footprint (F > 1) and clearance levels with L > 0 (the levels keep applying): there the call
 * is launch for launch and bit for bit the call it is with G = 0, and the two getters below answer POCS_E_STATE.
 *
 * pocs_get_region_counts serves the selected run (pocs_select_batch_run; plan p while plans are set; the run served last under
 * run-ahead): writes the table, E x G row-major, sets *regions = G and returns E, the waypoints covered -- a plan's own length, or
 * the waypoints before its stop under a risk bound (GMM, or MC with POCS_OPT_MC_RISK_BOUND).
 *   GMM  G[w][g] = the samples drawn at waypoint w whose collision flag is 0 and which are in region g: G[w][g] <= the waypoint's
 *        collision-free samples.  The unused twin of an odd shard's last pair does not count.
 *   MC   G[w][g] = the particles that have collided at no waypoint <= w and are in region g at w.
 * POCS_E_BUFFER for cap < E * G, POCS_E_ARG for null pointers, POCS_E_STATE -- the message says which -- when there was no call, G
 * was 0, a setter touched the regions since, or the last call is one the regions are not applied to.
 * pocs_get_batch_region_probabilities(region, waypoint): per run / plan of the last call, in run / plan order (after a run-ahead
 * batch: the run served last); waypoint -1 means each plan's own last waypoint.  Formed on the host:
 *   GMM  (prod_{v < w} (1 - p_v)) * (G[w][region] / N): p_v as the final probability's p_v is formed, the product in waypoint order
 *        from 1.0, the quotient one IEEE division.  NOTE what this number is: the estimator's independence product for "free up to
 *        w", times the share of waypoint w's samples that are free and in the region -- samples drawn from the belief truncated by
 *        the collisions before w;
 *   MC   G[w][region] / N, one IEEE division: exactly the cloud's joint share "never collided and in the region at w";
 *   -1.0 for a waypoint the run / plan was not evaluated at: behind a stop, or w >= W_p. */
#define POCS_MAX_REGIONS 4
#define POCS_REGION_TOUCH 0
#define POCS_REGION_POINT 1
int pocs_set_regions(pocs_ctx* ctx, const double* boxes, const int* kinds, int G);
int pocs_get_regions(const pocs_ctx* ctx, double* boxes, int* kinds, int cap);     /* writes and returns G */
int pocs_get_region_counts(pocs_ctx* ctx, unsigned long long* out, int cap, int* regions);
int pocs_get_batch_region_probabilities(pocs_ctx* ctx, int region, int waypoint, double* out, int cap);

/* ---- segment checks: collisions between waypoints, for both estimators (ours) ---------------------
 * Both estimators test poses at waypoints only: a particle or sample that is free at waypoint w and free at w + 1 counts as safe,
 * whatever stands between the two.  For a plan whose waypoints lie a robot length or more apart (RRT edges, lattice primitives)
 * that is a risk that is too low.  With J >= 2 checks per segment (at most POCS_MAX_SEGMENT_CHECKS):
 *   fraction   f_j = (double)j / (double)J, one IEEE division;
 *   sub-pose   an output of the motion model as it is (pocs_motion, csrc/pocs_model.h, its angle wrap included) on a control whose
 *              third entry is 0.0;
 *   touches    a pose "touches" at a waypoint when the pose itself or one of J - 1 sub-poses on the way into that waypoint touches
 *              (pocs_pose_collides, touching included).  Every result of both estimators is formed from that flag.
 * J = 1 (the default) is every call as it has always been, bit for bit and launch for launch.
 *   MC   a particle with pose p at waypoint s is driven by the step's noisy control u (the one the particle moves with):
 *        q_j = pocs_motion(p, {u[0], f_j * u[1], 0.0}) for 1 <= j <= J - 1, one IEEE multiplication.  The particle touches at
 *        waypoint s + 1 when its end pose (unchanged) or any q_j touches the world of waypoint s + 1 (world min(s + 1, S - 1) under a
 *        schedule).  Waypoint 0 is the initial cloud alone.  The hit counters (+1 per waypoint at which the particle touches), the
 *        first-collision profile, the counts and the MC risk bound are what they are, formed from that flag.
 *   GMM  a sample p drawn at waypoint w >= 1 has no history: its way in is restated backwards with u = the applied control of step
 *        w - 1 (the control the EKF carried the mixture with): q_j = pocs_motion(p, {-u[2], -(f_{J-j} * u[1]), 0.0}).  The sample's
 *        flag is: its own pose or any q_j touches the world of waypoint w.  The truncation, nFree / nColl, the moment sums, the
 *        per-waypoint and final probabilities, the risk bound and the stored flags follow from that flag.
 *        NOTE what this number is: the estimator with "collides on the way into w" in place of "collides at w".  The way in is
 *        approximated by the nominal control applied backwards from the sample: it is not a propagated sample path.
 * Segment counts B[w], how many collisions were found only BETWEEN waypoints -- a planner reads from them that its waypoint spacing
 * is too coarse for the world:
 *   GMM  the samples of waypoint w whose own pose is free and some sub-pose touches (the odd shard's unused twin does not count):
 *        B[w] <= the collisions at w;
 *   MC   the particles whose first touching waypoint is w and whose end pose at w is free: B[w] <= F[w]
 *        (pocs_mc_get_waypoint_counts);
 *   B[0] = 0 always.
 * pocs_set_segment_checks takes 1 <= J <= POCS_MAX_SEGMENT_CHECKS; anything else is POCS_E_ARG and the value in force stays.  Like
 * every setter it ends run-ahead serving.  J belongs to the context: it survives pocs_set_plans and pocs_set_footprint.  The text
 * channel has no command for it.  pocs_get_segment_checks returns the value in force.
 *
 * SERVED (J > 1), as a compound footprint is: whole calls on one GPU -- pocs_run_gmm_estimation, pocs_run_simulation,
 * pocs_mc_run_local -- as single runs, batches in both sub-batch forms, run-ahead, calls of plans with and without both risk bounds
 * (each plan on its own chain and clock), POCS_OPT_MC_WAYPOINT_COUNTS, POCS_OPT_STORE_SAMPLES (stored flags are the segment flags), over
 * static worlds of up to 64 boxes and obstacle schedules.  A GMM call of one run takes the ticket form (POCS_OPT_LONE_CALL has no
 * effect), an MC call the per-step form whatever POCS_OPT_MC_FUSED says, and counts as under POCS_OPT_MC_WAYPOINT_COUNTS.  J and the
 * fractions live in device memory and the controls in the runs' chain records: another J > 1 replays the cached graph.
 * REFUSED in both directions with POCS_E_STATE (POCS_E_ORDER for the setter inside a begin/end sequence), the context left as it
 * was -- segment checks change results: a tree of plans, a large world (more than 64 boxes), a shard, the exchange (created or
 * connected), a bound moments buffer, an open begin/end sequence and pocs_gmm_begin, POCS_OPT_OBSTACLE_COUNTS = 1, a compound
 * footprint with F > 1.  pocs_set_segment_checks(J > 1) under any of these names what is in the way; entering any of them while
 * J > 1 names the call and "segment checks are set (pocs_set_segment_checks)".
 * NOT applied while J > 1, never refused: clearance levels and watched regions, as under a compound footprint -- their getters
 * answer POCS_E_STATE and the call is the J > 1 call without them.
 *
 * pocs_get_segment_counts serves the selected run (pocs_select_batch_run; plan p while plans are set; the run served last under
 * run-ahead): writes B[0 .. E) and returns E, the waypoints evaluated -- a plan's own length, or the waypoints before its stop under
 * a risk bound.  POCS_E_BUFFER for cap < E, POCS_E_ARG for a null pointer, POCS_E_STATE -- the message says which -- when there was
 * no call, J was 1, the setter was touched since, or the last call is not a served shape. */
#define POCS_MAX_SEGMENT_CHECKS 8
int pocs_set_segment_checks(pocs_ctx* ctx, int J);
int pocs_get_segment_checks(const pocs_ctx* ctx);
int pocs_get_segment_counts(pocs_ctx* ctx, unsigned long long* out, int cap);

/* ---- round obstacles: discs beside the boxes, for both estimators (ours) ----------------------------
 * What moves in a mobile robot's world -- people, other robots -- reaches a planner as a centre and a radius per time step, and
 * pillars, table legs and lidar returns are the same shape.  A disc is {cx, cy, r}, r > 0, all finite.
 *   world     the collision world at waypoint w is the boxes in force at w together with the discs in force at w;
 *   touches   a pose touches when it touches a box, as ever, or a disc: with the footprint's centre (px, py), heading (sn, cs) and half
 *             extents (rx, ry) as the box test forms them, d = (cx - px, cy - py) turned into the footprint's frame (the box test's own
 *             d1, d2), q_i = max(|d_i| - r_i, 0), the pose touches the disc exactly when NOT fma(q1, q1, q2 q2) > r r -- the exact
 *             distance from the disc's centre to the footprint, touching included (csrc/pocs_collide.h: pocs_disc_narrow).
 * Every result of both estimators is formed from that flag.
 *   schedule  S tables of D discs, table min(w, S - 1) in force at waypoint w -- independent of the boxes' own schedule: a static room
 *             with moving pedestrians is pocs_set_obstacles plus pocs_set_discs(.., D, W);
 *   bound     boxes and discs share the table of POCS_MAX_OBSTACLES records: M + D <= 64.  pocs_set_discs, pocs_set_obstacles and
 *             pocs_set_obstacle_schedule refuse a combination above it with POCS_E_ARG and leave the context as it was.  The discs lie
 *             behind the boxes: the caller's box indices do not move.
 * pocs_set_discs: discs = S x D x {cx, cy, r}, 1 <= S <= POCS_MAX_WORLD_STEPS.  D = 0, or S = 0 with a null pointer, clears: every call is
 * again, launch for launch, what it is without discs.  POCS_E_ARG, the discs in force kept: a null pointer with D > 0, D or S out of
 * range, a value that is not finite, r <= 0.  Like every setter it ends run-ahead serving.  The discs belong to the context: they survive
 * pocs_set_plans, pocs_set_footprint (the records are re-prepared), pocs_set_obstacles and pocs_set_obstacle_schedule (re-composed).  A
 * context given discs and never boxes has a world (M = 0) and may run.  pocs_get_discs writes D and S (0 and 0 without discs);
 * pocs_get_world_steps answers max(Sb, Sd).  The text channel has no command for discs; its clearObstacles leaves them.
 * Discs of the same D and S with other numbers are overwritten in place and the cached graph is replayed (pocs_get_graph_captures does
 * not move): the planning cycle, where new predictions arrive with every call.
 *
 * SERVED (D > 0), as a compound footprint is: whole calls on one GPU -- pocs_run_gmm_estimation, pocs_run_simulation, pocs_mc_run_local
 * -- over at most 64 records, static or scheduled, as single runs, batches in both sub-batch forms, run-ahead, calls of plans with and
 * without both risk bounds, POCS_OPT_MC_WAYPOINT_COUNTS, POCS_OPT_STORE_SAMPLES (stored flags are the world's flags).  A GMM call of one
 * run takes the ticket form (POCS_OPT_LONE_CALL has no effect), an MC call the per-step form whatever POCS_OPT_MC_FUSED says.
 * REFUSED in both directions with POCS_E_STATE (POCS_E_ORDER for the setter inside a begin/end sequence), the context left as it was --
 * discs change results: a tree of plans, a large world (more than 64 boxes), a shard, the exchange (created or connected), a bound
 * moments buffer, an open begin/end sequence and pocs_gmm_begin, POCS_OPT_OBSTACLE_COUNTS = 1, a compound footprint with F > 1, segment
 * checks with J > 1.  pocs_set_discs under any of these names what is in the way; entering any of them while D > 0 names the call and
 * "discs are set (pocs_set_discs)".  pocs_probe_device_collide, which tests boxes, answers POCS_E_STATE while D > 0.
 * NOT applied while D > 0, never refused: clearance levels and watched regions -- their getters answer POCS_E_STATE and the call is the
 * call with discs and without them. */
int pocs_set_discs(pocs_ctx* ctx, const double* discs /* S x D x {cx, cy, r} */, int D, int S);
int pocs_get_discs(const pocs_ctx* ctx, int* D, int* S);

/* ---- uncertain discs: a position covariance per disc and step, for both estimators (ours) -----------
 * A disc's centre is a prediction: a pedestrian two seconds ahead is known to decimetres.  For every disc d and disc step s the caller
 * may give a position covariance {sxx, sxy, syy} (m^2); table min(w, Sd - 1) is in force at waypoint w, like the discs' own.
 *   factor    the host factorises a row as the initial covariance is factorised, in double arithmetic and this order:
 *             l00 = sqrt(sxx), l10 = sxy / l00, l11 = sqrt(syy - l10 l10).  A row of three zeros is a certain disc: it draws nothing.
 *   draw      a pose is one possible world.  For pose index i (the global sample index of a GMM call, the global particle index
 *             first + i of an MC call), the run's effective seed, disc index d in the caller's table and waypoint word v:
 *             words = Philox4x32-7(ctr = (lo32(i >> 1), hi32(i >> 1), v, 5 << 16 | d), key = seed) -- stream 5 --, h = i & 1,
 *             (z0, z1) = the table-form Box-Muller pair of (words[2 h], words[2 h + 1]); |z| < 6.661.
 *   displace  cx' = fma(l00, z0, cx), cy' = fma(l11, z1, fma(l10, z0, cy)).
 *   word      GMM calls: v = w, a fresh deviation per waypoint, as the samples themselves are fresh.  The GMM estimator carries only the
 *             robot's mixture across waypoints, so it treats the deviations as INDEPENDENT IN TIME; against a persistent truth that errs
 *             to the high side.  MC calls: persistent = POCS_DISC_NOISE_PERSISTENT gives v = 0, a particle's world keeps its deviation z,
 *             the obstacle's track is c_s + L_s z and a covariance that grows with s is a prediction that fans out;
 *             POCS_DISC_NOISE_PER_WAYPOINT gives v = w.  Under plans every plan runs on its own clock from 0, as everywhere.
 *   flag      broad phase AND narrow phase, as for every record: the broad phase on the NOMINAL centre with the record's fields 6 and 7
 *             grown by 6.67 |l00| and 6.67 (|l10| + |l11|) (conservative: |z| < 6.661), the narrow phase the disc test above on
 *             (cx', cy').  A certain disc, a box and every call without covariances are what they are without this; a pose touches
 *             the world when it touches a box or a disc, certain or displaced, and every result is formed from that flag.
 * pocs_set_disc_covariances: cov = S x D x {sxx, sxy, syy}; D and S must equal those of the discs in force (POCS_E_ARG otherwise;
 * POCS_E_STATE without discs).  A null pointer with D = 0 clears; all rows zero is the same as cleared: every call is then, launch for
 * launch, the discs call it is without this.  POCS_E_ARG, what was in force kept: a value that is not finite, a row that is neither
 * zeros nor has sxx > 0 and syy - l10 l10 > 0, a persistent other than 0 or 1.  POCS_E_ORDER inside a begin/end sequence.  Like every
 * setter it ends run-ahead serving.  pocs_set_discs with the same D and S keeps the covariances; another D or S, or clearing, drops
 * them.  They survive pocs_set_footprint, pocs_set_obstacles, pocs_set_obstacle_schedule and pocs_set_plans (re-composed).  Covariances
 * of the same shape with other numbers are overwritten in place and the cached graph is replayed (pocs_get_graph_captures does not
 * move): the planning cycle.  pocs_get_disc_covariances writes the table and the setting and returns S * D * 3 (0 when none,
 * POCS_E_BUFFER for a short buffer).
 * SERVED, REFUSED and NOT applied: exactly what discs serve, refuse and do not apply (the block above); covariances need discs, so
 * there is no refusal of their own. */
#define POCS_DISC_NOISE_PER_WAYPOINT 0
#define POCS_DISC_NOISE_PERSISTENT   1
int pocs_set_disc_covariances(pocs_ctx* ctx, const double* cov /* S x D x {sxx, sxy, syy} */, int D, int S, int persistent);
int pocs_get_disc_covariances(const pocs_ctx* ctx, double* out, int cap, int* persistent);   /* returns S*D*3, 0 when none */

/* ---- prediction hypotheses: weighted alternative tracks per round obstacle, for both estimators (ours) ----------
 * A trajectory predictor hands over a few alternatives with probabilities: "crosses in front of the robot, 0.3; waits at the kerb,
 * 0.7".  Every disc in force may be one ALTERNATIVE of a group; the disc schedule gives each alternative its track, the covariances
 * its spread, and this table its weight.  Hypotheses are per disc, not per disc step: an alternative is a whole track.
 *   groups      group[d] = -1: disc d is always there, and its weight is not read.  group[d] = g, 0 <= g < D: disc d is one alternative
 *               of group g.  The alternatives of a group exclude each other: for one pose at most one of them exists.  A group whose
 *               weights sum to less than 1 leaves room for "none of them"; a group of one alternative with weight p is an obstacle
 *               that exists with probability p (a door that may be open, a detection of low confidence).
 *   thresholds  exact integers, formed on the host in this order: n_d = floor(weight[d] * 4294967296.0) (the product is exact); within
 *               a group, in ascending d, lo_d = the sum of n_e over the earlier discs e < d of the same group, hi_d = lo_d + n_d.  The
 *               getter returns lo and hi: the probability of an alternative is exactly n_d / 2^32.  (group -1: lo = 0, hi = 2^32.)
 *   draw        a pose is one possible world.  For pose index i (the global sample index of a GMM call, the global particle index
 *               first + i of an MC call), the run's effective seed, group g and waypoint word v:
 *               words = Philox4x32-7(ctr = (lo32(i >> 1), hi32(i >> 1), v, 6 << 16 | g), key = seed) -- stream 6 --, h = i & 1,
 *               u = words[2 h].  Disc d exists for the pose iff lo_d <= u < hi_d: an integer compare, nothing is floating point.
 *   word        GMM calls: v = w, a fresh choice per waypoint.  The GMM estimator carries only the robot's mixture across waypoints,
 *               so it treats the choices as INDEPENDENT IN TIME, the approximation the covariances make; against a persistent truth it
 *               errs to the high side in the same way.  MC calls: v = 0 always -- a particle's world keeps its alternative for the
 *               whole roll-out, which is what a hypothesis means; there is no per-waypoint setting.  Plans run on their own clocks.
 *   flag        a gated disc record touches a pose iff the disc exists for the pose AND the record's test as it is without this says
 *               so (the broad phase on the nominal centre with the grown fields, the narrow phase, on the displaced centre for an
 *               uncertain disc).  Everything both estimators report is formed from the flag.  The deviation draw (stream 5) and the
 *               existence draw (stream 6) are independent.
 * pocs_set_disc_hypotheses: POCS_E_ARG, what was in force kept: D other than the D of the discs in force, a group outside [-1, D), a
 * weight that is not finite or outside (0, 1], n_d = 0, a group whose last hi exceeds 2^32, a null pointer with D > 0.  POCS_E_STATE
 * without discs; POCS_E_ORDER inside a begin/end sequence.  A null pointer with D = 0 clears, and so does a table whose groups are all
 * -1: every call is then, launch for launch, the call it is without this.  pocs_set_discs with the same D keeps the hypotheses,
 * whatever S is; another D, or clearing the discs, drops them.  They survive pocs_set_footprint, pocs_set_obstacles,
 * pocs_set_obstacle_schedule, pocs_set_plans and pocs_set_disc_covariances.  Hypotheses of the same D with other numbers are
 * overwritten in place and the cached graph is replayed (pocs_get_graph_captures does not move): the planning cycle, where new weights
 * arrive with every prediction.  pocs_get_disc_hypotheses writes up to cap entries of each array that is not null and returns D (0
 * when none, POCS_E_BUFFER for cap < D).
 * SERVED, REFUSED and NOT applied: exactly what discs serve, refuse and do not apply; hypotheses need discs.  One refusal of their
 * own, in both directions with POCS_E_STATE: a round footprint (pocs_set_footprint_disc). */
int pocs_set_disc_hypotheses(pocs_ctx* ctx, const int* group /* D */, const double* weight /* D */, int D);
int pocs_get_disc_hypotheses(const pocs_ctx* ctx, int* group, double* weight, unsigned long long* lo, unsigned long long* hi, int cap);   /* returns D, 0 when none */

/* ---- a round footprint: a disc of radius rho centred on the pose, for both estimators (ours) -----------
 * Most mobile bases are round.  Handed over as its bounding square such a robot is 27 % too large in area, and collisions are decided
 * at corners it does not have.  pocs_set_footprint_disc makes the footprint the disc of radius rho (finite, >= 0; 0 is a point robot,
 * for planners that inflate the obstacles themselves) centred on (x, y) of the pose.  The heading is never read by the collision test.
 *   records   boxes and discs are prepared as under pocs_set_discs, with ONE difference: the footprint's bounding radius in a record's
 *             fields 6 and 7 is rho, not the square's sqrt(hx^2 + hy^2).  An uncertain disc's growth is added exactly as before.
 *   flag      broad phase AND narrow phase, touching included.  dx = cx - x, dy = cy - y; |dx| > field 6 or |dy| > field 7: no.
 *             box:  e1 = fma(dx, ax, dy ay), e2 = fma(dy, ax, -(dx ay)), q_i = fmax(|e_i| - h_i, 0), touches = !(fma(q1, q1, q2 q2) > rho rho).
 *             disc: R = r + rho, touches = !(fma(dx, dx, dy dy) > R R); an uncertain disc: the broad phase on the nominal centre, this test
 *             on the displaced centre (stream 5, the keys, the waypoint word and persistence as above).
 *             A pose touches the world when it touches any record; every result of both estimators is formed from that flag.
 * REPLACEMENT: a footprint setter replaces the footprint.  pocs_set_footprint, the text channel's setFootprint and
 * pocs_set_footprint_parts return to boxes; pocs_set_footprint_disc replaces a single box and a compound footprint alike.  While the
 * disc is in force pocs_get_footprint_parts reports one part, the bounding square {0, 0, rho, rho}; pocs_get_footprint_disc returns 1
 * and writes rho (0, nothing written, under a box footprint).  POCS_E_ARG for a radius that is not finite or negative, the footprint
 * in force kept.  Like every setter it ends run-ahead serving.  Obstacles, schedules, discs and covariances set afterwards are prepared
 * for rho.
 * SERVED: whole calls on one GPU, GMM and MC -- single runs, batches in both sub-batch forms, run-ahead, plans with and without both
 * risk bounds, POCS_OPT_MC_WAYPOINT_COUNTS, stored samples -- over static worlds of up to 64 records, obstacle schedules, discs with
 * their own schedule and disc covariances, persistent and per waypoint.  MC calls take the per-step form whatever POCS_OPT_MC_FUSED says.
 * REFUSED in both directions (POCS_E_STATE; the setter inside a begin/end sequence: POCS_E_ORDER; the context is left as it was): a
 * tree of plans, a large world, a shard, the exchange created or connected, bound moments, an open sequence and pocs_gmm_begin,
 * POCS_OPT_OBSTACLE_COUNTS = 1, segment checks with J > 1, pocs_probe_device_collide.
 * NOT applied, never refused: clearance levels and watched regions (their getters answer POCS_E_STATE, "not applied"); they apply
 * again, bit for bit, once a box footprint is back. */
int pocs_set_footprint_disc(pocs_ctx* ctx, double radius);
int pocs_get_footprint_disc(const pocs_ctx* ctx, double* radius);   /* 1 and *radius = rho while in force, else 0 */

/* ---- results of the last run, for audits and parity tests ------------------------------- */
int pocs_get_path_length(const pocs_ctx* ctx);
int pocs_get_waypoint_probabilities(pocs_ctx* ctx, double* out, int cap);         /* `probabilities`, MCSimulator.h:660,678,817 */
int pocs_get_moments(pocs_ctx* ctx, int waypoint, double* out, int cap);          /* K x 11: nFree nColl Sx Sy St Sxx Sxy Sxt Syy Syt Stt */
int pocs_get_gmm_state(pocs_ctx* ctx, int waypoint, double* means3, double* covs9, double* weights, double* alive);  /* the mixture sampled at `waypoint`; alive[k] = 0 for a retired component */
int pocs_get_host_chain(pocs_ctx* ctx, double* applied3, double* noisy3, double* z, double* mu3, double* cov9); /* per step i<W-1; z is L per step */
long long pocs_copy_gmm_samples(pocs_ctx* ctx, double* xyt_aos, int16_t* flags, long long cap);  /* last waypoint's shard, 3 x n column-major like arma (x,y,theta triples) */
long long pocs_copy_particles(pocs_ctx* ctx, double* xyt_aos, uint32_t* hits, long long cap);   /* mcparticles / particlecollisions, MCSimulator.h:105,108 */
int pocs_measure_copy_bandwidth(pocs_ctx* ctx, long long bytes, double* gbps);  /* read+write GB/s of a plain streaming copy on this GPU: the measured HBM ceiling */
int pocs_measure_fill_bandwidth(pocs_ctx* ctx, long long bytes, double* gbps);  /* written GB/s of a plain streaming fill: the write-only ceiling (the GMM kernels read nothing) */
int pocs_get_kernel_time(pocs_ctx* ctx, double* total_ms, long long* launches);  /* hot-kernel time of the last run with POCS_OPT_PROFILE=1 (of the launches on the context's stream) */
int pocs_get_graph_captures(pocs_ctx* ctx, long long* gmm, long long* mc);  /* how often the launches of the whole GMM call and of the MC call have been captured into a
                                                                               hipGraph since the context was created (either may be null).  A call replays the cached graph
                                                                               while its launches -- kernels, grids, streams, argument bytes -- are the captured ones: setters
                                                                               that change none of them (a seed, a plan of the same length, obstacles of the same count) add nothing */
int pocs_get_exchange_wait(pocs_ctx* ctx, double* min_median_max_us);  /* sharded GMM calls through the library's own exchange (pocs_gmm_exchange_local /
                                                                          pocs_gmm_sample_exchange_local): how long the closers of the last begin..end sequence
                                                                          waited for the other ranks' moments, over its (run, waypoint) pairs -- the first thing
                                                                          to read when a multi-GPU run scales badly (ranks that drift apart show here) */
int pocs_probe_device_math(pocs_ctx* ctx, int n, const uint32_t* radius_words, const uint32_t* angle_words, const double* headings,
                           double* z0, double* z1, double* sn, double* cs, double* radius2);
/* TEST HOOK, no counterpart in the reference: the DEVICE's table-driven sampler functions on inputs the
   caller picks -- per i < n the Box-Muller pair (z0, z1) of the words (radius_words[i], angle_words[i]) with its squared radius,
   and sin / cos of headings[i] as the footprint test evaluates them -- through the same inline functions, tables and pinned
   constants as k_gmm_step.  A free-running launch meets a given word once in 2^32 draws; this puts the edge words (0, the
   cells' boundaries, 2^32 - 1, a heading on a sector's tie) in front of the oracle directly (tests/test_gpu_parity.py). */
int pocs_probe_device_radius_roots(pocs_ctx* ctx, uint32_t first_word, unsigned long long count, unsigned long long* mismatches,
                                   uint32_t* first_bad);
/* TEST HOOK beside pocs_probe_device_math: the mixture sampler takes the square root of its Box-Muller radius with one residual
   correction less than the correctly rounded sequence has; the radius' argument takes one value per
   32-bit word, so the two are compared on the DEVICE word by word.  For the words first_word .. first_word + count - 1
   (count >= 1, first_word + count <= 2^32) the device forms the argument through the staged tables as the sampling kernel
   does and takes both roots; mismatches: the number of words whose two roots differ in any bit; first_bad: the smallest such
   word (0 where there is none).  Sixteen calls of 2^28 words cover every argument (tests/test_radius_root_sweep.py).  POCS_E_ARG
   for a null pointer or a range outside the words. */
int pocs_probe_device_collide(pocs_ctx* ctx, int K, const double* params, int n, const double* poses_xyt, int* flag_full, int* flag_pair,
                              int* flag_pair_eager, int* nkeep, double* kept);
/* TEST HOOK, no counterpart in the reference: the DEVICE's collision test and the obstacle cull of the GMM sampling kernel on
   inputs the caller picks, against the collision world and footprint the context holds (pocs_set_obstacles / pocs_set_footprint;
   nothing else need be configured; under an obstacle schedule: world 0).  params: the sampler parameters of a mixture of K components, K x 12 doubles (per component
   mean[3], L00 L10 L11 L20 L21 L22 of the lower Cholesky factor, three unused); poses_xyt: n poses (x, y, theta), 1 <= n <= 2^20.
   One block stages the world and the mixture as a block of the sampling kernel does and culls the obstacle table against the
   mixture; then per pose i
     flag_full[i]        the footprint test on the full table, as the MC kernels stage and call it,
     flag_pair[i]        the two-pose form on the culled table (poses 2 j and 2 j + 1 one pair; an odd last pose is paired with
                         itself and gets 2 added should its two slots disagree), as the batch form of the sampling kernel calls it,
     flag_pair_eager[i]  the same in the form the kernel takes for a call of one run;
   nkeep: the number of records the cull kept; kept: room for 64 x 8 doubles, the kept records in table order (centre, axis, half
   extents, and the broad phase sized to the mixture's headings), zeros behind them.  A pose the mixture cannot draw may lose
   its obstacle to the cull: flag_pair is the kernel's answer only for poses within the mixture's reach.  Puts the poses a
   free-running launch never draws -- a few ulps from touching, at the edge of the mixture's reach -- in front of the oracle
   (tests/test_collision_probe.py).  POCS_E_ARG for a null pointer, n or K out of range and ANY input that is not finite;
   POCS_E_STATE for a context without a collision world. */
int pocs_probe_device_clearance(pocs_ctx* ctx, const double* fp4, const double* d, int L, const double* boxes, int M,
                                int n, const double* poses_xyt, int* level_out);
/* TEST HOOK beside pocs_probe_device_collide: the DEVICE's clearance level of poses the caller picks, for the caller's own footprint
   fp4 = {dx, dy, half_x, half_y}, distances d[0 .. L) (0 <= L <= POCS_MAX_CLEARANCE_LEVELS, as pocs_set_clearance_levels takes them)
   and table of M <= 64 boxes {cx, cy, half_x, half_y, yaw_rad}, prepared as the library prepares the context's.  One small launch
   stages them; per pose i < n it writes the smallest l whose grown footprint touches: -1 for the footprint itself, L for none --
   through the inline functions the kernels use (the single-pose form of the MC kernels, and the two-pose lane-mask form of the GMM
   sampling kernel on poses 2 j, 2 j + 1: 100 is added should the two ever disagree).  It reads nothing of the context's world,
   plans or modes, so it is never refused.  POCS_E_ARG for a null pointer, n outside 1 .. 2^20, bad distances or boxes and ANY
   input that is not finite. */
int pocs_probe_device_footprint_parts(pocs_ctx* ctx, const double* parts, int F, const double* boxes, int M,
                                      int n, const double* poses_xyt, int* touched_out);
/* TEST HOOK beside pocs_probe_device_clearance, equally self-contained: which parts of the caller's own compound footprint (F parts
   as pocs_set_footprint_parts takes them, 1 <= F <= POCS_MAX_FOOTPRINT_PARTS) touch the caller's own table of M <= 64 boxes {cx, cy,
   half_x, half_y, yaw_rad}, prepared as the library prepares the context's.  One small launch stages them; per pose i < n
   touched_out[i] is a bit mask, bit f set when part f touches -- through the inline functions the kernels use (the single-pose form
   of the MC kernels, and the two-pose lane-mask form of the GMM sampling kernel on poses 2 j, 2 j + 1: bit 8 is set should the two
   ever disagree).  It reads nothing of the context's world or modes, so it is never refused.  POCS_E_ARG for a null pointer, n
   outside 1 .. 2^20, bad parts or boxes and ANY input that is not finite. */
int pocs_probe_device_regions(pocs_ctx* ctx, const double* fp4, const double* boxes, const int* kinds, int G,
                              int n, const double* poses_xyt, int* mask_out);
/* TEST HOOK beside pocs_probe_device_clearance: which watched regions the DEVICE finds poses of the caller's in, for the caller's own
   footprint fp4 = {dx, dy, half_x, half_y} and G <= POCS_MAX_REGIONS boxes and kinds (as pocs_set_regions takes them), prepared as the
   library prepares the context's.  One small launch stages them; per pose i < n bit g of mask_out[i] means "in region g" through the
   single-pose function of the MC kernels, and bit 8 + g is set should the two-pose lane-mask form ever disagree.  It reads nothing of
   the context's world, plans, modes or regions, so it is never refused.  POCS_E_ARG for a null pointer, n outside 1 .. 2^20, bad
   boxes or kinds and ANY input that is not finite. */
int pocs_probe_device_segment(pocs_ctx* ctx, const double* fp4, const double* boxes, int M, const double* u3, int J, int backward,
                              int n, const double* poses_xyt, int* mask_out);
/* TEST HOOK beside pocs_probe_device_footprint_parts, equally self-contained: which of the segment checks' sub-poses the DEVICE finds
   touching, for the caller's own footprint fp4 = {dx, dy, half_x, half_y}, table of M <= 64 boxes {cx, cy, half_x, half_y, yaw_rad},
   control u3 and 1 <= J <= POCS_MAX_SEGMENT_CHECKS, prepared as the library prepares the context's.  backward 0 is the MC form: pose
   i is a particle at the segment's start, driven by u3 as a noisy control; backward 1 is the GMM form: pose i is a sample at the
   segment's end, u3 the applied control.  One small launch stages them; bit j of mask_out[i], 1 <= j <= J - 1, means sub-pose j
   touches, bit J that the end pose touches (the moved particle, or the sample itself) -- through the inline functions the kernels
   use (the single-pose form of the MC kernels, and the two-pose lane-mask form of the GMM sampling kernel on poses 2 j, 2 j + 1: bit
   16 is set should the two ever disagree).  It reads nothing of the context's world or modes, so it is never refused.  POCS_E_ARG for
   a null pointer, n outside 1 .. 2^20, J, M or backward out of range, a bad footprint or box and ANY input that is not finite. */
int pocs_probe_device_counts(pocs_ctx* ctx, int n, const int* K, const double* weights, const double* alive, const uint64_t* seeds,
                             const uint32_t* waypoints, const long long* n_total, double* counts_out);
/* TEST HOOK beside pocs_probe_device_math, equally self-contained: the DEVICE's component counts of a waypoint (DESIGN.md section 4,
   "degenerate cases") on inputs the caller picks.  n cases; case i is a mixture of K[i] components (1 <= K[i] <= 8): weights and
   alive are n rows of 8 doubles, of which case i reads the first K[i] -- the raw weights (survivor counts, or any finite numbers
   >= 0) and the alive flags (0 = retired) as the advance leaves them before it normalises; seeds[i] and waypoints[i] key the case's
   draws, and n_total[i] (1 .. 2^53: a count is exact in a double) is the number of samples its components share.  One small launch,
   one thread per case, divides the weights by their sum and draws the conditional binomials -- waiting times below
   n min(p, 1 - p) = 10, BTPE from there on -- through the inline functions the mixture advance calls on both of its paths (the
   speculated counts and their fallback); counts_out is n rows of 8, row i the CUMULATIVE counts n_0, n_0 + n_1, ... of case i (the
   last live component's entry is n_total[i]; all retired: component 0 gets everything), zeros behind its K[i].  A free-running call
   meets only the (n, p, seed) its own mixtures produce; this puts the switch between the two samplers, weights next to 0 and 1 and
   retired components in every position in front of the oracle (tests/test_degenerate_forms.py).  It reads nothing of the context's
   world, plans or modes, so it is never refused.  POCS_E_ARG for a null pointer, n outside 1 .. 2^20, a K or n_total out of range,
   a negative weight and ANY input that is not finite. */
int pocs_probe_device_discs(pocs_ctx* ctx, const double* fp4, const double* boxes, int M, const double* discs, int D,
                            int n, const double* poses_xyt, int* out);
/* TEST HOOK beside pocs_probe_device_segment, equally self-contained: which kinds of obstacle the DEVICE finds a pose touching, for the
   caller's own footprint fp4 = {dx, dy, half_x, half_y}, M boxes {cx, cy, half_x, half_y, yaw_rad} and D discs {cx, cy, r}, M + D <= 64,
   prepared and composed as the library prepares the context's.  One small launch stages them; out[i] bit 0: pose i touches some box,
   bit 1: some disc -- through the MC kernels' single-pose form on the full table --, bit 8 should the sampling kernel's two-pose
   lane-mask form (poses 2 j, 2 j + 1) ever disagree.  It reads nothing of the context's world or modes, so it is never refused.
   POCS_E_ARG for a null pointer, n outside 1 .. 2^20, M + D out of range, a bad footprint, box or disc and ANY input that is not finite. */
int pocs_probe_device_disc_noise(pocs_ctx* ctx, const double* fp4, const double* discs /* D x 3 */, const double* cov /* D x 3 */, int D,
                                 uint64_t seed, uint32_t waypoint_word, unsigned long long first /* even */, int n /* even */,
                                 const double* poses_xyt, double* centres_out /* n x D x 2 */, unsigned* flags_out /* n */);
/* TEST HOOK beside pocs_probe_device_discs, equally self-contained: uncertain discs on the DEVICE for the caller's own footprint, D <= 16
   discs {cx, cy, r} and covariances {sxx, sxy, syy} (zeros: a certain disc), prepared as the library prepares the context's.  Pose i has
   index first + i, the seed and the waypoint word are the caller's.  centres_out: the device's displaced centres; bit d of flags_out[i]:
   pose i touches displaced disc d -- through the MC kernels' single-pose form --, bit 31 should the sampling kernel's two-pose lane-mask
   form (poses 2 j, 2 j + 1) ever disagree.  Never refused.  POCS_E_ARG for a null pointer, D outside 1 .. 16, n outside 2 .. 2^20 or odd,
   an odd first, a bad footprint, disc or covariance and ANY input that is not finite. */
int pocs_probe_device_disc_hypotheses(pocs_ctx* ctx, const double* fp4, const double* discs /* D x 3 */, const double* cov /* D x 3, may be null */,
                                      const int* group /* D */, const double* weight /* D */, int D, uint64_t seed, uint32_t waypoint_word,
                                      unsigned long long first /* even */, int n /* even */, const double* poses_xyt,
                                      unsigned* exists_out /* n */, unsigned* flags_out /* n */);
/* TEST HOOK beside pocs_probe_device_disc_noise, equally self-contained: prediction hypotheses on the DEVICE for the caller's own
   footprint, D <= 32 discs, covariances (null: none) and hypotheses, prepared as the library prepares the context's.  Pose i has index
   first + i; the seed is the caller's and the waypoint word serves deviations and existence draws alike.  Bit d of exists_out[i]: disc d
   exists for pose i; bit d of flags_out[i]: pose i touches disc d -- through the MC kernels' single-pose form.  Should the sampling
   kernel's two-pose lane-mask form (poses 2 j, 2 j + 1) ever disagree, the pose's exists is 0 and its flags are all ones.  Never
   refused.  POCS_E_ARG for a null pointer but cov, D outside 1 .. 32, n outside 2 .. 2^20 or odd, an odd first, a bad footprint, disc,
   covariance or hypothesis table and ANY input that is not finite. */
int pocs_probe_device_footprint_disc(pocs_ctx* ctx, double radius, const double* boxes /* M x 5 */, int M, const double* discs /* D x 3 */, int D,
                                     const double* cov /* NULL or D x 3 */, uint64_t seed, uint32_t waypoint_word, unsigned long long first /* even */,
                                     int n, const double* poses_xyt, int* out /* n */);
/* TEST HOOK beside pocs_probe_device_discs, equally self-contained: the ROUND footprint's test on the DEVICE for the caller's own radius,
   M boxes and D discs (M + D <= 64) and, where cov is given, the discs' covariances {sxx, sxy, syy} (zeros: a certain disc), prepared as
   the library prepares the context's.  Pose i has index first + i; the seed and the waypoint word are the caller's (read under cov
   only).  out[i] bit 0: pose i touches some box, bit 1: some disc, displaced where cov says so -- both through the MC kernels'
   single-pose form on the full table --, bit 8 should the sampling kernel's two-pose lane-mask form (poses 2 j, 2 j + 1) ever disagree.
   It reads nothing of the context's world or modes, so it is never refused.  POCS_E_ARG for a null pointer, n outside 1 .. 2^20, M + D
   out of range, an odd first, a bad radius, box, disc or covariance and ANY input that is not finite. */
int pocs_get_sequence_time(pocs_ctx* ctx, double* ms, int* concurrent);  /* POCS_OPT_PROFILE=1, whole-run GMM calls: first sampling launch -> end of the last one, and how many
                                                                            sub-batches of the call were in flight side by side (their launches overlap: DESIGN.md section 5) */

#ifdef __cplusplus
}
#endif
#endif /* POCS_H */

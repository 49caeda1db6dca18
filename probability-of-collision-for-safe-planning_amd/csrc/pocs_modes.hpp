// pocs_modes.hpp -- what combines with what: the modes a context can be in and the ONE table of the pairs that exclude each
// other, host only (no HIP type, no context: tests/mode_table_demo.cpp prints it under g++).  Every setter, pocs_gmm_begin and the
// probe ask may_enter (pocs_ctx.hpp), which reads the context's mode word (modes_of) and this table; DESIGN.md section 9 has the
// matrix written out.
#pragma once
#include "../../include/pocs.h"

namespace pocs_modes {

enum Mode : unsigned {
  kPlans = 1u << 0,           // pocs_set_plans with P > 0
  kTree = 1u << 1,            // pocs_set_plan_tree with nodes > 0
  kShard = 1u << 2,           // pocs_set_shard with a range
  kXchgCreated = 1u << 3,     // pocs_xchg_create
  kXchgConnected = 1u << 4,   // pocs_xchg_connect
  kMoments = 1u << 5,         // pocs_gmm_bind_moments with a buffer
  kLargeWorld = 1u << 6,      // pocs_set_world with more than POCS_MAX_OBSTACLES boxes
  kObsCounts = 1u << 7,       // POCS_OPT_OBSTACLE_COUNTS = 1
  kFused = 1u << 8,           // POCS_OPT_MC_FUSED = 1
  kSequence = 1u << 9,        // pocs_gmm_begin ... pocs_gmm_end
  // Asks: calls that enter none of the modes above and are still refused under some of them.  Never part of a mode word.
  kSinglePlan = 1u << 10,     // pocs_set_path_length / _trajectory / _odometry / _batch: the single plan and its batch
  kBatch = 1u << 11,          // pocs_set_batch
  kRiskBound = 1u << 12,      // pocs_set_plan_risk_bound
  kSelectRun = 1u << 13,      // pocs_select_batch_run
  kProbe = 1u << 14,          // pocs_probe_device_collide
  kAddObstacle = 1u << 15,    // the text channel's addObstacle
  kAll = ~0u
};
constexpr int kNumModes = 10, kNumAsks = 6;

// A mode as a refusal names it -- what is in the way --, by bit; an ask is never in the way, its name serves the printed table.
static const char* const kNames[kNumModes + kNumAsks] = {
    "plans are set", "a tree of plans is set", "a shard is set", "the context has a buffer of the in-library exchange",
    "the context is connected to the in-library exchange", "a caller-owned moments buffer is bound (the step API)",
    "a large world is in force (pocs_set_world)", "POCS_OPT_OBSTACLE_COUNTS is on", "POCS_OPT_MC_FUSED is on",
    "a begin/end sequence is open", "single plan", "batch", "risk bound", "select run", "probe", "addObstacle"};
inline const char* name(Mode m) { return kNames[__builtin_ctz(m)]; }

// One row per excluding pair: the code when `a` is entered under `b`, the code when `b` is entered under `a` (POCS_OK: that
// direction is served -- plans may be set on a context that has only created its exchange buffer; an ask is never active), and
// the clause that explains it (%d: POCS_MAX_OBSTACLES).  The first matching row answers, so the ORDER of the rows is the order in
// which a call with two modes in its way names them.
struct Row { Mode a, b; int a_under_b, b_under_a; const char* clause; };

static const char* const kOneGpuPlans = "multi-GPU plan batches are not supported", * const kOneGpuTree = "trees run on one GPU";
static const char* const kAsBegun = "the sequence's launches are built from what pocs_gmm_begin saw";
static const char* const kStepSingle = "the step API serves a single plan, and its launches are built from what pocs_gmm_begin saw";

static const Row kRows[] = {
    {kPlans, kSequence, POCS_E_ORDER, POCS_E_STATE, kStepSingle},
    {kTree, kSequence, POCS_E_ORDER, POCS_E_STATE, kStepSingle},
    {kObsCounts, kSequence, POCS_E_ORDER, POCS_OK, kAsBegun},
    {kBatch, kSequence, POCS_E_ORDER, POCS_OK, kAsBegun},
    {kRiskBound, kSequence, POCS_E_ORDER, POCS_OK, kAsBegun},
    {kPlans, kTree, POCS_E_ORDER, POCS_E_ORDER, "plans and a tree exclude each other: clear with pocs_set_plans(ctx, 0, ...) / pocs_set_plan_tree(ctx, 0, ...) first"},
    {kSinglePlan, kPlans, POCS_E_ORDER, POCS_OK, "the plans hold the context's path and batch: clear them first with pocs_set_plans(ctx, 0, ...)"},
    {kSinglePlan, kTree, POCS_E_ORDER, POCS_OK, "the tree holds the context's path and batch: clear it first with pocs_set_plan_tree(ctx, 0, ...)"},
    {kSelectRun, kTree, POCS_E_ORDER, POCS_OK, "pocs_select_tree_node selects a node"},
    {kObsCounts, kLargeWorld, POCS_E_STATE, POCS_E_STATE, "the per-box counts serve worlds of at most %d boxes"},
    {kFused, kLargeWorld, POCS_E_STATE, POCS_E_STATE, "the fused roll-out serves worlds of at most %d boxes"},
    {kTree, kLargeWorld, POCS_E_STATE, POCS_E_STATE, "trees serve worlds of at most %d boxes"},
    {kPlans, kShard, POCS_E_STATE, POCS_E_STATE, kOneGpuPlans},
    {kTree, kShard, POCS_E_STATE, POCS_E_STATE, kOneGpuTree},
    {kShard, kLargeWorld, POCS_E_STATE, POCS_E_STATE, "sharded runs serve worlds of at most %d boxes"},
    {kPlans, kXchgCreated, POCS_OK, POCS_E_STATE, kOneGpuPlans},
    {kPlans, kXchgConnected, POCS_E_STATE, POCS_E_STATE, kOneGpuPlans},
    {kTree, kXchgCreated, POCS_OK, POCS_E_STATE, kOneGpuTree},
    {kTree, kXchgConnected, POCS_E_STATE, POCS_E_STATE, kOneGpuTree},
    {kXchgCreated, kLargeWorld, POCS_E_STATE, POCS_E_STATE, "the exchange serves worlds of at most %d boxes"},
    {kXchgConnected, kLargeWorld, POCS_E_STATE, POCS_E_STATE, "the exchange serves worlds of at most %d boxes"},
    {kMoments, kLargeWorld, POCS_E_STATE, POCS_E_STATE, "the step API serves worlds of at most %d boxes"},
    {kLargeWorld, kSequence, POCS_E_ORDER, POCS_E_STATE, "the step API serves worlds of at most %d boxes"},
    {kProbe, kLargeWorld, POCS_E_STATE, POCS_OK, "the probe stages worlds of at most %d boxes"},
    {kAddObstacle, kLargeWorld, POCS_E_ARG, POCS_OK, "the text channel serves worlds of at most %d boxes"},
};

// A compound footprint (pocs_set_footprint_parts with F > 1) is not a mode of the table: it changes results, so what it is not
// built for is refused in both directions -- entering any of these while it is set (may_enter asks in front of the table), and
// setting it under any of these (the setter asks) -- with POCS_E_STATE (the setter inside a begin/end sequence: POCS_E_ORDER).
constexpr unsigned kPartsExcluded = kTree | kShard | kXchgCreated | kXchgConnected | kMoments | kLargeWorld | kObsCounts | kSequence | kProbe;
static const char* const kPartsClause = "a compound footprint is served by whole calls on one GPU over worlds of at most 64 boxes, without per-box counts";

// Segment checks (pocs_set_segment_checks with J > 1) are no mode of the table either, for the same reason: they change results, so
// what they are not built for is refused in both directions, as under a compound footprint -- and a compound footprint itself, which
// is no bit of a mode word, is asked about beside this mask (seg_refuse, pocs_ctx.hpp; the two setters).
constexpr unsigned kSegExcluded = kTree | kShard | kXchgCreated | kXchgConnected | kMoments | kLargeWorld | kObsCounts | kSequence;
static const char* const kSegClause = "segment checks are served by whole calls on one GPU over worlds of at most 64 boxes, with a single footprint box and without per-box counts";

// Round obstacles (pocs_set_discs with D > 0) are no mode of the table either: they change results, so what they are not built for
// is refused in both directions -- and a compound footprint and segment checks, which are no bits of a mode word, are asked about
// beside this mask (discs_refuse, pocs_ctx.hpp; the three setters).
constexpr unsigned kDiscExcluded = kTree | kShard | kXchgCreated | kXchgConnected | kMoments | kLargeWorld | kObsCounts | kSequence;
static const char* const kDiscClause = "discs are served by whole calls on one GPU over worlds of at most 64 records, with a single footprint box, without per-box counts and segment checks";

// A round footprint (pocs_set_footprint_disc) is no mode of the table either, for the same reason: it changes results, so what it is
// not built for is refused in both directions -- and segment checks, which are no bit of a mode word, are asked about beside this mask
// (rfoot_refuse, pocs_ctx.hpp; the two setters).  A compound footprint needs no ask: a footprint setter replaces the footprint.
constexpr unsigned kRoundFpExcluded = kTree | kShard | kXchgCreated | kXchgConnected | kMoments | kLargeWorld | kObsCounts | kSequence | kProbe;
static const char* const kRoundFpClause = "a round footprint is served by whole calls on one GPU over worlds of at most 64 records, without per-box counts and segment checks";

// May a context whose active modes are `active` enter `enter`?  `among`: the modes asked about now -- a setter whose argument
// checks stand between two of its combination checks asks in stages, so that a call with two faults keeps its code.
struct Refusal { int code; Mode by; const char* clause; };
inline Refusal refusal(unsigned active, Mode enter, unsigned among = kAll) {
  active &= among;
  for (const Row& r : kRows) {
    if (r.a == enter && (active & r.b) && r.a_under_b) return {r.a_under_b, r.b, r.clause};
    if (r.b == enter && (active & r.a) && r.b_under_a) return {r.b_under_a, r.a, r.clause};
  }
  return {POCS_OK, enter, ""};
}

}  // namespace pocs_modes

// pocs_launch_forms.hpp -- which kernel a launch record asks for: the ONE place where the precedence of the features and what each of
// them needs, refuses and checks are written, host only (no HIP type, no context: tests/launch_forms_demo.cpp walks it under g++ and
// tests/test_launch_forms.py pins it to tests/golden/launch_forms.txt).  A chooser maps a record -- any type with the fields of
// pocs_gmm_launch / pocs_mc_launch that it reads -- to a form: the kernel's family and its template arguments other than K and TB, or
// the refusal.  pocs_kernels.hip maps a form to the kernel's address and launches it; a form without a kernel there is a refusal too.
// What the choosers answer is what the launchers' if / else ladders answered before them; where that looks unintended it is marked
// "quirk" and kept, for a later decision.
#pragma once

// The form word of the MC kernels: one of the three modes | the bits of a feature (pocs_dev_mc.hpp says what each one does).
enum { MC_PLAIN = 0, MC_COUNTS = 1, MC_STOP = 2, MC_BOXES = 4, MC_CLEAR = 8, MC_PARTS = 16, MC_REGIONS = 32, MC_SEG = 64, MC_ROUND = 128, MC_NOISE = 256,
       MC_RFOOT = 512, MC_HYP = 1024 };

namespace pocs_forms {

// The limits that the choosers check, restated so that this header needs no other: pocs_kernels.hip asserts that they are the library's.
constexpr int kMaxGaussians = 8, kMaxObstacles = 64, kMaxClearanceLevels = 4, kMaxFootprintParts = 4, kMaxRegions = 4, kMaxWorldRecords = 4096;

// The kernel families of the hot path that a chooser can name, each with the template arguments it has beside K and TB.
enum Arg : unsigned { kStore = 1, kLone = 2, kRisk = 4, kNT = 8, kWord = 16 };      // (in the order in which every family declares them)
#define POCS_FORM_FAMILIES(X)                                                                                                        \
  X(k_gmm_step, kStore | kLone) X(k_gmm_step_risk, kStore) X(k_gmm_step_boxes, kStore | kLone) X(k_gmm_step_risk_boxes, kStore)       \
  X(k_gmm_step_world, kStore) X(k_gmm_step_risk_world, kStore) X(k_gmm_step_clear, kStore) X(k_gmm_step_risk_clear, kStore)           \
  X(k_gmm_step_regions, kStore) X(k_gmm_step_risk_regions, kStore) X(k_gmm_step_parts, kStore) X(k_gmm_step_risk_parts, kStore)       \
  X(k_gmm_step_seg, kStore) X(k_gmm_step_risk_seg, kStore) X(k_gmm_step_round, kStore) X(k_gmm_step_risk_round, kStore)               \
  X(k_gmm_step_noise, kStore) X(k_gmm_step_risk_noise, kStore) X(k_gmm_step_rfoot, kStore) X(k_gmm_step_risk_rfoot, kStore)           \
  X(k_gmm_step_rfoot_noise, kStore) X(k_gmm_step_risk_rfoot_noise, kStore) X(k_gmm_step_hyp, 0) X(k_gmm_step_risk_hyp, 0)             \
  X(k_gmm_step_tree, kRisk) X(k_gmm_step_tree_boxes, kRisk)                                                                           \
  X(k_mc_init, kWord) X(k_mc_init_world, kWord) X(k_mc_step, kNT) X(k_mc_step_counts, kNT | kWord) X(k_mc_step_world, kNT | kWord)    \
  X(k_mc_fused, 0) X(k_mc_fused_counts, 0) X(k_mc_fused_boxes, 0) X(k_mc_fused_sched, kWord) X(k_mc_tree_step, kNT) X(k_mc_tree_step_boxes, kNT)
enum Family : int {
  refused = 0,
#define X(name, args) name,
  POCS_FORM_FAMILIES(X)
#undef X
};
struct FamilyRow { const char* name; unsigned args; };
static const FamilyRow kFamilies[] = {
    {"refused", 0},
#define X(name, args) {#name, args},
    POCS_FORM_FAMILIES(X)
#undef X
};

struct Form {
  Family fam;                    // refused: no launch
  bool store, lone, risk, nt;    // STORE, LONE, RISK, NT; false where the family has no such argument
  int word;                      // MODE, the OR of MC_* bits; 0 where the family has none
  explicit operator bool() const { return fam != refused; }
};
inline Form form(Family f, bool store, bool lone, bool risk, bool nt, int word) {
  const unsigned has = kFamilies[f].args;
  return {f, (has & kStore) && store, (has & kLone) && lone, (has & kRisk) && risk, (has & kNT) && nt, (has & kWord) ? word : 0};
}
constexpr Form kRefused = {refused, false, false, false, false, 0};

// The words of a record that take part in the choice, the FEATURES FIRST AND IN THE ORDER OF THEIR PRECEDENCE (both estimators: the
// first rule below whose words are all set answers, and the rules stand in this order).  kTree and kTail: pocs_gmm_launch alone.
enum Word : unsigned { kGates = 1u << 0, kRFoot = 1u << 1, kNoise = 1u << 2, kRound = 1u << 3, kSeg = 1u << 4, kParts = 1u << 5, kRegions = 1u << 6,
                       kClr = 1u << 7, kWorld = 1u << 8, kBoxes = 1u << 9, kLoneCall = 1u << 10, kTree = 1u << 11, kTail = 1u << 12 };
template <typename R>
unsigned feature_words(const R& a) {
  return (a.gates ? kGates : 0u) | (a.rfoot ? kRFoot : 0u) | (a.noise ? kNoise : 0u) | (a.round ? kRound : 0u) | (a.seg ? kSeg : 0u) |
         (a.parts ? kParts : 0u) | (a.regions ? kRegions : 0u) | (a.clr ? kClr : 0u) | (a.world ? kWorld : 0u) | (a.obs_counts ? kBoxes : 0u);
}
// What a rule checks of the values that travel with its feature, one short predicate each (below).
enum Check : unsigned { kM = 1u << 0, kM0 = 1u << 1, kFp = 1u << 2, kSegC = 1u << 3, kPartsF = 1u << 4, kRegG = 1u << 5, kClrL = 1u << 6, kKept = 1u << 7,
                        kWorldM = 1u << 8, kStep = 1u << 9, kStepIfWp = 1u << 10, kStepIfMode = 1u << 11, kCounting = 1u << 12, kStepOnly = 1u << 13 };
// A rule: the words that select it, the words it needs beside them, the words it refuses, its checks, and what it launches -- a GMM
// rule the family without and with the risk bound, an MC rule the feature bits of the form word (kWorld: the _world family).
struct Rule { unsigned match, needs, refuses, checks; Family plain, risk; int bits; };
template <typename R>
bool fits(const Rule& r, unsigned w, const R& a) {
  return (w & r.needs) == r.needs && !(w & r.refuses) && !((r.checks & kSegC) && !a.seg_counts) &&
         !((r.checks & kPartsF) && (a.parts_F < 2 || a.parts_F > kMaxFootprintParts)) &&
         !((r.checks & kRegG) && (!a.reg_counts || a.reg_G < 1 || a.reg_G > kMaxRegions)) &&
         !((r.checks & kClrL) && (!a.clr_counts || a.clr_L < 1 || a.clr_L > kMaxClearanceLevels));
}

// ---- GMM: one waypoint's sampling launch ------------------------------------------------------------------------------------------
constexpr unsigned kBelowRound = kSeg | kParts | kRegions | kClr, kTicket = kWorld | kBoxes | kLoneCall | kTree | kTail;   // (a ticket form's refusals)
static const Rule kGmmRules[] = {
    {kGates, kRound | kNoise, kRFoot | kBelowRound | kTicket, kM, k_gmm_step_hyp, k_gmm_step_risk_hyp, 0},
    {kRFoot | kNoise, 0, kBelowRound | kTicket, kM | kFp, k_gmm_step_rfoot_noise, k_gmm_step_risk_rfoot_noise, 0},
    {kRFoot, 0, kBelowRound | kTicket, kM | kFp, k_gmm_step_rfoot, k_gmm_step_risk_rfoot, 0},      // (`round` or not: the same family)
    {kNoise, kRound, kBelowRound | kTicket, kM, k_gmm_step_noise, k_gmm_step_risk_noise, 0},
    {kRound, 0, kBelowRound | kTicket, kM, k_gmm_step_round, k_gmm_step_risk_round, 0},
    {kSeg, 0, kParts | kRegions | kClr | kTicket, kM | kSegC, k_gmm_step_seg, k_gmm_step_risk_seg, 0},
    {kParts, 0, kClr | kTicket, kM | kPartsF, k_gmm_step_parts, k_gmm_step_risk_parts, 0},          // quirk: `regions` is not refused but ignored
    {kRegions, 0, kClr | kTicket, kM | kRegG, k_gmm_step_regions, k_gmm_step_risk_regions, 0},
    {kClr, 0, kTicket, kM | kClrL, k_gmm_step_clear, k_gmm_step_risk_clear, 0},
    {kWorld, 0, kBoxes | kLoneCall | kTree | kTail, kM0 | kKept, k_gmm_step_world, k_gmm_step_risk_world, 0},   // quirk: M == 0, not M <= the limit
    {kBoxes, 0, 0, kM, k_gmm_step_boxes, k_gmm_step_risk_boxes, 0},   // quirk: `tree_parent`, and `exchange_in_tail` without `risk`, are not looked at
    {0, 0, 0, 0, k_gmm_step, k_gmm_step_risk, 0},                     // quirk: nor here, and neither is M
};
template <typename R>
Form gmm_step_form(int K, const R& a) {
  if (K < 1 || K > kMaxGaussians) return kRefused;
  if (a.risk && (a.lone || a.exchange_in_tail || !a.stop || !a.surv)) return kRefused;   // the risk bound: a ticket form, single GPU, its two words
  const unsigned w = feature_words(a) | (a.lone ? kLoneCall : 0u) | (a.tree_parent ? kTree : 0u) | (a.exchange_in_tail ? kTail : 0u);
  for (const Rule& r : kGmmRules) {
    if ((w & r.match) != r.match) continue;
    if (!fits(r, w, a) || ((r.checks & kM) && a.M > kMaxObstacles) || ((r.checks & kM0) && a.M != 0) ||
        ((r.checks & kSegC) && !a.chain) || ((r.checks & kKept) && (!a.kept || !a.reach)) ||
        ((r.checks & kFp) && !(a.fp.dx == 0.0 && a.fp.dy == 0.0 && a.fp.hx == a.fp.hy && a.fp.hx >= 0.0)))      // a round footprint: {0, 0, rho, rho}
      return kRefused;
    return form(a.risk ? r.risk : r.plain, a.store != 0, a.lone != 0, false, false, 0);
  }
  return kRefused;
}
// One level of a tree of plans.  quirk: no feature but the per-box counts is looked at.
template <typename R>
Form gmm_tree_step_form(int K, const R& a) {
  if (K < 1 || K > kMaxGaussians || a.W != 1 || !a.tree_parent || a.lone || a.store || a.advance_in_tail || a.exchange_in_tail || a.run_cnt < 1 ||
      a.run_cnt > 256 || a.run_lo < 0 || a.run_lo + a.run_cnt > a.nruns || (a.risk && (!a.stop || !a.surv)))
    return kRefused;
  return form(a.obs_counts ? k_gmm_step_tree_boxes : k_gmm_step_tree, false, false, a.risk != 0, false, 0);
}

// ---- MC: the initial cloud (k_mc_init), one control (k_mc_step), the fused roll-out, one level of a tree -----------------------------
constexpr unsigned kNoTable = kWorld | kBoxes | kClr | kParts | kRegions | kSeg;      // (what the forms on top of MC_ROUND refuse)
static const Rule kMcRules[] = {
    {kGates | kNoise, kRound, kRFoot | kNoTable, kStep, refused, refused, MC_ROUND | MC_NOISE | MC_HYP},
    {kGates, kRound, kRFoot | kNoTable, kStep, refused, refused, MC_ROUND | MC_HYP},
    {kRFoot | kNoise, kRound, kNoTable, kStep, refused, refused, MC_ROUND | MC_NOISE | MC_RFOOT},      // (needs `round`; the GMM rule does not)
    {kRFoot, kRound, kNoTable, kStep, refused, refused, MC_ROUND | MC_RFOOT},
    {kNoise, kRound, kNoTable, kStep, refused, refused, MC_ROUND | MC_NOISE},
    {kRound, 0, kNoTable, kStep, refused, refused, MC_ROUND},
    {kSeg, 0, kWorld | kBoxes | kClr | kParts | kRegions, kStep | kSegC | kCounting | kStepOnly, refused, refused, MC_SEG},   // quirk: wp_mode 0 is refused here alone; k_mc_init ignores `seg` under the rules below
    {kParts, 0, kWorld | kBoxes | kClr, kStep | kPartsF, refused, refused, MC_PARTS},                // quirk: `regions` is not refused but ignored
    {kRegions, 0, kWorld | kBoxes | kClr, kStep | kRegG, refused, refused, MC_REGIONS},
    {kClr, 0, kWorld | kBoxes, kStep | kClrL, refused, refused, MC_CLEAR},
    {kWorld, 0, kBoxes, kWorldM | kStepIfWp, refused, refused, 0},
    {kBoxes, 0, 0, kStep | kCounting, refused, refused, MC_BOXES},
    {0, 0, 0, kStepIfMode, refused, refused, 0},
};
// `is_step`: k_mc_step's launch, which also checks its control index and obeys the risk bound (wp_mode 2).  quirk: a wp_mode that is
// none of 0, 1, 2 counts as 1 for k_mc_init and for the rules that need a counting mode, as 0 elsewhere.
template <typename R>
Form mc_form(bool is_step, const R& a) {
  if ((a.wp_mode != 0 && !a.wp_counts) || (a.obs_counts && !a.wp_mode)) return kRefused;
  if (is_step && a.wp_mode == 2 && (!a.wp_stop || a.wp_n < 1)) return kRefused;
  const unsigned w = feature_words(a);
  const bool step_ok = a.step >= 0 && a.step + 1 < a.W;
  for (const Rule& r : kMcRules) {
    if ((w & r.match) != r.match || ((r.checks & kStepOnly) && !is_step)) continue;
    int mode = !is_step ? (a.wp_mode ? MC_COUNTS : MC_PLAIN) : a.wp_mode == 2 ? MC_STOP : a.wp_mode == 1 ? MC_COUNTS : MC_PLAIN;
    if ((r.checks & kCounting) && mode == MC_PLAIN) { if (!a.wp_mode) return kRefused; mode = MC_COUNTS; }
    if (!fits(r, w, a) || ((r.checks & kClrL) && !a.clr_level) || ((r.checks & kWorldM) && (a.world_M < 1 || a.world_M > kMaxWorldRecords))) return kRefused;
    if (is_step && !step_ok && ((r.checks & kStep) || ((r.checks & kStepIfWp) && a.wp_mode != 0) || ((r.checks & kStepIfMode) && mode != MC_PLAIN)))
      return kRefused;
    const int word = mode | r.bits;
    if (r.match == kWorld) return form(is_step ? k_mc_step_world : k_mc_init_world, false, false, false, a.nontemporal != 0, word);
    if (is_step) return form(word == MC_PLAIN ? k_mc_step : k_mc_step_counts, false, false, false, a.nontemporal != 0, word);
    return form(k_mc_init, false, false, false, false, word);
  }
  return kRefused;
}
template <typename R> Form mc_init_form(const R& a) { return mc_form(false, a); }
template <typename R> Form mc_step_form(const R& a) { return mc_form(true, a); }
// The fused roll-out: the two plain modes, with or without per-box counts and an obstacle schedule -- no stop without a launch
// boundary per step, a large world is not staged, every other feature has the per-step form alone.  quirk: `gates`, `rfoot` and
// `noise` are not looked at (the host sets none of them without `round`).
template <typename R>
Form mc_fused_form(const R& a) {
  if (a.wp_mode == 2 || (a.wp_mode != 0 && !a.wp_counts) || (a.obs_counts && !a.wp_mode)) return kRefused;
  if (feature_words(a) & (kClr | kParts | kRegions | kSeg | kRound | kWorld)) return kRefused;
  const int word = a.obs_counts ? MC_COUNTS | MC_BOXES : a.wp_mode ? MC_COUNTS : MC_PLAIN;
  if (a.env_steps > 1) return form(k_mc_fused_sched, false, false, false, false, word);
  return form(word == MC_PLAIN ? k_mc_fused : word == MC_COUNTS ? k_mc_fused_counts : k_mc_fused_boxes, false, false, false, false, 0);
}
// One level of a tree of plans.  quirk: of the features, only a large world and the per-box counts are looked at.
template <typename R>
Form mc_tree_step_form(const R& a) {
  if (a.world || !a.tree_parent || !a.tree_sx || !a.tree_sy || !a.tree_sth || !a.tree_shits || !a.wp_counts || !a.total || a.nruns < 1 || a.nruns > 256 ||
      a.tree_dst_lo < 1 || a.tree_lo < a.tree_dst_lo || a.tree_src_lo < 0 || a.tree_src_lo >= a.tree_dst_lo || a.tree_sx == a.x)
    return kRefused;
  return form(a.obs_counts ? k_mc_tree_step_boxes : k_mc_tree_step, false, false, false, a.nontemporal != 0, 0);
}

}  // namespace pocs_forms

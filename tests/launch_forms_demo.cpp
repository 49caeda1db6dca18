// launch_forms_demo.cpp -- prints what csrc/pocs_launch_forms.hpp chooses, without a GPU: tests/test_launch_forms.py compares the
// output with tests/golden/launch_forms.txt.  Stand-in launch records (the fields the choosers read, nothing else) are enumerated
// over every setting of their choice words with every other value valid; one line per ACCEPTED record:
//   <launch> <the words that are set, or -> : <family><template arguments beside K and TB> ! <the single faults that refuse it, or ->
// Every fault of the launch's list is tried on every accepted record, so a fault that is absent from a line is one that the record's
// rule does not look at.  A record without a line is refused.
#include <cstdio>
#include <string>
#include <vector>

#include "../probability-of-collision-for-safe-planning_amd/csrc/pocs_launch_forms.hpp"

namespace {
using namespace pocs_forms;
const int kSome = 0;
const void* const P = &kSome;      // a valid pointer

struct GmmRec {      // the fields of pocs_gmm_launch that a chooser reads
  const void *gates, *noise, *seg, *parts, *regions, *clr, *world, *obs_counts, *tree_parent;
  int rfoot, round, risk, lone, store, exchange_in_tail, advance_in_tail;
  const void *stop, *surv, *seg_counts, *chain, *reg_counts, *clr_counts, *kept, *reach;
  int reg_G, clr_L, parts_F, M, W, nruns, run_lo, run_cnt;
  struct { double dx, dy, hx, hy; } fp;
};
struct McRec {       // the fields of pocs_mc_launch that a chooser reads
  const void *gates, *noise, *seg, *parts, *regions, *clr, *world, *obs_counts;
  int rfoot, round, wp_mode, nontemporal, env_steps;
  const void *wp_counts, *wp_stop, *seg_counts, *reg_counts, *clr_counts, *clr_level;
  long long wp_n;
  int reg_G, clr_L, parts_F, world_M, step, W, nruns;
  const void *tree_parent, *tree_sx, *tree_sy, *tree_sth, *tree_shits, *total, *x;
  int tree_lo, tree_dst_lo, tree_src_lo;
};

std::string text(const Form f) {
  if (!f) return "";
  const FamilyRow& row = kFamilies[f.fam];
  std::string s = row.name, args;
  const char* const tf[2] = {"false", "true"};
  auto add = [&](const std::string& v) { args += (args.empty() ? "" : ", ") + v; };
  if (row.args & kStore) add(tf[f.store]);
  if (row.args & kLone) add(tf[f.lone]);
  if (row.args & kRisk) add(tf[f.risk]);
  if (row.args & kNT) add(tf[f.nt]);
  if (row.args & kWord) add(std::to_string(f.word));
  return args.empty() ? s : s + "<" + args + ">";
}
// The six launches: "" = refused.
std::string gmm_step(int K, const GmmRec& a) { return text(gmm_step_form(K, a)); }
std::string gmm_tree_step(int K, const GmmRec& a) { return text(gmm_tree_step_form(K, a)); }
std::string mc_init(const McRec& a) { return text(mc_init_form(a)); }
std::string mc_step(const McRec& a) { return text(mc_step_form(a)); }
std::string mc_fused(const McRec& a) { return text(mc_fused_form(a)); }
std::string mc_tree_step(const McRec& a) { return text(mc_tree_step_form(a)); }
}  // namespace

// ---- the enumeration ----------------------------------------------------------------------------------------------------------------
namespace {
template <typename Rec> struct Fault { const char* name; void (*apply)(Rec&, int& K); };

// One line, if the record is accepted: its words, its form, and the faults of `faults` that, applied alone, refuse it.
template <typename Rec, typename Ask>
void line(const char* launch, const std::string& words, const Rec& a, const std::vector<Fault<Rec>>& faults, Ask ask) {
  const std::string f = ask(3, a);
  if (f.empty()) return;
  std::string refusing;
  for (const Fault<Rec>& x : faults) {
    Rec b = a;
    int K = 3;
    x.apply(b, K);
    if (ask(K, b).empty()) refusing += std::string(refusing.empty() ? "" : " ") + x.name;
  }
  printf("%s %s : %s ! %s\n", launch, words.empty() ? "-" : words.c_str(), f.c_str(), refusing.empty() ? "-" : refusing.c_str());
}
void word(std::string& s, bool set, const std::string& name) { if (set) s += (s.empty() ? "" : ",") + name; }

GmmRec gmm_valid() {
  GmmRec a = {};
  a.stop = a.surv = a.seg_counts = a.chain = a.reg_counts = a.clr_counts = a.kept = a.reach = P;
  a.reg_G = 2; a.clr_L = 2; a.parts_F = 2; a.M = 2; a.W = 4; a.nruns = 8; a.run_lo = 0; a.run_cnt = 8;
  a.fp = {0.0, 0.0, 0.5, 0.5};
  return a;
}
#define GF(name, stmt) {name, [](GmmRec& a, int& K) { (void)a; (void)K; stmt; }}
const std::vector<Fault<GmmRec>> kGmmFaults = {
    GF("stop=0", a.stop = nullptr), GF("surv=0", a.surv = nullptr), GF("seg_counts=0", a.seg_counts = nullptr), GF("chain=0", a.chain = nullptr),
    GF("reg_counts=0", a.reg_counts = nullptr), GF("reg_G=0", a.reg_G = 0), GF("reg_G=max+1", a.reg_G = kMaxRegions + 1),
    GF("clr_counts=0", a.clr_counts = nullptr), GF("clr_L=0", a.clr_L = 0), GF("clr_L=max+1", a.clr_L = kMaxClearanceLevels + 1),
    GF("parts_F=1", a.parts_F = 1), GF("parts_F=max+1", a.parts_F = kMaxFootprintParts + 1), GF("kept=0", a.kept = nullptr),
    GF("reach=0", a.reach = nullptr), GF("M=65", a.M = 65), GF("M=3", a.M = 3), GF("fp.dx!=0", a.fp.dx = 0.1), GF("fp.dy!=0", a.fp.dy = 0.1),
    GF("fp.hx!=hy", a.fp.hy = 0.7), GF("fp.hx<0", a.fp.hx = a.fp.hy = -0.5), GF("K=0", K = 0), GF("K=9", K = 9)};
const std::vector<Fault<GmmRec>> kGmmTreeFaults = {
    GF("stop=0", a.stop = nullptr), GF("surv=0", a.surv = nullptr), GF("tree_parent=0", a.tree_parent = nullptr), GF("advance_in_tail", a.advance_in_tail = 1),
    GF("exchange_in_tail", a.exchange_in_tail = 1), GF("run_cnt=0", a.run_cnt = 0), GF("run_cnt=257", (a.run_cnt = 257, a.nruns = 300)),
    GF("run_lo=-1", a.run_lo = -1), GF("run_lo+run_cnt>nruns", a.run_lo = 1), GF("M=65", a.M = 65), GF("K=0", K = 0), GF("K=9", K = 9)};

McRec mc_valid() {
  McRec a = {};
  a.wp_counts = a.wp_stop = a.seg_counts = a.reg_counts = a.clr_counts = a.clr_level = P;
  a.wp_n = 1000; a.reg_G = 2; a.clr_L = 2; a.parts_F = 2; a.world_M = 100; a.step = 1; a.W = 4; a.nruns = 8; a.env_steps = 1;
  static const int other = 0;
  a.tree_parent = a.tree_sx = a.tree_sy = a.tree_sth = a.tree_shits = a.total = P; a.x = &other;
  a.tree_lo = 3; a.tree_dst_lo = 3; a.tree_src_lo = 1;
  return a;
}
#define MF(name, stmt) {name, [](McRec& a, int&) { stmt; }}
const std::vector<Fault<McRec>> kMcFaults = {
    MF("wp_counts=0", a.wp_counts = nullptr), MF("wp_stop=0", a.wp_stop = nullptr), MF("wp_n=0", a.wp_n = 0), MF("step=-1", a.step = -1),
    MF("step=W-1", a.step = a.W - 1), MF("seg_counts=0", a.seg_counts = nullptr), MF("reg_counts=0", a.reg_counts = nullptr), MF("reg_G=0", a.reg_G = 0),
    MF("reg_G=max+1", a.reg_G = kMaxRegions + 1), MF("clr_counts=0", a.clr_counts = nullptr), MF("clr_level=0", a.clr_level = nullptr),
    MF("clr_L=0", a.clr_L = 0), MF("clr_L=max+1", a.clr_L = kMaxClearanceLevels + 1), MF("parts_F=1", a.parts_F = 1),
    MF("parts_F=max+1", a.parts_F = kMaxFootprintParts + 1), MF("world_M=0", a.world_M = 0), MF("world_M=max+1", a.world_M = kMaxWorldRecords + 1)};
const std::vector<Fault<McRec>> kMcTreeFaults = {
    MF("tree_parent=0", a.tree_parent = nullptr), MF("tree_sx=0", a.tree_sx = nullptr), MF("tree_sy=0", a.tree_sy = nullptr), MF("tree_sth=0", a.tree_sth = nullptr),
    MF("tree_shits=0", a.tree_shits = nullptr), MF("wp_counts=0", a.wp_counts = nullptr), MF("total=0", a.total = nullptr), MF("nruns=0", a.nruns = 0),
    MF("nruns=257", a.nruns = 257), MF("tree_dst_lo=0", a.tree_dst_lo = 0), MF("tree_lo<tree_dst_lo", a.tree_lo = 2),
    MF("tree_src_lo=-1", a.tree_src_lo = -1), MF("tree_src_lo=tree_dst_lo", a.tree_src_lo = a.tree_dst_lo), MF("tree_sx=x", a.tree_sx = a.x)};

// The ten feature words, the same for both records and in the order of the choosers' precedence: bit i of `bits` sets word i.
const char* const kFeatures[10] = {"gates", "rfoot", "noise", "round", "seg", "parts", "regions", "clr", "world", "obs_counts"};
template <typename Rec>
void set_features(Rec& a, unsigned bits, std::string& words) {
  const void** const ptr[10] = {&a.gates, nullptr, &a.noise, nullptr, &a.seg, &a.parts, &a.regions, &a.clr, &a.world, &a.obs_counts};
  for (int i = 0; i < 10; ++i) {
    if (!(bits >> i & 1u)) continue;
    if (ptr[i]) *ptr[i] = P; else (i == 1 ? a.rfoot : a.round) = 1;
    word(words, true, kFeatures[i]);
  }
}
}  // namespace

int main() {
  for (unsigned bits = 0; bits < (1u << 15); ++bits) {      // GMM step: the ten features, risk, lone, store, tree_parent, exchange_in_tail
    GmmRec a = gmm_valid();
    std::string w;
    set_features(a, bits & 1023u, w);
    if (a.world) a.M = 0;                                    // (a large world: the records travel in `kept`)
    a.risk = bits >> 10 & 1; a.lone = bits >> 11 & 1; a.store = bits >> 12 & 1; a.tree_parent = (bits >> 13 & 1) ? P : nullptr; a.exchange_in_tail = bits >> 14 & 1;
    word(w, a.risk, "risk"); word(w, a.lone, "lone"); word(w, a.store, "store"); word(w, a.tree_parent, "tree_parent"); word(w, a.exchange_in_tail, "exchange_in_tail");
    line("gmm_step", w, a, kGmmFaults, [](int K, const GmmRec& r) { return gmm_step(K, r); });
  }
  for (unsigned bits = 0; bits < 32; ++bits) {               // GMM tree step: obs_counts, risk, store, lone, W in {1, 2}
    GmmRec a = gmm_valid();
    std::string w;
    a.tree_parent = P; a.W = 1;
    a.obs_counts = (bits & 1) ? P : nullptr; a.risk = bits >> 1 & 1; a.store = bits >> 2 & 1; a.lone = bits >> 3 & 1; a.W = 1 + (bits >> 4 & 1);
    word(w, a.obs_counts, "obs_counts"); word(w, a.risk, "risk"); word(w, a.store, "store"); word(w, a.lone, "lone"); word(w, a.W == 2, "W=2");
    line("gmm_tree_step", w, a, kGmmTreeFaults, [](int K, const GmmRec& r) { return gmm_tree_step(K, r); });
  }
  // MC: the ten features x wp_mode 0, 1, 2 -- and 3, a value the host never sets -- x nontemporal (step) or env_steps 1, 7 (fused)
  for (int launch = 0; launch < 3; ++launch)
    for (unsigned bits = 0; bits < 1024u; ++bits)
      for (int wp = 0; wp < 4; ++wp)
        for (int v = 0; v < (launch == 0 ? 1 : 2); ++v) {
          McRec a = mc_valid();
          std::string w;
          set_features(a, bits, w);
          a.wp_mode = wp;
          word(w, wp != 0, "wp_mode=" + std::to_string(wp));
          if (launch == 1) { a.nontemporal = v; word(w, v, "nontemporal"); }
          if (launch == 2) { a.env_steps = v ? 7 : 1; word(w, v, "env_steps=7"); }
          if (launch == 0) line("mc_init", w, a, kMcFaults, [](int, const McRec& r) { return mc_init(r); });
          if (launch == 1) line("mc_step", w, a, kMcFaults, [](int, const McRec& r) { return mc_step(r); });
          if (launch == 2) line("mc_fused", w, a, kMcFaults, [](int, const McRec& r) { return mc_fused(r); });
        }
  for (unsigned bits = 0; bits < 8; ++bits) {                // MC tree step: obs_counts, nontemporal, world
    McRec a = mc_valid();
    std::string w;
    a.obs_counts = (bits & 1) ? P : nullptr; a.nontemporal = bits >> 1 & 1; a.world = (bits >> 2 & 1) ? P : nullptr;
    word(w, a.obs_counts, "obs_counts"); word(w, a.nontemporal, "nontemporal"); word(w, a.world, "world");
    line("mc_tree_step", w, a, kMcTreeFaults, [](int, const McRec& r) { return mc_tree_step(r); });
  }
  return 0;
}

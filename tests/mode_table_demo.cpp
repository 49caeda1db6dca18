// mode_table_demo.cpp -- prints csrc/pocs_modes.hpp (the modes of a context and the table of the pairs that exclude each other)
// without a GPU and without a context: tests/test_mode_table.py reads it.
//   mode <bit> <name>                      the ten modes; "ask": the calls that enter no mode and are still refused under one
//   row <a> <b> <a under b> <b under a> <clause>
//   enter <mode or ask> under <active mode, or 0 for none> <code>
#include <cstdio>

#include "../probability-of-collision-for-safe-planning_amd/csrc/pocs_modes.hpp"

int main() {
  using namespace pocs_modes;
  const int n = kNumModes + kNumAsks;
  for (int i = 0; i < n; ++i) printf("%s %u %s\n", i < kNumModes ? "mode" : "ask", 1u << i, name((Mode)(1u << i)));
  for (const Row& r : kRows) printf("row %u %u %d %d %s\n", (unsigned)r.a, (unsigned)r.b, r.a_under_b, r.b_under_a, r.clause);
  for (int i = 0; i < n; ++i) {
    printf("enter %u under 0 %d\n", 1u << i, refusal(0u, (Mode)(1u << i)).code);
    for (int j = 0; j < kNumModes; ++j) printf("enter %u under %u %d\n", 1u << i, 1u << j, refusal(1u << j, (Mode)(1u << i)).code);
  }
  return 0;
}

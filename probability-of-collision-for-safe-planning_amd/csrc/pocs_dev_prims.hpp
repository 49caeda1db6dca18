// pocs_dev_prims.hpp -- device primitives every kernel family uses, a part of pocs_kernels.hip (the only unit with device
// code; included there, inside its anonymous namespace).  Relies on no other part.
//
//   wave sums         dpp_f64, row_sum_u32, wave_sum_u32
//   table staging     stage_tables; request_tables / commit_tables with requests_issued between them
//   hand-offs         store_wt / load_wt (write-through, L1-bypassing), store16_nt / store4_nt (the sample stream),
//                     lane_value, uniform64, drain_stores, acquire_agent
//   diagnostic hooks  POCS_STAMP* / POCS_TUNE_*: no-ops unless built with -DPOCS_TUNING (pocs_tuning.h)

// Row sums by DPP: four steps (pairs, quads, half rows, rows) leave every lane of a 16-lane row
// holding its row's sum.  Every lane has a valid source in all four patterns, so `old` is never
// used; the shape is fixed, hence bitwise reproducible run to run.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  // (`old` = 0 with bound_ctrl: every lane has a valid source in the patterns used here, so `old` is never
  // taken, and the compiler need not copy the source to protect it)
  const int lo2 = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
  const int hi2 = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi2, lo2);
}
__device__ __forceinline__ unsigned row_sum_u32(unsigned v) {
  v += (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false);
  v += (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false);
  v += (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false);
  v += (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false);
  return v;
}
// Whole-wave sums (MC count kernel): row sums read back through SGPRs, added in row order.
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
  v = row_sum_u32(v);
  return (unsigned)__builtin_amdgcn_readlane((int)v, 0) + (unsigned)__builtin_amdgcn_readlane((int)v, 16) +
         (unsigned)__builtin_amdgcn_readlane((int)v, 32) + (unsigned)__builtin_amdgcn_readlane((int)v, 48);
}

// Stage the log / sector tables (12 KB) into LDS.  The log table's 1/c entries are DOUBLED on the way in:
// the device form of pocs_radius2_unit32 multiplies them with the mantissa in [1/2, 1) (pocs_math.h).
__device__ __forceinline__ void stage_tables(const pocs_tables* __restrict__ g, pocs_tables* s_tab) {
  const double* src = reinterpret_cast<const double*>(g);
  double* dst = reinterpret_cast<double*>(s_tab);
  constexpr int NLG = (int)(sizeof(g->lg) / sizeof(double));
  for (int j = threadIdx.x; j < (int)(sizeof(pocs_tables) / sizeof(double)); j += blockDim.x)
    dst[j] = (j < NLG && (j & 1) == 0) ? 2.0 * src[j] : src[j];
}

// The same in two steps for a block of TB threads (k_gmm_step's heads): the loads, into registers -- and, once everything
// else the head needs has been requested behind them, the stores.  (stage_tables' loop has a run-time stride: the
// compiler keeps it a loop and waits for every load before it issues the next, three memory round trips one after the
// other for 24 bytes per thread.)
constexpr int POCS_TABLE_DOUBLES = (int)(sizeof(pocs_tables) / sizeof(double));
template <int TB> struct table_regs { static constexpr int N = (POCS_TABLE_DOUBLES + TB - 1) / TB; };
template <int TB>
__device__ __forceinline__ void request_tables(const pocs_tables* __restrict__ g, const int tid, double (&v)[table_regs<TB>::N]) {
  const double* src = reinterpret_cast<const double*>(g);
#pragma unroll
  for (int u = 0; u < table_regs<TB>::N; ++u) { const int j = tid + u * TB; v[u] = (j < POCS_TABLE_DOUBLES) ? src[j] : 0.0; }
}
template <int TB>
__device__ __forceinline__ void commit_tables(pocs_tables* s_tab, const int tid, const double (&v)[table_regs<TB>::N]) {
  double* dst = reinterpret_cast<double*>(s_tab);
  constexpr int NLG = (int)(sizeof(s_tab->lg) / sizeof(double));
#pragma unroll
  for (int u = 0; u < table_regs<TB>::N; ++u) {
    const int j = tid + u * TB;
    if (j < POCS_TABLE_DOUBLES) dst[j] = (j < NLG && (j & 1) == 0) ? 2.0 * v[u] : v[u];
  }
}
// everything requested so far is in flight before anything that follows is issued (loads do not sink below it, stores do
// not rise above it): the head's requests, then ONE wait
__device__ __forceinline__ void requests_issued() { asm volatile("" ::: "memory"); }

// ---------------------------------------------------------------------------------------------
// Hand-offs between workgroups (the rows of a run's virtual slices -> the last arriver, inside a launch; mixture
// state and sampler parameters -> the blocks of the next waypoint's launch).  cdna_hip_programming.md Guideline 16,
// form R1: every handed-off byte is stored write-through (`sc1`: a relaxed agent-scope atomic
// store), every storing wave drains its stores (s_waitcnt vmcnt(0)), the block meets, ONE lane
// signals with an agent-scope atomic (ticket add / `ready` store).  The consumer polls or draws
// its ticket relaxed, then ONE agent-scope acquire fence (buffer_inv sc1: this CU's L1) + its
// vmcnt(0) + the block barrier, and only then are the bytes loaded -- with L1-bypassing loads on top
// (relaxed agent-scope atomic loads), so no stale line can be served whatever else shares the CU.
// tests/test_handoff_isa.py disassembles libpocs.so and checks that the emitted ISA has these shapes.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void store_wt(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double load_wt(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load(
      reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
typedef double v2d __attribute__((ext_vector_type(2)));
// The sample stream: SGPR base + 32-bit lane offset, non-temporal (the compiler, left to itself,
// builds a 64-bit address per lane and store: four vector adds per iteration)
__device__ __forceinline__ void store16_nt(const void* base_uniform, unsigned lane_bytes, v2d v) {
  asm volatile("global_store_dwordx4 %0, %1, %2 nt\n\ts_nop 1" ::"v"(lane_bytes), "v"(v), "s"(base_uniform) : "memory");
}
__device__ __forceinline__ void store4_nt(const void* base_uniform, unsigned lane_bytes, int v) {
  asm volatile("global_store_dword %0, %1, %2 nt" ::"v"(lane_bytes), "v"(v), "s"(base_uniform) : "memory");
}
// lane `l`'s value of v, in every lane
__device__ __forceinline__ double lane_value(double v, int l) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
// a 64-bit value the program knows to be wave-uniform, pinned into scalar registers
__device__ __forceinline__ long long uniform64(long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// consumer side, ONE lane, after its poll matched / its ticket came back: drop this CU's stale lines
__device__ __forceinline__ void acquire_agent() {
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the invalidate completes before the barrier releases the readers
}

// Diagnostic hooks (phase stamps, timing-only ablations of the sampling body): real only in a -DPOCS_TUNING build
// (csrc/pocs_tuning.h, tools/ablate.sh); the shipped library sees the no-ops / pass-throughs below.
#ifdef POCS_TUNING
#include "pocs_tuning.h"
#else
#define POCS_STAMP_BEGIN() do { } while (0)
#define POCS_STAMP(i) do { } while (0)
#define POCS_STAMP_COUNT(i) do { } while (0)
#define POCS_ADV_STAMP_BEGIN() do { } while (0)
#define POCS_ADV_STAMP(i) do { } while (0)
#define POCS_TUNE_NORMALS(...) __VA_ARGS__
#define POCS_TUNE_COLLIDE(...) __VA_ARGS__
#define POCS_TUNE_COLLIDE_STATS() do { } while (0)
#define POCS_TUNE_SKIP_MOMENTS false
#define POCS_TUNE_MOMENTS_ALT() do { } while (0)
#endif

// Extended-range MaxEnt backward pass: what extended.hip (fused and per-sweep
// shapes, planner, entry point) and extended_grid.hip (persistent grid shape)
// share -- the (mantissa, exponent) form of a partition value, the kernel
// arguments and the grid shape's plan and launch.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

#include "common.h"
#include "fixed_point.h"

namespace irlmx {

constexpr int kExtZero = INT_MIN;      // exponent of an exact zero: never raises a maximum
constexpr int kExtMinShift = -1100;    // ldexp(m, shift) is 0 below -1075 already
constexpr int kExtMaxStates = 1 << 19; // |e| grows by < 1100 per sweep: no int32 wrap within 2*S sweeps
constexpr size_t kExtLdsPerState = 2 * sizeof(double) + 2 * sizeof(int);
constexpr size_t kExtLdsMax = 160 * 1024;

struct ExtArgs {
  Model m;
  const double* w;  // [B][K][S] collapsed, reward-folded weights (bwd_weights_kernel)
  const double* reward;
  const uint8_t* term;
  const int32_t* bad;  // [B] non-finite weights (bwd_nonfinite_rule)
  double* pi;          // [B][S][A]
  int32_t* status;
};

struct ExtWs {
  double* wgt;     // [B][K][S]
  int32_t* bad;    // [B]
  double* man[2];  // [B][S] mantissas, ping and pong (per-sweep shape)
  int32_t* exp[2]; // [B][S] exponents
  size_t total;
};

// m * 2^(e - E) with the shift clamped to [kExtMinShift, 0]: the difference is
// taken in 64 bits (e and E may be far apart, or kExtZero).  A slot whose
// weight is 0 may hold e > E; its product is 0 at any finite shift.
__device__ inline double ext_aligned(double mant, int e, int E) {
  const long long d = (long long)e - (long long)E;
  const int sh = d < kExtMinShift ? kExtMinShift : (d > 0 ? 0 : (int)d);
  return ldexp(mant, sh);
}

// acc -> (mantissa, exponent) on top of the alignment exponent E
__device__ inline void ext_split(double acc, int E, double* mant, int* e) {
  if (acc == 0.0) { *mant = 0.0; *e = kExtZero; return; }
  if (!isfinite(acc)) { *mant = acc; *e = 0; return; }  // non-finite weights: the instance is NaN-filled
  int d;
  *mant = frexp(acc, &d);
  *e = E + d;
}

__device__ inline void ext_init_state(bool terminal, double* mant, int* e) {
  *mant = terminal ? 0.5 : 0.0;  // 1 = 0.5 * 2^1
  *e = terminal ? 1 : kExtZero;
}

// ---------------------------------------------------------------------------
// persistent grid shape (extended_grid.hip)
// ---------------------------------------------------------------------------

// states per thread, compiled slots, workgroups per instance, XCD grouping,
// instances per launch and sequential launches
struct ExtGridPlan {
  int spt, kmax, bpi, xcd, ipl, launches;
};

// granules of the grid shape, sized for the plan's instances per launch
struct ExtGridWs {
  unsigned long long* gran;   // [ipl][3][S][2] x 16 B: mantissa and exponent granules, rings of three sweeps
  unsigned long long* dgran;  // [ipl][4][bpi] x 16 B: three sweeps of block words + the XCC ids
  int* err;                   // [4]: error bits, rendezvous counters
};

// The <spt, kmax> instantiation of ext_grid_kernel, nullptr for a pair that is not compiled.
void* ext_grid_fn(int spt, int kmax);
// ceil(B / ipl) sequential persistent launches, each with zeroed granules and
// its own salt; reads every launch's outcome (synchronises the stream): 0,
// kClusterNotResident (rerun the whole call per sweep) or an IRLMX_E* code.
int ext_grid_run(const Model& m, const ExtGridPlan& gp, const ExtArgs& a, const ExtGridWs& ws, hipStream_t st);

}  // namespace irlmx

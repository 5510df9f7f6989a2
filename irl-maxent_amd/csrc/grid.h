// Persistent grid shape (grid.hip): its planner and its launch.
#pragma once

#include "fixed_point.h"

namespace irlmx {

constexpr int kGridThreads = 256;

// states per thread, workgroups per instance, workgroups dealt to XCD groups
struct GridPlan {
  int spt, bpi, xcd;
};
// The grid shape of `op` on this model; false when it does not apply.
bool grid_plan(const Model& m, int op, GridPlan* out);

// Arguments of the forward and backward grid kernels (linear_grid_kernel).
struct LinearGridArgs {
  Model m;
  const double* w;      // [B][K][S] forward gather weights / reward-folded backward weights
  const double* vin;    // forward: p0 [B][S]; backward: reward [B][S]
  const uint8_t* term;  // backward: terminal mask
  const int32_t* bad;   // [B] non-finite policy (forward) / weights (backward)
  double eps;
  long long max_iter;
  int rescale;
  double* out;          // forward: svf [B][S]; backward: pi [B][S][A]
  int64_t* iters;
  int32_t* status;
};

// One persistent launch of `op` (Args: LinearGridArgs, or SoftArgs for soft VI /
// VI), then its exchange-timeout word (synchronises the stream, like
// cluster_run): 0, kClusterNotResident (rerun per sweep) or an IRLMX_E* code.
template <class Args>
int grid_run(const Model& m, int op, const GridPlan& gp, Args a, const Ws& ws, hipStream_t st);

}  // namespace irlmx

// Model views and host helpers of the fixed-point passes that more than one
// translation unit uses (fixed_point.hip defines the host functions;
// extended.hip is the other user).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "common.h"

namespace irlmx {

constexpr int kFusedMaxStates = 4096;
constexpr int kMaxActions = 8;
constexpr int kSweepThreads = 256;

// Largest S run by the fused shape; IRLMX_FUSED_MAX_STATES lowers it (tests use
// 0 to drive every size through the sweep shape).
int fused_max_states();

// ---------------------------------------------------------------------------
// model views
// ---------------------------------------------------------------------------

struct Model {
  int S, A, K, W, H, B, stencil, shared, Kc, dense;
  int props;  // irlmx_mdp.props: IRLMX_PROPS_KNOWN | IRLMX_PROP_* from irlmx_mdp_properties, or 0 (unknown)
  const double* row_val;
  const int32_t* row_idx;
  const int32_t* col_idx;
  const double* col_val;
};

inline Model make_model(const irlmx_mdp* m) {
  Model o;
  o.S = m->n_states;
  o.A = m->n_actions;
  o.stencil = m->layout == IRLMX_LAYOUT_STENCIL5;
  o.dense = m->layout == IRLMX_LAYOUT_DENSE;
  o.K = o.stencil ? kStencilK : (o.dense ? m->n_states : m->k_row);
  o.Kc = o.stencil ? kStencilK : (o.dense ? m->n_states : m->k_col);
  o.W = m->width;
  o.H = m->height;
  o.B = m->batch;
  o.shared = m->shared != 0;
  o.row_val = m->row_val;
  o.row_idx = m->row_idx;
  o.col_idx = m->col_idx;
  o.col_val = m->col_val;
  o.props = m->props;
  return o;
}

__device__ inline size_t inst_of(const Model& m, int b) { return m.shared ? 0 : (size_t)b; }

// neighbour (row form) of s in slot k
__device__ inline int row_nbr(const Model& m, int b, int s, int k) {
  if (m.stencil) return stencil_nbr(s, k, m.W, m.H);
  const int t = m.row_idx[(inst_of(m, b) * m.K + k) * m.S + s];
  return IRLMX_DCHECK(t >= 0 && t < m.S, kCheckIndex) ? t : s;
}

__device__ inline double row_val(const Model& m, int b, int a, int k, int s) {
  return m.row_val[((inst_of(m, b) * m.A + a) * m.K + k) * m.S + s];
}

// source (column form) of target t in slot k
__device__ inline int col_src(const Model& m, int b, int t, int k) {
  if (m.stencil) return stencil_nbr(t, k, m.W, m.H);
  const int s = m.col_idx[(inst_of(m, b) * m.Kc + k) * m.S + t];
  return IRLMX_DCHECK(s >= 0 && s < m.S, kCheckIndex) ? s : t;
}

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// ---------------------------------------------------------------------------
// host helpers (fixed_point.hip)
// ---------------------------------------------------------------------------

// The model checks every entry point starts with: 0, or IRLMX_EINVAL with the message set.
int validate(const irlmx_mdp* mdp);

// Required array arguments of an entry point: NULL is rejected before any work
// is enqueued (a null device pointer would fault the GPU).
struct Arg {
  const void* p;
  const char* name;  // nullptr: optional argument
};
int need_all(const char* fn, std::initializer_list<Arg> args);

// The fused shape (one workgroup per instance) of `op` on this model: states
// per thread, compiled slot count and threads; false when it does not apply.
// `cluster_first`: grids of width 64 / 128 leave the forward and backward
// passes to the cluster shape (cluster.hip) even when they fit one CU.
struct FusedShape {
  int spt;
  int kmax;
  int threads;
};
bool fused_shape(const Model& m, int op, FusedShape* out, bool cluster_first = true);

// Enqueue bwd_weights_kernel: w[b][k][s] = exp(r[b][s]) * sum_a P[s, target_k(s), a],
// bad[b] |= 1 where a weight is non-finite (bwd_nonfinite_rule).
void bwd_weights_launch(const Model& m, const double* reward, double* w, int32_t* bad, hipStream_t st);

// The extended-range backward (extended.hip): whether this model is one it
// runs (else IRLMX_EINVAL and the message, prefixed by `fn`), its workspace
// and its plan (irlmx_workspace_bytes / irlmx_execution_plan with
// IRLMX_PLAN_EXTENDED_RANGE).
int extended_check_model(const Model& m, const char* fn);
size_t extended_workspace_bytes(const Model& m);
void extended_plan(const Model& m, int64_t* plan);

}  // namespace irlmx

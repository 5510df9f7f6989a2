// Model views, the workspace and its carver, the stopping-rule helpers, the
// argument struct of the Bellman kernels and the host plumbing of the
// fixed-point passes that more than one translation unit uses: the argument and
// workspace checks, the fused shape with its (SPT, KMAX) predicate, dispatcher
// (with_pair) and launcher (launch_fused), the slot classes, the per-sweep
// launch grid and the plan rows (fixed_point.hip defines what is not a
// template; grid.hip, extended_grid.hip, numpy_order.hip, extended.hip,
// policy_eval.hip, horizon.hip and soft_horizon.hip are the other users).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

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
// workspace (carve(), fixed_point.hip)
// ---------------------------------------------------------------------------

struct Ws {
  double* wgt;                // forward: [B][Kc][S] gather weights; backward: [B][K][S] reward-folded;
                              // policy evaluation: [B][K][S] policy-folded
  int32_t* bad;               // [B] forward: policy has a non-finite entry
  double* buf0;               // [B][S]   sweep path ping
  double* buf1;               // [B][S]   sweep path pong
  unsigned long long* slots;  // [B][3]
  int32_t* done;              // [B]
  int64_t* iters;             // [B]
  int32_t* ndone;             // [1]
  // cluster shape (stencil layouts too large for one CU); sizes as carve() takes them:
  unsigned long long* gran;   // cluster: [B][gran_inst_len(W, H)] x 16 B (two padded halo parities, cluster.h);
                              // grid: [B][3][S] x 16 B; dense grid: [B][2][S] x 16 B
  unsigned long long* sgran;  // cluster: [B][kSumRows][H] x 16 B (tile summaries by block % kSumSlots,
                              // then the XCC ids and the forward's full flags, cluster.h); grid: [B][4][bpi]; dense grid: [B][bpi] x 16 B
  unsigned long long* growth; // [2][B] growth / decay bounds (bwd_growth_kernel)
  int* err;                   // [4]: error bits, rendezvous counters
  size_t total;
};

// Consecutive 256-byte aligned pieces of a workspace at `base` (nullptr: sizes only).
struct Carver {
  char* base;
  size_t off = 0;
  template <class T>
  T* take(size_t bytes) {
    T* r = base ? (T*)(base + off) : nullptr;
    off += align256(bytes);
    return r;
  }
  size_t total() const { return off; }
};

// The workspace of `op` (IRLMX_OP_*) on this model, carved from `base` (nullptr: sizes only).
Ws carve(const Model& m, int op, void* base);
// IRLMX_EWORKSPACE and the message unless `bytes` at `ws` hold `need` (of `op`
// on this model: carve(m, op).total); a NULL `ws` passes only where need is 0.
int check_ws(size_t need, size_t bytes, void* ws);
int check_ws(const Model& m, int op, size_t bytes, void* ws);

// Arguments of the soft VI / VI kernels of every shape (fixed_point.hip fused
// and per sweep, grid.hip, numpy_order.hip).
struct SoftArgs {
  Model m;
  const double* reward;
  const double* phi;  // soft: terminal reward; unused by VI
  double discount;
  double eps;
  long long max_iter;
  int average;  // VI only
  double* pi;   // soft only, [B][S][A]
  double* value;
  int64_t* iters;
  int32_t* status;
};

// ---------------------------------------------------------------------------
// the stopping rule, fused shape
// ---------------------------------------------------------------------------

__device__ inline int finish_status(double delta, double eps) {
  if (delta != delta) return IRLMX_NONFINITE;
  return delta > eps ? IRLMX_MAXITER : IRLMX_OK;
}

// The reference's fixed-point loops stop after the first sweep whose
// max|x_new - x| is not > eps, NaN included (maxent.py:108, :335, solver.py:49).
// run_deferred keeps that rule without a per-sweep reduction: each lane records
// per sweep i "some |x_new - x| > eps" (bit i) and "some |x_new - x| is NaN"
// (bit 32 + i) for its states (record_delta), and the workgroup ORs the bits
// once per block of kDeferBlock sweeps.  If the block holds the stopping sweep
// k, restore() puts the block-start state back (LDS and registers; save() took
// it) and sweeps 0..k are replayed -- the same arithmetic, so the same bits.
// sweep(it, pos, bits) runs one sweep from buffer parity it & 1 and records at
// bit pos (the helpers put the barrier after it); slot[0..2] are zero on entry.
// Returns the status (OK, NONFINITE, MAXITER); `it` counts the sweeps done.
// One call site of sweep(), so it is inlined once.  run_each is the per-sweep
// form for kernels whose registers have no room for the block bookkeeping: the
// same bits, reduced every sweep with two ballots (no cross-lane shuffles).
constexpr int kDeferBlock = 32;
__device__ inline void record_delta(unsigned long long& bits, int pos, double d, double eps) {
  bits |= ((d > eps) ? 1ull : 0ull) << pos;
  bits |= ((d != d) ? 1ull : 0ull) << (32 + pos);
}
template <class Sweep, class Save, class Restore>
__device__ __attribute__((always_inline)) inline int run_deferred(long long max_iter, unsigned long long* slot,
                                                                  long long& it, Sweep&& sweep, Save&& save,
                                                                  Restore&& restore) {
  const int tid = threadIdx.x;
  for (int blk = 0;; ++blk) {
    save();
    int nb = kDeferBlock;
    if (max_iter > 0) nb = (int)min<long long>(nb, max_iter - it);
    int k = -1;
    unsigned nan = 0u;
    for (int pass = 0; pass < 2; ++pass) {  // the block, then (stop inside it) the replay
      unsigned long long bits = 0ull;
      const int cnt = pass == 0 ? nb : k + 1;
      for (int i = 0; i < cnt; ++i) {
        sweep(it + i, i, bits);
        __syncthreads();
      }
      if (pass == 1) break;
      bits = wave_or_u64(bits);
      if ((tid & (kWave - 1)) == 0 && bits) atomicOr(&slot[blk & 1], bits);
      if (tid == 0) slot[(blk & 1) ^ 1] = 0ull;  // last read in the previous block, before this block's barriers
      __syncthreads();
      const unsigned long long all = slot[blk & 1];
      const unsigned gt = (unsigned)all;
      nan = (unsigned)(all >> 32);
      const unsigned live = nb >= 32 ? 0xFFFFFFFFu : ((1u << nb) - 1u);
      const unsigned stop = (~gt | nan) & live;
      if (!stop) break;
      k = __builtin_ctz(stop);
      restore();
    }
    if (k >= 0) {
      it += k + 1;
      return ((nan >> k) & 1u) ? IRLMX_NONFINITE : IRLMX_OK;
    }
    it += nb;
    if (max_iter > 0 && it >= max_iter) return IRLMX_MAXITER;
  }
}
template <class Sweep>
__device__ __attribute__((always_inline)) inline int run_each(long long max_iter, unsigned long long* slot,
                                                              long long& it, Sweep&& sweep) {
  const int tid = threadIdx.x;
  for (int r3 = 0;; r3 = r3 == 2 ? 0 : r3 + 1) {
    unsigned long long bits = 0ull;
    sweep(it, 0, bits);
    const unsigned long long w = (__builtin_amdgcn_ballot_w64((bits & 1ull) != 0ull) ? 1ull : 0ull) |
                                 (__builtin_amdgcn_ballot_w64((bits >> 32) != 0ull) ? (1ull << 32) : 0ull);
    if ((tid & (kWave - 1)) == 0 && w) atomicOr(&slot[r3], w);
    if (tid == 0) slot[r3 == 2 ? 0 : r3 + 1] = 0ull;  // read two sweeps ago
    __syncthreads();
    const unsigned long long all = slot[r3];
    ++it;
    if (all >> 32) return IRLMX_NONFINITE;
    if (!(all & 1ull)) return IRLMX_OK;
    if (max_iter > 0 && it >= max_iter) return IRLMX_MAXITER;
  }
}

// ---------------------------------------------------------------------------
// the stopping rule, per-sweep shape
// ---------------------------------------------------------------------------

__device__ inline void block_max_to(unsigned long long v, unsigned long long* dst) {
  __shared__ unsigned long long red[kSweepThreads / kWave];
  v = wave_max_u64(v);
  const int wv = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) red[wv] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long m = 0;
    for (int i = 0; i < (int)(blockDim.x / kWave); ++i) m = red[i] > m ? red[i] : m;
    if (m) atomicMax(dst, m);
  }
}

// Common prologue: decides whether instance b converged after the previous
// sweep (`it` sweeps done so far); the first workgroup records the outcome.
__device__ inline bool sweep_should_stop(int b, long long it, int r3, double eps, long long max_iter,
                                         const Ws& ws, int32_t* status) {
  if (ws.done[b]) return true;
  if (it == 0) return false;
  const double prev = bits_double(ws.slots[b * 3 + (r3 == 0 ? 2 : r3 - 1)]);
  const bool cap = max_iter > 0 && it >= max_iter;
  if (prev > eps && !cap) return false;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ws.done[b] = 1;
    ws.iters[b] = it;
    status[b] = finish_status(prev, eps);
    atomicAdd(ws.ndone, 1);
  }
  return true;
}

// Host poll loop of the sweep shape: enqueue `chunk` sweeps, read the done
// counter, repeat.  Converged instances skip their sweeps, so over-enqueueing
// costs only empty launches.
template <typename LaunchOne>
static int run_until_done(const Ws& ws, int B, hipStream_t st, LaunchOne&& one) {
  long long it = 0;
  int r3 = 0;
  long long chunk = 32;
  for (;;) {
    for (long long c = 0; c < chunk; ++c) {
      one(it, r3);
      ++it;
      r3 = r3 == 2 ? 0 : r3 + 1;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "sweep launch");
    int32_t nd = 0;
    e = hipMemcpyAsync(&nd, ws.ndone, sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "poll");
    if (nd >= B) return 0;
    if (chunk < 4096) chunk *= 2;
  }
}

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
// The column form an ELL model's forward passes read: 0, or IRLMX_EINVAL and the message.
int need_col_form(const Model& m);

// Launch grid of the per-sweep kernels: kSweepThreads states per workgroup, one row per instance.
inline dim3 sweep_grid(const Model& m) { return dim3((m.S + kSweepThreads - 1) / kSweepThreads, m.B); }

// Slots per state a kernel compiles in for a model of K (5 / 8 / 16 / 32); 0 above `cap`.
constexpr int slot_class(int K, int cap) {
  const int k = K <= 5 ? 5 : (K <= 8 ? 8 : (K <= 16 ? 16 : (K <= 32 ? 32 : 0)));
  return k <= cap ? k : 0;
}

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
// (SPT, KMAX) pairs instantiated per op -- the one list fused_shape plans from
// and every kernel-pointer getter instantiates from (with_pair below; the
// extended and the horizon backward take IRLMX_OP_BACKWARD's): every pair listed compiles
// without VGPR spills at __launch_bounds__(1024) (tools/kernel_resources.py);
// the soft pass carries fp64 exp/log inline and so keeps fewer states per thread.
constexpr bool fused_pair_ok(int op, int spt, int kmax) {
  switch (op) {
    case IRLMX_OP_FORWARD:
    case IRLMX_OP_BACKWARD:
    case IRLMX_OP_POLICY_EVALUATION:  // (policy_eval.hip: the backward's register layout)
      return (kmax == 5 && spt <= 4) || (kmax == 8 && spt <= 2) || (kmax == 16 && spt <= 2) ||
             (kmax == 32 && spt == 1);
    case IRLMX_OP_SOFT_BACKWARD:
      return (kmax == 5 && spt <= 2) || (kmax == 8 && spt == 1) || (kmax == 16 && spt == 1);
    case IRLMX_OP_VALUE_ITERATION:
      return (kmax == 5 && spt <= 4) || (kmax == 8 && spt <= 4) || (kmax == 16 && spt == 1) ||
             (kmax == 32 && spt == 1);
    case IRLMX_OP_SOFT_BACKWARD_HORIZON:  // (soft_horizon.hip: rolled action loop, table re-read every step)
    case IRLMX_OP_VALUE_HORIZON:          // (the same skeleton and loops without exp / log)
      return (kmax == 5 && spt <= 4) || (kmax == 8 && spt <= 2) || (kmax == 16 && spt <= 2) ||
             (kmax == 32 && spt == 1);
  }
  return false;
}
// LDS of the ordinary fused kernels: two S-vectors, the convergence slots and
// run_deferred's block-start snapshot.
size_t fused_lds(const Model& m);

// f(integral_constant<int, SPT>, integral_constant<int, KMAX>) of the pair
// (spt, kmax) out of SPT in {1, 2, 4} x KMAX in {5, 8, 16, 32}; a null R for any
// other pair.  A kernel family's getter is one generic lambda that returns
// &kernel<SPT, KMAX> where its constexpr predicate admits the pair and nullptr
// (under `if constexpr`) where not: the predicate is the instantiation list.
template <class R, class F>
R with_pair(int spt, int kmax, F&& f) {
  R r = nullptr;
  auto at = [&](auto s, auto k) {
    if (spt == s && kmax == k) r = f(s, k);
  };
  auto row = [&](auto k) {
    at(std::integral_constant<int, 1>{}, k);
    at(std::integral_constant<int, 2>{}, k);
    at(std::integral_constant<int, 4>{}, k);
  };
  row(std::integral_constant<int, 5>{});
  row(std::integral_constant<int, 8>{});
  row(std::integral_constant<int, 16>{});
  row(std::integral_constant<int, 32>{});
  return r;
}

// One workgroup of `threads` per instance with `lds` bytes of dynamic LDS: 0, or
// hip_fail's code (`name` names the kernel in the launch's error text).
int launch_fused_kernel(const void* kfn, const char* name, int B, int threads, size_t lds, hipStream_t st, void* args);
template <class Args>
int launch_fused(void (*kfn)(Args), const char* name, int B, int threads, size_t lds, hipStream_t st, Args a) {
  return launch_fused_kernel((const void*)kfn, name, B, threads, lds, st, &a);
}

// Plan rows (irlmx_execution_plan's columns) of the two shapes every pass has.
void plan_fused(int64_t* plan, const FusedShape& fs, size_t lds);
void plan_sweep(int64_t* plan, int states_per_lane, int64_t launches);

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

// Policy evaluation (policy_eval.hip): whether this model is one it runs (else
// IRLMX_EINVAL and the message, prefixed by `fn`).
int policy_eval_check_model(const Model& m, const char* fn);

// The finite-horizon passes (horizon.hip, soft_horizon.hip; the rest of their
// host side is horizon.h): whether this model is one they run (else
// IRLMX_EINVAL and the message, prefixed by `fn`), their workspace and plan.
inline bool horizon_op(int op) {
  return op == IRLMX_OP_BACKWARD_HORIZON || op == IRLMX_OP_FORWARD_HORIZON || op == IRLMX_OP_SOFT_BACKWARD_HORIZON ||
         op == IRLMX_OP_VALUE_HORIZON;
}
int horizon_check_model(const Model& m, const char* fn);
size_t horizon_workspace_bytes(const Model& m, int op);
void horizon_plan(const Model& m, int op, int64_t* plan);
// Several states per thread run fused only from this many instances on (one
// workgroup per CU; IRLMX_HORIZON_FUSED_BATCH).
int horizon_fused_min_batch();

}  // namespace irlmx

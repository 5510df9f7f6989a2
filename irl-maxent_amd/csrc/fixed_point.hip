// Fixed-point sweeps of the MaxEnt-IRL inner loop on gfx950.
//
//   backward  (maxent.py:119-159)  zs <- exp(r) * sum_a P_a zs, 2*S sweeps, then za/zs
//   forward   (maxent.py:63-114)   d  <- p0 + sum_a P'_a^T (pi_a * d) until max|dd| <= eps
//   soft VI   (maxent.py:279-341)  v  <- fold_a softmax(v, r + g P_a v) until max|dv| <= eps
//   VI        (solver.py:9-104)    v  <- r + max_a / mean_a (g P_a v) until max|dv| <= eps
//
// Here: the C entry points of the four passes, route() -- the one place that
// decides a call's execution shape, read by the workspace carving, the reported
// plan and the entry points alike -- and the two shapes every layout can take:
//
//  * fused: one workgroup owns one instance for the WHOLE loop.  The two
//    ping-pong state vectors live in LDS (2*S*8 B <= 64 KiB at S = 4096), each
//    thread keeps the weights and neighbour indices of its SPT states in
//    registers, and a sweep costs one workgroup barrier: the convergence test
//    max|new - old| is a wave shuffle-max plus one LDS atomic max into a
//    3-slot ring, so there is no host round trip until the loop has converged.
//  * sweep: S too large for one CU.  One launch per sweep over all B
//    instances; vectors in HBM, per-instance max|delta| by one global atomic
//    per workgroup into a 3-slot ring, and a per-instance done flag that
//    freezes an instance once converged, so the host can enqueue sweeps in
//    chunks and only polls a done counter between chunks.
//
// The convergence word is the raw bits of |x| as uint64: for non-negative
// doubles integer order is numeric order and NaN sorts above +inf, so the
// integer max reproduces np.max(np.abs(.)) including NaN propagation, and
// `!(delta > eps)` stops on NaN exactly like the reference's `while delta > eps`.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <functional>

#include "cluster.h"
#include "dense.h"
#include "grid.h"
#include "numpy_order.h"

namespace irlmx {

int fused_max_states() {
  const char* e = getenv("IRLMX_FUSED_MAX_STATES");
  if (!e || !*e) return kFusedMaxStates;
  const int v = atoi(e);
  return v < kFusedMaxStates ? v : kFusedMaxStates;
}

// ---------------------------------------------------------------------------
// weight preparation
// ---------------------------------------------------------------------------

// Gather weights of the forward pass, one per (target t, slot k):
//   w[k][t] = sum_a P[s, t, a] * pi[s, a]  over non-terminal sources s = src_k(t)
// (P' of maxent.py:98-99 has the terminal rows cleared).  Any non-finite
// policy entry makes the reference's dense dgemv return NaN everywhere after
// one sweep (0 * NaN inside the dot), so such instances are flagged in `bad`.
__global__ void fwd_weights_kernel(Model m, const double* __restrict__ pi,
                                   const uint8_t* __restrict__ term, double* __restrict__ w,
                                   int32_t* __restrict__ bad) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (t >= m.S) return;
  const int S = m.S, A = m.A;
  const double* pib = pi + (size_t)b * S * A;
  const uint8_t* tb = term + (size_t)b * S;
  bool nonfinite = false;
  for (int a = 0; a < A; ++a) nonfinite |= !isfinite(pib[(size_t)t * A + a]);
  for (int k = 0; k < m.Kc; ++k) {
    double acc = 0.0;
    if (m.stencil) {
      if (stencil_valid(t, k, m.W, m.H)) {
        const int s = stencil_nbr(t, k, m.W, m.H);
        const int kk = stencil_opposite(k);  // direction from s back to t
        if (!tb[s])
          for (int a = 0; a < A; ++a) acc = fma(row_val(m, b, a, kk, s), pib[(size_t)s * A + a], acc);
      }
    } else {
      const int s = col_src(m, b, t, k);
      if (!tb[s]) {
        const size_t base = inst_of(m, b) * A;
        for (int a = 0; a < A; ++a)
          acc = fma(m.col_val[((base + a) * m.Kc + k) * S + t], pib[(size_t)s * A + a], acc);
      }
    }
    w[((size_t)b * m.Kc + k) * S + t] = acc;
  }
  if (nonfinite) atomicOr(&bad[b], 1);
}

// bwd_nonfinite_rule.  The reference's backward product is dense (maxent.py:155:
// P_a.dot(zs) over all S columns), so one non-finite partition value makes
// 0 * inf = NaN appear in every row within a sweep, and the returned policy is
// NaN everywhere.  The compact products here touch only stored neighbours, so
// every shape records "some zs value of the 2S - 1 collapsed sweeps was
// non-finite" (fused and sweep shapes: per sweep) and then writes NaN for the
// whole instance.  With rescaling on, values turn non-finite only through
// non-finite weights (a reward of +inf or NaN), which bwd_weights_kernel flags
// (the cluster shape fills such instances with NaN after its sweeps,
// bwd_nan_fill_kernel); calls without rescaling (the reference's overflow) do
// not run on the cluster shape.
// Collapsed, reward-folded backward weights of instance b:
//   w[b][k][s] = exp(r[b][s]) * sum_a P[s, target_k(s), a]
// so one backward sweep is zs'[s] = sum_k w[b][k][s] * zs[target_k(s)]
// (maxent.py:155-156 with the action sum and exp(r) taken out of the loop).
// Every shape (fused, sweep, cluster) uses these same weights in the same
// order, so the shapes stay bit-identical to each other.
__global__ void bwd_weights_kernel(Model m, const double* __restrict__ reward, double* __restrict__ w,
                                   int32_t* __restrict__ bad) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (s >= m.S) return;
  const size_t bi = m.shared ? 0 : (size_t)b;  // table instance
  const double er = exp(reward[(size_t)b * m.S + s]);
  bool nf = false;
  for (int k = 0; k < m.K; ++k) {
    double acc = 0.0;
    for (int a = 0; a < m.A; ++a)
      acc += m.row_val[((bi * m.A + a) * m.K + k) * m.S + s];
    const double wk = __dmul_rn(er, acc);
    nf |= !isfinite(wk);
    w[((size_t)b * m.K + k) * m.S + s] = wk;
  }
  // non-finite weights make some partition value non-finite within two sweeps,
  // and the reference's dense product then NaN everywhere (bwd_nonfinite_rule)
  if (nf) atomicOr(&bad[b], 1);
}

void bwd_weights_launch(const Model& m, const double* reward, double* w, int32_t* bad, hipStream_t st) {
  hipLaunchKernelGGL(bwd_weights_kernel, sweep_grid(m), dim3(kSweepThreads), 0, st, m, reward, w, bad);
}

// bwd_nonfinite_rule for the cluster shape: NaN policy for flagged instances
__global__ void bwd_nan_fill_kernel(Model m, const int32_t* __restrict__ bad, double* __restrict__ pi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (i < m.S * m.A && bad[b]) pi[(size_t)b * m.S * m.A + i] = kNaN;
}

// ---------------------------------------------------------------------------
// fused (one workgroup per instance) kernels
// ---------------------------------------------------------------------------

struct FwdArgs {
  Model m;
  const double* w;  // [B][Kc][S]
  const int32_t* bad;
  const double* p0;
  double eps;
  long long max_iter;
  double* out;
  int64_t* iters;
  int32_t* status;
};

// one barrier per sweep; LDS: two S-vectors + 3 convergence slots
template <int SPT, int KMAX>
__global__ void __launch_bounds__(1024) fwd_fused_kernel(FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Model& m = a.m;
  const int S = m.S, K = m.Kc;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  double* bufA = (double*)smem;
  double* bufB = bufA + S;
  unsigned long long* slot = (unsigned long long*)(bufB + S);
  double* snap = (double*)(slot + 4);  // run_deferred's block-start state (LDS: the registers are taken)

  if (a.bad[b]) {  // non-finite policy: the reference yields NaN after one sweep
    for (int s = tid; s < S; s += nt) a.out[(size_t)b * S + s] = __longlong_as_double(0x7ff8000000000000LL);
    if (tid == 0) { a.iters[b] = 1; a.status[b] = IRLMX_NONFINITE; }
    return;
  }

  double w[SPT][KMAX];
  int nb[SPT][KMAX];
  double p0[SPT], cur[SPT];
  const double* wb = a.w + (size_t)b * K * S;
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tid + j * nt;
    cur[j] = 0.0;
    p0[j] = 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) { w[j][k] = 0.0; nb[j][k] = 0; }
    if (s < S) {
      p0[j] = a.p0[(size_t)b * S + s];
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) { w[j][k] = wb[(size_t)k * S + s]; nb[j][k] = col_src(m, b, s, k); }
    }
  }
  for (int s = tid; s < S; s += nt) bufA[s] = 0.0;
  if (tid < 3) slot[tid] = 0ull;
  __syncthreads();

  long long it = 0;
  auto sweep = [&](long long it, int pos, unsigned long long& bits) __attribute__((always_inline)) {
    const double* din = (it & 1) ? bufB : bufA;
    double* dout = (it & 1) ? bufA : bufB;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int s = tid + j * nt;
      if (s < S) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (k < K) acc = fma(w[j][k], din[nb[j][k]], acc);
        const double nv = p0[j] + acc;
        dout[s] = nv;
        record_delta(bits, pos, fabs(nv - cur[j]), a.eps);
        cur[j] = nv;
      }
    }
  };
  // (the widest ELL rows fill the registers: the per-sweep reduction there)
  int status;
  if constexpr (SPT * KMAX < 32) {
    status = run_deferred(
        a.max_iter, slot, it, sweep,
        [&]() {
#pragma unroll
          for (int j = 0; j < SPT; ++j)
            if (tid + j * nt < S) snap[tid + j * nt] = cur[j];
        },
        [&]() {
          double* d0 = (it & 1) ? bufB : bufA;
#pragma unroll
          for (int j = 0; j < SPT; ++j)
            if (tid + j * nt < S) d0[tid + j * nt] = cur[j] = snap[tid + j * nt];
          __syncthreads();
        });
  } else {
    // the per-sweep max reduction (these kernels sit at the register limit)
    int r3 = 0;
    double delta = 0.0;
    for (;;) {
      const double* din = (it & 1) ? bufB : bufA;
      double* dout = (it & 1) ? bufA : bufB;
      unsigned long long mx = 0ull;
#pragma unroll
      for (int j = 0; j < SPT; ++j) {
        const int s = tid + j * nt;
        if (s < S) {
          double acc = 0.0;
#pragma unroll
          for (int k = 0; k < KMAX; ++k)
            if (k < K) acc = fma(w[j][k], din[nb[j][k]], acc);
          const double nv = p0[j] + acc;
          dout[s] = nv;
          const unsigned long long d = abs_bits(nv - cur[j]);
          mx = d > mx ? d : mx;
          cur[j] = nv;
        }
      }
      mx = wave_max_u64(mx);
      if ((tid & (kWave - 1)) == 0 && mx) atomicMax(&slot[r3], mx);
      if (tid == 0) slot[r3 == 2 ? 0 : r3 + 1] = 0ull;
      __syncthreads();
      delta = bits_double(slot[r3]);
      r3 = r3 == 2 ? 0 : r3 + 1;
      ++it;
      if (!(delta > a.eps)) break;
      if (a.max_iter > 0 && it >= a.max_iter) break;
    }
    status = finish_status(delta, a.eps);
  }
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tid + j * nt;
    if (s < S) a.out[(size_t)b * S + s] = cur[j];
  }
  if (tid == 0) { a.iters[b] = it; a.status[b] = status; }
}

struct BwdArgs {
  Model m;
  const double* w;  // [B][K][S] collapsed, reward-folded weights
  const double* reward;
  const uint8_t* term;
  int rescale;
  double* pi;  // [B][S][A]
  int32_t* status;
};

template <int SPT, int KMAX>
__global__ void __launch_bounds__(1024) bwd_fused_kernel(BwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Model& m = a.m;
  const int S = m.S, K = m.K, A = m.A;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  double* bufA = (double*)smem;
  double* bufB = bufA + S;
  unsigned long long* slot = (unsigned long long*)(bufB + S);

  double w[SPT][KMAX];
  int nb[SPT][KMAX];
  const double* wb = a.w + (size_t)b * K * S;
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tid + j * nt;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) { w[j][k] = 0.0; nb[j][k] = 0; }
    if (s < S) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) { w[j][k] = wb[(size_t)k * S + s]; nb[j][k] = row_nbr(m, b, s, k); }
    }
  }
  for (int s = tid; s < S; s += nt) bufA[s] = a.term[(size_t)b * S + s] ? 1.0 : 0.0;
  if (tid < 3) slot[tid] = 0ull;
  __syncthreads();

  // 2*S sweeps in all (maxent.py:154): the first 2*S - 1 on the action-summed
  // table, the last one per action because it also produces za.
  const long long collapsed = 2LL * S - 1;
  int e = 0, r3 = 0;
  bool nf = false;  // some partition value went non-finite (see bwd_nonfinite_rule)
  for (long long it = 0; it < collapsed; ++it) {
    const double* din = (it & 1) ? bufB : bufA;
    double* dout = (it & 1) ? bufA : bufB;
    if (a.rescale && it > 0) e = rescale_exponent(bits_double(slot[r3 == 0 ? 2 : r3 - 1]));
    unsigned long long mx = 0ull;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int s = tid + j * nt;
      if (s < S) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (k < K) acc = fma(w[j][k], din[nb[j][k]], acc);
        const double nv = ldexp(acc, e);
        dout[s] = nv;
        const unsigned long long d = abs_bits(nv);
        mx = d > mx ? d : mx;
        nf |= !isfinite(nv);
      }
    }
    if (a.rescale) {
      mx = wave_max_u64(mx);
      if ((tid & (kWave - 1)) == 0 && mx) atomicMax(&slot[r3], mx);
      if (tid == 0) slot[r3 == 2 ? 0 : r3 + 1] = 0ull;
    }
    __syncthreads();
    r3 = r3 == 2 ? 0 : r3 + 1;
  }
  const double* zs = (collapsed & 1) ? bufB : bufA;
  if (a.rescale && collapsed > 0) e = rescale_exponent(bits_double(slot[r3 == 0 ? 2 : r3 - 1]));
  const bool all_nan = __syncthreads_or(nf);
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tid + j * nt;
    if (s < S && all_nan) {
      for (int act = 0; act < A; ++act) a.pi[((size_t)b * S + s) * A + act] = kNaN;
    } else if (s < S) {
      const double er = exp(a.reward[(size_t)b * S + s]);
      double za[kMaxActions];
      double zsum = 0.0;
      for (int act = 0; act < A; ++act) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (k < K) acc = fma(row_val(m, b, act, k, s), zs[nb[j][k]], acc);
        za[act] = ldexp(__dmul_rn(er, acc), e);  // rounded product, then the sum (maxent.py:155-156)
        zsum = __dadd_rn(zsum, za[act]);
      }
      for (int act = 0; act < A; ++act) a.pi[((size_t)b * S + s) * A + act] = za[act] / zsum;
    }
  }
  if (tid == 0) a.status[b] = IRLMX_OK;
}

// per-state Bellman update shared by the fused and the sweep shapes.
// NB: neighbour lookup; CACHED uses the per-thread register copy.
template <bool SOFT, int KMAX, bool CACHED>
__device__ inline double bellman_update(const SoftArgs& a, int b, int s, const int* nb,
                                        const double* vin, double r, double phi) {
  const Model& m = a.m;
  const int K = m.K, A = m.A;
  double v = SOFT ? phi : 0.0;
#pragma unroll 1
  for (int act = 0; act < A; ++act) {
    double dot = 0.0;
    if (CACHED) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) dot = fma(row_val(m, b, act, k, s), vin[nb[k]], dot);
    } else {
      for (int k = 0; k < K; ++k) dot = fma(row_val(m, b, act, k, s), vin[row_nbr(m, b, s, k)], dot);
    }
    if (SOFT) {
      v = softmax2(v, __dadd_rn(r, __dmul_rn(a.discount, dot)));  // maxent.py:329-333
    } else {
      const double q = __dmul_rn(a.discount, dot);  // solver.py:44
      if (a.average) v = act == 0 ? q : __dadd_rn(v, q);
      else v = act == 0 ? q : ((v != v || q <= v) ? v : q);
    }
  }
  if (!SOFT) v = __dadd_rn(r, a.average ? v / (double)A : v);  // solver.py:47 / :99
  return v;
}

template <int KMAX, bool CACHED>
__device__ inline void soft_policy_row(const SoftArgs& a, int b, int s, const int* nb,
                                       const double* vold, double vnew, double r) {
  const Model& m = a.m;
#pragma unroll 1
  for (int act = 0; act < m.A; ++act) {
    double dot = 0.0;
    if (CACHED) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < m.K) dot = fma(row_val(m, b, act, k, s), vold[nb[k]], dot);
    } else {
      for (int k = 0; k < m.K; ++k) dot = fma(row_val(m, b, act, k, s), vold[row_nbr(m, b, s, k)], dot);
    }
    const double q = __dadd_rn(r, __dmul_rn(a.discount, dot));
    a.pi[((size_t)b * m.S + s) * m.A + act] = np_exp(q - vnew);  // maxent.py:341
  }
}

template <bool SOFT, int SPT, int KMAX>
__device__ __forceinline__ void bellman_fused_body(const SoftArgs& a, unsigned char* smem) {
  const Model& m = a.m;
  const int S = m.S, K = m.K;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  double* bufA = (double*)smem;
  double* bufB = bufA + S;
  unsigned long long* slot = (unsigned long long*)(bufB + S);
  double* snap = (double*)(slot + 4);  // run_deferred's block-start state (LDS: the registers are taken)

  int nb[SPT][KMAX];
  double r[SPT], phi[SPT], cur[SPT];
  const double v0 = SOFT ? -1e200 : 0.0;  // maxent.py:323 / solver.py:32
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tid + j * nt;
    r[j] = 0.0;
    phi[j] = 0.0;
    cur[j] = v0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) nb[j][k] = 0;
    if (s < S) {
      r[j] = a.reward[(size_t)b * S + s];
      if (SOFT) phi[j] = a.phi[(size_t)b * S + s];
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) nb[j][k] = row_nbr(m, b, s, k);
    }
  }
  for (int s = tid; s < S; s += nt) bufA[s] = v0;
  if (tid < 3) slot[tid] = 0ull;
  __syncthreads();

  long long it = 0;
  auto sweep = [&](long long it, int pos, unsigned long long& bits) __attribute__((always_inline)) {
    const double* vin = (it & 1) ? bufB : bufA;
    double* vout = (it & 1) ? bufA : bufB;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int s = tid + j * nt;
      if (s < S) {
        const double v = bellman_update<SOFT, KMAX, true>(a, b, s, nb[j], vin, r[j], phi[j]);
        vout[s] = v;
        record_delta(bits, pos, fabs(v - cur[j]), a.eps);
        cur[j] = v;
      }
    }
  };
  // (VI converges in tens of sweeps, where a block's overshoot and replay cost
  // more than a reduction per sweep; the widest rows fill the registers: per-
  // sweep bits there too)
  int status;
  if constexpr (SOFT && SPT * KMAX < 32) {
    status = run_deferred(
        a.max_iter, slot, it, sweep,
        [&]() {
#pragma unroll
          for (int j = 0; j < SPT; ++j)
            if (tid + j * nt < S) snap[tid + j * nt] = cur[j];
        },
        [&]() {
          double* v0w = (it & 1) ? bufB : bufA;
#pragma unroll
          for (int j = 0; j < SPT; ++j)
            if (tid + j * nt < S) v0w[tid + j * nt] = cur[j] = snap[tid + j * nt];
          __syncthreads();
        });
  } else {
    status = run_each(a.max_iter, slot, it, sweep);
  }
  const double* vold = (it & 1) ? bufA : bufB;  // input of the last sweep
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tid + j * nt;
    if (s < S) {
      if (a.value) a.value[(size_t)b * S + s] = cur[j];
      if (SOFT) soft_policy_row<KMAX, true>(a, b, s, nb[j], vold, cur[j], r[j]);
    }
  }
  if (tid == 0) {
    if (a.iters) a.iters[b] = it;
    a.status[b] = status;
  }
}

template <int SPT, int KMAX>
__global__ void __launch_bounds__(1024) soft_fused_kernel(SoftArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bellman_fused_body<true, SPT, KMAX>(a, smem);
}

template <int SPT, int KMAX>
__global__ void __launch_bounds__(1024) vi_fused_kernel(SoftArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  bellman_fused_body<false, SPT, KMAX>(a, smem);
}

// ---------------------------------------------------------------------------
// sweep (one launch per sweep, all instances) kernels
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(kSweepThreads)
fwd_sweep_kernel(FwdArgs a, Ws ws, long long it, int r3) {
  const Model& m = a.m;
  const int b = blockIdx.y;
  if (ws.bad[b]) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && !ws.done[b]) {
      ws.done[b] = 1; ws.iters[b] = 1; a.status[b] = IRLMX_NONFINITE; atomicAdd(ws.ndone, 1);
    }
    return;
  }
  if (sweep_should_stop(b, it, r3, a.eps, a.max_iter, ws, a.status)) return;
  const int S = m.S;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const double* din = ((it & 1) ? ws.buf1 : ws.buf0) + (size_t)b * S;
  double* dout = ((it & 1) ? ws.buf0 : ws.buf1) + (size_t)b * S;
  unsigned long long d = 0ull;
  if (s < S) {
    const double* wb = a.w + (size_t)b * m.Kc * S;
    double acc = 0.0;
    for (int k = 0; k < m.Kc; ++k) acc = fma(wb[(size_t)k * S + s], din[col_src(m, b, s, k)], acc);
    const double nv = a.p0[(size_t)b * S + s] + acc;
    dout[s] = nv;
    d = abs_bits(nv - din[s]);
  }
  block_max_to(d, &ws.slots[b * 3 + r3]);
  if (blockIdx.x == 0 && threadIdx.x == 0) ws.slots[b * 3 + (r3 == 2 ? 0 : r3 + 1)] = 0ull;
}

__global__ void fwd_finish_kernel(FwdArgs a, Ws ws) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  const int S = a.m.S;
  if (s >= S) return;
  double v;
  if (ws.bad[b]) v = __longlong_as_double(0x7ff8000000000000LL);
  else v = ((ws.iters[b] & 1) ? ws.buf1 : ws.buf0)[(size_t)b * S + s];
  a.out[(size_t)b * S + s] = v;
  if (s == 0) a.iters[b] = ws.iters[b];
}

__global__ void __launch_bounds__(kSweepThreads)
bwd_sweep_kernel(BwdArgs a, Ws ws, long long it, int r3) {
  const Model& m = a.m;
  const int S = m.S;
  const int b = blockIdx.y;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const double* din = ((it & 1) ? ws.buf1 : ws.buf0) + (size_t)b * S;
  double* dout = ((it & 1) ? ws.buf0 : ws.buf1) + (size_t)b * S;
  int e = 0;
  if (a.rescale && it > 0) e = rescale_exponent(bits_double(ws.slots[b * 3 + (r3 == 0 ? 2 : r3 - 1)]));
  unsigned long long d = 0ull;
  if (s < S) {
    const double* wb = a.w + (size_t)b * m.K * S;
    double acc = 0.0;
    for (int k = 0; k < m.K; ++k) acc = fma(wb[(size_t)k * S + s], din[row_nbr(m, b, s, k)], acc);
    const double nv = ldexp(acc, e);
    dout[s] = nv;
    d = abs_bits(nv);
    if (!isfinite(nv)) atomicOr(&ws.bad[b], 1);  // bwd_nonfinite_rule
  }
  if (a.rescale) {
    block_max_to(d, &ws.slots[b * 3 + r3]);
    if (blockIdx.x == 0 && threadIdx.x == 0) ws.slots[b * 3 + (r3 == 2 ? 0 : r3 + 1)] = 0ull;
  }
}

__global__ void bwd_init_kernel(BwdArgs a, Ws ws) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (s >= a.m.S) return;
  ws.buf0[(size_t)b * a.m.S + s] = a.term[(size_t)b * a.m.S + s] ? 1.0 : 0.0;
}

__global__ void bwd_final_kernel(BwdArgs a, Ws ws, long long collapsed, int r3) {
  const Model& m = a.m;
  const int S = m.S, A = m.A;
  const int b = blockIdx.y;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  if (ws.bad[b]) {  // bwd_nonfinite_rule
    for (int act = 0; act < A; ++act) a.pi[((size_t)b * S + s) * A + act] = kNaN;
    if (s == 0) a.status[b] = IRLMX_OK;
    return;
  }
  const double* zs = ((collapsed & 1) ? ws.buf1 : ws.buf0) + (size_t)b * S;
  int e = 0;
  if (a.rescale && collapsed > 0) e = rescale_exponent(bits_double(ws.slots[b * 3 + (r3 == 0 ? 2 : r3 - 1)]));
  const double er = exp(a.reward[(size_t)b * S + s]);
  double za[kMaxActions];
  double zsum = 0.0;
  for (int act = 0; act < A; ++act) {
    double acc = 0.0;
    for (int k = 0; k < m.K; ++k) acc = fma(row_val(m, b, act, k, s), zs[row_nbr(m, b, s, k)], acc);
    za[act] = ldexp(__dmul_rn(er, acc), e);
    zsum = __dadd_rn(zsum, za[act]);
  }
  for (int act = 0; act < A; ++act) a.pi[((size_t)b * S + s) * A + act] = za[act] / zsum;
  if (s == 0) a.status[b] = IRLMX_OK;
}

template <bool SOFT>
__global__ void __launch_bounds__(kSweepThreads)
bellman_sweep_kernel(SoftArgs a, Ws ws, long long it, int r3) {
  const Model& m = a.m;
  const int b = blockIdx.y;
  if (sweep_should_stop(b, it, r3, a.eps, a.max_iter, ws, a.status)) return;
  const int S = m.S;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const double* vin = ((it & 1) ? ws.buf1 : ws.buf0) + (size_t)b * S;
  double* vout = ((it & 1) ? ws.buf0 : ws.buf1) + (size_t)b * S;
  unsigned long long d = 0ull;
  if (s < S) {
    const double r = a.reward[(size_t)b * S + s];
    const double phi = SOFT ? a.phi[(size_t)b * S + s] : 0.0;
    const double v = bellman_update<SOFT, 1, false>(a, b, s, nullptr, vin, r, phi);
    vout[s] = v;
    d = abs_bits(v - vin[s]);
  }
  block_max_to(d, &ws.slots[b * 3 + r3]);
  if (blockIdx.x == 0 && threadIdx.x == 0) ws.slots[b * 3 + (r3 == 2 ? 0 : r3 + 1)] = 0ull;
}

template <bool SOFT>
__global__ void bellman_finish_kernel(SoftArgs a, Ws ws) {
  const Model& m = a.m;
  const int S = m.S;
  const int b = blockIdx.y;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const long long it = ws.iters[b];
  const double* vnew = ((it & 1) ? ws.buf1 : ws.buf0) + (size_t)b * S;
  const double* vold = ((it & 1) ? ws.buf0 : ws.buf1) + (size_t)b * S;
  if (a.value) a.value[(size_t)b * S + s] = vnew[s];
  if (SOFT) soft_policy_row<1, false>(a, b, s, nullptr, vold, vnew[s], a.reward[(size_t)b * S + s]);
  if (s == 0 && a.iters) a.iters[b] = it;
}

__global__ void fill_kernel(double* p, size_t n, double v) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// ---------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------

bool fused_shape(const Model& m, int op, FusedShape* out, bool cluster_first) {
  if (m.dense || m.S > fused_max_states() || m.A > kMaxActions) return false;
  // Grids of width 64 / 128 run the forward and backward passes on the cluster
  // shape even when they fit one CU: its register-resident pair layouts sweep
  // 4-5x faster than the general-sparsity fused kernel, and a single instance
  // then spreads over several CUs (cluster.hip).
  if (cluster_first && (op == IRLMX_OP_FORWARD || op == IRLMX_OP_BACKWARD) && m.stencil &&
      (m.W == 64 || m.W == 128) && env_int("IRLMX_CLUSTER", 1) != 0)
    return false;
  const int K = op == IRLMX_OP_FORWARD ? m.Kc : m.K;
  const int kmax = slot_class(K, 32);
  if (!kmax) return false;
  int spt = 1;
  while ((m.S + spt - 1) / spt > 1024) spt *= 2;
  if (!fused_pair_ok(op, spt, kmax)) return false;
  const int per = (m.S + spt - 1) / spt;
  out->spt = spt;
  out->kmax = kmax;
  out->threads = std::min(1024, ((per + kWave - 1) / kWave) * kWave);
  return true;
}

// two S-vectors, the convergence slots and (run_deferred) the block-start snapshot
size_t fused_lds(const Model& m) { return 3 * (size_t)m.S * sizeof(double) + 4 * sizeof(unsigned long long); }

// Kernel-pointer getters: fused_pair_ok() is each one's instantiation list (with_pair).
static void (*fwd_fused_fn(const FusedShape& f))(FwdArgs) {
  return with_pair<void (*)(FwdArgs)>(f.spt, f.kmax, [](auto s, auto k) {
    if constexpr (fused_pair_ok(IRLMX_OP_FORWARD, s, k)) return &fwd_fused_kernel<s, k>;
    else return nullptr;
  });
}
static void (*bwd_fused_fn(const FusedShape& f))(BwdArgs) {
  return with_pair<void (*)(BwdArgs)>(f.spt, f.kmax, [](auto s, auto k) {
    if constexpr (fused_pair_ok(IRLMX_OP_BACKWARD, s, k)) return &bwd_fused_kernel<s, k>;
    else return nullptr;
  });
}
static void (*bellman_fused_fn(bool soft, const FusedShape& f))(SoftArgs) {
  if (soft)
    return with_pair<void (*)(SoftArgs)>(f.spt, f.kmax, [](auto s, auto k) {
      if constexpr (fused_pair_ok(IRLMX_OP_SOFT_BACKWARD, s, k)) return &soft_fused_kernel<s, k>;
      else return nullptr;
    });
  return with_pair<void (*)(SoftArgs)>(f.spt, f.kmax, [](auto s, auto k) {
    if constexpr (fused_pair_ok(IRLMX_OP_VALUE_ITERATION, s, k)) return &vi_fused_kernel<s, k>;
    else return nullptr;
  });
}

// The fused shape's launch of an ordinary pass (`name` names it in a launch error).
template <class Args>
static int run_fused(void (*kfn)(Args), const char* name, const Model& m, const FusedShape& f, hipStream_t st,
                     const Args& a) {
  if (!kfn) { set_error("no fused kernel for spt=%d kmax=%d", f.spt, f.kmax); return IRLMX_EINVAL; }
  return launch_fused(kfn, name, m.B, f.threads, fused_lds(m), st, a);
}

int launch_fused_kernel(const void* kfn, const char* name, int B, int threads, size_t lds, hipStream_t st, void* args) {
  if (hipError_t e = hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return hip_fail(e, "hipFuncSetAttribute");
  (void)hipLaunchKernel(kfn, dim3(B), dim3(threads), &args, lds, st);  // `args`: the kernel's one parameter
  const hipError_t e = hipGetLastError();  // this launch's, or an earlier unchecked one's of the same call
  return e == hipSuccess ? 0 : hip_fail(e, name);
}

void plan_fused(int64_t* plan, const FusedShape& fs, size_t lds) {
  plan[0] = IRLMX_SHAPE_FUSED;
  plan[5] = fs.spt;
  plan[7] = fs.threads;
  plan[8] = 1;
  plan[9] = (int64_t)lds;
}

void plan_sweep(int64_t* plan, int states_per_lane, int64_t launches) {
  plan[0] = IRLMX_SHAPE_SWEEP;
  plan[5] = states_per_lane;
  plan[7] = kSweepThreads;
  plan[8] = launches;
}

int validate(const irlmx_mdp* mdp) {
  if (!mdp) { set_error("mdp is NULL"); return IRLMX_EINVAL; }
  const Model m = make_model(mdp);
  if (m.S <= 0 || m.A <= 0 || m.B <= 0) { set_error("bad sizes S=%d A=%d B=%d", m.S, m.A, m.B); return IRLMX_EINVAL; }
  if (m.A > kMaxActions) { set_error("n_actions=%d exceeds %d", m.A, kMaxActions); return IRLMX_EINVAL; }
  if (!m.row_val) { set_error("row_val is NULL"); return IRLMX_EINVAL; }
  if (m.stencil) {
    if (m.W <= 0 || m.H <= 0 || (long long)m.W * m.H != m.S) {
      set_error("stencil grid %dx%d != %d states", m.W, m.H, m.S);
      return IRLMX_EINVAL;
    }
  } else if (mdp->layout == IRLMX_LAYOUT_ELL) {
    if (!m.row_idx || m.K <= 0) { set_error("ELL row form missing"); return IRLMX_EINVAL; }
    if (m.K > m.S) { set_error("ELL k_row=%d out of range (1..%d)", m.K, m.S); return IRLMX_EINVAL; }
  } else if (m.dense) {
    if (!m.col_val) { set_error("DENSE action-summed rows (col_val) missing"); return IRLMX_EINVAL; }
    if ((long long)m.S * m.S * m.A > (1LL << 40)) { set_error("DENSE table too large (S=%d)", m.S); return IRLMX_EINVAL; }
  } else {
    set_error("unknown layout %d", mdp->layout);
    return IRLMX_EINVAL;
  }
  return 0;
}

int need_all(const char* fn, std::initializer_list<Arg> args) {
  for (const Arg& a : args)
    if (a.name && !a.p) {
      set_error("%s: %s is NULL", fn, a.name);
      return IRLMX_EINVAL;
    }
  return 0;
}

int need_col_form(const Model& m) {
  if (m.stencil || m.dense) return 0;
  if (!m.col_idx || !m.col_val || m.Kc <= 0) { set_error("ELL column form missing"); return IRLMX_EINVAL; }
  if (m.Kc > m.S) { set_error("ELL k_col=%d out of range (1..%d)", m.Kc, m.S); return IRLMX_EINVAL; }
  return 0;
}

int check_ws(size_t need, size_t bytes, void* ws) {
  if (bytes < need || (need && !ws)) {
    set_error("workspace too small: need %zu bytes, got %zu", need, bytes);
    return IRLMX_EWORKSPACE;
  }
  return 0;
}

int check_ws(const Model& m, int op, size_t bytes, void* ws) { return check_ws(carve(m, op, nullptr).total, bytes, ws); }

// ---------------------------------------------------------------------------
// dense-row path (dense.hip)
// ---------------------------------------------------------------------------

static DenseView dense_view(const Model& m) { return DenseView{m.S, m.A, m.B, m.shared, m.row_val, m.col_val}; }

static DenseBufs dense_bufs(const Ws& ws) {
  return DenseBufs{ws.buf0, ws.buf1, ws.slots, ws.done, ws.iters, ws.ndone, ws.bad, ws.wgt};
}

// Shared table, B instances: the collapsed backward sweep is the GEMM
// M [S x S] . ZS [S x B].  Measured on MI355X (tools/diag/dense_bench.py,
// profiles/r02_dense_gemm_bench.txt, microseconds per sweep):
//
//            streaming (VALU)      hand-written fp64 MFMA     rocBLAS dgemm (round 2, since dropped)
//   S=2048   B=4 16  B=16 40  B=64 112   16 / 19 / 43           117 / 117 / 117
//   S=4096   B=4 81  B=16 303 B=64 1227  29 / 34 / 80           447 / 448 / 450
//
// Streaming re-reads M from the 256 MB last-level cache, so it wins for few
// instances while M is small; the MFMA kernel (dense.hip dense_gemm_kernel, any
// S: zero-padded K tail) wins from 16 instances on, and from 4 on once M leaves
// that cache (S >= 4096).  IRLMX_DENSE_GEMM_MIN=<B> forces the batch threshold.
static bool dense_gemm(const Model& m) {
  if (!m.dense || !m.shared) return false;
  const int forced = env_int("IRLMX_DENSE_GEMM_MIN", 0);
  if (forced > 0) return m.B >= forced;
  return m.B >= 16 || (m.S >= 4096 && m.B >= 4);
}

// The persistent dense shape takes the forward and the collapsed backward
// whenever the rows fit in registers at one workgroup per CU (dense_grid.hip);
// a backward that the planner gives to the GEMM keeps it.
static bool dense_grid(const Model& m, int op, DenseGridPlan* out) {
  if (!m.dense) return false;
  if (op != IRLMX_OP_FORWARD && dense_gemm(m)) return false;
  if (op == IRLMX_OP_SOFT_BACKWARD || op == IRLMX_OP_VALUE_ITERATION) return dense_bellman_grid_plan(m.S, m.B, m.A, out);
  if (op != IRLMX_OP_FORWARD && op != IRLMX_OP_BACKWARD) return false;
  return dense_grid_plan(op == IRLMX_OP_FORWARD ? kModeFwd : kModeBwd, m.S, m.B, out);
}

// The execution shape of one call (IRLMX_SHAPE_*) with that shape's plan.  It
// names the first choice only: an entry point whose persistent launch finds
// its workgroups not co-resident, or whose cluster forward meets a non-finite
// value, reruns per sweep (a DENSE table without the GEMM: a dense grid is
// planned only where the GEMM is not).
struct Route {
  int shape;
  FusedShape fused;
  ClusterPlan cluster;
  GridPlan grid;
  DenseGridPlan dense;
};

// The route of `op` (IRLMX_OP_*), in order: fused; a DENSE table's shapes;
// cluster; grid; per sweep.  `rescale`: the backward call's flag -- without it
// the partition vector overflows like the reference's, and the call stays per
// sweep, where the non-finite bookkeeping is per sweep.  `compact`:
// bwd_compact, which may synchronise a stream, so it is asked only of a
// width-256 stencil backward that reaches the cluster planner.  `cluster`
// false leaves that planner out (carve(), whose rule for it is wider).
static Route route(const Model& m, int op, bool rescale, const std::function<bool()>& compact, bool cluster = true) {
  Route r{};
  if (fused_shape(m, op, &r.fused)) {
    r.shape = IRLMX_SHAPE_FUSED;
  } else if (m.dense) {
    r.shape = dense_grid(m, op, &r.dense)                ? IRLMX_SHAPE_DENSE_GRID
              : op != IRLMX_OP_FORWARD && dense_gemm(m) ? IRLMX_SHAPE_DENSE_GEMM
                                                         : IRLMX_SHAPE_DENSE;
  } else if (cluster && m.stencil && (op == IRLMX_OP_FORWARD || (op == IRLMX_OP_BACKWARD && rescale)) &&
             cluster_plan(m.W, m.H, m.B, op == IRLMX_OP_FORWARD ? kModeFwd : kModeBwd, &r.cluster,
                          op == IRLMX_OP_BACKWARD && m.W == 256 && compact())) {
    r.shape = IRLMX_SHAPE_CLUSTER;
  } else {
    r.shape = grid_plan(m, op, &r.grid) ? IRLMX_SHAPE_GRID : IRLMX_SHAPE_SWEEP;
  }
  return r;
}

// The workspace: sized from the route.
Ws carve(const Model& m, int op, void* base) {
  Ws w;
  Carver c{(char*)base};
  const size_t B = m.B, S = m.S;
  size_t nw = 0;
  if (op == IRLMX_OP_FORWARD) nw = B * m.Kc * S;  // dense: the per-instance gather matrices WT [B][S][S]
  if (op == IRLMX_OP_BACKWARD) nw = m.dense ? B * S : B * m.K * S;  // reward-folded; dense: the GEMM product
  if (op == IRLMX_OP_POLICY_EVALUATION) nw = B * m.K * S;           // policy-folded (policy_eval.hip)
  if ((op == IRLMX_OP_SOFT_BACKWARD || op == IRLMX_OP_VALUE_ITERATION) && m.dense && m.shared)
    nw = (size_t)m.A * B * S;  // the per-action GEMM products of a shared dense table
  w.wgt = c.take<double>(nw * sizeof(double));
  w.bad = c.take<int32_t>(B * sizeof(int32_t));
  const Route r = route(m, op, false, nullptr, false);
  const bool sweep = r.shape != IRLMX_SHAPE_FUSED;
  w.buf0 = c.take<double>(sweep ? B * S * sizeof(double) : 0);
  w.buf1 = c.take<double>(sweep ? B * S * sizeof(double) : 0);
  w.slots = c.take<unsigned long long>(B * 3 * sizeof(unsigned long long));
  w.done = c.take<int32_t>(B * sizeof(int32_t));
  w.iters = c.take<int64_t>(B * sizeof(int64_t));
  w.ndone = c.take<int32_t>(sizeof(int32_t) * 4);
  // The cluster granules go to every stencil forward and backward that is not
  // fused, a wider rule than the route's: a workspace is sized per model and
  // op, before a backward call says whether it rescales.
  const bool cl = sweep && m.stencil && (op == IRLMX_OP_FORWARD || op == IRLMX_OP_BACKWARD);
  const bool gr = r.shape == IRLMX_SHAPE_GRID, dg = r.shape == IRLMX_SHAPE_DENSE_GRID;
  // cluster halo exchange: [B][gran_inst_len] and [B][kSumRows][H] 16-byte granule pairs;
  // grid shape: [B][3][S] value and [B][3][bpi] block-delta granules;
  // dense grid shape: [B][2][S] value and [B][bpi] XCC-id granules
  const size_t gcl = cl ? B * gran_inst_len(m.W, m.H) * 16 : 0;   // cluster.h kGranRowPad layout
  w.gran = c.take<unsigned long long>(std::max(gcl, dg ? 2 * B * S * 16 : (gr ? 3 * B * S * 16 : 0)));
  w.sgran = c.take<unsigned long long>(cl ? kSumRows * B * (size_t)m.H * 16
                                          : (gr ? 4 * B * (size_t)r.grid.bpi * 16 : (dg ? B * (size_t)r.dense.bpi * 16 : 0)));
  w.growth = c.take<unsigned long long>(cl ? 2 * B * sizeof(unsigned long long) : 0);
  w.err = c.take<int>(cl || gr || dg ? 4 * sizeof(int) : 0);
  w.total = c.total();
  return w;
}

static DenseGridArgs dense_grid_args(const Model& m, const Ws& ws) {
  DenseGridArgs a{};
  a.S = m.S; a.A = m.A; a.B = m.B; a.shared = m.shared;
  a.gran = ws.gran; a.xgran = ws.sgran; a.err = ws.err;
  return a;
}

static int dense_backward(const Model& m, const Route& r, const double* reward, const uint8_t* terminal, int rescale,
                          double* p_action, int32_t* status, const Ws& ws, hipStream_t st) {
  const DenseView d = dense_view(m);
  const DenseBufs w = dense_bufs(ws);
  if (r.shape == IRLMX_SHAPE_DENSE_GRID) {  // one persistent launch, M's rows in registers
    DenseGridArgs a = dense_grid_args(m, ws);
    a.mat = m.col_val; a.P = m.row_val; a.vin = reward; a.term = terminal;
    a.rescale = rescale; a.out = p_action; a.status = status;
    const int rc = dense_grid_run(kModeBwd, r.dense, a, st);
    if (rc != kClusterNotResident) return rc;  // else: the per-sweep shape below
  }
  count_event(IRLMX_CTR_SWEEP_CALLS);
  dense_bwd_init_launch(d, terminal, w, st);
  const long long collapsed = 2LL * m.S - 1;
  const bool gemm = r.shape == IRLMX_SHAPE_DENSE_GEMM;
  int r3 = 0;
  for (long long it = 0; it < collapsed; ++it) {
    if (gemm) {
      // C [B][S] = ZS . M^T on the hand-written fp64 MFMA kernel, then the per-state update
      const double* zin = (it & 1) ? ws.buf1 : ws.buf0;
      if (hipError_t e = dense_gemm_launch(m.col_val, zin, ws.wgt, m.S, m.S, m.B, st)) return hip_fail(e, "dense gemm");
      dense_bwd_gemm_epilogue_launch(d, reward, rescale, w, it, r3, st);
    } else {
      dense_bwd_sweep_launch(d, reward, rescale, w, it, r3, st);
    }
    if (hipError_t e = hipGetLastError()) return hip_fail(e, "dense backward sweep");
    r3 = r3 == 2 ? 0 : r3 + 1;
  }
  dense_bwd_final_launch(d, reward, rescale, p_action, status, w, collapsed, r3, st);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, "dense backward");
}

}  // namespace irlmx

using namespace irlmx;

extern "C" int irlmx_dense_to_rows(const double* dense, int32_t n_states, int32_t n_actions, double* p_rows,
                                   double* m_rows, void* stream) {
  if (!dense || !p_rows || !m_rows || n_states <= 0 || n_actions <= 0 || n_actions > kMaxActions) {
    set_error("dense_to_rows: bad arguments (n_states=%d, n_actions=%d in 1..%d, dense %s, p_rows %s, m_rows %s)",
              n_states, n_actions, kMaxActions, dense ? "set" : "NULL", p_rows ? "set" : "NULL",
              m_rows ? "set" : "NULL");
    return IRLMX_EINVAL;
  }
  dense_rows_launch(dense, n_states, n_actions, p_rows, m_rows, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, "dense_to_rows");
}

namespace irlmx {
// The backward's tables fit the compact-weight cluster layout (cluster.hip,
// LAY 4: width 256 only)?  From the model's properties when the caller supplied
// them (irlmx_mdp_properties, checked once per table), else checked on the
// device per call (bwd_compact_ok_kernel), one int of device memory as the flag
// (`flag`, or one allocated for the check when the caller has none); that
// synchronises the stream.  IRLMX_COMPACT=0 turns the layout off.
static bool bwd_compact_check(const Model& m, int* flag, hipStream_t st) {
  if (hipMemsetAsync(flag, 0, sizeof(int), st) != hipSuccess) return false;
  hipLaunchKernelGGL(bwd_compact_ok_kernel, dim3((m.S + 255) / 256, m.shared ? 1 : m.B), dim3(256), 0, st,
                     m.row_val, m.W, m.H, m.A, flag);
  int h = 1;
  if (hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) return false;
  if (hipStreamSynchronize(st) != hipSuccess) return false;
  return h == 0;
}
static bool bwd_compact(const Model& m, int* flag, hipStream_t st) {
  if (!m.stencil || m.W != 256 || env_int("IRLMX_COMPACT", 1) == 0) return false;
  if (m.props & IRLMX_PROPS_KNOWN) return (m.props & IRLMX_PROP_COMPACT) != 0;
  if (flag) return bwd_compact_check(m, flag, st);
  if (hipMalloc((void**)&flag, sizeof(int)) != hipSuccess) return false;
  const bool compact = bwd_compact_check(m, flag, st);
  (void)hipFree(flag);
  return compact;
}
}  // namespace irlmx

// op carries IRLMX_PLAN_EXTENDED_RANGE (never true of a negative op, whose every
// bit is set: those stay "unknown op")
static bool extended_op(int op) { return op > 0 && (op & IRLMX_PLAN_EXTENDED_RANGE) != 0; }

// What the two model queries ask about an op (IRLMX_OP_*, with
// IRLMX_PLAN_EXTENDED_RANGE where it applies): a new op is one more case here.
struct OpQueries {
  bool known = false;                                             // (5, 7 and 10 stay the unknown ops they have always been)
  int (*check_model)(const Model& m, const char* fn) = nullptr;   // null: every model
  size_t (*bytes)(const Model& m, int op) = nullptr;              // null: carve(m, op).total
  void (*plan)(const Model& m, int op, int64_t* plan) = nullptr;  // null: the row of route(m, op)
};
static OpQueries op_queries(int op) {
  switch (op) {
    case IRLMX_OP_BACKWARD:
    case IRLMX_OP_FORWARD:
    case IRLMX_OP_SOFT_BACKWARD:
    case IRLMX_OP_VALUE_ITERATION:
      return {true};
    case IRLMX_OP_POLICY_EVALUATION:
      return {true, policy_eval_check_model};
    case IRLMX_OP_BACKWARD | IRLMX_PLAN_EXTENDED_RANGE:
      return {true, extended_check_model, [](const Model& m, int) { return extended_workspace_bytes(m); },
              [](const Model& m, int, int64_t* plan) { extended_plan(m, plan); }};
    case IRLMX_OP_BACKWARD_HORIZON:
    case IRLMX_OP_FORWARD_HORIZON:
    case IRLMX_OP_SOFT_BACKWARD_HORIZON:
    case IRLMX_OP_VALUE_HORIZON:
      return {true, horizon_check_model, horizon_workspace_bytes, horizon_plan};
  }
  return {};
}

// The extended-range flag goes with IRLMX_OP_BACKWARD alone.
static int check_extended_flag(int op) {
  if (!extended_op(op) || op == (IRLMX_OP_BACKWARD | IRLMX_PLAN_EXTENDED_RANGE)) return 0;
  set_error("IRLMX_PLAN_EXTENDED_RANGE applies to IRLMX_OP_BACKWARD only (and not with IRLMX_PLAN_NO_RESCALE)");
  return IRLMX_EINVAL;
}

// (an op this does not know is sized as carve() sizes it)
extern "C" size_t irlmx_workspace_bytes(const irlmx_mdp* mdp, int32_t op) {
  if (validate(mdp)) return 0;
  const Model m = make_model(mdp);
  if (check_extended_flag(op)) return 0;
  const OpQueries q = op_queries(op);
  if (q.check_model && q.check_model(m, "workspace_bytes")) return 0;
  return q.bytes ? q.bytes(m, op) : carve(m, op, nullptr).total;
}

extern "C" int irlmx_execution_plan(const irlmx_mdp* mdp, int32_t op, int64_t* plan) {
  if (int rc = validate(mdp)) return rc;
  if (!plan) { set_error("plan is NULL"); return IRLMX_EINVAL; }
  if (int rc = check_extended_flag(op)) return rc;
  // (a backward call with rescale = 0 never takes the cluster shape: see irlmx_backward_maxent)
  const bool no_rescale = op > 0 && !extended_op(op) && (op & IRLMX_PLAN_NO_RESCALE) != 0;
  if (no_rescale) op &= ~IRLMX_PLAN_NO_RESCALE;
  const OpQueries q = op_queries(op);
  if (!q.known) { set_error("unknown op %d", op); return IRLMX_EINVAL; }
  if (no_rescale && op != IRLMX_OP_BACKWARD) { set_error("IRLMX_PLAN_NO_RESCALE applies to IRLMX_OP_BACKWARD only"); return IRLMX_EINVAL; }
  const Model m = make_model(mdp);
  if (int rc = q.check_model ? q.check_model(m, "execution_plan") : 0) {
    if (horizon_op(op)) std::fill_n(plan, IRLMX_PLAN_LEN, 0);  // (as these ops always have, although the model is refused)
    return rc;
  }
  std::fill_n(plan, IRLMX_PLAN_LEN, 0);
  if (q.plan) {
    q.plan(m, op, plan);
    return 0;
  }
  // (the compact layout is data-dependent: from the table's properties, else checked on the device)
  const Route r = route(m, op, !no_rescale, [&] { return bwd_compact(m, nullptr, nullptr); });
  plan[0] = r.shape;
  switch (r.shape) {
    case IRLMX_SHAPE_FUSED:
      plan_fused(plan, r.fused, fused_lds(m));
      break;
    case IRLMX_SHAPE_CLUSTER: {
      const ClusterPlan& cp = r.cluster;
      plan[1] = cp.R; plan[2] = cp.G; plan[3] = cp.C; plan[4] = cp.per_launch; plan[5] = cp.spt;
      plan[6] = cp.pair; plan[7] = cp.nt; plan[8] = (m.B + cp.per_launch - 1) / cp.per_launch;
      plan[9] = (int64_t)cp.lds;
      break;
    }
    case IRLMX_SHAPE_GRID:  // (the G column: 1 = workgroups grouped by XCD)
      plan[2] = r.grid.xcd; plan[3] = r.grid.bpi; plan[4] = m.B; plan[5] = r.grid.spt;
      plan[7] = kGridThreads; plan[8] = 1;
      break;
    case IRLMX_SHAPE_DENSE_GRID:
      // (the R column: matrix rows per workgroup; spt: columns per thread; layout: soft VI / VI's
      // actions compiled per state, 0 for the forward / backward)
      plan[1] = r.dense.rb; plan[2] = r.dense.xcd; plan[3] = r.dense.bpi; plan[4] = m.B;
      plan[5] = r.dense.cpt; plan[6] = r.dense.at; plan[7] = kDenseGridThreads; plan[8] = 1;
      break;
    case IRLMX_SHAPE_DENSE:
    case IRLMX_SHAPE_DENSE_GEMM:
      plan[7] = kDenseThreads;
      plan[9] = dense_lds_vec(dense_view(m)) ? (int64_t)m.S * 8 : 0;
      break;
    case IRLMX_SHAPE_SWEEP:  // (policy evaluation: one state per lane; the launch count is the sweep count)
      plan_sweep(plan, op == IRLMX_OP_POLICY_EVALUATION ? 1 : 0, 0);
      break;
  }
  return 0;
}

extern "C" int irlmx_forward_svf(const irlmx_mdp* mdp, const double* p_initial, const uint8_t* terminal,
                                 const double* p_action, double eps, int64_t max_iter, double* svf,
                                 int64_t* iterations, int32_t* status, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  if (int rc = validate(mdp)) return rc;
  const Model m = make_model(mdp);
  if (int rc = need_col_form(m)) return rc;
  if (int rc = need_all("forward_svf", {{p_initial, "p_initial"}, {terminal, "terminal"}, {p_action, "p_action"},
                                        {svf, "svf"}, {iterations, "iterations"}, {status, "status"}}))
    return rc;
  if (int rc = check_ws(m, IRLMX_OP_FORWARD, workspace_bytes, workspace)) return rc;
  hipStream_t st = (hipStream_t)stream;
  Ws ws = carve(m, IRLMX_OP_FORWARD, workspace);
  hipError_t e = hipMemsetAsync(workspace, 0, ws.total, st);
  if (e != hipSuccess) return hip_fail(e, "workspace memset");
  const dim3 g = sweep_grid(m);
  if (!m.dense) hipLaunchKernelGGL(fwd_weights_kernel, g, dim3(kSweepThreads), 0, st, m, p_action, terminal, ws.wgt, ws.bad);
  FwdArgs a{m, ws.wgt, ws.bad, p_initial, eps, (long long)max_iter, svf, iterations, status};
  // dense rows (dense.hip): per-instance gather matrices WT
  const DenseView d = dense_view(m);
  const DenseBufs w = dense_bufs(ws);
  if (m.dense) dense_fwd_weights_launch(d, p_action, terminal, w, st);
  const Route r = route(m, IRLMX_OP_FORWARD, true, nullptr);
  switch (r.shape) {
    case IRLMX_SHAPE_FUSED:
      return run_fused(fwd_fused_fn(r.fused), "fwd_fused_ptr", m, r.fused, st, a);
    case IRLMX_SHAPE_DENSE_GRID: {  // one persistent launch, WT's rows in registers
      DenseGridArgs ga = dense_grid_args(m, ws);
      ga.mat = ws.wgt; ga.vin = p_initial; ga.bad = ws.bad; ga.eps = eps; ga.max_iter = (long long)max_iter;
      ga.out = svf; ga.iters = iterations; ga.status = status;
      const int rc = dense_grid_run(kModeFwd, r.dense, ga, st);
      if (rc != kClusterNotResident) return rc;
      break;
    }
    case IRLMX_SHAPE_CLUSTER: {
      ClusterArgs ca{};
      ca.W = m.W; ca.H = m.H; ca.S = m.S; ca.A = m.A;
      ca.wgt = ws.wgt; ca.vin = p_initial; ca.bad = ws.bad;
      ca.eps = eps; ca.max_iter = (long long)max_iter;
      ca.gran = ws.gran; ca.sgran = ws.sgran; ca.err = ws.err;
      ca.out = svf; ca.iters = iterations; ca.status = status;
      const int rc = cluster_run(kModeFwd, r.cluster, ca, m.B, st);
      if (rc != kClusterNonFinite && rc != kClusterNotResident) return rc;
      // an instance turned non-finite (rare): the cluster shape's convergence bits
      // drop NaN deltas, so rerun the call on the per-sweep shape, whose
      // bookkeeping is exact (same arithmetic, bit-identical results); likewise
      // when the tiles could not all run at once (another kernel holds CUs)
      if (rc == kClusterNonFinite) count_event(IRLMX_CTR_RERUN_NONFINITE);
      e = hipMemsetAsync(workspace, 0, ws.total, st);
      if (e != hipSuccess) return hip_fail(e, "workspace memset");
      hipLaunchKernelGGL(fwd_weights_kernel, g, dim3(kSweepThreads), 0, st, m, p_action, terminal, ws.wgt, ws.bad);
      break;
    }
    case IRLMX_SHAPE_GRID: {  // ELL models: one persistent launch
      const int rc = grid_run(m, IRLMX_OP_FORWARD, r.grid,
                              LinearGridArgs{m, ws.wgt, p_initial, nullptr, ws.bad, eps, (long long)max_iter, 0, svf,
                                             iterations, status},
                              ws, st);
      if (rc != kClusterNotResident) return rc;
      break;
    }
  }
  // the per-sweep shape: the route's choice, or the rerun of a persistent launch
  count_event(IRLMX_CTR_SWEEP_CALLS);
  int rc = run_until_done(ws, m.B, st, [&](long long it, int r3) {
    if (m.dense) dense_fwd_sweep_launch(d, p_initial, eps, (long long)max_iter, status, w, it, r3, st);
    else hipLaunchKernelGGL(fwd_sweep_kernel, g, dim3(kSweepThreads), 0, st, a, ws, it, r3);
  });
  if (rc) return rc;
  hipLaunchKernelGGL(fwd_finish_kernel, g, dim3(kSweepThreads), 0, st, a, ws);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, m.dense ? "dense forward" : "fwd_finish");
}

extern "C" int irlmx_backward_maxent(const irlmx_mdp* mdp, const double* reward, const uint8_t* terminal,
                                     int32_t rescale, double* p_action, int32_t* status, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (int rc = validate(mdp)) return rc;
  const Model m = make_model(mdp);
  if (int rc = need_all("backward_maxent",
                        {{reward, "reward"}, {terminal, "terminal"}, {p_action, "p_action"}, {status, "status"}}))
    return rc;
  if (int rc = check_ws(m, IRLMX_OP_BACKWARD, workspace_bytes, workspace)) return rc;
  hipStream_t st = (hipStream_t)stream;
  Ws ws = carve(m, IRLMX_OP_BACKWARD, workspace);
  hipError_t e = hipMemsetAsync(workspace, 0, ws.total, st);
  if (e != hipSuccess) return hip_fail(e, "workspace memset");
  if (!m.dense) bwd_weights_launch(m, reward, ws.wgt, ws.bad, st);
  const Route r = route(m, IRLMX_OP_BACKWARD, rescale != 0, [&] { return bwd_compact(m, ws.err + 3, st); });
  if (m.dense) return dense_backward(m, r, reward, terminal, rescale, p_action, status, ws, st);
  BwdArgs a{m, ws.wgt, reward, terminal, rescale, p_action, status};
  switch (r.shape) {
    case IRLMX_SHAPE_FUSED:
      return run_fused(bwd_fused_fn(r.fused), "bwd_fused_ptr", m, r.fused, st, a);
    case IRLMX_SHAPE_CLUSTER: {
      hipLaunchKernelGGL(bwd_growth_kernel, dim3(m.B), dim3(1024), 0, st, ws.wgt, m.W, m.S, m.B, ws.growth);
      ClusterArgs ca{};
      ca.W = m.W; ca.H = m.H; ca.S = m.S; ca.A = m.A;
      ca.tab_shared = m.shared ? 1 : 0;
      ca.wgt = ws.wgt; ca.row_val = m.row_val; ca.vin = reward; ca.term = terminal; ca.growth = ws.growth;
      ca.n_sweeps = 2LL * m.S - 1; ca.rescale = rescale;
      ca.gran = ws.gran; ca.sgran = ws.sgran; ca.err = ws.err;
      ca.out = p_action; ca.status = status;
      const int rc = cluster_run(kModeBwd, r.cluster, ca, m.B, st);
      if (rc != kClusterNotResident) {
        if (rc) return rc;
        // instances with non-finite weights: all NaN (bwd_nonfinite_rule), outside the sweep kernel
        hipLaunchKernelGGL(bwd_nan_fill_kernel, dim3((m.S * m.A + 255) / 256, m.B), dim3(256), 0, st, m, ws.bad,
                           p_action);
        e = hipGetLastError();
        return e == hipSuccess ? 0 : hip_fail(e, "backward nan fill");
      }
      // the tiles could not all run at once (another kernel holds CUs): rerun on
      // the per-sweep shape (same arithmetic, bit-identical results)
      e = hipMemsetAsync(workspace, 0, ws.total, st);
      if (e != hipSuccess) return hip_fail(e, "workspace memset");
      bwd_weights_launch(m, reward, ws.wgt, ws.bad, st);
      break;
    }
    case IRLMX_SHAPE_GRID: {  // ELL models: one persistent launch
      const int rc = grid_run(m, IRLMX_OP_BACKWARD, r.grid,
                              LinearGridArgs{m, ws.wgt, reward, terminal, ws.bad, 0.0, 0, rescale, p_action, nullptr,
                                             status},
                              ws, st);
      if (rc != kClusterNotResident) return rc;
      break;
    }
  }
  // the per-sweep shape: the route's choice, or the rerun of a persistent launch
  const dim3 g = sweep_grid(m);
  count_event(IRLMX_CTR_SWEEP_CALLS);
  hipLaunchKernelGGL(bwd_init_kernel, g, dim3(kSweepThreads), 0, st, a, ws);
  const long long collapsed = 2LL * m.S - 1;
  int r3 = 0;
  for (long long it = 0; it < collapsed; ++it) {
    hipLaunchKernelGGL(bwd_sweep_kernel, g, dim3(kSweepThreads), 0, st, a, ws, it, r3);
    r3 = r3 == 2 ? 0 : r3 + 1;
  }
  hipLaunchKernelGGL(bwd_final_kernel, g, dim3(kSweepThreads), 0, st, a, ws, collapsed, r3);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, "backward");
}

extern "C" int irlmx_mdp_properties(const irlmx_mdp* mdp, int32_t* props, void* stream) {
  if (int rc = validate(mdp)) return rc;
  if (!props) { set_error("mdp_properties: props is NULL"); return IRLMX_EINVAL; }
  Model m = make_model(mdp);
  m.props = 0;
  hipStream_t st = (hipStream_t)stream;
  int32_t p = IRLMX_PROPS_KNOWN;
  if (m.stencil) {
    int* flag = nullptr;
    hipError_t e = hipMallocAsync((void**)&flag, sizeof(int), st);
    if (e != hipSuccess) return hip_fail(e, "mdp_properties");
    const bool compact = bwd_compact_check(m, flag, st);
    e = hipFreeAsync(flag, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "mdp_properties");
    if (compact) p |= IRLMX_PROP_COMPACT;
  } else if (!m.dense) {
    bool sorted = false;
    if (int rc = ell_rows_sorted(m, st, &sorted)) return rc;
    if (sorted) p |= IRLMX_PROP_ELL_SORTED;
  }
  *props = p;
  return 0;
}

static int bellman_common(const irlmx_mdp* mdp, const double* reward, const double* phi, double discount,
                          double eps, int64_t max_iter, int average, double* p_action, double* value,
                          int64_t* iterations, int32_t* status, void* workspace, size_t workspace_bytes,
                          void* stream, bool soft) {
  if (int rc = validate(mdp)) return rc;
  const Model m = make_model(mdp);
  const int op = soft ? IRLMX_OP_SOFT_BACKWARD : IRLMX_OP_VALUE_ITERATION;
  if (int rc = need_all(soft ? "soft_backward" : "value_iteration",
                        {{reward, "reward"}, {phi, soft ? "terminal_reward" : nullptr},
                         {p_action, soft ? "p_action" : nullptr}, {value, soft ? nullptr : "value"},
                         {iterations, "iterations"}, {status, "status"}}))
    return rc;
  if (int rc = check_ws(m, op, workspace_bytes, workspace)) return rc;
  hipStream_t st = (hipStream_t)stream;
  Ws ws = carve(m, op, workspace);
  hipError_t e = hipMemsetAsync(workspace, 0, ws.total, st);
  if (e != hipSuccess) return hip_fail(e, "workspace memset");
  SoftArgs a{m, reward, phi, discount, eps, (long long)max_iter, average, p_action, value, iterations, status};
  const Route r = route(m, op, true, nullptr);
  if (r.shape == IRLMX_SHAPE_FUSED)
    return run_fused(bellman_fused_fn(soft, r.fused), soft ? "soft_fused_ptr" : "vi_fused_ptr", m, r.fused, st, a);
  const size_t n = (size_t)m.B * m.S;
  hipLaunchKernelGGL(fill_kernel, dim3((n + 255) / 256), dim3(256), 0, st, ws.buf0, n, soft ? -1e200 : 0.0);
  if (r.shape == IRLMX_SHAPE_DENSE_GRID) {  // one persistent launch, the A rows of each state in registers
    DenseGridArgs ga = dense_grid_args(m, ws);
    ga.P = m.row_val; ga.vin = reward; ga.phi = phi; ga.discount = discount; ga.average = average;
    ga.value = value; ga.eps = eps; ga.max_iter = (long long)max_iter;
    ga.out = p_action; ga.iters = iterations; ga.status = status;
    const int rc = dense_bellman_grid_run(soft, r.dense, ga, st);
    if (rc != kClusterNotResident) return rc;
  } else if (r.shape == IRLMX_SHAPE_GRID) {  // persistent grid shape: one launch for the whole loop
    const int rc = grid_run(m, op, r.grid, a, ws, st);
    if (rc != kClusterNotResident) return rc;
  }
  // the per-sweep shape: the route's choice, or the rerun of a persistent launch
  count_event(IRLMX_CTR_SWEEP_CALLS);
  const DenseView d = dense_view(m);  // dense rows (dense.hip)
  const DenseBufs w = dense_bufs(ws);
  const DenseBellman db{reward, phi, discount, eps, (long long)max_iter, average, soft ? 1 : 0, p_action, value,
                        iterations, status};
  const bool gemm = r.shape == IRLMX_SHAPE_DENSE_GEMM;  // the P . [v_1 .. v_B] products on the MFMA kernel
  hipError_t gerr = hipSuccess;
  const dim3 g = sweep_grid(m);
  // the Bellman sweep is a latency chain per state (A dots, A softmax folds):
  // smaller workgroups spread one instance over more CUs (IRLMX_BELLMAN_THREADS)
  const int bt = std::max(64, std::min(kSweepThreads, env_int("IRLMX_BELLMAN_THREADS", kSweepThreads)));
  const dim3 gb((m.S + bt - 1) / bt, m.B);
  int rc = run_until_done(ws, m.B, st, [&](long long it, int r3) {
    if (gemm) {
      const hipError_t e = dense_bellman_gemm_sweep_launch(d, db, w, it, r3, st);
      if (e != hipSuccess && gerr == hipSuccess) gerr = e;
    } else if (m.dense) dense_bellman_sweep_launch(d, db, w, it, r3, st);
    else if (soft) hipLaunchKernelGGL(bellman_sweep_kernel<true>, gb, dim3(bt), 0, st, a, ws, it, r3);
    else hipLaunchKernelGGL(bellman_sweep_kernel<false>, gb, dim3(bt), 0, st, a, ws, it, r3);
  });
  if (gerr != hipSuccess) return hip_fail(gerr, "dense gemm");
  if (rc) return rc;
  if (m.dense) dense_bellman_finish_launch(d, db, w, st);
  else if (soft) hipLaunchKernelGGL(bellman_finish_kernel<true>, g, dim3(kSweepThreads), 0, st, a, ws);
  else hipLaunchKernelGGL(bellman_finish_kernel<false>, g, dim3(kSweepThreads), 0, st, a, ws);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, m.dense ? "dense bellman" : "bellman finish");
}

extern "C" int irlmx_soft_backward(const irlmx_mdp* mdp, const double* reward, const double* terminal_reward,
                                   double discount, double eps, int64_t max_iter, double* p_action,
                                   double* value, int64_t* iterations, int32_t* status, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  return bellman_common(mdp, reward, terminal_reward, discount, eps, max_iter, 0, p_action, value, iterations,
                        status, workspace, workspace_bytes, stream, true);
}

extern "C" int irlmx_value_iteration(const irlmx_mdp* mdp, const double* reward, double discount, double eps,
                                     int32_t average, int64_t max_iter, double* value, int64_t* iterations,
                                     int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  return bellman_common(mdp, reward, nullptr, discount, eps, max_iter, average, nullptr, value, iterations,
                        status, workspace, workspace_bytes, stream, false);
}

extern "C" int irlmx_dense_gemm(const double* m, const double* z, double* c, int32_t rows, int32_t n, int32_t batch,
                                void* stream) {
  if (!m || !z || !c || rows <= 0 || n <= 0 || batch <= 0) {
    set_error("dense_gemm: bad arguments (rows=%d, n=%d, batch=%d, m %s, z %s, c %s)", rows, n, batch,
              m ? "set" : "NULL", z ? "set" : "NULL", c ? "set" : "NULL");
    return IRLMX_EINVAL;
  }
  const hipError_t e = dense_gemm_launch(m, z, c, rows, n, batch, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(e, "dense_gemm");
}

extern "C" int irlmx_dense_gemm_variant(int32_t rows, int32_t n, int32_t batch, int32_t* variant) {
  if (!variant || rows <= 0 || n <= 0 || batch <= 0) {
    set_error("dense_gemm_variant: bad arguments");
    return IRLMX_EINVAL;
  }
  int v[4];
  dense_gemm_variant(rows, n, batch, v);
  for (int i = 0; i < 4; ++i) variant[i] = v[i];
  return 0;
}

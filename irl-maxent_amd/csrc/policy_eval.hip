// Policy evaluation (irlmx_policy_evaluation) on gfx950: the value of a given
// stochastic policy,
//
//   v <- r + gamma * sum_a pi_a * (P_a v)   from v = 0 until max|v' - v| <= eps
//
// the fifth fixed-point loop beside the four of fixed_point.hip.  It collapses
// the way the backward and the forward do: the policy is folded into one
// weight per stored edge once per call,
//
//   w[b][k][s] = sum_a pi[b][s][a] * P[s, target_k(s), a]    A fmas in action order from 0
//                (0 at terminal states: their successors contribute nothing, v(s) = r(s))
//
// and a sweep is then K fused multiply-adds per state instead of A * K:
//
//   acc   = fma(w[k][s], v[target_k(s)], acc)                in slot order from 0
//   v'(s) = r(s) + gamma * acc                               the product rounded, then the sum
//
// Two shapes, chosen as for the other passes (fused_shape): fused -- one
// workgroup per instance for the whole loop, v ping-pongs in LDS, weights and
// neighbour indices in registers per (states per thread, slot class) pair, the
// exact stop through run_deferred (a gamma = 1 episodic evaluation runs
// 10^4-10^5 sweeps, as the forward does; the two pairs with 32 slots per thread
// reduce every sweep instead) -- and per sweep: one launch per sweep
// over all instances on the sweep shape's done flag, 3-slot convergence ring and
// host poll.  Same weights, slot order and statements in both: the same bits,
// sweep counts and status.  There is no persistent multi-CU shape (DESIGN.md
// section 4, "Policy evaluation").

#include <hip/hip_runtime.h>

#include "common.h"
#include "fixed_point.h"

namespace irlmx {

struct PeArgs {
  Model m;
  const double* w;  // [B][K][S] policy-folded weights (pe_weights_kernel)
  const double* reward;
  double discount;
  double eps;
  long long max_iter;
  double* value;
  int64_t* iters;
  int32_t* status;
};

// The row-form twin of fwd_weights_kernel: one weight per (state s, slot k).
// `term` may be null (no terminal handling).
__global__ void pe_weights_kernel(Model m, const double* __restrict__ pi, const uint8_t* __restrict__ term,
                                  double* __restrict__ w) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (s >= m.S) return;
  const int S = m.S, A = m.A;
  const double* pis = pi + ((size_t)b * S + s) * A;
  const bool terminal = term && term[(size_t)b * S + s];
  for (int k = 0; k < m.K; ++k) {
    double acc = 0.0;
    if (!terminal)
      for (int a = 0; a < A; ++a) acc = fma(pis[a], row_val(m, b, a, k, s), acc);
    w[((size_t)b * m.K + k) * S + s] = acc;
  }
}

__device__ inline double pe_update(double r, double discount, double acc) {
  return __dadd_rn(r, __dmul_rn(discount, acc));
}

// ---------------------------------------------------------------------------
// fused shape: one workgroup per instance for the whole loop
// ---------------------------------------------------------------------------

// one barrier per sweep; LDS: two S-vectors, the convergence slots and
// run_deferred's block-start snapshot (fused_lds)
template <int SPT, int KMAX>
__global__ void __launch_bounds__(1024) pe_fused_kernel(PeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pe_smem[];
  const Model& m = a.m;
  const int S = m.S, K = m.K;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  double* bufA = (double*)pe_smem;
  double* bufB = bufA + S;
  unsigned long long* slot = (unsigned long long*)(bufB + S);
  double* snap = (double*)(slot + 4);

  double w[SPT][KMAX];
  int nb[SPT][KMAX];
  double r[SPT], cur[SPT];
  const double* wb = a.w + (size_t)b * K * S;
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tid + j * nt;
    cur[j] = 0.0;
    r[j] = 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) { w[j][k] = 0.0; nb[j][k] = 0; }
    if (s < S) {
      r[j] = a.reward[(size_t)b * S + s];
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) { w[j][k] = wb[(size_t)k * S + s]; nb[j][k] = row_nbr(m, b, s, k); }
    }
  }
  for (int s = tid; s < S; s += nt) bufA[s] = 0.0;  // solver.py:32
  if (tid < 3) slot[tid] = 0ull;
  __syncthreads();

  long long it = 0;
  auto sweep = [&](long long sweep_it, int pos, unsigned long long& bits) __attribute__((always_inline)) {
    const double* vin = (sweep_it & 1) ? bufB : bufA;
    double* vout = (sweep_it & 1) ? bufA : bufB;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int s = tid + j * nt;
      if (s < S) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (k < K) acc = fma(w[j][k], vin[nb[j][k]], acc);
        const double nv = pe_update(r[j], a.discount, acc);
        vout[s] = nv;
        record_delta(bits, pos, fabs(nv - cur[j]), a.eps);
        cur[j] = nv;
      }
    }
  };
  // 32 slots per thread fill the registers (96 VGPRs of weights and indices of
  // the 128 a 1024-thread workgroup leaves each lane; run_deferred's block
  // bookkeeping spilled 76 there): those two pairs take the per-sweep max
  // reduction of fwd_fused_kernel -- the same stopping rule, the same bits
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
          double* v0 = (it & 1) ? bufB : bufA;
#pragma unroll
          for (int j = 0; j < SPT; ++j)
            if (tid + j * nt < S) v0[tid + j * nt] = cur[j] = snap[tid + j * nt];
          __syncthreads();
        });
  } else {
    int r3 = 0;
    double delta = 0.0;
    for (;;) {
      const double* vin = (it & 1) ? bufB : bufA;
      double* vout = (it & 1) ? bufA : bufB;
      unsigned long long mx = 0ull;
#pragma unroll
      for (int j = 0; j < SPT; ++j) {
        const int s = tid + j * nt;
        if (s < S) {
          double acc = 0.0;
#pragma unroll
          for (int k = 0; k < KMAX; ++k)
            if (k < K) acc = fma(w[j][k], vin[nb[j][k]], acc);
          const double nv = pe_update(r[j], a.discount, acc);
          vout[s] = nv;
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
    if (s < S) a.value[(size_t)b * S + s] = cur[j];
  }
  if (tid == 0) { a.iters[b] = it; a.status[b] = status; }
}

// ---------------------------------------------------------------------------
// per-sweep shape: one launch per sweep over all instances
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(kSweepThreads) pe_sweep_kernel(PeArgs a, Ws ws, long long it, int r3) {
  const Model& m = a.m;
  const int b = blockIdx.y;
  if (sweep_should_stop(b, it, r3, a.eps, a.max_iter, ws, a.status)) return;
  const int S = m.S;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const double* vin = ((it & 1) ? ws.buf1 : ws.buf0) + (size_t)b * S;
  double* vout = ((it & 1) ? ws.buf0 : ws.buf1) + (size_t)b * S;
  unsigned long long d = 0ull;
  if (s < S) {
    const double* wb = a.w + (size_t)b * m.K * S;
    double acc = 0.0;
    for (int k = 0; k < m.K; ++k) acc = fma(wb[(size_t)k * S + s], vin[row_nbr(m, b, s, k)], acc);
    const double nv = pe_update(a.reward[(size_t)b * S + s], a.discount, acc);
    vout[s] = nv;
    d = abs_bits(nv - vin[s]);
  }
  block_max_to(d, &ws.slots[b * 3 + r3]);
  if (blockIdx.x == 0 && threadIdx.x == 0) ws.slots[b * 3 + (r3 == 2 ? 0 : r3 + 1)] = 0ull;
}

__global__ void pe_finish_kernel(PeArgs a, Ws ws) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  const int S = a.m.S;
  if (s >= S) return;
  const long long it = ws.iters[b];
  a.value[(size_t)b * S + s] = ((it & 1) ? ws.buf1 : ws.buf0)[(size_t)b * S + s];
  if (s == 0) a.iters[b] = it;
}

// ---------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------

// (SPT, KMAX) pairs instantiated: fused_pair_ok's list for this op, the one
// fused_shape plans from (fixed_point.h); every pair compiles without VGPR
// spills at __launch_bounds__(1024) (tools/kernel_resources.py).
static void (*pe_fused_fn(const FusedShape& f))(PeArgs) {
  return with_pair<void (*)(PeArgs)>(f.spt, f.kmax, [](auto s, auto k) {
    if constexpr (fused_pair_ok(IRLMX_OP_POLICY_EVALUATION, s, k)) return &pe_fused_kernel<s, k>;
    else return nullptr;
  });
}

int policy_eval_check_model(const Model& m, const char* fn) {
  if (m.dense) {
    set_error("%s: policy evaluation does not run the DENSE layout (STENCIL5 and ELL only)", fn);
    return IRLMX_EINVAL;
  }
  return 0;
}

}  // namespace irlmx

using namespace irlmx;

extern "C" int irlmx_policy_evaluation(const irlmx_mdp* mdp, const double* reward, const double* p_action,
                                       const uint8_t* terminal, double discount, double eps, int64_t max_iter,
                                       double* value, int64_t* iterations, int32_t* status, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  if (int rc = validate(mdp)) return rc;
  const Model m = make_model(mdp);
  if (int rc = policy_eval_check_model(m, "policy_evaluation")) return rc;
  if (int rc = need_all("policy_evaluation", {{reward, "reward"}, {p_action, "p_action"}, {value, "value"},
                                              {iterations, "iterations"}, {status, "status"}}))
    return rc;
  if (!(discount >= 0.0 && discount <= 1.0)) {  // (NaN fails both comparisons)
    set_error("policy_evaluation: discount %g outside [0, 1]", discount);
    return IRLMX_EINVAL;
  }
  if (int rc = check_ws(m, IRLMX_OP_POLICY_EVALUATION, workspace_bytes, workspace)) return rc;
  hipStream_t st = (hipStream_t)stream;
  Ws ws = carve(m, IRLMX_OP_POLICY_EVALUATION, workspace);
  const dim3 g = sweep_grid(m);
  hipLaunchKernelGGL(pe_weights_kernel, g, dim3(kSweepThreads), 0, st, m, p_action, terminal, ws.wgt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "pe_weights_kernel");
  PeArgs a{m, ws.wgt, reward, discount, eps, (long long)max_iter, value, iterations, status};
  FusedShape fs;
  if (fused_shape(m, IRLMX_OP_POLICY_EVALUATION, &fs)) {
    void (*kfn)(PeArgs) = pe_fused_fn(fs);
    if (!kfn) { set_error("no policy evaluation fused kernel for spt=%d kmax=%d", fs.spt, fs.kmax); return IRLMX_EINVAL; }
    return launch_fused(kfn, "pe_fused_kernel", m.B, fs.threads, fused_lds(m), st, a);
  }
  // the sweep shape's state, everything carved after the weights (which
  // pe_weights_kernel writes in full): v = 0, the ring, the done flags and count;
  // the fused kernel keeps all of that in LDS and reads none of it
  const size_t head = (size_t)((char*)ws.bad - (char*)workspace);
  e = hipMemsetAsync(ws.bad, 0, ws.total - head, st);
  if (e != hipSuccess) return hip_fail(e, "workspace memset");
  count_event(IRLMX_CTR_SWEEP_CALLS);
  if (int rc = run_until_done(ws, m.B, st, [&](long long it, int r3) {
        hipLaunchKernelGGL(pe_sweep_kernel, g, dim3(kSweepThreads), 0, st, a, ws, it, r3);
      }))
    return rc;
  hipLaunchKernelGGL(pe_finish_kernel, g, dim3(kSweepThreads), 0, st, a, ws);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, "pe_finish_kernel");
}

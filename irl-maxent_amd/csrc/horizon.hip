// Finite-horizon MaxEnt (irlmx_backward_maxent_horizon, irlmx_forward_svf_horizon)
// on gfx950: Ziebart's Algorithm 1 for a fixed number of steps T, with no
// terminal state needed.
//
// Backward, for t = T-1 .. 0 from Z_T(s) = er(s) = exp(r(s)):
//
//   za_t(s,a) = er(s) * sum_k P[s, target_k(s), a] * Z_{t+1}(target_k(s))
//   Z_t(s)    = sum_a za_t(s,a)      (terminal s: Z_t(s) = er(s), held)
//   pi_t(s,a) = za_t(s,a) / Z_t'(s)  (Z_t' the sum just formed, also at terminals)
//
// Every Z is m * 2^e (extended.h); a step is "the last sweep, per action" of
// the extended backward (ext_policy_row's statement order) done at every step:
//   1. E = the largest neighbour exponent over the slots where some action has
//      a nonzero entry
//   2. per action, acc = fma(P, aligned z, acc) in slot order, za = er * acc rounded
//   3. zsum = the sequential action sum
//   4. pi = za / zsum
//   5. ext_split(zsum, E) gives Z_t(s)
//
// Forward, for t = 0 .. T-1 from d_0 = p0, D = p0:
//
//   w           = sum_a fma(P[u -> s', a], pi_t[u][a], w)   action order from 0; 0 for terminal u
//   d_{t+1}(s') = sum_k fma(w_k, d_t[u_k], acc)             every slot of the column form in slot
//                                                           order (fwd_weights_kernel's access: an
//                                                           off-grid stencil slot has w = 0, u = s')
//   D(s')       = D(s') + d_{t+1}(s')                       one rounded add per step
//
// Two shapes per pass, chosen like policy evaluation's: fused -- one workgroup
// per instance for all T steps, (mantissa, exponent) pairs (backward) or d_t
// (forward) ping-pong in LDS, one barrier per step -- and per sweep: one launch
// per step over all instances, buffers in the caller's workspace; the launch
// count is T, so the host never polls.  Same statements in both: the same bits.
// There is no persistent multi-CU shape ("Finite horizon").

#include <hip/hip_runtime.h>

#include "extended.h"
#include "horizon.h"
#include "horizon_rows.h"

namespace irlmx {

constexpr int kHzRegActions = 4;        // actions of the register-resident table variant

struct HzBwdArgs {
  Model m;
  const double* reward;
  const uint8_t* term;  // may be null
  int T;
  double* pi;      // [B][T][S][A]
  double* log_z0;  // [B][S], may be null
  int32_t* status;
};

struct HzFwdArgs {
  Model m;
  const double* p0;
  const uint8_t* term;  // may be null
  const double* pi;     // [B][T][S][A]
  int T;
  double* svf;    // [B][S]
  double* svf_t;  // [B][T+1][S], may be null
  int32_t* status;
};

// bwd_nonfinite_rule for this pass: a non-finite exp(r) anywhere in the instance
__device__ inline void hz_nan_state(const HzBwdArgs& a, int b, int t, int s) {
  double* out = a.pi + hz_pi_row(a.m, a.T, b, t, s);
  for (int act = 0; act < a.m.A; ++act) out[act] = kNaN;
  if (t == 0 && a.log_z0) a.log_z0[(size_t)b * a.m.S + s] = kNaN;
}

// ---------------------------------------------------------------------------
// fused shape: one workgroup per instance for all T steps
// ---------------------------------------------------------------------------

// REG: the A * K table values of every state of this lane stay in registers
// (A <= kHzRegActions); otherwise they are read from memory each step (L2).
template <int SPT, int KMAX, bool REG>
__global__ void __launch_bounds__(1024) hz_bwd_fused_kernel(HzBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hz_smem[];
  const Model& m = a.m;
  const int S = m.S, K = m.K, A = m.A, T = a.T;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  double* manA = (double*)hz_smem;
  double* manB = manA + S;
  int* expA = (int*)(manB + S);
  int* expB = expA + S;

  constexpr bool kHoldNb = KMAX <= 8;  // from 16 slots on: row_nbr at every use (hz_row rolls its slot loop)
  double er[SPT];
  int nb[kHoldNb ? SPT : 1][kHoldNb ? KMAX : 1];
  unsigned any[SPT];
  bool term[SPT];
  double tab[REG ? SPT : 1][REG ? kHzRegActions : 1][REG ? KMAX : 1];
  int nonfinite = 0;
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tid + j * nt;
    er[j] = 1.0;
    any[j] = 0u;
    term[j] = false;
    if constexpr (kHoldNb) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k) nb[j][k] = 0;
    }
    if (s < S) {
      er[j] = exp(a.reward[(size_t)b * S + s]);
      nonfinite |= !isfinite(er[j]);
      term[j] = a.term && a.term[(size_t)b * S + s] != 0;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) {
          if constexpr (kHoldNb) nb[j][k] = row_nbr(m, b, s, k);
          bool nz = false;
          for (int act = 0; act < A; ++act) nz |= row_val(m, b, act, k, s) != 0.0;
          any[j] |= (nz ? 1u : 0u) << k;
        }
      if constexpr (REG) {
#pragma unroll
        for (int act = 0; act < kHzRegActions; ++act)
#pragma unroll
          for (int k = 0; k < KMAX; ++k) tab[j][act][k] = (act < A && k < K) ? row_val(m, b, act, k, s) : 0.0;
      }
      ext_split(er[j], 0, &manA[s], &expA[s]);  // Z_T = exp(r)
    }
  }
  if (__syncthreads_or(nonfinite)) {  // NaN at every step (uniform over the workgroup)
    for (int t = 0; t < T; ++t)
      for (int s = tid; s < S; s += nt) hz_nan_state(a, b, t, s);
    if (tid == 0) a.status[b] = IRLMX_OK;
    return;
  }

  for (int it = 0; it < T; ++it) {
    const int t = T - 1 - it;
    const double* min_ = (it & 1) ? manB : manA;
    const int* ein = (it & 1) ? expB : expA;
    double* mout = (it & 1) ? manA : manB;
    int* eout = (it & 1) ? expA : expB;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int s = tid + j * nt;
      if (s < S) {
        double* out = a.pi + hz_pi_row(m, T, b, t, s);
        int E;
        double zsum;
        auto nbr = [&](int k) __attribute__((always_inline)) {
          if constexpr (kHoldNb) return nb[j][k];
          else return row_nbr(m, b, s, k);
        };
        if constexpr (REG)
          zsum = hz_row<kHzRegActions, KMAX, true>(K, A, er[j], min_, ein, nbr, any[j],
                                                   [&](int act, int k) { return tab[j][act][k]; }, out, &E);
        else
          zsum = hz_row<kMaxActions, KMAX, false>(K, A, er[j], min_, ein, nbr, any[j],
                                                  [&](int act, int k) { return row_val(m, b, act, k, s); }, out, &E);
        double zm;
        int ze;
        if (term[j]) ext_split(er[j], 0, &zm, &ze);  // absorbing: Z_t = exp(r), held
        else ext_split(zsum, E, &zm, &ze);
        mout[s] = zm;
        eout[s] = ze;
        if (t == 0 && a.log_z0) a.log_z0[(size_t)b * S + s] = hz_log_z(zm, ze);
      }
    }
    __syncthreads();
  }
  if (tid == 0) a.status[b] = IRLMX_OK;
}

// d_t ping-pongs in LDS, D in registers; the weights are folded from pi_t
// every step (nothing is held between steps but D)
template <int SPT>
__global__ void __launch_bounds__(1024) hz_fwd_fused_kernel(HzFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hz_smem[];
  const Model& m = a.m;
  const int S = m.S, T = a.T;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  double* dA = (double*)hz_smem;
  double* dB = dA + S;
  const uint8_t* tb = a.term ? a.term + (size_t)b * S : nullptr;
  double* marg = a.svf_t ? a.svf_t + (size_t)b * (T + 1) * S : nullptr;

  double D[SPT];
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tid + j * nt;
    D[j] = 0.0;
    if (s < S) {
      D[j] = a.p0[(size_t)b * S + s];
      dA[s] = D[j];
      if (marg) marg[s] = D[j];
    }
  }
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const double* din = (t & 1) ? dB : dA;
    double* dout = (t & 1) ? dA : dB;
    const double* pit = a.pi + hz_pi_row(m, T, b, t, 0);
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int s = tid + j * nt;
      if (s < S) {
        const double nd = hz_fwd_state(m, b, s, pit, tb, din);
        dout[s] = nd;
        D[j] = __dadd_rn(D[j], nd);
        if (marg) marg[(size_t)(t + 1) * S + s] = nd;
      }
    }
    __syncthreads();
  }
  int nonfinite = 0;
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = tid + j * nt;
    if (s < S) {
      a.svf[(size_t)b * S + s] = D[j];
      nonfinite |= !isfinite(D[j]);
    }
  }
  nonfinite = __syncthreads_or(nonfinite);
  if (tid == 0) a.status[b] = nonfinite ? IRLMX_NONFINITE : IRLMX_OK;
}

// ---------------------------------------------------------------------------
// per-sweep shape: one launch per step over all instances
// ---------------------------------------------------------------------------

__global__ void hz_bwd_init_kernel(HzBwdArgs a, HzWs ws) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (s >= a.m.S) return;
  const size_t i = (size_t)b * a.m.S + s;
  const double er = exp(a.reward[i]);
  if (!isfinite(er)) atomicOr(&ws.bad[b], 1);
  ext_split(er, 0, &ws.man[0][i], &ws.exp[0][i]);
  if (s == 0) a.status[b] = IRLMX_OK;
}

__global__ void __launch_bounds__(kSweepThreads) hz_bwd_step_kernel(HzBwdArgs a, HzWs ws, int t, int odd) {
  const Model& m = a.m;
  const int S = m.S;
  const int b = blockIdx.y;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  if (ws.bad[b]) { hz_nan_state(a, b, t, s); return; }
  const size_t i = (size_t)b * S + s;
  const double er = exp(a.reward[i]);
  int E;
  const double zsum = hz_row_loop(m, b, s, er, ws.man[odd] + (size_t)b * S, ws.exp[odd] + (size_t)b * S,
                                  a.pi + hz_pi_row(m, a.T, b, t, s), &E);
  double zm;
  int ze;
  if (a.term && a.term[i]) ext_split(er, 0, &zm, &ze);
  else ext_split(zsum, E, &zm, &ze);
  ws.man[odd ^ 1][i] = zm;
  ws.exp[odd ^ 1][i] = ze;
  if (t == 0 && a.log_z0) a.log_z0[i] = hz_log_z(zm, ze);
}

__global__ void hz_fwd_init_kernel(HzFwdArgs a, HzWs ws) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  const int S = a.m.S;
  if (s >= S) return;
  const size_t i = (size_t)b * S + s;
  const double p = a.p0[i];
  ws.man[0][i] = p;
  a.svf[i] = p;
  if (a.svf_t) a.svf_t[(size_t)b * (a.T + 1) * S + s] = p;
  if (s == 0) a.status[b] = IRLMX_OK;
}

__global__ void __launch_bounds__(kSweepThreads) hz_fwd_step_kernel(HzFwdArgs a, HzWs ws, int t, int odd) {
  const Model& m = a.m;
  const int S = m.S;
  const int b = blockIdx.y;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const size_t i = (size_t)b * S + s;
  const uint8_t* tb = a.term ? a.term + (size_t)b * S : nullptr;
  const double nd = hz_fwd_state(m, b, s, a.pi + hz_pi_row(m, a.T, b, t, 0), tb, ws.man[odd] + (size_t)b * S);
  ws.man[odd ^ 1][i] = nd;
  const double D = __dadd_rn(a.svf[i], nd);
  a.svf[i] = D;
  if (a.svf_t) a.svf_t[((size_t)b * (a.T + 1) + t + 1) * S + s] = nd;
  if (t == a.T - 1 && !isfinite(D)) atomicOr(&a.status[b], IRLMX_NONFINITE);
}

// ---------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------

// Pairs whose table values stay in registers (at most kHzRegActions actions).
static constexpr bool hz_pair_reg(int spt, int kmax) { return spt == 1 && kmax == 5; }

// (SPT, KMAX) pairs of the backward: the ordinary fused backward's list
// (fused_pair_ok), as the extended backward; every pair compiles without VGPR
// spills at __launch_bounds__(1024) (tools/kernel_resources.py; the table is in
// DESIGN.md section 4).
template <bool R_>
static void (*hz_bwd_fn(int spt, int kmax))(HzBwdArgs) {
  return with_pair<void (*)(HzBwdArgs)>(spt, kmax, [](auto s, auto k) {
    if constexpr (fused_pair_ok(IRLMX_OP_BACKWARD, s, k) && (!R_ || hz_pair_reg(s, k)))
      return &hz_bwd_fused_kernel<s, k, R_>;
    else return nullptr;
  });
}

static void (*hz_fwd_fn(int spt))(HzFwdArgs) {
  if (spt == 1) return &hz_fwd_fused_kernel<1>;
  if (spt == 2) return &hz_fwd_fused_kernel<2>;
  if (spt == 4) return &hz_fwd_fused_kernel<4>;
  return nullptr;
}

size_t hz_fused_lds(const Model& m, int op) {
  if (op == IRLMX_OP_BACKWARD_HORIZON) return (size_t)m.S * kExtLdsPerState;
  // (the forward's d_t and the value pass's v_t need no NpTables copy: 16 * S bytes)
  return (op == IRLMX_OP_SOFT_BACKWARD_HORIZON ? sizeof(NpTables) : 0) + 2 * (size_t)m.S * sizeof(double);
}

// Several states per thread (above 1,024 states) only from this many instances
// on (IRLMX_HORIZON_FUSED_BATCH; tests use 1): one workgroup steps 4,096 states
// in 24 us where a launch over 16 workgroups takes 11, so below one workgroup
// per CU the per-sweep shape is the faster one (measured, DESIGN.md section 4
// "Finite horizon": 64 x 64 fused / per sweep 2.2 at one instance, 1.5 at 64,
// 0.8 at 256; at one state per thread fused wins at every batch, 0.1 - 0.9).
int horizon_fused_min_batch() {
  const int forced_cus = env_int("IRLMX_PLAN_CUS", 0);
  const int cus = forced_cus > 0 ? forced_cus : device_cus();
  return env_int("IRLMX_HORIZON_FUSED_BATCH", cus > 0 ? cus : 256);
}

bool hz_fused_shape(const Model& m, int op, FusedShape* out) {
  // (the op whose fused_pair_ok list the kernels are instantiated from: the soft and the value pass have their own)
  const int pairs = op == IRLMX_OP_BACKWARD_HORIZON ? IRLMX_OP_BACKWARD : op == IRLMX_OP_FORWARD_HORIZON ? IRLMX_OP_FORWARD : op;
  if (!fused_shape(m, pairs, out, false)) return false;
  if (out->spt > 1 && m.B < horizon_fused_min_batch()) return false;
  return hz_fused_lds(m, op) <= kExtLdsMax;
}

HzWs hz_carve(const Model& m, int op, void* base) {
  HzWs w;
  Carver c{(char*)base};
  const size_t B = m.B, S = m.S;
  FusedShape fs;
  const bool sweep = !hz_fused_shape(m, op, &fs);
  const bool bwd = op == IRLMX_OP_BACKWARD_HORIZON;
  w.bad = c.take<int32_t>(sweep && bwd ? B * sizeof(int32_t) : 0);
  for (int i = 0; i < 2; ++i) w.man[i] = c.take<double>(sweep ? B * S * sizeof(double) : 0);
  for (int i = 0; i < 2; ++i) w.exp[i] = c.take<int32_t>(sweep && bwd ? B * S * sizeof(int32_t) : 0);
  w.total = c.total();
  return w;
}

int horizon_check_model(const Model& m, const char* fn) {
  if (m.dense) {
    set_error("%s: the finite-horizon passes do not run the DENSE layout (STENCIL5 and ELL only)", fn);
    return IRLMX_EINVAL;
  }
  return 0;
}

size_t horizon_workspace_bytes(const Model& m, int op) { return hz_carve(m, op, nullptr).total; }

void horizon_plan(const Model& m, int op, int64_t* plan) {
  FusedShape fs;
  if (hz_fused_shape(m, op, &fs)) return plan_fused(plan, fs, hz_fused_lds(m, op));
  plan_sweep(plan, 1, 0);  // one state per lane; the launch count is the horizon (the soft and the value pass's: + 1)
}

int hz_check_call(const Model& m, const char* fn, int op, int32_t horizon, size_t bytes, void* ws) {
  if (horizon < 1 || horizon > kHzMaxHorizon) {
    set_error("%s: horizon %d outside [1, %d]", fn, horizon, kHzMaxHorizon);
    return IRLMX_EINVAL;
  }
  return check_ws(horizon_workspace_bytes(m, op), bytes, ws);
}

}  // namespace irlmx

using namespace irlmx;

extern "C" int irlmx_backward_maxent_horizon(const irlmx_mdp* mdp, const double* reward, const uint8_t* terminal,
                                             int32_t horizon, double* p_action_t, double* log_z0, int32_t* status,
                                             void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "backward_maxent_horizon";
  if (int rc = validate(mdp)) return rc;
  const Model m = make_model(mdp);
  if (int rc = horizon_check_model(m, fn)) return rc;
  if (int rc = need_all(fn, {{reward, "reward"}, {p_action_t, "p_action_t"}, {status, "status"}})) return rc;
  if (int rc = hz_check_call(m, fn, IRLMX_OP_BACKWARD_HORIZON, horizon, workspace_bytes, workspace)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const HzBwdArgs a{m, reward, terminal, horizon, p_action_t, log_z0, status};
  return hz_launch(
      m, IRLMX_OP_BACKWARD_HORIZON, workspace, st, a, "horizon backward", "hz_bwd_fused_kernel",
      [&](const FusedShape& fs) {
        void (*kfn)(HzBwdArgs) = m.A <= kHzRegActions ? hz_bwd_fn<true>(fs.spt, fs.kmax) : nullptr;
        return kfn ? kfn : hz_bwd_fn<false>(fs.spt, fs.kmax);
      },
      [&](const HzWs& ws) {
        const hipError_t e = hipMemsetAsync(ws.bad, 0, (size_t)m.B * sizeof(int32_t), st);
        if (e != hipSuccess) return hip_fail(e, "workspace memset");
        return hz_launch_sweeps(m, hz_bwd_init_kernel, hz_bwd_step_kernel, a, ws, horizon, true, "horizon backward", st);
      });
}

extern "C" int irlmx_forward_svf_horizon(const irlmx_mdp* mdp, const double* p_initial, const uint8_t* terminal,
                                         const double* p_action_t, int32_t horizon, double* svf, double* svf_t,
                                         int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "forward_svf_horizon";
  if (int rc = validate(mdp)) return rc;
  const Model m = make_model(mdp);
  if (int rc = horizon_check_model(m, fn)) return rc;
  if (int rc = need_col_form(m)) return rc;
  if (int rc = need_all(fn, {{p_initial, "p_initial"}, {p_action_t, "p_action_t"}, {svf, "svf"}, {status, "status"}}))
    return rc;
  if (int rc = hz_check_call(m, fn, IRLMX_OP_FORWARD_HORIZON, horizon, workspace_bytes, workspace)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const HzFwdArgs a{m, p_initial, terminal, p_action_t, horizon, svf, svf_t, status};
  return hz_launch(
      m, IRLMX_OP_FORWARD_HORIZON, workspace, st, a, "horizon forward", "hz_fwd_fused_kernel",
      [&](const FusedShape& fs) { return hz_fwd_fn(fs.spt); },
      [&](const HzWs& ws) {
        return hz_launch_sweeps(m, hz_fwd_init_kernel, hz_fwd_step_kernel, a, ws, horizon, false, "horizon forward", st);
      });
}

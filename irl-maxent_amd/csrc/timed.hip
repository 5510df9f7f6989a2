// What consumes a time-indexed policy pi_t [B][T][S][A] on gfx950
// (include/irlmx_timed.h): rollouts of T steps (irlmx_rollout_horizon), the
// log-likelihood of stored demonstrations (irlmx_demo_log_likelihood_horizon)
// and the finite-horizon value of a reward (irlmx_value_horizon).
//
// The two trajectory calls are rollout.hip's with the policy row of step t read
// from pi_t[b][t]: one thread per trajectory, 256-thread workgroups, the
// generator, the pick rule and the guards shared through rollout.h.
//
// The value pass, from v_T(s) = r(s), for t = T-1 .. 0, per state s
// (include/irlmx_timed.h states the same order word for word):
//
//   1. per action a in index order, acc = fma(P[s, target_k(s), a], v_{t+1}(target_k(s)), acc)
//      from 0 over every stored slot in slot order (soft_horizon.hip's step 1)
//   2. with a policy: e = fma(pi_t(s, a), acc, e) from 0 in action order;
//      without one: q_a = r(s) + discount * acc, the product rounded before the
//      sum, and v = max_a q_a by irlmx_value_iteration's NaN rule
//   3. with a policy v_t(s) = r(s) + discount * e, the product rounded before
//      the sum; a terminal s holds v_t(s) = r(s) (absorbing)
//
// Two shapes, the same statements and so the same bits, routed and sized by
// horizon.h's machinery as it stands: fused -- one workgroup per instance for
// all T steps, v ping-pongs in LDS (16 * S bytes), one barrier per step -- and
// per sweep: one launch per step over all instances, v double-buffered in the
// caller's workspace; the launch count is T + 1, so the host never polls.  No
// exp / log: the fused kernels stage no NpTables.

#include <hip/hip_runtime.h>

#include "../../include/irlmx_timed.h"
#include "horizon.h"
#include "rollout.h"

namespace irlmx {

// ---------------------------------------------------------------------------
// rollouts of T steps under pi_t
// ---------------------------------------------------------------------------

struct TpRollArgs {
  Model m;
  const double* pi;     // [B][T][S][A]
  const uint8_t* term;  // may be null
  const int32_t* start;
  const uint64_t* seed;
  int N, T;
  int64_t* visits;
  int64_t* starts;
  int32_t* lengths;
  int32_t* status;
  int32_t* states;   // [B][N][T + 1] or null
  int32_t* actions;  // [B][N][T] or null (with states)
};

// rollout_kernel (rollout.hip) with max_len = T, the policy row of step t and an optional terminal mask
__global__ void __launch_bounds__(kRollThreads) tp_rollout_kernel(TpRollArgs a) {
  const Model& m = a.m;
  const long long tid = (long long)blockIdx.x * kRollThreads + threadIdx.x;
  if (tid >= (long long)m.B * a.N) return;
  const int b = (int)(tid / a.N), n = (int)(tid % a.N);
  const int S = m.S, A = m.A, K = m.K, T = a.T;
  int s = a.start[tid];
  if (s < 0 || s >= S) {
    a.lengths[tid] = 0;
    a.status[tid] = IRLMX_TRAJ_BAD_INDEX;
    return;
  }
  const size_t row = (size_t)b * S;
  int32_t* st_out = a.states ? a.states + (size_t)tid * ((size_t)T + 1) : nullptr;
  int32_t* ac_out = a.states ? a.actions + (size_t)tid * (size_t)T : nullptr;
  count(a.starts, row + s);
  if (st_out) st_out[0] = s;
  int len = 0, status = IRLMX_TRAJ_OK;
  if (!(a.term && a.term[row + s])) {
    const uint64_t seed = a.seed[b];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    status = IRLMX_TRAJ_TRUNCATED;
    for (int t = 0; t < T; ++t) {
      count(a.visits, row + s);
      const Philox r = philox4x32_10((uint32_t)t, (uint32_t)n, 0u, 0u, k0, k1);
      const double* pis = a.pi + hz_pi_row(m, T, b, t, s);
      const int act = pick(uniform53(r.x[0], r.x[1]), A, [&](int j) { return pis[j]; });
      if (act < 0) { status = IRLMX_TRAJ_BAD_POLICY; break; }
      const int k = pick(uniform53(r.x[2], r.x[3]), K, [&](int j) { return row_val(m, b, act, j, s); });
      if (k < 0) { status = IRLMX_TRAJ_BAD_TABLE; break; }
      const int nxt = m.stencil ? stencil_nbr(s, k, m.W, m.H) : m.row_idx[(inst_of(m, b) * K + k) * S + s];
      if (nxt < 0 || nxt >= S) { status = IRLMX_TRAJ_BAD_TABLE; break; }
      if (st_out) { ac_out[t] = act; st_out[t + 1] = nxt; }
      ++len;
      s = nxt;
      if (a.term && a.term[row + s]) { status = IRLMX_TRAJ_OK; break; }
    }
  }
  count(a.visits, row + s);  // the final state, whatever stopped the trajectory
  a.lengths[tid] = len;
  a.status[tid] = status;
}

// ---------------------------------------------------------------------------
// stored trajectories under pi_t: states [B][N][stride], actions [B][N][stride - 1]
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(kRollThreads)
tp_ll_traj_kernel(int S, int A, int B, int N, int stride, int T, const double* __restrict__ pi,
                  const int32_t* __restrict__ states, const int32_t* __restrict__ actions,
                  const int32_t* __restrict__ lengths, double* ll_traj, int32_t* status) {
  const long long tid = (long long)blockIdx.x * kRollThreads + threadIdx.x;
  if (tid >= (long long)B * N) return;
  const int32_t* st = states + (size_t)tid * stride;
  const int32_t* ac = actions + (size_t)tid * (stride - 1);
  const int len = lengths[tid];
  if (len > T || !traj_ok(st, ac, len, stride, S, A)) {  // (step t reads pi_t[t]: there is none beyond T - 1)
    status[tid] = IRLMX_TRAJ_BAD_INDEX;
    ll_traj[tid] = kNaN;
    return;
  }
  const double* pib = pi + (size_t)(tid / N) * T * S * A;
  double ll = 0.0;
  for (int t = 0; t < len; ++t) ll = __dadd_rn(ll, np_log(pib[((size_t)t * S + st[t]) * A + ac[t]]));
  ll_traj[tid] = ll;
  status[tid] = IRLMX_TRAJ_OK;
}

// ll[b] = the sequential sum of ll_traj[b][0..N): rollout.h's ll_sum under this file's kernel name
__global__ void __launch_bounds__(kRollThreads)
tp_ll_sum_kernel(int B, int N, const double* __restrict__ ll_traj, double* ll) {
  ll_sum(B, N, ll_traj, ll);
}

// ---------------------------------------------------------------------------
// the value pass
// ---------------------------------------------------------------------------

struct TpValueArgs {
  Model m;
  const double* reward;
  const uint8_t* term;  // may be null
  const double* pi;     // [B][T][S][A], null: the optimal value
  double discount;
  int T;
  double* value0;   // [B][S]
  double* value_t;  // [B][T + 1][S], may be null
  int32_t* status;
};

// per-sweep buffers (the fused kernel keeps v in LDS): hz_carve's man[0..1]
struct TpWs {
  double* v[2];  // [B][S] ping and pong
  size_t total;
};

// One state of one step (steps 1 - 3 above; the terminal rule is the caller's).
// `pis`: the policy row pi_t(s, :) or null.  KMAX as in soft_horizon.hip's
// sh_row: > 0 the slot class is compiled in and up to 8 slots unrolled, 0 (per
// sweep: any K) and from 16 slots on the slot loop is rolled.
template <int KMAX, class Nbr>
__device__ __attribute__((always_inline)) inline double tp_row(const Model& m, int b, int s, double r, double discount,
                                                               const double* vin, Nbr&& nbr, const double* pis) {
  const int K = m.K, A = m.A;
  double v = 0.0;  // the running maximum, or the policy's expectation e
#pragma unroll 1
  for (int act = 0; act < A; ++act) {
    double acc = 0.0;
    if constexpr (KMAX > 0 && KMAX <= 8) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) acc = fma(row_val(m, b, act, k, s), vin[nbr(k)], acc);
    } else {
#pragma unroll 1
      for (int k = 0; k < K; ++k) acc = fma(row_val(m, b, act, k, s), vin[nbr(k)], acc);
    }
    if (pis) {
      v = fma(pis[act], acc, v);
    } else {
      const double q = __dadd_rn(r, __dmul_rn(discount, acc));
      v = act == 0 ? q : ((v != v || q <= v) ? v : q);  // irlmx_value_iteration's maximum
    }
  }
  return pis ? __dadd_rn(r, __dmul_rn(discount, v)) : v;
}

__device__ inline void tp_store(const TpValueArgs& a, int b, int t, int s, double v) {
  const int S = a.m.S;
  if (a.value_t) a.value_t[((size_t)b * (a.T + 1) + t) * S + s] = v;
  if (t == 0) a.value0[(size_t)b * S + s] = v;
}

// fused shape: one workgroup per instance for all T steps
template <int SPT, int KMAX>
__global__ void __launch_bounds__(1024) tp_value_fused_kernel(TpValueArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tp_smem[];
  const Model& m = a.m;
  const int S = m.S, K = m.K, T = a.T;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  double* vA = (double*)tp_smem;
  double* vB = vA + S;

  // soft_horizon.hip's register plan: up to 10 neighbour indices per thread
  // stay in registers with the reward and the terminal flag; beyond that the
  // state loop is rolled and everything per state is read at its use.
  constexpr bool kHold = SPT * KMAX <= 10;
  double r[kHold ? SPT : 1];
  bool term[kHold ? SPT : 1];
  int nb[kHold ? SPT : 1][kHold ? KMAX : 1];
  if constexpr (kHold) {
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int s = tid + j * nt;
      r[j] = 0.0;
      term[j] = false;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) nb[j][k] = 0;
      if (s < S) {
        r[j] = a.reward[(size_t)b * S + s];
        term[j] = a.term && a.term[(size_t)b * S + s] != 0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (k < K) nb[j][k] = row_nbr(m, b, s, k);
      }
    }
  }
  for (int s = tid; s < S; s += nt) {  // v_T = r
    const double rs = a.reward[(size_t)b * S + s];
    vA[s] = rs;
    if (a.value_t) a.value_t[((size_t)b * (T + 1) + T) * S + s] = rs;
  }
  __syncthreads();

  int nonfinite = 0;
  for (int it = 0; it < T; ++it) {
    const int t = T - 1 - it;
    const double* vin = (it & 1) ? vB : vA;
    double* vout = (it & 1) ? vA : vB;
    auto state = [&](int s, double rs, bool ts, auto&& nbr) __attribute__((always_inline)) {
      double v = tp_row<KMAX>(m, b, s, rs, a.discount, vin, nbr, a.pi ? a.pi + hz_pi_row(m, T, b, t, s) : nullptr);
      if (ts) v = rs;  // absorbing: v_t = r, held
      vout[s] = v;
      tp_store(a, b, t, s, v);
      if (t == 0) nonfinite |= !isfinite(v);
    };
    if constexpr (kHold) {
#pragma unroll
      for (int j = 0; j < SPT; ++j) {
        const int s = tid + j * nt;
        if (s < S) state(s, r[j], term[j], [&](int k) __attribute__((always_inline)) { return nb[j][k]; });
      }
    } else {
#pragma unroll 1
      for (int s = tid; s < S; s += nt)
        state(s, a.reward[(size_t)b * S + s], a.term && a.term[(size_t)b * S + s] != 0,
              [&](int k) __attribute__((always_inline)) { return row_nbr(m, b, s, k); });
    }
    __syncthreads();
  }
  nonfinite = __syncthreads_or(nonfinite);
  if (tid == 0) a.status[b] = nonfinite ? IRLMX_NONFINITE : IRLMX_OK;
}

// per-sweep shape: one launch per step over all instances
__global__ void tp_value_init_kernel(TpValueArgs a, TpWs ws) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  const int S = a.m.S;
  if (s >= S) return;
  const size_t i = (size_t)b * S + s;
  const double r = a.reward[i];
  ws.v[0][i] = r;
  if (a.value_t) a.value_t[((size_t)b * (a.T + 1) + a.T) * S + s] = r;
  if (s == 0) a.status[b] = IRLMX_OK;
}

__global__ void __launch_bounds__(kSweepThreads) tp_value_step_kernel(TpValueArgs a, TpWs ws, int t, int odd) {
  const Model& m = a.m;
  const int S = m.S;
  const int b = blockIdx.y;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const size_t i = (size_t)b * S + s;
  const double r = a.reward[i];
  double v = tp_row<0>(m, b, s, r, a.discount, ws.v[odd] + (size_t)b * S,
                       [&](int k) __attribute__((always_inline)) { return row_nbr(m, b, s, k); },
                       a.pi ? a.pi + hz_pi_row(m, a.T, b, t, s) : nullptr);
  if (a.term && a.term[i]) v = r;
  ws.v[odd ^ 1][i] = v;
  tp_store(a, b, t, s, v);
  if (t == 0 && !isfinite(v)) atomicOr(&a.status[b], IRLMX_NONFINITE);
}

// fused_pair_ok(IRLMX_OP_VALUE_HORIZON, ..) is the instantiation list
// (fixed_point.h): the soft horizon pass's eight pairs.
static void (*tp_value_fn(int spt, int kmax))(TpValueArgs) {
  return with_pair<void (*)(TpValueArgs)>(spt, kmax, [](auto s, auto k) {
    if constexpr (fused_pair_ok(IRLMX_OP_VALUE_HORIZON, s, k)) return &tp_value_fused_kernel<s, k>;
    else return nullptr;
  });
}

// STENCIL5 / ELL, n_traj and the horizon of the two trajectory calls
static int tp_check_traj(const Model& m, const char* fn, int n_traj, int horizon) {
  if (int rc = horizon_check_model(m, fn)) return rc;
  if (n_traj < 1) { set_error("%s: n_traj=%d < 1", fn, n_traj); return IRLMX_EINVAL; }
  if (horizon < 1 || horizon > kHzMaxHorizon) {
    set_error("%s: horizon %d outside [1, %d]", fn, horizon, kHzMaxHorizon);
    return IRLMX_EINVAL;
  }
  return 0;
}

}  // namespace irlmx

using namespace irlmx;

extern "C" int irlmx_rollout_horizon(const irlmx_mdp* mdp, const double* p_action_t, const uint8_t* terminal,
                                     const int32_t* start, const uint64_t* seed, int32_t n_traj, int32_t horizon,
                                     int64_t* visits, int64_t* starts, int32_t* lengths, int32_t* traj_status,
                                     int32_t* states, int32_t* actions, void* stream) {
  const char* fn = "rollout_horizon";
  if (int rc = validate(mdp)) return rc;
  const Model m = make_model(mdp);
  if (int rc = tp_check_traj(m, fn, n_traj, horizon)) return rc;
  if (int rc = need_all(fn, {{p_action_t, "p_action_t"}, {start, "start"}, {seed, "seed"}, {visits, "visits"},
                             {starts, "starts"}, {lengths, "lengths"}, {traj_status, "traj_status"}}))
    return rc;
  if ((states == nullptr) != (actions == nullptr)) {
    set_error("%s: states and actions must both be NULL or both be set", fn);
    return IRLMX_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t hist = (size_t)m.B * m.S * sizeof(int64_t);
  hipError_t e = hipMemsetAsync(visits, 0, hist, st);
  if (e == hipSuccess) e = hipMemsetAsync(starts, 0, hist, st);
  if (e != hipSuccess) return hip_fail(e, "rollout_horizon memset");
  TpRollArgs a{m, p_action_t, terminal, start, seed, n_traj, horizon, visits, starts, lengths, traj_status, states, actions};
  hipLaunchKernelGGL(tp_rollout_kernel, dim3(traj_blocks((long long)m.B * n_traj)), dim3(kRollThreads), 0, st, a);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, "tp_rollout_kernel");
}

extern "C" int irlmx_demo_log_likelihood_horizon(int32_t n_states, int32_t n_actions, int32_t batch, int32_t n_traj,
                                                 int32_t stride, int32_t horizon, const double* p_action_t,
                                                 const int32_t* states, const int32_t* actions, const int32_t* lengths,
                                                 double* ll_traj, double* ll, int32_t* traj_status, void* stream) {
  const char* fn = "demo_log_likelihood_horizon";
  if (int rc = check_demo_sizes(fn, n_states, n_actions, batch, n_traj, stride)) return rc;
  if (horizon < 1 || horizon > kHzMaxHorizon) {
    set_error("%s: horizon %d outside [1, %d]", fn, horizon, kHzMaxHorizon);
    return IRLMX_EINVAL;
  }
  if (int rc = need_all(fn, {{p_action_t, "p_action_t"}, {states, "states"}, {actions, "actions"}, {lengths, "lengths"},
                             {ll_traj, "ll_traj"}, {ll, "ll"}, {traj_status, "traj_status"}}))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tp_ll_traj_kernel, dim3(traj_blocks((long long)batch * n_traj)), dim3(kRollThreads), 0, st, n_states,
                     n_actions, batch, n_traj, stride, horizon, p_action_t, states, actions, lengths, ll_traj,
                     traj_status);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "tp_ll_traj_kernel");
  hipLaunchKernelGGL(tp_ll_sum_kernel, dim3(traj_blocks(batch)), dim3(kRollThreads), 0, st, batch, n_traj, ll_traj, ll);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, "tp_ll_sum_kernel");
}

extern "C" int irlmx_value_horizon(const irlmx_mdp* mdp, const double* reward, const uint8_t* terminal,
                                   const double* p_action_t, double discount, int32_t horizon, double* value0,
                                   double* value_t, int32_t* status, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  const char* fn = "value_horizon";
  if (int rc = validate(mdp)) return rc;
  const Model m = make_model(mdp);
  if (int rc = horizon_check_model(m, fn)) return rc;
  if (int rc = need_all(fn, {{reward, "reward"}, {value0, "value0"}, {status, "status"}})) return rc;
  if (!(discount >= 0.0 && discount <= 1.0)) {  // NaN too
    set_error("%s: discount %g outside [0, 1]", fn, discount);
    return IRLMX_EINVAL;
  }
  if (int rc = hz_check_call(m, fn, IRLMX_OP_VALUE_HORIZON, horizon, workspace_bytes, workspace)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const TpValueArgs a{m, reward, terminal, p_action_t, discount, horizon, value0, value_t, status};
  return hz_launch(
      m, IRLMX_OP_VALUE_HORIZON, workspace, st, a, "horizon value", "tp_value_fused_kernel",
      [&](const FusedShape& fs) { return tp_value_fn(fs.spt, fs.kmax); },
      [&](const HzWs& w) {
        const TpWs ws{{w.man[0], w.man[1]}, w.total};
        return hz_launch_sweeps(m, tp_value_init_kernel, tp_value_step_kernel, a, ws, horizon, true, "horizon value",
                                st);
      });
}

// Demonstrations on gfx950, under a stationary policy pi [B][S][A] or a
// time-indexed one pi_t [B][T][S][A] (include/irlmx_timed.h): policy rollouts
// (irlmx_rollout, irlmx_rollout_horizon), the visit / start statistics of stored
// trajectories (irlmx_demo_statistics) and their log-likelihood under a policy
// (irlmx_demo_log_likelihood, irlmx_demo_log_likelihood_horizon).
//
// The rules below hold for both policy kinds: the kernels are templates on
// `TIMED`, and a time-indexed call differs in three places only -- step t reads
// its policy row from pi_t[b][t], the terminal mask may be null, and a stored
// trajectory longer than T is refused (there is no pi_t beyond T - 1).
//
// One thread per trajectory (b, n), 256-thread workgroups over B * N, a loop of
// at most max_len steps per thread.  Threads share nothing but integer
// atomicAdds into visits / starts: integer sums are order-free, so the counts
// do not depend on the schedule.  No persistent kernel, no cross-workgroup
// protocol, every loop bounded by an argument the host checked.
//
// Random numbers: Philox4x32-10, one block per step, counter (t, n, 0, 0), key
// (low, high 32 bits of seed[b]) -- the stream of a trajectory depends on its
// instance's seed, its index n and its step t only, not on the batch or the
// launch geometry.  Output words x0..x3 give the step's two uniforms as numpy
// builds a double from two 32-bit words:
//
//   u_action = ((x1 >> 5) * 2^26 + (x0 >> 6)) * 2^-53
//   u_next   = ((x3 >> 5) * 2^26 + (x2 >> 6)) * 2^-53
//
// pick(u, w[0..n)) draws index j with probability w_j / sum(w) (the same rule
// for the action, from the policy row, and the successor slot, from the table
// row of the drawn action): total = the sequential sum in index order (rounded
// adds); the row is invalid if an entry is negative or NaN or total is not a
// positive finite number; x = u * total (rounded); the result is the first j
// with x < c_j, c_j the same running sums -- or, when x rounded up to total,
// the last j with w_j > 0.  The compare is strict, so a slot of weight 0 (an
// off-grid stencil slot, an unused ELL slot) is never drawn.  Rows need not be
// normalised.  tests/rollout_twin.py restates all of it in numpy; the GPU
// tests compare bit for bit ("Demonstrations").
//
// The index guards (start states, ELL targets, stored states / actions,
// lengths) are always on, in every build: a bad index ends its trajectory with
// IRLMX_TRAJ_BAD_INDEX / _BAD_TABLE and is never used as an index.  The
// kernels are latency bound; the compares cost nothing measurable.

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/irlmx_timed.h"
#include "common.h"
#include "horizon.h"  // hz_pi_row, kHzMaxHorizon, horizon_check_model

namespace irlmx {

constexpr int kRollThreads = 256;
constexpr int kRollMaxLen = 1 << 20;

struct Philox {
  uint32_t x[4];
};

__host__ __device__ inline Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox{{c0, c1, c2, c3}};
}

// 53 random bits from two words, as numpy's next_double: [0, 1), exact in float64
__host__ __device__ inline double uniform53(uint32_t lo_word, uint32_t hi_word) {
  return ((double)(hi_word >> 5) * 67108864.0 + (double)(lo_word >> 6)) * 0x1p-53;
}

// The pick rule (above) over w(0) .. w(n - 1); -1 for an invalid row.
template <class Weight>
__device__ inline int pick(double u, int n, Weight&& w) {
  double total = 0.0;
  bool ok = true;
  for (int j = 0; j < n; ++j) {
    const double wj = w(j);
    ok = ok && wj >= 0.0;  // (false for a NaN)
    total = __dadd_rn(total, wj);
  }
  if (!ok || !(total > 0.0) || isinf(total)) return -1;
  const double x = __dmul_rn(u, total);
  double c = 0.0;
  int last = -1;
  for (int j = 0; j < n; ++j) {
    const double wj = w(j);
    c = __dadd_rn(c, wj);
    if (x < c) return j;
    if (wj > 0.0) last = j;
  }
  return last;
}

__device__ inline void count(int64_t* hist, size_t i) { atomicAdd((unsigned long long*)hist + i, 1ull); }

struct RollArgs {
  Model m;
  const double* pi;     // [B][S][A]; TIMED: [B][max_len][S][A]
  const uint8_t* term;  // TIMED: may be null
  const int32_t* start;
  const uint64_t* seed;
  int N, max_len;  // TIMED: max_len is the horizon T
  int64_t* visits;
  int64_t* starts;
  int32_t* lengths;
  int32_t* status;
  int32_t* states;   // [B][N][max_len + 1] or null
  int32_t* actions;  // [B][N][max_len] or null (with states)
};

template <bool TIMED>
__global__ void __launch_bounds__(kRollThreads) rollout_kernel(RollArgs a) {
  const Model& m = a.m;
  const long long tid = (long long)blockIdx.x * kRollThreads + threadIdx.x;
  if (tid >= (long long)m.B * a.N) return;
  const int b = (int)(tid / a.N), n = (int)(tid % a.N);
  const int S = m.S, A = m.A, K = m.K;
  int s = a.start[tid];
  if (s < 0 || s >= S) {
    a.lengths[tid] = 0;
    a.status[tid] = IRLMX_TRAJ_BAD_INDEX;
    return;
  }
  const size_t row = (size_t)b * S;
  auto terminal = [&](int at) {
    if constexpr (TIMED) return a.term && a.term[row + at];
    else return a.term[row + at] != 0;
  };
  int32_t* st_out = a.states ? a.states + (size_t)tid * ((size_t)a.max_len + 1) : nullptr;
  int32_t* ac_out = a.states ? a.actions + (size_t)tid * (size_t)a.max_len : nullptr;
  count(a.starts, row + s);
  if (st_out) st_out[0] = s;
  int len = 0, status = IRLMX_TRAJ_OK;
  if (!terminal(s)) {
    const uint64_t seed = a.seed[b];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    status = IRLMX_TRAJ_TRUNCATED;
    for (int t = 0; t < a.max_len; ++t) {
      count(a.visits, row + s);
      const Philox r = philox4x32_10((uint32_t)t, (uint32_t)n, 0u, 0u, k0, k1);
      const double* pis = a.pi + (TIMED ? hz_pi_row(m, a.max_len, b, t, s) : (row + s) * A);
      const int act = pick(uniform53(r.x[0], r.x[1]), A, [&](int j) { return pis[j]; });
      if (act < 0) { status = IRLMX_TRAJ_BAD_POLICY; break; }
      const int k = pick(uniform53(r.x[2], r.x[3]), K, [&](int j) { return row_val(m, b, act, j, s); });
      if (k < 0) { status = IRLMX_TRAJ_BAD_TABLE; break; }
      const int nxt = m.stencil ? stencil_nbr(s, k, m.W, m.H) : m.row_idx[(inst_of(m, b) * K + k) * S + s];
      if (nxt < 0 || nxt >= S) { status = IRLMX_TRAJ_BAD_TABLE; break; }
      if (st_out) { ac_out[t] = act; st_out[t + 1] = nxt; }
      ++len;
      s = nxt;
      if (terminal(s)) { status = IRLMX_TRAJ_OK; break; }
    }
  }
  count(a.visits, row + s);  // the final state (trajectory.py:43), whatever stopped the trajectory
  a.lengths[tid] = len;
  a.status[tid] = status;
}

// ---------------------------------------------------------------------------
// stored trajectories: states [B][N][stride], actions [B][N][stride - 1]
// ---------------------------------------------------------------------------

// Whether trajectory `tid` can be read: its length in [0, stride - 1], states
// 0..len in [0, S) and (actions non-null) actions 0..len - 1 in [0, A).
__device__ inline bool traj_ok(const int32_t* st, const int32_t* ac, int len, int stride, int S, int A) {
  if (len < 0 || len > stride - 1) return false;
  bool ok = true;
  for (int t = 0; t <= len; ++t) ok = ok && st[t] >= 0 && st[t] < S;
  if (ac)
    for (int t = 0; t < len; ++t) ok = ok && ac[t] >= 0 && ac[t] < A;
  return ok;
}

__global__ void __launch_bounds__(kRollThreads)
demo_statistics_kernel(int S, int B, int N, int stride, const int32_t* __restrict__ states,
                       const int32_t* __restrict__ lengths, int64_t* visits, int64_t* starts, int32_t* status) {
  const long long tid = (long long)blockIdx.x * kRollThreads + threadIdx.x;
  if (tid >= (long long)B * N) return;
  const int32_t* st = states + (size_t)tid * stride;
  const int len = lengths[tid];
  if (!traj_ok(st, nullptr, len, stride, S, 0)) {  // nothing of a bad trajectory is counted
    status[tid] = IRLMX_TRAJ_BAD_INDEX;
    return;
  }
  const size_t row = (size_t)(tid / N) * S;
  count(starts, row + st[0]);
  for (int t = 0; t <= len; ++t) count(visits, row + st[t]);
  status[tid] = IRLMX_TRAJ_OK;
}

// `pi` is [B][S][A] and T unused, or (TIMED) [B][T][S][A]: step t reads pi_t[t]
template <bool TIMED>
__global__ void __launch_bounds__(kRollThreads)
demo_ll_traj_kernel(int S, int A, int B, int N, int stride, int T, const double* __restrict__ pi,
                    const int32_t* __restrict__ states, const int32_t* __restrict__ actions,
                    const int32_t* __restrict__ lengths, double* ll_traj, int32_t* status) {
  const long long tid = (long long)blockIdx.x * kRollThreads + threadIdx.x;
  if (tid >= (long long)B * N) return;
  const int32_t* st = states + (size_t)tid * stride;
  const int32_t* ac = actions + (size_t)tid * (stride - 1);
  const int len = lengths[tid];
  if ((TIMED && len > T) || !traj_ok(st, ac, len, stride, S, A)) {  // (there is no pi_t beyond T - 1)
    status[tid] = IRLMX_TRAJ_BAD_INDEX;
    ll_traj[tid] = kNaN;
    return;
  }
  const size_t step = TIMED ? (size_t)S : 0;  // states between the rows of steps t and t + 1
  const double* pib = pi + (size_t)(tid / N) * (TIMED ? T : 1) * S * A;
  double ll = 0.0;
  for (int t = 0; t < len; ++t) ll = __dadd_rn(ll, np_log(pib[(t * step + st[t]) * A + ac[t]]));
  ll_traj[tid] = ll;
  status[tid] = IRLMX_TRAJ_OK;
}

// ll[b] = the sequential sum of ll_traj[b][0..N): one thread per instance
__global__ void __launch_bounds__(kRollThreads)
demo_ll_sum_kernel(int B, int N, const double* __restrict__ ll_traj, double* ll) {
  const int b = blockIdx.x * kRollThreads + threadIdx.x;
  if (b >= B) return;
  double acc = 0.0;
  for (int n = 0; n < N; ++n) acc = __dadd_rn(acc, ll_traj[(size_t)b * N + n]);
  ll[b] = acc;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

static unsigned traj_blocks(long long n) { return (unsigned)((n + kRollThreads - 1) / kRollThreads); }

// n_states / n_actions / batch / n_traj / stride of the calls on stored trajectories
static int check_demo_sizes(const char* fn, int S, int A, int B, int N, int stride) {
  if (S < 1 || A < 1 || B < 1) {
    set_error("%s: bad sizes S=%d A=%d B=%d", fn, S, A, B);
    return IRLMX_EINVAL;
  }
  if (N < 1) { set_error("%s: n_traj=%d < 1", fn, N); return IRLMX_EINVAL; }
  if (stride < 1) { set_error("%s: stride=%d < 1", fn, stride); return IRLMX_EINVAL; }
  return 0;
}

// What the two rollout calls do once their arguments are checked: the last
// check (states and actions), the histograms zeroed, one launch.
template <bool TIMED>
static int run_rollout(const char* fn, const RollArgs& a, hipStream_t st) {
  if ((a.states == nullptr) != (a.actions == nullptr)) {
    set_error("%s: states and actions must both be NULL or both be set", fn);
    return IRLMX_EINVAL;
  }
  const size_t hist = (size_t)a.m.B * a.m.S * sizeof(int64_t);
  hipError_t e = hipMemsetAsync(a.visits, 0, hist, st);
  if (e == hipSuccess) e = hipMemsetAsync(a.starts, 0, hist, st);
  if (e != hipSuccess) return hip_fail(e, (std::string(fn) + " memset").c_str());
  hipLaunchKernelGGL(rollout_kernel<TIMED>, dim3(traj_blocks((long long)a.m.B * a.N)), dim3(kRollThreads), 0, st, a);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, "rollout_kernel");
}

// The two log-likelihood calls after their checks: per trajectory, then per instance.
template <bool TIMED>
static int run_demo_ll(int S, int A, int B, int N, int stride, int T, const double* pi, const int32_t* states,
                       const int32_t* actions, const int32_t* lengths, double* ll_traj, double* ll, int32_t* status,
                       hipStream_t st) {
  hipLaunchKernelGGL(demo_ll_traj_kernel<TIMED>, dim3(traj_blocks((long long)B * N)), dim3(kRollThreads), 0, st, S, A,
                     B, N, stride, T, pi, states, actions, lengths, ll_traj, status);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "demo_ll_traj_kernel");
  hipLaunchKernelGGL(demo_ll_sum_kernel, dim3(traj_blocks(B)), dim3(kRollThreads), 0, st, B, N, ll_traj, ll);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, "demo_ll_sum_kernel");
}

static int check_horizon(const char* fn, int horizon) {
  if (horizon < 1 || horizon > kHzMaxHorizon) {
    set_error("%s: horizon %d outside [1, %d]", fn, horizon, kHzMaxHorizon);
    return IRLMX_EINVAL;
  }
  return 0;
}

}  // namespace irlmx

using namespace irlmx;

extern "C" int irlmx_rollout(const irlmx_mdp* mdp, const double* p_action, const uint8_t* terminal,
                             const int32_t* start, const uint64_t* seed, int32_t n_traj, int32_t max_len,
                             int64_t* visits, int64_t* starts, int32_t* lengths, int32_t* traj_status,
                             int32_t* states, int32_t* actions, void* stream) {
  if (int rc = validate(mdp)) return rc;
  const Model m = make_model(mdp);
  if (m.dense) {
    set_error("rollout: rollouts do not run the DENSE layout (STENCIL5 and ELL only)");
    return IRLMX_EINVAL;
  }
  if (int rc = need_all("rollout", {{p_action, "p_action"}, {terminal, "terminal"}, {start, "start"}, {seed, "seed"},
                                    {visits, "visits"}, {starts, "starts"}, {lengths, "lengths"},
                                    {traj_status, "traj_status"}}))
    return rc;
  if (n_traj < 1) { set_error("rollout: n_traj=%d < 1", n_traj); return IRLMX_EINVAL; }
  if (max_len < 1 || max_len > kRollMaxLen) {
    set_error("rollout: max_len=%d outside [1, %d]", max_len, kRollMaxLen);
    return IRLMX_EINVAL;
  }
  return run_rollout<false>("rollout", {m, p_action, terminal, start, seed, n_traj, max_len, visits, starts, lengths,
                                        traj_status, states, actions}, (hipStream_t)stream);
}

extern "C" int irlmx_rollout_horizon(const irlmx_mdp* mdp, const double* p_action_t, const uint8_t* terminal,
                                     const int32_t* start, const uint64_t* seed, int32_t n_traj, int32_t horizon,
                                     int64_t* visits, int64_t* starts, int32_t* lengths, int32_t* traj_status,
                                     int32_t* states, int32_t* actions, void* stream) {
  const char* fn = "rollout_horizon";
  if (int rc = validate(mdp)) return rc;
  const Model m = make_model(mdp);
  if (int rc = horizon_check_model(m, fn)) return rc;
  if (n_traj < 1) { set_error("%s: n_traj=%d < 1", fn, n_traj); return IRLMX_EINVAL; }
  if (int rc = check_horizon(fn, horizon)) return rc;
  if (int rc = need_all(fn, {{p_action_t, "p_action_t"}, {start, "start"}, {seed, "seed"}, {visits, "visits"},
                             {starts, "starts"}, {lengths, "lengths"}, {traj_status, "traj_status"}}))
    return rc;
  return run_rollout<true>(fn, {m, p_action_t, terminal, start, seed, n_traj, horizon, visits, starts, lengths,
                                traj_status, states, actions}, (hipStream_t)stream);
}

extern "C" int irlmx_demo_statistics(int32_t n_states, int32_t batch, int32_t n_traj, int32_t stride,
                                     const int32_t* states, const int32_t* lengths, int64_t* visits, int64_t* starts,
                                     int32_t* traj_status, void* stream) {
  if (int rc = check_demo_sizes("demo_statistics", n_states, 1, batch, n_traj, stride)) return rc;
  if (int rc = need_all("demo_statistics", {{states, "states"}, {lengths, "lengths"}, {visits, "visits"},
                                            {starts, "starts"}, {traj_status, "traj_status"}}))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t hist = (size_t)batch * n_states * sizeof(int64_t);
  hipError_t e = hipMemsetAsync(visits, 0, hist, st);
  if (e == hipSuccess) e = hipMemsetAsync(starts, 0, hist, st);
  if (e != hipSuccess) return hip_fail(e, "demo_statistics memset");
  hipLaunchKernelGGL(demo_statistics_kernel, dim3(traj_blocks((long long)batch * n_traj)), dim3(kRollThreads), 0, st,
                     n_states, batch, n_traj, stride, states, lengths, visits, starts, traj_status);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, "demo_statistics_kernel");
}

extern "C" int irlmx_demo_log_likelihood(int32_t n_states, int32_t n_actions, int32_t batch, int32_t n_traj,
                                         int32_t stride, const double* p_action, const int32_t* states,
                                         const int32_t* actions, const int32_t* lengths, double* ll_traj, double* ll,
                                         int32_t* traj_status, void* stream) {
  if (int rc = check_demo_sizes("demo_log_likelihood", n_states, n_actions, batch, n_traj, stride)) return rc;
  if (int rc = need_all("demo_log_likelihood", {{p_action, "p_action"}, {states, "states"}, {actions, "actions"},
                                                {lengths, "lengths"}, {ll_traj, "ll_traj"}, {ll, "ll"},
                                                {traj_status, "traj_status"}}))
    return rc;
  return run_demo_ll<false>(n_states, n_actions, batch, n_traj, stride, 0, p_action, states, actions, lengths, ll_traj,
                            ll, traj_status, (hipStream_t)stream);
}

extern "C" int irlmx_demo_log_likelihood_horizon(int32_t n_states, int32_t n_actions, int32_t batch, int32_t n_traj,
                                                 int32_t stride, int32_t horizon, const double* p_action_t,
                                                 const int32_t* states, const int32_t* actions, const int32_t* lengths,
                                                 double* ll_traj, double* ll, int32_t* traj_status, void* stream) {
  const char* fn = "demo_log_likelihood_horizon";
  if (int rc = check_demo_sizes(fn, n_states, n_actions, batch, n_traj, stride)) return rc;
  if (int rc = check_horizon(fn, horizon)) return rc;
  if (int rc = need_all(fn, {{p_action_t, "p_action_t"}, {states, "states"}, {actions, "actions"}, {lengths, "lengths"},
                             {ll_traj, "ll_traj"}, {ll, "ll"}, {traj_status, "traj_status"}}))
    return rc;
  return run_demo_ll<true>(n_states, n_actions, batch, n_traj, stride, horizon, p_action_t, states, actions, lengths,
                           ll_traj, ll, traj_status, (hipStream_t)stream);
}

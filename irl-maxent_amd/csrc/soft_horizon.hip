// The two finite-horizon value recursions on gfx950: MaxCausalEnt's soft
// Bellman recursion (irlmx_soft_backward_horizon), which makes a time-indexed
// policy pi_t [B][T][S][A], and the value of a reward under such a policy or
// under none (irlmx_value_horizon, include/irlmx_timed.h).  A fixed number of
// steps T, no convergence test.
//
// The soft pass, from V_T(s) = r(s), for t = T-1 .. 0, per state s
// (include/irlmx.h states the same order word for word):
//
//   1. per action a in index order, acc = fma(P[s, target_k(s), a], V_{t+1}(target_k(s)), acc)
//      from 0 over every stored slot in slot order; q_a = r(s) + discount * acc,
//      the product rounded before the sum
//   2. v = q_0, then v = softmax2(v, q_a) for a = 1 .. A-1 (common.h: numpy's exp / log)
//   3. pi_t(s, a) = np_exp(q_a - v)
//   4. V_t(s) = v; a terminal s holds V_t(s) = r(s) (absorbing) and keeps the row of step 3
//
// q_a rests in the output row between steps 1 and 3 (the action loop stays
// rolled: 2 (A - 1) + A inlined exp / log per state leave no registers for A
// values, and a dynamic index into registers would go to scratch), and the table
// is re-read every step.  The pass works in the log domain: finite rewards keep
// everything finite, and there is no extended-range form.
//
// The value pass, from v_T(s) = r(s), for t = T-1 .. 0, per state s
// (include/irlmx_timed.h states the same order word for word):
//
//   1. per action a in index order, acc as in the soft pass's step 1
//   2. with a policy: e = fma(pi_t(s, a), acc, e) from 0 in action order;
//      without one: q_a = r(s) + discount * acc, the product rounded before the
//      sum, and v = max_a q_a by irlmx_value_iteration's NaN rule
//   3. with a policy v_t(s) = r(s) + discount * e, the product rounded before
//      the sum; a terminal s holds v_t(s) = r(s) (absorbing)
//
// No exp / log: its fused kernels stage no NpTables.
//
// Both passes are one skeleton (`Pass`: SoftPass, ValuePass) in two shapes, the
// same statements and so the same bits, routed and sized by horizon.h: fused --
// one workgroup per instance for all T steps, the value ping-pongs in LDS, one
// barrier per step -- and per sweep: one launch per step over all instances,
// the value double-buffered in the caller's workspace; the launch count is
// T + 1, so the host never polls.

#include <hip/hip_runtime.h>

#include "../../include/irlmx_timed.h"
#include "horizon.h"
#include "horizon_rows.h"

namespace irlmx {

struct SoftHzArgs {
  Model m;
  const double* reward;
  const uint8_t* term;  // may be null
  double discount;
  int T;
  double* pi;      // [B][T][S][A]
  double* value0;  // [B][S], may be null
  int32_t* status;
};

struct ValueHzArgs {
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

// per-sweep buffers (the fused kernels keep the value in LDS): hz_carve's man[0..1]
struct ValueWs {
  double* v[2];  // [B][S] ping and pong
  size_t total;
};

// What a pass supplies to the skeleton below: its arguments, whether its rows
// need numpy's exp / log tables (staged in LDS in front of the value buffers),
// the row of one state of step t, and where a step's value is kept: store()
// at every step t = T .. 0 (T: the init phase), store0() at step 0, state
// i = b * S + s.
struct SoftPass {
  using Args = SoftHzArgs;
  static constexpr bool kTables = true;
  template <int KMAX, class Nbr>
  __device__ __attribute__((always_inline)) static double row(const Args& a, int b, int t, int s, double r,
                                                              const double* vin, Nbr&& nbr, const NpTables* tabs) {
    return sh_row<KMAX>(a.m, b, s, r, a.discount, vin, nbr, tabs, a.pi + hz_pi_row(a.m, a.T, b, t, s));
  }
  __device__ static void store(const Args&, int, int, int, double) {}  // only V_0 is an output
  __device__ static void store0(const Args& a, size_t i, double v) {
    if (a.value0) a.value0[i] = v;
  }
};

struct ValuePass {
  using Args = ValueHzArgs;
  static constexpr bool kTables = false;
  template <int KMAX, class Nbr>
  __device__ __attribute__((always_inline)) static double row(const Args& a, int b, int t, int s, double r,
                                                              const double* vin, Nbr&& nbr, const NpTables*) {
    return tp_row<KMAX>(a.m, b, s, r, a.discount, vin, nbr, a.pi ? a.pi + hz_pi_row(a.m, a.T, b, t, s) : nullptr);
  }
  __device__ static void store(const Args& a, int b, int t, int s, double v) {
    if (a.value_t) a.value_t[((size_t)b * (a.T + 1) + t) * a.m.S + s] = v;
  }
  __device__ static void store0(const Args& a, size_t i, double v) { a.value0[i] = v; }
};

// ---------------------------------------------------------------------------
// fused shape: one workgroup per instance for all T steps
// ---------------------------------------------------------------------------

template <class Pass, int SPT, int KMAX>
__global__ void __launch_bounds__(1024) value_hz_fused_kernel(typename Pass::Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char value_hz_smem[];
  const Model& m = a.m;
  const int S = m.S, K = m.K, T = a.T;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  NpTables* tabs = Pass::kTables ? (NpTables*)value_hz_smem : nullptr;
  double* vA = (double*)(value_hz_smem + (Pass::kTables ? sizeof(NpTables) : 0));
  double* vB = vA + S;

  // Up to 10 neighbour indices per thread stay in registers with the reward and
  // the terminal flag (the loop over this thread's states is then unrolled);
  // beyond that the state loop is rolled and everything per state is read at
  // its use: held, the soft pass's <4, 5> spills 16 VGPRs and <2, 8> 40 at 1024 threads.
  constexpr bool kHold = SPT * KMAX <= 10;
  double r[kHold ? SPT : 1];
  bool term[kHold ? SPT : 1];
  int nb[kHold ? SPT : 1][kHold ? KMAX : 1];
  if constexpr (Pass::kTables) np_stage_tables(tabs);
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
  for (int s = tid; s < S; s += nt) {  // V_T = r
    const double rs = a.reward[(size_t)b * S + s];
    vA[s] = rs;
    Pass::store(a, b, T, s, rs);
  }
  __syncthreads();

  int nonfinite = 0;
  for (int it = 0; it < T; ++it) {
    const int t = T - 1 - it;
    const double* vin = (it & 1) ? vB : vA;
    double* vout = (it & 1) ? vA : vB;
    auto state = [&](int s, double rs, bool ts, auto&& nbr) __attribute__((always_inline)) {
      double v = Pass::template row<KMAX>(a, b, t, s, rs, vin, nbr, tabs);
      if (ts) v = rs;  // absorbing: V_t = r, held
      vout[s] = v;
      Pass::store(a, b, t, s, v);
      if (t == 0) {
        Pass::store0(a, (size_t)b * S + s, v);
        nonfinite |= !isfinite(v);
      }
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

// ---------------------------------------------------------------------------
// per-sweep shape: one launch per step over all instances
// ---------------------------------------------------------------------------

template <class Pass>
__global__ void value_hz_init_kernel(typename Pass::Args a, ValueWs ws) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (s >= a.m.S) return;
  const size_t i = (size_t)b * a.m.S + s;
  const double r = a.reward[i];
  ws.v[0][i] = r;
  Pass::store(a, b, a.T, s, r);
  if (s == 0) a.status[b] = IRLMX_OK;
}

template <class Pass>
__global__ void __launch_bounds__(kSweepThreads) value_hz_step_kernel(typename Pass::Args a, ValueWs ws, int t, int odd) {
  const Model& m = a.m;
  const int S = m.S;
  const int b = blockIdx.y;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const size_t i = (size_t)b * S + s;
  const double r = a.reward[i];
  double v = Pass::template row<0>(a, b, t, s, r, ws.v[odd] + (size_t)b * S,
                                   [&](int k) __attribute__((always_inline)) { return row_nbr(m, b, s, k); }, &kNpTabs);
  if (a.term && a.term[i]) v = r;
  ws.v[odd ^ 1][i] = v;
  Pass::store(a, b, t, s, v);
  if (t == 0) {
    Pass::store0(a, i, v);
    if (!isfinite(v)) atomicOr(&a.status[b], IRLMX_NONFINITE);
  }
}

// ---------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------

// fused_pair_ok(IRLMX_OP_SOFT_BACKWARD_HORIZON, ..) is the instantiation list
// (fixed_point.h; the register table is in DESIGN.md section 4).
static void (*soft_hz_fn(int spt, int kmax))(SoftHzArgs) {
  return with_pair<void (*)(SoftHzArgs)>(spt, kmax, [](auto s, auto k) {
    if constexpr (fused_pair_ok(IRLMX_OP_SOFT_BACKWARD_HORIZON, s, k)) return &value_hz_fused_kernel<SoftPass, s, k>;
    else return nullptr;
  });
}

// fused_pair_ok(IRLMX_OP_VALUE_HORIZON, ..): the same eight pairs
static void (*value_hz_fn(int spt, int kmax))(ValueHzArgs) {
  return with_pair<void (*)(ValueHzArgs)>(spt, kmax, [](auto s, auto k) {
    if constexpr (fused_pair_ok(IRLMX_OP_VALUE_HORIZON, s, k)) return &value_hz_fused_kernel<ValuePass, s, k>;
    else return nullptr;
  });
}

// A checked call of either pass: fused, or T + 1 per-sweep launches on the carved workspace.
template <class Pass, class Pick>
static int value_hz_run(const Model& m, int op, void* workspace, hipStream_t st, const typename Pass::Args& a,
                        const char* pass, Pick&& pick) {
  return hz_launch(
      m, op, workspace, st, a, pass, "value_hz_fused_kernel", [&](const FusedShape& fs) { return pick(fs.spt, fs.kmax); },
      [&](const HzWs& w) {
        const ValueWs ws{{w.man[0], w.man[1]}, w.total};
        return hz_launch_sweeps(m, value_hz_init_kernel<Pass>, value_hz_step_kernel<Pass>, a, ws, a.T, true, pass, st);
      });
}

}  // namespace irlmx

using namespace irlmx;

extern "C" int irlmx_soft_backward_horizon(const irlmx_mdp* mdp, const double* reward, const uint8_t* terminal,
                                           double discount, int32_t horizon, double* p_action_t, double* value0,
                                           int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "soft_backward_horizon";
  if (int rc = validate(mdp)) return rc;
  const Model m = make_model(mdp);
  if (int rc = horizon_check_model(m, fn)) return rc;
  if (int rc = need_all(fn, {{reward, "reward"}, {p_action_t, "p_action_t"}, {status, "status"}})) return rc;
  if (!(discount >= 0.0 && discount <= 1.0)) {  // NaN too
    set_error("%s: discount %g outside [0, 1]", fn, discount);
    return IRLMX_EINVAL;
  }
  if (int rc = hz_check_call(m, fn, IRLMX_OP_SOFT_BACKWARD_HORIZON, horizon, workspace_bytes, workspace)) return rc;
  const SoftHzArgs a{m, reward, terminal, discount, horizon, p_action_t, value0, status};
  return value_hz_run<SoftPass>(m, IRLMX_OP_SOFT_BACKWARD_HORIZON, workspace, (hipStream_t)stream, a,
                                "soft horizon backward", soft_hz_fn);
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
  const ValueHzArgs a{m, reward, terminal, p_action_t, discount, horizon, value0, value_t, status};
  return value_hz_run<ValuePass>(m, IRLMX_OP_VALUE_HORIZON, workspace, (hipStream_t)stream, a, "horizon value",
                                 value_hz_fn);
}

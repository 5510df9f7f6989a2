// Finite-horizon MaxCausalEnt (irlmx_soft_backward_horizon) on gfx950: the soft
// Bellman recursion for a fixed number of steps T, with no terminal state, no
// discount below 1 and no convergence test needed.
//
// From V_T(s) = r(s), for t = T-1 .. 0, per state s (include/irlmx.h states the
// same order word for word):
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
// is re-read every step.  Two shapes, the same statements and so the same bits:
// fused -- one workgroup per instance for all T steps, V ping-pongs in LDS, one
// barrier per step -- and per sweep: one launch per step over all instances, V
// double-buffered in the caller's workspace; the launch count is T + 1, so the
// host never polls.  The pass works in the log domain: finite rewards keep
// everything finite, and there is no extended-range form.

#include <hip/hip_runtime.h>

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

// per-sweep buffers (the fused kernel keeps V in LDS): hz_carve's man[0..1]
struct ShWs {
  double* v[2];  // [B][S] ping and pong
  size_t total;
};

// ---------------------------------------------------------------------------
// fused shape: one workgroup per instance for all T steps
// ---------------------------------------------------------------------------

template <int SPT, int KMAX>
__global__ void __launch_bounds__(1024) soft_hz_fused_kernel(SoftHzArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char soft_hz_smem[];
  const Model& m = a.m;
  const int S = m.S, K = m.K, T = a.T;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  NpTables* tabs = (NpTables*)soft_hz_smem;
  double* vA = (double*)(soft_hz_smem + sizeof(NpTables));
  double* vB = vA + S;

  // Up to 10 neighbour indices per thread stay in registers with the reward and
  // the terminal flag (the loop over this thread's states is then unrolled);
  // beyond that the state loop is rolled and everything per state is read at
  // its use: held, <4, 5> spills 16 VGPRs and <2, 8> 40 at 1024 threads.
  constexpr bool kHold = SPT * KMAX <= 10;
  double r[kHold ? SPT : 1];
  bool term[kHold ? SPT : 1];
  int nb[kHold ? SPT : 1][kHold ? KMAX : 1];
  np_stage_tables(tabs);
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
  for (int s = tid; s < S; s += nt) vA[s] = a.reward[(size_t)b * S + s];  // V_T = r
  __syncthreads();

  int nonfinite = 0;
  for (int it = 0; it < T; ++it) {
    const int t = T - 1 - it;
    const double* vin = (it & 1) ? vB : vA;
    double* vout = (it & 1) ? vA : vB;
    auto state = [&](int s, double rs, bool ts, auto&& nbr) __attribute__((always_inline)) {
      double v = sh_row<KMAX>(m, b, s, rs, a.discount, vin, nbr, tabs, a.pi + hz_pi_row(m, T, b, t, s));
      if (ts) v = rs;  // absorbing: V_t = r, held
      vout[s] = v;
      if (t == 0) {
        if (a.value0) a.value0[(size_t)b * S + s] = v;
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

__global__ void soft_hz_init_kernel(SoftHzArgs a, ShWs ws) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (s >= a.m.S) return;
  const size_t i = (size_t)b * a.m.S + s;
  ws.v[0][i] = a.reward[i];
  if (s == 0) a.status[b] = IRLMX_OK;
}

__global__ void __launch_bounds__(kSweepThreads) soft_hz_step_kernel(SoftHzArgs a, ShWs ws, int t, int odd) {
  const Model& m = a.m;
  const int S = m.S;
  const int b = blockIdx.y;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const size_t i = (size_t)b * S + s;
  const double r = a.reward[i];
  double v = sh_row<0>(m, b, s, r, a.discount, ws.v[odd] + (size_t)b * S,
                       [&](int k) __attribute__((always_inline)) { return row_nbr(m, b, s, k); }, &kNpTabs,
                       a.pi + hz_pi_row(m, a.T, b, t, s));
  if (a.term && a.term[i]) v = r;
  ws.v[odd ^ 1][i] = v;
  if (t == 0) {
    if (a.value0) a.value0[i] = v;
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
    if constexpr (fused_pair_ok(IRLMX_OP_SOFT_BACKWARD_HORIZON, s, k)) return &soft_hz_fused_kernel<s, k>;
    else return nullptr;
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
  hipStream_t st = (hipStream_t)stream;
  const SoftHzArgs a{m, reward, terminal, discount, horizon, p_action_t, value0, status};
  return hz_launch(
      m, IRLMX_OP_SOFT_BACKWARD_HORIZON, workspace, st, a, "soft horizon backward", "soft_hz_fused_kernel",
      [&](const FusedShape& fs) { return soft_hz_fn(fs.spt, fs.kmax); },
      [&](const HzWs& w) {
        const ShWs ws{{w.man[0], w.man[1]}, w.total};
        return hz_launch_sweeps(m, soft_hz_init_kernel, soft_hz_step_kernel, a, ws, horizon, true,
                                "soft horizon backward", st);
      });
}

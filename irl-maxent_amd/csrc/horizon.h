// Host side of the finite-horizon passes (horizon.hip: IRLMX_OP_BACKWARD_HORIZON,
// IRLMX_OP_FORWARD_HORIZON; soft_horizon.hip: IRLMX_OP_SOFT_BACKWARD_HORIZON and
// IRLMX_OP_VALUE_HORIZON; expected_svf_horizon.hip routes by hz_fused_shape and
// has no op code; rollout.hip takes hz_pi_row and the horizon's range for its
// calls on time-indexed policies).  Their per-state device functions are
// horizon_rows.h's.
// horizon.hip defines what is not a template; fixed_point.h declares what the
// model queries ask (horizon_op, horizon_check_model, horizon_workspace_bytes, horizon_plan).
#pragma once

#include "fixed_point.h"

namespace irlmx {

constexpr int kHzMaxHorizon = 1 << 20;  // (backward: |e| grows by < 1100 per step, no int32 wrap)

__device__ inline size_t hz_pi_row(const Model& m, int T, int b, int t, int s) {
  return (((size_t)b * T + t) * m.S + s) * m.A;
}

// per-sweep buffers (the fused kernels keep all of this in LDS)
struct HzWs {
  int32_t* bad;     // [B] backward: some exp(r) is non-finite
  double* man[2];   // [B][S] backward mantissas / forward d_t / soft V_t / value v_t, ping and pong
  int32_t* exp[2];  // [B][S] backward exponents
  size_t total;
};

// LDS of `op`'s fused kernel: ping and pong of (mantissa, exponent), of d_t or v_t, or of V_t behind the NpTables copy.
size_t hz_fused_lds(const Model& m, int op);

// The fused shape of a horizon pass: the thread layout of the ordinary fused
// passes at every width (these passes have no cluster form), when its pair is
// instantiated (fused_pair_ok; the forward has no slot classes), its LDS fits
// (the soft pass's always does) and (several states per thread) the batch
// holds horizon_fused_min_batch() instances; else one launch per step.
bool hz_fused_shape(const Model& m, int op, FusedShape* out);

// The workspace of `op` carved from `base` (nullptr: sizes only): nothing for
// the fused shape, else man[0..1], and for the backward bad and exp[0..1].
HzWs hz_carve(const Model& m, int op, void* base);

// The horizon's range, then check_ws on hz_carve's total.
int hz_check_call(const Model& m, const char* fn, int op, int32_t horizon, size_t bytes, void* ws);

// The per-sweep shape: `init`, then `step` T times with (t, parity), t from
// T - 1 down (`descending`) or from 0 up; the launch count is fixed, so the
// host never polls.  `pass` names the pass in a launch error.
template <class Args, class W>
int hz_launch_sweeps(const Model& m, void (*init)(Args, W), void (*step)(Args, W, int, int), const Args& a,
                     const W& ws, int T, bool descending, const char* pass, hipStream_t st) {
  count_event(IRLMX_CTR_SWEEP_CALLS);
  const dim3 g = sweep_grid(m);
  hipLaunchKernelGGL(init, g, dim3(kSweepThreads), 0, st, a, ws);
  for (int it = 0; it < T; ++it)
    hipLaunchKernelGGL(step, g, dim3(kSweepThreads), 0, st, a, ws, descending ? T - 1 - it : it, it & 1);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, pass);
}

// A checked call of `op`: the fused kernel `pick(fs)` returns for the planned shape
// (`kernel` names it in a launch error), or `sweeps(ws)` on the carved workspace.
template <class Args, class Pick, class Sweeps>
int hz_launch(const Model& m, int op, void* workspace, hipStream_t st, const Args& a, const char* pass,
              const char* kernel, Pick&& pick, Sweeps&& sweeps) {
  FusedShape fs;
  if (!hz_fused_shape(m, op, &fs)) return sweeps(hz_carve(m, op, workspace));
  void (*kfn)(Args) = pick(fs);
  if (!kfn) { set_error("no %s fused kernel for spt=%d kmax=%d", pass, fs.spt, fs.kmax); return IRLMX_EINVAL; }
  return launch_fused(kfn, kernel, m.B, fs.threads, hz_fused_lds(m, op), st, a);
}

}  // namespace irlmx

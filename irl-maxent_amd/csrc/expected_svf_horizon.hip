// Finite-horizon expected state visitation in one call
// (irlmx_expected_svf_horizon, include/irlmx_expected_svf.h) on gfx950: the
// backward recursion of irlmx_backward_maxent_horizon (MAXENT) or of
// irlmx_soft_backward_horizon (CAUSAL) and the forward recursion of
// irlmx_forward_svf_horizon, without the policy tensor pi_t [B][T][S][A]
// between them.
//
// X_t is the backward's state at step t: V_t (CAUSAL), or Z_t as a mantissa and
// an int32 exponent (MAXENT).  pi_t depends only on the reward and X_{t+1}, so
// with C = `segment`:
//
//   pass 1   X_T from the reward; for t = T-1 .. C the recursion on the values
//            alone, X_t kept where t is a multiple of C (and X_T)
//   pass 2   for each segment [lo, hi) = [jC, min((j+1)C, T)), j ascending:
//            X_{hi-1} .. X_{lo+1} recomputed from X_hi into the segment buffer,
//            then for t = lo .. hi-1 the policy rows of step t from X_{t+1}
//            into one [S][A] buffer, one forward step under them, D += d_{t+1}
//
// which holds ceil(T/C) + C slices of [B][S] instead of T * A.  Every per-state
// function is the one horizon.hip and soft_horizon.hip run (horizon_rows.h:
// hz_row_loop, sh_row); a value-only step instantiates the same function with
// ROW = false, which compiles out the division (MAXENT) or the exp of the row
// (CAUSAL), on which no value depends.  So svf, objective0 and status carry the
// bits of the two-call path for every C.
//
// Two shapes, the same statements in both: per step -- one launch over all
// instances per value step, policy step and forward step, everything in the
// workspace; the launch count is fixed by T and C, so the host never polls --
// and fused -- one workgroup per instance, one state per thread, for both
// passes: d_t ping-pong and the step's policy rows in LDS, the slices in the
// workspace (written and read by the same workgroup, one barrier between
// dependent phases).

#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/irlmx_expected_svf.h"
#include "extended.h"
#include "horizon.h"
#include "horizon_rows.h"

namespace irlmx {

struct EshArgs {
  Model m;
  const double* reward;
  const uint8_t* term;  // may be null
  const double* p0;
  double discount;
  int T, C, nseg;  // C resolved (1 .. T); nseg = ceil(T / C)
  double* svf;     // [B][S]
  double* obj0;    // [B][S], may be null
  int32_t* status;
};

// Slices of X, each [B][S]: nseg checkpoints (slice j holds X at the end of
// segment j), C - 1 of the segment buffer, 2 of pass 1's ping-pong.
struct EshWs {
  int32_t* bad;  // [B] MAXENT: some exp(r) is non-finite
  double* xm;    // [slices][B][S] V_t, or the mantissas of Z_t
  int32_t* xe;   // [slices][B][S] MAXENT: the exponents
  double* pol;   // [B][S][A] per step: the step's policy rows
  double* d[2];  // [B][S] per step: d_t ping and pong
  int slices;
  size_t total;
};

// slice of X_t during pass 1 (C <= t <= T)
__host__ __device__ inline int esh_slice_pass1(int T, int C, int nseg, int t) {
  if (t == T) return nseg - 1;
  if (t % C == 0) return t / C - 1;
  return nseg + C - 1 + (t & 1);
}

// slice of X_t during segment j = [lo, hi) (lo < t <= hi)
__host__ __device__ inline int esh_slice_seg(int nseg, int j, int lo, int hi, int t) {
  return t == hi ? j : nseg + (t - lo - 1);
}

// One state of a value-only step: X_t(s) into slice `so` from X_{t+1} in slice
// `si`, by the ROW = false forms of the functions esh_policy_state calls.
template <int MODEL>
__device__ __attribute__((always_inline)) inline void esh_value_state(const EshArgs& a, const EshWs& ws, int b, int s,
                                                                      int si, int so, const NpTables* tabs) {
  const Model& m = a.m;
  const size_t B = m.B, S = m.S;
  const size_t i = (size_t)b * S + s;
  const size_t in = ((size_t)si * B + b) * S, out = ((size_t)so * B + b) * S + s;
  const bool term = a.term && a.term[i];
  if constexpr (MODEL == IRLMX_HORIZON_MODEL_MAXENT) {
    const double er = exp(a.reward[i]);
    double zm;
    int ze;
    if (term) {
      ext_split(er, 0, &zm, &ze);  // absorbing: Z_t = exp(r), held
    } else {
      int E;
      const double zsum = hz_row_loop<false>(m, b, s, er, ws.xm + in, ws.xe + in, nullptr, &E);
      ext_split(zsum, E, &zm, &ze);
    }
    ws.xm[out] = zm;
    ws.xe[out] = ze;
  } else {
    const double r = a.reward[i];
    ws.xm[out] = term ? r
                      : sh_row<0, false>(m, b, s, r, a.discount, ws.xm + in,
                                         [&](int k) __attribute__((always_inline)) { return row_nbr(m, b, s, k); },
                                         tabs, nullptr);
  }
}

// One state of step t's policy rows into `row` from X_{t+1} in slice `si`;
// step 0 also gives objective0.  Returns whether V_0(s) is non-finite (CAUSAL).
template <int MODEL>
__device__ __attribute__((always_inline)) inline bool esh_policy_state(const EshArgs& a, const EshWs& ws, int b, int s,
                                                                       int si, int t, bool bad, const NpTables* tabs,
                                                                       double* row) {
  const Model& m = a.m;
  const size_t B = m.B, S = m.S;
  const size_t i = (size_t)b * S + s;
  const size_t in = ((size_t)si * B + b) * S;
  if constexpr (MODEL == IRLMX_HORIZON_MODEL_MAXENT) {
    if (bad) {  // bwd_nonfinite_rule: NaN rows at every step
      for (int act = 0; act < m.A; ++act) row[act] = kNaN;
      if (t == 0 && a.obj0) a.obj0[i] = kNaN;
      return false;
    }
    const double er = exp(a.reward[i]);
    int E;
    const double zsum = hz_row_loop(m, b, s, er, ws.xm + in, ws.xe + in, row, &E);
    if (t == 0 && a.obj0) {
      double zm;
      int ze;
      if (a.term && a.term[i]) ext_split(er, 0, &zm, &ze);
      else ext_split(zsum, E, &zm, &ze);
      a.obj0[i] = hz_log_z(zm, ze);
    }
    return false;
  } else {
    const double r = a.reward[i];
    double v = sh_row<0>(m, b, s, r, a.discount, ws.xm + in,
                         [&](int k) __attribute__((always_inline)) { return row_nbr(m, b, s, k); }, tabs, row);
    if (t != 0) return false;
    if (a.term && a.term[i]) v = r;
    if (a.obj0) a.obj0[i] = v;
    return !isfinite(v);
  }
}

// ---------------------------------------------------------------------------
// per-step shape: one launch per value step, policy step and forward step
// ---------------------------------------------------------------------------

template <int MODEL>
__global__ void esh_init_kernel(EshArgs a, EshWs ws) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  const size_t B = a.m.B, S = a.m.S;
  if (s >= a.m.S) return;
  const size_t i = (size_t)b * S + s;
  const size_t xT = ((size_t)(a.nseg - 1) * B + b) * S + s;
  if constexpr (MODEL == IRLMX_HORIZON_MODEL_MAXENT) {
    const double er = exp(a.reward[i]);
    if (!isfinite(er)) atomicOr(&ws.bad[b], 1);
    ext_split(er, 0, &ws.xm[xT], &ws.xe[xT]);  // Z_T = exp(r)
  } else {
    ws.xm[xT] = a.reward[i];  // V_T = r
  }
  const double p = a.p0[i];
  ws.d[0][i] = p;
  a.svf[i] = p;
  if (s == 0) a.status[b] = IRLMX_OK;
}

template <int MODEL>
__global__ void __launch_bounds__(kSweepThreads) esh_value_kernel(EshArgs a, EshWs ws, int si, int so) {
  const int b = blockIdx.y;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.m.S) return;
  if (MODEL == IRLMX_HORIZON_MODEL_MAXENT && ws.bad[b]) return;  // no value is read: the rows are NaN
  esh_value_state<MODEL>(a, ws, b, s, si, so, &kNpTabs);
}

template <int MODEL>
__global__ void __launch_bounds__(kSweepThreads) esh_policy_kernel(EshArgs a, EshWs ws, int si, int t) {
  const int b = blockIdx.y;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= a.m.S) return;
  const bool bad = MODEL == IRLMX_HORIZON_MODEL_MAXENT && ws.bad[b];
  double* row = ws.pol + ((size_t)b * a.m.S + s) * a.m.A;
  if (esh_policy_state<MODEL>(a, ws, b, s, si, t, bad, &kNpTabs, row)) atomicOr(&a.status[b], IRLMX_NONFINITE);
}

__global__ void __launch_bounds__(kSweepThreads) esh_fwd_kernel(EshArgs a, EshWs ws, int t, int odd) {
  const Model& m = a.m;
  const int S = m.S;
  const int b = blockIdx.y;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const size_t i = (size_t)b * S + s;
  const uint8_t* tb = a.term ? a.term + (size_t)b * S : nullptr;
  const double nd = hz_fwd_state(m, b, s, ws.pol + (size_t)b * S * m.A, tb, ws.d[odd] + (size_t)b * S);
  ws.d[odd ^ 1][i] = nd;
  const double D = __dadd_rn(a.svf[i], nd);
  a.svf[i] = D;
  if (t == a.T - 1 && !isfinite(D)) atomicOr(&a.status[b], IRLMX_NONFINITE);
}

// ---------------------------------------------------------------------------
// fused shape: one workgroup per instance, one state per thread, both passes
// ---------------------------------------------------------------------------

template <int MODEL>
__global__ void __launch_bounds__(1024) esh_fused_kernel(EshArgs a, EshWs ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char esh_smem[];
  constexpr bool kCausal = MODEL == IRLMX_HORIZON_MODEL_CAUSAL;
  const Model& m = a.m;
  const int S = m.S, A = m.A, T = a.T, C = a.C, nseg = a.nseg;
  const int b = blockIdx.x, s = threadIdx.x;
  const bool live = s < S;
  const NpTables* tabs = &kNpTabs;
  double* dA = (double*)esh_smem;
  if constexpr (kCausal) {
    np_stage_tables((NpTables*)esh_smem);
    tabs = (const NpTables*)esh_smem;
    dA = (double*)(esh_smem + sizeof(NpTables));
  }
  double* dB = dA + S;
  double* pol = dB + S;  // [S][A]
  const uint8_t* tb = a.term ? a.term + (size_t)b * S : nullptr;
  const size_t i = (size_t)b * S + (live ? s : 0);

  double D = 0.0;
  int nonfinite = 0;
  if (live) {
    const size_t xT = ((size_t)(nseg - 1) * m.B + b) * S + s;
    if constexpr (kCausal) {
      ws.xm[xT] = a.reward[i];  // V_T = r
    } else {
      const double er = exp(a.reward[i]);
      nonfinite = !isfinite(er);
      ext_split(er, 0, &ws.xm[xT], &ws.xe[xT]);  // Z_T = exp(r)
    }
    D = a.p0[i];
    dA[s] = D;
  }
  const bool bad = __syncthreads_or(nonfinite) != 0;  // uniform over the workgroup; orders X_T, d_0 and the tables

  // pass 1: values only, checkpoints kept
  if (!bad)
    for (int t = T - 1; t >= C; --t) {
      if (live) esh_value_state<MODEL>(a, ws, b, s, esh_slice_pass1(T, C, nseg, t + 1), esh_slice_pass1(T, C, nseg, t), tabs);
      __syncthreads();
    }

  // pass 2: per segment the values again, then policy rows and forward steps
  int v0bad = 0;
  for (int j = 0; j < nseg; ++j) {
    const int lo = j * C, hi = min(lo + C, T);
    if (!bad)
      for (int t = hi - 1; t > lo; --t) {
        if (live) esh_value_state<MODEL>(a, ws, b, s, esh_slice_seg(nseg, j, lo, hi, t + 1), esh_slice_seg(nseg, j, lo, hi, t), tabs);
        __syncthreads();
      }
    for (int t = lo; t < hi; ++t) {
      const double* din = (t & 1) ? dB : dA;
      double* dout = (t & 1) ? dA : dB;
      if (live)
        v0bad |= esh_policy_state<MODEL>(a, ws, b, s, esh_slice_seg(nseg, j, lo, hi, t + 1), t, bad, tabs,
                                         pol + (size_t)s * A);
      __syncthreads();
      if (live) {
        const double nd = hz_fwd_state(m, b, s, pol, tb, din);
        dout[s] = nd;
        D = __dadd_rn(D, nd);
      }
      __syncthreads();
    }
  }
  nonfinite = v0bad;
  if (live) {
    a.svf[i] = D;
    nonfinite |= !isfinite(D);
  }
  nonfinite = __syncthreads_or(nonfinite);
  if (s == 0) a.status[b] = nonfinite ? IRLMX_NONFINITE : IRLMX_OK;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

static size_t esh_lds(const Model& m, int model) {
  return (model == IRLMX_HORIZON_MODEL_CAUSAL ? sizeof(NpTables) : 0) + sizeof(double) * (size_t)m.S * (m.A + 2);
}

// The forward's fused shape at one state per thread, when the LDS fits; else per step.
static bool esh_fused_shape(const Model& m, int model, FusedShape* fs) {
  if (!hz_fused_shape(m, IRLMX_OP_FORWARD_HORIZON, fs) || fs->spt != 1) return false;
  return esh_lds(m, model) <= kExtLdsMax;
}

// C as resolved: 0 is ceil(sqrt(T)), a value above T is T.
static int esh_segment(int T, int segment) {
  if (segment > T) return T;
  if (segment > 0) return segment;
  int c = (int)std::sqrt((double)T);
  while ((long long)c * c < T) ++c;
  while (c > 1 && (long long)(c - 1) * (c - 1) >= T) --c;
  return c;
}

static EshWs esh_carve(const Model& m, int model, int T, int C, void* base) {
  EshWs w;
  Carver c{(char*)base};
  const size_t B = m.B, S = m.S;
  const int nseg = (T + C - 1) / C;
  FusedShape fs;
  const bool sweep = !esh_fused_shape(m, model, &fs);
  const bool maxent = model == IRLMX_HORIZON_MODEL_MAXENT;
  w.slices = nseg + (C - 1) + (nseg > 1 ? 2 : 0);
  w.bad = c.take<int32_t>(sweep && maxent ? B * sizeof(int32_t) : 0);
  w.xm = c.take<double>((size_t)w.slices * B * S * sizeof(double));
  w.xe = c.take<int32_t>(maxent ? (size_t)w.slices * B * S * sizeof(int32_t) : 0);
  w.pol = c.take<double>(sweep ? B * S * m.A * sizeof(double) : 0);
  for (int i = 0; i < 2; ++i) w.d[i] = c.take<double>(sweep ? B * S * sizeof(double) : 0);
  w.total = c.total();
  return w;
}

// The checks of the model, `model`, `horizon` and `segment` the three entry points share.
static int esh_check(const irlmx_mdp* mdp, int32_t model, int32_t horizon, int32_t segment, const char* fn) {
  if (int rc = validate(mdp)) return rc;
  const Model m = make_model(mdp);
  if (int rc = horizon_check_model(m, fn)) return rc;
  if (int rc = need_col_form(m)) return rc;
  if (model != IRLMX_HORIZON_MODEL_MAXENT && model != IRLMX_HORIZON_MODEL_CAUSAL) {
    set_error("%s: model %d is neither IRLMX_HORIZON_MODEL_MAXENT nor IRLMX_HORIZON_MODEL_CAUSAL", fn, model);
    return IRLMX_EINVAL;
  }
  if (horizon < 1 || horizon > kHzMaxHorizon) {
    set_error("%s: horizon %d outside [1, %d]", fn, horizon, kHzMaxHorizon);
    return IRLMX_EINVAL;
  }
  if (segment < 0) {
    set_error("%s: segment %d is negative", fn, segment);
    return IRLMX_EINVAL;
  }
  return 0;
}

template <int MODEL>
static int esh_run(const Model& m, const EshArgs& a, const EshWs& ws, hipStream_t st) {
  FusedShape fs;
  if (esh_fused_shape(m, MODEL, &fs)) {
    void* args[] = {(void*)&a, (void*)&ws};  // (launch_fused takes kernels of one argument)
    const void* kfn = (const void*)&esh_fused_kernel<MODEL>;
    const size_t lds = esh_lds(m, MODEL);
    if (hipError_t e = hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
      return hip_fail(e, "hipFuncSetAttribute");
    (void)hipLaunchKernel(kfn, dim3(m.B), dim3(fs.threads), args, lds, st);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, "esh_fused_kernel");
  }
  count_event(IRLMX_CTR_SWEEP_CALLS);
  const int T = a.T, C = a.C, nseg = a.nseg;
  if (MODEL == IRLMX_HORIZON_MODEL_MAXENT) {
    const hipError_t e = hipMemsetAsync(ws.bad, 0, (size_t)m.B * sizeof(int32_t), st);
    if (e != hipSuccess) return hip_fail(e, "workspace memset");
  }
  const dim3 g = sweep_grid(m), th(kSweepThreads);
  hipLaunchKernelGGL(esh_init_kernel<MODEL>, g, th, 0, st, a, ws);
  for (int t = T - 1; t >= C; --t)
    hipLaunchKernelGGL(esh_value_kernel<MODEL>, g, th, 0, st, a, ws, esh_slice_pass1(T, C, nseg, t + 1),
                       esh_slice_pass1(T, C, nseg, t));
  for (int j = 0; j < nseg; ++j) {
    const int lo = j * C, hi = std::min(lo + C, T);
    for (int t = hi - 1; t > lo; --t)
      hipLaunchKernelGGL(esh_value_kernel<MODEL>, g, th, 0, st, a, ws, esh_slice_seg(nseg, j, lo, hi, t + 1),
                         esh_slice_seg(nseg, j, lo, hi, t));
    for (int t = lo; t < hi; ++t) {
      hipLaunchKernelGGL(esh_policy_kernel<MODEL>, g, th, 0, st, a, ws, esh_slice_seg(nseg, j, lo, hi, t + 1), t);
      hipLaunchKernelGGL(esh_fwd_kernel, g, th, 0, st, a, ws, t, t & 1);
    }
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, "expected svf horizon");
}

}  // namespace irlmx

using namespace irlmx;

static const char* const kEshFn = "expected_svf_horizon";

extern "C" size_t irlmx_expected_svf_horizon_workspace_bytes(const irlmx_mdp* mdp, int32_t model, int32_t horizon,
                                                             int32_t segment) {
  if (esh_check(mdp, model, horizon, segment, kEshFn)) return 0;
  return esh_carve(make_model(mdp), model, horizon, esh_segment(horizon, segment), nullptr).total;
}

extern "C" int irlmx_expected_svf_horizon_plan(const irlmx_mdp* mdp, int32_t model, int32_t horizon, int32_t segment,
                                               int64_t* plan) {
  if (int rc = esh_check(mdp, model, horizon, segment, kEshFn)) return rc;
  if (int rc = need_all(kEshFn, {{plan, "plan"}})) return rc;
  const Model m = make_model(mdp);
  const int C = esh_segment(horizon, segment);
  const EshWs ws = esh_carve(m, model, horizon, C, nullptr);
  FusedShape fs;
  const bool fused = esh_fused_shape(m, model, &fs);
  plan[0] = fused ? IRLMX_SHAPE_FUSED : IRLMX_SHAPE_SWEEP;
  plan[1] = C;
  plan[2] = ws.slices;
  plan[3] = fused ? 1 : 0;
  plan[4] = fused ? (int64_t)esh_lds(m, model) : 0;
  plan[5] = (int64_t)ws.total;
  return 0;
}

extern "C" int irlmx_expected_svf_horizon(const irlmx_mdp* mdp, int32_t model, const double* reward,
                                          const uint8_t* terminal, const double* p_initial, double discount,
                                          int32_t horizon, int32_t segment, double* svf, double* objective0,
                                          int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = kEshFn;
  if (int rc = esh_check(mdp, model, horizon, segment, fn)) return rc;
  const Model m = make_model(mdp);
  if (int rc = need_all(fn, {{reward, "reward"}, {p_initial, "p_initial"}, {svf, "svf"}, {status, "status"}})) return rc;
  if (model == IRLMX_HORIZON_MODEL_MAXENT ? discount != 1.0 : !(discount >= 0.0 && discount <= 1.0)) {  // NaN too
    set_error("%s: discount %g outside %s", fn, discount, model == IRLMX_HORIZON_MODEL_MAXENT ? "{1} (MAXENT)" : "[0, 1]");
    return IRLMX_EINVAL;
  }
  const int C = esh_segment(horizon, segment);
  const EshWs ws = esh_carve(m, model, horizon, C, workspace);
  if (workspace_bytes < ws.total || !workspace) {  // (the total is never 0: the slices)
    set_error("%s: workspace too small: need %zu bytes, got %zu", fn, ws.total, workspace_bytes);
    return IRLMX_EWORKSPACE;
  }
  const EshArgs a{m, reward, terminal, p_initial, discount, horizon, C, (horizon + C - 1) / C, svf, objective0, status};
  hipStream_t st = (hipStream_t)stream;
  return model == IRLMX_HORIZON_MODEL_MAXENT ? esh_run<IRLMX_HORIZON_MODEL_MAXENT>(m, a, ws, st)
                                             : esh_run<IRLMX_HORIZON_MODEL_CAUSAL>(m, a, ws, st);
}

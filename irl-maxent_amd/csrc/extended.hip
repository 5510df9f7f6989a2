// Extended-range MaxEnt backward pass (irlmx_backward_maxent_extended) on gfx950.
//
// The rescaled backward (fixed_point.hip, cluster.hip) keeps ONE power-of-two
// scale per instance, so the partition vector zs must fit float64's exponent
// range under a common scale.  A reward contrast of 4 along a grid 256 wide
// already spreads zs over more than 2^2098: the far states flush to 0, their
// policy rows are 0 / 0, and the rows beside the underflow front are finite
// and wrong ("Extended range").
//
// Here every partition value carries its own exponent:
//
//   z(s) = m(s) * 2^e(s),  m in [0.5, 1) or exactly 0 (frexp's form), e an int32,
//                          kExtZero for an exact zero
//
// and one collapsed sweep over the weights of bwd_weights_kernel is
//
//   E        = max e(nb_k) over the slots k with w_k != 0
//   acc      = fma(w_k, ldexp(m(nb_k), e(nb_k) - E), acc)   in slot order
//   (m', d)  = frexp(acc),  e' = E + d                      (acc == 0: zero)
//
// Slot order and the explicit fma are those of bwd_fused_kernel /
// bwd_sweep_kernel, and scaling every operand of an fma chain by one power of
// two commutes with rounding while nothing is subnormal: wherever the rescaled
// pass neither underflows nor overflows, this pass returns the same bits.
// There is no rescaling, no per-sweep maximum and no convergence test; the
// sweep count is the reference's 2*S (maxent.py:154), the last one per action.
//
// Three shapes: fused (one workgroup per instance, mantissas and exponents
// ping-pong in LDS, 24 B per state, one barrier per sweep), the persistent grid
// shape (extended_grid.hip: from 8,192 states on, one launch for all sweeps,
// the pairs exchanged as tagged granules) and per sweep (one launch per sweep
// over all instances, buffers in the caller's workspace; the launch count is
// fixed, so the host never polls).

#include <hip/hip_runtime.h>

#include <algorithm>

#include "cluster.h"
#include "extended.h"
#include "grid.h"

namespace irlmx {

// The last sweep, per action (maxent.py:155-159): every action of a state is
// aligned to the same E, za = er * acc rounded, the sequential action sum, and
// za / zsum, in which the common 2^E cancels.
__device__ inline void ext_policy_row(const ExtArgs& a, int b, int s, const double* zm, const int* ze) {
  const Model& m = a.m;
  const int K = m.K, A = m.A;
  double* out = a.pi + ((size_t)b * m.S + s) * A;
  int E = kExtZero;
  for (int k = 0; k < K; ++k) {
    bool any = false;
    for (int act = 0; act < A; ++act) any |= row_val(m, b, act, k, s) != 0.0;
    if (any) E = max(E, ze[row_nbr(m, b, s, k)]);
  }
  const double er = exp(a.reward[(size_t)b * m.S + s]);
  double za[kMaxActions];
  double zsum = 0.0;
  for (int act = 0; act < A; ++act) {
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
      const int n = row_nbr(m, b, s, k);
      acc = fma(row_val(m, b, act, k, s), ext_aligned(zm[n], ze[n], E), acc);
    }
    za[act] = __dmul_rn(er, acc);  // rounded product, then the sum (maxent.py:155-156)
    zsum = __dadd_rn(zsum, za[act]);
  }
  for (int act = 0; act < A; ++act) out[act] = za[act] / zsum;
}

__device__ inline void ext_nan_row(const ExtArgs& a, int b, int s) {
  double* out = a.pi + ((size_t)b * a.m.S + s) * a.m.A;
  for (int act = 0; act < a.m.A; ++act) out[act] = kNaN;
}

// ---------------------------------------------------------------------------
// fused shape: one workgroup per instance for the whole loop
// ---------------------------------------------------------------------------

template <int SPT, int KMAX>
__global__ void __launch_bounds__(1024) ext_fused_kernel(ExtArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ext_smem[];
  const Model& m = a.m;
  const int S = m.S, K = m.K;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  double* manA = (double*)ext_smem;
  double* manB = manA + S;
  int* expA = (int*)(manB + S);
  int* expB = expA + S;

  if (a.bad[b]) {  // bwd_nonfinite_rule: non-finite weights, NaN everywhere (uniform over the workgroup)
    for (int s = tid; s < S; s += nt) ext_nan_row(a, b, s);
    if (tid == 0) a.status[b] = IRLMX_OK;
    return;
  }

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
  for (int s = tid; s < S; s += nt) ext_init_state(a.term[(size_t)b * S + s] != 0, &manA[s], &expA[s]);
  __syncthreads();

  // 2*S sweeps in all (maxent.py:154): the first 2*S - 1 on the action-summed
  // table, the last one per action because it also produces za.
  const long long collapsed = 2LL * S - 1;
  for (long long it = 0; it < collapsed; ++it) {
    const double* min_ = (it & 1) ? manB : manA;
    const int* ein = (it & 1) ? expB : expA;
    double* mout = (it & 1) ? manA : manB;
    int* eout = (it & 1) ? expA : expB;
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int s = tid + j * nt;
      if (s < S) {
        int E = kExtZero;
        double acc = 0.0;
        if constexpr (KMAX <= 8) {  // neighbours read once, held in registers
          double zm[KMAX];
          int ze[KMAX];
#pragma unroll
          for (int k = 0; k < KMAX; ++k)
            if (k < K) {
              zm[k] = min_[nb[j][k]];
              ze[k] = ein[nb[j][k]];
              if (w[j][k] != 0.0) E = max(E, ze[k]);
            }
#pragma unroll
          for (int k = 0; k < KMAX; ++k)
            if (k < K) acc = fma(w[j][k], ext_aligned(zm[k], ze[k], E), acc);
        } else {  // many slots: the exponents are read twice instead (registers)
#pragma unroll
          for (int k = 0; k < KMAX; ++k)
            if (k < K && w[j][k] != 0.0) E = max(E, ein[nb[j][k]]);
#pragma unroll
          for (int k = 0; k < KMAX; ++k)
            if (k < K) acc = fma(w[j][k], ext_aligned(min_[nb[j][k]], ein[nb[j][k]], E), acc);
        }
        ext_split(acc, E, &mout[s], &eout[s]);
      }
    }
    __syncthreads();
  }
  const double* zm = (collapsed & 1) ? manB : manA;
  const int* ze = (collapsed & 1) ? expB : expA;
  for (int s = tid; s < S; s += nt) ext_policy_row(a, b, s, zm, ze);
  if (tid == 0) a.status[b] = IRLMX_OK;
}

// ---------------------------------------------------------------------------
// per-sweep shape: one launch per sweep over all instances
// ---------------------------------------------------------------------------

__global__ void ext_init_kernel(ExtArgs a, ExtWs ws) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (s >= a.m.S) return;
  const size_t i = (size_t)b * a.m.S + s;
  ext_init_state(a.term[i] != 0, &ws.man[0][i], &ws.exp[0][i]);
}

__global__ void __launch_bounds__(kSweepThreads) ext_sweep_kernel(ExtArgs a, ExtWs ws, int odd) {
  const Model& m = a.m;
  const int S = m.S, K = m.K;
  const int b = blockIdx.y;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  const double* min_ = ws.man[odd] + (size_t)b * S;
  const int* ein = ws.exp[odd] + (size_t)b * S;
  const double* wb = a.w + (size_t)b * K * S;
  int E = kExtZero;
  for (int k = 0; k < K; ++k)
    if (wb[(size_t)k * S + s] != 0.0) E = max(E, ein[row_nbr(m, b, s, k)]);
  double acc = 0.0;
  for (int k = 0; k < K; ++k) {
    const int n = row_nbr(m, b, s, k);
    acc = fma(wb[(size_t)k * S + s], ext_aligned(min_[n], ein[n], E), acc);
  }
  const size_t o = (size_t)b * S + s;
  ext_split(acc, E, &ws.man[odd ^ 1][o], &ws.exp[odd ^ 1][o]);
}

__global__ void __launch_bounds__(kSweepThreads) ext_final_kernel(ExtArgs a, ExtWs ws, int odd) {
  const int S = a.m.S;
  const int b = blockIdx.y;
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  if (a.bad[b]) ext_nan_row(a, b, s);  // bwd_nonfinite_rule
  else ext_policy_row(a, b, s, ws.man[odd] + (size_t)b * S, ws.exp[odd] + (size_t)b * S);
  if (s == 0) a.status[b] = IRLMX_OK;
}

// ---------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------

// (SPT, KMAX) pairs instantiated: those of the ordinary fused backward
// (fused_pair_ok); every pair compiles without VGPR spills at
// __launch_bounds__(1024) (tools/kernel_resources.py).
static void (*ext_fused_fn(const FusedShape& f))(ExtArgs) {
  return with_pair<void (*)(ExtArgs)>(f.spt, f.kmax, [](auto s, auto k) {
    if constexpr (fused_pair_ok(IRLMX_OP_BACKWARD, s, k)) return &ext_fused_kernel<s, k>;
    else return nullptr;
  });
}

static size_t ext_fused_lds(const Model& m) { return (size_t)m.S * kExtLdsPerState; }

// The fused shape of the extended pass: the ordinary fused backward's thread
// layout at every width (there is no cluster form to prefer at 64 / 128), when
// its registers (an instantiated pair: fused_shape asks fused_pair_ok) and LDS
// fit; else the per-sweep shape.
static bool ext_fused_shape(const Model& m, FusedShape* out) {
  return fused_shape(m, IRLMX_OP_BACKWARD, out, false) && ext_fused_lds(m) <= kExtLdsMax;
}

// Sequential launches above which a batch goes per sweep instead
// (IRLMX_EXT_GRID_MAX_LAUNCHES; measured, DESIGN.md section 4 "Extended range").
constexpr int kExtGridMaxLaunches = 1;
// Fewest states of the grid shape (IRLMX_EXT_GRID_MIN_STATES): an absolute
// count, twice the fused limit, whatever IRLMX_FUSED_MAX_STATES says.
constexpr int kExtGridMinStates = 8192;

// Workgroups per CU a launch without XCD grouping is planned for.  Measured
// (DESIGN.md section 4 "Extended range"): four 256 x 256 instances at one state
// per thread, 1,024 workgroups at 4 per CU with their hand-offs crossing XCDs,
// ran 1,291 ms against 1,170 ms per sweep; at two states per thread, 512
// workgroups at 2 per CU, 959 ms.  Grouped launches (every instance inside one
// XCD's L2) keep the full capacity: 16 128 x 128 instances at 4 per CU, 4.0 us
// per sweep.
constexpr int kExtGridPerCuUngrouped = 2;

// The persistent grid shape of the extended pass (after the fused shape,
// before the per-sweep one): the smallest states-per-thread whose launches,
// each with as many instances as fit, stay within the launch cap.  Each
// instance within one XCD's share (grid_plan's rule, from 8 instances on) when
// that costs no further launch.
static bool ext_grid_plan(const Model& m, ExtGridPlan* out) {
  if (m.dense || env_int("IRLMX_GRID", 1) == 0) return false;
  if (m.S < env_int("IRLMX_EXT_GRID_MIN_STATES", kExtGridMinStates)) return false;
  if (m.A > kMaxActions || 2LL * m.S + 1 > 0xFFFFFLL) return false;  // sweep tags: 20 bits
  const int kmax = slot_class(m.K, 16);
  if (!kmax) return false;
  const int max_launches = env_int("IRLMX_EXT_GRID_MAX_LAUNCHES", kExtGridMaxLaunches);
  const int forced_cus = env_int("IRLMX_PLAN_CUS", 0);
  const int cus = forced_cus > 0 ? forced_cus : device_cus();
  for (int spt = 1; spt <= 4; spt *= 2) {
    void* fn = ext_grid_fn(spt, kmax);
    if (!fn) continue;
    const int bpi = (m.S + spt * kGridThreads - 1) / (spt * kGridThreads);
    if (bpi > kGridThreads) continue;  // the block words are gathered one per thread
    const int cap = launch_capacity(fn, kGridThreads);
    if (cap < bpi) continue;  // not even one instance is co-resident
    // (one instance alone may take the whole capacity: there is nothing to split)
    const int plain = std::min(m.B, std::max(1, std::min(cap, kExtGridPerCuUngrouped * cus) / bpi));
    const int grouped = 8 * ((cap / 8) / bpi);
    int ipl = plain, xcd = 0;
    if (env_int("IRLMX_XCD_GROUP", 1) != 0 && m.B >= 8 && grouped >= 8) {
      const int gi = std::min(m.B, grouped);
      if ((m.B + gi - 1) / gi <= (m.B + plain - 1) / plain) { ipl = gi; xcd = 1; }
    }
    const int launches = (m.B + ipl - 1) / ipl;
    if (launches > max_launches) continue;  // more states per thread: fewer workgroups per instance
    *out = ExtGridPlan{spt, kmax, bpi, xcd, ipl, launches};
    return true;
  }
  return false;
}

static ExtWs ext_carve(const Model& m, void* base, ExtGridWs* grid = nullptr) {
  ExtWs w;
  Carver c{(char*)base};
  const size_t B = m.B, S = m.S;
  FusedShape fs;
  const bool sweep = !ext_fused_shape(m, &fs);
  w.wgt = c.take<double>(B * m.K * S * sizeof(double));
  w.bad = c.take<int32_t>(B * sizeof(int32_t));
  for (int i = 0; i < 2; ++i) w.man[i] = c.take<double>(sweep ? B * S * sizeof(double) : 0);
  for (int i = 0; i < 2; ++i) w.exp[i] = c.take<int32_t>(sweep ? B * S * sizeof(int32_t) : 0);
  // grid shape: the granules of one launch's instances, beside the per-sweep
  // buffers (which its rerun needs)
  ExtGridPlan gp;
  ExtGridWs g{nullptr, nullptr, nullptr};
  if (sweep && ext_grid_plan(m, &gp)) {
    g.gran = c.take<unsigned long long>((size_t)gp.ipl * 6 * S * 16);
    g.dgran = c.take<unsigned long long>((size_t)gp.ipl * 4 * gp.bpi * 16);
    g.err = c.take<int>(4 * sizeof(int));
  }
  if (grid) *grid = g;
  w.total = c.total();
  return w;
}

int extended_check_model(const Model& m, const char* fn) {
  if (m.dense) {
    set_error("%s: the extended-range backward does not run the DENSE layout (STENCIL5 and ELL only)", fn);
    return IRLMX_EINVAL;
  }
  if (m.S > kExtMaxStates) {
    set_error("%s: the extended-range backward takes at most %d states, got %d", fn, kExtMaxStates, m.S);
    return IRLMX_EINVAL;
  }
  return 0;
}

size_t extended_workspace_bytes(const Model& m) { return ext_carve(m, nullptr).total; }

void extended_plan(const Model& m, int64_t* plan) {
  FusedShape fs;
  if (ext_fused_shape(m, &fs)) return plan_fused(plan, fs, ext_fused_lds(m));
  ExtGridPlan gp;
  if (ext_grid_plan(m, &gp)) {
    plan[0] = IRLMX_SHAPE_GRID;
    plan[2] = gp.xcd;
    plan[3] = gp.bpi;
    plan[4] = gp.ipl;
    plan[5] = gp.spt;
    plan[7] = kGridThreads;
    plan[8] = gp.launches;
    return;
  }
  plan_sweep(plan, 1, 2LL * m.S - 1);  // sweep launches (plus the weights, the start vector and the per-action sweep)
}

}  // namespace irlmx

using namespace irlmx;

extern "C" int irlmx_backward_maxent_extended(const irlmx_mdp* mdp, const double* reward, const uint8_t* terminal,
                                              double* p_action, int32_t* status, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  if (int rc = validate(mdp)) return rc;
  const Model m = make_model(mdp);
  if (int rc = extended_check_model(m, "backward_maxent_extended")) return rc;
  if (int rc = need_all("backward_maxent_extended",
                        {{reward, "reward"}, {terminal, "terminal"}, {p_action, "p_action"}, {status, "status"}}))
    return rc;
  // (the need is never 0 -- the weights and flags are always carved -- so a NULL workspace never passes)
  if (int rc = check_ws(ext_carve(m, nullptr).total, workspace_bytes, workspace)) return rc;
  hipStream_t st = (hipStream_t)stream;
  ExtGridWs gws;
  ExtWs ws = ext_carve(m, workspace, &gws);
  hipError_t e = hipMemsetAsync(ws.bad, 0, (size_t)m.B * sizeof(int32_t), st);
  if (e != hipSuccess) return hip_fail(e, "workspace memset");
  bwd_weights_launch(m, reward, ws.wgt, ws.bad, st);
  ExtArgs a{m, ws.wgt, reward, terminal, ws.bad, p_action, status};
  FusedShape fs;
  if (ext_fused_shape(m, &fs)) {
    void (*kfn)(ExtArgs) = ext_fused_fn(fs);
    if (!kfn) { set_error("no extended fused kernel for spt=%d kmax=%d", fs.spt, fs.kmax); return IRLMX_EINVAL; }
    return launch_fused(kfn, "ext_fused_kernel", m.B, fs.threads, ext_fused_lds(m), st, a);
  }
  ExtGridPlan gp;
  if (gws.gran && ext_grid_plan(m, &gp)) {  // persistent launches; a rendezvous miss reruns the whole call below
    const int rc = ext_grid_run(m, gp, a, gws, st);
    if (rc != kClusterNotResident) return rc;
  }
  const dim3 g = sweep_grid(m);
  count_event(IRLMX_CTR_SWEEP_CALLS);
  hipLaunchKernelGGL(ext_init_kernel, g, dim3(kSweepThreads), 0, st, a, ws);
  const long long collapsed = 2LL * m.S - 1;
  for (long long it = 0; it < collapsed; ++it)
    hipLaunchKernelGGL(ext_sweep_kernel, g, dim3(kSweepThreads), 0, st, a, ws, (int)(it & 1));
  hipLaunchKernelGGL(ext_final_kernel, g, dim3(kSweepThreads), 0, st, a, ws, (int)(collapsed & 1));
  e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, "extended backward");
}

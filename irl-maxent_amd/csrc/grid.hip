// Persistent grid shape: soft VI / VI on stencil grids and all four passes of
// ELL models with S > 4096 (the kernels, their planner and their launch; the
// entry points of fixed_point.hip choose the shape).
//
// One launch runs the whole loop.  Every workgroup owns SPT * kGridThreads
// states of one instance, keeps their weights, reward and terminal reward in
// registers, and exchanges values with the rest of the instance every sweep
// through tagged granules in HBM (cluster.h: one 16-byte write-through store
// {lo, tag, hi, tag} per value, tag = call salt | sweep; readers poll their
// five stencil neighbours with sc1 loads until the tags match -- the data is
// the flag, one fabric round trip per sweep and no global barrier).  The
// convergence word travels the same way: each workgroup publishes the max
// |v_new - v_old| of its states as one granule, and with sweep k's neighbour
// values every workgroup also gathers all of sweep k's block maxima, so all of
// them take the reference's decision (`while delta > eps`, NaN included: the
// maxima are ordered bits, fixed_point.hip header) at the same sweep.  Values
// and maxima live in rings of three sweeps: a workgroup can only write sweep
// k + 3 after every workgroup of the instance has published sweep k + 2, i.e.
// finished reading sweep k.  Per-state arithmetic is bellman_update's, in the
// same order: results bit-identical to the fused and per-sweep shapes.

#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "cluster.h"
#include "grid.h"

namespace irlmx {

constexpr int kGridMaxActions = 5;

struct GridArgs {
  unsigned long long* gran;   // [B][3][S] x 16 B
  unsigned long long* dgran;  // [B][4][bpi] x 16 B: three sweeps of block maxima + the XCC ids
  int* err;
  int bpi;
  int nb;                     // instances
  int xcd_group;              // workgroups dealt to XCD groups (see the kernel)
  unsigned salt;
  int n_resident;             // workgroups that must run at once (coresident(), cluster.h)
};

// every workgroup of the launch running at once, or none goes on (the err[1..2]
// counters; err bit kErrNotResident tells the host to rerun per sweep)
__device__ inline bool grid_coresident(const GridArgs& g) {
  __shared__ int resident;
  if (threadIdx.x == 0) resident = coresident(g.err + 1, g.n_resident) ? 1 : 0;
  __syncthreads();
  if (!resident && threadIdx.x == 0) atomicOr(g.err, kErrNotResident);
  return resident != 0;
}

template <bool SOFT, int SPT, int KMAX>
__global__ void __launch_bounds__(kGridThreads) bellman_grid_kernel(SoftArgs a, GridArgs g) {
  const Model& m = a.m;
  const int S = m.S, A = m.A, Kr = m.K;  // Kr <= KMAX slots: the stencil's five or the ELL row form's
  // XCD grouping (as cluster.hip): workgroups are dealt round-robin over the 8
  // XCDs, so the workgroups of instance g + 8 j are all taken from XCD group g
  // and its hand-offs can stay in one L2 (checked below; speed only).  The grid
  // is padded to 8 equal groups; padding workgroups leave at once.
  int lin = blockIdx.x;
  if (g.xcd_group) {
    const int grp = blockIdx.x % 8, kk = blockIdx.x / 8;
    const int il = grp + 8 * (kk / g.bpi);
    if (il >= g.nb) return;
    lin = il * g.bpi + kk % g.bpi;
  }
  const int b = lin / g.bpi, blk = lin % g.bpi, tid = threadIdx.x;
  __shared__ NpTables npt_lds;
  const NpTables* const npt = &npt_lds;
  if (SOFT) np_stage_tables(&npt_lds);  // numpy exp / log tables in LDS (common.h); grid_coresident synchronises
  if (!grid_coresident(g)) return;
  constexpr int K = KMAX;
  __shared__ unsigned long long red_in[kGridThreads / kWave], red_out[kGridThreads / kWave];
  __shared__ int lflag;
  int sidx[SPT];
  bool ok[SPT];
  int nb[SPT][K];
  double w[SPT][kGridMaxActions][K];
  double r[SPT], phi[SPT], cur[SPT], q[SPT][kGridMaxActions];
  const double v0 = SOFT ? -1e200 : 0.0;  // maxent.py:323 / solver.py:32
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = (blk * SPT + j) * kGridThreads + tid;
    sidx[j] = s;
    ok[j] = s < S;
    const int ss = ok[j] ? s : 0;
    r[j] = a.reward[(size_t)b * S + ss];
    phi[j] = SOFT ? a.phi[(size_t)b * S + ss] : 0.0;
    cur[j] = v0;
#pragma unroll
    for (int k = 0; k < K; ++k) nb[j][k] = k < Kr ? row_nbr(m, b, ss, k) : ss;
#pragma unroll
    for (int act = 0; act < kGridMaxActions; ++act) {
      q[j][act] = 0.0;
#pragma unroll
      for (int k = 0; k < K; ++k) w[j][act][k] = (act < A && k < Kr) ? row_val(m, b, act, k, ss) : 0.0;
    }
  }
  if (tid == 0) lflag = 0;
  const Gran rg = gran_rsrc(g.gran + (size_t)b * 6 * S, 48u * (unsigned)S);
  const Gran rd = gran_rsrc(g.dgran + (size_t)b * 8 * g.bpi, 64u * (unsigned)g.bpi);
  const unsigned salt = (g.salt & 0xFFFu) << 20;
  // hand-off store form: write-through (sc1) in general; plain stores (kept in the
  // XCD's L2, where the readers' sc1 loads are served) when every workgroup of
  // the instance runs on the same XCD -- found by exchanging XCC ids once
  bool plain = false;
  {
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcc &= 0xFu;
    const unsigned htag = salt | 0xFFFFFu;
    if (tid == 0) gran_store(rd, (3u * (unsigned)g.bpi + (unsigned)blk) * 16u, xcc, htag, false);
    unsigned off[1] = {(3u * (unsigned)g.bpi + (unsigned)tid) * 16u};
    unsigned long long v[1] = {xcc};
    if (!gran_gather<1>(rd, rd, off, tid < g.bpi ? 1u : 0u, htag, v)) lflag = 1;
    const unsigned long long diff = wave_or_u64(tid < g.bpi ? (v[0] ^ xcc) : 0ull);
    if ((tid & (kWave - 1)) == 0) red_in[tid / kWave] = diff;
    __syncthreads();
    if (lflag) {
      if (tid == 0) atomicOr(g.err, 1);
      return;
    }
    unsigned long long any = 0ull;
#pragma unroll
    for (int i = 0; i < kGridThreads / kWave; ++i) any |= red_in[i];
    plain = g.xcd_group && any == 0ull;
    __syncthreads();
  }
  double delta = 0.0;
  long long k = 0;  // sweeps done: cur = v_k
  for (;;) {
    double nv[SPT][K];
    if (k == 0) {
#pragma unroll
      for (int j = 0; j < SPT; ++j)
#pragma unroll
        for (int kk = 0; kk < K; ++kk) nv[j][kk] = v0;
    } else {
      // sweep k's neighbour values and (threads < bpi) all block maxima, one round trip
      const unsigned tag = salt | ((unsigned)k & 0xFFFFFu);
      const unsigned slot = (unsigned)(k % 3);
      unsigned off[SPT * K + 1];
      using mask_t = typename std::conditional<(SPT * K + 1 > 32), unsigned long long, unsigned>::type;
      mask_t want = 0;
#pragma unroll
      for (int j = 0; j < SPT; ++j)
#pragma unroll
        for (int kk = 0; kk < K; ++kk) {
          off[j * K + kk] = (slot * (unsigned)S + (unsigned)nb[j][kk]) * 16u;
          want |= (mask_t)(ok[j] && kk < Kr ? 1u : 0u) << (j * K + kk);
        }
      off[SPT * K] = (slot * (unsigned)g.bpi + (unsigned)tid) * 16u;
      want |= (mask_t)(tid < g.bpi ? 1u : 0u) << (SPT * K);
      unsigned long long v[SPT * K + 1];
      if (!gran_gather<SPT * K + 1>(rg, rd, off, want, tag, v)) lflag = 1;
#pragma unroll
      for (int j = 0; j < SPT; ++j)
#pragma unroll
        for (int kk = 0; kk < K; ++kk) nv[j][kk] = (ok[j] && kk < Kr) ? bits_double(v[j * K + kk]) : 0.0;
      unsigned long long d = tid < g.bpi ? v[SPT * K] : 0ull;
      d = wave_max_u64(d);
      if ((tid & (kWave - 1)) == 0) red_in[tid / kWave] = d;
      __syncthreads();
      if (lflag) {
        if (tid == 0) atomicOr(g.err, 1);
        return;
      }
      unsigned long long mx = 0ull;
#pragma unroll
      for (int i = 0; i < kGridThreads / kWave; ++i) mx = red_in[i] > mx ? red_in[i] : mx;
      delta = bits_double(mx);
      if (!(delta > a.eps) || (a.max_iter > 0 && k >= a.max_iter)) break;  // maxent.py:326 / solver.py:40
    }
    // sweep k + 1 (bellman_update's arithmetic and order)
    unsigned long long dmax = 0ull;
    const unsigned tag1 = salt | ((unsigned)(k + 1) & 0xFFFFFu);
    const unsigned slot1 = (unsigned)((k + 1) % 3);
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      double v = SOFT ? phi[j] : 0.0;
#pragma unroll
      for (int act = 0; act < kGridMaxActions; ++act) {
        if (act >= A) break;
        double dot = 0.0;
#pragma unroll
        for (int kk = 0; kk < K; ++kk)
          if (kk < Kr) dot = fma(w[j][act][kk], nv[j][kk], dot);
        if (SOFT) {
          q[j][act] = __dadd_rn(r[j], __dmul_rn(a.discount, dot));
          v = softmax2(v, q[j][act], npt, SPT == 1);  // maxent.py:329-333
        } else {
          const double qq = __dmul_rn(a.discount, dot);  // solver.py:44
          if (a.average) v = act == 0 ? qq : __dadd_rn(v, qq);
          else v = act == 0 ? qq : ((v != v || qq <= v) ? v : qq);
        }
      }
      if (!SOFT) v = __dadd_rn(r[j], a.average ? v / (double)A : v);  // solver.py:47 / :99
      if (ok[j]) {
        const unsigned long long d = abs_bits(v - cur[j]);
        dmax = d > dmax ? d : dmax;
        gran_store(rg, (slot1 * (unsigned)S + (unsigned)sidx[j]) * 16u, dbits(v), tag1, plain);
      }
      cur[j] = v;
    }
    dmax = wave_max_u64(dmax);
    if ((tid & (kWave - 1)) == 0) red_out[tid / kWave] = dmax;
    __syncthreads();
    if (tid == 0) {
      unsigned long long mx = 0ull;
      for (int i = 0; i < kGridThreads / kWave; ++i) mx = red_out[i] > mx ? red_out[i] : mx;
      gran_store(rd, (slot1 * (unsigned)g.bpi + (unsigned)blk) * 16u, mx, tag1, plain);
    }
    ++k;
  }
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    if (!ok[j]) continue;
    const size_t o = (size_t)b * S + sidx[j];
    if (a.value) a.value[o] = cur[j];
    if (SOFT)
      for (int act = 0; act < A; ++act) a.pi[o * A + act] = np_exp(q[j][act] - cur[j], npt);  // maxent.py:341
  }
  if (blk == 0 && tid == 0) {
    if (a.iters) a.iters[b] = k;
    a.status[b] = finish_status(delta, a.eps);
  }
}

// The grid shape for the linear loops of ELL models (generic sparsity, S > 4096):
// the forward (MODE kModeFwd: d <- p0 + sum_k w[k] d[src_k], until max|dd| <= eps;
// fwd_sweep_kernel's arithmetic) and the backward (kModeBwd: 2S - 1 collapsed
// sweeps zs <- ldexp(sum_k w[k] zs[nbr_k], e), e from the previous sweep's
// maximum, then the per-action sweep; bwd_sweep_kernel / bwd_final_kernel's
// arithmetic).  Same exchange as bellman_grid_kernel; the block maxima carry
// max|dd| (forward) or max|zs| (backward: the rescale exponent, and a NaN /
// inf there is bwd_nonfinite_rule's flag -- ordered bits sort them above every
// finite value).
template <int MODE, int SPT, int KMAX>
__global__ void __launch_bounds__(kGridThreads) linear_grid_kernel(LinearGridArgs a, GridArgs g) {
  const Model& m = a.m;
  const int S = m.S;
  const int Kr = MODE == kModeFwd ? m.Kc : m.K;
  int lin = blockIdx.x;
  if (g.xcd_group) {
    const int grp = blockIdx.x % 8, kk = blockIdx.x / 8;
    const int il = grp + 8 * (kk / g.bpi);
    if (il >= g.nb) return;
    lin = il * g.bpi + kk % g.bpi;
  }
  const int b = lin / g.bpi, blk = lin % g.bpi, tid = threadIdx.x;
  if (!grid_coresident(g)) return;
  constexpr int K = KMAX;
  __shared__ unsigned long long red_in[kGridThreads / kWave], red_out[kGridThreads / kWave];
  __shared__ int lflag;
  int sidx[SPT];
  bool ok[SPT];
  int nb[SPT][K];
  double w[SPT][K], c0[SPT], cur[SPT];
  if (MODE == kModeFwd && a.bad[b]) {  // non-finite policy: the reference's dense product is NaN after one sweep
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int s = (blk * SPT + j) * kGridThreads + tid;
      if (s < S) a.out[(size_t)b * S + s] = kNaN;
    }
    if (blk == 0 && tid == 0) { a.iters[b] = 1; a.status[b] = IRLMX_NONFINITE; }
    return;
  }
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = (blk * SPT + j) * kGridThreads + tid;
    sidx[j] = s;
    ok[j] = s < S;
    const int ss = ok[j] ? s : 0;
    c0[j] = MODE == kModeFwd ? a.vin[(size_t)b * S + ss] : 0.0;
    cur[j] = MODE == kModeBwd ? (a.term[(size_t)b * S + ss] ? 1.0 : 0.0) : 0.0;  // maxent.py:146-147 / d = 0
#pragma unroll
    for (int k = 0; k < K; ++k) {
      nb[j][k] = k < Kr ? (MODE == kModeFwd ? col_src(m, b, ss, k) : row_nbr(m, b, ss, k)) : ss;
      w[j][k] = k < Kr ? a.w[((size_t)b * Kr + k) * S + ss] : 0.0;
    }
  }
  if (tid == 0) lflag = 0;
  const Gran rg = gran_rsrc(g.gran + (size_t)b * 6 * S, 48u * (unsigned)S);
  const Gran rd = gran_rsrc(g.dgran + (size_t)b * 8 * g.bpi, 64u * (unsigned)g.bpi);
  const unsigned salt = (g.salt & 0xFFFu) << 20;
  bool plain = false;
  {  // XCC ids (bellman_grid_kernel)
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcc &= 0xFu;
    const unsigned htag = salt | 0xFFFFFu;
    if (tid == 0) gran_store(rd, (3u * (unsigned)g.bpi + (unsigned)blk) * 16u, xcc, htag, false);
    unsigned off[1] = {(3u * (unsigned)g.bpi + (unsigned)tid) * 16u};
    unsigned long long v[1] = {xcc};
    if (!gran_gather<1>(rd, rd, off, tid < g.bpi ? 1u : 0u, htag, v)) lflag = 1;
    const unsigned long long diff = wave_or_u64(tid < g.bpi ? (v[0] ^ xcc) : 0ull);
    if ((tid & (kWave - 1)) == 0) red_in[tid / kWave] = diff;
    __syncthreads();
    if (lflag) {
      if (tid == 0) atomicOr(g.err, 1);
      return;
    }
    unsigned long long any = 0ull;
#pragma unroll
    for (int i = 0; i < kGridThreads / kWave; ++i) any |= red_in[i];
    plain = g.xcd_group && any == 0ull;
    __syncthreads();
  }
  // backward: publish the start vector as sweep 0 (its neighbours read it)
  const long long total = MODE == kModeBwd ? 2LL * S - 1 : -1;
  double delta = 0.0;
  unsigned long long gmax = 0ull;  // backward: max |zs| of the vector the next sweep reads
  bool nonfinite = false;
  long long k = 0;
  if (MODE == kModeBwd) {
    const unsigned tag0 = salt | 1u;  // tag of sweep k: salt | (k + 1), never 0 (a zeroed workspace)
    unsigned long long dm = 0ull;
#pragma unroll
    for (int j = 0; j < SPT; ++j)
      if (ok[j]) {
        gran_store(rg, (unsigned)sidx[j] * 16u, dbits(cur[j]), tag0, plain);
        const unsigned long long d = abs_bits(cur[j]);
        dm = d > dm ? d : dm;
      }
    dm = wave_max_u64(dm);
    if ((tid & (kWave - 1)) == 0) red_out[tid / kWave] = dm;
    __syncthreads();
    if (tid == 0) {
      unsigned long long mx = 0ull;
      for (int i = 0; i < kGridThreads / kWave; ++i) mx = red_out[i] > mx ? red_out[i] : mx;
      gran_store(rd, (unsigned)blk * 16u, mx, tag0, plain);
    }
  }
  double nv[SPT][K];  // the neighbours' values of the vector the next sweep reads
  for (;;) {
    if (MODE == kModeFwd && k == 0) {
#pragma unroll
      for (int j = 0; j < SPT; ++j)
#pragma unroll
        for (int kk = 0; kk < K; ++kk) nv[j][kk] = 0.0;
    } else {
      const unsigned tag = salt | ((unsigned)(k + 1) & 0xFFFFFu);
      const unsigned slot = (unsigned)(k % 3);
      unsigned off[SPT * K + 1];
      using mask_t = typename std::conditional<(SPT * K + 1 > 32), unsigned long long, unsigned>::type;
      mask_t want = 0;
#pragma unroll
      for (int j = 0; j < SPT; ++j)
#pragma unroll
        for (int kk = 0; kk < K; ++kk) {
          off[j * K + kk] = (slot * (unsigned)S + (unsigned)nb[j][kk]) * 16u;
          want |= (mask_t)(ok[j] && kk < Kr ? 1u : 0u) << (j * K + kk);
        }
      off[SPT * K] = (slot * (unsigned)g.bpi + (unsigned)tid) * 16u;
      want |= (mask_t)(tid < g.bpi ? 1u : 0u) << (SPT * K);
      unsigned long long v[SPT * K + 1];
      if (!gran_gather<SPT * K + 1>(rg, rd, off, want, tag, v)) lflag = 1;
#pragma unroll
      for (int j = 0; j < SPT; ++j)
#pragma unroll
        for (int kk = 0; kk < K; ++kk) nv[j][kk] = (ok[j] && kk < Kr) ? bits_double(v[j * K + kk]) : 0.0;
      unsigned long long d = tid < g.bpi ? v[SPT * K] : 0ull;
      d = wave_max_u64(d);
      if ((tid & (kWave - 1)) == 0) red_in[tid / kWave] = d;
      __syncthreads();
      if (lflag) {
        if (tid == 0) atomicOr(g.err, 1);
        return;
      }
      unsigned long long mx = 0ull;
#pragma unroll
      for (int i = 0; i < kGridThreads / kWave; ++i) mx = red_in[i] > mx ? red_in[i] : mx;
      if (MODE == kModeFwd) {
        delta = bits_double(mx);
        if (!(delta > a.eps) || (a.max_iter > 0 && k >= a.max_iter)) break;  // maxent.py:108
      } else {
        gmax = mx;
        nonfinite |= mx >= 0x7FF0000000000000ull;  // some |zs| is inf or NaN
        if (k >= total) break;  // neighbours of zs_{2S-1} gathered: the per-action sweep
      }
    }
    const int e = (MODE == kModeBwd && a.rescale && k > 0) ? rescale_exponent(bits_double(gmax)) : 0;
    unsigned long long dmax = 0ull;
    const unsigned tag1 = salt | ((unsigned)(k + 2) & 0xFFFFFu);
    const unsigned slot1 = (unsigned)((k + 1) % 3);
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      double acc = 0.0;
#pragma unroll
      for (int kk = 0; kk < K; ++kk)
        if (kk < Kr) acc = fma(w[j][kk], nv[j][kk], acc);
      const double v = MODE == kModeFwd ? c0[j] + acc : ldexp(acc, e);
      if (ok[j]) {
        const unsigned long long d = MODE == kModeFwd ? abs_bits(v - cur[j]) : abs_bits(v);
        dmax = d > dmax ? d : dmax;
        gran_store(rg, (slot1 * (unsigned)S + (unsigned)sidx[j]) * 16u, dbits(v), tag1, plain);
      }
      cur[j] = v;
    }
    dmax = wave_max_u64(dmax);
    if ((tid & (kWave - 1)) == 0) red_out[tid / kWave] = dmax;
    __syncthreads();
    if (tid == 0) {
      unsigned long long mx = 0ull;
      for (int i = 0; i < kGridThreads / kWave; ++i) mx = red_out[i] > mx ? red_out[i] : mx;
      gran_store(rd, (slot1 * (unsigned)g.bpi + (unsigned)blk) * 16u, mx, tag1, plain);
    }
    ++k;
  }
  if (MODE == kModeFwd) {
#pragma unroll
    for (int j = 0; j < SPT; ++j)
      if (ok[j]) a.out[(size_t)b * S + sidx[j]] = cur[j];
    if (blk == 0 && tid == 0) { a.iters[b] = k; a.status[b] = finish_status(delta, a.eps); }
  } else {
    // the last of the 2*S sweeps, per action (bwd_final_kernel's arithmetic)
    const int A = m.A;
    const int e = a.rescale ? rescale_exponent(bits_double(gmax)) : 0;
    const bool all_nan = nonfinite || a.bad[b];
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      if (!ok[j]) continue;
      const int s = sidx[j];
      double* pr = a.out + ((size_t)b * S + s) * A;
      if (all_nan) {
        for (int act = 0; act < A; ++act) pr[act] = kNaN;
        continue;
      }
      const double er = exp(a.vin[(size_t)b * S + s]);
      double za[kMaxActions];
      double zsum = 0.0;
      for (int act = 0; act < A; ++act) {
        double acc = 0.0;
        for (int kk = 0; kk < Kr; ++kk) acc = fma(row_val(m, b, act, kk, s), nv[j][kk], acc);
        za[act] = ldexp(__dmul_rn(er, acc), e);
        zsum = __dadd_rn(zsum, za[act]);
      }
      for (int act = 0; act < A; ++act) pr[act] = za[act] / zsum;
    }
    if (blk == 0 && tid == 0) a.status[b] = IRLMX_OK;
  }
}

// (SPT, KMAX) pairs instantiated.  The Bellman loops hold A x K weights per
// state: up to 16 slots, fewer states per thread as the slots grow.  The linear
// loops hold one weight per slot (ELL rows / columns of generic sparse models):
// also <2, 16> and <1, 32>.
constexpr bool bellman_grid_pair_ok(int spt, int kmax) {
  return (kmax == 5 && spt <= 4) || (kmax == 8 && spt <= 2) || (kmax == 16 && spt == 1);
}
constexpr bool linear_grid_pair_ok(int spt, int kmax) {
  return bellman_grid_pair_ok(spt, kmax) || (kmax == 16 && spt == 2) || (kmax == 32 && spt == 1);
}

// The <T, SPT, KMAX> instantiation of a grid kernel, nullptr for a pair that is not compiled.
template <bool SOFT>
static void* bellman_grid_fn(int spt, int kmax) {
  return with_pair<void*>(spt, kmax, [](auto s, auto k) {
    if constexpr (bellman_grid_pair_ok(s, k)) return (void*)&bellman_grid_kernel<SOFT, s, k>;
    else return nullptr;
  });
}
template <int MODE>
static void* linear_grid_fn(int spt, int kmax) {
  return with_pair<void*>(spt, kmax, [](auto s, auto k) {
    if constexpr (linear_grid_pair_ok(s, k)) return (void*)&linear_grid_kernel<MODE, s, k>;
    else return nullptr;
  });
}

// slots per state the grid kernels hold in registers (slot_class): the linear
// loops up to 32, the Bellman loops up to 16
static int grid_kmax(const Model& m) { return slot_class(m.K, 16); }
static int grid_kmax_lin(const Model& m) { return slot_class(m.K, 32); }
static int grid_kmax_fwd(const Model& m) { return slot_class(m.Kc, 32); }

static void* grid_fn(const Model& m, int op, int spt) {
  switch (op) {
    case IRLMX_OP_SOFT_BACKWARD: return bellman_grid_fn<true>(spt, grid_kmax(m));
    case IRLMX_OP_VALUE_ITERATION: return bellman_grid_fn<false>(spt, grid_kmax(m));
    case IRLMX_OP_FORWARD: return linear_grid_fn<kModeFwd>(spt, grid_kmax_fwd(m));
    case IRLMX_OP_BACKWARD: return linear_grid_fn<kModeBwd>(spt, grid_kmax_lin(m));
  }
  return nullptr;
}

// the smallest states-per-thread whose grid is co-resident (all workgroups must
// run at once: they wait on each other's granules); IRLMX_GRID=0 disables
bool grid_plan(const Model& m, int op, GridPlan* out) {
  if (m.dense || env_int("IRLMX_GRID", 1) == 0) return false;
  if (m.S <= fused_max_states()) return false;  // one workgroup holds it: the fused shape
  if (op == IRLMX_OP_SOFT_BACKWARD || op == IRLMX_OP_VALUE_ITERATION) {
    if (m.A > kGridMaxActions || !grid_kmax(m)) return false;
  } else if (op == IRLMX_OP_FORWARD || op == IRLMX_OP_BACKWARD) {
    // stencil grids run the cluster shape; ELL rows / columns of at most 32 slots here
    if (m.stencil || !(op == IRLMX_OP_FORWARD ? grid_kmax_fwd(m) : grid_kmax_lin(m)) || m.A > kMaxActions) return false;
  } else {
    return false;
  }
  for (int spt = 1; spt <= 4; spt *= 2) {
    void* fn = grid_fn(m, op, spt);
    if (!fn) continue;
    const int bpi = (m.S + spt * kGridThreads - 1) / (spt * kGridThreads);
    if (bpi > kGridThreads) continue;  // the block maxima are gathered one per thread
    const int cap = launch_capacity(fn, kGridThreads);
    // XCD groups: ceil(B / 8) instances per group, each group within one XCD's
    // share -- only from 8 instances on: fewer would leave XCDs idle (one 128x128
    // instance: soft VI 3.5 ms grouped on one XCD vs 3.1 ms spread, 812 sweeps)
    const bool xcd = env_int("IRLMX_XCD_GROUP", 1) != 0 && cap >= 8 && m.B >= 8 &&
                     (long long)((m.B + 7) / 8) * bpi <= cap / 8;
    if (xcd || (long long)bpi * m.B <= cap) {
      *out = GridPlan{spt, bpi, xcd ? 1 : 0};
      return true;
    }
  }
  return false;
}

static std::atomic<unsigned> g_grid_salt{1};

template <class Args>
int grid_run(const Model& m, int op, const GridPlan& gp, Args a, const Ws& ws, hipStream_t st) {
  // (launch_test_knobs, tests only: one workgroup more than launched -> the per-sweep rerun)
  GridArgs ga{ws.gran, ws.sgran, ws.err, gp.bpi, m.B, gp.xcd, g_grid_salt.fetch_add(1, std::memory_order_relaxed),
              gp.bpi * m.B + launch_test_knobs().extra_resident};
  void* args[] = {&a, &ga};
  const int grid = gp.xcd ? 8 * ((m.B + 7) / 8) * gp.bpi : gp.bpi * m.B;
  hipError_t e = hipLaunchKernel(grid_fn(m, op, gp.spt), dim3(grid), dim3(kGridThreads), args, 0, st);
  if (e != hipSuccess) return hip_fail(e, "grid launch");
  count_event(IRLMX_CTR_GRID_LAUNCHES);
  return grid_launch_outcome(ws.err, "grid", st);
}
template int grid_run(const Model&, int, const GridPlan&, LinearGridArgs, const Ws&, hipStream_t);
template int grid_run(const Model&, int, const GridPlan&, SoftArgs, const Ws&, hipStream_t);

}  // namespace irlmx

// The four passes in numpy's floating-point order (the irlmx_*_numpy_order
// entry points): every rounding where numpy / OpenBLAS put it, so results are
// bit-identical to the reference's on a Haswell-family host.  One workgroup
// per instance for the whole loop, the vectors in LDS (S <= 4096); no
// workspace and no choice of shape, only a kernel per layout.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "numpy_order.h"

namespace irlmx {

// ---------------------------------------------------------------------------
// backward pass in numpy's floating-point order (irlmx_backward_maxent_numpy_order)
// ---------------------------------------------------------------------------
//
// maxent.py:142-159 with every rounding where numpy / OpenBLAS put it on a
// Haswell-family x86-64 host (oracle/blas_order.c states and pins the order):
// p[a].dot(zs) per action -- four lane accumulators by column % 4 over the
// first S & ~3 columns (fma lanes for rows s < S & ~3, rounded-product lanes
// for the last row when S % 4 == 1; blocks of 2048 columns), lane sum
// (l0 + l2) + (l1 + l3), the last column fused on -- then er * dot rounded,
// zs = ((za0 + za1) + za2) + za3, and za / zs after exactly 2 S sweeps.  No
// rescaling: it overflows to NaN exactly where the reference does.  er is the
// caller's np.exp(reward) (ocml's exp may differ from numpy's in the last bit).
// One workgroup per instance; zs ping-pongs in LDS (S <= 4096).

constexpr int kNpBlock = 2048;  // OpenBLAS dgemv_t NBMAX

struct NpArgs {
  Model m;
  const double* er;     // [B][S] exp(reward), numpy's
  const uint8_t* term;  // [B][S]
  double* pi;           // [B][S][A]
  int32_t* status;
};

// one lane term: fma lanes (dgemv_kernel_4x4) or product-then-add lanes (dgemv_kernel_4x1)
__device__ inline void np_lane(double (&l)[2][4], int c, double v, double x, bool fused) {
  double& acc = l[c >= kNpBlock ? 1 : 0][c & 3];
  acc = fused ? fma(v, x, acc) : __dadd_rn(acc, __dmul_rn(v, x));
}

// p[a][s, :] . x in OpenBLAS dgemv_t order, from the row's stored entries in
// ascending column order (zero entries are exact no-ops while x is finite)
template <int LAYOUT>
__device__ double np_row_dot(const Model& m, int b, int a, int s, const double* x) {
  const int S = m.S, m1 = S & ~3;
  const bool fused = s < m1;
  double l[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
  double tail_v = 0.0;
  bool tail = false;
  auto put = [&](int c, double v) {
    if (c < m1) np_lane(l, c, v, x[c], fused);
    // S % 4 == 1: the one column c = S - 1 (an unused ELL slot may repeat it with value 0)
    else if (!tail || v != 0.0) { tail = true; tail_v = v; }
  };
  if (LAYOUT == IRLMX_LAYOUT_STENCIL5) {
    // ascending columns: -y, -x, self, +x, +y (k = 4, 2, 0, 1, 3)
    constexpr int order[kStencilK] = {4, 2, 0, 1, 3};
#pragma unroll
    for (int i = 0; i < kStencilK; ++i) {
      const int k = order[i];
      if (stencil_valid(s, k, m.W, m.H)) put(stencil_nbr(s, k, m.W, m.H), row_val(m, b, a, k, s));
    }
  } else if (LAYOUT == IRLMX_LAYOUT_ELL) {
    for (int k = 0; k < m.K; ++k) put(row_nbr(m, b, s, k), row_val(m, b, a, k, s));
  } else {
    const double* row = m.row_val + ((inst_of(m, b) * m.A + a) * (size_t)S + s) * S;
    for (int c = 0; c < S; ++c) put(c, row[c]);
  }
  double y = __dadd_rn(0.0, __dadd_rn(__dadd_rn(l[0][0], l[0][2]), __dadd_rn(l[0][1], l[0][3])));
  if (m1 > kNpBlock) y = __dadd_rn(y, __dadd_rn(__dadd_rn(l[1][0], l[1][2]), __dadd_rn(l[1][1], l[1][3])));
  if (tail) y = fma(tail_v, x[S - 1], y);
  return y;
}

// p'[a][:, t] . x in OpenBLAS dgemv_n order (numpy's P_a.T.dot(x), maxent.py:109;
// oracle/blas_order.c blas_order_dgemv_cols): for t < S & ~3 the sources in
// groups of four, each group one chain c = fma(.., c) in source order 4g + 1,
// 4g, 4g + 2, 4g + 3 (its first term a rounded product), added to the sum group
// after group; a last source s = S - 1 (S % 4 == 1) as a rounded product added
// last; the last output t = S - 1 one fma chain over the sources in order.
// Zero entries (terminal sources, unused slots) are exact no-ops while x is
// finite, so only stored entries are visited.  xs(s) = pi[s, a] * d[s], rounded.
constexpr int kNpColMax = 32;  // ELL column slots the numpy-order forward supports

template <int LAYOUT, typename XS>
__device__ double np_col_dot(const Model& m, int b, int a, int t, const uint8_t* term, XS xs) {
  const int S = m.S, n4 = S & ~3;
  if (LAYOUT == IRLMX_LAYOUT_DENSE) {
    const double* col = m.row_val + (inst_of(m, b) * m.A + a) * (size_t)S * S + t;  // P[s, t, a] at s * S
    auto v = [&](int s) { return term[s] ? 0.0 : col[(size_t)s * S]; };
    double out = 0.0;
    if (t >= n4) {
      for (int s = 0; s < S; ++s) out = fma(v(s), xs(s), out);
      return out;
    }
    for (int s = 0; s < n4; s += 4) {
      double c = __dmul_rn(v(s + 1), xs(s + 1));
      c = fma(v(s), xs(s), c);
      c = fma(v(s + 2), xs(s + 2), c);
      c = fma(v(s + 3), xs(s + 3), c);
      out = __dadd_rn(out, c);
    }
    for (int s = n4; s < S; ++s) out = __dadd_rn(out, __dmul_rn(v(s), xs(s)));
    return out;
  }
  // stored entries of column t, ascending by source
  constexpr int KM = LAYOUT == IRLMX_LAYOUT_STENCIL5 ? kStencilK : kNpColMax;
  int src[KM];
  double val[KM];
  int n = 0;
  if (LAYOUT == IRLMX_LAYOUT_STENCIL5) {
    constexpr int order[kStencilK] = {4, 2, 0, 1, 3};  // sources t - W, t - 1, t, t + 1, t + W
#pragma unroll
    for (int i = 0; i < kStencilK; ++i) {
      const int k = order[i];
      if (!stencil_valid(t, k, m.W, m.H)) continue;
      const int s = stencil_nbr(t, k, m.W, m.H);
      if (term[s]) continue;
      src[n] = s;
      val[n] = row_val(m, b, a, stencil_opposite(k), s);  // P[s, t, a]
      ++n;
    }
  } else {
    for (int k = 0; k < m.Kc && k < kNpColMax; ++k) {
      const int s = col_src(m, b, t, k);
      const double v = m.col_val[((inst_of(m, b) * m.A + a) * m.Kc + k) * S + t];
      if (term[s] || v == 0.0) continue;
      int j = n++;  // insertion by source (unused slots repeat t with value 0 and are skipped)
      for (; j > 0 && src[j - 1] > s; --j) { src[j] = src[j - 1]; val[j] = val[j - 1]; }
      src[j] = s;
      val[j] = v;
    }
  }
  double out = 0.0;
  if (t >= n4) {
    for (int i = 0; i < n; ++i) out = fma(val[i], xs(src[i]), out);
    return out;
  }
  int i = 0;
  while (i < n && src[i] < n4) {
    const int g = src[i] >> 2;
    int e = i;
    while (e < n && src[e] < n4 && (src[e] >> 2) == g) ++e;
    double c = 0.0;
    constexpr int qorder[4] = {1, 0, 2, 3};
#pragma unroll
    for (int qi = 0; qi < 4; ++qi)
      for (int j = i; j < e; ++j)
        if ((src[j] & 3) == qorder[qi]) c = fma(val[j], xs(src[j]), c);
    out = __dadd_rn(out, c);
    i = e;
  }
  for (; i < n; ++i) out = __dadd_rn(out, __dmul_rn(val[i], xs(src[i])));
  return out;
}

struct NpFwdArgs {
  Model m;
  const double* p0;     // [B][S]
  const uint8_t* term;  // [B][S]
  const double* pi;     // [B][S][A]
  double eps;
  long long max_iter;
  double* svf;          // [B][S]
  int64_t* iters;
  int32_t* status;
};

// Forward in numpy's order (irlmx_forward_svf_numpy_order): maxent.py:105-114
// with every rounding where numpy puts it -- x_a = pi[:, a] * d, y_a = P'_a^T x_a
// (np_col_dot), d_ = p0 + (((y_0 + y_1) + y_2) + ...), delta = max|d_ - d| -- so
// the SVF and the sweep count are bit-identical to the reference's on a
// Haswell-family host.  A non-finite policy or value meets the zero entries of
// the dense product (0 * NaN): every later entry is NaN, as in the reference.
template <int LAYOUT>
__global__ void __launch_bounds__(1024) fwd_numpy_order_kernel(NpFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Model& m = a.m;
  const int S = m.S, A = m.A;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  double* const buf0 = (double*)smem;  // (two named LDS pointers, not an array: ds_* accesses, not flat)
  double* const buf1 = buf0 + S;
  unsigned long long* slot = (unsigned long long*)(buf1 + S);  // [3] delta ring
  int* bad = (int*)(slot + 3);                                     // [2] sticky non-finite, by parity
  const double* pi = a.pi + (size_t)b * S * A;
  const double* p0 = a.p0 + (size_t)b * S;
  const uint8_t* term = a.term + (size_t)b * S;
  bool nf = false;
  for (int s = tid; s < S; s += nt) {
    buf0[s] = 0.0;  // maxent.py:105
    for (int act = 0; act < A; ++act) nf |= !isfinite(pi[(size_t)s * A + act]);
  }
  if (tid < 3) slot[tid] = 0ull;
  if (tid < 2) bad[tid] = 0;
  __syncthreads();
  if (nf) bad[1] = 1;  // a non-finite policy: the first sweep's product is NaN everywhere
  __syncthreads();
  long long it = 0;
  int r3 = 0;
  double delta = 0.0;
  for (;;) {
    const double* d = ((it & 1) ? buf1 : buf0);
    double* dn = ((it & 1) ? buf0 : buf1);
    const bool poisoned = bad[(it & 1) ^ 1] != 0;  // written in the previous sweep (or above)
    unsigned long long mx = 0ull;
    bool nfo = false;
    for (int t = tid; t < S; t += nt) {
      double v = 0.0;
      for (int act = 0; act < A; ++act) {
        auto xs = [&](int s) { return __dmul_rn(pi[(size_t)s * A + act], d[s]); };  // maxent.py:109
        const double y = poisoned ? kNaN : np_col_dot<LAYOUT>(m, b, act, t, term, xs);
        v = act == 0 ? y : __dadd_rn(v, y);  // np.array(d_).sum(axis=0)
      }
      const double nv = __dadd_rn(p0[t], v);  // maxent.py:110
      dn[t] = nv;
      nfo |= !isfinite(nv);
      const unsigned long long dd = abs_bits(nv - d[t]);
      mx = dd > mx ? dd : mx;
    }
    if (nfo) bad[it & 1] = 1;
    mx = wave_max_u64(mx);
    if ((tid & (kWave - 1)) == 0 && mx) atomicMax(&slot[r3], mx);
    if (tid == 0) slot[r3 == 2 ? 0 : r3 + 1] = 0ull;
    __syncthreads();
    delta = bits_double(slot[r3]);
    r3 = r3 == 2 ? 0 : r3 + 1;
    ++it;
    if (!(delta > a.eps)) break;  // maxent.py:108
    if (a.max_iter > 0 && it >= a.max_iter) break;
  }
  const double* d = ((it & 1) ? buf1 : buf0);
  for (int t = tid; t < S; t += nt) a.svf[(size_t)b * S + t] = d[t];
  if (tid == 0) {
    a.iters[b] = it;
    a.status[b] = finish_status(delta, a.eps);
  }
}

// The same forward for a STENCIL5 model with TPT targets per thread (512
// threads; S <= 1024, A <= 4): each thread keeps its targets' sources, the
// processing order of np_col_dot and every P[s, t, a] and pi[s, a] it
// multiplies in registers, so a sweep is five LDS reads per target and the
// chains -- no global load, no index arithmetic (the general kernel re-derives
// them every sweep, ~15 us per sweep at 64 states).
constexpr int kNpCachedThreads = 512;
constexpr int kNpCachedMaxStates = 2 * kNpCachedThreads;
constexpr int kNpCachedMaxActions = 4;
template <int TPT>
__global__ void __launch_bounds__(kNpCachedThreads) fwd_numpy_order_cached_kernel(NpFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Model& m = a.m;
  const int S = m.S, A = m.A, n4 = S & ~3;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  double* const buf0 = (double*)smem;  // (two named LDS pointers, not an array: ds_* accesses, not flat)
  double* const buf1 = buf0 + S;
  unsigned long long* slot = (unsigned long long*)(buf1 + S);
  int* bad = (int*)(slot + 3);
  const double* pi = a.pi + (size_t)b * S * A;
  const uint8_t* term = a.term + (size_t)b * S;
  // per target j: entries in processing order; kind: 0 chain continues, 1 chain
  // starts (the previous chain's sum added first), 2 tail source (rounded
  // product added), 3 tail output (one fma chain).  (Every array is indexed by
  // compile-time constants only: registers, not scratch.)
  int src[TPT][kStencilK], kind[TPT][kStencilK], n[TPT];
  double val[TPT][kNpCachedMaxActions][kStencilK], pw[TPT][kNpCachedMaxActions][kStencilK], p0t[TPT];
  constexpr int order[kStencilK] = {4, 2, 0, 1, 3};  // candidate sources t - W, t - 1, t, t + 1, t + W
#pragma unroll
  for (int j = 0; j < TPT; ++j) {
    const int t = tid + j * nt;
    n[j] = 0;
    p0t[j] = 0.0;
#pragma unroll
    for (int p = 0; p < kStencilK; ++p) {
      src[j][p] = 0;
      kind[j][p] = 0;
#pragma unroll
      for (int act = 0; act < kNpCachedMaxActions; ++act) { val[j][act][p] = 0.0; pw[j][act][p] = 0.0; }
    }
    if (t >= S) continue;
    p0t[j] = a.p0[(size_t)b * S + t];
    int cs[kStencilK], key[kStencilK];
    bool ok[kStencilK];
#pragma unroll
    for (int i = 0; i < kStencilK; ++i) {
      ok[i] = stencil_valid(t, order[i], m.W, m.H);
      cs[i] = stencil_nbr(t, order[i], m.W, m.H);
      ok[i] = ok[i] && !term[cs[i]];  // P' rows of terminal states are zero (maxent.py:99)
      // processing key: group, then source order 4g + 1, 4g, 4g + 2, 4g + 3; tail sources after
      const int q = cs[i] & 3;
      key[i] = t >= n4 ? cs[i] : (cs[i] < n4 ? 4 * (cs[i] >> 2) + (q == 1 ? 0 : q == 0 ? 1 : q) : 4 * S + cs[i]);
    }
#pragma unroll
    for (int i = 0; i < kStencilK; ++i) {
      if (!ok[i]) continue;
      int pos = 0;
      bool first = true;  // lowest key of its group among the valid sources
#pragma unroll
      for (int q = 0; q < kStencilK; ++q) {
        pos += (ok[q] && key[q] < key[i]) ? 1 : 0;
        first = first && !(ok[q] && key[q] < key[i] && (cs[q] >> 2) == (cs[i] >> 2));
      }
      const int kd = t >= n4 ? 3 : (cs[i] >= n4 ? 2 : (first ? 1 : 0));
#pragma unroll
      for (int p = 0; p < kStencilK; ++p)
        if (pos == p) {
          src[j][p] = cs[i];
          kind[j][p] = kd;
#pragma unroll
          for (int act = 0; act < kNpCachedMaxActions; ++act) {
            val[j][act][p] = act < A ? row_val(m, b, act, stencil_opposite(order[i]), cs[i]) : 0.0;
            pw[j][act][p] = act < A ? pi[(size_t)cs[i] * A + act] : 0.0;
          }
        }
      ++n[j];
    }
  }
  bool nf = false;
  for (int s = tid; s < S; s += nt) {
    buf0[s] = 0.0;  // maxent.py:105
    for (int act = 0; act < A; ++act) nf |= !isfinite(pi[(size_t)s * A + act]);
  }
  if (tid < 3) slot[tid] = 0ull;
  if (tid < 2) bad[tid] = 0;
  __syncthreads();
  if (nf) bad[1] = 1;
  __syncthreads();
  // convergence deferred over blocks of sweeps, replay of the stopping block
  // (run_deferred); the poison flags bad[] are part of the block-start state
  long long it = 0;
  auto sweep = [&](long long it, int pos, unsigned long long& bits) __attribute__((always_inline)) {
    const double* d = ((it & 1) ? buf1 : buf0);
    double* dn = ((it & 1) ? buf0 : buf1);
    const bool poisoned = bad[(it & 1) ^ 1] != 0;
    bool nfo = false;
#pragma unroll
    for (int j = 0; j < TPT; ++j) {
      const int t = tid + j * nt;
      if (t >= S) continue;
      double dv[kStencilK];
#pragma unroll
      for (int i = 0; i < kStencilK; ++i) dv[i] = d[src[j][i]];  // (unused entries: src 0, selected away below)
      // all actions' chains side by side, branch-free (the entries' kinds differ
      // between lanes): every step computes its candidates and selects, so the
      // four independent chains interleave instead of diverging
      double out[kNpCachedMaxActions], c[kNpCachedMaxActions];
#pragma unroll
      for (int act = 0; act < kNpCachedMaxActions; ++act) { out[act] = 0.0; c[act] = 0.0; }
      bool open = false;
#pragma unroll
      for (int i = 0; i < kStencilK; ++i) {
        const int kd = i < n[j] ? kind[j][i] : -1;  // -1: no entry
        const bool flush = open && (kd == 1 || kd == 2);
#pragma unroll
        for (int act = 0; act < kNpCachedMaxActions; ++act) {
          // every candidate computed, then selected: a conditional operator
          // around an arithmetic call compiles to an exec-mask branch per step
          const double vv = val[j][act][i];
          const double x = __dmul_rn(pw[j][act][i], dv[i]);  // maxent.py:109
          const double oc = __dadd_rn(out[act], c[act]);
          const double o1 = flush ? oc : out[act];
          const double cf = fma(vv, x, kd == 1 ? 0.0 : c[act]);
          const double f3 = fma(vv, x, out[act]);
          const double a2 = __dadd_rn(o1, __dmul_rn(vv, x));
          c[act] = (kd == 0 || kd == 1) ? cf : c[act];
          out[act] = kd == 3 ? f3 : (kd == 2 ? a2 : o1);
        }
        open = kd == 1 ? true : (kd == 2 ? false : open);
      }
      double v = 0.0;
#pragma unroll
      for (int act = 0; act < kNpCachedMaxActions; ++act) {
        if (act >= A) break;
        const double oc = __dadd_rn(out[act], c[act]);
        const double o = open ? oc : out[act];
        const double y = poisoned ? kNaN : o;
        v = act == 0 ? y : __dadd_rn(v, y);  // np.array(d_).sum(axis=0)
      }
      const double nv = __dadd_rn(p0t[j], v);  // maxent.py:110
      dn[t] = nv;
      nfo |= !isfinite(nv);
      record_delta(bits, pos, fabs(nv - d[t]), a.eps);
    }
    if (nfo) bad[it & 1] = 1;
  };
  double keep[TPT];
  int bad0 = 0, bad1 = 0;
  const int status = run_deferred(
      a.max_iter, slot, it, sweep,
      [&]() {
        const double* d0 = ((it & 1) ? buf1 : buf0);
#pragma unroll
        for (int j = 0; j < TPT; ++j) keep[j] = tid + j * nt < S ? d0[tid + j * nt] : 0.0;
        bad0 = bad[0];
        bad1 = bad[1];
      },
      [&]() {
        double* d0w = ((it & 1) ? buf1 : buf0);
#pragma unroll
        for (int j = 0; j < TPT; ++j)
          if (tid + j * nt < S) d0w[tid + j * nt] = keep[j];
        __syncthreads();  // every lane past its reads of bad[] before they are restored
        if (tid == 0) { bad[0] = bad0; bad[1] = bad1; }
        __syncthreads();
      });
  for (int t = tid; t < S; t += nt) a.svf[(size_t)b * S + t] = ((it & 1) ? buf1 : buf0)[t];
  if (tid == 0) {
    a.iters[b] = it;
    a.status[b] = status;
  }
}

// A thread's stencil rows in registers for the numpy-order kernels (TPT states
// per thread, A <= 4): per state j and candidate column i (ascending: -y, -x,
// self, +x, +y) the column, its dgemv lane (column % 4; 4 = the last column
// S - 1 of an S % 4 == 1 grid, fused on after the lane sum; -1 = off-grid) and
// P[s, c, a] -- np_row_dot's arithmetic without re-deriving indices or
// re-loading P every sweep.  Static indices only: registers, not scratch.
template <int TPT>
struct NpStencilRows {
  int col[TPT][kStencilK], lane[TPT][kStencilK];
  double val[TPT][kNpCachedMaxActions][kStencilK];

  __device__ __attribute__((always_inline)) void load(const Model& m, int b, int tid, int nt) {
    constexpr int order[kStencilK] = {4, 2, 0, 1, 3};
    const int S = m.S, m1 = S & ~3;
#pragma unroll
    for (int j = 0; j < TPT; ++j) {
      const int s = tid + j * nt;
#pragma unroll
      for (int i = 0; i < kStencilK; ++i) {
        const bool ok = s < S && stencil_valid(s, order[i], m.W, m.H);
        col[j][i] = ok ? stencil_nbr(s, order[i], m.W, m.H) : 0;
        lane[j][i] = ok ? (col[j][i] < m1 ? (col[j][i] & 3) : 4) : -1;
#pragma unroll
        for (int act = 0; act < kNpCachedMaxActions; ++act)
          val[j][act][i] = (ok && act < m.A) ? row_val(m, b, act, order[i], s) : 0.0;
      }
    }
  }
  // the vector at state j's columns
  __device__ __attribute__((always_inline)) void gather(int j, const double* v, double (&x)[kStencilK]) const {
#pragma unroll
    for (int i = 0; i < kStencilK; ++i) x[i] = lane[j][i] >= 0 ? v[col[j][i]] : 0.0;
  }
  // p[act][s, :] . v in OpenBLAS dgemv_t order (fused: rows s < S & ~3)
  __device__ __attribute__((always_inline)) double dot(int j, int act, bool fused, const double (&x)[kStencilK]) const {
    double l[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < kStencilK; ++i)  // ascending columns within a lane
        if (lane[j][i] == q)
          l[q] = fused ? fma(val[j][act][i], x[i], l[q]) : __dadd_rn(l[q], __dmul_rn(val[j][act][i], x[i]));
    double y = __dadd_rn(0.0, __dadd_rn(__dadd_rn(l[0], l[2]), __dadd_rn(l[1], l[3])));
#pragma unroll
    for (int i = 0; i < kStencilK; ++i)
      if (lane[j][i] == 4) y = fma(val[j][act][i], x[i], y);
    return y;
  }
};

// The numpy-order backward for a STENCIL5 model with TPT states per thread
// (512 threads; S <= 1024, A <= 4), the rows in registers (NpStencilRows).
template <int TPT>
__global__ void __launch_bounds__(kNpCachedThreads) bwd_numpy_order_cached_kernel(NpArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Model& m = a.m;
  const int S = m.S, A = m.A, m1 = S & ~3;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  double* const zbuf0 = (double*)smem;  // (two named LDS pointers, not an array: ds_* accesses, not flat)
  double* const zbuf1 = zbuf0 + S;
  int* bad = (int*)(zbuf1 + S);
  const double* er = a.er + (size_t)b * S;
  double* pi = a.pi + (size_t)b * S * A;
  NpStencilRows<TPT> rows;
  rows.load(m, b, tid, nt);
  double ers[TPT];
#pragma unroll
  for (int j = 0; j < TPT; ++j) ers[j] = tid + j * nt < S ? er[tid + j * nt] : 0.0;
  for (int s = tid; s < S; s += nt) zbuf0[s] = a.term[(size_t)b * S + s] ? 1.0 : 0.0;  // maxent.py:146-147
  if (tid < 2) bad[tid] = 0;
  __syncthreads();
  const long long n = 2LL * S;  // maxent.py:154
  for (long long it = 0; it < n; ++it) {
    const double* zin = ((it & 1) ? zbuf1 : zbuf0);
    double* zout = ((it & 1) ? zbuf0 : zbuf1);
    if (it > 0 && bad[(it - 1) & 1]) {  // the reference's overflow: NaN from here on (bwd_numpy_order_kernel)
      for (int s = tid; s < S; s += nt)
        for (int act = 0; act < A; ++act) pi[(size_t)s * A + act] = kNaN;
      if (tid == 0) a.status[b] = IRLMX_OK;
      return;
    }
    bool nf = false;
#pragma unroll
    for (int j = 0; j < TPT; ++j) {
      const int s = tid + j * nt;
      if (s >= S) continue;
      double x[kStencilK];
      rows.gather(j, zin, x);
      double z = 0.0;
#pragma unroll
      for (int act = 0; act < kNpCachedMaxActions; ++act) {
        if (act >= A) break;
        const double za = __dmul_rn(ers[j], rows.dot(j, act, s < m1, x));  // maxent.py:155
        z = act == 0 ? za : __dadd_rn(z, za);                               // maxent.py:156
        if (it == n - 1) pi[(size_t)s * A + act] = za;
      }
      zout[s] = z;
      nf |= !isfinite(z);
    }
    if (nf) bad[it & 1] = 1;
    __syncthreads();
  }
  const double* zs = ((n & 1) ? zbuf1 : zbuf0);
  for (int s = tid; s < S; s += nt)
    for (int act = 0; act < A; ++act) pi[(size_t)s * A + act] = pi[(size_t)s * A + act] / zs[s];  // maxent.py:159
  if (tid == 0) a.status[b] = IRLMX_OK;
}

template <int LAYOUT>
__global__ void __launch_bounds__(1024) bwd_numpy_order_kernel(NpArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Model& m = a.m;
  const int S = m.S, A = m.A;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  double* const zbuf0 = (double*)smem;  // (two named LDS pointers, not an array: ds_* accesses, not flat)
  double* const zbuf1 = zbuf0 + S;
  int* bad = (int*)(zbuf1 + S);  // [2] sticky: sweep k's output had a non-finite value (slot k & 1)
  const double* er = a.er + (size_t)b * S;
  double* pi = a.pi + (size_t)b * S * A;
  for (int s = tid; s < S; s += nt) zbuf0[s] = a.term[(size_t)b * S + s] ? 1.0 : 0.0;  // maxent.py:146-147
  if (tid < 2) bad[tid] = 0;
  __syncthreads();
  const long long n = 2LL * S;  // maxent.py:154
  for (long long it = 0; it < n; ++it) {
    const double* zin = ((it & 1) ? zbuf1 : zbuf0);
    double* zout = ((it & 1) ? zbuf0 : zbuf1);
    // a non-finite zs meets a zero entry of every dense row (0 * inf): the
    // reference's next dots are all NaN (a DENSE row visits every column itself)
    const bool poisoned = LAYOUT != IRLMX_LAYOUT_DENSE && it > 0 && bad[(it - 1) & 1];
    if (poisoned) {
      // from here every dot, za and zs is NaN (the overflow the reference hits at
      // about 13 x 13 and unit reward): the policy is NaN, no need to sweep on
      for (int s = tid; s < S; s += nt)
        for (int act = 0; act < A; ++act) pi[(size_t)s * A + act] = kNaN;
      if (tid == 0) a.status[b] = IRLMX_OK;
      return;
    }
    bool nf = false;
    for (int s = tid; s < S; s += nt) {
      double z = 0.0;
      for (int act = 0; act < A; ++act) {
        const double dot = np_row_dot<LAYOUT>(m, b, act, s, zin);
        const double za = __dmul_rn(er[s], dot);                 // maxent.py:155
        z = act == 0 ? za : __dadd_rn(z, za);                    // maxent.py:156
        if (it == n - 1) pi[(size_t)s * A + act] = za;
      }
      zout[s] = z;
      nf |= !isfinite(z);
    }
    if (nf) bad[it & 1] = 1;
    __syncthreads();
  }
  const double* zs = ((n & 1) ? zbuf1 : zbuf0);
  for (int s = tid; s < S; s += nt)
    for (int act = 0; act < A; ++act) pi[(size_t)s * A + act] = pi[(size_t)s * A + act] / zs[s];  // maxent.py:159
  if (tid == 0) a.status[b] = IRLMX_OK;
}

// Soft VI / VI in numpy's floating-point order (irlmx_soft_backward /
// irlmx_value_iteration with IRLMX_NUMPY_ORDER): every p[a].dot(v) as
// np_row_dot sums it, then the per-sweep kernel's statements.  VI has no
// transcendental function, so its values are bit-identical to the reference's
// on a Haswell-family host; soft VI's exp / log are ocml's (numpy's SIMD exp /
// log may differ in the last bit), its dot products follow numpy's order.
template <bool SOFT, int LAYOUT>
__global__ void __launch_bounds__(1024) bellman_numpy_order_kernel(SoftArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Model& m = a.m;
  const int S = m.S, A = m.A;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  __shared__ NpTables npt_lds;
  const NpTables* const npt = &npt_lds;
  double* const buf0 = (double*)smem;  // (two named LDS pointers, not an array: ds_* accesses, not flat)
  double* const buf1 = buf0 + S;
  unsigned long long* slot = (unsigned long long*)(buf1 + S);
  const double v0 = SOFT ? -1e200 : 0.0;  // maxent.py:323 / solver.py:29
  const double* rw = a.reward + (size_t)b * S;
  for (int s = tid; s < S; s += nt) buf0[s] = v0;
  if (tid < 3) slot[tid] = 0ull;
  if (SOFT) np_stage_tables(&npt_lds);  // numpy exp / log tables in LDS (common.h)
  __syncthreads();
  long long it = 0;
  int r3 = 0;
  double delta = 0.0;
  for (;;) {
    const double* vin = ((it & 1) ? buf1 : buf0);
    double* vout = ((it & 1) ? buf0 : buf1);
    unsigned long long mx = 0ull;
    for (int s = tid; s < S; s += nt) {
      const double r = rw[s];
      double v = SOFT ? a.phi[(size_t)b * S + s] : 0.0;
      for (int act = 0; act < A; ++act) {
        const double dot = np_row_dot<LAYOUT>(m, b, act, s, vin);
        if (SOFT) {
          v = softmax2(v, __dadd_rn(r, __dmul_rn(a.discount, dot)), npt, true);  // maxent.py:329-333
        } else {
          const double q = __dmul_rn(a.discount, dot);  // solver.py:44
          if (a.average) v = act == 0 ? q : __dadd_rn(v, q);
          else v = act == 0 ? q : ((v != v || q <= v) ? v : q);
        }
      }
      if (!SOFT) v = __dadd_rn(r, a.average ? v / (double)A : v);  // solver.py:47 / :99
      vout[s] = v;
      const unsigned long long d = abs_bits(v - vin[s]);
      mx = d > mx ? d : mx;
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
  const double* vold = ((it & 1) ? buf0 : buf1);  // input of the last sweep
  const double* vnew = ((it & 1) ? buf1 : buf0);
  for (int s = tid; s < S; s += nt) {
    if (a.value) a.value[(size_t)b * S + s] = vnew[s];
    if (SOFT)
      for (int act = 0; act < A; ++act) {
        const double q = __dadd_rn(rw[s], __dmul_rn(a.discount, np_row_dot<LAYOUT>(m, b, act, s, vold)));
        a.pi[((size_t)b * S + s) * A + act] = np_exp(q - vnew[s], npt);  // maxent.py:341
      }
  }
  if (tid == 0) {
    if (a.iters) a.iters[b] = it;
    a.status[b] = finish_status(delta, a.eps);
  }
}

// Soft VI / VI in numpy's order for a STENCIL5 model with TPT states per
// thread (512 threads; S <= 1024, A <= 4), the rows in registers (NpStencilRows).
template <bool SOFT, int TPT>
__global__ void __launch_bounds__(kNpCachedThreads) bellman_numpy_order_cached_kernel(SoftArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Model& m = a.m;
  const int S = m.S, A = m.A, m1 = S & ~3;
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  __shared__ NpTables npt_lds;
  const NpTables* const npt = &npt_lds;
  double* const buf0 = (double*)smem;  // (two named LDS pointers, not an array: ds_* accesses, not flat)
  double* const buf1 = buf0 + S;
  unsigned long long* slot = (unsigned long long*)(buf1 + S);
  const double v0 = SOFT ? -1e200 : 0.0;  // maxent.py:323 / solver.py:29
  NpStencilRows<TPT> rows;
  rows.load(m, b, tid, nt);
  double rr[TPT], ph[TPT];
#pragma unroll
  for (int j = 0; j < TPT; ++j) {
    const int s = tid + j * nt;
    rr[j] = s < S ? a.reward[(size_t)b * S + s] : 0.0;
    ph[j] = (SOFT && s < S) ? a.phi[(size_t)b * S + s] : 0.0;
  }
  for (int s = tid; s < S; s += nt) buf0[s] = v0;
  if (tid < 3) slot[tid] = 0ull;
  if (SOFT) np_stage_tables(&npt_lds);  // numpy exp / log tables in LDS (common.h)
  __syncthreads();
  // convergence deferred over blocks of sweeps, replay of the stopping block
  // (run_deferred: the stop after the first sweep whose max|v_new - v| is not
  // > eps, NaN included -- solver.py:49, maxent.py:335)
  long long it = 0;
  auto sweep = [&](long long it, int pos, unsigned long long& bits) __attribute__((always_inline)) {
    const double* vin = ((it & 1) ? buf1 : buf0);
    double* vout = ((it & 1) ? buf0 : buf1);
#pragma unroll
    for (int j = 0; j < TPT; ++j) {
      const int s = tid + j * nt;
      if (s >= S) continue;
      double x[kStencilK];
      rows.gather(j, vin, x);
      double v = SOFT ? ph[j] : 0.0;
#pragma unroll
      for (int act = 0; act < kNpCachedMaxActions; ++act) {
        if (act >= A) break;
        const double dot = rows.dot(j, act, s < m1, x);
        if (SOFT) {
          v = softmax2(v, __dadd_rn(rr[j], __dmul_rn(a.discount, dot)), npt, true);  // maxent.py:329-333
        } else {
          const double q = __dmul_rn(a.discount, dot);  // solver.py:44
          if (a.average) v = act == 0 ? q : __dadd_rn(v, q);
          else v = act == 0 ? q : ((v != v || q <= v) ? v : q);
        }
      }
      if (!SOFT) v = __dadd_rn(rr[j], a.average ? v / (double)A : v);  // solver.py:47 / :99
      vout[s] = v;
      record_delta(bits, pos, fabs(v - vin[s]), a.eps);
    }
  };
  // (VI: a reduction per sweep, as in bellman_fused_body)
  double keep[TPT];
  int status;
  if constexpr (SOFT) {
    status = run_deferred(
        a.max_iter, slot, it, sweep,
        [&]() {
          const double* v0p = ((it & 1) ? buf1 : buf0);
#pragma unroll
          for (int j = 0; j < TPT; ++j) keep[j] = tid + j * nt < S ? v0p[tid + j * nt] : 0.0;
        },
        [&]() {
          double* v0w = ((it & 1) ? buf1 : buf0);
#pragma unroll
          for (int j = 0; j < TPT; ++j)
            if (tid + j * nt < S) v0w[tid + j * nt] = keep[j];
          __syncthreads();
        });
  } else {
    status = run_each(a.max_iter, slot, it, sweep);
  }
  const double* vold = ((it & 1) ? buf0 : buf1);  // input of the last sweep
  const double* vnew = ((it & 1) ? buf1 : buf0);
#pragma unroll
  for (int j = 0; j < TPT; ++j) {
    const int s = tid + j * nt;
    if (s >= S) continue;
    if (a.value) a.value[(size_t)b * S + s] = vnew[s];
    if (SOFT) {
      double x[kStencilK];
      rows.gather(j, vold, x);
#pragma unroll
      for (int act = 0; act < kNpCachedMaxActions; ++act) {
        if (act >= A) break;
        const double q = __dadd_rn(rr[j], __dmul_rn(a.discount, rows.dot(j, act, s < m1, x)));
        a.pi[((size_t)b * S + s) * A + act] = np_exp(q - vnew[s], npt);  // maxent.py:341
      }
    }
  }
  if (tid == 0) {
    if (a.iters) a.iters[b] = it;
    a.status[b] = status;
  }
}

}  // namespace irlmx

using namespace irlmx;

// np_row_dot sums an ELL row's entries in slot order, which is numpy's order
// only when every action's nonzero entries sit in ascending column order
// (irlmx_dense_to_ell's layout; unused slots, value 0, are exact no-ops
// anywhere).  One thread per (table instance, row): *bad set on a violation.
__global__ void np_ell_ascending_kernel(Model m, int* bad) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (s >= m.S) return;
  for (int a = 0; a < m.A; ++a) {
    int last = -1;
    for (int k = 0; k < m.K; ++k) {
      if (row_val(m, b, a, k, s) == 0.0) continue;
      const int c = m.row_idx[((size_t)b * m.K + k) * m.S + s];
      if (c <= last) { atomicOr(bad, 1); return; }
      last = c;
    }
  }
}

int irlmx::ell_rows_sorted(const Model& m, hipStream_t st, bool* sorted) {
  int* flag = nullptr;
  hipError_t e = hipMallocAsync((void**)&flag, sizeof(int), st);
  if (e != hipSuccess) return hip_fail(e, "ELL row-order check");
  int h = 0;
  e = hipMemsetAsync(flag, 0, sizeof(int), st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(np_ell_ascending_kernel, dim3((m.S + 255) / 256, m.shared ? 1 : m.B), dim3(256), 0, st, m,
                       flag);
    e = hipMemcpyAsync(&h, flag, sizeof(int), hipMemcpyDeviceToHost, st);
  }
  (void)hipFreeAsync(flag, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_fail(e, "ELL row-order check");
  *sorted = h == 0;
  return 0;
}

// The numpy-order row dots' precondition on an ELL model (above); other
// layouts visit their entries in column order by construction.  From the
// model's properties when the caller supplied them (irlmx_mdp_properties: once
// per table), else checked on the device per call (synchronises).
static int np_check_ell_rows(const Model& m, const char* fn, hipStream_t st) {
  if (m.stencil || m.dense) return 0;
  bool sorted = true;
  if (m.props & IRLMX_PROPS_KNOWN) sorted = (m.props & IRLMX_PROP_ELL_SORTED) != 0;
  else if (int rc = ell_rows_sorted(m, st, &sorted)) return rc;
  if (!sorted) {
    set_error("%s: an ELL row holds its nonzero entries out of ascending column order (numpy's order needs "
              "irlmx_dense_to_ell's slot layout)", fn);
    return IRLMX_EINVAL;
  }
  return 0;
}

// numpy's order is restated for these sizes only
static int np_check_size(const Model& m, const char* fn) {
  if (m.S <= kFusedMaxStates && (m.S & 3) <= 1) return 0;
  set_error("%s: numpy's order is restated for S <= %d with S %% 4 in {0, 1}, got S=%d", fn, kFusedMaxStates, m.S);
  return IRLMX_EINVAL;
}

// The kernels of one numpy-order pass: STENCIL5 with the rows in registers at
// one and at two states per thread, then the general kernel of the STENCIL5,
// DENSE and ELL layouts.
template <class Args>
using NpKernels = void (*const[5])(Args);

// One workgroup per instance with `lds` bytes; `fn` names the pass in the error text.
template <class Args>
static int np_launch(NpKernels<Args>& k, const Model& m, const Args& a, size_t lds, const char* fn,
                     hipStream_t st) {
  const bool cached = m.stencil && m.S <= kNpCachedMaxStates && m.A <= kNpCachedMaxActions;
  void (*kfn)(Args) = k[cached ? (m.S <= kNpCachedThreads ? 0 : 1) : m.stencil ? 2 : (m.dense ? 3 : 4)];
  const int nthr = cached ? std::min(kNpCachedThreads, ((m.S + kWave - 1) / kWave) * kWave)
                          : (m.S >= 1024 ? 1024 : ((m.S + kWave - 1) / kWave) * kWave);
  return launch_fused(kfn, fn, m.B, nthr, lds, st, a);
}

template <bool SOFT>
static constexpr NpKernels<SoftArgs> kNpBellman = {
    bellman_numpy_order_cached_kernel<SOFT, 1>, bellman_numpy_order_cached_kernel<SOFT, 2>,
    bellman_numpy_order_kernel<SOFT, IRLMX_LAYOUT_STENCIL5>, bellman_numpy_order_kernel<SOFT, IRLMX_LAYOUT_DENSE>,
    bellman_numpy_order_kernel<SOFT, IRLMX_LAYOUT_ELL>};

extern "C" int irlmx_backward_maxent_numpy_order(const irlmx_mdp* mdp, const double* exp_reward,
                                                 const uint8_t* terminal, double* p_action, int32_t* status,
                                                 void* stream) {
  if (int rc = validate(mdp)) return rc;
  const Model m = make_model(mdp);
  if (int rc = need_all("backward_maxent_numpy_order", {{exp_reward, "exp_reward"}, {terminal, "terminal"},
                                                        {p_action, "p_action"}, {status, "status"}}))
    return rc;
  if (int rc = np_check_size(m, "backward_maxent_numpy_order")) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = np_check_ell_rows(m, "backward_maxent_numpy_order", st)) return rc;
  static constexpr NpKernels<NpArgs> k = {
      bwd_numpy_order_cached_kernel<1>, bwd_numpy_order_cached_kernel<2>, bwd_numpy_order_kernel<IRLMX_LAYOUT_STENCIL5>,
      bwd_numpy_order_kernel<IRLMX_LAYOUT_DENSE>, bwd_numpy_order_kernel<IRLMX_LAYOUT_ELL>};
  return np_launch(k, m, NpArgs{m, exp_reward, terminal, p_action, status},
                   2 * (size_t)m.S * sizeof(double) + 2 * sizeof(int), "backward_maxent_numpy_order", st);
}

extern "C" int irlmx_forward_svf_numpy_order(const irlmx_mdp* mdp, const double* p_initial,
                                             const uint8_t* terminal, const double* p_action, double eps,
                                             int64_t max_iter, double* svf, int64_t* iterations, int32_t* status,
                                             void* stream) {
  if (int rc = validate(mdp)) return rc;
  const Model m = make_model(mdp);
  if (int rc = need_all("forward_svf_numpy_order", {{p_initial, "p_initial"}, {terminal, "terminal"},
                                                    {p_action, "p_action"}, {svf, "svf"},
                                                    {iterations, "iterations"}, {status, "status"}}))
    return rc;
  if (int rc = np_check_size(m, "forward_svf_numpy_order")) return rc;
  if (mdp->layout == IRLMX_LAYOUT_ELL && (!m.col_idx || !m.col_val || m.Kc <= 0 || m.Kc > kNpColMax)) {
    set_error("forward_svf_numpy_order: ELL column form missing or k_col > %d", kNpColMax);
    return IRLMX_EINVAL;
  }
  static constexpr NpKernels<NpFwdArgs> k = {
      fwd_numpy_order_cached_kernel<1>, fwd_numpy_order_cached_kernel<2>, fwd_numpy_order_kernel<IRLMX_LAYOUT_STENCIL5>,
      fwd_numpy_order_kernel<IRLMX_LAYOUT_DENSE>, fwd_numpy_order_kernel<IRLMX_LAYOUT_ELL>};
  return np_launch(k, m, NpFwdArgs{m, p_initial, terminal, p_action, eps, (long long)max_iter, svf, iterations, status},
                   2 * (size_t)m.S * sizeof(double) + 3 * sizeof(unsigned long long) + 2 * sizeof(int),
                   "forward_svf_numpy_order", (hipStream_t)stream);
}

// Soft VI / VI in numpy's order: one workgroup per instance (S <= 4096, S % 4 in {0, 1}).
static int bellman_numpy_order(const irlmx_mdp* mdp, const double* reward, const double* phi, double discount,
                               double eps, int64_t max_iter, int average, double* p_action, double* value,
                               int64_t* iterations, int32_t* status, void* stream, bool soft) {
  if (int rc = validate(mdp)) return rc;
  const Model m = make_model(mdp);
  const char* fn = soft ? "soft_backward_numpy_order" : "value_iteration_numpy_order";
  if (int rc = need_all(fn, {{reward, "reward"}, {phi, soft ? "terminal_reward" : nullptr},
                             {p_action, soft ? "p_action" : nullptr}, {value, soft ? nullptr : "value"},
                             {iterations, "iterations"}, {status, "status"}}))
    return rc;
  if (int rc = np_check_size(m, fn)) return rc;
  if (int rc = np_check_ell_rows(m, fn, (hipStream_t)stream)) return rc;
  const SoftArgs a{m, reward, phi, discount, eps, (long long)max_iter, average, p_action, value, iterations, status};
  return np_launch(soft ? kNpBellman<true> : kNpBellman<false>, m, a,
                   2 * (size_t)m.S * sizeof(double) + 4 * sizeof(unsigned long long), fn, (hipStream_t)stream);
}

extern "C" int irlmx_soft_backward_numpy_order(const irlmx_mdp* mdp, const double* reward,
                                               const double* terminal_reward, double discount, double eps,
                                               int64_t max_iter, double* p_action, double* value,
                                               int64_t* iterations, int32_t* status, void* stream) {
  return bellman_numpy_order(mdp, reward, terminal_reward, discount, eps, max_iter, 0, p_action, value, iterations,
                             status, stream, true);
}

extern "C" int irlmx_value_iteration_numpy_order(const irlmx_mdp* mdp, const double* reward, double discount,
                                                 double eps, int32_t average, int64_t max_iter, double* value,
                                                 int64_t* iterations, int32_t* status, void* stream) {
  return bellman_numpy_order(mdp, reward, nullptr, discount, eps, max_iter, average, nullptr, value, iterations,
                             status, stream, false);
}

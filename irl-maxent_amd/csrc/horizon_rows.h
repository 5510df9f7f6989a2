// The per-state statements of the finite-horizon passes, shared by horizon.hip,
// soft_horizon.hip and expected_svf_horizon.hip so that all three compile the
// same text: the MaxEnt backward row (hz_row with its slot class compiled in,
// hz_row_loop with run-time loops) and hz_log_z, the MaxCausalEnt backward row
// (sh_row) and the value pass's row (tp_row, its slot loop slot_dot), and
// the forward step's folded weight and state (hz_fwd_weight, hz_fwd_state).
// hz_row_loop and sh_row have a value-only form (ROW = false): the same
// function with the statements that only the policy row needs compiled out.
#pragma once

#include <hip/hip_runtime.h>

#include "extended.h"
#include "horizon.h"

namespace irlmx {

// log Z = e * ln 2 + log m; -inf for an exact zero
__device__ inline double hz_log_z(double mant, int e) {
  if (e == kExtZero) return -(double)INFINITY;
  return fma((double)e, 0x1.62e42fefa39efp-1, log(mant));
}

// One state of one backward step with its slot class compiled in (nbr(k) is
// target_k(s), tab(act, k) is P[s, target_k(s), act]).  UNROLL: the action
// loop is unrolled, which a table held in registers needs (constant indices).
// A table read from memory keeps it rolled, so that only one action's loads
// are in flight (unrolled, the compiler hoists all A * K of them and spills),
// and za rests in the output row between the sum and the division (a dynamic
// index into registers would go to scratch).  From 16 slots on the slot loop
// is rolled too and nothing per slot is held.  Returns zsum, *Eout its
// alignment exponent.
template <int AMAX, int KMAX, bool UNROLL, class Nbr, class Tab>
__device__ __attribute__((always_inline)) inline double hz_row(int K, int A, double er, const double* zm,
                                                               const int* ze, Nbr&& nbr, unsigned any, Tab&& tab,
                                                               double* out, int* Eout) {
  int E = kExtZero;
  constexpr bool kHold = KMAX <= 8;  // neighbours read once, aligned once; else LDS is read per action
  double z[kHold ? KMAX : 1];
  if constexpr (kHold) {
    int e[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        e[k] = ze[nbr(k)];
        if ((any >> k) & 1u) E = max(E, e[k]);
      }
#pragma unroll
    for (int k = 0; k < KMAX; ++k) z[k] = k < K ? ext_aligned(zm[nbr(k)], e[k], E) : 0.0;
  } else {
#pragma unroll 4
    for (int k = 0; k < K; ++k)
      if ((any >> k) & 1u) E = max(E, ze[nbr(k)]);
  }
  auto action = [&](int act) __attribute__((always_inline)) {
    double acc = 0.0;
    if constexpr (kHold) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) acc = fma(tab(act, k), z[k], acc);
    } else {  // rolled: unrolled, 16 or 32 slots of loads in flight spill
#pragma unroll 4
      for (int k = 0; k < K; ++k) {
        const int n = nbr(k);
        acc = fma(tab(act, k), ext_aligned(zm[n], ze[n], E), acc);
      }
    }
    return __dmul_rn(er, acc);
  };
  double zsum = 0.0;
  if constexpr (UNROLL) {
    double za[AMAX];
#pragma unroll
    for (int act = 0; act < AMAX; ++act)
      if (act < A) {
        za[act] = action(act);
        zsum = __dadd_rn(zsum, za[act]);
      }
#pragma unroll
    for (int act = 0; act < AMAX; ++act)
      if (act < A) out[act] = za[act] / zsum;
  } else {
#pragma unroll 1
    for (int act = 0; act < A; ++act) {
      const double za = action(act);
      out[act] = za;
      zsum = __dadd_rn(zsum, za);
    }
#pragma unroll 1
    for (int act = 0; act < A; ++act) out[act] = out[act] / zsum;
  }
  *Eout = E;
  return zsum;
}

// The same statements with run-time loops (per-sweep shape: any K).  ROW =
// false is the value alone (expected_svf_horizon.hip's value-only steps): no
// za[], no division and nothing written to `out`, on which zsum does not depend.
template <bool ROW = true>
__device__ inline double hz_row_loop(const Model& m, int b, int s, double er, const double* zm, const int* ze,
                                     double* out, int* Eout) {
  const int K = m.K, A = m.A;
  int E = kExtZero;
  for (int k = 0; k < K; ++k) {
    bool any = false;
    for (int act = 0; act < A; ++act) any |= row_val(m, b, act, k, s) != 0.0;
    if (any) E = max(E, ze[row_nbr(m, b, s, k)]);
  }
  double za[ROW ? kMaxActions : 1];
  double zsum = 0.0;
  for (int act = 0; act < A; ++act) {
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
      const int n = row_nbr(m, b, s, k);
      acc = fma(row_val(m, b, act, k, s), ext_aligned(zm[n], ze[n], E), acc);
    }
    const double z = __dmul_rn(er, acc);
    if constexpr (ROW) za[act] = z;
    zsum = __dadd_rn(zsum, z);
  }
  if constexpr (ROW)
    for (int act = 0; act < A; ++act) out[act] = za[act] / zsum;
  *Eout = E;
  return zsum;
}

// Folded forward weight of slot k of target t under pi_t (`pit`: the step's
// [S][A] rows of instance b) and its source state: fwd_weights_kernel's access.
__device__ inline double hz_fwd_weight(const Model& m, int b, int t, int k, const double* __restrict__ pit,
                                       const uint8_t* __restrict__ tb, int* src) {
  const int S = m.S, A = m.A;
  double acc = 0.0;
  if (m.stencil) {
    const int s = stencil_nbr(t, k, m.W, m.H);
    *src = s;
    if (stencil_valid(t, k, m.W, m.H) && !(tb && tb[s])) {
      const int kk = stencil_opposite(k);  // direction from s back to t
      for (int a = 0; a < A; ++a) acc = fma(row_val(m, b, a, kk, s), pit[(size_t)s * A + a], acc);
    }
  } else {
    const int s = col_src(m, b, t, k);
    *src = s;
    if (!(tb && tb[s])) {
      const size_t base = inst_of(m, b) * A;
      for (int a = 0; a < A; ++a) acc = fma(m.col_val[((base + a) * m.Kc + k) * S + t], pit[(size_t)s * A + a], acc);
    }
  }
  return acc;
}

__device__ inline double hz_fwd_state(const Model& m, int b, int t, const double* __restrict__ pit,
                                      const uint8_t* __restrict__ tb, const double* din) {
  double acc = 0.0;
  for (int k = 0; k < m.Kc; ++k) {
    int u;
    const double w = hz_fwd_weight(m, b, t, k, pit, tb, &u);
    acc = fma(w, din[u], acc);
  }
  return acc;
}

// acc = fma(P[s, target_k(s), act], vin[target_k(s)], acc) from 0 over the
// slots in slot order.  KMAX > 0: the slot class is compiled in, and up to 8
// slots the loop is unrolled (nbr(k) may then be a register copy); from 16
// slots on, and with KMAX = 0 (per-sweep shape: any K), it is rolled.
template <int KMAX, class Nbr>
__device__ __attribute__((always_inline)) inline double slot_dot(const Model& m, int b, int act, int s,
                                                                 const double* vin, Nbr&& nbr) {
  const int K = m.K;
  double acc = 0.0;
  if constexpr (KMAX > 0 && KMAX <= 8) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) acc = fma(row_val(m, b, act, k, s), vin[nbr(k)], acc);
  } else {
#pragma unroll 1
    for (int k = 0; k < K; ++k) acc = fma(row_val(m, b, act, k, s), vin[nbr(k)], acc);
  }
  return acc;
}

// One state of one soft step (soft_horizon.hip's steps 1 - 3): writes the
// policy row `out`, returns v.  ROW = false is the value alone
// (expected_svf_horizon.hip's value-only steps): q_a is not parked in `out` and
// the closing exp of the row, on which v does not depend, is absent.
// The slot loop is slot_dot's, written out: called, the inlined loop's exit
// block is laid out behind the loop, and next to the inlined exp / log that
// costs expected_svf_horizon.hip's fused CAUSAL kernel three more spilled SGPRs
// and the soft step up to 1 % of its time (profiles/horizon_fold_resources.txt).
template <int KMAX, bool ROW = true, class Nbr>
__device__ __attribute__((always_inline)) inline double sh_row(const Model& m, int b, int s, double r, double discount,
                                                               const double* vin, Nbr&& nbr, const NpTables* tabs,
                                                               double* out) {
  const int K = m.K, A = m.A;
  double v = 0.0;
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
    const double q = __dadd_rn(r, __dmul_rn(discount, acc));
    if constexpr (ROW) out[act] = q;
    v = act == 0 ? q : softmax2(v, q, tabs);
  }
  if constexpr (ROW) {
#pragma unroll 1
    for (int act = 0; act < A; ++act) out[act] = np_exp(__dsub_rn(out[act], v), tabs);  // maxent.py:341
  }
  return v;
}

// One state of one step of the value pass (soft_horizon.hip's value steps
// 1 - 3; the terminal rule is the caller's).  `pis`: the policy row pi_t(s, :)
// or null (the optimal value).
template <int KMAX, class Nbr>
__device__ __attribute__((always_inline)) inline double tp_row(const Model& m, int b, int s, double r, double discount,
                                                               const double* vin, Nbr&& nbr, const double* pis) {
  const int A = m.A;
  double v = 0.0;  // the running maximum, or the policy's expectation e
#pragma unroll 1
  for (int act = 0; act < A; ++act) {
    const double acc = slot_dot<KMAX>(m, b, act, s, vin, nbr);
    if (pis) {
      v = fma(pis[act], acc, v);
    } else {
      const double q = __dadd_rn(r, __dmul_rn(discount, acc));
      v = act == 0 ? q : ((v != v || q <= v) ? v : q);  // irlmx_value_iteration's maximum
    }
  }
  return pis ? __dadd_rn(r, __dmul_rn(discount, v)) : v;
}

}  // namespace irlmx

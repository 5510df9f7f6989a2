// Device helpers the trajectory kernels share (rollout.hip: stationary policies;
// timed.hip: time-indexed ones): the counter-based generator, the pick rule, the
// histogram add and the guard of a stored trajectory.  rollout.hip's head comment
// states the rules; include/irlmx.h states them for the caller.
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

namespace irlmx {

constexpr int kRollThreads = 256;

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

// The pick rule (rollout.hip) over w(0) .. w(n - 1); -1 for an invalid row.
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

// ll[b] = the sequential sum of ll_traj[b][0..N): one thread per instance (the body of
// demo_ll_sum_kernel and of timed.hip's tp_ll_sum_kernel)
__device__ inline void ll_sum(int B, int N, const double* __restrict__ ll_traj, double* ll) {
  const int b = blockIdx.x * kRollThreads + threadIdx.x;
  if (b >= B) return;
  double acc = 0.0;
  for (int n = 0; n < N; ++n) acc = __dadd_rn(acc, ll_traj[(size_t)b * N + n]);
  ll[b] = acc;
}

inline unsigned traj_blocks(long long n) { return (unsigned)((n + kRollThreads - 1) / kRollThreads); }

// n_states / n_actions / batch / n_traj / stride of the calls on stored trajectories
inline int check_demo_sizes(const char* fn, int S, int A, int B, int N, int stride) {
  if (S < 1 || A < 1 || B < 1) {
    set_error("%s: bad sizes S=%d A=%d B=%d", fn, S, A, B);
    return IRLMX_EINVAL;
  }
  if (N < 1) { set_error("%s: n_traj=%d < 1", fn, N); return IRLMX_EINVAL; }
  if (stride < 1) { set_error("%s: stride=%d < 1", fn, stride); return IRLMX_EINVAL; }
  return 0;
}

}  // namespace irlmx

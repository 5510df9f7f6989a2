// Persistent grid shape of the extended-range backward (extended.hip): one
// launch runs all 2*S sweeps of up to `ipl` instances.
//
// The shape is grid.hip's (linear_grid_kernel<kModeBwd>): every workgroup owns
// SPT * kGridThreads states of one instance, keeps their collapsed weights and
// neighbour indices in registers, and exchanges values with the rest of the
// instance every sweep through the stock tagged granules of cluster.h.  A
// partition value m * 2^e travels as two granules side by side, the
// mantissa's 64 bits and the int32 exponent (kExtZero for an exact zero); a
// thread gathers its neighbours' pairs and one block word in a single
// gran_gather pass.  Values live in rings of three sweeps.
//
// The block word: after every sweep each workgroup publishes one granule that
// carries no data, and with sweep k's pairs every workgroup gathers all block
// words of sweep k.  It is what makes the ring of three safe.  A workgroup
// publishes its word of sweep k + 1 after the barrier that ends its gather of
// sweep k; so whoever holds every word of sweep k + 2 knows that sweep k + 1,
// and with it sweep k, has been read everywhere, and may overwrite slot k % 3
// with sweep k + 3.  The neighbour pairs alone do not say that on an ELL
// model, where the states that read a workgroup's values need not be the
// states it reads from.
//
// No rescale maximum, no convergence test, a fixed sweep count: one barrier per
// sweep.  Per-state arithmetic is ext_sweep_kernel's and ext_policy_row's,
// statement for statement: results bit-identical to the other two shapes.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "cluster.h"
#include "extended.h"
#include "grid.h"

namespace irlmx {

struct ExtGridArgs {
  unsigned long long* gran;   // [nb][3][S][2] x 16 B
  unsigned long long* dgran;  // [nb][4][bpi] x 16 B: three sweeps of block words + the XCC ids
  int* err;
  int bpi;
  int b0;                     // first instance of this launch
  int nb;                     // instances in this launch
  int xcd_group;              // workgroups dealt to XCD groups (grid.hip)
  unsigned salt;
  int n_resident;             // workgroups that must run at once (coresident(), cluster.h)
  unsigned long long gather_ticks;  // exchange timeout (kGatherTicks unless a test shortens it)
};

template <int SPT, int KMAX>
__global__ void __launch_bounds__(kGridThreads) ext_grid_kernel(ExtArgs a, ExtGridArgs g) {
  const Model& m = a.m;
  const int S = m.S, Kr = m.K;
  // XCD grouping (grid.hip): the workgroups of instance g + 8 j all come from
  // XCD group g; the grid is padded to 8 equal groups, padding leaves at once
  int lin = blockIdx.x;
  if (g.xcd_group) {
    const int grp = blockIdx.x % 8, kk = blockIdx.x / 8;
    const int il = grp + 8 * (kk / g.bpi);
    if (il >= g.nb) return;
    lin = il * g.bpi + kk % g.bpi;
  }
  const int il = lin / g.bpi, blk = lin % g.bpi, tid = threadIdx.x;
  const int b = g.b0 + il;
  __shared__ unsigned long long red_in[kGridThreads / kWave];
  __shared__ int lflag, resident;
  // every workgroup of the launch running at once, or none goes on (err[1..2];
  // err bit kErrNotResident tells the host to rerun per sweep)
  if (tid == 0) {
    lflag = 0;
    resident = coresident(g.err + 1, g.n_resident) ? 1 : 0;
  }
  __syncthreads();
  if (!resident) {
    if (tid == 0) atomicOr(g.err, kErrNotResident);
    return;
  }
  constexpr int K = KMAX;
  if (a.bad[b]) {  // bwd_nonfinite_rule: non-finite weights, NaN everywhere (uniform over the instance)
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      const int s = (blk * SPT + j) * kGridThreads + tid;
      if (s < S)
        for (int act = 0; act < m.A; ++act) a.pi[((size_t)b * S + s) * m.A + act] = kNaN;
    }
    if (blk == 0 && tid == 0) a.status[b] = IRLMX_OK;
    return;
  }
  int sidx[SPT];
  bool ok[SPT];
  int nb[SPT][K];
  double w[SPT][K];
  double cm[SPT];
  int ce[SPT];
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    const int s = (blk * SPT + j) * kGridThreads + tid;
    sidx[j] = s;
    ok[j] = s < S;
    const int ss = ok[j] ? s : 0;
    ext_init_state(a.term[(size_t)b * S + ss] != 0, &cm[j], &ce[j]);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      nb[j][k] = k < Kr ? row_nbr(m, b, ss, k) : ss;
      w[j][k] = k < Kr ? a.w[((size_t)b * Kr + k) * S + ss] : 0.0;  // padding slots: weight 0, skipped
    }
  }
  const Gran rg = gran_rsrc(g.gran + (size_t)il * 12 * S, 96u * (unsigned)S);
  const Gran rd = gran_rsrc(g.dgran + (size_t)il * 8 * g.bpi, 64u * (unsigned)g.bpi);
  const unsigned salt = (g.salt & 0xFFFu) << 20;
  // hand-off store form (grid.hip): write-through (sc1) in general, plain stores
  // when every workgroup of the instance runs on the same XCD -- found by
  // exchanging XCC ids once
  bool plain = false;
  {
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcc &= 0xFu;
    const unsigned htag = salt | 0xFFFFFu;
    if (tid == 0) gran_store(rd, (3u * (unsigned)g.bpi + (unsigned)blk) * 16u, xcc, htag, false);
    unsigned off[1] = {(3u * (unsigned)g.bpi + (unsigned)tid) * 16u};
    unsigned long long v[1] = {xcc};
    if (!gran_gather<1>(rd, rd, off, tid < g.bpi ? 1u : 0u, htag, v, g.gather_ticks)) lflag = 1;
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
  }
  // a pair's two granules: mantissa at 32 * index, exponent 16 bytes on
  auto publish = [&](unsigned slot, unsigned tag) {
#pragma unroll
    for (int j = 0; j < SPT; ++j)
      if (ok[j]) {
        const unsigned o = (slot * (unsigned)S + (unsigned)sidx[j]) * 32u;
        gran_store(rg, o, dbits(cm[j]), tag, plain);
        gran_store(rg, o + 16u, (unsigned long long)(unsigned)ce[j], tag, plain);
      }
    if (tid == 0) gran_store(rd, (slot * (unsigned)g.bpi + (unsigned)blk) * 16u, 0ull, tag, plain);
  };
  // sweep 0: the start vector; tag of sweep k: salt | (k + 1), never 0 (a zeroed workspace)
  publish(0u, salt | 1u);
  const long long total = 2LL * S - 1;  // collapsed sweeps (maxent.py:154); the last of the 2*S is per action
  double zm[SPT][K];  // the neighbours' pairs of the vector the next sweep reads
  int ze[SPT][K];
  for (long long k = 0;; ++k) {
    {
      constexpr int N = 2 * SPT * K + 1;
      const unsigned tag = salt | ((unsigned)(k + 1) & 0xFFFFFu);
      const unsigned slot = (unsigned)(k % 3);
      unsigned off[N];
      using mask_t = typename std::conditional<(N > 32), unsigned long long, unsigned>::type;
      mask_t want = 0;
#pragma unroll
      for (int j = 0; j < SPT; ++j)
#pragma unroll
        for (int kk = 0; kk < K; ++kk) {
          const int i = 2 * (j * K + kk);
          off[i] = (slot * (unsigned)S + (unsigned)nb[j][kk]) * 32u;
          off[i + 1] = off[i] + 16u;
          want |= (mask_t)(ok[j] && kk < Kr ? 3u : 0u) << i;
        }
      off[N - 1] = (slot * (unsigned)g.bpi + (unsigned)tid) * 16u;
      want |= (mask_t)(tid < g.bpi ? 1u : 0u) << (N - 1);
      unsigned long long v[N];
      if (!gran_gather<N>(rg, rd, off, want, tag, v, g.gather_ticks)) lflag = 1;
#pragma unroll
      for (int j = 0; j < SPT; ++j)
#pragma unroll
        for (int kk = 0; kk < K; ++kk) {
          const int i = 2 * (j * K + kk);
          const bool live = ok[j] && kk < Kr;
          zm[j][kk] = live ? bits_double(v[i]) : 0.0;
          ze[j][kk] = live ? (int)(unsigned)v[i + 1] : kExtZero;
        }
      __syncthreads();  // this workgroup has read sweep k: its next block word says so
      if (lflag) {
        if (tid == 0) atomicOr(g.err, 1);
        return;
      }
    }
    if (k >= total) break;  // neighbours of z_{2S-1} gathered: the per-action sweep
    // sweep k + 1 (ext_sweep_kernel's statements)
#pragma unroll
    for (int j = 0; j < SPT; ++j) {
      int E = kExtZero;
#pragma unroll
      for (int kk = 0; kk < K; ++kk)
        if (kk < Kr && w[j][kk] != 0.0) E = max(E, ze[j][kk]);
      double acc = 0.0;
#pragma unroll
      for (int kk = 0; kk < K; ++kk)
        if (kk < Kr) acc = fma(w[j][kk], ext_aligned(zm[j][kk], ze[j][kk], E), acc);
      ext_split(acc, E, &cm[j], &ce[j]);
    }
    publish((unsigned)((k + 1) % 3), salt | ((unsigned)(k + 2) & 0xFFFFFu));
  }
  // the last of the 2*S sweeps, per action (ext_policy_row's arithmetic on the gathered pairs)
  const int A = m.A;
#pragma unroll
  for (int j = 0; j < SPT; ++j) {
    if (!ok[j]) continue;
    const int s = sidx[j];
    double* out = a.pi + ((size_t)b * S + s) * A;
    int E = kExtZero;
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
      if (kk >= Kr) continue;
      bool any = false;
      for (int act = 0; act < A; ++act) any |= row_val(m, b, act, kk, s) != 0.0;
      if (any) E = max(E, ze[j][kk]);
    }
    const double er = exp(a.reward[(size_t)b * S + s]);
    double za[kMaxActions];
    double zsum = 0.0;
    for (int act = 0; act < A; ++act) {
      double acc = 0.0;
#pragma unroll
      for (int kk = 0; kk < K; ++kk)
        if (kk < Kr) acc = fma(row_val(m, b, act, kk, s), ext_aligned(zm[j][kk], ze[j][kk], E), acc);
      za[act] = __dmul_rn(er, acc);  // rounded product, then the sum (maxent.py:155-156)
      zsum = __dadd_rn(zsum, za[act]);
    }
    for (int act = 0; act < A; ++act) out[act] = za[act] / zsum;
  }
  if (blk == 0 && tid == 0) a.status[b] = IRLMX_OK;
}

// (SPT, KMAX) pairs whose gather, 2 * SPT * KMAX + 1 entries, fits gran_gather's
// 64-bit mask -- the list of the Bellman grid kernels (grid.hip); <2, 16> and
// <1, 32> stay on the per-sweep shape.  No pair spills VGPRs
// (tools/kernel_resources.py).
constexpr bool ext_grid_pair_ok(int spt, int kmax) { return 2 * spt * kmax + 1 <= 64; }

void* ext_grid_fn(int spt, int kmax) {
  return with_pair<void*>(spt, kmax, [](auto s, auto k) {
    if constexpr (ext_grid_pair_ok(s, k)) return (void*)&ext_grid_kernel<s, k>;
    else return nullptr;
  });
}

static std::atomic<unsigned> g_ext_grid_salt{1};

int ext_grid_run(const Model& m, const ExtGridPlan& gp, const ExtArgs& a, const ExtGridWs& ws, hipStream_t st) {
  void* fn = ext_grid_fn(gp.spt, gp.kmax);
  if (!fn) { set_error("no extended grid kernel for spt=%d kmax=%d", gp.spt, gp.kmax); return IRLMX_EINVAL; }
  const LaunchTestKnobs tk = launch_test_knobs();  // tests only (cluster.h)
  ExtArgs ka = a;
  for (int b0 = 0; b0 < m.B; b0 += gp.ipl) {
    const int nb = std::min(gp.ipl, m.B - b0);
    // zeroed granules, block words and err words for every launch
    hipError_t e = hipMemsetAsync(ws.gran, 0, (size_t)nb * 6 * m.S * 16, st);
    if (e == hipSuccess) e = hipMemsetAsync(ws.dgran, 0, (size_t)nb * 4 * gp.bpi * 16, st);
    if (e == hipSuccess) e = hipMemsetAsync(ws.err, 0, 4 * sizeof(int), st);
    if (e != hipSuccess) return hip_fail(e, "extended grid workspace memset");
    const int xcd = gp.xcd && nb >= 8;
    ExtGridArgs ga{ws.gran, ws.dgran, ws.err, gp.bpi, b0, nb, xcd,
                   g_ext_grid_salt.fetch_add(1, std::memory_order_relaxed), gp.bpi * nb + tk.extra_resident,
                   tk.gather_ticks};
    void* args[] = {&ka, &ga};
    const int grid = xcd ? 8 * ((nb + 7) / 8) * gp.bpi : gp.bpi * nb;
    e = hipLaunchKernel(fn, dim3(grid), dim3(kGridThreads), args, 0, st);
    if (e != hipSuccess) return hip_fail(e, "extended grid launch");
    count_event(IRLMX_CTR_GRID_LAUNCHES);
    if (const int rc = grid_launch_outcome(ws.err, "extended grid", st)) return rc;
  }
  return 0;
}

}  // namespace irlmx

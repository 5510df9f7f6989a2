// Host-side sanitizer driver ("Race detection / sanitizers").
//
// Built by tools/sanitize/Makefile: every irl-maxent_amd/csrc/*.hip source is
// compiled with its host code instrumented by AddressSanitizer +
// UndefinedBehaviorSanitizer (device code as usual: no GPU sanitizer) and linked
// with this driver.  It runs without a GPU: the planner is told the device shape
// through its test overrides (IRLMX_PLAN_CUS = 256 CUs, IRLMX_PLAN_GRID_PER_CU),
// and no call below gets past argument validation and planning, so nothing is
// ever enqueued.  What it exercises under the sanitizers:
//
//  * the tile planner (cluster.hip cluster_plan: R / G / C / states per lane /
//    LDS budget), the grid planner (grid.hip grid_plan), the choice of shape
//    (fixed_point.hip route) and the workspace carving it sizes
//    (fixed_point.hip carve) for widths 5..256, rectangular grids,
//    batches 1..256, all four ops, stencil / ELL / DENSE layouts -- through the
//    C ABI's irlmx_execution_plan and irlmx_workspace_bytes, with invariants
//    checked on every plan;
//  * every argument-validation path of every entry point (null models, bad
//    sizes, unknown layouts, NULL arrays, short workspaces), with the error text;
//  * the extended-range backward (extended.hip): its plan and workspace
//    (IRLMX_PLAN_EXTENDED_RANGE) for every stencil and ELL model above --
//    fused, the persistent grid shape (extended_grid.hip) or per sweep --, the
//    flag's refusal on the other ops and on DENSE tables, and the validation
//    and workspace paths of irlmx_backward_maxent_extended;
//  * policy evaluation (policy_eval.hip): the plan and workspace of
//    IRLMX_OP_POLICY_EVALUATION for every stencil and ELL model above (fused or
//    per sweep, never a persistent shape), its refusal of DENSE tables and of
//    the backward-only flags, and every validation path of
//    irlmx_policy_evaluation (NULL arrays, discount outside [0, 1] or NaN,
//    short workspace);
//  * the finite-horizon passes (horizon.hip): the plan and workspace of
//    IRLMX_OP_BACKWARD_HORIZON and IRLMX_OP_FORWARD_HORIZON for every stencil
//    and ELL model above (fused or per sweep), their refusal of DENSE tables
//    and of the backward-only flags, and every validation path of
//    irlmx_backward_maxent_horizon and irlmx_forward_svf_horizon (NULL arrays,
//    the optional ones, a horizon outside [1, 2^20], short workspace);
//  * the finite-horizon soft value iteration (soft_horizon.hip): every
//    validation path of irlmx_soft_backward_horizon (NULL arrays, the optional
//    ones, a discount outside [0, 1] or NaN, a horizon outside [1, 2^20], DENSE
//    tables, short workspace) and the plan and workspace of
//    IRLMX_OP_SOFT_BACKWARD_HORIZON on a fused and a per-sweep model;
//  * the demonstration calls (rollout.hip): every validation path of
//    irlmx_rollout (NULL arrays, n_traj, max_len below 1 and above its cap,
//    states without actions, DENSE tables), irlmx_demo_statistics and
//    irlmx_demo_log_likelihood (sizes, stride, NULL arrays);
//  * the calls on time-indexed policies (include/irlmx_timed.h; the value pass
//    in soft_horizon.hip, the two trajectory calls in rollout.hip): the
//    plan and workspace of IRLMX_OP_VALUE_HORIZON for every stencil and ELL
//    model above -- the soft horizon pass's, with 16 * S bytes of LDS when
//    fused -- and every validation path of irlmx_value_horizon,
//    irlmx_rollout_horizon and irlmx_demo_log_likelihood_horizon;
//  * the one-call expected SVF (expected_svf_horizon.hip,
//    include/irlmx_expected_svf.h): irlmx_expected_svf_horizon_workspace_bytes
//    and irlmx_expected_svf_horizon_plan for every model above, both models,
//    horizons 1 .. 2^20 and the segment lengths 0, 1, 3, T and T + 5 -- the
//    resolved segment, the slices, the shape and the header's memory bound --
//    and every validation path of irlmx_expected_svf_horizon.
//
// Exit status 0 and "host_check ok" on success.
//
// host_check --dump checks nothing: it prints the plan and the workspace size of
// every model and op of that sweep (dump_plans), to compare two builds of the
// library -- before and after a change to the planners -- byte for byte.

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/irlmx.h"
#include "../../include/irlmx_expected_svf.h"
#include "../../include/irlmx_timed.h"

static int g_fail = 0;
static long long g_checks = 0;

#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    ++g_checks;                                                           \
    if (!(cond)) {                                                        \
      if (g_fail < 50) {                                                  \
        fprintf(stderr, "FAIL %s:%d (%s): ", __FILE__, __LINE__, #cond);  \
        fprintf(stderr, __VA_ARGS__);                                     \
        fputc('\n', stderr);                                              \
      }                                                                   \
      ++g_fail;                                                           \
    }                                                                     \
  } while (0)

// Never dereferenced by the host code under test: it only checks pointers for NULL.
static double g_fake[16];
static void* fake() { return (void*)g_fake; }

static irlmx_mdp stencil(int w, int h, int a, int b, int shared) {
  irlmx_mdp m;
  memset(&m, 0, sizeof(m));
  m.layout = IRLMX_LAYOUT_STENCIL5;
  m.n_states = w * h;
  m.n_actions = a;
  m.width = w;
  m.height = h;
  m.k_row = m.k_col = 5;
  m.batch = b;
  m.shared = shared;
  m.row_val = g_fake;
  return m;
}

static irlmx_mdp ell(int s, int a, int k_row, int k_col, int b) {
  irlmx_mdp m;
  memset(&m, 0, sizeof(m));
  m.layout = IRLMX_LAYOUT_ELL;
  m.n_states = s;
  m.n_actions = a;
  m.k_row = k_row;
  m.k_col = k_col;
  m.batch = b;
  m.shared = 1;
  m.row_val = g_fake;
  m.row_idx = (const int32_t*)g_fake;
  m.col_idx = (const int32_t*)g_fake;
  m.col_val = g_fake;
  return m;
}

static irlmx_mdp dense(int s, int a, int b) {
  irlmx_mdp m = ell(s, a, s, s, b);
  m.layout = IRLMX_LAYOUT_DENSE;
  return m;
}

static const int kCus = 256;
static long long g_shapes[7];

// Invariants of one plan (include/irlmx.h, IRLMX_PLAN_LEN fields).
static void check_plan(const irlmx_mdp& m, int op, const int64_t* p, const char* what) {
  const int64_t shape = p[0];
  CHECK(shape >= IRLMX_SHAPE_FUSED && shape <= IRLMX_SHAPE_DENSE_GRID, "%s: shape %lld", what, (long long)shape);
  if (shape == IRLMX_SHAPE_FUSED) {
    CHECK(p[7] >= 64 && p[7] <= 1024 && p[7] % 64 == 0, "%s: fused threads %lld", what, (long long)p[7]);
    CHECK(p[5] * p[7] >= m.n_states, "%s: fused spt %lld x %lld < S %d", what, (long long)p[5], (long long)p[7],
          m.n_states);
    CHECK(p[9] <= 160 * 1024, "%s: fused LDS %lld", what, (long long)p[9]);
  } else if (shape == IRLMX_SHAPE_CLUSTER) {
    const int64_t R = p[1], G = p[2], C = p[3], per = p[4], spt = p[5], lay = p[6], nt = p[7], nl = p[8];
    const int H = m.height, W = m.width;
    CHECK(m.layout == IRLMX_LAYOUT_STENCIL5 && (op == IRLMX_OP_BACKWARD || op == IRLMX_OP_FORWARD), "%s", what);
    CHECK(R >= 1 && R <= H && G >= 1 && G <= 16, "%s: R %lld G %lld", what, (long long)R, (long long)G);
    CHECK(C == (H + R - 1) / R, "%s: C %lld for H %d R %lld", what, (long long)C, H, (long long)R);
    CHECK(per >= 1 && per * C <= kCus && per <= m.batch, "%s: per_launch %lld x C %lld", what, (long long)per,
          (long long)C);
    CHECK(nl == (m.batch + per - 1) / per, "%s: launches %lld", what, (long long)nl);
    const int64_t ext = (R + 2 * G < H ? R + 2 * G : H);
    CHECK(spt * nt >= ext * W, "%s: %lld slots < extended tile %lld", what, (long long)(spt * nt),
          (long long)(ext * W));
    CHECK(nt == 512 || nt == 1024, "%s: threads %lld", what, (long long)nt);
    CHECK(lay >= 0 && lay <= 3 && (lay == 0 || W == 64 || W == 128 || W == 256), "%s: layout %lld", what,
          (long long)lay);
    CHECK(p[9] > 0 && p[9] <= 160 * 1024, "%s: LDS %lld", what, (long long)p[9]);
  } else if (shape == IRLMX_SHAPE_GRID) {
    CHECK(p[3] >= 1 && p[4] == m.batch && p[7] == 256, "%s: grid bpi %lld", what, (long long)p[3]);
    CHECK(p[5] * p[7] * p[3] >= m.n_states, "%s: grid covers %lld < S", what, (long long)(p[5] * p[7] * p[3]));
  } else if (shape == IRLMX_SHAPE_DENSE || shape == IRLMX_SHAPE_DENSE_GEMM) {
    CHECK(m.layout == IRLMX_LAYOUT_DENSE, "%s: dense shape for layout %d", what, m.layout);
  } else if (shape == IRLMX_SHAPE_DENSE_GRID) {
    const int64_t rb = p[1], bpi = p[3], cpt = p[5], at = p[6];
    const bool bellman = op == IRLMX_OP_SOFT_BACKWARD || op == IRLMX_OP_VALUE_ITERATION;
    CHECK(m.layout == IRLMX_LAYOUT_DENSE, "%s", what);
    CHECK(p[7] == 512 && p[4] == m.batch && p[8] == 1, "%s: dense grid threads %lld", what, (long long)p[7]);
    CHECK(bellman ? (at >= m.n_actions && (at == 4 || at == 8)) : at == 0, "%s: dense grid actions %lld", what,
          (long long)at);
    CHECK(rb >= (bellman ? 2 : 4) && rb <= 64 && rb * cpt * (bellman ? at : 1) <= 64,
          "%s: dense grid rb %lld cpt %lld", what, (long long)rb, (long long)cpt);
    CHECK(cpt * 512 >= m.n_states && bpi == (m.n_states + rb - 1) / rb, "%s: dense grid covers", what);
    CHECK(bpi * m.batch <= kCus, "%s: dense grid %lld x %d workgroups", what, (long long)bpi, m.batch);
  }
}

static long long g_ext_shapes[3];

// The extended-range backward's plan and workspace for one model
// (IRLMX_OP_BACKWARD | IRLMX_PLAN_EXTENDED_RANGE), and the flag on the other ops.
static void extended_plan_and_workspace(const irlmx_mdp& m, const char* what) {
  const int op = IRLMX_OP_BACKWARD | IRLMX_PLAN_EXTENDED_RANGE;
  int64_t p[IRLMX_PLAN_LEN];
  for (auto& v : p) v = -7;
  const int rc = irlmx_execution_plan(&m, op, p);
  const size_t ws = irlmx_workspace_bytes(&m, op);
  if (m.layout == IRLMX_LAYOUT_DENSE) {
    CHECK(rc == IRLMX_EINVAL && strstr(irlmx_last_error(), "DENSE"), "%s: extended plan of a DENSE table rc %d", what, rc);
    CHECK(ws == 0, "%s: extended workspace of a DENSE table %zu", what, ws);
    return;
  }
  CHECK(rc == 0, "%s: extended plan rc %d (%s)", what, rc, irlmx_last_error());
  if (rc) return;
  const size_t S = (size_t)m.n_states, B = (size_t)m.batch;
  const size_t K = m.layout == IRLMX_LAYOUT_STENCIL5 ? 5 : (size_t)m.k_row;
  size_t floor = B * K * S * sizeof(double) + B * sizeof(int32_t);
  CHECK(p[0] == IRLMX_SHAPE_FUSED || p[0] == IRLMX_SHAPE_SWEEP || p[0] == IRLMX_SHAPE_GRID, "%s: extended shape %lld",
        what, (long long)p[0]);
  CHECK(p[1] == 0 && p[6] == 0, "%s: extended plan cluster fields", what);
  CHECK(p[0] == IRLMX_SHAPE_GRID || (p[2] == 0 && p[3] == 0 && p[4] == 0), "%s: extended plan grid fields", what);
  size_t slack = 8 * 256;
  if (p[0] == IRLMX_SHAPE_GRID) {
    // the persistent grid shape (extended_grid.hip): from 8,192 states on, up to 16 slots, workgroups of 256
    // threads, [3] of them per instance, [4] instances per launch within the planned capacity, [8] launches
    ++g_ext_shapes[1];
    const int64_t xcd = p[2], bpi = p[3], ipl = p[4], spt = p[5], nl = p[8];
    CHECK(S >= 8192 && S <= (size_t(1) << 18) && K <= 16, "%s: extended grid at S %zu K %zu", what, S, K);
    CHECK(((spt == 1 && K <= 16) || (spt == 2 && K <= 8) || (spt == 4 && K <= 5)) && p[7] == 256 && p[9] == 0, "%s: extended grid spt %lld",
          what, (long long)spt);
    CHECK(bpi == ((int64_t)S + 256 * spt - 1) / (256 * spt) && bpi <= 256, "%s: extended grid bpi %lld", what,
          (long long)bpi);
    CHECK(ipl >= 1 && ipl <= (int64_t)B && ipl * bpi <= 4 * kCus, "%s: extended grid %lld instances x %lld", what,
          (long long)ipl, (long long)bpi);
    CHECK(xcd == 0 || (xcd == 1 && B >= 8 && (ipl + 7) / 8 * bpi <= 4 * kCus / 8), "%s: extended grid xcd %lld", what,
          (long long)xcd);
    CHECK(xcd == 1 || ipl == 1 || ipl * bpi <= 2 * kCus, "%s: extended grid, ungrouped: %lld instances x %lld", what,
          (long long)ipl, (long long)bpi);
    CHECK(nl == ((int64_t)B + ipl - 1) / ipl && nl >= 1, "%s: extended grid launches %lld", what, (long long)nl);
    // the per-sweep buffers (the rerun's), one launch's granules and block words, the err words
    floor += B * S * 2 * (sizeof(double) + sizeof(int32_t)) + (size_t)ipl * (96 * S + 64 * (size_t)bpi) + 16;
    slack += 3 * 256;
  } else if (p[0] == IRLMX_SHAPE_FUSED) {
    ++g_ext_shapes[0];
    CHECK(S <= 4096 && K <= 32, "%s: extended fused at S %zu K %zu", what, S, K);
    CHECK(p[7] >= 64 && p[7] <= 1024 && p[7] % 64 == 0, "%s: extended fused threads %lld", what, (long long)p[7]);
    CHECK(p[5] >= 1 && p[5] <= 4 && p[5] * p[7] >= (int64_t)S, "%s: extended fused spt %lld", what, (long long)p[5]);
    CHECK(p[8] == 1 && p[9] == (int64_t)(24 * S) && p[9] <= 160 * 1024, "%s: extended fused LDS %lld", what,
          (long long)p[9]);
  } else {
    ++g_ext_shapes[2];
    CHECK(p[5] == 1 && p[7] == 256 && p[8] == 2 * (int64_t)S - 1 && p[9] == 0, "%s: extended sweep plan", what);
    floor += B * S * 2 * (sizeof(double) + sizeof(int32_t));
  }
  CHECK(ws >= floor && ws <= floor + slack && ws % 256 == 0, "%s: extended workspace %zu (floor %zu)", what, ws, floor);
  for (int other = IRLMX_OP_FORWARD; other <= IRLMX_OP_VALUE_ITERATION; ++other) {
    CHECK(irlmx_execution_plan(&m, other | IRLMX_PLAN_EXTENDED_RANGE, p) == IRLMX_EINVAL &&
              strstr(irlmx_last_error(), "IRLMX_OP_BACKWARD only"),
          "%s: extended flag on op %d", what, other);
    CHECK(irlmx_workspace_bytes(&m, other | IRLMX_PLAN_EXTENDED_RANGE) == 0, "%s: extended workspace of op %d", what,
          other);
  }
  CHECK(irlmx_execution_plan(&m, op | IRLMX_PLAN_NO_RESCALE, p) == IRLMX_EINVAL, "%s: extended + no-rescale", what);
}

static long long g_pe_shapes[3];

// Policy evaluation's plan and workspace for one model (IRLMX_OP_POLICY_EVALUATION):
// fused or per sweep, never a persistent shape; refused on DENSE tables.
static void policy_eval_plan_and_workspace(const irlmx_mdp& m, const char* what) {
  const int op = IRLMX_OP_POLICY_EVALUATION;
  int64_t p[IRLMX_PLAN_LEN];
  for (auto& v : p) v = -7;
  const int rc = irlmx_execution_plan(&m, op, p);
  const size_t ws = irlmx_workspace_bytes(&m, op);
  if (m.layout == IRLMX_LAYOUT_DENSE) {
    CHECK(rc == IRLMX_EINVAL && strstr(irlmx_last_error(), "DENSE"), "%s: policy evaluation plan of a DENSE table rc %d",
          what, rc);
    CHECK(ws == 0, "%s: policy evaluation workspace of a DENSE table %zu", what, ws);
    return;
  }
  CHECK(rc == 0, "%s: policy evaluation plan rc %d (%s)", what, rc, irlmx_last_error());
  if (rc) return;
  const size_t S = (size_t)m.n_states, B = (size_t)m.batch;
  const size_t K = m.layout == IRLMX_LAYOUT_STENCIL5 ? 5 : (size_t)m.k_row;
  size_t floor = B * K * S * sizeof(double) + B * (3 * sizeof(uint64_t) + sizeof(int32_t) + sizeof(int64_t));
  CHECK(p[0] == IRLMX_SHAPE_FUSED || p[0] == IRLMX_SHAPE_SWEEP, "%s: policy evaluation shape %lld", what, (long long)p[0]);
  CHECK(p[1] == 0 && p[2] == 0 && p[3] == 0 && p[4] == 0 && p[6] == 0, "%s: policy evaluation plan cluster fields", what);
  if (p[0] == IRLMX_SHAPE_FUSED) {
    ++g_pe_shapes[0];
    CHECK(S <= 4096 && K <= 32, "%s: policy evaluation fused at S %zu K %zu", what, S, K);
    CHECK(p[7] >= 64 && p[7] <= 1024 && p[7] % 64 == 0, "%s: policy evaluation fused threads %lld", what, (long long)p[7]);
    CHECK(p[5] >= 1 && p[5] <= 4 && p[5] * p[7] >= (int64_t)S, "%s: policy evaluation fused spt %lld", what, (long long)p[5]);
    CHECK(p[8] == 1 && p[9] == (int64_t)(24 * S + 32) && p[9] <= 160 * 1024, "%s: policy evaluation fused LDS %lld", what,
          (long long)p[9]);
  } else {
    ++g_pe_shapes[2];
    CHECK(p[5] == 1 && p[7] == 256 && p[8] == 0 && p[9] == 0, "%s: policy evaluation sweep plan", what);
    floor += B * S * 2 * sizeof(double);
  }
  CHECK(ws >= floor && ws <= floor + 16 * 256 && ws % 256 == 0, "%s: policy evaluation workspace %zu (floor %zu)", what, ws,
        floor);
  CHECK(irlmx_execution_plan(&m, op | IRLMX_PLAN_EXTENDED_RANGE, p) == IRLMX_EINVAL &&
            strstr(irlmx_last_error(), "IRLMX_OP_BACKWARD only"),
        "%s: extended flag on policy evaluation", what);
  CHECK(irlmx_workspace_bytes(&m, op | IRLMX_PLAN_EXTENDED_RANGE) == 0, "%s: extended workspace of policy evaluation", what);
  CHECK(irlmx_execution_plan(&m, op | IRLMX_PLAN_NO_RESCALE, p) == IRLMX_EINVAL && strstr(irlmx_last_error(), "NO_RESCALE"),
        "%s: no-rescale flag on policy evaluation", what);
}

static long long g_hz_shapes[3];

// The finite-horizon passes' plan and workspace for one model
// (IRLMX_OP_BACKWARD_HORIZON, IRLMX_OP_FORWARD_HORIZON): fused or per sweep,
// never a persistent shape; refused on DENSE tables.
static void horizon_plan_and_workspace(const irlmx_mdp& m, const char* what) {
  for (int op : {IRLMX_OP_BACKWARD_HORIZON, IRLMX_OP_FORWARD_HORIZON}) {
    const bool bwd = op == IRLMX_OP_BACKWARD_HORIZON;
    int64_t p[IRLMX_PLAN_LEN];
    for (auto& v : p) v = -7;
    const int rc = irlmx_execution_plan(&m, op, p);
    const size_t ws = irlmx_workspace_bytes(&m, op);
    if (m.layout == IRLMX_LAYOUT_DENSE) {
      CHECK(rc == IRLMX_EINVAL && strstr(irlmx_last_error(), "DENSE"), "%s: horizon plan %d of a DENSE table rc %d", what, op,
            rc);
      CHECK(ws == 0, "%s: horizon workspace %d of a DENSE table %zu", what, op, ws);
      continue;
    }
    CHECK(rc == 0, "%s: horizon plan %d rc %d (%s)", what, op, rc, irlmx_last_error());
    if (rc) continue;
    const size_t S = (size_t)m.n_states, B = (size_t)m.batch;
    const size_t K = m.layout == IRLMX_LAYOUT_STENCIL5 ? 5 : (size_t)(bwd ? m.k_row : m.k_col);
    CHECK(p[0] == IRLMX_SHAPE_FUSED || p[0] == IRLMX_SHAPE_SWEEP, "%s: horizon shape %lld", what, (long long)p[0]);
    CHECK(p[1] == 0 && p[2] == 0 && p[3] == 0 && p[4] == 0 && p[6] == 0, "%s: horizon plan cluster fields", what);
    if (p[0] == IRLMX_SHAPE_FUSED) {
      ++g_hz_shapes[0];
      CHECK(S <= 4096 && K <= 32, "%s: horizon fused at S %zu K %zu", what, S, K);
      CHECK(p[7] >= 64 && p[7] <= 1024 && p[7] % 64 == 0, "%s: horizon fused threads %lld", what, (long long)p[7]);
      CHECK(p[5] >= 1 && p[5] <= 4 && p[5] * p[7] >= (int64_t)S, "%s: horizon fused spt %lld", what, (long long)p[5]);
      CHECK(p[8] == 1 && p[9] == (int64_t)((bwd ? 24 : 16) * S) && p[9] <= 160 * 1024, "%s: horizon fused LDS %lld", what,
            (long long)p[9]);
      CHECK(ws == 0, "%s: horizon fused workspace %zu", what, ws);
    } else {
      ++g_hz_shapes[2];
      CHECK(p[5] == 1 && p[7] == 256 && p[8] == 0 && p[9] == 0, "%s: horizon sweep plan", what);
      const size_t floor = B * S * (bwd ? 24 : 16);
      CHECK(ws >= floor && ws <= floor + 8 * 256 && ws % 256 == 0, "%s: horizon workspace %zu (floor %zu)", what, ws, floor);
    }
    CHECK(irlmx_execution_plan(&m, op | IRLMX_PLAN_EXTENDED_RANGE, p) == IRLMX_EINVAL &&
              strstr(irlmx_last_error(), "IRLMX_OP_BACKWARD only"),
          "%s: extended flag on a horizon op", what);
    CHECK(irlmx_workspace_bytes(&m, op | IRLMX_PLAN_EXTENDED_RANGE) == 0, "%s: extended workspace of a horizon op", what);
    CHECK(irlmx_execution_plan(&m, op | IRLMX_PLAN_NO_RESCALE, p) == IRLMX_EINVAL && strstr(irlmx_last_error(), "NO_RESCALE"),
          "%s: no-rescale flag on a horizon op", what);
  }
}

// IRLMX_OP_VALUE_HORIZON answers as IRLMX_OP_SOFT_BACKWARD_HORIZON does, except for the fused kernel's LDS.
static void value_horizon_plan_and_workspace(const irlmx_mdp& m, const char* what) {
  const int op = IRLMX_OP_VALUE_HORIZON;
  int64_t p[IRLMX_PLAN_LEN], q[IRLMX_PLAN_LEN];
  for (auto& v : p) v = -7;
  for (auto& v : q) v = -7;
  const int rc = irlmx_execution_plan(&m, op, p);
  const size_t ws = irlmx_workspace_bytes(&m, op);
  const int rq = irlmx_execution_plan(&m, IRLMX_OP_SOFT_BACKWARD_HORIZON, q);
  CHECK(rc == rq && ws == irlmx_workspace_bytes(&m, IRLMX_OP_SOFT_BACKWARD_HORIZON), "%s: value horizon rc %d / %d, workspace %zu",
        what, rc, rq, ws);
  if (m.layout == IRLMX_LAYOUT_DENSE) {
    CHECK(rc == IRLMX_EINVAL && strstr(irlmx_last_error(), "DENSE") && ws == 0, "%s: value horizon plan of a DENSE table rc %d", what, rc);
    return;
  }
  CHECK(rc == 0, "%s: value horizon plan rc %d (%s)", what, rc, irlmx_last_error());
  if (rc) return;
  const size_t S = (size_t)m.n_states, B = (size_t)m.batch;
  for (int i = 0; i < 9; ++i) CHECK(p[i] == q[i], "%s: value horizon plan[%d] %lld, the soft pass's %lld", what, i, (long long)p[i], (long long)q[i]);
  if (p[0] == IRLMX_SHAPE_FUSED) {
    CHECK(p[9] == (int64_t)(16 * S) && q[9] == p[9] + 1536 && p[8] == 1 && ws == 0, "%s: value horizon fused LDS %lld workspace %zu", what,
          (long long)p[9], ws);
    CHECK(p[5] >= 1 && p[5] <= 4 && p[5] * p[7] >= (int64_t)S && p[7] % 64 == 0 && p[7] <= 1024, "%s: value horizon fused spt %lld threads %lld",
          what, (long long)p[5], (long long)p[7]);
  } else {
    CHECK(p[0] == IRLMX_SHAPE_SWEEP && p[5] == 1 && p[7] == 256 && p[8] == 0 && p[9] == 0, "%s: value horizon sweep plan", what);
    const size_t floor = B * S * 16;
    CHECK(ws >= floor && ws <= floor + 2 * 256 && ws % 256 == 0, "%s: value horizon workspace %zu (floor %zu)", what, ws, floor);
  }
  CHECK(irlmx_execution_plan(&m, op | IRLMX_PLAN_EXTENDED_RANGE, p) == IRLMX_EINVAL && strstr(irlmx_last_error(), "IRLMX_OP_BACKWARD only"),
        "%s: extended flag on the value horizon op", what);
  CHECK(irlmx_execution_plan(&m, op | IRLMX_PLAN_NO_RESCALE, p) == IRLMX_EINVAL && strstr(irlmx_last_error(), "NO_RESCALE"),
        "%s: no-rescale flag on the value horizon op", what);
}

// The one-call expected SVF's size and plan for one model (include/irlmx_expected_svf.h)
static long long g_esh_shapes[3];
static void expected_svf_plan_and_workspace(const irlmx_mdp& m, const char* what) {
  const size_t B = m.batch, S = m.n_states, A = m.n_actions;
  const bool dense = m.layout == IRLMX_LAYOUT_DENSE;
  const int64_t kc = m.layout == IRLMX_LAYOUT_STENCIL5 ? 5 : m.k_col;
  for (int model : {IRLMX_HORIZON_MODEL_MAXENT, IRLMX_HORIZON_MODEL_CAUSAL})
    for (int T : {1, 2, 40, 4096, 1 << 20})
      for (int seg : {0, 1, 3, T, T + 5}) {
        int64_t p[6];
        for (auto& v : p) v = -7;
        const int rc = irlmx_expected_svf_horizon_plan(&m, model, T, seg, p);
        const size_t ws = irlmx_expected_svf_horizon_workspace_bytes(&m, model, T, seg);
        if (dense) {
          CHECK(rc == IRLMX_EINVAL && strstr(irlmx_last_error(), "expected_svf_horizon: the finite-horizon passes do not run the DENSE") && ws == 0,
                "%s: expected svf plan of a DENSE table rc %d ws %zu", what, rc, ws);
          continue;
        }
        CHECK(rc == 0, "%s: expected svf plan rc %d (%s)", what, rc, irlmx_last_error());
        if (rc) continue;
        int64_t C = seg > T ? T : seg;
        if (seg == 0)
          for (C = 1; C * C < T; ++C) {}
        const int64_t nseg = (T + C - 1) / C;
        CHECK(p[1] == C && p[2] == nseg + C - 1 + (nseg > 1 ? 2 : 0), "%s: expected svf T %d segment %d: C %lld slices %lld", what, T,
              seg, (long long)p[1], (long long)p[2]);
        const size_t lds = (model == IRLMX_HORIZON_MODEL_CAUSAL ? 1536 : 0) + 8 * S * (A + 2);
        const bool fused = S <= 1024 && kc <= 32 && lds <= 160 * 1024;
        CHECK(p[0] == (fused ? IRLMX_SHAPE_FUSED : IRLMX_SHAPE_SWEEP) && p[3] == (fused ? 1 : 0) && p[4] == (fused ? (int64_t)lds : 0),
              "%s: expected svf shape %lld launches %lld LDS %lld", what, (long long)p[0], (long long)p[3], (long long)p[4]);
        CHECK(p[5] == (int64_t)ws && ws % 256 == 0 && ws >= (size_t)p[2] * B * S * (model == IRLMX_HORIZON_MODEL_MAXENT ? 12 : 8),
              "%s: expected svf workspace %zu, plan %lld", what, ws, (long long)p[5]);
        CHECK(ws <= (size_t)(nseg + C + (int64_t)A + 6) * B * S * 12 + 4096, "%s: expected svf workspace %zu above the bound (T %d C %lld)",
              what, ws, T, (long long)C);
        if (T == 40 && seg == 0) ++g_esh_shapes[p[0]];
      }
}

static void plan_and_workspace(const irlmx_mdp& m, const char* tag) {
  for (int op = IRLMX_OP_BACKWARD; op <= IRLMX_OP_VALUE_ITERATION; ++op) {
    char what[160];
    snprintf(what, sizeof(what), "%s op %d S %d B %d", tag, op, m.n_states, m.batch);
    int64_t plan[IRLMX_PLAN_LEN];
    for (auto& v : plan) v = -7;
    const int rc = irlmx_execution_plan(&m, op, plan);
    CHECK(rc == 0, "%s: plan rc %d (%s)", what, rc, irlmx_last_error());
    if (rc == 0) check_plan(m, op, plan, what);
    if (rc == 0 && plan[0] >= 0 && plan[0] < 7) ++g_shapes[plan[0]];
    if (op == IRLMX_OP_BACKWARD) {
      int64_t p2[IRLMX_PLAN_LEN];
      CHECK(irlmx_execution_plan(&m, op | IRLMX_PLAN_NO_RESCALE, p2) == 0, "%s: no-rescale plan", what);
      CHECK(p2[0] != IRLMX_SHAPE_CLUSTER, "%s: rescale=0 backward planned on the cluster shape", what);
      extended_plan_and_workspace(m, what);
      policy_eval_plan_and_workspace(m, what);
      horizon_plan_and_workspace(m, what);
      value_horizon_plan_and_workspace(m, what);
      expected_svf_plan_and_workspace(m, what);
    }
    const size_t ws = irlmx_workspace_bytes(&m, op);
    const size_t floor = (op == IRLMX_OP_BACKWARD || op == IRLMX_OP_FORWARD)
                             ? (size_t)m.batch * sizeof(int32_t)  // at least the per-instance flags
                             : 0;
    CHECK(ws >= floor && ws < (size_t(1) << 44), "%s: workspace %zu", what, ws);
    CHECK(ws % 256 == 0, "%s: workspace %zu not 256-aligned", what, ws);
  }
}

static int run_bwd(const irlmx_mdp* m, void* reward, void* term, void* pi, void* status, void* ws, size_t n) {
  return irlmx_backward_maxent(m, (const double*)reward, (const uint8_t*)term, 1, (double*)pi, (int32_t*)status, ws,
                               n, nullptr);
}

static int run_ext(const irlmx_mdp* m, void* reward, void* term, void* pi, void* status, void* ws, size_t n) {
  return irlmx_backward_maxent_extended(m, (const double*)reward, (const uint8_t*)term, (double*)pi, (int32_t*)status,
                                        ws, n, nullptr);
}

static int run_pe(const irlmx_mdp* m, void* reward, void* pi, void* term, double discount, void* value, void* iters,
                  void* status, void* ws, size_t n) {
  return irlmx_policy_evaluation(m, (const double*)reward, (const double*)pi, (const uint8_t*)term, discount, 1e-3, 0,
                                 (double*)value, (int64_t*)iters, (int32_t*)status, ws, n, nullptr);
}

static int run_hzb(const irlmx_mdp* m, void* reward, void* term, int horizon, void* pi, void* lz, void* status, void* ws,
                   size_t n) {
  return irlmx_backward_maxent_horizon(m, (const double*)reward, (const uint8_t*)term, horizon, (double*)pi, (double*)lz,
                                       (int32_t*)status, ws, n, nullptr);
}

static int run_hzf(const irlmx_mdp* m, void* p0, void* term, void* pi, int horizon, void* svf, void* svf_t, void* status,
                   void* ws, size_t n) {
  return irlmx_forward_svf_horizon(m, (const double*)p0, (const uint8_t*)term, (const double*)pi, horizon, (double*)svf,
                                   (double*)svf_t, (int32_t*)status, ws, n, nullptr);
}

static int run_shz(const irlmx_mdp* m, void* reward, void* term, double discount, int horizon, void* pi, void* v0,
                   void* status, void* ws, size_t n) {
  return irlmx_soft_backward_horizon(m, (const double*)reward, (const uint8_t*)term, discount, horizon, (double*)pi,
                                     (double*)v0, (int32_t*)status, ws, n, nullptr);
}

static int run_roll(const irlmx_mdp* m, int n_traj, int max_len, void* pi, void* term, void* start, void* seed,
                    void* visits, void* starts, void* lengths, void* status, void* states, void* actions) {
  return irlmx_rollout(m, (const double*)pi, (const uint8_t*)term, (const int32_t*)start, (const uint64_t*)seed, n_traj,
                       max_len, (int64_t*)visits, (int64_t*)starts, (int32_t*)lengths, (int32_t*)status,
                       (int32_t*)states, (int32_t*)actions, nullptr);
}

static int run_vhz(const irlmx_mdp* m, void* reward, void* term, void* pi, double discount, int horizon, void* v0, void* vt,
                   void* status, void* ws, size_t n) {
  return irlmx_value_horizon(m, (const double*)reward, (const uint8_t*)term, (const double*)pi, discount, horizon, (double*)v0,
                             (double*)vt, (int32_t*)status, ws, n, nullptr);
}

static int run_esh(const irlmx_mdp* m, int model, void* reward, void* term, void* p0, double discount, int horizon,
                   int segment, void* svf, void* obj, void* status, void* ws, size_t n) {
  return irlmx_expected_svf_horizon(m, model, (const double*)reward, (const uint8_t*)term, (const double*)p0, discount, horizon,
                                    segment, (double*)svf, (double*)obj, (int32_t*)status, ws, n, nullptr);
}

static int run_rollhz(const irlmx_mdp* m, int n_traj, int horizon, void* pi, void* term, void* start, void* seed,
                      void* visits, void* starts, void* lengths, void* status, void* states, void* actions) {
  return irlmx_rollout_horizon(m, (const double*)pi, (const uint8_t*)term, (const int32_t*)start, (const uint64_t*)seed,
                               n_traj, horizon, (int64_t*)visits, (int64_t*)starts, (int32_t*)lengths, (int32_t*)status,
                               (int32_t*)states, (int32_t*)actions, nullptr);
}

static void expect(int rc, int want, const char* msg_part, const char* what) {
  CHECK(rc == want, "%s: rc %d, want %d (%s)", what, rc, want, irlmx_last_error());
  CHECK(strstr(irlmx_last_error(), msg_part) != nullptr, "%s: message '%s' lacks '%s'", what, irlmx_last_error(),
        msg_part);
}

static void error_paths() {
  irlmx_mdp good = stencil(5, 5, 4, 1, 1);
  void* f = fake();
  const size_t need = irlmx_workspace_bytes(&good, IRLMX_OP_BACKWARD);
  expect(run_bwd(nullptr, f, f, f, f, f, need), IRLMX_EINVAL, "mdp is NULL", "null mdp");
  struct Bad {
    const char* name;
    irlmx_mdp m;
    const char* msg;
  };
  std::vector<Bad> bad;
  irlmx_mdp m = good; m.n_states = 0; bad.push_back({"S=0", m, "bad sizes"});
  m = good; m.n_actions = 9; bad.push_back({"A=9", m, "exceeds"});
  m = good; m.batch = -1; bad.push_back({"B<0", m, "bad sizes"});
  m = good; m.row_val = nullptr; bad.push_back({"row_val", m, "row_val is NULL"});
  m = good; m.width = 4; bad.push_back({"grid", m, "stencil grid"});
  m = good; m.width = -5; m.height = -5; bad.push_back({"negative grid", m, "stencil grid"});
  m = good; m.layout = 9; bad.push_back({"layout", m, "unknown layout"});
  m = ell(25, 4, 30, 3, 1); bad.push_back({"ell k_row", m, "out of range"});
  m = ell(25, 4, 3, 3, 1); m.row_idx = nullptr; bad.push_back({"ell row_idx", m, "ELL row form missing"});
  m = dense(25, 4, 1); m.col_val = nullptr; bad.push_back({"dense col_val", m, "missing"});
  m = dense(1 << 20, 4, 1); bad.push_back({"dense size", m, "too large"});
  const int ext_op = IRLMX_OP_BACKWARD | IRLMX_PLAN_EXTENDED_RANGE;
  const size_t ext_need = irlmx_workspace_bytes(&good, ext_op);
  CHECK(ext_need > 0, "extended workspace of a good model");
  expect(run_ext(nullptr, f, f, f, f, f, ext_need), IRLMX_EINVAL, "mdp is NULL", "extended null mdp");
  for (const Bad& b : bad) {
    expect(run_ext(&b.m, f, f, f, f, f, ext_need), IRLMX_EINVAL, b.msg, b.name);
    CHECK(irlmx_workspace_bytes(&b.m, ext_op) == 0, "%s: extended workspace of an invalid model", b.name);
    expect(run_bwd(&b.m, f, f, f, f, f, need), IRLMX_EINVAL, b.msg, b.name);
    int64_t plan[IRLMX_PLAN_LEN];
    expect(irlmx_execution_plan(&b.m, IRLMX_OP_FORWARD, plan), IRLMX_EINVAL, b.msg, b.name);
    int32_t props = 0;
    expect(irlmx_mdp_properties(&b.m, &props, nullptr), IRLMX_EINVAL, b.msg, b.name);
    CHECK(irlmx_workspace_bytes(&b.m, IRLMX_OP_FORWARD) == 0, "%s: workspace of an invalid model", b.name);
  }
  expect(run_bwd(&good, nullptr, f, f, f, f, need), IRLMX_EINVAL, "reward is NULL", "null reward");
  expect(run_bwd(&good, f, f, f, nullptr, f, need), IRLMX_EINVAL, "status is NULL", "null status");
  expect(run_bwd(&good, f, f, f, f, f, need - 1), IRLMX_EWORKSPACE, "workspace too small", "short workspace");
  expect(run_bwd(&good, f, f, f, f, nullptr, need), IRLMX_EWORKSPACE, "workspace too small", "null workspace");
  expect(run_ext(&good, nullptr, f, f, f, f, ext_need), IRLMX_EINVAL, "backward_maxent_extended: reward is NULL",
         "extended null reward");
  expect(run_ext(&good, f, nullptr, f, f, f, ext_need), IRLMX_EINVAL, "terminal is NULL", "extended null terminal");
  expect(run_ext(&good, f, f, nullptr, f, f, ext_need), IRLMX_EINVAL, "p_action is NULL", "extended null p_action");
  expect(run_ext(&good, f, f, f, nullptr, f, ext_need), IRLMX_EINVAL, "status is NULL", "extended null status");
  expect(run_ext(&good, f, f, f, f, f, ext_need - 1), IRLMX_EWORKSPACE, "workspace too small", "extended short workspace");
  expect(run_ext(&good, f, f, f, f, f, 0), IRLMX_EWORKSPACE, "workspace too small", "extended empty workspace");
  expect(run_ext(&good, f, f, f, f, nullptr, ext_need), IRLMX_EWORKSPACE, "workspace too small",
         "extended null workspace");
  {
    irlmx_mdp d = dense(25, 4, 1);
    expect(run_ext(&d, f, f, f, f, f, ext_need), IRLMX_EINVAL, "DENSE", "extended dense");
    irlmx_mdp big = stencil((1 << 19) + 1, 1, 4, 1, 1);
    expect(run_ext(&big, f, f, f, f, f, ext_need), IRLMX_EINVAL, "at most 524288 states", "extended S > 2^19");
    int64_t p[IRLMX_PLAN_LEN];
    expect(irlmx_execution_plan(&big, ext_op, p), IRLMX_EINVAL, "at most 524288 states", "extended plan S > 2^19");
    irlmx_mdp wide = ell(100, 4, 40, 3, 2);  // more slots than any fused kernel holds: per sweep
    expect(irlmx_execution_plan(&wide, ext_op, p), IRLMX_OK, "", "extended plan K = 40");
    CHECK(p[0] == IRLMX_SHAPE_SWEEP, "extended plan K = 40: shape %lld", (long long)p[0]);
  }
  {  // irlmx_policy_evaluation: every validation path, in the order the entry checks them
    const size_t pe_need = irlmx_workspace_bytes(&good, IRLMX_OP_POLICY_EVALUATION);
    CHECK(pe_need > 0, "policy evaluation workspace of a good model");
    expect(run_pe(nullptr, f, f, f, 0.9, f, f, f, f, pe_need), IRLMX_EINVAL, "mdp is NULL", "policy evaluation null mdp");
    for (const Bad& b : bad) {
      expect(run_pe(&b.m, f, f, f, 0.9, f, f, f, f, pe_need), IRLMX_EINVAL, b.msg, b.name);
      CHECK(irlmx_workspace_bytes(&b.m, IRLMX_OP_POLICY_EVALUATION) == 0, "%s: policy evaluation workspace of an invalid model",
            b.name);
    }
    irlmx_mdp d = dense(25, 4, 1);
    expect(run_pe(&d, f, f, f, 0.9, f, f, f, f, pe_need), IRLMX_EINVAL, "DENSE", "policy evaluation dense");
    expect(run_pe(&good, nullptr, f, f, 0.9, f, f, f, f, pe_need), IRLMX_EINVAL, "policy_evaluation: reward is NULL",
           "policy evaluation null reward");
    expect(run_pe(&good, f, nullptr, f, 0.9, f, f, f, f, pe_need), IRLMX_EINVAL, "p_action is NULL",
           "policy evaluation null p_action");
    expect(run_pe(&good, f, f, f, 0.9, nullptr, f, f, f, pe_need), IRLMX_EINVAL, "value is NULL", "policy evaluation null value");
    expect(run_pe(&good, f, f, f, 0.9, f, nullptr, f, f, pe_need), IRLMX_EINVAL, "iterations is NULL",
           "policy evaluation null iterations");
    expect(run_pe(&good, f, f, f, 0.9, f, f, nullptr, f, pe_need), IRLMX_EINVAL, "status is NULL",
           "policy evaluation null status");
    expect(run_pe(&good, f, f, f, 1.5, f, f, f, f, pe_need), IRLMX_EINVAL, "outside [0, 1]", "policy evaluation discount 1.5");
    expect(run_pe(&good, f, f, f, -0.5, f, f, f, f, pe_need), IRLMX_EINVAL, "outside [0, 1]", "policy evaluation discount < 0");
    expect(run_pe(&good, f, f, f, strtod("nan", nullptr), f, f, f, f, pe_need), IRLMX_EINVAL, "outside [0, 1]",
           "policy evaluation discount NaN");
    expect(run_pe(&good, f, f, nullptr, 0.9, f, f, f, f, pe_need - 1), IRLMX_EWORKSPACE, "workspace too small",
           "policy evaluation short workspace (terminal NULL is legal)");
    expect(run_pe(&good, f, f, f, 0.9, f, f, f, nullptr, pe_need), IRLMX_EWORKSPACE, "workspace too small",
           "policy evaluation null workspace");
    int64_t p[IRLMX_PLAN_LEN];
    irlmx_mdp wide = ell(100, 4, 40, 3, 2);  // more slots than any fused kernel holds: per sweep
    expect(irlmx_execution_plan(&wide, IRLMX_OP_POLICY_EVALUATION, p), IRLMX_OK, "", "policy evaluation plan K = 40");
    CHECK(p[0] == IRLMX_SHAPE_SWEEP, "policy evaluation plan K = 40: shape %lld", (long long)p[0]);
    expect(irlmx_execution_plan(&good, IRLMX_OP_POLICY_EVALUATION + 1, p), IRLMX_EINVAL, "unknown op 7", "op 7");
    expect(irlmx_execution_plan(&good, 5, p), IRLMX_EINVAL, "unknown op 5", "op 5 (never an op)");
  }
  {  // irlmx_backward_maxent_horizon, irlmx_forward_svf_horizon: every validation path, in the order the entries check them
    irlmx_mdp big = stencil(128, 40, 4, 2, 0);  // per sweep: its workspace is not empty (a fused model needs none)
    const size_t nb = irlmx_workspace_bytes(&big, IRLMX_OP_BACKWARD_HORIZON);
    const size_t nf = irlmx_workspace_bytes(&big, IRLMX_OP_FORWARD_HORIZON);
    CHECK(nb > 0 && nf > 0 && nb > nf, "horizon workspaces of a per-sweep model: %zu, %zu", nb, nf);
    CHECK(irlmx_workspace_bytes(&good, IRLMX_OP_BACKWARD_HORIZON) == 0 && irlmx_workspace_bytes(&good, IRLMX_OP_FORWARD_HORIZON) == 0,
          "horizon workspaces of a fused model");
    expect(run_hzb(nullptr, f, f, 8, f, f, f, f, nb), IRLMX_EINVAL, "mdp is NULL", "horizon backward null mdp");
    expect(run_hzf(nullptr, f, f, f, 8, f, f, f, f, nf), IRLMX_EINVAL, "mdp is NULL", "horizon forward null mdp");
    for (const Bad& b : bad) {
      expect(run_hzb(&b.m, f, f, 8, f, f, f, f, nb), IRLMX_EINVAL, b.msg, b.name);
      expect(run_hzf(&b.m, f, f, f, 8, f, f, f, f, nf), IRLMX_EINVAL, b.msg, b.name);
      CHECK(irlmx_workspace_bytes(&b.m, IRLMX_OP_BACKWARD_HORIZON) == 0 && irlmx_workspace_bytes(&b.m, IRLMX_OP_FORWARD_HORIZON) == 0,
            "%s: horizon workspace of an invalid model", b.name);
    }
    irlmx_mdp d = dense(25, 4, 1);
    expect(run_hzb(&d, f, f, 8, f, f, f, f, nb), IRLMX_EINVAL, "backward_maxent_horizon: the finite-horizon passes do not run the DENSE",
           "horizon backward dense");
    expect(run_hzf(&d, f, f, f, 8, f, f, f, f, nf), IRLMX_EINVAL, "forward_svf_horizon: the finite-horizon passes do not run the DENSE",
           "horizon forward dense");
    irlmx_mdp nocol = ell(25, 4, 3, 3, 1);
    nocol.col_idx = nullptr;
    expect(run_hzf(&nocol, f, f, f, 8, f, f, f, f, nf), IRLMX_EINVAL, "ELL column form missing", "horizon forward without columns");
    irlmx_mdp widecol = ell(25, 4, 3, 30, 1);
    expect(run_hzf(&widecol, f, f, f, 8, f, f, f, f, nf), IRLMX_EINVAL, "ELL k_col=30 out of range (1..25)", "horizon forward k_col > S");
    expect(run_hzb(&big, nullptr, f, 8, f, f, f, f, nb), IRLMX_EINVAL, "backward_maxent_horizon: reward is NULL", "horizon null reward");
    expect(run_hzb(&big, f, f, 8, nullptr, f, f, f, nb), IRLMX_EINVAL, "p_action_t is NULL", "horizon backward null p_action_t");
    expect(run_hzb(&big, f, f, 8, f, f, nullptr, f, nb), IRLMX_EINVAL, "status is NULL", "horizon backward null status");
    expect(run_hzf(&big, nullptr, f, f, 8, f, f, f, f, nf), IRLMX_EINVAL, "forward_svf_horizon: p_initial is NULL", "horizon null p_initial");
    expect(run_hzf(&big, f, f, nullptr, 8, f, f, f, f, nf), IRLMX_EINVAL, "p_action_t is NULL", "horizon forward null p_action_t");
    expect(run_hzf(&big, f, f, f, 8, nullptr, f, f, f, nf), IRLMX_EINVAL, "svf is NULL", "horizon null svf");
    expect(run_hzf(&big, f, f, f, 8, f, f, nullptr, f, nf), IRLMX_EINVAL, "status is NULL", "horizon forward null status");
    for (int h : {0, -1, (1 << 20) + 1}) {
      expect(run_hzb(&big, f, f, h, f, f, f, f, nb), IRLMX_EINVAL, "outside [1, 1048576]", "horizon backward out of range");
      expect(run_hzf(&big, f, f, f, h, f, f, f, f, nf), IRLMX_EINVAL, "outside [1, 1048576]", "horizon forward out of range");
    }
    // terminal, log_z0 and svf_t may be NULL: the calls get as far as the workspace check
    expect(run_hzb(&big, f, nullptr, 1 << 20, f, nullptr, f, f, nb - 1), IRLMX_EWORKSPACE, "workspace too small",
           "horizon backward short workspace (terminal and log_z0 NULL are legal)");
    expect(run_hzf(&big, f, nullptr, f, 1 << 20, f, nullptr, f, f, nf - 1), IRLMX_EWORKSPACE, "workspace too small",
           "horizon forward short workspace (terminal and svf_t NULL are legal)");
    expect(run_hzb(&big, f, f, 8, f, f, f, nullptr, nb), IRLMX_EWORKSPACE, "workspace too small", "horizon backward null workspace");
    expect(run_hzf(&big, f, f, f, 8, f, f, f, nullptr, nf), IRLMX_EWORKSPACE, "workspace too small", "horizon forward null workspace");
    int64_t p[IRLMX_PLAN_LEN];
    irlmx_mdp wide = ell(100, 4, 40, 3, 2);  // more row slots than any fused kernel holds: the backward per sweep
    expect(irlmx_execution_plan(&wide, IRLMX_OP_BACKWARD_HORIZON, p), IRLMX_OK, "", "horizon backward plan K = 40");
    CHECK(p[0] == IRLMX_SHAPE_SWEEP, "horizon backward plan K = 40: shape %lld", (long long)p[0]);
    expect(irlmx_execution_plan(&wide, IRLMX_OP_FORWARD_HORIZON, p), IRLMX_OK, "", "horizon forward plan K_c = 3");
    CHECK(p[0] == IRLMX_SHAPE_FUSED, "horizon forward plan K_c = 3: shape %lld", (long long)p[0]);
    expect(irlmx_execution_plan(&good, IRLMX_OP_FORWARD_HORIZON + 1, p), IRLMX_EINVAL, "unknown op 10", "op 10");
  }
  {  // irlmx_expected_svf_horizon: every validation path, in the order the entry checks them
    const int ME = IRLMX_HORIZON_MODEL_MAXENT, CA = IRLMX_HORIZON_MODEL_CAUSAL;
    const size_t n = irlmx_expected_svf_horizon_workspace_bytes(&good, ME, 8, 0);
    CHECK(n > 0 && n % 256 == 0 && n > irlmx_expected_svf_horizon_workspace_bytes(&good, CA, 8, 0), "expected svf workspaces: %zu", n);
    expect(run_esh(nullptr, ME, f, f, f, 1.0, 8, 0, f, f, f, f, n), IRLMX_EINVAL, "mdp is NULL", "expected svf null mdp");
    int64_t p[6];
    for (const Bad& b : bad) {
      expect(run_esh(&b.m, ME, f, f, f, 1.0, 8, 0, f, f, f, f, n), IRLMX_EINVAL, b.msg, b.name);
      expect(irlmx_expected_svf_horizon_plan(&b.m, ME, 8, 0, p), IRLMX_EINVAL, b.msg, b.name);
      CHECK(irlmx_expected_svf_horizon_workspace_bytes(&b.m, ME, 8, 0) == 0, "%s: expected svf workspace of an invalid model", b.name);
    }
    irlmx_mdp d = dense(25, 4, 1);
    expect(run_esh(&d, ME, f, f, f, 1.0, 8, 0, f, f, f, f, n), IRLMX_EINVAL,
           "expected_svf_horizon: the finite-horizon passes do not run the DENSE", "expected svf dense");
    irlmx_mdp nocol = ell(25, 4, 3, 3, 1);
    nocol.col_idx = nullptr;
    expect(run_esh(&nocol, ME, f, f, f, 1.0, 8, 0, f, f, f, f, n), IRLMX_EINVAL, "ELL column form missing", "expected svf without columns");
    for (int model : {-1, 2})
      expect(run_esh(&good, model, f, f, f, 1.0, 8, 0, f, f, f, f, n), IRLMX_EINVAL, "is neither IRLMX_HORIZON_MODEL_MAXENT nor",
             "expected svf model");
    for (int h : {0, -1, (1 << 20) + 1})
      expect(run_esh(&good, CA, f, f, f, 1.0, h, 0, f, f, f, f, n), IRLMX_EINVAL, "expected_svf_horizon: horizon", "expected svf horizon");
    expect(run_esh(&good, ME, f, f, f, 1.0, 8, -1, f, f, f, f, n), IRLMX_EINVAL, "segment -1 is negative", "expected svf segment");
    expect(run_esh(&good, ME, nullptr, f, f, 1.0, 8, 0, f, f, f, f, n), IRLMX_EINVAL, "expected_svf_horizon: reward is NULL", "expected svf null reward");
    expect(run_esh(&good, ME, f, f, nullptr, 1.0, 8, 0, f, f, f, f, n), IRLMX_EINVAL, "p_initial is NULL", "expected svf null p_initial");
    expect(run_esh(&good, ME, f, f, f, 1.0, 8, 0, nullptr, f, f, f, n), IRLMX_EINVAL, "svf is NULL", "expected svf null svf");
    expect(run_esh(&good, ME, f, f, f, 1.0, 8, 0, f, f, nullptr, f, n), IRLMX_EINVAL, "status is NULL", "expected svf null status");
    for (double g : {-0.1, 1.5, (double)NAN})
      expect(run_esh(&good, CA, f, f, f, g, 8, 0, f, f, f, f, n), IRLMX_EINVAL, "outside [0, 1]", "expected svf causal discount");
    for (double g : {0.9, 0.0, (double)NAN})
      expect(run_esh(&good, ME, f, f, f, g, 8, 0, f, f, f, f, n), IRLMX_EINVAL, "outside {1} (MAXENT)", "expected svf maxent discount");
    // terminal and objective0 may be NULL: the calls get as far as the workspace check
    expect(run_esh(&good, ME, f, nullptr, f, 1.0, 1 << 20, 0, f, nullptr, f, f, n), IRLMX_EWORKSPACE,
           "expected_svf_horizon: workspace too small", "expected svf short workspace (terminal and objective0 NULL are legal)");
    expect(run_esh(&good, CA, f, f, f, 0.0, 8, 0, f, f, f, f, 0), IRLMX_EWORKSPACE, "workspace too small", "expected svf no workspace");
    expect(run_esh(&good, ME, f, f, f, 1.0, 8, 0, f, f, f, f, n - 1), IRLMX_EWORKSPACE, "workspace too small", "expected svf short workspace");
    expect(run_esh(&good, ME, f, f, f, 1.0, 8, 0, f, f, f, nullptr, n), IRLMX_EWORKSPACE, "workspace too small", "expected svf null workspace");
    expect(irlmx_expected_svf_horizon_plan(&good, ME, 8, 0, nullptr), IRLMX_EINVAL, "plan is NULL", "expected svf null plan");
  }
  {  // irlmx_soft_backward_horizon: every validation path, in the order the entry checks them
    const int op = IRLMX_OP_SOFT_BACKWARD_HORIZON;
    irlmx_mdp big = stencil(128, 40, 4, 2, 0);  // per sweep: V's two buffers (a fused model needs no workspace)
    const size_t n = irlmx_workspace_bytes(&big, op);
    CHECK(n >= 2 * 2 * 5120 * sizeof(double) && n % 256 == 0, "soft horizon workspace of a per-sweep model: %zu", n);
    CHECK(irlmx_workspace_bytes(&good, op) == 0, "soft horizon workspace of a fused model");
    expect(run_shz(nullptr, f, f, 0.9, 8, f, f, f, f, n), IRLMX_EINVAL, "mdp is NULL", "soft horizon null mdp");
    for (const Bad& b : bad) {
      expect(run_shz(&b.m, f, f, 0.9, 8, f, f, f, f, n), IRLMX_EINVAL, b.msg, b.name);
      CHECK(irlmx_workspace_bytes(&b.m, op) == 0, "%s: soft horizon workspace of an invalid model", b.name);
    }
    int64_t p[IRLMX_PLAN_LEN];
    irlmx_mdp d = dense(25, 4, 1);
    expect(run_shz(&d, f, f, 0.9, 8, f, f, f, f, n), IRLMX_EINVAL,
           "soft_backward_horizon: the finite-horizon passes do not run the DENSE", "soft horizon dense");
    expect(irlmx_execution_plan(&d, op, p), IRLMX_EINVAL, "execution_plan: the finite-horizon passes do not run the DENSE",
           "soft horizon plan of a DENSE table");
    CHECK(irlmx_workspace_bytes(&d, op) == 0, "soft horizon workspace of a DENSE table");
    expect(run_shz(&big, nullptr, f, 0.9, 8, f, f, f, f, n), IRLMX_EINVAL, "soft_backward_horizon: reward is NULL", "soft horizon null reward");
    expect(run_shz(&big, f, f, 0.9, 8, nullptr, f, f, f, n), IRLMX_EINVAL, "p_action_t is NULL", "soft horizon null p_action_t");
    expect(run_shz(&big, f, f, 0.9, 8, f, f, nullptr, f, n), IRLMX_EINVAL, "status is NULL", "soft horizon null status");
    for (double g : {-0.1, 1.5, (double)NAN, (double)INFINITY})
      expect(run_shz(&big, f, f, g, 8, f, f, f, f, n), IRLMX_EINVAL, "outside [0, 1]", "soft horizon discount out of range");
    for (int h : {0, -1, (1 << 20) + 1})
      expect(run_shz(&big, f, f, 0.9, h, f, f, f, f, n), IRLMX_EINVAL, "outside [1, 1048576]", "soft horizon out of range");
    // terminal and value0 may be NULL, the discount 0 or 1: the calls get as far as the workspace check
    expect(run_shz(&big, f, nullptr, 1.0, 1 << 20, f, nullptr, f, f, n - 1), IRLMX_EWORKSPACE, "workspace too small",
           "soft horizon short workspace (terminal and value0 NULL are legal)");
    expect(run_shz(&big, f, f, 0.0, 8, f, f, f, nullptr, n), IRLMX_EWORKSPACE, "workspace too small", "soft horizon null workspace");
    expect(irlmx_execution_plan(&good, op, p), IRLMX_OK, "", "soft horizon plan of a fused model");
    CHECK(p[0] == IRLMX_SHAPE_FUSED && p[5] == 1 && p[8] == 1 && p[9] == 1536 + 16 * (int64_t)good.n_states,
          "soft horizon fused plan: shape %lld spt %lld LDS %lld", (long long)p[0], (long long)p[5], (long long)p[9]);
    expect(irlmx_execution_plan(&big, op, p), IRLMX_OK, "", "soft horizon plan of a per-sweep model");
    CHECK(p[0] == IRLMX_SHAPE_SWEEP && p[5] == 1 && p[7] == 256 && p[8] == 0 && p[9] == 0, "soft horizon sweep plan");
    irlmx_mdp wide = ell(100, 4, 40, 3, 2);  // more row slots than any fused kernel holds
    expect(irlmx_execution_plan(&wide, op, p), IRLMX_OK, "", "soft horizon plan K = 40");
    CHECK(p[0] == IRLMX_SHAPE_SWEEP, "soft horizon plan K = 40: shape %lld", (long long)p[0]);
    expect(irlmx_execution_plan(&good, op | IRLMX_PLAN_EXTENDED_RANGE, p), IRLMX_EINVAL, "IRLMX_OP_BACKWARD only",
           "extended flag on the soft horizon op");
    expect(irlmx_execution_plan(&good, op | IRLMX_PLAN_NO_RESCALE, p), IRLMX_EINVAL, "NO_RESCALE",
           "no-rescale flag on the soft horizon op");
    expect(irlmx_execution_plan(&good, 99, p), IRLMX_EINVAL, "unknown op 99", "op 99");
  }
  {  // irlmx_rollout, irlmx_demo_statistics, irlmx_demo_log_likelihood: every validation path
    expect(run_roll(nullptr, 8, 16, f, f, f, f, f, f, f, f, f, f), IRLMX_EINVAL, "mdp is NULL", "rollout null mdp");
    for (const Bad& b : bad) expect(run_roll(&b.m, 8, 16, f, f, f, f, f, f, f, f, f, f), IRLMX_EINVAL, b.msg, b.name);
    irlmx_mdp d = dense(25, 4, 1);
    expect(run_roll(&d, 8, 16, f, f, f, f, f, f, f, f, f, f), IRLMX_EINVAL, "rollout: ", "rollout dense");
    expect(run_roll(&d, 8, 16, f, f, f, f, f, f, f, f, f, f), IRLMX_EINVAL, "DENSE", "rollout dense");
    const char* names[8] = {"p_action", "terminal", "start", "seed", "visits", "starts", "lengths", "traj_status"};
    for (int i = 0; i < 8; ++i) {
      void* a[8] = {f, f, f, f, f, f, f, f};
      a[i] = nullptr;
      char msg[64];
      snprintf(msg, sizeof(msg), "rollout: %s is NULL", names[i]);
      expect(run_roll(&good, 8, 16, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], f, f), IRLMX_EINVAL, msg, msg);
    }
    expect(run_roll(&good, 0, 16, f, f, f, f, f, f, f, f, f, f), IRLMX_EINVAL, "n_traj=0 < 1", "rollout n_traj 0");
    expect(run_roll(&good, 8, 0, f, f, f, f, f, f, f, f, f, f), IRLMX_EINVAL, "max_len=0 outside [1, 1048576]",
           "rollout max_len 0");
    expect(run_roll(&good, 8, (1 << 20) + 1, f, f, f, f, f, f, f, f, f, f), IRLMX_EINVAL, "max_len=1048577 outside",
           "rollout max_len above the cap");
    expect(run_roll(&good, 8, 16, f, f, f, f, f, f, f, f, f, nullptr), IRLMX_EINVAL, "both be NULL or both be set",
           "rollout states without actions");
    expect(run_roll(&good, 8, 16, f, f, f, f, f, f, f, f, nullptr, f), IRLMX_EINVAL, "both be NULL or both be set",
           "rollout actions without states");
    int32_t* i32 = (int32_t*)f;
    int64_t* i64 = (int64_t*)f;
    double* dbl = (double*)f;
    expect(irlmx_demo_statistics(0, 1, 8, 17, i32, i32, i64, i64, i32, nullptr), IRLMX_EINVAL, "demo_statistics: bad sizes",
           "statistics S = 0");
    expect(irlmx_demo_statistics(25, 1, 0, 17, i32, i32, i64, i64, i32, nullptr), IRLMX_EINVAL, "n_traj=0 < 1",
           "statistics n_traj 0");
    expect(irlmx_demo_statistics(25, 1, 8, 0, i32, i32, i64, i64, i32, nullptr), IRLMX_EINVAL, "stride=0 < 1",
           "statistics stride 0");
    expect(irlmx_demo_statistics(25, 1, 8, 17, nullptr, i32, i64, i64, i32, nullptr), IRLMX_EINVAL,
           "demo_statistics: states is NULL", "statistics null states");
    expect(irlmx_demo_statistics(25, 1, 8, 17, i32, nullptr, i64, i64, i32, nullptr), IRLMX_EINVAL, "lengths is NULL",
           "statistics null lengths");
    expect(irlmx_demo_statistics(25, 1, 8, 17, i32, i32, nullptr, i64, i32, nullptr), IRLMX_EINVAL, "visits is NULL",
           "statistics null visits");
    expect(irlmx_demo_statistics(25, 1, 8, 17, i32, i32, i64, nullptr, i32, nullptr), IRLMX_EINVAL, "starts is NULL",
           "statistics null starts");
    expect(irlmx_demo_statistics(25, 1, 8, 17, i32, i32, i64, i64, nullptr, nullptr), IRLMX_EINVAL, "traj_status is NULL",
           "statistics null status");
    expect(irlmx_demo_log_likelihood(25, 0, 1, 8, 17, dbl, i32, i32, i32, dbl, dbl, i32, nullptr), IRLMX_EINVAL,
           "demo_log_likelihood: bad sizes", "likelihood A = 0");
    expect(irlmx_demo_log_likelihood(25, 4, 1, -2, 17, dbl, i32, i32, i32, dbl, dbl, i32, nullptr), IRLMX_EINVAL,
           "n_traj=-2 < 1", "likelihood n_traj < 0");
    expect(irlmx_demo_log_likelihood(25, 4, 1, 8, 0, dbl, i32, i32, i32, dbl, dbl, i32, nullptr), IRLMX_EINVAL,
           "stride=0 < 1", "likelihood stride 0");
    expect(irlmx_demo_log_likelihood(25, 4, 1, 8, 17, nullptr, i32, i32, i32, dbl, dbl, i32, nullptr), IRLMX_EINVAL,
           "demo_log_likelihood: p_action is NULL", "likelihood null p_action");
    expect(irlmx_demo_log_likelihood(25, 4, 1, 8, 17, dbl, nullptr, i32, i32, dbl, dbl, i32, nullptr), IRLMX_EINVAL,
           "states is NULL", "likelihood null states");
    expect(irlmx_demo_log_likelihood(25, 4, 1, 8, 17, dbl, i32, nullptr, i32, dbl, dbl, i32, nullptr), IRLMX_EINVAL,
           "actions is NULL", "likelihood null actions");
    expect(irlmx_demo_log_likelihood(25, 4, 1, 8, 17, dbl, i32, i32, nullptr, dbl, dbl, i32, nullptr), IRLMX_EINVAL,
           "lengths is NULL", "likelihood null lengths");
    expect(irlmx_demo_log_likelihood(25, 4, 1, 8, 17, dbl, i32, i32, i32, nullptr, dbl, i32, nullptr), IRLMX_EINVAL,
           "ll_traj is NULL", "likelihood null ll_traj");
    expect(irlmx_demo_log_likelihood(25, 4, 1, 8, 17, dbl, i32, i32, i32, dbl, nullptr, i32, nullptr), IRLMX_EINVAL,
           "ll is NULL", "likelihood null ll");
    expect(irlmx_demo_log_likelihood(25, 4, 1, 8, 17, dbl, i32, i32, i32, dbl, dbl, nullptr, nullptr), IRLMX_EINVAL,
           "traj_status is NULL", "likelihood null status");
  }
  {  // irlmx_value_horizon, irlmx_rollout_horizon, irlmx_demo_log_likelihood_horizon: every validation path
    const int op = IRLMX_OP_VALUE_HORIZON;
    irlmx_mdp big = stencil(128, 40, 4, 2, 0);  // per sweep: v's two buffers (a fused model needs no workspace)
    const size_t n = irlmx_workspace_bytes(&big, op);
    CHECK(n >= 2 * 2 * 5120 * sizeof(double) && n % 256 == 0, "value horizon workspace of a per-sweep model: %zu", n);
    CHECK(irlmx_workspace_bytes(&good, op) == 0, "value horizon workspace of a fused model");
    expect(run_vhz(nullptr, f, f, f, 0.9, 8, f, f, f, f, n), IRLMX_EINVAL, "mdp is NULL", "value horizon null mdp");
    expect(run_rollhz(nullptr, 8, 16, f, f, f, f, f, f, f, f, f, f), IRLMX_EINVAL, "mdp is NULL", "rollout horizon null mdp");
    for (const Bad& b : bad) {
      expect(run_vhz(&b.m, f, f, f, 0.9, 8, f, f, f, f, n), IRLMX_EINVAL, b.msg, b.name);
      expect(run_rollhz(&b.m, 8, 16, f, f, f, f, f, f, f, f, f, f), IRLMX_EINVAL, b.msg, b.name);
      CHECK(irlmx_workspace_bytes(&b.m, op) == 0, "%s: value horizon workspace of an invalid model", b.name);
    }
    int64_t p[IRLMX_PLAN_LEN];
    irlmx_mdp d = dense(25, 4, 1);
    expect(run_vhz(&d, f, f, f, 0.9, 8, f, f, f, f, n), IRLMX_EINVAL, "value_horizon: the finite-horizon passes do not run the DENSE",
           "value horizon dense");
    expect(run_rollhz(&d, 8, 16, f, f, f, f, f, f, f, f, f, f), IRLMX_EINVAL,
           "rollout_horizon: the finite-horizon passes do not run the DENSE", "rollout horizon dense");
    expect(irlmx_execution_plan(&d, op, p), IRLMX_EINVAL, "execution_plan: the finite-horizon passes do not run the DENSE",
           "value horizon plan of a DENSE table");
    expect(run_vhz(&big, nullptr, f, f, 0.9, 8, f, f, f, f, n), IRLMX_EINVAL, "value_horizon: reward is NULL", "value horizon null reward");
    expect(run_vhz(&big, f, f, f, 0.9, 8, nullptr, f, f, f, n), IRLMX_EINVAL, "value0 is NULL", "value horizon null value0");
    expect(run_vhz(&big, f, f, f, 0.9, 8, f, f, nullptr, f, n), IRLMX_EINVAL, "status is NULL", "value horizon null status");
    for (double g : {-0.1, 1.5, (double)NAN, (double)INFINITY})
      expect(run_vhz(&big, f, f, f, g, 8, f, f, f, f, n), IRLMX_EINVAL, "outside [0, 1]", "value horizon discount out of range");
    for (int h : {0, -1, (1 << 20) + 1}) {
      expect(run_vhz(&big, f, f, f, 0.9, h, f, f, f, f, n), IRLMX_EINVAL, "outside [1, 1048576]", "value horizon out of range");
      expect(run_rollhz(&good, 8, h, f, f, f, f, f, f, f, f, f, f), IRLMX_EINVAL, "outside [1, 1048576]", "rollout horizon out of range");
      expect(irlmx_demo_log_likelihood_horizon(25, 4, 1, 8, 17, h, (double*)f, (int32_t*)f, (int32_t*)f, (int32_t*)f, (double*)f,
                                               (double*)f, (int32_t*)f, nullptr),
             IRLMX_EINVAL, "demo_log_likelihood_horizon: horizon", "likelihood horizon out of range");
    }
    // terminal, p_action_t and value_t may be NULL, the discount 0 or 1: the calls get as far as the workspace check
    expect(run_vhz(&big, f, nullptr, nullptr, 1.0, 1 << 20, f, nullptr, f, f, n - 1), IRLMX_EWORKSPACE, "workspace too small",
           "value horizon short workspace (terminal, p_action_t and value_t NULL are legal)");
    expect(run_vhz(&big, f, f, f, 0.0, 8, f, f, f, nullptr, n), IRLMX_EWORKSPACE, "workspace too small", "value horizon null workspace");
    expect(irlmx_execution_plan(&good, op, p), IRLMX_OK, "", "value horizon plan of a fused model");
    CHECK(p[0] == IRLMX_SHAPE_FUSED && p[5] == 1 && p[8] == 1 && p[9] == 16 * (int64_t)good.n_states,
          "value horizon fused plan: shape %lld spt %lld LDS %lld", (long long)p[0], (long long)p[5], (long long)p[9]);
    expect(irlmx_execution_plan(&big, op, p), IRLMX_OK, "", "value horizon plan of a per-sweep model");
    CHECK(p[0] == IRLMX_SHAPE_SWEEP && p[5] == 1 && p[7] == 256 && p[8] == 0 && p[9] == 0, "value horizon sweep plan");
    const char* names[7] = {"p_action_t", "start", "seed", "visits", "starts", "lengths", "traj_status"};
    for (int i = 0; i < 7; ++i) {
      void* a[7] = {f, f, f, f, f, f, f};
      a[i] = nullptr;
      char msg[64];
      snprintf(msg, sizeof(msg), "rollout_horizon: %s is NULL", names[i]);
      expect(run_rollhz(&good, 8, 16, a[0], nullptr, a[1], a[2], a[3], a[4], a[5], a[6], f, f), IRLMX_EINVAL, msg, msg);
    }
    expect(run_rollhz(&good, 0, 16, f, f, f, f, f, f, f, f, f, f), IRLMX_EINVAL, "n_traj=0 < 1", "rollout horizon n_traj 0");
    expect(run_rollhz(&good, 8, 16, f, f, f, f, f, f, f, f, f, nullptr), IRLMX_EINVAL, "both be NULL or both be set",
           "rollout horizon states without actions");
    expect(run_rollhz(&good, 8, 16, f, f, f, f, f, f, f, f, nullptr, f), IRLMX_EINVAL, "both be NULL or both be set",
           "rollout horizon actions without states");
    int32_t* i32 = (int32_t*)f;
    double* dbl = (double*)f;
    expect(irlmx_demo_log_likelihood_horizon(25, 0, 1, 8, 17, 16, dbl, i32, i32, i32, dbl, dbl, i32, nullptr), IRLMX_EINVAL,
           "demo_log_likelihood_horizon: bad sizes", "timed likelihood A = 0");
    expect(irlmx_demo_log_likelihood_horizon(25, 4, 1, 0, 17, 16, dbl, i32, i32, i32, dbl, dbl, i32, nullptr), IRLMX_EINVAL,
           "n_traj=0 < 1", "timed likelihood n_traj 0");
    expect(irlmx_demo_log_likelihood_horizon(25, 4, 1, 8, 0, 16, dbl, i32, i32, i32, dbl, dbl, i32, nullptr), IRLMX_EINVAL,
           "stride=0 < 1", "timed likelihood stride 0");
    const char* lnames[7] = {"p_action_t", "states", "actions", "lengths", "ll_traj", "ll", "traj_status"};
    for (int i = 0; i < 7; ++i) {
      void* a[7] = {f, f, f, f, f, f, f};
      a[i] = nullptr;
      char msg[80];
      snprintf(msg, sizeof(msg), "demo_log_likelihood_horizon: %s is NULL", lnames[i]);
      expect(irlmx_demo_log_likelihood_horizon(25, 4, 1, 8, 17, 16, (double*)a[0], (int32_t*)a[1], (int32_t*)a[2], (int32_t*)a[3],
                                               (double*)a[4], (double*)a[5], (int32_t*)a[6], nullptr),
             IRLMX_EINVAL, msg, msg);
    }
  }
  expect(irlmx_forward_svf(&good, (double*)f, (uint8_t*)f, (double*)f, 1e-5, 0, (double*)f, nullptr, (int32_t*)f, f,
                           1 << 30, nullptr),
         IRLMX_EINVAL, "iterations is NULL", "forward null iterations");
  expect(irlmx_soft_backward(&good, (double*)f, nullptr, 0.7, 1e-5, 0, (double*)f, nullptr, (int64_t*)f,
                             (int32_t*)f, f, 1 << 30, nullptr),
         IRLMX_EINVAL, "terminal_reward is NULL", "soft null phi");
  expect(irlmx_value_iteration(&good, (double*)f, 0.9, 1e-3, 0, 0, nullptr, (int64_t*)f, (int32_t*)f, f, 1 << 30,
                               nullptr),
         IRLMX_EINVAL, "value is NULL", "vi null value");
  int64_t plan[IRLMX_PLAN_LEN];
  expect(irlmx_execution_plan(&good, 0, plan), IRLMX_EINVAL, "unknown op 0", "op 0");
  expect(irlmx_execution_plan(&good, -1, plan), IRLMX_EINVAL, "unknown op -1", "op -1");
  expect(irlmx_execution_plan(&good, IRLMX_OP_FORWARD | IRLMX_PLAN_NO_RESCALE, plan), IRLMX_EINVAL, "NO_RESCALE",
         "no-rescale forward");
  expect(irlmx_execution_plan(&good, IRLMX_OP_FORWARD, nullptr), IRLMX_EINVAL, "plan is NULL", "null plan");
  expect(irlmx_mdp_properties(nullptr, (int32_t*)f, nullptr), IRLMX_EINVAL, "mdp is NULL", "props null mdp");
  expect(irlmx_mdp_properties(&good, nullptr, nullptr), IRLMX_EINVAL, "props is NULL", "props null out");
  expect(irlmx_numpy_math(2, (double*)f, (double*)f, 4, nullptr), IRLMX_EINVAL, "unknown op 2", "npmath op");
  expect(irlmx_numpy_math(IRLMX_NPMATH_EXP, (double*)f, (double*)f, -1, nullptr), IRLMX_EINVAL, "< 0", "npmath n");
  expect(irlmx_numpy_math(IRLMX_NPMATH_LOG, nullptr, (double*)f, 4, nullptr), IRLMX_EINVAL, "NULL", "npmath null");
  expect(irlmx_numpy_math(IRLMX_NPMATH_EXP, nullptr, nullptr, 0, nullptr), IRLMX_OK, "", "npmath empty");
  expect(irlmx_build_icy_gridworld(0, (double*)f, 1, (double*)f, nullptr), IRLMX_EINVAL, "size=0", "icy size");
  expect(irlmx_build_gridworld(50000, 1, (double*)f, nullptr), IRLMX_EINVAL, "size=50000", "grid size");
  expect(irlmx_dense_to_stencil((double*)f, 5, 5, 4, (double*)f, nullptr, nullptr), IRLMX_EINVAL, "off_stencil NULL",
         "stencil flag");
  expect(irlmx_dense_to_rows((double*)f, 25, 9, (double*)f, (double*)f, nullptr), IRLMX_EINVAL, "n_actions=9",
         "rows actions");
  expect(irlmx_dense_ell_sizes((double*)f, 0, 4, (int32_t*)f, (int32_t*)f, nullptr), IRLMX_EINVAL, "n_states=0",
         "ell sizes");
  expect(irlmx_dense_to_ell((double*)f, 25, 4, 26, 3, (int32_t*)f, (double*)f, (int32_t*)f, (double*)f, nullptr),
         IRLMX_EINVAL, "k_row=26", "ell k");
  expect(irlmx_optimal_policy((int32_t*)f, 25, 4, 1, nullptr, (int64_t*)f, nullptr), IRLMX_EINVAL, "value NULL",
         "argmax value");
  expect(irlmx_stochastic_policy((int32_t*)f, 25, 0, 1, (double*)f, (double*)f, nullptr), IRLMX_EINVAL,
         "n_actions=0", "stochastic actions");
  int64_t ctr[IRLMX_COUNTERS_LEN + 4];
  CHECK(irlmx_counters(ctr, IRLMX_COUNTERS_LEN + 4) == IRLMX_COUNTERS_LEN, "counters length");
  CHECK(irlmx_counters(nullptr, 3) == IRLMX_COUNTERS_LEN, "counters length (NULL)");
}

// The models of the planner sweep, each handed to f(model, tag); returns their number.
template <class F>
static long long for_each_model(F&& f) {
  std::vector<int> widths, batches;
  for (int w = 5; w <= 40; ++w) widths.push_back(w);
  for (int w = 41; w <= 256; w += 9) widths.push_back(w);
  for (int w : {48, 63, 64, 65, 96, 127, 128, 129, 192, 255, 256}) widths.push_back(w);
  for (int b = 1; b <= 16; ++b) batches.push_back(b);
  for (int b : {17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256}) batches.push_back(b);
  long long models = 0;
  for (int w : widths) {
    for (int b : batches) {
      for (int shared = 0; shared <= 1; ++shared) {
        f(stencil(w, w, 4, b, shared), "square");
        f(stencil(w, w, 5, b, shared), "square A=5");
        models += 2;
      }
      if (w % 3 == 0) {  // rectangles: wide and tall
        f(stencil(w, 2 * w + 1, 4, b, 0), "tall");
        f(stencil(2 * w, w, 4, b, 0), "wide");
        models += 2;
      }
    }
  }
  // generic sparsity and dense rows: state counts around the fused / grid boundaries
  for (int s : {5, 25, 100, 1000, 4095, 4096, 4097, 10000, 16384, 40000}) {
    for (int k : {1, 2, 5, 8, 9, 16, 17, 32, 33}) {
      if (k > s) continue;
      for (int b : {1, 3, 16, 64, 256}) {
        f(ell(s, 4, k, k, b), "ell");
        f(ell(s, 4, k, (k % 5) + 1, b), "ell skew");
        models += 2;
      }
    }
  }
  for (int s : {7, 64, 301, 1040, 2048, 4096, 8192})
    for (int b : {1, 3, 4, 15, 16, 17, 64}) {
      f(dense(s, 4, b), "dense");
      ++models;
    }
  return models;
}

// --dump: for every model of the sweep and every op (the four passes, the
// backward with IRLMX_PLAN_NO_RESCALE and with IRLMX_PLAN_EXTENDED_RANGE, policy
// evaluation) one line with the plan's return code, plan[0..9] and the
// workspace bytes -- first with the planner's defaults, then with each of its
// shape switches set alone.  Two libraries that print the same text plan and
// size every call of the sweep alike.
static void dump_plans() {
  const char* const switches[][2] = {{nullptr, nullptr},
                                     {"IRLMX_FUSED_MAX_STATES", "0"},
                                     {"IRLMX_CLUSTER", "0"},
                                     {"IRLMX_GRID", "0"},
                                     {"IRLMX_DENSE_GEMM_MIN", "1"},
                                     {"IRLMX_EXT_GRID_MAX_LAUNCHES", "1000"}};
  const int ops[] = {IRLMX_OP_BACKWARD, IRLMX_OP_FORWARD, IRLMX_OP_SOFT_BACKWARD, IRLMX_OP_VALUE_ITERATION,
                     IRLMX_OP_BACKWARD | IRLMX_PLAN_NO_RESCALE, IRLMX_OP_BACKWARD | IRLMX_PLAN_EXTENDED_RANGE,
                     IRLMX_OP_POLICY_EVALUATION, IRLMX_OP_BACKWARD_HORIZON, IRLMX_OP_FORWARD_HORIZON,
                     IRLMX_OP_SOFT_BACKWARD_HORIZON, IRLMX_OP_VALUE_HORIZON};
  for (const auto& sw : switches) {
    if (sw[0]) setenv(sw[0], sw[1], 1);
    for_each_model([&](const irlmx_mdp& m, const char* tag) {
      for (int op : ops) {
        int64_t p[IRLMX_PLAN_LEN];
        for (auto& v : p) v = -7;
        const int rc = irlmx_execution_plan(&m, op, p);
        printf("%s=%s %s %dx%d S %d A %d K %d/%d B %d shared %d op %#x: rc %d plan", sw[0] ? sw[0] : "default",
               sw[0] ? sw[1] : "", tag, m.width, m.height, m.n_states, m.n_actions, m.k_row, m.k_col, m.batch, m.shared,
               op, rc);
        for (int64_t v : p) printf(" %lld", (long long)v);
        // (workspace_bytes takes no IRLMX_PLAN_NO_RESCALE: the backward's workspace serves both)
        printf(" ws %zu\n", irlmx_workspace_bytes(&m, op & ~IRLMX_PLAN_NO_RESCALE));
      }
    });
    if (sw[0]) unsetenv(sw[0]);
  }
}

int main(int argc, char** argv) {
  setenv("IRLMX_PLAN_CUS", "256", 1);          // the MI355X's CU count, without a device
  setenv("IRLMX_PLAN_GRID_PER_CU", "4", 1);
  if (argc > 1 && strcmp(argv[1], "--dump") == 0) {
    dump_plans();
    return 0;
  }
  CHECK(irlmx_abi_version() == IRLMX_ABI_VERSION, "abi version");
  error_paths();

  const long long plans = 4 * for_each_model([](const irlmx_mdp& m, const char* tag) { plan_and_workspace(m, tag); });
  if (g_fail) {
    fprintf(stderr, "host_check: %d of %lld checks failed\n", g_fail, g_checks);
    return 1;
  }
  CHECK(g_shapes[IRLMX_SHAPE_CLUSTER] > 1000 && g_shapes[IRLMX_SHAPE_GRID] > 100 && g_shapes[IRLMX_SHAPE_FUSED] > 100 &&
            g_shapes[IRLMX_SHAPE_DENSE_GEMM] > 0 && g_shapes[IRLMX_SHAPE_DENSE] > 0 &&
            g_shapes[IRLMX_SHAPE_DENSE_GRID] > 0,
        "every shape planned: fused %lld cluster %lld sweep %lld dense %lld gemm %lld grid %lld dense-grid %lld",
        g_shapes[0], g_shapes[1], g_shapes[2], g_shapes[3], g_shapes[4], g_shapes[5], g_shapes[6]);
  if (g_fail) {
    fprintf(stderr, "host_check: %d of %lld checks failed\n", g_fail, g_checks);
    return 1;
  }
  CHECK(g_ext_shapes[0] > 100 && g_ext_shapes[1] > 100 && g_ext_shapes[2] > 100,
        "extended shapes planned: fused %lld grid %lld sweep %lld", g_ext_shapes[0], g_ext_shapes[1], g_ext_shapes[2]);
  if (g_fail) {
    fprintf(stderr, "host_check: %d of %lld checks failed\n", g_fail, g_checks);
    return 1;
  }
  CHECK(g_pe_shapes[0] > 100 && g_pe_shapes[2] > 100, "policy evaluation shapes planned: fused %lld sweep %lld",
        g_pe_shapes[0], g_pe_shapes[2]);
  CHECK(g_hz_shapes[0] > 200 && g_hz_shapes[2] > 200, "horizon shapes planned: fused %lld sweep %lld", g_hz_shapes[0],
        g_hz_shapes[2]);
  CHECK(g_esh_shapes[0] > 200 && g_esh_shapes[2] > 200, "expected svf shapes planned: fused %lld per step %lld", g_esh_shapes[0],
        g_esh_shapes[2]);
  if (g_fail) {
    fprintf(stderr, "host_check: %d of %lld checks failed\n", g_fail, g_checks);
    return 1;
  }
  printf("host_check ok: %lld plans, %lld checks; shapes fused %lld cluster %lld sweep %lld dense %lld dense-gemm %lld "
         "grid %lld dense-grid %lld\n", plans, g_checks, g_shapes[0], g_shapes[1], g_shapes[2], g_shapes[3], g_shapes[4],
         g_shapes[5], g_shapes[6]);
  return 0;
}

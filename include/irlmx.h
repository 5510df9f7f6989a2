/*
 * irlmx -- MI355X-native MaxEnt-IRL inner loop: C ABI of libirlmx.so.
 *
 * The reference (narendasan/irl-maxent) has no FFI: its hot path is a set of
 * module-level numpy functions in src/maxent.py and src/solver.py that
 * src/main.py imports as `import maxent as M`, `import solver as S`
 * (main.py:4, 7).  Each entry point below replaces the numeric core of one of
 * those functions; the Python drop-in modules (irl-maxent_amd/maxent.py,
 * irl-maxent_amd/solver.py) keep the reference's names, signatures and return
 * types and call these through ctypes.
 *
 * Conventions
 *  - Every array pointer is a caller-owned DEVICE buffer (e.g. a torch tensor's
 *    data_ptr()); the library allocates nothing.  `stream` is a hipStream_t.
 *  - Instances: B independent problems are processed per call.  Per-instance
 *    arrays are packed [B][...] in the layouts stated per argument.
 *  - Return value: IRLMX_SUCCESS (0) or a negative IRLMX_E* code; the message
 *    of the last failure on this thread is irlmx_last_error().
 *  - Per-instance outcome codes (IRLMX_OK / _NONFINITE / _MAXITER) are written
 *    to `status`, and the number of sweeps each fixed-point loop ran to
 *    `iterations` -- the count of iterations of the reference's `while` loop.
 *  - Work is enqueued on `stream`.  Calls whose sweep count is data dependent
 *    and that do not fit one workgroup per instance (large state spaces)
 *    synchronise `stream` while they run; all others are fully asynchronous.
 *  - Arithmetic is IEEE float64 throughout, as in the reference.
 */
#ifndef IRLMX_H
#define IRLMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IRLMX_ABI_VERSION 1

/* transition-table layouts (see irlmx_mdp) */
#define IRLMX_LAYOUT_STENCIL5 1 /* grid-local: self, +x, -x, +y, -y on a width x height grid */
#define IRLMX_LAYOUT_ELL 2      /* generic sparse: k_row target slots per state */
#define IRLMX_LAYOUT_DENSE 3    /* dense rows: per-action S x S matrices (non-grid, dense P) */

/* return codes */
#define IRLMX_SUCCESS 0
#define IRLMX_EINVAL (-1)
#define IRLMX_EHIP (-2)
#define IRLMX_EWORKSPACE (-3)

/* per-instance status */
#define IRLMX_OK 0
#define IRLMX_NONFINITE 1 /* a NaN stopped the loop (the reference's `while delta > eps` exits on NaN) */
#define IRLMX_MAXITER 2   /* stopped by the optional sweep cap before convergence */

/* workspace owners (irlmx_workspace_bytes) */
#define IRLMX_OP_BACKWARD 1
#define IRLMX_OP_FORWARD 2
#define IRLMX_OP_SOFT_BACKWARD 3
#define IRLMX_OP_VALUE_ITERATION 4
#define IRLMX_OP_POLICY_EVALUATION 6 /* 5 stays an unknown op: ABI version 1 has always answered "unknown op 5" */
#define IRLMX_OP_BACKWARD_HORIZON 8  /* 5 and 7 stay unknown ops: tests and tools/sanitize pin both answers */
#define IRLMX_OP_FORWARD_HORIZON 9
#define IRLMX_OP_SOFT_BACKWARD_HORIZON 11 /* 10 stays an unknown op too: the same tests pin "unknown op 10" */
#define IRLMX_OP_VALUE_HORIZON 12 /* irlmx_value_horizon (irlmx_timed.h); 5, 7 and 10 stay unknown ops */

/*
 * Transition model P[from, to, action] of B instances (the reference's dense
 * `p_transition`, gridworld.py:124-142), stored compactly in HBM.
 *
 *  row form  (used by the backward passes and value iteration):
 *    row_val[b'][a][k][s] = P[s, target_k(s), a]       (float64)
 *    STENCIL5: target_k(s) is the k-th stencil neighbour of s; row_idx unused.
 *    ELL     : target_k(s) = row_idx[b'][k][s]; unused slots have value 0.
 *  column form (used by the forward SVF pass, ELL only; STENCIL5 derives it):
 *    col_idx[b'][k][t] = source state s of slot k of target t,
 *    col_val[b'][a][k][t] = P[s, t, a].
 *  dense form (DENSE: most (s, t) pairs nonzero, where ELL would gather ~S slots
 *  per state):
 *    row_val[b'][a][s][t] = P[s, t, a]     the reference's slices P[:, :, a]
 *                                          (maxent.py:102, 143, 320), row-major
 *    col_val[b'][s][t]    = sum_a P[s, t, a]  (action-summed, for the backward)
 *    row_idx, col_idx unused; k_row = k_col = n_states.
 *  b' = 0 when `shared` is nonzero (one table for all B instances), else b.
 *  props: 0 (unknown: entry points that depend on a table property check it on
 *  the device per call, which synchronises the stream) or the value
 *  irlmx_mdp_properties() returned for exactly these table contents.
 */
typedef struct irlmx_mdp {
  int32_t layout;
  int32_t n_states;
  int32_t n_actions;
  int32_t width;  /* STENCIL5 only */
  int32_t height; /* STENCIL5 only */
  int32_t k_row;  /* slots per state in the row form (5 for STENCIL5) */
  int32_t k_col;  /* slots per state in the column form (ELL) */
  int32_t batch;
  int32_t shared;
  int32_t props;  /* 0, or irlmx_mdp_properties()'s result for these tables (see there) */
  const double* row_val;
  const int32_t* row_idx;
  const int32_t* col_idx;
  const double* col_val;
} irlmx_mdp;

int irlmx_abi_version(void);
const char* irlmx_last_error(void);

/*
 * Process-wide event counters (diagnostics; no reference counterpart): how often
 * the persistent shapes ran and how often a call was rerun on the per-sweep
 * shape.  Copies min(n, IRLMX_COUNTERS_LEN) counters into out (host memory) and
 * returns IRLMX_COUNTERS_LEN.  Counts only grow; callers take differences.
 */
#define IRLMX_COUNTERS_LEN 6
#define IRLMX_CTR_CLUSTER_LAUNCHES 0   /* persistent cluster launches (stencil forward / backward) */
#define IRLMX_CTR_GRID_LAUNCHES 1      /* persistent grid and dense grid launches (soft VI / VI, ELL and DENSE passes) */
#define IRLMX_CTR_RERUN_NONFINITE 2    /* cluster forward saw a non-finite value: rerun per sweep (exact NaN rules) */
#define IRLMX_CTR_RERUN_NOT_RESIDENT 3 /* workgroups could not all run at once: rerun per sweep */
#define IRLMX_CTR_RERUN_TIMEOUT 4      /* a halo / value exchange timed out (a descheduled workgroup): rerun per sweep */
#define IRLMX_CTR_SWEEP_CALLS 5        /* calls (or reruns) that took the per-sweep shape */
int irlmx_counters(int64_t* out, int32_t n);

/*
 * Device bounds checks (diagnostics; no reference
 * counterpart).  A library built with -DIRLMX_DEVICE_CHECKS=1 checks, inside the
 * kernels, every ELL slot index against [0, S), every halo / value granule
 * offset against its buffer, and every persistent tile's row range against the
 * grid and its LDS buffer; a failed check skips the access and sets a bit
 * (1: index, 2: granule, 4: tile) instead of faulting.
 * irlmx_device_check_failures() synchronises the device and returns the bits
 * set since the last call (then clears them); always 0 in a normal build
 * (irlmx_device_checks_enabled() == 0), -1 on a HIP error.
 */
int irlmx_device_checks_enabled(void);
int64_t irlmx_device_check_failures(void);

/*
 * Structural properties of the model's tables (no reference counterpart), so
 * that calls need not re-check them: computed on the device once, written to
 * *props (IRLMX_PROPS_KNOWN | the IRLMX_PROP_* bits that hold); synchronises
 * `stream`.  Store the value in irlmx_mdp.props for later calls on the same
 * tables; it describes their contents when computed -- edit a table in place and
 * props must go back to 0 (or be recomputed).
 *   IRLMX_PROP_COMPACT     STENCIL5: the collapsed backward coefficients have
 *                          the structure of the compact-weight cluster layout
 *                          (equal +x / -x coefficients inside the grid, no self
 *                          coefficient off the border; used at width 256)
 *   IRLMX_PROP_ELL_SORTED  ELL: every row holds its nonzero entries in ascending
 *                          column order (the *_numpy_order entry points need it)
 */
#define IRLMX_PROPS_KNOWN 0x40000000
#define IRLMX_PROP_COMPACT 0x1
#define IRLMX_PROP_ELL_SORTED 0x2
int irlmx_mdp_properties(const irlmx_mdp* mdp, int32_t* props, void* stream);

/*
 * numpy's float64 exp / log as the kernels evaluate them (np_exp / np_log in
 * csrc/common.h: the soft VI softmax, maxent.py:260-276, and its policy,
 * maxent.py:341; diagnostics and parity tests, no reference counterpart):
 * y[i] = f(x[i]) for 0 <= i < n on device pointers, asynchronous on `stream`.
 * op IRLMX_NPMATH_EXP or IRLMX_NPMATH_LOG; n = 0 is a no-op.
 */
#define IRLMX_NPMATH_EXP 0
#define IRLMX_NPMATH_LOG 1
int irlmx_numpy_math(int32_t op, const double* x, double* y, int64_t n, void* stream);

/*
 * Bytes of device workspace `op` needs for this model (0 is a valid answer; a
 * multiple of 256).
 *
 * The call contract of every entry point that takes `workspace`,
 * `workspace_bytes` (tests/test_gpu_call_contract.py holds each of them, on
 * every execution shape, to all of it):
 *  - The contents of the workspace on entry are ignored: a call's results do not
 *    depend on them, so a workspace may come straight from an allocator or from
 *    an earlier call, of this or any other entry point.  Its contents on return
 *    are unspecified.
 *  - A call reads and writes nothing at or beyond workspace + workspace_bytes,
 *    and nothing before workspace.  workspace_bytes may be larger than the
 *    need; a need of 0 accepts a NULL workspace.
 *  - workspace is aligned as hipMalloc and torch's allocator align theirs, to
 *    256 bytes.  (The library does not check the alignment.)
 *  - The workspace belongs to the call until the work the call enqueued on
 *    `stream` has completed.  Two calls in flight at the same time -- on two
 *    streams, or from two host threads -- must not share one; calls that follow
 *    each other on one stream may.
 *  - A call that returns 0 writes every entry of every non-NULL output array:
 *    all of p_action / svf / value, `status` and `iterations` of every
 *    instance, the outputs of instances whose status is not IRLMX_OK included
 *    (an optional output that is given -- value, log_z0, svf_t, value0 -- likewise).
 *    No output entry is read before it is written: outputs may be
 *    uninitialised memory.
 *
 * Stream order, of every entry point that takes `stream` (with or without a
 * workspace; tests/test_gpu_stream_order.py holds each of them to it on a
 * non-blocking side stream, behind a device delay, with inputs that land
 * late):
 *  - Everything a call enqueues -- kernels, memsets, copies, stream-ordered
 *    allocations -- goes to `stream`, and a value the host reads back is read
 *    after a synchronise of `stream`.  Nothing goes to the default stream.
 *  - Inputs, workspace and outputs need only be valid in stream order: the
 *    work that produces an input may still be pending on `stream` when the call
 *    is made, and an input buffer may be overwritten by later work on `stream`
 *    as soon as the call has returned.  (The irlmx_mdp struct itself, and
 *    props, are host memory read during the call.)
 *  - Two calls on two streams, each with its own workspace and outputs, may be
 *    in flight together; each returns the bits it returns alone.
 *  - Whether a call may synchronise `stream` (block the host until the work
 *    queued on it, the call's own included, has run) depends on the entry point
 *    and the shape irlmx_execution_plan names.  "asynchronous" calls neither
 *    synchronise, nor allocate, nor wait for the device in any other way:
 *      fused shape of every pass                                asynchronous
 *      irlmx_backward_maxent: per sweep, DENSE streaming
 *        and DENSE GEMM (2*S - 1 sweeps, no host read)          asynchronous
 *      irlmx_backward_maxent_extended per sweep                 asynchronous
 *      the three *_horizon passes, both shapes                  asynchronous
 *      irlmx_timed.h: irlmx_value_horizon, both shapes;
 *        irlmx_rollout_horizon,
 *        irlmx_demo_log_likelihood_horizon                      asynchronous
 *      irlmx_expected_svf.h: irlmx_expected_svf_horizon,
 *        both shapes                                            asynchronous
 *      irlmx_rollout, irlmx_demo_statistics,
 *        irlmx_demo_log_likelihood, irlmx_numpy_math            asynchronous
 *      the four *_numpy_order calls: STENCIL5 and DENSE
 *        models, ELL models with props set                      asynchronous
 *        (ELL with props 0: the row-order check synchronises)
 *      irlmx_optimal_policy, irlmx_stochastic_policy,
 *        irlmx_build_icy_gridworld, irlmx_build_gridworld,
 *        irlmx_dense_to_stencil, irlmx_dense_to_rows,
 *        irlmx_dense_ell_sizes, irlmx_dense_to_ell,
 *        irlmx_dense_gemm                                       asynchronous
 *      irlmx_forward_svf, irlmx_soft_backward,
 *        irlmx_value_iteration, irlmx_policy_evaluation on
 *        the per-sweep, DENSE streaming and DENSE GEMM shapes
 *        (the host polls the done counter every chunk of
 *        sweeps)                                                may synchronise
 *      the cluster, grid and dense-grid shapes of every pass,
 *        the grid shape of irlmx_backward_maxent_extended
 *        (each launch's outcome is read on the host)            may synchronise
 *      irlmx_mdp_properties; a width-256 STENCIL5 backward
 *        or its plan with props 0                               synchronises
 */
size_t irlmx_workspace_bytes(const irlmx_mdp* mdp, int32_t op);

/*
 * Non-causal MaxEnt backward pass -- replaces the numeric core of
 * maxent.local_action_probabilities (reference src/maxent.py:119-159).
 *   reward   [B][S]     per-state reward r (the reference's `reward`)
 *   terminal [B][S]     1 for terminal states (zs[terminal] = 1, maxent.py:147)
 *   rescale  nonzero: multiply the partition vector by a power of two each sweep
 *            (ratio-preserving; keeps it finite where the reference overflows)
 *   p_action [B][S][A]  out: za / zs after exactly 2*S sweeps
 */
int irlmx_backward_maxent(const irlmx_mdp* mdp, const double* reward, const uint8_t* terminal,
                          int32_t rescale, double* p_action, int32_t* status, void* workspace,
                          size_t workspace_bytes, void* stream);

/*
 * The same backward pass with one exponent per state (no reference counterpart
 * beyond maxent.py:119-159 itself): every partition value is held as
 * m * 2^e, m a float64 in [0.5, 1) or 0 and e an int32, so the policy stays
 * finite -- and right -- where the partition vector spans more than float64's
 * exponent range and irlmx_backward_maxent, which keeps one scale per
 * instance, returns NaN rows and wrong finite rows beside them (a reward
 * contrast of 4 on a grid 256 wide is enough).  Same weights, slot order and
 * fused multiply-adds as irlmx_backward_maxent: bit-identical to it (rescale
 * != 0) wherever that pass neither underflows nor overflows.  Exactly 2*S
 * sweeps; fully asynchronous on `stream` on the fused and per-sweep shapes
 * (on the grid shape, below, the call synchronises `stream`: each launch's
 * outcome is read on the host).  Non-finite exp(reward) gives an
 * all-NaN policy for that instance; a state that cannot reach a terminal 0 / 0
 * = NaN, as in the reference.  STENCIL5 and ELL layouts, S <= 2^19;
 * IRLMX_EINVAL for DENSE.  Workspace: irlmx_workspace_bytes(mdp,
 * IRLMX_OP_BACKWARD | IRLMX_PLAN_EXTENDED_RANGE).  Three shapes, in this
 * order.  Fused: up to 4096 states, one workgroup per instance.  Grid: from
 * 8192 states on (an absolute floor, whatever IRLMX_FUSED_MAX_STATES says;
 * IRLMX_EXT_GRID_MIN_STATES moves it, tests use 0), models of at most 16
 * slots per state whose instance fits 256 workgroups of 256 threads with 1, 2
 * or 4 states per thread (S <= 2^18): one persistent launch runs all 2*S
 * sweeps of as many instances as can be co-resident, every partition value
 * exchanged per sweep as two tagged granules (mantissa, exponent); a batch
 * larger than that takes ceil(B / instances per launch) sequential launches.
 * The plan is the smallest states per thread at which these stay within
 * IRLMX_EXT_GRID_MAX_LAUNCHES (default 1: the measured break-even, DESIGN.md
 * section 4 "Extended range"; 0 switches the shape off, as IRLMX_GRID=0
 * does); at none, the call goes per sweep.  A launch whose workgroups
 * cannot all run at once, or whose exchange times out, sends the whole call
 * to the per-sweep shape (counters IRLMX_CTR_RERUN_*): same bits.  Per sweep:
 * everything else, 2*S - 1 launches (correct, and slow at config-4 size).
 */
int irlmx_backward_maxent_extended(const irlmx_mdp* mdp, const double* reward, const uint8_t* terminal,
                                   double* p_action, int32_t* status, void* workspace, size_t workspace_bytes,
                                   void* stream);

/*
 * The same backward pass in numpy's own floating-point order (no reference
 * counterpart beyond maxent.py:142-159 itself): every p[a].dot(zs) summed as
 * numpy's OpenBLAS dgemv_t sums it on a Haswell-family x86-64 host (lane
 * accumulators by column % 4, fused multiply-adds, lane and block sums), then
 * er * dot, the sequential action sum and za / zs -- so the policy is
 * bit-identical to the reference's there (oracle/blas_order.c pins the order,
 * against np.dot up to S = 4096 with one BLAS thread).  The reference's own bits
 * depend on its host: above S = 625 numpy's multi-threaded OpenBLAS moves some
 * rows to other kernels, so this is the reference run with
 * OPENBLAS_NUM_THREADS=1 there (any thread count up to 625 states).
 * No rescaling: it overflows to NaN where the reference does.
 *   exp_reward [B][S]  np.exp(reward) as the reference computes it (maxent.py:142)
 * Requires S <= 4096 and S % 4 in {0, 1} (every square grid); IRLMX_EINVAL otherwise.
 * ELL models: each row's nonzero entries in ascending column order per action
 * (irlmx_dense_to_ell's layout), checked on the device (or taken from props);
 * IRLMX_EINVAL otherwise.
 */
int irlmx_backward_maxent_numpy_order(const irlmx_mdp* mdp, const double* exp_reward,
                                      const uint8_t* terminal, double* p_action, int32_t* status,
                                      void* stream);

/*
 * Forward expected-SVF sweep -- replaces maxent.expected_svf_from_policy
 * (reference src/maxent.py:63-114): d <- p0 + sum_a P'_a^T (pi_a * d) from d = 0
 * until max|delta| <= eps, where P' has the terminal rows cleared.
 *   p_initial [B][S], terminal [B][S] (uint8), p_action [B][S][A]
 *   max_iter  <= 0: unbounded, like the reference
 *   svf [B][S] out; iterations [B] out (int64); status [B] out
 */
int irlmx_forward_svf(const irlmx_mdp* mdp, const double* p_initial, const uint8_t* terminal,
                      const double* p_action, double eps, int64_t max_iter, double* svf,
                      int64_t* iterations, int32_t* status, void* workspace,
                      size_t workspace_bytes, void* stream);

/*
 * The same forward pass in numpy's own floating-point order (no reference
 * counterpart beyond maxent.py:105-114 itself): x_a = pi[:, a] * d, every
 * P'_a^T . x_a summed as numpy's OpenBLAS dgemv_n sums it on a Haswell-family
 * x86-64 host (groups of four sources, see oracle/blas_order.c), the sequential
 * action sum, + p_initial, delta = max|d_ - d| -- so the SVF and the sweep
 * count are bit-identical to the reference's there.  One workgroup per
 * instance.  Requires S <= 4096, S % 4 in {0, 1} and (ELL) k_col <= 32.
 */
int irlmx_forward_svf_numpy_order(const irlmx_mdp* mdp, const double* p_initial, const uint8_t* terminal,
                                  const double* p_action, double eps, int64_t max_iter, double* svf,
                                  int64_t* iterations, int32_t* status, void* stream);

/*
 * MaxCausalEnt soft value iteration -- replaces
 * maxent.local_causal_action_probabilities (reference src/maxent.py:279-341).
 *   reward [B][S]; terminal_reward [B][S] = phi (-inf except 0 at terminals, or
 *   the caller's phi vector, maxent.py:313-317); discount = gamma
 *   p_action [B][S][A] out = exp(q - v); value [B][S] out = v (may be NULL)
 */
int irlmx_soft_backward(const irlmx_mdp* mdp, const double* reward, const double* terminal_reward,
                        double discount, double eps, int64_t max_iter, double* p_action,
                        double* value, int64_t* iterations, int32_t* status, void* workspace,
                        size_t workspace_bytes, void* stream);

/*
 * Value iteration -- replaces solver.value_iteration (average = 0, reference
 * src/solver.py:9-52) and solver.stochastic_value_iteration (average != 0,
 * src/solver.py:55-104).   value [B][S] out.
 */
int irlmx_value_iteration(const irlmx_mdp* mdp, const double* reward, double discount, double eps,
                          int32_t average, int64_t max_iter, double* value, int64_t* iterations,
                          int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Policy evaluation -- the value of a given stochastic policy (no reference
 * counterpart: solver.stochastic_value_iteration, src/solver.py:55-104, is the
 * uniform policy only): v <- r + gamma * sum_a pi_a * (P_a v) from v = 0
 * (solver.py:32) until max|v' - v| <= eps.  With it the expected value
 * difference p0 . (v* - v^pi) of a recovered reward is computed on the device.
 *   reward   [B][S]     the reward the policy is judged under
 *   p_action [B][S][A]  pi[s, a]; rows need not be normalised (weights, not
 *            probabilities, to the kernels): a MaxEnt policy with an exact-0 row
 *            is legal input and gives v(s) = r(s)
 *   terminal [B][S] or NULL: a state whose byte is set gets all-zero weights, so
 *            its successors contribute nothing and v(s) = r(s) bit for bit (the
 *            cleared terminal rows of maxent.py:98-99); NULL: no terminal
 *            handling, like solver.value_iteration
 *   value [B][S] out; iterations [B] out (int64); status [B] out
 * Statement order, the same in every shape (bit-identical values, sweep counts
 * and status):
 *   once per call  w[k][s] = sum_a pi[s, a] * P[s, target_k(s), a]: A fused
 *                  multiply-adds in action order from 0 (0 at terminal states)
 *   per sweep      acc = fma(w[k][s], v[target_k(s)], acc) in slot order from 0,
 *                  v'(s) = r(s) + gamma * acc: the product rounded, then the sum
 * The loop stops after the first sweep with max|v' - v| <= eps (IRLMX_OK), on a
 * NaN delta (IRLMX_NONFINITE) or at max_iter > 0 sweeps (IRLMX_MAXITER).
 * STENCIL5 and ELL layouts; IRLMX_EINVAL for DENSE and for a discount outside
 * [0, 1] (NaN included).  Models of at most 4096 states (ELL: at most 32 slots)
 * run one workgroup per instance, fully asynchronous; larger ones one launch
 * per sweep with a host poll -- there is no persistent multi-CU form of this
 * pass.  Workspace: irlmx_workspace_bytes(mdp, IRLMX_OP_POLICY_EVALUATION).
 */
int irlmx_policy_evaluation(const irlmx_mdp* mdp, const double* reward, const double* p_action,
                            const uint8_t* terminal /* may be NULL */, double discount, double eps,
                            int64_t max_iter, double* value, int64_t* iterations, int32_t* status,
                            void* workspace, size_t workspace_bytes, void* stream);

/*
 * Finite-horizon MaxEnt (no reference counterpart: the reference's passes,
 * maxent.py:63-159, are episodic): Ziebart's Algorithm 1 for a fixed number
 * of steps T = `horizon`, for models without a terminal state and for
 * demonstrations cut after T steps (irlmx_rollout's IRLMX_TRAJ_TRUNCATED).  A
 * visited state contributes its reward, the final one included (as `visits`
 * counts the final state), so with er = exp(reward), a path s_0 .. s_T has
 * weight prod_t er(s_t) P(s_t -> s_t+1 | a_t).
 *
 * irlmx_backward_maxent_horizon, for t = T-1 .. 0 from Z_T(s) = er(s):
 *   za_t(s,a) = er(s) * sum_k P[s, target_k(s), a] * Z_{t+1}(target_k(s))
 *   Z_t(s)    = sum_a za_t(s,a)       (terminal s: Z_t(s) = er(s), held: absorbing)
 *   pi_t(s,a) = za_t(s,a) / Z_t'(s)   Z_t' = the sum just formed, also at terminal states
 * Every Z is held as m * 2^e (m a float64 in [0.5, 1) or 0, e an int32, an
 * exact zero apart: irlmx_backward_maxent_extended's form).  Per state and
 * step the statement order is:
 *   1. E = the largest neighbour exponent over the slots where some action has
 *      a nonzero entry.
 *   2. Per action, acc = fma(P, aligned z, acc) in slot order, then za = er * acc
 *      rounded (aligned z = m * 2^(e - E), the shift clamped to [-1100, 0]).
 *   3. zsum = the sequential action sum.
 *   4. pi = za / zsum.
 *   5. (m, d) = frexp(zsum), e = E + d gives Z_t(s).
 * An instance with non-finite exp(r) writes NaN to every row of every step
 * (and to log_z0), and status stays IRLMX_OK, as the extended backward does;
 * 0 / 0 = NaN where no successor has weight.
 *   reward [B][S]; terminal [B][S] or NULL (no terminal state)
 *   horizon    1 .. 2^20, IRLMX_EINVAL outside: the exponent grows by less
 *              than 1,100 per step, so there is no int32 wrap
 *   p_action_t [B][T][S][A] out: pi_t, B * T * S * A * 8 bytes
 *   log_z0     [B][S] out or NULL: log Z_0(s) = fma((double)e, ln 2, log(m)),
 *              -inf for an exact zero: the log partition function of the paths
 *              from s (in a deterministic world sum_t r(s_t) - log Z_0(s_0) is
 *              a demonstration's exact log-likelihood)
 *
 * irlmx_forward_svf_horizon, for t = 0 .. T-1 from d_0 = p0 and D = p0:
 *   w           = sum_a fma(P[u -> s', a], pi_t[u][a], w)   action order from 0; 0 for terminal u
 *   d_{t+1}(s') = sum_k fma(w_k, d_t[u_k], acc)             slot order of the column form (every
 *                 slot: an off-grid STENCIL5 slot has w = 0 and u_k = s'; ELL slots as stored)
 *   D(s')       = D(s') + d_{t+1}(s')                       one rounded add per step
 *   svf [B][S] out = D; svf_t [B][T+1][S] out or NULL: the marginals d_0 .. d_T
 * status: IRLMX_NONFINITE if and only if the instance's returned svf holds a
 * non-finite entry; NaN propagates by IEEE rules in the order above (there is
 * no whole-instance poisoning rule and no convergence test).  The sweep count
 * is T.  Without terminals sum_s d_t(s) = 1 for every t, so sum D = T + 1.
 * In float64 (u = 2^-53, K_c column slots): a step rounds A times per weight
 * and K_c times per sum, so d_t is off by at most t (K_c + A) u relatively and
 * so is sum_s d_t, a sum of non-negative terms; D takes at most T rounded adds
 * of non-negative terms, T u more.  To first order every one of the T + 1
 * marginals in D is off by less than (T + 1) (K_c + A + 2) u relatively, and
 * with them |sum D - (T + 1)| / (T + 1) <= (T + 1) (K_c + A + 2) 2^-53: the
 * worst case.
 *
 * Both: STENCIL5 and ELL layouts, IRLMX_EINVAL for DENSE.  Two shapes, the
 * same bits in both: models of at most 1024 states whose slots fit the fused
 * planner (irlmx_execution_plan) run one workgroup per instance for all T
 * steps, and so do models of up to 4096 states once the batch holds a
 * workgroup for every CU (IRLMX_HORIZON_FUSED_BATCH moves that count: below
 * it one launch per step is faster, DESIGN.md section 4 "Finite horizon");
 * everything else one launch per step.  Both are fully asynchronous on
 * `stream`.  Workspace: irlmx_workspace_bytes(mdp, IRLMX_OP_BACKWARD_HORIZON /
 * IRLMX_OP_FORWARD_HORIZON), independent of T.
 */
int irlmx_backward_maxent_horizon(const irlmx_mdp* mdp, const double* reward, const uint8_t* terminal /* may be NULL */,
                                  int32_t horizon, double* p_action_t /* [B][T][S][A] */,
                                  double* log_z0 /* [B][S], may be NULL */, int32_t* status, void* workspace,
                                  size_t workspace_bytes, void* stream);
int irlmx_forward_svf_horizon(const irlmx_mdp* mdp, const double* p_initial, const uint8_t* terminal /* may be NULL */,
                              const double* p_action_t, int32_t horizon, double* svf /* [B][S] */,
                              double* svf_t /* [B][T+1][S], may be NULL */, int32_t* status, void* workspace,
                              size_t workspace_bytes, void* stream);

/*
 * Finite-horizon MaxCausalEnt (no reference counterpart beyond the statements
 * of maxent.py:279-341): the soft Bellman recursion for a fixed number of steps
 * T = `horizon` -- the causal model of irlmx_soft_backward for worlds without a
 * terminal state and demonstrations cut after T steps.  It needs no terminal
 * set and no discount below 1, and there is no convergence test: the sweep
 * count is T.  Its pi_t has the [B][T][S][A] layout irlmx_forward_svf_horizon
 * consumes; with p0 . V_0 as the objective, d(p0 . V_0) / d r(s) is that pass's
 * svf under pi_t, so e_features - svf is the exact likelihood gradient.
 *
 * From V_T(s) = r(s), for t = T-1 ... 0, per state s:
 *   1. Per action a in index order, accumulate
 *      acc = fma(P[s, target_k(s), a], V_{t+1}(target_k(s)), acc) from 0 over
 *      every stored slot in slot order.  Then q_a = r(s) + discount * acc, with
 *      the product rounded before the sum (as irlmx_soft_backward).
 *   2. v = q_0, then v = softmax2(v, q_a) for a = 1 ... A-1: max + log(1 +
 *      exp(min - max)) with numpy's exp / log (maxent.py:260-276, 331-333).
 *      There is no phi start: starting from q_0 equals the reference's
 *      softmax(-inf, q_0) exactly, without its -inf - -inf.
 *   3. pi_t(s, a) = np_exp(q_a - v) (maxent.py:341).  With A = 1 every row is 1.0.
 *   4. V_t(s) = v.  For a terminal s, V_t(s) = r(s) is held, so the state is
 *      absorbing; pi_t at a terminal s is still the row of step 3 (as the
 *      non-causal pass's terminal row divides by the sum just formed).
 * Conventions are those of irlmx_backward_maxent_horizon: a visited state
 * contributes its reward, the final one included, and with discount = 1 on a
 * deterministic table the two models coincide (V_0 = log Z_0).
 *   reward [B][S]; terminal [B][S] or NULL (no terminal state)
 *   discount   in [0, 1]; NaN or a value outside: IRLMX_EINVAL
 *   horizon    1 .. 2^20, IRLMX_EINVAL outside
 *   p_action_t [B][T][S][A] out: pi_t, B * T * S * A * 8 bytes
 *   value0     [B][S] out or NULL: V_0
 * Non-finite values spread by IEEE rules in the order above; a zero-weight ELL
 * padding slot that points at a non-finite V is included (0 * inf = NaN).
 * status: IRLMX_NONFINITE if and only if the instance's V_0 holds a non-finite
 * entry, whether or not value0 is given; a non-finite r(s) always reaches
 * V_0(s).  With finite rewards everything stays finite: the pass works in the
 * log domain, so there is no extended-range form.
 *
 * STENCIL5 and ELL layouts, IRLMX_EINVAL for DENSE.  Two shapes, the same bits
 * in both, routed as the horizon backward is: one workgroup per instance for
 * all T steps (V ping-pongs in LDS, one barrier per step) where the model's
 * (states per thread, slot class) pair is instantiated -- up to 1024 states,
 * and up to 4096 once the batch holds a workgroup for every CU
 * (IRLMX_HORIZON_FUSED_BATCH moves that count) -- else one launch per step
 * with V double-buffered in the workspace (T + 1 launches, no host poll).
 * Fully asynchronous on `stream`.  Workspace: irlmx_workspace_bytes(mdp,
 * IRLMX_OP_SOFT_BACKWARD_HORIZON), independent of T.
 */
int irlmx_soft_backward_horizon(const irlmx_mdp* mdp, const double* reward, const uint8_t* terminal /* may be NULL */,
                                double discount, int32_t horizon, double* p_action_t /* [B][T][S][A] */,
                                double* value0 /* [B][S], may be NULL */, int32_t* status, void* workspace,
                                size_t workspace_bytes, void* stream);

/*
 * Demonstrations on the device (no reference counterpart beyond the statistics
 * of maxent.py:15-60: the reference samples with numpy's global generator,
 * trajectory.py:52-128, which the trajectory.py drop-in follows draw for draw).
 * One thread per trajectory; all three calls are fully asynchronous on
 * `stream` and need no workspace.  STENCIL5 and ELL layouts; IRLMX_EINVAL for
 * DENSE.  Per-trajectory outcome codes (written to traj_status):
 */
#define IRLMX_TRAJ_OK 0         /* reached a terminal state */
#define IRLMX_TRAJ_TRUNCATED 1  /* still alive after max_len steps */
#define IRLMX_TRAJ_BAD_POLICY 2 /* a policy row with no positive finite total, or a negative or NaN entry */
#define IRLMX_TRAJ_BAD_TABLE 3  /* the same for the transition row of the drawn action, or the drawn ELL
                                   target outside [0, S) */
#define IRLMX_TRAJ_BAD_INDEX 4  /* a start state outside [0, S); in the two calls on stored trajectories a
                                   stored state or action out of range or a length outside [0, stride - 1] */
/*
 * The index checks behind codes 3 and 4 run in every build (not only with
 * IRLMX_DEVICE_CHECKS): a bad index ends its trajectory with the code and is
 * never used as an index.
 *
 * irlmx_rollout samples n_traj trajectories per instance from explicit start
 * states under the policy p_action:
 *   p_action [B][S][A]  weights of the actions per state (rows need not be
 *            normalised: a MaxEnt policy is not, exactly)
 *   terminal [B][S]     a trajectory ends when it enters a state whose byte is set
 *   start    [B][N]     start state of each trajectory
 *   seed     [B]        one 64-bit seed per instance
 *   max_len  1 .. 2^20  step cap per trajectory: the upper limit keeps a kernel
 *            from running unboundedly on a shared GPU (a policy that never
 *            reaches a terminal is legal input); IRLMX_EINVAL outside
 *   visits [B][S] out   visits of each state, the final state of every
 *            trajectory included (maxent.py:15-39 with identity features, times
 *            n_traj); starts [B][S] out: trajectories starting in each state
 *            (maxent.py:42-60, times n_traj).  Both zeroed by the call itself.
 *   lengths [B][N] out  steps taken; traj_status [B][N] out
 *   states [B][N][max_len + 1], actions [B][N][max_len]  out, both NULL or
 *            both set: states 0..length and actions 0..length - 1 of each
 *            trajectory; entries beyond are not written (nothing at all for a
 *            bad start state)
 * Random numbers: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl
 * constants 0x9E3779B9, 0xBB67AE85), one block per step with counter
 * (t, n, 0, 0) -- step t of trajectory n -- and key (low, high word of
 * seed[b]).  The stream of a trajectory therefore depends on its instance's
 * seed, n and t only: not on B, the instance's place in the batch or the launch.
 * From the output words x0..x3, u_action = ((x1 >> 5) * 2^26 + (x0 >> 6)) * 2^-53
 * and u_next likewise from x3, x2.  Both draws use one rule, pick(u, w): total =
 * the sum of w in index order; the row is invalid (codes 2 / 3) if an entry is
 * negative or NaN or total is not positive and finite; the result is the first
 * j with u * total < w_0 + .. + w_j, or the last j with w_j > 0 when the product
 * rounded up to total.  A slot of weight 0 is never drawn.  Per step in a
 * non-terminal state s: count s, a = pick(u_action, p_action[b][s][:]),
 * k = pick(u_next, P[s, target_k(s), a] over the K slots), s' = target_k(s).
 * However a trajectory stops, its current state is counted once more as its
 * final state; a terminal start state gives length 0.  Integer counts and a
 * counter-based generator: the results are the same bits on every run.
 *
 * irlmx_demo_statistics recomputes visits and starts (zeroed by the call) from
 * stored trajectories: states [B][N][stride] (entries 0..length read), lengths
 * [B][N].  A trajectory with code 4 counts nothing.
 *
 * irlmx_demo_log_likelihood: ll_traj[b][n] = sum over t < length of
 * log p_action[b][s_t][a_t], numpy's log (irlmx_numpy_math), added in step order;
 * log 0 = -inf is a legal result.  actions [B][N][stride - 1].  ll[b] = the sum of
 * ll_traj[b][:] in index order; a trajectory with code 4 has ll_traj = NaN.
 */
int irlmx_rollout(const irlmx_mdp* mdp, const double* p_action, const uint8_t* terminal, const int32_t* start,
                  const uint64_t* seed, int32_t n_traj, int32_t max_len, int64_t* visits, int64_t* starts,
                  int32_t* lengths, int32_t* traj_status, int32_t* states /* may be NULL */,
                  int32_t* actions /* may be NULL */, void* stream);
int irlmx_demo_statistics(int32_t n_states, int32_t batch, int32_t n_traj, int32_t stride /* states row length */,
                          const int32_t* states, const int32_t* lengths, int64_t* visits, int64_t* starts,
                          int32_t* traj_status, void* stream);
int irlmx_demo_log_likelihood(int32_t n_states, int32_t n_actions, int32_t batch, int32_t n_traj, int32_t stride,
                              const double* p_action, const int32_t* states, const int32_t* actions,
                              const int32_t* lengths, double* ll_traj, double* ll, int32_t* traj_status, void* stream);

/*
 * Soft value iteration and value iteration in numpy's own floating-point order
 * (no reference counterpart beyond maxent.py:326-341 / solver.py:40-50, 95-100
 * themselves): every p[a].dot(v) / p[a] @ v summed as numpy's OpenBLAS dgemv_t
 * sums it on a Haswell-family x86-64 host (see
 * irlmx_backward_maxent_numpy_order), then the same statements as
 * irlmx_soft_backward / irlmx_value_iteration.  Value iteration has no
 * transcendental function: its values and sweep counts are bit-identical to the
 * reference's there.  Soft VI's exp / log are the device's (numpy's SIMD exp /
 * log may differ in the last bit): its dot products, and with them the
 * mirror-symmetric ties of its policy, follow numpy.  No workspace.  The same
 * single-thread caveat above S = 625 and ELL slot-order check as
 * irlmx_backward_maxent_numpy_order.
 * Requires S <= 4096 and S % 4 in {0, 1}; IRLMX_EINVAL otherwise.
 */
int irlmx_soft_backward_numpy_order(const irlmx_mdp* mdp, const double* reward, const double* terminal_reward,
                                    double discount, double eps, int64_t max_iter, double* p_action,
                                    double* value, int64_t* iterations, int32_t* status, void* stream);
int irlmx_value_iteration_numpy_order(const irlmx_mdp* mdp, const double* reward, double discount, double eps,
                                      int32_t average, int64_t max_iter, double* value, int64_t* iterations,
                                      int32_t* status, void* stream);

/*
 * Execution plan a call of `op` (IRLMX_OP_*) on this model would run, without
 * running it (diagnostics and tests: the bench and the parity tests assert that
 * they exercise the same kernel instantiation).  No reference counterpart.
 * Writes plan[IRLMX_PLAN_LEN]:
 *   [0] shape (IRLMX_SHAPE_*)   [1] R rows per tile   [2] G ghost rows
 *   [3] C tiles per instance   [4] instances per launch   [5] states per lane
 *   [6] in-tile layout (0 per state, 1 pair rows, 2 column pairs, 3 column quads,
 *       4 column quads with compact weights: the backward at width 256, for
 *       tables with IRLMX_PROP_COMPACT -- without props, a width-256 STENCIL5
 *       backward plan checks the table on the device and synchronises)
 *   [7] threads per workgroup  [8] sequential launches   [9] LDS bytes
 * Cluster fields are 0 for the other shapes.  Depends on the current device.
 * IRLMX_OP_POLICY_EVALUATION plans the fused shape ([5], [7], [8] = 1, [9]) or
 * the per-sweep one ([5] = 1, [7]; [8] = 0: its launch count is the sweep
 * count); IRLMX_EINVAL for DENSE, here and 0 from irlmx_workspace_bytes.
 * IRLMX_OP_BACKWARD_HORIZON / IRLMX_OP_FORWARD_HORIZON likewise: fused ([5],
 * [7], [8] = 1, [9]) or per sweep ([5] = 1, [7]; [8] = 0: its launch count is
 * the horizon); IRLMX_EINVAL for DENSE.  IRLMX_OP_SOFT_BACKWARD_HORIZON uses
 * the same fields the same way (per sweep its launch count is the horizon + 1).
 * A backward plan assumes rescale != 0 unless op carries IRLMX_PLAN_NO_RESCALE.
 */
#define IRLMX_PLAN_LEN 10
#define IRLMX_SHAPE_FUSED 0   /* one workgroup per instance for the whole loop */
#define IRLMX_SHAPE_CLUSTER 1 /* persistent row tiles with halo exchanges */
#define IRLMX_SHAPE_SWEEP 2   /* one launch per sweep */
#define IRLMX_SHAPE_DENSE 3   /* DENSE layout: one launch per sweep, matrix rows streamed per instance */
#define IRLMX_SHAPE_DENSE_GEMM 4 /* DENSE, shared table: the backward sweep as one dgemm over all instances */
#define IRLMX_SHAPE_GRID 5    /* soft VI / VI on large grids: one persistent launch, values exchanged per sweep
                                 ([3] = workgroups per instance) */
#define IRLMX_SHAPE_DENSE_GRID 6 /* DENSE forward / backward / soft VI / VI: one persistent launch, [1] states
                                    per workgroup whose matrix rows sit in registers, [5] columns per thread,
                                    [3] workgroups per instance, [2] 1 = each instance on one XCD, [6] soft VI /
                                    VI: actions compiled per state; values exchanged per sweep */
#define IRLMX_PLAN_NO_RESCALE 0x100 /* OR into op (IRLMX_OP_BACKWARD only): the plan of a rescale = 0 call, which
                                      never takes the cluster shape (its overflow bookkeeping is per sweep) */
#define IRLMX_PLAN_EXTENDED_RANGE 0x200 /* OR into op (IRLMX_OP_BACKWARD only, here and in irlmx_workspace_bytes):
                                          irlmx_backward_maxent_extended -- shape fused or sweep, [5], [7], [8]
                                          (sweep: the 2*S - 1 sweep launches) and [9]; or grid: [2] 1 = each
                                          instance on one XCD, [3] workgroups per instance, [4] instances per
                                          launch, [5], [7] = 256, [8] sequential launches */
int irlmx_execution_plan(const irlmx_mdp* mdp, int32_t op, int64_t* plan);

/*
 * Policy extraction from a value function -- replaces
 * solver.optimal_policy_from_value (src/solver.py:107-124: argmax over the
 * values of the intended successors, first index on ties and NaN counted as
 * the maximum, as np.argmax) and solver.stochastic_policy_from_value
 * (src/solver.py:155-181: weighted successor values normalised per state).
 *   successor [S][A] (int32, shared by all instances): intended next state of
 *     (s, a), i.e. world.state_index_transition(s, a) (gridworld.py:105-122)
 *   value [B][S] -> policy [B][S] (int64)
 *   weighted_value [B][S] = w(value) elementwise -> p_policy [B][S][A]
 */
int irlmx_optimal_policy(const int32_t* successor, int32_t n_states, int32_t n_actions, int32_t batch,
                         const double* value, int64_t* policy, void* stream);
int irlmx_stochastic_policy(const int32_t* successor, int32_t n_states, int32_t n_actions, int32_t batch,
                            const double* weighted_value, double* p_policy, void* stream);

/*
 * World builders -- replace the O(S^2 A) Python constructors of
 * gridworld.IcyGridWorld / gridworld.GridWorld (src/gridworld.py:124-248),
 * emitting the STENCIL5 row form directly, bit-identical values.
 *   p_slip [B] (device), row_val [B][4][5][S] out (device)
 */
int irlmx_build_icy_gridworld(int32_t size, const double* p_slip, int32_t batch, double* row_val,
                              void* stream);
int irlmx_build_gridworld(int32_t size, int32_t batch, double* row_val, void* stream);

/*
 * Dense [S][S][A] float64 table (device) -> STENCIL5 row form on a width x height
 * grid.  *off_stencil (device int32) is set nonzero when some nonzero entry is
 * not a stencil neighbour (the table then needs the ELL layout).
 */
int irlmx_dense_to_stencil(const double* dense, int32_t width, int32_t height, int32_t n_actions,
                           double* row_val, int32_t* off_stencil, void* stream);

/*
 * Dense [S][S][A] float64 table (device, the reference's p_transition layout)
 * -> DENSE layout: p_rows [A][S][S] (P[s, t, a] at [a][s][t]) and m_rows [S][S]
 * (sum over actions in action order).  Replaces the per-call slice copies of
 * maxent.py:98-102, 143, 320 and solver.py:37 for genuinely dense models.
 */
int irlmx_dense_to_rows(const double* dense, int32_t n_states, int32_t n_actions, double* p_rows, double* m_rows,
                        void* stream);

/*
 * Dense [S][S][A] float64 table (device) -> ELL layout (any sparsity), in two
 * calls.  irlmx_dense_ell_sizes writes k_out[0] = max targets per source state
 * (union over actions) and k_out[1] = max sources per target state (device
 * int32[2]; col_count = device int32[S] scratch); the caller sizes the arrays
 * with max(1, k) and calls irlmx_dense_to_ell:
 *   row_idx [k_row][S], row_val [A][k_row][S]  targets of each state, ascending
 *   col_idx [k_col][S], col_val [A][k_col][S]  sources of each state, ascending
 * unused slots point at the state itself with value 0.  Replaces the host
 * conversion of the reference's dense p_transition (maxent.py:98-102, 143) for
 * non-grid models.
 */
int irlmx_dense_ell_sizes(const double* dense, int32_t n_states, int32_t n_actions, int32_t* k_out,
                          int32_t* col_count, void* stream);
int irlmx_dense_to_ell(const double* dense, int32_t n_states, int32_t n_actions, int32_t k_row, int32_t k_col,
                       int32_t* row_idx, double* row_val, int32_t* col_idx, double* col_val, void* stream);

/*
 * Batched fp64 GEMM on the matrix cores (v_mfma_f64_16x16x4_f64): c[b][r] =
 * sum_t m[r][t] * z[b][t] for m [rows][n], z [batch][n], c [batch][rows], all
 * row-major device arrays.  This is the P . [v_1 .. v_B] contraction of a dense
 * table shared by B instances (maxent.py:155, 329; solver.py:44), which the
 * DENSE-layout passes run through it (plan shape IRLMX_SHAPE_DENSE_GEMM); any n
 * (the K tail is zero-padded).  irlmx_dense_gemm_variant reports the kernel
 * variant such a call launches: variant[4] = {row tiles of 16 per workgroup,
 * instance tiles of 16, waves per workgroup, 16-byte loads (n even)}.
 */
int irlmx_dense_gemm(const double* m, const double* z, double* c, int32_t rows, int32_t n, int32_t batch,
                     void* stream);
int irlmx_dense_gemm_variant(int32_t rows, int32_t n, int32_t batch, int32_t* variant);

#ifdef __cplusplus
}
#endif

#endif /* IRLMX_H */

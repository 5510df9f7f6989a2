/*
 * irlmx_timed.h -- what consumes a time-indexed policy pi_t [B][T][S][A], the
 * output of irlmx_backward_maxent_horizon and irlmx_soft_backward_horizon
 * (irlmx.h): rollouts of exactly T steps, the log-likelihood of stored
 * demonstrations and the finite-horizon value of a reward.  They are the twins
 * of irlmx_rollout, irlmx_demo_log_likelihood and irlmx_policy_evaluation /
 * irlmx_value_iteration for policies that change with the step.
 *
 * Everything irlmx.h states for its own entry points holds here: return codes
 * and irlmx_last_error, the irlmx_mdp struct, the workspace call contract
 * (beside irlmx_workspace_bytes) and the stream order.  In the table of
 * irlmx.h's stream-order comment the three calls below read "asynchronous, both
 * shapes": none synchronises, allocates or waits for the device.  The entry
 * points live in this header of their own, so the function list of irlmx.h
 * (ABI version 1) stays as it is; tests/test_abi_timed.py holds this header to
 * the coverage rules tests/test_abi.py and tests/test_call_contract_host.py
 * hold irlmx.h to.
 *
 * STENCIL5 and ELL layouts; IRLMX_EINVAL for DENSE, as the other finite-horizon
 * passes.  `horizon` = T lies in 1 .. 2^20, IRLMX_EINVAL outside.  `terminal`
 * [B][S] may be NULL: no terminal state.
 */
#ifndef IRLMX_TIMED_H
#define IRLMX_TIMED_H

#include "irlmx.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * irlmx_rollout_horizon samples n_traj trajectories of at most T = `horizon`
 * steps per instance: it is irlmx_rollout with max_len = T whose step t draws
 * its action from pi_t[b][t][s][:] instead of p_action[b][s][:].
 *   p_action_t [B][T][S][A]  weights of the actions per step and state (rows
 *            need not be normalised)
 *   terminal [B][S] or NULL  a trajectory ends when it enters a state whose
 *            byte is set; NULL: no state ends a trajectory
 *   start [B][N], seed [B], n_traj, visits / starts [B][S] (both zeroed by the
 *            call itself), lengths / traj_status [B][N]: as irlmx_rollout's
 *   states [B][N][T + 1], actions [B][N][T]  out, both NULL or both set:
 *            states 0..length and actions 0..length - 1 of each trajectory;
 *            entries beyond are not written (nothing at all for a bad start state)
 * The generator is irlmx_rollout's: Philox4x32-10, one block per step with
 * counter (t, n, 0, 0) and key (low, high word of seed[b]); u_action from the
 * output words x1, x0 and u_next from x3, x2; both draws by pick(u, w).  Per
 * step t in a non-terminal state s: count s, a = pick(u_action,
 * p_action_t[b][t][s][:]), k = pick(u_next, P[s, target_k(s), a] over the K
 * slots), s' = target_k(s).  The index guards and the outcome codes
 * IRLMX_TRAJ_* are irlmx_rollout's, and however a trajectory stops, its
 * current state is counted once more as its final state; a terminal start
 * state gives length 0.  IRLMX_TRAJ_TRUNCATED keeps its meaning, "still alive
 * after T steps": it is the NORMAL outcome here -- without a terminal state
 * every sound trajectory ends with it, at length T, and counts T + 1 visits.
 * With a stationary policy repeated T times every output equals
 * irlmx_rollout's at max_len = T bit for bit.  One thread per trajectory,
 * 256-thread workgroups, no workspace; fully asynchronous on `stream`.
 */
int irlmx_rollout_horizon(const irlmx_mdp* mdp, const double* p_action_t, const uint8_t* terminal /* may be NULL */,
                          const int32_t* start, const uint64_t* seed, int32_t n_traj, int32_t horizon,
                          int64_t* visits, int64_t* starts, int32_t* lengths, int32_t* traj_status,
                          int32_t* states /* may be NULL */, int32_t* actions /* may be NULL */, void* stream);

/*
 * irlmx_demo_log_likelihood_horizon: the log-likelihood of stored trajectories
 * (states [B][N][stride], actions [B][N][stride - 1], lengths [B][N]: the
 * layout irlmx_rollout_horizon writes with stride = T + 1, and any other
 * stride >= 1) under p_action_t [B][T][S][A]:
 *   ll_traj[b][n] = sum over t < length of np_log(p_action_t[b][t][s_t][a_t]),
 *                   numpy's log (irlmx_numpy_math), one rounded add per step
 *                   from 0 in step order
 *   ll[b]         = the sequential sum of ll_traj[b][:] in index order
 * log 0 = -inf is a legal result.  A trajectory whose length lies outside
 * [0, min(stride - 1, horizon)] -- a length above `horizon` has no policy row
 * to read -- or with one of states 0..length outside [0, S) or of actions
 * 0..length - 1 outside [0, A) gets IRLMX_TRAJ_BAD_INDEX (4) and ll_traj = NaN;
 * every other trajectory gets IRLMX_TRAJ_OK.  The guards run in every build.
 * With a stationary policy repeated T times the outputs equal
 * irlmx_demo_log_likelihood's bit for bit.  No workspace; fully asynchronous.
 *
 * Telescoping.  On a deterministic table the non-causal pi_t of
 * irlmx_backward_maxent_horizon is er(s) Z_{t+1}(s') / Z_t(s), so a full-length
 * trajectory has sum_{t<T} log pi_t(s_t, a_t) = sum_{t<=T} r(s_t) - log Z_0(s_0)
 * exactly.  In float64 (u = 2^-53), to first order: each of the T ratios
 * carries at most K + A + 2 roundings (K in the slot sum, the product with
 * er, A in the action sum, the division; er = np_exp(r) among them), which its
 * log turns into an absolute error of (K + A + 2) u; each log rounds once more,
 * within 2 u |log pi_t| (numpy's log is within one unit in the last place); each
 * of the T adds rounds within u of the partial sum; and log_z0 = fma(e, ln 2,
 * log m) is within 4 u |log_z0|.  Hence
 *   |ll_traj - (sum_{t<=T} r(s_t) - log_z0(s_0))|
 *     <= u (T (K + A + 2) + 2 sum_t |log pi_t(s_t, a_t)| + T max_t |partial sum| + 4 |log_z0(s_0)|),
 * the right-hand side's own sum taken in extended precision: the worst case.
 * The first and the third term are the two parts that belong to the sum of
 * logs itself.  The second and the fourth are there because the statement
 * compares two float64 results, not one against the truth: np_log rounds its
 * own result (a faithful log of an inexact ratio is still off by its last
 * place), and log_z0 on the right-hand side is the device's rounded value, not
 * log Z_0.  Without them the inequality would not be a bound where |log pi_t|
 * or |log_z0| is large (a reward of -700 gives |log_z0| of several thousand:
 * its last place alone is 1e-12); on the tested input they add about 1 % to it.
 */
int irlmx_demo_log_likelihood_horizon(int32_t n_states, int32_t n_actions, int32_t batch, int32_t n_traj,
                                      int32_t stride, int32_t horizon, const double* p_action_t,
                                      const int32_t* states, const int32_t* actions, const int32_t* lengths,
                                      double* ll_traj, double* ll, int32_t* traj_status, void* stream);

/*
 * irlmx_value_horizon: the finite-horizon Bellman recursion of `reward` under a
 * time-indexed policy, or (p_action_t NULL) under the best action of every
 * step.  Conventions are those of irlmx_soft_backward_horizon: a visited state
 * contributes its reward, the final one included, and a terminal state is
 * absorbing.
 *
 * From v_T(s) = r(s), for t = T-1 ... 0, per state s:
 *   1. Per action a in index order, accumulate
 *      acc_a = fma(P[s, target_k(s), a], v_{t+1}(target_k(s)), acc_a) from 0
 *      over every stored slot in slot order.
 *   2. Combine the actions.
 *      With a policy: e = fma(pi_t(s, a), acc_a, e) from 0 in action order.  The
 *      weights are not folded into the table (they change every step), and
 *      the rows need not be normalised.
 *      With p_action_t NULL, the optimal value: q_a = r(s) + discount * acc_a,
 *      the product rounded before the sum; v = q_0, then for a = 1 ... A-1 v
 *      stays if v is NaN or q_a <= v and becomes q_a otherwise
 *      (irlmx_value_iteration's rule: a NaN q_a is taken, and then stays).
 *   3. With a policy v_t(s) = r(s) + discount * e, the product rounded before
 *      the sum.  For a terminal s, v_t(s) = r(s) is held in either form.
 *   reward [B][S]; terminal [B][S] or NULL
 *   p_action_t [B][T][S][A] or NULL (the optimal value)
 *   discount   in [0, 1]; NaN or a value outside: IRLMX_EINVAL
 *   horizon    1 .. 2^20, IRLMX_EINVAL outside
 *   value0     [B][S] out: v_0
 *   value_t    [B][T+1][S] out or NULL: v_0 .. v_T, every entry written, v_T = r
 *              included
 * Non-finite values spread by IEEE rules in the order above; a zero-weight slot
 * that points at a non-finite v is included (0 * inf = NaN).  status:
 * IRLMX_NONFINITE if and only if the instance's value0 holds a non-finite entry,
 * else IRLMX_OK.
 *
 * In float64 (u = 2^-53), to first order: a step rounds K times per slot sum,
 * A times in the action sum (or not at all in the maximum, which is
 * 1-Lipschitz), once in the product with the discount and once in the sum with
 * r, each relative to the sum of the absolute values of its terms.  With w_t
 * the same recursion on |r| (the majorant: |v_t| <= w_t <= (T + 1 - t) max|r|
 * for rows that sum to at most 1),
 *   |v_0(s) - exact| <= T (K + A + 2) u w_0(s)
 * and for a distribution p0: |p0 . v_0 - exact| <= T (K + A + 2) u (T + 1) max|r|.
 * Duality at discount 1: p0 . v_0 = D . r with D irlmx_forward_svf_horizon's svf
 * under the same pi_t, whose marginals are each within (T + 1) (K_c + A + 2) u
 * relatively (irlmx.h); so the two sides, each dotted in extended precision,
 * differ by at most
 *   ((T + 1) (K_c + A + 2) + T (K + A + 2)) u (T + 1) max|r|:
 * the worst case.
 *
 * Two shapes, the same bits in both, routed exactly as irlmx_soft_backward_horizon
 * is (the same (states per thread, slot class) pairs, IRLMX_HORIZON_FUSED_BATCH):
 * one workgroup per instance for all T steps, v ping-pongs in LDS (16 * S
 * bytes), one barrier per step; else one launch per step with v double-buffered
 * in the workspace (T + 1 launches, no host poll).  Fully asynchronous on
 * `stream`.  Workspace: irlmx_workspace_bytes(mdp, IRLMX_OP_VALUE_HORIZON),
 * independent of T; irlmx_execution_plan(mdp, IRLMX_OP_VALUE_HORIZON, plan)
 * names the shape.
 */
int irlmx_value_horizon(const irlmx_mdp* mdp, const double* reward, const uint8_t* terminal /* may be NULL */,
                        const double* p_action_t /* [B][T][S][A], may be NULL */, double discount, int32_t horizon,
                        double* value0 /* [B][S] */, double* value_t /* [B][T+1][S], may be NULL */, int32_t* status,
                        void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* IRLMX_TIMED_H */

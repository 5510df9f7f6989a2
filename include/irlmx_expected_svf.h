/*
 * irlmx_expected_svf.h -- the finite-horizon expected state visitation in one
 * call, from the reward to svf, for both finite-horizon models of irlmx.h:
 * what irlmx_backward_maxent_horizon (or irlmx_soft_backward_horizon) followed
 * by irlmx_forward_svf_horizon computes, without the time-indexed policy pi_t
 * [B][T][S][A] between them.  A gradient step needs svf and, for the objective,
 * log_z0 or V_0; it never reads pi_t, and that tensor (B * T * S * A * 8 bytes)
 * is what limits the horizon of the two-call path.  The memory here grows like
 * sqrt(T) * S.
 *
 * Everything irlmx.h states for its own entry points holds here: return codes
 * and irlmx_last_error, the irlmx_mdp struct, the workspace call contract and
 * the stream order.  In the table of irlmx.h's stream-order comment the call
 * below reads "asynchronous, both shapes": it never synchronises, allocates or
 * waits for the device, and its launch count is fixed by T and C.  The entry
 * points live in a header of their own, so the function lists of irlmx.h (ABI
 * version 1) and irlmx_timed.h stay as they are.  No op code and no counter is
 * added: irlmx_workspace_bytes and irlmx_execution_plan cannot express a size
 * that depends on T, so this call has a size query and a plan query of its own.
 *
 * STENCIL5 and ELL layouts (an ELL model with its column form); IRLMX_EINVAL
 * for DENSE, as the other finite-horizon passes.  Error texts are prefixed
 * "expected_svf_horizon: ".
 */
#ifndef IRLMX_EXPECTED_SVF_H
#define IRLMX_EXPECTED_SVF_H

#include "irlmx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IRLMX_HORIZON_MODEL_MAXENT 0   /* irlmx_backward_maxent_horizon's recursion */
#define IRLMX_HORIZON_MODEL_CAUSAL 1   /* irlmx_soft_backward_horizon's recursion   */

/*
 * irlmx_expected_svf_horizon.
 *   model      IRLMX_HORIZON_MODEL_MAXENT or _CAUSAL; anything else: IRLMX_EINVAL
 *   reward     [B][S]
 *   terminal   [B][S] or NULL: absorbing states, as in the two passes
 *   p_initial  [B][S]
 *   discount   CAUSAL: in [0, 1], NaN or a value outside: IRLMX_EINVAL.
 *              MAXENT: exactly 1.0, anything else: IRLMX_EINVAL
 *   horizon    T in 1 .. 2^20, IRLMX_EINVAL outside
 *   segment    C, the distance between kept slices.  0: C = ceil(sqrt(T)).  A
 *              value above T is T: all slices are then kept and nothing is
 *              computed twice.  Negative: IRLMX_EINVAL
 *   svf        [B][S] out: D = d_0 + .. + d_T
 *   objective0 [B][S] out or NULL: log_z0 (MAXENT), V_0 (CAUSAL)
 *   status     [B] out: IRLMX_NONFINITE if and only if either call of the
 *              two-call path would report it for that instance (svf holds a
 *              non-finite entry, or for CAUSAL V_0 does), else IRLMX_OK
 *
 * Algorithm.  X_t stands for V_t (CAUSAL), or for Z_t as a mantissa and int32
 * exponent pair (MAXENT).
 *   1. X_T is computed from the reward exactly as the existing backward does:
 *      V_T = r, Z_T = exp(r) split into mantissa and exponent.
 *   2. Pass 1 runs the existing recursion for t = T-1 down to C, values only,
 *      and keeps X_t where t is a multiple of C (and X_T).
 *   3. For each segment [lo, hi) = [jC, min((j+1)C, T)), in ascending j:
 *        recompute X_{hi-1} .. X_{lo+1} from X_hi into a segment buffer;
 *        for t = lo .. hi-1: form the policy rows of step t from X_{t+1} into
 *        one [B][S][A] buffer, run one forward step d_{t+1} from d_t under
 *        those rows, and accumulate D += d_{t+1}.
 *      Step t = 0 also yields objective0.
 *   4. Every per-state statement is the existing one, in the existing order:
 *      irlmx_soft_backward_horizon's steps 1 - 4 with its softmax2 and numpy's
 *      exp; irlmx_backward_maxent_horizon's steps 1 - 5 with its exponent
 *      alignment, frexp and division; irlmx_forward_svf_horizon's folded weight
 *      and slot sum with the rounded add into D.  MAXENT's rule for an instance
 *      with a non-finite exp(r) applies too: NaN rows at every step, log_z0
 *      NaN.  A value-only step performs the same operations on the value as the
 *      full step; it skips only what the value does not depend on (MAXENT: the
 *      division; CAUSAL: the exp of the row).
 *   5. Every output is therefore bit-identical to the two-call path for every
 *      C.  Where the two-call path gives NaN, NaN stands in the same places
 *      (payload bits are not promised).
 * The arithmetic is the backward's up to twice over (pass 1 and the segments'
 * recomputation, values only) plus its full steps once plus the forward's.
 *
 * Memory, with C' = min(C, T): ceil(T/C') kept slices, C' - 1 of the segment
 * buffer and (more than one segment) 2 of pass 1's ping-pong, each [B][S] at 12
 * bytes per state for MAXENT (a double and an int32) and 8 for CAUSAL; per
 * step also the [B][S][A] policy rows and d_t's ping and pong.  D is svf
 * itself.  irlmx_expected_svf_horizon_workspace_bytes returns at most
 *   (ceil(T/C') + C' + A + 6) * B * S * 12 + 4096
 * bytes (0 for arguments the call refuses), and the call allocates nothing
 * else.
 *
 * Two shapes, the same bits in both.  Per step: launches over all instances --
 * a value-only step, a policy-row step and a forward step; 1 + (T - C') +
 * (T - ceil(T/C')) + 2 T launches in all; counts one IRLMX_CTR_SWEEP_CALLS per
 * call.  Fused: one workgroup per instance and one state per thread runs both
 * passes and all segments in one launch, one barrier between dependent phases;
 * d_t's ping and pong and the step's [S][A] policy rows live in LDS (8 S (A + 2)
 * bytes, for CAUSAL behind the copy of numpy's tables), the slices in the
 * workspace, written and read by the same workgroup.  Fused runs where
 * irlmx_forward_svf_horizon's fused shape has one state per thread (at most
 * 1,024 states, at most 32 column slots) and that LDS fits 160 KB;
 * IRLMX_FUSED_MAX_STATES=0 forces the per-step shape, as elsewhere.
 */
int irlmx_expected_svf_horizon(const irlmx_mdp* mdp, int32_t model,
        const double* reward, const uint8_t* terminal /* may be NULL */,
        const double* p_initial, double discount, int32_t horizon, int32_t segment,
        double* svf /* [B][S] */, double* objective0 /* [B][S], may be NULL */,
        int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* The workspace of the call above with these arguments; 0 where it refuses them. */
size_t irlmx_expected_svf_horizon_workspace_bytes(const irlmx_mdp* mdp, int32_t model,
        int32_t horizon, int32_t segment);

/*
 * plan[0] shape (IRLMX_SHAPE_FUSED 0 or IRLMX_SHAPE_SWEEP 2, irlmx_execution_plan's
 * codes), [1] C as resolved, [2] slices held (kept, segment buffer, ping-pong),
 * [3] launches (0 means one per step, as counted above), [4] LDS bytes,
 * [5] workspace bytes.
 */
int irlmx_expected_svf_horizon_plan(const irlmx_mdp* mdp, int32_t model,
        int32_t horizon, int32_t segment, int64_t* plan /* [6] */);

#ifdef __cplusplus
}
#endif

#endif /* IRLMX_EXPECTED_SVF_H */

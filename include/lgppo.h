/* lgppo.h -- C ABI of the fused PPO loss head: what rsl_rl/algorithms/ppo.py:157-218 (PPO._compute_rl_loss, and the identical blocks
 * of PPO_EE / PPO_TS / PPO_DreamWaQ) and ppo_cts.py:193-267 (two policy row groups, one value group) compute behind the network forward
 * -- log-prob, ratio, surrogate, value loss, entropy, the KL of the adaptive schedule -- together with the gradient of the loss with
 * respect to the three network outputs, in one pass.  Same conventions as lgpolicy.h: plain device pointers with row strides in floats
 * and unit inner stride, the caller's HIP stream as void*; 0 on success, otherwise non-zero with the message in lgsim.h's last-error
 * call.  Tensors are float32; the partial sums are float64.
 *
 * Per policy row (A = n_actions columns; eps = clip_param):
 *   logp = sum_a [ -(a - mu)^2 / (2 sigma^2) - log sigma - 0.5 log 2 pi ],   r = exp(logp - old_log_prob)
 *   term = max(-Adv r, -Adv clamp(r, 1 - eps, 1 + eps))                       (PPO)
 *        = -(Adv r - |Adv| (r - 1)^2 / (2 eps))                               (LG_PPO_SPO)
 *   ent  = sum_a (0.5 + 0.5 log 2 pi + log sigma)
 *   kl   = sum_a [ log(sigma / old_sigma + 1e-5) + (old_sigma^2 + (old_mu - mu)^2) / (2 sigma^2) - 0.5 ]
 * per value row:
 *   term = max((v - R)^2, (v_t + clamp(v - v_t, -eps, eps) - R)^2)             (LG_PPO_CLIPPED_VALUE)
 *        = (R - v)^2                                                          (otherwise)
 * surrogate_g and kl_g are means over the rows of group g, the value loss over the value rows, the entropy over the policy rows of all
 * groups together, and
 *   loss = sum_g surrogate_g + value_loss_coef * value_loss - entropy_coef * entropy.
 * grad_mu, grad_sigma and grad_values are d loss / d mu, d sigma, d values for an upstream gradient of 1, with torch autograd's
 * conventions where branches meet: equal operands of a max share the gradient in halves (inside the clip range the halves add up to
 * the unclipped gradient), a clipped branch that wins contributes zero, clamp passes the gradient on its closed interval.
 * NaN is not silent: max and clamp are compares that pass a NaN on, so a NaN in a row reaches that row's gradients and every scalar the
 * row feeds, and nothing else.  What a row feeds: mu and sigma feed the surrogate, the KL and grad_mu / grad_sigma, sigma also the
 * entropy; actions, old_log_prob and advantages the surrogate and grad_mu / grad_sigma; old_mu and old_sigma the KL alone; values and
 * returns the value loss and grad_values, target_values too under LG_PPO_CLIPPED_VALUE and nothing otherwise (the column is not read).
 * This is torch autograd's reach of a NaN with one exception: for a NaN target value autograd returns the finite 2 (v - R) coef / B_v
 * in grad_values (max's backward hands the gradient to both operands when neither compare holds, clamp's zeroes the clipped one); here
 * that element is NaN, by the rule above.
 * Where float32 overflows (exp to inf, |Adv| infinite or near FLT_MAX) the gradients have the NaN / inf pattern of torch's float32
 * autograd: the two partials of sigma are added apart, so a row with an infinite d loss / d logp has NaN in grad_sigma (inf - inf), and
 * the 1 / B of the mean is applied to the advantage first.  sigma > 0 is the caller's contract: nothing checks it.
 */
#ifndef LGPPO_H
#define LGPPO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_PPO_MAX_ACTIONS 64
#define LG_PPO_MAX_GROUPS 2
#define LG_PPO_CLIPPED_VALUE 1u
#define LG_PPO_SPO 2u

/* The launch plan.  A workgroup is LG_PPO_THREADS lanes.  A policy row is carried by L lanes, L the power of two >= ceil(A / 4), each
 * with one quad of action columns, so a workgroup carries LG_PPO_THREADS / L policy rows, or LG_PPO_THREADS value rows, per sweep: a
 * tile.  The tiles of group 0, group 1 and the value group are numbered one behind the other; the grid is
 * min(tiles, LG_PPO_MAX_BLOCKS) workgroups, and workgroup b sweeps tiles b, b + grid, ...  Each workgroup leaves
 * LG_PPO_PARTIAL_SLOTS doubles in the partials slab, which a one-workgroup launch behind it sums in the order of the slab. */
#define LG_PPO_THREADS 256
#define LG_PPO_MAX_BLOCKS 512
#define LG_PPO_PARTIAL_SLOTS 6     /* surrogate 0, surrogate 1, entropy, kl 0, kl 1, value */

/* slots of `result` */
#define LG_PPO_R_LOSS 0
#define LG_PPO_R_SURROGATE 1       /* + group */
#define LG_PPO_R_VALUE 3
#define LG_PPO_R_ENTROPY 4
#define LG_PPO_R_KL 5              /* + group; 0 for a group without old_mu / old_sigma */
#define LG_PPO_RESULT_FLOATS 8

typedef struct LgPpoGroup {
    int32_t n_rows;                /* B_g >= 1 */
    int32_t mu_stride, sigma_stride, actions_stride, old_mu_stride, old_sigma_stride;   /* floats between rows, >= A */
    int32_t old_log_prob_stride, advantages_stride;                                      /* >= 1 */
    int32_t grad_mu_stride, grad_sigma_stride;                                           /* >= A */
    const float *mu, *sigma, *actions;       /* (B_g, A) */
    const float *old_mu, *old_sigma;         /* (B_g, A), or both NULL: no KL for this group */
    const float *old_log_prob, *advantages;  /* (B_g, 1) */
    float *grad_mu, *grad_sigma;             /* (B_g, A) out */
} LgPpoGroup;

typedef struct LgPpoLossArgs {
    int32_t n_groups;              /* 1 .. LG_PPO_MAX_GROUPS; group[n_groups ..] is not read */
    int32_t n_actions;             /* 1 .. LG_PPO_MAX_ACTIONS */
    uint32_t flags;
    int32_t n_value_rows;          /* B_v >= 1 */
    LgPpoGroup group[LG_PPO_MAX_GROUPS];
    const float *values, *returns, *target_values;   /* (B_v, 1) */
    float *grad_values;                              /* (B_v, 1) out */
    int32_t values_stride, returns_stride, target_values_stride, grad_values_stride;   /* >= 1 */
    /* doubles, as the learner holds them: the clip bounds are (float)(1 - clip_param), (float)(1 + clip_param) and +-(float)clip_param,
     * SPO divides by (float)(2 clip_param) -- what torch makes of the Python scalars */
    double clip_param;             /* > 0 */
    double value_loss_coef;
    double entropy_coef;
    double *partials;              /* workspace: lg_ppo_loss_workspace doubles, overwritten by every call */
    int64_t partials_capacity;     /* doubles available at `partials` */
    float *result;                 /* LG_PPO_RESULT_FLOATS floats out, the slots above; unnamed slots are written as 0 */
} LgPpoLossArgs;

/* Two launches on `stream`: the pass over all rows (gradients and per-workgroup partial sums), then the one-workgroup sum.  Allocates
 * nothing and never synchronises.  The sums are float64 and are combined in an order fixed by the plan, so two calls on the same inputs
 * give bit-identical results and gradients.  Refused before anything is enqueued, with a message that names the field: a null
 * descriptor, n_groups outside [1, LG_PPO_MAX_GROUPS], n_actions outside [1, LG_PPO_MAX_ACTIONS], unknown flag bits, n_rows or
 * n_value_rows below 1, a null tensor, a stride below its width, old_mu without old_sigma or the reverse, clip_param not above 0,
 * null partials or result, partials_capacity below lg_ppo_loss_workspace. */
int lg_ppo_loss(const LgPpoLossArgs *args, void *stream);

/* Doubles the partials slab needs for this descriptor: LG_PPO_PARTIAL_SLOTS per workgroup of the grid lg_ppo_loss would launch.  Launches
 * nothing and does not touch the device; reads n_groups, n_actions, the groups' n_rows and n_value_rows only.  0 with the last error set
 * on a refusal. */
int lg_ppo_loss_workspace(const LgPpoLossArgs *args);

#ifdef __cplusplus
}
#endif
#endif /* LGPPO_H */

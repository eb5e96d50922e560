/* lgtrainee.h -- C ABI of the fused learner passes of the explicit-estimator family: the two network passes of PPO_EE.update()
 * (rsl_rl/algorithms/ppo_ee.py:93-175) on ActorCriticEE (rsl_rl/modules/actor_critic_ee.py: three chains of Linear [+ ELU], a
 * Hardtanh(+-clip_actions) behind the actor).  Same contract as lgtrain.h, whose layer and chain structs are reused: plain device pointers
 * and row strides in floats, the caller's HIP stream as void*; 0 on success, otherwise non-zero with the message in lgsim.h's last-error
 * call; nothing is allocated, nothing synchronised.  Everything is float32.  Weights are read in place on every call.
 *
 * The RL pass (lg_train_ee_*), per row:   est = estimator(features);   mu = Hardtanh(actor([features | est]));   sigma = mu * 0 + std;
 *   values = critic(critic_obs).  The forward stores the concatenated actor input [features | est] (n_rows x (F + NL), dense), the actor's
 *   and the critic's hidden activations, mu, sigma and values; the estimator's hidden activations are not stored.  The backward is
 *   lgtrain.h's over the actor (whose layer 0 reads the stored concatenation) and the critic, grad_std riding along.
 * The estimator pass (lg_train_est_*):   p = estimator(features);   d = (p - labels) * mask (mask is (n_rows, 1) and broadcasts);
 *   loss = sum d^2 / (n_rows * NL);   d loss / d p = 2 d mask / (n_rows * NL), scaled in the backward by the scalar at `upstream`.
 *
 * Conventions:
 *   - The RL pass gives the estimator's parameters NO gradient and actor layer 0 computes no input gradient: the estimator chain's
 *     grad_weight / grad_bias are never read or written by lg_train_ee_backward.  In PPO_EE.update() the gradient autograd forms there is
 *     discarded unread (estimator_optimizer.zero_grad() precedes the estimator's own backward; the RL optimizer and its clip cover actor,
 *     critic and std only), so the parameter trajectory is the reference's.  There is no end-to-end estimator gradient from the RL loss.
 *   - The estimator loss follows the reference's arithmetic: the mask is a multiplication, not a select.  A non-finite prediction in a
 *     masked row still makes the loss non-finite (NaN * 0), as in torch.  The upstream scalar is read on the device: no host sync.
 *   - The loss sum is float64 in a fixed order: a row tile's workgroup adds its d^2 (each thread its elements in index order, the 256
 *     thread sums by a fixed binary tree) into one float64 partial in the workspace; the one-workgroup finalize launch adds the partials
 *     in tile order.  No float atomics, no hand-off between workgroups inside a launch: two calls on the same inputs give the same bits.
 *   - All else is as lgtrain.h: elu' from the stored output, the Hardtanh mask from the stored mu, a grad_sigma reaches grad_std only,
 *     gradients are overwritten (accumulation is autograd's job), addresses are clamped on ragged tiles, a NaN in one input row changes
 *     no other row's outputs.
 */
#ifndef LGTRAINEE_H
#define LGTRAINEE_H

#include <stdint.h>
#include "lgtrain.h"   /* LgTrainLayer, LgTrainChain, the slice rule's constants */

#ifdef __cplusplus
extern "C" {
#endif

#define LG_TRAIN_EE_CHAINS 3         /* 0 the estimator, 1 the actor, 2 the critic */
#define LG_TRAIN_EE_ESTIMATOR 0
#define LG_TRAIN_EE_ACTOR 1
#define LG_TRAIN_EE_CRITIC 2
/* The slice rule is lgtrain.h's with this in place of LG_TRAIN_TARGET_JOBS: the first layers of the EE nets have 120 to 336 tiles of 64 x 64,
 * and at 512 jobs a layer they would get 1 to 4 slices of 6144 to 24576 rows, one wave each, which the whole launch then waits for. */
#define LG_TRAIN_EE_TARGET_JOBS 2048
#define LG_TRAIN_EE_THREADS 256      /* of the estimator forward's workgroup: the leaves of the loss partial's tree */

typedef struct LgTrainEEArgs {
    int32_t n_rows;
    int32_t clip_on;
    float clip_actions;
    int32_t reserved;
    /* chain[ESTIMATOR].input: the features (n_rows, F); chain[CRITIC].input: the critic observations.  chain[ACTOR].input and in_stride are
     * NOT read: the actor's input is the concatenation in the workspace, and actor layer[0].n_in must be F + NL.  The estimator's
     * grad_weight / grad_bias are not read either. */
    LgTrainChain chain[LG_TRAIN_EE_CHAINS];
    const float *std;          /* (A) */
    float *grad_std;           /* (A), overwritten by lg_train_ee_backward */
    float *mu;                 /* (n_rows, A): written by forward, read by backward (the Hardtanh mask) */
    float *sigma;              /* (n_rows, A) */
    float *values;             /* (n_rows, V) */
    const float *grad_mu;      /* backward only, like the next two */
    const float *grad_sigma;
    const float *grad_values;
    int32_t mu_stride, sigma_stride, values_stride;
    int32_t grad_mu_stride, grad_sigma_stride, grad_values_stride;
    float *workspace;          /* LgTrainEEPlan::workspace_floats floats */
    int64_t workspace_capacity;
} LgTrainEEArgs;

typedef struct LgTrainEstArgs {
    int32_t n_rows;
    int32_t labels_stride;
    int32_t mask_stride;       /* floats between the rows of the (n_rows, 1) mask, >= 1 */
    int32_t reserved;
    LgTrainChain chain;        /* the estimator: input = the features */
    const float *labels;       /* (n_rows, NL), NL = the chain's last n_out */
    const float *mask;         /* (n_rows, 1): `terminated` */
    float *loss;               /* one float, written by lg_train_est_forward */
    const float *upstream;     /* one float on the device: d (whatever) / d loss; backward only */
    float *workspace;          /* LgTrainEEPlan::workspace_floats floats, 8-byte aligned (it holds the float64 partials) */
    int64_t workspace_capacity;
} LgTrainEstArgs;

/* The plan of either pass, a pure function of n_rows and the widths.  Offsets in floats from `workspace`; -1 / 0 where a pass has no such
 * item (the RL pass: every estimator entry, gl_off, partial_off, loss_tiles; the estimator pass: actor and critic entries, cat_off, std).
 *   cat_off       [features | est], (n_rows, F + NL) dense: actor layer 0's operand of the weight gradient
 *   h_off / g_off / p_off / slices / slice_rows: as LgTrainPlan, indexed by LG_TRAIN_EE_* chain
 *   gl_off        2 d mask / (n_rows NL), (n_rows, NL) dense, as the estimator forward leaves it; the backward scales it into g_off of
 *                 the last layer, so a forward can be differentiated more than once
 *   partial_off   loss_tiles float64 partials (an even offset) */
typedef struct LgTrainEEPlan {
    int32_t row_tile;          /* 32, 16 or 8: the largest whose two LDS activations fit 160 KB over the chains of the pass (the estimator
                                  pass keeps LG_TRAIN_EE_THREADS float64 of LDS for the loss tree besides) */
    int32_t lds_bytes;         /* dynamic LDS of the forward and input-gradient launches */
    int32_t slices[LG_TRAIN_EE_CHAINS][LG_POLICY_MAX_LAYERS];
    int32_t slice_rows[LG_TRAIN_EE_CHAINS][LG_POLICY_MAX_LAYERS];
    int32_t std_slices, std_slice_rows;
    int32_t weight_jobs;
    int32_t loss_tiles;        /* ceil(n_rows / row_tile) in the estimator pass */
    int32_t est_first_buffer;  /* RL pass: the LDS activation (0 / 1) the estimator chain starts in, so that it ends in 1 and the
                                  concatenation is formed in 0 */
    int32_t reserved;
    int64_t h_off[LG_TRAIN_EE_CHAINS][LG_POLICY_MAX_LAYERS];
    int64_t g_off[LG_TRAIN_EE_CHAINS][LG_POLICY_MAX_LAYERS];
    int64_t p_off[LG_TRAIN_EE_CHAINS][LG_POLICY_MAX_LAYERS];
    int64_t std_p_off;
    int64_t cat_off;
    int64_t gl_off;
    int64_t partial_off;
    int64_t workspace_floats;
} LgTrainEEPlan;

/* Touch no device and read no pointer: n_rows, n_layers, n_in, n_out only.  Refused: a null descriptor or plan, n_rows < 1, a layer count
 * outside [1, LG_POLICY_MAX_LAYERS], a width outside [1, LG_POLICY_MAX_WIDTH], widths that do not chain, actor layer[0].n_in other than
 * F + NL, a row tile of 8 that does not fit the LDS. */
int lg_train_ee_plan(const LgTrainEEArgs *args, LgTrainEEPlan *out);
int lg_train_est_plan(const LgTrainEstArgs *args, LgTrainEEPlan *out);

/* One launch, grid (row tiles, 2): workgroup y = 0 carries its rows through the estimator and then the actor in LDS (the concatenation is
 * formed in LDS, the features re-staged from global memory behind the estimator chain), y = 1 runs the critic.  Refused before the launch,
 * with a message that names the member: what the plan refuses, a null input (estimator, critic), weight, bias, std, mu, sigma, values or
 * workspace, a stride below its width, clip_on with clip_actions not >= 0, workspace_capacity below the plan. */
int lg_train_ee_forward(const LgTrainEEArgs *args, void *stream);

/* Three launches: input gradients, weight gradients, combine, over the actor and the critic.  Refused before any launch: what the
 * forward refuses, a null grad_weight / grad_bias of the actor or the critic, grad_std, grad_mu, grad_sigma or grad_values, a gradient
 * stride below its width. */
int lg_train_ee_backward(const LgTrainEEArgs *args, void *stream);

/* Two launches: the chain over row tiles (hidden activations, gl and one float64 partial per tile to the workspace), then the
 * one-workgroup finalize that writes *loss.  Refused before any launch: what the plan refuses, a null input, weight, bias, labels, mask,
 * loss or workspace, a workspace that is not 8-byte aligned, a stride below its width, workspace_capacity below the plan. */
int lg_train_est_forward(const LgTrainEstArgs *args, void *stream);

/* Three launches over the one chain; the input-gradient launch scales gl by *upstream.  Refused before any launch: what the forward
 * refuses but a null loss, a null upstream, grad_weight or grad_bias. */
int lg_train_est_backward(const LgTrainEstArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LGTRAINEE_H */

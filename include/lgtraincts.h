/* lgtraincts.h -- C ABI of the fused RL pass of the concurrent teacher-student family: the network pass of PPO_CTS._compute_rl_loss
 * (rsl_rl/algorithms/ppo_cts.py:193-267) on ActorCriticCTS (four chains of Linear [+ ELU]; a Hardtanh(+-clip_actions) behind the actor only
 * where the module has one).  Same contract as lgtraints.h, whose layer and chain structs (lgtrain.h's) are reused: plain device pointers and
 * row strides in floats, the caller's HIP stream as void*; 0 on success, otherwise non-zero with the message in lgsim.h's last-error call;
 * nothing is allocated, nothing synchronised.  Everything is float32.  Weights are read in place on every call.
 *
 * A mini-batch has three independent row sets: n_teacher rows of the teacher envs, n_student rows of the student envs, n_critic rows of the
 * critic (in the reference n_critic = n_teacher + n_student, another permutation of the same transitions; nothing here needs that).
 *   teacher rows:  z = privilege_encoder(privileged_obs);  mu[0] = actor([obs | z]);       sigma[0] = mu[0] * 0 + std
 *   student rows:  z = history_encoder(obs_history);       mu[1] = actor([student_obs | z]); sigma[1] = mu[1] * 0 + std
 *   critic rows:   values = critic(critic_obs)
 * (mu behind the Hardtanh under clip_on.)  The actor's stored regions ([obs | z], its hidden activations, its layer gradients) lie over one
 * row space of n_teacher + n_student rows, teacher rows first: the weight gradients see the actor as one chain of that many rows.
 *
 * The encoder step of PPO_CTS (_compute_encoder_loss, ppo_cts.py:269-278: mse_loss(history_encoder(h), privilege_encoder(p).detach()) with
 * no mask) is lgtraints.h's lg_train_enc_* with a mask of ones: (p - y) * 1.0f is exact, the scale 2 / (B Z) is the same.
 *
 * Conventions:
 *   - The RL pass never reads or writes the history encoder's gradient pointers and stores none of its activations.  rl_params of PPO_CTS
 *     are the actor, the critic, the privilege encoder and std; torch does accumulate an RL gradient in the history encoder's .grad, which
 *     history_encoder_optimizer.zero_grad() discards before the only optimizer that owns those parameters steps.  The student's latent is
 *     therefore a constant of this pass: the student rows' backward stops at actor layer 1.  This is a deliberate difference from torch's
 *     .grad; the parameters after every optimizer step are the reference's.
 *   - The encoder pass (lg_train_enc_*) leaves the privilege encoder's grad_weight / grad_bias alone, as in lgtraints.h.
 *   - The teacher rows continue through actor layer 0 for the latent columns [O, O + Z) only: they are G of the privilege encoder's last
 *     layer.  The teacher's observations and the student's [obs | z] get no gradient.  The critic's gradient reaches the critic only.
 *   - The privilege encoder's sums run over n_teacher rows, the actor's over n_teacher + n_student, the critic's over n_critic.  grad_std is
 *     the column sum of grad_sigma[0] over n_teacher rows plus that of grad_sigma[1] over n_student rows: the teacher's slice partials are
 *     added first, in slice order, then the student's.
 *   - All else is as lgtraints.h: elu' from the stored output, the Hardtanh mask from the stored mu (only where the module has one), a
 *     grad_sigma reaches grad_std only, gradients are overwritten (accumulation is autograd's job), addresses are clamped on ragged tiles to
 *     the group's own last row, a non-finite value in one input row changes no other row's outputs (no row of the other group and nothing
 *     of the critic in particular).  Plain stores only, no float atomics, no hand-off between workgroups inside a launch: two calls on the
 *     same inputs give the same bits.
 *   - The student regions start n_teacher * width floats into each region.  Where that is no multiple of 4 floats the student tiles' row
 *     copies take the scalar path: correct, slower.
 */
#ifndef LGTRAINCTS_H
#define LGTRAINCTS_H

#include <stdint.h>
#include "lgtrain.h"   /* LgTrainLayer, LgTrainChain, the slice rule's constants */
#include "lgtraints.h" /* LG_TRAIN_TS_TARGET_JOBS: the slice rule's job target here too */

#ifdef __cplusplus
extern "C" {
#endif

#define LG_TRAIN_CTS_CHAINS 4        /* LgTrainCTSArgs::chain and the plan's chain index */
#define LG_TRAIN_CTS_PRIVILEGE 0
#define LG_TRAIN_CTS_ACTOR 1
#define LG_TRAIN_CTS_CRITIC 2
#define LG_TRAIN_CTS_HISTORY 3
#define LG_TRAIN_CTS_GROUPS 2        /* mu, sigma, grad_mu, grad_sigma, their strides, the std slabs and enc_first_buffer: 0 teacher, 1 student */
#define LG_TRAIN_CTS_TEACHER 0
#define LG_TRAIN_CTS_STUDENT 1
#define LG_TRAIN_CTS_ROLES 3         /* LgTrainCTSPlan::tiles: teacher, student, critic */
#define LG_TRAIN_CTS_ROLE_CRITIC 2

typedef struct LgTrainCTSArgs {
    int32_t n_teacher;         /* each >= 1, independent of one another */
    int32_t n_student;
    int32_t n_critic;
    int32_t clip_on;           /* 0: the actor ends in its last Linear */
    float clip_actions;
    int32_t n_obs;             /* O; actor layer[0].n_in must be O + Z, Z the last n_out of both encoders */
    int32_t student_obs_stride;
    int32_t reserved;
    /* chain[PRIVILEGE].input: the teacher's privileged observations (n_teacher, P); chain[HISTORY].input: the student's observation
     * histories (n_student, H), its grad_weight / grad_bias are never read; chain[ACTOR].input: the teacher's observations (n_teacher, O),
     * in_stride their row stride; chain[CRITIC].input: the critic observations (n_critic, C). */
    LgTrainChain chain[LG_TRAIN_CTS_CHAINS];
    const float *student_obs;  /* (n_student, O), student_obs_stride floats between rows */
    const float *std;          /* (A) */
    float *grad_std;           /* (A), overwritten by lg_train_cts_backward */
    float *mu[LG_TRAIN_CTS_GROUPS];       /* (n_teacher, A), (n_student, A): written by forward, read by backward (the Hardtanh mask under clip_on) */
    float *sigma[LG_TRAIN_CTS_GROUPS];
    float *values;             /* (n_critic, V) */
    const float *grad_mu[LG_TRAIN_CTS_GROUPS];       /* backward only, like the next two */
    const float *grad_sigma[LG_TRAIN_CTS_GROUPS];
    const float *grad_values;
    int32_t mu_stride[LG_TRAIN_CTS_GROUPS], sigma_stride[LG_TRAIN_CTS_GROUPS];
    int32_t grad_mu_stride[LG_TRAIN_CTS_GROUPS], grad_sigma_stride[LG_TRAIN_CTS_GROUPS];
    int32_t values_stride, grad_values_stride;
    float *workspace;          /* LgTrainCTSPlan::workspace_floats floats */
    int64_t workspace_capacity;
} LgTrainCTSArgs;

/* The plan, a pure function of the three row counts and the widths.  Offsets in floats from `workspace`; -1 / 0 where there is no such
 * item (every entry of the history encoder: nothing of it is stored).
 *   cat_off       [obs | z], (n_teacher + n_student, O + Z) dense, teacher rows first: actor layer 0's operand of the weight gradient
 *   h_off / g_off the stored activations and layer gradients: (n_teacher, width) of the privilege encoder, (n_teacher + n_student, width) of
 *                 the actor with the student's rows n_teacher * width floats in, (n_critic, width) of the critic.  g_off of the privilege
 *                 encoder's last layer takes the latent columns of actor layer 0's input gradient.
 *   p_off / slices / slice_rows: the slice rule with LG_TRAIN_TS_TARGET_JOBS over n_teacher rows for the privilege encoder, n_teacher +
 *                 n_student for the actor, n_critic for the critic
 *   std_p_off     std_slices[0] partials of the teacher's grad_sigma (sliced over n_teacher), then std_slices[1] of the student's */
typedef struct LgTrainCTSPlan {
    int32_t row_tile;          /* 32, 16 or 8: the largest whose two LDS activations fit 160 KB over all four chains */
    int32_t lds_bytes;         /* dynamic LDS of the forward and input-gradient launches */
    int32_t slices[LG_TRAIN_CTS_CHAINS][LG_POLICY_MAX_LAYERS];
    int32_t slice_rows[LG_TRAIN_CTS_CHAINS][LG_POLICY_MAX_LAYERS];
    int32_t std_slices[LG_TRAIN_CTS_GROUPS], std_slice_rows[LG_TRAIN_CTS_GROUPS];
    int32_t tiles[LG_TRAIN_CTS_ROLES];           /* ceil(rows / row_tile) of the teacher, the student and the critic */
    int32_t weight_jobs;
    int32_t enc_first_buffer[LG_TRAIN_CTS_GROUPS];   /* the LDS activation (0 / 1) the privilege / history encoder starts in, so that it ends in
                                                    1, opposite the activation 0 the concatenation is formed in */
    int64_t h_off[LG_TRAIN_CTS_CHAINS][LG_POLICY_MAX_LAYERS];
    int64_t g_off[LG_TRAIN_CTS_CHAINS][LG_POLICY_MAX_LAYERS];
    int64_t p_off[LG_TRAIN_CTS_CHAINS][LG_POLICY_MAX_LAYERS];
    int64_t std_p_off;
    int64_t cat_off;
    int64_t workspace_floats;
} LgTrainCTSPlan;

/* Touches no device and reads no pointer: the row counts, n_obs, n_layers, n_in, n_out only.  Refused: a null descriptor or plan, a row
 * count < 1, n_teacher + n_student above 2^31 - 1, n_obs < 1, a layer count outside [1, LG_POLICY_MAX_LAYERS], a width outside [1, LG_POLICY_MAX_WIDTH], widths that do not
 * chain, the two encoders' output widths differing, actor layer[0].n_in other than O + Z, a row tile of 8 that does not fit the LDS. */
int lg_train_cts_plan(const LgTrainCTSArgs *args, LgTrainCTSPlan *out);

/* One launch, a one-dimensional grid of tiles[2] + tiles[0] + tiles[1] workgroups: the critic's tiles first (its workgroups are the long
 * ones), then the teacher's, then the student's.  A teacher tile carries its rows through the privilege encoder (hidden activations
 * stored) and the actor; a student tile through the history encoder (nothing stored) and the actor, into its own rows of the actor's
 * regions; a critic tile runs the critic.  Refused before the launch, with a message that names the member: what the plan refuses, a null
 * input, student_obs, weight, bias, std, mu, sigma, values or workspace, a stride below its width, clip_on with clip_actions not >= 0,
 * workspace_capacity below the plan. */
int lg_train_cts_forward(const LgTrainCTSArgs *args, void *stream);

/* Three launches: input gradients over the forward's grid (teacher: the actor, on through actor layer 0 and the privilege encoder;
 * student: the actor down to layer 1; critic), weight gradients (one wave per job, each job over the rows of its own chain; the two std
 * slabs read the two grad_sigma), combine over the privilege encoder, the actor and the critic.  Refused before any launch: what the
 * forward refuses, a null grad_weight / grad_bias of the privilege encoder, the actor or the critic, grad_std, grad_mu, grad_sigma or
 * grad_values, a gradient stride below its width. */
int lg_train_cts_backward(const LgTrainCTSArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LGTRAINCTS_H */

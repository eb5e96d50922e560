/* lgtraints.h -- C ABI of the fused learner passes of the teacher-student family: the two network passes of PPO_TS.update()
 * (rsl_rl/algorithms/ppo_ts.py:95-187) on ActorCriticTS (rsl_rl/modules/actor_critic_ts.py: four chains of Linear [+ ELU]; a
 * Hardtanh(+-clip_actions) behind the actor only where the module has one, ActorCriticTS itself has none).  Same contract as lgtrain.h and
 * lgtrainee.h, whose layer and chain structs are reused: plain device pointers and row strides in floats, the caller's HIP stream as void*;
 * 0 on success, otherwise non-zero with the message in lgsim.h's last-error call; nothing is allocated, nothing synchronised.  Everything is
 * float32.  Weights are read in place on every call.  This is PPO_TS's update only: ActorCriticCTS has the same members but updates two env
 * groups with other losses; its RL pass is lgtraincts.h's, its encoder step the encoder pass below with a mask of ones.
 *
 * The RL pass (lg_train_ts_*), per row:   z = privilege_encoder(privileged_obs);   mu = actor([obs | z]) (behind the Hardtanh under
 *   clip_on);   sigma = mu * 0 + std;   values = critic(critic_obs).  The forward stores the concatenated actor input [obs | z] (n_rows x
 *   (O + Z), dense), the hidden activations of the privilege encoder, the actor and the critic, mu, sigma and values.  The backward gives
 *   gradients for the actor, the critic, the privilege encoder and std: the RL gradient flows through the latent columns of actor layer 0's
 *   input into the privilege encoder.
 * The encoder pass (lg_train_enc_*):   p = history_encoder(obs_history);   y = privilege_encoder(privileged_obs), a constant of this pass;
 *   d = (p - y) * mask (mask is (n_rows, 1) and broadcasts);   loss = sum d^2 / (n_rows * Z);   d loss / d p = 2 d mask / (n_rows * Z),
 *   scaled in the backward by the scalar at `upstream`.  Gradients go to the history encoder only.
 *
 * Conventions:
 *   - Actor layer 0 DOES compute an input gradient, for the latent columns [O, O + Z) only: they are G of the privilege encoder's last
 *     layer (that chain ends in a Linear, so there is no activation derivative).  The observations get no gradient.  The critic's gradient
 *     reaches the critic only.
 *   - The RL pass never reads or writes the history encoder's gradient pointers (it has no history chain at all); the encoder pass never
 *     reads or writes the privilege encoder's grad_weight / grad_bias: the target is formed with no gradient, as under torch.no_grad().
 *   - The encoder loss follows the reference's arithmetic: the mask is a multiplication, not a select.  A non-finite prediction or target in
 *     a masked row still makes the loss non-finite (NaN * 0), as in torch.  The upstream scalar is read on the device: no host sync.  It is
 *     applied when gl is staged by the backward, so gl survives and a forward can be differentiated more than once.
 *   - The loss sum is float64 in a fixed order: a row tile's workgroup adds its d^2 (each thread its elements in index order, the 256
 *     thread sums by a fixed binary tree) into one float64 partial in the workspace; the one-workgroup finalize launch adds the partials
 *     in tile order.  No float atomics, no hand-off between workgroups inside a launch: two calls on the same inputs give the same bits.
 *   - All else is as lgtrain.h: elu' from the stored output, the Hardtanh mask from the stored mu, a grad_sigma reaches grad_std only,
 *     gradients are overwritten (accumulation is autograd's job), addresses are clamped on ragged tiles, a NaN in one input row changes
 *     no other row's outputs.
 */
#ifndef LGTRAINTS_H
#define LGTRAINTS_H

#include <stdint.h>
#include "lgtrain.h"   /* LgTrainLayer, LgTrainChain, the slice rule's constants */

#ifdef __cplusplus
extern "C" {
#endif

#define LG_TRAIN_TS_CHAINS 4         /* the plan's chain index: 0 the privilege encoder, 1 the actor, 2 the critic, 3 the history encoder */
#define LG_TRAIN_TS_PRIVILEGE 0
#define LG_TRAIN_TS_ACTOR 1
#define LG_TRAIN_TS_CRITIC 2
#define LG_TRAIN_TS_HISTORY 3
#define LG_TRAIN_TS_RL_CHAINS 3      /* LgTrainTSArgs::chain: privilege encoder, actor, critic, indexed as above */
#define LG_TRAIN_ENC_CHAINS 2        /* LgTrainEncArgs::chain */
#define LG_TRAIN_ENC_HISTORY 0
#define LG_TRAIN_ENC_PRIVILEGE 1
/* The slice rule is lgtrain.h's with this in place of LG_TRAIN_TARGET_JOBS.  go2_ts's largest first layers are the critic's 860 x 1024 (224
 * tiles of 64 x 64) and the history encoder's 900 x 256 (60 tiles).  At 512 jobs a layer the critic's would get 2 slices of 12288 rows of a
 * 24576-row mini-batch, one wave each, which the whole launch then waits for.  At 2048 it gets 9 slices of 2732 rows (2016 one-wave jobs:
 * about two per SIMD of the 256 compute units) and the history encoder's reaches the cap of 32 slices of 768 rows (1920 jobs); the combine
 * then adds at most 32 partials per element.  A higher target would only lengthen the combine: both layers already fill the machine. */
#define LG_TRAIN_TS_TARGET_JOBS 2048
#define LG_TRAIN_TS_THREADS 256      /* of the encoder forward's workgroup: the leaves of the loss partial's tree */

typedef struct LgTrainTSArgs {
    int32_t n_rows;
    int32_t clip_on;           /* 0: the actor ends in its last Linear (ActorCriticTS as it stands) */
    float clip_actions;
    int32_t n_obs;             /* O, the width of the observations; actor layer[0].n_in must be O + Z, Z the privilege encoder's last n_out */
    /* chain[PRIVILEGE].input: the privileged observations (n_rows, P); chain[ACTOR].input: the observations (n_rows, O), in_stride their
     * row stride; chain[CRITIC].input: the critic observations. */
    LgTrainChain chain[LG_TRAIN_TS_RL_CHAINS];
    const float *std;          /* (A) */
    float *grad_std;           /* (A), overwritten by lg_train_ts_backward */
    float *mu;                 /* (n_rows, A): written by forward, read by backward (the Hardtanh mask under clip_on) */
    float *sigma;              /* (n_rows, A) */
    float *values;             /* (n_rows, V) */
    const float *grad_mu;      /* backward only, like the next two */
    const float *grad_sigma;
    const float *grad_values;
    int32_t mu_stride, sigma_stride, values_stride;
    int32_t grad_mu_stride, grad_sigma_stride, grad_values_stride;
    float *workspace;          /* LgTrainTSPlan::workspace_floats floats */
    int64_t workspace_capacity;
} LgTrainTSArgs;

typedef struct LgTrainEncArgs {
    int32_t n_rows;
    int32_t mask_stride;       /* floats between the rows of the (n_rows, 1) mask, >= 1 */
    int32_t reserved[2];
    /* chain[HISTORY].input: the observation histories (n_rows, H); chain[PRIVILEGE].input: the privileged observations (n_rows, P).  The
     * privilege encoder's grad_weight / grad_bias are never read. */
    LgTrainChain chain[LG_TRAIN_ENC_CHAINS];
    const float *mask;         /* (n_rows, 1): `terminated` */
    float *loss;               /* one float, written by lg_train_enc_forward */
    const float *upstream;     /* one float on the device: d (whatever) / d loss; backward only */
    float *workspace;          /* LgTrainTSPlan::workspace_floats floats, 8-byte aligned (it holds the float64 partials) */
    int64_t workspace_capacity;
} LgTrainEncArgs;

/* The plan of either pass, a pure function of n_rows and the widths.  Offsets in floats from `workspace`; -1 / 0 where a pass has no such
 * item (the RL pass: every history-encoder entry, gl_off, y_off, partial_off, loss_tiles; the encoder pass: every entry of the other three
 * chains, cat_off, std).
 *   cat_off       [obs | z], (n_rows, O + Z) dense: actor layer 0's operand of the weight gradient
 *   h_off / g_off / p_off / slices / slice_rows: as LgTrainPlan, indexed by LG_TRAIN_TS_* chain.  g_off of the privilege encoder's last
 *                 layer takes the latent columns of actor layer 0's input gradient.
 *   gl_off        2 d mask / (n_rows Z), (n_rows, Z) dense, as the encoder forward leaves it; the backward scales it into g_off of the
 *                 history encoder's last layer
 *   y_off         the encoder targets, (n_rows, Z) dense: a row tile's workgroup writes its rows and reads only those back
 *   partial_off   loss_tiles float64 partials (an even offset) */
typedef struct LgTrainTSPlan {
    int32_t row_tile;          /* 32, 16 or 8: the largest whose two LDS activations fit 160 KB over the chains of the pass (the encoder
                                  pass keeps LG_TRAIN_TS_THREADS float64 of LDS for the loss tree besides) */
    int32_t lds_bytes;         /* dynamic LDS of the forward and input-gradient launches */
    int32_t slices[LG_TRAIN_TS_CHAINS][LG_POLICY_MAX_LAYERS];
    int32_t slice_rows[LG_TRAIN_TS_CHAINS][LG_POLICY_MAX_LAYERS];
    int32_t std_slices, std_slice_rows;
    int32_t weight_jobs;
    int32_t loss_tiles;        /* ceil(n_rows / row_tile) in the encoder pass */
    int32_t enc_first_buffer;  /* RL pass: the LDS activation (0 / 1) the privilege encoder starts in, so that it ends in 1, opposite the
                                  activation 0 the concatenation is formed in (and, in the backward, the latent gradient is read from) */
    int32_t reserved;
    int64_t h_off[LG_TRAIN_TS_CHAINS][LG_POLICY_MAX_LAYERS];
    int64_t g_off[LG_TRAIN_TS_CHAINS][LG_POLICY_MAX_LAYERS];
    int64_t p_off[LG_TRAIN_TS_CHAINS][LG_POLICY_MAX_LAYERS];
    int64_t std_p_off;
    int64_t cat_off;
    int64_t gl_off;
    int64_t y_off;
    int64_t partial_off;
    int64_t workspace_floats;
} LgTrainTSPlan;

/* Touch no device and read no pointer: n_rows, n_obs, n_layers, n_in, n_out only.  Refused: a null descriptor or plan, n_rows < 1, n_obs < 1,
 * a layer count outside [1, LG_POLICY_MAX_LAYERS], a width outside [1, LG_POLICY_MAX_WIDTH], widths that do not chain, actor layer[0].n_in
 * other than O + Z; in lg_train_enc_plan the two encoders' output widths differing; a row tile of 8 that does not fit the LDS. */
int lg_train_ts_plan(const LgTrainTSArgs *args, LgTrainTSPlan *out);
int lg_train_enc_plan(const LgTrainEncArgs *args, LgTrainTSPlan *out);

/* One launch, grid (row tiles, 2): workgroup y = 0 carries its rows through the privilege encoder (hidden activations stored) and then the
 * actor in LDS (the concatenation is formed in LDS from the observations and the latent), y = 1 runs the critic.  Refused before the launch,
 * with a message that names the member: what the plan refuses, a null input, weight, bias, std, mu, sigma, values or workspace, a stride
 * below its width, clip_on with clip_actions not >= 0, workspace_capacity below the plan. */
int lg_train_ts_forward(const LgTrainTSArgs *args, void *stream);

/* Three launches: input gradients (y = 0: the actor, on through actor layer 0 and the privilege encoder; y = 1: the critic), weight
 * gradients, combine, over three chains.  Refused before any launch: what the forward refuses, a null grad_weight / grad_bias of any of the
 * three chains, grad_std, grad_mu, grad_sigma or grad_values, a gradient stride below its width. */
int lg_train_ts_backward(const LgTrainTSArgs *args, void *stream);

/* Two launches: per row tile the privilege encoder (nothing stored but y), the history encoder (hidden activations stored), gl and one
 * float64 partial per tile to the workspace; then the one-workgroup finalize that writes *loss.  Refused before any launch: what the plan
 * refuses, a null input, weight, bias, mask, loss or workspace, a workspace that is not 8-byte aligned, a stride below its width,
 * workspace_capacity below the plan. */
int lg_train_enc_forward(const LgTrainEncArgs *args, void *stream);

/* Three launches over the history encoder; the input-gradient launch scales gl by *upstream.  Refused before any launch: what the forward
 * refuses but a null loss, a null upstream, grad_weight or grad_bias of the history encoder. */
int lg_train_enc_backward(const LgTrainEncArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LGTRAINTS_H */

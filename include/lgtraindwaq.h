/* lgtraindwaq.h -- C ABI of the fused learner passes of the DreamWaQ family: the two network passes of PPO_DreamWaQ.update()
 * (rsl_rl/algorithms/ppo_dreamwaq.py:140-236) on ActorCriticDreamWaQ (rsl_rl/modules/actor_critic_dreamwaq.py, rsl_rl/modules/vae.py: an
 * encoder of Linear + ELU whose LAST Linear carries an ELU too, four one-layer heads on its output, a decoder, the actor and the critic).
 * Same contract as lgtrain.h, lgtrainee.h and lgtraints.h, whose layer and chain structs are reused: plain device pointers and row strides in
 * floats, the caller's HIP stream as void*; 0 on success, otherwise non-zero with the message in lgsim.h's last-error call; nothing is
 * allocated, nothing synchronised.  Everything is float32.  Weights are read in place on every call.
 *
 * With h = encoder(obs_history) (n_rows, H), the heads latent_mu (L), latent_var (L), vel_mu (E), vel_var (E) = Linear(h), the two
 * log-variances behind a Hardtanh(+-var_clip), and the caller's noise eps (n_rows, L + E), columns [z | vel]:
 *     z = eps_z * exp(0.5 * latent_var) + latent_mu,      v = eps_v * exp(0.5 * vel_var) + vel_mu.
 * The RL pass (lg_train_dwaq_*), per row:   mu = actor([obs | z | v]) (behind the Hardtanh under clip_on);   sigma = mu * 0 + std;
 *   values = critic(critic_obs).  The forward stores the concatenated actor input (n_rows x (O + L + E), dense), the hidden activations of the
 *   actor and the critic, mu, sigma and values; nothing of the encoder or the heads.  The backward gives gradients for the actor, the critic
 *   and std ONLY: the reference clears the gradient the RL loss sends into the VAE before anything reads it (vae_optimizer.zero_grad()).
 * The VAE pass (lg_train_vae_*), with t = mask (n_rows, 1), B = n_rows:   rec = decoder([z | v]);
 *     est  = sum ((v - labels) t)^2 / (B E);       recl = sum ((rec - next_states) t)^2 / (B D);
 *     kld  = -0.5 (sum_i s_i) (sum_j t_j) / B^2,   s_i = sum_c (1 + latent_var - latent_mu^2 - exp(latent_var));
 *     loss = est + recl + kld_weight * kld.
 *   The kld is the reference's arithmetic: its (B,) row sums times its (B, 1) mask broadcast to (B, B) before the mean, so every row's s
 *   carries the factor T / B^2, T = sum t, whatever its own mask.  Gradients go to the encoder, the four heads and the decoder, scaled by the
 *   scalar at `upstream`.
 *
 * Conventions:
 *   - Masks are multiplications, not selects: NaN * 0 stays NaN, as in torch.  The upstream scalar is read on the device: no host sync.
 *   - The loss sums are float64 in a fixed order: a row tile's workgroup adds its (d_est)^2, (d_rec)^2, s and t (each thread its elements in
 *     index order, the 256 thread sums by a fixed binary tree) into four float64 partials in the workspace; the one-workgroup finalize adds
 *     the partials in tile order, writes the four losses and leaves T / B^2 (float32) in the workspace for the backward.
 *   - A log-variance's Hardtanh mask comes from the stored clipped value: >= var_clip or <= -var_clip passes nothing (a NaN passes the
 *     gradient on, as hardtanh_backward does); the encoder's last elu' from its stored output.
 *   - The gradients of the four heads through the encoder's output are added in head order (latent_mu, latent_var, vel_mu, vel_var).
 *   - All else is as lgtrain.h: plain stores, no float atomics, no hand-off between workgroups inside a launch (two calls on the same inputs
 *     give the same bits), gradients are overwritten, addresses are clamped on ragged tiles, a NaN in one input row changes no other row's
 *     outputs.
 */
#ifndef LGTRAINDWAQ_H
#define LGTRAINDWAQ_H

#include <stdint.h>
#include "lgtrain.h"   /* LgTrainLayer, LgTrainChain, the slice rule's constants */

#ifdef __cplusplus
extern "C" {
#endif

#define LG_TRAIN_DWAQ_CHAINS 7       /* the plan's chain index and LgTrainDwaqArgs::chain */
#define LG_TRAIN_DWAQ_ENCODER 0
#define LG_TRAIN_DWAQ_LATENT_MU 1    /* the four heads: one-layer chains whose input is the encoder's output (their `input` is not read) */
#define LG_TRAIN_DWAQ_LATENT_VAR 2
#define LG_TRAIN_DWAQ_VEL_MU 3
#define LG_TRAIN_DWAQ_VEL_VAR 4
#define LG_TRAIN_DWAQ_ACTOR 5
#define LG_TRAIN_DWAQ_CRITIC 6
#define LG_TRAIN_DWAQ_HEADS 4
#define LG_TRAIN_VAE_CHAINS 6        /* LgTrainVaeArgs::chain: the encoder and the heads as above, then the decoder */
#define LG_TRAIN_VAE_DECODER 5
/* The slice rule is lgtrain.h's with this in place of LG_TRAIN_TARGET_JOBS, for the reason lgtraints.h gives: go2_dreamwaq's largest first
 * layers are the critic's 885 x 512 and the encoder's 900 x 256 (60 tiles of 64 x 64). */
#define LG_TRAIN_DWAQ_TARGET_JOBS 2048
#define LG_TRAIN_DWAQ_THREADS 256    /* of the VAE forward's workgroup: the leaves of the loss partials' trees */
#define LG_TRAIN_VAE_LOSSES 4        /* LgTrainVaeArgs::loss: total, estimation, reconstruction, kld; also the partial streams (d_est^2, d_rec^2, s, t) */

typedef struct LgTrainDwaqArgs {
    int32_t n_rows;
    int32_t clip_on;           /* 0: the actor ends in its last Linear (ActorCriticDreamWaQ as it stands) */
    float clip_actions;
    int32_t n_obs;             /* O; actor layer[0].n_in must be O + L + E */
    float var_clip;            /* the Hardtanh behind latent_var and vel_var, >= 0 */
    int32_t noise_stride;
    int32_t reserved[2];
    /* chain[ENCODER].input: the observation histories; chain[ACTOR].input: the observations (n_rows, O), in_stride their row stride;
     * chain[CRITIC].input: the critic observations.  Gradient pointers of the encoder and the heads are never read. */
    LgTrainChain chain[LG_TRAIN_DWAQ_CHAINS];
    const float *noise;        /* (n_rows, L + E), columns [z | vel] */
    const float *std;          /* (A) */
    float *grad_std;           /* (A), overwritten by lg_train_dwaq_backward */
    float *mu;                 /* (n_rows, A): written by forward, read by backward (the Hardtanh mask under clip_on) */
    float *sigma;              /* (n_rows, A) */
    float *values;             /* (n_rows, V) */
    const float *grad_mu;      /* backward only, like the next two */
    const float *grad_sigma;
    const float *grad_values;
    int32_t mu_stride, sigma_stride, values_stride;
    int32_t grad_mu_stride, grad_sigma_stride, grad_values_stride;
    float *workspace;          /* LgTrainDwaqPlan::workspace_floats floats */
    int64_t workspace_capacity;
} LgTrainDwaqArgs;

typedef struct LgTrainVaeArgs {
    int32_t n_rows;
    int32_t labels_stride, next_states_stride, mask_stride, noise_stride;
    float var_clip;
    float kld_weight;
    int32_t reserved;
    LgTrainChain chain[LG_TRAIN_VAE_CHAINS];      /* chain[ENCODER].input: the observation histories; no other input is read */
    const float *labels;       /* (n_rows, E): the explicit-information labels */
    const float *next_states;  /* (n_rows, D), D the decoder's last n_out */
    const float *mask;         /* (n_rows, 1): `terminated` */
    const float *noise;        /* (n_rows, L + E), columns [z | vel]; the backward reads it again */
    float *loss;               /* LG_TRAIN_VAE_LOSSES floats, written by lg_train_vae_forward */
    const float *upstream;     /* one float on the device: d (whatever) / d loss[0]; backward only */
    float *workspace;          /* LgTrainDwaqPlan::workspace_floats floats, 8-byte aligned (it holds the float64 partials) */
    int64_t workspace_capacity;
} LgTrainVaeArgs;

/* The plan of either pass, a pure function of n_rows and the widths.  Offsets in floats from `workspace`; -1 / 0 where a pass has no such
 * item.  In the VAE pass chain index 5 is the decoder and index 6 is empty; in the RL pass only the actor and the critic have entries.
 *   cat_off       RL: [obs | z | v], (n_rows, O + L + E) dense; VAE: [z | v], (n_rows, L + E) dense: layer 0's weight-gradient operand
 *   enc_out_off   VAE: the encoder's last output (behind its ELU), (n_rows, H) dense: the heads' weight-gradient operand
 *   head_off[h]   VAE: head h's output (behind the clip), dense
 *   gl_rec_off / gl_est_off   2 d t / (B D) and 2 d t / (B E) as the forward leaves them; the backward scales them by *upstream
 *   partial_off   LG_TRAIN_VAE_LOSSES * loss_tiles float64 partials (an even offset), stream after stream; scale_off: T / B^2 behind them
 *   lds_x / lds_y the LDS activation (0 / 1) the encoder ends in, and the opposite one: the heads write four disjoint regions of lds_y at
 *                 row_tile * (the LDS strides of the heads before) floats; the VAE backward forms the head products in two regions of lds_x,
 *                 row_tile * (the stride of H) floats apart, adding one to the other in head order.  Both are counted in the widths that size the row tile. */
typedef struct LgTrainDwaqPlan {
    int32_t row_tile;          /* 32, 16 or 8 */
    int32_t lds_bytes;
    int32_t slices[LG_TRAIN_DWAQ_CHAINS][LG_POLICY_MAX_LAYERS];
    int32_t slice_rows[LG_TRAIN_DWAQ_CHAINS][LG_POLICY_MAX_LAYERS];
    int32_t std_slices, std_slice_rows;
    int32_t weight_jobs;
    int32_t loss_tiles;        /* ceil(n_rows / row_tile) in the VAE pass */
    int32_t lds_x, lds_y;
    int64_t h_off[LG_TRAIN_DWAQ_CHAINS][LG_POLICY_MAX_LAYERS];
    int64_t g_off[LG_TRAIN_DWAQ_CHAINS][LG_POLICY_MAX_LAYERS];
    int64_t p_off[LG_TRAIN_DWAQ_CHAINS][LG_POLICY_MAX_LAYERS];
    int64_t std_p_off;
    int64_t cat_off;
    int64_t enc_out_off;
    int64_t head_off[LG_TRAIN_DWAQ_HEADS];
    int64_t gl_rec_off, gl_est_off;
    int64_t partial_off, scale_off;
    int64_t workspace_floats;
} LgTrainDwaqPlan;

/* Touch no device and read no pointer.  Refused: a null descriptor or plan, n_rows < 1, n_obs < 1, a layer count outside
 * [1, LG_POLICY_MAX_LAYERS] (a head: other than 1), a width outside [1, LG_POLICY_MAX_WIDTH], widths that do not chain, a head whose n_in
 * is not H, a log-variance head whose n_out differs from its mean's, actor layer[0].n_in other than O + L + E, decoder layer[0].n_in other
 * than L + E, a row tile of 8 that does not fit the LDS. */
int lg_train_dwaq_plan(const LgTrainDwaqArgs *args, LgTrainDwaqPlan *out);
int lg_train_vae_plan(const LgTrainVaeArgs *args, LgTrainDwaqPlan *out);

/* One launch, grid (row tiles, 2): workgroup y = 0 carries its rows through the encoder and the heads (nothing stored), forms the draw and
 * the concatenation in LDS and runs the actor; y = 1 runs the critic.  Refused before the launch, with a message that names the member:
 * what the plan refuses, a null input, weight, bias, noise, std, mu, sigma, values or workspace, a stride below its width, var_clip not
 * >= 0, clip_on with clip_actions not >= 0, workspace_capacity below the plan. */
int lg_train_dwaq_forward(const LgTrainDwaqArgs *args, void *stream);

/* Three launches over the actor and the critic (input gradients, weight gradients, combine), grad_std riding along.  Refused before any
 * launch: what the forward refuses, a null grad_weight / grad_bias of the actor or the critic, grad_std, grad_mu, grad_sigma or
 * grad_values, a gradient stride below its width. */
int lg_train_dwaq_backward(const LgTrainDwaqArgs *args, void *stream);

/* Two launches: per row tile the encoder (every activation stored, its last output too), the heads (stored), the draw (stored), the
 * decoder, gl_est, gl_rec and four float64 partials; then the one-workgroup finalize.  Refused before any launch: what the plan refuses, a
 * null input, weight, bias, labels, next_states, mask, noise, loss or workspace, a workspace that is not 8-byte aligned, a stride below its
 * width, var_clip not >= 0, workspace_capacity below the plan. */
int lg_train_vae_forward(const LgTrainVaeArgs *args, void *stream);

/* Three launches over the encoder, the heads and the decoder.  The input-gradient launch runs, per row tile: the decoder down to layer 1,
 * one more layer over decoder layer 0 (no ELU factor), the four head gradients, the four head products summed in head order behind the
 * encoder's last elu', the encoder.  Refused before any launch: what the forward refuses but a null loss, a null upstream, grad_weight or
 * grad_bias of any chain. */
int lg_train_vae_backward(const LgTrainVaeArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LGTRAINDWAQ_H */

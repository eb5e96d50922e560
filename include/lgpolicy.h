/* lgpolicy.h -- C ABI of the fused policy step: what rsl_rl/algorithms/ppo.py:93-105 asks of ActorCritic / ActorCriticEE during a
 * rollout (act, evaluate, get_actions_log_prob, action_mean, action_std) in ONE launch; likewise PPO_TS / PPO_CTS / PPO_DreamWaQ.act of
 * ActorCriticTS / ActorCriticCTS / ActorCriticDreamWaQ.  For the TS family the `estimator` slot carries whichever encoder the call wants
 * (the privilege encoder on the privileged observations for act / act_teacher, the history encoder on the history for act_student); CTS
 * adds `encoder_b` for the rows from `n_split` on; DreamWaQ puts the VAE's encoder into `estimator` and its four heads into `head`.  Same conventions as lgrollout.h: plain device
 * pointers, sizes, the caller's HIP stream as void*; 0 on success, otherwise non-zero with the message in lgsim.h's last-error call.
 * Everything is float32.  Weights are read where torch keeps them (nn.Linear.weight is (out, in) row-major) on every call: nothing is
 * packed or cached, so an optimizer step between two calls is seen by the second.
 * NaN is not silent: a NaN in a row of an input reaches `mu`, `sigma`, `actions` and `log_prob` of that env row (and the head's `latent_out`
 * / `params_out` when it entered through the estimator chain), as with torch -- both clips (`clip_actions`, `logvar_clip`) are compares
 * that pass a NaN on, like torch.nn.Hardtanh; no other row and no output of a chain that did not read it changes a bit.  The same holds
 * for the states of a memory (below): a NaN in a row's observation or incoming state reaches that row's outputs and new state only.
 * A recurrent policy (rsl_rl/modules/actor_critic_recurrent.py: an LSTM or GRU in front of the actor and of the critic) passes
 * LgPolicyRecurrentArgs -- LgPolicyArgs with the two memories behind it -- to the _recurrent entry points; the memories run in the same
 * launch, ahead of the MLP they feed.
 */
#ifndef LGPOLICY_H
#define LGPOLICY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_POLICY_MAX_LAYERS 4
#define LG_POLICY_MAX_WIDTH 2048
#define LG_POLICY_MAX_RNN_LAYERS 2
#define LG_POLICY_MAX_RNN_HIDDEN (LG_POLICY_MAX_WIDTH / 4)   /* the gates of one cell, 4 H wide for both kinds, are one activation */
#define LG_POLICY_LSTM 1
#define LG_POLICY_GRU 2
#define LG_POLICY_DETERMINISTIC 1u   /* actor (and estimator) only; writes `mu` (and `chain.out` of the estimator): act_inference */
#define LG_POLICY_VALUES_ONLY 2u     /* critic only: evaluate */
#define LG_POLICY_STREAM_TAG 0x504F4C49u   /* fourth Philox counter word of the action draw */
#define LG_POLICY_LATENT_TAG 0x4C41544Eu   /* ... and of the VAE head's latent draw */

/* y = W x + b, then ELU(alpha = 1) where `elu` is set */
typedef struct LgPolicyLayer {
    const float *weight;   /* (out, in) row-major */
    const float *bias;     /* (out) */
    int32_t n_in;
    int32_t n_out;
    int32_t elu;
    int32_t reserved;
} LgPolicyLayer;

/* up to LG_POLICY_MAX_LAYERS layers on rows of `input`; n_layers == 0: the chain is absent */
typedef struct LgPolicyChain {
    const float *input;    /* (N, in_width), in_stride floats between rows */
    float *out;            /* (N, last out), out_stride floats between rows; may be NULL for the estimator.  The actor's output goes to `mu`. */
    int32_t n_layers;
    int32_t in_width;
    int32_t in_stride;
    int32_t out_stride;
    LgPolicyLayer layer[LG_POLICY_MAX_LAYERS];
} LgPolicyChain;

/* The VAE head of rsl_rl/modules/vae.py:65-101 behind the `estimator` chain (the VAE's encoder, whose last Linear may carry an ELU): four
 * Linear heads on the encoded vector (H), each (out, H) row-major and read in place; the two log-variances are clipped to +-logvar_clip.
 * Sampling: sample = eps * exp(0.5 logvar) + mu, and the actor reads [actor.input[:, :in_width] (F) | z (L) | vel (E)], formed in LDS, so
 * actor.layer[0].n_in = F + L + E.  LG_POLICY_DETERMINISTIC: no draw, the actor reads [obs | latent_mu | vel_mu].  eps is `noise`
 * ((N, L + E), columns in (z, vel) order) or, when NULL, Philox4x32-10 with counter (env, quad over the L + E columns, *counter,
 * LG_POLICY_LATENT_TAG), key = seed, Box-Muller as the action draw.  H == L == E == 0: no head. */
typedef struct LgPolicyHead {
    const float *latent_mu_w, *latent_mu_b;     /* (L, H), (L) */
    const float *latent_var_w, *latent_var_b;   /* (L, H), (L): the log-variance */
    const float *vel_mu_w, *vel_mu_b;           /* (E, H), (E) */
    const float *vel_var_w, *vel_var_b;         /* (E, H), (E) */
    int32_t H, L, E;
    float logvar_clip;
    const float *noise;            /* (N, L + E) with noise_stride, or NULL: Philox */
    float *latent_out;             /* optional (N, L + E): the samples (z, vel), or the means in deterministic mode */
    float *params_out;             /* optional (N, 2L + 2E): latent_mu, latent_logvar, vel_mu, vel_logvar; log-variances after the clip */
    float *dbg_latent_uniform;     /* optional (N, 4 * ceil((L + E) / 4)), dense: the uniforms the latent draw used */
    int32_t noise_stride;
    int32_t latent_stride;
    int32_t params_stride;
    int32_t reserved;
} LgPolicyHead;

/* One layer of a torch nn.LSTM / nn.GRU, read in place: weight_ih_l{k} (G H, in) and weight_hh_l{k} (G H, H) row-major, bias_ih_l{k} and
 * bias_hh_l{k} (G H); G = 4 with gate rows (i, f, g, o) for an LSTM, G = 3 with (r, z, n) for a GRU; `in` is in_width for layer 0, H behind. */
typedef struct LgPolicyRnnLayer {
    const float *weight_ih, *weight_hh, *bias_ih, *bias_hh;
} LgPolicyRnnLayer;

/* The memory in front of a chain (Memory of actor_critic_recurrent.py:92-116 in inference mode): one time step of an LSTM or GRU on rows
 * of `input`; the top layer's new h (N, H) is the chain's input, so the chain's own input / in_width / in_stride are not read and its
 * layer[0].n_in is H.  The cell is torch's:
 *   LSTM  gates = W_ih x + b_ih + W_hh h + b_hh;  c' = s(f) c + s(i) tanh(g);  h' = s(o) tanh(c')
 *   GRU   r = s(W_ir x + b_ir + W_hr h + b_hr), z likewise;  n = tanh(W_in x + b_in + r (W_hn h + b_hn));  h' = (1 - z) n + z h
 * and layer k > 0 reads the new h' of layer k - 1.  `h` (and `c`) are the live states, (n_layers, N, H) contiguous, UPDATED IN PLACE: a
 * workgroup reads and writes the state rows of its own env rows only, and has read a layer's previous state before it writes the new one.
 * reset_mask (N bytes, optional): a non-zero byte means that row's incoming state is read as zero (the reset(dones) of the step before).
 * h_prev_out / c_prev_out (optional, same layout): the state the call started from, after the mask -- what PPO.act stores with the
 * transition.  kind == 0 (an all-zero struct): no memory.  LG_POLICY_DETERMINISTIC runs memory_a only, LG_POLICY_VALUES_ONLY memory_c
 * only; a memory whose chain does not run is not touched. */
typedef struct LgPolicyMemory {
    int32_t kind;              /* 0 none, LG_POLICY_LSTM, LG_POLICY_GRU */
    int32_t n_layers;          /* 1 .. LG_POLICY_MAX_RNN_LAYERS */
    int32_t hidden;            /* H, 1 .. LG_POLICY_MAX_RNN_HIDDEN */
    int32_t in_width;
    int32_t in_stride;
    int32_t reserved;
    const float *input;        /* (N, in_width), in_stride floats between rows */
    LgPolicyRnnLayer layer[LG_POLICY_MAX_RNN_LAYERS];
    float *h;                  /* (n_layers, N, H) */
    float *c;                  /* (n_layers, N, H) for an LSTM, NULL for a GRU */
    float *h_prev_out;         /* optional (n_layers, N, H) */
    float *c_prev_out;         /* optional (n_layers, N, H), LSTM only */
    const uint8_t *reset_mask; /* optional (N) */
} LgPolicyMemory;

typedef struct LgPolicyArgs {
    int32_t n_envs;
    uint32_t flags;
    LgPolicyChain estimator;   /* optional; with it the actor's first layer reads (actor.input[:, :in_width], estimator output): the   */
    LgPolicyChain actor;       /* concatenation of actor_critic_ee.py:115-122, formed in LDS; layer[0].n_in = in_width + estimator out */
    LgPolicyChain critic;      /* optional */
    float clip_actions;        /* Hardtanh(+-clip_actions) behind the actor's last layer when clip_on */
    int32_t clip_on;
    const float *std;          /* (A) */
    const float *noise;        /* (N, A) with noise_stride, or NULL: Philox */
    int32_t noise_stride;
    int32_t actions_stride;
    int32_t mu_stride;
    int32_t sigma_stride;
    float *actions;            /* (N, A)  mu + sigma * z */
    float *mu;                 /* (N, A)  clipped actor output */
    float *sigma;              /* (N, A)  mu * 0 + std */
    float *log_prob;           /* (N, 1), log_prob_stride floats between rows: sum over a, in action order, of
                                  -(action - mu)^2 / (2 sigma^2) - log sigma - 0.5 log 2 pi */
    int32_t log_prob_stride;
    int32_t reserved;
    /* Philox4x32-10 draw (noise == NULL): counter (env, action quad, *counter, LG_POLICY_STREAM_TAG), key = seed; words (x, y) and (z, w)
     * each give two normals by Box-Muller: r = sqrt(-2 log(1 - u01(x))), (r cos, r sin)(2 pi u01(y)).  *counter is read by the act launch
     * and incremented by a one-lane launch enqueued behind it, so a captured call draws fresh numbers on every replay. */
    uint64_t seed;
    uint32_t *counter;
    float *dbg_uniform;        /* optional (N, 4 * ceil(A / 4)): the uniforms the draw used */
    /* Row groups (PPO_CTS, ppo_cts.py:110-135) when has_split: env rows [0, n_split) run `estimator` on estimator.input, rows
     * [n_split, n_envs) run `encoder_b` on encoder_b.input; both inputs (and both optional `out`s) are full-N matrices addressed by the
     * global env row, the first read only below the split, the second only from it on.  Both chains end at the same width and feed the
     * same actor layers and epilogue; the Philox counter keeps the global env index, and the critic stays one pass over all rows.  n_split
     * of 0 or n_envs leaves one group empty.  *counter is incremented once per call whichever draws use it. */
    LgPolicyChain encoder_b;
    int32_t n_split;
    int32_t has_split;         /* encoder_b and has_split come together */
    LgPolicyHead head;
} LgPolicyArgs;

/* LgPolicyArgs grown by the two memories, which lie directly behind its last member: every member of `args` is where it is in a plain
 * LgPolicyArgs and keeps its meaning, and an all-zero memory means "no memory", so a zero-filled tail describes the same call as `args`
 * alone.  No flag bit was added: flags & ~3u is refused as before. */
typedef struct LgPolicyRecurrentArgs {
    LgPolicyArgs args;
    LgPolicyMemory memory_a;   /* in front of the actor; excludes estimator, encoder_b and head */
    LgPolicyMemory memory_c;   /* in front of the critic */
} LgPolicyRecurrentArgs;

/* One act launch (plus the one-lane counter launch on the Philox path).  Allocates nothing and never synchronises.  Refused before any
 * launch: a null or inconsistent descriptor, more than LG_POLICY_MAX_LAYERS layers, a width outside [1, LG_POLICY_MAX_WIDTH], a stride
 * below its width, layer widths that do not chain, a row tile that does not fit the LDS; n_split outside [0, n_envs], encoder_b without
 * has_split or the reverse, group chains ending at different widths, head widths that do not chain (H against the estimator chain's
 * output, actor.layer[0].n_in against in_width + L + E), head together with encoder_b, neither latent noise nor a counter in sampling
 * mode, an (obs | latent) width above LG_POLICY_MAX_WIDTH. */
int lg_policy_act(const LgPolicyArgs *args, void *stream);

/* lg_policy_act with the memories: the same launch (and counter launch), the same refusals, and for a memory also an unknown kind, a layer
 * count outside [1, LG_POLICY_MAX_RNN_LAYERS], H outside [1, LG_POLICY_MAX_RNN_HIDDEN], a null parameter, input or state pointer, `c`
 * missing for an LSTM or given for a GRU, a chain whose layer[0].n_in is not H, a memory together with the estimator, encoder_b or the
 * head.  With both memories absent it is lg_policy_act on `args`. */
int lg_policy_act_recurrent(const LgPolicyRecurrentArgs *args, void *stream);

/* The stand-alone reset(dones) of actor_critic_recurrent.py:72-74: one launch that zeroes the rows of `h` (and `c`) of both memories whose
 * byte in `mask` ((N) bytes on the device) is non-zero; mask == NULL zeroes every row.  Only the memories' kind, n_layers, hidden, h and c
 * and args.n_envs are read.  Refused: no memory at all, or a memory that the act call would refuse for those members. */
int lg_policy_reset(const LgPolicyRecurrentArgs *args, const uint8_t *mask, void *stream);

/* rows of envs one workgroup carries for this descriptor (32, 16 or 8), or 0 with the last error set: what lg_policy_act would choose */
int lg_policy_row_tile(const LgPolicyArgs *args);
int lg_policy_row_tile_recurrent(const LgPolicyRecurrentArgs *args);

#ifdef __cplusplus
}
#endif
#endif /* LGPOLICY_H */

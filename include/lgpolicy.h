/* lgpolicy.h -- C ABI of the fused policy step: what rsl_rl/algorithms/ppo.py:93-105 asks of ActorCritic / ActorCriticEE during a
 * rollout (act, evaluate, get_actions_log_prob, action_mean, action_std) in ONE launch.  Same conventions as lgrollout.h: plain device
 * pointers, sizes, the caller's HIP stream as void*; 0 on success, otherwise non-zero with the message in lgsim.h's last-error call.
 * Everything is float32.  Weights are read where torch keeps them (nn.Linear.weight is (out, in) row-major) on every call: nothing is
 * packed or cached, so an optimizer step between two calls is seen by the second.
 */
#ifndef LGPOLICY_H
#define LGPOLICY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_POLICY_MAX_LAYERS 4
#define LG_POLICY_MAX_WIDTH 2048
#define LG_POLICY_DETERMINISTIC 1u   /* actor (and estimator) only; writes `mu` (and `chain.out` of the estimator): act_inference */
#define LG_POLICY_VALUES_ONLY 2u     /* critic only: evaluate */
#define LG_POLICY_STREAM_TAG 0x504F4C49u   /* fourth Philox counter word of the action draw */

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
} LgPolicyArgs;

/* One act launch (plus the one-lane counter launch on the Philox path).  Allocates nothing and never synchronises.  Refused before any
 * launch: a null or inconsistent descriptor, more than LG_POLICY_MAX_LAYERS layers, a width outside [1, LG_POLICY_MAX_WIDTH], a stride
 * below its width, layer widths that do not chain, a row tile that does not fit the LDS. */
int lg_policy_act(const LgPolicyArgs *args, void *stream);

/* rows of envs one workgroup carries for this descriptor (32, 16 or 8), or 0 with the last error set: what lg_policy_act would choose */
int lg_policy_row_tile(const LgPolicyArgs *args);

#ifdef __cplusplus
}
#endif
#endif /* LGPOLICY_H */

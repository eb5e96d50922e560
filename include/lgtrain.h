/* lgtrain.h -- C ABI of the fused learner pass: the training forward of the plain ActorCritic (rsl_rl/modules/actor_critic.py: two chains
 * of Linear [+ ELU], a Hardtanh(+-clip_actions) behind the actor, sigma = mu * 0 + std) and its backward, the block of PPO.update()
 * (rsl_rl/algorithms/ppo.py:124-148) between the mini-batch gather and the loss head (lgppo.h) and between the loss head and the optimizer
 * (lgoptim.h).  Same conventions as lgppo.h and lgoptim.h: plain device pointers and row strides in floats, the caller's HIP stream as
 * void*; 0 on success, otherwise non-zero with the message in lgsim.h's last-error call; nothing is allocated, nothing synchronised.
 * Everything is float32.  Weights are read where torch keeps them (nn.Linear.weight is (out, in) row-major, contiguous) on every call.
 *
 * Forward, per chain and row:   H_-1 = input row;   H_l = act_l(W_l H_(l-1) + b_l), act_l = ELU(alpha = 1) where `elu` is set;
 *   mu = Hardtanh(actor's last H) when clip_on (compares: a NaN stays a NaN), sigma = mu * 0 + std, values = critic's last H.
 *   Every hidden layer's H_l (after the ELU) is also stored to the workspace: it is the next layer's input and all the backward needs.
 * Backward, per chain:   G_L = grad_mu where -clip < mu < clip holds for the stored mu or is unordered, 0 elsewhere (hardtanh_backward),
 *   or grad_values;   G_(l-1) = (G_l W_l) * elu'(H_(l-1)),   elu'(h) = 1 for h > 0, h + 1 otherwise (from the stored OUTPUT);
 *   grad_weight_l = G_l^T H_(l-1),   grad_bias_l = column sums of G_l,   grad_std = column sums of grad_sigma.
 *   The gradients are OVERWRITTEN, never accumulated: accumulation into .grad is autograd's job.  No gradient for the inputs.
 *
 * Conventions:
 *   - The gradient that reaches mu through sigma = mu * 0 + std is taken as exactly zero.  Autograd forms grad_sigma * 0, which is NaN
 *     for a non-finite grad_sigma; here such a grad_sigma reaches grad_std only.
 *   - elu' from the stored output: h + 1 = fl(expm1(x)) + 1 differs from exp(x) by at most one ulp of 1 (for x below about -17 it is 0
 *     where exp(x) is a positive number below 1e-7).  A NaN h gives a NaN derivative, where torch's elu_backward gives 1: the NaN of
 *     a row reaches a superset of the parameter gradients it reaches in torch.
 *   - NaN is not silent and not contagious: a NaN in an input row reaches that row's mu (and sigma) or values only, and through the
 *     backward every parameter gradient that torch's would reach; no other row's output changes a bit.
 *   - No float atomics and no hand-off between workgroups inside a launch: two calls on the same inputs give the same bits.
 *   - All addressing of the workspace and of ragged tiles is on clamped indices: no out-of-range row or column is read or stored.
 */
#ifndef LGTRAIN_H
#define LGTRAIN_H

#include <stdint.h>
#include "lgpolicy.h"   /* LG_POLICY_MAX_LAYERS, LG_POLICY_MAX_WIDTH */

#ifdef __cplusplus
extern "C" {
#endif

#define LG_TRAIN_CHAINS 2            /* 0 the actor, 1 the critic */
#define LG_TRAIN_ACTOR 0
#define LG_TRAIN_CRITIC 1
/* The weight-gradient plan.  One wave owns a LG_TRAIN_WG_TILE x LG_TRAIN_WG_TILE tile of a layer's (out x in) gradient over one batch
 * slice.  Layer l of tiles_l = ceil(out / 64) * ceil(in / 64) tiles gets
 *     want_l  = min(max(1, floor(n_rows / LG_TRAIN_MIN_SLICE_ROWS)), max(1, floor(LG_TRAIN_TARGET_JOBS / tiles_l)), LG_TRAIN_MAX_SLICES)
 *     slice_rows_l = ceil(n_rows / want_l) rounded up to a multiple of 4,   slices_l = ceil(n_rows / slice_rows_l)
 * so that slices_l * tiles_l waves fill the chip with slice_rows_l never below 64 where there is more than one slice; grad_std counts as a layer of one tile. */
#define LG_TRAIN_WG_TILE 64
#define LG_TRAIN_MIN_SLICE_ROWS 64
#define LG_TRAIN_TARGET_JOBS 512
#define LG_TRAIN_MAX_SLICES 32

typedef struct LgTrainLayer {
    const float *weight;       /* (n_out, n_in) row-major, contiguous */
    const float *bias;         /* (n_out) */
    float *grad_weight;        /* (n_out, n_in), overwritten by lg_train_backward */
    float *grad_bias;          /* (n_out), overwritten */
    int32_t n_in;
    int32_t n_out;
    int32_t elu;
    int32_t reserved;
} LgTrainLayer;

typedef struct LgTrainChain {
    const float *input;        /* (n_rows, layer[0].n_in), in_stride floats between rows */
    int32_t in_stride;
    int32_t n_layers;          /* 1 .. LG_POLICY_MAX_LAYERS */
    LgTrainLayer layer[LG_POLICY_MAX_LAYERS];
} LgTrainChain;

typedef struct LgTrainArgs {
    int32_t n_rows;
    int32_t clip_on;
    float clip_actions;        /* Hardtanh(+-clip_actions) behind the actor's last layer when clip_on */
    int32_t reserved;
    LgTrainChain chain[LG_TRAIN_CHAINS];
    const float *std;          /* (A), A = the actor's last n_out */
    float *grad_std;           /* (A), overwritten by lg_train_backward */
    float *mu;                 /* (n_rows, A): written by forward, read by backward (the Hardtanh mask) */
    float *sigma;              /* (n_rows, A) */
    float *values;             /* (n_rows, V), V = the critic's last n_out */
    const float *grad_mu;      /* (n_rows, A): backward only, like the next two */
    const float *grad_sigma;   /* (n_rows, A) */
    const float *grad_values;  /* (n_rows, V) */
    int32_t mu_stride, sigma_stride, values_stride;
    int32_t grad_mu_stride, grad_sigma_stride, grad_values_stride;
    float *workspace;          /* LgTrainPlan::workspace_floats floats: forward writes the activations, backward reads them and writes
                                  the rest.  The backward of a forward must see the workspace (and mu) that forward left. */
    int64_t workspace_capacity;   /* floats available at `workspace` */
} LgTrainArgs;

/* What the launches of a descriptor do, a pure function of n_rows and the widths.  Offsets are in floats from `workspace`.
 *   h_off[c][l]   H_l of chain c, (n_rows, n_out_l) dense, for l < n_layers - 1 (the last layer's output is mu / values); -1 otherwise
 *   g_off[c][l]   G_l, (n_rows, n_out_l) dense, for every layer
 *   p_off[c][l]   slices[c][l] slabs of n_out * n_in + n_out floats: the partial grad_weight, then the partial grad_bias, of one slice
 *   std_p_off     std_slices slabs of A floats */
typedef struct LgTrainPlan {
    int32_t row_tile;          /* rows of one workgroup of the forward and of the input-gradient launch: 32, 16 or 8 */
    int32_t lds_bytes;         /* of those two launches */
    int32_t slices[LG_TRAIN_CHAINS][LG_POLICY_MAX_LAYERS];
    int32_t slice_rows[LG_TRAIN_CHAINS][LG_POLICY_MAX_LAYERS];
    int32_t std_slices, std_slice_rows;
    int32_t weight_jobs;       /* waves (workgroups of 64 lanes) of the weight-gradient launch */
    int32_t reserved;
    int64_t h_off[LG_TRAIN_CHAINS][LG_POLICY_MAX_LAYERS];
    int64_t g_off[LG_TRAIN_CHAINS][LG_POLICY_MAX_LAYERS];
    int64_t p_off[LG_TRAIN_CHAINS][LG_POLICY_MAX_LAYERS];
    int64_t std_p_off;
    int64_t workspace_floats;
} LgTrainPlan;

/* Touches no device and reads no pointer of the descriptor: n_rows, n_layers, n_in, n_out only.  Refused (non-zero, last error set): a
 * null descriptor or plan, n_rows < 1, a layer count outside [1, LG_POLICY_MAX_LAYERS], a width outside [1, LG_POLICY_MAX_WIDTH], widths
 * that do not chain, a row tile of 8 that does not fit the 160 KB of LDS. */
int lg_train_plan(const LgTrainArgs *args, LgTrainPlan *out);

/* One launch: a workgroup carries row_tile rows through every layer of one chain in LDS (the row-tile scheme of lg_policy_act: MFMA
 * 16x16x4 f32, ragged K, M and rows on clamped addresses), stores every hidden activation to the workspace and writes mu, sigma, values.
 * Refused before the launch, with a message that names the member: what lg_train_plan refuses, a null weight, bias, input, std, mu,
 * sigma, values or workspace, a stride below its width, clip_on with clip_actions not >= 0, workspace_capacity below the plan. */
int lg_train_forward(const LgTrainArgs *args, void *stream);

/* Three launches on `stream`: the input gradients (row-tile ownership, last layer to second; every G_l to the workspace), the weight
 * gradients (per layer, output tile and batch slice one wave; float32 partials per slice, grad_bias and grad_std riding along), the
 * combine (the partials of every element summed in slice order).  Refused before any launch: what lg_train_forward refuses, a null
 * grad_weight, grad_bias, grad_std, grad_mu, grad_sigma or grad_values, a gradient stride below its width. */
int lg_train_backward(const LgTrainArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LGTRAIN_H */

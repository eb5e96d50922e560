/* lgtraintcn.h -- C ABI of the supervised history-encoder pass of PPO_TS.update() (rsl_rl/algorithms/ppo_ts.py:174-187) where ActorCriticTS
 * builds its history encoder with history_encoder_type = "TCN" (rsl_rl/modules/actor_critic_ts.py:61-99): a stack of nn.Conv1d with no
 * activation between them, nn.Flatten, then a Linear / ELU chain (the "tail").  Same contract as lgtraints.h, whose chain structs are
 * reused: plain device pointers and row strides in floats, the caller's HIP stream as void*; 0 on success, otherwise non-zero with the
 * message in lgsim.h's last-error call; nothing is allocated, nothing synchronised.  Everything stored is float32; the sums of the conv
 * kernels (a forward output's taps, an input gradient's taps and channels, a weight gradient's rows) run in float64 and are rounded once.  Weights are read in place on
 * every call.  The RL pass of such a module has no history chain at all: it is lgtraints.h's lg_train_ts_* unchanged.
 *
 * Per row:   x_0 = obs_history as (1, H);   x_l = conv_l(x_(l-1)), l = 1 .. n_conv, with
 *              x_l[o][t] = bias[o] + sum_i sum_k W[o][i][k] x_(l-1)[i][t * stride + k * dilation - padding]   (taps outside [0, L_(l-1)) are 0),
 *              L_l = floor((L_(l-1) + 2 padding - dilation (kernel - 1) - 1) / stride) + 1;
 *   f = flatten(x_n), channel-major: f[c * L_n + t] = x_n[c][t], F = C_n L_n columns;   p = tail(f);
 *   y = privilege_encoder(privileged_obs), a constant of this pass;   d = (p - y) * mask;   loss = sum d^2 / (n_rows * Z), the float64
 *   ordered sum of lgtraints.h's encoder pass;   d loss / d p = 2 d mask / (n_rows * Z), scaled in the backward by the scalar at `upstream`.
 *
 * Limits (constants below): at most LG_TRAIN_TCN_MAX_CONV conv layers (the module's default depth), channels 1 .. 32 with the first c_in =
 * 1, kernel 1 .. 9, stride 1 .. 4, dilation 1 .. 8, 0 <= padding <= dilation (kernel - 1), H <= LG_POLICY_MAX_WIDTH, every L_l >= 1, and
 * F <= LG_POLICY_MAX_WIDTH because the tail's first operand is a row tile in LDS.  The module's own default does NOT fit: six layers of 30
 * channels on H = 900 give F = 30 * 113 = 3390 > 2048; it is refused by name with the number.
 *
 * Conventions:
 *   - The forward STORES every x_l, l = 1 .. n_conv, in the workspace (x_n is f); the backward recomputes nothing.  x_0 is read from
 *     `history` again by the weight gradient of conv 0.
 *   - Gradients go to the conv layers and the tail only.  The first conv computes no input gradient (there is none for obs_history); the
 *     privilege encoder's grad_weight / grad_bias are never read.  The tail's layer 0 does compute an input gradient, G_f, with no ELU
 *     factor: f is no activation.
 *   - The upstream scalar is read on the device and applied when gl is staged by the backward: gl survives, a forward can be differentiated
 *     more than once.
 *   - No float atomics, no hand-off between workgroups inside a launch; every sum has a fixed order: two calls on the same inputs give the
 *     same bits.  Gradients are overwritten (accumulation is autograd's job).  Addresses are clamped on ragged tiles.  A NaN in one history
 *     row changes no other row's f or gl.
 *   - The conv weight gradient: per layer E = c_out c_in kernel + c_out elements (the weight, then the bias).  A workgroup of
 *     LG_TRAIN_TCN_THREADS threads takes LG_TRAIN_TCN_WG_ELEMS elements of one batch slice: 32 lanes per element, lane j sums the positions
 *     t = j, j + 32, ... of a row into a float32 row partial, adds the row partials in row order in float64 (a bias gradient is a sum of
 *     n_rows L terms of both signs: the cancellation would otherwise cost digits that torch's blocked sums keep), and the 32 lane sums are
 *     added by a fixed binary tree in float64 and rounded to float32 once.  The slice rule is lgtrain.h's with tiles = ceil(E / LG_TRAIN_TCN_WG_ELEMS) and LG_TRAIN_TCN_TARGET_JOBS:
 *         want = min(max(1, n_rows / 64), max(1, 2048 / tiles), 32);  rows per slice = ceil(n_rows / want) rounded up to 4;
 *         slices = ceil(n_rows / rows per slice).
 *     The combine adds the slice partials in slice order.
 *   - The conv forward and input-gradient launches give each workgroup a block of conv_block_rows = ceil(n_rows / min(n_rows,
 *     LG_TRAIN_TCN_MAX_BLOCKS)) consecutive rows; it carries them layer by layer (one layer's weights in LDS at a time) and reads back only
 *     rows it wrote itself, behind a barrier.
 */
#ifndef LGTRAINTCN_H
#define LGTRAINTCN_H

#include <stdint.h>
#include "lgtrain.h"   /* LgTrainLayer, LgTrainChain, the slice rule's constants */

#ifdef __cplusplus
extern "C" {
#endif

#define LG_TRAIN_TCN_MAX_CONV 6
#define LG_TRAIN_TCN_MAX_CHANNELS 32
#define LG_TRAIN_TCN_MAX_KERNEL 9
#define LG_TRAIN_TCN_MAX_STRIDE 4
#define LG_TRAIN_TCN_MAX_DILATION 8
#define LG_TRAIN_TCN_TARGET_JOBS 2048   /* as LG_TRAIN_TS_TARGET_JOBS: of the tail's slice rule and of the conv weight gradient's */
#define LG_TRAIN_TCN_THREADS 256        /* of every row-tile and conv workgroup; the leaves of the loss partial's tree */
#define LG_TRAIN_TCN_WG_ELEMS 8         /* gradient elements per workgroup of the conv weight-gradient launch: 32 lanes each */
#define LG_TRAIN_TCN_MAX_BLOCKS 2048    /* workgroups of the conv forward and input-gradient launches */

typedef struct LgTrainConv {
    const float *weight;       /* (c_out, c_in, kernel), contiguous */
    const float *bias;         /* (c_out) */
    float *grad_weight;        /* backward only, overwritten */
    float *grad_bias;
    int32_t c_in, c_out, kernel, stride, padding, dilation;
} LgTrainConv;

typedef struct LgTrainTcnArgs {
    int32_t n_rows;
    int32_t mask_stride;       /* floats between the rows of the (n_rows, 1) mask, >= 1 */
    int32_t n_conv;            /* 1 .. LG_TRAIN_TCN_MAX_CONV */
    int32_t n_history;         /* H, the length of x_0 */
    LgTrainConv conv[LG_TRAIN_TCN_MAX_CONV];
    const float *history;      /* (n_rows, H) */
    int32_t history_stride;    /* floats between its rows, >= H */
    int32_t reserved;
    LgTrainChain tail;         /* layer[0].n_in = F; its input / in_stride are ignored: the tail reads f from the workspace */
    LgTrainChain privilege;    /* input: the privileged observations (n_rows, P); its gradient pointers are never read */
    const float *mask;         /* (n_rows, 1): `terminated` */
    float *loss;               /* one float, written by lg_train_tcn_forward */
    const float *upstream;     /* one float on the device; backward only */
    float *workspace;          /* LgTrainTcnPlan::workspace_floats floats, 8-byte aligned (it holds the float64 partials) */
    int64_t workspace_capacity;
} LgTrainTcnArgs;

/* A pure function of n_rows, n_history, the conv shapes and the chains' widths.  Offsets in floats from `workspace`; -1 where there is none.
 *   length[l]       L_l, l = 0 .. n_conv (length[0] = H); flat = F
 *   x_off[l]        x_l, (n_rows, C_l L_l) dense, l = 1 .. n_conv; x_off[n_conv] is f, the tail's input
 *   cg_off[l]       G_l = d loss / d x_l, same shape, l = 1 .. n_conv; cg_off[n_conv] is G_f, written by the tail's input-gradient launch
 *   conv_p_off[l]   conv_slices[l] slabs of E_l floats, layer l = 0 .. n_conv - 1 (zero-based here and in conv_slices / conv_slice_rows)
 *   h_off / g_off / p_off / slices / slice_rows: the tail's layers, as LgTrainTSPlan's
 *   gl_off, y_off, partial_off, loss_tiles: as LgTrainTSPlan's encoder pass */
typedef struct LgTrainTcnPlan {
    int32_t row_tile;          /* 32, 16 or 8: of the tail's launches, the largest whose two LDS activations fit beside the loss tree */
    int32_t lds_bytes;
    int32_t n_conv, flat;
    int32_t length[LG_TRAIN_TCN_MAX_CONV + 1];
    int32_t conv_block_rows, conv_blocks;
    int32_t conv_jobs;         /* workgroups of the conv weight-gradient launch */
    int32_t conv_slices[LG_TRAIN_TCN_MAX_CONV];
    int32_t conv_slice_rows[LG_TRAIN_TCN_MAX_CONV];
    int32_t conv_job0[LG_TRAIN_TCN_MAX_CONV];
    int32_t slices[LG_POLICY_MAX_LAYERS];
    int32_t slice_rows[LG_POLICY_MAX_LAYERS];
    int32_t weight_jobs;       /* waves of the tail's weight-gradient launch */
    int32_t loss_tiles;
    int64_t x_off[LG_TRAIN_TCN_MAX_CONV + 1];
    int64_t cg_off[LG_TRAIN_TCN_MAX_CONV + 1];
    int64_t conv_p_off[LG_TRAIN_TCN_MAX_CONV];
    int64_t h_off[LG_POLICY_MAX_LAYERS];
    int64_t g_off[LG_POLICY_MAX_LAYERS];
    int64_t p_off[LG_POLICY_MAX_LAYERS];
    int64_t gl_off;
    int64_t y_off;
    int64_t partial_off;
    int64_t workspace_floats;
} LgTrainTcnPlan;

/* Touches no device and reads no pointer.  Refused, naming the layer and the field: a null descriptor or plan, n_rows < 1, n_conv outside
 * [1, 6], n_history outside [1, LG_POLICY_MAX_WIDTH], conv[0].c_in other than 1, a c_in that is not the c_out before it, any conv field
 * outside the limits above, an L_l < 1, F above LG_POLICY_MAX_WIDTH, tail.layer[0].n_in other than F, what lg_train_enc_plan refuses of
 * the two chains, the two encoders' output widths differing. */
int lg_train_tcn_plan(const LgTrainTcnArgs *args, LgTrainTcnPlan *out);

/* Three launches: the conv stack from `history` into the workspace; per row tile the privilege encoder (nothing stored but y), the tail
 * from f (hidden activations stored), gl and one float64 partial per tile; the one-workgroup finalize that writes *loss.  Refused before
 * any launch: what the plan refuses, a null history, weight, bias, privilege input, mask, loss or workspace, a stride below its width, a
 * workspace that is not 8-byte aligned, workspace_capacity below the plan. */
int lg_train_tcn_forward(const LgTrainTcnArgs *args, void *stream);

/* Five launches: the tail's input gradients through its layer 0 into G_f (gl scaled by *upstream); the conv input gradients from the last
 * conv down to the second; the tail's weight gradients; the convs' weight and bias gradients; the combine.  Refused before any launch:
 * what the forward refuses but a null loss, a null upstream, grad_weight or grad_bias of a conv or a tail layer. */
int lg_train_tcn_backward(const LgTrainTcnArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LGTRAINTCN_H */

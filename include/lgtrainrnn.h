/* lgtrainrnn.h -- C ABI of the fused learner pass of the recurrent family: the training forward of ActorCriticRecurrent
 * (rsl_rl/modules/actor_critic_recurrent.py: memory_a -> actor, memory_c -> critic, each memory an nn.LSTM or nn.GRU of one or two layers
 * run over the padded trajectories of a mini-batch, unpad_trajectories, then the plain ActorCritic's two chains) and its backward through
 * the chains, through time and into every parameter of the memories.  Conventions are lgtrain.h's: plain device pointers and strides in
 * floats, the caller's HIP stream as void*; 0 on success, otherwise non-zero with the message in lgsim.h's last-error call; nothing is
 * allocated, nothing synchronised; everything is float32; gradients are OVERWRITTEN; no gradient for the observations or the start states.
 * The memories' parameters are read where torch keeps them: weight_ih_l{k} (G H, in), weight_hh_l{k} (G H, H), bias_ih_l{k}, bias_hh_l{k}
 * (G H), G = 4 with gate order i, f, g, o for an LSTM and G = 3 with r, z, n for a GRU.
 *
 * Rows.  The mini-batch is n_traj trajectories cut from T steps of E envs (E = train.n_rows / T).  x is (max_len, n_traj, in) with a time
 * stride and a row stride; mask is (T, n_traj) bytes (torch.bool) with a time stride: mask[t][j] != 0 for t < len_j.  THE MASK CONTRACT:
 * every column of the mask is a prefix of ones (its sum is len_j <= max_len), the trajectories are in env-major order and the lengths of
 * the trajectories of one env add up to T, as split_and_pad_trajectories produces them.  With s_j the sum of the lengths before j, step t
 * of trajectory j is step s_j % T + t of env s_j / T and has the UNPADDED ROW (s_j % T + t) E + s_j / T: the order of
 * unpad_trajectories(...).flatten(0, 1).  A mask outside the contract is the caller's error and cannot be checked without a host sync;
 * every row index it produces is clamped into [0, n_rows), so nothing is read or stored out of range, but the results are unspecified.
 * Padding (t >= len_j) is never read: what it holds (NaN included) reaches nothing.
 *
 * Forward, per memory, layer k and valid (j, t), with x_t the observation row (k = 0) or the layer below's h_t, h_-1 / c_-1 the start
 * states (L, n_traj, H):
 *   LSTM   a = W_ih x_t + b_ih + (W_hh h_(t-1) + b_hh);  i, f, o = sigmoid, g = tanh;  c_t = f c_(t-1) + i g;  h_t = o tanh(c_t)
 *   GRU    r, z = sigmoid(W_i x_t + b_i + (W_h h_(t-1) + b_h));  n = tanh(W_in x_t + b_in + r (W_hn h_(t-1) + b_hn));  h_t = (1 - z) n + z h_(t-1)
 * The top layer's h_t, at its unpadded row, is the input row of the memory's chain (train.chain[c].input is not read).  mu, sigma and
 * values are lgtrain.h's, (n_rows, A), (n_rows, A), (n_rows, V) in unpadded row order.
 * Backward: lgtrain.h's over the chains, continued through layer 0 of each chain into d loss / d h_t of the top layer; through time from
 * each trajectory's last step down to 0 with sigmoid' = s (1 - s) and tanh' = 1 - y^2 from the stored outputs; grad_weight_ih = sum D_t^T
 * x_t, grad_weight_hh = sum D_t^T h_(t-1), the bias gradients the column sums of D (a GRU's W_hn / b_hn take r D_n), over the n_rows
 * unpadded rows in lgtrain.h's slices, float32 partials per slice combined in slice order.
 * No float atomics, no hand-off between workgroups inside a launch: two calls on the same inputs give the same bits.
 */
#ifndef LGTRAINRNN_H
#define LGTRAINRNN_H

#include <stdint.h>
#include "lgtrain.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LG_TRAIN_RNN_MEMORIES 2          /* 0 memory_a (feeds the actor), 1 memory_c (feeds the critic) */
#define LG_TRAIN_RNN_MAX_LAYERS 2        /* LG_POLICY_MAX_RNN_LAYERS */
#define LG_TRAIN_RNN_MAX_HIDDEN 512      /* LG_POLICY_MAX_RNN_HIDDEN */
#define LG_TRAIN_RNN_LSTM 1              /* LG_POLICY_LSTM */
#define LG_TRAIN_RNN_GRU 2               /* LG_POLICY_GRU */
#define LG_TRAIN_RNN_TARGET_JOBS 2048    /* the weight-gradient job target of this pass (lgtrain.h's slice rule) */

typedef struct LgTrainRnnLayer {
    const float *weight_ih, *weight_hh, *bias_ih, *bias_hh;
    float *grad_weight_ih, *grad_weight_hh, *grad_bias_ih, *grad_bias_hh;     /* backward only, overwritten */
} LgTrainRnnLayer;

typedef struct LgTrainRnnMemory {
    int32_t kind;              /* LG_TRAIN_RNN_LSTM or LG_TRAIN_RNN_GRU */
    int32_t n_layers;          /* 1 .. LG_TRAIN_RNN_MAX_LAYERS */
    int32_t hidden;            /* H, 1 .. LG_TRAIN_RNN_MAX_HIDDEN; the memory's chain has layer[0].n_in = H */
    int32_t n_in;              /* 1 .. LG_POLICY_MAX_WIDTH */
    LgTrainRnnLayer layer[LG_TRAIN_RNN_MAX_LAYERS];
    const float *x;            /* (max_len, n_traj, n_in) */
    int64_t x_time_stride, x_row_stride;
    const float *h0;           /* (n_layers, n_traj, H) start states */
    const float *c0;           /* the same for an LSTM's cell state; not read for a GRU */
    int64_t h0_layer_stride, h0_row_stride, c0_layer_stride, c0_row_stride;
    const uint8_t *mask;       /* (T, n_traj) bytes; both memories name the same mask */
    int64_t mask_time_stride;  /* in bytes */
    int32_t max_len, n_traj, T, reserved;
} LgTrainRnnMemory;

typedef struct LgTrainRnnArgs {
    LgTrainArgs train;         /* n_rows = T E, the two chains (their `input` / `in_stride` are not read), the heads, the workspace */
    LgTrainRnnMemory memory[LG_TRAIN_RNN_MEMORIES];
} LgTrainRnnArgs;

/* A pure function of the sizes.  `train` is lgtrain.h's plan of the two chains over n_rows rows (its offsets lie behind the memories'
 * regions; its weight_jobs counts the chains' jobs and grad_std's).  Per memory m and layer k, offsets in floats from `workspace`, every
 * region (n_rows, .) dense in unpadded row order:
 *   gate_off   (n_rows, G H): W_ih x + b_ih from the input launch, overwritten by the activated gates by the time loop
 *   h_off      (n_rows, H) h_t;   hprev_off (n_rows, H) h_(t-1);   c_off (LSTM) c_t;   nh_off (GRU) W_hn h_(t-1) + b_hn
 *   dout_off   (n_rows, H) d loss / d h_t from above (the chain's input gradient or the upper layer's input gradient)
 *   dx_off     (n_rows, G H) D_t as W_ih / b_ih see it;   dh_off (GRU) as W_hh / b_hh see it (r D_n in the n block); -1 for an LSTM
 *   p_off[.][.][w], slices, slice_rows: the slice partials of (weight_ih, bias_ih) (w = 0) and (weight_hh, bias_hh) (w = 1)
 * index_off: n_traj lengths, n_traj first rows, n_rows source indices t n_traj + j, int32. */
typedef struct LgTrainRnnPlan {
    LgTrainPlan train;
    int32_t time_row_tile;     /* trajectories of one workgroup of the time-loop launches: 32, 16 or 8 */
    int32_t time_lds_bytes;
    int32_t time_tiles;        /* ceil(n_traj / time_row_tile) */
    int32_t n_envs;            /* E */
    int32_t weight_jobs;       /* all waves of the weight-gradient launch */
    int32_t reserved;
    int32_t slices[LG_TRAIN_RNN_MEMORIES][LG_TRAIN_RNN_MAX_LAYERS][2];
    int32_t slice_rows[LG_TRAIN_RNN_MEMORIES][LG_TRAIN_RNN_MAX_LAYERS][2];
    int64_t gate_off[LG_TRAIN_RNN_MEMORIES][LG_TRAIN_RNN_MAX_LAYERS];
    int64_t h_off[LG_TRAIN_RNN_MEMORIES][LG_TRAIN_RNN_MAX_LAYERS];
    int64_t hprev_off[LG_TRAIN_RNN_MEMORIES][LG_TRAIN_RNN_MAX_LAYERS];
    int64_t c_off[LG_TRAIN_RNN_MEMORIES][LG_TRAIN_RNN_MAX_LAYERS];
    int64_t nh_off[LG_TRAIN_RNN_MEMORIES][LG_TRAIN_RNN_MAX_LAYERS];
    int64_t dout_off[LG_TRAIN_RNN_MEMORIES][LG_TRAIN_RNN_MAX_LAYERS];
    int64_t dx_off[LG_TRAIN_RNN_MEMORIES][LG_TRAIN_RNN_MAX_LAYERS];
    int64_t dh_off[LG_TRAIN_RNN_MEMORIES][LG_TRAIN_RNN_MAX_LAYERS];
    int64_t p_off[LG_TRAIN_RNN_MEMORIES][LG_TRAIN_RNN_MAX_LAYERS][2];
    int64_t index_off;
    int64_t workspace_floats;
} LgTrainRnnPlan;

/* Touches no device and reads no pointer.  Refused: what lg_train_plan refuses, a kind, layer count, hidden size or input width outside
 * its range, a chain whose layer[0].n_in is not its memory's H, max_len, n_traj or T below 1, max_len above T, sizes that differ between
 * the two memories, n_rows that is no multiple of T or below T (more envs than trajectories), a tile of 8 that does not fit the LDS. */
int lg_train_rnn_plan(const LgTrainRnnArgs *args, LgTrainRnnPlan *out);

/* 2 + 2 L launches on `stream` (L = the larger layer count): the trajectory prologue (one workgroup: lengths, first rows, source
 * indices), per layer the input launch (W_ih x + b_ih over row tiles of the unpadded rows) and the time loop (a workgroup owns
 * time_row_tile trajectories of one memory and walks t inside the kernel), then lgtrain.h's forward launch on the top layers' h.
 * Refused before any launch: what the plan refuses, a null pointer, a stride below its width, two memories with different masks. */
int lg_train_rnn_forward(const LgTrainRnnArgs *args, void *stream);

/* 3 + 2 L - 1 launches: the chains' input gradients on through layer 0, per layer from the top the time loop backwards and (above layer
 * 0) the input gradient D W_ih for the layer below, the weight gradients of chains and memories in one launch, the combine. */
int lg_train_rnn_backward(const LgTrainRnnArgs *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LGTRAINRNN_H */

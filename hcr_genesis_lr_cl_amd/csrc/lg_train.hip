// lg_train.hip -- the fused learner pass behind include/lgtrain.h: the training forward of the plain ActorCritic and its backward.
//
// Reference call sites replaced: rsl_rl/algorithms/ppo.py:124-148 (PPO.update: actor_critic.act / evaluate on the mini-batch, and the
// share of loss.backward() that runs through the two MLPs) on rsl_rl/modules/actor_critic.py:57-123.
//
// Forward and input gradients use the row-tile scheme of lg_policy.hip (whose layer routine is COPIED into lg_train_tiles.h, cut down to one operand, so
// that policy_act_kernel keeps its registers): a workgroup (4 waves) owns R rows (32, 16 or 8: the largest whose two ping-pong
// activations fit the 160 KB LDS) and carries them through every layer of one chain (blockIdx.y).  One v_mfma_f32_16x16x4_f32 computes
// D[i][j] += sum_k A[i][k] B[k][j]; lane (r = lane & 15, h = lane >> 4) supplies A[r][h], B[h][r] and receives D[4h .. 4h+3][r].
//   forward         A = W (i = output neuron, k = input), B = X^T (j = row); a lane reads k = k0 + 4h .. + 3 as 16 bytes of both operands
//                   and feeds element e to the e-th of four MFMAs (the k order inside a 16-wide chunk is permuted, the products are the same)
//   input gradient  A = W^T (i = INPUT index of the layer, k = its output neuron n), B = G^T: the lane reads G[row r][n0 + 4h .. + 3] as 16
//                   bytes from LDS and, for MFMA e, W[n0 + 4h + e][k0 + r]: 16 lanes read 64 consecutive bytes of one weight row
//   weight gradient A = G^T (i = output neuron, k = batch row), B = H (j = input index): the lane reads G[row0 + h][n0 + r] and
//                   H[row0 + h][k0 + r], both coalesced over r.  One wave (a workgroup of 64 lanes) holds 4 x 4 accumulator tiles, a 64 x 64
//                   tile of the gradient, over one batch slice; rows behind the slice read as zero ON BOTH OPERANDS from clamped
//                   addresses, neurons and inputs behind the widths are computed on clamped addresses and never stored.
// The partials of a slice are plain stores into that slice's slab; the combine launch adds the slabs in slice order.  No atomics.
#include "lg_train_pass.h"    // the chain, plan, bind and launch routines, shared with lg_train_ee.hip and lg_train_ts.hip

struct TArgs : PArgs {
    TChain c[LG_TRAIN_CHAINS];
};
static_assert(sizeof(TArgs) <= 4096, "TArgs is passed by value: the kernel-argument segment is 4 KB");

template <int RB> __global__ __launch_bounds__(256) void train_forward_kernel(TArgs a) {
    extern __shared__ __align__(16) float lds[];
    const TChain &c = a.c[blockIdx.y];
    const int R = a.R, row0 = blockIdx.x * R;
    const int rows = min(R, a.N - row0);
    const bool actor = blockIdx.y == LG_TRAIN_ACTOR;
    const lds_f *m = chain_from_rows<RB>(a.ws, c, (lds_f *)lds, (lds_f *)lds + a.q_off, true, actor && a.clip_on, a.clip, R, rows, row0);
    const int sm = c.l[c.n_layers - 1].so;
    copy_out(m, sm, c.out, c.l[c.n_layers - 1].M, c.out_stride, rows, row0);
    if (actor) store_sigma(m, sm, a.A, a.std, a.sigma, a.sigma_stride, rows, row0);
}

template <int RB> __global__ __launch_bounds__(256) void train_input_grad_kernel(TArgs a) {
    extern __shared__ __align__(16) float lds[];
    const TChain &c = a.c[blockIdx.y];
    const int R = a.R, row0 = blockIdx.x * R;
    const int rows = min(R, a.N - row0);
    lds_f *b0 = (lds_f *)lds, *b1 = (lds_f *)lds + a.q_off;
    seed_last_g(a.ws, c, (c.n_layers & 1) ? b1 : b0, nullptr, nullptr, blockIdx.y == LG_TRAIN_ACTOR && a.clip_on, a.clip, R, rows, row0);
    __syncthreads();
    chain_backward<RB>(a.ws, c, b0, b1, R, rows, row0);
}

__global__ __launch_bounds__(64) void train_weight_grad_kernel(TArgs a) { wgrad_job(a, a.c, 0, LG_TRAIN_CHAINS); }

__global__ __launch_bounds__(256) void train_combine_kernel(TArgs a) { combine_all(a, a.c, 0, LG_TRAIN_CHAINS); }

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static const char *kChain[LG_TRAIN_CHAINS] = {"chain[0] (actor)", "chain[1] (critic)"};
static void (*const kForward[2])(TArgs) = {train_forward_kernel<1>, train_forward_kernel<2>};
static void (*const kInputGrad[2])(TArgs) = {train_input_grad_kernel<1>, train_input_grad_kernel<2>};
static bool raised_forward[2][64], raised_input_grad[2][64];

// the plan from the shapes alone; fills the shape part of `k` too
static int make_plan(const char *fn, const LgTrainArgs *p, LgTrainPlan &pl, TArgs &k) {
    const std::string f(fn);
    if (check_desc(f, p)) return 1;
    pl = LgTrainPlan{};
    k = TArgs{};
    int w[2] = {0, 0};
    for (int ci = 0; ci < LG_TRAIN_CHAINS; ci++)
        if (plan_chain(f + ": " + kChain[ci], p->chain[ci], k.c[ci], 0, w)) return 1;
    PassLayout lay;
    if (plan_layout(f, k, k.c, p->n_rows, 0, LG_TRAIN_CHAINS, LG_TRAIN_ACTOR, LG_TRAIN_TARGET_JOBS, w, 0, false, 0, lay)) return 1;
    plan_out(pl, k, k.c, lay);
    return 0;
}

// the pointers and strides; `backward`: the gradient members too
static int bind(const char *fn, const LgTrainArgs *p, const LgTrainPlan &pl, TArgs &k, bool backward) {
    const std::string f(fn);
    for (int ci = 0; ci < LG_TRAIN_CHAINS; ci++)
        if (bind_chain(f + ": " + kChain[ci], p->chain[ci], k.c[ci], p->chain[ci].layer[0].n_in, backward)) return 1;
    return bind_heads(f, p, k, k.c[LG_TRAIN_ACTOR], k.c[LG_TRAIN_CRITIC], pl.workspace_floats, backward);
}

extern "C" int lg_train_plan(const LgTrainArgs *args, LgTrainPlan *out) {
    if (!out) return lg_fail_msg("lg_train_plan: null plan");
    TArgs k;
    return make_plan("lg_train_plan", args, *out, k);
}

extern "C" int lg_train_forward(const LgTrainArgs *args, void *stream) {
    static const char *fn = "lg_train_forward";
    LgTrainPlan pl; TArgs k;
    if (make_plan(fn, args, pl, k) || bind(fn, args, pl, k, false)) return 1;
    return launch_tile(fn, kForward, raised_forward, LG_TRAIN_CHAINS, pl.lds_bytes, (hipStream_t)stream, k) || done(fn);
}

extern "C" int lg_train_backward(const LgTrainArgs *args, void *stream) {
    static const char *fn = "lg_train_backward";
    LgTrainPlan pl; TArgs k;
    if (make_plan(fn, args, pl, k) || bind(fn, args, pl, k, true)) return 1;
    return launch_backward(fn, kInputGrad, raised_input_grad, train_weight_grad_kernel, train_combine_kernel, LG_TRAIN_CHAINS, pl.lds_bytes, (hipStream_t)stream, k);
}

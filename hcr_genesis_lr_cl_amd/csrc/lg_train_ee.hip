// lg_train_ee.hip -- the fused learner passes of the explicit-estimator family behind include/lgtrainee.h: the RL pass of ActorCriticEE
// (estimator -> [features | est] -> actor, and the critic) with its backward over the actor and the critic, and the supervised estimator
// pass (chain, masked mean-squared error, backward).
//
// Reference call sites replaced: rsl_rl/algorithms/ppo_ee.py:141-175 (_compute_rl_loss's network calls, _compute_estimator_loss) and the
// share of the two loss.backward() calls of PPO_EE.update() (ppo_ee.py:108-131) that runs through the three MLPs of
// rsl_rl/modules/actor_critic_ee.py:39-79,115-133.
//
// The layer routines are lg_train_tiles.h's (the MFMA layouts are described in lg_train.hip), the chain, loss, plan and launch routines
// lg_train_pass.h's.  What is this family's own:
//   RL forward        grid (row tiles, 2).  y = 0: features -> LDS, the estimator chain ping-pongs so that its output ends in activation 1,
//                     the features are staged again (L2-resident) into activation 0 at the actor's stride with the estimator's output
//                     copied behind them, the concatenation goes to the workspace while the actor's first layer reads it.  y = 1: the critic.
//   estimator forward the chain, then per tile d = (p - y) t, gl = 2 d t / (N NL) to the workspace and the tile's float64 sum of d^2 by
//                     a fixed tree; a one-workgroup launch adds the tile partials in tile order.
//   backward          the three launches of lg_train.hip over the chains [c0, c1) of the pass: actor and critic, or the estimator alone
//                     (whose staged gl is scaled by the upstream scalar, read on the device).
// Plain stores only; two calls on the same inputs give the same bits.
#include "lg_train_pass.h"
#include "../../include/lgtrainee.h"

#define EST LG_TRAIN_EE_ESTIMATOR
#define ACT LG_TRAIN_EE_ACTOR
#define CRI LG_TRAIN_EE_CRITIC
static const int kRedBytes = LG_TRAIN_EE_THREADS * (int)sizeof(double);
static_assert(LG_TRAIN_EE_THREADS == kThreads, "the loss tree has one leaf per thread of the row-tile workgroup");

struct EArgs : PArgs {
    TChain c[LG_TRAIN_EE_CHAINS];
    const float *labels, *mask, *upstream;
    float *loss;
    int labels_stride, mask_stride;
    int est_start, est_pass;
    long long cat_off, gl_off, part_off;
};
static_assert(sizeof(EArgs) <= 4096, "EArgs is passed by value: the kernel-argument segment is 4 KB");

template <int RB> __global__ __launch_bounds__(256) void train_ee_forward_kernel(EArgs a) {
    extern __shared__ __align__(16) float lds[];
    const int R = a.R, row0 = blockIdx.x * R;
    const int rows = min(R, a.N - row0);
    lds_f *b0 = (lds_f *)lds, *b1 = (lds_f *)lds + a.q_off;
    if (blockIdx.y == 1) {
        const TChain &c = a.c[CRI];
        const lds_f *v = chain_from_rows<RB>(a.ws, c, b0, b1, true, false, a.clip, R, rows, row0);
        copy_out(v, c.l[c.n_layers - 1].so, c.out, c.l[c.n_layers - 1].M, c.out_stride, rows, row0);
        return;
    }
    const TChain &e = a.c[EST], &c = a.c[ACT];
    const int F = e.l[0].K, NL = e.l[e.n_layers - 1].M;
    const lds_f *p = chain_from_rows<RB>(a.ws, e, a.est_start ? b1 : b0, a.est_start ? b0 : b1, false, false, a.clip, R, rows, row0);       // ends in b1: est_start is chosen so
    const int sa = c.l[0].sa, sp = e.l[e.n_layers - 1].so;
    stage_rows(e.in, F, e.in_stride, b0, sa, R, rows, row0);                           // [features | est] in b0, at the actor's stride
    for (int i = threadIdx.x; i < R * NL; i += kThreads) {
        const int row = i / NL, col = i - row * NL;
        b0[row * sa + F + col] = row < rows ? p[row * sp + col] : 0.f;
    }
    __syncthreads();
    copy_out(b0, sa, a.ws + a.cat_off, F + NL, F + NL, rows, row0);
    const lds_f *m = chain_forward<RB>(a.ws, c, b0, b1, true, a.clip_on != 0, a.clip, R, rows, row0);
    const int sm = c.l[c.n_layers - 1].so;
    copy_out(m, sm, c.out, a.A, c.out_stride, rows, row0);
    store_sigma(m, sm, a.A, a.std, a.sigma, a.sigma_stride, rows, row0);
}

template <int RB> __global__ __launch_bounds__(256) void train_est_forward_kernel(EArgs a) {
    extern __shared__ __align__(16) float lds[];
    const TChain &c = a.c[EST];
    const int R = a.R, row0 = blockIdx.x * R;
    const int rows = min(R, a.N - row0);
    const lds_f *p = chain_from_rows<RB>(a.ws, c, (lds_f *)lds, (lds_f *)lds + a.q_off, true, false, a.clip, R, rows, row0);
    const int NL = c.l[c.n_layers - 1].M;
    mse_tile(p, c.l[c.n_layers - 1].so, NL, a.labels, a.labels_stride, a.mask, a.mask_stride, a.ws + a.gl_off, 2.0f / ((float)a.N * (float)NL),
             (volatile double *)(lds + a.red_off), (double *)(a.ws + a.part_off), rows, row0);
}

__global__ __launch_bounds__(256) void train_est_finalize_kernel(EArgs a) {
    loss_finalize((const double *)(a.ws + a.part_off), a.n_tiles, a.N, a.c[EST].l[a.c[EST].n_layers - 1].M, a.loss);
}

template <int RB> __global__ __launch_bounds__(256) void train_ee_input_grad_kernel(EArgs a) {
    extern __shared__ __align__(16) float lds[];
    const int ci = a.c0 + blockIdx.y;
    const TChain &c = a.c[ci];
    const int R = a.R, row0 = blockIdx.x * R;
    const int rows = min(R, a.N - row0);
    lds_f *b0 = (lds_f *)lds, *b1 = (lds_f *)lds + a.q_off;
    seed_last_g(a.ws, c, (c.n_layers & 1) ? b1 : b0, a.est_pass ? a.ws + a.gl_off : nullptr, a.upstream, ci == ACT && a.clip_on, a.clip, R, rows, row0);
    __syncthreads();
    chain_backward<RB>(a.ws, c, b0, b1, R, rows, row0);
}

__global__ __launch_bounds__(64) void train_ee_weight_grad_kernel(EArgs a) { wgrad_job(a, a.c, a.c0, a.c1); }

__global__ __launch_bounds__(256) void train_ee_combine_kernel(EArgs a) { combine_all(a, a.c, a.c0, a.c1); }

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static const char *kChainEE[LG_TRAIN_EE_CHAINS] = {"chain[0] (estimator)", "chain[1] (actor)", "chain[2] (critic)"};
static const char *kChainEst = "chain (estimator)";
static void (*const kForward[2])(EArgs) = {train_ee_forward_kernel<1>, train_ee_forward_kernel<2>};
static void (*const kEstForward[2])(EArgs) = {train_est_forward_kernel<1>, train_est_forward_kernel<2>};
static void (*const kInputGrad[2])(EArgs) = {train_ee_input_grad_kernel<1>, train_ee_input_grad_kernel<2>};
static bool raised_forward[2][64], raised_est_forward[2][64], raised_input_grad[2][64];

// offsets, slices and jobs of the chains [c0, c1) behind `off`, the LDS tile, and with extra_lds the estimator pass's loss regions
static int layout_ee(const std::string &f, int N, int c0, int c1, bool std_on, const int w[2], int extra_lds, long long off, LgTrainEEPlan &pl, EArgs &k) {
    PassLayout lay;
    if (plan_layout(f, k, k.c, N, c0, c1, std_on ? ACT : -1, LG_TRAIN_EE_TARGET_JOBS, w, extra_lds, false, off, lay)) return 1;
    plan_out(pl, k, k.c, lay);
    k.gl_off = pl.gl_off = lay.gl_off; k.part_off = pl.partial_off = lay.part_off;
    pl.loss_tiles = extra_lds ? k.n_tiles : 0;
    return 0;
}

static int make_plan_ee(const char *fn, const LgTrainEEArgs *p, LgTrainEEPlan &pl, EArgs &k) {
    const std::string f(fn);
    if (check_desc(f, p)) return 1;
    pl = LgTrainEEPlan{};
    k = EArgs{};
    int w[2] = {0, 0};
    const int ne = p->chain[EST].n_layers;
    k.est_start = pl.est_first_buffer = (ne & 1) ? 0 : 1;
    for (int ci = 0; ci < LG_TRAIN_EE_CHAINS; ci++)
        if (plan_chain(f + ": " + kChainEE[ci], p->chain[ci], k.c[ci], ci == EST ? k.est_start : 0, w)) return 1;
    const int F = k.c[EST].l[0].K, NL = k.c[EST].l[ne - 1].M;
    if (k.c[ACT].l[0].K != F + NL)
        return lg_fail_msg(f + ": " + kChainEE[ACT] + ".layer[0].n_in = " + std::to_string(k.c[ACT].l[0].K) + ", but [features | estimator output] has " +
                           std::to_string(F) + " + " + std::to_string(NL) + " columns");
    pl.cat_off = k.cat_off = 0;
    return layout_ee(f, p->n_rows, ACT, CRI + 1, true, w, 0, (long long)p->n_rows * (F + NL), pl, k);
}

static int make_plan_est(const char *fn, const LgTrainEstArgs *p, LgTrainEEPlan &pl, EArgs &k) {
    const std::string f(fn);
    if (check_desc(f, p)) return 1;
    pl = LgTrainEEPlan{};
    k = EArgs{};
    int w[2] = {0, 0};
    if (plan_chain(f + ": " + kChainEst, p->chain, k.c[EST], 0, w)) return 1;
    pl.cat_off = -1;
    k.est_pass = 1;
    return layout_ee(f, p->n_rows, EST, EST + 1, false, w, kRedBytes, 0, pl, k);
}

static int bind_ee(const char *fn, const LgTrainEEArgs *p, const LgTrainEEPlan &pl, EArgs &k, bool backward) {
    const std::string f(fn);
    for (int ci = 0; ci < LG_TRAIN_EE_CHAINS; ci++)      // the actor has no input of its own
        if (bind_chain(f + ": " + kChainEE[ci], p->chain[ci], k.c[ci], ci == ACT ? 0 : p->chain[ci].layer[0].n_in, backward && ci != EST)) return 1;
    if (bind_heads(f, p, k, k.c[ACT], k.c[CRI], pl.workspace_floats, backward)) return 1;
    k.c[ACT].in = p->workspace + pl.cat_off; k.c[ACT].in_stride = k.c[ACT].l[0].K;       // the stored concatenation
    return 0;
}

static int bind_est(const char *fn, const LgTrainEstArgs *p, const LgTrainEEPlan &pl, EArgs &k, bool backward) {
    const std::string f(fn);
    if (bind_chain(f + ": " + kChainEst, p->chain, k.c[EST], p->chain.layer[0].n_in, backward)) return 1;
    const int NL = k.c[EST].l[k.c[EST].n_layers - 1].M;
    if (!p->labels) return lg_fail_msg(f + ": labels is null");
    if (!p->mask) return lg_fail_msg(f + ": mask is null");
    if (p->labels_stride < NL) return lg_fail_msg(f + ": labels_stride = " + std::to_string(p->labels_stride) + " is below its width " + std::to_string(NL));
    if (p->mask_stride < 1) return lg_fail_msg(f + ": mask_stride = " + std::to_string(p->mask_stride) + " is below its width 1");
    if (!backward && !p->loss) return lg_fail_msg(f + ": loss is null");
    if (backward && !p->upstream) return lg_fail_msg(f + ": upstream is null");
    if (check_ws(f, p->workspace, p->workspace_capacity, pl.workspace_floats, true)) return 1;
    k.ws = p->workspace;
    k.labels = p->labels; k.labels_stride = p->labels_stride; k.mask = p->mask; k.mask_stride = p->mask_stride;
    k.loss = p->loss; k.upstream = p->upstream;
    return 0;
}

extern "C" int lg_train_ee_plan(const LgTrainEEArgs *args, LgTrainEEPlan *out) {
    if (!out) return lg_fail_msg("lg_train_ee_plan: null plan");
    EArgs k;
    return make_plan_ee("lg_train_ee_plan", args, *out, k);
}

extern "C" int lg_train_est_plan(const LgTrainEstArgs *args, LgTrainEEPlan *out) {
    if (!out) return lg_fail_msg("lg_train_est_plan: null plan");
    EArgs k;
    return make_plan_est("lg_train_est_plan", args, *out, k);
}

extern "C" int lg_train_ee_forward(const LgTrainEEArgs *args, void *stream) {
    static const char *fn = "lg_train_ee_forward";
    LgTrainEEPlan pl; EArgs k;
    if (make_plan_ee(fn, args, pl, k) || bind_ee(fn, args, pl, k, false)) return 1;
    return launch_tile(fn, kForward, raised_forward, 2, pl.lds_bytes, (hipStream_t)stream, k) || done(fn);
}

extern "C" int lg_train_ee_backward(const LgTrainEEArgs *args, void *stream) {
    static const char *fn = "lg_train_ee_backward";
    LgTrainEEPlan pl; EArgs k;
    if (make_plan_ee(fn, args, pl, k) || bind_ee(fn, args, pl, k, true)) return 1;
    return launch_backward(fn, kInputGrad, raised_input_grad, train_ee_weight_grad_kernel, train_ee_combine_kernel, k.c1 - k.c0, pl.lds_bytes, (hipStream_t)stream, k);
}

extern "C" int lg_train_est_forward(const LgTrainEstArgs *args, void *stream) {
    static const char *fn = "lg_train_est_forward";
    LgTrainEEPlan pl; EArgs k;
    if (make_plan_est(fn, args, pl, k) || bind_est(fn, args, pl, k, false)) return 1;
    if (launch_tile(fn, kEstForward, raised_est_forward, 1, pl.lds_bytes, (hipStream_t)stream, k)) return 1;
    hipLaunchKernelGGL(train_est_finalize_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, k);
    return done(fn);
}

extern "C" int lg_train_est_backward(const LgTrainEstArgs *args, void *stream) {
    static const char *fn = "lg_train_est_backward";
    LgTrainEEPlan pl; EArgs k;
    if (make_plan_est(fn, args, pl, k) || bind_est(fn, args, pl, k, true)) return 1;
    return launch_backward(fn, kInputGrad, raised_input_grad, train_ee_weight_grad_kernel, train_ee_combine_kernel, k.c1 - k.c0, pl.lds_bytes, (hipStream_t)stream, k);
}

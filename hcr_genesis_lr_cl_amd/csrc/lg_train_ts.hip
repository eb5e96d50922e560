// lg_train_ts.hip -- the fused learner passes of the teacher-student family behind include/lgtraints.h: the RL pass of ActorCriticTS
// (privilege encoder -> [obs | z] -> actor, and the critic) with its backward over the actor, the critic AND the privilege encoder, and the
// supervised history-encoder pass (history encoder against the privilege encoder's output as a constant target, masked mean-squared
// error, backward over the history encoder).
//
// Reference call sites replaced: rsl_rl/algorithms/ppo_ts.py:144-187 (_compute_rl_loss's network calls, _compute_encoder_loss) and the
// share of the two loss.backward() calls of PPO_TS.update() (ppo_ts.py:110-133) that runs through the four MLPs of
// rsl_rl/modules/actor_critic_ts.py:46-126,163-169.
//
// The layer routines are lg_train_tiles.h's (the MFMA layouts are described in lg_train.hip), the chain, loss, plan and launch routines
// lg_train_pass.h's.  What is this family's own:
//   RL forward        grid (row tiles, 2).  y = 0: privileged_obs -> LDS, the privilege encoder ping-pongs so that its output ends in
//                     activation 1 (its hidden activations go to the workspace: its backward needs them), the observations are staged into
//                     activation 0 at the actor's stride with the latent copied behind them, the concatenation goes to the workspace while
//                     the actor's first layer reads it.  y = 1: the critic.
//   RL input gradient y = 0 does not stop at actor layer 1: one more bwd_tile over actor layer 0 (no ELU factor: its input is no activation)
//                     leaves d loss / d [obs | z] in activation 0; its columns [O, O + Z) are G of the privilege encoder's last layer and
//                     are copied to activation 1, where that chain's parity expects them (it is where the forward left z), and to the
//                     workspace; the loop then carries on through the encoder against its stored H.
//   encoder forward   per row tile the privilege encoder (nothing stored; its rows of y go to a dense region of the workspace that this
//                     workgroup alone reads back behind a barrier), then the history encoder, d = (p - y) t, gl = 2 d t / (N Z) and the
//                     tile's float64 sum of d^2 by a fixed tree; a one-workgroup launch adds the tile partials in tile order.
//   backward          the three launches of lg_train.hip over the chains [c0, c1) of the pass: privilege encoder, actor and critic, or the
//                     history encoder alone (whose staged gl is scaled by the upstream scalar, read on the device).
// Plain stores only; two calls on the same inputs give the same bits.
#include "lg_train_pass.h"
#include "../../include/lgtraints.h"

#define PRI LG_TRAIN_TS_PRIVILEGE
#define ACT LG_TRAIN_TS_ACTOR
#define CRI LG_TRAIN_TS_CRITIC
#define HIS LG_TRAIN_TS_HISTORY
static const int kRedBytes = LG_TRAIN_TS_THREADS * (int)sizeof(double);
static_assert(LG_TRAIN_TS_THREADS == kThreads, "the loss tree has one leaf per thread of the row-tile workgroup");

struct SArgs : PArgs {
    TChain c[LG_TRAIN_TS_CHAINS];
    const float *obs;           // (N, O): the first columns of the actor's input
    const float *mask, *upstream;
    float *loss;
    int obs_stride, mask_stride;
    int enc_start, enc_pass;
    long long cat_off, gl_off, y_off, part_off;
};
static_assert(sizeof(SArgs) <= 4096, "SArgs is passed by value: the kernel-argument segment is 4 KB");

template <int RB> __global__ __launch_bounds__(256) void train_ts_forward_kernel(SArgs a) {
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
    const TChain &e = a.c[PRI], &c = a.c[ACT];
    const int Z = e.l[e.n_layers - 1].M, O = c.l[0].K - Z;
    const lds_f *z = chain_from_rows<RB>(a.ws, e, a.enc_start ? b1 : b0, a.enc_start ? b0 : b1, true, false, a.clip, R, rows, row0);        // ends in b1: enc_start is chosen so
    const int sa = c.l[0].sa, sz = e.l[e.n_layers - 1].so;
    stage_rows(a.obs, O, a.obs_stride, b0, sa, R, rows, row0);                         // [obs | z] in b0, at the actor's stride
    for (int i = threadIdx.x; i < R * Z; i += kThreads) {
        const int row = i / Z, col = i - row * Z;
        b0[row * sa + O + col] = row < rows ? z[row * sz + col] : 0.f;
    }
    __syncthreads();
    copy_out(b0, sa, a.ws + a.cat_off, O + Z, O + Z, rows, row0);
    const lds_f *m = chain_forward<RB>(a.ws, c, b0, b1, true, a.clip_on != 0, a.clip, R, rows, row0);
    const int sm = c.l[c.n_layers - 1].so;
    copy_out(m, sm, c.out, a.A, c.out_stride, rows, row0);
    store_sigma(m, sm, a.A, a.std, a.sigma, a.sigma_stride, rows, row0);
}

template <int RB> __global__ __launch_bounds__(256) void train_enc_forward_kernel(SArgs a) {
    extern __shared__ __align__(16) float lds[];
    const TChain &e = a.c[PRI], &c = a.c[HIS];
    const int R = a.R, row0 = blockIdx.x * R;
    const int rows = min(R, a.N - row0);
    lds_f *b0 = (lds_f *)lds, *b1 = (lds_f *)lds + a.q_off;
    const int Z = c.l[c.n_layers - 1].M;
    float *yw = a.ws + a.y_off;
    const lds_f *y = chain_from_rows<RB>(a.ws, e, b0, b1, false, false, a.clip, R, rows, row0);       // the target: nothing stored, no gradient
    copy_out(y, e.l[e.n_layers - 1].so, yw, Z, Z, rows, row0);                         // this tile's rows; read back below by this workgroup only
    __syncthreads();                                                                   // y has left the LDS before the history is staged over it
    const lds_f *p = chain_from_rows<RB>(a.ws, c, b0, b1, true, false, a.clip, R, rows, row0);
    mse_tile(p, c.l[c.n_layers - 1].so, Z, yw, Z, a.mask, a.mask_stride, a.ws + a.gl_off, 2.0f / ((float)a.N * (float)Z), (volatile double *)(lds + a.red_off),
             (double *)(a.ws + a.part_off), rows, row0);
}

__global__ __launch_bounds__(256) void train_enc_finalize_kernel(SArgs a) {
    loss_finalize((const double *)(a.ws + a.part_off), a.n_tiles, a.N, a.c[HIS].l[a.c[HIS].n_layers - 1].M, a.loss);
}

// grid (row tiles, 2) in the RL pass: y = 0 the actor and, through the latent, the privilege encoder; y = 1 the critic.  Grid (row tiles,
// 1) in the encoder pass: the history encoder.
template <int RB> __global__ __launch_bounds__(256) void train_ts_input_grad_kernel(SArgs a) {
    extern __shared__ __align__(16) float lds[];
    const int ci = a.enc_pass ? HIS : (blockIdx.y ? CRI : ACT);
    const TChain &c = a.c[ci];
    const int R = a.R, row0 = blockIdx.x * R;
    const int rows = min(R, a.N - row0);
    lds_f *b0 = (lds_f *)lds, *b1 = (lds_f *)lds + a.q_off;
    seed_last_g(a.ws, c, (c.n_layers & 1) ? b1 : b0, a.enc_pass ? a.ws + a.gl_off : nullptr, a.upstream, ci == ACT && a.clip_on, a.clip, R, rows, row0);
    __syncthreads();
    chain_backward<RB>(a.ws, c, b0, b1, R, rows, row0);
    if (ci != ACT) return;
    // G_0 of the actor sits in b1.  Through actor layer 0: d loss / d [obs | z] into b0 at the stride the concatenation had there.  No
    // ELU factor: the concatenation is no activation.
    const TLayer &L0 = c.l[0];
    bwd_layer<RB>(L0, b1, b0, false, R);
    __syncthreads();                                                   // b0 is complete; b1 (G_0 and its copy to the workspace) has been read
    const TChain &e = a.c[PRI];
    const int ne = e.n_layers;
    const TLayer &EL = e.l[ne - 1];
    const int Z = EL.M, O = L0.K - Z;
    lds_f *s0 = a.enc_start ? b1 : b0, *s1 = a.enc_start ? b0 : b1;    // the encoder's forward pair: its last output, hence its G_L, is in b1
    {
        lds_f *g = (ne & 1) ? s1 : s0;
        float *gws = a.ws + EL.g_off;
        for (int i = threadIdx.x; i < R * Z; i += kThreads) {
            const int row = i / Z, col = i - row * Z;
            const float v = b0[row * L0.sa + O + col];                 // rows behind `rows` carry zeros: their G_L was zero
            if (row < rows) gws[(size_t)(row0 + row) * Z + col] = v;
            g[row * EL.so + col] = v;
        }
    }
    __syncthreads();
    chain_backward<RB>(a.ws, e, s0, s1, R, rows, row0);
}

__global__ __launch_bounds__(64) void train_ts_weight_grad_kernel(SArgs a) { wgrad_job(a, a.c, a.c0, a.c1); }

__global__ __launch_bounds__(256) void train_ts_combine_kernel(SArgs a) { combine_all(a, a.c, a.c0, a.c1); }

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static const char *kChainTS[LG_TRAIN_TS_CHAINS] = {"chain[0] (privilege encoder)", "chain[1] (actor)", "chain[2] (critic)", ""};
static const char *kChainEnc[LG_TRAIN_ENC_CHAINS] = {"chain[0] (history encoder)", "chain[1] (privilege encoder)"};
static const int kEncChain[LG_TRAIN_ENC_CHAINS] = {HIS, PRI};          // LgTrainEncArgs::chain[i] is chain kEncChain[i] of the kernels
static void (*const kForward[2])(SArgs) = {train_ts_forward_kernel<1>, train_ts_forward_kernel<2>};
static void (*const kEncForward[2])(SArgs) = {train_enc_forward_kernel<1>, train_enc_forward_kernel<2>};
static void (*const kInputGrad[2])(SArgs) = {train_ts_input_grad_kernel<1>, train_ts_input_grad_kernel<2>};
static bool raised_forward[2][64], raised_enc_forward[2][64], raised_input_grad[2][64];

// offsets, slices and jobs of the chains [c0, c1) behind `off`, the LDS tile, and with extra_lds the encoder pass's loss regions
static int layout_ts(const std::string &f, int N, int c0, int c1, bool std_on, const int w[2], int extra_lds, long long off, LgTrainTSPlan &pl, SArgs &k) {
    PassLayout lay;
    if (plan_layout(f, k, k.c, N, c0, c1, std_on ? ACT : -1, LG_TRAIN_TS_TARGET_JOBS, w, extra_lds, true, off, lay)) return 1;
    plan_out(pl, k, k.c, lay);
    k.gl_off = pl.gl_off = lay.gl_off; k.y_off = pl.y_off = lay.y_off; k.part_off = pl.partial_off = lay.part_off;
    pl.loss_tiles = extra_lds ? k.n_tiles : 0;
    return 0;
}

static int make_plan_ts(const char *fn, const LgTrainTSArgs *p, LgTrainTSPlan &pl, SArgs &k) {
    const std::string f(fn);
    if (check_desc(f, p)) return 1;
    if (p->n_obs < 1) return lg_fail_msg(f + ": n_obs = " + std::to_string(p->n_obs) + " < 1");
    pl = LgTrainTSPlan{};
    k = SArgs{};
    int w[2] = {0, 0};
    const int ne = p->chain[PRI].n_layers;
    k.enc_start = pl.enc_first_buffer = (ne & 1) ? 0 : 1;
    for (int ci = 0; ci < LG_TRAIN_TS_RL_CHAINS; ci++)
        if (plan_chain(f + ": " + kChainTS[ci], p->chain[ci], k.c[ci], ci == PRI ? k.enc_start : 0, w)) return 1;
    const int O = p->n_obs, Z = k.c[PRI].l[ne - 1].M;
    if (k.c[ACT].l[0].K != O + Z)
        return lg_fail_msg(f + ": " + kChainTS[ACT] + ".layer[0].n_in = " + std::to_string(k.c[ACT].l[0].K) + ", but [obs | privilege encoder output] has " +
                           std::to_string(O) + " + " + std::to_string(Z) + " columns (n_obs + the privilege encoder's last n_out)");
    pl.cat_off = k.cat_off = 0;
    return layout_ts(f, p->n_rows, PRI, CRI + 1, true, w, 0, (long long)p->n_rows * (O + Z), pl, k);
}

static int make_plan_enc(const char *fn, const LgTrainEncArgs *p, LgTrainTSPlan &pl, SArgs &k) {
    const std::string f(fn);
    if (check_desc(f, p)) return 1;
    pl = LgTrainTSPlan{};
    k = SArgs{};
    int w[2] = {0, 0};
    for (int i = 0; i < LG_TRAIN_ENC_CHAINS; i++)
        if (plan_chain(f + ": " + kChainEnc[i], p->chain[i], k.c[kEncChain[i]], 0, w)) return 1;
    const int Zh = k.c[HIS].l[k.c[HIS].n_layers - 1].M, Zp = k.c[PRI].l[k.c[PRI].n_layers - 1].M;
    if (Zh != Zp)
        return lg_fail_msg(f + ": " + kChainEnc[LG_TRAIN_ENC_PRIVILEGE] + ".layer[" + std::to_string(k.c[PRI].n_layers - 1) + "].n_out = " + std::to_string(Zp) +
                           ", but the history encoder ends at " + std::to_string(Zh) + " columns: the two encoders' output widths differ");
    pl.cat_off = -1;
    k.enc_pass = 1;
    return layout_ts(f, p->n_rows, HIS, HIS + 1, false, w, kRedBytes, 0, pl, k);
}

static int bind_ts(const char *fn, const LgTrainTSArgs *p, const LgTrainTSPlan &pl, SArgs &k, bool backward) {
    const std::string f(fn);
    for (int ci = 0; ci < LG_TRAIN_TS_RL_CHAINS; ci++)
        if (bind_chain(f + ": " + kChainTS[ci], p->chain[ci], k.c[ci], ci == ACT ? p->n_obs : p->chain[ci].layer[0].n_in, backward)) return 1;
    if (bind_heads(f, p, k, k.c[ACT], k.c[CRI], pl.workspace_floats, backward)) return 1;
    k.obs = p->chain[ACT].input; k.obs_stride = p->chain[ACT].in_stride;
    k.c[ACT].in = p->workspace + pl.cat_off; k.c[ACT].in_stride = k.c[ACT].l[0].K;       // the stored concatenation
    return 0;
}

static int bind_enc(const char *fn, const LgTrainEncArgs *p, const LgTrainTSPlan &pl, SArgs &k, bool backward) {
    const std::string f(fn);
    for (int i = 0; i < LG_TRAIN_ENC_CHAINS; i++)
        if (bind_chain(f + ": " + kChainEnc[i], p->chain[i], k.c[kEncChain[i]], p->chain[i].layer[0].n_in, backward && i == LG_TRAIN_ENC_HISTORY)) return 1;
    if (!p->mask) return lg_fail_msg(f + ": mask is null");
    if (p->mask_stride < 1) return lg_fail_msg(f + ": mask_stride = " + std::to_string(p->mask_stride) + " is below its width 1");
    if (!backward && !p->loss) return lg_fail_msg(f + ": loss is null");
    if (backward && !p->upstream) return lg_fail_msg(f + ": upstream is null");
    if (check_ws(f, p->workspace, p->workspace_capacity, pl.workspace_floats, true)) return 1;
    k.ws = p->workspace;
    k.mask = p->mask; k.mask_stride = p->mask_stride;
    k.loss = p->loss; k.upstream = p->upstream;
    return 0;
}

extern "C" int lg_train_ts_plan(const LgTrainTSArgs *args, LgTrainTSPlan *out) {
    if (!out) return lg_fail_msg("lg_train_ts_plan: null plan");
    SArgs k;
    return make_plan_ts("lg_train_ts_plan", args, *out, k);
}

extern "C" int lg_train_enc_plan(const LgTrainEncArgs *args, LgTrainTSPlan *out) {
    if (!out) return lg_fail_msg("lg_train_enc_plan: null plan");
    SArgs k;
    return make_plan_enc("lg_train_enc_plan", args, *out, k);
}

extern "C" int lg_train_ts_forward(const LgTrainTSArgs *args, void *stream) {
    static const char *fn = "lg_train_ts_forward";
    LgTrainTSPlan pl; SArgs k;
    if (make_plan_ts(fn, args, pl, k) || bind_ts(fn, args, pl, k, false)) return 1;
    return launch_tile(fn, kForward, raised_forward, 2, pl.lds_bytes, (hipStream_t)stream, k) || done(fn);
}

extern "C" int lg_train_ts_backward(const LgTrainTSArgs *args, void *stream) {
    static const char *fn = "lg_train_ts_backward";
    LgTrainTSPlan pl; SArgs k;
    if (make_plan_ts(fn, args, pl, k) || bind_ts(fn, args, pl, k, true)) return 1;
    return launch_backward(fn, kInputGrad, raised_input_grad, train_ts_weight_grad_kernel, train_ts_combine_kernel, 2, pl.lds_bytes, (hipStream_t)stream, k);
}

extern "C" int lg_train_enc_forward(const LgTrainEncArgs *args, void *stream) {
    static const char *fn = "lg_train_enc_forward";
    LgTrainTSPlan pl; SArgs k;
    if (make_plan_enc(fn, args, pl, k) || bind_enc(fn, args, pl, k, false)) return 1;
    if (launch_tile(fn, kEncForward, raised_enc_forward, 1, pl.lds_bytes, (hipStream_t)stream, k)) return 1;
    hipLaunchKernelGGL(train_enc_finalize_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, k);
    return done(fn);
}

extern "C" int lg_train_enc_backward(const LgTrainEncArgs *args, void *stream) {
    static const char *fn = "lg_train_enc_backward";
    LgTrainTSPlan pl; SArgs k;
    if (make_plan_enc(fn, args, pl, k) || bind_enc(fn, args, pl, k, true)) return 1;
    return launch_backward(fn, kInputGrad, raised_input_grad, train_ts_weight_grad_kernel, train_ts_combine_kernel, 1, pl.lds_bytes, (hipStream_t)stream, k);
}

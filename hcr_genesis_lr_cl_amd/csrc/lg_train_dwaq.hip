// lg_train_dwaq.hip -- the fused learner passes of the DreamWaQ family behind include/lgtraindwaq.h: the RL pass of ActorCriticDreamWaQ
// (VAE encoder -> four heads -> reparameterised draw -> [obs | z | v] -> actor, and the critic) with its backward over the actor and the
// critic, and the VAE pass (encoder, heads, draw, decoder; estimation, reconstruction and KL losses; backward over all six chains).
//
// Reference call sites replaced: rsl_rl/algorithms/ppo_dreamwaq.py:193-236 (_compute_rl_loss's network calls, _compute_vae_loss) and the
// share of the two loss.backward() calls of PPO_DreamWaQ.update() (ppo_dreamwaq.py:151-173) that runs through rsl_rl/modules/vae.py and the
// two MLPs of rsl_rl/modules/actor_critic_dreamwaq.py:83-108,145-175.
//
// The layer routines are lg_train_tiles.h's (the MFMA layouts are described in lg_train.hip), the chain, loss, plan and launch routines
// lg_train_pass.h's.  What is this family's own:
//   LDS               the encoder starts in activation 0 and ends in X (activation n_layers & 1); Y is the other one.  The four heads read
//                     X and write four disjoint regions of Y, region h at R * (the output strides of the heads before it) floats.
//   RL forward        grid (row tiles, 2).  y = 0: encoder and heads with nothing stored, the log-variances clipped by the layer routine,
//                     the observations staged into X at the actor's stride with z and v drawn behind them, the concatenation to the
//                     workspace, the actor over the pair (X, Y).  y = 1: the critic.
//   VAE forward       per row tile the encoder (hidden activations and its last output stored), the heads (stored), the tile's float64 sums
//                     of s and t, the draw [z | v] into X (stored), gl_est and the sum of d_est^2, the decoder over (X, Y), gl_rec and the
//                     sum of d_rec^2; a one-workgroup launch adds the four partial streams in tile order and leaves T / B^2.
//   VAE input gradient  the decoder down to layer 1, one more layer over decoder layer 0 (no ELU factor) for d loss / d [z | v] in X, the
//                     four head gradients into the regions of Y (and the workspace), the four head products through a second region of X
//                     added in head order, times elu' of the stored encoder output: G of the encoder's last layer; the encoder's loop.
//   backward          the three launches of lg_train.hip over the chains [c0, c1) of the pass.
// Plain stores only; two calls on the same inputs give the same bits.
#include "lg_train_pass.h"
#include "../../include/lgtraindwaq.h"

#define ENC LG_TRAIN_DWAQ_ENCODER
#define LMU LG_TRAIN_DWAQ_LATENT_MU
#define LVAR LG_TRAIN_DWAQ_LATENT_VAR
#define VMU LG_TRAIN_DWAQ_VEL_MU
#define VVAR LG_TRAIN_DWAQ_VEL_VAR
#define ACT LG_TRAIN_DWAQ_ACTOR
#define CRI LG_TRAIN_DWAQ_CRITIC
#define DEC LG_TRAIN_VAE_DECODER
#define NH LG_TRAIN_DWAQ_HEADS
#define NQ LG_TRAIN_VAE_LOSSES
static const int kRedBytes = LG_TRAIN_DWAQ_THREADS * (int)sizeof(double);
static_assert(LG_TRAIN_DWAQ_THREADS == kThreads, "the loss trees have one leaf per thread of the row-tile workgroup");
static_assert(DEC == ACT && LVAR == LMU + 1 && VMU == LMU + 2 && VVAR == LMU + 3, "the heads are chains LMU + h; the decoder takes the actor's slot");

struct DArgs : PArgs {
    TChain c[LG_TRAIN_DWAQ_CHAINS];
    const float *obs;           // (N, O): the first columns of the actor's input
    const float *noise, *labels, *next, *mask, *upstream;
    float *loss;
    int obs_stride, noise_stride, labels_stride, next_stride, mask_stride;
    int x_off, y_off;           // LDS: the activation the encoder ends in, and the other one
    int hreg[NH], preg;         // LDS: head h's region of Y; the second region of X, where a head product waits to be added
    float var_clip, kld_weight;
    long long cat_off, enc_off, head_off[NH], gl_rec_off, gl_est_off, part_off, scale_off;
};
static_assert(sizeof(DArgs) <= 4096, "DArgs is passed by value: the kernel-argument segment is 4 KB");

// the four heads over the encoder's output in x, into their regions of y; a barrier has passed behind the last
template <int RB>
__device__ __forceinline__ void heads_forward(const DArgs &a, lds_f *x, lds_f *y, int R, int rows, int row0) {
    for (int h = 0; h < NH; h++) chain_forward<RB>(a.ws, a.c[LMU + h], x, y + a.hreg[h], false, (h & 1) != 0, a.var_clip, R, rows, row0);
}

// [z | v] = eps * exp(0.5 * log-variance) + mean from the heads' regions of y into dst (sd floats between rows); rows behind `rows` are zero
__device__ __forceinline__ void draw(const DArgs &a, const lds_f *y, lds_f *dst, int sd, int R, int rows, int row0) {
    const int L = a.c[LMU].l[0].M, W = L + a.c[VMU].l[0].M;
    for (int i = threadIdx.x; i < R * W; i += kThreads) {
        const int row = i / W, col = i - row * W;
        float v = 0.f;
        if (row < rows) {
            const int hm = col < L ? 0 : 2, cc = col < L ? col : col - L, so = a.c[LMU + hm].l[0].so;
            const float eps = a.noise[(size_t)(row0 + row) * a.noise_stride + col];
            v = eps * expf(0.5f * y[a.hreg[hm + 1] + row * so + cc]) + y[a.hreg[hm] + row * so + cc];
        }
        dst[row * sd + col] = v;
    }
}

// the workgroup's float64 sum of `acc` by the fixed tree of mse_tile, into part[this tile]
__device__ __forceinline__ void tile_sum(double acc, volatile double *red, double *part) {
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

template <int RB> __global__ __launch_bounds__(256) void train_dwaq_forward_kernel(DArgs a) {
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
    const TChain &c = a.c[ACT];
    lds_f *X = (lds_f *)lds + a.x_off, *Y = (lds_f *)lds + a.y_off;
    chain_from_rows<RB>(a.ws, a.c[ENC], b0, b1, false, false, a.clip, R, rows, row0);             // ends in X
    heads_forward<RB>(a, X, Y, R, rows, row0);
    const int LE = a.c[LMU].l[0].M + a.c[VMU].l[0].M, O = c.l[0].K - LE, sa = c.l[0].sa;
    stage_rows(a.obs, O, a.obs_stride, X, sa, R, rows, row0);                                    // [obs | z | v] in X, at the actor's stride
    draw(a, Y, X + O, sa, R, rows, row0);
    __syncthreads();
    copy_out(X, sa, a.ws + a.cat_off, O + LE, O + LE, rows, row0);
    const lds_f *m = chain_forward<RB>(a.ws, c, X, Y, true, a.clip_on != 0, a.clip, R, rows, row0);
    const int sm = c.l[c.n_layers - 1].so;
    copy_out(m, sm, c.out, a.A, c.out_stride, rows, row0);
    store_sigma(m, sm, a.A, a.std, a.sigma, a.sigma_stride, rows, row0);
}

// grid (row tiles, 2): y = 0 the actor over the pair its forward ran in, y = 1 the critic
template <int RB> __global__ __launch_bounds__(256) void train_dwaq_input_grad_kernel(DArgs a) {
    extern __shared__ __align__(16) float lds[];
    const int ci = ACT + blockIdx.y;
    const TChain &c = a.c[ci];
    const int R = a.R, row0 = blockIdx.x * R;
    const int rows = min(R, a.N - row0);
    lds_f *p0 = (lds_f *)lds + (ci == ACT ? a.x_off : 0), *p1 = (lds_f *)lds + (ci == ACT ? a.y_off : a.q_off);
    seed_last_g(a.ws, c, (c.n_layers & 1) ? p1 : p0, nullptr, nullptr, ci == ACT && a.clip_on, a.clip, R, rows, row0);
    __syncthreads();
    chain_backward<RB>(a.ws, c, p0, p1, R, rows, row0);
}

template <int RB> __global__ __launch_bounds__(256) void train_vae_forward_kernel(DArgs a) {
    extern __shared__ __align__(16) float lds[];
    const TChain &e = a.c[ENC], &d = a.c[DEC];
    const int R = a.R, row0 = blockIdx.x * R;
    const int rows = min(R, a.N - row0);
    lds_f *X = (lds_f *)lds + a.x_off, *Y = (lds_f *)lds + a.y_off;
    volatile double *red = (volatile double *)(lds + a.red_off);
    double *part = (double *)(a.ws + a.part_off);
    const TLayer &EL = e.l[e.n_layers - 1];
    chain_from_rows<RB>(a.ws, e, (lds_f *)lds, (lds_f *)lds + a.q_off, true, false, a.clip, R, rows, row0);      // ends in X
    copy_out(X, EL.so, a.ws + a.enc_off, EL.M, EL.M, rows, row0);                                // it carries an ELU and has four readers
    heads_forward<RB>(a, X, Y, R, rows, row0);
    const int L = a.c[LMU].l[0].M, E = a.c[VMU].l[0].M, so = a.c[LMU].l[0].so, sa = d.l[0].sa;
    for (int h = 0; h < NH; h++) copy_out(Y + a.hreg[h], a.c[LMU + h].l[0].so, a.ws + a.head_off[h], a.c[LMU + h].l[0].M, a.c[LMU + h].l[0].M, rows, row0);
    double acc_s = 0.0, acc_t = 0.0;
    for (int i = threadIdx.x; i < rows * L; i += kThreads) {
        const int row = i / L, col = i - row * L;
        const float mu = Y[a.hreg[0] + row * so + col], lv = Y[a.hreg[1] + row * so + col];
        acc_s += (double)(((1.0f + lv) - mu * mu) - expf(lv));
    }
    for (int i = threadIdx.x; i < rows; i += kThreads) acc_t += (double)a.mask[(size_t)(row0 + i) * a.mask_stride];
    draw(a, Y, X, sa, R, rows, row0);                                                            // the encoder's output has left X
    __syncthreads();
    copy_out(X, sa, a.ws + a.cat_off, L + E, L + E, rows, row0);
    tile_sum(acc_s, red, part + 2 * (size_t)a.n_tiles);
    tile_sum(acc_t, red, part + 3 * (size_t)a.n_tiles);
    mse_tile(X + L, sa, E, a.labels, a.labels_stride, a.mask, a.mask_stride, a.ws + a.gl_est_off, 2.0f / ((float)a.N * (float)E), red, part, rows, row0);
    const lds_f *rec = chain_forward<RB>(a.ws, d, X, Y, true, false, a.clip, R, rows, row0);
    const TLayer &DL = d.l[d.n_layers - 1];
    mse_tile(rec, DL.so, DL.M, a.next, a.next_stride, a.mask, a.mask_stride, a.ws + a.gl_rec_off, 2.0f / ((float)a.N * (float)DL.M), red, part + a.n_tiles, rows, row0);
}

// one workgroup: the four partial streams in tile order, the four losses, and T / B^2 for the backward
__global__ __launch_bounds__(256) void train_vae_finalize_kernel(DArgs a) {
    __shared__ double part[NQ][kThreads];
    const double *P = (const double *)(a.ws + a.part_off);
    double sum[NQ] = {0.0, 0.0, 0.0, 0.0};
    for (int t0 = 0; t0 < a.n_tiles; t0 += kThreads) {
        const int n = min(kThreads, a.n_tiles - t0);
        if ((int)threadIdx.x < n)
            for (int q = 0; q < NQ; q++) part[q][threadIdx.x] = P[(size_t)q * a.n_tiles + t0 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < n; i++)
                for (int q = 0; q < NQ; q++) sum[q] += part[q][i];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double B = (double)a.N, E = (double)a.c[VMU].l[0].M, D = (double)a.c[DEC].l[a.c[DEC].n_layers - 1].M;
        const double est = sum[0] / (B * E), rec = sum[1] / (B * D), f = sum[3] / (B * B), kld = -0.5 * sum[2] * f;
        a.loss[0] = (float)(est + rec + (double)a.kld_weight * kld);
        a.loss[1] = (float)est; a.loss[2] = (float)rec; a.loss[3] = (float)kld;
        a.ws[a.scale_off] = (float)f;
    }
}

template <int RB> __global__ __launch_bounds__(256) void train_vae_input_grad_kernel(DArgs a) {
    extern __shared__ __align__(16) float lds[];
    const TChain &e = a.c[ENC], &d = a.c[DEC];
    const int R = a.R, row0 = blockIdx.x * R;
    const int rows = min(R, a.N - row0);
    lds_f *X = (lds_f *)lds + a.x_off, *Y = (lds_f *)lds + a.y_off;
    seed_last_g(a.ws, d, (d.n_layers & 1) ? Y : X, a.ws + a.gl_rec_off, a.upstream, false, a.clip, R, rows, row0);
    __syncthreads();
    chain_backward<RB>(a.ws, d, X, Y, R, rows, row0);                  // G_0 of the decoder sits in Y
    const TLayer &D0 = d.l[0];
    bwd_layer<RB>(D0, Y, X, false, R);                                 // d loss / d [z | v] into X; no ELU factor: the draw is no activation
    __syncthreads();                                                   // X is complete; Y (G_0 and its copy to the workspace) has been read
    const int L = a.c[LMU].l[0].M, E = a.c[VMU].l[0].M, W = L + E;
    const float up = a.upstream[0], kf = a.kld_weight * a.ws[a.scale_off] * up, clip = a.var_clip;
    for (int i = threadIdx.x; i < R * W; i += kThreads) {
        const int row = i / W, col = i - row * W;
        const bool lat = col < L;
        const int hm = lat ? 0 : 2, cc = lat ? col : col - L, w = lat ? L : E;
        float gmu = 0.f, glv = 0.f;
        if (row < rows) {
            const size_t gr = (size_t)(row0 + row), at = gr * w + cc;
            const float lv = a.ws[a.head_off[hm + 1] + at], eps = a.noise[gr * a.noise_stride + col];
            float g = X[row * D0.sa + col];
            if (!lat) g += a.ws[a.gl_est_off + at] * up;
            gmu = g;
            glv = g * eps * (0.5f * expf(0.5f * lv));
            if (lat) {
                gmu += a.ws[a.head_off[0] + at] * kf;
                glv += -0.5f * (1.0f - expf(lv)) * kf;
            }
            if (lv >= clip || lv <= -clip) glv = 0.f;                  // hardtanh_backward from the stored output: a NaN passes the gradient on
            a.ws[a.c[LMU + hm].l[0].g_off + at] = gmu;
            a.ws[a.c[LMU + hm + 1].l[0].g_off + at] = glv;
        }
        const int so = a.c[LMU + hm].l[0].so;
        Y[a.hreg[hm] + row * so + cc] = gmu;
        Y[a.hreg[hm + 1] + row * so + cc] = glv;
    }
    __syncthreads();
    // the four head products in head order: the first into X, each further one into the region behind it and added; the last addition
    // carries the encoder's last elu' from its stored output and leaves G of that layer in X and in the workspace
    const TLayer &EL = e.l[e.n_layers - 1];
    const int H = EL.M, sx = EL.so;
    bwd_layer<RB>(a.c[LMU].l[0], Y + a.hreg[0], X, false, R);
    for (int h = 1; h < NH; h++) {
        bwd_layer<RB>(a.c[LMU + h].l[0], Y + a.hreg[h], X + a.preg, false, R);
        __syncthreads();
        for (int i = threadIdx.x; i < R * H; i += kThreads) {
            const int row = i / H, k = i - row * H;
            float v = X[row * sx + k] + X[a.preg + row * sx + k];
            if (h == NH - 1 && row < rows) {
                const size_t at = (size_t)(row0 + row) * H + k;
                if (EL.elu) {
                    const float hv = a.ws[a.enc_off + at];
                    v = v * (hv > 0.f ? 1.0f : hv + 1.0f);
                }
                a.ws[EL.g_off + at] = v;
            }
            X[row * sx + k] = v;
        }
        __syncthreads();
    }
    chain_backward<RB>(a.ws, e, (lds_f *)lds, (lds_f *)lds + a.q_off, R, rows, row0);
}

__global__ __launch_bounds__(64) void train_dwaq_weight_grad_kernel(DArgs a) { wgrad_job(a, a.c, a.c0, a.c1); }

__global__ __launch_bounds__(256) void train_dwaq_combine_kernel(DArgs a) { combine_all(a, a.c, a.c0, a.c1); }

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static const char *kChainRL[LG_TRAIN_DWAQ_CHAINS] = {"chain[0] (encoder)", "chain[1] (latent_mu)", "chain[2] (latent_var)", "chain[3] (vel_mu)", "chain[4] (vel_var)",
                                                     "chain[5] (actor)", "chain[6] (critic)"};
static const char *kChainVae[LG_TRAIN_VAE_CHAINS] = {"chain[0] (encoder)", "chain[1] (latent_mu)", "chain[2] (latent_var)", "chain[3] (vel_mu)", "chain[4] (vel_var)",
                                                     "chain[5] (decoder)"};
static void (*const kForward[2])(DArgs) = {train_dwaq_forward_kernel<1>, train_dwaq_forward_kernel<2>};
static void (*const kInputGrad[2])(DArgs) = {train_dwaq_input_grad_kernel<1>, train_dwaq_input_grad_kernel<2>};
static void (*const kVaeForward[2])(DArgs) = {train_vae_forward_kernel<1>, train_vae_forward_kernel<2>};
static void (*const kVaeInputGrad[2])(DArgs) = {train_vae_input_grad_kernel<1>, train_vae_input_grad_kernel<2>};
static bool raised_forward[2][64], raised_input_grad[2][64], raised_vae_forward[2][64], raised_vae_input_grad[2][64];

// the encoder and the four heads of either descriptor into k.c[ENC .. VVAR] and the LDS widths; `products`: the backward's head
// products need two regions of X
static int plan_front(const std::string &f, const char *const *names, const LgTrainChain *chain, DArgs &k, LgTrainDwaqPlan &pl, int w[2], bool products) {
    if (plan_chain(f + ": " + names[ENC], chain[ENC], k.c[ENC], 0, w)) return 1;
    const int ne = k.c[ENC].n_layers, xi = ne & 1, H = k.c[ENC].l[ne - 1].M;
    pl.lds_x = xi; pl.lds_y = xi ^ 1;
    int sum = 0;
    for (int h = 0; h < NH; h++) {
        const std::string cn = f + ": " + names[LMU + h];
        if (chain[LMU + h].n_layers != 1) return lg_fail_msg(cn + ".n_layers = " + std::to_string(chain[LMU + h].n_layers) + ", a head is one Linear");
        if (plan_chain(cn, chain[LMU + h], k.c[LMU + h], xi, w)) return 1;
        const TLayer &T = k.c[LMU + h].l[0];
        if (T.K != H) return lg_fail_msg(cn + ".layer[0].n_in = " + std::to_string(T.K) + ", but the encoder ends at " + std::to_string(H) + " columns");
        if ((h & 1) && T.M != k.c[LMU + h - 1].l[0].M)
            return lg_fail_msg(cn + ".layer[0].n_out = " + std::to_string(T.M) + ", but its mean's head has " + std::to_string(k.c[LMU + h - 1].l[0].M) + " columns");
        sum += T.so;
    }
    if (sum > w[xi ^ 1]) w[xi ^ 1] = sum;                                 // the four heads' disjoint outputs
    if (products && 2 * k.c[LMU].l[0].sa > w[xi]) w[xi] = 2 * k.c[LMU].l[0].sa;
    return 0;
}

// what follows the row tile: the LDS offsets of X, Y, the heads' regions and the products' regions
static void place_regions(DArgs &k) {
    const int xi = k.c[ENC].n_layers & 1;
    k.x_off = xi ? k.q_off : 0; k.y_off = xi ? 0 : k.q_off;
    int at = 0;
    for (int h = 0; h < NH; h++) { k.hreg[h] = k.R * at; at += k.c[LMU + h].l[0].so; }
    k.preg = k.R * k.c[LMU].l[0].sa;
}

static void plan_blank(LgTrainDwaqPlan &pl) {
    pl.cat_off = pl.enc_out_off = pl.gl_rec_off = pl.gl_est_off = pl.partial_off = pl.scale_off = -1;
    for (int h = 0; h < NH; h++) pl.head_off[h] = -1;
}

static int make_plan_rl(const char *fn, const LgTrainDwaqArgs *p, LgTrainDwaqPlan &pl, DArgs &k) {
    const std::string f(fn);
    if (check_desc(f, p)) return 1;
    if (p->n_obs < 1) return lg_fail_msg(f + ": n_obs = " + std::to_string(p->n_obs) + " < 1");
    pl = LgTrainDwaqPlan{};
    k = DArgs{};
    int w[2] = {0, 0};
    if (plan_front(f, kChainRL, p->chain, k, pl, w, false)) return 1;
    if (plan_chain(f + ": " + kChainRL[ACT], p->chain[ACT], k.c[ACT], pl.lds_x, w) || plan_chain(f + ": " + kChainRL[CRI], p->chain[CRI], k.c[CRI], 0, w)) return 1;
    const int O = p->n_obs, L = k.c[LMU].l[0].M, E = k.c[VMU].l[0].M;
    if (k.c[ACT].l[0].K != O + L + E)
        return lg_fail_msg(f + ": " + kChainRL[ACT] + ".layer[0].n_in = " + std::to_string(k.c[ACT].l[0].K) + ", but [obs | z | v] has " + std::to_string(O) + " + " +
                           std::to_string(L) + " + " + std::to_string(E) + " columns (n_obs + the widths of latent_mu and vel_mu)");
    PassLayout lay;
    if (plan_layout(f, k, k.c, p->n_rows, ACT, CRI + 1, ACT, LG_TRAIN_DWAQ_TARGET_JOBS, w, 0, false, (long long)p->n_rows * (O + L + E), lay)) return 1;
    plan_out(pl, k, k.c, lay);
    plan_blank(pl);
    pl.cat_off = k.cat_off = 0;
    place_regions(k);
    return 0;
}

static int make_plan_vae(const char *fn, const LgTrainVaeArgs *p, LgTrainDwaqPlan &pl, DArgs &k) {
    const std::string f(fn);
    if (check_desc(f, p)) return 1;
    pl = LgTrainDwaqPlan{};
    k = DArgs{};
    int w[2] = {0, 0};
    if (plan_front(f, kChainVae, p->chain, k, pl, w, true)) return 1;
    if (plan_chain(f + ": " + kChainVae[DEC], p->chain[DEC], k.c[DEC], pl.lds_x, w)) return 1;
    const long long N = p->n_rows, L = k.c[LMU].l[0].M, E = k.c[VMU].l[0].M, D = k.c[DEC].l[k.c[DEC].n_layers - 1].M;
    if (k.c[DEC].l[0].K != L + E)
        return lg_fail_msg(f + ": " + kChainVae[DEC] + ".layer[0].n_in = " + std::to_string(k.c[DEC].l[0].K) + ", but [z | v] has " + std::to_string(L) + " + " +
                           std::to_string(E) + " columns (the widths of latent_mu and vel_mu)");
    plan_blank(pl);
    long long off = 0;
    pl.cat_off = k.cat_off = off; off += N * (L + E);
    for (int h = 0; h < NH; h++) { pl.head_off[h] = k.head_off[h] = off; off += N * k.c[LMU + h].l[0].M; }
    pl.gl_rec_off = k.gl_rec_off = off; off += N * D;
    pl.gl_est_off = k.gl_est_off = off; off += N * E;
    PassLayout lay;
    if (plan_layout(f, k, k.c, p->n_rows, ENC, DEC + 1, -1, LG_TRAIN_DWAQ_TARGET_JOBS, w, kRedBytes, false, off, lay)) return 1;
    // plan_layout's loss regions are one (N, H) matrix, H the width chain ENC ends at, and one stream of tile partials at the end of the
    // workspace: the matrix takes the encoder's last output, the partials are lengthened to the four streams with T / B^2 behind them
    pl.enc_out_off = k.enc_off = lay.gl_off;
    pl.partial_off = k.part_off = lay.part_off;
    pl.scale_off = k.scale_off = lay.part_off + 2LL * NQ * k.n_tiles;
    lay.workspace_floats = pl.scale_off + 2;
    plan_out(pl, k, k.c, lay);
    pl.loss_tiles = k.n_tiles;
    place_regions(k);
    return 0;
}

static int check_var_clip(const std::string &f, float var_clip) {
    return var_clip >= 0.f ? 0 : lg_fail_msg(f + ": var_clip must be >= 0");
}

static int bind_noise(const std::string &f, const float *noise, int stride, DArgs &k) {
    const int W = k.c[LMU].l[0].M + k.c[VMU].l[0].M;
    if (!noise) return lg_fail_msg(f + ": noise is null");
    if (stride < W) return lg_fail_msg(f + ": noise_stride = " + std::to_string(stride) + " is below its width " + std::to_string(W));
    k.noise = noise; k.noise_stride = stride;
    return 0;
}

static int bind_rl(const char *fn, const LgTrainDwaqArgs *p, const LgTrainDwaqPlan &pl, DArgs &k, bool backward) {
    const std::string f(fn);
    for (int ci = 0; ci < LG_TRAIN_DWAQ_CHAINS; ci++) {                  // a head has no input of its own
        const int in_width = ci == ACT ? p->n_obs : (ci == ENC || ci == CRI) ? p->chain[ci].layer[0].n_in : 0;
        if (bind_chain(f + ": " + kChainRL[ci], p->chain[ci], k.c[ci], in_width, backward && ci >= ACT)) return 1;
    }
    if (check_var_clip(f, p->var_clip) || bind_noise(f, p->noise, p->noise_stride, k)) return 1;
    if (bind_heads(f, p, k, k.c[ACT], k.c[CRI], pl.workspace_floats, backward)) return 1;
    k.var_clip = p->var_clip;
    k.obs = p->chain[ACT].input; k.obs_stride = p->chain[ACT].in_stride;
    k.c[ACT].in = p->workspace + pl.cat_off; k.c[ACT].in_stride = k.c[ACT].l[0].K;       // the stored concatenation
    return 0;
}

static int bind_vae(const char *fn, const LgTrainVaeArgs *p, const LgTrainDwaqPlan &pl, DArgs &k, bool backward) {
    const std::string f(fn);
    for (int ci = 0; ci < LG_TRAIN_VAE_CHAINS; ci++)
        if (bind_chain(f + ": " + kChainVae[ci], p->chain[ci], k.c[ci], ci == ENC ? p->chain[ci].layer[0].n_in : 0, backward)) return 1;
    const int E = k.c[VMU].l[0].M, D = k.c[DEC].l[k.c[DEC].n_layers - 1].M;
    if (check_var_clip(f, p->var_clip) || bind_noise(f, p->noise, p->noise_stride, k)) return 1;
    if (!p->labels) return lg_fail_msg(f + ": labels is null");
    if (!p->next_states) return lg_fail_msg(f + ": next_states is null");
    if (!p->mask) return lg_fail_msg(f + ": mask is null");
    if (p->labels_stride < E) return lg_fail_msg(f + ": labels_stride = " + std::to_string(p->labels_stride) + " is below its width " + std::to_string(E));
    if (p->next_states_stride < D) return lg_fail_msg(f + ": next_states_stride = " + std::to_string(p->next_states_stride) + " is below its width " + std::to_string(D));
    if (p->mask_stride < 1) return lg_fail_msg(f + ": mask_stride = " + std::to_string(p->mask_stride) + " is below its width 1");
    if (!backward && !p->loss) return lg_fail_msg(f + ": loss is null");
    if (backward && !p->upstream) return lg_fail_msg(f + ": upstream is null");
    if (check_ws(f, p->workspace, p->workspace_capacity, pl.workspace_floats, true)) return 1;
    k.ws = p->workspace;
    k.var_clip = p->var_clip; k.kld_weight = p->kld_weight;
    k.labels = p->labels; k.labels_stride = p->labels_stride; k.next = p->next_states; k.next_stride = p->next_states_stride;
    k.mask = p->mask; k.mask_stride = p->mask_stride;
    k.loss = p->loss; k.upstream = p->upstream;
    for (int h = 0; h < NH; h++) { k.c[LMU + h].in = p->workspace + pl.enc_out_off; k.c[LMU + h].in_stride = k.c[LMU + h].l[0].K; }      // the stored encoder output
    k.c[DEC].in = p->workspace + pl.cat_off; k.c[DEC].in_stride = k.c[DEC].l[0].K;                                                     // the stored draw
    return 0;
}

extern "C" int lg_train_dwaq_plan(const LgTrainDwaqArgs *args, LgTrainDwaqPlan *out) {
    if (!out) return lg_fail_msg("lg_train_dwaq_plan: null plan");
    DArgs k;
    return make_plan_rl("lg_train_dwaq_plan", args, *out, k);
}

extern "C" int lg_train_vae_plan(const LgTrainVaeArgs *args, LgTrainDwaqPlan *out) {
    if (!out) return lg_fail_msg("lg_train_vae_plan: null plan");
    DArgs k;
    return make_plan_vae("lg_train_vae_plan", args, *out, k);
}

extern "C" int lg_train_dwaq_forward(const LgTrainDwaqArgs *args, void *stream) {
    static const char *fn = "lg_train_dwaq_forward";
    LgTrainDwaqPlan pl; DArgs k;
    if (make_plan_rl(fn, args, pl, k) || bind_rl(fn, args, pl, k, false)) return 1;
    return launch_tile(fn, kForward, raised_forward, 2, pl.lds_bytes, (hipStream_t)stream, k) || done(fn);
}

extern "C" int lg_train_dwaq_backward(const LgTrainDwaqArgs *args, void *stream) {
    static const char *fn = "lg_train_dwaq_backward";
    LgTrainDwaqPlan pl; DArgs k;
    if (make_plan_rl(fn, args, pl, k) || bind_rl(fn, args, pl, k, true)) return 1;
    return launch_backward(fn, kInputGrad, raised_input_grad, train_dwaq_weight_grad_kernel, train_dwaq_combine_kernel, 2, pl.lds_bytes, (hipStream_t)stream, k);
}

extern "C" int lg_train_vae_forward(const LgTrainVaeArgs *args, void *stream) {
    static const char *fn = "lg_train_vae_forward";
    LgTrainDwaqPlan pl; DArgs k;
    if (make_plan_vae(fn, args, pl, k) || bind_vae(fn, args, pl, k, false)) return 1;
    if (launch_tile(fn, kVaeForward, raised_vae_forward, 1, pl.lds_bytes, (hipStream_t)stream, k)) return 1;
    hipLaunchKernelGGL(train_vae_finalize_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, k);
    return done(fn);
}

extern "C" int lg_train_vae_backward(const LgTrainVaeArgs *args, void *stream) {
    static const char *fn = "lg_train_vae_backward";
    LgTrainDwaqPlan pl; DArgs k;
    if (make_plan_vae(fn, args, pl, k) || bind_vae(fn, args, pl, k, true)) return 1;
    return launch_backward(fn, kVaeInputGrad, raised_vae_input_grad, train_dwaq_weight_grad_kernel, train_dwaq_combine_kernel, 1, pl.lds_bytes, (hipStream_t)stream, k);
}

// lg_train_ts.hip -- the fused learner passes of the teacher-student family behind include/lgtraints.h: the RL pass of ActorCriticTS
// (privilege encoder -> [obs | z] -> actor, and the critic) with its backward over the actor, the critic AND the privilege encoder, and the
// supervised history-encoder pass (history encoder against the privilege encoder's output as a constant target, masked mean-squared
// error, backward over the history encoder).
//
// Reference call sites replaced: rsl_rl/algorithms/ppo_ts.py:144-187 (_compute_rl_loss's network calls, _compute_encoder_loss) and the
// share of the two loss.backward() calls of PPO_TS.update() (ppo_ts.py:110-133) that runs through the four MLPs of
// rsl_rl/modules/actor_critic_ts.py:46-126,163-169.
//
// The layer routines are lg_train_tiles.h's (shared with lg_train.hip, where the MFMA layouts are described, and lg_train_ee.hip).  What is
// new here:
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
#include <string>
#include "lg_train_tiles.h"
#include "../../include/lgtraints.h"

int lg_fail_msg(const std::string &m);   // lg_host.hip: sets the thread-local message, returns 1

#define PRI LG_TRAIN_TS_PRIVILEGE
#define ACT LG_TRAIN_TS_ACTOR
#define CRI LG_TRAIN_TS_CRITIC
#define HIS LG_TRAIN_TS_HISTORY
static const int kRedBytes = LG_TRAIN_TS_THREADS * (int)sizeof(double);
static_assert(LG_TRAIN_TS_THREADS == kThreads, "the loss tree has one leaf per thread of the row-tile workgroup");

struct SArgs {
    TChain c[LG_TRAIN_TS_CHAINS];
    float *ws;
    const float *obs;           // (N, O): the first columns of the actor's input
    const float *std, *grad_sigma;
    float *grad_std, *sigma;
    const float *mask, *upstream;
    float *loss;
    int N, R, q_off, red_off, A, clip_on;
    float clip;
    int obs_stride, sigma_stride, grad_sigma_stride, mask_stride;
    int std_S, std_rps, std_job0, n_jobs;
    int c0, c1;                 // the chains of the backward launches
    int enc_start, n_tiles, enc_pass;
    long long std_p_off, cat_off, gl_off, y_off, part_off;
};
static_assert(sizeof(SArgs) <= 4096, "SArgs is passed by value: the kernel-argument segment is 4 KB");

// the chain over the row tile; its input is staged in b0 and a barrier has passed.  Returns the activation that holds the last layer's
// output (a barrier has passed behind it).  store_h: every hidden activation to the workspace while the next layer reads it.
template <int RB>
__device__ __forceinline__ lds_f *chain_forward(const SArgs &a, const TChain &c, lds_f *b0, lds_f *b1, bool store_h, bool clip_last, int rows, int row0) {
    lds_f *buf[2] = {b0, b1};
    for (int li = 0; li < c.n_layers; li++) {
        const TLayer &L = c.l[li];
        const bool clip_on = clip_last && li == c.n_layers - 1;
        const int per_wave = (((L.M + 15) >> 4) + kWaves - 1) / kWaves;
        if (li && store_h) copy_out(buf[li & 1], L.sa, a.ws + c.l[li - 1].h_off, L.K, L.K, rows, row0);
        if (per_wave >= 4) fwd_tile<RB, 4>(L, buf[li & 1], buf[(li + 1) & 1], clip_on, a.clip, a.R);
        else if (per_wave >= 2) fwd_tile<RB, 2>(L, buf[li & 1], buf[(li + 1) & 1], clip_on, a.clip, a.R);
        else fwd_tile<RB, 1>(L, buf[li & 1], buf[(li + 1) & 1], clip_on, a.clip, a.R);
        __syncthreads();
    }
    return buf[c.n_layers & 1];
}

// one input-gradient layer: nxt = (cur W) * elu'(nxt), by the widest tile count the layer fills
template <int RB>
__device__ __forceinline__ void bwd_layer(const TLayer &L, const lds_f *cur, lds_f *nxt, bool prev_elu, int R) {
    const int per_wave = (((L.K + 15) >> 4) + kWaves - 1) / kWaves;
    if (per_wave >= 4) bwd_tile<RB, 4>(L, cur, nxt, prev_elu, R);
    else if (per_wave >= 2) bwd_tile<RB, 2>(L, cur, nxt, prev_elu, R);
    else bwd_tile<RB, 1>(L, cur, nxt, prev_elu, R);
}

// the input gradients of a chain from its last layer down to layer 1.  G of the last layer sits in b[n_layers & 1] at that layer's output
// stride and a barrier has passed; b0 / b1 are the activations the chain's forward started and continued in.  On return G_0 sits in b1
// and a barrier has passed behind it; it is read-only until the next barrier (its copy to the workspace is in flight).
template <int RB>
__device__ __forceinline__ void chain_backward(const SArgs &a, const TChain &c, lds_f *b0, lds_f *b1, int rows, int row0) {
    lds_f *buf[2] = {b0, b1};
    for (int li = c.n_layers - 1; li >= 1; li--) {
        const TLayer &L = c.l[li], &P = c.l[li - 1];
        lds_f *cur = buf[(li + 1) & 1], *nxt = buf[li & 1];
        if (P.elu) {                                                   // H_(l-1) into the destination tile: the epilogue turns it into G_(l-1) in place
            stage_rows(a.ws + P.h_off, L.K, L.K, nxt, L.sa, a.R, rows, row0);
            __syncthreads();
        }
        bwd_layer<RB>(L, cur, nxt, P.elu != 0, a.R);
        __syncthreads();
        copy_out(nxt, L.sa, a.ws + P.g_off, L.K, L.K, rows, row0);     // read-only until the barrier behind the next layer's stage
    }
}

template <int RB> __global__ __launch_bounds__(256) void train_ts_forward_kernel(SArgs a) {
    extern __shared__ __align__(16) float lds[];
    const int R = a.R, row0 = blockIdx.x * R;
    const int rows = min(R, a.N - row0);
    lds_f *b0 = (lds_f *)lds, *b1 = (lds_f *)lds + a.q_off;
    if (blockIdx.y == 1) {
        const TChain &c = a.c[CRI];
        stage_rows(c.in, c.l[0].K, c.in_stride, b0, c.l[0].sa, R, rows, row0);
        __syncthreads();
        const lds_f *v = chain_forward<RB>(a, c, b0, b1, true, false, rows, row0);
        copy_out(v, c.l[c.n_layers - 1].so, c.out, c.l[c.n_layers - 1].M, c.out_stride, rows, row0);
        return;
    }
    const TChain &e = a.c[PRI], &c = a.c[ACT];
    const int Z = e.l[e.n_layers - 1].M, O = c.l[0].K - Z;
    lds_f *s0 = a.enc_start ? b1 : b0, *s1 = a.enc_start ? b0 : b1;
    stage_rows(e.in, e.l[0].K, e.in_stride, s0, e.l[0].sa, R, rows, row0);
    __syncthreads();
    const lds_f *z = chain_forward<RB>(a, e, s0, s1, true, false, rows, row0);         // ends in b1: enc_start is chosen so
    const int sa = c.l[0].sa, sz = e.l[e.n_layers - 1].so;
    stage_rows(a.obs, O, a.obs_stride, b0, sa, R, rows, row0);                         // [obs | z] in b0, at the actor's stride
    for (int i = threadIdx.x; i < R * Z; i += kThreads) {
        const int row = i / Z, col = i - row * Z;
        b0[row * sa + O + col] = row < rows ? z[row * sz + col] : 0.f;
    }
    __syncthreads();
    copy_out(b0, sa, a.ws + a.cat_off, O + Z, O + Z, rows, row0);
    const lds_f *m = chain_forward<RB>(a, c, b0, b1, true, a.clip_on != 0, rows, row0);
    const int sm = c.l[c.n_layers - 1].so, A = a.A;
    copy_out(m, sm, c.out, A, c.out_stride, rows, row0);
    for (int t = threadIdx.x; t < rows * A; t += kThreads) {
        const int row = t / A, ai = t - row * A;
        a.sigma[(size_t)(row0 + row) * a.sigma_stride + ai] = m[row * sm + ai] * 0.f + a.std[ai];
    }
}

template <int RB> __global__ __launch_bounds__(256) void train_enc_forward_kernel(SArgs a) {
    extern __shared__ __align__(16) float lds[];
    const TChain &e = a.c[PRI], &c = a.c[HIS];
    const int R = a.R, row0 = blockIdx.x * R;
    const int rows = min(R, a.N - row0);
    lds_f *b0 = (lds_f *)lds, *b1 = (lds_f *)lds + a.q_off;
    const int Z = c.l[c.n_layers - 1].M;
    float *yw = a.ws + a.y_off;
    stage_rows(e.in, e.l[0].K, e.in_stride, b0, e.l[0].sa, R, rows, row0);
    __syncthreads();
    const lds_f *y = chain_forward<RB>(a, e, b0, b1, false, false, rows, row0);        // the target: nothing stored, no gradient
    copy_out(y, e.l[e.n_layers - 1].so, yw, Z, Z, rows, row0);                         // this tile's rows; read back below by this workgroup only
    __syncthreads();                                                                   // y has left the LDS before the history is staged over it
    stage_rows(c.in, c.l[0].K, c.in_stride, b0, c.l[0].sa, R, rows, row0);
    __syncthreads();
    const lds_f *p = chain_forward<RB>(a, c, b0, b1, true, false, rows, row0);
    const int sp = c.l[c.n_layers - 1].so;
    const float scale = 2.0f / ((float)a.N * (float)Z);
    float *gl = a.ws + a.gl_off;
    double acc = 0.0;
    for (int i = threadIdx.x; i < rows * Z; i += kThreads) {
        const int row = i / Z, col = i - row * Z;
        const float t = a.mask[(size_t)(row0 + row) * a.mask_stride];
        const float d = (p[row * sp + col] - yw[(size_t)(row0 + row) * Z + col]) * t;       // NaN * 0 stays NaN, as in torch
        gl[(size_t)(row0 + row) * Z + col] = d * t * scale;
        acc += (double)d * (double)d;
    }
    volatile double *red = (volatile double *)(lds + a.red_off);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {                                         // a fixed tree over the 256 thread sums
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) ((double *)(a.ws + a.part_off))[blockIdx.x] = red[0];
}

// one workgroup: the tile partials in tile order.  256 of them at a time reach LDS through parallel loads; thread 0 adds them in order.
__global__ __launch_bounds__(256) void train_enc_finalize_kernel(SArgs a) {
    __shared__ double part[kThreads];
    const double *P = (const double *)(a.ws + a.part_off);
    double sum = 0.0;
    for (int t0 = 0; t0 < a.n_tiles; t0 += kThreads) {
        const int n = min(kThreads, a.n_tiles - t0);
        if ((int)threadIdx.x < n) part[threadIdx.x] = P[t0 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < n; i++) sum += part[i];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.loss[0] = (float)(sum / ((double)a.N * (double)a.c[HIS].l[a.c[HIS].n_layers - 1].M));
}

// grid (row tiles, 2) in the RL pass: y = 0 the actor and, through the latent, the privilege encoder; y = 1 the critic.  Grid (row tiles,
// 1) in the encoder pass: the history encoder.
template <int RB> __global__ __launch_bounds__(256) void train_ts_input_grad_kernel(SArgs a) {
    extern __shared__ __align__(16) float lds[];
    const int ci = a.enc_pass ? HIS : (blockIdx.y ? CRI : ACT);
    const TChain &c = a.c[ci];
    const int R = a.R, row0 = blockIdx.x * R, nl = c.n_layers;
    const int rows = min(R, a.N - row0);
    lds_f *b0 = (lds_f *)lds, *b1 = (lds_f *)lds + a.q_off;
    {   // G of the last layer: gl times the upstream scalar (encoder pass), or the incoming gradient, behind the Hardtanh's mask for the actor
        const TLayer &L = c.l[nl - 1];
        lds_f *g = (nl & 1) ? b1 : b0;
        float *gws = a.ws + L.g_off;
        const bool mask = ci == ACT && a.clip_on;
        const int w = L.M;
        const float up = a.enc_pass ? a.upstream[0] : 1.f;
        for (int i = threadIdx.x; i < R * w; i += kThreads) {
            const int row = i / w, col = i - row * w;
            float v = 0.f;
            if (row < rows) {
                if (a.enc_pass) v = a.ws[a.gl_off + (size_t)(row0 + row) * w + col] * up;
                else {
                    v = c.gin[(size_t)(row0 + row) * c.gin_stride + col];
                    if (mask) {
                        const float m = c.out[(size_t)(row0 + row) * c.out_stride + col];
                        if (m >= a.clip || m <= -a.clip) v = 0.f;             // hardtanh_backward: a NaN mean passes the gradient on
                    }
                }
                gws[(size_t)(row0 + row) * w + col] = v;
            }
            g[row * L.so + col] = v;
        }
    }
    __syncthreads();
    chain_backward<RB>(a, c, b0, b1, rows, row0);
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
    chain_backward<RB>(a, e, s0, s1, rows, row0);
}

// one wave per job: (layer, 64 x 64 tile of its gradient, batch slice) of the chains [c0, c1), or a slice of grad_std's column sums
__global__ __launch_bounds__(64) void train_ts_weight_grad_kernel(SArgs a) {
    const int job = blockIdx.x;
    if (job >= a.std_job0) {
        colsum_wave(a.grad_sigma, a.grad_sigma_stride, a.A, a.ws + a.std_p_off, job - a.std_job0, a.std_rps, a.N);
        return;
    }
    int ci = a.c0, li = 0;
    for (int c = a.c0; c < a.c1; c++)
        for (int l = 0; l < a.c[c].n_layers; l++)
            if (job >= a.c[c].l[l].job0) { ci = c; li = l; }          // job0 rises with (c, l)
    const TChain &c = a.c[ci];
    const TLayer &L = c.l[li];
    wgrad_wave(L, a.ws + L.g_off, li ? a.ws + c.l[li - 1].h_off : c.in, li ? L.K : c.in_stride, a.ws, job - L.job0, a.N);    // the actor's `in` is the stored concatenation
}

__global__ __launch_bounds__(256) void train_ts_combine_kernel(SArgs a) {
    const long long stride = (long long)gridDim.x * blockDim.x, first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (int ci = a.c0; ci < a.c1; ci++)
        for (int li = 0; li < a.c[ci].n_layers; li++) combine_layer(a.c[ci].l[li], a.ws, first, stride);
    if (a.std_S) combine_cols(a.ws + a.std_p_off, a.A, a.std_S, a.grad_std, first, stride);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static const char *kChainTS[LG_TRAIN_TS_CHAINS] = {"chain[0] (privilege encoder)", "chain[1] (actor)", "chain[2] (critic)", ""};
static const char *kChainEnc[LG_TRAIN_ENC_CHAINS] = {"chain[0] (history encoder)", "chain[1] (privilege encoder)"};
static const int kEncChain[LG_TRAIN_ENC_CHAINS] = {HIS, PRI};          // LgTrainEncArgs::chain[i] is chain kEncChain[i] of the kernels

// widths and layer count of one chain into t; `first`: the LDS activation its input sits in
static int plan_chain(const std::string &cn, const LgTrainChain &c, TChain &t, int first, int w[2]) {
    if (c.n_layers < 1 || c.n_layers > kMaxL) return lg_fail_msg(cn + ".n_layers = " + std::to_string(c.n_layers) + " is outside [1, " + std::to_string(kMaxL) + "]");
    int width = c.layer[0].n_in;
    for (int li = 0; li < c.n_layers; li++) {
        const LgTrainLayer &l = c.layer[li];
        const std::string ln = cn + ".layer[" + std::to_string(li) + "]";
        if (l.n_in < 1 || l.n_in > LG_POLICY_MAX_WIDTH) return lg_fail_msg(ln + ".n_in = " + std::to_string(l.n_in) + " is outside [1, " + std::to_string(LG_POLICY_MAX_WIDTH) + "]");
        if (l.n_out < 1 || l.n_out > LG_POLICY_MAX_WIDTH) return lg_fail_msg(ln + ".n_out = " + std::to_string(l.n_out) + " is outside [1, " + std::to_string(LG_POLICY_MAX_WIDTH) + "]");
        if (l.n_in != width) return lg_fail_msg(ln + ".n_in = " + std::to_string(l.n_in) + ", but its input has " + std::to_string(width) + " columns");
        width = l.n_out;
        TLayer &L = t.l[li];
        L.K = l.n_in; L.M = l.n_out; L.elu = l.elu != 0;
        L.sa = lds_stride(l.n_in); L.so = lds_stride(l.n_out);
        if (L.sa > w[(li + first) & 1]) w[(li + first) & 1] = L.sa;
        if (L.so > w[(li + first + 1) & 1]) w[(li + first + 1) & 1] = L.so;
    }
    t.n_layers = c.n_layers;
    return 0;
}

// offsets, slices and jobs of the chains [c0, c1) behind `off`; the LDS tile
static int plan_rest(const std::string &f, int N, int c0, int c1, bool std_on, const int w[2], int extra_lds, long long off, LgTrainTSPlan &pl, SArgs &k) {
    int jobs = 0;
    for (int ci = 0; ci < LG_TRAIN_TS_CHAINS; ci++)
        for (int li = 0; li < LG_POLICY_MAX_LAYERS; li++) pl.h_off[ci][li] = pl.g_off[ci][li] = pl.p_off[ci][li] = -1;
    for (int ci = c0; ci < c1; ci++)
        for (int li = 0; li < k.c[ci].n_layers; li++) {
            TLayer &L = k.c[ci].l[li];
            if (li < k.c[ci].n_layers - 1) { L.h_off = pl.h_off[ci][li] = off; off += (long long)N * L.M; }
            L.g_off = pl.g_off[ci][li] = off; off += (long long)N * L.M;
        }
    for (int ci = c0; ci < c1; ci++)
        for (int li = 0; li < k.c[ci].n_layers; li++) {
            TLayer &L = k.c[ci].l[li];
            const int tn = (L.M + LG_TRAIN_WG_TILE - 1) / LG_TRAIN_WG_TILE;
            L.tiles_k = (L.K + LG_TRAIN_WG_TILE - 1) / LG_TRAIN_WG_TILE;
            slice_rule(N, (long long)tn * L.tiles_k, L.S, L.rps, LG_TRAIN_TS_TARGET_JOBS);
            pl.slices[ci][li] = L.S; pl.slice_rows[ci][li] = L.rps;
            L.p_off = pl.p_off[ci][li] = off; off += (long long)L.S * ((long long)L.M * L.K + L.M);
            L.job0 = jobs; jobs += L.S * tn * L.tiles_k;
        }
    pl.std_p_off = -1;
    if (std_on) {
        k.A = k.c[ACT].l[k.c[ACT].n_layers - 1].M;
        slice_rule(N, 1, k.std_S, k.std_rps, LG_TRAIN_TS_TARGET_JOBS);
        pl.std_slices = k.std_S; pl.std_slice_rows = k.std_rps;
        k.std_p_off = pl.std_p_off = off; off += (long long)k.std_S * k.A;
    }
    k.std_job0 = jobs; jobs += k.std_S;
    k.n_jobs = pl.weight_jobs = jobs;
    k.N = N; k.c0 = c0; k.c1 = c1;
    for (int R = 32; R >= 8; R >>= 1) {
        const size_t bytes = (size_t)R * (w[0] + w[1]) * sizeof(float) + extra_lds;
        if (bytes <= kLdsBytes) {
            k.R = pl.row_tile = R; k.q_off = R * w[0]; k.red_off = R * (w[0] + w[1]); pl.lds_bytes = (int)bytes;
            k.n_tiles = (N + R - 1) / R;
            if (extra_lds) {                                         // the encoder pass: gl, the targets and the float64 tile partials
                const int Z = k.c[HIS].l[k.c[HIS].n_layers - 1].M;
                k.gl_off = pl.gl_off = off; off += (long long)N * Z;
                k.y_off = pl.y_off = off; off += (long long)N * Z;
                off += off & 1;
                k.part_off = pl.partial_off = off; off += 2LL * k.n_tiles;
                pl.loss_tiles = k.n_tiles;
            }
            pl.workspace_floats = off;
            return 0;
        }
    }
    return lg_fail_msg(f + ": an 8-row tile of these widths (" + std::to_string(w[0] + w[1]) + " floats per row) does not fit the 160 KB of LDS");
}

static int make_plan_ts(const char *fn, const LgTrainTSArgs *p, LgTrainTSPlan &pl, SArgs &k) {
    const std::string f(fn);
    if (!p) return lg_fail_msg(f + ": null descriptor");
    if (p->n_rows < 1) return lg_fail_msg(f + ": n_rows = " + std::to_string(p->n_rows) + " < 1");
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
    pl.gl_off = pl.y_off = pl.partial_off = -1;
    return plan_rest(f, p->n_rows, PRI, CRI + 1, true, w, 0, (long long)p->n_rows * (O + Z), pl, k);
}

static int make_plan_enc(const char *fn, const LgTrainEncArgs *p, LgTrainTSPlan &pl, SArgs &k) {
    const std::string f(fn);
    if (!p) return lg_fail_msg(f + ": null descriptor");
    if (p->n_rows < 1) return lg_fail_msg(f + ": n_rows = " + std::to_string(p->n_rows) + " < 1");
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
    return plan_rest(f, p->n_rows, HIS, HIS + 1, false, w, kRedBytes, 0, pl, k);
}

static int bind_chain(const std::string &cn, const LgTrainChain &c, TChain &t, int in_width, bool grads) {
    if (!c.input) return lg_fail_msg(cn + ".input is null");
    if (c.in_stride < in_width) return lg_fail_msg(cn + ".in_stride = " + std::to_string(c.in_stride) + " is below its width " + std::to_string(in_width));
    t.in = c.input; t.in_stride = c.in_stride;
    for (int li = 0; li < c.n_layers; li++) {
        const LgTrainLayer &l = c.layer[li];
        const std::string ln = cn + ".layer[" + std::to_string(li) + "]";
        if (!l.weight) return lg_fail_msg(ln + ".weight is null");
        if (!l.bias) return lg_fail_msg(ln + ".bias is null");
        if (grads && !l.grad_weight) return lg_fail_msg(ln + ".grad_weight is null");
        if (grads && !l.grad_bias) return lg_fail_msg(ln + ".grad_bias is null");
        TLayer &L = t.l[li];
        L.W = l.weight; L.b = l.bias;
        L.gW = grads ? l.grad_weight : nullptr; L.gb = grads ? l.grad_bias : nullptr;      // gradient pointers of a chain outside the backward are not even copied
    }
    return 0;
}

static int check_ws(const std::string &f, const float *ws, long long cap, const LgTrainTSPlan &pl, bool align8) {
    if (!ws) return lg_fail_msg(f + ": workspace is null");
    if (align8 && ((uintptr_t)ws & 7)) return lg_fail_msg(f + ": workspace is not 8-byte aligned (it holds the float64 partials)");
    if (cap < pl.workspace_floats)
        return lg_fail_msg(f + ": workspace_capacity = " + std::to_string(cap) + " floats is below the plan's " + std::to_string((long long)pl.workspace_floats));
    return 0;
}

static int bind_ts(const char *fn, const LgTrainTSArgs *p, const LgTrainTSPlan &pl, SArgs &k, bool backward) {
    const std::string f(fn);
    for (int ci = 0; ci < LG_TRAIN_TS_RL_CHAINS; ci++)
        if (bind_chain(f + ": " + kChainTS[ci], p->chain[ci], k.c[ci], ci == ACT ? p->n_obs : p->chain[ci].layer[0].n_in, backward)) return 1;
    const int A = k.A, V = k.c[CRI].l[k.c[CRI].n_layers - 1].M;
    if (p->clip_on && !(p->clip_actions >= 0.f)) return lg_fail_msg(f + ": clip_actions must be >= 0 under clip_on");
    if (!p->std) return lg_fail_msg(f + ": std is null");
    if (!p->mu) return lg_fail_msg(f + ": mu is null");
    if (!p->sigma) return lg_fail_msg(f + ": sigma is null");
    if (!p->values) return lg_fail_msg(f + ": values is null");
    if (p->mu_stride < A) return lg_fail_msg(f + ": mu_stride = " + std::to_string(p->mu_stride) + " is below its width " + std::to_string(A));
    if (p->sigma_stride < A) return lg_fail_msg(f + ": sigma_stride = " + std::to_string(p->sigma_stride) + " is below its width " + std::to_string(A));
    if (p->values_stride < V) return lg_fail_msg(f + ": values_stride = " + std::to_string(p->values_stride) + " is below its width " + std::to_string(V));
    if (backward) {
        if (!p->grad_std) return lg_fail_msg(f + ": grad_std is null");
        if (!p->grad_mu) return lg_fail_msg(f + ": grad_mu is null");
        if (!p->grad_sigma) return lg_fail_msg(f + ": grad_sigma is null");
        if (!p->grad_values) return lg_fail_msg(f + ": grad_values is null");
        if (p->grad_mu_stride < A) return lg_fail_msg(f + ": grad_mu_stride = " + std::to_string(p->grad_mu_stride) + " is below its width " + std::to_string(A));
        if (p->grad_sigma_stride < A) return lg_fail_msg(f + ": grad_sigma_stride = " + std::to_string(p->grad_sigma_stride) + " is below its width " + std::to_string(A));
        if (p->grad_values_stride < V) return lg_fail_msg(f + ": grad_values_stride = " + std::to_string(p->grad_values_stride) + " is below its width " + std::to_string(V));
    }
    if (check_ws(f, p->workspace, p->workspace_capacity, pl, false)) return 1;
    k.ws = p->workspace;
    k.obs = p->chain[ACT].input; k.obs_stride = p->chain[ACT].in_stride;
    k.c[ACT].in = p->workspace + pl.cat_off; k.c[ACT].in_stride = k.c[ACT].l[0].K;       // the stored concatenation
    k.c[ACT].out = p->mu; k.c[ACT].out_stride = p->mu_stride;
    k.c[CRI].out = p->values; k.c[CRI].out_stride = p->values_stride;
    k.c[ACT].gin = p->grad_mu; k.c[ACT].gin_stride = p->grad_mu_stride;
    k.c[CRI].gin = p->grad_values; k.c[CRI].gin_stride = p->grad_values_stride;
    k.std = p->std; k.grad_std = p->grad_std; k.sigma = p->sigma; k.sigma_stride = p->sigma_stride;
    k.grad_sigma = p->grad_sigma; k.grad_sigma_stride = p->grad_sigma_stride;
    k.clip_on = p->clip_on != 0; k.clip = p->clip_actions;
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
    if (check_ws(f, p->workspace, p->workspace_capacity, pl, true)) return 1;
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

// once per device and kernel: dynamic LDS above 64 KB has to be asked for (an unsynchronised race sets the same value twice: harmless)
static int raise_lds(const char *fn, int which, int rb) {
    static bool raised[64][3][2];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return lg_fail_msg(std::string(fn) + ": no current HIP device");
    if (raised[dev][which][rb]) return 0;
    const void *fp[3][2] = {{(const void *)train_ts_forward_kernel<1>, (const void *)train_ts_forward_kernel<2>},
                            {(const void *)train_enc_forward_kernel<1>, (const void *)train_enc_forward_kernel<2>},
                            {(const void *)train_ts_input_grad_kernel<1>, (const void *)train_ts_input_grad_kernel<2>}};
    const hipError_t e = hipFuncSetAttribute(fp[which][rb], hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (e != hipSuccess) return lg_fail_msg(std::string(fn) + ": hipFuncSetAttribute: " + hipGetErrorString(e));
    raised[dev][which][rb] = true;
    return 0;
}

static int done(const char *fn) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : lg_fail_msg(std::string(fn) + ": " + hipGetErrorString(e));
}

// the three launches of a backward over the chains [c0, c1) of k
static int launch_backward(const char *fn, const LgTrainTSPlan &pl, const SArgs &k, hipStream_t stream) {
    const int rb = k.R == 32;
    if (raise_lds(fn, 2, rb)) return 1;
    const dim3 grid((unsigned)k.n_tiles, k.enc_pass ? 1u : 2u);
    if (rb) hipLaunchKernelGGL(train_ts_input_grad_kernel<2>, grid, dim3(kThreads), (size_t)pl.lds_bytes, stream, k);
    else hipLaunchKernelGGL(train_ts_input_grad_kernel<1>, grid, dim3(kThreads), (size_t)pl.lds_bytes, stream, k);
    hipLaunchKernelGGL(train_ts_weight_grad_kernel, dim3((unsigned)k.n_jobs), dim3(64), 0, stream, k);
    long long elems = k.A;
    for (int ci = k.c0; ci < k.c1; ci++)
        for (int li = 0; li < k.c[ci].n_layers; li++) {
            const long long n = (long long)k.c[ci].l[li].M * k.c[ci].l[li].K + k.c[ci].l[li].M;
            if (n > elems) elems = n;
        }
    long long blocks = (elems + 255) / 256;
    if (blocks > 1024) blocks = 1024;                    // grid-stride behind that
    hipLaunchKernelGGL(train_ts_combine_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, k);
    return done(fn);
}

extern "C" int lg_train_ts_forward(const LgTrainTSArgs *args, void *stream) {
    static const char *fn = "lg_train_ts_forward";
    LgTrainTSPlan pl; SArgs k;
    if (make_plan_ts(fn, args, pl, k) || bind_ts(fn, args, pl, k, false)) return 1;
    const int rb = k.R == 32;
    if (raise_lds(fn, 0, rb)) return 1;
    const dim3 grid((unsigned)k.n_tiles, 2);
    if (rb) hipLaunchKernelGGL(train_ts_forward_kernel<2>, grid, dim3(kThreads), (size_t)pl.lds_bytes, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(train_ts_forward_kernel<1>, grid, dim3(kThreads), (size_t)pl.lds_bytes, (hipStream_t)stream, k);
    return done(fn);
}

extern "C" int lg_train_ts_backward(const LgTrainTSArgs *args, void *stream) {
    static const char *fn = "lg_train_ts_backward";
    LgTrainTSPlan pl; SArgs k;
    if (make_plan_ts(fn, args, pl, k) || bind_ts(fn, args, pl, k, true)) return 1;
    return launch_backward(fn, pl, k, (hipStream_t)stream);
}

extern "C" int lg_train_enc_forward(const LgTrainEncArgs *args, void *stream) {
    static const char *fn = "lg_train_enc_forward";
    LgTrainTSPlan pl; SArgs k;
    if (make_plan_enc(fn, args, pl, k) || bind_enc(fn, args, pl, k, false)) return 1;
    const int rb = k.R == 32;
    if (raise_lds(fn, 1, rb)) return 1;
    if (rb) hipLaunchKernelGGL(train_enc_forward_kernel<2>, dim3((unsigned)k.n_tiles), dim3(kThreads), (size_t)pl.lds_bytes, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(train_enc_forward_kernel<1>, dim3((unsigned)k.n_tiles), dim3(kThreads), (size_t)pl.lds_bytes, (hipStream_t)stream, k);
    hipLaunchKernelGGL(train_enc_finalize_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, k);
    return done(fn);
}

extern "C" int lg_train_enc_backward(const LgTrainEncArgs *args, void *stream) {
    static const char *fn = "lg_train_enc_backward";
    LgTrainTSPlan pl; SArgs k;
    if (make_plan_enc(fn, args, pl, k) || bind_enc(fn, args, pl, k, true)) return 1;
    return launch_backward(fn, pl, k, (hipStream_t)stream);
}

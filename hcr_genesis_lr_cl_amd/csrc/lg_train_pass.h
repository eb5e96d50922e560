// lg_train_pass.h -- what a fused learner pass is made of around the layer routines of lg_train_tiles.h, once for lg_train.hip (the plain
// ActorCritic), lg_train_ee.hip (ActorCriticEE) and lg_train_ts.hip (ActorCriticTS): on the device the chain over a row tile forward and
// backward, the seed of the last layer's G, the masked mean-squared-error tile step with its float64 tree and the finalize, the
// weight-gradient job dispatch and the combine; on the host the chain and layout plans, the binds with their refusals, the LDS raise and
// the launches.  A unit keeps its __global__ kernels, its kernel-argument struct (the chains it has, behind PArgs) and its extern "C"
// entry points.  Everything here is inlined into the including unit; nothing is exported.
#ifndef LG_TRAIN_PASS_H
#define LG_TRAIN_PASS_H
#include <string>
#include "lg_train_tiles.h"

int lg_fail_msg(const std::string &m);   // lg_host.hip: sets the thread-local message, returns 1

// the kernel-argument members every pass has; TArgs, EArgs and SArgs put their chains (2, 3, 4) and what is theirs alone behind it
struct PArgs {
    float *ws;
    const float *std, *grad_sigma;
    float *grad_std, *sigma;
    int N, R, q_off, red_off, A, clip_on;
    float clip;
    int sigma_stride, grad_sigma_stride;
    int std_S, std_rps, std_job0, n_jobs;
    int c0, c1;                 // the chains of the backward launches
    int n_tiles;
    long long std_p_off;
};

// the chain over the row tile; its input is staged in b0 and a barrier has passed.  Returns the activation that holds the last layer's
// output (a barrier has passed behind it).  store_h: every hidden activation to the workspace while the next layer reads it.
template <int RB>
__device__ __forceinline__ lds_f *chain_forward(float *ws, const TChain &c, lds_f *b0, lds_f *b1, bool store_h, bool clip_last, float clip, int R, int rows, int row0) {
    lds_f *buf[2] = {b0, b1};
    for (int li = 0; li < c.n_layers; li++) {
        const TLayer &L = c.l[li];
        const bool clip_on = clip_last && li == c.n_layers - 1;
        const int per_wave = (((L.M + 15) >> 4) + kWaves - 1) / kWaves;
        if (li && store_h) copy_out(buf[li & 1], L.sa, ws + c.l[li - 1].h_off, L.K, L.K, rows, row0);
        if (per_wave >= 4) fwd_tile<RB, 4>(L, buf[li & 1], buf[(li + 1) & 1], clip_on, clip, R);
        else if (per_wave >= 2) fwd_tile<RB, 2>(L, buf[li & 1], buf[(li + 1) & 1], clip_on, clip, R);
        else fwd_tile<RB, 1>(L, buf[li & 1], buf[(li + 1) & 1], clip_on, clip, R);
        __syncthreads();
    }
    return buf[c.n_layers & 1];
}

// the same from the chain's own input rows, staged into b0 first
template <int RB>
__device__ __forceinline__ lds_f *chain_from_rows(float *ws, const TChain &c, lds_f *b0, lds_f *b1, bool store_h, bool clip_last, float clip, int R, int rows, int row0) {
    stage_rows(c.in, c.l[0].K, c.in_stride, b0, c.l[0].sa, R, rows, row0);
    __syncthreads();
    return chain_forward<RB>(ws, c, b0, b1, store_h, clip_last, clip, R, rows, row0);
}

// sigma = mu * 0 + std over the tile's rows, from the means in LDS (a NaN mean gives a NaN sigma, as in torch)
__device__ __forceinline__ void store_sigma(const lds_f *m, int sm, int A, const float *std, float *sigma, int stride, int rows, int row0) {
    for (int t = threadIdx.x; t < rows * A; t += kThreads) {
        const int row = t / A, ai = t - row * A;
        sigma[(size_t)(row0 + row) * stride + ai] = m[row * sm + ai] * 0.f + std[ai];
    }
}

// G of the chain's last layer into `g` (LDS, at that layer's output stride) and into the workspace: gl times the upstream scalar, read on
// the device (a loss pass: gl is not null), or the incoming gradient c.gin, behind the Hardtanh's mask where `mask` (the actor under
// clip_on); rows behind `rows` are zero
__device__ __forceinline__ void seed_last_g(float *ws, const TChain &c, lds_f *g, const float *gl, const float *upstream, bool mask, float clip, int R, int rows, int row0) {
    const TLayer &L = c.l[c.n_layers - 1];
    float *gws = ws + L.g_off;
    const int w = L.M;
    const float up = gl ? upstream[0] : 1.f;
    for (int i = threadIdx.x; i < R * w; i += kThreads) {
        const int row = i / w, col = i - row * w;
        float v = 0.f;
        if (row < rows) {
            if (gl) v = gl[(size_t)(row0 + row) * w + col] * up;
            else {
                v = c.gin[(size_t)(row0 + row) * c.gin_stride + col];
                if (mask) {
                    const float m = c.out[(size_t)(row0 + row) * c.out_stride + col];
                    if (m >= clip || m <= -clip) v = 0.f;                     // hardtanh_backward: a NaN mean passes the gradient on
                }
            }
            gws[(size_t)(row0 + row) * w + col] = v;
        }
        g[row * L.so + col] = v;
    }
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
__device__ __forceinline__ void chain_backward(float *ws, const TChain &c, lds_f *b0, lds_f *b1, int R, int rows, int row0) {
    lds_f *buf[2] = {b0, b1};
    for (int li = c.n_layers - 1; li >= 1; li--) {
        const TLayer &L = c.l[li], &P = c.l[li - 1];
        lds_f *cur = buf[(li + 1) & 1], *nxt = buf[li & 1];
        if (P.elu) {                                                   // H_(l-1) into the destination tile: the epilogue turns it into G_(l-1) in place
            stage_rows(ws + P.h_off, L.K, L.K, nxt, L.sa, R, rows, row0);
            __syncthreads();
        }
        bwd_layer<RB>(L, cur, nxt, P.elu != 0, R);
        __syncthreads();
        copy_out(nxt, L.sa, ws + P.g_off, L.K, L.K, rows, row0);       // read-only until the barrier behind the next layer's stage
    }
}

// the masked mean-squared error of a row tile: d = (p - y) t per element of the prediction p (LDS, NL columns) against the target rows y,
// gl = d t scale to the workspace for the backward, and the tile's float64 sum of d^2 by a fixed tree over the 256 thread sums in `red`
__device__ __forceinline__ void mse_tile(const lds_f *p, int sp, int NL, const float *y, int y_stride, const float *mask, int mask_stride, float *gl, float scale,
                                         volatile double *red, double *part, int rows, int row0) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < rows * NL; i += kThreads) {
        const int row = i / NL, col = i - row * NL;
        const float t = mask[(size_t)(row0 + row) * mask_stride];
        const float d = (p[row * sp + col] - y[(size_t)(row0 + row) * y_stride + col]) * t;       // NaN * 0 stays NaN, as in torch
        gl[(size_t)(row0 + row) * NL + col] = d * t * scale;
        acc += (double)d * (double)d;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// one workgroup: the tile partials in tile order.  256 of them at a time reach LDS through parallel loads; thread 0 adds them in order.
__device__ __forceinline__ void loss_finalize(const double *P, int n_tiles, int N, int NL, float *loss) {
    __shared__ double part[kThreads];
    double sum = 0.0;
    for (int t0 = 0; t0 < n_tiles; t0 += kThreads) {
        const int n = min(kThreads, n_tiles - t0);
        if ((int)threadIdx.x < n) part[threadIdx.x] = P[t0 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < n; i++) sum += part[i];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(sum / ((double)N * (double)NL));
}

// one wave per job: (layer, 64 x 64 tile of its gradient, batch slice) of the chains [c0, c1), or a slice of grad_std's column sums.  A
// chain's `in` is what its first layer read: the stored concatenation for an actor behind an encoder.
__device__ __forceinline__ void wgrad_job(const PArgs &a, const TChain *ch, int c0, int c1) {
    const int job = blockIdx.x;
    if (job >= a.std_job0) {
        colsum_wave(a.grad_sigma, a.grad_sigma_stride, a.A, a.ws + a.std_p_off, job - a.std_job0, a.std_rps, a.N);
        return;
    }
    int ci = c0, li = 0;
    for (int c = c0; c < c1; c++)
        for (int l = 0; l < ch[c].n_layers; l++)
            if (job >= ch[c].l[l].job0) { ci = c; li = l; }          // job0 rises with (c, l)
    const TChain &c = ch[ci];
    const TLayer &L = c.l[li];
    wgrad_wave(L, a.ws + L.g_off, li ? a.ws + c.l[li - 1].h_off : c.in, li ? L.K : c.in_stride, a.ws, job - L.job0, a.N);
}

// every element of every gradient of the chains [c0, c1), and of grad_std where the pass has one: its partials in slice order
__device__ __forceinline__ void combine_all(const PArgs &a, const TChain *ch, int c0, int c1) {
    const long long stride = (long long)gridDim.x * blockDim.x, first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (int ci = c0; ci < c1; ci++)
        for (int li = 0; li < ch[ci].n_layers; li++) combine_layer(ch[ci].l[li], a.ws, first, stride);
    if (a.std_S) combine_cols(a.ws + a.std_p_off, a.A, a.std_S, a.grad_std, first, stride);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
template <class P> static int check_desc(const std::string &f, const P *p) {
    if (!p) return lg_fail_msg(f + ": null descriptor");
    if (p->n_rows < 1) return lg_fail_msg(f + ": n_rows = " + std::to_string(p->n_rows) + " < 1");
    return 0;
}

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

// what plan_layout decides besides the members of PArgs and TLayer; an offset the pass has no region for is -1
struct PassLayout {
    int lds_bytes;
    long long gl_off, y_off, part_off, workspace_floats;
};

// the workspace behind `off`, the slices and the jobs of the chains [c0, c1) of `ch`, the std slab (act: the chain whose last width is A;
// -1: the pass has no std), the row tile, and for a loss pass (extra_lds: the bytes of its float64 tree) gl, the targets where `y_region`
// and the float64 tile partials
static int plan_layout(const std::string &f, PArgs &k, TChain *ch, int N, int c0, int c1, int act, int target_jobs, const int w[2], int extra_lds, bool y_region,
                       long long off, PassLayout &lay) {
    int jobs = 0;
    for (int ci = c0; ci < c1; ci++)
        for (int li = 0; li < ch[ci].n_layers; li++) {
            TLayer &L = ch[ci].l[li];
            if (li < ch[ci].n_layers - 1) { L.h_off = off; off += (long long)N * L.M; }
            L.g_off = off; off += (long long)N * L.M;
        }
    for (int ci = c0; ci < c1; ci++)
        for (int li = 0; li < ch[ci].n_layers; li++) {
            TLayer &L = ch[ci].l[li];
            const int tn = (L.M + LG_TRAIN_WG_TILE - 1) / LG_TRAIN_WG_TILE;
            L.tiles_k = (L.K + LG_TRAIN_WG_TILE - 1) / LG_TRAIN_WG_TILE;
            slice_rule(N, (long long)tn * L.tiles_k, L.S, L.rps, target_jobs);
            L.p_off = off; off += (long long)L.S * ((long long)L.M * L.K + L.M);
            L.job0 = jobs; jobs += L.S * tn * L.tiles_k;
        }
    if (act >= 0) {
        k.A = ch[act].l[ch[act].n_layers - 1].M;
        slice_rule(N, 1, k.std_S, k.std_rps, target_jobs);
        k.std_p_off = off; off += (long long)k.std_S * k.A;
    }
    k.std_job0 = jobs; jobs += k.std_S;
    k.n_jobs = jobs;
    k.N = N; k.c0 = c0; k.c1 = c1;
    lay.gl_off = lay.y_off = lay.part_off = -1;
    for (int R = 32; R >= 8; R >>= 1) {
        const size_t bytes = (size_t)R * (w[0] + w[1]) * sizeof(float) + extra_lds;
        if (bytes > kLdsBytes) continue;
        k.R = R; k.q_off = R * w[0]; k.red_off = R * (w[0] + w[1]); lay.lds_bytes = (int)bytes;
        k.n_tiles = (N + R - 1) / R;
        if (extra_lds) {
            const long long NL = ch[c0].l[ch[c0].n_layers - 1].M;
            lay.gl_off = off; off += N * NL;
            if (y_region) { lay.y_off = off; off += N * NL; }
            off += off & 1;
            lay.part_off = off; off += 2LL * k.n_tiles;
        }
        lay.workspace_floats = off;
        return 0;
    }
    return lg_fail_msg(f + ": an 8-row tile of these widths (" + std::to_string(w[0] + w[1]) + " floats per row) does not fit the 160 KB of LDS");
}

// the members every public plan struct has, from what plan_layout left in k, the chains and lay
template <class Plan, int NC> static void plan_out(Plan &pl, const PArgs &k, const TChain (&ch)[NC], const PassLayout &lay) {
    for (int ci = 0; ci < NC; ci++)
        for (int li = 0; li < LG_POLICY_MAX_LAYERS; li++) pl.h_off[ci][li] = pl.g_off[ci][li] = pl.p_off[ci][li] = -1;
    for (int ci = k.c0; ci < k.c1; ci++)
        for (int li = 0; li < ch[ci].n_layers; li++) {
            const TLayer &L = ch[ci].l[li];
            if (li < ch[ci].n_layers - 1) pl.h_off[ci][li] = L.h_off;
            pl.g_off[ci][li] = L.g_off; pl.p_off[ci][li] = L.p_off;
            pl.slices[ci][li] = L.S; pl.slice_rows[ci][li] = L.rps;
        }
    pl.row_tile = k.R; pl.lds_bytes = lay.lds_bytes;
    pl.std_slices = k.std_S; pl.std_slice_rows = k.std_rps; pl.std_p_off = k.std_S ? k.std_p_off : -1;
    pl.weight_jobs = k.n_jobs;
    pl.workspace_floats = lay.workspace_floats;
}

// pointers of one chain; in_width: the columns its input must have, 0: the chain has no input of its own.  grads: the chain is part of
// this backward; the gradient pointers of any other chain, and of every chain in a forward, are not even copied
static int bind_chain(const std::string &cn, const LgTrainChain &c, TChain &t, int in_width, bool grads) {
    if (in_width) {
        if (!c.input) return lg_fail_msg(cn + ".input is null");
        if (c.in_stride < in_width) return lg_fail_msg(cn + ".in_stride = " + std::to_string(c.in_stride) + " is below its width " + std::to_string(in_width));
        t.in = c.input; t.in_stride = c.in_stride;
    }
    for (int li = 0; li < c.n_layers; li++) {
        const LgTrainLayer &l = c.layer[li];
        const std::string ln = cn + ".layer[" + std::to_string(li) + "]";
        if (!l.weight) return lg_fail_msg(ln + ".weight is null");
        if (!l.bias) return lg_fail_msg(ln + ".bias is null");
        if (grads && !l.grad_weight) return lg_fail_msg(ln + ".grad_weight is null");
        if (grads && !l.grad_bias) return lg_fail_msg(ln + ".grad_bias is null");
        TLayer &L = t.l[li];
        L.W = l.weight; L.b = l.bias;
        L.gW = grads ? l.grad_weight : nullptr; L.gb = grads ? l.grad_bias : nullptr;
    }
    return 0;
}

static int check_ws(const std::string &f, const float *ws, long long cap, long long need, bool align8) {
    if (!ws) return lg_fail_msg(f + ": workspace is null");
    if (align8 && ((uintptr_t)ws & 7)) return lg_fail_msg(f + ": workspace is not 8-byte aligned (it holds the float64 partials)");
    if (cap < need) return lg_fail_msg(f + ": workspace_capacity = " + std::to_string(cap) + " floats is below the plan's " + std::to_string(need));
    return 0;
}

// the heads of an RL pass (P: LgTrainArgs, LgTrainEEArgs or LgTrainTSArgs) into k and its actor and critic chains, and the workspace
template <class P> static int bind_heads(const std::string &f, const P *p, PArgs &k, TChain &act, TChain &cri, long long need, bool backward) {
    const int A = k.A, V = cri.l[cri.n_layers - 1].M;
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
    if (check_ws(f, p->workspace, p->workspace_capacity, need, false)) return 1;
    act.out = p->mu; act.out_stride = p->mu_stride;
    cri.out = p->values; cri.out_stride = p->values_stride;
    act.gin = p->grad_mu; act.gin_stride = p->grad_mu_stride;
    cri.gin = p->grad_values; cri.gin_stride = p->grad_values_stride;
    k.ws = p->workspace; k.std = p->std; k.grad_std = p->grad_std; k.sigma = p->sigma; k.sigma_stride = p->sigma_stride;
    k.grad_sigma = p->grad_sigma; k.grad_sigma_stride = p->grad_sigma_stride;
    k.clip_on = p->clip_on != 0; k.clip = p->clip_actions;
    return 0;
}

static int done(const char *fn) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : lg_fail_msg(std::string(fn) + ": " + hipGetErrorString(e));
}

// once per device and kernel (`raised`: that kernel's flags): dynamic LDS above 64 KB has to be asked for (an unsynchronised race sets
// the same value twice: harmless)
static int raise_lds(const char *fn, const void *kernel, bool (&raised)[64]) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return lg_fail_msg(std::string(fn) + ": no current HIP device");
    if (raised[dev]) return 0;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (e != hipSuccess) return lg_fail_msg(std::string(fn) + ": hipFuncSetAttribute: " + hipGetErrorString(e));
    raised[dev] = true;
    return 0;
}

// a row-tile kernel over grid (row tiles, grid_y): kern[1] where the tile has 32 rows (RB = 2), kern[0] below; its LDS raised first
template <class K> static int launch_tile(const char *fn, void (*const (&kern)[2])(K), bool (&raised)[2][64], int grid_y, int lds_bytes, hipStream_t stream, const K &k) {
    const int rb = k.R == 32;
    if (raise_lds(fn, (const void *)kern[rb], raised[rb])) return 1;
    hipLaunchKernelGGL(kern[rb], dim3((unsigned)k.n_tiles, (unsigned)grid_y), dim3(kThreads), (size_t)lds_bytes, stream, k);
    return 0;
}

// the three launches of a backward over the chains [c0, c1) of k
template <class K> static int launch_backward(const char *fn, void (*const (&input_grad)[2])(K), bool (&raised)[2][64], void (*weight_grad)(K), void (*combine)(K), int grid_y,
                                              int lds_bytes, hipStream_t stream, const K &k) {
    if (launch_tile(fn, input_grad, raised, grid_y, lds_bytes, stream, k)) return 1;
    hipLaunchKernelGGL(weight_grad, dim3((unsigned)k.n_jobs), dim3(64), 0, stream, k);
    long long elems = k.A;
    for (int ci = k.c0; ci < k.c1; ci++)
        for (int li = 0; li < k.c[ci].n_layers; li++) {
            const long long n = (long long)k.c[ci].l[li].M * k.c[ci].l[li].K + k.c[ci].l[li].M;
            if (n > elems) elems = n;
        }
    long long blocks = (elems + 255) / 256;
    if (blocks > 1024) blocks = 1024;                    // grid-stride behind that
    hipLaunchKernelGGL(combine, dim3((unsigned)blocks), dim3(256), 0, stream, k);
    return done(fn);
}
#endif /* LG_TRAIN_PASS_H */

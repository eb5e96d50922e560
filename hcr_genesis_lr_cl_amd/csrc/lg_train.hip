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
#include <string>
#include "lg_train_tiles.h"   // the layer routines, shared with lg_train_ee.hip

int lg_fail_msg(const std::string &m);   // lg_host.hip: sets the thread-local message, returns 1

struct TArgs {
    TChain c[LG_TRAIN_CHAINS];
    float *ws;
    const float *std, *grad_sigma;
    float *grad_std, *sigma;
    int N, R, q_off, A, clip_on;
    float clip;
    int sigma_stride, grad_sigma_stride;
    int std_S, std_rps, std_job0, n_jobs;
    long long std_p_off;
};
static_assert(sizeof(TArgs) <= 4096, "TArgs is passed by value: the kernel-argument segment is 4 KB");

template <int RB> __global__ __launch_bounds__(256) void train_forward_kernel(TArgs a) {
    extern __shared__ __align__(16) float lds[];
    const TChain &c = a.c[blockIdx.y];
    const int R = a.R, row0 = blockIdx.x * R;
    const int rows = min(R, a.N - row0);
    lds_f *buf[2] = {(lds_f *)lds, (lds_f *)lds + a.q_off};
    stage_rows(c.in, c.l[0].K, c.in_stride, buf[0], c.l[0].sa, R, rows, row0);
    __syncthreads();
    for (int li = 0; li < c.n_layers; li++) {
        const TLayer &L = c.l[li];
        const bool last = li == c.n_layers - 1;
        const bool clip_on = last && blockIdx.y == LG_TRAIN_ACTOR && a.clip_on;
        const int per_wave = (((L.M + 15) >> 4) + kWaves - 1) / kWaves;
        // the activation the layer before left goes to the workspace while this layer reads it
        if (li) copy_out(buf[li & 1], L.sa, a.ws + c.l[li - 1].h_off, L.K, L.K, rows, row0);
        if (per_wave >= 4) fwd_tile<RB, 4>(L, buf[li & 1], buf[(li + 1) & 1], clip_on, a.clip, R);
        else if (per_wave >= 2) fwd_tile<RB, 2>(L, buf[li & 1], buf[(li + 1) & 1], clip_on, a.clip, R);
        else fwd_tile<RB, 1>(L, buf[li & 1], buf[(li + 1) & 1], clip_on, a.clip, R);
        __syncthreads();
    }
    const lds_f *m = buf[c.n_layers & 1];
    const int sm = c.l[c.n_layers - 1].so;
    copy_out(m, sm, c.out, c.l[c.n_layers - 1].M, c.out_stride, rows, row0);
    if (blockIdx.y != LG_TRAIN_ACTOR) return;
    const int A = a.A;
    for (int t = threadIdx.x; t < rows * A; t += kThreads) {
        const int row = t / A, ai = t - row * A;
        a.sigma[(size_t)(row0 + row) * a.sigma_stride + ai] = m[row * sm + ai] * 0.f + a.std[ai];
    }
}

template <int RB> __global__ __launch_bounds__(256) void train_input_grad_kernel(TArgs a) {
    extern __shared__ __align__(16) float lds[];
    const TChain &c = a.c[blockIdx.y];
    const int R = a.R, row0 = blockIdx.x * R, nl = c.n_layers;
    const int rows = min(R, a.N - row0);
    lds_f *buf[2] = {(lds_f *)lds, (lds_f *)lds + a.q_off};
    {   // G of the last layer: the incoming gradient, behind the Hardtanh's mask for the actor; rows behind `rows` are zero
        const TLayer &L = c.l[nl - 1];
        lds_f *g = buf[nl & 1];
        float *gws = a.ws + L.g_off;
        const bool mask = blockIdx.y == LG_TRAIN_ACTOR && a.clip_on;
        const int w = L.M;
        for (int i = threadIdx.x; i < R * w; i += kThreads) {
            const int row = i / w, col = i - row * w;
            float v = 0.f;
            if (row < rows) {
                v = c.gin[(size_t)(row0 + row) * c.gin_stride + col];
                if (mask) {
                    const float m = c.out[(size_t)(row0 + row) * c.out_stride + col];
                    if (m >= a.clip || m <= -a.clip) v = 0.f;                 // hardtanh_backward: a NaN mean passes the gradient on
                }
                gws[(size_t)(row0 + row) * w + col] = v;
            }
            g[row * L.so + col] = v;
        }
    }
    __syncthreads();
    for (int li = nl - 1; li >= 1; li--) {
        const TLayer &L = c.l[li], &P = c.l[li - 1];
        lds_f *cur = buf[(li + 1) & 1], *nxt = buf[li & 1];
        if (P.elu) {                                                   // H_(l-1) into the destination tile: the epilogue turns it into G_(l-1) in place
            stage_rows(a.ws + P.h_off, L.K, L.K, nxt, L.sa, R, rows, row0);
            __syncthreads();
        }
        const int per_wave = (((L.K + 15) >> 4) + kWaves - 1) / kWaves;
        if (per_wave >= 4) bwd_tile<RB, 4>(L, cur, nxt, P.elu != 0, R);
        else if (per_wave >= 2) bwd_tile<RB, 2>(L, cur, nxt, P.elu != 0, R);
        else bwd_tile<RB, 1>(L, cur, nxt, P.elu != 0, R);
        __syncthreads();
        // G_(l-1) to the workspace: `nxt` is read only (by this and by the next layer) until the barrier after the next layer's
        // stage, and `cur` is not written before that barrier either
        copy_out(nxt, L.sa, a.ws + P.g_off, L.K, L.K, rows, row0);
    }
}

// one wave per job: (layer, 64 x 64 tile of its gradient, batch slice), or a slice of grad_std's column sums
__global__ __launch_bounds__(64) void train_weight_grad_kernel(TArgs a) {
    const int job = blockIdx.x;
    if (job >= a.std_job0) {
        colsum_wave(a.grad_sigma, a.grad_sigma_stride, a.A, a.ws + a.std_p_off, job - a.std_job0, a.std_rps, a.N);
        return;
    }
    int ci = 0, li = 0;
    for (int c = 0; c < LG_TRAIN_CHAINS; c++)
        for (int l = 0; l < a.c[c].n_layers; l++)
            if (job >= a.c[c].l[l].job0) { ci = c; li = l; }          // job0 rises with (c, l)
    const TChain &c = a.c[ci];
    const TLayer &L = c.l[li];
    wgrad_wave(L, a.ws + L.g_off, li ? a.ws + c.l[li - 1].h_off : c.in, li ? L.K : c.in_stride, a.ws, job - L.job0, a.N);
}

// every element of every gradient: its partials in slice order
__global__ __launch_bounds__(256) void train_combine_kernel(TArgs a) {
    const long long stride = (long long)gridDim.x * blockDim.x, first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (int ci = 0; ci < LG_TRAIN_CHAINS; ci++)
        for (int li = 0; li < a.c[ci].n_layers; li++) combine_layer(a.c[ci].l[li], a.ws, first, stride);
    combine_cols(a.ws + a.std_p_off, a.A, a.std_S, a.grad_std, first, stride);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static const char *kChain[LG_TRAIN_CHAINS] = {"chain[0] (actor)", "chain[1] (critic)"};

// the plan from the shapes alone; fills the shape part of `k` too
static int make_plan(const char *fn, const LgTrainArgs *p, LgTrainPlan &pl, TArgs &k) {
    const std::string f(fn);
    if (!p) return lg_fail_msg(f + ": null descriptor");
    if (p->n_rows < 1) return lg_fail_msg(f + ": n_rows = " + std::to_string(p->n_rows) + " < 1");
    pl = LgTrainPlan{};
    k = TArgs{};
    const int N = p->n_rows;
    int w[2] = {0, 0};
    long long off = 0;
    for (int ci = 0; ci < LG_TRAIN_CHAINS; ci++) {
        const LgTrainChain &c = p->chain[ci];
        const std::string cn = f + ": " + kChain[ci];
        if (c.n_layers < 1 || c.n_layers > kMaxL) return lg_fail_msg(cn + ".n_layers = " + std::to_string(c.n_layers) + " is outside [1, " + std::to_string(kMaxL) + "]");
        int width = c.layer[0].n_in;
        for (int li = 0; li < c.n_layers; li++) {
            const LgTrainLayer &l = c.layer[li];
            const std::string ln = cn + ".layer[" + std::to_string(li) + "]";
            if (l.n_in < 1 || l.n_in > LG_POLICY_MAX_WIDTH) return lg_fail_msg(ln + ".n_in = " + std::to_string(l.n_in) + " is outside [1, " + std::to_string(LG_POLICY_MAX_WIDTH) + "]");
            if (l.n_out < 1 || l.n_out > LG_POLICY_MAX_WIDTH) return lg_fail_msg(ln + ".n_out = " + std::to_string(l.n_out) + " is outside [1, " + std::to_string(LG_POLICY_MAX_WIDTH) + "]");
            if (l.n_in != width) return lg_fail_msg(ln + ".n_in = " + std::to_string(l.n_in) + ", but its input has " + std::to_string(width) + " columns");
            width = l.n_out;
            TLayer &L = k.c[ci].l[li];
            L.K = l.n_in; L.M = l.n_out; L.elu = l.elu != 0;
            L.sa = lds_stride(l.n_in); L.so = lds_stride(l.n_out);
            if (L.sa > w[li & 1]) w[li & 1] = L.sa;
            if (L.so > w[(li + 1) & 1]) w[(li + 1) & 1] = L.so;
        }
        k.c[ci].n_layers = c.n_layers;
    }
    int jobs = 0;
    for (int ci = 0; ci < LG_TRAIN_CHAINS; ci++)
        for (int li = 0; li < LG_POLICY_MAX_LAYERS; li++) pl.h_off[ci][li] = pl.g_off[ci][li] = pl.p_off[ci][li] = -1;
    for (int ci = 0; ci < LG_TRAIN_CHAINS; ci++)
        for (int li = 0; li < k.c[ci].n_layers; li++) {
            TLayer &L = k.c[ci].l[li];
            if (li < k.c[ci].n_layers - 1) { L.h_off = pl.h_off[ci][li] = off; off += (long long)N * L.M; }
            L.g_off = pl.g_off[ci][li] = off; off += (long long)N * L.M;
        }
    for (int ci = 0; ci < LG_TRAIN_CHAINS; ci++)
        for (int li = 0; li < k.c[ci].n_layers; li++) {
            TLayer &L = k.c[ci].l[li];
            const int tn = (L.M + LG_TRAIN_WG_TILE - 1) / LG_TRAIN_WG_TILE;
            L.tiles_k = (L.K + LG_TRAIN_WG_TILE - 1) / LG_TRAIN_WG_TILE;
            slice_rule(N, (long long)tn * L.tiles_k, L.S, L.rps);
            pl.slices[ci][li] = L.S; pl.slice_rows[ci][li] = L.rps;
            L.p_off = pl.p_off[ci][li] = off; off += (long long)L.S * ((long long)L.M * L.K + L.M);
            L.job0 = jobs; jobs += L.S * tn * L.tiles_k;
        }
    const int na = k.c[LG_TRAIN_ACTOR].n_layers;
    k.A = k.c[LG_TRAIN_ACTOR].l[na - 1].M;
    slice_rule(N, 1, k.std_S, k.std_rps);
    pl.std_slices = k.std_S; pl.std_slice_rows = k.std_rps;
    k.std_p_off = pl.std_p_off = off; off += (long long)k.std_S * k.A;
    k.std_job0 = jobs; jobs += k.std_S;
    k.n_jobs = pl.weight_jobs = jobs;
    pl.workspace_floats = off;
    k.N = N;
    for (int R = 32; R >= 8; R >>= 1) {
        const size_t bytes = (size_t)R * (w[0] + w[1]) * sizeof(float);
        if (bytes <= kLdsBytes) {
            k.R = pl.row_tile = R; k.q_off = R * w[0]; pl.lds_bytes = (int)bytes;
            return 0;
        }
    }
    return lg_fail_msg(f + ": an 8-row tile of these widths (" + std::to_string(w[0] + w[1]) + " floats per row) does not fit the 160 KB of LDS");
}

// the pointers and strides; `backward`: the gradient members too
static int bind(const char *fn, const LgTrainArgs *p, const LgTrainPlan &pl, TArgs &k, bool backward) {
    const std::string f(fn);
    for (int ci = 0; ci < LG_TRAIN_CHAINS; ci++) {
        const LgTrainChain &c = p->chain[ci];
        const std::string cn = f + ": " + kChain[ci];
        if (!c.input) return lg_fail_msg(cn + ".input is null");
        if (c.in_stride < c.layer[0].n_in) return lg_fail_msg(cn + ".in_stride = " + std::to_string(c.in_stride) + " is below its width " + std::to_string(c.layer[0].n_in));
        k.c[ci].in = c.input; k.c[ci].in_stride = c.in_stride;
        for (int li = 0; li < c.n_layers; li++) {
            const LgTrainLayer &l = c.layer[li];
            const std::string ln = cn + ".layer[" + std::to_string(li) + "]";
            if (!l.weight) return lg_fail_msg(ln + ".weight is null");
            if (!l.bias) return lg_fail_msg(ln + ".bias is null");
            if (backward && !l.grad_weight) return lg_fail_msg(ln + ".grad_weight is null");
            if (backward && !l.grad_bias) return lg_fail_msg(ln + ".grad_bias is null");
            TLayer &L = k.c[ci].l[li];
            L.W = l.weight; L.b = l.bias; L.gW = l.grad_weight; L.gb = l.grad_bias;
        }
    }
    const int A = k.A, V = k.c[LG_TRAIN_CRITIC].l[k.c[LG_TRAIN_CRITIC].n_layers - 1].M;
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
    if (!p->workspace) return lg_fail_msg(f + ": workspace is null");
    if (p->workspace_capacity < pl.workspace_floats)
        return lg_fail_msg(f + ": workspace_capacity = " + std::to_string((long long)p->workspace_capacity) + " floats is below the plan's " + std::to_string((long long)pl.workspace_floats));
    k.c[LG_TRAIN_ACTOR].out = p->mu; k.c[LG_TRAIN_ACTOR].out_stride = p->mu_stride;
    k.c[LG_TRAIN_CRITIC].out = p->values; k.c[LG_TRAIN_CRITIC].out_stride = p->values_stride;
    k.c[LG_TRAIN_ACTOR].gin = p->grad_mu; k.c[LG_TRAIN_ACTOR].gin_stride = p->grad_mu_stride;
    k.c[LG_TRAIN_CRITIC].gin = p->grad_values; k.c[LG_TRAIN_CRITIC].gin_stride = p->grad_values_stride;
    k.ws = p->workspace; k.std = p->std; k.grad_std = p->grad_std; k.sigma = p->sigma; k.sigma_stride = p->sigma_stride;
    k.grad_sigma = p->grad_sigma; k.grad_sigma_stride = p->grad_sigma_stride;
    k.clip_on = p->clip_on != 0; k.clip = p->clip_actions;
    return 0;
}

extern "C" int lg_train_plan(const LgTrainArgs *args, LgTrainPlan *out) {
    if (!out) return lg_fail_msg("lg_train_plan: null plan");
    TArgs k;
    return make_plan("lg_train_plan", args, *out, k);
}

// once per device and kernel: dynamic LDS above 64 KB has to be asked for (an unsynchronised race sets the same value twice: harmless)
static int raise_lds(const char *fn, int which, int rb) {
    static bool raised[64][2][2];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return lg_fail_msg(std::string(fn) + ": no current HIP device");
    if (raised[dev][which][rb]) return 0;
    const void *fp = which ? (rb ? (const void *)train_input_grad_kernel<2> : (const void *)train_input_grad_kernel<1>)
                           : (rb ? (const void *)train_forward_kernel<2> : (const void *)train_forward_kernel<1>);
    const hipError_t e = hipFuncSetAttribute(fp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
    if (e != hipSuccess) return lg_fail_msg(std::string(fn) + ": hipFuncSetAttribute: " + hipGetErrorString(e));
    raised[dev][which][rb] = true;
    return 0;
}

extern "C" int lg_train_forward(const LgTrainArgs *args, void *stream) {
    static const char *fn = "lg_train_forward";
    LgTrainPlan pl; TArgs k;
    if (make_plan(fn, args, pl, k) || bind(fn, args, pl, k, false)) return 1;
    const int rb = k.R == 32;
    if (raise_lds(fn, 0, rb)) return 1;
    const dim3 grid((unsigned)((k.N + k.R - 1) / k.R), LG_TRAIN_CHAINS);
    if (rb) hipLaunchKernelGGL(train_forward_kernel<2>, grid, dim3(kThreads), (size_t)pl.lds_bytes, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(train_forward_kernel<1>, grid, dim3(kThreads), (size_t)pl.lds_bytes, (hipStream_t)stream, k);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : lg_fail_msg(std::string(fn) + ": " + hipGetErrorString(e));
}

extern "C" int lg_train_backward(const LgTrainArgs *args, void *stream) {
    static const char *fn = "lg_train_backward";
    LgTrainPlan pl; TArgs k;
    if (make_plan(fn, args, pl, k) || bind(fn, args, pl, k, true)) return 1;
    const int rb = k.R == 32;
    if (raise_lds(fn, 1, rb)) return 1;
    const dim3 grid((unsigned)((k.N + k.R - 1) / k.R), LG_TRAIN_CHAINS);
    if (rb) hipLaunchKernelGGL(train_input_grad_kernel<2>, grid, dim3(kThreads), (size_t)pl.lds_bytes, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(train_input_grad_kernel<1>, grid, dim3(kThreads), (size_t)pl.lds_bytes, (hipStream_t)stream, k);
    hipLaunchKernelGGL(train_weight_grad_kernel, dim3((unsigned)k.n_jobs), dim3(64), 0, (hipStream_t)stream, k);
    long long elems = k.A;
    for (int ci = 0; ci < LG_TRAIN_CHAINS; ci++)
        for (int li = 0; li < k.c[ci].n_layers; li++) {
            const long long n = (long long)k.c[ci].l[li].M * k.c[ci].l[li].K + k.c[ci].l[li].M;
            if (n > elems) elems = n;
        }
    long long blocks = (elems + 255) / 256;
    if (blocks > 1024) blocks = 1024;                    // grid-stride behind that
    hipLaunchKernelGGL(train_combine_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, k);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : lg_fail_msg(std::string(fn) + ": " + hipGetErrorString(e));
}

// lg_train_tcn.hip -- the supervised history-encoder pass of the teacher-student family behind include/lgtraintcn.h where the history
// encoder is a "TCN": a stack of strided, dilated nn.Conv1d (no activation between them), nn.Flatten, and a Linear / ELU tail, against
// the privilege encoder's output as a constant target (masked mean-squared error), with the backward over the tail and the convs.
//
// Reference call sites replaced: rsl_rl/algorithms/ppo_ts.py:174-187 (_compute_encoder_loss, its TCN branch) and the share of
// encoder_loss.backward() (ppo_ts.py:126-133) that runs through rsl_rl/modules/actor_critic_ts.py:61-99.
//
// The tail and the target are lg_train_ts.hip's encoder pass on the routines of lg_train_pass.h / lg_train_tiles.h, used as they are: the
// tail's input is bound to the dense f region the conv stack left in the workspace, and its input-gradient launch goes one layer further,
// through tail layer 0 (no ELU factor), into G_f.  What is this unit's own is the convolution.  At the reference's shapes it is traffic,
// not FLOPs (channels 1-1-1-1, five taps: about 20 kFLOP and 20 KB per row), and the widest layer the header admits has a 32 x 32 x 9
// weight on at most 2048 / 32 = 64 output positions per channel at the flatten: too short a GEMM to fill MFMA tiles per row, and an
// implicit GEMM over (row, t) would need the gather in LDS first.  So the three conv kernels are plain VALU code.  Their sums run in float64
// and are rounded to float32 once per stored element: a conv's bias gradient adds n_rows * L elements of G, so the independent roundings of
// a float32 accumulation in every layer above it would add up in it; the FLOPs are few enough for the float64 rate not to show.
//   conv forward        a workgroup owns a block of consecutive rows and carries them layer by layer; one layer's weights and bias sit in
//                       LDS (at most 32 * 32 * 9 + 32 floats = 36 KB), a lane owns output elements (o, t) of a row, consecutive lanes
//                       consecutive t: the loads of x and the store of y are runs.  x_l goes to the workspace (the weight gradient
//                       needs it) and is read back, behind a barrier, by the workgroup that wrote it.
//   conv input gradient the same blocks from the last conv down to the second, in gather form: a lane owns (i, u) of G_(l-1) and adds, tap
//                       after tap and output channel after output channel, the W[o][i][k] G_l[o][t] with t * stride + k * dilation -
//                       padding = u.  A position no output reads gets exactly 0.  No scatter: every element has one writer.
//   conv weight gradient a workgroup owns 8 gradient elements (o, i, k) or bias elements of one batch slice, 32 lanes each: lane j adds
//                       the positions t = j, j + 32, ... of a row into a float32 row partial, the row partials in row order in float64,
//                       and the 32 lane sums meet in a fixed binary tree in LDS, rounded to float32 once.  Taps in the padding contribute 0.
//   combine             every element of every gradient: its slice partials in slice order.
// Plain stores only; two calls on the same inputs give the same bits.
#include "lg_train_pass.h"
#include "../../include/lgtraintcn.h"

#define TAIL 0
#define PRI 1
static const int kRedBytes = LG_TRAIN_TCN_THREADS * (int)sizeof(double);
static const int kMaxW = LG_TRAIN_TCN_MAX_CHANNELS * LG_TRAIN_TCN_MAX_CHANNELS * LG_TRAIN_TCN_MAX_KERNEL;
static const int kLanes = LG_TRAIN_TCN_THREADS / LG_TRAIN_TCN_WG_ELEMS;      // per gradient element
static_assert(LG_TRAIN_TCN_THREADS == kThreads, "the loss tree has one leaf per thread of the row-tile workgroup");
static_assert(kLanes == 32, "the weight-gradient tree below starts at 16");

struct KConv {
    const float *W, *b;
    float *gW, *gb;
    int ci, co, K, s, p, d, Lin, Lout;
    int S, rps, job0, E;
    long long x_in, x_out, g_in, g_out, p_off;      // x_(l), x_(l+1), G_(l), G_(l+1) of zero-based layer l; x_in / g_in of layer 0: -1
};

struct NArgs : PArgs {
    TChain c[2];                // TAIL, PRI
    KConv v[LG_TRAIN_TCN_MAX_CONV];
    const float *hist, *mask, *upstream;
    float *loss;
    int hist_stride, mask_stride, n_conv, block_rows, conv_jobs, conv_blocks;
    long long gl_off, y_off, part_off;
};
static_assert(sizeof(NArgs) <= 4096, "NArgs is passed by value: the kernel-argument segment is 4 KB");

__device__ __forceinline__ const float *conv_input(const NArgs &a, const KConv &v, int l, int row) {
    return l ? a.ws + v.x_in + (size_t)row * (v.ci * v.Lin) : a.hist + (size_t)row * a.hist_stride;
}

// one layer's weights and bias into LDS; a barrier on both sides: the layer before has been read, and its rows in the workspace written
__device__ __forceinline__ void stage_conv(const KConv &v, float *w) {
    __syncthreads();
    const int nw = v.co * v.ci * v.K;
    for (int i = threadIdx.x; i < nw; i += kThreads) w[i] = v.W[i];
    for (int i = threadIdx.x; i < v.co; i += kThreads) w[kMaxW + i] = v.b[i];
    __syncthreads();
}

__global__ __launch_bounds__(256) void train_tcn_conv_forward_kernel(NArgs a) {
    __shared__ float w[kMaxW + LG_TRAIN_TCN_MAX_CHANNELS];
    const int r0 = blockIdx.x * a.block_rows, r1 = min(r0 + a.block_rows, a.N);
    for (int l = 0; l < a.n_conv; l++) {
        const KConv &v = a.v[l];
        stage_conv(v, w);
        const int no = v.co * v.Lout;
        for (int row = r0; row < r1; row++) {
            const float *x = conv_input(a, v, l, row);
            float *y = a.ws + v.x_out + (size_t)row * no;
            for (int e = threadIdx.x; e < no; e += kThreads) {
                const int o = e / v.Lout, t = e - o * v.Lout, base = t * v.s - v.p;
                double acc = 0.0;                                      // the taps add up in float64, rounded to float32 once
                for (int i = 0; i < v.ci; i++)
                    for (int k = 0; k < v.K; k++) {
                        const int u = base + k * v.d;
                        if (u >= 0 && u < v.Lin) acc += (double)w[(o * v.ci + i) * v.K + k] * (double)x[i * v.Lin + u];
                    }
                y[e] = (float)(acc + (double)w[kMaxW + o]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void train_tcn_conv_input_grad_kernel(NArgs a) {
    __shared__ float w[kMaxW + LG_TRAIN_TCN_MAX_CHANNELS];
    const int r0 = blockIdx.x * a.block_rows, r1 = min(r0 + a.block_rows, a.N);
    for (int l = a.n_conv - 1; l >= 1; l--) {
        const KConv &v = a.v[l];
        stage_conv(v, w);
        const int ni = v.ci * v.Lin, no = v.co * v.Lout;
        for (int row = r0; row < r1; row++) {
            const float *g = a.ws + v.g_out + (size_t)row * no;
            float *dx = a.ws + v.g_in + (size_t)row * ni;
            for (int e = threadIdx.x; e < ni; e += kThreads) {
                const int i = e / v.Lin, u = e - i * v.Lin;
                double acc = 0.0;
                for (int k = 0; k < v.K; k++) {
                    const int num = u + v.p - k * v.d;
                    if (num < 0) break;                                // falls with k
                    const int t = num / v.s;
                    if (t * v.s != num || t >= v.Lout) continue;
                    for (int o = 0; o < v.co; o++) acc += (double)w[(o * v.ci + i) * v.K + k] * (double)g[o * v.Lout + t];
                }
                dx[e] = (float)acc;
            }
        }
    }
}

__global__ __launch_bounds__(256) void train_tcn_conv_weight_grad_kernel(NArgs a) {
    __shared__ double red[kThreads];
    const int job = blockIdx.x;
    int l = 0;
    for (int i = 1; i < a.n_conv; i++)
        if (job >= a.v[i].job0) l = i;                                 // job0 rises with the layer
    const KConv &v = a.v[l];
    const int tiles = (v.E + LG_TRAIN_TCN_WG_ELEMS - 1) / LG_TRAIN_TCN_WG_ELEMS, rel = job - v.job0, s = rel / tiles, tb = rel - s * tiles;
    const int el = threadIdx.x / kLanes, j = threadIdx.x - el * kLanes;
    const int e = tb * LG_TRAIN_TCN_WG_ELEMS + el, ec = min(e, v.E - 1), nw = v.co * v.ci * v.K;
    const bool is_bias = ec >= nw;
    int o = ec - nw, i = 0, k = 0;
    if (!is_bias) {
        o = ec / (v.ci * v.K);
        const int rem = ec - o * v.ci * v.K;
        i = rem / v.K; k = rem - i * v.K;
    }
    const int rb = s * v.rps, re = min(rb + v.rps, a.N), shift = k * v.d - v.p, no = v.co * v.Lout;
    double acc = 0.0;                                                  // a row's partial is float32; the rows and the lanes add up in float64
    for (int row = rb; row < re; row++) {
        const float *g = a.ws + v.g_out + (size_t)row * no + o * v.Lout;
        const float *x = conv_input(a, v, l, row) + i * v.Lin;
        float part = 0.f;
        if (is_bias)
            for (int t = j; t < v.Lout; t += kLanes) part += g[t];
        else
            for (int t = j; t < v.Lout; t += kLanes) {
                const int u = t * v.s + shift;
                if (u >= 0 && u < v.Lin) part += g[t] * x[u];
            }
        acc += (double)part;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int st = kLanes / 2; st > 0; st >>= 1) {
        if (j < st) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + st];
        __syncthreads();
    }
    if (j == 0 && e < v.E) a.ws[v.p_off + (long long)s * v.E + e] = (float)red[threadIdx.x];
}

template <int RB> __global__ __launch_bounds__(256) void train_tcn_forward_kernel(NArgs a) {
    extern __shared__ __align__(16) float lds[];
    const TChain &e = a.c[PRI], &c = a.c[TAIL];
    const int R = a.R, row0 = blockIdx.x * R;
    const int rows = min(R, a.N - row0);
    lds_f *b0 = (lds_f *)lds, *b1 = (lds_f *)lds + a.q_off;
    const int Z = c.l[c.n_layers - 1].M;
    float *yw = a.ws + a.y_off;
    const lds_f *y = chain_from_rows<RB>(a.ws, e, b0, b1, false, false, a.clip, R, rows, row0);       // the target: nothing stored, no gradient
    copy_out(y, e.l[e.n_layers - 1].so, yw, Z, Z, rows, row0);                         // this tile's rows; read back below by this workgroup only
    __syncthreads();                                                                   // y has left the LDS before f is staged over it
    const lds_f *p = chain_from_rows<RB>(a.ws, c, b0, b1, true, false, a.clip, R, rows, row0);       // c.in is f
    mse_tile(p, c.l[c.n_layers - 1].so, Z, yw, Z, a.mask, a.mask_stride, a.ws + a.gl_off, 2.0f / ((float)a.N * (float)Z), (volatile double *)(lds + a.red_off),
             (double *)(a.ws + a.part_off), rows, row0);
}

__global__ __launch_bounds__(256) void train_tcn_finalize_kernel(NArgs a) {
    loss_finalize((const double *)(a.ws + a.part_off), a.n_tiles, a.N, a.c[TAIL].l[a.c[TAIL].n_layers - 1].M, a.loss);
}

// the tail's input gradients, then one layer further: through tail layer 0, with no ELU factor (f is no activation), into G_f
template <int RB> __global__ __launch_bounds__(256) void train_tcn_input_grad_kernel(NArgs a) {
    extern __shared__ __align__(16) float lds[];
    const TChain &c = a.c[TAIL];
    const int R = a.R, row0 = blockIdx.x * R;
    const int rows = min(R, a.N - row0);
    lds_f *b0 = (lds_f *)lds, *b1 = (lds_f *)lds + a.q_off;
    seed_last_g(a.ws, c, (c.n_layers & 1) ? b1 : b0, a.ws + a.gl_off, a.upstream, false, a.clip, R, rows, row0);
    __syncthreads();
    chain_backward<RB>(a.ws, c, b0, b1, R, rows, row0);               // G_0 sits in b1
    const TLayer &L0 = c.l[0];
    bwd_layer<RB>(L0, b1, b0, false, R);
    __syncthreads();
    copy_out(b0, L0.sa, a.ws + a.v[a.n_conv - 1].g_out, L0.K, L0.K, rows, row0);
}

__global__ __launch_bounds__(64) void train_tcn_weight_grad_kernel(NArgs a) { wgrad_job(a, a.c, TAIL, TAIL + 1); }

__global__ __launch_bounds__(256) void train_tcn_combine_kernel(NArgs a) {
    combine_all(a, a.c, TAIL, TAIL + 1);
    const long long stride = (long long)gridDim.x * blockDim.x, first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (int l = 0; l < a.n_conv; l++) {
        const KConv &v = a.v[l];
        const int nw = v.co * v.ci * v.K;
        const float *P = a.ws + v.p_off;
        for (long long e = first; e < v.E; e += stride) {
            float sum = P[e];
            for (int s = 1; s < v.S; s++) sum += P[(long long)s * v.E + e];
            if (e < nw) v.gW[e] = sum;
            else v.gb[e - nw] = sum;
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static void (*const kForward[2])(NArgs) = {train_tcn_forward_kernel<1>, train_tcn_forward_kernel<2>};
static void (*const kInputGrad[2])(NArgs) = {train_tcn_input_grad_kernel<1>, train_tcn_input_grad_kernel<2>};
static bool raised_forward[2][64], raised_input_grad[2][64];

static int outside(const std::string &what, int v, int lo, int hi) {
    return lg_fail_msg(what + " = " + std::to_string(v) + " is outside [" + std::to_string(lo) + ", " + std::to_string(hi) + "]");
}

static int make_plan(const char *fn, const LgTrainTcnArgs *p, LgTrainTcnPlan &pl, NArgs &k) {
    const std::string f(fn);
    if (check_desc(f, p)) return 1;
    pl = LgTrainTcnPlan{};
    k = NArgs{};
    const int N = p->n_rows, n = p->n_conv;
    if (n < 1 || n > LG_TRAIN_TCN_MAX_CONV) return outside(f + ": n_conv", n, 1, LG_TRAIN_TCN_MAX_CONV);
    if (p->n_history < 1 || p->n_history > LG_POLICY_MAX_WIDTH) return outside(f + ": n_history", p->n_history, 1, LG_POLICY_MAX_WIDTH);
    for (int l = 0; l <= LG_TRAIN_TCN_MAX_CONV; l++) pl.x_off[l] = pl.cg_off[l] = -1;
    for (int l = 0; l < LG_TRAIN_TCN_MAX_CONV; l++) pl.conv_p_off[l] = -1;
    pl.n_conv = k.n_conv = n;
    pl.length[0] = p->n_history;
    int chan = 1;
    for (int l = 0; l < n; l++) {
        const LgTrainConv &c = p->conv[l];
        const std::string cn = f + ": conv[" + std::to_string(l) + "]";
        if (c.c_in < 1 || c.c_in > LG_TRAIN_TCN_MAX_CHANNELS) return outside(cn + ".c_in", c.c_in, 1, LG_TRAIN_TCN_MAX_CHANNELS);
        if (c.c_out < 1 || c.c_out > LG_TRAIN_TCN_MAX_CHANNELS) return outside(cn + ".c_out", c.c_out, 1, LG_TRAIN_TCN_MAX_CHANNELS);
        if (c.c_in != chan)
            return lg_fail_msg(cn + ".c_in = " + std::to_string(c.c_in) + ", but its input has " + std::to_string(chan) + (l ? " channels" : " channel: obs_history is (1, H)"));
        if (c.kernel < 1 || c.kernel > LG_TRAIN_TCN_MAX_KERNEL) return outside(cn + ".kernel", c.kernel, 1, LG_TRAIN_TCN_MAX_KERNEL);
        if (c.stride < 1 || c.stride > LG_TRAIN_TCN_MAX_STRIDE) return outside(cn + ".stride", c.stride, 1, LG_TRAIN_TCN_MAX_STRIDE);
        if (c.dilation < 1 || c.dilation > LG_TRAIN_TCN_MAX_DILATION) return outside(cn + ".dilation", c.dilation, 1, LG_TRAIN_TCN_MAX_DILATION);
        if (c.padding < 0 || c.padding > c.dilation * (c.kernel - 1)) return outside(cn + ".padding", c.padding, 0, c.dilation * (c.kernel - 1));
        const int span = pl.length[l] + 2 * c.padding - c.dilation * (c.kernel - 1) - 1;
        if (span < 0)
            return lg_fail_msg(cn + ": its input of length " + std::to_string(pl.length[l]) + " is shorter than the window: the output length is below 1");
        pl.length[l + 1] = span / c.stride + 1;
        KConv &v = k.v[l];
        v.ci = c.c_in; v.co = c.c_out; v.K = c.kernel; v.s = c.stride; v.p = c.padding; v.d = c.dilation;
        v.Lin = pl.length[l]; v.Lout = pl.length[l + 1];
        v.E = v.co * v.ci * v.K + v.co;
        chan = c.c_out;
    }
    const int F = chan * pl.length[n];
    if (F > LG_POLICY_MAX_WIDTH)
        return lg_fail_msg(f + ": conv[" + std::to_string(n - 1) + "] leaves F = c_out * L = " + std::to_string(chan) + " * " + std::to_string(pl.length[n]) + " = " +
                           std::to_string(F) + " columns behind the flatten, above " + std::to_string(LG_POLICY_MAX_WIDTH) + ": the tail's first operand is a row tile in LDS");
    pl.flat = F;
    int w[2] = {0, 0};
    if (plan_chain(f + ": tail", p->tail, k.c[TAIL], 0, w) || plan_chain(f + ": privilege", p->privilege, k.c[PRI], 0, w)) return 1;
    if (k.c[TAIL].l[0].K != F)
        return lg_fail_msg(f + ": tail.layer[0].n_in = " + std::to_string(k.c[TAIL].l[0].K) + ", but the flattened conv output has " + std::to_string(chan) + " * " +
                           std::to_string(pl.length[n]) + " = " + std::to_string(F) + " columns");
    const int Zh = k.c[TAIL].l[k.c[TAIL].n_layers - 1].M, Zp = k.c[PRI].l[k.c[PRI].n_layers - 1].M;
    if (Zh != Zp)
        return lg_fail_msg(f + ": privilege.layer[" + std::to_string(k.c[PRI].n_layers - 1) + "].n_out = " + std::to_string(Zp) + ", but the history encoder ends at " +
                           std::to_string(Zh) + " columns: the two encoders' output widths differ");
    long long off = 0;
    for (int l = 1; l <= n; l++) { pl.x_off[l] = off; off += (long long)N * k.v[l - 1].co * pl.length[l]; }
    for (int l = 1; l <= n; l++) { pl.cg_off[l] = off; off += (long long)N * k.v[l - 1].co * pl.length[l]; }
    int jobs = 0;
    for (int l = 0; l < n; l++) {
        KConv &v = k.v[l];
        v.x_in = pl.x_off[l]; v.x_out = pl.x_off[l + 1]; v.g_in = pl.cg_off[l]; v.g_out = pl.cg_off[l + 1];
        const int tiles = (v.E + LG_TRAIN_TCN_WG_ELEMS - 1) / LG_TRAIN_TCN_WG_ELEMS;
        slice_rule(N, tiles, v.S, v.rps, LG_TRAIN_TCN_TARGET_JOBS);
        v.p_off = pl.conv_p_off[l] = off; off += (long long)v.S * v.E;
        v.job0 = pl.conv_job0[l] = jobs; jobs += v.S * tiles;
        pl.conv_slices[l] = v.S; pl.conv_slice_rows[l] = v.rps;
    }
    pl.conv_jobs = k.conv_jobs = jobs;
    const int blocks = N < LG_TRAIN_TCN_MAX_BLOCKS ? N : LG_TRAIN_TCN_MAX_BLOCKS;
    k.block_rows = pl.conv_block_rows = (N + blocks - 1) / blocks;
    k.conv_blocks = pl.conv_blocks = (N + k.block_rows - 1) / k.block_rows;
    PassLayout lay;
    if (plan_layout(f, k, k.c, N, TAIL, TAIL + 1, -1, LG_TRAIN_TCN_TARGET_JOBS, w, kRedBytes, true, off, lay)) return 1;
    for (int li = 0; li < LG_POLICY_MAX_LAYERS; li++) pl.h_off[li] = pl.g_off[li] = pl.p_off[li] = -1;
    for (int li = 0; li < k.c[TAIL].n_layers; li++) {
        const TLayer &L = k.c[TAIL].l[li];
        if (li < k.c[TAIL].n_layers - 1) pl.h_off[li] = L.h_off;
        pl.g_off[li] = L.g_off; pl.p_off[li] = L.p_off; pl.slices[li] = L.S; pl.slice_rows[li] = L.rps;
    }
    pl.row_tile = k.R; pl.lds_bytes = lay.lds_bytes; pl.weight_jobs = k.n_jobs; pl.loss_tiles = k.n_tiles;
    k.gl_off = pl.gl_off = lay.gl_off; k.y_off = pl.y_off = lay.y_off; k.part_off = pl.partial_off = lay.part_off;
    pl.workspace_floats = lay.workspace_floats;
    return 0;
}

static int bind(const char *fn, const LgTrainTcnArgs *p, const LgTrainTcnPlan &pl, NArgs &k, bool backward) {
    const std::string f(fn);
    if (!p->history) return lg_fail_msg(f + ": history is null");
    if (p->history_stride < p->n_history) return lg_fail_msg(f + ": history_stride = " + std::to_string(p->history_stride) + " is below its width " + std::to_string(p->n_history));
    for (int l = 0; l < p->n_conv; l++) {
        const LgTrainConv &c = p->conv[l];
        const std::string cn = f + ": conv[" + std::to_string(l) + "]";
        if (!c.weight) return lg_fail_msg(cn + ".weight is null");
        if (!c.bias) return lg_fail_msg(cn + ".bias is null");
        if (backward && !c.grad_weight) return lg_fail_msg(cn + ".grad_weight is null");
        if (backward && !c.grad_bias) return lg_fail_msg(cn + ".grad_bias is null");
        KConv &v = k.v[l];
        v.W = c.weight; v.b = c.bias; v.gW = backward ? c.grad_weight : nullptr; v.gb = backward ? c.grad_bias : nullptr;
    }
    if (bind_chain(f + ": tail", p->tail, k.c[TAIL], 0, backward)) return 1;
    if (bind_chain(f + ": privilege", p->privilege, k.c[PRI], p->privilege.layer[0].n_in, false)) return 1;
    if (!p->mask) return lg_fail_msg(f + ": mask is null");
    if (p->mask_stride < 1) return lg_fail_msg(f + ": mask_stride = " + std::to_string(p->mask_stride) + " is below its width 1");
    if (!backward && !p->loss) return lg_fail_msg(f + ": loss is null");
    if (backward && !p->upstream) return lg_fail_msg(f + ": upstream is null");
    if (check_ws(f, p->workspace, p->workspace_capacity, pl.workspace_floats, true)) return 1;
    k.ws = p->workspace;
    k.hist = p->history; k.hist_stride = p->history_stride;
    k.mask = p->mask; k.mask_stride = p->mask_stride;
    k.loss = p->loss; k.upstream = p->upstream;
    k.c[TAIL].in = p->workspace + pl.x_off[pl.n_conv]; k.c[TAIL].in_stride = pl.flat;       // f, as the conv stack left it
    return 0;
}

extern "C" int lg_train_tcn_plan(const LgTrainTcnArgs *args, LgTrainTcnPlan *out) {
    if (!out) return lg_fail_msg("lg_train_tcn_plan: null plan");
    NArgs k;
    return make_plan("lg_train_tcn_plan", args, *out, k);
}

extern "C" int lg_train_tcn_forward(const LgTrainTcnArgs *args, void *stream) {
    static const char *fn = "lg_train_tcn_forward";
    LgTrainTcnPlan pl; NArgs k;
    if (make_plan(fn, args, pl, k) || bind(fn, args, pl, k, false)) return 1;
    hipLaunchKernelGGL(train_tcn_conv_forward_kernel, dim3((unsigned)k.conv_blocks), dim3(kThreads), 0, (hipStream_t)stream, k);
    if (launch_tile(fn, kForward, raised_forward, 1, pl.lds_bytes, (hipStream_t)stream, k)) return 1;
    hipLaunchKernelGGL(train_tcn_finalize_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, k);
    return done(fn);
}

extern "C" int lg_train_tcn_backward(const LgTrainTcnArgs *args, void *stream) {
    static const char *fn = "lg_train_tcn_backward";
    LgTrainTcnPlan pl; NArgs k;
    if (make_plan(fn, args, pl, k) || bind(fn, args, pl, k, true)) return 1;
    const hipStream_t st = (hipStream_t)stream;
    if (launch_tile(fn, kInputGrad, raised_input_grad, 1, pl.lds_bytes, st, k)) return 1;
    if (k.n_conv > 1) hipLaunchKernelGGL(train_tcn_conv_input_grad_kernel, dim3((unsigned)k.conv_blocks), dim3(kThreads), 0, st, k);
    hipLaunchKernelGGL(train_tcn_weight_grad_kernel, dim3((unsigned)k.n_jobs), dim3(64), 0, st, k);
    hipLaunchKernelGGL(train_tcn_conv_weight_grad_kernel, dim3((unsigned)k.conv_jobs), dim3(kThreads), 0, st, k);
    long long elems = 1;
    for (int li = 0; li < k.c[TAIL].n_layers; li++) {
        const long long n = (long long)k.c[TAIL].l[li].M * k.c[TAIL].l[li].K + k.c[TAIL].l[li].M;
        if (n > elems) elems = n;
    }
    for (int l = 0; l < k.n_conv; l++)
        if (k.v[l].E > elems) elems = k.v[l].E;
    long long blocks = (elems + 255) / 256;
    if (blocks > 1024) blocks = 1024;                    // grid-stride behind that
    hipLaunchKernelGGL(train_tcn_combine_kernel, dim3((unsigned)blocks), dim3(256), 0, st, k);
    return done(fn);
}

// lg_train_rnn.hip -- the fused learner pass of the recurrent family behind include/lgtrainrnn.h: ActorCriticRecurrent's training forward
// (memory_a -> actor, memory_c -> critic over the padded trajectories of a mini-batch) and its backward through the chains, through time
// and into the memories' parameters.
//
// Reference call sites replaced: rsl_rl/algorithms/ppo.py:124-148 (PPO.update: actor_critic.act / evaluate with masks and hidden states)
// on rsl_rl/modules/actor_critic_recurrent.py:49-103 (Memory.forward in batch mode, unpad_trajectories) and the share of
// loss.backward() that runs through the two memories and the two MLPs.
//
// Everything the pass stores lives in UNPADDED ROW ORDER (row (s_j % T + t) E + s_j / T for step t of trajectory j, include/lgtrainrnn.h):
// the T E valid steps and nothing else, so the layer routines of lg_train_tiles.h and the chain, weight-gradient and combine routines of
// lg_train_pass.h run on a memory unchanged, each W_ih and W_hh of a layer being one TLayer without an activation:
//   index launch     one workgroup: the lengths (column sums of the mask), their prefix sums, each trajectory's first row, and per row the
//                    padded position t n_traj + j it came from.  Padding is never addressed again.
//   input launch     per layer, row tiles over the unpadded rows: W_ih x + b_ih by fwd_tile (x gathered in place from the padded
//                    observations for layer 0, the layer below's stored h above it).  No step depends on another here.
//   time forward     a workgroup owns R_t trajectories of one memory and walks t inside the kernel: h_(t-1) sits in LDS, W_hh h + b_hh by
//                    fwd_tile, the cell pointwise.  A step at or beyond a trajectory's length is skipped by a branch on its length.
//   time backward    the same ownership from the tile's last step down: D_t pointwise from the stored gates into LDS and the workspace,
//                    the carry dh_(t-1) = D_t W_hh by bwd_tile.
//   the chains       lg_train.hip's forward on the top layer's h; its input-gradient launch goes on through layer 0 into d loss / d h.
//   weight gradients every (weight, bias) pair of chains and memories as jobs of one launch: wgrad_wave over the unpadded rows (its
//                    copy below gathers layer 0's x rows through the index), partials per slice, combined in slice order.
// Plain stores only; two calls on the same inputs give the same bits.
#include "lg_train_pass.h"
#include "../../include/lgtrainrnn.h"

#define NM LG_TRAIN_RNN_MEMORIES
#define NL LG_TRAIN_RNN_MAX_LAYERS
#define LSTM LG_TRAIN_RNN_LSTM
#define IH 0
#define HH 1

struct MemK {
    const float *x, *h0, *c0;
    long long xts, xrs, hls, hrs, cls, crs;
    int kind, layers, H, In;
    long long gate_off[NL], h_off[NL], hprev_off[NL], c_off[NL], nh_off[NL], dout_off[NL], dx_off[NL], dh_off[NL];
    TLayer w[NL][2];            // [IH]: (weight_ih, bias_ih), K = the layer's input width; [HH]: (weight_hh, bias_hh), K = H; M = G H, no ELU
};
struct RArgs : PArgs {
    TChain c[LG_TRAIN_CHAINS];
    MemK m[NM];
    const uint8_t *mask;
    long long mts, index_off;
    int n_traj, max_len, T, E, Rt, t_tiles, layer, jobs_all;
};
static_assert(sizeof(RArgs) <= 4096, "RArgs is passed by value: the kernel-argument segment is 4 KB");

__device__ __forceinline__ int row_of(const RArgs &a, int first, int t) { return min(max(first + t * a.E, 0), a.N - 1); }

// the padded observation row an unpadded row came from, on clamped indices
__device__ __forceinline__ const float *x_row(const RArgs &a, const MemK &m, const int *map, int row) {
    const int p = max(map[row], 0), t = min(p / a.n_traj, a.max_len - 1), j = p - (p / a.n_traj) * a.n_traj;
    return m.x + (size_t)t * m.xts + (size_t)j * m.xrs;
}

template <int RB> __device__ __forceinline__ void fwd_layer(const TLayer &L, const lds_f *cur, lds_f *nxt, int R) {
    const int per_wave = (((L.M + 15) >> 4) + kWaves - 1) / kWaves;
    if (per_wave >= 4) fwd_tile<RB, 4>(L, cur, nxt, false, 0.f, R);
    else if (per_wave >= 2) fwd_tile<RB, 2>(L, cur, nxt, false, 0.f, R);
    else fwd_tile<RB, 1>(L, cur, nxt, false, 0.f, R);
}

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

// one workgroup.  Every row index is clamped (row_of): a mask outside the contract stores nothing out of range.
__global__ __launch_bounds__(256) void train_rnn_index_kernel(RArgs a) {
    __shared__ int part[kThreads];
    int *len = (int *)(a.ws + a.index_off), *first = len + a.n_traj, *map = first + a.n_traj;
    for (int j = threadIdx.x; j < a.n_traj; j += kThreads) {
        int n = 0;
        for (int t = 0; t < a.T; t++) n += a.mask[(size_t)t * a.mts + j] != 0;
        len[j] = min(n, a.max_len);
    }
    for (int i = threadIdx.x; i < a.N; i += kThreads) map[i] = 0;
    __syncthreads();
    const int per = (a.n_traj + kThreads - 1) / kThreads, jb = min((int)threadIdx.x * per, a.n_traj), je = min(jb + per, a.n_traj);
    int sum = 0;
    for (int j = jb; j < je; j++) sum += len[j];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int i = 0; i < kThreads; i++) { const int n = part[i]; part[i] = s; s += n; }
    }
    __syncthreads();
    int s = part[threadIdx.x];
    for (int j = jb; j < je; j++) {
        const int f = (s % a.T) * a.E + s / a.T, n = len[j];
        first[j] = f;
        for (int t = 0; t < n; t++) map[row_of(a, f, t)] = t * a.n_traj + j;
        s += n;
    }
}

// grid (row tiles of the unpadded rows, memories): W_ih x + b_ih of layer a.layer into the gate region
template <int RB> __global__ __launch_bounds__(256) void train_rnn_input_kernel(RArgs a) {
    extern __shared__ __align__(16) float lds[];
    const MemK &m = a.m[blockIdx.y];
    const int l = a.layer;
    if (l >= m.layers) return;
    const TLayer &L = m.w[l][IH];
    const int R = a.R, row0 = blockIdx.x * R, rows = min(R, a.N - row0);
    lds_f *b0 = (lds_f *)lds, *b1 = (lds_f *)lds + a.q_off;
    if (l) stage_rows(a.ws + m.h_off[l - 1], L.K, L.K, b0, L.sa, R, rows, row0);
    else {
        const int *map = (const int *)(a.ws + a.index_off) + 2 * a.n_traj;
        for (int i = threadIdx.x; i < R * L.K; i += kThreads) {
            const int row = i / L.K, col = i - row * L.K;
            b0[row * L.sa + col] = row < rows ? x_row(a, m, map, row0 + row)[col] : 0.f;
        }
    }
    __syncthreads();
    fwd_layer<RB>(L, b0, b1, R);
    __syncthreads();
    copy_out(b1, L.so, a.ws + m.gate_off[l], L.M, L.M, rows, row0);
}

// grid (trajectory tiles, memories): layer a.layer of one memory over the tile's trajectories, t inside
template <int RB> __global__ __launch_bounds__(256) void train_rnn_time_forward_kernel(RArgs a) {
    extern __shared__ __align__(16) float lds[];
    const MemK &m = a.m[blockIdx.y];
    const int l = a.layer;
    if (l >= m.layers) return;
    const TLayer &L = m.w[l][HH];
    const int R = a.Rt, j0 = blockIdx.x * R, H = m.H, GH = L.M, sH = L.sa, sG = L.so;
    const bool lstm = m.kind == LSTM;
    lds_f *hb = (lds_f *)lds, *cb = hb + R * sH, *gb = cb + R * sH;
    const int *len = (const int *)(a.ws + a.index_off), *first = len + a.n_traj;
    int steps = 0;
    for (int r = 0; r < R; r++) steps = max(steps, len[min(j0 + r, a.n_traj - 1)]);
    steps = min(steps, a.max_len);
    for (int i = threadIdx.x; i < R * H; i += kThreads) {
        const int row = i / H, col = i - row * H, j = min(j0 + row, a.n_traj - 1);
        hb[row * sH + col] = m.h0[(size_t)l * m.hls + (size_t)j * m.hrs + col];
        if (lstm) cb[row * sH + col] = m.c0[(size_t)l * m.cls + (size_t)j * m.crs + col];
    }
    __syncthreads();
    float *gate = a.ws + m.gate_off[l], *hout = a.ws + m.h_off[l], *hprev = a.ws + m.hprev_off[l];
    float *cst = a.ws + (lstm ? m.c_off[l] : m.nh_off[l]);
    for (int t = 0; t < steps; t++) {
        fwd_layer<RB>(L, hb, gb, R);                                  // W_hh h_(t-1) + b_hh
        __syncthreads();
        for (int i = threadIdx.x; i < R * H; i += kThreads) {
            const int row = i / H, col = i - row * H, j = j0 + row;
            if (j >= a.n_traj || t >= len[j]) continue;              // a step behind the trajectory's end: its state stays, nothing is stored
            const size_t r = (size_t)row_of(a, first[j], t);
            float *g = gate + r * GH + col;
            const lds_f *q = gb + row * sG + col;
            const float hp = hb[row * sH + col];
            float h;
            if (lstm) {
                const float gi = sigmoidf(g[0] + q[0]), gf = sigmoidf(g[H] + q[H]), gg = tanhf(g[2 * H] + q[2 * H]), go = sigmoidf(g[3 * H] + q[3 * H]);
                const float c = gf * cb[row * sH + col] + gi * gg;
                h = go * tanhf(c);
                g[0] = gi; g[H] = gf; g[2 * H] = gg; g[3 * H] = go;
                cb[row * sH + col] = c;
                cst[r * H + col] = c;
            } else {
                const float nh = q[2 * H];
                const float gr = sigmoidf(g[0] + q[0]), gz = sigmoidf(g[H] + q[H]), gn = tanhf(g[2 * H] + gr * nh);
                h = (1.f - gz) * gn + gz * hp;
                g[0] = gr; g[H] = gz; g[2 * H] = gn;
                cst[r * H + col] = nh;
            }
            hprev[r * H + col] = hp;
            hout[r * H + col] = h;
            hb[row * sH + col] = h;
        }
        __syncthreads();
    }
}

// the same grid and ownership, t from the tile's last step down to 0: D_t and the carries
template <int RB> __global__ __launch_bounds__(256) void train_rnn_time_backward_kernel(RArgs a) {
    extern __shared__ __align__(16) float lds[];
    const MemK &m = a.m[blockIdx.y];
    const int l = a.layer;
    if (l >= m.layers) return;
    const TLayer &L = m.w[l][HH];
    const int R = a.Rt, j0 = blockIdx.x * R, H = m.H, GH = L.M, sH = L.sa, sG = L.so;
    const bool lstm = m.kind == LSTM;
    lds_f *hb = (lds_f *)lds, *cb = hb + R * sH, *gb = cb + R * sH;   // hb: the carry dh; cb: the carry dc (LSTM), dh z (GRU)
    const int *len = (const int *)(a.ws + a.index_off), *first = len + a.n_traj;
    int steps = 0;
    for (int r = 0; r < R; r++) steps = max(steps, len[min(j0 + r, a.n_traj - 1)]);
    steps = min(steps, a.max_len);
    for (int i = threadIdx.x; i < R * sH; i += kThreads) { hb[i] = 0.f; cb[i] = 0.f; }
    __syncthreads();
    const float *gate = a.ws + m.gate_off[l], *hprev = a.ws + m.hprev_off[l], *dout = a.ws + m.dout_off[l];
    const float *cst = a.ws + (lstm ? m.c_off[l] : m.nh_off[l]);
    float *dx = a.ws + m.dx_off[l], *dh = lstm ? dx : a.ws + m.dh_off[l];
    for (int t = steps - 1; t >= 0; t--) {
        for (int i = threadIdx.x; i < R * H; i += kThreads) {
            const int row = i / H, col = i - row * H, j = j0 + row;
            lds_f *q = gb + row * sG + col;
            if (j >= a.n_traj || t >= len[j]) {                       // no step here: an exact zero reaches the carry
                q[0] = 0.f; q[H] = 0.f; q[2 * H] = 0.f;
                if (lstm) q[3 * H] = 0.f;
                continue;
            }
            const size_t r = (size_t)row_of(a, first[j], t);
            const float *g = gate + r * GH + col;
            const float d = dout[r * H + col] + hb[row * sH + col];
            if (lstm) {
                const float gi = g[0], gf = g[H], gg = g[2 * H], go = g[3 * H];
                const float cp = t ? cst[(size_t)row_of(a, first[j], t - 1) * H + col] : m.c0[(size_t)l * m.cls + (size_t)j * m.crs + col];
                const float tc = tanhf(cst[r * H + col]);
                const float dc = cb[row * sH + col] + d * go * (1.f - tc * tc);
                const float Di = dc * gg * gi * (1.f - gi), Df = dc * cp * gf * (1.f - gf), Dg = dc * gi * (1.f - gg * gg), Do = d * tc * go * (1.f - go);
                cb[row * sH + col] = dc * gf;
                float *o = dx + r * GH + col;
                o[0] = Di; o[H] = Df; o[2 * H] = Dg; o[3 * H] = Do;
                q[0] = Di; q[H] = Df; q[2 * H] = Dg; q[3 * H] = Do;
            } else {
                const float gr = g[0], gz = g[H], gn = g[2 * H], nh = cst[r * H + col], hp = hprev[r * H + col];
                const float Dn = d * (1.f - gz) * (1.f - gn * gn), Dr = Dn * nh * gr * (1.f - gr), Dz = d * (hp - gn) * gz * (1.f - gz);
                cb[row * sH + col] = d * gz;
                float *o = dx + r * GH + col, *p = dh + r * GH + col;
                o[0] = Dr; o[H] = Dz; o[2 * H] = Dn;
                p[0] = Dr; p[H] = Dz; p[2 * H] = Dn * gr;
                q[0] = Dr; q[H] = Dz; q[2 * H] = Dn * gr;
            }
        }
        __syncthreads();
        bwd_layer<RB>(L, gb, hb, false, R);                           // dh_(t-1) = D_t W_hh
        __syncthreads();
        if (!lstm) {
            for (int i = threadIdx.x; i < R * H; i += kThreads) {
                const int row = i / H, col = i - row * H;
                hb[row * sH + col] += cb[row * sH + col];
                cb[row * sH + col] = 0.f;
            }
            __syncthreads();
        }
    }
}

// grid (row tiles, memories): the upstream of the layer below a.layer, D W_ih, over the unpadded rows
template <int RB> __global__ __launch_bounds__(256) void train_rnn_input_grad_kernel(RArgs a) {
    extern __shared__ __align__(16) float lds[];
    const MemK &m = a.m[blockIdx.y];
    const int l = a.layer;
    if (l >= m.layers) return;
    const TLayer &L = m.w[l][IH];
    const int R = a.R, row0 = blockIdx.x * R, rows = min(R, a.N - row0);
    lds_f *b0 = (lds_f *)lds, *b1 = (lds_f *)lds + a.q_off;
    stage_rows(a.ws + m.dx_off[l], L.M, L.M, b1, L.so, R, rows, row0);
    __syncthreads();
    bwd_layer<RB>(L, b1, b0, false, R);
    __syncthreads();
    copy_out(b0, L.sa, a.ws + m.dout_off[l - 1], L.K, L.K, rows, row0);
}

// lg_train.hip's forward on the top layers' h
template <int RB> __global__ __launch_bounds__(256) void train_rnn_chain_forward_kernel(RArgs a) {
    extern __shared__ __align__(16) float lds[];
    const TChain &c = a.c[blockIdx.y];
    const int R = a.R, row0 = blockIdx.x * R, rows = min(R, a.N - row0);
    const bool actor = blockIdx.y == LG_TRAIN_ACTOR;
    const lds_f *mu = chain_from_rows<RB>(a.ws, c, (lds_f *)lds, (lds_f *)lds + a.q_off, true, actor && a.clip_on, a.clip, R, rows, row0);
    const int sm = c.l[c.n_layers - 1].so;
    copy_out(mu, sm, c.out, c.l[c.n_layers - 1].M, c.out_stride, rows, row0);
    if (actor) store_sigma(mu, sm, a.A, a.std, a.sigma, a.sigma_stride, rows, row0);
}

// lg_train.hip's input gradients, on through layer 0 (no activation factor: h is no ELU output) into the top layer's upstream
template <int RB> __global__ __launch_bounds__(256) void train_rnn_chain_backward_kernel(RArgs a) {
    extern __shared__ __align__(16) float lds[];
    const TChain &c = a.c[blockIdx.y];
    const MemK &m = a.m[blockIdx.y];
    const int R = a.R, row0 = blockIdx.x * R, rows = min(R, a.N - row0);
    lds_f *b0 = (lds_f *)lds, *b1 = (lds_f *)lds + a.q_off;
    seed_last_g(a.ws, c, (c.n_layers & 1) ? b1 : b0, nullptr, nullptr, blockIdx.y == LG_TRAIN_ACTOR && a.clip_on, a.clip, R, rows, row0);
    __syncthreads();
    chain_backward<RB>(a.ws, c, b0, b1, R, rows, row0);
    bwd_layer<RB>(c.l[0], b1, b0, false, R);
    __syncthreads();
    copy_out(b0, c.l[0].sa, a.ws + m.dout_off[m.layers - 1], m.H, m.H, rows, row0);
}

// lg_train_tiles.h's wgrad_wave for (weight_ih_l0, bias_ih_l0): the H operand's rows are the observation rows, gathered in place
__device__ __forceinline__ void wgrad_wave_x(const RArgs &a, const MemK &m, const TLayer &L, const float *G, int rel) {
    const int lane = threadIdx.x, r = lane & 15, h = lane >> 4;
    const int M = L.M, K = L.K, N = a.N;
    const int *map = (const int *)(a.ws + a.index_off) + 2 * a.n_traj;
    const int tiles_n = (M + LG_TRAIN_WG_TILE - 1) / LG_TRAIN_WG_TILE, per_slice = tiles_n * L.tiles_k;
    const int s = rel / per_slice, t = rel - s * per_slice, tn = t / L.tiles_k, tk = t - tn * L.tiles_k;
    const int n0 = tn * LG_TRAIN_WG_TILE, k0 = tk * LG_TRAIN_WG_TILE;
    const int rb = s * L.rps, re = min(rb + L.rps, N);
    int gc[kWT], hc[kWT];
#pragma unroll
    for (int i = 0; i < kWT; i++) {
        gc[i] = min(n0 + i * 16 + r, M - 1);
        hc[i] = min(k0 + i * 16 + r, K - 1);
    }
    f4 acc[kWT][kWT];
    float bsum[kWT];
#pragma unroll
    for (int i = 0; i < kWT; i++) {
        bsum[i] = 0.f;
#pragma unroll
        for (int j = 0; j < kWT; j++) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};
    }
    for (int row = rb + h; row < re + h; row += 4) {
        const bool ok = row < re;
        const int rc = min(row, re - 1);
        const float *xr = x_row(a, m, map, rc);
        float av[kWT], bv[kWT];
#pragma unroll
        for (int i = 0; i < kWT; i++) {
            const float g = G[(size_t)rc * M + gc[i]], x = xr[hc[i]];
            av[i] = ok ? g : 0.f;
            bv[i] = ok ? x : 0.f;
        }
#pragma unroll
        for (int i = 0; i < kWT; i++) {
            bsum[i] += av[i];
#pragma unroll
            for (int j = 0; j < kWT; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }
    float *P = a.ws + L.p_off + (size_t)s * ((size_t)M * K + M);
#pragma unroll
    for (int i = 0; i < kWT; i++)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int n = n0 + i * 16 + 4 * h + e;
#pragma unroll
            for (int j = 0; j < kWT; j++) {
                const int k = k0 + j * 16 + r;
                if (n < M && k < K) P[(size_t)n * K + k] = acc[i][j][e];
            }
        }
    if (tk == 0) {
#pragma unroll
        for (int i = 0; i < kWT; i++) {
            const float s0 = __shfl(bsum[i], r), s1 = __shfl(bsum[i], r + 16), s2 = __shfl(bsum[i], r + 32), s3 = __shfl(bsum[i], r + 48);
            const int n = n0 + i * 16 + r;
            if (h == 0 && n < M) P[(size_t)M * K + n] = ((s0 + s1) + s2) + s3;
        }
    }
}

// one wave per job: the chains' and grad_std's (lg_train_pass.h's wgrad_job) first, then per memory, layer and (IH, HH) pair
__global__ __launch_bounds__(64) void train_rnn_weight_grad_kernel(RArgs a) {
    const int job = blockIdx.x;
    if (job < a.n_jobs) { wgrad_job(a, a.c, 0, LG_TRAIN_CHAINS); return; }
    int mi = 0, li = 0, wi = 0;
    for (int m = 0; m < NM; m++)
        for (int l = 0; l < a.m[m].layers; l++)
            for (int w = 0; w < 2; w++)
                if (job >= a.m[m].w[l][w].job0) { mi = m; li = l; wi = w; }      // job0 rises with (m, l, w)
    const MemK &m = a.m[mi];
    const TLayer &L = m.w[li][wi];
    const float *G = a.ws + (wi == HH && m.kind != LSTM ? m.dh_off[li] : m.dx_off[li]);
    if (wi == HH) wgrad_wave(L, G, a.ws + m.hprev_off[li], L.K, a.ws, job - L.job0, a.N);
    else if (li) wgrad_wave(L, G, a.ws + m.h_off[li - 1], L.K, a.ws, job - L.job0, a.N);
    else wgrad_wave_x(a, m, L, G, job - L.job0);
}

__global__ __launch_bounds__(256) void train_rnn_combine_kernel(RArgs a) {
    combine_all(a, a.c, 0, LG_TRAIN_CHAINS);
    const long long stride = (long long)gridDim.x * blockDim.x, first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (int m = 0; m < NM; m++)
        for (int l = 0; l < a.m[m].layers; l++)
            for (int w = 0; w < 2; w++) combine_layer(a.m[m].w[l][w], a.ws, first, stride);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
typedef void (*const Pair[2])(RArgs);
static const char *kChain[LG_TRAIN_CHAINS] = {"chain[0] (actor)", "chain[1] (critic)"};
static const char *kMem[NM] = {"memory[0] (memory_a)", "memory[1] (memory_c)"};
static Pair kInput = {train_rnn_input_kernel<1>, train_rnn_input_kernel<2>};
static Pair kInputGrad = {train_rnn_input_grad_kernel<1>, train_rnn_input_grad_kernel<2>};
static Pair kTimeForward = {train_rnn_time_forward_kernel<1>, train_rnn_time_forward_kernel<2>};
static Pair kTimeBackward = {train_rnn_time_backward_kernel<1>, train_rnn_time_backward_kernel<2>};
static Pair kChainForward = {train_rnn_chain_forward_kernel<1>, train_rnn_chain_forward_kernel<2>};
static Pair kChainBackward = {train_rnn_chain_backward_kernel<1>, train_rnn_chain_backward_kernel<2>};
static bool raised[6][2][64];

static std::string range(const std::string &what, long long v, long long lo, long long hi) {
    return what + " = " + std::to_string(v) + " is outside [" + std::to_string(lo) + ", " + std::to_string(hi) + "]";
}

// the plan from the sizes alone; fills the size part of `k` too
static int make_plan(const char *fn, const LgTrainRnnArgs *p, LgTrainRnnPlan &pl, RArgs &k) {
    const std::string f(fn);
    if (!p) return lg_fail_msg(f + ": null descriptor");
    if (check_desc(f, &p->train)) return 1;
    pl = LgTrainRnnPlan{};
    k = RArgs{};
    const LgTrainRnnMemory &m0 = p->memory[0];
    for (int mi = 0; mi < NM; mi++) {
        const LgTrainRnnMemory &m = p->memory[mi];
        const std::string mn = f + ": " + kMem[mi];
        if (m.kind != LG_TRAIN_RNN_LSTM && m.kind != LG_TRAIN_RNN_GRU) return lg_fail_msg(mn + ".kind = " + std::to_string(m.kind) + " is neither LG_TRAIN_RNN_LSTM nor LG_TRAIN_RNN_GRU");
        if (m.n_layers < 1 || m.n_layers > NL) return lg_fail_msg(range(mn + ".n_layers", m.n_layers, 1, NL));
        if (m.hidden < 1 || m.hidden > LG_TRAIN_RNN_MAX_HIDDEN) return lg_fail_msg(range(mn + ".hidden", m.hidden, 1, LG_TRAIN_RNN_MAX_HIDDEN));
        if (m.n_in < 1 || m.n_in > LG_POLICY_MAX_WIDTH) return lg_fail_msg(range(mn + ".n_in", m.n_in, 1, LG_POLICY_MAX_WIDTH));
        if (m.T < 1) return lg_fail_msg(mn + ".T = " + std::to_string(m.T) + " < 1");
        if (m.n_traj < 1) return lg_fail_msg(mn + ".n_traj = " + std::to_string(m.n_traj) + " < 1");
        if (m.max_len < 1 || m.max_len > m.T) return lg_fail_msg(range(mn + ".max_len", m.max_len, 1, m.T) + " (1, T)");
        if (m.T != m0.T || m.n_traj != m0.n_traj || m.max_len != m0.max_len)
            return lg_fail_msg(mn + ": max_len, n_traj, T = " + std::to_string(m.max_len) + ", " + std::to_string(m.n_traj) + ", " + std::to_string(m.T) +
                               ", but memory[0] has " + std::to_string(m0.max_len) + ", " + std::to_string(m0.n_traj) + ", " + std::to_string(m0.T));
    }
    const int N = p->train.n_rows, T = m0.T, n_traj = m0.n_traj;
    if (N % T) return lg_fail_msg(f + ": n_rows = " + std::to_string(N) + " is no multiple of T = " + std::to_string(T));
    const int E = N / T;
    if (n_traj < E || n_traj > N)
        return lg_fail_msg(f + ": n_traj = " + std::to_string(n_traj) + " is outside [" + std::to_string(E) + ", " + std::to_string(N) + "] (n_rows / T envs, n_rows steps)");
    if ((long long)m0.max_len * n_traj > INT32_MAX) return lg_fail_msg(f + ": max_len * n_traj is above 2^31 - 1");
    int w[2] = {0, 0};
    for (int ci = 0; ci < LG_TRAIN_CHAINS; ci++) {
        if (plan_chain(f + ": " + kChain[ci], p->train.chain[ci], k.c[ci], 0, w)) return 1;
        if (k.c[ci].l[0].K != p->memory[ci].hidden)
            return lg_fail_msg(f + ": " + kChain[ci] + ".layer[0].n_in = " + std::to_string(k.c[ci].l[0].K) + ", but " + kMem[ci] + ".hidden = " + std::to_string(p->memory[ci].hidden));
    }
    long long off = 0;
    int t_floats = 0;
    for (int mi = 0; mi < NM; mi++) {
        const LgTrainRnnMemory &m = p->memory[mi];
        MemK &q = k.m[mi];
        q.kind = m.kind; q.layers = m.n_layers; q.H = m.hidden; q.In = m.n_in;
        const int H = m.hidden, GH = (m.kind == LG_TRAIN_RNN_LSTM ? 4 : 3) * H;
        for (int l = 0; l < NL; l++)
            pl.gate_off[mi][l] = pl.h_off[mi][l] = pl.hprev_off[mi][l] = pl.c_off[mi][l] = pl.nh_off[mi][l] = pl.dout_off[mi][l] = pl.dx_off[mi][l] = pl.dh_off[mi][l] =
                pl.p_off[mi][l][IH] = pl.p_off[mi][l][HH] = -1;
        for (int l = 0; l < m.n_layers; l++) {
            for (int wi = 0; wi < 2; wi++) {
                TLayer &L = q.w[l][wi];
                L.K = wi == IH && l == 0 ? m.n_in : H; L.M = GH; L.elu = 0;
                L.sa = lds_stride(L.K); L.so = lds_stride(GH);
            }
            if (q.w[l][IH].sa > w[0]) w[0] = q.w[l][IH].sa;
            if (q.w[l][IH].so > w[1]) w[1] = q.w[l][IH].so;
            pl.gate_off[mi][l] = q.gate_off[l] = off; off += (long long)N * GH;
            pl.h_off[mi][l] = q.h_off[l] = off; off += (long long)N * H;
            pl.hprev_off[mi][l] = q.hprev_off[l] = off; off += (long long)N * H;
            if (m.kind == LG_TRAIN_RNN_LSTM) { pl.c_off[mi][l] = q.c_off[l] = off; }
            else { pl.nh_off[mi][l] = q.nh_off[l] = off; }
            off += (long long)N * H;
            pl.dout_off[mi][l] = q.dout_off[l] = off; off += (long long)N * H;
            pl.dx_off[mi][l] = q.dx_off[l] = off; off += (long long)N * GH;
            if (m.kind != LG_TRAIN_RNN_LSTM) { pl.dh_off[mi][l] = q.dh_off[l] = off; off += (long long)N * GH; }
        }
        const int need = 2 * lds_stride(H) + lds_stride(GH);
        if (need > t_floats) t_floats = need;
    }
    pl.index_off = k.index_off = off; off += 2LL * n_traj + N;
    PassLayout lay;
    if (plan_layout(f, k, k.c, N, 0, LG_TRAIN_CHAINS, LG_TRAIN_ACTOR, LG_TRAIN_RNN_TARGET_JOBS, w, 0, false, off, lay)) return 1;
    plan_out(pl.train, k, k.c, lay);
    off = lay.workspace_floats;
    int jobs = k.n_jobs;
    for (int mi = 0; mi < NM; mi++)
        for (int l = 0; l < k.m[mi].layers; l++)
            for (int wi = 0; wi < 2; wi++) {
                TLayer &L = k.m[mi].w[l][wi];
                const int tn = (L.M + LG_TRAIN_WG_TILE - 1) / LG_TRAIN_WG_TILE;
                L.tiles_k = (L.K + LG_TRAIN_WG_TILE - 1) / LG_TRAIN_WG_TILE;
                slice_rule(N, (long long)tn * L.tiles_k, L.S, L.rps, LG_TRAIN_RNN_TARGET_JOBS);
                pl.slices[mi][l][wi] = L.S; pl.slice_rows[mi][l][wi] = L.rps;
                L.p_off = pl.p_off[mi][l][wi] = off; off += (long long)L.S * ((long long)L.M * L.K + L.M);
                L.job0 = jobs; jobs += L.S * tn * L.tiles_k;
            }
    k.jobs_all = pl.weight_jobs = jobs;
    pl.workspace_floats = off;
    k.n_traj = n_traj; k.max_len = m0.max_len; k.T = T; k.E = pl.n_envs = E;
    for (int R = 32; R >= 8; R >>= 1) {
        const size_t bytes = (size_t)R * t_floats * sizeof(float);
        if (bytes > kLdsBytes) continue;
        k.Rt = pl.time_row_tile = R; pl.time_lds_bytes = (int)bytes;
        k.t_tiles = pl.time_tiles = (n_traj + R - 1) / R;
        return 0;
    }
    return lg_fail_msg(f + ": an 8-trajectory tile of these memories (" + std::to_string(t_floats) + " floats per trajectory) does not fit the 160 KB of LDS");
}

// the pointers and strides; `backward`: the gradient members too
static int bind(const char *fn, const LgTrainRnnArgs *p, const LgTrainRnnPlan &pl, RArgs &k, bool backward) {
    const std::string f(fn);
    static const char *pn[4] = {"weight_ih", "weight_hh", "bias_ih", "bias_hh"};
    for (int mi = 0; mi < NM; mi++) {
        const LgTrainRnnMemory &m = p->memory[mi];
        MemK &q = k.m[mi];
        const std::string mn = f + ": " + kMem[mi];
        for (int l = 0; l < m.n_layers; l++) {
            const LgTrainRnnLayer &s = m.layer[l];
            const float *par[4] = {s.weight_ih, s.weight_hh, s.bias_ih, s.bias_hh};
            float *gr[4] = {s.grad_weight_ih, s.grad_weight_hh, s.grad_bias_ih, s.grad_bias_hh};
            for (int i = 0; i < 4; i++) {
                if (!par[i]) return lg_fail_msg(mn + ".layer[" + std::to_string(l) + "]." + pn[i] + " is null");
                if (backward && !gr[i]) return lg_fail_msg(mn + ".layer[" + std::to_string(l) + "].grad_" + pn[i] + " is null");
            }
            q.w[l][IH].W = s.weight_ih; q.w[l][IH].b = s.bias_ih; q.w[l][HH].W = s.weight_hh; q.w[l][HH].b = s.bias_hh;
            if (backward) { q.w[l][IH].gW = s.grad_weight_ih; q.w[l][IH].gb = s.grad_bias_ih; q.w[l][HH].gW = s.grad_weight_hh; q.w[l][HH].gb = s.grad_bias_hh; }
        }
        if (!m.x) return lg_fail_msg(mn + ".x is null");
        if (!m.h0) return lg_fail_msg(mn + ".h0 is null");
        if (m.kind == LG_TRAIN_RNN_LSTM && !m.c0) return lg_fail_msg(mn + ".c0 is null");
        if (!m.mask) return lg_fail_msg(mn + ".mask is null");
        if (m.x_row_stride < m.n_in) return lg_fail_msg(mn + ".x_row_stride = " + std::to_string(m.x_row_stride) + " is below its width " + std::to_string(m.n_in));
        if (m.x_time_stride < 0) return lg_fail_msg(mn + ".x_time_stride = " + std::to_string(m.x_time_stride) + " < 0");
        if (m.h0_row_stride < m.hidden) return lg_fail_msg(mn + ".h0_row_stride = " + std::to_string(m.h0_row_stride) + " is below its width " + std::to_string(m.hidden));
        if (m.h0_layer_stride < 0) return lg_fail_msg(mn + ".h0_layer_stride = " + std::to_string(m.h0_layer_stride) + " < 0");
        if (m.kind == LG_TRAIN_RNN_LSTM && m.c0_row_stride < m.hidden)
            return lg_fail_msg(mn + ".c0_row_stride = " + std::to_string(m.c0_row_stride) + " is below its width " + std::to_string(m.hidden));
        if (m.kind == LG_TRAIN_RNN_LSTM && m.c0_layer_stride < 0) return lg_fail_msg(mn + ".c0_layer_stride = " + std::to_string(m.c0_layer_stride) + " < 0");
        if (m.mask_time_stride < m.n_traj) return lg_fail_msg(mn + ".mask_time_stride = " + std::to_string(m.mask_time_stride) + " is below n_traj = " + std::to_string(m.n_traj));
        if (m.mask != p->memory[0].mask || m.mask_time_stride != p->memory[0].mask_time_stride) return lg_fail_msg(mn + ".mask is not memory[0]'s mask");
        q.x = m.x; q.xts = m.x_time_stride; q.xrs = m.x_row_stride;
        q.h0 = m.h0; q.hls = m.h0_layer_stride; q.hrs = m.h0_row_stride;
        q.c0 = m.c0; q.cls = m.c0_layer_stride; q.crs = m.c0_row_stride;
    }
    k.mask = p->memory[0].mask; k.mts = p->memory[0].mask_time_stride;
    for (int ci = 0; ci < LG_TRAIN_CHAINS; ci++)
        if (bind_chain(f + ": " + kChain[ci], p->train.chain[ci], k.c[ci], 0, backward)) return 1;
    if (bind_heads(f, &p->train, k, k.c[LG_TRAIN_ACTOR], k.c[LG_TRAIN_CRITIC], pl.workspace_floats, backward)) return 1;
    for (int ci = 0; ci < LG_TRAIN_CHAINS; ci++) {                        // a chain reads its memory's top layer where the time loop left it
        k.c[ci].in = p->train.workspace + k.m[ci].h_off[k.m[ci].layers - 1];
        k.c[ci].in_stride = k.m[ci].H;
    }
    return 0;
}

static int launch_time(const char *fn, Pair &kern, bool (&r)[2][64], int lds_bytes, hipStream_t stream, const RArgs &k) {
    const int rb = k.Rt == 32;
    if (raise_lds(fn, (const void *)kern[rb], r[rb])) return 1;
    hipLaunchKernelGGL(kern[rb], dim3((unsigned)k.t_tiles, NM), dim3(kThreads), (size_t)lds_bytes, stream, k);
    return 0;
}

extern "C" int lg_train_rnn_plan(const LgTrainRnnArgs *args, LgTrainRnnPlan *out) {
    if (!out) return lg_fail_msg("lg_train_rnn_plan: null plan");
    RArgs k;
    return make_plan("lg_train_rnn_plan", args, *out, k);
}

extern "C" int lg_train_rnn_forward(const LgTrainRnnArgs *args, void *stream) {
    static const char *fn = "lg_train_rnn_forward";
    LgTrainRnnPlan pl; RArgs k;
    if (make_plan(fn, args, pl, k) || bind(fn, args, pl, k, false)) return 1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(train_rnn_index_kernel, dim3(1), dim3(kThreads), 0, st, k);
    const int layers = k.m[0].layers > k.m[1].layers ? k.m[0].layers : k.m[1].layers;
    for (k.layer = 0; k.layer < layers; k.layer++) {
        if (launch_tile(fn, kInput, raised[0], NM, pl.train.lds_bytes, st, k)) return 1;
        if (launch_time(fn, kTimeForward, raised[1], pl.time_lds_bytes, st, k)) return 1;
    }
    return launch_tile(fn, kChainForward, raised[2], LG_TRAIN_CHAINS, pl.train.lds_bytes, st, k) || done(fn);
}

extern "C" int lg_train_rnn_backward(const LgTrainRnnArgs *args, void *stream) {
    static const char *fn = "lg_train_rnn_backward";
    LgTrainRnnPlan pl; RArgs k;
    if (make_plan(fn, args, pl, k) || bind(fn, args, pl, k, true)) return 1;
    hipStream_t st = (hipStream_t)stream;
    if (launch_tile(fn, kChainBackward, raised[3], LG_TRAIN_CHAINS, pl.train.lds_bytes, st, k)) return 1;
    const int layers = k.m[0].layers > k.m[1].layers ? k.m[0].layers : k.m[1].layers;
    for (k.layer = layers - 1; k.layer >= 0; k.layer--) {
        if (launch_time(fn, kTimeBackward, raised[4], pl.time_lds_bytes, st, k)) return 1;
        if (k.layer && launch_tile(fn, kInputGrad, raised[5], NM, pl.train.lds_bytes, st, k)) return 1;
    }
    hipLaunchKernelGGL(train_rnn_weight_grad_kernel, dim3((unsigned)k.jobs_all), dim3(64), 0, st, k);
    long long elems = k.A;
    auto widest = [&elems](const TLayer &L) { const long long n = (long long)L.M * L.K + L.M; if (n > elems) elems = n; };
    for (int ci = 0; ci < LG_TRAIN_CHAINS; ci++)
        for (int li = 0; li < k.c[ci].n_layers; li++) widest(k.c[ci].l[li]);
    for (int mi = 0; mi < NM; mi++)
        for (int l = 0; l < k.m[mi].layers; l++) { widest(k.m[mi].w[l][IH]); widest(k.m[mi].w[l][HH]); }
    long long blocks = (elems + 255) / 256;
    if (blocks > 1024) blocks = 1024;                    // grid-stride behind that
    hipLaunchKernelGGL(train_rnn_combine_kernel, dim3((unsigned)blocks), dim3(256), 0, st, k);
    return done(fn);
}

// lg_policy.hip -- the fused policy step behind include/lgpolicy.h.
//
// Reference call sites replaced: rsl_rl/algorithms/ppo.py:93-105 (PPO.act: actor_critic.act, evaluate, get_actions_log_prob, action_mean,
// action_std) on rsl_rl/modules/actor_critic.py:57-123 and actor_critic_ee.py:33-142 -- about 25 torch launches per rollout step (eight
// f32 GEMMs, their ELUs, a randn, the log-prob arithmetic, five copy_ into the storage rows) as ONE launch.
//
// Layout.  A workgroup (4 waves) owns a tile of R env rows (32, 16 or 8: `plan` takes the largest whose activations fit the 160 KB LDS)
// and carries it through every layer of one sequence: blockIdx.y = 0 is [estimator ->] actor -> sampling epilogue, blockIdx.y = 1 the
// critic.  Activations ping-pong between two LDS buffers (row stride = 4 mod 64 floats, so the 16 rows of a b128 fragment read fall on
// different banks); weights are read from global memory where torch keeps them, (out, in) row-major, four consecutive k per lane.
//
// One MFMA v_mfma_f32_16x16x4_f32 computes D[i][j] += sum_k A[i][k] B[k][j] with A = W (i = output neuron), B = X^T (j = env row): lane
// (r = lane & 15, h = lane >> 4) supplies W[n0 + r][k] and X[row r][k] and receives D rows 4h .. 4h+3 of column r, i.e. FOUR CONSECUTIVE
// NEURONS OF ONE ENV ROW -- for the actor's last layer one action quad, which is what one Philox block serves.  A lane loads k = k0 + 4h
// .. + 3 as one 16-byte read and feeds element e to the e-th of four MFMAs, so the k order inside a 16-wide chunk is permuted; the sum is
// the same set of products (an exact-f32 fmaf chain, cdna_hip_programming.md section 3).  A wave holds NT (1, 2, 4) neuron tiles x RB (1, 2)
// row blocks of accumulators, NT * RB >= 2 independent chains wherever the layer is wide enough to matter.  No width is assumed to be a
// tile multiple: the K tail is loaded element by element with zeros behind K on BOTH operands, neurons >= out and rows >= N are computed
// on clamped addresses and never stored.
//
// Row groups (CTS, rsl_rl/algorithms/ppo_cts.py:110-135).  With `encoder_b` / `n_split` the policy tiles (blockIdx.y = 0) are two runs: tiles
// [0, tiles_a) carry env rows [0, n_split) through seq[0] (estimator -> actor), the rest carry [n_split, N) through seq[1] (encoder_b -> the
// same actor layers).  A tile never straddles the split: it knows its sequence's [row_begin, row_end), rows behind row_end are staged as
// zeros and never stored, and every global row address is row0 + row < row_end.  The critic (blockIdx.y = 1) stays one run over [0, N).
//
// VAE head (DreamWaQ, rsl_rl/modules/vae.py:65-101).  The four heads are FOUR LAYERS that read the same activation (the encoder's output)
// and write disjoint columns of the next one, [latent_mu | latent_logvar | vel_mu | vel_logvar] (a layer names its source and destination
// activation; the clip of the two log-variances is the layer clip the actor's end already has).  `reparam` then forms the actor's input
// [obs | z | vel] in the other buffer: sample = eps * exp(0.5 logvar) + mu, or the means in deterministic mode.
//
// Memories (rsl_rl/modules/actor_critic_recurrent.py: an LSTM / GRU in front of the actor and of the critic).  A memory is a PREFIX of its
// sequence: blockIdx.y = 0 runs memory_a -> actor -> epilogue, the critic's run memory_c -> critic.  Per rnn layer:
//   stage   X = [x, padded to a multiple of 4 floats | h_prev] is one activation (the pad keeps the h part on the 16-byte alignment of the
//           b128 fragment reads); h_prev is masked by reset_mask on load and goes to h_prev_out from the same load.  For layer 0 the x
//           part is the staged observation; for layer 1 it is the h' the cell of layer 0 left there (below).
//   gates   layers with TWO operands (KLayer::W2): an LSTM's W_ih x + W_hh h lands in one 4H-wide activation G with one layer; a GRU
//           takes three layers into G = [r | z | n_x | n_h]: (r, z) with both operands, n_x from x alone, n_h from h alone (r multiplies
//           the hidden part only, bias included).
//   cell    pointwise, one lane per (env row, hidden unit), a sibling of `reparam`: reads the unit's four gate columns (and c_prev from
//           global memory, masked, copied to c_prev_out; a GRU's h_prev from X), writes c' and h' to the global states and h' OVER
//           COLUMN j OF G -- the only reader of G[row][j] is the lane that writes it.  So G's columns [0, H) become the next input: the
//           actor's, or the x part of rnn layer 1, whose h_prev is then staged behind it into the dead gate columns of G.
// In-place safety of the states: a workgroup touches only the state rows of its own tile; the stage of a layer (all reads of that
// layer's h) is separated by a barrier from its cell (the writes), and c is read and written by the same lane; the policy run touches
// memory_a only, the critic's run memory_c only.  expf / tanhf are the device library's, not fast-math intrinsics: parity with torch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/lgpolicy.h"
#include "lg_math.h"

int lg_fail_msg(const std::string &m);   // lg_host.hip: sets the thread-local message, returns 1

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // weight rows start wherever in * 4 bytes puts them
typedef __attribute__((address_space(3))) float lds_f;               // activations: explicit LDS pointers (ds_* instead of flat_*)
typedef __attribute__((address_space(3))) f4 lds_f4;

static const int kThreads = 256, kWaves = 4, kMaxSeqLayers = 3 * LG_POLICY_MAX_LAYERS;   // leading chain, four heads, actor; or a memory's gate layers (<= 6), actor
static const size_t kLdsBytes = 160u * 1024u;      // gfx950: 160 KB per workgroup

struct KLayer {
    const float *W, *b;
    const float *W2, *b2;   // second operand (NULL: none): the sum runs on over W2[n][0 .. K2) * src[row][src_col2 + k], and b2[n] joins the bias
    float *gout;            // global destination of this layer's output (NULL: LDS only)
    const float *cat_src;   // rows copied into columns [0, cat_w) of the output activation (the EE concatenation)
    int K, M, elu, clip_on;
    float clip;
    int out_col, gstride, cat_w, cat_stride;
    int src, dst;           // activation read and written; activation i lives in buffer i & 1 with row stride PSeq::stride[i] ...
    int sa, so;             // ... which `plan` copies here (stride[src], stride[dst]) so that a layer's operands are one read of its KLayer
    int src_col, K2, src_col2;   // first column of the source read by W (a multiple of 4); the second operand's K and column
};
struct KMem {                            // a memory as the kernel walks it
    float *h, *c, *h_prev_out, *c_prev_out;     // (n_layers, N, H)
    const uint8_t *mask;
    int kind, n_layers, H;
    int cell_after[LG_POLICY_MAX_RNN_LAYERS];   // sequence-relative index of rnn layer k's last gate layer: its cell follows
    int x_col[LG_POLICY_MAX_RNN_LAYERS];        // column of h_prev in layer k's input activation (the padded x width)
};
struct KSeq {                            // one sequence as the kernel walks it: its layers are l[first .. first + n_layers) of KArgs
    const float *in;
    int in_w, in_stride, stride0;       // the staged input and its LDS row stride
    int first, n_layers, epilogue;
    int row_begin, row_end;             // the env rows this sequence serves
    int reparam_after;                  // index of the last head layer (the reparameterisation follows it), or -1
    int mem;                            // index into KArgs::mem of the memory this sequence starts with, or -1
};
struct KHead {                           // the reparameterisation behind the four head layers
    const float *obs, *noise;           // the actor's features (N, F); eps (N, L + E) or NULL: Philox
    float *latent_out, *dbg_uniform;
    int F, L, E, obs_stride, noise_stride, latent_stride, determ;
    int sx;                             // LDS row stride of the activation [obs | z | vel]
};
// every layer of the launch, packed: two group sequences of leading chain + actor and the critic (CTS, 20), or leading chain + four
// heads + actor and the critic (DreamWaQ, 16).  A sequence takes only the slots it uses, so the block stays near the size it had.
static const int kMaxLayers = 5 * LG_POLICY_MAX_LAYERS;
struct KArgs {
    KSeq seq[3];
    KLayer l[kMaxLayers];
    KHead head;
    KMem mem[2];
    int N, R, q_off, A;
    int tiles_a, seq_y1;                // policy tiles below tiles_a run seq[0], the others seq[1]; blockIdx.y = 1 runs seq[seq_y1]
    const float *std, *noise;
    float *actions, *mu, *sigma, *log_prob, *dbg_uniform;
    const unsigned *counter;
    int noise_stride, actions_stride, mu_stride, sigma_stride, log_prob_stride;
    unsigned seed_lo, seed_hi;
};
static_assert(sizeof(KArgs) <= 4096, "KArgs is passed by value: the kernel-argument segment is 4 KB");

// one layer for the workgroup's row tile: nxt[row][out_col + n] = act(b[n] + sum_k W[n][k] cur[row][k])
// TWO: the layer has a second operand (a memory's gate layer); without it the loop below runs once and is the single K loop it always was
template <int RB, int NT, bool TWO>
__device__ __forceinline__ void layer_tile(const KLayer &L, const lds_f *cur, int sa, lds_f *nxt, int so, int R, int rows, int row0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, h = lane >> 4;
    const int M = L.M, tiles = (M + 15) >> 4, n_op = TWO ? 2 : 1;
    for (int tb = wave * NT; tb < tiles; tb += kWaves * NT) {
        f4 acc[RB][NT];
#pragma unroll
        for (int i = 0; i < NT; i++)
#pragma unroll
            for (int j = 0; j < RB; j++) acc[j][i] = (f4){0.f, 0.f, 0.f, 0.f};
        for (int op = 0; op < n_op; op++) {      // the second operand continues the same accumulator chains
            const float *Wm = TWO && op ? L.W2 : L.W;
            const int K = TWO && op ? L.K2 : L.K, col = TWO && op ? L.src_col2 : L.src_col;
            const float *wp[NT];
            const lds_f *xp[RB];
#pragma unroll
            for (int i = 0; i < NT; i++) {
                const int n = min((tb + i) * 16 + r, M - 1);
                wp[i] = Wm + (size_t)n * K + 4 * h;
            }
#pragma unroll
            for (int j = 0; j < RB; j++) xp[j] = cur + min(j * 16 + r, R - 1) * sa + col + 4 * h;
            int k0 = 0;
            for (; k0 + 16 <= K; k0 += 16) {
                f4 av[NT], bv[RB];
#pragma unroll
                for (int i = 0; i < NT; i++) av[i] = *(const f4u *)(wp[i] + k0);
#pragma unroll
                for (int j = 0; j < RB; j++) bv[j] = *(const lds_f4 *)(xp[j] + k0);
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int j = 0; j < RB; j++)
#pragma unroll
                        for (int i = 0; i < NT; i++) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][e], bv[j][e], acc[j][i], 0, 0, 0);
            }
            if (k0 < K) {                        // K tail: element-wise, zeros behind K on both operands
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const bool ok = k0 + 4 * h + e < K;
                    float bs[RB];
#pragma unroll
                    for (int j = 0; j < RB; j++) bs[j] = ok ? xp[j][k0 + e] : 0.f;
#pragma unroll
                    for (int i = 0; i < NT; i++) {
                        const float as = ok ? wp[i][k0 + e] : 0.f;
#pragma unroll
                        for (int j = 0; j < RB; j++) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, bs[j], acc[j][i], 0, 0, 0);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NT; i++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int n = (tb + i) * 16 + 4 * h + e;
                if (n < M) {
                    const float bias = TWO ? L.b[n] + L.b2[n] : L.b[n];
#pragma unroll
                    for (int j = 0; j < RB; j++) {
                        const int row = j * 16 + r;
                        float v = acc[j][i][e] + bias;
                        if (L.elu) v = v > 0.f ? v : expm1f(v);
                        if (L.clip_on) v = v < -L.clip ? -L.clip : (v > L.clip ? L.clip : v);     // compares, not fminf / fmaxf: a NaN stays a NaN, as with torch's Hardtanh
                        if (row < R) nxt[row * so + L.out_col + n] = v;
                        if (L.gout && row < rows) L.gout[(size_t)(row0 + row) * L.gstride + n] = v;
                    }
                }
            }
    }
}

template <int RB> __device__ __forceinline__ void layer(const KLayer &L, const lds_f *cur, int sa, lds_f *nxt, int so, int R, int rows, int row0) {
    const int per_wave = (((L.M + 15) >> 4) + kWaves - 1) / kWaves;
    if (L.W2) {
        if (per_wave >= 4) layer_tile<RB, 4, true>(L, cur, sa, nxt, so, R, rows, row0);
        else if (per_wave >= 2) layer_tile<RB, 2, true>(L, cur, sa, nxt, so, R, rows, row0);
        else layer_tile<RB, 1, true>(L, cur, sa, nxt, so, R, rows, row0);
    } else if (per_wave >= 4) layer_tile<RB, 4, false>(L, cur, sa, nxt, so, R, rows, row0);
    else if (per_wave >= 2) layer_tile<RB, 2, false>(L, cur, sa, nxt, so, R, rows, row0);
    else layer_tile<RB, 1, false>(L, cur, sa, nxt, so, R, rows, row0);
}

// rows [0, R) x columns [0, w) of a global (N, w) matrix into an LDS activation; rows behind N read as zero
__device__ __forceinline__ void stage_rows(const float *src, int w, int stride, lds_f *dst, int sd, int R, int rows, int row0) {
    for (int i = threadIdx.x; i < R * w; i += kThreads) {
        const int row = i / w, c = i - row * w;
        dst[row * sd + c] = row < rows ? src[(size_t)(row0 + row) * stride + c] : 0.f;
    }
}

// four uniforms of one Philox block and the four normals Box-Muller makes of them: (x, y) and (z, w) give two each
__device__ __forceinline__ void draw4(unsigned env, unsigned quad, unsigned counter, unsigned tag, unsigned seed_lo, unsigned seed_hi, float *u, float *z) {
    const U4 c = {env, quad, counter, tag};
    const U4 x = philox4x32_10(c, seed_lo, seed_hi);
    u[0] = u01(x.x); u[1] = u01(x.y); u[2] = u01(x.z); u[3] = u01(x.w);
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const float rad = sqrtf(-2.0f * logf(1.0f - u[2 * p])), th = 6.283185307179586f * u[2 * p + 1];
        z[2 * p] = rad * cosf(th);
        z[2 * p + 1] = rad * sinf(th);
    }
}

// par[row] = [latent_mu (L) | latent_logvar (L) | vel_mu (E) | vel_logvar (E)] -> x[row] = [obs (F) | z (L) | vel (E)]: one lane per
// (env row, quad of the L + E sampled columns); vae.py:84-92, or the means alone (vae.py:98-101) in deterministic mode
__device__ __forceinline__ void reparam(const KArgs &a, const lds_f *par, int sp, lds_f *x, int sx, int R, int rows, int row0) {
    const KHead &hd = a.head;
    const int L = hd.L, E = hd.E, W = L + E, Q = (W + 3) >> 2;
    stage_rows(hd.obs, hd.F, hd.obs_stride, x, sx, R, rows, row0);
    for (int t = threadIdx.x; t < R * Q; t += kThreads) {
        const int row = t / Q, q = t - row * Q;
        const size_t env = (size_t)row0 + row;
        float eps[4] = {0.f, 0.f, 0.f, 0.f};
        if (row < rows && !hd.determ) {
            if (hd.noise) {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (4 * q + e < W) eps[e] = hd.noise[env * hd.noise_stride + 4 * q + e];
            } else {
                float u[4];
                draw4((unsigned)env, (unsigned)q, a.counter[0], LG_POLICY_LATENT_TAG, a.seed_lo, a.seed_hi, u, eps);
                if (hd.dbg_uniform)
#pragma unroll
                    for (int e = 0; e < 4; e++) hd.dbg_uniform[env * (4 * Q) + 4 * q + e] = u[e];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int c = 4 * q + e;
            if (c < W) {
                const int im = c < L ? c : 2 * L + (c - L), iv = c < L ? L + c : 2 * L + E + (c - L);
                const float mu = par[row * sp + im];
                const float v = hd.determ ? mu : eps[e] * expf(0.5f * par[row * sp + iv]) + mu;
                x[row * sx + hd.F + c] = v;
                if (hd.latent_out && row < rows) hd.latent_out[env * hd.latent_stride + c] = v;
            }
        }
    }
}

// rnn layer k's incoming h of the tile's rows into columns [col, col + H) of an LDS activation: masked rows and rows behind the tile's end
// read as zero (a select: a NaN in a masked state does not get through); h_prev_out takes the same values
__device__ __forceinline__ void stage_state(const KMem &m, int k, int N, lds_f *dst, int sd, int col, int R, int rows, int row0) {
    const int H = m.H;
    const size_t base = (size_t)k * N * H;
    for (int i = threadIdx.x; i < R * H; i += kThreads) {
        const int row = i / H, j = i - row * H;
        float v = 0.f;
        if (row < rows) {
            const size_t env = (size_t)row0 + row, at = base + env * H + j;
            if (!(m.mask && m.mask[env])) v = m.h[at];
            if (m.h_prev_out) m.h_prev_out[at] = v;
        }
        dst[row * sd + col + j] = v;
    }
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// the cell of rnn layer k: g[row] holds the gates (LSTM [i | f | g | o], GRU [r | z | n_x | n_h], each H wide), x[row][hcol ..] the
// (masked) incoming h.  One lane per (env row, unit j): h' replaces g[row][j], which only this lane reads; h' and c' go to the global
// states of the tile's own rows, whose previous values this workgroup has read before (h: `stage_state`, a barrier ago; c: this lane).
__device__ __forceinline__ void cell(const KMem &m, int k, int N, lds_f *g, int sg, const lds_f *x, int sx, int hcol, int R, int rows, int row0) {
    const int H = m.H;
    const size_t base = (size_t)k * N * H;
    for (int i = threadIdx.x; i < R * H; i += kThreads) {
        const int row = i / H, j = i - row * H;
        const bool live = row < rows;
        const size_t env = (size_t)row0 + row, at = base + env * H + j;
        lds_f *gr = g + row * sg;
        float hn;
        if (m.kind == LG_POLICY_LSTM) {
            float cp = 0.f;
            if (live) {
                if (!(m.mask && m.mask[env])) cp = m.c[at];
                if (m.c_prev_out) m.c_prev_out[at] = cp;
            }
            const float cn = sigmoidf_(gr[H + j]) * cp + sigmoidf_(gr[j]) * tanhf(gr[2 * H + j]);
            hn = sigmoidf_(gr[3 * H + j]) * tanhf(cn);
            if (live) m.c[at] = cn;
        } else {
            const float r = sigmoidf_(gr[j]), z = sigmoidf_(gr[H + j]);
            const float n = tanhf(gr[2 * H + j] + r * gr[3 * H + j]);
            hn = (1.0f - z) * n + z * x[row * sx + hcol + j];
        }
        gr[j] = hn;
        if (live) m.h[at] = hn;
    }
}

template <int RB> __global__ __launch_bounds__(256) void policy_act_kernel(KArgs a) {
    extern __shared__ __align__(16) float lds[];
    int tile = blockIdx.x, si = a.seq_y1;
    if (blockIdx.y == 0) {
        si = tile >= a.tiles_a;
        if (si) tile -= a.tiles_a;
    }
    const KSeq &s = a.seq[si];
    const int R = a.R, row0 = s.row_begin + tile * R;
    if (row0 >= s.row_end) return;                       // the whole workgroup: the critic's run can be a tile shorter than the policy's two
    const int rows = min(R, s.row_end - row0);
    lds_f *buf[2] = {(lds_f *)lds, (lds_f *)lds + a.q_off};
    stage_rows(s.in, s.in_w, s.in_stride, buf[0], s.stride0, R, rows, row0);
    if (s.mem >= 0) stage_state(a.mem[s.mem], 0, a.N, buf[0], s.stride0, a.mem[s.mem].x_col[0], R, rows, row0);
    __syncthreads();
    for (int li = 0; li < s.n_layers; li++) {
        const KLayer &L = a.l[s.first + li];
        lds_f *nxt = buf[L.dst & 1];
        layer<RB>(L, buf[L.src & 1], L.sa, nxt, L.so, R, rows, row0);
        if (L.cat_src) stage_rows(L.cat_src, L.cat_w, L.cat_stride, nxt, L.so, R, rows, row0);
        __syncthreads();
        if (li == s.reparam_after) {
            reparam(a, nxt, L.so, buf[(L.dst + 1) & 1], a.head.sx, R, rows, row0);
            __syncthreads();
        }
        if (s.mem >= 0) {
            const KMem &m = a.mem[s.mem];
            for (int k = 0; k < m.n_layers; k++)
                if (li == m.cell_after[k]) {
                    cell(m, k, a.N, nxt, L.so, buf[L.src & 1], L.sa, m.x_col[k], R, rows, row0);
                    __syncthreads();
                    if (k + 1 < m.n_layers) {            // the gates are dead: the next layer's h_prev goes behind the new h'
                        stage_state(m, k + 1, a.N, nxt, L.so, m.x_col[k + 1], R, rows, row0);
                        __syncthreads();
                    }
                }
        }
    }
    if (!s.epilogue) return;
    // sampling epilogue: one lane per (env row, action quad); the log-prob terms replace mu in LDS, then one lane per row sums them in order
    const KLayer &last = a.l[s.first + s.n_layers - 1];
    lds_f *m = buf[last.dst & 1];
    const int sm = last.so, A = a.A, Q = (A + 3) >> 2;
    for (int t = threadIdx.x; t < R * Q; t += kThreads) {
        const int row = t / Q, q = t - row * Q;
        if (row >= rows) continue;
        const size_t env = (size_t)row0 + row;
        float z[4];
        if (a.noise) {
#pragma unroll
            for (int e = 0; e < 4; e++) z[e] = 4 * q + e < A ? a.noise[env * a.noise_stride + 4 * q + e] : 0.f;
        } else {
            float u[4];
            draw4((unsigned)env, (unsigned)q, a.counter[0], LG_POLICY_STREAM_TAG, a.seed_lo, a.seed_hi, u, z);
            if (a.dbg_uniform)
#pragma unroll
                for (int e = 0; e < 4; e++) a.dbg_uniform[env * (4 * Q) + 4 * q + e] = u[e];
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int ai = 4 * q + e;
            if (ai < A) {
                const float mu = m[row * sm + ai], sg = mu * 0.f + a.std[ai];
                const float act = mu + sg * z[e], d = act - mu;
                a.actions[env * a.actions_stride + ai] = act;
                a.mu[env * a.mu_stride + ai] = mu;
                a.sigma[env * a.sigma_stride + ai] = sg;
                m[row * sm + ai] = -(d * d) / (2.0f * (sg * sg)) - logf(sg) - 0.9189385332046727f;     // torch.distributions.Normal.log_prob
            }
        }
    }
    __syncthreads();
    for (int row = threadIdx.x; row < rows; row += kThreads) {
        float lp = 0.f;
        for (int ai = 0; ai < A; ai++) lp += m[row * sm + ai];
        a.log_prob[((size_t)row0 + row) * a.log_prob_stride] = lp;
    }
}

// behind the act launch on the same stream: no workgroup of the act launch writes the cell it reads
__global__ void policy_counter_kernel(unsigned *counter) {
    if (threadIdx.x == 0) counter[0] = counter[0] + 1u;
}

// the stand-alone reset(dones): tensor blockIdx.y of up to four (h and c of both memories), one lane per element; plain vector stores
struct KReset {
    float *t[4];
    long long len[4];                    // n_layers * N * H
    int H[4];
    const uint8_t *mask;
    int N;
};
__global__ __launch_bounds__(256) void policy_reset_kernel(KReset a) {
    float *t = a.t[blockIdx.y];
    const long long len = a.len[blockIdx.y], per = (long long)a.N * a.H[blockIdx.y];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (long long)gridDim.x * blockDim.x) {
        const int env = (int)((i % per) / a.H[blockIdx.y]);
        if (!a.mask || a.mask[env]) t[i] = 0.f;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static int lds_stride(int w) { return ((((w + 3) & ~3) - 4 + 63) / 64) * 64 + 4; }

// false with the refusal in `err`
static bool check_chain(const LgPolicyChain &c, const char *name, int first_in, std::string &err, bool behind_memory = false) {
    if (c.n_layers < 1 || c.n_layers > LG_POLICY_MAX_LAYERS) { err = std::string(name) + ": 1 .. 4 layers"; return false; }
    if (!behind_memory && (!c.input || c.in_width < 1 || c.in_stride < c.in_width)) { err = std::string(name) + ": null input, width < 1 or stride < width"; return false; }
    int w = first_in;
    for (int i = 0; i < c.n_layers; i++) {
        const LgPolicyLayer &l = c.layer[i];
        if (!l.weight || !l.bias) { err = std::string(name) + ": null weight or bias in layer " + std::to_string(i); return false; }
        if (l.n_in < 1 || l.n_in > LG_POLICY_MAX_WIDTH || l.n_out < 1 || l.n_out > LG_POLICY_MAX_WIDTH) {
            err = std::string(name) + ": layer " + std::to_string(i) + " width outside [1, " + std::to_string(LG_POLICY_MAX_WIDTH) + "]";
            return false;
        }
        if (l.n_in != w) { err = std::string(name) + ": layer " + std::to_string(i) + " takes " + std::to_string(l.n_in) + " inputs, its input has " + std::to_string(w); return false; }
        w = l.n_out;
    }
    return true;
}

// false with the refusal in `err`; `states_only`: what lg_policy_reset reads (kind, n_layers, hidden, h, c)
static bool check_memory(const LgPolicyMemory &m, const char *name, bool states_only, std::string &err) {
    const std::string n(name);
    if (m.kind != LG_POLICY_LSTM && m.kind != LG_POLICY_GRU) { err = n + ": unknown kind " + std::to_string(m.kind) + " (1 LSTM, 2 GRU)"; return false; }
    if (m.n_layers < 1 || m.n_layers > LG_POLICY_MAX_RNN_LAYERS) { err = n + ": 1 .. " + std::to_string(LG_POLICY_MAX_RNN_LAYERS) + " rnn layers"; return false; }
    if (m.hidden < 1 || m.hidden > LG_POLICY_MAX_RNN_HIDDEN) { err = n + ": hidden size outside [1, " + std::to_string(LG_POLICY_MAX_RNN_HIDDEN) + "]"; return false; }
    if (!m.h) { err = n + ": null state h"; return false; }
    if (m.kind == LG_POLICY_LSTM && !m.c) { err = n + ": an LSTM without its cell state c"; return false; }
    if (m.kind == LG_POLICY_GRU && (m.c || m.c_prev_out)) { err = n + ": a GRU has no cell state (c / c_prev_out given)"; return false; }
    if (states_only) return true;
    if (!m.input || m.in_width < 1 || m.in_width > LG_POLICY_MAX_WIDTH || m.in_stride < m.in_width) { err = n + ": null input, width outside [1, " + std::to_string(LG_POLICY_MAX_WIDTH) + "] or stride < width"; return false; }
    for (int k = 0; k < m.n_layers; k++) {
        const LgPolicyRnnLayer &l = m.layer[k];
        if (!l.weight_ih || !l.weight_hh || !l.bias_ih || !l.bias_hh) { err = n + ": null weight or bias in rnn layer " + std::to_string(k); return false; }
    }
    return true;
}

// a sequence while `plan` builds it (host only): `pack` copies what the kernel needs into KArgs
struct PSeq {
    const float *in;
    int in_w, in_stride, n_layers, epilogue, n_act, row_begin, row_end, reparam_after, mem;
    int stride[kMaxSeqLayers + 1];      // LDS row stride of activation i; activation i lives in buffer i & 1
    KLayer l[kMaxSeqLayers];
};

static void start_seq(PSeq &s, const LgPolicyChain &first, int row_begin, int row_end) {
    s.in = first.input; s.in_w = first.in_width; s.in_stride = first.in_stride;
    s.stride[0] = lds_stride(s.in_w);
    s.n_act = 1; s.row_begin = row_begin; s.row_end = row_end; s.reparam_after = -1; s.mem = -1;
}

// one more layer reading the newest activation; `new_act`: it opens a new activation of width `act_w` (otherwise it shares the newest
// one with the layer before it, at column `out_col`)
static KLayer &put_layer(PSeq &s, const float *W, const float *b, int K, int M, int elu, bool new_act, int act_w, int out_col) {
    KLayer &L = s.l[s.n_layers++];
    L = KLayer{};
    L.W = W; L.b = b; L.K = K; L.M = M; L.elu = elu; L.out_col = out_col;
    if (new_act) { s.stride[s.n_act] = lds_stride(act_w); s.n_act++; }
    L.src = s.n_act - 2; L.dst = s.n_act - 1;
    return L;
}

// a sequence that starts with memory `m` (KArgs::mem[slot]): per rnn layer its gate layers; the cell leaves h' in columns [0, H) of the
// gate activation, which the next rnn layer (with its own h_prev behind the padded h') or the chain reads
static void start_memory_seq(PSeq &s, const LgPolicyMemory &m, KMem &km, int slot, int N) {
    const int H = m.hidden, lstm = m.kind == LG_POLICY_LSTM;
    const int gw = 4 * H > ((H + 3) & ~3) + H ? 4 * H : ((H + 3) & ~3) + H;      // the gates, or the next layer's [h' | h_prev] (H = 1)
    s.in = m.input; s.in_w = m.in_width; s.in_stride = m.in_stride;
    s.stride[0] = lds_stride(((m.in_width + 3) & ~3) + H);
    s.n_act = 1; s.row_begin = 0; s.row_end = N; s.reparam_after = -1; s.mem = slot;
    km = KMem{};
    km.h = m.h; km.c = m.c; km.h_prev_out = m.h_prev_out; km.c_prev_out = m.c_prev_out; km.mask = m.reset_mask;
    km.kind = m.kind; km.n_layers = m.n_layers; km.H = H;
    int in = m.in_width;
    for (int k = 0; k < m.n_layers; k++) {
        const LgPolicyRnnLayer &l = m.layer[k];
        const int xc = (in + 3) & ~3;
        km.x_col[k] = xc;
        KLayer &g = put_layer(s, l.weight_ih, l.bias_ih, in, lstm ? 4 * H : 2 * H, 0, true, gw, 0);     // LSTM: all four gates; GRU: r, z
        g.W2 = l.weight_hh; g.b2 = l.bias_hh; g.K2 = H; g.src_col2 = xc;
        if (!lstm) {
            put_layer(s, l.weight_ih + (size_t)2 * H * in, l.bias_ih + 2 * H, in, H, 0, false, 0, 2 * H);                       // n_x
            put_layer(s, l.weight_hh + (size_t)2 * H * H, l.bias_hh + 2 * H, H, H, 0, false, 0, 3 * H).src_col = xc;         // n_h
        }
        km.cell_after[k] = s.n_layers - 1;
        in = H;
    }
}

static void put_chain(PSeq &s, const LgPolicyChain &c, float *gout, int gstride) {
    for (int i = 0; i < c.n_layers; i++) {
        KLayer &L = put_layer(s, c.layer[i].weight, c.layer[i].bias, c.layer[i].n_in, c.layer[i].n_out, c.layer[i].elu, true, c.layer[i].n_out, 0);
        if (i == c.n_layers - 1) { L.gout = gout; L.gstride = gstride; }
    }
}

// a leading chain whose output lands behind the features in the actor's input activation (the EE / TS concatenation)
static void put_leading(PSeq &s, const LgPolicyChain &e, const LgPolicyChain &ac, int actor_in) {
    put_chain(s, e, e.out, e.out_stride);
    KLayer &L = s.l[s.n_layers - 1];
    L.out_col = ac.in_width; L.cat_src = ac.input; L.cat_w = ac.in_width; L.cat_stride = ac.in_stride;
    s.stride[s.n_act - 1] = lds_stride(actor_in);
}

// the launch plan of one call: which sequences run, their LDS strides, the row tile.  Returns 0 and fills k / n_y / lds_bytes, or the refusal.
static int plan(const LgPolicyArgs *p, const LgPolicyMemory *mem_a, const LgPolicyMemory *mem_c, KArgs &k, int &n_y, size_t &lds_bytes) {
    if (!p) return lg_fail_msg("lg_policy_act: null descriptor");
    if (p->n_envs < 1) return lg_fail_msg("lg_policy_act: n_envs < 1");
    const bool values_only = p->flags & LG_POLICY_VALUES_ONLY, determ = p->flags & LG_POLICY_DETERMINISTIC;
    if ((p->flags & ~3u) || (values_only && determ)) return lg_fail_msg("lg_policy_act: bad flags");
    const bool has_est = p->estimator.n_layers != 0, has_critic = p->critic.n_layers != 0;
    const bool has_b = p->encoder_b.n_layers != 0;
    const LgPolicyHead &h = p->head;
    const bool has_head = h.H != 0 || h.L != 0 || h.E != 0;
    const bool has_mem_a = mem_a && mem_a->kind != 0, has_mem_c = mem_c && mem_c->kind != 0;
    const int N = p->n_envs;
    std::string err;
    k = KArgs{};
    PSeq seq[3] = {};
    int n_seq = 0, n_policy = 0;
    if (!values_only) {
        const LgPolicyChain &e = p->estimator, &ac = p->actor, &eb = p->encoder_b;
        if (has_mem_a) {
            if (has_est || has_b || has_head) return lg_fail_msg("lg_policy_act: memory_a together with the estimator, encoder_b or the VAE head");
            if (!check_memory(*mem_a, "lg_policy_act: memory_a", false, err)) return lg_fail_msg(err);
        }
        if (p->n_split < 0 || p->n_split > N) return lg_fail_msg("lg_policy_act: n_split outside [0, n_envs]");
        if (has_b && !p->has_split) return lg_fail_msg("lg_policy_act: encoder_b without n_split (has_split is not set)");
        if (!has_b && (p->has_split || p->n_split)) return lg_fail_msg("lg_policy_act: n_split without encoder_b");
        if (has_b && !has_est) return lg_fail_msg("lg_policy_act: encoder_b without an estimator chain for the rows below the split");
        if (has_b && has_head) return lg_fail_msg("lg_policy_act: the VAE head and encoder_b exclude each other");
        if (has_head && !has_est) return lg_fail_msg("lg_policy_act: the VAE head needs the estimator chain as its encoder");
        int actor_in = ac.in_width;
        if (has_mem_a) actor_in = mem_a->hidden;
        if (has_est) {
            if (!check_chain(e, "lg_policy_act: estimator", e.in_width, err)) return lg_fail_msg(err);
            const int e_out = e.layer[e.n_layers - 1].n_out;
            if (e.out && e.out_stride < e_out) return lg_fail_msg("lg_policy_act: estimator out_stride < width");
            if (has_head) {
                if (h.L < 1 || h.E < 1) return lg_fail_msg("lg_policy_act: head widths L and E must be >= 1");
                if (h.H != e_out) return lg_fail_msg("lg_policy_act: head takes H = " + std::to_string(h.H) + " inputs, the estimator chain gives " + std::to_string(e_out));
                if (!h.latent_mu_w || !h.latent_mu_b || !h.latent_var_w || !h.latent_var_b || !h.vel_mu_w || !h.vel_mu_b || !h.vel_var_w || !h.vel_var_b)
                    return lg_fail_msg("lg_policy_act: null head weight or bias");
                if (!(h.logvar_clip >= 0.f)) return lg_fail_msg("lg_policy_act: logvar_clip must be >= 0");
                if ((long long)ac.in_width + h.L + h.E > LG_POLICY_MAX_WIDTH) return lg_fail_msg("lg_policy_act: actor input (obs, latent) wider than 2048");
                actor_in += h.L + h.E;
                if (h.latent_out && h.latent_stride < h.L + h.E) return lg_fail_msg("lg_policy_act: latent_stride < L + E");
                if (h.params_out && h.params_stride < 2 * (h.L + h.E)) return lg_fail_msg("lg_policy_act: params_stride < 2 L + 2 E");
                if (!determ && (h.noise ? h.noise_stride < h.L + h.E : !p->counter))
                    return lg_fail_msg("lg_policy_act: head noise_stride < L + E, or neither latent noise nor a Philox counter");
            } else {
                actor_in += e_out;
                if (actor_in > LG_POLICY_MAX_WIDTH) return lg_fail_msg("lg_policy_act: actor input (features, estimator output) wider than 2048");
            }
        }
        if (has_b) {
            if (!check_chain(eb, "lg_policy_act: encoder_b", eb.in_width, err)) return lg_fail_msg(err);
            const int b_out = eb.layer[eb.n_layers - 1].n_out, e_out = e.layer[e.n_layers - 1].n_out;
            if (b_out != e_out) return lg_fail_msg("lg_policy_act: the group chains end at different widths (" + std::to_string(e_out) + ", " + std::to_string(b_out) + ")");
            if (eb.out && eb.out_stride < b_out) return lg_fail_msg("lg_policy_act: encoder_b out_stride < width");
        }
        if (!check_chain(ac, "lg_policy_act: actor", actor_in, err, has_mem_a)) return lg_fail_msg(err);
        const int A = ac.layer[ac.n_layers - 1].n_out;
        if (!p->mu || p->mu_stride < A) return lg_fail_msg("lg_policy_act: null mu or mu_stride < actions");
        if (!determ) {
            if (!p->actions || !p->sigma || !p->log_prob || !p->std) return lg_fail_msg("lg_policy_act: null actions / sigma / log_prob / std");
            if (p->actions_stride < A || p->sigma_stride < A || p->log_prob_stride < 1) return lg_fail_msg("lg_policy_act: a destination stride below its width");
            if (p->noise ? p->noise_stride < A : !p->counter) return lg_fail_msg("lg_policy_act: noise_stride < actions, or neither noise nor a Philox counter");
        }
        if (p->clip_on && !(p->clip_actions >= 0.f)) return lg_fail_msg("lg_policy_act: clip_actions must be >= 0");
        const int split = has_b ? p->n_split : N;
        for (int g = 0; g < (has_b ? 2 : 1); g++) {
            PSeq &s = seq[n_seq++];
            const LgPolicyChain &lead = g ? eb : e;
            if (has_mem_a) start_memory_seq(s, *mem_a, k.mem[0], 0, N);
            else start_seq(s, has_est ? lead : ac, g ? split : 0, g ? N : split);
            if (has_head) {
                put_chain(s, e, e.out, e.out_stride);
                const int L = h.L, E = h.E, PW = 2 * (L + E);
                const float *W[4] = {h.latent_mu_w, h.latent_var_w, h.vel_mu_w, h.vel_var_w}, *B[4] = {h.latent_mu_b, h.latent_var_b, h.vel_mu_b, h.vel_var_b};
                const int M[4] = {L, L, E, E}, col[4] = {0, L, 2 * L, 2 * L + E};
                for (int i = 0; i < 4; i++) {
                    KLayer &hl = put_layer(s, W[i], B[i], h.H, M[i], 0, i == 0, PW, col[i]);
                    if (i & 1) { hl.clip_on = 1; hl.clip = h.logvar_clip; }
                    if (h.params_out) { hl.gout = h.params_out + col[i]; hl.gstride = h.params_stride; }
                }
                s.reparam_after = s.n_layers - 1;
                s.stride[s.n_act] = k.head.sx = lds_stride(actor_in);       // [obs | z | vel], formed by `reparam` in the other buffer
                s.n_act++;
            } else if (has_est) {
                put_leading(s, lead, ac, actor_in);
            }
            put_chain(s, ac, determ ? p->mu : nullptr, p->mu_stride);
            KLayer &last = s.l[s.n_layers - 1];
            last.clip_on = p->clip_on != 0; last.clip = p->clip_actions;
            s.epilogue = !determ;
        }
        n_policy = n_seq;
        k.A = A;
        if (has_head) {
            KHead &d = k.head;
            d.obs = ac.input; d.obs_stride = ac.in_stride; d.F = ac.in_width; d.L = h.L; d.E = h.E; d.determ = determ;
            d.noise = determ ? nullptr : h.noise; d.noise_stride = h.noise_stride;
            d.latent_out = h.latent_out; d.latent_stride = h.latent_stride;
            d.dbg_uniform = (determ || h.noise) ? nullptr : h.dbg_latent_uniform;
        }
    }
    if (has_critic && !determ) {
        const LgPolicyChain &c = p->critic;
        if (has_mem_c && !check_memory(*mem_c, "lg_policy_act: memory_c", false, err)) return lg_fail_msg(err);
        if (!check_chain(c, "lg_policy_act: critic", has_mem_c ? mem_c->hidden : c.in_width, err, has_mem_c)) return lg_fail_msg(err);
        if (!c.out || c.out_stride < c.layer[c.n_layers - 1].n_out) return lg_fail_msg("lg_policy_act: null values or stride < width");
        PSeq &s = seq[n_seq++];
        if (has_mem_c) start_memory_seq(s, *mem_c, k.mem[1], 1, N);
        else start_seq(s, c, 0, N);
        put_chain(s, c, c.out, c.out_stride);
    } else if (values_only) {
        return lg_fail_msg("lg_policy_act: values_only without a critic");
    }
    if (values_only) n_policy = 1;                       // the critic alone: it is the blockIdx.y = 0 run
    k.N = N;
    k.std = p->std; k.noise = p->noise; k.actions = p->actions; k.mu = p->mu; k.sigma = p->sigma; k.log_prob = p->log_prob;
    k.dbg_uniform = p->dbg_uniform; k.counter = p->counter;
    k.noise_stride = p->noise_stride; k.actions_stride = p->actions_stride; k.mu_stride = p->mu_stride; k.sigma_stride = p->sigma_stride;
    k.log_prob_stride = p->log_prob_stride;
    k.seed_lo = (unsigned)p->seed; k.seed_hi = (unsigned)(p->seed >> 32);
    k.seq_y1 = n_policy;
    n_y = n_seq > n_policy ? 2 : 1;
    int n_l = 0;                                         // pack: each sequence's layers, with their two LDS strides, into the shared array
    for (int q = 0; q < n_seq; q++) {
        const PSeq &s = seq[q];
        k.seq[q] = KSeq{s.in, s.in_w, s.in_stride, s.stride[0], n_l, s.n_layers, s.epilogue, s.row_begin, s.row_end, s.reparam_after, s.mem};
        for (int i = 0; i < s.n_layers; i++) {
            KLayer &L = k.l[n_l++] = s.l[i];
            L.sa = s.stride[L.src]; L.so = s.stride[L.dst];
        }
    }
    // buffer 0 holds the even activations, buffer 1 the odd ones: each as wide as its widest
    int w[2] = {0, 0};
    for (int q = 0; q < n_seq; q++)
        for (int i = 0; i < seq[q].n_act; i++)
            if (seq[q].stride[i] > w[i & 1]) w[i & 1] = seq[q].stride[i];
    for (int R = 32; R >= 8; R >>= 1) {
        lds_bytes = (size_t)R * (w[0] + w[1]) * sizeof(float);
        if (lds_bytes <= kLdsBytes) {
            k.R = R; k.q_off = R * w[0];
            k.tiles_a = (k.seq[0].row_end - k.seq[0].row_begin + R - 1) / R;
            return 0;
        }
    }
    return lg_fail_msg("lg_policy_act: an 8-row tile of these widths does not fit the LDS");
}

// tiles along x: the policy's one or two runs, or the critic's if that is longer
static unsigned grid_x(const KArgs &k) {
    int t = k.tiles_a;
    if (k.seq_y1 == 2) t += (k.seq[1].row_end - k.seq[1].row_begin + k.R - 1) / k.R;
    const int all = (k.N + k.R - 1) / k.R;
    return (unsigned)(t > all ? t : all);
}

extern "C" int lg_policy_row_tile(const LgPolicyArgs *args) {
    KArgs k; int n_y; size_t lds;
    return plan(args, nullptr, nullptr, k, n_y, lds) ? 0 : k.R;
}

extern "C" int lg_policy_row_tile_recurrent(const LgPolicyRecurrentArgs *args) {
    KArgs k; int n_y; size_t lds;
    if (!args) { lg_fail_msg("lg_policy_act: null descriptor"); return 0; }
    return plan(&args->args, &args->memory_a, &args->memory_c, k, n_y, lds) ? 0 : k.R;
}

static int act(const LgPolicyArgs *args, const LgPolicyMemory *mem_a, const LgPolicyMemory *mem_c, void *stream) {
    KArgs k; int n_y; size_t lds;
    if (plan(args, mem_a, mem_c, k, n_y, lds)) return 1;
    // once per device and kernel: dynamic LDS above 64 KB has to be asked for.  Not synchronised on purpose: two threads racing here
    // both set the same attribute to the same value, which is harmless.
    static bool lds_raised[64][2];
    const int rb = k.R == 32;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return lg_fail_msg("lg_policy_act: no current HIP device");
    if (!lds_raised[dev][rb]) {
        const hipError_t e = rb ? hipFuncSetAttribute((const void *)policy_act_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes)
                                : hipFuncSetAttribute((const void *)policy_act_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes);
        if (e != hipSuccess) return lg_fail_msg(std::string("lg_policy_act: hipFuncSetAttribute: ") + hipGetErrorString(e));
        lds_raised[dev][rb] = true;
    }
    const dim3 grid(grid_x(k), (unsigned)n_y);
    if (rb) hipLaunchKernelGGL(policy_act_kernel<2>, grid, dim3(kThreads), lds, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(policy_act_kernel<1>, grid, dim3(kThreads), lds, (hipStream_t)stream, k);
    if (k.seq[0].epilogue && (!k.noise || (k.seq[0].reparam_after >= 0 && !k.head.noise))) hipLaunchKernelGGL(policy_counter_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, args->counter);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : lg_fail_msg(std::string("lg_policy_act: ") + hipGetErrorString(e));
}

extern "C" int lg_policy_act(const LgPolicyArgs *args, void *stream) { return act(args, nullptr, nullptr, stream); }

extern "C" int lg_policy_act_recurrent(const LgPolicyRecurrentArgs *args, void *stream) {
    if (!args) return lg_fail_msg("lg_policy_act: null descriptor");
    return act(&args->args, &args->memory_a, &args->memory_c, stream);
}

extern "C" int lg_policy_reset(const LgPolicyRecurrentArgs *args, const uint8_t *mask, void *stream) {
    if (!args) return lg_fail_msg("lg_policy_reset: null descriptor");
    const int n_envs = args->args.n_envs;
    if (n_envs < 1) return lg_fail_msg("lg_policy_reset: n_envs < 1");
    KReset k = {};
    int n = 0;
    long long longest = 0;
    std::string err;
    const LgPolicyMemory *mem[2] = {&args->memory_a, &args->memory_c};
    const char *name[2] = {"lg_policy_reset: memory_a", "lg_policy_reset: memory_c"};
    for (int i = 0; i < 2; i++) {
        const LgPolicyMemory &m = *mem[i];
        if (m.kind == 0) continue;
        if (!check_memory(m, name[i], true, err)) return lg_fail_msg(err);
        float *t[2] = {m.h, m.c};
        for (int j = 0; j < 2; j++)
            if (t[j]) {
                k.t[n] = t[j]; k.H[n] = m.hidden; k.len[n] = (long long)m.n_layers * n_envs * m.hidden;
                if (k.len[n] > longest) longest = k.len[n];
                n++;
            }
    }
    if (n == 0) return lg_fail_msg("lg_policy_reset: the descriptor has no memory");
    k.mask = mask; k.N = n_envs;
    long long blocks = (longest + 255) / 256;
    if (blocks > 4096) blocks = 4096;                    // grid-stride behind that
    hipLaunchKernelGGL(policy_reset_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, (hipStream_t)stream, k);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : lg_fail_msg(std::string("lg_policy_reset: ") + hipGetErrorString(e));
}

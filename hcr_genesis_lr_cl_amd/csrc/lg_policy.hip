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

static const int kThreads = 256, kWaves = 4, kMaxSeqLayers = 2 * LG_POLICY_MAX_LAYERS;
static const size_t kLdsBytes = 160u * 1024u;      // gfx950: 160 KB per workgroup

struct KLayer {
    const float *W, *b;
    float *gout;            // global destination of this layer's output (NULL: LDS only)
    const float *cat_src;   // rows copied into columns [0, cat_w) of the output activation (the EE concatenation)
    int K, M, elu, clip_on;
    float clip;
    int out_col, gstride, cat_w, cat_stride;
};
struct KSeq {
    const float *in;
    int in_w, in_stride, n_layers, epilogue;
    int stride[kMaxSeqLayers + 1];      // LDS row stride of activation i; activation i lives in buffer i & 1
    KLayer l[kMaxSeqLayers];
};
struct KArgs {
    KSeq seq[2];
    int N, R, q_off, A;
    const float *std, *noise;
    float *actions, *mu, *sigma, *log_prob, *dbg_uniform;
    const unsigned *counter;
    int noise_stride, actions_stride, mu_stride, sigma_stride, log_prob_stride;
    unsigned seed_lo, seed_hi;
};

// one layer for the workgroup's row tile: nxt[row][out_col + n] = act(b[n] + sum_k W[n][k] cur[row][k])
template <int RB, int NT>
__device__ __forceinline__ void layer_tile(const KLayer &L, const lds_f *cur, int sa, lds_f *nxt, int so, int R, int rows, int row0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, h = lane >> 4;
    const int K = L.K, M = L.M, tiles = (M + 15) >> 4;
    for (int tb = wave * NT; tb < tiles; tb += kWaves * NT) {
        f4 acc[RB][NT];
        const float *wp[NT];
        const lds_f *xp[RB];
#pragma unroll
        for (int i = 0; i < NT; i++) {
            const int n = min((tb + i) * 16 + r, M - 1);
            wp[i] = L.W + (size_t)n * K + 4 * h;
#pragma unroll
            for (int j = 0; j < RB; j++) acc[j][i] = (f4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < RB; j++) xp[j] = cur + min(j * 16 + r, R - 1) * sa + 4 * h;
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
#pragma unroll
        for (int i = 0; i < NT; i++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int n = (tb + i) * 16 + 4 * h + e;
                if (n < M) {
                    const float bias = L.b[n];
#pragma unroll
                    for (int j = 0; j < RB; j++) {
                        const int row = j * 16 + r;
                        float v = acc[j][i][e] + bias;
                        if (L.elu) v = v > 0.f ? v : expm1f(v);
                        if (L.clip_on) v = fminf(fmaxf(v, -L.clip), L.clip);
                        if (row < R) nxt[row * so + L.out_col + n] = v;
                        if (L.gout && row < rows) L.gout[(size_t)(row0 + row) * L.gstride + n] = v;
                    }
                }
            }
    }
}

template <int RB> __device__ __forceinline__ void layer(const KLayer &L, const lds_f *cur, int sa, lds_f *nxt, int so, int R, int rows, int row0) {
    const int per_wave = (((L.M + 15) >> 4) + kWaves - 1) / kWaves;
    if (per_wave >= 4) layer_tile<RB, 4>(L, cur, sa, nxt, so, R, rows, row0);
    else if (per_wave >= 2) layer_tile<RB, 2>(L, cur, sa, nxt, so, R, rows, row0);
    else layer_tile<RB, 1>(L, cur, sa, nxt, so, R, rows, row0);
}

// rows [0, R) x columns [0, w) of a global (N, w) matrix into an LDS activation; rows behind N read as zero
__device__ __forceinline__ void stage_rows(const float *src, int w, int stride, lds_f *dst, int sd, int R, int rows, int row0) {
    for (int i = threadIdx.x; i < R * w; i += kThreads) {
        const int row = i / w, c = i - row * w;
        dst[row * sd + c] = row < rows ? src[(size_t)(row0 + row) * stride + c] : 0.f;
    }
}

template <int RB> __global__ __launch_bounds__(256) void policy_act_kernel(KArgs a) {
    extern __shared__ __align__(16) float lds[];
    const KSeq &s = a.seq[blockIdx.y];
    const int R = a.R, row0 = blockIdx.x * R, rows = min(R, a.N - row0);
    lds_f *buf[2] = {(lds_f *)lds, (lds_f *)lds + a.q_off};
    stage_rows(s.in, s.in_w, s.in_stride, buf[0], s.stride[0], R, rows, row0);
    __syncthreads();
    for (int li = 0; li < s.n_layers; li++) {
        const KLayer &L = s.l[li];
        lds_f *nxt = buf[(li + 1) & 1];
        layer<RB>(L, buf[li & 1], s.stride[li], nxt, s.stride[li + 1], R, rows, row0);
        if (L.cat_src) stage_rows(L.cat_src, L.cat_w, L.cat_stride, nxt, s.stride[li + 1], R, rows, row0);
        __syncthreads();
    }
    if (!s.epilogue) return;
    // sampling epilogue: one lane per (env row, action quad); the log-prob terms replace mu in LDS, then one lane per row sums them in order
    lds_f *m = buf[s.n_layers & 1];
    const int sm = s.stride[s.n_layers], A = a.A, Q = (A + 3) >> 2;
    for (int t = threadIdx.x; t < R * Q; t += kThreads) {
        const int row = t / Q, q = t - row * Q;
        if (row >= rows) continue;
        const size_t env = (size_t)row0 + row;
        float z[4];
        if (a.noise) {
#pragma unroll
            for (int e = 0; e < 4; e++) z[e] = 4 * q + e < A ? a.noise[env * a.noise_stride + 4 * q + e] : 0.f;
        } else {
            const U4 c = {(unsigned)env, (unsigned)q, a.counter[0], LG_POLICY_STREAM_TAG};
            const U4 x = philox4x32_10(c, a.seed_lo, a.seed_hi);
            const float u[4] = {u01(x.x), u01(x.y), u01(x.z), u01(x.w)};
#pragma unroll
            for (int p = 0; p < 2; p++) {
                const float rad = sqrtf(-2.0f * logf(1.0f - u[2 * p])), th = 6.283185307179586f * u[2 * p + 1];
                z[2 * p] = rad * cosf(th);
                z[2 * p + 1] = rad * sinf(th);
            }
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

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static int lds_stride(int w) { return ((((w + 3) & ~3) - 4 + 63) / 64) * 64 + 4; }

// false with the refusal in `err`
static bool check_chain(const LgPolicyChain &c, const char *name, int first_in, std::string &err) {
    if (c.n_layers < 1 || c.n_layers > LG_POLICY_MAX_LAYERS) { err = std::string(name) + ": 1 .. 4 layers"; return false; }
    if (!c.input || c.in_width < 1 || c.in_stride < c.in_width) { err = std::string(name) + ": null input, width < 1 or stride < width"; return false; }
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

static void put_chain(KSeq &s, const LgPolicyChain &c, float *gout, int gstride) {
    for (int i = 0; i < c.n_layers; i++) {
        KLayer &L = s.l[s.n_layers];
        L = KLayer{};
        L.W = c.layer[i].weight; L.b = c.layer[i].bias; L.K = c.layer[i].n_in; L.M = c.layer[i].n_out; L.elu = c.layer[i].elu;
        if (i == c.n_layers - 1) { L.gout = gout; L.gstride = gstride; }
        s.stride[s.n_layers + 1] = lds_stride(L.M);
        s.n_layers++;
    }
}

// the launch plan of one call: which sequences run, their LDS strides, the row tile.  Returns 0 and fills k / n_seq / lds_bytes, or the refusal.
static int plan(const LgPolicyArgs *p, KArgs &k, int &n_seq, size_t &lds_bytes) {
    if (!p) return lg_fail_msg("lg_policy_act: null descriptor");
    if (p->n_envs < 1) return lg_fail_msg("lg_policy_act: n_envs < 1");
    const bool values_only = p->flags & LG_POLICY_VALUES_ONLY, determ = p->flags & LG_POLICY_DETERMINISTIC;
    if ((p->flags & ~3u) || (values_only && determ)) return lg_fail_msg("lg_policy_act: bad flags");
    const bool has_est = p->estimator.n_layers != 0, has_critic = p->critic.n_layers != 0;
    std::string err;
    k = KArgs{};
    n_seq = 0;
    if (!values_only) {
        const LgPolicyChain &e = p->estimator, &ac = p->actor;
        int actor_in = ac.in_width;
        if (has_est) {
            if (!check_chain(e, "lg_policy_act: estimator", e.in_width, err)) return lg_fail_msg(err);
            if (e.out && e.out_stride < e.layer[e.n_layers - 1].n_out) return lg_fail_msg("lg_policy_act: estimator out_stride < width");
            actor_in += e.layer[e.n_layers - 1].n_out;
            if (actor_in > LG_POLICY_MAX_WIDTH) return lg_fail_msg("lg_policy_act: actor input (features, estimator output) wider than 2048");
        }
        if (!check_chain(ac, "lg_policy_act: actor", actor_in, err)) return lg_fail_msg(err);
        const int A = ac.layer[ac.n_layers - 1].n_out;
        if (!p->mu || p->mu_stride < A) return lg_fail_msg("lg_policy_act: null mu or mu_stride < actions");
        if (!determ) {
            if (!p->actions || !p->sigma || !p->log_prob || !p->std) return lg_fail_msg("lg_policy_act: null actions / sigma / log_prob / std");
            if (p->actions_stride < A || p->sigma_stride < A || p->log_prob_stride < 1) return lg_fail_msg("lg_policy_act: a destination stride below its width");
            if (p->noise ? p->noise_stride < A : !p->counter) return lg_fail_msg("lg_policy_act: noise_stride < actions, or neither noise nor a Philox counter");
        }
        KSeq &s = k.seq[n_seq++];
        const LgPolicyChain &first = has_est ? e : ac;
        s.in = first.input; s.in_w = first.in_width; s.in_stride = first.in_stride;
        s.stride[0] = lds_stride(s.in_w);
        if (has_est) {
            put_chain(s, e, e.out, e.out_stride);
            KLayer &L = s.l[s.n_layers - 1];             // its output lands behind the features in the actor's input activation
            L.out_col = ac.in_width; L.cat_src = ac.input; L.cat_w = ac.in_width; L.cat_stride = ac.in_stride;
            s.stride[s.n_layers] = lds_stride(actor_in);
        }
        put_chain(s, ac, determ ? p->mu : nullptr, p->mu_stride);
        KLayer &last = s.l[s.n_layers - 1];
        last.clip_on = p->clip_on != 0; last.clip = p->clip_actions;
        if (last.clip_on && !(p->clip_actions >= 0.f)) return lg_fail_msg("lg_policy_act: clip_actions must be >= 0");
        s.epilogue = !determ;
        k.A = A;
    }
    if (has_critic && !determ) {
        const LgPolicyChain &c = p->critic;
        if (!check_chain(c, "lg_policy_act: critic", c.in_width, err)) return lg_fail_msg(err);
        if (!c.out || c.out_stride < c.layer[c.n_layers - 1].n_out) return lg_fail_msg("lg_policy_act: null values or stride < width");
        KSeq &s = k.seq[n_seq++];
        s.in = c.input; s.in_w = c.in_width; s.in_stride = c.in_stride;
        s.stride[0] = lds_stride(s.in_w);
        put_chain(s, c, c.out, c.out_stride);
    } else if (values_only) {
        return lg_fail_msg("lg_policy_act: values_only without a critic");
    }
    k.N = p->n_envs;
    k.std = p->std; k.noise = p->noise; k.actions = p->actions; k.mu = p->mu; k.sigma = p->sigma; k.log_prob = p->log_prob;
    k.dbg_uniform = p->dbg_uniform; k.counter = p->counter;
    k.noise_stride = p->noise_stride; k.actions_stride = p->actions_stride; k.mu_stride = p->mu_stride; k.sigma_stride = p->sigma_stride;
    k.log_prob_stride = p->log_prob_stride;
    k.seed_lo = (unsigned)p->seed; k.seed_hi = (unsigned)(p->seed >> 32);
    // buffer 0 holds the even activations, buffer 1 the odd ones: each as wide as its widest
    int w[2] = {0, 0};
    for (int q = 0; q < n_seq; q++)
        for (int i = 0; i <= k.seq[q].n_layers; i++)
            if (k.seq[q].stride[i] > w[i & 1]) w[i & 1] = k.seq[q].stride[i];
    for (int R = 32; R >= 8; R >>= 1) {
        lds_bytes = (size_t)R * (w[0] + w[1]) * sizeof(float);
        if (lds_bytes <= kLdsBytes) {
            k.R = R; k.q_off = R * w[0];
            return 0;
        }
    }
    return lg_fail_msg("lg_policy_act: an 8-row tile of these widths does not fit the LDS");
}

extern "C" int lg_policy_row_tile(const LgPolicyArgs *args) {
    KArgs k; int n_seq; size_t lds;
    return plan(args, k, n_seq, lds) ? 0 : k.R;
}

extern "C" int lg_policy_act(const LgPolicyArgs *args, void *stream) {
    KArgs k; int n_seq; size_t lds;
    if (plan(args, k, n_seq, lds)) return 1;
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
    const dim3 grid((unsigned)((k.N + k.R - 1) / k.R), (unsigned)n_seq);
    if (rb) hipLaunchKernelGGL(policy_act_kernel<2>, grid, dim3(kThreads), lds, (hipStream_t)stream, k);
    else hipLaunchKernelGGL(policy_act_kernel<1>, grid, dim3(kThreads), lds, (hipStream_t)stream, k);
    if (k.seq[0].epilogue && !k.noise) hipLaunchKernelGGL(policy_counter_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, args->counter);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : lg_fail_msg(std::string("lg_policy_act: ") + hipGetErrorString(e));
}

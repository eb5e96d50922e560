// lg_train_tiles.h -- the layer routines of the fused learner passes, shared by lg_train.hip (the plain ActorCritic, include/lgtrain.h),
// lg_train_ee.hip (ActorCriticEE, include/lgtrainee.h) and lg_train_ts.hip (ActorCriticTS, include/lgtraints.h): the row-tile forward and
// input-gradient layers, the weight-gradient wave, the combine of the slice partials, and the host's LDS stride and slice rules.  What a
// pass builds from them (chains, loss, plan, bind, launch) is lg_train_pass.h, which includes this header.  The MFMA operand layouts are
// described at the top of lg_train.hip.  Everything here is inlined into the kernels of the including unit; nothing is exported.
#ifndef LG_TRAIN_TILES_H
#define LG_TRAIN_TILES_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/lgtrain.h"

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // weight rows start wherever in * 4 bytes puts them
typedef __attribute__((address_space(3))) float lds_f;
typedef __attribute__((address_space(3))) f4 lds_f4;

static const int kThreads = 256, kWaves = 4, kMaxL = LG_POLICY_MAX_LAYERS;
static const size_t kLdsBytes = 160u * 1024u;      // gfx950: 160 KB per workgroup
static const int kWT = LG_TRAIN_WG_TILE / 16;      // accumulator tiles per side of a weight-gradient wave

struct TLayer {
    const float *W, *b;
    float *gW, *gb;
    int K, M, elu;
    int sa, so;                 // LDS row strides of the layer's input and output activation
    int S, rps;                 // batch slices of the weight gradient and rows per slice
    int tiles_k, job0;          // 64-wide tiles along the input index; first job of this layer in the weight-gradient launch
    long long h_off, g_off, p_off;
};
struct TChain {
    const float *in;            // the chain's input rows
    const float *gin;           // grad_mu / grad_values
    float *out;                 // mu / values
    int in_stride, gin_stride, out_stride, n_layers;
    TLayer l[kMaxL];
};

// rows [0, R) x columns [0, w) of a global (N, w) matrix into an LDS activation, coalesced over the columns (16-byte accesses where the
// width, the stride and the base allow); rows behind `rows` read as zero
__device__ __forceinline__ void stage_rows(const float *src, int w, int stride, lds_f *dst, int sd, int R, int rows, int row0) {
    if (((w | stride) & 3) == 0 && ((uintptr_t)src & 15) == 0) {
        const int q = w >> 2;
        for (int i = threadIdx.x; i < R * q; i += kThreads) {
            const int row = i / q, c = (i - row * q) * 4;
            *(lds_f4 *)(dst + row * sd + c) = row < rows ? *(const f4 *)(src + (size_t)(row0 + row) * stride + c) : (f4){0.f, 0.f, 0.f, 0.f};
        }
        return;
    }
    for (int i = threadIdx.x; i < R * w; i += kThreads) {
        const int row = i / w, c = i - row * w;
        dst[row * sd + c] = row < rows ? src[(size_t)(row0 + row) * stride + c] : 0.f;
    }
}

// the tile's rows [0, rows) x columns [0, w) of an LDS activation to a global (N, w) matrix, coalesced likewise.  The MFMA's result layout
// (a lane holds four neurons of ONE row) would store 4 bytes into 64 different rows per instruction; through the LDS tile a row is written
// as a run.
__device__ __forceinline__ void copy_out(const lds_f *src, int ss, float *dst, int w, int stride, int rows, int row0) {
    if (((w | stride) & 3) == 0 && ((uintptr_t)dst & 15) == 0) {
        const int q = w >> 2;
        for (int i = threadIdx.x; i < rows * q; i += kThreads) {
            const int row = i / q, c = (i - row * q) * 4;
            *(f4 *)(dst + (size_t)(row0 + row) * stride + c) = *(const lds_f4 *)(src + row * ss + c);
        }
        return;
    }
    for (int i = threadIdx.x; i < rows * w; i += kThreads) {
        const int row = i / w, c = i - row * w;
        dst[(size_t)(row0 + row) * stride + c] = src[row * ss + c];
    }
}

// forward layer for the workgroup's row tile: nxt[row][n] = act(b[n] + sum_k W[n][k] cur[row][k]), in LDS only
template <int RB, int NT>
__device__ __forceinline__ void fwd_tile(const TLayer &L, const lds_f *cur, lds_f *nxt, bool clip_on, float clip, int R) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, h = lane >> 4;
    const int M = L.M, K = L.K, sa = L.sa, so = L.so, tiles = (M + 15) >> 4;
    for (int tb = wave * NT; tb < tiles; tb += kWaves * NT) {
        f4 acc[RB][NT];
#pragma unroll
        for (int i = 0; i < NT; i++)
#pragma unroll
            for (int j = 0; j < RB; j++) acc[j][i] = (f4){0.f, 0.f, 0.f, 0.f};
        const float *wp[NT];
        const lds_f *xp[RB];
#pragma unroll
        for (int i = 0; i < NT; i++) wp[i] = L.W + (size_t)min((tb + i) * 16 + r, M - 1) * K + 4 * h;
#pragma unroll
        for (int j = 0; j < RB; j++) xp[j] = cur + min(j * 16 + r, R - 1) * sa + 4 * h;
        int k0 = 0;
        f4 an[NT], bn[RB];                       // the next chunk's fragments, in flight while this chunk's MFMAs issue
        if (K >= 16) {
#pragma unroll
            for (int i = 0; i < NT; i++) an[i] = *(const f4u *)(wp[i]);
#pragma unroll
            for (int j = 0; j < RB; j++) bn[j] = *(const lds_f4 *)(xp[j]);
        }
        for (; k0 + 16 <= K; k0 += 16) {
            f4 av[NT], bv[RB];
#pragma unroll
            for (int i = 0; i < NT; i++) av[i] = an[i];
#pragma unroll
            for (int j = 0; j < RB; j++) bv[j] = bn[j];
            if (k0 + 32 <= K) {
#pragma unroll
                for (int i = 0; i < NT; i++) an[i] = *(const f4u *)(wp[i] + k0 + 16);
#pragma unroll
                for (int j = 0; j < RB; j++) bn[j] = *(const lds_f4 *)(xp[j] + k0 + 16);
            }
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
                for (int j = 0; j < RB; j++)
#pragma unroll
                    for (int i = 0; i < NT; i++) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][e], bv[j][e], acc[j][i], 0, 0, 0);
        }
        if (k0 < K) {                            // K tail: element-wise, zeros behind K on both operands
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
                        if (clip_on) v = v < -clip ? -clip : (v > clip ? clip : v);      // compares: a NaN stays a NaN, as with torch's Hardtanh
                        if (row < R) nxt[row * so + n] = v;
                    }
                }
            }
    }
}

// input gradient of a layer for the row tile: nxt[row][k] = (sum_n cur[row][n] W[n][k]) * elu'(h), where h = H_(l-1)[row][k] is what nxt[row][k]
// holds on entry (staged there when prev_elu): the lane that reads it is the one that overwrites it.  LDS only.
template <int RB, int NT>
__device__ __forceinline__ void bwd_tile(const TLayer &L, const lds_f *cur, lds_f *nxt, bool prev_elu, int R) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, h = lane >> 4;
    const int M = L.M, K = L.K, sg = L.so, sx = L.sa, tiles = (K + 15) >> 4;
    for (int tb = wave * NT; tb < tiles; tb += kWaves * NT) {
        f4 acc[RB][NT];
#pragma unroll
        for (int i = 0; i < NT; i++)
#pragma unroll
            for (int j = 0; j < RB; j++) acc[j][i] = (f4){0.f, 0.f, 0.f, 0.f};
        const float *wp[NT];
        const lds_f *gp[RB];
#pragma unroll
        for (int i = 0; i < NT; i++) wp[i] = L.W + min((tb + i) * 16 + r, K - 1);       // column k of W; the neuron's row is added per MFMA
#pragma unroll
        for (int j = 0; j < RB; j++) gp[j] = cur + min(j * 16 + r, R - 1) * sg + 4 * h;
        int n0 = 0;
        float an[4][NT];                         // the next chunk's fragments, in flight while this chunk's MFMAs issue
        f4 bn[RB];
        if (M >= 16) {
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
                for (int i = 0; i < NT; i++) an[e][i] = wp[i][(size_t)(4 * h + e) * K];
#pragma unroll
            for (int j = 0; j < RB; j++) bn[j] = *(const lds_f4 *)(gp[j]);
        }
        for (; n0 + 16 <= M; n0 += 16) {
            float av[4][NT];
            f4 bv[RB];
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
                for (int i = 0; i < NT; i++) av[e][i] = an[e][i];
#pragma unroll
            for (int j = 0; j < RB; j++) bv[j] = bn[j];
            if (n0 + 32 <= M) {
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int i = 0; i < NT; i++) an[e][i] = wp[i][(size_t)(n0 + 16 + 4 * h + e) * K];
#pragma unroll
                for (int j = 0; j < RB; j++) bn[j] = *(const lds_f4 *)(gp[j] + n0 + 16);
            }
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
                for (int i = 0; i < NT; i++)
#pragma unroll
                    for (int j = 0; j < RB; j++) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e][i], bv[j][e], acc[j][i], 0, 0, 0);
        }
        if (n0 < M) {                            // ragged reduction tail: zeros behind M on both operands, addresses clamped
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int n = n0 + 4 * h + e;
                const bool ok = n < M;
                const size_t wrow = (size_t)min(n, M - 1) * K;
                float bs[RB];
#pragma unroll
                for (int j = 0; j < RB; j++) bs[j] = ok ? gp[j][n0 + e] : 0.f;
#pragma unroll
                for (int i = 0; i < NT; i++) {
                    const float as = ok ? wp[i][wrow] : 0.f;
#pragma unroll
                    for (int j = 0; j < RB; j++) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, bs[j], acc[j][i], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NT; i++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int k = (tb + i) * 16 + 4 * h + e;
                if (k < K) {
#pragma unroll
                    for (int j = 0; j < RB; j++) {
                        const int row = j * 16 + r;
                        if (row < R) {
                            float v = acc[j][i][e];
                            if (prev_elu) {
                                const float hv = nxt[row * sx + k];
                                v = v * (hv > 0.f ? 1.0f : hv + 1.0f);
                            }
                            nxt[row * sx + k] = v;
                        }
                    }
                }
            }
    }
}

// the weight-gradient wave (64 lanes): job `rel` of layer L, (batch slice, 64 x 64 tile of the gradient), from G = G_l (N, M) dense and
// H = H_(l-1) (N, K), hs floats between rows; the partials go to the slice's slab at ws + L.p_off
__device__ __forceinline__ void wgrad_wave(const TLayer &L, const float *G, const float *H, int hs, float *ws, int rel, int N) {
    const int lane = threadIdx.x, r = lane & 15, h = lane >> 4;
    const int M = L.M, K = L.K;
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
    for (int row = rb + h; row < re + h; row += 4) {                // rb + 4 q + h: the wave leaves the loop together
        const bool ok = row < re;
        const size_t rc = (size_t)min(row, re - 1);
        float av[kWT], bv[kWT];
#pragma unroll
        for (int i = 0; i < kWT; i++) {
            const float g = G[rc * M + gc[i]], x = H[rc * hs + hc[i]];
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
    float *P = ws + L.p_off + (size_t)s * ((size_t)M * K + M);
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
    if (tk == 0) {                                                   // the bias partial: the four row phases of a column in a fixed order
#pragma unroll
        for (int i = 0; i < kWT; i++) {
            const float s0 = __shfl(bsum[i], r), s1 = __shfl(bsum[i], r + 16), s2 = __shfl(bsum[i], r + 32), s3 = __shfl(bsum[i], r + 48);
            const int n = n0 + i * 16 + r;
            if (h == 0 && n < M) P[(size_t)M * K + n] = ((s0 + s1) + s2) + s3;
        }
    }
}

// slice `s` of the column sums of an (N, A) matrix (grad_sigma, for grad_std): one wave, partials to P + s * A
__device__ __forceinline__ void colsum_wave(const float *src, int stride, int A, float *P, int s, int rps, int N) {
    const int rb = s * rps, re = min(rb + rps, N);
    P += (size_t)s * A;
    for (int col = threadIdx.x; col < A; col += 64) {
        float sum = 0.f;
        for (int row = rb; row < re; row++) sum += src[(size_t)row * stride + col];
        P[col] = sum;
    }
}

// every element of a layer's gradient: its partials in slice order
__device__ __forceinline__ void combine_layer(const TLayer &L, const float *ws, long long first, long long stride) {
    const long long nw = (long long)L.M * L.K, n = nw + L.M;
    const float *P = ws + L.p_off;
    for (long long e = first; e < n; e += stride) {
        float sum = P[e];
        for (int s = 1; s < L.S; s++) sum += P[s * n + e];
        if (e < nw) L.gW[e] = sum;
        else L.gb[e - nw] = sum;
    }
}

__device__ __forceinline__ void combine_cols(const float *P, int A, int S, float *dst, long long first, long long stride) {
    for (long long e = first; e < A; e += stride) {
        float sum = P[e];
        for (int s = 1; s < S; s++) sum += P[(long long)s * A + e];
        dst[e] = sum;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static inline int lds_stride(int w) { return ((((w + 3) & ~3) - 4 + 63) / 64) * 64 + 4; }

static inline void slice_rule(int n_rows, long long tiles, int &S, int &rps, int target_jobs = LG_TRAIN_TARGET_JOBS) {
    long long want = n_rows / LG_TRAIN_MIN_SLICE_ROWS;
    if (want < 1) want = 1;
    long long by_jobs = target_jobs / tiles;
    if (by_jobs < 1) by_jobs = 1;
    if (want > by_jobs) want = by_jobs;
    if (want > LG_TRAIN_MAX_SLICES) want = LG_TRAIN_MAX_SLICES;
    long long per = ((long long)n_rows + want - 1) / want;
    per = (per + 3) & ~3LL;
    rps = (int)per;
    S = (int)(((long long)n_rows + per - 1) / per);
}
#endif /* LG_TRAIN_TILES_H */

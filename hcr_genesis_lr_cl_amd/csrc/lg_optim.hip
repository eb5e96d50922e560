// lg_optim.hip -- the fused optimizer step (include/lgoptim.h): global gradient norm, clip coefficient, the adaptive learning-rate rule
// and torch.optim.Adam's update of up to LG_ADAM_MAX_TENSORS parameter tensors, in two launches that read nothing back.
//
// Layout: the tensors are cut into chunks of LG_ADAM_CHUNK floats numbered one behind the other; workgroup b sweeps chunks b, b + grid,
//   ...  The chunk -> tensor lookup is uniform per workgroup: a prefix table of chunk ends rides in the argument block next to the tensor
//   descriptors, and the lookup walks it on scalar values (the chunks of a workgroup ascend, so the walk resumes where it stopped).  A
//   whole chunk of a tensor whose four base addresses are 16-byte aligned moves as one 16-byte access per lane, every other chunk (a
//   ragged tail, a view at an odd offset) as 4-byte accesses: lg_ppo.hip treats its row tails the same way.
// Reduction: adam_norm_kernel -- every lane a float64 accumulator of g * g over its elements in chunk order, folded per workgroup
//   (xor butterfly inside each wave, then waves 0..3 in order by one lane) into slot b of the slab.  adam_update_kernel -- every workgroup
//   sums the slab itself (lane t takes slots t, t + 256, then the same fold), so every workgroup holds the same bits of the norm without
//   a third launch or a grid barrier.  No step depends on which workgroup finishes first and nothing is accumulated with atomics.
// The cell: learning rate and step count are two doubles on the device.  Lane 0 of workgroup 0 of adam_norm_kernel alone advances them
//   and nothing else reads them in that launch; adam_update_kernel, enqueued behind it on the same stream, only reads them.
// min is a compare that passes a NaN on ("NaN is not silent"); sqrtf, / and pow are the device library's, not
//   fast-math intrinsics: parity with torch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <string>
#include "../../include/lgoptim.h"

int lg_fail_msg(const std::string &m);   // lg_host.hip: sets the thread-local message, returns 1

typedef float f4a __attribute__((ext_vector_type(4)));   // 16-byte aligned: used on the aligned path alone

static const int kThreads = LG_ADAM_THREADS, kWaves = LG_ADAM_THREADS / 64, kChunk = LG_ADAM_CHUNK;
static_assert(LG_ADAM_CHUNK == 4 * LG_ADAM_THREADS, "a chunk is one 16-byte access per lane");
static_assert(LG_ADAM_MAX_BLOCKS <= 2 * LG_ADAM_THREADS, "adam_update_kernel sums the slab as slots t and t + 256");

struct KAdam {
    LgAdamTensor t[LG_ADAM_MAX_TENSORS];
    long long chunk_end[LG_ADAM_MAX_TENSORS];   // the chunks of tensor i are [chunk_end[i - 1], chunk_end[i])
    long long chunks;
    int n_tensors, n_blocks, clip, kl_rule;
    float max_grad_norm, w1, b2, w2, eps;       // (float)max_grad_norm, (float)(1 - beta1), (float)beta2, (float)(1 - beta2), (float)eps
    double beta1, beta2, desired_kl;
    const float *kl;
    double *state, *partials;
    float *result;
};
static_assert(sizeof(KAdam) <= 4096, "the kernels take the descriptor by value: HIP's kernel-argument block is 4 KB");

// x of all lanes of the workgroup -> the same sum in every lane, in a fixed order
__device__ __forceinline__ double block_sum(double x) {
    __shared__ double part[kWaves];
    __shared__ double total;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    if (lane == 0) part[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = part[0];
        for (int w = 1; w < kWaves; w++) s += part[w];
        total = s;
    }
    __syncthreads();
    return total;
}

// the chunk's tensor (the walk resumes at `i`), its first element and its length
struct Chunk { float *param, *exp_avg, *exp_avg_sq; const float *grad; int n; bool vec; };

__device__ __forceinline__ Chunk find_chunk(const KAdam &k, long long c, int &i) {
    while (i < k.n_tensors - 1 && c >= k.chunk_end[i]) i++;
    float *const p = k.t[i].param, *const m = k.t[i].exp_avg, *const v = k.t[i].exp_avg_sq;
    const float *const g = k.t[i].grad;
    const long long off = (c - (i ? k.chunk_end[i - 1] : 0)) * kChunk, left = k.t[i].numel - off;
    Chunk ch;
    ch.param = p + off; ch.exp_avg = m + off; ch.exp_avg_sq = v + off; ch.grad = g + off;
    ch.n = (int)(left < kChunk ? left : kChunk);
    ch.vec = ch.n == kChunk && (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;   // off is a multiple of 4 KB
    return ch;
}

__global__ __launch_bounds__(LG_ADAM_THREADS) void adam_norm_kernel(KAdam k) {
    double acc = 0.0;
    int i = 0;
    for (long long c = blockIdx.x; c < k.chunks; c += gridDim.x) {       // block-uniform: every lane of a wave takes the same branch
        const Chunk ch = find_chunk(k, c, i);
        const float *g = ch.grad;
        if (ch.vec) {
            const f4a x = *reinterpret_cast<const f4a *>(g + 4 * threadIdx.x);
            acc += (double)x.x * (double)x.x;
            acc += (double)x.y * (double)x.y;
            acc += (double)x.z * (double)x.z;
            acc += (double)x.w * (double)x.w;
        } else {
            for (int e = threadIdx.x; e < ch.n; e += kThreads) acc += (double)g[e] * (double)g[e];
        }
    }
    const double s = block_sum(acc);
    if (threadIdx.x == 0) k.partials[blockIdx.x] = s;
    if (blockIdx.x == 0 && threadIdx.x == 0) {       // the one writer of the cell; adam_update_kernel reads it behind this launch
        double lr = k.state[LG_ADAM_S_LR];
        if (k.kl_rule) {
            const double kl = (double)*k.kl;
            if (kl > k.desired_kl * 2.0) {
                const double x = lr / 1.5;
                lr = x > 1e-5 ? x : 1e-5;
            } else if (kl < k.desired_kl / 2.0 && kl > 0.0) {
                const double x = lr * 1.5;
                lr = x < 1e-2 ? x : 1e-2;
            }
            k.state[LG_ADAM_S_LR] = lr;
        }
        k.state[LG_ADAM_S_STEP] = k.state[LG_ADAM_S_STEP] + 1.0;
    }
}

__global__ __launch_bounds__(LG_ADAM_THREADS) void adam_update_kernel(KAdam k) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < k.n_blocks; b += kThreads) acc += k.partials[b];
    const float total = (float)sqrt(block_sum(acc));
    float coef = 1.f;
    if (k.clip) {
        const float c = k.max_grad_norm / (total + 1e-6f);
        coef = c > 1.f ? 1.f : c;                    // torch.clamp(max = 1): a NaN stays
    }
    const double lr = k.state[LG_ADAM_S_LR], step = k.state[LG_ADAM_S_STEP];
    const double bc1 = 1.0 - pow(k.beta1, step), bc2 = 1.0 - pow(k.beta2, step);
    const float neg_step_size = (float)(-(lr / bc1)), bc2_sqrt = (float)sqrt(bc2);
    const float w1 = k.w1, b2 = k.b2, w2 = k.w2, eps = k.eps;
    int i = 0;
    for (long long c = blockIdx.x; c < k.chunks; c += gridDim.x) {
        const Chunk ch = find_chunk(k, c, i);
        const float *gp = ch.grad;
        float *pp = ch.param, *mp = ch.exp_avg, *vp = ch.exp_avg_sq;
        if (ch.vec) {
            const int e = 4 * threadIdx.x;
            const f4a g4 = *reinterpret_cast<const f4a *>(gp + e);
            f4a p4 = *reinterpret_cast<f4a *>(pp + e), m4 = *reinterpret_cast<f4a *>(mp + e), v4 = *reinterpret_cast<f4a *>(vp + e);
            for (int j = 0; j < 4; j++) {
                const float g = g4[j] * coef;
                const float m = m4[j] + (g - m4[j]) * w1;
                const float v = v4[j] * b2 + w2 * g * g;
                p4[j] = p4[j] + neg_step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
                m4[j] = m; v4[j] = v;
            }
            *reinterpret_cast<f4a *>(pp + e) = p4;
            *reinterpret_cast<f4a *>(mp + e) = m4;
            *reinterpret_cast<f4a *>(vp + e) = v4;
        } else {
            for (int e = threadIdx.x; e < ch.n; e += kThreads) {
                const float g = gp[e] * coef;
                const float m = mp[e] + (g - mp[e]) * w1;
                const float v = vp[e] * b2 + w2 * g * g;
                pp[e] = pp[e] + neg_step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
                mp[e] = m; vp[e] = v;
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        k.result[LG_ADAM_R_GRAD_NORM] = total;
        k.result[LG_ADAM_R_CLIP_COEF] = coef;
        k.result[LG_ADAM_R_LR] = (float)lr;
        k.result[LG_ADAM_R_STEP] = (float)step;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// the part of the descriptor the plan reads; `msg` names the field on a refusal
static bool plan_shape(const LgAdamArgs *a, KAdam &k, std::string &msg) {
    if (!a) { msg = "null descriptor"; return false; }
    if (a->n_tensors < 1 || a->n_tensors > LG_ADAM_MAX_TENSORS) { msg = "n_tensors = " + std::to_string(a->n_tensors) + " is outside [1, " + std::to_string(LG_ADAM_MAX_TENSORS) + "]"; return false; }
    long long c = 0;
    for (int i = 0; i < LG_ADAM_MAX_TENSORS; i++) {
        if (i < a->n_tensors) {
            if (a->tensor[i].numel < 1) { msg = "tensor[" + std::to_string(i) + "].numel < 1"; return false; }
            c += (long long)((a->tensor[i].numel - 1) / kChunk + 1);
        }
        k.chunk_end[i] = c;
    }
    k.chunks = c;
    k.n_tensors = a->n_tensors;
    k.n_blocks = (int)(c < LG_ADAM_MAX_BLOCKS ? c : LG_ADAM_MAX_BLOCKS);
    return true;
}

extern "C" int lg_adam_workspace(const LgAdamArgs *args) {
    KAdam k = {}; std::string msg;
    if (!plan_shape(args, k, msg)) { lg_fail_msg("lg_adam_step: " + msg); return 0; }
    return k.n_blocks;
}

extern "C" int lg_adam_step(const LgAdamArgs *args, void *stream) {
    KAdam k = {}; std::string msg;
    if (!plan_shape(args, k, msg)) return lg_fail_msg("lg_adam_step: " + msg);
    const LgAdamArgs &a = *args;
    for (int i = 0; i < a.n_tensors; i++) {
        const LgAdamTensor &T = a.tensor[i];
        const struct { const void *p; const char *name; } t[] = {{T.param, "param"}, {T.grad, "grad"}, {T.exp_avg, "exp_avg"}, {T.exp_avg_sq, "exp_avg_sq"}};
        for (const auto &x : t)
            if (!x.p) return lg_fail_msg("lg_adam_step: tensor[" + std::to_string(i) + "]." + x.name + " is null");
        k.t[i] = T;
    }
    if (a.flags & ~(LG_ADAM_CLIP | LG_ADAM_KL_RULE)) return lg_fail_msg("lg_adam_step: flags has unknown bits");
    const bool clip = (a.flags & LG_ADAM_CLIP) != 0, kl_rule = (a.flags & LG_ADAM_KL_RULE) != 0;
    if (kl_rule && !a.kl) return lg_fail_msg("lg_adam_step: kl is null with LG_ADAM_KL_RULE");
    if (!kl_rule && a.kl) return lg_fail_msg("lg_adam_step: kl is set without LG_ADAM_KL_RULE");
    if (kl_rule && (!(a.desired_kl > 0.0) || !std::isfinite(a.desired_kl))) return lg_fail_msg("lg_adam_step: desired_kl must be a finite number above 0 with LG_ADAM_KL_RULE");
    if (clip && !(a.max_grad_norm > 0.0)) return lg_fail_msg("lg_adam_step: max_grad_norm must be above 0 with LG_ADAM_CLIP");
    if (!(a.beta1 >= 0.0 && a.beta1 < 1.0)) return lg_fail_msg("lg_adam_step: beta1 = " + std::to_string(a.beta1) + " is outside [0, 1)");
    if (!(a.beta2 >= 0.0 && a.beta2 < 1.0)) return lg_fail_msg("lg_adam_step: beta2 = " + std::to_string(a.beta2) + " is outside [0, 1)");
    if (!(a.eps >= 0.0)) return lg_fail_msg("lg_adam_step: eps is below 0");
    if (!a.state) return lg_fail_msg("lg_adam_step: state is null");
    if (!a.partials) return lg_fail_msg("lg_adam_step: partials is null");
    if (a.partials_capacity < (long long)k.n_blocks)
        return lg_fail_msg("lg_adam_step: partials_capacity = " + std::to_string((long long)a.partials_capacity) + " is below the " + std::to_string(k.n_blocks) + " doubles of lg_adam_workspace");
    if (!a.result) return lg_fail_msg("lg_adam_step: result is null");

    k.clip = clip; k.kl_rule = kl_rule;
    k.max_grad_norm = clip ? (float)a.max_grad_norm : 0.f;
    k.w1 = (float)(1.0 - a.beta1); k.b2 = (float)a.beta2; k.w2 = (float)(1.0 - a.beta2); k.eps = (float)a.eps;
    k.beta1 = a.beta1; k.beta2 = a.beta2; k.desired_kl = kl_rule ? a.desired_kl : 0.0;
    k.kl = a.kl; k.state = a.state; k.partials = a.partials; k.result = a.result;
    hipLaunchKernelGGL(adam_norm_kernel, dim3((unsigned)k.n_blocks), dim3(kThreads), 0, (hipStream_t)stream, k);
    hipLaunchKernelGGL(adam_update_kernel, dim3((unsigned)k.n_blocks), dim3(kThreads), 0, (hipStream_t)stream, k);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : lg_fail_msg(std::string("lg_adam_step: ") + hipGetErrorString(e));
}

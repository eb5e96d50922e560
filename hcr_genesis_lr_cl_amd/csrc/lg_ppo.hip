// lg_ppo.hip -- the fused PPO loss head (include/lgppo.h): surrogate, value loss, entropy, KL and the gradient of the loss with respect
// to mu, sigma and values, for one or two policy row groups and one value group, in one pass plus a one-workgroup sum.
//
// Layout: a policy row is carried by L = 2^k >= ceil(A / 4) neighbouring lanes of one wave, lane q of them holding action columns
//   [4 q, 4 q + 4); the row sums (log-prob, entropy, KL) are float64 butterflies (__shfl_xor over the L lanes), after which every lane of
//   the row knows the ratio and the row's d loss / d logp and writes the gradients of its own quad.  A value row is one lane.  The
//   gradients need only the 1 / B factors, never the reduced sums, so they are written in the pass that forms the partials.
// Reduction: every lane keeps LG_PPO_PARTIAL_SLOTS float64 accumulators over the tiles its workgroup sweeps (tile order), the workgroup
//   folds them (butterfly inside each wave, then waves 0..3 in order) into its row of the partials slab, and ppo_finalize_kernel -- one
//   workgroup enqueued behind the pass on the same stream -- sums the slab rows (lane t takes rows t, t + 256, ... in order, then the same
//   fold) and writes the result vector.  No step depends on which workgroup finishes first and nothing is accumulated with atomics, so
//   the scalars are bit-reproducible; the gradients are pure per-row functions of the inputs.
// max and clamp are compares that pass a NaN on ("NaN is not silent"); expf / logf are the device library's,
//   not fast-math intrinsics: parity with torch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <string>
#include "../../include/lgppo.h"

int lg_fail_msg(const std::string &m);   // lg_host.hip: sets the thread-local message, returns 1

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // rows start wherever the caller's view puts them

static const int kThreads = LG_PPO_THREADS, kWaves = LG_PPO_THREADS / 64, kSlots = LG_PPO_PARTIAL_SLOTS;
enum { S_SUR0 = 0, S_SUR1 = 1, S_ENT = 2, S_KL0 = 3, S_KL1 = 4, S_VAL = 5 };

struct KGroup {
    const float *mu, *sigma, *actions, *old_mu, *old_sigma, *old_log_prob, *advantages;
    float *grad_mu, *grad_sigma;
    int n_rows, mu_stride, sigma_stride, actions_stride, old_mu_stride, old_sigma_stride, old_log_prob_stride, advantages_stride,
        grad_mu_stride, grad_sigma_stride;
    float inv_rows;                 // 1 / B_g
};
struct KPpo {
    KGroup g[LG_PPO_MAX_GROUPS];
    const float *values, *returns, *target_values;
    float *grad_values;
    int values_stride, returns_stride, target_values_stride, grad_values_stride;
    int n_value_rows, A, lpr_log2, spo, clipped_value;
    long long tile_end[LG_PPO_MAX_GROUPS], tiles;      // tiles of group 0 end at tile_end[0], of group 1 at tile_end[1], the value group's at tiles
    float ratio_lo, ratio_hi, clip, two_clip;          // (float)(1 - eps), (float)(1 + eps), (float)eps, (float)(2 eps)
    float value_scale;                                 // value_loss_coef / B_v
    float entropy_scale;                               // entropy_coef / (all policy rows)
    double *partials;
};
struct KFinal {
    const double *partials;
    float *result;
    int n_blocks, n_groups, has_kl[LG_PPO_MAX_GROUPS];
    double rows[LG_PPO_MAX_GROUPS], policy_rows, value_rows, value_loss_coef, entropy_coef;
};

// torch.max / torch.clamp on floats: a NaN operand is the result
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ float nan_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// the lane's quad of row `p` (columns c0 .. c0 + 3 below A); columns that do not exist read as `fill`
__device__ __forceinline__ void load_quad(const float *p, int c0, int A, bool on, float fill, float v[4]) {
    v[0] = v[1] = v[2] = v[3] = fill;
    if (!on) return;
    if (c0 + 4 <= A) {
        const f4u x = *reinterpret_cast<const f4u *>(p + c0);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
        for (int j = 0; j < 4; j++)
            if (c0 + j < A) v[j] = p[c0 + j];
    }
}

__device__ __forceinline__ void store_quad(float *p, int c0, int A, const float v[4]) {
    if (c0 + 4 <= A) {
        f4u x; x.x = v[0]; x.y = v[1]; x.z = v[2]; x.w = v[3];
        *reinterpret_cast<f4u *>(p + c0) = x;
    } else {
        for (int j = 0; j < 4; j++)
            if (c0 + j < A) p[c0 + j] = v[j];
    }
}

__device__ __forceinline__ void policy_tile(const KPpo &k, const KGroup &G, int gi, long long tile, double acc[kSlots]) {
    const int lpr = 1 << k.lpr_log2, A = k.A;
    const long long row = tile * (kThreads >> k.lpr_log2) + (threadIdx.x >> k.lpr_log2);
    const int q = threadIdx.x & (lpr - 1), c0 = 4 * q;
    const bool valid = row < G.n_rows, on = valid && c0 < A, has_kl = G.old_mu != nullptr;
    const size_t r = valid ? (size_t)row : 0;
    float mu[4], sg[4], ac[4], omu[4], osg[4];
    load_quad(G.mu + r * G.mu_stride, c0, A, on, 0.f, mu);
    load_quad(G.sigma + r * G.sigma_stride, c0, A, on, 1.f, sg);
    load_quad(G.actions + r * G.actions_stride, c0, A, on, 0.f, ac);
    if (has_kl) {
        load_quad(G.old_mu + r * G.old_mu_stride, c0, A, on, 0.f, omu);
        load_quad(G.old_sigma + r * G.old_sigma_stride, c0, A, on, 1.f, osg);
    }
    const float old_lp = valid ? G.old_log_prob[r * G.old_log_prob_stride] : 0.f;
    const float adv = valid ? G.advantages[r * G.advantages_stride] : 0.f;
    double lp = 0.0, ent = 0.0, kl = 0.0;
    float dmu[4], dsg[4], inv_s[4];      // d logp / d mu, the (a - mu)^2 / sigma^3 part of d logp / d sigma, 1 / sigma
    for (int j = 0; j < 4; j++) {
        const bool col = on && c0 + j < A;
        const float d = ac[j] - mu[j], s = sg[j], var = s * s, ls = logf(s);
        const float t_lp = -(d * d) / (2.f * var) - ls;
        inv_s[j] = 1.f / s;
        dmu[j] = d / var;
        dsg[j] = (d * d) / (var * s);
        if (col) { lp += (double)t_lp; ent += (double)ls; }
        if (col && has_kl) {
            const float dm = omu[j] - mu[j];
            kl += (double)(logf(s / osg[j] + 1.e-5f) + (osg[j] * osg[j] + dm * dm) / (2.f * var) - 0.5f);
        }
    }
    for (int m = 1; m < lpr; m <<= 1) {          // the row's lanes are neighbours inside one wave: every lane ends with the row sums
        lp += __shfl_xor(lp, m);
        ent += __shfl_xor(ent, m);
        kl += __shfl_xor(kl, m);
    }
    // the per-column constants once per row and in float64: as a float in every column term, 0.5 log 2 pi is off by 1.6e-8, the same way
    // in every column, and A of those shift the row's log-prob (1e-6 at A = 64) instead of averaging out
    lp -= (double)A * 0.918938533204672742;
    ent += (double)A * 1.418938533204672742;
    const float ratio = expf((float)(lp - (double)old_lp));
    // the row's surrogate term and d loss / d ratio.  The 1 / B of the mean goes into the advantage first, as in autograd's backward:
    // |Adv| near FLT_MAX then overflows where the gradient itself does and not in a factor that 1 / B would have brought back.
    const float adv_b = adv * G.inv_rows;
    float term, g;
    if (k.spo) {
        const float e = ratio - 1.f;
        term = -(adv * ratio - fabsf(adv) * (e * e) / k.two_clip);
        g = -(adv_b - fabsf(adv_b) * (2.f * e) / k.two_clip);
    } else {
        const float rc = nan_clamp(ratio, k.ratio_lo, k.ratio_hi);
        const float s1 = -adv * ratio, s2 = -adv * rc;
        const bool inside = ratio >= k.ratio_lo && ratio <= k.ratio_hi;      // clamp's closed interval
        term = nan_max(s1, s2);
        g = s1 > s2 ? -adv_b : (s2 > s1 ? 0.f : (s1 == s2 ? (inside ? -adv_b : -0.5f * adv_b) : NAN));
    }
    const float dlp = g * ratio;                 // d loss / d logp of this row
    if (valid && q == 0) {
        acc[S_SUR0 + gi] += (double)term;
        acc[S_ENT] += ent;
        acc[S_KL0 + gi] += kl;
    }
    if (on) {
        float gm[4], gs[4];
        for (int j = 0; j < 4; j++) {
            gm[j] = dlp * dmu[j];
            // the two partials of sigma apart, as autograd adds them: a row whose d loss / d logp is infinite gives inf - inf = NaN
            gs[j] = dlp * dsg[j] - dlp * inv_s[j] - k.entropy_scale * inv_s[j];
        }
        store_quad(G.grad_mu + r * G.grad_mu_stride, c0, A, gm);
        store_quad(G.grad_sigma + r * G.grad_sigma_stride, c0, A, gs);
    }
}

__device__ __forceinline__ void value_tile(const KPpo &k, long long tile, double acc[kSlots]) {
    const long long row = tile * kThreads + threadIdx.x;
    if (row >= k.n_value_rows) return;
    const size_t r = (size_t)row;
    const float v = k.values[r * k.values_stride], R = k.returns[r * k.returns_stride];
    float term, g;
    if (k.clipped_value) {
        const float vt = k.target_values[r * k.target_values_stride];
        const float d = v - vt, vc = vt + nan_clamp(d, -k.clip, k.clip);
        const float e1 = v - R, e2 = vc - R, l1 = e1 * e1, l2 = e2 * e2;
        const float g1 = 2.f * e1, g2 = (d >= -k.clip && d <= k.clip) ? 2.f * e2 : 0.f;
        term = nan_max(l1, l2);
        g = l1 > l2 ? g1 : (l2 > l1 ? g2 : (l1 == l2 ? 0.5f * g1 + 0.5f * g2 : NAN));
    } else {
        const float e = R - v;
        term = e * e;
        g = -2.f * e;
    }
    acc[S_VAL] += (double)term;
    k.grad_values[r * k.grad_values_stride] = g * k.value_scale;
}

// acc[] of all lanes of the workgroup -> out[] by thread 0, in a fixed order
__device__ __forceinline__ void block_fold(double acc[kSlots], double *out) {
    __shared__ double part[kWaves][kSlots];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = 0; s < kSlots; s++) {
        double x = acc[s];
        for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
        if (lane == 0) part[wave][s] = x;
    }
    __syncthreads();
    if (threadIdx.x < kSlots) {
        double x = part[0][threadIdx.x];
        for (int w = 1; w < kWaves; w++) x += part[w][threadIdx.x];
        out[threadIdx.x] = x;
    }
}

__global__ __launch_bounds__(LG_PPO_THREADS) void ppo_loss_kernel(KPpo k) {
    double acc[kSlots];
    for (int s = 0; s < kSlots; s++) acc[s] = 0.0;
    for (long long t = blockIdx.x; t < k.tiles; t += gridDim.x) {       // block-uniform: every lane of a wave takes the same branch
        if (t < k.tile_end[0]) policy_tile(k, k.g[0], 0, t, acc);
        else if (t < k.tile_end[1]) policy_tile(k, k.g[1], 1, t - k.tile_end[0], acc);
        else value_tile(k, t - k.tile_end[1], acc);
    }
    block_fold(acc, k.partials + (size_t)blockIdx.x * kSlots);
}

__global__ __launch_bounds__(LG_PPO_THREADS) void ppo_finalize_kernel(KFinal f) {
    __shared__ double tot[kSlots];
    double acc[kSlots];
    for (int s = 0; s < kSlots; s++) acc[s] = 0.0;
    for (int b = threadIdx.x; b < f.n_blocks; b += kThreads)
        for (int s = 0; s < kSlots; s++) acc[s] += f.partials[(size_t)b * kSlots + s];
    block_fold(acc, tot);
    __syncthreads();
    if (threadIdx.x == 0) {
        double sur[LG_PPO_MAX_GROUPS] = {0.0, 0.0}, klm[LG_PPO_MAX_GROUPS] = {0.0, 0.0};
        double loss = 0.0;
        for (int g = 0; g < f.n_groups; g++) {
            sur[g] = tot[S_SUR0 + g] / f.rows[g];
            klm[g] = f.has_kl[g] ? tot[S_KL0 + g] / f.rows[g] : 0.0;
            loss += sur[g];
        }
        const double val = tot[S_VAL] / f.value_rows, ent = tot[S_ENT] / f.policy_rows;
        loss += f.value_loss_coef * val - f.entropy_coef * ent;
        float *r = f.result;
        r[LG_PPO_R_LOSS] = (float)loss;
        r[LG_PPO_R_SURROGATE] = (float)sur[0]; r[LG_PPO_R_SURROGATE + 1] = (float)sur[1];
        r[LG_PPO_R_VALUE] = (float)val;
        r[LG_PPO_R_ENTROPY] = (float)ent;
        r[LG_PPO_R_KL] = (float)klm[0]; r[LG_PPO_R_KL + 1] = (float)klm[1];
        r[7] = 0.f;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
struct Plan { int lpr_log2, n_blocks; long long tile_end[LG_PPO_MAX_GROUPS], tiles; };

// the part of the descriptor the plan reads; `msg` names the field on a refusal
static bool plan_shape(const LgPpoLossArgs *a, Plan &p, std::string &msg) {
    if (!a) { msg = "null descriptor"; return false; }
    if (a->n_groups < 1 || a->n_groups > LG_PPO_MAX_GROUPS) { msg = "n_groups = " + std::to_string(a->n_groups) + " is outside [1, " + std::to_string(LG_PPO_MAX_GROUPS) + "]"; return false; }
    if (a->n_actions < 1 || a->n_actions > LG_PPO_MAX_ACTIONS) { msg = "n_actions = " + std::to_string(a->n_actions) + " is outside [1, " + std::to_string(LG_PPO_MAX_ACTIONS) + "]"; return false; }
    if (a->n_value_rows < 1) { msg = "n_value_rows < 1"; return false; }
    const int quads = (a->n_actions + 3) / 4;
    p.lpr_log2 = 0;
    while ((1 << p.lpr_log2) < quads) p.lpr_log2++;
    const int rows_per_tile = kThreads >> p.lpr_log2;
    long long t = 0;
    for (int g = 0; g < LG_PPO_MAX_GROUPS; g++) {
        if (g < a->n_groups) {
            if (a->group[g].n_rows < 1) { msg = "group[" + std::to_string(g) + "].n_rows < 1"; return false; }
            t += ((long long)a->group[g].n_rows + rows_per_tile - 1) / rows_per_tile;
        }
        p.tile_end[g] = t;
    }
    p.tiles = t + ((long long)a->n_value_rows + kThreads - 1) / kThreads;
    p.n_blocks = (int)(p.tiles < LG_PPO_MAX_BLOCKS ? p.tiles : LG_PPO_MAX_BLOCKS);
    return true;
}

extern "C" int lg_ppo_loss_workspace(const LgPpoLossArgs *args) {
    Plan p; std::string msg;
    if (!plan_shape(args, p, msg)) { lg_fail_msg("lg_ppo_loss: " + msg); return 0; }
    return p.n_blocks * kSlots;
}

extern "C" int lg_ppo_loss(const LgPpoLossArgs *args, void *stream) {
    Plan p; std::string msg;
    if (!plan_shape(args, p, msg)) return lg_fail_msg("lg_ppo_loss: " + msg);
    const LgPpoLossArgs &a = *args;
    if (a.flags & ~(LG_PPO_CLIPPED_VALUE | LG_PPO_SPO)) return lg_fail_msg("lg_ppo_loss: flags has unknown bits");
    if (!(a.clip_param > 0.0) || !std::isfinite(a.clip_param)) return lg_fail_msg("lg_ppo_loss: clip_param must be a finite number above 0");
    if (!std::isfinite(a.value_loss_coef)) return lg_fail_msg("lg_ppo_loss: value_loss_coef is not finite");
    if (!std::isfinite(a.entropy_coef)) return lg_fail_msg("lg_ppo_loss: entropy_coef is not finite");
    const int A = a.n_actions;
    KPpo k = {};
    KFinal f = {};
    long long policy_rows = 0;
    for (int g = 0; g < a.n_groups; g++) {
        const LgPpoGroup &G = a.group[g];
        const std::string w = "lg_ppo_loss: group[" + std::to_string(g) + "].";
        const struct { const void *p; int stride, width; const char *name; } t[] = {
            {G.mu, G.mu_stride, A, "mu"}, {G.sigma, G.sigma_stride, A, "sigma"}, {G.actions, G.actions_stride, A, "actions"},
            {G.old_log_prob, G.old_log_prob_stride, 1, "old_log_prob"}, {G.advantages, G.advantages_stride, 1, "advantages"},
            {G.grad_mu, G.grad_mu_stride, A, "grad_mu"}, {G.grad_sigma, G.grad_sigma_stride, A, "grad_sigma"}};
        for (const auto &x : t) {
            if (!x.p) return lg_fail_msg(w + x.name + " is null");
            if (x.stride < x.width) return lg_fail_msg(w + x.name + "_stride = " + std::to_string(x.stride) + " is below the width " + std::to_string(x.width));
        }
        if ((G.old_mu == nullptr) != (G.old_sigma == nullptr)) return lg_fail_msg(w + (G.old_mu ? "old_mu without old_sigma" : "old_sigma without old_mu"));
        if (G.old_mu && G.old_mu_stride < A) return lg_fail_msg(w + "old_mu_stride = " + std::to_string(G.old_mu_stride) + " is below the width " + std::to_string(A));
        if (G.old_sigma && G.old_sigma_stride < A) return lg_fail_msg(w + "old_sigma_stride = " + std::to_string(G.old_sigma_stride) + " is below the width " + std::to_string(A));
        KGroup &K = k.g[g];
        K.mu = G.mu; K.sigma = G.sigma; K.actions = G.actions; K.old_mu = G.old_mu; K.old_sigma = G.old_sigma;
        K.old_log_prob = G.old_log_prob; K.advantages = G.advantages; K.grad_mu = G.grad_mu; K.grad_sigma = G.grad_sigma;
        K.n_rows = G.n_rows; K.mu_stride = G.mu_stride; K.sigma_stride = G.sigma_stride; K.actions_stride = G.actions_stride;
        K.old_mu_stride = G.old_mu_stride; K.old_sigma_stride = G.old_sigma_stride; K.old_log_prob_stride = G.old_log_prob_stride;
        K.advantages_stride = G.advantages_stride; K.grad_mu_stride = G.grad_mu_stride; K.grad_sigma_stride = G.grad_sigma_stride;
        K.inv_rows = 1.f / (float)G.n_rows;
        f.rows[g] = (double)G.n_rows; f.has_kl[g] = G.old_mu != nullptr;
        policy_rows += G.n_rows;
    }
    const struct { const void *p; int stride; const char *name; } v[] = {
        {a.values, a.values_stride, "values"}, {a.returns, a.returns_stride, "returns"}, {a.target_values, a.target_values_stride, "target_values"},
        {a.grad_values, a.grad_values_stride, "grad_values"}};
    for (const auto &x : v) {
        if (!x.p) return lg_fail_msg(std::string("lg_ppo_loss: ") + x.name + " is null");
        if (x.stride < 1) return lg_fail_msg(std::string("lg_ppo_loss: ") + x.name + "_stride = " + std::to_string(x.stride) + " is below the width 1");
    }
    if (!a.partials) return lg_fail_msg("lg_ppo_loss: partials is null");
    if (a.partials_capacity < (long long)p.n_blocks * kSlots)
        return lg_fail_msg("lg_ppo_loss: partials_capacity = " + std::to_string((long long)a.partials_capacity) + " is below the " + std::to_string(p.n_blocks * kSlots) + " doubles of lg_ppo_loss_workspace");
    if (!a.result) return lg_fail_msg("lg_ppo_loss: result is null");

    k.values = a.values; k.returns = a.returns; k.target_values = a.target_values; k.grad_values = a.grad_values;
    k.values_stride = a.values_stride; k.returns_stride = a.returns_stride; k.target_values_stride = a.target_values_stride;
    k.grad_values_stride = a.grad_values_stride;
    k.n_value_rows = a.n_value_rows; k.A = A; k.lpr_log2 = p.lpr_log2;
    k.spo = (a.flags & LG_PPO_SPO) != 0; k.clipped_value = (a.flags & LG_PPO_CLIPPED_VALUE) != 0;
    k.tile_end[0] = p.tile_end[0]; k.tile_end[1] = p.tile_end[1]; k.tiles = p.tiles;
    k.ratio_lo = (float)(1.0 - a.clip_param); k.ratio_hi = (float)(1.0 + a.clip_param);
    k.clip = (float)a.clip_param; k.two_clip = (float)(2.0 * a.clip_param);
    k.value_scale = (float)(a.value_loss_coef / (double)a.n_value_rows);
    k.entropy_scale = (float)(a.entropy_coef / (double)policy_rows);
    k.partials = a.partials;
    f.partials = a.partials; f.result = a.result; f.n_blocks = p.n_blocks; f.n_groups = a.n_groups;
    f.policy_rows = (double)policy_rows; f.value_rows = (double)a.n_value_rows;
    f.value_loss_coef = a.value_loss_coef; f.entropy_coef = a.entropy_coef;
    hipLaunchKernelGGL(ppo_loss_kernel, dim3((unsigned)p.n_blocks), dim3(kThreads), 0, (hipStream_t)stream, k);
    hipLaunchKernelGGL(ppo_finalize_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, f);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : lg_fail_msg(std::string("lg_ppo_loss: ") + hipGetErrorString(e));
}

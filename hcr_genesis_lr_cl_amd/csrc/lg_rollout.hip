// lg_rollout.hip -- rollout-side kernels behind include/lgrollout.h.
//
// Reference call sites replaced: rsl_rl/storage/rollout_storage.py:89-102 (add_transitions: nine copy_ launches per step),
// rsl_rl/algorithms/ppo.py:106-113 (time-out bootstrap of the reward) and rollout_storage.py:124-138 / rollout_storage_cts.py:81-114
// (compute_returns: a 24-iteration Python loop of ~8 elementwise launches each, then mean / std / normalise).  All of it is HBM-bound
// streaming work: one env per lane, consecutive lanes on consecutive envs, every array touched once.
//
// What the entry points share: `gae_kernel<G>` is the one GAE body (G = 1: lg_rollout_gae, G = 2: lg_rollout_gae_groups) behind the one
// host function `gae`; the four data movers (padded sources, start hidden states, un-padding, the mini-batch gather) take their float /
// float4 choice, element width, FastDivs and element total from one `MovePlan` built by `plan_move`, which also refuses a destination of
// 2^31 floats or more, and pick their instantiation through `by_width`; every launch ends in `launched` and sizes its grid by `grid_for`.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/lgrollout.h"

extern "C" const char *lg_last_error(void);
int lg_fail_msg(const std::string &m);   // lg_host.hip: sets the thread-local message, returns 1

// the epilogue of every entry point: what the launches just enqueued reported
static int launched(const char *fn) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : lg_fail_msg(std::string(fn) + ": " + hipGetErrorString(e));
}
// blocks of 256 lanes for `total` elements, at most `cap` (the kernels stride over the rest); the caps differ per kernel on purpose
static unsigned grid_for(long long total, long long cap) {
    const long long blocks = (total + 255) / 256;
    return (unsigned)(blocks > cap ? cap : (blocks < 1 ? 1 : blocks));
}
static const long long kMaxFlat = 0x7fffffffLL;          // the kernels index each tensor with 32 bits

struct RecordArgs {
    int n; const float *rew; const uint8_t *reset, *time_outs; const float *values; float gamma; float *rewards; uint8_t *dones;
    LgRowCopy c[LG_ROLLOUT_MAX_COPIES]; int nc;
};

__global__ __launch_bounds__(256) void rollout_record_kernel(RecordArgs a) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long long e = tid; e < a.n; e += stride) {
        float r = a.rew[e];
        if (a.time_outs && a.time_outs[e]) r += a.gamma * a.values[e];       // ppo.py:110-111
        a.rewards[e] = r;
        a.dones[e] = a.reset[e];
    }
    // row copies: each segment its own flat index space, consecutive lanes on consecutive floats of a row
    for (int s = 0; s < a.nc; s++) {
        const LgRowCopy c = a.c[s];
        const long long tot = (long long)a.n * c.width;
        for (long long i = tid; i < tot; i += stride) {
            const long long e = i / c.width;
            const int k = (int)(i - e * c.width);
            c.dst[i] = c.src[e * (long long)c.src_stride + k];
        }
    }
}

extern "C" int lg_rollout_record(int32_t n_envs, const float *rew, const uint8_t *reset, const uint8_t *time_outs, const float *values_row,
                                 float gamma, float *rewards_row, uint8_t *dones_row, const LgRowCopy *copies, int32_t n_copies, void *stream) {
    if (n_envs < 1 || !rew || !reset || !rewards_row || !dones_row) return lg_fail_msg("lg_rollout_record: null / empty argument");
    if (time_outs && !values_row) return lg_fail_msg("lg_rollout_record: the time-out bootstrap needs the value row");
    if (n_copies < 0 || n_copies > LG_ROLLOUT_MAX_COPIES || (n_copies && !copies)) return lg_fail_msg("lg_rollout_record: bad copy list");
    RecordArgs a;
    a.n = n_envs; a.rew = rew; a.reset = reset; a.time_outs = time_outs; a.values = values_row; a.gamma = gamma;
    a.rewards = rewards_row; a.dones = dones_row; a.nc = n_copies;
    long long most = n_envs;
    for (int i = 0; i < n_copies; i++) {
        if (!copies[i].src || !copies[i].dst || copies[i].width < 1 || copies[i].src_stride < copies[i].width)
            return lg_fail_msg("lg_rollout_record: bad row copy (null pointer, width < 1 or stride < width)");
        a.c[i] = copies[i];
        const long long tot = (long long)n_envs * copies[i].width;
        if (tot > most) most = tot;
    }
    hipLaunchKernelGGL(rollout_record_kernel, dim3(grid_for(most, 4096)), dim3(256), 0, (hipStream_t)stream, a);
    return launched("lg_rollout_record");
}

// ---- GAE: one env per lane, T steps backwards; per-block partial sums of the raw advantages for the normalisation ----
// (sum, sum of squares) per group: wave, then block reduction of the 2 * G doubles; one atomic per double and block
template <int G> __device__ inline void block_sums_to(double (&s)[2 * G], double *scratch) {
    for (int off = 32; off > 0; off >>= 1)
        for (int q = 0; q < 2 * G; q++) s[q] += __shfl_down(s[q], off, 64);
    __shared__ double sh[2 * G][4];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    if (l == 0)
        for (int q = 0; q < 2 * G; q++) sh[q][w] = s[q];
    __syncthreads();
    if (threadIdx.x < 2 * G) {
        double acc = 0.0;
        for (int k = 0; k < (int)(blockDim.x >> 6); k++) acc += sh[threadIdx.x][k];
        atomicAdd(&scratch[threadIdx.x], acc);
    }
}

// G = 1: the raw advantages of all envs go to adv_first (T, N, 1).  G = 2 (rollout_storage_cts.py:81-114): those of envs [0, n_first) go to
// adv_first (T, n_first, 1), the rest to adv_rest (T, N - n_first, 1); a block may hold envs of both groups, so every lane carries both
// pairs of sums (one of them zero) through the reduction.
template <int G> __global__ __launch_bounds__(256) void gae_kernel(int T, int N, int n_first, const float *__restrict__ values,
                                                                   const float *__restrict__ rewards, const uint8_t *__restrict__ dones,
                                                                   const float *__restrict__ last_values, float gamma, float lam,
                                                                   float *__restrict__ returns, float *__restrict__ adv_first,
                                                                   float *__restrict__ adv_rest, double *scratch) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    double s[2 * G] = {};
    if (e < N) {
        const bool first = G == 1 || e < n_first;
        float *__restrict__ out = first ? adv_first : adv_rest;
        const int n = G == 1 ? N : (first ? n_first : N - n_first), col = first ? e : e - n_first;
        double s1 = 0.0, s2 = 0.0;
        float adv = 0.f, next_v = last_values[e];
        for (int t = T - 1; t >= 0; t--) {
            const size_t i = (size_t)t * N + e;
            const float v = values[i];
            const float nt = 1.0f - (float)dones[i];
            const float delta = rewards[i] + nt * gamma * next_v - v;
            adv = delta + nt * gamma * lam * adv;
            const float ret = adv + v;
            returns[i] = ret;
            const float a = ret - v;                       // rollout_storage.py:137: returns - values (not `adv`: same f32 rounding as the reference)
            out[(size_t)t * n + col] = a;
            s1 += (double)a; s2 += (double)a * (double)a;
            next_v = v;
        }
        s[0] = first ? s1 : 0.0; s[1] = first ? s2 : 0.0;
        if constexpr (G == 2) { s[2] = first ? 0.0 : s1; s[3] = first ? 0.0 : s2; }
    }
    block_sums_to<G>(s, scratch);
}

__global__ __launch_bounds__(256) void adv_normalize_kernel(long long total, float *__restrict__ adv, const double *scratch) {
    const double n = (double)total;
    const double mean = scratch[0] / n;
    double var = (scratch[1] - n * mean * mean) / (n - 1.0);     // torch.std: unbiased
    if (var < 0.0) var = 0.0;
    const float m = (float)mean, inv = 1.0f / ((float)sqrt(var) + 1e-8f);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        adv[i] = (adv[i] - m) * inv;
}

// both entry points: memset of the sums, the recurrence, one normalisation per group.  groups == 1: n_first == n_envs, adv_rest unused.
static int gae(const char *fn, int groups, int32_t n_steps, int32_t n_envs, int32_t n_first, const float *values, const float *rewards,
               const uint8_t *dones, const float *last_values, float gamma, float lam, float *returns, float *adv_first, float *adv_rest,
               double *scratch, void *stream) {
    const std::string at = std::string(fn) + ": ";
    if (n_steps < 1 || n_envs < 1 || !values || !rewards || !dones || !last_values || !returns || !adv_first || (groups == 2 && !adv_rest) || !scratch)
        return lg_fail_msg(at + "null / empty argument");
    if (groups == 2 && (n_first < 1 || n_first >= n_envs)) return lg_fail_msg(at + "n_first outside [1, n_envs - 1]");
    const long long tots[2] = {(long long)n_steps * n_first, (long long)n_steps * (n_envs - n_first)};
    float *const advs[2] = {adv_first, adv_rest};
    for (int g = 0; g < groups; g++)
        if (tots[g] < 2) return lg_fail_msg(at + "the normalisation needs at least two entries" + (groups == 2 ? " per group" : ""));
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(scratch, 0, 2 * groups * sizeof(double), st);
    if (e != hipSuccess) return lg_fail_msg(at + hipGetErrorString(e));
    hipLaunchKernelGGL(groups == 2 ? gae_kernel<2> : gae_kernel<1>, dim3((n_envs + 255) / 256), dim3(256), 0, st, n_steps, n_envs, n_first, values,
                       rewards, dones, last_values, gamma, lam, returns, adv_first, adv_rest, scratch);
    for (int g = 0; g < groups; g++)
        hipLaunchKernelGGL(adv_normalize_kernel, dim3(grid_for(tots[g], 2048)), dim3(256), 0, st, tots[g], advs[g], scratch + 2 * g);
    return launched(fn);
}

extern "C" int lg_rollout_gae(int32_t n_steps, int32_t n_envs, const float *values, const float *rewards, const uint8_t *dones,
                              const float *last_values, float gamma, float lam, float *returns, float *advantages, double *scratch,
                              void *stream) {
    return gae("lg_rollout_gae", 1, n_steps, n_envs, n_envs, values, rewards, dones, last_values, gamma, lam, returns, advantages, nullptr, scratch,
               stream);
}

extern "C" int lg_rollout_gae_groups(int32_t n_steps, int32_t n_envs, int32_t n_first, const float *values, const float *rewards, const uint8_t *dones,
                                     const float *last_values, float gamma, float lam, float *returns, float *adv_first, float *adv_rest,
                                     double *scratch, void *stream) {
    return gae("lg_rollout_gae_groups", 2, n_steps, n_envs, n_first, values, rewards, dones, last_values, gamma, lam, returns, adv_first, adv_rest,
               scratch, stream);
}

// ---- recurrent policies: trajectory index, padded trajectories / masks / start hidden states, un-padding ------------------------
// Reference call sites replaced: rsl_rl/utils/utils.py:33-65 (split_and_pad_trajectories: every trajectory length to the host, one tensor
// per trajectory, pad_sequence), utils.py:67-71 (unpad_trajectories) and rollout_storage.py:203-228 (a torch.sum used as a slice bound and
// a boolean-mask gather over the whole hidden-state tensor, per mini-batch).  A trajectory starts at t = 0 and behind every done, ends at
// a done or at t = T-1; trajectories are numbered env-major, then by time.  The index is (3, capacity) int32: env, t_start, length.
#define LG_TRAJ_BLOCK 1024
#define LG_TRAJ_WAVES (LG_TRAJ_BLOCK / 64)

// exclusive prefix sum of v over the 1024-thread block (wave scan by shuffles, the 16 wave totals by the first wave); *total = block sum
__device__ inline int block_exclusive_scan(int v, int *sh, int *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(inc, off, 64); if (lane >= off) inc += o; }
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    if (w == 0) {
        const int x = lane < LG_TRAJ_WAVES ? sh[lane] : 0;
        int xi = x;
        for (int off = 1; off < LG_TRAJ_WAVES; off <<= 1) { const int o = __shfl_up(xi, off, 64); if (lane >= off) xi += o; }
        if (lane < LG_TRAJ_WAVES) sh[lane] = xi - x;
        if (lane == LG_TRAJ_WAVES - 1) sh[LG_TRAJ_WAVES] = xi;
    }
    __syncthreads();
    const int ex = sh[w] + inc - v;
    *total = sh[LG_TRAJ_WAVES];
    __syncthreads();                                   // sh is written again by the next tile
    return ex;
}

__device__ inline int block_max(int v, int *sh) {
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    int m = 0;
    for (int k = 0; k < LG_TRAJ_WAVES; k++) m = sh[k] > m ? sh[k] : m;
    return m;
}

// One workgroup; one lane per env walks its T flags (consecutive lanes on consecutive envs: coalesced, as in gae_kernel), env tiles of 1024
// with a carry.  No atomics: the numbering is the scan's, so it is the same on every call.  Latency-bound and tiny (T * N bytes in, a
// few hundred KB out): one launch that replaces a host round trip, not something to tune.
__global__ __launch_bounds__(LG_TRAJ_BLOCK) void traj_index_kernel(int T, int N, const uint8_t *__restrict__ dones, int *__restrict__ traj_offset,
                                                                   int *__restrict__ traj, int cap, int *__restrict__ header) {
    __shared__ int sh[LG_TRAJ_WAVES + 1];
    int carry = 0, longest = 0;
    for (int base = 0; base < N; base += LG_TRAJ_BLOCK) {
        const int e = base + (int)threadIdx.x;
        int cnt = 0;
        if (e < N) {
            cnt = 1;
            for (int t = 0; t < T - 1; t++) cnt += dones[(size_t)t * N + e] != 0;
        }
        int total;
        const int ex = block_exclusive_scan(cnt, sh, &total);
        if (e < N) {
            int j = carry + ex, start = 0;
            traj_offset[e] = j;
            for (int t = 0; t < T; t++) {
                if (t == T - 1 || dones[(size_t)t * N + e]) {
                    const int len = t - start + 1;
                    if (j < cap) { traj[j] = e; traj[(size_t)cap + j] = start; traj[2 * (size_t)cap + j] = len; }
                    longest = len > longest ? len : longest;
                    j++;
                    start = t + 1;
                }
            }
        }
        carry += total;
    }
    longest = block_max(longest, sh);
    if (threadIdx.x == 0) { traj_offset[N] = carry; header[0] = carry; header[1] = longest; }
}

// The same index from a (T, n_traj) mask alone (what unpad_trajectories is given): length = the column's count, and because the
// trajectories of one env fill its T steps in order, the running sum of the lengths is env * T + t_start.  header = (steps covered, longest);
// a trajectory that would run past its env's last step (a mask no rollout produces) reports INT32_MAX as the longest, so the caller sees it.
__global__ __launch_bounds__(LG_TRAJ_BLOCK) void mask_index_kernel(int T, int n_traj, const uint8_t *__restrict__ masks, int *__restrict__ traj,
                                                                   int cap, int *__restrict__ header) {
    __shared__ int sh[LG_TRAJ_WAVES + 1];
    int carry = 0, longest = 0;
    for (int base = 0; base < n_traj; base += LG_TRAJ_BLOCK) {
        const int j = base + (int)threadIdx.x;
        int len = 0;
        if (j < n_traj)
            for (int t = 0; t < T; t++) len += masks[(size_t)t * n_traj + j] != 0;
        int total;
        const int p = carry + block_exclusive_scan(len, sh, &total);
        if (j < n_traj && j < cap) { traj[j] = p / T; traj[(size_t)cap + j] = p % T; traj[2 * (size_t)cap + j] = len; }
        const int seen = p % T + len > T ? INT32_MAX : len;
        longest = seen > longest ? seen : longest;
        carry += total;
    }
    longest = block_max(longest, sh);
    if (threadIdx.x == 0) { header[0] = carry; header[1] = longest; }
}

// Division of a flat index below 2^31 by a divisor fixed per launch: q = (n * m) >> sh with m = ceil(2^sh / d), sh = 31 + ceil(log2 d).
// Exact: m = (2^sh + e) / d with 0 <= e < d <= 2^(sh - 31), so n * m / 2^sh = n / d + n * e / (d * 2^sh) and the excess is below 1 / d for
// n < 2^31.  The gathers split every flat index twice, and two of the hardware's ~20-instruction u32 divisions per 4-byte element bind
// the scalar path by arithmetic instead of HBM.
struct FastDiv { unsigned m, sh; };
static FastDiv fast_div(unsigned d) {
    unsigned s = 0;
    while ((1ull << s) < d) s++;
    FastDiv f;
    f.sh = 31 + s;
    f.m = (unsigned)(((1ull << f.sh) + d - 1) / d);
    return f;
}
__device__ inline unsigned div_by(unsigned n, FastDiv f) { return (unsigned)(((unsigned long long)n * f.m) >> f.sh); }
// How one data mover walks its destination: a flat index over `outer` x `inner` rows of `dv` elements, each a float4 where width, stride and
// both pointers allow and a float otherwise; i / by_row is the outer index, (i % row) / by_w the inner one.
struct MovePlan { unsigned vec, dv, total; FastDiv by_row, by_w; };

static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// false: the destination (outer, inner, width) has 2^31 floats or more, which the 32-bit index does not reach.  `most` keeps the largest total.
static bool plan_move(MovePlan &p, bool may_vec, int width, int stride, const void *src, const void *dst, long long outer, long long inner,
                      long long &most) {
    if (outer * inner * width > kMaxFlat) return false;
    p.vec = may_vec && width % 4 == 0 && stride % 4 == 0 && aligned16(src) && aligned16(dst);
    p.dv = (unsigned)width / (p.vec ? 4 : 1);
    p.total = (unsigned)(outer * inner) * p.dv;
    p.by_row = fast_div((unsigned)inner * p.dv);
    p.by_w = fast_div(p.dv);
    if (p.total > most) most = p.total;
    return true;
}

// f(float4()) where the plan moves float4, f(float()) otherwise: the one place that turns `vec` into a type
template <typename F> __host__ __device__ inline void by_width(unsigned vec, F &&f) {
    if (vec) f(float4());
    else f(float());
}

// one tensor of lg_rollout_pad; layers == 0: a padded source (T, N, width), layers > 0: the start states of a (T, layers, N, width) tensor
struct PadSegment { LgRowCopy c; int layers; MovePlan p; };
struct PadArgs {
    int T, N, n_traj, cap; const int *traj; uint8_t *masks; FastDiv by_traj;
    PadSegment seg[2 * LG_ROLLOUT_MAX_COPIES]; int ns;
};

__device__ inline void zero_of(float &v) { v = 0.f; }
__device__ inline void zero_of(float4 &v) { v = make_float4(0.f, 0.f, 0.f, 0.f); }

// HID false: padded[t', j, :] = src[t_start_j + t', env_j, :] for t' < length_j, else 0.
// HID true:  hid[l, j, :] = saved[t_start_j, l, env_j, :]: the state the policy held when trajectory j began.
// Gather: the flat index runs over the destination, every element is written once (zeros included), consecutive lanes on consecutive
// elements of a row.  Sizes < 2^31 (plan_move refuses anything larger).
template <typename V, bool HID> __device__ inline void pad_segment(const PadArgs &a, const PadSegment &g, unsigned tid, unsigned stride) {
    constexpr unsigned W = sizeof(V) / sizeof(float);
    const unsigned dv = g.p.dv, sv = (unsigned)g.c.src_stride / W, row = (unsigned)a.n_traj * dv, tot = g.p.total;
    const V *__restrict__ src = (const V *)g.c.src;
    V *__restrict__ dst = (V *)g.c.dst;
    const int *env = a.traj, *start = a.traj + a.cap, *len = a.traj + 2 * (size_t)a.cap;
    for (unsigned i = tid; i < tot; i += stride) {
        const unsigned o = div_by(i, g.p.by_row), r = i - o * row, j = div_by(r, g.p.by_w), k = r - j * dv;
        V v;
        zero_of(v);
        const int t = start[j] + (HID ? 0 : (int)o), e = env[j];
        if ((HID || (int)o < len[j]) && t < a.T && e < a.N)
            v = src[(HID ? ((size_t)t * g.layers + o) * a.N + e : (size_t)t * a.N + e) * sv + k];
        dst[i] = v;
    }
}

__global__ __launch_bounds__(256) void rollout_pad_kernel(PadArgs a) {
    const unsigned stride = gridDim.x * blockDim.x, tid = blockIdx.x * blockDim.x + threadIdx.x;
    for (int s = 0; s < a.ns; s++) {
        const PadSegment &g = a.seg[s];
        by_width(g.p.vec, [&](auto v) {
            if (g.layers) pad_segment<decltype(v), true>(a, g, tid, stride);
            else pad_segment<decltype(v), false>(a, g, tid, stride);
        });
    }
    if (a.masks) {                                      // (T, n_traj) even where the longest trajectory is shorter than T (utils.py:64)
        const int *len = a.traj + 2 * (size_t)a.cap;
        const unsigned tot = (unsigned)a.T * (unsigned)a.n_traj;
        for (unsigned i = tid; i < tot; i += stride) {
            const unsigned t = div_by(i, a.by_traj), j = i - t * (unsigned)a.n_traj;
            a.masks[i] = (int)t < len[j];
        }
    }
}

// the inverse: dst[t_start_j + t', env_j, :] = padded[t', j, :] for t' < length_j.  The trajectories tile the (T, N) grid, so this
// scatter writes every destination element exactly once; the bounds test keeps a malformed mask from writing outside dst.
template <typename V> __global__ __launch_bounds__(256) void rollout_unpad_kernel(int T, int N, int n_traj, int cap, const int *__restrict__ traj,
                                                                                  const V *__restrict__ src, V *__restrict__ dst, MovePlan p) {
    const unsigned stride = gridDim.x * blockDim.x, dv = p.dv, row = (unsigned)n_traj * dv;
    const int *env = traj, *start = traj + cap, *len = traj + 2 * (size_t)cap;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < p.total; i += stride) {
        const unsigned tp = div_by(i, p.by_row), r = i - tp * row, j = div_by(r, p.by_w), k = r - j * dv;
        const int t = start[j] + (int)tp, e = env[j];
        if ((int)tp < len[j] && t < T && e < N) dst[((size_t)t * N + e) * dv + k] = src[i];
    }
}

extern "C" int lg_rollout_traj_index(int32_t n_steps, int32_t n_envs, const uint8_t *dones, int32_t *traj_offset, int32_t *traj,
                                     int32_t capacity, int32_t *header, void *stream) {
    if (n_steps < 1 || n_envs < 1 || !dones || !traj_offset || !traj || !header) return lg_fail_msg("lg_rollout_traj_index: null / empty argument");
    if ((long long)n_steps * n_envs > kMaxFlat) return lg_fail_msg("lg_rollout_traj_index: n_steps * n_envs overflows 32 bits");
    if (capacity < n_envs) return lg_fail_msg("lg_rollout_traj_index: capacity below n_envs (every env has at least one trajectory)");
    hipLaunchKernelGGL(traj_index_kernel, dim3(1), dim3(LG_TRAJ_BLOCK), 0, (hipStream_t)stream, n_steps, n_envs, dones, traj_offset, traj, capacity,
                       header);
    return launched("lg_rollout_traj_index");
}

extern "C" int lg_rollout_mask_index(int32_t n_steps, int32_t n_traj, const uint8_t *masks, int32_t *traj, int32_t capacity, int32_t *header,
                                     void *stream) {
    if (n_steps < 1 || n_traj < 1 || !masks || !traj || !header) return lg_fail_msg("lg_rollout_mask_index: null / empty argument");
    if ((long long)n_steps * n_traj > kMaxFlat) return lg_fail_msg("lg_rollout_mask_index: n_steps * n_traj overflows 32 bits");
    if (capacity < n_traj) return lg_fail_msg("lg_rollout_mask_index: capacity below n_traj");
    hipLaunchKernelGGL(mask_index_kernel, dim3(1), dim3(LG_TRAJ_BLOCK), 0, (hipStream_t)stream, n_steps, n_traj, masks, traj, capacity, header);
    return launched("lg_rollout_mask_index");
}

extern "C" int lg_rollout_pad(int32_t n_steps, int32_t n_envs, const int32_t *traj, int32_t capacity, int32_t n_traj, int32_t rows,
                              const LgRowCopy *sources, int32_t n_sources, const LgRowCopy *hidden, const int32_t *hidden_layers,
                              int32_t n_hidden, uint8_t *masks, void *stream) {
    if (n_steps < 1 || n_envs < 1 || !traj || n_traj < 1 || rows < 1) return lg_fail_msg("lg_rollout_pad: null / empty argument");
    if ((long long)n_steps * n_envs > kMaxFlat) return lg_fail_msg("lg_rollout_pad: n_steps * n_envs overflows 32 bits");
    if (capacity < n_traj) return lg_fail_msg("lg_rollout_pad: index capacity below n_traj");
    if (rows > n_steps) return lg_fail_msg("lg_rollout_pad: more padded rows than steps");
    if (n_sources < 0 || n_sources > LG_ROLLOUT_MAX_COPIES || (n_sources && !sources)) return lg_fail_msg("lg_rollout_pad: bad source list");
    if (n_hidden < 0 || n_hidden > LG_ROLLOUT_MAX_COPIES || (n_hidden && (!hidden || !hidden_layers))) return lg_fail_msg("lg_rollout_pad: bad hidden-state list");
    if (!n_sources && !n_hidden && !masks) return lg_fail_msg("lg_rollout_pad: nothing to write");
    PadArgs a;
    a.T = n_steps; a.N = n_envs; a.n_traj = n_traj; a.cap = capacity; a.traj = traj; a.masks = masks;
    a.ns = n_sources + n_hidden; a.by_traj = fast_div((unsigned)n_traj);
    long long most = masks ? (long long)n_steps * n_traj : 1;
    if (most > kMaxFlat) return lg_fail_msg("lg_rollout_pad: mask larger than 2^31 entries");
    for (int i = 0; i < a.ns; i++) {
        const bool hid = i >= n_sources;
        PadSegment &g = a.seg[i];
        g.c = hid ? hidden[i - n_sources] : sources[i];
        g.layers = hid ? hidden_layers[i - n_sources] : 0;
        if (!hid && (!g.c.src || !g.c.dst || g.c.width < 1 || g.c.src_stride < g.c.width))
            return lg_fail_msg("lg_rollout_pad: bad source (null pointer, width < 1 or stride < width)");
        if (hid && (!g.c.src || !g.c.dst || g.c.width < 1 || g.c.src_stride != g.c.width || g.layers < 1))
            return lg_fail_msg("lg_rollout_pad: bad hidden state (null pointer, width < 1, layers < 1 or rows not contiguous)");
        if (!plan_move(g.p, true, g.c.width, g.c.src_stride, g.c.src, g.c.dst, hid ? g.layers : rows, n_traj, most))
            return lg_fail_msg("lg_rollout_pad: tensor larger than 2^31 entries");
    }
    hipLaunchKernelGGL(rollout_pad_kernel, dim3(grid_for(most, 4096)), dim3(256), 0, (hipStream_t)stream, a);
    return launched("lg_rollout_pad");
}

extern "C" int lg_rollout_unpad(int32_t n_steps, int32_t n_envs, const int32_t *traj, int32_t capacity, int32_t n_traj, int32_t rows,
                                const float *padded, float *dst, int32_t width, void *stream) {
    if (n_steps < 1 || n_envs < 1 || !traj || n_traj < 1 || rows < 1 || !padded || !dst) return lg_fail_msg("lg_rollout_unpad: null / empty argument");
    if (width < 1) return lg_fail_msg("lg_rollout_unpad: width < 1");
    if (capacity < n_traj) return lg_fail_msg("lg_rollout_unpad: index capacity below n_traj");
    MovePlan p;
    long long most = 0;
    if ((long long)n_steps * n_envs > kMaxFlat || !plan_move(p, true, width, width, padded, dst, rows, n_traj, most))
        return lg_fail_msg("lg_rollout_unpad: tensor larger than 2^31 entries");
    by_width(p.vec, [&](auto v) {
        using V = decltype(v);
        hipLaunchKernelGGL(rollout_unpad_kernel<V>, dim3(grid_for(most, 4096)), dim3(256), 0, (hipStream_t)stream, n_steps, n_envs, n_traj, capacity, traj,
                           (const V *)padded, (V *)dst, p);
    });
    return launched("lg_rollout_unpad");
}

// ---- mini-batches: every tensor of one mini-batch gathered in one launch -------------------------------------------------------------
// Reference call sites replaced: the 9 index gathers per mini-batch of rollout_storage.py:170-186 and the 11 to 16 of rollout_storage_ee.py:
// 141-151, _ts.py:103-114, _dreamwaq.py:108-120 and _cts.py:160-177 (with the `[:, a:b].flatten(0, 1)` copies of _cts.py:126-140, made on
// every call).  blockIdx.y is the item; within an item the flat index runs over the destination, consecutive lanes on consecutive floats
// of a row, so every destination element is written once and a row of the source is read by neighbouring lanes.
struct GatherArgs {
    LgGatherItem it[LG_ROLLOUT_MAX_GATHER];
    MovePlan p[LG_ROLLOUT_MAX_GATHER];                                       // inner = 1: rows of dv elements
    FastDiv by_group[LG_ROLLOUT_MAX_GATHER];
};

__device__ inline void load_of(float &v, const float *src, size_t at) { v = src[at]; }
__device__ inline void load_of(float4 &v, const float4 *src, size_t at) { v = src[at]; }
__device__ inline void load_of(float &v, const uint8_t *src, size_t at) { v = 1.0f - (float)src[at]; }

// S: the source's element type, V: what moves (float4 only with S = float4)
template <typename S, typename V> __device__ inline void gather_item(const LgGatherItem &c, const MovePlan &p, FastDiv by_group) {
    constexpr unsigned W = sizeof(V) / sizeof(float);
    const unsigned dv = p.dv, sv = (unsigned)c.src_stride / W, tot = p.total;
    const unsigned stride = gridDim.x * blockDim.x, group = (unsigned)c.group;
    const bool plain = c.group == c.n_envs;                                   // env_offset is 0 then: the index is the source row
    const S *__restrict__ src = (const S *)c.src;
    V *__restrict__ dst = (V *)c.dst;
    const int64_t *__restrict__ index = c.index;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += stride) {
        const unsigned j = div_by(i, p.by_w), k = i - j * dv;
        unsigned r = (unsigned)index[j];
        if (!plain) { const unsigned t = div_by(r, by_group); r = t * (unsigned)c.n_envs + (unsigned)c.env_offset + (r - t * group); }
        V v;
        load_of(v, src, (size_t)r * sv + k);
        dst[i] = v;
    }
}

__global__ __launch_bounds__(256) void rollout_gather_kernel(GatherArgs a) {
    const int s = blockIdx.y;
    const LgGatherItem &c = a.it[s];
    if (c.kind == LG_GATHER_NOT_U8) gather_item<uint8_t, float>(c, a.p[s], a.by_group[s]);
    else by_width(a.p[s].vec, [&](auto v) { gather_item<decltype(v), decltype(v)>(c, a.p[s], a.by_group[s]); });
}

extern "C" int lg_rollout_gather(const LgGatherItem *items, int32_t n_items, void *stream) {
    if (!items || n_items < 1 || n_items > LG_ROLLOUT_MAX_GATHER) return lg_fail_msg("lg_rollout_gather: bad item list (null, empty or more than 16 items)");
    GatherArgs a;
    long long most = 0;
    for (int i = 0; i < n_items; i++) {
        const LgGatherItem &c = items[i];
        const std::string at = "lg_rollout_gather: item " + std::to_string(i) + ": ";
        if (c.rows > 0 && (!c.src || !c.dst || !c.index)) return lg_fail_msg(at + "null pointer");
        if (c.width < 1 || c.src_stride < c.width) return lg_fail_msg(at + "width < 1 or stride < width");
        if (c.kind != LG_GATHER_F32 && c.kind != LG_GATHER_NOT_U8) return lg_fail_msg(at + "unknown kind");
        if (c.group < 1 || c.env_offset < 0 || (long long)c.env_offset + c.group > c.n_envs) return lg_fail_msg(at + "env window outside the envs (group < 1 or env_offset + group > n_envs)");
        if (c.rows < 0) return lg_fail_msg(at + "rows < 0");
        if (!plan_move(a.p[i], c.kind == LG_GATHER_F32, c.width, c.src_stride, c.src, c.dst, c.rows, 1, most))
            return lg_fail_msg(at + "destination of 2^31 elements or more");
        a.it[i] = c;
        a.by_group[i] = fast_div((unsigned)c.group);
    }
    if (most == 0) return 0;                              // every item empty: nothing to write
    // at most 1024 blocks x 16 items: enough lanes in flight to cover the gathers' latency
    hipLaunchKernelGGL(rollout_gather_kernel, dim3(grid_for(most, 1024), (unsigned)n_items), dim3(256), 0, (hipStream_t)stream, a);
    return launched("lg_rollout_gather");
}

// lg_runner.hip -- the on-policy runner's per-step book-keeping behind include/lgrunner.h.
//
// Reference call sites replaced: rsl_rl/runners/on_policy_runner.py:128-136 (cur_reward_sum += rewards, (dones > 0).nonzero(), two
// .cpu().numpy().tolist() into deque(maxlen=100): a device-to-host round trip per env step with logging on) and the per-step
// ep_infos.append(infos['episode']) whose values :178-187 average at log time.  Both kernels are latency-bound and tiny (a few N floats):
// they exist to take host work and synchronisation out of the rollout loop, not to be tuned.  lg_rollout.hip's traj_index_kernel is the
// model: one workgroup, env tiles of 1024 with a carried block scan, no atomics, so the numbering is the scan's on every call.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "../../include/lgrunner.h"

int lg_fail_msg(const std::string &m);   // lg_host.hip: sets the thread-local message, returns 1

static int launched(const char *fn) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : lg_fail_msg(std::string(fn) + ": " + hipGetErrorString(e));
}

#define LG_RUNNER_WAVES (LG_RUNNER_THREADS / 64)

// exclusive prefix sum of v over the 1024-lane block (wave scan by shuffles, the 16 wave totals by the first wave); *total = block sum
__device__ inline int runner_exclusive_scan(int v, int *sh, int *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(inc, off, 64); if (lane >= off) inc += o; }
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    if (w == 0) {
        const int x = lane < LG_RUNNER_WAVES ? sh[lane] : 0;
        int xi = x;
        for (int off = 1; off < LG_RUNNER_WAVES; off <<= 1) { const int o = __shfl_up(xi, off, 64); if (lane >= off) xi += o; }
        if (lane < LG_RUNNER_WAVES) sh[lane] = xi - x;
        if (lane == LG_RUNNER_WAVES - 1) sh[LG_RUNNER_WAVES] = xi;
    }
    __syncthreads();
    const int ex = sh[w] + inc - v;
    *total = sh[LG_RUNNER_WAVES];
    __syncthreads();                                   // sh is written again by the next tile
    return ex;
}

// One workgroup.  Pass 1 counts the dones (the ring drops the pushes that the same call would overwrite, so the total comes first); pass
// 2 walks the env tiles again with the carried rank: add, push in env order, zero, store.  Every lane reads *count before the barriers of
// pass 1, lane 0 writes it behind those of pass 2.
__global__ __launch_bounds__(LG_RUNNER_THREADS) void episode_stats_kernel(int N, const float *__restrict__ rewards, const uint8_t *__restrict__ dones,
                                                                          float *__restrict__ cur_sum, float *__restrict__ cur_len,
                                                                          float *__restrict__ ring_reward, float *__restrict__ ring_length, int cap,
                                                                          long long *count) {
    __shared__ int sh[LG_RUNNER_WAVES + 1];
    const long long count0 = *count;
    int mine = 0;
    for (int e = (int)threadIdx.x; e < N; e += LG_RUNNER_THREADS) mine += dones[e] != 0;
    int n_done;
    runner_exclusive_scan(mine, sh, &n_done);
    const int first_kept = n_done - cap;               // ranks below it would be overwritten by this call's own later pushes
    int carry = 0;
    for (int base = 0; base < N; base += LG_RUNNER_THREADS) {
        const int e = base + (int)threadIdx.x;
        int d = 0;
        float s = 0.f, l = 0.f;
        if (e < N) {
            s = cur_sum[e] + rewards[e];
            l = cur_len[e] + 1.0f;
            d = dones[e] != 0;
        }
        int total;
        const int ex = runner_exclusive_scan(d, sh, &total);
        if (e < N) {
            if (d) {
                const int rank = carry + ex;
                if (rank >= first_kept) {
                    const int slot = (int)((count0 + (long long)rank) % (long long)cap);
                    ring_reward[slot] = s;
                    ring_length[slot] = l;
                }
                s = 0.f;
                l = 0.f;
            }
            cur_sum[e] = s;
            cur_len[e] = l;
        }
        carry += total;
    }
    if (threadIdx.x == 0) *count = count0 + (long long)n_done;
}

// One workgroup per row: lane j adds the envs j, j + 256, ... that reset at `step` in float64, the lane sums by a fixed binary tree.
__global__ __launch_bounds__(LG_RUNNER_INFO_THREADS) void episode_info_kernel(int N, int rows_a, const float *__restrict__ sums_a, int stride_a,
                                                                              const float *__restrict__ sums_b, int stride_b,
                                                                              const int *__restrict__ done_step, int step, double inv_len,
                                                                              double *__restrict__ last, double *__restrict__ acc, long long *n_acc) {
    __shared__ double sh_sum[LG_RUNNER_INFO_THREADS];
    __shared__ int sh_cnt[LG_RUNNER_INFO_THREADS];
    const int r = (int)blockIdx.x, tid = (int)threadIdx.x;
    const float *row = r < rows_a ? sums_a + (size_t)r * (size_t)stride_a : sums_b + (size_t)(r - rows_a) * (size_t)stride_b;
    double s = 0.0;
    int c = 0;
    for (int e = tid; e < N; e += LG_RUNNER_INFO_THREADS)
        if (done_step[e] == step) { s += (double)row[e]; c++; }
    sh_sum[tid] = s;
    sh_cnt[tid] = c;
    __syncthreads();
    for (int off = LG_RUNNER_INFO_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) { sh_sum[tid] += sh_sum[tid + off]; sh_cnt[tid] += sh_cnt[tid + off]; }
        __syncthreads();
    }
    if (tid == 0) {
        double v = last[r];
        if (sh_cnt[0] > 0) { v = sh_sum[0] / (double)sh_cnt[0] * inv_len; last[r] = v; }
        acc[r] += v;
        if (r == 0) *n_acc += 1;
    }
}

extern "C" int lg_runner_episode_stats(int32_t n, const float *rewards, const uint8_t *dones, float *cur_reward_sum, float *cur_episode_length,
                                       float *ring_reward, float *ring_length, int32_t cap, int64_t *count, void *stream) {
    if (n < 1) return lg_fail_msg("lg_runner_episode_stats: n < 1");
    if (cap < 1) return lg_fail_msg("lg_runner_episode_stats: cap < 1");
    if (!rewards || !dones || !cur_reward_sum || !cur_episode_length || !ring_reward || !ring_length || !count)
        return lg_fail_msg("lg_runner_episode_stats: null argument");
    hipLaunchKernelGGL(episode_stats_kernel, dim3(1), dim3(LG_RUNNER_THREADS), 0, (hipStream_t)stream, n, rewards, dones, cur_reward_sum,
                       cur_episode_length, ring_reward, ring_length, cap, (long long *)count);
    return launched("lg_runner_episode_stats");
}

extern "C" int lg_runner_episode_info(int32_t n, int32_t rows_a, const float *sums_a, int32_t stride_a, int32_t rows_b, const float *sums_b,
                                      int32_t stride_b, const int32_t *done_step, int32_t step, double inv_episode_length_s, double *last,
                                      double *acc, int64_t *n_acc, void *stream) {
    if (n < 1) return lg_fail_msg("lg_runner_episode_info: n < 1");
    if (rows_a < 1 || rows_b < 0 || (long long)rows_a + rows_b > LG_RUNNER_MAX_ROWS)
        return lg_fail_msg("lg_runner_episode_info: rows_a < 1, rows_b < 0 or more than LG_RUNNER_MAX_ROWS rows");
    if (!sums_a || (rows_b > 0 && !sums_b) || !done_step || !last || !acc || !n_acc) return lg_fail_msg("lg_runner_episode_info: null argument");
    if (stride_a < n || (rows_b > 0 && stride_b < n)) return lg_fail_msg("lg_runner_episode_info: row stride below n");
    hipLaunchKernelGGL(episode_info_kernel, dim3((unsigned)(rows_a + rows_b)), dim3(LG_RUNNER_INFO_THREADS), 0, (hipStream_t)stream, n, rows_a, sums_a,
                       stride_a, sums_b, stride_b, done_step, step, inv_episode_length_s, last, acc, (long long *)n_acc);
    return launched("lg_runner_episode_info");
}

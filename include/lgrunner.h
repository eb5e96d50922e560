/* lgrunner.h -- C ABI of the on-policy runner's per-step book-keeping (rsl_rl/runners/on_policy_runner.py:126-136 and the episode-info
 * mean of :178-187) as two HIP kernels, so that a rollout with logging on issues no device-to-host copy.  Same conventions as
 * lgrollout.h: plain device pointers, sizes, the caller's HIP stream as void*; 0 on success, otherwise non-zero with the message in
 * lgsim.h's last-error call; nothing is allocated, nothing synchronised.  All state is the caller's and lives on the device.
 *
 * Conventions:
 *   - One workgroup of LG_RUNNER_THREADS lanes per launch (lg_runner_episode_info: one per row).  No atomics, no hand-off between
 *     workgroups, every sum in a fixed order: two calls on the same inputs and state give the same bits.
 *   - Non-finite rewards and sums pass through unchanged.
 */
#ifndef LGRUNNER_H
#define LGRUNNER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_RUNNER_THREADS 1024      /* lanes of lg_runner_episode_stats' one workgroup: the env tile of its carried scan */
#define LG_RUNNER_INFO_THREADS 256  /* lanes of each row's workgroup of lg_runner_episode_info: the leaves of its float64 tree */
#define LG_RUNNER_MAX_ROWS 1024     /* rows of lg_runner_episode_info, both blocks together */

/* One env step of on_policy_runner.py:130-136:
 *   cur_reward_sum[e] += rewards[e];  cur_episode_length[e] += 1        (single float32 adds: the reference's own operations)
 *   every env with dones[e] != 0, in ASCENDING env order, pushes (cur_reward_sum[e], cur_episode_length[e]) to the ring and zeroes both
 *   *count += n_done
 * The ring is collections.deque(maxlen = cap): push k of this call (k = 0 .. n_done - 1, env order) lands in slot (*count + k) % cap, and
 * where one call finishes more than cap episodes only the last cap of them are written (the others would be overwritten within the call;
 * they are counted).  The oldest live entry is slot *count % cap once *count >= cap, else slot 0; min(*count, cap) entries are live.
 * rewards (n) f32; dones (n) uint8 / bool bytes; cur_reward_sum, cur_episode_length (n) f32; ring_reward, ring_length (cap) f32; count: one
 * int64.  Refused before the launch: n < 1, cap < 1, a null pointer. */
int lg_runner_episode_stats(int32_t n, const float *rewards, const uint8_t *dones, float *cur_reward_sum, float *cur_episode_length,
                            float *ring_reward, float *ring_length, int32_t cap, int64_t *count, void *stream);

/* One env step of the episode-info log (legged_robot.py:128-138 as the step kernels snapshot it, on_policy_runner.py:129, 178-187):
 *   if any env has done_step[e] == step:   last[r] = (sum over those envs of done_sums[r][e]) / (their number) * inv_episode_length_s
 *   otherwise last[r] keeps its value (the reference leaves the previous dict in infos); before any reset it is the caller's zeros
 *   acc[r] += last[r];   *n_acc += 1
 * so that acc[r] / *n_acc at log time is the reference's mean over the per-step values it appended.  Rows r = 0 .. rows_a - 1 come from
 * sums_a ((rows_a, n) f32, stride_a floats between rows, >= n), rows rows_a .. rows_a + rows_b - 1 from sums_b likewise (the constraint
 * counters of go2_cat; rows_b = 0: no second block, its pointer is not looked at).  The sum runs in float64: lane j of the row's workgroup
 * adds the envs j, j + LG_RUNNER_INFO_THREADS, ... in ascending order and the lane sums are added by a fixed binary tree.
 * done_step (n) int32; last, acc (rows_a + rows_b) f64; n_acc one int64.  Refused before the launch: n < 1, rows_a < 1, rows_b < 0,
 * rows_a + rows_b > LG_RUNNER_MAX_ROWS, a stride below n, a null pointer. */
int lg_runner_episode_info(int32_t n, int32_t rows_a, const float *sums_a, int32_t stride_a, int32_t rows_b, const float *sums_b,
                           int32_t stride_b, const int32_t *done_step, int32_t step, double inv_episode_length_s, double *last, double *acc,
                           int64_t *n_acc, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LGRUNNER_H */

/* lgrollout.h -- C ABI of the rollout-side fusion: the per-step record of the reference's
 * RolloutStorage.add_transitions (rsl_rl/storage/rollout_storage.py:89-102) and its compute_returns
 * (rollout_storage.py:124-138) as HIP kernels.  Same conventions as lgsim.h: plain device pointers, sizes, the caller's HIP
 * stream as void*; 0 on success, otherwise non-zero with the message in lgsim.h's last-error call.  All storage tensors are the reference's:
 * (T, N, width) float32 row-major, dones (T, N, 1) uint8.
 */
#ifndef LGROLLOUT_H
#define LGROLLOUT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_ROLLOUT_MAX_COPIES 8

/* one strided row copy of lg_rollout_record: dst[e * width + k] = src[e * src_stride + k], k < width */
typedef struct LgRowCopy {
    const float *src;
    float *dst;
    int32_t width;
    int32_t src_stride;   /* floats between consecutive envs in src (history windows are strided views) */
} LgRowCopy;

/* One step's transition written into row `t` of the storage in ONE launch (the reference issues nine copy_ calls,
 * rollout_storage.py:92-100, after the bootstrap of rsl_rl/algorithms/ppo.py:106-113):
 *   rewards_row[e] = rew[e] + gamma * values_row[e] * time_outs[e]      (time_outs may be NULL: no bootstrap)
 *   dones_row[e]   = reset[e]
 *   and up to LG_ROLLOUT_MAX_COPIES strided row copies (observations, critic observations, labels ...).
 * rew: (N) f32, reset / time_outs: (N) uint8, values_row / rewards_row: (N) f32 rows of the (T, N, 1) tensors. */
int lg_rollout_record(int32_t n_envs, const float *rew, const uint8_t *reset, const uint8_t *time_outs, const float *values_row,
                      float gamma, float *rewards_row, uint8_t *dones_row, const LgRowCopy *copies, int32_t n_copies, void *stream);

/* Generalised advantage estimation over a finished rollout plus the advantage normalisation, rollout_storage.py:124-138:
 *   for t = T-1 .. 0:  next_v = t == T-1 ? last_values : values[t+1];  nt = 1 - dones[t]
 *                      delta = rewards[t] + nt * gamma * next_v - values[t];  adv = delta + nt * gamma * lam * adv
 *                      returns[t] = adv + values[t]
 *   advantages = returns - values;  advantages = (advantages - mean) / (std + 1e-8)   (std unbiased, over all T * N entries)
 * One thread per env walks its T steps (coalesced over envs); mean / std by one block reduction pass in f64.
 * scratch: device buffer of at least 2 doubles (sum, sum of squares). */
int lg_rollout_gae(int32_t n_steps, int32_t n_envs, const float *values, const float *rewards, const uint8_t *dones,
                   const float *last_values, float gamma, float lam, float *returns, float *advantages, double *scratch, void *stream);

/* ---- recurrent policies (rollout_storage.py:187-236, rsl_rl/utils/utils.py:33-71) -------------------------------------------------
 * A trajectory starts at t = 0 and behind every done, and ends at a done or at t = T-1; trajectories are numbered env-major, then by
 * time (the reference's transpose(1, 0) flattening).  The trajectory index `traj` is (3, capacity) int32: row 0 the env, row 1 t_start,
 * row 2 the length of each trajectory. */

/* dones (T, N, 1) uint8 -> traj_offset[N + 1] (first trajectory of every env; [N] = n_traj), traj (entries at or beyond capacity are
 * not written), header = (n_traj, longest length).  capacity >= N; T * N always suffices.  One workgroup, no atomics: the numbering
 * is the same on every call. */
int lg_rollout_traj_index(int32_t n_steps, int32_t n_envs, const uint8_t *dones, int32_t *traj_offset, int32_t *traj, int32_t capacity,
                          int32_t *header, void *stream);

/* The same index from a trajectory mask (T, n_traj) uint8 / bool alone: the trajectories of one env fill its T steps in order, so the
 * running sum of the lengths is env * T + t_start.  header = (steps covered = T * envs, longest length; INT32_MAX if a trajectory would
 * run past its env's last step, which no mask of a rollout does). */
int lg_rollout_mask_index(int32_t n_steps, int32_t n_traj, const uint8_t *masks, int32_t *traj, int32_t capacity, int32_t *header,
                          void *stream);

/* One launch, every destination element written exactly once (no memset needed):
 *   sources[i]: src (T, N, width) with src_stride floats between envs (rows of T are N * src_stride apart), dst (rows, n_traj, width):
 *               dst[t', j, :] = src[t_start_j + t', env_j, :] if t' < length_j else 0         (rows = the longest length, <= T)
 *   hidden[i]:  src (T, hidden_layers[i], N, width) contiguous, dst (hidden_layers[i], n_traj, width): dst[l, j, :] = src[t_start_j, l, env_j, :]
 *   masks:      (T, n_traj) uint8, masks[t, j] = t < length_j; may be NULL
 * float4 moves where width, stride and the pointers allow, scalar otherwise.  Each destination must stay below 2^31 elements. */
int lg_rollout_pad(int32_t n_steps, int32_t n_envs, const int32_t *traj, int32_t capacity, int32_t n_traj, int32_t rows,
                   const LgRowCopy *sources, int32_t n_sources, const LgRowCopy *hidden, const int32_t *hidden_layers, int32_t n_hidden,
                   uint8_t *masks, void *stream);

/* The inverse of one source of lg_rollout_pad: dst[t_start_j + t', env_j, :] = padded[t', j, :] for t' < length_j; padded (rows, n_traj,
 * width), dst (T, N, width), both contiguous.  With an index that tiles the (T, N) grid every element of dst is written exactly once. */
int lg_rollout_unpad(int32_t n_steps, int32_t n_envs, const int32_t *traj, int32_t capacity, int32_t n_traj, int32_t rows,
                     const float *padded, float *dst, int32_t width, void *stream);

/* ---- mini-batches (rollout_storage.py:148-186 and the generators of rollout_storage_ee / _ts / _cts / _dreamwaq.py) -----------------
 * One item of lg_rollout_gather: dst (rows, width) float32 contiguous, dst[j, :] = f(src[row(index[j]), :]) with
 *   row(r) = (r / group) * n_envs + env_offset + r % group
 * so that index r addresses x[:, env_offset : env_offset + group].flatten(0, 1)[r] of a (T, n_envs, width) tensor without the flattened
 * copy; a plain gather is group = n_envs, env_offset = 0.  src_stride is the distance between consecutive source rows, in elements.
 * kind LG_GATHER_F32: src float32, f(x) = x.  kind LG_GATHER_NOT_U8: src uint8, f(x) = 1.0f - x (the `terminated_batch` of the
 * explicit-estimator, teacher-student and DreamWaQ generators).  index is int64 (what torch.randperm yields); its values must address
 * rows inside src and stay below 2^31: they are NOT checked on the device. */
#define LG_ROLLOUT_MAX_GATHER 16
#define LG_GATHER_F32 0
#define LG_GATHER_NOT_U8 1

typedef struct LgGatherItem {
    const void *src;
    float *dst;
    const int64_t *index;
    int32_t rows;         /* entries of index = rows of dst; 0 skips the item, whose pointers are then not looked at */
    int32_t width;
    int32_t src_stride;
    int32_t kind;
    int32_t group;
    int32_t env_offset;
    int32_t n_envs;
} LgGatherItem;

/* Every tensor of one mini-batch in ONE launch: up to LG_ROLLOUT_MAX_GATHER items, each with its own index pointer and row count.
 * Consecutive lanes on consecutive floats of a row; float4 moves where kind, width, stride and both pointers allow, scalar otherwise.
 * Every destination element is written exactly once.  Refused before the launch: a null pointer, width < 1, src_stride < width,
 * group < 1, env_offset < 0, env_offset + group > n_envs, rows < 0, an unknown kind, n_items outside [1, LG_ROLLOUT_MAX_GATHER], a
 * destination of 2^31 elements or more. */
int lg_rollout_gather(const LgGatherItem *items, int32_t n_items, void *stream);

/* lg_rollout_gae for two groups of envs (rollout_storage_cts.py:81-114): one pass of the recurrence over all N envs into returns
 * (T, N, 1); the raw advantages returns - values of envs [0, n_first) go to adv_first (T, n_first, 1) and those of [n_first, N) to
 * adv_rest (T, N - n_first, 1), both contiguous, and each group is normalised by its own mean and unbiased std.
 * scratch: device buffer of at least 4 doubles (sum, sum of squares per group).  Refused: n_first < 1, n_first >= N, a group with
 * fewer than two entries. */
int lg_rollout_gae_groups(int32_t n_steps, int32_t n_envs, int32_t n_first, const float *values, const float *rewards, const uint8_t *dones,
                          const float *last_values, float gamma, float lam, float *returns, float *adv_first, float *adv_rest,
                          double *scratch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LGROLLOUT_H */

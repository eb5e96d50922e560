/* lgoptim.h -- C ABI of the fused optimizer step: what every learner of the reference runs behind loss.backward()
 * (rsl_rl/algorithms/ppo.py:135-138: nn.utils.clip_grad_norm_(params, max_grad_norm); optimizer.step() with torch.optim.Adam's defaults)
 * together with the adaptive learning-rate rule in front of it (ppo.py:193-206), as two launches that read nothing back: the global
 * gradient norm, the clip coefficient, the learning rate and the step count, and the Adam update of every parameter tensor.  Same
 * conventions as lgppo.h: plain device pointers, the caller's HIP stream as void*; 0 on success, otherwise non-zero with the message in
 * lgsim.h's last-error call.  Tensors are float32; the norm's partial sums, the learning rate and the step count are float64.
 *
 * The learning rate and the step count live in a two-double cell on the device (`state`), so a captured graph that holds the call keeps
 * counting and keeps adapting its rate when it is replayed.
 *
 * Per call, with lr and step read from the cell:
 *   step += 1
 *   under LG_ADAM_KL_RULE, on k = (double)*kl:   k > 2 desired_kl               -> lr = max(1e-5, lr / 1.5)
 *                                                k < desired_kl / 2 and k > 0   -> lr = min(1e-2, lr * 1.5)
 *                                                otherwise (a NaN k included: every compare fails) lr stays
 *   total = (float)sqrt(sum over all tensors of g^2)                   the sum in float64
 *   coef  = min(max_grad_norm / (total + 1e-6f), 1.0f)   in float32    under LG_ADAM_CLIP, else 1
 *   bc1 = 1 - pow(beta1, step), bc2 = 1 - pow(beta2, step), step_size = lr / bc1, bc2_sqrt = sqrt(bc2)                 in float64
 * and per element in float32, in the operation order of torch's single-tensor Adam, the scalars rounded to float the way torch rounds
 * a Python scalar into a float32 op:
 *   g' = g * coef
 *   m  = m + (g' - m) * (float)(1 - beta1)
 *   v  = v * (float)beta2 + (float)(1 - beta2) * g' * g'
 *   p  = p + (float)(-step_size) * (m / (sqrtf(v) / (float)bc2_sqrt + (float)eps))
 * (torch's lerp_ takes this form for a weight 1 - beta1 below 0.5, i.e. beta1 above 0.5; it is the form used here for every beta1.)
 *
 * Gradients are read and never written: the clipped gradient g' exists in registers only.  This is the one visible departure from
 * clip_grad_norm_, which scales .grad in place.
 * NaN is not silent: a NaN in any gradient makes the total norm NaN, the clip coefficient NaN (min is a compare that passes it on) and
 * with it every parameter and both moments of every tensor of the call, as torch does.  An infinite gradient gives total = inf and
 * coef = 0: inf * 0 = NaN in that element, g' = 0 elsewhere.  Without LG_ADAM_CLIP a NaN stays in its own element.
 * Out of scope: weight decay, AMSGrad, maximize.
 */
#ifndef LGOPTIM_H
#define LGOPTIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LG_ADAM_MAX_TENSORS 64     /* the descriptor travels to the kernels by value: 64 x 40 B and the scalars stay under HIP's 4 KB
                                      kernel-argument block, where a table in device memory would need an upload whenever a .grad moves */
#define LG_ADAM_CLIP 1u            /* clip the gradients to max_grad_norm */
#define LG_ADAM_KL_RULE 2u         /* apply the adaptive learning-rate rule from *kl */

/* The launch plan, a pure function of the numels.  Tensor i is cut into chunks of LG_ADAM_CHUNK floats (LG_ADAM_THREADS lanes x one
 * 16-byte access), the last one possibly ragged; the chunks of tensor 0, tensor 1, ... are numbered one behind the other; the grid is
 * min(chunks, LG_ADAM_MAX_BLOCKS) workgroups of LG_ADAM_THREADS lanes and workgroup b sweeps chunks b, b + grid, ...  A whole chunk of a
 * tensor whose four base addresses are 16-byte aligned moves in 16-byte accesses, every other chunk in 4-byte ones. */
#define LG_ADAM_CHUNK 1024
#define LG_ADAM_THREADS 256
#define LG_ADAM_MAX_BLOCKS 512

#define LG_ADAM_STATE_DOUBLES 2    /* slots of `state` */
#define LG_ADAM_S_LR 0
#define LG_ADAM_S_STEP 1

#define LG_ADAM_RESULT_FLOATS 4    /* slots of `result` */
#define LG_ADAM_R_GRAD_NORM 0      /* total gradient norm before clipping */
#define LG_ADAM_R_CLIP_COEF 1      /* clip coefficient applied (1 without LG_ADAM_CLIP) */
#define LG_ADAM_R_LR 2             /* learning rate used, rounded to float */
#define LG_ADAM_R_STEP 3           /* step count after the call */

/* One parameter tensor: four contiguous float32 arrays of numel elements.  A base pointer may sit on any 4-byte boundary (a parameter
 * may be a view into a larger storage). */
typedef struct LgAdamTensor {
    float *param, *exp_avg, *exp_avg_sq;   /* updated in place */
    const float *grad;                     /* read, never written */
    int64_t numel;                         /* >= 1 */
} LgAdamTensor;

typedef struct LgAdamArgs {
    int32_t n_tensors;             /* 1 .. LG_ADAM_MAX_TENSORS; tensor[n_tensors ..] is not read */
    uint32_t flags;
    LgAdamTensor tensor[LG_ADAM_MAX_TENSORS];
    double beta1, beta2;           /* in [0, 1) */
    double eps;                    /* >= 0 */
    double max_grad_norm;          /* > 0 under LG_ADAM_CLIP, not read otherwise */
    double desired_kl;             /* > 0 under LG_ADAM_KL_RULE, not read otherwise */
    const float *kl;               /* device scalar, e.g. element LG_PPO_R_KL of the loss head's result vector; non-null if and only if
                                      LG_ADAM_KL_RULE is set */
    double *state;                 /* LG_ADAM_STATE_DOUBLES doubles on the device: learning rate, step count; read and advanced */
    double *partials;              /* workspace: lg_adam_workspace doubles, overwritten by every call, never read before it is written */
    int64_t partials_capacity;     /* doubles available at `partials` */
    float *result;                 /* LG_ADAM_RESULT_FLOATS floats out, the slots above */
} LgAdamArgs;

#ifdef __cplusplus
static_assert(sizeof(LgAdamArgs) <= 3072, "LgAdamArgs and the plan's prefix table must fit the 4 KB kernel-argument block");
#else
_Static_assert(sizeof(LgAdamArgs) <= 3072, "LgAdamArgs and the plan's prefix table must fit the 4 KB kernel-argument block");
#endif

/* Two launches on `stream`.  The first forms the sum of g^2 (every lane a float64 accumulator over its elements in chunk order, folded
 * per workgroup in a fixed order into slot b of the slab) and, in one lane of workgroup 0 alone, advances the state cell.  The second
 * sums the slab in every workgroup in one fixed order, so that every workgroup holds the same bits, and updates the tensors; workgroup 0
 * writes `result`.  Allocates nothing, never synchronises, uses no atomics: two calls on the same inputs give bit-identical results.
 * Refused before anything is enqueued, with a message that names the field: a null descriptor, n_tensors outside
 * [1, LG_ADAM_MAX_TENSORS], a numel below 1, a null param, grad, exp_avg or exp_avg_sq, unknown flag bits, kl null with LG_ADAM_KL_RULE or
 * set without it, LG_ADAM_KL_RULE with desired_kl not above 0, LG_ADAM_CLIP with max_grad_norm not above 0, beta1 or beta2 outside [0, 1),
 * eps below 0, null state, partials or result, partials_capacity below lg_adam_workspace. */
int lg_adam_step(const LgAdamArgs *args, void *stream);

/* Doubles the partials slab needs for this descriptor: the grid size of the plan.  Launches nothing and does not touch the device; reads
 * n_tensors and the numels only.  0 with the last error set on a refusal. */
int lg_adam_workspace(const LgAdamArgs *args);

#ifdef __cplusplus
}
#endif
#endif /* LGOPTIM_H */

"""Golden vectors for the fused learner passes of the concurrent teacher-student family (include/lgtraincts.h, and include/lgtraints.h's
encoder pass with a mask of ones) and for the whole fused PPO_CTS update (RL pass, two-group loss head, optimizer; encoder pass, optimizer)
from the reference's own PPO_CTS.update() (rsl_rl/algorithms/ppo_cts.py:137-191) on a tiny ActorCriticCTS: the net of
gen_ppo_ts_train_fixtures.py (O = 7 observations, P = 5 privileged observations, Z = 3 latent dims, H = 14 history, 9 critic observations,
A = 3; actor 10 -> 16 -> 8 -> 3, critic 9 -> 16 -> 8 -> 1, privilege encoder 5 -> 8 -> 4 -> 3, history encoder 14 -> 8 -> 4 -> 3), everything
float64 on the CPU, schedule="adaptive", 2 epochs x 3 mini-batches, num_encoder_epochs = 2, over a storage of 8 envs (num_teacher = 5) x 6
steps filled through PPO_CTS.act / process_env_step from a seeded generator with dones of probability 0.25: 10 teacher, 6 student and 16
critic rows per mini-batch, 6 RL steps and 12 encoder steps.

Build-container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_ppo_cts_train_fixtures.py
Output: tests/golden/ppo_cts_train.npz:
  names, shapes          the parameter names in the order of actor_critic.parameters(), and their shapes
  rl_names, enc_names    the names in the order of PPO_CTS.rl_params (actor, critic, privilege encoder, std) and of
                         history_encoder.parameters()
  cfg                    [lr0, beta1, beta2, eps, max_grad_norm, desired_kl, rl_steps, clip_param, value_loss_coef, entropy_coef, encoder_lr,
                          enc_steps, num_encoder_epochs]
  init                   every parameter before the first step, flattened one behind the other in `names` order, float64
  per RL step:           the mini-batch columns of COLUMNS as PPO_CTS._compute_rl_loss received them; mu_t, sigma_t, mu_s, sigma_s, values;
                         loss, teacher_surrogate, student_surrogate; kl (of the teacher rows, the reference's formula) and lr (read at the
                         clip: PPO_CTS sets the rate inside _compute_rl_loss); grad_norm; grads (the gradients of rl_params before the clip,
                         flattened in rl_names order); params (EVERY parameter after the step)
  per encoder step:      enc_history, enc_privileged as _compute_encoder_loss received them; enc_loss; enc_grads (before the clip, enc_names
                         order); enc_grad_norm; enc_params (every parameter after the step)
Asserted here, so that rounding to float32 moves no decision: no KL within 1 % of a threshold of the rate rule; no gradient norm (either
loop) within 1 % of max_grad_norm.  Also asserted, because the fused pass relies on it: at every RL clip torch HAS accumulated a non-zero
gradient in the history encoder, which history_encoder_optimizer.zero_grad() discards before those parameters ever step.  ActorCriticCTS has
no Hardtanh, so there is no clip margin to keep.  Written through ref_harness.save; `python tests/golden/check_fixtures.py` checks that the
output still equals the committed file."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

rh.load_reference()
import torch  # noqa: E402

LR0, ENC_LR, MAX_GRAD_NORM, DESIRED_KL = 1e-3, 1e-3, 1.75, 1.5e-4
CLIP_PARAM, VALUE_LOSS_COEF, ENTROPY_COEF = 0.2, 1.0, 0.01
O, P, Z, H, N_COBS, A, N_ENVS, N_TEACHER, T, EPOCHS, MINI_BATCHES, ENC_EPOCHS, P_DONE = 7, 5, 3, 14, 9, 3, 8, 5, 6, 2, 3, 2, 0.25
COLUMNS = ("teacher_obs", "teacher_privileged_obs", "teacher_actions", "teacher_old_log_prob", "teacher_advantages", "teacher_old_mu",
           "teacher_old_sigma", "student_obs", "student_obs_history", "student_actions", "student_old_log_prob", "student_advantages", "critic_obs",
           "target_values", "returns")
SEED = 50


def main(seed=SEED, write=True):
    import contextlib
    import io
    from rsl_rl.algorithms import ppo_cts as ppo_module
    from rsl_rl.algorithms.ppo_cts import PPO_CTS
    from rsl_rl.modules import ActorCriticCTS
    torch.set_num_threads(1)
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):            # the module prints its four MLPs
        ac = ActorCriticCTS(O, A, P, H, Z, N_COBS, actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8], privilege_encoder_hidden_dims=[8, 4],
                            history_encoder_hidden_dims=[8, 4]).double()
    alg = PPO_CTS(ac, num_learning_epochs=EPOCHS, num_mini_batches=MINI_BATCHES, learning_rate=LR0, max_grad_norm=MAX_GRAD_NORM,
                  schedule="adaptive", desired_kl=DESIRED_KL, entropy_coef=ENTROPY_COEF, clip_param=CLIP_PARAM, value_loss_coef=VALUE_LOSS_COEF,
                  use_clipped_value_loss=True, device="cpu", encoder_lr=ENC_LR, num_encoder_epochs=ENC_EPOCHS, num_teacher=N_TEACHER)
    alg.init_storage(N_ENVS, T, [O], [P], [H], [N_COBS], [A])
    for t in range(T):
        alg.act(torch.randn(N_ENVS, O, generator=g), torch.randn(N_ENVS, P, generator=g), torch.randn(N_ENVS, H, generator=g),
                torch.randn(N_ENVS, N_COBS, generator=g))
        alg.process_env_step(torch.randn(N_ENVS, generator=g), (torch.rand(N_ENVS, generator=g) < P_DONE), {})
    alg.compute_returns(torch.randn(N_ENVS, N_COBS, generator=g))

    names = [n for n, _ in ac.named_parameters()]
    by_id = {id(p): n for n, p in ac.named_parameters()}
    rl_names = [by_id[id(p)] for p in alg.rl_params]
    enc_params = list(ac.history_encoder.parameters())
    enc_names = [by_id[id(p)] for p in enc_params]
    n64 = lambda x: x.detach().numpy().astype(np.float64).copy()
    flat = lambda xs: np.concatenate([n64(x).reshape(-1) for x in xs])
    steps, enc_steps = EPOCHS * MINI_BATCHES, EPOCHS * MINI_BATCHES * ENC_EPOCHS
    arrays = {"names": np.array(names), "shapes": np.array([(list(p.shape) + [0, 0])[:2] for p in ac.parameters()], np.int64),
              "rl_names": np.array(rl_names), "enc_names": np.array(enc_names)}
    arrays["cfg"] = np.array([LR0, 0.9, 0.999, 1e-8, MAX_GRAD_NORM, DESIRED_KL, steps, CLIP_PARAM, VALUE_LOSS_COEF, ENTROPY_COEF, ENC_LR, enc_steps,
                              ENC_EPOCHS], np.float64)
    arrays["init"] = flat(ac.parameters())
    rl_keys = COLUMNS + ("mu_t", "sigma_t", "mu_s", "sigma_s", "values", "loss", "teacher_surrogate", "student_surrogate", "kl", "lr", "grad_norm",
                         "grads", "params")
    enc_keys = ("enc_history", "enc_privileged", "enc_loss", "enc_grads", "enc_grad_norm", "enc_params")
    rec = {k: [] for k in rl_keys + enc_keys}

    clip0, loss0, enc_loss0, update0 = ppo_module.nn.utils.clip_grad_norm_, alg._compute_rl_loss, alg._compute_encoder_loss, ac.update_distribution
    seen = {}

    def update_distribution(observations, observation_history, privilege_observations, act_type):
        update0(observations, observation_history, privilege_observations, act_type)
        seen[act_type] = (n64(ac.action_mean), n64(ac.action_std))

    def compute_rl_loss(t_obs, t_pobs, t_actions, t_old_log_prob, t_adv, t_old_mu, t_old_sigma, s_obs, s_hist, s_actions, s_old_log_prob, s_adv, cobs,
                        target_values, returns, hid, masks):
        for k, v in zip(COLUMNS, (t_obs, t_pobs, t_actions, t_old_log_prob, t_adv, t_old_mu, t_old_sigma, s_obs, s_hist, s_actions, s_old_log_prob, s_adv,
                                  cobs, target_values, returns)):
            rec[k].append(n64(v))
        seen.clear()
        out = loss0(t_obs, t_pobs, t_actions, t_old_log_prob, t_adv, t_old_mu, t_old_sigma, s_obs, s_hist, s_actions, s_old_log_prob, s_adv, cobs,
                    target_values, returns, hid, masks)
        (mu_t, sigma_t), (mu_s, sigma_s) = seen["teacher"], seen["student"]
        for k, v in (("mu_t", mu_t), ("sigma_t", sigma_t), ("mu_s", mu_s), ("sigma_s", sigma_s)):
            rec[k].append(v)
        with torch.no_grad():
            rec["values"].append(n64(ac.evaluate(cobs)))
        old_mu, old_sigma = n64(t_old_mu), n64(t_old_sigma)
        rec["kl"].append(float(np.sum(np.log(sigma_t / old_sigma + 1.e-5) + (old_sigma ** 2 + (old_mu - mu_t) ** 2) / (2.0 * sigma_t ** 2) - 0.5,
                                      axis=-1).mean()))
        rec["loss"].append(float(out[0].detach()))
        rec["teacher_surrogate"].append(float(out[1]))
        rec["student_surrogate"].append(float(out[2]))
        return out

    def compute_encoder_loss(history, pobs):
        rec["enc_history"].append(n64(history))
        rec["enc_privileged"].append(n64(pobs))
        out = enc_loss0(history, pobs)
        rec["enc_loss"].append(float(out))
        return out

    def clip(parameters, max_norm, *a, **k):
        parameters = list(parameters)
        assert max_norm == MAX_GRAD_NORM
        if [id(p) for p in parameters] == [id(p) for p in alg.rl_params]:
            # torch does send the RL loss into the history encoder; nothing ever reads it (the module docstring)
            assert all(p.grad is not None for p in enc_params) and any(float(p.grad.abs().max()) > 0 for p in enc_params)
            rec["grads"].append(flat(p.grad for p in parameters))
            rec["lr"].append(float(alg.optimizer.param_groups[0]["lr"]))
            total = clip0(parameters, max_norm, *a, **k)
            rec["grad_norm"].append(float(total))
        else:
            assert [id(p) for p in parameters] == [id(p) for p in enc_params]
            rec["enc_grads"].append(flat(p.grad for p in parameters))
            total = clip0(parameters, max_norm, *a, **k)
            rec["enc_grad_norm"].append(float(total))
        return total

    alg._compute_rl_loss, alg._compute_encoder_loss, ac.update_distribution = compute_rl_loss, compute_encoder_loss, update_distribution
    ppo_module.nn.utils.clip_grad_norm_ = clip
    try:
        for opt, key in ((alg.optimizer, "params"), (alg.history_encoder_optimizer, "enc_params")):
            def step(*a, _step0=opt.step, _key=key, **k):
                out = _step0(*a, **k)
                rec[_key].append(flat(ac.parameters()))
                return out
            opt.step = step
        alg.update()
    finally:
        ppo_module.nn.utils.clip_grad_norm_ = clip0
    assert all(len(rec[k]) == steps for k in rl_keys) and all(len(rec[k]) == enc_steps for k in enc_keys), {k: len(v) for k, v in rec.items()}
    assert rec["teacher_obs"][0].shape == (10, O) and rec["student_obs"][0].shape == (6, O) and rec["critic_obs"][0].shape == (16, N_COBS)
    # no KL within 1 % of a threshold of the rate rule, no norm within 1 % of the clip: rounding to float32 moves no decision
    assert all(abs(k / (2 * DESIRED_KL) - 1.0) > 0.01 and abs(k / (DESIRED_KL / 2) - 1.0) > 0.01 and k > 0 for k in rec["kl"]), rec["kl"]
    assert all(abs(n / MAX_GRAD_NORM - 1.0) > 0.01 for n in rec["grad_norm"] + rec["enc_grad_norm"]), (rec["grad_norm"], rec["enc_grad_norm"])
    for k, v in rec.items():
        arrays[k] = np.stack([np.asarray(x, np.float64) for x in v])
    if not write:
        return arrays
    rh.save("ppo_cts_train", arrays, "kl", [f"{k:.3e}" for k in rec["kl"]], "lr", [f"{x:.3e}" for x in rec["lr"]],
            "norm", [f"{n:.3f}" for n in rec["grad_norm"]], "enc_norm", [f"{n:.3f}" for n in rec["enc_grad_norm"]])


if __name__ == "__main__":
    main()

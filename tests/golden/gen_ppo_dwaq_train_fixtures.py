"""Golden vectors for the fused learner passes of the DreamWaQ family (include/lgtraindwaq.h) and for the whole fused PPO_DreamWaQ update
(RL pass, loss head, optimizer; VAE pass, optimizer) from the reference's own PPO_DreamWaQ.update()
(rsl_rl/algorithms/ppo_dreamwaq.py:140-236) on a tiny ActorCriticDreamWaQ (O = 7 observations, 9 privileged (critic) observations, H = 14
history, L = 3 latent dims, E = 2 explicit dims, D = 5 decoder outputs, A = 3; actor 12 -> 8 -> 4 -> 3, critic 9 -> 8 -> 4 -> 1, encoder
14 -> 8 -> 6 -> 10 with an ELU behind every Linear, heads 10 -> 3 / 3 / 2 / 2, decoder 5 -> 8 -> 4 -> 5), everything float64 on the CPU,
schedule="adaptive", 2 epochs x 3 mini-batches, num_encoder_epochs = 2, vae_kld_weight = 0.5, over a storage of 8 envs x 6 steps filled
through PPO_DreamWaQ.act / process_env_step from a seeded generator with dones of probability 0.25.  The two log-variance heads' initial
weights are scaled by VAR_SCALE so that the +-5 Hardtanh clips some log-variances and passes others in every step.

The reparameterisation noise is the reference's own: vae.reparameterize runs as it stands, and torch.randn_like is wrapped for the
duration of the update so that every eps it draws (z, then vel, per VAE forward) is recorded.

Build-container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_ppo_dwaq_train_fixtures.py
Output: tests/golden/ppo_dwaq_train.npz:
  names, shapes          the parameter names in the order of actor_critic.parameters(), and their shapes
  rl_names, vae_names    the names in the order of PPO_DreamWaQ.rl_parameters (actor, critic, std) and of vae.parameters()
  cfg                    [lr0, beta1, beta2, eps, max_grad_norm, desired_kl, rl_steps, clip_param, value_loss_coef, entropy_coef, encoder_lr,
                          vae_steps, num_encoder_epochs, vae_kld_weight, var_clip]
  init                   every parameter before the first step, flattened one behind the other in `names` order, float64
  per RL step:           the mini-batch columns obs, critic_obs, obs_history, actions, target_values, advantages, returns, old_log_prob,
                         old_mu, old_sigma as PPO_DreamWaQ._compute_rl_loss received them; noise ((B, L + E), columns [z | vel]); mu, sigma,
                         values; loss; kl and lr; grad_norm; grads (the gradients of rl_parameters before the clip, flattened in rl_names
                         order); params (EVERY parameter after the step)
  per VAE step:          vae_history, vae_labels, vae_next_states, vae_terminated as _compute_vae_loss received them; vae_noise; vae_losses
                         (total, estimation, reconstruction, kld); vae_grads (before the clip, vae_names order); vae_grad_norm; vae_params
                         (every parameter after the step)
The steps interleave as the update runs them: RL step s, then VAE steps 2 s and 2 s + 1, so RL step s + 1 sees the VAE those two left.
Asserted here, so that rounding to float32 moves no decision: no KL within 1 % of a threshold of the rate rule; no gradient norm (either
loop) within 1 % of max_grad_norm; every VAE batch has a masked and an unmasked row; every step has a clipped and an unclipped
log-variance and none within 1e-3 of the clip.  Written through ref_harness.save; `python tests/golden/check_fixtures.py` checks that the
output still equals the committed file."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

rh.load_reference()
import torch  # noqa: E402

LR0, ENC_LR, MAX_GRAD_NORM, DESIRED_KL, KLD_WEIGHT = 1e-3, 1e-3, 2.0, 1.5e-4, 0.5
CLIP_PARAM, VALUE_LOSS_COEF, ENTROPY_COEF = 0.2, 1.0, 0.01
O, N_COBS, H, L, E, D, A, N_ENVS, T, EPOCHS, MINI_BATCHES, VAE_EPOCHS, P_DONE = 7, 9, 14, 3, 2, 5, 3, 8, 6, 2, 3, 2, 0.25
VAR_CLIP, VAR_SCALE = 5.0, 30.0
COLUMNS = ("obs", "critic_obs", "obs_history", "actions", "target_values", "advantages", "returns", "old_log_prob", "old_mu", "old_sigma")
SEED = 57


def main(seed=SEED, write=True):
    from rsl_rl.algorithms import ppo_dreamwaq as ppo_module
    from rsl_rl.algorithms.ppo_dreamwaq import PPO_DreamWaQ
    from rsl_rl.modules import ActorCriticDreamWaQ
    torch.set_num_threads(1)
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    ac = ActorCriticDreamWaQ(O, A, N_COBS, H, L, E, D, actor_hidden_dims=[8, 4], critic_hidden_dims=[8, 4], encoder_hidden_dims=[8, 6],
                             decoder_hidden_dims=[8, 4]).double()
    with torch.no_grad():
        for head in (ac.vae.latent_var[0], ac.vae.vel_var[0]):
            head.weight.mul_(VAR_SCALE)
    assert ac.vae.latent_var[1].max_val == VAR_CLIP == -ac.vae.latent_var[1].min_val == ac.vae.vel_var[1].max_val
    alg = PPO_DreamWaQ(ac, num_learning_epochs=EPOCHS, num_mini_batches=MINI_BATCHES, learning_rate=LR0, max_grad_norm=MAX_GRAD_NORM,
                       schedule="adaptive", desired_kl=DESIRED_KL, entropy_coef=ENTROPY_COEF, clip_param=CLIP_PARAM, value_loss_coef=VALUE_LOSS_COEF,
                       use_clipped_value_loss=True, device="cpu", encoder_lr=ENC_LR, num_encoder_epochs=VAE_EPOCHS, vae_kld_weight=KLD_WEIGHT)
    alg.init_storage(N_ENVS, T, [O], [N_COBS], [H], [E], [D], [A])
    for t in range(T):
        alg.act(torch.randn(N_ENVS, O, generator=g), torch.randn(N_ENVS, N_COBS, generator=g), torch.randn(N_ENVS, H, generator=g),
                torch.randn(N_ENVS, E, generator=g))
        alg.process_env_step(torch.randn(N_ENVS, generator=g), (torch.rand(N_ENVS, generator=g) < P_DONE), {}, torch.randn(N_ENVS, D, generator=g))
    alg.compute_returns(torch.randn(N_ENVS, N_COBS, generator=g))

    names = [n for n, _ in ac.named_parameters()]
    by_id = {id(p): n for n, p in ac.named_parameters()}
    rl_names = [by_id[id(p)] for p in alg.rl_parameters]
    vae_params = list(ac.vae.parameters())
    vae_names = [by_id[id(p)] for p in vae_params]
    n64 = lambda x: x.detach().numpy().astype(np.float64).copy()
    flat = lambda xs: np.concatenate([n64(x).reshape(-1) for x in xs])
    steps, vae_steps = EPOCHS * MINI_BATCHES, EPOCHS * MINI_BATCHES * VAE_EPOCHS
    arrays = {"names": np.array(names), "shapes": np.array([(list(p.shape) + [0, 0])[:2] for p in ac.parameters()], np.int64),
              "rl_names": np.array(rl_names), "vae_names": np.array(vae_names)}
    arrays["cfg"] = np.array([LR0, 0.9, 0.999, 1e-8, MAX_GRAD_NORM, DESIRED_KL, steps, CLIP_PARAM, VALUE_LOSS_COEF, ENTROPY_COEF, ENC_LR, vae_steps,
                              VAE_EPOCHS, KLD_WEIGHT, VAR_CLIP], np.float64)
    arrays["init"] = flat(ac.parameters())
    rl_keys = COLUMNS + ("noise", "mu", "sigma", "values", "loss", "kl", "lr", "grad_norm", "grads", "params")
    vae_keys = ("vae_history", "vae_labels", "vae_next_states", "vae_terminated", "vae_noise", "vae_losses", "vae_grads", "vae_grad_norm", "vae_params")
    rec = {k: [] for k in rl_keys + vae_keys}
    draws, logvars, margins = [], [], []

    clip0, adjust0, loss0, vae_loss0, randn_like0 = ppo_module.nn.utils.clip_grad_norm_, alg._adjust_learning_rate, alg._compute_rl_loss, \
        alg._compute_vae_loss, torch.randn_like

    def randn_like(x, *a, **k):
        eps = randn_like0(x, *a, **k)
        draws.append(n64(eps))
        return eps

    def take_noise():
        assert len(draws) == 2 and draws[0].shape[1] == L and draws[1].shape[1] == E, [d.shape for d in draws]       # z, then vel
        eps = np.concatenate(draws, axis=1)
        del draws[:]
        pre = np.concatenate(logvars, axis=1)
        del logvars[:]
        margins.append((int((np.abs(pre) >= VAR_CLIP).sum()), int((np.abs(pre) < VAR_CLIP).sum()), float(np.abs(np.abs(pre) - VAR_CLIP).min())))
        return eps

    hooks = [m.register_forward_hook(lambda _m, _i, out: logvars.append(n64(out))) for m in (ac.vae.latent_var[0], ac.vae.vel_var[0])]

    def compute_rl_loss(obs, cobs, history, actions, target_values, advantages, returns, old_log_prob, old_mu, old_sigma, hid, masks):
        for k, v in zip(COLUMNS, (obs, cobs, history, actions, target_values, advantages, returns, old_log_prob, old_mu, old_sigma)):
            rec[k].append(n64(v))
        out = loss0(obs, cobs, history, actions, target_values, advantages, returns, old_log_prob, old_mu, old_sigma, hid, masks)
        rec["noise"].append(take_noise())
        rec["mu"].append(n64(ac.action_mean))
        rec["sigma"].append(n64(ac.action_std))
        with torch.no_grad():
            rec["values"].append(n64(ac.evaluate(cobs)))
        rec["loss"].append(float(out[0]))
        return out

    def compute_vae_loss(history, terminated, labels, next_states):
        for k, v in zip(("vae_history", "vae_terminated", "vae_labels", "vae_next_states"), (history, terminated, labels, next_states)):
            rec[k].append(n64(v))
        out = vae_loss0(history, terminated, labels, next_states)
        rec["vae_noise"].append(take_noise())
        rec["vae_losses"].append(np.array([float(v) for v in out]))
        return out

    def adjust(sigma, old_sigma, mu, old_mu):
        with torch.no_grad():
            rec["kl"].append(float(torch.sum(torch.log(sigma / old_sigma + 1.e-5) + (old_sigma ** 2 + (old_mu - mu) ** 2) / (2.0 * sigma ** 2) - 0.5,
                                             dim=-1).mean()))
        return adjust0(sigma, old_sigma, mu, old_mu)

    def clip(parameters, max_norm, *a, **k):
        parameters = list(parameters)
        assert max_norm == MAX_GRAD_NORM
        if [id(p) for p in parameters] == [id(p) for p in alg.rl_parameters]:
            rec["grads"].append(flat(p.grad for p in parameters))
            rec["lr"].append(float(alg.optimizer.param_groups[0]["lr"]))
            total = clip0(parameters, max_norm, *a, **k)
            rec["grad_norm"].append(float(total))
        else:
            assert [id(p) for p in parameters] == [id(p) for p in vae_params]
            rec["vae_grads"].append(flat(p.grad for p in parameters))
            total = clip0(parameters, max_norm, *a, **k)
            rec["vae_grad_norm"].append(float(total))
        return total

    alg._adjust_learning_rate, alg._compute_rl_loss, alg._compute_vae_loss = adjust, compute_rl_loss, compute_vae_loss
    ppo_module.nn.utils.clip_grad_norm_ = clip
    torch.randn_like = randn_like
    try:
        for opt, key in ((alg.optimizer, "params"), (alg.vae_optimizer, "vae_params")):
            def step(*a, _step0=opt.step, _key=key, **k):
                out = _step0(*a, **k)
                rec[_key].append(flat(ac.parameters()))
                return out
            opt.step = step
        alg.update()
    finally:
        ppo_module.nn.utils.clip_grad_norm_ = clip0
        torch.randn_like = randn_like0
        for h in hooks:
            h.remove()
    assert all(len(rec[k]) == steps for k in rl_keys) and all(len(rec[k]) == vae_steps for k in vae_keys), {k: len(v) for k, v in rec.items()}
    assert not draws and not logvars and len(margins) == steps + vae_steps
    # no KL within 1 % of a threshold of the rate rule, no norm within 1 % of the clip: rounding to float32 moves no decision
    assert all(abs(k / (2 * DESIRED_KL) - 1.0) > 0.01 and abs(k / (DESIRED_KL / 2) - 1.0) > 0.01 and k > 0 for k in rec["kl"]), rec["kl"]
    assert all(abs(n / MAX_GRAD_NORM - 1.0) > 0.01 for n in rec["grad_norm"] + rec["vae_grad_norm"]), (rec["grad_norm"], rec["vae_grad_norm"])
    assert all(0 < t.sum() < t.size and set(np.unique(t)) <= {0.0, 1.0} for t in rec["vae_terminated"]), [t.sum() for t in rec["vae_terminated"]]
    assert all(c > 0 and u > 0 and m > 1e-3 for c, u, m in margins), margins
    for k, v in rec.items():
        arrays[k] = np.stack([np.asarray(x, np.float64) for x in v])
    if not write:
        return arrays
    rh.save("ppo_dwaq_train", arrays, "kl", [f"{k:.3e}" for k in rec["kl"]], "lr", [f"{x:.3e}" for x in rec["lr"]],
            "norm", [f"{n:.3f}" for n in rec["grad_norm"]], "vae_norm", [f"{n:.3f}" for n in rec["vae_grad_norm"]],
            "masked", [int(t.size - t.sum()) for t in rec["vae_terminated"]], "clipped", [c for c, _, _ in margins])


if __name__ == "__main__":
    main()

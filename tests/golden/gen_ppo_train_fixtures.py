"""Golden vectors for the fused learner pass (include/lgtrain.h) and for the whole fused update step (train pass, loss head, optimizer)
from the reference's own PPO.update() (rsl_rl/algorithms/ppo.py:124-148) on the tiny ActorCritic of gen_ppo_update_fixtures.py (actor and
critic 7 -> 16 -> 8 -> A, the same sizes), everything float64 on the CPU, schedule="adaptive", 2 epochs x 3 mini-batches over a storage
filled through PPO.act / process_env_step from a seeded generator.

Build-container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_ppo_train_fixtures.py
Output: tests/golden/ppo_train.npz:
  names, shapes          the parameter names in the order of actor_critic.parameters(), and their shapes (rows, columns; 0: no such axis)
  cfg                    [lr0, beta1, beta2, eps, max_grad_norm, desired_kl, steps, clip_param, value_loss_coef, entropy_coef, clip_actions]
  init                   every parameter before the first step, flattened one behind the other in that order, float64
  per step (steps, ...): the mini-batch columns obs, critic_obs, actions, target_values, advantages, returns, old_log_prob, old_mu,
                         old_sigma as PPO._compute_rl_loss received them; mu, sigma, values as the module computed them; loss; kl and lr
                         (the KL the rule saw, the rate in force for the step); grad_norm; grads (every parameter gradient before the
                         clip, flattened likewise); params (every parameter after the step)
clip_actions is chosen so that, asserted here, between 10 % and 90 % of the means of every step saturate and no pre-clip mean lies within
1e-4 of +-clip_actions, so no rounding moves a mask decision.  Written through ref_harness.save; `python tests/golden/check_fixtures.py`
checks that the output still equals the committed file."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

rh.load_reference()
import torch  # noqa: E402

LR0, MAX_GRAD_NORM, DESIRED_KL, CLIP_ACTIONS = 1e-3, 1.75, 1.5e-4, 0.12
CLIP_PARAM, VALUE_LOSS_COEF, ENTROPY_COEF = 0.2, 1.0, 0.01
N_OBS, N_COBS, A, N_ENVS, T, EPOCHS, MINI_BATCHES = 7, 7, 3, 8, 6, 2, 3
COLUMNS = ("obs", "critic_obs", "actions", "target_values", "advantages", "returns", "old_log_prob", "old_mu", "old_sigma")


def main(seed=59):
    from rsl_rl.algorithms import PPO, ppo as ppo_module
    from rsl_rl.modules import ActorCritic
    torch.set_num_threads(1)
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    ac = ActorCritic(N_OBS, N_COBS, A, actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8], clip_actions=CLIP_ACTIONS).double()
    alg = PPO(ac, num_learning_epochs=EPOCHS, num_mini_batches=MINI_BATCHES, learning_rate=LR0, max_grad_norm=MAX_GRAD_NORM,
              schedule="adaptive", desired_kl=DESIRED_KL, entropy_coef=ENTROPY_COEF, clip_param=CLIP_PARAM, value_loss_coef=VALUE_LOSS_COEF,
              use_clipped_value_loss=True, device="cpu")
    alg.init_storage(N_ENVS, T, [N_OBS], [N_COBS], [A])
    for t in range(T):
        alg.act(torch.randn(N_ENVS, N_OBS, generator=g), torch.randn(N_ENVS, N_COBS, generator=g))
        alg.process_env_step(torch.randn(N_ENVS, generator=g), (torch.rand(N_ENVS, generator=g) < 0.1), {})
    alg.compute_returns(torch.randn(N_ENVS, N_COBS, generator=g))

    names = [n for n, _ in ac.named_parameters()]
    n64 = lambda x: x.detach().numpy().astype(np.float64).copy()
    flat = lambda xs: np.concatenate([n64(x).reshape(-1) for x in xs])
    steps = EPOCHS * MINI_BATCHES
    arrays = {"names": np.array(names), "shapes": np.array([(list(p.shape) + [0, 0])[:2] for p in ac.parameters()], np.int64)}
    arrays["cfg"] = np.array([LR0, 0.9, 0.999, 1e-8, MAX_GRAD_NORM, DESIRED_KL, steps, CLIP_PARAM, VALUE_LOSS_COEF, ENTROPY_COEF, CLIP_ACTIONS],
                             np.float64)
    arrays["init"] = flat(ac.parameters())
    rec = {k: [] for k in COLUMNS + ("mu", "sigma", "values", "loss", "kl", "lr", "grad_norm", "grads", "params")}
    saturated, margins = [], []

    clip0, adjust0, loss0 = ppo_module.nn.utils.clip_grad_norm_, alg._adjust_learning_rate, alg._compute_rl_loss

    def compute_rl_loss(obs, cobs, actions, target_values, advantages, returns, old_log_prob, old_mu, old_sigma, hid, masks):
        for k, v in zip(COLUMNS, (obs, cobs, actions, target_values, advantages, returns, old_log_prob, old_mu, old_sigma)):
            rec[k].append(n64(v))
        out = loss0(obs, cobs, actions, target_values, advantages, returns, old_log_prob, old_mu, old_sigma, hid, masks)
        rec["mu"].append(n64(ac.action_mean))
        rec["sigma"].append(n64(ac.action_std))
        with torch.no_grad():
            rec["values"].append(n64(ac.evaluate(cobs)))
            pre = ac.actor[:-1](obs)
        rec["loss"].append(float(out[0]))
        saturated.append(float((pre.abs() >= CLIP_ACTIONS).double().mean()))
        margins.append(float((pre.abs() - CLIP_ACTIONS).abs().min()))
        return out

    def adjust(sigma, old_sigma, mu, old_mu):
        with torch.no_grad():
            rec["kl"].append(float(torch.sum(torch.log(sigma / old_sigma + 1.e-5) + (old_sigma ** 2 + (old_mu - mu) ** 2) / (2.0 * sigma ** 2) - 0.5,
                                             dim=-1).mean()))
        return adjust0(sigma, old_sigma, mu, old_mu)

    def clip(parameters, max_norm, *a, **k):
        parameters = list(parameters)
        assert max_norm == MAX_GRAD_NORM and len(parameters) == len(names)
        rec["grads"].append(flat(p.grad for p in parameters))
        rec["lr"].append(float(alg.optimizer.param_groups[0]["lr"]))
        total = clip0(parameters, max_norm, *a, **k)
        rec["grad_norm"].append(float(total))
        return total

    alg._adjust_learning_rate, alg._compute_rl_loss = adjust, compute_rl_loss
    ppo_module.nn.utils.clip_grad_norm_ = clip
    try:
        step0 = alg.optimizer.step

        def step(*a, **k):
            out = step0(*a, **k)
            rec["params"].append(flat(ac.parameters()))
            return out
        alg.optimizer.step = step
        alg.update()
    finally:
        ppo_module.nn.utils.clip_grad_norm_ = clip0
    assert all(len(v) == steps for v in rec.values()), {k: len(v) for k, v in rec.items()}
    assert all(0.1 <= s <= 0.9 for s in saturated), saturated
    assert all(m >= 1e-4 for m in margins), margins
    # no KL within 1 % of a threshold of the rate rule, no norm within 1 % of the clip: rounding to float32 moves no decision
    assert all(abs(k / (2 * DESIRED_KL) - 1.0) > 0.01 and abs(k / (DESIRED_KL / 2) - 1.0) > 0.01 and k > 0 for k in rec["kl"]), rec["kl"]
    assert all(abs(n / MAX_GRAD_NORM - 1.0) > 0.01 for n in rec["grad_norm"]), rec["grad_norm"]
    for k, v in rec.items():
        arrays[k] = np.stack([np.asarray(x, np.float64) for x in v])
    rh.save("ppo_train", arrays, "saturated", [f"{s:.2f}" for s in saturated], "margin", f"{min(margins):.2e}", "kl", [f"{k:.3e}" for k in rec["kl"]],
            "lr", [f"{x:.3e}" for x in rec["lr"]], "norm", [f"{n:.3f}" for n in rec["grad_norm"]])


if __name__ == "__main__":
    main()

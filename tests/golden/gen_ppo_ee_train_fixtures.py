"""Golden vectors for the fused learner passes of the explicit-estimator family (include/lgtrainee.h) and for the whole fused PPO_EE update
(RL pass, loss head, optimizer; estimator pass, optimizer) from the reference's own PPO_EE.update() (rsl_rl/algorithms/ppo_ee.py:93-139)
on a tiny ActorCriticEE (F = 7 features, NL = 3 labels, 9 critic observations, A = 3; actor 10 -> 16 -> 8 -> 3, critic 9 -> 16 -> 8 -> 1,
estimator 7 -> 8 -> 4 -> 3), everything float64 on the CPU, schedule="adaptive", 2 epochs x 3 mini-batches, num_estimator_epochs = 2, over
a storage of 8 envs x 6 steps filled through PPO_EE.act / process_env_step from a seeded generator with dones of probability 0.25.

Build-container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_ppo_ee_train_fixtures.py
Output: tests/golden/ppo_ee_train.npz:
  names, shapes          the parameter names in the order of actor_critic.parameters() (std, actor, critic, estimator), and their shapes
  rl_names, est_names    the names in the order of PPO_EE.rl_parameters (actor, critic, std) and of estimator.parameters()
  cfg                    [lr0, beta1, beta2, eps, max_grad_norm, desired_kl, rl_steps, clip_param, value_loss_coef, entropy_coef, clip_actions,
                          estimator_lr, est_steps, num_estimator_epochs]
  init                   every parameter before the first step, flattened one behind the other in `names` order, float64
  per RL step:           the mini-batch columns critic_obs, features, actions, target_values, advantages, returns, old_log_prob, old_mu,
                         old_sigma as PPO_EE._compute_rl_loss received them; mu, sigma, values; loss; kl and lr; grad_norm; grads (the
                         gradients of rl_parameters before the clip, flattened in rl_names order); params (EVERY parameter after the step)
  per estimator step:    est_features, est_labels, est_terminated as _compute_estimator_loss received them; est_loss; est_grads (before the
                         clip, est_names order); est_grad_norm; est_params (every parameter after the step)
Asserted here, so that rounding to float32 moves no decision: between 10 % and 90 % of the pre-clip means of every RL step saturate and
none lies within 1e-4 of +-clip_actions; no KL within 1 % of a threshold of the rate rule; no gradient norm (either loop) within 1 % of
max_grad_norm; every estimator batch has a masked and an unmasked row.  Written through ref_harness.save; `python
tests/golden/check_fixtures.py` checks that the output still equals the committed file."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

rh.load_reference()
import torch  # noqa: E402

LR0, EST_LR, MAX_GRAD_NORM, DESIRED_KL, CLIP_ACTIONS = 1e-3, 1e-3, 1.75, 1.5e-4, 0.3
CLIP_PARAM, VALUE_LOSS_COEF, ENTROPY_COEF = 0.2, 1.0, 0.01
F, NL, N_COBS, A, N_ENVS, T, EPOCHS, MINI_BATCHES, EST_EPOCHS, P_DONE = 7, 3, 9, 3, 8, 6, 2, 3, 2, 0.25
COLUMNS = ("critic_obs", "features", "actions", "target_values", "advantages", "returns", "old_log_prob", "old_mu", "old_sigma")
SEED = 50


def main(seed=SEED, clip_actions=CLIP_ACTIONS, write=True):
    from rsl_rl.algorithms import ppo_ee as ppo_module
    from rsl_rl.algorithms.ppo_ee import PPO_EE
    from rsl_rl.modules import ActorCriticEE
    torch.set_num_threads(1)
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    ac = ActorCriticEE(N_COBS, A, F, NL, actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8], estimator_hidden_dims=[8, 4],
                       clip_actions=clip_actions).double()
    alg = PPO_EE(ac, num_learning_epochs=EPOCHS, num_mini_batches=MINI_BATCHES, learning_rate=LR0, max_grad_norm=MAX_GRAD_NORM,
                 schedule="adaptive", desired_kl=DESIRED_KL, entropy_coef=ENTROPY_COEF, clip_param=CLIP_PARAM, value_loss_coef=VALUE_LOSS_COEF,
                 use_clipped_value_loss=True, device="cpu", estimator_lr=EST_LR, num_estimator_epochs=EST_EPOCHS)
    alg.init_storage(N_ENVS, T, [N_COBS], [F], [NL], [A])
    for t in range(T):
        alg.act(torch.randn(N_ENVS, F, generator=g), torch.randn(N_ENVS, N_COBS, generator=g), torch.randn(N_ENVS, NL, generator=g))
        alg.process_env_step(torch.randn(N_ENVS, generator=g), (torch.rand(N_ENVS, generator=g) < P_DONE), {})
    alg.compute_returns(torch.randn(N_ENVS, N_COBS, generator=g))

    names = [n for n, _ in ac.named_parameters()]
    by_id = {id(p): n for n, p in ac.named_parameters()}
    rl_names = [by_id[id(p)] for p in alg.rl_parameters]
    est_params = list(ac.estimator.parameters())
    est_names = [by_id[id(p)] for p in est_params]
    n64 = lambda x: x.detach().numpy().astype(np.float64).copy()
    flat = lambda xs: np.concatenate([n64(x).reshape(-1) for x in xs])
    steps, est_steps = EPOCHS * MINI_BATCHES, EPOCHS * MINI_BATCHES * EST_EPOCHS
    arrays = {"names": np.array(names), "shapes": np.array([(list(p.shape) + [0, 0])[:2] for p in ac.parameters()], np.int64),
              "rl_names": np.array(rl_names), "est_names": np.array(est_names)}
    arrays["cfg"] = np.array([LR0, 0.9, 0.999, 1e-8, MAX_GRAD_NORM, DESIRED_KL, steps, CLIP_PARAM, VALUE_LOSS_COEF, ENTROPY_COEF, clip_actions,
                              EST_LR, est_steps, EST_EPOCHS], np.float64)
    arrays["init"] = flat(ac.parameters())
    rl_keys = COLUMNS + ("mu", "sigma", "values", "loss", "kl", "lr", "grad_norm", "grads", "params")
    est_keys = ("est_features", "est_labels", "est_terminated", "est_loss", "est_grads", "est_grad_norm", "est_params")
    rec = {k: [] for k in rl_keys + est_keys}
    saturated, margins = [], []

    clip0, adjust0, loss0, est_loss0 = ppo_module.nn.utils.clip_grad_norm_, alg._adjust_learning_rate, alg._compute_rl_loss, alg._compute_estimator_loss

    def compute_rl_loss(cobs, feats, actions, target_values, advantages, returns, old_log_prob, old_mu, old_sigma, hid, masks):
        for k, v in zip(COLUMNS, (cobs, feats, actions, target_values, advantages, returns, old_log_prob, old_mu, old_sigma)):
            rec[k].append(n64(v))
        out = loss0(cobs, feats, actions, target_values, advantages, returns, old_log_prob, old_mu, old_sigma, hid, masks)
        rec["mu"].append(n64(ac.action_mean))
        rec["sigma"].append(n64(ac.action_std))
        with torch.no_grad():
            rec["values"].append(n64(ac.evaluate(cobs)))
            pre = ac.actor[:-1](torch.cat((feats, ac.estimator(feats)), dim=-1))
        rec["loss"].append(float(out[0]))
        saturated.append(float((pre.abs() >= clip_actions).double().mean()))
        margins.append(float((pre.abs() - clip_actions).abs().min()))
        return out

    def compute_estimator_loss(feats, labels, terminated):
        rec["est_features"].append(n64(feats))
        rec["est_labels"].append(n64(labels))
        rec["est_terminated"].append(n64(terminated))
        out = est_loss0(feats, labels, terminated)
        rec["est_loss"].append(float(out))
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
            assert [id(p) for p in parameters] == [id(p) for p in est_params]
            rec["est_grads"].append(flat(p.grad for p in parameters))
            total = clip0(parameters, max_norm, *a, **k)
            rec["est_grad_norm"].append(float(total))
        return total

    alg._adjust_learning_rate, alg._compute_rl_loss, alg._compute_estimator_loss = adjust, compute_rl_loss, compute_estimator_loss
    ppo_module.nn.utils.clip_grad_norm_ = clip
    try:
        for opt, key in ((alg.optimizer, "params"), (alg.estimator_optimizer, "est_params")):
            def step(*a, _step0=opt.step, _key=key, **k):
                out = _step0(*a, **k)
                rec[_key].append(flat(ac.parameters()))
                return out
            opt.step = step
        alg.update()
    finally:
        ppo_module.nn.utils.clip_grad_norm_ = clip0
    assert all(len(rec[k]) == steps for k in rl_keys) and all(len(rec[k]) == est_steps for k in est_keys), {k: len(v) for k, v in rec.items()}
    assert all(0.1 <= s <= 0.9 for s in saturated), saturated
    assert all(m >= 1e-4 for m in margins), margins
    # no KL within 1 % of a threshold of the rate rule, no norm within 1 % of the clip: rounding to float32 moves no decision
    assert all(abs(k / (2 * DESIRED_KL) - 1.0) > 0.01 and abs(k / (DESIRED_KL / 2) - 1.0) > 0.01 and k > 0 for k in rec["kl"]), rec["kl"]
    assert all(abs(n / MAX_GRAD_NORM - 1.0) > 0.01 for n in rec["grad_norm"] + rec["est_grad_norm"]), (rec["grad_norm"], rec["est_grad_norm"])
    assert all(0 < t.sum() < t.size and set(np.unique(t)) <= {0.0, 1.0} for t in rec["est_terminated"]), [t.sum() for t in rec["est_terminated"]]
    for k, v in rec.items():
        arrays[k] = np.stack([np.asarray(x, np.float64) for x in v])
    if not write:
        return arrays
    rh.save("ppo_ee_train", arrays, "saturated", [f"{s:.2f}" for s in saturated], "margin", f"{min(margins):.2e}", "kl", [f"{k:.3e}" for k in rec["kl"]],
            "lr", [f"{x:.3e}" for x in rec["lr"]], "norm", [f"{n:.3f}" for n in rec["grad_norm"]], "est_norm", [f"{n:.3f}" for n in rec["est_grad_norm"]],
            "masked", [int(t.size - t.sum()) for t in rec["est_terminated"]])


if __name__ == "__main__":
    main()

"""Golden vectors for the fused optimizer step (include/lgoptim.h) from the reference's own PPO.update()
(rsl_rl/algorithms/ppo.py:124-148: per mini-batch the adaptive learning-rate rule, loss.backward(), clip_grad_norm_, Adam.step()) on a
tiny ActorCritic (actor and critic 7 -> 16 -> 8 -> A), everything float64 on the CPU, schedule="adaptive", 2 epochs x 3 mini-batches
over a storage filled through PPO.act / process_env_step from a seeded generator.

Build-container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_ppo_update_fixtures.py
Output: tests/golden/ppo_update.npz:
  names, shapes          the parameter names in the order of actor_critic.parameters(), and their shapes (rows, columns; 0: no such axis)
  cfg                    [lr0, beta1, beta2, eps, max_grad_norm, desired_kl, steps]
  init                   every parameter before the first step, flattened one behind the other in that order, float64
  kl, lr                 per step: the KL the rule saw and the learning rate in force for that step (after the rule), float64
  grad_norm              per step: what clip_grad_norm_ returned (the total norm before clipping), float64
  grads                  (steps, P) the gradients of each step before the clip, flattened likewise, float64
  params                 (steps, P) every parameter after each step, float64
torch.nn.utils.clip_grad_norm_ (as rsl_rl.algorithms.ppo sees it) is wrapped in a recorder that snapshots the gradients and the rate and
then calls the original; PPO._adjust_learning_rate in one that restates the KL of its arguments and then calls the original.
max_grad_norm is chosen so that some steps clip and some do not, desired_kl so that the rate rises, falls and stays; no KL lies within
1 % of a threshold of the rule, so rounding it to float32 moves no decision.  Written through ref_harness.save;
`python tests/golden/check_fixtures.py` checks that the output still equals the committed file."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

rh.load_reference()
import torch  # noqa: E402

LR0, MAX_GRAD_NORM, DESIRED_KL = 1e-3, 1.75, 1.5e-4
N_OBS, N_COBS, A, N_ENVS, T, EPOCHS, MINI_BATCHES = 7, 7, 3, 8, 6, 2, 3


def main(seed=53):
    from rsl_rl.algorithms import PPO, ppo as ppo_module
    from rsl_rl.modules import ActorCritic
    torch.set_num_threads(1)
    torch.set_default_dtype(torch.float64)          # the storage and the networks alike
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    ac = ActorCritic(N_OBS, N_COBS, A, actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8]).double()
    alg = PPO(ac, num_learning_epochs=EPOCHS, num_mini_batches=MINI_BATCHES, learning_rate=LR0, max_grad_norm=MAX_GRAD_NORM,
              schedule="adaptive", desired_kl=DESIRED_KL, entropy_coef=0.01, device="cpu")
    alg.init_storage(N_ENVS, T, [N_OBS], [N_COBS], [A])
    for t in range(T):
        alg.act(torch.randn(N_ENVS, N_OBS, generator=g), torch.randn(N_ENVS, N_COBS, generator=g))
        alg.process_env_step(torch.randn(N_ENVS, generator=g), (torch.rand(N_ENVS, generator=g) < 0.1), {})
    alg.compute_returns(torch.randn(N_ENVS, N_COBS, generator=g))

    names = [n for n, _ in ac.named_parameters()]
    n64 = lambda x: x.detach().numpy().astype(np.float64).copy()
    flat = lambda xs: np.concatenate([n64(x).reshape(-1) for x in xs])
    arrays = {"names": np.array(names), "shapes": np.array([(list(p.shape) + [0, 0])[:2] for p in ac.parameters()], np.int64)}
    arrays["cfg"] = np.array([LR0, 0.9, 0.999, 1e-8, MAX_GRAD_NORM, DESIRED_KL, EPOCHS * MINI_BATCHES], np.float64)
    arrays["init"] = flat(ac.parameters())
    kls, lrs, norms, grads = [], [], [], []

    clip0, adjust0 = ppo_module.nn.utils.clip_grad_norm_, alg._adjust_learning_rate

    def adjust(sigma, old_sigma, mu, old_mu):
        with torch.no_grad():
            kls.append(float(torch.sum(torch.log(sigma / old_sigma + 1.e-5) + (old_sigma ** 2 + (old_mu - mu) ** 2) / (2.0 * sigma ** 2) - 0.5,
                                       dim=-1).mean()))
        return adjust0(sigma, old_sigma, mu, old_mu)

    def clip(parameters, max_norm, *a, **k):
        parameters = list(parameters)
        assert max_norm == MAX_GRAD_NORM and len(parameters) == len(names)
        grads.append(flat(p.grad for p in parameters))
        lrs.append(float(alg.optimizer.param_groups[0]["lr"]))
        total = clip0(parameters, max_norm, *a, **k)
        norms.append(float(total))
        return total

    alg._adjust_learning_rate = adjust
    ppo_module.nn.utils.clip_grad_norm_ = clip
    try:
        # PPO.update() runs all six steps in one call; the parameters after each step are taken where the next step begins
        step0 = alg.optimizer.step
        after = []

        def step(*a, **k):
            out = step0(*a, **k)
            after.append(flat(ac.parameters()))
            return out
        alg.optimizer.step = step
        alg.update()
    finally:
        ppo_module.nn.utils.clip_grad_norm_ = clip0
    steps = EPOCHS * MINI_BATCHES
    assert len(kls) == len(lrs) == len(norms) == len(grads) == len(after) == steps
    arrays["grads"], arrays["params"] = np.stack(grads), np.stack(after)
    arrays["kl"], arrays["lr"], arrays["grad_norm"] = np.array(kls), np.array(lrs), np.array(norms)
    clipped = [n > MAX_GRAD_NORM for n in norms]
    assert any(clipped) and not all(clipped), norms
    assert all(abs(n / MAX_GRAD_NORM - 1.0) > 0.01 for n in norms), norms
    moves = [b / a for a, b in zip([LR0] + lrs[:-1], lrs)]
    assert any(m > 1 for m in moves) and any(m < 1 for m in moves) and any(m == 1 for m in moves), (kls, lrs)
    assert all(abs(k / (2 * DESIRED_KL) - 1.0) > 0.01 and abs(k / (DESIRED_KL / 2) - 1.0) > 0.01 and k > 0 for k in kls), kls
    rh.save("ppo_update", arrays, "kl", [f"{k:.3e}" for k in kls], "lr", [f"{x:.3e}" for x in lrs], "norm", [f"{n:.3f}" for n in norms])


if __name__ == "__main__":
    main()

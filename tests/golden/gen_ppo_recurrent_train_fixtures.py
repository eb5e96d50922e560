"""Golden vectors for the recurrent learner pass (include/lgtrainrnn.h) and for the whole fused recurrent update step (train pass, loss head,
optimizer) from the reference's own PPO.update() (rsl_rl/algorithms/ppo.py:124-148) on ActorCriticRecurrent
(rsl_rl/modules/actor_critic_recurrent.py): obs 7, critic obs 9, A = 3, H = 8, actor and critic 8 -> 16 -> 8 -> A / 1, a two-layer LSTM in
one file and a one-layer GRU in the other, everything float64 on the CPU, schedule="adaptive", 2 epochs x 2 mini-batches over 6 steps of 8
envs filled through PPO.act / process_env_step from a seeded generator.  The initial parameters and the drawn observations, rewards and
last critic observations are float32 values held in float64.

Build-container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_ppo_recurrent_train_fixtures.py
Output: tests/golden/ppo_recurrent_train_lstm.npz and tests/golden/ppo_recurrent_train_gru.npz:
  what gen_ppo_train_fixtures.py records (names, shapes, cfg, init, and per step the stored columns (T, E, .) of the mini-batch's envs, mu,
  sigma, values (T E, .) in the order of unpad_trajectories(...).flatten(0, 1), loss, kl, lr, grad_norm, grads), cfg with three more
  entries (T, the number of rnn layers, 1 for an LSTM), and
  param_steps                    (steps, n): every parameter after step s minus the same before it.  The parameters after step s are init plus
                                 the first s + 1 rows (to an ulp); a float64 step compresses where a float64 parameter does not, and the
                                 two-layer LSTM's 2903 parameters would otherwise make the largest fixture of the project
  padded_obs, padded_critic_obs  the padded set of the whole storage, (max_len, n_traj, .)
  masks                          (T, n_traj) bool
  hid_a_h, hid_a_c | hid_c_h     the start states of every trajectory, (layers, n_traj, H): an LSTM's actor's (h, c), which the reference hands its
                                 critic too (rollout_storage.py:231), or a GRU's actor's and critic's h
  traj_range, env_range          per step (first, last) of the mini-batch's trajectories and (start, stop) of its envs
ActorCriticRecurrent does not pass clip_actions on to ActorCritic; the generator sets the actor's Hardtanh itself.  The reference's
unpad_trajectories indexes the (max_len, n_traj) output with the (T, n_traj) masks and cannot take max_len < T; the generator pads the
memory's output with zero rows up to T first, which changes nothing where the reference works.
Asserted here (the seed conditions): in every mini-batch some env holds at least two trajectories; some trajectory has length 1; max_len <
T; between 10 % and 90 % of the means of every step saturate and no pre-clip mean lies within 1e-4 of +-clip_actions; no KL within 1 % of
a threshold of the rate rule, no norm within 1 % of the clip.  Written through ref_harness.save; `python tests/golden/check_fixtures.py`
checks that the output still equals the committed files."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

rh.load_reference()
import torch  # noqa: E402

LR0, MAX_GRAD_NORM, DESIRED_KL = 1e-3, 1.75, 1.5e-4
CLIP_PARAM, VALUE_LOSS_COEF, ENTROPY_COEF = 0.2, 1.0, 0.01
N_OBS, N_COBS, A, H, N_ENVS, T, EPOCHS, MINI_BATCHES, P_DONE, WARM_UP = 7, 9, 3, 8, 8, 6, 2, 2, 0.3, 3
COLUMNS = ("actions", "target_values", "advantages", "returns", "old_log_prob", "old_mu", "old_sigma")
SETS = {"lstm": dict(layers=2, seed=1, clip_actions=0.1), "gru": dict(layers=1, seed=1, clip_actions=0.1)}


def main(kind, layers, seed, clip_actions, save=True):
    from rsl_rl.algorithms import PPO, ppo as ppo_module
    from rsl_rl.modules import ActorCriticRecurrent, actor_critic_recurrent as acr
    torch.set_num_threads(1)
    torch.set_default_dtype(torch.float32)          # the initial parameters and every draw below are float32 values, held in float64: they
    torch.manual_seed(seed)                         # are what a float32 learner starts from exactly, and they compress
    g = torch.Generator().manual_seed(seed)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).double()
    ac = ActorCriticRecurrent(N_OBS, N_COBS, A, actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8], rnn_type=kind, rnn_hidden_size=H,
                              rnn_num_layers=layers).double()
    torch.set_default_dtype(torch.float64)
    ac.actor[-1] = torch.nn.Hardtanh(-clip_actions, clip_actions)
    alg = PPO(ac, num_learning_epochs=EPOCHS, num_mini_batches=MINI_BATCHES, learning_rate=LR0, max_grad_norm=MAX_GRAD_NORM,
              schedule="adaptive", desired_kl=DESIRED_KL, entropy_coef=ENTROPY_COEF, clip_param=CLIP_PARAM, value_loss_coef=VALUE_LOSS_COEF,
              use_clipped_value_loss=True, device="cpu")
    alg.init_storage(N_ENVS, T, [N_OBS], [N_COBS], [A])
    with torch.no_grad():                           # the runner collects without a graph: the hidden states carry none into the storage
        for t in range(WARM_UP):                    # an earlier rollout's last steps: the recorded one starts from states that are not zero
            alg.act(randn(N_ENVS, N_OBS), randn(N_ENVS, N_COBS))
            alg.process_env_step(randn(N_ENVS), torch.zeros(N_ENVS, dtype=torch.bool), {})
        alg.storage.clear()
        for t in range(T):
            alg.act(randn(N_ENVS, N_OBS), randn(N_ENVS, N_COBS))
            alg.process_env_step(randn(N_ENVS), (torch.rand(N_ENVS, generator=g) < P_DONE), {})
        alg.compute_returns(randn(N_ENVS, N_COBS))

    names = [n for n, _ in ac.named_parameters()]
    n64 = lambda x: x.detach().numpy().astype(np.float64).copy()
    flat = lambda xs: np.concatenate([n64(x).reshape(-1) for x in xs])
    steps = EPOCHS * MINI_BATCHES
    arrays = {"names": np.array(names), "shapes": np.array([(list(p.shape) + [0, 0])[:2] for p in ac.parameters()], np.int64)}
    arrays["cfg"] = np.array([LR0, 0.9, 0.999, 1e-8, MAX_GRAD_NORM, DESIRED_KL, steps, CLIP_PARAM, VALUE_LOSS_COEF, ENTROPY_COEF, clip_actions, T, layers,
                              float(kind == "lstm")], np.float64)
    arrays["init"] = flat(ac.parameters())
    rec = {k: [] for k in COLUMNS + ("mu", "sigma", "values", "loss", "kl", "lr", "grad_norm", "grads", "params", "traj_range", "env_range")}
    saturated, margins, padded, lens_per_env = [], [], {}, []

    def unpad(trajectories, masks):                 # the reference's, on an output padded back to the masks' T rows
        pad = trajectories.new_zeros((masks.shape[0] - trajectories.shape[0],) + tuple(trajectories.shape[1:]))
        return unpad0(torch.cat([trajectories, pad]), masks)

    clip0, adjust0, loss0, unpad0 = ppo_module.nn.utils.clip_grad_norm_, alg._adjust_learning_rate, alg._compute_rl_loss, acr.unpad_trajectories
    first = [0]

    def compute_rl_loss(obs, cobs, actions, target_values, advantages, returns, old_log_prob, old_mu, old_sigma, hid, masks):
        for k, v in zip(COLUMNS, (actions, target_values, advantages, returns, old_log_prob, old_mu, old_sigma)):
            rec[k].append(n64(v))
        i = len(rec["loss"]) % MINI_BATCHES
        if i == 0:
            first[0] = 0
        n_traj, e = int(masks.shape[1]), N_ENVS // MINI_BATCHES
        rec["traj_range"].append([first[0], first[0] + n_traj])
        rec["env_range"].append([i * e, (i + 1) * e])
        if len(rec["loss"]) < MINI_BATCHES:         # the first epoch sees every trajectory once
            lstm = isinstance(hid[0], (list, tuple))
            assert not lstm or hid[1] is hid[0]     # the reference hands an LSTM's critic the actor's start states
            for k, v in (("padded_obs", obs), ("padded_critic_obs", cobs), ("masks", masks), ("hid_a_h", hid[0][0] if lstm else hid[0]),
                         ("hid_a_c", hid[0][1] if lstm else None), ("hid_c_h", None if lstm else hid[1])):
                if v is not None:
                    padded.setdefault(k, []).append(v.detach().numpy().copy())
            lens_per_env.append(n64(masks.sum(0)))
        first[0] += n_traj
        out = loss0(obs, cobs, actions, target_values, advantages, returns, old_log_prob, old_mu, old_sigma, hid, masks)
        rec["mu"].append(n64(ac.action_mean.flatten(0, 1)))
        rec["sigma"].append(n64(ac.action_std.flatten(0, 1)))
        with torch.no_grad():
            rec["values"].append(n64(ac.evaluate(cobs, masks=masks, hidden_states=hid[1]).flatten(0, 1)))
            pre = ac.actor[:-1](ac.memory_a(obs, masks, hid[0]))
        rec["loss"].append(float(out[0].detach()))
        saturated.append(float((pre.abs() >= clip_actions).double().mean()))
        margins.append(float((pre.abs() - clip_actions).abs().min()))
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
    ppo_module.nn.utils.clip_grad_norm_, acr.unpad_trajectories = clip, unpad
    try:
        step0 = alg.optimizer.step

        def step(*a, **k):
            out = step0(*a, **k)
            rec["params"].append(flat(ac.parameters()))
            return out
        alg.optimizer.step = step
        alg.update()
    finally:
        ppo_module.nn.utils.clip_grad_norm_, acr.unpad_trajectories = clip0, unpad0
    assert all(len(v) == steps for v in rec.values()), {k: len(v) for k, v in rec.items()}
    # the seed conditions
    lens = np.concatenate(lens_per_env)
    assert all(len(l) > N_ENVS // MINI_BATCHES for l in lens_per_env), "in every mini-batch some env holds at least two trajectories"
    assert (lens == 1).any(), "some trajectory has length 1"
    assert padded["padded_obs"][0].shape[0] < T, "max_len < T"
    assert all(0.1 <= s <= 0.9 for s in saturated), saturated
    assert all(m >= 1e-4 for m in margins), margins
    # no KL within 1 % of a threshold of the rate rule, no norm within 1 % of the clip: rounding to float32 moves no decision
    assert all(abs(k / (2 * DESIRED_KL) - 1.0) > 0.01 and abs(k / (DESIRED_KL / 2) - 1.0) > 0.01 and k > 0 for k in rec["kl"]), rec["kl"]
    assert all(abs(n / MAX_GRAD_NORM - 1.0) > 0.01 for n in rec["grad_norm"]), rec["grad_norm"]
    for k, v in rec.items():
        arrays[k] = np.stack([np.asarray(x, np.int64 if k.endswith("_range") else np.float64) for x in v])
    arrays["param_steps"] = np.diff(np.concatenate([arrays["init"][None], arrays.pop("params")]), axis=0)
    for k, v in padded.items():
        arrays[k] = np.concatenate(v, axis=1)
    if save:
        rh.save(f"ppo_recurrent_train_{kind}", arrays, "lens", [int(n) for n in lens], "saturated", [f"{s:.2f}" for s in saturated], "margin",
                f"{min(margins):.2e}", "kl", [f"{k:.3e}" for k in rec["kl"]], "lr", [f"{x:.3e}" for x in rec["lr"]], "norm",
                [f"{n:.3f}" for n in rec["grad_norm"]])
    return arrays


if __name__ == "__main__":
    for kind, kw in SETS.items():
        main(kind, **kw)

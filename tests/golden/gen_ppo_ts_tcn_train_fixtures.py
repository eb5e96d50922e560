"""Golden vectors for the fused learner passes of ActorCriticTS with a "TCN" history encoder (include/lgtraintcn.h for the encoder pass,
include/lgtraints.h for the RL pass) and for the whole fused PPO_TS update from the reference's own PPO_TS.update()
(rsl_rl/algorithms/ppo_ts.py:95-187, the TCN branch of _compute_encoder_loss) on a tiny ActorCriticTS (O = 7 observations, P = 5 privileged
observations, Z = 3 latent dims, H = 14 history, 9 critic observations, A = 3; actor 10 -> 16 -> 8 -> 3, critic 9 -> 16 -> 8 -> 1,
privilege encoder 5 -> 8 -> 4 -> 3; history_encoder_type = "TCN" with channel dims [2, 3], dilation [1, 2], stride [1, 2], kernel_size 3,
final layer 4: Conv1d(1, 2, 3, padding 1), Conv1d(2, 3, 3, stride 2, padding 2, dilation 2), Flatten, Linear(21, 4), ELU, Linear(4, 3)),
everything float64 on the CPU, schedule="adaptive", 2 epochs x 3 mini-batches, num_encoder_epochs = 2, over a storage of 8 envs x 6 steps
filled through PPO_TS.act / process_env_step from a seeded generator with dones of probability 0.25.

Build-container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_ppo_ts_tcn_train_fixtures.py
Output: tests/golden/ppo_ts_tcn_train.npz, laid out as tests/golden/gen_ppo_ts_train_fixtures.py lays out ppo_ts_train.npz (names, shapes,
rl_names, enc_names, cfg, init, the per-RL-step and per-encoder-step arrays), with `shapes` in three columns (a Conv1d weight is (c_out,
c_in, k); unused columns are 0) and enc_history as _compute_encoder_loss received it, (B, H), before its unsqueeze.  The same margins are
asserted here, so that rounding to float32 moves no decision: no KL within 1 % of a threshold of the rate rule; no gradient norm (either
loop) within 1 % of max_grad_norm; every encoder batch has a masked and an unmasked row.  Arrays only.  Written through ref_harness.save;
`python tests/golden/check_fixtures.py` checks that the output still equals the committed file."""
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
O, P, Z, H, N_COBS, A, N_ENVS, T, EPOCHS, MINI_BATCHES, ENC_EPOCHS, P_DONE = 7, 5, 3, 14, 9, 3, 8, 6, 2, 3, 2, 0.25
COLUMNS = ("obs", "privileged_obs", "critic_obs", "actions", "target_values", "advantages", "returns", "old_log_prob", "old_mu", "old_sigma")
SEED = 50


def main(seed=SEED, write=True):
    from rsl_rl.algorithms import ppo_ts as ppo_module
    from rsl_rl.algorithms.ppo_ts import PPO_TS
    from rsl_rl.modules import ActorCriticTS
    torch.set_num_threads(1)
    torch.set_default_dtype(torch.float64)
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    ac = ActorCriticTS(O, A, P, H, Z, N_COBS, actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8], privilege_encoder_hidden_dims=[8, 4],
                       history_encoder_type="TCN", history_encoder_channel_dims=[2, 3], history_encoder_dilation=[1, 2],
                       history_encoder_stride=[1, 2], history_encoder_final_layer_dim=4, kernel_size=3).double()
    alg = PPO_TS(ac, num_learning_epochs=EPOCHS, num_mini_batches=MINI_BATCHES, learning_rate=LR0, max_grad_norm=MAX_GRAD_NORM,
                 schedule="adaptive", desired_kl=DESIRED_KL, entropy_coef=ENTROPY_COEF, clip_param=CLIP_PARAM, value_loss_coef=VALUE_LOSS_COEF,
                 use_clipped_value_loss=True, device="cpu", encoder_lr=ENC_LR, num_encoder_epochs=ENC_EPOCHS)
    alg.init_storage(N_ENVS, T, [O], [P], [H], [N_COBS], [A])
    for t in range(T):
        alg.act(torch.randn(N_ENVS, O, generator=g), torch.randn(N_ENVS, P, generator=g), torch.randn(N_ENVS, H, generator=g),
                torch.randn(N_ENVS, N_COBS, generator=g))
        alg.process_env_step(torch.randn(N_ENVS, generator=g), (torch.rand(N_ENVS, generator=g) < P_DONE), {})
    alg.compute_returns(torch.randn(N_ENVS, N_COBS, generator=g))

    names = [n for n, _ in ac.named_parameters()]
    by_id = {id(p): n for n, p in ac.named_parameters()}
    rl_names = [by_id[id(p)] for p in alg.rl_parameters]
    enc_params = list(ac.history_encoder.parameters())
    enc_names = [by_id[id(p)] for p in enc_params]
    n64 = lambda x: x.detach().numpy().astype(np.float64).copy()
    flat = lambda xs: np.concatenate([n64(x).reshape(-1) for x in xs])
    steps, enc_steps = EPOCHS * MINI_BATCHES, EPOCHS * MINI_BATCHES * ENC_EPOCHS
    arrays = {"names": np.array(names), "shapes": np.array([(list(p.shape) + [0, 0, 0])[:3] for p in ac.parameters()], np.int64),
              "rl_names": np.array(rl_names), "enc_names": np.array(enc_names)}
    arrays["cfg"] = np.array([LR0, 0.9, 0.999, 1e-8, MAX_GRAD_NORM, DESIRED_KL, steps, CLIP_PARAM, VALUE_LOSS_COEF, ENTROPY_COEF, ENC_LR, enc_steps,
                              ENC_EPOCHS], np.float64)
    arrays["init"] = flat(ac.parameters())
    rl_keys = COLUMNS + ("mu", "sigma", "values", "loss", "kl", "lr", "grad_norm", "grads", "params")
    enc_keys = ("enc_history", "enc_privileged", "enc_terminated", "enc_loss", "enc_grads", "enc_grad_norm", "enc_params")
    rec = {k: [] for k in rl_keys + enc_keys}

    clip0, adjust0, loss0, enc_loss0 = ppo_module.nn.utils.clip_grad_norm_, alg._adjust_learning_rate, alg._compute_rl_loss, alg._compute_encoder_loss

    def compute_rl_loss(obs, pobs, cobs, actions, target_values, advantages, returns, old_log_prob, old_mu, old_sigma, hid, masks):
        for k, v in zip(COLUMNS, (obs, pobs, cobs, actions, target_values, advantages, returns, old_log_prob, old_mu, old_sigma)):
            rec[k].append(n64(v))
        out = loss0(obs, pobs, cobs, actions, target_values, advantages, returns, old_log_prob, old_mu, old_sigma, hid, masks)
        rec["mu"].append(n64(ac.action_mean))
        rec["sigma"].append(n64(ac.action_std))
        with torch.no_grad():
            rec["values"].append(n64(ac.evaluate(cobs)))
        rec["loss"].append(float(out[0]))
        return out

    def compute_encoder_loss(history, pobs, terminated):
        rec["enc_history"].append(n64(history))
        rec["enc_privileged"].append(n64(pobs))
        rec["enc_terminated"].append(n64(terminated))
        out = enc_loss0(history, pobs, terminated)
        rec["enc_loss"].append(float(out))
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
            assert all(p.grad is None for p in enc_params) or len(rec["enc_grads"]) > 0      # the RL loss sends nothing into the history encoder
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

    alg._adjust_learning_rate, alg._compute_rl_loss, alg._compute_encoder_loss = adjust, compute_rl_loss, compute_encoder_loss
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
    # no KL within 1 % of a threshold of the rate rule, no norm within 1 % of the clip: rounding to float32 moves no decision
    assert all(abs(k / (2 * DESIRED_KL) - 1.0) > 0.01 and abs(k / (DESIRED_KL / 2) - 1.0) > 0.01 and k > 0 for k in rec["kl"]), rec["kl"]
    assert all(abs(n / MAX_GRAD_NORM - 1.0) > 0.01 for n in rec["grad_norm"] + rec["enc_grad_norm"]), (rec["grad_norm"], rec["enc_grad_norm"])
    assert all(0 < t.sum() < t.size and set(np.unique(t)) <= {0.0, 1.0} for t in rec["enc_terminated"]), [t.sum() for t in rec["enc_terminated"]]
    for k, v in rec.items():
        arrays[k] = np.stack([np.asarray(x, np.float64) for x in v])
    if not write:
        return arrays
    rh.save("ppo_ts_tcn_train", arrays, "kl", [f"{k:.3e}" for k in rec["kl"]], "lr", [f"{x:.3e}" for x in rec["lr"]],
            "norm", [f"{n:.3f}" for n in rec["grad_norm"]], "enc_norm", [f"{n:.3f}" for n in rec["enc_grad_norm"]],
            "masked", [int(t.size - t.sum()) for t in rec["enc_terminated"]])


if __name__ == "__main__":
    main()

"""Golden vectors for the recurrent half of the rollout storage from the reference's own rsl_rl classes: PPO with ActorCriticRecurrent
(rsl_rl/modules/actor_critic_recurrent.py; LSTM and GRU, 2 layers x 32) filling a RolloutStorage over TWO consecutive rollouts
(rsl_rl/storage/rollout_storage.py:89-119: the second one starts with hidden states, the first with None), compute_returns, and every
tensor that reccurent_mini_batch_generator(4, 1) yields (:187-236, through rsl_rl/utils/utils.py:33-65).  PPO.process_env_step zeroes
the hidden states of finished envs (ppo.py:117), so the stored start states behind a done are zero rows and the others are not.

Build-container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_rollout_recurrent_fixtures.py
Output: tests/golden/rollout_recurrent_<rnn>_r<k>_<part>.npz for rnn in lstm / gru, rollout k in 0 / 1, split into parts so that every
file stays under the committed-file limit (steps: per-step inputs and the storage's value-derived tensors; hidden_a / hidden_c: the
full saved_hidden_states_a / _c; batches_obs / batches_rest: every yielded tensor of every mini-batch, plus the LSTM critic's own start
states that the reference does not yield), and tests/golden/rollout_recurrent_short.npz (every env done at the same step, so that the
longest trajectory is shorter than the rollout).
Written through ref_harness.save; `python tests/golden/check_fixtures.py` checks that the output still equals the committed files."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

rh.load_reference()
import torch  # noqa: E402

LIMIT = 1 << 20
YIELD = ("obs", "critic_obs", "actions", "values", "advantages", "returns", "logp", "mu", "sigma")


def save(name, arrays):
    path = rh.save(name, arrays)
    assert os.path.getsize(path) < LIMIT, path


def as_lists(hidden_states):
    """(actor tensors, critic tensors) of what ActorCriticRecurrent.get_hidden_states returns, None before the first act."""
    hid_a, hid_c = hidden_states
    if hid_a is None and hid_c is None:
        return None
    tup = lambda h: tuple(h) if isinstance(h, (tuple, list)) else (h,)
    return [x.numpy().copy() for x in tup(hid_a)], [x.numpy().copy() for x in tup(hid_c)]


def trajectory_starts(dones):
    """(env, t_start) of every trajectory, env-major then by time: t = 0 and every step behind a done."""
    T, N = dones.shape
    return [(e, t) for e in range(N) for t in range(T) if t == 0 or dones[t - 1, e]]


def run(rnn, N=48, T=24, seed=5):
    from rsl_rl.algorithms import PPO
    from rsl_rl.modules import ActorCriticRecurrent
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    ac = ActorCriticRecurrent(45, 61, 12, actor_hidden_dims=[32, 16], critic_hidden_dims=[32, 16], activation="elu", rnn_type=rnn,
                              rnn_hidden_size=32, rnn_num_layers=2, init_noise_std=1.0)
    alg = PPO(ac, device="cpu")
    alg.init_storage(N, T, [45], [61], [12])
    obs = torch.from_numpy(rng.normal(size=(N, 45)).astype(np.float32))
    cobs = torch.from_numpy(rng.normal(size=(N, 61)).astype(np.float32))
    n_traj = []
    for k in range(2):
        out = {n: [] for n in ("obs", "critic_obs", "actions", "values", "logp", "mu", "sigma", "rew", "dones", "time_outs")}
        handed = []
        with torch.inference_mode():
            for t in range(T):
                handed.append(as_lists(ac.get_hidden_states()))          # what PPO.act puts into the transition
                actions = alg.act(obs, cobs)
                tr = alg.transition
                out["obs"].append(obs.numpy().copy()); out["critic_obs"].append(cobs.numpy().copy())
                out["actions"].append(actions.numpy().copy()); out["values"].append(tr.values.numpy().copy())
                out["logp"].append(tr.actions_log_prob.numpy().copy()); out["mu"].append(tr.action_mean.numpy().copy())
                out["sigma"].append(tr.action_sigma.numpy().copy())
                rew = torch.from_numpy((rng.normal(size=N) * 0.05 + 0.02).astype(np.float32))
                dones = torch.from_numpy(rng.random(N) < 0.08)
                time_outs = dones & torch.from_numpy(rng.random(N) < 0.5)
                out["rew"].append(rew.numpy().copy()); out["dones"].append(dones.numpy().astype(np.uint8))
                out["time_outs"].append(time_outs.numpy().astype(np.uint8))
                alg.process_env_step(rew, dones, {"time_outs": time_outs})
                obs = torch.from_numpy(rng.normal(size=(N, 45)).astype(np.float32))
                cobs = torch.from_numpy(rng.normal(size=(N, 61)).astype(np.float32))
            critic_memory = ac.memory_c.hidden_states
            last_values = alg.actor_critic.evaluate(cobs).detach()      # recorded for the GAE check ...
            ac.memory_c.hidden_states = critic_memory                    # ... without a second step of the critic's memory
            alg.compute_returns(cobs)
            st = alg.storage
            batches = list(st.reccurent_mini_batch_generator(4, 1))
        steps = {n: np.stack(v) for n, v in out.items()}
        steps.update(gamma=np.float32(alg.gamma), lam=np.float32(alg.lam), last_values=last_values.numpy().copy(),
                     hidden_none_at_step0=np.bool_(handed[0] is None))
        for n, src in (("observations", "obs"), ("privileged_observations", "critic_obs"), ("actions", "actions"), ("mu", "mu"), ("sigma", "sigma")):
            assert np.array_equal(getattr(st, n).numpy(), steps[src]), n
        assert np.array_equal(st.values.numpy(), steps["values"]) and np.array_equal(st.actions_log_prob.numpy()[..., 0], steps["logp"])
        for n in ("rewards", "dones", "returns", "advantages"):
            steps["st_" + n] = getattr(st, n).numpy().copy()
        saved_a = [x.numpy().copy() for x in st.saved_hidden_states_a]
        saved_c = [x.numpy().copy() for x in st.saved_hidden_states_c]
        # the hidden states handed to add_transitions at step t ARE row t of the saved tensors, so they are stored once; the only step
        # with nothing handed over is step 0 of the first rollout, whose row stays zero
        assert (handed[0] is None) == (k == 0) and all(h is not None for h in handed[1:])
        for t in range(T):
            if handed[t] is None:
                assert not any(x[t].any() for x in saved_a + saved_c)
            else:
                assert all(np.array_equal(x[t], h) for x, h in zip(saved_a + saved_c, handed[t][0] + handed[t][1]))
        d = steps["dones"].astype(bool)
        starts = trajectory_starts(d)
        per_env = np.bincount([e for e, _ in starts], minlength=N)
        assert d.sum() > steps["time_outs"].sum() > 0 and (d.sum(0) == 0).any() and (per_env >= 3).any()
        nonzero_start = [bool(saved_a[0][t, :, e].any()) for e, t in starts]
        # first rollout: every trajectory starts from zeros (nothing handed over at t = 0, zeroed behind a done); second: the t = 0 rows do not
        assert not any(nonzero_start) if k == 0 else (any(nonzero_start) and not all(nonzero_start))
        n_traj.append(len(starts))
        obs_part, rest = {}, {}
        first = 0
        for b, batch in enumerate(batches):
            for n, x in zip(YIELD, batch[:9]):
                (obs_part if n in ("obs", "critic_obs") else rest)[f"b{b}_{n}"] = x.numpy().copy()
            obs_part[f"b{b}_masks"] = batch[10].numpy().copy()
            hid_a, hid_c = batch[9]
            for side, hid in (("a", hid_a), ("c", hid_c)):
                hid = hid if isinstance(hid, (list, tuple)) else [hid]
                for i, x in enumerate(hid):
                    assert x.is_contiguous()
                    rest[f"b{b}_hid_{side}{i}"] = x.numpy().copy()
            last = first + batch[10].shape[1]
            for i, x in enumerate(saved_c):                              # the critic's own start states ("own" mode), (L, trajectories, H)
                rest[f"b{b}_own_c{i}"] = np.stack([x[t, :, e, :] for e, t in starts[first:last]], axis=1)
            if rnn == "lstm":                                            # rollout_storage.py:231: the critic is handed the actor's
                assert all(np.array_equal(rest[f"b{b}_hid_c{i}"], rest[f"b{b}_hid_a{i}"]) for i in range(2))
                assert k == 0 or not all(np.array_equal(rest[f"b{b}_own_c{i}"], rest[f"b{b}_hid_c{i}"]) for i in range(2))
            else:
                assert np.array_equal(rest[f"b{b}_own_c0"], rest[f"b{b}_hid_c0"])
            first = last
        assert first == len(starts)
        save(f"rollout_recurrent_{rnn}_r{k}_steps", steps)
        save(f"rollout_recurrent_{rnn}_r{k}_hidden_a", {f"saved_a{i}": x for i, x in enumerate(saved_a)})
        save(f"rollout_recurrent_{rnn}_r{k}_hidden_c", {f"saved_c{i}": x for i, x in enumerate(saved_c)})
        save(f"rollout_recurrent_{rnn}_r{k}_batches_obs", obs_part)
        save(f"rollout_recurrent_{rnn}_r{k}_batches_rest", rest)
        st.clear()
    print(rnn, "trajectories per rollout", n_traj)


def short():
    """T = 6, N = 3, every env done at t = 2: two trajectories of length 3 per env, so pad_sequence gives 3 rows and the mask keeps 6."""
    from rsl_rl.utils import split_and_pad_trajectories
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.normal(size=(6, 3, 5)).astype(np.float32))
    dones = torch.zeros(6, 3, 1, dtype=torch.uint8)
    dones[2] = 1
    padded, masks = split_and_pad_trajectories(x, dones)
    assert padded.shape == (3, 6, 5) and masks.shape == (6, 6)
    save("rollout_recurrent_short", dict(x=x.numpy(), dones=dones.numpy(), padded=padded.numpy().copy(), masks=masks.numpy().copy()))


if __name__ == "__main__":
    run("lstm")
    run("gru")
    short()

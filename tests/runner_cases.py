"""The runner's book-keeping cases, shared by tests/test_runner_host.py (CPU) and tests/test_gpu_runner.py (GPU): one case table, the
restatement of rsl_rl/runners/on_policy_runner.py:130-136 in numpy and collections.deque, the restatement of the episode-info mean in
float64, the reader of tests/golden/runner_learn.npz, and the scripted env and module that replay it.  Nothing here loads the HIP library."""
import os
from collections import deque

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "runner_learn.npz")
STEPS = 8
STATS_N = (1, 63, 64, 65, 1023, 1024, 1025, 4096)     # the wave edge and the workgroup tile edge
STATS_CAP = (1, 7, 100)
INFO_R, INFO_N = (1, 35), (1, 65, 1025, 4096)


def done_counts(n, cap):
    """Dones per step over the first six of the 8 steps: 1, cap, 0, cap - 1, cap + 1 and all N (each clipped to N); two seeded steps
    follow.  The step of cap pushes starts at ring position 1, so with N >= cap > 1 it wraps in its middle (`wraps_mid_step`)."""
    return [min(k, n) for k in (1, cap, 0, cap - 1, cap + 1, n)]


def wraps_mid_step(dones, cap):
    """Does some step start at a ring position p > 0 and push more than cap - p episodes?"""
    count = 0
    for d in dones:
        k = int(np.count_nonzero(d))
        if count % cap and k > cap - count % cap:
            return True
        count += k
    return False


def stats_inputs(n, cap, seed, dtype=np.uint8):
    """(rewards (8, n) float32, dones (8, n) dtype): the done counts of `done_counts` at seeded places, two more steps at p = 0.3; a NaN
    and an inf reward on envs that finish later, so both reach the ring."""
    rng = np.random.default_rng(seed)
    rew = (rng.normal(size=(STEPS, n)) * 0.7 + 0.1).astype(np.float32)
    dones = np.zeros((STEPS, n), bool)
    for s, k in enumerate(done_counts(n, cap)):
        dones[s, rng.choice(n, size=k, replace=False)] = True
    dones[6:] = rng.random((2, n)) < 0.3
    rew[0, 0] = np.nan
    rew[3, n // 2] = np.inf
    return rew, dones.astype(dtype)


class StatsRestatement:
    """on_policy_runner.py:130-136, statement by statement, in numpy float32 and collections.deque."""

    def __init__(self, n, cap=100):
        self.rewbuffer, self.lenbuffer = deque(maxlen=cap), deque(maxlen=cap)
        self.cur_reward_sum, self.cur_episode_length = np.zeros(n, np.float32), np.zeros(n, np.float32)
        self.count = 0

    def update(self, rewards, dones):
        self.cur_reward_sum += np.asarray(rewards, np.float32)
        self.cur_episode_length += np.float32(1)
        new_ids = np.nonzero(np.asarray(dones) > 0)[0]
        self.rewbuffer.extend(self.cur_reward_sum[new_ids].tolist())
        self.lenbuffer.extend(self.cur_episode_length[new_ids].tolist())
        self.cur_reward_sum[new_ids] = 0
        self.cur_episode_length[new_ids] = 0
        self.count += len(new_ids)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


class InfoRestatement:
    """The episode-info log in float64: `last` is the mean over the envs reset at this step of their snapshot sums, times the inverse
    episode length; it stays where no env reset and is zero before any reset; `acc` adds it every step."""

    def __init__(self, rows):
        self.last, self.acc, self.n_acc = np.zeros(rows), np.zeros(rows), 0

    def update(self, sums, done_step, step, inv_len):
        m = np.asarray(done_step) == step
        if m.any():
            self.last = np.asarray(sums, np.float64)[:, m].mean(axis=1) * inv_len
        self.acc = self.acc + self.last
        self.n_acc += 1

    def means(self):
        return self.acc / self.n_acc


def info_steps(rows, n, seed):
    """[(sums (rows, n) float32, done_step (n,) int32, step)]: before any reset, one reset, none, all envs, a seeded share, none."""
    rng = np.random.default_rng(seed)
    done_step = np.full(n, -1, np.int32)
    sums = np.zeros((rows, n), np.float32)
    out = []
    for step, who in enumerate(("none", "one", "none", "all", "some", "none"), start=5):
        m = {"none": np.zeros(n, bool), "one": np.arange(n) == n // 3, "all": np.ones(n, bool), "some": rng.random(n) < 0.4}[who]
        done_step = np.where(m, step, done_step).astype(np.int32)
        fresh = (rng.normal(size=(rows, n)) * 5 + rng.normal(size=(rows, 1)) * 50).astype(np.float32)
        sums = np.where(m[None, :], fresh, sums).astype(np.float32)
        out.append((sums.copy(), done_step.copy(), step))
    return out


# ---- the golden fixture (tests/golden/gen_runner_fixtures.py) ---------------------------------------------------------------------------------
CFG_KEYS = ("num_envs", "steps", "iterations", "epochs", "mini_batches", "lr0", "desired_kl", "gamma", "lam", "clip", "entropy_coef",
            "max_grad_norm", "value_loss_coef", "episode_length_s", "capacity")


def load_fixture(path=GOLDEN):
    z = np.load(path)
    fx = {k: z[k] for k in z.files}
    cfg = dict(zip(CFG_KEYS, (float(v) for v in z["cfg"])))
    for k in ("num_envs", "steps", "iterations", "epochs", "mini_batches", "capacity"):
        cfg[k] = int(cfg[k])
    fx["cfg"] = cfg
    fx["names"] = [str(n) for n in z["names"]]
    fx["shape_of"] = {n: tuple(int(d) for d in s if d) for n, s in zip(fx["names"], z["shapes"])}
    fx["ep_keys"] = [str(k) for k in z["ep_keys"]]
    return fx


def split_params(fx, flat):
    out, at = {}, 0
    for n in fx["names"]:
        size = int(np.prod(fx["shape_of"][n]))
        out[n] = np.asarray(flat[at:at + size]).reshape(fx["shape_of"][n]).copy()
        at += size
    assert at == len(flat)
    return out


def fixture_episode_values(fx):
    """infos['episode'][key] of every step as the scripted env of the generator forms it, in float64: (S, R)."""
    inv = 1.0 / fx["cfg"]["episode_length_s"]
    S = fx["rew"].shape[0]
    r = InfoRestatement(len(fx["ep_keys"]))
    out = []
    for s in range(S):
        r.update(fx["ep_sums"][s], np.where(fx["dones"][s], s, -1), s, inv)
        out.append(r.last.copy())
    return np.array(out)


def train_cfg(fx):
    c = fx["cfg"]
    return dict(runner=dict(policy_class_name="ActorCritic", algorithm_class_name="PPO", num_steps_per_env=c["steps"], save_interval=1000,
                            experiment_name="runner_fixture", run_name=""),
                algorithm=dict(num_learning_epochs=c["epochs"], num_mini_batches=c["mini_batches"], clip_param=c["clip"], gamma=c["gamma"],
                               lam=c["lam"], value_loss_coef=c["value_loss_coef"], entropy_coef=c["entropy_coef"], learning_rate=c["lr0"],
                               max_grad_norm=c["max_grad_norm"], use_clipped_value_loss=True, schedule="adaptive", desired_kl=c["desired_kl"]),
                policy=dict(actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8], activation="elu", init_noise_std=1.0))


def make_actor_critic(n_obs, n_critic_obs, n_actions, actor_hidden, critic_hidden, clip_actions=100.0, **extra):
    """rsl_rl.modules.ActorCritic's members and parameter order (std, actor.*, critic.*) as a plain torch module; `extra`: members of
    another family by name (memory_a=..., estimator=...), for the refusals."""
    import torch
    nn = torch.nn

    def mlp(i, hidden, o, tail=None):
        layers, d = [], i
        for h in hidden:
            layers += [nn.Linear(d, h), nn.ELU()]
            d = h
        layers.append(nn.Linear(d, o))
        if tail is not None:
            layers.append(tail)
        return nn.Sequential(*layers)

    class ActorCritic(nn.Module):
        is_recurrent = False

        def __init__(self):
            super().__init__()
            self.std = nn.Parameter(torch.ones(n_actions))
            self.actor = mlp(n_obs, actor_hidden, n_actions, nn.Hardtanh(-clip_actions, clip_actions))
            self.critic = mlp(n_critic_obs, critic_hidden, 1)
            for k, v in extra.items():
                setattr(self, k, v)
    return ActorCritic()


class Recorder:
    """A writer: anything with add_scalar."""

    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), step))


class ReplayEnv:
    """The VecEnv surface around the fixture's arrays on a device, the reset snapshot stated through `episode_info_source` as a fused
    env's engine states it: step s copies ep_sums[s] into the rows of the envs it resets and writes s into their done_step."""

    def __init__(self, fx, device):
        import torch
        t = lambda a, **k: torch.as_tensor(np.ascontiguousarray(a), **k).to(device)
        self.device, self.s = device, 0
        self.obs, self.priv, self.rew = t(fx["obs"]), t(fx["priv"]), t(fx["rew"])
        self.dones, self.time_outs, self.ep_sums = t(fx["dones"]), t(fx["time_outs"]), t(fx["ep_sums"])
        self.num_envs, self.num_obs, self.num_privileged_obs = self.obs.shape[1], self.obs.shape[2], self.priv.shape[2]
        self.num_actions, self.max_episode_length = fx["noise"].shape[2], 1000
        self.episode_length_buf = torch.zeros(self.num_envs, dtype=torch.long, device=device)
        self.keys = [(k, r) for r, k in enumerate(fx["ep_keys"])]
        self.inv_len = 1.0 / fx["cfg"]["episode_length_s"]
        self.done_sums = torch.zeros(len(self.keys), self.num_envs, device=device)
        self.done_step = torch.full((self.num_envs,), -1, dtype=torch.int32, device=device)
        self.actions = []

    def get_observations(self):
        return self.obs[self.s]

    def get_privileged_observations(self):
        return self.priv[self.s]

    def reset(self):
        return self.get_observations(), self.get_privileged_observations()

    def step(self, actions):
        import torch
        s = self.s
        self.actions.append(actions.clone())
        m = self.dones[s]
        self.done_sums.copy_(torch.where(m[None, :], self.ep_sums[s], self.done_sums))
        self.done_step.copy_(torch.where(m, torch.full_like(self.done_step, s), self.done_step))
        self.s += 1
        return self.obs[self.s], self.priv[self.s], self.rew[s], m, {"time_outs": self.time_outs[s]}

    def episode_info_source(self):
        return dict(sums_a=self.done_sums, sums_b=None, done_step=self.done_step, step=self.s - 1, inv_episode_length_s=self.inv_len,
                    keys=self.keys)

"""The training loop of the plain ActorCritic learner, put together from the fused pieces: `PPO` (rsl_rl/algorithms/ppo.py), `OnPolicyRunner`
(rsl_rl/runners/on_policy_runner.py) and `EpisodeStats`, the runner's per-step book-keeping on the device (include/lgrunner.h).

  * `EpisodeStats`: on_policy_runner.py:126-136 keeps two `deque(maxlen=100)` on the host and pays `(dones > 0).nonzero()` and two
    `.cpu().numpy().tolist()` per env step with logging on; `ep_infos.append(infos['episode'])` reads the env's lazy episode dict, which
    synchronises too.  Here both are one launch each per step (`lg_runner_episode_stats`, `lg_runner_episode_info`) on state that stays on
    the device, and `read()` is the one copy to the host, at log time.
  * `PPO`: the reference's constructor keywords and surface, built from `FusedPolicy` (act, evaluate), `RolloutStorage` (record, GAE, the
    mini-batch gather), `FusedTrainPass`, `FusedPPOLoss` and `FusedAdam` (clip, the KL-adaptive rate on the device, Adam).
  * `OnPolicyRunner`: `learn`, `log`, `save`, `load`, `get_inference_policy` with the reference's checkpoint keys and scalar tags.  The rollout
    loop issues, per step, the policy launch, the env step, the record launch and the two stats launches, and nothing else.

Only the plain `ActorCritic` is built: recurrent, EE, TS, CTS and DreamWaQ modules are refused by name.  There is no CPU path."""
from __future__ import annotations

import os
import statistics
import time

import torch

from . import abi
from .optim import FusedAdam
from .policy import FusedPolicy
from .ppo_loss import FusedPPOLoss
from .rollout import RolloutStorage
from .train import FusedTrainPass

_FOREIGN = (("memory_a", "ActorCriticRecurrent"), ("memory_c", "ActorCriticRecurrent"), ("estimator", "ActorCriticEE"),
            ("privilege_encoder", "ActorCriticTS / ActorCriticCTS"), ("history_encoder", "ActorCriticTS / ActorCriticCTS"),
            ("vae", "ActorCriticDreamWaQ"))
_POLICY_CLASSES, _ALGORITHM_CLASSES = ("ActorCritic",), ("PPO",)


def _call(dev, name, *args):
    """Entry point `name` of include/lgrunner.h on the current stream of `dev` (each takes the stream last); a refusal is a RuntimeError."""
    lib = abi.load_lib()
    abi.check(getattr(lib, name)(*args, torch.cuda.current_stream(dev).cuda_stream), lib)


def _hip_device(device, owner):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"{owner}: the module is on {dev}, not on a HIP device (there is no CPU path)")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _refuse_families(actor_critic, owner):
    for attr, family in _FOREIGN:
        if getattr(actor_critic, attr, None) is not None:
            raise ValueError(f"{owner}: the module has .{attr} ({family}); only the plain ActorCritic learner is built, the other learners "
                             "keep the reference's loop around their fused pieces")
    if getattr(actor_critic, "is_recurrent", False):
        raise ValueError(f"{owner}: the module is recurrent (is_recurrent); only the plain ActorCritic learner is built")
    for need in ("actor", "critic", "std"):
        if getattr(actor_critic, need, None) is None:
            raise ValueError(f"{owner}: the module has no .{need}")


# ---- the book-keeping ---------------------------------------------------------------------------------------------------------------
def episode_info_source(env):
    """What `lg_runner_episode_info` reads of an env: dict(sums_a (R, N) f32, sums_b (R2, N) f32 or None, done_step (N,) int32, step,
    inv_episode_length_s, keys = [(episode key, row)]).  An env may state it itself (`env.episode_info_source()`); a fused env of this
    package is read through its engine: the step kernels snapshot every resetting env's episode sums into `episode_done_sums` (go2_cat:
    also the constraint counters into `cstr_done_sums`, the second row block) and the step index into `episode_done_step`."""
    own = getattr(env, "episode_info_source", None)
    if own is not None:
        return own()
    buf, jpl = env._engine.buf, env.simulator._model.joints_per_leg
    keys = []
    for name in env.episode_sums:
        row = abi.R_COUNT + abi.CSTR_NAMES.index(name[5:]) if name.startswith("cstr_") else abi.reward_id(name, jpl)
        keys.append(("rew_" + name, row))
    sums_b = buf["cstr_done_sums"] if any(r >= abi.R_COUNT for _, r in keys) else None
    return dict(sums_a=buf["episode_done_sums"], sums_b=sums_b, done_step=buf["episode_done_step"], step=int(env.common_step_counter),
                inv_episode_length_s=1.0 / float(env.max_episode_length_s), keys=keys)


class EpisodeStats:
    """`rewbuffer`, `lenbuffer`, `cur_reward_sum`, `cur_episode_length` and the `ep_infos` means of the reference's runner, on the device.

    `update(rewards, dones)` and `update_info(env)` are one launch each, read nothing back and do not synchronise (`update` can be
    captured in a HIP graph: every address is fixed at construction).  `read()` is one copy to the host."""

    def __init__(self, num_envs, capacity=100, device="cuda:0"):
        if int(capacity) < 1:
            raise ValueError(f"EpisodeStats: capacity = {capacity}; the ring holds at least one episode")
        if int(num_envs) < 1:
            raise ValueError(f"EpisodeStats: num_envs = {num_envs}")
        self.device = _hip_device(device, "EpisodeStats")
        self.num_envs, self.capacity = int(num_envs), int(capacity)
        z = lambda *s, **k: torch.zeros(*s, device=self.device, **k)
        self._cur = z(2, self.num_envs)                      # cur_reward_sum, cur_episode_length
        self._ring = z(2, self.capacity)                     # ring_reward, ring_length
        self._counts = z(2, dtype=torch.int64)               # episodes pushed so far, info steps accumulated
        self._info = None                                    # (2, R) float64: last, acc; sized by the first update_info
        self.info_keys = []                                  # [(episode key, row)]

    cur_reward_sum = property(lambda self: self._cur[0])
    cur_episode_length = property(lambda self: self._cur[1])

    def _flags(self, name, x, dtypes):
        if (not torch.is_tensor(x) or x.dtype not in dtypes or x.numel() != self.num_envs or not x.is_contiguous() or x.device != self.device):
            got = f"{tuple(x.shape)} {x.dtype} on {x.device}" if torch.is_tensor(x) else type(x).__name__
            raise ValueError(f"EpisodeStats: {name} must hold {self.num_envs} contiguous elements of {' / '.join(str(d) for d in dtypes)} on "
                             f"{self.device}, got {got}")
        return x.data_ptr()

    def update(self, rewards, dones):
        """on_policy_runner.py:130-136 for one env step.  rewards: N contiguous float32; dones: N contiguous bool / uint8; nothing is
        converted (a conversion is a hidden launch)."""
        rew = self._flags("rewards", rewards, (torch.float32,))
        done = self._flags("dones", dones, (torch.bool, torch.uint8))
        _call(self.device, "lg_runner_episode_stats", self.num_envs, rew, done, self._cur[0].data_ptr(), self._cur[1].data_ptr(),
              self._ring[0].data_ptr(), self._ring[1].data_ptr(), self.capacity, self._counts[0:].data_ptr())

    def update_info(self, env):
        """One step of the episode-info log from the env's reset snapshot (`episode_info_source`)."""
        self.update_info_from(**episode_info_source(env))

    def update_info_from(self, sums_a, done_step, step, inv_episode_length_s, keys=None, sums_b=None):
        rows_a, rows_b = int(sums_a.shape[0]), (0 if sums_b is None else int(sums_b.shape[0]))
        for name, t, dt in (("sums_a", sums_a, torch.float32), ("sums_b", sums_b, torch.float32), ("done_step", done_step, torch.int32)):
            if t is None:
                continue
            n = t.shape[-1] if t.dim() else 0
            if t.dtype != dt or t.device != self.device or n != self.num_envs or t.stride(-1) != 1 or t.dim() != (1 if name == "done_step" else 2):
                raise ValueError(f"EpisodeStats: {name} must be {'(N,)' if name == 'done_step' else '(rows, N)'} {dt} with unit inner stride on "
                                 f"{self.device}, N = {self.num_envs}; got {tuple(t.shape)} {t.dtype} strides {t.stride()} on {t.device}")
        if self._info is None:
            with torch.inference_mode(False):                # the runner's rollout runs under inference_mode; the state outlives it
                self._info = torch.zeros(2, rows_a + rows_b, dtype=torch.float64, device=self.device)
            self.info_keys = list(keys) if keys is not None else [(f"row_{r}", r) for r in range(rows_a + rows_b)]
        elif self._info.shape[1] != rows_a + rows_b:
            raise ValueError(f"EpisodeStats: {rows_a + rows_b} rows, the state was sized for {self._info.shape[1]}")
        stride = lambda t: int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), self.num_envs)
        _call(self.device, "lg_runner_episode_info", self.num_envs, rows_a, sums_a.data_ptr(), stride(sums_a), rows_b,
              0 if sums_b is None else sums_b.data_ptr(), 0 if sums_b is None else stride(sums_b), done_step.data_ptr(), int(step),
              float(inv_episode_length_s), self._info[0].data_ptr(), self._info[1].data_ptr(), self._counts[1:].data_ptr())

    # ---- the one read-back -----------------------------------------------------------------------------------------------------------
    def pack(self):
        """The logged state as one float64 device vector (float32 and the counts convert exactly): what `unpack` takes once it is on the
        host.  A caller with more to read (the runner's log) appends to it and copies once."""
        parts = [self._counts.double(), self._ring.double().reshape(-1)]
        if self._info is not None:
            parts.append(self._info.reshape(-1))
        return torch.cat(parts)

    def unpack(self, host):
        """dict(rewbuffer, lenbuffer: the deque contents oldest first as Python floats; episode: {key: mean over the steps since the last
        clear}; count) from `pack()` on the host."""
        v = host.tolist()
        count, n_acc, cap = int(v[0]), int(v[1]), self.capacity
        ring = v[2:2 + 2 * cap]
        live, first = min(count, cap), (count % cap if count >= cap else 0)
        order = [(first + k) % cap for k in range(live)]
        out = dict(rewbuffer=[ring[i] for i in order], lenbuffer=[ring[cap + i] for i in order], count=count, episode={})
        if self._info is not None and n_acc > 0:
            acc = v[2 + 2 * cap + self._info.shape[1]:]
            out["episode"] = {key: acc[row] / n_acc for key, row in self.info_keys}
        return out

    def clear_info(self):
        """`ep_infos.clear()`: the means start over; the last value stays, as the env's dict does."""
        if self._info is not None:
            self._info[1].zero_()
        self._counts[1:].zero_()

    def read(self, clear=True):
        out = self.unpack(self.pack().cpu())
        if clear:
            self.clear_info()
        return out

    def state_dict(self):
        return dict(num_envs=self.num_envs, capacity=self.capacity, cur=self._cur.clone(), ring=self._ring.clone(), counts=self._counts.clone(),
                    info=None if self._info is None else self._info.clone(), info_keys=[list(k) for k in self.info_keys])

    def load_state_dict(self, sd):
        if int(sd["num_envs"]) != self.num_envs or int(sd["capacity"]) != self.capacity:
            raise ValueError(f"EpisodeStats: the state is of {sd['num_envs']} envs and capacity {sd['capacity']}, this object of "
                             f"{self.num_envs} and {self.capacity}")
        self._cur.copy_(sd["cur"])
        self._ring.copy_(sd["ring"])
        self._counts.copy_(sd["counts"])
        self.info_keys = [(k, int(r)) for k, r in sd["info_keys"]]
        if sd["info"] is None:
            self._info = None
        elif self._info is not None and self._info.shape == sd["info"].shape:
            self._info.copy_(sd["info"])
        else:
            self._info = sd["info"].to(self.device, torch.float64).clone()


# ---- the learner --------------------------------------------------------------------------------------------------------------------
class PPO:
    """rsl_rl/algorithms/ppo.py:39-148 for the plain ActorCritic.  `device=None`: where the module lives."""

    def __init__(self, actor_critic, num_learning_epochs=1, num_mini_batches=1, clip_param=0.2, gamma=0.998, lam=0.95, value_loss_coef=1.0,
                 entropy_coef=0.0, learning_rate=1e-3, max_grad_norm=1.0, use_clipped_value_loss=True, schedule="fixed", desired_kl=0.01,
                 use_spo=False, device=None, seed=0):
        _refuse_families(actor_critic, "PPO")
        if schedule not in ("fixed", "adaptive"):
            raise ValueError(f"PPO: schedule = {schedule!r}; expected 'fixed' or 'adaptive'")
        self.device = _hip_device(device if device is not None else actor_critic.std.device, "PPO")
        self.actor_critic = actor_critic
        self.actor_critic.to(self.device)
        self.desired_kl, self.schedule, self.use_spo = desired_kl, schedule, use_spo
        self.clip_param, self.num_learning_epochs, self.num_mini_batches = clip_param, num_learning_epochs, num_mini_batches
        self.value_loss_coef, self.entropy_coef, self.gamma, self.lam = value_loss_coef, entropy_coef, gamma, lam
        self.max_grad_norm, self.use_clipped_value_loss = max_grad_norm, use_clipped_value_loss
        self.storage = None                                  # init_storage
        self.policy = FusedPolicy(actor_critic, seed=seed, device=self.device)
        self.train_pass = FusedTrainPass(actor_critic)
        self.loss_fn = FusedPPOLoss(clip_param, value_loss_coef, entropy_coef, use_clipped_value_loss, use_spo)
        adaptive = schedule == "adaptive" and desired_kl is not None
        self.optimizer = FusedAdam(actor_critic.parameters(), lr=learning_rate, max_grad_norm=max_grad_norm,
                                   desired_kl=desired_kl if adaptive else None)
        self._adaptive = adaptive
        self._obs = self._critic_obs = None

    @property
    def learning_rate(self):
        """The rate in the optimizer's device cell.  Synchronises: for the log."""
        return self.optimizer.lr

    def init_storage(self, num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, action_shape, env=None):
        """`env`: an env built with cfg.hip.obs_sets = num_transitions_per_env + 1 lends the storage its observation rows (zero-copy)."""
        self.storage = RolloutStorage(num_envs, num_transitions_per_env, actor_obs_shape, critic_obs_shape, action_shape, self.device, env=env)

    def test_mode(self):
        self.actor_critic.eval()

    def train_mode(self):
        self.actor_critic.train()

    def act(self, obs, critic_obs, noise=None):
        """ppo.py:93-105 in one launch, written straight into storage row `storage.step`; returns that row's actions.  `noise` ((N, A)
        float32) replaces the Philox draw: action = mean + std * noise."""
        self._obs, self._critic_obs = obs, critic_obs
        return self.policy.act(obs, critic_obs, storage=self.storage, noise=noise)

    def process_env_step(self, rewards, dones, infos):
        """ppo.py:107-117 in one record launch: the time-out bootstrap, reward, done and the observation rows of the step."""
        self.storage.add_step(rewards, dones, infos.get("time_outs"), self.gamma, observations=self._obs, critic_observations=self._critic_obs)
        self._obs = self._critic_obs = None

    def compute_returns(self, last_critic_obs):
        self.storage.compute_returns(self.policy.evaluate(last_critic_obs), self.gamma, self.lam)

    def update(self):
        """ppo.py:124-148.  The two means are accumulated on the device and read once, behind the loop."""
        sums = torch.zeros(2, device=self.device)
        for obs_batch, critic_obs_batch, actions_batch, target_values_batch, advantages_batch, returns_batch, old_actions_log_prob_batch, \
                old_mu_batch, old_sigma_batch, _hid, _masks in self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs):
            mu, sigma, values = self.train_pass(obs_batch, critic_obs_batch)
            out = self.loss_fn(mu, sigma, values, actions_batch, old_actions_log_prob_batch, advantages_batch, returns_batch, target_values_batch,
                               old_mu_batch, old_sigma_batch)
            self.optimizer.zero_grad()
            out.loss.backward()
            self.optimizer.step(kl_mean=out.kl_mean if self._adaptive else None)
            sums[0] += out.value_loss
            sums[1] += out.surrogate_loss
        num_updates = self.num_learning_epochs * self.num_mini_batches
        mean_value_loss, mean_surrogate_loss = (x / num_updates for x in sums.tolist())
        self.storage.clear()
        return mean_value_loss, mean_surrogate_loss


# ---- the runner ---------------------------------------------------------------------------------------------------------------------
def _default_writer(log_dir):
    try:
        from torch.utils.tensorboard import SummaryWriter
    except Exception as e:      # noqa: BLE001 -- tensorboard is optional; without it the caller brings the writer
        raise ValueError("OnPolicyRunner: log_dir is set, torch.utils.tensorboard cannot be imported "
                         f"({type(e).__name__}) and no writer was given: pass writer= (any object with add_scalar(tag, value, step))") from e
    return SummaryWriter(log_dir=log_dir, flush_secs=10)


class OnPolicyRunner:
    """rsl_rl/runners/on_policy_runner.py:46-260 for `policy_class_name = "ActorCritic"`, `algorithm_class_name = "PPO"`.

    `actor_critic=None` builds `rsl_rl.modules.ActorCritic(num_obs, num_critic_obs, num_actions, **train_cfg["policy"])` where that package
    can be imported; otherwise the caller passes the module.  `writer=None` with a `log_dir` takes torch.utils.tensorboard's SummaryWriter.
    Logging is on with a `log_dir` or a `writer`; checkpoints are written with a `log_dir` only.  `noise_source`, if set, is called as
    `noise_source(iteration, step)` and its (N, A) tensor is the draw of that step's `act` (tests replay recorded draws through it)."""

    def __init__(self, env, train_cfg, log_dir=None, device=None, actor_critic=None, writer=None):
        self.cfg, self.alg_cfg, self.policy_cfg, self.all_cfg = train_cfg["runner"], train_cfg["algorithm"], train_cfg["policy"], train_cfg
        for key, known, what in (("policy_class_name", _POLICY_CLASSES, "policy"), ("algorithm_class_name", _ALGORITHM_CLASSES, "algorithm")):
            name = self.cfg.get(key, known[0])
            if name not in known:
                raise ValueError(f"OnPolicyRunner: {key} = {name!r}; only {' / '.join(known)} is built, the other {what} classes keep the "
                                 "reference's runner")
        if actor_critic is not None:
            _refuse_families(actor_critic, "OnPolicyRunner")
        self.log_dir = log_dir
        self.writer = writer if writer is not None else (_default_writer(log_dir) if log_dir is not None else None)
        self.env = env
        num_critic_obs = env.num_privileged_obs if env.num_privileged_obs is not None else env.num_obs
        if actor_critic is None:
            try:
                from rsl_rl.modules import ActorCritic
            except Exception as e:      # noqa: BLE001
                raise ValueError(f"OnPolicyRunner: rsl_rl.modules cannot be imported ({type(e).__name__}): pass actor_critic=") from e
            actor_critic = ActorCritic(env.num_obs, num_critic_obs, env.num_actions, **self.policy_cfg)
            if device is None:
                actor_critic.to(env.device)
        self.device = _hip_device(device if device is not None else actor_critic.std.device, "OnPolicyRunner")
        self.alg = PPO(actor_critic, device=self.device, **self.alg_cfg)
        self.num_steps_per_env, self.save_interval = int(self.cfg["num_steps_per_env"]), int(self.cfg["save_interval"])
        self.env.reset()                                     # before the storage: lent observation rows start at the env's current copy
        engine = getattr(env, "_engine", None)
        lend = engine is not None and int(engine.task.obs_sets) == self.num_steps_per_env + 1
        self.alg.init_storage(env.num_envs, self.num_steps_per_env, [env.num_obs], [env.num_privileged_obs], [env.num_actions],
                              env=env if lend else None)
        self.stats = EpisodeStats(env.num_envs, 100, self.device)
        self.noise_source = None
        self.verbose = True
        self.tot_timesteps, self.tot_time, self.current_learning_iteration = 0, 0, 0
        self.rewbuffer, self.lenbuffer = [], []              # the deques' contents as of the last log

    @property
    def logging(self):
        return self.writer is not None

    def learn(self, num_learning_iterations, init_at_random_ep_len=False):
        env, alg, T = self.env, self.alg, self.num_steps_per_env
        if init_at_random_ep_len:
            env.episode_length_buf = torch.randint_like(env.episode_length_buf, high=int(env.max_episode_length))
        alg.actor_critic.train()
        alg.storage.clear()                                  # row 0 is the env's current observation, whatever stepped the env since
        tot_iter = self.current_learning_iteration + num_learning_iterations
        for it in range(self.current_learning_iteration, tot_iter):
            start = time.time()
            with torch.inference_mode():
                obs = env.get_observations()                 # read again every iteration: a storage with lent rows re-bases the env's cycle
                privileged_obs = env.get_privileged_observations()
                critic_obs = privileged_obs if privileged_obs is not None else obs
                for i in range(T):
                    actions = alg.act(obs, critic_obs, noise=None if self.noise_source is None else self.noise_source(it, i))
                    obs, privileged_obs, rewards, dones, infos = env.step(actions)
                    critic_obs = privileged_obs if privileged_obs is not None else obs
                    alg.process_env_step(rewards, dones, infos)
                    if self.logging:
                        self.stats.update(rewards, dones)
                        self.stats.update_info(env)
                stop = time.time()
                collection_time = stop - start
                start = stop
                alg.compute_returns(critic_obs)
            mean_value_loss, mean_surrogate_loss = alg.update()
            stop = time.time()
            learn_time = stop - start
            if self.logging:
                self.log(dict(it=it, collection_time=collection_time, learn_time=learn_time, mean_value_loss=mean_value_loss,
                              mean_surrogate_loss=mean_surrogate_loss, num_learning_iterations=num_learning_iterations, infos=infos))
            if self.log_dir is not None and it % self.save_interval == 0:
                self.save(os.path.join(self.log_dir, f"model_{it}.pt"))
        self.current_learning_iteration += num_learning_iterations
        if self.log_dir is not None:
            self.save(os.path.join(self.log_dir, f"model_{self.current_learning_iteration}.pt"))

    def log(self, locs, width=80, pad=35):
        """on_policy_runner.py:171-238 from one copy to the host: the stats' state, the learning rate cell, the mean noise std and the
        episode entries that are no reward sums (terrain_level, max_command_x, a task's lazy entries: their value at log time, not the
        reference's mean over the steps)."""
        self.tot_timesteps += self.num_steps_per_env * self.env.num_envs
        iteration_time = locs["collection_time"] + locs["learn_time"]
        self.tot_time += iteration_time
        it = locs["it"]
        summed = {k for k, _ in self.stats.info_keys}
        late, host_vals = [], {}
        episode = (locs.get("infos") or {}).get("episode")
        if episode is not None:
            for key in episode:
                if key in summed:
                    continue
                v = episode[key]
                if torch.is_tensor(v) and v.device.type == "cuda":
                    late.append((key, v.detach().double().reshape(-1).mean().reshape(1)))
                else:
                    host_vals[key] = float(torch.as_tensor(v, dtype=torch.float64).mean())
        head = self.stats.pack()
        tail = [self.alg.optimizer._state[abi.ADAM_S_LR:abi.ADAM_S_LR + 1], self.alg.actor_critic.std.detach().double().mean().reshape(1)]
        host = torch.cat([head, *tail, *(v for _, v in late)]).cpu()
        st = self.stats.unpack(host[:head.numel()])
        self.stats.clear_info()
        rest = host[head.numel():].tolist()
        learning_rate, mean_std = rest[0], rest[1]
        host_vals.update({key: x for (key, _), x in zip(late, rest[2:])})
        self.rewbuffer, self.lenbuffer = st["rewbuffer"], st["lenbuffer"]
        w = self.writer
        ep_string = ""
        for key, value in list(st["episode"].items()) + list(host_vals.items()):
            w.add_scalar("Episode/" + key, value, it)
            ep_string += f"{f'Mean episode {key}:':>{pad}} {value:.4f}\n"
        fps = int(self.num_steps_per_env * self.env.num_envs / iteration_time)
        w.add_scalar("Loss/value_function", locs["mean_value_loss"], it)
        w.add_scalar("Loss/surrogate", locs["mean_surrogate_loss"], it)
        w.add_scalar("Loss/learning_rate", learning_rate, it)
        w.add_scalar("Policy/mean_noise_std", mean_std, it)
        w.add_scalar("Perf/total_fps", fps, it)
        w.add_scalar("Perf/collection time", locs["collection_time"], it)
        w.add_scalar("Perf/learning_time", locs["learn_time"], it)
        if len(self.rewbuffer) > 0:
            mean_reward, mean_length = statistics.mean(self.rewbuffer), statistics.mean(self.lenbuffer)
            w.add_scalar("Train/mean_reward", mean_reward, it)
            w.add_scalar("Train/mean_episode_length", mean_length, it)
            w.add_scalar("Train/mean_reward/time", mean_reward, self.tot_time)
            w.add_scalar("Train/mean_episode_length/time", mean_length, self.tot_time)
        if not self.verbose:
            return
        title = f" \033[1m Learning iteration {it}/{self.current_learning_iteration + locs['num_learning_iterations']} \033[0m "
        s = (f"{'#' * width}\n{title.center(width, ' ')}\n\n"
             f"{'Computation:':>{pad}} {fps:.0f} steps/s (collection: {locs['collection_time']:.3f}s, learning {locs['learn_time']:.3f}s)\n"
             f"{'Value function loss:':>{pad}} {locs['mean_value_loss']:.4f}\n{'Surrogate loss:':>{pad}} {locs['mean_surrogate_loss']:.4f}\n"
             f"{'Mean action noise std:':>{pad}} {mean_std:.2f}\n")
        if len(self.rewbuffer) > 0:
            s += f"{'Mean reward:':>{pad}} {mean_reward:.2f}\n{'Mean episode length:':>{pad}} {mean_length:.2f}\n"
        s += ep_string + (f"{'-' * width}\n{'Total timesteps:':>{pad}} {self.tot_timesteps}\n{'Iteration time:':>{pad}} {iteration_time:.2f}s\n"
                          f"{'Total time:':>{pad}} {self.tot_time:.2f}s\n")
        print(s)

    def save(self, path, infos=None):
        torch.save({"model_state_dict": self.alg.actor_critic.state_dict(), "optimizer_state_dict": self.alg.optimizer.state_dict(),
                    "iter": self.current_learning_iteration, "infos": infos}, path)

    def load(self, path, load_optimizer=True):
        loaded = torch.load(path, map_location=self.device)
        self.alg.actor_critic.load_state_dict(loaded["model_state_dict"])
        if load_optimizer:
            self.alg.optimizer.load_state_dict(loaded["optimizer_state_dict"])
        self.current_learning_iteration = loaded["iter"]
        return loaded["infos"]

    def get_inference_policy(self, device=None):
        """The clipped mean as one launch (`FusedPolicy.act_inference`); the module stays on its HIP device."""
        self.alg.actor_critic.eval()
        if device is not None:
            _hip_device(device, "OnPolicyRunner.get_inference_policy")
        return self.alg.policy.act_inference

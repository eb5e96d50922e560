"""Golden vectors for the fused training loop (hcr_genesis_lr_cl_amd/runner.py) from the reference's own OnPolicyRunner.learn()
(rsl_rl/runners/on_policy_runner.py:100-155) around its PPO (rsl_rl/algorithms/ppo.py) on the CPU: a scripted VecEnv whose observations,
rewards, dones, time_outs and infos['episode'] values come from a seeded generator and ignore the actions, a tiny ActorCritic (actor
7 -> 16 -> 8 -> 3, critic 9 -> 16 -> 8 -> 1), three iterations of 8 steps on 16 envs, 2 epochs x 2 mini-batches, schedule="adaptive".
The done probability is high enough that more than 100 episodes finish, so deque(maxlen=100) wraps.  The run is made twice on the same
inputs: in float64 (torch.set_default_dtype) and as a float32 twin.  The book-keeping (cur_reward_sum, cur_episode_length, rewbuffer,
lenbuffer) is float32 in both, as the reference fixes dtype=torch.float there, and is asserted bit-identical between the two.

Build-container only:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_runner_fixtures.py
Output: tests/golden/runner_learn.npz:
  cfg                       [num_envs, steps per env, iterations, epochs, mini-batches, lr0, desired_kl, gamma, lam, clip, entropy_coef,
                             max_grad_norm, value_loss_coef, episode_length_s, deque capacity]
  obs, priv                 (S + 1, N, 7) / (S + 1, N, 9) float32: what the env offers before step s (row S: after the last step)
  rew, dones, time_outs     (S, N) float32 / bool / bool: what step s returns;  ep_sums (S, R, N) float32: the episode sums a reset at step s
                            snapshots;  ep_keys: the R keys of infos['episode'];  infos['episode'][key] is, at a step with dones,
                            mean(ep_sums[s, r][done envs]) / episode_length_s in float32, otherwise the previous step's dict (zeros at first)
  noise                     (S, N, 3) float32: the Gaussian draw of every act: actions = mean + std * noise (Normal.sample is replaced by that
                            line around a seeded draw, in both runs; asserted equal to (actions - mean) / std of the float64 run)
  perm                      (iterations, T * N) int64: the torch.randperm result of every update (drawn in the float64 run, replayed in the twin)
  names, shapes, init       the parameters in actor_critic.parameters() order; init float32 (both runs start from it)
  per iteration, float64 run and twin (suffix 32):  returns, advantages (iterations, T, N);  losses (iterations, 2): mean value loss, mean
                            surrogate loss;  lr (iterations,): the rate after the update;  params (iterations, P);  kl (iterations, steps)
  rewbuffer, lenbuffer      (iterations, 100) float32 with buffer_len (iterations,): the deques' contents oldest first at every log
  scalar_tags               every tag the writer saw in iteration 0 in order (later iterations write the same);  scalar_names / scalar_values
                            (iterations, n) and scalar_values32: the values of the tags that do not depend on the wall clock
The generator asserts that the twin takes the float64 run's learning-rate decisions, that the rate rises, falls and stays somewhere, and
that no KL lies within 1 % of a threshold of the rule.  Written through ref_harness.save; `python tests/golden/check_fixtures.py` checks
that the output still equals the committed file."""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

rh.load_reference()
import torch  # noqa: E402

N, T, ITERS, EPOCHS, MINI_BATCHES = 16, 8, 3, 2, 2
N_OBS, N_PRIV, A, R = 7, 9, 3, 3
LR0, DESIRED_KL, GAMMA, LAM, CLIP, ENTROPY, MAX_GRAD_NORM, VALUE_COEF = 1e-3, 4e-4, 0.99, 0.95, 0.2, 0.01, 1.0, 1.0
EPISODE_LENGTH_S, CAP, P_DONE = 20.0, 100, 0.4
EP_KEYS = ("rew_tracking_lin_vel", "rew_torques", "rew_action_rate")
S = T * ITERS
WALL_CLOCK = ("Perf/", "/time")


def script(seed):
    rng = np.random.default_rng(seed)
    f = np.float32
    dones = rng.random((S, N)) < P_DONE
    dones[1] = False                                      # a step with no reset: the previous episode dict stays
    dones[2] = True                                       # a step where every env resets
    return dict(obs=rng.normal(size=(S + 1, N, N_OBS)).astype(f), priv=rng.normal(size=(S + 1, N, N_PRIV)).astype(f),
                rew=(0.5 * rng.normal(size=(S, N)) + 0.2).astype(f), dones=dones, time_outs=dones & (rng.random((S, N)) < 0.3),
                ep_sums=(3.0 * rng.normal(size=(S, R, N))).astype(f), noise=rng.normal(size=(S, N, A)).astype(f))


class ScriptedEnv:
    """The VecEnv surface the reference's runner reads (rsl_rl/env/vec_env.py); every output is a row of the script in the default dtype."""

    def __init__(self, sc):
        self.sc, self.s = sc, 0
        self.num_envs, self.num_obs, self.num_privileged_obs, self.num_actions = N, N_OBS, N_PRIV, A
        self.max_episode_length, self.device = 1000, "cpu"
        self.episode_length_buf = torch.zeros(N, dtype=torch.long)
        self.episode = {k: torch.zeros((), dtype=torch.float32) for k in EP_KEYS}

    def _t(self, x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(torch.get_default_dtype())

    def get_observations(self):
        return self._t(self.sc["obs"][self.s])

    def get_privileged_observations(self):
        return self._t(self.sc["priv"][self.s])

    def reset(self):
        return self.get_observations(), self.get_privileged_observations()

    def step(self, actions):
        s, sc = self.s, self.sc
        dones = torch.from_numpy(sc["dones"][s].copy())
        ids = dones.nonzero(as_tuple=False).flatten()
        if len(ids) > 0:                                  # legged_robot.py:128-138: a fresh dict per reset, float32
            self.episode = {k: torch.mean(torch.from_numpy(sc["ep_sums"][s, r].copy())[ids]) / EPISODE_LENGTH_S for r, k in enumerate(EP_KEYS)}
        self.s += 1
        infos = {"episode": self.episode, "time_outs": torch.from_numpy(sc["time_outs"][s].copy())}
        return self.get_observations(), self.get_privileged_observations(), self._t(sc["rew"][s]), dones, infos


class Recorder:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), step))


def run(dtype, sc, init, perms):
    """One learn() of three iterations in `dtype`.  perms: None (draw and record) or the recorded permutations (replay)."""
    from rsl_rl.modules import actor_critic as ac_module
    from rsl_rl.runners import OnPolicyRunner
    torch.set_default_dtype(dtype)
    torch.manual_seed(7)
    cfg = dict(runner=dict(policy_class_name="ActorCritic", algorithm_class_name="PPO", num_steps_per_env=T, save_interval=1000,
                           experiment_name="runner_fixture", run_name="", max_iterations=ITERS),
               algorithm=dict(num_learning_epochs=EPOCHS, num_mini_batches=MINI_BATCHES, clip_param=CLIP, gamma=GAMMA, lam=LAM,
                              value_loss_coef=VALUE_COEF, entropy_coef=ENTROPY, learning_rate=LR0, max_grad_norm=MAX_GRAD_NORM,
                              use_clipped_value_loss=True, schedule="adaptive", desired_kl=DESIRED_KL),
               policy=dict(actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8], activation="elu", init_noise_std=1.0))
    env = ScriptedEnv(sc)
    rec = dict(returns=[], advantages=[], losses=[], lr=[], params=[], kl=[], rewbuffer=[], lenbuffer=[], perm=[], drawn=[], scalars=[])
    n64 = lambda x: x.detach().numpy().astype(np.float64).copy()
    flat = lambda xs: np.concatenate([n64(x).reshape(-1) for x in xs])
    draws = iter(range(S))
    sample0, randperm0 = ac_module.Normal.sample, torch.randperm

    def sample(self, sample_shape=torch.Size()):
        if not torch.is_inference_mode_enabled():          # PPO.update calls act() for the distribution alone and drops the sample
            return self.mean.detach()
        z = torch.from_numpy(sc["noise"][next(draws)].copy()).to(self.mean.dtype)
        a = self.mean + self.stddev * z
        rec["drawn"].append(n64((a - self.mean) / self.stddev))
        return a

    def randperm(n, *a, **k):
        p = randperm0(n, *a, **k) if perms is None else torch.from_numpy(perms[len(rec["perm"])].copy())
        assert p.numel() == T * N
        rec["perm"].append(p.numpy().astype(np.int64).copy())
        return p

    with tempfile.TemporaryDirectory() as log_dir, contextlib.redirect_stdout(io.StringIO()):
        runner = OnPolicyRunner(env, cfg, log_dir=log_dir, device="cpu")
        ac, alg = runner.alg.actor_critic, runner.alg
        with torch.no_grad():
            for p, v in zip(ac.parameters(), init(ac)):
                p.copy_(torch.from_numpy(v).to(dtype))
        runner.writer = Recorder()                        # before learn(): the stubbed SummaryWriter is never constructed
        update0, adjust0, log0 = alg.update, alg._adjust_learning_rate, runner.log

        def adjust(sigma, old_sigma, mu, old_mu):
            with torch.no_grad():
                rec["kl"].append(float(torch.sum(torch.log(sigma / old_sigma + 1.e-5) + (old_sigma ** 2 + (old_mu - mu) ** 2) / (2.0 * sigma ** 2)
                                                 - 0.5, dim=-1).mean()))
            return adjust0(sigma, old_sigma, mu, old_mu)

        def update():
            rec["returns"].append(n64(alg.storage.returns)[..., 0])
            rec["advantages"].append(n64(alg.storage.advantages)[..., 0])
            out = update0()
            rec["losses"].append([float(out[0]), float(out[1])])
            rec["lr"].append(float(alg.learning_rate))
            rec["params"].append(flat(ac.parameters()))
            return out

        def log(locs, *a, **k):
            rec["rewbuffer"].append(list(locs["rewbuffer"]))
            rec["lenbuffer"].append(list(locs["lenbuffer"]))
            n0 = len(runner.writer.rows)
            out = log0(locs, *a, **k)
            rec["scalars"].append(runner.writer.rows[n0:])
            return out

        alg.update, alg._adjust_learning_rate, runner.log = update, adjust, log
        ac_module.Normal.sample, torch.randperm = sample, randperm
        try:
            runner.learn(ITERS)
        finally:
            ac_module.Normal.sample, torch.randperm = sample0, randperm0
    rec["names"] = [n for n, _ in ac.named_parameters()]
    rec["shapes"] = [(list(p.shape) + [0, 0])[:2] for p in ac.parameters()]
    assert len(rec["perm"]) == ITERS and len(rec["kl"]) == ITERS * EPOCHS * MINI_BATCHES and len(rec["drawn"]) == S
    return rec


def main(seed=61):
    torch.set_num_threads(1)
    sc = script(seed)
    first = {}

    def init(ac):                                         # both runs start from the float32 run's own initialisation
        if not first:
            first["init"] = [p.detach().numpy().astype(np.float32).copy() for p in ac.parameters()]
        return first["init"]
    torch.set_default_dtype(torch.float32)
    torch.manual_seed(seed)
    from rsl_rl.modules import ActorCritic
    with contextlib.redirect_stdout(io.StringIO()):
        init(ActorCritic(N_OBS, N_PRIV, A, actor_hidden_dims=[16, 8], critic_hidden_dims=[16, 8]))
    r64 = run(torch.float64, sc, init, None)
    r32 = run(torch.float32, sc, init, r64["perm"])
    torch.set_default_dtype(torch.float32)

    steps = EPOCHS * MINI_BATCHES
    # the rule's decisions: the same in both runs, all three kinds present, no KL near a threshold
    def moves(r):
        lrs, out, lr = [], [], LR0
        for k in r["kl"]:
            new = max(1e-5, lr / 1.5) if k > 2 * DESIRED_KL else min(1e-2, lr * 1.5) if (k < DESIRED_KL / 2 and k > 0) else lr
            out.append(int(np.sign(new - lr)))
            lr = new
            lrs.append(lr)
        assert all(abs(lrs[(i + 1) * steps - 1] / r["lr"][i] - 1) < 1e-12 for i in range(ITERS)), (lrs, r["lr"])
        return out
    m64, m32 = moves(r64), moves(r32)
    assert m64 == m32, (m64, m32)
    assert 1 in m64 and -1 in m64 and 0 in m64, (m64, r64["kl"])
    for r in (r64, r32):
        assert all(abs(k / (2 * DESIRED_KL) - 1) > 0.01 and abs(k / (DESIRED_KL / 2) - 1) > 0.01 and k > 0 for k in r["kl"]), r["kl"]
    # the draws are what the reference's own actions carry, and the book-keeping is float32 in both runs
    assert np.abs(np.stack(r64["drawn"]) - sc["noise"]).max() < 1e-12
    assert r64["rewbuffer"] == r32["rewbuffer"] and r64["lenbuffer"] == r32["lenbuffer"]
    n_eps = int(sc["dones"].sum())
    assert n_eps > CAP and len(r64["rewbuffer"][-1]) == CAP and len(r64["rewbuffer"][0]) < CAP, (n_eps, [len(b) for b in r64["rewbuffer"]])
    assert all(np.float32(x) == x for b in r64["rewbuffer"] + r64["lenbuffer"] for x in b)

    tags = [t for t, _, _ in r64["scalars"][0]]
    assert all([t for t, _, _ in s] == tags for r in (r64, r32) for s in r["scalars"]), "the tags differ between iterations"
    names = [t for t in tags if not any(w in t for w in WALL_CLOCK)]
    values = lambda r: np.array([[dict((t, v) for t, v, _ in s)[n] for n in names] for s in r["scalars"]], np.float64)
    pad = lambda bufs: np.array([list(b) + [0.0] * (CAP - len(b)) for b in bufs], np.float32)

    arrays = {"cfg": np.array([N, T, ITERS, EPOCHS, MINI_BATCHES, LR0, DESIRED_KL, GAMMA, LAM, CLIP, ENTROPY, MAX_GRAD_NORM, VALUE_COEF,
                               EPISODE_LENGTH_S, CAP], np.float64)}
    for k in ("obs", "priv", "rew", "dones", "time_outs", "ep_sums", "noise"):
        arrays[k] = sc[k]
    arrays["ep_keys"] = np.array(EP_KEYS)
    arrays["perm"] = np.stack(r64["perm"])
    arrays["names"], arrays["shapes"] = np.array(r64["names"]), np.array(r64["shapes"], np.int64)
    arrays["init"] = np.concatenate([v.reshape(-1) for v in first["init"]])
    for suffix, r in (("", r64), ("32", r32)):
        arrays["returns" + suffix], arrays["advantages" + suffix] = np.stack(r["returns"]), np.stack(r["advantages"])
        arrays["losses" + suffix], arrays["lr" + suffix] = np.array(r["losses"], np.float64), np.array(r["lr"], np.float64)
        arrays["params" + suffix] = np.stack(r["params"])
        arrays["kl" + suffix] = np.array(r["kl"], np.float64).reshape(ITERS, steps)
    arrays["rewbuffer"], arrays["lenbuffer"] = pad(r64["rewbuffer"]), pad(r64["lenbuffer"])
    arrays["buffer_len"] = np.array([len(b) for b in r64["rewbuffer"]], np.int64)
    arrays["scalar_tags"], arrays["scalar_names"] = np.array(tags), np.array(names)
    arrays["scalar_values"], arrays["scalar_values32"] = values(r64), values(r32)
    rh.save("runner_learn", arrays, "episodes", n_eps, "moves", m64, "kl", [f"{k:.2e}" for k in r64["kl"]], "lr", [f"{x:.3e}" for x in r64["lr"]])


if __name__ == "__main__":
    main()

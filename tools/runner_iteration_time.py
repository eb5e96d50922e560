"""Developer tool (GPU only, never read by bench.py): what the runner's per-step book-keeping costs on go2, 4096 envs x 24 steps, with
the policy nets of the config (actor and critic num_observations -> 512 -> 256 -> 128 -> num_actions / 1).  The rollout half of one
iteration -- per step `PPO.act`, `env.step`, `PPO.process_env_step` and the book-keeping -- three ways:

  (i)   off:    no book-keeping (the reference's `log_dir is None`);
  (ii)  stats:  `EpisodeStats.update` + `update_info` (csrc/lg_runner.hip: two launches, nothing read back);
  (iii) torch:  the reference's seven statements (rsl_rl/runners/on_policy_runner.py:128-136) as torch ops on the same tensors:
                ep_infos.append, two in-place adds, (dones > 0).nonzero(), two .cpu().numpy().tolist() into deque(maxlen=100), two zeroings;

and (iv) whole: one whole `OnPolicyRunner.learn(1)` with logging on (rollout, returns, 5 epochs x 4 mini-batches, the log's read-back).

Method: a fresh child process per side and round (the parent never opens the device), the sides alternating within every round.  A child
of (ii) or (iii) first runs --warmup rollouts with BOTH book-keepings side by side and refuses to time anything if the ring contents
(rewbuffer, lenbuffer) or the running sums differ in a bit; then it takes --repeats samples of its side alone.  A sample is the host
wall-clock time of one rollout (24 steps) from a synchronised device to a synchronised device: the quantity of interest is host stalls,
which device events do not see.  Episode lengths start at random so that episodes end within the first rollouts.  Median and p10-p90 over
all samples of a side are printed.

    python tools/runner_iteration_time.py [--rounds 3] [--repeats 10] [--envs 4096] [--steps 24] [--sides off,stats,torch,whole]

Prints a table and one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from collections import deque

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
SIDES = ("off", "stats", "torch", "whole")
ALGORITHM = dict(num_learning_epochs=5, num_mini_batches=4, clip_param=0.2, gamma=0.99, lam=0.95, value_loss_coef=1.0, entropy_coef=0.01,
                 learning_rate=1e-3, max_grad_norm=1.0, use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.01)


class Recorder:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), step))


def actor_critic(n_obs, n_critic_obs, n_actions, hidden):
    """rsl_rl.modules.ActorCritic's members as a plain module (that package is not needed to time the loop)."""
    import torch
    nn = torch.nn

    def mlp(i, o, tail=None):
        layers, d = [], i
        for h in hidden:
            layers += [nn.Linear(d, h), nn.ELU()]
            d = h
        return nn.Sequential(*layers, nn.Linear(d, o), *([tail] if tail is not None else []))

    class ActorCritic(nn.Module):
        is_recurrent = False

        def __init__(self):
            super().__init__()
            self.std = nn.Parameter(torch.ones(n_actions))
            self.actor, self.critic = mlp(n_obs, n_actions, nn.Hardtanh(-100.0, 100.0)), mlp(n_critic_obs, 1)
    return ActorCritic()


class TorchBook:
    """on_policy_runner.py:108-112, 128-136, statement for statement."""

    def __init__(self, n, dev):
        import torch
        self.ep_infos, self.rewbuffer, self.lenbuffer = [], deque(maxlen=100), deque(maxlen=100)
        self.cur_reward_sum = torch.zeros(n, dtype=torch.float, device=dev)
        self.cur_episode_length = torch.zeros(n, dtype=torch.float, device=dev)

    def step(self, rewards, dones, infos):
        if 'episode' in infos:
            self.ep_infos.append(infos['episode'])
        self.cur_reward_sum += rewards
        self.cur_episode_length += 1
        new_ids = (dones > 0).nonzero(as_tuple=False)
        self.rewbuffer.extend(self.cur_reward_sum[new_ids][:, 0].cpu().numpy().tolist())
        self.lenbuffer.extend(self.cur_episode_length[new_ids][:, 0].cpu().numpy().tolist())
        self.cur_reward_sum[new_ids] = 0
        self.cur_episode_length[new_ids] = 0


def child(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("runner_iteration_time.py: no GPU -- a time is only measured on the device")
    from hcr_genesis_lr_cl_amd.envs import TASKS, set_seed
    from hcr_genesis_lr_cl_amd.runner import OnPolicyRunner
    dev, side, T = "cuda:0", args.child, args.steps
    cls, cfg_cls = TASKS["go2"]
    cfg = cfg_cls()
    cfg.env.num_envs = args.envs
    cfg.hip.obs_sets = T + 1
    set_seed(int(cfg.seed))
    env = cls(cfg, None, dev, True)
    torch.manual_seed(1)
    module = actor_critic(env.num_obs, env.num_privileged_obs or env.num_obs, env.num_actions, [int(h) for h in args.hidden.split(",")]).to(dev)
    train_cfg = dict(runner=dict(policy_class_name="ActorCritic", algorithm_class_name="PPO", num_steps_per_env=T, save_interval=10 ** 9),
                     algorithm=ALGORITHM, policy={})
    run = OnPolicyRunner(env, train_cfg, actor_critic=module, writer=Recorder())
    run.verbose = False
    alg, stats, book = run.alg, run.stats, TorchBook(env.num_envs, dev)
    env.episode_length_buf = torch.randint_like(env.episode_length_buf, high=int(env.max_episode_length))

    def rollout(books):
        with torch.inference_mode():
            alg.storage.clear()
            obs = env.get_observations()
            priv = env.get_privileged_observations()
            critic_obs = priv if priv is not None else obs
            for _ in range(T):
                actions = alg.act(obs, critic_obs)
                obs, priv, rewards, dones, infos = env.step(actions)
                critic_obs = priv if priv is not None else obs
                alg.process_env_step(rewards, dones, infos)
                if "stats" in books:
                    stats.update(rewards, dones)
                    stats.update_info(env)
                if "torch" in books:
                    book.step(rewards, dones, infos)
                    book.ep_infos.clear()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = dict(side=side, envs=env.num_envs, steps=T, zero_copy=bool(alg.storage.zero_copy), episodes=0)
    if side == "whole":
        for _ in range(args.warmup):
            run.learn(1)
        out["ms"] = [timed(lambda: run.learn(1)) for _ in range(args.repeats)]
        out["episodes"] = int(stats.read(clear=False)["count"])
    else:
        both = ("stats", "torch") if side != "off" else ()
        for _ in range(args.warmup):
            rollout(both)
        if both:
            got = stats.read()
            bits = lambda x: np.asarray(x, np.float32).view(np.uint32)
            same = (np.array_equal(bits(got["rewbuffer"]), bits(list(book.rewbuffer))) and np.array_equal(bits(got["lenbuffer"]), bits(list(book.lenbuffer)))
                    and torch.equal(stats.cur_reward_sum.view(torch.int32), book.cur_reward_sum.view(torch.int32))
                    and torch.equal(stats.cur_episode_length.view(torch.int32), book.cur_episode_length.view(torch.int32)))
            if not same or got["count"] < 100:
                sys.exit(f"runner_iteration_time.py: {side}: after {args.warmup} rollouts the two book-keepings disagree (or fewer than 100 "
                         f"episodes ended: {got['count']}) -- nothing timed")
            out["episodes"] = got["count"]
        out["ms"] = [timed(lambda: rollout((side,))) for _ in range(args.repeats)]
    print("CHILD " + json.dumps(out))


def stat(v):
    s = sorted(v)
    return dict(median=statistics.median(v), min=s[0], max=s[-1], p10=s[len(s) // 10], p90=s[(9 * len(s)) // 10], samples=len(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--hidden", default="512,256,128", help="actor_hidden_dims = critic_hidden_dims of the go2 policy")
    ap.add_argument("--sides", default=",".join(SIDES))
    ap.add_argument("--child", choices=SIDES, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    from hcr_genesis_lr_cl_amd import build as b
    want = [s for s in args.sides.split(",") if s]
    times, info = {}, {}
    for _ in range(args.rounds):
        for side in want:                                    # a fresh process per side, the sides alternating
            cmd = [sys.executable, os.path.abspath(__file__), "--child", side, "--repeats", str(args.repeats), "--warmup", str(args.warmup),
                   "--envs", str(args.envs), "--steps", str(args.steps), "--hidden", args.hidden]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = next((l for l in r.stdout.splitlines() if l.startswith("CHILD ")), None)
            if r.returncode != 0 or line is None:
                sys.exit(f"runner_iteration_time.py: the {side} process failed (exit status {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            d = json.loads(line[6:])
            times.setdefault(side, []).extend(d.pop("ms"))
            info[side] = d
    res = dict(tool="runner_iteration_time", rounds=args.rounds, repeats=args.repeats, envs=args.envs, steps=args.steps, hidden=args.hidden,
               source_hash=b.source_hash(), sides=info, ms={s: stat(v) for s, v in times.items()})
    print(f"go2, {args.envs} envs x {args.steps} steps, nets {args.hidden}: host wall-clock per rollout (whole: per learn(1) iteration)")
    for s, v in res["ms"].items():
        print(f"  {s:6s}: median {v['median']:8.3f} ms   min {v['min']:8.3f}   p10-p90 {v['p10']:8.3f} - {v['p90']:8.3f}   max {v['max']:8.3f}   "
              f"({v['samples']} samples, {info[s]['episodes']} episodes ended in the warm-up)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Developer tool (GPU only, never read by bench.py): time of one go2 mini-batch of the learner (24576 rows; actor and critic
num_observations -> 512 -> 256 -> 128 -> num_actions / 1 with ELU, Hardtanh behind the actor, std) in three cuts:

  forward   the training forward alone: mu, sigma, values with everything the backward needs kept
  fwd_bwd   zero_grad, forward, FusedPPOLoss, loss.backward()
  update    the same and FusedAdam.step(kl_mean=out.kl_mean): one whole mini-batch step of PPO.update()

on four sides:

  fused_eager   FusedTrainPass (csrc/lg_train.hip) for the networks, eager
  fused_graph   the same, each cut captured once on one stream and replayed as one HIP graph
  torch_eager   the torch module (nn.Sequential, autograd) for the networks, eager: the code before FusedTrainPass existed
  torch_graph   the same, captured and replayed as one HIP graph

The loss head and the optimizer are the fused ones on every side, so the difference between a fused and a torch side is the networks'
forward and backward alone.  The hidden sizes are the reference's go2 policy settings, which config.py does not carry (--hidden);
num_observations and num_actions are read from hcr_genesis_lr_cl_amd/config.py.

Method: a fresh child process per side and round (the parent never opens the device), the sides alternating within every round; a child
first checks that its side's outputs and parameter gradients agree with the torch module's on the same seeded weights and batch (relative
to each tensor's largest magnitude), warms up, then takes --repeats samples per cut, each the device-event time around a burst of --burst
calls divided by the burst length.  Everything runs on one side stream.  Median and p10-p90 over all samples of a side are printed.

    python tools/train_pass_time.py [--rounds 2] [--repeats 10] [--burst 5] [--rows 24576] [--sides fused_eager,...]

Prints a table and one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
SIDES = ("fused_eager", "torch_eager", "fused_graph", "torch_graph")
CUTS = ("forward", "fwd_bwd", "update")
CLIP_ACTIONS, DESIRED_KL = 100.0, 0.01


def build_module(hidden, dev, seed):
    import torch
    import torch.nn as nn
    from hcr_genesis_lr_cl_amd.config import GO2Cfg
    n_obs, A = int(GO2Cfg.env.num_observations), int(GO2Cfg.env.num_actions)

    def chain(last, clip):
        widths, mods = [n_obs, *hidden, last], []
        for i in range(len(widths) - 1):
            mods.append(nn.Linear(widths[i], widths[i + 1]))
            if i < len(widths) - 2:
                mods.append(nn.ELU())
        return nn.Sequential(*mods, *([nn.Hardtanh(-clip, clip)] if clip else []))

    class ActorCritic(nn.Module):
        def __init__(self):
            super().__init__()
            self.std = nn.Parameter(torch.ones(A))
            self.actor, self.critic = chain(A, CLIP_ACTIONS), chain(1, None)
    torch.manual_seed(seed)
    return ActorCritic().to(dev), n_obs, A


def batch(rows, n_obs, A, dev, seed):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    old_mu, old_sigma = 0.3 * r(rows, A), torch.ones(rows, A)
    actions = old_mu + old_sigma * r(rows, A)
    old_lp = (-(actions - old_mu) ** 2 / (2 * old_sigma ** 2) - old_sigma.log() - 0.9189385332046727).sum(-1, keepdim=True)
    target = r(rows, 1)
    cols = dict(obs=r(rows, n_obs), critic_obs=r(rows, n_obs), actions=actions, old_log_prob=old_lp, advantages=r(rows, 1),
                returns=target + 0.5 * r(rows, 1), target_values=target, old_mu=old_mu, old_sigma=old_sigma)
    return {k: v.to(dev) for k, v in cols.items()}


def child(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("train_pass_time.py: no GPU -- a time is only measured on the device")
    side_stream = torch.cuda.Stream()
    with torch.cuda.stream(side_stream):
        out = time_side(args, "cuda:0", side_stream)
    print("CHILD " + json.dumps(out))


def time_side(args, dev, side_stream):
    import torch
    from hcr_genesis_lr_cl_amd.optim import FusedAdam
    from hcr_genesis_lr_cl_amd.ppo_loss import FusedPPOLoss
    from hcr_genesis_lr_cl_amd.train import FusedTrainPass
    hidden, side = [int(h) for h in args.hidden.split(",")], args.child
    loss_fn = FusedPPOLoss(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01)

    def learner(fused):
        """(module, the three cuts as functions) of one side over a fresh module with the seeded weights."""
        m, n_obs, A = build_module(hidden, dev, 1)
        t = batch(args.rows, n_obs, A, dev, 2)
        tp = FusedTrainPass(m) if fused else None
        opt = FusedAdam(m.named_parameters(), lr=1e-3, max_grad_norm=1.0, desired_kl=DESIRED_KL)

        def forward():
            if fused:
                return tp(t["obs"], t["critic_obs"])
            mu = m.actor(t["obs"])
            return mu, mu * 0.0 + m.std, m.critic(t["critic_obs"])

        def fwd_bwd():
            opt.zero_grad()
            mu, sigma, values = forward()
            out = loss_fn(mu, sigma, values, t["actions"], t["old_log_prob"], t["advantages"], t["returns"], t["target_values"], t["old_mu"],
                          t["old_sigma"])
            out.loss.backward()
            return out

        def update():
            opt.step(kl_mean=fwd_bwd().kl_mean)
        return m, dict(forward=forward, fwd_bwd=fwd_bwd, update=update)

    # agreement with the torch module: outputs and gradients of one fwd_bwd on the seeded weights
    ref, ref_cuts = learner(False)
    ref_out = [x.detach().clone() for x in ref_cuts["forward"]()]
    ref_cuts["fwd_bwd"]()
    m, cuts = learner(side.startswith("fused"))
    got_out = [x.detach().clone() for x in cuts["forward"]()]
    cuts["fwd_bwd"]()
    side_stream.synchronize()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    agree = max([rel(a, b) for a, b in zip(got_out, ref_out)] + [rel(p.grad, q.grad) for p, q in zip(m.parameters(), ref.parameters())])
    if not agree <= 1e-3:
        sys.exit(f"train_pass_time.py: {side}: outputs or gradients disagree with the torch module by {agree:.3e} (relative) -- nothing timed")
    del ref, ref_cuts

    times = {}
    for cut in CUTS:
        fn = cuts[cut]
        if side.endswith("graph"):
            for _ in range(3):                                       # torch's recipe: a few eager calls on the capture stream first
                fn()
            side_stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side_stream):
                fn()
            fn = graph.replay

        def burst():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.burst):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / args.burst
        for _ in range(args.warmup):
            burst()
        times[cut] = [burst() for _ in range(args.repeats)]
    return dict(rows=args.rows, floats=sum(p.numel() for p in m.parameters()), agree=agree, us=times)


def stat(v):
    s = sorted(v)
    return dict(median=statistics.median(v), min=s[0], max=s[-1], p10=s[len(s) // 10], p90=s[(9 * len(s)) // 10], samples=len(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--burst", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=24576)
    ap.add_argument("--hidden", default="512,256,128", help="actor_hidden_dims = critic_hidden_dims of the go2 policy")
    ap.add_argument("--sides", default=",".join(SIDES))
    ap.add_argument("--child", choices=SIDES, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    from hcr_genesis_lr_cl_amd import build as b
    want = [s for s in args.sides.split(",") if s]
    times, agree, shape = {}, {}, {}
    for _ in range(args.rounds):
        for side in want:                                    # a fresh process per side, the sides alternating
            cmd = [sys.executable, os.path.abspath(__file__), "--child", side, "--repeats", str(args.repeats), "--burst", str(args.burst),
                   "--warmup", str(args.warmup), "--hidden", args.hidden, "--rows", str(args.rows)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = next((l for l in r.stdout.splitlines() if l.startswith("CHILD ")), None)
            if r.returncode != 0 or line is None:
                sys.exit(f"train_pass_time.py: the {side} process failed (exit status {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            d = json.loads(line[6:])
            for cut in CUTS:
                times.setdefault(side, {}).setdefault(cut, []).extend(d["us"][cut])
            agree[side], shape = d["agree"], dict(rows=d["rows"], floats=d["floats"])
    res = dict(tool="train_pass_time", rounds=args.rounds, repeats=args.repeats, burst=args.burst, source_hash=b.source_hash(), **shape,
               max_rel_diff_vs_torch=agree, call_us={s: {c: stat(v) for c, v in cuts.items()} for s, cuts in times.items()})
    print(f"go2 mini-batch: {shape['rows']} rows, {shape['floats']} parameters")
    for s, cuts in res["call_us"].items():
        for c, v in cuts.items():
            print(f"  {s:12s} {c:8s}: median {v['median']:9.1f} us   min {v['min']:9.1f}   p10-p90 {v['p10']:9.1f} - {v['p90']:9.1f}   max {v['max']:9.1f}   "
                  f"({v['samples']} samples; against the torch module: {agree[s]:.1e} relative)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

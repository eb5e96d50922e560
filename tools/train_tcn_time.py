"""Developer tool (GPU only, never read by bench.py): time of one mini-batch of the teacher-student learner where ActorCriticTS has its "TCN"
history encoder (PPO_TS, 24576 rows = 4096 envs x 24 steps / 4 mini-batches), for the reference's go2_ts TCN settings and a wider variant,

  go2_ts_tcn    H 900; Conv1d channels [1, 1, 1, 1], dilation [1, 1, 2, 1], stride [1, 2, 1, 2], kernel 5, padding 2 d; F = 225; tail 225-128-94
  go2_ts_tcn8   the same with channels [8, 8, 8, 8]; F = 1800; tail 1800-128-94: reported without a target, so the cost of wider layers is on record

(privilege encoder 94-256-128-94, actor 139-512-256-128-12, critic 860-1024-256-128-1 in both) in three cuts:

  enc_forward  the encoder loss alone: conv stack, flatten, tail, target, masked mean-squared error
  enc_step     zero_grad, the encoder loss, backward, FusedAdam.step(): one history-encoder step
  minibatch    one RL step (zero_grad, forward, FusedPPOLoss, backward, FusedAdam.step(kl_mean)) and one encoder step

on four sides:

  fused_eager   FusedTrainPassTSTcn (csrc/lg_train_tcn.hip for the encoder pass, csrc/lg_train_ts.hip for the RL pass), eager
  fused_graph   the same, each cut captured once on one stream and replayed as one HIP graph
  torch_eager   the torch module (nn.Conv1d stack, Flatten, Linear, no_grad target, mse_loss, autograd), eager: what runs without this pass
  torch_graph   the same, captured and replayed as one HIP graph

FusedPPOLoss and FusedAdam are on every side, so the difference between a fused and a torch side is the networks' passes alone.

Method (as tools/train_tcn_time.py): a fresh child process per side and round (the parent never opens the device), the sides alternating
within every round; a child first checks that its side's encoder loss and parameter gradients agree with the torch module's on the same
seeded weights and batch, warms up, then takes --repeats samples per cut, each the device-event time around a burst of --burst calls divided
by the burst length.  Everything runs on one side stream.  Median and p10-p90 over all samples of a side.

    python tools/train_tcn_time.py [--rounds 2] [--repeats 10] [--burst 5] [--rows 24576] [--tasks go2_ts_tcn,go2_ts_tcn8] [--sides fused_eager,...]

The per-kernel split is a run of its own:   rocprofv3 --kernel-trace --stats -d <dir> -- python tools/train_tcn_time.py --child fused_eager
--task go2_ts_tcn --repeats 2 --burst 2 --warmup 1

Prints a table, the verdict on the minibatch cut (fused p90 against torch p10, and fused p10 against torch p90, eager and graph) and one JSON
line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
SIDES = ("fused_eager", "torch_eager", "fused_graph", "torch_graph")
CUTS = ("enc_forward", "enc_step", "minibatch")
DESIRED_KL = 0.01
H, KERNEL, DILATION, STRIDE, FINAL = 900, 5, (1, 1, 2, 1), (1, 2, 1, 2), 128          # go2_ts_config.py:73-79
# task -> (privilege encoder, actor, critic widths, TCN channel dims): the reference's network settings of go2_ts
TASKS = {"go2_ts_tcn": ([94, 256, 128, 94], [139, 512, 256, 128, 12], [860, 1024, 256, 128, 1], (1, 1, 1, 1)),
         "go2_ts_tcn8": ([94, 256, 128, 94], [139, 512, 256, 128, 12], [860, 1024, 256, 128, 1], (8, 8, 8, 8))}


def build_module(task, dev, seed):
    import torch
    import torch.nn as nn
    priv, actor, critic, channels = TASKS[task]

    def tcn():
        """actor_critic_ts.py:77-99"""
        mods, cin, length = [], 1, H
        for cout, d, st in zip(channels, DILATION, STRIDE):
            mods.append(nn.Conv1d(cin, cout, KERNEL, stride=st, padding=d * (KERNEL - 1) // 2, dilation=d))
            cin, length = cout, (length - 1) // st + 1
        return nn.Sequential(*mods, nn.Flatten(), nn.Linear(length * cin, FINAL), nn.ELU(), nn.Linear(FINAL, priv[-1]))

    def chain(widths):
        mods = []
        for i in range(len(widths) - 1):
            mods.append(nn.Linear(widths[i], widths[i + 1]))
            if i < len(widths) - 2:
                mods.append(nn.ELU())
        return nn.Sequential(*mods)

    class ActorCriticTS(nn.Module):
        def __init__(self):
            super().__init__()
            self.std = nn.Parameter(torch.ones(actor[-1]))
            self.privilege_encoder, self.history_encoder, self.actor, self.critic = chain(priv), tcn(), chain(actor), chain(critic)
    torch.manual_seed(seed)
    return ActorCriticTS().to(dev)


def batch(task, rows, dev, seed):
    import torch
    priv, actor, critic, _ = TASKS[task]
    A = actor[-1]
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    old_mu, old_sigma = 0.3 * r(rows, A), torch.ones(rows, A)
    actions = old_mu + old_sigma * r(rows, A)
    old_lp = (-(actions - old_mu) ** 2 / (2 * old_sigma ** 2) - old_sigma.log() - 0.9189385332046727).sum(-1, keepdim=True)
    target = r(rows, 1)
    cols = dict(obs=r(rows, actor[0] - priv[-1]), privileged_obs=r(rows, priv[0]), critic_obs=r(rows, critic[0]), obs_history=r(rows, H),
                terminated=(torch.rand(rows, 1, generator=g) > 0.02).float(), actions=actions, old_log_prob=old_lp, advantages=r(rows, 1),
                returns=target + 0.5 * r(rows, 1), target_values=target, old_mu=old_mu, old_sigma=old_sigma)
    return {k: v.to(dev) for k, v in cols.items()}


def child(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("train_tcn_time.py: no GPU -- a time is only measured on the device")
    side_stream = torch.cuda.Stream()
    with torch.cuda.stream(side_stream):
        out = time_side(args, "cuda:0", side_stream)
    print("CHILD " + json.dumps(out))


def time_side(args, dev, side_stream):
    import torch
    from hcr_genesis_lr_cl_amd.optim import FusedAdam
    from hcr_genesis_lr_cl_amd.ppo_loss import FusedPPOLoss
    from hcr_genesis_lr_cl_amd.train import FusedTrainPassTSTcn
    side, task = args.child, args.task
    loss_fn = FusedPPOLoss(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01)

    def learner(fused):
        """(module, the cuts as functions) of one side over a fresh module with the seeded weights."""
        m = build_module(task, dev, 1)
        t = batch(task, args.rows, dev, 2)
        tp = FusedTrainPassTSTcn(m) if fused else None
        rl_params = list(m.actor.parameters()) + list(m.critic.parameters()) + list(m.privilege_encoder.parameters()) + [m.std]
        enc_params = list(m.history_encoder.parameters())
        rl_opt = FusedAdam(rl_params, lr=1e-3, max_grad_norm=1.0, desired_kl=DESIRED_KL)
        enc_opt = FusedAdam(enc_params, lr=1e-3, max_grad_norm=1.0)

        def rl_forward():
            if fused:
                return tp(t["obs"], t["privileged_obs"], t["critic_obs"])
            mu = m.actor(torch.cat((t["obs"], m.privilege_encoder(t["privileged_obs"])), dim=-1))
            return mu, mu * 0.0 + m.std, m.critic(t["critic_obs"])

        def rl_fwd_bwd():
            rl_opt.zero_grad()
            mu, sigma, values = rl_forward()
            out = loss_fn(mu, sigma, values, t["actions"], t["old_log_prob"], t["advantages"], t["returns"], t["target_values"], t["old_mu"],
                          t["old_sigma"])
            out.loss.backward()
            return out

        def rl_step():
            rl_opt.step(kl_mean=rl_fwd_bwd().kl_mean)

        def enc_fwd_bwd():
            enc_opt.zero_grad()
            if fused:
                loss = tp.encoder_loss(t["obs_history"], t["privileged_obs"], t["terminated"])
            else:
                with torch.no_grad():
                    target = m.privilege_encoder(t["privileged_obs"])
                loss = torch.nn.functional.mse_loss(m.history_encoder(t["obs_history"].unsqueeze(1)) * t["terminated"], target * t["terminated"])
            loss.backward()
            return loss

        def enc_forward():
            if fused:
                return tp.encoder_loss(t["obs_history"], t["privileged_obs"], t["terminated"])
            with torch.no_grad():
                target = m.privilege_encoder(t["privileged_obs"])
                return torch.nn.functional.mse_loss(m.history_encoder(t["obs_history"].unsqueeze(1)) * t["terminated"], target * t["terminated"])

        def enc_step():
            enc_fwd_bwd()
            enc_opt.step()

        def minibatch():
            rl_step()
            enc_step()
        return m, rl_params, enc_params, dict(rl_forward=rl_forward, rl_fwd_bwd=rl_fwd_bwd, enc_fwd_bwd=enc_fwd_bwd, enc_forward=enc_forward, rl_step=rl_step,
                                              enc_step=enc_step, minibatch=minibatch)

    # agreement with the torch module: outputs, encoder loss and gradients of one forward and backward of each pass on the seeded weights
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    sides = [learner(False), learner(side.startswith("fused"))]
    seen = []
    for m, rl_params, enc_params, cuts in sides:
        outs = [x.detach().clone() for x in cuts["rl_forward"]()]
        cuts["rl_fwd_bwd"]()
        rl_grads = [p.grad.detach().clone() for p in rl_params]
        loss = cuts["enc_fwd_bwd"]().detach().clone().reshape(1)
        seen.append(outs + [loss] + rl_grads + [p.grad.detach().clone() for p in enc_params])
    side_stream.synchronize()
    agree = max(rel(a, b) for a, b in zip(seen[1], seen[0]))
    if not agree <= 1e-3:
        sys.exit(f"train_tcn_time.py: {task} {side}: outputs, loss or gradients disagree with the torch module by {agree:.3e} (relative) -- nothing timed")
    m, _, _, cuts = sides[1]
    del sides, seen

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
    ap.add_argument("--tasks", default=",".join(TASKS))
    ap.add_argument("--sides", default=",".join(SIDES))
    ap.add_argument("--child", choices=SIDES, help=argparse.SUPPRESS)
    ap.add_argument("--task", choices=tuple(TASKS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    from hcr_genesis_lr_cl_amd import build as b
    want = [s for s in args.sides.split(",") if s]
    res = dict(tool="train_tcn_time", rounds=args.rounds, repeats=args.repeats, burst=args.burst, source_hash=b.source_hash(), tasks={})
    for task in [t for t in args.tasks.split(",") if t]:
        times, agree, shape = {}, {}, {}
        for _ in range(args.rounds):
            for side in want:                                    # a fresh process per side, the sides alternating
                cmd = [sys.executable, os.path.abspath(__file__), "--child", side, "--task", task, "--repeats", str(args.repeats), "--burst",
                       str(args.burst), "--warmup", str(args.warmup), "--rows", str(args.rows)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                line = next((l for l in r.stdout.splitlines() if l.startswith("CHILD ")), None)
                if r.returncode != 0 or line is None:
                    sys.exit(f"train_tcn_time.py: the {task} {side} process failed (exit status {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                d = json.loads(line[6:])
                for cut in CUTS:
                    times.setdefault(side, {}).setdefault(cut, []).extend(d["us"][cut])
                agree[side], shape = d["agree"], dict(rows=d["rows"], floats=d["floats"])
        call_us = {s: {c: stat(v) for c, v in cuts.items()} for s, cuts in times.items()}
        print(f"{task} mini-batch: {shape['rows']} rows, {shape['floats']} parameters")
        for s, cuts in call_us.items():
            for c, v in cuts.items():
                print(f"  {s:12s} {c:10s}: median {v['median']:9.1f} us   min {v['min']:9.1f}   p10-p90 {v['p10']:9.1f} - {v['p90']:9.1f}   max {v['max']:9.1f}   "
                      f"({v['samples']} samples; against the torch module: {agree[s]:.1e} relative)")
        verdict = {}
        for form in ("eager", "graph"):
            f, t = call_us.get("fused_" + form), call_us.get("torch_" + form)
            if f and t:
                verdict[form] = bool(f["minibatch"]["p90"] < t["minibatch"]["p10"])
                weak = bool(f["minibatch"]["p10"] < t["minibatch"]["p90"])
                print(f"  minibatch, {form}: fused p90 {f['minibatch']['p90']:.1f} us {'<' if verdict[form] else '>='} torch p10 {t['minibatch']['p10']:.1f} us: "
                      f"{'the fused side wins, the intervals separate' if verdict[form] else 'NO separated win'}; fused p10 {f['minibatch']['p10']:.1f} us "
                      f"{'<' if weak else '>='} torch p90 {t['minibatch']['p90']:.1f} us")
        res["tasks"][task] = dict(**shape, max_rel_diff_vs_torch=agree, call_us=call_us, fused_wins=verdict)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

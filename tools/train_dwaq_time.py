"""Developer tool (GPU only, never read by bench.py): time of one mini-batch of the DreamWaQ learner (PPO_DreamWaQ on ActorCriticDreamWaQ;
18000 rows = 3000 envs x 24 steps / 4 mini-batches, what the reference's go2_dreamwaq configuration gives) for the shipped configuration,

  go2_dreamwaq   encoder 900-256-128-80 (an ELU behind every Linear), heads 80 -> 16 / 16 / 24 / 24 (log-variances behind Hardtanh +-5),
                 decoder 40-256-128-45, actor 85-512-256-128-12 (no Hardtanh), critic 885-1024-256-128-1, vae_kld_weight 2

in four cuts:

  rl_forward   the RL training forward alone: mu, sigma, values with everything the backward needs kept
  rl_step      zero_grad, forward, FusedPPOLoss, loss.backward(), FusedAdam.step(kl_mean): one RL step of PPO_DreamWaQ.update()
  vae_step     zero_grad, the VAE loss, backward, FusedAdam.step(): one VAE step
  minibatch    one RL step and num_encoder_epochs = 1 VAE step: what PPO_DreamWaQ.update() costs per mini-batch

on four sides:

  fused_eager   FusedTrainPassDreamWaQ (csrc/lg_train_dwaq.hip) for the networks and the VAE loss, eager
  fused_graph   the same, each cut captured once on one stream and replayed as one HIP graph
  torch_eager   the torch module (nn.Sequential, the reparameterised draw, torch.cat, mse_loss, the broadcast KL term, autograd), eager: the
                code before FusedTrainPassDreamWaQ
  torch_graph   the same, captured and replayed as one HIP graph

FusedPPOLoss and FusedAdam are on every side, so the difference between a fused and a torch side is the networks' passes alone.  Both sides
read the same caller-owned noise tensors (a captured graph needs them), so neither pays for a random draw.  The torch side's RL backward
also runs through the VAE, as the reference's does before vae_optimizer.zero_grad() discards that gradient; the fused side never forms it.
The torch side writes the KL term as the product of its two sums: the reference's (B, B) product is 1.3 GB at 18000 rows and would only
slow the torch side down.

Method (as tools/train_dwaq_time.py): a fresh child process per side and round (the parent never opens the device), the sides alternating
within every round; a child first checks that its side's outputs, VAE losses and parameter gradients agree with the torch module's on the
same seeded weights and batch, warms up, then takes --repeats samples per cut, each the device-event time around a burst of --burst calls
divided by the burst length.  Everything runs on one side stream.  Median and p10-p90 over all samples of a side.

    python tools/train_dwaq_time.py [--rounds 2] [--repeats 10] [--burst 5] [--rows 18000] [--sides fused_eager,...]

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
CUTS = ("rl_forward", "rl_step", "vae_step", "minibatch")
DESIRED_KL = 0.01
KLD_WEIGHT, VAR_CLIP = 2.0, 5.0
# task -> (encoder, L, E, decoder, actor, critic) widths: the reference's network settings of go2_dreamwaq
TASKS = {"go2_dreamwaq": ([900, 256, 128, 80], 16, 24, [40, 256, 128, 45], [85, 512, 256, 128, 12], [885, 1024, 256, 128, 1])}


def build_module(task, dev, seed):
    import torch
    import torch.nn as nn
    enc, L, E, dec, actor, critic = TASKS[task]

    def chain(widths, last_elu=False):
        mods = []
        for i in range(len(widths) - 1):
            mods.append(nn.Linear(widths[i], widths[i + 1]))
            if i < len(widths) - 2 or last_elu:
                mods.append(nn.ELU())
        return nn.Sequential(*mods)

    class VAE(nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder = chain(enc, True)
            self.latent_mu = nn.Linear(enc[-1], L)
            self.latent_var = nn.Sequential(nn.Linear(enc[-1], L), nn.Hardtanh(-VAR_CLIP, VAR_CLIP))
            self.vel_mu = nn.Linear(enc[-1], E)
            self.vel_var = nn.Sequential(nn.Linear(enc[-1], E), nn.Hardtanh(-VAR_CLIP, VAR_CLIP))
            self.decoder = chain(dec)

        def forward(self, history, noise):
            h = self.encoder(history)
            lmu, llv, vmu, vlv = self.latent_mu(h), self.latent_var(h), self.vel_mu(h), self.vel_var(h)
            return noise[:, :L] * torch.exp(0.5 * llv) + lmu, noise[:, L:] * torch.exp(0.5 * vlv) + vmu, lmu, llv

    class ActorCriticDreamWaQ(nn.Module):
        def __init__(self):
            super().__init__()
            self.vae, self.actor, self.critic = VAE(), chain(actor), chain(critic)
            self.std = nn.Parameter(torch.ones(actor[-1]))
    torch.manual_seed(seed)
    return ActorCriticDreamWaQ().to(dev)


def batch(task, rows, dev, seed):
    import torch
    enc, L, E, dec, actor, critic = TASKS[task]
    A = actor[-1]
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    old_mu, old_sigma = 0.3 * r(rows, A), torch.ones(rows, A)
    actions = old_mu + old_sigma * r(rows, A)
    old_lp = (-(actions - old_mu) ** 2 / (2 * old_sigma ** 2) - old_sigma.log() - 0.9189385332046727).sum(-1, keepdim=True)
    target = r(rows, 1)
    cols = dict(obs=r(rows, actor[0] - L - E), critic_obs=r(rows, critic[0]), obs_history=r(rows, enc[0]), noise=r(rows, L + E), vae_noise=r(rows, L + E),
                labels=r(rows, E), next_states=r(rows, dec[-1]), terminated=(torch.rand(rows, 1, generator=g) > 0.02).float(), actions=actions,
                old_log_prob=old_lp, advantages=r(rows, 1), returns=target + 0.5 * r(rows, 1), target_values=target, old_mu=old_mu, old_sigma=old_sigma)
    return {k: v.to(dev) for k, v in cols.items()}


def child(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("train_dwaq_time.py: no GPU -- a time is only measured on the device")
    side_stream = torch.cuda.Stream()
    with torch.cuda.stream(side_stream):
        out = time_side(args, "cuda:0", side_stream)
    print("CHILD " + json.dumps(out))


def time_side(args, dev, side_stream):
    import torch
    from hcr_genesis_lr_cl_amd.optim import FusedAdam
    from hcr_genesis_lr_cl_amd.ppo_loss import FusedPPOLoss
    from hcr_genesis_lr_cl_amd.train import FusedTrainPassDreamWaQ
    side, task = args.child, args.task
    loss_fn = FusedPPOLoss(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01)

    def learner(fused):
        """(module, the cuts as functions) of one side over a fresh module with the seeded weights."""
        m = build_module(task, dev, 1)
        t = batch(task, args.rows, dev, 2)
        tp = FusedTrainPassDreamWaQ(m, kld_weight=KLD_WEIGHT) if fused else None
        rl_params = list(m.actor.parameters()) + list(m.critic.parameters()) + [m.std]
        vae_params = list(m.vae.parameters())
        rl_opt = FusedAdam(rl_params, lr=1e-3, max_grad_norm=1.0, desired_kl=DESIRED_KL)
        vae_opt = FusedAdam(vae_params, lr=1e-3, max_grad_norm=1.0)
        F = torch.nn.functional

        def rl_forward():
            if fused:
                return tp(t["obs"], t["obs_history"], t["critic_obs"], t["noise"])
            z, v, _, _ = m.vae(t["obs_history"], t["noise"])
            mu = m.actor(torch.cat((t["obs"], z, v), dim=-1))
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

        def vae_fwd_bwd():
            vae_opt.zero_grad()
            if fused:
                out = tp.vae_loss(t["obs_history"], t["labels"], t["next_states"], t["terminated"], t["vae_noise"])
                loss, parts = out.loss, torch.stack([out.explicit_estimation_loss, out.reconstruction_loss, out.kld_loss])
            else:
                term = t["terminated"]
                z, v, lmu, llv = m.vae(t["obs_history"], t["vae_noise"])
                rec = m.vae.decoder(torch.cat((z, v), dim=1))
                est, recl = F.mse_loss(v * term, t["labels"] * term), F.mse_loss(rec * term, t["next_states"] * term)
                s = torch.sum(1 + llv - lmu ** 2 - llv.exp(), dim=1)
                kld = -0.5 * (s.sum() * term.sum()) / float(s.shape[0]) ** 2          # the mean of the reference's (B, B) product
                loss, parts = est + recl + KLD_WEIGHT * kld, torch.stack([est, recl, kld]).detach()
            loss.backward()
            return torch.cat([loss.detach().reshape(1), parts])

        def vae_step():
            vae_fwd_bwd()
            vae_opt.step()

        def minibatch():
            rl_step()
            vae_step()
        return m, rl_params, vae_params, dict(rl_forward=rl_forward, rl_fwd_bwd=rl_fwd_bwd, vae_fwd_bwd=vae_fwd_bwd, rl_step=rl_step, vae_step=vae_step,
                                              minibatch=minibatch)

    # agreement with the torch module: outputs, VAE losses and gradients of one forward and backward of each pass on the seeded weights
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    sides = [learner(False), learner(side.startswith("fused"))]
    seen = []
    for m, rl_params, vae_params, cuts in sides:
        outs = [x.detach().clone() for x in cuts["rl_forward"]()]
        cuts["rl_fwd_bwd"]()
        rl_grads = [p.grad.detach().clone() for p in rl_params]
        losses = cuts["vae_fwd_bwd"]().clone()
        seen.append(outs + [losses] + rl_grads + [p.grad.detach().clone() for p in vae_params])
    side_stream.synchronize()
    agree = max(rel(a, b) for a, b in zip(seen[1], seen[0]))
    if not agree <= 1e-3:
        sys.exit(f"train_dwaq_time.py: {task} {side}: outputs, loss or gradients disagree with the torch module by {agree:.3e} (relative) -- nothing timed")
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
    ap.add_argument("--rows", type=int, default=18000)
    ap.add_argument("--tasks", default=",".join(TASKS))
    ap.add_argument("--sides", default=",".join(SIDES))
    ap.add_argument("--child", choices=SIDES, help=argparse.SUPPRESS)
    ap.add_argument("--task", choices=tuple(TASKS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    from hcr_genesis_lr_cl_amd import build as b
    want = [s for s in args.sides.split(",") if s]
    res = dict(tool="train_dwaq_time", rounds=args.rounds, repeats=args.repeats, burst=args.burst, source_hash=b.source_hash(), tasks={})
    for task in [t for t in args.tasks.split(",") if t]:
        times, agree, shape = {}, {}, {}
        for _ in range(args.rounds):
            for side in want:                                    # a fresh process per side, the sides alternating
                cmd = [sys.executable, os.path.abspath(__file__), "--child", side, "--task", task, "--repeats", str(args.repeats), "--burst",
                       str(args.burst), "--warmup", str(args.warmup), "--rows", str(args.rows)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                line = next((l for l in r.stdout.splitlines() if l.startswith("CHILD ")), None)
                if r.returncode != 0 or line is None:
                    sys.exit(f"train_dwaq_time.py: the {task} {side} process failed (exit status {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
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

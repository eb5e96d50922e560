"""Developer tool (GPU only, never read by bench.py): time of one mini-batch of the recurrent learner (PPO on ActorCriticRecurrent) for the
go2_lstm set of DESIGN.md section 10b: obs 45, critic obs 61, one LSTM layer of H = 256 per memory, actor and critic 256-256-256-256-out,
A = 12; 4096 envs, T = 24, 4 mini-batches, so 1024 envs and 24576 unpadded rows per mini-batch, cut into trajectories by dones drawn with
probability --p-done per step (about 1500 trajectories),

in two cuts:

  rl_forward   the training forward alone: mu, sigma and values of the mini-batch, with everything the backward needs kept
  rl_step      zero_grad, forward, FusedPPOLoss, loss.backward(), FusedAdam.step(kl_mean): one mini-batch step of PPO.update()

on four sides:

  fused_eager   FusedTrainPassRecurrent (csrc/lg_train_rnn.hip) for the memories and the MLPs, eager
  fused_graph   the same, each cut captured once on one stream and replayed as one HIP graph
  torch_eager   the torch module (nn.LSTM over the padded trajectories, the unpadding, nn.Sequential, autograd), eager: the code before
                FusedTrainPassRecurrent.  The boolean-mask gather of unpad_trajectories synchronises with the host and cannot be captured,
                so both torch sides unpad by an index_select on row indices computed once, outside the timed region: the torch side is
                not charged for that mask
  torch_graph   the same, captured and replayed as one HIP graph

FusedPPOLoss and FusedAdam are on every side, so the difference between a fused and a torch side is the network passes alone.

Method (as tools/train_cts_time.py): a fresh child process per side and round (the parent never opens the device), the sides alternating
within every round; a child first checks that its side's outputs and parameter gradients agree with the torch module's on the same seeded
weights and batch and refuses to time a side that disagrees, warms up, then takes --repeats samples per cut, each the device-event time
around a burst of --burst calls divided by the burst length.  Everything runs on one side stream.  Median and p10-p90 over all samples of
a side.

    python tools/train_recurrent_time.py [--rounds 2] [--repeats 10] [--burst 5] [--envs 1024] [--steps 24] [--p-done 0.02] [--sides fused_eager,...]

Prints a table, the verdict on the rl_step cut (fused p90 against torch p10, and fused p10 against torch p90, eager and graph) and one JSON
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
CUTS = ("rl_forward", "rl_step")
DESIRED_KL = 0.01
# set -> obs, critic obs, rnn kind, layers, H, the hidden widths of both MLPs, A
SETS = {"go2_lstm": dict(obs=45, cobs=61, kind="lstm", layers=1, H=256, mlp=[256, 256, 256], A=12)}


def build_module(name, dev, seed):
    import torch
    import torch.nn as nn
    d = SETS[name]

    def chain(widths, clip):
        mods = []
        for i in range(len(widths) - 1):
            mods.append(nn.Linear(widths[i], widths[i + 1]))
            if i < len(widths) - 2:
                mods.append(nn.ELU())
        return nn.Sequential(*mods, *([nn.Hardtanh(-clip, clip)] if clip else []))

    class Memory(nn.Module):
        def __init__(self, n_in):
            super().__init__()
            self.rnn = (nn.LSTM if d["kind"] == "lstm" else nn.GRU)(input_size=n_in, hidden_size=d["H"], num_layers=d["layers"])

    class ActorCriticRecurrent(nn.Module):
        is_recurrent = True

        def __init__(self):
            super().__init__()
            self.actor, self.critic = chain([d["H"], *d["mlp"], d["A"]], 100.0), chain([d["H"], *d["mlp"], 1], None)
            self.std = nn.Parameter(torch.ones(d["A"]))
            self.memory_a, self.memory_c = Memory(d["obs"]), Memory(d["cobs"])
    torch.manual_seed(seed)
    return ActorCriticRecurrent().to(dev)


def batch(name, envs, steps, p_done, dev, seed):
    """One recurrent mini-batch as RolloutStorage.reccurent_mini_batch_generator yields it, and the columns of the loss head."""
    import torch
    d = SETS[name]
    T, E, A, H, L = steps, envs, d["A"], d["H"], d["layers"]
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    dones = torch.rand(T, E, generator=g) < p_done
    dones[-1] = True
    flat = dones.t().reshape(-1)
    ends = flat.nonzero()[:, 0]
    lens = ends - torch.cat((ends.new_tensor([-1]), ends[:-1]))
    n_traj, max_len = int(lens.numel()), int(lens.max())
    masks = lens.unsqueeze(0) > torch.arange(T).unsqueeze(1)
    pad = lambda w: torch.where(masks[:max_len, :, None], r(max_len, n_traj, w), torch.zeros(()))
    start = lambda: [0.3 * r(L, n_traj, H) for _ in range(2 if d["kind"] == "lstm" else 1)]
    hid_a, hid_c = start(), start()
    N = T * E
    old_mu, old_sigma = 0.3 * r(N, A), torch.ones(N, A)
    actions = old_mu + old_sigma * r(N, A)
    old_lp = (-(actions - old_mu) ** 2 / (2 * old_sigma ** 2) - old_sigma.log() - 0.9189385332046727).sum(-1, keepdim=True)
    target = r(N, 1)
    cols = dict(obs=pad(d["obs"]), critic_obs=pad(d["cobs"]), masks=masks, actions=actions, old_log_prob=old_lp, advantages=r(N, 1), old_mu=old_mu,
                old_sigma=old_sigma, returns=target + 0.5 * r(N, 1), target_values=target)
    cols = {k: v.to(dev) for k, v in cols.items()}
    to = lambda h: [t.to(dev) for t in h] if len(h) > 1 else h[0].to(dev)
    cols["hid"] = (to(hid_a), to(hid_c))
    # unpad_trajectories as a gather: row t E + e of the unpadded order comes from row j max_len + t' of the (n_traj, max_len) flattening
    m = masks[:max_len].t()
    src = m.reshape(-1).nonzero()[:, 0]                                   # trajectory-major valid positions: env-major, time inside
    cols["unpad_index"] = src.view(E, T).t().reshape(-1).to(dev)          # (e, t) -> (t, e)
    return cols, dict(envs=E, steps=T, n_traj=n_traj, max_len=max_len)


def child(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("train_recurrent_time.py: no GPU -- a time is only measured on the device")
    side_stream = torch.cuda.Stream()
    with torch.cuda.stream(side_stream):
        out = time_side(args, "cuda:0", side_stream)
    print("CHILD " + json.dumps(out))


def time_side(args, dev, side_stream):
    import torch
    from hcr_genesis_lr_cl_amd.optim import FusedAdam
    from hcr_genesis_lr_cl_amd.ppo_loss import FusedPPOLoss
    from hcr_genesis_lr_cl_amd.train import FusedTrainPassRecurrent
    side, name = args.child, args.set
    loss_fn = FusedPPOLoss(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01)
    shape = {}

    def learner(fused):
        """(module, the cuts as functions) of one side over a fresh module with the seeded weights."""
        m = build_module(name, dev, 1)
        t, sizes = batch(name, args.envs, args.steps, args.p_done, dev, 2)
        shape.update(sizes)
        tp = FusedTrainPassRecurrent(m) if fused else None
        opt = FusedAdam(m.named_parameters(), lr=1e-3, max_grad_norm=1.0, desired_kl=DESIRED_KL)
        tup = lambda h: tuple(h) if isinstance(h, list) else h

        def rl_forward():
            if fused:
                return tp(t["obs"], t["critic_obs"], t["masks"], t["hid"], n_envs=args.envs)
            tops = []
            for mem, x, h in ((m.memory_a, t["obs"], t["hid"][0]), (m.memory_c, t["critic_obs"], t["hid"][1])):
                y, _ = mem.rnn(x, tup(h))
                tops.append(y.transpose(1, 0).flatten(0, 1).index_select(0, t["unpad_index"]))
            mu = m.actor(tops[0])
            return mu, mu * 0.0 + m.std, m.critic(tops[1])

        def rl_fwd_bwd():
            opt.zero_grad()
            mu, sigma, values = rl_forward()
            out = loss_fn(mu, sigma, values, t["actions"], t["old_log_prob"], t["advantages"], t["returns"], t["target_values"], t["old_mu"], t["old_sigma"])
            out.loss.backward()
            return out

        def rl_step():
            opt.step(kl_mean=rl_fwd_bwd().kl_mean)
        return m, dict(rl_forward=rl_forward, rl_fwd_bwd=rl_fwd_bwd, rl_step=rl_step)

    # agreement with the torch module: outputs and gradients of one forward and backward on the seeded weights
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    sides = [learner(False), learner(side.startswith("fused"))]
    seen = []
    for m, cuts in sides:
        outs = [x.detach().clone() for x in cuts["rl_forward"]()]
        cuts["rl_fwd_bwd"]()
        seen.append(outs + [p.grad.detach().clone() for p in m.parameters()])
    side_stream.synchronize()
    agree = max(rel(a, b) for a, b in zip(seen[1], seen[0]))
    if not agree <= 1e-3:
        sys.exit(f"train_recurrent_time.py: {name} {side}: outputs or gradients disagree with the torch module by {agree:.3e} (relative) -- nothing timed")
    m, cuts = sides[1]
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
    return dict(shape=shape, floats=sum(p.numel() for p in m.parameters()), agree=agree, us=times)


def stat(v):
    s = sorted(v)
    return dict(median=statistics.median(v), min=s[0], max=s[-1], p10=s[len(s) // 10], p90=s[(9 * len(s)) // 10], samples=len(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--burst", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--p-done", type=float, default=0.02)
    ap.add_argument("--sets", default=",".join(SETS))
    ap.add_argument("--sides", default=",".join(SIDES))
    ap.add_argument("--child", choices=SIDES, help=argparse.SUPPRESS)
    ap.add_argument("--set", choices=tuple(SETS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    from hcr_genesis_lr_cl_amd import build as b
    want = [s for s in args.sides.split(",") if s]
    res = dict(tool="train_recurrent_time", rounds=args.rounds, repeats=args.repeats, burst=args.burst, source_hash=b.source_hash(), sets={})
    for name in [t for t in args.sets.split(",") if t]:
        times, agree, shape = {}, {}, {}
        for _ in range(args.rounds):
            for side in want:                                    # a fresh process per side, the sides alternating
                cmd = [sys.executable, os.path.abspath(__file__), "--child", side, "--set", name, "--repeats", str(args.repeats), "--burst", str(args.burst),
                       "--warmup", str(args.warmup), "--envs", str(args.envs), "--steps", str(args.steps), "--p-done", str(args.p_done)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                line = next((l for l in r.stdout.splitlines() if l.startswith("CHILD ")), None)
                if r.returncode != 0 or line is None:
                    sys.exit(f"train_recurrent_time.py: the {name} {side} process failed (exit status {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                d = json.loads(line[6:])
                print(f"train_recurrent_time.py: {name} {side}: {len(d['us'][CUTS[-1]])} samples per cut", file=sys.stderr, flush=True)
                for cut in CUTS:
                    times.setdefault(side, {}).setdefault(cut, []).extend(d["us"][cut])
                agree[side], shape = d["agree"], dict(d["shape"], floats=d["floats"])
        call_us = {s: {c: stat(v) for c, v in cuts.items()} for s, cuts in times.items()}
        print(f"{name} mini-batch: {shape['envs']} envs x {shape['steps']} steps in {shape['n_traj']} trajectories (max_len {shape['max_len']}), "
              f"{shape['floats']} parameters")
        for s, cuts in call_us.items():
            for c, v in cuts.items():
                print(f"  {s:12s} {c:10s}: median {v['median']:9.1f} us   min {v['min']:9.1f}   p10-p90 {v['p10']:9.1f} - {v['p90']:9.1f}   max {v['max']:9.1f}   "
                      f"({v['samples']} samples; against the torch module: {agree[s]:.1e} relative)")
        verdict = {}
        for form in ("eager", "graph"):
            f, t = call_us.get("fused_" + form), call_us.get("torch_" + form)
            if f and t:
                verdict[form] = bool(f["rl_step"]["p90"] < t["rl_step"]["p10"])
                weak = bool(f["rl_step"]["p10"] < t["rl_step"]["p90"])
                print(f"  rl_step, {form}: fused p90 {f['rl_step']['p90']:.1f} us {'<' if verdict[form] else '>='} torch p10 {t['rl_step']['p10']:.1f} us: "
                      f"{'the fused side wins, the intervals separate' if verdict[form] else 'NO separated win'}; fused p10 {f['rl_step']['p10']:.1f} us "
                      f"{'<' if weak else '>='} torch p90 {t['rl_step']['p90']:.1f} us")
        res["sets"][name] = dict(**shape, max_rel_diff_vs_torch=agree, call_us=call_us, fused_wins=verdict)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

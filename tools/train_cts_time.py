"""Developer tool (GPU only, never read by bench.py): time of one mini-batch of the concurrent teacher-student learner (PPO_CTS on
ActorCriticCTS) for the shipped CTS configuration: 4096 envs of which 3072 teachers, 24 steps, 4 mini-batches, so 18432 teacher + 6144
student + 24576 critic rows, on config.py's go2_cts sizes,

  go2_cts  privilege encoder 99-256-128-99, actor 144-512-256-128-12 (no Hardtanh), critic 885-1024-256-128-1, history encoder 900-256-128-99

in four cuts:

  rl_forward   the RL training forward alone: both groups' mu and sigma and the values, with everything the backward needs kept
  rl_step      zero_grad, forward, FusedPPOLoss.cts, loss.backward(), FusedAdam.step(kl_mean): one RL step of PPO_CTS.update()
  enc_step     zero_grad, the encoder loss on the student rows, backward, FusedAdam.step(): one history-encoder step
  minibatch    one RL step and num_encoder_epochs = 1 encoder step: what PPO_CTS.update() costs per mini-batch

on four sides:

  fused_eager   FusedTrainPassCTS (csrc/lg_train_cts.hip, and csrc/lg_train_ts.hip's encoder kernels) for the networks and the encoder loss, eager
  fused_graph   the same, each cut captured once on one stream and replayed as one HIP graph
  torch_eager   the torch module (nn.Sequential, two torch.cat, no_grad target, mse_loss, autograd), eager: the code before FusedTrainPassCTS
  torch_graph   the same, captured and replayed as one HIP graph

FusedPPOLoss.cts and FusedAdam are on every side, so the difference between a fused and a torch side is the networks' passes alone.  The
torch side also pays the RL gradient of the history encoder, which the reference computes and then discards; the fused side does not.

Method (as tools/train_ts_time.py): a fresh child process per side and round (the parent never opens the device), the sides alternating
within every round; a child first checks that its side's outputs, encoder loss and parameter gradients agree with the torch module's on the
same seeded weights and batch and refuses to time a side that disagrees, warms up, then takes --repeats samples per cut, each the
device-event time around a burst of --burst calls divided by the burst length.  Everything runs on one side stream.  Median and p10-p90
over all samples of a side.

    python tools/train_cts_time.py [--rounds 2] [--repeats 10] [--burst 5] [--teacher 18432] [--student 6144] [--critic 24576] [--sides fused_eager,...]

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
CUTS = ("rl_forward", "rl_step", "enc_step", "minibatch")
DESIRED_KL = 0.01
# task -> (privilege encoder, actor, critic, history encoder) widths: config.py's go2_cts sizes
TASKS = {"go2_cts": ([99, 256, 128, 99], [144, 512, 256, 128, 12], [885, 1024, 256, 128, 1], [900, 256, 128, 99])}


def build_module(task, dev, seed):
    import torch
    import torch.nn as nn
    priv, actor, critic, hist = TASKS[task]

    def chain(widths):
        mods = []
        for i in range(len(widths) - 1):
            mods.append(nn.Linear(widths[i], widths[i + 1]))
            if i < len(widths) - 2:
                mods.append(nn.ELU())
        return nn.Sequential(*mods)

    class ActorCriticCTS(nn.Module):
        def __init__(self):
            super().__init__()
            self.std = nn.Parameter(torch.ones(actor[-1]))
            self.privilege_encoder, self.history_encoder, self.actor, self.critic = chain(priv), chain(hist), chain(actor), chain(critic)
    torch.manual_seed(seed)
    return ActorCriticCTS().to(dev)


def batch(task, rows, dev, seed):
    """The 18 columns of one mini-batch; rows = (teacher, student, critic)."""
    import torch
    priv, actor, critic, hist = TASKS[task]
    A, O = actor[-1], actor[0] - priv[-1]
    bt, bs, bc = rows
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    cols = {}
    for tag, n in (("teacher", bt), ("student", bs)):
        old_mu, old_sigma = 0.3 * r(n, A), torch.ones(n, A)
        actions = old_mu + old_sigma * r(n, A)
        old_lp = (-(actions - old_mu) ** 2 / (2 * old_sigma ** 2) - old_sigma.log() - 0.9189385332046727).sum(-1, keepdim=True)
        cols.update({f"{tag}_obs": r(n, O), f"{tag}_privileged_obs": r(n, priv[0]), f"{tag}_actions": actions, f"{tag}_old_log_prob": old_lp,
                     f"{tag}_advantages": r(n, 1), f"{tag}_old_mu": old_mu, f"{tag}_old_sigma": old_sigma})
    target = r(bc, 1)
    cols.update(student_obs_history=r(bs, hist[0]), critic_obs=r(bc, critic[0]), returns=target + 0.5 * r(bc, 1), target_values=target)
    return {k: v.to(dev) for k, v in cols.items()}


def child(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("train_cts_time.py: no GPU -- a time is only measured on the device")
    side_stream = torch.cuda.Stream()
    with torch.cuda.stream(side_stream):
        out = time_side(args, "cuda:0", side_stream)
    print("CHILD " + json.dumps(out))


def time_side(args, dev, side_stream):
    import torch
    from hcr_genesis_lr_cl_amd.optim import FusedAdam
    from hcr_genesis_lr_cl_amd.ppo_loss import FusedPPOLoss
    from hcr_genesis_lr_cl_amd.train import FusedTrainPassCTS
    side, task = args.child, args.task
    loss_fn = FusedPPOLoss(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01)

    def learner(fused):
        """(module, the cuts as functions) of one side over a fresh module with the seeded weights."""
        m = build_module(task, dev, 1)
        t = batch(task, (args.teacher, args.student, args.critic), dev, 2)
        tp = FusedTrainPassCTS(m) if fused else None
        rl_params = list(m.actor.parameters()) + list(m.critic.parameters()) + list(m.privilege_encoder.parameters()) + [m.std]
        enc_params = list(m.history_encoder.parameters())
        rl_opt = FusedAdam(rl_params, lr=1e-3, max_grad_norm=1.0, desired_kl=DESIRED_KL)
        enc_opt = FusedAdam(enc_params, lr=1e-3, max_grad_norm=1.0)

        def rl_forward():
            if fused:
                return tp(t["teacher_obs"], t["teacher_privileged_obs"], t["student_obs"], t["student_obs_history"], t["critic_obs"])
            mu_t = m.actor(torch.cat((t["teacher_obs"], m.privilege_encoder(t["teacher_privileged_obs"])), dim=-1))
            mu_s = m.actor(torch.cat((t["student_obs"], m.history_encoder(t["student_obs_history"])), dim=-1))
            return mu_t, mu_t * 0.0 + m.std, mu_s, mu_s * 0.0 + m.std, m.critic(t["critic_obs"])

        def rl_fwd_bwd():
            rl_opt.zero_grad()
            mu_t, sigma_t, mu_s, sigma_s, values = rl_forward()
            out = loss_fn.cts(teacher=dict(mu=mu_t, sigma=sigma_t, actions=t["teacher_actions"], old_log_prob=t["teacher_old_log_prob"],
                                           advantages=t["teacher_advantages"], old_mu=t["teacher_old_mu"], old_sigma=t["teacher_old_sigma"]),
                              student=dict(mu=mu_s, sigma=sigma_s, actions=t["student_actions"], old_log_prob=t["student_old_log_prob"],
                                           advantages=t["student_advantages"]),
                              values=values, returns=t["returns"], target_values=t["target_values"])
            out.loss.backward()
            return out

        def rl_step():
            rl_opt.step(kl_mean=rl_fwd_bwd().kl_mean)

        def enc_fwd_bwd():
            enc_opt.zero_grad()
            if fused:
                loss = tp.encoder_loss(t["student_obs_history"], t["student_privileged_obs"])
            else:
                with torch.no_grad():
                    target = m.privilege_encoder(t["student_privileged_obs"])
                loss = torch.nn.functional.mse_loss(m.history_encoder(t["student_obs_history"]), target)
            loss.backward()
            return loss

        def enc_step():
            enc_fwd_bwd()
            enc_opt.step()

        def minibatch():
            rl_step()
            enc_step()
        return m, rl_params, enc_params, dict(rl_forward=rl_forward, rl_fwd_bwd=rl_fwd_bwd, enc_fwd_bwd=enc_fwd_bwd, rl_step=rl_step, enc_step=enc_step,
                                              minibatch=minibatch)

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
        sys.exit(f"train_cts_time.py: {task} {side}: outputs, loss or gradients disagree with the torch module by {agree:.3e} (relative) -- nothing timed")
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
    return dict(rows=[args.teacher, args.student, args.critic], floats=sum(p.numel() for p in m.parameters()), agree=agree, us=times)


def stat(v):
    s = sorted(v)
    return dict(median=statistics.median(v), min=s[0], max=s[-1], p10=s[len(s) // 10], p90=s[(9 * len(s)) // 10], samples=len(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--burst", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--teacher", type=int, default=18432)
    ap.add_argument("--student", type=int, default=6144)
    ap.add_argument("--critic", type=int, default=24576)
    ap.add_argument("--tasks", default=",".join(TASKS))
    ap.add_argument("--sides", default=",".join(SIDES))
    ap.add_argument("--child", choices=SIDES, help=argparse.SUPPRESS)
    ap.add_argument("--task", choices=tuple(TASKS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    from hcr_genesis_lr_cl_amd import build as b
    want = [s for s in args.sides.split(",") if s]
    res = dict(tool="train_cts_time", rounds=args.rounds, repeats=args.repeats, burst=args.burst, source_hash=b.source_hash(), tasks={})
    for task in [t for t in args.tasks.split(",") if t]:
        times, agree, shape = {}, {}, {}
        for _ in range(args.rounds):
            for side in want:                                    # a fresh process per side, the sides alternating
                cmd = [sys.executable, os.path.abspath(__file__), "--child", side, "--task", task, "--repeats", str(args.repeats), "--burst",
                       str(args.burst), "--warmup", str(args.warmup), "--teacher", str(args.teacher), "--student", str(args.student), "--critic", str(args.critic)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                line = next((l for l in r.stdout.splitlines() if l.startswith("CHILD ")), None)
                if r.returncode != 0 or line is None:
                    sys.exit(f"train_cts_time.py: the {task} {side} process failed (exit status {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                d = json.loads(line[6:])
                print(f"train_cts_time.py: {task} {side}: {len(d['us'][CUTS[-1]])} samples per cut", file=sys.stderr, flush=True)
                for cut in CUTS:
                    times.setdefault(side, {}).setdefault(cut, []).extend(d["us"][cut])
                agree[side], shape = d["agree"], dict(rows=d["rows"], floats=d["floats"])
        call_us = {s: {c: stat(v) for c, v in cuts.items()} for s, cuts in times.items()}
        print(f"{task} mini-batch: {shape['rows'][0]} teacher + {shape['rows'][1]} student + {shape['rows'][2]} critic rows, {shape['floats']} parameters")
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

"""Developer tool (GPU only, never read by bench.py): time of the PPO loss head of one mini-batch -- everything PPO._compute_rl_loss does
behind the network forward, forward plus backward to the gradients of mu, sigma and values -- at the go2 training sizes, three ways:

  (i)   fused:        `FusedPPOLoss` (csrc/lg_ppo.hip: the pass and its one-workgroup sum) and its backward (three scalings);
  (ii)  torch_eager:  the torch ops of rsl_rl/algorithms/ppo.py:157-218 (ppo_cts.py:193-267 for the two-group size) with autograd, eager;
  (iii) torch_graph:  the same ops, forward and backward, captured once and replayed as one HIP graph.

Sizes: `go2` is one mini-batch of GO2Cfg: B = num_envs * steps / mini_batches rows (num_envs and num_actions are read from
hcr_genesis_lr_cl_amd/config.py; --steps 24 and --mini-batches 4 are the reference's go2 runner settings, which config.py does not carry),
`go2_cts` the same rows split teacher : student as GO2CTSCfg.env.num_teacher : the rest, one value group over all of them.

Method: a fresh child process per side and round (the parent never opens the device), the sides alternating within every round; a child
first checks that its side agrees with the fused call on the same seeded inputs (loss to 1e-5 relative, gradients to 1e-6 absolute), warms
up, then takes --repeats samples per size, each the device-event time around a burst of --burst calls divided by the burst length: the
time per call on the device queue with the calls enqueued back to back.  Median and p10-p90 over all samples of a side are printed.

    python tools/ppo_loss_time.py [--rounds 3] [--repeats 20] [--burst 20] [--sides fused,torch_eager,torch_graph]

Prints a table and one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
SIDES = ("fused", "torch_eager", "torch_graph")
CLIP, VALUE_COEF, ENTROPY_COEF = 0.2, 1.0, 0.01


def sizes(steps, mini_batches):
    from hcr_genesis_lr_cl_amd.config import GO2Cfg, GO2CTSCfg
    n, A = int(GO2Cfg.env.num_envs), int(GO2Cfg.env.num_actions)
    B = n * steps // mini_batches
    teachers = B * int(GO2CTSCfg.env.num_teacher) // int(GO2CTSCfg.env.num_envs)
    return {"go2": dict(rows=[B], A=A), "go2_cts": dict(rows=[teachers, B - teachers], A=A)}


def make_inputs(size, dev, seed=1):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    groups = []
    for B in size["rows"]:
        mu, sigma = 0.5 * rn(B, size["A"]), 0.3 + 0.9 * torch.rand(B, size["A"], generator=g)
        old_mu, old_sigma = mu + 0.05 * sigma * rn(B, size["A"]), sigma * torch.exp(0.03 * rn(B, size["A"]))
        actions = old_mu + old_sigma * rn(B, size["A"])
        old_lp = (-(actions - old_mu) ** 2 / (2 * old_sigma ** 2) - old_sigma.log() - 0.9189385332046727).sum(-1, keepdim=True)
        groups.append(dict(mu=mu, sigma=sigma, actions=actions, old_log_prob=old_lp, advantages=rn(B, 1), old_mu=old_mu, old_sigma=old_sigma))
    Bv = sum(size["rows"])
    values = rn(Bv, 1)
    target = values + 0.25 * rn(Bv, 1)
    out = dict(groups=[{k: v.to(dev) for k, v in g.items()} for g in groups], values=values.to(dev), returns=(target + 0.5 * rn(Bv, 1)).to(dev),
               target_values=target.to(dev))
    for g in out["groups"]:
        g["mu"].requires_grad_()
        g["sigma"].requires_grad_()
    out["values"].requires_grad_()
    return out


def leaves(x):
    return [t for g in x["groups"] for t in (g["mu"], g["sigma"])] + [x["values"]]


def torch_loss(x):
    """ppo.py:157-218 / ppo_cts.py:193-267 behind the forward: (loss, kl of the first group)."""
    import torch
    surrogate, entropies, kl = [], [], None
    for i, g in enumerate(x["groups"]):
        mu, sigma = g["mu"], g["sigma"]
        logp = (-(g["actions"] - mu) ** 2 / (2 * sigma ** 2) - sigma.log() - 0.9189385332046727).sum(dim=-1)
        entropies.append((1.4189385332046727 + sigma.log()).sum(dim=-1))
        if i == 0:
            with torch.no_grad():
                kl = torch.sum(torch.log(sigma / g["old_sigma"] + 1.e-5) + (torch.square(g["old_sigma"]) + torch.square(g["old_mu"] - mu))
                               / (2.0 * torch.square(sigma)) - 0.5, axis=-1).mean()
        ratio = torch.exp(logp - torch.squeeze(g["old_log_prob"]))
        adv = torch.squeeze(g["advantages"])
        surrogate.append(torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP)).mean())
    v, R, vt = x["values"], x["returns"], x["target_values"]
    vc = vt + (v - vt).clamp(-CLIP, CLIP)
    value_loss = torch.max((v - R).pow(2), (vc - R).pow(2)).mean()
    entropy = (torch.cat(entropies, dim=0) if len(entropies) > 1 else entropies[0]).mean()
    return sum(surrogate) + VALUE_COEF * value_loss - ENTROPY_COEF * entropy, kl


def child(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("ppo_loss_time.py: no GPU -- a time is only measured on the device")
    from hcr_genesis_lr_cl_amd.ppo_loss import FusedPPOLoss
    dev = "cuda:0"
    loss_fn = FusedPPOLoss(CLIP, VALUE_COEF, ENTROPY_COEF)
    # Everything -- inputs, the agreement check, warm-up, capture, timing -- runs on ONE side stream.  Autograd ties the gradient sink of
    # a leaf to the stream of its first backward; a first backward on the default stream makes a later captured backward synchronise with
    # the default stream, which a capture cannot do (the runtime faulted on it).  So the default stream never sees these tensors, and the
    # graph is captured on the stream that warmed it up: one stream, no parallel branches.
    side_stream = torch.cuda.Stream()
    with torch.cuda.stream(side_stream):
        out = time_sizes(args, loss_fn, dev, side_stream)
    print("CHILD " + json.dumps(out))


def time_sizes(args, loss_fn, dev, side_stream):
    import torch
    out = {}
    for name, size in sizes(args.steps, args.mini_batches).items():
        x = make_inputs(size, dev)

        def fused():
            if len(x["groups"]) == 1:
                g = x["groups"][0]
                r = loss_fn(g["mu"], g["sigma"], x["values"], g["actions"], g["old_log_prob"], g["advantages"], x["returns"], x["target_values"],
                            g["old_mu"], g["old_sigma"])
            else:
                t, s = x["groups"]
                s = {k: v for k, v in s.items() if k not in ("old_mu", "old_sigma")}
                r = loss_fn.cts(teacher=t, student=s, values=x["values"], returns=x["returns"], target_values=x["target_values"])
            return r.loss, r.kl_mean, torch.autograd.grad(r.loss, leaves(x))

        def eager():
            loss, kl = torch_loss(x)
            return loss, kl, torch.autograd.grad(loss, leaves(x))

        a, b = fused(), eager()
        side_stream.synchronize()
        la, lb = a[0].detach().item(), b[0].detach().item()
        agree = dict(loss=abs(la - lb) / max(1.0, abs(lb)), kl=abs(float(a[1]) - float(b[1])),
                     grads=max(float((p - q).abs().max()) for p, q in zip(a[2], b[2])))
        if agree["loss"] > 1e-5 or agree["kl"] > 1e-5 or agree["grads"] > 1e-6:
            sys.exit(f"ppo_loss_time.py: {name}: the fused call and the torch ops disagree ({agree}) -- nothing timed")
        fn = fused if args.child == "fused" else eager
        if args.child == "torch_graph":
            for _ in range(3):
                eager()
            side_stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side_stream):
                kept = eager()              # noqa: F841  (the graph's outputs stay alive)
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
        out[name] = dict(rows=size["rows"], A=size["A"], agree=agree, us=[burst() for _ in range(args.repeats)])
    return out


def stat(v):
    s = sorted(v)
    return dict(median=statistics.median(v), min=s[0], max=s[-1], p10=s[len(s) // 10], p90=s[(9 * len(s)) // 10], samples=len(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=24, help="num_steps_per_env of the go2 runner")
    ap.add_argument("--mini-batches", type=int, default=4, help="num_mini_batches of the go2 runner")
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
                   "--warmup", str(args.warmup), "--steps", str(args.steps), "--mini-batches", str(args.mini_batches)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = next((l for l in r.stdout.splitlines() if l.startswith("CHILD ")), None)
            if r.returncode != 0 or line is None:
                sys.exit(f"ppo_loss_time.py: the {side} process failed (exit status {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            for name, d in json.loads(line[6:]).items():
                times.setdefault(name, {}).setdefault(side, []).extend(d["us"])
                agree[name], shape[name] = d["agree"], dict(rows=d["rows"], A=d["A"])
    res = dict(tool="ppo_loss_time", rounds=args.rounds, repeats=args.repeats, burst=args.burst, source_hash=b.source_hash(),
               sizes={n: dict(shape[n], max_abs_diff_vs_torch=agree[n], call_us={s: stat(v) for s, v in t.items()}) for n, t in times.items()})
    for name, d in res["sizes"].items():
        print(f"{name}: rows {d['rows']}, A = {d['A']}, fused against torch: loss {d['max_abs_diff_vs_torch']['loss']:.1e} (relative), "
              f"gradients {d['max_abs_diff_vs_torch']['grads']:.1e}")
        for s, v in d["call_us"].items():
            print(f"  {s:12s}: median {v['median']:8.1f} us   min {v['min']:8.1f}   p10-p90 {v['p10']:8.1f} - {v['p90']:8.1f}   max {v['max']:8.1f}   ({v['samples']} samples)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

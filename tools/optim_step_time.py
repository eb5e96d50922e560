"""Developer tool (GPU only, never read by bench.py): time of the optimizer block of one go2 mini-batch step -- what follows
loss.backward() in rsl_rl/algorithms/ppo.py:137-138, the gradient-norm clip and the Adam update -- on the parameter tensors of the
reference's ActorCritic for GO2Cfg (actor and critic num_observations -> 512 -> 256 -> 128 -> num_actions / 1, and std: 17 tensors),
five ways:

  (i)   fused:        `FusedAdam.step()` (csrc/lg_optim.hip: the norm launch and the update launch);
  (ii)  torch_eager:  nn.utils.clip_grad_norm_ + torch.optim.Adam, torch's defaults, eager;
  (iii) torch_fused:  the same with Adam(fused=True);
  (iv)  torch_graph:  (ii) with capturable=True, captured once on a single stream and replayed as one HIP graph;
  (v)   fused_graph:  the fused call captured once and replayed as one HIP graph.

The hidden sizes are the reference's go2 policy settings, which config.py does not carry (--hidden); num_observations and num_actions are
read from hcr_genesis_lr_cl_amd/config.py.

Method: a fresh child process per side and round (the parent never opens the device), the sides alternating within every round; a child
first checks that three steps of its side agree with three fused steps on the same seeded parameters and gradients (parameters to 1e-6
absolute), warms up, then takes --repeats samples, each the device-event time around a burst of --burst calls divided by the burst length:
the time per call on the device queue with the calls enqueued back to back.  Everything runs on one side stream.  Median and p10-p90 over
all samples of a side are printed.

    python tools/optim_step_time.py [--rounds 3] [--repeats 20] [--burst 20] [--sides fused,torch_eager,...]

Prints a table and one JSON line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
SIDES = ("fused", "torch_eager", "torch_fused", "torch_graph", "fused_graph")
LR, MAX_GRAD_NORM = 1e-3, 1.0


def shapes(hidden):
    from hcr_genesis_lr_cl_amd.config import GO2Cfg
    n_obs, A = int(GO2Cfg.env.num_observations), int(GO2Cfg.env.num_actions)
    out = [(A,)]                                                     # std
    for last in (A, 1):                                              # actor, critic
        widths = [n_obs, *hidden, last]
        for a, b in zip(widths[:-1], widths[1:]):
            out += [(b, a), (b,)]
    return out


def make(shapes_, dev, seed):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [(0.1 * torch.randn(*s, generator=g)).to(dev) for s in shapes_]


def child(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("optim_step_time.py: no GPU -- a time is only measured on the device")
    side_stream = torch.cuda.Stream()
    with torch.cuda.stream(side_stream):
        out = time_side(args, "cuda:0", side_stream)
    print("CHILD " + json.dumps(out))


def time_side(args, dev, side_stream):
    import torch
    from hcr_genesis_lr_cl_amd.optim import FusedAdam
    sh = shapes([int(h) for h in args.hidden.split(",")])
    grads = [make(sh, dev, 100 + s) for s in range(3)]                # total norm ~ 0.1 sqrt(377241) = 61: every step clips
    side = args.child

    def stepper(params):
        """The step function of this child's side over `params`, whose .grad tensors are static."""
        for p in params:
            p.grad = torch.zeros_like(p)
        if side.startswith("fused"):
            opt = FusedAdam(params, lr=LR, max_grad_norm=MAX_GRAD_NORM)
            return opt.step
        kw = dict(torch_eager={}, torch_fused=dict(fused=True), torch_graph=dict(capturable=True))[side]
        opt = torch.optim.Adam(params, lr=LR, **kw)

        def step():
            torch.nn.utils.clip_grad_norm_(params, MAX_GRAD_NORM)
            opt.step()
        return step

    def run3(step, params):
        for g in grads:
            for p, x in zip(params, g):
                p.grad.copy_(x)
            step()
        return [p.detach().clone() for p in params]

    def fresh():
        params = [p.requires_grad_() for p in make(sh, dev, 1)]
        return params, stepper(params)

    ref_params = make(sh, dev, 1)
    ref_opt = FusedAdam(ref_params, lr=LR, max_grad_norm=MAX_GRAD_NORM)
    for p in ref_params:
        p.grad = torch.zeros_like(p)
    want = run3(ref_opt.step, ref_params)
    params, step = fresh()
    fn = step
    if side.endswith("graph"):
        for p, x in zip(params, grads[0]):
            p.grad.copy_(x)
        if side == "torch_graph":                                     # torch's recipe: a few eager steps on the capture stream first
            for _ in range(3):
                step()
        side_stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side_stream):
            step()
        fn = graph.replay
    if side == "torch_graph":       # its optimizer has taken warm-up steps: the agreement is that of an eager capturable twin
        twin, twin_step = fresh()
        got = run3(twin_step, twin)
    else:                           # capturing runs nothing, so the fused graph itself starts where the fused call started
        got = run3(fn, params)
    side_stream.synchronize()
    agree = max(float((a - b).abs().max()) for a, b in zip(got, want))
    if not agree <= 1e-6:
        sys.exit(f"optim_step_time.py: {side}: three steps disagree with the fused call by {agree:.3e} -- nothing timed")

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
    return dict(tensors=len(sh), floats=sum(p.numel() for p in params), agree=agree, us=[burst() for _ in range(args.repeats)])


def stat(v):
    s = sorted(v)
    return dict(median=statistics.median(v), min=s[0], max=s[-1], p10=s[len(s) // 10], p90=s[(9 * len(s)) // 10], samples=len(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
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
                   "--warmup", str(args.warmup), "--hidden", args.hidden]
            r = subprocess.run(cmd, capture_output=True, text=True)
            line = next((l for l in r.stdout.splitlines() if l.startswith("CHILD ")), None)
            if r.returncode != 0 or line is None:
                sys.exit(f"optim_step_time.py: the {side} process failed (exit status {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            d = json.loads(line[6:])
            times.setdefault(side, []).extend(d["us"])
            agree[side], shape = d["agree"], dict(tensors=d["tensors"], floats=d["floats"])
    res = dict(tool="optim_step_time", rounds=args.rounds, repeats=args.repeats, burst=args.burst, source_hash=b.source_hash(), **shape,
               max_abs_diff_vs_fused=agree, call_us={s: stat(v) for s, v in times.items()})
    print(f"go2 ActorCritic: {shape['tensors']} tensors, {shape['floats']} floats")
    for s, v in res["call_us"].items():
        print(f"  {s:12s}: median {v['median']:8.1f} us   min {v['min']:8.1f}   p10-p90 {v['p10']:8.1f} - {v['p90']:8.1f}   max {v['max']:8.1f}   "
              f"({v['samples']} samples; parameters against fused after 3 steps: {agree[s]:.1e})")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

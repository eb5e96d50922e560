"""What the GPU files of the train passes (tests/test_gpu_train.py, tests/test_gpu_train_ee.py, tests/test_gpu_train_ts.py,
tests/test_gpu_train_edges.py) share, in one copy: moving arrays to and from the device, the bit comparison, the `_ragged` case rule, the
reference's PPO mini-batch steps in torch ops on the CPU, the per-step parameter-parity check, the capture / warm-up / replay driver and
the printer of the parity ratios.  Imported by those files only.  No test functions here."""
import copy

import numpy as np
import torch
import torch.nn as nn

from hcr_genesis_lr_cl_amd import ppo_loss
from tests import optim_cases as oc

DEV = torch.device("cuda")
COTANGENTS = ("grad_mu", "grad_sigma", "grad_values")
HALF_LOG_2PI = 0.9189385332046727          # a normal log-density's constant, as the reference writes it


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    return set(a) == set(b) and all(np.array_equal(np.asarray(a[k], np.float32).view(np.uint32), np.asarray(b[k], np.float32).view(np.uint32)) for k in a)


# ---- the cases of a parity table ----------------------------------------------------------------------------------------------------------------
def parity_cases(mod):
    return list(mod.CASES) + [f"{net}_ragged" for net in mod.RAGGED_SLICE_NETS]


def case_inputs(mod, name, seed_base, check=None):
    """make_inputs of a table case of the case module `mod`; `<net>_ragged`: the net at the smallest batch its plans slice raggedly,
    which lies within the tables' 257 rows and passes the file's own check(net, batch)."""
    if not name.endswith("_ragged"):
        return mod.make_inputs(name)
    net = name[:-len("_ragged")]
    b = mod.smallest_ragged_b(net)
    assert b <= 257
    if check is not None:
        check(net, b)
    return mod.make_inputs(dict(net=net, B=b, seed=seed_base + len(net)))


# ---- the reference's update in torch ops ------------------------------------------------------------------------------------------------------
def torch_rl_step(outputs, c, cfg):
    """(loss, KL) of the reference's PPO mini-batch step (ppo.py:157-218) from the module's (mu, sigma, value) and the columns `c`."""
    mu, sigma, value = outputs
    clip = cfg["clip_param"]
    logp = (-(c["actions"] - mu) ** 2 / (2 * sigma ** 2) - sigma.log() - HALF_LOG_2PI).sum(-1)
    with torch.no_grad():
        kl = torch.sum(torch.log(sigma / c["old_sigma"] + 1.e-5) + (c["old_sigma"] ** 2 + (c["old_mu"] - mu) ** 2) / (2.0 * sigma ** 2) - 0.5,
                       dim=-1).mean()
    ratio, adv = torch.exp(logp - c["old_log_prob"].squeeze(-1)), c["advantages"].squeeze(-1)
    surrogate = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)).mean()
    vc = c["target_values"] + (value - c["target_values"]).clamp(-clip, clip)
    value_loss = torch.max((value - c["returns"]).pow(2), (vc - c["returns"]).pow(2)).mean()
    entropy = (1.4189385332046727 + sigma.log()).sum(-1).mean()
    return surrogate + cfg["value_loss_coef"] * value_loss - cfg["entropy_coef"] * entropy, kl


def torch_rl_update(fx, columns, forward, params, snap, dtype):
    """The RL mini-batch steps of the reference's update on the fixture's columns (rounded to float32 first) in torch ops of `dtype` on the
    CPU: forward(columns of a step) -> (mu, sigma, value), the loss of torch_rl_step, the host rate rule and its three lines, Adam on
    `params` behind the norm clip.  Returns (snap() after every step, the rates)."""
    cfg = fx["cfg"]
    opt = torch.optim.Adam(params, lr=cfg["lr0"], betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"])
    lr, lrs, out = cfg["lr0"], [], []
    for s in range(cfg["steps"]):
        c = {k: torch.from_numpy(np.asarray(fx[k][s], np.float32)).to(dtype) for k in columns}
        loss, kl = torch_rl_step(forward(c), c, cfg)
        lr = ppo_loss.adjust_learning_rate(kl, lr, cfg["desired_kl"])
        for group in opt.param_groups:
            group["lr"] = lr
        opt.zero_grad()
        loss.backward()
        nn.utils.clip_grad_norm_(params, cfg["max_grad_norm"])
        opt.step()
        lrs.append(lr)
        out.append(snap())
    return out, lrs


def check_parameters(got, ref64, ref32, s, report):
    """Every parameter (dicts by name) after step s against the parity rule of tests/optim_cases.py; prints the worst ratio first."""
    worst, bad = 0.0, []
    for name, r64 in ref64.items():
        err, bound = oc.max_err(got[name], r64), oc.parity_bound(oc.max_err(ref32[name], r64), r64)
        worst = max(worst, err / (bound / oc.PARITY_FACTOR))
        if not err <= bound:
            bad.append((name, err, bound))
    print(f"fixture step {s}: worst parameter ratio {worst:.3f} (allowed {oc.PARITY_FACTOR:g})")
    report.append((f"fixture step {s}", dict(parameters=worst)))
    assert not bad, (s, bad)


def fixture_batches(fx, columns, steps):
    return [{k: dev(fx[k][s]) for k in columns} for s in range(steps)]


# ---- one update as a HIP graph ------------------------------------------------------------------------------------------------------------------
def replays_like_eager_steps(module, learner, batches):
    """learner(m).step(batch) captured on one stream as a HIP graph and replayed once per batch, the batch rewritten in place in between:
    every parameter, the first optimizer's rate and every optimizer's step count are those of the eager steps, bit for bit.  module():
    a fresh module on the device; learner(m): an object with step(batch) and .optimizers."""
    eager = module()
    le = learner(eager)
    for b in batches:
        le.step(b)
    torch.cuda.synchronize()

    m = module()
    static = {k: torch.zeros_like(v) for k, v in batches[0].items()}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):                                   # warm-up on the side stream, on a module of its own
        learner(copy.deepcopy(m)).step(batches[0])
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    lg = learner(m)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        lg.step(static)
    torch.cuda.synchronize()
    assert all(o.step_count == 0 for o in lg.optimizers)              # capturing runs nothing
    for b in batches:
        for k, v in b.items():
            static[k].copy_(v)
        graph.replay()
    torch.cuda.synchronize()
    assert all(o.step_count == len(batches) for o in lg.optimizers) and lg.optimizers[0].lr == le.optimizers[0].lr
    for (n, a), b in zip(m.named_parameters(), eager.parameters()):
        assert np.array_equal(host(a).view(np.uint32), host(b).view(np.uint32)), n


def print_parity_ratios(report):
    """The worst |kernel - f64| / max(|torch-f32 - f64|, ulp) per tensor class over every parity check of a file, for DESIGN.md's table."""
    worst = {}
    for _, ratios in report:
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for k, v in worst.items():
        print(f"PARITY {k}: {v:.3f} over {len(report)} checks")

"""The fused optimizer step on the GPU (hcr_genesis_lr_cl_amd/optim.py, csrc/lg_optim.hip) against the float64 restatement of
tests/optim_cases.py, which tests/test_optim_host.py pins to the reference's own PPO.update() and to clip_grad_norm_ + torch.optim.Adam:
parity of every parameter and moment on the case table and on the golden fixture's six steps, bit-reproducibility, the workspace, the
learning-rate cell, gradients left alone, None gradients, NaN and inf, checkpoints to and from torch.optim.Adam, graph capture, and the
loss head and the optimizer end to end."""
import copy
import os
import struct

import numpy as np
import pytest
import torch
import torch.nn as nn

from hcr_genesis_lr_cl_amd import abi, optim, ppo_loss
from tests import optim_cases as oc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ppo_update.npz")
DEV = "cuda:0"


def at_offset(x, off=1):
    """The float32 numpy array on the device as a view `off` floats into a larger storage: misaligned for 16-byte access."""
    store = torch.zeros(x.size + off, device=DEV)
    store[off:].copy_(torch.from_numpy(np.ascontiguousarray(x).reshape(-1)))
    return store[off:].view(x.shape)


def device_params(params, view=False):
    return [at_offset(x) if view and i == 0 else torch.from_numpy(x).to(DEV) for i, x in enumerate(params)]


def set_grads(ps, grads, view=False):
    for i, (p, g) in enumerate(zip(ps, grads)):
        p.grad = None if g is None else (at_offset(g) if view and i == 0 else torch.from_numpy(np.ascontiguousarray(g)).to(DEV))


def snapshot(opt):
    torch.cuda.synchronize()
    n = lambda ts: [t.detach().cpu().numpy().astype(np.float64).reshape(-1) for t in ts]
    return dict(params=n(opt.params), exp_avg=n(opt.exp_avg), exp_avg_sq=n(opt.exp_avg_sq))


def bits(opt):
    torch.cuda.synchronize()
    return [t.detach().cpu().numpy().copy().view(np.uint32) for ts in (opt.params, opt.exp_avg, opt.exp_avg_sq) for t in ts] + \
        [opt._state.cpu().numpy().copy().view(np.uint64)]


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def run_fused(params, grads_per_step, view=False, kls=None, **kw):
    """A fresh FusedAdam over device copies of `params`, one step per entry of grads_per_step.  Returns (optimizer, result vector of
    every step as numpy)."""
    ps = device_params(params, view)
    opt = optim.FusedAdam(ps, **kw)
    results = []
    for s, grads in enumerate(grads_per_step):
        set_grads(ps, grads, view)
        info = opt.step(kl_mean=None if kls is None else torch.tensor(kls[s], dtype=torch.float32, device=DEV))
        results.append(info.result.clone())
    torch.cuda.synchronize()
    return opt, [r.cpu().numpy() for r in results]


_CACHE = {}


def case_data(name, scale):
    """Inputs and both restatements (every step) of a table case at a gradient scale, computed once and shared."""
    if (name, scale) not in _CACHE:
        h = oc.hyper(name)
        kw = dict(lr0=h["lr"], betas=h["betas"], eps=h["eps"], max_grad_norm=h["max_grad_norm"])
        params, grads = oc.make_inputs(name, scale)
        _CACHE[name, scale] = (params, grads, oc.restate(params, grads, **kw), oc.restate(params, grads, dtype=torch.float32, **kw))
    return _CACHE[name, scale]


RATIOS = []      # (label, worst ratio at factor 1) of every parity check of this module, printed by the last test


# ---- parity -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oc.CASES))
def test_parity_on_the_table(name):
    c, h = oc.CASES[name], oc.hyper(name)
    for label, scale in oc.SCALES.items():
        params, grads, ref64, ref32 = case_data(name, scale)
        for steps in c.get("steps", oc.STEPS):
            opt, results = run_fused(params, grads[:steps], view=c.get("view", False), lr=h["lr"], betas=h["betas"], eps=h["eps"],
                                     max_grad_norm=h["max_grad_norm"])
            if c.get("view"):
                assert all(t.data_ptr() % 16 == 4 for t in (opt.params[0], opt.params[0].grad, opt.exp_avg[0], opt.exp_avg_sq[0]))
            for s, r in enumerate(results):                           # the result vector of every step
                want = ref64[s]
                assert abs(r[abi.ADAM_R_GRAD_NORM] - want["grad_norm"]) <= 2.0 ** -23 * want["grad_norm"], (label, s)
                assert abs(r[abi.ADAM_R_CLIP_COEF] - want["clip_coef"]) <= 4 * 2.0 ** -24 * want["clip_coef"], (label, s)
                assert (r[abi.ADAM_R_CLIP_COEF] == 1.0) == (want["grad_norm"] <= h["max_grad_norm"])
                assert r[abi.ADAM_R_LR] == np.float32(h["lr"]) and r[abi.ADAM_R_STEP] == s + 1
            oc.check_parity(snapshot(opt), ref64[steps - 1], ref32[steps - 1], f"{name} {label} {steps} step(s)", RATIOS)


@pytest.fixture(scope="module")
def fixture():
    return oc.load_fixture(FIXTURE)


def test_fixture_steps_with_the_device_rate_rule(fixture):
    """The six steps of the reference's PPO.update(): its float64 gradients rounded to float32, the rate rule on the device fed by its
    KLs as float32.  The learning rates are the fixture's exactly; the parameters lie within the parity rule of the float64 restatement
    of the same float32 inputs."""
    cfg = fixture["cfg"]
    f32 = lambda xs: [np.asarray(x, np.float32) for x in xs]
    params, grads, kls = f32(fixture["init"]), [f32(g) for g in fixture["grads"]], [np.float32(k) for k in fixture["kl"]]
    kw = dict(lr0=cfg["lr0"], kls=[float(k) for k in kls], betas=cfg["betas"], eps=cfg["eps"], max_grad_norm=cfg["max_grad_norm"],
              desired_kl=cfg["desired_kl"])
    ref64, ref32 = oc.restate(params, grads, **kw), oc.restate(params, grads, dtype=torch.float32, **kw)
    ps = device_params(params)
    opt = optim.FusedAdam(ps, lr=cfg["lr0"], betas=cfg["betas"], eps=cfg["eps"], max_grad_norm=cfg["max_grad_norm"], desired_kl=cfg["desired_kl"])
    for s in range(cfg["steps"]):
        set_grads(ps, grads[s])
        info = opt.step(kl_mean=torch.tensor(kls[s], device=DEV))
        assert struct.pack("d", opt.lr) == struct.pack("d", float(fixture["lr"][s])), (s, opt.lr, fixture["lr"][s])
        assert info.lr.item() == np.float32(fixture["lr"][s]) and info.step.item() == s + 1
        assert (info.clip_coef.item() < 1.0) == (fixture["grad_norm"][s] > cfg["max_grad_norm"])
        oc.check_parity(snapshot(opt), ref64[s], ref32[s], f"fixture step {s}", RATIOS)
    # and the float64 restatement of the float32 inputs is the reference's own result up to the rounding of those inputs
    assert max(np.abs(x - y).max() for x, y in zip(ref64[-1]["params"], fixture["params"][-1])) < 1e-5


# ---- reproducibility and the workspace -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t64_ragged", "two_sweeps"])
def test_two_fresh_optimizers_give_identical_bits(name):
    params, grads, _, _ = case_data(name, 1.0)
    grads = [grads[s % len(grads)] for s in range(3)]
    a, ra = run_fused(params, grads)
    b, rb = run_fused(params, grads)
    assert same_bits(bits(a), bits(b)) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(ra, rb))
    assert a.step_count == 3


def test_slab_and_result_are_written_before_they_are_read():
    """The slab and the result vector filled with NaN, the slab 64 doubles larger than the plan: the bits of a clean call, and the extra
    64 untouched."""
    params, grads, _, _ = case_data("t64_ragged", 1.0)
    clean, rc = run_fused(params, grads[:2])
    ps = device_params(params)
    opt = optim.FusedAdam(ps)
    need = optim.workspace_doubles([p.numel() for p in ps])
    assert opt._partials.numel() == need
    opt._partials = torch.full((need + 64,), float("nan"), dtype=torch.float64, device=DEV)
    opt._result.fill_(float("nan"))
    results = []
    for g in grads[:2]:
        set_grads(ps, g)
        results.append(opt.step().result.clone())
    assert same_bits(bits(opt), bits(clean))
    assert all(np.array_equal(r.cpu().numpy().view(np.uint32), c.view(np.uint32)) for r, c in zip(results, rc))
    slab = opt._partials.cpu().numpy()
    assert np.isnan(slab[need:]).all() and np.isfinite(slab[:need]).all()


# ---- the cell ------------------------------------------------------------------------------------------------------------------------------
def test_rate_cell_follows_the_host_rule_bit_for_bit():
    """The tie table of the host test through step(kl_mean=...): opt.lr is the host rule's double, info.step counts up."""
    want = oc.tie_expected(ppo_loss.adjust_learning_rate)
    p = torch.ones(5, device=DEV)
    opt = optim.FusedAdam([p], lr=1e-3, desired_kl=oc.TIE_DESIRED_KL)
    for i, ((kl, lr0), lr) in enumerate(zip(oc.tie_table(), want)):
        if lr0 is not None:
            opt.set_lr(lr0)
        p.grad = torch.full((5,), 0.25, device=DEV)
        info = opt.step(kl_mean=torch.tensor(kl, device=DEV))
        assert struct.pack("d", opt.lr) == struct.pack("d", lr), (i, float(kl), opt.lr, lr)
        assert info.step.item() == i + 1 and info.lr.item() == np.float32(lr) and opt.step_count == i + 1
    before = opt.lr
    p.grad = torch.full((5,), 0.25, device=DEV)
    opt.step()                                                        # without kl_mean the rate stays
    assert opt.lr == before and opt.step_count == len(want) + 1
    with pytest.raises(ValueError, match="kl_mean was given, but the optimizer has no desired_kl"):
        optim.FusedAdam([p]).step(kl_mean=torch.tensor(0.01, device=DEV))


def test_gradients_are_not_written():
    params, grads, ref64, _ = case_data("tiny_actor", 30.0)
    ps = device_params(params)
    opt = optim.FusedAdam(ps)
    set_grads(ps, grads[0])
    before = [p.grad.clone() for p in ps]
    info = opt.step()
    assert info.clip_coef.item() < 0.1                                # a clipped step
    assert all(torch.equal(p.grad.view(torch.int32), g.view(torch.int32)) for p, g in zip(ps, before))


def test_a_none_gradient_leaves_its_parameter_out():
    params, grads, _, _ = case_data("tiny_actor", 1.0)
    with_none = [[None if i == 2 else g for i, g in enumerate(gs)] for gs in grads[:3]]
    a, _ = run_fused(params, with_none)
    b, _ = run_fused(params[:2] + params[3:], [gs[:2] + gs[3:] for gs in grads[:3]])
    torch.cuda.synchronize()
    assert np.array_equal(a.params[2].cpu().numpy().view(np.uint32), params[2].view(np.uint32))
    assert not a.exp_avg[2].any().item() and not a.exp_avg_sq[2].any().item()
    for mine, other in ((a.params, b.params), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq)):
        for x, y in zip(mine[:2] + mine[3:], other):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # no gradient at all: nothing is launched, the step count stays
    ps = device_params(params)
    opt = optim.FusedAdam(ps)
    info = opt.step()
    torch.cuda.synchronize()
    assert opt.step_count == 0 and info.step.item() == 0 and all(np.array_equal(p.cpu().numpy(), x) for p, x in zip(ps, params))
    opt.zero_grad()
    set_grads(ps, grads[0])
    opt.step()
    opt.zero_grad()
    assert all(p.grad is None for p in ps) and opt.step_count == 1


# ---- NaN is not silent --------------------------------------------------------------------------------------------------------------------
def test_one_nan_gradient_reaches_everything():
    params, grads, _, _ = case_data("tiny_actor", 1.0)
    g = [x.copy() for x in grads[0]]
    g[2][-1] = np.nan                                                 # a middle tensor's ragged tail (128 floats: the 4-byte path)
    opt, results = run_fused(params, [g])
    snap = snapshot(opt)
    assert all(np.isnan(x).all() for field in oc.FIELDS for x in snap[field])
    assert np.isnan(results[0][abi.ADAM_R_GRAD_NORM]) and np.isnan(results[0][abi.ADAM_R_CLIP_COEF])
    assert results[0][abi.ADAM_R_STEP] == 1 and results[0][abi.ADAM_R_LR] == np.float32(1e-3)
    assert all(np.array_equal(p.grad.cpu().numpy(), x, equal_nan=True) for p, x in zip(opt.params, g))


def test_one_inf_gradient_has_torchs_pattern():
    """total = inf, coef = 0: inf * 0 = NaN in that element, zero moments and an unmoved parameter elsewhere -- element by element the
    pattern of clip_grad_norm_ + torch.optim.Adam in float32 on the CPU."""
    params, grads, _, _ = case_data("t64_ragged", 1.0)
    g = [x.copy() for x in grads[0]]
    where = max(range(len(g)), key=lambda i: g[i].size)               # a tensor with a whole chunk (the 16-byte path) and a tail
    assert g[where].size > abi.ADAM_CHUNK
    g[where][7] = np.inf
    opt, results = run_fused(params, [g])
    want = oc.torch_reference(params, [g], dtype=torch.float32)[0]
    snap = snapshot(opt)
    assert np.isinf(results[0][abi.ADAM_R_GRAD_NORM]) and results[0][abi.ADAM_R_CLIP_COEF] == 0.0
    n_nan = 0
    for field in oc.FIELDS:
        for x, y in zip(snap[field], want[field]):
            y = y.reshape(-1)
            assert np.array_equal(np.isnan(x), np.isnan(y)) and np.array_equal(x == 0, y == 0) and np.array_equal(np.isfinite(x), np.isfinite(y))
            assert np.array_equal(x[np.isfinite(x)], y[np.isfinite(y)])          # coef = 0: nothing else moved, on either side
            n_nan += int(np.isnan(x).sum())
    assert n_nan == 3                                                 # that element of the parameter and of both moments


# ---- checkpoints ------------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_with_torch_adam():
    """2 fused steps -> state_dict -> (torch.optim.Adam on the device, 2 torch steps) and (a fresh FusedAdam, 2 fused steps): both within
    the parity rule of the float64 restatement of all four steps, and the reloaded fused run is the uninterrupted one bit for bit."""
    params, grads, ref64, ref32 = case_data("tiny_actor", 1.0)
    first, _ = run_fused(params, grads[:2])
    sd = first.state_dict()
    assert sd["state"][0]["step"].item() == 2.0 and sd["param_groups"][0]["lr"] == 1e-3 and len(sd["state"]) == len(params)
    start = [p.detach().clone() for p in first.params]

    ps = [nn.Parameter(p.clone()) for p in start]
    adam = torch.optim.Adam(ps, lr=5e-4)                              # lr, betas and eps come from the checkpoint
    adam.load_state_dict(copy.deepcopy(sd))                           # torch keeps the step tensors it is handed and counts in them
    assert adam.param_groups[0]["lr"] == 1e-3
    for gs in grads[2:4]:
        set_grads(ps, gs)
        torch.nn.utils.clip_grad_norm_(ps, 1.0)
        adam.step()
    torch.cuda.synchronize()
    n = lambda ts: [t.detach().cpu().numpy().astype(np.float64).reshape(-1) for t in ts]
    torch_side = dict(params=n(ps), exp_avg=n([adam.state[p]["exp_avg"] for p in ps]), exp_avg_sq=n([adam.state[p]["exp_avg_sq"] for p in ps]))
    oc.check_parity(torch_side, ref64[3], ref32[3], "checkpoint -> torch.optim.Adam", RATIOS)

    qs = [p.clone() for p in start]
    again = optim.FusedAdam(qs, lr=5e-4)
    again.load_state_dict(sd)
    assert again.lr == 1e-3 and again.step_count == 2
    for gs in grads[2:4]:
        set_grads(qs, gs)
        again.step()
    oc.check_parity(snapshot(again), ref64[3], ref32[3], "checkpoint -> FusedAdam", RATIOS)
    straight, _ = run_fused(params, grads[:4])
    assert same_bits(bits(again), bits(straight))

    back = optim.FusedAdam([p.detach().clone() for p in ps])          # and torch's checkpoint loads here
    back.load_state_dict(adam.state_dict())
    assert back.step_count == 4 and back.lr == 1e-3
    assert all(torch.equal(m, adam.state[p]["exp_avg"]) for m, p in zip(back.exp_avg, ps))
    bad = copy.deepcopy(adam.state_dict())
    bad["state"][1]["step"] = torch.tensor(3.0)
    with pytest.raises(ValueError, match="step counts differ"):
        back.load_state_dict(bad)


# ---- graph capture ----------------------------------------------------------------------------------------------------------------------------
def test_captured_step_replays_like_eager_calls():
    """One opt.step(kl_mean=kl) captured on one side stream (no parallel branches), replayed three times with the gradients and the KL
    rewritten in place in between: parameters, moments, rate and step count are those of three eager calls bit for bit -- nothing of the
    step lives on the host."""
    params, grads, _, _ = case_data("tiny_actor", 1.0)
    kls = [np.float32(0.001), np.float32(0.05), np.float32(0.01)]     # rises, falls, stays at desired_kl = 0.01
    eager, eager_results = run_fused(params, grads[:3], kls=kls, desired_kl=0.01)
    assert eager_results[0][abi.ADAM_R_LR] > eager_results[1][abi.ADAM_R_LR] == eager_results[2][abi.ADAM_R_LR]

    ps = device_params(params)
    opt = optim.FusedAdam(ps, desired_kl=0.01)
    static_grads = [torch.zeros_like(p) for p in ps]
    for p, g in zip(ps, static_grads):
        p.grad = g
    kl = torch.zeros((), device=DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):                                   # warm-up on the side stream, on an optimizer of its own
        warm = optim.FusedAdam([p.clone() for p in ps], desired_kl=0.01)
        for p in warm.params:
            p.grad = torch.ones_like(p)
        warm.step(kl_mean=kl)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        info = opt.step(kl_mean=kl)
    torch.cuda.synchronize()
    assert opt.step_count == 0                                        # capturing runs nothing
    for s in range(3):
        for g, x in zip(static_grads, grads[s]):
            g.copy_(torch.from_numpy(x).to(DEV))
        kl.fill_(float(kls[s]))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(info.result.cpu().numpy().view(np.uint32), eager_results[s].view(np.uint32)), s
    assert same_bits(bits(opt), bits(eager)) and opt.step_count == 3


# ---- the loss head and the optimizer together ---------------------------------------------------------------------------------------------------
class TinyActorCritic(nn.Module):
    def __init__(self, n_obs=7, n_actions=3):
        super().__init__()
        self.std = nn.Parameter(0.8 * torch.ones(n_actions))
        self.actor = nn.Sequential(nn.Linear(n_obs, 16), nn.ELU(), nn.Linear(16, 8), nn.ELU(), nn.Linear(8, n_actions))
        self.critic = nn.Sequential(nn.Linear(n_obs, 16), nn.ELU(), nn.Linear(16, 8), nn.ELU(), nn.Linear(8, 1))


def _torch_update(model, batches, dtype, desired_kl, lr0=1e-3, clip=0.2, max_grad_norm=1.0):
    """The reference's mini-batch step in torch ops of `dtype` on the CPU: the loss of ppo.py:157-218, the host rate rule, and its three
    lines.  Returns (parameters as float64 numpy, learning rates, KLs)."""
    model = model.to(dtype)
    opt = torch.optim.Adam(model.parameters(), lr=lr0)
    lr, lrs, kls = lr0, [], []
    for b in batches:
        t = {k: torch.from_numpy(v).to(dtype) for k, v in b.items()}
        mu, value = model.actor(t["obs"]), model.critic(t["obs"])
        sigma = mu * 0.0 + model.std
        logp = (-(t["actions"] - mu) ** 2 / (2 * sigma ** 2) - sigma.log() - 0.9189385332046727).sum(-1)
        with torch.no_grad():
            kl = torch.sum(torch.log(sigma / t["old_sigma"] + 1.e-5) + (t["old_sigma"] ** 2 + (t["old_mu"] - mu) ** 2) / (2.0 * sigma ** 2) - 0.5,
                           dim=-1).mean()
        lr = ppo_loss.adjust_learning_rate(kl, lr, desired_kl)
        for group in opt.param_groups:
            group["lr"] = lr
        ratio = torch.exp(logp - t["old_log_prob"].squeeze(-1))
        adv = t["advantages"].squeeze(-1)
        surrogate = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)).mean()
        vc = t["target_values"] + (value - t["target_values"]).clamp(-clip, clip)
        value_loss = torch.max((value - t["returns"]).pow(2), (vc - t["returns"]).pow(2)).mean()
        entropy = (1.4189385332046727 + sigma.log()).sum(-1).mean()
        loss = surrogate + 1.0 * value_loss - 0.01 * entropy
        opt.zero_grad()
        loss.backward()
        nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)
        opt.step()
        lrs.append(lr)
        kls.append(float(kl))
    return [p.detach().double().numpy().reshape(-1).copy() for p in model.parameters()], lrs, kls


def test_loss_head_and_optimizer_end_to_end():
    """FusedPPOLoss -> backward() -> FusedAdam.step(kl_mean=out.kl_mean) for 3 mini-batches against a float64 copy of the module that runs
    the reference's three lines and the host rate rule: the parameters within the parity rule (its float32 side: the same torch code in
    float32 on the CPU), the learning-rate sequences equal."""
    torch.manual_seed(7)
    rng = np.random.default_rng(7)
    model = TinyActorCritic()
    B, A, desired_kl = 96, 3, 0.02
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    batches = []
    for pert in (0.05, 0.2, 0.1):                                  # how far the stored distribution lies from the network's: the KL
        obs = f(rng.normal(size=(B, 7)))
        with torch.no_grad():
            mu = model.actor(torch.from_numpy(obs)).numpy()
        old_mu, old_sigma = f(mu + pert * rng.normal(size=(B, A))), f(0.8 * np.exp(0.03 * rng.normal(size=(B, A))))
        actions = f(old_mu + old_sigma * rng.normal(size=(B, A)))
        old_lp = f((-(actions - old_mu) ** 2 / (2 * old_sigma ** 2) - np.log(old_sigma) - 0.9189385332046727).sum(-1, keepdims=True))
        target = f(rng.normal(size=(B, 1)))
        batches.append(dict(obs=obs, actions=actions, old_mu=old_mu, old_sigma=old_sigma, old_log_prob=old_lp, advantages=f(rng.normal(size=(B, 1))),
                            target_values=target, returns=f(target + 0.5 * rng.normal(size=(B, 1)))))
    ref64, lrs64, kls64 = _torch_update(copy.deepcopy(model), batches, torch.float64, desired_kl)
    ref32, lrs32, _ = _torch_update(copy.deepcopy(model), batches, torch.float32, desired_kl)
    # the inputs' own property: every KL at least 5 % from a threshold of the rule, and the rate moves
    assert all(abs(k / (2 * desired_kl) - 1) > 0.05 and abs(k / (desired_kl / 2) - 1) > 0.05 and k > 0 for k in kls64), kls64
    assert lrs64 == lrs32 and len(set(lrs64)) > 1, (lrs64, kls64)

    gpu = copy.deepcopy(model).to(DEV)
    loss_fn = ppo_loss.FusedPPOLoss(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01)
    opt = optim.FusedAdam(gpu.named_parameters(), lr=1e-3, max_grad_norm=1.0, desired_kl=desired_kl)
    assert opt.names[0] == "std"
    lrs = []
    for b in batches:
        t = {k: torch.from_numpy(v).to(DEV) for k, v in b.items()}
        mu, value = gpu.actor(t["obs"]), gpu.critic(t["obs"])
        sigma = mu * 0.0 + gpu.std
        out = loss_fn(mu, sigma, value, t["actions"], t["old_log_prob"], t["advantages"], t["returns"], t["target_values"], t["old_mu"], t["old_sigma"])
        opt.zero_grad()
        out.loss.backward()
        opt.step(kl_mean=out.kl_mean)
        lrs.append(opt.lr)
    assert lrs == lrs64, (lrs, lrs64, kls64)
    got = [p.detach().cpu().numpy().astype(np.float64).reshape(-1) for p in gpu.parameters()]
    worst, bad = 0.0, []
    for name, x, r64, r32 in zip(opt.names, got, ref64, ref32):
        err, bound = oc.max_err(x, r64), oc.parity_bound(oc.max_err(r32, r64), r64)
        worst = max(worst, err / (bound / oc.PARITY_FACTOR))
        print(f"end to end {name}: |kernel - f64| {err:.3e}, torch-f32 {oc.max_err(r32, r64):.3e}, bound {bound:.3e}")
        if not err <= bound:
            bad.append((name, err, bound))
    RATIOS.append(("end to end", worst))
    assert not bad, bad


def test_zz_print_the_parity_ratios():
    """Not a check of its own: the worst |kernel - f64| / max(|torch-f32 - f64|, ulp) of every parity check above, for DESIGN.md's table."""
    for label, ratio in RATIOS:
        print(f"PARITY {label}: {ratio:.3f}")
    assert all(r <= oc.PARITY_FACTOR for _, r in RATIOS)

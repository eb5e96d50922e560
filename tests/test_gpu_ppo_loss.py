"""The fused PPO loss head on the GPU (hcr_genesis_lr_cl_amd/ppo_loss.py, csrc/lg_ppo.hip) against the float64 restatement of
tests/ppo_loss_cases.py, which tests/test_ppo_loss_host.py pins to the reference's own classes: parity of every scalar and gradient on
the case table and on the golden fixture's rows, the autograd connection, bit-reproducibility, NaN rows, strided views and graph capture."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from hcr_genesis_lr_cl_amd import abi, ppo_loss
from tests import ppo_loss_cases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ppo_loss.npz")
DEV = "cuda:0"
SENTINEL = -12345.0


def to_device(inp, put=None):
    """The numpy inputs as device tensors; `put(array, name)` places one array (default: a contiguous tensor)."""
    put = put or (lambda x, name: torch.from_numpy(x).to(DEV))
    return dict(groups=[{k: None if v is None else put(v, k) for k, v in g.items()} for g in inp["groups"]],
                **{k: put(inp[k], k) for k in ("values", "returns", "target_values")})


def run(dev, clipped, spo, ent, clip=pc.CLIP, value_loss_coef=1.0, out=None):
    """One lg_ppo_loss call on device tensors; `out` may bring its own output tensors.  Returns (restate-shaped numpy result, raw tensors)."""
    groups = []
    out = out or {}
    for gi, g in enumerate(dev["groups"]):
        groups.append(dict(g, grad_mu=out.get(f"grad_mu{gi}", torch.empty_like(g["mu"].contiguous())),
                           grad_sigma=out.get(f"grad_sigma{gi}", torch.empty_like(g["mu"].contiguous()))))
    rows, vrows, A = [g["mu"].shape[0] for g in groups], dev["values"].shape[0], groups[0]["mu"].shape[1]
    grad_values = out.get("grad_values", torch.empty(vrows, 1, device=DEV))
    partials = out.get("partials", torch.empty(ppo_loss.workspace_doubles(rows, vrows, A), dtype=torch.float64, device=DEV))
    result = out.get("result", torch.full((abi.PPO_RESULT_FLOATS,), float("nan"), device=DEV))
    flags = (abi.PPO_CLIPPED_VALUE if clipped else 0) | (abi.PPO_SPO if spo else 0)
    args = ppo_loss.ppo_loss_args(groups, dev["values"], dev["returns"], dev["target_values"], grad_values, partials, result, clip,
                                  value_loss_coef, ent, flags)
    ppo_loss.launch(args, torch.device(DEV))
    raw = dict(result=result, grad_values=grad_values, grad_mu=[g["grad_mu"] for g in groups], grad_sigma=[g["grad_sigma"] for g in groups])
    return collect(raw, [g["old_mu"] is not None for g in groups]), raw


def collect(raw, has_kl):
    torch.cuda.synchronize()
    r = raw["result"].cpu().numpy().astype(np.float64)
    n = lambda t: t.cpu().numpy().astype(np.float64)
    gs = range(len(has_kl))
    return dict(loss=r[abi.PPO_R_LOSS], surrogate=[r[abi.PPO_R_SURROGATE + g] for g in gs], value_loss=r[abi.PPO_R_VALUE],
                entropy=r[abi.PPO_R_ENTROPY], kl=[r[abi.PPO_R_KL + g] if has_kl[g] else None for g in gs],
                grad_mu=[n(raw["grad_mu"][g]) for g in gs], grad_sigma=[n(raw["grad_sigma"][g]) for g in gs], grad_values=n(raw["grad_values"]))


def same_bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for (_, x), (_, y) in zip(pc.outputs(a), pc.outputs(b)))


_CACHE = {}


def case_data(name):
    """Inputs and both restatements of a table case, computed once and shared by every test that needs them."""
    if name not in _CACHE:
        inp = pc.make_inputs(name)
        _CACHE[name] = (inp, pc.restate_case(name, inp), pc.restate_case(name, inp, dtype=torch.float32))
    return _CACHE[name]


def cfg_of(name):
    c = pc.CASES[name]
    return dict(clipped=c["clipped"], spo=c["spo"], ent=c["ent"])


# ---- parity -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pc.CASES))
def test_parity_on_the_table(name):
    inp, ref64, ref32 = case_data(name)
    got, raw = run(to_device(inp), **cfg_of(name))
    assert raw["result"][7].item() == 0.0 and all(raw["result"][abi.PPO_R_KL + g].item() == 0.0
                                                   for g, kl in enumerate(pc.CASES[name]["kl"]) if not kl)
    if len(pc.CASES[name]["rows"]) == 1:
        assert raw["result"][abi.PPO_R_SURROGATE + 1].item() == 0.0 and raw["result"][abi.PPO_R_KL + 1].item() == 0.0
    pc.check_parity(got, ref64, ref32, name)


def test_parity_on_the_fixture_rows():
    """The golden fixture's cases (network outputs of the reference's own classes, rounded to float32) through the kernel."""
    for name, c in pc.load_fixture(FIXTURE).items():
        inp = pc.as_float32(c["inp"])
        ref64, ref32 = pc.restate(inp, **c["cfg"]), pc.restate(inp, dtype=torch.float32, **c["cfg"])
        got, _ = run(to_device(inp), **c["cfg"])
        pc.check_parity(got, ref64, ref32, "fixture " + name)
        # and the reference's own float64 numbers, which saw the unrounded network outputs: a float32 rounding of mu / sigma / values away
        assert abs(got["loss"] - c["want"]["loss"]) < 1e-4 * max(1.0, abs(c["want"]["loss"]))


# ---- through autograd -------------------------------------------------------------------------------------------------------------------
def _tiny_nets(seed=5):
    torch.manual_seed(seed)
    actor = nn.Sequential(nn.Linear(7, 16), nn.ELU(), nn.Linear(16, 5))
    critic = nn.Sequential(nn.Linear(9, 16), nn.ELU(), nn.Linear(16, 1))
    return actor, critic, nn.Parameter(0.5 + 0.5 * torch.rand(5))


def test_loss_backward_reaches_the_parameters():
    name = "b257_a5"
    inp, cfg = pc.make_inputs(name), cfg_of(name)
    g = inp["groups"][0]
    actor, critic, std = _tiny_nets()
    rng = np.random.default_rng(3)
    obs, cobs = rng.normal(size=(257, 7)).astype(np.float32), rng.normal(size=(257, 9)).astype(np.float32)

    def forward(actor, critic, std, x, cx):
        mu = actor(x)
        return mu, mu * 0. + std, critic(cx)

    def params(*mods):
        return [p for m in mods for p in (m.parameters() if isinstance(m, nn.Module) else [m])]

    # the stored columns are placed around THESE networks' outputs, as make_inputs does around its own
    a64, c64, s64 = copy.deepcopy(actor).double(), copy.deepcopy(critic).double(), nn.Parameter(std.detach().double())
    with torch.no_grad():
        mu0, sg0, v0 = (t.numpy() for t in forward(a64, c64, s64, torch.from_numpy(obs).double(), torch.from_numpy(cobs).double()))
    rng2 = np.random.default_rng(4)
    g = dict(g, old_mu=(mu0 + 0.1 * sg0 * rng2.normal(size=mu0.shape)).astype(np.float32), old_sigma=(sg0 * 1.03).astype(np.float32))
    g["actions"] = (g["old_mu"] + g["old_sigma"] * rng2.normal(size=mu0.shape)).astype(np.float32)
    g["old_log_prob"] = pc.old_log_prob_for(mu0, sg0, g["actions"], pc.gap_ratio(rng2, 257)).reshape(-1, 1)
    tv = (v0 - pc.gap_step(rng2, 257).reshape(-1, 1)).astype(np.float32)
    ret = (tv + 0.5 * rng2.normal(size=tv.shape)).astype(np.float32)

    def reference(dtype):
        a, c, s = (copy.deepcopy(actor).to(dtype), copy.deepcopy(critic).to(dtype), nn.Parameter(std.detach().to(dtype)))
        mu, sigma, v = forward(a, c, s, torch.from_numpy(obs).to(dtype), torch.from_numpy(cobs).to(dtype))
        t = lambda x: torch.from_numpy(x).to(dtype)
        logp = (-(t(g["actions"]) - mu) ** 2 / (2 * sigma ** 2) - torch.log(sigma) - 0.5 * np.log(2 * np.pi)).sum(-1)
        r = torch.exp(logp - t(g["old_log_prob"]).reshape(-1))
        adv = t(g["advantages"]).reshape(-1)
        sur = torch.max(-adv * r, -adv * torch.clamp(r, 1.0 - pc.CLIP, 1.0 + pc.CLIP)).mean()
        vc = t(tv) + (v - t(tv)).clamp(-pc.CLIP, pc.CLIP)
        vl = torch.max((v - t(ret)) ** 2, (vc - t(ret)) ** 2).mean()
        ent = (0.5 + 0.5 * np.log(2 * np.pi) + torch.log(sigma)).sum(-1).mean()
        loss = sur + vl - cfg["ent"] * ent
        return [x.double().numpy() for x in torch.autograd.grad(loss, params(a, c, s))], loss.item()

    ref64, loss64 = reference(torch.float64)
    ref32, _ = reference(torch.float32)
    actor, critic, std = actor.to(DEV), critic.to(DEV), nn.Parameter(std.detach().to(DEV))
    d = lambda x: torch.from_numpy(x).to(DEV)
    loss_fn = ppo_loss.FusedPPOLoss(clip_param=pc.CLIP, value_loss_coef=1.0, entropy_coef=cfg["ent"])

    def fused():
        mu, sigma, v = forward(actor, critic, std, d(obs), d(cobs))
        return loss_fn(mu, sigma, v, d(g["actions"]), d(g["old_log_prob"]), d(g["advantages"]), d(ret), d(tv), d(g["old_mu"]), d(g["old_sigma"]))

    out = fused()
    assert out.loss.requires_grad and out.loss.dim() == 0 and out.loss.grad_fn is not None
    for s in (out.surrogate_loss, out.value_loss, out.entropy, out.kl_mean):
        assert s.dim() == 0 and not s.requires_grad and s.grad_fn is None
    assert float(out.kl_mean) > 0 and abs(out.loss.detach().item() - loss64) <= 1e-5 * max(1.0, abs(loss64))
    ps = params(actor, critic, std)
    out.loss.backward()
    got = [p.grad.detach().cpu().double().numpy() for p in ps]
    # through the networks' float32 backward both sides sum 257 rows per parameter in their own order: the rule's torch side carries that
    for i, (x, r64, r32) in enumerate(zip(got, ref64, ref32)):
        err, bound = pc.max_err(x, r64), pc.parity_bound(pc.max_err(r32, r64), r64)
        print(f"parameter {i} {x.shape}: err {err:.3e}, torch-f32 err {pc.max_err(r32, r64):.3e}, bound {bound:.3e}")
        assert err <= bound, (i, err, bound)
    for p in ps:
        p.grad = None
    (2 * fused().loss).backward()                      # a non-unit upstream factor scales the stored gradients
    for p, x in zip(ps, got):
        assert np.allclose(p.grad.cpu().double().numpy(), 2 * x, rtol=1e-5, atol=1e-9)
    adj = ppo_loss.adjust_learning_rate(out.kl_mean, 1e-3, float(out.kl_mean) / 4)
    assert adj == 1e-3 / 1.5


def test_cts_form_returns_both_surrogates():
    name = "cts_17_5"
    inp, ref64, ref32 = case_data(name)
    dev = to_device(inp)
    for g in dev["groups"]:
        g["mu"].requires_grad_(); g["sigma"].requires_grad_()
    dev["values"].requires_grad_()
    c = pc.CASES[name]
    loss_fn = ppo_loss.FusedPPOLoss(entropy_coef=c["ent"], use_clipped_value_loss=c["clipped"], use_spo=c["spo"])
    t, s = ({k: v for k, v in g.items() if v is not None} for g in dev["groups"])
    out = loss_fn.cts(teacher=t, student=s, values=dev["values"], returns=dev["returns"], target_values=dev["target_values"])
    out.loss.backward()
    raw = dict(result=out.result, grad_values=dev["values"].grad, grad_mu=[g["mu"].grad for g in dev["groups"]],
               grad_sigma=[g["sigma"].grad for g in dev["groups"]])
    assert out.teacher_surrogate_loss.data_ptr() != out.student_surrogate_loss.data_ptr() and not out.student_surrogate_loss.requires_grad
    pc.check_parity(collect(raw, c["kl"]), ref64, ref32, name + " (cts)")


# ---- reproducible -----------------------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical():
    inp, _, _ = case_data(pc.LARGEST)
    dev = to_device(inp)
    a, _ = run(dev, **cfg_of(pc.LARGEST))
    b, _ = run(dev, **cfg_of(pc.LARGEST))
    assert same_bits(a, b) and np.isfinite(a["loss"])


# ---- NaN --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b257_a12", "b257_a12_spo"])
def test_nan_row_stays_in_its_row(name):
    inp, _, _ = case_data(name)
    clean, _ = run(to_device(inp), **cfg_of(name))
    bad = copy.deepcopy(inp)
    row = 130
    bad["groups"][0]["mu"][row, 7] = np.nan
    got, _ = run(to_device(bad), **cfg_of(name))
    assert np.isnan(got["loss"]) and np.isnan(got["surrogate"][0]) and np.isnan(got["kl"][0])
    assert np.isnan(got["grad_mu"][0][row]).all() and np.isnan(got["grad_sigma"][0][row]).all()
    keep = np.arange(257) != row
    assert np.array_equal(got["grad_mu"][0][keep], clean["grad_mu"][0][keep]) and np.array_equal(got["grad_sigma"][0][keep], clean["grad_sigma"][0][keep])
    assert got["value_loss"] == clean["value_loss"] and np.array_equal(got["grad_values"], clean["grad_values"])
    assert got["entropy"] == clean["entropy"]          # the entropy reads sigma only


# ---- strides ----------------------------------------------------------------------------------------------------------------------------
def _strided(x, name=None):
    """x as a view of row stride width + 3 whose base lies 4 bytes past a 16-byte boundary; gap columns hold SENTINEL."""
    x = torch.as_tensor(x)
    n, w = x.shape
    buf = torch.full((n * (w + 3) + 8,), SENTINEL, device=DEV)
    off = ((4 - buf.data_ptr()) % 16) // 4
    wide = buf[off:off + n * (w + 3)].view(n, w + 3)
    view = wide[:, :w]
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 and (n == 1 or view.stride(0) == w + 3)
    view._wide = wide
    return view


@pytest.mark.parametrize("name", ["b65_a4", "b257_a5", "b1025_a13", "cts_17_5"])
def test_strided_views_equal_the_contiguous_call(name):
    inp, _, _ = case_data(name)
    strided_equals_contiguous(inp, pc.CASES[name], cfg_of(name))


def strided_equals_contiguous(inp, c, cfg):
    """Every input and output of case dict `c` as a `_strided` view: the bits of the contiguous call, and no gap column written."""
    want, _ = run(to_device(inp), **cfg)
    dev = to_device(inp, _strided)
    out = {"grad_values": _strided(torch.full((c["vrows"], 1), SENTINEL))}
    for gi, B in enumerate(c["rows"]):
        out[f"grad_mu{gi}"], out[f"grad_sigma{gi}"] = _strided(torch.full((B, c["A"]), SENTINEL)), _strided(torch.full((B, c["A"]), SENTINEL))
    got, raw = run(dev, out=out, **cfg)
    assert same_bits(got, want)
    for t in [raw["grad_values"]] + raw["grad_mu"] + raw["grad_sigma"]:
        w = t.shape[1]
        assert (t._wide[:, w:] == SENTINEL).all() and not (t == SENTINEL).any()          # no gap column is written, every column is


# ---- capture ----------------------------------------------------------------------------------------------------------------------------
def test_captured_call_replays_on_changed_inputs():
    name = "b1025_a13"
    inp, _, _ = case_data(name)
    other = pc.make_inputs(dict(pc.CASES[name], seed=99))
    dev = to_device(inp)
    c = pc.CASES[name]
    out = dict(grad_mu0=torch.empty(1025, 13, device=DEV), grad_sigma0=torch.empty(1025, 13, device=DEV), grad_values=torch.empty(1025, 1, device=DEV),
               partials=torch.empty(ppo_loss.workspace_doubles(c["rows"], c["vrows"], c["A"]), dtype=torch.float64, device=DEV),
               result=torch.empty(abi.PPO_RESULT_FLOATS, device=DEV))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run(dev, out=out, **cfg_of(name))                   # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):            # one stream, no parallel branches: the pass and the sum behind it
        flags = abi.PPO_CLIPPED_VALUE
        g = dict(dev["groups"][0], grad_mu=out["grad_mu0"], grad_sigma=out["grad_sigma0"])
        args = ppo_loss.ppo_loss_args([g], dev["values"], dev["returns"], dev["target_values"], out["grad_values"], out["partials"],
                                      out["result"], pc.CLIP, 1.0, c["ent"], flags)
        ppo_loss.launch(args, torch.device(DEV))
    new = to_device(other)
    for k, v in new["groups"][0].items():                   # the inputs change in place
        if v is not None:
            dev["groups"][0][k].copy_(v)
    for k in ("values", "returns", "target_values"):
        dev[k].copy_(new[k])
    for t in out.values():
        t.fill_(7.0) if t.dtype == torch.float32 else t.fill_(float("nan"))      # a slab slot read before it is written shows
    graph.replay()
    raw = dict(result=out["result"], grad_values=out["grad_values"], grad_mu=[out["grad_mu0"]], grad_sigma=[out["grad_sigma0"]])
    replayed = collect(raw, c["kl"])
    fresh, _ = run(new, **cfg_of(name))
    assert same_bits(replayed, fresh)
    first, _ = run(to_device(inp), **cfg_of(name))
    assert not same_bits(replayed, first)

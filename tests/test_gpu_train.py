"""The fused learner pass on the GPU (hcr_genesis_lr_cl_amd/train.py, csrc/lg_train.hip) against the float64 restatement of
tests/train_cases.py under the project's parity rule, and its conventions: .grad through FusedPPOLoss and its accumulation, bit-identical
repeats, Hardtanh-saturated means, strided views, the NaN row, the non-finite grad_sigma, weights changed in place, the stale-forward
refusal, the six steps of the reference's PPO.update() end to end (train pass, FusedPPOLoss, FusedAdam) and one whole update step as a
HIP graph."""
import os

import numpy as np
import pytest
import torch

from hcr_genesis_lr_cl_amd import optim, ppo_loss, train
from tests import train_cases as tc
from tests import train_gpu as tg
from tests.train_gpu import COTANGENTS, DEV, dev, host, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ppo_train.npz")
RATIOS = []
references = tc.references


def run(x, m=None, tp=None):
    """One forward and one backward of the case's three cotangents on a fresh module: (name -> numpy array, module, pass)."""
    m = m if m is not None else tc.Module(x, DEV)
    tp = tp if tp is not None else train.FusedTrainPass(m)
    for p in m.parameters():
        p.grad = None
    mu, sigma, values = tp(dev(x["obs"]), dev(x["critic_obs"]))
    torch.autograd.backward([mu, sigma, values], [dev(x[k]) for k in COTANGENTS])
    torch.cuda.synchronize()
    got = tc.named(x, dict(mu=host(mu), sigma=host(sigma), values=host(values)), [host(p.grad) for p in m.ordered_parameters()])
    return got, m, tp


# ---- parity -----------------------------------------------------------------------------------------------------------------------------------
PARITY_CASES = tg.parity_cases(tc)


def _slices_raggedly(net, b):
    p = train.plan(b, *tc.NETS[net])
    assert any(S > 1 and b % per for S, per in zip(list(p.slices[0]) + list(p.slices[1]), list(p.slice_rows[0]) + list(p.slice_rows[1])) if S)


def case_inputs(name):
    return tg.case_inputs(tc, name, 400, _slices_raggedly)


@pytest.mark.parametrize("name", PARITY_CASES)
def test_parity_on_the_table(name):
    x = case_inputs(name)
    got, _, _ = run(x)
    ref64, ref32 = references(x)
    tc.check_parity(got, ref64, ref32, name, RATIOS)


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------------
def _loss_inputs(x, rng):
    B, A = x["obs"].shape[0], x["actor"][-1]
    fw = tc.forward(x)
    f = lambda v: np.ascontiguousarray(v, dtype=np.float32)
    old_mu, old_sigma = f(fw["mu"] + 0.1 * rng.normal(size=(B, A))), f(fw["sigma"] * np.exp(0.03 * rng.normal(size=(B, A))))
    actions = f(old_mu + old_sigma * rng.normal(size=(B, A)))
    old_lp = f((-(actions - old_mu) ** 2 / (2 * old_sigma ** 2) - np.log(old_sigma) - tg.HALF_LOG_2PI).sum(-1, keepdims=True))
    target = f(rng.normal(size=(B, 1)))
    return dict(actions=actions, old_log_prob=old_lp, advantages=f(rng.normal(size=(B, 1))), returns=f(target + 0.5 * rng.normal(size=(B, 1))),
                target_values=target, old_mu=old_mu, old_sigma=old_sigma)


def test_backward_through_the_loss_head_fills_grad_and_accumulates():
    """loss.backward() through FusedPPOLoss leaves in .grad exactly what the direct call computes from the loss head's own gradients; a
    second backward without zero_grad accumulates (autograd's g + g, bit for bit twice the first)."""
    x = tc.make_inputs("tiny_b257")
    cols = {k: dev(v) for k, v in _loss_inputs(x, np.random.default_rng(5)).items()}
    m = tc.Module(x, DEV)
    tp = train.FusedTrainPass(m)
    loss_fn = ppo_loss.FusedPPOLoss(clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01)
    obs, cobs = dev(x["obs"]), dev(x["critic_obs"])

    def step():
        mu, sigma, values = tp(obs, cobs)
        out = loss_fn(mu, sigma, values, cols["actions"], cols["old_log_prob"], cols["advantages"], cols["returns"], cols["target_values"],
                      cols["old_mu"], cols["old_sigma"])
        out.loss.backward()
        return mu, sigma, values
    mu, sigma, values = step()
    first = [host(p.grad).copy() for p in m.ordered_parameters()]
    assert all(p.grad is not None and p.grad.shape == p.shape for p in m.parameters())
    # the direct call: the loss head's gradients for detached outputs, handed to the pass's backward as cotangents
    leaves = [t.detach().requires_grad_(True) for t in (mu, sigma, values)]
    loss_fn(*leaves, cols["actions"], cols["old_log_prob"], cols["advantages"], cols["returns"], cols["target_values"], cols["old_mu"],
            cols["old_sigma"]).loss.backward()
    y = dict(x, grad_mu=host(leaves[0].grad), grad_sigma=host(leaves[1].grad), grad_values=host(leaves[2].grad))
    direct, _, _ = run(y)
    names = tc.param_names(x["actor"], x["critic"])
    assert all(np.array_equal(g.view(np.uint32), direct[n].view(np.uint32)) for n, g in zip(names, first))
    ref64, ref32 = references(y)
    tc.check_parity(dict(direct), ref64, ref32, "through the loss head", RATIOS)
    step()                                                            # no zero_grad in between
    second = [host(p.grad) for p in m.ordered_parameters()]
    assert all(np.array_equal(b, a + a) for a, b in zip(first, second))


@pytest.mark.parametrize("name", ["tiny_b257", "go2_b257"])
def test_repeats_are_bit_identical(name):
    x = tc.make_inputs(name)
    a, m, tp = run(x)
    b, _, _ = run(x, m, tp)                                           # the same pass again: its workspace is reused
    c, _, _ = run(x)                                                  # a fresh module and pass
    assert same_bits(a, b) and same_bits(a, c)


def test_saturated_means_pass_no_gradient_into_the_actor():
    x = tc.make_inputs("tiny_b257")
    clean, _, _ = run(x)
    sat = np.abs(clean["mu"]) >= np.float32(x["clip"])
    assert 0.1 <= sat.mean() <= 0.9 and np.array_equal(np.abs(clean["mu"][sat]), np.full(sat.sum(), np.float32(x["clip"])))
    y = dict(x, grad_mu=np.where(sat, np.float32(1e30) * np.sign(x["grad_mu"]), x["grad_mu"]).astype(np.float32))
    assert same_bits(run(y)[0], clean)                                # whatever arrives at a saturated mean is dropped
    y["grad_mu"][sat] = np.nan
    assert same_bits(run(y)[0], clean)
    # rows whose means all saturate contribute nothing: without them the actor's gradients are those of the other rows alone
    rows = sat.all(1)
    assert rows.any() and not rows.all()
    z = dict(x, grad_mu=np.where(rows[:, None], 0, x["grad_mu"]).astype(np.float32))
    assert same_bits(run(z)[0], clean)
    # and an actor without the Hardtanh lets every gradient through: the mask is the Hardtanh's, not the kernel's
    free = dict(x, clip=None)
    got, _, _ = run(free)
    tc.check_parity(got, *references(free), "no clip", RATIOS)
    assert not np.array_equal(got["actor.0.weight"], clean["actor.0.weight"])


# ---- addressing -------------------------------------------------------------------------------------------------------------------------------
def test_strided_views_of_every_matrix_leave_the_gaps_untouched():
    """The C ABI through train.train_args on column slices of wider matrices (inputs, outputs, incoming gradients): the same bits as the
    contiguous call, and every gap column keeps its fill."""
    x = tc.make_inputs("tiny_b33")
    clean, _, _ = run(x)
    m = tc.Module(x, DEV)
    D = m.std.device                                                  # with its index, as the parameters carry it
    spec = train.describe(m, D)
    B, A, FILL = 33, 3, 7.25
    wide = {k: torch.full((B, w), FILL, device=DEV) for k, w in (("in", 24), ("out", 16), ("grad", 19))}
    obs, cobs = wide["in"][:, 3:8], wide["in"][:, 11:17]
    mu, sigma, values = wide["out"][:, 1:4], wide["out"][:, 6:9], wide["out"][:, 13:14]
    gm, gs, gv = wide["grad"][:, 2:5], wide["grad"][:, 9:12], wide["grad"][:, 17:18]
    for view, k in ((obs, "obs"), (cobs, "critic_obs"), (gm, "grad_mu"), (gs, "grad_sigma"), (gv, "grad_values")):
        view.copy_(dev(x[k]))
    before = {k: host(v).copy() for k, v in wide.items()}
    ws = torch.empty(int(train.plan(B, spec.actor.widths, spec.critic.widths).workspace_floats), device=DEV)
    train.forward(train.train_args(spec, obs, cobs, mu, sigma, values, ws, device=D), D)
    grads = [torch.full_like(p, FILL) for p in spec.parameters()]
    a = train.train_args(spec, obs, cobs, mu, sigma, values, ws, grads, gm, gs, gv, device=D)
    assert (a.chain[0].in_stride, a.mu_stride, a.values_stride, a.grad_sigma_stride) == (24, 16, 16, 19)
    train.backward(a, D)
    torch.cuda.synchronize()
    got = tc.named(x, dict(mu=host(mu), sigma=host(sigma), values=host(values)), [host(g) for g in grads])
    assert same_bits(got, clean)
    after = {k: host(v) for k, v in wide.items()}
    assert np.array_equal(after["in"], before["in"]) and np.array_equal(after["grad"], before["grad"])
    gaps = np.ones(16, bool)
    gaps[[1, 2, 3, 6, 7, 8, 13]] = False
    assert (after["out"][:, gaps] == FILL).all()


def test_weights_changed_in_place_are_seen():
    x = tc.make_inputs("tiny_b33")
    _, m, tp = run(x)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(0.5)
    y = dict(x, params=[host(p).copy() for p in m.ordered_parameters()])
    again, _, _ = run(y, m, tp)
    fresh, _, _ = run(y)
    assert same_bits(again, fresh)
    tc.check_parity(again, *references(y), "weights halved in place", RATIOS)


def test_backward_of_an_overwritten_forward_is_refused():
    x = tc.make_inputs("tiny_b33")
    m = tc.Module(x, DEV)
    tp = train.FusedTrainPass(m)
    obs, cobs = dev(x["obs"]), dev(x["critic_obs"])
    mu1, _, _ = tp(obs, cobs)
    mu2, _, values2 = tp(obs, cobs)
    with pytest.raises(RuntimeError, match=r"FusedTrainPass: backward of forward call 1, but forward call 2 has overwritten"):
        mu1.sum().backward()
    assert all(p.grad is None for p in m.parameters())
    (mu2.sum() + values2.sum()).backward()                             # the newest forward is still good
    assert all(p.grad is not None for p in m.parameters())
    with torch.no_grad():
        tp(obs, cobs)                                                  # an evaluation in between counts: it rewrote the workspace
    mu4, _, _ = tp(obs[:9], cobs[:9])
    mu5, _, _ = tp(obs, cobs)
    with pytest.raises(RuntimeError, match=r"forward call 4, but forward call 5"):
        mu4.sum().backward()


# ---- non-finite values ------------------------------------------------------------------------------------------------------------------------
def test_a_nan_row_stays_in_its_row_and_reaches_the_gradients_torch_reaches():
    x = tc.make_inputs("tiny_b257")
    clean, _, _ = run(x)
    y = dict(x, obs=x["obs"].copy())
    y["obs"][37, 2] = np.nan
    got, _, _ = run(y)
    others = np.arange(257) != 37
    assert np.isnan(got["mu"][37]).all() and np.isnan(got["sigma"][37]).all()
    for k in ("mu", "sigma"):
        assert np.array_equal(got[k][others].view(np.uint32), clean[k][others].view(np.uint32))
    names = tc.param_names(x["actor"], x["critic"])
    for n in ["values"] + [n for n in names if n.startswith("critic")]:          # the critic read another matrix: not a bit changes
        assert np.array_equal(got[n].view(np.uint32), clean[n].view(np.uint32)), n
    theirs = tc.torch_pass(y)
    for n, g in zip(names, theirs["grads"]):
        if n.startswith("actor"):
            assert (np.isnan(got[n]) | ~np.isnan(g)).all(), n            # wherever torch's gradient is NaN, so is the kernel's
    assert np.isnan(got["actor.2.weight"]).all() and np.isnan(got["actor.0.weight"][:, 2]).all() and np.isfinite(got["actor.2.bias"]).all()
    assert np.array_equal(got["std"].view(np.uint32), clean["std"].view(np.uint32))
    # the same through the critic
    z = dict(x, critic_obs=x["critic_obs"].copy())
    z["critic_obs"][256, 0] = np.inf
    got, _, _ = run(z)
    assert not np.isfinite(got["values"][256]).any() and np.array_equal(got["values"][:256].view(np.uint32), clean["values"][:256].view(np.uint32))
    for n in ["mu", "sigma", "std"] + [n for n in names if n.startswith("actor")]:
        assert np.array_equal(got[n].view(np.uint32), clean[n].view(np.uint32)), n


def test_a_non_finite_grad_sigma_reaches_grad_std_only():
    """include/lgtrain.h: the path sigma = mu * 0 + std -> mu is taken as exactly zero, where autograd's grad_sigma * 0 is NaN."""
    x = tc.make_inputs("tiny_b257")
    clean, _, _ = run(x)
    row = int(np.flatnonzero(np.abs(clean["mu"][:, 1]) < np.float32(x["clip"]))[3])       # an unsaturated mean: autograd's NaN gets through the Hardtanh
    for bad in (np.inf, np.nan):
        y = dict(x, grad_sigma=x["grad_sigma"].copy())
        y["grad_sigma"][row, 1] = bad
        got, _, _ = run(y)
        assert not np.isfinite(got["std"][1]) and np.array_equal(got["std"][[0, 2]].view(np.uint32), clean["std"][[0, 2]].view(np.uint32))
        for n in got:
            if n != "std":
                assert np.array_equal(got[n].view(np.uint32), clean[n].view(np.uint32)), n
        theirs = dict(zip(tc.param_names(x["actor"], x["critic"]), tc.torch_pass(y)["grads"]))
        assert np.isnan(theirs["actor.0.weight"]).any()               # the departure: autograd poisons the actor here




# ---- the whole update -------------------------------------------------------------------------------------------------------------------------
def _init_inputs(fx):
    return dict(tc.fixture_step(fx, 0), params=[np.asarray(p, np.float32) for p in fx["init"]])


def _torch_update(fx, dtype):
    """The reference's mini-batch steps on the fixture's columns in torch ops of `dtype` on the CPU (tests/train_gpu.torch_rl_update).
    Returns (per step the parameters by name as float64 numpy, rates)."""
    m = tc.Module(_init_inputs(fx), dtype=dtype)
    assert [n for n, _ in m.named_parameters()] == fx["names"]
    snap = lambda: {n: p.detach().double().numpy().copy() for n, p in m.named_parameters()}
    return tg.torch_rl_update(fx, tc.FIXTURE_COLUMNS, lambda c: m(c["obs"], c["critic_obs"]), list(m.parameters()), snap, dtype)


class _Learner:
    """FusedTrainPass + FusedPPOLoss + FusedAdam on a module: the fused PPO mini-batch step."""

    def __init__(self, m, cfg):
        self.tp = train.FusedTrainPass(m)
        self.loss_fn = ppo_loss.FusedPPOLoss(clip_param=cfg["clip_param"], value_loss_coef=cfg["value_loss_coef"], entropy_coef=cfg["entropy_coef"])
        self.opt = optim.FusedAdam(m.named_parameters(), lr=cfg["lr0"], betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"],
                                   max_grad_norm=cfg["max_grad_norm"], desired_kl=cfg["desired_kl"])
        self.optimizers = (self.opt,)

    def step(self, t):
        mu, sigma, values = self.tp(t["obs"], t["critic_obs"])
        out = self.loss_fn(mu, sigma, values, t["actions"], t["old_log_prob"], t["advantages"], t["returns"], t["target_values"], t["old_mu"], t["old_sigma"])
        self.opt.zero_grad()
        out.loss.backward()
        self.opt.step(kl_mean=out.kl_mean)
        return out


def test_fixture_update_end_to_end():
    """The six steps of the reference's PPO.update() through FusedTrainPass, FusedPPOLoss and FusedAdam: the learning rates are the
    fixture's, the parameters after every step lie within the parity rule of the float64 run of the same torch code on the float32
    inputs (its float32 side: that code in float32 on the CPU), and that float64 run is the fixture up to the rounding of its inputs."""
    fx = tc.load_fixture(FIXTURE)
    cfg = fx["cfg"]
    ref64, lrs64 = _torch_update(fx, torch.float64)
    ref32, lrs32 = _torch_update(fx, torch.float32)
    assert lrs64 == lrs32 == [float(v) for v in fx["lr"]]
    assert max(np.abs(ref64[-1][n] - b).max() for n, b in zip(fx["names"], fx["params"][-1])) < 1e-5
    m = tc.Module(_init_inputs(fx), DEV)
    learner = _Learner(m, cfg)
    for s, t in enumerate(tg.fixture_batches(fx, tc.FIXTURE_COLUMNS, cfg["steps"])):
        learner.step(t)
        assert learner.opt.lr == float(fx["lr"][s]), (s, learner.opt.lr, fx["lr"][s])
        tg.check_parameters({n: host(p) for n, p in m.named_parameters()}, ref64[s], ref32[s], s, RATIOS)


def test_captured_update_step_replays_like_eager_steps():
    """One whole update step (train pass forward, loss head, backward, optimizer) captured on one stream as a HIP graph and replayed three
    times with the mini-batch rewritten in place in between: the parameters, the rate and the step count are those of three eager steps
    bit for bit."""
    fx = tc.load_fixture(FIXTURE)
    x = _init_inputs(fx)
    tg.replays_like_eager_steps(lambda: tc.Module(x, DEV), lambda m: _Learner(m, fx["cfg"]), tg.fixture_batches(fx, tc.FIXTURE_COLUMNS, 3))


def test_zz_print_the_parity_ratios():
    """Not a check of its own: the worst |kernel - f64| / max(|torch-f32 - f64|, ulp) per tensor class over every parity check above, for
    DESIGN.md's table."""
    tg.print_parity_ratios(RATIOS)

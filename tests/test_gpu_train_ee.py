"""The explicit-estimator learner passes on the GPU (hcr_genesis_lr_cl_amd/train.py's FusedTrainPassEE, csrc/lg_train_ee.hip) against the
float64 restatement of tests/train_ee_cases.py under the project's parity rule, and their conventions: the reference's whole PPO_EE.update()
end to end (6 RL steps, 12 estimator steps; FusedTrainPassEE, FusedPPOLoss, two FusedAdams), bit-identical repeats, one RL step plus one
estimator step as a HIP graph, strided views, weights changed in place, the stale-forward refusal per pass, the estimator's .grad left
alone by the RL backward, the fully masked batch and the NaN row."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from hcr_genesis_lr_cl_amd import optim, ppo_loss, train
from tests import train_ee_cases as ec
from tests import train_gpu as tg
from tests.train_gpu import COTANGENTS, DEV, dev, host, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ppo_ee_train.npz")
RATIOS = []


def run(x, m=None, tp=None):
    """Both passes once on a fresh module: the RL forward and the backward of the case's three cotangents, then the estimator loss and
    its backward under the case's upstream factor.  (name -> numpy array, module, pass)."""
    m = m if m is not None else ec.Module(x, DEV)
    tp = tp if tp is not None else train.FusedTrainPassEE(m)
    for p in m.parameters():
        p.grad = None
    f = dev(x["features"])
    mu, sigma, values = tp(f, dev(x["critic_obs"]))
    torch.autograd.backward([mu, sigma, values], [dev(x[k]) for k in COTANGENTS])
    assert all(p.grad is None for p in m.estimator_parameters())              # the RL pass gives the estimator nothing
    loss = tp.estimator_loss(f, dev(x["labels"]), dev(x["terminated"]))
    (loss * float(x["upstream"])).backward()
    torch.cuda.synchronize()
    got = ec.named(x, dict(mu=host(mu), sigma=host(sigma), values=host(values)), [host(p.grad) for p in m.rl_parameters()], host(loss),
                   [host(p.grad) for p in m.estimator_parameters()])
    return got, m, tp


# ---- parity -----------------------------------------------------------------------------------------------------------------------------------
PARITY_CASES = tg.parity_cases(ec)


def case_inputs(name):
    return tg.case_inputs(ec, name, 800)


@pytest.mark.parametrize("name", PARITY_CASES)
def test_parity_on_the_table(name):
    x = case_inputs(name)
    got, _, _ = run(x)
    ref64, ref32 = ec.references(x)
    ec.check_parity(got, ref64, ref32, name, RATIOS)


# ---- the whole update -------------------------------------------------------------------------------------------------------------------------
def _init_inputs(fx):
    return dict(ec.fixture_inputs(fx, {k: np.asarray(v, np.float32) for k, v in fx["init"].items()}))


def _torch_update(fx, dtype):
    """The reference's PPO_EE.update() on the fixture's columns (rounded to float32 first) in torch ops of `dtype` on the CPU: the RL steps
    of tests/train_gpu.torch_rl_update, then the estimator steps.  Returns (per step, RL steps then estimator steps, the parameters by name
    as float64 numpy; the RL rates)."""
    cfg = fx["cfg"]
    m = ec.Module(_init_inputs(fx), dtype=dtype)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dtype)
    snap = lambda: {n: p.detach().double().numpy().copy() for n, p in m.named_parameters()}
    out, lrs = tg.torch_rl_update(fx, ec.FIXTURE_COLUMNS, lambda c: m(c["features"], c["critic_obs"]), m.rl_parameters(), snap, dtype)
    est_opt = torch.optim.Adam(m.estimator_parameters(), lr=cfg["estimator_lr"], betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"])
    for s in range(cfg["est_steps"]):
        loss = m.estimator_loss(t(fx["est_features"][s]), t(fx["est_labels"][s]), t(fx["est_terminated"][s]))
        est_opt.zero_grad()
        loss.backward()
        nn.utils.clip_grad_norm_(m.estimator_parameters(), cfg["max_grad_norm"])
        est_opt.step()
        out.append(snap())
    return out, lrs


class _Learner:
    """FusedTrainPassEE + FusedPPOLoss + two FusedAdams on a module: the fused PPO_EE mini-batch steps."""

    def __init__(self, m, cfg):
        self.tp = train.FusedTrainPassEE(m)
        self.loss_fn = ppo_loss.FusedPPOLoss(clip_param=cfg["clip_param"], value_loss_coef=cfg["value_loss_coef"], entropy_coef=cfg["entropy_coef"])
        betas = (cfg["beta1"], cfg["beta2"])
        self.rl_opt = optim.FusedAdam(list(zip(self.tp.spec.rl_parameter_names(), self.tp.rl_parameters())), lr=cfg["lr0"], betas=betas, eps=cfg["eps"],
                                      max_grad_norm=cfg["max_grad_norm"], desired_kl=cfg["desired_kl"])
        self.est_opt = optim.FusedAdam(list(zip(self.tp.spec.estimator_parameter_names(), self.tp.estimator_parameters())), lr=cfg["estimator_lr"],
                                       betas=betas, eps=cfg["eps"], max_grad_norm=cfg["max_grad_norm"])
        self.optimizers = (self.rl_opt, self.est_opt)

    def rl_step(self, c):
        mu, sigma, values = self.tp(c["features"], c["critic_obs"])
        out = self.loss_fn(mu, sigma, values, c["actions"], c["old_log_prob"], c["advantages"], c["returns"], c["target_values"], c["old_mu"], c["old_sigma"])
        self.rl_opt.zero_grad()
        out.loss.backward()
        self.rl_opt.step(kl_mean=out.kl_mean)
        return out

    def est_step(self, e):
        loss = self.tp.estimator_loss(e["est_features"], e["est_labels"], e["est_terminated"])
        self.est_opt.zero_grad()
        loss.backward()
        self.est_opt.step()
        return loss

    def step(self, b):
        """One RL step and one estimator step on a batch that holds the columns of both."""
        self.rl_step(b)
        self.est_step(b)


def test_fixture_update_end_to_end():
    """The reference's PPO_EE.update(), 6 RL steps then 12 estimator steps, through FusedTrainPassEE, FusedPPOLoss and two FusedAdams: the
    learning rates are the fixture's and every parameter after every step lies within the parity rule of the float64 run of the same torch
    code on the float32 inputs (its float32 side: that code in float32 on the CPU); that float64 run is the fixture up to the rounding
    of its inputs."""
    fx = ec.load_fixture(FIXTURE)
    cfg = fx["cfg"]
    ref64, lrs64 = _torch_update(fx, torch.float64)
    ref32, lrs32 = _torch_update(fx, torch.float32)
    assert lrs64 == lrs32 == [float(v) for v in fx["lr"]]
    assert max(np.abs(ref64[-1][n] - fx["est_params"][-1][n]).max() for n in fx["names"]) < 1e-5
    assert max(np.abs(ref64[cfg["steps"] - 1][n] - fx["params"][-1][n]).max() for n in fx["names"]) < 1e-5
    m = ec.Module(_init_inputs(fx), DEV)
    learner = _Learner(m, cfg)
    rl, est = tg.fixture_batches(fx, ec.FIXTURE_COLUMNS, cfg["steps"]), tg.fixture_batches(fx, ec.EST_COLUMNS, cfg["est_steps"])
    for s in range(cfg["steps"] + cfg["est_steps"]):
        if s < cfg["steps"]:
            learner.rl_step(rl[s])
            assert learner.rl_opt.lr == float(fx["lr"][s]), (s, learner.rl_opt.lr, fx["lr"][s])
        else:
            loss = learner.est_step(est[s - cfg["steps"]])
            assert abs(float(loss.detach()) - fx["est_loss"][s - cfg["steps"]]) < 1e-4
        tg.check_parameters({n: host(p) for n, p in m.named_parameters()}, ref64[s], ref32[s], s, RATIOS)
    assert learner.rl_opt.step_count == cfg["steps"] and learner.est_opt.step_count == cfg["est_steps"]


def test_captured_steps_replay_like_eager_steps():
    """One RL step plus one estimator step captured on one stream as a HIP graph and replayed three times with the mini-batches rewritten
    in place in between: every parameter, the rate and the step counts are those of three eager pairs of steps, bit for bit."""
    fx = ec.load_fixture(FIXTURE)
    x = _init_inputs(fx)
    both = [{**c, **e} for c, e in zip(tg.fixture_batches(fx, ec.FIXTURE_COLUMNS, 3), tg.fixture_batches(fx, ec.EST_COLUMNS, 3))]
    tg.replays_like_eager_steps(lambda: ec.Module(x, DEV), lambda m: _Learner(m, fx["cfg"]), both)


# ---- determinism, addressing, state -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fixture_b257", "go2_ee_b257"])
def test_repeats_are_bit_identical(name):
    x = ec.make_inputs(name)
    a, m, tp = run(x)
    b, _, _ = run(x, m, tp)                                           # the same pass again: its workspaces are reused
    c, _, _ = run(x)                                                  # a fresh module and pass
    assert same_bits(a, b) and same_bits(a, c)


def test_strided_views_of_every_matrix_leave_the_gaps_untouched():
    """The C ABI through train.ee_args / est_args on column slices of wider matrices: the same bits as the contiguous call, and every
    gap column keeps its fill."""
    x = ec.make_inputs("fixture_b33")
    x["upstream"] = np.float32(1.0)
    clean, _, _ = run(x)
    m = ec.Module(x, DEV)
    D = m.std.device
    spec = train.describe_ee(m, D)
    B, FILL = 33, 7.25
    wide = {k: torch.full((B, w), FILL, device=DEV) for k, w in (("in", 40), ("out", 16), ("grad", 19))}
    feats, cobs, labels, term = wide["in"][:, 3:10], wide["in"][:, 13:22], wide["in"][:, 25:28], wide["in"][:, 33:34]
    mu, sigma, values = wide["out"][:, 1:4], wide["out"][:, 6:9], wide["out"][:, 13:14]
    gm, gs, gv = wide["grad"][:, 2:5], wide["grad"][:, 9:12], wide["grad"][:, 17:18]
    for view, k in ((feats, "features"), (cobs, "critic_obs"), (labels, "labels"), (term, "terminated"), (gm, "grad_mu"), (gs, "grad_sigma"),
                    (gv, "grad_values")):
        view.copy_(dev(x[k]))
    before = {k: host(v).copy() for k, v in wide.items()}
    ws = torch.empty(int(train.plan_ee(B, *ec.NETS["fixture"]).workspace_floats), device=DEV)
    train._call("lg_train_ee_forward", train.ee_args(spec, feats, cobs, mu, sigma, values, ws, device=D), D)
    rl_grads = [torch.full_like(p, FILL) for p in spec.rl_parameters()]
    a = train.ee_args(spec, feats, cobs, mu, sigma, values, ws, rl_grads, gm, gs, gv, device=D)
    assert (a.chain[0].in_stride, a.chain[2].in_stride, a.mu_stride, a.grad_sigma_stride) == (40, 40, 16, 19)
    train._call("lg_train_ee_backward", a, D)
    ews = torch.empty(int(train.plan_est(B, ec.NETS["fixture"][0]).workspace_floats), device=DEV)
    loss, up = torch.full((), FILL, device=DEV), torch.ones(1, device=DEV)
    train._call("lg_train_est_forward", train.est_args(spec, feats, labels, term, loss, ews, device=D), D)
    est_grads = [torch.full_like(p, FILL) for p in spec.estimator_parameters()]
    e = train.est_args(spec, feats, labels, term, None, ews, est_grads, up, device=D)
    assert (e.chain.in_stride, e.labels_stride, e.mask_stride) == (40, 40, 40)
    train._call("lg_train_est_backward", e, D)
    torch.cuda.synchronize()
    got = ec.named(x, dict(mu=host(mu), sigma=host(sigma), values=host(values)), [host(g) for g in rl_grads], host(loss), [host(g) for g in est_grads])
    assert same_bits(got, clean)
    after = {k: host(v) for k, v in wide.items()}
    assert np.array_equal(after["in"], before["in"]) and np.array_equal(after["grad"], before["grad"])
    gaps = np.ones(16, bool)
    gaps[[1, 2, 3, 6, 7, 8, 13]] = False
    assert (after["out"][:, gaps] == FILL).all()


def test_weights_changed_in_place_are_seen():
    x = ec.make_inputs("fixture_b33")
    _, m, tp = run(x)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(0.5)
    y = dict(x, rl_params=[host(p).copy() for p in m.rl_parameters()], est_params=[host(p).copy() for p in m.estimator_parameters()])
    again, _, _ = run(y, m, tp)
    fresh, _, _ = run(y)
    assert same_bits(again, fresh)
    ec.check_parity(again, *ec.references(y), "weights halved in place", RATIOS)


def test_each_pass_refuses_a_backward_after_its_own_later_forward_only():
    x = ec.make_inputs("fixture_b33")
    m = ec.Module(x, DEV)
    tp = train.FusedTrainPassEE(m)
    f, c, y, t = dev(x["features"]), dev(x["critic_obs"]), dev(x["labels"]), dev(x["terminated"])
    mu1, _, _ = tp(f, c)
    mu2, _, values2 = tp(f, c)
    with pytest.raises(RuntimeError, match=r"FusedTrainPassEE: backward of RL forward call 1, but RL forward call 2 has overwritten"):
        mu1.sum().backward()
    assert all(p.grad is None for p in m.parameters())
    l1 = tp.estimator_loss(f, y, t)
    l2 = tp.estimator_loss(f, y, t)
    with pytest.raises(RuntimeError, match=r"FusedTrainPassEE: backward of estimator forward call 1, but estimator forward call 2 has overwritten"):
        l1.backward()
    assert all(p.grad is None for p in m.parameters())
    # the passes do not invalidate each other: an RL forward behind the estimator forward, then both backwards, newest first or not
    mu3, _, values3 = tp(f, c)
    l2.backward()
    (mu3.sum() + values3.sum()).backward()
    assert all(p.grad is not None for p in m.parameters())
    l4 = tp.estimator_loss(f, y, t)
    with pytest.raises(RuntimeError, match=r"RL forward call 2, but RL forward call 3"):
        (mu2.sum() + values2.sum()).backward()
    mu5, _, _ = tp(f[:9], c[:9])
    l4.backward()                                                      # the RL forward in between left the estimator's workspace alone
    mu5.sum().backward()
    # and the interleaved results are those of the passes run apart
    for p in m.parameters():
        p.grad = None
    apart, _, _ = run(x, m, tp)
    for p in m.parameters():
        p.grad = None
    loss = tp.estimator_loss(f, y, t)
    mu, sigma, values = tp(f, c)
    (loss * float(x["upstream"])).backward()
    torch.autograd.backward([mu, sigma, values], [dev(x[k]) for k in COTANGENTS])
    torch.cuda.synchronize()
    got = ec.named(x, dict(mu=host(mu), sigma=host(sigma), values=host(values)), [host(p.grad) for p in m.rl_parameters()], host(loss),
                   [host(p.grad) for p in m.estimator_parameters()])
    assert same_bits(got, apart)


def test_rl_backward_leaves_the_estimators_grad_untouched():
    x = ec.make_inputs("fixture_b257")
    m = ec.Module(x, DEV)
    tp = train.FusedTrainPassEE(m)
    marks = []
    for i, p in enumerate(m.estimator_parameters()):
        p.grad = torch.full_like(p, 3.5 + i)
        marks.append((p.grad, host(p.grad).copy()))
    mu, sigma, values = tp(dev(x["features"]), dev(x["critic_obs"]))
    torch.autograd.backward([mu, sigma, values], [dev(x[k]) for k in COTANGENTS])
    torch.cuda.synchronize()
    for p, (g, before) in zip(m.estimator_parameters(), marks):
        assert p.grad is g and np.array_equal(host(p.grad), before)
    assert all(p.grad is not None for p in m.rl_parameters())
    # torch's autograd would have sent something there: the gradient the reference discards unread
    assert any(np.abs(g).max() > 0 for g in ec.torch_passes(x)["est_rl_grads"])


def test_a_fully_masked_batch_gives_zero_loss_and_zero_gradients():
    x = ec.make_inputs("fixture_b257")
    x["terminated"] = np.zeros_like(x["terminated"])
    got, _, _ = run(x)
    assert got["loss"][0] == 0.0
    assert all((got[n] == 0).all() for n in ec.est_names(x["est"]))


# ---- non-finite values ------------------------------------------------------------------------------------------------------------------------
def test_a_nan_row_stays_in_its_row_and_reaches_what_torch_reaches():
    x = ec.make_inputs("fixture_b257")
    clean, _, _ = run(x)
    row = int(np.flatnonzero(x["terminated"][:, 0] == 1)[5])                 # an unmasked row
    y = dict(x, features=x["features"].copy())
    y["features"][row, 2] = np.nan
    got, _, _ = run(y)
    others = np.arange(257) != row
    assert np.isnan(got["mu"][row]).all() and np.isnan(got["sigma"][row]).all()
    for k in ("mu", "sigma"):
        assert np.array_equal(got[k][others].view(np.uint32), clean[k][others].view(np.uint32))
    rl, est = ec.rl_names(x["actor"], x["critic"]), ec.est_names(x["est"])
    for n in ["values"] + [n for n in rl if n.startswith("critic")]:         # the critic read another matrix: not a bit changes
        assert np.array_equal(got[n].view(np.uint32), clean[n].view(np.uint32)), n
    assert np.array_equal(got["std"].view(np.uint32), clean["std"].view(np.uint32))
    theirs = ec.torch_passes(y)
    assert np.isnan(theirs["loss"]) and np.isnan(got["loss"][0])
    for n, g in list(zip(rl, theirs["rl_grads"])) + list(zip(est, theirs["est_grads"])):
        assert (np.isnan(got[n]) | ~np.isnan(g)).all(), n                      # wherever torch's gradient is NaN, so is the kernel's
    assert np.isnan(got["actor.0.weight"][:, 2]).all() and np.isnan(got["estimator.0.weight"][:, 2]).all()
    # in a masked row the loss is still NaN (the mask is a multiplication), and the RL outputs behave as above
    masked = int(np.flatnonzero(x["terminated"][:, 0] == 0)[2])
    z = dict(x, features=x["features"].copy())
    z["features"][masked, 0] = np.nan
    got, _, _ = run(z)
    assert np.isnan(got["loss"][0]) and np.isnan(ec.torch_passes(z)["loss"])
    others = np.arange(257) != masked
    assert np.isnan(got["mu"][masked]).all() and np.array_equal(got["mu"][others].view(np.uint32), clean["mu"][others].view(np.uint32))
    # the same through the critic: values of that row only
    w = dict(x, critic_obs=x["critic_obs"].copy())
    w["critic_obs"][256, 0] = np.inf
    got, _, _ = run(w)
    assert not np.isfinite(got["values"][256]).any() and np.array_equal(got["values"][:256].view(np.uint32), clean["values"][:256].view(np.uint32))
    for n in ["mu", "sigma", "std", "loss"] + [n for n in rl if n.startswith("actor")] + est:
        assert np.array_equal(got[n].view(np.uint32), clean[n].view(np.uint32)), n


def test_zz_print_the_parity_ratios():
    """Not a check of its own: the worst |kernel - f64| / max(|torch-f32 - f64|, ulp) per tensor class over every parity check above, for
    DESIGN.md's table."""
    tg.print_parity_ratios(RATIOS)

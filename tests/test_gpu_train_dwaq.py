"""The DreamWaQ learner passes on the GPU (hcr_genesis_lr_cl_amd/train.py's FusedTrainPassDreamWaQ, csrc/lg_train_dwaq.hip) against the
float64 restatement of tests/train_dwaq_cases.py under the project's parity rule, and their conventions: the reference's whole
PPO_DreamWaQ.update() end to end (6 RL steps with 2 VAE steps behind each; FusedTrainPassDreamWaQ, FusedPPOLoss, two FusedAdams),
bit-identical repeats, one RL step plus one VAE step as a HIP graph with caller-owned noise, strided views, weights changed in place, the
stale-forward refusal per pass, the VAE's .grad left alone by the RL backward and the actor's, critic's and std's by the VAE backward, the
fully masked batch, the saturated log-variance column that passes nothing through its head, and the NaN row."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from hcr_genesis_lr_cl_amd import optim, ppo_loss, train
from tests import train_dwaq_cases as dc
from tests import train_gpu as tg
from tests.train_gpu import COTANGENTS, DEV, dev, host, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ppo_dwaq_train.npz")
RATIOS = []
VAE_INPUTS = ("obs_history", "labels", "next_states", "terminated", "vae_noise")


def losses_of(out):
    return host(torch.stack([out.loss.detach(), out.explicit_estimation_loss, out.reconstruction_loss, out.kld_loss])).astype(np.float64)


def run(x, m=None, tp=None):
    """Both passes once on a fresh module: the RL forward and the backward of the case's three cotangents, then the VAE loss and its backward
    under the case's upstream factor.  (name -> numpy array with the four losses under "losses", module, pass).  Asserts on the way that the
    RL backward gave the VAE nothing and that the VAE backward left the RL gradients bit for bit."""
    m = m if m is not None else dc.Module(x, DEV)
    tp = tp if tp is not None else train.FusedTrainPassDreamWaQ(m, kld_weight=x["kld_weight"])
    for p in m.parameters():
        p.grad = None
    mu, sigma, values = tp(dev(x["obs"]), dev(x["obs_history"]), dev(x["critic_obs"]), dev(x["noise"]))
    torch.autograd.backward([mu, sigma, values], [dev(x[k]) for k in COTANGENTS])
    assert all(p.grad is None for p in m.vae_parameters())                    # the RL pass gives the VAE nothing
    rl_grads = [host(p.grad).copy() for p in m.rl_parameters()]
    out = tp.vae_loss(*(dev(x[k]) for k in VAE_INPUTS))
    assert out.loss.requires_grad and not out.kld_loss.requires_grad and out.loss.dim() == 0 and out.kld_loss.device.type == "cuda"
    (out.loss * float(x["upstream"])).backward()
    torch.cuda.synchronize()
    for p, g in zip(m.rl_parameters(), rl_grads):                             # the VAE pass gives the RL parameters nothing
        assert np.array_equal(host(p.grad).view(np.uint32), g.view(np.uint32))
    got = dc.named(x, dict(mu=host(mu), sigma=host(sigma), values=host(values)), rl_grads, [host(p.grad) for p in m.vae_parameters()])
    got["losses"] = losses_of(out)
    return got, m, tp


def check(got, x, label):
    dc.check_case({k: v for k, v in got.items() if k != "losses"}, got["losses"], x, label, RATIOS)


# ---- parity -----------------------------------------------------------------------------------------------------------------------------------
PARITY_CASES = tg.parity_cases(dc)


@pytest.mark.parametrize("name", PARITY_CASES)
def test_parity_on_the_table(name):
    x = tg.case_inputs(dc, name, 1500)
    got, _, _ = run(x)
    check(got, x, name)


def test_the_default_noise_is_one_device_draw_per_call():
    x = dc.make_inputs("fixture_b33")
    m = dc.Module(x, DEV)
    tp = train.FusedTrainPassDreamWaQ(m)
    a = tp(dev(x["obs"]), dev(x["obs_history"]), dev(x["critic_obs"]))
    b = tp(dev(x["obs"]), dev(x["obs_history"]), dev(x["critic_obs"]))
    assert torch.isfinite(a[0]).all() and not torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])      # the critic sees no noise
    out = tp.vae_loss(*(dev(x[k]) for k in VAE_INPUTS[:-1]))
    out.loss.backward()
    assert torch.isfinite(out.loss) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.vae_parameters())


# ---- the whole update -------------------------------------------------------------------------------------------------------------------------
def _init_inputs(fx):
    return dict(dc.fixture_inputs(fx, {k: np.asarray(v, np.float32) for k, v in fx["init"].items()}))


def _torch_update(fx, dtype):
    """The reference's PPO_DreamWaQ.update() on the fixture's columns (rounded to float32 first) in torch ops of `dtype` on the CPU: per
    mini-batch the RL step of tests/train_gpu.torch_rl_step with the host rate rule, then the VAE steps, each optimizer zeroing its own
    gradients only.  Returns (per step in the order they run, the parameters by name as float64 numpy; the RL rates)."""
    cfg = fx["cfg"]
    m = dc.Module(_init_inputs(fx), dtype=dtype)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dtype)
    snap = lambda: {n: p.detach().double().numpy().copy() for n, p in m.named_parameters()}
    betas = (cfg["beta1"], cfg["beta2"])
    rl_opt = torch.optim.Adam(m.rl_parameters(), lr=cfg["lr0"], betas=betas, eps=cfg["eps"])
    vae_opt = torch.optim.Adam(m.vae_parameters(), lr=cfg["encoder_lr"], betas=betas, eps=cfg["eps"])
    lr, lrs, out = cfg["lr0"], [], []
    for s in range(cfg["steps"]):
        c = {k: t(fx[k][s]) for k in dc.FIXTURE_COLUMNS}
        loss, kl = tg.torch_rl_step(m(c["obs"], c["obs_history"], c["critic_obs"], c["noise"]), c, cfg)
        lr = ppo_loss.adjust_learning_rate(kl, lr, cfg["desired_kl"])
        for group in rl_opt.param_groups:
            group["lr"] = lr
        rl_opt.zero_grad()
        loss.backward()
        nn.utils.clip_grad_norm_(m.rl_parameters(), cfg["max_grad_norm"])
        rl_opt.step()
        lrs.append(lr)
        out.append(snap())
        for v in range(cfg["vae_epochs"] * s, cfg["vae_epochs"] * (s + 1)):
            losses = m.vae_loss(*(t(fx[k][v]) for k in ("vae_history", "vae_labels", "vae_next_states", "vae_terminated", "vae_noise")))
            vae_opt.zero_grad()
            losses[0].backward()
            nn.utils.clip_grad_norm_(m.vae_parameters(), cfg["max_grad_norm"])
            vae_opt.step()
            out.append(snap())
    return out, lrs


class _Learner:
    """FusedTrainPassDreamWaQ + FusedPPOLoss + two FusedAdams on a module: the fused PPO_DreamWaQ mini-batch steps."""

    def __init__(self, m, cfg):
        self.tp = train.FusedTrainPassDreamWaQ(m, kld_weight=cfg["kld_weight"])
        self.loss_fn = ppo_loss.FusedPPOLoss(clip_param=cfg["clip_param"], value_loss_coef=cfg["value_loss_coef"], entropy_coef=cfg["entropy_coef"])
        betas = (cfg["beta1"], cfg["beta2"])
        self.rl_opt = optim.FusedAdam(list(zip(self.tp.spec.rl_parameter_names(), self.tp.rl_parameters())), lr=cfg["lr0"], betas=betas, eps=cfg["eps"],
                                      max_grad_norm=cfg["max_grad_norm"], desired_kl=cfg["desired_kl"])
        self.vae_opt = optim.FusedAdam(list(zip(self.tp.spec.vae_parameter_names(), self.tp.vae_parameters())), lr=cfg["encoder_lr"],
                                       betas=betas, eps=cfg["eps"], max_grad_norm=cfg["max_grad_norm"])
        self.optimizers = (self.rl_opt, self.vae_opt)

    def rl_step(self, c):
        mu, sigma, values = self.tp(c["obs"], c["obs_history"], c["critic_obs"], c["noise"])
        out = self.loss_fn(mu, sigma, values, c["actions"], c["old_log_prob"], c["advantages"], c["returns"], c["target_values"], c["old_mu"], c["old_sigma"])
        self.rl_opt.zero_grad()
        out.loss.backward()
        self.rl_opt.step(kl_mean=out.kl_mean)
        return out

    def vae_step(self, e):
        out = self.tp.vae_loss(e["vae_history"], e["vae_labels"], e["vae_next_states"], e["vae_terminated"], e["vae_noise"])
        self.vae_opt.zero_grad()
        out.loss.backward()
        self.vae_opt.step()
        return out

    def step(self, b):
        """One RL step and one VAE step on a batch that holds the columns of both."""
        self.rl_step(b)
        self.vae_step(b)


def test_fixture_update_end_to_end():
    """The reference's PPO_DreamWaQ.update(), 6 RL steps with 2 VAE steps behind each, through FusedTrainPassDreamWaQ, FusedPPOLoss and two
    FusedAdams: the learning rates are the fixture's, the four VAE losses are the fixture's to float32 accuracy, and every parameter after
    each of the 18 steps lies within the parity rule of the float64 run of the same torch code on the float32 inputs (its float32 side: that
    code in float32 on the CPU); that float64 run is the fixture up to the rounding of its inputs."""
    fx = dc.load_fixture(FIXTURE)
    cfg = fx["cfg"]
    ref64, lrs64 = _torch_update(fx, torch.float64)
    ref32, lrs32 = _torch_update(fx, torch.float32)
    assert lrs64 == lrs32 == [float(v) for v in fx["lr"]]
    assert max(np.abs(ref64[-1][n] - fx["vae_params"][-1][n]).max() for n in fx["names"]) < 1e-5
    m = dc.Module(_init_inputs(fx), DEV)
    learner = _Learner(m, cfg)
    rl, vae = tg.fixture_batches(fx, dc.FIXTURE_COLUMNS, cfg["steps"]), tg.fixture_batches(fx, dc.VAE_COLUMNS, cfg["vae_steps"])
    at = 0
    for s in range(cfg["steps"]):
        learner.rl_step(rl[s])
        assert learner.rl_opt.lr == float(fx["lr"][s]), (s, learner.rl_opt.lr, fx["lr"][s])
        tg.check_parameters({n: host(p) for n, p in m.named_parameters()}, ref64[at], ref32[at], at, RATIOS)
        at += 1
        for v in range(cfg["vae_epochs"] * s, cfg["vae_epochs"] * (s + 1)):
            out = learner.vae_step(vae[v])
            assert np.abs(losses_of(out) - fx["vae_losses"][v]).max() < 1e-4 * np.abs(fx["vae_losses"][v]).max(), (v, losses_of(out), fx["vae_losses"][v])
            tg.check_parameters({n: host(p) for n, p in m.named_parameters()}, ref64[at], ref32[at], at, RATIOS)
            at += 1
    assert learner.rl_opt.step_count == cfg["steps"] and learner.vae_opt.step_count == cfg["vae_steps"]


def test_captured_steps_replay_like_eager_steps():
    """One RL step plus one VAE step captured on one stream as a HIP graph and replayed three times with the mini-batches AND the two noise
    tensors (caller-owned) rewritten in place in between: every parameter, the rate and the step counts are those of three eager pairs of
    steps, bit for bit."""
    fx = dc.load_fixture(FIXTURE)
    x = _init_inputs(fx)
    both = [{**c, **e} for c, e in zip(tg.fixture_batches(fx, dc.FIXTURE_COLUMNS, 3), tg.fixture_batches(fx, dc.VAE_COLUMNS, 3))]
    tg.replays_like_eager_steps(lambda: dc.Module(x, DEV), lambda m: _Learner(m, fx["cfg"]), both)


# ---- determinism, addressing, state -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fixture_b257", "go2_dwaq_b257"])
def test_repeats_are_bit_identical(name):
    x = dc.make_inputs(name)
    a, m, tp = run(x)
    b, _, _ = run(x, m, tp)                                           # the same pass again: its workspaces are reused
    c, _, _ = run(x)                                                  # a fresh module and pass
    assert same_bits(a, b) and same_bits(a, c)


def test_strided_views_of_every_matrix_leave_the_gaps_untouched():
    """The C ABI through train.dwaq_args / vae_args on column slices of wider matrices: the same bits as the contiguous call, and every gap
    column keeps its fill."""
    x = dc.make_inputs("fixture_b33")
    x["upstream"] = np.float32(1.0)
    clean, _, _ = run(x)
    m = dc.Module(x, DEV)
    D = m.std.device
    spec = train.describe_dwaq(m, D)
    f = dc.NETS["fixture"]
    B, FILL = 33, 7.25
    wide = {k: torch.full((B, w), FILL, device=DEV) for k, w in (("in", 72), ("out", 16), ("grad", 19))}
    cols = dict(obs=(1, 8), obs_history=(10, 24), critic_obs=(26, 35), noise=(37, 42), labels=(44, 46), next_states=(48, 53), terminated=(55, 56),
                vae_noise=(58, 63))
    v = {k: wide["in"][:, a:b] for k, (a, b) in cols.items()}
    mu, sigma, values = wide["out"][:, 1:4], wide["out"][:, 6:9], wide["out"][:, 13:14]
    gm, gs, gv = wide["grad"][:, 2:5], wide["grad"][:, 9:12], wide["grad"][:, 17:18]
    for view, k in [(v[k], k) for k in cols] + [(gm, "grad_mu"), (gs, "grad_sigma"), (gv, "grad_values")]:
        view.copy_(dev(x[k]))
    before = {k: host(t).copy() for k, t in wide.items()}
    ws = torch.empty(int(train.plan_dwaq(B, *f[:3], *f[4:]).workspace_floats), device=DEV)
    rl_in = (v["obs"], v["obs_history"], v["critic_obs"], v["noise"])
    train._call("lg_train_dwaq_forward", train.dwaq_args(spec, *rl_in, mu, sigma, values, ws, device=D), D)
    rl_grads = [torch.full_like(p, FILL) for p in spec.rl_parameters()]
    a = train.dwaq_args(spec, *rl_in, mu, sigma, values, ws, rl_grads, gm, gs, gv, device=D)
    assert (a.chain[0].in_stride, a.chain[5].in_stride, a.chain[6].in_stride, a.noise_stride, a.mu_stride, a.grad_sigma_stride) == (72, 72, 72, 72, 16, 19)
    train._call("lg_train_dwaq_backward", a, D)
    vws = torch.empty(int(train.plan_vae(B, *f[:4]).workspace_floats), device=DEV)
    pad = torch.full((12,), FILL, device=DEV)
    losses, up = pad[4:8], torch.ones(1, device=DEV)
    vae_in = (v["obs_history"], v["labels"], v["next_states"], v["terminated"], v["vae_noise"])
    train._call("lg_train_vae_forward", train.vae_args(spec, *vae_in, x["kld_weight"], losses, vws, device=D), D)
    vae_grads = [torch.full_like(p, FILL) for p in spec.vae_parameters()]
    e = train.vae_args(spec, *vae_in, x["kld_weight"], None, vws, vae_grads, up, device=D)
    assert (e.chain[0].in_stride, e.labels_stride, e.next_states_stride, e.mask_stride, e.noise_stride) == (72, 72, 72, 72, 72)
    train._call("lg_train_vae_backward", e, D)
    torch.cuda.synchronize()
    got = dc.named(x, dict(mu=host(mu), sigma=host(sigma), values=host(values)), [host(g) for g in rl_grads], [host(g) for g in vae_grads])
    got["losses"] = host(losses).astype(np.float64)
    assert same_bits(got, clean)
    after = {k: host(t) for k, t in wide.items()}
    assert np.array_equal(after["in"], before["in"]) and np.array_equal(after["grad"], before["grad"])
    gaps = np.ones(16, bool)
    gaps[[1, 2, 3, 6, 7, 8, 13]] = False
    assert (after["out"][:, gaps] == FILL).all() and (host(pad)[[0, 1, 2, 3, 8, 9, 10, 11]] == FILL).all()


def test_weights_changed_in_place_are_seen():
    x = dc.make_inputs("fixture_b33")
    _, m, tp = run(x)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(0.5)
    y = dict(x, rl_params=[host(p).copy() for p in m.rl_parameters()], vae_params=[host(p).copy() for p in m.vae_parameters()])
    again, _, _ = run(y, m, tp)
    fresh, _, _ = run(y)
    assert same_bits(again, fresh)
    # halving the weights moves the means and the log-variances under the clips the case placed; none of them ends near its clip
    fr = dc.front(y, y["obs_history"])
    assert np.abs(np.abs(np.concatenate([fr["pre"][1], fr["pre"][3]], axis=1)) - y["var_clip"]).min() >= 1e-3
    assert np.abs(np.abs(dc.rl_forward(dict(y, clip=None))["mu"]) - y["clip"]).min() >= 1e-3
    check(again, y, "weights halved in place")


def test_each_pass_refuses_a_backward_after_its_own_later_forward_only():
    x = dc.make_inputs("fixture_b33")
    m = dc.Module(x, DEV)
    tp = train.FusedTrainPassDreamWaQ(m, kld_weight=x["kld_weight"])
    o, h, c, n = (dev(x[k]) for k in ("obs", "obs_history", "critic_obs", "noise"))
    vin = tuple(dev(x[k]) for k in VAE_INPUTS)
    mu1, _, _ = tp(o, h, c, n)
    mu2, _, values2 = tp(o, h, c, n)
    with pytest.raises(RuntimeError, match=r"FusedTrainPassDreamWaQ: backward of RL forward call 1, but RL forward call 2 has overwritten"):
        mu1.sum().backward()
    assert all(q.grad is None for q in m.parameters())
    l1 = tp.vae_loss(*vin)
    l2 = tp.vae_loss(*vin)
    with pytest.raises(RuntimeError, match=r"FusedTrainPassDreamWaQ: backward of VAE forward call 1, but VAE forward call 2 has overwritten"):
        l1.loss.backward()
    assert all(q.grad is None for q in m.parameters())
    # the passes do not invalidate each other: an RL forward behind the VAE forward, then both backwards, newest first or not
    mu3, _, values3 = tp(o, h, c, n)
    l2.loss.backward()
    (mu3.sum() + values3.sum()).backward()
    assert all(q.grad is not None for q in m.parameters())
    l4 = tp.vae_loss(*vin)
    with pytest.raises(RuntimeError, match=r"RL forward call 2, but RL forward call 3"):
        (mu2.sum() + values2.sum()).backward()
    mu5, _, _ = tp(o[:9], h[:9], c[:9], n[:9])
    l4.loss.backward()                                                 # the RL forward in between left the VAE's workspace alone
    mu5.sum().backward()
    # and the interleaved results are those of the passes run apart
    apart, _, _ = run(x, m, tp)
    for q in m.parameters():
        q.grad = None
    out = tp.vae_loss(*vin)
    mu, sigma, values = tp(o, h, c, n)
    (out.loss * float(x["upstream"])).backward()
    torch.autograd.backward([mu, sigma, values], [dev(x[k]) for k in COTANGENTS])
    torch.cuda.synchronize()
    got = dc.named(x, dict(mu=host(mu), sigma=host(sigma), values=host(values)), [host(q.grad) for q in m.rl_parameters()],
                   [host(q.grad) for q in m.vae_parameters()])
    got["losses"] = losses_of(out)
    assert same_bits(got, apart)


def test_each_backward_leaves_the_other_parameters_grad_untouched():
    x = dc.make_inputs("fixture_b257")
    m = dc.Module(x, DEV)
    tp = train.FusedTrainPassDreamWaQ(m, kld_weight=x["kld_weight"])

    def mark(params):
        out = []
        for i, p in enumerate(params):
            p.grad = torch.full_like(p, 3.5 + i)
            out.append((p, p.grad, host(p.grad).copy()))
        return out
    marks = mark(m.vae_parameters())
    mu, sigma, values = tp(dev(x["obs"]), dev(x["obs_history"]), dev(x["critic_obs"]), dev(x["noise"]))
    torch.autograd.backward([mu, sigma, values], [dev(x[k]) for k in COTANGENTS])
    torch.cuda.synchronize()
    for p, g, before in marks:                                        # the RL backward: every vae .grad is the same tensor, same bits
        assert p.grad is g and np.array_equal(host(p.grad), before)
    assert all(p.grad is not None for p in m.rl_parameters())
    for p in m.parameters():
        p.grad = None
    marks = mark(m.rl_parameters())
    tp.vae_loss(*(dev(x[k]) for k in VAE_INPUTS)).loss.backward()
    torch.cuda.synchronize()
    for p, g, before in marks:                                        # the VAE backward: actor, critic and std likewise
        assert p.grad is g and np.array_equal(host(p.grad), before)
    assert all(p.grad is not None and np.abs(host(p.grad)).max() > 0 for p in m.vae_parameters())


def test_a_fully_masked_batch_gives_zero_losses_and_zero_gradients():
    """t = 0 everywhere: the estimation and reconstruction losses and their gradients are zero, and so is the KL term, by the broadcast
    (its factor is T / B^2 = 0 for every row)."""
    x = dc.make_inputs("fixture_b257")
    x["terminated"] = np.zeros_like(x["terminated"])
    got, _, _ = run(x)
    assert (got["losses"] == 0.0).all()
    assert all((got[n] == 0).all() for n in dc.vae_names(x["enc"], x["dec"]))


def test_a_saturated_log_variance_column_passes_nothing_through_its_head():
    """Column 0 of latent_var far above the clip in every row: row 0 of that head's weight gradient and its bias gradient's element 0 are
    exactly zero; with the clip out of reach they are not."""
    x = dc.make_inputs("fixture_b33")
    names = dc.vae_names(x["enc"], x["dec"])
    x["vae_params"] = [p.copy() for p in x["vae_params"]]
    x["vae_params"][names.index("vae.latent_var.0.bias")][0] = 50.0
    got, _, _ = run(x)
    assert (got["vae.latent_var.0.weight"][0] == 0).all() and got["vae.latent_var.0.bias"][0] == 0 and np.abs(got["vae.latent_var.0.weight"][1:]).max() > 0
    check(got, x, "a saturated log-variance column")
    free, _, _ = run(dict(x, var_clip=100.0))
    assert np.abs(free["vae.latent_var.0.weight"][0]).max() > 0 and free["vae.latent_var.0.bias"][0] != 0


# ---- non-finite values ------------------------------------------------------------------------------------------------------------------------
def test_a_nan_row_stays_in_its_row_and_reaches_what_torch_reaches():
    x = dc.make_inputs("fixture_b257")
    clean, _, _ = run(x)
    rl, vae = dc.rl_names(x["actor"], x["critic"]), dc.vae_names(x["enc"], x["dec"])
    bits = lambda a, b: np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
    row = int(np.flatnonzero(x["terminated"][:, 0] == 1)[5])                 # an unmasked row
    y = dict(x, obs_history=x["obs_history"].copy())
    y["obs_history"][row, 2] = np.nan                                        # through the encoder, the heads and the draw into the actor
    got, _, _ = run(y)
    others = np.arange(257) != row
    assert np.isnan(got["mu"][row]).all() and np.isnan(got["sigma"][row]).all()
    for k in ("mu", "sigma"):
        assert bits(got[k][others], clean[k][others])
    for n in ["values", "std"] + [n for n in rl if n.startswith("critic")]:  # the critic read another matrix: not a bit changes
        assert bits(got[n], clean[n]), n
    theirs = dc.torch_passes(y)
    assert np.isnan(theirs["losses"]).all() and np.isnan(got["losses"]).all()      # the row's v, rec and s are NaN
    for n, g in list(zip(rl, theirs["rl_grads"])) + list(zip(vae, theirs["vae_grads"])):
        assert (np.isnan(got[n]) | ~np.isnan(g)).all(), n                      # wherever torch's gradient is NaN, so is the kernel's
    assert np.isnan(got["vae.encoder.0.weight"][:, 2]).all() and np.isnan(theirs["vae_grads"][0][:, 2]).all()
    # a NaN observation: the actor only
    y = dict(x, obs=x["obs"].copy())
    y["obs"][row, 1] = np.nan
    got, _, _ = run(y)
    theirs = dc.torch_passes(y)
    assert np.isnan(got["mu"][row]).all() and bits(got["mu"][others], clean["mu"][others])
    for n, g in zip(rl, theirs["rl_grads"]):
        assert (np.isnan(got[n]) | ~np.isnan(g)).all(), n
    assert np.isnan(got["actor.0.weight"][:, 1]).all()
    assert np.isfinite(got["losses"]).all() and all(bits(got[n], clean[n]) for n in vae + ["losses"])      # the VAE pass never reads obs
    # a NaN target in a MASKED row: the reconstruction loss and the total are NaN (the mask is a multiplication), the other two are not
    masked = int(np.flatnonzero(x["terminated"][:, 0] == 0)[2])
    z = dict(x, next_states=x["next_states"].copy())
    z["next_states"][masked, 0] = np.nan
    got, _, _ = run(z)
    theirs = dc.torch_passes(z)
    assert list(np.isnan(got["losses"])) == list(np.isnan(theirs["losses"])) == [True, False, True, False]
    for n, g in zip(vae, theirs["vae_grads"]):
        assert (np.isnan(got[n]) | ~np.isnan(g)).all(), n
    for n in ["mu", "sigma", "values"] + rl:                                 # the RL pass never reads the targets
        assert bits(got[n], clean[n]), n
    # the same through the critic: values of that row only
    w = dict(x, critic_obs=x["critic_obs"].copy())
    w["critic_obs"][256, 0] = np.inf
    got, _, _ = run(w)
    assert not np.isfinite(got["values"][256]).any() and bits(got["values"][:256], clean["values"][:256])
    for n in ["mu", "sigma", "std", "losses"] + [n for n in rl if not n.startswith("critic")] + vae:
        assert bits(got[n], clean[n]), n


def test_zz_print_the_parity_ratios():
    """Not a check of its own: the worst |kernel - f64| / max(|torch-f32 - f64|, ulp) per tensor class over every parity check above, for
    DESIGN.md's table."""
    tg.print_parity_ratios(RATIOS)

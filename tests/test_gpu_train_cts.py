"""The concurrent teacher-student learner passes on the GPU (hcr_genesis_lr_cl_amd/train.py's FusedTrainPassCTS, csrc/lg_train_cts.hip and the
encoder kernels of csrc/lg_train_ts.hip) against the float64 restatement of tests/train_cts_cases.py under the project's parity rule, and
their conventions: the reference's whole PPO_CTS.update() end to end (6 RL steps, 12 encoder steps; FusedTrainPassCTS, FusedPPOLoss.cts, two
FusedAdams), one RL step plus one encoder step as a HIP graph, the .grad each pass leaves alone, bit-identical repeats, a NaN row in the teacher's, the student's and the critic's input,
strided 16-byte rows of every input, output and cotangent, and the stale-forward refusal."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from hcr_genesis_lr_cl_amd import optim, ppo_loss, train
from tests import train_cts_cases as cc
from tests import train_gpu as tg
from tests.train_gpu import DEV, dev, host, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ppo_cts_train.npz")
RATIOS = []
RL_INPUTS = ("teacher_obs", "teacher_privileged_obs", "student_obs", "student_obs_history", "critic_obs")
ENC_INPUTS = ("student_obs_history", "student_privileged_obs")


def run(x, m=None, tp=None):
    """Both passes once on a fresh module: the RL forward and the backward of the case's five cotangents, then the encoder loss and its
    backward under the case's upstream factor.  (name -> numpy array, module, pass).  Asserts on the way that the RL backward gave the
    history encoder nothing and that the encoder backward left the RL parameters' gradients bit for bit."""
    m = m if m is not None else cc.Module(x, DEV)
    tp = tp if tp is not None else train.FusedTrainPassCTS(m)
    for p in m.parameters():
        p.grad = None
    outs = tp(*(dev(x[k]) for k in RL_INPUTS))
    torch.autograd.backward(list(outs), [dev(x[k]) for k in cc.COTANGENTS])
    assert all(p.grad is None for p in m.encoder_parameters())                # the RL pass gives the history encoder nothing
    rl_grads = [host(p.grad).copy() for p in m.rl_parameters()]
    loss = tp.encoder_loss(*(dev(x[k]) for k in ENC_INPUTS))
    (loss * float(x["upstream"])).backward()
    torch.cuda.synchronize()
    for p, g in zip(m.rl_parameters(), rl_grads):                             # the encoder pass gives the RL parameters nothing
        assert np.array_equal(host(p.grad).view(np.uint32), g.view(np.uint32))
    got = cc.named(x, dict(zip(cc.OUTPUTS, (host(o) for o in outs))), rl_grads, host(loss), [host(p.grad) for p in m.encoder_parameters()])
    return got, m, tp


# ---- parity -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.CASES))
def test_parity_on_the_table(name):
    x = cc.make_inputs(name)
    got, _, tp = run(x)
    c = cc.CASES[name]
    assert list(tp.plan(c["Bt"], c["Bs"], c["Bc"]).tiles) == cc.restated_plan_cts(c["Bt"], c["Bs"], c["Bc"], *cc.NETS[c["net"]])["tiles"]
    ref64, ref32 = cc.references(x)
    cc.check_parity(got, ref64, ref32, name, RATIOS)


# ---- the whole update -------------------------------------------------------------------------------------------------------------------------
def _init_inputs(fx):
    return dict(cc.fixture_inputs(fx, {k: np.asarray(v, np.float32) for k, v in fx["init"].items()}))


def _log_prob(actions, mu, sigma):
    return (-(actions - mu) ** 2 / (2 * sigma ** 2) - sigma.log() - tg.HALF_LOG_2PI).sum(-1)


def _torch_update(fx, dtype):
    """The reference's PPO_CTS.update() on the fixture's columns (rounded to float32 first) in torch ops of `dtype` on the CPU: per RL
    step the two surrogates, the value loss and the entropy over both groups (ppo_cts.py:193-267), the host rate rule on the teacher's KL,
    Adam on rl_params behind the norm clip; then the encoder steps.  Returns (per step, RL steps then encoder steps, the parameters by name
    as float64 numpy; the RL rates)."""
    cfg = fx["cfg"]
    m = cc.Module(_init_inputs(fx), dtype=dtype)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dtype)
    snap = lambda: {n: p.detach().double().numpy().copy() for n, p in m.named_parameters()}
    betas, clip = (cfg["beta1"], cfg["beta2"]), cfg["clip_param"]
    opt = torch.optim.Adam(m.rl_parameters(), lr=cfg["lr0"], betas=betas, eps=cfg["eps"])
    lr, lrs, out = cfg["lr0"], [], []
    for s in range(cfg["steps"]):
        c = {k: t(fx[k][s]) for k in cc.FIXTURE_COLUMNS}
        mu_t, sigma_t, mu_s, sigma_s, value = m(*(c[k] for k in RL_INPUTS))
        with torch.no_grad():
            kl = torch.sum(torch.log(sigma_t / c["teacher_old_sigma"] + 1.e-5) + (c["teacher_old_sigma"] ** 2 + (c["teacher_old_mu"] - mu_t) ** 2)
                           / (2.0 * sigma_t ** 2) - 0.5, dim=-1).mean()
        surrogates = []
        for g, mu, sigma in (("teacher", mu_t, sigma_t), ("student", mu_s, sigma_s)):
            ratio = torch.exp(_log_prob(c[g + "_actions"], mu, sigma) - c[g + "_old_log_prob"].squeeze(-1))
            adv = c[g + "_advantages"].squeeze(-1)
            surrogates.append(torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)).mean())
        vc = c["target_values"] + (value - c["target_values"]).clamp(-clip, clip)
        value_loss = torch.max((value - c["returns"]).pow(2), (vc - c["returns"]).pow(2)).mean()
        entropy = torch.cat([(1.4189385332046727 + sg.log()).sum(-1) for sg in (sigma_t, sigma_s)]).mean()
        loss = cfg["value_loss_coef"] * value_loss + surrogates[0] + surrogates[1] - cfg["entropy_coef"] * entropy
        lr = ppo_loss.adjust_learning_rate(kl, lr, cfg["desired_kl"])
        for group in opt.param_groups:
            group["lr"] = lr
        opt.zero_grad()
        loss.backward()
        nn.utils.clip_grad_norm_(m.rl_parameters(), cfg["max_grad_norm"])
        opt.step()
        lrs.append(lr)
        out.append(snap())
    enc_opt = torch.optim.Adam(m.encoder_parameters(), lr=cfg["encoder_lr"], betas=betas, eps=cfg["eps"])
    for s in range(cfg["enc_steps"]):
        loss = m.encoder_loss(t(fx["enc_history"][s]), t(fx["enc_privileged"][s]))
        enc_opt.zero_grad()                                                  # discards what the RL steps left in the history encoder's .grad
        loss.backward()
        nn.utils.clip_grad_norm_(m.encoder_parameters(), cfg["max_grad_norm"])
        enc_opt.step()
        out.append(snap())
    return out, lrs


class _Learner:
    """FusedTrainPassCTS + FusedPPOLoss.cts + two FusedAdams on a module: the fused PPO_CTS mini-batch steps."""

    def __init__(self, m, cfg):
        self.tp = train.FusedTrainPassCTS(m)
        self.loss_fn = ppo_loss.FusedPPOLoss(clip_param=cfg["clip_param"], value_loss_coef=cfg["value_loss_coef"], entropy_coef=cfg["entropy_coef"])
        betas = (cfg["beta1"], cfg["beta2"])
        self.rl_opt = optim.FusedAdam(list(zip(self.tp.spec.rl_parameter_names(), self.tp.rl_parameters())), lr=cfg["lr0"], betas=betas, eps=cfg["eps"],
                                      max_grad_norm=cfg["max_grad_norm"], desired_kl=cfg["desired_kl"])
        self.enc_opt = optim.FusedAdam(list(zip(self.tp.spec.encoder_parameter_names(), self.tp.encoder_parameters())), lr=cfg["encoder_lr"],
                                       betas=betas, eps=cfg["eps"], max_grad_norm=cfg["max_grad_norm"])
        self.optimizers = (self.rl_opt, self.enc_opt)

    def rl_step(self, c):
        mu_t, sigma_t, mu_s, sigma_s, values = self.tp(*(c[k] for k in RL_INPUTS))       # the five outputs feed the loss head directly
        out = self.loss_fn.cts(
            teacher=dict(mu=mu_t, sigma=sigma_t, actions=c["teacher_actions"], old_log_prob=c["teacher_old_log_prob"], advantages=c["teacher_advantages"],
                         old_mu=c["teacher_old_mu"], old_sigma=c["teacher_old_sigma"]),
            student=dict(mu=mu_s, sigma=sigma_s, actions=c["student_actions"], old_log_prob=c["student_old_log_prob"], advantages=c["student_advantages"]),
            values=values, returns=c["returns"], target_values=c["target_values"])
        self.rl_opt.zero_grad()
        out.loss.backward()
        self.rl_opt.step(kl_mean=out.kl_mean)
        return out

    def enc_step(self, e):
        loss = self.tp.encoder_loss(e["enc_history"], e["enc_privileged"])
        self.enc_opt.zero_grad()
        loss.backward()
        self.enc_opt.step()
        return loss

    def step(self, b):
        """One RL step and one encoder step on a batch that holds the columns of both."""
        self.rl_step(b)
        self.enc_step(b)


def test_fixture_update_end_to_end():
    """The reference's PPO_CTS.update(), 6 RL steps then 12 encoder steps, through FusedTrainPassCTS, FusedPPOLoss.cts and two FusedAdams:
    the learning rates are the fixture's and every parameter after each of the 18 steps lies within the parity rule of the float64 run of
    the same torch code on the float32 inputs (its float32 side: that code in float32 on the CPU); that float64 run is the fixture up to
    the rounding of its inputs.  The history encoder's parameters are the reference's although its .grad never saw the RL loss."""
    fx = cc.load_fixture(FIXTURE)
    cfg = fx["cfg"]
    ref64, lrs64 = _torch_update(fx, torch.float64)
    ref32, lrs32 = _torch_update(fx, torch.float32)
    assert lrs64 == lrs32 == [float(v) for v in fx["lr"]]
    assert max(np.abs(ref64[-1][n] - fx["enc_params"][-1][n]).max() for n in fx["names"]) < 1e-5
    assert max(np.abs(ref64[cfg["steps"] - 1][n] - fx["params"][-1][n]).max() for n in fx["names"]) < 1e-5
    m = cc.Module(_init_inputs(fx), DEV)
    learner = _Learner(m, cfg)
    rl, enc = tg.fixture_batches(fx, cc.FIXTURE_COLUMNS, cfg["steps"]), tg.fixture_batches(fx, cc.ENC_COLUMNS, cfg["enc_steps"])
    for s in range(cfg["steps"] + cfg["enc_steps"]):
        if s < cfg["steps"]:
            out = learner.rl_step(rl[s])
            assert learner.rl_opt.lr == float(fx["lr"][s]), (s, learner.rl_opt.lr, fx["lr"][s])
            assert abs(float(out.teacher_surrogate_loss) - fx["teacher_surrogate"][s]) < 1e-4 and abs(float(out.student_surrogate_loss) - fx["student_surrogate"][s]) < 1e-4
            assert all(p.grad is None for p in m.encoder_parameters())
        else:
            loss = learner.enc_step(enc[s - cfg["steps"]])
            assert abs(float(loss.detach()) - fx["enc_loss"][s - cfg["steps"]]) < 1e-4
        tg.check_parameters({n: host(p) for n, p in m.named_parameters()}, ref64[s], ref32[s], s, RATIOS)
    assert learner.rl_opt.step_count == cfg["steps"] and learner.enc_opt.step_count == cfg["enc_steps"]


def test_captured_steps_replay_like_eager_steps():
    """One RL step plus one encoder step captured on one stream as a HIP graph and replayed three times with the mini-batches rewritten in
    place in between: every parameter, the rate and the step counts are those of three eager pairs of steps, bit for bit (the ones column
    of the encoder pass is filled inside the captured region when it is first made there)."""
    fx = cc.load_fixture(FIXTURE)
    x = _init_inputs(fx)
    both = [{**c, **e} for c, e in zip(tg.fixture_batches(fx, cc.FIXTURE_COLUMNS, 3), tg.fixture_batches(fx, cc.ENC_COLUMNS, 3))]
    tg.replays_like_eager_steps(lambda: cc.Module(x, DEV), lambda m: _Learner(m, fx["cfg"]), both)


# ---- the .grad conventions --------------------------------------------------------------------------------------------------------------------
def test_each_backward_leaves_the_other_encoders_grad_untouched():
    x = cc.make_inputs("fixture_above_tile")
    m = cc.Module(x, DEV)
    tp = train.FusedTrainPassCTS(m)

    def mark(params):
        out = []
        for i, p in enumerate(params):
            p.grad = torch.full_like(p, 3.5 + i)
            out.append((p, p.grad, host(p.grad).copy()))
        return out
    marks = mark(m.encoder_parameters())
    outs = tp(*(dev(x[k]) for k in RL_INPUTS))
    torch.autograd.backward(list(outs), [dev(x[k]) for k in cc.COTANGENTS])
    torch.cuda.synchronize()
    for p, g, before in marks:                                        # the RL backward: the history encoder's .grad is the same tensor, same bits
        assert p.grad is g and np.array_equal(host(p.grad), before)
    assert all(p.grad is not None and np.abs(host(p.grad)).max() > 0 for p in m.privilege_encoder.parameters())      # through the teacher's latent
    theirs = cc.torch_passes(x)                                       # torch, by contrast, does send the RL cotangents into the history encoder
    assert any(np.abs(g).max() > 0 for g in theirs["enc_rl_grads"])
    for p in m.parameters():
        p.grad = None
    marks = mark(m.privilege_encoder.parameters())
    tp.encoder_loss(*(dev(x[k]) for k in ENC_INPUTS)).backward()
    torch.cuda.synchronize()
    for p, g, before in marks:                                        # the encoder backward: the privilege encoder's .grad likewise
        assert p.grad is g and np.array_equal(host(p.grad), before)
    assert all(p.grad is not None for p in m.encoder_parameters())
    assert all(p.grad is None for p in list(m.actor.parameters()) + list(m.critic.parameters()) + [m.std])
    # no input gets a gradient: neither the teacher's observations nor the student's [obs | z]
    ins = [dev(x[k]).requires_grad_(True) for k in RL_INPUTS]
    outs = tp(*ins)
    torch.autograd.backward(list(outs), [dev(x[k]) for k in cc.COTANGENTS])
    assert all(i.grad is None for i in ins)


# ---- determinism, addressing, state -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fixture_straddle", "go2_cts"])
def test_repeats_are_bit_identical(name):
    x = cc.make_inputs(name)
    a, m, tp = run(x)
    b, _, _ = run(x, m, tp)                                           # the same pass again: its workspaces are reused
    c, _, _ = run(x)                                                  # a fresh module and pass
    assert same_bits(a, b) and same_bits(a, c)


def _carve(shapes, fill):
    """One wide matrix filled with `fill` and a view of (rows, width) per entry of `shapes`, each starting on a multiple of 4 floats with
    at least 4 floats of gap behind it; the row stride is a multiple of 4 floats, so every view's rows are 16-byte aligned."""
    offs, at = [], 0
    for _, w in shapes:
        offs.append(at)
        at += (w + 3) // 4 * 4 + 4
    wide = torch.full((max(n for n, _ in shapes), at), fill, device=DEV)
    assert wide.stride(0) % 4 == 0 and all(o % 4 == 0 for o in offs)
    return wide, [wide[:n, o:o + w] for (n, w), o in zip(shapes, offs)]


# the fixture net (odd widths: the scalar copies) and a net whose every matrix has rows of whole 16-byte groups (the vector copies under a
# stride; Bt a multiple of 4, so the student's workspace regions take them too)
STRIDED = {"fixture": "fixture_above_tile", "rows16": dict(widths=([8, 6, 4], [16, 9, 4], [12, 5, 1], [20, 7, 4]), Bt=36, Bs=18, Bc=40, seed=1790)}


@pytest.mark.parametrize("which", list(STRIDED))
def test_strided_views_of_every_matrix_leave_the_gaps_untouched(which):
    """The C ABI through train.cts_args on column slices of wider matrices with 16-byte aligned rows, for every input, output and
    cotangent: the same bits as the contiguous call, and every gap column keeps its fill.  The encoder pass the same through
    FusedTrainPassCTS.encoder_loss."""
    x = cc.make_inputs(STRIDED[which])
    x["upstream"] = np.float32(1.0)
    clean, _, _ = run(x)
    m = cc.Module(x, DEV)
    D = m.std.device
    spec = train.describe_cts(m, D)
    bt, bs, bc = (x[k].shape[0] for k in ("teacher_obs", "student_obs", "critic_obs"))
    A, V, FILL = x["actor"][-1], x["critic"][-1], 7.25
    in_keys = RL_INPUTS + ("student_privileged_obs",)
    wide_in, in_views = _carve([x[k].shape for k in in_keys], FILL)
    out_shapes = [(bt, A), (bt, A), (bs, A), (bs, A), (bc, V)]
    wide_out, outs = _carve(out_shapes, FILL)
    wide_cot, cots = _carve(out_shapes, FILL)
    for view, k in list(zip(in_views, in_keys)) + list(zip(cots, cc.COTANGENTS)):
        view.copy_(dev(x[k]))
    ins, s_hist, s_pobs = in_views[:5], in_views[3], in_views[5]
    before = [host(w).copy() for w in (wide_in, wide_cot)]
    ws = torch.empty(int(train.plan_cts(bt, bs, bc, x["priv"], x["actor"], x["critic"], x["hist"]).workspace_floats), device=DEV)
    train._call("lg_train_cts_forward", train.cts_args(spec, *ins, *outs, ws, device=D), D)
    rl_grads = [torch.full_like(p, FILL) for p in spec.rl_parameters()]
    a = train.cts_args(spec, *ins, *outs, ws, rl_grads, *cots, device=D)
    assert {a.chain[i].in_stride for i in range(4)} | {a.student_obs_stride} == {wide_in.stride(0)}
    assert set(a.mu_stride) | set(a.sigma_stride) | {a.values_stride} == {wide_out.stride(0)}
    assert set(a.grad_mu_stride) | set(a.grad_sigma_stride) | {a.grad_values_stride} == {wide_cot.stride(0)}
    train._call("lg_train_cts_backward", a, D)
    tp = train.FusedTrainPassCTS(m)
    loss = tp.encoder_loss(s_hist, s_pobs)
    loss.backward()
    torch.cuda.synchronize()
    got = cc.named(x, dict(zip(cc.OUTPUTS, (host(o) for o in outs))), [host(g) for g in rl_grads], host(loss), [host(p.grad) for p in m.encoder_parameters()])
    assert same_bits(got, clean)
    assert np.array_equal(host(wide_in), before[0]) and np.array_equal(host(wide_cot), before[1])
    written = torch.zeros_like(wide_out, dtype=torch.bool)
    for o in outs:
        written[:o.shape[0], o.storage_offset() % wide_out.stride(0):o.storage_offset() % wide_out.stride(0) + o.shape[1]] = True
    after, written = host(wide_out), host(written)
    assert (after[~written] == FILL).all() and not (after[written] == FILL).any()


def test_each_pass_refuses_a_backward_after_its_own_later_forward_only():
    x = cc.make_inputs("fixture_odd_teacher")
    m = cc.Module(x, DEV)
    tp = train.FusedTrainPassCTS(m)
    ins, enc = [dev(x[k]) for k in RL_INPUTS], [dev(x[k]) for k in ENC_INPUTS]
    first = tp(*ins)
    second = tp(*ins)
    with pytest.raises(RuntimeError, match=r"FusedTrainPassCTS: backward of RL forward call 1, but RL forward call 2 has overwritten"):
        first[0].sum().backward()
    assert all(q.grad is None for q in m.parameters())
    l1 = tp.encoder_loss(*enc)
    l2 = tp.encoder_loss(*enc)
    with pytest.raises(RuntimeError, match=r"FusedTrainPassCTS: backward of encoder forward call 1, but encoder forward call 2 has overwritten"):
        l1.backward()
    assert all(q.grad is None for q in m.parameters())
    # the passes do not invalidate each other
    l2.backward()
    (second[2].sum() + second[4].sum()).backward()
    assert all(q.grad is not None for q in m.parameters())
    # and a refused input grows nothing and counts nothing
    calls = tp._rl.calls
    with pytest.raises(ValueError, match=r"FusedTrainPassCTS: student_obs_history must be \(9, 14\) float32"):
        tp(ins[0], ins[1], ins[2], ins[3][:5], ins[4])
    assert tp._rl.calls == calls


# ---- non-finite values ------------------------------------------------------------------------------------------------------------------------
def _bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_a_nan_row_stays_in_its_row_and_in_its_group():
    x = cc.make_inputs("fixture_above_tile")
    clean, _, _ = run(x)
    rl, enc = cc.rl_names(x["actor"], x["critic"], x["priv"]), cc.enc_names(x["hist"])
    critic = ["values"] + [n for n in rl if n.startswith("critic")]
    # a teacher privileged_obs row: that teacher row of mu / sigma only; the student's outputs, the critic and the encoder pass keep every bit
    row = 5
    y = dict(x, teacher_privileged_obs=x["teacher_privileged_obs"].copy())
    y["teacher_privileged_obs"][row, 2] = np.nan
    got, _, _ = run(y)
    others = np.arange(x["teacher_obs"].shape[0]) != row
    assert np.isnan(got["mu_t"][row]).all() and np.isnan(got["sigma_t"][row]).all()
    assert _bits(got["mu_t"][others], clean["mu_t"][others]) and _bits(got["sigma_t"][others], clean["sigma_t"][others])
    for n in ["mu_s", "sigma_s", "std", "loss"] + critic + enc:
        assert _bits(got[n], clean[n]), n
    theirs = cc.torch_passes(y)
    for n, g in zip(rl, theirs["rl_grads"]):
        assert (np.isnan(got[n]) | ~np.isnan(g)).all(), n                     # wherever torch's gradient is NaN, so is the kernel's
    assert np.isnan(got["privilege_encoder.0.weight"][:, 2]).all() and np.isnan(got["actor.0.weight"]).any()
    # a student obs_history row: that student row only; the teacher's outputs, the privilege encoder's gradients and the critic keep every bit
    row = x["student_obs"].shape[0] - 1                                       # in the ragged last tile
    y = dict(x, student_obs_history=x["student_obs_history"].copy())
    y["student_obs_history"][row, 0] = np.nan
    got, _, _ = run(y)
    assert np.isnan(got["mu_s"][row]).all() and np.isnan(got["sigma_s"][row]).all()
    assert _bits(got["mu_s"][:row], clean["mu_s"][:row]) and _bits(got["sigma_s"][:row], clean["sigma_s"][:row])
    for n in ["mu_t", "sigma_t", "std"] + critic + [n for n in rl if n.startswith("privilege_encoder")]:
        assert _bits(got[n], clean[n]), n
    assert np.isnan(got["actor.0.weight"]).any() and np.isnan(got["loss"][0])   # the shared actor sees it; the encoder pass read the same history
    theirs = cc.torch_passes(y)
    for n, g in zip(rl, theirs["rl_grads"]):
        assert (np.isnan(got[n]) | ~np.isnan(g)).all(), n
    # a critic_obs row: values of that row and the critic's gradients only
    row = x["critic_obs"].shape[0] - 1
    y = dict(x, critic_obs=x["critic_obs"].copy())
    y["critic_obs"][row, 0] = np.nan
    got, _, _ = run(y)
    assert np.isnan(got["values"][row]).all() and _bits(got["values"][:row], clean["values"][:row])
    for n in ["mu_t", "sigma_t", "mu_s", "sigma_s", "std", "loss"] + [n for n in rl if not n.startswith("critic")] + enc:
        assert _bits(got[n], clean[n]), n
    assert np.isnan(got["critic.0.weight"][:, 0]).all()


def test_zz_print_the_parity_ratios():
    """Not a check of its own: the worst |kernel - f64| / max(|torch-f32 - f64|, ulp) per tensor class over every parity check above, for
    DESIGN.md's table."""
    tg.print_parity_ratios(RATIOS)

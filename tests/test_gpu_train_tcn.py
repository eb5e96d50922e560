"""The TCN history-encoder pass on the GPU (hcr_genesis_lr_cl_amd/train.py's FusedTrainPassTSTcn, csrc/lg_train_tcn.hip) against the
float64 restatement of tests/train_tcn_cases.py under the project's parity rule, and its conventions: the reference's whole
PPO_TS.update() on the TCN module end to end (6 RL steps, 12 encoder steps; FusedTrainPassTSTcn, FusedPPOLoss, two FusedAdams),
bit-identical repeats, one RL step plus one encoder step as a HIP graph, the (B, 1, H) and (B, H) inputs, strided views, the upstream
scalar and accumulation, the stale-forward refusal, the NaN history row, the rollout of such a module through FusedPolicy(student=False)
and the workspace's extent."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from hcr_genesis_lr_cl_amd import optim, policy, ppo_loss, rollout, train
from tests import train_gpu as tg
from tests import train_tcn_cases as nc
from tests.train_gpu import DEV, dev, host, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ppo_ts_tcn_train.npz")
RATIOS = []


def read_f(tp, n_rows):
    """f, (n_rows, F), as the conv stack left it in the pass's workspace."""
    p = tp.plan_encoder(n_rows)
    off = int(p.x_off[p.n_conv])
    return host(tp.workspace[off:off + n_rows * p.flat]).reshape(n_rows, p.flat).copy()


def run(x, m=None, tp=None, history=None, terminated=None, upstream=None):
    """The encoder pass once: the loss, its backward under the case's upstream factor.  (name -> numpy array: loss, f and every
    history-encoder gradient; module; pass).  Asserts on the way that nothing reached the other chains."""
    m = m if m is not None else nc.Module(x, DEV)
    tp = tp if tp is not None else train.FusedTrainPassTSTcn(m)
    for p in m.parameters():
        p.grad = None
    h = dev(x["obs_history"]) if history is None else history
    t = dev(x["terminated"]) if terminated is None else terminated
    loss = tp.encoder_loss(h, dev(x["privileged_obs"]), t)
    (loss * float(x["upstream"] if upstream is None else upstream)).backward()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in m.rl_parameters())                     # the target carries no gradient; the RL chains take no part
    B = x["obs_history"].shape[0]
    got = nc.named(x, dict(loss=host(loss), f=read_f(tp, B), grads=[host(p.grad) for p in m.encoder_parameters()]))
    return got, m, tp


# ---- parity -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,b", nc.ALL, ids=nc.IDS)
def test_parity_on_the_table(name, b):
    x = nc.make_inputs(name, b)
    got, _, tp = run(x)
    ref64, ref32 = nc.references(x)
    RATIOS.append((f"{name}_b{b}", nc.check_parity(got, ref64, ref32, f"{name}_b{b}")))
    want = nc.restated_plan(b, x["H"], x["convs"], x["tail"], x["priv"])
    assert tp.workspace.numel() == want["workspace_floats"] == tp.plan_encoder(b).workspace_floats


# ---- the whole update -------------------------------------------------------------------------------------------------------------------------
def _init_inputs(fx):
    return dict(nc.fixture_inputs(fx, {k: np.asarray(v, np.float32) for k, v in fx["init"].items()}))


def _torch_update(fx, dtype):
    """The reference's PPO_TS.update() on the fixture's columns (rounded to float32 first) in torch ops of `dtype` on the CPU: the RL steps
    of tests/train_gpu.torch_rl_update, then the encoder steps through the Conv1d stack.  (the parameters by name after every step; the RL
    rates)."""
    cfg = fx["cfg"]
    m = nc.Module(_init_inputs(fx), dtype=dtype)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dtype)
    snap = lambda: {n: p.detach().double().numpy().copy() for n, p in m.named_parameters()}
    out, lrs = tg.torch_rl_update(fx, nc.FIXTURE_COLUMNS, lambda c: m(c["obs"], c["privileged_obs"], c["critic_obs"]), m.rl_parameters(), snap, dtype)
    enc_opt = torch.optim.Adam(m.encoder_parameters(), lr=cfg["encoder_lr"], betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"])
    for s in range(cfg["enc_steps"]):
        loss = m.encoder_loss(t(fx["enc_history"][s]), t(fx["enc_privileged"][s]), t(fx["enc_terminated"][s]))
        enc_opt.zero_grad()
        loss.backward()
        nn.utils.clip_grad_norm_(m.encoder_parameters(), cfg["max_grad_norm"])
        enc_opt.step()
        out.append(snap())
    return out, lrs


class _Learner:
    """FusedTrainPassTSTcn + FusedPPOLoss + two FusedAdams on a module: the fused PPO_TS mini-batch steps."""

    def __init__(self, m, cfg):
        self.tp = train.FusedTrainPassTSTcn(m)
        self.loss_fn = ppo_loss.FusedPPOLoss(clip_param=cfg["clip_param"], value_loss_coef=cfg["value_loss_coef"], entropy_coef=cfg["entropy_coef"])
        betas = (cfg["beta1"], cfg["beta2"])
        self.rl_opt = optim.FusedAdam(list(zip(self.tp.spec.rl_parameter_names(), self.tp.rl_parameters())), lr=cfg["lr0"], betas=betas, eps=cfg["eps"],
                                      max_grad_norm=cfg["max_grad_norm"], desired_kl=cfg["desired_kl"])
        self.enc_opt = optim.FusedAdam(list(zip(self.tp.spec.encoder_parameter_names(), self.tp.encoder_parameters())), lr=cfg["encoder_lr"],
                                       betas=betas, eps=cfg["eps"], max_grad_norm=cfg["max_grad_norm"])
        self.optimizers = (self.rl_opt, self.enc_opt)

    def rl_step(self, c):
        mu, sigma, values = self.tp(c["obs"], c["privileged_obs"], c["critic_obs"])
        out = self.loss_fn(mu, sigma, values, c["actions"], c["old_log_prob"], c["advantages"], c["returns"], c["target_values"], c["old_mu"], c["old_sigma"])
        self.rl_opt.zero_grad()
        out.loss.backward()
        self.rl_opt.step(kl_mean=out.kl_mean)
        return out

    def enc_step(self, e):
        loss = self.tp.encoder_loss(e["enc_history"], e["enc_privileged"], e["enc_terminated"])
        self.enc_opt.zero_grad()
        loss.backward()
        self.enc_opt.step()
        return loss

    def step(self, b):
        self.rl_step(b)
        self.enc_step(b)


def test_fixture_update_end_to_end():
    """The reference's PPO_TS.update() on the TCN module, 6 RL steps then 12 encoder steps, through FusedTrainPassTSTcn, FusedPPOLoss and
    two FusedAdams: the rates are the fixture's, the encoder parameters are in history_encoder.parameters() order, and every parameter
    after each of the 18 steps lies within the parity rule of the float64 run of the same torch code on the float32 inputs; that float64
    run is the fixture up to the rounding of its inputs."""
    fx = nc.load_fixture(FIXTURE)
    cfg = fx["cfg"]
    ref64, lrs64 = _torch_update(fx, torch.float64)
    ref32, lrs32 = _torch_update(fx, torch.float32)
    assert lrs64 == lrs32 == [float(v) for v in fx["lr"]]
    assert max(np.abs(ref64[-1][n] - fx["enc_params"][-1][n]).max() for n in fx["names"]) < 1e-5
    assert max(np.abs(ref64[cfg["steps"] - 1][n] - fx["params"][-1][n]).max() for n in fx["names"]) < 1e-5
    m = nc.Module(_init_inputs(fx), DEV)
    learner = _Learner(m, cfg)
    assert learner.tp.spec.encoder_parameter_names() == fx["enc_names"] and len(learner.tp.rl_parameters()) == len(fx["rl_names"])
    assert all(a is b for a, b in zip(learner.tp.encoder_parameters(), m.history_encoder.parameters()))
    rl, enc = tg.fixture_batches(fx, nc.FIXTURE_COLUMNS, cfg["steps"]), tg.fixture_batches(fx, nc.ENC_COLUMNS, cfg["enc_steps"])
    for s in range(cfg["steps"] + cfg["enc_steps"]):
        if s < cfg["steps"]:
            learner.rl_step(rl[s])
            assert learner.rl_opt.lr == float(fx["lr"][s]), (s, learner.rl_opt.lr, fx["lr"][s])
        else:
            loss = learner.enc_step(enc[s - cfg["steps"]])
            assert abs(float(loss.detach()) - fx["enc_loss"][s - cfg["steps"]]) < 1e-4
        tg.check_parameters({n: host(p) for n, p in m.named_parameters()}, ref64[s], ref32[s], s, RATIOS)
    assert learner.rl_opt.step_count == cfg["steps"] and learner.enc_opt.step_count == cfg["enc_steps"]


def test_captured_steps_replay_like_eager_steps():
    """One RL step plus one encoder step (forward, backward, FusedAdam each) captured on one stream as a HIP graph and replayed three times
    with the mini-batches rewritten in place in between: every parameter, the rate and the step counts are those of three eager pairs of
    steps, bit for bit."""
    fx = nc.load_fixture(FIXTURE)
    x = _init_inputs(fx)
    both = [{**c, **e} for c, e in zip(tg.fixture_batches(fx, nc.FIXTURE_COLUMNS, 3), tg.fixture_batches(fx, nc.ENC_COLUMNS, 3))]
    tg.replays_like_eager_steps(lambda: nc.Module(x, DEV), lambda m: _Learner(m, fx["cfg"]), both)


# ---- determinism, addressing, state -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,b", [("tiny", 33), ("go2_ts", 129), ("wide", 17)])
def test_repeats_are_bit_identical(name, b):
    x = nc.make_inputs(name, b)
    a, m, tp = run(x)
    again, _, _ = run(x, m, tp)                                       # the same pass again: its workspace is reused
    fresh, _, _ = run(x)                                              # a fresh module and pass
    assert same_bits(a, again) and same_bits(a, fresh)


def test_input_forms_give_the_same_bits():
    """(B, 1, H) as the reference unsqueezes it and (B, H); a row-strided obs_history and a mask of stride > 1: the bits of the contiguous
    call, and the gap columns keep their fill."""
    x = nc.make_inputs("ref90", 31)
    clean, m, tp = run(x)
    h = dev(x["obs_history"])
    three, _, _ = run(x, m, tp, history=h.unsqueeze(1))
    assert same_bits(clean, three)
    FILL = 7.25
    wide = torch.full((31, 128), FILL, device=DEV)
    hist, term = wide[:, 3:93], wide[:, 100:101]
    hist.copy_(h)
    term.copy_(dev(x["terminated"]))
    before = host(wide).copy()
    strided, _, _ = run(x, m, tp, history=hist, terminated=term)
    assert same_bits(clean, strided) and np.array_equal(host(wide), before)
    strided3, _, _ = run(x, m, tp, history=hist.unsqueeze(1), terminated=term)
    assert same_bits(clean, strided3)
    a = train.tcn_args(tp.spec, hist.unsqueeze(1), dev(x["privileged_obs"]), term, torch.zeros((), device=DEV), None, device=m.std.device)
    assert (a.history_stride, a.mask_stride, a.n_history, a.history) == (128, 128, 90, wide.data_ptr() + 12)


def test_upstream_scales_every_gradient_and_backward_twice_accumulates():
    x = nc.make_inputs("odd37", 9)
    one, m, tp = run(x, upstream=1.0)
    four, _, _ = run(x, m, tp, upstream=4.0)                          # a power of two: every product is exact
    names = nc.enc_names(x["convs"], x["tail"])
    assert one["loss"] == four["loss"] and all(np.array_equal(four[n], 4.0 * one[n]) for n in names)
    assert all(np.abs(one[n]).max() > 0 for n in names)
    nc.check_parity(run(x, m, tp, upstream=0.37)[0], *(nc.named(dict(x, upstream=0.37), e) for e in (
        nc.enc_pass(dict(x, upstream=0.37)), nc.torch_pass(dict(x, upstream=0.37)))), "upstream 0.37")
    for p in m.parameters():
        p.grad = None
    args = [dev(x[k]) for k in ("obs_history", "privileged_obs", "terminated")]
    tp.encoder_loss(*args).backward()
    tp.encoder_loss(*args).backward()                                 # autograd accumulates; the kernel overwrites its own buffers
    torch.cuda.synchronize()
    assert all(np.array_equal(host(p.grad), 2.0 * one[n]) for n, p in zip(names, m.encoder_parameters()))


def test_a_backward_whose_forward_was_overwritten_raises():
    x = nc.make_inputs("tiny", 5)
    m = nc.Module(x, DEV)
    tp = train.FusedTrainPassTSTcn(m)
    args = [dev(x[k]) for k in ("obs_history", "privileged_obs", "terminated")]
    l1 = tp.encoder_loss(*args)
    mu, _, values = tp(dev(x["obs"]), dev(x["privileged_obs"]), dev(x["critic_obs"]))       # another pass: its own workspace and counter
    l2 = tp.encoder_loss(*args)
    with pytest.raises(RuntimeError, match=r"FusedTrainPassTSTcn: backward of encoder forward call 1, but encoder forward call 2 has overwritten"):
        l1.backward()
    l2.backward()
    (mu.sum() + values.sum()).backward()
    assert all(p.grad is not None for p in m.parameters())


# ---- non-finite values ------------------------------------------------------------------------------------------------------------------------
def test_a_nan_history_row_stays_in_its_row():
    """A NaN in one (masked) history row: the loss is NaN as in torch (the mask is a multiplication), and every other row's f and gl are
    the clean run's bits."""
    x = nc.make_inputs("ref90", 257)
    clean, m, tp = run(x)
    p = tp.plan_encoder(257)
    Z = x["tail"][-1]
    gl = lambda: host(tp.workspace[int(p.gl_off):int(p.gl_off) + 257 * Z]).reshape(257, Z).copy()
    gl0 = gl()
    row = int(np.flatnonzero(x["terminated"][:, 0] == 0)[2])
    y = dict(x, obs_history=x["obs_history"].copy())
    y["obs_history"][row, 40] = np.nan
    got, _, _ = run(y, m, tp)
    others = np.arange(257) != row
    assert np.isnan(got["loss"][0]) and np.isnan(nc.torch_pass(y)["loss"])
    assert np.isnan(got["f"][row]).any()
    assert np.array_equal(got["f"][others].view(np.uint32), clean["f"][others].view(np.uint32))
    assert np.array_equal(gl()[others].view(np.uint32), gl0[others].view(np.uint32))


# ---- the rollout ------------------------------------------------------------------------------------------------------------------------------
def test_rollout_with_student_false_is_the_mlp_modules_rollout():
    """FusedPolicy(m_tcn, student=False).act into a RolloutStorageTS: bit for bit what FusedPolicy gives on a module with the same actor,
    critic, privilege encoder and std and an MLP history encoder; act_student raises; without student=False the module is refused."""
    x = nc.make_inputs("tiny", 33)
    m_tcn, m_mlp = nc.Module(x, DEV), nc.Module(x, DEV, mlp_history=[x["H"], 4, x["tail"][-1]])
    with pytest.raises(ValueError, match=r"FusedPolicy: history_encoder\[0\] is Conv1d"):
        policy.FusedPolicy(m_tcn, seed=11)
    n, T = 33, 2
    obs, priv, hist, cobs = (dev(x[k]) for k in ("obs", "privileged_obs", "obs_history", "critic_obs"))
    rows = []
    for m, kw in ((m_tcn, dict(student=False)), (m_mlp, {})):
        st = rollout.RolloutStorageTS(n, T, [nc.O], [nc.P], [x["H"]], [nc.C], [nc.A], DEV)
        st.step = 1
        fp = policy.FusedPolicy(m, seed=11, **kw)
        act = fp.act(obs, cobs, storage=st, privileged_obs=priv, obs_history=hist)
        torch.cuda.synchronize()
        assert act.data_ptr() == st.actions[1].data_ptr()
        rows.append({k: host(getattr(st, k)[1]).copy() for k in ("actions", "mu", "sigma", "actions_log_prob", "values")})
        rows[-1]["teacher"] = host(fp.act_teacher(obs, priv)).copy()
        rows[-1]["evaluate"] = host(fp.evaluate(cobs)).copy()
        if kw:
            with pytest.raises(ValueError, match=r"FusedPolicy: act_student runs the history encoder, which student=False left unread"):
                fp.act_student(obs, hist)
            tr = rollout.RolloutStorageTS.Transition()
            fp.fill_transition(tr, obs, cobs, privileged_obs=priv, obs_history=hist)
            assert tr.observation_histories is hist and tr.privileged_observations is priv
    assert same_bits(rows[0], rows[1]) and np.abs(rows[0]["mu"]).max() > 0


# ---- the workspace ----------------------------------------------------------------------------------------------------------------------------
def test_workspace_holds_nothing_outside_the_plan():
    """A workspace longer than the plan, filled with a sentinel: the C entry points write nothing behind workspace_floats, and the pass's
    own workspace is exactly the plan's."""
    x = nc.make_inputs("six", 33)
    clean, m, tp = run(x)
    need = int(tp.plan_encoder(33).workspace_floats)
    assert tp.workspace.numel() == need
    D = m.std.device
    ws = torch.full((need + 4096,), 7.25, device=DEV)
    h, p, t = (dev(x[k]) for k in ("obs_history", "privileged_obs", "terminated"))
    loss, up = torch.zeros((), device=DEV), torch.full((1,), float(x["upstream"]), device=DEV)
    train._call("lg_train_tcn_forward", train.tcn_args(tp.spec, h, p, t, loss, ws, device=D), D)
    grads = [torch.full_like(q, 7.25) for q in tp.encoder_parameters()]
    train._call("lg_train_tcn_backward", train.tcn_args(tp.spec, h, p, t, None, ws, grads, up, device=D), D)
    torch.cuda.synchronize()
    assert (host(ws[need:]) == 7.25).all()
    got = nc.named(x, dict(loss=host(loss), f=host(ws[int(tp.plan_encoder(33).x_off[6]):][:33 * 32]).reshape(33, 32), grads=[host(g) for g in grads]))
    assert same_bits(got, clean)


def test_zz_print_the_parity_ratios():
    """Not a check of its own: the worst |kernel - f64| / max(|torch-f32 - f64|, ulp) per tensor class over every parity check above, for
    DESIGN.md's table."""
    tg.print_parity_ratios(RATIOS)

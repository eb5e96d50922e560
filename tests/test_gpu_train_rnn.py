"""The recurrent learner pass on the GPU (hcr_genesis_lr_cl_amd/train.py's FusedTrainPassRecurrent, csrc/lg_train_rnn.hip) against torch's
own nn.LSTM / nn.GRU, the reference's unpadding and autograd on the CPU in float64 under the project's parity rule (the yardstick: the same
in float32), and its conventions: bit-identical repeats, padding that reaches nothing, a NaN that stays in its trajectory, one update step
as a HIP graph, the reference's whole PPO.update() on ActorCriticRecurrent end to end, and mini-batches straight from RolloutStorage filled
by FusedPolicy."""
import os

import numpy as np
import pytest
import torch

from hcr_genesis_lr_cl_amd import optim, policy, ppo_loss, rollout, train
from tests import train_gpu as tg
from tests import train_rnn_cases as rc
from tests.train_gpu import DEV, dev, host, same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = {k: os.path.join(ROOT, "tests", "golden", f"ppo_recurrent_train_{k}.npz") for k in ("lstm", "gru")}
RATIOS = []
FILL = 7.25          # what the neighbours of a view hold
_REFS = {}


def references(name):
    """(float64, float32) of torch on the CPU for a table case, computed once."""
    if name not in _REFS:
        x = rc.make_inputs(name)
        _REFS[name] = (rc.torch_reference(x, torch.float64), rc.torch_reference(x, torch.float32))
    return _REFS[name]


def batch(x):
    """The four arguments of the pass on the device as the generator yields them: views [:, first:first + n_traj] of a wider padded set,
    the start states as a tensor (GRU) or a list [h, c] (LSTM), hid_c the same object as hid_a where the case shares them."""
    first, n = x["first"], x["n_traj"]
    wide = lambda a, fill: torch.from_numpy(np.concatenate([np.full(a.shape[:1] + (first,) + a.shape[2:], fill, a.dtype), a,
                                                            np.full(a.shape[:1] + (2,) + a.shape[2:], fill, a.dtype)], 1)).to(DEV)[:, first:first + n]
    obs, cobs, masks = wide(x["obs"], FILL), wide(x["critic_obs"], FILL), wide(x["masks"], True)
    hid = []
    for m in "ac":
        h = [dev(x["h0_" + m])] + ([dev(x["c0_" + m])] if x["kind"] == "lstm" else [])
        hid.append(h if len(h) > 1 else h[0])
    if x["shared"]:
        hid[1] = hid[0]
    return obs, cobs, masks, tuple(hid)


def run(x, m=None, tp=None):
    """The forward and the backward of the case's three cotangents on a fresh module: (name -> numpy array, module, pass)."""
    m = m if m is not None else rc.Recurrent(x).to(DEV)
    tp = tp if tp is not None else train.FusedTrainPassRecurrent(m)
    for p in m.parameters():
        p.grad = None
    outs = tp(*batch(x), n_envs=x["E"])
    torch.autograd.backward(list(outs), [dev(x[k]) for k in tg.COTANGENTS])
    torch.cuda.synchronize()
    got = dict(zip(("mu", "sigma", "values"), (host(o) for o in outs)))
    got.update({n: host(p.grad) for n, p in zip(x["names"], m.parameters())})
    return got, m, tp


# ---- parity -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.CASES))
def test_parity_on_the_table(name):
    x = rc.make_inputs(name)
    got, _, tp = run(x)
    assert [n for n in tp.spec.parameter_names()] == x["names"] and len(tp.parameters()) <= 33
    pl, want = tp.plan(x["T"] * x["E"], x["max_len"], x["n_traj"], x["T"]), rc.plan_of_case(x)
    assert (pl.time_row_tile, pl.time_tiles, pl.train.row_tile, pl.workspace_floats) == \
        (want["time_row_tile"], want["time_tiles"], want["train"]["row_tile"], want["workspace_floats"])
    ref64, ref32 = references(name)
    rc.check_parity(got, ref64, ref32, name, RATIOS)


def test_the_table_covers_its_edges():
    """The tiles the case table is there for: 31, 32 and 33 trajectories against the 32-trajectory tile, 9 against the 8-trajectory tile of
    H = 512, every done pattern, both cells at both depths, a view, shared start states, an actor without a Hardtanh."""
    xs = {n: rc.make_inputs(n) for n in rc.CASES if "256" not in n and "512" not in n}
    plans = {n: rc.plan_of_case(x) for n, x in xs.items()}
    assert {x["n_traj"] for n, x in xs.items() if plans[n]["time_row_tile"] == 32} >= {31, 32, 33}
    big = rc.CASES["lstm1_h512_t2"]
    assert rc.plan(14, 2, 9, 2, "lstm", [(1, 512, 45), (1, 512, 61)], [512, 32, 3], [512, 32, 1])["time_row_tile"] == 8 and big["E"] + big["dones"] == 9
    assert {(x["kind"], x["layers"]) for x in xs.values()} == {("lstm", 1), ("lstm", 2), ("gru", 1), ("gru", 2)}
    assert {x["T"] for x in xs.values()} == {1, 2, 6} and any(x["max_len"] < x["T"] for x in xs.values()) and any(x["E"] == 1 for x in xs.values())
    assert any((x["lens"] == 1).sum() >= x["T"] for x in xs.values()) and any(x["n_traj"] == x["E"] and x["T"] > 1 for x in xs.values())
    assert any(x["first"] for x in xs.values()) and any(x["shared"] and x["kind"] == "lstm" for x in xs.values())
    assert any(x["clip"] is None for x in xs.values()) and any(x["clip"] is not None for x in xs.values())


# ---- conventions ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lstm2_h64_t6", "gru2_h65_t2"])
def test_repeats_are_bit_identical(name):
    x = rc.make_inputs(name)
    a, m, tp = run(x)
    b, _, _ = run(x, m, tp)                                           # the same pass again: its workspace is reused
    c, _, _ = run(x)                                                  # a fresh module and pass
    assert same_bits(a, b) and same_bits(a, c)


@pytest.mark.parametrize("name", ["lstm2_h17_short", "gru1_h17_short", "lstm1_h7_t6"])
def test_padding_reaches_nothing(name):
    """NaN in every padded position (and the FILL of the view's neighbours): every output and gradient keeps its bits."""
    clean, _, _ = run(rc.make_inputs(name))
    x = rc.make_inputs(name, pad=np.nan)
    assert np.isnan(x["obs"]).any() and np.isnan(x["critic_obs"]).any()
    got, _, _ = run(x)
    assert same_bits(got, clean)


@pytest.mark.parametrize("name", ["lstm1_h7_t6", "gru2_h65_t2", "lstm2_h64_t6"])
def test_a_nan_step_stays_in_its_trajectory(name):
    """A NaN in one trajectory's observation at step t: that trajectory's rows from t on are NaN, the parameter gradients of the actor's
    side are reached, and no other row of any output changes a bit; the critic's side read other tensors and keeps every bit."""
    x = rc.make_inputs(name)
    clean, _, _ = run(x)
    j = int(np.flatnonzero(x["lens"] >= 2)[1])
    t = 1
    y = dict(x, obs=x["obs"].copy())
    y["obs"][t, j, 2] = np.nan
    got, _, _ = run(y)
    tt, jj, row = rc.positions(x["lens"], x["T"], x["E"])
    hit = np.zeros(x["T"] * x["E"], bool)
    hit[row[(jj == j) & (tt >= t)]] = True
    assert hit.sum() == x["lens"][j] - t
    for k in ("mu", "sigma"):
        assert np.isnan(got[k][hit]).all() and np.array_equal(got[k][~hit].view(np.uint32), clean[k][~hit].view(np.uint32))
    for n in ["values", "std"] + [n for n in x["names"] if n.startswith(("critic", "memory_c"))]:
        assert np.array_equal(got[n].view(np.uint32), clean[n].view(np.uint32)), n
    for n in ("memory_a.rnn.weight_ih_l0", "memory_a.rnn.weight_hh_l0", "memory_a.rnn.bias_ih_l0", "actor.0.weight"):
        assert np.isnan(got[n]).any(), n


def test_backward_of_an_overwritten_forward_is_refused():
    x = rc.make_inputs("gru1_h7_none")
    m = rc.Recurrent(x).to(DEV)
    tp = train.FusedTrainPassRecurrent(m)
    b = batch(x)
    mu1, _, _ = tp(*b, n_envs=x["E"])
    mu2, _, v2 = tp(*b)                                                # without n_envs: the one read-back of mask.sum()
    assert mu2.shape == mu1.shape
    with pytest.raises(RuntimeError, match=r"FusedTrainPassRecurrent: backward of forward call 1, but forward call 2 has overwritten"):
        mu1.sum().backward()
    (mu2.sum() + v2.sum()).backward()
    assert all(p.grad is not None for p in m.parameters())


# ---- the whole update -------------------------------------------------------------------------------------------------------------------------
STATE_KEYS = ("h0_a", "c0_a", "h0_c", "c0_c")


def _update_columns(fx):
    """The fixture with the pass's inputs of every step beside its stored columns: (fx + obs, critic_obs, masks and the start states per
    step, the column names)."""
    steps = [rc.fixture_inputs(fx, s) for s in range(fx["cfg"]["steps"])]
    keys = ("obs", "critic_obs", "masks") + tuple(k for k in STATE_KEYS if steps[0][k] is not None)
    return dict(fx, **{k: [x[k] for x in steps] for k in keys}), rc.FIXTURE_COLUMNS + keys


def _hidden(c, lstm):
    """(hid_a, hid_c) as the generator yields them, from a step's columns; an LSTM's critic is handed the actor's start states."""
    hid_a = [c["h0_a"], c["c0_a"]] if lstm else c["h0_a"]
    return hid_a, (hid_a if lstm else c["h0_c"])


def _forward(m, c, lstm):
    tup = lambda h: tuple(h) if isinstance(h, list) else h
    hid_a, hid_c = _hidden(c, lstm)
    return m(c["obs"], c["critic_obs"], c["masks"] > 0.5, tup(hid_a), tup(hid_c))


def _torch_update(fx, dtype):
    """The reference's mini-batch steps on the fixture's columns in torch ops of `dtype` on the CPU (tests/train_gpu.torch_rl_update) around
    torch's own nn.LSTM / nn.GRU.  Returns (per step the parameters by name as float64 numpy, rates)."""
    fxu, columns = _update_columns(fx)
    m = rc.Recurrent(rc.fixture_inputs(fx, 0), dtype)
    snap = lambda: {n: p.detach().double().numpy().copy() for n, p in zip(fx["names"], m.parameters())}
    return tg.torch_rl_update(fxu, columns, lambda c: _forward(m, c, bool(fx["cfg"]["lstm"])), list(m.parameters()), snap, dtype)


def _torch_step(fx, s, before, dtype):
    """Step s alone from the parameters `before`, in torch ops of `dtype` on the CPU: the outputs, the loss and every gradient before the
    clip, by name."""
    fxu, columns = _update_columns(fx)
    x = rc.fixture_inputs(fx, s, before)
    m = rc.Recurrent(x, dtype)
    c = {k: torch.from_numpy(np.asarray(fxu[k][s], np.float32)).to(dtype) for k in columns}
    outs = _forward(m, c, bool(fx["cfg"]["lstm"]))
    loss, _ = tg.torch_rl_step(outs, c, fx["cfg"])
    loss.backward()
    out = dict(zip(("mu", "sigma", "values"), outs), loss=loss, **{n: p.grad for n, p in zip(x["names"], m.parameters())})
    return {k: v.detach().numpy() for k, v in out.items()}


class _Learner:
    """FusedTrainPassRecurrent + FusedPPOLoss + FusedAdam on a module: the fused recurrent PPO mini-batch step."""

    def __init__(self, m, cfg):
        self.tp, self.lstm = train.FusedTrainPassRecurrent(m), bool(cfg["lstm"])
        self.loss_fn = ppo_loss.FusedPPOLoss(clip_param=cfg["clip_param"], value_loss_coef=cfg["value_loss_coef"], entropy_coef=cfg["entropy_coef"])
        self.opt = optim.FusedAdam(m.named_parameters(), lr=cfg["lr0"], betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["eps"],
                                   max_grad_norm=cfg["max_grad_norm"], desired_kl=cfg["desired_kl"])
        self.optimizers = (self.opt,)

    def backward(self, t):
        """The step up to the gradients before the clip: (the loss head's result, (mu, sigma, values))."""
        n_envs = t["actions"].shape[0] // t["masks"].shape[0]                     # from shapes: nothing is read back
        outs = self.tp(t["obs"], t["critic_obs"], t["masks"], _hidden(t, self.lstm), n_envs=n_envs)
        out = self.loss_fn(*outs, t["actions"], t["old_log_prob"], t["advantages"], t["returns"], t["target_values"], t["old_mu"], t["old_sigma"])
        self.opt.zero_grad()
        out.loss.backward()
        return out, outs

    def step(self, t):
        out, _ = self.backward(t)
        self.opt.step(kl_mean=out.kl_mean)
        return out


def _batches(fx, steps):
    fxu, columns = _update_columns(fx)
    return [{k: (torch.from_numpy(np.ascontiguousarray(fxu[k][s])).to(DEV) if k == "masks" else dev(fxu[k][s])) for k in columns} for s in steps]


@pytest.mark.parametrize("kind", list(FIXTURES))
def test_fixture_update_end_to_end(kind):
    """The four steps of the reference's PPO.update() on ActorCriticRecurrent through FusedTrainPassRecurrent, FusedPPOLoss and FusedAdam:
    the learning rates are the fixture's; per step the outputs, the loss and the gradients before the clip lie within the parity rule of
    that step in torch float64 from the parameters the learner had (its float32 side: the same step in torch float32), and the parameters
    after every step within the rule of the float64 run of the same torch code on the float32 inputs, which is the fixture up to the
    rounding of its inputs."""
    fx = rc.load_fixture(FIXTURES[kind])
    cfg = fx["cfg"]
    ref64, lrs64 = _torch_update(fx, torch.float64)
    ref32, lrs32 = _torch_update(fx, torch.float32)
    assert lrs64 == lrs32 == [float(v) for v in fx["lr"]]
    assert max(np.abs(ref64[-1][n] - b).max() for n, b in zip(fx["names"], fx["params"][-1])) < 1e-5
    m = rc.Recurrent(rc.fixture_inputs(fx, 0)).to(DEV)
    learner = _Learner(m, cfg)
    for s, t in enumerate(_batches(fx, range(cfg["steps"]))):
        before = [host(p).astype(np.float64) for p in m.parameters()]
        out, outs = learner.backward(t)
        got = dict(zip(("mu", "sigma", "values"), (host(o) for o in outs)), loss=host(out.loss))
        got.update({n: host(p.grad).copy() for n, p in zip(rc.fixture_inputs(fx, s)["names"], m.parameters())})
        learner.opt.step(kl_mean=out.kl_mean)
        assert learner.opt.lr == float(fx["lr"][s]), (s, learner.opt.lr, fx["lr"][s])
        rc.check_parity(got, _torch_step(fx, s, before, torch.float64), _torch_step(fx, s, before, torch.float32), f"{kind} fixture step {s}", RATIOS)
        tg.check_parameters(dict(zip(fx["names"], (host(p) for p in m.parameters()))), ref64[s], ref32[s], s, RATIOS)


@pytest.mark.parametrize("kind", list(FIXTURES))
def test_captured_update_step_replays_like_eager_steps(kind):
    """One whole update step (the pass's forward, loss head, backward, optimizer) captured on one stream as a HIP graph and replayed three
    times with the mini-batch rewritten in place in between: the parameters, the rate and the step count are those of three eager steps
    bit for bit.  The three mini-batches are the fixture's first with its observations and start states scaled, and the columns of three
    steps."""
    fx = rc.load_fixture(FIXTURES[kind])
    batches = _batches(fx, (0, 2, 0))
    for i, b in enumerate(batches):
        for k in ("obs", "critic_obs") + tuple(k for k in STATE_KEYS if k in b):
            b[k] = b[k] * (1.0 - 0.25 * i)
        b["advantages"] = b["advantages"] * (1.0 + 0.5 * i)
    x = rc.fixture_inputs(fx, 0)
    tg.replays_like_eager_steps(lambda: rc.Recurrent(x).to(DEV), lambda m: _Learner(m, fx["cfg"]), batches)


# ---- the three halves together ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,critic_hidden", [("lstm2_h64_t6", "reference"), ("lstm1_h7_t6", "own"), ("gru2_h65_t2", "reference")])
def test_mini_batches_from_the_storage_filled_by_the_fused_policy(name, critic_hidden):
    """FusedPolicy.act(..., storage=st) fills a RolloutStorage over T steps with dones; every mini-batch of its recurrent generator goes
    into the pass as it is yielded: the outputs and gradients keep the parity rule against torch on the same tensors, the means equal what
    the rollout stored for the same parameters, and so do the values where the critic starts from its own states."""
    x = rc.make_inputs(name)
    T, n, nmb = 6, 12, 2
    m = rc.Recurrent(x).to(DEV)
    fp = policy.FusedPolicy(m, seed=3)
    st = rollout.RolloutStorage(n, T, [x["obs_widths"][0]], [x["obs_widths"][1]], [x["A"]], DEV, lstm_critic_hidden=critic_hidden)
    g = torch.Generator().manual_seed(11)
    dones = torch.rand(T, n, generator=g) < 0.25
    assert dones[:-1].any() and not dones[:-1].all(0).any()
    prev = None
    for t in range(T):
        o, c = torch.randn(n, x["obs_widths"][0], generator=g).to(DEV), torch.randn(n, x["obs_widths"][1], generator=g).to(DEV)
        fp.act(o, c, storage=st, reset=prev)
        prev = dones[t].to(DEV)
        st.add_step(torch.zeros(n, device=DEV), prev, None, 0.99, observations=o, critic_observations=c)
    tp = train.FusedTrainPassRecurrent(m)
    lstm = x["kind"] == "lstm"
    for i, b in enumerate(st.reccurent_mini_batch_generator(nmb, 1)):
        obs_b, cobs_b, actions_b, values_b, (hid_a, hid_c), masks = b[0], b[1], b[2], b[3], b[9], b[10]
        assert (hid_c is hid_a) == (lstm and critic_hidden == "reference")
        E = actions_b.shape[1]
        cot = {k: torch.randn((T * E, w), generator=g) for k, w in zip(tg.COTANGENTS, (x["A"], x["A"], 1))}
        for p in m.parameters():
            p.grad = None
        outs = tp(obs_b, cobs_b, masks, (hid_a, hid_c), n_envs=E)
        torch.autograd.backward(list(outs), [v.to(DEV) for v in cot.values()])
        torch.cuda.synchronize()
        got = dict(zip(("mu", "sigma", "values"), (host(o) for o in outs)))
        got.update({k: host(p.grad) for k, p in zip(x["names"], m.parameters())})
        np.testing.assert_allclose(got["mu"], host(st.mu[:, i * E:(i + 1) * E].flatten(0, 1)), atol=2e-5, rtol=0)
        if not (lstm and critic_hidden == "reference"):
            np.testing.assert_allclose(got["values"], host(values_b.flatten(0, 1)), atol=2e-5, rtol=0)
        states = lambda h: [host(t) for t in h] if isinstance(h, list) else [host(h), None]
        (ha, ca), (hc, cc) = states(hid_a), states(hid_c)
        y = dict(x, obs=host(obs_b), critic_obs=host(cobs_b), masks=host(masks), h0_a=ha, c0_a=ca, h0_c=hc, c0_c=cc, T=T, E=E, n_traj=int(masks.shape[1]),
                 max_len=int(obs_b.shape[0]), **{k: v.numpy() for k, v in cot.items()})
        rc.check_parity(got, rc.torch_reference(y, torch.float64), rc.torch_reference(y, torch.float32), f"{name} storage mini-batch {i}", RATIOS)


def test_zz_print_the_parity_ratios():
    """Not a check of its own: the worst |kernel - f64| / max(|torch-f32 - f64|, ulp) per tensor class over every parity check above, for
    DESIGN.md's table."""
    tg.print_parity_ratios(RATIOS)

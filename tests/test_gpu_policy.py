"""The fused policy step on the device (csrc/lg_policy.hip behind hcr_genesis_lr_cl_amd.policy.FusedPolicy) against the same modules
evaluated by torch on the CPU in float64: forward parity at every reference net shape and ragged batch sizes, the sampling epilogue with
injected noise and with the Philox draw, capture and replay, the modes, the storages, and a 24-step rollout.

The forward-parity rule (factor, floor and their derivation) and the numpy restatements live in tests/test_policy_host.py."""
import copy

import numpy as np
import pytest
import torch

from tests.test_policy_host import NETS, make_net, max_err, parity_bound, philox_normals, philox_uniforms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 33, 257)          # below, across and ragged against every row tile (8, 16, 32)
CLIP = 0.05
_CASES = {}


def case(name, clip=CLIP):
    """Per net set (and clip), computed once and shared: the module, seeded inputs for the largest N and the float64 / float32 CPU results."""
    if (name, clip) not in _CASES:
        m, d = make_net(name, clip), NETS[name]
        g = torch.Generator().manual_seed(11)
        n = max(SIZES)
        obs, cobs = torch.randn(n, d["obs"], generator=g), torch.randn(n, d["cobs"], generator=g)
        m64 = copy.deepcopy(m).double()
        with torch.no_grad():
            ref = dict(mu=m64.mean(obs.double()).numpy(), values=m64.critic(cobs.double()).numpy())
            f32 = dict(mu=m.mean(obs).numpy(), values=m.critic(cobs).numpy())
            if d["est"]:
                ref["labels"], f32["labels"] = m64.estimator(obs.double()).numpy(), m.estimator(obs).numpy()
        _CASES[name, clip] = dict(module=m, gpu=copy.deepcopy(m).to(DEV), obs=obs, cobs=cobs, ref=ref, f32=f32, noise=torch.randn(n, d["A"], generator=g))
    return _CASES[name, clip]


def fused(name, seed=0, clip=CLIP):
    from hcr_genesis_lr_cl_amd.policy import FusedPolicy
    return FusedPolicy(case(name, clip)["gpu"], seed=seed)


def run(name, n, clip=CLIP, **kw):
    c = case(name, clip)
    fp = fused(name, kw.pop("seed", 0), clip)
    lab = torch.full((n, NETS[name]["est"][1]), 7.5, device=DEV) if NETS[name]["est"] else None
    noise = c["noise"][:n].to(DEV) if kw.pop("inject", True) else None
    act = fp.act(c["obs"][:n].to(DEV), c["cobs"][:n].to(DEV), noise=noise, labels=lab, **kw)
    torch.cuda.synchronize()
    return fp, act, lab


# ---- forward parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(NETS))
def test_forward_parity(name, n):
    """max |kernel - f64| <= PARITY_FACTOR * max(max |torch f32 - f64|, one ulp of the largest output), for mu, values and the estimator
    output; DESIGN.md section 10 records the measured figures."""
    c = case(name)
    fp, _, lab = run(name, n)
    got = dict(mu=fp.last_mu, values=fp.last_values)
    if lab is not None:
        got["labels"] = lab
    for k, x in got.items():
        ref = c["ref"][k][:n]
        ek, et = max_err(x.cpu().numpy(), ref), max_err(c["f32"][k][:n], ref)
        print(f"parity {name} N={n} {k}: kernel {ek:.3e} torch-f32 {et:.3e} bound {parity_bound(et, ref):.3e} max|ref| {np.abs(ref).max():.3e}")
        assert ek <= parity_bound(et, ref), (k, ek, et)
    mu = fp.last_mu.cpu().numpy()
    if n > 1:
        assert np.abs(mu).max() == np.float32(CLIP) and np.abs(mu).min() < CLIP          # both Hardtanh branches ran


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(NETS))
def test_forward_parity_of_the_unclipped_mean(name, n):
    """The same nets without the Hardtanh: with the small clip most means saturate (at N = 1 possibly all of them, which would leave the
    mu comparison above empty), so here every actor output carries the whole chain's error."""
    c = case(name, None)
    fp, _, _ = run(name, n, clip=None)
    ref = c["ref"]["mu"][:n]
    ek, et = max_err(fp.last_mu.cpu().numpy(), ref), max_err(c["f32"]["mu"][:n], ref)
    print(f"parity unclipped {name} N={n} mu: kernel {ek:.3e} torch-f32 {et:.3e} bound {parity_bound(et, ref):.3e} max|ref| {np.abs(ref).max():.3e}")
    assert np.abs(ref).max() > 2 * CLIP                                      # outputs the small clip would have cut
    assert ek <= parity_bound(et, ref), (ek, et)


# ---- the epilogue with injected noise ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "go2", "tron1_pf_ee"])
def test_epilogue_follows_the_written_formula(name):
    """Given the kernel's own mu: sigma is std bit for bit; actions = mu + sigma * z within one rounding of each operand; the log-prob is
    sum_a -(action - mu)^2 / (2 sigma^2) - log sigma - log sqrt(2 pi) with d = action - mu taken from the float32 action."""
    n = 33
    c = case(name)
    fp, act, _ = run(name, n)
    u = 2.0 ** -24
    mu, sg = fp.last_mu.cpu().numpy().astype(np.float64), fp.last_sigma.cpu().numpy()
    std = c["module"].std.detach().numpy()
    assert np.array_equal(sg, np.broadcast_to(std, sg.shape))
    z = c["noise"][:n].numpy().astype(np.float64)
    sg = sg.astype(np.float64)
    a64 = mu + sg * z
    a = act.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(a - a64) <= 2 * u * (np.abs(mu) + np.abs(sg * z)))              # one rounding of the product, one of the sum
    # d carries the action's rounding (<= u |action|); each of the ~6 float32 operations of a term adds <= u of its magnitude; the
    # A-term running sum adds <= A u sum |term|
    d = a64 - mu
    mag = d * d / (2 * sg * sg) + np.abs(np.log(sg)) + 0.9189385332046727
    lp64 = (-(d * d) / (2 * sg * sg) - np.log(sg) - 0.9189385332046727).sum(-1)
    A = mu.shape[1]
    bound = (np.abs(d) * 2 * u * (np.abs(a64) + np.abs(mu)) / (sg * sg) + 8 * u * mag).sum(-1) + A * u * mag.sum(-1)
    err = np.abs(fp.last_log_prob.cpu().numpy()[:, 0] - lp64)
    print(f"epilogue {name}: log-prob max err {err.max():.3e}, smallest bound {bound.min():.3e}")
    assert np.all(err <= bound)


def test_storage_row_is_the_only_thing_written():
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    n, T, name = 33, 3, "go2"
    c = case(name)
    st = RolloutStorage(n, T, [45], [45], [12], DEV)
    tensors = {k: v for k, v in vars(st).items() if torch.is_tensor(v) and v.dtype == torch.float32 and v.dim() == 3}
    for v in tensors.values():
        v.fill_(7.5)
    others = {k: v for k, v in vars(st).items() if torch.is_tensor(v) and k not in tensors}          # dones (uint8), the GAE scratch (float64) ...
    assert "dones" in others
    for v in others.values():
        v.fill_(3)
    before = {k: v.clone() for k, v in others.items()}
    st.step = 1
    fp = fused(name)
    act = fp.act(c["obs"][:n].to(DEV), c["cobs"][:n].to(DEV), storage=st, noise=c["noise"][:n].to(DEV))
    torch.cuda.synchronize()
    assert act.data_ptr() == st.actions[1].data_ptr() and st.step == 1
    written = {"actions", "mu", "sigma", "actions_log_prob", "values"}
    for k, v in tensors.items():
        for t in range(T):
            if k in written and t == 1:
                assert not (v[t] == 7.5).any(), k
            else:
                assert (v[t] == 7.5).all(), (k, t)
    for k, v in others.items():
        assert torch.equal(v, before[k]), k
    own = fused(name)
    own.act(c["obs"][:n].to(DEV), c["cobs"][:n].to(DEV), noise=c["noise"][:n].to(DEV))
    torch.cuda.synchronize()
    for k, x in (("actions", own.last_actions), ("mu", own.last_mu), ("sigma", own.last_sigma), ("actions_log_prob", own.last_log_prob),
                 ("values", own.last_values)):
        assert torch.equal(tensors[k][1], x), k


# ---- the Philox draw ------------------------------------------------------------------------------------------------------------------------
def test_philox_draw_matches_the_restatement():
    """Uniforms bit for bit (debug output); normals z = (action - mu) / sigma against the float64 Box-Muller on those uniforms.  Bound: the
    device's logf / sqrtf / sinf / cosf are within 2 ulp, so |dz| <= 3 * 2^-23 |z| + 2^-22 r <= 2e-6 for r < 5.8 -- 1e-5 is taken -- plus the
    rounding of recovering z from the stored float32 action, 2^-22 (|mu| + |action|) / sigma."""
    name, n, seed = "go2", 4096, (0xABCD << 32) | 0x1234
    c = case(name)
    g = torch.Generator().manual_seed(5)
    obs = torch.randn(n, 45, generator=g).to(DEV)
    fp = fused(name, seed)
    fp.counter.fill_(41)
    dbg = torch.zeros(n, 12, device=DEV)
    outs = []
    for _ in range(2):
        a = fp.act(obs, obs, _dbg_uniform=dbg)
        outs.append((a.cpu().numpy().astype(np.float64), fp.last_mu.cpu().numpy().astype(np.float64), fp.last_sigma.cpu().numpy().astype(np.float64),
                     dbg.cpu().numpy().copy()))
    assert int(fp.counter.item()) == 43
    for k, (a, mu, sg, u) in enumerate(outs):
        assert np.array_equal(u, philox_uniforms(seed, 41 + k, n, 12)), k
        z, want = (a - mu) / sg, philox_normals(seed, 41 + k, n, 12)
        assert np.all(np.abs(z - want) <= 1e-5 + 2.0 ** -22 * (np.abs(mu) + np.abs(a)) / sg), k
        assert abs(want.mean()) < 5 / np.sqrt(z.size) and abs(z.mean()) < 0.0226 and abs(z.var() - 1) < 0.032       # n = 49 152, 5 sigma
    assert not np.any(outs[0][3] == outs[1][3])
    fp.counter.fill_(41)                                     # the same seed and counter: the same bits
    again = fp.act(obs, obs).cpu().numpy().astype(np.float64)
    assert np.array_equal(again, outs[0][0])


def test_capture_and_replay_draw_consecutive_counters():
    name, n, seed = "go2", 33, 77
    c = case(name)
    obs, cobs = c["obs"][:n].to(DEV), c["cobs"][:n].to(DEV)
    fp = fused(name, seed)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fp.act(obs, cobs)                                   # warm-up outside the capture, as bench.py does: counter 0
    torch.cuda.current_stream().wait_stream(s)
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        act = fp.act(obs, cobs)
    torch.cuda.synchronize()
    assert int(fp.counter.item()) == 1                      # capturing enqueues nothing
    ref = c["ref"]["mu"][:n]
    for k in (1, 2):
        gph.replay()
        torch.cuda.synchronize()
        a, mu, sg = (x.cpu().numpy().astype(np.float64) for x in (act, fp.last_mu, fp.last_sigma))
        assert max_err(mu, ref) <= parity_bound(max_err(c["f32"]["mu"][:n], ref), ref)
        assert max_err(fp.last_values.cpu().numpy(), c["ref"]["values"][:n]) <= parity_bound(max_err(c["f32"]["values"][:n], c["ref"]["values"][:n]),
                                                                                            c["ref"]["values"][:n])
        want = philox_normals(seed, k, n, 12)
        assert np.all(np.abs((a - mu) / sg - want) <= 1e-5 + 2.0 ** -22 * (np.abs(mu) + np.abs(a)) / sg), k
        assert int(fp.counter.item()) == k + 1


# ---- modes and storages -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "go2_ee"])
def test_modes(name):
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    n = 33
    c = case(name)
    obs, cobs, noise = c["obs"][:n].to(DEV), c["cobs"][:n].to(DEV), c["noise"][:n].to(DEV)
    fp, act, _ = run(name, n)
    mu, values = fp.last_mu.clone(), fp.last_values.clone()
    assert torch.equal(fp.act_inference(obs), mu)
    assert torch.equal(fp.evaluate(cobs), values)
    fp.last_values.fill_(7.5)                               # a call without critic observations writes no values
    fp.act(obs, None, noise=noise)
    torch.cuda.synchronize()
    assert fp.last_values is None and (fp._buffers(n)["values"] == 7.5).all() and torch.equal(fp.last_mu, mu)
    tr = RolloutStorage.Transition()
    out = fp.fill_transition(tr, obs, cobs, noise=noise)
    torch.cuda.synchronize()
    filled = {k for k, v in vars(tr).items() if v is not None}
    assert filled == {"actions", "values", "actions_log_prob", "action_mean", "action_sigma", "observations", "critic_observations"}   # ppo.py:97-104
    assert out is tr.actions and torch.equal(tr.actions, act) and torch.equal(tr.values, values) and torch.equal(tr.action_mean, mu)
    assert tr.actions_log_prob.shape == (n,) and tr.observations is obs and tr.critic_observations is cobs


def test_stacked_explicit_estimator_storage():
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorageEE
    name, n, T = "go2_ee", 33, 2
    c = case(name)
    st = RolloutStorageEE(n, T, [870], [900], [24], [12], DEV)
    st.estimator_features[1].copy_(c["obs"][:n])
    st.privileged_observations[1].copy_(c["cobs"][:n])
    st.step = 1
    fp = fused(name)
    lab = torch.zeros(n, 24, device=DEV)
    fp.act(st.estimator_features[1], st.privileged_observations[1], storage=st, noise=c["noise"][:n].to(DEV), labels=lab)
    torch.cuda.synchronize()
    for k, x in (("mu", st.mu[1]), ("values", st.values[1]), ("labels", lab)):
        ref = c["ref"][k][:n]
        assert max_err(x.cpu().numpy(), ref) <= parity_bound(max_err(c["f32"][k][:n], ref), ref), k
    assert not st.mu[0].any() and not st.estimator_labels.any()


def _go2_env(n, T):
    from hcr_genesis_lr_cl_amd.config import GO2Cfg
    from hcr_genesis_lr_cl_amd.envs import GO2, set_seed
    cfg = GO2Cfg()
    cfg.env.num_envs = n
    cfg.hip.obs_sets = T + 1
    set_seed(1)
    env = GO2(cfg, None, DEV, True)
    env.reset()
    return env


def test_a_replaced_layer_is_seen():
    """The descriptor cache is keyed by the live module's layer objects: a layer swapped in after a call is the one the next call reads."""
    import torch.nn as nn
    from hcr_genesis_lr_cl_amd.policy import FusedPolicy
    n = 33
    c = case("tiny")
    m = copy.deepcopy(c["gpu"])
    fp = FusedPolicy(m)
    cobs = c["cobs"][:n].to(DEV)
    v0 = fp.evaluate(cobs).clone()
    torch.manual_seed(3)
    m.critic[0] = nn.Linear(6, 33).to(DEV)
    v1 = fp.evaluate(cobs).clone()
    with torch.no_grad():
        want = copy.deepcopy(m).cpu().double().critic(c["cobs"][:n].double()).numpy()
        f32 = copy.deepcopy(m).cpu().critic(c["cobs"][:n]).numpy()
    assert not torch.equal(v0, v1) and max_err(v1.cpu().numpy(), want) <= parity_bound(max_err(f32, want), want)


def test_rollout_end_to_end_zero_copy():
    """go2, 64 envs, 24 steps of act -> step -> add_step -> compute_returns with FusedPolicy on zero-copy observation rows and injected
    noise; the torch modules (CPU float32) act on the observations the env produced and on the same noise, and their actions, values and
    returns are stored in a second storage with the same rewards and dones.  Per step, the two storages' actions, values and returns
    differ by no more than the forward-parity bound of that quantity at that step: parity_bound(error of the torch-float32 side against
    float64, float64 reference), the float64 references being the double modules on the same observations and noise and the float64 GAE
    (oracle/rollout_oracle.py) on their values."""
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    from oracle import rollout_oracle as ro
    n, T, gamma, lam = 64, 24, 0.99, 0.95
    c = case("go2")
    m, m64 = c["module"], copy.deepcopy(c["module"]).double()
    std = m.std.detach()
    env = _go2_env(n, T)
    st = RolloutStorage(n, T, [45], [None], [12], DEV, env=env)
    assert st.zero_copy
    ref = RolloutStorage(n, T, [45], [None], [12], DEV)
    fp = fused("go2")
    noise = torch.randn(T, n, 12, generator=torch.Generator().manual_seed(2))
    noise_dev = noise.to(DEV)
    a64, v64, rew64 = np.zeros((T, n, 12)), np.zeros((T, n, 1)), np.zeros((T, n, 1))
    for t in range(T):
        obs = env.get_observations()
        assert obs.data_ptr() == st.observations[t].data_ptr()
        act = fp.act(obs, obs, storage=st, noise=noise_dev[t])
        o = obs.cpu()
        with torch.no_grad():
            ref.actions[t].copy_(m.actor(o) + std * noise[t])
            ref.values[t].copy_(m.critic(o))
            a64[t] = (m64.actor(o.double()) + std.double() * noise[t].double()).numpy()
            v64[t] = m64.critic(o.double()).numpy()
        out = env.step(act)
        rew64[t, :, 0] = out[-3].cpu().numpy().astype(np.float64) + float(np.float32(gamma)) * v64[t, :, 0] * out[-1]["time_outs"].cpu().numpy()
        st.add_step(out[-3], out[-2], out[-1]["time_outs"], gamma)
        ref.add_step(out[-3], out[-2], out[-1]["time_outs"], gamma)
    last = env.get_observations()
    st.compute_returns(fp.evaluate(last), gamma, lam)
    with torch.no_grad():
        ref.compute_returns(m.critic(last.cpu()).to(DEV), gamma, lam)
        last64 = m64.critic(last.cpu().double()).numpy()
    torch.cuda.synchronize()
    assert torch.equal(st.dones, ref.dones)
    r64 = ro.compute_returns_f64(v64, rew64, st.dones.cpu().numpy(), last64, gamma, lam)[0]
    worst = {}
    for k, x64 in (("actions", a64), ("values", v64), ("returns", r64)):
        got, torch32 = getattr(st, k).cpu().numpy().astype(np.float64), getattr(ref, k).cpu().numpy().astype(np.float64)
        for t in range(T):
            d, bound = float(np.abs(got[t] - torch32[t]).max()), parity_bound(max_err(torch32[t], x64[t]), x64[t])
            if k not in worst or d / bound > worst[k][0] / worst[k][1]:
                worst[k] = (d, bound, t)
    print("rollout, worst step per tensor (|fused - torch|, parity bound, step): " + ", ".join(f"{k} {d:.3e} {b:.3e} {t}" for k, (d, b, t) in worst.items()))
    for k, (d, b, t) in worst.items():
        assert d <= b, (k, t, d, b)

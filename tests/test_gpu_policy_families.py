"""The fused policy step for the teacher-student (TS), concurrent teacher-student (CTS) and DreamWaQ families on the device
(csrc/lg_policy.hip behind hcr_genesis_lr_cl_amd.policy.FusedPolicy) against the same modules evaluated by torch on the CPU in float64:
forward parity per family, the CTS row split, the VAE head with injected and with Philox noise, capture and replay, the three storages,
replaced layers, and an 8-step Go2CTS rollout.

The forward-parity rule and the Philox restatements are those of tests/test_policy_host.py; the stand-in modules, the latent-draw
restatement and the float64 discrimination checks (what a wrong encoder, a dropped clip or swapped latents would give) live in
tests/test_policy_families_host.py."""
import copy

import numpy as np
import pytest
import torch

from tests.test_policy_families_host import DWAQ_NETS, TS_NETS, latent_normals, latent_uniforms, make_dwaq, make_ts
from tests.test_policy_host import max_err, parity_bound, philox_uniforms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 33, 257)          # below, across and ragged against every row tile (8, 16, 32)
CLIP = 0.05
_CASES = {}


def _np(d):
    return {k: v.numpy() for k, v in d.items()}


def ts_case(name, clip=None):
    """Per TS net set (and clip), computed once and shared: module, seeded inputs for the largest N, float64 / float32 CPU results."""
    if (name, clip) not in _CASES:
        m, d = make_ts(name, clip), TS_NETS[name]
        g = torch.Generator().manual_seed(11)
        n = max(SIZES)
        x = {k: torch.randn(n, d[k], generator=g) for k in ("obs", "priv", "hist", "cobs")}
        m64 = copy.deepcopy(m).double()
        x64 = {k: v.double() for k, v in x.items()}
        with torch.no_grad():
            ref = _np(dict(teacher=m64.mean(x64["obs"], x64["priv"]), student=m64.mean(x64["obs"], x64["hist"], True), values=m64.critic(x64["cobs"])))
            f32 = _np(dict(teacher=m.mean(x["obs"], x["priv"]), student=m.mean(x["obs"], x["hist"], True), values=m.critic(x["cobs"])))
        _CASES[name, clip] = dict(module=m, gpu=copy.deepcopy(m).to(DEV), ref=ref, f32=f32, noise=torch.randn(n, d["A"], generator=g), **x)
    return _CASES[name, clip]


def dw_case(name, clip=None):
    if (name, clip) not in _CASES:
        m, d = make_dwaq(name, clip), DWAQ_NETS[name]
        g = torch.Generator().manual_seed(11)
        n = max(SIZES)
        x = {k: torch.randn(n, d[k], generator=g) for k in ("obs", "hist", "cobs")}
        eps = torch.randn(n, d["L"] + d["E"], generator=g)
        m64 = copy.deepcopy(m).double()
        with torch.no_grad():
            ref = _np(m64.forward_all(x["obs"].double(), x["hist"].double(), eps.double()))
            f32 = _np(m.forward_all(x["obs"], x["hist"], eps))
            det64, det32 = _np(m64.forward_all(x["obs"].double(), x["hist"].double())), _np(m.forward_all(x["obs"], x["hist"]))
            ref.update(values=m64.critic(x["cobs"].double()).numpy(), det_latent=det64["latent"], det_mu=det64["mu"])
            f32.update(values=m.critic(x["cobs"]).numpy(), det_latent=det32["latent"], det_mu=det32["mu"])
        _CASES[name, clip] = dict(module=m, gpu=copy.deepcopy(m).to(DEV), ref=ref, f32=f32, eps=eps, noise=torch.randn(n, d["A"], generator=g), **x)
    return _CASES[name, clip]


def fused(c, seed=0):
    from hcr_genesis_lr_cl_amd.policy import FusedPolicy
    return FusedPolicy(c["gpu"], seed=seed)


def dev(c, n, *keys):
    return [c[k][:n].to(DEV) for k in keys]


def in_parity(tag, got, c, key, rows=slice(None)):
    """The project's rule: max |kernel - f64| <= parity_bound(max |torch f32 - f64|, f64), printed before it is asserted."""
    ref, f32 = c["ref"][key][rows], c["f32"][key][rows]
    if ref.shape[0] == 0:
        return
    ek, et = max_err(got.cpu().numpy(), ref), max_err(f32, ref)
    print(f"parity {tag} {key}: kernel {ek:.3e} torch-f32 {et:.3e} ratio {ek / max(et, 1e-30):.2f} bound {parity_bound(et, ref):.3e} max|ref| {np.abs(ref).max():.3e}")
    assert ek <= parity_bound(et, ref), (tag, key, ek, et)


# ---- forward parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["tiny_ts", "go2_ts"])
def test_ts_forward_parity(name, n):
    """The teacher through `act` (as PPO_TS.act), the deterministic means of `act_teacher` / `act_student`, and the values."""
    c = ts_case(name)
    fp = fused(c)
    obs, priv, hist, cobs, noise = dev(c, n, "obs", "priv", "hist", "cobs", "noise")
    fp.act(obs, cobs, privileged_obs=priv, noise=noise)
    torch.cuda.synchronize()
    tag = f"{name} N={n}"
    in_parity(tag, fp.last_mu, c, "teacher", slice(0, n))
    in_parity(tag, fp.last_values, c, "values", slice(0, n))
    mu = fp.last_mu.clone()
    assert torch.equal(fp.act_teacher(obs, priv), mu)
    in_parity(tag, fp.act_student(obs, hist), c, "student", slice(0, n))
    assert torch.equal(fp.evaluate(cobs), fp.last_values)
    assert fp.row_tile() == {"tiny_ts": 32, "go2_ts": 16}[name]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(DWAQ_NETS))
def test_dreamwaq_forward_parity(name, n):
    """Injected latent and action noise: the distribution parameters (clipped log-variances), the samples (z, vel), mu and the values.
    The sampled latent carries the log-variance error e_lv through exp: |eps| * std * e_lv / 2 -- on the torch-float32 side as well, so the
    rule needs no other factor for it (DESIGN.md section 10 has the measured figures)."""
    c, d = dw_case(name), DWAQ_NETS[name]
    L, E = d["L"], d["E"]
    fp = fused(c)
    obs, hist, cobs, noise, eps = dev(c, n, "obs", "hist", "cobs", "noise", "eps")
    lat, par = torch.full((n, L + E + 3), 7.5, device=DEV), torch.full((n, 2 * (L + E)), 7.5, device=DEV)
    fp.act(obs, cobs, obs_history=hist, noise=noise, latent_noise=eps, latent=lat[:, :L + E], latent_params=par)
    torch.cuda.synchronize()
    tag = f"{name} N={n}"
    in_parity(tag, par, c, "params", slice(0, n))
    in_parity(tag, lat[:, :L + E], c, "latent", slice(0, n))
    in_parity(tag, fp.last_mu, c, "mu", slice(0, n))
    in_parity(tag, fp.last_values, c, "values", slice(0, n))
    assert (lat[:, L + E:] == 7.5).all()                                             # the row stride is respected
    p = par.cpu().numpy()
    lv = np.concatenate((p[:, L:2 * L], p[:, 2 * L + E:]), axis=1)
    assert np.abs(lv).max() <= 5.0
    if n > 1:
        assert (lv == 5.0).any() and (lv == -5.0).any() and (np.abs(lv) < 5.0).any()   # both clip branches and the open one ran


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(DWAQ_NETS))
def test_dreamwaq_deterministic(name, n):
    """act_inference: no draw; `latent` receives (latent_mu, vel_mu) -- bit for bit the means the sampling call reports -- and mu is the
    actor on [obs | latent_mu | vel_mu]."""
    c, d = dw_case(name), DWAQ_NETS[name]
    L, E = d["L"], d["E"]
    fp = fused(c)
    obs, hist, cobs, noise, eps = dev(c, n, "obs", "hist", "cobs", "noise", "eps")
    par, lat = torch.zeros(n, 2 * (L + E), device=DEV), torch.zeros(n, L + E, device=DEV)
    fp.act(obs, cobs, obs_history=hist, noise=noise, latent_noise=eps, latent_params=par)
    counter = int(fp.counter.item())
    mu = fp.act_inference(obs, hist, latent=lat)
    torch.cuda.synchronize()
    assert torch.equal(lat, torch.cat((par[:, :L], par[:, 2 * L:2 * L + E]), dim=1))
    in_parity(f"{name} N={n}", lat, c, "det_latent", slice(0, n))
    in_parity(f"{name} N={n}", mu, c, "det_mu", slice(0, n))
    assert int(fp.counter.item()) == counter == 0                                    # injected noise and inference draw nothing


# ---- the CTS split ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n,k", [("tiny_ts", 33, k) for k in (0, 1, 17, 32, 33)] + [("go2_cts", 257, k) for k in (100, 192)])
def test_cts_split(name, n, k):
    """Rows [0, k) in parity with the privilege encoder's float64 mean, rows [k, N) with the history encoder's; NaN in the rows a group
    must not read changes no bit of any output; the action uniforms do not depend on k."""
    c, d = ts_case(name), TS_NETS[name]
    fp = fused(c, seed=5)
    obs, priv, hist, cobs, noise = dev(c, n, "obs", "priv", "hist", "cobs", "noise")
    fp.act(obs, cobs, privileged_obs=priv, obs_history=hist, num_teacher=k, noise=noise)
    torch.cuda.synchronize()
    tag = f"{name} N={n} k={k}"
    in_parity(tag, fp.last_mu[:k], c, "teacher", slice(0, k))
    in_parity(tag, fp.last_mu[k:], c, "student", slice(k, n))
    in_parity(tag, fp.last_values, c, "values", slice(0, n))
    outs = [x.clone() for x in (fp.last_actions, fp.last_mu, fp.last_sigma, fp.last_log_prob, fp.last_values)]
    priv_nan, hist_nan = priv.clone(), hist.clone()
    priv_nan[k:], hist_nan[:k] = float("nan"), float("nan")
    fp.act(obs, cobs, privileged_obs=priv_nan, obs_history=hist_nan, num_teacher=k, noise=noise)
    torch.cuda.synchronize()
    for a, b in zip(outs, (fp.last_actions, fp.last_mu, fp.last_sigma, fp.last_log_prob, fp.last_values)):
        assert torch.isfinite(b).all() and torch.equal(a, b)
    A = d["A"]
    dbg = torch.zeros(n, 4 * ((A + 3) // 4), device=DEV)
    fp.counter.fill_(9)
    fp.act(obs, cobs, privileged_obs=priv, obs_history=hist, num_teacher=k, _dbg_uniform=dbg)
    torch.cuda.synchronize()
    assert np.array_equal(dbg.cpu().numpy(), philox_uniforms(5, 9, n, A))            # the global env index, whatever k
    assert int(fp.counter.item()) == 10 and torch.equal(fp.last_mu, outs[1])


# ---- the epilogue with injected noise ---------------------------------------------------------------------------------------------------
def _epilogue(fp, act, std, z):
    """The checks and the bound of tests/test_gpu_policy.py::test_epilogue_follows_the_written_formula, on the kernel's own mu."""
    u = 2.0 ** -24
    mu, sg = fp.last_mu.cpu().numpy().astype(np.float64), fp.last_sigma.cpu().numpy()
    assert np.array_equal(sg, np.broadcast_to(std, sg.shape))
    sg = sg.astype(np.float64)
    a64 = mu + sg * z
    a = act.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(a - a64) <= 2 * u * (np.abs(mu) + np.abs(sg * z)))
    d = a64 - mu
    mag = d * d / (2 * sg * sg) + np.abs(np.log(sg)) + 0.9189385332046727
    lp64 = (-(d * d) / (2 * sg * sg) - np.log(sg) - 0.9189385332046727).sum(-1)
    A = mu.shape[1]
    bound = (np.abs(d) * 2 * u * (np.abs(a64) + np.abs(mu)) / (sg * sg) + 8 * u * mag).sum(-1) + A * u * mag.sum(-1)
    err = np.abs(fp.last_log_prob.cpu().numpy()[:, 0] - lp64)
    print(f"epilogue: log-prob max err {err.max():.3e}, smallest bound {bound.min():.3e}")
    assert np.all(err <= bound)
    return mu


@pytest.mark.parametrize("name", ["tiny_ts", "tiny_dwaq"])
def test_epilogue_follows_the_written_formula(name):
    n = 33
    if name == "tiny_ts":
        c = ts_case(name, CLIP)
        fp = fused(c)
        obs, priv, hist, cobs, noise = dev(c, n, "obs", "priv", "hist", "cobs", "noise")
        act = fp.act(obs, cobs, privileged_obs=priv, obs_history=hist, num_teacher=17, noise=noise)
    else:
        c = dw_case(name, CLIP)
        fp = fused(c)
        obs, hist, cobs, noise, eps = dev(c, n, "obs", "hist", "cobs", "noise", "eps")
        act = fp.act(obs, cobs, obs_history=hist, noise=noise, latent_noise=eps)
    torch.cuda.synchronize()
    mu = _epilogue(fp, act, c["module"].std.detach().numpy(), c["noise"][:n].numpy().astype(np.float64))
    assert np.abs(mu).max() == np.float32(CLIP) and np.abs(mu).min() < CLIP             # both Hardtanh branches of the actor ran


# ---- the Philox draws -----------------------------------------------------------------------------------------------------------------------
def _check_latent(lat, par, L, E, want):
    """z = (sample - mu) / std against the float64 Box-Muller: the bound of tests/test_gpu_policy.py's action draw (1e-5 on z) plus the
    rounding of recovering z from the stored float32 sample and of the device's expf (2 ulp of std)."""
    lat, par = lat.cpu().numpy().astype(np.float64), par.cpu().numpy().astype(np.float64)
    mu = np.concatenate((par[:, :L], par[:, 2 * L:2 * L + E]), axis=1)
    std = np.exp(0.5 * np.concatenate((par[:, L:2 * L], par[:, 2 * L + E:]), axis=1))
    z = (lat - mu) / std
    assert np.all(np.abs(z - want) <= 1e-5 + 2.0 ** -22 * (np.abs(mu) + np.abs(lat)) / std + 2.0 ** -21 * np.abs(want))


def test_philox_draws_match_the_restatements():
    name, n, seed = "go2_dreamwaq", 257, (0xABCD << 32) | 0x1234
    c, d = dw_case(name), DWAQ_NETS[name]
    L, E, A = d["L"], d["E"], d["A"]
    W = L + E
    fp = fused(c, seed)
    fp.counter.fill_(41)
    obs, hist, cobs = dev(c, n, "obs", "hist", "cobs")
    dbg, dbl = torch.zeros(n, 4 * ((A + 3) // 4), device=DEV), torch.zeros(n, 4 * ((W + 3) // 4), device=DEV)
    lat, par = torch.zeros(n, W, device=DEV), torch.zeros(n, 2 * W, device=DEV)
    for k in (41, 42):
        fp.act(obs, cobs, obs_history=hist, latent=lat, latent_params=par, _dbg_uniform=dbg, _dbg_latent_uniform=dbl)
        torch.cuda.synchronize()
        assert np.array_equal(dbg.cpu().numpy(), philox_uniforms(seed, k, n, A)), k
        assert np.array_equal(dbl.cpu().numpy(), latent_uniforms(seed, k, n, W)), k
        _check_latent(lat, par, L, E, latent_normals(seed, k, n, W))
    assert int(fp.counter.item()) == 43                                              # once per call, though two draws read it
    in_parity(f"{name} N={n}", par, c, "params", slice(0, n))


def test_capture_and_replay_draw_consecutive_counters():
    name, n, seed = "tiny_dwaq", 33, 77
    c, d = dw_case(name), DWAQ_NETS[name]
    L, E, A = d["L"], d["E"], d["A"]
    W = L + E
    fp = fused(c, seed)
    obs, hist, cobs = dev(c, n, "obs", "hist", "cobs")
    dbg, dbl = torch.zeros(n, 4 * ((A + 3) // 4), device=DEV), torch.zeros(n, 4 * ((W + 3) // 4), device=DEV)
    lat, par = torch.zeros(n, W, device=DEV), torch.zeros(n, 2 * W, device=DEV)
    call = lambda: fp.act(obs, cobs, obs_history=hist, latent=lat, latent_params=par, _dbg_uniform=dbg, _dbg_latent_uniform=dbl)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                              # warm-up outside the capture: counter 0
    torch.cuda.current_stream().wait_stream(s)
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        call()
    torch.cuda.synchronize()
    assert int(fp.counter.item()) == 1                      # capturing enqueues nothing
    for k in (1, 2, 3):
        gph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(dbg.cpu().numpy(), philox_uniforms(seed, k, n, A)), k
        assert np.array_equal(dbl.cpu().numpy(), latent_uniforms(seed, k, n, W)), k
        _check_latent(lat, par, L, E, latent_normals(seed, k, n, W))
        assert int(fp.counter.item()) == k + 1


# ---- storages -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ts", "cts", "dreamwaq"])
def test_storage_row_is_the_only_thing_written(kind):
    from hcr_genesis_lr_cl_amd import rollout
    n, T = 33, 2
    if kind == "dreamwaq":
        c, d = dw_case("tiny_dwaq"), DWAQ_NETS["tiny_dwaq"]
        st = rollout.RolloutStorageDreamWaQ(n, T, [d["obs"]], [d["cobs"]], [d["hist"]], [d["E"]], [d["obs"]], [d["A"]], DEV)
        obs, hist, cobs, noise, eps = dev(c, n, "obs", "hist", "cobs", "noise", "eps")
        kw, mu_key = dict(obs_history=hist, latent_noise=eps), "mu"
    else:
        c, d = ts_case("tiny_ts"), TS_NETS["tiny_ts"]
        shapes = ([d["obs"]], [d["priv"]], [d["hist"]], [d["cobs"]], [d["A"]], DEV)
        st = rollout.RolloutStorageTS(n, T, *shapes) if kind == "ts" else rollout.RolloutStorageCTS(n, 17, T, *shapes)
        obs, priv, hist, cobs, noise = dev(c, n, "obs", "priv", "hist", "cobs", "noise")
        kw, mu_key = dict(privileged_obs=priv, obs_history=hist), "teacher"      # num_teacher: the CTS storage's
    tensors = {k: v for k, v in vars(st).items() if torch.is_tensor(v) and v.dtype == torch.float32 and v.dim() == 3}
    for v in tensors.values():
        v.fill_(7.5)
    others = {k: v for k, v in vars(st).items() if torch.is_tensor(v) and k not in tensors}
    assert "dones" in others and "observation_histories" in tensors
    for v in others.values():
        v.fill_(3)
    before = {k: v.clone() for k, v in others.items()}
    st.step = 1
    fp = fused(c)
    act = fp.act(obs, cobs, storage=st, noise=noise, **kw)
    torch.cuda.synchronize()
    assert act.data_ptr() == st.actions[1].data_ptr() and st.step == 1
    written = {"actions", "mu", "sigma", "actions_log_prob", "values"}
    for k, v in tensors.items():
        for t in range(T):
            assert ((v[t] == 7.5).all() if not (k in written and t == 1) else not (v[t] == 7.5).any()), (k, t)
    for k, v in others.items():
        assert torch.equal(v, before[k]), k
    tag = f"storage {kind}"
    if kind == "cts":
        in_parity(tag, st.mu[1][:17], c, "teacher", slice(0, 17))
        in_parity(tag, st.mu[1][17:], c, "student", slice(17, n))
    else:
        in_parity(tag, st.mu[1], c, mu_key, slice(0, n))
    in_parity(tag, st.values[1], c, "values", slice(0, n))
    own = fused(c)                                                                     # actions, sigma, log-prob: the same bits as without a storage
    own.act(obs, cobs, noise=noise, num_teacher=17 if kind == "cts" else None, **kw)
    torch.cuda.synchronize()
    for k, x in (("actions", own.last_actions), ("mu", own.last_mu), ("sigma", own.last_sigma), ("actions_log_prob", own.last_log_prob),
                 ("values", own.last_values)):
        assert torch.equal(tensors[k][1], x), k
    _epilogue(own, own.last_actions, c["module"].std.detach().numpy(), c["noise"][:n].numpy().astype(np.float64))


def test_fill_transition_by_family():
    from hcr_genesis_lr_cl_amd import rollout
    n = 33
    c = ts_case("tiny_ts")
    obs, priv, hist, cobs, noise = dev(c, n, "obs", "priv", "hist", "cobs", "noise")
    tr = rollout.RolloutStorageTS.Transition()
    fp = fused(c)
    out = fp.fill_transition(tr, obs, cobs, noise=noise, privileged_obs=priv, obs_history=hist)
    torch.cuda.synchronize()
    assert {k for k, v in vars(tr).items() if v is not None} == {"actions", "values", "actions_log_prob", "action_mean", "action_sigma", "observations",
                                                                 "privileged_observations", "observation_histories", "critic_observations"}     # ppo_ts.py:81-92
    assert out is tr.actions and tr.privileged_observations is priv and tr.observation_histories is hist and tr.actions_log_prob.shape == (n,)
    in_parity("fill_transition ts", tr.action_mean, c, "teacher", slice(0, n))
    c = dw_case("tiny_dwaq")
    obs, hist, cobs, noise, eps = dev(c, n, "obs", "hist", "cobs", "noise", "eps")
    tr = rollout.RolloutStorageDreamWaQ.Transition()
    lab = torch.zeros(n, 2, device=DEV)
    fused(c).fill_transition(tr, obs, cobs, noise=noise, obs_history=hist, latent_noise=eps, explicit_info_labels=lab)
    torch.cuda.synchronize()
    assert {k for k, v in vars(tr).items() if v is not None} == {"actions", "values", "actions_log_prob", "action_mean", "action_sigma", "observations",
                                                                 "privileged_observations", "observation_histories", "explicit_info_labels"}    # ppo_dreamwaq.py:127-137
    assert tr.privileged_observations is cobs and tr.explicit_info_labels is lab
    in_parity("fill_transition dreamwaq", tr.action_mean, c, "mu", slice(0, n))


# ---- replaced layers ------------------------------------------------------------------------------------------------------------------------
def test_a_replaced_encoder_or_head_layer_is_seen():
    import torch.nn as nn
    from hcr_genesis_lr_cl_amd.policy import FusedPolicy
    n = 33
    c, d = ts_case("tiny_ts"), TS_NETS["tiny_ts"]
    m = copy.deepcopy(c["gpu"])
    fp = FusedPolicy(m)
    obs, priv = dev(c, n, "obs", "priv")
    v0 = fp.act_teacher(obs, priv).clone()
    torch.manual_seed(3)
    m.privilege_encoder[0] = nn.Linear(d["priv"], d["penc"][0]).to(DEV)
    v1 = fp.act_teacher(obs, priv).clone()
    cpu = copy.deepcopy(m).cpu()
    with torch.no_grad():
        want = copy.deepcopy(cpu).double().mean(c["obs"][:n].double(), c["priv"][:n].double()).numpy()
        f32 = cpu.mean(c["obs"][:n], c["priv"][:n]).numpy()
    assert not torch.equal(v0, v1) and max_err(v1.cpu().numpy(), want) <= parity_bound(max_err(f32, want), want)
    c, d = dw_case("tiny_dwaq"), DWAQ_NETS["tiny_dwaq"]
    m = copy.deepcopy(c["gpu"])
    fp = FusedPolicy(m)
    obs, hist = dev(c, n, "obs", "hist")
    v0 = fp.act_inference(obs, hist).clone()
    m.vae.vel_mu = nn.Linear(d["H"], d["E"]).to(DEV)
    v1 = fp.act_inference(obs, hist).clone()
    cpu = copy.deepcopy(m).cpu()
    with torch.no_grad():
        want = copy.deepcopy(cpu).double().forward_all(c["obs"][:n].double(), c["hist"][:n].double())["mu"].numpy()
        f32 = cpu.forward_all(c["obs"][:n], c["hist"][:n])["mu"].numpy()
    assert not torch.equal(v0, v1) and max_err(v1.cpu().numpy(), want) <= parity_bound(max_err(f32, want), want)


# ---- one rollout ----------------------------------------------------------------------------------------------------------------------------
def test_cts_rollout_end_to_end():
    """Go2CTS, 64 envs with 48 teachers, 8 steps of act -> step -> add_step -> compute_returns with FusedPolicy and injected noise, built as
    tests/test_gpu_policy.py::test_rollout_end_to_end_zero_copy: the torch modules (CPU float32, the reference's two-pass data flow) act on
    the observations the env produced and on the same noise; per step the two storages' actions, values and returns differ by no more
    than the parity bound of that quantity at that step.  The TS storages hold no zero-copy rows, so the four observation rows are copied
    by `add_step`."""
    from hcr_genesis_lr_cl_amd.config import GO2CTSCfg
    from hcr_genesis_lr_cl_amd.envs import Go2CTS, set_seed
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorageCTS
    from oracle import rollout_oracle as ro
    n, k, T, gamma, lam = 64, 48, 8, 0.99, 0.95
    c = ts_case("go2_cts")
    m, m64 = c["module"], copy.deepcopy(c["module"]).double()
    std = m.std.detach()
    cfg = GO2CTSCfg()
    cfg.env.num_envs, cfg.env.num_teacher = n, k
    set_seed(1)
    env = Go2CTS(cfg, None, DEV, True)
    env.reset()
    shapes = ([45], [99], [900], [885], [12], DEV)
    st, ref = RolloutStorageCTS(n, k, T, *shapes), RolloutStorageCTS(n, k, T, *shapes)
    fp = fused(c)
    noise = torch.randn(T, n, 12, generator=torch.Generator().manual_seed(2))
    noise_dev = noise.to(DEV)
    a64, v64, rew64 = np.zeros((T, n, 12)), np.zeros((T, n, 1)), np.zeros((T, n, 1))
    for t in range(T):
        obs, priv, hist, cobs = (x.clone() for x in env.get_observations())
        assert (obs.shape[1], priv.shape[1], hist.shape[1], cobs.shape[1]) == (45, 99, 900, 885)
        act = fp.act(obs, cobs, storage=st, privileged_obs=priv, obs_history=hist, noise=noise_dev[t])
        o, p, h, co = obs.cpu(), priv.cpu(), hist.cpu(), cobs.cpu()
        with torch.no_grad():
            ref.actions[t].copy_(m.mean_split(o, p, h, k) + std * noise[t])
            ref.values[t].copy_(m.critic(co))
            a64[t] = (m64.mean_split(o.double(), p.double(), h.double(), k) + std.double() * noise[t].double()).numpy()
            v64[t] = m64.critic(co.double()).numpy()
        out = env.step(act)
        rew64[t, :, 0] = out[-3].cpu().numpy().astype(np.float64) + float(np.float32(gamma)) * v64[t, :, 0] * out[-1]["time_outs"].cpu().numpy()
        rows = dict(observations=obs, privileged_observations=priv, observation_histories=hist, critic_observations=cobs)
        st.add_step(out[-3], out[-2], out[-1]["time_outs"], gamma, **rows)
        ref.add_step(out[-3], out[-2], out[-1]["time_outs"], gamma, **rows)
    last = env.get_observations()[3]
    st.compute_returns(fp.evaluate(last), gamma, lam)
    with torch.no_grad():
        ref.compute_returns(m.critic(last.cpu()).to(DEV), gamma, lam)
        last64 = m64.critic(last.cpu().double()).numpy()
    torch.cuda.synchronize()
    assert torch.equal(st.dones, ref.dones) and torch.equal(st.observation_histories, ref.observation_histories)
    r64 = ro.compute_returns_f64(v64, rew64, st.dones.cpu().numpy(), last64, gamma, lam)[0]
    worst = {}
    for key, x64 in (("actions", a64), ("values", v64), ("returns", r64)):
        got, torch32 = getattr(st, key).cpu().numpy().astype(np.float64), getattr(ref, key).cpu().numpy().astype(np.float64)
        for t in range(T):
            dlt, bound = float(np.abs(got[t] - torch32[t]).max()), parity_bound(max_err(torch32[t], x64[t]), x64[t])
            if key not in worst or dlt / bound > worst[key][0] / worst[key][1]:
                worst[key] = (dlt, bound, t)
    print("rollout, worst step per tensor (|fused - torch|, parity bound, step): " + ", ".join(f"{q} {a:.3e} {b:.3e} {t}" for q, (a, b, t) in worst.items()))
    for key, (dlt, b, t) in worst.items():
        assert dlt <= b, (key, t, dlt, b)

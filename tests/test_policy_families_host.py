"""Host side of the fused policy step for the teacher-student (TS), concurrent teacher-student (CTS) and DreamWaQ families
(hcr_genesis_lr_cl_amd/policy.py, include/lgpolicy.h): the descriptors `FusedPolicy` builds for duck-typed stand-ins and for the reference's
own modules, every refusal (Python's before the library is touched, the entry point's before a launch), the numpy restatement of the
latent draw, and the float64 discrimination checks that make the comparisons of tests/test_gpu_policy_families.py able to fail.  No GPU
needed: nothing is launched.  The parity rule and the Philox restatements are those of tests/test_policy_host.py."""
import copy
import ctypes as C
import importlib.util
import os
import re
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from hcr_genesis_lr_cl_amd import abi, policy
from oracle import philox
from tests.test_policy_host import HEADER, PARITY_FACTOR, max_err, mlp, parity_bound, philox_normals, philox_uniforms

_GO2 = dict(obs=45, A=12, cobs=885, actor=[512, 256, 128], critic=[1024, 256, 128])
# TS / CTS: (obs, privileged, history, latent, privilege-encoder hidden, history-encoder hidden); `teachers`: the CTS split at 4096 envs
TS_NETS = {
    "tiny_ts": dict(obs=5, priv=7, hist=11, latent=3, penc=[9, 6], henc=[10], actor=[33, 7], A=3, cobs=6, critic=[33, 7]),   # depths differ on purpose
    "go2_ts": dict(_GO2, priv=99, hist=900, latent=99, penc=[256, 128], henc=[256, 128]),
    "go2_cts": dict(_GO2, priv=99, hist=900, latent=99, penc=[256, 128], henc=[256, 128], teachers=3072),
}
# DreamWaQ: history -> enc hidden -> H (with the trailing ELU) -> four heads (L, L, E, E); the actor reads obs + L + E
DWAQ_NETS = {
    "tiny_dwaq": dict(obs=5, hist=11, enc=[9], H=10, L=3, E=2, actor=[33, 7], A=3, cobs=6, critic=[33, 7], logvar_clip=5.0),
    "go2_dreamwaq": dict(_GO2, hist=900, enc=[256, 128], H=80, L=16, E=24, logvar_clip=5.0),
}
ROW_TILE = {"tiny_ts": 32, "tiny_dwaq": 32, "go2_ts": 16, "go2_cts": 16, "go2_dreamwaq": 16}
VAR_SCALE = 6.0          # on the two log-variance heads: pre-clip values of both signs beyond the clip and inside it


class StandInTS(nn.Module):
    """ActorCriticTS / ActorCriticCTS by duck typing: .privilege_encoder, .history_encoder, .actor, .critic, .std."""
    is_recurrent = False

    def __init__(self, d, clip):
        super().__init__()
        self.privilege_encoder = mlp(d["priv"], d["penc"], d["latent"])
        self.history_encoder = mlp(d["hist"], d["henc"], d["latent"])
        self.actor = mlp(d["obs"] + d["latent"], d["actor"], d["A"], nn.Hardtanh(-clip, clip) if clip is not None else None)
        self.critic = mlp(d["cobs"], d["critic"], 1)
        self.std = nn.Parameter(torch.ones(d["A"]))

    def mean(self, obs, x, student=False):
        return self.actor(torch.cat((obs, (self.history_encoder if student else self.privilege_encoder)(x)), dim=-1))

    def mean_split(self, obs, priv, hist, k):
        """ppo_cts.py:115-127: rows [0, k) with the privilege encoder, the rest with the history encoder."""
        return torch.cat((self.mean(obs[:k], priv[:k]), self.mean(obs[k:], hist[k:], True)), dim=0)


class StandInVAE(nn.Module):
    def __init__(self, d):
        super().__init__()
        W = d["L"] + d["E"]
        self.encoder = nn.Sequential(*mlp(d["hist"], d["enc"], d["H"]), nn.ELU())
        self.latent_mu, self.vel_mu = nn.Linear(d["H"], d["L"]), nn.Linear(d["H"], d["E"])
        c = d["logvar_clip"]
        self.latent_var = nn.Sequential(nn.Linear(d["H"], d["L"]), nn.Hardtanh(-c, c))
        self.vel_var = nn.Sequential(nn.Linear(d["H"], d["E"]), nn.Hardtanh(-c, c))
        self.decoder = mlp(W, [7], 4)                    # the learner's: FusedPolicy ignores it


class StandInDWAQ(nn.Module):
    """ActorCriticDreamWaQ by duck typing: .vae (encoder, four heads), .actor, .critic, .std."""
    is_recurrent = False

    def __init__(self, d, clip):
        super().__init__()
        self.vae = StandInVAE(d)
        self.actor = mlp(d["obs"] + d["L"] + d["E"], d["actor"], d["A"], nn.Hardtanh(-clip, clip) if clip is not None else None)
        self.critic = mlp(d["cobs"], d["critic"], 1)
        self.std = nn.Parameter(torch.ones(d["A"]))

    def forward_all(self, obs, hist, eps=None, drop_clip=False, swap=False):
        """vae.py:65-101 and actor_critic_dreamwaq.py:145-171 with eps ((N, L + E), columns (z, vel)) in place of randn; eps None: the
        means (act_inference).  `drop_clip` / `swap` are the two deliberately wrong variants of the discrimination test."""
        v = self.vae
        h = v.encoder(hist)
        lm, vm = v.latent_mu(h), v.vel_mu(h)
        lv, vv = (v.latent_var[0](h), v.vel_var[0](h)) if drop_clip else (v.latent_var(h), v.vel_var(h))
        L = lm.shape[1]
        if eps is None:
            z, vel = lm, vm
        else:
            z, vel = eps[:, :L] * torch.exp(0.5 * lv) + lm, eps[:, L:] * torch.exp(0.5 * vv) + vm
        latent = torch.cat((vel, z) if swap else (z, vel), dim=-1)
        return dict(params=torch.cat((lm, lv, vm, vv), dim=-1), latent=latent, mu=self.actor(torch.cat((obs, latent), dim=-1)))


def _seed(m, A, seed):
    """tests/test_policy_host.py::make_net's weights: uniform +-1.5 / sqrt(in), biases +-0.5, std in [0.5, 1.5)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.Linear):
                mod.weight.copy_((torch.rand(mod.weight.shape, generator=g) * 2 - 1) * 1.5 / mod.in_features ** 0.5)
                mod.bias.copy_(torch.rand(mod.bias.shape, generator=g) - 0.5)
        m.std.copy_(0.5 + torch.rand(A, generator=g))
    return m


def make_ts(name, clip=0.05, seed=3):
    return _seed(StandInTS(TS_NETS[name], clip), TS_NETS[name]["A"], seed)


def make_dwaq(name, clip=0.05, seed=3):
    m = _seed(StandInDWAQ(DWAQ_NETS[name], clip), DWAQ_NETS[name]["A"], seed)
    with torch.no_grad():
        for head in (m.vae.latent_var[0], m.vae.vel_var[0]):
            head.weight.mul_(VAR_SCALE)
            head.bias.mul_(VAR_SCALE)
            head.weight[1::2].neg_()                     # every other output mirrored: with few outputs one sign could be missing
            head.bias[1::2].neg_()
    return m


def latent_uniforms(seed, counter, n_envs, width):
    """(N, 4 * ceil(width / 4)) float32: counter (env, quad over the L + E columns, call counter, LG_POLICY_LATENT_TAG), key = seed."""
    q = (width + 3) // 4
    env, quad = np.meshgrid(np.arange(n_envs, dtype=np.uint64), np.arange(q, dtype=np.uint64), indexing="ij")
    w = philox.philox4x32_10(env, quad, counter, abi.POLICY_LATENT_TAG, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.stack([philox.u01(x) for x in w], axis=-1).reshape(n_envs, 4 * q)


def latent_normals(seed, counter, n_envs, width):
    """(N, width) float64: Box-Muller exactly as tests/test_policy_host.py::philox_normals forms it, on the latent stream's uniforms."""
    u = latent_uniforms(seed, counter, n_envs, width).reshape(n_envs, -1, 2)
    rad = np.sqrt(-2.0 * np.log(1.0 - u[..., 0].astype(np.float64)))
    th = (np.float32(6.283185307179586) * u[..., 1]).astype(np.float32).astype(np.float64)
    return np.stack([rad * np.cos(th), rad * np.sin(th)], axis=-1).reshape(n_envs, -1)[:, :width]


def _widths(ch):
    return [ch.layer[0].n_in] + [ch.layer[i].n_out for i in range(ch.n_layers)]


def _lin(seq):
    return [x for x in seq if isinstance(x, nn.Linear)]


def _out(n, A):
    z = lambda w: torch.zeros(n, w)
    return dict(actions=z(A), mu=z(A), sigma=z(A), log_prob=z(1), values=z(1))


# ---- the struct and the new constant ------------------------------------------------------------------------------------------------------
def test_header_and_mirror_carry_the_new_fields():
    text = open(HEADER).read()
    assert int(re.search(r"#define LG_POLICY_LATENT_TAG (0x[0-9A-Fa-f]+)u", text).group(1), 16) == abi.POLICY_LATENT_TAG != abi.POLICY_STREAM_TAG
    names = [f for f, _ in abi.LgPolicyArgs._fields_]
    assert names[-4:] == ["encoder_b", "n_split", "has_split", "head"] and names.index("dbg_uniform") == len(names) - 5     # appended
    head = [f for f, _ in abi.LgPolicyHead._fields_]
    for f in head:
        assert re.search(rf"\b{f}\b", text), f
    assert {"H", "L", "E", "logvar_clip", "noise", "noise_stride", "latent_out", "params_out", "dbg_latent_uniform"} <= set(head)


# ---- descriptors --------------------------------------------------------------------------------------------------------------------------
def _check_ts(m, d, clip, n=7):
    spec = policy.describe(m)
    assert spec.family == "ts" and spec.chain_order == ["privilege_encoder", "history_encoder", "actor", "critic"]
    assert spec.clip_actions == clip and spec.num_actions == d["A"] and (spec.obs_width, spec.latent_width) == (d["obs"], d["latent"])
    z = lambda w: torch.zeros(n, w)
    obs, priv, hist, cobs, t = z(d["obs"]), z(d["priv"]), z(d["hist"]), z(d["cobs"]), _out(n, d["A"])
    cnt = torch.zeros(1, dtype=torch.int32)
    pe, he = _lin(m.privilege_encoder), _lin(m.history_encoder)
    a = policy.policy_args(spec, obs, cobs, counter=cnt, privileged_obs=priv, **t)                       # the teacher, as PPO_TS.act
    assert _widths(a.estimator) == [d["priv"]] + d["penc"] + [d["latent"]] and a.estimator.input == priv.data_ptr()
    assert (a.estimator.in_width, a.estimator.in_stride, a.estimator.out) == (d["priv"], d["priv"], None)
    assert a.estimator.layer[0].weight == pe[0].weight.data_ptr() and a.estimator.layer[len(pe) - 1].bias == pe[-1].bias.data_ptr()   # in place
    assert [a.estimator.layer[i].elu for i in range(len(pe))] == [1] * len(d["penc"]) + [0]
    assert _widths(a.actor) == [d["obs"] + d["latent"]] + d["actor"] + [d["A"]]
    assert (a.actor.input, a.actor.in_width, a.actor.in_stride) == (obs.data_ptr(), d["obs"], d["obs"])
    assert _widths(a.critic) == [d["cobs"]] + d["critic"] + [1] and a.critic.input == cobs.data_ptr()
    assert (a.encoder_b.n_layers, a.n_split, a.has_split, a.head.H, a.head.L, a.head.E) == (0, 0, 0, 0, 0, 0)
    assert a.counter == cnt.data_ptr() and a.std == m.std.data_ptr()
    s = policy.policy_args(spec, obs, None, mu=t["mu"], flags=abi.POLICY_DETERMINISTIC, obs_history=hist, student=True)       # act_student
    assert _widths(s.estimator) == [d["hist"]] + d["henc"] + [d["latent"]] and s.estimator.input == hist.data_ptr()
    assert s.estimator.layer[0].weight == he[0].weight.data_ptr() and s.encoder_b.n_layers == 0 and s.actions is None and s.critic.n_layers == 0
    s = policy.policy_args(spec, obs, None, mu=t["mu"], flags=abi.POLICY_DETERMINISTIC, privileged_obs=priv)                  # act_teacher
    assert s.estimator.input == priv.data_ptr() and s.estimator.layer[0].weight == pe[0].weight.data_ptr() and s.has_split == 0
    for k in (0, 3, n):                                                                                  # CTS: both chains, full-N tensors
        c = policy.policy_args(spec, obs, cobs, counter=cnt, privileged_obs=priv, obs_history=hist, num_teacher=k, **t)
        assert (c.n_split, c.has_split) == (k, 1)
        assert _widths(c.estimator) == [d["priv"]] + d["penc"] + [d["latent"]] and c.estimator.input == priv.data_ptr()
        assert _widths(c.encoder_b) == [d["hist"]] + d["henc"] + [d["latent"]] and c.encoder_b.input == hist.data_ptr()
        assert (c.encoder_b.in_width, c.encoder_b.in_stride) == (d["hist"], d["hist"])
        assert c.encoder_b.layer[0].weight == he[0].weight.data_ptr() and c.encoder_b.layer[len(he) - 1].bias == he[-1].bias.data_ptr()
        assert c.head.H == 0 and c.critic.n_layers == len(d["critic"]) + 1
    v = policy.policy_args(spec, None, cobs, values=t["values"], flags=abi.POLICY_VALUES_ONLY)
    assert v.actor.n_layers == 0 and v.estimator.n_layers == 0 and v.critic.n_layers == len(d["critic"]) + 1
    return a, c


def _check_dwaq(m, d, clip, n=7):
    spec = policy.describe(m)
    assert spec.family == "dreamwaq" and spec.chain_order == ["vae.encoder", "actor", "critic"]
    L, E, W = d["L"], d["E"], d["L"] + d["E"]
    assert spec.clip_actions == clip and (spec.obs_width, spec.latent_width) == (d["obs"], W) and spec.head.clip == d["logvar_clip"]
    z = lambda w: torch.zeros(n, w)
    obs, hist, cobs, t = z(d["obs"]), z(d["hist"]), z(d["cobs"]), _out(n, d["A"])
    cnt, eps, lat, par = torch.zeros(1, dtype=torch.int32), z(W), z(W + 3)[:, :W], z(2 * W)
    v = m.vae
    enc = _lin(v.encoder)
    a = policy.policy_args(spec, obs, cobs, counter=cnt, obs_history=hist, latent=lat, latent_params=par, **t)
    assert _widths(a.estimator) == [d["hist"]] + d["enc"] + [d["H"]] and a.estimator.input == hist.data_ptr()
    assert [a.estimator.layer[i].elu for i in range(len(enc))] == [1] * len(enc)                        # the trailing ELU is carried
    assert a.estimator.layer[0].weight == enc[0].weight.data_ptr()
    h = a.head
    assert (h.H, h.L, h.E, h.logvar_clip) == (d["H"], L, E, d["logvar_clip"])
    assert (h.latent_mu_w, h.latent_mu_b) == (v.latent_mu.weight.data_ptr(), v.latent_mu.bias.data_ptr())             # in place
    assert (h.latent_var_w, h.latent_var_b) == (v.latent_var[0].weight.data_ptr(), v.latent_var[0].bias.data_ptr())
    assert (h.vel_mu_w, h.vel_mu_b) == (v.vel_mu.weight.data_ptr(), v.vel_mu.bias.data_ptr())
    assert (h.vel_var_w, h.vel_var_b) == (v.vel_var[0].weight.data_ptr(), v.vel_var[0].bias.data_ptr())
    assert (h.noise, h.latent_out, h.latent_stride, h.params_out, h.params_stride) == (None, lat.data_ptr(), W + 3, par.data_ptr(), 2 * W)
    assert a.counter == cnt.data_ptr() and (a.encoder_b.n_layers, a.n_split, a.has_split) == (0, 0, 0)
    assert _widths(a.actor) == [d["obs"] + W] + d["actor"] + [d["A"]] and (a.actor.input, a.actor.in_width) == (obs.data_ptr(), d["obs"])
    assert _widths(a.critic) == [d["cobs"]] + d["critic"] + [1]
    b = policy.policy_args(spec, obs, cobs, obs_history=hist, latent_noise=eps, noise=z(d["A"]), **t)    # both draws injected: no counter
    assert (b.head.noise, b.head.noise_stride, b.counter, b.head.latent_out) == (eps.data_ptr(), W, None, None)
    b = policy.policy_args(spec, obs, cobs, counter=cnt, obs_history=hist, latent_noise=eps, **t)         # the action draw still needs it
    assert b.counter == cnt.data_ptr()
    s = policy.policy_args(spec, obs, None, mu=t["mu"], flags=abi.POLICY_DETERMINISTIC, obs_history=hist, latent=lat)         # act_inference
    assert s.head.H == d["H"] and s.head.noise is None and s.head.latent_out == lat.data_ptr() and s.actions is None and s.counter is None
    return a


@pytest.mark.parametrize("name", list(TS_NETS))
def test_descriptor_of_ts_stand_ins(name):
    a, c = _check_ts(make_ts(name), TS_NETS[name], 0.05)
    lib = abi.load_lib()                      # the launch plan alone: nothing is enqueued
    assert lib.lg_policy_row_tile(C.byref(a)) == ROW_TILE[name], lib.lg_last_error()
    assert lib.lg_policy_row_tile(C.byref(c)) == ROW_TILE[name], lib.lg_last_error()


@pytest.mark.parametrize("name", list(DWAQ_NETS))
def test_descriptor_of_dreamwaq_stand_ins(name):
    a = _check_dwaq(make_dwaq(name), DWAQ_NETS[name], 0.05)
    lib = abi.load_lib()
    assert lib.lg_policy_row_tile(C.byref(a)) == ROW_TILE[name], lib.lg_last_error()


def _reference_family_modules():
    from tests.golden.ref_harness import REF
    d = os.path.join(REF, "rsl_rl", "modules")
    if not os.path.exists(os.path.join(d, "actor_critic_dreamwaq.py")):
        pytest.skip("no reference checkout (LG_REFERENCE)")
    names = ("rsl_rl", "rsl_rl.modules")             # actor_critic_dreamwaq.py imports rsl_rl.modules.actor_critic_ts by its absolute name
    saved = {k: sys.modules.get(k) for k in names}
    out = {}
    try:
        for k in names:
            pkg = types.ModuleType(k)
            pkg.__path__ = [d] if k.endswith("modules") else []
            sys.modules[k] = pkg
        for n in ("actor_critic", "vae", "actor_critic_ts", "actor_critic_cts", "actor_critic_dreamwaq"):
            sp = importlib.util.spec_from_file_location(f"rsl_rl.modules.{n}", os.path.join(d, n + ".py"))
            mod = importlib.util.module_from_spec(sp)
            sys.modules[sp.name] = mod
            sp.loader.exec_module(mod)
            out[n] = mod
    finally:
        for k in [k for k in sys.modules if k == "rsl_rl" or k.startswith("rsl_rl.")]:
            del sys.modules[k]
        for k, v in saved.items():
            if v is not None:
                sys.modules[k] = v
    return out["actor_critic_ts"].ActorCriticTS, out["actor_critic_cts"].ActorCriticCTS, out["actor_critic_dreamwaq"].ActorCriticDreamWaQ


def test_descriptor_of_reference_modules(capsys):
    TS, CTS, DWAQ = _reference_family_modules()
    d = TS_NETS["go2_ts"]
    for cls in (TS, CTS):
        m = cls(d["obs"], d["A"], d["priv"], d["hist"], d["latent"], d["cobs"], d["actor"], d["critic"], d["penc"],
                **({"history_encoder_type": "MLP"} if cls is TS else {}), history_encoder_hidden_dims=d["henc"])
        _check_ts(m, d, None)
    d = DWAQ_NETS["go2_dreamwaq"]
    m = DWAQ(d["obs"], d["A"], d["cobs"], d["hist"], d["L"], d["E"], d["obs"], d["actor"], d["critic"], d["enc"], [64, 32])
    assert d["H"] == 2 * d["L"] + 2 * d["E"]          # vae.py:32: the reference's encoder ends at 2L + 2E
    _check_dwaq(m, d, None)


# ---- refusals: all before the library is touched -----------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(abi, "load_lib", boom)


def test_refusals_name_the_layer_or_the_argument(no_library):
    """`describe` and `policy_args`, which is where `FusedPolicy.act` / `act_teacher` / ... form their descriptor before the entry point
    is called.  They are exercised directly and not through a `FusedPolicy`, because its constructor loads the library (and wants a HIP
    device), which this test forbids."""
    d = TS_NETS["tiny_ts"]
    z = lambda w, n=4: torch.zeros(n, w)
    m = make_ts("tiny_ts")
    m.history_encoder = nn.Sequential(nn.Conv1d(1, 4, 5), nn.Flatten(), nn.Linear(28, 3))             # the "TCN" option
    with pytest.raises(ValueError, match=r"history_encoder\[0\] is Conv1d"):
        policy.describe(m)
    m = make_ts("tiny_ts")
    m.history_encoder[2] = nn.Linear(10, 4)
    with pytest.raises(ValueError, match="privilege_encoder gives 3 latent dims, history_encoder 4"):
        policy.describe(m)
    m = make_dwaq("tiny_dwaq")
    m.vae.latent_var[1] = nn.Hardtanh(-5.0, 4.0)
    with pytest.raises(ValueError, match=r"vae\.latent_var\[1\] \(Hardtanh\(-5.0, 4.0\)\) must be a symmetric clip"):
        policy.describe(m)
    m = make_dwaq("tiny_dwaq")
    m.vae.vel_var[1] = nn.Hardtanh(-4.0, 4.0)
    with pytest.raises(ValueError, match=r"vae\.latent_var clips to 5.0, vae\.vel_var to 4.0"):
        policy.describe(m)
    m = make_dwaq("tiny_dwaq")
    m.vae.vel_mu = nn.Linear(9, 2)
    with pytest.raises(ValueError, match=r"vae\.vel_mu takes 9 inputs, vae\.latent_mu 10"):
        policy.describe(m)
    m = make_dwaq("tiny_dwaq")
    m.vae.latent_mu = nn.Sequential(nn.Linear(10, 3))
    with pytest.raises(ValueError, match=r"vae\.latent_mu is Sequential, expected a Linear"):
        policy.describe(m)
    # latent width != actor input - obs: the actor of tiny_ts takes 8 = 5 + 3, here the obs rows are 6 wide
    spec = policy.describe(make_ts("tiny_ts"))
    t = _out(4, 3)
    with pytest.raises(ValueError, match=r"actor\[0\] takes 8 inputs, \(obs, latent\) has 6 \+ 3"):
        policy.policy_args(spec, z(6), z(6), privileged_obs=z(7), **t)
    dspec = policy.describe(make_dwaq("tiny_dwaq"))
    with pytest.raises(ValueError, match=r"actor\[0\] takes 10 inputs, \(obs, latent\) has 4 \+ 5"):
        policy.policy_args(dspec, z(4), z(6), obs_history=z(11), **t)
    for k in (-1, 5, 2.5):
        with pytest.raises(ValueError, match=r"num_teacher=.* is outside \[0, 4\]"):
            policy.policy_args(spec, z(5), z(6), privileged_obs=z(7), obs_history=z(11), num_teacher=k, **t)
    with pytest.raises(ValueError, match="privileged_obs is missing"):
        policy.policy_args(spec, z(5), z(6), **t)
    with pytest.raises(ValueError, match="obs_history is missing"):
        policy.policy_args(spec, z(5), z(6), privileged_obs=z(7), num_teacher=2, **t)
    with pytest.raises(ValueError, match="obs_history is missing"):
        policy.policy_args(spec, z(5), None, mu=t["mu"], flags=abi.POLICY_DETERMINISTIC, student=True)
    with pytest.raises(ValueError, match="privileged_obs must be"):
        policy.policy_args(spec, z(5), z(6), privileged_obs=z(7, 3), **t)
    with pytest.raises(ValueError, match="latent_noise was given, the module has no .vae"):
        policy.policy_args(spec, z(5), z(6), privileged_obs=z(7), latent_noise=z(5), **t)
    with pytest.raises(ValueError, match="obs_history is missing"):
        policy.policy_args(dspec, z(5), z(6), **t)
    with pytest.raises(ValueError, match="privileged_obs was given, the module has no .privilege_encoder"):
        policy.policy_args(dspec, z(5), z(6), obs_history=z(11), privileged_obs=z(7), **t)
    with pytest.raises(ValueError, match="latent_noise must be"):
        policy.policy_args(dspec, z(5), z(6), obs_history=z(11), latent_noise=z(4), **t)
    from tests.test_policy_host import make_net
    plain = policy.describe(make_net("tiny"))
    with pytest.raises(ValueError, match="obs_history was given, the module has neither"):
        policy.policy_args(plain, z(5), z(6), obs_history=z(11), **t)
    with pytest.raises(ValueError, match="num_teacher was given"):
        policy.policy_args(plain, z(5), z(6), num_teacher=2, **t)
    m = make_ts("tiny_ts")
    m.estimator = mlp(5, [4], 2)
    with pytest.raises(ValueError, match="one family at a time"):
        policy.describe(m)


def test_host_entry_point_refuses_before_a_launch():
    """Each refusal include/lgpolicy.h lists for the new fields, through lg_policy_row_tile / lg_policy_act(..., None): nothing is enqueued
    (there is no device here)."""
    lib = abi.load_lib()
    z = lambda w: torch.zeros(4, w)
    t = _out(4, 3)
    spec, dspec = policy.describe(make_ts("tiny_ts")), policy.describe(make_dwaq("tiny_dwaq"))
    keep = [z(5), z(6), z(7), z(11), z(3), z(5)]                                   # alive while the descriptors point at them
    obs, cobs, priv, hist, noise, eps = keep
    cts = lambda: policy.policy_args(spec, obs, cobs, privileged_obs=priv, obs_history=hist, num_teacher=2, noise=noise, **t)
    dw = lambda **kw: policy.policy_args(dspec, obs, cobs, obs_history=hist, noise=noise, latent_noise=eps, **t, **kw)

    def refused(a, msg, act=False):
        rc = lib.lg_policy_act(C.byref(a), None) != 0 if act else lib.lg_policy_row_tile(C.byref(a)) == 0
        assert rc and msg in lib.lg_last_error(), (msg, lib.lg_last_error())

    assert lib.lg_policy_row_tile(C.byref(cts())) == 32 and lib.lg_policy_row_tile(C.byref(dw())) == 32
    for k in (-1, 5):
        a = cts()
        a.n_split = k
        refused(a, b"n_split outside [0, n_envs]", act=k == 5)
    a = cts()
    a.has_split = 0
    refused(a, b"encoder_b without n_split")
    a = cts()
    a.encoder_b.n_layers = 0
    refused(a, b"n_split without encoder_b", act=True)
    a = policy.policy_args(spec, obs, cobs, privileged_obs=priv, noise=noise, **t)
    a.n_split = 2
    refused(a, b"n_split without encoder_b")
    a = cts()
    a.encoder_b.layer[1].n_out = 4
    refused(a, b"the group chains end at different widths (3, 4)")
    a = cts()
    a.encoder_b.layer[1].n_in = 9
    refused(a, b"encoder_b: layer 1 takes 9 inputs")
    a = dw()
    a.head.H = 9
    refused(a, b"head takes H = 9 inputs, the estimator chain gives 10", act=True)
    a = dw()
    a.head.E = 1
    refused(a, b"actor: layer 0 takes 10 inputs, its input has 9")
    a = dw()
    b = cts()
    a.encoder_b, a.n_split, a.has_split = b.encoder_b, 2, 1
    refused(a, b"the VAE head and encoder_b exclude each other", act=True)
    a = dw()
    a.head.noise = None
    refused(a, b"neither latent noise nor a Philox counter", act=True)
    a = dw()
    a.head.noise_stride = 4
    refused(a, b"head noise_stride < L + E")
    lat, par = z(5), z(10)
    a = dw(latent=lat, latent_params=par)
    assert lib.lg_policy_row_tile(C.byref(a)) == 32
    a.head.latent_stride = 4
    refused(a, b"latent_stride < L + E", act=True)
    a = dw(latent=lat, latent_params=par)
    a.head.params_stride = 9
    refused(a, b"params_stride < 2 L + 2 E")
    a = dw()
    a.head.latent_var_b = None
    refused(a, b"null head weight or bias")
    a = dw()
    a.actor.in_width = a.actor.in_stride = 2044                                    # (obs | latent) = 2049 wide
    refused(a, b"actor input (obs, latent) wider than 2048", act=True)
    a = cts()
    a.actor.in_width = a.actor.in_stride = 2046
    refused(a, b"wider than 2048")
    lab = z(3)
    a = cts()
    a.encoder_b.out, a.encoder_b.out_stride = lab.data_ptr(), 2
    refused(a, b"encoder_b out_stride < width", act=True)
    a.encoder_b.out_stride = 3                                                     # ... and a wide enough one plans
    assert lib.lg_policy_row_tile(C.byref(a)) == 32
    a = cts()
    a.estimator.n_layers = 0
    refused(a, b"encoder_b without an estimator chain")
    a = dw()
    a.estimator.n_layers = 0
    refused(a, b"the VAE head needs the estimator chain", act=True)
    a = dw()                                                                       # a descriptor without the new fields plans as before
    a.head = abi.LgPolicyHead()
    refused(a, b"actor: layer 0 takes 10 inputs, its input has 15")


# ---- the latent draw ----------------------------------------------------------------------------------------------------------------------
def test_latent_draw_restatement():
    seed = (0x1234 << 32) | 0xBEEF
    z = latent_normals(seed, 7, 2048, 40)
    assert z.shape == (2048, 40) and np.isfinite(z).all()
    assert np.array_equal(z[100:200], latent_normals(seed, 7, 200, 40)[100:])        # a pure function of (seed, counter, env, column)
    assert np.array_equal(z[:, :5], latent_normals(seed, 7, 2048, 5))                # ... and not of the width
    u = latent_uniforms(seed, 7, 2048, 5)
    assert u.shape == (2048, 8) and u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    # the same (env, quad, counter) on the action stream: other uniforms everywhere, so the two draws of one call are independent
    ua = philox_uniforms(seed, 7, 2048, 8)
    assert ua.shape == u.shape and not np.any(u == ua)
    assert not np.any(z[:, :12] == philox_normals(seed, 7, 2048, 12))
    assert not np.any(z == latent_normals(seed, 8, 2048, 40))                        # the shared counter cell: fresh numbers per call
    n = z.size                                                                       # 5-sigma bounds of the moments, n = 81 920
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n)
    # one block by hand against oracle/philox.py: env 3, quad 1 -> columns 4 .. 7
    w = philox.philox4x32_10(np.uint64(3), np.uint64(1), 7, abi.POLICY_LATENT_TAG, seed & 0xFFFFFFFF, seed >> 32)
    assert np.array_equal(np.array([philox.u01(x) for x in w], np.float32).reshape(-1), latent_uniforms(seed, 7, 4, 8)[3, 4:8])


# ---- discrimination: what a wrong kernel would give is far outside the parity bound -----------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_ts", "go2_cts"])
def test_parity_rule_fails_the_other_groups_encoder(name):
    d = TS_NETS[name]
    m = make_ts(name, clip=None)
    g = torch.Generator().manual_seed(11)
    n = 33
    obs, priv, hist = (torch.randn(n, d[k], generator=g) for k in ("obs", "priv", "hist"))
    m64 = copy.deepcopy(m).double()
    with torch.no_grad():
        for student, x in ((False, priv), (True, hist)):
            ref = m64.mean(obs.double(), x.double(), student).numpy()
            bound = parity_bound(max_err(m.mean(obs, x, student).numpy(), ref), ref)
            # what a tile on the wrong side of the split computes: the other group's encoder on the other group's input
            other = m64.mean(obs.double(), (priv if student else hist).double(), not student).numpy()
            per_row = np.abs(other - ref).max(axis=1)
            print(f"{name} student={student}: bound {bound:.3e}, smallest per-row distance to the other group's mean {per_row.min():.3e}")
            assert per_row.min() > 100 * bound


@pytest.mark.parametrize("name", list(DWAQ_NETS))
def test_parity_rule_fails_a_dropped_clip_and_swapped_latents(name):
    d = DWAQ_NETS[name]
    m = make_dwaq(name, clip=None)
    g = torch.Generator().manual_seed(11)
    n = 33
    obs, hist, eps = torch.randn(n, d["obs"], generator=g), torch.randn(n, d["hist"], generator=g), torch.randn(n, d["L"] + d["E"], generator=g)
    m64 = copy.deepcopy(m).double()
    with torch.no_grad():
        ref = {k: v.numpy() for k, v in m64.forward_all(obs.double(), hist.double(), eps.double()).items()}
        f32 = {k: v.numpy() for k, v in m.forward_all(obs, hist, eps).items()}
        raw = {k: v.numpy() for k, v in m64.forward_all(obs.double(), hist.double(), eps.double(), drop_clip=True).items()}
        swp = {k: v.numpy() for k, v in m64.forward_all(obs.double(), hist.double(), eps.double(), swap=True).items()}
    L, E, c = d["L"], d["E"], d["logvar_clip"]
    lv = np.concatenate((raw["params"][:, L:2 * L], raw["params"][:, 2 * L + E:]), axis=1)         # the unclipped log-variances
    assert (lv < -c).any() and (lv > c).any() and ((lv > -c) & (lv < c)).any()                      # the clip test cannot be empty
    for k in ("params", "latent", "mu"):
        bound = parity_bound(max_err(f32[k], ref[k]), ref[k])
        print(f"{name} {k}: bound {bound:.3e}, dropped clip {max_err(raw[k], ref[k]):.3e}, swapped (z, vel) {max_err(swp[k], ref[k]):.3e}")
        assert max_err(raw[k], ref[k]) > 100 * bound, k
        if k != "params":
            assert max_err(swp[k], ref[k]) > 100 * bound, k
    assert PARITY_FACTOR == 8.0

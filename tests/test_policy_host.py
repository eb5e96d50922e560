"""Host side of the fused policy step (hcr_genesis_lr_cl_amd/policy.py, include/lgpolicy.h): the ctypes mirror against the header, the
descriptor `FusedPolicy` builds for every reference net set, its refusals, and the numpy restatements that tests/test_gpu_policy.py checks
the kernel against -- the Philox-normal draw (on oracle/philox.py) and the forward-parity rule.  No GPU needed: nothing is launched."""
import copy
import ctypes as C
import importlib.util
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from hcr_genesis_lr_cl_amd import abi, policy
from oracle import philox

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lgpolicy.h")

# (estimator features or actor obs, estimator hidden / labels or None, actor hidden, actions, critic obs, critic hidden): bench.py::ppo_rollout
NETS = {
    "tiny": dict(obs=5, est=None, actor=[33, 7], A=3, cobs=6, critic=[33, 7]),                 # no dimension is a tile multiple
    "go2": dict(obs=45, est=None, actor=[512, 256, 128], A=12, cobs=45, critic=[512, 256, 128]),
    "go2_ee": dict(obs=900, est=([256, 128], 24), actor=[512, 256, 128], A=12, cobs=870, critic=[1024, 256, 128]),
    "tron1_pf_ee": dict(obs=310, est=([256, 128], 17), actor=[512, 256, 128], A=6, cobs=1340, critic=[1024, 256, 128]),
}


def mlp(i, hidden, o, tail=None):
    layers, d = [], i
    for h in hidden:
        layers += [nn.Linear(d, h), nn.ELU()]
        d = h
    layers.append(nn.Linear(d, o))
    if tail is not None:
        layers.append(tail)
    return nn.Sequential(*layers)


class StandIn(nn.Module):
    """An rsl_rl-style actor-critic by duck typing: .actor, .critic, optional .estimator, .std."""
    is_recurrent = False

    def __init__(self, actor, critic, std, estimator=None):
        super().__init__()
        self.actor, self.critic = actor, critic
        if estimator is not None:
            self.estimator = estimator
        self.std = nn.Parameter(std)

    def mean(self, obs):
        return self.actor(torch.cat((obs, self.estimator(obs)), dim=-1)) if hasattr(self, "estimator") else self.actor(obs)


def make_net(name, clip=0.05, seed=3):
    """The net set `name` with seeded weights: uniform +-1.5 / sqrt(in) and biases +-0.5, so that hidden pre-activations take both signs (the
    ELU branch) and actor outputs pass the small `clip` (the Hardtanh branch); std in [0.5, 1.5)."""
    d = NETS[name]
    E = d["est"][1] if d["est"] else 0
    est = mlp(d["obs"], d["est"][0], E) if d["est"] else None
    m = StandIn(mlp(d["obs"] + E, d["actor"], d["A"], nn.Hardtanh(-clip, clip) if clip is not None else None), mlp(d["cobs"], d["critic"], 1),
                torch.ones(d["A"]), est)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.Linear):
                mod.weight.copy_((torch.rand(mod.weight.shape, generator=g) * 2 - 1) * 1.5 / mod.in_features ** 0.5)
                mod.bias.copy_(torch.rand(mod.bias.shape, generator=g) - 0.5)
        m.std.copy_(0.5 + torch.rand(d["A"], generator=g))
    return m


# ---- numpy restatements -----------------------------------------------------------------------------------------------------------------
def philox_uniforms(seed, counter, n_envs, num_actions):
    """(N, 4 * Q) float32: the uniforms of include/lgpolicy.h -- counter (env, action quad, call counter, stream tag), key = seed."""
    q = (num_actions + 3) // 4
    env, quad = np.meshgrid(np.arange(n_envs, dtype=np.uint64), np.arange(q, dtype=np.uint64), indexing="ij")
    w = philox.philox4x32_10(env, quad, counter, abi.POLICY_STREAM_TAG, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.stack([philox.u01(x) for x in w], axis=-1).reshape(n_envs, 4 * q)


def philox_normals(seed, counter, n_envs, num_actions):
    """(N, A) float64: Box-Muller on each pair of uniforms, r = sqrt(-2 log(1 - u0)), angle = float32(2 pi) * u1 rounded to float32 as the
    kernel forms it; the transcendental functions in float64."""
    u = philox_uniforms(seed, counter, n_envs, num_actions).reshape(n_envs, -1, 2)
    rad = np.sqrt(-2.0 * np.log(1.0 - u[..., 0].astype(np.float64)))
    th = (np.float32(6.283185307179586) * u[..., 1]).astype(np.float32).astype(np.float64)
    z = np.stack([rad * np.cos(th), rad * np.sin(th)], axis=-1).reshape(n_envs, -1)
    return z[:, :num_actions]


def np_forward(seq, x, drop_last_column=False):
    """A float32 restatement of an nn.Sequential of Linear / ELU / Hardtanh; `drop_last_column` is the deliberately wrong K tail: the last
    input column of every Linear is left out of the sum."""
    x = np.asarray(x, np.float32)
    for m in seq:
        if isinstance(m, nn.Linear):
            w, b = m.weight.detach().numpy().astype(np.float32), m.bias.detach().numpy().astype(np.float32)
            k = w.shape[1] - (1 if drop_last_column else 0)
            x = (x[:, :k] @ w[:, :k].T + b).astype(np.float32)
        elif isinstance(m, nn.ELU):
            x = np.where(x > 0, x, np.expm1(np.minimum(x, 0))).astype(np.float32)
        elif isinstance(m, nn.Hardtanh):
            x = np.clip(x, m.min_val, m.max_val).astype(np.float32)
    return x


# The forward-parity rule.  The kernel, torch's CPU GEMM and numpy's all form each output as a float32 sum of the same K products and
# differ in the ORDER: the MFMA is one sequential fmaf chain per output (rounding error a random walk of K steps), a CPU GEMM keeps 8 to 16
# vector-lane partial sums per output (K / 16 steps each, then a short tree): in the random-walk model the chain is up to sqrt(16) = 4 times
# the blocked sum.  A factor 2 covers the max-over-outputs statistic of a few hundred to a few thousand samples and expm1's last-ulp
# differences between a device and a host libm.  Hence 8.  An error below one float32 ulp of the largest output is not resolvable and is
# lifted to it: that floor comes from the number format, not from either implementation.
PARITY_FACTOR = 8.0


def parity_bound(err_torch_f32, ref64):
    return PARITY_FACTOR * max(float(err_torch_f32), float(np.abs(ref64).max()) * 2.0 ** -23)


def max_err(x, ref64):
    return float(np.abs(np.asarray(x, np.float64) - ref64).max())


# ---- the struct ---------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header():
    structs = [("LgPolicyLayer", abi.LgPolicyLayer), ("LgPolicyChain", abi.LgPolicyChain), ("LgPolicyArgs", abi.LgPolicyArgs)]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs:
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['printf("MAX_LAYERS %d\\n", LG_POLICY_MAX_LAYERS);', 'printf("MAX_WIDTH %d\\n", LG_POLICY_MAX_WIDTH);',
              'printf("DETERMINISTIC %u\\n", LG_POLICY_DETERMINISTIC);', 'printf("VALUES_ONLY %u\\n", LG_POLICY_VALUES_ONLY);',
              'printf("STREAM_TAG %u\\n", LG_POLICY_STREAM_TAG);', "return 0;}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        with open(src, "w") as f:
            f.write("\n".join(lines))
        subprocess.run(["gcc", "-o", exe, src], check=True)
        got = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for cname, cls in structs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert (int(got["MAX_LAYERS"]), int(got["MAX_WIDTH"])) == (abi.POLICY_MAX_LAYERS, abi.POLICY_MAX_WIDTH)
    assert (int(got["DETERMINISTIC"]), int(got["VALUES_ONLY"]), int(got["STREAM_TAG"])) == (abi.POLICY_DETERMINISTIC, abi.POLICY_VALUES_ONLY,
                                                                                              abi.POLICY_STREAM_TAG)


def test_library_exports_the_policy_entry_points():
    import re
    declared = set(re.findall(r"\b(lg_\w+)\s*\(", open(HEADER).read()))
    assert declared == set(abi.POLICY_EXPORTS)
    lib = C.CDLL(abi.lib_path())
    for sym in declared:
        assert hasattr(lib, sym), sym


# ---- the descriptor -----------------------------------------------------------------------------------------------------------------------
def _chain_widths(ch):
    return [ch.layer[0].n_in] + [ch.layer[i].n_out for i in range(ch.n_layers)]


def _check_descriptor(m, d, clip, n=7):
    spec = policy.describe(m)
    E = d["est"][1] if d["est"] else 0
    assert spec.chain_order == (["estimator"] if d["est"] else []) + ["actor", "critic"]
    assert spec.concat is bool(d["est"]) and spec.clip_actions == clip and spec.num_actions == d["A"]
    A = d["A"]
    z = lambda w: torch.zeros(n, w)
    obs, cobs, lab = z(d["obs"]), z(d["cobs"]), (z(E) if E else None)
    t = dict(actions=z(A), mu=z(A), sigma=z(A), log_prob=z(1), values=z(1))
    a = policy.policy_args(spec, obs, cobs, labels=lab, counter=torch.zeros(1, dtype=torch.int32), seed=(5 << 32) | 9, **t)
    assert a.n_envs == n and a.flags == 0 and a.seed == (5 << 32) | 9
    assert _chain_widths(a.actor) == [d["obs"] + E] + d["actor"] + [A]
    assert _chain_widths(a.critic) == [d["cobs"]] + d["critic"] + [1]
    assert (a.actor.in_width, a.actor.in_stride, a.actor.input) == (d["obs"], d["obs"], obs.data_ptr())     # the features part of the concatenation
    assert [a.actor.layer[i].elu for i in range(a.actor.n_layers)] == [1] * len(d["actor"]) + [0]
    if d["est"]:
        assert _chain_widths(a.estimator) == [d["obs"]] + d["est"][0] + [E]
        assert a.estimator.input == obs.data_ptr() and a.estimator.out == lab.data_ptr() and a.estimator.out_stride == E
    else:
        assert a.estimator.n_layers == 0
    assert (a.clip_on, a.clip_actions) == ((1, np.float32(clip)) if clip is not None else (0, 0.0))
    lin = [x for x in m.actor if isinstance(x, nn.Linear)]
    assert a.actor.layer[0].weight == lin[0].weight.data_ptr() and a.actor.layer[a.actor.n_layers - 1].bias == lin[-1].bias.data_ptr()   # in place
    assert a.std == m.std.data_ptr() and a.critic.out == t["values"].data_ptr() and a.log_prob_stride == 1 and a.mu_stride == A
    return a


@pytest.mark.parametrize("name", list(NETS))
def test_descriptor_of_stand_ins(name):
    a = _check_descriptor(make_net(name, clip=0.05), NETS[name], 0.05)
    lib = abi.load_lib()                      # the launch plan alone: nothing is enqueued
    assert lib.lg_policy_row_tile(C.byref(a)) == {"tiny": 32, "go2": 32, "go2_ee": 16, "tron1_pf_ee": 16}[name]


def test_descriptor_modes():
    m, d = make_net("go2_ee"), NETS["go2_ee"]
    spec = policy.describe(m)
    a = policy.policy_args(spec, torch.zeros(3, 900), mu=torch.zeros(3, 12), flags=abi.POLICY_DETERMINISTIC)
    assert a.critic.n_layers == 0 and a.actions is None and a.estimator.n_layers == 3 and a.n_envs == 3
    a = policy.policy_args(spec, None, torch.zeros(4, 870), values=torch.zeros(4, 1), flags=abi.POLICY_VALUES_ONLY)
    assert a.actor.n_layers == 0 and a.critic.n_layers == 4 and a.n_envs == 4
    rows = torch.zeros(5, 64)                                                     # a strided view is addressed in place
    a = policy.policy_args(spec, torch.zeros(5, 900), None, actions=rows[:, :12], mu=rows[:, 16:28], sigma=rows[:, 32:44],
                           log_prob=rows[:, 48:49], noise=torch.zeros(5, 12))
    assert a.actions_stride == 64 and a.mu == rows.data_ptr() + 64 and a.critic.n_layers == 0 and a.counter is None


def _reference_modules():
    from tests.golden.ref_harness import REF
    d = os.path.join(REF, "rsl_rl", "modules")
    if not os.path.exists(os.path.join(d, "actor_critic_ee.py")):
        pytest.skip("no reference checkout (LG_REFERENCE)")
    pkg = types.ModuleType("_ref_policy_modules")
    pkg.__path__ = [d]
    sys.modules[pkg.__name__] = pkg
    out = []
    for n in ("actor_critic", "actor_critic_ee"):
        sp = importlib.util.spec_from_file_location(f"{pkg.__name__}.{n}", os.path.join(d, n + ".py"))
        mod = importlib.util.module_from_spec(sp)
        sys.modules[sp.name] = mod
        sp.loader.exec_module(mod)
        out.append(mod)
    return out[0].ActorCritic, out[1].ActorCriticEE


def test_descriptor_of_reference_modules(capsys):
    ActorCritic, ActorCriticEE = _reference_modules()
    d = NETS["go2"]
    _check_descriptor(ActorCritic(d["obs"], d["cobs"], d["A"], d["actor"], d["critic"], clip_actions=100.0), d, 100.0)
    for name in ("go2_ee", "tron1_pf_ee"):
        d = NETS[name]
        m = ActorCriticEE(d["cobs"], d["A"], d["obs"], d["est"][1], d["actor"], d["critic"], d["est"][0], clip_actions=100.0)
        _check_descriptor(m, d, 100.0)


# ---- refusals: all before the library is touched ---------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(abi, "load_lib", boom)


def test_refusals_name_the_layer(no_library):
    dev = torch.device("cuda:0")
    with pytest.raises(ValueError, match="not on a HIP device"):
        policy.FusedPolicy(make_net("tiny"))
    with pytest.raises(ValueError, match=r"actor\[0\]\.weight is on cpu"):
        policy.describe(make_net("tiny"), dev)
    m = make_net("tiny")
    m.actor[1] = nn.Tanh()
    with pytest.raises(ValueError, match=r"actor\[1\] is Tanh"):
        policy.describe(m)
    m = make_net("tiny")
    m.critic[3] = nn.ELU(alpha=0.5)
    with pytest.raises(ValueError, match=r"critic\[3\] is ELU\(alpha=0.5\)"):
        policy.describe(m)
    m = make_net("tiny")
    m.critic.append(nn.Hardtanh(-1.0, 1.0))
    with pytest.raises(ValueError, match=r"critic\[5\] is Hardtanh"):
        policy.describe(m)
    m = make_net("tiny")
    m.actor[2] = m.actor[2].double()
    with pytest.raises(ValueError, match=r"actor\[2\]\.weight is torch.float64"):
        policy.describe(m)
    m = make_net("tiny")
    m.actor[0].weight.data = torch.zeros(5, 33).t()
    with pytest.raises(ValueError, match=r"actor\[0\]\.weight is not contiguous"):
        policy.describe(m)
    m = StandIn(mlp(5, [2049], 3), mlp(5, [7], 1), torch.ones(3))
    with pytest.raises(ValueError, match=r"actor\[0\] is 5 -> 2049, widths are limited to 2048"):
        policy.describe(m)
    m = StandIn(mlp(5, [8, 8, 8, 8], 3), mlp(5, [7], 1), torch.ones(3))
    with pytest.raises(ValueError, match="actor has 5 Linear layers"):
        policy.describe(m)
    m = make_net("tiny")
    m.is_recurrent = True
    with pytest.raises(ValueError, match="recurrent"):
        policy.describe(m)
    m = make_net("go2_ee")
    m.actor[0] = nn.Linear(900, 512)
    with pytest.raises(ValueError, match=r"actor\[0\] takes 900 inputs, \(features, estimator output\) has 900 \+ 24"):
        policy.describe(m)
    spec = policy.describe(make_net("tiny"))
    with pytest.raises(ValueError, match="obs must be"):
        policy.policy_args(spec, torch.zeros(4, 5, dtype=torch.float64), None, mu=torch.zeros(4, 3), flags=abi.POLICY_DETERMINISTIC)
    with pytest.raises(ValueError, match="noise must be"):
        z = lambda w: torch.zeros(4, w)
        policy.policy_args(spec, z(5), None, z(3), z(3), z(3), z(1), noise=torch.zeros(4, 6)[:, ::2])


def test_host_entry_point_refuses_before_a_launch():
    """What gets past Python still meets the entry point's own checks: nothing is enqueued (there is no device here)."""
    lib = abi.load_lib()
    spec = policy.describe(make_net("tiny"))
    z = lambda w: torch.zeros(4, w)
    mk = lambda: policy.policy_args(spec, z(5), z(6), z(3), z(3), z(3), z(1), z(1), noise=z(3))
    a = mk()
    a.actor.layer[1].n_in = 34
    assert lib.lg_policy_row_tile(C.byref(a)) == 0 and b"layer 1 takes 34 inputs" in lib.lg_last_error()
    a = mk()
    a.actor.layer[0].n_out = a.actor.layer[1].n_in = 4096
    assert lib.lg_policy_row_tile(C.byref(a)) == 0 and b"width outside" in lib.lg_last_error()
    a = mk()
    a.actor.n_layers = 5
    assert lib.lg_policy_act(C.byref(a), None) != 0 and b"1 .. 4 layers" in lib.lg_last_error()
    a = mk()
    a.noise = None
    assert lib.lg_policy_act(C.byref(a), None) != 0 and b"neither noise nor a Philox counter" in lib.lg_last_error()
    a = mk()
    a.flags = abi.POLICY_VALUES_ONLY
    a.critic.n_layers = 0
    assert lib.lg_policy_act(C.byref(a), None) != 0 and b"values_only without a critic" in lib.lg_last_error()


# ---- the draw -----------------------------------------------------------------------------------------------------------------------------
def test_philox_normal_restatement():
    seed = (0x1234 << 32) | 0xBEEF
    z = philox_normals(seed, 7, 4096, 12)
    assert z.shape == (4096, 12) and np.isfinite(z).all()
    assert np.array_equal(z, philox_normals(seed, 7, 4096, 12))                      # a pure function of (seed, counter, env, action)
    assert np.array_equal(z[100:200], philox_normals(seed, 7, 200, 12)[100:])        # ... and not of the batch
    z1 = philox_normals(seed, 8, 4096, 12)
    assert not np.any(z == z1)                                                       # successive counters: fresh numbers everywhere
    assert not np.any(z == philox_normals(seed + 1, 7, 4096, 12))
    u = philox_uniforms(seed, 7, 4096, 6)                                            # A = 6: two quads, the second half used
    assert u.shape == (4096, 8) and u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    assert philox_normals(seed, 7, 4096, 6).shape == (4096, 6)
    n = z.size                                                                       # 5-sigma bounds of the moments, n = 49 152
    assert abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n)
    assert abs(np.mean(z[:, 0] * z[:, 1])) < 5 / np.sqrt(4096)                       # the two normals of one pair are uncorrelated


# ---- the parity rule tells a wrong K tail from a summation order ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny", "go2"])
def test_parity_rule_fails_a_dropped_last_column(name):
    m, d = make_net(name), NETS[name]
    x = torch.randn(33, d["obs"], generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ref = copy.deepcopy(m).double().actor(x.double()).numpy()
        err_torch = max_err(m.actor(x).numpy(), ref)
    bound = parity_bound(err_torch, ref)
    good, bad = np_forward(m.actor, x.numpy()), np_forward(m.actor, x.numpy(), drop_last_column=True)
    assert np.abs(ref).max() == 0.05 and np.abs(ref).min() < 0.05                    # both Hardtanh branches are exercised
    assert max_err(good, ref) <= bound                                               # another summation order passes
    assert max_err(bad, ref) > 100 * bound                                           # the wrong tail does not, by a wide margin

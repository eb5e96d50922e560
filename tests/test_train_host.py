"""Host side of the fused learner pass (hcr_genesis_lr_cl_amd/train.py, include/lgtrain.h): the ctypes mirror against the header, the
exports and the translation unit, the float64 restatement of tests/train_cases.py against the golden fixture of the reference's own
PPO.update() (tests/golden/ppo_train.npz) and against torch float64 autograd, every refusal of the entry points and of the Python
surface, the plan of lg_train_plan against the restated rule, the coverage of the case table and the parity rule that
tests/test_gpu_train.py holds the kernels to.  No GPU needed: nothing is launched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from hcr_genesis_lr_cl_amd import abi, train
from tests import ppo_loss_cases as pc
from tests import train_abi as ta
from tests import train_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lgtrain.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ppo_train.npz")


# ---- the structs --------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header():
    structs = [("LgTrainLayer", abi.LgTrainLayer), ("LgTrainChain", abi.LgTrainChain), ("LgTrainArgs", abi.LgTrainArgs),
               ("LgTrainPlan", abi.LgTrainPlan)]
    consts = dict(LG_TRAIN_CHAINS=abi.TRAIN_CHAINS, LG_TRAIN_ACTOR=abi.TRAIN_ACTOR, LG_TRAIN_CRITIC=abi.TRAIN_CRITIC,
                  LG_TRAIN_WG_TILE=abi.TRAIN_WG_TILE, LG_TRAIN_MIN_SLICE_ROWS=abi.TRAIN_MIN_SLICE_ROWS,
                  LG_TRAIN_TARGET_JOBS=abi.TRAIN_TARGET_JOBS, LG_TRAIN_MAX_SLICES=abi.TRAIN_MAX_SLICES,
                  LG_POLICY_MAX_LAYERS=abi.POLICY_MAX_LAYERS, LG_POLICY_MAX_WIDTH=abi.POLICY_MAX_WIDTH)
    ta.check_layout(HEADER, structs, consts)
    assert (tc.WG_TILE, tc.MIN_SLICE_ROWS, tc.TARGET_JOBS, tc.MAX_SLICES) == (abi.TRAIN_WG_TILE, abi.TRAIN_MIN_SLICE_ROWS, abi.TRAIN_TARGET_JOBS,
                                                                             abi.TRAIN_MAX_SLICES)
    assert abi.TRAIN_WG_TILE % 16 == 0 and abi.TRAIN_MIN_SLICE_ROWS % 4 == 0


def test_library_exports_the_train_entry_points():
    declared = ta.check_exports(HEADER, abi.TRAIN_EXPORTS, "lg_train", ["lg_train_pass.h"])
    assert declared == {"lg_train_plan", "lg_train_forward", "lg_train_backward"}
    from hcr_genesis_lr_cl_amd import build
    assert f"{len(build.units())} translation units" in build.__doc__
    for unit in ("lg_train.hip", "lg_train_pass.h"):                           # the pass routines live in the shared header
        source = open(os.path.join(ROOT, "hcr_genesis_lr_cl_amd", "csrc", unit)).read()
        assert "atomic" not in source.lower().replace("no atomics", "")        # determinism is the house rule
    assert "lg_train" not in open(os.path.join(ROOT, "hcr_genesis_lr_cl_amd", "csrc", "lg_policy.hip")).read()   # the layer routine is a copy


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return tc.load_fixture(FIXTURE)


def test_fixture_is_the_tiny_actor_critic(fx):
    assert fx["names"] == ["std"] + [f"{c}.{i}.{k}" for c in ("actor", "critic") for i in (0, 2, 4) for k in ("weight", "bias")]
    assert fx["actor"] == [7, 16, 8, 3] and fx["critic"] == [7, 16, 8, 1] and fx["cfg"]["steps"] == 6
    assert fx["obs"].shape == (6, 16, 7) and fx["mu"].shape == (6, 16, 3) and fx["values"].shape == (6, 16, 1)
    clip = fx["cfg"]["clip_actions"]
    for s in range(6):
        pre = tc.forward(dict(tc.fixture_step(fx, s), clip=None))["mu"]
        assert 0.1 <= (np.abs(pre) >= clip).mean() <= 0.9 and np.abs(np.abs(pre) - clip).min() >= 1e-4


def test_restatement_matches_the_reference_update(fx):
    """Per step of the reference's PPO.update(): forward, the loss head's restatement (tests/ppo_loss_cases.py) for the incoming gradients,
    the hand-written backward: outputs, loss and every parameter gradient to 1e-12."""
    cfg = fx["cfg"]
    for s in range(cfg["steps"]):
        x = tc.fixture_step(fx, s)
        fw = tc.forward(x)
        for k in ("mu", "sigma", "values"):
            assert tc.max_err(fw[k], fx[k][s]) <= 1e-12, (s, k)
        r = pc.restate(tc.fixture_loss_inputs(fx, s, fw["mu"], fw["sigma"], fw["values"]), True, False, cfg["entropy_coef"], clip=cfg["clip_param"],
                       value_loss_coef=cfg["value_loss_coef"])
        assert abs(float(r["loss"]) - fx["loss"][s]) <= 1e-12
        x.update(grad_mu=r["grad_mu"][0], grad_sigma=r["grad_sigma"][0], grad_values=r["grad_values"])
        for name, g, want in zip(fx["names"], tc.backward(x), fx["grads"][s]):
            assert g.shape == want.shape and tc.max_err(g, want) <= 1e-12, (s, name)


@pytest.mark.parametrize("case", ["tiny_b33", "tiny_b128", "deep4_b257", "one_four_b31", "k65_m17_b33", "k1_m1_b33", "tiny_noclip_b33", "go2_b31"])
def test_restatement_matches_torch_float64_autograd(case):
    x = tc.make_inputs(case)
    fw, grads, ref = tc.forward(x), tc.backward(x), tc.torch_pass(x, torch.float64)
    for k in ("mu", "sigma", "values"):
        assert tc.max_err(fw[k], ref[k]) <= 1e-12 * max(1.0, np.abs(ref[k]).max())
    for name, g, want in zip(tc.param_names(x["actor"], x["critic"]), grads, ref["grads"]):
        assert tc.max_err(g, want) <= 1e-12 * max(1.0, np.abs(want).max()), name
    sliced = tc.backward(x, slices=12)
    for g, want in zip(sliced, grads):
        assert tc.max_err(g, want) <= 1e-12 * max(1.0, np.abs(want).max())
    # the module helper computes the same pass (what the GPU file hands to FusedTrainPass)
    m = tc.Module(x, dtype=torch.float64)
    mu, sigma, values = m(torch.as_tensor(x["obs"]).double(), torch.as_tensor(x["critic_obs"]).double())
    assert tc.max_err(mu.detach().numpy(), fw["mu"]) <= 1e-12 and tc.max_err(values.detach().numpy(), fw["values"]) <= 1e-12 * max(1.0, np.abs(fw["values"]).max())


def test_elu_derivative_from_the_stored_output():
    """elu' = h + 1 with h = fl32(expm1(x)) against exp(x): at most one float32 ulp of 1 apart, over the whole range."""
    x = -np.concatenate([np.logspace(-8, 2, 4001), [0.0, 16.0, 17.0, 17.5, 18.0, 50.0, 104.0]])
    h = np.expm1(x).astype(np.float32)
    d = (h + np.float32(1.0)).astype(np.float64)
    assert np.abs(d - np.exp(x)).max() <= 2.0 ** -23
    assert (h[x < -18] == -1.0).all()                                       # where the stored output pins at -1, the derivative is 0


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
PLAN_BATCHES = (1, 4, 31, 33, 64, 65, 127, 128, 129, 130, 257, 2048, 4097, 24576)


@pytest.mark.parametrize("net", ["tiny", "go2", "deep4", "one_four", "k1_m1", "k65_m65", "k17_m4"])
def test_plan_against_the_restated_rule(net):
    actor, critic = tc.NETS[net]
    for b in PLAN_BATCHES:
        p, want = train.plan(b, actor, critic), tc.restated_plan(b, actor, critic)
        assert (p.row_tile, p.lds_bytes, p.workspace_floats, p.weight_jobs, p.std_p_off) == \
            (want["row_tile"], want["lds_bytes"], want["workspace_floats"], want["weight_jobs"], want["std_p_off"]), (net, b)
        assert (p.std_slices, p.std_slice_rows) == want["std"]
        for ci, c in enumerate((actor, critic)):
            n = len(c) - 1
            assert list(p.slices[ci])[:n] == want["slices"][ci] and list(p.slice_rows[ci])[:n] == want["slice_rows"][ci], (net, b, ci)
            assert list(p.h_off[ci])[:n] == want["h_off"][ci] and list(p.g_off[ci])[:n] == want["g_off"][ci] and list(p.p_off[ci])[:n] == want["p_off"][ci]
            assert all(v == -1 for v in list(p.h_off[ci])[n:] + list(p.g_off[ci])[n:] + list(p.p_off[ci])[n:])
            for S, per in zip(want["slices"][ci], want["slice_rows"][ci]):
                assert per % 4 == 0 and (S - 1) * per < b <= S * per and 1 <= S <= tc.MAX_SLICES and (S == 1 or per >= tc.MIN_SLICE_ROWS)


def test_plan_edges():
    go2 = train.plan(24576, *tc.NETS["go2"])
    assert go2.row_tile == 32 and go2.lds_bytes == 32 * (260 + 516) * 4 and [list(s) for s in go2.slices] == [[32, 16, 32, 32]] * 2
    assert [list(s) for s in go2.slice_rows] == [[768, 1536, 768, 768]] * 2 and (go2.std_slices, go2.std_slice_rows) == (32, 768)
    assert train.plan(127, *tc.NETS["go2"]).slices[0][1] == 1 and train.plan(128, *tc.NETS["go2"]).slices[0][1] == 2
    wide = train.plan(100, [2048, 2048, 2048, 4], [8, 1])                     # 2052 + 2052 floats a row: the 8-row tile
    assert wide.row_tile == 8 and wide.lds_bytes == 8 * 4104 * 4 and wide.slices[0][0] == 1            # 1024 tiles: one slice
    assert train.plan(100, [1000, 1200, 4], [8, 1]).row_tile == 16
    assert tc.smallest_ragged_b("tiny") == tc.smallest_ragged_b("go2") == 129


# ---- refusals of the entry points: nothing is enqueued (there is no device here) -----------------------------------------------------------
def _good_args(backward=True):
    x = tc.make_inputs("tiny_b33")
    m = tc.Module(x)
    spec = train.describe(m)
    t = lambda k: torch.as_tensor(x[k])
    keep = dict(m=m, obs=t("obs"), cobs=t("critic_obs"), mu=torch.zeros(33, 3), sigma=torch.zeros(33, 3), values=torch.zeros(33, 1),
                gm=t("grad_mu"), gs=t("grad_sigma"), gv=t("grad_values"), grads=[torch.zeros_like(p) for p in spec.parameters()])
    keep["ws"] = torch.zeros(int(train.plan(33, spec.actor.widths, spec.critic.widths).workspace_floats))
    a = train.train_args(spec, keep["obs"], keep["cobs"], keep["mu"], keep["sigma"], keep["values"], keep["ws"],
                         keep["grads"] if backward else None, keep["gm"], keep["gs"], keep["gv"])
    a._keep = keep
    return a


# (mutation, message, which entry points refuse it: p plan, f forward, b backward)
ENTRY_REFUSALS = [
    (ta.set_path(("n_rows",), 0), b"n_rows = 0 < 1", "pfb"), (ta.set_path(("n_rows",), -3), b"n_rows = -3 < 1", "pfb"),
    (ta.set_path(("chain", 0, "n_layers"), 0), b"chain[0] (actor).n_layers = 0 is outside [1, 4]", "pfb"),
    (ta.set_path(("chain", 1, "n_layers"), 5), b"chain[1] (critic).n_layers = 5 is outside [1, 4]", "pfb"),
    (ta.set_path(("chain", 0, "layer", 1, "n_in"), 32), b"chain[0] (actor).layer[1].n_in = 32, but its input has 33 columns", "pfb"),
    (ta.set_path(("chain", 1, "layer", 0, "n_out"), 16), b"chain[1] (critic).layer[1].n_in = 17, but its input has 16 columns", "pfb"),
    (ta.set_path(("chain", 0, "layer", 2, "n_out"), 0), b"chain[0] (actor).layer[2].n_out = 0 is outside [1, 2048]", "pfb"),
    (ta.set_path(("chain", 0, "layer", 0, "n_in"), 2049), b"chain[0] (actor).layer[0].n_in = 2049 is outside [1, 2048]", "pfb"),
    (ta.set_path(("chain", 0, "input"), None), b"chain[0] (actor).input is null", "fb"),
    (ta.set_path(("chain", 1, "in_stride"), 5), b"chain[1] (critic).in_stride = 5 is below its width 6", "fb"),
    (ta.set_path(("chain", 0, "layer", 1, "weight"), None), b"chain[0] (actor).layer[1].weight is null", "fb"),
    (ta.set_path(("chain", 1, "layer", 0, "bias"), None), b"chain[1] (critic).layer[0].bias is null", "fb"),
    (ta.set_path(("chain", 0, "layer", 2, "grad_weight"), None), b"chain[0] (actor).layer[2].grad_weight is null", "b"),
    (ta.set_path(("chain", 1, "layer", 1, "grad_bias"), None), b"chain[1] (critic).layer[1].grad_bias is null", "b"),
    (ta.set_path(("clip_actions",), -1.0), b"clip_actions must be >= 0 under clip_on", "fb"),
    (ta.set_path(("clip_actions",), float("nan")), b"clip_actions must be >= 0 under clip_on", "fb"),
    (ta.set_path(("std",), None), b"std is null", "fb"), (ta.set_path(("mu",), None), b"mu is null", "fb"), (ta.set_path(("sigma",), None), b"sigma is null", "fb"),
    (ta.set_path(("values",), None), b"values is null", "fb"),
    (ta.set_path(("mu_stride",), 2), b"mu_stride = 2 is below its width 3", "fb"), (ta.set_path(("sigma_stride",), 0), b"sigma_stride = 0 is below its width 3", "fb"),
    (ta.set_path(("values_stride",), 0), b"values_stride = 0 is below its width 1", "fb"),
    (ta.set_path(("grad_std",), None), b"grad_std is null", "b"), (ta.set_path(("grad_mu",), None), b"grad_mu is null", "b"),
    (ta.set_path(("grad_sigma",), None), b"grad_sigma is null", "b"), (ta.set_path(("grad_values",), None), b"grad_values is null", "b"),
    (ta.set_path(("grad_mu_stride",), 2), b"grad_mu_stride = 2 is below its width 3", "b"),
    (ta.set_path(("grad_sigma_stride",), 1), b"grad_sigma_stride = 1 is below its width 3", "b"),
    (ta.set_path(("grad_values_stride",), 0), b"grad_values_stride = 0 is below its width 1", "b"),
    (ta.set_path(("workspace",), None), b"workspace is null", "fb"),
    (ta.set_path(("workspace_capacity",), 10), b"workspace_capacity = 10 floats is below the plan's", "fb"),
]


@pytest.mark.parametrize("i", range(len(ENTRY_REFUSALS)))
def test_entry_points_refuse(i):
    ta.refuse(ENTRY_REFUSALS, i, _good_args, "lg_train", abi.LgTrainPlan)


def test_entry_points_refuse_null_descriptors_and_the_lds():
    lib = abi.load_lib()
    assert lib.lg_train_plan(None, C.byref(abi.LgTrainPlan())) != 0 and b"lg_train_plan: null descriptor" in lib.lg_last_error()
    assert lib.lg_train_plan(C.byref(_good_args()), None) != 0 and b"lg_train_plan: null plan" in lib.lg_last_error()
    assert lib.lg_train_forward(None, None) != 0 and b"lg_train_forward: null descriptor" in lib.lg_last_error()
    assert lib.lg_train_backward(None, None) != 0 and b"lg_train_backward: null descriptor" in lib.lg_last_error()
    # widths within the limit never exceed the LDS (two rows of 2052 floats, 8 of them: 131 KB), so the refusal is unreachable through
    # the limits; it is pinned where it would start
    assert 8 * 2 * tc.lds_stride(abi.POLICY_MAX_WIDTH) * 4 <= tc.LDS_BYTES < 16 * 2 * tc.lds_stride(abi.POLICY_MAX_WIDTH) * 4
    assert "does not fit the 160 KB of LDS" in open(os.path.join(ROOT, "hcr_genesis_lr_cl_amd", "csrc", "lg_train_pass.h")).read()
    with pytest.raises(RuntimeError, match=r"lg_train_plan: chain\[0\] \(actor\)\.n_layers = 5"):
        train.plan(4, [3] * 6, [3, 1])
    # a forward-only descriptor (no gradient members) is what forward takes and backward refuses
    a = _good_args(backward=False)
    assert lib.lg_train_backward(C.byref(a), None) != 0 and b"grad_weight is null" in lib.lg_last_error()


# ---- refusals of the Python surface -------------------------------------------------------------------------------------------------------
class _AC(nn.Module):
    def __init__(self, actor=None, critic=None, A=3):
        super().__init__()
        self.actor = actor if actor is not None else nn.Sequential(nn.Linear(5, 8), nn.ELU(), nn.Linear(8, A), nn.Hardtanh(-1.0, 1.0))
        self.critic = critic if critic is not None else nn.Sequential(nn.Linear(6, 8), nn.ELU(), nn.Linear(8, 1))
        self.std = nn.Parameter(torch.ones(A))


def test_describe_takes_the_plain_actor_critic():
    spec = train.describe(_AC())
    assert spec.actor.widths == [5, 8, 3] and spec.critic.widths == [6, 8, 1] and spec.actor.elu == [True, False] and spec.clip_actions == 1.0
    assert spec.parameter_names() == ["std", "actor.0.weight", "actor.0.bias", "actor.1.weight", "actor.1.bias", "critic.0.weight", "critic.0.bias",
                                      "critic.1.weight", "critic.1.bias"]
    go2 = tc.Module(dict(actor=tc.NETS["go2"][0], critic=tc.NETS["go2"][1], clip=100.0, params=[]))
    assert len(train.describe(go2).parameters()) == 17 == len(list(go2.parameters()))


def _break(f):
    m = _AC()
    f(m)
    return m


SURFACE_REFUSALS = [
    (lambda: _break(lambda m: setattr(m.actor[0], "weight", nn.Parameter(torch.zeros(8, 5, dtype=torch.float64)))),
     r"actor\[0\]\.weight is torch\.float64, the kernel reads float32"),
    (lambda: _break(lambda m: setattr(m.critic[2], "weight", nn.Parameter(torch.zeros(1, 16)[:, ::2]))), r"critic\[2\]\.weight is not contiguous"),
    (lambda: _break(lambda m: setattr(m, "std", nn.Parameter(torch.ones(3, dtype=torch.float16)))), r"std is torch\.float16"),
    (lambda: _AC(actor=nn.Sequential(nn.Linear(5, 8), nn.Tanh(), nn.Linear(8, 3))), r"actor\[1\] is Tanh; only Linear and ELU \(and a final Hardtanh\)"),
    (lambda: _AC(critic=nn.Sequential(nn.Linear(6, 8), nn.ReLU(), nn.Linear(8, 1))), r"critic\[1\] is ReLU; only Linear and ELU are built"),
    (lambda: _AC(actor=nn.Sequential(nn.Linear(5, 8), nn.ELU(alpha=2.0), nn.Linear(8, 3))), r"actor\[1\] is ELU\(alpha=2\.0\), only alpha = 1"),
    (lambda: _AC(critic=nn.Sequential(nn.Linear(6, 8), nn.ELU(), nn.Linear(8, 1), nn.Hardtanh(-1, 1))), r"critic\[3\] is Hardtanh"),
    (lambda: _AC(actor=nn.Sequential(nn.Linear(5, 8), nn.ELU(), nn.Linear(8, 3), nn.Hardtanh(-1.0, 2.0))), r"actor\[3\] \(Hardtanh\(-1\.0, 2\.0\)\) must be the symmetric clip"),
    (lambda: _AC(actor=nn.Sequential(nn.Linear(5, 8), nn.ELU(), nn.Linear(7, 3))), r"actor\[2\] takes 7 inputs, the layer before it gives 8"),
    (lambda: _AC(actor=nn.Sequential(nn.Linear(5, 8, bias=False), nn.ELU(), nn.Linear(8, 3))), r"actor\[0\] has no bias"),
    (lambda: _AC(actor=nn.Sequential(*[nn.Linear(5, 5) for _ in range(5)], nn.Linear(5, 3))), r"actor has 6 Linear layers, the kernel takes 4"),
    (lambda: _AC(actor=nn.Sequential(nn.Linear(5, 3), nn.ELU())), r"actor ends in an ELU"),
    (lambda: _AC(actor=nn.Sequential(nn.Linear(5, 4000), nn.ELU(), nn.Linear(4000, 3))), r"actor\[0\] is 5 -> 4000, widths are limited to 2048"),
    (lambda: _AC(actor=nn.LSTM(5, 3)), r"actor is LSTM, expected an nn\.Sequential"),
    (lambda: _break(lambda m: setattr(m, "std", nn.Parameter(torch.ones(4)))), r"std has shape \(4,\), the actor has 3 outputs"),
    (lambda: _break(lambda m: setattr(m, "estimator", nn.Sequential(nn.Linear(5, 2)))), r"the module has \.estimator \(ActorCriticEE\)"),
    (lambda: _break(lambda m: setattr(m, "privilege_encoder", nn.Sequential(nn.Linear(5, 2)))), r"\.privilege_encoder \(ActorCriticTS / ActorCriticCTS\)"),
    (lambda: _break(lambda m: setattr(m, "history_encoder", nn.Sequential(nn.Linear(5, 2)))), r"\.history_encoder \(ActorCriticTS / ActorCriticCTS\)"),
    (lambda: _break(lambda m: setattr(m, "vae", nn.Sequential(nn.Linear(5, 2)))), r"\.vae \(ActorCriticDreamWaQ\)"),
    (lambda: _break(lambda m: setattr(m, "memory_a", nn.LSTM(5, 2))), r"\.memory_a \(ActorCriticRecurrent\)"),
    (lambda: _break(lambda m: setattr(m, "is_recurrent", True)), r"the module is recurrent"),
    (lambda: _break(lambda m: delattr(m, "std")), r"the module has no \.std"),
]


@pytest.mark.parametrize("i", range(len(SURFACE_REFUSALS)))
def test_describe_refuses(i):
    make, msg = SURFACE_REFUSALS[i]
    with pytest.raises(ValueError, match="FusedTrainPass: .*" + msg):
        train.describe(make())


def test_the_surface_refuses_devices_and_tensors():
    with pytest.raises(ValueError, match=r"FusedTrainPass: the module is on cpu, not on a HIP device \(there is no CPU path\)"):
        train.FusedTrainPass(_AC())
    with pytest.raises(ValueError, match=r"FusedTrainPass: actor\[0\]\.weight is on cpu, not on cuda:0"):
        train.describe(_AC(), torch.device("cuda:0"))
    spec = train.describe(_AC())
    ok = dict(obs=torch.zeros(4, 5), critic_obs=torch.zeros(4, 6), mu=torch.zeros(4, 3), sigma=torch.zeros(4, 3), values=torch.zeros(4, 1))
    call = lambda **kw: train.train_args(spec, *[{**ok, **kw}[k] for k in ("obs", "critic_obs", "mu", "sigma", "values")], None)
    assert call().n_rows == 4
    for kw, msg in ((dict(obs=torch.zeros(4, 6)), r"obs must be \(4, 5\) float32 with unit inner stride; got \(4, 6\)"),
                    (dict(obs=torch.zeros(4, 5, dtype=torch.float64)), r"obs must be \(4, 5\) float32.*torch\.float64"),
                    (dict(obs=torch.zeros(5, 4).t()), r"obs must be \(4, 5\) float32 with unit inner stride.*strides \(1, 4\)"),
                    (dict(critic_obs=torch.zeros(3, 6)), r"critic_obs must be \(4, 6\)"), (dict(obs=torch.zeros(0, 5)), r"obs must be a \(B, 5\) float32 tensor with B >= 1"),
                    (dict(mu=torch.zeros(4, 2)), r"mu must be \(4, 3\)"), (dict(values=torch.zeros(4)), r"values must be \(4, 1\)")):
        with pytest.raises(ValueError, match="FusedTrainPass: " + msg):
            call(**kw)
    # strided views are addressed in place
    wide = torch.zeros(4, 16)
    a = call(obs=wide[:, 2:7], mu=wide[:, 8:11])
    assert (a.chain[0].input, a.chain[0].in_stride, a.mu, a.mu_stride) == (wide.data_ptr() + 8, 16, wide.data_ptr() + 32, 16)
    # a weight swapped for a non-contiguous one after the pass was built is refused at the call
    spec.actor.linears[0].weight = nn.Parameter(torch.zeros(5, 8).t())
    with pytest.raises(ValueError, match=r"FusedTrainPass: actor layer 0 weight is not contiguous"):
        call()


# ---- the case table -----------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_the_edges():
    nets = {c["net"] for c in tc.CASES.values()}
    assert set(tc.SWEEP) <= nets and len(tc.SWEEP) == 36 and {"tiny", "go2", "deep4", "one_four"} <= nets
    assert tc.NETS["tiny"] == ([5, 33, 7, 3], [6, 17, 1]) and tc.NETS["go2"] == ([45, 512, 256, 128, 12], [45, 512, 256, 128, 1])
    depth = {n: (len(a) - 1, len(c) - 1) for n, (a, c) in tc.NETS.items()}
    assert depth["one_four"] == (1, 4) and depth["deep4"][0] == 4 and depth["tiny"] == (3, 2)          # one layer, four, different depths in one call
    for net in ("tiny", "go2", "deep4", "one_four"):
        assert {tc.CASES[f"{net}_b{b}"]["B"] for b in tc.BATCHES} == {1, 31, 33, 257}
    plans = {name: tc.restated_plan(c["B"], *tc.NETS[c["net"]]) for name, c in tc.CASES.items()}
    S = lambda name: [s for chain in plans[name]["slices"] for s in chain]
    assert set(S("tiny_b33")) == {1} and set(S("tiny_b128")) == {2} and 128 % plans["tiny_b128"]["slice_rows"][0][0] == 0          # S = 1; S > 1 exact
    assert max(S("go2_b257")) > 1 and 257 % plans["go2_b257"]["slice_rows"][0][0] != 0                  # S > 1 with a ragged last slice
    assert all(tc.smallest_ragged_b(n) == 129 for n in tc.RAGGED_SLICE_NETS)
    assert all(c["B"] % plans[n]["row_tile"] for n, c in tc.CASES.items() if c["B"] in (1, 31, 33, 257))                  # a partial last row tile
    assert plans["go2_b257"]["row_tile"] == 32 and 33 > plans["tiny_b33"]["row_tile"] - 1
    assert any(c["B"] == 1 for c in tc.CASES.values())
    # widths 0, 1 and 15 (mod 16) as a GEMM's reduction and as its output, in the forward (in, out) and thereby in both backward GEMMs
    ins = {w % 16 for a, c in tc.NETS.values() for ch in (a, c) for w in ch[:-1]}
    outs = {w % 16 for a, c in tc.NETS.values() for ch in (a, c) for w in ch[1:]}
    hidden = {w % 16 for a, c in tc.NETS.values() for ch in (a, c) for w in ch[1:-1]}
    assert {0, 1, 15} <= ins and {0, 1, 15} <= outs and {0, 1, 15} <= hidden
    assert all(c[-1] == 1 for _, c in tc.NETS.values()) and [1, 1, 3] == tc.NETS["k1_m1"][0]             # an out-width of 1
    assert any(c.get("clip", 0) is None for c in tc.CASES.values())                                     # an actor without a Hardtanh
    for name in ("tiny_b33", "go2_b257", "deep4_b31", "k65_m17_b33"):
        x = tc.make_inputs(name)
        pre = tc.forward(dict(x, clip=None))["mu"]
        assert 0.1 <= (np.abs(pre) >= x["clip"]).mean() <= 0.9 and np.abs(np.abs(pre) - x["clip"]).min() >= 1e-3
        hs = np.concatenate([h.reshape(-1) for acts in tc.forward(x)["acts"] for h in acts[1:-1]])
        assert 0.2 <= (hs <= 0).mean() <= 0.8                                                           # both branches of elu'


# ---- the parity rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiny_b257", "deep4_b257"])
def test_parity_rule_passes_float32_and_catches_wrong_backwards(case):
    """A float32 numpy evaluation of the restatement passes the rule; a dropped last slice, a dropped Hardtanh mask and elu' = 1 each miss
    the bound by more than a factor 10 on some tensor."""
    x = tc.make_inputs(case)
    r64 = tc.named(x, tc.forward(x), tc.backward(x))
    t32 = tc.torch_pass(x)
    r32 = tc.named(x, t32, t32["grads"])
    per = tc.restated_plan(257, x["actor"], x["critic"])["slice_rows"][0][0]
    assert per < 257
    tc.check_parity(tc.named(x, tc.forward(x, np.float32), tc.backward(x, np.float32, slices=per)), r64, r32, case + " numpy f32")
    for wrong in ("drop_last_slice", "no_mask", "elu1"):
        bad = tc.named(x, tc.forward(x), tc.backward(x, wrong=wrong, slices=per))
        worst = max(tc.max_err(bad[k], r64[k]) / tc.parity_bound(tc.max_err(r32[k], r64[k]), r64[k]) for k in r64)
        assert worst > 10.0, (wrong, worst)
        with pytest.raises(AssertionError):
            tc.check_parity(bad, r64, r32, f"{case} {wrong}")


def test_sigma_path_convention_in_numpy():
    """Autograd sends grad_sigma * 0 into mu: NaN for a non-finite grad_sigma.  The restatement (and the kernel) take that path as zero."""
    x = tc.make_inputs("tiny_b33")
    x["grad_sigma"] = x["grad_sigma"].copy()
    x["grad_sigma"][4, 1] = np.inf
    ours, theirs = tc.backward(x), tc.torch_pass(x, torch.float64)["grads"]
    names = tc.param_names(x["actor"], x["critic"])
    assert np.isinf(ours[0][1]) and all(np.isfinite(g).all() for g in ours[1:])
    assert any(np.isnan(g).any() for n, g in zip(names, theirs) if n.startswith("actor"))
    assert all(np.isfinite(g).all() for n, g in zip(names, theirs) if n.startswith("critic"))

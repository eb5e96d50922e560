"""Host side of the TCN history-encoder pass (hcr_genesis_lr_cl_amd/train.py's FusedTrainPassTSTcn, include/lgtraintcn.h): the ctypes
mirror against the header, the exports and the translation unit, lg_train_tcn_plan against the restated rules at every case, the float64
restatement of tests/train_tcn_cases.py against torch float64 autograd on nn.Conv1d and against the golden fixture of the reference's own
PPO_TS.update() on a TCN module (tests/golden/ppo_ts_tcn_train.npz), every refusal of nets.describe_tcn, train.describe_ts_tcn,
train.tcn_args and the entry points, the unchanged refusals of the other surfaces on the same module, policy.describe(m, student=False),
the float32 twin in the kernels' order of sums under half the parity rule, and nine planted defects that the rule must catch.  No GPU
needed: nothing is launched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from hcr_genesis_lr_cl_amd import abi, nets, policy, train
from tests import optim_cases as oc
from tests import ppo_loss_cases as pc
from tests import train_abi as ta
from tests import train_support as sup
from tests import train_tcn_cases as nc
from tests import train_ts_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lgtraintcn.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ppo_ts_tcn_train.npz")
CSRC = os.path.join(ROOT, "hcr_genesis_lr_cl_amd", "csrc")
OWNER = "FusedTrainPassTSTcn"


# ---- the structs, the exports, the unit -------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header():
    structs = [("LgTrainConv", abi.LgTrainConv), ("LgTrainTcnArgs", abi.LgTrainTcnArgs), ("LgTrainTcnPlan", abi.LgTrainTcnPlan),
               ("LgTrainChain", abi.LgTrainChain)]
    consts = dict(LG_TRAIN_TCN_MAX_CONV=abi.TRAIN_TCN_MAX_CONV, LG_TRAIN_TCN_MAX_CHANNELS=abi.TRAIN_TCN_MAX_CHANNELS,
                  LG_TRAIN_TCN_MAX_KERNEL=abi.TRAIN_TCN_MAX_KERNEL, LG_TRAIN_TCN_MAX_STRIDE=abi.TRAIN_TCN_MAX_STRIDE,
                  LG_TRAIN_TCN_MAX_DILATION=abi.TRAIN_TCN_MAX_DILATION, LG_TRAIN_TCN_TARGET_JOBS=abi.TRAIN_TCN_TARGET_JOBS,
                  LG_TRAIN_TCN_THREADS=abi.TRAIN_TCN_THREADS, LG_TRAIN_TCN_WG_ELEMS=abi.TRAIN_TCN_WG_ELEMS,
                  LG_TRAIN_TCN_MAX_BLOCKS=abi.TRAIN_TCN_MAX_BLOCKS, LG_POLICY_MAX_LAYERS=abi.POLICY_MAX_LAYERS, LG_POLICY_MAX_WIDTH=abi.POLICY_MAX_WIDTH)
    ta.check_layout(HEADER, structs, consts)
    assert (nc.MAX_CONV, nc.MAX_CHANNELS, nc.MAX_KERNEL, nc.MAX_STRIDE, nc.MAX_DILATION, nc.MAX_WIDTH) == (
        abi.TRAIN_TCN_MAX_CONV, abi.TRAIN_TCN_MAX_CHANNELS, abi.TRAIN_TCN_MAX_KERNEL, abi.TRAIN_TCN_MAX_STRIDE, abi.TRAIN_TCN_MAX_DILATION, abi.POLICY_MAX_WIDTH)
    assert (nc.TARGET_JOBS, nc.WG_ELEMS, nc.MAX_BLOCKS, nc.RED_BYTES) == (abi.TRAIN_TCN_TARGET_JOBS, abi.TRAIN_TCN_WG_ELEMS, abi.TRAIN_TCN_MAX_BLOCKS,
                                                                         abi.TRAIN_TCN_THREADS * 8)
    assert nc.LANES * abi.TRAIN_TCN_WG_ELEMS == abi.TRAIN_TCN_THREADS


def test_library_exports_the_entry_points():
    declared = ta.check_exports(HEADER, abi.TRAIN_TCN_EXPORTS, "lg_train_tcn", ["lg_train_tiles.h", "lg_train_pass.h"])
    assert declared == {"lg_train_tcn_plan", "lg_train_tcn_forward", "lg_train_tcn_backward"}
    from hcr_genesis_lr_cl_amd import build
    assert f"{len(build.units())} translation units" in build.__doc__
    assert "TRAIN_TCN_EXPORTS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "train_tcn" in open(os.path.join(ROOT, "tools", "register_table.py")).read()
    src = open(os.path.join(CSRC, "lg_train_tcn.hip")).read()
    assert '#include "lg_train_pass.h"' in src and "atomic" not in src.lower()                  # determinism is the house rule
    # the header states the slice rule, the limits and that the module's default does not fit
    head = open(HEADER).read()
    for text in ("want = min(max(1, n_rows / 64), max(1, 2048 / tiles), 32)", "30 * 113 = 3390", "STORES every x_l"):
        assert text in head, text


# ---- the case table ---------------------------------------------------------------------------------------------------------------------------
def test_case_table_reaches_the_edges():
    assert len(nc.ALL) == 18 and set(nc.CASES) == set(nc.LENGTHS)
    for name, c in nc.CASES.items():
        assert nc.lengths(c["H"], c["convs"]) == nc.LENGTHS[name], name
        assert c["tail"][0] == c["convs"][-1][1] * nc.LENGTHS[name][-1], name
        h = torch.zeros(1, 1, c["H"])
        for ci, co, k, s, p, d in c["convs"]:                                                     # the lengths are torch's
            h = nn.Conv1d(ci, co, k, stride=s, padding=p, dilation=d)(h)
        assert h.shape[2] == nc.LENGTHS[name][-1], name
    assert nc.CASES["tiny"]["convs"][0][2] > nc.CASES["tiny"]["H"] // 2                           # a window wider than half the row
    assert nc.LENGTHS["ref90"][3:] == [45, 23] and nc.CASES["ref90"]["convs"] == nc.GO2_TS["convs"] == nc.CASES["go2_ts"]["convs"]
    p = lambda b: nc.restated_plan(b, nc.CASES["go2_ts"]["H"], nc.CASES["go2_ts"]["convs"], nc.CASES["go2_ts"]["tail"], nc.priv_widths("go2_ts"))
    ragged = next(b for b in range(1, 4096) if any(S > 1 and b % per for S, per in zip(p(b)["conv_slices"], p(b)["conv_slice_rows"])))
    assert ragged == 129 == nc.CASES["go2_ts"]["B"][0]                                           # the smallest raggedly sliced batch
    assert all(c[0] == 32 or c[1] == 32 for c in nc.CASES["wide"]["convs"]) and nc.CASES["wide"]["convs"][1][:2] == (32, 32)
    odd = nc.CASES["odd37"]["convs"]
    assert odd[0][2] == 1 and odd[1][3] == 3 and (37 - 4 * 2 - 1) % 3 != 0 and odd[1][4:] == (0, 4) and odd[2][2] % 2 == 0
    assert nc.LENGTHS["odd37"][3] > nc.LENGTHS["odd37"][2] and len({c[1] for c in odd}) == 4
    x = nc.make_inputs("skip", 3)                                                                 # positions no output reads: exactly 0
    G1 = nc.enc_pass(x)["G"][1]
    assert (G1[:, :, 1::2] == 0).all() and np.abs(G1[x["terminated"][:, 0] == 1][:, :, 0::2]).min() > 0
    six = nc.CASES["six"]["convs"]
    assert len(six) == nc.MAX_CONV and six[4][4:] == (8, 4) and nc.LENGTHS["six"][4] == 16
    assert nc.LENGTHS["one"] == [5, 1] and nc.CASES["fmax"]["tail"][0] == nc.MAX_WIDTH
    for name, b in nc.ALL:
        t = nc.make_inputs(name, b)["terminated"]
        assert b == 1 or 0 < t.sum() < t.size, (name, b)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------
def _check_plan(p, w, n, nt):
    for k in ("flat", "conv_jobs", "conv_block_rows", "conv_blocks", "row_tile", "lds_bytes", "weight_jobs", "gl_off", "y_off", "partial_off", "loss_tiles",
              "workspace_floats"):
        assert getattr(p, k) == w[k], k
    for k in ("length", "x_off", "cg_off"):
        assert list(getattr(p, k))[:n + 1] == w[k], k
    for k in ("conv_p_off", "conv_slices", "conv_slice_rows", "conv_job0"):
        assert list(getattr(p, k))[:n] == w[k], k
    for k in ("h_off", "g_off", "p_off", "slices", "slice_rows"):
        assert list(getattr(p, k))[:nt] == w[k], k
    assert p.n_conv == n and p.partial_off % 2 == 0
    assert all(v == -1 for k in ("x_off", "cg_off") for v in list(getattr(p, k))[n + 1:]) and all(v == -1 for v in list(p.conv_p_off)[n:])
    assert all(v == -1 for k in ("h_off", "g_off", "p_off") for v in list(getattr(p, k))[nt:]) and p.h_off[nt - 1] == -1


@pytest.mark.parametrize("name", list(nc.CASES))
def test_plan_against_the_restated_rules(name):
    c = nc.CASES[name]
    for b in tuple(c["B"]) + (64, 129, 4097, 24576):
        p = train.plan_tcn(b, c["H"], c["convs"], c["tail"], nc.priv_widths(name))
        _check_plan(p, nc.restated_plan(b, c["H"], c["convs"], c["tail"], nc.priv_widths(name)), len(c["convs"]), len(c["tail"]) - 1)


def test_plan_edges():
    g = nc.GO2_TS
    p = train.plan_tcn(24576, g["H"], g["convs"], g["tail"], [94, 256, 128, 94])
    assert list(p.length)[:5] == [900, 900, 450, 450, 225] and p.flat == 225 and (p.conv_block_rows, p.conv_blocks) == (12, 2048)
    assert list(p.conv_slices)[:4] == [32] * 4 and list(p.conv_slice_rows)[:4] == [768] * 4 and p.conv_jobs == 4 * 32 and p.row_tile == 32
    assert 435 * 2 ** 20 < p.workspace_floats * 4 < 436 * 2 ** 20                                 # 435 MiB at go2_ts, 380 of them x_l and G_l
    w = nc.CASES["wide"]
    q = train.plan_tcn(17, w["H"], w["convs"], w["tail"], nc.priv_widths("wide"))
    assert q.conv_jobs == -(-(32 * 3 + 32) // 8) + -(-(32 * 32 * 3 + 32) // 8) and list(q.conv_slices)[:2] == [1, 1]
    f = nc.CASES["fmax"]
    assert train.plan_tcn(9, f["H"], f["convs"], f["tail"], nc.priv_widths("fmax")).row_tile == 16        # F at the limit, a narrow second buffer


# ---- the restatement against torch and the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,b", nc.ALL, ids=nc.IDS)
def test_restatement_matches_torch_float64_autograd(name, b):
    x = nc.make_inputs(name, b)
    e, t = nc.enc_pass(x), nc.torch_pass(x, torch.float64)
    rel = lambda a, c: sup.max_err(a, c) <= 1e-12 * max(1.0, np.abs(c).max())
    assert rel(e["loss"], t["loss"]) and rel(e["f"], t["f"])
    for n, g, want in zip(nc.enc_names(x["convs"], x["tail"]), e["grads"], t["grads"]):
        assert g.shape == want.shape and rel(g, want), n
    k = nc.enc_pass(x, kernel_order=True)                             # the kernels' order of sums changes no float64 digit that matters
    assert rel(k["loss"], e["loss"]) and all(rel(a, c) for a, c in zip(k["grads"], e["grads"]))
    twice = nc.enc_pass(x, upstream=2.0 * float(x["upstream"]))      # the upstream scalar scales the gradients, not the loss
    assert twice["loss"] == e["loss"] and all(rel(a, 2.0 * c) for a, c in zip(twice["grads"], e["grads"]))
    m = nc.Module(x, dtype=torch.float64)                             # what the GPU file hands to FusedTrainPassTSTcn
    d = lambda key: torch.as_tensor(x[key]).double()
    assert rel(m.encoder_loss(d("obs_history"), d("privileged_obs"), d("terminated")).detach().numpy(), e["loss"])


@pytest.fixture(scope="module")
def fx():
    return nc.load_fixture(FIXTURE)


def test_fixture_is_the_tiny_tcn_module(fx):
    net = nc.FIXTURE_NET
    assert fx["conv_shapes"] == [(co, ci, k) for ci, co, k, *_ in net["convs"]] and fx["tail"] == net["tail"] == [21, 4, 3]
    assert (fx["priv"], fx["actor"], fx["critic"]) == (net["priv"], net["actor"], net["critic"])
    assert nc.lengths(net["H"], net["convs"]) == [14, 14, 7] and fx["enc_names"] == nc.enc_names(net["convs"], net["tail"])
    assert fx["cfg"]["steps"] == 6 and fx["cfg"]["enc_steps"] == 12 and fx["cfg"]["enc_epochs"] == 2 and fx["enc_history"].shape == (12, 16, 14)
    assert os.path.getsize(FIXTURE) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "ppo_dwaq_train.npz"))
    for t in fx["enc_terminated"]:
        assert 0 < t.sum() < t.size and set(np.unique(t)) <= {0.0, 1.0}
    d, m = fx["cfg"]["desired_kl"], fx["cfg"]["max_grad_norm"]
    assert all(abs(k / (2 * d) - 1) > 0.01 and abs(k / (d / 2) - 1) > 0.01 for k in fx["kl"])
    assert all(abs(n / m - 1) > 0.01 for n in list(fx["grad_norm"]) + list(fx["enc_grad_norm"]))
    z = np.load(FIXTURE)
    assert z["shapes"].shape[1] == 3 and all(z[k].dtype.kind in "fiU" for k in z.files)           # arrays only


def test_restatement_matches_the_reference_update(fx):
    """Every one of the 6 RL steps and 12 encoder steps of the reference's PPO_TS.update() on the TCN module: the RL pass restated by
    tests/train_ts_cases.py (it has no history chain), the loss head's restatement, the TCN encoder pass restated here and the restated
    optimizer reproduce outputs, losses, gradients, norms, rates and every parameter to 1e-12."""
    cfg = fx["cfg"]
    params = {k: v.copy() for k, v in fx["init"].items()}
    state, lr = {}, cfg["lr0"]
    for s in range(cfg["steps"]):
        x = nc.fixture_inputs(fx, params, rl_step=s)
        fw = sc.rl_forward(x)
        for k in ("mu", "sigma", "values"):
            assert sup.max_err(fw[k], fx[k][s]) <= 1e-12, (s, k)
        r = pc.restate(sup.fixture_loss_inputs(fx, s, fw["mu"], fw["sigma"], fw["values"]), True, False, cfg["entropy_coef"], clip=cfg["clip_param"],
                       value_loss_coef=cfg["value_loss_coef"])
        assert abs(float(r["loss"]) - fx["loss"][s]) <= 1e-12 and abs(float(r["kl"][0]) - fx["kl"][s]) <= 1e-12
        x.update(grad_mu=r["grad_mu"][0], grad_sigma=r["grad_sigma"][0], grad_values=r["grad_values"])
        grads = sc.rl_backward(x)
        for name, g, want in zip(fx["rl_names"], grads, fx["grads"][s]):
            assert g.shape == want.shape and sup.max_err(g, want) <= 1e-12, (s, name)
        step = ta.adam(x["rl_params"], grads, state, lr, cfg, kl=float(r["kl"][0]))
        lr = step["lr"]
        assert lr == fx["lr"][s] and abs(step["grad_norm"] - fx["grad_norm"][s]) <= 1e-12
        params.update(zip(fx["rl_names"], step["params"]))
        for n in fx["names"]:
            assert sup.max_err(params[n], fx["params"][s][n]) <= 1e-12, (s, n)
    state = {}
    for s in range(cfg["enc_steps"]):
        x = nc.fixture_inputs(fx, params, enc_step=s)
        e = nc.enc_pass(x)
        assert abs(float(e["loss"]) - fx["enc_loss"][s]) <= 1e-12
        for name, g, want in zip(fx["enc_names"], e["grads"], fx["enc_grads"][s]):
            assert g.shape == want.shape and sup.max_err(g, want) <= 1e-12, (s, name)
        step = ta.adam(x["enc_params"], e["grads"], state, cfg["encoder_lr"], cfg)
        assert abs(step["grad_norm"] - fx["enc_grad_norm"][s]) <= 1e-12
        params.update(zip(fx["enc_names"], step["params"]))
        for n in fx["names"]:
            assert sup.max_err(params[n], fx["enc_params"][s][n]) <= 1e-12, (s, n)


# ---- the float32 twin and the planted defects -------------------------------------------------------------------------------------------------
REFS = {}


def refs(name, b):
    """(inputs, float64 restatement, torch CPU float32) of a case: computed once, shared, left unchanged."""
    if (name, b) not in REFS:
        x = nc.make_inputs(name, b)
        REFS[name, b] = (x,) + nc.references(x)
    return REFS[name, b]


@pytest.mark.parametrize("name,b", nc.ALL, ids=nc.IDS)
def test_float32_twin_in_the_kernels_order_keeps_half_the_rule(name, b):
    x, r64, r32 = refs(name, b)
    nc.check_parity(nc.named(x, nc.enc_pass(x, np.float32, kernel_order=True)), r64, r32, f"numpy f32 {name}_b{b}", factor=oc.PARITY_FACTOR / 2)


# defect -> the cases at which it must show; "drop_last" shows only where (L_in + 2 p - d (k - 1) - 1) % s == 0 under a stride above 1
DEFECTS = {
    "pad_edge": [("tiny", 33), ("six", 33)], "no_dilation": [("ref90", 31), ("odd37", 9)], "no_stride": [("tiny", 33), ("ref90", 31)],
    "drop_last": [("ref90", 31), ("skip", 3)], "flatten": [("tiny", 33), ("wide", 17)], "bias_no_t": [("tiny", 33), ("go2_ts", 129)],
    "garbage": [("skip", 3)], "tail0_elu": [("tiny", 33), ("ref90", 257)], "upstream_twice": [("tiny", 5), ("one", 4)],
}


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_parity_rule_catches_the_planted_defects(defect):
    """Each defect, planted in the float32 twin, fails check_parity at its cases; the factor by which it misses the rule is printed."""
    for name, b in DEFECTS[defect]:
        x, r64, r32 = refs(name, b)
        wrong = nc.named(x, nc.enc_pass(x, np.float32, kernel_order=True, wrong=defect))
        worst = 0.0
        for k in r64:
            unit = oc.parity_bound(sup.max_err(r32[k], r64[k]), r64[k])
            worst = max(worst, sup.max_err(wrong[k], r64[k]) / unit)
        print(f"defect {defect} at {name}_b{b}: misses the rule by a factor {worst:.3g}")
        assert worst > 1.0
        with pytest.raises(AssertionError):
            nc.check_parity(wrong, r64, r32, f"{defect} {name}_b{b}")
    if defect == "garbage":                                           # the planted value reaches layer 0's weight gradient
        x, r64, _ = refs("skip", 3)
        wrong = nc.named(x, nc.enc_pass(x, np.float32, wrong=defect))
        assert sup.max_err(wrong["history_encoder.0.weight"], r64["history_encoder.0.weight"]) > 0.1


# ---- refusals of the entry points: nothing is enqueued (there is no device here) --------------------------------------------------------------
class _TS(nn.Module):
    """O = 4, P = 5, Z = 2, H = 6: the module of tests/test_train_ts_host.py's refusal tests, its history encoder the TCN they build."""

    def __init__(self, history_encoder=None, privilege_encoder=None, actor=None):
        super().__init__()
        self.actor = actor if actor is not None else nn.Sequential(nn.Linear(6, 8), nn.ELU(), nn.Linear(8, 3))
        self.critic = nn.Sequential(nn.Linear(6, 8), nn.ELU(), nn.Linear(8, 1))
        self.privilege_encoder = privilege_encoder if privilege_encoder is not None else nn.Sequential(nn.Linear(5, 4), nn.ELU(), nn.Linear(4, 2))
        self.history_encoder = history_encoder if history_encoder is not None else _tcn()
        self.std = nn.Parameter(torch.ones(3))


def _tcn(*convs, tail=None):
    convs = convs or (nn.Conv1d(1, 3, 5, padding=2), nn.Conv1d(3, 3, 5, stride=2, padding=2))
    return nn.Sequential(*convs, nn.Flatten(), *(tail or (nn.Linear(9, 4), nn.ELU(), nn.Linear(4, 2))))


def _good(backward=True):
    m = _TS()
    spec = train.describe_ts_tcn(m, None, 6)
    keep = dict(m=m, h=torch.zeros(33, 6), p=torch.zeros(33, 5), t=torch.ones(33, 1), loss=torch.zeros(()), up=torch.ones(1),
                grads=[torch.zeros_like(p) for p in spec.encoder_parameters()])
    keep["ws"] = torch.zeros(int(train.plan_tcn(33, 6, spec.history_encoder.shapes, spec.history_encoder.tail.widths, [5, 4, 2]).workspace_floats))
    a = train.tcn_args(spec, keep["h"], keep["p"], keep["t"], keep["loss"], keep["ws"], keep["grads"] if backward else None, keep["up"])
    a._keep = keep
    return a


REFUSALS = [
    (ta.set_path(("n_rows",), 0), b"n_rows = 0 < 1", "pfb"),
    (ta.set_path(("n_conv",), 0), b"n_conv = 0 is outside [1, 6]", "pfb"), (ta.set_path(("n_conv",), 7), b"n_conv = 7 is outside [1, 6]", "pfb"),
    (ta.set_path(("n_history",), 0), b"n_history = 0 is outside [1, 2048]", "pfb"), (ta.set_path(("n_history",), 2049), b"n_history = 2049 is outside [1, 2048]", "pfb"),
    (ta.set_path(("conv", 0, "c_in"), 2), b"conv[0].c_in = 2, but its input has 1 channel: obs_history is (1, H)", "pfb"),
    (ta.set_path(("conv", 1, "c_in"), 2), b"conv[1].c_in = 2, but its input has 3 channels", "pfb"),
    (ta.set_path(("conv", 0, "c_in"), 0), b"conv[0].c_in = 0 is outside [1, 32]", "pfb"),
    (ta.set_path(("conv", 1, "c_out"), 33), b"conv[1].c_out = 33 is outside [1, 32]", "pfb"),
    (ta.set_path(("conv", 0, "kernel"), 10), b"conv[0].kernel = 10 is outside [1, 9]", "pfb"), (ta.set_path(("conv", 1, "kernel"), 0), b"conv[1].kernel = 0 is outside [1, 9]", "pfb"),
    (ta.set_path(("conv", 1, "stride"), 5), b"conv[1].stride = 5 is outside [1, 4]", "pfb"), (ta.set_path(("conv", 0, "stride"), 0), b"conv[0].stride = 0 is outside [1, 4]", "pfb"),
    (ta.set_path(("conv", 0, "dilation"), 9), b"conv[0].dilation = 9 is outside [1, 8]", "pfb"),
    (ta.set_path(("conv", 0, "padding"), 5), b"conv[0].padding = 5 is outside [0, 4]", "pfb"), (ta.set_path(("conv", 1, "padding"), -1), b"conv[1].padding = -1 is outside [0, 4]", "pfb"),
    (lambda a: (setattr(a.conv[0], "padding", 0), setattr(a.conv[0], "dilation", 2)), b"conv[0]: its input of length 6 is shorter than the window: the output length is below 1", "pfb"),
    (ta.set_path(("conv", 1, "stride"), 1), b"tail.layer[0].n_in = 9, but the flattened conv output has 3 * 6 = 18 columns", "pfb"),
    (ta.set_path(("tail", "n_layers"), 5), b"tail.n_layers = 5 is outside [1, 4]", "pfb"),
    (ta.set_path(("tail", "layer", 1, "n_in"), 5), b"tail.layer[1].n_in = 5, but its input has 4 columns", "pfb"),
    (ta.set_path(("privilege", "n_layers"), 0), b"privilege.n_layers = 0 is outside [1, 4]", "pfb"),
    (ta.set_path(("privilege", "layer", 1, "n_out"), 3), b"privilege.layer[1].n_out = 3, but the history encoder ends at 2 columns: the two encoders' output widths differ", "pfb"),
    (ta.set_path(("history",), None), b"history is null", "fb"), (ta.set_path(("history_stride",), 5), b"history_stride = 5 is below its width 6", "fb"),
    (ta.set_path(("conv", 0, "weight"), None), b"conv[0].weight is null", "fb"), (ta.set_path(("conv", 1, "bias"), None), b"conv[1].bias is null", "fb"),
    (ta.set_path(("conv", 1, "grad_weight"), None), b"conv[1].grad_weight is null", "b"), (ta.set_path(("conv", 0, "grad_bias"), None), b"conv[0].grad_bias is null", "b"),
    (ta.set_path(("tail", "layer", 0, "weight"), None), b"tail.layer[0].weight is null", "fb"),
    (ta.set_path(("tail", "layer", 1, "grad_bias"), None), b"tail.layer[1].grad_bias is null", "b"),
    (ta.set_path(("privilege", "input"), None), b"privilege.input is null", "fb"), (ta.set_path(("privilege", "in_stride"), 4), b"privilege.in_stride = 4 is below its width 5", "fb"),
    (ta.set_path(("privilege", "layer", 0, "bias"), None), b"privilege.layer[0].bias is null", "fb"),
    (ta.set_path(("mask",), None), b"mask is null", "fb"), (ta.set_path(("mask_stride",), 0), b"mask_stride = 0 is below its width 1", "fb"),
    (ta.set_path(("loss",), None), b"loss is null", "f"), (ta.set_path(("upstream",), None), b"upstream is null", "b"),
    (ta.set_path(("workspace",), None), b"workspace is null", "fb"),
    (lambda a: setattr(a, "workspace", a.workspace + 4), b"workspace is not 8-byte aligned", "fb"),
    (ta.set_path(("workspace_capacity",), 10), b"workspace_capacity = 10 floats is below the plan's", "fb"),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_entry_points_refuse(i):
    ta.refuse(REFUSALS, i, _good, "lg_train_tcn", abi.LgTrainTcnPlan)


def test_entry_points_refuse_null_descriptors_the_default_module_and_f_above_the_limit():
    lib = abi.load_lib()
    plan = lib.lg_train_tcn_plan
    assert plan(None, C.byref(abi.LgTrainTcnPlan())) != 0 and b"lg_train_tcn_plan: null descriptor" in lib.lg_last_error()
    assert plan(C.byref(_good()), None) != 0 and b"lg_train_tcn_plan: null plan" in lib.lg_last_error()
    for d in ("_forward", "_backward"):
        assert getattr(lib, "lg_train_tcn" + d)(None, None) != 0 and ("lg_train_tcn" + d + ": null descriptor").encode() in lib.lg_last_error()
    assert lib.lg_train_tcn_backward(C.byref(_good(backward=False)), None) != 0               # a forward-only descriptor is what backward refuses
    a = _good()
    assert all(not a.privilege.layer[i].grad_weight and not a.privilege.layer[i].grad_bias for i in range(2))          # tcn_args does not even fill them
    # the module's own default: six layers of 30 channels on H = 900
    default = nc._pattern([30] * 6, 5, [1, 2, 1, 2, 1, 2], [1, 1, 2, 1, 4, 1])
    with pytest.raises(RuntimeError, match=r"lg_train_tcn_plan: conv\[5\] leaves F = c_out \* L = 30 \* 113 = 3390 columns behind the flatten, above 2048"):
        train.plan_tcn(64, 900, default, [3390, 128, 94], [94, 256, 128, 94])
    f = nc.CASES["fmax"]                                              # F at the limit passes; the same net on H = 257 is refused
    assert train.plan_tcn(9, 256, f["convs"], f["tail"], nc.priv_widths("fmax")).flat == 2048
    with pytest.raises(RuntimeError, match=r"conv\[0\] leaves F = c_out \* L = 8 \* 257 = 2056 columns"):
        train.plan_tcn(9, 257, f["convs"], [2056, 4, 2], nc.priv_widths("fmax"))


# ---- refusals of the Python surface -----------------------------------------------------------------------------------------------------------
def _set(conv, **kw):
    for k, v in kw.items():
        setattr(conv, k, v)
    return conv


TCN_REFUSALS = [
    (lambda: _tcn(nn.Conv1d(1, 4, 5, padding=2), nn.Conv1d(4, 4, 5, padding=2, groups=2), tail=(nn.Linear(24, 2),)), r"history_encoder\[1\]\.groups = 2, only groups = 1"),
    (lambda: _tcn(nn.Conv1d(1, 3, 5, padding=2, padding_mode="reflect"), tail=(nn.Linear(18, 2),)), r"history_encoder\[0\]\.padding_mode = 'reflect', only 'zeros'"),
    (lambda: _tcn(nn.Conv1d(1, 3, 5, padding="same"), tail=(nn.Linear(18, 2),)), r"history_encoder\[0\]\.padding = 'same', only an integer padding"),
    (lambda: _tcn(nn.Conv1d(1, 3, 5, padding=2, bias=False), tail=(nn.Linear(18, 2),)), r"history_encoder\[0\]\.bias is None"),
    (lambda: nn.Sequential(nn.Conv1d(1, 3, 5, padding=2), nn.ELU(), nn.Conv1d(3, 3, 5, padding=2), nn.Flatten(), nn.Linear(18, 2)),
     r"history_encoder\[1\] is ELU; an activation between the convolutions is not built"),
    (lambda: nn.Sequential(nn.Conv1d(1, 3, 5, padding=2), nn.Conv1d(3, 3, 5, padding=2)), r"history_encoder has no Flatten behind its Conv1d layers"),
    (lambda: nn.Sequential(nn.Conv1d(1, 3, 5, padding=2), nn.Linear(6, 2)), r"history_encoder\[1\] is Linear; expected Conv1d layers, then a Flatten"),
    (lambda: _tcn(nn.Conv1d(2, 3, 5, padding=2), tail=(nn.Linear(18, 2),)), r"history_encoder\[0\]\.in_channels = 2, obs_history is one channel"),
    (lambda: _tcn(nn.Conv1d(1, 3, 5, padding=2), nn.Conv1d(2, 3, 5, padding=2), tail=(nn.Linear(18, 2),)), r"history_encoder\[1\]\.in_channels = 2, the conv before it gives 3"),
    (lambda: _tcn(nn.Conv1d(1, 33, 5, padding=2), tail=(nn.Linear(198, 2),)), r"history_encoder\[0\]\.out_channels = 33 is outside \[1, 32\]"),
    (lambda: _tcn(nn.Conv1d(1, 3, 11, padding=5), tail=(nn.Linear(18, 2),)), r"history_encoder\[0\]\.kernel_size = 11 is outside \[1, 9\]"),
    (lambda: _tcn(nn.Conv1d(1, 3, 5, stride=5, padding=2), tail=(nn.Linear(6, 2),)), r"history_encoder\[0\]\.stride = 5 is outside \[1, 4\]"),
    (lambda: _tcn(nn.Conv1d(1, 3, 2, dilation=9, padding=2), tail=(nn.Linear(3, 2),)), r"history_encoder\[0\]\.dilation = 9 is outside \[1, 8\]"),
    (lambda: _tcn(nn.Conv1d(1, 3, 3, padding=3), tail=(nn.Linear(30, 2),)), r"history_encoder\[0\]\.padding = 3 is outside \[0, dilation \* \(kernel_size - 1\) = 2\]"),
    (lambda: _tcn(*[nn.Conv1d(1, 1, 1) for _ in range(7)], tail=(nn.Linear(6, 2),)), r"history_encoder\[6\] is Conv1d number 7, the kernel takes 6"),
    (lambda: nn.Sequential(nn.Conv1d(1, 3, 5, padding=2), nn.Flatten(0, -1), nn.Linear(18, 2)), r"history_encoder\[1\] is Flatten\(0, -1\), only Flatten\(1, -1\)"),
    (lambda: _tcn(tail=(nn.Linear(9, 4), nn.Tanh(), nn.Linear(4, 2))), r"history_encoder\[4\] is Tanh; only Linear and ELU are built"),
    (lambda: _tcn(tail=(nn.Linear(9, 4), nn.ELU(), nn.Linear(5, 2))), r"history_encoder\[5\] takes 5 inputs, the layer before it gives 4"),
    (lambda: _tcn(tail=(nn.Linear(9, 4), nn.ELU())), r"history_encoder ends in an ELU"),
    (lambda: _tcn(_set(nn.Conv1d(1, 3, 5, padding=2), weight=nn.Parameter(torch.zeros(3, 1, 5, dtype=torch.float64))), tail=(nn.Linear(18, 2),)),
     r"history_encoder\[0\]\.weight is torch\.float64"),
    (lambda: _tcn(_set(nn.Conv1d(1, 3, 5, padding=2), weight=nn.Parameter(torch.zeros(5, 1, 3).permute(2, 1, 0))), tail=(nn.Linear(18, 2),)),
     r"history_encoder\[0\]\.weight is not contiguous"),
    (lambda: _tcn(tail=(nn.Linear(10, 4), nn.ELU(), nn.Linear(4, 2))), r"history_encoder\[3\]\.in_features = 10, but the flattened conv output has 3 \* 3 = 9 columns for H = 6"),
    (lambda: _tcn(nn.Conv1d(1, 3, 9), tail=(nn.Linear(3, 2),)), r"history_encoder\[0\] has a window of dilation \* \(kernel_size - 1\) \+ 1 = 9 on a padded input of 6"),
]


@pytest.mark.parametrize("i", range(len(TCN_REFUSALS)))
def test_describe_tcn_refuses(i):
    make, msg = TCN_REFUSALS[i]
    with pytest.raises(ValueError, match=OWNER + ": " + msg):
        nets.describe_tcn("history_encoder", make(), None, OWNER, 6)
    with pytest.raises(ValueError, match=OWNER + ": " + msg):
        train.describe_ts_tcn(_TS(history_encoder=make()), None, 6)


def test_describe_tcn_takes_the_module_and_the_limits():
    spec = train.describe_ts_tcn(_TS(), None, 6)
    h = spec.history_encoder
    assert h.shapes == [(1, 3, 5, 1, 2, 1), (3, 3, 5, 2, 2, 1)] and h.lengths(6) == [6, 6, 3] and h.tail.widths == [9, 4, 2]
    m = _TS()
    assert all(a is b for a, b in zip(train.describe_ts_tcn(m).encoder_parameters(), m.history_encoder.parameters()))
    assert train.describe_ts_tcn(m).encoder_parameter_names() == [f"history_encoder.{n}" for n, _ in m.history_encoder.named_parameters()]
    want = list(m.actor.parameters()) + list(m.critic.parameters()) + list(m.privilege_encoder.parameters()) + [m.std]
    assert all(a is b for a, b in zip(train.describe_ts_tcn(m).rl_parameters(), want))
    with pytest.raises(ValueError, match=OWNER + r": obs_history has 2049 columns, the kernel takes 1 to 2048"):
        h.lengths(2049)
    with pytest.raises(ValueError, match=OWNER + r": obs_history has 0 columns"):
        h.lengths(0)
    with pytest.raises(ValueError, match=OWNER + r": history_encoder\[3\]\.in_features = 9, but the flattened conv output has 3 \* 4 = 12 columns for H = 7"):
        h.lengths(7)
    default = nn.Sequential(*[nn.Conv1d(ci, co, k, stride=s, padding=p, dilation=d) for ci, co, k, s, p, d in
                              nc._pattern([30] * 6, 5, [1, 2, 1, 2, 1, 2], [1, 1, 2, 1, 4, 1])], nn.Flatten(), nn.Linear(3390, 128), nn.ELU(), nn.Linear(128, 2))
    with pytest.raises(ValueError, match=OWNER + r": history_encoder\[5\] leaves out_channels \* L = 30 \* 113 = 3390 columns behind the Flatten for H = 900"):
        train.describe_ts_tcn(_TS(history_encoder=default), None, 900)
    with pytest.raises(ValueError, match=OWNER + r": history_encoder\[7\] is 3390 -> 128, widths are limited to 2048"):
        train.describe_ts_tcn(_TS(history_encoder=default))          # without H the tail's own width limit refuses it


def test_describe_ts_tcn_refuses_the_family_rules_and_the_mlp():
    with pytest.raises(ValueError, match=OWNER + r": history_encoder has no Conv1d layer: it is an MLP, which FusedTrainPassTS builds"):
        train.describe_ts_tcn(_TS(history_encoder=nn.Sequential(nn.Linear(6, 4), nn.ELU(), nn.Linear(4, 2))))
    with pytest.raises(ValueError, match=OWNER + r": history_encoder ends at 3 columns, privilege_encoder at 2: the latent widths differ"):
        train.describe_ts_tcn(_TS(history_encoder=_tcn(tail=(nn.Linear(9, 3),))))
    with pytest.raises(ValueError, match=OWNER + r": the module has no \.history_encoder"):
        m = _TS()
        m.history_encoder = None
        train.describe_ts_tcn(m)
    with pytest.raises(ValueError, match=OWNER + r": the module has \.estimator \(ActorCriticEE\) beside its encoders"):
        m = _TS()
        m.estimator = nn.Sequential(nn.Linear(5, 2))
        train.describe_ts_tcn(m)
    with pytest.raises(ValueError, match=OWNER + r": privilege_encoder\[1\] is Tanh"):
        train.describe_ts_tcn(_TS(privilege_encoder=nn.Sequential(nn.Linear(5, 4), nn.Tanh(), nn.Linear(4, 2))))
    with pytest.raises(ValueError, match=OWNER + r": actor\[0\] takes 2 inputs, but \[obs \| latent\] has O \+ 2 columns"):
        train.describe_ts_tcn(_TS(actor=nn.Sequential(nn.Linear(2, 8), nn.ELU(), nn.Linear(8, 3))))
    with pytest.raises(ValueError, match=OWNER + r": history_encoder is GRU, expected an nn\.Sequential of Conv1d, Flatten"):
        train.describe_ts_tcn(_TS(history_encoder=nn.GRU(6, 2)))
    with pytest.raises(ValueError, match=OWNER + r": the module is on cpu, not on a HIP device \(there is no CPU path\)"):
        train.FusedTrainPassTSTcn(_TS())
    with pytest.raises(ValueError, match=OWNER + r": privilege_encoder\[0\]\.weight is on cpu, not on cuda:0"):
        train.describe_ts_tcn(_TS(), torch.device("cuda:0"))
    assert "act_student through the TCN stays on torch" in train.FusedTrainPassTSTcn.__doc__
    assert "FusedTrainPassTSTcn" in train.FusedTrainPassTS.__doc__ and "keeps the torch path" not in train.FusedTrainPassTS.__doc__
    assert "keeps\n    the torch path" not in train.FusedTrainPassCTS.__doc__


def test_tcn_args_addresses_in_place_and_refuses():
    spec = train.describe_ts_tcn(_TS())
    ok = dict(h=torch.zeros(4, 6), p=torch.zeros(4, 5), t=torch.ones(4, 1), loss=torch.zeros(()))
    call = lambda **kw: train.tcn_args(spec, *[{**ok, **kw}[k] for k in ("h", "p", "t", "loss")], None)
    a = call()
    assert (a.n_rows, a.n_history, a.n_conv, a.mask_stride, a.history_stride) == (4, 6, 2, 1, 6)
    assert (a.conv[1].c_in, a.conv[1].c_out, a.conv[1].kernel, a.conv[1].stride, a.conv[1].padding, a.conv[1].dilation) == (3, 3, 5, 2, 2, 1)
    assert a.tail.n_layers == 2 and (a.tail.layer[0].n_in, a.tail.layer[0].elu, a.tail.layer[1].n_out) == (9, 1, 2) and not a.conv[0].grad_weight
    assert call(h=torch.zeros(4, 1, 6)).history_stride == 6                                      # (B, 1, H) as ppo_ts.py:176-178 unsqueezes it
    wide = torch.zeros(4, 16)
    b = call(h=wide[:, 2:8].unsqueeze(1), p=wide[:, 9:14], t=wide[:, 15:16])
    assert (b.history, b.history_stride, b.privilege.input, b.privilege.in_stride, b.mask, b.mask_stride) == (
        wide.data_ptr() + 8, 16, wide.data_ptr() + 36, 16, wide.data_ptr() + 60, 16)
    for kw, msg in ((dict(h=torch.zeros(4, 7)), r"history_encoder\[3\]\.in_features = 9, but the flattened conv output has 3 \* 4 = 12 columns for H = 7"),
                    (dict(h=torch.zeros(4, 2, 6)), r"obs_history must be a \(B, H\) or \(B, 1, H\) float32 tensor"),
                    (dict(h=torch.zeros(0, 6)), r"obs_history must be a \(B, H\) or \(B, 1, H\) float32 tensor with B >= 1"),
                    (dict(h=torch.zeros(4, 6, dtype=torch.float64)), r"obs_history must be \(4, 6\) float32"),
                    (dict(p=torch.zeros(4, 6)), r"privileged_obs must be \(4, 5\) float32"), (dict(t=torch.ones(4)), r"terminated must be \(4, 1\)"),
                    (dict(loss=torch.zeros(2)), r"the loss must be one float32")):
        with pytest.raises(ValueError, match=OWNER + ": " + msg):
            call(**kw)
    with pytest.raises(ValueError, match=OWNER + r": the workspace must be a contiguous float32 tensor"):
        train.tcn_args(spec, ok["h"], ok["p"], ok["t"], ok["loss"], torch.zeros(8, dtype=torch.float64))


# ---- the other surfaces on the same module: unchanged -----------------------------------------------------------------------------------------
def test_the_other_surfaces_refuse_the_module_as_before_and_student_false_takes_it():
    m = _TS()
    with pytest.raises(ValueError, match=r"FusedTrainPassTS: history_encoder\[0\] is Conv1d; only Linear and ELU are built"):
        train.describe_ts(m)
    with pytest.raises(ValueError, match=r"FusedTrainPassCTS: history_encoder\[0\] is Conv1d; only Linear and ELU are built"):
        train.describe_cts(m)
    with pytest.raises(ValueError, match=r"FusedPolicy: history_encoder\[0\] is Conv1d; only Linear and ELU are built"):
        policy.describe(m)
    with pytest.raises(ValueError, match=r"FusedPolicy: history_encoder\[0\] is Conv1d"):
        policy.describe(m, None, True)
    spec = policy.describe(m, student=False)
    assert spec.family == "ts" and spec.history_encoder is None and spec.privilege_encoder.widths == [5, 4, 2] and spec.latent_width == 2
    assert spec.chain_order == ["privilege_encoder", "actor", "critic"]
    mlp = _TS(history_encoder=nn.Sequential(nn.Linear(6, 4), nn.ELU(), nn.Linear(4, 2)))
    assert policy.describe(mlp).history_encoder.widths == [6, 4, 2] and policy.describe(mlp, student=False).history_encoder is None
    z = lambda w: torch.zeros(4, w)
    a = policy.policy_args(spec, z(4), z(6), z(3), z(3), z(3), z(1), z(1), counter=torch.zeros(1, dtype=torch.int32), privileged_obs=z(5), obs_history=z(6))
    assert a is not None                                              # the teacher's rollout descriptor builds without a history encoder
    for kw in (dict(student=True, obs_history=z(6)), dict(num_teacher=2, privileged_obs=z(5), obs_history=z(6))):
        with pytest.raises(ValueError, match=r"FusedPolicy: (the student call|num_teacher) runs the history encoder, which student=False left unread"):
            policy.policy_args(spec, z(4), z(6), z(3), z(3), z(3), z(1), z(1), counter=torch.zeros(1, dtype=torch.int32), **kw)
    assert "student=False" in policy.FusedPolicy.act_student.__doc__ and "stays on torch" in policy.FusedPolicy.act_student.__doc__

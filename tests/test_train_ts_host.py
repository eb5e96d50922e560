"""Host side of the teacher-student learner passes (hcr_genesis_lr_cl_amd/train.py's FusedTrainPassTS, include/lgtraints.h): the ctypes
mirror against the header, the exports and the translation unit, the float64 restatement of tests/train_ts_cases.py against the golden
fixture of the reference's own PPO_TS.update() (tests/golden/ppo_ts_train.npz) and against torch float64 autograd, the plans of
lg_train_ts_plan / lg_train_enc_plan against the restated rules, every refusal of the entry points and of describe_ts, the float32
restatement in the kernel's order of sums under half the parity rule, three planted defects that the rule must catch, and the coverage of
the case table.  No GPU needed: nothing is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from hcr_genesis_lr_cl_amd import abi, train
from tests import optim_cases as oc
from tests import ppo_loss_cases as pc
from tests import train_abi as ta
from tests import train_cases as tc
from tests import train_ts_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lgtraints.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ppo_ts_train.npz")
CSRC = os.path.join(ROOT, "hcr_genesis_lr_cl_amd", "csrc")
PRI, ACT, CRI, HIS = abi.TRAIN_TS_PRIVILEGE, abi.TRAIN_TS_ACTOR, abi.TRAIN_TS_CRITIC, abi.TRAIN_TS_HISTORY


# ---- the structs --------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header():
    structs = [("LgTrainTSArgs", abi.LgTrainTSArgs), ("LgTrainEncArgs", abi.LgTrainEncArgs), ("LgTrainTSPlan", abi.LgTrainTSPlan),
               ("LgTrainChain", abi.LgTrainChain)]
    consts = dict(LG_TRAIN_TS_CHAINS=abi.TRAIN_TS_CHAINS, LG_TRAIN_TS_PRIVILEGE=PRI, LG_TRAIN_TS_ACTOR=ACT, LG_TRAIN_TS_CRITIC=CRI,
                  LG_TRAIN_TS_HISTORY=HIS, LG_TRAIN_TS_RL_CHAINS=abi.TRAIN_TS_RL_CHAINS, LG_TRAIN_ENC_CHAINS=abi.TRAIN_ENC_CHAINS,
                  LG_TRAIN_ENC_HISTORY=abi.TRAIN_ENC_HISTORY, LG_TRAIN_ENC_PRIVILEGE=abi.TRAIN_ENC_PRIVILEGE, LG_TRAIN_TS_THREADS=abi.TRAIN_TS_THREADS,
                  LG_TRAIN_TS_TARGET_JOBS=abi.TRAIN_TS_TARGET_JOBS, LG_POLICY_MAX_LAYERS=abi.POLICY_MAX_LAYERS)
    ta.check_layout(HEADER, structs, consts)
    assert sc.RED_BYTES == abi.TRAIN_TS_THREADS * 8 and sc.TARGET_JOBS == abi.TRAIN_TS_TARGET_JOBS


def test_library_exports_the_entry_points():
    declared = ta.check_exports(HEADER, abi.TRAIN_TS_EXPORTS, "lg_train_ts", ["lg_train_tiles.h", "lg_train_pass.h"])
    assert declared == {"lg_train_ts_plan", "lg_train_ts_forward", "lg_train_ts_backward", "lg_train_enc_plan", "lg_train_enc_forward",
                        "lg_train_enc_backward"}
    from hcr_genesis_lr_cl_amd import build
    assert f"{len(build.units())} translation units" in build.__doc__
    assert "TRAIN_TS_EXPORTS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()          # the build's export check covers the list
    # one copy of the layer and pass routines: the unit includes the shared header (and through it the tiles) and defines none of them
    src = open(os.path.join(CSRC, "lg_train_ts.hip")).read()
    assert '#include "lg_train_tiles.h"' in open(os.path.join(CSRC, "lg_train_pass.h")).read()
    for fn in ("stage_rows", "copy_out", "fwd_tile", "bwd_tile", "wgrad_wave", "combine_layer", "lds_stride", "slice_rule", "chain_forward",
               "chain_backward", "bwd_layer", "seed_last_g", "mse_tile", "loss_finalize", "wgrad_job", "combine_all", "plan_chain", "plan_layout",
               "plan_rest", "bind_chain", "bind_heads", "check_ws", "done", "raise_lds", "launch_backward"):
        assert '#include "lg_train_pass.h"' in src and not re.findall(r"\b(?:void|int|lds_f \*) ?" + fn + r"\(", src), fn
    for unit in ("lg_train_ts.hip", "lg_train_pass.h"):
        assert "atomic" not in open(os.path.join(CSRC, unit)).read().lower()                    # determinism is the house rule


# ---- the restatement against the fixture ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return sc.load_fixture(FIXTURE)


def test_fixture_is_the_tiny_actor_critic_ts(fx):
    assert (fx["priv"], fx["actor"], fx["critic"], fx["hist"]) == sc.NETS["fixture"] == ([5, 8, 4, 3], [10, 16, 8, 3], [9, 16, 8, 1], [14, 8, 4, 3])
    assert fx["cfg"]["steps"] == 6 and fx["cfg"]["enc_steps"] == 12 and fx["cfg"]["enc_epochs"] == 2
    assert fx["rl_names"][-1] == "std" and all(n.startswith("history_encoder") for n in fx["enc_names"])
    assert fx["rl_names"] == [f"{c}.{i}.{k}" for c in ("actor", "critic", "privilege_encoder") for i in (0, 2, 4) for k in ("weight", "bias")] + ["std"]
    assert fx["obs"].shape == (6, 16, 7) and fx["privileged_obs"].shape == (6, 16, 5) and fx["critic_obs"].shape == (6, 16, 9)
    assert fx["enc_history"].shape == (12, 16, 14) and fx["enc_privileged"].shape == (12, 16, 5) and fx["enc_terminated"].shape == (12, 16, 1)
    for t in fx["enc_terminated"]:
        assert 0 < t.sum() < t.size and set(np.unique(t)) <= {0.0, 1.0}
    d, m = fx["cfg"]["desired_kl"], fx["cfg"]["max_grad_norm"]
    assert all(abs(k / (2 * d) - 1) > 0.01 and abs(k / (d / 2) - 1) > 0.01 for k in fx["kl"])
    assert all(abs(n / m - 1) > 0.01 for n in list(fx["grad_norm"]) + list(fx["enc_grad_norm"]))


def test_restatement_matches_the_reference_update(fx):
    """Every one of the 6 RL steps and 12 encoder steps of the reference's PPO_TS.update(): the restated passes, the loss head's restatement
    and the restated optimizer reproduce outputs, losses, gradients (the privilege encoder's through the latent included), norms, rates and
    every parameter to 1e-12."""
    cfg = fx["cfg"]
    params = {k: v.copy() for k, v in fx["init"].items()}
    state, lr = {}, cfg["lr0"]
    for s in range(cfg["steps"]):
        x = sc.fixture_inputs(fx, params, rl_step=s)
        fw = sc.rl_forward(x)
        for k in ("mu", "sigma", "values"):
            assert tc.max_err(fw[k], fx[k][s]) <= 1e-12, (s, k)
        r = pc.restate(sc.fixture_loss_inputs(fx, s, fw["mu"], fw["sigma"], fw["values"]), True, False, cfg["entropy_coef"], clip=cfg["clip_param"],
                       value_loss_coef=cfg["value_loss_coef"])
        assert abs(float(r["loss"]) - fx["loss"][s]) <= 1e-12 and abs(float(r["kl"][0]) - fx["kl"][s]) <= 1e-12
        x.update(grad_mu=r["grad_mu"][0], grad_sigma=r["grad_sigma"][0], grad_values=r["grad_values"])
        grads = sc.rl_backward(x)
        for name, g, want in zip(fx["rl_names"], grads, fx["grads"][s]):
            assert g.shape == want.shape and tc.max_err(g, want) <= 1e-12, (s, name)
        assert any(np.abs(g).max() > 0 for n, g in zip(fx["rl_names"], grads) if n.startswith("privilege_encoder"))
        step = ta.adam(x["rl_params"], grads, state, lr, cfg, kl=float(r["kl"][0]))
        lr = step["lr"]
        assert lr == fx["lr"][s] and abs(step["grad_norm"] - fx["grad_norm"][s]) <= 1e-12
        params.update(zip(fx["rl_names"], step["params"]))
        for n in fx["names"]:                                   # the history encoder's parameters stay: the RL step does not touch them
            assert tc.max_err(params[n], fx["params"][s][n]) <= 1e-12, (s, n)
    state = {}
    for s in range(cfg["enc_steps"]):
        x = sc.fixture_inputs(fx, params, enc_step=s)
        e = sc.enc_pass(x)
        assert abs(float(e["loss"]) - fx["enc_loss"][s]) <= 1e-12 and e["priv_grads"] is None
        for name, g, want in zip(fx["enc_names"], e["grads"], fx["enc_grads"][s]):
            assert g.shape == want.shape and tc.max_err(g, want) <= 1e-12, (s, name)
        step = ta.adam(x["enc_params"], e["grads"], state, cfg["encoder_lr"], cfg)
        assert abs(step["grad_norm"] - fx["enc_grad_norm"][s]) <= 1e-12
        params.update(zip(fx["enc_names"], step["params"]))
        for n in fx["names"]:                                   # the privilege encoder's too: the encoder step leaves it alone
            assert tc.max_err(params[n], fx["enc_params"][s][n]) <= 1e-12, (s, n)


HOST_CASES = ["fixture_b33", "fixture_b257", "fixture_noclip_b33", "one_four_b31", "go2_ts_b31", "go2_ts_noclip_b31", "o1_z1_b33", "o5_z17_b33",
              "o65_z4_b33", "o16_z65_b33", "wide_b9"]


@pytest.mark.parametrize("case", HOST_CASES)
def test_restatement_matches_torch_float64_autograd(case):
    x = sc.make_inputs(case)
    ref = sc.torch_passes(x, torch.float64)
    fw, e = sc.rl_forward(x), sc.enc_pass(x)
    rel = lambda a, b: tc.max_err(a, b) <= 1e-12 * max(1.0, np.abs(b).max())
    assert all(rel(fw[k], ref[k]) for k in ("mu", "sigma", "values")) and rel(e["loss"], ref["loss"])
    for name, g, want in zip(sc.rl_names(x["actor"], x["critic"], x["priv"]), sc.rl_backward(x), ref["rl_grads"]):
        assert g.shape == want.shape and rel(g, want), name
    for name, g, want in zip(sc.enc_names(x["hist"]), e["grads"], ref["enc_grads"]):
        assert g.shape == want.shape and rel(g, want), name
    rl_s, enc_s, tile = sc.kernel_order_slices(x)
    for g, want in zip(sc.rl_backward(x, slices=rl_s), sc.rl_backward(x)):
        assert rel(g, want)
    tiled = sc.enc_pass(x, slices=enc_s, row_tile=tile)
    assert rel(tiled["loss"], e["loss"]) and all(rel(a, b) for a, b in zip(tiled["grads"], e["grads"]))
    # the conventions, as autograd has them: nothing reaches the history encoder from the RL cotangents, nothing the privilege encoder from
    # the encoder loss, and the RL cotangents do reach the privilege encoder
    assert all(g is None for g in ref["enc_rl_grads"]) and all(g is None for g in ref["priv_enc_grads"])
    n_priv = 2 * (len(x["priv"]) - 1)
    assert all(np.abs(g).max() > 0 for g in ref["rl_grads"][-1 - n_priv:-1])
    # the upstream scalar scales the encoder's gradients, not the loss
    twice = sc.enc_pass(x, upstream=2.0 * float(x["upstream"]))
    assert twice["loss"] == e["loss"] and all(rel(a, 2.0 * b) for a, b in zip(twice["grads"], e["grads"]))
    # the module helper computes the same passes (what the GPU file hands to FusedTrainPassTS)
    m = sc.Module(x, dtype=torch.float64)
    d = lambda k: torch.as_tensor(x[k]).double()
    mu, sigma, values = m(d("obs"), d("privileged_obs"), d("critic_obs"))
    assert rel(mu.detach().numpy(), fw["mu"]) and rel(values.detach().numpy(), fw["values"])
    assert rel(m.encoder_loss(d("obs_history"), d("privileged_obs"), d("terminated")).detach().numpy(), e["loss"])


def test_masked_rows_and_the_mask_as_a_multiplication():
    x = sc.make_inputs("fixture_b33")
    off = dict(x, terminated=np.zeros_like(x["terminated"]))
    e = sc.enc_pass(off)
    assert e["loss"] == 0.0 and all((g == 0).all() for g in e["grads"])
    row = int(np.flatnonzero(x["terminated"][:, 0] == 0)[0])
    for key in ("obs_history", "privileged_obs"):               # a NaN prediction or a NaN target in a masked row: NaN * 0, in both
        bad = dict(x, **{key: x[key].copy()})
        bad[key][row, 1] = np.nan
        assert np.isnan(sc.enc_pass(bad)["loss"]) and np.isnan(sc.torch_passes(bad, torch.float64)["loss"])


# ---- the float32 restatement and the planted defects ------------------------------------------------------------------------------------------
def _restated(x, dtype=np.float64, rl_wrong=None, enc_wrong=None, kernel_order=False):
    rl_s, enc_s, tile = sc.kernel_order_slices(x) if kernel_order else (None, None, None)
    e = sc.enc_pass(x, dtype, slices=enc_s, row_tile=tile, wrong=enc_wrong)
    rl = sc.rl_backward(x, dtype, slices=rl_s, wrong=rl_wrong)
    if e["priv_grads"] is not None:                             # what autograd would accumulate into the privilege encoder's .grad
        na, nc = 2 * (len(x["actor"]) - 1), 2 * (len(x["critic"]) - 1)
        rl = rl[:na + nc] + [a + b for a, b in zip(rl[na + nc:-1], e["priv_grads"])] + rl[-1:]
    return sc.named(x, sc.rl_forward(x, dtype), rl, e["loss"], e["grads"])


@pytest.mark.parametrize("case", ["fixture_b257", "go2_ts_b257", "one_four_b33", "o5_z17_b33", "fixture_noclip_b33"])
def test_float32_restatement_in_the_kernels_order_keeps_half_the_rule(case):
    x = sc.make_inputs(case)
    r64, r32 = sc.references(x)
    sc.check_parity(_restated(x, np.float32, kernel_order=True), r64, r32, f"numpy f32 {case}", factor=oc.PARITY_FACTOR / 2)


def test_parity_rule_catches_the_planted_defects():
    x = sc.make_inputs("fixture_b257")
    r64, r32 = sc.references(x)
    sc.check_parity(_restated(x), r64, r32, "the restatement itself")
    with pytest.raises(AssertionError, match=r"privilege_encoder\.\d\.(weight|bias)"):
        sc.check_parity(_restated(x, rl_wrong="latent_cols0"), r64, r32, "latent gradient from columns [0, Z)")
    with pytest.raises(AssertionError, match=r"privilege_encoder\.\d\.(weight|bias)"):
        sc.check_parity(_restated(x, enc_wrong="target_grad"), r64, r32, "a target that passes the gradient on")
    # a select and a multiplication part ways only where a masked row is not finite: the rule sees it there
    row = int(np.flatnonzero(x["terminated"][:, 0] == 0)[0])
    y = dict(x, obs_history=x["obs_history"].copy())
    y["obs_history"][row, 0] = np.nan
    q64, q32 = sc.references(y)
    assert np.isnan(q64["loss"]).all() and np.isnan(q32["loss"]).all()
    wrong = _restated(y, enc_wrong="select")
    assert np.isfinite(wrong["loss"]).all()
    with pytest.raises(AssertionError, match=r"loss"):
        sc.check_parity(wrong, q64, q32, "the mask as a select")
    for case in ("o4_z5_b33", "o17_z16_b33"):                   # the column defect at other boundaries
        x = sc.make_inputs(case)
        r64, r32 = sc.references(x)
        with pytest.raises(AssertionError):
            sc.check_parity(_restated(x, rl_wrong="latent_cols0"), r64, r32, case)


# ---- the plans ----------------------------------------------------------------------------------------------------------------------------
PLAN_BATCHES = (1, 4, 31, 33, 64, 65, 127, 128, 129, 130, 257, 2048, 4097, 8193, 24576)


@pytest.mark.parametrize("net", ["fixture", "go2_ts", "one_four", "wide"] + sc.SWEEP)
def test_plans_against_the_restated_rules(net):
    priv, actor, critic, hist = sc.NETS[net]
    for b in PLAN_BATCHES if net in ("fixture", "go2_ts", "one_four", "wide") else (33, 257):
        p, want = train.plan_ts(b, priv, actor, critic), sc.restated_plan_ts(b, priv, actor, critic)
        assert (p.row_tile, p.lds_bytes, p.workspace_floats, p.weight_jobs, p.std_p_off, p.cat_off, p.enc_first_buffer) == \
            (want["row_tile"], want["lds_bytes"], want["workspace_floats"], want["weight_jobs"], want["std_p_off"], 0, want["enc_first_buffer"]), (net, b)
        assert (p.std_slices, p.std_slice_rows) == want["std"] and (p.gl_off, p.y_off, p.partial_off, p.loss_tiles) == (-1, -1, -1, 0)
        assert all(v == -1 for k in ("h_off", "g_off", "p_off") for v in getattr(p, k)[HIS])
        for i, (ci, c) in enumerate(((PRI, priv), (ACT, actor), (CRI, critic))):
            n = len(c) - 1
            for k in ("slices", "slice_rows", "h_off", "g_off", "p_off"):
                assert list(getattr(p, k)[ci])[:n] == want[k][i], (net, b, k)
            assert all(v == -1 for k in ("h_off", "g_off", "p_off") for v in list(getattr(p, k)[ci])[n:])
        q, want = train.plan_enc(b, hist, priv), sc.restated_plan_enc(b, hist, priv)
        assert (q.row_tile, q.lds_bytes, q.workspace_floats, q.weight_jobs, q.gl_off, q.y_off, q.partial_off, q.loss_tiles) == \
            (want["row_tile"], want["lds_bytes"], want["workspace_floats"], want["weight_jobs"], want["gl_off"], want["y_off"], want["partial_off"],
             want["loss_tiles"]), (net, b)
        n = len(hist) - 1
        for k in ("slices", "slice_rows", "h_off", "g_off", "p_off"):
            assert list(getattr(q, k)[HIS])[:n] == want[k][0], (net, b, k)
        assert all(v == -1 for k in ("h_off", "g_off", "p_off") for ci in (PRI, ACT, CRI) for v in getattr(q, k)[ci])
        assert q.partial_off % 2 == 0 and (q.cat_off, q.std_p_off, q.std_slices) == (-1, -1, 0)


def test_plan_edges():
    priv, actor, critic, hist = sc.NETS["go2_ts"]
    p, q = train.plan_ts(24576, priv, actor, critic), train.plan_enc(24576, hist, priv)
    assert p.row_tile == 16 and p.lds_bytes <= tc.LDS_BYTES < 2 * p.lds_bytes
    assert q.row_tile == 32 and q.lds_bytes == 150528
    assert list(p.slices[CRI])[0] == 9 and list(p.slice_rows[CRI])[0] == 2732 and list(q.slices[HIS])[0] == 32 and list(q.slice_rows[HIS])[0] == 768
    assert train.plan_ts(33, *sc.NETS["fixture"][:3]).enc_first_buffer == 0 and train.plan_ts(33, *sc.NETS["o4_z5"][:3]).enc_first_buffer == 1
    assert train.plan_ts(33, *sc.NETS["one_four"][:3]).enc_first_buffer == 0
    w = sc.NETS["wide"]
    assert train.plan_ts(9, *w[:3]).row_tile == 8 and train.plan_enc(9, w[3], w[0]).row_tile == 8
    f = sc.NETS["fixture"]
    q = train.plan_enc(8193, f[3], f[0])
    assert q.loss_tiles == 257 and list(q.slices[HIS]) [:3] == [32, 32, 32] and 8193 % list(q.slice_rows[HIS])[0] != 0


# ---- refusals of the entry points: nothing is enqueued (there is no device here) -----------------------------------------------------------
def _good_ts(backward=True):
    x = sc.make_inputs("fixture_b33")
    m = sc.Module(x)
    spec = train.describe_ts(m)
    t = lambda k: torch.as_tensor(x[k])
    keep = dict(m=m, o=t("obs"), p=t("privileged_obs"), c=t("critic_obs"), mu=torch.zeros(33, 3), sigma=torch.zeros(33, 3), values=torch.zeros(33, 1),
                gm=t("grad_mu"), gs=t("grad_sigma"), gv=t("grad_values"), grads=[torch.zeros_like(p) for p in spec.rl_parameters()])
    keep["ws"] = torch.zeros(int(train.plan_ts(33, *sc.NETS["fixture"][:3]).workspace_floats))
    a = train.ts_args(spec, keep["o"], keep["p"], keep["c"], keep["mu"], keep["sigma"], keep["values"], keep["ws"], keep["grads"] if backward else None,
                      keep["gm"], keep["gs"], keep["gv"])
    a._keep = keep
    return a


def _good_enc(backward=True):
    x = sc.make_inputs("fixture_b33")
    m = sc.Module(x)
    spec = train.describe_ts(m)
    t = lambda k: torch.as_tensor(x[k])
    keep = dict(m=m, h=t("obs_history"), p=t("privileged_obs"), t=t("terminated"), loss=torch.zeros(()), up=torch.ones(1),
                grads=[torch.zeros_like(p) for p in spec.encoder_parameters()])
    f = sc.NETS["fixture"]
    keep["ws"] = torch.zeros(int(train.plan_enc(33, f[3], f[0]).workspace_floats))
    a = train.enc_args(spec, keep["h"], keep["p"], keep["t"], keep["loss"], keep["ws"], keep["grads"] if backward else None, keep["up"])
    a._keep = keep
    return a


# (mutation, message, which entry points refuse it: p plan, f forward, b backward)
TS_REFUSALS = [
    (ta.set_path(("n_rows",), 0), b"n_rows = 0 < 1", "pfb"),
    (ta.set_path(("n_obs",), 0), b"n_obs = 0 < 1", "pfb"),
    (ta.set_path(("chain", 0, "n_layers"), 0), b"chain[0] (privilege encoder).n_layers = 0 is outside [1, 4]", "pfb"),
    (ta.set_path(("chain", 1, "n_layers"), 5), b"chain[1] (actor).n_layers = 5 is outside [1, 4]", "pfb"),
    (ta.set_path(("chain", 2, "layer", 1, "n_in"), 15), b"chain[2] (critic).layer[1].n_in = 15, but its input has 16 columns", "pfb"),
    (ta.set_path(("chain", 0, "layer", 2, "n_out"), 0), b"chain[0] (privilege encoder).layer[2].n_out = 0 is outside [1, 2048]", "pfb"),
    (ta.set_path(("chain", 2, "layer", 0, "n_in"), 2049), b"chain[2] (critic).layer[0].n_in = 2049 is outside [1, 2048]", "pfb"),
    (ta.set_path(("chain", 1, "layer", 0, "n_in"), 11), b"chain[1] (actor).layer[0].n_in = 11, but [obs | privilege encoder output] has 7 + 3 columns", "pfb"),
    (ta.set_path(("n_obs",), 6), b"chain[1] (actor).layer[0].n_in = 10, but [obs | privilege encoder output] has 6 + 3 columns", "pfb"),
    (ta.set_path(("chain", 0, "input"), None), b"chain[0] (privilege encoder).input is null", "fb"),
    (ta.set_path(("chain", 1, "input"), None), b"chain[1] (actor).input is null", "fb"),
    (ta.set_path(("chain", 2, "input"), None), b"chain[2] (critic).input is null", "fb"),
    (ta.set_path(("chain", 0, "in_stride"), 4), b"chain[0] (privilege encoder).in_stride = 4 is below its width 5", "fb"),
    (ta.set_path(("chain", 1, "in_stride"), 6), b"chain[1] (actor).in_stride = 6 is below its width 7", "fb"),
    (ta.set_path(("chain", 2, "in_stride"), 8), b"chain[2] (critic).in_stride = 8 is below its width 9", "fb"),
    (ta.set_path(("chain", 0, "layer", 1, "weight"), None), b"chain[0] (privilege encoder).layer[1].weight is null", "fb"),
    (ta.set_path(("chain", 1, "layer", 0, "bias"), None), b"chain[1] (actor).layer[0].bias is null", "fb"),
    (ta.set_path(("chain", 1, "layer", 2, "grad_weight"), None), b"chain[1] (actor).layer[2].grad_weight is null", "b"),
    (ta.set_path(("chain", 2, "layer", 1, "grad_bias"), None), b"chain[2] (critic).layer[1].grad_bias is null", "b"),
    (ta.set_path(("chain", 0, "layer", 0, "grad_weight"), None), b"chain[0] (privilege encoder).layer[0].grad_weight is null", "b"),
    (ta.set_path(("chain", 0, "layer", 2, "grad_bias"), None), b"chain[0] (privilege encoder).layer[2].grad_bias is null", "b"),
    (lambda a: (setattr(a, "clip_on", 1), setattr(a, "clip_actions", -1.0)), b"clip_actions must be >= 0 under clip_on", "fb"),
    (lambda a: (setattr(a, "clip_on", 1), setattr(a, "clip_actions", float("nan"))), b"clip_actions must be >= 0 under clip_on", "fb"),
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
ENC_REFUSALS = [
    (ta.set_path(("n_rows",), -2), b"n_rows = -2 < 1", "pfb"),
    (ta.set_path(("chain", 0, "n_layers"), 5), b"chain[0] (history encoder).n_layers = 5 is outside [1, 4]", "pfb"),
    (ta.set_path(("chain", 1, "n_layers"), 0), b"chain[1] (privilege encoder).n_layers = 0 is outside [1, 4]", "pfb"),
    (ta.set_path(("chain", 0, "layer", 1, "n_in"), 9), b"chain[0] (history encoder).layer[1].n_in = 9, but its input has 8 columns", "pfb"),
    (ta.set_path(("chain", 0, "layer", 0, "n_out"), 4000), b"chain[0] (history encoder).layer[0].n_out = 4000 is outside [1, 2048]", "pfb"),
    (ta.set_path(("chain", 1, "layer", 2, "n_out"), 4), b"chain[1] (privilege encoder).layer[2].n_out = 4, but the history encoder ends at 3 columns: the two "
                                                  b"encoders' output widths differ", "pfb"),
    (ta.set_path(("chain", 0, "layer", 2, "n_out"), 2), b"chain[1] (privilege encoder).layer[2].n_out = 3, but the history encoder ends at 2 columns", "pfb"),
    (ta.set_path(("chain", 0, "input"), None), b"chain[0] (history encoder).input is null", "fb"),
    (ta.set_path(("chain", 1, "input"), None), b"chain[1] (privilege encoder).input is null", "fb"),
    (ta.set_path(("chain", 0, "in_stride"), 3), b"chain[0] (history encoder).in_stride = 3 is below its width 14", "fb"),
    (ta.set_path(("chain", 1, "in_stride"), 4), b"chain[1] (privilege encoder).in_stride = 4 is below its width 5", "fb"),
    (ta.set_path(("chain", 0, "layer", 2, "weight"), None), b"chain[0] (history encoder).layer[2].weight is null", "fb"),
    (ta.set_path(("chain", 1, "layer", 0, "bias"), None), b"chain[1] (privilege encoder).layer[0].bias is null", "fb"),
    (ta.set_path(("chain", 0, "layer", 0, "grad_weight"), None), b"chain[0] (history encoder).layer[0].grad_weight is null", "b"),
    (ta.set_path(("chain", 0, "layer", 2, "grad_bias"), None), b"chain[0] (history encoder).layer[2].grad_bias is null", "b"),
    (ta.set_path(("mask",), None), b"mask is null", "fb"),
    (ta.set_path(("mask_stride",), 0), b"mask_stride = 0 is below its width 1", "fb"),
    (ta.set_path(("loss",), None), b"loss is null", "f"), (ta.set_path(("upstream",), None), b"upstream is null", "b"),
    (ta.set_path(("workspace",), None), b"workspace is null", "fb"),
    (lambda a: setattr(a, "workspace", a.workspace + 4), b"workspace is not 8-byte aligned", "fb"),
    (ta.set_path(("workspace_capacity",), 10), b"workspace_capacity = 10 floats is below the plan's", "fb"),
]


@pytest.mark.parametrize("i", range(len(TS_REFUSALS)))
def test_rl_entry_points_refuse(i):
    ta.refuse(TS_REFUSALS, i, _good_ts, "lg_train_ts", abi.LgTrainTSPlan)


@pytest.mark.parametrize("i", range(len(ENC_REFUSALS)))
def test_encoder_entry_points_refuse(i):
    ta.refuse(ENC_REFUSALS, i, _good_enc, "lg_train_enc", abi.LgTrainTSPlan)


def test_entry_points_refuse_null_descriptors_and_the_lds():
    lib = abi.load_lib()
    for fn, good in (("lg_train_ts", _good_ts), ("lg_train_enc", _good_enc)):
        plan = getattr(lib, fn + "_plan")
        assert plan(None, C.byref(abi.LgTrainTSPlan())) != 0 and (fn + "_plan: null descriptor").encode() in lib.lg_last_error()
        assert plan(C.byref(good()), None) != 0 and (fn + "_plan: null plan").encode() in lib.lg_last_error()
        for d in ("_forward", "_backward"):
            assert getattr(lib, fn + d)(None, None) != 0 and (fn + d + ": null descriptor").encode() in lib.lg_last_error()
        a = good(backward=False)                                              # a forward-only descriptor is what backward refuses
        assert getattr(lib, fn + "_backward")(C.byref(a), None) != 0
    assert 8 * 2 * tc.lds_stride(abi.POLICY_MAX_WIDTH) * 4 + sc.RED_BYTES <= tc.LDS_BYTES
    assert "does not fit the 160 KB of LDS" in open(os.path.join(CSRC, "lg_train_pass.h")).read()
    # the encoder pass leaves the privilege encoder's gradient members alone: train.enc_args does not even fill them
    a = _good_enc()
    assert all(not a.chain[abi.TRAIN_ENC_PRIVILEGE].layer[i].grad_weight and not a.chain[abi.TRAIN_ENC_PRIVILEGE].layer[i].grad_bias for i in range(3))
    assert all(a.chain[abi.TRAIN_ENC_HISTORY].layer[i].grad_weight for i in range(3))
    assert lib.lg_train_enc_plan(C.byref(a), C.byref(abi.LgTrainTSPlan())) == 0
    # and the RL descriptor has no history chain at all
    assert C.sizeof(abi.LgTrainTSArgs().chain) == abi.TRAIN_TS_RL_CHAINS * C.sizeof(abi.LgTrainChain)


# ---- refusals of the Python surface -------------------------------------------------------------------------------------------------------
class _TS(nn.Module):
    """O = 4, P = 5, Z = 2, H = 6."""

    def __init__(self, privilege_encoder=None, history_encoder=None, actor=None, critic=None, A=3):
        super().__init__()
        self.actor = actor if actor is not None else nn.Sequential(nn.Linear(6, 8), nn.ELU(), nn.Linear(8, A))
        self.critic = critic if critic is not None else nn.Sequential(nn.Linear(6, 8), nn.ELU(), nn.Linear(8, 1))
        self.privilege_encoder = privilege_encoder if privilege_encoder is not None else nn.Sequential(nn.Linear(5, 4), nn.ELU(), nn.Linear(4, 2))
        self.history_encoder = history_encoder if history_encoder is not None else nn.Sequential(nn.Linear(6, 4), nn.ELU(), nn.Linear(4, 2))
        self.std = nn.Parameter(torch.ones(A))


def test_describe_ts_takes_actor_critic_ts():
    m = _TS()
    spec = train.describe_ts(m)
    assert spec.privilege_encoder.widths == [5, 4, 2] and spec.history_encoder.widths == [6, 4, 2] and spec.actor.widths == [6, 8, 3]
    assert spec.critic.widths == [6, 8, 1] and spec.clip_actions is None and (spec.num_obs, spec.num_latent, spec.num_actions) == (4, 2, 3)
    assert spec.rl_parameter_names() == [f"{c}.{i}.{k}" for c in ("actor", "critic", "privilege_encoder") for i in (0, 1) for k in ("weight", "bias")] + ["std"]
    assert spec.encoder_parameter_names() == ["history_encoder.0.weight", "history_encoder.0.bias", "history_encoder.1.weight", "history_encoder.1.bias"]
    want = list(m.actor.parameters()) + list(m.critic.parameters()) + list(m.privilege_encoder.parameters()) + [m.std]       # PPO_TS.rl_parameters
    assert len(spec.rl_parameters()) == len(want) and all(a is b for a, b in zip(spec.rl_parameters(), want))
    assert all(a is b for a, b in zip(spec.encoder_parameters(), m.history_encoder.parameters()))
    clipped = train.describe_ts(_TS(actor=nn.Sequential(nn.Linear(6, 8), nn.ELU(), nn.Linear(8, 3), nn.Hardtanh(-0.5, 0.5))))
    assert clipped.clip_actions == 0.5
    # the other passes keep refusing the family exactly as before
    with pytest.raises(ValueError, match=r"FusedTrainPass: the module has \.privilege_encoder \(ActorCriticTS / ActorCriticCTS\); only the plain ActorCritic"):
        train.describe(m)
    with pytest.raises(ValueError, match=r"FusedTrainPassEE: the module has no \.estimator"):
        train.describe_ee(m)
    assert "PPO_TS's update only" in train.FusedTrainPassTS.__doc__ and "ActorCriticCTS" in train.FusedTrainPassTS.__doc__


def _break(f, **kw):
    m = _TS(**kw)
    f(m)
    return m


def _tcn():
    return nn.Sequential(nn.Conv1d(1, 3, 5, padding=2), nn.Conv1d(3, 3, 5, stride=2, padding=2), nn.Flatten(), nn.Linear(9, 4), nn.ELU(), nn.Linear(4, 2))


SURFACE_REFUSALS = [
    (lambda: _TS(history_encoder=_tcn()), r"FusedTrainPassTS: history_encoder\[0\] is Conv1d; only Linear and ELU are built"),
    (lambda: _TS(history_encoder=nn.Sequential(nn.Flatten(), nn.Linear(6, 2))), r"FusedTrainPassTS: history_encoder\[0\] is Flatten"),
    (lambda: _TS(history_encoder=nn.Sequential(nn.Linear(6, 4), nn.ELU(), nn.Linear(4, 3))), r"FusedTrainPassTS: history_encoder ends at 3 columns, privilege_encoder at 2: the latent widths differ"),
    (lambda: _break(lambda m: setattr(m, "estimator", nn.Sequential(nn.Linear(5, 2)))), r"FusedTrainPassTS: the module has \.estimator \(ActorCriticEE\) beside its encoders"),
    (lambda: _break(lambda m: setattr(m, "history_encoder", None)), r"FusedTrainPassTS: the module has no \.history_encoder"),
    (lambda: _break(lambda m: delattr(m, "history_encoder")), r"FusedTrainPassTS: the module has no \.history_encoder"),
    (lambda: _break(lambda m: setattr(m, "privilege_encoder", None)), r"FusedTrainPassTS: the module has no \.privilege_encoder"),
    (lambda: _TS(actor=nn.Sequential(nn.Linear(2, 8), nn.ELU(), nn.Linear(8, 3))), r"FusedTrainPassTS: actor\[0\] takes 2 inputs, but \[obs \| latent\] has O \+ 2 columns with O >= 1"),
    (lambda: _break(lambda m: setattr(m, "vae", nn.Sequential(nn.Linear(5, 2)))), r"\.vae \(ActorCriticDreamWaQ\) beside"),
    (lambda: _break(lambda m: setattr(m, "memory_a", nn.LSTM(5, 2))), r"\.memory_a \(ActorCriticRecurrent\) beside"),
    (lambda: _break(lambda m: setattr(m, "memory_c", nn.LSTM(5, 2))), r"\.memory_c \(ActorCriticRecurrent\) beside"),
    (lambda: _break(lambda m: setattr(m, "is_recurrent", True)), r"FusedTrainPassTS: the module is recurrent"),
    (lambda: _break(lambda m: delattr(m, "critic")), r"FusedTrainPassTS: the module has no \.critic"),
    (lambda: _TS(privilege_encoder=nn.Sequential(nn.Linear(5, 4), nn.Tanh(), nn.Linear(4, 2))), r"privilege_encoder\[1\] is Tanh; only Linear and ELU are built"),
    (lambda: _TS(privilege_encoder=nn.Sequential(nn.Linear(5, 4), nn.ELU(), nn.Linear(4, 2), nn.Hardtanh(-1, 1))), r"privilege_encoder\[3\] is Hardtanh"),
    (lambda: _TS(history_encoder=nn.Sequential(nn.Linear(6, 4), nn.ELU(alpha=0.5), nn.Linear(4, 2))), r"history_encoder\[1\] is ELU\(alpha=0\.5\), only alpha = 1"),
    (lambda: _TS(history_encoder=nn.Sequential(*[nn.Linear(6, 6) for _ in range(5)], nn.Linear(6, 2))), r"history_encoder has 6 Linear layers, the kernel takes 4"),
    (lambda: _TS(history_encoder=nn.GRU(6, 2)), r"history_encoder is GRU, expected an nn\.Sequential"),
    (lambda: _TS(critic=nn.Sequential(nn.Linear(6, 8), nn.ReLU(), nn.Linear(8, 1))), r"critic\[1\] is ReLU"),
    (lambda: _break(lambda m: setattr(m.privilege_encoder[0], "weight", nn.Parameter(torch.zeros(4, 5, dtype=torch.float64)))), r"privilege_encoder\[0\]\.weight is torch\.float64"),
    (lambda: _break(lambda m: setattr(m, "std", nn.Parameter(torch.ones(4)))), r"FusedTrainPassTS: std has shape \(4,\), the actor has 3 outputs"),
]


@pytest.mark.parametrize("i", range(len(SURFACE_REFUSALS)))
def test_describe_ts_refuses(i):
    make, msg = SURFACE_REFUSALS[i]
    with pytest.raises(ValueError, match=msg):
        train.describe_ts(make())


def test_the_surface_refuses_devices_and_tensors():
    with pytest.raises(ValueError, match=r"FusedTrainPassTS: the module is on cpu, not on a HIP device \(there is no CPU path\)"):
        train.FusedTrainPassTS(_TS())
    with pytest.raises(ValueError, match=r"privilege_encoder\[0\]\.weight is on cpu, not on cuda:0"):
        train.describe_ts(_TS(), torch.device("cuda:0"))
    spec = train.describe_ts(_TS())
    ok = dict(o=torch.zeros(4, 4), p=torch.zeros(4, 5), c=torch.zeros(4, 6), mu=torch.zeros(4, 3), sigma=torch.zeros(4, 3), values=torch.zeros(4, 1))
    call = lambda **kw: train.ts_args(spec, *[{**ok, **kw}[k] for k in ("o", "p", "c", "mu", "sigma", "values")], None)
    assert call().n_rows == 4 and call().n_obs == 4 and call().clip_on == 0
    for kw, msg in ((dict(o=torch.zeros(4, 5)), r"FusedTrainPassTS: actor\[0\] takes 6 inputs, but \[obs \| latent\] has 5 \+ 2 columns"),
                    (dict(p=torch.zeros(4, 6)), r"FusedTrainPassTS: privileged_obs must be \(4, 5\) float32"),
                    (dict(c=torch.zeros(3, 6)), r"critic_obs must be \(4, 6\)"), (dict(o=torch.zeros(0, 4)), r"obs must be a \(B, O\) float32 tensor with B >= 1"),
                    (dict(mu=torch.zeros(4, 2)), r"mu must be \(4, 3\)")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    enc = lambda **kw: train.enc_args(spec, *[{**dict(h=torch.zeros(4, 6), p=ok["p"], t=torch.ones(4, 1), loss=torch.zeros(())), **kw}[k]
                                              for k in ("h", "p", "t", "loss")], None)
    assert enc().n_rows == 4 and enc().mask_stride == 1
    for kw, msg in ((dict(h=torch.zeros(4, 7)), r"obs_history must be \(4, 6\)"), (dict(t=torch.ones(4)), r"terminated must be \(4, 1\)"),
                    (dict(t=torch.ones(4, 1, dtype=torch.uint8)), r"terminated must be \(4, 1\) float32"), (dict(loss=torch.zeros(2)), r"the loss must be one float32")):
        with pytest.raises(ValueError, match=msg):
            enc(**kw)
    wide = torch.zeros(4, 16)                                                 # strided views are addressed in place
    a = enc(h=wide[:, 2:8], p=wide[:, 9:14], t=wide[:, 15:16])
    his, pri = a.chain[abi.TRAIN_ENC_HISTORY], a.chain[abi.TRAIN_ENC_PRIVILEGE]
    assert (his.input, his.in_stride, pri.input, pri.in_stride, a.mask, a.mask_stride) == \
        (wide.data_ptr() + 8, 16, wide.data_ptr() + 36, 16, wide.data_ptr() + 60, 16)


# ---- the case table -----------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_the_edges():
    nets = {c["net"] for c in sc.CASES.values()}
    assert set(sc.SWEEP) <= nets and len(sc.SWEEP) == 36 and {"fixture", "one_four", "go2_ts", "wide"} <= nets
    assert sc.NETS["go2_ts"] == ([94, 256, 128, 94], [139, 512, 256, 128, 12], [860, 1024, 256, 128, 1], [900, 256, 128, 94])
    assert all(p[-1] == h[-1] and a[0] > p[-1] for p, a, _, h in sc.NETS.values())
    assert (len(sc.NETS["one_four"][0]) - 1, len(sc.NETS["one_four"][1]) - 1) == (1, 4)
    for net in ("fixture", "one_four") + sc.REAL:
        assert {sc.CASES[f"{net}_b{b}"]["B"] for b in sc.BATCHES} == {1, 31, 33, 257}
    O = {sc.NETS[n][1][0] - sc.NETS[n][0][-1] for n in sc.SWEEP}
    Z = {sc.NETS[n][0][-1] for n in sc.SWEEP}
    assert O == Z == {1, 4, 5, 16, 17, 65} and {o % 4 for o in O} >= {0, 1} and 1 in Z              # the boundary off and on a multiple of 4; Z = 1
    assert any(o % 16 and (o % 16) + z > 16 for o in O for z in Z)                                  # a latent slice across 16-column tiles
    assert {0, 1} == {sc.restated_plan_ts(33, *sc.NETS[n][:3])["enc_first_buffer"] for n in ("fixture", "o4_z5")}
    assert {sc.CASES[c]["B"] for c in ("wide_b1", "wide_b9")} == {1, 9}
    w = sc.NETS["wide"]
    assert sc.restated_plan_ts(9, *w[:3])["row_tile"] == 8 and sc.restated_plan_enc(9, w[3], w[0])["row_tile"] == 8
    g = sc.NETS["go2_ts"]
    assert sc.restated_plan_ts(257, *g[:3])["row_tile"] == 16
    assert (sc.restated_plan_enc(257, g[3], g[0])["row_tile"], sc.restated_plan_enc(257, g[3], g[0])["lds_bytes"]) == (32, 150528)
    f = sc.NETS["fixture"]
    big = sc.restated_plan_enc(sc.CASES["fixture_b8193"]["B"], f[3], f[0])
    assert big["loss_tiles"] > 256 and big["slices"][0][0] == tc.MAX_SLICES and 8193 % big["slice_rows"][0][0]       # second finalize trip; 32 slices, short last
    assert sc.restated_plan_ts(8193, *f[:3])["slices"][1][0] == tc.MAX_SLICES
    for net in sc.RAGGED_SLICE_NETS:
        assert 64 < sc.smallest_ragged_b(net) <= 257
    assert sc.make_inputs("fixture_noclip_b33")["clip"] is None and sc.make_inputs("go2_ts_noclip_b31")["clip"] is None
    for name in ("fixture_b33", "go2_ts_b31", "o65_z17_b33"):
        x = sc.make_inputs(name)
        pre = sc.rl_forward(dict(x, clip=None))["mu"]
        assert 0.1 <= (np.abs(pre) >= x["clip"]).mean() <= 0.9 and np.abs(np.abs(pre) - x["clip"]).min() >= 1e-3
    x = sc.make_inputs("fixture_b257")
    assert 0.1 <= 1 - x["terminated"].mean() <= 0.6                                                     # masked and unmasked rows
    # what this table stops short of (the 16-row tile in both passes, the 8-row tile beyond net `wide`, four-layer encoders, 31 slices, the
    # finalize's second trip from 8-row tiles, the two passes on different tiles) are the rows of kind "ts" of tests/train_edges.py
    from tests import train_edges as te
    ts = [c for c in te.CASES if te.ROWS[c[0]]["kind"] == "ts"]
    assert te.TS_TABLE_TAGS <= set().union(*(te.claimed(*c) for c in ts)) and {te.ROWS[r]["R"] for r, _ in ts} >= {(16, 16), (8, 8), (8, 32), (16, 32)}
    assert all(te.claimed(*c) <= te.tags(*c) for c in ts)

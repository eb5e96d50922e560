"""Host side of the concurrent teacher-student learner passes (hcr_genesis_lr_cl_amd/train.py's FusedTrainPassCTS, include/lgtraincts.h):
the ctypes mirror against the header, the exports and the translation unit, the float64 restatement of tests/train_cts_cases.py against the
golden fixture of the reference's own PPO_CTS.update() (tests/golden/ppo_cts_train.npz) and against torch float64 autograd, the plan of
lg_train_cts_plan against the restated rules, every refusal of the entry points and of describe_cts / cts_args, the float32 restatement in
the kernel's order of sums under half the parity rule, seven planted defects that the rule must catch, and the coverage of the case
table.  No GPU needed: nothing is launched."""
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
from tests import train_cts_cases as cc
from tests import train_support as sup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lgtraincts.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ppo_cts_train.npz")
CSRC = os.path.join(ROOT, "hcr_genesis_lr_cl_amd", "csrc")
PRI, ACT, CRI, HIS = abi.TRAIN_CTS_PRIVILEGE, abi.TRAIN_CTS_ACTOR, abi.TRAIN_CTS_CRITIC, abi.TRAIN_CTS_HISTORY


# ---- the structs --------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header():
    structs = [("LgTrainCTSArgs", abi.LgTrainCTSArgs), ("LgTrainCTSPlan", abi.LgTrainCTSPlan), ("LgTrainChain", abi.LgTrainChain)]
    consts = dict(LG_TRAIN_CTS_CHAINS=abi.TRAIN_CTS_CHAINS, LG_TRAIN_CTS_PRIVILEGE=PRI, LG_TRAIN_CTS_ACTOR=ACT, LG_TRAIN_CTS_CRITIC=CRI,
                  LG_TRAIN_CTS_HISTORY=HIS, LG_TRAIN_CTS_GROUPS=abi.TRAIN_CTS_GROUPS, LG_TRAIN_CTS_TEACHER=abi.TRAIN_CTS_TEACHER,
                  LG_TRAIN_CTS_STUDENT=abi.TRAIN_CTS_STUDENT, LG_TRAIN_CTS_ROLES=abi.TRAIN_CTS_ROLES, LG_TRAIN_CTS_ROLE_CRITIC=abi.TRAIN_CTS_ROLE_CRITIC,
                  LG_TRAIN_TS_TARGET_JOBS=abi.TRAIN_TS_TARGET_JOBS, LG_POLICY_MAX_LAYERS=abi.POLICY_MAX_LAYERS)
    ta.check_layout(HEADER, structs, consts)
    assert cc.TARGET_JOBS == abi.TRAIN_TS_TARGET_JOBS


def test_library_exports_the_entry_points():
    declared = ta.check_exports(HEADER, abi.TRAIN_CTS_EXPORTS, "lg_train_cts", ["lg_train_tiles.h", "lg_train_pass.h"])
    assert declared == {"lg_train_cts_plan", "lg_train_cts_forward", "lg_train_cts_backward"}
    from hcr_genesis_lr_cl_amd import build
    assert f"{len(build.units())} translation units" in build.__doc__
    assert "TRAIN_CTS_EXPORTS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()         # the build's export check covers the list
    # one copy of the layer and pass routines: the unit includes the shared header and defines none of them
    src = open(os.path.join(CSRC, "lg_train_cts.hip")).read()
    for fn in ("stage_rows", "copy_out", "fwd_tile", "bwd_tile", "wgrad_wave", "colsum_wave", "combine_layer", "combine_cols", "lds_stride", "slice_rule",
               "chain_forward", "chain_from_rows", "chain_backward", "bwd_layer", "seed_last_g", "store_sigma", "combine_all", "plan_chain", "bind_chain",
               "check_ws", "done", "raise_lds"):
        assert '#include "lg_train_pass.h"' in src and not re.findall(r"\b(?:void|int|lds_f \*) ?" + fn + r"\(", src), fn
        assert fn in src or fn in ("lds_stride", "combine_layer", "combine_cols", "fwd_tile", "bwd_tile"), fn       # and uses them
    assert "atomic" not in src.lower()                                                           # determinism is the house rule
    assert "train_cts" in open(os.path.join(ROOT, "tools", "register_table.py")).read()


# ---- the restatement against the fixture ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return cc.load_fixture(FIXTURE)


def test_fixture_is_the_tiny_actor_critic_cts(fx):
    assert (fx["priv"], fx["actor"], fx["critic"], fx["hist"]) == cc.NETS["fixture"] == ([5, 8, 4, 3], [10, 16, 8, 3], [9, 16, 8, 1], [14, 8, 4, 3])
    assert fx["cfg"]["steps"] == 6 and fx["cfg"]["enc_steps"] == 12 and fx["cfg"]["enc_epochs"] == 2
    assert fx["rl_names"] == [f"{c}.{i}.{k}" for c in ("actor", "critic", "privilege_encoder") for i in (0, 2, 4) for k in ("weight", "bias")] + ["std"]
    assert all(n.startswith("history_encoder") for n in fx["enc_names"])
    assert fx["teacher_obs"].shape == (6, 10, 7) and fx["teacher_privileged_obs"].shape == (6, 10, 5) and fx["student_obs"].shape == (6, 6, 7)
    assert fx["student_obs_history"].shape == (6, 6, 14) and fx["critic_obs"].shape == (6, 16, 9)
    assert fx["mu_t"].shape == (6, 10, 3) and fx["mu_s"].shape == (6, 6, 3) and fx["values"].shape == (6, 16, 1)
    assert fx["enc_history"].shape == (12, 6, 14) and fx["enc_privileged"].shape == (12, 6, 5)
    d, m = fx["cfg"]["desired_kl"], fx["cfg"]["max_grad_norm"]
    assert all(abs(k / (2 * d) - 1) > 0.01 and abs(k / (d / 2) - 1) > 0.01 for k in fx["kl"])
    assert all(abs(n / m - 1) > 0.01 for n in list(fx["grad_norm"]) + list(fx["enc_grad_norm"]))
    assert len(set(float(v) for v in fx["lr"])) > 2                                              # the rate rule moves


def test_restatement_matches_the_reference_update(fx):
    """Every one of the 6 RL steps and 12 encoder steps of the reference's PPO_CTS.update(): the restated passes, the two-group loss head's
    restatement and the restated optimizer reproduce outputs, loss, surrogates, KL, gradients (the privilege encoder's through the
    teacher's latent included), norms, rates and EVERY parameter to 1e-12 -- with no RL gradient for the history encoder at all, which is
    the convention of include/lgtraincts.h: the gradient torch accumulates there is never read."""
    cfg = fx["cfg"]
    params = {k: v.copy() for k, v in fx["init"].items()}
    state, lr = {}, cfg["lr0"]
    for s in range(cfg["steps"]):
        x = cc.fixture_inputs(fx, params, rl_step=s)
        fw = cc.rl_forward(x)
        for k in cc.OUTPUTS:
            assert tc.max_err(fw[k], fx[k][s]) <= 1e-12, (s, k)
        r = pc.restate(cc.fixture_loss_inputs(fx, s, fw), True, False, cfg["entropy_coef"], clip=cfg["clip_param"], value_loss_coef=cfg["value_loss_coef"])
        assert abs(float(r["loss"]) - fx["loss"][s]) <= 1e-12 and abs(float(r["kl"][0]) - fx["kl"][s]) <= 1e-12 and r["kl"][1] is None
        assert abs(float(r["surrogate"][0]) - fx["teacher_surrogate"][s]) <= 1e-12 and abs(float(r["surrogate"][1]) - fx["student_surrogate"][s]) <= 1e-12
        x.update(grad_mu_t=r["grad_mu"][0], grad_sigma_t=r["grad_sigma"][0], grad_mu_s=r["grad_mu"][1], grad_sigma_s=r["grad_sigma"][1],
                 grad_values=r["grad_values"])
        grads = cc.rl_backward(x)
        for name, g, want in zip(fx["rl_names"], grads, fx["grads"][s]):
            assert g.shape == want.shape and tc.max_err(g, want) <= 1e-12, (s, name)
        assert any(np.abs(g).max() > 0 for n, g in zip(fx["rl_names"], grads) if n.startswith("privilege_encoder"))
        step = ta.adam(x["rl_params"], grads, state, lr, cfg, kl=float(r["kl"][0]))
        lr = step["lr"]
        assert lr == fx["lr"][s] and abs(step["grad_norm"] - fx["grad_norm"][s]) <= 1e-12
        params.update(zip(fx["rl_names"], step["params"]))
        for n in fx["names"]:                                   # the history encoder's parameters stay: no RL step ever moves them
            assert tc.max_err(params[n], fx["params"][s][n]) <= 1e-12, (s, n)
    state = {}
    for s in range(cfg["enc_steps"]):
        x = cc.fixture_inputs(fx, params, enc_step=s)
        e = cc.enc_pass(x)
        assert abs(float(e["loss"]) - fx["enc_loss"][s]) <= 1e-12 and e["priv_grads"] is None
        for name, g, want in zip(fx["enc_names"], e["grads"], fx["enc_grads"][s]):
            assert g.shape == want.shape and tc.max_err(g, want) <= 1e-12, (s, name)
        step = ta.adam(x["enc_params"], e["grads"], state, cfg["encoder_lr"], cfg)
        assert abs(step["grad_norm"] - fx["enc_grad_norm"][s]) <= 1e-12
        params.update(zip(fx["enc_names"], step["params"]))
        for n in fx["names"]:                                   # the privilege encoder's too: the encoder step leaves it alone
            assert tc.max_err(params[n], fx["enc_params"][s][n]) <= 1e-12, (s, n)


@pytest.mark.parametrize("case", list(cc.CASES))
def test_restatement_matches_torch_float64_autograd(case):
    x = cc.make_inputs(case)
    ref = cc.torch_passes(x, torch.float64)
    fw, e = cc.rl_forward(x), cc.enc_pass(x)
    rel = lambda a, b: tc.max_err(a, b) <= 1e-12 * max(1.0, np.abs(b).max())
    assert all(rel(fw[k], ref[k]) for k in cc.OUTPUTS) and rel(e["loss"], ref["loss"])
    for name, g, want in zip(cc.rl_names(x["actor"], x["critic"], x["priv"]), cc.rl_backward(x), ref["rl_grads"]):
        assert g.shape == want.shape and rel(g, want), name
    for name, g, want in zip(cc.enc_names(x["hist"]), e["grads"], ref["enc_grads"]):
        assert g.shape == want.shape and rel(g, want), name
    rl_s, enc_s, tile = cc.kernel_order_slices(x)
    for g, want in zip(cc.rl_backward(x, slices=rl_s), cc.rl_backward(x)):
        assert rel(g, want)
    tiled = cc.enc_pass(x, slices=enc_s, row_tile=tile)
    assert rel(tiled["loss"], e["loss"]) and all(rel(a, b) for a, b in zip(tiled["grads"], e["grads"]))
    # as autograd has it: the RL cotangents DO reach the history encoder (the gradient the reference discards), the encoder loss sends
    # nothing into the privilege encoder, and the RL cotangents reach the privilege encoder
    assert all(g is not None for g in ref["enc_rl_grads"]) and any(np.abs(g).max() > 0 for g in ref["enc_rl_grads"])
    assert all(g is None for g in ref["priv_enc_grads"])
    n_priv = 2 * (len(x["priv"]) - 1)
    assert x["teacher_obs"].shape[0] == 1 or all(np.abs(g).max() > 0 for g in ref["rl_grads"][-1 - n_priv:-1])      # one row may sit on the clip
    # the module helper computes the same passes (what the GPU file hands to FusedTrainPassCTS)
    m = cc.Module(x, dtype=torch.float64)
    d = lambda k: torch.as_tensor(x[k]).double()
    outs = m(d("teacher_obs"), d("teacher_privileged_obs"), d("student_obs"), d("student_obs_history"), d("critic_obs"))
    assert all(rel(o.detach().numpy(), fw[k]) for o, k in zip(outs, cc.OUTPUTS))
    assert rel(m.encoder_loss(d("student_obs_history"), d("student_privileged_obs")).detach().numpy(), e["loss"])


# ---- the float32 restatement and the planted defects ------------------------------------------------------------------------------------------
def _restated(x, dtype=np.float64, wrong=None, kernel_order=False):
    rl_s, enc_s, tile = cc.kernel_order_slices(x) if kernel_order else (None, None, None)
    e = cc.enc_pass(x, dtype, slices=enc_s, row_tile=tile)
    return cc.named(x, cc.rl_forward(x, dtype, wrong), cc.rl_backward(x, dtype, slices=rl_s, wrong=wrong), e["loss"], e["grads"])


@pytest.mark.parametrize("case", list(cc.CASES))
def test_float32_restatement_in_the_kernels_order_keeps_half_the_rule(case):
    x = cc.make_inputs(case)
    r64, r32 = cc.references(x)
    cc.check_parity(_restated(x, np.float32, kernel_order=True), r64, r32, f"numpy f32 {case}", factor=oc.PARITY_FACTOR / 2)


DEFECTS = [("student_latent_from_priv", r"mu|actor"), ("actor_teacher_rows_only", r"actor\.\d\.(weight|bias)"), ("student_rows_at_0", r"actor\.\d\.(weight|bias)"),
           ("priv_all_rows", r"privilege_encoder\.\d\.(weight|bias)"), ("latent_cols0", r"privilege_encoder\.\d\.(weight|bias)"), ("std_one_group", r"std"),
           ("critic_bt_rows", r"critic\.\d\.(weight|bias)")]


@pytest.mark.parametrize("wrong,where", DEFECTS)
def test_parity_rule_catches_the_planted_defects(wrong, where):
    """Each defect is a change of the restatement alone and fails the unchanged rule, on a case of more than one tile per group and on the
    case whose actor slice holds rows of both groups."""
    assert wrong in cc.WRONG
    for case in ("fixture_above_tile", "fixture_straddle", "ts_r16"):
        x = cc.make_inputs(case)
        r64, r32 = cc.references(x)
        cc.check_parity(_restated(x), r64, r32, "the restatement itself")
        with pytest.raises(AssertionError, match=where):
            cc.check_parity(_restated(x, wrong=wrong), r64, r32, f"{wrong} on {case}")
    assert {d for d, _ in DEFECTS} == set(cc.WRONG)


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
def _check_plan(net, bt, bs, bc):
    priv, actor, critic, hist = cc.NETS[net]
    p, want = train.plan_cts(bt, bs, bc, priv, actor, critic, hist), cc.restated_plan_cts(bt, bs, bc, priv, actor, critic, hist)
    assert (p.row_tile, p.lds_bytes, p.workspace_floats, p.weight_jobs, p.std_p_off, p.cat_off) == \
        (want["row_tile"], want["lds_bytes"], want["workspace_floats"], want["weight_jobs"], want["std_p_off"], 0), (net, bt, bs, bc)
    assert list(p.enc_first_buffer) == want["enc_first_buffer"] and list(p.tiles) == want["tiles"]
    assert [(s, r) for s, r in zip(p.std_slices, p.std_slice_rows)] == want["std"]
    assert all(v == -1 for k in ("h_off", "g_off", "p_off") for v in getattr(p, k)[HIS]) and not any(p.slices[HIS])       # nothing of it is stored
    for i, (ci, c) in enumerate(((PRI, priv), (ACT, actor), (CRI, critic))):
        n = len(c) - 1
        for k in ("slices", "slice_rows", "h_off", "g_off", "p_off"):
            assert list(getattr(p, k)[ci])[:n] == want[k][i], (net, bt, bs, bc, k)
        assert all(v == -1 for k in ("h_off", "g_off", "p_off") for v in list(getattr(p, k)[ci])[n:])
    return p


@pytest.mark.parametrize("case", list(cc.CASES))
def test_plan_against_the_restated_rules(case):
    c = cc.CASES[case]
    _check_plan(c["net"], c["Bt"], c["Bs"], c["Bc"])
    for rows in ((1, 1, 1), (64, 65, 1), (129, 128, 4097), (18432, 6144, 24576)):
        _check_plan(c["net"], *rows)


def test_plan_edges():
    g = cc.NETS["go2_cts"]
    p = train.plan_cts(18432, 6144, 24576, *g)
    assert p.row_tile == 16 and p.lds_bytes <= tc.LDS_BYTES < 2 * p.lds_bytes and list(p.tiles) == [1152, 384, 1536]
    assert list(p.slices[CRI])[0] == 9 and list(p.slice_rows[CRI])[0] == 2732                    # the critic's first layer, as in go2_ts
    assert list(p.std_slices) == [32, 32] and list(p.std_slice_rows) == [576, 192]
    assert [train.plan_cts(5, 5, 5, *cc.NETS[f"enc_{a}_{b}"]).enc_first_buffer[:] for a, b in cc.ENC_DEPTHS] == [[0, 0], [0, 1], [1, 0], [1, 1]]
    assert cc.tile_of("fixture") == 32 and cc.tile_of("ts_r16") == 16 and cc.tile_of("ts_r8_z") == 8 and cc.tile_of("go2_cts") == 16
    # the row counts are independent: the critic's regions follow n_critic alone
    a, b = train.plan_cts(7, 9, 16, *cc.NETS["fixture"]), train.plan_cts(7, 9, 100, *cc.NETS["fixture"])
    assert list(a.g_off[ACT]) == list(b.g_off[ACT]) and list(a.g_off[PRI]) == list(b.g_off[PRI]) and a.workspace_floats < b.workspace_floats


# ---- refusals of the entry points: nothing is enqueued (there is no device here) -----------------------------------------------------------
def _good(backward=True):
    x = cc.make_inputs("fixture_odd_teacher")
    m = cc.Module(x)
    spec = train.describe_cts(m)
    t = lambda k: torch.as_tensor(x[k])
    keep = dict(m=m, ins=[t(k) for k in ("teacher_obs", "teacher_privileged_obs", "student_obs", "student_obs_history", "critic_obs")],
                outs=[torch.zeros(7, 3), torch.zeros(7, 3), torch.zeros(9, 3), torch.zeros(9, 3), torch.zeros(16, 1)], cot=[t(k) for k in cc.COTANGENTS],
                grads=[torch.zeros_like(p) for p in spec.rl_parameters()])
    keep["ws"] = torch.zeros(int(train.plan_cts(7, 9, 16, *cc.NETS["fixture"]).workspace_floats))
    a = train.cts_args(spec, *keep["ins"], *keep["outs"], keep["ws"], keep["grads"] if backward else None, *keep["cot"])
    a._keep = keep
    return a


def _set_item(name, i, value):
    return lambda a: getattr(a, name).__setitem__(i, value)


CTS_REFUSALS = [
    (ta.set_path(("n_teacher",), 0), b"n_teacher = 0 < 1", "pfb"),
    (ta.set_path(("n_student",), -1), b"n_student = -1 < 1", "pfb"),
    (ta.set_path(("n_critic",), 0), b"n_critic = 0 < 1", "pfb"),
    (ta.set_path(("n_obs",), 0), b"n_obs = 0 < 1", "pfb"),
    (lambda a: (setattr(a, "n_teacher", 2 ** 31 - 1), setattr(a, "n_student", 1)), b"n_teacher + n_student is above 2^31 - 1", "pfb"),
    (ta.set_path(("chain", 0, "n_layers"), 0), b"chain[0] (privilege encoder).n_layers = 0 is outside [1, 4]", "pfb"),
    (ta.set_path(("chain", 1, "n_layers"), 5), b"chain[1] (actor).n_layers = 5 is outside [1, 4]", "pfb"),
    (ta.set_path(("chain", 3, "n_layers"), 5), b"chain[3] (history encoder).n_layers = 5 is outside [1, 4]", "pfb"),
    (ta.set_path(("chain", 2, "layer", 1, "n_in"), 15), b"chain[2] (critic).layer[1].n_in = 15, but its input has 16 columns", "pfb"),
    (ta.set_path(("chain", 0, "layer", 2, "n_out"), 0), b"chain[0] (privilege encoder).layer[2].n_out = 0 is outside [1, 2048]", "pfb"),
    (ta.set_path(("chain", 3, "layer", 0, "n_in"), 2049), b"chain[3] (history encoder).layer[0].n_in = 2049 is outside [1, 2048]", "pfb"),
    (ta.set_path(("chain", 3, "layer", 2, "n_out"), 4), b"chain[3] (history encoder).layer[2].n_out = 4, but the privilege encoder ends at 3 columns: the two "
                                                  b"encoders' output widths differ", "pfb"),
    (ta.set_path(("chain", 1, "layer", 0, "n_in"), 11), b"chain[1] (actor).layer[0].n_in = 11, but [obs | encoder output] has 7 + 3 columns", "pfb"),
    (ta.set_path(("n_obs",), 6), b"chain[1] (actor).layer[0].n_in = 10, but [obs | encoder output] has 6 + 3 columns", "pfb"),
    (ta.set_path(("chain", 0, "input"), None), b"chain[0] (privilege encoder).input is null", "fb"),
    (ta.set_path(("chain", 1, "input"), None), b"chain[1] (actor).input is null", "fb"),
    (ta.set_path(("chain", 2, "input"), None), b"chain[2] (critic).input is null", "fb"),
    (ta.set_path(("chain", 3, "input"), None), b"chain[3] (history encoder).input is null", "fb"),
    (ta.set_path(("student_obs",), None), b"student_obs is null", "fb"),
    (ta.set_path(("chain", 0, "in_stride"), 4), b"chain[0] (privilege encoder).in_stride = 4 is below its width 5", "fb"),
    (ta.set_path(("chain", 1, "in_stride"), 6), b"chain[1] (actor).in_stride = 6 is below its width 7", "fb"),
    (ta.set_path(("chain", 2, "in_stride"), 8), b"chain[2] (critic).in_stride = 8 is below its width 9", "fb"),
    (ta.set_path(("chain", 3, "in_stride"), 13), b"chain[3] (history encoder).in_stride = 13 is below its width 14", "fb"),
    (ta.set_path(("student_obs_stride",), 6), b"student_obs_stride = 6 is below its width 7", "fb"),
    (ta.set_path(("chain", 0, "layer", 1, "weight"), None), b"chain[0] (privilege encoder).layer[1].weight is null", "fb"),
    (ta.set_path(("chain", 3, "layer", 2, "bias"), None), b"chain[3] (history encoder).layer[2].bias is null", "fb"),
    (ta.set_path(("chain", 1, "layer", 2, "grad_weight"), None), b"chain[1] (actor).layer[2].grad_weight is null", "b"),
    (ta.set_path(("chain", 2, "layer", 1, "grad_bias"), None), b"chain[2] (critic).layer[1].grad_bias is null", "b"),
    (ta.set_path(("chain", 0, "layer", 0, "grad_weight"), None), b"chain[0] (privilege encoder).layer[0].grad_weight is null", "b"),
    (lambda a: (setattr(a, "clip_on", 1), setattr(a, "clip_actions", -1.0)), b"clip_actions must be >= 0 under clip_on", "fb"),
    (lambda a: (setattr(a, "clip_on", 1), setattr(a, "clip_actions", float("nan"))), b"clip_actions must be >= 0 under clip_on", "fb"),
    (ta.set_path(("std",), None), b"std is null", "fb"),
    (_set_item("mu", 0, None), b"mu[0] (teacher) is null", "fb"), (_set_item("mu", 1, None), b"mu[1] (student) is null", "fb"),
    (_set_item("sigma", 0, None), b"sigma[0] (teacher) is null", "fb"), (_set_item("sigma", 1, None), b"sigma[1] (student) is null", "fb"),
    (ta.set_path(("values",), None), b"values is null", "fb"),
    (_set_item("mu_stride", 1, 2), b"mu_stride[1] (student) = 2 is below its width 3", "fb"),
    (_set_item("sigma_stride", 0, 0), b"sigma_stride[0] (teacher) = 0 is below its width 3", "fb"),
    (ta.set_path(("values_stride",), 0), b"values_stride = 0 is below its width 1", "fb"),
    (ta.set_path(("grad_std",), None), b"grad_std is null", "b"),
    (_set_item("grad_mu", 0, None), b"grad_mu[0] (teacher) is null", "b"), (_set_item("grad_mu", 1, None), b"grad_mu[1] (student) is null", "b"),
    (_set_item("grad_sigma", 0, None), b"grad_sigma[0] (teacher) is null", "b"), (_set_item("grad_sigma", 1, None), b"grad_sigma[1] (student) is null", "b"),
    (ta.set_path(("grad_values",), None), b"grad_values is null", "b"),
    (_set_item("grad_mu_stride", 0, 2), b"grad_mu_stride[0] (teacher) = 2 is below its width 3", "b"),
    (_set_item("grad_sigma_stride", 1, 1), b"grad_sigma_stride[1] (student) = 1 is below its width 3", "b"),
    (ta.set_path(("grad_values_stride",), 0), b"grad_values_stride = 0 is below its width 1", "b"),
    (ta.set_path(("workspace",), None), b"workspace is null", "fb"),
    (ta.set_path(("workspace_capacity",), 10), b"workspace_capacity = 10 floats is below the plan's", "fb"),
]


@pytest.mark.parametrize("i", range(len(CTS_REFUSALS)))
def test_entry_points_refuse(i):
    ta.refuse(CTS_REFUSALS, i, _good, "lg_train_cts", abi.LgTrainCTSPlan)


def test_entry_points_refuse_null_descriptors_and_ignore_the_history_gradients():
    lib = abi.load_lib()
    assert lib.lg_train_cts_plan(None, C.byref(abi.LgTrainCTSPlan())) != 0 and b"lg_train_cts_plan: null descriptor" in lib.lg_last_error()
    assert lib.lg_train_cts_plan(C.byref(_good()), None) != 0 and b"lg_train_cts_plan: null plan" in lib.lg_last_error()
    for d in ("_forward", "_backward"):
        assert getattr(lib, "lg_train_cts" + d)(None, None) != 0 and ("lg_train_cts" + d + ": null descriptor").encode() in lib.lg_last_error()
    assert lib.lg_train_cts_backward(C.byref(_good(backward=False)), None) != 0          # a forward-only descriptor is what backward refuses
    # the RL descriptor leaves the history encoder's gradient members null and the pass does not ask for them: with every other member
    # good, the first thing a backward misses on this machine is the device
    a = _good()
    assert all(not a.chain[HIS].layer[i].grad_weight and not a.chain[HIS].layer[i].grad_bias for i in range(3))
    assert all(a.chain[c].layer[i].grad_weight for c in (PRI, ACT, CRI) for i in range(3))
    assert lib.lg_train_cts_plan(C.byref(a), C.byref(abi.LgTrainCTSPlan())) == 0
    if not torch.cuda.is_available():
        assert lib.lg_train_cts_backward(C.byref(a), None) != 0 and b"grad" not in lib.lg_last_error() and b"null" not in lib.lg_last_error()
    assert "does not fit the 160 KB of LDS" in open(os.path.join(CSRC, "lg_train_cts.hip")).read()


# ---- refusals of the Python surface -------------------------------------------------------------------------------------------------------
class _CTS(nn.Module):
    """O = 4, P = 5, Z = 2, H = 6."""

    def __init__(self, privilege_encoder=None, history_encoder=None, actor=None, critic=None, A=3):
        super().__init__()
        self.actor = actor if actor is not None else nn.Sequential(nn.Linear(6, 8), nn.ELU(), nn.Linear(8, A))
        self.critic = critic if critic is not None else nn.Sequential(nn.Linear(6, 8), nn.ELU(), nn.Linear(8, 1))
        self.privilege_encoder = privilege_encoder if privilege_encoder is not None else nn.Sequential(nn.Linear(5, 4), nn.ELU(), nn.Linear(4, 2))
        self.history_encoder = history_encoder if history_encoder is not None else nn.Sequential(nn.Linear(6, 4), nn.ELU(), nn.Linear(4, 2))
        self.std = nn.Parameter(torch.ones(A))


def test_describe_cts_takes_actor_critic_cts():
    m = _CTS()
    spec = train.describe_cts(m)
    assert isinstance(spec, train.TrainSpecTS)
    assert spec.privilege_encoder.widths == [5, 4, 2] and spec.history_encoder.widths == [6, 4, 2] and spec.actor.widths == [6, 8, 3]
    assert spec.critic.widths == [6, 8, 1] and spec.clip_actions is None and (spec.num_obs, spec.num_latent, spec.num_actions) == (4, 2, 3)
    want = list(m.actor.parameters()) + list(m.critic.parameters()) + list(m.privilege_encoder.parameters()) + [m.std]       # PPO_CTS.rl_params
    assert len(spec.rl_parameters()) == len(want) and all(a is b for a, b in zip(spec.rl_parameters(), want))
    assert all(a is b for a, b in zip(spec.encoder_parameters(), m.history_encoder.parameters()))
    assert train.describe_cts(_CTS(actor=nn.Sequential(nn.Linear(6, 8), nn.ELU(), nn.Linear(8, 3), nn.Hardtanh(-0.5, 0.5)))).clip_actions == 0.5
    # FusedTrainPassTS keeps accepting what it accepted, and points at the new class
    assert train.describe_ts(m).actor.widths == [6, 8, 3]
    assert "PPO_TS's update only" in train.FusedTrainPassTS.__doc__ and "FusedTrainPassCTS" in train.FusedTrainPassTS.__doc__
    for cls in (train.FusedTrainPassCTS,):
        assert "PPO_CTS" in cls.__doc__ and "history encoder's .grad is left as it was" in cls.__doc__


def _break(f, **kw):
    m = _CTS(**kw)
    f(m)
    return m


def _tcn():
    return nn.Sequential(nn.Conv1d(1, 3, 5, padding=2), nn.Conv1d(3, 3, 5, stride=2, padding=2), nn.Flatten(), nn.Linear(9, 4), nn.ELU(), nn.Linear(4, 2))


SURFACE_REFUSALS = [
    (lambda: _CTS(history_encoder=_tcn()), r"FusedTrainPassCTS: history_encoder\[0\] is Conv1d; only Linear and ELU are built"),
    (lambda: _CTS(history_encoder=nn.Sequential(nn.Flatten(), nn.Linear(6, 2))), r"FusedTrainPassCTS: history_encoder\[0\] is Flatten"),
    (lambda: _CTS(history_encoder=nn.Sequential(nn.Linear(6, 4), nn.ELU(), nn.Linear(4, 3))),
     r"FusedTrainPassCTS: history_encoder ends at 3 columns, privilege_encoder at 2: the latent widths differ"),
    (lambda: _break(lambda m: setattr(m, "estimator", nn.Sequential(nn.Linear(5, 2)))),
     r"FusedTrainPassCTS: the module has \.estimator \(ActorCriticEE\) beside its encoders; only ActorCriticCTS is built"),
    (lambda: _break(lambda m: setattr(m, "history_encoder", None)), r"FusedTrainPassCTS: the module has no \.history_encoder; ActorCriticCTS has"),
    (lambda: _break(lambda m: delattr(m, "privilege_encoder")), r"FusedTrainPassCTS: the module has no \.privilege_encoder"),
    (lambda: _CTS(actor=nn.Sequential(nn.Linear(2, 8), nn.ELU(), nn.Linear(8, 3))),
     r"FusedTrainPassCTS: actor\[0\] takes 2 inputs, but \[obs \| latent\] has O \+ 2 columns with O >= 1"),
    (lambda: _break(lambda m: setattr(m, "vae", nn.Sequential(nn.Linear(5, 2)))), r"FusedTrainPassCTS: the module has \.vae \(ActorCriticDreamWaQ\) beside"),
    (lambda: _break(lambda m: setattr(m, "memory_a", nn.LSTM(5, 2))), r"FusedTrainPassCTS: the module has \.memory_a \(ActorCriticRecurrent\) beside"),
    (lambda: _break(lambda m: setattr(m, "is_recurrent", True)), r"FusedTrainPassCTS: the module is recurrent"),
    (lambda: _break(lambda m: delattr(m, "critic")), r"FusedTrainPassCTS: the module has no \.critic"),
    (lambda: _CTS(privilege_encoder=nn.Sequential(nn.Linear(5, 4), nn.Tanh(), nn.Linear(4, 2))), r"FusedTrainPassCTS: privilege_encoder\[1\] is Tanh; only Linear and ELU"),
    (lambda: _CTS(history_encoder=nn.GRU(6, 2)), r"FusedTrainPassCTS: history_encoder is GRU, expected an nn\.Sequential"),
    (lambda: _CTS(critic=nn.Sequential(nn.Linear(6, 8), nn.ReLU(), nn.Linear(8, 1))), r"FusedTrainPassCTS: critic\[1\] is ReLU"),
    (lambda: _break(lambda m: setattr(m, "std", nn.Parameter(torch.ones(4)))), r"FusedTrainPassCTS: std has shape \(4,\), the actor has 3 outputs"),
]


@pytest.mark.parametrize("i", range(len(SURFACE_REFUSALS)))
def test_describe_cts_refuses(i):
    make, msg = SURFACE_REFUSALS[i]
    with pytest.raises(ValueError, match=msg):
        train.describe_cts(make())


def test_the_surface_refuses_devices_and_tensors():
    with pytest.raises(ValueError, match=r"FusedTrainPassCTS: the module is on cpu, not on a HIP device \(there is no CPU path\)"):
        train.FusedTrainPassCTS(_CTS())
    with pytest.raises(ValueError, match=r"FusedTrainPassCTS: privilege_encoder\[0\]\.weight is on cpu, not on cuda:0"):
        train.describe_cts(_CTS(), torch.device("cuda:0"))
    spec = train.describe_cts(_CTS())
    ok = dict(to=torch.zeros(4, 4), tp=torch.zeros(4, 5), so=torch.zeros(3, 4), sh=torch.zeros(3, 6), c=torch.zeros(9, 6), mt=torch.zeros(4, 3), st=torch.zeros(4, 3),
              ms=torch.zeros(3, 3), ss=torch.zeros(3, 3), v=torch.zeros(9, 1))
    call = lambda **kw: train.cts_args(spec, *[{**ok, **kw}[k] for k in ("to", "tp", "so", "sh", "c", "mt", "st", "ms", "ss", "v")], None)
    a = call()
    assert (a.n_teacher, a.n_student, a.n_critic, a.n_obs, a.clip_on) == (4, 3, 9, 4, 0)
    for kw, msg in ((dict(to=torch.zeros(4, 5)), r"FusedTrainPassCTS: teacher_obs must be \(4, 4\) float32"),
                    (dict(tp=torch.zeros(3, 5)), r"FusedTrainPassCTS: teacher_privileged_obs must be \(4, 5\) float32"),
                    (dict(so=torch.zeros(3, 4, dtype=torch.float64)), r"student_obs must be \(3, 4\) float32"),
                    (dict(sh=torch.zeros(4, 6)), r"student_obs_history must be \(3, 6\)"), (dict(c=torch.zeros(9, 7)), r"critic_obs must be \(9, 6\)"),
                    (dict(to=torch.zeros(0, 4)), r"teacher_obs must be a \(B, 4\) float32 tensor with B >= 1"),
                    (dict(so=torch.zeros(4)), r"student_obs must be a \(B, 4\) float32 tensor with B >= 1"),
                    (dict(c=None), r"critic_obs must be a \(B, 6\) float32 tensor with B >= 1"),
                    (dict(ms=torch.zeros(4, 3)), r"student mu must be \(3, 3\)"), (dict(st=torch.zeros(4, 2)), r"teacher sigma must be \(4, 3\)"),
                    (dict(v=torch.zeros(4, 1)), r"values must be \(9, 1\)")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    wide = torch.zeros(9, 16)                                                 # strided views are addressed in place
    a = call(to=wide[:4, 1:5], so=wide[:3, 6:10], c=wide[:, 10:16])
    assert (a.chain[ACT].input, a.chain[ACT].in_stride, a.student_obs, a.student_obs_stride, a.chain[CRI].in_stride) == \
        (wide.data_ptr() + 4, 16, wide.data_ptr() + 24, 16, 16)
    # the encoder pass's descriptor in the new owner's name
    with pytest.raises(ValueError, match=r"FusedTrainPassCTS: obs_history must be \(3, 6\)"):
        train.enc_args(spec, torch.zeros(3, 7), torch.zeros(3, 5), torch.ones(3, 1), torch.zeros(()), None, owner="FusedTrainPassCTS")


# ---- the case table -----------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_the_edges():
    R = cc.R
    assert R == 32
    rows = {(c["Bt"], c["Bs"], c["Bc"]) for c in cc.CASES.values() if c["net"] == "fixture"}
    assert {(1, 1, 1), (R - 1, 1, R), (R, R + 1, 2 * R + 1), (R + 1, R - 1, 1), (1, 2 * R + 1, 3 * R + 3), (7, 9, 16)} <= rows
    f = cc.NETS["fixture"]
    c = cc.CASES["fixture_straddle"]
    p = cc.restated_plan_cts(c["Bt"], c["Bs"], c["Bc"], *f)
    b = c["Bt"] + c["Bs"]
    assert any(S > 1 and b % per and c["Bt"] % per and c["Bt"] < per for S, per in zip(p["slices"][1], p["slice_rows"][1]))      # slice 0 holds both groups
    assert b == sup.smallest_ragged_b(lambda n: dict(slices=[cc.restated_plan_cts(max(n, 2) - 1, 1, 1, *f)["slices"][1]],
                                                     slice_rows=[cc.restated_plan_cts(max(n, 2) - 1, 1, 1, *f)["slice_rows"][1]]))
    c = cc.CASES["fixture_priv_ragged"]
    p = cc.restated_plan_cts(c["Bt"], c["Bs"], c["Bc"], *f)
    assert any(S > 1 and c["Bt"] % per for S, per in zip(p["slices"][0], p["slice_rows"][0])) and c["Bt"] == cc.ragged_teacher_rows("fixture")
    from tests import train_edges as te
    assert cc.NETS["ts_r16"][0] == te.ROWS["ts_r16"]["priv"] and cc.NETS["ts_r8_z"][3] == te.ROWS["ts_r8_z"]["hist"]
    assert (cc.tile_of("ts_r16"), cc.tile_of("ts_r8_z")) == (16, 8)
    assert {cc.NETS[n][0][-1] for n in ("ts_r16", "ts_r8_z")} == {37, 65} and all(cc.NETS[n][1][0] % 4 for n in ("ts_r16", "ts_r8_z"))
    assert (cc.NETS["ts_r8_z"][1][0] - 65) % 4 and (cc.NETS["ts_r16"][1][0] - 37) % 16          # O off a multiple of 4; the latent across 16-column tiles
    depths = {(len(cc.NETS[f"enc_{a}_{b}"][0]) - 1, len(cc.NETS[f"enc_{a}_{b}"][3]) - 1) for a, b in cc.ENC_DEPTHS}
    assert {d for pair in depths for d in pair} == {1, 2, 3, 4}
    assert {tuple(cc.restated_plan_cts(5, 5, 5, *cc.NETS[f"enc_{a}_{b}"])["enc_first_buffer"]) for a, b in cc.ENC_DEPTHS} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    g = cc.CASES["go2_cts"]
    assert (g["Bt"], g["Bs"], g["Bc"]) == (24, 9, 33)
    assert cc.NETS["go2_cts"] == ([99, 256, 128, 99], [144, 512, 256, 128, 12], [885, 1024, 256, 128, 1], [900, 256, 128, 99])
    assert all(p[-1] == h[-1] and a[0] > p[-1] for p, a, _, h in cc.NETS.values())
    clips = [cc.make_inputs(n)["clip"] for n in ("fixture_odd_teacher", "fixture_above_tile")]
    assert clips[0] is not None and clips[1] is None                                              # with and without a Hardtanh
    x = cc.make_inputs("fixture_straddle")
    pre = cc.rl_forward(dict(x, clip=None))
    pre = np.concatenate([pre["mu_t"], pre["mu_s"]])
    assert 0.1 <= (np.abs(pre) >= x["clip"]).mean() <= 0.9 and np.abs(np.abs(pre) - x["clip"]).min() >= 1e-3

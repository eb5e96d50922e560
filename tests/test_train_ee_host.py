"""Host side of the explicit-estimator learner passes (hcr_genesis_lr_cl_amd/train.py's FusedTrainPassEE, include/lgtrainee.h): the ctypes
mirror against the header, the exports and the translation unit, the float64 restatement of tests/train_ee_cases.py against the golden
fixture of the reference's own PPO_EE.update() (tests/golden/ppo_ee_train.npz) and against torch float64 autograd, the plans of
lg_train_ee_plan / lg_train_est_plan against the restated rules, every refusal of the entry points and of describe_ee, and the coverage of
the case table.  No GPU needed: nothing is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from hcr_genesis_lr_cl_amd import abi, train
from tests import ppo_loss_cases as pc
from tests import train_abi as ta
from tests import train_cases as tc
from tests import train_ee_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lgtrainee.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ppo_ee_train.npz")
CSRC = os.path.join(ROOT, "hcr_genesis_lr_cl_amd", "csrc")
TILE_ROUTINES = ("stage_rows", "copy_out", "fwd_tile", "bwd_tile", "wgrad_wave", "combine_layer", "lds_stride", "slice_rule")
PASS_ROUTINES = ("chain_forward", "chain_from_rows", "store_sigma", "seed_last_g", "bwd_layer", "chain_backward", "mse_tile", "loss_finalize",
                 "wgrad_job", "combine_all", "check_desc", "plan_chain", "plan_layout", "plan_out", "bind_chain", "check_ws", "bind_heads", "done",
                 "raise_lds", "launch_tile", "launch_backward")
DEFINES = r"^(?:template <[^>]*> *)?(?:static |inline |__device__ |__forceinline__ )+[\w ]*[ *]"       # a definition at file scope of ...


# ---- the structs --------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header():
    structs = [("LgTrainEEArgs", abi.LgTrainEEArgs), ("LgTrainEstArgs", abi.LgTrainEstArgs), ("LgTrainEEPlan", abi.LgTrainEEPlan),
               ("LgTrainChain", abi.LgTrainChain)]
    consts = dict(LG_TRAIN_EE_CHAINS=abi.TRAIN_EE_CHAINS, LG_TRAIN_EE_ESTIMATOR=abi.TRAIN_EE_ESTIMATOR, LG_TRAIN_EE_ACTOR=abi.TRAIN_EE_ACTOR,
                  LG_TRAIN_EE_CRITIC=abi.TRAIN_EE_CRITIC, LG_TRAIN_EE_THREADS=abi.TRAIN_EE_THREADS, LG_TRAIN_EE_TARGET_JOBS=abi.TRAIN_EE_TARGET_JOBS, LG_POLICY_MAX_LAYERS=abi.POLICY_MAX_LAYERS)
    ta.check_layout(HEADER, structs, consts)
    assert ec.RED_BYTES == abi.TRAIN_EE_THREADS * 8 and ec.TARGET_JOBS == abi.TRAIN_EE_TARGET_JOBS


def test_library_exports_the_entry_points():
    declared = ta.check_exports(HEADER, abi.TRAIN_EE_EXPORTS, "lg_train_ee", ["lg_train_tiles.h", "lg_train_pass.h"])
    assert declared == {"lg_train_ee_plan", "lg_train_ee_forward", "lg_train_ee_backward", "lg_train_est_plan", "lg_train_est_forward",
                        "lg_train_est_backward"}
    from hcr_genesis_lr_cl_amd import build
    assert any(u[0] == "lg_train" and "lg_train_tiles.h" in u[3] and "lg_train_pass.h" in u[3] for u in build.units())
    assert "TRAIN_EE_EXPORTS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()          # the build's export check covers the list
    # one copy of the layer routines and of the pass routines: every unit reaches both headers, none defines any of them
    units = {u: open(os.path.join(CSRC, u)).read() for u in ("lg_train.hip", "lg_train_ee.hip", "lg_train_ts.hip")}
    for header, fns in (("lg_train_tiles.h", TILE_ROUTINES), ("lg_train_pass.h", PASS_ROUTINES)):
        text = open(os.path.join(CSRC, header)).read()
        other = open(os.path.join(CSRC, "lg_train_pass.h" if header == "lg_train_tiles.h" else "lg_train_tiles.h")).read()
        for fn in fns:
            assert len(re.findall(DEFINES + fn + r"\(", text, flags=re.M)) == 1, fn
            assert not re.findall(DEFINES + fn + r"\(", other, flags=re.M), fn
            for unit, src in units.items():
                assert '#include "lg_train_pass.h"' in src and not re.findall(DEFINES + fn + r"\(", src, flags=re.M), (unit, fn)
    assert not any(re.findall(DEFINES + r"plan_rest\(", src, flags=re.M) for src in units.values())      # plan_layout has taken its place
    assert '#include "lg_train_tiles.h"' in open(os.path.join(CSRC, "lg_train_pass.h")).read()
    for unit in ("lg_train_ee.hip", "lg_train_tiles.h", "lg_train_pass.h"):
        assert "atomic" not in open(os.path.join(CSRC, unit)).read().lower()                    # determinism is the house rule


# ---- the restatement against the fixture ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return ec.load_fixture(FIXTURE)


def test_fixture_is_the_tiny_actor_critic_ee(fx):
    assert fx["est"] == [7, 8, 4, 3] and fx["actor"] == [10, 16, 8, 3] and fx["critic"] == [9, 16, 8, 1]
    assert (fx["est"], fx["actor"], fx["critic"]) == ec.NETS["fixture"]
    assert fx["cfg"]["steps"] == 6 and fx["cfg"]["est_steps"] == 12 and fx["cfg"]["est_epochs"] == 2
    assert fx["names"][0] == "std" and fx["rl_names"][-1] == "std" and all(n.startswith("estimator") for n in fx["est_names"])
    assert fx["rl_names"] == [f"{c}.{i}.{k}" for c in ("actor", "critic") for i in (0, 2, 4) for k in ("weight", "bias")] + ["std"]
    assert fx["features"].shape == (6, 16, 7) and fx["critic_obs"].shape == (6, 16, 9) and fx["est_terminated"].shape == (12, 16, 1)
    clip = fx["cfg"]["clip_actions"]
    for s in range(6):
        x = ec.fixture_inputs(fx, fx["init"] if s == 0 else fx["params"][s - 1], rl_step=s)
        pre = ec.rl_forward(dict(x, clip=None))["mu"]
        assert 0.1 <= (np.abs(pre) >= clip).mean() <= 0.9 and np.abs(np.abs(pre) - clip).min() >= 1e-4
    for t in fx["est_terminated"]:
        assert 0 < t.sum() < t.size and set(np.unique(t)) <= {0.0, 1.0}


def test_restatement_matches_the_reference_update(fx):
    """Every RL step and every estimator step of the reference's PPO_EE.update(): the restated passes, the loss head's restatement and the
    restated optimizer reproduce outputs, losses, gradients, norms, rates and every parameter to 1e-12.  That the parameters agree while
    the RL pass gives the estimator no gradient is the proof that dropping it is harmless."""
    cfg = fx["cfg"]
    params = {k: v.copy() for k, v in fx["init"].items()}
    state, lr = {}, cfg["lr0"]
    for s in range(cfg["steps"]):
        x = ec.fixture_inputs(fx, params, rl_step=s)
        fw = ec.rl_forward(x)
        for k in ("mu", "sigma", "values"):
            assert tc.max_err(fw[k], fx[k][s]) <= 1e-12, (s, k)
        r = pc.restate(ec.fixture_loss_inputs(fx, s, fw["mu"], fw["sigma"], fw["values"]), True, False, cfg["entropy_coef"], clip=cfg["clip_param"],
                       value_loss_coef=cfg["value_loss_coef"])
        assert abs(float(r["loss"]) - fx["loss"][s]) <= 1e-12 and abs(float(r["kl"][0]) - fx["kl"][s]) <= 1e-12
        x.update(grad_mu=r["grad_mu"][0], grad_sigma=r["grad_sigma"][0], grad_values=r["grad_values"])
        grads = ec.rl_backward(x)
        for name, g, want in zip(fx["rl_names"], grads, fx["grads"][s]):
            assert g.shape == want.shape and tc.max_err(g, want) <= 1e-12, (s, name)
        step = ta.adam(x["rl_params"], grads, state, lr, cfg, kl=float(r["kl"][0]))
        lr = step["lr"]
        assert lr == fx["lr"][s] and abs(step["grad_norm"] - fx["grad_norm"][s]) <= 1e-12
        params.update(zip(fx["rl_names"], step["params"]))
        for n in fx["names"]:                                   # the estimator's parameters stay: the RL step does not touch them
            assert tc.max_err(params[n], fx["params"][s][n]) <= 1e-12, (s, n)
    state = {}
    for s in range(cfg["est_steps"]):
        x = ec.fixture_inputs(fx, params, est_step=s)
        e = ec.est_pass(x)
        assert abs(float(e["loss"]) - fx["est_loss"][s]) <= 1e-12
        for name, g, want in zip(fx["est_names"], e["grads"], fx["est_grads"][s]):
            assert g.shape == want.shape and tc.max_err(g, want) <= 1e-12, (s, name)
        step = ta.adam(x["est_params"], e["grads"], state, cfg["estimator_lr"], cfg)
        assert abs(step["grad_norm"] - fx["est_grad_norm"][s]) <= 1e-12
        params.update(zip(fx["est_names"], step["params"]))
        for n in fx["names"]:
            assert tc.max_err(params[n], fx["est_params"][s][n]) <= 1e-12, (s, n)


HOST_CASES = ["fixture_b33", "fixture_b257", "one_four_b31", "go2_ee_b31", "tron1_pf_ee_b1", "f1_n1_b33", "f5_n17_b33", "f65_n4_b33", "f16_n65_b33"]


@pytest.mark.parametrize("case", HOST_CASES)
def test_restatement_matches_torch_float64_autograd(case):
    x = ec.make_inputs(case)
    ref = ec.torch_passes(x, torch.float64)
    fw, e = ec.rl_forward(x), ec.est_pass(x)
    rel = lambda a, b: tc.max_err(a, b) <= 1e-12 * max(1.0, np.abs(b).max())
    assert all(rel(fw[k], ref[k]) for k in ("mu", "sigma", "values")) and rel(e["loss"], ref["loss"])
    for name, g, want in zip(ec.rl_names(x["actor"], x["critic"]), ec.rl_backward(x), ref["rl_grads"]):
        assert g.shape == want.shape and rel(g, want), name
    for name, g, want in zip(ec.est_names(x["est"]), e["grads"], ref["est_grads"]):
        assert g.shape == want.shape and rel(g, want), name
    for g, want in zip(ec.rl_backward(x, slices=12), ec.rl_backward(x)):
        assert rel(g, want)
    # autograd does send a gradient into the estimator from the RL cotangents: the one the reference discards and the pass does not form
    assert any(np.abs(g).max() > 0 for g in ref["est_rl_grads"])
    # the upstream scalar scales the estimator's gradients, not the loss
    twice = ec.est_pass(x, upstream=2.0 * float(x["upstream"]))
    assert twice["loss"] == e["loss"] and all(rel(a, 2.0 * b) for a, b in zip(twice["grads"], e["grads"]))
    # the module helper computes the same passes (what the GPU file hands to FusedTrainPassEE)
    m = ec.Module(x, dtype=torch.float64)
    d = lambda k: torch.as_tensor(x[k]).double()
    mu, sigma, values = m(d("features"), d("critic_obs"))
    assert rel(mu.detach().numpy(), fw["mu"]) and rel(values.detach().numpy(), fw["values"])
    assert rel(m.estimator_loss(d("features"), d("labels"), d("terminated")).detach().numpy(), e["loss"])


def test_masked_rows_and_the_mask_as_a_multiplication():
    x = ec.make_inputs("fixture_b33")
    off = dict(x, terminated=np.zeros_like(x["terminated"]))
    e = ec.est_pass(off)
    assert e["loss"] == 0.0 and all((g == 0).all() for g in e["grads"])
    row = int(np.flatnonzero(x["terminated"][:, 0] == 0)[0])
    bad = dict(x, features=x["features"].copy())
    bad["features"][row, 1] = np.nan
    assert np.isnan(ec.est_pass(bad)["loss"]) and np.isnan(ec.torch_passes(bad, torch.float64)["loss"])        # NaN * 0, in both


# ---- the plans ----------------------------------------------------------------------------------------------------------------------------
PLAN_BATCHES = (1, 4, 31, 33, 64, 65, 127, 128, 129, 130, 257, 2048, 4097, 24576)


@pytest.mark.parametrize("net", ["fixture", "go2_ee", "tron1_pf_ee", "one_four", "f1_n1", "f65_n65", "f17_n4"])
def test_plans_against_the_restated_rules(net):
    est, actor, critic = ec.NETS[net]
    for b in PLAN_BATCHES:
        p, want = train.plan_ee(b, est, actor, critic), ec.restated_plan_ee(b, est, actor, critic)
        assert (p.row_tile, p.lds_bytes, p.workspace_floats, p.weight_jobs, p.std_p_off, p.cat_off, p.est_first_buffer) == \
            (want["row_tile"], want["lds_bytes"], want["workspace_floats"], want["weight_jobs"], want["std_p_off"], 0, want["est_first_buffer"]), (net, b)
        assert (p.std_slices, p.std_slice_rows) == want["std"] and (p.gl_off, p.partial_off, p.loss_tiles) == (-1, -1, 0)
        assert all(v == -1 for k in ("h_off", "g_off", "p_off") for v in getattr(p, k)[abi.TRAIN_EE_ESTIMATOR])
        for i, (ci, c) in enumerate(((abi.TRAIN_EE_ACTOR, actor), (abi.TRAIN_EE_CRITIC, critic))):
            n = len(c) - 1
            for k in ("slices", "slice_rows", "h_off", "g_off", "p_off"):
                assert list(getattr(p, k)[ci])[:n] == want[k][i], (net, b, k)
            assert all(v == -1 for k in ("h_off", "g_off", "p_off") for v in list(getattr(p, k)[ci])[n:])
        q, want = train.plan_est(b, est), ec.restated_plan_est(b, est)
        assert (q.row_tile, q.lds_bytes, q.workspace_floats, q.weight_jobs, q.gl_off, q.partial_off, q.loss_tiles) == \
            (want["row_tile"], want["lds_bytes"], want["workspace_floats"], want["weight_jobs"], want["gl_off"], want["partial_off"], want["loss_tiles"]), (net, b)
        n = len(est) - 1
        for k in ("slices", "slice_rows", "h_off", "g_off", "p_off"):
            assert list(getattr(q, k)[0])[:n] == want[k][0], (net, b, k)
        assert q.partial_off % 2 == 0 and (q.cat_off, q.std_p_off, q.std_slices) == (-1, -1, 0)


def test_plan_edges():
    for net in ec.REAL:                                         # the row tile of both shipped configurations is 16
        est, actor, critic = ec.NETS[net]
        p = train.plan_ee(24576, est, actor, critic)
        assert p.row_tile == 16 and p.lds_bytes <= tc.LDS_BYTES < 2 * p.lds_bytes
        assert train.plan_est(24576, est).row_tile == 32
    assert train.plan_ee(33, *ec.NETS["fixture"]).est_first_buffer == 0 and train.plan_ee(33, *ec.NETS["f4_n5"]).est_first_buffer == 1
    assert train.plan_ee(33, *ec.NETS["one_four"]).est_first_buffer == 0
    # the concatenated input counts: an actor input of 2048 beside narrow chains takes the 8-row tile
    assert train.plan_ee(100, [2040, 8, 8], [2048, 2048, 2048, 4], [8, 1]).row_tile == 8


# ---- refusals of the entry points: nothing is enqueued (there is no device here) -----------------------------------------------------------
def _good_ee(backward=True):
    x = ec.make_inputs("fixture_b33")
    m = ec.Module(x)
    spec = train.describe_ee(m)
    t = lambda k: torch.as_tensor(x[k])
    keep = dict(m=m, f=t("features"), c=t("critic_obs"), mu=torch.zeros(33, 3), sigma=torch.zeros(33, 3), values=torch.zeros(33, 1),
                gm=t("grad_mu"), gs=t("grad_sigma"), gv=t("grad_values"), grads=[torch.zeros_like(p) for p in spec.rl_parameters()])
    keep["ws"] = torch.zeros(int(train.plan_ee(33, *ec.NETS["fixture"]).workspace_floats))
    a = train.ee_args(spec, keep["f"], keep["c"], keep["mu"], keep["sigma"], keep["values"], keep["ws"], keep["grads"] if backward else None,
                      keep["gm"], keep["gs"], keep["gv"])
    a._keep = keep
    return a


def _good_est(backward=True):
    x = ec.make_inputs("fixture_b33")
    m = ec.Module(x)
    spec = train.describe_ee(m)
    t = lambda k: torch.as_tensor(x[k])
    keep = dict(m=m, f=t("features"), y=t("labels"), t=t("terminated"), loss=torch.zeros(()), up=torch.ones(1),
                grads=[torch.zeros_like(p) for p in spec.estimator_parameters()])
    keep["ws"] = torch.zeros(int(train.plan_est(33, ec.NETS["fixture"][0]).workspace_floats))
    a = train.est_args(spec, keep["f"], keep["y"], keep["t"], keep["loss"], keep["ws"], keep["grads"] if backward else None, keep["up"])
    a._keep = keep
    return a


# (mutation, message, which entry points refuse it: p plan, f forward, b backward)
EE_REFUSALS = [
    (ta.set_path(("n_rows",), 0), b"n_rows = 0 < 1", "pfb"),
    (ta.set_path(("chain", 0, "n_layers"), 0), b"chain[0] (estimator).n_layers = 0 is outside [1, 4]", "pfb"),
    (ta.set_path(("chain", 1, "n_layers"), 5), b"chain[1] (actor).n_layers = 5 is outside [1, 4]", "pfb"),
    (ta.set_path(("chain", 2, "layer", 1, "n_in"), 15), b"chain[2] (critic).layer[1].n_in = 15, but its input has 16 columns", "pfb"),
    (ta.set_path(("chain", 0, "layer", 2, "n_out"), 0), b"chain[0] (estimator).layer[2].n_out = 0 is outside [1, 2048]", "pfb"),
    (ta.set_path(("chain", 2, "layer", 0, "n_in"), 2049), b"chain[2] (critic).layer[0].n_in = 2049 is outside [1, 2048]", "pfb"),
    (ta.set_path(("chain", 1, "layer", 0, "n_in"), 11), b"chain[1] (actor).layer[0].n_in = 11, but [features | estimator output] has 7 + 3 columns", "pfb"),
    (ta.set_path(("chain", 0, "input"), None), b"chain[0] (estimator).input is null", "fb"),
    (ta.set_path(("chain", 2, "input"), None), b"chain[2] (critic).input is null", "fb"),
    (ta.set_path(("chain", 0, "in_stride"), 6), b"chain[0] (estimator).in_stride = 6 is below its width 7", "fb"),
    (ta.set_path(("chain", 2, "in_stride"), 8), b"chain[2] (critic).in_stride = 8 is below its width 9", "fb"),
    (ta.set_path(("chain", 0, "layer", 1, "weight"), None), b"chain[0] (estimator).layer[1].weight is null", "fb"),
    (ta.set_path(("chain", 1, "layer", 0, "bias"), None), b"chain[1] (actor).layer[0].bias is null", "fb"),
    (ta.set_path(("chain", 1, "layer", 2, "grad_weight"), None), b"chain[1] (actor).layer[2].grad_weight is null", "b"),
    (ta.set_path(("chain", 2, "layer", 1, "grad_bias"), None), b"chain[2] (critic).layer[1].grad_bias is null", "b"),
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
EST_REFUSALS = [
    (ta.set_path(("n_rows",), -2), b"n_rows = -2 < 1", "pfb"),
    (ta.set_path(("chain", "n_layers"), 5), b"chain (estimator).n_layers = 5 is outside [1, 4]", "pfb"),
    (ta.set_path(("chain", "layer", 1, "n_in"), 9), b"chain (estimator).layer[1].n_in = 9, but its input has 8 columns", "pfb"),
    (ta.set_path(("chain", "layer", 0, "n_out"), 4000), b"chain (estimator).layer[0].n_out = 4000 is outside [1, 2048]", "pfb"),
    (ta.set_path(("chain", "input"), None), b"chain (estimator).input is null", "fb"),
    (ta.set_path(("chain", "in_stride"), 3), b"chain (estimator).in_stride = 3 is below its width 7", "fb"),
    (ta.set_path(("chain", "layer", 2, "weight"), None), b"chain (estimator).layer[2].weight is null", "fb"),
    (ta.set_path(("chain", "layer", 0, "bias"), None), b"chain (estimator).layer[0].bias is null", "fb"),
    (ta.set_path(("chain", "layer", 0, "grad_weight"), None), b"chain (estimator).layer[0].grad_weight is null", "b"),
    (ta.set_path(("chain", "layer", 2, "grad_bias"), None), b"chain (estimator).layer[2].grad_bias is null", "b"),
    (ta.set_path(("labels",), None), b"labels is null", "fb"), (ta.set_path(("mask",), None), b"mask is null", "fb"),
    (ta.set_path(("labels_stride",), 2), b"labels_stride = 2 is below its width 3", "fb"),
    (ta.set_path(("mask_stride",), 0), b"mask_stride = 0 is below its width 1", "fb"),
    (ta.set_path(("loss",), None), b"loss is null", "f"), (ta.set_path(("upstream",), None), b"upstream is null", "b"),
    (ta.set_path(("workspace",), None), b"workspace is null", "fb"),
    (lambda a: setattr(a, "workspace", a.workspace + 4), b"workspace is not 8-byte aligned", "fb"),
    (ta.set_path(("workspace_capacity",), 10), b"workspace_capacity = 10 floats is below the plan's", "fb"),
]


@pytest.mark.parametrize("i", range(len(EE_REFUSALS)))
def test_rl_entry_points_refuse(i):
    ta.refuse(EE_REFUSALS, i, _good_ee, "lg_train_ee", abi.LgTrainEEPlan)


@pytest.mark.parametrize("i", range(len(EST_REFUSALS)))
def test_estimator_entry_points_refuse(i):
    ta.refuse(EST_REFUSALS, i, _good_est, "lg_train_est", abi.LgTrainEEPlan)


def test_entry_points_refuse_null_descriptors_and_the_lds():
    lib = abi.load_lib()
    for fn, good in (("lg_train_ee", _good_ee), ("lg_train_est", _good_est)):
        plan = getattr(lib, fn + "_plan")
        assert plan(None, C.byref(abi.LgTrainEEPlan())) != 0 and (fn + "_plan: null descriptor").encode() in lib.lg_last_error()
        assert plan(C.byref(good()), None) != 0 and (fn + "_plan: null plan").encode() in lib.lg_last_error()
        for d in ("_forward", "_backward"):
            assert getattr(lib, fn + d)(None, None) != 0 and (fn + d + ": null descriptor").encode() in lib.lg_last_error()
        a = good(backward=False)                                              # a forward-only descriptor is what backward refuses
        assert getattr(lib, fn + "_backward")(C.byref(a), None) != 0
    # widths within the limit never exceed the LDS at 8 rows, with the loss tree's 2 KB too; the refusal is pinned where it would start
    assert 8 * 2 * tc.lds_stride(abi.POLICY_MAX_WIDTH) * 4 + ec.RED_BYTES <= tc.LDS_BYTES
    assert "does not fit the 160 KB of LDS" in open(os.path.join(CSRC, "lg_train_pass.h")).read()
    # the RL backward leaves the estimator's gradient members alone: null ones are taken
    a = _good_ee()
    assert all(not a.chain[0].layer[i].grad_weight for i in range(3))
    assert lib.lg_train_ee_plan(C.byref(a), C.byref(abi.LgTrainEEPlan())) == 0


# ---- refusals of the Python surface -------------------------------------------------------------------------------------------------------
class _EE(nn.Module):
    def __init__(self, estimator=None, actor=None, critic=None, A=3):
        super().__init__()
        self.actor = actor if actor is not None else nn.Sequential(nn.Linear(7, 8), nn.ELU(), nn.Linear(8, A), nn.Hardtanh(-1.0, 1.0))
        self.critic = critic if critic is not None else nn.Sequential(nn.Linear(6, 8), nn.ELU(), nn.Linear(8, 1))
        self.estimator = estimator if estimator is not None else nn.Sequential(nn.Linear(5, 4), nn.ELU(), nn.Linear(4, 2))
        self.std = nn.Parameter(torch.ones(A))


def test_describe_ee_takes_actor_critic_ee():
    spec = train.describe_ee(_EE())
    assert spec.estimator.widths == [5, 4, 2] and spec.actor.widths == [7, 8, 3] and spec.critic.widths == [6, 8, 1] and spec.clip_actions == 1.0
    assert (spec.num_features, spec.num_labels, spec.num_actions) == (5, 2, 3)
    assert spec.rl_parameter_names() == ["actor.0.weight", "actor.0.bias", "actor.1.weight", "actor.1.bias", "critic.0.weight", "critic.0.bias",
                                         "critic.1.weight", "critic.1.bias", "std"]
    assert spec.estimator_parameter_names() == ["estimator.0.weight", "estimator.0.bias", "estimator.1.weight", "estimator.1.bias"]
    m = _EE()
    s = train.describe_ee(m)
    assert all(a is b for a, b in zip(s.rl_parameters(), list(m.actor.parameters()) + list(m.critic.parameters()) + [m.std]))     # the reference's order
    assert all(a is b for a, b in zip(s.estimator_parameters(), m.estimator.parameters()))
    with pytest.raises(ValueError, match=r"FusedTrainPass: the module has \.estimator \(ActorCriticEE\)"):      # the plain pass still refuses it
        train.describe(m)


def _break(f, **kw):
    m = _EE(**kw)
    f(m)
    return m


SURFACE_REFUSALS = [
    (lambda: _break(lambda m: setattr(m, "estimator", None)), r"FusedTrainPassEE: the module has no \.estimator"),
    (lambda: _EE(estimator=nn.Sequential(nn.Linear(5, 4), nn.Tanh(), nn.Linear(4, 2))), r"estimator\[1\] is Tanh; only Linear and ELU are built"),
    (lambda: _EE(estimator=nn.Sequential(nn.Linear(5, 4), nn.ELU(), nn.Linear(4, 2), nn.Hardtanh(-1, 1))), r"estimator\[3\] is Hardtanh"),
    (lambda: _EE(estimator=nn.Sequential(nn.Linear(5, 4), nn.ELU(alpha=0.5), nn.Linear(4, 2))), r"estimator\[1\] is ELU\(alpha=0\.5\), only alpha = 1"),
    (lambda: _EE(estimator=nn.Sequential(nn.Linear(5, 4), nn.ELU(), nn.Linear(3, 2))), r"estimator\[2\] takes 3 inputs, the layer before it gives 4"),
    (lambda: _EE(estimator=nn.Sequential(*[nn.Linear(5, 5) for _ in range(5)], nn.Linear(5, 2))), r"estimator has 6 Linear layers, the kernel takes 4"),
    (lambda: _EE(estimator=nn.Sequential(nn.Linear(5, 4000), nn.ELU(), nn.Linear(4000, 2))), r"estimator\[0\] is 5 -> 4000, widths are limited to 2048"),
    (lambda: _EE(estimator=nn.Sequential(nn.Linear(5, 2), nn.ELU())), r"estimator ends in an ELU"),
    (lambda: _EE(estimator=nn.GRU(5, 2)), r"estimator is GRU, expected an nn\.Sequential"),
    (lambda: _EE(estimator=nn.Sequential(nn.Linear(5, 4), nn.ELU(), nn.Linear(4, 3))), r"FusedTrainPassEE: actor\[0\] takes 7 inputs, but \[features \| estimator output\] has 5 \+ 3 columns"),
    (lambda: _EE(actor=nn.Sequential(nn.Linear(7, 8), nn.ELU(), nn.Linear(8, 3), nn.Hardtanh(-1.0, 1.0), nn.ELU())), r"actor\[3\] \(Hardtanh\(-1\.0, 1\.0\)\) must be the symmetric clip behind the actor's last Linear"),
    (lambda: _EE(critic=nn.Sequential(nn.Linear(6, 8), nn.ReLU(), nn.Linear(8, 1))), r"critic\[1\] is ReLU"),
    (lambda: _break(lambda m: setattr(m.estimator[0], "weight", nn.Parameter(torch.zeros(4, 5, dtype=torch.float64)))), r"estimator\[0\]\.weight is torch\.float64"),
    (lambda: _break(lambda m: setattr(m, "std", nn.Parameter(torch.ones(4)))), r"FusedTrainPassEE: std has shape \(4,\), the actor has 3 outputs"),
    (lambda: _break(lambda m: setattr(m, "privilege_encoder", nn.Sequential(nn.Linear(5, 2)))), r"FusedTrainPassEE: the module has \.privilege_encoder \(ActorCriticTS / ActorCriticCTS\) beside \.estimator"),
    (lambda: _break(lambda m: setattr(m, "history_encoder", nn.Sequential(nn.Linear(5, 2)))), r"\.history_encoder \(ActorCriticTS / ActorCriticCTS\) beside"),
    (lambda: _break(lambda m: setattr(m, "vae", nn.Sequential(nn.Linear(5, 2)))), r"\.vae \(ActorCriticDreamWaQ\) beside"),
    (lambda: _break(lambda m: setattr(m, "memory_a", nn.LSTM(5, 2))), r"\.memory_a \(ActorCriticRecurrent\) beside"),
    (lambda: _break(lambda m: setattr(m, "memory_c", nn.LSTM(5, 2))), r"\.memory_c \(ActorCriticRecurrent\) beside"),
    (lambda: _break(lambda m: setattr(m, "is_recurrent", True)), r"FusedTrainPassEE: the module is recurrent"),
    (lambda: _break(lambda m: delattr(m, "critic")), r"FusedTrainPassEE: the module has no \.critic"),
]


@pytest.mark.parametrize("i", range(len(SURFACE_REFUSALS)))
def test_describe_ee_refuses(i):
    make, msg = SURFACE_REFUSALS[i]
    with pytest.raises(ValueError, match=msg):
        train.describe_ee(make())


def test_the_surface_refuses_devices_and_tensors():
    with pytest.raises(ValueError, match=r"FusedTrainPassEE: the module is on cpu, not on a HIP device \(there is no CPU path\)"):
        train.FusedTrainPassEE(_EE())
    with pytest.raises(ValueError, match=r"estimator\[0\]\.weight is on cpu, not on cuda:0"):
        train.describe_ee(_EE(), torch.device("cuda:0"))
    spec = train.describe_ee(_EE())
    ok = dict(f=torch.zeros(4, 5), c=torch.zeros(4, 6), mu=torch.zeros(4, 3), sigma=torch.zeros(4, 3), values=torch.zeros(4, 1))
    call = lambda **kw: train.ee_args(spec, *[{**ok, **kw}[k] for k in ("f", "c", "mu", "sigma", "values")], None)
    assert call().n_rows == 4 and call().chain[abi.TRAIN_EE_ACTOR].input is None
    for kw, msg in ((dict(f=torch.zeros(4, 6)), r"estimator_features must be \(4, 5\) float32"), (dict(c=torch.zeros(3, 6)), r"critic_obs must be \(4, 6\)"),
                    (dict(f=torch.zeros(0, 5)), r"estimator_features must be a \(B, 5\) float32 tensor with B >= 1"), (dict(mu=torch.zeros(4, 2)), r"mu must be \(4, 3\)")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    est = lambda **kw: train.est_args(spec, *[{**dict(f=ok["f"], y=torch.zeros(4, 2), t=torch.ones(4, 1), loss=torch.zeros(())), **kw}[k]
                                              for k in ("f", "y", "t", "loss")], None)
    assert est().n_rows == 4 and est().labels_stride == 2 and est().mask_stride == 1
    for kw, msg in ((dict(y=torch.zeros(4, 3)), r"estimator_labels must be \(4, 2\)"), (dict(t=torch.ones(4)), r"terminated must be \(4, 1\)"),
                    (dict(t=torch.ones(4, 1, dtype=torch.uint8)), r"terminated must be \(4, 1\) float32"), (dict(loss=torch.zeros(2)), r"the loss must be one float32")):
        with pytest.raises(ValueError, match=msg):
            est(**kw)
    wide = torch.zeros(4, 16)                                                 # strided views are addressed in place
    a = est(f=wide[:, 2:7], y=wide[:, 8:10], t=wide[:, 15:16])
    assert (a.chain.input, a.chain.in_stride, a.labels, a.labels_stride, a.mask, a.mask_stride) == \
        (wide.data_ptr() + 8, 16, wide.data_ptr() + 32, 16, wide.data_ptr() + 60, 16)


# ---- the case table -----------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_the_edges():
    nets = {c["net"] for c in ec.CASES.values()}
    assert set(ec.SWEEP) <= nets and len(ec.SWEEP) == 36 and {"fixture", "one_four", "go2_ee", "tron1_pf_ee"} <= nets
    assert ec.NETS["go2_ee"] == ([900, 256, 128, 24], [924, 512, 256, 128, 12], [870, 1024, 256, 128, 1])
    assert ec.NETS["tron1_pf_ee"] == ([310, 256, 128, 17], [327, 512, 256, 128, 6], [1340, 1024, 256, 128, 1])
    assert all(a[0] == e[0] + e[-1] for e, a, _ in ec.NETS.values())
    assert (len(ec.NETS["one_four"][0]) - 1, len(ec.NETS["one_four"][1]) - 1) == (1, 4)
    for net in ("fixture", "one_four") + ec.REAL:
        assert {ec.CASES[f"{net}_b{b}"]["B"] for b in ec.BATCHES} == {1, 31, 33, 257}
    assert max(c["B"] for c in ec.CASES.values()) == 257
    F = {ec.NETS[n][0][0] for n in ec.SWEEP}
    NL = {ec.NETS[n][0][-1] for n in ec.SWEEP}
    assert F == NL == {1, 4, 5, 16, 17, 65} and {f % 4 for f in F} >= {0, 1} and 1 in NL           # the boundary off and on a multiple of 4; NL = 1
    assert any(e[0] < 64 < e[0] + e[-1] for e, _, _ in (ec.NETS[n] for n in ec.SWEEP))              # F + NL across 64
    assert {0, 1} == {ec.restated_plan_ee(33, *ec.NETS[n])["est_first_buffer"] for n in ("fixture", "f4_n5")}
    for net in ec.RAGGED_SLICE_NETS:
        assert 64 < ec.smallest_ragged_b(net) <= 257
    for name in ("fixture_b33", "go2_ee_b31", "f65_n17_b33"):
        x = ec.make_inputs(name)
        pre = ec.rl_forward(dict(x, clip=None))["mu"]
        assert 0.1 <= (np.abs(pre) >= x["clip"]).mean() <= 0.9 and np.abs(np.abs(pre) - x["clip"]).min() >= 1e-3
    x = ec.make_inputs("fixture_b257")
    assert 0.1 <= 1 - x["terminated"].mean() <= 0.6                                                     # masked and unmasked rows


def test_parity_rule_passes_float32_and_catches_a_select_for_the_mask():
    """A float32 numpy evaluation of the restatement passes the rule; an estimator loss averaged over the unmasked rows only misses it."""
    x = ec.make_inputs("fixture_b257")
    r64, r32 = ec.references(x)
    e32 = ec.est_pass(x, np.float32)
    ec.check_parity(ec.named(x, ec.rl_forward(x, np.float32), ec.rl_backward(x, np.float32), e32["loss"], e32["grads"]), r64, r32, "numpy f32")
    e = ec.est_pass(x)
    scale = x["terminated"].size / x["terminated"].sum()
    bad = ec.named(x, ec.rl_forward(x), ec.rl_backward(x), e["loss"] * scale, [g * scale for g in e["grads"]])
    with pytest.raises(AssertionError):
        ec.check_parity(bad, r64, r32, "mean over the unmasked rows")

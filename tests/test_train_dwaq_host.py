"""Host side of the DreamWaQ learner passes (hcr_genesis_lr_cl_amd/train.py's FusedTrainPassDreamWaQ, include/lgtraindwaq.h): the ctypes
mirror against the header, the exports and the translation unit, the float64 restatement of tests/train_dwaq_cases.py against the golden
fixture of the reference's own PPO_DreamWaQ.update() (tests/golden/ppo_dwaq_train.npz) and against torch float64 autograd, the plans of
lg_train_dwaq_plan / lg_train_vae_plan against the restated rules, every refusal of the entry points and of describe_dwaq, the float32
restatement in the kernel's order of sums under half the parity rule, five planted defects that the rule must catch, and the coverage of
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
from tests import train_dwaq_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lgtraindwaq.h")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ppo_dwaq_train.npz")
CSRC = os.path.join(ROOT, "hcr_genesis_lr_cl_amd", "csrc")
ENC, LMU, ACT, CRI, DEC = abi.TRAIN_DWAQ_ENCODER, abi.TRAIN_DWAQ_LATENT_MU, abi.TRAIN_DWAQ_ACTOR, abi.TRAIN_DWAQ_CRITIC, abi.TRAIN_VAE_DECODER


# ---- the structs --------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header():
    structs = [("LgTrainDwaqArgs", abi.LgTrainDwaqArgs), ("LgTrainVaeArgs", abi.LgTrainVaeArgs), ("LgTrainDwaqPlan", abi.LgTrainDwaqPlan),
               ("LgTrainChain", abi.LgTrainChain)]
    consts = dict(LG_TRAIN_DWAQ_CHAINS=abi.TRAIN_DWAQ_CHAINS, LG_TRAIN_DWAQ_ENCODER=ENC, LG_TRAIN_DWAQ_LATENT_MU=LMU,
                  LG_TRAIN_DWAQ_LATENT_VAR=abi.TRAIN_DWAQ_LATENT_VAR, LG_TRAIN_DWAQ_VEL_MU=abi.TRAIN_DWAQ_VEL_MU, LG_TRAIN_DWAQ_VEL_VAR=abi.TRAIN_DWAQ_VEL_VAR,
                  LG_TRAIN_DWAQ_ACTOR=ACT, LG_TRAIN_DWAQ_CRITIC=CRI, LG_TRAIN_DWAQ_HEADS=abi.TRAIN_DWAQ_HEADS, LG_TRAIN_VAE_CHAINS=abi.TRAIN_VAE_CHAINS,
                  LG_TRAIN_VAE_DECODER=DEC, LG_TRAIN_VAE_LOSSES=abi.TRAIN_VAE_LOSSES, LG_TRAIN_DWAQ_THREADS=abi.TRAIN_DWAQ_THREADS,
                  LG_TRAIN_DWAQ_TARGET_JOBS=abi.TRAIN_DWAQ_TARGET_JOBS, LG_POLICY_MAX_LAYERS=abi.POLICY_MAX_LAYERS)
    ta.check_layout(HEADER, structs, consts)
    assert dc.RED_BYTES == abi.TRAIN_DWAQ_THREADS * 8 and dc.TARGET_JOBS == abi.TRAIN_DWAQ_TARGET_JOBS and dc.N_LOSSES == abi.TRAIN_VAE_LOSSES


def test_library_exports_the_entry_points():
    declared = ta.check_exports(HEADER, abi.TRAIN_DWAQ_EXPORTS, "lg_train_dwaq", ["lg_train_tiles.h", "lg_train_pass.h"])
    assert declared == {"lg_train_dwaq_plan", "lg_train_dwaq_forward", "lg_train_dwaq_backward", "lg_train_vae_plan", "lg_train_vae_forward",
                        "lg_train_vae_backward"}
    from hcr_genesis_lr_cl_amd import build
    assert f"{len(build.units())} translation units" in build.__doc__
    assert "TRAIN_DWAQ_EXPORTS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()        # the build's export check covers the list
    assert '"train_dwaq": "lg_train_dwaq.hip"' in open(os.path.join(ROOT, "tools", "register_table.py")).read()
    # one copy of the layer and pass routines: the unit includes the shared header and defines none of them
    src = open(os.path.join(CSRC, "lg_train_dwaq.hip")).read()
    for fn in ("stage_rows", "copy_out", "fwd_tile", "bwd_tile", "wgrad_wave", "combine_layer", "lds_stride", "slice_rule", "chain_forward",
               "chain_backward", "bwd_layer", "seed_last_g", "mse_tile", "loss_finalize", "wgrad_job", "combine_all", "plan_chain", "plan_layout",
               "plan_out", "bind_chain", "bind_heads", "check_ws", "done", "raise_lds", "launch_tile", "launch_backward"):
        assert '#include "lg_train_pass.h"' in src and not re.findall(r"\b(?:void|int|lds_f \*) ?" + fn + r"\(", src), fn
    assert "atomic" not in src.lower()                                                          # determinism is the house rule


# ---- the restatement against the fixture ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    return dc.load_fixture(FIXTURE)


def test_fixture_is_the_tiny_actor_critic_dreamwaq(fx):
    assert (fx["enc"], fx["L"], fx["E"], fx["dec"], fx["actor"], fx["critic"]) == dc.NETS["fixture"]
    cfg = fx["cfg"]
    assert cfg["steps"] == 6 and cfg["vae_steps"] == 12 and cfg["vae_epochs"] == 2 and cfg["kld_weight"] not in (0.0, 1.0) and cfg["var_clip"] == 5.0
    assert fx["rl_names"] == [f"{c}.{i}.{k}" for c in ("actor", "critic") for i in (0, 2, 4) for k in ("weight", "bias")] + ["std"]
    assert fx["vae_names"] == [n for n in fx["names"] if n.startswith("vae.")] and len(fx["vae_names"]) == 20
    assert [n.split(".")[1] for n in fx["vae_names"][6:14:2]] == list(dc.HEADS)
    assert fx["obs"].shape == (6, 16, 7) and fx["obs_history"].shape == (6, 16, 14) and fx["noise"].shape == (6, 16, 5)
    assert fx["vae_history"].shape == (12, 16, 14) and fx["vae_noise"].shape == (12, 16, 5) and fx["vae_losses"].shape == (12, 4)
    for s in range(6):                                           # the VAE steps of a mini-batch see the RL step's histories
        assert all(np.array_equal(fx["vae_history"][2 * s + e], fx["obs_history"][s]) for e in (0, 1))
    for t in fx["vae_terminated"]:
        assert 0 < t.sum() < t.size and set(np.unique(t)) <= {0.0, 1.0}
    d, m = cfg["desired_kl"], cfg["max_grad_norm"]
    assert all(abs(k / (2 * d) - 1) > 0.01 and abs(k / (d / 2) - 1) > 0.01 for k in fx["kl"])
    assert all(abs(n / m - 1) > 0.01 for n in list(fx["grad_norm"]) + list(fx["vae_grad_norm"]))
    for s in range(12):                                          # a clipped and an unclipped log-variance in every VAE step, none near the clip
        x = dc.fixture_inputs(fx, fx["vae_params"][s - 1] if s else fx["params"][0], vae_step=s)
        pre = np.concatenate([dc.front(x, x["obs_history"])["pre"][i] for i in (1, 3)], axis=1)
        assert (np.abs(pre) >= 5.0).any() and (np.abs(pre) < 5.0).any() and np.abs(np.abs(pre) - 5.0).min() > 1e-3


def test_restatement_matches_the_reference_update(fx):
    """Every one of the 6 RL steps and 12 VAE steps of the reference's PPO_DreamWaQ.update(), interleaved as it runs them: the restated
    passes, the loss head's restatement and the restated optimizers reproduce outputs, the four losses, gradients, norms, rates and EVERY
    parameter to 1e-12.  That every parameter agrees after an RL step also shows that the VAE takes nothing from the RL loss."""
    cfg = fx["cfg"]
    params = {k: v.copy() for k, v in fx["init"].items()}
    rl_state, vae_state, lr = {}, {}, cfg["lr0"]
    for s in range(cfg["steps"]):
        x = dc.fixture_inputs(fx, params, rl_step=s)
        fw = dc.rl_forward(x)
        for k in ("mu", "sigma", "values"):
            assert tc.max_err(fw[k], fx[k][s]) <= 1e-12, (s, k)
        r = pc.restate(dc.fixture_loss_inputs(fx, s, fw["mu"], fw["sigma"], fw["values"]), True, False, cfg["entropy_coef"], clip=cfg["clip_param"],
                       value_loss_coef=cfg["value_loss_coef"])
        assert abs(float(r["loss"]) - fx["loss"][s]) <= 1e-12 and abs(float(r["kl"][0]) - fx["kl"][s]) <= 1e-12
        x.update(grad_mu=r["grad_mu"][0], grad_sigma=r["grad_sigma"][0], grad_values=r["grad_values"])
        grads = dc.rl_backward(x)
        for name, g, want in zip(fx["rl_names"], grads, fx["grads"][s]):
            assert g.shape == want.shape and tc.max_err(g, want) <= 1e-12, (s, name)
        step = ta.adam(x["rl_params"], grads, rl_state, lr, cfg, kl=float(r["kl"][0]))
        lr = step["lr"]
        assert lr == fx["lr"][s] and abs(step["grad_norm"] - fx["grad_norm"][s]) <= 1e-12
        params.update(zip(fx["rl_names"], step["params"]))
        for n in fx["names"]:                                   # the VAE's parameters stay: the RL step does not touch them
            assert tc.max_err(params[n], fx["params"][s][n]) <= 1e-12, (s, n)
        for v in range(cfg["vae_epochs"] * s, cfg["vae_epochs"] * (s + 1)):
            x = dc.fixture_inputs(fx, params, vae_step=v)
            e = dc.vae_pass(x)
            assert tc.max_err(e["losses"], fx["vae_losses"][v]) <= 1e-12 * max(1.0, np.abs(fx["vae_losses"][v]).max()), (v, e["losses"])
            for name, g, want in zip(fx["vae_names"], e["grads"], fx["vae_grads"][v]):
                assert g.shape == want.shape and tc.max_err(g, want) <= 1e-12 * max(1.0, np.abs(want).max()), (v, name)
            step = ta.adam(x["vae_params"], e["grads"], vae_state, cfg["encoder_lr"], cfg)
            assert abs(step["grad_norm"] - fx["vae_grad_norm"][v]) <= 1e-12 * fx["vae_grad_norm"][v]
            params.update(zip(fx["vae_names"], step["params"]))
            for n in fx["names"]:                               # actor, critic and std stay: the VAE step leaves them alone
                assert tc.max_err(params[n], fx["vae_params"][v][n]) <= 1e-12, (v, n)


HOST_CASES = ["fixture_b33", "fixture_b257", "fixture_noclip_b33", "one_one_b31", "go2_dwaq_b31", "l1_e1_b33", "l5_e17_b33", "l65_e4_b33", "l16_e65_b33",
              "h1_b33", "h80_b33", "wide_b9"]


@pytest.mark.parametrize("case", HOST_CASES)
def test_restatement_matches_torch_float64_autograd(case):
    x = dc.make_inputs(case)
    ref = dc.torch_passes(x, torch.float64)
    fw, e = dc.rl_forward(x), dc.vae_pass(x)
    rel = lambda a, b: tc.max_err(a, b) <= 1e-12 * max(1.0, np.abs(b).max())
    assert all(rel(fw[k], ref[k]) for k in ("mu", "sigma", "values")) and rel(e["losses"], ref["losses"])
    for name, g, want in zip(dc.rl_names(x["actor"], x["critic"]), dc.rl_backward(x), ref["rl_grads"]):
        assert g.shape == want.shape and rel(g, want), name
    for name, g, want in zip(dc.vae_names(x["enc"], x["dec"]), e["grads"], ref["vae_grads"]):
        assert g.shape == want.shape and rel(g, want), name
    rl_s, vae_s, tile = dc.kernel_order_slices(x)
    for g, want in zip(dc.rl_backward(x, slices=rl_s), dc.rl_backward(x)):
        assert rel(g, want)
    tiled = dc.vae_pass(x, slices=vae_s, row_tile=tile)
    assert rel(tiled["losses"], e["losses"]) and all(rel(a, b) for a, b in zip(tiled["grads"], e["grads"]))
    # the conventions, as autograd has them: the RL cotangents DO reach the VAE (the pass drops that gradient, as the reference's zero_grad
    # does); the VAE loss reaches neither actor, critic nor std
    assert any(g is not None and np.abs(g).max() > 0 for g in ref["vae_rl_grads"]) and all(g is None for g in ref["rl_vae_grads"])
    # the upstream scalar scales the gradients, not the losses
    twice = dc.vae_pass(x, upstream=2.0 * float(x["upstream"]))
    assert np.array_equal(twice["losses"], e["losses"]) and all(rel(a, 2.0 * b) for a, b in zip(twice["grads"], e["grads"]))
    # the module helper computes the same passes (what the GPU file hands to FusedTrainPassDreamWaQ)
    m = dc.Module(x, dtype=torch.float64)
    d = lambda k: torch.as_tensor(x[k]).double()
    mu, sigma, values = m(d("obs"), d("obs_history"), d("critic_obs"), d("noise"))
    assert rel(mu.detach().numpy(), fw["mu"]) and rel(values.detach().numpy(), fw["values"])
    got = m.vae_loss(d("obs_history"), d("labels"), d("next_states"), d("terminated"), d("vae_noise"))
    assert rel(np.array([float(v.detach()) for v in got]), e["losses"])
    assert [n for n, _ in m.vae.named_parameters()] == [n[4:] for n in dc.vae_names(x["enc"], x["dec"])]
    assert [n for n, p in m.named_parameters() if not n.startswith("vae.") and n != "std"] + ["std"] == dc.rl_names(x["actor"], x["critic"])


def test_the_kld_broadcasts_and_masked_rows():
    """The KL term carries T / B^2 on every row whatever its own mask; a fully masked batch gives zero for all three terms and every
    gradient; the mask is a multiplication."""
    x = dc.make_inputs("fixture_b33")
    e = dc.vae_pass(x)
    t = x["terminated"].astype(np.float64)
    fr = e["front"]
    s = (1 + fr["out"][1] - fr["out"][0] ** 2 - np.exp(fr["out"][1])).sum(1)
    assert abs(e["losses"][3] - (-0.5 * (s * t).mean())) <= 1e-12 * abs(e["losses"][3]) and (s * t).shape == (33, 33)      # (B,) x (B, 1): literally
    assert abs(e["losses"][3] - (-0.5 * (s * t[:, 0]).mean())) > 1e-3 * abs(e["losses"][3])               # not the per-row mask
    masked = np.flatnonzero(t[:, 0] == 0)
    assert len(masked) and np.abs(e["head_g"][0][masked]).max() > 0                                        # a masked row still has a KL gradient
    off = dict(x, terminated=np.zeros_like(x["terminated"]))
    z = dc.vae_pass(off)
    assert (z["losses"] == 0).all() and all((g == 0).all() for g in z["grads"])
    row = int(masked[0])
    for key in ("obs_history", "next_states", "labels"):        # a NaN in a masked row: NaN * 0, here and in torch
        bad = dict(x, **{key: x[key].copy()})
        bad[key][row, 1] = np.nan
        assert np.isnan(dc.vae_pass(bad)["losses"][0]) and np.isnan(dc.torch_passes(bad, torch.float64)["losses"][0])


# ---- the float32 restatement and the planted defects ------------------------------------------------------------------------------------------
def _restated(x, dtype=np.float64, wrong=None, kernel_order=False):
    rl_s, vae_s, tile = dc.kernel_order_slices(x) if kernel_order else (None, None, None)
    e = dc.vae_pass(x, dtype, slices=vae_s, row_tile=tile, wrong=wrong)
    return dc.named(x, dc.rl_forward(x, dtype), dc.rl_backward(x, dtype, slices=rl_s), e["grads"]), e["losses"]


@pytest.mark.parametrize("case", ["fixture_b257", "go2_dwaq_b257", "one_one_b33", "l5_e17_b33", "fixture_noclip_b33"])
def test_float32_restatement_in_the_kernels_order_keeps_half_the_rule(case):
    x = dc.make_inputs(case)
    got, losses = _restated(x, np.float32, kernel_order=True)
    dc.check_case(got, losses, x, f"numpy f32 {case}", factor=oc.PARITY_FACTOR / 2)


def test_every_table_draw_lets_the_float32_restatement_keep_half_the_rule():
    """The criterion a draw has to meet to be a table case (tests/train_dwaq_cases.RESEEDED): an evaluation that is not the kernel's, float32
    numpy in the kernel's order of sums, stays within half the rule of the one torch float32 evaluation the rule divides by.  The six
    default draws that do not are on record with the seeds that replaced them; they still fail it."""
    for name in dc.CASES:
        x = dc.make_inputs(name)
        dc.check_case(*_restated(x, np.float32, kernel_order=True), x, f"numpy f32 {name}", factor=oc.PARITY_FACTOR / 2)
    names = list(dc.CASES)
    for name, seed in dc.RESEEDED.items():
        assert dc.CASES[name]["seed"] == seed and seed >= 1393
        x = dc.make_inputs(dict(dc.CASES[name], seed=1392 if name == "fixture_b8193" else 1300 + names.index(name)))
        with pytest.raises(AssertionError):
            dc.check_case(*_restated(x, np.float32, kernel_order=True), x, f"the default draw of {name}", factor=oc.PARITY_FACTOR / 2)


def test_parity_rule_catches_the_planted_defects():
    x = dc.make_inputs("fixture_b257")
    refs = dc.references(x)
    dc.check_case(*_restated(x), x, "the restatement itself", refs=refs)
    for wrong, match in (("kld_per_row", r"loss|latent_mu|latent_var|encoder"), ("est_from_mu", r"loss|vel_var|vel_mu"),
                         ("latent_cols", r"latent_mu|latent_var|encoder"), ("no_var_mask", r"latent_var|vel_var|encoder")):
        with pytest.raises(AssertionError, match=match):
            dc.check_case(*_restated(x, wrong=wrong), x, wrong, refs=refs)
    # each defect is caught in the tensors it should reach, not by accident elsewhere
    r64, r32 = refs[0], refs[1]
    for wrong, name in (("kld_per_row", "vae.latent_mu.weight"), ("est_from_mu", "vae.vel_var.0.weight"), ("latent_cols", "vae.latent_mu.weight"),
                        ("no_var_mask", "vae.vel_var.0.weight")):
        got, _ = _restated(x, wrong=wrong)
        with pytest.raises(AssertionError):
            dc.check_parity({name: got[name]}, {name: r64[name]}, {name: r32[name]}, f"{wrong} in {name}")
    # a select and a multiplication part ways only where a masked row is not finite: the rule sees it there
    row = int(np.flatnonzero(x["terminated"][:, 0] == 0)[0])
    y = dict(x, next_states=x["next_states"].copy())
    y["next_states"][row, 0] = np.nan
    qrefs = dc.references(y)
    assert np.isnan(qrefs[2][0][1]["loss"]).all() and np.isnan(qrefs[3][0][1]["loss"]).all()
    wrong = _restated(y, wrong="select")
    assert np.isfinite(wrong[1]).all()
    with pytest.raises(AssertionError, match=r"the mask as a select"):
        dc.check_case(*wrong, y, "the mask as a select", refs=qrefs)
    with pytest.raises(AssertionError, match=r"loss"):                # the reconstruction loss itself, and through it the total
        dc.check_parity(dc.named_losses(wrong[1])[2][1], qrefs[2][2][1], qrefs[3][2][1], "the mask as a select: rec_loss")
    for case in ("l4_e5_b33", "l17_e16_b33"):                   # the column defect at other boundaries
        x = dc.make_inputs(case)
        with pytest.raises(AssertionError):
            dc.check_case(*_restated(x, wrong="latent_cols"), x, case)


# ---- the plans ----------------------------------------------------------------------------------------------------------------------------
PLAN_BATCHES = (1, 4, 31, 33, 64, 65, 127, 128, 129, 130, 257, 2048, 4097, 8193, 18000)
NAMED_NETS = ["fixture", "go2_dwaq", "one_one", "wide"]


@pytest.mark.parametrize("net", NAMED_NETS + dc.SWEEP + dc.HWIDTHS)
def test_plans_against_the_restated_rules(net):
    enc, L, E, dec, actor, critic = dc.NETS[net]
    for b in PLAN_BATCHES if net in NAMED_NETS else (33, 257):
        p, want = train.plan_dwaq(b, enc, L, E, actor, critic), dc.restated_plan_dwaq(b, enc, L, E, actor, critic)
        assert (p.row_tile, p.lds_bytes, p.workspace_floats, p.weight_jobs, p.std_p_off, p.cat_off, p.lds_x, p.lds_y) == \
            (want["row_tile"], want["lds_bytes"], want["workspace_floats"], want["weight_jobs"], want["std_p_off"], 0, want["lds_x"], want["lds_x"] ^ 1), (net, b)
        assert (p.std_slices, p.std_slice_rows) == want["std"] and (p.enc_out_off, p.gl_rec_off, p.gl_est_off, p.partial_off, p.scale_off, p.loss_tiles) == \
            (-1, -1, -1, -1, -1, 0) and list(p.head_off) == [-1] * 4
        assert all(v == -1 for k in ("h_off", "g_off", "p_off") for ci in range(ACT) for v in getattr(p, k)[ci])
        for i, (ci, c) in enumerate(((ACT, actor), (CRI, critic))):
            n = len(c) - 1
            for k in ("slices", "slice_rows", "h_off", "g_off", "p_off"):
                assert list(getattr(p, k)[ci])[:n] == want[k][i], (net, b, k)
            assert all(v == -1 for k in ("h_off", "g_off", "p_off") for v in list(getattr(p, k)[ci])[n:])
        q, want = train.plan_vae(b, enc, L, E, dec), dc.restated_plan_vae(b, enc, L, E, dec)
        for k in ("row_tile", "lds_bytes", "workspace_floats", "weight_jobs", "cat_off", "enc_out_off", "gl_rec_off", "gl_est_off", "partial_off", "scale_off",
                  "loss_tiles", "lds_x"):
            assert getattr(q, k) == want[k], (net, b, k)
        assert list(q.head_off) == want["head_off"] and q.partial_off % 2 == 0 and (q.std_p_off, q.std_slices) == (-1, 0)
        for ci, c in enumerate([enc] + dc.head_widths(enc, L, E) + [dec]):
            n = len(c) - 1
            for k in ("slices", "slice_rows", "h_off", "g_off", "p_off"):
                assert list(getattr(q, k)[ci])[:n] == want[k][ci], (net, b, k)
        assert all(v == -1 for k in ("h_off", "g_off", "p_off") for v in getattr(q, k)[CRI])


def test_plan_edges():
    enc, L, E, dec, actor, critic = dc.NETS["go2_dwaq"]
    p, q = train.plan_dwaq(18000, enc, L, E, actor, critic), train.plan_vae(18000, enc, L, E, dec)
    assert p.row_tile == 16 and p.lds_bytes <= tc.LDS_BYTES < 2 * p.lds_bytes
    # the VAE pass keeps the 32-row tile: the head products go through two regions of X, not four
    assert q.row_tile == 32 and q.lds_bytes == 32 * (900 + 264) * 4 + dc.RED_BYTES and (q.lds_x, q.lds_y) == (1, 0)
    assert 32 * (900 + 4 * 132) * 4 + dc.RED_BYTES > tc.LDS_BYTES
    assert list(q.slices[ENC])[0] == 32 and list(p.slices[CRI])[0] == 9
    # the heads' four regions are counted: with a one-layer encoder 4 -> 2 and heads of 65 columns the tile's widths are the regions'
    r = dc.restated_plan_vae(33, [4, 2], 65, 65, [130, 3])
    assert r["lds_bytes"] == 32 * (max(132, 4, 2 * 4) + 4 * 68) * 4 + dc.RED_BYTES
    assert train.plan_vae(33, [4, 2], 65, 65, [130, 3]).lds_bytes == r["lds_bytes"]
    w = dc.NETS["wide"]
    assert train.plan_dwaq(9, *w[:3], *w[4:]).row_tile == 8 and train.plan_vae(9, *w[:4]).row_tile == 8
    f = dc.NETS["fixture"]
    q = train.plan_vae(8193, *f[:4])
    assert q.loss_tiles == 257 and list(q.slices[ENC])[:3] == [32, 32, 32] and 8193 % list(q.slice_rows[ENC])[0] != 0
    assert q.scale_off == q.partial_off + 2 * 4 * 257 and q.workspace_floats == q.scale_off + 2


# ---- refusals of the entry points: nothing is enqueued (there is no device here) -----------------------------------------------------------
def _good_rl(backward=True):
    x = dc.make_inputs("fixture_b33")
    m = dc.Module(x)
    spec = train.describe_dwaq(m)
    t = lambda k: torch.as_tensor(x[k])
    keep = dict(m=m, o=t("obs"), h=t("obs_history"), c=t("critic_obs"), n=t("noise"), mu=torch.zeros(33, 3), sigma=torch.zeros(33, 3), values=torch.zeros(33, 1),
                gm=t("grad_mu"), gs=t("grad_sigma"), gv=t("grad_values"), grads=[torch.zeros_like(p) for p in spec.rl_parameters()])
    f = dc.NETS["fixture"]
    keep["ws"] = torch.zeros(int(train.plan_dwaq(33, *f[:3], *f[4:]).workspace_floats))
    a = train.dwaq_args(spec, keep["o"], keep["h"], keep["c"], keep["n"], keep["mu"], keep["sigma"], keep["values"], keep["ws"],
                        keep["grads"] if backward else None, keep["gm"], keep["gs"], keep["gv"])
    a._keep = keep
    return a


def _good_vae(backward=True):
    x = dc.make_inputs("fixture_b33")
    m = dc.Module(x)
    spec = train.describe_dwaq(m)
    t = lambda k: torch.as_tensor(x[k])
    keep = dict(m=m, h=t("obs_history"), l=t("labels"), s=t("next_states"), t=t("terminated"), n=t("vae_noise"), loss=torch.zeros(4), up=torch.ones(1),
                grads=[torch.zeros_like(p) for p in spec.vae_parameters()])
    keep["ws"] = torch.zeros(int(train.plan_vae(33, *dc.NETS["fixture"][:4]).workspace_floats))
    a = train.vae_args(spec, keep["h"], keep["l"], keep["s"], keep["t"], keep["n"], 0.5, keep["loss"], keep["ws"], keep["grads"] if backward else None, keep["up"])
    a._keep = keep
    return a


# (mutation, message, which entry points refuse it: p plan, f forward, b backward)
RL_REFUSALS = [
    (ta.set_path(("n_rows",), 0), b"n_rows = 0 < 1", "pfb"),
    (ta.set_path(("n_obs",), 0), b"n_obs = 0 < 1", "pfb"),
    (ta.set_path(("chain", 0, "n_layers"), 0), b"chain[0] (encoder).n_layers = 0 is outside [1, 4]", "pfb"),
    (ta.set_path(("chain", 5, "n_layers"), 5), b"chain[5] (actor).n_layers = 5 is outside [1, 4]", "pfb"),
    (ta.set_path(("chain", 2, "n_layers"), 2), b"chain[2] (latent_var).n_layers = 2, a head is one Linear", "pfb"),
    (ta.set_path(("chain", 6, "layer", 1, "n_in"), 15), b"chain[6] (critic).layer[1].n_in = 15, but its input has 8 columns", "pfb"),
    (ta.set_path(("chain", 0, "layer", 2, "n_out"), 0), b"chain[0] (encoder).layer[2].n_out = 0 is outside [1, 2048]", "pfb"),
    (ta.set_path(("chain", 3, "layer", 0, "n_in"), 9), b"chain[3] (vel_mu).layer[0].n_in = 9, but the encoder ends at 10 columns", "pfb"),
    (ta.set_path(("chain", 2, "layer", 0, "n_out"), 4), b"chain[2] (latent_var).layer[0].n_out = 4, but its mean's head has 3 columns", "pfb"),
    (ta.set_path(("chain", 4, "layer", 0, "n_out"), 1), b"chain[4] (vel_var).layer[0].n_out = 1, but its mean's head has 2 columns", "pfb"),
    (ta.set_path(("chain", 5, "layer", 0, "n_in"), 13), b"chain[5] (actor).layer[0].n_in = 13, but [obs | z | v] has 7 + 3 + 2 columns", "pfb"),
    (ta.set_path(("n_obs",), 6), b"chain[5] (actor).layer[0].n_in = 12, but [obs | z | v] has 6 + 3 + 2 columns", "pfb"),
    (ta.set_path(("chain", 0, "input"), None), b"chain[0] (encoder).input is null", "fb"),
    (ta.set_path(("chain", 5, "input"), None), b"chain[5] (actor).input is null", "fb"),
    (ta.set_path(("chain", 6, "input"), None), b"chain[6] (critic).input is null", "fb"),
    (ta.set_path(("chain", 0, "in_stride"), 13), b"chain[0] (encoder).in_stride = 13 is below its width 14", "fb"),
    (ta.set_path(("chain", 5, "in_stride"), 6), b"chain[5] (actor).in_stride = 6 is below its width 7", "fb"),
    (ta.set_path(("chain", 6, "in_stride"), 8), b"chain[6] (critic).in_stride = 8 is below its width 9", "fb"),
    (ta.set_path(("chain", 0, "layer", 1, "weight"), None), b"chain[0] (encoder).layer[1].weight is null", "fb"),
    (ta.set_path(("chain", 4, "layer", 0, "bias"), None), b"chain[4] (vel_var).layer[0].bias is null", "fb"),
    (ta.set_path(("chain", 5, "layer", 2, "grad_weight"), None), b"chain[5] (actor).layer[2].grad_weight is null", "b"),
    (ta.set_path(("chain", 6, "layer", 1, "grad_bias"), None), b"chain[6] (critic).layer[1].grad_bias is null", "b"),
    (ta.set_path(("noise",), None), b"noise is null", "fb"),
    (ta.set_path(("noise_stride",), 4), b"noise_stride = 4 is below its width 5", "fb"),
    (ta.set_path(("var_clip",), -1.0), b"var_clip must be >= 0", "fb"),
    (ta.set_path(("var_clip",), float("nan")), b"var_clip must be >= 0", "fb"),
    (lambda a: (setattr(a, "clip_on", 1), setattr(a, "clip_actions", -1.0)), b"clip_actions must be >= 0 under clip_on", "fb"),
    (ta.set_path(("std",), None), b"std is null", "fb"), (ta.set_path(("mu",), None), b"mu is null", "fb"), (ta.set_path(("sigma",), None), b"sigma is null", "fb"),
    (ta.set_path(("values",), None), b"values is null", "fb"),
    (ta.set_path(("mu_stride",), 2), b"mu_stride = 2 is below its width 3", "fb"), (ta.set_path(("values_stride",), 0), b"values_stride = 0 is below its width 1", "fb"),
    (ta.set_path(("grad_std",), None), b"grad_std is null", "b"), (ta.set_path(("grad_mu",), None), b"grad_mu is null", "b"),
    (ta.set_path(("grad_sigma",), None), b"grad_sigma is null", "b"), (ta.set_path(("grad_values",), None), b"grad_values is null", "b"),
    (ta.set_path(("grad_sigma_stride",), 1), b"grad_sigma_stride = 1 is below its width 3", "b"),
    (ta.set_path(("workspace",), None), b"workspace is null", "fb"),
    (ta.set_path(("workspace_capacity",), 10), b"workspace_capacity = 10 floats is below the plan's", "fb"),
]
VAE_REFUSALS = [
    (ta.set_path(("n_rows",), -2), b"n_rows = -2 < 1", "pfb"),
    (ta.set_path(("chain", 0, "n_layers"), 5), b"chain[0] (encoder).n_layers = 5 is outside [1, 4]", "pfb"),
    (ta.set_path(("chain", 5, "n_layers"), 0), b"chain[5] (decoder).n_layers = 0 is outside [1, 4]", "pfb"),
    (ta.set_path(("chain", 1, "n_layers"), 0), b"chain[1] (latent_mu).n_layers = 0, a head is one Linear", "pfb"),
    (ta.set_path(("chain", 0, "layer", 1, "n_in"), 9), b"chain[0] (encoder).layer[1].n_in = 9, but its input has 8 columns", "pfb"),
    (ta.set_path(("chain", 5, "layer", 0, "n_out"), 4000), b"chain[5] (decoder).layer[0].n_out = 4000 is outside [1, 2048]", "pfb"),
    (ta.set_path(("chain", 1, "layer", 0, "n_in"), 11), b"chain[1] (latent_mu).layer[0].n_in = 11, but the encoder ends at 10 columns", "pfb"),
    (ta.set_path(("chain", 5, "layer", 0, "n_in"), 6), b"chain[5] (decoder).layer[0].n_in = 6, but [z | v] has 3 + 2 columns", "pfb"),
    (ta.set_path(("chain", 0, "input"), None), b"chain[0] (encoder).input is null", "fb"),
    (ta.set_path(("chain", 0, "in_stride"), 3), b"chain[0] (encoder).in_stride = 3 is below its width 14", "fb"),
    (ta.set_path(("chain", 0, "layer", 2, "weight"), None), b"chain[0] (encoder).layer[2].weight is null", "fb"),
    (ta.set_path(("chain", 5, "layer", 0, "bias"), None), b"chain[5] (decoder).layer[0].bias is null", "fb"),
    (ta.set_path(("chain", 0, "layer", 0, "grad_weight"), None), b"chain[0] (encoder).layer[0].grad_weight is null", "b"),
    (ta.set_path(("chain", 3, "layer", 0, "grad_bias"), None), b"chain[3] (vel_mu).layer[0].grad_bias is null", "b"),
    (ta.set_path(("chain", 5, "layer", 2, "grad_bias"), None), b"chain[5] (decoder).layer[2].grad_bias is null", "b"),
    (ta.set_path(("labels",), None), b"labels is null", "fb"), (ta.set_path(("next_states",), None), b"next_states is null", "fb"),
    (ta.set_path(("mask",), None), b"mask is null", "fb"), (ta.set_path(("noise",), None), b"noise is null", "fb"),
    (ta.set_path(("labels_stride",), 1), b"labels_stride = 1 is below its width 2", "fb"),
    (ta.set_path(("next_states_stride",), 4), b"next_states_stride = 4 is below its width 5", "fb"),
    (ta.set_path(("mask_stride",), 0), b"mask_stride = 0 is below its width 1", "fb"),
    (ta.set_path(("noise_stride",), 3), b"noise_stride = 3 is below its width 5", "fb"),
    (ta.set_path(("var_clip",), -0.5), b"var_clip must be >= 0", "fb"),
    (ta.set_path(("loss",), None), b"loss is null", "f"), (ta.set_path(("upstream",), None), b"upstream is null", "b"),
    (ta.set_path(("workspace",), None), b"workspace is null", "fb"),
    (lambda a: setattr(a, "workspace", a.workspace + 4), b"workspace is not 8-byte aligned", "fb"),
    (ta.set_path(("workspace_capacity",), 10), b"workspace_capacity = 10 floats is below the plan's", "fb"),
]


@pytest.mark.parametrize("i", range(len(RL_REFUSALS)))
def test_rl_entry_points_refuse(i):
    ta.refuse(RL_REFUSALS, i, _good_rl, "lg_train_dwaq", abi.LgTrainDwaqPlan)


@pytest.mark.parametrize("i", range(len(VAE_REFUSALS)))
def test_vae_entry_points_refuse(i):
    ta.refuse(VAE_REFUSALS, i, _good_vae, "lg_train_vae", abi.LgTrainDwaqPlan)


def test_entry_points_refuse_null_descriptors_and_the_lds():
    lib = abi.load_lib()
    for fn, good in (("lg_train_dwaq", _good_rl), ("lg_train_vae", _good_vae)):
        plan = getattr(lib, fn + "_plan")
        assert plan(None, C.byref(abi.LgTrainDwaqPlan())) != 0 and (fn + "_plan: null descriptor").encode() in lib.lg_last_error()
        assert plan(C.byref(good()), None) != 0 and (fn + "_plan: null plan").encode() in lib.lg_last_error()
        for d in ("_forward", "_backward"):
            assert getattr(lib, fn + d)(None, None) != 0 and (fn + d + ": null descriptor").encode() in lib.lg_last_error()
        a = good(backward=False)                                              # a forward-only descriptor is what backward refuses
        assert getattr(lib, fn + "_backward")(C.byref(a), None) != 0
    # an encoder that ends 2048 wide asks the VAE backward for two 2052-float product regions beside a 2052-float activation: no 8-row tile
    with pytest.raises(RuntimeError, match=r"lg_train_vae_plan: an 8-row tile of these widths \(\d+ floats per row\) does not fit the 160 KB of LDS"):
        train.plan_vae(9, [2048, 2048], 3, 2, [5, 2048, 3])
    # the RL descriptor leaves the VAE's gradient members alone: train.dwaq_args does not even fill them
    a = _good_rl()
    assert all(not a.chain[ci].layer[li].grad_weight and not a.chain[ci].layer[li].grad_bias for ci in range(ACT) for li in range(3))
    assert all(a.chain[ci].layer[li].grad_weight for ci in (ACT, CRI) for li in range(3))
    # and the VAE descriptor has neither an actor nor a critic
    assert C.sizeof(abi.LgTrainVaeArgs().chain) == abi.TRAIN_VAE_CHAINS * C.sizeof(abi.LgTrainChain)


# ---- refusals of the Python surface -------------------------------------------------------------------------------------------------------
class _VAE(nn.Module):
    """H = 6, L = 2, E = 3, D = 4."""

    def __init__(self, encoder=None, decoder=None, latent_var=None, vel_var=None, vel_mu=None):
        super().__init__()
        self.encoder = encoder if encoder is not None else nn.Sequential(nn.Linear(7, 5), nn.ELU(), nn.Linear(5, 6), nn.ELU())
        self.latent_mu = nn.Linear(6, 2)
        self.latent_var = latent_var if latent_var is not None else nn.Sequential(nn.Linear(6, 2), nn.Hardtanh(-5.0, 5.0))
        self.vel_mu = vel_mu if vel_mu is not None else nn.Linear(6, 3)
        self.vel_var = vel_var if vel_var is not None else nn.Sequential(nn.Linear(6, 3), nn.Hardtanh(-5.0, 5.0))
        self.decoder = decoder if decoder is not None else nn.Sequential(nn.Linear(5, 8), nn.ELU(), nn.Linear(8, 4))


class _DW(nn.Module):
    """O = 4, so actor[0] = 4 + 2 + 3."""

    def __init__(self, vae=None, actor=None, critic=None, A=3):
        super().__init__()
        self.vae = vae if vae is not None else _VAE()
        self.actor = actor if actor is not None else nn.Sequential(nn.Linear(9, 8), nn.ELU(), nn.Linear(8, A))
        self.critic = critic if critic is not None else nn.Sequential(nn.Linear(6, 8), nn.ELU(), nn.Linear(8, 1))
        self.std = nn.Parameter(torch.ones(A))


def test_describe_dwaq_takes_actor_critic_dreamwaq():
    m = _DW()
    spec = train.describe_dwaq(m)
    assert spec.encoder.widths == [7, 5, 6] and spec.encoder.elu == [True, True] and [h.widths for h in spec.heads] == [[6, 2], [6, 2], [6, 3], [6, 3]]
    assert spec.decoder.widths == [5, 8, 4] and spec.actor.widths == [9, 8, 3] and spec.critic.widths == [6, 8, 1]
    assert (spec.num_obs, spec.num_latent, spec.num_explicit, spec.num_actions, spec.var_clip, spec.clip_actions) == (4, 2, 3, 3, 5.0, None)
    want = list(m.actor.parameters()) + list(m.critic.parameters()) + [m.std]                    # PPO_DreamWaQ.rl_parameters
    assert len(spec.rl_parameters()) == len(want) and all(a is b for a, b in zip(spec.rl_parameters(), want))
    assert len(spec.vae_parameters()) == 16 and all(a is b for a, b in zip(spec.vae_parameters(), m.vae.parameters()))
    clipped = train.describe_dwaq(_DW(actor=nn.Sequential(nn.Linear(9, 8), nn.ELU(), nn.Linear(8, 3), nn.Hardtanh(-0.5, 0.5))))
    assert clipped.clip_actions == 0.5
    # the other passes keep refusing the family exactly as before, and a trailing ELU anywhere else
    with pytest.raises(ValueError, match=r"FusedTrainPass: the module has \.vae \(ActorCriticDreamWaQ\); only the plain ActorCritic"):
        train.describe(m)
    with pytest.raises(ValueError, match=r"FusedTrainPassEE: the module has no \.estimator"):
        train.describe_ee(m)
    with pytest.raises(ValueError, match=r"FusedTrainPassTS: the module has no \.privilege_encoder"):
        train.describe_ts(m)
    doc = train.FusedTrainPassDreamWaQ.__doc__
    assert "NOT the reference's stream" in doc and "caller-owned noise tensor" in doc and "(B, B)" in doc
    import inspect
    assert list(inspect.signature(train.FusedTrainPassDreamWaQ.__init__).parameters)[1:] == ["actor_critic", "kld_weight"]
    assert list(inspect.signature(train.FusedTrainPassDreamWaQ.__call__).parameters)[1:] == ["obs", "obs_history", "critic_obs", "latent_noise"]
    assert list(inspect.signature(train.FusedTrainPassDreamWaQ.vae_loss).parameters)[1:] == ["obs_history", "explicit_info_labels", "next_states", "terminated",
                                                                                             "latent_noise"]


def _break(f, **kw):
    m = _DW(**kw)
    f(m)
    return m


SURFACE_REFUSALS = [
    (lambda: _break(lambda m: delattr(m, "vae")), r"FusedTrainPassDreamWaQ: the module has no \.vae"),
    (lambda: _break(lambda m: setattr(m, "estimator", nn.Sequential(nn.Linear(5, 2)))), r"FusedTrainPassDreamWaQ: the module has \.estimator \(ActorCriticEE\) beside \.vae"),
    (lambda: _break(lambda m: setattr(m, "privilege_encoder", nn.Sequential(nn.Linear(5, 2)))), r"\.privilege_encoder \(ActorCriticTS / ActorCriticCTS\) beside \.vae"),
    (lambda: _break(lambda m: setattr(m, "history_encoder", nn.Sequential(nn.Linear(5, 2)))), r"\.history_encoder \(ActorCriticTS / ActorCriticCTS\) beside \.vae"),
    (lambda: _break(lambda m: setattr(m, "memory_a", nn.LSTM(5, 2))), r"\.memory_a \(ActorCriticRecurrent\) beside"),
    (lambda: _break(lambda m: setattr(m, "memory_c", nn.LSTM(5, 2))), r"\.memory_c \(ActorCriticRecurrent\) beside"),
    (lambda: _break(lambda m: setattr(m, "is_recurrent", True)), r"FusedTrainPassDreamWaQ: the module is recurrent"),
    (lambda: _break(lambda m: delattr(m, "critic")), r"FusedTrainPassDreamWaQ: the module has no \.critic"),
    (lambda: _break(lambda m: delattr(m.vae, "decoder")), r"FusedTrainPassDreamWaQ: the module's \.vae has no \.decoder"),
    (lambda: _DW(vae=_VAE(decoder=nn.Sequential(nn.Linear(5, 8), nn.ELU(), nn.Linear(8, 4), nn.ELU()))), r"FusedTrainPassDreamWaQ: decoder ends in an ELU"),
    (lambda: _DW(actor=nn.Sequential(nn.Linear(9, 8), nn.ELU(), nn.Linear(8, 3), nn.ELU())), r"FusedTrainPassDreamWaQ: actor ends in an ELU"),
    (lambda: _DW(vae=_VAE(encoder=nn.Sequential(nn.Linear(7, 5), nn.Tanh(), nn.Linear(5, 6)))), r"encoder\[1\] is Tanh; only Linear and ELU are built"),
    (lambda: _DW(vae=_VAE(encoder=nn.Sequential(nn.Linear(7, 5), nn.ELU(), nn.Linear(5, 7), nn.ELU()))), r"vae\.latent_mu takes 6 inputs, the encoder ends at 7 columns"),
    (lambda: _DW(vae=_VAE(latent_var=nn.Linear(6, 2))), r"vae\.latent_var is not Sequential\(Linear, Hardtanh\)"),
    (lambda: _DW(vae=_VAE(vel_var=nn.Sequential(nn.Linear(6, 3), nn.Hardtanh(-5.0, 4.0)))), r"vae\.vel_var\[1\] \(Hardtanh\(-5\.0, 4\.0\)\) must be a symmetric clip"),
    (lambda: _DW(vae=_VAE(vel_var=nn.Sequential(nn.Linear(6, 3), nn.Hardtanh(-4.0, 4.0)))), r"vae\.latent_var clips to 5\.0, vae\.vel_var to 4\.0; the kernel takes one clip"),
    (lambda: _DW(vae=_VAE(latent_var=nn.Sequential(nn.Linear(6, 3), nn.Hardtanh(-5.0, 5.0)))), r"vae\.latent_mu has 2 outputs, vae\.latent_var 3"),
    (lambda: _DW(vae=_VAE(vel_mu=nn.Sequential(nn.Linear(6, 3)))), r"vae\.vel_mu is Sequential, expected a Linear"),
    (lambda: _DW(vae=_VAE(vel_mu=nn.Linear(6, 3, bias=False))), r"vae\.vel_mu has no bias"),
    (lambda: _DW(vae=_VAE(decoder=nn.Sequential(nn.Linear(6, 8), nn.ELU(), nn.Linear(8, 4)))), r"decoder\[0\] takes 6 inputs, but \[z \| v\] has 2 \+ 3 columns"),
    (lambda: _DW(actor=nn.Sequential(nn.Linear(5, 8), nn.ELU(), nn.Linear(8, 3))), r"actor\[0\] takes 5 inputs, but \[obs \| z \| v\] has O \+ 2 \+ 3 columns with O >= 1"),
    (lambda: _DW(critic=nn.Sequential(nn.Linear(6, 8), nn.ReLU(), nn.Linear(8, 1))), r"critic\[1\] is ReLU"),
    (lambda: _break(lambda m: setattr(m.vae.encoder[0], "weight", nn.Parameter(torch.zeros(5, 7, dtype=torch.float64)))), r"encoder\[0\]\.weight is torch\.float64"),
    (lambda: _break(lambda m: setattr(m, "std", nn.Parameter(torch.ones(4)))), r"FusedTrainPassDreamWaQ: std has shape \(4,\), the actor has 3 outputs"),
    (lambda: _break(lambda m: setattr(m.vae, "extra", nn.Linear(2, 2))), r"vae\.parameters\(\) are not the encoder's, latent_mu's"),
]


@pytest.mark.parametrize("i", range(len(SURFACE_REFUSALS)))
def test_describe_dwaq_refuses(i):
    make, msg = SURFACE_REFUSALS[i]
    with pytest.raises(ValueError, match=msg):
        train.describe_dwaq(make())


def test_the_surface_refuses_devices_and_tensors():
    with pytest.raises(ValueError, match=r"FusedTrainPassDreamWaQ: the module is on cpu, not on a HIP device \(there is no CPU path\)"):
        train.FusedTrainPassDreamWaQ(_DW())
    with pytest.raises(ValueError, match=r"is on cpu, not on cuda:0"):
        train.describe_dwaq(_DW(), torch.device("cuda:0"))
    spec = train.describe_dwaq(_DW())
    ok = dict(o=torch.zeros(4, 4), h=torch.zeros(4, 7), c=torch.zeros(4, 6), n=torch.zeros(4, 5), mu=torch.zeros(4, 3), sigma=torch.zeros(4, 3), values=torch.zeros(4, 1))
    call = lambda **kw: train.dwaq_args(spec, *[{**ok, **kw}[k] for k in ("o", "h", "c", "n", "mu", "sigma", "values")], None)
    a = call()
    assert (a.n_rows, a.n_obs, a.clip_on, a.var_clip, a.noise_stride) == (4, 4, 0, 5.0, 5)
    for kw, msg in ((dict(o=torch.zeros(4, 5)), r"FusedTrainPassDreamWaQ: obs must be \(4, 4\) float32"),
                    (dict(h=torch.zeros(4, 6)), r"obs_history must be \(4, 7\)"), (dict(c=torch.zeros(3, 6)), r"critic_obs must be \(4, 6\)"),
                    (dict(n=torch.zeros(4, 4)), r"latent_noise must be \(4, 5\)"), (dict(o=torch.zeros(0, 4)), r"obs must be a \(B, 4\) float32 tensor with B >= 1"),
                    (dict(mu=torch.zeros(4, 2)), r"mu must be \(4, 3\)")):
        with pytest.raises(ValueError, match=msg):
            call(**kw)
    vok = dict(h=ok["h"], l=torch.zeros(4, 3), s=torch.zeros(4, 4), t=torch.ones(4, 1), n=ok["n"], loss=torch.zeros(4))
    vae = lambda **kw: train.vae_args(spec, *[{**vok, **kw}[k] for k in ("h", "l", "s", "t", "n")], 0.25, {**vok, **kw}["loss"], None)
    a = vae()
    assert (a.n_rows, a.mask_stride, a.kld_weight, a.var_clip) == (4, 1, 0.25, 5.0)
    for kw, msg in ((dict(h=torch.zeros(4, 8)), r"obs_history must be \(4, 7\)"), (dict(l=torch.zeros(4, 2)), r"explicit_info_labels must be \(4, 3\)"),
                    (dict(s=torch.zeros(4, 5)), r"next_states must be \(4, 4\)"), (dict(t=torch.ones(4)), r"terminated must be \(4, 1\)"),
                    (dict(n=torch.zeros(4, 5, dtype=torch.float64)), r"latent_noise must be \(4, 5\) float32"),
                    (dict(loss=torch.zeros(1)), r"FusedTrainPassDreamWaQ: the losses must be 4 float32")):
        with pytest.raises(ValueError, match=msg):
            vae(**kw)
    wide = torch.zeros(4, 24)                                                 # strided views are addressed in place
    a = vae(h=wide[:, 1:8], l=wide[:, 9:12], s=wide[:, 12:16], t=wide[:, 17:18], n=wide[:, 19:24])
    assert (a.chain[0].input, a.chain[0].in_stride, a.labels, a.labels_stride, a.next_states, a.mask, a.mask_stride, a.noise, a.noise_stride) == \
        (wide.data_ptr() + 4, 24, wide.data_ptr() + 36, 24, wide.data_ptr() + 48, wide.data_ptr() + 68, 24, wide.data_ptr() + 76, 24)


# ---- the case table -----------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_the_edges():
    nets = {c["net"] for c in dc.CASES.values()}
    assert set(dc.SWEEP) <= nets and len(dc.SWEEP) == 36 and set(dc.HWIDTHS) <= nets and {"fixture", "one_one", "go2_dwaq", "wide"} <= nets
    assert dc.NETS["go2_dwaq"] == ([900, 256, 128, 80], 16, 24, [40, 256, 128, 45], [85, 512, 256, 128, 12], [885, 1024, 256, 128, 1])
    assert all(d[0] == L + E and a[0] > L + E for _, L, E, d, a, _ in dc.NETS.values())
    assert (len(dc.NETS["one_one"][0]) - 1, len(dc.NETS["one_one"][3]) - 1) == (1, 1)
    for net in ("fixture", "one_one") + dc.REAL:
        assert {dc.CASES[f"{net}_b{b}"]["B"] for b in dc.BATCHES} == {1, 31, 33, 257}
    Ls, Es = {dc.NETS[n][1] for n in dc.SWEEP}, {dc.NETS[n][2] for n in dc.SWEEP}
    assert Ls == Es == {1, 4, 5, 16, 17, 65}
    O = {(dc.NETS[n][4][0] - dc.NETS[n][1] - dc.NETS[n][2]) for n in dc.SWEEP}
    OL = {(dc.NETS[n][4][0] - dc.NETS[n][2]) for n in dc.SWEEP}
    assert {o % 4 == 0 for o in O} == {True, False} and {o % 4 == 0 for o in OL} == {True, False}      # O and O + L off and on multiples of 4
    assert {dc.NETS[n][0][-1] for n in dc.HWIDTHS} == {1, 5, 80}
    assert {0, 1} == {dc.restated_plan_vae(33, *dc.NETS[n][:4])["lds_x"] for n in ("fixture", "one_one", "l4_e5")}
    w = dc.NETS["wide"]
    assert dc.restated_plan_dwaq(9, *w[:3], *w[4:])["row_tile"] == 8 and dc.restated_plan_vae(9, *w[:4])["row_tile"] == 8
    g = dc.NETS["go2_dwaq"]
    assert dc.restated_plan_dwaq(257, *g[:3], *g[4:])["row_tile"] == 16 and dc.restated_plan_vae(257, *g[:4])["row_tile"] == 32
    f = dc.NETS["fixture"]
    big = dc.restated_plan_vae(dc.CASES["fixture_b8193"]["B"], *f[:4])
    assert big["loss_tiles"] > 256 and big["slices"][0][0] == tc.MAX_SLICES and 8193 % big["slice_rows"][0][0]       # second finalize trip; 32 slices, short last
    for net in dc.RAGGED_SLICE_NETS:
        assert 64 < dc.smallest_ragged_b(net) <= 257
    assert dc.make_inputs("fixture_noclip_b33")["clip"] is None
    for name in ("fixture_b33", "go2_dwaq_b31", "l65_e17_b33", "one_one_b257"):
        x = dc.make_inputs(name)
        pre = dc.rl_forward(dict(x, clip=None))["mu"]
        assert 0.1 <= (np.abs(pre) >= x["clip"]).mean() <= 0.9 and np.abs(np.abs(pre) - x["clip"]).min() >= 1e-3
        for hist in ("obs_history",):
            lv = np.concatenate([dc.front(x, x[hist])["pre"][i] for i in (1, 3)], axis=1)
            assert 0.1 <= (np.abs(lv) >= x["var_clip"]).mean() <= 0.9 and np.abs(np.abs(lv) - x["var_clip"]).min() >= 1e-3
    x = dc.make_inputs("fixture_b257")
    assert 0.1 <= 1 - x["terminated"].mean() <= 0.6                                                     # masked and unmasked rows

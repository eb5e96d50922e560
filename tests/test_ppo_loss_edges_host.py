"""Host side of the fused PPO loss head's edge cases (tests/ppo_loss_edges.py): the plan of every width case against
lg_ppo_loss_workspace, the coverage the tables are there for, that every hand-built tie / boundary / overflow row IS what its name says
(evaluated in torch float32 on the CPU), that every arm of both gradient selectors is present, the reach of a NaN per input tensor as
the restatement sees it, and that make_inputs' `clip` key left the draws of the existing cases alone.  No GPU: nothing is launched."""
import numpy as np
import pytest
import torch

from hcr_genesis_lr_cl_amd import abi, ppo_loss
from tests import ppo_loss_cases as pc
from tests import ppo_loss_edges as pe
from tests.test_ppo_loss_host import plan as host_plan


# ---- A. widths and sweeps ---------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_header_s():
    assert (pe.THREADS, pe.MAX_BLOCKS, pe.SLOTS) == (abi.PPO_THREADS, abi.PPO_MAX_BLOCKS, abi.PPO_PARTIAL_SLOTS)
    assert max(c["A"] for c in pe.WIDTH_CASES.values()) == abi.PPO_MAX_ACTIONS


@pytest.mark.parametrize("name", list(pe.WIDTH_CASES))
def test_workspace_of_the_width_cases(name):
    c = pe.WIDTH_CASES[name]
    p = pe.plan(c)
    assert (p["tiles"], p["blocks"]) == host_plan(c["rows"], c["vrows"], c["A"])
    assert ppo_loss.workspace_doubles(c["rows"], c["vrows"], c["A"]) == min(p["tiles"], 512) * 6
    if name == "w64":
        assert c["rows"] == [p["per_tile"]]                                                           # one tile, exactly full
    else:
        assert all(b % p["per_tile"] != 0 for b in c["rows"])                                         # every other last policy tile is ragged


def test_width_table_keeps_its_coverage():
    cs = pe.WIDTH_CASES
    want = dict(w2=(1, 256), w8=(2, 128), w16=(4, 64), w17=(8, 32), w29=(8, 32), w32=(8, 32), w33=(16, 16), w48=(16, 16), w63=(16, 16),
                w64=(16, 16), cts_w64=(16, 16), cts_sweep_w64=(16, 16))
    assert {n: (pe.plan(c)["lanes"], pe.plan(c)["per_tile"]) for n, c in cs.items()} == want
    assert {pe.plan(c)["lanes"] for c in cs.values()} == {1, 2, 4, 8, 16}
    assert {16, 32, 63, 64} <= {c["A"] for c in cs.values()}
    assert all(all(c["kl"]) or len(c["rows"]) == 2 for c in cs.values())
    assert {(c["clipped"], c["spo"]) for c in cs.values()} == {(True, False), (False, False), (True, True), (False, True)}
    for n in pe.STRIDED:                                                                              # a whole quad AND a scalar tail, L 8 and 16
        assert cs[n]["A"] % 4 != 0 and cs[n]["A"] > 4
    assert {pe.plan(cs[n])["lanes"] for n in pe.STRIDED} == {8, 16}
    # the two-group sweep: more tiles than workgroups, one workgroup with tiles of group 0 and group 1, another with group 0 and value
    c = cs[pe.SWEEP]
    p = pe.plan(c)
    assert len(c["rows"]) == 2 and all(c["kl"]) and p["ends"] == [257, 514] and p["tiles"] == 547 > p["blocks"] == 512
    kinds = [pe.kinds_of_workgroup(c, b) for b in range(p["blocks"])]
    assert [b for b, k in enumerate(kinds) if k == [0, 1]] == [0, 1]
    assert [b for b, k in enumerate(kinds) if k == [0, "v"]] == list(range(2, 35))
    assert sum(len(k) for k in kinds) == p["tiles"] and max(len(k) for k in kinds) == 2
    assert max(sum(c["rows"]) * c["A"] for c in cs.values()) == 8199 * 64                               # the largest input


@pytest.fixture(scope="module")
def width_inputs():
    return {name: pc.make_inputs(c) for name, c in pe.WIDTH_CASES.items()}


def test_width_inputs_sit_on_both_sides_of_every_branch(width_inputs):
    for name, inp in width_inputs.items():
        pc.assert_both_sides(name, inp, pc.CLIP)


# ---- B. the hand-built rows are what their names say ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", pe.TIE_WIDTHS)
def test_tie_rows_take_the_arm_they_are_named_for(A):
    f = np.float32
    for overflow, prow, vrow in ((False, pe.POLICY_ROWS, pe.VALUE_ROWS), (True, pe.POLICY_OVERFLOW_ROWS, pe.VALUE_OVERFLOW_ROWS)):
        inp = pe.tie_inputs(A, overflow)
        arms, r = pe.policy_arm(inp["groups"][0], pe.TIE_CLIP)
        assert arms == [row[3] for row in prow], list(zip([row[0] for row in prow], arms))
        adv = inp["groups"][0]["advantages"].reshape(-1)
        for (name, a, log_ratio, _), ri, ai in zip(prow, r, adv):
            assert ai == f(a) and np.signbit(ai) == np.signbit(f(a)), name
            if name.startswith("ratio == 1"):
                assert ri == f(1.0), name                                                             # exactly
            elif "inside" in name:
                assert f(0.75) < ri < f(1.25) and ri != f(1.0), name
            elif "outside" in name:
                assert f(0.0) < ri < f(0.75) or f(1.25) < ri < f(np.inf), name
            elif "above" in name:
                assert f(1.25) < ri < f(np.inf), name
            elif "below" in name:
                assert f(0.0) < ri < f(0.75), name
            elif name.startswith("expf = inf"):
                assert ri == f(np.inf) and log_ratio == 100.0, name
            else:
                assert name.startswith("expf = 0") and ri == f(0.0) and log_ratio == -200.0, name
        varms, d = pe.value_arm(inp["values"], inp["target_values"], inp["returns"], pe.TIE_CLIP)
        assert varms == [row[4] for row in vrow], list(zip([row[0] for row in vrow], varms))
        steps = {row[0]: di for row, di in zip(vrow, d)}
        if not overflow:
            assert steps["step == +eps"] == f(0.25) and steps["step == -eps"] == f(-0.25)               # on the closed interval's ends
            v, vt = inp["values"].reshape(-1), inp["target_values"].reshape(-1)
            i, j = [row[0] for row in vrow].index("rounded up inside"), [row[0] for row in vrow].index("rounded down inside")
            assert vt[i] + (v[i] - vt[i]) == np.nextafter(v[i], f(1)) and vt[j] + (v[j] - vt[j]) == np.nextafter(v[j], f(0))
    # the kernel's log-prob of these rows (float64 sum of the float column terms, the constant in float64) is old_log_prob to < 2^-25:
    # expf of that is 1.0f whichever way it rounds
    g = pe.tie_inputs(A)["groups"][0]
    d = g["actions"][0] - g["mu"][0]
    lp = (-(d * d) / f(2)).astype(np.float64).sum() - A * 0.5 * np.log(2 * np.pi)
    assert abs(lp - np.float64(g["old_log_prob"][0, 0])) < 2.0 ** -25 and np.exp(f(lp - np.float64(g["old_log_prob"][0, 0]))) == f(1)
    # the float32 clip bounds the rows are built against are exact
    assert f(1 - pe.TIE_CLIP) == 0.75 and f(1 + pe.TIE_CLIP) == 1.25 and f(2 * pe.TIE_CLIP) == 0.5 and float(f(pe.TIE_CLIP)) == pe.TIE_CLIP


def test_tie_rows_give_the_gradients_the_table_states():
    """The value table's third column against torch's own float32 autograd (clip 0.25, coef 1): d term / d v = B * grad_values."""
    for overflow, vrow in ((False, pe.VALUE_ROWS), (True, pe.VALUE_OVERFLOW_ROWS)):
        inp = pe.tie_inputs(1, overflow)
        got = pc.restate(inp, True, False, 0.0, clip=pe.TIE_CLIP, dtype=torch.float32)["grad_values"].reshape(-1) * len(vrow)
        for (name, _, _, _, _, want), x in zip(vrow, got):
            if want is not None:
                assert x == want, (name, x, want)
    # Adv = +-0 rows: term and gradients are zero (of either sign) in torch's float32 autograd
    for A in pe.TIE_WIDTHS:
        for spo in (False, True):
            ref = pc.restate(pe.tie_inputs(A), True, spo, 0.0, clip=pe.TIE_CLIP, dtype=torch.float32)
            zero = [i for i, row in enumerate(pe.POLICY_ROWS) if row[1] == 0.0]
            assert len(zero) == 4 and (ref["grad_mu"][0][zero] == 0).all() and (ref["grad_sigma"][0][zero] == 0).all()


def test_every_arm_of_both_selectors_is_present():
    """Over the hand-built rows of part B and the NaN rows of part C, in torch float32 on the CPU."""
    policy, value = set(), set()
    for A in pe.TIE_WIDTHS:
        for overflow in (False, True):
            inp = pe.tie_inputs(A, overflow)
            policy |= set(pe.policy_arm(inp["groups"][0], pe.TIE_CLIP)[0])
            value |= set(pe.value_arm(inp["values"], inp["target_values"], inp["returns"], pe.TIE_CLIP)[0])
    assert policy == set(pe.POLICY_ARMS) - {"nan"} and value == set(pe.VALUE_ARMS) - {"nan"}
    for base in pe.NAN_BASES:
        c, group = pe.nan_case(base, "advantages")
        inp = pc.make_inputs(c)
        row, col = pe.nan_places(c, group, "advantages")[0]
        arms, _ = pe.policy_arm(pe.with_nan(inp, group, "advantages", row, col)["groups"][group], pc.CLIP)
        assert arms[row] == "nan" and arms.count("nan") == 1
        policy.add(arms[row])
        row, col = pe.nan_places(c, group, "target_values")[1]
        bad = pe.with_nan(inp, group, "target_values", row, col)
        varms, _ = pe.value_arm(bad["values"], bad["target_values"], bad["returns"], pc.CLIP)
        assert varms[row] == "nan" and varms.count("nan") == 1
        value.add(varms[row])
    assert policy == set(pe.POLICY_ARMS) and value == set(pe.VALUE_ARMS)


# ---- C. the reach of a NaN ------------------------------------------------------------------------------------------------------------------------
def test_nan_places_cover_what_they_should():
    for base, (c0, group) in pe.NAN_BASES.items():
        p = pe.plan(c0)
        for tensor in pe.GROUP_TENSORS + pe.VALUE_TENSORS:
            c, g = pe.nan_case(base, tensor)
            assert g == group and c["rows"] == c0["rows"] and c["seed"] == c0["seed"]
            places = pe.nan_places(c, g, tensor)
            B = c["vrows"] if tensor in pe.VALUE_TENSORS else c["rows"][g]
            per_tile = pe.THREADS if tensor in pe.VALUE_TENSORS else p["per_tile"]
            assert B % per_tile != 0 and (B - 1) in [r for r, _ in places]                            # the last row of a ragged last tile
            assert all(0 <= r < B for r, _ in places)
            if tensor in ("mu", "sigma", "actions", "old_mu", "old_sigma"):
                assert (c["A"] - 1) in [col for _, col in places] and len({r for r, _ in places}) == 3
    assert pe.NAN_BASES["w33"][0]["A"] % 4 == 1 and pe.NAN_BASES["cts_17_5"][1] == 1                  # a scalar-tail quad; group 1
    # the same inputs with and without group 1's old columns
    a, b = pc.make_inputs(pe.nan_case("cts_17_5", "mu")[0]), pc.make_inputs(pe.nan_case("cts_17_5", "old_mu")[0])
    assert a["groups"][1]["old_mu"] is None and b["groups"][1]["old_mu"] is not None
    assert all(np.array_equal(a["groups"][1][k], b["groups"][1][k]) for k in ("mu", "sigma", "actions", "old_log_prob", "advantages"))


@pytest.mark.parametrize("tensor", pe.GROUP_TENSORS + pe.VALUE_TENSORS)
def test_nan_reach_is_the_restatement_s_except_for_target_values(tensor):
    """nan_reach (include/lgppo.h's rule) against torch's float32 autograd on the two-group base: the same scalars and gradient rows turn
    NaN and no others -- except grad_values under a NaN target value, where torch.max's backward hands the full gradient to both
    operands, clamp's backward zeroes the clipped one, and autograd returns the finite 2 (v - R) coef / B.  The kernel returns NaN there
    (DESIGN.md section 11); this test pins the departure."""
    c, group = pe.nan_case("cts_17_5", tensor)
    inp = pc.make_inputs(c)
    row, col = pe.nan_places(c, group, tensor)[0]
    ref = pc.restate(pe.with_nan(inp, group, tensor, row, col), **pe.cfg(c), dtype=torch.float32)
    scalars, grads = pe.nan_reach(tensor, group, c["kl"][group], c["clipped"])
    for name, x in pc.outputs(ref):
        if np.ndim(x) == 0:
            assert bool(np.isnan(x)) == (name in scalars), (tensor, name)
        elif name == "grad_values" and tensor == "target_values":
            v, R = inp["values"][row, 0], inp["returns"][row, 0]
            assert not np.isnan(x).any() and x[row, 0] == np.float32(np.float32(2) * (v - R)) * np.float32(1.0 / c["vrows"])
        else:
            nan_rows = np.isnan(x).any(axis=1)
            assert np.array_equal(np.flatnonzero(nan_rows), [row] if name in grads else []), (tensor, name)
            assert np.isnan(x[nan_rows]).all()
    # the issue's own example: v = 1, R = 0, v_t = NaN -> loss NaN, gradient 2.0
    one = dict(pe.tie_inputs(1), values=np.ones((1, 1), np.float32), returns=np.zeros((1, 1), np.float32), target_values=np.full((1, 1), np.nan, np.float32))
    ref = pc.restate(one, True, False, 0.0, clip=pe.TIE_CLIP, dtype=torch.float32)
    assert np.isnan(ref["loss"]) and ref["grad_values"][0, 0] == 2.0


# ---- D. the clip key ----------------------------------------------------------------------------------------------------------------------------------
def _make_inputs_before_the_clip_key(c):
    """make_inputs as it stood before it took `clip`: the draws of the existing cases are held to it bit for bit."""
    rng = np.random.default_rng(c["seed"])
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    A, groups = c["A"], []
    for B, kl in zip(c["rows"], c["kl"]):
        mu, sigma = f(rng.normal(size=(B, A)) * 0.5), f(0.3 + 0.9 * rng.random((B, A)))
        old_mu, old_sigma = f(mu + 0.1 * sigma * rng.normal(size=(B, A))), f(sigma * np.exp(0.05 * rng.normal(size=(B, A))))
        actions = f(old_mu + old_sigma * rng.normal(size=(B, A)))
        groups.append(dict(mu=mu, sigma=sigma, actions=actions, old_log_prob=pc.old_log_prob_for(mu, sigma, actions, pc.gap_ratio(rng, B)).reshape(B, 1),
                           advantages=f(rng.normal(size=(B, 1))), old_mu=old_mu if kl else None, old_sigma=old_sigma if kl else None))
    Bv = c["vrows"]
    values = f(rng.normal(size=(Bv, 1)))
    target_values = f(values.astype(np.float64) - pc.gap_step(rng, Bv).reshape(Bv, 1))
    returns = f(target_values + 0.5 * rng.normal(size=(Bv, 1)))
    return dict(groups=groups, values=values, returns=returns, target_values=target_values)


def _same_inputs(a, b, keys=pe.GROUP_TENSORS, value_keys=pe.VALUE_TENSORS):
    same = lambda x, y: (x is None and y is None) or (x.dtype == y.dtype and x.tobytes() == y.tobytes())
    return all(same(ga[k], gb[k]) for ga, gb in zip(a["groups"], b["groups"]) for k in keys) and all(same(a[k], b[k]) for k in value_keys)


def test_clip_key_leaves_the_existing_draws_alone():
    for name, c in pc.CASES.items():
        assert "clip" not in c
        assert _same_inputs(pc.make_inputs(name), _make_inputs_before_the_clip_key(c)), name
    # another clip moves the two placed columns and nothing else: the random stream is consumed alike
    c = pc.CASES["b257_a12"]
    a, b = pc.make_inputs(c), pc.make_inputs(dict(c, clip=0.3))
    free = tuple(k for k in pe.GROUP_TENSORS if k != "old_log_prob")
    assert _same_inputs(a, b, keys=free, value_keys=("values",)) and not _same_inputs(a, b, keys=("old_log_prob",), value_keys=("target_values",))


def test_clip_cases_sit_on_both_sides_of_their_own_boundaries():
    assert {(c["clip"], c["value_loss_coef"]) for c in pe.CLIP_CASES.values()} == {(0.1, 0.5), (0.1, 2.0), (0.3, 0.5), (0.3, 2.0)}
    assert len(pe.CLIP_CASES) == 12 and {c["spo"] for c in pe.CLIP_CASES.values()} == {False, True}
    for name, c in pe.CLIP_CASES.items():
        pc.assert_both_sides(name, pc.make_inputs(c), c["clip"])
        assert pe.cfg(c)["clip"] == c["clip"] and pe.cfg(c)["value_loss_coef"] == c["value_loss_coef"]

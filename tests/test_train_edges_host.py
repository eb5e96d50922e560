"""Host side of the train passes' edge table (tests/train_edges.py): every row plans the row tile it states, in lg_train_plan /
lg_train_ee_plan / lg_train_est_plan and in the restated plans; every tag a row claims follows from its plan; the table as a whole keeps
the paths it is there for; the float32 restatement in the kernel's order stays within HALF the parity rule's factor at every case (so no
GPU comparison is decided by the draw); three wrong variants at the new shapes fail the rule; and the restatement still is torch's
float64 autograd there.  No GPU needed: nothing is launched."""
import numpy as np
import pytest
import torch

from hcr_genesis_lr_cl_amd import abi, train
from tests import train_cases as tc
from tests import train_edges as te
from tests import train_ee_cases as ec
from tests.optim_cases import PARITY_FACTOR

IDS = [te.case_id(c) for c in te.CASES]


# ---- the table reaches what it claims ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", te.CASES, ids=IDS)
def test_every_row_plans_its_tile_and_reaches_its_tags(case):
    row, B = case
    d, w, t = te.ROWS[row], te.widths(row), te.reach_tags(row, B)
    if d["kind"] == "plain":
        p = train.plan(B, *w)
        assert p.row_tile == d["R"] == t["row_tile"][0] and p.lds_bytes == t["lds_bytes"][0] and p.weight_jobs == t["weight_jobs"][0]
        got = [(S, per) for ci, c in enumerate(w) for S, per in zip(list(p.slices[ci])[:len(c) - 1], list(p.slice_rows[ci])[:len(c) - 1])]
        got.append((p.std_slices, p.std_slice_rows))
    else:
        p, q = train.plan_ee(B, *w), train.plan_est(B, w[0])
        assert (p.row_tile, q.row_tile) == d["R"] == t["row_tile"] and (p.lds_bytes, q.lds_bytes) == t["lds_bytes"]
        assert p.est_first_buffer == t["est_first_buffer"] and q.loss_tiles == t["loss_tiles"] == -(-B // q.row_tile)
        got = [(S, per) for ci, c in ((abi.TRAIN_EE_ACTOR, w[1]), (abi.TRAIN_EE_CRITIC, w[2]))
               for S, per in zip(list(p.slices[ci])[:len(c) - 1], list(p.slice_rows[ci])[:len(c) - 1])]
        got.append((p.std_slices, p.std_slice_rows))
        got += list(zip(list(q.slices[0])[:len(w[0]) - 1], list(q.slice_rows[0])[:len(w[0]) - 1]))
    assert got == [s[:2] for s in t["slices"]]
    assert all(S >= 1 and 0 < last <= per and (S - 1) * per + last == B for S, per, last in t["slices"])
    missing = te.claimed(row, B) - te.tags(row, B)
    assert not missing, (case, missing, sorted(te.tags(row, B)))


def test_the_table_keeps_the_paths_it_is_there_for():
    reached = {(row, B): te.claimed(row, B) for row, B in te.CASES}
    everything = set().union(*reached.values())
    assert te.TABLE_TAGS <= everything, te.TABLE_TAGS - everything
    plain = {k: v for k, v in reached.items() if te.ROWS[k[0]]["kind"] == "plain"}
    for tag in ("R=16", "R=8", "nt4-ragged-fwd", "nt4-ragged-bwd", "S=32", "unequal-S", "max-width"):          # in the plain pass itself
        assert any(tag in v for v in plain.values()), tag
    assert any({"S=31", "last-slice%4!=0"} <= v for v in plain.values()) and any({"S=32", "last-slice%4!=0"} <= v for v in plain.values())
    ee8 = {k: v for k, v in reached.items() if te.ROWS[k[0]]["kind"] == "ee" and "R=8" in v}
    assert {"efb=0", "efb=1"} <= set().union(*ee8.values())                  # both placements of the estimator's input at R = 8
    assert any("loss-tiles>256" in v for v in ee8.values())                  # the second finalize trip from 8-row tiles too
    assert {"loss-tiles=257", "loss-tiles=258"} <= set().union(*reached.values())     # the second trip holding one partial, and two
    # what the old tables stop short of
    assert max(c["B"] for c in tc.CASES.values()) <= 257 and max(c["B"] for c in ec.CASES.values()) <= 257
    assert all(tc.restated_plan(c["B"], *tc.NETS[c["net"]])["row_tile"] == 32 for c in tc.CASES.values())
    assert all(ec.restated_plan_est(c["B"], ec.NETS[c["net"]][0])["loss_tiles"] <= te.FINALIZE_TRIP for c in ec.CASES.values())
    assert "_edge" not in tc.NETS and "_edge" not in ec.NETS                  # the old tables are as they were
    # the tag rules at their thresholds
    assert [te.nt_of(w) for w in (1, 64, 65, 192, 193, 2048)] == [1, 1, 2, 2, 4, 4]
    assert te._nt4_ragged(197) and te._nt4_ragged(209) and not te._nt4_ragged(256) and not te._nt4_ragged(193 - 1) and not te._nt4_ragged(250)
    assert te.reach_tags("r8", 25)["lds_bytes"] == (131328,) and te.reach_tags("max", 13)["weight_jobs"] == (3137,)
    t = te.reach_tags("go2", 2049)
    assert {s[0] for s in t["slices"]} == {31, 16} and te.reach_tags("tiny", 2049)["slices"][0] == (31, 68, 9)
    assert te.reach_tags("tiny", 2113)["slices"][0] == (32, 68, 5) and tc.MAX_SLICES == 32


def test_the_strided_rows_are_the_16_byte_path():
    """Every matrix of the strided test is a multiple of 4 wide; placement `vector` keeps base and stride on 16 bytes with stride != width,
    the other two break exactly one of the two."""
    for w in te.VEC_PLAIN + te.VEC_EE:
        assert w[0] % 4 == 0 and w[-1] % 4 == 0
    assert te.VEC_EE[1][0] == te.VEC_EE[0][0] + te.VEC_EE[0][-1]
    off, stride = te.PLACEMENTS["vector"]
    assert off % 4 == 0 and stride % 4 == 0 and stride > off + max(w[0] for w in te.VEC_PLAIN + te.VEC_EE)
    off, stride = te.PLACEMENTS["misaligned_base"]
    assert off % 4 != 0 and stride % 4 == 0
    off, stride = te.PLACEMENTS["odd_stride"]
    assert off % 4 == 0 and stride % 4 != 0


# ---- the reference alone stays inside the rule ------------------------------------------------------------------------------------------------
HALF = []


@pytest.mark.parametrize("case", te.CASES, ids=IDS)
def test_float32_in_kernel_order_stays_within_half_the_rule(case):
    row, B = case
    x, (r64, r32) = te.inputs(row, B), te.references(row, B)
    ps = te.plans(row, B)
    got = te.f32_in_kernel_order(x, ps[0] if len(ps) == 1 else ps)
    worst = te.check(row, got, r64, r32, te.case_id(case) + " numpy f32 in kernel order", HALF)
    assert max(worst.values()) <= te.HALF_FACTOR == PARITY_FACTOR / 2, (case, worst)
    if x["clip"] is not None:                                        # the Hardtanh still masks some means and passes others
        sat = np.abs(r64["mu"]) >= x["clip"]
        print(f"{te.case_id(case)}: {sat.mean():.4f} of the means saturate")
        assert B * x["actor"][-1] < 64 or 0 < sat.sum() < sat.size


def test_zz_print_the_float32_ratios():
    worst = {}
    for _, ratios in HALF:
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for k, v in worst.items():
        print(f"NUMPY-F32 {k}: {v:.3f} over {len(HALF)} checks")


# ---- discrimination at the new shapes -----------------------------------------------------------------------------------------------------------
def test_dropping_nine_of_2049_rows_fails_the_rule():
    x, (r64, r32) = te.inputs("tiny", 2049), te.references("tiny", 2049)
    p = te.plans("tiny", 2049)[0]
    per = (p["std"][1], *p["slice_rows"])
    assert te.reach_tags("tiny", 2049)["last_slice"] == [9]
    bad = tc.named(x, tc.forward(x), tc.backward(x, wrong="drop_last_slice", slices=per))
    assert te.worst_ratio(bad, r64, r32) > 1.0
    with pytest.raises(AssertionError):
        tc.check_parity(bad, r64, r32, "tiny_b2049 without its last slice")
    tc.check_parity(tc.named(x, tc.forward(x), tc.backward(x, slices=per)), r64, r32, "tiny_b2049 sliced, float64")      # the slicing itself is no error


def test_a_finalize_that_stops_at_256_partials_fails_the_rule():
    x, (r64, r32) = te.inputs("fixture", 8193), te.references("fixture", 8193)
    est = te.plans("fixture", 8193)[1]
    assert est["loss_tiles"] == te.FINALIZE_TRIP + 1
    d = ec.est_pass(x)["d"]
    whole = te.loss_by_tiles(d, est["row_tile"])
    assert abs(whole - float(r64["loss"][0])) <= 1e-12 * whole
    bad = dict(r64, loss=np.asarray(te.loss_by_tiles(d, est["row_tile"], keep=te.FINALIZE_TRIP)).reshape(1))
    assert te.worst_ratio(bad, r64, r32) > 1.0
    with pytest.raises(AssertionError):
        ec.check_parity(bad, r64, r32, "fixture_b8193 without the second trip")


def test_a_lost_row_clamp_fails_the_rule():
    x, (r64, r32) = te.inputs("r8", 25), te.references("r8", 25)
    bad = dict(r64, mu=te.lost_row_clamp(r64["mu"]), values=te.lost_row_clamp(r64["values"]))
    assert np.array_equal(bad["mu"][:8], r64["mu"][:8]) and np.array_equal(bad["mu"][8:16], r64["mu"][:8]) and np.array_equal(bad["mu"][24], r64["mu"][16])
    for k in ("mu", "values"):                                        # each output alone is caught
        assert te.worst_ratio(dict(r64, **{k: bad[k]}), r64, r32) > 1.0, k
    with pytest.raises(AssertionError):
        tc.check_parity(bad, r64, r32, "r8_b25 with rows 8..15 of each group from rows 0..7")


# ---- the restatement is torch's float64 autograd at the new rows --------------------------------------------------------------------------------
AUTOGRAD_CASES = [("r16", 17), ("r8", 9), ("max", 13), ("nt4r", 33), ("tiny", 2049), ("go2", 2049), ("fixture", 2049), ("ee_wide8_a", 9), ("ee_wide8_b", 9)]


@pytest.mark.parametrize("case", AUTOGRAD_CASES, ids=[te.case_id(c) for c in AUTOGRAD_CASES])
def test_restatement_matches_torch_float64_autograd(case):
    row, B = case
    assert case in te.CASES and {c[0] for c in AUTOGRAD_CASES} >= {r for r in te.ROWS if "net" not in te.ROWS[r]}
    x, (r64, _) = te.inputs(row, B), te.references(row, B)
    if te.ROWS[row]["kind"] == "plain":
        t = tc.torch_pass(x, torch.float64)
        want = tc.named(x, t, t["grads"])
    else:
        t = ec.torch_passes(x, torch.float64)
        want = ec.named(x, t, t["rl_grads"], t["loss"], t["est_grads"])
    assert set(want) == set(r64)
    for name, ref in want.items():
        assert tc.max_err(r64[name], ref) <= 1e-12 * max(1.0, np.abs(ref).max()), name
    # and the per-layer slicing of the restatement changes nothing in float64
    ps = te.plans(row, B)
    if len(ps) == 1:
        sliced = tc.named(x, tc.forward(x), tc.backward(x, slices=(ps[0]["std"][1], *ps[0]["slice_rows"])))
    else:
        e = ec.est_pass(x, slices=ps[1]["slice_rows"][0])
        sliced = ec.named(x, ec.rl_forward(x), ec.rl_backward(x, slices=(ps[0]["std"][1], *ps[0]["slice_rows"])), e["loss"], e["grads"])
    for name, ref in want.items():
        assert tc.max_err(sliced[name], ref) <= 1e-12 * max(1.0, np.abs(ref).max()), name

"""Host side of the train passes' edge table (tests/train_edges.py), plain, EE and teacher-student (TS) rows alike: every row plans the row
tile it states, in lg_train_plan / lg_train_ee_plan / lg_train_est_plan / lg_train_ts_plan / lg_train_enc_plan and in the restated plans
(a TS row its enc_first_buffer too); every tag a row claims follows from its plan; the table as a whole, and its TS rows by themselves,
keep the paths they are there for; the float32 restatement in the kernel's order stays within HALF the parity rule's factor at every case
(so no GPU comparison is decided by the draw); wrong variants at the new shapes fail the rule; and the restatement still is torch's
float64 autograd there.  No GPU needed: nothing is launched."""
import numpy as np
import pytest
import torch

from hcr_genesis_lr_cl_amd import abi, train
from tests import train_cases as tc
from tests import train_edges as te
from tests import train_ee_cases as ec
from tests import train_ts_cases as sc
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
    elif d["kind"] == "ts":
        p, q = train.plan_ts(B, *w[:3]), train.plan_enc(B, w[3], w[0])
        assert (p.row_tile, q.row_tile) == d["R"] == t["row_tile"] and (p.lds_bytes, q.lds_bytes) == t["lds_bytes"]
        assert (p.weight_jobs, q.weight_jobs) == t["weight_jobs"]
        assert p.enc_first_buffer == t["enc_first_buffer"] and f"efb={p.enc_first_buffer}" in te.claimed(row, B)
        assert q.loss_tiles == t["loss_tiles"] == -(-B // q.row_tile)
        got = [(S, per) for ci, c in ((abi.TRAIN_TS_PRIVILEGE, w[0]), (abi.TRAIN_TS_ACTOR, w[1]), (abi.TRAIN_TS_CRITIC, w[2]))
               for S, per in zip(list(p.slices[ci])[:len(c) - 1], list(p.slice_rows[ci])[:len(c) - 1])]
        got.append((p.std_slices, p.std_slice_rows))
        got += list(zip(list(q.slices[abi.TRAIN_TS_HISTORY])[:len(w[3]) - 1], list(q.slice_rows[abi.TRAIN_TS_HISTORY])[:len(w[3]) - 1]))
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


def test_the_teacher_student_rows_keep_the_paths_they_are_there_for():
    """TS_TABLE_TAGS from the TS rows alone, and the combinations the kernels' own code paths need: both placements of the privilege
    encoder under the 8-row tile, Z = 65 there, the 16-row tile in BOTH passes, a four-layer privilege encoder, differing tiles, 31 and 32
    slices with ragged last ones, and the finalize's second trip from 8-row tiles."""
    ts = {(row, B): te.claimed(row, B) for row, B in te.CASES if te.ROWS[row]["kind"] == "ts"}
    everything = set().union(*ts.values())
    assert te.TS_TABLE_TAGS <= everything, te.TS_TABLE_TAGS - everything
    assert te.TS_TABLE_TAGS >= {"R=16", "R=8", "efb=0", "efb=1", "priv-layers=4", "Z>16", "R-differs", "S=31", "S=32", "last-slice%4!=0", "unequal-S",
                                "loss-tiles>256"}
    r8 = {k: v for k, v in ts.items() if te.ROWS[k[0]]["R"] == (8, 8)}
    assert {"efb=0", "efb=1"} <= set().union(*r8.values())                   # both placements of the privilege encoder at R = 8
    assert any({"efb=1", "loss-tiles>256", "S=31"} <= v for v in r8.values())  # the second finalize trip from 8-row tiles
    assert any({"Z>16", "efb=0", "tiles>2"} <= v and te.widths(k[0])[0][-1] == 65 for k, v in r8.items())
    r16 = {k: v for k, v in ts.items() if te.ROWS[k[0]]["R"] == (16, 16)}    # the 16-row tile in both passes, never planned before
    assert any({"Z>16", "efb=1", "nt4-ragged-fwd", "nt4-ragged-bwd"} <= v for v in r16.values())
    assert any({"S=31", "unequal-S", "last-slice=9"} <= v for v in r16.values())
    for need in ("one-row-tile", "tile-one-short", "tile-one-over", "tiles>2"):
        assert any(need in v for v in r16.values()) and any(need in v for v in r8.values()), need
    assert any({"priv-layers=4", "S=31", "last-slice=9"} <= v for v in ts.values()) and any({"priv-layers=4", "S=32", "last-slice=5"} <= v for v in ts.values())
    assert any({"R-differs", "R=8", "R=32", "loss-tiles=2"} <= v for v in ts.values())     # differing tiles with more than one encoder tile
    assert any({"R-differs", "unequal-S", "multi-tile-gradients"} <= v for v in ts.values())
    assert {len(te.widths(r)[0]) - 1 for r, d in te.ROWS.items() if d["kind"] == "ts"} == {1, 2, 3, 4}
    # what the TS case table stops short of: no 16-row tile in both passes, the 8-row tile on net `wide` alone, no four-layer encoder
    def rt(c):
        priv, actor, critic, hist = sc.NETS[c["net"]]
        return sc.restated_plan_ts(c["B"], priv, actor, critic)["row_tile"], sc.restated_plan_enc(c["B"], hist, priv)["row_tile"]
    tiles = {name: rt(c) for name, c in sc.CASES.items()}
    assert (16, 16) not in tiles.values() and {n for n, r in tiles.items() if 8 in r} == {"wide_b1", "wide_b9"}
    assert max(len(n[0]) - 1 for n in sc.NETS.values()) == 3 and "_edge" not in sc.NETS
    # the plans as the issue's table states them
    t = te.reach_tags("ts_r16", 2049)
    assert {s[0] for s in t["slices"]} == {31, 16} and t["last_slice"] == [9] and t["loss_tiles"] == 129 and t["lds_bytes"] == (90624, 90624 + sc.RED_BYTES)
    assert te.reach_tags("ts_r8_even", 2049)["loss_tiles"] == te.FINALIZE_TRIP + 1 and te.reach_tags("ts_r8_even", 9)["lds_bytes"][0] == 8 * 2 * 1348 * 4
    assert te.reach_tags("ts_deep4", 2113)["slices"][0] == (32, 68, 5) and te.reach_tags("ts_mix", 41)["row_tile"] == (8, 32)


def test_the_strided_rows_are_the_16_byte_path():
    """Every matrix of the strided test is a multiple of 4 wide; placement `vector` keeps base and stride on 16 bytes with stride != width,
    the other two break exactly one of the two."""
    for w in te.VEC_PLAIN + te.VEC_EE + te.VEC_TS:
        assert w[0] % 4 == 0 and w[-1] % 4 == 0
    assert te.VEC_EE[1][0] == te.VEC_EE[0][0] + te.VEC_EE[0][-1]
    priv, actor, _, hist = te.VEC_TS
    assert actor[0] - priv[-1] == 12 and priv[-1] == hist[-1] == 4           # O = 12: the observations and the latent both on 16 bytes
    off, stride = te.PLACEMENTS["vector"]
    assert off % 4 == 0 and stride % 4 == 0 and stride > off + max(w[0] for w in te.VEC_PLAIN + te.VEC_EE)
    for off, stride in te.PLACEMENTS.values():                               # the 20-column history fits every placement, flush right in `vector`
        assert stride >= off + max(w[0] for w in te.VEC_TS) and stride != max(w[0] for w in te.VEC_TS)
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


# ---- discrimination at the teacher-student rows: each a change of the float64 restatement, none touches a kernel ----------------------------------
def _fails(row, bad, r64, r32, label, match=None):
    assert te.worst_ratio(bad, r64, r32) > 1.0, label
    with pytest.raises(AssertionError, match=match):
        te.check(row, bad, r64, r32, label)


def test_ts_dropping_the_nine_row_slice_of_the_privilege_encoder_fails_the_rule():
    x, (r64, r32) = te.inputs("ts_deep4", 2049), te.references("ts_deep4", 2049)
    rl_s, _, _ = sc.kernel_order_slices(x)
    assert te.reach_tags("ts_deep4", 2049)["last_slice"] == [9] and set(rl_s["priv"]) == {68}
    named = lambda grads: dict(r64, **dict(zip(sc.rl_names(x["actor"], x["critic"], x["priv"]), grads)))
    bad = named(sc.rl_backward(x, slices=rl_s, wrong="priv_drop_last_slice"))
    assert all(np.array_equal(bad[k], v) for k, v in named(sc.rl_backward(x, slices=rl_s)).items() if not k.startswith("privilege_encoder"))
    _fails("ts_deep4", bad, r64, r32, "ts_deep4_b2049 without the privilege encoder's last slice", r"privilege_encoder\.\d\.(weight|bias)")
    for k in (k for k in r64 if k.startswith("privilege_encoder")):          # every one of its eight tensors alone is caught
        assert te.worst_ratio(dict(r64, **{k: bad[k]}), r64, r32) > 1.0, k
    te.check("ts_deep4", named(sc.rl_backward(x, slices=rl_s)), r64, r32, "ts_deep4_b2049 sliced, float64")          # the slicing itself is no error
    with pytest.raises(ValueError):
        sc.rl_backward(x, wrong="priv_drop_last_slice")


def test_ts_a_finalize_that_stops_at_256_partials_of_8_rows_fails_the_rule():
    x, (r64, r32) = te.inputs("ts_r8_even", 2049), te.references("ts_r8_even", 2049)
    enc = te.plans("ts_r8_even", 2049)[1]
    assert enc["loss_tiles"] == te.FINALIZE_TRIP + 1 and enc["row_tile"] == 8
    d = sc.enc_pass(x)["d"]
    whole = te.loss_by_tiles(d, 8)
    assert abs(whole - float(r64["loss"][0])) <= 1e-12 * whole
    # the 257th tile is row 2048 alone: under the row's default seed 900 + 2049 that row is masked, its partial zero and this defect no
    # error at all, so the case has a seed (tests/train_edges.py) that leaves the row unmasked
    assert x["terminated"][2048, 0] == 1.0 and te.seed_of("ts_r8_even", 2049) != 900 + 2049
    bad = dict(r64, loss=np.asarray(te.loss_by_tiles(d, 8, keep=te.FINALIZE_TRIP)).reshape(1))
    _fails("ts_r8_even", bad, r64, r32, "ts_r8_even_b2049 without the second trip", r"loss")


def test_ts_a_lost_row_clamp_at_8_rows_fails_the_rule():
    _, (r64, r32) = te.inputs("ts_r8_z", 25), te.references("ts_r8_z", 25)
    bad = dict(r64, mu=te.lost_row_clamp(r64["mu"]), values=te.lost_row_clamp(r64["values"]))
    assert np.array_equal(bad["mu"][8:16], r64["mu"][:8]) and np.array_equal(bad["mu"][24], r64["mu"][16])
    for k in ("mu", "values"):
        assert te.worst_ratio(dict(r64, **{k: bad[k]}), r64, r32) > 1.0, k
    _fails("ts_r8_z", bad, r64, r32, "ts_r8_z_b25 with rows 8..15 of each group from rows 0..7", r"mu")


@pytest.mark.parametrize("case", [("ts_r16", 49), ("ts_r8_z", 25)], ids=te.case_id)
def test_ts_a_latent_gradient_from_the_first_columns_fails_the_rule(case):
    """tests/test_train_ts_host.py's column defect where the latent is wider than a 16-column tile and the row tile is small."""
    row, B = case
    x, (r64, r32) = te.inputs(row, B), te.references(row, B)
    assert x["priv"][-1] > 16 and te.ROWS[row]["R"][0] < 32
    names = sc.rl_names(x["actor"], x["critic"], x["priv"])
    bad = dict(r64, **dict(zip(names, sc.rl_backward(x, wrong="latent_cols0"))))
    _fails(row, bad, r64, r32, f"{te.case_id(case)} latent gradient from columns [0, Z)", r"privilege_encoder\.\d\.(weight|bias)")
    assert all(np.array_equal(bad[k], r64[k]) for k in r64 if not k.startswith("privilege_encoder"))


def test_ts_targets_read_back_at_the_other_pass_tile_fail_the_rule():
    """The y region addressed by the RL pass's 8-row tile where the encoder pass plans 32: the target of tile t of 32 rows is taken from rows
    [8 t, 8 t + 32).  The row's first batch, 9 rows, was tried first: it is one tile, t = 0, which the defect leaves as it is (the rule
    passes it, asserted below), so the row got 41 rows, whose second tile then reads rows 8..16."""
    assert te.ROWS["ts_mix"]["R"] == (8, 32)

    def wrong_targets(B):
        x, (r64, r32) = te.inputs("ts_mix", B), te.references("ts_mix", B)
        rows = np.arange(B)
        src = 8 * (rows // 32) + rows % 32                                   # the row whose target row r gets
        e = sc.enc_pass(dict(x, privileged_obs=x["privileged_obs"][src]))    # a target is a function of its own row alone
        return x, r64, r32, dict(loss=np.asarray(e["loss"]).reshape(1), **dict(zip(sc.enc_names(x["hist"]), e["grads"])))
    x, r64, r32, bad = wrong_targets(9)
    assert all(np.array_equal(bad[k], r64[k]) for k in bad)
    x, r64, r32, bad = wrong_targets(41)
    _fails("ts_mix", dict(r64, **bad), r64, r32, "ts_mix_b41 with the targets of tile 1 from rows 8..16", r"loss|history_encoder")
    assert te.worst_ratio(dict(r64, loss=bad["loss"]), r64, r32) > 1.0       # the loss alone is caught
    for k in sc.enc_names(x["hist"]):                                         # and each gradient of the history encoder alone
        assert te.worst_ratio(dict(r64, **{k: bad[k]}), r64, r32) > 1.0, k


# ---- the restatement is torch's float64 autograd at the new rows --------------------------------------------------------------------------------
AUTOGRAD_CASES = [("r16", 17), ("r8", 9), ("max", 13), ("nt4r", 33), ("tiny", 2049), ("go2", 2049), ("fixture", 2049), ("ee_wide8_a", 9), ("ee_wide8_b", 9),
                  ("ts_r16", 17), ("ts_r16", 2049), ("ts_r8_even", 9), ("ts_r8_z", 9), ("ts_deep4", 2049), ("ts_mix", 41), ("ts_fixture", 2049)]


@pytest.mark.parametrize("case", AUTOGRAD_CASES, ids=[te.case_id(c) for c in AUTOGRAD_CASES])
def test_restatement_matches_torch_float64_autograd(case):
    row, B = case
    assert case in te.CASES and {c[0] for c in AUTOGRAD_CASES} >= {r for r in te.ROWS if "net" not in te.ROWS[r]}
    x, (r64, _) = te.inputs(row, B), te.references(row, B)
    if te.ROWS[row]["kind"] == "plain":
        t = tc.torch_pass(x, torch.float64)
        want = tc.named(x, t, t["grads"])
    elif te.ROWS[row]["kind"] == "ts":
        t = sc.torch_passes(x, torch.float64)
        want = sc.named(x, t, t["rl_grads"], t["loss"], t["enc_grads"])
        assert all(g is None for g in t["enc_rl_grads"]) and all(g is None for g in t["priv_enc_grads"])
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
    elif te.ROWS[row]["kind"] == "ts":
        rl_s, enc_s, tile = sc.kernel_order_slices(x)
        e = sc.enc_pass(x, slices=enc_s, row_tile=tile)
        sliced = sc.named(x, sc.rl_forward(x), sc.rl_backward(x, slices=rl_s), e["loss"], e["grads"])
    else:
        e = ec.est_pass(x, slices=ps[1]["slice_rows"][0])
        sliced = ec.named(x, ec.rl_forward(x), ec.rl_backward(x, slices=(ps[0]["std"][1], *ps[0]["slice_rows"])), e["loss"], e["grads"])
    for name, ref in want.items():
        assert tc.max_err(sliced[name], ref) <= 1e-12 * max(1.0, np.abs(ref).max()), name

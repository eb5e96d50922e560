"""Host side of the recurrent pass's edge table (tests/train_rnn_edges.py): every tag a row claims follows from the restated plan, the
drawn lengths and the restated index kernel, which reproduces rc.positions on every row; lg_train_rnn_plan equals the restated plan,
unequal memories included; the float64 restatement is torch's float64 autograd there; the float32 restatement in the kernels' order of
sums stays within HALF the parity rule's factor (so no GPU comparison is decided by the draw); the clipped share of the means; four planted
defects that the rule catches by a large factor where they apply and that change nothing where they do not; the saturated rows saturate.
No GPU needed: nothing is launched."""
import hashlib

import numpy as np
import pytest

from tests import train_rnn_cases as rc
from tests import train_rnn_edges as re
from tests import train_support as sup
from tests.test_train_rnn_host import _check_plan


# ---- the table reaches what it claims ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", re.NAMES)
def test_every_row_reaches_its_tags(name):
    x = re.inputs(name)
    missing = set(re.ROWS[name]["reach"]) - re.tags(name)
    assert not missing, (name, missing, sorted(re.tags(name)))
    # the restated index kernel is rc.positions: the same steps in the same order on the same rows, and the region the kernel must leave
    idx, (t, j, row) = re.index_kernel(x["lens"], x["T"], x["E"]), rc.positions(x["lens"], x["T"], x["E"])
    assert all(np.array_equal(a, b) for a, b in zip(idx["rows"], (t, j, row)))
    lens, first, row_map = re.index_region(x)
    assert np.array_equal(idx["first"], first) and np.array_equal(idx["map"], row_map) and lens.sum() == x["T"] * x["E"] == len(set(row.tolist()))
    assert idx["per"] == -(-x["n_traj"] // re.THREADS) and idx["ranges"][0][0] == 0 and max(je for _, je in idx["ranges"]) == x["n_traj"]
    assert all(a[1] == b[0] for a, b in zip(idx["ranges"], idx["ranges"][1:]))                  # the chunks tile the trajectories


def test_the_table_keeps_the_paths_it_is_there_for():
    claimed = {n: set(re.ROWS[n]["reach"]) for n in re.NAMES}
    everything = set().union(*claimed.values())
    assert re.TABLE_TAGS <= everything, re.TABLE_TAGS - everything
    xs = {n: re.inputs(n) for n in re.NAMES}
    assert all(xs[n]["n_traj"] > re.THREADS for n in re.IDX_ROWS) and [re.index_kernel(xs[n]["lens"], xs[n]["T"], xs[n]["E"])["per"] for n in re.IDX_ROWS] == [2, 3, 6]
    # what the old table stops short of: one trajectory per thread, T <= 6, equal memories, one K tile, at most 3 slices
    old = {n: rc.make_inputs(n) for n in rc.CASES}
    assert max(x["n_traj"] for x in old.values()) <= re.THREADS and max(x["T"] for x in old.values()) == 6 and max(max(x["obs_widths"]) for x in old.values()) <= sup.WG_TILE
    assert all(rc.mems_of(x)[0] == rc.mems_of(x)[1] for x in old.values())
    assert max(s[3] for x in old.values() for s in re.memory_slices(x, rc.plan_of_case(x))) <= 3
    # the tiles at their thresholds: H16 is the smallest LSTM width of the 16-trajectory tile, a GRU at 512 plans 8 (164 608 B at 16)
    tile = lambda kind, H: rc.plan(12, 2, 7, 2, kind, [(1, H, 11), (1, H, 13)], [H, 8, 3], [H, 8, 1])
    assert re.H16 == 197 and tile("lstm", 196)["time_row_tile"] == 32 and tile("lstm", 197)["time_row_tile"] == 16
    assert tile("gru", 512)["time_row_tile"] == 8 and 16 * (2 * sup.lds_stride(512) + sup.lds_stride(1536)) * 4 == 164608 > sup.LDS_BYTES
    assert tile("gru", 512)["time_lds_bytes"] == 82304 and tile("lstm", 197)["time_lds_bytes"] == 16 * 1356 * 4
    # idx_1497 is the workload's chunking (1496 trajectories) at 32 slices everywhere
    p = rc.plan_of_case(xs["idx_1497"])
    assert -(-1496 // re.THREADS) == 6 and {s[3:] for s in re.memory_slices(xs["idx_1497"], p)} == {(32, 264, 210)} and p["time_tiles"] == 47
    assert re._tile_alone(xs["mix_tile"], 0) == 32 and re._tile_alone(xs["mix_tile"], 1) == 16 == rc.plan_of_case(xs["mix_tile"])["time_row_tile"]


OLD_INPUTS_SHA256 = "07a469721ba5047008cd45da543bb47b5a176b6b283c61b84092d4a4339374b8"


def test_the_old_table_draws_what_it_drew():
    """critic_mem and obs_scale change no case without them: the sha256 over every array of make_inputs of the 13 old cases (dtype, shape,
    bytes; the parameters in the order of the case's names), taken before tests/train_rnn_cases.py learnt them."""
    h = hashlib.sha256()
    for name in rc.CASES:
        x = rc.make_inputs(name)
        for k in ("lens", "masks", "obs", "critic_obs", "h0_a", "c0_a", "h0_c", "c0_c", "grad_mu", "grad_sigma", "grad_values"):
            if x[k] is not None:
                h.update(f"{name}.{k}.{x[k].dtype}.{x[k].shape}".encode() + np.ascontiguousarray(x[k]).tobytes())
        for k in x["names"]:
            v = x["params"][k]
            h.update(f"{name}.{k}.{v.dtype}.{v.shape}".encode() + v.tobytes())
        h.update(repr((x["clip"], x["names"], x["actor_widths"], x["critic_widths"], x["n_traj"], x["max_len"])).encode())
    assert h.hexdigest() == OLD_INPUTS_SHA256


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", re.NAMES)
def test_plan_matches_the_restated_rules(name):
    x = re.inputs(name)
    p = _check_plan(x["T"] * x["E"], x["max_len"], x["n_traj"], x["T"], x["kind"], re.memories(x), x["actor_widths"], x["critic_widths"])
    want = rc.plan_of_case(x)
    assert (p.time_row_tile, p.time_tiles, p.train.row_tile) == (want["time_row_tile"], want["time_tiles"], want["train"]["row_tile"])
    assert f"Rt={p.time_row_tile}" in re.tags(name)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", re.NAMES)
def test_restatement_matches_torch_float64_autograd(name):
    """As tests/test_train_rnn_host.py holds the old table: the float64 restatement, one sum and sliced, against torch's own nn.LSTM /
    nn.GRU, the reference's unpadding and autograd to 1e-12 relative; the clipped share of the means where there is a Hardtanh."""
    x, (ref, _) = re.inputs(name), re.references(name)
    rel = lambda a, b: sup.max_err(a, b) <= 1e-12 * max(1.0, np.abs(b).max())
    for r in (rc.restate(x, np.float64), rc.restate(x, np.float64, sliced=True), rc.restate(x, np.float64, rows=re.index_rows())):
        assert set(ref) == set(r) - {"pre_clip"} == {"mu", "sigma", "values"} | set(x["names"])
        for k, want in ref.items():
            assert r[k].shape == want.shape and rel(r[k], want), k
    if x["clip"] is not None:
        sat = (np.abs(ref["mu"]) >= x["clip"]).mean()
        assert 0.1 <= sat <= 0.9, sat
    else:
        assert name in ("idx_529", "idx_1497")


@pytest.mark.parametrize("name", re.NAMES)
def test_float32_restatement_keeps_half_the_rule(name):
    """A condition on the inputs, verified here: numpy float32 in the kernels' order of sums within factor 4 of the rule's 8.  Every row
    keeps it on its first seed (100 + its position; the largest, idx_1497, at 2.78 on memory_c.rnn.bias_ih_l1): no seed was replaced."""
    x, (r64, r32) = re.inputs(name), re.references(name)
    assert x["seed"] == 101 + re.NAMES.index(name)
    rc.check_parity(rc.restate(x, np.float32, sliced=True), r64, r32, f"numpy f32 {name}", factor=re.HALF_FACTOR)


@pytest.mark.parametrize("name", list(re.SATURATED))
def test_saturated_rows_saturate_and_keep_half_the_rule(name):
    """The observations scaled by SATURATED[name]: at least half of layer 0's gate pre-activations lie beyond 20 in the float64
    restatement, every reference tensor is finite, the restatement still is torch's, and float32 in the kernels' order keeps half the rule."""
    x, (r64, r32) = re.inputs(name, True), re.references(name, True)
    assert x["obs_scale"] == re.SATURATED[name] and np.array_equal(x["lens"], re.inputs(name)["lens"])
    pre = re.layer0_gate_preactivations(x)
    share = (np.abs(pre) > re.SATURATION).mean()
    print(f"{name} x {x['obs_scale']:g}: {share:.3f} of {pre.size} layer-0 gate pre-activations beyond {re.SATURATION:g}, the largest {np.abs(pre).max():.1f}")
    assert share >= 0.5 and all(np.isfinite(v).all() for v in r64.values()) and all(np.isfinite(v).all() for v in r32.values())
    r = rc.restate(x, np.float64)
    assert all(sup.max_err(r[k], v) <= 1e-12 * max(1.0, np.abs(v).max()) for k, v in r64.items())
    assert 0.1 <= (np.abs(r64["mu"]) >= x["clip"]).mean() <= 0.9
    with np.errstate(over="ignore"):                                   # expf(276) is inf in float32: the sigmoid is an exact 0 there
        r32k = rc.restate(x, np.float32, sliced=True)
    rc.check_parity(r32k, r64, r32, f"numpy f32 saturated {name}", factor=re.HALF_FACTOR)


# ---- the planted defects ------------------------------------------------------------------------------------------------------------------
# the rows the issue of this table names for each defect; APPLIES says where else it changes something
NAMED = dict(chunk_restart=set(re.IDX_ROWS), ih_first_k_tile={"wide_x"}, shallow_loop={"mix_c_deep"}, tail_tile_state={"t16_15", "t8_7"})


@pytest.mark.parametrize("defect", re.DEFECTS)
def test_parity_rule_catches_the_planted_defects(defect):
    """Each defect is a change of the restatement alone.  On every row it applies to, some tensor leaves the unchanged rule's bound by more
    than LARGE times; on every other row the restatement with the defect is the restatement without it, bit for bit, and that lies within
    the rule."""
    applies = {n for n in re.NAMES if re.APPLIES[defect](re.inputs(n))}
    assert NAMED[defect] <= applies and (defect == "tail_tile_state" or NAMED[defect] == applies), (defect, sorted(applies))
    for name in re.NAMES:
        x, (r64, r32) = re.inputs(name), re.references(name)
        good, bad = rc.restate(x, np.float64), re.restate_with(x, defect)
        if name not in applies:
            assert all(np.array_equal(good[k], bad[k]) for k in good), (defect, name)
            rc.check_parity(bad, r64, r32, f"{defect} on {name}, where it does not apply")
            continue
        over = re.ratios(bad, r64, r32)
        worst = max(over, key=over.get)
        print(f"{defect} on {name}: {worst} is {over[worst]:.3g} times its bound")
        assert over[worst] > re.LARGE, (defect, name, over[worst])
        with pytest.raises(AssertionError):
            rc.check_parity(bad, r64, r32, f"{defect} on {name}")


def test_tail_tile_state_is_nothing_on_a_last_tile_of_one():
    """t16_17, t16_33, t8_17 and mix_tile end on a tile of one trajectory, which is trajectory n_traj - 1 itself, and t16_16 and t8_8 on a
    full one: the defect cannot show there, whatever the kernel does.  Their partner rows one short of the tile carry it."""
    tails = {n: re._tail(re.inputs(n))[1] for n in re.NAMES}
    assert {n for n, k in tails.items() if k == 1} >= {"t16_17", "t16_33", "t8_17", "mix_tile"} and (tails["t16_15"], tails["t8_7"]) == (15, 7)
    assert tails["t16_16"] == 16 and tails["t8_8"] == 8

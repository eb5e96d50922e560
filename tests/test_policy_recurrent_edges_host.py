"""Host side of the recurrent policy step's edge tests (tests/policy_recurrent_edges.py holds the table): the row tile each row plans,
through `lg_policy_row_tile_recurrent` and through a Python restatement of the plan; the coverage the table as a whole must keep -- every
two-operand gate body, the K tails of the second operand, H = 1, uneven memories, the batch sizes at each tile; the descriptor of a module
whose memories differ; and the discrimination checks that make the parity comparisons of tests/test_gpu_policy_recurrent_edges.py able
to fail.  No GPU needed: nothing is launched.  (`RolloutStorage` has no CPU form, so the saved-state rows of an uneven module are
checked in the device file.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from hcr_genesis_lr_cl_amd import abi
from tests import policy_edges as pe
from tests import policy_recurrent_edges as pre
from tests.test_policy_host import PARITY_FACTOR, max_err, parity_bound
from tests.test_policy_recurrent_host import (LAST_KEYS, RESET_BEFORE, RNETS, STATE_VARIANTS, VARIANTS, _args, make_rnet, mem_dims, np_steps,
                                              state_keys)


# ---- the planned tile -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pre.ROWS))
def test_planned_tile_is_the_claimed_one(name):
    d = pre.ROWS[name]
    _, a, t, mem = _args(make_rnet(d), d, prev=True, mask=True)
    lib = abi.load_lib()                      # the launch plan alone: nothing is enqueued
    assert lib.lg_policy_row_tile_recurrent(C.byref(a)) == d["R"], lib.lg_last_error()
    assert pre.planned_tile(d) == d["R"]      # the kernel file's words, restated


def test_plan_restatement_on_the_documented_figures():
    """The LDS table of DESIGN.md 10b, and both sides of every threshold the table's comment derives."""
    strides = lambda d: pe.buffer_strides(pre.sequences(d))
    assert strides(RNETS["tiny_lstm2"]) == [68, 68] and pre.planned_tile(RNETS["tiny_gru2"]) == 32
    assert strides(RNETS["go2_lstm"]) == [324, 1028] and pre.planned_tile(RNETS["go2_lstm"]) == 16
    assert strides(RNETS["gru512"]) == [580, 2052] and pre.planned_tile(RNETS["gru512"]) == 8
    assert strides(pre.ROWS["lstm2_512"]) == [2052, 2052] and 8 * (2052 + 2052) * 4 == 131328 <= pe.LDS_BYTES < 16 * (2052 + 2052) * 4
    assert [sum(strides(pre.ROWS[n])) for n in ("lstm_225", "lstm_226", "lstm_481", "lstm_482", "gru2_145", "gru2_146")] == [1224, 1288, 2504, 2568, 1160, 1288]
    assert 32 * 1280 * 4 == 16 * 2560 * 4 == pe.LDS_BYTES
    assert strides(pre.ROWS["wideobs_lstm"]) == [2116, 132] and strides(pre.ROWS["crit8"]) == [580, 2052]
    assert [pre.gate_width(h) for h in (1, 2, 3, 7, 512)] == [5, 8, 12, 28, 2048] and [pre.pad4(w) for w in (1, 4, 5, 2047)] == [4, 4, 8, 2048]
    assert pre.sequences(RNETS["tiny_gru2"]) == [[8 + 7, 28, 28, 33, 7, 3], [8 + 7, 28, 28, 33, 7, 1]]
    assert pre.sequences(pre.ROWS["sweep_lstm_1_31"]) == [[4 + 1, 5, 5, 33, 1], [8 + 31, 124, 9, 1]]


# ---- coverage: what keeps a later edit of the table from silently dropping an edge --------------------------------------------------------
BODIES = [(rb, nt) for rb in (2, 1) for nt in (1, 2, 4)]


def test_table_covers_every_edge():
    """Every (RB, NT, two operands) body is reachable for BOTH kinds: RB = 2 is the 32-row tile, where any H up to 225 (LSTM) plans it;
    RB = 1 with a small NT needs a small H at a 16- or 8-row tile, which a wide observation or the other memory forces.  No pair is
    unreachable.  Take a row out of the table and one of these tags goes with it."""
    tags = set()
    for d in pre.ROWS.values():
        tags |= pre.row_tags(d)
    need = {f"<{rb},{nt},two>:{kind}" for rb, nt in BODIES for kind in ("lstm", "gru")}
    need |= {"H=1", "H=1,two-layers", "K2<16", "K2%16=0", "K2%16=1", "K2%16=15", "K2%16=other", "x_col[0]!=in", "x_col[1]!=H", "uneven-H",
             "uneven-depth", "uneven-in"}
    need |= {f"R={R},N={what}" for R in (32, 16, 8) for what in ("1", "R", "R+1", "2R+1")}
    need |= {f"H={h}:{kind}" for kind, hs in pre.SWEEP_H.items() for h in hs}
    assert need <= tags, sorted(need - tags)
    assert set(pre.SWEEP_H["lstm"]) == {1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65} and set(pre.SWEEP_H["gru"]) == set(pre.SWEEP_H["lstm"]) | {96, 97}
    assert {(rb, nt) for d in pre.ROWS.values() for rb, nt, two in pre.bodies(d) if two} == set(BODIES)
    sweep = {n: d for n, d in pre.ROWS.items() if n.startswith("sweep_")}
    assert len(sweep) == 14 + 16 and all(d["R"] == 32 and d["sizes"] == (33,) for d in sweep.values())
    for d in sweep.values():                                                         # paired, uneven in all three, every obs width and A taken
        assert d["H"] != d["H_c"] and d["layers"] + d["layers_c"] == 3 and d["obs"] != d["cobs"]
    assert {d["obs"] for d in sweep.values()} == {d["cobs"] for d in sweep.values()} == set(pre.SWEEP_OBS) and {d["A"] for d in sweep.values()} == {1, 3, 4, 5, 12}
    for kind, hs in pre.SWEEP_H.items():                                             # every H as memory_a's and as memory_c's
        assert sorted(d["H"] for d in sweep.values() if d["kind"] == kind) == sorted(d["H_c"] for d in sweep.values() if d["kind"] == kind) == sorted(hs)
    # the NT thresholds, both sides, where the gate layer's neuron count puts them
    assert [pe.neuron_tiles(4 * h)[1] for h in (16, 17, 48, 49)] == [1, 2, 2, 4] and [pe.neuron_tiles(2 * h)[1] for h in (32, 33, 96, 97)] == [1, 2, 2, 4]
    assert [pe.neuron_tiles(h)[1] for h in (64, 65)] == [1, 2]
    for name, d in pre.ROWS.items():
        if not name.startswith("sweep_"):
            assert d["sizes"] == (1, d["R"], d["R"] + 1, 2 * d["R"] + 1), name
    assert pre.bodies(pre.ROWS["wideobs_lstm"]) >= {(1, 2, True), (1, 1, True)} and pre.bodies(pre.ROWS["wideobs_gru"]) >= {(1, 2, True), (1, 1, True)}
    assert (1, 1, True) in pre.bodies(pre.ROWS["crit8"]) and (1, 4, True) in pre.bodies(pre.ROWS["crit8"])      # H 7 beside H 512, at 8 rows
    assert max(n * max(mem_dims(d, "a")[2], mem_dims(d, "c")[2]) for d in pre.ROWS.values() for n in d["sizes"]) <= 33 * 482      # the GPU file stays quick
    assert len(pre.CASES) == 30 + 4 * 10


# ---- uneven descriptors -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sweep_lstm_1_31", "sweep_gru_97_31", "wideobs_lstm", "crit8"])
def test_descriptor_of_uneven_modules(name):
    d = pre.ROWS[name]
    m = make_rnet(d)
    n = 7
    spec, a, t, mem = _args(m, d, n, prev=True, mask=True)
    kind = abi.POLICY_LSTM if d["kind"] == "lstm" else abi.POLICY_GRU
    for ma, ms, mod, w, src in ((a.memory_a, spec.memory_a, m.memory_a, "a", t["obs"]), (a.memory_c, spec.memory_c, m.memory_c, "c", t["cobs"])):
        inp, layers, H = mem_dims(d, w)
        assert (ms.layers, ms.hidden, ms.input_size) == (layers, H, inp)
        assert (ma.kind, ma.n_layers, ma.hidden, ma.in_width, ma.in_stride, ma.input) == (kind, layers, H, inp, inp, src.data_ptr())
        for k in range(abi.POLICY_MAX_RNN_LAYERS):
            for f in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                assert getattr(ma.layer[k], f) == (getattr(mod.rnn, f"{f}_l{k}").data_ptr() if k < layers else None), (w, k, f)
        for k in state_keys(d["kind"]):
            if k.endswith(w):
                assert tuple(mem[k].shape) == (layers, n, H) and getattr(ma, k[0]) == mem[k].data_ptr()
                assert getattr(ma, k[0] + "_prev_out") == mem[k.replace("_", "_prev_")].data_ptr()
        assert ma.reset_mask == mem["reset"].data_ptr()
    assert (a.actor.layer[0].n_in, a.critic.layer[0].n_in) == (d["H"], d["H_c"]) and d["H"] != d["H_c"]
    # a state of the OTHER memory's shape is refused by name, before a descriptor exists
    from hcr_genesis_lr_cl_amd import policy
    z = lambda w: torch.zeros(n, w)
    with pytest.raises(ValueError, match="h_c must be a contiguous"):
        policy.policy_args(spec, t["obs"], t["cobs"], z(d["A"]), z(d["A"]), z(d["A"]), z(1), z(1), noise=z(d["A"]), memory=dict(mem, h_c=mem["h_a"]))


# ---- discrimination ---------------------------------------------------------------------------------------------------------------------------
HOST_N = 33
WRONG_ROWS = ("sweep_lstm_1_31", "sweep_lstm_17_65", "sweep_lstm_16_64", "sweep_gru_1_32", "sweep_gru_48_4", "sweep_gru_31_97", "wideobs_lstm",
              "lstm_225", "gru2_145")


def applies_to(variant, d):
    """The memories ("a", "c") in which the mistake `variant` exists for net set `d`."""
    kind = {**VARIANTS, **STATE_VARIANTS}[variant]
    if kind not in (None, d["kind"]):
        return ""
    if variant in ("stale_layer", "prev_of_layer0"):
        return "".join(w for w in "ac" if mem_dims(d, w)[1] == 2)
    if variant == "swapped_memories":
        return "c" if mem_dims(d, "a")[1:] == mem_dims(d, "c")[1:] else ""
    return "ac"


WRONG = [(n, v) for n in WRONG_ROWS for v in (*VARIANTS, *STATE_VARIANTS) if applies_to(v, pre.ROWS[n])]


def _errs(name, got, n):
    s = pre.edge_shared(name, n)
    ref, f32 = s["ref"][-1], s["f32"][-1]
    return {k: (max_err(got[k], ref[k]), parity_bound(max_err(f32[k], ref[k]), ref[k])) for k in LAST_KEYS if k in ref}


def test_every_variant_runs_on_every_nt_class_and_on_uneven_rows():
    """Per mistake and kind it exists in: the sweep rows it runs on put it into a memory of each NT class of the gate layer (a stale or
    mis-staged layer: into a TWO-layer memory of each class); every sweep row is uneven.  The swapped memories need two of one shape."""
    ran = {}
    for n, v in WRONG:
        d = pre.ROWS[n]
        for w in applies_to(v, d) if n.startswith("sweep_") else "":
            ran.setdefault((v, d["kind"]), set()).add(pe.neuron_tiles((4 if d["kind"] == "lstm" else 2) * mem_dims(d, w)[2])[1])
    for v, kind in {**VARIANTS, **STATE_VARIANTS}.items():
        for k in ("lstm", "gru") if kind is None else (kind,):
            if v == "swapped_memories":
                assert any(vv == v and pre.ROWS[n]["kind"] == k for n, vv in WRONG), k
            else:
                assert ran[v, k] == {1, 2, 4}, (v, k, ran.get((v, k)))
    assert any(v == "no_bhh" for n, v in WRONG if n == "wideobs_lstm")


@pytest.mark.parametrize("name,variant", WRONG)
def test_parity_rule_fails_the_wrong_cells(name, variant):
    """Each wrong cell or state handling exceeds the bound in a state or the output of every memory it exists in (five steps, two resets)."""
    d, s = pre.ROWS[name], pre.edge_shared(name, HOST_N)
    errs = _errs(name, np_steps(s["module"], s["inp"], variant), HOST_N)
    for w in applies_to(variant, d):
        keys = [k for k in ("mu" if w == "a" else "values", "h_" + w, "c_" + w) if k in errs]
        for k in keys:
            print(f"wrong {variant} {name} {k}: err {errs[k][0]:.3e} bound {errs[k][1]:.3e} ratio {errs[k][0] / errs[k][1]:.1f}")
        assert any(errs[k][0] > errs[k][1] for k in keys), (w, {k: errs[k] for k in keys})
    assert PARITY_FACTOR == 8.0


@pytest.mark.parametrize("name", list(pre.ROWS))
def test_numpy_cells_stay_within_the_rule(name):
    """The honest float32 restatement, at every row and its largest N: another evaluation order of the same cells is inside the bound
    the wrong ones exceed."""
    n = max(pre.ROWS[name]["sizes"])
    s = pre.edge_shared(name, n)
    for k, (e, b) in _errs(name, np_steps(s["module"], s["inp"]), n).items():
        print(f"numpy cells {name} {k}: err {e:.3e} bound {b:.3e}")
        assert e <= b, (k, e, b)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def test_inputs_have_no_equal_rows_or_columns():
    """Per row of the table and step: no two env rows and no two columns of the observations, the noise or a start state are equal, and
    neither are two rows of the outputs the comparisons rest on: a shifted tile or a repeated row cannot pass.  Both masks are mixed."""
    for name, d in pre.ROWS.items():
        n = max(d["sizes"])
        s = pre.edge_shared(name, n)
        inp = s["inp"]
        mats = [x for k in ("obs", "cobs", "noise") for x in inp[k].numpy()] + [x for v in inp["start"].values() for x in v.numpy()]
        for a in mats:
            assert np.unique(a, axis=0).shape == a.shape and np.unique(a, axis=1).shape == a.shape, name
        for k in ("mu", "values", "h_a", "h_c"):
            ref = s["ref"][-1][k].reshape(-1, s["ref"][-1][k].shape[-1])
            assert np.unique(ref, axis=0).shape == ref.shape, (name, k)
        assert all(inp["masks"][t].any() and not inp["masks"][t].all() for t in RESET_BEFORE), name

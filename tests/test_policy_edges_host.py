"""Host side of the fused policy step's edge tests (tests/policy_edges.py holds the table): the row tile each row plans, through
`lg_policy_row_tile` and through a Python restatement of the plan; the coverage the table as a whole must keep; the NaN semantics of the
torch reference, which is where tests/test_gpu_policy_edges.py takes its expectation from; and the discrimination checks that make the
parity comparisons on the 8-row tile and the ragged sweeps able to fail.  No GPU needed: nothing is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

from hcr_genesis_lr_cl_amd import abi, policy
from tests import policy_edges as pe
from tests.test_policy_families_host import DWAQ_NETS, make_dwaq
from tests.test_policy_host import PARITY_FACTOR, make_net, max_err, np_forward, parity_bound


def _descriptor(name, n=7):
    """The LgPolicyArgs `FusedPolicy.act` would build for table row `name` (host tensors: nothing is launched)."""
    d = pe.EDGE_NETS[name]
    spec = policy.describe(pe.make_edge(name))
    z = lambda w: torch.zeros(n, w)
    kw = dict(actions=z(d["A"]), mu=z(d["A"]), sigma=z(d["A"]), log_prob=z(1), values=z(1), counter=torch.zeros(1, dtype=torch.int32))
    if d["kind"] == "dwaq":
        kw["obs_history"] = z(d["hist"])
    keep = [z(d["obs"]), z(d["cobs"]), kw]
    return policy.policy_args(spec, keep[0], keep[1], **kw), keep


# ---- the planned tile -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pe.EDGE_NETS))
def test_planned_tile_is_the_claimed_one(name):
    d = pe.EDGE_NETS[name]
    a, keep = _descriptor(name)
    lib = abi.load_lib()                      # the launch plan alone: nothing is enqueued
    assert lib.lg_policy_row_tile(C.byref(a)) == d["R"], lib.lg_last_error()
    assert pe.planned_tile(d) == d["R"]       # the header's words, restated
    assert set(d["reach"]) <= pe.row_tags(d), set(d["reach"]) - pe.row_tags(d)


def test_plan_restatement_on_the_documented_figures():
    assert [pe.lds_stride(w) for w in (1, 4, 5, 68, 69, 2047, 2048, 520, 1989, 453, 452)] == [4, 4, 68, 68, 132, 2052, 2052, 580, 2052, 516, 452]
    assert 16 * (2052 + 580) * 4 == 168448 > pe.LDS_BYTES >= 8 * (2052 + 580) * 4          # wide8, as the table's comment derives it
    assert 16 * (2052 + 516) * 4 > pe.LDS_BYTES >= 16 * (2052 + 452) * 4                   # wide8_ee against wide16_ee: one neuron apart
    assert pe.planned_tile(dict(kind="plain", obs=2048, actor=[2048], A=1, cobs=1, critic=[1])) == 8      # a 2048-2048 pair fits at 8
    assert [pe.neuron_tiles(m) for m in (1, 64, 65, 192, 193, 256, 520)] == [(1, 1), (4, 1), (5, 2), (12, 2), (13, 4), (16, 4), (33, 4)]


# ---- coverage: what keeps a later edit of the table from silently dropping an edge --------------------------------------------------------
def test_table_covers_every_edge():
    tags = set()
    for d in pe.EDGE_NETS.values():
        tags |= pe.row_tags(d)
    need = {"R=8", "R=16", "R=32", "nt1-exact", "nt1-ragged", "nt2-exact", "nt2-ragged", "nt4-exact", "nt4-ragged", "K<4", "K<16", "K=16", "K%16=1",
            "K%16=15", "K%4!=0", "M=1", "A%4=0", "A%4=1", "A%4=3", "cat-col%4!=0", "(L+E)%4!=0"}
    assert need <= tags, need - tags
    for k in pe.SWEEP_K:
        assert f"K={k}" in tags
    for m in pe.SWEEP_M:
        assert f"M={m}" in tags
    assert set(pe.SWEEP_K) == {1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65}
    assert set(pe.SWEEP_M) == {1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 80, 192, 193, 208}
    sweep = [d for n, d in pe.EDGE_NETS.items() if n.startswith("sweep_")]
    assert len(sweep) == len(pe.SWEEP_K) == len(pe.SWEEP_M) and {d["A"] for d in sweep} == {1, 3, 4, 5, 12}      # paired, not crossed
    for name in ("wide8", "wide8_ee", "wide8_dwaq"):
        assert pe.EDGE_NETS[name]["R"] == 8 and pe.EDGE_NETS[name]["sizes"] == (1, 8, 9, 33)
    assert all(d["sizes"] == (33,) for d in sweep)
    assert len(pe.CASES) <= 32                                                                                        # the GPU file stays quick


def test_inputs_have_no_equal_rows_or_columns():
    for name in ("wide8", "wide8_dwaq", "sweep_1_1"):
        c = pe.edge_case(name)
        for k in ("mu", "values"):
            ref = c["ref"][k]
            assert np.unique(ref, axis=0).shape == ref.shape, (name, k)          # ... and neither have the outputs the comparisons rest on


# ---- the reference's NaN semantics: the expectation of the GPU test, taken from torch and not from the kernel -----------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("clip", [0.05, None])
@pytest.mark.parametrize("name", ["tiny", "go2"])
def test_reference_passes_a_nan_to_its_own_row(name, clip, dtype):
    m = make_net(name, clip).to(dtype)
    g = torch.Generator().manual_seed(11)
    n, bad = 33, [5, 32]
    A = m.std.shape[0]
    obs, z = torch.randn(n, m.actor[0].in_features, generator=g).to(dtype), torch.randn(n, A, generator=g).to(dtype)
    poisoned = obs.clone()
    poisoned[bad, 0] = float("nan")
    with torch.no_grad():
        clean, got = pe.torch_act(m, m.mean(obs), z), pe.torch_act(m, m.mean(poisoned), z)
    ok = [i for i in range(n) if i not in bad]
    for k, v in got.items():
        assert torch.isnan(v[bad]).all(), k                                       # every element of the poisoned rows, clip or no clip
        assert torch.equal(v[ok], clean[k][ok]) and torch.isfinite(v[ok]).all(), k
    if clip is not None:
        assert clean["mu"].abs().max() == clip                                    # the Hardtanh was live


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_reference_dreamwaq_passes_a_nan_in_the_history(dtype):
    d = DWAQ_NETS["tiny_dwaq"]
    m = make_dwaq("tiny_dwaq", 0.05).to(dtype)
    g = torch.Generator().manual_seed(11)
    n, bad, L, E = 33, [5, 32], d["L"], d["E"]
    obs, hist, eps = (torch.randn(n, w, generator=g).to(dtype) for w in (d["obs"], d["hist"], L + E))
    poisoned = hist.clone()
    poisoned[bad, 3] = float("nan")
    with torch.no_grad():
        clean, got = m.forward_all(obs, hist, eps), m.forward_all(obs, poisoned, eps)
    ok = [i for i in range(n) if i not in bad]
    logvar = torch.cat((got["params"][:, L:2 * L], got["params"][:, 2 * L + E:]), dim=1)
    assert torch.isnan(logvar[bad]).all()                                         # through Hardtanh(-5, 5)
    for k in ("params", "latent", "mu"):
        assert torch.isnan(got[k][bad]).all(), k
        assert torch.equal(got[k][ok], clean[k][ok]), k


# ---- discrimination -------------------------------------------------------------------------------------------------------------------------
def test_parity_rule_fails_duplicated_rows_and_a_dropped_tile():
    """On wide8 at N = 33: the honest float32 restatement is within the bound; rows 8 .. 15 of a 16-row block holding row 7 (what the 8-row
    tile's clamped fragment rows would give if they were stored) and a ragged sweep that loses its last neuron tile are both far outside."""
    c = pe.edge_case("wide8")
    m, n = c["module"], 33
    for chain, x, key in ((m.actor, c["obs"], "mu"), (m.critic, c["cobs"], "values")):
        ref = c["ref"][key]
        bound = parity_bound(max_err(c["f32"][key], ref), ref)
        good, dup, drop = np_forward(chain, x.numpy()), pe.np_dup_rows(chain, x.numpy()), pe.np_drop_ragged_tile(chain, x.numpy())
        print(f"wide8 {key}: bound {bound:.3e}, honest {max_err(good, ref):.3e}, duplicated rows {max_err(dup, ref):.3e}, dropped tile {max_err(drop, ref):.3e}")
        assert max_err(good, ref) <= bound
        assert max_err(dup, ref) > 100 * bound and max_err(drop, ref) > 100 * bound
        per_row = np.abs(dup - ref).max(axis=1)                                   # every duplicated row is caught on its own, not only the worst
        assert all(per_row[r] > 100 * bound for b in (0, 16) for r in range(b + 8, b + 16))
    assert PARITY_FACTOR == 8.0

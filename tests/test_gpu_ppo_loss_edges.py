"""The fused PPO loss head on the GPU at its edges (tests/ppo_loss_edges.py; tests/test_ppo_loss_edges_host.py proves the tables are what
they claim): every row width up to 64 and a two-group call of more than one sweep, rows built ON the gradient selectors' ties and
boundaries, rows where float32 over- or underflows, one NaN at a time in each of the ten inputs, clip_param other than 0.2, and a
partials slab that is dirty.  Every comparison is the parity rule of tests/ppo_loss_cases.py (factor 8), bit equality, or equality of
the non-finite pattern with torch's own float32 autograd on the CPU."""
import numpy as np
import pytest
import torch

from hcr_genesis_lr_cl_amd import abi, ppo_loss
from tests import ppo_loss_cases as pc
from tests import ppo_loss_edges as pe
from tests.test_gpu_ppo_loss import DEV, case_data, cfg_of, run, same_bits, strided_equals_contiguous, to_device

pytestmark = pytest.mark.gpu

_CACHE = {}


def edge_data(name):
    """Inputs and both restatements of a width or clip case, computed once and shared."""
    if name not in _CACHE:
        c = pe.WIDTH_CASES.get(name) or pe.CLIP_CASES[name]
        inp = pc.make_inputs(c)
        _CACHE[name] = (c, inp, pc.restate(inp, **pe.cfg(c)), pc.restate(inp, dtype=torch.float32, **pe.cfg(c)))
    return _CACHE[name]


# ---- A. widths and sweeps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pe.WIDTH_CASES))
def test_parity_at_every_width(name):
    c, inp, ref64, ref32 = edge_data(name)
    got, raw = run(to_device(inp), **pe.cfg(c))
    assert all(raw["result"][abi.PPO_R_KL + g].item() == 0.0 for g, kl in enumerate(c["kl"]) if not kl)
    pc.check_parity(got, ref64, ref32, name)


def test_two_group_sweep_is_bit_identical():
    c, inp, _, _ = edge_data(pe.SWEEP)
    dev = to_device(inp)
    a, _ = run(dev, **pe.cfg(c))
    b, _ = run(dev, **pe.cfg(c))
    assert same_bits(a, b) and np.isfinite(a["loss"])


@pytest.mark.parametrize("name", pe.STRIDED)
def test_strided_views_at_eight_and_sixteen_lanes(name):
    c, inp, _, _ = edge_data(name)
    strided_equals_contiguous(inp, c, pe.cfg(c))


def test_a_row_s_gradients_do_not_depend_on_its_place():
    """w33's rows (A = 33, 16 lanes per row, 16 rows per tile; no entropy term, whose scale carries the number of policy rows) moved
    about: the gradients move with the rows, bit for bit."""
    c, inp, _, _ = edge_data("w33")
    kw = dict(pe.cfg(c), ent=0.0)
    B = c["rows"][0]
    assert B == 17 and pe.plan(c)["per_tile"] == 16
    base, _ = run(to_device(inp), **kw)
    swap = lambda i, j: np.array([j if r == i else (i if r == j else r) for r in range(B)])
    for perm in (swap(0, 5), swap(B - 1, 5), np.arange(B)[::-1].copy()):         # row 5 first; last, alone in the ragged tile; all reversed
        got, _ = run(to_device(pe.take_rows(inp, perm)), **kw)
        for key in ("grad_mu", "grad_sigma"):
            assert np.array_equal(got[key][0], base[key][0][perm]), key
        assert np.array_equal(got["grad_values"], base["grad_values"][perm])
    # as the only row of group 1 behind sixteen rows of group 0: 1 / B is 1 against 1 / 16, an exact power of two
    head = pe.take_rows(inp, np.arange(16))
    base16, _ = run(to_device(head), **kw)
    two = dict(head, groups=[head["groups"][0], pe.take_rows(inp, np.array([5]))["groups"][0]])
    got, _ = run(to_device(two), **kw)
    for key in ("grad_mu", "grad_sigma"):
        assert np.array_equal(got[key][0], base16[key][0]), key
        assert np.array_equal(got[key][1][0], 16.0 * base16[key][0][5]) and np.isfinite(got[key][1]).all(), key
    assert np.array_equal(got["grad_values"], base16["grad_values"])


# ---- B. ties, boundaries, overflow ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", pe.TIE_WIDTHS)
@pytest.mark.parametrize("spo", [False, True])
def test_rows_on_the_ties_and_boundaries(A, spo):
    """The rows that stay finite, in one call at clip_param = 0.25: the parity rule against float64, torch-CPU-float32 as its scale."""
    inp = pe.tie_inputs(A)
    kw = dict(clipped=True, spo=spo, ent=0.0, clip=pe.TIE_CLIP)
    ref64, ref32 = pc.restate(inp, **kw), pc.restate(inp, dtype=torch.float32, **kw)
    got, _ = run(to_device(inp), **kw)
    pc.check_parity(got, ref64, ref32, f"ties A={A} spo={spo}")
    zero = [i for i, row in enumerate(pe.POLICY_ROWS) if row[1] == 0.0]           # Adv = +-0: zero of either sign
    assert (got["grad_mu"][0][zero] == 0).all() and (got["grad_sigma"][0][zero] == 0).all()
    if spo:
        # ratio == 1.0f exactly in the kernel too: SPO's (ratio - 1) term then vanishes and d loss / d logp is -Adv / B to the bit, where
        # one ulp of ratio would move it by 2.4e-7 of itself.  One float32 product behind it: d / sigma^2 at A = 13, -1 / sigma at A = 1.
        f = np.float32
        adv_b = inp["groups"][0]["advantages"][:2, 0] * (f(1) / f(len(pe.POLICY_ROWS)))
        d = inp["groups"][0]["actions"][:2] - inp["groups"][0]["mu"][:2]
        want = (-adv_b[:, None] * d) if A > 1 else adv_b[:, None] * np.ones((2, 1), f)
        assert np.array_equal(got["grad_mu" if A > 1 else "grad_sigma"][0][:2], want.astype(np.float64))
    # the value table's third column is exact in float32 (coef 1): d term / d v = B * grad_values
    for (name, _, _, _, _, want), x in zip(pe.VALUE_ROWS, got["grad_values"].reshape(-1) * len(pe.VALUE_ROWS)):
        if want is not None:
            assert x == want, (name, x, want)


@pytest.mark.parametrize("A", pe.TIE_WIDTHS)
@pytest.mark.parametrize("spo", [False, True])
def test_rows_that_overflow_float32(A, spo):
    """expf to inf and to 0, Adv = +-inf and 3e38, v_t and R = +inf: float64 does not overflow where float32 does, so the reference is
    torch's own float32 autograd.  Row by row the gradients have its NaN / +inf / -inf / finite pattern, element by element; the finite
    elements keep the parity rule against its value with the rule's floor (one float32 ulp of the row's largest magnitude) as the
    scale; the scalars have its pattern."""
    inp = pe.tie_inputs(A, overflow=True)
    kw = dict(clipped=True, spo=spo, ent=0.0, clip=pe.TIE_CLIP)
    ref = pc.restate(inp, dtype=torch.float32, **kw)
    got, _ = run(to_device(inp), **kw)
    bad = []
    for (name, x), (_, r) in zip(pc.outputs(got), pc.outputs(ref)):
        x, r = np.atleast_2d(x), np.atleast_2d(r)
        rows = pe.VALUE_OVERFLOW_ROWS if name == "grad_values" else pe.POLICY_OVERFLOW_ROWS
        for i in range(x.shape[0]):
            label = f"A={A} spo={spo} {name}" + (f" [{rows[i][0]}]" if "grad" in name else "")
            print(f"{label}: kernel {x[i][:4]}, torch f32 {r[i][:4]}")
            if not np.array_equal(pe.pattern(x[i]), pe.pattern(r[i])):
                bad.append(label)
                continue
            fin = np.isfinite(r[i])
            if fin.any() and pc.max_err(x[i][fin], r[i][fin]) > pc.parity_bound(0.0, r[i][fin]):
                bad.append(label + " (finite elements)")
    assert not bad, bad
    vg = got["grad_values"].reshape(-1) * len(pe.VALUE_OVERFLOW_ROWS)
    assert [float(v) for v in vg] == [row[5] for row in pe.VALUE_OVERFLOW_ROWS]


# ---- C. one NaN at a time ---------------------------------------------------------------------------------------------------------------------------
_CLEAN = {}


def _clean(base, tensor, clipped):
    c, group = pe.nan_case(base, tensor)
    key = (base, tuple(c["kl"]), clipped)
    if key not in _CLEAN:
        inp = pc.make_inputs(c)
        _CLEAN[key] = (inp, run(to_device(inp), **dict(pe.cfg(c), clipped=clipped))[0])
    return (c, group) + _CLEAN[key]


def _check_reach(got, clean, scalars, grads, row, label):
    for (name, x), (_, y) in zip(pc.outputs(got), pc.outputs(clean)):
        if np.ndim(x) == 0:
            assert np.isfinite(y), (label, name)
            assert np.isnan(x) if name in scalars else x == y, (label, name, x, y)
        elif name in grads:
            keep = np.arange(x.shape[0]) != row
            assert np.isnan(x[row]).all() and np.array_equal(x[keep], y[keep]), (label, name)
        else:
            assert np.array_equal(x, y), (label, name)


@pytest.mark.parametrize("tensor", pe.GROUP_TENSORS + pe.VALUE_TENSORS)
@pytest.mark.parametrize("base", list(pe.NAN_BASES))
def test_one_nan_reaches_what_its_row_feeds_and_nothing_else(base, tensor):
    """include/lgppo.h: "a NaN in a row reaches that row's gradients and every scalar the row feeds, and nothing else" -- `nan_reach` per
    tensor; everything else keeps the bits of the clean run.  A NaN target value under the clipped value loss gives a NaN gradient,
    where torch autograd returns a finite one (tests/test_ppo_loss_edges_host.py pins that side)."""
    c, group, inp, clean = _clean(base, tensor, pe.NAN_BASES[base][0]["clipped"])
    assert c["clipped"]
    scalars, grads = pe.nan_reach(tensor, group, c["kl"][group], True)
    for row, col in pe.nan_places(c, group, tensor):
        got, _ = run(to_device(pe.with_nan(inp, group, tensor, row, col)), **pe.cfg(c))
        _check_reach(got, clean, scalars, grads, row, f"{base} {tensor}[{row}, {col}]")


@pytest.mark.parametrize("base", list(pe.NAN_BASES))
def test_unclipped_value_loss_does_not_read_the_target_values(base):
    c, group, inp, clean = _clean(base, "target_values", False)
    bad = dict(inp, target_values=np.full_like(inp["target_values"], np.nan))
    got, _ = run(to_device(bad), **dict(pe.cfg(c), clipped=False))
    assert pe.nan_reach("target_values", group, c["kl"][group], False) == ([], [])
    assert same_bits(got, clean) and np.isfinite(got["loss"])


# ---- D. other clip values, a dirty slab -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pe.CLIP_CASES))
def test_parity_at_other_clip_values(name):
    c, inp, ref64, ref32 = edge_data(name)
    got, _ = run(to_device(inp), **pe.cfg(c))
    pc.check_parity(got, ref64, ref32, name)


def _dirty(doubles):
    return dict(partials=torch.full((doubles,), float("nan"), dtype=torch.float64, device=DEV),
                result=torch.full((abi.PPO_RESULT_FLOATS,), float("nan"), device=DEV))


@pytest.mark.parametrize("name", ["b257_a12", "cts_17_5"])
def test_a_dirty_oversized_slab_changes_nothing(name):
    inp, _, _ = case_data(name)
    c = pc.CASES[name]
    need = ppo_loss.workspace_doubles(c["rows"], c["vrows"], c["A"])
    fresh, _ = run(to_device(inp), **cfg_of(name))
    out = _dirty(need + 64)
    got, _ = run(to_device(inp), out=out, **cfg_of(name))
    assert same_bits(got, fresh) and np.isfinite(got["loss"])
    slab = out["partials"].cpu().numpy()
    assert np.isnan(slab[need:]).all() and len(slab[need:]) == 64                                    # nothing behind the plan's rows is written
    assert np.isfinite(slab[:need]).all()


def test_a_small_call_on_the_slab_of_a_large_one():
    """b40001_a13 (512 workgroups) and then b1_a12 (2 workgroups) on the same slab: the small call reads its own rows only."""
    big, small = pc.LARGEST, "b1_a12"
    cb = pc.CASES[big]
    out = _dirty(ppo_loss.workspace_doubles(cb["rows"], cb["vrows"], cb["A"]))
    assert out["partials"].numel() == abi.PPO_MAX_BLOCKS * abi.PPO_PARTIAL_SLOTS
    first, _ = run(to_device(case_data(big)[0]), out=dict(out), **cfg_of(big))
    assert np.isfinite(first["loss"]) and torch.isfinite(out["partials"]).all()
    inp = case_data(small)[0]
    got, _ = run(to_device(inp), out=dict(out), **cfg_of(small))
    fresh, _ = run(to_device(inp), **cfg_of(small))
    assert same_bits(got, fresh) and np.isfinite(got["loss"])

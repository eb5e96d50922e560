"""The recurrent learner pass on the GPU (hcr_genesis_lr_cl_amd/train.py's FusedTrainPassRecurrent, csrc/lg_train_rnn.hip) at the edges of
tests/train_rnn_edges.py, which the table of tests/test_gpu_train_rnn.py does not reach: more than 256 trajectories (the index kernel's
chunked prefix sum, up to per = 6 as the go2_lstm workload runs it), the 16- and 8-trajectory time tiles one short, full and one over,
memories of different depth and width, observation rows wider than one K tile of the gathered weight gradient and of width 1, H = 1, 32
slices with a last one off a multiple of 4 rows, T = 24.  Every row runs as that file runs its cases (its `run`) against torch on the CPU
in float64 under the same factor-8 parity rule; the index region exactly; strided observations and start states and uint8 masks; repeats;
NaN in the padding; saturated gates."""
import numpy as np
import pytest
import torch

from hcr_genesis_lr_cl_amd import train
from tests import train_gpu as tg
from tests import train_rnn_cases as rc
from tests import train_rnn_edges as re
from tests.test_gpu_train_rnn import run
from tests.train_gpu import DEV, dev, host, same_bits

pytestmark = pytest.mark.gpu

RATIOS = []


def sizes(x):
    return x["T"] * x["E"], x["max_len"], x["n_traj"], x["T"]


def check_plan(tp, x):
    """The plan the pass reports is the restated one: both tiles, the workspace, and the slices of every (weight, bias) pair of the memories."""
    pl, want = tp.plan(*sizes(x)), rc.plan_of_case(x)
    assert (pl.time_row_tile, pl.time_tiles, pl.train.row_tile, pl.workspace_floats, pl.index_off) == \
        (want["time_row_tile"], want["time_tiles"], want["train"]["row_tile"], want["workspace_floats"], want["index_off"])
    for mi, l, wi, S, per, _ in re.memory_slices(x, want):
        assert (pl.slices[mi][l][wi], pl.slice_rows[mi][l][wi]) == (S, per), (mi, l, wi)
    return pl


# ---- parity -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", re.NAMES)
def test_parity_on_the_edge_table(name):
    x = re.inputs(name)
    got, _, tp = run(x)
    assert tp.spec.parameter_names() == x["names"]
    pl = check_plan(tp, x)
    assert f"Rt={pl.time_row_tile}" in re.ROWS[name]["reach"] or not any(t.startswith("Rt=") for t in re.ROWS[name]["reach"])
    ref64, ref32 = re.references(name)
    rc.check_parity(got, ref64, ref32, name, RATIOS)


# ---- the index region -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", re.IDX_ROWS)
def test_index_region_is_exact(name):
    """len, first and map as the index kernel leaves them at plan.index_off after a forward call, as integers against rc.lengths_of and
    rc.positions: no tolerance.  A wrong first[j] permutes rows between trajectories without a refusal or a NaN."""
    x = re.inputs(name)
    _, _, tp = run(x)
    N, _, n_traj, _ = sizes(x)
    off = int(tp.plan(*sizes(x)).index_off)
    region = host(tp.workspace[off:off + 2 * n_traj + N].view(torch.int32)).astype(np.int64)
    lens, first, row_map = re.index_region(x)
    assert np.array_equal(region[:n_traj], lens) and np.array_equal(region[n_traj:2 * n_traj], first) and np.array_equal(region[2 * n_traj:], row_map)
    assert len(set(region[2 * n_traj:].tolist())) == N                         # every row from a padded position of its own


# ---- strides ----------------------------------------------------------------------------------------------------------------------------------
def strided_batch(x, first=3):
    """The case's values laid out in place in wider tensors whose every other element is NaN (True for the masks): observations as columns
    [2, 2 + w) of rows 5 columns wider, start states as [:, first:first + n_traj, :H] of a tensor wider in both dimensions, the masks as
    uint8 columns [first, first + n_traj)."""
    n = x["n_traj"]
    nan = float("nan")

    def columns(a):
        wide = torch.full(a.shape[:2] + (a.shape[2] + 5,), nan, device=DEV)
        wide[..., 2:2 + a.shape[2]] = dev(a)
        return wide[..., 2:2 + a.shape[2]]

    def state(a):
        wide = torch.full((a.shape[0], first + n + 2, a.shape[2] + 3), nan, device=DEV)
        wide[:, first:first + n, :a.shape[2]] = dev(a)
        return wide[:, first:first + n, :a.shape[2]]

    masks = torch.ones((x["T"], first + n + 2), dtype=torch.uint8, device=DEV)
    masks[:, first:first + n] = torch.from_numpy(x["masks"].astype(np.uint8)).to(DEV)
    hid = []
    for m in "ac":
        h = [state(x["h0_" + m])] + ([state(x["c0_" + m])] if x["kind"] == "lstm" else [])
        hid.append(h if len(h) > 1 else h[0])
    return columns(x["obs"]), columns(x["critic_obs"]), masks[:, first:first + n], tuple(hid)


@pytest.mark.parametrize("name", ["mix_a_deep", "wide_x", "t16_17"])
def test_strided_inputs_keep_every_bit(name):
    x = re.inputs(name)
    clean, _, _ = run(x)
    b = strided_batch(x)
    m = rc.Recurrent(x).to(DEV)
    tp = train.FusedTrainPassRecurrent(m)
    N, _, n, T = sizes(x)
    A = x["A"]
    a = train.rnn_args(tp.spec, *b, x["E"], torch.empty(N, A, device=DEV), torch.empty(N, A, device=DEV), torch.empty(N, 1, device=DEV), None, device=tp.device)
    for mem, (L, H, w) in zip(a.memory, re.memories(x)):                       # the strides handed over are not the dense ones
        assert (mem.x_row_stride, mem.x_time_stride) == (w + 5, n * (w + 5)) and mem.x_row_stride > w
        assert mem.h0_row_stride == H + 3 > H and (L == 1 or mem.h0_layer_stride == (n + 5) * (H + 3) != n * H)
        assert mem.mask_time_stride == n + 5 > n and (x["kind"] != "lstm" or mem.c0_row_stride == H + 3)
    assert b[2].dtype == torch.uint8 and not b[0].is_contiguous()
    outs = tp(*b, n_envs=x["E"])
    torch.autograd.backward(list(outs), [dev(x[k]) for k in tg.COTANGENTS])
    torch.cuda.synchronize()
    got = dict(zip(("mu", "sigma", "values"), (host(o) for o in outs)))
    got.update({k: host(p.grad) for k, p in zip(x["names"], m.parameters())})
    assert all(np.isfinite(v).all() for v in got.values())
    assert same_bits(got, clean)


# ---- conventions ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["idx_1497", "mix_c_deep"])
def test_repeats_are_bit_identical(name):
    x = re.inputs(name)
    a, m, tp = run(x)
    b, _, _ = run(x, m, tp)                                           # the same pass again: its workspace is reused
    c, _, _ = run(x)                                                  # a fresh module and pass
    assert same_bits(a, b) and same_bits(a, c)


@pytest.mark.parametrize("name", ["idx_529", "mix_a_deep"])
def test_padding_reaches_nothing(name):
    """NaN in every padded position: every output and gradient keeps the bits of the clean run."""
    clean, _, _ = run(re.inputs(name))
    x = rc.make_inputs(re.case_of(name), pad=np.nan)
    assert np.isnan(x["obs"]).any() and np.isnan(x["critic_obs"]).any()
    got, _, _ = run(x)
    assert same_bits(got, clean)


@pytest.mark.parametrize("name", list(re.SATURATED))
def test_saturated_gates_stay_finite_and_within_the_rule(name):
    """Observations scaled until at least half of layer 0's gate pre-activations lie beyond 20 (tests/test_train_rnn_edges_host.py holds
    that): expf overflows in the sigmoids, every output and gradient is finite, and the parity rule holds unchanged."""
    x = re.inputs(name, True)
    got, _, tp = run(x)
    check_plan(tp, x)
    assert all(np.isfinite(v).all() for v in got.values())
    ref64, ref32 = re.references(name, True)
    rc.check_parity(got, ref64, ref32, f"{name} saturated x{re.SATURATED[name]:g}", RATIOS)


def test_zz_print_the_parity_ratios():
    """Not a check of its own: the worst |kernel - f64| / max(|torch-f32 - f64|, ulp) per tensor class over every parity check above, for
    DESIGN.md's table."""
    tg.print_parity_ratios(RATIOS)

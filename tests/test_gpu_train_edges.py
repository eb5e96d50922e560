"""The fused learner passes on the GPU (csrc/lg_train.hip, csrc/lg_train_ee.hip, csrc/lg_train_ts.hip, csrc/lg_train_pass.h,
csrc/lg_train_tiles.h) at the edges of tests/train_edges.py, which the tables of tests/test_gpu_train.py, tests/test_gpu_train_ee.py and
tests/test_gpu_train_ts.py do not reach: the 16- and 8-row tiles, NT = 4 over ragged widths, 31 and 32 batch slices with a short last one,
layers of unequal slice counts, the finalize kernels' second trip, and the 16-byte row accesses under a stride; for the teacher-student
(TS) passes also both placements of the privilege encoder and a latent wider than a 16-column tile under the small tiles, four-layer
encoders, and the two passes on different row tiles.  Every case runs as those three files run theirs (their `run`) against the float64
restatement under the same factor-8 parity rule; bit-identical repeats, the independence of rows across the small tiles, and strided
views with widths that are multiples of 4."""
import numpy as np
import pytest
import torch

from hcr_genesis_lr_cl_amd import train
from tests import train_cases as tc
from tests import train_edges as te
from tests import train_ee_cases as ec
from tests import train_gpu as tg
from tests import train_ts_cases as sc
from tests.test_gpu_train import run as run_plain
from tests.test_gpu_train_ee import run as run_ee
from tests.test_gpu_train_ts import run as run_ts
from tests.train_gpu import DEV, dev, host, same_bits

pytestmark = pytest.mark.gpu

RATIOS = []
FILL = 7.25
RUN = {"plain": run_plain, "ee": run_ee, "ts": run_ts}


def run_case(row, B, x=None):
    """One run of a case on a fresh module, after the plan has been held to the row tile the table states."""
    d = te.ROWS[row]
    x = x if x is not None else te.inputs(row, B)
    if d["kind"] == "plain":
        m = tc.Module(x, DEV)
        tp = train.FusedTrainPass(m)
        assert tp.plan(B).row_tile == d["R"]
        return run_plain(x, m, tp)
    if d["kind"] == "ts":
        m = sc.Module(x, DEV)
        tp = train.FusedTrainPassTS(m)
        assert (tp.plan(B).row_tile, tp.encoder_plan(B).row_tile) == d["R"]
        assert f"efb={tp.plan(B).enc_first_buffer}" in te.claimed(row, B)
        return run_ts(x, m, tp)
    m = ec.Module(x, DEV)
    tp = train.FusedTrainPassEE(m)
    assert (tp.plan(B).row_tile, tp.estimator_plan(B).row_tile) == d["R"]
    return run_ee(x, m, tp)


# ---- parity -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", te.CASES, ids=[te.case_id(c) for c in te.CASES])
def test_parity_on_the_edge_table(case):
    row, B = case
    got, _, _ = run_case(row, B)
    ref64, ref32 = te.references(row, B)
    n = len(RATIOS)
    te.check(row, got, ref64, ref32, te.case_id(case), RATIOS)
    assert len(RATIOS) == n + 1 and RATIOS[-1][0] == te.case_id(case)


# ---- determinism ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("r8", 25), ("tiny", 2113), ("fixture", 8193), ("ts_r8_z", 25), ("ts_r16", 2049), ("ts_r8_even", 2049)], ids=te.case_id)
def test_repeats_are_bit_identical(case):
    """The 8-row tile, the 32-slice combine and the two-trip finalize: the same pass again on its own workspace, and a fresh one.  TS: the
    8-row tile with Z = 65, unequal slices from 16-row tiles, and the two-trip finalize from 8-row tiles."""
    row, B = case
    assert case in te.CASES
    run = RUN[te.ROWS[row]["kind"]]
    x = te.inputs(row, B)
    a, m, tp = run_case(row, B)
    b, _, _ = run(x, m, tp)
    c, _, _ = run_case(row, B)
    assert same_bits(a, b) and same_bits(a, c)


# ---- rows across the small tiles --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("r8", 25), ("r16", 49)], ids=te.case_id)
def test_rows_are_independent_across_the_small_tiles(case):
    """A NaN in the last row of the first tile and another in the first row of the next, in obs and in critic_obs: those two rows of mu,
    sigma and values are NaN and every other row keeps the bits of the clean run."""
    row, B = case
    R = te.ROWS[row]["R"]
    assert case in te.CASES and R in (8, 16) and B > 2 * R
    x = te.inputs(row, B)
    clean, _, _ = run_case(row, B)
    y = dict(x, obs=x["obs"].copy(), critic_obs=x["critic_obs"].copy())
    for k in ("obs", "critic_obs"):
        y[k][R - 1, 2] = np.nan
        y[k][R, 0] = np.nan
    got, _, _ = run_case(row, B, y)
    others = np.ones(B, bool)
    others[[R - 1, R]] = False
    for k in ("mu", "sigma", "values"):
        assert np.isnan(got[k][~others]).all(), k
        assert np.array_equal(got[k][others].view(np.uint32), clean[k][others].view(np.uint32)), k


@pytest.mark.parametrize("case", [("ts_r16", 49), ("ts_r8_z", 25)], ids=te.case_id)
def test_ts_rows_are_independent_across_the_small_tiles(case):
    """The same two rows, through the path that only the TS pass has: a NaN in privileged_obs reaches the actor through the latent copied
    behind the observations.  Those two rows of mu and sigma are NaN, every other row of them and every row of values keeps the clean run's
    bits, the critic's gradients too, and the encoder loss (whose targets those rows are) is NaN.  A NaN in obs_history alone leaves mu,
    sigma, values and every RL gradient bit for bit."""
    row, B = case
    R = te.ROWS[row]["R"][0]
    assert case in te.CASES and te.ROWS[row]["R"] in ((8, 8), (16, 16)) and B > 2 * R
    x = te.inputs(row, B)
    rl = sc.rl_names(x["actor"], x["critic"], x["priv"])
    clean, _, _ = run_case(row, B)
    y = dict(x, privileged_obs=x["privileged_obs"].copy())
    y["privileged_obs"][R - 1, 2] = np.nan
    y["privileged_obs"][R, 0] = np.nan
    got, _, _ = run_case(row, B, y)
    others = np.ones(B, bool)
    others[[R - 1, R]] = False
    for k in ("mu", "sigma"):
        assert np.isnan(got[k][~others]).all(), k
        assert np.array_equal(got[k][others].view(np.uint32), clean[k][others].view(np.uint32)), k
    for k in ["values"] + [n for n in rl if n.startswith("critic")]:
        assert np.array_equal(got[k].view(np.uint32), clean[k].view(np.uint32)), k
    assert np.isnan(got["loss"][0])
    theirs = sc.torch_passes(y)
    for n, g in zip(rl, theirs["rl_grads"]):                               # wherever torch's gradient is NaN, so is the kernel's
        assert (np.isnan(got[n]) | ~np.isnan(g)).all(), n
    assert np.isnan(got["privilege_encoder.0.weight"][:, [0, 2]]).all()    # back through the latent into the encoder's first layer
    z = dict(x, obs_history=x["obs_history"].copy())
    z["obs_history"][R - 1, 2] = np.nan
    z["obs_history"][R, 0] = np.nan
    got, _, _ = run_case(row, B, z)
    assert np.isnan(got["loss"][0])
    for k in ["mu", "sigma", "values"] + rl:                                 # the RL pass never reads the history
        assert np.array_equal(got[k].view(np.uint32), clean[k].view(np.uint32)), k


# ---- the 16-byte rows under a stride ----------------------------------------------------------------------------------------------------------
def _place(B, w, place):
    """(the wider filled matrix, its (B, w) view) of a placement; None: the matrix itself."""
    if place is None:
        t = torch.full((B, w), FILL, device=DEV)
        return t, t
    off, stride = place
    wide = torch.full((B, stride), FILL, device=DEV)
    return wide, wide[:, off:off + w]


class _Placed:
    """The matrices of one call, each placed alike: inputs filled from the case, outputs left at the fill."""

    def __init__(self, x, B, place, inputs, outputs):
        self.place, self.wide, self.view, self.inputs = place, {}, {}, list(inputs)
        for k, w in list(inputs.items()) + list(outputs.items()):
            self.wide[k], self.view[k] = _place(B, w, place)
        for k in inputs:
            self.view[k].copy_(dev(x[k]))
        self.before = {k: host(v).copy() for k, v in self.wide.items()}

    def check_untouched(self):
        """Inputs and incoming gradients unchanged; every gap column of an output keeps its fill."""
        for k, wide in self.wide.items():
            after = host(wide)
            if k in self.inputs:
                assert np.array_equal(after, self.before[k]), k
            elif self.place is not None:
                off, w = self.place[0], self.view[k].shape[1]
                gaps = np.ones(after.shape[1], bool)
                gaps[off:off + w] = False
                assert (after[:, gaps] == FILL).all(), k


def _abi_plain(x, place):
    B, (actor, critic) = te.VEC_B, te.VEC_PLAIN
    m = tc.Module(x, DEV)
    D = m.std.device
    spec = train.describe(m, D)
    A, V = actor[-1], critic[-1]
    p = _Placed(x, B, place, dict(obs=actor[0], critic_obs=critic[0], grad_mu=A, grad_sigma=A, grad_values=V), dict(mu=A, sigma=A, values=V))
    v = p.view
    ws = torch.empty(int(train.plan(B, actor, critic).workspace_floats), device=DEV)
    train.forward(train.train_args(spec, v["obs"], v["critic_obs"], v["mu"], v["sigma"], v["values"], ws, device=D), D)
    grads = [torch.full_like(q, FILL) for q in spec.parameters()]
    a = train.train_args(spec, v["obs"], v["critic_obs"], v["mu"], v["sigma"], v["values"], ws, grads, v["grad_mu"], v["grad_sigma"], v["grad_values"], device=D)
    if place is not None:
        assert (a.chain[0].in_stride, a.chain[1].in_stride, a.mu_stride, a.sigma_stride, a.values_stride, a.grad_mu_stride, a.grad_sigma_stride,
                a.grad_values_stride) == (place[1],) * 8
        assert (a.chain[0].input % 16 == 0) == (place[0] % 4 == 0) and (a.mu % 16 == 0) == (place[0] % 4 == 0)
    train.backward(a, D)
    torch.cuda.synchronize()
    p.check_untouched()
    return tc.named(x, {k: host(v[k]) for k in ("mu", "sigma", "values")}, [host(g) for g in grads])


def _abi_ee(x, place):
    B, (est, actor, critic) = te.VEC_B, te.VEC_EE
    m = ec.Module(x, DEV)
    D = m.std.device
    spec = train.describe_ee(m, D)
    A, V, NL = actor[-1], critic[-1], est[-1]
    p = _Placed(x, B, place, dict(features=est[0], critic_obs=critic[0], labels=NL, terminated=1, grad_mu=A, grad_sigma=A, grad_values=V),
                dict(mu=A, sigma=A, values=V))
    v = p.view
    ws = torch.empty(int(train.plan_ee(B, est, actor, critic).workspace_floats), device=DEV)
    train._call("lg_train_ee_forward", train.ee_args(spec, v["features"], v["critic_obs"], v["mu"], v["sigma"], v["values"], ws, device=D), D)
    rl_grads = [torch.full_like(q, FILL) for q in spec.rl_parameters()]
    a = train.ee_args(spec, v["features"], v["critic_obs"], v["mu"], v["sigma"], v["values"], ws, rl_grads, v["grad_mu"], v["grad_sigma"], v["grad_values"], device=D)
    train._call("lg_train_ee_backward", a, D)
    ews = torch.empty(int(train.plan_est(B, est).workspace_floats), device=DEV)
    loss, up = torch.full((), FILL, device=DEV), torch.full((1,), float(x["upstream"]), device=DEV)
    train._call("lg_train_est_forward", train.est_args(spec, v["features"], v["labels"], v["terminated"], loss, ews, device=D), D)
    est_grads = [torch.full_like(q, FILL) for q in spec.estimator_parameters()]
    e = train.est_args(spec, v["features"], v["labels"], v["terminated"], None, ews, est_grads, up, device=D)
    if place is not None:
        assert (a.chain[0].in_stride, a.chain[2].in_stride, a.mu_stride, a.values_stride, a.grad_sigma_stride, e.chain.in_stride, e.labels_stride,
                e.mask_stride) == (place[1],) * 8
    train._call("lg_train_est_backward", e, D)
    torch.cuda.synchronize()
    p.check_untouched()
    return ec.named(x, {k: host(v[k]) for k in ("mu", "sigma", "values")}, [host(g) for g in rl_grads], host(loss), [host(g) for g in est_grads])


def _abi_ts(x, place):
    B, (priv, actor, critic, hist) = te.VEC_B, te.VEC_TS
    m = sc.Module(x, DEV)
    D = m.std.device
    spec = train.describe_ts(m, D)
    A, V, Z = actor[-1], critic[-1], priv[-1]
    p = _Placed(x, B, place, dict(obs=actor[0] - Z, privileged_obs=priv[0], critic_obs=critic[0], obs_history=hist[0], terminated=1, grad_mu=A,
                                  grad_sigma=A, grad_values=V), dict(mu=A, sigma=A, values=V))
    v = p.view
    ws = torch.empty(int(train.plan_ts(B, priv, actor, critic).workspace_floats), device=DEV)
    train._call("lg_train_ts_forward", train.ts_args(spec, v["obs"], v["privileged_obs"], v["critic_obs"], v["mu"], v["sigma"], v["values"], ws, device=D), D)
    rl_grads = [torch.full_like(q, FILL) for q in spec.rl_parameters()]
    a = train.ts_args(spec, v["obs"], v["privileged_obs"], v["critic_obs"], v["mu"], v["sigma"], v["values"], ws, rl_grads, v["grad_mu"], v["grad_sigma"],
                      v["grad_values"], device=D)
    train._call("lg_train_ts_backward", a, D)
    ews = torch.empty(int(train.plan_enc(B, hist, priv).workspace_floats), device=DEV)
    loss, up = torch.full((), FILL, device=DEV), torch.full((1,), float(x["upstream"]), device=DEV)
    train._call("lg_train_enc_forward", train.enc_args(spec, v["obs_history"], v["privileged_obs"], v["terminated"], loss, ews, device=D), D)
    enc_grads = [torch.full_like(q, FILL) for q in spec.encoder_parameters()]
    e = train.enc_args(spec, v["obs_history"], v["privileged_obs"], v["terminated"], None, ews, enc_grads, up, device=D)
    if place is not None:
        assert (a.chain[0].in_stride, a.chain[1].in_stride, a.chain[2].in_stride, a.mu_stride, a.sigma_stride, a.values_stride, a.grad_mu_stride,
                a.grad_sigma_stride, a.grad_values_stride, e.chain[0].in_stride, e.chain[1].in_stride, e.mask_stride) == (place[1],) * 12
        assert (a.chain[1].input % 16 == 0) == (place[0] % 4 == 0) and (e.chain[0].input % 16 == 0) == (place[0] % 4 == 0)
    train._call("lg_train_enc_backward", e, D)
    torch.cuda.synchronize()
    p.check_untouched()
    return sc.named(x, {k: host(v[k]) for k in ("mu", "sigma", "values")}, [host(g) for g in rl_grads], host(loss), [host(g) for g in enc_grads])


@pytest.mark.parametrize("kind", ["plain", "ee", "ts"])
def test_vector_rows_under_a_stride(kind):
    """The C ABI on column slices of wider filled matrices, every width a multiple of 4: base and stride on 16 bytes (the 16-byte accesses
    with stride != width), a base off 16 bytes and an odd stride (the fallbacks) each give the bits of the contiguous call, which lies
    within the parity rule; gaps, inputs and incoming gradients are untouched."""
    x = te.draw(kind, dict(plain=te.VEC_PLAIN, ee=te.VEC_EE, ts=te.VEC_TS)[kind], te.VEC_B, 977)
    call = dict(plain=_abi_plain, ee=_abi_ee, ts=_abi_ts)[kind]
    clean = call(x, None)
    ref64, ref32 = te.KINDS[kind].mod.references(x)
    te.KINDS[kind].mod.check_parity(clean, ref64, ref32, f"vector rows, {kind}, contiguous", RATIOS)
    through_autograd, _, _ = RUN[kind](x)
    assert same_bits(clean, through_autograd)
    for name, place in te.PLACEMENTS.items():
        assert same_bits(call(x, place), clean), name


def test_zz_print_the_parity_ratios():
    """Not a check of its own: the worst |kernel - f64| / max(|torch-f32 - f64|, ulp) per tensor class over every parity check above, for
    DESIGN.md."""
    tg.print_parity_ratios(RATIOS)

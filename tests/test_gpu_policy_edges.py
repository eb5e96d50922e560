"""The fused policy step on the device at the edges the workload's nets do not reach (csrc/lg_policy.hip; the table is tests/policy_edges.py):
the 8-row tile, NT = 2 / 4 sweeps that end ragged, the K boundaries of the 16-wide main loop, row strides above the width and bases off
the 16-byte boundary on every matrix of the ABI, NaN inputs, and parameters updated in place between two calls or two graph replays.

The oracle is the same torch module on the CPU in float64 under the forward-parity rule of tests/test_policy_host.py (factor 8); what the
table's rows plan and reach, the reference's NaN semantics and the discrimination checks are in tests/test_policy_edges_host.py."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import policy_edges as pe
from tests.test_gpu_policy_families import _epilogue
from tests.test_policy_families_host import DWAQ_NETS, TS_NETS, make_dwaq, make_ts
from tests.test_policy_host import NETS, make_net, max_err, parity_bound, philox_uniforms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLIP = 0.05
_GPU = {}


def on_gpu(name, clip=None):
    """The table row's module on the device, moved once."""
    if (name, clip) not in _GPU:
        _GPU[name, clip] = copy.deepcopy(pe.edge_case(name, clip)["module"]).to(DEV)
    return _GPU[name, clip]


def fused(module, seed=0):
    from hcr_genesis_lr_cl_amd.policy import FusedPolicy
    return FusedPolicy(module, seed=seed)


def dev(c, n, *keys):
    return [c[k][:n].to(DEV) for k in keys]


# ---- 1. forward parity over the table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", pe.CASES)
def test_forward_parity_over_the_table(name, n):
    """mu (no Hardtanh: every output carries the whole chain's error), values, the estimator output, and DreamWaQ's params / latents / mu
    with injected noise, against float64 under `parity_bound`; the row tile is the one the table claims."""
    d, c = pe.EDGE_NETS[name], pe.edge_case(name)
    fp = fused(on_gpu(name))
    obs, cobs, noise = dev(c, n, "obs", "cobs", "noise")
    got, kw = {}, {}
    if d["kind"] == "ee":
        kw["labels"] = got["labels"] = torch.full((n, d["est"][1]), 7.5, device=DEV)
    if d["kind"] == "dwaq":
        W = d["L"] + d["E"]
        hist, eps = dev(c, n, "hist", "eps")
        got["latent"], got["params"] = torch.full((n, W), 7.5, device=DEV), torch.full((n, 2 * W), 7.5, device=DEV)
        kw.update(obs_history=hist, latent_noise=eps, latent=got["latent"], latent_params=got["params"])
    fp.act(obs, cobs, noise=noise, **kw)
    torch.cuda.synchronize()
    got.update(mu=fp.last_mu, values=fp.last_values)
    for k, x in got.items():
        pe.check_parity(f"{name} N={n}", x.cpu().numpy(), c, k, n)
    assert fp.row_tile() == d["R"]
    assert int(fp.counter.item()) == 0                                               # both draws injected: nothing was drawn


# ---- 2. the epilogue on the 8-row tile ------------------------------------------------------------------------------------------------------
def test_epilogue_on_the_8_row_tile():
    """wide8 at N = 9 (a full tile and a one-row tile), A = 5 (the second action quad has one live lane): the checks of
    tests/test_gpu_policy_families.py::_epilogue with injected noise; then the Philox path, uniforms bit for bit, the counter once."""
    name, n, seed = "wide8", 9, (0xABCD << 32) | 0x1234
    c, A = pe.edge_case(name, CLIP), pe.EDGE_NETS[name]["A"]
    fp = fused(on_gpu(name, CLIP), seed)
    assert fp.row_tile() == 8
    obs, cobs, noise = dev(c, n, "obs", "cobs", "noise")
    act = fp.act(obs, cobs, noise=noise)
    torch.cuda.synchronize()
    mu = _epilogue(fp, act, c["module"].std.detach().numpy(), c["noise"][:n].numpy().astype(np.float64))
    pe.check_parity(f"{name} clipped N={n}", mu, c, "mu", n)
    assert np.abs(mu).max() == np.float32(CLIP)                                      # the Hardtanh ran on this tile
    mu0, counter = fp.last_mu.clone(), 41
    fp.counter.fill_(counter)
    dbg = torch.full((n, 4 * ((A + 3) // 4)), 7.5, device=DEV)
    act = fp.act(obs, cobs, _dbg_uniform=dbg)
    torch.cuda.synchronize()
    assert np.array_equal(dbg.cpu().numpy(), philox_uniforms(seed, counter, n, A))
    assert int(fp.counter.item()) == counter + 1 and torch.equal(fp.last_mu, mu0)
    assert torch.isfinite(act).all() and not torch.equal(act, mu0)


# ---- 3. strides and misaligned bases --------------------------------------------------------------------------------------------------------
def _padded(n, w, fill=None):
    """An (n, w) view at column 1 of an (n, w + 3) tensor of 7.5: row stride w + 3, base 4 bytes past a 16-byte boundary."""
    whole = torch.full((n, w + 3), 7.5, device=DEV)
    view = whole[:, 1:1 + w]
    if fill is not None:
        view.copy_(fill)
    assert view.data_ptr() % 16 == 4 and view.stride(0) == w + 3
    return whole, view


def _stride_case(family):
    """(module, inputs by keyword, outputs by keyword and width, other keywords) of one family; the inputs are CPU tensors."""
    g = torch.Generator().manual_seed(11)
    r = lambda w: torch.randn(33, w, generator=g)
    if family == "tiny":
        d = NETS["tiny"]
        return make_net("tiny", CLIP), dict(obs=r(d["obs"]), critic_obs=r(d["cobs"]), noise=r(d["A"])), {}, d["A"], {}
    if family == "tiny_ee":
        d = dict(obs=5, est=([9], 2), actor=[33, 7], A=3, cobs=6, critic=[33, 7])
        return pe.make_plain(d, CLIP), dict(obs=r(5), critic_obs=r(6), noise=r(3)), dict(labels=2), 3, {}
    if family == "tiny_ts":
        d = TS_NETS["tiny_ts"]
        x = dict(obs=r(d["obs"]), critic_obs=r(d["cobs"]), privileged_obs=r(d["priv"]), obs_history=r(d["hist"]), noise=r(d["A"]))
        return make_ts("tiny_ts", CLIP), x, {}, d["A"], dict(num_teacher=17)
    d = DWAQ_NETS["tiny_dwaq"]
    W = d["L"] + d["E"]
    x = dict(obs=r(d["obs"]), critic_obs=r(d["cobs"]), obs_history=r(d["hist"]), noise=r(d["A"]), latent_noise=r(W))
    return make_dwaq("tiny_dwaq", CLIP), x, dict(latent=W, latent_params=2 * W), d["A"], {}


@pytest.mark.parametrize("family", ["tiny", "tiny_ee", "tiny_ts", "tiny_dwaq"])
def test_strides_and_misaligned_bases(family):
    """Straight through `policy_args` and `lg_policy_act`: every matrix the ABI gives a stride -- obs, critic obs, privileged obs, history,
    noise, latent noise; actions, mu, sigma, log-prob, values, labels, latent, latent params -- once contiguous and once as a view with
    stride width + 3 whose base is 4 bytes past a 16-byte boundary.  The same kernel sums in the same order, so every output is equal bit
    for bit, and no gap column is touched."""
    from hcr_genesis_lr_cl_amd import abi, policy
    m, x, extra_out, A, kw = _stride_case(family)
    m = m.to(DEV)
    spec = policy.describe(m, torch.device(DEV))
    lib = abi.load_lib()
    n = 33
    outs = dict(actions=A, mu=A, sigma=A, log_prob=1, values=1, **extra_out)
    stream = torch.cuda.current_stream().cuda_stream

    def call(inputs, outputs):
        a = policy.policy_args(spec, inputs["obs"], inputs["critic_obs"], **{k: v for k, v in inputs.items() if k not in ("obs", "critic_obs")},
                               **outputs, **kw)
        abi.check(lib.lg_policy_act(C.byref(a), stream), lib)
        torch.cuda.synchronize()
        return a

    flat_in = {k: v.to(DEV) for k, v in x.items()}
    flat_out = {k: torch.full((n, w), 7.5, device=DEV) for k, w in outs.items()}
    call(flat_in, flat_out)
    pad_in = {k: _padded(n, v.shape[1], v.to(DEV)) for k, v in x.items()}
    pad_out = {k: _padded(n, w) for k, w in outs.items()}
    a = call({k: v[1] for k, v in pad_in.items()}, {k: v[1] for k, v in pad_out.items()})
    assert (a.actor.in_stride, a.critic.in_stride, a.noise_stride, a.mu_stride, a.log_prob_stride) == (x["obs"].shape[1] + 3, x["critic_obs"].shape[1] + 3,
                                                                                                      A + 3, A + 3, 4)
    for k, (whole, view) in pad_out.items():
        assert not (flat_out[k] == 7.5).any() and torch.isfinite(flat_out[k]).all(), k          # the contiguous call wrote everything
        assert torch.equal(view, flat_out[k]), k
        assert (whole[:, 0] == 7.5).all() and (whole[:, 1 + view.shape[1]:] == 7.5).all(), k
    for k, (whole, view) in pad_in.items():
        assert (whole[:, 0] == 7.5).all() and (whole[:, 1 + view.shape[1]:] == 7.5).all() and torch.equal(view, flat_in[k]), k


# ---- 4. NaN is not silent -------------------------------------------------------------------------------------------------------------------
BAD_ROWS = [5, 32]            # 32: the last, partial tile of N = 33


def _poison_run(fp, x, poison_key, **kw):
    """Two calls on N = 33 rows that are the first N of (N + 1)-row allocations whose last row is NaN: clean, and with a NaN in
    BAD_ROWS of `poison_key`.  Returns the two sets of outputs."""
    n = 33
    res = []
    for poisoned in (False, True):
        t = {}
        for k, v in x.items():
            whole = torch.cat((v[:n], torch.full((1, v.shape[1]), float("nan"))), dim=0).to(DEV)
            if poisoned and k == poison_key:
                whole[BAD_ROWS, v.shape[1] // 2] = float("nan")
            t[k] = whole[:n]
        out = {k: torch.full((n, w), 7.5, device=DEV) for k, w in kw.items()}
        fp.act(t["obs"], t["cobs"], noise=t["noise"], **{k: v for k, v in t.items() if k not in ("obs", "cobs", "noise")}, **out)
        torch.cuda.synchronize()
        out.update(mu=fp.last_mu.clone(), sigma=fp.last_sigma.clone(), actions=fp.last_actions.clone(), log_prob=fp.last_log_prob.clone(),
                   values=fp.last_values.clone())
        res.append(out)
    return res


def _check_poisoned(tag, clean, got, nan_keys):
    """The expectation of tests/test_policy_edges_host.py (torch's semantics): the poisoned rows are NaN in `nan_keys`; every other row of
    every output, and every row of the others, is bit for bit the clean call's."""
    n = 33
    ok = [i for i in range(n) if i not in BAD_ROWS]
    assert n - len(ok) <= 2                                                          # the cap: at most 2 of the 33 rows leave the bit-for-bit comparison
    for k, v in got.items():
        print(f"nan {tag} {k}: poisoned rows {v[BAD_ROWS].flatten()[:6].tolist()}")
    for k, v in got.items():
        assert torch.isfinite(clean[k]).all(), (tag, k)
        if k in nan_keys:
            assert torch.isnan(v[BAD_ROWS]).all(), (tag, k, v[BAD_ROWS])
            assert torch.equal(v[ok], clean[k][ok]), (tag, k)
        else:
            assert torch.equal(v, clean[k]), (tag, k)


@pytest.mark.parametrize("clip", [CLIP, None])
@pytest.mark.parametrize("name", ["tiny", "go2"])
def test_nan_observation_reaches_its_own_row(name, clip):
    """A NaN observation is a NaN mean, sigma, action and log-prob of that env row, with the Hardtanh and without it, as with torch
    (`torch.nn.Hardtanh` passes a NaN on); the values, whose input was clean, and all other rows do not change a bit."""
    d = NETS[name]
    g = torch.Generator().manual_seed(11)
    x = dict(obs=torch.randn(33, d["obs"], generator=g), cobs=torch.randn(33, d["cobs"], generator=g), noise=torch.randn(33, d["A"], generator=g))
    fp = fused(make_net(name, clip).to(DEV))
    clean, got = _poison_run(fp, x, "obs")
    if clip is not None:
        assert clean["mu"].abs().max() == CLIP                                       # the clip is live
    _check_poisoned(f"{name} clip={clip}", clean, got, ("mu", "sigma", "actions", "log_prob"))


def test_nan_history_reaches_the_dreamwaq_row():
    """tiny_dwaq: a NaN history row is NaN in all four distribution parameters (the clipped log-variances among them), both latents, and
    mu / sigma / actions / log-prob of that row."""
    d = DWAQ_NETS["tiny_dwaq"]
    W = d["L"] + d["E"]
    g = torch.Generator().manual_seed(11)
    x = {k: torch.randn(33, w, generator=g) for k, w in (("obs", d["obs"]), ("cobs", d["cobs"]), ("obs_history", d["hist"]), ("noise", d["A"]),
                                                         ("latent_noise", W))}
    fp = fused(make_dwaq("tiny_dwaq", CLIP).to(DEV))
    clean, got = _poison_run(fp, x, "obs_history", latent=W, latent_params=2 * W)
    lv = torch.cat((clean["latent_params"][:, d["L"]:2 * d["L"]], clean["latent_params"][:, 2 * d["L"] + d["E"]:]), dim=1)
    assert (lv == 5.0).any() and (lv == -5.0).any() and (lv.abs() < 5.0).any()       # both branches of the log-variance clip and the open one
    _check_poisoned("tiny_dwaq", clean, got, ("mu", "sigma", "actions", "log_prob", "latent", "latent_params"))


# ---- 5. in-place updates are read -----------------------------------------------------------------------------------------------------------
def _update_in_place(m):
    """An optimizer-like step on one layer of each chain and on std, in place."""
    with torch.no_grad():
        m.actor[2].weight.add_(0.01)
        m.actor[2].bias.add_(0.25)
        m.critic[0].weight.add_(-0.01)
        m.critic[0].bias.add_(0.25)
        m.std.mul_(1.5)


def _check_updated(tag, fp, m, c, n, before):
    cpu = copy.deepcopy(m).cpu()
    with torch.no_grad():
        ref = dict(mu=copy.deepcopy(cpu).double().mean(c["obs"][:n].double()).numpy(), values=copy.deepcopy(cpu).double().critic(c["cobs"][:n].double()).numpy())
        f32 = dict(mu=cpu.mean(c["obs"][:n]).numpy(), values=cpu.critic(c["cobs"][:n]).numpy())
    for k, x in (("mu", fp.last_mu), ("values", fp.last_values)):
        ek, et = max_err(x.cpu().numpy(), ref[k]), max_err(f32[k], ref[k])
        print(f"parity {tag} {k}: kernel {ek:.3e} torch-f32 {et:.3e} bound {parity_bound(et, ref[k]):.3e}, moved by {float((x - before[k]).abs().max()):.3e}")
        assert ek <= parity_bound(et, ref[k]), (tag, k, ek, et)
        assert float((x - before[k]).abs().max()) > 100 * parity_bound(et, ref[k]), (tag, k)          # the old parameters would be far outside
    assert torch.equal(fp.last_sigma, cpu.std.detach().to(DEV).expand_as(fp.last_sigma)) and not torch.equal(fp.last_sigma, before["sigma"])


def _go2_inputs(n):
    g = torch.Generator().manual_seed(11)
    d = NETS["go2"]
    return dict(obs=torch.randn(n, d["obs"], generator=g), cobs=torch.randn(n, d["cobs"], generator=g), noise=torch.randn(n, d["A"], generator=g))


def test_in_place_update_is_read_by_the_next_call():
    n = 33
    c = _go2_inputs(n)
    m = make_net("go2", None).to(DEV)
    fp = fused(m)
    obs, cobs, noise = dev(c, n, "obs", "cobs", "noise")
    fp.act(obs, cobs, noise=noise)
    torch.cuda.synchronize()
    before = dict(mu=fp.last_mu.clone(), values=fp.last_values.clone(), sigma=fp.last_sigma.clone())
    _update_in_place(m)
    fp.act(obs, cobs, noise=noise)
    torch.cuda.synchronize()
    _check_updated("in-place go2", fp, m, c, n, before)


def test_in_place_update_is_read_by_the_next_replay():
    n = 33
    c = _go2_inputs(n)
    m = make_net("go2", None).to(DEV)
    fp = fused(m)
    obs, cobs, noise = dev(c, n, "obs", "cobs", "noise")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fp.act(obs, cobs, noise=noise)                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        fp.act(obs, cobs, noise=noise)
    gph.replay()
    torch.cuda.synchronize()
    before = dict(mu=fp.last_mu.clone(), values=fp.last_values.clone(), sigma=fp.last_sigma.clone())
    _update_in_place(m)
    torch.cuda.synchronize()
    gph.replay()
    torch.cuda.synchronize()
    _check_updated("in-place go2, replayed", fp, m, c, n, before)

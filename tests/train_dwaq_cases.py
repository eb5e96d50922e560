"""The cases of the DreamWaQ learner passes (include/lgtraindwaq.h), shared by tests/test_train_dwaq_host.py (CPU) and
tests/test_gpu_train_dwaq.py (GPU): one net table, one case table, the input generator, a numpy restatement of both passes built on
tests/train_support.py's layers and batch sums (float64: the reference of every comparison; float32 with the plan's slices and row tile:
the kernel's order of sums), the same passes as torch autograd on the CPU in the reference's own arithmetic (the (B,) x (B, 1) broadcast of
the KL term included), the plans restated, a Module with the reference's member names, and the loader of the golden fixture
(tests/golden/gen_ppo_dwaq_train_fixtures.py); the plan's rules, the parity rule and the fixture readers are tests/train_support.py's.
Nothing here loads the HIP library."""
import numpy as np
import torch

from tests import train_support as sup
from tests.train_support import CLASSES, chain_backward, check_parity, fixture_loss_inputs, tensor_class          # noqa: F401

# name -> (encoder widths, L, E, decoder widths, actor widths, critic widths).  EVERY encoder layer carries an ELU, the last too; the four
# heads are H -> L, L, E, E with H the encoder's last width; decoder[0] = L + E; actor[0] = O + L + E.  The actor ends in a Hardtanh only
# where the case has a clip.
NETS = {
    "fixture":  ([14, 8, 6, 10], 3, 2, [5, 8, 4, 5], [12, 8, 4, 3], [9, 8, 4, 1]),
    "go2_dwaq": ([900, 256, 128, 80], 16, 24, [40, 256, 128, 45], [85, 512, 256, 128, 12], [885, 1024, 256, 128, 1]),
    "one_one":  ([9, 7], 4, 3, [7, 6], [12, 19, 16, 15, 4], [6, 17, 1]),       # decoder layer 0 is also its last; the encoder's only layer carries the ELU
    "wide":     ([2048, 2048, 8], 3, 2, [5, 7, 3], [2048, 2048, 3], [8, 5, 1]),      # the 8-row tile in both passes
}
RAGGED = (1, 4, 5, 16, 17, 65)
_OBS = {1: 3, 4: 4, 5: 4, 16: 1, 17: 16, 65: 3}            # O per L: O and O + L fall off and on multiples of 4
for _l in RAGGED:
    for _e in RAGGED:
        NETS[f"l{_l}_e{_e}"] = ([5, 6, 7], _l, _e, [_l + _e, 9, 4], [_OBS[_l] + _l + _e, 9, 3], [4, 5, 1])
SWEEP = [f"l{l}_e{e}" for l in RAGGED for e in RAGGED]
for _h in (1, 5, 80):                                      # the encoder's output width: the heads' K
    NETS[f"h{_h}"] = ([6, 7, _h], 5, 4, [9, 6, 3], [12, 8, 2], [4, 5, 1])
HWIDTHS = ["h1", "h5", "h80"]
REAL = ("go2_dwaq",)

BATCHES = (1, 31, 33, 257)
CASES = {}
for _net in ("fixture", "one_one") + REAL:
    for _b in BATCHES:
        CASES[f"{_net}_b{_b}"] = dict(net=_net, B=_b, seed=1300 + len(CASES))
for _net in SWEEP + HWIDTHS:
    CASES[f"{_net}_b33"] = dict(net=_net, B=33, seed=1300 + len(CASES))
for _b in (1, 9):
    CASES[f"wide_b{_b}"] = dict(net="wide", B=_b, seed=1300 + len(CASES))
CASES["fixture_noclip_b33"] = dict(net="fixture", B=33, seed=1390, clip=None)          # ActorCriticDreamWaQ as it stands: no Hardtanh
# 257 loss tiles of 32 rows (the finalize kernel's second trip over four partial streams) and the cap of 32 slices with a short last one
CASES["fixture_b8193"] = dict(net="fixture", B=8193, seed=1392)
RAGGED_SLICE_NETS = ("fixture", "one_one") + REAL        # plus, per net, the smallest B either plan slices raggedly
# A draw is a table case only if the float32 numpy restatement in the kernel's order of sums keeps HALF the parity rule on it
# (tests/test_train_dwaq_host.py holds the whole table to that, on the CPU).  The rule divides by ONE torch float32 evaluation; where that
# evaluation happens to land within a fraction of an ulp (a (1, 1) `values` at B = 1, a bias gradient of five elements), any other float32
# evaluation of the same numbers, numpy's included, is several times worse, and the case measures the draw's luck, not a kernel.  Six
# default draws (seed 1300 + the case's index, 1392 for fixture_b8193) fail that criterion; each takes the next free seed from 1393 on at
# which it holds (1393 fails it for go2_dwaq_b1, `values` 0.08 ulp on the torch side, and 1399 for fixture_b8193).
RESEEDED = dict(go2_dwaq_b1=1394, l4_e65_b33=1395, l16_e5_b33=1396, h5_b33=1397, wide_b1=1398, fixture_b8193=1400)
for _name, _seed in RESEEDED.items():
    CASES[_name] = dict(CASES[_name], seed=_seed)

RED_BYTES = 256 * 8            # the VAE forward's float64 tree (LG_TRAIN_DWAQ_THREADS doubles)
TARGET_JOBS = 2048             # LG_TRAIN_DWAQ_TARGET_JOBS
N_LOSSES = 4                   # LG_TRAIN_VAE_LOSSES
HEADS = ("latent_mu", "latent_var", "vel_mu", "vel_var")
LOSSES = ("loss", "est_loss", "rec_loss", "kld_loss")
KLD_WEIGHT = 0.5


def head_widths(enc, L, E):
    return [[enc[-1], w] for w in (L, L, E, E)]


# ---- the plans ------------------------------------------------------------------------------------------------------------------------------
def _front_widths(enc, L, E, products):
    """The LDS widths behind the encoder and the heads, and the activation X the encoder ends in."""
    xi = (len(enc) - 1) & 1
    w = sup.lds_widths([(enc, 0)] + [(h, xi) for h in head_widths(enc, L, E)])
    w[xi ^ 1] = max(w[xi ^ 1], 2 * sup.lds_stride(L) + 2 * sup.lds_stride(E))          # the heads' four disjoint regions
    if products:
        w[xi] = max(w[xi], 2 * sup.lds_stride(enc[-1]))                                # the backward's two product regions
    return w, xi


def restated_plan_dwaq(n_rows, enc, L, E, actor, critic):
    """include/lgtraindwaq.h's plan of the RL pass; the per-chain lists hold the actor and the critic (chains 5 and 6)."""
    w, xi = _front_widths(enc, L, E, False)
    w = [max(a, b) for a, b in zip(w, sup.lds_widths(((actor, xi), (critic, 0))))]
    row_tile, lds_bytes = sup.row_tile(w)
    d, off, jobs = sup.offsets(n_rows, (actor, critic), n_rows * actor[0], TARGET_JOBS)
    std = sup.slice_rule(n_rows, 1, TARGET_JOBS)
    d.update(row_tile=row_tile, lds_bytes=lds_bytes, lds_x=xi, cat_off=0, std=std, std_p_off=off, workspace_floats=off + std[0] * actor[-1],
             weight_jobs=jobs + std[0])
    return d


def restated_plan_vae(n_rows, enc, L, E, dec):
    """The VAE pass: the per-chain lists hold the encoder, the four heads and the decoder (chains 0-5)."""
    w, xi = _front_widths(enc, L, E, True)
    w = [max(a, b) for a, b in zip(w, sup.lds_widths(((dec, xi),)))]
    row_tile, lds_bytes = sup.row_tile(w, RED_BYTES)
    off = n_rows * (L + E)
    head_off = []
    for wd in (L, L, E, E):
        head_off.append(off)
        off += n_rows * wd
    gl_rec, gl_est = off, off + n_rows * dec[-1]
    off = gl_est + n_rows * E
    d, off, jobs = sup.offsets(n_rows, [enc] + head_widths(enc, L, E) + [dec], off, TARGET_JOBS)
    enc_out = off
    off += n_rows * enc[-1]
    off += off & 1
    tiles = -(-n_rows // row_tile)
    d.update(row_tile=row_tile, lds_bytes=lds_bytes, lds_x=xi, cat_off=0, head_off=head_off, gl_rec_off=gl_rec, gl_est_off=gl_est, enc_out_off=enc_out,
             partial_off=off, scale_off=off + 2 * N_LOSSES * tiles, loss_tiles=tiles, workspace_floats=off + 2 * N_LOSSES * tiles + 2, weight_jobs=jobs)
    return d


def smallest_ragged_b(net):
    """The smallest batch at which some layer of either pass gets more than one slice and a last slice shorter than the others."""
    enc, L, E, dec, actor, critic = NETS[net]
    return sup.smallest_ragged_b(lambda b: restated_plan_dwaq(b, enc, L, E, actor, critic), lambda b: restated_plan_vae(b, enc, L, E, dec))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def _chain_names(name, c, step=2):          # the names torch gives: an ELU sits between the Linears of a Sequential
    return [f"{name}.{step * i}.{k}" for i in range(len(c) - 1) for k in ("weight", "bias")]


def rl_names(actor, critic):
    """PPO_DreamWaQ.rl_parameters' order: actor, critic, std."""
    return _chain_names("actor", actor) + _chain_names("critic", critic) + ["std"]


def vae_names(enc, dec):
    """vae.parameters()' order: encoder, latent_mu, latent_var, vel_mu, vel_var, decoder."""
    return _chain_names("vae.encoder", enc) + [f"vae.{h}.{k}" for h in ("latent_mu", "latent_var.0", "vel_mu", "vel_var.0") for k in ("weight", "bias")] + \
        _chain_names("vae.decoder", dec)


def make_inputs(case):
    """float32 numpy inputs of a case (a name of CASES, or a dict of B, seed and either `net` or `widths` = a NETS tuple): dict(enc, L, E,
    dec, actor, critic (widths), clip, var_clip, kld_weight, rl_params (rl_names order), vae_params (vae_names order), obs, obs_history,
    critic_obs, noise (the RL pass's), labels, next_states, terminated, vae_noise, grad_mu, grad_sigma, grad_values, upstream).  Both clips as
    tests/train_support.place_clip places them: a good share of the means and of the log-variances saturates and none lies within 1e-3 of
    its clip.  A case with clip=None has no Hardtanh behind the actor."""
    c = CASES[case] if isinstance(case, str) else case
    enc, L, E, dec, actor, critic = c["widths"] if "widths" in c else NETS[c["net"]]
    rng, B, f = np.random.default_rng(c["seed"]), c["B"], np.float32
    std = (0.5 + rng.random(actor[-1])).astype(f)
    heads = [p for h in head_widths(enc, L, E) for p in sup.draw_layers(rng, h)]
    for i in (2, 6):                                      # the log-variance heads reach well past +-1
        heads[i] = (heads[i] * f(3.0)).astype(f)
    x = dict(enc=list(enc), L=L, E=E, dec=list(dec), actor=list(actor), critic=list(critic), clip=None, var_clip=None, kld_weight=KLD_WEIGHT,
             rl_params=sup.draw_layers(rng, actor) + sup.draw_layers(rng, critic) + [std],
             vae_params=sup.draw_layers(rng, enc) + heads + sup.draw_layers(rng, dec),
             obs=rng.normal(size=(B, actor[0] - L - E)).astype(f), obs_history=rng.normal(size=(B, enc[0])).astype(f),
             critic_obs=rng.normal(size=(B, critic[0])).astype(f), noise=rng.normal(size=(B, L + E)).astype(f),
             labels=rng.normal(size=(B, E)).astype(f), next_states=rng.normal(size=(B, dec[-1])).astype(f),
             terminated=(rng.random((B, 1)) > 0.3).astype(f), vae_noise=rng.normal(size=(B, L + E)).astype(f),
             grad_mu=rng.normal(size=(B, actor[-1])).astype(f), grad_sigma=rng.normal(size=(B, actor[-1])).astype(f),
             grad_values=rng.normal(size=(B, critic[-1])).astype(f), upstream=f(0.75))
    fr = front(x, x["obs_history"])
    x["var_clip"] = sup.place_clip(np.concatenate([fr["pre"][1], fr["pre"][3]], axis=1))
    if not ("clip" in c and c["clip"] is None):
        x["clip"] = sup.place_clip(rl_forward(x)["mu"])
    return x


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def elu(h, dtype):
    return np.where(h > 0, h, np.expm1(np.minimum(h, 0))).astype(dtype)


def split_vae(x, dtype=np.float64):
    """(encoder, [latent_mu, latent_var, vel_mu, vel_var], decoder) as lists of (W, b) from x["vae_params"]."""
    ne = 2 * (len(x["enc"]) - 1)
    p = x["vae_params"]
    return sup.pairs(p[:ne], dtype), sup.pairs(p[ne:ne + 8], dtype), sup.pairs(p[ne + 8:], dtype)


def split_rl(x, dtype=np.float64):
    na = 2 * (len(x["actor"]) - 1)
    p = x["rl_params"]
    return sup.pairs(p[:na], dtype), sup.pairs(p[na:-1], dtype), np.asarray(p[-1]).astype(dtype)


def front(x, history, dtype=np.float64, noise=None):
    """The encoder (an ELU behind EVERY layer), the four heads and, with `noise`, the draw: dict(acts (the encoder's [input, outputs...]),
    pre (the heads before the clip), out (behind it), z, v)."""
    enc, heads, _ = split_vae(x, dtype)
    acts = [np.asarray(history).astype(dtype)]
    for W, b in enc:
        acts.append(elu(acts[-1] @ W.T + b, dtype))
    pre = [(acts[-1] @ W.T + b).astype(dtype) for W, b in heads]
    vc = x["var_clip"]
    out = [pre[0], sup.hardtanh(pre[1], vc, dtype), pre[2], sup.hardtanh(pre[3], vc, dtype)]
    d = dict(acts=acts, pre=pre, out=out)
    if noise is not None:
        eps = np.asarray(noise).astype(dtype)
        L = x["L"]
        d["z"] = (eps[:, :L] * np.exp(dtype(0.5) * out[1]) + out[0]).astype(dtype)
        d["v"] = (eps[:, L:] * np.exp(dtype(0.5) * out[3]) + out[2]).astype(dtype)
    return d


def rl_forward(x, dtype=np.float64):
    """dict(mu, sigma, values, cat, acts=(actor, critic activations)) of include/lgtraindwaq.h's RL forward."""
    actor, critic, std = split_rl(x, dtype)
    fr = front(x, x["obs_history"], dtype, x["noise"])
    cat = np.concatenate([np.asarray(x["obs"]).astype(dtype), fr["z"], fr["v"]], axis=1)
    aa = sup.mlp(actor, cat, dtype)
    ca = sup.mlp(critic, np.asarray(x["critic_obs"]).astype(dtype), dtype)
    mu = sup.hardtanh(aa[-1], x["clip"], dtype)
    return dict(mu=mu, sigma=mu * 0 + std, values=ca[-1], cat=cat, acts=(aa, ca))


def rl_backward(x, dtype=np.float64, slices=None):
    """The gradients of the RL pass in rl_names order (actor, critic, std); the VAE gets none.  `slices`: dict(std=rows, actor=[rows per
    layer], critic=[...]) as the plan slices each sum, or None."""
    fw = rl_forward(x, dtype)
    actor, critic, _ = split_rl(x, dtype)
    aa, ca = fw["acts"]
    B, s = fw["mu"].shape[0], slices or {}
    ga, _ = chain_backward(actor, aa, sup.masked_grad_mu(x["grad_mu"], fw["mu"], x["clip"], dtype), dtype, s.get("actor"))
    gc, _ = chain_backward(critic, ca, np.asarray(x["grad_values"]).astype(dtype), dtype, s.get("critic"))
    return ga + gc + [sup.slice_sum(int(s.get("std", B)), np.asarray(x["grad_sigma"]).astype(dtype))]


def _tile_sum(a, row_tile):
    """The float64 sum of `a` over the batch: at once, or per row tile and then in tile order."""
    a = a.astype(np.float64)
    if not row_tile:
        return a.sum()
    total = 0.0
    for r0 in range(0, a.shape[0], row_tile):
        total = total + a[r0:r0 + row_tile].sum()
    return total


WRONG = ("kld_per_row", "est_from_mu", "latent_cols", "no_var_mask", "select")


def vae_pass(x, dtype=np.float64, upstream=None, slices=None, row_tile=None, wrong=None):
    """dict(losses (total, estimation, reconstruction, kld), grads (vae_names order), z, v, rec, head_g) of the VAE pass, in the reference's
    arithmetic: est = sum ((v - labels) t)^2 / (B E), recl = sum ((rec - next) t)^2 / (B D), kld = -0.5 (sum_i s_i)(sum_j t_j) / B^2 (the
    (B,) x (B, 1) broadcast), loss = est + recl + kld_weight kld; the gradients times `upstream` (default x["upstream"]).  `slices`: rows per
    slice per layer, [encoder, the four heads ..., decoder]; row_tile: the four sums as float64 partials per tile added in tile order.
    Planted defects (`wrong`): kld_per_row, the KL term with each row under its own mask (the "fixed" broadcast); est_from_mu, vel_mu in
    place of the sampled v in the estimation loss; latent_cols, the latent gradient from the decoder's LAST L input columns; no_var_mask,
    the log-variance gradients past their Hardtanh's mask; select, the mask as a select."""
    assert wrong is None or wrong in WRONG
    enc, heads, dec = split_vae(x, dtype)
    fr = front(x, x["obs_history"], dtype, x["vae_noise"])
    lmu, llv, vmu, vlv = fr["out"]
    z, v, L, E = fr["z"], fr["v"], x["L"], x["E"]
    eps = np.asarray(x["vae_noise"]).astype(dtype)
    t = np.asarray(x["terminated"]).astype(dtype)
    B, D, kw = t.shape[0], x["dec"][-1], dtype(x["kld_weight"])
    da = sup.mlp(dec, np.concatenate([z, v], axis=1), dtype)
    rec = da[-1]
    pv = vmu if wrong == "est_from_mu" else v
    with np.errstate(invalid="ignore"):
        if wrong == "select":
            d_est, d_rec = np.where(t != 0, pv - np.asarray(x["labels"]).astype(dtype), 0).astype(dtype), \
                np.where(t != 0, rec - np.asarray(x["next_states"]).astype(dtype), 0).astype(dtype)
        else:
            d_est = ((pv - np.asarray(x["labels"]).astype(dtype)) * t).astype(dtype)
            d_rec = ((rec - np.asarray(x["next_states"]).astype(dtype)) * t).astype(dtype)
    s_el = (((1 + llv) - lmu * lmu) - np.exp(llv)).astype(dtype)
    est = _tile_sum(d_est ** 2 if dtype == np.float64 else d_est.astype(np.float64) ** 2, row_tile) / (B * E)
    recl = _tile_sum(d_rec.astype(np.float64) ** 2, row_tile) / (B * D)
    T = _tile_sum(t, row_tile)
    f64 = T / (float(B) * float(B))
    if wrong == "kld_per_row":
        kld = -0.5 * float((s_el.astype(np.float64).sum(1) * t[:, 0].astype(np.float64)).sum()) / B
        row_f = (t / dtype(B)).astype(dtype)                      # each row's own factor t_i / B
    else:
        kld = -0.5 * _tile_sum(s_el, row_tile) * f64
        row_f = dtype(f64)
    losses = np.array([est + recl + float(kw) * kld, est, recl, kld], np.float64)
    up = dtype(x["upstream"] if upstream is None else upstream)
    if dtype == np.float32:
        G_dec = ((d_rec * t * dtype(2.0 / (dtype(B) * dtype(D)))) * up).astype(dtype)
        g_est = ((d_est * t * dtype(2.0 / (dtype(B) * dtype(E)))) * up).astype(dtype)
    else:
        G_dec = (2 * d_rec * t / (B * D) * up).astype(dtype)
        g_est = (2 * d_est * t / (B * E) * up).astype(dtype)
    s = slices or [None] * 6
    gdec, dzv = chain_backward(dec, da, G_dec, dtype, s[5], input_grad=True)
    g_z = dzv[:, E:] if wrong == "latent_cols" else dzv[:, :L]
    g_v = dzv[:, L:]
    kf = (kw * row_f * up)
    if wrong == "est_from_mu":
        G_vmu, g_v_draw = (g_v + g_est).astype(dtype), g_v
    else:
        G_vmu = g_v_draw = (g_v + g_est).astype(dtype)
    G = [(g_z + lmu * kf).astype(dtype),
         (g_z * eps[:, :L] * (dtype(0.5) * np.exp(dtype(0.5) * llv)) + dtype(-0.5) * (1 - np.exp(llv)) * kf).astype(dtype),
         G_vmu,
         (g_v_draw * eps[:, L:] * (dtype(0.5) * np.exp(dtype(0.5) * vlv))).astype(dtype)]
    if wrong != "no_var_mask":
        vc = x["var_clip"]
        for i, lv in ((1, llv), (3, vlv)):
            G[i] = np.where((lv >= vc) | (lv <= -vc), 0, G[i]).astype(dtype)
    h = fr["acts"][-1]
    ghead, dh = [], None
    for i, (Gi, hd) in enumerate(zip(G, heads)):
        g, p = chain_backward([hd], [h, None], np.ascontiguousarray(Gi), dtype, s[1 + i], input_grad=True)
        ghead += g
        dh = p if dh is None else (dh + p).astype(dtype)          # in head order
    G_enc = (dh * np.where(h > 0, 1, h + 1)).astype(dtype)
    genc, _ = chain_backward(enc, fr["acts"], G_enc, dtype, s[0])
    return dict(losses=losses.astype(dtype) if dtype == np.float32 else losses, grads=genc + ghead + gdec, z=z, v=v, rec=rec, head_g=G, front=fr)


def kernel_order_slices(x):
    """The rows per slice of every batch sum as the restated plans give them: (rl_backward's `slices`, vae_pass's `slices`, the VAE pass's row
    tile)."""
    B = np.asarray(x["obs"]).shape[0]
    p = restated_plan_dwaq(B, x["enc"], x["L"], x["E"], x["actor"], x["critic"])
    q = restated_plan_vae(B, x["enc"], x["L"], x["E"], x["dec"])
    return dict(std=p["std"][1], actor=p["slice_rows"][0], critic=p["slice_rows"][1]), q["slice_rows"], q["row_tile"]


# ---- the torch side -------------------------------------------------------------------------------------------------------------------------
BROADCAST_ROWS = 4096          # above this the (B, B) product of the KL term is written as the product of its two sums


def _vae_t(hist, noise, vae, x):
    """The reference's VAE forward in torch ops: ((z, v), (latent_mu, latent_var, vel_mu, vel_var)) from the parameters in vae_names order."""
    F = torch.nn.functional
    ne = 2 * (len(x["enc"]) - 1)
    h = hist
    for i in range(0, ne, 2):
        h = F.elu(F.linear(h, vae[i], vae[i + 1]))
    lin = [F.linear(h, vae[ne + 2 * i], vae[ne + 2 * i + 1]) for i in range(4)]
    vc = float(x["var_clip"])
    lmu, llv, vmu, vlv = lin[0], F.hardtanh(lin[1], -vc, vc), lin[2], F.hardtanh(lin[3], -vc, vc)
    L = x["L"]
    z = noise[:, :L] * torch.exp(0.5 * llv) + lmu
    v = noise[:, L:] * torch.exp(0.5 * vlv) + vmu
    return (z, v), (lmu, llv, vmu, vlv)


def _vae_loss_t(vae, x, hist, labels, nxt, term, noise):
    """PPO_DreamWaQ._compute_vae_loss in torch ops: (loss, est, rec, kld)."""
    F = torch.nn.functional
    (z, v), (lmu, llv, _, _) = _vae_t(hist, noise, vae, x)
    ne = 2 * (len(x["enc"]) - 1)
    rec = sup.mlp_t(torch.cat([z, v], dim=1), vae[ne + 8:])
    est = F.mse_loss(v * term, labels * term)
    recl = F.mse_loss(rec * term, nxt * term)
    s = torch.sum(1 + llv - lmu ** 2 - llv.exp(), dim=1)
    if s.shape[0] <= BROADCAST_ROWS:
        kld = -0.5 * torch.mean(s * term)                      # (B,) times (B, 1): the reference's (B, B) product
    else:
        kld = -0.5 * (s.sum() * term.sum()) / float(s.shape[0]) ** 2
    return est + recl + float(x["kld_weight"]) * kld, est, recl, kld


def torch_passes(x, dtype=torch.float32):
    """Both passes as torch computes them on the CPU in `dtype`: dict(mu, sigma, values, rl_grads, vae_rl_grads (what the RL cotangents send
    into the VAE: they DO reach it; the pass discards them as the reference's zero_grad does), losses, vae_grads, rl_vae_grads (what the VAE
    loss sends into actor, critic and std: None each)), float64 numpy."""
    t = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)
    rl = [t(p).requires_grad_(True) for p in x["rl_params"]]
    vae = [t(p).requires_grad_(True) for p in x["vae_params"]]
    na = 2 * (len(x["actor"]) - 1)
    (z, v), _ = _vae_t(t(x["obs_history"]), t(x["noise"]), vae, x)
    mu = sup.mlp_t(torch.cat((t(x["obs"]), z, v), dim=-1), rl[:na])
    if x["clip"] is not None:
        mu = torch.nn.functional.hardtanh(mu, -x["clip"], x["clip"])
    sigma = mu * 0.0 + rl[-1]
    values = sup.mlp_t(t(x["critic_obs"]), rl[na:-1])
    n = lambda v: None if v is None else v.detach().double().numpy().copy()
    out = dict(mu=n(mu), sigma=n(sigma), values=n(values))
    if "grad_mu" in x:
        torch.autograd.backward([mu, sigma, values], [t(x["grad_mu"]), t(x["grad_sigma"]), t(x["grad_values"])])
        out.update(rl_grads=[n(p.grad) for p in rl], vae_rl_grads=[n(p.grad) for p in vae])
        for p in rl + vae:
            p.grad = None
    losses = _vae_loss_t(vae, x, t(x["obs_history"]), t(x["labels"]), t(x["next_states"]), t(x["terminated"]), t(x["vae_noise"]))
    (losses[0] * float(x.get("upstream", 1.0))).backward()
    out.update(losses=np.array([float(l.detach().double()) for l in losses]), vae_grads=[n(p.grad) for p in vae], rl_vae_grads=[n(p.grad) for p in rl])
    return out


def named(x, outs, rl_grads, vae_grads):
    """dict name -> array of both passes' outputs and gradients; the four losses are in named_losses."""
    d = dict(mu=outs["mu"], sigma=outs["sigma"], values=outs["values"])
    d.update(zip(rl_names(x["actor"], x["critic"]), rl_grads))
    d.update(zip(vae_names(x["enc"], x["dec"]), vae_grads))
    return d


def named_losses(losses):
    """The four loss scalars one dict at a time under the name `loss`, which is what tests/train_support.tensor_class knows: [(label,
    {"loss": array})]."""
    a = np.asarray(losses, np.float64).reshape(-1)
    return [(k, dict(loss=a[i:i + 1])) for i, k in enumerate(LOSSES)]


def references(x):
    """(float64 restatement, torch CPU float32) of a case as `named` dicts, and the same for the four losses as lists of named_losses."""
    fw, e, t32 = rl_forward(x), vae_pass(x), torch_passes(x)
    return named(x, fw, rl_backward(x), e["grads"]), named(x, t32, t32["rl_grads"], t32["vae_grads"]), named_losses(e["losses"]), named_losses(t32["losses"])


def check_case(got, got_losses, x, label, report=None, factor=None, refs=None):
    """check_parity of a result (`named` dict and four losses) against references(x): the tensors at once, the four losses one at a time."""
    r64, r32, l64, l32 = refs if refs is not None else references(x)
    kw = {} if factor is None else dict(factor=factor)
    check_parity(got, r64, r32, label, report, **kw)
    for (k, g), (_, a), (_, b) in zip(named_losses(got_losses), l64, l32):
        check_parity(g, a, b, f"{label} {k}", report, **kw)


# ---- the module -----------------------------------------------------------------------------------------------------------------------------
class VAE(torch.nn.Module):
    """rsl_rl/modules/vae.py's members by name: encoder (an ELU behind every Linear), latent_mu, latent_var (Linear + Hardtanh), vel_mu,
    vel_var, decoder, registered in that order."""

    def __init__(self, x):
        super().__init__()
        nn, mods = torch.nn, []
        for i in range(len(x["enc"]) - 1):
            mods += [nn.Linear(x["enc"][i], x["enc"][i + 1]), nn.ELU()]
        self.encoder = nn.Sequential(*mods)
        H, vc = x["enc"][-1], float(x["var_clip"])
        self.latent_mu = nn.Linear(H, x["L"])
        self.latent_var = nn.Sequential(nn.Linear(H, x["L"]), nn.Hardtanh(-vc, vc))
        self.vel_mu = nn.Linear(H, x["E"])
        self.vel_var = nn.Sequential(nn.Linear(H, x["E"]), nn.Hardtanh(-vc, vc))
        self.decoder = sup.sequential(x["dec"], None)


class Module(torch.nn.Module):
    """ActorCriticDreamWaQ's members as FusedTrainPassDreamWaQ reads them, registered in the reference's order (vae, actor, critic, std),
    holding a case's parameters.  The actor ends in a Hardtanh where the case has a clip (ActorCriticDreamWaQ itself has none)."""

    def __init__(self, x, device="cpu", dtype=torch.float32):
        super().__init__()
        self.x = dict(enc=x["enc"], L=x["L"], E=x["E"], dec=x["dec"], var_clip=x["var_clip"], kld_weight=x["kld_weight"])
        self.vae = VAE(x)
        self.actor, self.critic = sup.sequential(x["actor"], x["clip"]), sup.sequential(x["critic"], None)
        self.std = torch.nn.Parameter(torch.zeros(x["actor"][-1]))
        self.to(device=device, dtype=dtype)
        sup.set_parameters(self.rl_parameters() + self.vae_parameters(), list(x["rl_params"]) + list(x["vae_params"]), dtype)

    def rl_parameters(self):
        return list(self.actor.parameters()) + list(self.critic.parameters()) + [self.std]

    def vae_parameters(self):
        return list(self.vae.parameters())

    def forward(self, obs, obs_history, critic_obs, noise):
        (z, v), _ = _vae_t(obs_history, noise, self.vae_parameters(), self.x)
        mu = self.actor(torch.cat((obs, z, v), dim=-1))
        return mu, mu * 0.0 + self.std, self.critic(critic_obs)

    def vae_loss(self, obs_history, labels, next_states, terminated, noise):
        return _vae_loss_t(self.vae_parameters(), self.x, obs_history, labels, next_states, terminated, noise)


# ---- the golden fixture ---------------------------------------------------------------------------------------------------------------------
FIXTURE_COLUMNS = ("obs", "critic_obs", "obs_history", "noise", "actions", "target_values", "advantages", "returns", "old_log_prob", "old_mu", "old_sigma")
VAE_COLUMNS = ("vae_history", "vae_labels", "vae_next_states", "vae_terminated", "vae_noise")
CFG_KEYS = ("lr0", "beta1", "beta2", "eps", "max_grad_norm", "desired_kl", "steps", "clip_param", "value_loss_coef", "entropy_coef", "encoder_lr",
            "vae_steps", "vae_epochs", "kld_weight", "var_clip")


def load_fixture(path):
    """tests/train_support.load_two_pass_fixture's dict with enc / dec / actor / critic widths, L and E: per RL step the columns, noise, mu,
    sigma, values, loss, kl, lr, grad_norm, grads, params; per VAE step vae_history, vae_labels, vae_next_states, vae_terminated, vae_noise,
    vae_losses, vae_grads, vae_grad_norm, vae_params.  The steps interleave: RL step s, then VAE steps vae_epochs * s ..."""
    chains = dict(enc="vae.encoder", dec="vae.decoder", actor="actor", critic="critic")
    fx = sup.load_two_pass_fixture(path, CFG_KEYS, chains, "vae", FIXTURE_COLUMNS + VAE_COLUMNS + (
        "mu", "sigma", "values", "loss", "kl", "lr", "grad_norm", "vae_losses", "vae_grad_norm"))
    fx["L"], fx["E"] = fx["shapes"]["vae.latent_mu.weight"][0], fx["shapes"]["vae.vel_mu.weight"][0]
    return fx


def fixture_inputs(fx, params, rl_step=None, vae_step=None):
    """The inputs of one step of the fixture around `params` (name -> array), as make_inputs shapes them, float64.  No actor clip: the
    reference's ActorCriticDreamWaQ has no Hardtanh."""
    x = dict(enc=fx["enc"], L=fx["L"], E=fx["E"], dec=fx["dec"], actor=fx["actor"], critic=fx["critic"], clip=None, var_clip=fx["cfg"]["var_clip"],
             kld_weight=fx["cfg"]["kld_weight"], rl_params=[params[n] for n in fx["rl_names"]], vae_params=[params[n] for n in fx["vae_names"]], upstream=1.0)
    if rl_step is not None:
        x.update(obs=fx["obs"][rl_step], obs_history=fx["obs_history"][rl_step], critic_obs=fx["critic_obs"][rl_step], noise=fx["noise"][rl_step])
    if vae_step is not None:
        x.update(obs_history=fx["vae_history"][vae_step], labels=fx["vae_labels"][vae_step], next_states=fx["vae_next_states"][vae_step],
                 terminated=fx["vae_terminated"][vae_step], vae_noise=fx["vae_noise"][vae_step])
    return x

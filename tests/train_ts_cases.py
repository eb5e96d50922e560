"""The cases of the teacher-student learner passes (include/lgtraints.h), shared by tests/test_train_ts_host.py (CPU) and
tests/test_gpu_train_ts.py (GPU): one net table, one case table, the input generator, a numpy restatement of both passes built on
tests/train_cases.py's layers and batch sums (float64: the reference of every comparison; float32 with the plan's slices: the kernel's
order of sums), the same passes as torch autograd on the CPU, the plans restated, the parity rule and the loader of the golden fixture
(tests/golden/gen_ppo_ts_train_fixtures.py).  Nothing here loads the HIP library."""
import numpy as np
import torch

from tests import train_cases as tc
from tests.optim_cases import PARITY_FACTOR

# name -> (privilege encoder widths, actor widths, critic widths, history encoder widths); actor[0] = O + Z, both encoders end at Z.
# Hidden layers carry an ELU; the actor ends in a Hardtanh only where the case has a clip.
NETS = {
    "fixture":  ([5, 8, 4, 3], [10, 16, 8, 3], [9, 16, 8, 1], [14, 8, 4, 3]),
    "go2_ts":   ([94, 256, 128, 94], [139, 512, 256, 128, 12], [860, 1024, 256, 128, 1], [900, 256, 128, 94]),
    "one_four": ([6, 5], [12, 19, 16, 15, 4], [6, 17, 1], [9, 7, 5]),       # a privilege encoder of one layer beside an actor of four
    "wide":     ([8, 8], [2048, 2048, 3], [8, 5, 1], [2048, 2048, 8]),      # the 8-row tile in both passes
}
RAGGED = (1, 4, 5, 16, 17, 65)
for _o in RAGGED:              # the concatenation boundary O off and on a multiple of 4, Z = 1, the latent slice across 16-column tiles
    for _z in RAGGED:
        NETS[f"o{_o}_z{_z}"] = ([3, 6, _z], [_o + _z, 9, 3], [_o, 5, 1], [5, 7, _z])
SWEEP = [f"o{o}_z{z}" for o in RAGGED for z in RAGGED]
REAL = ("go2_ts",)

BATCHES = (1, 31, 33, 257)
CASES = {}
for _net in ("fixture", "one_four") + REAL:
    for _b in BATCHES:
        CASES[f"{_net}_b{_b}"] = dict(net=_net, B=_b, seed=900 + len(CASES))
for _net in SWEEP:
    CASES[f"{_net}_b33"] = dict(net=_net, B=33, seed=900 + len(CASES))
for _b in (1, 9):
    CASES[f"wide_b{_b}"] = dict(net="wide", B=_b, seed=900 + len(CASES))
CASES["fixture_noclip_b33"] = dict(net="fixture", B=33, seed=990, clip=None)          # ActorCriticTS as it stands: no Hardtanh
CASES["go2_ts_noclip_b31"] = dict(net="go2_ts", B=31, seed=991, clip=None)
# 257 loss tiles of 32 rows (the finalize kernel's second trip) and the cap of 32 slices with a short last one (31 x 260 + 133 rows)
CASES["fixture_b8193"] = dict(net="fixture", B=8193, seed=992)
RAGGED_SLICE_NETS = ("fixture", "one_four") + REAL        # plus, per net, the smallest B either plan slices raggedly

RED_BYTES = 256 * 8            # the encoder forward's float64 tree (LG_TRAIN_TS_THREADS doubles)
TARGET_JOBS = 2048             # LG_TRAIN_TS_TARGET_JOBS
CHAIN_NAMES = ("privilege_encoder", "actor", "critic", "history_encoder")          # LG_TRAIN_TS_* order


def slice_rule(n_rows, tiles):
    """tests/train_cases.slice_rule with include/lgtraints.h's job target."""
    want = min(max(1, n_rows // tc.MIN_SLICE_ROWS), max(1, TARGET_JOBS // tiles), tc.MAX_SLICES)
    per = (-(-n_rows // want) + 3) & ~3
    return -(-n_rows // per), per


# ---- the plans ------------------------------------------------------------------------------------------------------------------------------
def _lds(chains_first):
    w = [0, 0]
    for c, first in chains_first:
        for i, width in enumerate(c):
            w[(i + first) & 1] = max(w[(i + first) & 1], tc.lds_stride(width))
    return w


def _offsets(n_rows, chains, off):
    """h_off, g_off, then p_off / slices of the chains, as include/lgtrain.h lays them out; returns (dict, off, jobs)."""
    h_off, g_off, p_off, slices, rows, jobs = [], [], [], [], [], 0
    for c in chains:
        h, g = [], []
        for li in range(len(c) - 1):
            if li < len(c) - 2:
                h.append(off)
                off += n_rows * c[li + 1]
            else:
                h.append(-1)
            g.append(off)
            off += n_rows * c[li + 1]
        h_off.append(h)
        g_off.append(g)
    for c in chains:
        p, s, r = [], [], []
        for li in range(len(c) - 1):
            K, M = c[li], c[li + 1]
            tiles = -(-M // tc.WG_TILE) * -(-K // tc.WG_TILE)
            S, per = slice_rule(n_rows, tiles)
            p.append(off)
            off += S * (M * K + M)
            jobs += S * tiles
            s.append(S)
            r.append(per)
        p_off.append(p)
        slices.append(s)
        rows.append(r)
    return dict(h_off=h_off, g_off=g_off, p_off=p_off, slices=slices, slice_rows=rows), off, jobs


def restated_plan_ts(n_rows, priv, actor, critic):
    """include/lgtraints.h's plan of the RL pass; the per-chain lists hold the privilege encoder, the actor and the critic (chains 0-2)."""
    first = 0 if (len(priv) - 1) & 1 else 1
    w = _lds(((priv, first), (actor, 0), (critic, 0)))
    row_tile = next((r for r in (32, 16, 8) if r * (w[0] + w[1]) * 4 <= tc.LDS_BYTES), 0)
    d, off, jobs = _offsets(n_rows, (priv, actor, critic), n_rows * actor[0])
    std = slice_rule(n_rows, 1)
    d.update(row_tile=row_tile, lds_bytes=row_tile * (w[0] + w[1]) * 4, enc_first_buffer=first, cat_off=0, std=std, std_p_off=off,
             workspace_floats=off + std[0] * actor[-1], weight_jobs=jobs + std[0])
    return d


def restated_plan_enc(n_rows, hist, priv):
    """The encoder pass: the per-chain lists hold the history encoder alone (chain 3)."""
    w = _lds(((hist, 0), (priv, 0)))
    row_tile = next((r for r in (32, 16, 8) if r * (w[0] + w[1]) * 4 + RED_BYTES <= tc.LDS_BYTES), 0)
    d, off, jobs = _offsets(n_rows, (hist,), 0)
    gl_off = off
    off += n_rows * hist[-1]
    y_off = off
    off += n_rows * hist[-1]
    off += off & 1
    tiles = -(-n_rows // row_tile)
    d.update(row_tile=row_tile, lds_bytes=row_tile * (w[0] + w[1]) * 4 + RED_BYTES, gl_off=gl_off, y_off=y_off, partial_off=off, loss_tiles=tiles,
             workspace_floats=off + 2 * tiles, weight_jobs=jobs)
    return d


def smallest_ragged_b(net):
    """The smallest batch at which some layer of either pass gets more than one slice and a last slice shorter than the others."""
    priv, actor, critic, hist = NETS[net]
    for b in range(1, 4096):
        for p in (restated_plan_ts(b, priv, actor, critic), restated_plan_enc(b, hist, priv)):
            for S, per in [x for c in zip(p["slices"], p["slice_rows"]) for x in zip(*c)]:
                if S > 1 and b % per:
                    return b
    raise AssertionError(net)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def _chain_names(name, c):
    return [f"{name}.{i}.{k}" for i in range(len(c) - 1) for k in ("weight", "bias")]


def rl_names(actor, critic, priv):
    """PPO_TS.rl_parameters' order: actor, critic, privilege encoder, std."""
    return _chain_names("actor", actor) + _chain_names("critic", critic) + _chain_names("privilege_encoder", priv) + ["std"]


def enc_names(hist):
    return _chain_names("history_encoder", hist)


def _layers(rng, ch):
    out = []
    for li in range(len(ch) - 1):
        out.append((rng.normal(size=(ch[li + 1], ch[li])) * (1.3 / np.sqrt(ch[li]))).astype(np.float32))
        out.append((0.2 * rng.normal(size=ch[li + 1])).astype(np.float32))
    return out


def make_inputs(case):
    """float32 numpy inputs of a case: dict(priv, actor, critic, hist (widths), clip, rl_params (rl_names order), enc_params, obs,
    privileged_obs, critic_obs, obs_history, terminated, grad_mu, grad_sigma, grad_values, upstream).  The clip as
    tests/train_cases.make_inputs places it: a good share of the means saturates, no pre-clip mean within 1e-3 of it; a case with
    clip=None has no Hardtanh."""
    c = CASES[case] if isinstance(case, str) else case
    priv, actor, critic, hist = NETS[c["net"]]
    rng, B, f = np.random.default_rng(c["seed"]), c["B"], np.float32
    std = (0.5 + rng.random(actor[-1])).astype(f)
    x = dict(priv=priv, actor=actor, critic=critic, hist=hist, clip=None,
             rl_params=_layers(rng, actor) + _layers(rng, critic) + _layers(rng, priv) + [std], enc_params=_layers(rng, hist),
             obs=rng.normal(size=(B, actor[0] - priv[-1])).astype(f), privileged_obs=rng.normal(size=(B, priv[0])).astype(f),
             critic_obs=rng.normal(size=(B, critic[0])).astype(f), obs_history=rng.normal(size=(B, hist[0])).astype(f),
             terminated=(rng.random((B, 1)) > 0.3).astype(f),
             grad_mu=rng.normal(size=(B, actor[-1])).astype(f), grad_sigma=rng.normal(size=(B, actor[-1])).astype(f),
             grad_values=rng.normal(size=(B, critic[-1])).astype(f), upstream=f(0.75))
    if "clip" in c and c["clip"] is None:
        return x
    pre = rl_forward(x)["mu"]
    clip = float(f(np.median(np.abs(pre))))
    while np.abs(np.abs(pre) - clip).min() < 1e-3:
        clip = float(f(clip + 2.5e-3))
    x["clip"] = clip
    return x


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def _pairs(ps, dtype):
    return [(np.asarray(ps[i]).astype(dtype), np.asarray(ps[i + 1]).astype(dtype)) for i in range(0, len(ps), 2)]


def split_rl(x, dtype=np.float64):
    """(actor, critic, privilege encoder) as lists of (W, b), and std, from x["rl_params"]."""
    na, nc = 2 * (len(x["actor"]) - 1), 2 * (len(x["critic"]) - 1)
    p = x["rl_params"]
    return _pairs(p[:na], dtype), _pairs(p[na:na + nc], dtype), _pairs(p[na + nc:-1], dtype), np.asarray(p[-1]).astype(dtype)


def rl_forward(x, dtype=np.float64):
    """dict(mu, sigma, values, cat, acts=(privilege encoder, actor, critic activations)) of include/lgtraints.h's RL forward."""
    actor, critic, priv, std = split_rl(x, dtype)
    pa = tc._mlp(priv, np.asarray(x["privileged_obs"]).astype(dtype), dtype)
    cat = np.concatenate([np.asarray(x["obs"]).astype(dtype), pa[-1]], axis=1)
    aa = tc._mlp(actor, cat, dtype)
    ca = tc._mlp(critic, np.asarray(x["critic_obs"]).astype(dtype), dtype)
    mu = aa[-1]
    if x["clip"] is not None:
        mu = np.where(mu < -x["clip"], -x["clip"], np.where(mu > x["clip"], x["clip"], mu)).astype(dtype)
    return dict(mu=mu, sigma=mu * 0 + std, values=ca[-1], cat=cat, acts=(pa, aa, ca))


def chain_backward(layers, acts, G, dtype, pers=None, input_grad=False, drop_last=False):
    """The gradients [W0, b0, W1, b1, ...] of one chain from G of its last layer (elu' from the stored output), the batch sums per slice of
    pers[li] rows as the kernel forms them; with input_grad also G through layer 0, with no activation factor.  drop_last: every sum without
    its last slice (a planted defect)."""
    B, out = G.shape[0], []
    for li in range(len(layers) - 1, -1, -1):
        H, per = acts[li], B if pers is None else int(pers[li])
        out = [tc.slice_sum(per, G, H, drop_last=drop_last), tc.slice_sum(per, G, phases=4, drop_last=drop_last)] + out
        if li:
            G = ((G @ layers[li][0]) * np.where(H > 0, 1, H + 1)).astype(dtype)
    return out, ((G @ layers[0][0]).astype(dtype) if input_grad else None)


def rl_backward(x, dtype=np.float64, slices=None, wrong=None):
    """The gradients of the RL pass in rl_names order (actor, critic, privilege encoder, std).  The latent columns [O, O + Z) of actor layer
    0's input gradient are G of the privilege encoder's last layer.  `slices`: dict(std=rows, actor=[rows per layer], critic=[...],
    priv=[...]) as the plan slices each sum, or None.  Planted defects: wrong="latent_cols0" takes the latent gradient from columns [0, Z),
    wrong="priv_drop_last_slice" leaves the last slice out of the privilege encoder's sums (it needs `slices` with more than one)."""
    fw = rl_forward(x, dtype)
    actor, critic, priv, _ = split_rl(x, dtype)
    pa, aa, ca = fw["acts"]
    B, s = fw["mu"].shape[0], slices or {}
    g_mu = np.asarray(x["grad_mu"]).astype(dtype)
    if x["clip"] is not None:
        g_mu = np.where((fw["mu"] >= x["clip"]) | (fw["mu"] <= -x["clip"]), 0, g_mu).astype(dtype)
    ga, dcat = chain_backward(actor, aa, g_mu, dtype, s.get("actor"), input_grad=True)
    gc, _ = chain_backward(critic, ca, np.asarray(x["grad_values"]).astype(dtype), dtype, s.get("critic"))
    Z = pa[-1].shape[1]
    O = dcat.shape[1] - Z
    gz = dcat[:, :Z] if wrong == "latent_cols0" else dcat[:, O:]
    drop = wrong == "priv_drop_last_slice"
    if drop and not ("priv" in s and B > max(s["priv"])):
        raise ValueError("priv_drop_last_slice needs more than one slice in every sum of the privilege encoder")
    gp, _ = chain_backward(priv, pa, np.ascontiguousarray(gz), dtype, s.get("priv"), drop_last=drop)
    return ga + gc + gp + [tc.slice_sum(int(s.get("std", B)), np.asarray(x["grad_sigma"]).astype(dtype))]


def enc_pass(x, dtype=np.float64, upstream=None, slices=None, wrong=None, row_tile=None):
    """dict(loss, grads (enc_names order), pred, target, d, priv_grads) of the encoder pass: y = privilege_encoder(privileged_obs) as a
    constant, d = (p - y) t, loss = sum d^2 / (B Z), d loss / d p = 2 d t / (B Z), times `upstream` (default x["upstream"]).  priv_grads is
    None: the target carries no gradient.  `slices`: rows per slice per layer; row_tile: the loss as float64 partials per tile added in tile
    order.  Planted defects: wrong="target_grad" lets the gradient through the target (priv_grads is then what reaches the privilege
    encoder), wrong="select" applies the mask as a select."""
    hist = _pairs(x["enc_params"], dtype)
    priv = split_rl(x, dtype)[2]
    ha = tc._mlp(hist, np.asarray(x["obs_history"]).astype(dtype), dtype)
    pa = tc._mlp(priv, np.asarray(x["privileged_obs"]).astype(dtype), dtype)
    t = np.asarray(x["terminated"]).astype(dtype)
    with np.errstate(invalid="ignore"):
        d = np.where(t != 0, ha[-1] - pa[-1], 0).astype(dtype) if wrong == "select" else ((ha[-1] - pa[-1]) * t).astype(dtype)
    n, B = d.size, d.shape[0]
    up = dtype(x["upstream"] if upstream is None else upstream)
    if dtype == np.float32:
        G = ((d * t * dtype(2.0 / (dtype(B) * dtype(d.shape[1])))) * up).astype(dtype)
    else:
        G = (2 * d * t / n * up).astype(dtype)
    grads, _ = chain_backward(hist, ha, G, dtype, slices)
    priv_grads = chain_backward(priv, pa, -G, dtype)[0] if wrong == "target_grad" else None
    sq = d.astype(np.float64) ** 2
    if row_tile:
        loss = 0.0
        for r0 in range(0, B, row_tile):
            loss = loss + sq[r0:r0 + row_tile].sum()
        loss = loss / n
    else:
        loss = sq.sum() / n
    return dict(loss=dtype(loss) if dtype == np.float32 else loss, grads=grads, pred=ha[-1], target=pa[-1], d=d, priv_grads=priv_grads)


def kernel_order_slices(x):
    """The rows per slice of every batch sum as the restated plans give them: (rl_backward's `slices`, enc_pass's `slices`, the encoder
    pass's row tile)."""
    B = np.asarray(x["obs"]).shape[0]
    p, q = restated_plan_ts(B, x["priv"], x["actor"], x["critic"]), restated_plan_enc(B, x["hist"], x["priv"])
    return dict(std=p["std"][1], priv=p["slice_rows"][0], actor=p["slice_rows"][1], critic=p["slice_rows"][2]), q["slice_rows"][0], q["row_tile"]


def _mlp_t(h, ps):
    for i in range(0, len(ps), 2):
        h = torch.nn.functional.linear(h, ps[i], ps[i + 1])
        if i < len(ps) - 2:
            h = torch.nn.functional.elu(h)
    return h


def torch_passes(x, dtype=torch.float32):
    """Both passes as torch computes them on the CPU in `dtype`: dict(mu, sigma, values, rl_grads, enc_rl_grads (what the RL cotangents
    send into the history encoder: None each), loss, enc_grads, priv_enc_grads (what the encoder loss sends into the privilege encoder:
    None each, the target is formed under no_grad)), float64 numpy."""
    t = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)
    rl = [t(p).requires_grad_(True) for p in x["rl_params"]]
    enc = [t(p).requires_grad_(True) for p in x["enc_params"]]
    na, nc = 2 * (len(x["actor"]) - 1), 2 * (len(x["critic"]) - 1)
    priv = rl[na + nc:-1]
    mu = _mlp_t(torch.cat((t(x["obs"]), _mlp_t(t(x["privileged_obs"]), priv)), dim=-1), rl[:na])
    if x["clip"] is not None:
        mu = torch.nn.functional.hardtanh(mu, -x["clip"], x["clip"])
    sigma = mu * 0.0 + rl[-1]
    values = _mlp_t(t(x["critic_obs"]), rl[na:na + nc])
    n = lambda v: None if v is None else v.detach().double().numpy().copy()
    out = dict(mu=n(mu), sigma=n(sigma), values=n(values))
    if "grad_mu" in x:
        torch.autograd.backward([mu, sigma, values], [t(x["grad_mu"]), t(x["grad_sigma"]), t(x["grad_values"])])
        out.update(rl_grads=[n(p.grad) for p in rl], enc_rl_grads=[n(p.grad) for p in enc])
        for p in rl:
            p.grad = None
    term = t(x["terminated"])
    with torch.no_grad():
        target = _mlp_t(t(x["privileged_obs"]), priv)
    loss = torch.nn.functional.mse_loss(_mlp_t(t(x["obs_history"]), enc) * term, target * term)
    (loss * float(x.get("upstream", 1.0))).backward()
    out.update(loss=n(loss), enc_grads=[n(p.grad) for p in enc], priv_enc_grads=[n(p.grad) for p in priv])
    return out


# ---- the parity rule (tests/train_cases.py's, with the loss as an output) -------------------------------------------------------------------
CLASSES = ("outputs", "loss", "grad_weight", "grad_bias", "grad_std")


def tensor_class(name):
    return "outputs" if name in ("mu", "sigma", "values") else "loss" if name == "loss" else "grad_std" if name == "std" else \
        "grad_weight" if name.endswith("weight") else "grad_bias"


def check_parity(got, ref64, ref32, label, report=None, factor=PARITY_FACTOR):
    """Every tensor of ref64 against |kernel - f64| <= factor * max(|torch-CPU-f32 - f64|, ulp of the tensor's largest magnitude), factor =
    PARITY_FACTOR unless a test holds something to a share of the rule; prints the worst ratio of each class before it asserts."""
    worst, bad = {}, []
    for name, r64 in ref64.items():
        err, err32 = tc.max_err(got[name], r64), tc.max_err(ref32[name], r64)
        unit = tc.parity_bound(err32, r64) / PARITY_FACTOR
        bound = factor * unit
        ratio = err / unit if unit else (0.0 if err == 0.0 else float("inf"))
        k = tensor_class(name)
        worst[k] = max(worst.get(k, 0.0), ratio if np.isfinite(ratio) else float("inf"))
        if not (np.isfinite(err) and err <= bound):
            bad.append(f"{label} {name}: |kernel - f64| = {err:.3e} above {bound:.3e} (torch f32 {err32:.3e})")
    print(f"{label}: worst |kernel - f64| / max(|f32 - f64|, ulp): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" (allowed {factor:g})")
    if report is not None:
        report.append((label, worst))
    assert not bad, "\n".join(bad)
    return worst


def named(x, outs, rl_grads, loss, enc_grads):
    """dict name -> array of both passes' outputs and gradients."""
    d = dict(mu=outs["mu"], sigma=outs["sigma"], values=outs["values"], loss=np.asarray(loss, np.float64).reshape(1))
    d.update(zip(rl_names(x["actor"], x["critic"], x["priv"]), rl_grads))
    d.update(zip(enc_names(x["hist"]), enc_grads))
    return d


def references(x):
    """(float64 restatement, torch CPU float32) of a case, as `named` dicts."""
    fw, e, t32 = rl_forward(x), enc_pass(x), torch_passes(x)
    return named(x, fw, rl_backward(x), e["loss"], e["grads"]), named(x, t32, t32["rl_grads"], t32["loss"], t32["enc_grads"])


# ---- the module -----------------------------------------------------------------------------------------------------------------------------
class Module(torch.nn.Module):
    """ActorCriticTS's members as FusedTrainPassTS reads them, with rl_parameters() in the reference's order (actor, critic, privilege
    encoder, std), holding a case's parameters.  The actor ends in a Hardtanh where the case has a clip (ActorCriticTS itself has none)."""

    def __init__(self, x, device="cpu", dtype=torch.float32):
        super().__init__()
        nn = torch.nn

        def chain(widths, clip):
            mods = []
            for i in range(len(widths) - 1):
                mods.append(nn.Linear(widths[i], widths[i + 1]))
                if i < len(widths) - 2:
                    mods.append(nn.ELU())
            if clip is not None:
                mods.append(nn.Hardtanh(-clip, clip))
            return nn.Sequential(*mods)
        self.std = nn.Parameter(torch.zeros(x["actor"][-1]))
        self.privilege_encoder, self.history_encoder = chain(x["priv"], None), chain(x["hist"], None)
        self.actor, self.critic = chain(x["actor"], x["clip"]), chain(x["critic"], None)
        self.to(device=device, dtype=dtype)
        with torch.no_grad():
            for p, v in zip(self.rl_parameters() + self.encoder_parameters(), list(x["rl_params"]) + list(x["enc_params"])):
                p.copy_(torch.as_tensor(np.asarray(v)).to(dtype))

    def rl_parameters(self):
        return list(self.actor.parameters()) + list(self.critic.parameters()) + list(self.privilege_encoder.parameters()) + [self.std]

    def encoder_parameters(self):
        return list(self.history_encoder.parameters())

    def forward(self, obs, privileged_obs, critic_obs):
        mu = self.actor(torch.cat((obs, self.privilege_encoder(privileged_obs)), dim=-1))
        return mu, mu * 0.0 + self.std, self.critic(critic_obs)

    def encoder_loss(self, obs_history, privileged_obs, terminated):
        with torch.no_grad():
            target = self.privilege_encoder(privileged_obs)
        return torch.nn.functional.mse_loss(self.history_encoder(obs_history) * terminated, target * terminated)


# ---- the golden fixture ---------------------------------------------------------------------------------------------------------------------
FIXTURE_COLUMNS = ("obs", "privileged_obs", "critic_obs", "actions", "target_values", "advantages", "returns", "old_log_prob", "old_mu", "old_sigma")
ENC_COLUMNS = ("enc_history", "enc_privileged", "enc_terminated")
CFG_KEYS = ("lr0", "beta1", "beta2", "eps", "max_grad_norm", "desired_kl", "steps", "clip_param", "value_loss_coef", "entropy_coef", "encoder_lr",
            "enc_steps", "enc_epochs")


def load_fixture(path):
    """dict(names, rl_names, enc_names, shapes (by name), priv / actor / critic / hist widths, cfg, init, per RL step the columns, mu, sigma,
    values, loss, kl, lr, grad_norm, grads, params; per encoder step enc_history, enc_privileged, enc_terminated, enc_loss, enc_grads,
    enc_grad_norm, enc_params), float64; init / params / enc_params as dicts name -> array, grads / enc_grads as lists in rl_names /
    enc_names order."""
    z = np.load(path)
    names = [str(n) for n in z["names"]]
    shapes = {n: tuple(int(d) for d in s if d) for n, s in zip(names, z["shapes"])}

    def split(flat, order):
        out, at = [], 0
        for n in order:
            size = int(np.prod(shapes[n]))
            out.append(flat[at:at + size].reshape(shapes[n]).copy())
            at += size
        assert at == flat.size
        return out
    cfg = dict(zip(CFG_KEYS, (float(v) for v in z["cfg"])))
    for k in ("steps", "enc_steps", "enc_epochs"):
        cfg[k] = int(cfg[k])
    rl, enc = [str(n) for n in z["rl_names"]], [str(n) for n in z["enc_names"]]
    widths = lambda chain: [shapes[n][1] for n in names if n.startswith(chain) and n.endswith("weight")][:1] + \
        [shapes[n][0] for n in names if n.startswith(chain) and n.endswith("weight")]
    out = dict(names=names, rl_names=rl, enc_names=enc, shapes=shapes, cfg=cfg, priv=widths("privilege_encoder"), actor=widths("actor"),
               critic=widths("critic"), hist=widths("history_encoder"),
               init=dict(zip(names, split(z["init"], names))), params=[dict(zip(names, split(p, names))) for p in z["params"]],
               enc_params=[dict(zip(names, split(p, names))) for p in z["enc_params"]], grads=[split(g, rl) for g in z["grads"]],
               enc_grads=[split(g, enc) for g in z["enc_grads"]])
    for k in FIXTURE_COLUMNS + ENC_COLUMNS + ("mu", "sigma", "values", "loss", "kl", "lr", "grad_norm", "enc_loss", "enc_grad_norm"):
        out[k] = z[k]
    return out


def fixture_inputs(fx, params, rl_step=None, enc_step=None):
    """The inputs of one step of the fixture around `params` (name -> array), as make_inputs shapes them, float64.  No clip: the
    reference's ActorCriticTS has no Hardtanh."""
    x = dict(priv=fx["priv"], actor=fx["actor"], critic=fx["critic"], hist=fx["hist"], clip=None, rl_params=[params[n] for n in fx["rl_names"]],
             enc_params=[params[n] for n in fx["enc_names"]], upstream=1.0)
    if rl_step is not None:
        x.update(obs=fx["obs"][rl_step], privileged_obs=fx["privileged_obs"][rl_step], critic_obs=fx["critic_obs"][rl_step])
    if enc_step is not None:
        x.update(obs_history=fx["enc_history"][enc_step], privileged_obs=fx["enc_privileged"][enc_step], terminated=fx["enc_terminated"][enc_step])
    return x


def fixture_loss_inputs(fx, s, mu, sigma, values):
    """tests/ppo_loss_cases.restate's input for RL step s of the fixture around the given network outputs."""
    g = dict(mu=mu, sigma=sigma, actions=fx["actions"][s], advantages=fx["advantages"][s], old_log_prob=fx["old_log_prob"][s],
             old_mu=fx["old_mu"][s], old_sigma=fx["old_sigma"][s])
    return dict(groups=[g], values=values, returns=fx["returns"][s], target_values=fx["target_values"][s])

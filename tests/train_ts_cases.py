"""The cases of the teacher-student learner passes (include/lgtraints.h), shared by tests/test_train_ts_host.py (CPU) and
tests/test_gpu_train_ts.py (GPU): one net table, one case table, the input generator, a numpy restatement of both passes built on
tests/train_support.py's layers and batch sums (float64: the reference of every comparison; float32 with the plan's slices: the kernel's
order of sums), the same passes as torch autograd on the CPU, the plans restated and the loader of the golden fixture
(tests/golden/gen_ppo_ts_train_fixtures.py); the plan's rules, the parity rule and the fixture readers are tests/train_support.py's.
Nothing here loads the HIP library."""
import numpy as np
import torch

from tests import train_support as sup
from tests.train_support import CLASSES, chain_backward, check_parity, fixture_loss_inputs, tensor_class          # noqa: F401

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


# ---- the plans ------------------------------------------------------------------------------------------------------------------------------
def restated_plan_ts(n_rows, priv, actor, critic):
    """include/lgtraints.h's plan of the RL pass; the per-chain lists hold the privilege encoder, the actor and the critic (chains 0-2)."""
    first = 0 if (len(priv) - 1) & 1 else 1
    row_tile, lds_bytes = sup.row_tile(sup.lds_widths(((priv, first), (actor, 0), (critic, 0))))
    d, off, jobs = sup.offsets(n_rows, (priv, actor, critic), n_rows * actor[0], TARGET_JOBS)
    std = sup.slice_rule(n_rows, 1, TARGET_JOBS)
    d.update(row_tile=row_tile, lds_bytes=lds_bytes, enc_first_buffer=first, cat_off=0, std=std, std_p_off=off,
             workspace_floats=off + std[0] * actor[-1], weight_jobs=jobs + std[0])
    return d


def restated_plan_enc(n_rows, hist, priv):
    """The encoder pass: the per-chain lists hold the history encoder alone (chain 3)."""
    row_tile, lds_bytes = sup.row_tile(sup.lds_widths(((hist, 0), (priv, 0))), RED_BYTES)
    d, off, jobs = sup.offsets(n_rows, (hist,), 0, TARGET_JOBS)
    gl_off = off
    off += n_rows * hist[-1]
    y_off = off
    off += n_rows * hist[-1]
    off += off & 1
    tiles = -(-n_rows // row_tile)
    d.update(row_tile=row_tile, lds_bytes=lds_bytes, gl_off=gl_off, y_off=y_off, partial_off=off, loss_tiles=tiles, workspace_floats=off + 2 * tiles,
             weight_jobs=jobs)
    return d


def smallest_ragged_b(net):
    """The smallest batch at which some layer of either pass gets more than one slice and a last slice shorter than the others."""
    priv, actor, critic, hist = NETS[net]
    return sup.smallest_ragged_b(lambda b: restated_plan_ts(b, priv, actor, critic), lambda b: restated_plan_enc(b, hist, priv))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def _chain_names(name, c):
    return [f"{name}.{i}.{k}" for i in range(len(c) - 1) for k in ("weight", "bias")]


def rl_names(actor, critic, priv):
    """PPO_TS.rl_parameters' order: actor, critic, privilege encoder, std."""
    return _chain_names("actor", actor) + _chain_names("critic", critic) + _chain_names("privilege_encoder", priv) + ["std"]


def enc_names(hist):
    return _chain_names("history_encoder", hist)


def make_inputs(case):
    """float32 numpy inputs of a case (a name of CASES, or a dict of B, seed and either `net` or `widths` = (priv, actor, critic, hist)):
    dict(priv, actor, critic, hist (widths), clip, rl_params (rl_names order), enc_params, obs, privileged_obs, critic_obs, obs_history,
    terminated, grad_mu, grad_sigma, grad_values, upstream).  The clip as tests/train_support.place_clip places it; a case with clip=None
    has no Hardtanh."""
    c, (priv, actor, critic, hist) = sup.case_of(case, CASES, NETS)
    rng, B, f = np.random.default_rng(c["seed"]), c["B"], np.float32
    std = (0.5 + rng.random(actor[-1])).astype(f)
    x = dict(priv=priv, actor=actor, critic=critic, hist=hist, clip=None,
             rl_params=sup.draw_layers(rng, actor) + sup.draw_layers(rng, critic) + sup.draw_layers(rng, priv) + [std],
             enc_params=sup.draw_layers(rng, hist),
             obs=rng.normal(size=(B, actor[0] - priv[-1])).astype(f), privileged_obs=rng.normal(size=(B, priv[0])).astype(f),
             critic_obs=rng.normal(size=(B, critic[0])).astype(f), obs_history=rng.normal(size=(B, hist[0])).astype(f),
             terminated=(rng.random((B, 1)) > 0.3).astype(f),
             grad_mu=rng.normal(size=(B, actor[-1])).astype(f), grad_sigma=rng.normal(size=(B, actor[-1])).astype(f),
             grad_values=rng.normal(size=(B, critic[-1])).astype(f), upstream=f(0.75))
    if "clip" in c and c["clip"] is None:
        return x
    x["clip"] = sup.place_clip(rl_forward(x)["mu"])
    return x


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def split_rl(x, dtype=np.float64):
    """(actor, critic, privilege encoder) as lists of (W, b), and std, from x["rl_params"]."""
    na, nc = 2 * (len(x["actor"]) - 1), 2 * (len(x["critic"]) - 1)
    p = x["rl_params"]
    return sup.pairs(p[:na], dtype), sup.pairs(p[na:na + nc], dtype), sup.pairs(p[na + nc:-1], dtype), np.asarray(p[-1]).astype(dtype)


def rl_forward(x, dtype=np.float64):
    """dict(mu, sigma, values, cat, acts=(privilege encoder, actor, critic activations)) of include/lgtraints.h's RL forward."""
    actor, critic, priv, std = split_rl(x, dtype)
    pa = sup.mlp(priv, np.asarray(x["privileged_obs"]).astype(dtype), dtype)
    cat = np.concatenate([np.asarray(x["obs"]).astype(dtype), pa[-1]], axis=1)
    aa = sup.mlp(actor, cat, dtype)
    ca = sup.mlp(critic, np.asarray(x["critic_obs"]).astype(dtype), dtype)
    mu = sup.hardtanh(aa[-1], x["clip"], dtype)
    return dict(mu=mu, sigma=mu * 0 + std, values=ca[-1], cat=cat, acts=(pa, aa, ca))


def rl_backward(x, dtype=np.float64, slices=None, wrong=None):
    """The gradients of the RL pass in rl_names order (actor, critic, privilege encoder, std).  The latent columns [O, O + Z) of actor layer
    0's input gradient are G of the privilege encoder's last layer.  `slices`: dict(std=rows, actor=[rows per layer], critic=[...],
    priv=[...]) as the plan slices each sum, or None.  Planted defects: wrong="latent_cols0" takes the latent gradient from columns [0, Z),
    wrong="priv_drop_last_slice" leaves the last slice out of the privilege encoder's sums (it needs `slices` with more than one)."""
    fw = rl_forward(x, dtype)
    actor, critic, priv, _ = split_rl(x, dtype)
    pa, aa, ca = fw["acts"]
    B, s = fw["mu"].shape[0], slices or {}
    g_mu = sup.masked_grad_mu(x["grad_mu"], fw["mu"], x["clip"], dtype)
    ga, dcat = chain_backward(actor, aa, g_mu, dtype, s.get("actor"), input_grad=True)
    gc, _ = chain_backward(critic, ca, np.asarray(x["grad_values"]).astype(dtype), dtype, s.get("critic"))
    Z = pa[-1].shape[1]
    O = dcat.shape[1] - Z
    gz = dcat[:, :Z] if wrong == "latent_cols0" else dcat[:, O:]
    drop = wrong == "priv_drop_last_slice"
    if drop and not ("priv" in s and B > max(s["priv"])):
        raise ValueError("priv_drop_last_slice needs more than one slice in every sum of the privilege encoder")
    gp, _ = chain_backward(priv, pa, np.ascontiguousarray(gz), dtype, s.get("priv"), drop_last=drop)
    return ga + gc + gp + [sup.slice_sum(int(s.get("std", B)), np.asarray(x["grad_sigma"]).astype(dtype))]


def enc_pass(x, dtype=np.float64, upstream=None, slices=None, wrong=None, row_tile=None):
    """dict(loss, grads (enc_names order), pred, target, d, priv_grads) of the encoder pass: y = privilege_encoder(privileged_obs) as a
    constant, d = (p - y) t, loss = sum d^2 / (B Z), d loss / d p = 2 d t / (B Z), times `upstream` (default x["upstream"]).  priv_grads is
    None: the target carries no gradient.  `slices`: rows per slice per layer; row_tile: the loss as float64 partials per tile added in tile
    order.  Planted defects: wrong="target_grad" lets the gradient through the target (priv_grads is then what reaches the privilege
    encoder), wrong="select" applies the mask as a select."""
    hist = sup.pairs(x["enc_params"], dtype)
    priv = split_rl(x, dtype)[2]
    ha = sup.mlp(hist, np.asarray(x["obs_history"]).astype(dtype), dtype)
    pa = sup.mlp(priv, np.asarray(x["privileged_obs"]).astype(dtype), dtype)
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


def torch_passes(x, dtype=torch.float32):
    """Both passes as torch computes them on the CPU in `dtype`: dict(mu, sigma, values, rl_grads, enc_rl_grads (what the RL cotangents
    send into the history encoder: None each), loss, enc_grads, priv_enc_grads (what the encoder loss sends into the privilege encoder:
    None each, the target is formed under no_grad)), float64 numpy."""
    t = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)
    rl = [t(p).requires_grad_(True) for p in x["rl_params"]]
    enc = [t(p).requires_grad_(True) for p in x["enc_params"]]
    na, nc = 2 * (len(x["actor"]) - 1), 2 * (len(x["critic"]) - 1)
    priv = rl[na + nc:-1]
    mu = sup.mlp_t(torch.cat((t(x["obs"]), sup.mlp_t(t(x["privileged_obs"]), priv)), dim=-1), rl[:na])
    if x["clip"] is not None:
        mu = torch.nn.functional.hardtanh(mu, -x["clip"], x["clip"])
    sigma = mu * 0.0 + rl[-1]
    values = sup.mlp_t(t(x["critic_obs"]), rl[na:na + nc])
    n = lambda v: None if v is None else v.detach().double().numpy().copy()
    out = dict(mu=n(mu), sigma=n(sigma), values=n(values))
    if "grad_mu" in x:
        torch.autograd.backward([mu, sigma, values], [t(x["grad_mu"]), t(x["grad_sigma"]), t(x["grad_values"])])
        out.update(rl_grads=[n(p.grad) for p in rl], enc_rl_grads=[n(p.grad) for p in enc])
        for p in rl:
            p.grad = None
    term = t(x["terminated"])
    with torch.no_grad():
        target = sup.mlp_t(t(x["privileged_obs"]), priv)
    loss = torch.nn.functional.mse_loss(sup.mlp_t(t(x["obs_history"]), enc) * term, target * term)
    (loss * float(x.get("upstream", 1.0))).backward()
    out.update(loss=n(loss), enc_grads=[n(p.grad) for p in enc], priv_enc_grads=[n(p.grad) for p in priv])
    return out


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
        self.std = torch.nn.Parameter(torch.zeros(x["actor"][-1]))
        self.privilege_encoder, self.history_encoder = sup.sequential(x["priv"], None), sup.sequential(x["hist"], None)
        self.actor, self.critic = sup.sequential(x["actor"], x["clip"]), sup.sequential(x["critic"], None)
        self.to(device=device, dtype=dtype)
        sup.set_parameters(self.rl_parameters() + self.encoder_parameters(), list(x["rl_params"]) + list(x["enc_params"]), dtype)

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
    """tests/train_support.load_two_pass_fixture's dict with priv / actor / critic / hist widths: per RL step the columns, mu, sigma, values,
    loss, kl, lr, grad_norm, grads, params; per encoder step enc_history, enc_privileged, enc_terminated, enc_loss, enc_grads,
    enc_grad_norm, enc_params."""
    chains = dict(priv="privilege_encoder", actor="actor", critic="critic", hist="history_encoder")
    return sup.load_two_pass_fixture(path, CFG_KEYS, chains, "enc", FIXTURE_COLUMNS + ENC_COLUMNS + (
        "mu", "sigma", "values", "loss", "kl", "lr", "grad_norm", "enc_loss", "enc_grad_norm"))


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

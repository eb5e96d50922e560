"""The cases of the explicit-estimator learner passes (include/lgtrainee.h), shared by tests/test_train_ee_host.py (CPU) and
tests/test_gpu_train_ee.py (GPU): one net table, one case table, the input generator, a numpy float64 restatement of both passes built on
tests/train_cases.py's forward / backward, the same passes as torch autograd on the CPU, the plans restated, the parity rule and the
loader of the golden fixture (tests/golden/gen_ppo_ee_train_fixtures.py).  Nothing here loads the HIP library."""
import numpy as np
import torch

from tests import train_cases as tc
from tests.optim_cases import PARITY_FACTOR

# name -> (estimator widths, actor widths, critic widths); actor[0] = F + NL.  Hidden layers carry an ELU, the actor ends in a Hardtanh.
NETS = {
    "fixture":     ([7, 8, 4, 3], [10, 16, 8, 3], [9, 16, 8, 1]),
    "go2_ee":      ([900, 256, 128, 24], [924, 512, 256, 128, 12], [870, 1024, 256, 128, 1]),
    "tron1_pf_ee": ([310, 256, 128, 17], [327, 512, 256, 128, 6], [1340, 1024, 256, 128, 1]),
    "one_four":    ([7, 5], [12, 19, 16, 15, 4], [6, 17, 1]),          # an estimator of one layer beside an actor of four
}
RAGGED = (1, 4, 5, 16, 17, 65)
for _f in RAGGED:              # the concatenation boundary F off and on a multiple of 4, NL = 1, F + NL across 64
    for _n in RAGGED:
        NETS[f"f{_f}_n{_n}"] = ([_f, 6, _n], [_f + _n, 9, 3], [_f, 5, 1])
SWEEP = [f"f{f}_n{n}" for f in RAGGED for n in RAGGED]
REAL = ("go2_ee", "tron1_pf_ee")

BATCHES = (1, 31, 33, 257)
CASES = {}
for _net in ("fixture", "one_four") + REAL:
    for _b in BATCHES:
        CASES[f"{_net}_b{_b}"] = dict(net=_net, B=_b, seed=500 + len(CASES))
for _net in SWEEP:
    CASES[f"{_net}_b33"] = dict(net=_net, B=33, seed=500 + len(CASES))
RAGGED_SLICE_NETS = ("fixture", "one_four") + REAL        # plus, per net, the smallest B either plan slices raggedly
assert max(c["B"] for c in CASES.values()) <= 257

RED_BYTES = 256 * 8            # the estimator forward's float64 tree (LG_TRAIN_EE_THREADS doubles)
TARGET_JOBS = 2048             # LG_TRAIN_EE_TARGET_JOBS


def slice_rule(n_rows, tiles):
    """tests/train_cases.slice_rule with include/lgtrainee.h's job target."""
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


def restated_plan_ee(n_rows, est, actor, critic):
    """include/lgtrainee.h's plan of the RL pass; the per-chain lists hold the actor and the critic (chains 1 and 2)."""
    first = 0 if (len(est) - 1) & 1 else 1
    w = _lds(((est, first), (actor, 0), (critic, 0)))
    row_tile = next((r for r in (32, 16, 8) if r * (w[0] + w[1]) * 4 <= tc.LDS_BYTES), 0)
    d, off, jobs = _offsets(n_rows, (actor, critic), n_rows * actor[0])
    std = slice_rule(n_rows, 1)
    d.update(row_tile=row_tile, lds_bytes=row_tile * (w[0] + w[1]) * 4, est_first_buffer=first, cat_off=0, std=std, std_p_off=off,
             workspace_floats=off + std[0] * actor[-1], weight_jobs=jobs + std[0])
    return d


def restated_plan_est(n_rows, est):
    w = _lds(((est, 0),))
    row_tile = next((r for r in (32, 16, 8) if r * (w[0] + w[1]) * 4 + RED_BYTES <= tc.LDS_BYTES), 0)
    d, off, jobs = _offsets(n_rows, (est,), 0)
    gl_off = off
    off += n_rows * est[-1]
    off += off & 1
    tiles = -(-n_rows // row_tile)
    d.update(row_tile=row_tile, lds_bytes=row_tile * (w[0] + w[1]) * 4 + RED_BYTES, gl_off=gl_off, partial_off=off, loss_tiles=tiles,
             workspace_floats=off + 2 * tiles, weight_jobs=jobs)
    return d


def smallest_ragged_b(net):
    """The smallest batch at which some layer of either pass gets more than one slice and a last slice shorter than the others."""
    est, actor, critic = NETS[net]
    for b in range(1, 4096):
        for p in (restated_plan_ee(b, est, actor, critic), restated_plan_est(b, est)):
            for S, per in [x for c in zip(p["slices"], p["slice_rows"]) for x in zip(*c)]:
                if S > 1 and b % per:
                    return b
    raise AssertionError(net)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def rl_names(actor, critic):
    return [f"{n}.{i}.{k}" for n, c in (("actor", actor), ("critic", critic)) for i in range(len(c) - 1) for k in ("weight", "bias")] + ["std"]


def est_names(est):
    return [f"estimator.{i}.{k}" for i in range(len(est) - 1) for k in ("weight", "bias")]


def _layers(rng, ch):
    out = []
    for li in range(len(ch) - 1):
        out.append((rng.normal(size=(ch[li + 1], ch[li])) * (1.3 / np.sqrt(ch[li]))).astype(np.float32))
        out.append((0.2 * rng.normal(size=ch[li + 1])).astype(np.float32))
    return out


def make_inputs(case):
    """float32 numpy inputs of a case: dict(est, actor, critic (widths), clip, rl_params (rl_names order: actor, critic, std), est_params,
    features, critic_obs, labels, terminated, grad_mu, grad_sigma, grad_values, upstream).  The clip as tests/train_cases.make_inputs
    places it: a good share of the means saturates, no pre-clip mean within 1e-3 of it."""
    c = CASES[case] if isinstance(case, str) else case
    est, actor, critic = NETS[c["net"]]
    rng, B, f = np.random.default_rng(c["seed"]), c["B"], np.float32
    std = (0.5 + rng.random(actor[-1])).astype(f)
    x = dict(est=est, actor=actor, critic=critic, clip=None, rl_params=_layers(rng, actor) + _layers(rng, critic) + [std], est_params=_layers(rng, est),
             features=rng.normal(size=(B, est[0])).astype(f), critic_obs=rng.normal(size=(B, critic[0])).astype(f),
             labels=rng.normal(size=(B, est[-1])).astype(f), terminated=(rng.random((B, 1)) > 0.3).astype(f),
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


def _plain(x, dtype):
    """The RL pass as a plain actor-critic pass of tests/train_cases.py on obs = [features | estimator(features)]."""
    feats = np.asarray(x["features"]).astype(dtype)
    est = tc._mlp(_pairs(x["est_params"], dtype), feats, dtype)[-1]
    y = dict(actor=x["actor"], critic=x["critic"], clip=x["clip"], params=[x["rl_params"][-1]] + list(x["rl_params"][:-1]),
             obs=np.concatenate([feats, est], axis=1), critic_obs=x["critic_obs"])
    for k in ("grad_mu", "grad_sigma", "grad_values"):
        if k in x:
            y[k] = x[k]
    return y


def rl_forward(x, dtype=np.float64):
    """dict(mu, sigma, values, cat) of include/lgtrainee.h's RL forward in numpy `dtype`."""
    y = _plain(x, dtype)
    fw = tc.forward(y, dtype)
    return dict(mu=fw["mu"], sigma=fw["sigma"], values=fw["values"], cat=y["obs"])


def rl_backward(x, dtype=np.float64, slices=None):
    """The gradients of the RL pass in rl_names order; the estimator gets none (the concatenation is a constant of this pass)."""
    g = tc.backward(_plain(x, dtype), dtype, slices=slices)
    return g[1:] + g[:1]


def est_pass(x, dtype=np.float64, upstream=None, slices=None):
    """dict(loss, grads (est_names order), pred, d) of the estimator pass: d = (p - y) t, loss = sum d^2 / (B NL), d loss / d p =
    2 d t / (B NL), times `upstream` (default x["upstream"]).  `slices` (rows per slice, one number or one per layer): the batch sums are
    formed per slice and added in slice order, as the kernel does."""
    layers = _pairs(x["est_params"], dtype)
    acts = tc._mlp(layers, np.asarray(x["features"]).astype(dtype), dtype)
    t, y = np.asarray(x["terminated"]).astype(dtype), np.asarray(x["labels"]).astype(dtype)
    d = (acts[-1] - y) * t
    n, B = d.size, d.shape[0]
    up = dtype(x["upstream"] if upstream is None else upstream)
    G = (2 * d * t / n * up).astype(dtype)
    grads = []
    for li in range(len(layers) - 1, -1, -1):
        H = acts[li]
        per = B if slices is None else int(slices) if isinstance(slices, (int, np.integer)) else int(slices[li])
        grads = [tc.slice_sum(per, G, H), tc.slice_sum(per, G, phases=4)] + grads
        if li:
            G = ((G @ layers[li][0]) * np.where(H > 0, 1, H + 1)).astype(dtype)
    return dict(loss=(d * d).sum() / n, grads=grads, pred=acts[-1], d=d)


def _mlp_t(h, ps):
    for i in range(0, len(ps), 2):
        h = torch.nn.functional.linear(h, ps[i], ps[i + 1])
        if i < len(ps) - 2:
            h = torch.nn.functional.elu(h)
    return h


def torch_passes(x, dtype=torch.float32):
    """Both passes as torch computes them on the CPU in `dtype`: dict(mu, sigma, values, rl_grads, est_rl_grads (what autograd sends into
    the estimator from the RL cotangents: the gradient the reference discards), loss, est_grads), float64 numpy."""
    t = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)
    rl = [t(p).requires_grad_(True) for p in x["rl_params"]]
    est = [t(p).requires_grad_(True) for p in x["est_params"]]
    na = 2 * (len(x["actor"]) - 1)
    feats = t(x["features"])
    mu = _mlp_t(torch.cat((feats, _mlp_t(feats, est)), dim=-1), rl[:na])
    if x["clip"] is not None:
        mu = torch.nn.functional.hardtanh(mu, -x["clip"], x["clip"])
    sigma = mu * 0.0 + rl[-1]
    values = _mlp_t(t(x["critic_obs"]), rl[na:-1])
    n = lambda v: v.detach().double().numpy().copy()
    out = dict(mu=n(mu), sigma=n(sigma), values=n(values))
    if "grad_mu" in x:
        torch.autograd.backward([mu, sigma, values], [t(x["grad_mu"]), t(x["grad_sigma"]), t(x["grad_values"])])
        out.update(rl_grads=[n(p.grad) for p in rl], est_rl_grads=[n(p.grad) for p in est])
        for p in est:
            p.grad = None
    term = t(x["terminated"])
    loss = torch.nn.functional.mse_loss(_mlp_t(feats, est) * term, t(x["labels"]) * term)
    (loss * float(x.get("upstream", 1.0))).backward()
    out.update(loss=n(loss), est_grads=[n(p.grad) for p in est])
    return out


# ---- the parity rule (tests/train_cases.py's, with the loss as an output) -------------------------------------------------------------------
CLASSES = ("outputs", "loss", "grad_weight", "grad_bias", "grad_std")


def tensor_class(name):
    return "outputs" if name in ("mu", "sigma", "values") else "loss" if name == "loss" else "grad_std" if name == "std" else \
        "grad_weight" if name.endswith("weight") else "grad_bias"


def check_parity(got, ref64, ref32, label, report=None):
    """Every tensor of ref64 against |kernel - f64| <= PARITY_FACTOR * max(|torch-CPU-f32 - f64|, ulp of the tensor's largest magnitude);
    prints the worst ratio of each class before it asserts."""
    worst, bad = {}, []
    for name, r64 in ref64.items():
        err, err32 = tc.max_err(got[name], r64), tc.max_err(ref32[name], r64)
        bound = tc.parity_bound(err32, r64)
        ratio = err / (bound / PARITY_FACTOR) if bound else (0.0 if err == 0.0 else float("inf"))
        k = tensor_class(name)
        worst[k] = max(worst.get(k, 0.0), ratio if np.isfinite(ratio) else float("inf"))
        if not (np.isfinite(err) and err <= bound):
            bad.append(f"{label} {name}: |kernel - f64| = {err:.3e} above {bound:.3e} (torch f32 {err32:.3e})")
    print(f"{label}: worst |kernel - f64| / max(|f32 - f64|, ulp): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" (allowed {PARITY_FACTOR:g})")
    if report is not None:
        report.append((label, worst))
    assert not bad, "\n".join(bad)
    return worst


def named(x, outs, rl_grads, loss, est_grads):
    """dict name -> array of both passes' outputs and gradients."""
    d = dict(mu=outs["mu"], sigma=outs["sigma"], values=outs["values"], loss=np.asarray(loss).reshape(1))
    d.update(zip(rl_names(x["actor"], x["critic"]), rl_grads))
    d.update(zip(est_names(x["est"]), est_grads))
    return d


def references(x):
    """(float64 restatement, torch CPU float32) of a case, as `named` dicts."""
    fw, e, t32 = rl_forward(x), est_pass(x), torch_passes(x)
    return named(x, fw, rl_backward(x), e["loss"], e["grads"]), named(x, t32, t32["rl_grads"], t32["loss"], t32["est_grads"])


# ---- the module -----------------------------------------------------------------------------------------------------------------------------
class Module(torch.nn.Module):
    """ActorCriticEE's members as FusedTrainPassEE reads them, with rl_parameters() in the reference's order (actor, critic, std),
    holding a case's parameters."""

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
        self.actor, self.critic, self.estimator = chain(x["actor"], x["clip"]), chain(x["critic"], None), chain(x["est"], None)
        self.std = nn.Parameter(torch.zeros(x["actor"][-1]))
        self.to(device=device, dtype=dtype)
        with torch.no_grad():
            for p, v in zip(self.rl_parameters() + self.estimator_parameters(), list(x["rl_params"]) + list(x["est_params"])):
                p.copy_(torch.as_tensor(np.asarray(v)).to(dtype))

    def rl_parameters(self):
        return list(self.actor.parameters()) + list(self.critic.parameters()) + [self.std]

    def estimator_parameters(self):
        return list(self.estimator.parameters())

    def forward(self, features, critic_obs):
        mu = self.actor(torch.cat((features, self.estimator(features)), dim=-1))
        return mu, mu * 0.0 + self.std, self.critic(critic_obs)

    def estimator_loss(self, features, labels, terminated):
        return torch.nn.functional.mse_loss(self.estimator(features) * terminated, labels * terminated)


# ---- the golden fixture ---------------------------------------------------------------------------------------------------------------------
FIXTURE_COLUMNS = ("critic_obs", "features", "actions", "target_values", "advantages", "returns", "old_log_prob", "old_mu", "old_sigma")
CFG_KEYS = ("lr0", "beta1", "beta2", "eps", "max_grad_norm", "desired_kl", "steps", "clip_param", "value_loss_coef", "entropy_coef", "clip_actions",
            "estimator_lr", "est_steps", "est_epochs")


def load_fixture(path):
    """dict(names, rl_names, est_names, shapes (by name), est / actor / critic widths, cfg, init, per RL step the columns, mu, sigma, values,
    loss, kl, lr, grad_norm, grads, params; per estimator step est_features, est_labels, est_terminated, est_loss, est_grads, est_grad_norm,
    est_params), float64; init / params / est_params as dicts name -> array, grads / est_grads as lists in rl_names / est_names order."""
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
    for k in ("steps", "est_steps", "est_epochs"):
        cfg[k] = int(cfg[k])
    rl, est = [str(n) for n in z["rl_names"]], [str(n) for n in z["est_names"]]
    widths = lambda chain: [shapes[n][1] for n in names if n.startswith(chain) and n.endswith("weight")][:1] + \
        [shapes[n][0] for n in names if n.startswith(chain) and n.endswith("weight")]
    out = dict(names=names, rl_names=rl, est_names=est, shapes=shapes, cfg=cfg, est=widths("estimator"), actor=widths("actor"), critic=widths("critic"),
               init=dict(zip(names, split(z["init"], names))), params=[dict(zip(names, split(p, names))) for p in z["params"]],
               est_params=[dict(zip(names, split(p, names))) for p in z["est_params"]], grads=[split(g, rl) for g in z["grads"]],
               est_grads=[split(g, est) for g in z["est_grads"]])
    for k in FIXTURE_COLUMNS + ("mu", "sigma", "values", "loss", "kl", "lr", "grad_norm", "est_features", "est_labels", "est_terminated", "est_loss",
                                "est_grad_norm"):
        out[k] = z[k]
    return out


def fixture_inputs(fx, params, rl_step=None, est_step=None):
    """The inputs of one step of the fixture around `params` (name -> array), as make_inputs shapes them, float64."""
    x = dict(est=fx["est"], actor=fx["actor"], critic=fx["critic"], clip=fx["cfg"]["clip_actions"], rl_params=[params[n] for n in fx["rl_names"]],
             est_params=[params[n] for n in fx["est_names"]], upstream=1.0)
    if rl_step is not None:
        x.update(features=fx["features"][rl_step], critic_obs=fx["critic_obs"][rl_step])
    if est_step is not None:
        x.update(features=fx["est_features"][est_step], labels=fx["est_labels"][est_step], terminated=fx["est_terminated"][est_step])
    return x


def fixture_loss_inputs(fx, s, mu, sigma, values):
    """tests/ppo_loss_cases.restate's input for RL step s of the fixture around the given network outputs."""
    g = dict(mu=mu, sigma=sigma, actions=fx["actions"][s], advantages=fx["advantages"][s], old_log_prob=fx["old_log_prob"][s],
             old_mu=fx["old_mu"][s], old_sigma=fx["old_sigma"][s])
    return dict(groups=[g], values=values, returns=fx["returns"][s], target_values=fx["target_values"][s])

"""The cases of the explicit-estimator learner passes (include/lgtrainee.h), shared by tests/test_train_ee_host.py (CPU) and
tests/test_gpu_train_ee.py (GPU): one net table, one case table, the input generator, a numpy float64 restatement of both passes built on
tests/train_cases.py's forward / backward, the same passes as torch autograd on the CPU, the plans restated and the loader of the golden
fixture (tests/golden/gen_ppo_ee_train_fixtures.py); the chain arithmetic, the plan's rules, the parity rule and the fixture readers are
tests/train_support.py's.  Nothing here loads the HIP library."""
import numpy as np
import torch

from tests import train_cases as tc
from tests import train_support as sup
from tests.train_support import CLASSES, check_parity, fixture_loss_inputs, tensor_class          # noqa: F401

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


# ---- the plans ------------------------------------------------------------------------------------------------------------------------------
def restated_plan_ee(n_rows, est, actor, critic):
    """include/lgtrainee.h's plan of the RL pass; the per-chain lists hold the actor and the critic (chains 1 and 2)."""
    first = 0 if (len(est) - 1) & 1 else 1
    row_tile, lds_bytes = sup.row_tile(sup.lds_widths(((est, first), (actor, 0), (critic, 0))))
    d, off, jobs = sup.offsets(n_rows, (actor, critic), n_rows * actor[0], TARGET_JOBS)
    std = sup.slice_rule(n_rows, 1, TARGET_JOBS)
    d.update(row_tile=row_tile, lds_bytes=lds_bytes, est_first_buffer=first, cat_off=0, std=std, std_p_off=off,
             workspace_floats=off + std[0] * actor[-1], weight_jobs=jobs + std[0])
    return d


def restated_plan_est(n_rows, est):
    row_tile, lds_bytes = sup.row_tile(sup.lds_widths(((est, 0),)), RED_BYTES)
    d, off, jobs = sup.offsets(n_rows, (est,), 0, TARGET_JOBS)
    gl_off = off
    off += n_rows * est[-1]
    off += off & 1
    tiles = -(-n_rows // row_tile)
    d.update(row_tile=row_tile, lds_bytes=lds_bytes, gl_off=gl_off, partial_off=off, loss_tiles=tiles, workspace_floats=off + 2 * tiles,
             weight_jobs=jobs)
    return d


def smallest_ragged_b(net):
    """The smallest batch at which some layer of either pass gets more than one slice and a last slice shorter than the others."""
    est, actor, critic = NETS[net]
    return sup.smallest_ragged_b(lambda b: restated_plan_ee(b, est, actor, critic), lambda b: restated_plan_est(b, est))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def rl_names(actor, critic):
    return [f"{n}.{i}.{k}" for n, c in (("actor", actor), ("critic", critic)) for i in range(len(c) - 1) for k in ("weight", "bias")] + ["std"]


def est_names(est):
    return [f"estimator.{i}.{k}" for i in range(len(est) - 1) for k in ("weight", "bias")]


def make_inputs(case):
    """float32 numpy inputs of a case (a name of CASES, or a dict of B, seed and either `net` or `widths` = (est, actor, critic)): dict(est,
    actor, critic (widths), clip, rl_params (rl_names order: actor, critic, std), est_params, features, critic_obs, labels, terminated,
    grad_mu, grad_sigma, grad_values, upstream).  The clip as tests/train_support.place_clip places it."""
    c, (est, actor, critic) = sup.case_of(case, CASES, NETS)
    rng, B, f = np.random.default_rng(c["seed"]), c["B"], np.float32
    std = (0.5 + rng.random(actor[-1])).astype(f)
    x = dict(est=est, actor=actor, critic=critic, clip=None, rl_params=sup.draw_layers(rng, actor) + sup.draw_layers(rng, critic) + [std],
             est_params=sup.draw_layers(rng, est),
             features=rng.normal(size=(B, est[0])).astype(f), critic_obs=rng.normal(size=(B, critic[0])).astype(f),
             labels=rng.normal(size=(B, est[-1])).astype(f), terminated=(rng.random((B, 1)) > 0.3).astype(f),
             grad_mu=rng.normal(size=(B, actor[-1])).astype(f), grad_sigma=rng.normal(size=(B, actor[-1])).astype(f),
             grad_values=rng.normal(size=(B, critic[-1])).astype(f), upstream=f(0.75))
    if "clip" in c and c["clip"] is None:
        return x
    x["clip"] = sup.place_clip(rl_forward(x)["mu"])
    return x


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def _plain(x, dtype):
    """The RL pass as a plain actor-critic pass of tests/train_cases.py on obs = [features | estimator(features)]."""
    feats = np.asarray(x["features"]).astype(dtype)
    est = sup.mlp(sup.pairs(x["est_params"], dtype), feats, dtype)[-1]
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
    layers = sup.pairs(x["est_params"], dtype)
    acts = sup.mlp(layers, np.asarray(x["features"]).astype(dtype), dtype)
    t, y = np.asarray(x["terminated"]).astype(dtype), np.asarray(x["labels"]).astype(dtype)
    d = (acts[-1] - y) * t
    n = d.size
    up = dtype(x["upstream"] if upstream is None else upstream)
    G = (2 * d * t / n * up).astype(dtype)
    pers = [int(slices)] * len(layers) if isinstance(slices, (int, np.integer)) else slices
    grads, _ = sup.chain_backward(layers, acts, G, dtype, pers)
    return dict(loss=(d * d).sum() / n, grads=grads, pred=acts[-1], d=d)


def torch_passes(x, dtype=torch.float32):
    """Both passes as torch computes them on the CPU in `dtype`: dict(mu, sigma, values, rl_grads, est_rl_grads (what autograd sends into
    the estimator from the RL cotangents: the gradient the reference discards), loss, est_grads), float64 numpy."""
    t = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)
    rl = [t(p).requires_grad_(True) for p in x["rl_params"]]
    est = [t(p).requires_grad_(True) for p in x["est_params"]]
    na = 2 * (len(x["actor"]) - 1)
    feats = t(x["features"])
    mu = sup.mlp_t(torch.cat((feats, sup.mlp_t(feats, est)), dim=-1), rl[:na])
    if x["clip"] is not None:
        mu = torch.nn.functional.hardtanh(mu, -x["clip"], x["clip"])
    sigma = mu * 0.0 + rl[-1]
    values = sup.mlp_t(t(x["critic_obs"]), rl[na:-1])
    n = lambda v: v.detach().double().numpy().copy()
    out = dict(mu=n(mu), sigma=n(sigma), values=n(values))
    if "grad_mu" in x:
        torch.autograd.backward([mu, sigma, values], [t(x["grad_mu"]), t(x["grad_sigma"]), t(x["grad_values"])])
        out.update(rl_grads=[n(p.grad) for p in rl], est_rl_grads=[n(p.grad) for p in est])
        for p in est:
            p.grad = None
    term = t(x["terminated"])
    loss = torch.nn.functional.mse_loss(sup.mlp_t(feats, est) * term, t(x["labels"]) * term)
    (loss * float(x.get("upstream", 1.0))).backward()
    out.update(loss=n(loss), est_grads=[n(p.grad) for p in est])
    return out


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
        self.actor, self.critic, self.estimator = sup.sequential(x["actor"], x["clip"]), sup.sequential(x["critic"], None), sup.sequential(x["est"], None)
        self.std = torch.nn.Parameter(torch.zeros(x["actor"][-1]))
        self.to(device=device, dtype=dtype)
        sup.set_parameters(self.rl_parameters() + self.estimator_parameters(), list(x["rl_params"]) + list(x["est_params"]), dtype)

    def rl_parameters(self):
        return list(self.actor.parameters()) + list(self.critic.parameters()) + [self.std]

    def estimator_parameters(self):
        return list(self.estimator.parameters())

    def forward(self, features, critic_obs):
        mu = self.actor(torch.cat((features, self.estimator(features)), dim=-1))
        return mu, mu * 0.0 + self.std, self.critic(critic_obs)

    def estimator_loss(self, features, labels, terminated):
        return torch.nn.functional.mse_loss(self.estimator(features) * terminated, labels * terminated)


# ---- the golden fixture (tests/golden/gen_ppo_ee_train_fixtures.py) -------------------------------------------------------------------------
FIXTURE_COLUMNS = ("critic_obs", "features", "actions", "target_values", "advantages", "returns", "old_log_prob", "old_mu", "old_sigma")
EST_COLUMNS = ("est_features", "est_labels", "est_terminated")
CFG_KEYS = ("lr0", "beta1", "beta2", "eps", "max_grad_norm", "desired_kl", "steps", "clip_param", "value_loss_coef", "entropy_coef", "clip_actions",
            "estimator_lr", "est_steps", "est_epochs")


def load_fixture(path):
    """tests/train_support.load_two_pass_fixture's dict with est / actor / critic widths: per RL step the columns, mu, sigma, values, loss,
    kl, lr, grad_norm, grads, params; per estimator step est_features, est_labels, est_terminated, est_loss, est_grads, est_grad_norm,
    est_params."""
    return sup.load_two_pass_fixture(path, CFG_KEYS, dict(est="estimator", actor="actor", critic="critic"), "est", FIXTURE_COLUMNS + EST_COLUMNS + (
        "mu", "sigma", "values", "loss", "kl", "lr", "grad_norm", "est_loss", "est_grad_norm"))


def fixture_inputs(fx, params, rl_step=None, est_step=None):
    """The inputs of one step of the fixture around `params` (name -> array), as make_inputs shapes them, float64."""
    x = dict(est=fx["est"], actor=fx["actor"], critic=fx["critic"], clip=fx["cfg"]["clip_actions"], rl_params=[params[n] for n in fx["rl_names"]],
             est_params=[params[n] for n in fx["est_names"]], upstream=1.0)
    if rl_step is not None:
        x.update(features=fx["features"][rl_step], critic_obs=fx["critic_obs"][rl_step])
    if est_step is not None:
        x.update(features=fx["est_features"][est_step], labels=fx["est_labels"][est_step], terminated=fx["est_terminated"][est_step])
    return x

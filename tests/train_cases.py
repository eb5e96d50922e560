"""The fused learner pass's cases, shared by tests/test_train_host.py (CPU) and tests/test_gpu_train.py (GPU): one net table, one case
table, the input generator, a numpy restatement of include/lgtrain.h's forward and hand-written backward in a chosen dtype (float64: the
reference of every comparison), the same pass as torch autograd on the CPU (float32: the torch-CPU-f32 side of the parity rule; float64:
the check of the restatement) and the plan restated, all on the one copy of the chain arithmetic, the plan's rules, the parity rule and
the fixture readers in tests/train_support.py.  Nothing here loads the HIP library."""
import numpy as np
import torch

from tests import train_support as sup
from tests.train_support import (CLASSES, LDS_BYTES, MAX_SLICES, MIN_SLICE_ROWS, WG_TILE, check_parity, fixture_loss_inputs, lds_stride,  # noqa: F401
                                 max_err, parity_bound, slice_sum, tensor_class)

# name -> (actor widths, critic widths), [in, out_0, ..., out_last] each; every hidden layer carries an ELU, the actor ends in a Hardtanh
NETS = {
    "tiny":     ([5, 33, 7, 3], [6, 17, 1]),
    "go2":      ([45, 512, 256, 128, 12], [45, 512, 256, 128, 1]),
    "deep4":    ([9, 20, 31, 16, 4], [9, 15, 48, 1]),               # a 4-layer chain; hidden widths 0 and 15 mod 16
    "one_four": ([7, 5], [7, 19, 16, 15, 1]),                      # a chain of one layer beside one of four
}
RAGGED = (1, 4, 5, 16, 17, 65)
for _k in RAGGED:                                                   # two-layer nets: K and M each as the reduction and as the output width
    for _m in RAGGED:
        NETS[f"k{_k}_m{_m}"] = ([_k, _m, 3], [_m, _k, 1])
SWEEP = [f"k{k}_m{m}" for k in RAGGED for m in RAGGED]

BATCHES = (1, 31, 33, 257)
# name -> net, rows, seed; `clip`: None for an actor without a Hardtanh
CASES = {}
for _net in ("tiny", "go2", "deep4", "one_four"):
    for _b in BATCHES:
        CASES[f"{_net}_b{_b}"] = dict(net=_net, B=_b, seed=100 + len(CASES))
for _net in SWEEP:
    CASES[f"{_net}_b33"] = dict(net=_net, B=33, seed=100 + len(CASES))
CASES["tiny_b128"] = dict(net="tiny", B=128, seed=301)             # two slices, exact
CASES["tiny_noclip_b33"] = dict(net="tiny", B=33, seed=302, clip=None)
RAGGED_SLICE_NETS = ("tiny", "go2")                                 # plus, for each, the smallest B the plan slices raggedly (smallest_ragged_b)

TARGET_JOBS = 512              # LG_TRAIN_TARGET_JOBS


def restated_plan(n_rows, actor, critic):
    """dict(row_tile, lds_bytes, slices, slice_rows, std, h_off, g_off, p_off, std_p_off, workspace_floats, weight_jobs) of
    include/lgtrain.h's plan for chains of these widths."""
    row_tile, lds_bytes = sup.row_tile(sup.lds_widths(((actor, 0), (critic, 0))))
    d, off, jobs = sup.offsets(n_rows, (actor, critic), 0, TARGET_JOBS)
    std = sup.slice_rule(n_rows, 1, TARGET_JOBS)
    d.update(row_tile=row_tile, lds_bytes=lds_bytes, std=std, std_p_off=off, workspace_floats=off + std[0] * actor[-1], weight_jobs=jobs + std[0])
    return d


def smallest_ragged_b(net):
    """The smallest batch at which some layer of the net gets more than one slice and a last slice shorter than the others."""
    return sup.smallest_ragged_b(lambda b: restated_plan(b, *NETS[net]))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def param_names(actor, critic):
    return ["std"] + [f"{n}.{i}.{k}" for n, c in (("actor", actor), ("critic", critic)) for i in range(len(c) - 1) for k in ("weight", "bias")]


def make_inputs(case):
    """float32 numpy inputs of a case (a name of CASES, or a dict of B, seed and either `net` or `widths` = (actor, critic)): dict(actor,
    critic (widths), clip, params (list in param_names order: std, then weight and bias per layer), obs, critic_obs, grad_mu, grad_sigma,
    grad_values).  The clip as tests/train_support.place_clip places it; a case with clip=None has no Hardtanh."""
    c, (actor, critic) = sup.case_of(case, CASES, NETS)
    rng, B, f = np.random.default_rng(c["seed"]), c["B"], np.float32
    std = (0.5 + rng.random(actor[-1])).astype(f)
    x = dict(actor=actor, critic=critic, params=[std] + sup.draw_layers(rng, actor) + sup.draw_layers(rng, critic),
             obs=rng.normal(size=(B, actor[0])).astype(f), critic_obs=rng.normal(size=(B, critic[0])).astype(f),
             grad_mu=rng.normal(size=(B, actor[-1])).astype(f), grad_sigma=rng.normal(size=(B, actor[-1])).astype(f),
             grad_values=rng.normal(size=(B, critic[-1])).astype(f), clip=None)
    if "clip" in c and c["clip"] is None:
        return x
    x["clip"] = sup.place_clip(forward(x, np.float64)["mu"])
    return x


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def _chains(x, dtype):
    p, na = x["params"], 2 * (len(x["actor"]) - 1)
    return np.asarray(p[0]).astype(dtype), sup.pairs(p[1:1 + na], dtype), sup.pairs(p[1 + na:], dtype)


def forward(x, dtype=np.float64):
    """dict(mu, sigma, values, acts=(actor activations, critic activations)) of include/lgtrain.h's forward in numpy `dtype`."""
    std, actor, critic = _chains(x, dtype)
    a = sup.mlp(actor, np.asarray(x["obs"]).astype(dtype), dtype)
    c = sup.mlp(critic, np.asarray(x["critic_obs"]).astype(dtype), dtype)
    mu = sup.hardtanh(a[-1], x["clip"], dtype)
    return dict(mu=mu, sigma=mu * 0 + std, values=c[-1], acts=(a, c))


def backward(x, dtype=np.float64, wrong=None, slices=None):
    """The hand-written backward of include/lgtrain.h in numpy `dtype`: the gradients in param_names order.  `slices` (rows per slice):
    the batch sums are formed per slice and added in slice order, as the kernel does; one number for every sum, or (std, [per actor
    layer], [per critic layer]) as the plan gives each layer its own.  wrong = "no_mask" / "elu1" / "drop_last_slice" are deliberately
    wrong variants for the rule's own test."""
    fw = forward(x, dtype)
    _, actor, critic = _chains(x, dtype)
    B = fw["mu"].shape[0]
    if slices is None or isinstance(slices, (int, np.integer)):
        std_per = int(slices or B)
        layer_per = [[std_per] * len(actor), [std_per] * len(critic)]
    else:
        std_per, layer_per = int(slices[0]), [[int(p) for p in c] for c in slices[1:]]
    drop = wrong == "drop_last_slice"
    if drop and not (slices and B > max([std_per] + [p for c in layer_per for p in c])):
        raise ValueError("drop_last_slice needs more than one slice")
    g_mu = sup.masked_grad_mu(x["grad_mu"], fw["mu"], None if wrong == "no_mask" else x["clip"], dtype)
    grads = [sup.slice_sum(std_per, np.asarray(x["grad_sigma"]).astype(dtype), drop_last=drop)]
    for layers, acts, G, pers in ((actor, fw["acts"][0], g_mu, layer_per[0]), (critic, fw["acts"][1], np.asarray(x["grad_values"]).astype(dtype), layer_per[1])):
        grads += sup.chain_backward(layers, acts, G, dtype, pers, drop_last=drop, elu1=wrong == "elu1")[0]
    return grads


def torch_pass(x, dtype=torch.float32):
    """The same pass as the torch module computes it on the CPU in `dtype` (Linear, ELU, Hardtanh, mu * 0 + std; autograd for the
    gradients of the three incoming cotangents): dict(mu, sigma, values, grads), float64 numpy arrays."""
    t = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)
    params = [t(p).requires_grad_(True) for p in x["params"]]
    na = len(x["actor"]) - 1
    mu = sup.mlp_t(t(x["obs"]), params[1:1 + 2 * na])
    if x["clip"] is not None:
        mu = torch.nn.functional.hardtanh(mu, -x["clip"], x["clip"])
    sigma = mu * 0.0 + params[0]
    values = sup.mlp_t(t(x["critic_obs"]), params[1 + 2 * na:])
    torch.autograd.backward([mu, sigma, values], [t(x["grad_mu"]), t(x["grad_sigma"]), t(x["grad_values"])])
    n = lambda v: v.detach().double().numpy().copy()
    return dict(mu=n(mu), sigma=n(sigma), values=n(values), grads=[n(p.grad) for p in params])


def named(x, outs, grads):
    """dict name -> array of a pass's outputs and gradients."""
    d = dict(mu=outs["mu"], sigma=outs["sigma"], values=outs["values"])
    d.update(zip(param_names(x["actor"], x["critic"]), grads))
    return d


def references(x):
    """(float64 restatement, torch CPU float32) of a case, as `named` dicts."""
    t32 = torch_pass(x)
    return named(x, forward(x), backward(x)), named(x, t32, t32["grads"])


# ---- the module -----------------------------------------------------------------------------------------------------------------------------
class Module(torch.nn.Module):
    """The plain ActorCritic's members as FusedTrainPass reads them (.actor, .critic, .std), holding a case's parameters."""

    def __init__(self, x, device="cpu", dtype=torch.float32):
        super().__init__()
        self.std = torch.nn.Parameter(torch.zeros(x["actor"][-1]))    # first, as in the reference's ActorCritic: parameters() starts with it
        self.actor, self.critic = sup.sequential(x["actor"], x["clip"]), sup.sequential(x["critic"], None)
        self.to(device=device, dtype=dtype)
        sup.set_parameters(self.ordered_parameters(), x["params"], dtype)

    def ordered_parameters(self):
        """In param_names order."""
        return [self.std] + [p for c in (self.actor, self.critic) for m in c if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)]

    def forward(self, obs, critic_obs):
        mu = self.actor(obs)
        return mu, mu * 0.0 + self.std, self.critic(critic_obs)


# ---- the golden fixture (tests/golden/gen_ppo_train_fixtures.py) ----------------------------------------------------------------------------
FIXTURE_COLUMNS = ("obs", "critic_obs", "actions", "target_values", "advantages", "returns", "old_log_prob", "old_mu", "old_sigma")


def load_fixture(path):
    """dict(names, shapes, actor, critic (widths), cfg, init=[arrays], per step: the mini-batch columns, mu, sigma, values, loss, kl, lr,
    grad_norm, grads=[per step [arrays]], params=[per step [arrays]]), everything float64."""
    z = np.load(path)
    names, by_name = sup.fixture_shapes(z)
    split = lambda flat: sup.split_flat(flat, by_name, names)
    keys = ("lr0", "beta1", "beta2", "eps", "max_grad_norm", "desired_kl", "steps", "clip_param", "value_loss_coef", "entropy_coef", "clip_actions")
    cfg = dict(zip(keys, (float(v) for v in z["cfg"])))
    cfg["steps"] = int(cfg["steps"])
    out = dict(names=names, shapes=[by_name[n] for n in names], cfg=cfg, actor=sup.chain_widths(names, by_name, "actor"),
               critic=sup.chain_widths(names, by_name, "critic"), init=split(z["init"]), grads=[split(g) for g in z["grads"]],
               params=[split(p) for p in z["params"]])
    for k in FIXTURE_COLUMNS + ("mu", "sigma", "values", "loss", "kl", "lr", "grad_norm"):
        out[k] = z[k]
    return out


def fixture_step(fx, s, params=None):
    """The inputs of step s of the fixture as make_inputs shapes them (float64, no incoming gradients yet); `params`: instead of the
    fixture's own parameters before that step."""
    params = params if params is not None else (fx["init"] if s == 0 else fx["params"][s - 1])
    return dict(actor=fx["actor"], critic=fx["critic"], clip=fx["cfg"]["clip_actions"], params=list(params), obs=fx["obs"][s],
                critic_obs=fx["critic_obs"][s])

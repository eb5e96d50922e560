"""The fused learner pass's cases, shared by tests/test_train_host.py (CPU) and tests/test_gpu_train.py (GPU): one net table, one case
table, the input generator, a numpy restatement of include/lgtrain.h's forward and hand-written backward in a chosen dtype (float64: the
reference of every comparison), the same pass as torch autograd on the CPU (float32: the torch-CPU-f32 side of the parity rule; float64:
the check of the restatement), the slice rule restated, and the parity rule.  Nothing here loads the HIP library."""
import numpy as np
import torch

from tests.optim_cases import PARITY_FACTOR

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

# the plan's constants (include/lgtrain.h), restated
WG_TILE, MIN_SLICE_ROWS, TARGET_JOBS, MAX_SLICES, LDS_BYTES = 64, 64, 512, 32, 160 * 1024


def lds_stride(w):
    return (((((w + 3) & ~3) - 4 + 63) // 64) * 64) + 4


def slice_rule(n_rows, tiles):
    """(slices, rows per slice) of a layer of `tiles` 64 x 64 gradient tiles."""
    want = min(max(1, n_rows // MIN_SLICE_ROWS), max(1, TARGET_JOBS // tiles), MAX_SLICES)
    per = (-(-n_rows // want) + 3) & ~3
    return -(-n_rows // per), per


def restated_plan(n_rows, actor, critic):
    """dict(row_tile, lds_bytes, slices, slice_rows, std, h_off, g_off, p_off, std_p_off, workspace_floats, weight_jobs) of
    include/lgtrain.h's plan for chains of these widths."""
    w = [0, 0]
    for c in (actor, critic):
        for i, width in enumerate(c):
            w[i & 1] = max(w[i & 1], lds_stride(width))
    row_tile = next((r for r in (32, 16, 8) if r * (w[0] + w[1]) * 4 <= LDS_BYTES), 0)
    off, h_off, g_off, p_off, slices, rows, jobs = 0, [], [], [], [], [], 0
    for c in (actor, critic):
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
    for c in (actor, critic):
        p, s, r = [], [], []
        for li in range(len(c) - 1):
            K, M = c[li], c[li + 1]
            tiles = -(-M // WG_TILE) * -(-K // WG_TILE)
            S, per = slice_rule(n_rows, tiles)
            p.append(off)
            off += S * (M * K + M)
            jobs += S * tiles
            s.append(S)
            r.append(per)
        p_off.append(p)
        slices.append(s)
        rows.append(r)
    std = slice_rule(n_rows, 1)
    std_p_off = off
    off += std[0] * actor[-1]
    return dict(row_tile=row_tile, lds_bytes=row_tile * (w[0] + w[1]) * 4, slices=slices, slice_rows=rows, std=std, h_off=h_off, g_off=g_off,
                p_off=p_off, std_p_off=std_p_off, workspace_floats=off, weight_jobs=jobs + std[0])


def smallest_ragged_b(net):
    """The smallest batch at which some layer of the net gets more than one slice and a last slice shorter than the others."""
    actor, critic = NETS[net]
    for b in range(1, 4096):
        p = restated_plan(b, actor, critic)
        for S, per in [x for c in zip(p["slices"], p["slice_rows"]) for x in zip(*c)]:
            if S > 1 and b % per:
                return b
    raise AssertionError(net)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def param_names(actor, critic):
    return ["std"] + [f"{n}.{i}.{k}" for n, c in (("actor", actor), ("critic", critic)) for i in range(len(c) - 1) for k in ("weight", "bias")]


def make_inputs(case):
    """float32 numpy inputs of a case: dict(actor, critic (widths), clip, params (list in param_names order: std, then weight and bias per
    layer), obs, critic_obs, grad_mu, grad_sigma, grad_values).  The clip is placed so that a good share of the means saturates and no
    pre-clip mean lies within 1e-3 of it, so that no rounding moves a mask decision."""
    c = CASES[case] if isinstance(case, str) else case
    actor, critic = NETS[c["net"]]
    rng, B = np.random.default_rng(c["seed"]), c["B"]
    f = np.float32
    params = [(0.5 + rng.random(actor[-1])).astype(f)]
    for ch in (actor, critic):
        for li in range(len(ch) - 1):
            params.append((rng.normal(size=(ch[li + 1], ch[li])) * (1.3 / np.sqrt(ch[li]))).astype(f))
            params.append((0.2 * rng.normal(size=ch[li + 1])).astype(f))
    x = dict(actor=actor, critic=critic, params=params, obs=rng.normal(size=(B, actor[0])).astype(f),
             critic_obs=rng.normal(size=(B, critic[0])).astype(f), grad_mu=rng.normal(size=(B, actor[-1])).astype(f),
             grad_sigma=rng.normal(size=(B, actor[-1])).astype(f), grad_values=rng.normal(size=(B, critic[-1])).astype(f), clip=None)
    if "clip" in c and c["clip"] is None:
        return x
    pre = forward(x, np.float64)["mu"]
    clip = float(f(np.median(np.abs(pre))))
    while np.abs(np.abs(pre) - clip).min() < 1e-3:
        clip = float(f(clip + 2.5e-3))
    x["clip"] = clip
    return x


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def _chains(x, dtype):
    p = [np.asarray(t).astype(dtype) for t in x["params"]]
    na = len(x["actor"]) - 1
    return p[0], [(p[1 + 2 * i], p[2 + 2 * i]) for i in range(na)], [(p[1 + 2 * na + 2 * i], p[2 + 2 * na + 2 * i]) for i in range(len(x["critic"]) - 1)]


def _mlp(layers, h, dtype):
    acts = [h]
    for i, (W, b) in enumerate(layers):
        h = h @ W.T + b
        if i < len(layers) - 1:
            h = np.where(h > 0, h, np.expm1(np.minimum(h, 0))).astype(dtype)
        acts.append(h)
    return acts


def forward(x, dtype=np.float64):
    """dict(mu, sigma, values, acts=(actor activations, critic activations)) of include/lgtrain.h's forward in numpy `dtype`."""
    std, actor, critic = _chains(x, dtype)
    a = _mlp(actor, np.asarray(x["obs"]).astype(dtype), dtype)
    c = _mlp(critic, np.asarray(x["critic_obs"]).astype(dtype), dtype)
    mu = a[-1]
    if x["clip"] is not None:
        mu = np.where(mu < -x["clip"], -x["clip"], np.where(mu > x["clip"], x["clip"], mu)).astype(dtype)
    return dict(mu=mu, sigma=mu * 0 + std, values=c[-1], acts=(a, c))


def slice_sum(per, g, h=None, phases=1, drop_last=False):
    """The sum over the batch of g (or of g^T h) as the kernels form it: per slice of `per` rows, the slices added in slice order.  phases
    = 4: a column sum of a slice is ((s0 + s1) + s2) + s3 with s_p over the rows p, p + 4, ... of the slice, as the weight-gradient wave
    forms a bias partial; 1: row after row, as grad_std's column sums.  drop_last: without the last slice (a wrong variant)."""
    def cols(a):
        if phases == 1:
            return a.sum(0)
        s = [a[p::phases].sum(0) for p in range(phases)]
        out = s[0]
        for v in s[1:]:
            out = out + v
        return out
    parts = [cols(g[s:s + per]) if h is None else g[s:s + per].T @ h[s:s + per] for s in range(0, g.shape[0], per)]
    if drop_last:
        parts = parts[:-1]
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    return out


def backward(x, dtype=np.float64, wrong=None, slices=None):
    """The hand-written backward of include/lgtrain.h in numpy `dtype`: the gradients in param_names order.  `slices` (rows per slice):
    the batch sums are formed per slice and added in slice order, as the kernel does; one number for every sum, or (std, [per actor
    layer], [per critic layer]) as the plan gives each layer its own.  wrong = "no_mask" / "elu1" / "drop_last_slice" are deliberately
    wrong variants for the rule's own test."""
    fw = forward(x, dtype)
    std, actor, critic = _chains(x, dtype)
    B = fw["mu"].shape[0]
    if slices is None or isinstance(slices, (int, np.integer)):
        std_per, layer_per = int(slices or B), None
    else:
        std_per, layer_per = int(slices[0]), [[int(p) for p in c] for c in slices[1:]]

    if wrong == "drop_last_slice" and not (slices and B > max([std_per] + [p for c in layer_per or [] for p in c])):
        raise ValueError("drop_last_slice needs more than one slice")

    def bsum(per, g, h=None, phases=1):
        return slice_sum(per, g, h, phases, drop_last=wrong == "drop_last_slice")

    grads = [bsum(std_per, np.asarray(x["grad_sigma"]).astype(dtype))]
    g_mu = np.asarray(x["grad_mu"]).astype(dtype)
    if x["clip"] is not None and wrong != "no_mask":
        g_mu = np.where((fw["mu"] >= x["clip"]) | (fw["mu"] <= -x["clip"]), 0, g_mu).astype(dtype)
    for ci, (layers, acts, G) in enumerate(((actor, fw["acts"][0], g_mu), (critic, fw["acts"][1], np.asarray(x["grad_values"]).astype(dtype)))):
        out = []
        for li in range(len(layers) - 1, -1, -1):
            H, per = acts[li], layer_per[ci][li] if layer_per else std_per
            out = [bsum(per, G, H), bsum(per, G, phases=4)] + out
            if li:
                d = np.ones_like(H) if wrong == "elu1" else np.where(H > 0, 1, H + 1)
                G = ((G @ layers[li][0]) * d).astype(dtype)
        grads += out
    return grads


def torch_pass(x, dtype=torch.float32):
    """The same pass as the torch module computes it on the CPU in `dtype` (Linear, ELU, Hardtanh, mu * 0 + std; autograd for the
    gradients of the three incoming cotangents): dict(mu, sigma, values, grads), float64 numpy arrays."""
    t = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)
    params = [t(p).requires_grad_(True) for p in x["params"]]
    na = len(x["actor"]) - 1

    def mlp(h, ps):
        for i in range(0, len(ps), 2):
            h = torch.nn.functional.linear(h, ps[i], ps[i + 1])
            if i < len(ps) - 2:
                h = torch.nn.functional.elu(h)
        return h
    mu = mlp(t(x["obs"]), params[1:1 + 2 * na])
    if x["clip"] is not None:
        mu = torch.nn.functional.hardtanh(mu, -x["clip"], x["clip"])
    sigma = mu * 0.0 + params[0]
    values = mlp(t(x["critic_obs"]), params[1 + 2 * na:])
    torch.autograd.backward([mu, sigma, values], [t(x["grad_mu"]), t(x["grad_sigma"]), t(x["grad_values"])])
    n = lambda v: v.detach().double().numpy().copy()
    return dict(mu=n(mu), sigma=n(sigma), values=n(values), grads=[n(p.grad) for p in params])


# ---- the parity rule ------------------------------------------------------------------------------------------------------------------------
# Per tensor (mu, sigma, values and every parameter gradient): |kernel - f64| <= PARITY_FACTOR * max(|torch-CPU-f32 - f64|, one float32 ulp
# of that tensor's largest magnitude), both sides on the same float32 inputs: the rule of tests/optim_cases.py, whose factor 8 comes from
# the number formats.  Here the two float32 evaluations differ in (a) the order of every dot product (the MFMA's k permutation and the
# batch slices against torch's blocked GEMM), each side a sum of the same products with roundings of at most half an ulp of its partial
# sums: one side at most twice the other; (b) expm1f and elu' = h + 1 against torch's exp: one rounding more on one side, a factor 2 on
# the share of the error that passes an ELU; (c) the statistic is a maximum over the elements of two error samples of like spread, a
# factor 2 except in a vanishing share of draws.
CLASSES = ("outputs", "grad_weight", "grad_bias", "grad_std")


def tensor_class(name):
    return "outputs" if name in ("mu", "sigma", "values") else "grad_std" if name == "std" else "grad_weight" if name.endswith("weight") else "grad_bias"


def max_err(a, ref):
    return float(np.abs(np.asarray(a, np.float64).reshape(-1) - np.asarray(ref, np.float64).reshape(-1)).max())


def parity_bound(err_f32, ref64):
    return PARITY_FACTOR * max(float(err_f32), float(np.abs(ref64).max()) * 2.0 ** -23)


def check_parity(got, ref64, ref32, label, report=None):
    """got / ref64 / ref32: dict name -> array (mu, sigma, values and the parameter names).  Every tensor against the rule; prints the worst
    ratio of each tensor class before it asserts.  Returns {class: worst |kernel - f64| / max(|f32 - f64|, ulp)}."""
    worst, bad = {k: 0.0 for k in CLASSES}, []
    for name, r64 in ref64.items():
        err, err32 = max_err(got[name], r64), max_err(ref32[name], r64)
        bound = parity_bound(err32, r64)
        ratio = err / (bound / PARITY_FACTOR) if bound else (0.0 if err == 0.0 else float("inf"))
        k = tensor_class(name)
        worst[k] = max(worst[k], ratio if np.isfinite(ratio) else float("inf"))
        if not (np.isfinite(err) and err <= bound):
            bad.append(f"{label} {name}: |kernel - f64| = {err:.3e} above {bound:.3e} (torch f32 {err32:.3e})")
    print(f"{label}: worst |kernel - f64| / max(|f32 - f64|, ulp): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" (allowed {PARITY_FACTOR:g})")
    if report is not None:
        report.append((label, worst))
    assert not bad, "\n".join(bad)
    return worst


def named(x, outs, grads):
    """dict name -> array of a pass's outputs and gradients."""
    d = dict(mu=outs["mu"], sigma=outs["sigma"], values=outs["values"])
    d.update(zip(param_names(x["actor"], x["critic"]), grads))
    return d


# ---- the module -----------------------------------------------------------------------------------------------------------------------------
class Module(torch.nn.Module):
    """The plain ActorCritic's members as FusedTrainPass reads them (.actor, .critic, .std), holding a case's parameters."""

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
        self.std = nn.Parameter(torch.zeros(x["actor"][-1]))          # first, as in the reference's ActorCritic: parameters() starts with it
        self.actor, self.critic = chain(x["actor"], x["clip"]), chain(x["critic"], None)
        self.to(device=device, dtype=dtype)
        with torch.no_grad():
            for p, v in zip(self.ordered_parameters(), x["params"]):
                p.copy_(torch.as_tensor(np.asarray(v)).to(dtype))

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
    shapes = [tuple(int(d) for d in s if d) for s in z["shapes"]]
    sizes = [int(np.prod(s)) for s in shapes]
    ends = np.cumsum(sizes)
    split = lambda flat: [flat[e - n:e].reshape(s).copy() for n, e, s in zip(sizes, ends, shapes)]
    keys = ("lr0", "beta1", "beta2", "eps", "max_grad_norm", "desired_kl", "steps", "clip_param", "value_loss_coef", "entropy_coef", "clip_actions")
    cfg = dict(zip(keys, (float(v) for v in z["cfg"])))
    cfg["steps"] = int(cfg["steps"])
    names = [str(n) for n in z["names"]]
    widths = lambda chain: [shapes[names.index(n)][1] for n in names if n.startswith(chain) and n.endswith("weight")][:1] + \
        [shapes[names.index(n)][0] for n in names if n.startswith(chain) and n.endswith("weight")]
    out = dict(names=names, shapes=shapes, cfg=cfg, actor=widths("actor"), critic=widths("critic"), init=split(z["init"]),
               grads=[split(g) for g in z["grads"]], params=[split(p) for p in z["params"]])
    for k in FIXTURE_COLUMNS + ("mu", "sigma", "values", "loss", "kl", "lr", "grad_norm"):
        out[k] = z[k]
    return out


def fixture_step(fx, s, params=None):
    """The inputs of step s of the fixture as make_inputs shapes them (float64, no incoming gradients yet); `params`: instead of the
    fixture's own parameters before that step."""
    params = params if params is not None else (fx["init"] if s == 0 else fx["params"][s - 1])
    return dict(actor=fx["actor"], critic=fx["critic"], clip=fx["cfg"]["clip_actions"], params=list(params), obs=fx["obs"][s],
                critic_obs=fx["critic_obs"][s])


def fixture_loss_inputs(fx, s, mu, sigma, values):
    """tests/ppo_loss_cases.restate's input for step s of the fixture around the given network outputs."""
    g = dict(mu=mu, sigma=sigma, actions=fx["actions"][s], advantages=fx["advantages"][s], old_log_prob=fx["old_log_prob"][s],
             old_mu=fx["old_mu"][s], old_sigma=fx["old_sigma"][s])
    return dict(groups=[g], values=values, returns=fx["returns"][s], target_values=fx["target_values"][s])

"""The fused optimizer step's cases, shared by tests/test_optim_host.py (CPU) and tests/test_gpu_optim.py (GPU): one case table, the
input generator, a torch restatement of include/lgoptim.h on the CPU in a chosen dtype (float64: the reference of every comparison;
float32: the torch-CPU-f32 side of the parity rule), the tie table of the learning-rate rule, and the parity rule.  Nothing here loads
the HIP library."""
import numpy as np
import torch

SCALES = {"never": 0.01, "mixed": 1.0, "always": 30.0}      # gradient scale -> what the clip does over a run
# the total gradient norm of step s is scale * NORM_PROFILE[s] * max_grad_norm: at scale 1 on both sides of the clip threshold and at
# least 10 % away from it, at 0.01 always below, at 30 always above
NORM_PROFILE = (1.5, 0.6, 1.3, 0.8, 1.1)
STEPS = (1, 5)
DEFAULTS = dict(betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0, lr=1e-3)
TWO_SWEEPS = 512 * 1024 + 1

# name -> numels; `view`: parameter 0 (and its gradient and moments) is a view at a 1-float offset into a larger storage, so all four of
# its arrays miss the 16-byte alignment; `steps`: the step counts run (default STEPS)
CASES = {
    "n1":          dict(numels=[1], seed=31),
    "n3":          dict(numels=[3], seed=32),
    "n4":          dict(numels=[4], seed=33),
    "n5":          dict(numels=[5], seed=34),
    "n1023":       dict(numels=[1023], seed=35),
    "n1024":       dict(numels=[1024], seed=36),
    "n1025":       dict(numels=[1025], seed=37),
    "tiny_actor":  dict(numels=[16 * 7, 16, 8 * 16, 8, 12], seed=38),
    "view_off1":   dict(numels=[2048 + 5, 12], view=True, seed=39),
    "t64_ragged":  dict(numels=[1 + (37 * i * i + 11 * i) % 1500 for i in range(64)], seed=40),
    "two_sweeps":  dict(numels=[TWO_SWEEPS], steps=(1,), seed=41),
    "other_hyper": dict(numels=[16 * 7, 16, 1025, 12], betas=(0.8, 0.9), eps=1e-5, max_grad_norm=0.5, seed=42),
}


def hyper(case):
    c = CASES[case] if isinstance(case, str) else case
    return {k: c.get(k, v) for k, v in DEFAULTS.items()}


def make_inputs(case, scale, steps=None):
    """float32 numpy inputs of a table case: (params, grads_per_step).  The gradients of step s, all tensors together, have the norm
    scale * NORM_PROFILE[s] * max_grad_norm (up to their rounding to float32)."""
    c = CASES[case] if isinstance(case, str) else case
    rng, h = np.random.default_rng(c["seed"]), hyper(c)
    steps = steps if steps is not None else max(c.get("steps", STEPS))
    params = [(0.5 * rng.normal(size=n)).astype(np.float32) for n in c["numels"]]
    grads = []
    for s in range(steps):
        z = [rng.normal(size=n) for n in c["numels"]]
        total = np.sqrt(sum(float((x * x).sum()) for x in z))
        grads.append([(x * (scale * NORM_PROFILE[s % len(NORM_PROFILE)] * h["max_grad_norm"] / total)).astype(np.float32) for x in z])
    return params, grads


def adjust_rate(kl, lr, desired_kl):
    """ppo_loss.adjust_learning_rate, restated (the host test compares the two bit for bit)."""
    kl = float(kl)
    if kl > desired_kl * 2.0:
        return max(1e-5, lr / 1.5)
    if kl < desired_kl / 2.0 and kl > 0.0:
        return min(1e-2, lr * 1.5)
    return lr


def restate(params, grads_per_step, lr0=1e-3, kls=None, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0, desired_kl=None, dtype=torch.float64,
            exp_avg=None, exp_avg_sq=None, step0=0, wrong=None):
    """The clip, the rate rule and Adam of include/lgoptim.h in torch ops of `dtype` on the CPU, in the header's operation order.  The
    total norm is torch's norm of the per-tensor norms in `dtype` (what clip_grad_norm_ forms).  A gradient that is None leaves its tensor
    out of that step.  kls: one KL per step (None: the rate stays).  Returns a list, one entry per step, of
    dict(params, exp_avg, exp_avg_sq: lists of float64 numpy arrays; lr, grad_norm, clip_coef, step).
    wrong="no_bias_correction" / "clip_per_tensor" are deliberately wrong variants for the rule's own test."""
    t = lambda x: torch.as_tensor(np.asarray(x)).to(dtype).clone()
    p = [t(x) for x in params]
    m = [torch.zeros_like(x) if exp_avg is None else t(exp_avg[i]) for i, x in enumerate(p)]
    v = [torch.zeros_like(x) if exp_avg_sq is None else t(exp_avg_sq[i]) for i, x in enumerate(p)]
    lr, step, out = float(lr0), int(step0), []
    beta1, beta2 = betas
    n = lambda xs: [x.double().numpy().copy() for x in xs]
    for s, grads in enumerate(grads_per_step):
        if kls is not None and kls[s] is not None:
            lr = adjust_rate(kls[s], lr, desired_kl)
        live = [i for i, g in enumerate(grads) if g is not None]
        if not live:
            out.append(dict(params=n(p), exp_avg=n(m), exp_avg_sq=n(v), lr=lr, grad_norm=float("nan"), clip_coef=float("nan"), step=step))
            continue
        step += 1
        g = {i: t(grads[i]) for i in live}
        total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g[i]) for i in live]))
        coef = torch.ones((), dtype=dtype)
        if max_grad_norm is not None:
            coef = torch.clamp(torch.full((), max_grad_norm, dtype=dtype) / (total + 1e-6), max=1.0)
        bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
        if wrong == "no_bias_correction":
            bc1 = bc2 = 1.0
        step_size, bc2_sqrt = lr / bc1, bc2 ** 0.5
        for i in live:
            c = coef if wrong != "clip_per_tensor" else torch.clamp(max_grad_norm / (torch.linalg.vector_norm(g[i]) + 1e-6), max=1.0)
            gc = g[i] * c
            m[i] = m[i] + (gc - m[i]) * (1 - beta1)
            v[i] = v[i] * beta2 + ((1 - beta2) * gc) * gc
            p[i] = p[i] + (-step_size) * (m[i] / (v[i].sqrt() / bc2_sqrt + eps))
        out.append(dict(params=n(p), exp_avg=n(m), exp_avg_sq=n(v), lr=lr, grad_norm=float(total), clip_coef=float(coef), step=step))
    return out


def torch_reference(params, grads_per_step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=1.0, dtype=torch.float64):
    """The reference's three lines themselves: clip_grad_norm_ and torch.optim.Adam (single-tensor, torch's defaults) on the CPU.  Returns
    per step dict(params, exp_avg, exp_avg_sq, grad_norm)."""
    ps = [torch.nn.Parameter(torch.as_tensor(np.asarray(x)).to(dtype).clone()) for x in params]
    opt = torch.optim.Adam(ps, lr=lr, betas=betas, eps=eps)
    out = []
    n = lambda xs: [x.detach().double().numpy().copy() for x in xs]
    for grads in grads_per_step:
        opt.zero_grad()
        for q, g in zip(ps, grads):
            q.grad = torch.as_tensor(np.asarray(g)).to(dtype).clone()
        total = torch.nn.utils.clip_grad_norm_(ps, max_grad_norm)
        opt.step()
        out.append(dict(params=n(ps), exp_avg=n([opt.state[q]["exp_avg"] for q in ps]), exp_avg_sq=n([opt.state[q]["exp_avg_sq"] for q in ps]),
                        grad_norm=float(total)))
    return out


# ---- the learning-rate rule on ties ---------------------------------------------------------------------------------------------------------
TIE_DESIRED_KL = 2.0 ** -7


def tie_table():
    """[(kl as float32, learning rate before)]: the thresholds 2 * desired and desired / 2 themselves (exactly representable: the rate
    stays), their float32 neighbours on either side, 0, -1 and NaN (all stay), then a run of rises from 5e-3 that pins at 1e-2 and a run of
    falls from 2e-5 that pins at 1e-5.  The runs carry lr = None: the rate the step before left."""
    f = np.float32
    hi, lo = f(2.0 ** -6), f(2.0 ** -8)
    rows = [(hi, 1e-3), (lo, 1e-3), (np.nextafter(hi, f(1)), 1e-3), (np.nextafter(hi, f(0)), 1e-3), (np.nextafter(lo, f(1)), 1e-3),
            (np.nextafter(lo, f(0)), 1e-3), (f(0.0), 1e-3), (f(-1.0), 1e-3), (f(np.nan), 1e-3)]
    rows += [(f(2.0 ** -10), 5e-3)] + [(f(2.0 ** -10), None)] * 3          # 5e-3 -> 7.5e-3 -> 1e-2 -> 1e-2 -> 1e-2
    rows += [(f(1.0), 2e-5)] + [(f(1.0), None)] * 3                        # 2e-5 -> 1.33e-5 -> 1e-5 -> 1e-5 -> 1e-5
    return rows


def tie_expected(rule):
    """The rate after every row of the tie table under `rule(kl, lr, desired_kl)`."""
    out, lr = [], None
    for kl, lr0 in tie_table():
        lr = rule(float(kl), lr0 if lr0 is not None else lr, TIE_DESIRED_KL)
        out.append(lr)
    return out


# ---- the parity rule ------------------------------------------------------------------------------------------------------------------------
# Per tensor, for param, exp_avg and exp_avg_sq: |kernel - f64| <= PARITY_FACTOR * max(|torch-CPU-f32 - f64|, one float32 ulp of that
# tensor's largest magnitude), both sides restating the same float32 inputs: the form of the loss head's rule (tests/ppo_loss_cases.py).
# The factor comes from the number formats, not from the kernel.  sqrtf and / are correctly rounded on both sides and add nothing.  The
# two float32 evaluations differ in three ways, each worth a factor 2 at most:
#   (a) the compiler contracts a * b + c into one rounding where torch rounds twice, and (1 - beta2) * g' * g' may associate the other
#       way: every element's chain has the same handful of roundings of at most half an ulp on both sides, one side at most twice the other;
#   (b) the clip coefficient is a common factor of every g': the kernel forms the norm in float64 and rounds once, torch forms float32
#       norms of float32 norms; either coefficient is within two float32 roundings of the exact one, so the share of the error that the
#       coefficient carries into m (once) and v (twice) is at most twice as large on one side as on the other;
#   (c) the statistic is a maximum over the elements of two error samples of like spread, and the larger maximum of two such samples
#       exceeds the smaller by less than 2 except in a vanishing share of draws.
# Hence 8, the loss head's figure and its ceiling.  An error below one float32 ulp of the tensor's largest magnitude is not resolvable
# and is lifted to it (a one-element tensor's float32 side can be exact by luck): that floor comes from the number format.
PARITY_FACTOR = 8.0
FIELDS = ("params", "exp_avg", "exp_avg_sq")


def parity_bound(err_f32, ref64):
    return PARITY_FACTOR * max(float(err_f32), float(np.abs(ref64).max()) * 2.0 ** -23)


def max_err(x, ref64):
    return float(np.abs(np.asarray(x, np.float64).reshape(-1) - np.asarray(ref64, np.float64).reshape(-1)).max())


def check_parity(got, ref64, ref32, label, report=None):
    """got / ref64 / ref32: dict(params, exp_avg, exp_avg_sq) of per-tensor arrays.  Every tensor of every field against the rule; prints
    the worst ratio of each field before it asserts.  Returns the worst ratio err / (bound at factor 1)."""
    worst, bad = 0.0, []
    for field in FIELDS:
        field_worst = 0.0
        for i, (x, r64, r32) in enumerate(zip(got[field], ref64[field], ref32[field])):
            err, err32 = max_err(x, r64), max_err(r32, r64)
            bound = parity_bound(err32, r64)
            ratio = err / (bound / PARITY_FACTOR) if bound else 0.0
            field_worst = max(field_worst, ratio if np.isfinite(ratio) else float("inf"))
            if not (np.isfinite(err) and err <= bound):
                bad.append(f"{label} {field}[{i}]: |kernel - f64| = {err:.3e} above {bound:.3e} (torch f32 {err32:.3e})")
        print(f"{label} {field}: worst |kernel - f64| / max(|f32 - f64|, ulp) = {field_worst:.3f} (allowed {PARITY_FACTOR:g})")
        worst = max(worst, field_worst)
    if report is not None:
        report.append((label, worst))
    assert not bad, "\n".join(bad)
    return worst


# ---- the golden fixture (tests/golden/gen_ppo_update_fixtures.py) ---------------------------------------------------------------------------
def load_fixture(path):
    """dict(names, shapes, cfg=dict(lr0, betas, eps, max_grad_norm, desired_kl, steps), init=[arrays], kl, lr, grad_norm,
    grads=[per step [arrays]], params=[per step [arrays]]), everything float64."""
    z = np.load(path)
    sizes = [int(max(1, r) * max(1, c)) for r, c in z["shapes"]]
    ends = np.cumsum(sizes)
    split = lambda flat: [flat[e - n:e].copy() for n, e in zip(sizes, ends)]
    lr0, beta1, beta2, eps, max_grad_norm, desired_kl, steps = (float(x) for x in z["cfg"])
    return dict(names=[str(n) for n in z["names"]], shapes=[tuple(int(d) for d in s if d) for s in z["shapes"]],
                cfg=dict(lr0=lr0, betas=(beta1, beta2), eps=eps, max_grad_norm=max_grad_norm, desired_kl=desired_kl, steps=int(steps)),
                init=split(z["init"]), kl=z["kl"], lr=z["lr"], grad_norm=z["grad_norm"],
                grads=[split(g) for g in z["grads"]], params=[split(p) for p in z["params"]])

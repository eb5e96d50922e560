"""The fused PPO loss head's cases, shared by tests/test_ppo_loss_host.py (CPU) and tests/test_gpu_ppo_loss.py (GPU): one case table,
the input generator, a torch restatement of the formulas of include/lgppo.h in a chosen dtype (float64: the reference of every
comparison; float32: the torch-CPU-f32 side of the parity rule), and the parity rule.  Nothing here loads the HIP library."""
import math

import numpy as np
import torch

CLIP = 0.2
GAP = 0.01            # no ratio and no value step lies within GAP of a clip boundary (asserted at 1e-4 by the host test)
P_OUTSIDE = 0.35      # share of rows drawn outside the clip range

# name -> rows of each policy group, value rows, actions, flags, entropy coefficient, KL per group, seed
CASES = {
    "b1_a12":        dict(rows=[1], vrows=1, A=12, clipped=True, spo=False, ent=0.01, kl=[True], seed=11),
    "b63_a1":        dict(rows=[63], vrows=63, A=1, clipped=False, spo=False, ent=0.0, kl=[True], seed=12),
    "b64_a3":        dict(rows=[64], vrows=64, A=3, clipped=True, spo=True, ent=0.01, kl=[False], seed=13),
    "b65_a4":        dict(rows=[65], vrows=65, A=4, clipped=False, spo=True, ent=0.0, kl=[True], seed=14),
    "b257_a5":       dict(rows=[257], vrows=257, A=5, clipped=True, spo=False, ent=0.01, kl=[True], seed=15),
    "b257_a12":      dict(rows=[257], vrows=257, A=12, clipped=True, spo=False, ent=0.01, kl=[True], seed=16),
    "b257_a12_spo":  dict(rows=[257], vrows=257, A=12, clipped=True, spo=True, ent=0.0, kl=[True], seed=17),
    "b1025_a13":     dict(rows=[1025], vrows=1025, A=13, clipped=True, spo=False, ent=0.0, kl=[False], seed=18),
    "cts_17_5":      dict(rows=[17, 5], vrows=22, A=12, clipped=True, spo=False, ent=0.01, kl=[True, False], seed=19),
    "cts_300_1":     dict(rows=[300, 1], vrows=301, A=12, clipped=True, spo=False, ent=0.0, kl=[True, True], seed=20),
    "cts_65_64":     dict(rows=[65, 64], vrows=257, A=5, clipped=False, spo=False, ent=0.01, kl=[True, False], seed=21),
    "b40001_a13":    dict(rows=[40001], vrows=40001, A=13, clipped=True, spo=False, ent=0.01, kl=[True], seed=22),    # more than one sweep
}
LARGEST = "b40001_a13"
INPUT_KEYS = ("mu", "sigma", "actions", "old_log_prob", "advantages", "old_mu", "old_sigma")


def log_prob64(mu, sigma, actions):
    mu, sigma, actions = (np.asarray(x, np.float64) for x in (mu, sigma, actions))
    return (-(actions - mu) ** 2 / (2 * sigma ** 2) - np.log(sigma) - 0.5 * math.log(2 * math.pi)).sum(-1)


def gap_ratio(rng, n, clip=CLIP):
    """n ratios: P_OUTSIDE of them outside [1 - clip, 1 + clip] (half on each side), none within GAP of either bound."""
    u, where = rng.random(n), rng.random(n)
    lo = (1 - 2.5 * clip) + u * (1.5 * clip - GAP)                 # [0.5, 0.8 - GAP)
    hi = (1 + clip + GAP) + u * (1.5 * clip - GAP)                 # [1.2 + GAP, 1.5)
    mid = (1 - clip + GAP) + u * (2 * clip - 2 * GAP)              # [0.8 + GAP, 1.2 - GAP)
    return np.where(where < P_OUTSIDE / 2, lo, np.where(where < P_OUTSIDE, hi, mid))


def gap_step(rng, n, clip=CLIP):
    """n value steps v - v_t: P_OUTSIDE of them beyond +-clip, none within GAP of it; both signs."""
    u, where, sign = rng.random(n), rng.random(n), np.where(rng.random(n) < 0.5, -1.0, 1.0)
    return sign * np.where(where < P_OUTSIDE, (clip + GAP) + u * 2 * clip, u * (clip - GAP))


def old_log_prob_for(mu, sigma, actions, ratio):
    """The float32 old log-prob column that puts the row's ratio at `ratio` (up to its own rounding, ~1e-6 relative)."""
    return (log_prob64(mu, sigma, actions) - np.log(ratio)).astype(np.float32)


def make_inputs(case):
    """float32 numpy inputs of a table case: dict(groups=[{mu, sigma, actions, old_log_prob, advantages, old_mu, old_sigma}], values,
    returns, target_values).  The old log-prob and the target values are free input columns, so they are chosen to put the ratio and the
    value step where gap_ratio / gap_step drew them: both sides of every branch, never on one.  A case given as a dict may carry `clip`
    (default CLIP), the boundaries the ratios and steps are placed around; the draws of a case do not depend on it."""
    c = CASES[case] if isinstance(case, str) else case
    rng, clip = np.random.default_rng(c["seed"]), c.get("clip", CLIP)      # gap_ratio / gap_step draw the same numbers at every clip
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    A, groups = c["A"], []
    for B, kl in zip(c["rows"], c["kl"]):
        mu, sigma = f(rng.normal(size=(B, A)) * 0.5), f(0.3 + 0.9 * rng.random((B, A)))
        old_mu, old_sigma = f(mu + 0.1 * sigma * rng.normal(size=(B, A))), f(sigma * np.exp(0.05 * rng.normal(size=(B, A))))
        actions = f(old_mu + old_sigma * rng.normal(size=(B, A)))
        g = dict(mu=mu, sigma=sigma, actions=actions, old_log_prob=old_log_prob_for(mu, sigma, actions, gap_ratio(rng, B, clip)).reshape(B, 1),
                 advantages=f(rng.normal(size=(B, 1))), old_mu=old_mu if kl else None, old_sigma=old_sigma if kl else None)
        groups.append(g)
    Bv = c["vrows"]
    values = f(rng.normal(size=(Bv, 1)))
    target_values = f(values.astype(np.float64) - gap_step(rng, Bv, clip).reshape(Bv, 1))
    returns = f(target_values + 0.5 * rng.normal(size=(Bv, 1)))
    return dict(groups=groups, values=values, returns=returns, target_values=target_values)


def assert_both_sides(name, inp, clip=CLIP):
    """In float64: at B >= 63 between 10 % and 60 % of the rows have the ratio outside [1 - clip, 1 + clip], likewise |v - v_t| > clip, both
    sides and both signs of the advantage occur, and no row lies within 1e-4 of a boundary.  No row is excluded."""
    for g in inp["groups"]:
        r = np.exp(log_prob64(g["mu"], g["sigma"], g["actions"]) - g["old_log_prob"].astype(np.float64).reshape(-1))
        assert np.minimum(np.abs(r - (1 - clip)), np.abs(r - (1 + clip))).min() > 1e-4, name
        share = np.mean((r < 1 - clip) | (r > 1 + clip))
        if len(r) >= 63:
            assert 0.10 <= share <= 0.60, (name, share)
            assert (r < 1 - clip).any() and (r > 1 + clip).any() and (g["advantages"] > 0).any() and (g["advantages"] < 0).any()
    d = inp["values"].astype(np.float64) - inp["target_values"].astype(np.float64)
    assert np.abs(np.abs(d) - clip).min() > 1e-4, name
    if len(d) >= 63:
        assert 0.10 <= np.mean(np.abs(d) > clip) <= 0.60, name
        assert (d > clip).any() and (d < -clip).any()


def restate(inp, clipped, spo, ent, clip=CLIP, value_loss_coef=1.0, dtype=torch.float64, break_tie=False, drop_kl_eps=False):
    """The formulas of include/lgppo.h in torch ops of `dtype` on the CPU, gradients by autograd (so torch's conventions where branches
    meet are torch's own).  Returns numpy float64: loss, surrogate (per group), value_loss, entropy, kl (per group, None without old_mu),
    grad_mu / grad_sigma (per group), grad_values.  break_tie / drop_kl_eps are deliberately wrong variants for the rule's own test."""
    t = lambda x: torch.as_tensor(np.asarray(x)).to(dtype)
    half_log_2pi = 0.5 * math.log(2 * math.pi)
    leaves, surrogate, entropies, kls = [], [], [], []
    for g in inp["groups"]:
        mu, sigma = t(g["mu"]).requires_grad_(), t(g["sigma"]).requires_grad_()
        leaves += [mu, sigma]
        a, adv, old_lp = t(g["actions"]), t(g["advantages"]).reshape(-1), t(g["old_log_prob"]).reshape(-1)
        logp = (-(a - mu) ** 2 / (2 * sigma ** 2) - torch.log(sigma) - half_log_2pi).sum(-1)
        r = torch.exp(logp - old_lp)
        if spo:
            s = -(adv * r - torch.abs(adv) * (r - 1.0) ** 2 / (2.0 * clip))
        else:
            rc = torch.clamp(r, 1.0 - clip, 1.0 + clip)
            s = torch.max(-adv * r, -adv * (rc.detach() if break_tie else rc))
        surrogate.append(s.mean())
        entropies.append((0.5 + half_log_2pi + torch.log(sigma)).sum(-1))
        if g.get("old_mu") is not None:
            om, osg = t(g["old_mu"]), t(g["old_sigma"])
            with torch.no_grad():
                kls.append(torch.sum(torch.log(sigma / osg + (0.0 if drop_kl_eps else 1.e-5)) + (osg ** 2 + (om - mu) ** 2) / (2.0 * sigma ** 2) - 0.5,
                                     dim=-1).mean())
        else:
            kls.append(None)
    v = t(inp["values"]).requires_grad_()
    R, vt = t(inp["returns"]), t(inp["target_values"])
    if clipped:
        vc = vt + (v - vt).clamp(-clip, clip)
        value_loss = torch.max((v - R) ** 2, (vc - R) ** 2).mean()
    else:
        value_loss = ((R - v) ** 2).mean()
    entropy = torch.cat(entropies).mean()
    loss = sum(surrogate) + value_loss_coef * value_loss - ent * entropy
    grads = torch.autograd.grad(loss, leaves + [v])
    n = lambda x: x.detach().double().numpy()
    return dict(loss=n(loss), surrogate=[n(s) for s in surrogate], value_loss=n(value_loss), entropy=n(entropy),
                kl=[None if k is None else n(k) for k in kls], grad_mu=[n(x) for x in grads[0:-1:2]], grad_sigma=[n(x) for x in grads[1:-1:2]],
                grad_values=n(grads[-1]))


def restate_case(case, inp=None, dtype=torch.float64, **kw):
    c = CASES[case]
    return restate(inp if inp is not None else make_inputs(case), c["clipped"], c["spo"], c["ent"], dtype=dtype, **kw)


def outputs(res):
    """(name, array) of every scalar and gradient of a restate()-shaped result, flat."""
    out = [("loss", res["loss"]), ("value_loss", res["value_loss"]), ("entropy", res["entropy"]), ("grad_values", res["grad_values"])]
    for g in range(len(res["surrogate"])):
        out += [(f"surrogate[{g}]", res["surrogate"][g]), (f"grad_mu[{g}]", res["grad_mu"][g]), (f"grad_sigma[{g}]", res["grad_sigma"][g])]
        if res["kl"][g] is not None:
            out.append((f"kl[{g}]", res["kl"][g]))
    return out


# The parity rule, in the project's form (tests/test_policy_host.py): |kernel - f64| <= PARITY_FACTOR * max(|torch-CPU-f32 - f64|, one
# float32 ulp of the largest magnitude of that output).  The kernel accumulates every sum in float64, so the sums add nothing: what is
# left is elementwise.  Both float32 sides run the same chain per element -- about a dozen roundings of at most half an ulp, one logf per
# action and one expf per row -- and differ in three ways, each worth a factor 2 at most: (a) the device library's expf / logf are
# specified to 1 ulp where a host libm is within half an ulp to one; (b) the order of the products differs (the kernel forms
# g * r * (1 / B) and multiplies the quad by it, autograd applies its factors one backward node at a time) and the compiler contracts
# a * b + c into one rounding where torch rounds twice; (c) the statistic is a maximum over up to 5e5 elements of two error samples of
# like spread, and the larger maximum of two such samples exceeds the smaller by less than 2 except in a vanishing share of draws.
# Hence 8, the same figure and for the same kind of reasons as the forward-parity rule.  An error below one float32 ulp of the largest
# output is not resolvable and is lifted to it: that floor comes from the number format, not from either implementation.
PARITY_FACTOR = 8.0


def parity_bound(err_f32, ref64):
    return PARITY_FACTOR * max(float(err_f32), float(np.abs(ref64).max()) * 2.0 ** -23)


def max_err(x, ref64):
    return float(np.abs(np.asarray(x, np.float64) - np.asarray(ref64, np.float64)).max())


def check_parity(got, ref64, ref32, label, report=None):
    """Every output of `got` (restate()-shaped) against the rule; prints each figure before it asserts.  Returns [(name, err, bound)]."""
    rows = []
    for (name, x), (_, r64), (_, r32) in zip(outputs(got), outputs(ref64), outputs(ref32)):
        err, err32 = max_err(x, r64), max_err(r32, r64)
        bound = parity_bound(err32, r64)
        rows.append((name, err, err32, bound))
        print(f"{label} {name}: kernel err {err:.3e}, torch-f32 err {err32:.3e}, bound {bound:.3e}, ratio {err / bound if bound else 0.0:.3f}")
    if report is not None:
        report.extend((label, *r) for r in rows)
    for name, err, err32, bound in rows:
        assert np.isfinite(err) and err <= bound, f"{label} {name}: |kernel - f64| = {err:.3e} above {bound:.3e} (torch f32 {err32:.3e})"
    return rows


# ---- the golden fixture (tests/golden/gen_ppo_loss_fixtures.py) ----------------------------------------------------------------------------
def load_fixture(path):
    """{case: dict(cfg=dict(clipped, spo, ent, clip, vlc), inp=<make_inputs-shaped, mu / sigma / values float64>, want=<restate-shaped>,
    desired_kl, lr_after)}.  The student group of the two-group case has no KL in the reference, so its old_mu / old_sigma are left out."""
    z = np.load(path)
    out = {}
    for name in [str(n) for n in z["cases"]]:
        k = lambda key: z[f"{name}.{key}"]
        clipped, spo, ent, clip, vlc, n_groups = k("cfg")
        groups = []
        for gi in range(int(n_groups)):
            g = {key: k(f"g{gi}.{key}") for key in INPUT_KEYS}
            if gi == 1:
                g["old_mu"] = g["old_sigma"] = None
            groups.append(g)
        gs = range(int(n_groups))
        want = dict(loss=k("loss"), surrogate=[k(f"g{g}.surrogate") for g in gs], value_loss=k("value_loss"), entropy=k("entropy"),
                    kl=[None] * int(n_groups), grad_mu=[k(f"g{g}.grad_mu") for g in gs], grad_sigma=[k(f"g{g}.grad_sigma") for g in gs],
                    grad_values=k("grad_values"))
        out[name] = dict(cfg=dict(clipped=bool(clipped), spo=bool(spo), ent=float(ent), clip=float(clip), value_loss_coef=float(vlc)),
                         inp=dict(groups=groups, values=k("values"), returns=k("returns"), target_values=k("target_values")), want=want,
                         desired_kl=k("desired_kl"), lr_after=k("lr_after"))
    return out


def as_float32(inp):
    """The inputs as the kernel takes them: every array float32 (the fixture keeps the double networks' outputs as float64)."""
    f = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float32)
    return dict(groups=[{k: f(v) for k, v in g.items()} for g in inp["groups"]], values=f(inp["values"]), returns=f(inp["returns"]),
                target_values=f(inp["target_values"]))

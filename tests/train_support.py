"""What the train-pass case modules (tests/train_cases.py, tests/train_ee_cases.py, tests/train_ts_cases.py, tests/train_edges.py) share, in
one copy: the plan of csrc/lg_train_pass.h restated (constants, LDS fold, row tile, slice rule, workspace layout), the draws of a case's
layers and clip, the chain arithmetic in numpy (forward, batch sums per slice, the layer-by-layer backward), its torch side, the parity
rule, and the readers of the golden fixtures.  A family's module adds only what is its own: which chains, how they are joined, its
heads.  No test functions here; nothing loads the HIP library."""
import numpy as np
import torch

from tests.optim_cases import PARITY_FACTOR, max_err, parity_bound          # the same bound and error as the optimizer's rule: one copy

# ---- the plan (csrc/lg_train_pass.h, csrc/lg_train_tiles.h), restated ------------------------------------------------------------------------
WG_TILE, MIN_SLICE_ROWS, MAX_SLICES, LDS_BYTES = 64, 64, 32, 160 * 1024
ROW_TILES = (32, 16, 8)


def lds_stride(w):
    return (((((w + 3) & ~3) - 4 + 63) // 64) * 64) + 4


def slice_rule(n_rows, tiles, target_jobs):
    """(slices, rows per slice) of a layer of `tiles` 64 x 64 gradient tiles under a pass's job target."""
    want = min(max(1, n_rows // MIN_SLICE_ROWS), max(1, target_jobs // tiles), MAX_SLICES)
    per = (-(-n_rows // want) + 3) & ~3
    return -(-n_rows // per), per


def lds_widths(chains_first):
    """The two activation buffers' row strides: the widest layer each holds, over (widths, buffer of the chain's input) pairs."""
    w = [0, 0]
    for c, first in chains_first:
        for i, width in enumerate(c):
            w[(i + first) & 1] = max(w[(i + first) & 1], lds_stride(width))
    return w


def row_tile(w, extra=0):
    """(row tile, LDS bytes): the largest tile whose two buffers, and `extra` bytes beside them, fit the LDS; 0 rows if none does."""
    r = next((r for r in ROW_TILES if r * (w[0] + w[1]) * 4 + extra <= LDS_BYTES), 0)
    return r, r * (w[0] + w[1]) * 4 + extra


def offsets(n_rows, chains, off, target_jobs):
    """h_off, g_off, then p_off / slices of the chains, as the plan lays them out from float `off` on; returns (dict, off, jobs)."""
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
            tiles = -(-M // WG_TILE) * -(-K // WG_TILE)
            S, per = slice_rule(n_rows, tiles, target_jobs)
            p.append(off)
            off += S * (M * K + M)
            jobs += S * tiles
            s.append(S)
            r.append(per)
        p_off.append(p)
        slices.append(s)
        rows.append(r)
    return dict(h_off=h_off, g_off=g_off, p_off=p_off, slices=slices, slice_rows=rows), off, jobs


def plan_slices(p):
    """[(slices, rows per slice)] of every layer of a restated plan, chain after chain."""
    return [x for c in zip(p["slices"], p["slice_rows"]) for x in zip(*c)]


def smallest_ragged_b(*plans):
    """The smallest batch at which some layer of some plan (each a function of the batch) gets more than one slice and a last slice shorter
    than the others."""
    for b in range(1, 4096):
        if any(S > 1 and b % per for plan in plans for S, per in plan_slices(plan(b))):
            return b
    raise AssertionError("no ragged batch below 4096")


# ---- draws ----------------------------------------------------------------------------------------------------------------------------------
def case_of(case, cases, nets):
    """(case dict, chains) of a table name or of a case dict, which names its net or carries its `widths` itself."""
    c = cases[case] if isinstance(case, str) else case
    return c, (tuple(list(w) for w in c["widths"]) if "widths" in c else nets[c["net"]])


def draw_layers(rng, widths):
    """[W0, b0, W1, b1, ...] of a chain, float32."""
    out = []
    for li in range(len(widths) - 1):
        out.append((rng.normal(size=(widths[li + 1], widths[li])) * (1.3 / np.sqrt(widths[li]))).astype(np.float32))
        out.append((0.2 * rng.normal(size=widths[li + 1])).astype(np.float32))
    return out


def place_clip(pre):
    """A clip for the pre-clip means `pre` such that a good share of them saturates and none lies within 1e-3 of it, so that no rounding
    moves a mask decision."""
    f = np.float32
    clip = float(f(np.median(np.abs(pre))))
    while np.abs(np.abs(pre) - clip).min() < 1e-3:
        clip = float(f(clip + 2.5e-3))
    return clip


# ---- the chain arithmetic in numpy ----------------------------------------------------------------------------------------------------------
def pairs(ps, dtype):
    return [(np.asarray(ps[i]).astype(dtype), np.asarray(ps[i + 1]).astype(dtype)) for i in range(0, len(ps), 2)]


def mlp(layers, h, dtype):
    """The activations [input, layer 0's output, ...] of a chain: an ELU behind every layer but the last."""
    acts = [h]
    for i, (W, b) in enumerate(layers):
        h = h @ W.T + b
        if i < len(layers) - 1:
            h = np.where(h > 0, h, np.expm1(np.minimum(h, 0))).astype(dtype)
        acts.append(h)
    return acts


def hardtanh(mu, clip, dtype):
    return mu if clip is None else np.where(mu < -clip, -clip, np.where(mu > clip, clip, mu)).astype(dtype)


def masked_grad_mu(g_mu, mu, clip, dtype):
    """grad_mu behind the Hardtanh: zero wherever the clipped mean `mu` sits on the clip."""
    g_mu = np.asarray(g_mu).astype(dtype)
    return g_mu if clip is None else np.where((mu >= clip) | (mu <= -clip), 0, g_mu).astype(dtype)


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


def chain_backward(layers, acts, G, dtype, pers=None, input_grad=False, drop_last=False, elu1=False):
    """The gradients [W0, b0, W1, b1, ...] of one chain from G of its last layer (elu' from the stored output), the batch sums per slice of
    pers[li] rows as the kernel forms them; with input_grad also G through layer 0, with no activation factor.  Planted defects: drop_last,
    every sum without its last slice; elu1, elu' = 1."""
    B, out = G.shape[0], []
    for li in range(len(layers) - 1, -1, -1):
        H, per = acts[li], B if pers is None else int(pers[li])
        out = [slice_sum(per, G, H, drop_last=drop_last), slice_sum(per, G, phases=4, drop_last=drop_last)] + out
        if li:
            d = np.ones_like(H) if elu1 else np.where(H > 0, 1, H + 1)
            G = ((G @ layers[li][0]) * d).astype(dtype)
    return out, ((G @ layers[0][0]).astype(dtype) if input_grad else None)


# ---- the torch side -------------------------------------------------------------------------------------------------------------------------
def mlp_t(h, ps):
    for i in range(0, len(ps), 2):
        h = torch.nn.functional.linear(h, ps[i], ps[i + 1])
        if i < len(ps) - 2:
            h = torch.nn.functional.elu(h)
    return h


def sequential(widths, clip):
    """Linear, ELU, ..., Linear of a chain as the reference builds it, a Hardtanh behind it where there is a clip."""
    nn, mods = torch.nn, []
    for i in range(len(widths) - 1):
        mods.append(nn.Linear(widths[i], widths[i + 1]))
        if i < len(widths) - 2:
            mods.append(nn.ELU())
    if clip is not None:
        mods.append(nn.Hardtanh(-clip, clip))
    return nn.Sequential(*mods)


def set_parameters(params, values, dtype):
    with torch.no_grad():
        for p, v in zip(params, values):
            p.copy_(torch.as_tensor(np.asarray(v)).to(dtype))


# ---- the parity rule ------------------------------------------------------------------------------------------------------------------------
# Per tensor (mu, sigma, values, a pass's loss and every parameter gradient): |kernel - f64| <= PARITY_FACTOR * max(|torch-CPU-f32 - f64|,
# one float32 ulp of that tensor's largest magnitude), both sides on the same float32 inputs: the rule of tests/optim_cases.py, whose
# factor 8 comes from the number formats.  Here the two float32 evaluations differ in (a) the order of every dot product (the MFMA's k
# permutation and the batch slices against torch's blocked GEMM), each side a sum of the same products with roundings of at most half an
# ulp of its partial sums: one side at most twice the other; (b) expm1f and elu' = h + 1 against torch's exp: one rounding more on one
# side, a factor 2 on the share of the error that passes an ELU; (c) the statistic is a maximum over the elements of two error samples
# of like spread, a factor 2 except in a vanishing share of draws.
CLASSES = ("outputs", "loss", "grad_weight", "grad_bias", "grad_std")


def tensor_class(name):
    return "outputs" if name in ("mu", "sigma", "values") else "loss" if name == "loss" else "grad_std" if name == "std" else \
        "grad_weight" if name.endswith("weight") else "grad_bias"


def check_parity(got, ref64, ref32, label, report=None, factor=PARITY_FACTOR):
    """got / ref64 / ref32: dict name -> array.  Every tensor of ref64 against |kernel - f64| <= factor * max(|torch-CPU-f32 - f64|, ulp of
    the tensor's largest magnitude), factor = PARITY_FACTOR unless a test holds something to a share of the rule; prints the worst ratio of
    each tensor class, in CLASSES order, before it asserts.  Returns {class: worst |kernel - f64| / max(|f32 - f64|, ulp)}."""
    seen, bad = {}, []
    for name, r64 in ref64.items():
        err, err32 = max_err(got[name], r64), max_err(ref32[name], r64)
        unit = parity_bound(err32, r64) / PARITY_FACTOR
        bound = factor * unit
        ratio = err / unit if unit else (0.0 if err == 0.0 else float("inf"))
        k = tensor_class(name)
        seen[k] = max(seen.get(k, 0.0), ratio if np.isfinite(ratio) else float("inf"))
        if not (np.isfinite(err) and err <= bound):
            bad.append(f"{label} {name}: |kernel - f64| = {err:.3e} above {bound:.3e} (torch f32 {err32:.3e})")
    worst = {k: seen[k] for k in CLASSES if k in seen}
    print(f"{label}: worst |kernel - f64| / max(|f32 - f64|, ulp): " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" (allowed {factor:g})")
    if report is not None:
        report.append((label, worst))
    assert not bad, "\n".join(bad)
    return worst


# ---- the golden fixtures (tests/golden/gen_ppo*_train_fixtures.py) ----------------------------------------------------------------------------
def fixture_shapes(z):
    """(names, name -> shape) of a fixture's parameters."""
    names = [str(n) for n in z["names"]]
    return names, {n: tuple(int(d) for d in s if d) for n, s in zip(names, z["shapes"])}


def split_flat(flat, shapes, order):
    """The arrays named in `order`, cut from one flat vector that holds them back to back."""
    out, at = [], 0
    for n in order:
        size = int(np.prod(shapes[n]))
        out.append(flat[at:at + size].reshape(shapes[n]).copy())
        at += size
    assert at == flat.size
    return out


def chain_widths(names, shapes, chain):
    """[in, out_0, ..., out_last] of the chain whose weights' names start with `chain`."""
    w = [shapes[n] for n in names if n.startswith(chain) and n.endswith("weight")]
    return [s[1] for s in w][:1] + [s[0] for s in w]


def load_two_pass_fixture(path, cfg_keys, chains, second, columns):
    """The fixture of an update of RL steps and steps of a second pass (`second`: "est" or "enc", the prefix of its arrays): dict(names,
    rl_names, <second>_names, shapes (by name), the widths of `chains` (key -> the chain's name), cfg, init, params and <second>_params
    (dicts name -> array, one per step), grads and <second>_grads (lists in rl_names / <second>_names order, one per step), and every
    array of `columns`), float64."""
    z = np.load(path)
    names, shapes = fixture_shapes(z)
    cfg = dict(zip(cfg_keys, (float(v) for v in z["cfg"])))
    for k in ("steps", second + "_steps", second + "_epochs"):
        cfg[k] = int(cfg[k])
    rl, other = [str(n) for n in z["rl_names"]], [str(n) for n in z[second + "_names"]]
    by_name = lambda flat: dict(zip(names, split_flat(flat, shapes, names)))
    out = dict(names=names, rl_names=rl, shapes=shapes, cfg=cfg, init=by_name(z["init"]), params=[by_name(p) for p in z["params"]],
               grads=[split_flat(g, shapes, rl) for g in z["grads"]])
    out.update({second + "_names": other, second + "_params": [by_name(p) for p in z[second + "_params"]],
                second + "_grads": [split_flat(g, shapes, other) for g in z[second + "_grads"]]})
    out.update({key: chain_widths(names, shapes, chain) for key, chain in chains.items()})
    for k in columns:
        out[k] = z[k]
    return out


def fixture_loss_inputs(fx, s, mu, sigma, values):
    """tests/ppo_loss_cases.restate's input for RL step s of a fixture around the given network outputs."""
    g = dict(mu=mu, sigma=sigma, actions=fx["actions"][s], advantages=fx["advantages"][s], old_log_prob=fx["old_log_prob"][s],
             old_mu=fx["old_mu"][s], old_sigma=fx["old_sigma"][s])
    return dict(groups=[g], values=values, returns=fx["returns"][s], target_values=fx["target_values"][s])

"""The edge cases of the fused policy step (csrc/lg_policy.hip) that the workload's own nets do not reach: ONE table of net sets, each row
with the row tile it plans and the kernel paths it is there to reach, and the helpers the two test files on it share --
tests/test_policy_edges_host.py (no GPU: the planned tile, the coverage of the table, the reference's NaN semantics, discrimination) and
tests/test_gpu_policy_edges.py (the kernel against float64).  No test functions here, nothing needs a GPU.

Built on what exists: `mlp`, `StandIn`, `np_forward`, `parity_bound` (the project's factor 8: the tolerance everywhere) and `max_err` of
tests/test_policy_host.py, the stand-in modules and the seeding of tests/test_policy_families_host.py.  The reference is the same torch
module on the CPU in float64; its float32 run supplies the `err_torch_f32` of the parity rule."""
import copy

import numpy as np
import torch
import torch.nn as nn

from tests.test_policy_families_host import VAR_SCALE, StandInDWAQ, _seed
from tests.test_policy_host import StandIn, max_err, mlp, np_forward, parity_bound

LDS_BYTES = 160 * 1024        # csrc/lg_policy.hip: "the largest [R of 32, 16, 8] whose activations fit the 160 KB LDS"
WAVES = 4                     # ... "a workgroup (4 waves)"
WIDE_SIZES = (1, 8, 9, 33)    # against the 8-row tile: a one-row tile, a full one, a full one plus a one-row one, four full ones plus one row
SWEEP_N = 33

# ---- the table ------------------------------------------------------------------------------------------------------------------------------
# kind: "plain" (actor, critic), "ee" (estimator -> actor, critic), "dwaq" (VAE encoder, four heads, reparam -> actor, critic).
# R: the row tile `plan` must choose.  reach: tags of `row_tags` this row is there for; test_policy_edges_host.py verifies each.
# wide8: the LDS strides are 2052 (2047 inputs) + 580 (520 neurons) floats; 16 rows of that are 168 448 B > 160 KB, so R = 8.
# wide8_ee / wide8_dwaq: the smallest widths that plan 8 -- 1989 = 64 * 31 + 5 is the narrowest activation with stride 2052 and 453 =
# 64 * 7 + 5 the narrowest with stride 516; 2052 + 516 = 2568 floats, 8 more than the 2560 that 16 rows may take.  wide16_ee is wide8_ee
# with ONE neuron less (452: stride 452, 2504 floats): the other side of the threshold, and the table's R = 16 row.
EDGE_NETS = {
    "wide8": dict(kind="plain", obs=2047, actor=[520, 65], A=5, cobs=1301, critic=[193], R=8, sizes=WIDE_SIZES,
                  reach=("R=8", "K%16=15", "K%4!=0", "nt4-ragged", "nt2-ragged", "A%4=1")),
    "wide8_ee": dict(kind="ee", obs=1978, est=([21], 11), actor=[453, 40], A=3, cobs=37, critic=[19], R=8, sizes=WIDE_SIZES,
                     reach=("R=8", "cat-col%4!=0", "nt4-ragged", "A%4=3")),
    "wide16_ee": dict(kind="ee", obs=1978, est=([21], 11), actor=[452, 40], A=3, cobs=37, critic=[19], R=16, sizes=(SWEEP_N,),
                      reach=("R=16", "cat-col%4!=0", "nt4-ragged")),
    "wide8_dwaq": dict(kind="dwaq", obs=1984, hist=77, enc=[256], H=18, L=3, E=2, actor=[453, 24], A=7, cobs=37, critic=[19], logvar_clip=5.0,
                       R=8, sizes=WIDE_SIZES, reach=("R=8", "(L+E)%4!=0", "nt4-exact", "nt4-ragged", "A%4=3")),
}
# The width sweep: two-layer chains K -> M -> A (actor) and K' -> M' -> 1 (critic), ELU between.  The two lists are PAIRED, not crossed:
# net i takes (K, M)[i] for the actor and (K, M)[i + 7] for the critic, so every value runs in both kinds of workgroup.  M is also the
# next layer's K.  M covers the NT thresholds 1 -> 2 (64 | 65) and 2 -> 4 (192 | 193) and M < 4.
SWEEP_K = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65)
SWEEP_M = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 80, 192, 193, 208)
SWEEP_A = (1, 3, 4, 5, 12)
for _i, (_k, _m) in enumerate(zip(SWEEP_K, SWEEP_M)):
    _j = (_i + len(SWEEP_K) // 2) % len(SWEEP_K)
    EDGE_NETS[f"sweep_{_k}_{_m}"] = dict(kind="plain", obs=_k, actor=[_m], A=SWEEP_A[_i % len(SWEEP_A)], cobs=SWEEP_K[_j], critic=[SWEEP_M[_j]],
                                         R=32, sizes=(SWEEP_N,), reach=(f"K={_k}", f"M={_m}"))
CASES = [(name, n) for name, d in EDGE_NETS.items() for n in d["sizes"]]


# ---- the launch plan, restated from the words of csrc/lg_policy.hip and include/lgpolicy.h -----------------------------------------------
def lds_stride(w):
    """Row stride of a w-wide activation in LDS: w rounded up to 4 floats, then to the next value that is 4 mod 64."""
    return ((((w + 3) & ~3) - 4 + 63) // 64) * 64 + 4


def sequences(d):
    """The activation widths each workgroup kind walks, in order; activation i lives in buffer i & 1.  The estimator's output lands in the
    actor's input activation (obs | labels); DreamWaQ's four heads share one activation (2L + 2E) and `reparam` forms (obs | z | vel)."""
    critic = [d["cobs"], *d["critic"], 1]
    if d["kind"] == "ee":
        return [[d["obs"], *d["est"][0], d["obs"] + d["est"][1], *d["actor"], d["A"]], critic]
    if d["kind"] == "dwaq":
        W = d["L"] + d["E"]
        return [[d["hist"], *d["enc"], d["H"], 2 * W, d["obs"] + W, *d["actor"], d["A"]], critic]
    return [[d["obs"], *d["actor"], d["A"]], critic]


def buffer_strides(seqs):
    """Row strides of the two LDS buffers for these sequences of activation widths: each as wide as the widest activation it holds."""
    w = [0, 0]
    for seq in seqs:
        for i, width in enumerate(seq):
            w[i & 1] = max(w[i & 1], lds_stride(width))
    return w


def tile_of(seqs):
    """The largest R of 32, 16, 8 at which the two buffers fit the LDS; 0: none does."""
    w = buffer_strides(seqs)
    return next((R for R in (32, 16, 8) if R * (w[0] + w[1]) * 4 <= LDS_BYTES), 0)


def planned_tile(d):
    return tile_of(sequences(d))


def layers(d):
    """(K, M) of every Linear the launch runs."""
    chain = lambda w: list(zip(w[:-1], w[1:]))
    out = chain([d["cobs"], *d["critic"], 1])
    if d["kind"] == "ee":
        E = d["est"][1]
        return out + chain([d["obs"], *d["est"][0], E]) + chain([d["obs"] + E, *d["actor"], d["A"]])
    if d["kind"] == "dwaq":
        L, E, H = d["L"], d["E"], d["H"]
        return out + chain([d["hist"], *d["enc"], H]) + [(H, L), (H, L), (H, E), (H, E)] + chain([d["obs"] + L + E, *d["actor"], d["A"]])
    return out + chain([d["obs"], *d["actor"], d["A"]])


def neuron_tiles(M):
    """(tiles, NT): 16-neuron tiles of an M-wide layer and how many of them one wave holds: per_wave = ceil(tiles / 4 waves); 4 when that
    is at least 4, 2 when at least 2, otherwise 1."""
    tiles = (M + 15) // 16
    per_wave = (tiles + WAVES - 1) // WAVES
    return tiles, 4 if per_wave >= 4 else 2 if per_wave >= 2 else 1


def layer_tags(K, M):
    """What a K -> M layer reaches.  `ntX-exact`: every neuron of every sweep is real (M a multiple of 16 * NT).  `ntX-ragged`: a wave's last
    sweep holds a tile index past `tiles` (NT = 2, 4: the neuron clamp to M - 1 and the suppressed store) or, for NT = 1, a partial tile."""
    tiles, nt = neuron_tiles(M)
    t = {f"K={K}", f"M={M}"}
    if M % (16 * nt) == 0:
        t.add(f"nt{nt}-exact")
    if tiles % nt or (nt == 1 and M % 16):
        t.add(f"nt{nt}-ragged")
    t |= {tag for tag, on in (("K<4", K < 4), ("K<16", 4 <= K < 16), ("K=16", K == 16), ("K%16=1", K > 16 and K % 16 == 1),
                              ("K%16=15", K > 16 and K % 16 == 15), ("K%4!=0", K % 4 != 0), ("M=1", M == 1)) if on}
    return t


def row_tags(d):
    t = {f"R={planned_tile(d)}", f"A%4={d['A'] % 4}"}
    for K, M in layers(d):
        t |= layer_tags(K, M)
    if d["kind"] == "ee" and d["obs"] % 4:
        t.add("cat-col%4!=0")                      # the estimator's output lands at a column that is no multiple of 4
    if d["kind"] == "dwaq" and (d["L"] + d["E"]) % 4:
        t.add("(L+E)%4!=0")
    return t


# ---- modules, inputs, references ---------------------------------------------------------------------------------------------------------------
def make_plain(d, clip=None, seed=3):
    """A plain or explicit-estimator stand-in from a dict of widths, with the weights of tests/test_policy_host.py::make_net."""
    E = d["est"][1] if d.get("est") else 0
    est = mlp(d["obs"], d["est"][0], E) if E else None
    m = StandIn(mlp(d["obs"] + E, d["actor"], d["A"], nn.Hardtanh(-clip, clip) if clip is not None else None), mlp(d["cobs"], d["critic"], 1),
                torch.ones(d["A"]), est)
    return _seed(m, d["A"], seed)


def make_edge(name, clip=None, seed=3):
    d = EDGE_NETS[name]
    if d["kind"] != "dwaq":
        return make_plain(d, clip, seed)
    m = _seed(StandInDWAQ(d, clip), d["A"], seed)
    with torch.no_grad():                                   # as tests/test_policy_families_host.py::make_dwaq: log-variances on both sides of the clip
        for head in (m.vae.latent_var[0], m.vae.vel_var[0]):
            head.weight.mul_(VAR_SCALE)
            head.bias.mul_(VAR_SCALE)
            head.weight[1::2].neg_()
            head.bias[1::2].neg_()
    return m


def _np(d):
    return {k: v.numpy() for k, v in d.items()}


def forward_all(m, x, eps=None):
    """Every output the kernel reports for module `m` on the inputs `x` (a dict), as torch computes it in x's dtype."""
    if hasattr(m, "vae"):
        out = m.forward_all(x["obs"], x["hist"], eps)
    else:
        out = dict(mu=m.mean(x["obs"]))
        if hasattr(m, "estimator"):
            out["labels"] = m.estimator(x["obs"])
    out["values"] = m.critic(x["cobs"])
    return out


def seeded_inputs(widths, n, seed=11):
    """Seeded randn matrices; no two rows and no two columns of any of them are equal, so a duplicated row or neuron cannot pass."""
    g = torch.Generator().manual_seed(seed)
    x = {k: torch.randn(n, w, generator=g) for k, w in widths.items()}
    for k, v in x.items():
        a = v.numpy()
        assert np.unique(a, axis=0).shape == a.shape and np.unique(a, axis=1).shape == a.shape, k
    return x


_CASES = {}


def edge_case(name, clip=None):
    """Per table row (and clip), computed once, shared and left unchanged: the module, seeded inputs for the largest N of the row, and the
    float64 / float32 CPU results."""
    if (name, clip) not in _CASES:
        d = EDGE_NETS[name]
        m = make_edge(name, clip)
        n = max(d["sizes"])
        widths = dict(obs=d["obs"], cobs=d["cobs"], noise=d["A"])
        if d["kind"] == "dwaq":
            widths.update(hist=d["hist"], eps=d["L"] + d["E"])
        x = seeded_inputs(widths, n)
        noise, eps = x.pop("noise"), x.pop("eps", None)
        m64 = copy.deepcopy(m).double()
        with torch.no_grad():
            ref = _np(forward_all(m64, {k: v.double() for k, v in x.items()}, None if eps is None else eps.double()))
            f32 = _np(forward_all(m, x, eps))
        _CASES[name, clip] = dict(module=m, ref=ref, f32=f32, noise=noise, eps=eps, **x)
    return _CASES[name, clip]


def check_parity(tag, got, c, key, n):
    """The project's rule on rows [0, n) of output `key`, printed in the `parity ...` line format before it is asserted."""
    ref, f32 = c["ref"][key][:n], c["f32"][key][:n]
    ek, et = max_err(np.asarray(got), ref), max_err(f32, ref)
    print(f"parity {tag} {key}: kernel {ek:.3e} torch-f32 {et:.3e} ratio {ek / max(et, 1e-30):.2f} bound {parity_bound(et, ref):.3e} max|ref| {np.abs(ref).max():.3e}")
    assert ek <= parity_bound(et, ref), (tag, key, ek, et)


def torch_act(m, mu, z):
    """What PPO.act reads off the module once the mean is known (actor_critic.py: Normal(mean, mean * 0 + std) with argument validation
    off, as the reference sets it): sigma, actions = mu + sigma z, and the summed log-prob."""
    sigma = mu * 0.0 + m.std
    actions = mu + sigma * z
    lp = torch.distributions.Normal(mu, sigma, validate_args=False).log_prob(actions).sum(-1, keepdim=True)
    return dict(mu=mu, sigma=sigma, actions=actions, log_prob=lp)


# ---- deliberately wrong restatements (float32 numpy): what the 8-row tile and the ragged sweep could get wrong ---------------------------------
def np_dup_rows(seq, x):
    """`np_forward` with row 7 of every 16-row block copied into its rows 8 .. 15: the clamped fragment rows of the 8-row tile, stored."""
    y = np_forward(seq, x).copy()
    for b in range(0, y.shape[0] - 8, 16):
        y[b + 8:b + 16] = y[b + 7]
    return y


def np_drop_ragged_tile(seq, x):
    """`np_forward` in which a layer whose waves end on a ragged sweep (tiles % NT != 0) never stores its last neuron tile: zeros there."""
    mods, x, dropped = list(seq), np.asarray(x, np.float32), 0
    for i, m in enumerate(mods):
        if not isinstance(m, nn.Linear):
            continue
        x = np_forward(mods[i:i + 2] if i + 1 < len(mods) and not isinstance(mods[i + 1], nn.Linear) else [m], x)
        tiles, nt = neuron_tiles(m.out_features)
        if tiles % nt:
            x = x.copy()
            x[:, (tiles - 1) * 16:] = 0.0
            dropped += 1
    assert dropped, "no layer of this chain has a ragged sweep"
    return x

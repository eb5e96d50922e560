"""The edge cases of the fused PPO loss head (csrc/lg_ppo.hip) that tests/ppo_loss_cases.py's table does not reach, and the helpers the two
test files on them share -- tests/test_ppo_loss_edges_host.py (no GPU: the plan, the coverage, that every hand-built row is what its name
says) and tests/test_gpu_ppo_loss_edges.py (the kernel).  Four parts: (A) row widths up to LG_PPO_MAX_ACTIONS and a two-group call of more
than one sweep; (B) rows built by hand ON the places where the gradient selectors' branches meet, and rows where float32 over- or
underflows; (C) one NaN at a time in each of the ten input tensors, with the outputs it must and must not reach; (D) clip_param other
than 0.2.  No test functions here, nothing loads the HIP library.

Built on tests/ppo_loss_cases.py: `make_inputs`, `restate`, the parity rule (PARITY_FACTOR = 8: the only tolerance anywhere here)."""
import copy
import math

import numpy as np
import torch

from tests import ppo_loss_cases as pc

THREADS, MAX_BLOCKS, SLOTS = 256, 512, 6          # include/lgppo.h; tests/test_ppo_loss_host.py pins abi's copies to the header

# ---- A. widths and sweeps ---------------------------------------------------------------------------------------------------------------------
# make_inputs-style cases (passed as dicts).  L = lanes per row, the power of two >= ceil(A / 4); every last policy tile is ragged but w64's,
# which is exactly full.
WIDTH_CASES = {
    "w2":            dict(rows=[129], vrows=129, A=2, clipped=True, spo=False, ent=0.01, kl=[True], seed=31),               # L 1, 256 rows / tile
    "w8":            dict(rows=[129], vrows=1, A=8, clipped=False, spo=True, ent=0.0, kl=[True], seed=32),                  # L 2, 128
    "w16":           dict(rows=[65], vrows=65, A=16, clipped=True, spo=False, ent=0.01, kl=[True], seed=33),                # L 4, 64
    "w17":           dict(rows=[33], vrows=33, A=17, clipped=True, spo=False, ent=0.0, kl=[True], seed=34),                 # L 8, 32
    "w29":           dict(rows=[1], vrows=300, A=29, clipped=False, spo=False, ent=0.01, kl=[True], seed=35),               # L 8, 32
    "w32":           dict(rows=[97], vrows=97, A=32, clipped=True, spo=True, ent=0.01, kl=[True], seed=36),                 # L 8, 32
    "w33":           dict(rows=[17], vrows=17, A=33, clipped=True, spo=False, ent=0.01, kl=[True], seed=37),                # L 16, 16
    "w48":           dict(rows=[49], vrows=49, A=48, clipped=False, spo=True, ent=0.0, kl=[True], seed=38),                 # L 16, 16
    "w63":           dict(rows=[31], vrows=31, A=63, clipped=True, spo=False, ent=0.01, kl=[True], seed=39),                # L 16, 16
    "w64":           dict(rows=[16], vrows=16, A=64, clipped=True, spo=False, ent=0.0, kl=[True], seed=40),                 # L 16, 16
    "cts_w64":       dict(rows=[17, 3], vrows=20, A=64, clipped=True, spo=False, ent=0.01, kl=[True, False], seed=41),
    "cts_sweep_w64": dict(rows=[4100, 4099], vrows=8199, A=64, clipped=True, spo=False, ent=0.01, kl=[True, True], seed=42),  # 547 tiles
}
SWEEP = "cts_sweep_w64"
STRIDED = ("w17", "w33", "w63")          # the 16-byte quad path and the scalar tail, unaligned, at L = 8 and 16


def cfg(c):
    """The keyword arguments of `restate` and of the GPU test's `run` for a case dict."""
    out = dict(clipped=c["clipped"], spo=c["spo"], ent=c["ent"])
    if "clip" in c:
        out["clip"] = c["clip"]
    if "value_loss_coef" in c:
        out["value_loss_coef"] = c["value_loss_coef"]
    return out


def plan(c):
    """include/lgppo.h's launch plan in its own words: lanes per row, rows per tile, the tile number behind each group, workgroups."""
    lanes = 1
    while lanes < (c["A"] + 3) // 4:
        lanes *= 2
    per_tile = THREADS // lanes
    ends, t = [], 0
    for b in c["rows"]:
        t += (b + per_tile - 1) // per_tile
        ends.append(t)
    tiles = t + (c["vrows"] + THREADS - 1) // THREADS
    return dict(lanes=lanes, per_tile=per_tile, ends=ends, tiles=tiles, blocks=min(tiles, MAX_BLOCKS))


def kinds_of_workgroup(c, b):
    """The kinds of tile workgroup b sweeps, in order: 0 / 1 for the policy groups, "v" for the value group."""
    p = plan(c)
    return [next((g for g, e in enumerate(p["ends"]) if t < e), "v") for t in range(b, p["tiles"], p["blocks"])]


def take_rows(inp, rows, value_rows=None, group=0):
    """A one-group make_inputs-shaped dict of the given rows of `group` (an index array: a permutation, a subset) and value rows."""
    g = {k: None if v is None else np.ascontiguousarray(v[rows]) for k, v in inp["groups"][group].items()}
    vr = rows if value_rows is None else value_rows
    return dict(groups=[g], **{k: np.ascontiguousarray(inp[k][vr]) for k in ("values", "returns", "target_values")})


# ---- B. ties, boundaries, overflow: clip_param = 0.25, so (float)(1 +- eps), +-(float)eps and (float)(2 eps) are exact --------------------------
TIE_CLIP = 0.25
HALF_LOG_2PI = np.float32(0.5 * math.log(2 * math.pi))
# |a - mu| of the A = 13 rows, column 0 and the twelve others: with sigma = 1 the column's log-prob term -(d * d) / 2 - 0 - 0.9189385f
# rounds to -1.0f exactly (two of eight neighbouring floats that do), so a float32 log-prob is -13 in any order of summation; and the
# float64 sum of the thirteen floats -(d * d) / 2 is within 2.1e-9 of -13 (1 - 0.5 log 2 pi), so the kernel's log-prob (float64 sums, the
# constant in float64) is -13 to less than 2^-26: ratio == 1.0f on both sides.  tests/test_ppo_loss_edges_host.py asserts both.
UNIT_D = (np.float32(float.fromhex("0x1.9c4ef2p-2")), np.float32(float.fromhex("0x1.9c4ef4p-2")))
INF = float("inf")

# name, v, v_t, R, arm of the value selector, d term / d v (before the coef / B factor; None: the arm alone is pinned)
VALUE_ROWS = [
    ("tie outside",           1.0,   0.0,   0.625, "tie outside",     0.375),       # l1 == l2 = 0.140625: half of 2 (v - R), the clipped half gives 0
    ("tie inside",            0.125, 0.0,   3.0,   "tie inside",     -5.75),        # 2 (v - R)
    ("step == +eps",          0.25,  0.0,   1.0,   "tie inside",     -1.5),         # the closed interval: 2 (v - R)
    ("step == -eps",         -0.25,  0.0,   1.0,   "tie inside",     -2.5),
    ("clipped wins",          1.0,   0.0,   0.75,  "l2 > l1 outside", 0.0),         # l1 = 0.0625 < l2 = 0.25
    ("unclipped wins",        1.0,   0.0,   0.5,   "l1 > l2",         1.0),         # l1 = 0.25 > l2 = 0.0625
    ("rounded up inside",     0.1,   0.017, 0.0,   "l2 > l1 inside",  None),        # v_t + (v - v_t) is one ulp above v: the clipped operand wins INSIDE
    ("rounded down inside",   0.1,   0.013, 0.0,   "l1 > l2",         None),        # ... one ulp below
]
VALUE_OVERFLOW_ROWS = [
    ("v_t = +inf",            1.0,   INF,   0.0,   "l2 > l1 outside", 0.0),         # the clipped operand wins at inf and passes nothing
    ("R = +inf",              1.0,   0.0,   INF,   "tie outside",    -INF),
]
# name, Adv, log of the ratio (logp - old_log_prob, placed exactly), arm of the PPO selector
POLICY_ROWS = [
    ("ratio == 1, Adv = +1",  1.0,  0.0,               "tie inside"),
    ("ratio == 1, Adv = -1", -1.0,  0.0,               "tie inside"),
    ("Adv = +0, inside",      0.0,  math.log(1.125),   "tie inside"),
    ("Adv = -0, inside",     -0.0,  math.log(0.875),   "tie inside"),
    ("Adv = +0, outside",     0.0,  math.log(2.0),     "tie outside"),              # -0 * r == -0 * clamp(r): the only finite tie outside
    ("Adv = -0, outside",    -0.0,  math.log(0.5),     "tie outside"),
    ("inside, Adv = +1",      1.0,  math.log(1.125),   "tie inside"),
    ("inside, Adv = -1",     -1.0,  math.log(0.875),   "tie inside"),
    ("above, Adv = +1",       1.0,  math.log(2.0),     "s2 > s1"),
    ("above, Adv = -1",      -1.0,  math.log(2.0),     "s1 > s2"),
    ("below, Adv = +1",       1.0,  math.log(0.5),     "s1 > s2"),
    ("below, Adv = -1",      -1.0,  math.log(0.5),     "s2 > s1"),
]
# +100 and -200 and nothing closer: far from float32's overflow (88.7) and flush (-103.3) thresholds, so every expf agrees on inf and 0
POLICY_OVERFLOW_ROWS = [
    ("expf = inf, Adv = +1",  1.0,  100.0,             "s2 > s1"),                  # term -1.25, 0 * inf in the gradient
    ("expf = inf, Adv = -1", -1.0,  100.0,             "s1 > s2"),
    ("expf = 0, Adv = +1",    1.0, -200.0,             "s1 > s2"),                  # -0 > -0.75
    ("expf = 0, Adv = -1",   -1.0, -200.0,             "s2 > s1"),
    ("Adv = +inf, above",     INF,  math.log(2.0),     "tie outside"),
    ("Adv = -inf, above",    -INF,  math.log(2.0),     "tie outside"),
    ("Adv = +inf, below",     INF,  math.log(0.5),     "tie outside"),
    ("Adv = -inf, below",    -INF,  math.log(0.5),     "tie outside"),
    ("Adv = 3e38, above",     3e38, math.log(2.0),     "tie outside"),              # both operands overflow to -inf
]
TIE_WIDTHS = (1, 13)
POLICY_ARMS = ("s1 > s2", "s2 > s1", "tie inside", "tie outside", "nan")
VALUE_ARMS = ("l1 > l2", "l2 > l1 inside", "l2 > l1 outside", "tie inside", "tie outside", "nan")


def tie_inputs(A, overflow=False):
    """The hand-built rows as a one-group make_inputs-shaped dict.  A = 1: sigma = 1 and actions = mu, so the log-prob is the one float
    -0.9189385; A = 13: mu = 0, sigma = 1, actions = +-UNIT_D, so it is -13 (see UNIT_D).  old_log_prob = (float)(logp - log ratio) places the ratio."""
    f = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    rows = POLICY_OVERFLOW_ROWS if overflow else POLICY_ROWS
    vals = VALUE_OVERFLOW_ROWS if overflow else VALUE_ROWS
    B = len(rows)
    if A == 1:
        mu, logp = np.full((B, 1), 0.375), np.float32(-HALF_LOG_2PI)
        actions = mu.copy()
    else:
        assert A == 13
        mu, logp = np.zeros((B, A)), np.float32(-13.0)
        size = np.where(np.arange(A) == 0, np.float64(UNIT_D[0]), np.float64(UNIT_D[1]))
        actions = np.tile(np.where(np.arange(A) % 2 == 0, 1.0, -1.0) * size, (B, 1))
    sigma = np.ones((B, A))
    old_lp = f([np.float64(logp) - r[2] for r in rows]).reshape(B, 1)
    g = dict(mu=f(mu), sigma=f(sigma), actions=f(actions), old_log_prob=old_lp, advantages=f([r[1] for r in rows]).reshape(B, 1),
             old_mu=f(mu + 0.125), old_sigma=f(sigma * 1.25))
    col = lambda i: f([r[i] for r in vals]).reshape(len(vals), 1)
    return dict(groups=[g], values=col(1), target_values=col(2), returns=col(3))


def policy_arm(g, clip):
    """The arm of the kernel's PPO selector each row of group dict `g` takes, evaluated in torch float32 on the CPU: one of POLICY_ARMS;
    also the float32 ratios."""
    t = lambda x: torch.from_numpy(np.asarray(x, np.float32))
    mu, sigma, a = t(g["mu"]), t(g["sigma"]), t(g["actions"])
    logp = (-(a - mu) ** 2 / (2 * sigma ** 2) - torch.log(sigma) - 0.5 * math.log(2 * math.pi)).sum(-1)
    r = torch.exp(logp - t(g["old_log_prob"]).reshape(-1))
    adv = t(g["advantages"]).reshape(-1)
    s1, s2 = -adv * r, -adv * torch.clamp(r, 1.0 - clip, 1.0 + clip)
    inside = (r >= 1.0 - clip) & (r <= 1.0 + clip)
    arms = []
    for i in range(len(r)):
        if s1[i] > s2[i]:
            arms.append("s1 > s2")
        elif s2[i] > s1[i]:
            arms.append("s2 > s1")
        elif s1[i] == s2[i]:
            arms.append("tie inside" if inside[i] else "tie outside")
        else:
            arms.append("nan")
    return arms, r.numpy()


def value_arm(values, target_values, returns, clip):
    """Likewise for the clipped value loss: one of VALUE_ARMS per row; also the float32 steps v - v_t."""
    t = lambda x: torch.from_numpy(np.asarray(x, np.float32)).reshape(-1)
    v, vt, R = t(values), t(target_values), t(returns)
    d = v - vt
    vc = vt + d.clamp(-clip, clip)
    l1, l2 = (v - R) ** 2, (vc - R) ** 2
    inside = (d >= -clip) & (d <= clip)
    arms = []
    for i in range(len(v)):
        where = " inside" if inside[i] else " outside"
        if l1[i] > l2[i]:
            arms.append("l1 > l2")
        elif l2[i] > l1[i]:
            arms.append("l2 > l1" + where)
        elif l1[i] == l2[i]:
            arms.append("tie" + where)
        else:
            arms.append("nan")
    return arms, d.numpy()


def pattern(x):
    """The non-finite pattern of an array, element by element: 0 finite, 1 +inf, 2 -inf, 3 NaN."""
    x = np.asarray(x, np.float64)
    return np.where(np.isnan(x), 3, np.where(np.isposinf(x), 1, np.where(np.isneginf(x), 2, 0)))


# ---- C. one NaN at a time -----------------------------------------------------------------------------------------------------------------------
GROUP_TENSORS = ("mu", "sigma", "actions", "old_log_prob", "advantages", "old_mu", "old_sigma")
VALUE_TENSORS = ("values", "returns", "target_values")
# base name -> (case, group that takes the NaN).  The two-group base hands the kernel group 1's old_mu / old_sigma only when the NaN goes
# there (the reference's CTS has no student KL): the draws are the same either way.
NAN_BASES = {"b257_a12": (pc.CASES["b257_a12"], 0), "w33": (WIDTH_CASES["w33"], 0), "cts_17_5": (pc.CASES["cts_17_5"], 1)}


def nan_case(base, tensor):
    c, group = NAN_BASES[base]
    if tensor in ("old_mu", "old_sigma") and not c["kl"][group]:
        c = dict(c, kl=[True] * len(c["rows"]))
    return c, group


def nan_places(c, group, tensor):
    """(row, column) of the three places: a middle row, the last row (of the ragged last tile), the last action column (the scalar-tail
    quad where A is not a multiple of 4).  A column tensor has the two rows."""
    B = c["vrows"] if tensor in VALUE_TENSORS else c["rows"][group]
    mid, last = B // 2, B - 1
    if tensor in VALUE_TENSORS or tensor in ("old_log_prob", "advantages"):
        return [(mid, 0), (last, 0)]
    return [(mid, 1), (last, c["A"] // 2), (B // 3, c["A"] - 1)]


def with_nan(inp, group, tensor, row, col):
    bad = copy.deepcopy(inp)
    (bad if tensor in VALUE_TENSORS else bad["groups"][group])[tensor][row, col] = np.nan
    return bad


def nan_reach(tensor, group, has_kl, clipped):
    """include/lgppo.h's "a NaN in a row reaches that row's gradients and every scalar the row feeds, and nothing else", per input tensor:
    (names of `outputs()` scalars that turn NaN, gradient arrays whose one row turns NaN).  Everything else keeps its bits."""
    sur, kl = f"surrogate[{group}]", [f"kl[{group}]"] if has_kl else []
    pol = [f"grad_mu[{group}]", f"grad_sigma[{group}]"]
    if tensor == "mu":
        return ["loss", sur] + kl, pol
    if tensor == "actions":                                     # the KL does not read the actions
        return ["loss", sur], pol
    if tensor == "sigma":
        return ["loss", sur, "entropy"] + kl, pol
    if tensor in ("old_log_prob", "advantages"):
        return ["loss", sur], pol
    if tensor in ("old_mu", "old_sigma"):
        return kl, []
    if tensor in ("values", "returns") or (tensor == "target_values" and clipped):
        return ["loss", "value_loss"], ["grad_values"]
    assert tensor == "target_values"
    return [], []                                               # the unclipped value loss does not read the column


# ---- D. other clip values -------------------------------------------------------------------------------------------------------------------------
CLIP_BASES = {"b257_a12": pc.CASES["b257_a12"], "b257_a12_spo": pc.CASES["b257_a12_spo"], "w33": WIDTH_CASES["w33"]}
CLIP_POINTS = tuple((clip, vlc) for clip in (0.1, 0.3) for vlc in (0.5, 2.0))              # (clip_param, value_loss_coef)
CLIP_CASES = {f"{name}_clip{clip}_vlc{vlc}": dict(c, clip=clip, value_loss_coef=vlc) for name, c in CLIP_BASES.items() for clip, vlc in CLIP_POINTS}

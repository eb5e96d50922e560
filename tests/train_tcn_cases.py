"""The cases of the TCN history-encoder pass (include/lgtraintcn.h), shared by tests/test_train_tcn_host.py (CPU) and
tests/test_gpu_train_tcn.py (GPU): one case table, the input generator, the pass restated in numpy (float64: the reference of every
comparison; float32 in the kernels' order of sums: the twin), the same pass as torch autograd on the CPU, the plan restated, the module
the GPU file hands to FusedTrainPassTSTcn and the loader of the golden fixture (tests/golden/gen_ppo_ts_tcn_train_fixtures.py).  The chain
arithmetic, the plan rules it shares with the other passes and the parity rule are tests/train_support.py's.  Nothing here loads the HIP
library."""
import numpy as np
import torch

from tests import train_support as sup

MAX_CONV, MAX_CHANNELS, MAX_KERNEL, MAX_STRIDE, MAX_DILATION, MAX_WIDTH = 6, 32, 9, 4, 8, 2048          # include/lgtraintcn.h's limits
TARGET_JOBS, WG_ELEMS, LANES, MAX_BLOCKS, RED_BYTES = 2048, 8, 32, 2048, 256 * 8
P, O, A, C = 5, 4, 3, 6             # privileged, actor and critic observation widths and actions of every case's other chains


def _pattern(channels, k, strides, dilations):
    """The reference's layer pattern (actor_critic_ts.py:78-88): padding = dilation * (k - 1) // 2."""
    cin = [1] + list(channels[:-1])
    return [(ci, co, k, s, d * (k - 1) // 2, d) for ci, co, s, d in zip(cin, channels, strides, dilations)]


# name -> dict(H, convs = [(c_in, c_out, kernel, stride, padding, dilation)], tail widths [F, ..., Z], B = batches, seed).  What each reaches
# is the table of the issue that asked for this pass: see test_case_table_reaches_the_edges.  The draw of (case, B) is seeded by seed * 1000 + B.
# Re-seeds (`reseed`: B -> seed in place of the case's), made because the float32 twin alone missed HALF the parity rule on the CPU, where
# torch's own float32 error happened to be small: tiny B = 5 (history_encoder.1.bias at 4.20 of the allowed 4), one B = 1 (loss at 4.23), and,
# once the conv sums ran in float64, wide B = 1 (loss at 5.23: the tail's and torch's float32 roundings alone, one row).
CASES = {
    "tiny":   dict(H=6, convs=[(1, 3, 5, 1, 2, 1), (3, 3, 5, 2, 2, 1)], tail=[9, 4, 2], B=(1, 5, 33), seed=1300, reseed={5: 1310}),
    "ref90":  dict(H=90, convs=_pattern([1, 1, 1, 1], 5, [1, 2, 1, 2], [1, 1, 2, 1]), tail=[23, 16, 5], B=(1, 31, 257), seed=1301),
    "go2_ts": dict(H=900, convs=_pattern([1, 1, 1, 1], 5, [1, 2, 1, 2], [1, 1, 2, 1]), tail=[225, 128, 94], B=(129,), seed=1302),
    "wide":   dict(H=40, convs=[(1, 32, 3, 1, 1, 1), (32, 32, 3, 2, 1, 1)], tail=[640, 8, 3], B=(1, 17), seed=1303, reseed={1: 1314}),
    "odd37":  dict(H=37, convs=[(1, 5, 1, 1, 0, 1), (5, 7, 3, 3, 0, 4), (7, 3, 4, 1, 3, 1), (3, 4, 7, 2, 1, 1)], tail=[20, 6, 3], B=(1, 9), seed=1304),
    "skip":   dict(H=9, convs=[(1, 2, 3, 1, 1, 1), (2, 2, 1, 2, 0, 1)], tail=[10, 4, 2], B=(3,), seed=1305),
    "six":    dict(H=64, convs=_pattern([4] * 6, 5, [1, 2, 1, 2, 1, 2], [1, 1, 2, 1, 4, 1]), tail=[32, 8, 3], B=(1, 33), seed=1306),
    "one":    dict(H=5, convs=[(1, 2, 5, 1, 0, 1)], tail=[2, 3, 2], B=(1, 4), seed=1307, reseed={1: 1311}),
    "fmax":   dict(H=256, convs=[(1, 8, 3, 1, 1, 1)], tail=[2048, 4, 2], B=(1, 9), seed=1308),
}
LENGTHS = {"tiny": [6, 6, 3], "ref90": [90, 90, 45, 45, 23], "go2_ts": [900, 900, 450, 450, 225], "wide": [40, 40, 20], "odd37": [37, 37, 10, 13, 5],
           "skip": [9, 9, 5], "six": [64, 64, 32, 32, 16, 16, 8], "one": [5, 1], "fmax": [256, 256]}
ALL = [(name, b) for name, c in CASES.items() for b in c["B"]]
IDS = [f"{name}_b{b}" for name, b in ALL]
# the timing workloads of tools/train_tcn_time.py: the reference's go2_ts TCN settings, and the 8-channel variant
GO2_TS = dict(H=900, convs=_pattern([1, 1, 1, 1], 5, [1, 2, 1, 2], [1, 1, 2, 1]), tail=[225, 128, 94])
GO2_TS_8 = dict(H=900, convs=_pattern([8, 8, 8, 8], 5, [1, 2, 1, 2], [1, 1, 2, 1]), tail=[1800, 128, 94])


def lengths(H, convs):
    """[H, L_1, ..., L_n]: L_l = floor((L_(l-1) + 2 p - d (k - 1) - 1) / s) + 1."""
    out = [H]
    for _, _, k, s, p, d in convs:
        out.append((out[-1] + 2 * p - d * (k - 1) - 1) // s + 1)
    return out


def priv_widths(case):
    c = CASES[case] if isinstance(case, str) else case
    return [P, 8, c["tail"][-1]]


# ---- the plan (include/lgtraintcn.h), restated ------------------------------------------------------------------------------------------------
def conv_slice_rule(n_rows, conv):
    """(slices, rows per slice) of a conv's weight gradient: the shared slice rule with tiles = ceil(E / 8), E = c_out c_in k + c_out."""
    ci, co, k = conv[:3]
    return sup.slice_rule(n_rows, -(-(co * ci * k + co) // WG_ELEMS), TARGET_JOBS)


def restated_plan(n_rows, H, convs, tail, priv):
    L = lengths(H, convs)
    n = len(convs)
    size = [n_rows * convs[l][1] * L[l + 1] for l in range(n)]
    x_off, cg_off, off = [-1], [-1], 0
    for l in range(n):
        x_off.append(off)
        off += size[l]
    for l in range(n):
        cg_off.append(off)
        off += size[l]
    conv_p_off, conv_slices, conv_rows, job0, jobs = [], [], [], [], 0
    for ci, co, k, *_ in convs:
        E = co * ci * k + co
        S, per = conv_slice_rule(n_rows, (ci, co, k))
        conv_p_off.append(off)
        off += S * E
        job0.append(jobs)
        jobs += S * -(-E // WG_ELEMS)
        conv_slices.append(S)
        conv_rows.append(per)
    row_tile, lds_bytes = sup.row_tile(sup.lds_widths(((tail, 0), (priv, 0))), RED_BYTES)
    d, off, wjobs = sup.offsets(n_rows, (tail,), off, TARGET_JOBS)
    gl_off = off
    off += n_rows * tail[-1]
    y_off = off
    off += n_rows * tail[-1]
    off += off & 1
    tiles = -(-n_rows // row_tile)
    blocks = min(n_rows, MAX_BLOCKS)
    block_rows = -(-n_rows // blocks)
    return dict(length=L, flat=convs[-1][1] * L[-1], x_off=x_off, cg_off=cg_off, conv_p_off=conv_p_off, conv_slices=conv_slices, conv_slice_rows=conv_rows,
                conv_job0=job0, conv_jobs=jobs, conv_block_rows=block_rows, conv_blocks=-(-n_rows // block_rows), row_tile=row_tile, lds_bytes=lds_bytes,
                h_off=d["h_off"][0], g_off=d["g_off"][0], p_off=d["p_off"][0], slices=d["slices"][0], slice_rows=d["slice_rows"][0], weight_jobs=wjobs,
                gl_off=gl_off, y_off=y_off, partial_off=off, loss_tiles=tiles, workspace_floats=off + 2 * tiles)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def enc_names(convs, tail):
    """history_encoder.parameters() order under the indices of the Sequential: the convs, the Flatten, Linear / ELU / ... / Linear."""
    at = list(range(len(convs))) + [len(convs) + 1 + 2 * j for j in range(len(tail) - 1)]
    return [f"history_encoder.{i}.{k}" for i in at for k in ("weight", "bias")]


def make_inputs(case, B=None, seed=None):
    """float32 numpy inputs of a case (a name of CASES or a dict of H, convs, tail, seed) at batch B: dict(H, convs, tail, priv, actor, critic
    (widths), enc_params (enc_names order: conv weights are (c_out, c_in, k)), rl_params (actor, critic, privilege encoder, std),
    obs_history, privileged_obs, terminated, obs, critic_obs, upstream).  Row 0 is unmasked and, where B > 1, row 1 masked."""
    c = CASES[case] if isinstance(case, str) else case
    B = c["B"][0] if B is None else B
    seed = c.get("reseed", {}).get(B, c["seed"]) if seed is None else seed
    rng, f = np.random.default_rng(seed * 1000 + B), np.float32
    Z = c["tail"][-1]
    priv, actor, critic = [P, 8, Z], [O + Z, 8, A], [C, 8, 1]
    enc = []
    for ci, co, k, *_ in c["convs"]:
        enc.append((rng.normal(size=(co, ci, k)) * (1.3 / np.sqrt(ci * k))).astype(f))
        enc.append((0.2 * rng.normal(size=co)).astype(f))
    enc += sup.draw_layers(rng, c["tail"])
    term = (rng.random((B, 1)) > 0.3).astype(f)
    term[0, 0] = 1.0                                                  # B = 1: the one row counts
    if B > 1:
        term[1, 0] = 0.0
    return dict(H=c["H"], convs=[tuple(v) for v in c["convs"]], tail=list(c["tail"]), priv=priv, actor=actor, critic=critic, enc_params=enc,
                rl_params=sup.draw_layers(rng, actor) + sup.draw_layers(rng, critic) + sup.draw_layers(rng, priv) + [(0.5 + rng.random(A)).astype(f)],
                obs_history=rng.normal(size=(B, c["H"])).astype(f), privileged_obs=rng.normal(size=(B, P)).astype(f), terminated=term,
                obs=rng.normal(size=(B, O)).astype(f), critic_obs=rng.normal(size=(B, C)).astype(f), upstream=f(0.75), clip=None)


# ---- the restatement --------------------------------------------------------------------------------------------------------------------------
def _taps(Lin, Lout, k, s, p, d):
    """(t, u, valid) of tap k: the input position u = t s + k d - p of every output position t, and whether it lies in the input."""
    t = np.arange(Lout)
    u = t * s + k * d - p
    return t, u, (u >= 0) & (u < Lin)


def conv_forward(x, W, b, conv, dtype, wrong=None):
    """x (B, c_in, L_in) -> (B, c_out, L_out): per output the products tap after tap, input channel after input channel, then the bias: the
    kernel's order.  Taps in the padding contribute 0.  Planted defects: wrong="pad_edge" reads the edge value there; "drop_last" leaves
    the last output position out (at its bias) where (L_in + 2 p - d (k - 1) - 1) % s == 0."""
    ci, co, K, s, p, d = conv
    Lin = x.shape[2]
    Lout = (Lin + 2 * p - d * (K - 1) - 1) // s + 1
    acc = np.zeros((x.shape[0], co, Lout), np.float64)              # the kernel's taps add up in float64, rounded to `dtype` once
    for i in range(ci):
        for k in range(K):
            _, u, ok = _taps(Lin, Lout, k, s, p, d)
            xs = x[:, i, np.clip(u, 0, Lin - 1)]
            if wrong != "pad_edge":
                xs = np.where(ok[None, :], xs, dtype(0))
            acc = acc + W[None, :, i, k, None].astype(np.float64) * xs[:, None, :]
    if wrong == "drop_last" and (Lin + 2 * p - d * (K - 1) - 1) % s == 0:
        acc[:, :, -1] = 0
    return (acc + b[None, :, None].astype(np.float64)).astype(dtype)


def conv_input_grad(G, W, conv, Lin, dtype, wrong=None):
    """G (B, c_out, L_out) -> d loss / d x (B, c_in, L_in): per (i, u) tap after tap, output channel after output channel, over the (t, k)
    with t s + k d - p = u.  Planted defects: wrong="no_dilation" / "no_stride" forget d / s here; "garbage" leaves 1.0 at positions no
    output reads, as a kernel would that scatters into an uninitialised buffer."""
    ci, co, K, s, p, d = conv
    if wrong == "no_dilation":
        d = 1
    Lout = G.shape[2]
    dx = np.zeros((G.shape[0], ci, Lin), np.float64)                # in float64 as the kernel adds them, rounded to `dtype` once
    seen = np.zeros(Lin, bool)
    for k in range(K):
        t, u, ok = _taps(Lin, Lout, k, 1 if wrong == "no_stride" else s, p, d)
        seen[u[ok]] = True
        for o in range(co):
            dx[:, :, u[ok]] = dx[:, :, u[ok]] + W[o, :, k][None, :, None].astype(np.float64) * G[:, o, t[ok]][:, None, :]
    if wrong == "garbage":
        dx[:, :, ~seen] = 1
    return dx.astype(dtype)


def _lane_tree(parts, dtype):
    """parts (..., rows, T) -> (...): lane j = t % 32 adds its positions of a row in order into a row partial of `dtype`, the row partials in
    row order in float64, and the 32 lane sums meet in the kernel's binary tree in float64, rounded to `dtype` once."""
    rows, T = parts.shape[-2:]
    pad = -T % LANES
    a = np.concatenate([parts, np.zeros(parts.shape[:-1] + (pad,), dtype)], axis=-1).reshape(parts.shape[:-1] + ((T + pad) // LANES, LANES))
    a = np.cumsum(a, axis=-2, dtype=dtype)[..., -1, :]                  # (..., rows, 32): a row's partial per lane
    a = np.cumsum(a, axis=-2, dtype=np.float64)[..., -1, :]             # (..., 32): the rows in order
    n = LANES
    while n > 1:
        n //= 2
        a = a[..., :n] + a[..., n:2 * n]
    return a[..., 0].astype(dtype)


def conv_weight_grad(G, x, conv, dtype, per=None, wrong=None):
    """(dW (c_out, c_in, k), db (c_out)) from G (B, c_out, L_out) and the layer's input x (B, c_in, L_in).  per: rows per batch slice, the sums
    in the kernel's order (lanes, rows, tree, slices in slice order); None: plain sums.  Planted defect: wrong="bias_no_t" sums the bias
    gradient over the rows at t = 0 only."""
    ci, co, K, s, p, d = conv
    B, _, Lout = G.shape
    Lin = x.shape[2]
    xs = np.zeros((K, B, ci, Lout), dtype)
    for k in range(K):
        _, u, ok = _taps(Lin, Lout, k, s, p, d)
        xs[k] = np.where(ok[None, None, :], x[:, :, np.clip(u, 0, Lin - 1)], dtype(0))
    Gb = G[:, :, :1] if wrong == "bias_no_t" else G
    if per is None:
        return np.einsum("bot,kbit->oik", G, xs).astype(dtype), Gb.sum((0, 2)).astype(dtype)
    dW, db = None, None
    for r0 in range(0, B, per):
        g, gb = G[r0:r0 + per], Gb[r0:r0 + per]
        prod = (g[None, :, :, None, :] * xs[:, r0:r0 + per, None, :, :]).astype(dtype)          # (k, rows, o, i, t)
        w = _lane_tree(np.moveaxis(prod, 1, -2), dtype).transpose(1, 2, 0)                       # (k, o, i) -> (o, i, k)
        bb = _lane_tree(np.moveaxis(gb, 0, -2), dtype)
        dW, db = (w, bb) if dW is None else ((dW + w).astype(dtype), (db + bb).astype(dtype))
    return dW, db


def split_enc(x, dtype):
    n = len(x["convs"])
    e = [np.asarray(v).astype(dtype) for v in x["enc_params"]]
    return [(e[2 * l], e[2 * l + 1]) for l in range(n)], sup.pairs(e[2 * n:], dtype)


def priv_layers(x, dtype):
    na, nc = 2 * (len(x["actor"]) - 1), 2 * (len(x["critic"]) - 1)
    return sup.pairs(x["rl_params"][na + nc:-1], dtype)


def enc_pass(x, dtype=np.float64, upstream=None, kernel_order=False, wrong=None):
    """dict(loss, f, gl, grads (enc_names order), xs (every x_l), G (every G_l, None for l = 0)) of include/lgtraintcn.h's pass.
    kernel_order: every batch sum in the restated plan's slices and the loss by its row tiles.  `wrong`: one planted defect: those of
    conv_forward, conv_input_grad and conv_weight_grad, "flatten" (position-major), "tail0_elu" (an ELU factor on G_f), "upstream_twice"."""
    convs, tail = split_enc(x, dtype)
    B = np.asarray(x["obs_history"]).shape[0]
    plan = restated_plan(B, x["H"], x["convs"], x["tail"], x["priv"]) if kernel_order else None
    xs = [np.asarray(x["obs_history"]).astype(dtype)[:, None, :]]
    for (W, b), conv in zip(convs, x["convs"]):
        xs.append(conv_forward(xs[-1], W, b, conv, dtype, wrong))
    f = (xs[-1].transpose(0, 2, 1) if wrong == "flatten" else xs[-1]).reshape(B, -1)
    ta = sup.mlp(tail, f, dtype)
    y = sup.mlp(priv_layers(x, dtype), np.asarray(x["privileged_obs"]).astype(dtype), dtype)[-1]
    t = np.asarray(x["terminated"]).astype(dtype)
    with np.errstate(invalid="ignore"):
        d = ((ta[-1] - y) * t).astype(dtype)
    up = dtype(x["upstream"] if upstream is None else upstream)
    if dtype == np.float32:
        gl = (d * t * dtype(2.0 / (dtype(B) * dtype(d.shape[1])))).astype(dtype)
    else:
        gl = 2 * d * t / d.size
    G = (gl * up * (up if wrong == "upstream_twice" else 1)).astype(dtype)
    tail_grads, Gf = sup.chain_backward(tail, ta, G, dtype, plan["slice_rows"] if plan else None, input_grad=True)
    if wrong == "tail0_elu":
        Gf = (Gf * np.where(f > 0, 1, f + 1)).astype(dtype)
    Gs = [None] * len(convs) + [Gf.reshape(xs[-1].shape)]
    for l in range(len(convs) - 1, 0, -1):
        Gs[l] = conv_input_grad(Gs[l + 1], convs[l][0], x["convs"][l], xs[l].shape[2], dtype, wrong)
    grads = []
    for l, conv in enumerate(x["convs"]):
        grads += list(conv_weight_grad(Gs[l + 1], xs[l], conv, dtype, plan["conv_slice_rows"][l] if plan else None, wrong))
    sq = d.astype(np.float64) ** 2
    if plan:
        loss = 0.0
        for r0 in range(0, B, plan["row_tile"]):
            loss = loss + sq[r0:r0 + plan["row_tile"]].sum()
        loss = loss / d.size
    else:
        loss = sq.sum() / d.size
    return dict(loss=dtype(loss) if dtype == np.float32 else loss, f=f, gl=gl, grads=grads + tail_grads, xs=xs, G=Gs)


def torch_pass(x, dtype=torch.float32):
    """The pass as torch computes it on the CPU in `dtype` (nn.functional.conv1d, flatten, the tail, mse_loss on the masked pair, backward
    with the upstream scalar): dict(loss, f, grads), float64 numpy."""
    t = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)
    enc = [t(p).requires_grad_(True) for p in x["enc_params"]]
    n = len(x["convs"])
    h = t(x["obs_history"]).unsqueeze(1)
    for l, (_, _, _, s, p, d) in enumerate(x["convs"]):
        h = torch.nn.functional.conv1d(h, enc[2 * l], enc[2 * l + 1], stride=s, padding=p, dilation=d)
    f = h.flatten(1)
    term = t(x["terminated"])
    with torch.no_grad():
        na, nc = 2 * (len(x["actor"]) - 1), 2 * (len(x["critic"]) - 1)
        target = sup.mlp_t(t(x["privileged_obs"]), [t(p) for p in x["rl_params"][na + nc:-1]])
    loss = torch.nn.functional.mse_loss(sup.mlp_t(f, enc[2 * n:]) * term, target * term)
    (loss * float(x.get("upstream", 1.0))).backward()
    num = lambda v: v.detach().double().numpy().copy()
    return dict(loss=num(loss), f=num(f), grads=[num(p.grad) for p in enc])


def named(x, e):
    """dict name -> array of a pass: loss, f and every gradient under its parameter's name."""
    d = dict(loss=np.asarray(e["loss"], np.float64).reshape(1), f=np.asarray(e["f"]))
    d.update(zip(enc_names(x["convs"], x["tail"]), e["grads"]))
    return d


def references(x):
    """(float64 restatement, torch CPU float32) of a case, as `named` dicts; computed once per case and left unchanged."""
    return named(x, enc_pass(x)), named(x, torch_pass(x))


def check_parity(got, ref64, ref32, label, factor=sup.PARITY_FACTOR):
    """tests/train_support.check_parity, unchanged, on loss, f and every gradient.  f goes in under the name "mu": the rule's report
    classes a tensor by its name, and f is an output of the forward like mu."""
    ren = lambda d: {("mu" if k == "f" else k): v for k, v in d.items()}
    return sup.check_parity(ren(got), ren(ref64), ren(ref32), label, factor=factor)


# ---- the module -------------------------------------------------------------------------------------------------------------------------------
def tcn_sequential(convs, tail):
    nn = torch.nn
    mods = [nn.Conv1d(ci, co, k, stride=s, padding=p, dilation=d) for ci, co, k, s, p, d in convs] + [nn.Flatten()]
    return nn.Sequential(*mods, *sup.sequential(tail, None))


class Module(torch.nn.Module):
    """ActorCriticTS's members with a "TCN" history encoder as FusedTrainPassTSTcn reads them, holding a case's parameters; `mlp_history`:
    an MLP history encoder of these widths instead (the twin of the rollout test)."""

    def __init__(self, x, device="cpu", dtype=torch.float32, mlp_history=None):
        super().__init__()
        self.std = torch.nn.Parameter(torch.zeros(x["actor"][-1]))
        self.privilege_encoder = sup.sequential(x["priv"], None)
        self.history_encoder = tcn_sequential(x["convs"], x["tail"]) if mlp_history is None else sup.sequential(mlp_history, None)
        self.actor, self.critic = sup.sequential(x["actor"], None), sup.sequential(x["critic"], None)
        self.to(device=device, dtype=dtype)
        sup.set_parameters(self.rl_parameters(), x["rl_params"], dtype)
        if mlp_history is None:
            sup.set_parameters(self.encoder_parameters(), x["enc_params"], dtype)

    def rl_parameters(self):
        return list(self.actor.parameters()) + list(self.critic.parameters()) + list(self.privilege_encoder.parameters()) + [self.std]

    def encoder_parameters(self):
        return list(self.history_encoder.parameters())

    def forward(self, obs, privileged_obs, critic_obs):
        mu = self.actor(torch.cat((obs, self.privilege_encoder(privileged_obs)), dim=-1))
        return mu, mu * 0.0 + self.std, self.critic(critic_obs)

    def encoder_loss(self, obs_history, privileged_obs, terminated):
        """ppo_ts.py:174-187 with its TCN branch: the history as (B, 1, H)."""
        with torch.no_grad():
            target = self.privilege_encoder(privileged_obs)
        h = obs_history.unsqueeze(1) if obs_history.dim() == 2 else obs_history
        return torch.nn.functional.mse_loss(self.history_encoder(h) * terminated, target * terminated)


# ---- the golden fixture (tests/golden/gen_ppo_ts_tcn_train_fixtures.py) -----------------------------------------------------------------------
FIXTURE_COLUMNS = ("obs", "privileged_obs", "critic_obs", "actions", "target_values", "advantages", "returns", "old_log_prob", "old_mu", "old_sigma")
ENC_COLUMNS = ("enc_history", "enc_privileged", "enc_terminated")
CFG_KEYS = ("lr0", "beta1", "beta2", "eps", "max_grad_norm", "desired_kl", "steps", "clip_param", "value_loss_coef", "entropy_coef", "encoder_lr",
            "enc_steps", "enc_epochs")
FIXTURE_NET = dict(H=14, convs=[(1, 2, 3, 1, 1, 1), (2, 3, 3, 2, 2, 2)], tail=[21, 4, 3], priv=[5, 8, 4, 3], actor=[10, 16, 8, 3], critic=[9, 16, 8, 1])


def load_fixture(path):
    """tests/train_support.load_two_pass_fixture's dict of the reference's PPO_TS.update() on the TCN module: priv / actor / critic widths,
    the conv shapes (c_out, c_in, k) and the tail's widths read from the stored shapes, and the arrays ppo_ts_train.npz has."""
    chains = dict(priv="privilege_encoder", actor="actor", critic="critic")
    fx = sup.load_two_pass_fixture(path, CFG_KEYS, chains, "enc", FIXTURE_COLUMNS + ENC_COLUMNS + (
        "mu", "sigma", "values", "loss", "kl", "lr", "grad_norm", "enc_loss", "enc_grad_norm"))
    w = [fx["shapes"][n] for n in fx["enc_names"] if n.endswith("weight")]
    fx["conv_shapes"] = [s for s in w if len(s) == 3]
    lin = [s for s in w if len(s) == 2]
    fx["tail"] = [lin[0][1]] + [s[0] for s in lin]
    return fx


def fixture_inputs(fx, params, rl_step=None, enc_step=None):
    """The inputs of one step of the fixture around `params` (name -> array), as make_inputs shapes them, float64.  The conv settings
    the arrays do not hold (stride, padding, dilation) are FIXTURE_NET's, checked against the stored shapes by the host file."""
    x = dict(FIXTURE_NET, clip=None, rl_params=[params[n] for n in fx["rl_names"]], enc_params=[params[n] for n in fx["enc_names"]], upstream=1.0)
    if rl_step is not None:
        x.update(obs=fx["obs"][rl_step], privileged_obs=fx["privileged_obs"][rl_step], critic_obs=fx["critic_obs"][rl_step])
    if enc_step is not None:
        x.update(obs_history=fx["enc_history"][enc_step], privileged_obs=fx["enc_privileged"][enc_step], terminated=fx["enc_terminated"][enc_step])
    return x

"""The case table of the recurrent learner pass (include/lgtrainrnn.h, csrc/lg_train_rnn.hip) and its arithmetic restated in numpy: the
trajectory split, the sequence forward of an LSTM / GRU of one or two layers over the padded trajectories, the unpadding, the two MLPs and
the whole backward, in float64 (the oracle of the host tests, pinned to torch's own nn.LSTM / nn.GRU + autograd there) and in float32 with
the batch sums per slice in slice order as the kernels form them.  The chain arithmetic, slice_sum, the plan rules and check_parity are
tests/train_support.py's.  No test functions here; nothing loads the HIP library."""
import numpy as np
import torch

from tests import train_support as ts

TARGET_JOBS, MAX_LAYERS, MAX_HIDDEN = 2048, 2, 512
GATES = dict(lstm=4, gru=3)
RNN_PARAMS = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
DEFECTS = ("gate_order", "no_dh_carry", "no_dc_carry", "whh_uses_ht", "zero_start", "padded_step", "bhn_without_r", "z_swapped", "layer1_old_h",
           "traj_major_rows")

# kind, layers, H; T steps of E envs; dones: "none", "last" (the last step only), "every" (env 1 % E at every step), "short" (every env once
# in the middle and nowhere else, so that every trajectory is short and max_len < T), or a number of further dones drawn before the last step;
# obs / critic obs widths; the hidden widths of the two MLPs; clip: a Hardtanh behind the actor; first: the padded tensors are views
# [:, first:first + n_traj] of a wider padded set; shared: memory_c is handed memory_a's start states (the same objects).
# critic_mem=(layers, H): memory_c's own depth and width (tests/train_rnn_edges.py); without it memory_c has memory_a's.  obs_scale: a factor on
# both observations (the same file's saturated rows).  A case without either draws what it drew before they existed.
# The time loop's tile is 32 trajectories below H = 128: n_traj = E + dones is 31, 32, 33 in the first three; 8 at H = 512: 9 there.
CASES = {
    "lstm1_h7_t6":      dict(kind="lstm", layers=1, H=7, T=6, E=27, dones=4, obs=(11, 13), actor=(24, 10), critic=(20,), clip=True, seed=1),
    "gru1_h17_t6":      dict(kind="gru", layers=1, H=17, T=6, E=28, dones=4, obs=(11, 13), actor=(24, 10), critic=(20,), clip=True, seed=2),
    "lstm2_h64_t6":     dict(kind="lstm", layers=2, H=64, T=6, E=29, dones=4, obs=(11, 13), actor=(24,), critic=(20, 9), clip=True, first=3, shared=True, seed=3),
    "gru2_h65_t2":      dict(kind="gru", layers=2, H=65, T=2, E=30, dones=3, obs=(5, 17), actor=(24, 10), critic=(20,), clip=False, first=2, seed=4),
    "lstm1_h65_t1":     dict(kind="lstm", layers=1, H=65, T=1, E=5, dones="none", obs=(11, 13), actor=(), critic=(20,), clip=False, seed=5),
    "gru1_h7_none":     dict(kind="gru", layers=1, H=7, T=6, E=9, dones="none", obs=(11, 13), actor=(24, 10), critic=(20,), clip=True, seed=6),
    "lstm1_h17_every":  dict(kind="lstm", layers=1, H=17, T=6, E=3, dones="every", obs=(11, 13), actor=(24, 10), critic=(20,), clip=True, seed=7),
    "gru2_h64_last":    dict(kind="gru", layers=2, H=64, T=6, E=4, dones="last", obs=(11, 13), actor=(24,), critic=(20,), clip=True, seed=8),
    "lstm2_h17_short":  dict(kind="lstm", layers=2, H=17, T=6, E=5, dones="short", obs=(11, 13), actor=(24, 10), critic=(20,), clip=True, seed=9),
    "gru1_h64_one_env": dict(kind="gru", layers=1, H=64, T=6, E=1, dones=2, obs=(11, 13), actor=(24, 10), critic=(20,), clip=False, seed=10),
    "gru1_h17_short":   dict(kind="gru", layers=1, H=17, T=6, E=33, dones="short", obs=(11, 13), actor=(24,), critic=(20,), clip=True, first=1, seed=11),
    "lstm1_h256_t3":    dict(kind="lstm", layers=1, H=256, T=3, E=9, dones=1, obs=(45, 61), actor=(32,), critic=(32,), clip=True, seed=12),
    "lstm1_h512_t2":    dict(kind="lstm", layers=1, H=512, T=2, E=7, dones=2, obs=(45, 61), actor=(32,), critic=(32,), clip=True, shared=True, seed=13),
}
TINY = ("lstm2_h17_short", "gru2_h64_last", "lstm1_h17_every", "gru1_h17_t6")       # the sets of the planted-defect tests


# ---- the plan (csrc/lg_train_rnn.hip: make_plan), restated --------------------------------------------------------------------------------------
def plan(n_rows, max_len, n_traj, T, kind, memories, actor_widths, critic_widths):
    """LgTrainRnnPlan's members as a dict; `memories`: (layers, H, input width) of memory_a and memory_c."""
    G, N = GATES[kind], n_rows
    w = ts.lds_widths([(actor_widths, 0), (critic_widths, 0)])
    out = dict(n_envs=N // T, index_off=0)
    names = ("gate_off", "h_off", "hprev_off", "c_off", "nh_off", "dout_off", "dx_off", "dh_off")
    for n in names:
        out[n] = [[-1] * MAX_LAYERS for _ in memories]
    off, t_floats = 0, 0
    for mi, (layers, H, n_in) in enumerate(memories):
        for l in range(layers):
            w[0] = max(w[0], ts.lds_stride(H if l else n_in))
            w[1] = max(w[1], ts.lds_stride(G * H))
            for n, size in (("gate_off", G * H), ("h_off", H), ("hprev_off", H), ("c_off" if kind == "lstm" else "nh_off", H), ("dout_off", H), ("dx_off", G * H)) \
                    + ((("dh_off", G * H),) if kind == "gru" else ()):
                out[n][mi][l] = off
                off += N * size
        t_floats = max(t_floats, 2 * ts.lds_stride(H) + ts.lds_stride(G * H))
    out["index_off"] = off
    off += 2 * n_traj + N
    chains, off, jobs = ts.offsets(N, [actor_widths, critic_widths], off, TARGET_JOBS)
    S, per = ts.slice_rule(N, 1, TARGET_JOBS)
    out["train"] = dict(chains, std_slices=S, std_slice_rows=per, std_p_off=off, weight_jobs=jobs + S)
    out["train"]["row_tile"], out["train"]["lds_bytes"] = ts.row_tile(w)
    off += S * actor_widths[-1]
    out["train"]["workspace_floats"] = off
    jobs += S
    out["slices"], out["slice_rows"], out["p_off"] = ([[[0, 0] for _ in range(MAX_LAYERS)] for _ in memories] for _ in range(3))
    for mi, (layers, H, n_in) in enumerate(memories):
        for l in range(MAX_LAYERS):
            for wi in range(2):
                out["p_off"][mi][l][wi] = -1
        for l in range(layers):
            for wi, K in enumerate((H if l else n_in, H)):
                M = G * H
                tiles = -(-M // ts.WG_TILE) * -(-K // ts.WG_TILE)
                S, per = ts.slice_rule(N, tiles, TARGET_JOBS)
                out["slices"][mi][l][wi], out["slice_rows"][mi][l][wi], out["p_off"][mi][l][wi] = S, per, off
                off += S * (M * K + M)
                jobs += S * tiles
    out["weight_jobs"], out["workspace_floats"] = jobs, off
    r = next((r for r in ts.ROW_TILES if r * t_floats * 4 <= ts.LDS_BYTES), 0)
    out["time_row_tile"], out["time_lds_bytes"], out["time_tiles"] = r, r * t_floats * 4, -(-n_traj // r) if r else 0
    return out


def mems_of(c):
    """[(layers, H)] of memory_a and memory_c of a case: memory_c has memory_a's unless the case carries critic_mem."""
    return [(c["layers"], c["H"]), tuple(c.get("critic_mem") or (c["layers"], c["H"]))]


def plan_of_case(inp):
    mem = [(L, H, o) for (L, H), o in zip(mems_of(inp), inp["obs_widths"])]
    return plan(inp["T"] * inp["E"], inp["max_len"], inp["n_traj"], inp["T"], inp["kind"], mem, inp["actor_widths"], inp["critic_widths"])


# ---- the draws ----------------------------------------------------------------------------------------------------------------------------------
def draw_dones(rng, T, E, dones):
    d = np.zeros((T, E), bool)
    if dones == "every":
        d[:, 1 % E] = True
    elif dones == "short":
        d[rng.integers(T // 2 - 1, T // 2 + 1, size=E), np.arange(E)] = True        # both parts shorter than T
    elif isinstance(dones, int):
        free = [(t, e) for t in range(T - 1) for e in range(E)]
        for i in rng.choice(len(free), size=dones, replace=False):
            d[free[i]] = True
    if dones not in ("short", "none"):
        d[T - 1] = True                                                            # the rollout's end closes every env's last trajectory
    return d


def lengths_of(dones, short=False):
    """The trajectory lengths in env-major order (rsl_rl/utils/utils.py:33-65): a trajectory ends with a done or with the rollout."""
    T, E = dones.shape
    lens = []
    for e in range(E):
        n = 0
        for t in range(T):
            n += 1
            if dones[t, e] or t == T - 1:
                lens.append(n)
                n = 0
    return np.asarray(lens)


def positions(lens, T, E, traj_major=False):
    """(t, j, unpadded row) of every valid step, in (j, t) order: step t of trajectory j is row (s_j % T + t) E + s_j // T."""
    s = np.cumsum(lens) - lens
    t = np.concatenate([np.arange(n) for n in lens])
    j = np.repeat(np.arange(len(lens)), lens)
    row = s[j] + t if traj_major else (s[j] % T + t) * E + s[j] // T
    return t, j, row


def names_of(case):
    c = case
    (La, Ha), (Lc, Hc) = mems_of(c)
    a, k = [Ha, *c["actor"], c["A"]], [Hc, *c["critic"], 1]
    return ["std"] + [f"{ch}.{i}.{n}" for ch, w in (("actor", a), ("critic", k)) for i in range(len(w) - 1) for n in ("weight", "bias")] + \
        [f"{m}.rnn.{n}_l{l}" for m, L in (("memory_a", La), ("memory_c", Lc)) for l in range(L) for n in RNN_PARAMS]


def make_inputs(case, pad=0.0):
    """The arrays of a case (a table name or a dict): everything float32 but the masks; `pad`: what the padding holds."""
    c = dict(CASES[case] if isinstance(case, str) else case)
    c.setdefault("A", 3)
    rng = np.random.default_rng(1000 + c["seed"])
    f = np.float32
    kind, H, T, E, G = c["kind"], c["H"], c["T"], c["E"], GATES[c["kind"]]
    mems = mems_of(c)
    lens = lengths_of(draw_dones(rng, T, E, c["dones"]))
    n_traj, max_len = len(lens), int(lens.max())
    t_idx, j_idx, _ = positions(lens, T, E)
    first, shared = c.get("first", 0), bool(c.get("shared", False))
    inp = dict(c, lens=lens, n_traj=n_traj, max_len=max_len, first=first, shared=shared, obs_widths=c["obs"], pad=pad,
               actor_widths=[H, *c["actor"], c["A"]], critic_widths=[mems[1][1], *c["critic"], 1])
    masks = np.zeros((T, n_traj), bool)
    masks[t_idx, j_idx] = True
    inp["masks"] = masks
    for key, O in zip(("obs", "critic_obs"), c["obs"]):
        x = np.full((max_len, n_traj, O), pad, f)
        x[t_idx, j_idx] = rng.normal(size=(len(t_idx), O)).astype(f)
        if "obs_scale" in c:                                                       # tests/train_rnn_edges.py: observations that saturate the gates
            x[t_idx, j_idx] *= f(c["obs_scale"])
        inp[key] = x
    for m, (L, Hm) in zip("ac", mems):
        inp["h0_" + m] = (0.5 * rng.normal(size=(L, n_traj, Hm))).astype(f)
        inp["c0_" + m] = (0.5 * rng.normal(size=(L, n_traj, Hm))).astype(f) if kind == "lstm" else None
    if shared:
        inp["h0_c"], inp["c0_c"] = inp["h0_a"], inp["c0_a"]
    values = [(0.5 + 0.5 * rng.random(c["A"])).astype(f)] + ts.draw_layers(rng, inp["actor_widths"]) + ts.draw_layers(rng, inp["critic_widths"])
    for O, (L, Hm) in zip(c["obs"], mems):
        bound = 1.0 / np.sqrt(Hm)
        for l in range(L):
            K = Hm if l else O
            values += [rng.uniform(-bound, bound, size=s).astype(f) for s in ((G * Hm, K), (G * Hm, Hm), (G * Hm,), (G * Hm,))]
    inp["names"] = names_of(c)
    inp["params"] = dict(zip(inp["names"], values))
    N = T * E
    inp["grad_mu"], inp["grad_sigma"], inp["grad_values"] = (rng.normal(size=(N, w)).astype(f) for w in (c["A"], c["A"], 1))
    inp["clip"] = None
    if c["clip"]:
        inp["clip"] = ts.place_clip(restate(inp, np.float64)["pre_clip"])
    return inp


# ---- the arithmetic in numpy --------------------------------------------------------------------------------------------------------------------
def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def _memory_params(inp, m, dtype):
    return [[np.asarray(inp["params"][f"memory_{m}.rnn.{n}_l{l}"]).astype(dtype) for n in RNN_PARAMS] for l in range(mems_of(inp)["ac".index(m)][0])]


def memory_forward(kind, params, x, lens, h0, c0, dtype, defects=()):
    """Per layer the stored sequences (max_len, n_traj, .) of one memory over the padded input x: the activated gates, c (LSTM), nh (GRU),
    h and h_prev; steps at or behind a trajectory's length leave the state as it is and store zeros."""
    max_len, n_traj = x.shape[:2]
    valid = np.arange(max_len)[:, None] < lens[None, :]
    inp, out = np.where(valid[:, :, None], x, 0).astype(dtype), []
    for l, (Wih, Whh, bih, bhh) in enumerate(params):
        H = Whh.shape[1]
        h = (np.zeros_like(h0[l]) if "zero_start" in defects else h0[l]).astype(dtype)
        c = None if c0 is None else (np.zeros_like(c0[l]) if "zero_start" in defects else c0[l]).astype(dtype)
        st = dict(gates=[], c=[], nh=[], h=[], hprev=[], x=inp)
        prev_below = np.zeros((n_traj, inp.shape[2]), dtype)
        for t in range(max_len):
            v = valid[t][:, None]
            xt = inp[t]
            if l and "layer1_old_h" in defects:
                xt, prev_below = prev_below, inp[t]
            ax, ah = (xt @ Wih.T + bih).astype(dtype), (h @ Whh.T + bhh).astype(dtype)
            if kind == "lstm":
                a = ax + ah
                if "gate_order" in defects:
                    i, f, o, g = _sig(a[:, :H]), _sig(a[:, H:2 * H]), _sig(a[:, 2 * H:3 * H]), np.tanh(a[:, 3 * H:])
                else:
                    i, f, g, o = _sig(a[:, :H]), _sig(a[:, H:2 * H]), np.tanh(a[:, 2 * H:3 * H]), _sig(a[:, 3 * H:])
                cn = (f * c + i * g).astype(dtype)
                hn = (o * np.tanh(cn)).astype(dtype)
                gates = np.concatenate([i, f, g, o], 1)
                st["c"].append(np.where(v, cn, 0).astype(dtype))
                c = np.where(v, cn, c).astype(dtype)
            else:
                r, z = _sig(ax[:, :H] + ah[:, :H]), _sig(ax[:, H:2 * H] + ah[:, H:2 * H])
                nh = ah[:, 2 * H:]
                n = np.tanh(ax[:, 2 * H:] + r * nh)
                hn = (z * n + (1 - z) * h if "z_swapped" in defects else (1 - z) * n + z * h).astype(dtype)
                gates = np.concatenate([r, z, n], 1)
                st["nh"].append(np.where(v, nh, 0).astype(dtype))
            st["gates"].append(np.where(v, gates, 0).astype(dtype))
            st["hprev"].append(np.where(v, h, 0).astype(dtype))
            st["h"].append(np.where(v, hn, 0).astype(dtype))
            h = np.where(v, hn, h).astype(dtype)
        for k in ("gates", "c", "nh", "h", "hprev"):
            st[k] = np.stack(st[k]) if st[k] else None
        out.append(st)
        inp = st["h"]
    return out


def memory_backward(kind, params, stored, lens, h0, c0, d_top, order, pers, dtype, defects=()):
    """[weight_ih, weight_hh, bias_ih, bias_hh] gradients per layer of one memory from d loss / d h of its top layer (max_len, n_traj, H).
    `order`: (t, j) index arrays of the valid steps in unpadded row order, the order of the batch sums; pers[l] = (rows per slice of the ih
    pair, of the hh pair) or None for one slice."""
    max_len = d_top.shape[0]
    valid = np.arange(max_len)[:, None] < lens[None, :]
    grads, dout = [None] * len(params), d_top
    for l in range(len(params) - 1, -1, -1):
        Wih, Whh = params[l][0], params[l][1]
        st, H = stored[l], Whh.shape[1]
        dh = np.zeros_like(dout[0])
        dc = np.zeros_like(dout[0])
        DX, DH = np.zeros(st["gates"].shape, dtype), np.zeros(st["gates"].shape, dtype)
        for t in range(max_len - 1, -1, -1):
            v = valid[t][:, None]
            d = (dout[t] + dh).astype(dtype)
            g = st["gates"][t]
            if kind == "lstm":
                i, f, gg, o = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
                cp = st["c"][t - 1] if t else (np.zeros_like(c0[l]) if "zero_start" in defects else c0[l]).astype(dtype)
                tc = np.tanh(st["c"][t])
                dcn = (dc + d * o * (1 - tc * tc)).astype(dtype)
                D = np.concatenate([dcn * gg * i * (1 - i), dcn * cp * f * (1 - f), dcn * i * (1 - gg * gg), d * tc * o * (1 - o)], 1).astype(dtype)
                D = np.where(v, D, 0).astype(dtype)
                dc = np.zeros_like(dc) if "no_dc_carry" in defects else np.where(v, dcn * f, dc).astype(dtype)
                DX[t] = DH[t] = D
                direct = 0
            else:
                r, z, n = g[:, :H], g[:, H:2 * H], g[:, 2 * H:]
                hp, nh = st["hprev"][t], st["nh"][t]
                Dn = d * (1 - z) * (1 - n * n)
                Dz = d * (hp - n) * z * (1 - z)
                Dr = Dn * nh * r * (1 - r)
                DX[t] = np.where(v, np.concatenate([Dr, Dz, Dn], 1), 0).astype(dtype)
                DH[t] = np.where(v, np.concatenate([Dr, Dz, Dn if "bhn_without_r" in defects else Dn * r], 1), 0).astype(dtype)
                direct = np.where(v, d * z, 0)
            dh = np.zeros_like(dh) if "no_dh_carry" in defects else ((DH[t] @ Whh).astype(dtype) + direct).astype(dtype)
        tt, jj = order
        per = pers[l] if pers is not None else (len(tt), len(tt))
        Gx, Gh = DX[tt, jj], DH[tt, jj]
        hm = (st["h"] if "whh_uses_ht" in defects else st["hprev"])[tt, jj]
        grads[l] = [ts.slice_sum(per[0], Gx, st["x"][tt, jj]), ts.slice_sum(per[1], Gh, hm), ts.slice_sum(per[0], Gx, phases=4), ts.slice_sum(per[1], Gh, phases=4)]
        dout = (DX @ Wih).astype(dtype)
    return grads


def restate(inp, dtype, defects=(), sliced=False, rows=None):
    """mu, sigma, values and every parameter gradient (by name) of a case under the cotangents grad_mu, grad_sigma, grad_values, and
    `pre_clip`, the means before the Hardtanh.  sliced: the batch sums per slice in slice order as the plan cuts them (the float32 side of
    the host tests); otherwise one sum.  rows: a function (lens, T, E) -> (t, j, row) in place of `positions` (tests/train_rnn_edges.py's
    restatement of the index kernel, which may give a row to two steps: the later one in (j, t) order holds it, as a store would).  Two
    defects beside DEFECTS, for memories that differ and observations wider than a gradient tile (tests/train_rnn_edges.py):
    shallow_loop, both memories run memory_a's depth (the critic reads the last layer that ran, the layers behind get no gradient);
    ih_first_k_tile, grad weight_ih_l0 keeps its columns below WG_TILE only."""
    kind, T, E, A = inp["kind"], inp["T"], inp["E"], inp["A"]
    lens = np.minimum(inp["lens"] + 1, inp["max_len"]) if "padded_step" in defects else inp["lens"]
    t_idx, j_idx, row = positions(lens, T, E, "traj_major_rows" in defects) if rows is None else rows(lens, T, E)
    depth = mems_of(inp)[0][0] if "shallow_loop" in defects else MAX_LAYERS
    mem_params = [_memory_params(inp, m, dtype) for m in "ac"]
    N = T * E
    if "padded_step" in defects:                     # the counted steps run over the rows: keep what lands inside
        keep = row < N
        t_idx, j_idx, row = t_idx[keep], j_idx[keep], row[keep]
    by_row = np.argsort(row, kind="stable")
    order = (t_idx[by_row], j_idx[by_row])
    pl = plan_of_case(inp) if sliced else None
    P = {k: np.asarray(v).astype(dtype) for k, v in inp["params"].items()}
    out, tops, stored = {}, [], []
    for mi, (m, key) in enumerate((("a", "obs"), ("c", "critic_obs"))):
        st = memory_forward(kind, mem_params[mi][:depth], inp[key].astype(dtype), lens, inp["h0_" + m], inp["c0_" + m], dtype, defects)
        top = np.zeros((N, mems_of(inp)[mi][1]), dtype)
        top[row] = st[-1]["h"][t_idx, j_idx]
        tops.append(top)
        stored.append(st)
    chains = {}
    for ch, top, widths in (("actor", tops[0], inp["actor_widths"]), ("critic", tops[1], inp["critic_widths"])):
        layers = [(P[f"{ch}.{i}.weight"], P[f"{ch}.{i}.bias"]) for i in range(len(widths) - 1)]
        chains[ch] = (layers, ts.mlp(layers, top, dtype))
    pre = chains["actor"][1][-1]
    mu = ts.hardtanh(pre, inp["clip"], dtype)
    out.update(pre_clip=pre, mu=mu, sigma=(mu * 0 + P["std"]).astype(dtype), values=chains["critic"][1][-1])
    S_std = pl["train"]["std_slice_rows"] if sliced else N
    out["std"] = ts.slice_sum(S_std, inp["grad_sigma"].astype(dtype))
    for ci, (ch, G, mi, m) in enumerate((("actor", ts.masked_grad_mu(inp["grad_mu"], mu, inp["clip"], dtype), 0, "a"),
                                         ("critic", inp["grad_values"].astype(dtype), 1, "c"))):
        layers, acts = chains[ch]
        g, gin = ts.chain_backward(layers, acts, G, dtype, pl["train"]["slice_rows"][ci] if sliced else None, input_grad=True)
        for i in range(len(layers)):
            out[f"{ch}.{i}.weight"], out[f"{ch}.{i}.bias"] = g[2 * i], g[2 * i + 1]
        d_top = np.zeros((inp["max_len"], inp["n_traj"], mems_of(inp)[mi][1]), dtype)
        d_top[t_idx, j_idx] = gin[row]
        mg = memory_backward(kind, mem_params[mi][:depth], stored[mi], lens, inp["h0_" + m], inp["c0_" + m], d_top, order,
                             pl["slice_rows"][mi] if sliced else None, dtype, defects)
        mg += [[np.zeros_like(p) for p in layer] for layer in mem_params[mi][depth:]]
        for l, gl in enumerate(mg):
            for n, v in zip(RNN_PARAMS, gl):
                out[f"memory_{m}.rnn.{n}_l{l}"] = v
        if "ih_first_k_tile" in defects:
            out[f"memory_{m}.rnn.weight_ih_l0"] = np.where(np.arange(inp["obs_widths"][mi]) < ts.WG_TILE, out[f"memory_{m}.rnn.weight_ih_l0"], 0).astype(dtype)
    return out


# ---- the torch side -----------------------------------------------------------------------------------------------------------------------------
class Memory(torch.nn.Module):
    def __init__(self, kind, n_in, H, layers):
        super().__init__()
        self.rnn = (torch.nn.LSTM if kind == "lstm" else torch.nn.GRU)(input_size=n_in, hidden_size=H, num_layers=layers)


class Recurrent(torch.nn.Module):
    """ActorCriticRecurrent's members (rsl_rl/modules/actor_critic_recurrent.py) in its parameter order, with a case's values."""
    is_recurrent = True

    def __init__(self, inp, dtype=torch.float32):
        super().__init__()
        self.actor, self.critic = ts.sequential(inp["actor_widths"], inp["clip"]), ts.sequential(inp["critic_widths"], None)
        self.std = torch.nn.Parameter(torch.ones(inp["A"]))
        (La, Ha), (Lc, Hc) = mems_of(inp)
        self.memory_a = Memory(inp["kind"], inp["obs_widths"][0], Ha, La)
        self.memory_c = Memory(inp["kind"], inp["obs_widths"][1], Hc, Lc)
        self.to(dtype)
        params = list(self.parameters())                  # std, actor, critic, memory_a, memory_c: the order of inp["names"]
        assert len(params) == len(inp["names"])
        ts.set_parameters(params, [inp["params"][n] for n in inp["names"]], dtype)

    def forward(self, obs, critic_obs, masks, hid_a, hid_c):
        """(mu, sigma, values) as act / evaluate of the reference in batch mode compute them."""
        out = []
        for mem, x, hid in ((self.memory_a, obs, hid_a), (self.memory_c, critic_obs, hid_c)):
            y, _ = mem.rnn(x, hid)
            y = torch.cat([y, y.new_zeros((masks.shape[0] - y.shape[0],) + tuple(y.shape[1:]))])        # max_len < T: the masks have T rows
            out.append(y.transpose(1, 0)[masks.transpose(1, 0)].view(-1, masks.shape[0], y.shape[-1]).transpose(1, 0).flatten(0, 1))
        mu = self.actor(out[0])
        return mu, mu * 0 + self.std, self.critic(out[1])


def hidden_of(inp, m, dtype, device="cpu"):
    h, c = (None if a is None else torch.from_numpy(a).to(dtype).to(device) for a in (inp["h0_" + m], inp["c0_" + m]))
    return h if c is None else (h, c)


def torch_reference(inp, dtype):
    """The same dict as restate's (without pre_clip) from torch's nn.LSTM / nn.GRU, the reference's unpadding and autograd, on the CPU."""
    m = Recurrent(inp, dtype)
    t = lambda a: torch.from_numpy(np.nan_to_num(np.asarray(a, np.float32), nan=0.0)).to(dtype)
    valid = torch.from_numpy(inp["masks"][:inp["max_len"]])[:, :, None]
    obs, cobs = (torch.where(valid, t(inp[k]), torch.zeros((), dtype=dtype)) for k in ("obs", "critic_obs"))
    mu, sigma, values = m(obs, cobs, torch.from_numpy(inp["masks"]), hidden_of(inp, "a", dtype), hidden_of(inp, "c", dtype))
    ((mu * t(inp["grad_mu"])).sum() + (sigma * t(inp["grad_sigma"])).sum() + (values * t(inp["grad_values"])).sum()).backward()
    out = dict(mu=mu, sigma=sigma, values=values)
    out.update({n: p.grad for n, p in zip(inp["names"], m.parameters())})
    return {k: v.detach().numpy() for k, v in out.items()}


# ---- the parity rule ----------------------------------------------------------------------------------------------------------------------------
def _class_name(name):
    """A memory parameter under a name train_support.tensor_class sorts as the weight or the bias it is."""
    return name.replace("weight_", "").replace("bias_", "") + (".weight" if ".rnn.weight_" in name else ".bias") if ".rnn." in name else name


def check_parity(got, ref64, ref32, label, report=None, factor=ts.PARITY_FACTOR):
    """train_support.check_parity over every tensor of ref64, the memories' parameters in the classes of their kind."""
    r = lambda d: {_class_name(k): v for k, v in d.items() if k in ref64}
    return ts.check_parity(r(got), r(ref64), r(ref32), label, report, factor)


# ---- the golden fixtures (tests/golden/gen_ppo_recurrent_train_fixtures.py) ----------------------------------------------------------------------
FIXTURE_COLUMNS = ("actions", "target_values", "advantages", "returns", "old_log_prob", "old_mu", "old_sigma")
CFG_KEYS = ("lr0", "beta1", "beta2", "eps", "max_grad_norm", "desired_kl", "steps", "clip_param", "value_loss_coef", "entropy_coef", "clip_actions", "T", "layers",
            "lstm")


def load_fixture(path):
    """dict(names (the fixture's, torch's), cfg, init=[arrays], per step: the stored columns flattened to (T E, .) rows, mu, sigma, values,
    loss, kl, lr, grad_norm, grads=[per step [arrays]], params=[per step [arrays]], traj_range, env_range; the padded set, the masks and
    the start states of the whole storage), float64."""
    z = np.load(path)
    names, by_name = ts.fixture_shapes(z)
    split = lambda flat: ts.split_flat(flat, by_name, names)
    cfg = dict(zip(CFG_KEYS, (float(v) for v in z["cfg"])))
    for k in ("steps", "T", "layers", "lstm"):
        cfg[k] = int(cfg[k])
    out = dict(names=names, cfg=cfg, init=split(z["init"]), grads=[split(g) for g in z["grads"]],
               params=[split(p) for p in z["init"][None] + np.cumsum(z["param_steps"], axis=0)],
               actor=ts.chain_widths(names, by_name, "actor"), critic=ts.chain_widths(names, by_name, "critic"))
    for k in FIXTURE_COLUMNS:
        out[k] = z[k].reshape(z[k].shape[0], -1, z[k].shape[-1])
    for k in ("mu", "sigma", "values", "loss", "kl", "lr", "grad_norm", "traj_range", "env_range", "padded_obs", "padded_critic_obs", "masks", "hid_a_h"):
        out[k] = z[k]
    out["hid_a_c"] = z["hid_a_c"] if cfg["lstm"] else None
    out["hid_c_h"], out["hid_c_c"] = (out["hid_a_h"], out["hid_a_c"]) if cfg["lstm"] else (z["hid_c_h"], None)      # rollout_storage.py:231
    return out


def fixture_inputs(fx, s, params=None, dtype=np.float64):
    """Step s of a fixture as make_inputs shapes a case (no clip placement, zero cotangents); `params`: instead of the fixture's own
    parameters before that step."""
    cfg = fx["cfg"]
    params = params if params is not None else (fx["init"] if s == 0 else fx["params"][s - 1])
    first, last = (int(v) for v in fx["traj_range"][s])
    masks = fx["masks"][:, first:last]
    T, E, H, A = cfg["T"], int(fx["env_range"][s][1] - fx["env_range"][s][0]), fx["actor"][0], fx["actor"][-1]
    c = dict(kind="lstm" if cfg["lstm"] else "gru", layers=cfg["layers"], H=H, A=A, T=T, E=E, actor=tuple(fx["actor"][1:-1]), critic=tuple(fx["critic"][1:-1]))
    inp = dict(c, lens=masks.sum(0).astype(np.int64), n_traj=last - first, max_len=int(fx["padded_obs"].shape[0]), first=first, shared=bool(cfg["lstm"]),
               obs_widths=(fx["padded_obs"].shape[2], fx["padded_critic_obs"].shape[2]), actor_widths=list(fx["actor"]), critic_widths=list(fx["critic"]),
               masks=masks, obs=fx["padded_obs"][:, first:last].astype(dtype), critic_obs=fx["padded_critic_obs"][:, first:last].astype(dtype),
               clip=cfg["clip_actions"], names=names_of(c))
    for m in "ac":
        for n in "hc":
            a = fx[f"hid_{m}_{n}"]
            inp[f"{n}0_{m}"] = None if a is None else np.ascontiguousarray(a[:, first:last]).astype(dtype)
    inp["params"] = dict(zip(inp["names"], (np.asarray(p).astype(dtype) for p in params)))
    N = T * E
    inp["grad_mu"], inp["grad_sigma"], inp["grad_values"] = (np.zeros((N, w), dtype) for w in (A, A, 1))
    return inp

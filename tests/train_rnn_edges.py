"""The edge cases of the recurrent learner pass (csrc/lg_train_rnn.hip, include/lgtrainrnn.h, hcr_genesis_lr_cl_amd/train.py's
FusedTrainPassRecurrent) that the table of tests/train_rnn_cases.py does not reach: ONE table of rows, each a case of that module with the
kernel paths it is there to reach, and the helpers the two test files on it share -- tests/test_train_rnn_edges_host.py (no GPU: the tags
of every row from the restated plan, the drawn lengths and the index kernel's chunking restated here; the plan of the library; the
restatement against torch; the float32 restatement inside half the rule; four planted defects) and tests/test_gpu_train_rnn_edges.py (the
kernels against float64).  No test functions here, nothing needs a GPU.

Built on what exists: make_inputs, restate, plan_of_case, torch_reference and check_parity of tests/train_rnn_cases.py (a case may carry
critic_mem=(layers, H) for a memory_c of its own depth and width, and obs_scale), the parity rule of tests/train_support.py.  The old table
stays as it is."""
import functools

import numpy as np
import torch

from tests import train_rnn_cases as rc
from tests import train_support as sup

THREADS = 256                  # csrc/lg_train_tiles.h: kThreads, the one workgroup of train_rnn_index_kernel
HALF_FACTOR = sup.PARITY_FACTOR / 2        # the float32 restatement stays within half the rule's factor 8: no GPU comparison is decided by the draw
LARGE = 100.0                  # tests/test_train_rnn_host.py's "large factor" above the rule's own bound
_STD = dict(obs=(11, 13), actor=(24, 10), critic=(20,), clip=True)


def _smallest_h(kind, tile):
    """The smallest hidden width whose time loop (2 lds_stride(H) + lds_stride(G H) floats per trajectory) no longer fits the next larger
    trajectory tile: `tile` is what make_plan chooses from there on."""
    need = lambda H: (2 * sup.lds_stride(H) + sup.lds_stride(rc.GATES[kind] * H)) * 4
    return next(H for H in range(1, rc.MAX_HIDDEN + 1) if 2 * tile * need(H) > sup.LDS_BYTES)


H16 = _smallest_h("lstm", 16)          # 197: 2 x 260 + 836 = 1356 floats per trajectory, 32 of them are 173 568 B > 160 KB; 196 has 1228: 157 184 B

# ---- the table ------------------------------------------------------------------------------------------------------------------------------
# A row is a case of tests/train_rnn_cases.py (n_traj = E + dones) and `reach`, the tags of `tags` it must have.
# idx_*:  more than 256 trajectories, so that a thread of the index kernel owns a chunk of `per` of them: 257 = 128 x 2 + 1 (a last chunk of
#         one and 127 threads without any), 529 = 176 x 3 + 1, 1497 = 249 x 6 + 3 (per = 6 as DESIGN 13f's go2_lstm mini-batch of 1496).
#         idx_1497 has 6 x 1399 = 8394 rows: every pair of both memories sums in 32 slices of 264 rows, the last of 210 = 2 mod 4 (1400 envs
#         and 97 dones, 8400 rows, would end on a last slice of 216 rows, a multiple of 4); its time loop has 47 tiles of 32.
# t16_*:  H16 = 197, the smallest LSTM width that plans the 16-trajectory tile, at 15 / 16 / 17 / 33 trajectories.
# t8_*:   a GRU at H = 512: 2 x 516 + 1540 = 2572 floats per trajectory, 16 of them are 164 608 B > 160 KB, so 8; at 7 / 8 / 17 trajectories.
# mix_*:  memories that differ (critic_mem): the deeper actor (the critic's blocks of the layer-1 launches return at once), the deeper
#         critic, and a 16-trajectory tile that memory_c alone asks for while memory_a alone would run 32.
# wide_x: 130 observation columns are three K tiles of wgrad_wave_x, the last 2 columns wide; the critic observes one column.
# h1:     H = 1, two layers.  t24_*: T = 24, with dones and with every trajectory T steps long.
# idx_529 and idx_1497 have no Hardtanh: among their 4680 and 25 182 means train_support.place_clip finds no clip that keeps 1e-3 from every
#         one before it has left the bulk (the clipped shares would be 0.06 and 0.005, outside [0.1, 0.9]); idx_257 has it.
# Seeds: each row's first seed was 100 + its position; test_float32_restatement_keeps_half_the_rule names what a replaced one gave.
ROWS = {
    "idx_257": dict(kind="gru", layers=1, H=7, T=2, E=250, dones=7, seed=101, reach=("per=2", "ragged-chunk", "last-chunk=1", "empty-threads", "n_traj=257")),
    "idx_529": dict(kind="lstm", layers=1, H=17, T=3, E=520, dones=9, clip=False, seed=102, reach=("per=3", "ragged-chunk", "last-chunk=1", "empty-threads", "S>=16", "n_traj=529")),
    "idx_1497": dict(kind="gru", layers=2, H=7, T=6, E=1399, dones=98, clip=False, seed=103,
                     reach=("per=6", "ragged-chunk", "last-chunk=3", "empty-threads", "S=32-every-memory-pair", "last-slice%4!=0", "time-tiles>=47", "n_traj=1497")),
    "t16_15": dict(kind="lstm", layers=1, H=H16, T=2, E=12, dones=3, seed=104, reach=("Rt=16", "tile-one-short", "n_traj=15")),
    "t16_16": dict(kind="lstm", layers=1, H=H16, T=3, E=13, dones=3, seed=105, reach=("Rt=16", "tile-full", "n_traj=16")),
    "t16_17": dict(kind="lstm", layers=1, H=H16, T=2, E=14, dones=3, seed=106, reach=("Rt=16", "tile-one-over", "n_traj=17")),
    "t16_33": dict(kind="lstm", layers=1, H=H16, T=3, E=29, dones=4, seed=107, reach=("Rt=16", "tiles=3", "tile-one-over", "n_traj=33")),
    "t8_7": dict(kind="gru", layers=1, H=512, T=2, E=5, dones=2, seed=108, reach=("Rt=8", "gru", "tile-one-short", "n_traj=7")),
    "t8_8": dict(kind="gru", layers=1, H=512, T=2, E=6, dones=2, seed=109, reach=("Rt=8", "gru", "tile-full", "n_traj=8")),
    "t8_17": dict(kind="gru", layers=1, H=512, T=2, E=14, dones=3, seed=110, reach=("Rt=8", "gru", "tiles=3", "tile-one-over", "n_traj=17")),
    "mix_a_deep": dict(kind="lstm", layers=2, H=17, critic_mem=(1, 64), T=6, E=9, dones=4, seed=111, reach=("layers-differ", "H-differ", "critic-returns-early")),
    "mix_c_deep": dict(kind="gru", layers=1, H=65, critic_mem=(2, 7), T=6, E=9, dones=4, shared=False, seed=112,
                       reach=("layers-differ", "H-differ", "actor-returns-early")),
    "mix_tile": dict(kind="lstm", layers=1, H=7, critic_mem=(1, H16), T=2, E=14, dones=3, seed=113, reach=("Rt=16", "Rt-from-memory_c", "H-differ", "n_traj=17")),
    "wide_x": dict(kind="lstm", layers=1, H=17, T=6, E=12, dones=4, obs=(130, 1), seed=114, reach=("tiles_k=3", "k-tail=2", "n_in=1")),
    "h1": dict(kind="gru", layers=2, H=1, T=6, E=5, dones=3, obs=(3, 2), actor=(4,), seed=115, reach=("H=1",)),
    "t24_lstm": dict(kind="lstm", layers=1, H=17, T=24, E=3, dones=5, seed=116, reach=("T=24",)),
    "t24_gru_full": dict(kind="gru", layers=2, H=7, T=24, E=2, dones="last", seed=117, reach=("T=24", "every-trajectory-full")),
}
NAMES = list(ROWS)
IDX_ROWS = ("idx_257", "idx_529", "idx_1497")
# what the table as a whole is there for
TABLE_TAGS = {"per=2", "per=3", "per=6", "ragged-chunk", "empty-threads", "S=32-every-memory-pair", "last-slice%4!=0", "Rt=16", "Rt=8", "tile-one-short",
              "tile-full", "tile-one-over", "tiles=3", "layers-differ", "H-differ", "critic-returns-early", "actor-returns-early", "Rt-from-memory_c",
              "tiles_k=3", "n_in=1", "H=1", "T=24", "every-trajectory-full"}
# Two rows again with observations scaled until the gates saturate: in the float64 restatement at least half of layer 0's gate
# pre-activations, the ones an observation reaches, lie beyond 20 in magnitude (a sigmoid there is within 2e-9 of 0 or 1).  Layer 1 of h1
# reads h in [-1, 1] through weights in [-1, 1]: its pre-activations stay below 4 whatever the observations are.
SATURATED = {"t24_lstm": 96.0, "h1": 64.0}           # shares 0.66 and 0.78; no pre-activation beyond 276
SATURATION = 20.0


def case_of(name, **more):
    c = dict(_STD, **{k: v for k, v in ROWS[name].items() if k != "reach"})
    c.update(more)
    return c


@functools.lru_cache(maxsize=None)
def inputs(name, saturated=False):
    """The float32 inputs of a row (shared: treat as read-only); saturated: with its observations scaled by SATURATED[name]."""
    return rc.make_inputs(case_of(name, **(dict(obs_scale=SATURATED[name]) if saturated else {})))


@functools.lru_cache(maxsize=None)
def references(name, saturated=False):
    """(torch CPU float64, torch CPU float32) of a row, computed once (shared: treat as read-only)."""
    x = inputs(name, saturated)
    return rc.torch_reference(x, torch.float64), rc.torch_reference(x, torch.float32)


# ---- the index kernel's chunking, restated --------------------------------------------------------------------------------------------------
def index_kernel(lens, T, E, defects=()):
    """train_rnn_index_kernel on the lengths `lens`: thread i of the one workgroup owns trajectories [jb, je) = [i per, i per + per) cut at
    n_traj, per = ceil(n_traj / 256); part[i], the sum of its lengths, becomes the exclusive prefix over the threads; the thread then walks
    its chunk with a running s from part[i]: first[j] = (s % T) E + s / T, map[first[j] + t E] = t n_traj + j, s += len[j].  Row indices
    are clamped to [0, T E) as row_of does.  dict(per, ranges, first, map, rows=(t, j, row) in (j, t) order as rc.positions gives them).
    Planted defect chunk_restart: the running sum restarts at the chunk's start for every trajectory of the chunk, s = part[i] each time,
    so that the trajectories of a chunk land on each other; with per = 1 a chunk has one trajectory and nothing changes."""
    lens = np.asarray(lens)
    n_traj, N = len(lens), T * E
    per = -(-n_traj // THREADS)
    ranges = [(min(i * per, n_traj), min(min(i * per, n_traj) + per, n_traj)) for i in range(THREADS)]
    part = [int(lens[jb:je].sum()) for jb, je in ranges]
    s, prefix = 0, []
    for n in part:
        prefix.append(s)
        s += n
    first, row_map = np.zeros(n_traj, np.int64), np.zeros(N, np.int64)
    tt, jj, rows = [], [], []
    for i, (jb, je) in enumerate(ranges):
        s = prefix[i]
        for j in range(jb, je):
            if "chunk_restart" in defects:
                s = prefix[i]
            f = (s % T) * E + s // T
            first[j] = f
            for t in range(int(lens[j])):
                r = min(max(f + t * E, 0), N - 1)
                row_map[r] = t * n_traj + j
                tt.append(t), jj.append(j), rows.append(r)
            s += int(lens[j])
    return dict(per=per, ranges=ranges, first=first, map=row_map, rows=(np.asarray(tt), np.asarray(jj), np.asarray(rows)))


def index_rows(defects=()):
    """rc.restate's `rows` from the restated index kernel."""
    return lambda lens, T, E: index_kernel(lens, T, E, defects)["rows"]


def index_region(x):
    """(len, first, map) of a case as the index kernel must leave them at plan.index_off, from rc.lengths_of / rc.positions alone."""
    t, j, row = rc.positions(x["lens"], x["T"], x["E"])
    row_map = np.zeros(x["T"] * x["E"], np.int64)
    row_map[row] = t * x["n_traj"] + j
    return np.asarray(x["lens"], np.int64), row[t == 0], row_map


# ---- what a row reaches ---------------------------------------------------------------------------------------------------------------------
def memories(x):
    return [(L, H, o) for (L, H), o in zip(rc.mems_of(x), x["obs_widths"])]


def _tile_alone(x, mi):
    """The trajectory tile make_plan would choose if both memories were memory mi."""
    m = memories(x)[mi]
    w = [[m[1], 8, 1]] * 2
    return rc.plan(x["T"] * x["E"], x["max_len"], x["n_traj"], x["T"], x["kind"], [m, m], *w)["time_row_tile"]


def memory_slices(x, p):
    """(memory, layer, pair, slices, rows per slice, rows of the last slice) of every (weight, bias) pair of the memories in the plan p."""
    N = x["T"] * x["E"]
    return [(mi, l, wi, p["slices"][mi][l][wi], p["slice_rows"][mi][l][wi], N - (p["slices"][mi][l][wi] - 1) * p["slice_rows"][mi][l][wi])
            for mi, (L, _, _) in enumerate(memories(x)) for l in range(L) for wi in range(2)]


def tags(name):
    """The set of tag strings a row reaches, from the restated plan, the drawn lengths and the restated index kernel."""
    x = inputs(name)
    p, idx = rc.plan_of_case(x), index_kernel(x["lens"], x["T"], x["E"])
    n_traj, Rt, mem = x["n_traj"], p["time_row_tile"], memories(x)
    (La, Ha, _), (Lc, Hc, _) = mem
    chunks = [je - jb for jb, je in idx["ranges"] if je > jb]
    out = {f"per={idx['per']}", f"last-chunk={chunks[-1]}", f"n_traj={n_traj}", f"Rt={Rt}", f"time-tiles={p['time_tiles']}", f"T={x['T']}", x["kind"]}
    if chunks[-1] < idx["per"]:
        out.add("ragged-chunk")
    if any(jb == je == n_traj for jb, je in idx["ranges"]):
        out.add("empty-threads")
    sl = memory_slices(x, p)
    if min(s[3] for s in sl) >= 16:
        out.add("S>=16")
    if all(s[3] == sup.MAX_SLICES for s in sl):
        out.add("S=32-every-memory-pair")
    if any(s[3] > 1 and s[5] % 4 for s in sl):
        out.add("last-slice%4!=0")
    if p["time_tiles"] >= 47:
        out.add("time-tiles>=47")
    if p["time_tiles"] == 3:
        out.add("tiles=3")
    rem = n_traj % Rt
    out |= ({"tile-one-short"} if rem == Rt - 1 else set()) | ({"tile-full"} if rem == 0 else set()) | ({"tile-one-over"} if rem == 1 and n_traj > Rt else set())
    if La != Lc:
        out |= {"layers-differ", "critic-returns-early" if Lc < La else "actor-returns-early"}
    if Ha != Hc:
        out.add("H-differ")
    if _tile_alone(x, 1) == Rt < _tile_alone(x, 0):
        out.add("Rt-from-memory_c")
    tiles_k = [-(-m[2] // sup.WG_TILE) for m in mem]
    out.add(f"tiles_k={max(tiles_k)}")
    out |= {f"k-tail={m[2] % sup.WG_TILE}" for m, k in zip(mem, tiles_k) if k > 1 and m[2] % sup.WG_TILE}
    out |= {f"n_in={m[2]}" for m in mem if m[2] == 1} | {f"H={m[1]}" for m in mem if m[1] == 1}
    if (x["lens"] == x["T"]).all():
        out.add("every-trajectory-full")
    return out


# ---- the planted defects --------------------------------------------------------------------------------------------------------------------
# Each a change of the restatement alone, and where it applies: on every other row the restatement with the defect is the restatement.
DEFECTS = ("chunk_restart", "ih_first_k_tile", "shallow_loop", "tail_tile_state")


def _tail(x):
    """(first trajectory, trajectories) of the last time tile."""
    Rt = rc.plan_of_case(x)["time_row_tile"]
    j0 = (x["n_traj"] - 1) // Rt * Rt
    return j0, x["n_traj"] - j0


APPLIES = dict(chunk_restart=lambda x: x["n_traj"] > THREADS,                                       # per >= 2: a chunk of more than one trajectory
               ih_first_k_tile=lambda x: max(x["obs_widths"]) > sup.WG_TILE,                        # a second K tile
               shallow_loop=lambda x: rc.mems_of(x)[1][0] > rc.mems_of(x)[0][0],                    # memory_c deeper than memory_a
               tail_tile_state=lambda x: 1 < _tail(x)[1] < rc.plan_of_case(x)["time_row_tile"])     # a partial last tile of more than one trajectory


def restate_with(x, defect, dtype=np.float64):
    """rc.restate of a row with one planted defect.  tail_tile_state: the trajectories of a partial last time tile start from trajectory
    n_traj - 1's h0 (and c0): the clamp min(j0 + row, n_traj - 1), which is there for the rows behind the last trajectory, taken for the
    row's own index.  A last tile of one trajectory is that trajectory: nothing changes there."""
    if defect == "chunk_restart":
        return rc.restate(x, dtype, rows=index_rows((defect,)))
    if defect == "tail_tile_state":
        j0, n = _tail(x)
        y = dict(x)
        if n < rc.plan_of_case(x)["time_row_tile"]:
            for k in ("h0_a", "c0_a", "h0_c", "c0_c"):
                if x[k] is not None:
                    y[k] = x[k].copy()
                    y[k][:, j0:] = x[k][:, -1:]
        return rc.restate(y, dtype)
    return rc.restate(x, dtype, defects=(defect,))


def ratios(got, ref64, ref32):
    """name -> |got - f64| / (the rule's bound): above 1 fails the rule."""
    return {k: sup.max_err(got[k], ref64[k]) / sup.parity_bound(sup.max_err(ref32[k], ref64[k]), ref64[k]) for k in ref64}


# ---- saturation -----------------------------------------------------------------------------------------------------------------------------
def layer0_gate_preactivations(x):
    """Every gate pre-activation of layer 0 of both memories at the valid steps, float64: W_ih x + b_ih + W_hh h + b_hh per gate, the
    GRU's candidate W_in x + b_in + r (W_hn h + b_hn)."""
    f = np.float64
    valid = np.arange(x["max_len"])[:, None] < x["lens"][None, :]
    out = []
    for m, key in (("a", "obs"), ("c", "critic_obs")):
        params = rc._memory_params(x, m, f)
        st = rc.memory_forward(x["kind"], params, x[key].astype(f), x["lens"], x["h0_" + m], x["c0_" + m], f)[0]
        Wih, Whh, bih, bhh = params[0]
        ax, ah = st["x"] @ Wih.T + bih, st["hprev"] @ Whh.T + bhh
        if x["kind"] == "gru":
            H = Whh.shape[1]
            pre = np.concatenate([(ax + ah)[..., :2 * H], ax[..., 2 * H:] + st["gates"][..., :H] * ah[..., 2 * H:]], -1)
        else:
            pre = ax + ah
        out.append(pre[valid].ravel())
    return np.concatenate(out)

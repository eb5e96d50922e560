"""The edge cases of the recurrent fused policy step (the memory prefix of csrc/lg_policy.hip) that the six net sets of
tests/test_policy_recurrent_host.py do not reach: ONE table of net sets, each row with the row tile it plans, and the helpers the two test
files on it share -- tests/test_policy_recurrent_edges_host.py (no GPU: the planned tile, the coverage of the table, uneven descriptors,
discrimination) and tests/test_gpu_policy_recurrent_edges.py (the kernel against float64).  No test functions here, nothing needs a GPU.

Built on what exists: the stand-in, its seeding, the inputs, the float64 oracle / float32 yardstick (`shared`) and the numpy cells of
tests/test_policy_recurrent_host.py, whose optional keys `H_c`, `layers_c` and `mlp_c` give the critic's memory and MLP their own
sizes; `lds_stride`, `tile_of`, `buffer_strides` and `neuron_tiles` of tests/policy_edges.py, extended here to a memory-led sequence."""
from tests import policy_edges as pe
from tests.test_policy_recurrent_host import mem_dims, shared

SWEEP_N = 33
# The H sweep at the 32-row tile.  PAIRED, not crossed: row i gives memory_a H[i] and memory_c H[i + half], so every value runs in both
# kinds of workgroup.  An LSTM's gate layer has 4H neurons (NT 1 | 2 at H 16 | 17, 2 | 4 at 48 | 49), a GRU's (r, z) layer 2H (32 | 33,
# 96 | 97) and its n layers H (64 | 65).  H is also K2, the second operand's K: 1, 3 .. 15 have no full 16-wide chunk, 16 .. 64 are
# whole chunks, 17, 33, 49, 65, 97 a one-element tail behind them, 31 a 15-element one.  Depth alternates 2 / 1 and differs between the
# two memories of a row; H = 1 has TWO layers in memory_a of row 0 (its gate activation is pad4(1) + 1 = 5 wide, not 4).
SWEEP_H = {"lstm": (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65), "gru": (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 96, 97)}
SWEEP_OBS = (1, 2, 3, 4, 5, 15, 16, 17, 33)
ROWS = {}
for _kind, _hs in SWEEP_H.items():
    for _i, _h in enumerate(_hs):
        _hc = _hs[(_i + len(_hs) // 2) % len(_hs)]
        ROWS[f"sweep_{_kind}_{_h}_{_hc}"] = dict(kind=_kind, obs=SWEEP_OBS[_i % 9], cobs=SWEEP_OBS[(_i + 4) % 9], H=_h, H_c=_hc, layers=2 - _i % 2,
                                                 layers_c=1 + _i % 2, mlp=[33], mlp_c=[9], A=pe.SWEEP_A[_i % 5], R=32, sizes=(SWEEP_N,))


def _sizes(R):
    """A one-row tile, a full one, a full one plus one row, two full ones plus one row."""
    return (1, R, R + 1, 2 * R + 1)


# Tile thresholds, both memories alike (strides in floats: X = [x, padded | h_prev], G = the gates; 32 rows may take 1280, 16 rows 2560):
#   one LSTM layer   H 225: 324 + 900 = 1224 -> 32      H 226: 324 + 964 = 1288 -> 16      H 481: 580 + 1924 = 2504 -> 16      H 482: 580 + 1988 = 2568 -> 8
#   two GRU layers   H 145: G twice, 580 + 580 = 1160 -> 32      H 146: 644 + 644 = 1288 -> 16
#   two LSTM layers  H 512: 2052 + 2052 -> 8, the figure of DESIGN.md 10b
for _name, _kind, _layers, _h, _r in (("lstm_225", "lstm", 1, 225, 32), ("lstm_226", "lstm", 1, 226, 16), ("lstm_481", "lstm", 1, 481, 16),
                                      ("lstm_482", "lstm", 1, 482, 8), ("gru2_145", "gru", 2, 145, 32), ("gru2_146", "gru", 2, 146, 16),
                                      ("lstm2_512", "lstm", 2, 512, 8)):
    ROWS[_name] = dict(kind=_kind, obs=45, cobs=45, H=_h, layers=_layers, mlp=[32], A=3, R=_r, sizes=_sizes(_r))
# A small H at a small tile: a 2047-wide observation makes X 2116 floats, which with a 132-wide G fits 16 rows and not 32; in crit8 the
# critic's memory (580 + 2052) plans 8 rows and the actor's tiny one runs at them.
ROWS["wideobs_lstm"] = dict(kind="lstm", obs=2047, cobs=1301, H=20, H_c=7, layers=1, layers_c=2, mlp=[33], mlp_c=[9], A=5, R=16, sizes=_sizes(16))
ROWS["wideobs_gru"] = dict(kind="gru", obs=2047, cobs=1301, H=40, H_c=7, layers=2, layers_c=1, mlp=[33], mlp_c=[9], A=3, R=16, sizes=_sizes(16))
ROWS["crit8"] = dict(kind="gru", obs=5, cobs=45, H=7, H_c=512, layers=1, layers_c=1, mlp=[33], mlp_c=[32], A=3, R=8, sizes=_sizes(8))
for _name, _d in ROWS.items():
    _d["name"] = _name
CASES = [(name, n) for name, d in ROWS.items() for n in d["sizes"]]


# ---- the launch plan of a memory-led sequence, restated from the words of csrc/lg_policy.hip -------------------------------------------------
def pad4(w):
    return (w + 3) & ~3


def gate_width(H):
    """The gate activation: 4H, or the next rnn layer's [h', padded | h_prev] where that is wider (H = 1)."""
    return max(4 * H, pad4(H) + H)


def sequences(d):
    """The activation widths the policy's and the critic's workgroups walk: X = [x, padded to 4 floats | h_prev], the gates once per rnn
    layer, then the MLP's widths.  Activation i lives in buffer i & 1."""
    out = []
    for w, mlp, last in (("a", d["mlp"], d["A"]), ("c", d.get("mlp_c", d["mlp"]), 1)):
        inp, layers, H = mem_dims(d, w)
        out.append([pad4(inp) + H] + [gate_width(H)] * layers + list(mlp) + [last])
    return out


def planned_tile(d):
    return pe.tile_of(sequences(d))


def layers(d, w):
    """(K, M, K2) of every layer memory `w`'s sequence runs; K2: the second operand's K (0: the layer has one operand).  An LSTM's rnn
    layer is one layer of 4H neurons on x and h; a GRU's is (r, z) on both, n_x on x alone and n_h on h alone."""
    inp, n, H = mem_dims(d, w)
    out = []
    for _ in range(n):
        out += [(inp, 4 * H, H)] if d["kind"] == "lstm" else [(inp, 2 * H, H), (inp, H, 0), (H, H, 0)]
        inp = H
    widths = [H, *(d["mlp"] if w == "a" else d.get("mlp_c", d["mlp"])), d["A"] if w == "a" else 1]
    return out + [(k, m, 0) for k, m in zip(widths[:-1], widths[1:])]


def bodies(d):
    """The `layer_tile<RB, NT, TWO>` instantiations this row's launch reaches, as (RB, NT, two operands)."""
    rb = 2 if planned_tile(d) == 32 else 1
    return {(rb, pe.neuron_tiles(M)[1], bool(K2)) for w in "ac" for _, M, K2 in layers(d, w)}


def row_tags(d):
    """What a row reaches, as tags; tests/test_policy_recurrent_edges_host.py holds the union over the table to the list it must keep."""
    R = planned_tile(d)
    t = {f"R={R}"} | {f"<{rb},{nt},two>:{d['kind']}" for rb, nt, two in bodies(d) if two}
    t |= {f"R={R},N={what}" for n in d["sizes"] for what, at in (("1", 1), ("R", R), ("R+1", R + 1), ("2R+1", 2 * R + 1)) if n == at}
    dims = [mem_dims(d, w) for w in "ac"]
    for inp, n, H in dims:
        k2 = H % 16
        t.add("K2<16" if H < 16 else "K2%16=0" if k2 == 0 else "K2%16=1" if k2 == 1 else "K2%16=15" if k2 == 15 else "K2%16=other")
        t |= {tag for tag, on in (("H=1", H == 1), ("H=1,two-layers", H == 1 and n == 2), ("x_col[0]!=in", inp % 4 != 0),
                                  ("x_col[1]!=H", n == 2 and H % 4 != 0), ("two-layers", n == 2), (f"H={H}:{d['kind']}", True)) if on}
    t |= {tag for tag, i in (("uneven-in", 0), ("uneven-depth", 1), ("uneven-H", 2)) if dims[0][i] != dims[1][i]}
    return t


def edge_shared(name, n):
    """`shared` of tests/test_policy_recurrent_host.py for a row of this table: module, inputs, float64 oracle, float32 yardstick, once."""
    return shared(ROWS[name], n)

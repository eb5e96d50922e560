"""Host side of the recurrent fused policy step (LgPolicyMemory in include/lgpolicy.h, `describe` / `policy_args` of
hcr_genesis_lr_cl_amd/policy.py): the ctypes mirror of LgPolicyMemory and of the grown descriptor, LgPolicyRecurrentArgs, against the header, the descriptor of every recurrent net set, every refusal, and
the float32 numpy restatement of torch's LSTM / GRU cell that tests/test_gpu_policy_recurrent.py holds the kernel to -- with the proof that
the parity rule of tests/test_policy_host.py tells the usual cell mistakes from a summation order.  No GPU needed: nothing is launched.

The stand-in modules follow rsl_rl/modules/actor_critic_recurrent.py by duck typing (`is_recurrent`, `.memory_a.rnn`, `.memory_c.rnn`, `.actor`,
`.critic`, `.std`); the oracle is torch's own nn.LSTM / nn.GRU and the MLPs on the CPU in float64, from deep copies of the same module."""
import copy
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn as nn

from hcr_genesis_lr_cl_amd import abi, policy
from tests.test_policy_host import HEADER, max_err, mlp, np_forward, parity_bound

# obs, critic obs, rnn kind, rnn layers, H, hidden widths of actor and critic, actions
RNETS = {
    "tiny_lstm1": dict(obs=5, cobs=6, kind="lstm", layers=1, H=7, mlp=[33, 7], A=3),       # H = 7: no tile multiple, not a multiple of 4
    "tiny_lstm2": dict(obs=5, cobs=6, kind="lstm", layers=2, H=7, mlp=[33, 7], A=3),
    "tiny_gru1": dict(obs=5, cobs=6, kind="gru", layers=1, H=7, mlp=[33, 7], A=3),
    "tiny_gru2": dict(obs=5, cobs=6, kind="gru", layers=2, H=7, mlp=[33, 7], A=3),
    "go2_lstm": dict(obs=45, cobs=45, kind="lstm", layers=1, H=256, mlp=[256, 256, 256], A=12),
    "gru512": dict(obs=45, cobs=45, kind="gru", layers=1, H=512, mlp=[512, 256, 128], A=12),   # the width limit: the 8-row tile
}
ROW_TILE = {"tiny_lstm1": 32, "tiny_lstm2": 32, "tiny_gru1": 32, "tiny_gru2": 32, "go2_lstm": 16, "gru512": 8}
STEPS = 5
RESET_BEFORE = (2, 4)         # a reset mask is applied before these steps of the five


def net(name):
    """A net set: its RNETS name, or the dict itself (tests/policy_recurrent_edges.py has a table of its own, whose rows carry "name")."""
    return RNETS[name] if isinstance(name, str) else name


def net_key(name):
    return name if isinstance(name, str) else name["name"]


def mem_dims(d, w):
    """(input width, rnn layers, H) of memory_a (w = "a") or memory_c ("c"): the critic's takes the optional keys `layers_c` and `H_c`."""
    return (d["obs"], d["layers"], d["H"]) if w == "a" else (d["cobs"], d.get("layers_c", d["layers"]), d.get("H_c", d["H"]))


class Memory(nn.Module):
    """One time step of an rnn on its own hidden states (None: zeros), as the reference's Memory in inference mode."""

    def __init__(self, input_size, kind, layers, hidden):
        super().__init__()
        self.rnn = (nn.LSTM if kind == "lstm" else nn.GRU)(input_size, hidden, layers)
        self.hidden_states = None

    def forward(self, x):
        out, self.hidden_states = self.rnn(x.unsqueeze(0), self.hidden_states)
        return out.squeeze(0)

    def reset(self, dones):
        for h in self.hidden_states if isinstance(self.hidden_states, tuple) else (self.hidden_states,):
            h[..., dones, :] = 0.0


class RecurrentStandIn(nn.Module):
    """memory_a -> actor, memory_c -> critic from a net-set dict.  The optional keys `H_c`, `layers_c` and `mlp_c` give the critic's
    memory and MLP sizes of their own (default: `H`, `layers`, `mlp`, as in every RNETS row)."""
    is_recurrent = True

    def __init__(self, d, clip=None):
        super().__init__()
        (in_a, layers_a, H_a), (in_c, layers_c, H_c) = mem_dims(d, "a"), mem_dims(d, "c")
        self.memory_a = Memory(in_a, d["kind"], layers_a, H_a)
        self.memory_c = Memory(in_c, d["kind"], layers_c, H_c)
        self.actor = mlp(H_a, d["mlp"], d["A"], nn.Hardtanh(-clip, clip) if clip is not None else None)
        self.critic = mlp(H_c, d.get("mlp_c", d["mlp"]), 1)
        self.std = nn.Parameter(torch.ones(d["A"]))

    def mean(self, obs):
        return self.actor(self.memory_a(obs))

    def value(self, cobs):
        return self.critic(self.memory_c(cobs))

    def get_hidden_states(self):
        return self.memory_a.hidden_states, self.memory_c.hidden_states

    def reset(self, dones):
        self.memory_a.reset(dones)
        self.memory_c.reset(dones)


def make_rnet(name, clip=None, seed=3):
    """The recurrent net set `name`, seeded in the style of `make_net`: every weight matrix uniform +-1.5 / sqrt(in) (for the rnn `in` is the
    matrix's own column count), biases +-0.5, std in [0.5, 1.5).  No Hardtanh by default, so that every actor output carries the whole
    chain's error instead of saturating at the clip."""
    d = net(name)
    m = RecurrentStandIn(d, clip)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 2:
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * 1.5 / p.shape[1] ** 0.5)
            else:
                p.copy_(torch.rand(p.shape, generator=g) - 0.5)
        m.std.copy_(0.5 + torch.rand(d["A"], generator=g))
    return m


def state_keys(kind):
    return ("h_a", "c_a", "h_c", "c_c") if kind == "lstm" else ("h_a", "h_c")


def make_inputs(name, n, seed=11):
    """Seeded inputs of STEPS steps at batch size n: observations, injected noise, incoming states uniform +-1 and the two reset masks
    (row 0 is done in the first and alive in the second, so that N = 1 sees both)."""
    d = net(name)
    g = torch.Generator().manual_seed(seed)
    obs, cobs = torch.randn(STEPS, n, d["obs"], generator=g), torch.randn(STEPS, n, d["cobs"], generator=g)
    noise = torch.randn(STEPS, n, d["A"], generator=g)
    start = {k: torch.rand(mem_dims(d, k[-1])[1], n, mem_dims(d, k[-1])[2], generator=g) * 2 - 1 for k in state_keys(d["kind"])}
    masks = {t: torch.rand(n, generator=g) < 0.3 for t in RESET_BEFORE}
    masks[RESET_BEFORE[0]][0], masks[RESET_BEFORE[1]][0] = True, False
    return dict(obs=obs, cobs=cobs, noise=noise, start=start, masks=masks)


def load_states(m, start, dtype):
    """Give the stand-in's memories the states `start` (a dict by state_keys), as fresh tensors of `dtype`."""
    for mem, w in ((m.memory_a, "a"), (m.memory_c, "c")):
        h = start["h_" + w].to(dtype).clone()
        mem.hidden_states = (h, start["c_" + w].to(dtype).clone()) if "c_" + w in start else h


def read_states(m):
    out = {}
    for mem, w in ((m.memory_a, "a"), (m.memory_c, "c")):
        hs = mem.hidden_states
        if isinstance(hs, tuple):
            out["h_" + w], out["c_" + w] = hs[0].clone(), hs[1].clone()
        else:
            out["h_" + w] = hs.clone()
    return out


def torch_steps(m, inp, dtype, steps=STEPS):
    """The oracle (dtype float64) or the yardstick (float32): a deep copy of `m` in `dtype` run over the steps from the given states with
    the reset masks.  Per step a dict of numpy arrays: `pre` (states the step started from, after the reset), mu, values, actions,
    log_prob and the new states."""
    m = copy.deepcopy(m).to(dtype)
    load_states(m, inp["start"], dtype)
    out = []
    with torch.no_grad():
        for t in range(steps):
            if t in inp["masks"]:
                m.reset(inp["masks"][t])
            pre = read_states(m)
            mu, v = m.mean(inp["obs"][t].to(dtype)), m.value(inp["cobs"][t].to(dtype))
            sigma = mu * 0 + m.std
            actions = mu + sigma * inp["noise"][t].to(dtype)
            lp = torch.distributions.Normal(mu, sigma).log_prob(actions).sum(-1, keepdim=True)
            r = dict(mu=mu, values=v, actions=actions, log_prob=lp, **read_states(m))
            r = {k: x.numpy() for k, x in r.items()}
            r["pre"] = {k: x.numpy() for k, x in pre.items()}
            out.append(r)
    return out


# ---- float32 numpy restatement of the cells, with the deliberately wrong variants --------------------------------------------------------
VARIANTS = {"ifog": "lstm", "r_whole": "gru", "z_swapped": "gru", "no_bhh": None, "stale_layer": None}      # which kind a variant applies to
# what the state handling could get wrong (tests/test_policy_recurrent_edges_host.py runs them): a reset that zeroes h and leaves c; rnn
# layer 1 staged from layer 0's incoming h; the critic's run reading the actor's states (only where both have one shape)
STATE_VARIANTS = {"c_not_reset": "lstm", "prev_of_layer0": None, "swapped_memories": None}


def _sig(x):
    return (1.0 / (1.0 + np.exp(-x, dtype=np.float32))).astype(np.float32)


def np_memory_step(rnn, x, h, c, variant=None):
    """One time step of `rnn` (nn.LSTM / nn.GRU) on x (N, in) from states h (and c) (layers, N, H), all float32; returns (top h', h', c').
    `variant`: None, or one of VARIANTS -- gate order (i, f, o, g); r applied to the whole sum; z and 1 - z swapped; b_hh dropped; layer 2
    reading the OLD h of layer 1 -- or `prev_of_layer0` of STATE_VARIANTS: layer 1 starts from layer 0's incoming h."""
    lstm = isinstance(rnn, nn.LSTM)
    H = rnn.hidden_size
    f32 = lambda t: t.detach().numpy().astype(np.float32)
    h_new, c_new = np.empty_like(h), (np.empty_like(c) if lstm else None)
    x = np.asarray(x, np.float32)
    for k in range(rnn.num_layers):
        w_ih, w_hh, b_ih, b_hh = (f32(getattr(rnn, f"{n}_l{k}")) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
        if variant == "no_bhh":
            b_hh = np.zeros_like(b_hh)
        hk = h[0] if variant == "prev_of_layer0" else h[k]
        gx, gh = (x @ w_ih.T + b_ih).astype(np.float32), (hk @ w_hh.T + b_hh).astype(np.float32)
        if lstm:
            g = gx + gh
            order = (0, 1, 3, 2) if variant == "ifog" else (0, 1, 2, 3)
            i, f, gg, o = (g[:, q * H:(q + 1) * H] for q in order)
            c_new[k] = _sig(f) * c[k] + _sig(i) * np.tanh(gg)
            h_new[k] = _sig(o) * np.tanh(c_new[k])
        else:
            r, z = _sig(gx[:, :H] + gh[:, :H]), _sig(gx[:, H:2 * H] + gh[:, H:2 * H])
            n = np.tanh(r * (gx[:, 2 * H:] + gh[:, 2 * H:]) if variant == "r_whole" else gx[:, 2 * H:] + r * gh[:, 2 * H:])
            h_new[k] = z * n + (1 - z) * hk if variant == "z_swapped" else (1 - z) * n + z * hk
        x = h[k] if variant == "stale_layer" else h_new[k]
    return h_new[-1], h_new, c_new


def np_steps(m, inp, variant=None, steps=STEPS):
    """The numpy restatement of `torch_steps`' last step: mu, values and the states after `steps` steps.  `variant`: one of VARIANTS, or of
    STATE_VARIANTS."""
    st = {k: v.numpy().astype(np.float32).copy() for k, v in inp["start"].items()}
    for t in range(steps):
        if t in inp["masks"]:
            for k, v in st.items():
                if not (variant == "c_not_reset" and k.startswith("c_")):
                    v[:, inp["masks"][t].numpy()] = 0
        top, pre = {}, dict(st)                                  # the states this step starts from: a cell returns new arrays
        for w, mem, x in (("a", m.memory_a, inp["obs"][t]), ("c", m.memory_c, inp["cobs"][t])):
            src = "a" if variant == "swapped_memories" else w
            top[w], st["h_" + w], c = np_memory_step(mem.rnn, x.numpy(), pre["h_" + src], pre.get("c_" + src), variant)
            if c is not None:
                st["c_" + w] = c
    return dict(mu=np_forward(m.actor, top["a"]), values=np_forward(m.critic, top["c"]), **st)


_SHARED = {}


def shared(name, n):
    """Per (net set, N), computed once and left unchanged: the module, the inputs, the float64 oracle and the float32 yardstick."""
    key = (net_key(name), n)
    if key not in _SHARED:
        m, inp = make_rnet(name), make_inputs(name, n)
        _SHARED[key] = dict(module=m, inp=inp, ref=torch_steps(m, inp, torch.float64), f32=torch_steps(m, inp, torch.float32))
    return _SHARED[key]


# ---- the struct ---------------------------------------------------------------------------------------------------------------------------
def test_memory_struct_and_grown_args_match_header():
    structs = [("LgPolicyRnnLayer", abi.LgPolicyRnnLayer), ("LgPolicyMemory", abi.LgPolicyMemory), ("LgPolicyArgs", abi.LgPolicyArgs),
               ("LgPolicyRecurrentArgs", abi.LgPolicyRecurrentArgs)]      # a ctypes subclass: _fields_ lists the two memories, sizeof the whole
    consts = ["MAX_RNN_LAYERS", "MAX_RNN_HIDDEN", "LSTM", "GRU", "MAX_WIDTH"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs:
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += [f'printf("{c} %d\\n", (int)LG_POLICY_{c});' for c in consts]
    lines += ['printf("ARGS_AT %zu\\n", offsetof(LgPolicyRecurrentArgs, args));', "return 0;}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        with open(src, "w") as f:
            f.write("\n".join(lines))
        subprocess.run(["gcc", "-o", exe, src], check=True)
        got = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for cname, cls in structs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert [int(got[c]) for c in consts] == [abi.POLICY_MAX_RNN_LAYERS, abi.POLICY_MAX_RNN_HIDDEN, abi.POLICY_LSTM, abi.POLICY_GRU, abi.POLICY_MAX_WIDTH]
    assert 4 * abi.POLICY_MAX_RNN_HIDDEN == abi.POLICY_MAX_WIDTH                    # the gates of one cell are one activation
    # the two memories are APPENDED behind an unchanged LgPolicyArgs (C: `args` is the first member), and all-zero members mean "no memory"
    assert int(got["ARGS_AT"]) == 0
    A, R = abi.LgPolicyArgs, abi.LgPolicyRecurrentArgs
    assert issubclass(R, A) and R.memory_a.offset == C.sizeof(A) == A.head.offset + C.sizeof(abi.LgPolicyHead)
    assert R.memory_c.offset == R.memory_a.offset + C.sizeof(abi.LgPolicyMemory) and C.sizeof(R) == R.memory_c.offset + C.sizeof(abi.LgPolicyMemory)
    assert R.head.offset == A.head.offset and R().memory_a.kind == 0 and not hasattr(A, "memory_a")


def test_header_declares_the_reset_entry_point():
    declared = set(re.findall(r"\b(lg_\w+)\s*\(", open(HEADER).read()))
    assert declared == set(abi.POLICY_EXPORTS) and {"lg_policy_act_recurrent", "lg_policy_row_tile_recurrent", "lg_policy_reset"} <= declared
    lib = C.CDLL(abi.lib_path())
    for sym in declared:
        assert hasattr(lib, sym), sym


# ---- the descriptor -----------------------------------------------------------------------------------------------------------------------
def _memory_tensors(d, n, prev=False, mask=False):
    z = lambda k: torch.zeros(mem_dims(d, k[-1])[1], n, mem_dims(d, k[-1])[2])
    t = {k: z(k) for k in state_keys(d["kind"])}
    if prev:
        t.update({k.replace("_", "_prev_"): z(k) for k in state_keys(d["kind"])})
    if mask:
        t["reset"] = torch.zeros(n, dtype=torch.uint8)
    return t


def _args(m, d, n=7, flags=0, **mem_kw):
    spec = policy.describe(m)
    z = lambda w: torch.zeros(n, w)
    mem = _memory_tensors(d, n, **mem_kw)
    t = dict(obs=z(d["obs"]), cobs=z(d["cobs"]), actions=z(d["A"]), mu=z(d["A"]), sigma=z(d["A"]), log_prob=z(1), values=z(1), noise=z(d["A"]))
    if flags == abi.POLICY_DETERMINISTIC:
        a = policy.policy_args(spec, t["obs"], mu=t["mu"], flags=flags, memory={k: v for k, v in mem.items() if k.endswith("_a")})
    elif flags == abi.POLICY_VALUES_ONLY:
        a = policy.policy_args(spec, None, t["cobs"], values=t["values"], flags=flags, memory={k: v for k, v in mem.items() if k.endswith("_c")})
    else:
        a = policy.policy_args(spec, t["obs"], t["cobs"], t["actions"], t["mu"], t["sigma"], t["log_prob"], t["values"], noise=t["noise"], memory=mem)
    return spec, a, t, mem


@pytest.mark.parametrize("name", list(RNETS))
def test_describe_and_descriptor_of_recurrent_stand_ins(name):
    d, m = RNETS[name], make_rnet(name)
    spec, a, t, mem = _args(m, d, prev=True, mask=True)
    assert spec.family == "recurrent" and spec.chain_order == ["memory_a", "actor", "memory_c", "critic"]
    assert (spec.memory_a.kind, spec.memory_c.kind) == (d["kind"], d["kind"]) and (spec.memory_a.layers, spec.memory_a.hidden) == (d["layers"], d["H"])
    assert (spec.obs_width, spec.critic_obs_width, spec.num_actions) == (d["obs"], d["cobs"], d["A"]) and not spec.concat
    kind = abi.POLICY_LSTM if d["kind"] == "lstm" else abi.POLICY_GRU
    for ma, mod, w, src in ((a.memory_a, m.memory_a, "a", t["obs"]), (a.memory_c, m.memory_c, "c", t["cobs"])):
        assert (ma.kind, ma.n_layers, ma.hidden, ma.in_width, ma.in_stride) == (kind, d["layers"], d["H"], src.shape[1], src.shape[1])
        assert ma.input == src.data_ptr()
        for k in range(d["layers"]):                                                   # every parameter where torch keeps it
            for f in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                assert getattr(ma.layer[k], f) == getattr(mod.rnn, f"{f}_l{k}").data_ptr(), (w, k, f)
        for k in range(d["layers"], abi.POLICY_MAX_RNN_LAYERS):
            assert ma.layer[k].weight_ih is None
        assert ma.h == mem["h_" + w].data_ptr() and ma.h_prev_out == mem["h_prev_" + w].data_ptr() and ma.reset_mask == mem["reset"].data_ptr()
        if d["kind"] == "lstm":
            assert ma.c == mem["c_" + w].data_ptr() and ma.c_prev_out == mem["c_prev_" + w].data_ptr()
        else:
            assert ma.c is None and ma.c_prev_out is None
    assert a.actor.layer[0].n_in == d["H"] and a.critic.layer[0].n_in == d["H"] and a.estimator.n_layers == 0 and a.head.H == 0
    assert isinstance(a, abi.LgPolicyRecurrentArgs)
    assert abi.load_lib().lg_policy_row_tile_recurrent(C.byref(a)) == ROW_TILE[name]   # the launch plan alone: nothing is enqueued


def test_descriptor_modes_and_views():
    d, m = RNETS["tiny_lstm2"], make_rnet("tiny_lstm2")
    _, a, _, _ = _args(m, d, flags=abi.POLICY_DETERMINISTIC)
    assert a.memory_a.kind == abi.POLICY_LSTM and a.memory_c.kind == 0 and a.critic.n_layers == 0 and a.memory_a.h_prev_out is None
    _, a, _, _ = _args(m, d, flags=abi.POLICY_VALUES_ONLY)
    assert a.memory_a.kind == 0 and a.memory_c.kind == abi.POLICY_LSTM and a.actor.n_layers == 0 and a.memory_c.reset_mask is None
    spec = policy.describe(m)
    wide, mem = torch.zeros(4, 64), _memory_tensors(d, 4)                              # a strided observation view is addressed in place
    z = lambda w: torch.zeros(4, w)
    a = policy.policy_args(spec, wide[:, 8:13], wide[:, 32:38], z(3), z(3), z(3), z(1), z(1), noise=z(3), memory=mem)
    assert (a.memory_a.input, a.memory_a.in_stride, a.memory_c.input, a.memory_c.in_stride) == (wide.data_ptr() + 32, 64, wide.data_ptr() + 128, 64)
    with pytest.raises(ValueError, match="h_a must be a contiguous"):
        policy.policy_args(spec, z(5), z(6), z(3), z(3), z(3), z(1), z(1), noise=z(3), memory=dict(mem, h_a=torch.zeros(2, 5, 7)))
    with pytest.raises(ValueError, match="state c_c of memory_c is missing"):
        policy.policy_args(spec, z(5), z(6), z(3), z(3), z(3), z(1), z(1), noise=z(3), memory={k: v for k, v in mem.items() if k != "c_c"})
    with pytest.raises(ValueError, match="reset must be a mask"):
        policy.policy_args(spec, z(5), z(6), z(3), z(3), z(3), z(1), z(1), noise=z(3), memory=dict(mem, reset=torch.tensor([0, 2])))
    g = make_rnet("tiny_gru1")
    with pytest.raises(ValueError, match="c_a was given, memory_a.rnn is a GRU"):
        policy.policy_args(policy.describe(g), z(5), z(6), z(3), z(3), z(3), z(1), z(1), noise=z(3),
                           memory=dict(_memory_tensors(RNETS["tiny_gru1"], 4), c_a=torch.zeros(1, 4, 7)))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _with_rnn(rnn, name="tiny_lstm1", which="memory_a"):
    m = make_rnet(name)
    getattr(m, which).rnn = rnn
    return m


@pytest.mark.parametrize("match,build", [
    (r"memory_a\.rnn is bidirectional", lambda: _with_rnn(nn.LSTM(5, 7, bidirectional=True))),
    (r"memory_a\.rnn has proj_size=3", lambda: _with_rnn(nn.LSTM(5, 7, proj_size=3))),
    (r"memory_c\.rnn has dropout=0\.5", lambda: _with_rnn(nn.LSTM(6, 7, 2, dropout=0.5), "tiny_lstm2", "memory_c")),
    (r"memory_a\.rnn has bias=False", lambda: _with_rnn(nn.GRU(5, 7, bias=False), "tiny_gru1")),
    (r"memory_a\.rnn has batch_first=True", lambda: _with_rnn(nn.GRU(5, 7, batch_first=True), "tiny_gru1")),
    (r"memory_c\.rnn has num_layers=3", lambda: _with_rnn(nn.LSTM(6, 7, 3), which="memory_c")),
    (r"memory_a\.rnn has hidden_size=513", lambda: _with_rnn(nn.LSTM(5, 513))),
    (r"memory_a\.rnn is an LSTM, memory_c\.rnn a GRU", lambda: _with_rnn(nn.GRU(6, 7), which="memory_c")),
    (r"memory_a\.rnn is Linear", lambda: _with_rnn(nn.Linear(5, 7))),
    (r"memory_a\.rnn\.weight_ih_l0 is torch\.float64", lambda: _with_rnn(nn.LSTM(5, 7).double())),
    (r"actor\[0\] takes 7 inputs \(in_features\), memory_a\.rnn gives hidden_size = 8", lambda: _with_rnn(nn.LSTM(5, 8))),
    (r"critic\[0\] takes 7 inputs \(in_features\), memory_c\.rnn gives hidden_size = 9", lambda: _with_rnn(nn.GRU(6, 9), "tiny_gru1", "memory_c")),
])
def test_describe_refusals_name_the_attribute(match, build):
    with pytest.raises(ValueError, match=match):
        policy.describe(build())


def test_describe_refuses_parameters_the_kernel_cannot_read_in_place():
    m = make_rnet("tiny_gru2")
    m.memory_c.rnn.weight_ih_l1.data = torch.zeros(7, 21).t()
    with pytest.raises(ValueError, match=r"memory_c\.rnn\.weight_ih_l1 is not contiguous"):
        policy.describe(m)
    with pytest.raises(ValueError, match=r"memory_a\.rnn\.weight_ih_l0 is on cpu"):
        policy.describe(make_rnet("tiny_gru2"), torch.device("cuda:0"))


def test_describe_refuses_a_memory_beside_another_family():
    for attr, mod in (("estimator", mlp(5, [4], 2)), ("privilege_encoder", mlp(5, [4], 2)), ("history_encoder", mlp(5, [4], 2)), ("vae", nn.Module())):
        m = make_rnet("tiny_lstm1")
        setattr(m, attr, mod)
        with pytest.raises(ValueError, match=rf"a memory together with \.{attr}"):
            policy.describe(m)


def test_recurrent_without_memories_is_still_refused():
    m = make_rnet("tiny_lstm1")
    del m.memory_c
    with pytest.raises(ValueError, match="recurrent.*memory_a and .memory_c"):
        policy.describe(m)

    class Other(nn.Module):
        is_recurrent = True
    with pytest.raises(ValueError, match="recurrent"):
        policy.describe(Other())


def test_host_entry_point_refuses_a_bad_memory_before_a_launch():
    """What gets past Python meets the entry point's own checks; nothing is enqueued (there is no device here)."""
    lib = abi.load_lib()
    refused = lambda a, msg: lib.lg_policy_row_tile_recurrent(C.byref(a)) == 0 and msg in lib.lg_last_error()
    for name in ("tiny_lstm2", "tiny_gru2"):
        d, m = RNETS[name], make_rnet(name)
        keep = []

        def mk():
            _, a, t, mem = _args(m, d, prev=True, mask=True)
            keep.append((t, mem))
            return a
        assert lib.lg_policy_row_tile_recurrent(C.byref(mk())) == 32
        assert lib.lg_policy_act_recurrent(None, None) != 0 and b"null descriptor" in lib.lg_last_error()
        a = mk(); a.memory_a.kind = 3
        assert refused(a, b"memory_a: unknown kind 3")
        a = mk(); a.memory_c.n_layers = 3
        assert refused(a, b"memory_c: 1 .. 2 rnn layers")
        a = mk(); a.memory_a.hidden = 513
        assert refused(a, b"memory_a: hidden size outside [1, 512]")
        a = mk(); a.memory_a.hidden = 0
        assert refused(a, b"memory_a: hidden size outside [1, 512]")
        a = mk(); a.memory_c.layer[1].bias_hh = None
        assert refused(a, b"memory_c: null weight or bias in rnn layer 1")
        a = mk(); a.memory_a.h = None
        assert refused(a, b"memory_a: null state h")
        a = mk(); a.memory_a.input = None
        assert refused(a, b"memory_a: null input")
        a = mk(); a.memory_a.hidden = 8
        assert refused(a, b"actor: layer 0 takes 7 inputs, its input has 8")
        a = mk(); a.memory_c.hidden = 6
        assert refused(a, b"critic: layer 0 takes 7 inputs, its input has 6")
        if d["kind"] == "lstm":
            a = mk(); a.memory_c.c = None
            assert refused(a, b"memory_c: an LSTM without its cell state c")
        else:
            a = mk(); a.memory_a.c = a.memory_a.h
            assert refused(a, b"memory_a: a GRU has no cell state")
        a = mk(); a.estimator = a.critic
        assert refused(a, b"memory_a together with the estimator, encoder_b or the VAE head")
        a = mk(); a.head.H, a.head.L, a.head.E = 4, 2, 2
        assert refused(a, b"memory_a together with")
        a = mk(); a.flags = 4
        assert refused(a, b"bad flags")                                                # no new flag bit
        a = mk(); a.memory_a.kind = 3
        assert lib.lg_policy_reset(C.byref(a), None, None) != 0 and b"lg_policy_reset: memory_a: unknown kind 3" in lib.lg_last_error()
    plain = abi.LgPolicyRecurrentArgs()
    plain.n_envs = 4
    assert lib.lg_policy_reset(C.byref(plain), None, None) != 0 and b"the descriptor has no memory" in lib.lg_last_error()


# ---- the cells: restatement, parity rule, discrimination --------------------------------------------------------------------------------
HOST_N = 33
LAST_KEYS = ("mu", "values", "h_a", "c_a", "h_c", "c_c")


def _errs(name, got):
    s = shared(name, HOST_N)
    ref, f32 = s["ref"][-1], s["f32"][-1]
    out = {}
    for k in LAST_KEYS:
        if k in ref:
            out[k] = (max_err(got[k], ref[k]), parity_bound(max_err(f32[k], ref[k]), ref[k]))
    return out


@pytest.mark.parametrize("name", list(RNETS))
def test_numpy_cells_agree_with_the_float64_oracle(name):
    """Five consecutive steps with a reset before steps 2 and 4: another float32 evaluation order of the same cells stays within the rule."""
    s = shared(name, HOST_N)
    assert all(s["inp"]["masks"][t].any() and not s["inp"]["masks"][t].all() for t in RESET_BEFORE)
    for k, (e, b) in _errs(name, np_steps(s["module"], s["inp"])).items():
        print(f"numpy cells {name} {k}: err {e:.3e} bound {b:.3e}")
        assert e <= b, (k, e, b)
    pre = s["ref"][RESET_BEFORE[0]]["pre"]["h_a"]
    assert not pre[:, s["inp"]["masks"][RESET_BEFORE[0]].numpy()].any() and pre.any()          # the oracle's reset took the masked rows only


# every (set, mistake) pair in which the mistake exists: a gate order only for an LSTM, r and z only for a GRU, a stale layer only with two
WRONG = [(n, v) for n in ("tiny_lstm1", "tiny_lstm2", "tiny_gru1", "tiny_gru2", "go2_lstm") for v, kind in VARIANTS.items()
         if kind in (None, RNETS[n]["kind"]) and (v != "stale_layer" or RNETS[n]["layers"] == 2)]


@pytest.mark.parametrize("name,variant", WRONG)
def test_parity_rule_fails_the_wrong_cells(name, variant):
    """Each deliberately wrong cell exceeds the bound in the states AND in the outputs, so the GPU tests can tell it from rounding."""
    s = shared(name, HOST_N)
    errs = _errs(name, np_steps(s["module"], s["inp"], variant))
    for k in ("mu", "values", "h_a", "h_c"):
        e, b = errs[k]
        print(f"wrong cell {variant} {name} {k}: err {e:.3e} bound {b:.3e} ratio {e / b:.1f}")
        assert e > b, (k, e, b)

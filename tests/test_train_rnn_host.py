"""Host side of the recurrent learner pass (hcr_genesis_lr_cl_amd/train.py's FusedTrainPassRecurrent, include/lgtrainrnn.h): the ctypes mirror
against the header, the exports and the translation unit, the plan of lg_train_rnn_plan against the restated rules, every refusal of the
entry points and of describe_recurrent / rnn_args, the float64 restatement of tests/train_rnn_cases.py against torch's own nn.LSTM / nn.GRU
and autograd and against the golden fixtures of the reference's PPO.update() on ActorCriticRecurrent, the float32 restatement in the
kernels' order of sums under half the parity rule, ten planted defects that the rule must catch by a large factor, and the seed conditions
of the fixtures.  No GPU needed: nothing is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from hcr_genesis_lr_cl_amd import abi, train
from tests import optim_cases as oc
from tests import ppo_loss_cases as pc
from tests import train_abi as ta
from tests import train_rnn_cases as rc
from tests import train_support as sup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lgtrainrnn.h")
CSRC = os.path.join(ROOT, "hcr_genesis_lr_cl_amd", "csrc")
OWNER = "FusedTrainPassRecurrent"


# ---- the structs --------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header():
    structs = [("LgTrainRnnArgs", abi.LgTrainRnnArgs), ("LgTrainRnnPlan", abi.LgTrainRnnPlan), ("LgTrainRnnMemory", abi.LgTrainRnnMemory),
               ("LgTrainRnnLayer", abi.LgTrainRnnLayer), ("LgTrainArgs", abi.LgTrainArgs), ("LgTrainPlan", abi.LgTrainPlan)]
    consts = dict(LG_TRAIN_RNN_MEMORIES=abi.TRAIN_RNN_MEMORIES, LG_TRAIN_RNN_MAX_LAYERS=abi.TRAIN_RNN_MAX_LAYERS, LG_TRAIN_RNN_MAX_HIDDEN=abi.TRAIN_RNN_MAX_HIDDEN,
                  LG_TRAIN_RNN_LSTM=abi.TRAIN_RNN_LSTM, LG_TRAIN_RNN_GRU=abi.TRAIN_RNN_GRU, LG_TRAIN_RNN_TARGET_JOBS=abi.TRAIN_RNN_TARGET_JOBS,
                  LG_POLICY_MAX_LAYERS=abi.POLICY_MAX_LAYERS)
    ta.check_layout(HEADER, structs, consts)
    assert (abi.TRAIN_RNN_MAX_LAYERS, abi.TRAIN_RNN_MAX_HIDDEN, abi.TRAIN_RNN_LSTM, abi.TRAIN_RNN_GRU) == \
        (abi.POLICY_MAX_RNN_LAYERS, abi.POLICY_MAX_RNN_HIDDEN, abi.POLICY_LSTM, abi.POLICY_GRU)               # what FusedPolicy rolls out
    assert (rc.TARGET_JOBS, rc.MAX_LAYERS, rc.MAX_HIDDEN) == (abi.TRAIN_RNN_TARGET_JOBS, abi.TRAIN_RNN_MAX_LAYERS, abi.TRAIN_RNN_MAX_HIDDEN)


def test_library_exports_the_entry_points():
    declared = ta.check_exports(HEADER, abi.TRAIN_RNN_EXPORTS, "lg_train_rnn", ["lg_train_tiles.h", "lg_train_pass.h"])
    assert declared == {"lg_train_rnn_plan", "lg_train_rnn_forward", "lg_train_rnn_backward"}
    from hcr_genesis_lr_cl_amd import build
    assert f"{len(build.units())} translation units" in build.__doc__
    assert "TRAIN_RNN_EXPORTS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()         # the build's export check covers the list
    # one copy of the layer and pass routines: the unit includes the shared header and defines none of them
    src = open(os.path.join(CSRC, "lg_train_rnn.hip")).read()
    for fn in ("stage_rows", "copy_out", "fwd_tile", "bwd_tile", "wgrad_wave", "colsum_wave", "combine_layer", "combine_cols", "lds_stride", "slice_rule",
               "chain_forward", "chain_from_rows", "chain_backward", "bwd_layer", "seed_last_g", "store_sigma", "wgrad_job", "combine_all", "plan_chain",
               "plan_layout", "plan_out", "bind_chain", "bind_heads", "check_ws", "done", "raise_lds", "launch_tile"):
        assert '#include "lg_train_pass.h"' in src and not re.findall(r"\b(?:void|int|lds_f \*) ?" + fn + r"\(", src), fn
        assert fn in src or fn in ("colsum_wave", "combine_cols", "chain_forward", "check_ws"), fn                # and uses them
    assert "atomic" not in src.lower()                                                           # determinism is the house rule
    assert "train_rnn" in open(os.path.join(ROOT, "tools", "register_table.py")).read()


# ---- a descriptor on the host -------------------------------------------------------------------------------------------------------------
_KEEP = []          # the tensors a descriptor points to


def descriptor(x, backward=True):
    """LgTrainRnnArgs of a case through train.rnn_args on CPU tensors (device None): every pointer is real, nothing is launched."""
    m = rc.Recurrent(x)
    spec = train.describe_recurrent(m)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    hid = []
    for w in "ac":
        h = [t(x["h0_" + w])] + ([t(x["c0_" + w])] if x["kind"] == "lstm" else [])
        hid.append(h if len(h) > 1 else h[0])
    N, A = x["T"] * x["E"], x["A"]
    outs = [torch.zeros(N, A), torch.zeros(N, A), torch.zeros(N, 1)]
    pl = train.plan_rnn(N, x["max_len"], x["n_traj"], x["T"], x["kind"], [(x["layers"], x["H"], o) for o in x["obs_widths"]], x["actor_widths"], x["critic_widths"])
    ws = torch.zeros(int(pl.workspace_floats))
    grads = [torch.zeros_like(p) for p in spec.parameters()] if backward else None
    cot = [t(x[k]) for k in ("grad_mu", "grad_sigma", "grad_values")] if backward else []
    tensors = [t(x["obs"]), t(x["critic_obs"]), t(x["masks"]), tuple(hid)]
    _KEEP.append((m, tensors, outs, ws, grads, cot))
    return train.rnn_args(spec, *tensors, x["E"], *outs, ws, grads, *cot), pl, spec


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
GO2 = dict(kind="lstm", layers=1, H=256, obs=(45, 61), actor=[256, 512, 256, 128, 12], critic=[256, 512, 256, 128, 1])


def _check_plan(N, max_len, n_traj, T, kind, mem, actor, critic):
    p, want = train.plan_rnn(N, max_len, n_traj, T, kind, mem, actor, critic), rc.plan(N, max_len, n_traj, T, kind, mem, actor, critic)
    for k in ("time_row_tile", "time_lds_bytes", "time_tiles", "n_envs", "weight_jobs", "index_off", "workspace_floats"):
        assert getattr(p, k) == want[k], k
    for k in ("gate_off", "h_off", "hprev_off", "c_off", "nh_off", "dout_off", "dx_off", "dh_off"):
        assert [list(v) for v in getattr(p, k)] == want[k], k
    for k in ("slices", "slice_rows", "p_off"):
        got = [[list(w) for w in m] for m in getattr(p, k)]
        assert all(got[mi][l] == want[k][mi][l] for mi in range(2) for l in range(mem[mi][0])), k
    t = want["train"]
    assert (p.train.row_tile, p.train.lds_bytes, p.train.std_slices, p.train.std_slice_rows, p.train.std_p_off, p.train.weight_jobs, p.train.workspace_floats) == \
        (t["row_tile"], t["lds_bytes"], t["std_slices"], t["std_slice_rows"], t["std_p_off"], t["weight_jobs"], t["workspace_floats"])
    for ci, c in enumerate((actor, critic)):
        n = len(c) - 1
        for k in ("slices", "slice_rows", "h_off", "g_off", "p_off"):
            assert list(getattr(p.train, k)[ci])[:n] == t[k][ci], k
    return p


@pytest.mark.parametrize("name", list(rc.CASES))
def test_plan_matches_the_restated_rules(name):
    x = rc.make_inputs(name)
    _check_plan(x["T"] * x["E"], x["max_len"], x["n_traj"], x["T"], x["kind"], [(x["layers"], x["H"], o) for o in x["obs_widths"]], x["actor_widths"],
                x["critic_widths"])


def test_plan_of_the_go2_set_and_of_the_limits():
    mem = [(1, 256, 45), (1, 256, 61)]
    p = _check_plan(24 * 1024, 24, 1100, 24, "lstm", mem, GO2["actor"], GO2["critic"])
    assert (p.time_row_tile, p.time_tiles, p.train.row_tile) == (16, 69, 16)              # 4 H = 1024 gate columns beside 2 x 256 (time loop), beside 512 (row tiles)
    # H = 512 runs at 8 trajectories; uneven memories take the larger need; the widest input the smallest row tile
    assert _check_plan(48, 6, 9, 6, "lstm", [(2, 512, 2048), (1, 64, 5)], [512, 8, 2], [64, 8, 1]).time_row_tile == 8
    assert _check_plan(48, 6, 9, 6, "gru", [(1, 512, 7), (2, 512, 9)], [512, 8, 2], [512, 8, 1]).time_row_tile == 8
    assert _check_plan(48, 6, 9, 6, "gru", [(1, 128, 7), (1, 128, 9)], [128, 8, 2], [128, 8, 1]).time_row_tile == 32
    assert _check_plan(48, 6, 9, 6, "lstm", [(1, 256, 7), (1, 200, 9)], [256, 8, 2], [200, 8, 1]).time_row_tile == 16


# ---- the refusals of the entry points -----------------------------------------------------------------------------------------------------
def _good():
    return descriptor(rc.make_inputs("lstm2_h17_short"))[0]


_X = rc.make_inputs("lstm2_h17_short")
_N, _NT, _T, _ML = _X["T"] * _X["E"], _X["n_traj"], _X["T"], _X["max_len"]
MA, MC = "memory[0] (memory_a)", "memory[1] (memory_c)"
REFUSALS = [
    (ta.set_path(("train", "n_rows"), 0), "n_rows = 0 < 1", "pfb"),
    (ta.set_path(("memory", 0, "kind"), 3), f"{MA}.kind = 3 is neither LG_TRAIN_RNN_LSTM nor LG_TRAIN_RNN_GRU", "pfb"),
    (ta.set_path(("memory", 1, "n_layers"), 3), f"{MC}.n_layers = 3 is outside [1, 2]", "pfb"),
    (ta.set_path(("memory", 0, "n_layers"), 0), f"{MA}.n_layers = 0 is outside [1, 2]", "pfb"),
    (ta.set_path(("memory", 0, "hidden"), 513), f"{MA}.hidden = 513 is outside [1, 512]", "pfb"),
    (ta.set_path(("memory", 1, "n_in"), 2049), f"{MC}.n_in = 2049 is outside [1, 2048]", "pfb"),
    (ta.set_path(("memory", 0, "T"), 0), f"{MA}.T = 0 < 1", "pfb"),
    (ta.set_path(("memory", 0, "n_traj"), 0), f"{MA}.n_traj = 0 < 1", "pfb"),
    (ta.set_path(("memory", 0, "max_len"), _T + 1), f"{MA}.max_len = {_T + 1} is outside [1, {_T}] (1, T)", "pfb"),
    (ta.set_path(("memory", 1, "n_traj"), _NT + 1), f"{MC}: max_len, n_traj, T = {_ML}, {_NT + 1}, {_T}, but memory[0] has {_ML}, {_NT}, {_T}", "pfb"),
    (ta.set_path(("train", "n_rows"), _N + 1), f"n_rows = {_N + 1} is no multiple of T = {_T}", "pfb"),
    (ta.set_path(("train", "n_rows"), _T * (_NT + 1)), f"n_traj = {_NT} is outside [{_NT + 1}, {_T * (_NT + 1)}] (n_rows / T envs, n_rows steps)", "pfb"),
    (ta.set_path(("train", "chain", 0, "layer", 0, "n_in"), 18), f"chain[0] (actor).layer[0].n_in = 18, but {MA}.hidden = 17", "pfb"),
    (ta.set_path(("train", "chain", 1, "n_layers"), 0), "chain[1] (critic).n_layers = 0 is outside [1, 4]", "pfb"),
    (ta.set_path(("train", "chain", 1, "layer", 1, "n_in"), 21), "chain[1] (critic).layer[1].n_in = 21, but its input has 20 columns", "pfb"),
    (ta.set_path(("memory", 0, "layer", 0, "weight_ih"), None), f"{MA}.layer[0].weight_ih is null", "fb"),
    (ta.set_path(("memory", 0, "layer", 1, "weight_hh"), None), f"{MA}.layer[1].weight_hh is null", "fb"),
    (ta.set_path(("memory", 1, "layer", 0, "bias_ih"), None), f"{MC}.layer[0].bias_ih is null", "fb"),
    (ta.set_path(("memory", 1, "layer", 1, "bias_hh"), None), f"{MC}.layer[1].bias_hh is null", "fb"),
    (ta.set_path(("memory", 1, "x"), None), f"{MC}.x is null", "fb"),
    (ta.set_path(("memory", 0, "h0"), None), f"{MA}.h0 is null", "fb"),
    (ta.set_path(("memory", 0, "c0"), None), f"{MA}.c0 is null", "fb"),
    (ta.set_path(("memory", 0, "mask"), None), f"{MA}.mask is null", "fb"),
    (ta.set_path(("memory", 0, "x_row_stride"), 10), f"{MA}.x_row_stride = 10 is below its width 11", "fb"),
    (ta.set_path(("memory", 0, "x_time_stride"), -1), f"{MA}.x_time_stride = -1 < 0", "fb"),
    (ta.set_path(("memory", 1, "h0_row_stride"), 16), f"{MC}.h0_row_stride = 16 is below its width 17", "fb"),
    (ta.set_path(("memory", 1, "h0_layer_stride"), -1), f"{MC}.h0_layer_stride = -1 < 0", "fb"),
    (ta.set_path(("memory", 1, "c0_row_stride"), 16), f"{MC}.c0_row_stride = 16 is below its width 17", "fb"),
    (ta.set_path(("memory", 1, "c0_layer_stride"), -1), f"{MC}.c0_layer_stride = -1 < 0", "fb"),
    (ta.set_path(("memory", 0, "mask_time_stride"), _NT - 1), f"{MA}.mask_time_stride = {_NT - 1} is below n_traj = {_NT}", "fb"),
    (ta.set_path(("memory", 1, "mask"), 64), f"{MC}.mask is not memory[0]'s mask", "fb"),
    (ta.set_path(("train", "chain", 0, "layer", 0, "weight"), None), "chain[0] (actor).layer[0].weight is null", "fb"),
    (ta.set_path(("train", "chain", 1, "layer", 1, "bias"), None), "chain[1] (critic).layer[1].bias is null", "fb"),
    (ta.set_path(("train", "std"), None), "std is null", "fb"),
    (ta.set_path(("train", "mu"), None), "mu is null", "fb"),
    (ta.set_path(("train", "sigma_stride"), 2), "sigma_stride = 2 is below its width 3", "fb"),
    (ta.set_path(("train", "clip_actions"), -1.0), "clip_actions must be >= 0 under clip_on", "fb"),
    (ta.set_path(("train", "workspace"), None), "workspace is null", "fb"),
    (ta.set_path(("train", "workspace_capacity"), 100), "workspace_capacity = 100 floats is below the plan's", "fb"),
    (ta.set_path(("memory", 0, "layer", 0, "grad_weight_ih"), None), f"{MA}.layer[0].grad_weight_ih is null", "b"),
    (ta.set_path(("memory", 1, "layer", 1, "grad_bias_hh"), None), f"{MC}.layer[1].grad_bias_hh is null", "b"),
    (ta.set_path(("train", "chain", 0, "layer", 0, "grad_weight"), None), "chain[0] (actor).layer[0].grad_weight is null", "b"),
    (ta.set_path(("train", "grad_std"), None), "grad_std is null", "b"),
    (ta.set_path(("train", "grad_mu"), None), "grad_mu is null", "b"),
    (ta.set_path(("train", "grad_values_stride"), 0), "grad_values_stride = 0 is below its width 1", "b"),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_entry_points_refuse(i):
    ta.refuse([(m, msg.encode(), who) for m, msg, who in REFUSALS], i, _good, "lg_train_rnn", abi.LgTrainRnnPlan)


def test_null_descriptor_and_plan_are_refused():
    lib = abi.load_lib()
    a = _good()
    assert lib.lg_train_rnn_plan(None, C.byref(abi.LgTrainRnnPlan())) != 0 and lib.lg_last_error() == b"lg_train_rnn_plan: null descriptor"
    assert lib.lg_train_rnn_plan(C.byref(a), None) != 0 and lib.lg_last_error() == b"lg_train_rnn_plan: null plan"
    assert lib.lg_train_rnn_forward(None, None) != 0 and lib.lg_last_error() == b"lg_train_rnn_forward: null descriptor"
    assert lib.lg_train_rnn_backward(None, None) != 0 and lib.lg_last_error() == b"lg_train_rnn_backward: null descriptor"
    # an 8-trajectory tile always fits at H <= 512; the chains' own LDS refusal still reaches through
    assert lib.lg_train_rnn_plan(C.byref(a), C.byref(abi.LgTrainRnnPlan())) == 0


def test_descriptor_addresses_everything_in_place():
    x = rc.make_inputs("gru2_h65_t2")
    a, pl, spec = descriptor(x)
    m, tensors = _KEEP[-1][0], _KEEP[-1][1]
    assert a.memory[0].x == tensors[0].data_ptr() and a.memory[1].x == tensors[1].data_ptr() and a.memory[0].mask == a.memory[1].mask == tensors[2].data_ptr()
    assert (a.memory[0].x_time_stride, a.memory[0].x_row_stride) == (x["n_traj"] * 5, 5) and a.memory[1].h0 == tensors[3][1].data_ptr()
    assert a.memory[1].layer[1].weight_hh == m.memory_c.rnn.weight_hh_l1.data_ptr() and not a.memory[0].c0
    assert (a.train.n_rows, a.memory[0].max_len, a.memory[0].n_traj, a.memory[0].T) == (x["T"] * x["E"], x["max_len"], x["n_traj"], x["T"])
    assert [p.data_ptr() for p in spec.parameters()] == [p.data_ptr() for p in m.parameters()] and spec.parameter_names() == x["names"]


# ---- the refusals of the Python side ------------------------------------------------------------------------------------------------------
def _module(**change):
    x = rc.make_inputs("gru1_h7_none")
    m = rc.Recurrent(x)
    for k, v in change.items():
        obj, _, attr = k.rpartition("__")
        setattr(m if not obj else getattr(m, obj), attr, v)
    return m


MODULE_REFUSALS = [
    (lambda: _module(is_recurrent=False), "the module is not recurrent (is_recurrent); FusedTrainPass is the pass of the plain ActorCritic"),
    (lambda: _module(memory_c=None), "a recurrent policy (actor_critic.is_recurrent) needs .memory_a and .memory_c, each with an nn.LSTM or nn.GRU as .rnn; other "
                                     "recurrent modules keep the torch path"),
    (lambda: _module(estimator=nn.Linear(2, 2)), "a memory together with .estimator; memories are built for the plain actor-critic only"),
    (lambda: _module(memory_a__rnn=nn.RNN(11, 7)), "memory_a.rnn is RNN, expected an nn.LSTM or nn.GRU"),
    (lambda: _module(memory_a__rnn=nn.GRU(11, 7, bidirectional=True)), "memory_a.rnn is bidirectional; a rollout step has no backward direction"),
    (lambda: _module(memory_c__rnn=nn.LSTM(13, 7, proj_size=3)), "memory_c.rnn has proj_size=3; projections are not built into the kernel"),
    (lambda: _module(memory_c__rnn=nn.GRU(13, 7, num_layers=2, dropout=0.5)), "memory_c.rnn has dropout=0.5; dropout between rnn layers is not built into the kernel"),
    (lambda: _module(memory_a__rnn=nn.GRU(11, 7, bias=False)), "memory_a.rnn has bias=False; the kernel reads bias_ih and bias_hh"),
    (lambda: _module(memory_a__rnn=nn.GRU(11, 7, batch_first=True)), "memory_a.rnn has batch_first=True; the reference's Memory feeds (1, N, in)"),
    (lambda: _module(memory_a__rnn=nn.GRU(11, 7, num_layers=3)), "memory_a.rnn has num_layers=3, the kernel takes 2"),
    (lambda: _module(memory_a__rnn=nn.GRU(11, 513)), "memory_a.rnn has hidden_size=513, the gates (4 H) are limited to 2048: H <= 512"),
    (lambda: _module(memory_c__rnn=nn.GRU(2049, 7)), "memory_c.rnn has input_size=2049, widths are limited to 2048"),
    (lambda: _module(memory_a__rnn=nn.LSTM(11, 7)), "memory_a.rnn is an LSTM, memory_c.rnn a GRU; one kind for both"),
    (lambda: _module(memory_a__rnn=nn.GRU(11, 8)), "actor[0] takes 7 inputs (in_features), memory_a.rnn gives hidden_size = 8"),
    (lambda: _module(memory_c__rnn=nn.GRU(13, 7).double()), "memory_c.rnn.weight_ih_l0 is torch.float64, the kernel reads float32"),
]


@pytest.mark.parametrize("i", range(len(MODULE_REFUSALS)))
def test_describe_refuses(i):
    make, msg = MODULE_REFUSALS[i]
    with pytest.raises(ValueError) as e:
        train.describe_recurrent(make())
    assert str(e.value) == f"{OWNER}: {msg}"


def test_the_other_passes_still_refuse_a_recurrent_module_and_there_is_no_cpu_path():
    m = _module()
    with pytest.raises(ValueError) as e:
        train.describe(m)
    assert str(e.value) == "FusedTrainPass: the module has .memory_a (ActorCriticRecurrent); only the plain ActorCritic is built, the other learners keep the torch path"
    del m.memory_a, m.memory_c
    with pytest.raises(ValueError) as e:
        train.describe(m)
    assert str(e.value) == "FusedTrainPass: the module is recurrent (is_recurrent); the recurrent update keeps the torch path"
    with pytest.raises(ValueError) as e:
        train.FusedTrainPassRecurrent(_module())
    assert str(e.value) == f"{OWNER}: the module is on cpu, not on a HIP device (there is no CPU path)"


def _call_args(**change):
    """rnn_args on the CPU tensors of a case with one argument replaced."""
    x = rc.make_inputs("lstm2_h17_short")
    spec = train.describe_recurrent(rc.Recurrent(x))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    N = x["T"] * x["E"]
    kw = dict(obs=t(x["obs"]), critic_obs=t(x["critic_obs"]), masks=t(x["masks"]),
              hid=([t(x["h0_a"]), t(x["c0_a"])], [t(x["h0_c"]), t(x["c0_c"])]), n_envs=x["E"], mu=torch.zeros(N, 3), sigma=torch.zeros(N, 3), values=torch.zeros(N, 1))
    kw.update(change)
    return train.rnn_args(spec, kw["obs"], kw["critic_obs"], kw["masks"], kw["hid"], kw["n_envs"], kw["mu"], kw["sigma"], kw["values"], None)


_ML_NT = (_ML, _NT)
ARG_REFUSALS = [
    (dict(masks=torch.zeros(_T, _NT)), f"masks must be (T, n_traj) bool with unit inner stride; got ({_T}, {_NT}) torch.float32 with strides ({_NT}, 1)"),
    (dict(masks=torch.zeros(_NT, _T, dtype=torch.bool).t()), f"masks must be (T, n_traj) bool with unit inner stride; got ({_T}, {_NT}) torch.bool with strides (1, {_T})"),
    (dict(obs=torch.zeros(_T + 1, _NT, 11)), f"obs must be (max_len, {_NT}, width) with 1 <= max_len <= T = {_T}, as the masks say; got ({_T + 1}, {_NT}, 11)"),
    (dict(obs=torch.zeros(_ML, _NT + 1, 11)), f"obs must be (max_len, {_NT}, width) with 1 <= max_len <= T = {_T}, as the masks say; got ({_ML}, {_NT + 1}, 11)"),
    (dict(n_envs=0), f"n_envs = 0 must be an int in [1, n_traj = {_NT}]"),
    (dict(n_envs=_NT + 1), f"n_envs = {_NT + 1} must be an int in [1, n_traj = {_NT}]"),
    (dict(obs=torch.zeros(_ML, _NT, 12)), f"obs must be (max_len, n_traj, 11) float32 with unit inner stride; got ({_ML}, {_NT}, 12) torch.float32 with strides "
                                          f"({_NT * 12}, 12, 1) on cpu"),
    (dict(critic_obs=torch.zeros(_ML, _NT, 13, dtype=torch.float64)), f"critic_obs must be (max_len, n_traj, 13) float32 with unit inner stride; got ({_ML}, {_NT}, 13) "
                                                                      f"torch.float64 with strides ({_NT * 13}, 13, 1) on cpu"),
    (dict(critic_obs=torch.zeros(_ML - 1, _NT, 13)), f"critic_obs is ({_ML - 1}, {_NT}, .), obs ({_ML}, {_NT}, .)"),
    (dict(hid=torch.zeros(2, _NT, 17)), "hid_states must be the pair (hid_a, hid_c) of the mini-batch generator"),
    (dict(hid=(torch.zeros(2, _NT, 17), torch.zeros(2, _NT, 17))), "hid_states of memory_a holds 1 tensors, an LSTM has 2"),
    (dict(hid=([torch.zeros(2, _NT, 17), torch.zeros(2, _NT, 17)], [torch.zeros(2, _NT, 17), torch.zeros(1, _NT, 17)])),
     f"hid_states of memory_c c must be (2, {_NT}, 17) float32 with unit inner stride; got (1, {_NT}, 17) torch.float32 with strides ({_NT * 17}, 17, 1) on cpu"),
    (dict(mu=torch.zeros(_N, 4)), f"mu must be ({_N}, 3) float32 with unit inner stride; got ({_N}, 4) torch.float32 on cpu, strides (4, 1)"),
]


@pytest.mark.parametrize("i", range(len(ARG_REFUSALS)))
def test_rnn_args_refuses(i):
    change, msg = ARG_REFUSALS[i]
    with pytest.raises(ValueError) as e:
        _call_args(**change)
    assert str(e.value) == f"{OWNER}: {msg}"


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
_REFS = {}


def references(name):
    if name not in _REFS:
        x = rc.make_inputs(name)
        _REFS[name] = (x, rc.torch_reference(x, torch.float64), rc.torch_reference(x, torch.float32))
    return _REFS[name]


@pytest.mark.parametrize("name", list(rc.CASES))
def test_restatement_matches_torch_float64_autograd(name):
    """The float64 restatement against torch's own nn.LSTM / nn.GRU, the reference's unpadding and autograd, to 1e-12 relative: this pins
    the restatement, sliced sums included."""
    x, ref, _ = references(name)
    rel = lambda a, b: sup.max_err(a, b) <= 1e-12 * max(1.0, np.abs(b).max())
    for r in (rc.restate(x, np.float64), rc.restate(x, np.float64, sliced=True)):
        assert set(ref) == set(r) - {"pre_clip"} == {"mu", "sigma", "values"} | set(x["names"])
        for k, want in ref.items():
            assert r[k].shape == want.shape and rel(r[k], want), k
    if x["clip"] is not None:
        sat = (np.abs(ref["mu"]) >= x["clip"]).mean()
        assert 0.1 <= sat <= 0.9, sat


@pytest.mark.parametrize("name", list(rc.CASES))
def test_float32_restatement_in_the_kernels_order_keeps_half_the_rule(name):
    x, r64, r32 = references(name)
    rc.check_parity(rc.restate(x, np.float32, sliced=True), r64, r32, f"numpy f32 {name}", factor=oc.PARITY_FACTOR / 2)


APPLIES = dict(gate_order=lambda x: x["kind"] == "lstm", no_dc_carry=lambda x: x["kind"] == "lstm", bhn_without_r=lambda x: x["kind"] == "gru",
               z_swapped=lambda x: x["kind"] == "gru", layer1_old_h=lambda x: x["layers"] == 2, padded_step=lambda x: (x["lens"] < x["max_len"]).any())
LARGE = 100.0        # "a large factor" above the rule's own bound


@pytest.mark.parametrize("defect", rc.DEFECTS)
def test_parity_rule_catches_the_planted_defects(defect):
    """Each defect is a change of the restatement alone; on every tiny set it applies to, some tensor leaves the unchanged rule's bound by
    more than LARGE times."""
    seen = 0
    for name in rc.TINY:
        x, r64, r32 = references(name)
        if not APPLIES.get(defect, lambda x: True)(x):
            continue
        seen += 1
        rc.check_parity(rc.restate(x, np.float64), r64, r32, "the restatement itself")
        bad = rc.restate(x, np.float64, defects=(defect,))
        over = {k: sup.max_err(bad[k], r64[k]) / oc.parity_bound(sup.max_err(r32[k], r64[k]), r64[k]) for k in r64}
        worst = max(over, key=over.get)
        print(f"{defect} on {name}: {worst} is {over[worst]:.3g} times its bound")
        assert over[worst] > LARGE, (defect, name, over[worst])
        with pytest.raises(AssertionError):
            rc.check_parity(bad, r64, r32, f"{defect} on {name}")
    assert seen >= 1


def test_the_case_table_covers_what_it_is_for():
    xs = {n: references(n)[0] for n in rc.CASES}
    assert {x["H"] for x in xs.values()} == {7, 17, 64, 65, 256, 512}
    assert {(x["kind"], x["layers"]) for x in xs.values()} == {("lstm", 1), ("lstm", 2), ("gru", 1), ("gru", 2)}
    assert {x["T"] for x in xs.values()} >= {1, 2, 6}
    tiles = {n: rc.plan_of_case(x)["time_row_tile"] for n, x in xs.items()}
    assert {x["n_traj"] for n, x in xs.items() if tiles[n] == 32} >= {31, 32, 33}
    assert tiles["lstm1_h512_t2"] == 8 and xs["lstm1_h512_t2"]["n_traj"] == 9 and (xs["lstm1_h256_t3"]["T"], xs["lstm1_h256_t3"]["E"]) == (3, 9)
    assert any(x["max_len"] < x["T"] for x in xs.values()) and any(x["E"] == 1 for x in xs.values())
    assert any((x["lens"] == 1).sum() >= x["T"] for x in xs.values())                       # a done at every step of one env
    assert any(x["n_traj"] == x["E"] and x["T"] > 1 for x in xs.values())                   # no done at all
    assert any(x["first"] for x in xs.values()) and any(x["shared"] and x["kind"] == "lstm" for x in xs.values())
    assert any(x["clip"] is None for x in xs.values()) and any(x["clip"] is not None for x in xs.values())
    assert all(a in rc.CASES for a in rc.TINY)


# ---- the golden fixtures ------------------------------------------------------------------------------------------------------------------
FIXTURES = {k: os.path.join(ROOT, "tests", "golden", f"ppo_recurrent_train_{k}.npz") for k in ("lstm", "gru")}


@pytest.fixture(scope="module", params=list(FIXTURES))
def fx(request):
    return rc.load_fixture(FIXTURES[request.param])


def test_fixture_is_the_tiny_recurrent_module_and_meets_its_seed_conditions(fx):
    cfg = fx["cfg"]
    assert (fx["actor"], fx["critic"]) == ([8, 16, 8, 3], [8, 16, 8, 1]) and (cfg["T"], cfg["steps"]) == (6, 4) and cfg["layers"] == (2 if cfg["lstm"] else 1)
    assert fx["padded_obs"].shape[2] == 7 and fx["padded_critic_obs"].shape[2] == 9 and fx["hid_a_h"].shape[0] == cfg["layers"] and fx["hid_a_h"].shape[2] == 8
    assert fx["names"][:13] == ["std"] + [f"{c}.{i}.{k}" for c in ("actor", "critic") for i in (0, 2, 4) for k in ("weight", "bias")]
    assert fx["names"][13:] == [f"{m}.rnn.{n}_l{l}" for m in ("memory_a", "memory_c") for l in range(cfg["layers"]) for n in rc.RNN_PARAMS]
    assert all(os.path.getsize(p) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "ppo_dwaq_train.npz")) for p in FIXTURES.values())
    lens = fx["masks"].sum(0)
    assert fx["masks"].shape == (6, len(lens)) and fx["padded_obs"].shape[0] == lens.max() < cfg["T"]               # max_len < T in every mini-batch
    assert (lens == 1).any() and np.abs(fx["hid_a_h"]).max() > 0                                                    # a start state that is not zero
    for s in range(cfg["steps"]):
        x = rc.fixture_inputs(fx, s)
        assert x["n_traj"] > x["E"] == 4 and x["lens"].sum() == 24 and (s < 2 or x["first"] == fx["traj_range"][s - 2][0])
        pre = rc.restate(x, np.float64)["pre_clip"]
        assert 0.1 <= (np.abs(pre) >= cfg["clip_actions"]).mean() <= 0.9 and np.abs(np.abs(pre) - cfg["clip_actions"]).min() >= 1e-4
    assert fx["traj_range"][0][0] == 0 and fx["traj_range"][1][0] == fx["traj_range"][0][1] > 0                     # a view with first > 0
    d, m = cfg["desired_kl"], cfg["max_grad_norm"]
    assert all(abs(k / (2 * d) - 1) > 0.01 and abs(k / (d / 2) - 1) > 0.01 for k in fx["kl"]) and all(abs(n / m - 1) > 0.01 for n in fx["grad_norm"])
    assert len({cfg["lr0"]} | set(float(v) for v in fx["lr"])) > 1                                                  # the rate rule moves


def test_restatement_matches_the_reference_update(fx):
    """Every step of the reference's PPO.update() on ActorCriticRecurrent: the restated pass, the loss head's restatement and the restated
    optimizer reproduce outputs, loss, KL, every gradient before the clip, norm, rate and every parameter to 1e-12."""
    cfg = fx["cfg"]
    params, state, lr = [p.copy() for p in fx["init"]], {}, cfg["lr0"]
    for s in range(cfg["steps"]):
        x = rc.fixture_inputs(fx, s, params)
        fw = rc.restate(x, np.float64)
        for k in ("mu", "sigma", "values"):
            assert sup.max_err(fw[k], fx[k][s]) <= 1e-12, (s, k)
        r = pc.restate(sup.fixture_loss_inputs(fx, s, fw["mu"], fw["sigma"], fw["values"]), True, False, cfg["entropy_coef"], clip=cfg["clip_param"],
                       value_loss_coef=cfg["value_loss_coef"])
        assert abs(float(r["loss"]) - fx["loss"][s]) <= 1e-12 and abs(float(r["kl"][0]) - fx["kl"][s]) <= 1e-12
        x.update(grad_mu=r["grad_mu"][0], grad_sigma=r["grad_sigma"][0], grad_values=r["grad_values"])
        back = rc.restate(x, np.float64)
        grads = [back[n] for n in x["names"]]
        for name, g, want in zip(fx["names"], grads, fx["grads"][s]):
            assert g.shape == want.shape and sup.max_err(g, want) <= 1e-12, (s, name)
        step = ta.adam(params, grads, state, lr, cfg, kl=float(r["kl"][0]))
        lr = step["lr"]
        assert lr == fx["lr"][s] and abs(step["grad_norm"] - fx["grad_norm"][s]) <= 1e-12
        params = step["params"]
        for name, p, want in zip(fx["names"], params, fx["params"][s]):
            assert sup.max_err(p, want) <= 1e-12, (s, name)

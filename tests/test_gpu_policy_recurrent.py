"""The recurrent fused policy step on the device (the memory prefix of csrc/lg_policy.hip behind FusedPolicy) against torch's own nn.LSTM /
nn.GRU and MLPs on the CPU in float64: one- and five-step parity at every net set and ragged batch sizes, the snapshots and storage rows,
the folded and the stand-alone reset, the modes, NaN isolation, a replaced rnn, capture and replay, and a 6-step rollout through the
recurrent mini-batch generator.

Stand-ins, inputs, oracle (float64) and yardstick (float32 CPU) come from tests/test_policy_recurrent_host.py, the parity rule
(`parity_bound`, `max_err`) from tests/test_policy_host.py, unchanged."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.test_policy_host import max_err, parity_bound
from tests.test_policy_recurrent_host import RESET_BEFORE, RNETS, STEPS, load_states, make_inputs, make_rnet, net, net_key, shared, state_keys

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = {name: ((17,) if name == "gru512" else (1, 33, 67)) for name in RNETS}      # 33, 67: ragged against every row tile; several tiles
CASES = [(name, n) for name in RNETS for n in SIZES[name]]
_GPU = {}


def gpu_module(name):
    """The module of net set `name` (an RNETS name, or a row of another table: see `net`) on the device, moved once."""
    if net_key(name) not in _GPU:
        _GPU[net_key(name)] = copy.deepcopy(make_rnet(name)).to(DEV)
    return _GPU[net_key(name)]


def fused(name, module=None):
    from hcr_genesis_lr_cl_amd.policy import FusedPolicy
    return FusedPolicy(module if module is not None else gpu_module(name))


def to_reference(start, kind):
    """A dict of states by state_keys in the form of get_hidden_states, on the device."""
    one = lambda w: (start["h_" + w].to(DEV), start["c_" + w].to(DEV)) if kind == "lstm" else start["h_" + w].to(DEV)
    return one("a"), one("c")


def live(fp, kind):
    """The live states as a dict by state_keys (the tensors themselves)."""
    a, c = fp.get_hidden_states()
    return dict(h_a=a[0], c_a=a[1], h_c=c[0], c_c=c[1]) if kind == "lstm" else dict(h_a=a, h_c=c)


def snapshot(fp, kind):
    a, c = fp.last_hidden_states
    return dict(h_a=a[0], c_a=a[1], h_c=c[0], c_c=c[1]) if kind == "lstm" else dict(h_a=a, h_c=c)


def started(name, n):
    """A FusedPolicy whose states of batch size n hold the case's incoming states."""
    s = shared(name, n)
    fp = fused(name)
    fp.set_hidden_states(to_reference(s["inp"]["start"], net(name)["kind"]), n=n)
    return fp, s


def step(fp, inp, t, **kw):
    return fp.act(inp["obs"][t].to(DEV), inp["cobs"][t].to(DEV), noise=inp["noise"][t].to(DEV), **kw)


def check_step(name, n, fp, s, t):
    """Outputs and states after step t against the float64 oracle, each within the parity rule on the float32 yardstick of the same step."""
    kind, name = net(name)["kind"], net_key(name)
    torch.cuda.synchronize()
    got = dict(mu=fp.last_mu, values=fp.last_values, actions=fp.last_actions, log_prob=fp.last_log_prob, **live(fp, kind))
    ref, f32 = s["ref"][t], s["f32"][t]
    for k, x in got.items():
        ek, et = max_err(x.cpu().numpy(), ref[k]), max_err(f32[k], ref[k])
        print(f"recurrent parity {name} N={n} step {t} {k}: kernel {ek:.3e} torch-f32 {et:.3e} bound {parity_bound(et, ref[k]):.3e}")
        assert ek <= parity_bound(et, ref[k]), (k, ek, et)
    std = s["module"].std.detach().numpy()
    assert np.array_equal(fp.last_sigma.cpu().numpy(), np.broadcast_to(std, (n, std.size)))


# ---- parity -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", CASES)
def test_one_step_parity(name, n):
    fp, s = started(name, n)
    step(fp, s["inp"], 0)
    check_step(name, n, fp, s, 0)


@pytest.mark.parametrize("name,n", CASES)
def test_five_step_parity(name, n):
    """The reset before step 2 goes through `reset=`, the one before step 4 through `reset()`; the last step's outputs and states are
    compared, the float32 yardstick having accumulated over the same five steps."""
    fp, s = started(name, n)
    inp = s["inp"]
    for t in range(STEPS):
        if t == RESET_BEFORE[0]:
            step(fp, inp, t, reset=inp["masks"][t].to(DEV))
            continue
        if t == RESET_BEFORE[1]:
            fp.reset(inp["masks"][t].to(DEV))
        step(fp, inp, t)
    check_step(name, n, fp, s, STEPS - 1)


# ---- snapshots and storage --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_lstm2", "tiny_gru2", "go2_lstm"])
def test_snapshots_and_storage_rows(name):
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    d, n, T = RNETS[name], 33, 3
    fp, s = started(name, n)
    inp, kind = s["inp"], d["kind"]
    states = live(fp, kind)
    addresses = {k: v.data_ptr() for k, v in states.items()}
    mask = inp["masks"][RESET_BEFORE[0]].to(DEV)
    expect = {k: v.clone() for k, v in states.items()}
    for v in expect.values():
        v[:, mask] = 0
    step(fp, inp, 0, reset=mask)                                                  # without a storage: the object's own snapshot buffers
    torch.cuda.synchronize()
    for k, v in snapshot(fp, kind).items():
        assert torch.equal(v, expect[k]), k
        assert not torch.equal(states[k], expect[k])                              # ... while the live state moved on
    st = RolloutStorage(n, T, [d["obs"]], [d["cobs"]], [d["A"]], DEV)
    st.step = 1
    expect = {k: v.clone() for k, v in states.items()}
    step(fp, inp, 1, storage=st)                                                  # allocates the saved lists, as add_step would
    torch.cuda.synchronize()
    saved = dict(zip(state_keys(kind), st.saved_hidden_states_a + st.saved_hidden_states_c))      # (h, c) of the actor's, then of the critic's
    assert len(st.saved_hidden_states_a) == len(st.saved_hidden_states_c) == (2 if kind == "lstm" else 1)
    for k, v in saved.items():
        assert v.shape == (T, d["layers"], n, d["H"])
        assert torch.equal(v[1], expect[k]) and torch.equal(snapshot(fp, kind)[k], expect[k]), k
        assert snapshot(fp, kind)[k].data_ptr() == v[1].data_ptr()                # the snapshot IS the storage row
        assert not v[0].any() and not v[2].any()                                  # no other row
    # a further call into the same storage: only the five policy rows and the saved-state rows of step 1 change
    tensors = {k: v for k, v in vars(st).items() if torch.is_tensor(v)}
    for v in list(saved.values()) + list(tensors.values()):
        v.fill_(7.5 if v.dtype == torch.float32 else 3)
    before = {k: v.clone() for k, v in tensors.items()}
    expect = {k: v.clone() for k, v in states.items()}
    step(fp, inp, 2, storage=st)
    torch.cuda.synchronize()
    written = {"actions", "mu", "sigma", "actions_log_prob", "values"}
    for k, v in tensors.items():
        for t in range(v.shape[0]) if v.dim() == 3 and v.shape[0] == T else [None]:
            same = torch.equal(v if t is None else v[t], before[k] if t is None else before[k][t])
            assert same != (k in written and t == 1), (k, t)
    for k, v in saved.items():
        assert torch.equal(v[1], expect[k]) and (v[0] == 7.5).all() and (v[2] == 7.5).all(), k
    assert st.step == 1 and {k: v.data_ptr() for k, v in live(fp, kind).items()} == addresses      # three calls later: the same addresses
    st.add_step(torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV), None, 0.99,
                observations=inp["obs"][2].to(DEV), critic_observations=inp["cobs"][2].to(DEV))     # no hidden_states: nothing more is stored
    torch.cuda.synchronize()
    for k, v in saved.items():
        assert torch.equal(v[1], expect[k]) and (v[2] == 7.5).all(), k


# ---- reset --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_lstm2", "tiny_gru1", "go2_lstm"])
def test_reset_folded_equals_stand_alone(name):
    n, kind = 33, RNETS[name]["kind"]
    fa, s = started(name, n)
    fb, _ = started(name, n)
    inp = s["inp"]
    mask = inp["masks"][RESET_BEFORE[0]].to(DEV)
    before = {k: v.clone() for k, v in live(fb, kind).items()}
    step(fa, inp, 0, reset=mask)
    fb.reset(mask)
    torch.cuda.synchronize()
    for k, v in live(fb, kind).items():
        assert not v[:, mask].any() and torch.equal(v[:, ~mask], before[k][:, ~mask]) and v[:, ~mask].any(), k     # unmasked rows: bit-unchanged
    step(fb, inp, 0)
    torch.cuda.synchronize()
    for k in ("last_actions", "last_mu", "last_sigma", "last_log_prob", "last_values"):
        assert torch.equal(getattr(fa, k), getattr(fb, k)), k
    for k, v in live(fa, kind).items():
        assert torch.equal(v, live(fb, kind)[k]), k
        assert torch.equal(snapshot(fa, kind)[k], snapshot(fb, kind)[k]), k
    # a uint8 mask with values other than 0 / 1 counts as done; a list of indices is refused
    fc, _ = started(name, n)
    step(fc, inp, 0, reset=mask.to(torch.uint8) * 200)
    torch.cuda.synchronize()
    for k, v in live(fa, kind).items():
        assert torch.equal(v, live(fc, kind)[k]), k
    with pytest.raises(ValueError, match="reset must be a mask"):
        fc.reset(torch.nonzero(mask).flatten())
    fc.reset(mask.to(torch.uint8) * 3)
    torch.cuda.synchronize()
    assert all(not v[:, mask].any() and v[:, ~mask].any() for v in live(fc, kind).values())
    fc.reset(None)
    torch.cuda.synchronize()
    assert all(not v.any() for v in live(fc, kind).values())


# ---- modes --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_lstm2", "tiny_gru2"])
def test_modes_advance_one_memory_each(name):
    n, kind = 33, RNETS[name]["kind"]
    fp, s = started(name, n)
    inp = s["inp"]
    before = {k: v.clone() for k, v in live(fp, kind).items()}
    mu = fp.act_inference(inp["obs"][0].to(DEV))
    torch.cuda.synchronize()
    now = live(fp, kind)
    for k in before:
        assert torch.equal(now[k], before[k]) == k.endswith("_c"), k                 # memory_a moved, memory_c did not
    ref, f32 = s["ref"][0], s["f32"][0]
    for k, x in (("mu", mu), ("h_a", now["h_a"])):
        assert max_err(x.cpu().numpy(), ref[k]) <= parity_bound(max_err(f32[k], ref[k]), ref[k]), k
    after_a = {k: v.clone() for k, v in now.items()}
    v = fp.evaluate(inp["cobs"][0].to(DEV))
    torch.cuda.synchronize()
    for k in before:
        assert torch.equal(now[k], after_a[k]) == k.endswith("_a"), k                # the reverse
    for k, x in (("values", v), ("h_c", now["h_c"])):
        assert max_err(x.cpu().numpy(), ref[k]) <= parity_bound(max_err(f32[k], ref[k]), ref[k]), k
    with pytest.raises(ValueError, match="reset= needs critic_obs"):
        fp.act(inp["obs"][0].to(DEV), None, noise=inp["noise"][0].to(DEV), reset=inp["masks"][RESET_BEFORE[0]].to(DEV))
    for k in before:                                                                  # ... refused before anything ran
        assert torch.equal(now[k], after_a[k]) == k.endswith("_a"), k


# ---- isolation ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["obs", "h"])
@pytest.mark.parametrize("name", ["tiny_lstm2", "tiny_gru2", "go2_lstm"])
def test_nan_stays_in_its_row(name, where):
    """N = 33: the poisoned row shares its tile with its neighbours and the last tile is ragged."""
    n, row, kind = 33, 5, RNETS[name]["kind"]
    clean, s = started(name, n)
    inp = s["inp"]
    step(clean, inp, 0)
    bad, _ = started(name, n)
    obs = inp["obs"][0].clone()
    if where == "obs":
        obs[row, 2] = float("nan")
    else:
        live(bad, kind)["h_a"][-1, row, 3] = float("nan")
    bad.act(obs.to(DEV), inp["cobs"][0].to(DEV), noise=inp["noise"][0].to(DEV))
    torch.cuda.synchronize()
    others = torch.arange(n, device=DEV) != row
    for k in ("last_actions", "last_mu", "last_log_prob"):
        g, c = getattr(bad, k), getattr(clean, k)
        assert torch.isnan(g[row]).all() and torch.equal(g[others], c[others]), k
    assert torch.equal(bad.last_sigma[others], clean.last_sigma[others]) and torch.isnan(bad.last_sigma[row]).all()
    assert torch.equal(bad.last_values, clean.last_values)                            # the critic's run never read it
    lb, lc = live(bad, kind), live(clean, kind)
    for k in lb:
        assert torch.equal(lb[k][:, others], lc[k][:, others]), k
        if k.endswith("_c"):
            assert torch.equal(lb[k], lc[k]), k
    assert torch.isnan(lb["h_a"][-1, row]).all()                                      # the top layer's new state of that row
    if where == "obs":
        assert torch.isnan(lb["h_a"][:, row]).all()                                   # through every layer


# ---- a replaced rnn -----------------------------------------------------------------------------------------------------------------------
def test_a_replaced_rnn_is_seen():
    name, n = "tiny_gru1", 33
    d = RNETS[name]
    m = copy.deepcopy(gpu_module(name))
    fp = fused(name, m)
    s = shared(name, n)
    inp = s["inp"]
    start = to_reference(inp["start"], "gru")
    fp.set_hidden_states(start, n=n)
    mu0 = fp.act_inference(inp["obs"][0].to(DEV)).clone()
    fresh = nn.GRU(d["obs"], d["H"], d["layers"])
    with torch.no_grad():
        for p in fresh.parameters():
            p.uniform_(-0.6, 0.6)
    m.memory_a.rnn = copy.deepcopy(fresh).to(DEV)
    fp.set_hidden_states(start)
    mu1 = fp.act_inference(inp["obs"][0].to(DEV)).clone()
    torch.cuda.synchronize()
    cpu = copy.deepcopy(s["module"])
    cpu.memory_a.rnn = fresh
    with torch.no_grad():
        m64, m32 = copy.deepcopy(cpu).double(), cpu
        load_states(m64, inp["start"], torch.float64)
        load_states(m32, inp["start"], torch.float32)
        ref, f32 = m64.mean(inp["obs"][0].double()).numpy(), m32.mean(inp["obs"][0]).numpy()
    bound = parity_bound(max_err(f32, ref), ref)
    assert max_err(mu1.cpu().numpy(), ref) <= bound                                   # the second call follows the new weights ...
    assert max_err(mu0.cpu().numpy(), ref) > bound                                    # ... which the first did not have


# ---- capture and replay -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiny_lstm2", "go2_lstm"])
def test_capture_and_replay(name):
    n, kind = 33, RNETS[name]["kind"]
    eager, s = started(name, n)
    inp = s["inp"]
    masks = [torch.zeros(n, dtype=torch.bool), inp["masks"][RESET_BEFORE[0]], inp["masks"][RESET_BEFORE[1]]]
    want = []
    mask_e = torch.zeros(n, dtype=torch.bool, device=DEV)
    obs_e, cobs_e, noise_e = (torch.zeros_like(inp[k][0], device=DEV) for k in ("obs", "cobs", "noise"))
    for t in range(3):
        mask_e.copy_(masks[t]); obs_e.copy_(inp["obs"][t]); cobs_e.copy_(inp["cobs"][t]); noise_e.copy_(inp["noise"][t])
        eager.act(obs_e, cobs_e, noise=noise_e, reset=mask_e)
        torch.cuda.synchronize()
        want.append({k: v.clone() for k, v in dict(actions=eager.last_actions, log_prob=eager.last_log_prob, values=eager.last_values,
                                                   **live(eager, kind)).items()})
    fp, _ = started(name, n)
    mask, obs, cobs, noise = (torch.zeros_like(x) for x in (mask_e, obs_e, cobs_e, noise_e))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fp.act(obs, cobs, noise=noise, reset=mask)                                    # warm-up outside the capture: buffers and descriptor exist
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                     # one stream, one act launch
        fp.act(obs, cobs, noise=noise, reset=mask)
    torch.cuda.synchronize()
    fp.set_hidden_states(to_reference(inp["start"], kind))                            # the warm-up moved them; capturing enqueued nothing
    for t in range(3):
        mask.copy_(masks[t]); obs.copy_(inp["obs"][t]); cobs.copy_(inp["cobs"][t]); noise.copy_(inp["noise"][t])
        graph.replay()
        torch.cuda.synchronize()
        got = dict(actions=fp.last_actions, log_prob=fp.last_log_prob, values=fp.last_values, **live(fp, kind))
        for k, v in want[t].items():
            assert torch.equal(got[k], v), (t, k)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_rollout_through_the_recurrent_generator():
    """T = 6, N = 40, go2_lstm: FusedPolicy.act(storage=, reset=) + add_step against the torch module through add_transitions with
    hidden_states, on the CPU in float32 (the yardstick) and in float64 (the oracle); both are stored as float32.  Every policy starts
    from the same non-zero states and takes two steps before the rollout, as a policy in its second rollout would: the trajectories that
    begin at t = 0 then start from COMPUTED states (every later trajectory begins behind a reset, from zeros)."""
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    name, T, n = "go2_lstm", 6, 40
    d = RNETS[name]
    g = torch.Generator().manual_seed(5)
    obs, cobs = torch.randn(T, n, d["obs"], generator=g), torch.randn(T, n, d["cobs"], generator=g)
    noise, rew = torch.randn(T, n, d["A"], generator=g), torch.randn(T, n, generator=g)
    dones = torch.rand(T, n, generator=g) < 0.25                                      # trajectories of unequal length
    assert dones.any(0).sum() > n // 2 and not dones.all(0).any() and dones[:-1].sum(0).unique().numel() > 2
    new = lambda: RolloutStorage(n, T, [d["obs"]], [d["cobs"]], [d["A"]], DEV, lstm_critic_hidden="own")

    warm = make_inputs(name, n, seed=7)
    st_f, fp = new(), fused(name)
    fp.set_hidden_states(to_reference(warm["start"], d["kind"]), n=n)
    for w in range(2):
        step(fp, warm, w)
    prev = None
    for t in range(T):
        o, c = obs[t].to(DEV), cobs[t].to(DEV)
        fp.act(o, c, storage=st_f, noise=noise[t].to(DEV), reset=prev)
        prev = dones[t].to(DEV)
        st_f.add_step(rew[t].to(DEV), prev, None, 0.99, observations=o, critic_observations=c)

    def by_torch(module, dtype, dev):
        st = new()
        load_states(module, warm["start"], dtype)
        with torch.no_grad():
            for w in range(2):
                module.mean(warm["obs"][w].to(dev, dtype)), module.value(warm["cobs"][w].to(dev, dtype))
            for t in range(T):
                tr = RolloutStorage.Transition()
                tr.hidden_states = tuple(tuple(x.to(DEV, torch.float32) for x in hs) for hs in module.get_hidden_states())
                mu, v = module.mean(obs[t].to(dev, dtype)), module.value(cobs[t].to(dev, dtype))
                sigma = mu * 0 + module.std
                tr.actions = mu + sigma * noise[t].to(dev, dtype)
                tr.actions_log_prob = torch.distributions.Normal(mu, sigma).log_prob(tr.actions).sum(-1)
                tr.action_mean, tr.action_sigma, tr.values = mu, sigma, v
                for k in ("actions", "actions_log_prob", "action_mean", "action_sigma", "values"):
                    setattr(tr, k, getattr(tr, k).to(DEV, torch.float32))
                tr.observations, tr.critic_observations = obs[t].to(DEV), cobs[t].to(DEV)
                tr.rewards, tr.dones = rew[t].to(DEV), dones[t].to(DEV)
                st.add_transitions(tr)
                module.reset(dones[t].to(dev))
        return st
    st_32 = by_torch(copy.deepcopy(make_rnet(name)), torch.float32, "cpu")
    st_64 = by_torch(copy.deepcopy(make_rnet(name)).double(), torch.float64, "cpu")
    torch.cuda.synchronize()
    for w in ("a", "c"):                                                               # every stored pre-step state, not only the trajectory starts
        for j, what in enumerate(("h", "c")):
            got, y, ref = (getattr(st, "saved_hidden_states_" + w)[j].cpu().numpy() for st in (st_f, st_32, st_64))
            ref = ref.astype(np.float64)
            ek, et = max_err(got, ref), max_err(y, ref)
            print(f"rollout saved {what}_{w}: kernel {ek:.3e} torch-f32 {et:.3e} bound {parity_bound(et, ref):.3e}")
            assert got.shape == ref.shape == (T, d["layers"], n, d["H"]) and ek <= parity_bound(et, ref), (w, what, ek, et)
            zero = np.zeros((T, n), bool)
            zero[1:] = dones[:-1].numpy()
            assert not got[zero[:, None, :].repeat(d["layers"], 1)].any() and np.abs(got[0]).min() > 0      # zeros exactly behind a done
    batches = [list(st.reccurent_mini_batch_generator(2, 1)) for st in (st_f, st_32, st_64)]
    assert len(batches[0]) == 2
    for bf, b32, b64 in zip(*batches):
        assert torch.equal(bf[-1], b32[-1]) and torch.equal(bf[-1], b64[-1])           # the same masks ...
        assert bf[0].shape == b32[0].shape and bf[1].shape == b32[1].shape and bf[0].shape[1] > n // 2 and bf[0].shape[0] <= T    # ... and trajectories
        assert torch.equal(bf[0], b32[0]) and torch.equal(bf[1], b32[1])               # padded observation rows are copies
        for w in (0, 1):                                                               # start hidden states of the actor's and the critic's memory
            for j, what in enumerate(("h", "c")):
                ref = b64[9][w][j].cpu().numpy().astype(np.float64)
                ek, et = max_err(bf[9][w][j].cpu().numpy(), ref), max_err(b32[9][w][j].cpu().numpy(), ref)
                print(f"rollout start {what}_{'ac'[w]}: kernel {ek:.3e} torch-f32 {et:.3e} bound {parity_bound(et, ref):.3e}")
                assert bf[9][w][j].shape == b64[9][w][j].shape and ek <= parity_bound(et, ref), (w, what, ek, et)
                assert np.abs(ref).max() > 0.01                                        # the starts at t = 0 are computed states
        for i, what in ((2, "actions"), (3, "values"), (6, "log_prob"), (7, "mu")):    # the policy rows the storage kept
            ref = b64[i].cpu().numpy().astype(np.float64)
            ek, et = max_err(bf[i].cpu().numpy(), ref), max_err(b32[i].cpu().numpy(), ref)
            print(f"rollout {what}: kernel {ek:.3e} torch-f32 {et:.3e} bound {parity_bound(et, ref):.3e}")
            assert ek <= parity_bound(et, ref), (what, ek, et)

"""Recurrent policies in hcr_genesis_lr_cl_amd.rollout.RolloutStorage: stored hidden states, the trajectory index, padded trajectories,
masks, start hidden states and un-padding, against golden vectors produced by rsl_rl's own PPO + ActorCriticRecurrent + RolloutStorage
(tests/golden/rollout_recurrent_*.npz, written by tests/golden/gen_rollout_recurrent_fixtures.py).

Everything the new kernels move is a copy or a zero, so those comparisons are exact (assert_array_equal).  The value-derived rows
(rewards, returns, advantages) go through the record / GAE kernels and keep the tolerances of tests/test_rollout.py.  `Restatement` below
is the same computation in vectorised numpy, checked against the fixtures on the CPU and then used as the checker at sizes no
fixture covers."""
import glob
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
YIELD = ("obs", "critic_obs", "actions", "values", "advantages", "returns", "logp", "mu", "sigma")
EXACT = ("obs", "critic_obs", "actions", "values", "logp", "mu", "sigma")
GAE_TOL = {"returns": dict(rtol=1e-5, atol=2e-6), "advantages": dict(rtol=1e-5, atol=5e-6)}      # tests/test_rollout.py
REPLAY_TOL = 1e-5                                                                                 # the project's float tolerance for replays


def load(rnn, k):
    """One rollout of the fixture: its parts merged into one dict."""
    fx = {}
    parts = sorted(glob.glob(os.path.join(GOLDEN, f"rollout_recurrent_{rnn}_r{k}_*.npz")))
    assert len(parts) == 5, parts
    for p in parts:
        with np.load(p) as z:
            fx.update({n: z[n] for n in z.files})
    fx["n_hid"] = 2 if rnn == "lstm" else 1
    return fx


class Restatement:
    """Trajectory index, padding, masks and start hidden states of a rollout with done flags `dones` (T, N), in numpy.

    A trajectory starts at t = 0 and behind every done and ends at a done or at t = T-1.  In the env-major flattening (position e * T + t)
    the ends are the positions of the flags once the last step of every env counts as one; each start is the position behind the
    previous end."""

    def __init__(self, dones):
        d = np.asarray(dones).reshape(dones.shape[0], -1).astype(bool).copy()
        self.T, self.N = d.shape
        d[-1] = True
        ends = np.flatnonzero(d.T.reshape(-1))
        starts = np.concatenate(([0], ends[:-1] + 1))
        self.env, self.t_start, self.length = starts // self.T, starts % self.T, ends - starts + 1
        self.n_traj, self.max_len = len(starts), int(self.length.max())
        self.offset = np.searchsorted(self.env, np.arange(self.N + 1))        # first trajectory of every env; [N] = n_traj

    def pad(self, x, rows=None):
        """(T, N, ...) -> (max_len, n_traj, ...): row t' of trajectory j is x[t_start_j + t', env_j], zero from length_j on."""
        tp = np.arange(self.max_len if rows is None else rows)[:, None]
        valid = tp < self.length[None, :]
        got = x[np.minimum(self.t_start[None, :] + tp, self.T - 1), self.env[None, :]]
        return np.where(valid.reshape(valid.shape + (1,) * (x.ndim - 2)), got, np.zeros((), x.dtype))

    def masks(self):
        return np.arange(self.T)[:, None] < self.length[None, :]

    def start_hidden(self, saved):
        """(T, L, N, H) -> (L, n_traj, H): the state held when each trajectory began."""
        return np.ascontiguousarray(saved[self.t_start, :, self.env, :].transpose(1, 0, 2))

    def unpad(self, padded):
        """(rows, n_traj, ...) -> (T, N, ...): every valid row back to its step and env."""
        out = np.zeros((self.T, self.N) + padded.shape[2:], padded.dtype)
        for tp in range(padded.shape[0]):
            j = np.flatnonzero(self.length > tp)
            out[self.t_start[j] + tp, self.env[j]] = padded[tp, j]
        return out


# ---- CPU: the restatement reproduces the reference's arrays --------------------------------------------------------------------------
@pytest.mark.parametrize("rnn", ["lstm", "gru"])
@pytest.mark.parametrize("k", [0, 1])
def test_restatement_reproduces_rsl_rl(rnn, k):
    fx = load(rnn, k)
    T, N = fx["dones"].shape
    r = Restatement(fx["dones"])
    obs, cobs, masks = r.pad(fx["obs"]), r.pad(fx["critic_obs"]), r.masks()
    hid_a = [r.start_hidden(fx[f"saved_a{i}"]) for i in range(fx["n_hid"])]
    hid_c = [r.start_hidden(fx[f"saved_c{i}"]) for i in range(fx["n_hid"])]
    per, first = N // 4, 0
    for b in range(4):
        lo, hi = r.offset[b * per], r.offset[(b + 1) * per]
        assert lo == first
        first = hi
        np.testing.assert_array_equal(obs[:, lo:hi], fx[f"b{b}_obs"])
        np.testing.assert_array_equal(cobs[:, lo:hi], fx[f"b{b}_critic_obs"])
        np.testing.assert_array_equal(masks[:, lo:hi], fx[f"b{b}_masks"])
        assert fx[f"b{b}_masks"].dtype == np.bool_ and fx[f"b{b}_masks"].shape[0] == T
        for i in range(fx["n_hid"]):
            np.testing.assert_array_equal(hid_a[i][:, lo:hi], fx[f"b{b}_hid_a{i}"])
            np.testing.assert_array_equal(hid_c[i][:, lo:hi], fx[f"b{b}_own_c{i}"])
            # rollout_storage.py:231: an LSTM's critic is handed the actor's states, a GRU's its own
            np.testing.assert_array_equal((hid_a if rnn == "lstm" else hid_c)[i][:, lo:hi], fx[f"b{b}_hid_c{i}"])
        for n in ("actions", "mu", "sigma", "values"):
            np.testing.assert_array_equal(fx[n][:, b * per:(b + 1) * per].reshape(fx[f"b{b}_{n}"].shape), fx[f"b{b}_{n}"])
    assert first == r.n_traj
    np.testing.assert_array_equal(r.unpad(obs), fx["obs"])
    # the fixture is worth something: real terminations as well as time-outs, an env that never resets, an env with three trajectories,
    # and (second rollout) trajectories that start from a non-zero state
    assert fx["dones"].sum() > fx["time_outs"].sum() > 0 and (fx["dones"].sum(0) == 0).any() and (np.diff(r.offset) >= 3).any()
    assert bool(fx["hidden_none_at_step0"]) == (k == 0) and hid_a[0].any() == (k == 1)


def test_restatement_short_trajectories():
    """Every env done at the same step: the padded tensor has max_len (3) rows, the mask keeps T (6)."""
    fx = np.load(os.path.join(GOLDEN, "rollout_recurrent_short.npz"))
    r = Restatement(fx["dones"])
    assert (r.n_traj, r.max_len) == (6, 3) and fx["padded"].shape == (3, 6, 5) and fx["masks"].shape == (6, 6)
    np.testing.assert_array_equal(r.pad(fx["x"]), fx["padded"])
    np.testing.assert_array_equal(r.masks(), fx["masks"])


def test_recurrent_exports_are_declared():
    """The new entry points are in the header, in abi.ROLLOUT_EXPORTS and in the built library."""
    import ctypes
    import re
    from hcr_genesis_lr_cl_amd import abi
    new = {"lg_rollout_traj_index", "lg_rollout_mask_index", "lg_rollout_pad", "lg_rollout_unpad"}
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "lgrollout.h")).read()
    assert new <= set(abi.ROLLOUT_EXPORTS) and new <= set(re.findall(r"\b(lg_\w+)\s*\(", header))
    assert abi.ROLLOUT_MAX_COPIES == 8 and "#define LG_ROLLOUT_MAX_COPIES 8" in header
    lib = ctypes.CDLL(abi.lib_path())
    for sym in new:
        getattr(lib, sym)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
def hidden_at(fx, t, dev):
    """What the policy hands over at step t: ((h, c), (h, c)) for an LSTM, (h, h) for a GRU, None before the first act."""
    import torch
    if t == 0 and bool(fx["hidden_none_at_step0"]):
        return None
    g = lambda n: torch.from_numpy(fx[n][t]).to(dev)
    if fx["n_hid"] == 2:
        return (g("saved_a0"), g("saved_a1")), (g("saved_c0"), g("saved_c1"))
    return g("saved_a0"), g("saved_c0")


def fill(st, fx, path):
    import torch
    dev = st.device
    T, N = fx["rew"].shape
    g = lambda n, t: torch.from_numpy(fx[n][t]).to(dev)
    for t in range(T):
        crit = g("critic_obs", t)
        if path == "add_step":
            st.actions[t].copy_(g("actions", t)); st.values[t].copy_(g("values", t)); st.actions_log_prob[t, :, 0].copy_(g("logp", t))
            st.mu[t].copy_(g("mu", t)); st.sigma[t].copy_(g("sigma", t))
            st.add_step(g("rew", t), g("dones", t).bool(), g("time_outs", t).bool(), float(fx["gamma"]), observations=g("obs", t),
                        critic_observations=crit, hidden_states=hidden_at(fx, t, dev))
        else:
            tr = type(st).Transition()
            tr.observations, tr.critic_observations, tr.actions, tr.values = g("obs", t), crit, g("actions", t), g("values", t)
            tr.actions_log_prob, tr.action_mean, tr.action_sigma = g("logp", t), g("mu", t), g("sigma", t)
            tr.rewards = torch.from_numpy(fx["st_rewards"][t][:, 0]).to(dev)          # as PPO.process_env_step leaves them
            tr.dones = g("dones", t).bool()
            tr.hidden_states = hidden_at(fx, t, dev) if hidden_at(fx, t, dev) is not None else (None, None)
            st.add_transitions(tr)
    st.compute_returns(torch.from_numpy(fx["last_values"]).to(dev), float(fx["gamma"]), float(fx["lam"]))


def check_batches(st, fx, rnn, privileged=True):
    import torch
    T, N = fx["rew"].shape
    c = lambda x: x.cpu().numpy()
    batches = list(st.reccurent_mini_batch_generator(4, 1))
    torch.cuda.synchronize()
    assert len(batches) == 4 and all(len(b) == 11 for b in batches)
    for b, batch in enumerate(batches):
        for n, x in zip(YIELD, batch[:9]):
            want = fx[f"b{b}_{n}"] if (privileged or n != "critic_obs") else fx[f"b{b}_obs"]
            assert x.dtype == torch.float32 and tuple(x.shape) == want.shape, (b, n, x.shape, want.shape)
            if n in EXACT:
                np.testing.assert_array_equal(c(x), want, err_msg=f"{b} {n}")
            else:
                print(f"batch {b} {n}: max abs difference {np.abs(c(x) - want).max():.3e}")
                np.testing.assert_allclose(c(x), want, err_msg=f"{b} {n}", **GAE_TOL[n])
        masks = batch[10]
        assert masks.dtype == torch.bool and masks.shape[0] == T
        np.testing.assert_array_equal(c(masks), fx[f"b{b}_masks"])
        hid_a, hid_c = batch[9]
        critic_key = "hid_c" if st.lstm_critic_hidden == "reference" else "own_c"
        for hid, key in ((hid_a, "hid_a"), (hid_c, critic_key)):
            if rnn == "gru":
                assert torch.is_tensor(hid)
                hid = [hid]
            assert isinstance(hid, list) and len(hid) == fx["n_hid"]
            for i, h in enumerate(hid):
                assert h.is_contiguous() and h.dtype == torch.float32
                np.testing.assert_array_equal(c(h), fx[f"b{b}_{key}{i}"], err_msg=f"{b} {key}{i}")


@pytest.mark.gpu
@pytest.mark.parametrize("rnn", ["lstm", "gru"])
@pytest.mark.parametrize("path", ["add_transitions", "add_step"])
def test_hidden_states_and_mini_batches_match_rsl_rl(rnn, path):
    """Two consecutive rollouts on one storage, filled either way: the stored hidden states equal the reference's (row 0 of the first rollout
    stays zero), the value-derived rows keep the GAE tolerances, and every tensor of every recurrent mini-batch equals the fixture."""
    import torch
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    dev = "cuda:0"
    st = RolloutStorage(48, 24, [45], [61], [12], dev)
    c = lambda x: x.cpu().numpy()
    for k in range(2):
        fx = load(rnn, k)
        fill(st, fx, path)
        torch.cuda.synchronize()
        assert len(st.saved_hidden_states_a) == len(st.saved_hidden_states_c) == fx["n_hid"]
        for i in range(fx["n_hid"]):
            assert st.saved_hidden_states_a[i].shape == (24, 2, 48, 32) and st.saved_hidden_states_a[i].dtype == torch.float32
            np.testing.assert_array_equal(c(st.saved_hidden_states_a[i]), fx[f"saved_a{i}"])
            np.testing.assert_array_equal(c(st.saved_hidden_states_c[i]), fx[f"saved_c{i}"])
        np.testing.assert_array_equal(c(st.observations), fx["obs"]); np.testing.assert_array_equal(c(st.privileged_observations), fx["critic_obs"])
        np.testing.assert_array_equal(c(st.dones), fx["st_dones"])
        np.testing.assert_allclose(c(st.rewards), fx["st_rewards"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(c(st.returns), fx["st_returns"], **GAE_TOL["returns"])
        np.testing.assert_allclose(c(st.advantages), fx["st_advantages"], **GAE_TOL["advantages"])
        check_batches(st, fx, rnn)
        if rnn == "lstm":
            st.lstm_critic_hidden = "own"
            check_batches(st, fx, rnn)
            st.lstm_critic_hidden = "reference"
        st.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("rnn", ["lstm", "gru"])
def test_mini_batches_without_privileged_observations(rnn):
    """No privileged observations: the critic's padded observations are the actor's (rollout_storage.py:192-193)."""
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    st = RolloutStorage(48, 24, [45], [None], [12], "cuda:0", lstm_critic_hidden="own")
    fx = load(rnn, 1)
    fill(st, fx, "add_transitions")
    check_batches(st, fx, rnn, privileged=False)
    batch = next(st.reccurent_mini_batch_generator(4, 1))
    assert batch[1].data_ptr() == batch[0].data_ptr()
    with pytest.raises(ValueError):
        RolloutStorage(48, 24, [45], [None], [12], "cuda:0", lstm_critic_hidden="critic")


@pytest.mark.gpu
def test_short_trajectories_pad_to_max_len_and_mask_to_T():
    import torch
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    fx = np.load(os.path.join(GOLDEN, "rollout_recurrent_short.npz"))
    st = RolloutStorage(3, 6, [5], [None], [2], "cuda:0")
    st.observations.copy_(torch.from_numpy(fx["x"]))
    st.dones.copy_(torch.from_numpy(fx["dones"]))
    index, n_traj, max_len, offset = st.trajectory_index()
    assert (n_traj, max_len, offset) == (6, 3, [0, 2, 4, 6])
    (padded,), _, masks = st.pad_trajectories([st.observations])
    assert padded.shape == (3, 6, 5) and masks.shape == (6, 6) and masks.dtype == torch.bool
    np.testing.assert_array_equal(padded.cpu().numpy(), fx["padded"])
    np.testing.assert_array_equal(masks.cpu().numpy(), fx["masks"])


def random_storage(N, T, D, rate, seed, hidden=True):
    """A storage whose tensors are set directly: observations (D wide), privileged observations (61, or 64 beside a ragged D so that one
    launch mixes float4 and scalar moves), dones at `rate`, one actor hidden tensor with H = 32 and one critic tensor with H = 6."""
    import torch
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    rng = np.random.default_rng(seed)
    st = RolloutStorage(N, T, [D], [61 if D % 4 == 0 else 64], [12], "cuda:0")
    host = dict(obs=rng.normal(size=(T, N, D)).astype(np.float32), critic=rng.normal(size=st.privileged_observations.shape).astype(np.float32),
                dones=(rng.random((T, N, 1)) < rate).astype(np.uint8), hid_a=rng.normal(size=(T, 2, N, 32)).astype(np.float32),
                hid_c=rng.normal(size=(T, 1, N, 6)).astype(np.float32))
    st.observations.copy_(torch.from_numpy(host["obs"])); st.privileged_observations.copy_(torch.from_numpy(host["critic"]))
    st.dones.copy_(torch.from_numpy(host["dones"]))
    if hidden:
        st.saved_hidden_states_a = [torch.from_numpy(host["hid_a"]).to(st.device)]
        st.saved_hidden_states_c = [torch.from_numpy(host["hid_c"]).to(st.device)]
    return st, host


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [0.0, 0.02, 1.0])
@pytest.mark.parametrize("D", [45, 61, 64])
@pytest.mark.parametrize("N", [4096, 4097, 1])
def test_scale_and_ragged_sizes_match_the_restatement(N, D, rate):
    """Whole outputs against the restatement, no element left out: index, offsets, padded observations of both widths (float4 and scalar
    in one launch), masks, start hidden states, and the mini-batch slices.  Done rate 1.0 is the capacity worst case: T * N trajectories."""
    import torch
    T = 24
    st, host = random_storage(N, T, D, rate, seed=N + D)
    r = Restatement(host["dones"])
    index, n_traj, max_len, offset = st.trajectory_index()
    assert (n_traj, max_len) == (r.n_traj, r.max_len) and index.shape == (3, T * N) and index.dtype == torch.int32
    if rate == 1.0:
        assert n_traj == T * N and max_len == 1
    if rate == 0.0:
        assert n_traj == N and max_len == T
    np.testing.assert_array_equal(np.asarray(offset), r.offset)
    np.testing.assert_array_equal(index[:, :n_traj].cpu().numpy(), np.stack([r.env, r.t_start, r.length]))
    padded, hid, masks = st.pad_trajectories([st.observations, st.privileged_observations], (index, n_traj, max_len, offset),
                                             st.saved_hidden_states_a + st.saved_hidden_states_c)
    want = dict(obs=r.pad(host["obs"]), critic=r.pad(host["critic"]), masks=r.masks(), hid_a=r.start_hidden(host["hid_a"]),
                hid_c=r.start_hidden(host["hid_c"]))
    assert padded[0].shape == (max_len, n_traj, D) and masks.shape == (T, n_traj)
    for got, n in ((padded[0], "obs"), (padded[1], "critic"), (masks, "masks"), (hid[0], "hid_a"), (hid[1], "hid_c")):
        assert got.is_contiguous()
        np.testing.assert_array_equal(got.cpu().numpy(), want[n], err_msg=n)
    nmb = 4 if N >= 4 else 1
    per = N // nmb
    batches = list(st.reccurent_mini_batch_generator(nmb, 2))
    assert len(batches) == 2 * nmb
    for b, batch in enumerate(batches):
        lo, hi = r.offset[(b % nmb) * per], r.offset[(b % nmb + 1) * per]
        np.testing.assert_array_equal(batch[0].cpu().numpy(), want["obs"][:, lo:hi])
        np.testing.assert_array_equal(batch[1].cpu().numpy(), want["critic"][:, lo:hi])
        np.testing.assert_array_equal(batch[10].cpu().numpy(), want["masks"][:, lo:hi])
        assert batch[9][0].is_contiguous() and batch[9][1].is_contiguous()
        np.testing.assert_array_equal(batch[9][0].cpu().numpy(), want["hid_a"][:, lo:hi])
        np.testing.assert_array_equal(batch[9][1].cpu().numpy(), want["hid_c"][:, lo:hi])
        assert batch[2].shape == (T, per, 12) and batch[2].data_ptr() == st.actions[:, (b % nmb) * per:].data_ptr()


@pytest.mark.gpu
def test_two_calls_are_bit_identical():
    """No atomics decide the numbering: index, padded tensors, masks and hidden states of two calls on one storage are the same bits."""
    import torch
    st, _ = random_storage(4097, 24, 45, 0.05, seed=3)
    runs = []
    for _ in range(2):
        index, n_traj, max_len, offset = st.trajectory_index()
        padded, hid, masks = st.pad_trajectories([st.observations, st.privileged_observations], (index, n_traj, max_len, offset),
                                                 st.saved_hidden_states_a + st.saved_hidden_states_c)
        runs.append([index[:, :n_traj].clone(), torch.tensor(offset), *padded, *hid, masks])
    for a, b in zip(*runs):
        assert a.shape == b.shape and torch.equal(a.view(torch.uint8) if a.dtype == torch.bool else a, b.view(torch.uint8) if b.dtype == torch.bool else b)
        if a.dtype == torch.float32:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [45, 64])
def test_unpad_inverts_pad(D):
    """unpad_trajectories(pad(x)) == x for the whole rollout and for each mini-batch slice (views of the padded set, env numbers relative
    to the mini-batch, the index rebuilt from the masks alone); its gradient is the pad gather."""
    import torch
    from hcr_genesis_lr_cl_amd.rollout import unpad_trajectories
    T, N = 24, 515
    st, host = random_storage(N, T, D, 0.05, seed=D)
    r = Restatement(host["dones"])
    (padded,), _, masks = st.pad_trajectories([st.observations])
    back = unpad_trajectories(padded, masks)
    assert back.shape == (T, N, D) and back.is_contiguous()
    np.testing.assert_array_equal(back.cpu().numpy(), host["obs"])
    np.testing.assert_array_equal(r.unpad(padded.cpu().numpy()), host["obs"])
    per = N // 4
    for b in range(4):
        lo, hi = r.offset[b * per], r.offset[(b + 1) * per]
        part = unpad_trajectories(padded[:, lo:hi], masks[:, lo:hi])
        np.testing.assert_array_equal(part.cpu().numpy(), host["obs"][:, b * per:(b + 1) * per])
    x = padded.clone().requires_grad_(True)
    w = torch.randn(T, N, D, device=st.device)
    (unpad_trajectories(x, masks) * w).sum().backward()
    np.testing.assert_array_equal(x.grad.cpu().numpy(), r.pad(w.cpu().numpy()))
    keep = torch.from_numpy(np.delete(np.arange(r.n_traj), int(np.flatnonzero(r.length < T)[0]))).to(st.device)
    with pytest.raises(ValueError):
        unpad_trajectories(padded[:, keep], masks[:, keep])      # a trajectory is missing: not whole envs
    last = r.offset[1:-1] - 1                                    # last trajectory of every env but the final one
    j = int(last[np.flatnonzero(r.length[last] != r.length[last + 1])[0]])
    swapped = torch.arange(r.n_traj, device=st.device)
    swapped[j], swapped[j + 1] = j + 1, j                        # two trajectories of different lengths change places across an env boundary:
    with pytest.raises(ValueError):                              # whole envs in total, but one now runs past its env's last step
        unpad_trajectories(padded[:, swapped], masks[:, swapped])


@pytest.mark.gpu
def test_padded_batches_replay_the_sequence_the_policy_saw():
    """The property the feature exists for.  An LSTM memory (nn.LSTM + nn.Linear) runs in collection mode over the rollout step by step,
    its state zeroed at dones and stored before every step; then in batch mode over each mini-batch's padded observations, start states
    and masks, un-padded.  Same sequences, same start states, so the outputs agree to the replay tolerance (f32 GEMMs of different batch
    shapes do not round alike)."""
    import torch
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage, unpad_trajectories
    T, N, dev = 24, 64, "cuda:0"
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    lstm, lin = torch.nn.LSTM(45, 32, num_layers=2).to(dev), torch.nn.Linear(32, 8).to(dev)
    st = RolloutStorage(N, T, [45], [None], [12], dev)
    state, seen = None, []
    with torch.no_grad():
        for t in range(T):
            obs = torch.from_numpy(rng.normal(size=(N, 45)).astype(np.float32)).to(dev)
            done = torch.from_numpy(rng.random(N) < 0.08).to(dev)
            handed = (state, state) if state is not None else None
            out, state = lstm(obs.unsqueeze(0), state)
            seen.append(lin(out.squeeze(0)))
            st.add_step(torch.zeros(N, device=dev), done, None, 0.99, observations=obs, hidden_states=handed)
            for s in state:
                s[:, done, :] = 0.0
        seen = torch.stack(seen)
        worst, first = 0.0, 0
        for b, batch in enumerate(st.reccurent_mini_batch_generator(4, 1)):
            obs_b, (hid_a, _), masks = batch[0], batch[9], batch[10]
            out, _ = lstm(obs_b, tuple(hid_a))
            got = lin(unpad_trajectories(out, masks))
            want = seen[:, b * (N // 4):(b + 1) * (N // 4)]
            assert got.shape == want.shape
            worst = max(worst, float((got - want).abs().max()))
            first += masks.shape[1]
    print(f"collection vs batch mode: max abs difference {worst:.3e} over {first} trajectories")
    assert first > N and worst <= REPLAY_TOL


@pytest.mark.gpu
def test_feed_forward_generator_ignores_hidden_states():
    """mini_batch_generator on a storage that also holds hidden states yields what it yields without them."""
    import torch
    a, _ = random_storage(256, 24, 45, 0.05, seed=9, hidden=True)
    b, _ = random_storage(256, 24, 45, 0.05, seed=9, hidden=False)
    out = []
    for st in (a, b):
        torch.manual_seed(4)
        out.append(list(st.mini_batch_generator(4, 2)))
    assert len(out[0]) == len(out[1]) == 8
    for x, y in zip(*out):
        assert x[9] == (None, None) and x[10] is None and len(x) == 11
        for p, q in zip(x[:9], y[:9]):
            assert torch.equal(p, q)
    with pytest.raises(RuntimeError):
        next(b.reccurent_mini_batch_generator(4, 1))              # nothing stored: an error, not silence


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch():
    import ctypes as C
    import torch
    from hcr_genesis_lr_cl_amd import abi
    lib = abi.load_lib()
    dev = "cuda:0"
    T, N = 4, 8
    dones = torch.zeros(T, N, 1, dtype=torch.uint8, device=dev)
    off = torch.zeros(N + 1, dtype=torch.int32, device=dev)
    traj = torch.zeros(3, T * N, dtype=torch.int32, device=dev)
    head = torch.zeros(2, dtype=torch.int32, device=dev)
    src, dst = torch.zeros(T, N, 5, device=dev), torch.zeros(T, T * N, 5, device=dev)
    p = lambda x: x.data_ptr()

    def refused(rc, text):
        assert rc != 0 and text in lib.lg_last_error().decode(), lib.lg_last_error()

    def copies(n, width=5):
        arr = (abi.LgRowCopy * max(n, 1))()
        for i in range(n):
            arr[i].src, arr[i].dst, arr[i].width, arr[i].src_stride = p(src), p(dst), width, max(width, 1)
        return arr

    refused(lib.lg_rollout_traj_index(T, N, 0, p(off), p(traj), T * N, p(head), 0), "null / empty")
    refused(lib.lg_rollout_traj_index(0, N, p(dones), p(off), p(traj), T * N, p(head), 0), "null / empty")
    refused(lib.lg_rollout_traj_index(1 << 20, 1 << 20, p(dones), p(off), p(traj), T * N, p(head), 0), "overflows")
    refused(lib.lg_rollout_traj_index(T, N, p(dones), p(off), p(traj), N - 1, p(head), 0), "capacity")
    refused(lib.lg_rollout_pad(T, N, 0, T * N, N, T, copies(1), 1, None, None, 0, 0, 0), "null / empty")
    refused(lib.lg_rollout_pad(1 << 20, 1 << 20, p(traj), T * N, N, T, copies(1), 1, None, None, 0, 0, 0), "overflows")
    refused(lib.lg_rollout_pad(T, N, p(traj), T * N, N, T, copies(1, width=0), 1, None, None, 0, 0, 0), "width < 1")
    refused(lib.lg_rollout_pad(T, N, p(traj), T * N, N, T, copies(9), 9, None, None, 0, 0, 0), "bad source list")
    refused(lib.lg_rollout_pad(T, N, p(traj), N - 1, N, T, copies(1), 1, None, None, 0, 0, 0), "capacity below n_traj")
    refused(lib.lg_rollout_pad(T, N, p(traj), T * N, N, T, copies(1), 1, copies(1), (C.c_int32 * 1)(0), 1, 0, 0), "layers < 1")
    refused(lib.lg_rollout_unpad(T, N, p(traj), T * N, N, T, p(dst), p(src), 0, 0), "width < 1")
    refused(lib.lg_rollout_unpad(T, N, p(traj), N - 1, N, T, p(dst), p(src), 5, 0), "capacity below n_traj")
    refused(lib.lg_rollout_mask_index(T, N, 0, p(traj), N, p(head), 0), "null / empty")
    torch.cuda.synchronize()
    assert not traj.any() and not head.any() and not dst.any()                  # nothing was launched

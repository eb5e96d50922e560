"""Rollout-side fusion: the record and GAE kernels behind hcr_genesis_lr_cl_amd.rollout.RolloutStorage against
golden vectors produced by rsl_rl's own PPO + RolloutStorage (tests/golden/rollout_gae.npz).  Tolerance 1e-5 (f32 recurrence
over 24 steps with FMA contraction; mean / std accumulated in f64 on the device, f32 in torch).

Below the fixture tests (N = 48, T = 24: one workgroup, one partial wave), the feed-forward kernels at the sizes the benchmark runs them at
and at every edge of their grids, against float64 references (oracle/rollout_oracle.py) with bounds that come from the reference's own
float32 error or from the number format, never from the kernels:

  * GAE (`gae_kernel`, `adv_normalize_kernel`), GAE_CASES: returns within 4 * err_ref + 1 ulp(max |returns|) of the float64 recurrence,
    err_ref being the error of the plain float32 restatement on the same inputs; then, separately, the normalised advantages within
    4 ulp(max |normalised advantage|) of float64 normalisation of the kernel's own raw advantages (returns - values reproduces them bit
    for bit), so that a wave or block lost from the (sum, sum of squares) reduction cannot hide under the recurrence's tolerance;
  * the record kernel (`rollout_record_kernel`): every destination row inside a sentinel-filled allocation that is compared whole;
  * `add_step` / `add_transitions` input handling, `mini_batch_generator` contents and `get_statistics`.

Measured on an MI355X (gfx950) over GAE_CASES: the returns' error is at most 7.022e-06 and at most 1.38 x err_ref of its case; the
normalised advantages are within 1.52 ulp of the case's scale (bound 4), so no case needs more than the bounds above.  Two calls on one
storage gave bit-identical advantages; the time-out bootstrap is within 0.500 ulp (one fused multiply-add).  Per case:

      N    T  done gamma   lam | max|ret|   err_ref    kernel     bound | max|adv|   adv err   in ulp
      1   24  0.08  0.99  0.95 |    0.243 2.878e-07 2.382e-07 1.166e-06 |    2.803 2.375e-07     1.00
      1  100   0.0   1.0   1.0 |    2.931 5.055e-07 5.055e-07 2.261e-06 |    3.064 8.902e-08     0.37
      1   24   1.0  0.99   0.0 |    0.117 5.588e-08 5.588e-08 2.310e-07 |    2.869 1.969e-07     0.83
     63   24  0.08  0.99  0.95 |    4.372 1.578e-06 1.716e-06 6.790e-06 |    3.146 3.253e-07     1.36
     63    1   0.0   1.0   1.0 |    3.182 1.490e-07 1.490e-07 8.345e-07 |    2.159 9.564e-08     0.40
     64   24   0.0  0.99  0.95 |    4.467 2.292e-06 1.443e-06 9.645e-06 |    3.338 3.235e-07     1.36
     64  100  0.08  0.99   0.0 |    4.070 3.232e-07 3.410e-07 1.770e-06 |    3.647 2.443e-07     1.02
     65   24   1.0   1.0   1.0 |    0.424 1.192e-07 1.192e-07 5.066e-07 |    3.487 2.030e-07     0.85
     65    1  0.08  0.99  0.95 |    2.885 1.771e-07 1.771e-07 9.470e-07 |    2.352 1.566e-07     0.66
    255   24  0.08   1.0   1.0 |    9.279 1.997e-06 1.997e-06 8.941e-06 |    3.921 2.925e-07     1.23
    255  100   0.0  0.99  0.95 |    5.872 4.012e-06 3.673e-06 1.652e-05 |    2.642 2.268e-07     0.95
    256   24  0.08  0.99  0.95 |    4.491 2.073e-06 1.408e-06 8.767e-06 |    3.397 2.077e-07     0.87
    256    1   1.0  0.99   0.0 |    0.465 1.192e-07 1.192e-07 5.066e-07 |    3.263 3.100e-07     1.30
    257   24   0.0  0.99   0.0 |    3.752 3.997e-07 3.508e-07 1.837e-06 |    4.556 4.202e-07     0.88
    257  100   1.0  0.99  0.95 |    0.523 1.192e-07 1.192e-07 5.364e-07 |    4.348 4.152e-07     0.87
   4096   24  0.08  0.99  0.95 |    4.732 2.360e-06 2.123e-06 9.918e-06 |    4.480 3.058e-07     0.64
   4096   24   0.0   1.0   1.0 |   10.819 2.757e-06 2.757e-06 1.198e-05 |    3.504 2.623e-07     1.10
   4096  100  0.08   1.0   1.0 |   30.908 7.022e-06 7.022e-06 3.000e-05 |    9.115 8.491e-07     0.89
   4096    1  0.08  0.99   0.0 |    4.045 3.703e-07 3.313e-07 1.958e-06 |    4.339 4.048e-07     0.85
   4096   24   1.0  0.99   0.0 |    0.507 1.937e-07 1.937e-07 8.345e-07 |    4.310 3.575e-07     0.75
   4096  100   1.0  0.99  0.95 |    0.521 2.384e-07 2.384e-07 1.013e-06 |    5.572 7.246e-07     1.52
   4097   24  0.08  0.99  0.95 |    4.954 2.135e-06 1.871e-06 9.018e-06 |    3.917 2.010e-07     0.84
   4097  100   0.0  0.99   0.0 |    4.587 4.706e-07 6.484e-07 2.359e-06 |    4.917 3.764e-07     0.79
   4097   24   1.0   1.0   1.0 |    0.512 1.788e-07 1.788e-07 7.749e-07 |    4.627 2.576e-07     0.54
   4097    1   0.0  0.99  0.95 |    3.689 4.376e-07 3.468e-07 1.989e-06 |    3.963 2.663e-07     1.12
  32769   24  0.08  0.99  0.95 |    5.373 2.757e-06 2.057e-06 1.151e-05 |    4.529 3.549e-07     0.74
  32769   24   0.0   1.0   1.0 |   10.839 2.950e-06 2.950e-06 1.276e-05 |    3.813 2.794e-07     1.17
  32769    1   1.0  0.99  0.95 |    0.487 1.192e-07 1.192e-07 5.066e-07 |    3.897 1.559e-07     0.65
  32769  100  0.08  0.99   0.0 |    4.808 7.433e-07 6.684e-07 3.450e-06 |    5.136 3.776e-07     0.79
"""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_gae.npz")
STATS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_stats.npz")


def test_rollout_oracle_reproduces_rsl_rl():
    from oracle import rollout_oracle as ro
    fx = np.load(GOLD)
    T = fx["rew"].shape[0]
    for t in range(T):
        np.testing.assert_allclose(ro.bootstrap_rewards(fx["rew"][t], fx["values"][t], fx["time_outs"][t], fx["gamma"]), fx["st_rewards"][t][:, 0],
                                   rtol=1e-6, atol=1e-7)
    np.testing.assert_array_equal(fx["st_dones"][..., 0], fx["dones"])
    ret, adv = ro.compute_returns(fx["values"], fx["st_rewards"], fx["st_dones"], fx["last_values"], fx["gamma"], fx["lam"])
    np.testing.assert_allclose(ret, fx["st_returns"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(adv, fx["st_advantages"], rtol=1e-5, atol=2e-6)
    assert fx["time_outs"].sum() > 10 and fx["dones"].sum() > fx["time_outs"].sum()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["add_step", "add_transitions"])
def test_rollout_storage_matches_rsl_rl(path):
    """Both ways of filling it: the fused `add_step` (bootstrap in the kernel) and the reference's own entry point
    `add_transitions` (rewards already bootstrapped by PPO.process_env_step)."""
    import torch
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    fx = np.load(GOLD)
    T, N = fx["rew"].shape
    dev = "cuda:0"
    st = RolloutStorage(N, T, [45], [61], [12], dev)
    g = lambda k, t: torch.from_numpy(fx[k][t]).to(dev)
    wide = torch.zeros(N, 200, device=dev)                      # the actor observation arrives as a strided window of a wider row
    for t in range(T):
        wide[:, 100:145] = g("obs", t)
        obs = wide[:, 100:145]
        assert not obs.is_contiguous()
        if path == "add_step":
            st.actions[t].copy_(g("actions", t)); st.values[t].copy_(g("values", t)); st.actions_log_prob[t, :, 0].copy_(g("logp", t))
            st.mu[t].copy_(g("mu", t)); st.sigma[t].copy_(g("sigma", t))
            st.add_step(g("rew", t), g("dones", t).bool(), g("time_outs", t).bool(), float(fx["gamma"]), observations=obs, critic_observations=g("critic_obs", t))
        else:
            tr = RolloutStorage.Transition()
            tr.observations, tr.critic_observations, tr.actions, tr.values = obs, g("critic_obs", t), g("actions", t), g("values", t)
            tr.actions_log_prob, tr.action_mean, tr.action_sigma = g("logp", t), g("mu", t), g("sigma", t)
            tr.rewards = torch.from_numpy(fx["st_rewards"][t][:, 0]).to(dev)          # as PPO.process_env_step leaves them
            tr.dones = g("dones", t).bool()
            st.add_transitions(tr)
    with pytest.raises(AssertionError):
        st.add_step(g("rew", 0), g("dones", 0).bool(), None, 0.0)
    st.compute_returns(torch.from_numpy(fx["last_values"]).to(dev), float(fx["gamma"]), float(fx["lam"]))
    torch.cuda.synchronize()
    c = lambda x: x.cpu().numpy()
    np.testing.assert_array_equal(c(st.observations), fx["obs"]); np.testing.assert_array_equal(c(st.privileged_observations), fx["critic_obs"])
    np.testing.assert_array_equal(c(st.dones), fx["st_dones"])
    np.testing.assert_allclose(c(st.rewards), fx["st_rewards"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(c(st.returns), fx["st_returns"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(c(st.advantages), fx["st_advantages"], rtol=1e-5, atol=5e-6)
    assert abs(float(st.advantages.mean())) < 1e-6 and abs(float(st.advantages.std()) - 1.0) < 1e-5
    batches = list(st.mini_batch_generator(4, 1))
    assert len(batches) == 4 and batches[0][0].shape == (T * N // 4, 45) and batches[0][1].shape == (T * N // 4, 61)
    st.clear()
    assert st.step == 0


@pytest.mark.gpu
def test_zero_copy_observation_rows_follow_the_env():
    """With cfg.hip.obs_sets = T + 1 the storage's observation rows are the env's observation copies: after T steps row t
    holds the observation the policy acted on at step t, without any copy; the next rollout starts from row 0 again."""
    import torch
    from hcr_genesis_lr_cl_amd.config import GO2Cfg
    from hcr_genesis_lr_cl_amd.envs import GO2, set_seed
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    T, N = 6, 64
    cfg = GO2Cfg()
    cfg.env.num_envs = N
    cfg.hip.obs_sets = T + 1
    set_seed(1)
    env = GO2(cfg, None, "cuda:0", True)
    obs, _ = env.reset()
    st = RolloutStorage(N, T, [45], [None], [12], "cuda:0", env=env)
    assert st.zero_copy and st.observations.data_ptr() == env._engine.buf.raw("obs_buf").data_ptr()
    g = torch.Generator(device="cuda"); g.manual_seed(0)
    for r in range(3):
        seen = []
        obs = env.get_observations()
        for t in range(T):
            assert obs.data_ptr() == st.observations[t].data_ptr()          # the policy reads the storage row itself
            seen.append(obs.clone())
            st.values[t].zero_()
            obs, _, rew, done, extras = env.step(torch.randn(N, 12, generator=g, device="cuda"))
            st.add_step(rew, done, extras["time_outs"], 0.99)
        torch.cuda.synchronize()
        for t in range(T):
            assert torch.equal(st.observations[t], seen[t]), (r, t)
        last = obs.clone()
        st.clear()
        assert torch.equal(env.get_observations(), last) and env.get_observations().data_ptr() == st.observations[0].data_ptr()


# ---- CPU: the float64 references reproduce the reference's arrays ---------------------------------------------------------------------
def test_f64_oracle_agrees_with_rsl_rl():
    """compute_returns_f64 / normalise_f64 against rsl_rl's own float32 results, at the tolerances the float32 restatement is held to."""
    from oracle import rollout_oracle as ro
    fx = np.load(GOLD)
    ret, raw, adv = ro.compute_returns_f64(fx["values"], fx["st_rewards"], fx["st_dones"], fx["last_values"], fx["gamma"], fx["lam"])
    assert ret.dtype == raw.dtype == adv.dtype == np.float64 and ret.shape == raw.shape == adv.shape == fx["st_returns"].shape
    np.testing.assert_allclose(ret, fx["st_returns"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(adv, fx["st_advantages"], rtol=1e-5, atol=2e-6)
    np.testing.assert_array_equal(raw, ret - fx["values"].astype(np.float64))
    np.testing.assert_allclose(ro.normalise_f64(fx["st_returns"] - fx["values"]), fx["st_advantages"], rtol=1e-5, atol=2e-6)
    assert abs(adv.mean()) < 1e-12 and abs(adv.std(ddof=1) - 1.0) < 1e-7


def test_statistics_oracle_reproduces_rsl_rl():
    """rollout_oracle.get_statistics against values recorded from the reference's RolloutStorage.get_statistics (rollout_stats.npz).  The
    mean length is exact (small integers).  The reference's mean reward is a float32 sum of n values divided by n: its error is at most
    (n - 1) * 2^-24 * mean|x| for the sum plus one rounding of the quotient, which is the bound used."""
    from oracle import rollout_oracle as ro
    fx = np.load(STATS)
    names = sorted(k[:-len("_dones")] for k in fx.files if k.endswith("_dones"))
    assert names == ["all", "first", "last", "none", "random"]
    for n in names:
        dones, rewards = fx[n + "_dones"], fx[n + "_rewards"]
        before = dones.copy()
        length, reward = ro.get_statistics(dones, rewards)
        np.testing.assert_array_equal(dones, before)
        assert length.dtype == np.float32 and length == fx[n + "_length"], (n, length, fx[n + "_length"])
        bound = (rewards.size - 1) * 2.0 ** -24 * np.abs(rewards).mean(dtype=np.float64) + 2.0 ** -24 * abs(reward)
        assert abs(reward - float(fx[n + "_reward"])) <= bound, (n, reward, fx[n + "_reward"], bound)
    T, N = fx["none_dones"].shape[:2]
    assert fx["none_length"] == T and fx["all_length"] == 1 and fx["last_length"] == T          # a done on the last step ends nothing early
    assert fx["first_dones"][1:].sum() == 0 and 1 < fx["first_length"] < T and 1 < fx["random_length"] < T


# ---- GPU: GAE and normalisation at the benchmark's size and at the edges of the grids ---------------------------------------------------
G0, G1, G2 = (0.99, 0.95), (1.0, 1.0), (0.99, 0.0)
# (N, T, done rate, (gamma, lam)): every value of every axis, the corners, and the sizes the kernels' grids change shape at -- 64 (one
# wave), 256 (one block), 4096 (benchmark), 32769 x 24 (above the 2048 x 256 lanes of the normalise grid, so it strides)
GAE_CASES = [
    (1, 24, 0.08, G0), (1, 100, 0.0, G1), (1, 24, 1.0, G2),
    (63, 24, 0.08, G0), (63, 1, 0.0, G1), (64, 24, 0.0, G0), (64, 100, 0.08, G2), (65, 24, 1.0, G1), (65, 1, 0.08, G0),
    (255, 24, 0.08, G1), (255, 100, 0.0, G0), (256, 24, 0.08, G0), (256, 1, 1.0, G2), (257, 24, 0.0, G2), (257, 100, 1.0, G0),
    (4096, 24, 0.08, G0), (4096, 24, 0.0, G1), (4096, 100, 0.08, G1), (4096, 1, 0.08, G2), (4096, 24, 1.0, G2), (4096, 100, 1.0, G0),
    (4097, 24, 0.08, G0), (4097, 100, 0.0, G2), (4097, 24, 1.0, G1), (4097, 1, 0.0, G0),
    (32769, 24, 0.08, G0), (32769, 24, 0.0, G1), (32769, 1, 1.0, G0), (32769, 100, 0.08, G2),
]


def ulp32(x):
    """The spacing of float32 at |x|."""
    return float(np.spacing(np.float32(abs(x))))


def gae_inputs(N, T, rate, seed):
    """Values, rewards with a per-env bias (a wave or a block missing from the sums moves the mean), dones at `rate`, last values."""
    rng = np.random.default_rng(seed)
    rewards = (0.02 + 0.05 * rng.normal(size=(T, N)) + 0.3 * np.sin(np.arange(N))[None, :]).astype(np.float32)[..., None]
    return dict(values=rng.normal(size=(T, N, 1)).astype(np.float32), rewards=rewards,
                dones=(rng.random((T, N, 1)) < rate).astype(np.uint8), last_values=rng.normal(size=(N, 1)).astype(np.float32))


def gae_storage(N, T, host=None):
    """A storage with the smallest rows there are, its GAE inputs set directly."""
    import torch
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    st = RolloutStorage(N, T, [1], [None], [1], "cuda:0")
    if host is not None:
        for k in ("values", "rewards", "dones"):
            getattr(st, k).copy_(torch.from_numpy(host[k]))
    return st


def check_gae(st, host, gamma, lam, tag):
    """Both stages on what `compute_returns` left in `st`; prints one line of figures before it asserts."""
    from oracle import rollout_oracle as ro
    c = lambda x: x.cpu().numpy()
    ret64, _, _ = ro.compute_returns_f64(host["values"], host["rewards"], host["dones"], host["last_values"], gamma, lam)
    ret32, _ = ro.compute_returns(host["values"], host["rewards"], host["dones"], host["last_values"], gamma, lam)
    returns, adv = c(st.returns), c(st.advantages)
    assert returns.dtype == adv.dtype == np.float32 and returns.shape == adv.shape == ret64.shape
    for k in ("values", "rewards", "dones"):
        np.testing.assert_array_equal(c(getattr(st, k)), host[k], err_msg=k)               # inputs are left alone
    # stage 1: the recurrence, against the float32 restatement's own error
    err_ref, err = float(np.abs(ret32 - ret64).max()), float(np.abs(returns - ret64).max())
    bound1 = 4.0 * err_ref + ulp32(np.abs(ret64).max())
    # stage 2: the normalisation of the kernel's own raw advantages
    raw = returns - host["values"]                                                          # float32, as gae_kernel forms it
    want = ro.normalise_f64(raw)
    scale = ulp32(np.abs(want).max())
    err2 = float(np.abs(adv.astype(np.float64) - want).max())
    mean, std = adv.mean(dtype=np.float64), adv.std(ddof=1, dtype=np.float64)
    print(f"{tag}: max|returns| {np.abs(ret64).max():.3f} err_ref {err_ref:.3e} kernel {err:.3e} bound {bound1:.3e} | "
          f"max|adv| {np.abs(want).max():.3f} adv err {err2:.3e} = {err2 / scale:.2f} ulp | mean {mean:+.2e} std-1 {std - 1.0:+.2e}")
    assert np.isfinite(returns).all() and np.isfinite(adv).all()
    assert err <= bound1, (tag, err, err_ref, bound1)
    assert err2 <= 4.0 * scale, (tag, err2, scale)
    assert abs(mean) < 1e-6 and abs(std - 1.0) < 1e-5, (tag, mean, std)
    return returns, adv


@pytest.mark.gpu
@pytest.mark.parametrize("N,T,rate,gl", GAE_CASES, ids=[f"N{n}-T{t}-d{r}-g{g}-l{l}" for n, t, r, (g, l) in GAE_CASES])
def test_gae_at_scale_matches_f64(N, T, rate, gl):
    import torch
    host = gae_inputs(N, T, rate, seed=N * 131 + T)
    st = gae_storage(N, T, host)
    st.compute_returns(torch.from_numpy(host["last_values"]).to(st.device), *gl)
    torch.cuda.synchronize()
    check_gae(st, host, *gl, tag=f"N={N} T={T} done={rate} gamma={gl[0]} lam={gl[1]}")


def test_gae_cases_cover_every_axis():
    """The case table holds what it is meant to: every value of every axis, N = 1 only with T >= 2, and a size above the normalise grid."""
    assert {c[0] for c in GAE_CASES} == {1, 63, 64, 65, 255, 256, 257, 4096, 4097, 32769} and {c[1] for c in GAE_CASES} == {1, 24, 100}
    assert {c[2] for c in GAE_CASES} == {0.0, 0.08, 1.0} and {c[3] for c in GAE_CASES} == {G0, G1, G2}
    assert all(n * t >= 2 for n, t, _, _ in GAE_CASES) and 25 <= len(GAE_CASES) <= 35 and len(set(GAE_CASES)) == len(GAE_CASES)
    assert any(n * t > 2048 * 256 for n, t, _, _ in GAE_CASES) and (4096, 24, 0.08, G0) in GAE_CASES
    for n in (1, 4096, 4097, 32769):                                                        # the corners of rate x (gamma, lam) at the large sizes
        assert {c[2] for c in GAE_CASES if c[0] == n} == {0.0, 0.08, 1.0}


@pytest.mark.gpu
def test_gae_twice_on_one_storage():
    """The second call starts from a zeroed (sum, sum of squares): returns are the same bits; the advantages may differ by the order of
    the float64 atomics alone, i.e. by at most one rounding of the mean or of 1 / std: 1 ulp of the largest |advantage|."""
    import torch
    N, T, gl = 4097, 24, G0
    host = gae_inputs(N, T, 0.08, seed=7)
    st = gae_storage(N, T, host)
    lv = torch.from_numpy(host["last_values"]).to(st.device)
    runs = []
    for k in range(2):
        st.compute_returns(lv, *gl)
        torch.cuda.synchronize()
        runs.append(check_gae(st, host, *gl, tag=f"call {k}"))
    (r0, a0), (r1, a1) = runs
    np.testing.assert_array_equal(r0.view(np.int32), r1.view(np.int32))
    diff = float(np.abs(a0.astype(np.float64) - a1).max())
    print(f"advantages of two calls: {int((a0 != a1).sum())} of {a0.size} differ, max {diff:.3e}")
    assert diff <= ulp32(np.abs(a0).max())


@pytest.mark.gpu
@pytest.mark.parametrize("N,T", [(4097, 24), (1, 2)])
def test_gae_all_zero_rollout(N, T):
    """Zero rewards and values: variance 0, so the normalisation divides by the 1e-8 alone, and 0 * 1e8 is exactly 0."""
    import torch
    st = gae_storage(N, T)
    st.advantages.fill_(float("nan")); st.returns.fill_(float("nan"))
    st.compute_returns(torch.zeros(N, 1, device=st.device), *G0)
    torch.cuda.synchronize()
    assert torch.equal(st.advantages, torch.zeros_like(st.advantages)) and torch.equal(st.returns, torch.zeros_like(st.returns))
    assert torch.isfinite(st.advantages).all()


@pytest.mark.gpu
def test_gae_on_a_side_stream():
    """compute_returns enqueues on the current stream: the inputs are written by torch ops on a side stream, behind a long-running op on
    that stream, and nothing waits for the device between them and the kernels."""
    import torch
    N, T, gl = 4096, 24, G0
    host = gae_inputs(N, T, 0.08, seed=11)
    st = gae_storage(N, T)
    dev = st.device
    staged = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    busy = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        for _ in range(8):
            busy = busy @ busy * 1e-3                                                       # keeps the stream occupied while the rest is enqueued
        for k in ("values", "rewards", "dones"):
            getattr(st, k).copy_(staged[k])
        lv = staged["last_values"] * 1.0
        st.compute_returns(lv, *gl)
    side.synchronize()
    check_gae(st, host, *gl, tag="side stream")


# ---- GPU: the record kernel; every destination row lies inside a sentinel-filled allocation that is compared whole ----------------------
SENTINEL, SENTINEL_U8, MARGIN = -7777.25, 0xAB, 37
# (width, column offset in the source row, columns behind the window): offset = behind = 0 is a contiguous source (stride == width)
COPY_SETS = {
    "none": [],
    "one_w3_window": [(3, 2, 1)],
    "one_w320": [(320, 0, 0)],
    "all_8_slots": [(1, 0, 0), (3, 5, 0), (45, 0, 0), (61, 100, 39), (64, 0, 0), (320, 0, 0), (1, 3, 4), (64, 1, 0)],
}


class RecordCase:
    """One add_step into row 1 of a three-row storage whose tensors are filled with sentinels: rows 0 and 2 are the margins of the
    reward and done rows.  The copies go through `extra_copies` into rows cut from the middle of one sentinel-filled pool, an odd
    number of floats apart, so that neither the sources nor the destinations are aligned alike."""

    def __init__(self, N, layout, seed):
        import torch
        self.N, self.layout, self.dev = N, layout, "cuda:0"
        self.rng = np.random.default_rng(seed)
        self.wide, offs, at = [], [], MARGIN
        for width, off, behind in layout:
            self.wide.append(self.rng.normal(size=(N, off + width + behind)).astype(np.float32))
            offs.append(at)
            at += N * width + MARGIN
        self.pool_host = np.full(at, SENTINEL, np.float32)
        self.want_pool = self.pool_host.copy()
        for (width, off, _), w, o in zip(layout, self.wide, offs):
            self.want_pool[o:o + N * width] = w[:, off:off + width].reshape(-1)
        self.offs = offs
        self.rew = (0.02 + 0.05 * self.rng.normal(size=N)).astype(np.float32)
        self.values = self.rng.normal(size=(N, 1)).astype(np.float32)
        self.reset = self.rng.random(N) < 0.3
        self.gamma = 0.99
        self.torch = torch

    def run(self, mode):
        """mode: None (no bootstrap; the value row is NaN), "all", "none" or "random" time-outs.  Returns nothing; asserts."""
        from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
        torch, N, dev = self.torch, self.N, self.dev
        st = RolloutStorage(N, 3, [2], [None], [1], dev)
        st.rewards.fill_(SENTINEL); st.dones.fill_(SENTINEL_U8); st.values.fill_(SENTINEL)
        values = np.full((N, 1), np.nan, np.float32) if mode is None else self.values
        st.values[1].copy_(torch.from_numpy(values))
        time_outs = None if mode is None else {"all": np.ones(N, bool), "none": np.zeros(N, bool), "random": self.rng.random(N) < 0.5}[mode]
        pool = torch.from_numpy(self.pool_host).to(dev)
        wide = [torch.from_numpy(w).to(dev) for w in self.wide]
        copies = []
        for (width, off, behind), w, o in zip(self.layout, wide, self.offs):
            src = w[:, off:off + width]
            assert src.stride(0) == off + width + behind and (src.is_contiguous() == (off + behind == 0) or N == 1)
            copies.append((src, pool[o:o + N * width].view(N, width)))
        rew = torch.from_numpy(self.rew).to(dev)
        # bool and uint8 flags both reach the kernel as bytes: alternate between them
        reset = torch.from_numpy(self.reset).to(dev) if mode in (None, "all") else torch.from_numpy(self.reset.astype(np.uint8)).to(dev)
        to = None if time_outs is None else (torch.from_numpy(time_outs).to(dev) if mode != "all" else torch.from_numpy(time_outs.astype(np.uint8)).to(dev))
        st.step = 1
        st.add_step(rew, reset, to, self.gamma, extra_copies=copies)
        torch.cuda.synchronize()
        assert st.step == 2
        c = lambda x: x.cpu().numpy()
        # the sources are unchanged
        np.testing.assert_array_equal(c(rew), self.rew); np.testing.assert_array_equal(c(reset).astype(bool), self.reset)
        if to is not None:
            np.testing.assert_array_equal(c(to).astype(bool), time_outs)
        for w, h in zip(wide, self.wide):
            np.testing.assert_array_equal(c(w), h)
        want_values = np.full((3, N, 1), SENTINEL, np.float32)
        want_values[1] = values
        np.testing.assert_array_equal(c(st.values), want_values)
        # every destination, margins included
        np.testing.assert_array_equal(c(pool), self.want_pool, err_msg=f"copies {mode}")
        want_dones = np.full((3, N, 1), SENTINEL_U8, np.uint8)
        want_dones[1, :, 0] = self.reset
        np.testing.assert_array_equal(c(st.dones), want_dones, err_msg=f"dones {mode}")
        got = c(st.rewards)
        assert (got[0] == np.float32(SENTINEL)).all() and (got[2] == np.float32(SENTINEL)).all(), f"reward margins {mode}"
        if time_outs is None or not time_outs.any():
            np.testing.assert_array_equal(got[1, :, 0], self.rew, err_msg=f"rewards {mode}")
        else:
            # ppo.py:110-111 in float64 (gamma as the ABI's float32); the kernel's one multiply-add, contracted or not, is within 1 ulp of it
            want = self.rew.astype(np.float64) + np.float64(np.float32(self.gamma)) * self.values[:, 0].astype(np.float64) * time_outs
            err = np.abs(got[1, :, 0].astype(np.float64) - want)
            tol = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            print(f"N={N} {mode}: bootstrap error at most {float((err / tol).max()):.3f} ulp")
            assert (err <= tol).all(), f"rewards {mode}"


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(COPY_SETS))
@pytest.mark.parametrize("N", [1, 65, 4096, 4097])
def test_record_kernel_at_scale(N, layout):
    """N = 4097 with a 320-wide row is 1,311,040 floats, above the record grid's 4096 x 256 lanes: the copy loop strides."""
    case = RecordCase(N, COPY_SETS[layout], seed=N + len(layout))
    for mode in (None, "all", "none", "random"):
        case.run(mode)


def test_record_cases_cover_the_issue():
    widths = {w for lay in COPY_SETS.values() for w, _, _ in lay}
    assert widths == {1, 3, 45, 61, 64, 320} and len(COPY_SETS["all_8_slots"]) == 8 and COPY_SETS["none"] == []
    assert any(o + b for _, o, b in COPY_SETS["all_8_slots"]) and any(o + b == 0 for _, o, b in COPY_SETS["all_8_slots"])
    assert 4097 * 320 > 4096 * 256


# ---- GPU: inputs the reference accepts, and inputs the fused path refuses ---------------------------------------------------------------
def _transition(N, dev, seed):
    import torch
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    rng = np.random.default_rng(seed)
    g = lambda *s: torch.from_numpy(rng.normal(size=s).astype(np.float32)).to(dev)
    tr = RolloutStorage.Transition()
    tr.observations, tr.critic_observations, tr.actions, tr.values = g(N, 5), g(N, 7), g(N, 2), g(N, 1)
    tr.actions_log_prob, tr.action_mean, tr.action_sigma = g(N), g(N, 2), g(N, 2)
    tr.rewards = g(N)
    tr.dones = torch.from_numpy(rng.random(N) < 0.4).to(dev)
    return tr


@pytest.mark.gpu
@pytest.mark.parametrize("rew_dtype", ["float32", "float64"])
@pytest.mark.parametrize("done_dtype", ["bool", "uint8", "int32", "int64", "float32"])
def test_add_transitions_stores_what_the_reference_copy_would(done_dtype, rew_dtype):
    """rollout_storage.py:95-96 copy_ whatever dtype they are given into the float32 / uint8 rows (the reference's BaseTask.reset_buf is
    torch.int): every accepted dtype and both shapes give exactly the rows that bool dones and float32 rewards give."""
    import torch
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    N, dev = 65, "cuda:0"
    tr = _transition(N, dev, seed=3)
    base = RolloutStorage(N, 2, [5], [7], [2], dev)
    base.add_transitions(tr)
    want_rew, want_dones = base.rewards[0].clone(), base.dones[0].clone()
    assert torch.equal(want_rew[:, 0], tr.rewards) and torch.equal(want_dones[:, 0].bool(), tr.dones) and 0 < int(tr.dones.sum()) < N
    rew, dones = tr.rewards.to(getattr(torch, rew_dtype)), tr.dones.to(getattr(torch, done_dtype))
    spread = torch.zeros(N, 3, dtype=rew.dtype, device=dev)
    spread[:, 1] = rew
    for shape, r in (((N,), rew), ((N, 1), rew), ((N,), spread[:, 1])):                     # the last: every third element of a wider buffer
        st = RolloutStorage(N, 2, [5], [7], [2], dev)
        st.rewards.fill_(SENTINEL); st.dones.fill_(SENTINEL_U8)
        tr.rewards, tr.dones = r.view(shape), dones.view(shape)
        st.add_transitions(tr)
        torch.cuda.synchronize()
        assert st.step == 1
        assert torch.equal(st.rewards[0], want_rew) and torch.equal(st.dones[0], want_dones), (shape, r.stride())
        assert (st.rewards[1] == SENTINEL).all() and (st.dones[1] == SENTINEL_U8).all()
        assert torch.equal(st.observations[0], tr.observations) and torch.equal(st.privileged_observations[0], tr.critic_observations)


@pytest.mark.gpu
def test_add_step_refuses_wrong_inputs_before_any_launch():
    """The fused path takes bare pointers: a wrong dtype, element count, stride or device is a ValueError before anything is enqueued, not a
    hidden conversion; a ninth copy is the library's refusal, not a truncated list; an overflow stays the reference's AssertionError."""
    import torch
    from hcr_genesis_lr_cl_amd import abi
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    N, T, dev = 8, 3, "cuda:0"
    st = RolloutStorage(N, T, [5], [7], [2], dev)
    st.rewards.fill_(SENTINEL); st.dones.fill_(SENTINEL_U8); st.observations.fill_(SENTINEL); st.privileged_observations.fill_(SENTINEL)
    st.step = 1
    rew, flag = torch.ones(N, device=dev), torch.ones(N, dtype=torch.bool, device=dev)
    every_other = lambda dtype: torch.ones(2 * N, dtype=dtype, device=dev)[::2]
    bad_rew = [rew.double(), rew.half(), rew.int(), torch.ones(N + 1, device=dev), torch.ones(N - 1, device=dev), torch.ones(N, 2, device=dev),
               every_other(torch.float32), torch.ones(1, device=dev).expand(N), rew.cpu(), rew.tolist()]
    bad_flag = [flag.int(), flag.long(), flag.float(), torch.ones(N + 1, dtype=torch.bool, device=dev), torch.ones(N - 1, dtype=torch.uint8, device=dev),
                every_other(torch.bool), every_other(torch.uint8), torch.ones(1, dtype=torch.bool, device=dev).expand(N), flag.cpu()]
    obs, crit = torch.ones(N, 5, device=dev), torch.ones(N, 7, device=dev)
    refused = 0
    for r in bad_rew:
        with pytest.raises(ValueError, match="rew"):
            st.add_step(r, flag, flag, 0.99, observations=obs, critic_observations=crit)
        refused += 1
    for f in bad_flag:
        with pytest.raises(ValueError, match="reset"):
            st.add_step(rew, f, flag, 0.99, observations=obs, critic_observations=crit)
        with pytest.raises(ValueError, match="time_outs"):
            st.add_step(rew, flag, f, 0.99, observations=obs, critic_observations=crit)
        refused += 2
    for src in (obs.double(), torch.ones(N, 6, device=dev), torch.ones(5, N, device=dev).t(), torch.ones(N - 1, 5, device=dev), obs.cpu()):
        with pytest.raises(ValueError, match="row copies"):
            st.add_step(rew, flag, flag, 0.99, observations=src)
        refused += 1
    nine = [(torch.ones(N, 2, device=dev), torch.full((N, 2), SENTINEL, device=dev)) for _ in range(abi.ROLLOUT_MAX_COPIES + 1)]
    with pytest.raises(RuntimeError, match="lg_rollout_record: bad copy list"):
        st.add_step(rew, flag, flag, 0.99, extra_copies=nine)
    torch.cuda.synchronize()
    assert refused == len(bad_rew) + 2 * len(bad_flag) + 5 and st.step == 1
    for x, s in ((st.rewards, SENTINEL), (st.dones, SENTINEL_U8), (st.observations, SENTINEL), (st.privileged_observations, SENTINEL)):
        assert (x == s).all()
    assert all((dst == SENTINEL).all() for _, dst in nine)
    st.add_step(rew, flag, None, 0.0, extra_copies=nine[:abi.ROLLOUT_MAX_COPIES])            # eight are taken, and only row 1 is written
    torch.cuda.synchronize()
    assert st.step == 2 and (st.rewards[1] == 1).all() and (st.dones[1] == 1).all() and (st.rewards[0] == SENTINEL).all() and (st.rewards[2] == SENTINEL).all()
    assert all((dst == 1).all() for _, dst in nine[:-1]) and (nine[-1][1] == SENTINEL).all()
    st.step = T
    with pytest.raises(AssertionError, match="overflow"):
        st.add_step(rew.double(), flag, None, 0.0)                                           # the overflow is reported first, as before
    with pytest.raises(AssertionError, match="overflow"):
        st.add_transitions(_transition(N, dev, seed=1))


# ---- GPU: what a mini-batch holds, and the statistics ---------------------------------------------------------------------------------
BATCH_ORDER = ("observations", "privileged_observations", "actions", "values", "advantages", "returns", "actions_log_prob", "mu", "sigma")


def tag_samples(st):
    """Random contents with column 0 of tensor k (in the order PPO.update unpacks) set to k * T * N + t * N + e: every row names the
    tensor and the sample it came from (9 * T * N stays below 2^24, so float32 holds it).  Returns the host copies, flattened."""
    import torch
    T, N = st.num_transitions_per_env, st.num_envs
    assert 9 * T * N < 1 << 24
    rng = np.random.default_rng(T * N)
    ids = np.arange(T * N, dtype=np.float32).reshape(T, N)
    host = {}
    for k, name in enumerate(BATCH_ORDER):
        x = getattr(st, name)
        if x is None:
            continue
        h = rng.normal(size=tuple(x.shape)).astype(np.float32)
        h[..., 0] = k * T * N + ids
        x.copy_(torch.from_numpy(h))
        host[name] = h.reshape(T * N, -1)
    return host


def check_mini_batches(st, host, nmb, epochs):
    import torch
    T, N = st.num_transitions_per_env, st.num_envs
    per = T * N // nmb
    batches = list(st.mini_batch_generator(nmb, epochs))
    torch.cuda.synchronize()
    assert len(batches) == nmb * epochs
    blocks = []
    for b, batch in enumerate(batches):
        assert len(batch) == 11 and batch[9] == (None, None) and batch[10] is None
        ids = batch[0][:, 0].cpu().numpy().astype(np.int64)
        assert ids.shape == (per,)
        for k, (name, x) in enumerate(zip(BATCH_ORDER, batch[:9])):
            src = host.get(name)
            if src is None:                                                                  # no privileged observations: the critic gets the actor's
                assert name == "privileged_observations" and torch.equal(x, batch[0])
                continue
            assert x.dtype == torch.float32 and x.is_contiguous()
            np.testing.assert_array_equal(x.cpu().numpy(), src[ids], err_msg=f"batch {b}: item {k} is not {name} at the observations' sample ids")
        blocks.append(ids)
    epoch = np.concatenate(blocks[:nmb])
    assert len(epoch) == nmb * per and len(np.unique(epoch)) == len(epoch) and epoch.min() >= 0 and epoch.max() < nmb * per
    if nmb * per > 64:
        assert not np.array_equal(epoch, np.sort(epoch))                                     # a permutation, not the identity
    for b in range(nmb, len(blocks)):
        np.testing.assert_array_equal(blocks[b], blocks[b % nmb], err_msg="later epochs replay the blocks of the first")


@pytest.mark.gpu
@pytest.mark.parametrize("nmb,epochs", [(4, 2), (1, 1), (7, 1)])
@pytest.mark.parametrize("N,T,privileged", [(65, 24, True), (65, 3, True), (4097, 24, False)])
def test_mini_batches_hold_matching_samples(N, T, privileged, nmb, epochs):
    """65 x 24 = 1560 divides by 4 and not by 7, 65 x 3 = 195 by neither, 4097 x 24 = 98328 by 4 and not by 7."""
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    st = RolloutStorage(N, T, [45], [61] if privileged else [None], [12], "cuda:0")
    check_mini_batches(st, tag_samples(st), nmb, epochs)


@pytest.mark.gpu
def test_mini_batches_of_a_zero_copy_storage():
    """`observations` is a slice of the env's observation copies (obs_sets = T + 1): the generator gathers from it like from its own."""
    from hcr_genesis_lr_cl_amd.config import GO2Cfg
    from hcr_genesis_lr_cl_amd.envs import GO2, set_seed
    from hcr_genesis_lr_cl_amd.rollout import RolloutStorage
    T, N = 6, 64
    cfg = GO2Cfg()
    cfg.env.num_envs = N
    cfg.hip.obs_sets = T + 1
    set_seed(1)
    env = GO2(cfg, None, "cuda:0", True)
    env.reset()
    st = RolloutStorage(N, T, [45], [None], [12], "cuda:0", env=env)
    raw = env._engine.buf.raw("obs_buf")
    assert st.zero_copy and st.observations.data_ptr() == raw.data_ptr() and raw.shape[0] == T + 1
    last = raw[T].clone()
    check_mini_batches(st, tag_samples(st), 4, 2)
    assert (raw[T] == last).all()                                                            # the row behind the storage's slice is not touched


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [0.0, 0.05, 1.0])
def test_statistics_match_the_oracle(rate):
    import torch
    from oracle import rollout_oracle as ro
    N, T = 4097, 24
    host = gae_inputs(N, T, rate, seed=int(rate * 100) + 5)
    st = gae_storage(N, T, host)
    length, reward = st.get_statistics()
    torch.cuda.synchronize()
    want_length, want_reward = ro.get_statistics(host["dones"], host["rewards"])
    print(f"done rate {rate}: mean length {float(length)!r} (oracle {float(want_length)!r}), mean reward {float(reward)!r} "
          f"(oracle {want_reward!r}, relative difference {abs(float(reward) - want_reward) / abs(want_reward):.2e})")
    assert length.dtype == torch.float32 and np.float32(length.item()) == want_length
    assert abs(float(reward) - want_reward) <= 1e-6 * abs(want_reward)
    np.testing.assert_array_equal(st.dones.cpu().numpy(), host["dones"])
    if rate == 0.0:
        assert want_length == T
    if rate == 1.0:
        assert want_length == 1

"""The host restatement of the product path's random draws (oracle/philox.py, oracle/draw_map.py), on the CPU: Philox against
the Random123 known answers, the uniform mapping, the structure of the slot -> (env words, counter, word) map of every registered
task, shard invariance, and the statistics of the uniforms the map yields.  tests/test_gpu_draws.py pins the map to the kernels."""
import numpy as np
import pytest

from hcr_genesis_lr_cl_amd import abi
from oracle import draw_map
from oracle.philox import philox4x32_10, u01

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]

TASK_NAMES = ("go2", "go2_wtw", "go2_ee", "go2_ts", "go2_cts", "go2_dreamwaq", "go2_cat", "tron1_pf", "tron1_pf_ee", "tron1_sf")


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = tuple(int(v) for v in philox4x32_10(*ctr, *key))
        assert got == want, [hex(v) for v in got]
    # vectorised: the three vectors in one call
    c = np.array([k[0] for k in KAT], np.uint64).T
    k = np.array([k[1] for k in KAT], np.uint64).T
    out = np.stack(philox4x32_10(*c, *k), 1)
    assert [tuple(int(v) for v in r) for r in out] == [k_[2] for k_ in KAT]


def test_u01_range_and_grid():
    r = np.array([0, 1, 0xFFFFFF, 0x1000000, 0xFFFFFFFF, 0x80000000, 0x12345678], np.uint64)
    u = u01(r)
    assert u.dtype == np.float32
    assert u[0] == 0.0 and u[4] < 1.0 and u[4] == np.float32(1 - 2.0 ** -24) and u[3] == 0.0
    rng = np.random.default_rng(0)
    u = u01(rng.integers(0, 2 ** 32, 1 << 16, dtype=np.uint64))
    assert (u >= 0).all() and (u < 1).all()
    m = u.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(m, np.round(m))


def layout(name):
    from hcr_genesis_lr_cl_amd import builders
    from hcr_genesis_lr_cl_amd.envs import TASKS
    from hcr_genesis_lr_cl_amd.model_compiler import load_model
    cfg = TASKS[name][1]()
    model = load_model(cfg.asset.name)
    task = builders.make_task_cfg(model, cfg)
    return task, model


def documented_batch_wide(name, S):
    if name == "go2_wtw":
        return {S.task_cb + 4, S.task_reset + 4}             # gait index at the callback and at reset
    if name.startswith("tron1"):
        return {S.task_reset}                                # sit coin
    return set()


@pytest.fixture(scope="module", params=TASK_NAMES)
def task_layout(request):
    task, model = layout(request.param)
    return request.param, task, model


def test_map_structure(task_layout):
    name, task, model = task_layout
    S = task.slots
    R = draw_map.rules(S, model.n_legs, model.joints_per_leg, task.obs_layout)
    assert len(R) == S.n_slots
    used = [(s, r) for s, r in enumerate(R) if r is not None]
    # every group that is not observation noise has a rule for its whole width (task groups where the task reads them)
    noise = set(range(S.noise, S.n_slots))
    A = model.n_dof
    for g, w in (("cb_cmd", 3), ("push", 2), ("reset_cmd", 3), ("reset_dof", A), ("reset_root_xy", 2), ("reset_lin_vel", 3),
                 ("reset_ang_vel", 3), ("dr_friction", 1), ("dr_mass", 1), ("dr_com", 3), ("dr_kp", A), ("dr_kd", A), ("dr_joint", 3),
                 ("terrain_level", 1)):
        assert all(R[getattr(S, g) + k] is not None for k in range(w)), g
    # the noisy entries of the actor frame all have a rule, the noise-free ones (zero scale) none
    nv = np.ctypeslib.as_array(task.noise_vec)[:task.obs_frame]
    for i in range(task.obs_frame):
        assert (R[S.noise + i] is not None) == (nv[i] != 0), (i, nv[i])
    # no two slots read the same (env words, counter, word)
    keys = [(r.batch_wide, r.counter, r.word) for _, r in used]
    dup = {k for k in keys if keys.count(k) > 1}
    assert not dup, [(s, r) for s, r in used if (r.batch_wide, r.counter, r.word) in dup]
    assert all(0 <= r.word < 4 for _, r in used)
    # exactly the documented batch-wide slots use the all-ones env words
    assert {s for s, r in used if r.batch_wide} == documented_batch_wide(name, S)
    # and the uniforms follow: batch-wide slots equal across env ids, every other used slot varies
    gids = np.arange(64, dtype=np.uint64) + np.uint64(3 << 32)
    U = draw_map.task_uniforms(task, model, gids, 12345)
    for s, r in used:
        if r.batch_wide:
            assert (U[:, s] == U[0, s]).all(), s
        else:
            assert len(np.unique(U[:, s])) > 32, (s, r)
    assert noise >= {s for s, r in enumerate(R) if r is None and s >= S.noise}


def test_shard_invariance(task_layout):
    name, task, model = task_layout
    base = (1 << 32) + 7                                     # e_hi nonzero
    gids = np.arange(base, base + 1000, dtype=np.uint64)
    full = draw_map.task_uniforms(task, model, gids, 999)
    for a, b in ((0, 1), (0, 333), (333, 1000), (517, 518)):
        np.testing.assert_array_equal(draw_map.task_uniforms(task, model, gids[a:b], 999), full[a:b])
    # a different e_hi is a different env
    other = draw_map.task_uniforms(task, model, gids - np.uint64(1 << 32), 999)
    R = draw_map.rules(task.slots, model.n_legs, model.joints_per_leg, task.obs_layout)
    per_env = [s for s, r in enumerate(R) if r is not None and not r.batch_wide]
    assert (other[:, per_env] != full[:, per_env]).mean() > 0.99


def ks_distance(u):
    x = np.sort(u.astype(np.float64))
    n = len(x)
    i = np.arange(1, n + 1)
    return max(np.max(i / n - x), np.max(x - (i - 1) / n))


def corr(a, b):
    a = a.astype(np.float64) - a.mean()
    b = b.astype(np.float64) - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


STAT_LAYOUTS = ("go2", "go2_wtw", "go2_ee", "go2_ts", "tron1_pf", "tron1_pf_ee", "tron1_sf")   # every distinct (slots, legs, joints, obs layout)


@pytest.mark.parametrize("name", STAT_LAYOUTS)
def test_uniform_statistics(name):
    """KS distance to U(0,1) per slot <= 2.2 / sqrt(n), and |Pearson r| <= 6 / sqrt(n) for every slot pair, for each slot
    against the same slot of env g + 1 and of step t + 1.  2^12 envs x 32 steps per layout (batch-wide slots: 2^17 steps)."""
    task, model = layout(name)
    R = draw_map.rules(task.slots, model.n_legs, model.joints_per_leg, task.obs_layout)
    per_env = [s for s, r in enumerate(R) if r is not None and not r.batch_wide]
    batch = [s for s, r in enumerate(R) if r is not None and r.batch_wide]
    G, T = 1 << 12, 32
    g0, t0 = (1 << 32) - 1000, 40000                          # the env ids cross 2^32
    gids = (np.arange(G + 1, dtype=np.uint64) + np.uint64(g0))
    U = np.stack([draw_map.task_uniforms(task, model, gids, t0 + t) for t in range(T + 1)])   # (T + 1, G + 1, n_slots)
    X = U[:T, :G].reshape(-1, U.shape[-1])
    n = X.shape[0]
    assert n >= 1 << 17
    ks_bound, r_bound = 2.2 / np.sqrt(n), 6 / np.sqrt(n)
    for s in per_env:
        assert ks_distance(X[:, s]) <= ks_bound, (s, R[s])
        assert abs(corr(X[:, s], U[:T, 1:, s].reshape(-1))) <= r_bound, ("env + 1", s)
        assert abs(corr(X[:, s], U[1:, :G, s].reshape(-1))) <= r_bound, ("step + 1", s)
    C = np.corrcoef(X[:, per_env + batch].astype(np.float64), rowvar=False)
    np.fill_diagonal(C, 0)
    k = len(per_env)
    bad = np.argwhere(np.abs(C[:k, :]) > r_bound)            # pairs with at least one per-env slot (batch x batch below)
    assert not len(bad), [((per_env + batch)[i], (per_env + batch)[j], C[i, j]) for i, j in bad[:5]]
    if batch:
        steps = np.arange(1 << 17, dtype=np.int64) + 7
        B = draw_map.task_uniforms(task, model, np.zeros(len(steps), np.uint64), steps)[:, batch]
        nb = len(steps)
        for i, s in enumerate(batch):
            assert ks_distance(B[:, i]) <= 2.2 / np.sqrt(nb), s
            assert abs(corr(B[:-1, i], B[1:, i])) <= 6 / np.sqrt(nb), ("step + 1", s)
            for j in range(i):
                assert abs(corr(B[:, i], B[:, j])) <= 6 / np.sqrt(nb), (s, batch[j])
        # a batch-wide value does not depend on which env asks
        B2 = draw_map.task_uniforms(task, model, np.full(len(steps), 123456789, np.uint64), steps)[:, batch]
        np.testing.assert_array_equal(B, B2)

"""The synthetic MDP fixtures (tests/synthetic_mdp.py) on the CPU: every task's recorded batch reaches the branches the GPU replays
rely on (tests/test_gpu_mdp.py test_kernel_matches_oracle_on_synthetic_batches), record() is deterministic, and the harness's
check fails on an oracle perturbed by one part in 1e4 or by one step of one env's episode length."""
import numpy as np
import pytest

from hcr_genesis_lr_cl_amd import abi, builders
from hcr_genesis_lr_cl_amd.model_compiler import load_model
from tests import mdp_harness as h
from tests import synthetic_mdp as sm

GAIT_QUAD = ("go2_wtw",)
SIT = ("tron1_pf_ee", "tron1_sf")


def _task(task):
    cfg = h.TASKS[task].cfg()
    model = load_model(cfg.asset.name)
    return cfg, model, builders.make_task_cfg(model, cfg)


@pytest.mark.parametrize("N", [4096, 4093])
@pytest.mark.parametrize("task", sm.TASKS)
def test_synthetic_fixture_exercises_the_branches(task, N):
    cfg, model, T = _task(task)
    fx = sm.recorded(task, N)
    steps = len(fx["counter"])
    assert steps >= sm.min_steps(task) and fx["rew"].shape == (steps, N)
    c = fx["counter"]
    assert (np.diff(c) == 1).all() and (c % int(T.push_interval) == 0).any()                       # consecutive, push step inside
    assert not (c % int(T.max_episode_length) == 0).any() or task == "go2"                         # the gate only where it is split
    reset, to = fx["reset"].astype(bool), fx["time_out"].astype(bool)
    fail = reset & ~to
    assert to.any(axis=1).all() and fail.sum() >= 50 and to.sum() >= 200                         # time-outs on every step, failures
    # what made an env fail this step, counted where the oracle's fail_buf went up by one: termination-link force alone,
    # projected gravity alone
    from oracle import mdp_oracle as mo
    term = model.find_link_indices(cfg.asset.terminate_after_contacts_on)
    Fl = fx["script_link_contact_forces"]
    by_force = (np.linalg.norm(Fl[:, :, term], axis=-1) > 10.0).any(-1) if term else np.zeros(reset.shape, bool)
    qs = fx["script_base_quat"]
    pgz = mo.quat_rotate_inverse(qs.reshape(-1, 4), np.tile(np.array([0, 0, -1], np.float32), (qs[..., 0].size, 1)))[:, 2].reshape(reset.shape)
    by_pg = pgz > T.max_projected_gravity
    fb_prev = np.concatenate([np.zeros((1, N), fx["fail_buf"].dtype), fx["fail_buf"][:-1]])
    went_up = (fx["fail_buf"] == fb_prev + 1) & ~reset
    assert (went_up & by_pg & ~by_force).sum() >= 50
    assert (went_up & by_force & ~by_pg).sum() >= 50 or not term
    assert ((reset & ~to) & by_force & ~by_pg).sum() >= 5 or not term                            # failure resets by force alone
    fb, thr = fx["fail_buf"], int(T.fail_threshold)
    assert ((fb == thr) & ~reset).sum() >= 5 and ((fb == thr - 1) & ~reset).sum() >= 5              # at and one below the threshold
    ep = fx["ep_len"]
    assert ((ep % int(T.resample_steps) == 0) & (ep > 0)).any(axis=1).all()                       # callback resampling every step
    cmd = fx["commands"]
    n2 = np.linalg.norm(cmd[..., :2], axis=-1)               # (the yaw column follows the heading command on every step)
    assert (n2 == 0).sum() >= 100 and (np.linalg.norm(cmd[..., :3], axis=-1) > 0.2).sum() >= 1000     # dropped and kept commands
    assert (np.abs(fx["actions_in"]) > T.clip_actions).sum() >= 100                              # actions beyond the clip
    # contacts: feet touching down and leaving between steps
    feet = [int(i) for i in model.arrays["foot_link"][:model.n_legs]]
    fz = fx["script_link_contact_forces"][:, :, feet, 2]
    on = fz > 1.0
    assert (on[1:] & ~on[:-1]).sum() >= 1000 and (~on[1:] & on[:-1]).sum() >= 1000
    if "feet_air_time" in fx.files and T.reward_scales[abi.REWARD_ID["feet_air_time"]] != 0:        # in the oracle's own outputs
        fat, keep = fx["feet_air_time"], ~reset[1:, :, None]
        touch = (fat[:-1] > 0) & (fat[1:] == 0) & keep                 # first contact after air time: the clock restarts
        air = (fat[1:] > fat[:-1]) & (fat[:-1] > 0) & keep             # still in the air: the clock runs on
        assert touch.sum() >= 1000 and air.sum() >= 1000
        if "last_contacts" in fx.files:
            lc = fx["last_contacts"].astype(bool)
            assert (lc[1:] & ~lc[:-1]).sum() >= 1000 and (~lc[1:] & lc[:-1]).sum() >= 1000
    # projected gravity either side of the limit, upside-down bases, headings next to +-pi, pitch next to +-pi/2
    q = fx["script_base_quat"].reshape(-1, 4)
    pg = mo.quat_rotate_inverse(q, np.tile(np.array([0, 0, -1], np.float32), (len(q), 1)))[:, 2]
    assert (pg > T.max_projected_gravity).sum() >= 100 and (pg > 0.9).sum() >= 50
    eul = mo.get_euler_xyz(q)
    assert (np.abs(eul[:, 2]) > np.pi - 0.05).sum() >= 100 and (np.abs(eul[:, 1]) > 1.5).sum() >= 100
    # DOF positions beyond both soft limits
    from hcr_genesis_lr_cl_amd import config as cfgmod
    soft = cfgmod.soft_dof_limits(model, cfg)
    dp = fx["script_dof_pos"]
    assert (dp < soft[:, 0]).sum() >= 100 and (dp > soft[:, 1]).sum() >= 100
    # observations beyond clip_obs: the clip binds somewhere in what the task clips
    if task != "go2_cat":       # go2_cat: actions clipped to +-10 and an unclipped actor history, nothing of it reaches 100
        clipped = [k for k in ("obs", "priv", "feat_new", "priv_new") if k in fx.files and (np.abs(fx[k]) == T.clip_obs).any()]
        assert clipped, "no observation reached clip_obs"
    if task == "go2":                                                                                # command curriculum fired
        assert fx["cmd_range_x"][0][1] == 0.5 and fx["cmd_range_x"][-1][1] == 1.0
    if h.TASKS[task].rough:                                                                             # terrain curriculum
        lv = np.concatenate([fx["init_terrain_levels"][None], fx["terrain_levels"]])
        d, ml = np.diff(lv, axis=0), int(T.max_terrain_level)
        assert (d == 1).sum() >= 50 and (d == -1).sum() >= 50 and ((d != 0) & (np.abs(d) != 1)).sum() >= 10
        assert ((lv[:-1] == 0) & (d == 0) & reset).sum() >= 5                                        # moved down at level 0: stays
        assert (lv == 0).any() and (lv == ml - 1).any()
        assert np.ptp(fx["measured_heights"]) > 0.1
    if task in GAIT_QUAD:
        ts = fx["task_state"]
        th = ts[..., 6:10].reshape(-1, 4)
        assert len({tuple(r) for r in th}) == 4                                                      # every row of the theta table
        pb = (th[:, 2] == th[:, 3]) & (th[:, 0] == 0) & (th[:, 1] == 0)                               # pronk / bound
        assert pb.sum() >= 100 and (ts[..., 4].reshape(-1)[pb] == fx["init_behavior_ranges"][4]).all()
        assert (ts[1:, :, 0] < ts[:-1, :, 0]).sum() >= 500                                           # gait clocks wrapped
        assert (ts[..., 1] < 0.01).any() and (ts[..., 1] > 0.95).any()                               # phi near 0 and 1
    if task in SIT:
        if task == "tron1_pf_ee":
            sit = (np.abs(fx["sim_base_quat"][:, :, 1]) > 0.05) & reset
        else:
            sit = reset & (np.abs(fx["sim_dof_pos"][:, :, 2] - 1.35) < 1e-6)
        assert sit.sum() >= 50 and (reset & ~sit).sum() >= 50                                       # both outcomes of the sit coin
    if task == "go2_cat":
        p = fx["cstr_prob"]
        assert set(np.unique(p)) == {0.0, 0.25, 1.0}
        assert ((np.diff(fx["cstr_sums"], axis=0) > 0).sum(axis=(0, 2)) >= 20).all()                # all nine constraints occur


@pytest.mark.parametrize("task", sm.TASKS)
def test_record_is_deterministic(task):
    a = sm.record(task, sm.synth_fixture(task, 200, seed=3))
    b = sm.record(task, sm.synth_fixture(task, 200, seed=3))
    assert a.keys() == b.keys()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    c = sm.synth_fixture(task, 200, seed=4)
    assert not np.array_equal(a["actions_in"], c["actions_in"])


def _perturbed(how, name=None):
    class Perturbed(h.OracleStepper):
        def __init__(self, spec, fx, N):
            super().__init__(spec, fx, N)
            o = self.o
            if how == "scale":                   # one reward scale of the task, one part in 1e4
                k = abi.reward_id(name, o.model.joints_per_leg)
                o.scales[k] *= np.float32(1 + 1e-4)
            else:                                # one env one step further into its episode
                o.episode_length_buf[N // 2] += 1
    return Perturbed


@pytest.mark.parametrize("how", ["scale", "episode_length"])
@pytest.mark.parametrize("task", sm.TASKS)
@pytest.mark.parametrize("tolerances", ["check-default", "gpu-synthetic"])
def test_check_catches_a_perturbed_oracle(task, how, tolerances):
    """At the oracle's tolerances and at the ones the GPU comparison applies (TaskSpec.synth_tol).  The perturbed scale is the one
    of the reward term with the largest episode sum of the batch, every term's sum changes by 1e-4 of itself."""
    spec = h.TASKS[task]
    fx = sm.recorded(task, 256)
    tol = h.ORACLE_TOL if tolerances == "check-default" else spec.synth_tol()
    h.replay(spec, fx, h.OracleStepper, tol)                                           # the unperturbed oracle passes
    names = [str(n) for n in fx["reward_names"]]
    name = names[int(np.argmax(np.abs(fx["episode_sums"][-1]).max(axis=1)))]
    with pytest.raises(AssertionError):
        h.replay(spec, fx, _perturbed(how, name), tol)

"""GPU parity, MDP phases: the HIP kernel (PRE|POST|RESET launches through the C ABI, physics
read-backs and uniform draws injected) against (a) the golden vectors produced by the
reference's own GO2 class and (b) the numpy oracle at 4096 envs on random inputs.
Float tolerance 1e-5 abs/rel (f32 sums in a different association order + fused multiply-add);
integer / boolean outputs exact."""
import os

import numpy as np
import pytest

from oracle import mdp_oracle as mo
from tests import mdp_harness as h
from tests.mdp_harness import get, load_sim, make_engine, put

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["64", "1", "0"], ids=["history-window", "history-window-min-slack", "history-shift"])
def history_mode(request, monkeypatch):
    """Stacked observations three ways: sliding window with the default slack, with the smallest legal slack (a
    compaction every `stack` steps), and the in-place shift."""
    monkeypatch.setenv("LG_OBS_SLACK", request.param)

@pytest.fixture(params=["split", "fused-profile"])
def tail(request, monkeypatch, history_mode):
    """Which instantiation of the MDP phases a golden replay goes through:
      split          env_step_kernel<PRE | POST | RESET> (one leg per lane) -- the generic body;
      fused-profile  the component-layout tail of the task's profile, i.e. the code the fused launch of env.step() / bench.py runs after its
                     physics (quad_sim_kernel<.., PROF 1 / 2 / 3 / 4 / 6>), in its INJ instantiation: the sub-steps and the read-back are
                     replaced by loads of the recorded read-backs, Philox by the recorded uniforms (lg_quad.h).  Needs the sliding history
                     window (the tails hard-wire it): skipped in the history-shift mode.
    Every PRE | POST | RESET launch of the test is checked through lg_last_kernel: it ran the instantiation the parameter names."""
    from hcr_genesis_lr_cl_amd import abi
    from hcr_genesis_lr_cl_amd.engine import Engine
    if request.param == "fused-profile":
        if os.environ.get("LG_OBS_SLACK") == "0":
            pytest.skip("the component-layout tails need the sliding history window")
        monkeypatch.setenv("LG_SIM_LAYOUT", "2")
    seen, orig = [], Engine.step

    def step(self, phases, actions, counter):
        orig(self, phases, actions, counter)
        if phases == (abi.PHASE_PRE | abi.PHASE_POST | abi.PHASE_RESET):
            seen.append(self.last_kernel())
    monkeypatch.setattr(Engine, "step", step)
    yield request.param
    if seen:
        inj = ["lg_launch_quad_inj" in k for k in seen]
        assert all(inj) if request.param == "fused-profile" else not any(inj), (request.param, sorted(set(seen)))


def replay_golden(task):
    """The kernel through the task's golden fixture at the kernel tolerances of tests/mdp_harness.py TASKS."""
    spec = h.TASKS[task]
    h.replay(spec, h.golden(spec), h.KernelStepper, spec.golden_tol())


def test_kernel_reproduces_reference_go2_golden_vectors(tail):
    replay_golden("go2")


def test_kernel_matches_numpy_oracle_at_4096_envs():
    import torch
    from hcr_genesis_lr_cl_amd import abi
    from tests.golden_inputs import random_mdp_inputs
    N = 4096
    eng, model, cfg, task = make_engine(N)
    rng = np.random.default_rng(11)
    origins = np.zeros((N, 3), np.float32); origins[:, :2] = rng.uniform(-40, 40, (N, 2))
    put(eng, "env_origins", origins)
    orc = mo.MdpOracle(model, cfg, task, N, origins)
    ep = rng.integers(0, 1001, N).astype(np.int32)
    cmds = (rng.normal(size=(N, 4)) * [0.4, 0.4, 0.5, 1.5]).astype(np.float32)
    orc.episode_length_buf[:] = ep; orc.commands[:] = cmds
    put(eng, "episode_length_buf", ep); put(eng, "commands", cmds)
    fb = rng.integers(0, 7, N); orc.fail_buf[:] = fb; put(eng, "fail_buf", fb)
    for t, counter in enumerate((748, 749, 750, 751)):
        sim, actions, R = random_mdp_inputs(rng, model, cfg, N, task.slots.n_slots)
        load_sim(eng, sim); put(eng, "rand_in", R)
        eng.step(abi.PHASE_PRE | abi.PHASE_POST | abi.PHASE_RESET, torch.from_numpy(actions).cuda(), counter)
        orc.step(sim, actions, R, counter)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(get(eng, "reset_buf").astype(bool), orc.reset_buf)
        np.testing.assert_array_equal(get(eng, "episode_length_buf"), orc.episode_length_buf)
        np.testing.assert_array_equal(get(eng, "fail_buf"), orc.fail_buf)
        np.testing.assert_array_equal(get(eng, "last_contacts").astype(bool), orc.last_contacts)
        for name, ref in (("obs_buf", orc.obs_buf), ("rew_buf", orc.rew_buf), ("commands", orc.commands),
                          ("feet_air_time", orc.feet_air_time), ("episode_sums", orc.episode_sums),
                          ("dof_pos", sim["dof_pos"]), ("base_pos", sim["base_pos"]), ("base_lin_vel_w", sim["base_lin_vel_w"]),
                          ("friction_values", orc.friction_values), ("base_com_bias", orc.base_com_bias)):
            # the yaw command goes through atan2f of the forward vector (device libm, few ulp) and a
            # difference of angles: 5e-5 rad absolute on that column, 1e-5 elsewhere
            tol = 5e-5 if name in ("commands", "obs_buf") else 1e-5
            np.testing.assert_allclose(get(eng, name), ref, rtol=1e-5, atol=tol, err_msg=f"{name} step {t}")
        # per-env reset snapshots behind the lazy extras["episode"] means
        if orc.done_sums is not None:
            sums, cnt = orc.done_sums
            m = get(eng, "episode_done_step") == counter
            assert m.sum() == cnt
            np.testing.assert_allclose(get(eng, "episode_done_sums")[:, m].sum(1), sums, rtol=1e-4, atol=1e-4)


# ------------------------------- go2_wtw ------------------------------------------------------
def test_kernel_reproduces_reference_go2_wtw_golden_vectors(tail):
    """Env 0 is excluded: the reference couples it to the whole batch through two index-flatten bugs
    (go2_wtw.py:33-34, 455-462) which the kernel does not reproduce (envs/go2_wtw.py docstring)."""
    replay_golden("go2_wtw")


# ------------------------------- every task against the oracle on synthetic batches ---------------------------------------
def _synth_params():
    """(task, tail, history mode): fused-profile only where the task has an INJ profile tail and only with the sliding window
    (the component-layout tails hard-wire it); go2_cat, tron1_pf and tron1_sf are split only."""
    modes = (("64", "history-window"), ("1", "history-window-min-slack"), ("0", "history-shift"))
    return [pytest.param(task, tail, m, id=f"{task}-{tail}-{mid}") for task, spec in h.TASKS.items() for tail in ("split", "fused-profile")
            for m, mid in modes if tail == "split" or (spec.inj_tail and m != "0")]


@pytest.mark.parametrize("N", [4096, 4093])
@pytest.mark.parametrize("task,tail,history_mode", _synth_params(), indirect=["tail", "history_mode"])
def test_kernel_matches_oracle_on_synthetic_batches(task, N, tail):
    """Every task's MDP instantiations against the oracle on a synthetic batch (tests/synthetic_mdp.py): 4096 envs, and 4093 for a
    partly filled last wave / workgroup / PROF 6 group of 8 envs; long enough for two compactions of the smallest-slack history
    window; inputs that cross every decision of the MDP phases with a margin.  Expected values are the oracle's, recorded once
    per batch; tolerances of TaskSpec.synth_tol (the golden replays' kernel tolerances)."""
    from tests import synthetic_mdp as sm
    spec = h.TASKS[task]
    h.replay(spec, sm.recorded(task, N), h.KernelStepper, spec.synth_tol())


def test_wtw_env_runs_and_histories_shift():
    import torch
    from hcr_genesis_lr_cl_amd.envs import make_env
    env, cfg = make_env("go2_wtw", 256)
    obs, priv = env.reset()
    assert obs.shape == (256, 305) and priv.shape == (256, 495)
    g = torch.Generator(device="cuda"); g.manual_seed(0)
    prev = None
    for t in range(30):
        obs, priv, rew, done, _ = env.step(torch.randn(256, 12, generator=g, device="cuda"))
        if prev is not None:
            keep = ~done
            # frames 1..4 of the previous step are frames 0..3 now (oldest -> newest)
            assert torch.equal(obs[keep][:, :244], prev[0][keep][:, 61:])
            assert torch.equal(priv[keep][:, :396], prev[1][keep][:, 99:])
            assert (obs[done][:, :244] == 0).all()
        prev = (obs.clone(), priv.clone())
    assert torch.isfinite(obs).all() and torch.isfinite(priv).all() and torch.isfinite(rew).all()
    assert float(env.gait_period.min()) >= 0.3 and float(env.phi.max()) < 1.0


# ------------------------------- go2_ee (rough terrain) ------------------------------------------
def test_kernel_reproduces_reference_go2_ee_golden_vectors(tail):
    replay_golden("go2_ee")


@pytest.mark.parametrize("head", ["go2_ts", "go2_cts", "go2_dreamwaq", "go2_cat"])
def test_kernel_reproduces_reference_head_golden_vectors(head, tail):
    """the other Go2-rough heads.  Golden vectors from the reference's own Go2TS / Go2CTS / Go2Dreamwaq classes as
    configured (tests/golden/gen_mdp_fixtures.py, GEN["go2_ts"] ...): actor frame, newest frames of the 20-deep actor history and the
    5-deep critic stack (full stacks at the last step), the single-frame auxiliary output, rewards, resets, curricula."""
    if head == "go2_cat" and tail == "fused-profile":
        pytest.skip("go2_cat has no component-layout tail: its MDP phases are the leg-per-lane launch in the product too")
    replay_golden(head)


@pytest.mark.parametrize("head", ["go2_ts", "go2_cts", "go2_dreamwaq", "go2_cat"])
def test_head_env_returns_the_reference_tuple(head):
    """Arity and shapes of step() / reset() / get_observations() (legged_robot_ts.py:59-83, legged_robot_dreamwaq.py:63-89)."""
    import torch
    from hcr_genesis_lr_cl_amd.envs import make_env
    env, cfg = make_env(head, 64)
    r = env.reset()
    out = env.step(torch.zeros(64, 12, device="cuda"))
    if head == "go2_dreamwaq":
        assert len(r) == 5 and len(out) == 8
        obs, priv, hist, explicit, nxt, rew, done, extras = out
        assert explicit.shape == (64, 24) and nxt.shape == (64, 45) and priv.shape == (64, 5 * 177)
    else:
        assert len(r) == 4 and len(out) == 7
        obs, priv, hist, critic, rew, done, extras = out
        assert priv.shape == (64, 99) and critic.shape == (64, 5 * 177)
        if head == "go2_cts":
            assert "teacher_terrain_level" in extras["episode"] and "student_terrain_level" in extras["episode"]
        if head == "go2_cat":
            g = torch.Generator(device="cuda"); g.manual_seed(0)
            for _ in range(30):
                out = env.step(torch.randn(64, 12, generator=g, device="cuda") * 3.0)
            ep = out[-1]["episode"]
            p = env.cstr_prob
            assert 0.0 <= float(ep["cstr_probs"]) <= 1.0 and "rew_cstr_action_rate" in list(ep)
            assert set(p.unique().tolist()) <= {0.0, 0.25, 1.0} and float(p.max()) > 0
            assert float(env.episode_sums["cstr_action_rate"].max()) > 0 and (out[4] >= 0).all()
            obs, priv, hist, critic, rew, done, extras = out
    assert obs.shape == (64, 45) and hist.shape == (64, 900) and rew.shape == (64,) and done.dtype == torch.bool
    assert torch.equal(obs, hist[:, -45:]) and all(torch.isfinite(o).all() for o in out[:-3])
    assert [o.shape for o in env.get_observations()] == [o.shape for o in out[:len(r)]]


def test_sim_phase_terrain_sampling_matches_numpy_sampler():
    """a7/a8 on the GPU: after a physics step on the heightfield, measured_heights / height_around_feet /
    normals / contact states written by the kernel equal the (reference-pinned) numpy sampler applied to
    the kernel's own final base pose and feet positions."""
    import torch
    from hcr_genesis_lr_cl_amd import abi
    from hcr_genesis_lr_cl_amd.envs import make_env
    np.random.seed(3)
    env, cfg = make_env("go2_ee", 512)
    env.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(2)
    for _ in range(25):
        env.step(torch.randn(512, 12, generator=g, device="cuda"))
    # one bare physics step so that the read-backs are not modified by resets afterwards
    env._engine.step(abi.PHASE_SIM, torch.randn(512, 12, generator=g, device="cuda"), 0)
    torch.cuda.synchronize()
    b = {k: v.detach().cpu().numpy() for k, v in env._engine.buf.items() if torch.is_tensor(v)}
    t, c = env.simulator._terrain, cfg.terrain
    hp = b["height_points"]
    mh = mo.sample_heights(b["base_pos"], b["base_quat"], hp, t.height_field_raw, c.border_size, c.horizontal_scale, c.vertical_scale)
    har, nrm = mo.feet_terrain_info(b["feet_pos"], t.height_field_raw, c.border_size, c.horizontal_scale, c.vertical_scale)
    # a sample point within float round-off of a cell edge may fall in the neighbouring cell: allow a handful
    bad = np.abs(b["measured_heights"] - mh) > 1e-6
    assert bad.mean() < 2e-3, bad.mean()
    assert (np.abs(b["height_around_feet"] - har) > 1e-6).mean() < 2e-3
    assert (np.abs(b["normal_vector_around_feet"] - nrm) > 1e-5).mean() < 5e-3
    st = (np.linalg.norm(b["link_contact_forces"], axis=-1) > 1.0).astype(np.float32)
    np.testing.assert_array_equal(b["link_contact_states"], st)
    assert np.ptp(mh) > 0.05          # the robots really are on uneven ground


def test_go2_ee_env_surface_and_terrain_curriculum():
    import torch
    from hcr_genesis_lr_cl_amd.envs import make_env
    np.random.seed(3)
    env, cfg = make_env("go2_ee", 1024)
    f, l, p = env.reset()
    assert f.shape == (1024, 900) and l.shape == (1024, 24) and p.shape == (1024, 870)
    lv0 = env.simulator.terrain_levels.clone()
    assert int(lv0.max()) <= 1                       # max_init_terrain_level (genesis_simulator.py:518-522)
    env.episode_length_buf[:] = torch.randint(0, 1000, (1024,), device="cuda", dtype=torch.int32)
    g = torch.Generator(device="cuda"); g.manual_seed(4)
    for t in range(300):
        f, l, p, rew, done, extras = env.step(torch.randn(1024, 12, generator=g, device="cuda") * 0.3)
    assert torch.isfinite(f).all() and torch.isfinite(p).all() and torch.isfinite(rew).all()
    lv = env.simulator.terrain_levels
    assert int(lv.min()) >= 0 and int(lv.max()) < 10 and not torch.equal(lv, lv0)
    org = env.simulator.env_origins
    to = torch.from_numpy(env.simulator._terrain.env_origins).float().cuda()
    assert torch.allclose(org, to[lv.long(), env.simulator.terrain_types.long()])
    assert "terrain_level" in list(extras["episode"])


# ------------------------------- tron1_pf_ee (biped) ----------------------------------------------
def test_kernel_reproduces_reference_tron1_pf_ee_golden_vectors(tail):
    """Env 0 excluded for the same reason as in the wtw test (reference index-flatten bugs on the gait clock / indicator)."""
    replay_golden("tron1_pf_ee")


def test_tron1_env_runs_physics_and_mdp():
    import torch
    from hcr_genesis_lr_cl_amd.envs import make_env
    np.random.seed(3)
    env, cfg = make_env("tron1_pf_ee", 512)
    f, l, p = env.reset()
    assert f.shape == (512, 310) and l.shape == (512, 17) and p.shape == (512, 1340)
    g = torch.Generator(device="cuda"); g.manual_seed(6)
    nres = 0
    for t in range(200):
        f, l, p, rew, done, extras = env.step(torch.randn(512, 6, generator=g, device="cuda") * 0.5)
        nres += int(done.sum())
    assert torch.isfinite(f).all() and torch.isfinite(p).all() and torch.isfinite(rew).all() and torch.isfinite(l).all()
    s = env.simulator
    assert s.link_contact_forces.shape == (512, 9, 3) and s.feet_pos.shape == (512, 2, 3) and s.dof_pos.shape == (512, 6)
    assert float(s.dr_joint_armature.min()) >= 0.11 - 1e-6 and float(s.dr_joint_armature.max()) <= 0.13 + 1e-6
    assert nres > 0 and float(s.base_pos[:, 2].max()) < 3.0
    # sit-pose resets happen (pitched base, tron1_pf_ee.py:277-310)
    assert float(env.theta.max()) <= 1.5 + 1e-6


# ------------------------------- tron1_pf (biped on the plane) ------------------------------------
def test_kernel_reproduces_reference_tron1_pf_golden_vectors():
    """TRON1PF on the plane, golden vectors from the reference's own class (gen_mdp_fixtures.py, GEN["tron1_pf"])."""
    replay_golden("tron1_pf")


def test_tron1_pf_env_rollout():
    """The task through the VecEnv surface: 5-tuple, shapes of tron1_pf_config.py:6-14, physics + MDP fused for the biped."""
    import torch
    from hcr_genesis_lr_cl_amd.envs import make_env
    env, cfg = make_env("tron1_pf", 256)
    obs, priv = env.reset()
    assert obs.shape == (256, 135) and priv.shape == (256, 225) and env.num_actions == 6
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    n_reset = 0
    for t in range(200):
        obs, priv, rew, done, extras = env.step(torch.randn(256, 6, generator=g, device="cuda"))
        n_reset += int(done.sum())
    assert torch.isfinite(obs).all() and torch.isfinite(priv).all() and torch.isfinite(rew).all()
    assert n_reset > 50 and "rew_no_fly" in list(extras["episode"])
    assert float(env.simulator.base_pos[:, 2].max()) < 1.5


def test_cat_job_wide_flag_is_raised_by_the_physics_launch():
    """go2_cat: the SIM launch raises command_ranges[CR_ANY_FAST + (counter & 1)] iff some env moves a joint faster than 4 rad/s
    (what the reference's (N,) x (N,1) broadcast amounts to, go2_cat.py:179-180); the MDP launch clears the other slot."""
    import torch
    from hcr_genesis_lr_cl_amd import abi
    from hcr_genesis_lr_cl_amd.envs import make_env
    env, cfg = make_env("go2_cat", 256)
    env.reset()
    eng, cr = env._engine, env._engine.buf["command_ranges"]
    c = env.common_step_counter
    for scale, want in ((0.0, 0.0), (6.0, 1.0), (0.0, None)):
        c += 1
        if scale == 0.0 and want is not None:        # everybody at rest in the air: nothing moves fast
            s = env.simulator
            s.dof_vel.zero_(); s._base_lin_vel_w.zero_(); s._base_ang_vel_w.zero_(); s.base_pos[:, 2] += 1.0
            s.dof_pos.copy_(s.default_dof_pos.expand_as(s.dof_pos))
        eng.step(abi.PHASE_PRE | abi.PHASE_SIM, torch.randn(256, 12, device="cuda") * scale, c)
        torch.cuda.synchronize()
        flag = float(cr[abi.CR_ANY_FAST + (c & 1)])
        assert flag == float((env.simulator.dof_vel.abs() > 4.0).any())
        if want is not None:
            assert flag == want
        eng.step(abi.PHASE_POST | abi.PHASE_RESET, None, c)
        torch.cuda.synchronize()
        assert float(cr[abi.CR_ANY_FAST + ((c + 1) & 1)]) == 0.0
    env.common_step_counter = c
    with pytest.raises(RuntimeError):
        eng.step(abi.PHASE_ALL, torch.zeros(256, 12, device="cuda"), c + 1)      # CaT cannot run as one launch


# ------------------------------- tron1_sf (8-DOF sole-foot biped on the plane) ---------------------
def test_kernel_reproduces_reference_tron1_sf_golden_vectors():
    """TRON1SF, golden vectors from the reference's own class (gen_mdp_fixtures.py, GEN["tron1_sf"]): four-joint legs in the
    MDP phases, the sole-foot reward terms, the sit-pose coin, the 10-frame stacks with the kp / kd blocks in the critic frame."""
    replay_golden("tron1_sf")


def test_tron1_sf_env_rollout():
    """The task through the VecEnv surface: 5-tuple, shapes of tron1_sf_config.py:6-15, physics + MDP in one leg-per-lane launch."""
    import torch
    from hcr_genesis_lr_cl_amd.envs import make_env
    env, cfg = make_env("tron1_sf", 256)
    obs, priv = env.reset()
    assert obs.shape == (256, 330) and priv.shape == (256, 720) and env.num_actions == 8
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    n_reset = 0
    for t in range(300):
        obs, priv, rew, done, extras = env.step(torch.randn(256, 8, generator=g, device="cuda") * 0.5)
        n_reset += int(done.sum())
    assert torch.isfinite(obs).all() and torch.isfinite(priv).all() and torch.isfinite(rew).all()
    keys = list(extras["episode"])
    assert n_reset > 20 and {"rew_foot_flat", "rew_hip_pos_zero_command", "rew_no_fly"} <= set(keys)
    assert float(env.simulator.base_pos[:, 2].max()) < 1.6 and float(env.simulator.dof_vel.abs().max()) <= 30.0 + 1e-3

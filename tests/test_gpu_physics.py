"""GPU parity, physics phase: HIP SIM launch (through the C ABI) vs. the f64 CPU oracle on the same seeded states, and first
principles on the kernel alone.  Cases, tolerances and the comparison are tests/physics_harness.py's;
tests/test_physics_harness.py runs the same cases on the CPU with the f32 oracle in the kernel's place."""
import dataclasses

import numpy as np
import pytest

from tests import physics_harness as ph

pytestmark = pytest.mark.gpu

LAYOUTS = [pytest.param(k, id=v) for k, v in ph.LAYOUTS.items()]


def _engine(layout, n, robot="go2", cfg_class="GO2Cfg", **opt_overrides):
    built = ph.build(ph.PhysicsCase(robot, cfg_class, n=n, **opt_overrides), layout)
    return built, ph.EngineStepper(built, n)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_control_step_matches_oracle(layout, seed):
    ph.run_case(ph.CASES[f"plane-{seed}"], layout, ph.EngineStepper)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_free_flight_matches_oracle_tightly(layout):
    ph.run_case(ph.CASES["free-flight"], layout, ph.EngineStepper)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_static_stance_on_gpu(layout):
    """The kernel alone (no oracle): stiff stance settles with sum Fz = m g on the feet."""
    import torch
    from hcr_genesis_lr_cl_amd import config as cfgmod
    built, s = _engine(layout, 64, gains=(80.0, 1.0))
    eng = s.engine
    eng.buf["dof_pos"][:] = torch.tensor(cfgmod.default_dof_pos(built.cfg)).cuda()
    eng.buf["base_pos"][:, 2] = 0.335
    act = torch.zeros(64, 12, device="cuda")
    for _ in range(200):
        s.step(act)
    got = s.arrays(("link_contact_forces", "dof_vel"))
    f = got["link_contact_forces"].reshape(64, -1, 3)
    mg = built.model.total_mass * 9.81
    assert np.allclose(f[:, :, 2].sum(1), mg, rtol=0.02)
    assert np.all(f[:, [4, 8, 12, 16], 2].sum(1) > 0.98 * f[:, :, 2].sum(1))
    assert np.abs(got["dof_vel"]).max() < 0.05


@pytest.mark.parametrize("layout", LAYOUTS)
def test_extreme_actions_stay_finite(layout):
    import torch
    case = ph.PhysicsCase("go2", "GO2Cfg", seed=9)
    built = ph.build(case, layout)
    s = ph.EngineStepper(built, case.n)
    s.load(ph.initial_state(case, built)[0])
    act = torch.full((case.n, 12), 100.0, device="cuda")
    act[::2] *= -1
    for _ in range(50):
        s.step(act)
    for k, v in s.arrays(("dof_pos", "dof_vel", "base_pos", "base_quat", "link_contact_forces")).items():
        assert np.isfinite(v).all(), k


@pytest.mark.parametrize("robot,rough,layout", [("tron1_pf", False, 1), ("tron1_pf", False, 2), ("go2", True, 1), ("go2", True, 2),
                                                ("tron1_pf", True, 1), ("tron1_pf", True, 2), ("tron1_sf", False, 1), ("tron1_sf", False, 2)])
def test_one_control_step_matches_oracle_other_configs(robot, rough, layout):
    """The other robot / terrain combinations of the BASELINE configs."""
    ph.run_case(ph.CASES[f"{robot}-{'rough' if rough else 'plane'}"], layout, ph.EngineStepper)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("iters", [1, 3])
def test_other_sweep_counts_match_oracle(layout, iters):
    """The contact / limit sweep count is an option (cfg.hip.contact_iters): both kernels follow the CPU restatement at
    1 and 3 sweeps as well as at the default 2."""
    ph.run_case(ph.CASES[f"sweeps-{iters}"], layout, ph.EngineStepper)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("every", [2, 4])
def test_reused_contact_w_matches_oracle(layout, every):
    """LgSimOptions.contact_w_every: the feet's operational-space matrices are recomputed on sub-steps 0, k, 2k ... only (every foot,
    in contact or not) and reused in between -- both kernels follow the CPU restatement's statement of that rule, two control steps."""
    case = ph.CASES[f"reused-w-{every}"]
    ph.run_case(case, layout, ph.EngineStepper)
    # and the option does something: the default rule gives a (slightly) different trajectory
    built = ph.build(case, layout)
    st, actions = ph.initial_state(case, built)
    refs = [ph.OracleStepper(b, "f64") for b in (built, ph.build(dataclasses.replace(case, contact_w_every=1), layout))]
    for r in refs:
        r.load(st)
        for _ in range(case.steps):
            r.step(actions)
    assert np.abs(refs[1].st.arr["dof_vel"] - refs[0].st.arr["dof_vel"]).max() > 1e-4


@pytest.mark.parametrize("layout", [None, 1], ids=["auto", "leg-per-lane"])
def test_nonfinite_state_is_counted_and_ends_the_episode(layout, monkeypatch):
    """the non-finite guard re-seats the robot, and it is never silent -- LgBuffers.nonfinite_count goes up and the env
    terminates in the same step (reset_buf = 1, not a time-out), in the fused launch and in the split launches; in the one-launch
    leg-per-lane step (LG_SIM_LAYOUT=1) too, where the guard's flag reaches the MDP phases in a register."""
    import torch
    from hcr_genesis_lr_cl_amd.envs import make_env
    if layout is None:
        monkeypatch.delenv("LG_SIM_LAYOUT", raising=False)
    else:
        monkeypatch.setenv("LG_SIM_LAYOUT", str(layout))
    for task in ("go2", "tron1_pf_ee", "go2_cat", "tron1_sf"):      # tron1_sf: four joints per leg
        env, cfg = make_env(task, 64)
        env.reset()
        g = torch.Generator(device="cuda"); g.manual_seed(3)
        for _ in range(3):
            env.step(torch.randn(64, env.num_actions, generator=g, device="cuda"))
        eng = env._engine
        assert eng.nonfinite_count() == 0
        eng.buf["dof_vel"][5, 1] = float("nan")
        eng.buf["base_pos"][9, 2] = float("inf")
        out = env.step(torch.randn(64, env.num_actions, generator=g, device="cuda"))
        done, extras = out[-2], out[-1]
        assert eng.nonfinite_count() == 2, task
        assert bool(done[5]) and bool(done[9]) and not bool(extras["time_outs"][5]) and not bool(extras["time_outs"][9]), task
        for k in ("dof_pos", "dof_vel", "base_pos", "base_quat", "obs_buf", "rew_buf"):
            assert bool(torch.isfinite(eng.buf[k]).all()), (task, k)
        assert int(eng.buf["fail_buf"][5]) == 0 and int(eng.buf["episode_length_buf"][5]) == 0     # the reset went through
        env.step(torch.randn(64, env.num_actions, generator=g, device="cuda"))
        assert eng.nonfinite_count() == 2, task
        if layout == 1 and task != "go2_cat":
            assert "LG_PHASE_ALL" in eng.last_kernel(), eng.last_kernel()


@pytest.mark.parametrize("task", ["go2_ee", "tron1_pf_ee", "tron1_sf"])
def test_no_robot_is_thrown_by_the_contact_solver(task):
    """Regression (round 2): with friction ratios up to 1.7 the sliding branch of the foot contact could jam -- friction coupling
    cancelling the normal compliance, f_n = rn / (1 + kappa a_eff) with a_eff -> 0 -- and throw a robot (39 kN on one foot, 47 m/s,
    110 m high; 0.025 % of env-steps of a random go2_ee rollout, reproduced by the f64 CPU oracle on the same state).  The coupling
    is now limited to 3/4 of A_nn in both kernels and the oracle.  Same seeds as the rollout that showed it at step 3."""
    import torch
    from hcr_genesis_lr_cl_amd.envs import make_env
    n = 4096
    env, cfg = make_env(task, n)
    env.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    env.episode_length_buf = torch.randint(0, 1000, (n,), generator=g, device="cuda", dtype=torch.int32)
    s = env.simulator
    worst_v = worst_h = worst_f = 0.0
    for t in range(120):
        env.step(torch.randn(n, env.num_actions, generator=g, device="cuda"))
        worst_v = max(worst_v, float(s._base_lin_vel_w[:, 2].abs().max()))
        worst_h = max(worst_h, float((s.base_pos[:, 2] - s.env_origins[:, 2]).max()))
        worst_f = max(worst_f, float(s.link_contact_forces.norm(dim=-1).max()))
    assert worst_v < 6.0 and worst_h < 3.0 and worst_f < 6000.0, (worst_v, worst_h, worst_f)


# ---- first principles on the kernel itself (no oracle in the loop) ------------------------------------------------------------
# robot: (config, n, rng seed, pose jitter, mean-drift bound or None, worst-drift bound) at dt = 2 ms
MOMENTUM = {"go2": ("GO2Cfg", 64, 7, 0.2, None, 2e-2),                 # measured: 7e-3 / 5e-3 at worst, means 1.8e-3 / 1.0e-3
            "tron1_pf": ("TRON1PFCfg", 48, 9, 0.15, 6e-3, 8e-2),
            "tron1_sf": ("TRON1SFCfg", 48, 9, 0.15, 6e-3, 8e-2)}         # measured: 3.0e-3 / 1.2e-3 mean, 3.1e-2 worst


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("robot", list(MOMENTUM))
def test_zero_gravity_momentum_is_conserved_by_the_kernel(robot, layout):
    """Internal (actuator, joint-limit, damping) torques cannot change the total momentum.  Floating robots in zero gravity, random
    twists / joint rates / actions, 48 ms of simulated time: the linear and angular momentum (computed from the kernel's state by an
    independent numpy FK, physics_harness.momentum) drift only by the O(dt) global error of the first-order integrator -- small at
    dt = 2 ms and at least 2.5x smaller at dt = 0.5 ms (a force that did not belong there would not scale; measured: /4.01).  go2, the
    biped (two legs per env: eight envs per wave in the component layout) and the four-joint legs of TRON1-SF (fourth joint in the
    quad's spare lane)."""
    cfg_class, n, seed, jitter, mean_max, worst_max = MOMENTUM[robot]
    drift = []
    for dt, ctrl_steps in ((2e-3, 6), (5e-4, 24)):
        built, s = _engine(layout, n, robot, cfg_class, gravity_z=0.0, dt=dt)
        rng = np.random.default_rng(seed)
        st = ph.floating_state(built, n, 3.0, rng, jitter)
        s.load(st)
        m0 = [ph.momentum(built.model, st, e) for e in range(n)]
        act = rng.normal(size=(n, built.model.n_dof)).astype(np.float32)
        for _ in range(ctrl_steps):
            s.step(act)
        ph.read_back(s, st)
        assert np.abs(s.arrays([ph.FORCES])[ph.FORCES]).max() == 0.0
        dl, da = [], []
        for e in range(n):
            l1, a1, _ = ph.momentum(built.model, st, e)
            l0, a0, _ = m0[e]
            dl.append(np.linalg.norm(l1 - l0) / max(np.linalg.norm(l0), 1.0))
            da.append(np.linalg.norm(a1 - a0) / max(np.linalg.norm(a0), 1.0))
        drift.append((float(np.mean(dl)), float(np.mean(da)), float(np.max(dl)), float(np.max(da))))
    print(robot, layout, "momentum drift (mean lin, mean ang, max lin, max ang) at dt = 2 ms / 0.5 ms:", drift)
    if mean_max is not None:
        assert drift[0][0] < mean_max and drift[0][1] < mean_max, drift
    assert drift[0][2] < worst_max and drift[0][3] < worst_max, drift
    assert drift[1][0] < drift[0][0] / 2.5 + 2e-6 and drift[1][1] < drift[0][1] / 2.5 + 2e-6, drift


@pytest.mark.parametrize("layout", LAYOUTS)
def test_mirror_symmetry_of_the_kernel(layout):
    """Left/right mirrored state + mirrored actions give the mirrored next state (three control steps with contact), in both
    layouts.  The go2 URDF is not perfectly mirror symmetric (calf collision cylinders 0.012 vs 0.013 m), hence 2e-3."""
    from hcr_genesis_lr_cl_amd import config as cfgmod
    n = 32
    built, s = _engine(layout, n)
    st = ph.floating_state(built, n, 0.36)
    rng = np.random.default_rng(3)
    perm = np.array([3, 4, 5, 0, 1, 2, 9, 10, 11, 6, 7, 8]); sgn = np.array([-1, 1, 1] * 4, np.float32)
    acts = np.zeros((n, 12), np.float32)
    for e in range(0, n, 2):
        q = cfgmod.default_dof_pos(built.cfg) + rng.uniform(-0.2, 0.2, 12).astype(np.float32)
        qd = rng.normal(size=12).astype(np.float32)
        a = rng.normal(size=12).astype(np.float32)
        v, w = rng.normal(size=3) * 0.3, rng.normal(size=3) * 0.3
        st.arr["dof_pos"][e], st.arr["dof_vel"][e] = q, qd
        st.arr["dof_pos"][e + 1], st.arr["dof_vel"][e + 1] = q[perm] * sgn, qd[perm] * sgn
        st.arr["base_lin_vel_w"][e] = v; st.arr["base_lin_vel_w"][e + 1] = v * [1, -1, 1]
        st.arr["base_ang_vel_w"][e] = w; st.arr["base_ang_vel_w"][e + 1] = w * [-1, 1, -1]
        acts[e], acts[e + 1] = a, a[perm] * sgn
    s.load(st)
    for _ in range(3):
        s.step(acts)
    got = s.arrays(("dof_pos", "base_pos", "base_lin_vel_w"))
    np.testing.assert_allclose(got["dof_pos"][1::2], got["dof_pos"][0::2][:, perm] * sgn, atol=2e-3)
    np.testing.assert_allclose(got["base_pos"][1::2] * [1, -1, 1], got["base_pos"][0::2], atol=1e-3)
    np.testing.assert_allclose(got["base_lin_vel_w"][1::2] * [1, -1, 1], got["base_lin_vel_w"][0::2], atol=2e-2)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_free_fall_closed_form_on_the_kernel(layout):
    """No contact, kp = kd = 0: the base follows the semi-implicit Euler closed form z_n = z0 - g dt^2 n (n + 1) / 2 and a
    multibody falling under gravity alone has no relative acceleration (joints and attitude stay put)."""
    n = 8
    built, s = _engine(layout, n)
    st = ph.floating_state(built, n, 50.0)
    st.arr["dof_vel"][:] = 0
    st.arr["kp_scale"][:] = 0; st.arr["kd_scale"][:] = 0          # PD gains off through their per-env multipliers
    s.load(st)
    act = np.zeros((n, 12), np.float32)
    n_ctrl = 10
    for _ in range(n_ctrl):
        s.step(act)
    got = s.arrays(("base_pos", "base_lin_vel_w", "dof_vel", "base_ang_vel_w", "base_quat"))
    k = n_ctrl * 4
    z = 50.0 - 9.81 * 0.005 ** 2 * k * (k + 1) / 2
    np.testing.assert_allclose(got["base_pos"][:, 2], z, atol=5e-5)            # f32 at z = 50: 4e-6 per ulp
    np.testing.assert_allclose(got["base_lin_vel_w"][:, 2], -9.81 * 0.005 * k, atol=2e-5)
    np.testing.assert_allclose(got["dof_vel"], 0, atol=2e-4)
    np.testing.assert_allclose(got["base_ang_vel_w"], 0, atol=2e-4)

"""GPU parity, MDP phases: the HIP kernel (PRE|POST|RESET launches through the C ABI, physics
read-backs and uniform draws injected) against (a) the golden vectors produced by the
reference's own GO2 class and (b) the numpy oracle at 4096 envs on random inputs.
Float tolerance 1e-5 abs/rel (f32 sums in a different association order + fused multiply-add);
integer / boolean outputs exact."""
import os

import numpy as np
import pytest

from tests.test_mdp_oracle import GOLD, replay, check_against_fixture
from oracle import mdp_oracle as mo

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


SIM_KEYS = ("base_pos", "base_quat", "base_lin_vel_w", "base_ang_vel_w", "dof_pos", "dof_vel", "torques",
            "link_contact_forces", "feet_pos", "feet_vel", "last_dof_vel", "last_feet_vel")


def make_engine(N, env_origins=None, cfg_cls=None):
    import torch
    from hcr_genesis_lr_cl_amd import builders
    from hcr_genesis_lr_cl_amd.config import GO2Cfg
    from hcr_genesis_lr_cl_amd.engine import Engine
    from hcr_genesis_lr_cl_amd.model_compiler import load_model
    cfg = (cfg_cls or GO2Cfg)()
    model = load_model(cfg.asset.name)
    desc, opts, task = builders.make_model_desc(model, cfg), builders.make_sim_options(model, cfg), builders.make_task_cfg(model, cfg)
    eng = Engine(model, desc, opts, task, N, "cuda:0", inject_rand=True)
    drop_unused_joint_dr(eng, task)
    cr = cfg.commands.ranges
    eng.buf["command_ranges"][:8] = torch.tensor(list(cr.lin_vel_x) + list(cr.lin_vel_y) + list(cr.ang_vel_yaw) + list(cr.heading))
    if env_origins is not None:
        eng.buf["env_origins"].copy_(torch.from_numpy(env_origins))
    return eng, model, cfg, task


def drop_unused_joint_dr(eng, task):
    """What HipSimulator does for a task without per-env joint parameters (simulator.py:310-316): the three (N, 1) arrays are unbound, the
    kernel takes armature / frictionloss / damping from the model -- and the task fits its profile (lg_host.hip flat_profile ...)."""
    if not int(task.dr_joint_on):
        for k in ("joint_armature", "joint_friction", "joint_damping"):
            eng.buf.pop(k)
        eng.bind()


def put(eng, name, arr):
    import torch
    t = eng.buf[name]
    t.copy_(torch.from_numpy(np.ascontiguousarray(arr)).reshape(t.shape).to(t.dtype))


def get(eng, name):
    return eng.buf[name].detach().cpu().numpy()


def load_sim(eng, sim):
    for k in SIM_KEYS:
        put(eng, k, sim[k])
    q = sim["base_quat"]
    put(eng, "base_lin_vel", mo.quat_rotate_inverse(q, sim["base_lin_vel_w"]))
    put(eng, "base_ang_vel", mo.quat_rotate_inverse(q, sim["base_ang_vel_w"]))
    put(eng, "projected_gravity", mo.quat_rotate_inverse(q, np.tile(np.array([0, 0, -1], np.float32), (len(q), 1))))
    put(eng, "base_euler", mo.get_euler_xyz(q))


class KernelStepper:
    def __init__(self, fx, N):
        import torch
        self.eng, self.model, self.cfg, self.task = make_engine(N, fx["init_env_origins"])
        put(self.eng, "episode_length_buf", fx["init_episode_length_buf"])
        put(self.eng, "commands", fx["init_commands"])
        self.names = [str(n) for n in fx["reward_names"]]
        self.cmd_range_x = [-0.5, 0.5]

    def step(self, t, sim, actions, R, counter, override):
        import torch
        from hcr_genesis_lr_cl_amd import abi
        eng = self.eng
        k = abi.REWARD_ID["tracking_lin_vel"]
        if override:
            eng.buf["episode_sums"][k].fill_(override)
            eng.buf["episode_length_buf"][:4] = 1000
        load_sim(eng, sim)
        put(eng, "rand_in", R)
        act = torch.from_numpy(actions).cuda()
        if counter % 1000 == 0:       # command-curriculum gate, same split as envs/legged_robot.py
            eng.step(abi.PHASE_PRE | abi.PHASE_POST, act, counter)
            ids = eng.buf["reset_buf"].nonzero().flatten()
            if len(ids):
                mean = torch.mean(eng.buf["episode_sums"][k][ids]) / 1000.0
                if mean > 0.8 * (1.0 * 0.02):
                    self.cmd_range_x = [max(self.cmd_range_x[0] - 0.5, -1.0), min(self.cmd_range_x[1] + 0.5, 1.0)]
                    eng.buf["command_ranges"][0] = self.cmd_range_x[0]
                    eng.buf["command_ranges"][1] = self.cmd_range_x[1]
            eng.step(abi.PHASE_RESET, None, counter)
        else:
            eng.step(abi.PHASE_PRE | abi.PHASE_POST | abi.PHASE_RESET, act, counter)
        torch.cuda.synchronize()
        es = get(eng, "episode_sums")
        return dict(obs=get(eng, "obs_buf"), rew=get(eng, "rew_buf"), reset=get(eng, "reset_buf"), time_out=get(eng, "time_out_buf"),
                    commands=get(eng, "commands"), ep_len=get(eng, "episode_length_buf"), fail_buf=get(eng, "fail_buf"),
                    feet_air_time=get(eng, "feet_air_time"), last_contacts=get(eng, "last_contacts"),
                    episode_sums=np.stack([es[abi.REWARD_ID[n]] for n in self.names]),
                    act_hist=np.stack([get(eng, "actions"), get(eng, "last_actions"), get(eng, "llast_actions")]),
                    sim_dof_pos=get(eng, "dof_pos"), sim_dof_vel=get(eng, "dof_vel"), sim_base_pos=get(eng, "base_pos"),
                    sim_base_quat=get(eng, "base_quat"), sim_base_lin_vel_w=get(eng, "base_lin_vel_w"),
                    sim_projected_gravity=get(eng, "projected_gravity"), sim_base_lin_vel=get(eng, "base_lin_vel"),
                    dr=np.concatenate([get(eng, "friction_values"), get(eng, "added_base_mass"), get(eng, "base_com_bias"),
                                       get(eng, "rand_push_vels")[:, :2]], 1),
                    cmd_range_x=np.array(self.cmd_range_x, np.float32))


def test_kernel_reproduces_reference_go2_golden_vectors(tail):
    replay(KernelStepper, lambda t, fx, out: check_against_fixture(t, fx, out, rtol=1e-5, atol=1e-5))


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
class WtwKernelStepper:
    def __init__(self, fx, N):
        import torch
        from hcr_genesis_lr_cl_amd.config import GO2WTWCfg
        self.eng, self.model, self.cfg, self.task = make_engine(N, fx["init_env_origins"], GO2WTWCfg)
        eng = self.eng
        put(eng, "episode_length_buf", fx["init_episode_length_buf"])
        put(eng, "commands", fx["init_commands"])
        eng.buf["command_ranges"][8:17] = torch.from_numpy(fx["init_behavior_ranges"]).cuda()
        ts = np.zeros((N, 22), np.float32)
        ts[:, 0:1], ts[:, 1:2], ts[:, 2:3] = fx["init_gait_time"], fx["init_phi"], fx["init_gait_period"]
        ts[:, 3], ts[:, 4], ts[:, 5] = 0.27, 0.04, 0.0          # mid / min initial targets (go2_wtw.py:337-346)
        ts[:, 6:10] = fx["init_theta"]
        put(eng, "task_state", ts)
        eng.buf["friction_values"].fill_(0.0); eng.buf["added_base_mass"].fill_(1.0)    # the fake simulator's initial values
        self.names = [str(n) for n in fx["reward_names"]]

    def step(self, t, sim, actions, R, counter, override):
        import torch
        from hcr_genesis_lr_cl_amd import abi
        eng = self.eng
        load_sim(eng, sim)
        put(eng, "rand_in", R)
        eng.step(abi.PHASE_PRE | abi.PHASE_POST | abi.PHASE_RESET, torch.from_numpy(actions).cuda(), counter)
        torch.cuda.synchronize()
        es = get(eng, "episode_sums")
        return dict(obs=get(eng, "obs_buf"), priv=get(eng, "priv_obs_buf"), rew=get(eng, "rew_buf"), reset=get(eng, "reset_buf"),
                    time_out=get(eng, "time_out_buf"), commands=get(eng, "commands"), ep_len=get(eng, "episode_length_buf"),
                    fail_buf=get(eng, "fail_buf"), episode_sums=np.stack([es[abi.REWARD_ID[n]] for n in self.names]),
                    act_hist=np.stack([get(eng, "actions"), get(eng, "last_actions"), get(eng, "llast_actions")]),
                    sim_dof_pos=get(eng, "dof_pos"), sim_base_pos=get(eng, "base_pos"), sim_base_lin_vel_w=get(eng, "base_lin_vel_w"),
                    dr_pd=np.concatenate([get(eng, "kp_scale"), get(eng, "kd_scale")], 1), task_state=get(eng, "task_state"))


def test_kernel_reproduces_reference_go2_wtw_golden_vectors(tail):
    """Env 0 is excluded: the reference couples it to the whole batch through two index-flatten bugs
    (go2_wtw.py:33-34, 455-462) which the kernel does not reproduce (envs/go2_wtw.py docstring)."""
    from tests.test_mdp_oracle import GOLD_WTW
    from tests.test_mdp_oracle import check_wtw
    replay(WtwKernelStepper, lambda t, fx, out: check_wtw(t, fx, out, rtol=1e-5, atol=1e-5, skip_env0=True), GOLD_WTW)


# ------------------------------- every task against the oracle on synthetic batches ---------------------------------------
def synth_kernel_stepper(task):
    if task in ("go2_ts", "go2_cts", "go2_dreamwaq", "go2_cat"):
        return type("KStepper_" + task, (EEKernelStepper,), {"head": task})
    return {"go2": KernelStepper, "go2_wtw": WtwKernelStepper, "go2_ee": EEKernelStepper, "tron1_pf_ee": Tron1KernelStepper,
            "tron1_pf": PFKernelStepper, "tron1_sf": SFKernelStepper}[task]


def _synth_params():
    """(task, tail, history mode): fused-profile only where the task has an INJ profile tail and only with the sliding window
    (the component-layout tails hard-wire it); go2_cat, tron1_pf and tron1_sf are split only."""
    from tests.synthetic_mdp import TASKS, INJ_TAIL
    modes = (("64", "history-window"), ("1", "history-window-min-slack"), ("0", "history-shift"))
    return [pytest.param(task, tail, m, id=f"{task}-{tail}-{mid}") for task in TASKS for tail in ("split", "fused-profile")
            for m, mid in modes if tail == "split" or (task in INJ_TAIL and m != "0")]


@pytest.mark.parametrize("N", [4096, 4093])
@pytest.mark.parametrize("task,tail,history_mode", _synth_params(), indirect=["tail", "history_mode"])
def test_kernel_matches_oracle_on_synthetic_batches(task, N, tail):
    """Every task's MDP instantiations against the oracle on a synthetic batch (tests/synthetic_mdp.py): 4096 envs, and 4093 for a
    partly filled last wave / workgroup / PROF 6 group of 8 envs; long enough for two compactions of the smallest-slack history
    window; inputs that cross every decision of the MDP phases with a margin.  Expected values are the oracle's, recorded once
    per batch; tolerances of sm.synth_check (the golden replays' kernel tolerances)."""
    from tests import synthetic_mdp as sm
    fx = sm.recorded(task, N)
    sm.replay(task, fx, synth_kernel_stepper(task), sm.synth_check(task))


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
class EEKernelStepper:
    head = "go2_ee"

    def __init__(self, fx, N):
        import torch
        from hcr_genesis_lr_cl_amd import builders
        from hcr_genesis_lr_cl_amd.engine import Engine
        from hcr_genesis_lr_cl_amd.model_compiler import load_model
        from tests.test_mdp_oracle import ee_terrain
        cfg, terrain = ee_terrain(fx, self.head)
        self.cfg, self.terrain = cfg, terrain
        model = load_model("go2")
        desc, opts, task = builders.make_model_desc(model, cfg), builders.make_sim_options(model, cfg, terrain), builders.make_task_cfg(model, cfg)
        eng = self.eng = Engine(model, desc, opts, task, N, "cuda:0", inject_rand=True)
        drop_unused_joint_dr(eng, task)
        eng.set_terrain(terrain.height_field_raw, terrain.env_origins, fx["init_height_points"])
        cr = cfg.commands.ranges
        eng.buf["command_ranges"][:8] = torch.tensor(list(cr.lin_vel_x) + list(cr.lin_vel_y) + list(cr.ang_vel_yaw) + list(cr.heading))
        put(eng, "env_origins", fx["init_env_origins"]); put(eng, "episode_length_buf", fx["init_episode_length_buf"])
        put(eng, "commands", fx["init_commands"])
        put(eng, "terrain_levels", fx["init_terrain_levels"]); put(eng, "terrain_types", fx["init_terrain_types"])
        eng.buf["friction_values"].fill_(0.0); eng.buf["added_base_mass"].fill_(1.0)
        self.names = [str(n) for n in fx["reward_names"]]
        self.fx = fx

    def step(self, t, sim, actions, R, counter, override):
        import torch
        from hcr_genesis_lr_cl_amd import abi
        eng, fx = self.eng, self.fx
        load_sim(eng, sim)
        # terrain read-backs of the SIM phase (checked separately against the numpy sampler): injected
        put(eng, "measured_heights", fx["measured_heights"][t]); put(eng, "height_around_feet", fx["height_around_feet"][t])
        put(eng, "normal_vector_around_feet", fx["normals"][t])
        put(eng, "rand_in", R)
        if "cstr_prob" in eng.buf:       # go2_cat: the job-wide "some env moves a joint faster than 4 rad/s" flag (envs/go2_ts.py Go2CaT._any_fast)
            eng.buf["command_ranges"][abi.CR_ANY_FAST + (counter & 1)] = float(np.any(np.abs(sim["dof_vel"]) > 4.0))   # what the SIM phase raises
        eng.step(abi.PHASE_PRE | abi.PHASE_POST | abi.PHASE_RESET, torch.from_numpy(actions).cuda(), counter)
        torch.cuda.synchronize()
        es = get(eng, "episode_sums")
        lab = get(eng, "labels_buf")
        from tests.test_mdp_oracle import HEADS
        W, cols = HEADS[self.head][1], HEADS[self.head][2]
        return dict(feat_new=get(eng, "obs_buf")[:, -45:], priv_new=get(eng, "priv_obs_buf")[:, -W:], labels=lab, rew=get(eng, "rew_buf"),
                    reset=get(eng, "reset_buf"), time_out=get(eng, "time_out_buf"), commands=get(eng, "commands"),
                    ep_len=get(eng, "episode_length_buf"), fail_buf=get(eng, "fail_buf"), feet_air_time=get(eng, "feet_air_time"),
                    episode_sums=np.stack([es[abi.REWARD_ID[n]] for n in self.names]), sim_dof_pos=get(eng, "dof_pos"),
                    sim_base_pos=get(eng, "base_pos"), terrain_levels=get(eng, "terrain_levels"), env_origins=get(eng, "env_origins"),
                    measured_heights=fx["measured_heights"][t], height_around_feet=fx["height_around_feet"][t], normals=fx["normals"][t],
                    contact_states=get(eng, "priv_obs_buf")[:, -W:][:, cols], feat_full=get(eng, "obs_buf"), priv_full=get(eng, "priv_obs_buf"),
                    obs=get(eng, "obs_buf")[:, -45:], cstr_prob=get(eng, "cstr_prob") if "cstr_prob" in eng.buf else None,
                    cstr_sums=get(eng, "cstr_sums") if "cstr_sums" in eng.buf else None)


def test_kernel_reproduces_reference_go2_ee_golden_vectors(tail):
    from tests.test_mdp_oracle import replay_ee, check_ee
    replay_ee(EEKernelStepper, lambda t, fx, out: check_ee(t, fx, out, rtol=1e-5, atol=5e-5))


@pytest.mark.parametrize("head", ["go2_ts", "go2_cts", "go2_dreamwaq", "go2_cat"])
def test_kernel_reproduces_reference_head_golden_vectors(head, tail):
    """the other Go2-rough heads.  Golden vectors from the reference's own Go2TS / Go2CTS / Go2Dreamwaq classes as
    configured (tests/golden/gen_mdp_fixtures.py gen_head): actor frame, newest frames of the 20-deep actor history and the
    5-deep critic stack (full stacks at the last step), the single-frame auxiliary output, rewards, resets, curricula."""
    from tests.test_mdp_oracle import replay_ee, check_head, head_gold
    if head == "go2_cat" and tail == "fused-profile":
        pytest.skip("go2_cat has no component-layout tail: its MDP phases are the leg-per-lane launch in the product too")
    stepper = type("KStepper_" + head, (EEKernelStepper,), {"head": head})
    replay_ee(stepper, lambda t, fx, out: check_head(t, fx, out, rtol=1e-5, atol=5e-5), head_gold(head))


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
class Tron1KernelStepper:
    def __init__(self, fx, N):
        import torch
        from hcr_genesis_lr_cl_amd import builders
        from hcr_genesis_lr_cl_amd.engine import Engine
        from hcr_genesis_lr_cl_amd.model_compiler import load_model
        from tests.test_mdp_oracle import tron1_terrain
        cfg, terrain = tron1_terrain(fx)
        model = load_model("tron1_pf")
        desc, opts, task = builders.make_model_desc(model, cfg), builders.make_sim_options(model, cfg, terrain), builders.make_task_cfg(model, cfg)
        eng = self.eng = Engine(model, desc, opts, task, N, "cuda:0", inject_rand=True)
        drop_unused_joint_dr(eng, task)
        eng.set_terrain(terrain.height_field_raw, terrain.env_origins, fx["init_height_points"])
        cr = cfg.commands.ranges
        eng.buf["command_ranges"][:8] = torch.tensor(list(cr.lin_vel_x) + list(cr.lin_vel_y) + list(cr.ang_vel_yaw) + list(cr.heading))
        for k in ("env_origins", "episode_length_buf", "commands", "terrain_levels", "terrain_types"):
            put(eng, k, fx["init_" + k])
        ts = np.zeros((N, 12), np.float32)
        ts[:, 0:1], ts[:, 1:2], ts[:, 2], ts[:, 4:6] = fx["init_gait_time"], fx["init_phi"], 0.5, fx["init_theta"]
        put(eng, "task_state", ts)
        eng.buf["friction_values"].fill_(0.0); eng.buf["added_base_mass"].fill_(1.0)
        self.names = [str(n) for n in fx["reward_names"]]
        self.fx = fx

    def step(self, t, sim, actions, R, counter, override):
        import torch
        from hcr_genesis_lr_cl_amd import abi
        eng, fx = self.eng, self.fx
        load_sim(eng, sim)
        put(eng, "measured_heights", fx["measured_heights"][t]); put(eng, "height_around_feet", fx["height_around_feet"][t])
        put(eng, "normal_vector_around_feet", fx["normals"][t])
        put(eng, "rand_in", R)
        eng.step(abi.PHASE_PRE | abi.PHASE_POST | abi.PHASE_RESET, torch.from_numpy(actions).cuda(), counter)
        torch.cuda.synchronize()
        es, tsb = get(eng, "episode_sums"), get(eng, "task_state")
        return dict(feat_new=get(eng, "obs_buf")[:, -31:], priv_new=get(eng, "priv_obs_buf")[:, -134:], labels=get(eng, "labels_buf"),
                    rew=get(eng, "rew_buf"), reset=get(eng, "reset_buf"), time_out=get(eng, "time_out_buf"), commands=get(eng, "commands"),
                    ep_len=get(eng, "episode_length_buf"), fail_buf=get(eng, "fail_buf"),
                    episode_sums=np.stack([es[abi.REWARD_ID[n]] for n in self.names]),
                    act_hist=np.stack([get(eng, "actions"), get(eng, "last_actions"), get(eng, "llast_actions")]),
                    sim_dof_pos=get(eng, "dof_pos"), sim_base_pos=get(eng, "base_pos"), sim_base_quat=get(eng, "base_quat"),
                    terrain_levels=get(eng, "terrain_levels"), env_origins=get(eng, "env_origins"),
                    measured_heights=fx["measured_heights"][t], height_around_feet=fx["height_around_feet"][t], normals=fx["normals"][t],
                    dr_joint=np.concatenate([get(eng, "joint_armature"), get(eng, "joint_friction"), get(eng, "joint_damping")], 1),
                    task_state=np.concatenate([tsb[:, 0:2], tsb[:, 4:12]], 1), feat_full=get(eng, "obs_buf"), priv_full=get(eng, "priv_obs_buf"))


def test_kernel_reproduces_reference_tron1_pf_ee_golden_vectors(tail):
    """Env 0 excluded for the same reason as in the wtw test (reference index-flatten bugs on the gait clock / indicator)."""
    from tests.test_mdp_oracle import GOLD_TRON1, replay_rough, check_tron1
    replay_rough(GOLD_TRON1, Tron1KernelStepper, lambda t, fx, out: check_tron1(t, fx, out, rtol=1e-5, atol=5e-5, skip_env0=True))


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
class PFKernelStepper:
    def __init__(self, fx, N):
        from hcr_genesis_lr_cl_amd.config import TRON1PFCfg
        self.eng, self.model, self.cfg, self.task = make_engine(N, fx["init_env_origins"], TRON1PFCfg)
        eng = self.eng
        put(eng, "episode_length_buf", fx["init_episode_length_buf"])
        put(eng, "commands", fx["init_commands"])
        eng.buf["friction_values"].fill_(0.0); eng.buf["added_base_mass"].fill_(1.0)    # the fake simulator's initial values
        self.names = [str(n) for n in fx["reward_names"]]

    def step(self, t, sim, actions, R, counter, override):
        import torch
        from hcr_genesis_lr_cl_amd import abi
        eng = self.eng
        load_sim(eng, sim)
        put(eng, "rand_in", R)
        eng.step(abi.PHASE_PRE | abi.PHASE_POST | abi.PHASE_RESET, torch.from_numpy(actions).cuda(), counter)
        torch.cuda.synchronize()
        es = get(eng, "episode_sums")
        return dict(obs=get(eng, "obs_buf"), priv=get(eng, "priv_obs_buf"), rew=get(eng, "rew_buf"), reset=get(eng, "reset_buf"),
                    time_out=get(eng, "time_out_buf"), commands=get(eng, "commands"), ep_len=get(eng, "episode_length_buf"),
                    fail_buf=get(eng, "fail_buf"), feet_air_time=get(eng, "feet_air_time"),
                    episode_sums=np.stack([es[abi.REWARD_ID[n]] for n in self.names]),
                    act_hist=np.stack([get(eng, "actions"), get(eng, "last_actions"), get(eng, "llast_actions")]),
                    sim_dof_pos=get(eng, "dof_pos"), sim_base_pos=get(eng, "base_pos"), sim_base_lin_vel_w=get(eng, "base_lin_vel_w"),
                    dr=np.concatenate([get(eng, "friction_values"), get(eng, "added_base_mass"), get(eng, "base_com_bias"),
                                       get(eng, "rand_push_vels")[:, :2]], 1))


def test_kernel_reproduces_reference_tron1_pf_golden_vectors():
    """TRON1PF on the plane, golden vectors from the reference's own class (gen_mdp_fixtures.py gen_tron1_pf)."""
    from tests.test_mdp_oracle import GOLD_PF, check_pf
    replay(PFKernelStepper, lambda t, fx, out: check_pf(t, fx, out, rtol=1e-5, atol=5e-5), GOLD_PF)


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
class SFKernelStepper:
    def __init__(self, fx, N):
        from tests.test_mdp_oracle import sf_cfg
        self.eng, self.model, self.cfg, self.task = make_engine(N, fx["init_env_origins"], sf_cfg)
        eng = self.eng
        put(eng, "episode_length_buf", fx["init_episode_length_buf"])
        put(eng, "commands", fx["init_commands"])
        eng.buf["friction_values"].fill_(0.0); eng.buf["added_base_mass"].fill_(1.0)    # the fake simulator's initial values
        for k in ("joint_armature", "joint_friction", "joint_damping"):
            eng.buf[k].fill_(0.0)
        self.names = [str(n) for n in fx["reward_names"]]

    def step(self, t, sim, actions, R, counter, override):
        import torch
        from hcr_genesis_lr_cl_amd import abi
        eng = self.eng
        sim.pop("foot_quat", None)     # the kernel derives the foot orientation from base_quat and dof_pos
        load_sim(eng, sim)
        put(eng, "rand_in", R)
        eng.step(abi.PHASE_PRE | abi.PHASE_POST | abi.PHASE_RESET, torch.from_numpy(actions).cuda(), counter)
        torch.cuda.synchronize()
        es = get(eng, "episode_sums")
        return dict(obs=get(eng, "obs_buf"), priv=get(eng, "priv_obs_buf"), rew=get(eng, "rew_buf"), reset=get(eng, "reset_buf"),
                    time_out=get(eng, "time_out_buf"), commands=get(eng, "commands"), ep_len=get(eng, "episode_length_buf"),
                    fail_buf=get(eng, "fail_buf"), feet_air_time=get(eng, "feet_air_time"),
                    episode_sums=np.stack([es[abi.reward_id(n, 4)] for n in self.names]),
                    act_hist=np.stack([get(eng, "actions"), get(eng, "last_actions"), get(eng, "llast_actions")]),
                    sim_dof_pos=get(eng, "dof_pos"), sim_base_pos=get(eng, "base_pos"), sim_base_quat=get(eng, "base_quat"),
                    sim_base_lin_vel_w=get(eng, "base_lin_vel_w"),
                    dr=np.concatenate([get(eng, "friction_values"), get(eng, "added_base_mass"), get(eng, "base_com_bias"),
                                       get(eng, "rand_push_vels")[:, :2]], 1),
                    dr_pd=np.concatenate([get(eng, "kp_scale"), get(eng, "kd_scale")], 1),
                    dr_joint=np.concatenate([get(eng, "joint_armature"), get(eng, "joint_friction"), get(eng, "joint_damping")], 1))


def test_kernel_reproduces_reference_tron1_sf_golden_vectors():
    """TRON1SF, golden vectors from the reference's own class (gen_mdp_fixtures.py gen_tron1_sf): four-joint legs in the
    MDP phases, the sole-foot reward terms, the sit-pose coin, the 10-frame stacks with the kp / kd blocks in the critic frame."""
    from tests.test_mdp_oracle import GOLD_SF, check_sf
    replay(SFKernelStepper, lambda t, fx, out: check_sf(t, fx, out, rtol=1e-5, atol=5e-5), GOLD_SF)


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

"""One harness for every MDP replay: a fixture (golden, tests/golden/*_mdp.npz, or synthetic, tests/synthetic_mdp.py) stepped through
the numpy oracle (oracle/mdp_oracle.py) or the HIP kernel's MDP phases, each step's outputs compared with the fixture's.

TASKS holds what differs between the tasks, one TaskSpec each: configuration, terrain, gait layout, the outputs compared and the
kernel tolerances.  Both steppers expose the post-step state under the engine's buffer names (`stepper[name]`), so that outputs()
forms the compared quantities once for both.  CPU-safe: torch and the engine are imported inside the functions that need them."""
import dataclasses
import os

import numpy as np

from hcr_genesis_lr_cl_amd import abi

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

# outputs that carry the yaw command, an atan2f of the forward vector on the device
YAW_KEYS = ("obs", "priv", "commands")
# the physics read-backs the MDP phases start from (engine buffer names)
SIM_KEYS = ("base_pos", "base_quat", "base_lin_vel_w", "base_ang_vel_w", "dof_pos", "dof_vel", "torques", "link_contact_forces",
            "feet_pos", "feet_vel", "last_dof_vel", "last_feet_vel")
# the SIM phase's terrain read-backs: fixture / oracle name -> engine buffer
TERRAIN_READ_BACKS = {"measured_heights": "measured_heights", "height_around_feet": "height_around_feet",
                      "normals": "normal_vector_around_feet"}
ORACLE_TOL = dict(rtol=2e-6, atol=2e-6)      # float sums may associate differently than torch


@dataclasses.dataclass(frozen=True)
class TaskSpec:
    name: str
    cfg_class: str                    # hcr_genesis_lr_cl_amd.config class; the model is its asset
    exact: tuple                      # compared as int64
    floats: tuple                     # compared with assert_allclose
    rough: bool = False               # Terrain from the fixture's terrain_seed; levels, types and origins; terrain read-backs
    gait: str = None                  # None, "wtw" or "biped": the task_state layout (TASK_STATE)
    go2: bool = False                 # go2's generator: esum_override, the command-curriculum split at counter % 1000 == 0, the
    #                                   oracle's own initial DR values, dr compared on the rows a reset drew
    inj_tail: bool = False            # has an INJ instantiation of its profile's component-layout tail (lg_quad.h)
    stacks: bool = False              # last step: the full stacks feat_full / priv_full against feat_last / priv_last
    cstr: bool = False                # CaT: cstr_prob / cstr_sums exact
    frames: tuple = None              # rough: (actor frame width, critic frame width, contact-state columns of the critic frame)
    labels: tuple = ()                # (key, what the failure message calls it) where that is not the key
    kernel_atol: float = 5e-5         # kernel vs golden and synthetic: rtol 1e-5 and this atol
    kernel_skip_env0: bool = False    # the reference's index-flatten bugs on the gait clock / indicator (go2_wtw.py:33-34, 455-462),
    #                                   reproduced by the oracle, not by the kernel (envs/go2_wtw.py docstring)
    reward_scales: tuple = ()         # (reward term, scale) set on the config as the golden generator did

    @property
    def gold(self):
        return os.path.join(GOLDEN, f"{self.name}_mdp.npz")

    def cfg(self):
        from hcr_genesis_lr_cl_amd import config as cfgmod
        cfg = getattr(cfgmod, self.cfg_class)()
        for k, v in self.reward_scales:
            setattr(cfg.rewards.scales, k, v)
        return cfg

    def golden_tol(self):
        """The kernel against the golden vectors."""
        return dict(rtol=1e-5, atol=self.kernel_atol, skip_env0=self.kernel_skip_env0)

    def synth_tol(self):
        """The kernel against the oracle on a synthetic batch: the golden tolerances, with 5e-5 on the yaw keys where atol is tighter."""
        return dict(self.golden_tol(), atol_yaw=5e-5 if self.kernel_atol < 5e-5 else None)


_ROUGH_EXACT = ("reset", "time_out", "ep_len", "fail_buf", "terrain_levels")
_GO2_ROUGH_FLOATS = ("measured_heights", "height_around_feet", "normals", "contact_states", "feat_new", "priv_new", "labels", "rew",
                     "commands", "feet_air_time", "episode_sums", "sim_dof_pos", "sim_base_pos", "env_origins")
_PLANE_EXACT = ("reset", "time_out", "ep_len", "fail_buf")
_PF_FLOATS = ("obs", "priv", "rew", "commands", "feet_air_time", "episode_sums", "act_hist", "sim_dof_pos", "sim_base_pos",
              "sim_base_lin_vel_w", "dr")


def _go2_head(name, cfg_class, **kw):
    """go2_ts / go2_cts / go2_dreamwaq / go2_cat: go2_ee's physics and rewards, other packaging; 17 contact-state links as configured
    (common_cfgs.py:100-101), critic frames 177 wide."""
    return TaskSpec(name, cfg_class, _ROUGH_EXACT, _GO2_ROUGH_FLOATS + ("obs",), rough=True, stacks=True,
                    frames=(45, 177, slice(79, 96)), labels=(("obs", "clipped actor frame"),), **kw)


TASKS = {s.name: s for s in (
    TaskSpec("go2", "GO2Cfg", ("reset", "time_out", "ep_len", "fail_buf", "last_contacts"),
             ("obs", "rew", "commands", "feet_air_time", "episode_sums", "act_hist", "sim_dof_pos", "sim_dof_vel", "sim_base_pos",
              "sim_base_quat", "sim_base_lin_vel_w", "sim_projected_gravity", "sim_base_lin_vel", "cmd_range_x"),
             go2=True, inj_tail=True, kernel_atol=1e-5),
    TaskSpec("go2_wtw", "GO2WTWCfg", _PLANE_EXACT,
             ("obs", "priv", "rew", "commands", "episode_sums", "act_hist", "sim_dof_pos", "sim_base_pos", "sim_base_lin_vel_w", "dr_pd",
              "task_state"),
             gait="wtw", inj_tail=True, kernel_atol=1e-5, kernel_skip_env0=True),
    TaskSpec("go2_ee", "GO2EECfg", _ROUGH_EXACT, _GO2_ROUGH_FLOATS, rough=True, inj_tail=True, stacks=True,
             frames=(45, 174, slice(76, 93))),
    _go2_head("go2_ts", "GO2TSCfg", inj_tail=True),
    _go2_head("go2_cts", "GO2CTSCfg", inj_tail=True),
    _go2_head("go2_dreamwaq", "GO2DreamwaqCfg", inj_tail=True),
    _go2_head("go2_cat", "GO2CaTCfg", cstr=True),
    TaskSpec("tron1_pf", "TRON1PFCfg", _PLANE_EXACT, _PF_FLOATS),
    TaskSpec("tron1_pf_ee", "TRON1PFEECfg", _ROUGH_EXACT,
             ("measured_heights", "height_around_feet", "normals", "feat_new", "priv_new", "labels", "rew", "commands", "episode_sums",
              "act_hist", "sim_dof_pos", "sim_base_pos", "sim_base_quat", "env_origins", "dr_joint", "task_state"),
             rough=True, gait="biped", inj_tail=True, stacks=True, frames=(31, 134, None), kernel_skip_env0=True),
    # keep_ankle_pitch_zero_in_air: the class defines it, the shipped config leaves it unscaled
    TaskSpec("tron1_sf", "TRON1SFCfg", _PLANE_EXACT, _PF_FLOATS + ("sim_base_quat", "dr_pd", "dr_joint"),
             reward_scales=(("keep_ankle_pitch_zero_in_air", 0.2),)),
)}


# ------------------------------------------------------------------------------------------------------------------------------
# task_state rows of the kernel (include/lgsim.h) as (oracle attribute, width); None: a column the oracle does not hold
TASK_STATE = {
    "wtw": (("gait_time", 1), ("phi", 1), ("gait_period", 1), ("base_height_target", 1), ("foot_clearance_target", 1),
            ("pitch_target", 1), ("theta", 4), ("clock_input", 8), ("exp_C_frc", 4)),                  # LG_TASK_STATE_WTW
    "biped": (("gait_time", 1), ("phi", 1), ("gait_period", 1), (None, 1), ("theta", 2), ("clock_input", 4), ("exp_C_frc", 2)),
}                                                                                                      # LG_TASK_STATE_BIPED
GAIT = {0: None, 1: "wtw", 2: "biped"}        # LgTaskCfg.gait_mode


def task_state_rows(gait, o):
    """The kernel's task_state rows from the oracle's gait attributes."""
    return np.concatenate([getattr(o, a) if a else np.zeros((o.N, w), np.float32) for a, w in TASK_STATE[gait]], 1)


def set_task_state(gait, o, rows, command_ranges=None):
    """The oracle's gait attributes from the kernel's task_state rows; for wtw also the behaviour ranges from command_ranges[8:17]."""
    c = 0
    for a, w in TASK_STATE[gait]:
        if a:
            getattr(o, a)[:] = rows[:, c:c + w]
        c += w
    if gait == "wtw" and command_ranges is not None:
        set_behavior_ranges(o, command_ranges[8:17])


def set_behavior_ranges(o, br):
    """The oracle's behaviour ranges from the nine floats of MdpOracle.behavior_ranges() / command_ranges[8:17]."""
    o.gait_period_range, o.base_height_target_range = list(br[0:2]), list(br[2:4])
    o.foot_clearance_target_range, o.pitch_target_range, o.num_gaits = list(br[4:6]), list(br[6:8]), int(br[8])


def recorded_task_state(gait, rows):
    """task_state as the fixtures record it: the biped's without its gait period and pad (tron1_pf_ee.py keeps the period fixed)."""
    return rows if gait == "wtw" else np.delete(rows, [2, 3], axis=1)


# ------------------------------------------------------------------------------------------------------------------------------
class Fixture(dict):
    """A fixture held in memory; `.files` as on the NpzFile of a golden fixture."""
    @property
    def files(self):
        return list(self.keys())


def golden(spec):
    return Fixture(np.load(spec.gold))


def fixture_steps(fx):
    """(t, sim_in, actions, R, counter, esum_override) of every step: the physics read-backs the step's MDP phases start from
    (script_* and the previous velocities), copied since the steppers modify them in place.  foot_quat, which the reference read
    from rigid_body_states, is left out: the oracle and the kernel derive it from base_quat and dof_pos.  T and N are those of
    the uniforms, which every fixture holds, recorded or not."""
    for t in range(fx["rand"].shape[0]):
        sim = {k[len("script_"):]: fx[k][t].copy() for k in fx.files if k.startswith("script_") and k != "script_foot_quat"}
        sim["last_dof_vel"] = fx["last_dof_vel_in"][t].copy()
        sim["last_feet_vel"] = fx["last_feet_vel_in"][t].copy()
        yield t, sim, fx["actions_in"][t].copy(), fx["rand"][t], int(fx["counter"][t]), float(fx["esum_override"][t])


def replay(spec, fx, stepper, tol):
    """Drive `stepper(spec, fx, N)` through the fixture, checking every step at the tolerances `tol` (keyword arguments of check)."""
    st = stepper(spec, fx, fx["rand"].shape[1])
    for t, sim, actions, R, counter, override in fixture_steps(fx):
        check(spec, t, fx, st.step(t, sim, actions, R, counter, override), **tol)


def outputs(spec, st, fx):
    """The quantities check() compares, formed from a stepper's post-step buffers st[name]."""
    keys = spec.exact + spec.floats + (("dr",) if spec.go2 else ()) + (("cstr_prob", "cstr_sums") if spec.cstr else ())
    keys += ("feat_full", "priv_full") if spec.stacks else ()
    return {k: _output(spec, st, fx, k) for k in keys}


_BUFFER = dict(reset="reset_buf", time_out="time_out_buf", ep_len="episode_length_buf", rew="rew_buf", labels="labels_buf",
               priv="priv_obs_buf", feat_full="obs_buf", priv_full="priv_obs_buf")
_JOINED = dict(dr_pd=("kp_scale", "kd_scale"), dr_joint=("joint_armature", "joint_friction", "joint_damping"))


def _output(spec, st, fx, k):
    if k.startswith("sim_"):
        return st[k[len("sim_"):]]
    if k in _BUFFER:
        return st[_BUFFER[k]]
    if k == "act_hist":
        return np.stack([st["actions"], st["last_actions"], st["llast_actions"]])
    if k in _JOINED:
        return np.concatenate([st[b] for b in _JOINED[k]], 1)
    if k == "dr":
        return np.concatenate([st["friction_values"], st["added_base_mass"], st["base_com_bias"], st["rand_push_vels"][:, :2]], 1)
    if k == "episode_sums":
        es = st["episode_sums"]
        return np.stack([es[abi.reward_id(str(n), st.model.joints_per_leg)] for n in fx["reward_names"]])
    if k == "task_state":
        return recorded_task_state(spec.gait, st["task_state"])
    if k == "cmd_range_x":
        return st["command_ranges"][:2]
    actor, critic, cols = spec.frames or (None, None, None)
    if k == "obs":          # the rough heads: the newest actor frame
        return st["obs_buf"][:, -actor:] if spec.rough else st["obs_buf"]
    if k == "feat_new":
        return st["obs_buf"][:, -actor:]
    if k == "priv_new":
        return st["priv_obs_buf"][:, -critic:]
    if k == "contact_states":
        return st["priv_obs_buf"][:, -critic:][:, cols]
    return st[k]


def check(spec, t, fx, out, rtol, atol, atol_yaw=None, skip_env0=False):
    """Step t's outputs against the fixture: spec.exact as int64, spec.floats at rtol / atol (atol_yaw on YAW_KEYS), all envs or all
    but env 0."""
    env = slice(1, None) if skip_env0 else slice(None)

    def envs(k, a):           # the env axis is 1 of the (term or history, N) stacks
        return a[:, env] if k in ("episode_sums", "act_hist", "cstr_sums") else a[env]
    labels = dict(spec.labels)
    for k in spec.exact:
        np.testing.assert_array_equal(envs(k, np.asarray(out[k]).astype(np.int64)), envs(k, fx[k][t].astype(np.int64)), err_msg=f"{k} @ step {t}")
    for k in spec.floats:
        got = np.asarray(out[k])
        a = atol_yaw if atol_yaw is not None and k in YAW_KEYS else atol
        np.testing.assert_allclose(envs(k, got), envs(k, fx[k][t].reshape(got.shape)), rtol=rtol, atol=a,
                                   err_msg=f"{labels.get(k, k)} @ step {t}")
    if spec.go2:
        # DR values: friction/mass/com from the fake simulator's draws; added mass starts at 1 in the reference's buffer
        # (genesis_simulator.py:648) but 0 here until the first reset of an env
        dr_ref, dr = fx["dr"][t], np.asarray(out["dr"])
        touched = np.abs(dr_ref[:, 1] - 1.0) > 0
        touched[0] &= not skip_env0
        np.testing.assert_allclose(dr[touched], dr_ref[touched], rtol=rtol, atol=atol, err_msg=f"dr @ step {t}")
    if spec.stacks and t == fx["rand"].shape[0] - 1:
        np.testing.assert_allclose(out["feat_full"][env], fx["feat_last"][env], rtol=rtol, atol=atol, err_msg="stacked estimator features")
        np.testing.assert_allclose(out["priv_full"][env], fx["priv_last"][env], rtol=rtol, atol=atol, err_msg="stacked critic obs")
    if spec.cstr:          # termination probability and per-episode violation counters, exact
        for k in ("cstr_prob", "cstr_sums"):
            np.testing.assert_array_equal(envs(k, np.asarray(out[k])), envs(k, fx[k][t]), err_msg=f"{k} @ step {t}")


# ------------------------------------------------------------------------------------------------------------------------------
class OracleStepper:
    """MdpOracle in the fixture's initial state.  The fixture's generator started from a fake simulator with friction 0 and added
    mass 1 (genesis_simulator.py:646-649 before the create-time randomisation, which the fake does not perform); the go2 fixture
    compares the DR values only where a reset drew them, so go2 starts from the oracle's own values."""

    def __init__(self, spec, fx, N):
        from hcr_genesis_lr_cl_amd import builders
        from hcr_genesis_lr_cl_amd.model_compiler import load_model
        from oracle.mdp_oracle import MdpOracle
        self.spec, self.fx, self.cfg = spec, fx, spec.cfg()
        self.model = load_model(self.cfg.asset.name)
        task = builders.make_task_cfg(self.model, self.cfg)
        o = self.o = MdpOracle(self.model, self.cfg, task, N, fx["init_env_origins"])
        o.episode_length_buf[:] = fx["init_episode_length_buf"]
        o.commands[:] = fx["init_commands"]
        if not spec.go2:
            o.friction_values[:] = 0
            o.added_base_mass[:] = 1
        self.terrain = None
        if spec.rough:
            from hcr_genesis_lr_cl_amd.terrain import Terrain
            np.random.seed(int(fx["terrain_seed"]))
            self.terrain = Terrain(self.cfg.terrain)
            o.terrain_levels[:], o.terrain_types[:] = fx["init_terrain_levels"], fx["init_terrain_types"]
            o.terrain_origins = self.terrain.env_origins.astype(np.float32)
        if spec.gait:
            o.theta[:], o.gait_time[:], o.phi[:] = fx["init_theta"], fx["init_gait_time"], fx["init_phi"]
        if spec.gait == "wtw":
            o.gait_period[:] = fx["init_gait_period"]
            set_behavior_ranges(o, fx["init_behavior_ranges"])
        self.sim = {}

    def __getitem__(self, name):
        if name == "task_state":
            return task_state_rows(self.spec.gait, self.o)
        return self.sim[name] if name in self.sim else getattr(self.o, name)

    def step(self, t, sim, actions, R, counter, override):
        from oracle import mdp_oracle as mo
        o = self.o
        if self.spec.go2 and override:
            o.episode_sums[abi.REWARD_ID["tracking_lin_vel"]][:] = override
            o.episode_length_buf[:4] = 1000
        if self.terrain is not None:
            c, hf = self.cfg.terrain, self.terrain.height_field_raw
            sim["measured_heights"] = mo.sample_heights(sim["base_pos"], sim["base_quat"], self.fx["init_height_points"], hf,
                                                        c.border_size, c.horizontal_scale, c.vertical_scale)
            sim["height_around_feet"], sim["normals"] = mo.feet_terrain_info(sim["feet_pos"].reshape(len(actions), o.F, 3), hf,
                                                                              c.border_size, c.horizontal_scale, c.vertical_scale)
        o.step(sim, actions, R, counter)
        self.sim = sim
        out = outputs(self.spec, self, self.fx)
        if "obs" in out:      # the kernel clips the actor history as it stores it, the reference only the frames it returns
            out["obs"] = np.clip(out["obs"], -100.0, 100.0)
        return out


class KernelStepper:
    """The HIP kernel's MDP phases (PRE | POST | RESET through the C ABI) from the OracleStepper's initial state, with the fixture's
    physics read-backs, uniforms and, on rough terrain, terrain read-backs injected."""

    def __init__(self, spec, fx, N):
        import torch
        start = OracleStepper(spec, fx, N)
        o = start.o
        self.spec, self.fx, self.model = spec, fx, start.model
        self.eng, *_ = make_engine(N, start.cfg, terrain=start.terrain, height_points=fx["init_height_points"] if spec.rough else None)
        for k in ("env_origins", "episode_length_buf", "commands", "friction_values", "added_base_mass", "terrain_levels",
                  "terrain_types", "joint_armature", "joint_friction", "joint_damping"):
            if k in self.eng.buf:
                put(self.eng, k, getattr(o, k))
        if spec.gait:
            put(self.eng, "task_state", task_state_rows(spec.gait, o))
        if spec.gait == "wtw":
            self.eng.buf["command_ranges"][8:17] = torch.from_numpy(o.behavior_ranges()).cuda()
        self.sim = {}

    def __getitem__(self, name):
        return self.sim[name] if name in TERRAIN_READ_BACKS else get(self.eng, name)

    def step(self, t, sim, actions, R, counter, override):
        import torch
        eng, fx = self.eng, self.fx
        k = abi.REWARD_ID["tracking_lin_vel"]
        if self.spec.go2 and override:
            eng.buf["episode_sums"][k].fill_(override)
            eng.buf["episode_length_buf"][:4] = 1000
        if self.spec.rough:      # the SIM phase's terrain read-backs (checked separately against the numpy sampler)
            sim.update({n: fx[n][t] for n in TERRAIN_READ_BACKS})
        load_sim(eng, sim)
        put(eng, "rand_in", R)
        if "cstr_prob" in eng.buf:       # go2_cat: the job-wide "some env moves a joint faster than 4 rad/s" flag (envs/go2_ts.py Go2CaT._any_fast)
            eng.buf["command_ranges"][abi.CR_ANY_FAST + (counter & 1)] = float(np.any(np.abs(sim["dof_vel"]) > 4.0))   # what the SIM phase raises
        act = torch.from_numpy(actions).cuda()
        if self.spec.go2 and counter % 1000 == 0:       # command-curriculum gate, same split as envs/legged_robot.py
            eng.step(abi.PHASE_PRE | abi.PHASE_POST, act, counter)
            ids = eng.buf["reset_buf"].nonzero().flatten()
            if len(ids):
                mean = torch.mean(eng.buf["episode_sums"][k][ids]) / 1000.0
                if mean > 0.8 * (1.0 * 0.02):
                    cr = eng.buf["command_ranges"]
                    cr[0], cr[1] = max(float(cr[0]) - 0.5, -1.0), min(float(cr[1]) + 0.5, 1.0)
            eng.step(abi.PHASE_RESET, None, counter)
        else:
            eng.step(abi.PHASE_PRE | abi.PHASE_POST | abi.PHASE_RESET, act, counter)
        torch.cuda.synchronize()
        self.sim = sim
        return outputs(self.spec, self, fx)


# ------------------------------------------------------------------------------------------------------------------------------
def make_engine(N, cfg=None, terrain=None, height_points=None, inject_rand=True, seed=None, env_id_offset=0):
    """An Engine on cuda:0 for `cfg` (default GO2Cfg) with the config's command ranges in command_ranges[:8]; the heightfield of
    `terrain` with its origins and `height_points` uploaded.  Returns (engine, model, cfg, task)."""
    import torch
    from hcr_genesis_lr_cl_amd import builders
    from hcr_genesis_lr_cl_amd.config import GO2Cfg
    from hcr_genesis_lr_cl_amd.engine import Engine
    from hcr_genesis_lr_cl_amd.model_compiler import load_model
    cfg = cfg or GO2Cfg()
    model = load_model(cfg.asset.name)
    desc, opts = builders.make_model_desc(model, cfg), builders.make_sim_options(model, cfg, terrain)
    task = builders.make_task_cfg(model, cfg, seed=seed, env_id_offset=env_id_offset)
    eng = Engine(model, desc, opts, task, N, "cuda:0", inject_rand=inject_rand)
    drop_unused_joint_dr(eng, task)
    if terrain is not None:
        eng.set_terrain(terrain.height_field_raw, terrain.env_origins, height_points)
    cr = cfg.commands.ranges
    eng.buf["command_ranges"][:8] = torch.tensor(list(cr.lin_vel_x) + list(cr.lin_vel_y) + list(cr.ang_vel_yaw) + list(cr.heading))
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
    """The physics read-backs (and, where `sim` holds them, the terrain read-backs) into the engine, with the base-frame quantities
    the SIM phase derives from them."""
    from oracle import mdp_oracle as mo
    for k in SIM_KEYS:
        put(eng, k, sim[k])
    for k, b in TERRAIN_READ_BACKS.items():
        if k in sim:
            put(eng, b, sim[k])
    q = sim["base_quat"]
    put(eng, "base_lin_vel", mo.quat_rotate_inverse(q, sim["base_lin_vel_w"]))
    put(eng, "base_ang_vel", mo.quat_rotate_inverse(q, sim["base_ang_vel_w"]))
    put(eng, "projected_gravity", mo.quat_rotate_inverse(q, np.tile(np.array([0, 0, -1], np.float32), (len(q), 1))))
    put(eng, "base_euler", mo.get_euler_xyz(q))

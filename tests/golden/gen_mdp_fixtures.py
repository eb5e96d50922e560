"""Generates golden vectors for the MDP part of the hot path by RUNNING THE REFERENCE'S OWN
env classes (legged_gym/envs/...) on CPU against a fake simulator that feeds scripted physics
read-backs.  Output: tests/golden/<task>_mdp.npz (inputs + expected outputs per step), one per task of mdp_harness.TASKS.

Needs the reference checkout:   PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_mdp_fixtures.py [task ...]      (default: all)
generate(name) is the one generator; GEN holds what differs between the tasks and READ where every recorded array comes from.
tests/golden/check_fixtures.py checks that this and the other generators still reproduce the committed files byte for byte.

What is pinned: everything LeggedRobot.step does around the physics -- action clip/history
(legged_robot.py:230-239), command resampling + heading command + push schedule (:300-334),
termination (:78-92), every active reward term and the alphabetical sum (:150-168, 458-608),
reset_idx bookkeeping incl. command curriculum (:94-148, 336-348), task reset distributions
and observation layout/noise/clip (go2.py:17-134, legged_robot.py:48-49).
Uniform draws of the reference are intercepted (DrawRecorder) and stored per env in the slot
layout of include/lgsim.h's LgRandSlots, so the kernel can be fed the very same numbers.
"""
import contextlib
import dataclasses
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_harness as rh  # noqa: E402

rh.load_reference()
import torch  # noqa: E402

from hcr_genesis_lr_cl_amd import builders  # noqa: E402
from hcr_genesis_lr_cl_amd.model_compiler import load_model  # noqa: E402
from tests.mdp_harness import TASKS, TASK_STATE, recorded_task_state  # noqa: E402

torch.set_num_threads(2)


def rand_quat(rng, n, tilt):
    rpy = rng.normal(size=(n, 3)) * [tilt, tilt, 1.5]
    cr, sr = np.cos(rpy[:, 0] / 2), np.sin(rpy[:, 0] / 2)
    cp, sp = np.cos(rpy[:, 1] / 2), np.sin(rpy[:, 1] / 2)
    cy, sy = np.cos(rpy[:, 2] / 2), np.sin(rpy[:, 2] / 2)
    q = np.stack([cy * sr * cp - sy * cr * sp, cy * cr * sp + sy * sr * cp, sy * cr * cp - cy * sr * sp,
                  cy * cr * cp + sy * sr * sp], 1)
    return q.astype(np.float32)


class FakeSimulator:
    """Duck-typed stand-in for GenesisSimulator: serves scripted read-backs, records writes."""

    def __init__(self, cfg, sim_params, device, headless):
        from legged_gym.utils.math_utils import quat_rotate_inverse
        self._qri = quat_rotate_inverse
        self._cfg, self._device = cfg, device
        N = self._num_envs = cfg.env.num_envs
        A = self._num_actions = cfg.env.num_actions
        self.model = load_model(cfg.asset.name)
        m = self.model
        L, F = m.n_links, m.n_legs
        z = lambda *s: torch.zeros(*s)
        self._base_pos, self._base_quat, self._base_euler = z(N, 3), z(N, 4), z(N, 3)
        self._base_quat[:, 3] = 1
        self._base_lin_vel, self._base_ang_vel, self._projected_gravity = z(N, 3), z(N, 3), z(N, 3)
        self._base_lin_vel_w, self._base_ang_vel_w = z(N, 3), z(N, 3)
        self._dof_pos, self._dof_vel, self._last_dof_vel, self._torques = z(N, A), z(N, A), z(N, A), z(N, A)
        self._link_contact_forces = z(N, L, 3)
        self._feet_pos, self._feet_vel, self._last_feet_vel = z(N, F, 3), z(N, F, 3), z(N, F, 3)
        self._feet_indices = m.find_link_indices([n for n in m.link_names if cfg.asset.foot_name in n])
        self._termination_contact_indices = m.find_link_indices(cfg.asset.terminate_after_contacts_on)
        self._penalized_contact_indices = m.find_link_indices(cfg.asset.penalize_contacts_on)
        self._default_dof_pos = torch.tensor([cfg.init_state.default_joint_angles[n] for n in cfg.asset.dof_names]).unsqueeze(0)
        lim = torch.tensor(np.stack([m.arrays["q_lo"], m.arrays["q_hi"]], 1), dtype=torch.float)
        for i in range(A):  # genesis_simulator.py:373-382
            mid = (lim[i, 0] + lim[i, 1]) / 2
            r = lim[i, 1] - lim[i, 0]
            lim[i, 0] = mid - 0.5 * r * cfg.rewards.soft_dof_pos_limit
            lim[i, 1] = mid + 0.5 * r * cfg.rewards.soft_dof_pos_limit
        self._dof_pos_limits = lim
        self._base_init_pos = torch.tensor(cfg.init_state.pos)
        self._base_init_quat = torch.tensor(cfg.init_state.rot)
        self._custom_origins = cfg.terrain.mesh_type in ("heightfield", "trimesh")
        self._env_origins = z(N, 3)
        self._env_origins[:, :2] = torch.from_numpy(np.random.default_rng(5).uniform(-5, 5, (N, 2)).astype(np.float32))
        self._measured_heights = z(N, 187)
        self._friction_values, self._added_base_mass = z(N, 1), torch.ones(N, 1)
        self._base_com_bias, self._rand_push_vels = z(N, 3), z(N, 3)
        self._kp_scale, self._kd_scale = torch.ones(N, A), torch.ones(N, A)
        self._joint_armature, self._joint_friction, self._joint_damping = z(N, 1), z(N, 1), z(N, 1)
        self.dof_names = list(cfg.asset.dof_names)   # tron1_pf_ee.py:171 reads simulator.dof_names (absent from the reference ABC)
        self._global_gravity = torch.tensor([0., 0., -1.]).repeat(N, 1)
        self._rigid_body_states = z(N, L, 13)                   # only [:, feet, 3:7] is read (tron1_sf.py:300)
        self._rigid_body_states[:, :, 6] = 1
        self.script, self.t, self.rec = None, -1, None

    # -- scripted physics ------------------------------------------------------------------
    def step(self, actions):
        self._last_dof_vel[:] = self._dof_vel
        self._last_feet_vel[:] = self._feet_vel
        self.t += 1

    def post_physics_step(self):
        s = {k: torch.from_numpy(v[self.t]) for k, v in self.script.items()}
        for k in ("base_pos", "base_quat", "base_lin_vel_w", "base_ang_vel_w", "dof_pos", "dof_vel", "torques",
                  "link_contact_forces", "feet_pos", "feet_vel"):
            getattr(self, "_" + k)[:] = s[k].reshape(getattr(self, "_" + k).shape)
        if "foot_quat" in s:
            self._rigid_body_states[:, self._feet_indices, 3:7] = s["foot_quat"]
        self._base_lin_vel[:] = self._qri(self._base_quat, self._base_lin_vel_w)
        self._base_ang_vel[:] = self._qri(self._base_quat, self._base_ang_vel_w)
        self._projected_gravity = self._qri(self._base_quat, self._global_gravity)
        from legged_gym.utils.math_utils import get_euler_xyz
        self._base_euler[:] = get_euler_xyz(self._base_quat)

    # -- writes (semantics of genesis_simulator.py:62-158) ---------------------------------------
    def reset_idx(self, env_ids):
        """Order and formulas of genesis_simulator.py:62-82, 665-739; draws go through the recorder."""
        d = self._cfg.domain_rand
        n = len(env_ids)
        ids = torch.as_tensor(env_ids)
        if d.randomize_friction:
            lo, hi = d.friction_range
            self._friction_values[env_ids] = self.rec.tagged("dr_friction", (n, 1), ids) * (hi - lo) + lo
        if d.randomize_base_mass:
            lo, hi = d.added_mass_range
            self._added_base_mass[env_ids] = self.rec.tagged("dr_mass", (n, 1), ids) * (hi - lo) + lo
        if d.randomize_com_displacement:
            for k, (lo, hi) in enumerate((d.com_pos_x_range, d.com_pos_y_range, d.com_pos_z_range)):
                self._base_com_bias[env_ids, k] = self.rec.tagged(f"dr_com+{k}", (n, 1), ids).squeeze(1) * (hi - lo) + lo
        for k, (flag, rng_name, buf) in enumerate((("randomize_joint_armature", "joint_armature_range", "_joint_armature"),
                                                   ("randomize_joint_friction", "joint_friction_range", "_joint_friction"),
                                                   ("randomize_joint_damping", "joint_damping_range", "_joint_damping"))):
            if getattr(d, flag):
                lo, hi = getattr(d, rng_name)
                getattr(self, buf)[env_ids, 0] = self.rec.tagged(f"dr_joint+{k}", (n,), ids) * (hi - lo) + lo
        if d.randomize_pd_gain:
            A = self._num_actions
            self._kp_scale[env_ids] = (d.kp_range[1] - d.kp_range[0]) * self.rec.tagged("dr_kp", (n, A), ids) + d.kp_range[0]
            self._kd_scale[env_ids] = (d.kd_range[1] - d.kd_range[0]) * self.rec.tagged("dr_kd", (n, A), ids) + d.kd_range[0]
        self._last_dof_vel[env_ids] = 0.
        self._last_feet_vel[env_ids] = 0.

    def reset_dofs(self, env_ids, dof_pos, dof_vel):
        self._dof_pos[env_ids] = dof_pos[:]
        self._dof_vel[env_ids] = dof_vel[:]

    def reset_root_states(self, env_ids, base_pos, base_quat, base_lin_vel, base_ang_vel):
        self._base_pos[env_ids, :] = base_pos[:]
        self._base_quat[env_ids, :] = base_quat[:]
        self._projected_gravity = self._qri(self._base_quat, self._global_gravity)
        self._base_lin_vel[env_ids] = base_lin_vel[:]
        self._base_ang_vel[env_ids] = base_ang_vel[:]
        self._base_lin_vel_w[env_ids] = base_lin_vel[:]
        self._base_ang_vel_w[env_ids] = base_ang_vel[:]

    def push_robots(self):
        m = self._cfg.domain_rand.max_push_vel_xy
        env_ids = torch.arange(self._num_envs)  # noqa: F841  (picked up by the recorder)
        push = self.rec.rand_float(-m, m, (self._num_envs, 2), "cpu")
        self._rand_push_vels[:, :2] = push.clone()
        self._base_lin_vel_w[:, :2] += push

    def update_sensors(self):
        pass

    def draw_debug_vis(self):
        pass

    def set_viewer_camera(self, eye, target):
        pass


for _p in ("rigid_body_states", "feet_indices", "termination_contact_indices", "penalized_contact_indices", "dof_pos_limits",
           "base_init_pos", "base_init_quat", "base_lin_vel", "base_ang_vel", "projected_gravity", "dof_pos",
           "dof_vel", "last_dof_vel", "feet_pos", "feet_vel", "last_feet_vel", "base_pos", "base_quat",
           "base_euler", "measured_heights", "link_contact_forces", "torques", "default_dof_pos", "custom_origins",
           "env_origins"):
    setattr(FakeSimulator, _p, property(lambda s, _n="_" + _p: getattr(s, _n)))
FakeSimulator.feet_contact_indices = property(lambda s: s._feet_indices)
FakeSimulator.dr_friction_values = property(lambda s: s._friction_values)
FakeSimulator.dr_added_base_mass = property(lambda s: s._added_base_mass)
FakeSimulator.dr_base_com_bias = property(lambda s: s._base_com_bias)
FakeSimulator.dr_rand_push_vels = property(lambda s: s._rand_push_vels)


class RoughFakeSimulator(FakeSimulator):
    """Adds the heightfield side: the terrain comes from the reference's own Terrain class, and the
    height sampling / feet terrain info / contact states / terrain curriculum are the reference's own
    GenesisSimulator methods executed on this object (genesis_simulator.py:53-60, 140-148, 496-610)."""
    TERRAIN_SEED = 3

    def __init__(self, cfg, sim_params, device, headless):
        super().__init__(cfg, sim_params, device, headless)
        from legged_gym.simulator.genesis_simulator import GenesisSimulator as GS
        from legged_gym.utils.terrain import Terrain
        self.GS = GS
        np.random.seed(self.TERRAIN_SEED)
        self._terrain = Terrain(cfg.terrain)
        self._height_samples = torch.tensor(self._terrain.heightsamples).view(self._terrain.tot_rows, self._terrain.tot_cols)
        N = self._num_envs
        self._custom_origins = True
        self._max_terrain_level = cfg.terrain.num_rows
        rng = np.random.default_rng(17)
        self._terrain_levels = torch.from_numpy(rng.integers(0, cfg.terrain.num_rows, N))
        self._terrain_types = torch.div(torch.arange(N), (N / cfg.terrain.num_cols), rounding_mode='floor').to(torch.long)
        self._terrain_origins = torch.from_numpy(self._terrain.env_origins).to(torch.float)
        self._env_origins = self._terrain_origins[self._terrain_levels, self._terrain_types].clone()
        GS._init_height_points(self)
        self._measured_heights = torch.zeros(N, self._num_height_points)
        F = self.model.n_legs
        self._normal_vector_around_feet = torch.zeros(N, F * 3)
        self._height_around_feet = torch.zeros(N, F, 9)
        self._contact_state_link_indices = self.model.find_link_indices(cfg.asset.contact_state_link_names)
        self._link_contact_states = torch.zeros(N, len(self._contact_state_link_indices))

    def post_physics_step(self):
        super().post_physics_step()
        self._link_contact_states = 1. * (torch.norm(self._link_contact_forces[:, self._contact_state_link_indices, :], dim=-1) > 1.)
        self.GS._update_surrounding_heights(self)
        self.GS._calc_terrain_info_around_feet(self)

    def update_terrain_curriculum(self, env_ids, move_up, move_down):
        # the randint of genesis_simulator.py:144-145 goes through the recorder
        orig = torch.randint_like
        torch.randint_like = lambda t, high: self.rec.randint_like(t, high, env_ids)
        try:
            self.GS.update_terrain_curriculum(self, env_ids, move_up, move_down)
        finally:
            torch.randint_like = orig


for _p in ("terrain_levels", "terrain_types", "link_contact_states", "normal_vector_around_feet", "height_around_feet"):
    setattr(RoughFakeSimulator, _p, property(lambda s, _n="_" + _p: getattr(s, _n)))


def make_script(rng, model, cfg, N, T):
    """Scripted read-backs: independent plausible states per step, biased to exercise branches."""
    A, L, F = model.n_dof, model.n_links, model.n_legs
    q0 = np.array([cfg.init_state.default_joint_angles[n] for n in cfg.asset.dof_names], np.float32)
    s = {}
    s["base_pos"] = (rng.normal(size=(T, N, 3)) * [2, 2, 0.03] + [0, 0, 0.32]).astype(np.float32)
    rng.random((T, N))           # unused, but part of the stream every fixture was drawn from
    s["base_quat"] = np.stack([rand_quat(rng, N, 0.15) for t in range(T)])
    big = rng.random((T, N)) < 0.08
    for t in range(T):
        if big[t].any():
            s["base_quat"][t][big[t]] = rand_quat(rng, int(big[t].sum()), 1.3)
    s["base_lin_vel_w"] = (rng.normal(size=(T, N, 3)) * [0.6, 0.4, 0.15]).astype(np.float32)
    s["base_ang_vel_w"] = (rng.normal(size=(T, N, 3)) * [0.5, 0.5, 0.8]).astype(np.float32)
    s["dof_pos"] = (q0 + rng.normal(size=(T, N, A)) * 0.35).astype(np.float32)
    s["dof_vel"] = (rng.normal(size=(T, N, A)) * 3.0).astype(np.float32)
    s["torques"] = (rng.normal(size=(T, N, A)) * 8.0).astype(np.float32)
    f = np.zeros((T, N, L, 3), np.float32)
    feet = [int(i) for i in model.arrays["foot_link"][:F]]
    for l in range(L):
        if l in feet:
            on = rng.random((T, N)) < 0.6
            f[:, :, l, 2] = on * rng.uniform(0.05, 80, (T, N))
            f[:, :, l, :2] = on[..., None] * rng.normal(size=(T, N, 2)) * 10
        else:
            on = rng.random((T, N)) < (0.06 if l == 0 else 0.1)
            f[:, :, l] = on[..., None] * rng.normal(size=(T, N, 3)) * (12 if l == 0 else 3)
    s["link_contact_forces"] = f
    s["feet_pos"] = (rng.normal(size=(T, N, F, 3)) * [0.2, 0.15, 0.03] + [0, 0, 0.05]).astype(np.float32)
    s["feet_vel"] = (rng.normal(size=(T, N, F, 3)) * [0.8, 0.4, 0.5]).astype(np.float32)
    return s


def slots_from_calls(calls, slots, N, A, policy_dof_groups):
    """Scatter the recorded draws of one step into the (N, n_slots) row layout."""
    R = np.zeros((N, slots.n_slots), np.float32)
    seen = {}
    for c in calls:
        key = (c["caller"], c["parent"])
        k = seen.get(key, 0)
        seen[key] = k + 1
        u = c["u"].numpy()
        ids = None if c["env_ids"] is None else c["env_ids"].numpy()
        if c["caller"] == "_resample_commands":
            base = slots.cb_cmd if c["parent"] == "_post_physics_step_callback" else slots.reset_cmd
            R[ids, base + k] = u[:, 0]
        elif c["caller"] == "push_robots":
            R[:, slots.push:slots.push + 2] = u
        elif c["caller"] == "_reset_dofs":
            cols = policy_dof_groups[k]
            for j, col in enumerate(cols):
                R[ids, slots.reset_dof + col] = u[:, j]
        elif c["caller"] == "_reset_root_states":
            if u.shape[1] == 2:
                base = slots.reset_root_xy
            else:
                k3 = seen.get("root3", 0)
                seen["root3"] = k3 + 1
                base = [slots.reset_lin_vel, slots.reset_ang_vel][k3]
            R[ids, base:base + u.shape[1]] = u
        elif c["caller"].startswith("tag:"):
            name, _, off = c["caller"][4:].partition("+")
            base = getattr(slots, name) + (int(off) if off else 0)
            uu = u.reshape(len(ids), -1)
            R[ids, base:base + uu.shape[1]] = uu
        elif c["caller"] == "torch_rand:reset_idx":          # tron1_pf_ee.py:220-225: theta offset, gait time
            R[ids, slots.task_reset + 1 + k] = u[:, 0]
        elif c["caller"] == "np_random:reset_idx":           # tron1_pf_ee.py:204 sit-pose coin, one per call
            R[ids, slots.task_reset] = float(u[0])
        elif c["caller"] == "_reset_root_states_sit_pose":
            if u.shape[1] == 2:
                R[ids, slots.reset_root_xy:slots.reset_root_xy + 2] = u
        elif c["caller"] == "_resample_behavior_params":
            base = slots.task_cb if c["parent"] == "_post_physics_step_callback" else slots.task_reset
            R[ids, base + k] = u[:, 0]
        elif c["caller"] == "randint:_resample_behavior_params":
            base = slots.task_cb if c["parent"] == "_post_physics_step_callback" else slots.task_reset
            R[ids, base + 4] = float(u[0])
        elif c["caller"] == "randint_like":
            R[ids, slots.terrain_level] = u
        elif c["caller"] == "rand_like":
            R[:, slots.noise:slots.noise + u.shape[1]] = u
        else:
            raise RuntimeError(f"unmapped draw from {c['caller']} <- {c['parent']}")
    return R


# ------------------------------------------------------------------------------------------------------------------------------
# What differs between the tasks.  mdp_harness.TASKS[name] already states the config class and reward scales, rough / gait / cstr /
# stacks and the frame widths; a Gen adds what only the generator needs.  Hooks that draw from `rng` are called at fixed points of
# generate(): make_script, place, episode clocks, commands, gait state, then one action draw per step.
def _onto_tiles(script, sim, rng):
    """Base xy around each env's origin, some far enough to be promoted (> 4 m); returns the origins."""
    org = sim._env_origins.numpy()
    T, N = script["base_pos"].shape[:2]
    off = rng.normal(size=(T, N, 2)) * 1.5 + np.where(rng.random((T, N, 1)) < 0.3, 4.5, 0.0)
    script["base_pos"][:, :, :2] = (org[None, :, :2] + off).astype(np.float32)
    return org


def _biped_feet(script):
    script["feet_pos"][:, :, :, :2] = script["feet_pos"][:, :, :, :2] * 0.4 + script["base_pos"][:, :, None, :2]


def place_go2_rough(script, sim, rng):
    org = _onto_tiles(script, sim, rng)
    script["base_pos"][:, :, 2] += org[None, :, 2]
    script["feet_pos"][:, :, :, :2] += script["base_pos"][:, :, None, :2]
    script["feet_pos"][:, :, :, 2] += org[None, :, None, 2]


def place_tron1_rough(script, sim, rng):
    org = _onto_tiles(script, sim, rng)
    script["base_pos"][:, :, 2] += org[None, :, 2] + 0.4
    _biped_feet(script)
    script["feet_pos"][:, :, :, 2] += org[None, :, None, 2]


def place_tron1_pf(script, sim, rng):
    script["base_pos"][:, :, 2] += 0.36                       # nominal base height 0.68
    _biped_feet(script)


def _mat_to_quat(R):
    """xyzw quaternions of rotation matrices (..., 3, 3), w >= 0 branch-free enough for the tilts scripted here."""
    w = np.sqrt(np.maximum(0.0, 1.0 + R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2])) / 2
    x = np.sqrt(np.maximum(0.0, 1.0 + R[..., 0, 0] - R[..., 1, 1] - R[..., 2, 2])) / 2 * np.sign(R[..., 2, 1] - R[..., 1, 2] + 1e-30)
    y = np.sqrt(np.maximum(0.0, 1.0 - R[..., 0, 0] + R[..., 1, 1] - R[..., 2, 2])) / 2 * np.sign(R[..., 0, 2] - R[..., 2, 0] + 1e-30)
    z = np.sqrt(np.maximum(0.0, 1.0 - R[..., 0, 0] - R[..., 1, 1] + R[..., 2, 2])) / 2 * np.sign(R[..., 1, 0] - R[..., 0, 1] + 1e-30)
    q = np.stack([x, y, z, w], -1)
    return (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(np.float32)


def place_tron1_sf(script, sim, rng):
    """The foot orientation the class reads from rigid_body_states (tron1_sf.py:300) is scripted consistently with the scripted
    base orientation and joint angles."""
    from oracle.mdp_oracle import foot_rotations
    script["base_pos"][:, :, 2] += 0.43                       # nominal base height 0.75
    _biped_feet(script)
    script["foot_quat"] = np.stack([_mat_to_quat(foot_rotations(sim.model, q, p)) for q, p in zip(script["base_quat"], script["dof_pos"])])


def gait_wtw(env, rng, N):
    """Widen the behaviour ranges / gait set as the curriculum would, so every table entry is exercised."""
    env.num_gaits = 4
    env.gait_period_range = [0.3, 0.6]
    env.base_height_target_range = [0.2, 0.34]
    env.foot_clearance_target_range = [0.04, 0.12]
    env.pitch_target_range = [-0.3, 0.3]
    env.theta[:] = torch.from_numpy(rng.choice([0.0, 0.5], (N, 4)).astype(np.float32))
    env.gait_period[:] = torch.from_numpy(rng.uniform(0.3, 0.6, (N, 1)).astype(np.float32))
    env.gait_time[:] = torch.from_numpy(rng.uniform(0.0, 0.3, (N, 1)).astype(np.float32))
    env.phi[:] = env.gait_time / env.gait_period


def gait_biped(env, rng, N):
    env.theta[:, 0] = torch.from_numpy(rng.uniform(0, 1, N).astype(np.float32))
    env.theta[:, 1] = env.theta[:, 0] + 0.5
    env.gait_time[:] = torch.from_numpy(rng.uniform(0.0, 0.45, (N, 1)).astype(np.float32))
    env.phi[:] = env.gait_time / env.gait_period


# TaskSpec.gait -> (initial-state hook, the init_* keys it adds, the reference's per-foot exp_C_frc_<foot> attributes)
GAIT = {"wtw": (gait_wtw, ("theta", "gait_period", "gait_time", "phi"), ("fl", "fr", "rl", "rr")),
        "biped": (gait_biped, ("theta", "gait_time", "phi"), ("left", "right"))}


def go2_gate(env, t):
    """Cross the command-curriculum gate (counter 1000) soon after step 30, with episode sums above it; returns the value written.  Not
    done for go2_wtw / tron1_pf_ee: the reference calls a method that does not exist there (`self.update_command_curriculum`,
    go2_wtw.py:121, tron1_pf_ee.py:201) and would raise."""
    if t == 30:
        env.common_step_counter = 995
    if env.common_step_counter + 1 != 1000:
        return 0.0
    env.episode_sums["tracking_lin_vel"][:] = 18.5               # > 0.8 * scale * max_len = 16
    env.episode_length_buf[:4] = 1000                            # make sure somebody resets at this step
    return 18.5


def cat_limits(sim):
    """Properties of the Simulator ABC that CaT's constraints read (simulator.py: torque_limits, dof_vel_limits)."""
    type(sim).torque_limits = property(lambda s_: torch.tensor(s_.model.arrays["effort"], dtype=torch.float))
    type(sim).dof_vel_limits = property(lambda s_: torch.tensor(s_._cfg.asset.dof_vel_limits, dtype=torch.float).unsqueeze(0))


def still_commands(env):
    env.commands[:3] = 0.0            # standing-still envs (feet_contact_stand_still, CaT's style constraint)


def near_zero_commands(env):
    env.commands[::3, :3] *= 0.05     # hip_pos_zero_command, the air-time gate


@dataclasses.dataclass(frozen=True)
class Gen:
    module: str                       # the reference's task module; its config class lives in <module>_config
    cls: str
    cfg: str
    N: int
    T: int
    seed: int                         # of the recorder's stream; the script, initial state and actions draw from seed + 1
    returns: tuple                    # names for the tuple env.step() returns: obs / feat = actor side, priv = critic side
    keys: tuple                       # per-step arrays in the fixture's order (READ)
    groups: tuple                     # policy dofs of each _reset_dofs draw
    clocks: tuple                     # episode lengths to start from, so that resampling (commands: ep_len % 500 == 0) and time-outs
    #                                   (ep_len > 1000) occur inside the window
    counter: int = 495                # common_step_counter to start from: a push at the next multiple of the push interval
    patch: tuple = ()                 # PATCHABLE globals the task draws from, besides torch.rand_like
    patch_late: tuple = ()            # the same, installed only once the env is constructed
    place: object = None              # (script, sim, rng): put the scripted robots where the task's terrain / height terms expect them
    commands: object = None           # (env): command tweaks after the common draw
    big_action: float = 60.0          # action scale on every 7th step (clipping)


_LEGS3 = ((0, 3, 6, 9), (1, 4, 7, 10), (2, 5, 8, 11))                    # go2.py:30-35
_PLANE = ("obs", "priv", "rew", "reset", "extras")
_EE = ("feat", "labels", "priv", "rew", "reset", "extras")
_CLOCKS = (3, 120, 470, 495, 498, 499, 960, 985, 995, 998, 999, 1000)
_BIPED_CLOCKS = (3, 120, 470, 495, 498, 499, 968, 977, 985, 992, 995, 998, 999, 1000)
_TAIL = ("last_dof_vel_in", "last_feet_vel_in", "esum_override")
_ROUGH_KEYS = ("terrain_levels", "env_origins", "measured_heights", "height_around_feet", "normals")
_BIPED_KEYS = ("actions_in", "rand", "counter", "obs", "priv", "rew", "reset", "time_out", "commands", "ep_len", "fail_buf", "feet_air_time",
               "episode_sums", "act_hist", "sim_dof_pos", "sim_base_pos")


def _head(name, cls, returns=("obs", "labels", "feat", "priv", "rew", "reset", "extras")):
    """go2_ts / go2_cts / go2_dreamwaq / go2_cat (legged_gym/envs/__init__.py:82-86) AS CONFIGURED, recorded like go2_ee plus the
    clipped actor frame; `labels` is the single-frame auxiliary output (TS / CTS / CaT: privileged encoder input; Dreamwaq: explicit
    labels | next state).  As configured the asset selects 17 contact-state links while the size fields assume 12
    (go2_ts_config.py:8-14): what the class EMITS is pinned."""
    return Gen(f"legged_gym.envs.go2.{name}.{name}", cls, cls + "Cfg", 16, 36, 41, returns,
               ("actions_in", "rand", "counter", "obs", "feat_new", "priv_new", "labels", "rew", "reset", "time_out", "commands", "ep_len",
                "fail_buf", "feet_air_time", "episode_sums", "sim_dof_pos", "sim_base_pos") + _ROUGH_KEYS + ("contact_states",) + _TAIL
               + ("cstr_prob", "cstr_sums"),
               _LEGS3, (3, 470, 495, 498, 499, 968, 972, 977, 981, 985, 989, 992, 995, 998, 999, 1000),
               place=place_go2_rough, commands=still_commands)


# Rough tasks store only the newest frame of each stack per step (feat_new / priv_new) plus the full stacks at the last step
# (feat_last / priv_last) to keep the fixtures small; the stacking itself is checked on those.
GEN = {
    "go2": Gen("legged_gym.envs.go2.go2", "GO2", "GO2Cfg", 24, 64, 7, _PLANE,
               ("actions_in", "rand", "counter", "obs", "rew", "reset", "time_out", "commands", "ep_len", "fail_buf", "feet_air_time",
                "last_contacts", "episode_sums", "act_hist", "sim_dof_pos", "sim_dof_vel", "sim_base_pos", "sim_base_quat",
                "sim_base_lin_vel_w", "sim_projected_gravity", "sim_base_lin_vel", "dr", "cmd_range_x") + _TAIL,
               _LEGS3, (3, 120, 470, 480, 495, 498, 499, 960, 985, 995, 998, 999, 1000), counter=745),
    # periodic-gait rewards, behaviour parameters, 5-frame histories
    "go2_wtw": Gen("legged_gym.envs.go2.go2_wtw.go2_wtw", "GO2WTW", "GO2WTWCfg", 24, 64, 11, _PLANE,
                   ("actions_in", "rand", "counter", "obs", "priv", "rew", "reset", "time_out", "commands", "ep_len", "fail_buf",
                    "episode_sums", "act_hist", "sim_dof_pos", "sim_base_pos", "sim_base_lin_vel_w", "dr_pd", "task_state") + _TAIL,
                   (tuple(range(12)),),                                   # legged_robot.py:279-280: one (n, 12) draw
                   (3, 120, 245, 248, 249, 395, 398, 399, 498, 499, 748, 960, 985, 995, 998, 999, 1000), counter=745,
                   patch=("torch.randint",)),
    # heightfield terrain, terrain curriculum, estimator features / labels / critic stacks (go2_ee.py, legged_robot_ee.py)
    "go2_ee": Gen("legged_gym.envs.go2.go2_ee.go2_ee", "Go2EE", "Go2EECfg", 24, 48, 21, _EE,
                  ("actions_in", "rand", "counter", "feat_new", "priv_new", "labels", "rew", "reset", "time_out", "commands", "ep_len",
                   "fail_buf", "feet_air_time", "episode_sums", "sim_dof_pos", "sim_base_pos") + _ROUGH_KEYS + ("contact_states",) + _TAIL,
                  _LEGS3, _CLOCKS, place=place_go2_rough),
    "go2_ts": _head("go2_ts", "Go2TS"),
    "go2_cts": _head("go2_cts", "Go2CTS"),
    "go2_dreamwaq": _head("go2_dreamwaq", "Go2Dreamwaq", ("obs", "priv", "feat", "explicit", "next_state", "rew", "reset", "extras")),
    "go2_cat": _head("go2_cat", "Go2CaT"),
    # the point-foot biped on the plane: base-class resets, 5-frame actor / critic stacks, `no_fly`.  Its module draws nothing itself.
    "tron1_pf": Gen("legged_gym.envs.tron1_pf.tron1_pf", "TRON1PF", "TRON1PFCfg", 16, 40, 51, _PLANE,
                    _BIPED_KEYS + ("sim_base_lin_vel_w", "dr") + _TAIL,
                    (tuple(range(6)),), _BIPED_CLOCKS, place=place_tron1_pf),     # legged_robot.py:279-280: one (n, 6) draw
    # 6-DOF biped, heightfield + curriculum, biped periodic gait, sit-pose resets (theta offset, gait time: torch.rand; the coin:
    # np.random.random), all domain randomisation incl. joint armature / friction / damping.  The env is constructed with the
    # original torch.rand.
    "tron1_pf_ee": Gen("legged_gym.envs.tron1_pf.tron1_pf_ee.tron1_pf_ee", "TRON1PF_EE", "TRON1PF_EECfg", 24, 48, 31, _EE,
                       ("actions_in", "rand", "counter", "feat_new", "priv_new", "labels", "rew", "reset", "time_out", "commands",
                        "ep_len", "fail_buf", "episode_sums", "act_hist", "sim_dof_pos", "sim_base_pos", "sim_base_quat") + _ROUGH_KEYS
                       + ("dr_joint", "task_state") + _TAIL,
                       ((0, 3), (1, 4), (2, 5)), _CLOCKS,                 # tron1_pf_ee.py:268-273
                       patch=("np.random.random",), patch_late=("torch.rand",), place=place_tron1_rough, big_action=30.0),
    # the 8-DOF sole-foot biped on the plane: 10-frame stacks, the batch-wide sit-pose coin, `hip_pos_zero_command` / `foot_flat`
    # (and `keep_ankle_pitch_zero_in_air`, which TaskSpec.reward_scales gives a scale so that it is pinned too)
    "tron1_sf": Gen("legged_gym.envs.tron1_sf.tron1_sf", "TRON1SF", "TRON1SFCfg", 16, 44, 61, _PLANE,
                    _BIPED_KEYS + ("sim_base_quat", "sim_base_lin_vel_w", "dr", "dr_pd", "dr_joint") + _TAIL,
                    ((0, 3), (1, 4), (2, 5), (3, 6)), _BIPED_CLOCKS,      # tron1_sf.py:224-231: the 6-DOF index pairs on the 8-DOF vector
                    patch=("np.random.random",), place=place_tron1_sf, commands=near_zero_commands),
}
assert list(GEN) == list(TASKS)


# ------------------------------------------------------------------------------------------------------------------------------
def _np(x):
    return x.numpy().copy()


def _u8(x):
    return x.numpy().astype(np.uint8)


def _cat(*xs):
    return np.concatenate([x.numpy() for x in xs], 1).copy()


def _task_state(s):
    """mdp_harness.TASK_STATE's columns from the env's attributes (the reference keeps exp_C_frc per foot), as the fixtures record them."""
    feet = GAIT[s.spec.gait][2]
    cols = [torch.zeros(s.N, w) if a is None else
            torch.cat([getattr(s.env, f"exp_C_frc_{f}") for f in feet], 1) if a == "exp_C_frc" else getattr(s.env, a)
            for a, w in TASK_STATE[s.spec.gait]]
    return recorded_task_state(s.spec.gait, _cat(*cols))


_CSTR = ("torque", "dof_vel", "action_rate", "base_height", "collision", "feet_stumble", "dof_pos", "base_orientation", "stand_still")

# fixture key -> its value for one step, from s: spec, g, env, sim, N, slots, names, and per step act, override, r (env.step()'s
# results by name) and calls.  sim_<x> is the fake simulator's _<x>.  last_*_in are read before the step, everything else after.
BEFORE_STEP = ("last_dof_vel_in", "last_feet_vel_in")       # what the kernel is given as "last" values for this step
READ = {
    "last_dof_vel_in": lambda s: _np(s.sim._dof_vel),
    "last_feet_vel_in": lambda s: _np(s.sim._feet_vel),
    "actions_in": lambda s: _np(s.act),
    "rand": lambda s: slots_from_calls(s.calls, s.slots, s.N, s.act.shape[1], s.g.groups),
    "counter": lambda s: s.env.common_step_counter,
    "esum_override": lambda s: s.override,
    "obs": lambda s: _np(s.r["obs"]),
    "priv": lambda s: _np(s.r["priv"]),
    "feat_new": lambda s: _np(s.r["feat"][:, -s.spec.frames[0]:]),
    "priv_new": lambda s: _np(s.r["priv"][:, -s.spec.frames[1]:]),
    "labels": lambda s: _np(s.r["labels"]),
    "rew": lambda s: _np(s.r["rew"]),
    "reset": lambda s: _u8(s.r["reset"]),
    "time_out": lambda s: _u8(s.env.time_out_buf),
    "commands": lambda s: _np(s.env.commands),
    "ep_len": lambda s: _np(s.env.episode_length_buf),
    "fail_buf": lambda s: _np(s.env.fail_buf),
    "feet_air_time": lambda s: _np(s.env.feet_air_time),
    "last_contacts": lambda s: _u8(s.env.last_contacts),
    "episode_sums": lambda s: np.stack([_np(s.env.episode_sums[n]) for n in s.names]),
    "act_hist": lambda s: np.stack([_np(s.env.actions), _np(s.env.last_actions), _np(s.env.llast_actions)]),
    "dr": lambda s: _cat(s.sim._friction_values, s.sim._added_base_mass, s.sim._base_com_bias, s.sim._rand_push_vels[:, :2]),
    "dr_pd": lambda s: _cat(s.sim._kp_scale, s.sim._kd_scale),
    "dr_joint": lambda s: _cat(s.sim._joint_armature, s.sim._joint_friction, s.sim._joint_damping),
    "cmd_range_x": lambda s: np.array(s.env.command_ranges["lin_vel_x"], np.float32),
    "task_state": _task_state,
    "terrain_levels": lambda s: _np(s.sim._terrain_levels),
    "env_origins": lambda s: _np(s.sim._env_origins),
    "measured_heights": lambda s: _np(s.sim._measured_heights),
    "height_around_feet": lambda s: _np(s.sim._height_around_feet),
    "normals": lambda s: _np(s.sim._normal_vector_around_feet),
    "contact_states": lambda s: _np(s.sim._link_contact_states),
    "cstr_prob": lambda s: _np(s.env.cstr_prob) if s.spec.cstr else np.zeros(s.N, np.float32),
    "cstr_sums": lambda s: np.stack([_np(s.env.episode_sums["cstr_" + n]) for n in _CSTR]) if s.spec.cstr else np.zeros((0, s.N), np.float32),
}


def read(s, key):
    return _np(getattr(s.sim, "_" + key[len("sim_"):])) if key.startswith("sim_") else READ[key](s)


PATCHABLE = {"torch.rand_like": (torch, "rand_like", "rand_like"), "torch.randint": (torch, "randint", "randint"),
             "torch.rand": (torch, "rand", "torch_rand"), "np.random.random": (np.random, "random", "np_random")}


@contextlib.contextmanager
def patched(rec, names, others=()):
    """Serve the PATCHABLE globals `names` from the recorder and set `others` ((object, attribute, value)); restore all on exit."""
    targets = [(obj, attr, getattr(rec, method)) for obj, attr, method in map(PATCHABLE.get, names)] + list(others)
    saved = [(obj, attr, getattr(obj, attr)) for obj, attr, _ in targets]
    for obj, attr, value in targets:
        setattr(obj, attr, value)
    try:
        yield
    finally:
        for obj, attr, value in saved:
            setattr(obj, attr, value)


def generate(name):
    """Run the reference's task class for TASKS[name] / GEN[name] on the fake simulator and save <name>_mdp.npz."""
    import legged_gym.envs.base.base_task as base_task
    import legged_gym.envs.base.legged_robot as lr_mod
    from legged_gym.utils.helpers import class_to_dict
    spec, g = TASKS[name], GEN[name]
    N, T = g.N, g.T
    mod = importlib.import_module(g.module)
    rec = rh.DrawRecorder(g.seed)
    # the base class's uniform source, and the task module's own copy of the name where it has one
    draws = [(m, "torch_rand_float", rec.rand_float) for m in (lr_mod, mod) if hasattr(m, "torch_rand_float")]
    with contextlib.ExitStack() as stack:
        stack.enter_context(patched(rec, ("torch.rand_like",) + g.patch,
                                    [(base_task, "GenesisSimulator", RoughFakeSimulator if spec.rough else FakeSimulator)] + draws))
        cfg = getattr(importlib.import_module(g.module + "_config"), g.cfg)()
        cfg.env.num_envs = N
        if hasattr(cfg.env, "num_teacher"):
            cfg.env.num_teacher = N // 4 * 3
        for k, v in spec.reward_scales:
            setattr(cfg.rewards.scales, k, v)
        env = getattr(mod, g.cls)(cfg, class_to_dict(cfg.sim), "cpu", True)
        stack.enter_context(patched(rec, g.patch_late))
        sim = env.simulator
        sim.rec = rec
        if spec.cstr:
            cat_limits(sim)
        rng = np.random.default_rng(g.seed + 1)
        script = make_script(rng, sim.model, cfg, N, T)
        if g.place:
            g.place(script, sim, rng)
        sim.script = script
        # initial MDP state: as after construction, with the episode clocks spread
        env.episode_length_buf[:] = torch.from_numpy(rng.choice(g.clocks, N).astype(np.int32))
        env.commands[:] = torch.from_numpy((rng.normal(size=(N, 4)) * [0.4, 0.4, 0.5, 1.5]).astype(np.float32))
        if g.commands:
            g.commands(env)
        env.common_step_counter = g.counter
        env.reset_buf[:] = 0
        env.extras.setdefault("episode", {})      # exists after the runner's env.reset(); go2_cts.py:96 / go2_cat.py:101 index it on every step
        init = dict(episode_length_buf=env.episode_length_buf, commands=env.commands, env_origins=sim._env_origins)
        if spec.go2:
            init["default_dof_pos"] = sim._default_dof_pos
        if spec.rough:
            init.update(terrain_levels=sim._terrain_levels, terrain_types=sim._terrain_types, height_points=sim._height_points[0, :, :2])
        if spec.gait:
            set_gait, gait_keys, _ = GAIT[spec.gait]
            set_gait(env, rng, N)
            init.update({k: getattr(env, k) for k in gait_keys})
        init = {k: _np(v) for k, v in init.items()}
        if spec.gait == "wtw":
            init["behavior_ranges"] = np.array(env.gait_period_range + env.base_height_target_range + env.foot_clearance_target_range +
                                               env.pitch_target_range + [env.num_gaits], np.float32)
        rec.take()
        s = types.SimpleNamespace(spec=spec, g=g, env=env, sim=sim, N=N, names=env.reward_names,
                                  slots=builders.make_task_cfg(sim.model, spec.cfg()).slots)
        out = {k: [] for k in g.keys}
        for t in range(T):
            s.override = go2_gate(env, t) if spec.go2 else 0.0
            s.act = torch.from_numpy((rng.normal(size=(N, cfg.env.num_actions)) * (1.0 if t % 7 else g.big_action)).astype(np.float32))
            for k in BEFORE_STEP:
                out[k].append(read(s, k))
            s.r = dict(zip(g.returns, env.step(s.act), strict=True))
            s.calls = rec.take()
            if "explicit" in s.r:                                         # go2_dreamwaq
                s.r["labels"] = torch.cat([s.r["explicit"], s.r["next_state"]], dim=-1)
            for k in g.keys:
                if k not in BEFORE_STEP:
                    out[k].append(read(s, k))
        arrays = {k: np.stack(v) for k, v in out.items()}
        if spec.stacks:
            arrays["feat_last"], arrays["priv_last"] = _np(s.r["feat"]), _np(s.r["priv"])
        arrays.update({"script_" + k: v for k, v in sim.script.items()})
        arrays.update({"init_" + k: v for k, v in init.items()})
        arrays["reward_names"] = np.array(s.names)
        if spec.rough:
            arrays["terrain_seed"] = RoughFakeSimulator.TERRAIN_SEED
        moved = ("levels moved", int((arrays["terrain_levels"][-1] != init["terrain_levels"]).sum())) if spec.rough else ()
        rh.save(f"{name}_mdp", arrays, "resets/step", arrays["reset"].sum(1), *moved)


if __name__ == "__main__":
    for task in sys.argv[1:] or TASKS:
        generate(task)

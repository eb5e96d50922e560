"""ctypes mirror of include/lgsim.h, include/lgrollout.h, include/lgsensor.h, include/lgpolicy.h, include/lgppo.h, include/lgoptim.h, include/lgtrain.h, include/lgtrainee.h, include/lgtraints.h, include/lgtraintcn.h and include/lgrunner.h (the C ABI) and the loader of the HIP library.

Field order and types must match the header exactly; tests/test_abi.py compiles a C
probe that prints sizeof/offsetof for every struct and compares them with these classes.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

MAX_JPL = 4
MAX_LEGS = 4
MAX_DOF = 12
MAX_BODIES = 13
MAX_LINKS = 24
MAX_SPHERES = 64
MAX_OBS = 192
NUM_REWARDS = 40
CMD_RANGE_FLOATS = 24
TASK_STATE_WTW = 22
TASK_STATE_BIPED = 12

PHASE_PRE, PHASE_SIM, PHASE_POST, PHASE_RESET, PHASE_ALL = 1, 2, 4, 8, 15
FAIL_NONFINITE = 1 << 20      # LG_FAIL_NONFINITE

# alphabetical evaluation order of the reference (helpers.py:10-25); index = enum LgReward
REWARD_NAMES = [
    "action_rate", "action_smoothness", "ang_vel_xy", "base_height", "biped_periodic_gait",
    "collision", "dof_acc", "dof_close_to_default", "dof_pos_limits", "dof_pos_stand_still",
    "dof_power", "dof_vel", "dof_vel_stand_still", "feet_air_time", "feet_contact_stand_still",
    "feet_distance", "foot_acc", "foot_clearance", "foot_landing_vel", "hip_pos", "keep_balance",
    "lin_vel_z", "no_fly", "orientation", "quad_periodic_gait", "torques", "tracking_ang_vel",
    "tracking_base_height", "tracking_foot_clearance", "tracking_lin_vel", "tracking_orientation",
    "termination",
]
R_COUNT = len(REWARD_NAMES)
REWARD_ID = {n: i for i, n in enumerate(REWARD_NAMES)}
# terms of the 4-joint sole-foot biped (tron1_sf.py:281-308) share the ids of quadruped-only terms (include/lgsim.h LG_R_FOOT_FLAT ...)
REWARD_ALIASES_JPL4 = {"hip_pos_zero_command": "hip_pos", "foot_flat": "quad_periodic_gait", "keep_ankle_pitch_zero_in_air": "tracking_foot_clearance"}


def reward_id(name, joints_per_leg=3):
    """enum LgReward value of a reward-scale name for a robot with that many joints per leg."""
    if joints_per_leg == 4 and name in REWARD_ALIASES_JPL4:
        return REWARD_ID[REWARD_ALIASES_JPL4[name]]
    if joints_per_leg == 4 and name in REWARD_ALIASES_JPL4.values():
        raise KeyError(f"reward term {name} does not exist for four-joint legs")
    return REWARD_ID[name]


def reward_names(joints_per_leg=3):
    """Names by enum LgReward value as they read for that robot (episode-sum keys)."""
    inv = {v: k for k, v in REWARD_ALIASES_JPL4.items()} if joints_per_leg == 4 else {}
    return [inv.get(n, n) for n in REWARD_NAMES]
OBS_GO2, OBS_GO2_WTW, OBS_GO2_EE, OBS_TRON1_EE, OBS_PROGRAM = 0, 1, 2, 3, 4

f32, i32, u32, i64, u64 = C.c_float, C.c_int32, C.c_uint32, C.c_int64, C.c_uint64
fp = C.POINTER(C.c_float)


class LgModelDesc(C.Structure):
    _fields_ = [
        ("n_legs", i32), ("n_bodies", i32), ("n_links", i32), ("n_spheres", i32),
        ("mass", f32 * MAX_BODIES), ("com", f32 * 3 * MAX_BODIES), ("inertia", f32 * 6 * MAX_BODIES),
        ("jpos", f32 * 3 * MAX_BODIES), ("jrot", f32 * 9 * MAX_BODIES), ("axis", f32 * 3 * MAX_BODIES),
        ("q_lo", f32 * MAX_DOF), ("q_hi", f32 * MAX_DOF), ("effort", f32 * MAX_DOF), ("vel_limit", f32 * MAX_DOF),
        ("armature", f32 * MAX_DOF), ("damping", f32 * MAX_DOF), ("frictionloss", f32 * MAX_DOF),
        ("link_body", i32 * MAX_LINKS), ("link_pos", f32 * 3 * MAX_LINKS),
        ("sph_body", i32 * MAX_SPHERES), ("sph_link", i32 * MAX_SPHERES),
        ("sph_pos", f32 * 3 * MAX_SPHERES), ("sph_r", f32 * MAX_SPHERES), ("sph_w", f32 * MAX_SPHERES),
        ("body_sph_start", i32 * (MAX_BODIES + 1)),
        ("foot_link", i32 * MAX_LEGS), ("foot_sphere", i32 * MAX_LEGS),
        ("term_link_mask", u32), ("pen_link_mask", u32), ("state_link_mask", u32),
    ]


class LgSimOptions(C.Structure):
    _fields_ = [
        ("dt", f32), ("decimation", i32), ("gravity_z", f32), ("contact_k", f32), ("contact_b", f32),
        ("terrain_friction", f32), ("limit_k", f32), ("limit_b", f32), ("contact_iters", i32), ("contact_margin", f32), ("limit_margin", f32),
        ("max_base_lin_vel", f32), ("max_base_ang_vel", f32), ("joint_vel_clamp", f32), ("action_scale", f32),
        ("kp", f32 * MAX_DOF), ("kd", f32 * MAX_DOF), ("default_dof_pos", f32 * MAX_DOF),
        ("base_init_pos", f32 * 3), ("bound_x", f32 * 2), ("bound_y", f32 * 2),
        ("terrain_rows", i32), ("terrain_cols", i32), ("hscale", f32), ("vscale", f32), ("border", f32),
        ("n_height_points", i32), ("feet_terrain_info", i32), ("sim_layout", i32), ("contact_w_every", i32),
    ]


class LgRandSlots(C.Structure):
    _fields_ = [(n, i32) for n in (
        "n_slots", "cb_cmd", "push", "reset_cmd", "reset_dof", "reset_root_xy", "reset_lin_vel",
        "reset_ang_vel", "dr_friction", "dr_mass", "dr_com", "dr_kp", "dr_kd", "dr_joint",
        "terrain_level", "task_cb", "task_reset", "noise")]


MAX_SEGS = 8
NUM_CSTR = 9
CR_ANY_FAST = 17
CSTR_NAMES = ["torque", "dof_vel", "action_rate", "base_height", "collision", "feet_stumble", "dof_pos", "base_orientation", "stand_still"]
(SEG_END, SEG_FRAME, SEG_DR, SEG_DR_JOINT, SEG_BASE_LIN_VEL, SEG_CONTACT_STATES, SEG_HEIGHTS, SEG_FEET_REL_HEIGHTS,
 SEG_FEET_HEIGHTS, SEG_FEET_NORMALS, SEG_FOOT_CLEARANCE, SEG_NEXT_STATE, SEG_LAST_ACTIONS, SEG_DR_BASE, SEG_FEET_AIR_TIME, SEG_KP,
 SEG_KD) = range(17)


class LgObsProgram(C.Structure):
    _fields_ = [("n_segs", i32), ("clip", i32), ("kind", i32 * MAX_SEGS), ("offset", i32 * MAX_SEGS), ("scale", f32 * MAX_SEGS)]


class LgTaskCfg(C.Structure):
    _fields_ = [
        ("obs_layout", i32), ("num_obs", i32), ("num_priv_obs", i32), ("obs_frame", i32), ("priv_frame", i32),
        ("obs_stack", i32), ("priv_stack", i32), ("obs_slack", i32), ("obs_sets", i32),
        ("control_dt", f32), ("clip_actions", f32), ("clip_obs", f32), ("max_episode_length", f32),
        ("fail_threshold", f32), ("max_projected_gravity", f32),
        ("resample_steps", i32), ("push_interval", i32), ("max_push_vel_xy", f32), ("heading_command", i32),
        ("yaw_clip", f32 * 2),
        ("reward_scales", f32 * NUM_REWARDS), ("soft_dof_lo", f32 * MAX_DOF), ("soft_dof_hi", f32 * MAX_DOF),
        ("only_positive_rewards", i32),
        ("tracking_sigma", f32), ("base_height_target", f32), ("foot_clearance_target", f32),
        ("foot_height_offset", f32), ("foot_clearance_sigma", f32), ("about_landing_threshold", f32),
        ("feet_air_time_threshold", f32), ("base_height_sigma", f32), ("euler_sigma", f32),
        ("foot_distance_threshold", f32), ("no_fly_contact_threshold", f32), ("air_time_cmd_dims", i32), ("foot_clearance_ref", i32),
        ("obs_scale_lin_vel", f32), ("obs_scale_ang_vel", f32), ("obs_scale_dof_pos", f32),
        ("obs_scale_dof_vel", f32), ("obs_scale_height", f32),
        ("add_noise", i32), ("noise_vec", f32 * MAX_OBS),
        ("reset_dof_lo", f32 * MAX_DOF), ("reset_dof_span", f32 * MAX_DOF),
        ("reset_root_xy_lo", f32), ("reset_root_xy_span", f32), ("custom_origins", i32),
        ("reset_lin_vel_lo", f32), ("reset_lin_vel_span", f32), ("reset_ang_vel_lo", f32), ("reset_ang_vel_span", f32),
        ("base_init_quat", f32 * 4),
        ("dr_friction_on", i32), ("dr_mass_on", i32), ("dr_com_on", i32), ("dr_pd_on", i32), ("dr_joint_on", i32),
        ("dr_friction_lo", f32), ("dr_friction_span", f32), ("dr_mass_lo", f32), ("dr_mass_span", f32),
        ("dr_com_lo", f32 * 3), ("dr_com_span", f32 * 3),
        ("dr_kp_lo", f32), ("dr_kp_span", f32), ("dr_kd_lo", f32), ("dr_kd_span", f32),
        ("dr_joint_lo", f32 * 3), ("dr_joint_span", f32 * 3),
        ("friction_offset", f32), ("kp_offset", f32), ("kd_offset", f32),
        ("terrain_curriculum", i32), ("max_terrain_level", i32), ("terrain_cols_n", i32),
        ("num_labels", i32), ("heights_offset", f32), ("heights_clip_scale", i32),
        ("terrain_env_length", f32), ("episode_length_s", f32),
        ("gait_mode", i32), ("double_shift", i32), ("behavior_resample_steps", i32), ("num_gait_max", i32),
        ("b_swing", f32), ("gait_period_fixed", f32), ("theta_table", f32 * 4 * 4),
        ("sit_percent", f32), ("sit_pos", f32 * 3), ("sit_quat", f32 * 4), ("sit_dof_pos", f32 * MAX_DOF),
        ("task_state_width", i32),
        ("priv_prog", LgObsProgram), ("labels_prog", LgObsProgram),
        ("cat_enable", i32), ("cat_soft_p", f32), ("cat_action_rate", f32), ("cat_min_base_height", f32),
        ("cat_max_projected_gravity", f32), ("dof_vel_limits", f32 * MAX_DOF),
        ("slots", LgRandSlots), ("seed", u64), ("env_id_offset", i64),
    ]


_BUF_FIELDS = [
    ("n_envs", i32),
    *[(n, C.c_void_p) for n in (
        "base_pos", "base_quat", "base_lin_vel_w", "base_ang_vel_w", "dof_pos", "dof_vel",
        "friction_values", "added_base_mass", "base_com_bias", "kp_scale", "kd_scale",
        "joint_armature", "joint_friction", "joint_damping", "rand_push_vels", "env_origins",
        "base_lin_vel", "base_ang_vel", "projected_gravity", "base_euler",
        "last_base_lin_vel", "last_base_ang_vel", "last_dof_vel", "last_feet_vel",
        "torques", "link_contact_forces", "feet_pos", "feet_vel",
        "link_contact_states", "measured_heights", "height_around_feet", "normal_vector_around_feet",
        "height_points", "terrain_levels", "terrain_types", "terrain_origins",
        "actions", "last_actions", "llast_actions", "commands",
        "feet_air_time", "last_contacts", "episode_length_buf", "fail_buf",
        "reset_buf", "time_out_buf",
        "rew_buf", "obs_buf", "priv_obs_buf", "labels_buf", "obs_dirty",
        "episode_sums", "episode_done_sums", "episode_done_step", "cstr_prob", "cstr_sums", "cstr_done_sums",
        "command_ranges", "task_state", "rand_in", "nonfinite_count")],
]


class LgBuffers(C.Structure):
    _fields_ = _BUF_FIELDS


BUFFER_NAMES = [n for n, _ in _BUF_FIELDS[1:]]


def fill_array(dst, src):
    """Copy a numpy array into a (possibly nested) ctypes array field."""
    a = np.ascontiguousarray(np.asarray(src)).reshape(-1)
    n = C.sizeof(dst) // 4
    if a.size > n:
        raise ValueError(f"array of {a.size} does not fit field of {n}")
    leaf = _leaf_type(type(dst))
    np_t = np.float32 if leaf is C.c_float else (np.uint32 if leaf is C.c_uint32 else np.int32)
    buf = np.zeros(n, dtype=np_t)
    buf[:a.size] = a.astype(np_t)
    C.memmove(dst, buf.ctypes.data, n * 4)


def _leaf_type(t):
    while hasattr(t, "_type_") and not isinstance(t._type_, str):
        t = t._type_
    return t


def model_desc(model, term_links=(), pen_links=(), state_links=()):
    """Pack a RobotModel (model_compiler.py) into LgModelDesc."""
    a = model.arrays
    d = LgModelDesc()
    d.n_legs, d.n_bodies = int(a["n_legs"]), int(a["n_bodies"])
    d.n_links, d.n_spheres = int(a["n_links"]), int(a["n_spheres"])
    for k in ("mass", "com", "inertia", "jpos", "jrot", "axis", "q_lo", "q_hi", "effort", "vel_limit", "armature",
              "damping", "frictionloss", "link_body", "link_pos", "sph_body", "sph_link", "sph_pos",
              "sph_r", "sph_w", "body_sph_start", "foot_link", "foot_sphere"):
        fill_array(getattr(d, k), a[k])
    mask = lambda ids: int(sum(1 << int(i) for i in ids))
    d.term_link_mask, d.pen_link_mask, d.state_link_mask = mask(term_links), mask(pen_links), mask(state_links)
    return d


_LIB = None
LIB_NAME = "liblgsim.so"


class HipExtensionMissing(RuntimeError):
    pass


def lib_path():
    # LG_LIB lets a developer point at an experimental build of the same ABI (still a HIP library, never a fallback)
    return os.environ.get("LG_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", LIB_NAME)


def load_lib():
    """dlopen the HIP engine.  There is no CPU fallback: a missing library is an error."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise HipExtensionMissing(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). The product path has no CPU fallback.")
    lib = C.CDLL(p)
    H = C.c_void_p
    lib.lg_create.argtypes = [C.POINTER(LgModelDesc), C.POINTER(LgSimOptions), C.POINTER(LgTaskCfg), C.POINTER(H)]
    lib.lg_destroy.argtypes = [H]
    lib.lg_set_task.argtypes = [H, C.POINTER(LgTaskCfg)]
    lib.lg_set_terrain.argtypes = [H, C.c_void_p, i32, i32]
    lib.lg_bind.argtypes = [H, C.POINTER(LgBuffers)]
    lib.lg_step.argtypes = [H, u32, C.c_void_p, i64, C.c_void_p]
    lib.lg_time_steps.argtypes = [H, C.c_void_p, i64, i32, C.c_void_p, C.POINTER(C.c_float)]
    lib.lg_obs_window.argtypes = [H, C.POINTER(i32)]
    lib.lg_obs_set.argtypes = [H, C.POINTER(i32)]
    lib.lg_obs_set_select.argtypes = [H, i32]
    lib.lg_obs_window_select.argtypes = [H, i32]
    lib.lg_profile.argtypes = [H, i32]
    lib.lg_profile_read.argtypes = [H, C.POINTER(C.c_float), C.POINTER(i32)]
    lib.lg_philox.argtypes = [C.POINTER(u32 * 4), C.POINTER(u32 * 2), C.POINTER(u32 * 4)]
    lib.lg_philox.restype = C.c_int
    lib.lg_dpp_kat.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.lg_dpp_kat.restype = C.c_int
    lib.lg_dpp_kat_cases.argtypes = []
    lib.lg_dpp_kat_cases.restype = C.c_int
    lib.lg_dpp_kat_run.argtypes = [C.c_void_p, C.c_void_p, i32, i32, C.c_void_p, C.c_void_p]
    lib.lg_dpp_kat_run.restype = C.c_int
    lib.lg_stream_copy.argtypes = [C.c_void_p, C.c_void_p, i64, i32, C.c_void_p, C.POINTER(C.c_float)]
    lib.lg_stream_copy.restype = C.c_int
    lib.lg_terrain_generate.argtypes = [C.c_void_p, i32, C.c_void_p, C.c_void_p, C.c_void_p, i32, i32, i32, i32, i32, i32, C.c_double, C.c_void_p, C.c_void_p]
    lib.lg_terrain_generate.restype = C.c_int
    if hasattr(lib, "lg_terrain_max_kind"):      # absent from libraries older than the stepping-stone / gap / pit / wave tiles
        lib.lg_terrain_max_kind.argtypes = []
        lib.lg_terrain_max_kind.restype = C.c_int
    lib.lg_rollout_record.argtypes = [i32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, f32, C.c_void_p, C.c_void_p,
                                      C.POINTER(LgRowCopy), i32, C.c_void_p]
    lib.lg_rollout_gae.argtypes = [i32, i32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, f32, f32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]
    lib.lg_rollout_record.restype = lib.lg_rollout_gae.restype = C.c_int
    vp = C.c_void_p
    lib.lg_rollout_traj_index.argtypes = [i32, i32, vp, vp, vp, i32, vp, vp]
    lib.lg_rollout_mask_index.argtypes = [i32, i32, vp, vp, i32, vp, vp]
    lib.lg_rollout_pad.argtypes = [i32, i32, vp, i32, i32, i32, C.POINTER(LgRowCopy), i32, C.POINTER(LgRowCopy), C.POINTER(i32), i32, vp, vp]
    lib.lg_rollout_unpad.argtypes = [i32, i32, vp, i32, i32, i32, vp, vp, i32, vp]
    lib.lg_rollout_gather.argtypes = [C.POINTER(LgGatherItem), i32, vp]
    lib.lg_rollout_gae_groups.argtypes = [i32, i32, i32, vp, vp, vp, vp, f32, f32, vp, vp, vp, vp, vp]
    for f in ROLLOUT_EXPORTS[2:]:
        getattr(lib, f).restype = C.c_int
    lib.lg_depth_render.argtypes = [C.POINTER(LgDepthCam), C.POINTER(LgDepthScene), vp, vp, vp]
    lib.lg_depth_render.restype = C.c_int
    lib.lg_policy_act.argtypes = [C.POINTER(LgPolicyArgs), vp]
    lib.lg_policy_row_tile.argtypes = [C.POINTER(LgPolicyArgs)]
    lib.lg_policy_act_recurrent.argtypes = [C.POINTER(LgPolicyRecurrentArgs), vp]
    lib.lg_policy_row_tile_recurrent.argtypes = [C.POINTER(LgPolicyRecurrentArgs)]
    lib.lg_policy_reset.argtypes = [C.POINTER(LgPolicyRecurrentArgs), vp, vp]
    for f in POLICY_EXPORTS:
        getattr(lib, f).restype = C.c_int
    if hasattr(lib, "lg_ppo_loss"):              # absent from libraries older than the fused PPO loss head
        lib.lg_ppo_loss.argtypes = [C.POINTER(LgPpoLossArgs), vp]
        lib.lg_ppo_loss_workspace.argtypes = [C.POINTER(LgPpoLossArgs)]
        for f in PPO_EXPORTS:
            getattr(lib, f).restype = C.c_int
    if hasattr(lib, "lg_adam_step"):             # absent from libraries older than the fused optimizer step
        lib.lg_adam_step.argtypes = [C.POINTER(LgAdamArgs), vp]
        lib.lg_adam_workspace.argtypes = [C.POINTER(LgAdamArgs)]
        for f in OPTIM_EXPORTS:
            getattr(lib, f).restype = C.c_int
    if hasattr(lib, "lg_train_forward"):         # absent from libraries older than the fused learner pass
        lib.lg_train_plan.argtypes = [C.POINTER(LgTrainArgs), C.POINTER(LgTrainPlan)]
        lib.lg_train_forward.argtypes = [C.POINTER(LgTrainArgs), vp]
        lib.lg_train_backward.argtypes = [C.POINTER(LgTrainArgs), vp]
        for f in TRAIN_EXPORTS:
            getattr(lib, f).restype = C.c_int
    if hasattr(lib, "lg_train_ee_forward"):      # absent from libraries older than the explicit-estimator learner passes
        lib.lg_train_ee_plan.argtypes = [C.POINTER(LgTrainEEArgs), C.POINTER(LgTrainEEPlan)]
        lib.lg_train_ee_forward.argtypes = [C.POINTER(LgTrainEEArgs), vp]
        lib.lg_train_ee_backward.argtypes = [C.POINTER(LgTrainEEArgs), vp]
        lib.lg_train_est_plan.argtypes = [C.POINTER(LgTrainEstArgs), C.POINTER(LgTrainEEPlan)]
        lib.lg_train_est_forward.argtypes = [C.POINTER(LgTrainEstArgs), vp]
        lib.lg_train_est_backward.argtypes = [C.POINTER(LgTrainEstArgs), vp]
        for f in TRAIN_EE_EXPORTS:
            getattr(lib, f).restype = C.c_int
    if hasattr(lib, "lg_train_ts_forward"):      # absent from libraries older than the teacher-student learner passes
        lib.lg_train_ts_plan.argtypes = [C.POINTER(LgTrainTSArgs), C.POINTER(LgTrainTSPlan)]
        lib.lg_train_ts_forward.argtypes = [C.POINTER(LgTrainTSArgs), vp]
        lib.lg_train_ts_backward.argtypes = [C.POINTER(LgTrainTSArgs), vp]
        lib.lg_train_enc_plan.argtypes = [C.POINTER(LgTrainEncArgs), C.POINTER(LgTrainTSPlan)]
        lib.lg_train_enc_forward.argtypes = [C.POINTER(LgTrainEncArgs), vp]
        lib.lg_train_enc_backward.argtypes = [C.POINTER(LgTrainEncArgs), vp]
    if hasattr(lib, "lg_train_dwaq_forward"):    # absent from libraries older than the DreamWaQ learner passes
        lib.lg_train_dwaq_plan.argtypes = [C.POINTER(LgTrainDwaqArgs), C.POINTER(LgTrainDwaqPlan)]
        lib.lg_train_dwaq_forward.argtypes = [C.POINTER(LgTrainDwaqArgs), vp]
        lib.lg_train_dwaq_backward.argtypes = [C.POINTER(LgTrainDwaqArgs), vp]
        lib.lg_train_vae_plan.argtypes = [C.POINTER(LgTrainVaeArgs), C.POINTER(LgTrainDwaqPlan)]
        lib.lg_train_vae_forward.argtypes = [C.POINTER(LgTrainVaeArgs), vp]
        lib.lg_train_vae_backward.argtypes = [C.POINTER(LgTrainVaeArgs), vp]
        for f in TRAIN_TS_EXPORTS:
            getattr(lib, f).restype = C.c_int
    if hasattr(lib, "lg_train_cts_forward"):     # absent from libraries older than the concurrent teacher-student learner pass
        lib.lg_train_cts_plan.argtypes = [C.POINTER(LgTrainCTSArgs), C.POINTER(LgTrainCTSPlan)]
        lib.lg_train_cts_forward.argtypes = [C.POINTER(LgTrainCTSArgs), vp]
        lib.lg_train_cts_backward.argtypes = [C.POINTER(LgTrainCTSArgs), vp]
        for f in TRAIN_CTS_EXPORTS:
            getattr(lib, f).restype = C.c_int
    if hasattr(lib, "lg_train_rnn_forward"):     # absent from libraries older than the recurrent learner pass
        lib.lg_train_rnn_plan.argtypes = [C.POINTER(LgTrainRnnArgs), C.POINTER(LgTrainRnnPlan)]
        lib.lg_train_rnn_forward.argtypes = [C.POINTER(LgTrainRnnArgs), vp]
        lib.lg_train_rnn_backward.argtypes = [C.POINTER(LgTrainRnnArgs), vp]
        for f in TRAIN_RNN_EXPORTS:
            getattr(lib, f).restype = C.c_int
    if hasattr(lib, "lg_train_tcn_forward"):     # absent from libraries older than the TCN history-encoder pass
        lib.lg_train_tcn_plan.argtypes = [C.POINTER(LgTrainTcnArgs), C.POINTER(LgTrainTcnPlan)]
        lib.lg_train_tcn_forward.argtypes = [C.POINTER(LgTrainTcnArgs), vp]
        lib.lg_train_tcn_backward.argtypes = [C.POINTER(LgTrainTcnArgs), vp]
        for f in TRAIN_TCN_EXPORTS:
            getattr(lib, f).restype = C.c_int
    if hasattr(lib, "lg_runner_episode_stats"):  # absent from libraries older than the runner's book-keeping kernels
        lib.lg_runner_episode_stats.argtypes = [i32, vp, vp, vp, vp, vp, vp, i32, vp, vp]
        lib.lg_runner_episode_info.argtypes = [i32, i32, vp, i32, i32, vp, i32, vp, i32, C.c_double, vp, vp, vp, vp]
        for f in RUNNER_EXPORTS:
            getattr(lib, f).restype = C.c_int
    lib.lg_last_error.restype = C.c_char_p
    lib.lg_last_kernel.argtypes = [H]
    lib.lg_last_kernel.restype = C.c_char_p
    lib.lg_abi_version.restype = C.c_int
    for f in ("lg_create", "lg_destroy", "lg_set_task", "lg_set_terrain", "lg_bind", "lg_step", "lg_time_steps", "lg_obs_window", "lg_obs_set", "lg_obs_set_select", "lg_obs_window_select", "lg_profile",
              "lg_profile_read"):
        getattr(lib, f).restype = C.c_int
    _LIB = lib
    return lib


EXPORTS = ["lg_create", "lg_destroy", "lg_set_task", "lg_set_terrain", "lg_bind", "lg_step",
           "lg_time_steps", "lg_obs_window", "lg_obs_set", "lg_obs_set_select", "lg_obs_window_select", "lg_profile", "lg_profile_read", "lg_philox", "lg_dpp_kat", "lg_dpp_kat_cases", "lg_dpp_kat_run", "lg_stream_copy", "lg_terrain_generate", "lg_terrain_max_kind", "lg_last_kernel", "lg_last_error",
           "lg_abi_version"]
ROLLOUT_EXPORTS = ["lg_rollout_record", "lg_rollout_gae", "lg_rollout_traj_index", "lg_rollout_mask_index", "lg_rollout_pad",
                   "lg_rollout_unpad", "lg_rollout_gather", "lg_rollout_gae_groups"]          # include/lgrollout.h
SENSOR_EXPORTS = ["lg_depth_render"]                                                          # include/lgsensor.h
POLICY_EXPORTS = ["lg_policy_act", "lg_policy_row_tile", "lg_policy_act_recurrent", "lg_policy_row_tile_recurrent", "lg_policy_reset"]   # include/lgpolicy.h
PPO_EXPORTS = ["lg_ppo_loss", "lg_ppo_loss_workspace"]                                        # include/lgppo.h
PPO_MAX_ACTIONS, PPO_MAX_GROUPS = 64, 2
PPO_CLIPPED_VALUE, PPO_SPO = 1, 2
PPO_THREADS, PPO_MAX_BLOCKS, PPO_PARTIAL_SLOTS = 256, 512, 6
PPO_R_LOSS, PPO_R_SURROGATE, PPO_R_VALUE, PPO_R_ENTROPY, PPO_R_KL, PPO_RESULT_FLOATS = 0, 1, 3, 4, 5, 8
OPTIM_EXPORTS = ["lg_adam_step", "lg_adam_workspace"]                                         # include/lgoptim.h
ADAM_MAX_TENSORS = 64
ADAM_CLIP, ADAM_KL_RULE = 1, 2
ADAM_CHUNK, ADAM_THREADS, ADAM_MAX_BLOCKS = 1024, 256, 512
ADAM_STATE_DOUBLES, ADAM_S_LR, ADAM_S_STEP = 2, 0, 1
ADAM_RESULT_FLOATS, ADAM_R_GRAD_NORM, ADAM_R_CLIP_COEF, ADAM_R_LR, ADAM_R_STEP = 4, 0, 1, 2, 3
TRAIN_EXPORTS = ["lg_train_plan", "lg_train_forward", "lg_train_backward"]                    # include/lgtrain.h
TRAIN_CHAINS, TRAIN_ACTOR, TRAIN_CRITIC = 2, 0, 1
TRAIN_WG_TILE, TRAIN_MIN_SLICE_ROWS, TRAIN_TARGET_JOBS, TRAIN_MAX_SLICES = 64, 64, 512, 32
TRAIN_EE_EXPORTS = ["lg_train_ee_plan", "lg_train_est_plan", "lg_train_ee_forward", "lg_train_ee_backward", "lg_train_est_forward",
                    "lg_train_est_backward"]                                                  # include/lgtrainee.h
TRAIN_EE_CHAINS, TRAIN_EE_ESTIMATOR, TRAIN_EE_ACTOR, TRAIN_EE_CRITIC, TRAIN_EE_THREADS = 3, 0, 1, 2, 256
TRAIN_EE_TARGET_JOBS = 2048
TRAIN_TS_EXPORTS = ["lg_train_ts_plan", "lg_train_enc_plan", "lg_train_ts_forward", "lg_train_ts_backward", "lg_train_enc_forward",
                    "lg_train_enc_backward"]                                                  # include/lgtraints.h
TRAIN_TS_CHAINS, TRAIN_TS_PRIVILEGE, TRAIN_TS_ACTOR, TRAIN_TS_CRITIC, TRAIN_TS_HISTORY, TRAIN_TS_RL_CHAINS = 4, 0, 1, 2, 3, 3
TRAIN_ENC_CHAINS, TRAIN_ENC_HISTORY, TRAIN_ENC_PRIVILEGE = 2, 0, 1
TRAIN_TS_TARGET_JOBS, TRAIN_TS_THREADS = 2048, 256
TRAIN_DWAQ_EXPORTS = ["lg_train_dwaq_plan", "lg_train_vae_plan", "lg_train_dwaq_forward", "lg_train_dwaq_backward", "lg_train_vae_forward",
                      "lg_train_vae_backward"]                                                # include/lgtraindwaq.h
TRAIN_DWAQ_CHAINS, TRAIN_DWAQ_ENCODER, TRAIN_DWAQ_LATENT_MU, TRAIN_DWAQ_LATENT_VAR, TRAIN_DWAQ_VEL_MU, TRAIN_DWAQ_VEL_VAR = 7, 0, 1, 2, 3, 4
TRAIN_DWAQ_ACTOR, TRAIN_DWAQ_CRITIC, TRAIN_DWAQ_HEADS, TRAIN_VAE_CHAINS, TRAIN_VAE_DECODER, TRAIN_VAE_LOSSES = 5, 6, 4, 6, 5, 4
TRAIN_DWAQ_TARGET_JOBS, TRAIN_DWAQ_THREADS = 2048, 256
TRAIN_CTS_EXPORTS = ["lg_train_cts_plan", "lg_train_cts_forward", "lg_train_cts_backward"]   # include/lgtraincts.h
TRAIN_CTS_CHAINS, TRAIN_CTS_PRIVILEGE, TRAIN_CTS_ACTOR, TRAIN_CTS_CRITIC, TRAIN_CTS_HISTORY = 4, 0, 1, 2, 3
TRAIN_CTS_GROUPS, TRAIN_CTS_TEACHER, TRAIN_CTS_STUDENT, TRAIN_CTS_ROLES, TRAIN_CTS_ROLE_CRITIC = 2, 0, 1, 3, 2
TRAIN_RNN_EXPORTS = ["lg_train_rnn_plan", "lg_train_rnn_forward", "lg_train_rnn_backward"]   # include/lgtrainrnn.h
TRAIN_RNN_MEMORIES, TRAIN_RNN_MAX_LAYERS, TRAIN_RNN_MAX_HIDDEN, TRAIN_RNN_LSTM, TRAIN_RNN_GRU, TRAIN_RNN_TARGET_JOBS = 2, 2, 512, 1, 2, 2048
TRAIN_TCN_EXPORTS = ["lg_train_tcn_plan", "lg_train_tcn_forward", "lg_train_tcn_backward"]   # include/lgtraintcn.h
TRAIN_TCN_MAX_CONV, TRAIN_TCN_MAX_CHANNELS, TRAIN_TCN_MAX_KERNEL, TRAIN_TCN_MAX_STRIDE, TRAIN_TCN_MAX_DILATION = 6, 32, 9, 4, 8
TRAIN_TCN_TARGET_JOBS, TRAIN_TCN_THREADS, TRAIN_TCN_WG_ELEMS, TRAIN_TCN_MAX_BLOCKS = 2048, 256, 8, 2048
RUNNER_EXPORTS = ["lg_runner_episode_stats", "lg_runner_episode_info"]                       # include/lgrunner.h
RUNNER_THREADS, RUNNER_INFO_THREADS, RUNNER_MAX_ROWS = 1024, 256, 1024
# argument types by entry point, in the header's order (tests/test_runner_host.py compares them with the prototypes)
RUNNER_SIGNATURES = {
    "lg_runner_episode_stats": ("int32_t", "const float *", "const uint8_t *", "float *", "float *", "float *", "float *", "int32_t", "int64_t *", "void *"),
    "lg_runner_episode_info": ("int32_t", "int32_t", "const float *", "int32_t", "int32_t", "const float *", "int32_t", "const int32_t *", "int32_t",
                               "double", "double *", "double *", "int64_t *", "void *"),
}
POLICY_MAX_LAYERS, POLICY_MAX_WIDTH = 4, 2048
POLICY_MAX_RNN_LAYERS, POLICY_MAX_RNN_HIDDEN = 2, 512
POLICY_LSTM, POLICY_GRU = 1, 2
POLICY_DETERMINISTIC, POLICY_VALUES_ONLY = 1, 2
POLICY_STREAM_TAG = 0x504F4C49
POLICY_LATENT_TAG = 0x4C41544E
DEPTH_MAX_CELLS = 4096
ROLLOUT_MAX_COPIES = 8
ROLLOUT_MAX_GATHER = 16
GATHER_F32, GATHER_NOT_U8 = 0, 1


TILE_SLOPE, TILE_UNIFORM, TILE_STAIRS, TILE_OBSTACLES = 0, 1, 2, 3
TILE_STONES, TILE_GAP, TILE_PIT, TILE_WAVE = 4, 5, 6, 7
TILE_IAUX_KINDS = (TILE_OBSTACLES, TILE_STONES)      # aux_off indexes iaux (ints) for these, aux (doubles) for the others


class LgTerrainTile(C.Structure):
    _fields_ = [("kind", i32), ("row", i32), ("col", i32), ("ip", i32 * 5), ("aux_off", i32)]


class LgRowCopy(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("width", i32), ("src_stride", i32)]


class LgGatherItem(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("index", C.c_void_p), ("rows", i32), ("width", i32), ("src_stride", i32),
                ("kind", i32), ("group", i32), ("env_offset", i32), ("n_envs", i32)]


class LgDepthCam(C.Structure):
    _fields_ = [("width", i32), ("height", i32), ("mount_pos", f32 * 3), ("mount_quat", f32 * 4), ("min_range", f32), ("max_range", f32),
                ("near_clip", f32), ("far_clip", f32), ("normalize", i32)]


class LgDepthScene(C.Structure):
    _fields_ = [("n_envs", i32), ("base_pos", C.c_void_p), ("base_quat", C.c_void_p), ("heightfield", C.c_void_p), ("rows", i32), ("cols", i32),
                ("hscale", f32), ("vscale", f32), ("border", f32)]


class LgPolicyLayer(C.Structure):
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("n_in", i32), ("n_out", i32), ("elu", i32), ("reserved", i32)]


class LgPolicyChain(C.Structure):
    _fields_ = [("input", C.c_void_p), ("out", C.c_void_p), ("n_layers", i32), ("in_width", i32), ("in_stride", i32), ("out_stride", i32),
                ("layer", LgPolicyLayer * POLICY_MAX_LAYERS)]


class LgPolicyHead(C.Structure):
    _fields_ = [(f"{h}_{k}", C.c_void_p) for h in ("latent_mu", "latent_var", "vel_mu", "vel_var") for k in ("w", "b")] + [
        ("H", i32), ("L", i32), ("E", i32), ("logvar_clip", f32), ("noise", C.c_void_p), ("latent_out", C.c_void_p),
        ("params_out", C.c_void_p), ("dbg_latent_uniform", C.c_void_p), ("noise_stride", i32), ("latent_stride", i32),
        ("params_stride", i32), ("reserved", i32)]


class LgPolicyRnnLayer(C.Structure):
    _fields_ = [("weight_ih", C.c_void_p), ("weight_hh", C.c_void_p), ("bias_ih", C.c_void_p), ("bias_hh", C.c_void_p)]


class LgPolicyMemory(C.Structure):
    _fields_ = [("kind", i32), ("n_layers", i32), ("hidden", i32), ("in_width", i32), ("in_stride", i32), ("reserved", i32),
                ("input", C.c_void_p), ("layer", LgPolicyRnnLayer * POLICY_MAX_RNN_LAYERS), ("h", C.c_void_p), ("c", C.c_void_p),
                ("h_prev_out", C.c_void_p), ("c_prev_out", C.c_void_p), ("reset_mask", C.c_void_p)]


class LgPolicyArgs(C.Structure):
    _fields_ = [("n_envs", i32), ("flags", u32), ("estimator", LgPolicyChain), ("actor", LgPolicyChain), ("critic", LgPolicyChain),
                ("clip_actions", f32), ("clip_on", i32), ("std", C.c_void_p), ("noise", C.c_void_p),
                ("noise_stride", i32), ("actions_stride", i32), ("mu_stride", i32), ("sigma_stride", i32),
                ("actions", C.c_void_p), ("mu", C.c_void_p), ("sigma", C.c_void_p), ("log_prob", C.c_void_p),
                ("log_prob_stride", i32), ("reserved", i32), ("seed", u64), ("counter", C.c_void_p), ("dbg_uniform", C.c_void_p),
                ("encoder_b", LgPolicyChain), ("n_split", i32), ("has_split", i32), ("head", LgPolicyHead)]


class LgPolicyRecurrentArgs(LgPolicyArgs):
    """struct { LgPolicyArgs args; LgPolicyMemory memory_a, memory_c; }: a ctypes subclass lays its own fields out behind the base's, so
    the members of `args` are attributes of this object as they are of a plain LgPolicyArgs."""
    _fields_ = [("memory_a", LgPolicyMemory), ("memory_c", LgPolicyMemory)]


class LgPpoGroup(C.Structure):
    _fields_ = [("n_rows", i32)] + [(f"{n}_stride", i32) for n in ("mu", "sigma", "actions", "old_mu", "old_sigma", "old_log_prob", "advantages",
                                                                    "grad_mu", "grad_sigma")] + [
        (n, C.c_void_p) for n in ("mu", "sigma", "actions", "old_mu", "old_sigma", "old_log_prob", "advantages", "grad_mu", "grad_sigma")]


class LgPpoLossArgs(C.Structure):
    _fields_ = [("n_groups", i32), ("n_actions", i32), ("flags", u32), ("n_value_rows", i32), ("group", LgPpoGroup * PPO_MAX_GROUPS),
                ("values", C.c_void_p), ("returns", C.c_void_p), ("target_values", C.c_void_p), ("grad_values", C.c_void_p),
                ("values_stride", i32), ("returns_stride", i32), ("target_values_stride", i32), ("grad_values_stride", i32),
                ("clip_param", C.c_double), ("value_loss_coef", C.c_double), ("entropy_coef", C.c_double),
                ("partials", C.c_void_p), ("partials_capacity", i64), ("result", C.c_void_p)]


class LgAdamTensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("grad", C.c_void_p), ("numel", i64)]


class LgAdamArgs(C.Structure):
    _fields_ = [("n_tensors", i32), ("flags", u32), ("tensor", LgAdamTensor * ADAM_MAX_TENSORS),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("max_grad_norm", C.c_double), ("desired_kl", C.c_double),
                ("kl", C.c_void_p), ("state", C.c_void_p), ("partials", C.c_void_p), ("partials_capacity", i64), ("result", C.c_void_p)]


class LgTrainLayer(C.Structure):
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("grad_weight", C.c_void_p), ("grad_bias", C.c_void_p),
                ("n_in", i32), ("n_out", i32), ("elu", i32), ("reserved", i32)]


class LgTrainChain(C.Structure):
    _fields_ = [("input", C.c_void_p), ("in_stride", i32), ("n_layers", i32), ("layer", LgTrainLayer * POLICY_MAX_LAYERS)]


class LgTrainArgs(C.Structure):
    _fields_ = [("n_rows", i32), ("clip_on", i32), ("clip_actions", f32), ("reserved", i32), ("chain", LgTrainChain * TRAIN_CHAINS),
                ("std", C.c_void_p), ("grad_std", C.c_void_p), ("mu", C.c_void_p), ("sigma", C.c_void_p), ("values", C.c_void_p),
                ("grad_mu", C.c_void_p), ("grad_sigma", C.c_void_p), ("grad_values", C.c_void_p),
                ("mu_stride", i32), ("sigma_stride", i32), ("values_stride", i32),
                ("grad_mu_stride", i32), ("grad_sigma_stride", i32), ("grad_values_stride", i32),
                ("workspace", C.c_void_p), ("workspace_capacity", i64)]


class LgTrainPlan(C.Structure):
    _fields_ = [("row_tile", i32), ("lds_bytes", i32), ("slices", i32 * POLICY_MAX_LAYERS * TRAIN_CHAINS),
                ("slice_rows", i32 * POLICY_MAX_LAYERS * TRAIN_CHAINS), ("std_slices", i32), ("std_slice_rows", i32),
                ("weight_jobs", i32), ("reserved", i32), ("h_off", i64 * POLICY_MAX_LAYERS * TRAIN_CHAINS),
                ("g_off", i64 * POLICY_MAX_LAYERS * TRAIN_CHAINS), ("p_off", i64 * POLICY_MAX_LAYERS * TRAIN_CHAINS),
                ("std_p_off", i64), ("workspace_floats", i64)]


class LgTrainEEArgs(C.Structure):
    _fields_ = [("n_rows", i32), ("clip_on", i32), ("clip_actions", f32), ("reserved", i32), ("chain", LgTrainChain * TRAIN_EE_CHAINS),
                ("std", C.c_void_p), ("grad_std", C.c_void_p), ("mu", C.c_void_p), ("sigma", C.c_void_p), ("values", C.c_void_p),
                ("grad_mu", C.c_void_p), ("grad_sigma", C.c_void_p), ("grad_values", C.c_void_p),
                ("mu_stride", i32), ("sigma_stride", i32), ("values_stride", i32),
                ("grad_mu_stride", i32), ("grad_sigma_stride", i32), ("grad_values_stride", i32),
                ("workspace", C.c_void_p), ("workspace_capacity", i64)]


class LgTrainEstArgs(C.Structure):
    _fields_ = [("n_rows", i32), ("labels_stride", i32), ("mask_stride", i32), ("reserved", i32), ("chain", LgTrainChain),
                ("labels", C.c_void_p), ("mask", C.c_void_p), ("loss", C.c_void_p), ("upstream", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_capacity", i64)]


class LgTrainEEPlan(C.Structure):
    _fields_ = [("row_tile", i32), ("lds_bytes", i32), ("slices", i32 * POLICY_MAX_LAYERS * TRAIN_EE_CHAINS),
                ("slice_rows", i32 * POLICY_MAX_LAYERS * TRAIN_EE_CHAINS), ("std_slices", i32), ("std_slice_rows", i32),
                ("weight_jobs", i32), ("loss_tiles", i32), ("est_first_buffer", i32), ("reserved", i32),
                ("h_off", i64 * POLICY_MAX_LAYERS * TRAIN_EE_CHAINS), ("g_off", i64 * POLICY_MAX_LAYERS * TRAIN_EE_CHAINS),
                ("p_off", i64 * POLICY_MAX_LAYERS * TRAIN_EE_CHAINS), ("std_p_off", i64), ("cat_off", i64), ("gl_off", i64),
                ("partial_off", i64), ("workspace_floats", i64)]


class LgTrainTSArgs(C.Structure):
    _fields_ = [("n_rows", i32), ("clip_on", i32), ("clip_actions", f32), ("n_obs", i32), ("chain", LgTrainChain * TRAIN_TS_RL_CHAINS),
                ("std", C.c_void_p), ("grad_std", C.c_void_p), ("mu", C.c_void_p), ("sigma", C.c_void_p), ("values", C.c_void_p),
                ("grad_mu", C.c_void_p), ("grad_sigma", C.c_void_p), ("grad_values", C.c_void_p),
                ("mu_stride", i32), ("sigma_stride", i32), ("values_stride", i32),
                ("grad_mu_stride", i32), ("grad_sigma_stride", i32), ("grad_values_stride", i32),
                ("workspace", C.c_void_p), ("workspace_capacity", i64)]


class LgTrainEncArgs(C.Structure):
    _fields_ = [("n_rows", i32), ("mask_stride", i32), ("reserved", i32 * 2), ("chain", LgTrainChain * TRAIN_ENC_CHAINS),
                ("mask", C.c_void_p), ("loss", C.c_void_p), ("upstream", C.c_void_p), ("workspace", C.c_void_p), ("workspace_capacity", i64)]


class LgTrainTSPlan(C.Structure):
    _fields_ = [("row_tile", i32), ("lds_bytes", i32), ("slices", i32 * POLICY_MAX_LAYERS * TRAIN_TS_CHAINS),
                ("slice_rows", i32 * POLICY_MAX_LAYERS * TRAIN_TS_CHAINS), ("std_slices", i32), ("std_slice_rows", i32),
                ("weight_jobs", i32), ("loss_tiles", i32), ("enc_first_buffer", i32), ("reserved", i32),
                ("h_off", i64 * POLICY_MAX_LAYERS * TRAIN_TS_CHAINS), ("g_off", i64 * POLICY_MAX_LAYERS * TRAIN_TS_CHAINS),
                ("p_off", i64 * POLICY_MAX_LAYERS * TRAIN_TS_CHAINS), ("std_p_off", i64), ("cat_off", i64), ("gl_off", i64), ("y_off", i64),
                ("partial_off", i64), ("workspace_floats", i64)]


class LgTrainDwaqArgs(C.Structure):
    _fields_ = [("n_rows", i32), ("clip_on", i32), ("clip_actions", f32), ("n_obs", i32), ("var_clip", f32), ("noise_stride", i32),
                ("reserved", i32 * 2), ("chain", LgTrainChain * TRAIN_DWAQ_CHAINS), ("noise", C.c_void_p),
                ("std", C.c_void_p), ("grad_std", C.c_void_p), ("mu", C.c_void_p), ("sigma", C.c_void_p), ("values", C.c_void_p),
                ("grad_mu", C.c_void_p), ("grad_sigma", C.c_void_p), ("grad_values", C.c_void_p),
                ("mu_stride", i32), ("sigma_stride", i32), ("values_stride", i32),
                ("grad_mu_stride", i32), ("grad_sigma_stride", i32), ("grad_values_stride", i32),
                ("workspace", C.c_void_p), ("workspace_capacity", i64)]


class LgTrainVaeArgs(C.Structure):
    _fields_ = [("n_rows", i32), ("labels_stride", i32), ("next_states_stride", i32), ("mask_stride", i32), ("noise_stride", i32),
                ("var_clip", f32), ("kld_weight", f32), ("reserved", i32), ("chain", LgTrainChain * TRAIN_VAE_CHAINS),
                ("labels", C.c_void_p), ("next_states", C.c_void_p), ("mask", C.c_void_p), ("noise", C.c_void_p), ("loss", C.c_void_p),
                ("upstream", C.c_void_p), ("workspace", C.c_void_p), ("workspace_capacity", i64)]


class LgTrainDwaqPlan(C.Structure):
    _fields_ = [("row_tile", i32), ("lds_bytes", i32), ("slices", i32 * POLICY_MAX_LAYERS * TRAIN_DWAQ_CHAINS),
                ("slice_rows", i32 * POLICY_MAX_LAYERS * TRAIN_DWAQ_CHAINS), ("std_slices", i32), ("std_slice_rows", i32),
                ("weight_jobs", i32), ("loss_tiles", i32), ("lds_x", i32), ("lds_y", i32),
                ("h_off", i64 * POLICY_MAX_LAYERS * TRAIN_DWAQ_CHAINS), ("g_off", i64 * POLICY_MAX_LAYERS * TRAIN_DWAQ_CHAINS),
                ("p_off", i64 * POLICY_MAX_LAYERS * TRAIN_DWAQ_CHAINS), ("std_p_off", i64), ("cat_off", i64), ("enc_out_off", i64),
                ("head_off", i64 * TRAIN_DWAQ_HEADS), ("gl_rec_off", i64), ("gl_est_off", i64), ("partial_off", i64), ("scale_off", i64),
                ("workspace_floats", i64)]


class LgTrainCTSArgs(C.Structure):
    _fields_ = [("n_teacher", i32), ("n_student", i32), ("n_critic", i32), ("clip_on", i32), ("clip_actions", f32), ("n_obs", i32),
                ("student_obs_stride", i32), ("reserved", i32), ("chain", LgTrainChain * TRAIN_CTS_CHAINS), ("student_obs", C.c_void_p),
                ("std", C.c_void_p), ("grad_std", C.c_void_p), ("mu", C.c_void_p * TRAIN_CTS_GROUPS), ("sigma", C.c_void_p * TRAIN_CTS_GROUPS),
                ("values", C.c_void_p), ("grad_mu", C.c_void_p * TRAIN_CTS_GROUPS), ("grad_sigma", C.c_void_p * TRAIN_CTS_GROUPS),
                ("grad_values", C.c_void_p), ("mu_stride", i32 * TRAIN_CTS_GROUPS), ("sigma_stride", i32 * TRAIN_CTS_GROUPS),
                ("grad_mu_stride", i32 * TRAIN_CTS_GROUPS), ("grad_sigma_stride", i32 * TRAIN_CTS_GROUPS), ("values_stride", i32),
                ("grad_values_stride", i32), ("workspace", C.c_void_p), ("workspace_capacity", i64)]


class LgTrainCTSPlan(C.Structure):
    _fields_ = [("row_tile", i32), ("lds_bytes", i32), ("slices", i32 * POLICY_MAX_LAYERS * TRAIN_CTS_CHAINS),
                ("slice_rows", i32 * POLICY_MAX_LAYERS * TRAIN_CTS_CHAINS), ("std_slices", i32 * TRAIN_CTS_GROUPS),
                ("std_slice_rows", i32 * TRAIN_CTS_GROUPS), ("tiles", i32 * TRAIN_CTS_ROLES), ("weight_jobs", i32),
                ("enc_first_buffer", i32 * TRAIN_CTS_GROUPS), ("h_off", i64 * POLICY_MAX_LAYERS * TRAIN_CTS_CHAINS),
                ("g_off", i64 * POLICY_MAX_LAYERS * TRAIN_CTS_CHAINS), ("p_off", i64 * POLICY_MAX_LAYERS * TRAIN_CTS_CHAINS), ("std_p_off", i64),
                ("cat_off", i64), ("workspace_floats", i64)]


class LgTrainConv(C.Structure):
    _fields_ = [("weight", C.c_void_p), ("bias", C.c_void_p), ("grad_weight", C.c_void_p), ("grad_bias", C.c_void_p),
                ("c_in", i32), ("c_out", i32), ("kernel", i32), ("stride", i32), ("padding", i32), ("dilation", i32)]


class LgTrainTcnArgs(C.Structure):
    _fields_ = [("n_rows", i32), ("mask_stride", i32), ("n_conv", i32), ("n_history", i32), ("conv", LgTrainConv * TRAIN_TCN_MAX_CONV),
                ("history", C.c_void_p), ("history_stride", i32), ("reserved", i32), ("tail", LgTrainChain), ("privilege", LgTrainChain),
                ("mask", C.c_void_p), ("loss", C.c_void_p), ("upstream", C.c_void_p), ("workspace", C.c_void_p), ("workspace_capacity", i64)]


class LgTrainTcnPlan(C.Structure):
    _fields_ = [("row_tile", i32), ("lds_bytes", i32), ("n_conv", i32), ("flat", i32), ("length", i32 * (TRAIN_TCN_MAX_CONV + 1)),
                ("conv_block_rows", i32), ("conv_blocks", i32), ("conv_jobs", i32), ("conv_slices", i32 * TRAIN_TCN_MAX_CONV),
                ("conv_slice_rows", i32 * TRAIN_TCN_MAX_CONV), ("conv_job0", i32 * TRAIN_TCN_MAX_CONV), ("slices", i32 * POLICY_MAX_LAYERS),
                ("slice_rows", i32 * POLICY_MAX_LAYERS), ("weight_jobs", i32), ("loss_tiles", i32),
                ("x_off", i64 * (TRAIN_TCN_MAX_CONV + 1)), ("cg_off", i64 * (TRAIN_TCN_MAX_CONV + 1)), ("conv_p_off", i64 * TRAIN_TCN_MAX_CONV),
                ("h_off", i64 * POLICY_MAX_LAYERS), ("g_off", i64 * POLICY_MAX_LAYERS), ("p_off", i64 * POLICY_MAX_LAYERS),
                ("gl_off", i64), ("y_off", i64), ("partial_off", i64), ("workspace_floats", i64)]


def check(rc, lib=None):
    if rc != 0:
        lib = lib or load_lib()
        raise RuntimeError("lgsim: " + lib.lg_last_error().decode())


class LgTrainRnnLayer(C.Structure):
    _fields_ = [("weight_ih", C.c_void_p), ("weight_hh", C.c_void_p), ("bias_ih", C.c_void_p), ("bias_hh", C.c_void_p),
                ("grad_weight_ih", C.c_void_p), ("grad_weight_hh", C.c_void_p), ("grad_bias_ih", C.c_void_p), ("grad_bias_hh", C.c_void_p)]


class LgTrainRnnMemory(C.Structure):
    _fields_ = [("kind", i32), ("n_layers", i32), ("hidden", i32), ("n_in", i32), ("layer", LgTrainRnnLayer * TRAIN_RNN_MAX_LAYERS),
                ("x", C.c_void_p), ("x_time_stride", i64), ("x_row_stride", i64), ("h0", C.c_void_p), ("c0", C.c_void_p),
                ("h0_layer_stride", i64), ("h0_row_stride", i64), ("c0_layer_stride", i64), ("c0_row_stride", i64), ("mask", C.c_void_p),
                ("mask_time_stride", i64), ("max_len", i32), ("n_traj", i32), ("T", i32), ("reserved", i32)]


class LgTrainRnnArgs(C.Structure):
    _fields_ = [("train", LgTrainArgs), ("memory", LgTrainRnnMemory * TRAIN_RNN_MEMORIES)]


_RNN_I32 = i32 * 2 * TRAIN_RNN_MAX_LAYERS * TRAIN_RNN_MEMORIES
_RNN_OFF = i64 * TRAIN_RNN_MAX_LAYERS * TRAIN_RNN_MEMORIES


class LgTrainRnnPlan(C.Structure):
    _fields_ = [("train", LgTrainPlan), ("time_row_tile", i32), ("time_lds_bytes", i32), ("time_tiles", i32), ("n_envs", i32), ("weight_jobs", i32),
                ("reserved", i32), ("slices", _RNN_I32), ("slice_rows", _RNN_I32), ("gate_off", _RNN_OFF), ("h_off", _RNN_OFF),
                ("hprev_off", _RNN_OFF), ("c_off", _RNN_OFF), ("nh_off", _RNN_OFF), ("dout_off", _RNN_OFF), ("dx_off", _RNN_OFF), ("dh_off", _RNN_OFF),
                ("p_off", i64 * 2 * TRAIN_RNN_MAX_LAYERS * TRAIN_RNN_MEMORIES), ("index_off", i64), ("workspace_floats", i64)]

"""Synthetic MDP fixtures: large, long batches built to cross every decision of the MDP phases, with expected values from the
numpy oracle (oracle/mdp_oracle.py, itself pinned to the reference by the golden replays of tests/test_mdp_oracle.py).

synth_fixture(task, N, seed, steps) returns the inputs a golden fixture holds (init_*, script_* read-backs, last_*_in,
actions_in, rand, counter, esum_override, reward names, terrain seed); record(task, fx) replays them through the oracle stepper
of tests/mdp_harness.py and adds its outputs under the keys the task's check reads.  The result replays through the kernel
stepper exactly like a golden fixture.

Every continuous quantity a decision of the MDP phases compares with a threshold is kept at least 1e-3 (relative, or absolute
where the threshold is 0) away from it, so that a different f32 association order cannot flip the decision; the inputs are
built one step at a time against a live oracle so that state-dependent quantities (distance from the env origin, commands
after a resample, previous actions) can be placed too.  CPU only: no GPU import."""
import functools

import numpy as np

from hcr_genesis_lr_cl_amd import abi, builders
from hcr_genesis_lr_cl_amd import config as cfgmod
from hcr_genesis_lr_cl_amd.model_compiler import load_model
from oracle import mdp_oracle as mo
from tests import mdp_harness as h

f32 = np.float32
TASKS = tuple(h.TASKS)
MARGIN = 1e-3


def min_steps(task):
    cfg = h.TASKS[task].cfg()
    T = builders.make_task_cfg(load_model(cfg.asset.name), cfg)
    return 2 * max(int(T.obs_stack), int(T.priv_stack)) + 2


def first_counter(task, steps):
    """Consecutive counters covering the task's push step near the middle; for go2 also the command-curriculum gate
    (3000 is a multiple of both 750 and 1000).  The other tasks stay clear of the gate, which only go2's kernel stepper splits."""
    return {"go2": 3000, "go2_wtw": 750}.get(task, 500) - steps // 2


# ------------------------------------------------------------------------------------------------------------------------------
def _away(v, th, margin=MARGIN):
    """v moved out of [th - m, th + m] (m = margin * max(|th|, 1e-1)) to the nearer edge."""
    v = np.asarray(v, np.float64)
    m = margin * max(abs(float(th)), 0.1)
    near = np.abs(v - th) < m
    return np.where(near, np.where(v >= th, th + m, th - m), v)


def _quat(rpy):
    cr, sr, cp, sp, cy, sy = [f(rpy[:, i] / 2) for i in range(3) for f in (np.cos, np.sin)]
    return np.stack([cy * sr * cp - sy * cr * sp, cy * cr * sp + sy * sr * cp, sy * cr * cp - cy * sr * sp, cy * cr * cp + sy * sr * sp], 1).astype(f32)


def _heading_cmd(q, c3, T):
    fwd = mo.quat_apply(q, np.tile(np.array([1, 0, 0], f32), (len(q), 1)))
    heading = np.arctan2(fwd[:, 1], fwd[:, 0]).astype(f32)
    return heading, np.clip(f32(0.5) * mo.wrap_to_pi(c3 - heading), f32(T.yaw_clip[0]), f32(T.yaw_clip[1]))


def _heading_ok(heading, c3):
    """The heading away from +-pi (where atan2 jumps), c3 - heading away from the jumps of wrap_to_pi (pi and -2 pi)."""
    d = c3 - heading
    bad = (np.pi - np.abs(heading) < 2e-3) | (np.abs(d - np.pi) < 4e-3) | (np.abs(d + 2 * np.pi) < 4e-3)
    return ~bad


def _forces(rng, N, L, feet, links_on_p, T, chronic_term, term):
    """Contact forces whose decision quantities (norms vs 0.1 / 1 / 10 N, vertical foot force vs the contact and no-fly
    thresholds, tangential vs vertical for the stumble constraint) all keep the margin."""
    f = np.zeros((N, L, 3))
    fz_bins = [(0.0, 0.0), (0.02, 0.08), (0.12, 0.9), (1.1, 9.0), (11.0, 80.0)]
    for l in range(L):
        if l in feet:
            b = rng.integers(0, len(fz_bins), N)
            lo, hi = np.array([fz_bins[i][0] for i in b]), np.array([fz_bins[i][1] for i in b])
            fz = rng.uniform(lo, hi)
            k = np.where(rng.random(N) < 0.8, rng.uniform(0, 3.6, N), rng.uniform(4.2, 8, N))      # |Fxy| / Fz either side of sqrt(15)
            k = np.where(fz == 0, 0.0, k)
            a = rng.uniform(0, 2 * np.pi, N)
            for th in (0.1, 1.0, 10.0, float(T.no_fly_contact_threshold)):
                fz = _away(fz * (fz > 0), th) * (fz > 0)
            f[:, l, 2], f[:, l, 0], f[:, l, 1] = fz, fz * k * np.cos(a), fz * k * np.sin(a)
        else:
            on = rng.random(N) < links_on_p
            d = rng.normal(size=(N, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            mag = np.exp(rng.uniform(np.log(0.02), np.log(60), N))
            if l in term:
                on |= chronic_term
                mag = np.where(chronic_term, rng.uniform(12, 60, N), mag)
            for th in (0.1, 1.0, 10.0):
                mag = _away(mag, th)
            f[:, l] = (on * mag)[:, None] * d
    # the foot norms too (contact states, penalised links): scale the whole vector out of a threshold's margin, which leaves the
    # tangential / vertical ratio alone; repeat while either the norm or the vertical force sits next to a threshold
    for l in feet:
        for _ in range(20):
            n, fz = np.linalg.norm(f[:, l], axis=1), f[:, l, 2]
            bad = np.zeros(N, bool)
            for th in (0.1, 1.0, 10.0):
                bad |= np.abs(n - th) < MARGIN * th
            for th in (0.1, 1.0, 10.0, float(T.no_fly_contact_threshold)):
                bad |= (np.abs(fz - th) < MARGIN * th)
            if not bad.any():
                break
            f[bad, l] *= 1.0 + 4 * MARGIN
    return f.astype(f32)


def synth_fixture(task, N, seed=0, steps=None):
    """Inputs of a synthetic fixture for `task` at N envs over `steps` control steps (default: the minimum that compacts the
    smallest-slack history window twice, at least 24 so that the push step sits well inside)."""
    spec = h.TASKS[task]
    cfg = spec.cfg()
    model = load_model(cfg.asset.name)
    T = builders.make_task_cfg(model, cfg)
    S = T.slots
    A, L, F = model.n_dof, model.n_links, model.n_legs
    steps = steps or max(min_steps(task), 24)
    rng = np.random.default_rng([seed, N, TASKS.index(task)])
    c0 = first_counter(task, steps)
    q0 = cfgmod.default_dof_pos(cfg).astype(np.float64)
    soft = cfgmod.soft_dof_limits(model, cfg).astype(np.float64)
    feet = [int(i) for i in model.arrays["foot_link"][:F]]
    term = model.find_link_indices(cfg.asset.terminate_after_contacts_on)
    maxep = int(T.max_episode_length)
    fx = h.Fixture()
    fx["reward_names"] = np.load(spec.gold)["reward_names"]     # the reference's reward terms, in its order
    # ---- initial state
    ep = rng.integers(0, maxep + 1, N)
    k = rng.random(N)
    ep = np.where(k < 0.3, maxep - rng.integers(0, steps + 1, N), ep)                  # time-outs on every step
    ep = np.where((k >= 0.3) & (k < 0.4), rng.integers(0, 3, N), ep)                   # just reset
    fx["init_episode_length_buf"] = ep.astype(np.int32)
    cmd = np.zeros((N, 4))
    cmd[:, :3] = rng.normal(size=(N, 3)) * [0.5, 0.4, 0.5]
    cmd[:, 3] = rng.uniform(-np.pi, np.pi, N)
    cmd[rng.random(N) < 0.15, :3] = 0                                                   # dropped commands (|cmd| <= 0.2)
    fx["init_commands"] = cmd.astype(f32)
    terrain = None
    if spec.rough:
        fx["terrain_seed"] = np.array(1000 + seed)
        np.random.seed(int(fx["terrain_seed"]))
        from hcr_genesis_lr_cl_amd.terrain import Terrain
        terrain = Terrain(cfg.terrain)
        nl, nt = terrain.env_origins.shape[:2]
        lv = rng.integers(0, nl, N)
        lv[rng.random(N) < 0.2] = 0
        lv[rng.random(N) < 0.2] = nl - 1
        ty = rng.integers(0, nt, N)
        fx["init_terrain_levels"], fx["init_terrain_types"] = lv.astype(np.int64), ty.astype(np.int64)
        fx["init_env_origins"] = terrain.env_origins[lv, ty].astype(f32)
        px, py = cfg.terrain.measured_points_x, cfg.terrain.measured_points_y
        fx["init_height_points"] = np.stack(np.meshgrid(px, py, indexing="ij"), -1).reshape(-1, 2).astype(f32)
    else:
        o = np.zeros((N, 3), f32)
        o[:, :2] = rng.uniform(-40, 40, (N, 2))
        fx["init_env_origins"] = o
    if T.gait_mode == 1:
        bp = cfg.rewards.behavior_params_range
        fx["init_behavior_ranges"] = np.array(list(bp.gait_period_range) + list(bp.base_height_target_range)
                                              + list(bp.foot_clearance_target_range) + list(bp.pitch_target_range) + [4], f32)
        tt = np.ctypeslib.as_array(T.theta_table).reshape(4, 4)
        fx["init_theta"] = tt[rng.integers(0, 4, N)].astype(f32)
        gp = rng.uniform(*bp.gait_period_range, N)
        dt = float(T.control_dt)
        gt = np.where(rng.random(N) < 0.3, gp - dt * rng.uniform(0.6, 1.4, N), rng.uniform(0, 1, N) * gp)   # clocks about to wrap
        gt = np.where(rng.random(N) < 0.1, rng.uniform(0, 0.002, N), gt)                                  # phi near 0
        fx["init_gait_period"], fx["init_gait_time"] = gp[:, None].astype(f32), gt[:, None].astype(f32)
        fx["init_phi"] = (fx["init_gait_time"] / fx["init_gait_period"]).astype(f32)
    if T.gait_mode == 2:
        tt = np.ctypeslib.as_array(T.theta_table).reshape(4, 4)
        th0 = (f32(tt[0, 0]) + rng.random(N, dtype=f32)).astype(f32)
        fx["init_theta"] = np.stack([th0, th0 + f32(tt[0, 1] - tt[0, 0])], 1).astype(f32)
        gp = f32(T.gait_period_fixed)
        gt = np.where(rng.random(N) < 0.3, gp - float(T.control_dt) * rng.uniform(0.6, 1.4, N), rng.uniform(0, 1, N) * gp)
        fx["init_gait_time"] = gt[:, None].astype(f32)
        fx["init_phi"] = (fx["init_gait_time"] / gp).astype(f32)
    # ---- a live oracle: the state the next step's inputs are placed against
    live = h.OracleStepper(spec, fx, N)
    o = live.o
    # chronic failures: a run of consecutive failing steps ending at, one below and beyond the threshold
    thr = int(T.fail_threshold)
    chronic = rng.random(N) < 0.06
    run_len = rng.choice([thr - 1, thr, thr + 1, thr + 3], N)
    run_t0 = rng.integers(0, max(steps - thr - 3, 1), N)
    base_h = float(cfg.init_state.pos[2]) - 0.1
    rows = {k: [] for k in ("base_pos", "base_quat", "base_lin_vel_w", "base_ang_vel_w", "dof_pos", "dof_vel", "torques",
                            "link_contact_forces", "feet_pos", "feet_vel")}
    ins = {k: [] for k in ("actions_in", "rand", "counter", "esum_override", "last_dof_vel_in", "last_feet_vel_in")}
    clip_layout = T.obs_layout in (abi.OBS_GO2, abi.OBS_GO2_WTW, abi.OBS_GO2_EE, abi.OBS_TRON1_EE)
    tq_lim = model.arrays["effort"][:A].astype(np.float64)
    vlim = np.ctypeslib.as_array(T.dof_vel_limits)[:A].astype(np.float64)
    for t in range(steps):
        counter = c0 + t
        R = rng.random((N, S.n_slots)).astype(np.float64)
        # the draws the reference makes once per call for the whole batch (read at its first env) are env-independent in the
        # product too (one Philox counter for all envs, oracle/draw_map.py): one value per step, as the injected uniforms
        if T.sit_percent > 0:          # the sit coin, either side of sit_percent on alternate steps
            sp = float(T.sit_percent)
            R[:, S.task_reset] = rng.uniform(0, sp - 0.01) if t % 2 == 0 else rng.uniform(sp + 0.01, 1)
        if T.gait_mode == 1:           # gait index floor(u * 4): every row of the theta table in turn, away from the bin edges
            R[:, S.task_cb + 4] = (t % 4 + rng.uniform(0.05, 0.95)) / 4
            R[:, S.task_reset + 4] = ((t + 2) % 4 + rng.uniform(0.05, 0.95)) / 4
        if T.terrain_curriculum:
            ml = int(T.max_terrain_level)
            R[:, S.terrain_level] = (rng.integers(0, ml, N) + rng.uniform(0.05, 0.95, N)) / ml
        # ---- base pose
        chronic_now = chronic & (t >= run_t0) & (t < run_t0 + run_len)
        roll = rng.normal(size=N) * 0.15
        pitch = rng.normal(size=N) * 0.15
        u = rng.random(N)
        roll = np.where(u < 0.04, np.pi + rng.normal(size=N) * 0.4, roll)                   # upside down
        pitch = np.where((u >= 0.04) & (u < 0.08), np.sign(rng.normal(size=N)) * rng.uniform(1.52, 1.56, N), pitch)   # Euler edge
        by_force = chronic_now & (rng.random(N) < 0.5) & bool(term)
        roll = np.where(chronic_now & ~by_force, np.pi * 0.8, roll)
        yaw = rng.uniform(-np.pi, np.pi, N)
        yaw = np.where(rng.random(N) < 0.1, np.sign(rng.normal(size=N)) * (np.pi - rng.uniform(0.003, 0.05, N)), yaw)   # heading wrap
        # commands as the step will see them: callback resample, heading, then (for resets) the reset resample
        ep_next = o.episode_length_buf + 1
        cb = np.nonzero(ep_next % T.resample_steps == 0)[0]
        cr = o.command_ranges.astype(np.float64)
        for _ in range(20):
            c = o.commands.astype(np.float64).copy()
            c[cb, 0] = (cr[1] - cr[0]) * R[cb, S.cb_cmd] + cr[0]
            c[cb, 1] = (cr[3] - cr[2]) * R[cb, S.cb_cmd + 1] + cr[2]
            c[cb, 3] = (cr[7] - cr[6]) * R[cb, S.cb_cmd + 2] + cr[6]
            n_cb = np.sqrt(c[cb, 0] ** 2 + c[cb, 1] ** 2 + o.commands[cb, 2].astype(np.float64) ** 2)
            bad = np.zeros(N, bool)
            bad[cb] = np.abs(n_cb - 0.2) < 0.2 * MARGIN * 5
            c[cb, :3] *= (n_cb > 0.2)[:, None]
            q = _quat(np.stack([roll, pitch, yaw], 1))
            heading, c2 = _heading_cmd(q, c[:, 3].astype(f32), T)
            bad |= ~_heading_ok(heading.astype(np.float64), c[:, 3].astype(f32).astype(np.float64))
            c[:, 2] = c2
            # after the reset resample (x, y from the reset slots, yaw from the heading): keep vs 0.2
            cx = (cr[1] - cr[0]) * R[:, S.reset_cmd] + cr[0]
            cy = (cr[3] - cr[2]) * R[:, S.reset_cmd + 1] + cr[2]
            bad |= np.abs(np.sqrt(cx ** 2 + cy ** 2 + c2.astype(np.float64) ** 2) - 0.2) < 0.2 * MARGIN * 5
            xyz, xy = np.sqrt(np.sum(c[:, :3] ** 2, 1)), np.sqrt(np.sum(c[:, :2] ** 2, 1))
            bad |= (np.abs(xyz - 0.1) < 1e-3) | (np.abs(xy - 0.1) < 1e-3)           # stand-still and air-time gates
            bad |= (np.abs(np.sqrt(cx ** 2 + cy ** 2 + c2.astype(np.float64) ** 2) - 0.1) < 1e-3)
            if not bad.any():
                break
            yaw[bad] = rng.uniform(-np.pi + 0.01, np.pi - 0.01, int(bad.sum()))
            R[bad, S.cb_cmd:S.cb_cmd + 3] = rng.random((int(bad.sum()), 3))
            R[bad, S.reset_cmd:S.reset_cmd + 3] = rng.random((int(bad.sum()), 3))
        # projected gravity away from the termination thresholds
        for _ in range(20):
            q = _quat(np.stack([roll, pitch, yaw], 1))
            pgz = mo.quat_rotate_inverse(q, np.tile(np.array([0, 0, -1], f32), (N, 1)))[:, 2].astype(np.float64)
            bad = np.zeros(N, bool)
            for th in {float(T.max_projected_gravity), float(getattr(T, "cat_max_projected_gravity", 0) or T.max_projected_gravity)}:
                bad |= np.abs(pgz - th) < MARGIN * max(abs(th), 0.1)
            if not bad.any():
                break
            roll[bad] += 0.01
        s = {"base_quat": q}
        # ---- base position: xy from the current origin (terrain curriculum distances either side of both thresholds)
        org = o.env_origins.astype(np.float64)
        r = rng.uniform(0, 7, N)
        a = rng.uniform(0, 2 * np.pi, N)
        if T.terrain_curriculum:
            r = _away(r, float(T.terrain_env_length) / 2)
            down = np.linalg.norm(c[:, :2], axis=1) * float(T.episode_length_s) * 0.5
            for _ in range(5):
                r = np.where(np.abs(r - down) < MARGIN * np.maximum(down, 0.1), r + 0.05, r)
                r = _away(r, float(T.terrain_env_length) / 2)
        bp = np.zeros((N, 3))
        bp[:, 0], bp[:, 1] = org[:, 0] + r * np.cos(a), org[:, 1] + r * np.sin(a)
        bp[:, 2] = org[:, 2] + base_h + rng.normal(size=N) * 0.05
        s["base_pos"] = bp.astype(f32)
        if terrain is not None:
            ct = cfg.terrain
            mh = mo.sample_heights(s["base_pos"], q, fx["init_height_points"], terrain.height_field_raw, ct.border_size,
                                   ct.horizontal_scale, ct.vertical_scale)
            bp[:, 2] = mh.mean(1) + base_h + rng.normal(size=N) * 0.08
            if T.cat_enable:
                d = _away(bp[:, 2] - mh.astype(np.float64).mean(1), float(T.cat_min_base_height))
                bp[:, 2] = d + mh.astype(np.float64).mean(1)
            s["base_pos"] = bp.astype(f32)
        # ---- velocities: a few far beyond what the observation clip lets through
        lv = rng.normal(size=(N, 3)) * [0.6, 0.4, 0.15]
        lv[rng.random(N) < 0.03] *= 150.0
        av = rng.normal(size=(N, 3)) * [0.5, 0.5, 0.8]
        if clip_layout:
            av[rng.random(N) < 0.03] *= 1000.0
        s["base_lin_vel_w"], s["base_ang_vel_w"] = lv.astype(f32), av.astype(f32)
        # ---- joints: positions either side of the soft limits, velocities / torques either side of their limits
        dp = q0 + rng.normal(size=(N, A)) * 0.35
        u = rng.random(N)
        j = rng.integers(0, A, N)
        idx = np.arange(N)
        dp[idx, j] = np.where(u < 0.08, soft[j, 0] - rng.uniform(0.01, 0.3, N), dp[idx, j])
        j2 = (j + 1 + rng.integers(0, A - 1, N)) % A
        dp[idx, j2] = np.where(u < 0.04, soft[j2, 1] + rng.uniform(0.01, 0.3, N), dp[idx, j2])    # both at once: cat flag 6
        dp[idx, j2] = np.where((u >= 0.08) & (u < 0.12), soft[j2, 1] + rng.uniform(0.01, 0.3, N), dp[idx, j2])
        for a_ in range(A):
            dp[:, a_] = _away(_away(dp[:, a_], soft[a_, 0]), soft[a_, 1])
        dv = rng.normal(size=(N, A)) * 3
        dv[idx, j] = np.where(rng.random(N) < 0.05, np.sign(rng.normal(size=N)) * rng.uniform(1.05, 2, N) * np.minimum(vlim[j], 60), dv[idx, j])
        dv[rng.random(N) < 0.02] *= 1000.0                                                            # frames beyond clip_obs
        for a_ in range(A):
            for th in (4.0, vlim[a_], -4.0, -vlim[a_]):
                if abs(th) < 1e6:
                    dv[:, a_] = _away(dv[:, a_], th)
        tq = rng.normal(size=(N, A)) * 8
        tq[idx, j] = np.where(rng.random(N) < 0.05, np.sign(rng.normal(size=N)) * tq_lim[j] * rng.uniform(1.02, 1.5, N), tq[idx, j])
        for a_ in range(A):
            tq[:, a_] = _away(_away(tq[:, a_], tq_lim[a_]), -tq_lim[a_])
        if not clip_layout:      # the actor history of these layouts is not clipped (legged_robot_ts.py:71): keep its frames in range
            dv = np.clip(dv, -1900, 1900)
        s["dof_pos"], s["dof_vel"], s["torques"] = dp.astype(f32), dv.astype(f32), tq.astype(f32)
        s["link_contact_forces"] = _forces(rng, N, L, feet, 0.1, T, by_force, term)
        fp = np.zeros((N, F, 3))
        fp[:, :, :2] = bp[:, None, :2] + rng.normal(size=(N, F, 2)) * [0.2, 0.15]
        fz0 = org[:, 2:3] if terrain is None else mh.mean(1, keepdims=True).astype(np.float64)
        fp[:, :, 2] = fz0 + np.abs(rng.normal(size=(N, F))) * 0.06
        if T.about_landing_threshold:
            fp[:, :, 2] = _away(fp[:, :, 2] - float(T.foot_height_offset), float(T.about_landing_threshold)) + float(T.foot_height_offset)
        s["feet_pos"] = fp.astype(f32)
        s["feet_vel"] = (rng.normal(size=(N, F, 3)) * [0.8, 0.4, 0.5]).astype(f32)
        for k_, v in s.items():
            rows[k_].append(v)
        # ---- actions: some beyond clip_actions; for CaT the action-rate constraint either side of its limit
        act = rng.normal(size=(N, A)) * np.where(rng.random((N, 1)) < 0.05, 80, 1)
        if T.cat_enable:
            ca = float(T.clip_actions)
            dt = float(T.control_dt)
            prev = o.actions.astype(np.float64)
            for a_ in range(A):
                d = np.clip(act[:, a_], -ca, ca) - prev[:, a_]
                for th in (float(T.cat_action_rate) * dt, -float(T.cat_action_rate) * dt):
                    d = _away(d, th)
                act[:, a_] = np.where(np.abs(act[:, a_]) < ca, prev[:, a_] + d, act[:, a_])
        ins["actions_in"].append(act.astype(f32))
        ins["rand"].append(R.astype(f32))
        ins["counter"].append(counter)
        ins["esum_override"].append(18.5 if task == "go2" and counter % maxep == 0 else 0.0)
        ins["last_dof_vel_in"].append((rng.normal(size=(N, A)) * 3).astype(f32))
        ins["last_feet_vel_in"].append((rng.normal(size=(N, F, 3)) * [0.8, 0.4, 0.5]).astype(f32))
        # advance the live oracle on exactly these inputs
        sim = {k_: v.copy() for k_, v in s.items()}
        sim["last_dof_vel"], sim["last_feet_vel"] = ins["last_dof_vel_in"][-1].copy(), ins["last_feet_vel_in"][-1].copy()
        live.step(t, sim, ins["actions_in"][-1], ins["rand"][-1], counter, ins["esum_override"][-1])
    for k_, v in rows.items():
        fx["script_" + k_] = np.stack(v)
    for k_, v in ins.items():
        fx[k_] = np.array(v, f32) if k_ == "esum_override" else np.stack(v) if k_ != "counter" else np.array(v, np.int64)
    return fx


def record(task, fx):
    """fx with the oracle's outputs added under the keys the task's check reads (feat_last / priv_last: the full stacks at the
    last step)."""
    spec = h.TASKS[task]
    st = h.OracleStepper(spec, fx, fx["rand"].shape[1])
    outs, last = [], {}
    for step in h.fixture_steps(fx):
        out = st.step(*step)
        last = {k: np.array(out.pop(k), copy=True) for k in ("feat_full", "priv_full") if k in out}
        outs.append({k: np.array(v, copy=True) for k, v in out.items()})
    out_fx = h.Fixture(fx)
    for k in outs[0]:
        out_fx[k] = np.stack([o_[k] for o_ in outs])
    if last:
        out_fx["feat_last"], out_fx["priv_last"] = last["feat_full"], last["priv_full"]
    return out_fx


@functools.lru_cache(maxsize=2)
def recorded(task, N, seed=0):
    """record(task, synth_fixture(task, N, seed)), cached: one oracle run per batch, whatever tail or history mode replays it."""
    return record(task, synth_fixture(task, N, seed))

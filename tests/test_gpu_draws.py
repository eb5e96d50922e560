"""GPU: the kernels' Philox draws against the host restatement of the draw map (oracle/philox.py, oracle/draw_map.py).

  * Philox on the chip equals the numpy Philox bit for bit.
  * The generic leg-per-lane launch (env_step_kernel<PRE | POST | RESET>) drawing from Philox equals the numpy MDP oracle fed with
    R = draw_map.uniforms(...): the 4096-env comparison of tests/test_gpu_mdp.py without injected draws, plus a ragged batch on a
    global env id offset above 2^32.
  * Every product launch that env.step() selects for a registered task (lg_host.hip lg_step: the fused quadruped tails RS / PROF 1-4
    and the generic PROF 0 tail, the biped tails PROF 0 / 5 / 6, the two-launch path with the plain and the replicated MDP launch):
    each quantity drawn in the step -- reset DOFs, root position and twist, commands, friction, mass, CoM, kp / kd scales, joint
    DR, gait phase, the sit coin, push velocities, callback commands and the observation noise -- equals the value its formula
    gives on the uniform the map names.  A draw that reads another quantity's word, or a per-env draw that is batch-wide, fails.
"""
import numpy as np
import pytest

from oracle import draw_map
from oracle import mdp_oracle as mo
from oracle.philox import philox4x32_10
from tests import mdp_harness as h
from tests import physics_harness as ph

pytestmark = pytest.mark.gpu


def test_philox_on_chip_matches_numpy():
    import ctypes as C
    import torch
    from hcr_genesis_lr_cl_amd import abi
    assert torch.cuda.is_available()          # the torch runtime first, as everywhere else in the suite
    lib = abi.load_lib()
    rng = np.random.default_rng(4)
    n = 10000
    ctr = rng.integers(0, 2 ** 32, (n, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, (n, 2), dtype=np.uint64)
    ctr[:8, 3] = [0, 1, 0x40000000, 0x40000001, 0x80000000, 0x80000200, 0xFFFFFFFF, 0x7FFFFFFF]   # the counter spaces' edges
    want = np.stack(philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[:, 0], key[:, 1]), 1)
    got = np.zeros((n, 4), np.uint64)
    o = (C.c_uint32 * 4)()
    for i in range(n):
        c, k = (C.c_uint32 * 4)(*(int(v) for v in ctr[i])), (C.c_uint32 * 2)(*(int(v) for v in key[i]))
        abi.check(lib.lg_philox(C.byref(c), C.byref(k), C.byref(o)), lib)
        got[i] = tuple(o)
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,env_id_offset", [(4096, 0), (4093, (1 << 32) + 12345)], ids=["4096", "ragged-offset"])
def test_split_launch_philox_matches_oracle_with_draw_map(N, env_id_offset):
    """tests/test_gpu_mdp.py test_kernel_matches_numpy_oracle_at_4096_envs with the kernel drawing from Philox and the oracle fed
    R = draw_map.uniforms(...) of the kernel's global env ids and counter.  The counters cross go2's push step (750) and the episode
    clocks are spread so that command resampling (every 500 steps of an episode) and time-outs happen in the window."""
    import torch
    from hcr_genesis_lr_cl_amd import abi
    from tests.golden_inputs import random_mdp_inputs
    from tests.mdp_harness import get, load_sim, put
    eng, model, cfg, task = h.make_engine(N, inject_rand=False, seed=0x1234_5678_9ABC, env_id_offset=env_id_offset)
    assert "rand_in" not in eng.buf
    rng = np.random.default_rng(13)
    origins = np.zeros((N, 3), np.float32); origins[:, :2] = rng.uniform(-40, 40, (N, 2))
    put(eng, "env_origins", origins)
    orc = mo.MdpOracle(model, cfg, task, N, origins)
    ep = rng.integers(0, 1001, N).astype(np.int32)
    ep[:64] = [499, 999, 1000, 498] * 16                      # cb resample / time-out on the first steps for sure
    cmds = (rng.normal(size=(N, 4)) * [0.4, 0.4, 0.5, 1.5]).astype(np.float32)
    orc.episode_length_buf[:] = ep; orc.commands[:] = cmds
    put(eng, "episode_length_buf", ep); put(eng, "commands", cmds)
    fb = rng.integers(0, 7, N); orc.fail_buf[:] = fb; put(eng, "fail_buf", fb)
    gids = np.arange(N, dtype=np.uint64) + np.uint64(env_id_offset)
    n_reset = n_cb = 0
    for t, counter in enumerate((749, 750, 751)):
        sim, actions, _ = random_mdp_inputs(rng, model, cfg, N, task.slots.n_slots)
        R = draw_map.task_uniforms(task, model, gids, counter)
        load_sim(eng, sim)
        eng.step(abi.PHASE_PRE | abi.PHASE_POST | abi.PHASE_RESET, torch.from_numpy(actions).cuda(), counter)
        assert "lg_launch_env<" in eng.last_kernel() and "inj" not in eng.last_kernel(), eng.last_kernel()
        n_cb += int(((orc.episode_length_buf + 1) % task.resample_steps == 0).sum())
        orc.step(sim, actions, R, counter)
        torch.cuda.synchronize()
        n_reset += int(orc.reset_buf.sum())
        np.testing.assert_array_equal(get(eng, "reset_buf").astype(bool), orc.reset_buf)
        np.testing.assert_array_equal(get(eng, "episode_length_buf"), orc.episode_length_buf)
        np.testing.assert_array_equal(get(eng, "fail_buf"), orc.fail_buf)
        np.testing.assert_array_equal(get(eng, "last_contacts").astype(bool), orc.last_contacts)
        for name, ref in (("obs_buf", orc.obs_buf), ("rew_buf", orc.rew_buf), ("commands", orc.commands),
                          ("feet_air_time", orc.feet_air_time), ("episode_sums", orc.episode_sums),
                          ("dof_pos", sim["dof_pos"]), ("dof_vel", sim["dof_vel"]), ("base_pos", sim["base_pos"]),
                          ("base_lin_vel_w", sim["base_lin_vel_w"]), ("base_ang_vel_w", sim["base_ang_vel_w"]),
                          ("friction_values", orc.friction_values), ("added_base_mass", orc.added_base_mass),
                          ("base_com_bias", orc.base_com_bias), ("rand_push_vels", orc.rand_push_vels[:, :2] if counter % task.push_interval == 0 else None)):
            if ref is None:
                continue
            got = get(eng, name)[:, :2] if name == "rand_push_vels" else get(eng, name)
            # the yaw command goes through atan2f (device libm, few ulp): 5e-5 rad on that column, 1e-5 elsewhere
            tol = 5e-5 if name in ("commands", "obs_buf") else 1e-5
            np.testing.assert_allclose(got, ref, rtol=1e-5, atol=tol, err_msg=f"{name} step {t}")
    assert n_reset > 50 and n_cb > 10, (n_reset, n_cb)


# ------------------------------------------------------------------------------------------------------------------------------
# (task, environment switches, the instantiation lg_last_kernel must name for the last launch of a step[, {"gate": the two launches of the
# command-curriculum step (the three steps then run across counter 1000), "physics": the launch of the first of two engine calls}])
L1 = {"LG_SIM_LAYOUT": "1"}
PRODUCT = [
    ("go2", {}, "lg_launch_quad_rs<4, 1, false>"),
    ("go2", {"LG_REWARD_SET_CONST": "0"}, "lg_launch_quad<4, true, PR, 1, 3>"),
    # the command-curriculum gate (counter 1000): POST in the fused launch, then a RESET-only launch that makes every reset draw
    ("go2", {}, "lg_launch_quad_rs<4, 1, false>",
     {"gate": ("lg_launch_quad<4, true, LG_PHASE_POST, 0, 3>", "lg_launch_env<LEGS, LG_PHASE_RESET, 0, JPL, false>")}),
    ("go2_wtw", {}, "lg_launch_quad_rs<4, 2, false>"),
    # in-place history shift: outside every profile, the fused launch runs the generic PROF 0 tail (go2 has no history to shift)
    ("go2_wtw", {"LG_OBS_SLACK": "0"}, "lg_launch_quad<4, true, PR, 0, 3>"),
    ("go2_ee", {"LG_OBS_SLACK": "0"}, "lg_launch_quad<4, true, PR, 0, 3>"),
    ("go2_ee", {}, "lg_launch_quad_rs<4, 3, false>"),
    ("go2_ts", {}, "lg_launch_quad_rs<4, 4, false>"),
    ("tron1_pf_ee", {}, "lg_launch_quad<2, true, PR, 6, 3>"),
    ("tron1_pf_ee", {"LG_BIPED_TAIL": "0"}, "lg_launch_quad<2, true, PR, 5, 3>"),
    ("tron1_pf_ee", {"LG_BIPED_FUSE": "0"}, "lg_launch_env<LEGS, PR, 0, JPL, "),
    ("tron1_pf", {}, "lg_launch_quad<2, true, PR, 0, 3>"),
    ("tron1_sf", {"LG_MDP_REPLICAS": "0"}, "lg_launch_env<LEGS, PR, 0, 4, false>"),
    ("tron1_sf", {"LG_MDP_REPLICAS": "1"}, "lg_launch_env<LEGS, PR, 0, 4, true>"),
    ("go2_cat", {"LG_MDP_REPLICAS": "0"}, "lg_launch_env<LEGS, PR, 0, JPL, false>"),
    ("go2_cat", {"LG_MDP_REPLICAS": "1"}, "lg_launch_env<LEGS, PR, 0, JPL, true>"),
    # the large-batch route (lg_host.hip plan(), layout 1): the whole step in ONE leg-per-lane launch, env_step_kernel<.., LG_PHASE_ALL>
    # with the MDP working set parked in LDS across the physics and the read-backs handed over in registers (lg_kernel.h STASH)
    ("go2", L1, "lg_launch_env<4, LG_PHASE_ALL, 1, 3, false>"),
    ("go2", L1, "lg_launch_env<4, LG_PHASE_ALL, 1, 3, false>",
     {"gate": ("lg_launch_env<LEGS, LG_PHASE_PRE | LG_PHASE_SIM | LG_PHASE_POST, 0, JPL, false>", "lg_launch_env<LEGS, LG_PHASE_RESET, 0, JPL, false>")}),
    *((t, L1, "lg_launch_env<LEGS, LG_PHASE_ALL, 0, JPL, false>") for t in ("go2_wtw", "go2_ee", "go2_ts", "tron1_pf_ee", "tron1_pf", "tron1_sf")),
    # go2_cat keeps its two calls (the job-wide CaT flag passes between them): its physics call is PRE | SIM (envs/go2_ts.py Go2CaT)
    ("go2_cat", L1, "lg_launch_env<LEGS, PR, 0, JPL, false>", {"physics": "lg_launch_env<LEGS, LG_PHASE_PRE | LG_PHASE_SIM, 0, JPL, false>"}),
]
PHYS_KEYS = ("base_pos", "base_quat", "base_lin_vel_w", "base_ang_vel_w", "dof_pos", "dof_vel", "torques", "feet_pos", "feet_vel")   # of ph.TOL
MDP_ORACLE_LAYOUTS = (mo.abi.OBS_GO2, mo.abi.OBS_GO2_WTW, mo.abi.OBS_GO2_EE, mo.abi.OBS_TRON1_EE)   # go2, go2_wtw, go2_ee, tron1_pf_ee


def _pid(case):
    return case[0] + "".join(f"-{k[3:].lower()}{v}" for k, v in case[1].items()) + ("-gate" if len(case) > 3 and "gate" in case[3] else "")


WORST_DRAW = [0.0]          # largest |drawn quantity - its formula on the mapped uniform| _close has seen (printed per row, not asserted)


def _close(got, want, what, atol=1e-5):
    if np.size(got):
        WORST_DRAW[0] = max(WORST_DRAW[0], float(np.abs(np.asarray(got, np.float64) - want).max()))
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=atol, err_msg=what)


def _first_counter(task, U_of, gate, sit):
    """Counter before the three steps: across the push step (or the curriculum gate); for a task with the sit coin, a window whose
    three coins fall on both sides of sit_percent."""
    if gate:
        return int(task.max_episode_length) - 2
    P = int(task.push_interval)
    for s in range(P - 3, P):
        if not sit:
            return P - 2
        coins = [U_of(s + 1 + t)[0, task.slots.task_reset] < task.sit_percent for t in range(3)]
        if any(coins) and not all(coins):
            return s
    raise AssertionError("no window with both sit-coin outcomes next to the push step")


@pytest.mark.parametrize("case", PRODUCT, ids=[_pid(c) for c in PRODUCT])
def test_product_launch_draws_follow_the_map(case, monkeypatch):
    """4096 envs in tests.util.random_sim_state states, episode clocks spread so that time-outs, command and behaviour resampling
    happen, three env.step() calls across the task's push step (or the curriculum gate).  After each step:
      * envs that reset: every drawn quantity formed on the host from the uniform draw_map names for (seed, global env id, counter)
        equals what the launch wrote, terrain levels sent from the top row and the new origins included;
      * envs that do not reset: the physics equals oracle.sim_step(.., "f64") on the same pre-step state and actions (DESIGN.md
        section 2 contract, at most 0.5 % of envs off on a heightfield), push velocities, callback commands and go2_wtw's behaviour
        targets follow the map, and for go2, go2_wtw, go2_ee and tron1_pf_ee (the layouts bench.py times) every MDP output equals
        MdpOracle.step seeded from the launch's pre-step state and fed its read-backs and R = draw_map (env 0 of the gait tasks
        left out, see _check_mdp_oracle);
      * all envs: the observation noise follows the map."""
    import torch
    from hcr_genesis_lr_cl_amd import abi
    from hcr_genesis_lr_cl_amd.engine import Engine
    from hcr_genesis_lr_cl_amd.envs import make_env
    from oracle import oracle as orc
    from tests.util import random_sim_state, load_state_into_engine
    name, switches, want = case[:3]
    extra = case[3] if len(case) > 3 else {}
    gate = "gate" in extra
    WORST_DRAW[0] = 0.0
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    launches, orig = [], Engine.step

    def step(self, phases, actions, counter):
        orig(self, phases, actions, counter)
        launches.append(self.last_kernel())
    monkeypatch.setattr(Engine, "step", step)
    N = 4096
    env, cfg = make_env(name, N)
    env.reset()
    eng, task, model = env._engine, env._engine.task, env._engine.model
    S, A = task.slots, model.n_dof
    b = eng.buf
    host = lambda k: b[k].detach().cpu().numpy()
    gids = np.arange(N, dtype=np.uint64) + np.uint64(int(task.env_id_offset))
    U_of = lambda c: draw_map.task_uniforms(task, model, gids, c)
    st, _ = random_sim_state(model, cfg, N, seed=17)
    load_state_into_engine(eng, st)
    g = torch.Generator(device="cuda"); g.manual_seed(21)
    maxep = int(task.max_episode_length)
    ep = torch.randint(0, maxep + 1, (N,), generator=g, device="cuda", dtype=torch.int32)
    ep[:32] = int(task.resample_steps) - 1                     # callback command resampling on the first step
    for t in range(3):
        ep[32 * (t + 1):32 * (t + 2)] = maxep - t                # time-outs on every step
    if task.gait_mode == 1:
        ep[128:160] = int(task.behavior_resample_steps) - 1    # behaviour resampling on the first step
        bp = cfg.rewards.behavior_params_range                  # widen the behaviour ranges and allow every gait so each draw shows
        cr = list(bp.gait_period_range) + list(bp.base_height_target_range) + list(bp.foot_clearance_target_range) + list(bp.pitch_target_range)
        b["command_ranges"][8:16] = torch.tensor(cr, dtype=torch.float32)
        b["command_ranges"][16] = float(task.num_gait_max)
    env.episode_length_buf[:] = ep
    top = np.zeros(N, bool)
    if task.terrain_curriculum:                                 # envs that time out on the first step leave the top row for a random one
        mx = int(task.max_terrain_level)
        top[32:64] = True
        lv = b["terrain_levels"]; lv[32:64] = mx - 1
        org = b["env_origins"]; org[32:64] = b["base_pos"][32:64]
        org[32:64, 0] -= float(task.terrain_env_length)
    sit = task.sit_percent > 0
    env.common_step_counter = _first_counter(task, U_of, gate, sit)
    q0 = mo.cfgmod.default_dof_pos(cfg)
    nv = np.ctypeslib.as_array(task.noise_vec)[:task.obs_frame].astype(np.float32)
    hf = env.simulator._terrain.height_field_raw if int(eng.opts.terrain_rows) > 0 else None
    seen = dict(reset=0, cb=0, push=0, sit=set(), behavior=0, top=0, phys=0, mdp=0)
    for t in range(3):
        torch.cuda.synchronize()
        pre = {k: host(k).copy() for k in b.keys() if torch.is_tensor(b[k])}
        hs = orc.HostState(model, N, q0, cfg.init_state.pos[2])
        for k in hs.arr:
            if k in pre:
                hs.arr[k][:] = pre[k].reshape(N, -1)
        for k in ("joint_armature", "joint_friction", "joint_damping"):     # per-env joint parameters ride along when bound
            if k in pre:
                hs.arr[k] = pre[k].reshape(N, 1).copy()
        act = torch.randn(N, A, generator=g, device="cuda") * (1.0 if t else 3.0)
        ca = float(cfg.normalization.clip_actions)
        del launches[:]
        env.step(act)
        torch.cuda.synchronize()
        c = env.common_step_counter
        is_gate = gate and c % maxep == 0
        if is_gate:
            assert all(any(w in k for k in launches) for w in extra["gate"]), launches
        else:
            assert want in launches[-1], launches          # go2_cat: physics, then the MDP launch (two engine calls)
            assert "physics" not in extra or (len(launches) == 2 and extra["physics"] in launches[0]), launches
        U = U_of(c)
        u = lambda slot, k=1: U[:, slot:slot + k]
        post = {k: host(k) for k in b.keys() if torch.is_tensor(b[k])}
        rs = post["reset_buf"] != 0
        ids = np.nonzero(rs)[0]
        keep = ~rs
        seen["reset"] += len(ids)
        CR = post["command_ranges"]
        push_step = task.push_interval > 0 and c % task.push_interval == 0
        push = np.zeros((N, 3), np.float32)
        # ---- push (genesis_simulator.py:150-158): every env on the push step
        if push_step:
            m = np.float32(task.max_push_vel_xy)
            _close(post["rand_push_vels"][:, :2], (m + m) * u(S.push, 2) - m, "push velocities")
            push[:, :2] = post["rand_push_vels"][:, :2]
            seen["push"] += 1
        # ---- physics of the envs that did not reset against the f64 oracle from the same pre-step state
        orc.sim_step(eng.desc, eng.opts, hs, np.clip(act.cpu().numpy(), -ca, ca), "f64", threads=16, heightfield=hf)
        hs.arr["base_lin_vel_w"] += push                       # the push lands on the physics result (MdpOracle.step does the same)
        # on a heightfield a sample within round-off of a cell edge may fall in the neighbouring cell (0.5 % of
        # envs); on the plane one env per step may flip a contact or limit branch between f32 and f64 (deeply penetrating random states)
        rule, cap = (ph.ENV_SHARE, 0.005) if hf is not None else (ph.ENV_COUNT, 1)
        off = ph.compare(post, hs.arr, PHYS_KEYS, rule=rule, cap=cap, envs=keep, joint=True, label=name)[ph.ANY]
        seen["phys"] += int(keep.sum())
        seen["phys_off"] = seen.get("phys_off", 0) + int(round(off * keep.sum()))
        # ---- callback command resampling (legged_robot.py:300-315) of envs that did not reset
        cb = keep & (post["episode_length_buf"] % task.resample_steps == 0) & (post["episode_length_buf"] > 0)
        seen["cb"] += int(cb.sum())
        _check_commands(post["commands"], U, S.cb_cmd, CR, cb, task, "callback commands")
        # ---- go2_wtw behaviour resampling (go2_wtw.py:180-218): at the callback and at reset, one gait index for the batch
        if task.gait_mode == 1:
            ts = post["task_state"]
            beh = keep & (post["episode_length_buf"] % task.behavior_resample_steps == 0) & (post["episode_length_buf"] > 0)
            seen["behavior"] += int(beh.sum()) + len(ids)
            tt = np.ctypeslib.as_array(task.theta_table).reshape(-1, 4)
            for mask, base in ((beh, S.task_cb), (rs, S.task_reset)):
                if not mask.any():
                    continue
                for k in range(4):
                    want_k = (CR[9 + 2 * k] - CR[8 + 2 * k]) * U[mask, base + k] + CR[8 + 2 * k]
                    sel = min(int(np.floor(U[0, base + 4] * CR[16])), int(CR[16]) - 1)
                    th = tt[sel]
                    if k == 2 and th[0] == 0 and th[1] == 0 and ((th[2] == 0 and th[3] == 0) or (th[2] == 0.5 and th[3] == 0.5)):
                        want_k = np.full_like(want_k, CR[12])    # pronk / bound keep the lowest clearance
                    _close(ts[mask, 2 + k], want_k, f"behaviour target {k}")
                _close(ts[mask, 6:10], np.tile(th, (int(mask.sum()), 1)), "gait offsets (batch-wide gait index)")
        if len(ids):
            # ---- reset_idx: commands, DOFs, root state, DR
            _check_commands(post["commands"], U, S.reset_cmd, CR, rs, task, "reset commands")
            sat = bool(sit and U[0, S.task_reset] < task.sit_percent)
            if sit:
                seen["sit"].add(sat)
            if sat:
                _close(post["dof_pos"][ids], np.tile(np.ctypeslib.as_array(task.sit_dof_pos)[:A], (len(ids), 1)), "sit dof_pos")
                np.testing.assert_array_equal(post["base_lin_vel_w"][ids], 0)
                xy = np.ctypeslib.as_array(task.sit_pos)[:2] + post["env_origins"][ids, :2]
                if task.custom_origins:
                    xy = xy + (np.float32(task.reset_root_xy_span) * u(S.reset_root_xy, 2) + np.float32(task.reset_root_xy_lo))[ids]
                _close(post["base_pos"][ids, :2], xy, "sit root xy")
            else:
                lo, span = np.ctypeslib.as_array(task.reset_dof_lo)[:A], np.ctypeslib.as_array(task.reset_dof_span)[:A]
                _close(post["dof_pos"][ids], (q0 + (span * u(S.reset_dof, A) + lo))[ids], "reset dof_pos")
                _close(post["base_lin_vel_w"][ids], (np.float32(task.reset_lin_vel_span) * u(S.reset_lin_vel, 3) + np.float32(task.reset_lin_vel_lo))[ids], "reset lin vel")
                _close(post["base_ang_vel_w"][ids], (np.float32(task.reset_ang_vel_span) * u(S.reset_ang_vel, 3) + np.float32(task.reset_ang_vel_lo))[ids], "reset ang vel")
                xy = np.array(cfg.init_state.pos[:2], np.float32) + post["env_origins"][ids, :2]
                if task.custom_origins:
                    xy = xy + (np.float32(task.reset_root_xy_span) * u(S.reset_root_xy, 2) + np.float32(task.reset_root_xy_lo))[ids]
                _close(post["base_pos"][ids, :2], xy, "reset root xy")
            np.testing.assert_array_equal(post["dof_vel"][ids], 0)
            if task.dr_friction_on:
                _close(post["friction_values"][ids], (np.float32(task.dr_friction_span) * u(S.dr_friction) + np.float32(task.dr_friction_lo))[ids], "friction")
            if task.dr_mass_on:
                _close(post["added_base_mass"][ids], (np.float32(task.dr_mass_span) * u(S.dr_mass) + np.float32(task.dr_mass_lo))[ids], "mass")
            if task.dr_com_on:
                com = np.ctypeslib.as_array(task.dr_com_span)[:3] * u(S.dr_com, 3) + np.ctypeslib.as_array(task.dr_com_lo)[:3]
                _close(post["base_com_bias"][ids], com[ids].astype(np.float32), "CoM")
            if task.dr_pd_on:
                _close(post["kp_scale"][ids], (np.float32(task.dr_kp_span) * u(S.dr_kp, A) + np.float32(task.dr_kp_lo))[ids], "kp scale")
                _close(post["kd_scale"][ids], (np.float32(task.dr_kd_span) * u(S.dr_kd, A) + np.float32(task.dr_kd_lo))[ids], "kd scale")
            if task.dr_joint_on and "joint_armature" in post:
                js, jl = np.ctypeslib.as_array(task.dr_joint_span)[:3], np.ctypeslib.as_array(task.dr_joint_lo)[:3]
                for k, key in enumerate(("joint_armature", "joint_friction", "joint_damping")):
                    _close(post[key].reshape(N)[ids], (np.float32(js[k]) * U[ids, S.dr_joint + k] + np.float32(jl[k])), key)
            if task.gait_mode == 2:                              # tron1_pf_ee.py:220-226 (layout LG_TASK_STATE_BIPED)
                ts = post["task_state"]
                tt = np.ctypeslib.as_array(task.theta_table).reshape(4, 4)
                _close(ts[ids, 4], np.float32(tt[0, 0]) + U[ids, S.task_reset + 1], "gait phase offset")
                _close(ts[ids, 0], U[ids, S.task_reset + 2] * np.float32(task.gait_period_fixed), "gait clock")
            if task.terrain_curriculum and c > 0:
                lv, mx = post["terrain_levels"], int(task.max_terrain_level)
                hit = top & rs
                seen["top"] += int(hit.sum())
                rnd = np.minimum(np.floor(U[:, S.terrain_level] * mx).astype(np.int64), mx - 1)
                np.testing.assert_array_equal(lv[hit], rnd[hit])
                top &= ~rs
                to = post["terrain_origins"]
                assert to.ndim == 3, to.shape
                _close(post["env_origins"][ids], to[lv[ids], post["terrain_types"][ids]], "terrain origins")
        # ---- go2 and the other benchmarked layouts: every MDP output of the envs that did not reset against MdpOracle.step on the
        #      launch's own read-backs
        if task.obs_layout in MDP_ORACLE_LAYOUTS and not is_gate:
            seen["mdp"] += _check_mdp_oracle(model, cfg, task, N, pre, post, push, np.clip(act.cpu().numpy(), -ca, ca), U, c, keep,
                                             env.simulator._terrain if hf is not None else None)
        # ---- observation noise: the newest actor frame minus the same frame formed noise-free from the launch's own state
        _check_obs_noise(env, task, model, cfg, post, U, nv, q0, b)
    print("product", _pid(case), seen, "worst draw error %.3g" % WORST_DRAW[0])
    assert seen["reset"] > 60 and seen["phys"] > 3 * N - 1000, seen
    assert seen["cb"] > 20 or gate, seen
    assert seen["push"] == (0 if gate else 1), seen
    assert seen["sit"] == ({True, False} if sit else set()), seen
    assert seen["behavior"] > 20 if task.gait_mode == 1 else True, seen
    assert seen["top"] > 10 if task.terrain_curriculum else True, seen
    assert seen["mdp"] > 2 * N - 1000 if task.obs_layout in MDP_ORACLE_LAYOUTS and not gate else True, seen


def _check_mdp_oracle(model, cfg, task, N, pre, post, push, actions, U, c, keep, terrain=None):
    """MdpOracle.step from the launch's pre-step MDP state and post-step physics read-backs (the push taken out of the velocity: the
    oracle applies it), R = draw_map; compared on the envs that did not reset, tolerances of tests/test_gpu_mdp.py.  The gait tasks
    leave out env 0: the oracle reproduces the reference's index-flatten bug on its gait clock and indicator (go2_wtw.py:33-34,
    455-462), which the kernel does not (envs/go2_wtw.py docstring)."""
    from hcr_genesis_lr_cl_amd import abi
    L = task.obs_layout
    orc = mo.MdpOracle(model, cfg, task, N, pre["env_origins"].copy())
    for k in ("actions", "last_actions", "llast_actions", "commands", "feet_air_time", "friction_values", "added_base_mass",
              "base_com_bias", "rand_push_vels", "kp_scale", "kd_scale", "joint_armature", "joint_friction", "joint_damping"):
        if k in pre:
            getattr(orc, k)[:] = pre[k].reshape(getattr(orc, k).shape)
    orc.last_contacts[:] = pre["last_contacts"] != 0
    orc.episode_length_buf[:] = pre["episode_length_buf"]
    orc.fail_buf[:] = pre["fail_buf"]
    orc.episode_sums[:] = pre["episode_sums"]
    orc.command_ranges[:] = pre["command_ranges"][:8]
    gait = h.GAIT[int(task.gait_mode)]
    if gait:
        h.set_task_state(gait, orc, pre["task_state"], pre["command_ranges"])
    if terrain is not None:
        orc.terrain_levels[:], orc.terrain_types[:] = pre["terrain_levels"], pre["terrain_types"]
        orc.terrain_origins = terrain.env_origins.astype(np.float32)
    sim = {k: post[k].reshape(N, -1).copy() for k in h.SIM_KEYS}
    sim["base_lin_vel_w"] -= push
    if "measured_heights" in post and post["measured_heights"].size:       # the SIM phase's terrain read-backs of this step
        sim["measured_heights"] = post["measured_heights"].reshape(N, -1).copy()
        sim["height_around_feet"] = post["height_around_feet"].reshape(N, -1).copy()
        sim["normals"] = post["normal_vector_around_feet"].reshape(N, -1).copy()
    orc.step(sim, actions, U, c)
    k = keep.copy()
    if task.gait_mode:
        k[0] = False
    assert not orc.reset_buf[k].any()
    np.testing.assert_array_equal(post["reset_buf"][k].astype(bool), orc.reset_buf[k])
    np.testing.assert_array_equal(post["episode_length_buf"][k], orc.episode_length_buf[k])
    np.testing.assert_array_equal(post["fail_buf"][k], orc.fail_buf[k])
    np.testing.assert_array_equal(post["last_contacts"][k].astype(bool), orc.last_contacts[k])
    FR = int(task.obs_frame)
    # the newest actor frame (observation noise from R = draw_map) and critic frame; the yaw command goes through atan2f: 5e-5 on
    # the frames and the commands, 1e-5 elsewhere
    checks = [("obs_buf", post["obs_buf"].reshape(N, -1)[:, -FR:], orc.obs_buf[:, -FR:], 5e-5), ("rew_buf", post["rew_buf"], orc.rew_buf, 1e-5),
              ("commands", post["commands"], orc.commands, 5e-5), ("feet_air_time", post["feet_air_time"], orc.feet_air_time, 1e-5),
              ("actions", post["actions"], orc.actions, 1e-5)]
    if L != abi.OBS_GO2:
        PF = int(task.priv_frame)
        checks.append(("priv_obs_buf", post["priv_obs_buf"].reshape(N, -1)[:, -PF:], orc.priv_obs_buf[:, -PF:], 5e-5))
    if L in (abi.OBS_GO2_EE, abi.OBS_TRON1_EE):
        checks.append(("labels_buf", post["labels_buf"].reshape(N, -1), orc.labels_buf, 1e-5))
    if gait:
        checks.append(("task_state", h.recorded_task_state(gait, post["task_state"]),
                       h.recorded_task_state(gait, h.task_state_rows(gait, orc)), 1e-5))
    for name, got, ref, tol in checks:
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-5, atol=tol, err_msg=name)
    np.testing.assert_allclose(post["episode_sums"][:, k], orc.episode_sums[:, k], rtol=1e-5, atol=1e-5, err_msg="episode_sums")
    return int(k.sum())


def _check_commands(cmd, U, slot, CR, mask, task, what):
    """legged_robot.py:317-334: x, y (and heading or yaw) from three uniforms; all three zeroed when |(x, y, yaw)| <= 0.2."""
    if not mask.any():
        return
    x = (CR[1] - CR[0]) * U[:, slot] + CR[0]
    y = (CR[3] - CR[2]) * U[:, slot + 1] + CR[2]
    z = (CR[7] - CR[6] if task.heading_command else CR[5] - CR[4]) * U[:, slot + 2] + (CR[6] if task.heading_command else CR[4])
    got = cmd[mask]
    kept = np.abs(got[:, :2]).sum(1) > 0
    _close(got[kept, 0], x[mask][kept], what + " x")
    _close(got[kept, 1], y[mask][kept], what + " y")
    if task.heading_command:
        _close(got[:, 3], z[mask], what + " heading")
    else:
        _close(got[kept, 2], z[mask][kept], what + " yaw")
    # dropped ones: below the 0.2 norm with their own x, y
    dropped = ~kept
    assert (np.hypot(x[mask][dropped], y[mask][dropped]) <= 0.2 + 1e-6).all(), what


def _check_obs_noise(env, task, model, cfg, post, U, nv, q0, b):
    from hcr_genesis_lr_cl_amd import abi
    N, A, S = env.num_envs, model.n_dof, task.slots
    FR = int(task.obs_frame)
    obs = b["obs_buf"].detach().cpu().numpy().reshape(N, -1)[:, -FR:]
    sc = cfg.normalization.obs_scales
    W = 9 + 3 * A
    clean = np.concatenate([post["commands"][:, :3] * np.array([sc.lin_vel, sc.lin_vel, sc.ang_vel], np.float32), post["projected_gravity"],
                            post["base_ang_vel"] * np.float32(sc.ang_vel), (post["dof_pos"] - q0) * np.float32(sc.dof_pos),
                            post["dof_vel"] * np.float32(sc.dof_vel), post["actions"]], 1).astype(np.float32)
    if task.obs_layout == abi.OBS_TRON1_EE:
        # the clock entries, noise-free, from the critic frame (it starts with the actor frame)
        pf = int(task.priv_frame)
        priv = b["priv_obs_buf"].detach().cpu().numpy().reshape(N, -1)[:, -pf:]
        clean = np.concatenate([clean, priv[:, W:FR]], 1)
    n = clean.shape[1]
    co = np.float32(task.clip_obs)
    want = np.clip(clean + (np.float32(2) * U[:, S.noise:S.noise + n] - np.float32(1)) * nv[:n], -co, co)
    # the yaw command is an atan2f of the forward vector: 5e-5 on it, as in tests/test_gpu_mdp.py
    np.testing.assert_allclose(obs[:, :n], want, rtol=1e-5, atol=5e-5, err_msg="observation noise")
    assert (nv[:n] != 0).sum() >= 3 + 2 * A

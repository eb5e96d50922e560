"""One harness for every physics parity test: a PhysicsCase (CASES) is turned into model / options / terrain by build() and into a seeded
batch of states by initial_state(), stepped by the HIP SIM launch (EngineStepper) or the C oracle (OracleStepper), and the two results
are held against each other by compare().

SIM_OUT, TOL and the force rule are the tolerance contract of DESIGN.md section 2 (HIP physics vs the f64 C oracle), stated here and
nowhere else: the kernel computes in f32 in a different formulation (world-aligned axes about the base origin, leg- or component-per-
lane) from the oracle (body coordinates, dense 6x6), so agreement is f32 round-off amplified by the stiff contact (k = 4e4 N/m: 1e-6 m
of position noise is 0.04 N).  CPU-safe: torch and the engine are imported inside the functions that need them, and with
OracleStepper("f32") standing in for the kernel every case runs without a GPU (tests/test_physics_harness.py)."""
import collections
import dataclasses
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

SIM_OUT = ("base_pos", "base_quat", "base_lin_vel_w", "base_ang_vel_w", "dof_pos", "dof_vel", "torques", "link_contact_forces",
           "feet_pos", "feet_vel", "base_lin_vel", "base_ang_vel", "projected_gravity", "base_euler", "last_dof_vel", "last_feet_vel",
           "last_base_lin_vel", "last_base_ang_vel")
TOL = dict(base_pos=2e-5, base_quat=2e-5, base_lin_vel_w=2e-3, base_ang_vel_w=1e-2, dof_pos=2e-4, dof_vel=3e-2, torques=5e-3,
           feet_pos=1e-4, feet_vel=2e-2, base_lin_vel=2e-3, base_ang_vel=1e-2, projected_gravity=2e-5, base_euler=5e-5,
           last_dof_vel=0, last_feet_vel=0, last_base_lin_vel=0, last_base_ang_vel=0)
RTOL = 1e-4
FORCES = "link_contact_forces"          # 1 % + 0.3 N whatever the scale: the last sub-step's force of a stiff implicit contact
FORCE_REL, FORCE_ABS = 0.01, 0.3
STATE = ("base_pos", "base_quat", "base_lin_vel_w", "base_ang_vel_w", "dof_pos", "dof_vel")
POSE = ("dof_pos", "dof_vel", "base_pos", "base_quat")

LAYOUTS = {1: "leg-per-lane", 2: "component-per-lane"}       # LgSimOptions.sim_layout: the two physics kernels
EIGHT = (0.2, 0.1, 0.1, 0.1, 0.1, 0.2, 0.1, 0.1)             # terrain_proportions with every kind in its own column

# outlier rules of compare(); `cap` is a share for the *_SHARE rules and a count for ENV_COUNT
ALL = "all entries"
ENTRY_SHARE = "share of entries"       # heightfield: a sphere within round-off of a cell edge can see the neighbouring facet
ENV_COUNT = "count of envs"            # several steps through stiff contact: an env on a branch edge of the contact law may differ
ENV_SHARE = "share of envs"
ANY = "any key"                        # in compare()'s result under the env rules: the envs with an entry off in any of the keys


@dataclasses.dataclass(frozen=True)
class PhysicsCase:
    robot: str
    cfg_class: str                     # hcr_genesis_lr_cl_amd.config class
    terrain: str = "plane"             # "plane" (the config's terrain switched off where it has one), "rough" or "eight_kind"
    n: int = 512
    seed: int = 4                      # of tests.util.random_sim_state
    airborne_frac: float = 0.3
    z_offset: float = 0.0
    steps: int = 1                     # control steps
    contact_iters: int = None          # LgSimOptions overrides; None keeps what the config gives
    contact_w_every: int = None
    gravity_z: float = None
    dt: float = None
    gains: tuple = None                # (kp, kd) on every joint
    joint_params: bool = False         # TRON1: per-env armature / frictionloss / damping drawn as the task's DR would
    keys: tuple = SIM_OUT
    tol: tuple = ()                    # ((key, atol), ...) in place of TOL's
    rtol: float = RTOL
    scale: float = 1.0                 # on the absolute tolerances (not on the force rule)
    rule: str = ALL
    cap: float = 0
    contact_free: bool = False         # no contact at all: the forces are exactly zero


_ROUGH = dict(terrain="rough", scale=3.0, rule=ENTRY_SHARE, cap=5e-3)
_EIGHT = dict(_ROUGH, terrain="eight_kind")
CASES = {
    **{f"plane-{s}": PhysicsCase("go2", "GO2Cfg", seed=s) for s in (0, 1, 2)},
    # no contacts at all: pure ABA + PD + integration, four sub-steps -> near round-off
    "free-flight": PhysicsCase("go2", "GO2Cfg", seed=5, airborne_frac=1.1, z_offset=2.0, contact_free=True, rtol=2e-5,
                               keys=("dof_pos", "dof_vel", "base_pos", "base_ang_vel_w", "base_lin_vel_w"),
                               tol=(("dof_pos", 2e-5), ("dof_vel", 2e-3), ("base_pos", 2e-6), ("base_ang_vel_w", 1e-3), ("base_lin_vel_w", 2e-4))),
    # TRON1: the 2-lanes-per-env instantiation, joint_rot / armature / damping tables; tron1_sf: the four-joint chains and the sole contact
    "tron1_pf-plane": PhysicsCase("tron1_pf", "TRON1PFEECfg", joint_params=True),
    "tron1_sf-plane": PhysicsCase("tron1_sf", "TRON1SFCfg", joint_params=True),
    # the heightfield contact (bilinear height + gradient normal) on stairs / slopes / obstacles
    "go2-rough": PhysicsCase("go2", "GO2EECfg", **_ROUGH),
    "tron1_pf-rough": PhysicsCase("tron1_pf", "TRON1PFEECfg", joint_params=True, **_ROUGH),
    **{f"sweeps-{i}": PhysicsCase("go2", "GO2Cfg", n=256, seed=13, contact_iters=i, keys=POSE + (FORCES,)) for i in (1, 3)},
    **{f"reused-w-{k}": PhysicsCase("go2", "GO2Cfg", n=256, seed=17, steps=2, contact_w_every=k, keys=POSE, scale=2.0, rule=ENV_COUNT, cap=2)
       for k in (2, 4)},
    # stepping stones (10 m holes), gaps, pits and waves next to the older kinds, every tile populated
    "go2-eight-kind": PhysicsCase("go2", "GO2EECfg", **_EIGHT),
    "tron1_pf-eight-kind": PhysicsCase("tron1_pf", "TRON1PFEECfg", joint_params=True, **_EIGHT),
}

Built = collections.namedtuple("Built", "model cfg desc opts task terrain")


def build(case, layout):
    """The only place that turns a case into make_model_desc / make_sim_options / make_task_cfg / Terrain."""
    from hcr_genesis_lr_cl_amd import builders, config as cfgmod
    from hcr_genesis_lr_cl_amd.model_compiler import load_model
    cfg = getattr(cfgmod, case.cfg_class)()
    cfg.hip.sim_layout = layout
    t = cfg.terrain
    if case.terrain == "plane":
        t.mesh_type, t.measure_heights, t.curriculum, t.obtain_terrain_info_around_feet = "plane", False, False, False
    model = load_model(case.robot)
    terrain = _terrain(case, cfg)
    desc, opts, task = builders.make_model_desc(model, cfg), builders.make_sim_options(model, cfg, terrain), builders.make_task_cfg(model, cfg)
    opts.sim_layout = layout           # whatever the developer switch LG_SIM_LAYOUT says
    for k in ("contact_iters", "contact_w_every", "gravity_z", "dt"):
        if getattr(case, k) is not None:
            setattr(opts, k, getattr(case, k))
    if case.gains:
        for j in range(model.n_dof):
            opts.kp[j], opts.kd[j] = case.gains
    return Built(model, cfg, desc, opts, task, terrain)


def _terrain(case, cfg):
    """rough: the config's own map from seed 3.  eight_kind: its map with every kind in its own column, curriculum rows and a 20 m
    border, generated from the seed of tests/golden/terrain_kinds_eight_curriculum.npz (tests/test_terrain_kinds.py pins that file to
    the reference) and equal to it."""
    if case.terrain == "plane":
        return None
    from hcr_genesis_lr_cl_amd.terrain import Terrain
    if case.terrain == "rough":
        np.random.seed(3)
        return Terrain(cfg.terrain)
    g = np.load(os.path.join(GOLDEN, "terrain_kinds_eight_curriculum.npz"))
    cfg.terrain.terrain_proportions, cfg.terrain.curriculum, cfg.terrain.border_size = list(EIGHT), True, 20.0
    np.random.seed(int(g["seed"]))
    terrain = Terrain(cfg.terrain)
    np.testing.assert_array_equal(terrain.height_field_raw, g["height_field_raw"])
    return terrain


def initial_state(case, built):
    """(HostState, actions): tests.util.random_sim_state; on a heightfield the robots scattered over the tiles and dropped onto the
    local ground (into the holes and gaps as well)."""
    from tests.util import random_sim_state
    n, terrain, t = case.n, built.terrain, built.cfg.terrain
    st, actions = random_sim_state(built.model, built.cfg, n, case.seed, case.airborne_frac, case.z_offset)
    if terrain is not None:
        from oracle import mdp_oracle as mo
        rng = np.random.default_rng(8)
        tiles = terrain.env_origins.reshape(-1, 3)
        if case.terrain == "eight_kind":
            pick = tiles[rng.permutation(np.arange(n) % len(tiles))]            # every tile gets robots
        else:
            pick = tiles[rng.integers(0, len(tiles), n)]
        st.arr["base_pos"][:, :2] = pick[:, :2] + rng.uniform(-3, 3, (n, 2))
        st.arr["env_origins"][:] = pick
        h = mo.sample_heights(st.arr["base_pos"], np.tile([0, 0, 0, 1.0], (n, 1)).astype(np.float32), np.zeros((1, 2), np.float32),
                              terrain.height_field_raw, t.border_size, t.horizontal_scale, t.vertical_scale)
        st.arr["base_pos"][:, 2] += h[:, 0]
        if case.terrain == "eight_kind":
            assert (h[:, 0] < -9.0).any()                                        # some robots really stand in the stepping-stone holes
    if case.joint_params:
        st.arr["joint_armature"] = np.random.default_rng(1).uniform(0.11, 0.13, (n, 1)).astype(np.float32)
        st.arr["joint_friction"] = np.random.default_rng(2).uniform(0.0, 0.01, (n, 1)).astype(np.float32)
        st.arr["joint_damping"] = np.random.default_rng(3).uniform(1.4, 1.45, (n, 1)).astype(np.float32)
    return st, actions


def floating_state(built, n, height, rng=None, jitter=0.0):
    """Robots at the default pose `height` above the origin; with `rng`, random twists and joint rates and the pose jittered."""
    from hcr_genesis_lr_cl_amd import config as cfgmod
    from oracle import oracle as orc
    st = orc.HostState(built.model, n, cfgmod.default_dof_pos(built.cfg), height)
    if rng is not None:
        A = built.model.n_dof
        st.arr["base_lin_vel_w"][:] = rng.normal(size=(n, 3))
        st.arr["base_ang_vel_w"][:] = rng.normal(size=(n, 3))
        st.arr["dof_vel"][:] = rng.normal(size=(n, A))
        st.arr["dof_pos"][:] += rng.uniform(-jitter, jitter, (n, A)).astype(np.float32)
    st.arr["base_pos"][:, :2] = 0
    return st


# ------------------------------------------------------------------------------------------------------------------------------
class EngineStepper:
    """The HIP SIM launch through the C ABI on cuda:0, `n` envs, the case's terrain uploaded."""

    def __init__(self, built, n):
        from hcr_genesis_lr_cl_amd.engine import Engine
        self.engine = eng = Engine(built.model, built.desc, built.opts, built.task, n, "cuda:0")
        if built.terrain is not None:
            t = built.cfg.terrain
            hx, hy = np.meshgrid(t.measured_points_x, t.measured_points_y, indexing="ij")
            eng.set_terrain(built.terrain.height_field_raw, built.terrain.env_origins, np.stack([hx.ravel(), hy.ravel()], 1).astype(np.float32))

    def load(self, st):
        from tests.util import load_state_into_engine
        load_state_into_engine(self.engine, st)

    def step(self, actions):
        import torch
        from hcr_genesis_lr_cl_amd import abi
        act = actions if torch.is_tensor(actions) else torch.from_numpy(actions).cuda()
        self.engine.step(abi.PHASE_SIM, act, 0)

    def arrays(self, names):
        from tests.util import engine_arrays
        return engine_arrays(self.engine, list(names))


class OracleStepper:
    """oracle.sim_step at `precision` ("f64": the reference; "f32": a stand-in for the kernel) on its own copy of the state."""

    def __init__(self, built, precision):
        self.built, self.precision = built, precision

    def load(self, st):
        self.st = st.copy()

    def step(self, actions):
        from oracle import oracle as orc
        b = self.built
        orc.sim_step(b.desc, b.opts, self.st, actions, self.precision, threads=8,
                     heightfield=None if b.terrain is None else b.terrain.height_field_raw)

    def arrays(self, names):
        return {k: self.st.arr[k].reshape(self.st.n, -1) for k in names}


def read_back(stepper, st, names=STATE):
    """The stepper's state into the HostState `st`."""
    got = stepper.arrays(names)
    for k in names:
        st.arr[k][:] = got[k].reshape(st.arr[k].shape)


def run_case(case, layout, stepper):
    """One case, `stepper(built, n)` against the f64 oracle from the same state and actions: compare()'s per-key outlier shares."""
    built = build(case, layout)
    st, actions = initial_state(case, built)
    test, ref = stepper(built, case.n), OracleStepper(built, "f64")
    test.load(st), ref.load(st)
    for _ in range(case.steps):
        test.step(actions)
        ref.step(actions)
    got = test.arrays(case.keys + ((FORCES,) if case.contact_free else ()))
    if case.contact_free:
        assert np.abs(got[FORCES]).max() == 0.0
    return compare(got, ref.arrays(case.keys), case.keys, case.scale, case.rule, case.cap, dict(case.tol), case.rtol)


# ------------------------------------------------------------------------------------------------------------------------------
def compare(got, ref, keys, scale=1.0, rule=ALL, cap=0, tol=None, rtol=RTOL, envs=None, joint=False, label=""):
    """`got` against `ref` on `keys`.  An entry is off when |got - ref| > scale * atol + rtol * |ref| (atol from `tol`, else TOL), a
    force when |got - ref| > 0.3 N + 1 % of |ref|, or when it is not finite.  Then, per key,
      ALL          no entry is off;
      ENTRY_SHARE  at most `cap` of the entries are off (of the forces: fewer than `cap`);
      ENV_COUNT    at most `cap` envs have an entry off;
      ENV_SHARE    at most `cap` of the envs have an entry off
    -- with `joint`, the env rules count the envs with an entry off in any of the keys.  `envs` masks the envs compared.  Returns the
    share of entries (entry rules) or of envs (env rules) off per key, and under the env rules that of envs off in any key (ANY); a
    failure names key, count and largest error."""
    assert rule in (ALL, ENTRY_SHARE, ENV_COUNT, ENV_SHARE), rule
    tol = dict(TOL, **(tol or {}))
    per_env = rule in (ENV_COUNT, ENV_SHARE)
    bad, worst = {}, {}
    for k in keys:
        r = np.asarray(ref[k]).reshape(len(ref[k]), -1)
        g = np.asarray(got[k]).reshape(r.shape)
        if envs is not None:
            g, r = g[envs], r[envs]
        err = np.abs(g - r)
        off = ~(err <= (FORCE_ABS + FORCE_REL * np.abs(r) if k == FORCES else scale * tol[k] + rtol * np.abs(r)))
        bad[k], worst[k] = off.any(axis=1) if per_env else off, float(err.max())
    if per_env:
        bad[ANY], worst[ANY] = np.any([bad[k] for k in keys], axis=0), worst
    for k in ([ANY] if joint else keys):
        _rule(rule, cap, bad[k], k == FORCES, (label, k, int(bad[k].sum()), worst[k]))
    return {k: float(b.mean()) for k, b in bad.items()}


def _rule(rule, cap, bad, forces, msg):
    if rule == ALL:
        assert not bad.any(), msg
    elif rule == ENTRY_SHARE:
        assert ((~bad).mean() > 1.0 - cap) if forces else (bad.mean() <= cap), msg
    elif rule == ENV_COUNT:
        assert bad.sum() <= cap, msg
    else:
        assert bad.sum() <= cap * bad.size, msg


# ------------------------------------------------------------------------------------------------------------------------------
def momentum(model, st, e=0):
    """Linear + angular momentum about the world origin from the state (independent FK in numpy)."""
    a = model.arrays
    from hcr_genesis_lr_cl_amd.model_compiler import _sym
    def qmat(q):
        x, y, z, w = q
        return np.array([[1-2*(y*y+z*z), 2*(x*y-z*w), 2*(x*z+y*w)], [2*(x*y+z*w), 1-2*(x*x+z*z), 2*(y*z-x*w)],
                         [2*(x*z-y*w), 2*(y*z+x*w), 1-2*(x*x+y*y)]])
    def rod(u, t):
        K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
        return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K
    s = {k: v[e].astype(np.float64) for k, v in st.arr.items()}
    R, P = [qmat(s["base_quat"])], [s["base_pos"]]
    W, V = [s["base_ang_vel_w"]], [s["base_lin_vel_w"]]
    nb = int(a["mass"].shape[0])
    for i in range(1, nb):
        p = int(a["parent"][i])
        Rpc = a["jrot"][i].reshape(3, 3) @ rod(a["axis"][i], s["dof_pos"][i - 1])
        R.append(R[p] @ Rpc)
        Pi = P[p] + R[p] @ a["jpos"][i]
        P.append(Pi)
        V.append(V[p] + np.cross(W[p], Pi - P[p]))
        W.append(W[p] + R[i] @ a["axis"][i] * s["dof_vel"][i - 1])
    lin, ang, mtot, com = np.zeros(3), np.zeros(3), 0.0, np.zeros(3)
    for i in range(nb):
        c = P[i] + R[i] @ a["com"][i]
        vc = V[i] + np.cross(W[i], c - P[i])
        Iw = R[i] @ _sym(a["inertia"][i]) @ R[i].T
        lin += a["mass"][i] * vc
        ang += Iw @ W[i] + a["mass"][i] * np.cross(c, vc)
        mtot += a["mass"][i]; com += a["mass"][i] * c
    return lin, ang, com / mtot

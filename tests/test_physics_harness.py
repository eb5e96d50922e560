"""CPU: tests/physics_harness.py without a GPU.  Every case the GPU tests hold against the f64 oracle runs here with the f32 oracle in
the kernel's place -- through the same build(), initial_state() and compare(), keys, scale, rule and cap -- so each case's inputs are
ones on which the reference alone meets the contract; compare() is shown to fail just beyond each rule and to pass just inside it;
build() gives the option struct of builders.make_sim_options."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import physics_harness as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("layout", list(ph.LAYOUTS))
@pytest.mark.parametrize("name", list(ph.CASES))
def test_f32_oracle_meets_the_contract_on_every_case(name, layout):
    """Measured: no outlier on the plane, in free flight (worst errors there: dof_pos 2.4e-7, dof_vel 7.6e-6, base_pos 4.8e-7), on the
    other configs' planes, at other sweep counts and with reused W; on the eight-kind map go2's worst entry share is 0.26 %
    (projected_gravity), tron1_pf's 0.065 %, against the 0.5 % cap."""
    shares = ph.run_case(ph.CASES[name], layout, lambda built, n: ph.OracleStepper(built, "f32"))
    print(f"{name} layout {layout}: worst outlier share {max(shares.values()):.4%} ({max(shares, key=shares.get)})")


# ---- compare() can fail ---------------------------------------------------------------------------------------------------------
N, W = 200, 10          # 2000 entries a key: a 0.5 % cap is 10 entries, or one env


@pytest.fixture(scope="module")
def ref():
    rng = np.random.default_rng(0)
    return {k: rng.normal(size=(N, W)) * (50.0 if k == ph.FORCES else 1.0) for k in ph.SIM_OUT}


def _off(ref, key, entries, factor, scale=1.0):
    """A copy of `ref` with the given (env, column) entries of `key` moved by `factor` times their bound."""
    got = {k: v.copy() for k, v in ref.items()}
    for e, c in entries:
        r = abs(ref[key][e, c])
        bound = ph.FORCE_ABS + ph.FORCE_REL * r if key == ph.FORCES else scale * ph.TOL[key] + ph.RTOL * r
        got[key][e, c] += factor * bound
    return got


def _fails(*a, **k):
    with pytest.raises(AssertionError):
        ph.compare(*a, **k)
    return True


def test_compare_all_entries(ref):
    assert max(ph.compare(ref, ref, ph.SIM_OUT).values()) == 0.0
    ph.compare(_off(ref, "dof_pos", [(3, 4)], 0.99), ref, ph.SIM_OUT)
    assert _fails(_off(ref, "dof_pos", [(3, 4)], 2.0), ref, ph.SIM_OUT)
    ph.compare(_off(ref, "dof_pos", [(3, 4)], 2.0), ref, ph.SIM_OUT, scale=3.0)        # the scale is on the absolute tolerance
    ph.compare(_off(ref, "last_dof_vel", [(0, 0)], 0.5), ref, ph.SIM_OUT)               # the snapshots: rtol alone
    assert _fails(_off(ref, "last_dof_vel", [(0, 0)], 1.5), ref, ph.SIM_OUT)
    got = _off(ref, "base_quat", [], 0)
    got["base_quat"][7, 1] = np.nan
    assert _fails(got, ref, ph.SIM_OUT)                                                 # a non-finite entry is off under every rule
    assert _fails(got, ref, ph.SIM_OUT, rule=ph.ENV_COUNT, cap=0)
    ph.compare(_off(ref, "dof_pos", [(3, 4)], 2.0), ref, ["dof_pos"], tol=dict(dof_pos=1e-3))   # a per-key tolerance in TOL's place
    assert _fails(_off(ref, "dof_pos", [(3, 4)], 0.5), ref, ["dof_pos"], tol=dict(dof_pos=2e-5), rtol=2e-5)


def test_compare_force_rule(ref):
    """1 % + 0.3 N, whatever the scale."""
    ph.compare(_off(ref, ph.FORCES, [(5, 6)], 1 - 1e-6), ref, ph.SIM_OUT, scale=3.0)
    for scale in (1.0, 3.0):
        assert _fails(_off(ref, ph.FORCES, [(5, 6)], 1 + 1e-6), ref, ph.SIM_OUT, scale=scale)


def test_compare_share_of_entries(ref):
    kw = dict(scale=3.0, rule=ph.ENTRY_SHARE, cap=5e-3)
    ten = [(e, e % W) for e in range(10)]
    shares = ph.compare(_off(ref, "feet_vel", ten, 1.01, 3.0), ref, ph.SIM_OUT, **kw)
    assert shares["feet_vel"] == 10 / (N * W) and shares["dof_pos"] == 0.0
    assert _fails(_off(ref, "feet_vel", ten + [(50, 0)], 1.01, 3.0), ref, ph.SIM_OUT, **kw)
    # the forces' share of entries within the rule has to exceed 99.5 %
    ph.compare(_off(ref, ph.FORCES, ten[:9], 1.01), ref, ph.SIM_OUT, **kw)
    assert _fails(_off(ref, ph.FORCES, ten, 1.01), ref, ph.SIM_OUT, **kw)


def test_compare_count_of_envs(ref):
    kw = dict(scale=2.0, rule=ph.ENV_COUNT, cap=2)
    two = [(11, 0), (11, 5), (90, 2)]                     # two envs, three entries
    shares = ph.compare(_off(ref, "dof_vel", two, 1.01, 2.0), ref, ph.POSE, **kw)
    assert shares["dof_vel"] == shares[ph.ANY] == 2 / N
    assert _fails(_off(ref, "dof_vel", two + [(150, 9)], 1.01, 2.0), ref, ph.POSE, **kw)
    # per key unless `joint`: two envs in one key and a third in another
    got = _off(ref, "dof_vel", two, 1.01, 2.0)
    got["base_pos"][150, 1] += 1.0
    assert ph.compare(got, ref, ph.POSE, **kw)[ph.ANY] == 3 / N
    assert _fails(got, ref, ph.POSE, joint=True, **kw)
    # envs left out of the comparison do not count
    keep = np.ones(N, bool); keep[150] = False
    ph.compare(got, ref, ph.POSE, joint=True, envs=keep, **kw)


def test_compare_share_of_envs(ref):
    kw = dict(rule=ph.ENV_SHARE, cap=0.005, joint=True)   # of 200 envs: one
    got = _off(ref, "torques", [(20, 0), (20, 1)], 1.01)
    assert ph.compare(got, ref, ph.SIM_OUT, **kw)[ph.ANY] == 1 / N
    got["feet_pos"][21, 0] += 1.0
    assert _fails(got, ref, ph.SIM_OUT, **kw)
    keep = np.ones(N, bool); keep[100:] = False           # of 100 envs: none
    assert _fails(_off(ref, "torques", [(20, 0)], 1.01), ref, ph.SIM_OUT, envs=keep, **kw)


# ---- build() ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(ph.LAYOUTS))
def test_build_gives_the_builders_options(layout):
    from hcr_genesis_lr_cl_amd import builders, config as cfgmod
    from hcr_genesis_lr_cl_amd.model_compiler import load_model
    from hcr_genesis_lr_cl_amd.terrain import Terrain
    # plane, with every override
    cfg = cfgmod.GO2Cfg()
    cfg.hip.sim_layout = layout
    want = builders.make_sim_options(load_model("go2"), cfg)
    want.contact_iters, want.contact_w_every, want.gravity_z, want.dt = 3, 4, 0.0, 5e-4
    for j in range(12):
        want.kp[j], want.kd[j] = 80.0, 1.0
    case = ph.PhysicsCase("go2", "GO2Cfg", contact_iters=3, contact_w_every=4, gravity_z=0.0, dt=5e-4, gains=(80.0, 1.0))
    assert bytes(ph.build(case, layout).opts) == bytes(want)
    assert bytes(ph.build(ph.CASES["plane-0"], layout).opts) != bytes(want)
    # rough: the config's own heightfield from seed 3
    cfg = cfgmod.TRON1PFEECfg()
    cfg.hip.sim_layout = layout
    np.random.seed(3)
    terrain = Terrain(cfg.terrain)
    built = ph.build(ph.CASES["tron1_pf-rough"], layout)
    assert bytes(built.opts) == bytes(builders.make_sim_options(load_model("tron1_pf"), cfg, terrain))
    assert built.opts.terrain_rows > 0 and built.opts.n_height_points > 0 and built.opts.sim_layout == layout
    np.testing.assert_array_equal(built.terrain.height_field_raw, terrain.height_field_raw)


def test_harness_imports_without_torch():
    code = "import sys; import tests.physics_harness; assert 'torch' not in sys.modules, 'torch imported'"
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)

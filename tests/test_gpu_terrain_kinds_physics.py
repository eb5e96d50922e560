"""GPU: the physics and the env stack on stepping stones (10 m holes), gaps (5 m), pits and waves, and selected-terrain mode end to
end.  The maps are tests/golden/terrain_kinds_*.npz (tests/test_terrain_kinds.py pins them to the reference)."""
import json
import os

import numpy as np
import pytest

from tests import physics_harness as ph

pytestmark = pytest.mark.gpu

G = ph.GOLDEN


def _play_kwargs():
    """The eight terrain_kwargs sets of legged_gym/scripts/play.py:36-64, as stored with the selected-mode fixtures."""
    out = []
    for f in sorted(os.listdir(G)):
        if f.startswith("terrain_kinds_selected_"):
            out.append(json.loads(str(np.load(os.path.join(G, f))["overrides"]))["terrain_kwargs"])
    assert len(out) == 8
    return out


@pytest.mark.parametrize("robot,layout", [("go2", 1), ("go2", 2), ("tron1_pf", 1), ("tron1_pf", 2)])
def test_one_control_step_on_eight_kind_map_matches_oracle(robot, layout):
    """The heightfield contact on the new tiles against the unchanged f64 oracle, robots scattered over all 100 tiles and dropped onto
    the local ground (into the holes and gaps as well); the tolerance and outlier contract of the rough-terrain cases."""
    shares = ph.run_case(ph.CASES[f"{robot}-eight-kind"], layout, ph.EngineStepper)
    print(f"{robot} layout {layout}: worst outlier share {max(shares.values()):.4%} ({max(shares, key=shares.get)})")


def _finite(out):
    """Observations (estimator features / labels, privileged observations) and rewards of a step or reset are all finite."""
    import torch
    ts = [x for x in out if isinstance(x, torch.Tensor) and x.is_floating_point()]
    return len(ts) >= 2 and all(bool(torch.isfinite(x).all()) for x in ts)


def _make(name, num_envs, **terrain):
    """envs.make_env (envs/__init__.py:30-37), with terrain overrides applied to the task config before the env is built."""
    from hcr_genesis_lr_cl_amd.envs import TASKS, set_seed
    cls, cfg_cls = TASKS[name]
    cfg = cfg_cls()
    cfg.env.num_envs = int(num_envs)
    for k, v in terrain.items():
        setattr(cfg.terrain, k, v)
    set_seed(int(cfg.seed))
    return cls(cfg, None, "cuda:0", True), cfg


@pytest.mark.parametrize("task", ["go2_ee", "tron1_pf_ee"])
def test_random_rollout_on_eight_kind_map_stays_sane(task):
    """4096 envs, 150 control steps of random actions on map (a)'s proportions: nothing non-finite, nobody thrown upward (falling
    into a 10 m hole legitimately reaches about 14 m/s downward)."""
    import torch
    env, cfg = _make(task, 4096, terrain_proportions=list(ph.EIGHT))
    t = env.simulator._terrain
    assert t.heightsamples_dev is not None and int(t.height_field_raw.min()) == -2000 and (t.height_field_raw == -1000).any()
    env.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    b = env._engine.buf
    up = down = rise = 0.0
    for _ in range(150):
        out = env.step(torch.randn(env.num_envs, env.num_actions, generator=g, device="cuda"))
        vz = b["base_lin_vel_w"].view(env.num_envs, -1)[:, 2]
        up, down = max(up, float(vz.max())), min(down, float(vz.min()))
        rise = max(rise, float((b["base_pos"].view(env.num_envs, -1)[:, 2] - env.simulator.env_origins[:, 2]).max()))
        assert _finite(out)
    torch.cuda.synchronize()
    print(f"{task}: max upward base velocity {up:.2f} m/s, max downward {-down:.2f} m/s, max base height above origin {rise:.2f} m")
    assert env._engine.nonfinite_count() == 0
    assert torch.isfinite(b["link_contact_forces"]).all()
    assert up < 6.0 and rise < 3.0


@pytest.mark.parametrize("kwargs", _play_kwargs(), ids=lambda kw: kw["type"].rsplit(".", 1)[-1])
@pytest.mark.parametrize("task", ["go2_ee", "tron1_pf_ee"])
def test_play_config_selected_terrain_end_to_end(task, kwargs):
    """legged_gym/scripts/play.py's terrain overrides (2 x 2 tiles, 5 m border, selected mode) for each of its kwargs sets: the env
    builds, resets and steps with finite observations and rewards, and every env origin is the row of terrain.env_origins at
    (terrain_levels, terrain_types) (genesis_simulator.py:518-528)."""
    import copy
    import torch
    kw = copy.deepcopy(kwargs)
    env, cfg = _make(task, 32, num_rows=2, num_cols=2, border_size=5.0, curriculum=False, selected=True, terrain_kwargs=kw)
    assert cfg.terrain.terrain_kwargs == kwargs
    sim = env.simulator
    t = sim._terrain
    assert t.heightsamples_dev is not None and t.height_field_raw.shape == (2 * 80 + 100, 2 * 80 + 100)
    assert _finite(env.reset())
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    for _ in range(50):
        assert _finite(env.step(torch.randn(env.num_envs, env.num_actions, generator=g, device="cuda")))
    torch.cuda.synchronize()
    lv, ty = sim.terrain_levels.long().cpu().numpy(), sim.terrain_types.long().cpu().numpy()
    want = t.env_origins[lv, ty].astype(np.float32)
    np.testing.assert_array_equal(sim.env_origins.cpu().numpy(), want)

"""Golden heightfields for the stepping-stone, gap, pit and wave tiles and for selected-terrain mode, from the reference's own
Terrain class (build container only; the .npz files are what travels).

Each terrain_kinds_<name>.npz holds the int16 grid (compressed), the env origins, the seed, `after` = np.random.random() drawn right
after generation (it pins numpy's generator state) and the terrain overrides that produced it (applied to the go2_ee config), so the
tests rebuild the same config from the file:
  eight_curriculum / eight_random  every kind, both slope signs and both stair signs in their own column (curriculum: column j is
                                   choice j / 10 + 0.001), and the same proportions randomized;
  selected_<generator>             legged_gym/scripts/play.py:26-64 overrides (2 x 2 tiles, 5 m border, selected) with each of its
                                   eight terrain_kwargs sets;
  nav_six                          a six-entry go2_nav-style proportions list (legged_gym/envs/go2/go2_nav/go2_nav_config.py:30).
Written through ref_harness.save; `python tests/golden/check_fixtures.py` checks that the output still equals the committed files.
"""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

EIGHT = [0.2, 0.1, 0.1, 0.1, 0.1, 0.2, 0.1, 0.1]
PLAY = dict(num_rows=2, num_cols=2, border_size=5.0, curriculum=False, selected=True)
PLAY_KWARGS = [
    {"type": "terrain_utils.random_uniform_terrain", "min_height": -0.05, "max_height": 0.05, "step": 0.005, "downsampled_scale": 0.2},
    {"type": "terrain_utils.pyramid_sloped_terrain", "slope": -0.4, "platform_size": 3.0},
    {"type": "terrain_utils.pyramid_stairs_terrain", "step_width": 0.31, "step_height": -0.1, "platform_size": 3.0},
    {"type": "terrain_utils.discrete_obstacles_terrain", "max_height": 0.1, "min_size": 1.0, "max_size": 2.0, "num_rects": 20,
     "platform_size": 3.0},
    {"type": "terrain_utils.wave_terrain", "amplitude": 0.1, "num_waves": 2},
    {"type": "terrain_utils.stepping_stones_terrain", "stone_size": 1.0, "max_height": 0.1, "stone_distance": 0.3, "platform_size": 3.0},
    {"type": "terrain_utils.gap_terrain", "gap_size": 0.2, "platform_size": 3.0},
    {"type": "terrain_utils.pit_terrain", "depth": 0.2, "platform_size": 3.0},
]
MAPS = {"eight_curriculum": dict(terrain_proportions=EIGHT, curriculum=True),
        "eight_random": dict(terrain_proportions=EIGHT, curriculum=False),
        "nav_six": dict(terrain_proportions=[0.2, 0.2, 0.2, 0.2, 0.1, 0.1], curriculum=True)}
for kw in PLAY_KWARGS:
    MAPS["selected_" + kw["type"].rsplit(".", 1)[-1][:-len("_terrain")]] = dict(PLAY, terrain_kwargs=kw)
SEED = 3


def main():
    import ref_harness as rh
    rh.load_reference()
    import legged_gym.envs  # noqa: F401  (resolves the reference's import cycle first)
    from legged_gym.utils.terrain import Terrain
    from legged_gym.envs.go2.go2_ee.go2_ee_config import Go2EECfg
    for name, over in MAPS.items():
        cfg = Go2EECfg()
        for k, v in over.items():
            setattr(cfg.terrain, k, copy.deepcopy(v))      # the reference pops "type" out of terrain_kwargs
        np.random.seed(SEED)
        t = Terrain(cfg.terrain)
        after = np.random.random()
        rh.save(f"terrain_kinds_{name}", dict(height_field_raw=t.height_field_raw, env_origins=t.env_origins, seed=SEED, after=after,
                                              overrides=json.dumps(over, sort_keys=True)),
                t.height_field_raw.shape, t.height_field_raw.min(), t.height_field_raw.max())


if __name__ == "__main__":
    main()

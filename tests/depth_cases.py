"""Inputs shared by test_depth_oracle.py (CPU) and test_gpu_depth.py: one synthetic terrain, the camera cases, the tolerance, and
the float64 reference images, computed once per process.

Terrain: a 64 x 48 int16 grid (non-square, so that a transposed index shows), hscale 0.1 m, vscale 5 mm, border 1 m: a slope in both
directions with a 5-sample ripple (so that the patches are twisted, not planar), a 1 m step over one cell at row 30, and a pit at
-2000 samples (-10 m).  The world spans x in [-1, 5.3], y in [-1, 3.7].

Tolerance (ISSUE: 1e-3 m unless the float32 run of the oracle on these very inputs differs from float64 by more than 2.5e-4 m, then
4 x that maximum): F32_MAX_DIFF below is that maximum, re-measured and asserted by test_depth_oracle.py::test_float32_oracle_within_tolerance,
which also asserts that the float32 oracle leaves NO pixel of any case outside TOL.
"""
import functools

import numpy as np

from tests import depth_oracle as do

HSCALE, VSCALE, BORDER = 0.1, 0.005, 1.0
MIN_RANGE, MAX_RANGE, HFOV = 0.1, 5.0, 75.0
SHAPES = {"80x60": (80, 60, 5), "7x5": (7, 5, 3)}          # width, height, envs: 4800 pixels are no multiple of the block; 35 are less than a wave
CAMERAS = ("down", "forward", "border", "sky", "below", "nan")
TERRAINS = ("grid", "plane")
F32_MAX_DIFF = 2.5e-4          # upper bound of the float32-vs-float64 oracle difference on these inputs (measured: see DESIGN.md section 6)
TOL = 1e-3
MAX_OUTLIER_SHARE = 1e-3       # a last-bit difference can move a grazing ray's hit to another cell
# cases of the normalisation test and its clips: each case has ranges below NORM_NEAR, between the clips and above NORM_FAR
# (asserted on the CPU by test_depth_oracle.py::test_cases_cover_what_they_claim)
NORM_CASES = [("80x60", "forward", "grid"), ("7x5", "border", "grid"), ("80x60", "forward", "plane")]
NORM_NEAR, NORM_FAR = 0.8, 4.0


def terrain():
    i, j = np.meshgrid(np.arange(64), np.arange(48), indexing="ij")
    hf = 3 * i + 1 * j + (i * 7 + j * 13) % 5
    hf[30:, :] += 200
    hf[10:16, 20:28] = -2000
    return hf.astype(np.int16)


def scene(kind):
    return {"heightfield": terrain() if kind == "grid" else None, "hscale": HSCALE, "vscale": VSCALE, "border": BORDER}


def quat_from_euler_xyz(roll, pitch, yaw):
    cy, sy, cr, sr, cp, sp = np.cos(yaw * 0.5), np.sin(yaw * 0.5), np.cos(roll * 0.5), np.sin(roll * 0.5), np.cos(pitch * 0.5), np.sin(pitch * 0.5)
    return np.stack([cy * sr * cp - sy * cr * sp, cy * cr * sp + sy * sr * cp, sy * cr * cp - cy * sr * sp, cy * cr * cp + sy * sr * sp], -1)


def ray_directions(width, height, hfov_deg=HFOV):
    """The table of include/lgsensor.h, restated (the product's is hcr_genesis_lr_cl_amd.sensor.ray_directions)."""
    f = width / (2.0 * np.tan(np.radians(hfov_deg) / 2.0))
    v, u = np.meshgrid(np.arange(height) + 0.5 - height / 2.0, np.arange(width) + 0.5 - width / 2.0, indexing="ij")
    d = np.stack([np.ones_like(u), -u / f, -v / f], -1)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)


def case(shape, camera, terrain_kind):
    """(cam dict, scene dict, base_pos (N, 3) f32, base_quat (N, 4) f32, ray_dirs (P, 3) f32) of one case.  The poses are float32
    because that is what the engine holds; the oracle reads the same float32 numbers."""
    W, H, N = SHAPES[shape]
    sc = scene(terrain_kind)
    mount_pitch = {"down": 1.57, "forward": 0.4, "border": 0.3, "sky": -1.2, "below": 0.4, "nan": 0.4}[camera]
    cam = {"width": W, "height": H, "mount_pos": (0.3, 0.0, 0.1), "mount_quat": tuple(quat_from_euler_xyz(0.0, mount_pitch, 0.0)),
           "min_range": MIN_RANGE, "max_range": MAX_RANGE, "near_clip": 0.0, "far_clip": 4.0, "normalize": 0}
    xy = np.array([[0.7, 0.3], [1.4, 1.6], [1.0, 1.35], [3.4, 2.2], [4.6, 0.1]])            # on the slope, before the step, beside the pit
    yaw = np.array([0.3, 0.2, 3.0, 1.0, -2.5])                                             # env 1 faces the step, env 2 the pit
    roll, pitch = np.array([0.05, -0.1, 0.0, 0.2, -0.15]), np.array([-0.1, 0.05, 0.15, 0.0, 0.1])
    above = {"down": 1.8, "forward": 0.5, "border": 0.6, "sky": 1.6, "below": -0.6, "nan": 0.5}[camera]
    if camera == "border":                                                                  # at the grid's edges, looking outwards
        xy = np.array([[-0.7, 0.5], [1.5, 3.5], [5.1, 2.0], [2.0, -0.8], [-0.9, -0.9]])
        yaw = np.array([np.pi, np.pi / 2, 0.0, -np.pi / 2, -2.4])
    pos = np.concatenate([xy, (do.surface_height(sc, xy[:, 0], xy[:, 1]) + above)[:, None]], 1)
    if camera == "below":                                                                   # keep the camera itself under the surface
        roll, pitch = roll * 0, pitch * 0
    quat = quat_from_euler_xyz(roll, pitch, yaw)
    pos, quat = pos[:N].astype(np.float32), quat[:N].astype(np.float32)
    if camera == "nan":
        pos[1, 0] = np.nan
    return cam, sc, pos, quat, ray_directions(W, H).astype(np.float32)


def all_cases():
    return [(s, c, t) for t in TERRAINS for s in SHAPES for c in CAMERAS]


@functools.lru_cache(maxsize=None)
def reference(shape, camera, terrain_kind):
    """The float64 oracle's raw range image of a case; computed once, read-only."""
    cam, sc, pos, quat, dirs = case(shape, camera, terrain_kind)
    img = do.render(cam, sc, pos, quat, dirs, np.float64)
    img.setflags(write=False)
    return img


def compare(got, want, cam):
    """(largest difference, number of pixels beyond TOL, all finite and inside [min_range, max_range])."""
    got = np.asarray(got, np.float64)
    diff = np.abs(got - want)
    inside = bool(np.isfinite(got).all() and (got >= np.float32(cam["min_range"])).all() and (got <= np.float32(cam["max_range"])).all())
    return float(np.nanmax(diff)), int((~(diff <= TOL)).sum()), inside

"""Depth camera: host side of include/lgsensor.h.

The reference mounts a gs.sensors.DepthCamera on the base (genesis_simulator.py:803-819), keeps ``depth_images (N, num_history, H, W)``
(:446-453) and clips / normalises what it reads (:741-750).  Here the image is ray-cast against the terrain by one HIP launch
(csrc/lg_sensor.hip); this module builds what that launch needs from the config -- the per-pixel direction table and the mount pose --
and states the update cadence of the depth task (go2_ts_depth.py:157-158, 223-226, 238-239).

Decisions:
  * the value is the RANGE along the pixel's ray, not the planar depth along the optical axis;
  * ``euler`` is read in radians, roll-pitch-yaw, through quat_from_euler_xyz (math_utils.py:111-125), as the reference's own IsaacGym
    glue reads the same field (isaacgym_simulator.py:693-699);
  * only the terrain is seen, the robot's own links are not.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import abi


def quat_from_euler_xyz(roll, pitch, yaw):
    """math_utils.py:111-125 in float64: xyzw."""
    cy, sy, cr, sr, cp, sp = math.cos(yaw * 0.5), math.sin(yaw * 0.5), math.cos(roll * 0.5), math.sin(roll * 0.5), \
        math.cos(pitch * 0.5), math.sin(pitch * 0.5)
    return np.array([cy * sr * cp - sy * cr * sp, cy * cr * sp + sy * sr * cp, sy * cr * cp - cy * sr * sp, cy * cr * cp + sy * sr * sp])


def ray_directions(width, height, hfov_deg):
    """(height * width, 3) float64 unit directions in the camera frame (x forward, y left, z up), pixels row-major with row 0 at the top
    and column 0 at the left.  Pixel (u, v) looks along (1, -(u + 0.5 - W/2) / f, -(v + 0.5 - H/2) / f) with f = W / (2 tan(hfov / 2));
    pixels are square, so the vertical field of view follows from the aspect ratio (warp/warp_cam.py:41-49)."""
    W, H = int(width), int(height)
    if W < 1 or H < 1 or not 0.0 < float(hfov_deg) < 180.0:
        raise ValueError(f"depth camera: resolution {W} x {H} / horizontal field of view {hfov_deg} deg out of range")
    f = W / (2.0 * math.tan(math.radians(float(hfov_deg)) / 2.0))
    u = (np.arange(W, dtype=np.float64) + 0.5 - W / 2.0) / f
    v = (np.arange(H, dtype=np.float64) + 0.5 - H / 2.0) / f
    d = np.stack([np.ones((H, W)), -np.broadcast_to(u[None, :], (H, W)), -np.broadcast_to(v[:, None], (H, W))], axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return d.reshape(H * W, 3)


def depth_cadence_tick(counter, decimation):
    """One env step of go2_ts_depth.py:223-226, 238-239: (render at this step?, counter after the step).  The counter starts at 0, a
    render happens when it equals decimation + 1 and zeroes it, and it is incremented at the end of every step."""
    render = counter == decimation + 1
    return render, (0 if render else counter) + 1


def depth_update_steps(decimation, n_steps):
    """The 1-based env steps among the first n_steps at which the image is rendered: decimation + 2, then every decimation + 1."""
    out, counter = [], 0
    for k in range(1, int(n_steps) + 1):
        render, counter = depth_cadence_tick(counter, decimation)
        if render:
            out.append(k)
    return out


def make_depth_cam(cfg, normalize=True):
    """LgDepthCam of cfg.sensor.depth_camera_config: near_plane / far_plane are the sensor's range (genesis_simulator.py:816-817),
    near_clip / far_clip the normalisation's (:745-750)."""
    c = cfg.sensor.depth_camera_config
    if int(c.num_history) != 1:
        raise ValueError(f"depth camera: num_history = {c.num_history} is not supported, only num_history = 1 (no reference config uses "
                         "another value, and the reference re-normalises the older slots on every update)")
    cam = abi.LgDepthCam()
    cam.width, cam.height = int(c.resolution[0]), int(c.resolution[1])
    abi.fill_array(cam.mount_pos, np.asarray(c.pos, np.float64))
    abi.fill_array(cam.mount_quat, quat_from_euler_xyz(*[float(a) for a in c.euler]))
    cam.min_range, cam.max_range = float(c.near_plane), float(c.far_plane)
    cam.near_clip, cam.far_clip = float(c.near_clip), float(c.far_clip)
    cam.normalize = 1 if normalize else 0
    return cam


def make_depth_scene(n_envs, base_pos, base_quat, opts, height_samples):
    """LgDepthScene over live device tensors: the engine's base pose buffers and the heightfield registered with lg_set_terrain
    (None on a plane).  `opts` is the engine's LgSimOptions."""
    sc = abi.LgDepthScene()
    sc.n_envs = int(n_envs)
    sc.base_pos, sc.base_quat = base_pos.data_ptr(), base_quat.data_ptr()
    if height_samples is not None:
        sc.heightfield = height_samples.data_ptr()
        sc.rows, sc.cols = int(height_samples.shape[0]), int(height_samples.shape[1])
        sc.hscale, sc.vscale, sc.border = float(opts.hscale), float(opts.vscale), float(opts.border)
    return sc


def render(lib, cam, scene, ray_dirs, out, stream):
    """One lg_depth_render launch into `out` (N, H, W) float32 contiguous on `stream`."""
    abi.check(lib.lg_depth_render(C.byref(cam), C.byref(scene), ray_dirs.data_ptr(), out.data_ptr(), stream), lib)

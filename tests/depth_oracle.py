"""Numpy statement of the depth camera of include/lgsensor.h: the surface the robots stand on (terrain_at's bilinear patch with
its clamped extension outside the grid) and the range along each pixel's ray to its first point at or below that surface.

Everything runs in `dtype` (float64 by default: the oracle; float32 to measure what the number format alone costs).  Rays are
processed together, one numpy pass per visited grid cell; the cell walk and the in-cell quadratic are the definition of
include/lgsensor.h, written independently of csrc/lg_sensor.hip.  `surface_height` and `march` are a second, brute-force statement
of the same surface (no cells, no roots) that test_depth_oracle.py holds `render` against.
"""
import numpy as np


def quat_matrix(q, dtype=np.float64):
    """(..., 4) xyzw unit quaternions -> (..., 3, 3) rotation matrices."""
    q = np.asarray(q, dtype)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    one, two = dtype(1), dtype(2)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                  two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                  two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], axis=-1)
    return R.reshape(q.shape[:-1] + (3, 3))


def world_rays(cam, base_pos, base_quat, ray_dirs, dtype=np.float64):
    """Origins (N, 3) and unit directions (N, P, 3) in the world: origin = p + R_base mount_pos, direction = R_base R_mount dir."""
    Rb = quat_matrix(base_quat, dtype)
    Rm = quat_matrix(np.asarray(cam["mount_quat"], dtype), dtype)
    with np.errstate(invalid="ignore"):
        o = np.asarray(base_pos, dtype) + Rb @ np.asarray(cam["mount_pos"], dtype)
        d = np.einsum("nij,pj->npi", Rb @ Rm, np.asarray(ray_dirs, dtype))
    return o, d


def _corner(hf, i, j, vscale, dtype):
    rows, cols = hf.shape
    return hf[np.clip(i, 0, rows - 1), np.clip(j, 0, cols - 1)].astype(dtype) * dtype(vscale)


def surface_height(scene, x, y, dtype=np.float64):
    """terrain_at (csrc/lg_kernel.h): clamped cell index, clamped fraction, bilinear in the four corners; 0 on the plane."""
    hf = scene.get("heightfield")
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    if hf is None:
        return np.zeros(np.broadcast(x, y).shape, dtype)
    rows, cols = hf.shape
    gx, gy = (x + dtype(scene["border"])) / dtype(scene["hscale"]), (y + dtype(scene["border"])) / dtype(scene["hscale"])
    ix = np.clip(np.floor(gx).astype(np.int64), 0, rows - 2)
    iy = np.clip(np.floor(gy).astype(np.int64), 0, cols - 2)
    fx, fy = np.clip(gx - ix, 0, 1).astype(dtype), np.clip(gy - iy, 0, 1).astype(dtype)
    vs = dtype(scene["vscale"])
    h00, h10 = hf[ix, iy].astype(dtype) * vs, hf[ix + 1, iy].astype(dtype) * vs
    h01, h11 = hf[ix, iy + 1].astype(dtype) * vs, hf[ix + 1, iy + 1].astype(dtype) * vs
    return (h00 * (1 - fx) + h10 * fx) * (1 - fy) + (h01 * (1 - fx) + h11 * fx) * fy


def cell_cap(cam, scene):
    """The walk's iteration cap of include/lgsensor.h."""
    return 2 * int(np.ceil(np.float32(cam["max_range"]) / np.float32(scene["hscale"]))) + 4


def hit_distance(cam, scene, o, d, dtype=np.float64):
    """First t in [0, max_range] with z(t) <= h(x(t), y(t)) for rays o + t d (o, d: (R, 3)); inf without one, and for non-finite rays."""
    o, d = np.asarray(o, dtype), np.asarray(d, dtype)
    R = o.shape[0]
    inf = dtype(np.inf)
    max_range = dtype(cam["max_range"])
    hit = np.full(R, inf, dtype)
    ok = np.isfinite(o).all(1) & np.isfinite(d).all(1)
    o, d = np.where(ok[:, None], o, 0).astype(dtype), np.where(ok[:, None], d, 0).astype(dtype)
    ox, oy, oz, dx, dy, dz = o[:, 0], o[:, 1], o[:, 2], d[:, 0], d[:, 1], d[:, 2]
    hf = scene.get("heightfield")
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if hf is None:
            t = np.where(oz <= 0, dtype(0), np.where(dz < 0, -oz / dz, inf))
            return np.where(ok & (t <= max_range), t, inf).astype(dtype)
        hs, vs, border = dtype(scene["hscale"]), scene["vscale"], dtype(scene["border"])
        gx0, gy0 = (ox + border) / hs, (oy + border) / hs
        flx, fly = np.clip(np.floor(gx0), -1e9, 1e9), np.clip(np.floor(gy0), -1e9, 1e9)
        i0, j0 = flx.astype(np.int64), fly.astype(np.int64)
        fx0, fy0 = np.clip(gx0 - flx, 0, 1).astype(dtype), np.clip(gy0 - fly, 0, 1).astype(dtype)
        dgx, dgy = dx / hs, dy / hs
        sx, sy = np.where(dgx > 0, 1, -1), np.where(dgy > 0, 1, -1)
        px, py = (dgx > 0).astype(np.int64), (dgy > 0).astype(np.int64)
        di, dj = np.zeros(R, np.int64), np.zeros(R, np.int64)
        t_enter = np.zeros(R, dtype)
        active = ok.copy()
        for _ in range(cell_cap(cam, scene)):
            if not active.any():
                break
            tx = np.where(dgx != 0, ((di + px).astype(dtype) - fx0) / dgx, inf).astype(dtype)
            ty = np.where(dgy != 0, ((dj + py).astype(dtype) - fy0) / dgy, inf).astype(dtype)
            t_exit = np.minimum(np.fmin(tx, ty), max_range)
            S = t_exit - t_enter
            z0 = oz + t_enter * dz
            i, j = i0 + di, j0 + dj
            h00, h10 = _corner(hf, i, j, vs, dtype), _corner(hf, i + 1, j, vs, dtype)
            h01, h11 = _corner(hf, i, j + 1, vs, dtype), _corner(hf, i + 1, j + 1, vs, dtype)
            u0 = np.clip(fx0 + t_enter * dgx - di.astype(dtype), 0, 1).astype(dtype)
            v0 = np.clip(fy0 + t_enter * dgy - dj.astype(dtype), 0, 1).astype(dtype)
            b, c, e = h10 - h00, h01 - h00, (h11 - h01) - (h10 - h00)
            C = z0 - (h00 + b * u0 + c * v0 + e * u0 * v0)
            B = dz - b * dgx - c * dgy - e * (u0 * dgy + v0 * dgx)
            A = -e * dgx * dgy
            disc = B * B - dtype(4) * A * C
            q = dtype(-0.5) * (B + np.copysign(np.sqrt(np.maximum(disc, 0)), B))
            r1, r2 = q / A, C / q
            s = np.full(R, inf, dtype)
            m1 = (disc >= 0) & (r1 > 0) & (r1 <= S)
            s[m1] = r1[m1]
            m2 = (disc >= 0) & (r2 > 0) & (r2 <= S) & (r2 < s)
            s[m2] = r2[m2]
            s[C <= 0] = 0
            found = active & np.isfinite(s)
            hit[found] = (t_enter + s)[found]
            active &= ~found & (t_exit < max_range)
            stepx = tx <= ty
            di = np.where(stepx, di + sx, di)
            dj = np.where(stepx, dj, dj + sy)
            t_enter = t_exit
    return hit


def finish(cam, hit, dtype=np.float64):
    """Range from the hit distance: no hit -> max_range, clamp to [min_range, max_range]; then the clip-and-scale of
    genesis_simulator.py:745-750 when cam["normalize"]."""
    lo, hi = dtype(cam["min_range"]), dtype(cam["max_range"])
    v = np.maximum(np.where(hit < hi, hit, hi), lo).astype(dtype)
    if cam.get("normalize"):
        v = normalize(cam, v, dtype)
    return v


def normalize(cam, v, dtype=np.float64):
    near, far = dtype(cam["near_clip"]), dtype(cam["far_clip"])
    return ((np.clip(v, near, far) - near) / (far - near) - dtype(0.5)).astype(dtype)


def render(cam, scene, base_pos, base_quat, ray_dirs, dtype=np.float64):
    """(N, height, width) image of include/lgsensor.h's lg_depth_render.  cam: width, height, mount_pos, mount_quat, min_range,
    max_range, near_clip, far_clip, normalize; scene: heightfield (rows, cols) int16 or None, hscale, vscale, border."""
    o, d = world_rays(cam, base_pos, base_quat, ray_dirs, dtype)
    N, P = d.shape[:2]
    hit = hit_distance(cam, scene, np.repeat(o, P, axis=0), d.reshape(N * P, 3), dtype)
    return finish(cam, hit, dtype).reshape(N, int(cam["height"]), int(cam["width"]))


def march(cam, scene, o, d, step=1e-3):
    """Brute force in float64: the first sample t = k * step (k = 0, 1, ...) up to max_range at or below the surface; inf without one."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    ts = np.arange(0.0, float(cam["max_range"]) + 0.5 * step, step)
    out = np.full(o.shape[0], np.inf)
    for r in range(o.shape[0]):
        x, y, z = o[r, 0] + ts * d[r, 0], o[r, 1] + ts * d[r, 1], o[r, 2] + ts * d[r, 2]
        below = np.nonzero(z <= surface_height(scene, x, y))[0]
        if below.size:
            out[r] = ts[below[0]]
    return out

"""CPU: the depth camera's oracle (tests/depth_oracle.py) against closed forms and brute-force marching, the direction table, the
C layout of include/lgsensor.h against the ctypes mirrors, the update cadence, and the float32-vs-float64 measurement that fixes the
tolerance of tests/test_gpu_depth.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from hcr_genesis_lr_cl_amd import abi, sensor
from hcr_genesis_lr_cl_amd import config as cfgmod
from tests import depth_cases as dc
from tests import depth_oracle as do

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lgsensor.h")


def _cam(**kw):
    cam = {"width": 16, "height": 12, "mount_pos": (0.3, 0.0, 0.1), "mount_quat": tuple(dc.quat_from_euler_xyz(0.0, 0.5, 0.0)),
           "min_range": 0.1, "max_range": 5.0, "near_clip": 0.0, "far_clip": 4.0, "normalize": 0}
    cam.update(kw)
    return cam


def _poses():
    pos = np.array([[0.4, 0.2, 1.1], [2.0, 1.5, 0.9], [3.0, 0.7, 1.6]])
    quat = dc.quat_from_euler_xyz(np.array([0.1, -0.2, 0.0]), np.array([0.0, 0.2, -0.1]), np.array([0.5, -2.0, 2.8]))
    return pos, quat


def _plane_range(cam, o, d, n, c):
    """Closed form: range of rays o + t d to the plane n . p = c, seen from above (n . o > c), clamped like the sensor."""
    denom, num = d @ n, c - o @ n
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(denom < 0, num[:, None] / denom, np.inf)
    return np.clip(np.where(t <= cam["max_range"], t, cam["max_range"]), cam["min_range"], cam["max_range"])


def test_oracle_flat_grid_is_ray_plane():
    cam, (pos, quat) = _cam(), _poses()
    sc = {"heightfield": np.full((64, 48), 40, np.int16), "hscale": 0.1, "vscale": 0.005, "border": 1.0}
    dirs = dc.ray_directions(16, 12)
    got = do.render(cam, sc, pos, quat, dirs)
    o, d = do.world_rays(cam, pos, quat, dirs)
    want = _plane_range(cam, o, d, np.array([0.0, 0.0, 1.0]), 0.2)
    np.testing.assert_allclose(got.reshape(3, -1), want, rtol=0, atol=1e-12)
    assert (want < cam["max_range"]).any() and (want == cam["max_range"]).any()
    # the same flat ground as the plane of rows == 0, 0.2 m lower
    got0 = do.render(cam, {"heightfield": None, "hscale": 0.1, "vscale": 0.005, "border": 1.0}, pos - [0, 0, 0.2], quat, dirs)
    np.testing.assert_allclose(got0, got, rtol=0, atol=1e-12)


def test_oracle_linear_ramp_is_ray_plane():
    """h = a i + b j is a bilinear patch exactly; poses whose rays stay inside the grid (outside it the surface is clamped, not a ramp)."""
    i, j = np.meshgrid(np.arange(120), np.arange(110), indexing="ij")
    sc = {"heightfield": (4 * i - 3 * j).astype(np.int16), "hscale": 0.1, "vscale": 0.005, "border": 5.0}
    cam, (pos, quat) = _cam(max_range=3.0), _poses()
    pos = pos + [0.0, 0.0, 0.3]
    dirs = dc.ray_directions(16, 12)
    got = do.render(cam, sc, pos, quat, dirs)
    gxs, gys = 4 * 0.005 / 0.1, -3 * 0.005 / 0.1                     # z = gxs (x + border) + gys (y + border)
    o, d = do.world_rays(cam, pos, quat, dirs)
    want = _plane_range(cam, o, d, np.array([-gxs, -gys, 1.0]), (gxs + gys) * 5.0)
    np.testing.assert_allclose(got.reshape(3, -1), want, rtol=0, atol=1e-11)
    assert (want < cam["max_range"]).mean() > 0.3


def test_oracle_rough_grid_against_1mm_marching():
    """On a rough grid the cell walk and the quadratic agree with 1 mm brute-force marching over terrain_at's surface: the march never
    finds the surface before the oracle's hit, the oracle's hit lies ON the surface, and the march finds it within its 1 mm step."""
    rng = np.random.default_rng(5)
    sc = {"heightfield": rng.integers(-30, 31, (64, 48)).astype(np.int16), "hscale": 0.1, "vscale": 0.005, "border": 1.0}
    cam, (pos, quat) = _cam(width=12, height=9, max_range=4.0), _poses()
    pos = np.concatenate([pos, [[-0.8, -0.7, 0.5]]])                 # one camera in the clamped extension, looking out of the grid
    quat = np.concatenate([quat, dc.quat_from_euler_xyz(np.array([0.0]), np.array([0.0]), np.array([-2.4]))])
    dirs = dc.ray_directions(12, 9)
    o, d = do.world_rays(cam, pos, quat, dirs)
    o, d = np.repeat(o, dirs.shape[0], axis=0), d.reshape(-1, 3)
    hit = do.hit_distance(cam, sc, o, d)
    brute = do.march(cam, sc, o, d, 1e-3)
    found = np.isfinite(hit)
    assert 0.3 < found.mean() < 1.0
    p = o[found] + hit[found, None] * d[found]
    np.testing.assert_allclose(p[:, 2], do.surface_height(sc, p[:, 0], p[:, 1]), rtol=0, atol=1e-9)
    assert (brute[found] >= hit[found] - 1e-9).all()
    assert (brute[found] <= hit[found] + 1e-3 + 1e-9).all()
    # without a hit the march may only find a graze shorter than its own step near max_range's end: nothing at all here
    assert not np.isfinite(brute[~found]).any()


def test_direction_table():
    W, H, hfov = 80, 60, 75.0
    d = sensor.ray_directions(W, H, hfov).reshape(H, W, 3)
    np.testing.assert_allclose(np.linalg.norm(d, axis=-1), 1.0, rtol=0, atol=1e-15)
    c = d[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1]             # the centre four straddle +x
    assert (c[..., 0] > 0.999).all()
    assert (c[:, 0, 1] > 0).all() and (c[:, 1, 1] < 0).all() and (c[0, :, 2] > 0).all() and (c[1, :, 2] < 0).all()
    np.testing.assert_allclose(c.sum((0, 1))[1:], 0.0, atol=1e-15)
    # the image's left edge (half a pixel beyond column 0's centre) is at hfov / 2
    f = W / (2 * np.tan(np.radians(hfov) / 2))
    mid = d[:, 0]                                                    # column 0: y / x = (W/2 - 0.5) / f
    np.testing.assert_allclose(mid[:, 1] / mid[:, 0], (W / 2 - 0.5) / f, rtol=1e-14)
    np.testing.assert_allclose(np.degrees(np.arctan((W / 2) / f)), hfov / 2, rtol=1e-14)
    assert (d[0, :, 2] > 0).all() and (d[-1, :, 2] < 0).all()        # row 0 looks up
    assert (d[:, 0, 1] > 0).all() and (d[:, -1, 1] < 0).all()        # column 0 looks left (+y)
    np.testing.assert_allclose(d.reshape(-1, 3), dc.ray_directions(W, H, hfov), rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        sensor.ray_directions(80, 60, 180.0)


def test_sensor_struct_layouts_match_header():
    structs = [("LgDepthCam", abi.LgDepthCam), ("LgDepthScene", abi.LgDepthScene)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, cls in structs:
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append(f'printf("LG_DEPTH_MAX_CELLS %d\\n", LG_DEPTH_MAX_CELLS);')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "p.c"), os.path.join(tmp, "p")
        with open(src, "w") as f:
            f.write("\n".join(lines))
        subprocess.run(["gcc", "-o", exe, src], check=True)
        got = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for cname, cls in structs:
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert int(got["LG_DEPTH_MAX_CELLS"]) == abi.DEPTH_MAX_CELLS


def test_library_exports_sensor_symbols():
    import re
    if not os.path.exists(abi.lib_path()):
        from hcr_genesis_lr_cl_amd import build
        build.build()
    with open(HEADER) as f:
        declared = set(re.findall(r"\b(lg_\w+)\s*\(", f.read()))
    assert declared == set(abi.SENSOR_EXPORTS)
    lib = C.CDLL(abi.lib_path())                                     # loads without a GPU; nothing is called
    for sym in declared:
        assert hasattr(lib, sym), sym


def test_cadence_decimation_5():
    assert sensor.depth_update_steps(5, 20) == [7, 13, 19]
    assert sensor.depth_update_steps(0, 5) == [2, 3, 4, 5]
    counter, seen = 0, []
    for k in range(1, 21):
        render, counter = sensor.depth_cadence_tick(counter, 5)
        seen.append((render, counter))
    assert [k + 1 for k, (r, _) in enumerate(seen) if r] == [7, 13, 19] and seen[6] == (True, 1) and seen[5] == (False, 6)


def test_depth_config_fields():
    cfg = cfgmod.GO2TSCfg()
    c = cfg.sensor.depth_camera_config
    assert cfg.sensor.add_depth is False and tuple(c.resolution) == (80, 60) and c.num_history == 1 and c.decimation == 5
    assert (c.near_clip, c.far_clip, c.near_plane, c.far_plane) == (0.1, 10.0, 0.1, 10.0)
    assert cfgmod.depth_hfov_deg(cfg) == 75.0
    c.fov_horizontal = 60
    assert cfgmod.depth_hfov_deg(cfg) == 60.0 and cfgmod.depth_hfov_deg(cfgmod.GO2TSCfg()) == 75.0
    cam = sensor.make_depth_cam(cfg)
    assert (cam.width, cam.height, cam.normalize) == (80, 60, 1) and list(cam.mount_quat) == [0.0, 0.0, 0.0, 1.0]
    c.euler = (0.0, 1.57, 0.0)                                      # radians: pitch 1.57 looks down
    q = np.array(list(sensor.make_depth_cam(cfg).mount_quat))
    np.testing.assert_allclose(do.quat_matrix(q) @ [1.0, 0.0, 0.0], [np.cos(1.57), 0.0, -np.sin(1.57)], atol=1e-7)
    c.num_history = 2
    with pytest.raises(ValueError, match="num_history"):
        sensor.make_depth_cam(cfg)


def test_float32_oracle_within_tolerance():
    """The measurement behind the tolerance: the oracle run in float32 on the GPU tests' own inputs against float64.  Its maximum stays
    below dc.F32_MAX_DIFF (so the tolerance is the issue's 1e-3 m) and it leaves no pixel of any case outside the tolerance."""
    worst = 0.0
    for shape, camera, terrain_kind in dc.all_cases():
        cam, sc, pos, quat, dirs = dc.case(shape, camera, terrain_kind)
        want = dc.reference(shape, camera, terrain_kind)
        got = do.render(cam, sc, pos, quat, dirs, np.float32)
        assert got.dtype == np.float32
        diff, beyond, inside = dc.compare(got, want, cam)
        print(f"depth f32 oracle vs f64: {terrain_kind:5s} {shape:5s} {camera:7s} max diff {diff:.3e} m, beyond tolerance {beyond}")
        assert beyond == 0 and inside, (shape, camera, terrain_kind, diff)
        worst = max(worst, diff)
    assert worst <= dc.F32_MAX_DIFF, worst
    assert dc.TOL == 1e-3


def test_cases_cover_what_they_claim():
    hi, lo = dc.MAX_RANGE, dc.MIN_RANGE
    for terrain_kind in dc.TERRAINS:
        ref = {c: dc.reference("80x60", c, terrain_kind) for c in dc.CAMERAS}
        assert (ref["sky"] == hi).all() and (ref["below"] == lo).all()
        assert (ref["nan"][1] == hi).all() and (ref["nan"][0] < hi).any()
        for c in ("down", "forward", "border"):
            assert ((ref[c] > lo) & (ref[c] < hi)).mean() > 0.25, (terrain_kind, c)
    for case in dc.NORM_CASES:                                       # both clips of the normalisation test bite, and some pixels lie between
        r = dc.reference(*case)
        assert (r < dc.NORM_NEAR).any() and (r > dc.NORM_FAR).any() and ((r > dc.NORM_NEAR) & (r < dc.NORM_FAR)).any(), case
    # the transposed grid is a different image (a transposed index shows)
    cam, sc, pos, quat, dirs = dc.case("7x5", "down", "grid")
    sc_t = dict(sc, heightfield=np.ascontiguousarray(sc["heightfield"].T))
    assert np.abs(do.render(cam, sc_t, pos, quat, dirs) - dc.reference("7x5", "down", "grid")).max() > 0.05


def test_argument_errors_are_refused_before_any_launch():
    """Null pointers, non-positive sizes, max_range <= min_range, far_clip <= near_clip and a heightfield the walk cannot bound: each
    returns an error with its own message.  Nothing is launched, so this runs without a GPU (the pointers are never read)."""
    lib = abi.load_lib()
    buf = (C.c_float * 16)()
    ptr = C.addressof(buf)

    def call(cam_kw=None, scene_kw=None, dirs=ptr, out=ptr, cam=True, scene=True):
        cm = abi.LgDepthCam(width=4, height=2, min_range=0.1, max_range=5.0, near_clip=0.0, far_clip=5.0, normalize=1)
        cm.mount_quat[3] = 1.0
        sc = abi.LgDepthScene(n_envs=1, base_pos=ptr, base_quat=ptr, heightfield=ptr, rows=2, cols=2, hscale=0.1, vscale=0.005, border=0.0)
        for k, v in (cam_kw or {}).items():
            setattr(cm, k, v)
        for k, v in (scene_kw or {}).items():
            setattr(sc, k, v)
        rc = lib.lg_depth_render(C.byref(cm) if cam else None, C.byref(sc) if scene else None, dirs, out, None)
        return rc, lib.lg_last_error().decode()

    bad = [(dict(cam=False), "null"), (dict(scene=False), "null"), (dict(dirs=None), "null"), (dict(out=None), "null"),
           (dict(scene_kw={"base_pos": None}), "null base pose"), (dict(scene_kw={"base_quat": None}), "null base pose"),
           (dict(scene_kw={"heightfield": None}), "heightfield"), (dict(scene_kw={"rows": 1}), "heightfield"), (dict(scene_kw={"rows": -3}), "heightfield"),
           (dict(scene_kw={"cols": 1}), "heightfield"), (dict(scene_kw={"hscale": 0.0}), "scales"), (dict(scene_kw={"hscale": float("nan")}), "scales"),
           (dict(scene_kw={"hscale": 1e-4}), "LG_DEPTH_MAX_CELLS"),
           (dict(cam_kw={"width": 0}), "non-positive"), (dict(cam_kw={"height": -1}), "non-positive"), (dict(scene_kw={"n_envs": 0}), "non-positive"),
           (dict(cam_kw={"max_range": 0.1}), "min_range < max_range"), (dict(cam_kw={"max_range": float("nan")}), "min_range < max_range"),
           (dict(cam_kw={"max_range": float("inf")}), "min_range < max_range"), (dict(cam_kw={"min_range": -1.0}), "min_range < max_range"),
           (dict(cam_kw={"far_clip": 0.0}), "near_clip < far_clip"), (dict(cam_kw={"near_clip": 6.0}), "near_clip < far_clip"),
           (dict(cam_kw={"width": 1 << 16, "height": 1 << 15}), "2^31")]
    for kw, msg in bad:
        rc, err = call(**kw)
        assert rc != 0 and err.startswith("lg_depth_render:") and msg in err, (kw, rc, err)

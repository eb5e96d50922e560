"""GPU: the depth camera (include/lgsensor.h, csrc/lg_sensor.hip) against the float64 oracle of tests/depth_oracle.py on the
cases of tests/depth_cases.py, its normalisation, and the sensor through HipSimulator and the env (cadence, checkpoint, off by
default).  Every range comparison is on the raw range (normalize = 0).

Tolerance: 1e-3 m (tests/depth_cases.py: the float32 oracle differs from float64 by ~1e-5 m on these inputs, below the 2.5e-4 m at
which the issue's 1e-3 m would be replaced); at most 0.1 % of a case's pixels may exceed it, and those must still be finite and
inside [min_range, max_range]."""
import numpy as np
import pytest

from tests import depth_cases as dc
from tests import depth_oracle as do

pytestmark = pytest.mark.gpu


def cam_struct(cam):
    from hcr_genesis_lr_cl_amd import abi
    c = abi.LgDepthCam()
    c.width, c.height = int(cam["width"]), int(cam["height"])
    abi.fill_array(c.mount_pos, cam["mount_pos"])
    abi.fill_array(c.mount_quat, cam["mount_quat"])
    c.min_range, c.max_range, c.near_clip, c.far_clip = cam["min_range"], cam["max_range"], cam["near_clip"], cam["far_clip"]
    c.normalize = int(cam["normalize"])
    return c


def cam_dict(c):
    """The oracle's camera from the struct the product built (the float32 numbers the kernel reads)."""
    return {"width": c.width, "height": c.height, "mount_pos": tuple(c.mount_pos), "mount_quat": tuple(c.mount_quat), "min_range": c.min_range,
            "max_range": c.max_range, "near_clip": c.near_clip, "far_clip": c.far_clip, "normalize": c.normalize}


def run_kernel(cam, sc, pos, quat, dirs):
    import torch
    from hcr_genesis_lr_cl_amd import abi, sensor
    lib = abi.load_lib()
    dev = "cuda:0"
    t_pos, t_quat, t_dirs = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) for a in (pos, quat, dirs))
    hf = torch.from_numpy(sc["heightfield"]).to(dev) if sc["heightfield"] is not None else None
    opts = abi.LgSimOptions(hscale=sc["hscale"], vscale=sc["vscale"], border=sc["border"])
    scene = sensor.make_depth_scene(pos.shape[0], t_pos, t_quat, opts, hf)
    out = torch.full((pos.shape[0], cam["height"], cam["width"]), -7.0, device=dev)
    sensor.render(lib, cam_struct(cam), scene, t_dirs, out, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_against(got, want, cam, what):
    diff, beyond, inside = dc.compare(got, want, cam)
    print(f"depth kernel vs f64 oracle: {what}: max diff {diff:.3e} m, {beyond} of {got.size} pixels beyond {dc.TOL} m")
    assert inside, what
    assert beyond <= int(dc.MAX_OUTLIER_SHARE * got.size), (what, diff, beyond)


@pytest.mark.parametrize("shape,camera,terrain_kind", dc.all_cases(), ids=["-".join(c) for c in dc.all_cases()])
def test_kernel_matches_oracle(shape, camera, terrain_kind):
    cam, sc, pos, quat, dirs = dc.case(shape, camera, terrain_kind)
    got = run_kernel(cam, sc, pos, quat, dirs)
    check_against(got, dc.reference(shape, camera, terrain_kind), cam, f"{terrain_kind} {shape} {camera}")


@pytest.mark.parametrize("shape,camera,terrain_kind", dc.NORM_CASES, ids=["-".join(c) for c in dc.NORM_CASES])
def test_normalised_output_is_clip_and_scale_of_raw(shape, camera, terrain_kind):
    """genesis_simulator.py:745-750 in the same launch.  The clips lie inside [min_range, max_range] and every case has ranges on both
    sides of each (tests/depth_cases.py NORM_CASES), so both clips bite."""
    cam, sc, pos, quat, dirs = dc.case(shape, camera, terrain_kind)
    cam = dict(cam, near_clip=dc.NORM_NEAR, far_clip=dc.NORM_FAR)
    raw = run_kernel(cam, sc, pos, quat, dirs)
    got = run_kernel(dict(cam, normalize=1), sc, pos, quat, dirs)
    near, far = np.float32(cam["near_clip"]), np.float32(cam["far_clip"])
    want = (np.clip(raw, near, far) - near) / (far - near) - np.float32(0.5)
    print(f"depth normalised vs formula on raw: {terrain_kind} {shape} {camera}: max diff {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
    assert got.min() == -0.5 and got.max() == 0.5


def make_cfg(task, n, add_depth=True):
    from hcr_genesis_lr_cl_amd.envs import TASKS
    cls, cfg_cls = TASKS[task]
    cfg = cfg_cls()
    cfg.env.num_envs = n
    if cfg.terrain.mesh_type == "heightfield":
        cfg.terrain.num_rows = cfg.terrain.num_cols = 2          # a 2 x 2-tile terrain
        cfg.terrain.max_init_terrain_level = 1
    cfg.sensor.add_depth = add_depth
    c = cfg.sensor.depth_camera_config                           # go2_ts_depth_config.py:155-165, looking forward and down
    c.near_clip, c.far_clip, c.near_plane, c.far_plane = 0.0, 5.0, 0.1, 5.0
    c.fov_horizontal, c.pos, c.euler = 75, (0.3, 0.0, 0.1), (0.0, 0.5, 0.0)
    return cls, cfg


def make_env(task, n, add_depth=True):
    from hcr_genesis_lr_cl_amd.envs import set_seed
    cls, cfg = make_cfg(task, n, add_depth)
    set_seed(int(cfg.seed))
    return cls(cfg, None, "cuda:0", True)


@pytest.mark.parametrize("task", ["go2_ts", "go2"])
def test_simulator_update_sensors_matches_oracle(task):
    """HipSimulator with add_depth: depth_images (N, 1, H, W); one update_sensors() is the oracle's image of the engine's own pose and
    terrain (go2_ts: heightfield; go2: the plane)."""
    import torch
    from hcr_genesis_lr_cl_amd import config as cfgmod
    from hcr_genesis_lr_cl_amd.envs import set_seed
    from hcr_genesis_lr_cl_amd.simulator import HipSimulator
    N = 8
    _, cfg = make_cfg(task, N)
    set_seed(int(cfg.seed))
    sim = HipSimulator(cfg, cfgmod.class_to_dict(cfg.sim), "cuda:0", True)
    assert sim.depth_images.shape == (N, 1, 60, 80) and sim.depth_images.dtype == torch.float32 and not sim.depth_images.any()
    g = torch.Generator().manual_seed(3)
    rpy = (torch.rand(N, 3, generator=g) - 0.5) * torch.tensor([0.4, 0.4, 6.0])
    q = torch.from_numpy(dc.quat_from_euler_xyz(*rpy.double().numpy().T)).float()
    sim.base_quat[:] = q.to("cuda:0")
    sim.base_pos[:, :2] += ((torch.rand(N, 2, generator=g) - 0.5) * 3.0).to("cuda:0")
    sim.base_pos[:, 2] += 0.3
    sim._depth_cam.normalize = 0
    assert sim.update_sensors() is None
    torch.cuda.synchronize()
    raw = sim.depth_images[:, 0].cpu().numpy()
    hf = sim._height_samples.cpu().numpy().astype(np.int16) if task == "go2_ts" else None
    assert (hf is not None) == (sim._depth_scene.rows > 0) and (hf is None or hf.shape == (sim._depth_scene.rows, sim._depth_scene.cols))
    sc = {"heightfield": hf, "hscale": sim._opts.hscale, "vscale": sim._opts.vscale, "border": sim._opts.border}
    cam = cam_dict(sim._depth_cam)
    pos, quat, dirs = sim.base_pos.cpu().numpy(), sim.base_quat.cpu().numpy(), sim._depth_ray_dirs.cpu().numpy()
    want = do.render(cam, sc, pos, quat, dirs, np.float64)
    assert dc.compare(do.render(cam, sc, pos, quat, dirs, np.float32), want, cam)[1:] == (0, True)     # inputs the float32 oracle itself passes
    assert ((want > cam["min_range"]) & (want < cam["max_range"])).mean() > 0.3
    check_against(raw, want, cam, f"simulator {task}")
    sim._depth_cam.normalize = 1                                 # what the task classes read: clipped and normalised
    assert sim.update_depth_images() is None and sim.draw_debug_depth_images() is None
    torch.cuda.synchronize()
    np.testing.assert_allclose(sim.depth_images[:, 0].cpu().numpy(), do.normalize(cam, raw, np.float32), rtol=0, atol=1e-6)


@pytest.fixture(scope="module")
def rollout():
    """20 env steps of go2_ts with the depth camera: the image and the counter after every step, and a checkpoint taken after step 9."""
    import torch
    N = 8
    env = make_env("go2_ts", N)
    env.reset_idx(torch.arange(N, device="cuda:0"))
    g = torch.Generator(device="cuda:0").manual_seed(11)
    acts = [torch.randn(N, env.num_actions, generator=g, device="cuda:0") for _ in range(20)]
    assert env.depth_images.shape == (N, 1, 60, 80) and not env.depth_images.any() and env.depth_image_update_counter == 0
    images, counters, sd = [], [], None
    for k, a in enumerate(acts, 1):
        env.step(a)
        images.append(env.depth_images.clone())
        counters.append(env.depth_image_update_counter)
        if k == 9:
            sd = env.state_dict()
    torch.cuda.synchronize()
    return {"acts": acts, "images": images, "counters": counters, "sd": sd, "N": N}


def test_env_renders_at_steps_7_13_19(rollout):
    import torch
    images = rollout["images"]
    prev, changed = torch.zeros_like(images[0]), []
    for k, img in enumerate(images, 1):
        if not torch.equal(img, prev):
            changed.append(k)
        prev = img
    assert changed == [7, 13, 19]
    assert rollout["counters"][5:8] == [6, 1, 2]
    last = images[-1]
    assert torch.isfinite(last).all() and last.min() >= -0.5 and last.max() <= 0.5 and last.std() > 0.01


def test_env_checkpoint_resumes_depth_bit_exact(rollout, tmp_path):
    import torch
    path = str(tmp_path / "depth_ckpt.pt")
    torch.save(rollout["sd"], path)
    env = make_env("go2_ts", rollout["N"])
    env.reset_idx(torch.arange(rollout["N"], device="cuda:0"))
    env.load_checkpoint(path)
    assert env.depth_image_update_counter == rollout["counters"][8] and torch.equal(env.depth_images, rollout["images"][8])
    for k in range(10, 21):
        env.step(rollout["acts"][k - 1])
        assert env.depth_image_update_counter == rollout["counters"][k - 1], k
        assert torch.equal(env.depth_images, rollout["images"][k - 1]), k
    with pytest.raises(ValueError, match="add_depth"):
        make_env("go2_ts", rollout["N"], add_depth=False).load_checkpoint(path)


def test_without_add_depth_nothing_changes():
    import torch
    env = make_env("go2", 8, add_depth=False)
    assert env.simulator.depth_images is None and env.depth_images is None
    assert env.simulator.update_sensors() is None and env.simulator.update_depth_images() is None
    env.reset()
    for _ in range(8):
        env.step(torch.zeros(8, env.num_actions, device="cuda:0"))
    assert env.depth_images is None and "depth" not in env.state_dict()


def test_num_history_other_than_one_is_refused():
    cls, cfg = make_cfg("go2", 8)
    cfg.sensor.depth_camera_config.num_history = 2
    with pytest.raises(ValueError, match="num_history"):
        cls(cfg, None, "cuda:0", True)

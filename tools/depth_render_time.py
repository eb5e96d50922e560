"""Developer tool (GPU only, never read by bench.py): time of the depth camera's render launch (`lg_depth_render`, include/lgsensor.h) at
the size a vision student is trained at: 4096 envs, 80 x 60 pixels, on go2_ts's curriculum heightfield (10 x 10 tiles of 8 m, 0.1 m
cells), robots standing at their env origins with a random heading and a small random tilt.

Two mounts are timed, because the length of the cell walk depends on where the camera looks: the reference's depth task
(go2_ts_depth_config.py:155-165: far plane 5 m, euler (0, 1.57, 0), i.e. straight down) and the same camera pitched 0.3 rad below the
horizon (rays that run out to the far plane).  Kernel time is taken from device events around `--iters` back-to-back launches after a
warm-up, repeated `--repeats` times; the median and the spread are printed.  From it: rays per second, and the bytes of the image
written per second as a share of this device's measured stream-copy bandwidth (`lg_stream_copy`, read + write bytes per second) -- the
kernel is a latency-bound gather, so that share says how far from a pure streaming write it runs, not how well it does.

    python tools/depth_render_time.py [--envs 4096] [--iters 200] [--repeats 7]

Prints a table and one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("depth_render_time.py: no GPU -- a time is only measured on the device")
    from hcr_genesis_lr_cl_amd import abi, sensor
    from hcr_genesis_lr_cl_amd import build as b
    from hcr_genesis_lr_cl_amd import config as cfgmod
    from hcr_genesis_lr_cl_amd.envs import set_seed
    from hcr_genesis_lr_cl_amd.simulator import HipSimulator
    N, dev = args.envs, "cuda:0"
    cfg = cfgmod.GO2TSCfg()
    cfg.env.num_envs = N
    cfg.sensor.add_depth = True
    c = cfg.sensor.depth_camera_config
    c.near_clip, c.far_clip, c.near_plane, c.far_plane, c.fov_horizontal = 0.0, 5.0, 0.1, 5.0, 75
    set_seed(int(cfg.seed))
    sim = HipSimulator(cfg, cfgmod.class_to_dict(cfg.sim), dev, True)
    g = torch.Generator().manual_seed(1)
    rpy = (torch.rand(N, 3, generator=g, dtype=torch.float64) - 0.5) * torch.tensor([0.3, 0.3, 6.28], dtype=torch.float64)
    cy, sy, cr, sr, cp, sp = (f(rpy[:, k] * 0.5) for k in (2, 0, 1) for f in (torch.cos, torch.sin))
    sim.base_quat[:] = torch.stack([cy * sr * cp - sy * cr * sp, cy * cr * sp + sy * sr * cp, sy * cr * cp - cy * sr * sp,
                                    cy * cr * cp + sy * sr * sp], 1).float().to(dev)
    lib, stream = sim._engine.lib, torch.cuda.current_stream().cuda_stream
    H, W = sim.depth_images.shape[2:]
    out_bytes = sim.depth_images.numel() * 4
    src, dst = torch.empty(1 << 28, dtype=torch.uint8, device=dev), torch.empty(1 << 28, dtype=torch.uint8, device=dev)
    gbs = C.c_float()
    abi.check(lib.lg_stream_copy(src.data_ptr(), dst.data_ptr(), src.numel(), 20, stream, C.byref(gbs)), lib)
    copy_bw = gbs.value * 1e9
    del src, dst
    res = dict(tool="depth_render_time", envs=N, width=W, height=H, rays=N * H * W, out_bytes=out_bytes, iters=args.iters, repeats=args.repeats,
               heightfield=[sim._depth_scene.rows, sim._depth_scene.cols], stream_copy_bytes_per_s=copy_bw, source_hash=b.source_hash(),
               device=torch.cuda.get_device_name(0), mounts={})
    print(f"{N} envs x {W} x {H} = {N * H * W / 1e6:.2f} M rays, {out_bytes / 1e6:.1f} MB image, heightfield {sim._depth_scene.rows} x {sim._depth_scene.cols}, "
          f"stream copy {copy_bw / 1e12:.2f} TB/s (read + write)")
    for name, pitch in (("down (go2_ts_depth: euler 0, 1.57, 0)", 1.57), ("forward (pitch 0.3)", 0.3)):
        abi.fill_array(sim._depth_cam.mount_quat, sensor.quat_from_euler_xyz(0.0, pitch, 0.0))
        for _ in range(args.warmup):
            sim.update_depth_images()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                sim.update_depth_images()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / args.iters)
        med = statistics.median(us)
        img = sim.depth_images
        hit = float(((img > -0.5) & (img < 0.5)).float().mean())
        r = dict(us_per_render=dict(median=med, min=min(us), max=max(us)), rays_per_s=N * H * W / (med * 1e-6),
                 out_bytes_per_s=out_bytes / (med * 1e-6), share_of_stream_copy=out_bytes / (med * 1e-6) / copy_bw, share_of_rays_that_hit=hit)
        res["mounts"][name] = r
        print(f"  {name:40s}: median {med:8.1f} us  (min {min(us):8.1f}, max {max(us):8.1f})   {r['rays_per_s'] / 1e9:6.2f} G rays/s   "
              f"image written at {r['out_bytes_per_s'] / 1e12:.3f} TB/s = {100 * r['share_of_stream_copy']:.1f} % of stream copy   {100 * hit:.0f} % of rays hit")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time of the ray-cast scene generator, none asserted:
  (a) v2x_lidar_cast alone (both launches, HIP events, buffers allocated once) at 10 and at 640 sweeps of 32 x 2048 rays against make_world's scenes
      (24 cars + 8 walls per frame), with the returns per sweep and the ray-box tests per second;
  (b) a 2-frame x 5-agent batch, host clock from idle device to idle device: utils/raycast_scene.raycast_batch_on_device (make_world on the host, then
      cast, visible boxes, voxelise, densify, IoU targets on the device) against train/loop.synthetic_batch_on_device(targets="iou") (make_scene's host
      loop, upload, voxelise, densify, IoU targets).  The two ALTERNATE in one process, a fresh seed per repeat, medians over the repeats, and the
      ratio ray-cast / sampled;
  (c) the training step those batches feed (FaFNet, 5 agents x 2 frames, the hipGraph engine) on the same clock, and each generator's share of a step.

    python3 tools/lidar_bench.py [--repeats 24] [--out profiles/lidar_cast_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", default=5, type=int)
    ap.add_argument("--frames", default=2, type=int)
    ap.add_argument("--sweeps", default=[10, 640], type=int, nargs="+", help="sweeps per call of (a) (multiples of --agents)")
    ap.add_argument("--iters", default=10, type=int)
    ap.add_argument("--rounds", default=5, type=int)
    ap.add_argument("--repeats", default=24, type=int, help="alternations of (b), at least 20")
    ap.add_argument("--steps", default=20, type=int, help="training steps timed in (c)")
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--out", default="", type=str)
    args = ap.parse_args(argv)
    from v2x_sim_amd import ops, tuning
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.det import FaFNet
    from v2x_sim_amd.train.loop import init_for_training, make_optimizer, synthetic_batch_on_device
    from v2x_sim_amd.utils import postprocess, raycast_scene
    from v2x_sim_amd.utils.CoDetModule import FaFModule
    if not torch.cuda.is_available():
        raise SystemExit("lidar_bench.py measures on the MI355X: no GPU, no figure")
    dev = torch.device("cuda:0")
    cfg = Config("train", binary=True, only_det=True)
    grid = ops.VoxelGrid(cfg.voxel_size, cfg.area_extents)
    anchors = postprocess.build_anchor_map(cfg)
    med = lambda v: float(np.median(v))
    beams, steps = 32, 2048
    lines = ["ray-cast scenes: %d x %d rays per sweep, make_world's 24 cars + 8 walls per frame, on %s" % (beams, steps, torch.cuda.get_device_name(0))]

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.iters

    # ---- (a) the cast alone
    beam, az = (torch.from_numpy(t).to(dev) for t in ops.ring_table(beams, steps))
    for n in args.sweeps:
        world = raycast_scene.make_world(n // args.agents, args.agents, seed=args.seed)
        d = raycast_scene.world_on_device(world, dev)
        kw = dict(ground_z=raycast_scene.GROUND_Z, sigma_r=0.02, seed=args.seed)
        out = ops.lidar_cast(d["sensors"], d["frame_of"], d["boxes"], d["box_count"], beam, az, beams * steps, **kw)
        call = lambda: ops.lidar_cast(d["sensors"], d["frame_of"], d["boxes"], d["box_count"], beam, az, beams * steps, out=out, **kw)
        events(call)
        t = [events(call) for _ in range(args.rounds)]
        tests = float(n) * beams * steps * float(world["box_count"].mean())
        lines += ["",
                  "(a) v2x_lidar_cast alone, %d sweeps (%d agents x %d frames), points + hit + box_hits (2 launches, HIP events, %d calls): %9.1f us per call   "
                  "[rounds: %s]" % (n, args.agents, n // args.agents, args.iters, med(t), " ".join("%.1f" % v for v in t)),
                  "    %.0f returns per sweep of %d rays; %.2f G ray-box tests per call = %.1f G tests/s; workspace %.1f MB"
                  % (float(out["n_pts"].float().mean()), beams * steps, tests / 1e9, tests / (med(t) * 1e-6) / 1e9,
                     ops._lib.load().v2x_lidar_cast_workspace_size(n, beams, steps, int(d["boxes"].shape[1])) / 1e6)]
        del out

    # ---- (b) a batch from each generator, alternating
    def raycast(seed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data = synthetic_batch_on_device(cfg, args.frames, args.agents, seed, dev, grid, anchors, scene="raycast")
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), data

    def sampled(seed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        data = synthetic_batch_on_device(cfg, args.frames, args.agents, seed, dev, grid, anchors, targets="iou")
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), data

    for warm in range(3):
        raycast(1000 + warm), sampled(1000 + warm)
    t_ray, t_smp = [], []
    for rep in range(max(args.repeats, 20)):
        t_ray.append(raycast(args.seed * 7919 + rep)[0])
        t_smp.append(sampled(args.seed * 7919 + rep)[0])
    ratio = med(t_ray) / med(t_smp)
    _, d_ray = raycast(args.seed)
    _, d_smp = sampled(args.seed)
    occ = lambda data: float(data["bev_seq"].sum()) / data["bev_seq"].shape[0]
    pos = lambda data: float(data["labels"][..., 1].sum()) / data["labels"].shape[0]
    lines += ["",
              "(b) one batch of %d frames x %d agents, host clock, device idle before and after, %d alternations in one process" % (args.frames, args.agents, len(t_ray)),
              "    raycast_batch_on_device (make_world + 5 device calls)                    : %9.2f ms per batch   [min %.2f, max %.2f]"
              % (med(t_ray), min(t_ray), max(t_ray)),
              "    synthetic_batch_on_device(targets=\"iou\") (make_scene's host loop + upload) : %9.2f ms per batch   [min %.2f, max %.2f]"
              % (med(t_smp), min(t_smp), max(t_smp)),
              "    ray-cast / sampled = %.3f" % ratio,
              "    per item: %.0f occupied voxels and %.1f positive anchors ray-cast, %.0f and %.1f sampled" % (occ(d_ray), pos(d_ray), occ(d_smp), pos(d_smp))]

    # ---- (c) the step they feed
    tuning.set("TRAIN_HIP", 1)
    tuning.set("TRAIN_GRAPH", 1)
    model = init_for_training(FaFNet(cfg, kd_flag=0, num_agent=args.agents), seed=1).to(dev)
    opt, _ = make_optimizer(model, 1e-3, 1000)
    module = FaFModule(model, None, cfg, opt, 0)
    for _ in range(5):
        module.step(d_ray, args.frames, args.agents)
    t_step = []
    for _ in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        module.step(d_ray, args.frames, args.agents)
        torch.cuda.synchronize()
        t_step.append(1e3 * (time.perf_counter() - t0))
    lines += ["",
              "(c) FaFModule.step on that batch (FaFNet, hipGraph engine), the same clock            : %9.2f ms per step    [min %.2f, max %.2f]"
              % (med(t_step), min(t_step), max(t_step)),
              "    a ray-cast batch is %.2f of a step, a sampled batch %.2f of a step" % (med(t_ray) / med(t_step), med(t_smp) / med(t_step))]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

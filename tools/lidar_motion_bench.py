#!/usr/bin/env python3
"""Time of the MOVING ray cast (DESIGN.md section 3.12 "moving scenes"), none asserted:
  (a) v2x_lidar_cast_moving against v2x_lidar_cast on the same world with all velocities zero (the same bytes), at 10 and at 640 sweeps of 32 x 2048
      rays against make_world's scenes -- the shapes of profiles/lidar_cast_bench.txt.  The two ALTERNATE in one process, round by round (HIP events
      around `--iters` calls, buffers allocated once); medians over the rounds and the ratio moving / static;
  (b) a scenes=2, steps=10, agents=5 sequence end to end, host clock from idle device to idle device: make_moving_world on the host, then
      utils/raycast_scene.raycast_sequence_on_device (one cast, one ground-truth call, voxelise, densify, IoU targets: 100 maps), a fresh seed per repeat;
  (c) the training step one item group of it feeds (FaFNet, 5 agents x 2 items, the hipGraph engine) on the same clock.

    python3 tools/lidar_motion_bench.py [--out profiles/lidar_motion_bench.txt]
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
    ap.add_argument("--sweeps", default=[10, 640], type=int, nargs="+", help="sweeps per call of (a) (multiples of --agents)")
    ap.add_argument("--iters", default=10, type=int)
    ap.add_argument("--rounds", default=7, type=int)
    ap.add_argument("--scenes", default=2, type=int)
    ap.add_argument("--seq_steps", default=10, type=int)
    ap.add_argument("--repeats", default=20, type=int)
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
        raise SystemExit("lidar_motion_bench.py measures on the MI355X: no GPU, no figure")
    dev = torch.device("cuda:0")
    cfg = Config("train", binary=True, only_det=True)
    grid = ops.VoxelGrid(cfg.voxel_size, cfg.area_extents)
    anchors = postprocess.build_anchor_map(cfg)
    med = lambda v: float(np.median(v))
    beams, steps = 32, 2048
    lines = ["moving ray cast: %d x %d rays per sweep, make_world's 24 cars + 8 walls per frame, on %s" % (beams, steps, torch.cuda.get_device_name(0))]

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.iters

    # ---- (a) moving against static on the same world, alternating
    beam, az = (torch.from_numpy(t).to(dev) for t in ops.ring_table(beams, steps))
    az_time = torch.from_numpy(ops.az_time_table(steps, 0.1)).to(dev)
    for n in args.sweeps:
        world = raycast_scene.make_world(n // args.agents, args.agents, seed=args.seed)
        d = raycast_scene.world_on_device(world, dev)
        F, cap = d["boxes"].shape[:2]
        svel, bvel = torch.zeros((n, 2), device=dev), torch.zeros((F, cap, 2), device=dev)
        time_of = torch.full((n,), 0.4, device=dev)
        kw = dict(ground_z=raycast_scene.GROUND_Z, sigma_r=0.02, seed=args.seed)
        out_s = ops.lidar_cast(d["sensors"], d["frame_of"], d["boxes"], d["box_count"], beam, az, beams * steps, **kw)
        out_m = ops.lidar_cast_moving(d["sensors"], svel, time_of, d["frame_of"], d["boxes"], bvel, d["box_count"], beam, az, az_time, beams * steps, **kw)
        same = all(torch.equal(out_s[k], out_m[k]) for k in out_s)
        static = lambda: ops.lidar_cast(d["sensors"], d["frame_of"], d["boxes"], d["box_count"], beam, az, beams * steps, out=out_s, **kw)
        moving = lambda: ops.lidar_cast_moving(d["sensors"], svel, time_of, d["frame_of"], d["boxes"], bvel, d["box_count"], beam, az, az_time,
                                               beams * steps, out=out_m, **kw)
        events(static), events(moving)
        t_s, t_m = [], []
        for _ in range(args.rounds):
            t_s.append(events(static))
            t_m.append(events(moving))
        lines += ["",
                  "(a) %d sweeps (%d agents x %d frames), points + hit + box_hits, 2 launches each, HIP events around %d calls, %d alternating rounds; "
                  "outputs identical: %s" % (n, args.agents, n // args.agents, args.iters, args.rounds, same),
                  "    v2x_lidar_cast        : %9.1f us per call   [rounds: %s]" % (med(t_s), " ".join("%.1f" % v for v in t_s)),
                  "    v2x_lidar_cast_moving : %9.1f us per call   [rounds: %s]" % (med(t_m), " ".join("%.1f" % v for v in t_m)),
                  "    moving / static = %.3f" % (med(t_m) / med(t_s))]
        del out_s, out_m

    # ---- (b) a sequence end to end
    def sequence(seed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        world = raycast_scene.make_moving_world(args.scenes, args.agents, seed)
        t1 = time.perf_counter()
        data = raycast_scene.raycast_sequence_on_device(cfg, world, args.seq_steps, device=dev, grid=grid, anchors=anchors, seed=seed)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), 1e3 * (t1 - t0), data

    for warm in range(3):
        sequence(1000 + warm)
    runs = [sequence(args.seed * 7919 + rep) for rep in range(args.repeats)]
    t_seq, t_world = [r[0] for r in runs], [r[1] for r in runs]
    data = runs[-1][2]
    maps = data["bev_seq"].shape[0]
    lines += ["",
              "(b) a sequence of %d scenes x %d steps x %d agents = %d maps, host clock, device idle before and after, %d repeats"
              % (args.scenes, args.seq_steps, args.agents, maps, len(t_seq)),
              "    make_moving_world + raycast_sequence_on_device : %9.2f ms per sequence [min %.2f, max %.2f] = %.3f ms per map; make_moving_world alone %.2f ms"
              % (med(t_seq), min(t_seq), max(t_seq), med(t_seq) / maps, med(t_world)),
              "    per map: %.0f occupied voxels, %.1f positive anchors, %.1f ground-truth boxes"
              % (float(data["bev_seq"].sum()) / maps, float(data["labels"][..., 1].sum()) / maps, float(data["gt_count"].sum()) / maps)]

    # ---- (c) the step such a batch feeds
    tuning.set("TRAIN_HIP", 1)
    tuning.set("TRAIN_GRAPH", 1)
    batch = synthetic_batch_on_device(cfg, 2, args.agents, args.seed, dev, grid, anchors, scene="raycast-moving")
    model = init_for_training(FaFNet(cfg, kd_flag=0, num_agent=args.agents), seed=1).to(dev)
    opt, _ = make_optimizer(model, 1e-3, 1000)
    module = FaFModule(model, None, cfg, opt, 0)
    for _ in range(5):
        module.step(batch, 2, args.agents)
    t_step = []
    for _ in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        module.step(batch, 2, args.agents)
        torch.cuda.synchronize()
        t_step.append(1e3 * (time.perf_counter() - t0))
    lines += ["",
              "(c) FaFModule.step on 2 items x %d agents of a moving world (FaFNet, hipGraph engine), the same clock : %9.2f ms per step [min %.2f, max %.2f]"
              % (args.agents, med(t_step), min(t_step), max(t_step)),
              "    the sequence costs %.2f of a step per 10 maps" % (med(t_seq) / maps * 10 / med(t_step))]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

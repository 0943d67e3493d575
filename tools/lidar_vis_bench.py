#!/usr/bin/env python3
"""Time of the free-space ray walk, none asserted, on the product grid 256 x 256 x 13 with sweeps of 32 x 2048 rays cast
against make_world's scenes (24 cars + 8 walls per frame):
  (a) at 10 and at 640 sweeps, HIP events, buffers allocated once, the four calls ALTERNATING round by round in one process: v2x_lidar_cast and
      v2x_voxelize_bits (the yardsticks, unchanged code) and v2x_lidar_freespace_bits in its two forms on the same clouds -- the LDS form the shape
      selects, and the general form, reached by handing the same call an output 4 bytes off a 16-byte boundary (the LDS form stores 16-byte words,
      so the shape rule gives such a call to the device-scope atomics: same grid, same rays, same bytes);
  (b) the "any" form of a 2-frame x 5-agent batch: 50 jobs into 10 ego grids, both forms, beside v2x_voxelize_fused_bits on the same jobs;
  (c) a segmentation batch of 2 frames x 5 agents end to end, host clock from idle device to idle device, alternating:
      utils/raycast_scene.raycast_seg_batch_on_device (observed "own" and "any") against tools/seg/train_seg.py::seg_batch on the sampled scenes, and
      the free-space call's share of the ray-cast batch.

    python3 tools/lidar_vis_bench.py [--out profiles/lidar_vis_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd"), os.path.join(ROOT, "tools", "seg")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", default=5, type=int)
    ap.add_argument("--frames", default=2, type=int)
    ap.add_argument("--sweeps", default=[10, 640], type=int, nargs="+", help="sweeps per call of (a) (multiples of --agents)")
    ap.add_argument("--iters", default=5, type=int)
    ap.add_argument("--rounds", default=7, type=int)
    ap.add_argument("--repeats", default=20, type=int, help="alternations of (c)")
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--out", default="", type=str)
    args = ap.parse_args(argv)
    from train_seg import seg_batch
    from v2x_sim_amd import ops
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.utils import raycast_scene
    if not torch.cuda.is_available():
        raise SystemExit("lidar_vis_bench.py measures on the MI355X: no GPU, no figure")
    dev = torch.device("cuda:0")
    cfg = Config("train", binary=True, only_det=True)
    grid = ops.VoxelGrid(cfg.voxel_size, cfg.area_extents)
    X, Y, Z = grid.dims
    med = lambda v: float(np.median(v))
    beams, steps = 32, 2048
    lines = ["free-space ray walk: %d x %d rays per sweep, grid %d x %d x %d, make_world's 24 cars + 8 walls per frame, on %s"
             % (beams, steps, X, Y, Z, torch.cuda.get_device_name(0))]

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.iters

    def misaligned(n):
        buf = torch.empty((n * X * Y + 4,), dtype=torch.int32, device=dev)
        off = next(o for o in range(1, 5) if (buf.data_ptr() + 4 * o) % 16 == 4)
        return buf[off:off + n * X * Y].view(n, X, Y)

    def alternate(calls):
        for fn in calls.values():
            events(fn)                                                 # warm-up: code objects, the LDS opt-in
        t = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, fn in calls.items():
                t[k].append(events(fn))
        return t

    def row(name, t):
        return "    %-58s: %10.1f us per call   [rounds: %s]" % (name, med(t), " ".join("%.1f" % v for v in t))

    beam, az = (torch.from_numpy(t).to(dev) for t in ops.ring_table(beams, steps))
    t_free10 = None
    for n in args.sweeps:
        world = raycast_scene.make_world(n // args.agents, args.agents, seed=args.seed)
        d = raycast_scene.world_on_device(world, dev)
        kw = dict(ground_z=raycast_scene.GROUND_Z, sigma_r=0.02, seed=args.seed)
        out = ops.lidar_cast(d["sensors"], d["frame_of"], d["boxes"], d["box_count"], beam, az, beams * steps, **kw)
        pts, cnt = out["points"], out["n_pts"]
        occ = torch.empty((n, X, Y), dtype=torch.int32, device=dev)
        lds, gen = torch.empty((n, X, Y), dtype=torch.int32, device=dev), misaligned(n)
        t = alternate({
            "cast": lambda: ops.lidar_cast(d["sensors"], d["frame_of"], d["boxes"], d["box_count"], beam, az, beams * steps, out=out, **kw),
            "vox": lambda: ops.voxelize_bits(pts, cnt, grid, out=occ),
            "lds": lambda: ops.freespace_bits(pts, cnt, grid, out=lds),
            "gen": lambda: ops.freespace_bits(pts, cnt, grid, out=gen),
        })
        torch.cuda.synchronize()
        assert torch.equal(lds, gen), "the two forms differ"
        rays = float(cnt.float().sum())
        vox_set = float(sum(int(((lds >> z) & 1).sum()) for z in range(Z)))
        if n == 10:
            t_free10 = med(t["lds"])
        lines += ["", "(a) %d sweeps (%d agents x %d frames), HIP events, %d calls per round, the four alternating:" % (n, args.agents, n // args.agents, args.iters),
                  row("v2x_lidar_cast (points + hit + box_hits)", t["cast"]), row("v2x_voxelize_bits on its clouds", t["vox"]),
                  row("v2x_lidar_freespace_bits, LDS form (16-row bands)", t["lds"]), row("v2x_lidar_freespace_bits, general form (misaligned output)", t["gen"]),
                  "    LDS / general = %.3f; spread of the LDS rounds %.1f %%, of the general rounds %.1f %%"
                  % (med(t["lds"]) / med(t["gen"]), 100 * (max(t["lds"]) - min(t["lds"])) / med(t["lds"]), 100 * (max(t["gen"]) - min(t["gen"])) / med(t["gen"])),
                  "    %.0f rays per call, %.1f M rays/s in the LDS form; %.0f voxels traversed per sweep of %d (%.1f %%); free-space / cast = %.2f, / voxelize = %.1f"
                  % (rays, rays / med(t["lds"]), vox_set / n, X * Y * Z, 100 * vox_set / n / (X * Y * Z), med(t["lds"]) / med(t["cast"]),
                     med(t["lds"]) / med(t["vox"]))]
        if n == args.agents * args.frames:
            # ---- (b) the "any" form on the same clouds
            xf, src, dst = (torch.from_numpy(a).to(dev) for a in raycast_scene.fused_jobs(world, args.frames, args.agents))
            t = alternate({
                "fused": lambda: ops.voxelize_fused_bits(pts, cnt, xf, src, dst, n, grid),
                "lds": lambda: ops.freespace_bits(pts, cnt, grid, xform=xf, src_cloud=src, dst_grid=dst, n_grids=n, out=lds),
                "gen": lambda: ops.freespace_bits(pts, cnt, grid, xform=xf, src_cloud=src, dst_grid=dst, n_grids=n, out=gen),
            })
            torch.cuda.synchronize()
            assert torch.equal(lds, gen), "the two forms differ"
            lines += ["", "(b) the \"any\" form: %d jobs (every agent of a frame into every ego grid) into %d grids, the three alternating:" % (len(src), n),
                      row("v2x_voxelize_fused_bits on the same jobs (allocates its output)", t["fused"]),
                      row("v2x_lidar_freespace_bits, LDS form", t["lds"]), row("v2x_lidar_freespace_bits, general form", t["gen"]),
                      "    LDS / general = %.3f" % (med(t["lds"]) / med(t["gen"]))]
        del out, pts, cnt, occ, lds, gen

    # ---- (c) a segmentation batch end to end
    def clock(fn, seed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(seed)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    gens = {
        "own": lambda s: raycast_scene.raycast_seg_batch_on_device(cfg, args.frames, args.agents, s, dev, observed="own", grid=grid),
        "any": lambda s: raycast_scene.raycast_seg_batch_on_device(cfg, args.frames, args.agents, s, dev, observed="any", grid=grid),
        "all": lambda s: raycast_scene.raycast_seg_batch_on_device(cfg, args.frames, args.agents, s, dev, observed="all", grid=grid),
        "sampled": lambda s: seg_batch(cfg, args.frames, args.agents, s, dev, grid),
    }
    for warm in range(3):
        for fn in gens.values():
            clock(fn, 1000 + warm)
    t = {k: [] for k in gens}
    for rep in range(max(args.repeats, 20)):
        for k, fn in gens.items():
            t[k].append(clock(fn, args.seed * 7919 + rep))
    lab = gens["own"](args.seed)["labels"]
    lines += ["", "(c) one segmentation batch of %d frames x %d agents, host clock, device idle before and after, %d alternations in one process"
              % (args.frames, args.agents, len(t["own"]))]
    for k, what in (("own", "raycast_seg_batch_on_device(observed=\"own\")"), ("any", "raycast_seg_batch_on_device(observed=\"any\")"),
                    ("all", "raycast_seg_batch_on_device(observed=\"all\")"), ("sampled", "train_seg.seg_batch on the sampled scenes (host label maps)")):
        lines.append("    %-58s: %10.2f ms per batch   [min %.2f, max %.2f]" % (what, med(t[k]), min(t[k]), max(t[k])))
    lines.append("    ray-cast own / sampled = %.3f, any / sampled = %.3f; %.1f %% of the cells of an \"own\" batch are the ignore class"
                 % (med(t["own"]) / med(t["sampled"]), med(t["any"]) / med(t["sampled"]), 100 * float((lab == 255).float().mean())))
    if t_free10 is not None:
        lines.append("    the free-space call of (a) at 10 sweeps, %.1f us, is %.1f %% of an \"own\" batch" % (t_free10, 100 * t_free10 * 1e-3 / med(t["own"])))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

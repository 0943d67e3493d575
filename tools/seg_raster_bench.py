#!/usr/bin/env python3
"""Time of the segmentation labels of a step at 10 and 40 maps of 256 x 256 (5 agents x 2 and x 8 frames), none asserted, for two
loads: the synthetic scenes' boxes, and 64 random boxes per item (1-8 m extents, classes 1-7, all inside the grid):
  (a) today's path: utils/synthetic_scene.seg_labels per item on the host + stack + upload + synchronise (host clock, the device idle before and
      after).  seg_labels knows one class: the 64-box load is painted as class 1 there, the time is what the loop costs;
  (b) pad + upload of the boxes + ops.rasterize_seg (csrc/seg_raster.hip; labels only, as a training step needs them) + synchronise, the same clock;
      and the ratio (b) / (a);
  (c) the call alone on HIP events into buffers allocated once (labels + hist: both launches), next to the same call with every count 0 -- the fixed
      cost: every output element is written whatever the boxes are;
  (d) the label bytes written per call as a fraction of what v2x_calib_stream writes (the write ceiling).
Several rounds each, medians, every round shown.

    python3 tools/seg_raster_bench.py [--items 10 40] [--out profiles/seg_raster_bench.txt]
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
    ap.add_argument("--items", default=[10, 40], type=int, nargs="+", help="maps per call (multiples of --agents)")
    ap.add_argument("--iters", default=50, type=int)
    ap.add_argument("--rounds", default=5, type=int)
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--out", default="", type=str)
    args = ap.parse_args(argv)
    from v2x_sim_amd import calibrate, ops
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.utils import synthetic_scene
    if not torch.cuda.is_available():
        raise SystemExit("seg_raster_bench.py measures on the MI355X: no GPU, no figure")
    dev = torch.device("cuda:0")
    cfg = Config("train", binary=True, only_det=True)
    X, Y = cfg.map_dims[:2]
    med = lambda v: float(np.median(v))
    write_tbs = max(calibrate.stream_rate(0, 1, total_bytes=1 << 30, wg_per_cu=w, device=dev) for w in (2, 4, 8))
    lines = ["segmentation labels of one training step, grid %d x %d, 8 classes, on %s" % (X, Y, torch.cuda.get_device_name(0)),
             "write ceiling: v2x_calib_stream 0 read : 1 write, 1 GiB, best of 2 / 4 / 8 workgroups per CU: %.2f TB/s" % write_tbs]

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.iters

    def host_clock(fn):
        fn()
        t = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t.append(1e3 * (time.perf_counter() - t0))
        return t

    rng = np.random.default_rng(args.seed)
    for n in args.items:
        frames = n // args.agents
        b = synthetic_scene.make_batch(frames, args.agents, seed=args.seed, ground_pts=10, clutter_pts=10, pts_per_car=4)
        scene_lists = [np.asarray(b["gt_boxes"][a][f], np.float32).reshape(-1, 5) for a in range(args.agents) for f in range(frames)]
        dense_lists = [np.concatenate([rng.uniform(-28, 28, (64, 2)), rng.uniform(1, 8, (64, 2)), rng.uniform(-3.2, 3.2, (64, 1))], 1).astype(np.float32)
                       for _ in range(n)]
        dense_cls = [rng.integers(1, 8, 64).astype(np.uint8) for _ in range(n)]
        for what, lists, classes in (("the synthetic scenes' boxes", scene_lists, None), ("64 boxes per item", dense_lists, dense_cls)):
            n_boxes = sum(g.shape[0] for g in lists)

            def host_path():
                labels = np.stack([synthetic_scene.seg_labels(g, cfg) for g in lists])
                out = torch.from_numpy(labels).to(dev)
                torch.cuda.synchronize()
                return out

            def device_path():
                boxes, cls, count = ops.pad_box_lists(lists, classes)
                res = ops.rasterize_seg(torch.from_numpy(boxes).to(dev), torch.from_numpy(cls).to(dev), torch.from_numpy(count).to(dev), cfg, want=())
                torch.cuda.synchronize()
                return res["labels"]

            host_labels, dev_labels = host_path(), device_path()
            same = bool(torch.equal(host_labels != 0, dev_labels != 0))
            t_host, t_dev = host_clock(host_path), host_clock(device_path)
            boxes, cls, count = ops.pad_box_lists(lists, classes)
            d_boxes, d_cls, d_count = torch.from_numpy(boxes).to(dev), torch.from_numpy(cls).to(dev), torch.from_numpy(count).to(dev)
            d_zero = torch.zeros_like(d_count)
            out = ops.rasterize_seg(d_boxes, d_cls, d_count, cfg, want=("hist",))
            call = lambda: ops.rasterize_seg(d_boxes, d_cls, d_count, cfg, want=("hist",), out=out)
            empty = lambda: ops.rasterize_seg(d_boxes, d_cls, d_zero, cfg, want=("hist",), out=out)
            events(call), events(empty)
            t_call, t_empty = [events(call) for _ in range(args.rounds)], [events(empty) for _ in range(args.rounds)]
            covered = float((dev_labels != 0).float().mean())
            nbytes = float(n * X * Y)
            rate, rate_empty = nbytes / (med(t_call) * 1e-6) / 1e12, nbytes / (med(t_empty) * 1e-6) / 1e12
            lines += ["",
                      "%d maps (%d agents x %d frames), %s: %d boxes (cap %d), %.1f %% of the cells covered; covered cells equal on both paths: %s"
                      % (n, args.agents, frames, what, n_boxes, boxes.shape[1], 100 * covered, same),
                      "(a) seg_labels per item + stack + upload + synchronise, host clock             : %9.2f ms per step   [rounds: %s]"
                      % (med(t_host), " ".join("%.2f" % v for v in t_host)),
                      "(b) pad + upload + v2x_seg_rasterize + synchronise, host clock                 : %9.2f ms per step   [rounds: %s]"
                      % (med(t_dev), " ".join("%.2f" % v for v in t_dev)),
                      "    (b) / (a) = %.3f" % (med(t_dev) / med(t_host)),
                      "(c) v2x_seg_rasterize alone, labels + hist (2 launches, HIP events, %d calls)   : %9.1f us per call   [rounds: %s]"
                      % (args.iters, med(t_call), " ".join("%.1f" % v for v in t_call)),
                      "    the same with every count 0 (the fixed cost: launches and writes)          : %9.1f us per call   [rounds: %s]"
                      % (med(t_empty), " ".join("%.1f" % v for v in t_empty)),
                      "(d) 1 B per cell = %.2f MB of labels per call: %.3f TB/s = %.1f %% of the write ceiling; with no boxes %.3f TB/s = %.1f %%"
                      % (nbytes / 1e6, rate, 100 * rate / write_tbs, rate_empty, 100 * rate_empty / write_tbs)]
            del out
    lines += ["", "((c) times a loop of calls between two HIP events: it is the larger of the device time and the time the host needs to issue a call -- "
              "ops.rasterize_seg allocates the workspace and makes one ctypes call, two launches)"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

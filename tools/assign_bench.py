#!/usr/bin/env python3
"""Time of the training targets of a step on the synthetic scenes, at 10 and 40 items (5 agents x 2 and x 8 frames), none asserted:
  * the radius rule as the training loop runs it: utils/synthetic_scene.anchor_targets_sparse per item on the host, then dense_targets_on_device
    (host clock, the device idle before and after);
  * the IoU rule: upload of the padded boxes + v2x_det_assign_targets (csrc/det_assign.hip) for all items, the same host clock; and the call alone
    on HIP events, into buffers allocated once -- with the scenes' boxes and with every count 0 (the write phase alone: every output element is
    written whatever the boxes are), its 33 output bytes per anchor (labels, reg_targets, reg_loss_mask) against what v2x_calib_stream writes;
  * positives per box under both rules.
--train STEPS appends one run each of tools/det/train_codet.py --targets radius and --targets iou (same seed, lowerbound detector, the step as one
hipGraph) with their loss columns.

    python3 tools/assign_bench.py [--items 10 40] [--train 300] [--out profiles/assign_targets_bench.txt]
"""
import argparse
import contextlib
import importlib.util
import io
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
    ap.add_argument("--items", default=[10, 40], type=int, nargs="+", help="items per call (multiples of --agents)")
    ap.add_argument("--iters", default=50, type=int)
    ap.add_argument("--rounds", default=5, type=int)
    ap.add_argument("--train", default=0, type=int, help="steps of the two training runs (0: none)")
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--out", default="", type=str)
    args = ap.parse_args(argv)
    from v2x_sim_amd import calibrate, ops
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.utils import postprocess, synthetic_scene
    if not torch.cuda.is_available():
        raise SystemExit("assign_bench.py measures on the MI355X: no GPU, no figure")
    dev = torch.device("cuda:0")
    cfg = Config("train")
    anchors = postprocess.build_anchor_map(cfg)
    d_anchors = torch.from_numpy(anchors).to(dev)
    X, Y, A = anchors.shape[:3]
    med = lambda v: float(np.median(v))
    write_tbs = max(calibrate.stream_rate(0, 1, total_bytes=1 << 30, wg_per_cu=w, device=dev) for w in (2, 4, 8))
    lines = ["anchor targets of one training step on the synthetic scenes (24 cars per scene), grid %d x %d x %d, on %s" % (X, Y, A, torch.cuda.get_device_name(0)),
             "write ceiling: v2x_calib_stream 0 read : 1 write, 1 GiB, best of 2 / 4 / 8 workgroups per CU: %.2f TB/s" % write_tbs]

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.iters

    for n in args.items:
        frames = n // args.agents
        b = synthetic_scene.make_batch(frames, args.agents, seed=args.seed)
        lists = [np.asarray(b["gt_boxes"][a][f], np.float32).reshape(-1, 5) for a in range(args.agents) for f in range(frames)]
        n_boxes = sum(g.shape[0] for g in lists)

        def radius_path():
            pos, reg = [], []
            for m, g in enumerate(lists):
                p, r = synthetic_scene.anchor_targets_sparse(g, anchors)
                pos.append(np.concatenate([np.full((p.shape[0], 1), m, np.int64), p], 1))
                reg.append(r)
            out = synthetic_scene.dense_targets_on_device(np.concatenate(pos), np.concatenate(reg), n, anchors.shape, dev)
            torch.cuda.synchronize()
            return out, sum(p.shape[0] for p in pos)

        def pad():
            cap = max(1, max(g.shape[0] for g in lists))
            boxes, count = np.zeros((n, cap, 5), np.float32), np.zeros((n,), np.int32)
            for m, g in enumerate(lists):
                boxes[m, :g.shape[0]], count[m] = g, g.shape[0]
            return boxes, count

        def iou_path():
            boxes, count = pad()
            res = ops.assign_targets(torch.from_numpy(boxes).to(dev), torch.from_numpy(count).to(dev), d_anchors, want=())
            torch.cuda.synchronize()
            return res

        def host_clock(fn):
            fn()
            t = []
            for _ in range(args.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                t.append(1e3 * (time.perf_counter() - t0))
            return t

        (_, radius_pos), res = radius_path(), iou_path()
        iou_pos = int(res["reg_loss_mask"].sum())
        ignored = int((res["labels"].sum(-1) == 0).sum())
        matched = int((res["gt_best"] >= 0).sum())
        t_radius, t_iou = host_clock(radius_path), host_clock(iou_path)
        boxes, count = pad()
        d_boxes, d_count, d_zero = torch.from_numpy(boxes).to(dev), torch.from_numpy(count).to(dev), torch.zeros((n,), dtype=torch.int32, device=dev)
        out = {k: v for k, v in res.items()}
        call = lambda: ops.assign_targets(d_boxes, d_count, d_anchors, want=(), out=out)
        empty = lambda: ops.assign_targets(d_boxes, d_zero, d_anchors, want=(), out=out)
        events(call), events(empty)
        t_call, t_empty = [events(call) for _ in range(args.rounds)], [events(empty) for _ in range(args.rounds)]
        nbytes = 33.0 * n * X * Y * A
        rate = nbytes / (med(t_call) * 1e-6) / 1e12
        rate_empty = nbytes / (med(t_empty) * 1e-6) / 1e12
        lines += ["",
                  "%d items (%d agents x %d frames), %d boxes (gt_cap %d), %d of them reach an anchor" % (n, args.agents, frames, n_boxes, boxes.shape[1], matched),
                  "radius rule, host loop per item + dense_targets_on_device, host clock        : %9.2f ms per step   [rounds: %s]"
                  % (med(t_radius), " ".join("%.1f" % v for v in t_radius)),
                  "IoU rule, pad + upload + v2x_det_assign_targets + synchronise, host clock    : %9.2f ms per step   [rounds: %s]"
                  % (med(t_iou), " ".join("%.2f" % v for v in t_iou)),
                  "v2x_det_assign_targets alone (2 launches, HIP events, %d calls per round)     : %9.1f us per call   [rounds: %s]"
                  % (args.iters, med(t_call), " ".join("%.1f" % v for v in t_call)),
                  "  the same with every count 0 (nothing but the writes)                       : %9.1f us per call   [rounds: %s]"
                  % (med(t_empty), " ".join("%.1f" % v for v in t_empty)),
                  "  33 B per anchor = %.1f MB per call: %.2f TB/s = %.0f %% of the write ceiling; with no boxes %.2f TB/s = %.0f %%"
                  % (nbytes / 1e6, rate, 100 * rate / write_tbs, rate_empty, 100 * rate_empty / write_tbs),
                  "positives per box: radius rule %.1f (%d), IoU rule %.1f (%d; %d anchors ignored)"
                  % (radius_pos / max(n_boxes, 1), radius_pos, iou_pos / max(matched, 1), iou_pos, ignored)]
        if rate < 0.5 * write_tbs:
            share = 100.0 * med(t_empty) / med(t_call)
            lines.append("  below half the ceiling: the write phase alone takes %.0f %% of the call (a thread stores its anchor's 24 + 8 + 1 bytes at a stride of A rows: "
                         "partial lines per store instruction), the IoU phase (fp64 clipping in the tiles the boxes reach) the remaining %.0f %%" % (share, 100.0 - share))
        del out, res

    if args.train > 0:
        spec = importlib.util.spec_from_file_location("train_codet_cli", os.path.join(ROOT, "tools", "det", "train_codet.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        for rule in ("radius", "iou"):
            buf = io.StringIO()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(buf):
                mod.main(["--com", "lowerbound", "--steps", str(args.train), "--batch", "2", "--seed", str(args.seed), "--engine", "hip-graph", "--log",
                          "--targets", rule])
            dt = time.perf_counter() - t0
            lines += ["", "tools/det/train_codet.py --com lowerbound --engine hip-graph --steps %d --batch 2 --seed %d --targets %s   (%.1f s, %.1f ms per step with "
                      "scene generation)" % (args.train, args.seed, rule, dt, 1e3 * dt / args.train)]
            lines += ["  " + ln for ln in buf.getvalue().splitlines() if ln.startswith("step") or ln.startswith("epoch")]
        lines += ["(the two losses are normalised by their own positives and are not comparable in size; what the columns say is whether each rule's loss falls)"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time of the corner localisation loss (Config.loss_type = "corner_loss") on the MI355X, none asserted:
  * forward + backward of train/loss.py::detection_loss(loss_type="corner_loss") at 10 and 40 maps of the config's anchor grid (256 x 256 x 6) on the
    kernels (csrc/det_corner_loss.hip, three launches) and as the PyTorch-op statement of the same function (TRAIN_LOSS_HIP = 0), and the same pair
    for "faf_loss" (csrc/det_loss.hip) -- the four forms alternate inside every round, HIP events around `--iters` calls, the median of the rounds;
  * the 10-map FaFNet step captured as one hipGraph (train/graph_step.py) with corner_loss next to the faf_loss one, alternating in the same way,
    and the one expectation there is: the corner step costs no more than the smooth-L1 step plus the difference of the two loss kernels' own times.

    python3 tools/corner_loss_bench.py [--maps 10 40] [--out profiles/corner_loss_bench.txt]
"""
import argparse
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default=[10, 40], type=int, nargs="+")
    ap.add_argument("--iters", default=50, type=int)
    ap.add_argument("--rounds", default=7, type=int)
    ap.add_argument("--step-maps", default=10, type=int, help="maps of the captured FaFNet step (5 agents x frames); 0: skip")
    ap.add_argument("--positives", default=0.01, type=float, help="share of selected anchors")
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--out", default="", type=str)
    args = ap.parse_args(argv)
    from v2x_sim_amd import tuning
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.train.loss import corner_anchor_table, detection_loss
    from v2x_sim_amd.utils import postprocess
    if not torch.cuda.is_available():
        raise SystemExit("corner_loss_bench.py measures on the MI355X: no GPU, no figure")
    dev = torch.device("cuda:0")
    cfg = Config("train")
    anchors = postprocess.build_anchor_map(cfg)
    X, Y, A = anchors.shape[:3]
    table = corner_anchor_table(anchors, dev)
    med = lambda v: float(np.median(v))          # noqa: E731
    lines = ["detection loss, forward + backward, anchor grid %d x %d x %d, %.1f %% of the anchors selected, on %s" % (X, Y, A, 100 * args.positives,
                                                                                                                 torch.cuda.get_device_name(0)),
             "HIP events around %d calls, %d rounds, the four forms alternating inside every round; median [rounds]" % (args.iters, args.rounds)]

    def events(fn, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / iters          # us per call

    kernel_us = {}
    for n in args.maps:
        g = torch.Generator().manual_seed(args.seed + n)
        M = X * Y * A
        cls = (torch.randn(n, M, 2, generator=g) * 2.0).to(dev).requires_grad_(True)
        loc = torch.zeros(n, X, Y, A, 1, 6)
        loc[..., :4] = torch.randn(n, X, Y, A, 1, 4, generator=g) * 0.3
        th = (torch.rand(n, X, Y, A, 1, generator=g) - 0.5) * 2.0
        loc[..., 4], loc[..., 5] = torch.sin(th), torch.cos(th)
        loc = loc.to(dev).requires_grad_(True)
        mask = (torch.rand(n, X, Y, A, 1, generator=g) < args.positives).to(dev)
        lab = torch.zeros(n, X, Y, A, 2)
        lab[..., 0] = 1.0
        lab = lab.to(dev)
        lab[mask[..., 0]] = torch.tensor([0.0, 1.0], device=dev)
        tgt = torch.zeros(n, X, Y, A, 1, 6, device=dev)
        tgt[..., 5] = 1.0
        tgt = torch.where(mask[..., None], tgt + 0.1, torch.zeros_like(tgt))

        def form(loss_type, hip):
            def fn():
                tuning.set("TRAIN_LOSS_HIP", hip)
                cls.grad = loc.grad = None
                detection_loss({"cls": cls, "loc": loc}, lab, tgt, mask, loss_type=loss_type, anchors=table)[0].backward()
            return fn
        prev = (tuning.set("TRAIN_HIP", 1), tuning.set("TRAIN_LOSS_HIP", 1))
        forms = [("corner_loss, kernels (det_corner_loss.hip) ", form("corner_loss", 1)), ("corner_loss, PyTorch ops                  ", form("corner_loss", 0)),
                 ("faf_loss,    kernels (det_loss.hip)        ", form("faf_loss", 1)), ("faf_loss,    PyTorch ops                  ", form("faf_loss", 0))]
        try:
            for _, fn in forms:
                events(fn, 5)
            t = [[] for _ in forms]
            for _ in range(args.rounds):
                for k, (_, fn) in enumerate(forms):
                    t[k].append(events(fn, args.iters))
        finally:
            tuning.set("TRAIN_HIP", prev[0])
            tuning.set("TRAIN_LOSS_HIP", prev[1])
        nbytes = n * M * (2 * 4 * 2 + 1) * 2 + n * M * (2 + 6) * 4          # forward and backward read cls, labels, mask; backward writes dcls, dloc
        lines += ["", "%d maps = %d anchors (%d selected); the unselected anchors' codes are not read: %.0f MB per forward + backward" % (
            n, n * M, int(mask.sum()), nbytes / 1e6)]
        for (name, _), v in zip(forms, t):
            lines.append("  %s: %9.1f us   [%s]" % (name, med(v), " ".join("%.0f" % x for x in v)))
        ck, co, fk, fo = (med(v) for v in t)
        kernel_us[n] = (ck, fk)
        lines.append("  corner_loss: PyTorch ops / kernels = %.1f x;  faf_loss: %.1f x;  corner kernels - faf kernels = %+.1f us;  corner kernels move %.2f TB/s"
                     % (co / ck, fo / fk, ck - fk, nbytes / (ck * 1e-6) / 1e12))
        if ck >= co:
            lines.append("  THE KERNEL PATH IS NOT FASTER than the PyTorch ops at %d maps (the switch semantics stay as they are)" % n)
        del cls, loc, lab, tgt, mask

    if args.step_maps > 0:
        from v2x_sim_amd.models.det import FaFNet
        from v2x_sim_amd.train.graph_step import GraphedTrainStep
        from v2x_sim_amd.train.loop import init_for_training, synthetic_batch_on_device
        agents = 5
        frames = max(1, args.step_maps // agents)
        prev = tuning.set("TRAIN_HIP", 1)
        try:
            base = init_for_training(FaFNet(cfg, kd_flag=0, num_agent=agents), seed=1).to(dev)
            data = synthetic_batch_on_device(cfg, frames, agents, seed=3, device=dev)
            steps = {}
            for lt in ("faf_loss", "corner_loss"):
                model = copy.deepcopy(base).train()
                opt = torch.optim.Adam(model.parameters(), lr=torch.tensor(1e-3, device=dev), capturable=True)
                steps[lt] = GraphedTrainStep(model, opt, data, frames, loss_type=lt, anchors=table)
            t = {lt: [] for lt in steps}
            for lt, s in steps.items():
                events(lambda s=s: s(data), 5)
            for _ in range(args.rounds):
                for lt, s in steps.items():
                    t[lt].append(events(lambda s=s: s(data), 20))
        finally:
            tuning.set("TRAIN_HIP", prev)
        tf, tc = med(t["faf_loss"]), med(t["corner_loss"])
        lines += ["", "FaFNet training step captured as one hipGraph, %d maps (%d agents x %d frames), HIP events around 20 replays (input copies included), alternating" % (
            agents * frames, agents, frames),
            "  faf_loss   : %9.1f us per step   [%s]" % (tf, " ".join("%.0f" % x for x in t["faf_loss"])),
            "  corner_loss: %9.1f us per step   [%s]" % (tc, " ".join("%.0f" % x for x in t["corner_loss"]))]
        n = agents * frames
        if n in kernel_us:
            ck, fk = kernel_us[n]
            lines.append("  corner step - faf step = %+.1f us; the two loss kernels' own difference at %d maps = %+.1f us: the expectation (no more than that) %s"
                         % (tc - tf, n, ck - fk, "HOLDS to within 1 % of the step (the allowance for the rounds' spread)" if tc - tf <= max(ck - fk, 0.0) + 0.01 * tf else "DOES NOT HOLD (beyond 1 % of the step)"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

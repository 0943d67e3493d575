#!/usr/bin/env python3
"""Forward time of the segmentation variants next to their detection twins: forward_nhwc of every class of models/seg that has a twin, 5 agents,
at 1 frame and at 64 frames (320 maps), seeded synthetic weights and clouds.  Device events around `--iters` calls, median of `--rounds`; the seg
class and its twin alternate inside each round.  when2com is timed with inference 'activated' (links chosen by the seeded weights).  Nothing is
asserted.

    python3 tools/seg_variants_bench.py [--frames 1,64] [--out <file>]      (the committed record: section 2 of profiles/seg_variants_bench.txt)
"""
import argparse
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
    ap.add_argument("--agents", default=5, type=int)
    ap.add_argument("--frames", default="1,64", type=str)
    ap.add_argument("--iters", default=0, type=int, help="calls per round (default: 20 at one frame, 3 at 64)")
    ap.add_argument("--rounds", default=5, type=int)
    ap.add_argument("--out", default="", type=str)
    args = ap.parse_args(argv)
    from v2x_sim_amd import ops
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models import det, seg
    from v2x_sim_amd.utils.synthetic import init_synthetic_weights, synthetic_points, synthetic_poses
    if not torch.cuda.is_available():
        raise SystemExit("seg_variants_bench.py measures on the MI355X: no GPU, no figure")
    dev = torch.device("cuda:0")
    A = args.agents
    cfg = Config("test")
    pairs = [("v2v", seg.V2VNetSeg, det.V2VNet), ("when2com", seg.When2comSeg, det.When2com), ("when2com sparse", seg.When2comSeg, det.When2com),
             ("sum", seg.SumFusionSeg, det.SumFusion), ("mean", seg.MeanFusionSeg, det.MeanFusion), ("max", seg.MaxFusionSeg, det.MaxFusion),
             ("cat", seg.CatFusionSeg, det.CatFusion), ("disco", seg.DiscoNetSeg, det.DiscoNet)]
    lines = ["forward_nhwc, %d agents, seeded synthetic weights and clouds, on %s; us per call, median of %d rounds (seg / twin alternating)"
             % (A, torch.cuda.get_device_name(0), args.rounds),
             "%-16s %7s %14s %14s %9s" % ("--com", "frames", "seg class", "det twin", "seg/det")]
    grid = ops.VoxelGrid()
    for B in [int(v) for v in args.frames.split(",")]:
        iters = args.iters or (20 if B == 1 else 3)
        pts = torch.from_numpy(synthetic_points(A * B, 16384, seed=21)).to(dev)
        x0 = ops.bits_to_nhwc(ops.voxelize_bits(pts, torch.full((A * B,), 16384, dtype=torch.int32, device=dev), grid), 13, 32)
        T = torch.from_numpy(synthetic_poses(B, A, seed=22)).to(dev)
        nat = torch.full((B, A), A)
        for name, S, D in pairs:
            kw = dict(num_agent=A, **({"sparse": True} if name.endswith("sparse") else {}))
            w2c = name.startswith("when2com")
            models = [init_synthetic_weights(cls(cfg, **kw), seed=4).to(dev).eval() for cls in (S, D)]
            plans = [m.make_plan(nat, B, dev) for m in models]

            def run(i):
                if w2c:
                    return models[i].forward_nhwc(x0, T, nat, training=False, inference="activated", batch_size=B, plan=plans[i])
                return models[i].forward_nhwc(x0, T, nat, batch_size=B, plan=plans[i])

            def timed(i):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    run(i)
                e1.record()
                e1.synchronize()
                return 1e3 * e0.elapsed_time(e1) / iters
            with torch.no_grad():
                for i in (0, 1):          # warm-up: packing, code objects, the shapes of the timed window
                    run(i)
                    run(i)
                torch.cuda.synchronize()
                t = np.zeros((args.rounds, 2))
                for r in range(args.rounds):
                    for i in ((0, 1) if r % 2 == 0 else (1, 0)):
                        t[r, i] = timed(i)
            ts, td = float(np.median(t[:, 0])), float(np.median(t[:, 1]))
            lines.append("%-16s %7d %14.1f %14.1f %9.3f" % (name, B, ts, td, ts / td))
            print(lines[-1], flush=True)
            del models, plans
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

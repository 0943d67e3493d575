#!/usr/bin/env python3
"""Segmentation evaluation for every --com of detection except `late`, with the communication flags.

    python tools/seg/eval_seg.py --data synthetic --com v2v --resume out/epoch_1.pth --compress_level 2 --only_v2i 1
    python tools/seg/eval_seg.py --data synthetic --com who2com --resume out/epoch_1.pth      (a when2com checkpoint; also prints the communication rate)

--com lowerbound | upperbound | v2v is tools/seg/test_seg.py's own evaluation (that file stays as it is: it is part of the test surface);
--com when2com | who2com | sum | mean | max | cat | disco is evaluated HERE, by the same loop over the same flags plus --inference
(softmax | activated | argmax_test; default 'activated', who2com -- a When2comSeg, as in tools/det/test_codet.py -- 'argmax_test').
Either way --compress_level k (0..8) and --only_v2i 0|1 reach the model's constructor through comm.model_flags and are checked against the record
tools/seg/train_seg.py keeps in its checkpoints (v2x_sim_amd/utils/comm.py::run_eval_driver).  when2com takes --compress_level; under
--only_v2i 1 the When2comSeg constructor raises its NotImplementedError (when2com has no agreed reading under a link mask).
--p_com_outage p, --pose_noise sigma and --channel_seed s (degraded links drawn on the device) travel the same way but are an
evaluation condition: no checkpoint records them, --com lowerbound / upperbound refuse them, when2com / who2com take --pose_noise only; the realised
share of links up is printed after the IoUs."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OWN_COMS = ["when2com", "who2com", "sum", "mean", "max", "cat", "disco"]      # evaluated by evaluate() below; the others by test_seg.main


def build_parser():
    """test_seg.py's flags with every --com, and --inference (the communication flags are run_eval_driver's)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("-d", "--data", default="synthetic", type=str)
    ap.add_argument("--com", default="v2v", choices=["lowerbound", "upperbound", "v2v"] + OWN_COMS)
    ap.add_argument("--inference", default=None, choices=["softmax", "activated", "argmax_test"],
                    help="when2com / who2com: default 'activated' (when2com), 'argmax_test' (who2com)")
    ap.add_argument("--resume", default="", type=str)
    ap.add_argument("--num_agent", default=5, type=int)
    ap.add_argument("--frames", default=8, type=int)
    ap.add_argument("--batch", default=2, type=int)
    ap.add_argument("--seed", default=4242, type=int)
    ap.add_argument("--rsu", default=1, type=int, help="parsed dataset: 1 = agent0 (the RSU) takes part, 0 = vehicles only")
    ap.add_argument("--scene", default="sampled", choices=["sampled", "raycast"],
                    help="synthetic data: raycast = tools/seg/train_seg.py's ray-cast world (any --com is then evaluated by this file's loop)")
    ap.add_argument("--observed", default="own", choices=["own", "any", "all"], help="--scene raycast: which cells count as observed (the others are ignored)")
    return ap


def evaluate(argv):
    """test_seg.main's loop for the classes of models/seg it does not build -> {'iou', 'miou', 'confusion'} and, for the when2com pair,
    'num_connect' (When2com.num_connect averaged over the frames; printed)."""
    import torch
    args = build_parser().parse_args(argv)
    from train_seg import seg_batch
    from v2x_sim_amd import ops
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.seg import COM_CLASSES, When2comSeg, default_inference
    from v2x_sim_amd.utils.SegModule import SegModule, iou_from_confusion
    from v2x_sim_amd.utils.synthetic import init_synthetic_weights
    config = Config("test", binary=True, only_det=True)
    A = args.num_agent
    model = COM_CLASSES[args.com](config, num_agent=A)       # the communication flags arrive through comm.model_flags
    if not torch.cuda.is_available():
        raise SystemExit("eval_seg.py needs the MI355X: the hot path has no CPU fallback")
    device = torch.device("cuda:0")
    inference = args.inference or default_inference(args.com)
    if args.resume:
        ckpt = torch.load(args.resume, map_location="cpu")
        model.load_state_dict(ckpt.get("model_state_dict", ckpt), strict=True)   # a key mismatch must not score init weights
    else:
        print("no --resume given: evaluating seeded synthetic weights")
        init_synthetic_weights(model, seed=0)
    model = model.to(device).eval()
    module = SegModule(model, None, config, None, 0)
    grid = ops.VoxelGrid(config.voxel_size, config.area_extents)
    conf = torch.zeros((model.n_classes, model.n_classes), dtype=torch.int64, device=device)
    if args.data != "synthetic":
        from v2x_sim_amd.datasets import V2XSimSeg, seg_batch_on_device
        first = 0 if args.rsu else 1
        roots = [os.path.join(args.data, "agent%d" % k) for k in range(first, first + A)]
        dataset = V2XSimSeg(dataset_roots=roots, config=config, split="test", val=True, densify="none")
        batches = ([dataset[i] for i in range(s0, min(s0 + args.batch, len(dataset)))] for s0 in range(0, len(dataset), args.batch))
        batches = ((seg_batch_on_device(smp, grid, device), len(smp)) for smp in batches)
    else:
        batches = ((seg_batch(config, min(args.batch, args.frames - s0), A, args.seed + s0, device, grid, n_classes=model.n_classes, scene=args.scene,
                              observed=args.observed), min(args.batch, args.frames - s0)) for s0 in range(0, args.frames, args.batch))
    connect = []
    for data, B in batches:
        _, c = module.predict(data, batch_size=B, label=data["labels"].to(torch.uint8), inference=inference)
        conf += c
        if isinstance(model, When2comSeg):
            connect.append((module.last_num_connect * B, B))
    iou = iou_from_confusion(conf.cpu())
    present = ~torch.isnan(iou)
    for k in range(model.n_classes):
        if present[k]:
            print("class %d IoU %.4f" % (k, float(iou[k])))
    miou = float(iou[present].mean())
    print("mIoU %.4f over %d present classes" % (miou, int(present.sum())))
    res = {"iou": iou, "miou": miou, "confusion": conf.cpu()}
    if isinstance(model, When2comSeg):
        # When2com.num_connect per batch, weighted by its frames: off-diagonal non-zero links per agent and frame
        res["num_connect"] = sum(c for c, _ in connect) / max(1, sum(b for _, b in connect))
        print("communication rate (%s) %.3f" % (inference, res["num_connect"]))
    return res


def main(argv=None):
    import test_seg
    from v2x_sim_amd.utils import comm
    argv = sys.argv[1:] if argv is None else list(argv)
    peek = argparse.ArgumentParser(add_help=False)
    peek.add_argument("--com", default="v2v", type=str)
    peek.add_argument("--scene", default="sampled", type=str)
    known = peek.parse_known_args(argv)[0]
    # test_seg.py stays as it is and knows the sampled scene only: a ray-cast evaluation of its three --com runs through the loop above
    return comm.run_eval_driver(evaluate if known.com in OWN_COMS or known.scene != "sampled" else test_seg.main, argv)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""tools/det/test_codet.py with the scorer on the device:

    python tools/det/map_codet.py --data /path/V2X-Sim-det/test --com v2v --resume ckpt.pth --num_agent 5 --map_engine device

--map_engine host (the default) IS test_codet.py: its main() runs with the other arguments, unchanged.  --map_engine device runs the same
evaluation -- same flags, same dataset, model, FaFModule.predict_all loop, same printed lines, same returned dict -- but scores with ONE
v2x_det_map call for all agents and both thresholds (v2x_sim_amd/utils/det_metrics.py::DetMap) instead of the Python
eval_map per agent and threshold.  test_codet.py itself is one of the files that stay as they are, so the loop is restated here;
tests/test_gpu_det_map.py holds the two engines to the same output.  tools/det/eval_codet.py drives this file, so the flag travels with
--compress_level, --only_v2i, --com late and the degraded-link flags."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import test_codet  # noqa: E402

IOU_THRS = (0.5, 0.7)


def build_parser():
    ap = test_codet.build_parser()
    ap.add_argument("--map_engine", default="host", choices=["host", "device"],
                    help="host: test_codet.py's own scoring (utils/postprocess.py::eval_map per agent and threshold); device: one v2x_det_map call for all of them")
    return ap


def _without_flag(argv):
    out, skip = [], False
    for a in argv:
        if skip:
            skip = False
        elif a == "--map_engine":
            skip = True
        elif not a.startswith("--map_engine="):
            out.append(a)
    return out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = build_parser().parse_args(argv)
    if args.map_engine == "host":
        return test_codet.main(_without_flag(argv))
    from v2x_sim_amd.configs import Config, ConfigGlobal
    from v2x_sim_amd.datasets import V2XSimDet, collate_dense
    from v2x_sim_amd.models.det import CatFusion, DiscoNet, FaFNet, MaxFusion, MeanFusion, SumFusion, V2VNet, When2com
    from v2x_sim_amd.utils.CoDetModule import FaFModule
    from v2x_sim_amd.utils.det_metrics import DetMap
    from v2x_sim_amd.utils.synthetic import init_synthetic_weights

    if not torch.cuda.is_available():
        raise SystemExit("map_codet.py needs the MI355X: the hot path has no CPU fallback")
    device = torch.device("cuda:0")
    # ---- test_codet.py's set-up, restated
    config, config_global = Config("test", binary=True, only_det=True), ConfigGlobal("test", binary=True, only_det=True)
    first = 0 if args.rsu else 1
    roots = [os.path.join(args.data, "agent%d" % k) for k in range(first, first + args.num_agent)]
    dataset = V2XSimDet(dataset_roots=roots, config=config, config_global=config_global, split="test", val=True)
    A = args.num_agent
    if args.com in ("lowerbound", "upperbound"):
        model = FaFNet(config, layer=args.layer, kd_flag=0, num_agent=A)
    elif args.com == "v2v":
        model = V2VNet(config, gnn_iter_times=args.gnn_iter_times, layer=args.layer, layer_channel=256, num_agent=A)
    elif args.com in ("sum", "mean", "max", "cat", "disco"):
        model = {"sum": SumFusion, "mean": MeanFusion, "max": MaxFusion, "cat": CatFusion, "disco": DiscoNet}[args.com](
            config, layer=args.layer, kd_flag=0, num_agent=A)
    else:
        model = When2com(config, layer=args.layer, warp_flag=args.warp_flag, num_agent=A)
    if args.resume:
        ckpt = torch.load(args.resume, map_location="cpu")
        model.load_state_dict(ckpt.get("model_state_dict", ckpt), strict=True)
        model.eval()
    else:
        print("no --resume given: evaluating seeded synthetic weights (there is no released checkpoint in this tree)")
        init_synthetic_weights(model, seed=args.seed)
    model = model.to(device)
    module = FaFModule(model, None, config, None, 0)
    module.score_thr = args.score_thr
    inference = args.inference or ("argmax_test" if args.com == "who2com" else "activated")

    # ---- the loop: one DetMap.update per (agent, frame) slot that is not None, where test_codet.py appends to its lists
    det_map = DetMap(iou_thrs=IOU_THRS, n_groups=A)
    # test_codet.py reads the detections' extents by the module's axis and the ground truth's as w along the heading: the same here
    cols = [0, 1, 3, 2, 4] if module.wh_axis == "h_along_heading" else [0, 1, 2, 3, 4]
    n_frames = [0] * A
    for start in range(0, len(dataset), args.batch):
        samples = [dataset[i] for i in range(start, min(start + args.batch, len(dataset)))]
        B = len(samples)
        bevs, trans, nat = collate_dense(samples)
        data = {"bev_seq": bevs.to(device), "trans_matrices": trans.to(device), "num_agent": nat}
        _, _, _, seq = module.predict_all(data, B, validation=False, num_agent=A, inference=inference)
        for k in range(A):
            for b in range(B):
                if seq[k][b] is not None:   # paired BY FRAME: frame b's detections meet frame b's ground truth
                    n_frames[k] += 1
                    det_map.update({"boxes": np.asarray(seq[k][b]["boxes"], np.float32).reshape(-1, 5)[:, cols], "scores": seq[k][b]["scores"]},
                                   samples[b][k][12], group=k)
        if args.log:
            print("frames %d-%d done" % (start, start + B - 1))

    table = det_map.result(device)
    means = {iou: [] for iou in IOU_THRS}
    for k in range(A):
        line = "agent%d:" % (k + first)
        for t, iou in enumerate(IOU_THRS):
            ap = float(table["ap"][k, t])
            means[iou].append(ap)
            line += "  mAP@%.1f %.2f" % (iou, 100 * ap)
        print(line + "  (%d frames, %d gt)" % (n_frames[k], int(table["num_gt"][k])))
    print("average local mAP@0.5 %.2f  mAP@0.7 %.2f" % (100 * float(np.mean(means[0.5])), 100 * float(np.mean(means[0.7]))))
    return {iou: float(np.mean(v)) for iou, v in means.items()}


if __name__ == "__main__":
    main()

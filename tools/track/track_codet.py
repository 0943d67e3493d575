#!/usr/bin/env python3
"""Tracking driver (row f-5): detection checkpoint + parsed detection set -> MOT-challenge text per agent and scene, which is what TrackEval reads.

    python tools/track/track_codet.py --data /path/V2X-Sim-det/test --com v2v --resume ckpt.pth --out tracks/

The parsed set (README.md:66-79 layout, agent{k}/{scene}_{frame}/0.npy) is walked in {scene}_{frame} order.  `--batch` scenes advance in parallel:
a step runs FaFModule.predict_all on frame t of each of them, and ONE SortTracker with num_agent x batch streams (stream = agent * batch + slot) takes
every map's detections in one launch; the tracker is reset when a group of scenes ends.  Output, one file per agent and scene,
<out>/agent{k}/{scene}.txt, a line per reported track:

    frame,id,x1,y1,w,h,score,-1,-1,-1

(frame counted from 1 within the scene, the box = the stand-up box of the filter's state, score = the score of the detection the track took).
What is and is not covered: tools/track/README.md."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DET_CAP = 64


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("-d", "--data", required=True, type=str, help="the {split} directory holding agent{k}/")
    ap.add_argument("--out", required=True, type=str, help="directory for the MOT-challenge text files")
    ap.add_argument("--com", default="v2v", choices=["lowerbound", "upperbound", "v2v", "when2com", "who2com", "sum", "mean", "max", "cat", "disco", "late"])
    ap.add_argument("--resume", default="", type=str, help="checkpoint with 'model_state_dict' (or a bare state_dict)")
    ap.add_argument("--num_agent", default=5, type=int)
    ap.add_argument("--rsu", default=1, type=int, help="1: agent0 (the RSU) takes part, 0: vehicles only")
    ap.add_argument("--layer", default=3, type=int)
    ap.add_argument("--gnn_iter_times", default=1, type=int)
    ap.add_argument("--inference", default=None, type=str, help="softmax | activated | argmax_test")
    ap.add_argument("--warp_flag", default=1, type=int)
    ap.add_argument("--batch", default=1, type=int, help="scenes tracked in parallel")
    ap.add_argument("--score_thr", default=0.7, type=float)
    ap.add_argument("--seed", default=0, type=int, help="synthetic-weights seed when --resume is not given")
    ap.add_argument("--direct", default=1, type=int, choices=[0, 1], help="1: abewley master's shortcut before the optimal assignment, 0: always the assignment")
    ap.add_argument("--max_age", default=1, type=int)
    ap.add_argument("--min_hits", default=3, type=int)
    ap.add_argument("--iou_threshold", default=0.3, type=float)
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    from v2x_sim_amd.configs import Config, ConfigGlobal
    from v2x_sim_amd.datasets import V2XSimDet, collate_dense
    from v2x_sim_amd.models.det import CatFusion, DiscoNet, FaFNet, MaxFusion, MeanFusion, SumFusion, V2VNet, When2com
    from v2x_sim_amd.utils.CoDetModule import FaFModule
    from v2x_sim_amd.utils.synthetic import init_synthetic_weights
    from v2x_sim_amd.utils.tracking import SortTracker

    if not torch.cuda.is_available():
        raise SystemExit("track_codet.py needs the MI355X: the hot path has no CPU fallback")
    device = torch.device("cuda:0")
    config, config_global = Config("test", binary=True, only_det=True), ConfigGlobal("test", binary=True, only_det=True)
    first = 0 if args.rsu else 1
    roots = [os.path.join(args.data, "agent%d" % k) for k in range(first, first + args.num_agent)]
    dataset = V2XSimDet(dataset_roots=roots, config=config, config_global=config_global, split="test", val=True)
    A = args.num_agent
    if args.com in ("lowerbound", "upperbound", "late"):       # late: the lowerbound detector, boxes exchanged afterwards
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
        print("no --resume given: tracking the detections of seeded synthetic weights (there is no released checkpoint in this tree)")
        init_synthetic_weights(model, seed=args.seed)
    model = model.to(device)
    module = FaFModule(model, None, config, None, 0)
    module.score_thr = args.score_thr
    if args.com == "late":
        module.late_fusion = True
    inference = args.inference or ("argmax_test" if args.com == "who2com" else "activated")

    # the samples of every scene, in frame order ({scene}_{frame} names, already sorted numerically by the dataset)
    scenes = {}
    for idx, name in enumerate(dataset.seq_names):
        scenes.setdefault(name.split("_")[0], []).append(idx)
    order = list(scenes)
    B = max(1, args.batch)
    tracker = SortTracker(A * B, max_age=args.max_age, min_hits=args.min_hits, iou_threshold=args.iou_threshold, direct=bool(args.direct),
                          wh_axis=module.wh_axis, device=device)
    written, n_lines, truncated = [], 0, 0
    for g0 in range(0, len(order), B):
        group = order[g0:g0 + B]
        tracker.reset()                                                 # scene boundary: empty streams, ids from 1
        files = {}
        for k in range(A):
            os.makedirs(os.path.join(args.out, "agent%d" % (k + first)), exist_ok=True)
            for scene in group:
                path = os.path.join(args.out, "agent%d" % (k + first), "%s.txt" % scene)
                files[(k, scene)] = open(path, "w")
                written.append(path)
        for t in range(max(len(scenes[s]) for s in group)):
            slots = [b for b, s in enumerate(group) if t < len(scenes[s])]      # scenes that still have a frame t
            samples = [dataset[scenes[group[b]][t]] for b in slots]
            bevs, trans, nat = collate_dense(samples)
            data = {"bev_seq": bevs.to(device), "trans_matrices": trans.to(device), "num_agent": nat}
            _, _, _, seq = module.predict_all(data, len(slots), validation=False, num_agent=A, inference=inference)
            boxes = np.zeros((A * B, DET_CAP, 5), np.float32)
            count = np.zeros((A * B,), np.int32)                        # a finished scene's streams and empty sweeps: no detections
            scores = np.zeros((A * B, DET_CAP), np.float32)
            for k in range(A):
                for j, b in enumerate(slots):
                    det = seq[k][j]
                    if det is None or len(det["boxes"]) == 0:
                        continue
                    top = np.argsort(-det["scores"], kind="stable")[:DET_CAP]       # the tracker reads the 64 best of a map
                    truncated += len(det["boxes"]) > DET_CAP
                    boxes[k * B + b, :len(top)] = det["boxes"][top]
                    scores[k * B + b, :len(top)] = det["scores"][top]
                    count[k * B + b] = len(top)
            tb, ids, di, n = tracker.update(torch.from_numpy(boxes).to(device), torch.from_numpy(count).to(device))
            tb, ids, di, n = tb.cpu().numpy(), ids.cpu().numpy(), di.cpu().numpy(), n.cpu().numpy()
            for k in range(A):
                for b in slots:
                    s = k * B + b
                    for r in range(int(n[s])):
                        x1, y1, x2, y2 = tb[s, r]
                        files[(k, group[b])].write("%d,%d,%.4f,%.4f,%.4f,%.4f,%.4f,-1,-1,-1\n" % (t + 1, ids[s, r], x1, y1, x2 - x1, y2 - y1,
                                                                                               scores[s, di[s, r]]))
                        n_lines += 1
        for f in files.values():
            f.close()
    if truncated:
        print("%d maps had more than %d detections: the tracker read the %d best" % (truncated, DET_CAP, DET_CAP))
    print("%d scenes x %d agents -> %d files, %d track lines under %s" % (len(order), A, len(written), n_lines, args.out))
    if args.com == "late":
        from v2x_sim_amd.utils import comm
        print(comm.late_report(module.late_stats))
    return {"files": written, "lines": n_lines}


if __name__ == "__main__":
    main()

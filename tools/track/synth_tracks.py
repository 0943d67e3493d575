#!/usr/bin/env python3
"""Synthetic tracking sequences (rows f-2 / f-5): moving ray-cast worlds -> ground-truth AND tracker MOT-challenge text, the two directories
tools/track/eval_track.py scores.

    python tools/track/synth_tracks.py --scenes 2 --steps 20 --num_agent 5 --gt own --detections gt --out seq/ --score
    python tools/track/synth_tracks.py --scenes 2 --steps 20 --detections model --com v2v --resume ckpt.pth --out seq/ --score

`--scenes` worlds of cars driving in lanes (utils/raycast_scene.make_moving_world) are swept for `--steps` steps, `--dt` apart, by every agent's LiDAR
in ONE v2x_lidar_cast_moving call (a sweep takes `--sweep_time`: a moving car is met where it is when the beam passes), and the ground truth with its
identities comes from ONE v2x_lidar_visible_boxes_moving call (DESIGN.md section 3.12 "moving scenes").
  <out>/gt/agent{k}/scene{w}.txt    a line per ground-truth box: frame,id,x1,y1,w,h,1,-1,-1,-1 -- frame from 1, id = 1 + the car's box index in its
                                    world, the box = the stand-up box of the rotated ground-truth box in the agent's frame at mid-sweep
                                    (postprocess.box_corners / standup with the module's wh_axis).  --gt own: the cars this agent got returns
                                    from; --gt any: the cars any agent of the scene got returns from at that step.
  <out>/trk/agent{k}/scene{w}.txt   SortTracker's output in track_codet.py's format.  --detections gt: the tracker is fed the ground-truth boxes
                                    themselves -- an upper bound on the tracker alone; --detections model: FaFModule.predict_all on the sweeps,
                                    exactly as track_codet.py does with a parsed set.
`--score` calls eval_track.py on the two directories and returns its record.  The step, the sweep duration and the speeds are this build's choices,
not V2X-Sim's; what is and is not covered: tools/track/README.md."""
import argparse
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

DET_CAP = 64


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, type=str, help="directory for gt/ and trk/")
    ap.add_argument("--scenes", default=2, type=int, help="worlds")
    ap.add_argument("--steps", default=20, type=int, help="sweeps per agent and world")
    ap.add_argument("--num_agent", default=5, type=int)
    ap.add_argument("--seed", default=0, type=int, help="the worlds' seed (and the synthetic weights' when --resume is not given)")
    ap.add_argument("--gt", default="own", choices=["own", "any"], help="whose returns make a car ground truth")
    ap.add_argument("--detections", default="gt", choices=["gt", "model"], help="what the tracker is fed")
    ap.add_argument("--score", action="store_true", help="score trk/ against gt/ with eval_track.py")
    ap.add_argument("--dt", default=0.2, type=float, help="seconds between two sweeps of an agent")
    ap.add_argument("--sweep_time", default=0.1, type=float, help="seconds a sweep takes")
    ap.add_argument("--beams", default=32, type=int)
    ap.add_argument("--az_steps", default=2048, type=int)
    ap.add_argument("--elev_deg", default=None, type=float, nargs=2, metavar=("LO", "HI"), help="the ring's elevations (default: ops.ring_table's)")
    ap.add_argument("--sigma_r", default=0.02, type=float)
    ap.add_argument("--gt_min_hits", default=5, type=int, help="returns a car needs to be ground truth")
    ap.add_argument("--com", default="lowerbound", choices=["lowerbound", "upperbound", "v2v", "when2com", "who2com", "sum", "mean", "max", "cat", "disco", "late"])
    ap.add_argument("--resume", default="", type=str, help="checkpoint with 'model_state_dict' (or a bare state_dict)")
    ap.add_argument("--layer", default=3, type=int)
    ap.add_argument("--gnn_iter_times", default=1, type=int)
    ap.add_argument("--inference", default=None, type=str, help="softmax | activated | argmax_test")
    ap.add_argument("--warp_flag", default=1, type=int)
    ap.add_argument("--score_thr", default=0.7, type=float)
    ap.add_argument("--direct", default=1, type=int, choices=[0, 1])
    ap.add_argument("--max_age", default=1, type=int)
    ap.add_argument("--min_hits", default=3, type=int, help="the tracker's min_hits")
    ap.add_argument("--iou_threshold", default=0.3, type=float)
    return ap


def gt_lines(boxes, ids, frame, wh_axis="w_along_heading"):
    """Ground-truth rows (k, 5) x, y, w, h, yaw with their box indices (k,) -> MOT-challenge lines of frame `frame` (from 1): id = 1 + index, the
    stand-up box of the rotated box."""
    from v2x_sim_amd.utils import postprocess
    boxes = np.asarray(boxes, np.float32).reshape(-1, 5)
    if not len(boxes):
        return []
    su = postprocess.standup(postprocess.box_corners(boxes, wh_axis))
    return ["%d,%d,%.4f,%.4f,%.4f,%.4f,1,-1,-1,-1\n" % (frame, 1 + int(i), x1, y1, x2 - x1, y2 - y1) for i, (x1, y1, x2, y2) in zip(ids, su)]


def _build_module(args, config, device):
    import torch
    from v2x_sim_amd.models.det import CatFusion, DiscoNet, FaFNet, MaxFusion, MeanFusion, SumFusion, V2VNet, When2com
    from v2x_sim_amd.utils.CoDetModule import FaFModule
    from v2x_sim_amd.utils.synthetic import init_synthetic_weights
    A = args.num_agent
    if args.com in ("lowerbound", "upperbound", "late"):
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
    module = FaFModule(model.to(device), None, config, None, 0)
    module.score_thr = args.score_thr
    if args.com == "late":
        module.late_fusion = True
    return module


def main(argv=None, world=None):
    """world: a make_moving_world dict to use instead of make_moving_world(--scenes, --num_agent, --seed) (its shapes win)."""
    args = build_parser().parse_args(argv)
    import torch
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.utils import raycast_scene
    from v2x_sim_amd.utils.tracking import SortTracker

    if not torch.cuda.is_available():
        raise SystemExit("synth_tracks.py needs the MI355X: the hot path has no CPU fallback")
    device = torch.device("cuda:0")
    config = Config("test", binary=True, only_det=True)
    world = raycast_scene.make_moving_world(args.scenes, args.num_agent, args.seed) if world is None else world
    W = world["boxes"].shape[0]
    A = world["sensors"].shape[0] // W
    T, B, args.num_agent = args.steps, W * args.steps, A
    data = raycast_scene.raycast_sequence_on_device(config, world, T, dt=args.dt, sweep_time=args.sweep_time, device=device, with_targets=False,
                                                    gt=args.gt, min_hits=args.gt_min_hits, gt_lists=True, beams=args.beams, az_steps=args.az_steps,
                                                    sigma_r=args.sigma_r, seed=args.seed, elev_deg=args.elev_deg)
    module = _build_module(args, config, device) if args.detections == "model" else None
    wh_axis = module.wh_axis if module is not None else config.box_wh_axis
    inference = args.inference or ("argmax_test" if args.com == "who2com" else "activated")

    def path(side, a, w):
        d = os.path.join(args.out, side, "agent%d" % a)
        os.makedirs(d, exist_ok=True)
        return os.path.join(d, "scene%d.txt" % w)

    n_gt = 0
    for a in range(A):
        for w in range(W):
            with open(path("gt", a, w), "w") as fh:
                for k in range(T):
                    lines = gt_lines(data["gt_boxes"][a][w * T + k], data["gt_id_lists"][a][w * T + k], k + 1, wh_axis)
                    fh.writelines(lines)
                    n_gt += len(lines)

    tracker = SortTracker(A * W, max_age=args.max_age, min_hits=args.min_hits, iou_threshold=args.iou_threshold, direct=bool(args.direct),
                          wh_axis=wh_axis, device=device)
    files = {(a, w): open(path("trk", a, w), "w") for a in range(A) for w in range(W)}
    n_trk = truncated = 0
    for k in range(T):
        boxes = np.zeros((A * W, DET_CAP, 5), np.float32)
        count = np.zeros((A * W,), np.int32)
        scores = np.ones((A * W, DET_CAP), np.float32)
        if module is None:
            for a in range(A):
                for w in range(W):
                    g = data["gt_boxes"][a][w * T + k][:DET_CAP]
                    boxes[a * W + w, :len(g)], count[a * W + w] = g, len(g)
        else:
            items = torch.as_tensor([w * T + k for w in range(W)], device=device)
            rows = (torch.arange(A, device=device)[:, None] * B + items[None, :]).reshape(-1)          # agent-major rows of this step's items
            step = {"bev_seq": data["bev_seq"][rows], "trans_matrices": data["trans_matrices"][items], "num_agent": data["num_agent"][items.cpu()]}
            _, _, _, seq = module.predict_all(step, W, validation=False, num_agent=A, inference=inference)
            for a in range(A):
                for w in range(W):
                    det = seq[a][w]
                    if det is None or len(det["boxes"]) == 0:
                        continue
                    top = np.argsort(-det["scores"], kind="stable")[:DET_CAP]
                    truncated += len(det["boxes"]) > DET_CAP
                    boxes[a * W + w, :len(top)], scores[a * W + w, :len(top)], count[a * W + w] = det["boxes"][top], det["scores"][top], len(top)
        tb, ids, di, n = tracker.update(torch.from_numpy(boxes).to(device), torch.from_numpy(count).to(device))
        tb, ids, di, n = tb.cpu().numpy(), ids.cpu().numpy(), di.cpu().numpy(), n.cpu().numpy()
        for (a, w), fh in files.items():
            s = a * W + w
            for r in range(int(n[s])):
                x1, y1, x2, y2 = tb[s, r]
                fh.write("%d,%d,%.4f,%.4f,%.4f,%.4f,%.4f,-1,-1,-1\n" % (k + 1, ids[s, r], x1, y1, x2 - x1, y2 - y1, scores[s, di[s, r]]))
                n_trk += 1
    for fh in files.values():
        fh.close()
    if truncated:
        print("%d maps had more than %d detections: the tracker read the %d best" % (truncated, DET_CAP, DET_CAP))
    print("%d scenes x %d steps x %d agents -> %d ground-truth lines, %d track lines under %s" % (W, T, A, n_gt, n_trk, args.out))
    res = {"gt": os.path.join(args.out, "gt"), "trk": os.path.join(args.out, "trk"), "gt_lines": n_gt, "trk_lines": n_trk}
    if args.score:
        spec = importlib.util.spec_from_file_location("eval_track_cli", os.path.join(os.path.dirname(os.path.abspath(__file__)), "eval_track.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        res["score"] = mod.main(["--gt", res["gt"], "--trk", res["trk"]])
    return res


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What scoring detection mAP costs at the size of a test split: 5 agents x 1000 frames, about 20 ground truths and about 30 detections per map
(post_refs-style fields: ground truths on a 7 m lattice, detections perturbed from them or dropped anywhere), thresholds 0.5 and 0.7, three ways --
(a) `utils/postprocess.py::eval_map`, the path of tools/det/test_codet.py today: per agent and threshold, pure Python (timed on --host_frames frames
    per agent and scaled to the split);
(b) `eval_map_device` per agent and threshold: v2x_match_detections on the device, the sort and the cumulative sums in numpy (ten calls);
(c) `DetMap.result()`: padding on the host, ONE upload, ONE v2x_det_map call, download (a host clock that ends in a synchronise) -- and the
    v2x_det_map call alone on device-resident tensors (device events around its four launches).
The repetitions of (b) and (c) alternate; medians are reported.  (c) is also timed at --scale times the maps: the ranking is a binary search per
(detection, map of its group), so it grows with the SQUARE of the maps per agent.  Nothing here is asserted.

    python3 tools/map_bench.py [--agents 5] [--frames 1000] [--rounds 7] [--out profiles/det_map_bench.txt]"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

THRS = (0.5, 0.7)


def make_split(agents, frames, seed, det_cap=64, gt_cap=32):
    """-> padded host arrays of agents * frames maps, frame-major (the tool's order), every map in descending score order."""
    import post_refs as PR
    rng = np.random.default_rng(seed)
    n = agents * frames
    det, sc = np.zeros((n, det_cap, 5), np.float32), np.zeros((n, det_cap), np.float32)
    gt = np.zeros((n, gt_cap, 5), np.float32)
    dc, gc = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i in range(n):
        ng, nd = int(rng.integers(15, 26)), int(rng.integers(22, 39))
        g = PR._gt_field(rng, ng)
        src = g[rng.integers(0, ng, nd)].astype(np.float64)
        src[:, :2] += rng.normal(0, 0.35, (nd, 2))
        src[:, 2:4] *= rng.uniform(0.85, 1.2, (nd, 2))
        src[:, 4] += rng.normal(0, 0.12, nd)
        stray = rng.random(nd) < 0.2
        src[stray, :2] = rng.uniform(0.0, 7.0 * math.ceil(math.sqrt(ng)), (int(stray.sum()), 2))
        s = np.sort(np.round(rng.uniform(0.7, 1.0, nd), 4).astype(np.float32))[::-1]
        det[i, :nd], sc[i, :nd], gt[i, :ng], dc[i], gc[i] = src, s, g, nd, ng
    group = (np.arange(n) % agents).astype(np.int32)
    return det, sc, dc, gt, gc, group


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", default=5, type=int)
    ap.add_argument("--frames", default=1000, type=int)
    ap.add_argument("--host_frames", default=20, type=int, help="frames per agent that eval_map (a) is timed on")
    ap.add_argument("--scale", default=10, type=int, help="(c) is timed again at this many times the maps")
    ap.add_argument("--rounds", default=7, type=int)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_map_bench.txt"))
    args = ap.parse_args(argv)
    from v2x_sim_amd import ops
    from v2x_sim_amd.utils import postprocess as P
    from v2x_sim_amd.utils.det_metrics import DetMap
    dev = torch.device("cuda:0")
    A, F = args.agents, args.frames
    det, sc, dc, gt, gc, group = make_split(A, F, seed=2024)
    n = len(group)
    d_in = [torch.from_numpy(a).to(dev) for a in (det, sc, dc, gt, gc, group)]
    sel = [torch.from_numpy(np.nonzero(group == a)[0]).to(dev) for a in range(A)]
    per_agent = [[t[s].contiguous() for t in d_in[:3]] for s in sel]
    gt_lists = [[gt[i, :gc[i]] for i in np.nonzero(group == a)[0]] for a in range(A)]

    def run_b():
        t0 = time.perf_counter()
        out = [[P.eval_map_device(per_agent[a][0], per_agent[a][1], per_agent[a][2], gt_lists[a], thr)[0] for thr in THRS] for a in range(A)]
        return (time.perf_counter() - t0) * 1e3, np.array(out)

    def filled():
        m = DetMap(iou_thrs=THRS, n_groups=A)
        t0 = time.perf_counter()
        for i in range(n):
            m.update({"boxes": det[i, :dc[i]], "scores": sc[i, :dc[i]]}, gt[i, :gc[i]], group=int(group[i]))
        return m, (time.perf_counter() - t0) * 1e3

    def run_c(m):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = m.result(dev)
        return (time.perf_counter() - t0) * 1e3, res["ap"]

    def run_call(tensors, groups):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = ops.det_map(*tensors, iou_thrs=thr_dev, n_groups=groups)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out[0].cpu().numpy()

    thr_dev = torch.tensor(THRS, dtype=torch.float32, device=dev)
    m, update_ms = filled()
    big = [torch.cat([t] * args.scale).contiguous() for t in d_in]
    big[1] = (big[1] - torch.rand(big[1].shape[0], 1, device=dev) * 1e-3).contiguous()      # per-map offset: descending order kept, fewer exact ties
    mb = DetMap(iou_thrs=THRS, n_groups=A)
    mb.update_batch(*big)
    run_b(), run_c(m), run_call(d_in, A), run_call(big, A)          # warm-up: allocator, first launches
    tb, tc, tcall, tbig, tbig_res = [], [], [], [], []
    for _ in range(args.rounds):
        ms, ap_b = run_b()
        tb.append(ms)
        ms, ap_c = run_c(m)
        tc.append(ms)
        ms, ap_call = run_call(d_in, A)
        tcall.append(ms)
        ms, _ = run_call(big, A)
        tbig.append(ms)
        ms, _ = run_c(mb)
        tbig_res.append(ms)
    # (a): the host path on a fraction of the split
    hf = min(args.host_frames, F)
    t0 = time.perf_counter()
    ap_a = []
    for a in range(A):
        idx = np.nonzero(group == a)[0][:hf]
        dets = [{"corners": P.box_corners(det[i, :dc[i]]), "scores": sc[i, :dc[i]]} for i in idx]
        anns = [P.box_corners(gt[i, :gc[i]].astype(np.float64)) for i in idx]
        ap_a.append([P.eval_map(dets, anns, thr)[0] for thr in THRS])
    host_ms = (time.perf_counter() - t0) * 1e3
    med = lambda v: float(np.median(v))
    n_det = int(dc.sum())
    lines = ["detection mAP of %d agents x %d frames (%d maps, %d detections, %d ground truths; thresholds %s) on %s; medians of %d alternating rounds" % (
                 A, F, n, n_det, int(gc.sum()), THRS, torch.cuda.get_device_name(0), args.rounds),
             "mean AP over agents: DetMap %s   eval_map_device %s" % (np.round(ap_c.mean(0), 6).tolist(), np.round(ap_b.mean(0), 6).tolist()),
             "(a) eval_map, host (the tool today)  : %10.1f ms for %d frames per agent = %.0f ms for the split (scaled x%.0f; 2 thresholds x %d agents)" % (
                 host_ms, hf, host_ms * F / hf, F / hf, A),
             "(b) eval_map_device, %2d calls        : %10.1f ms (min %.1f)" % (A * len(THRS), med(tb), min(tb)),
             "(c) DetMap.result(), all of it       : %10.1f ms (min %.1f; host padding + one upload + the call + download; the %d update() calls before it: %.0f ms)" % (
                 med(tc), min(tc), n, update_ms),
             "    one v2x_det_map call alone       : %10.3f ms (min %.3f; device events, 4 launches, workspace %d bytes)" % (med(tcall), min(tcall), 2 * n * det.shape[1]),
             "(c) at %2dx the maps (%d maps)     : %10.3f ms the call alone (min %.3f); DetMap.result() from update_batch %.1f ms" % (
                 args.scale, n * args.scale, med(tbig), min(tbig), med(tbig_res)),
             "largest |DetMap - eval_map_device| over the table %.3g; |the call alone - DetMap| %.3g" % (
                 float(np.abs(ap_c - ap_b).max()), float(np.abs(ap_call - ap_c).max()))]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

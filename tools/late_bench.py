#!/usr/bin/env python3
"""Time of late fusion (csrc/late_fuse.hip: late_fuse_kernel) at the bench size: 320 egos (5 agents x 64 frames), every agent's detections those
of a scene of `--cars` cars seen within 30 m, with noise.  Three figures, none asserted:
  * the fused call (v2x_det_late_fuse: one launch when no ego is pending, the second returns at once);
  * v2x_det_nms_candidates on the same 320 maps (the per-agent NMS that precedes it in FaFModule.predict_all), for scale;
  * the numpy path (utils/postprocess.late_fusion) on the same detections.

    python3 tools/late_bench.py [--frames 64] [--cars 40] [--cap 4096] [--out profiles/late_fuse_bench.txt]
"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_input(A, B, cars, cap, seed=0):
    """-> boxes (A*B, cap, 5), scores (A*B, cap), counts (A*B,), trans (B, A, A, 4, 4) in the dataset's convention."""
    rng = np.random.default_rng(seed)
    boxes = np.zeros((A * B, cap, 5), np.float32)
    scores = np.zeros((A * B, cap), np.float32)
    counts = np.zeros(A * B, np.int32)
    trans = np.zeros((B, A, A, 4, 4), np.float32)
    for b in range(B):
        world = []
        while len(world) < cars:
            c = rng.uniform(-40, 40, 2)
            if all(np.hypot(*(c - o[:2])) > 6.0 for o in world):
                world.append(np.array([c[0], c[1], 2.0 + rng.uniform(-0.15, 0.15), 4.4 + rng.uniform(-0.4, 0.4), rng.uniform(-math.pi, math.pi)]))
        world = np.asarray(world)
        poses = []
        for _ in range(A):
            yaw, x, y = rng.uniform(-math.pi, math.pi), *rng.uniform(-12, 12, 2)
            M = np.eye(4)
            M[0, 0], M[0, 1], M[1, 0], M[1, 1], M[0, 3], M[1, 3] = math.cos(yaw), -math.sin(yaw), math.sin(yaw), math.cos(yaw), x, y
            poses.append(M)
        for i in range(A):
            for j in range(A):
                G = np.linalg.inv(poses[i]) @ poses[j]
                trans[b, i, j] = G
                trans[b, i, j, 0, 3], trans[b, i, j, 1, 3] = -G[1, 3], G[0, 3]
        for j in range(A):
            inv = np.linalg.inv(poses[j])
            near = np.hypot(world[:, 0] - poses[j][0, 3], world[:, 1] - poses[j][1, 3]) <= 30.0
            d = world[near].copy()
            n = d.shape[0]
            d[:, :2] = (d[:, :2] + rng.normal(0, 0.1, (n, 2))) @ inv[:2, :2].T + inv[:2, 3]
            d[:, 2:4] *= 1 + rng.normal(0, 0.03, (n, 2))
            d[:, 4] += rng.normal(0, 0.05, n) - math.atan2(poses[j][1, 0], poses[j][0, 0])
            d = d[(np.abs(d[:, 0]) < 32) & (np.abs(d[:, 1]) < 32)]
            n = d.shape[0]
            s = np.sort(rng.uniform(0.7, 0.999, n))[::-1]
            boxes[j * B + b, :n], scores[j * B + b, :n], counts[j * B + b] = d, s, n
    return boxes, scores, counts, trans


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", default=5, type=int)
    ap.add_argument("--frames", default=64, type=int)
    ap.add_argument("--cars", default=40, type=int)
    ap.add_argument("--cap", default=4096, type=int, help="cap_in = cap_out, FaFModule.cap")
    ap.add_argument("--iters", default=200, type=int)
    ap.add_argument("--rounds", default=5, type=int)
    ap.add_argument("--out", default="", type=str)
    args = ap.parse_args(argv)
    from v2x_sim_amd import ops
    from v2x_sim_amd.utils import postprocess as P
    if not torch.cuda.is_available():
        raise SystemExit("late_bench.py measures on the MI355X: no GPU, no figure")
    dev = torch.device("cuda:0")
    A, B, cap = args.agents, args.frames, args.cap
    extents = ((-32.0, 32.0), (-32.0, 32.0))
    boxes, scores, counts, trans = make_input(A, B, args.cars, cap)
    d_boxes, d_scores, d_counts = (torch.from_numpy(a).to(dev) for a in (boxes, scores, counts))
    rigid = torch.from_numpy(P.late_rigid_from_trans(trans)).to(dev)
    link = torch.ones((B, A, A), dtype=torch.uint8, device=dev)
    # the same maps as candidates of the per-agent NMS: one unit anchor at the origin, code = (x, y, log w, log h, sin yaw, cos yaw)
    n = A * B
    anchors = torch.tensor([[0.0, 0.0, 1.0, 1.0, 0.0, 1.0]], dtype=torch.float32, device=dev).repeat(64, 1)
    codes = np.zeros((n, cap, 6), np.float32)
    codes[..., 0:2] = boxes[..., 0:2]
    codes[..., 2:4] = np.log(np.maximum(boxes[..., 2:4], 1e-3))
    codes[..., 4], codes[..., 5] = np.sin(boxes[..., 4]), np.cos(boxes[..., 4])
    slot = np.arange(cap, dtype=np.uint64)[None, :]
    keys = ((~scores.view(np.uint32)).astype(np.uint64) & np.uint64(0xffffffff)) << np.uint64(32) | slot
    d_keys, d_codes = torch.from_numpy(keys.view(np.int64)).to(dev), torch.from_numpy(codes).to(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.iters

    fuse = lambda: ops.late_fuse(d_boxes, d_scores, d_counts, rigid, link, extents, 0.01, cap_out=cap)
    nms = lambda: ops.det_nms_candidates(d_keys, d_codes, d_counts, anchors, 0.01)
    out = fuse()
    pre = nms()
    torch.cuda.synchronize()
    fcount, pcount = out[3].cpu().numpy(), pre[3].cpu().numpy()
    assert (fcount >= 0).all() and (pcount >= 0).all(), "the bench input must stay within the capacities"
    src_agent = out[2].cpu().numpy() // cap
    from_nb = sum(int((src_agent[r, :fcount[r]] != r // B).sum()) for r in range(n))
    timed(fuse), timed(nms)
    t_fuse = [timed(fuse) for _ in range(args.rounds)]
    t_nms = [timed(nms) for _ in range(args.rounds)]
    t_alt = [(timed(fuse), timed(nms)) for _ in range(args.rounds)]       # alternating: the same figures with the two interleaved

    seq = [[{"boxes": boxes[j * B + b, :counts[j * B + b]], "scores": scores[j * B + b, :counts[j * B + b]]} for b in range(B)] for j in range(A)]
    t0 = time.perf_counter()
    host = P.late_fusion(seq, trans, A, extents)
    t_host = time.perf_counter() - t0
    same = all(len(host[i][b]["scores"]) == fcount[i * B + b] for i in range(A) for b in range(B))

    med = lambda v: float(np.median(v))
    lines = ["late_fuse_kernel: %d egos (%d agents x %d frames), cap_in = cap_out = %d; medians of %d rounds x %d calls on %s"
             % (n, A, B, cap, args.rounds, args.iters, torch.cuda.get_device_name(0)),
             "per agent %.1f detections (max %d); per ego %.1f kept after fusion (max %d), %.1f of them from neighbours"
             % (counts.mean(), counts.max(), fcount.mean(), fcount.max(), from_nb / n),
             "v2x_det_late_fuse (2 launches, the second returns at once)      : %8.1f us per call   [rounds: %s]" % (med(t_fuse), " ".join("%.1f" % v for v in t_fuse)),
             "v2x_det_nms_candidates on the same %d maps, for scale           : %8.1f us per call   [rounds: %s]" % (n, med(t_nms), " ".join("%.1f" % v for v in t_nms)),
             "interleaved                                                      : %8.1f / %.1f us" % (med([a for a, _ in t_alt]), med([b for _, b in t_alt])),
             "numpy path (utils/postprocess.late_fusion), one call, host clock : %8.1f ms  (same counts as the kernel: %s)" % (1e3 * t_host, same),
             "times include the python wrapper's four output allocations (torch.empty) per call"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What scoring the HOTA family costs (csrc/hota.hip) at the size of a test split: 50 sequences x 100 frames x 40 objects, three ways --
(1) ONE v2x_hota_sequences call on padded device arrays (device events around the call: its five launches and nothing else), and the whole of
`Hota.result()` around it (padding on the host, upload, the call, download: a host clock that ends in a synchronise);
(2) the float64 reference of tests/hota_refs.py on the host (timed on --host_seqs sequences and scaled);
(3) for scale, `ClearMot`'s per-frame path (one assignment launch and three host synchronisations per frame; timed on --clear_seqs sequences and scaled).
Nothing here is asserted, and the host reference being faster than the device call is a result like any other: the metric lives in the library because the
product has no CPU path, not because it is slow.

    python3 tools/hota_bench.py [--seqs 50] [--frames 100] [--objects 40] [--out profiles/hota_bench.txt]

Scene per sequence: `objects` boxes of 4.5 x 2 m on a jittered 8 m grid with constant velocities; a track = the object's box with 0.15 m centre noise and 3 %
size noise, missing in 10 % of the frames, under an id that changes at two random frames of the sequence; up to two stray tracks per frame."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_sequence(seed, objects, frames):
    """-> hota_refs frames: [(gt_boxes float32 [n][4], gt_ids, trk_boxes float32 [m][4], trk_ids)]."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(objects)))
    grid = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:objects] * 8.0
    pos = grid + rng.uniform(-1.5, 1.5, (objects, 2))
    vel = rng.uniform(-0.3, 0.3, (objects, 2))
    size = np.array([4.5, 2.0])
    cuts = np.sort(rng.integers(1, frames, (objects, 2)), 1)
    out, stray = [], 0
    for f in range(frames):
        c = pos + vel * f
        gt = np.concatenate([c - size / 2, c + size / 2], 1).astype(np.float32)
        cn = c + rng.normal(0, 0.15, c.shape)
        sz = size * (1 + 0.03 * rng.normal(0, 1, c.shape))
        tb = np.concatenate([cn - sz / 2, cn + sz / 2], 1)
        seen = rng.random(objects) >= 0.10
        ids = (np.arange(objects) * 3 + (f >= cuts[:, 0]) + (f >= cuts[:, 1]))[seen].tolist()
        tb = tb[seen]
        for _ in range(int(rng.integers(0, 3))):
            cs = rng.uniform(0, 8.0 * side, 2)
            tb = np.concatenate([tb, np.concatenate([cs - size / 2, cs + size / 2])[None]])
            ids.append(10 ** 6 + stray)
            stray += 1
        out.append((gt, list(range(objects)), tb.astype(np.float32), ids))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", default=50, type=int)
    ap.add_argument("--frames", default=100, type=int)
    ap.add_argument("--objects", default=40, type=int)
    ap.add_argument("--rounds", default=7, type=int)
    ap.add_argument("--host_seqs", default=2, type=int)
    ap.add_argument("--clear_seqs", default=2, type=int)
    ap.add_argument("--out", default="", type=str)
    args = ap.parse_args(argv)
    from v2x_sim_amd import _lib, ops
    from v2x_sim_amd.utils.mot_metrics import ClearMot, Hota
    import hota_refs as H
    dev = torch.device("cuda:0")
    seqs = [make_sequence(s, args.objects, args.frames) for s in range(args.seqs)]
    on_dev = [[(torch.from_numpy(g).to(dev), gi, torch.from_numpy(t).to(dev), ti) for g, gi, t, ti in q] for q in seqs]

    # (1) the whole of Hota.result(), and the library call alone on the arrays it builds
    def collected():
        m = Hota()
        for q in on_dev:
            for fr in q:
                m.update(*fr)
            m.new_sequence()
        return m

    def whole():
        m = collected()
        t0 = time.perf_counter()
        r = m.result()                                                   # ends in the download of the outputs: synchronised
        return r, time.perf_counter() - t0

    res, _ = whole()
    whole_s = [whole()[1] for _ in range(args.rounds)]
    a = collected().padded()
    S, F, cap = a[0].shape[:3]
    n_gt_ids, n_trk_ids = a[6], a[7]
    ws_bytes = _lib.load().v2x_hota_workspace_size(S, F, cap, n_gt_ids, n_trk_ids, len(H.ALPHAS))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    timed(lambda: ops.hota_sequences(*a))
    call_ms = [timed(lambda: ops.hota_sequences(*a)) for _ in range(args.rounds)]   # includes the allocation of the workspace and of the outputs (torch's cache)

    # (2) the float64 reference on the host
    hs = min(args.host_seqs, args.seqs)
    t0 = time.perf_counter()
    refs = [H.score_sequence(q) for q in seqs[:hs]]
    host = (time.perf_counter() - t0) / hs
    dev_max = max(float(np.abs(res["sequences"][s]["per_alpha"]["AssA"] - refs[s]["AssA"]).max()) for s in range(hs))
    same = all(res["sequences"][s]["per_alpha"]["TP"].tolist() == refs[s]["TP"].tolist() for s in range(hs))

    # (3) ClearMot, frame by frame
    cs = min(args.clear_seqs, args.seqs)
    ClearMot().update(*on_dev[0][0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for q in on_dev[:cs]:
        c = ClearMot()
        for fr in q:
            c.update(*fr)
    clear = (time.perf_counter() - t0) / cs

    lines = ["HOTA of %d sequences x %d frames x %d objects on %s (padded: cap %d, %d ground-truth ids, %d track ids per sequence; medians of %d rounds)"
             % (S, F, args.objects, torch.cuda.get_device_name(0), cap, n_gt_ids, n_trk_ids, args.rounds),
             "combined HOTA %.4f DetA %.4f AssA %.4f LocA %.4f" % (res["HOTA"], res["DetA"], res["AssA"], res["LocA"]),
             "one v2x_hota_sequences call : %9.3f ms (device events; 5 launches, workspace %d bytes = %.1f MiB)" % (float(np.median(call_ms)), ws_bytes,
                                                                                                                 ws_bytes / 2.0 ** 20),
             "Hota.result(), all of it    : %9.3f ms (host padding + upload + the call + download)" % (1e3 * float(np.median(whole_s))),
             "host reference (hota_refs)  : %9.3f ms per sequence (float64 numpy + python assignment, %d sequences) = %.0f ms for %d sequences (scaled)"
             % (1e3 * host, hs, 1e3 * host * S, S),
             "ClearMot, frame by frame    : %9.3f ms per sequence (%d sequences) = %.0f ms for %d sequences (scaled); it scores MOTA / MOTP, not HOTA: for scale"
             % (1e3 * clear, cs, 1e3 * clear * S, S),
             "agreement with the reference on those %d sequences: TP equal for every alpha: %s; largest |AssA - reference| %.3g" % (hs, same, dev_max)]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

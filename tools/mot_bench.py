#!/usr/bin/env python3
"""What scoring the CLEAR MOT and Identity families costs (csrc/mot_seq.hip) at the size of a test split: 50 sequences x 100 frames x 40 objects
(tools/hota_bench.py's scenes, generated the same way), four measurements --
(1) ONE v2x_mot_sequences call on padded device arrays: device events around the call (its five launches and torch's cached allocation of the workspace
    and the outputs), the median of --rounds calls after a warm-up call;
(2) the whole of `ClearIdentity.result()` around it (padding on the host, upload, the call, download: a host clock that ends in a synchronise);
(3) the per-frame `ClearMot` (one assignment launch and several host synchronisations per frame) on --clear_seqs sequences, scaled to the split: the
    path the batched call replaces in tools/track/eval_track.py, and the baseline;
(4) the call on ONE identity-stress sequence of --stress_ids x --stress_ids ids (tests/mot_refs.py::group_frames: a dense integer pmc), where the wide
    assignment dominates.
Agreement with the float64 reference (tests/mot_refs.py) on --host_seqs sequences is printed with the largest |MOTP_sum - reference| and its bound.
Nothing here is asserted.

    python3 tools/mot_bench.py [--seqs 50] [--frames 100] [--objects 40] [--out profiles/mot_bench.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", default=50, type=int)
    ap.add_argument("--frames", default=100, type=int)
    ap.add_argument("--objects", default=40, type=int)
    ap.add_argument("--rounds", default=15, type=int)
    ap.add_argument("--host_seqs", default=2, type=int)
    ap.add_argument("--clear_seqs", default=2, type=int)
    ap.add_argument("--stress_ids", default=200, type=int)
    ap.add_argument("--stress_frames", default=60, type=int)
    ap.add_argument("--out", default="", type=str)
    args = ap.parse_args(argv)
    from v2x_sim_amd import _lib, ops
    from v2x_sim_amd.utils.mot_metrics import ClearIdentity, ClearMot
    from hota_bench import make_sequence
    import mot_refs as M
    dev = torch.device("cuda:0")
    seqs = [make_sequence(s, args.objects, args.frames) for s in range(args.seqs)]

    def on_device(q):
        return [(torch.from_numpy(g).to(dev), gi, torch.from_numpy(t).to(dev), ti) for g, gi, t, ti in q]

    on_dev = [on_device(q) for q in seqs]

    def collected(split):
        m = ClearIdentity()
        for q in split:
            for fr in q:
                m.update(*fr)
            m.new_sequence()
        return m

    def whole():
        m = collected(on_dev)
        t0 = time.perf_counter()
        r = m.result()                                                   # ends in the download of the outputs: synchronised
        return r, time.perf_counter() - t0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def call_ms(a):
        timed(lambda: ops.mot_sequences(*a))                             # warm-up: code objects, torch's allocator
        return [timed(lambda: ops.mot_sequences(*a)) for _ in range(args.rounds)]

    # (1), (2)
    res, _ = whole()
    whole_s = [whole()[1] for _ in range(max(3, args.rounds // 3))]
    a = collected(on_dev).padded()
    S, F, cap = a[0].shape[:3]
    ws_bytes = _lib.load().v2x_mot_workspace_size(S, F, cap, a[6], a[7])
    split_ms = call_ms(a)

    # agreement with the float64 reference
    hs = min(args.host_seqs, args.seqs)
    refs = [M.score_sequence(q) for q in seqs[:hs]]
    same = all(all(res["sequences"][s][k] == refs[s][k] for k in M.COUNTS) for s in range(hs))
    dev_max = max(abs(res["sequences"][s]["MOTP_sum"] - refs[s]["MOTP_sum"]) for s in range(hs))
    bound = min(M.motp_bound(r) for r in refs)

    # (3) ClearMot, frame by frame
    cs = min(args.clear_seqs, args.seqs)
    ClearMot().update(*on_dev[0][0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    online = []
    for q in on_dev[:cs]:
        c = ClearMot()
        for fr in q:
            c.update(*fr)
        online.append(c)
    clear = (time.perf_counter() - t0) / cs
    witness = all((c.tp, c.fn, c.fp, c.idsw) == tuple(res["sequences"][s][k] for k in ("TP", "FN", "FP", "IDSW")) for s, c in enumerate(online))

    # (4) one identity-stress sequence
    stress = M.group_frames(99, args.stress_ids, args.stress_ids, args.stress_frames)
    sa = collected([on_device(stress)]).padded()
    stress_ms = call_ms(sa)
    sres = collected([on_device(stress)]).result()
    sref = M.score_sequence(stress)

    split_med, whole_med = float(np.median(split_ms)), 1e3 * float(np.median(whole_s))
    lines = ["CLEAR MOT + Identity of %d sequences x %d frames x %d objects on %s (padded: cap %d, %d ground-truth ids, %d track ids per sequence; medians of %d "
             "calls after one warm-up call)" % (S, F, args.objects, torch.cuda.get_device_name(0), cap, a[6], a[7], args.rounds),
             "combined MOTA %.4f MOTP %.4f IDSW %d IDF1 %.4f IDR %.4f IDP %.4f MT %d PT %d ML %d Frag %d"
             % tuple(res[k] for k in ("MOTA", "MOTP", "IDSW", "IDF1", "IDR", "IDP", "MT", "PT", "ML", "Frag")),
             "one v2x_mot_sequences call  : %9.3f ms (device events; min %.3f, max %.3f; 5 launches, workspace %d bytes = %.1f MiB)"
             % (split_med, min(split_ms), max(split_ms), ws_bytes, ws_bytes / 2.0 ** 20),
             "ClearIdentity.result()      : %9.3f ms (host padding + upload + the call + download)" % whole_med,
             "ClearMot, frame by frame    : %9.3f ms per sequence (%d sequences) = %.0f ms for %d sequences (scaled): the baseline; %.0f x the call, %.1f x "
             "ClearIdentity.result()" % (1e3 * clear, cs, 1e3 * clear * S, S, 1e3 * clear * S / split_med, 1e3 * clear * S / whole_med),
             "one stress sequence         : %9.3f ms (device events; %d frames, %d x %d ids, IDTP %d, greedy would reach %d; reference IDTP %d)"
             % (float(np.median(stress_ms)), args.stress_frames, sa[6], sa[7], sres["IDTP"], M.identity_greedy(sref["pmc"]), sref["IDTP"]),
             "agreement with the float64 reference on %d sequences: the eleven integers equal: %s; largest |MOTP_sum - reference| %.3g (bound (TP + 2) 2^-52 "
             "MOTP_sum = %.3g); ClearMot's TP / FN / FP / IDSW equal on its %d sequences: %s" % (hs, same, dev_max, bound, cs, witness)]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

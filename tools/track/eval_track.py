#!/usr/bin/env python3
"""Tracking scorer (row f-5): two directories of MOT-challenge text -> the benchmark's tracking columns.

    python tools/track/eval_track.py --gt gt_tracks/ --trk tracks/ [--out scores.json]

Both directories hold text files of lines `frame,id,x1,y1,w,h,...` (the track side is what track_codet.py writes; further columns are ignored).  Files
are paired by their path relative to the directory; a file present on one side only is scored against an empty sequence, and the tool says so.  A
sequence's frames are the numbers from the first to the last frame either file names (a frame neither names is an empty frame).
One table row per file and one combined row -- TrackEval's default metric set: HOTA, DetA, AssA, DetRe, DetPr, AssRe, AssPr, LocA
(v2x_sim_amd/utils/mot_metrics.py::Hota: all files in ONE library call), MOTA, MOTP, IDSW, MT, ML, Frag (CLEAR) and IDF1, IDR, IDP (Identity), the last
two families from `ClearIdentity`: all files in ONE more library call; the combined row follows TrackEval's combination rules (counts add).
`--out` writes the same record as JSON, which additionally holds PT, the CLEAR and ID counts (TP, FN, FP, IDTP, IDFN, IDFP, MOTP_sum), MODA, sMOTA,
CLR_Re, CLR_Pr and OWTA, HOTA(0), LocA(0), HOTALocA(0); main(argv) returns it.  At most 64 boxes per frame and side, 2048 ids per file and side."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

COLUMNS = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA", "MOTA", "MOTP", "IDSW", "IDF1", "IDR", "IDP", "MT", "ML", "Frag")
INT_COLUMNS = ("IDSW", "MT", "ML", "Frag")


def read_mot(path):
    """MOT-challenge text -> {frame: (ids [n] list of int, boxes float32 [n][4] as x1, y1, x2, y2)}; blank lines and lines starting with # are skipped."""
    rows = {}
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            v = line.split(",")
            if len(v) < 6:
                raise ValueError("%s:%d: expected frame,id,x1,y1,w,h,..., got %r" % (path, no, line))
            x1, y1, w, h = (float(t) for t in v[2:6])
            ids, boxes = rows.setdefault(int(float(v[0])), ([], []))
            ids.append(int(float(v[1])))
            boxes.append((x1, y1, x1 + w, y1 + h))
    return {f: (ids, np.array(boxes, dtype=np.float32).reshape(-1, 4)) for f, (ids, boxes) in rows.items()}


def list_files(root):
    out = []
    for base, _, names in os.walk(root):
        out += [os.path.relpath(os.path.join(base, n), root) for n in names if n.endswith(".txt")]
    return sorted(out)


def sequence_frames(gt, trk):
    """Two read_mot records -> [(gt_ids, gt_boxes, trk_ids, trk_boxes)] for every frame number from the first to the last either side names."""
    numbers = list(gt) + list(trk)
    if not numbers:
        return []
    none = ([], np.zeros((0, 4), dtype=np.float32))
    return [gt.get(f, none) + trk.get(f, none) for f in range(min(numbers), max(numbers) + 1)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gt", required=True, type=str, help="directory of ground-truth MOT-challenge text files")
    ap.add_argument("--trk", required=True, type=str, help="directory of tracker output (tools/track/track_codet.py --out)")
    ap.add_argument("--out", default="", type=str, help="write the record as JSON")
    args = ap.parse_args(argv)
    import torch
    from v2x_sim_amd.utils.mot_metrics import HOTA_FIELDS, ClearIdentity, Hota, hota_extras

    if not torch.cuda.is_available():
        raise SystemExit("eval_track.py needs the MI355X: the hot path has no CPU fallback")
    device = torch.device("cuda:0")
    gt_files, trk_files = set(list_files(args.gt)), set(list_files(args.trk))
    names = sorted(gt_files | trk_files)
    if not names:
        raise SystemExit("no .txt files under %s or %s" % (args.gt, args.trk))
    hota, clear, notes = Hota(), ClearIdentity(), []
    for name in names:
        note = "" if name in gt_files and name in trk_files else ("no tracker file: scored as an empty sequence" if name in gt_files
                                                                  else "no ground-truth file: scored as an empty sequence")
        if note:
            print("%s: %s" % (name, note))
        notes.append(note)
        gt = read_mot(os.path.join(args.gt, name)) if name in gt_files else {}
        trk = read_mot(os.path.join(args.trk, name)) if name in trk_files else {}
        frames = sequence_frames(gt, trk)
        gb = torch.from_numpy(np.concatenate([f[1] for f in frames] + [np.zeros((0, 4), np.float32)])).to(device)      # one upload per side and file
        tb = torch.from_numpy(np.concatenate([f[3] for f in frames] + [np.zeros((0, 4), np.float32)])).to(device)
        g0 = t0 = 0
        for gi, gbox, ti, tbox in frames:
            g1, t1 = g0 + len(gi), t0 + len(ti)
            hota.update(gb[g0:g1], gi, tb[t0:t1], ti)
            clear.update(gb[g0:g1], gi, tb[t0:t1], ti)
            g0, t0 = g1, t1
        hota.new_sequence()
        clear.new_sequence()
    res, cres = hota.result(), clear.result()

    def row(name, h, c, note=""):
        r = {"name": name}
        r.update({k: h[k] for k in HOTA_FIELDS})
        r.update(hota_extras(h))
        r.update({k: v for k, v in c.items() if k != "sequences"})
        if note:
            r["note"] = note
        return r

    record = {"files": [row(n, h, c, note) for n, h, c, note in zip(names, res["sequences"], cres["sequences"], notes)],
              "combined": row("COMBINED", res, cres)}
    width = max(len(n) for n in names + ["COMBINED"])
    print("%-*s " % (width, "file") + " ".join("%7s" % c for c in COLUMNS))
    for r in record["files"] + [record["combined"]]:
        print("%-*s " % (width, r["name"]) + " ".join(("%7d" % r[c]) if c in INT_COLUMNS else ("%7.4f" % r[c]) for c in COLUMNS))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(record, fh, indent=1)
    return record


if __name__ == "__main__":
    main()

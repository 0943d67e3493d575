"""Row f-5: the CLEAR MOT metric (MOTA / MOTP / ID switches) in TrackEval's reading (clear.py).

Per frame: similarity = IoU of the axis-aligned boxes (torch, fp64 on the device), threshold 0.5, score = 1000 [the GT's tracker id of the
PREVIOUS frame == this tracker id] + IoU with the entries below the threshold zeroed, optimal assignment, matched = score > 0.

The assignment runs on `ops.assign_iou` (the tracker's own association kernel).  The +1000 continuity term is handled by taking the
continuity-preferred pairs FIRST, not by scaling (1000 + IoU in fp32 would leave 14 bits of the IoU): a GT has at most one previous tracker id
and a tracker id at most one GT, so the continuity pairs above the threshold form a partial matching by themselves, and because one bonus
outweighs any sum of IoUs (<= 64) every optimum of TrackEval's score contains all of them (replacing the two pairs that block one loses < 2 and
wins > 1000).  They are fixed, their rows and columns zeroed, and the kernel assigns the rest on the thresholded IoUs: the same optimum.

The HOTA family (`Hota`; TrackEval's hota.py) is frame-independent once the global alignment score is known, so it is NOT scored
frame by frame: `update` only collects, `result` pads every sequence to one shape and makes ONE `ops.hota_sequences` call (csrc/hota.hip, five launches)
for all of them; what remains on the host is the arithmetic on 19 x 7 numbers per sequence.  `hota_extras` adds OWTA and the `(0)` variants from that record.

`ClearIdentity` scores CLEAR MOT (with MT / PT / ML / Frag) and the Identity family (IDF1, IDR, IDP) of whole sequences the same way: collect, pad (one padding
for both classes), ONE `ops.mot_sequences` call (csrc/mot_seq.hip, five launches: the frames of a sequence are walked in order by one wave, the ID assignment
over the sequence's id space by one workgroup).  `ClearMot` stays the online class for a tracker that is scored while it runs."""
import numpy as np
import torch

from .. import ops_track


def _iou64(a, b):
    a = a.to(torch.float64)[:, None, :]
    b = b.to(torch.float64)[None, :, :]
    w = (torch.minimum(a[..., 2], b[..., 2]) - torch.maximum(a[..., 0], b[..., 0])).clamp_min(0)
    h = (torch.minimum(a[..., 3], b[..., 3]) - torch.maximum(a[..., 1], b[..., 1])).clamp_min(0)
    wh = w * h
    o = wh / ((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - wh)
    return torch.where(torch.isfinite(o), o, torch.zeros_like(o))


class ClearMot(object):
    """update(gt_boxes (G, 4), gt_ids (G,), trk_boxes (T, 4), trk_ids (T,)) per frame, boxes x1, y1, x2, y2 on the device, G, T <= 64;
    result() -> MOTA, MOTP, IDSW, TP, FP, FN."""

    def __init__(self, threshold=0.5):
        self.threshold = float(threshold)
        self.tp = self.fp = self.fn = self.idsw = 0
        self.iou_sum = 0.0
        self._prev = {}
        self._prev_step = {}

    def update(self, gt_boxes, gt_ids, trk_boxes, trk_ids):
        if not gt_boxes.is_cuda or not trk_boxes.is_cuda:
            raise RuntimeError("ClearMot runs on the MI355X (cuda) device; the v2x_sim_amd hot path has no CPU fallback")
        gt_ids = [int(g) for g in (gt_ids.tolist() if torch.is_tensor(gt_ids) else gt_ids)]
        trk_ids = [int(t) for t in (trk_ids.tolist() if torch.is_tensor(trk_ids) else trk_ids)]
        ng, nt = len(gt_ids), len(trk_ids)
        cap = ops_track.TRACK_CAP
        if ng > cap or nt > cap:
            raise ValueError("ClearMot takes at most %d ground-truth boxes and %d tracks per frame" % (cap, cap))
        if ng == 0 or nt == 0:
            self.fn += ng
            self.fp += nt
            self._prev_step = {}
            return
        sim = _iou64(gt_boxes.reshape(ng, 4), trk_boxes.reshape(nt, 4))
        eps = torch.finfo(torch.float64).eps
        sim_t = torch.where(sim < self.threshold - eps, torch.zeros_like(sim), sim)
        sim_h = sim_t.cpu()
        col = {t: c for c, t in enumerate(trk_ids)}
        pairs = []
        for r, g in enumerate(gt_ids):                      # the continuity-preferred pairs first (module docstring)
            c = col.get(self._prev_step.get(g), -1)
            if c >= 0 and float(sim_h[r, c]) > 0:
                pairs.append((r, c))
        rest = sim_t.clone()
        if pairs:
            idx = torch.as_tensor(pairs, dtype=torch.long, device=rest.device)
            rest[idx[:, 0], :] = 0
            rest[:, idx[:, 1]] = 0
        m = torch.zeros((1, cap, cap), dtype=torch.float32, device=rest.device)
        m[0, :ng, :nt] = rest.to(torch.float32)
        n_r = torch.full((1,), ng, dtype=torch.int32, device=rest.device)
        n_c = torch.full((1,), nt, dtype=torch.int32, device=rest.device)
        r2c = ops_track.assign_iou(m, n_r, n_c, thr=self.threshold, direct=False)[0, :ng].tolist()
        pairs += [(r, c) for r, c in enumerate(r2c) if c >= 0 and float(sim_h[r, c]) > 0]
        step = {}
        for r, c in pairs:
            g, t = gt_ids[r], trk_ids[c]
            if g in self._prev and self._prev[g] != t:
                self.idsw += 1
            step[g] = t
            self.iou_sum += float(sim_h[r, c])
        self._prev.update(step)
        self._prev_step = step
        self.tp += len(step)
        self.fn += ng - len(step)
        self.fp += nt - len(step)

    def result(self):
        gt = self.tp + self.fn
        return {"MOTA": (self.tp - self.fp - self.idsw) / gt if gt else 0.0, "MOTP": self.iou_sum / self.tp if self.tp else 0.0,
                "IDSW": self.idsw, "TP": self.tp, "FP": self.fp, "FN": self.fn}


HOTA_FIELDS = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")


def _hota_fields(tp, fn, fp, loc, ass_a, ass_re, ass_pr, alphas):
    """Per-alpha arrays of one sequence or of a combination -> the result record (scalars = means over alpha)."""
    tpf, fnf, fpf = tp.astype(np.float64), fn.astype(np.float64), fp.astype(np.float64)
    det_a = tpf / np.maximum(1, tpf + fnf + fpf)
    per = {"HOTA": np.sqrt(det_a * ass_a), "DetA": det_a, "AssA": ass_a, "DetRe": tpf / np.maximum(1, tpf + fnf), "DetPr": tpf / np.maximum(1, tpf + fpf),
           "AssRe": ass_re, "AssPr": ass_pr, "LocA": np.maximum(1e-10, loc) / np.maximum(1e-10, tpf), "TP": tp, "FN": fn, "FP": fp, "loc": loc}
    out = {k: float(np.mean(per[k])) for k in HOTA_FIELDS + ("TP", "FN", "FP")}
    out["alphas"] = alphas
    out["per_alpha"] = per
    return out


def _checked_frame(who, gt_boxes, gt_ids, trk_boxes, trk_ids):
    """One frame as the collecting metrics (Hota, ClearIdentity) keep it: (gt_boxes float32 (G, 4) on the device, gt_ids list, trk_boxes, trk_ids)."""
    if not gt_boxes.is_cuda or not trk_boxes.is_cuda:
        raise RuntimeError("%s runs on the MI355X (cuda) device; the v2x_sim_amd hot path has no CPU fallback" % who)
    gt_ids = [int(g) for g in (gt_ids.tolist() if torch.is_tensor(gt_ids) else gt_ids)]
    trk_ids = [int(t) for t in (trk_ids.tolist() if torch.is_tensor(trk_ids) else trk_ids)]
    cap = ops_track.TRACK_CAP
    if len(gt_ids) > cap or len(trk_ids) > cap:
        raise ValueError("%s takes at most %d ground-truth boxes and %d tracks per frame" % (who, cap, cap))
    if len(set(gt_ids)) != len(gt_ids) or len(set(trk_ids)) != len(trk_ids):
        raise ValueError("%s: an id occurs twice in one frame" % who)
    return gt_boxes.reshape(len(gt_ids), 4).to(torch.float32), gt_ids, trk_boxes.reshape(len(trk_ids), 4).to(torch.float32), trk_ids


def _pad_sequences(seqs):
    """list (sequence) of lists of _checked_frame's frames -> every sequence padded to one shape, ids renumbered per sequence in order of first
    appearance: (gt_boxes, gt_ids, gt_count, trk_boxes, trk_ids, trk_count, n_gt_ids, n_trk_ids), or None without a sequence."""
    if not seqs:
        return None
    S = len(seqs)
    F = max([len(q) for q in seqs] + [1])
    cap = max([max(len(fr[1]), len(fr[3])) for q in seqs for fr in q] + [1])
    ids = np.zeros((2, S, F, cap), dtype=np.int32)
    count = np.zeros((2, S, F), dtype=np.int32)
    n_ids = [0, 0]
    boxes, dest = ([], []), ([], [])                    # per side: the frames' box tensors and their rows in the padded array
    for s, q in enumerate(seqs):
        remap = ({}, {})
        for f, fr in enumerate(q):
            for side in (0, 1):
                b, i = fr[2 * side], fr[2 * side + 1]
                n = len(i)
                ids[side, s, f, :n] = [remap[side].setdefault(v, len(remap[side])) for v in i]
                count[side, s, f] = n
                if n:
                    boxes[side].append(b)
                    dest[side].append((s * F + f) * cap + np.arange(n))
        n_ids = [max(n_ids[side], len(remap[side])) for side in (0, 1)]
    dev = next((b[0].device for b in boxes if b), torch.device("cuda", torch.cuda.current_device()))
    padded = []
    for side in (0, 1):
        p = torch.zeros((S * F * cap, 4), dtype=torch.float32, device=dev)
        if boxes[side]:
            p[torch.from_numpy(np.concatenate(dest[side])).to(dev)] = torch.cat(boxes[side])
        padded.append(p.view(S, F, cap, 4))
    ids_d, count_d = torch.from_numpy(ids).to(dev), torch.from_numpy(count).to(dev)
    return padded[0], ids_d[0], count_d[0], padded[1], ids_d[1], count_d[1], n_ids[0], n_ids[1]


class Hota(object):
    """update(gt_boxes (G, 4), gt_ids (G,), trk_boxes (T, 4), trk_ids (T,)) adds one frame to the current sequence (boxes x1, y1, x2, y2 on the device,
    read as float32; ids host integers of any value, unique within the frame; G, T <= 64), new_sequence() closes it.
    result() -> HOTA, DetA, AssA, DetRe, DetPr, AssRe, AssPr, LocA and TP, FN, FP as means over the thresholds, "alphas", "per_alpha" (the same
    fields and the matched-similarity sum "loc" as arrays), and "sequences": the same record for every sequence.  Sequences combine as TrackEval
    combines them: counts and loc add, AssA / AssRe / AssPr are TP-weighted means, the detection fields and HOTA are recomputed."""

    def __init__(self, alphas=None):
        self.alphas = np.array(ops_track.HOTA_ALPHAS if alphas is None else alphas, dtype=np.float64).reshape(-1)
        self._closed = []
        self._frames = []

    def update(self, gt_boxes, gt_ids, trk_boxes, trk_ids):
        self._frames.append(_checked_frame("Hota", gt_boxes, gt_ids, trk_boxes, trk_ids))

    def new_sequence(self):
        self._closed.append(self._frames)
        self._frames = []

    def padded(self):
        """Every sequence padded to one shape, ids renumbered per sequence in order of first appearance: the arguments of ops.hota_sequences --
        (gt_boxes, gt_ids, gt_count, trk_boxes, trk_ids, trk_count, n_gt_ids, n_trk_ids), or None without a sequence."""
        return _pad_sequences(self._closed + ([self._frames] if self._frames else []))

    def result(self):
        args = self.padded()
        A = len(self.alphas)
        S = 0 if args is None else args[0].shape[0]
        tp, fn, fp = (np.zeros((S, A), dtype=np.int64) for _ in range(3))
        ass, loc = np.zeros((S, A, 3)), np.zeros((S, A))
        if S:
            out_i, out_f = ops_track.hota_sequences(*args, alpha=torch.from_numpy(self.alphas).to(args[0].device))
            out_i, out_f = out_i.cpu().numpy().astype(np.int64), out_f.cpu().numpy()
            tp, fn, fp = out_i[..., 0], out_i[..., 1], out_i[..., 2]
            ass, loc = out_f[..., :3], out_f[..., 3]
        tps = np.maximum(1, tp.sum(0))
        w = [(ass[..., k] * tp).sum(0) / tps for k in range(3)]
        out = _hota_fields(tp.sum(0), fn.sum(0), fp.sum(0), loc.sum(0), w[0], w[1], w[2], self.alphas)
        out["sequences"] = [_hota_fields(tp[s], fn[s], fp[s], loc[s], ass[s, :, 0], ass[s, :, 1], ass[s, :, 2], self.alphas) for s in range(S)]
        return out


def hota_extras(record):
    """A Hota.result() record or one of its "sequences" -> TrackEval's remaining HOTA-family fields: OWTA = the mean over alpha of sqrt(DetRe AssA),
    and HOTA(0), LocA(0), HOTALocA(0) = the first threshold's HOTA, LocA and their product."""
    per = record["per_alpha"]
    hota0, loc0 = float(per["HOTA"][0]), float(per["LocA"][0])
    return {"OWTA": float(np.mean(np.sqrt(per["DetRe"] * per["AssA"]))), "HOTA(0)": hota0, "LocA(0)": loc0, "HOTALocA(0)": hota0 * loc0}


CLEAR_ID_COUNTS = ops_track.MOT_FIELDS_I + ("MOTP_sum",)
CLEAR_ID_FIELDS = ("MOTA", "MOTP", "MODA", "sMOTA", "CLR_Re", "CLR_Pr", "IDF1", "IDR", "IDP")


def _clear_id_fields(c):
    """The eleven counts and MOTP_sum of one sequence or of a combination -> the record with the ratios."""
    tp, fn, fp, idsw, motp = c["TP"], c["FN"], c["FP"], c["IDSW"], c["MOTP_sum"]
    idtp, idfn, idfp = c["IDTP"], c["IDFN"], c["IDFP"]
    gt = max(1, tp + fn)
    out = dict(c)
    out.update({"MOTA": (tp - fp - idsw) / gt, "MOTP": motp / max(1, tp), "MODA": (tp - fp) / gt, "sMOTA": (motp - fp - idsw) / gt, "CLR_Re": tp / gt,
                "CLR_Pr": tp / max(1, tp + fp), "IDR": idtp / max(1, idtp + idfn), "IDP": idtp / max(1, idtp + idfp),
                "IDF1": idtp / max(1.0, idtp + 0.5 * idfp + 0.5 * idfn)})
    return out


class ClearIdentity(object):
    """The CLEAR MOT family and the Identity family of whole sequences, batched: Hota's protocol.  update(gt_boxes (G, 4), gt_ids (G,), trk_boxes (T, 4),
    trk_ids (T,)) adds one frame to the current sequence (boxes x1, y1, x2, y2 on the device, read as float32; ids host integers of any value, unique
    within the frame; G, T <= 64), new_sequence() closes it.  result() pads (Hota's padding), makes ONE `ops.mot_sequences` call (csrc/mot_seq.hip, five
    launches) and returns TP, FN, FP, IDSW, MT, PT, ML, Frag, IDTP, IDFN, IDFP, MOTP_sum, MOTA, MOTP, MODA, sMOTA, CLR_Re, CLR_Pr, IDF1, IDR, IDP of the
    combination (every count and MOTP_sum add, the ratios are recomputed) and "sequences": the same record per sequence.
    `ClearMot` remains the online class: one frame at a time, the same CLEAR reading."""

    def __init__(self, threshold=0.5):
        self.threshold = float(threshold)
        self._closed = []
        self._frames = []

    def update(self, gt_boxes, gt_ids, trk_boxes, trk_ids):
        self._frames.append(_checked_frame("ClearIdentity", gt_boxes, gt_ids, trk_boxes, trk_ids))

    def new_sequence(self):
        self._closed.append(self._frames)
        self._frames = []

    def padded(self):
        """The arguments of ops.mot_sequences without thr (Hota.padded's tuple), or None without a sequence."""
        return _pad_sequences(self._closed + ([self._frames] if self._frames else []))

    def result(self):
        args = self.padded()
        seqs = []
        if args is not None:
            out_i, out_f = ops_track.mot_sequences(*args, thr=self.threshold)
            out_i, out_f = out_i.cpu().numpy().astype(np.int64), out_f.cpu().numpy()
            for s in range(out_i.shape[0]):
                c = {k: int(out_i[s, j]) for j, k in enumerate(ops_track.MOT_FIELDS_I)}
                c["MOTP_sum"] = float(out_f[s, 0])
                seqs.append(c)
        total = {k: sum(c[k] for c in seqs) for k in ops_track.MOT_FIELDS_I}
        total["MOTP_sum"] = float(sum(c["MOTP_sum"] for c in seqs))
        out = _clear_id_fields(total)
        out["sequences"] = [_clear_id_fields(c) for c in seqs]
        return out

"""Row f-5: the CLEAR MOT metric (MOTA / MOTP / ID switches) in TrackEval's reading (clear.py).

Per frame: similarity = IoU of the axis-aligned boxes (torch, fp64 on the device), threshold 0.5, score = 1000 [the GT's tracker id of the
PREVIOUS frame == this tracker id] + IoU with the entries below the threshold zeroed, optimal assignment, matched = score > 0.

The assignment runs on `ops.assign_iou` (the tracker's own association kernel).  The +1000 continuity term is handled by taking the
continuity-preferred pairs FIRST, not by scaling (1000 + IoU in fp32 would leave 14 bits of the IoU): a GT has at most one previous tracker id
and a tracker id at most one GT, so the continuity pairs above the threshold form a partial matching by themselves, and because one bonus
outweighs any sum of IoUs (<= 64) every optimum of TrackEval's score contains all of them (replacing the two pairs that block one loses < 2 and
wins > 1000).  They are fixed, their rows and columns zeroed, and the kernel assigns the rest on the thresholded IoUs: the same optimum."""
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

"""Row f-1: the detection metric of a whole split -- mmdet "area" AP per agent and IoU threshold -- in ONE device call.

`DetMap.update` only collects (one map = the detections of one agent in one frame and that frame's ground truth), `result` pads every map to one
shape, uploads once and makes ONE `ops.det_map` call (csrc/det_map.hip, four launches: matching with one "taken" set per threshold, the counts,
the ranking of every group by binary searches over the maps' sorted lists, the AP walk); what comes back is the (agents x thresholds) table.
`utils/postprocess.py::eval_map` -- the Python loop this replaces -- stays the host reference: same matching rule, same tie order, same float64
arithmetic."""
import numpy as np
import torch

from .. import ops_post
from .postprocess import WH_AXES


class DetMap(object):
    """update(det, gt_boxes, group=0) per map: det = dict(boxes (M, 5), scores (M,)) as FaFModule.predict_all returns it (any order: the map is
    sorted stably by descending score, as eval_map does), gt_boxes (G, 5); update_batch(...) takes padded device tensors as v2x_det_postprocess
    leaves them; result() -> dict(ap (n_groups, T) float64, mean_ap (T,), num_gt, num_det, num_tp)."""

    def __init__(self, iou_thrs=(0.5, 0.7), n_groups=1, wh_axis="w_along_heading"):
        self.iou_thrs = tuple(float(t) for t in iou_thrs)
        if not 1 <= len(self.iou_thrs) <= ops_post.DET_MAP_MAX_THR or not all(0.0 < t <= 1.0 for t in self.iou_thrs):
            raise ValueError("DetMap: 1..%d IoU thresholds in (0, 1], got %s" % (ops_post.DET_MAP_MAX_THR, self.iou_thrs))
        self.n_groups = int(n_groups)
        if not 1 <= self.n_groups <= ops_post.DET_MAP_MAX_GROUPS:
            raise ValueError("DetMap: n_groups = %d outside [1, %d]" % (self.n_groups, ops_post.DET_MAP_MAX_GROUPS))
        if wh_axis not in WH_AXES:
            raise ValueError("wh_axis must be one of %s" % (WH_AXES,))
        self._swap = wh_axis == "h_along_heading"      # the kernels' boxes carry w along the heading: exchange the extents of both sides
        self._maps = []          # (boxes (M, 5) fp32, scores (M,) fp32, gt (G, 5) fp32, group)
        self._batches = []       # (det_boxes, det_scores, det_count, gt_boxes, gt_count, group) on the device

    def _group(self, group):
        group = int(group)
        if not (group == -1 or 0 <= group < self.n_groups):
            raise ValueError("DetMap: group %d outside [0, %d) (-1: the map takes no part)" % (group, self.n_groups))
        return group

    def update(self, det, gt_boxes, group=0):
        boxes, scores = det["boxes"], det["scores"]
        if torch.is_tensor(boxes):
            boxes = boxes.detach().cpu().numpy()
        if torch.is_tensor(scores):
            scores = scores.detach().cpu().numpy()
        if torch.is_tensor(gt_boxes):
            gt_boxes = gt_boxes.detach().cpu().numpy()
        boxes = np.asarray(boxes, np.float32).reshape(-1, 5)
        scores = np.asarray(scores, np.float32).reshape(-1)
        gt = np.asarray(gt_boxes, np.float32).reshape(-1, 5)
        if boxes.shape[0] != scores.shape[0]:
            raise ValueError("DetMap.update: %d boxes, %d scores" % (boxes.shape[0], scores.shape[0]))
        if not np.isfinite(scores).all():
            raise ValueError("DetMap.update: a detection score is not finite")
        if boxes.shape[0] > ops_post.DET_MAP_MAX_DET or gt.shape[0] > ops_post.DET_MAP_MAX_GT:
            raise ValueError("DetMap.update: at most %d detections and %d ground truths per map" % (ops_post.DET_MAP_MAX_DET, ops_post.DET_MAP_MAX_GT))
        order = np.argsort(-scores, kind="stable")          # -0.0 and +0.0 tie here as on the device
        boxes, scores = boxes[order], scores[order]
        if self._swap:
            boxes, gt = boxes[:, [0, 1, 3, 2, 4]], gt[:, [0, 1, 3, 2, 4]]
        self._maps.append((boxes, scores, gt, self._group(group)))

    def update_batch(self, det_boxes, det_scores, det_count, gt_boxes, gt_count, group):
        """Padded device tensors, each map in descending score order: det_boxes (n, det_cap, 5), det_scores (n, det_cap), det_count (n,),
        gt_boxes (n, gt_cap, 5), gt_count (n,), group (n,) (or one int for all maps).  They stay on the device.  Raises ValueError on a negative
        count, a non-finite counted score or a map that is not sorted."""
        if not det_boxes.is_cuda:
            raise RuntimeError("DetMap.update_batch takes tensors on the MI355X (cuda) device")
        n = int(det_boxes.shape[0])
        if not torch.is_tensor(group):
            group = torch.full((n,), self._group(group), dtype=torch.int32, device=det_boxes.device)
        det_count, gt_count = det_count.to(torch.int32), gt_count.to(torch.int32)
        live = (group >= 0) & (group < self.n_groups)
        if bool(((det_count < 0) | (gt_count < 0)).any()):
            raise ValueError("DetMap.update_batch: a negative count (v2x_det_postprocess's overflow marker?) -- score that map through update()")
        if bool(((group < -1) | (group >= self.n_groups)).any()):
            raise ValueError("DetMap.update_batch: a group outside [0, %d) (-1: the map takes no part)" % self.n_groups)
        pos = torch.arange(det_boxes.shape[1], device=det_boxes.device)[None, :]
        counted = live[:, None] & (pos < det_count.clamp(max=det_boxes.shape[1])[:, None])
        if not bool(torch.isfinite(det_scores.float()[counted]).all()):
            raise ValueError("DetMap.update_batch: a detection score is not finite")
        sc = det_scores.float()
        if bool((counted[:, 1:] & (sc[:, 1:] > sc[:, :-1])).any()):          # the matching walks in this order and the ranking searches it
            raise ValueError("DetMap.update_batch: a map is not in descending score order (update() sorts; this entry does not)")
        if self._swap:
            det_boxes, gt_boxes = det_boxes[..., [0, 1, 3, 2, 4]], gt_boxes[..., [0, 1, 3, 2, 4]]
        self._batches.append((det_boxes.float(), det_scores.float(), det_count, gt_boxes.float(), gt_count, group.to(torch.int32)))

    def padded(self, device):
        """Everything collected, as one set of padded device tensors (one upload of the host-side maps)."""
        parts = list(self._batches)
        if self._maps:
            n = len(self._maps)
            det_cap = max(1, max(len(m[1]) for m in self._maps))
            gt_cap = max(1, max(len(m[2]) for m in self._maps))
            db, ds = np.zeros((n, det_cap, 5), np.float32), np.zeros((n, det_cap), np.float32)
            gb = np.zeros((n, gt_cap, 5), np.float32)
            dc, gc, gr = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
            for i, (boxes, scores, gt, group) in enumerate(self._maps):
                db[i, :len(scores)], ds[i, :len(scores)], gb[i, :len(gt)] = boxes, scores, gt
                dc[i], gc[i], gr[i] = len(scores), len(gt), group
            parts.append(tuple(torch.from_numpy(a).to(device) for a in (db, ds, dc, gb, gc, gr)))
        if len(parts) == 1:
            return tuple(t.contiguous() for t in parts[0])
        det_cap, gt_cap = max(p[0].shape[1] for p in parts), max(p[3].shape[1] for p in parts)

        def pad(t, cap):
            if t.shape[1] == cap:
                return t
            shape = list(t.shape)
            shape[1] = cap - t.shape[1]
            return torch.cat([t, torch.zeros(shape, dtype=t.dtype, device=t.device)], 1)
        return (torch.cat([pad(p[0], det_cap) for p in parts]).contiguous(), torch.cat([pad(p[1], det_cap) for p in parts]).contiguous(),
                torch.cat([p[2] for p in parts]).contiguous(), torch.cat([pad(p[3], gt_cap) for p in parts]).contiguous(),
                torch.cat([p[4] for p in parts]).contiguous(), torch.cat([p[5] for p in parts]).contiguous())

    def result(self, device=None):
        T = len(self.iou_thrs)
        if not self._maps and not self._batches:
            z = np.zeros((self.n_groups, T))
            return {"ap": z, "mean_ap": z.mean(0), "num_gt": np.zeros(self.n_groups, np.int64), "num_det": np.zeros(self.n_groups, np.int64),
                    "num_tp": np.zeros((self.n_groups, T), np.int64)}
        if device is None:
            device = self._batches[0][0].device if self._batches else torch.device("cuda:0")
        if torch.device(device).type != "cuda":
            raise RuntimeError("DetMap runs on the MI355X (cuda) device; the v2x_sim_amd hot path has no CPU fallback")
        ap, num_gt, num_det, num_tp = ops_post.det_map(*self.padded(device), iou_thrs=self.iou_thrs, n_groups=self.n_groups)
        ap = ap.cpu().numpy()
        return {"ap": ap, "mean_ap": ap.mean(0), "num_gt": num_gt.cpu().numpy(), "num_det": num_det.cpu().numpy(), "num_tp": num_tp.cpu().numpy()}

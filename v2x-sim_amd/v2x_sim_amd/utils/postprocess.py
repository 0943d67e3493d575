"""Detection post-processing and mAP, host-side numpy like the
reference's own Python post-processing.

Mirrors (from recollection -- the files are not in /root/reference; README.md:36 names the
detection task, README.md:101 the benchmark scripts that call them):
  * coperception/utils/postprocess.py::apply_nms_det  -- softmax foreground score, score
    threshold, 'faf' anchor decode, NMS on the axis-aligned "stand-up" boxes of the rotated boxes;
  * coperception/utils/mean_ap.py::eval_map           -- mmdet-style AP (area under the
    monotone precision envelope) with ROTATED-box IoU.  Upstream uses shapely polygons; shapely is
    not available here, so the convex-polygon intersection is a Sutherland-Hodgman clip.

Build-owned spec, frozen here because upstream cannot be consulted:
  box code (x, y, w, h, sin, cos):  x = xa + dx,  y = ya + dy,  w = wa*exp(dw),  h = ha*exp(dh),
  heading = atan2(sa, ca) + atan2(ds, dc);   score = softmax(cls)[..., 1] per anchor;
  keep score >= 0.7 (upstream's test-time threshold), NMS IoU threshold 0.01 on stand-up boxes.
This module never touches the GPU kernels; it consumes the fp32 logits they (or the oracle) emit,
so "mAP parity" = same function applied to both sets of logits.
"""
import math

import numpy as np


def build_anchor_map(config):
    """(X, Y, A, 6) anchors [x, y, w, h, sin, cos] at the BEV cell centres, metres."""
    X, Y = config.map_dims[0], config.map_dims[1]
    vx, vy = config.voxel_size[0], config.voxel_size[1]
    x0, y0 = config.area_extents[0][0], config.area_extents[1][0]
    xs = x0 + (np.arange(X) + 0.5) * vx
    ys = y0 + (np.arange(Y) + 0.5) * vy
    anc = np.zeros((X, Y, len(config.anchor_size), 6), dtype=np.float32)
    anc[..., 0] = xs[:, None, None]
    anc[..., 1] = ys[None, :, None]
    for a, (w, h, yaw) in enumerate(config.anchor_size):
        anc[:, :, a, 2], anc[:, :, a, 3] = w, h
        anc[:, :, a, 4], anc[:, :, a, 5] = math.sin(yaw), math.cos(yaw)
    return anc


def softmax_fg(cls_logits):
    """cls (..., 2) logits -> foreground probability."""
    z = cls_logits - cls_logits.max(axis=-1, keepdims=True)
    e = np.exp(z)
    return e[..., 1] / e.sum(axis=-1)


def decode_boxes(loc, anchors):
    """loc, anchors (..., 6) -> (..., 5) [x, y, w, h, yaw]."""
    x = anchors[..., 0] + loc[..., 0]
    y = anchors[..., 1] + loc[..., 1]
    w = anchors[..., 2] * np.exp(np.clip(loc[..., 2], -4.0, 4.0))
    h = anchors[..., 3] * np.exp(np.clip(loc[..., 3], -4.0, 4.0))
    yaw = np.arctan2(anchors[..., 4], anchors[..., 5]) + np.arctan2(loc[..., 4], loc[..., 5])
    return np.stack([x, y, w, h, yaw], axis=-1)


WH_AXES = ("w_along_heading", "h_along_heading")


def box_corners(boxes, wh_axis="w_along_heading"):
    """(N, 5) [x, y, w, h, yaw] -> (N, 4, 2) corners, counter-clockwise.  wh_axis (oracle/ASSUMPTIONS.md row 48, both readings): which extent
    runs along the box's heading -- "w_along_heading" (default) or "h_along_heading" (the rectangle with the extents exchanged);
    Config.box_wh_axis selects it for FaFModule."""
    x, y, w, h, yaw = (boxes[:, i] for i in range(5))
    if wh_axis == "h_along_heading":
        w, h = h, w
    elif wh_axis != "w_along_heading":
        raise ValueError("wh_axis must be one of %s" % (WH_AXES,))
    c, s = np.cos(yaw), np.sin(yaw)
    dx = np.stack([w / 2, -w / 2, -w / 2, w / 2], 1)
    dy = np.stack([h / 2, h / 2, -h / 2, -h / 2], 1)
    cx = x[:, None] + dx * c[:, None] - dy * s[:, None]
    cy = y[:, None] + dx * s[:, None] + dy * c[:, None]
    return np.stack([cx, cy], -1)


def standup(corners):
    """(N, 4, 2) -> (N, 4) axis-aligned [x1, y1, x2, y2]."""
    return np.concatenate([corners.min(1), corners.max(1)], 1)


def nms_standup(boxes_xyxy, scores, iou_thr=0.01, max_out=None):
    order = np.argsort(-scores, kind="stable")
    x1, y1, x2, y2 = (boxes_xyxy[:, i] for i in range(4))
    area = (x2 - x1) * (y2 - y1)
    keep = []
    while order.size:
        i = order[0]
        keep.append(i)
        if max_out and len(keep) >= max_out:
            break
        rest = order[1:]
        iw = np.maximum(0.0, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]))
        ih = np.maximum(0.0, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]))
        inter = iw * ih
        iou = inter / (area[i] + area[rest] - inter + 1e-12)
        order = rest[iou <= iou_thr]
    return np.asarray(keep, dtype=np.int64)


def apply_nms_det(loc, cls, anchors, score_thr=0.7, nms_thr=0.01, max_out=None, wh_axis="w_along_heading"):
    """One agent.  loc (X, Y, A, 1, 6) or (X, Y, A, 6); cls (X*Y*A, 2); anchors (X, Y, A, 6).
    -> dict(boxes (M, 5), corners (M, 4, 2), scores (M,))."""
    loc = np.asarray(loc, dtype=np.float32).reshape(-1, 6)
    anchors = np.asarray(anchors, dtype=np.float32).reshape(-1, 6)
    score = softmax_fg(np.asarray(cls, dtype=np.float32).reshape(-1, 2))
    sel = np.nonzero(score >= score_thr)[0]
    if sel.size == 0:
        return {"boxes": np.zeros((0, 5), np.float32), "corners": np.zeros((0, 4, 2), np.float32),
                "scores": np.zeros((0,), np.float32)}
    if sel.size > 20000:
        # upstream's greedy NMS is O(kept x candidates): a detector that fires on a large part of the map (an untrained or diverged model)
        # keeps this host path busy for minutes per map -- say so instead of looking hung
        import warnings
        warnings.warn("apply_nms_det: %d of %d anchors pass the score threshold %.2f; the host NMS will take a long time "
                      "(is the model trained?)" % (sel.size, score.size, score_thr), RuntimeWarning, stacklevel=2)
    boxes = decode_boxes(loc[sel], anchors[sel])
    corners = box_corners(boxes, wh_axis)
    keep = nms_standup(standup(corners), score[sel], nms_thr, max_out)
    return {"boxes": boxes[keep], "corners": corners[keep], "scores": score[sel][keep]}


# ------------------------------------------------------------------ late fusion (upstream test_codet.py --com late)
def _late_rigid_fields(T, atan2, stack, zeros_like):
    """THE pose convention of late fusion, written once for numpy and torch: T (..., 4, 4) float64 in the WARP's axis convention (the dataset's
    trans_matrices: T03 = -t_y, T13 = t_x, synthetic_scene.make_scene) -> (..., 8) float64 (r00, r01, tx, r10, r11, ty, dyaw, 0)."""
    return stack([T[..., 0, 0], T[..., 0, 1], T[..., 1, 3], T[..., 1, 0], T[..., 1, 1], -T[..., 0, 3], atan2(T[..., 1, 0], T[..., 0, 0]),
                  zeros_like(T[..., 0, 0])], -1)


def late_rigid_from_trans(trans_matrices):
    """trans_matrices (..., 4, 4), the dataset's (entry [b, i, j] = the pose of agent j w.r.t. ego i) -> (..., 8) fp32 numpy: the box transform
    of v2x_det_late_fuse, derived on the host in float64 and rounded once."""
    T = np.asarray(trans_matrices.detach().cpu().numpy() if hasattr(trans_matrices, "detach") else trans_matrices, dtype=np.float64)
    return _late_rigid_fields(T, np.arctan2, np.stack, np.zeros_like).astype(np.float32)


def late_rigid_from_trans_torch(trans_matrices):
    """The same derivation where a torch tensor lives (FaFModule.predict_all: the matrices are already on the device and no device-to-host copy
    is to be added): float64, rounded once, -> (..., 8) fp32 tensor on that device.  Seven of the eight fields are copies or a negation; dyaw is
    torch.atan2 in float64, which tests/test_late_refs_cpu.py (CPU tensors) and tests/test_gpu_late_fuse.py (the device) hold bit-equal to
    late_rigid_from_trans after the rounding to fp32 on their seeded poses ("late fusion")."""
    import torch
    return _late_rigid_fields(trans_matrices.to(torch.float64), torch.atan2, torch.stack, torch.zeros_like).to(torch.float32)


def late_transform(boxes, rigid8):
    """(N, 5) fp32 boxes of a neighbour, (8,) fp32 rigid -> (N, 5) fp32 in the ego's frame: numpy's separate float32 operations, which are the
    kernel's (__fmul_rn / __fadd_rn), bit for bit."""
    b = np.asarray(boxes, np.float32).reshape(-1, 5)
    r = np.asarray(rigid8, np.float32)
    out = b.copy()
    out[:, 0] = (r[0] * b[:, 0] + r[1] * b[:, 1]) + r[2]
    out[:, 1] = (r[3] * b[:, 0] + r[4] * b[:, 1]) + r[5]
    out[:, 4] = b[:, 4] + r[6]
    return out


def late_candidates(boxes_of, scores_of, ego, rigid_row, link_row, extents):
    """The merged candidate list of one ego, ungathered order: boxes_of[j] (N_j, 5), scores_of[j] (N_j,) fp32 per agent (None: no list),
    rigid_row (A, 8), link_row (A,) -> boxes (N, 5) fp32, scores (N,) fp32, agent (N,), rank (N,).  The ego's own enter as they are; a neighbour's
    are transformed and cropped to x_lo <= x' < x_hi, y_lo <= y' < y_hi; non-finite fields and scores not >= 0 drop a candidate."""
    (x_lo, x_hi), (y_lo, y_hi) = (np.float32(v) for v in extents[0]), (np.float32(v) for v in extents[1])
    bs, ss, ag, rk = [np.zeros((0, 5), np.float32)], [np.zeros((0,), np.float32)], [np.zeros((0,), np.int64)], [np.zeros((0,), np.int64)]
    for j in range(len(link_row)):
        if boxes_of[j] is None or (j != ego and not link_row[j]):
            continue
        src = np.asarray(boxes_of[j], np.float32).reshape(-1, 5)
        sc = np.asarray(scores_of[j], np.float32).reshape(-1)
        with np.errstate(all="ignore"):
            b = src.copy() if j == ego else late_transform(src, rigid_row[j])
            ok = np.isfinite(src).all(1) & np.isfinite(b).all(1) & np.isfinite(sc) & (sc >= 0)
            if j != ego:
                ok &= (b[:, 0] >= x_lo) & (b[:, 0] < x_hi) & (b[:, 1] >= y_lo) & (b[:, 1] < y_hi)
        w = np.nonzero(ok)[0]
        bs.append(b[w]), ss.append(sc[w]), ag.append(np.full(w.shape, j, np.int64)), rk.append(w)
    return np.concatenate(bs), np.concatenate(ss), np.concatenate(ag), np.concatenate(rk)


def late_order(scores, agent, rank, ego):
    """Score descending; ties: the ego's own boxes, then neighbours by ascending agent index, then ascending rank in the source list."""
    return np.lexsort((rank, np.where(agent == ego, -1, agent), -np.asarray(scores, np.float64)))


def late_fusion(seq_dets, trans_matrices, num_agent, extents, link=None, nms_thr=0.01, wh_axis="w_along_heading"):
    """The numpy mirror of v2x_det_late_fuse on FaFModule.predict_all's per-agent results: seq_dets[k][b] = dict(boxes, scores, ...) or None,
    trans_matrices (B, A, A, 4, 4), link (B, A, A) or None (everybody hears everybody) -> the same nest with, per present ego, dict(boxes,
    corners, scores, src_agent): its own detections and its linked neighbours' in its frame, cropped to `extents`, after one more stand-up NMS
    in fp32 (nms_standup: what the kernel mirrors).  Agents whose slot is None are absent: they send nothing and get None."""
    A = num_agent
    Bn = len(seq_dets[0]) if A else 0
    rigid = late_rigid_from_trans(trans_matrices)
    swap = wh_axis == "h_along_heading"            # the kernels' boxes carry w along the heading: exchange, fuse, exchange back
    out = [[None] * Bn for _ in range(A)]
    for b in range(Bn):
        boxes_of = [None if seq_dets[j][b] is None else np.asarray(seq_dets[j][b]["boxes"], np.float32).reshape(-1, 5)[:, [0, 1, 3, 2, 4] if swap else slice(None)]
                    for j in range(A)]
        scores_of = [None if seq_dets[j][b] is None else seq_dets[j][b]["scores"] for j in range(A)]
        for i in range(A):
            if boxes_of[i] is None or (link is not None and not link[b][i][i]):
                continue
            row = np.ones(A, bool) if link is None else np.asarray(link[b][i]).astype(bool)
            bx, sc, ag, rk = late_candidates(boxes_of, scores_of, i, rigid[b, i], row, extents)
            order = late_order(sc, ag, rk, i)
            bx, sc, ag = bx[order], sc[order], ag[order]
            keep = nms_standup(standup(box_corners(bx)), -np.arange(len(sc), dtype=np.float64), nms_thr) if len(sc) else np.zeros(0, np.int64)
            kb = bx[keep][:, [0, 1, 3, 2, 4]] if swap else bx[keep]
            out[i][b] = {"boxes": kb, "corners": box_corners(kb, wh_axis) if len(keep) else np.zeros((0, 4, 2), np.float32), "scores": sc[keep],
                         "src_agent": ag[keep]}
    return out


# ------------------------------------------------------------------ rotated IoU + AP
def _poly_area(p):
    x, y = p[:, 0], p[:, 1]
    return 0.5 * abs(float(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))))


def _clip(subject, a, b):
    """Sutherland-Hodgman: keep the part of `subject` left of the directed edge a->b."""
    out = []
    n = len(subject)
    for i in range(n):
        p, q = subject[i], subject[(i + 1) % n]
        sp = (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
        sq = (b[0] - a[0]) * (q[1] - a[1]) - (b[1] - a[1]) * (q[0] - a[0])
        if sp >= 0:
            out.append(p)
        if (sp >= 0) != (sq >= 0):
            t = sp / (sp - sq)
            out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def rotated_iou(c1, c2):
    """IoU of two convex quadrilaterals given as (4, 2) counter-clockwise corners."""
    poly = [tuple(p) for p in c1]
    for i in range(4):
        if not poly:
            return 0.0
        poly = _clip(poly, tuple(c2[i]), tuple(c2[(i + 1) % 4]))
    if len(poly) < 3:
        return 0.0
    inter = _poly_area(np.asarray(poly))
    union = _poly_area(np.asarray(c1)) + _poly_area(np.asarray(c2)) - inter
    return inter / union if union > 0 else 0.0


def eval_map(det_results, annotations, iou_thr=0.5):
    """Single-class mmdet-style AP.

    det_results: list (one per sample) of dict(corners (M,4,2), scores (M,));
    annotations: list of (G, 4, 2) ground-truth corner arrays.
    Returns (ap, dict(recall, precision, num_gt, num_det))."""
    scores, tps = [], []
    num_gt = 0
    for det, gt in zip(det_results, annotations):
        gt = np.asarray(gt, dtype=np.float64).reshape(-1, 4, 2)
        num_gt += gt.shape[0]
        order = np.argsort(-det["scores"], kind="stable")
        taken = np.zeros(gt.shape[0], dtype=bool)
        gt_box = standup(gt) if gt.shape[0] else None
        for j in order:
            c = np.asarray(det["corners"][j], dtype=np.float64)
            best, best_g = 0.0, -1
            if gt.shape[0]:
                bb = np.concatenate([c.min(0), c.max(0)])
                cand = np.nonzero((gt_box[:, 0] <= bb[2]) & (gt_box[:, 2] >= bb[0]) &
                                  (gt_box[:, 1] <= bb[3]) & (gt_box[:, 3] >= bb[1]))[0]
                for g in cand:
                    v = rotated_iou(c, gt[g])
                    if v > best:
                        best, best_g = v, g
            scores.append(det["scores"][j])
            if best >= iou_thr and not taken[best_g]:
                taken[best_g] = True
                tps.append(1)
            else:
                tps.append(0)
    return average_precision(scores, tps, num_gt)


def average_precision(scores, tps, num_gt):
    """mmdet 'area' AP from per-detection (score, true-positive flag) pairs of ALL images (image-major, per image in descending
    score order) and the number of ground-truth boxes.  -> (ap, info) like eval_map."""
    scores, tps = np.asarray(scores, dtype=np.float64).reshape(-1), np.asarray(tps).reshape(-1).astype(np.int64)
    if num_gt == 0 or scores.size == 0:
        return 0.0, {"recall": np.zeros(0), "precision": np.zeros(0), "num_gt": num_gt, "num_det": int(scores.size)}
    order = np.argsort(-scores, kind="stable")
    tp = np.cumsum(tps[order])
    fp = np.cumsum(1 - tps[order])
    recall = tp / num_gt
    precision = tp / np.maximum(tp + fp, 1e-12)
    mrec = np.concatenate([[0.0], recall, [1.0]])
    mpre = np.concatenate([[0.0], precision, [0.0]])
    for i in range(mpre.size - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    idx = np.nonzero(mrec[1:] != mrec[:-1])[0]
    ap = float(np.sum((mrec[idx + 1] - mrec[idx]) * mpre[idx + 1]))
    return ap, {"recall": recall, "precision": precision, "num_gt": num_gt, "num_det": int(scores.size)}


def eval_map_device(det_boxes, det_scores, det_count, gt_boxes_list, iou_thr=0.5):
    """eval_map with the IoU + matching step on the MI355X (v2x_match_detections): det_boxes (n, cap, 5), det_scores (n, cap),
    det_count (n,) as v2x_det_postprocess leaves them ON THE DEVICE (descending score per map), gt_boxes_list = per image a
    (G, 5) host array.  Only (score, tp) pairs come back to the host for the final sort + cumulative sums."""
    import torch
    from .. import ops
    n = det_boxes.shape[0]
    gt_cap = max(1, max((len(g) for g in gt_boxes_list), default=1))
    gt = np.zeros((n, gt_cap, 5), np.float32)
    gcount = np.zeros((n,), np.int32)
    for i, g in enumerate(gt_boxes_list):
        g = np.asarray(g, np.float32).reshape(-1, 5)
        gt[i, :g.shape[0]] = g
        gcount[i] = g.shape[0]
    dev = det_boxes.device
    if bool((det_count < 0).any()):
        # v2x_det_postprocess's overflow signal (more than `cap` candidates): clamping would score that map with ZERO detections while its
        # ground truth still counts.  The caller re-runs such maps through the host path (FaFModule.postprocess does) before scoring.
        bad = torch.nonzero(det_count < 0).flatten().tolist()
        raise ValueError("eval_map_device: maps %s overflowed the device candidate capacity (count < 0); run them through "
                         "apply_nms_det and pass their detections in, or raise the capacity" % bad[:8])
    cnt = det_count.to(torch.int32).contiguous()
    tp = ops.match_detections(det_boxes.contiguous(), cnt, torch.from_numpy(gt).to(dev), torch.from_numpy(gcount).to(dev), iou_thr)
    cnt_h, tp_h, sc_h = cnt.cpu().numpy(), tp.cpu().numpy(), det_scores.cpu().numpy()
    scores = np.concatenate([sc_h[i, :cnt_h[i]] for i in range(n)]) if n else np.zeros(0)
    tps = np.concatenate([tp_h[i, :cnt_h[i]] for i in range(n)]) if n else np.zeros(0, np.int64)
    return average_precision(scores, tps, int(gcount.sum()))

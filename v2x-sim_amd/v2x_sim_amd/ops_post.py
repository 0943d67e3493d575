"""Row f-1 (post-processing and metric): python wrappers over v2x_det_postprocess[_rotated], the fused candidate heads + v2x_det_nms_candidates,
v2x_det_late_fuse, v2x_rotated_iou and v2x_match_detections; and the IoU anchor assignment of row f-3 (v2x_det_assign_targets), which shares their box geometry.  Re-exported by ops.py (`ops.det_postprocess` ...)."""
import ctypes as C

import numpy as np
import torch

from . import _launch, _lib
from ._launch import _Prof, _dev, _stream  # noqa: F401
from ._lib import ConvDesc, V2X_EPI_DET


def det_postprocess(cls, loc, anchors, score_thr=0.7, nms_thr=0.01, cap=4096, rotated=False):
    """cls (n, M, 2) fp32, loc (n, ..., 6) fp32 with M anchors per map, anchors (M, 6) fp32 on the device ->
    (boxes (n, cap, 5), scores (n, cap), index (n, cap) int32, count (n,) int32); count < 0: more than `cap` candidates.
    rotated=True: suppression on the rotated boxes' polygon IoU instead of upstream's stand-up boxes."""
    lib = _lib.load()
    n, M = cls.shape[0], cls.shape[1]
    loc = loc.reshape(n, M, 6)
    anchors = anchors.reshape(M, 6)
    dev = cls.device
    boxes = torch.empty((n, cap, 5), dtype=torch.float32, device=dev)
    scores = torch.empty((n, cap), dtype=torch.float32, device=dev)
    index = torch.empty((n, cap), dtype=torch.int32, device=dev)
    count = torch.empty((n,), dtype=torch.int32, device=dev)
    keys = torch.empty((n, cap), dtype=torch.int64, device=dev)
    cnt = torch.empty((n,), dtype=torch.int32, device=dev)
    fn = lib.v2x_det_postprocess_rotated if rotated else lib.v2x_det_postprocess
    _lib.check(fn(_dev(cls, torch.float32, "cls"), _dev(loc, torch.float32, "loc"),
                                       _dev(anchors, torch.float32, "anchors"), n, M, C.c_float(score_thr),
                                       C.c_float(nms_thr), cap, _dev(boxes, torch.float32, "boxes"),
                                       _dev(scores, torch.float32, "scores"), _dev(index, torch.int32, "index"),
                                       _dev(count, torch.int32, "count"), _dev(keys, torch.int64, "keys"),
                                       _dev(cnt, torch.int32, "cnt"), _stream()), "v2x_det_postprocess")
    return boxes, scores, index, count


def conv2d_det(pc, x, score_thr, cap=4096):
    """The fused detection heads (packing.pack_heads_det; conv_halo.hip V2X_EPI_DET) on the decoder's output x (N, H, W, 32) bf16:
    softmax(cls)[1] >= score_thr is evaluated in the epilogue, only the candidates leave the kernel.
    -> keys (N, cap) int64, codes (N, cap, 6) fp32, counts (N,) int32 (the true count even when > cap) for det_nms_candidates."""
    lib = _lib.load()
    N, H, W, Cx = x.shape
    if Cx != pc.C0 or pc.epilogue != _lib.V2X_EPI_DET:
        raise ValueError("conv2d_det needs the det-heads packing and a %d-channel input" % pc.C0)
    keys = torch.empty((N, cap), dtype=torch.int64, device=x.device)
    codes = torch.empty((N, cap, 6), dtype=torch.float32, device=x.device)
    counts = torch.zeros((N,), dtype=torch.int32, device=x.device)
    d = ConvDesc()
    d.in0, d.in1 = _dev(x, torch.bfloat16, "x").value, None
    d.C0, d.C1, d.up0 = pc.C0, 0, 0
    d.N, d.H, d.W = N, H, W
    d.ksize, d.stride, d.pad = 3, 1, 1
    d.Cout, d.w_rows, d.w_kpad = pc.Cout, pc.w_rows, pc.w_kpad
    d.weight, d.scale, d.shift = pc.weight.data_ptr(), pc.scale.data_ptr(), pc.shift.data_ptr()
    d.epilogue, d.relu = _lib.V2X_EPI_DET, int(bool(pc.relu))
    d.out, d.out_cstride, d.out_coff = keys.data_ptr(), cap, 0
    d.out2, d.split, d.out2_cstride = codes.data_ptr(), 0, 6
    d.w_layout = 1
    d.Cout2, d.relu2 = pc.Cout2, 0
    d.weight2, d.scale2, d.shift2 = pc.weight2.data_ptr(), pc.scale2.data_ptr(), pc.shift2.data_ptr()
    d.det_counts, d.det_thr, d.det_cap = counts.data_ptr(), float(score_thr), cap
    prof = None
    if _launch.PROFILE is not None:
        M = N * H * W
        prof = _Prof(_lib.conv_plan(d, "v2x_conv2d_plan(%s, det)" % pc.name), 2.0 * M * (64 * 9 * 32 + 48 * 64), x.numel() * 2 + pc.weight.numel() * 2, pc.name)
    rc = lib.v2x_conv2d(C.byref(d), _stream())
    if prof is not None:
        prof.done()
    _lib.check(rc, "v2x_conv2d(%s, det)" % pc.name)
    return keys, codes, counts


def det_nms_candidates(keys, codes, counts, anchors, nms_thr=0.01, rotated=False):
    """Second half of det_postprocess for the candidates conv2d_det selected: sort, 'faf' decode, greedy NMS.
    -> (boxes (n, cap, 5), scores (n, cap), index (n, cap) int32, count (n,) int32), identical to det_postprocess on the logits."""
    lib = _lib.load()
    n, cap = keys.shape
    anchors = anchors.reshape(-1, 6)
    M = anchors.shape[0]
    dev = keys.device
    boxes = torch.empty((n, cap, 5), dtype=torch.float32, device=dev)
    scores = torch.empty((n, cap), dtype=torch.float32, device=dev)
    index = torch.empty((n, cap), dtype=torch.int32, device=dev)
    count = torch.empty((n,), dtype=torch.int32, device=dev)
    _lib.check(lib.v2x_det_nms_candidates(_dev(keys, torch.int64, "keys"), _dev(codes, torch.float32, "codes"), _dev(counts, torch.int32, "counts"),
                                          _dev(anchors, torch.float32, "anchors"), n, M, cap, C.c_float(nms_thr), int(bool(rotated)),
                                          _dev(boxes, torch.float32, "boxes"), _dev(scores, torch.float32, "scores"),
                                          _dev(index, torch.int32, "index"), _dev(count, torch.int32, "count"), _stream()),
               "v2x_det_nms_candidates")
    return boxes, scores, index, count


def late_fuse(boxes, scores, counts, rigid, link, extents, nms_thr=0.01, rotated=False, cap_out=None):
    """Late fusion in one call (v2x_det_late_fuse): boxes (A*B, cap_in, 5), scores (A*B, cap_in), counts (A*B,) as det_postprocess / det_nms_candidates
    leave them on the device (rows agent-major), rigid (B, A, A, 8) fp32 (utils/postprocess.late_rigid_from_trans), link (B, A, A) uint8 or bool,
    extents ((x_lo, x_hi), (y_lo, y_hi), ...) -> (boxes (A*B, cap_out, 5), scores (A*B, cap_out), src (A*B, cap_out) int32 = j*cap_in + rank,
    count (A*B,) int32; negative: not computed, see include/v2x_amd.h)."""
    lib = _lib.load()
    B, A = link.shape[0], link.shape[1]
    n, cap_in = scores.shape
    if n != A * B or tuple(rigid.shape) != (B, A, A, 8) or tuple(link.shape) != (B, A, A) or tuple(boxes.shape) != (n, cap_in, 5) or counts.numel() != n:
        raise ValueError("late_fuse: boxes %s, scores %s, counts %s do not match rigid %s / link %s" % (tuple(boxes.shape), tuple(scores.shape),
                                                                                                 tuple(counts.shape), tuple(rigid.shape), tuple(link.shape)))
    cap_out = cap_in if cap_out is None else int(cap_out)
    dev = boxes.device
    if link.dtype == torch.bool:
        link = link.to(torch.uint8)
    out_boxes = torch.empty((n, cap_out, 5), dtype=torch.float32, device=dev)
    out_scores = torch.empty((n, cap_out), dtype=torch.float32, device=dev)
    out_src = torch.empty((n, cap_out), dtype=torch.int32, device=dev)
    out_count = torch.empty((n,), dtype=torch.int32, device=dev)
    (x_lo, x_hi), (y_lo, y_hi) = extents[0], extents[1]
    _lib.check(lib.v2x_det_late_fuse(_dev(boxes, torch.float32, "boxes") if n else None, _dev(scores, torch.float32, "scores") if n else None,
                                     _dev(counts, torch.int32, "counts") if n else None, A, B, cap_in,
                                     _dev(rigid, torch.float32, "rigid") if n else None, _dev(link, torch.uint8, "link") if n else None,
                                     C.c_float(x_lo), C.c_float(x_hi), C.c_float(y_lo), C.c_float(y_hi), C.c_float(nms_thr), int(bool(rotated)), cap_out,
                                     _dev(out_boxes, torch.float32, "out_boxes") if n else None, _dev(out_scores, torch.float32, "out_scores") if n else None,
                                     _dev(out_src, torch.int32, "out_src") if n else None, _dev(out_count, torch.int32, "out_count") if n else None,
                                     _stream()), "v2x_det_late_fuse")
    return out_boxes, out_scores, out_src, out_count


ASSIGN_OUTPUTS = {"labels": (torch.float32, (2,)), "reg_targets": (torch.float32, (1, 6)), "reg_loss_mask": (torch.uint8, (1,)),
                  "assoc": (torch.int32, ()), "anchor_iou": (torch.float32, ())}


def assign_targets(gt_boxes, gt_count, anchors, pos_thr=0.6, neg_thr=0.45, force_match=True, want=("assoc", "anchor_iou"), out=None):
    """Detection training targets by rotated IoU (v2x_det_assign_targets; the rule: DESIGN.md section 3.7 "IoU assignment").
    gt_boxes (n, gt_cap, 5) fp32 (x, y, w, h, yaw), gt_count (n,) int32, anchors (X, Y, A, 6) fp32, all on the device ->
    dict: labels (n, X, Y, A, 2) fp32, reg_targets (n, X, Y, A, 1, 6) fp32, reg_loss_mask (n, X, Y, A, 1) uint8 (what FaFModule.step reads),
    gt_max_iou (n, gt_cap) fp32, gt_best (n, gt_cap) int32, and the optional outputs named in `want`: assoc (n, X, Y, A) int32, anchor_iou
    (n, X, Y, A) fp32.  out: a dict of existing tensors to write into (any subset of the keys; e.g. the static buffers a captured step reads);
    an optional output present in `out` is written too.  Every element of every output is written."""
    lib = _lib.load()
    n, gt_cap = int(gt_boxes.shape[0]), int(gt_boxes.shape[1])
    X, Y, A = (int(v) for v in anchors.shape[:3])
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] != 5 or gt_count.numel() != n or tuple(anchors.shape) != (X, Y, A, 6):
        raise ValueError("assign_targets: gt_boxes %s, gt_count %s, anchors %s" % (tuple(gt_boxes.shape), tuple(gt_count.shape), tuple(anchors.shape)))
    unknown = (set(want) - {"assoc", "anchor_iou"}) | (set(out or ()) - set(ASSIGN_OUTPUTS) - {"gt_max_iou", "gt_best"})
    if unknown:
        raise ValueError("assign_targets: unknown output %s" % sorted(unknown))
    dev = gt_boxes.device
    res = dict(out) if out is not None else {}

    def buf(name, dtype, shape):
        t = res.get(name)
        if t is None:
            t = res[name] = torch.empty(shape, dtype=dtype, device=dev)
        elif tuple(t.shape) != tuple(shape) or (t.dtype != dtype and not (dtype == torch.uint8 and t.dtype == torch.bool)):
            raise ValueError("assign_targets: out[%r] is %s %s, needs %s %s" % (name, t.dtype, tuple(t.shape), dtype, tuple(shape)))
        return t.view(torch.uint8) if t.dtype == torch.bool else t

    ptr = {}
    for name, (dtype, tail) in ASSIGN_OUTPUTS.items():
        if name in ("assoc", "anchor_iou") and name not in want and name not in res:
            ptr[name] = None
            continue
        t = buf(name, dtype, (n, X, Y, A) + tail)
        ptr[name] = _dev(t, dtype, name) if n else None
    gmax = buf("gt_max_iou", torch.float32, (n, gt_cap))
    gbest = buf("gt_best", torch.int32, (n, gt_cap))
    nbytes = lib.v2x_det_assign_workspace_size(n, X, Y, A, gt_cap)
    if nbytes < 0:
        raise ValueError("assign_targets: sizes out of range (n=%d, X=%d, Y=%d, A=%d, gt_cap=%d; gt_cap <= 256)" % (n, X, Y, A, gt_cap))
    ws = torch.empty((max(nbytes, 8) // 8,), dtype=torch.int64, device=dev)
    _lib.check(lib.v2x_det_assign_targets(_dev(gt_boxes, torch.float32, "gt_boxes") if n else None, _dev(gt_count, torch.int32, "gt_count") if n else None,
                                          n, gt_cap, _dev(anchors, torch.float32, "anchors"), X, Y, A, C.c_float(pos_thr), C.c_float(neg_thr),
                                          int(bool(force_match)), ptr["labels"], ptr["reg_targets"], ptr["reg_loss_mask"], ptr["assoc"], ptr["anchor_iou"],
                                          _dev(gmax, torch.float32, "gt_max_iou") if n else None, _dev(gbest, torch.int32, "gt_best") if n else None,
                                          _dev(ws, torch.int64, "workspace"), nbytes, _stream()), "v2x_det_assign_targets")
    return res


def assign_targets_sparse_keys(res, item=0):
    """One item of assign_targets' result -> the sparse training keys an upstream-produced 0.npy carries (datasets/V2XSimDet.UPSTREAM_TARGET_KEYS
    + gt_max_iou), as host arrays: allocation_mask (X, Y, A) bool = the positive anchors, label_sparse (n_alloc,) int64 = 1, reg_target_sparse
    (n_alloc, 1, 6) fp32, reg_loss_mask (X, Y, A, 1) bool, gt_max_iou (gt_cap,) fp32.  datasets.V2XSimDet.upstream_dense_targets turns them back
    into the dense fields.  The format has no ignore state: an ignored anchor (label (0, 0)) reads back as background."""
    labels = res["labels"][item].cpu().numpy()
    reg = res["reg_targets"][item].cpu().numpy()
    mask = res["reg_loss_mask"][item].cpu().numpy().astype(bool)
    alloc = labels[..., 1] > 0
    return {"allocation_mask": alloc, "label_sparse": np.ones((int(alloc.sum()),), np.int64), "reg_target_sparse": reg[alloc],
            "reg_loss_mask": mask, "gt_max_iou": res["gt_max_iou"][item].cpu().numpy()}


def rotated_iou(boxes_a, boxes_b):
    """boxes (na, 5), (nb, 5) fp32 (x, y, w, h, yaw) on the device -> (na, nb) fp32 IoU of the rotated rectangles."""
    lib = _lib.load()
    na, nb = boxes_a.shape[0], boxes_b.shape[0]
    out = torch.zeros((na, nb), dtype=torch.float32, device=boxes_a.device)
    if na and nb:
        _lib.check(lib.v2x_rotated_iou(_dev(boxes_a, torch.float32, "boxes_a"), na, _dev(boxes_b, torch.float32, "boxes_b"), nb,
                                       _dev(out, torch.float32, "iou"), _stream()), "v2x_rotated_iou")
    return out


def match_detections(det_boxes, det_count, gt_boxes, gt_count, iou_thr, want_iou=False):
    """eval_map's matching on the device.  det_boxes (n, det_cap, 5) fp32 in descending-score order, det_count (n,) int32,
    gt_boxes (n, gt_cap, 5) fp32, gt_count (n,) int32 -> tp (n, det_cap) int32 [, best_iou (n, det_cap) fp32]."""
    lib = _lib.load()
    n, det_cap, _ = det_boxes.shape
    gt_cap = gt_boxes.shape[1]
    tp = torch.zeros((n, det_cap), dtype=torch.int32, device=det_boxes.device)
    best = torch.zeros((n, det_cap), dtype=torch.float32, device=det_boxes.device) if want_iou else None
    _lib.check(lib.v2x_match_detections(_dev(det_boxes, torch.float32, "det_boxes"), _dev(det_count, torch.int32, "det_count"), det_cap,
                                        _dev(gt_boxes, torch.float32, "gt_boxes"), _dev(gt_count, torch.int32, "gt_count"), gt_cap, n,
                                        C.c_float(iou_thr), _dev(tp, torch.int32, "tp"),
                                        _dev(best, torch.float32, "best_iou") if best is not None else None, _stream()),
               "v2x_match_detections")
    return (tp, best) if want_iou else tp


DET_MAP_MAX_THR, DET_MAP_MAX_GROUPS, DET_MAP_MAX_DET, DET_MAP_MAX_GT = 8, 64, 4096, 8192      # csrc/det_map.hip


def det_map(det_boxes, det_scores, det_count, gt_boxes, gt_count, group, iou_thrs=(0.5, 0.7), n_groups=1, want_flags=False):
    """The AP table of a whole split in ONE v2x_det_map call (csrc/det_map.hip).  det_boxes (n, det_cap, 5) fp32, each map
    in descending score order, det_scores (n, det_cap) fp32 (finite), det_count (n,) int32, gt_boxes (n, gt_cap, 5) fp32, gt_count (n,) int32,
    group (n,) int32 (the agent of each map in [0, n_groups); -1: the map takes no part), all on the device; iou_thrs: 1..8 floats in (0, 1] (or a
    device fp32 tensor) -> ap (n_groups, T) float64, num_gt (n_groups,) int64, num_det (n_groups,) int64, num_tp (n_groups, T) int64
    [, tp (T, n, det_cap) uint8, rank (n, det_cap) int32] on the device."""
    lib = _lib.load()
    n, det_cap = int(det_boxes.shape[0]), int(det_boxes.shape[1])
    gt_cap = int(gt_boxes.shape[1])
    dev = det_boxes.device
    if torch.is_tensor(iou_thrs):
        thr = iou_thrs.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        vals = thr.cpu().tolist()             # at most eight floats: the C entry cannot read device values, so the range is checked here
    else:
        vals = [float(v) for v in iou_thrs]
        thr = None
    if not all(0.0 < v <= 1.0 for v in vals):
        raise ValueError("det_map: every IoU threshold must lie in (0, 1], got %s" % (vals,))
    if thr is None:
        thr = torch.tensor(vals, dtype=torch.float32, device=dev)
    T, n_groups = int(thr.numel()), int(n_groups)
    if not (1 <= T <= DET_MAP_MAX_THR and 1 <= n_groups <= DET_MAP_MAX_GROUPS):
        raise ValueError("det_map: %d thresholds (1..%d), %d groups (1..%d)" % (T, DET_MAP_MAX_THR, n_groups, DET_MAP_MAX_GROUPS))
    if det_scores.shape != (n, det_cap) or det_count.shape != (n,) or gt_count.shape != (n,) or group.shape != (n,) or gt_boxes.shape[0] != n:
        raise ValueError("det_map: det_scores (n, det_cap), det_count, gt_count, group (n,) and gt_boxes (n, gt_cap, 5) must agree with det_boxes")
    ap = torch.zeros((n_groups, T), dtype=torch.float64, device=dev)
    num_gt = torch.zeros((n_groups,), dtype=torch.int64, device=dev)
    num_det = torch.zeros((n_groups,), dtype=torch.int64, device=dev)
    num_tp = torch.zeros((n_groups, T), dtype=torch.int64, device=dev)
    tp = torch.zeros((T, n, det_cap), dtype=torch.uint8, device=dev) if want_flags else None
    rank = torch.full((n, det_cap), -1, dtype=torch.int32, device=dev) if want_flags else None
    if n:
        nbytes = lib.v2x_det_map_workspace_size(n, det_cap, gt_cap, n_groups, T)
        if nbytes < 0:
            raise ValueError("det_map: sizes out of range (det_cap %d in [1, 4096], gt_cap %d in [1, 8192], n * det_cap < 2^31)" % (det_cap, gt_cap))
        ws = torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=dev)
        _lib.check(lib.v2x_det_map(_dev(det_boxes, torch.float32, "det_boxes"), _dev(det_scores, torch.float32, "det_scores"),
                                   _dev(det_count, torch.int32, "det_count"), det_cap, _dev(gt_boxes, torch.float32, "gt_boxes"),
                                   _dev(gt_count, torch.int32, "gt_count"), gt_cap, _dev(group, torch.int32, "group"), n, n_groups,
                                   _dev(thr, torch.float32, "iou_thr"), T, _dev(ap, torch.float64, "ap"), _dev(num_gt, torch.int64, "num_gt"),
                                   _dev(num_det, torch.int64, "num_det"), _dev(num_tp, torch.int64, "num_tp"),
                                   _dev(tp, torch.uint8, "tp") if want_flags else None, _dev(rank, torch.int32, "rank") if want_flags else None,
                                   _dev(ws, torch.uint8, "workspace"), int(nbytes), _stream()), "v2x_det_map")
    return (ap, num_gt, num_det, num_tp, tp, rank) if want_flags else (ap, num_gt, num_det, num_tp)

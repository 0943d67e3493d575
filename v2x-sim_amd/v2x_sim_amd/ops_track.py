"""Row f-5 (tracking): python wrappers over v2x_assign_iou and v2x_sort_step (csrc/track.hip) v2x_hota_sequences (csrc/hota.hip) and v2x_mot_sequences (csrc/mot_seq.hip).
Re-exported by ops.py (`ops.sort_step` ...)."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._launch import _dev, _stream

TRACK_CAP = 64      # tracks per stream, detections read per map, rows / columns of a matrix: one wave
HOTA_MAX_ALPHA = 32
MOT_MAX_IDS = 2048  # ids per side of one sequence in mot_sequences: the assignment over the id space sits in one workgroup's LDS
MOT_FIELDS_I = ("TP", "FN", "FP", "IDSW", "MT", "PT", "ML", "Frag", "IDTP", "IDFN", "IDFP")
HOTA_ALPHAS = np.arange(0.05, 0.99, 0.05)      # TrackEval's 19 thresholds, numpy's exact float64 values


def assign_iou(iou, n_rows, n_cols, thr=0.3, direct=True):
    """iou (n, cap_r, cap_c) fp32, n_rows / n_cols (n,) int32 on the device, cap_r, cap_c <= 64 -> row_to_col (n, cap_r) int32 (-1: unmatched).
    direct: abewley's shortcut (at most one entry > thr per row and column -> those entries) before the optimal assignment."""
    lib = _lib.load()
    n, cap_r, cap_c = iou.shape
    out = torch.empty((n, cap_r), dtype=torch.int32, device=iou.device)
    _lib.check(lib.v2x_assign_iou(_dev(iou, torch.float32, "iou"), _dev(n_rows, torch.int32, "n_rows"), _dev(n_cols, torch.int32, "n_cols"), n, cap_r, cap_c,
                                  C.c_float(thr), int(bool(direct)), _dev(out, torch.int32, "row_to_col"), _stream()), "v2x_assign_iou")
    return out


def sort_step(det_boxes, det_count, trk_f, trk_i, stream_i, out=None, box_format=0, iou_thr=0.3, max_age=1, min_hits=3, direct=True):
    """One SORT frame for all n streams in one launch; the state tensors are updated in place.
    det_boxes (n, det_cap, 4) xyxy [box_format 0] or (n, det_cap, 5) x, y, w, h, yaw [1: w along the heading, 2: h], det_count (n,) int32;
    trk_f (n, t_cap, 17) fp32, trk_i (n, t_cap, 5) int32, stream_i (n, 4) int32 (include/v2x_amd.h; all-zero = empty).
    out: (boxes (n, t_cap, 4) fp32, ids (n, t_cap) int32, det (n, t_cap) int32, count (n,) int32) to write into, or None to allocate.
    -> out."""
    lib = _lib.load()
    n, det_cap, width = det_boxes.shape
    if width != (4 if box_format == 0 else 5):
        raise ValueError("box_format %d takes boxes of %d numbers, got %d" % (box_format, 4 if box_format == 0 else 5, width))
    t_cap = trk_f.shape[1]
    if tuple(trk_f.shape) != (n, t_cap, 17) or tuple(trk_i.shape) != (n, t_cap, 5) or tuple(stream_i.shape) != (n, 4):
        raise ValueError("state shapes must be (n, t_cap, 17), (n, t_cap, 5), (n, 4) with n = %d" % n)
    dev = det_boxes.device
    if out is None:
        out = (torch.empty((n, t_cap, 4), dtype=torch.float32, device=dev), torch.empty((n, t_cap), dtype=torch.int32, device=dev),
               torch.empty((n, t_cap), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev))
    boxes, ids, det, count = out
    if tuple(boxes.shape) != (n, t_cap, 4) or tuple(ids.shape) != (n, t_cap) or tuple(det.shape) != (n, t_cap) or tuple(count.shape) != (n,):
        raise ValueError("output shapes must be (n, t_cap, 4), (n, t_cap), (n, t_cap), (n,)")
    _lib.check(lib.v2x_sort_step(_dev(det_boxes, torch.float32, "det_boxes"), _dev(det_count, torch.int32, "det_count"), n, det_cap, int(box_format),
                                 _dev(trk_f, torch.float32, "trk_f"), _dev(trk_i, torch.int32, "trk_i"), _dev(stream_i, torch.int32, "stream_i"), t_cap,
                                 C.c_float(iou_thr), int(max_age), int(min_hits), int(bool(direct)), _dev(boxes, torch.float32, "out_boxes"),
                                 _dev(ids, torch.int32, "out_ids"), _dev(det, torch.int32, "out_det"), _dev(count, torch.int32, "out_count"), _stream()),
               "v2x_sort_step")
    return out


def hota_sequences(gt_boxes, gt_ids, gt_count, trk_boxes, trk_ids, trk_count, n_gt_ids, n_trk_ids, alpha=None):
    """The HOTA counts of S padded sequences in ONE library call (five launches, no host synchronisation).
    gt_boxes (S, F, cap, 4) fp32 xyxy, gt_ids (S, F, cap) int32, gt_count (S, F) int32, the same for the tracks, cap <= 64; ids per sequence in
    [0, n_gt_ids) / [0, n_trk_ids); alpha: (n_alpha,) float64 on the device or None for HOTA_ALPHAS.
    -> out_i (S, n_alpha, 3) int32 = TP, FN, FP; out_f (S, n_alpha, 4) float64 = AssA, AssRe, AssPr, the sum of the matched similarities."""
    lib = _lib.load()
    S, F, cap, four = gt_boxes.shape
    if four != 4 or tuple(trk_boxes.shape) != (S, F, cap, 4):
        raise ValueError("gt_boxes and trk_boxes must both be (S, F, cap, 4), got %s and %s" % (tuple(gt_boxes.shape), tuple(trk_boxes.shape)))
    for name, t, shape in (("gt_ids", gt_ids, (S, F, cap)), ("trk_ids", trk_ids, (S, F, cap)), ("gt_count", gt_count, (S, F)), ("trk_count", trk_count, (S, F))):
        if tuple(t.shape) != shape:
            raise ValueError("%s must be %s, got %s" % (name, shape, tuple(t.shape)))
    dev = gt_boxes.device
    if alpha is None:
        alpha = torch.from_numpy(HOTA_ALPHAS).to(dev)
    n_alpha = alpha.numel()
    nbytes = lib.v2x_hota_workspace_size(S, F, cap, int(n_gt_ids), int(n_trk_ids), n_alpha)
    if nbytes == 0:
        raise ValueError("hota_sequences: S = %d, F = %d, cap = %d, n_gt_ids = %d, n_trk_ids = %d, n_alpha = %d out of range (F >= 1, cap in [1, %d], n_alpha in "
                         "[1, %d])" % (S, F, cap, n_gt_ids, n_trk_ids, n_alpha, TRACK_CAP, HOTA_MAX_ALPHA))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    out_i = torch.empty((S, n_alpha, 3), dtype=torch.int32, device=dev)
    out_f = torch.empty((S, n_alpha, 4), dtype=torch.float64, device=dev)
    _lib.check(lib.v2x_hota_sequences(_dev(gt_boxes, torch.float32, "gt_boxes"), _dev(gt_ids, torch.int32, "gt_ids"), _dev(gt_count, torch.int32, "gt_count"),
                                      _dev(trk_boxes, torch.float32, "trk_boxes"), _dev(trk_ids, torch.int32, "trk_ids"),
                                      _dev(trk_count, torch.int32, "trk_count"), S, F, cap, int(n_gt_ids), int(n_trk_ids),
                                      _dev(alpha, torch.float64, "alpha"), n_alpha, _dev(ws, torch.uint8, "workspace"), nbytes,
                                      _dev(out_i, torch.int32, "out_i"), _dev(out_f, torch.float64, "out_f"), _stream()), "v2x_hota_sequences")
    return out_i, out_f


def mot_sequences(gt_boxes, gt_ids, gt_count, trk_boxes, trk_ids, trk_count, n_gt_ids, n_trk_ids, thr=0.5):
    """The CLEAR MOT and Identity counts of S padded sequences in ONE library call (five launches, no host synchronisation).
    The arguments of hota_sequences: gt_boxes (S, F, cap, 4) fp32 xyxy, gt_ids (S, F, cap) int32, gt_count (S, F) int32, the same for the tracks,
    cap <= 64; ids per sequence in [0, n_gt_ids) / [0, n_trk_ids), both <= MOT_MAX_IDS; thr: the similarity threshold of both families.
    -> out_i (S, 11) int32 = MOT_FIELDS_I (TP, FN, FP, IDSW, MT, PT, ML, Frag, IDTP, IDFN, IDFP); out_f (S, 1) float64 = the sum of the matched
    similarities (MOTP = that sum / TP)."""
    lib = _lib.load()
    S, F, cap, four = gt_boxes.shape
    if four != 4 or tuple(trk_boxes.shape) != (S, F, cap, 4):
        raise ValueError("gt_boxes and trk_boxes must both be (S, F, cap, 4), got %s and %s" % (tuple(gt_boxes.shape), tuple(trk_boxes.shape)))
    for name, t, shape in (("gt_ids", gt_ids, (S, F, cap)), ("trk_ids", trk_ids, (S, F, cap)), ("gt_count", gt_count, (S, F)), ("trk_count", trk_count, (S, F))):
        if tuple(t.shape) != shape:
            raise ValueError("%s must be %s, got %s" % (name, shape, tuple(t.shape)))
    if not np.isfinite(float(thr)):
        raise ValueError("mot_sequences: thr = %r is not finite" % (thr,))
    dev = gt_boxes.device
    nbytes = lib.v2x_mot_workspace_size(S, F, cap, int(n_gt_ids), int(n_trk_ids))
    if nbytes == 0:
        raise ValueError("mot_sequences: S = %d, F = %d, cap = %d, n_gt_ids = %d, n_trk_ids = %d out of range (F >= 1, cap in [1, %d], ids per side in "
                         "[0, %d])" % (S, F, cap, n_gt_ids, n_trk_ids, TRACK_CAP, MOT_MAX_IDS))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    out_i = torch.empty((S, len(MOT_FIELDS_I)), dtype=torch.int32, device=dev)
    out_f = torch.empty((S, 1), dtype=torch.float64, device=dev)
    _lib.check(lib.v2x_mot_sequences(_dev(gt_boxes, torch.float32, "gt_boxes"), _dev(gt_ids, torch.int32, "gt_ids"), _dev(gt_count, torch.int32, "gt_count"),
                                     _dev(trk_boxes, torch.float32, "trk_boxes"), _dev(trk_ids, torch.int32, "trk_ids"),
                                     _dev(trk_count, torch.int32, "trk_count"), S, F, cap, int(n_gt_ids), int(n_trk_ids), C.c_double(float(thr)),
                                     _dev(ws, torch.uint8, "workspace"), nbytes, _dev(out_i, torch.int32, "out_i"), _dev(out_f, torch.float64, "out_f"),
                                     _stream()), "v2x_mot_sequences")
    return out_i, out_f

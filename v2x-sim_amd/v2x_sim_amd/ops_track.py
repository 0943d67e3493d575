"""Row f-5 (tracking): python wrappers over v2x_assign_iou and v2x_sort_step (csrc/track.hip).  Re-exported by ops.py (`ops.sort_step` ...)."""
import ctypes as C

import torch

from . import _lib
from ._launch import _dev, _stream

TRACK_CAP = 64      # tracks per stream, detections read per map, rows / columns of a matrix: one wave


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

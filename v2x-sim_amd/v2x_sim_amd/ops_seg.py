"""Rows a8 / f-3 (segmentation training targets): the python wrapper over v2x_seg_rasterize -- the boxes of every item of a batch painted into the
uint8 class map that v2x_seg_loss_* and v2x_seg_argmax_confusion read -- and the class weights computed from its histogram.  Re-exported by ops.py
(`ops.rasterize_seg` ...)."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._launch import _dev, _stream

RASTER_MAX_BOXES = 256


def seg_grid(grid):
    """-> (x0, y0, vx, vy, X, Y) of the label map: from an ops.VoxelGrid, a Config (area_extents / voxel_size / map_dims) or that 6-tuple itself."""
    if hasattr(grid, "extents") and hasattr(grid, "voxel"):
        return (grid.extents[0][0], grid.extents[1][0], grid.voxel[0], grid.voxel[1], int(grid.dims[0]), int(grid.dims[1]))
    if hasattr(grid, "area_extents"):
        return (float(grid.area_extents[0][0]), float(grid.area_extents[1][0]), float(grid.voxel_size[0]), float(grid.voxel_size[1]),
                int(grid.map_dims[0]), int(grid.map_dims[1]))
    x0, y0, vx, vy, X, Y = grid
    return (float(x0), float(y0), float(vx), float(vy), int(X), int(Y))


def rasterize_seg(boxes, cls, count, grid, n_classes=8, rank=None, want=("hist",), out=None):
    """Segmentation labels from boxes (v2x_seg_rasterize; the rule: DESIGN.md section 3.8 "Box rasterization").
    boxes (n, cap, 5) fp32 (x, y, w, h, yaw), cls (n, cap) uint8, count (n,) int32, all on the device; grid: see seg_grid; rank: (n_classes,) uint8
    on the device or None (a higher class id paints over a lower one) ->
    dict: labels (n, X, Y) uint8 and the optional outputs named in `want`: owner (n, X, Y) int32 = the winning box's index or -1, hist
    (n, n_classes + 1) int64 = cells per label, the last column counting the ignore label 255.  out: a dict of existing tensors to write into (any
    subset of the keys; an optional output present in `out` is written too).  Every element of every output is written."""
    lib = _lib.load()
    if boxes.dim() != 3 or boxes.shape[2] != 5 or tuple(cls.shape) != tuple(boxes.shape[:2]) or count.numel() != boxes.shape[0]:
        raise ValueError("rasterize_seg: boxes %s, cls %s, count %s" % (tuple(boxes.shape), tuple(cls.shape), tuple(count.shape)))
    n, cap = int(boxes.shape[0]), int(boxes.shape[1])
    x0, y0, vx, vy, X, Y = seg_grid(grid)
    n_classes = int(n_classes)
    unknown = (set(want) - {"owner", "hist"}) | (set(out or ()) - {"labels", "owner", "hist"})
    if unknown:
        raise ValueError("rasterize_seg: unknown output %s" % sorted(unknown))
    if rank is not None and tuple(rank.shape) != (n_classes,):
        raise ValueError("rasterize_seg: rank %s, needs (%d,)" % (tuple(rank.shape), n_classes))
    dev = boxes.device
    res = dict(out) if out is not None else {}
    shapes = {"labels": (torch.uint8, (n, X, Y)), "owner": (torch.int32, (n, X, Y)), "hist": (torch.int64, (n, n_classes + 1))}
    ptr = {}
    for name, (dtype, shape) in shapes.items():
        if name != "labels" and name not in want and name not in res:
            ptr[name] = None
            continue
        t = res.get(name)
        if t is None:
            t = res[name] = torch.empty(shape, dtype=dtype, device=dev)
        elif tuple(t.shape) != shape or t.dtype != dtype:
            raise ValueError("rasterize_seg: out[%r] is %s %s, needs %s %s" % (name, t.dtype, tuple(t.shape), dtype, shape))
        ptr[name] = _dev(t, dtype, name) if n else None
    ws, nbytes = None, 0
    if "hist" in res:
        nbytes = lib.v2x_seg_rasterize_workspace_size(n, X, Y, n_classes)
        if nbytes < 0:
            raise ValueError("rasterize_seg: sizes out of range (n=%d, X=%d, Y=%d, n_classes=%d in [2, 32])" % (n, X, Y, n_classes))
        ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.int32, device=dev)
    _lib.check(lib.v2x_seg_rasterize(_dev(boxes, torch.float32, "boxes") if n else None, _dev(cls, torch.uint8, "cls") if n else None,
                                     _dev(count, torch.int32, "count") if n else None, n, cap, C.c_float(x0), C.c_float(y0), C.c_float(vx), C.c_float(vy),
                                     X, Y, n_classes, _dev(rank, torch.uint8, "rank") if rank is not None and n else None, ptr["labels"], ptr["owner"],
                                     ptr["hist"], _dev(ws, torch.int32, "workspace") if ws is not None and n else None, nbytes, _stream()),
               "v2x_seg_rasterize")
    return res


def pad_box_lists(box_lists, class_lists=None):
    """One (G_m, 5) array of boxes (and one (G_m,) array of class ids; None: every box is class 1) per item -> host arrays padded to the longest
    list: boxes (n, cap, 5) fp32, cls (n, cap) uint8, count (n,) int32."""
    lists = [np.asarray(g, np.float32).reshape(-1, 5) for g in box_lists]
    cap = max([1] + [g.shape[0] for g in lists])
    if cap > RASTER_MAX_BOXES:
        raise ValueError("an item holds %d boxes, the rasterizer takes at most %d" % (cap, RASTER_MAX_BOXES))
    if class_lists is not None and len(class_lists) != len(lists):
        raise ValueError("class_lists holds %d lists for %d items" % (len(class_lists), len(lists)))
    boxes = np.zeros((len(lists), cap, 5), np.float32)
    cls = np.zeros((len(lists), cap), np.uint8)
    count = np.zeros((len(lists),), np.int32)
    for m, g in enumerate(lists):
        boxes[m, :g.shape[0]], count[m] = g, g.shape[0]
        if class_lists is None:
            cls[m, :g.shape[0]] = 1
        else:
            c = np.asarray(class_lists[m]).reshape(-1)
            if c.shape[0] != g.shape[0] or (c.size and (c.min() < 0 or c.max() > 255)):
                raise ValueError("item %d: %d class ids in [0, 255] needed, got %s" % (m, g.shape[0], c))
            cls[m, :g.shape[0]] = c
    return boxes, cls, count


def median_frequency_weights(hist, n_classes):
    """Median-frequency class weights from cells-per-label counts (any shape ending in >= n_classes columns, summed over the leading ones; a trailing
    ignore column is not a class): w_c = median(f) / f_c over the classes with f_c > 0, 0 for the absent ones."""
    h = np.asarray(hist, np.float64).reshape(-1, np.asarray(hist).shape[-1])[:, :n_classes].sum(0)
    w = np.zeros((n_classes,), np.float64)
    seen = h > 0
    if seen.any():
        f = h[seen] / h[seen].sum()
        w[seen] = np.median(f) / f
    return w.tolist()

"""Row f-2 (visibility maps): the python wrappers over v2x_lidar_freespace_bits, v2x_vis_bits_to_dense_f32 and v2x_vis_mask_labels -- the voxels the
rays of a sweep crossed before they returned, upstream's three-state `vis_maps` from them, and segmentation labels with the cells nobody observed set
to the ignore class.  The rule: DESIGN.md section 3.13.  Re-exported by ops.py (`ops.freespace_bits` ...)."""
import ctypes as C
import math

import torch

from . import _lib
from ._launch import _dev, _dev_opt, _stream


def freespace_bits(points, n_pts, grid, origin=None, xform=None, src_cloud=None, dst_grid=None, n_grids=None, out=None):
    """The voxels some ray passed through (v2x_lidar_freespace_bits).  points (n_clouds, max_pts, stride >= 3) fp32 and n_pts (n_clouds,) int32 as
    ops.voxelize_bits reads them; grid: an ops.VoxelGrid with Z <= 32.  Jobs as in ops.voxelize_fused_bits: job j walks the rays of cloud src_cloud[j]
    from origin[j] (n_jobs, 3) fp32 (None: the zero vector, a ray-cast sweep) to each point, both moved by xform[j] (n_jobs, 3, 4) fp32 (None:
    identity), into grid dst_grid[j]; src_cloud and dst_grid (n_jobs,) int32 come together, or neither: job j = cloud j -> grid j.  n_grids: the number
    of target grids (needed with dst_grid; otherwise n_clouds).  -> trav_bits (n_grids, X, Y) int32, every word written.  Occupied is
    ops.voxelize_bits' / ops.voxelize_fused_bits' result on the same clouds and jobs, free is trav & ~occ."""
    lib = _lib.load()
    if points.dim() != 3 or points.shape[2] < 3:
        raise ValueError("freespace_bits: points must be (n_clouds, max_pts, stride >= 3), got %s" % (tuple(points.shape),))
    n, mp, st = (int(v) for v in points.shape)
    if tuple(n_pts.shape) != (n,):
        raise ValueError("freespace_bits: n_pts must hold one count per cloud: expected shape (%d,), got %s" % (n, tuple(n_pts.shape)))
    if (src_cloud is None) != (dst_grid is None):
        raise ValueError("freespace_bits: src_cloud and dst_grid come together or not at all")
    if src_cloud is not None:
        n_jobs = int(src_cloud.shape[0])
        if tuple(src_cloud.shape) != (n_jobs,) or tuple(dst_grid.shape) != (n_jobs,):
            raise ValueError("freespace_bits: src_cloud %s and dst_grid %s must both be (n_jobs,)" % (tuple(src_cloud.shape), tuple(dst_grid.shape)))
        if n_grids is None:
            raise ValueError("freespace_bits: n_grids is needed with dst_grid (the indices are device data)")
    else:
        n_jobs = n
        if n_grids is None:
            n_grids = n
    n_grids = int(n_grids)
    if n_grids < 0 or n_jobs > 65535:
        raise ValueError("freespace_bits: n_grids=%d must be >= 0 and n_jobs=%d <= 65535" % (n_grids, n_jobs))
    if xform is not None and tuple(xform.shape) != (n_jobs, 3, 4):
        raise ValueError("freespace_bits: xform %s, needs (%d, 3, 4)" % (tuple(xform.shape), n_jobs))
    if origin is not None and tuple(origin.shape) != (n_jobs, 3):
        raise ValueError("freespace_bits: origin %s, needs (%d, 3)" % (tuple(origin.shape), n_jobs))
    X, Y, Z = grid.dims
    if not 1 <= Z <= 32:
        raise ValueError("freespace_bits: Z=%d must be in [1, 32]" % Z)
    if out is None:
        out = torch.empty((n_grids, X, Y), dtype=torch.int32, device=points.device)
    elif tuple(out.shape) != (n_grids, X, Y):
        raise ValueError("freespace_bits: out %s, needs %s" % (tuple(out.shape), (n_grids, X, Y)))
    _lib.check(lib.v2x_lidar_freespace_bits(_dev(points, torch.float32, "points"), _dev(n_pts, torch.int32, "n_pts"), n, mp, st,
                                            _dev_opt(origin, torch.float32, "origin"), _dev_opt(xform, torch.float32, "xform"),
                                            _dev_opt(src_cloud, torch.int32, "src_cloud"), _dev_opt(dst_grid, torch.int32, "dst_grid"), n_jobs, n_grids,
                                            grid._ext, grid._vox, grid._dims, _dev(out, torch.int32, "trav_bits"), _stream()), "v2x_lidar_freespace_bits")
    return out


def _bit_pair(what, occ_bits, trav_bits):
    if occ_bits.dim() != 3 or tuple(trav_bits.shape) != tuple(occ_bits.shape):
        raise ValueError("%s: occ_bits %s and trav_bits %s must both be (n, X, Y)" % (what, tuple(occ_bits.shape), tuple(trav_bits.shape)))
    return (int(v) for v in occ_bits.shape)


def vis_maps(occ_bits, trav_bits, Z, p_occ=0.7, p_free=0.4, out=None):
    """Upstream's vis_maps (v2x_vis_bits_to_dense_f32): occ_bits, trav_bits (n, X, Y) int32 -> (n, X, Y, Z) fp32 holding the log-odds log(p / (1 - p))
    of p_occ where occupied, of p_free where trav & ~occ, and 0 (p = 0.5) where unknown.  Every element is written."""
    lib = _lib.load()
    n, X, Y = _bit_pair("vis_maps", occ_bits, trav_bits)
    Z = int(Z)
    if not 1 <= Z <= 32:
        raise ValueError("vis_maps: Z=%d must be in [1, 32]" % Z)
    if not (0.0 < p_occ < 1.0 and 0.0 < p_free < 1.0):
        raise ValueError("vis_maps: p_occ=%r and p_free=%r must lie in (0, 1)" % (p_occ, p_free))
    if out is None:
        out = torch.empty((n, X, Y, Z), dtype=torch.float32, device=occ_bits.device)
    elif tuple(out.shape) != (n, X, Y, Z):
        raise ValueError("vis_maps: out %s, needs %s" % (tuple(out.shape), (n, X, Y, Z)))
    _lib.check(lib.v2x_vis_bits_to_dense_f32(_dev(occ_bits, torch.int32, "occ_bits"), _dev(trav_bits, torch.int32, "trav_bits"), n, X, Y, Z,
                                             C.c_float(math.log(p_occ / (1.0 - p_occ))), C.c_float(math.log(p_free / (1.0 - p_free))), C.c_float(0.0),
                                             _dev(out, torch.float32, "out"), _stream()), "v2x_vis_bits_to_dense_f32")
    return out


def mask_unobserved(labels, occ_bits, trav_bits, z_mask=None, ignore=255, out=None):
    """Labels with the cells nobody observed ignored (v2x_vis_mask_labels): labels (n, X, Y) uint8, occ_bits, trav_bits (n, X, Y) int32 -> (n, X, Y)
    uint8 = `ignore` where ((occ | trav) & z_mask) == 0, else labels.  z_mask: the z bits that count (None: all 32).  out: the tensor to write into;
    out=labels masks in place."""
    lib = _lib.load()
    n, X, Y = _bit_pair("mask_unobserved", occ_bits, trav_bits)
    if tuple(labels.shape) != (n, X, Y):
        raise ValueError("mask_unobserved: labels %s, needs %s" % (tuple(labels.shape), (n, X, Y)))
    z_mask = 0xffffffff if z_mask is None else int(z_mask)
    if not 0 <= z_mask <= 0xffffffff or not 0 <= int(ignore) <= 255:
        raise ValueError("mask_unobserved: z_mask=%r must fit 32 bits and ignore=%r one byte" % (z_mask, ignore))
    if out is None:
        out = torch.empty((n, X, Y), dtype=torch.uint8, device=labels.device)
    elif tuple(out.shape) != (n, X, Y):
        raise ValueError("mask_unobserved: out %s, needs %s" % (tuple(out.shape), (n, X, Y)))
    _lib.check(lib.v2x_vis_mask_labels(_dev(labels, torch.uint8, "labels"), _dev(occ_bits, torch.int32, "occ_bits"), _dev(trav_bits, torch.int32, "trav_bits"),
                                       n, X, Y, C.c_uint32(z_mask), int(ignore), _dev(out, torch.uint8, "labels_out"), _stream()), "v2x_vis_mask_labels")
    return out

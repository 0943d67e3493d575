"""Stage-level python wrappers over the C ABI (one per SURVEY.md section 8 row).

PyTorch is plumbing here: it owns device memory and the stream; all arithmetic
happens inside libv2x_amd.so.  Every wrapper refuses non-device tensors -- there
is deliberately no eager/CPU fallback.
"""
import ctypes as C
import functools

import torch

from . import _lib, tuning
from ._lib import ConvDesc, V2X_EPI_BF16, V2X_EPI_F32, V2X_EPI_GRU, V2X_FUSE_MAX, V2X_FUSE_MEAN, V2X_FUSE_WSUM  # noqa: F401


from . import _launch
from ._launch import _Prof, _dev, _dev_opt, _stream  # noqa: F401


# Latency dispatch.  Kernel forms whose choice depends on the NUMBER of maps in a launch (split-K of the streamed layers, the 1-tap stride-2
# kernel below four tiles per CU) change the fp32 summation order, so they are never taken silently: the caller declares a latency launch.
# tuning SMALL_BATCH: 0 never; 1 every launch of the process (the explicit pin, also for the sharded runners); 2 (default) only inside a
# `with ops.latency_dispatch():` block -- the plain single-GPU model classes enter one in forward_nhwc() (@ops.latency_entry: the common entry
# of forward(), forward_points() and the Seg / Det modules), the sharded runners (R-rank == 1-rank bitwise) never do.
# NOT only a summation order: the streamed parity-class kernel (conv5_1, conv6_1: w_layout 4) has no split-K form, so a declared latency
# launch that splits takes `Layer.latency` -- the layer's 9-TAP bf16 weights -- while a throughput launch of the same model multiplies the PRE-SUMMED
# parity-class weights (fp32 sums of 1, 2 or 4 taps rounded to bf16 once).  The two forms agree with the fp32 oracle layer to the same bound
# (tests/test_gpu_parity_class.py) but differ from each other by that weight rounding, not just by summation order; one-frame inference mixes them
# (conv7_1 / conv8_1 parity-class, conv5_1 / conv6_1 9-tap).  Bounded end to end: tests/test_gpu_bits_input.py (latency vs throughput logits of one frame
# within 2e-2 of max|ref|) and tests/test_gpu_models.py (either dispatch within TOL of the oracle).
import threading as _threading

_latency = _threading.local()   # per THREAD: a latency forward in one thread must not switch a sharded runner or a training step in another
                                # thread to the split-K / 1-tap forms (that would break their R-rank == 1-rank bitwise guarantee)


class latency_dispatch:
    """Context manager: launches of THIS thread inside the block are declared latency launches (see above)."""

    def __init__(self, target=0):
        self.target = target      # > 0: the number of workgroups small_batch_splitk aims at inside this block (default 320; the training graph's sweep)

    def __enter__(self):
        _latency.depth = getattr(_latency, "depth", 0) + 1
        self.prev, _latency.target = getattr(_latency, "target", 0), self.target
        return self

    def __exit__(self, *exc):
        _latency.depth -= 1
        _latency.target = self.prev
        return False


def latency_entry(fn):
    """Decorator of the plain single-GPU model entries (forward_nhwc of every model class): launches inside are declared latency launches."""
    @functools.wraps(fn)
    def wrapped(*a, **k):
        with latency_dispatch():
            return fn(*a, **k)
    return wrapped


def latency_launches():
    sb = tuning.get("SMALL_BATCH")
    return sb == 1 or (sb == 2 and getattr(_latency, "depth", 0) > 0)


def _conv_shape(pc, N, H, W):
    """What the packed layer and the extent determine of a v2x_conv_desc; the caller adds the tensors."""
    d = ConvDesc()
    d.C0, d.C1, d.up0 = pc.C0, pc.C1, pc.up0
    d.N, d.H, d.W = N, H, W
    d.ksize, d.stride, d.pad = pc.ksize, pc.stride, pc.pad
    d.Cout, d.w_rows, d.w_kpad = pc.Cout, pc.w_rows, pc.w_kpad
    d.epilogue, d.relu = pc.epilogue, int(bool(pc.relu))
    d.w_layout = pc.w_layout or 0
    if pc.Cout2:
        d.Cout2, d.relu2 = pc.Cout2, int(bool(pc.relu2))
    return d


def _conv_desc(pc, N, H, W):
    """_conv_shape with the layer's packed parameters; the caller adds the activations and the output."""
    d = _conv_shape(pc, N, H, W)
    d.weight = pc.weight.data_ptr()
    d.scale = pc.scale.data_ptr()
    d.shift = pc.shift.data_ptr() if pc.shift is not None else None
    if pc.Cout2:
        d.weight2, d.scale2, d.shift2 = pc.weight2.data_ptr(), pc.scale2.data_ptr(), pc.shift2.data_ptr()
    return d


_NEVER_READ = 16   # placeholder address of every tensor of a plan descriptor: non-null and 16-byte aligned as the dispatch asks, never dereferenced


def _plan_desc(pc, N, H, W, bits):
    """The descriptor conv_kernel_name and covers hand to v2x_conv2d_plan: _conv_shape with a placeholder for every tensor (so a PackedConv that
    carries no tensors yet -- packing.train_conv_shape -- can be asked about), one unsplit output window, no split-K."""
    d = _conv_shape(pc, N, H, W)
    d.in0 = d.weight = d.scale = d.shift = d.out = _NEVER_READ
    if pc.C1:
        d.in1 = _NEVER_READ
    if pc.Cout2:
        d.weight2 = d.scale2 = d.shift2 = _NEVER_READ
    if bits:
        d.in_format, d.in_zbits = 1, 1
    d.out_cstride = pc.Cout2 or pc.Cout
    if pc.epilogue == _lib.V2X_EPI_DET:      # the candidate epilogue's outputs as conv2d_det sets them: keys, codes (6 per candidate), counts
        d.out2, d.out2_cstride, d.det_counts, d.det_cap, d.det_thr, d.out_cstride = _NEVER_READ, 6, _NEVER_READ, 4096, 0.5, 4096
    return d


def conv_kernel_name(pc, H, W, bits=False, N=1):
    """Name of the kernel v2x_conv2d launches for layer pc on N maps of H x W (the layer's full-resolution input extent), as rocprofv3 prints it:
    asked of the library's own dispatch (v2x_conv2d_plan), nothing is launched.  Every tensor is a 16-byte aligned placeholder: the answer
    is the one for aligned tensors (a misaligned 1x1 launch takes the gather kernel; conv2d's profiling branch asks with its real descriptor)."""
    d = _plan_desc(pc, N, H, W, bits)
    d.small_batch = 1 if latency_launches() else 0
    return _lib.conv_plan(d, "v2x_conv2d_plan(%s)" % pc.name)


def covers(pc, H, W, bits=False):
    """Has v2x_conv2d a kernel for layer pc on maps of H x W (bits: on the voxelizer's bit grid)?  The library's own dispatch answers; the
    boolean is kept on the packing -- never a kernel name, which follows the switches, the number of maps and the latency declaration (the covered
    set follows none: tests/test_coverage_cpu.py).  A refusal's text stays in v2x_last_error; _lib.check re-reads it after its own failing call."""
    hit = pc.covered.get((H, W, bits))
    if hit is None:
        buf = C.create_string_buffer(512)
        hit = pc.covered[(H, W, bits)] = _lib.load().v2x_conv2d_plan(C.byref(_plan_desc(pc, 1, H, W, bits)), buf, len(buf)) == 0
    return hit


@functools.lru_cache(maxsize=None)
def wgrad_covers(H, W, cin, cout):
    """Has v2x_conv3x3_wgrad a kernel for cin -> cout channels on maps of H x W?  The library's answer (a workspace slot count of 0: no), kept."""
    return _lib.load().v2x_conv3x3_wgrad_splits(1, H, W, cin, cout) != 0


# ------------------------------------------------------------------ a1
class VoxelGrid:
    """Geometry of the BEV grid (upstream Config.voxel_size / area_extents)."""

    def __init__(self, voxel_size=(0.25, 0.25, 0.4), area_extents=((-32.0, 32.0), (-32.0, 32.0), (-3.0, 2.0))):
        import math
        self.voxel = tuple(float(v) for v in voxel_size)
        self.extents = tuple((float(lo), float(hi)) for lo, hi in area_extents)
        self.dims = tuple(int(math.ceil(hi / v) - 1 - math.floor(lo / v) + 1)
                          for (lo, hi), v in zip(self.extents, self.voxel))
        self._ext = (C.c_double * 6)(*[x for lohi in self.extents for x in lohi])
        self._vox = (C.c_double * 3)(*self.voxel)
        self._dims = (C.c_int32 * 3)(*self.dims)


def voxelize_bits(points, n_pts, grid, out=None):
    """points (n_clouds, max_pts, stride>=3) fp32, n_pts (n_clouds,) int32 -> bits (n_clouds, X, Y) int32."""
    lib = _lib.load()
    if points.dim() != 3:
        raise ValueError("points must be (n_clouds, max_pts, stride)")
    n, mp, st = points.shape
    if tuple(n_pts.shape) != (n,):
        raise ValueError("n_pts must hold one count per cloud: expected shape (%d,), got %s" % (n, tuple(n_pts.shape)))
    X, Y, Z = grid.dims
    if out is None:
        out = torch.empty((n, X, Y), dtype=torch.int32, device=points.device)
    vl = tuning.get("VOXELIZE_LDS")
    lds = Z <= 16 and X * Y * 2 <= 128 * 1024 and (X * Y) % 8 == 0 and mp > 0 and vl != 0 and (vl == 2 or n > 48)
    prof = (_Prof("voxelize_lds_kernel", 0, points.numel() * 4 + out.numel() * 4) if lds else
            _Prof("voxelize_scatter_kernel", 0, points.numel() * 4 + 2 * out.numel() * 4))
    rc = lib.v2x_voxelize_bits(_dev(points, torch.float32, "points"), _dev(n_pts, torch.int32, "n_pts"), n, mp, st,
                               grid._ext, grid._vox, grid._dims, _dev(out, torch.int32, "bits"), _stream())
    prof.done()
    _lib.check(rc, "v2x_voxelize_bits")
    return out


def voxelize_fused_bits(points, n_pts, xform, src_cloud, dst_grid, n_grids, grid):
    """Early fusion: job j scatters cloud src_cloud[j], moved by xform[j] (n_jobs, 3, 4) fp32, into grid dst_grid[j].
    -> bits (n_grids, X, Y) int32."""
    lib = _lib.load()
    n, mp, st = points.shape
    n_jobs = xform.shape[0]
    if tuple(n_pts.shape) != (n,):
        raise ValueError("n_pts must hold one count per cloud: expected shape (%d,), got %s" % (n, tuple(n_pts.shape)))
    if tuple(xform.shape) != (n_jobs, 3, 4) or src_cloud.shape[0] != n_jobs or dst_grid.shape[0] != n_jobs:
        raise ValueError("xform (n_jobs, 3, 4), src_cloud (n_jobs,), dst_grid (n_jobs,) expected")
    X, Y, Z = grid.dims
    out = torch.empty((n_grids, X, Y), dtype=torch.int32, device=points.device)
    rc = lib.v2x_voxelize_fused_bits(_dev(points, torch.float32, "points"), _dev(n_pts, torch.int32, "n_pts"), n, mp, st,
                                     _dev(xform, torch.float32, "xform"), _dev(src_cloud, torch.int32, "src_cloud"),
                                     _dev(dst_grid, torch.int32, "dst_grid"), n_jobs, n_grids, grid._ext, grid._vox,
                                     grid._dims, _dev(out, torch.int32, "bits"), _stream())
    _lib.check(rc, "v2x_voxelize_fused_bits")
    return out


def bits_to_dense(bits, Z):
    lib = _lib.load()
    n, X, Y = bits.shape
    out = torch.empty((n, X, Y, Z), dtype=torch.float32, device=bits.device)
    _lib.check(lib.v2x_bits_to_dense_f32(_dev(bits, torch.int32, "bits"), n, X, Y, Z, _dev(out, torch.float32, "out"),
                                         _stream()), "v2x_bits_to_dense_f32")
    return out


def bits_to_nhwc(bits, Z, c_pad=16, out=None):
    lib = _lib.load()
    n, X, Y = bits.shape
    if out is None:
        out = torch.empty((n, X, Y, c_pad), dtype=torch.bfloat16, device=bits.device)
    prof = _Prof("bits_to_nhwc_bf16_kernel", 0, bits.numel() * 4 + out.numel() * 2)
    rc = lib.v2x_bits_to_nhwc_bf16(_dev(bits, torch.int32, "bits"), n, X, Y, Z, c_pad,
                                   _dev(out, torch.bfloat16, "out"), _stream())
    prof.done()
    _lib.check(rc, "v2x_bits_to_nhwc_bf16")
    return out


def dense_to_nhwc(bev, c_pad=16, out=None):
    """bev (n, X, Y, Z) fp32 -> (n, X, Y, c_pad) bf16."""
    lib = _lib.load()
    n, X, Y, Z = bev.shape
    if out is None:
        out = torch.empty((n, X, Y, c_pad), dtype=torch.bfloat16, device=bev.device)
    _lib.check(lib.v2x_dense_f32_to_nhwc_bf16(_dev(bev, torch.float32, "bev"), n, X, Y, Z, c_pad,
                                              _dev(out, torch.bfloat16, "out"), _stream()),
               "v2x_dense_f32_to_nhwc_bf16")
    return out


def bits_to_indices(bits, Z, cap):
    """-> (idx (n, cap, 3) int32 sorted lexicographically, counts (n,) int32)."""
    lib = _lib.load()
    n, X, Y = bits.shape
    idx = torch.zeros((n, cap, 3), dtype=torch.int32, device=bits.device)
    counts = torch.zeros((n,), dtype=torch.int32, device=bits.device)
    scratch = torch.empty((n, X), dtype=torch.int32, device=bits.device)
    _lib.check(lib.v2x_bits_to_indices(_dev(bits, torch.int32, "bits"), n, X, Y, Z, _dev(idx, torch.int32, "idx"), cap,
                                       _dev(counts, torch.int32, "counts"), _dev(scratch, torch.int32, "scratch"),
                                       _stream()), "v2x_bits_to_indices")
    return idx, counts


def indices_to_bits(idx, counts, grid):
    """idx (n, cap, 3) int32 sparse voxel indices, counts (n,) int32 -> bits (n, X, Y) int32 (the densify
    scatter of the parsed-dataset reader, on the GPU)."""
    lib = _lib.load()
    n, cap, three = idx.shape
    if three != 3:
        raise ValueError("idx must be (n, cap, 3)")
    X, Y, Z = grid.dims
    out = torch.empty((n, X, Y), dtype=torch.int32, device=idx.device)
    _lib.check(lib.v2x_indices_to_bits(_dev(idx, torch.int32, "idx"), _dev(counts, torch.int32, "counts"), n, cap,
                                       X, Y, Z, _dev(out, torch.int32, "bits"), _stream()), "v2x_indices_to_bits")
    return out


# ------------------------------------------------------------------ a2/a4/a6/a7/a8
class PackedConv:
    """Device-resident packed parameters of one conv layer (see packing.py)."""

    __slots__ = ("weight", "scale", "shift", "C0", "C1", "Cout", "ksize", "stride", "pad", "up0", "epilogue", "relu",
                 "w_rows", "w_kpad", "name", "w_layout", "Cout2", "weight2", "scale2", "shift2", "relu2",
                 "repack",   # packing.pack_conv_device: what packing.RepackPlan needs to rebuild `weight` in place (None otherwise)
                 "covered")  # covers(): {(H, W, bits): v2x_conv2d has a kernel for this packing at that extent}

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))
        self.covered = {}


def conv_out_hw(pc, H, W):
    Ho = (H + 2 * pc.pad - pc.ksize) // pc.stride + 1
    Wo = (W + 2 * pc.pad - pc.ksize) // pc.stride + 1
    return Ho, Wo


def conv2d(pc, in0, in1=None, out=None, out_coff=0, split=0, zbits=0, splitk=0):
    """in0 (N, H>>up0, W>>up0, C0) bf16 NHWC [, in1 (N, H, W, C1)] -> out (N, Ho, Wo, Cout) NHWC.

    split > 0: returns (out[..., :split], out2[..., Cout-split]) as two contiguous tensors.
    splitk > 1 (streamed stride-1 layers without a chained 1x1): the small-batch form, see small_batch_splitk()."""
    lib = _lib.load()
    # the gather kernel does its row arithmetic in 24 bits (N*H*W < 2^24): larger batches go through in slices of whole
    # maps (contiguous NHWC views, same stream) -- the only kernel with that limit, and only 256x256 inputs reach it
    if not pc.w_layout and in0.dtype != torch.int32:
        Hx, Wx = (in1.shape[1], in1.shape[2]) if in1 is not None else (in0.shape[1] << pc.up0, in0.shape[2] << pc.up0)
        N0 = in0.shape[0]
        if N0 * Hx * Wx >= (1 << 24) and N0 > 1:
            Ho, Wo = conv_out_hw(pc, Hx, Wx)
            odt = torch.float32 if pc.epilogue == V2X_EPI_F32 else torch.bfloat16
            cfin = pc.Cout2 if pc.Cout2 else pc.Cout
            o1 = o2 = None
            if split:
                o1 = torch.empty((N0, Ho, Wo, split), dtype=odt, device=in0.device)
                o2 = torch.empty((N0, Ho, Wo, cfin - split), dtype=odt, device=in0.device)
            elif out is None:
                out = torch.empty((N0, Ho, Wo, cfin), dtype=odt, device=in0.device)
            step = max(1, ((1 << 24) - 1) // (Hx * Wx))
            for a0 in range(0, N0, step):
                sl = slice(a0, min(a0 + step, N0))
                r = conv2d(pc, in0[sl], None if in1 is None else in1[sl], None if split else out[sl], out_coff, split, zbits)
                if split:
                    o1[sl].copy_(r[0])
                    o2[sl].copy_(r[1])
            return (o1, o2) if split else out
    from_bits = in0.dtype == torch.int32  # the voxelizer's bit grid (N, H, W): first layer, halo kernel only
    if from_bits:
        if pc.w_layout != 1 or in1 is not None or in0.dim() != 3 or not (1 <= zbits <= 32):
            raise ValueError("bit-grid input needs a halo-packed single-source layer and 1 <= zbits <= 32")
        p_in0 = _dev(in0, torch.int32, "in0").value
        in0_shape = (in0.shape[0], in0.shape[1], in0.shape[2], pc.C0)
    else:
        p_in0 = _dev(in0, torch.bfloat16, "in0").value
        in0_shape = tuple(in0.shape)
    N = in0.shape[0]
    p_in1 = None
    if in1 is not None:
        p_in1 = _dev(in1, torch.bfloat16, "in1").value
        H, W = in1.shape[1], in1.shape[2]
        if in1.shape[3] != pc.C1 or in1.shape[0] != N:
            raise ValueError("in1 shape %s does not match C1=%d" % (tuple(in1.shape), pc.C1))
        if (in0.shape[1] << pc.up0, in0.shape[2] << pc.up0) != (H, W):
            raise ValueError("in0 %s (up0=%d) does not match in1 %s" % (tuple(in0.shape), pc.up0, tuple(in1.shape)))
    else:
        if pc.C1:
            raise ValueError("layer %s expects a second source" % pc.name)
        H, W = in0.shape[1] << pc.up0, in0.shape[2] << pc.up0
    if in0_shape[3] != pc.C0:
        raise ValueError("in0 has %d channels, layer %s expects %d" % (in0_shape[3], pc.name, pc.C0))
    Ho, Wo = conv_out_hw(pc, H, W)
    odt = torch.float32 if pc.epilogue == V2X_EPI_F32 else torch.bfloat16
    cfin = pc.Cout2 if pc.Cout2 else pc.Cout  # channels of the tensor that is actually written
    out2 = None
    if split:
        out = torch.empty((N, Ho, Wo, split), dtype=odt, device=in0.device)
        out2 = torch.empty((N, Ho, Wo, cfin - split), dtype=odt, device=in0.device)
    elif out is None:
        out = torch.empty((N, Ho, Wo, cfin), dtype=odt, device=in0.device)
    elif tuple(out.shape[:3]) != (N, Ho, Wo):
        raise ValueError("out shape %s != %s" % (tuple(out.shape), (N, Ho, Wo, "*")))
    d = _conv_desc(pc, N, H, W)
    d.in0, d.in1 = p_in0, p_in1
    if from_bits:
        d.in_format, d.in_zbits = 1, zbits
    d.out = _dev(out, odt, "out").value
    d.out_cstride, d.out_coff = out.shape[3], out_coff
    if split:
        d.out2, d.split, d.out2_cstride = out2.data_ptr(), split, out2.shape[3]
    ws = None
    if splitk > 1:
        ws = torch.empty((splitk, N * Ho * Wo, pc.w_rows), dtype=torch.float32, device=in0.device)
        d.splitk, d.splitk_ws = splitk, ws.data_ptr()
    d.small_batch = 1 if latency_launches() else 0
    prof = None
    if _launch.PROFILE is not None:
        rows_logical = 3 * pc.Cout if pc.epilogue == V2X_EPI_GRU else pc.Cout
        k_logical = pc.ksize * pc.ksize * (zbits if from_bits else pc.C0 + pc.C1)   # bit-grid input: zbits real channels, the rest padding
        M = N * Ho * Wo
        nbytes = in0.numel() * (4 if from_bits else 2) + (in1.numel() * 2 if in1 is not None else 0) + pc.weight.numel() * 2 \
            + M * cfin * (4 if pc.epilogue == V2X_EPI_F32 else 2)
        flops = 2.0 * M * (rows_logical * k_logical + (pc.Cout2 or 0) * pc.Cout)
        if pc.w_layout in (3, 4):   # parity-class forms: the FLOPs the kernel EXECUTES (4 taps on the upsampled source); the reference's 9-tap count is
            flops = 2.0 * M * pc.Cout * (4 * pc.C0 + 9 * pc.C1)   # reported separately (bench.py: reference_flops)
        prof = _Prof(_lib.conv_plan(d, "v2x_conv2d_plan(%s)" % pc.name), flops, nbytes, pc.name)   # the descriptor about to be launched
    rc = lib.v2x_conv2d(C.byref(d), _stream())
    if prof is not None:
        prof.done()
    _lib.check(rc, "v2x_conv2d(%s)" % pc.name)
    return (out, out2) if split else out


# ------------------------------------------------------------------ communication codec (compress_level; codec.hip)
class PackedCodec:
    """Device-resident packed parameters of the compress / decompress pair (packing.pack_codec): `weight` = the MFMA fragments of both
    matrices (include/v2x_amd.h), `ss` = their folded scales and shifts."""

    __slots__ = ("name", "C", "Cc", "weight", "ss")

    def __init__(self, name, C, Cc, weight, ss):
        self.name, self.C, self.Cc, self.weight, self.ss = name, C, Cc, weight, ss


def _codec_rows(pc, t, channels, what):
    if t.shape[-1] != channels:
        raise ValueError("%s: %s has %d channels, expected %d" % (pc.name, what, t.shape[-1], channels))
    return t.numel() // channels


def codec(pc, x, want_msg=False):
    """x (..., C) bf16 NHWC -> y of the same shape: relu(bn_d(Wd relu(bn_c(Wc x)))) in one launch, the Cc-channel message kept in registers.
    want_msg: -> (y, msg (..., Cc) bf16), the message an agent would send (natural channel order)."""
    M = _codec_rows(pc, x, pc.C, "x")
    y = torch.empty_like(x)
    msg = torch.empty(tuple(x.shape[:-1]) + (pc.Cc,), dtype=torch.bfloat16, device=x.device) if want_msg else None
    prof = _Prof("codec_kernel<%d, %d, fused>" % (pc.C, pc.Cc), 4.0 * M * pc.C * pc.Cc, M * (4 * pc.C + (2 * pc.Cc if want_msg else 0)), pc.name)
    rc = _lib.load().v2x_codec_1x1(_dev(x, torch.bfloat16, "x"), M, pc.C, pc.Cc, _dev(pc.weight, torch.bfloat16, "weight"), _dev(pc.ss, torch.float32, "ss"),
                                   _dev(y, torch.bfloat16, "y"), _dev_opt(msg, torch.bfloat16, "msg"), _stream())
    prof.done()
    _lib.check(rc, "v2x_codec_1x1(%s)" % pc.name)
    return (y, msg) if want_msg else y


def codec_compress(pc, x):
    """The sender's half: x (..., C) bf16 -> msg (..., Cc) bf16."""
    M = _codec_rows(pc, x, pc.C, "x")
    msg = torch.empty(tuple(x.shape[:-1]) + (pc.Cc,), dtype=torch.bfloat16, device=x.device)
    prof = _Prof("codec_kernel<%d, %d, compress>" % (pc.C, pc.Cc), 2.0 * M * pc.C * pc.Cc, M * 2 * (pc.C + pc.Cc), pc.name)
    rc = _lib.load().v2x_codec_compress(_dev(x, torch.bfloat16, "x"), M, pc.C, pc.Cc, _dev(pc.weight, torch.bfloat16, "weight"),
                                        _dev(pc.ss, torch.float32, "ss"), _dev(msg, torch.bfloat16, "msg"), _stream())
    prof.done()
    _lib.check(rc, "v2x_codec_compress(%s)" % pc.name)
    return msg


def codec_decompress(pc, msg):
    """The receiver's half: msg (..., Cc) bf16 -> y (..., C) bf16; codec_decompress(codec_compress(x)) is bit-identical to codec(x)."""
    M = _codec_rows(pc, msg, pc.Cc, "msg")
    y = torch.empty(tuple(msg.shape[:-1]) + (pc.C,), dtype=torch.bfloat16, device=msg.device)
    prof = _Prof("codec_kernel<%d, %d, decompress>" % (pc.C, pc.Cc), 2.0 * M * pc.C * pc.Cc, M * 2 * (pc.C + pc.Cc), pc.name)
    rc = _lib.load().v2x_codec_decompress(_dev(msg, torch.bfloat16, "msg"), M, pc.C, pc.Cc, _dev(pc.weight, torch.bfloat16, "weight"),
                                          _dev(pc.ss, torch.float32, "ss"), _dev(y, torch.bfloat16, "y"), _stream())
    prof.done()
    _lib.check(rc, "v2x_codec_decompress(%s)" % pc.name)
    return y


def pair_eligible(pa, pb, in0, zbits):
    """conv_halo_pair.hip covers: bit-grid input, two halo-packed 3x3 s1 32 -> 32 bf16 layers, H % 8 == 0, W % 32 == 0."""
    ok = lambda pc: (pc is not None and pc.w_layout == 1 and pc.ksize == 3 and pc.stride == 1 and pc.C0 == 32 and not pc.C1  # noqa: E731
                     and pc.Cout == 32 and not pc.Cout2 and pc.epilogue == V2X_EPI_BF16)
    return (ok(pa) and ok(pb) and in0.dtype == torch.int32 and in0.dim() == 3 and 1 <= zbits <= 16
            and in0.shape[1] % 8 == 0 and in0.shape[2] % 32 == 0 and tuning.get("CONV_PAIR") != 0)


def conv2d_pair(pa, pb, bits, zbits, out=None):
    """pb(pa(bits)) in one launch, the intermediate map never stored (conv_pre_1 -> conv_pre_2).  bits (N, H, W) int32."""
    lib = _lib.load()
    N, H, W = bits.shape
    if out is None:
        out = torch.empty((N, H, W, pb.Cout), dtype=torch.bfloat16, device=bits.device)
    da, db = _conv_desc(pa, N, H, W), _conv_desc(pb, N, H, W)
    da.in0 = _dev(bits, torch.int32, "bits").value
    da.in_format, da.in_zbits = 1, zbits
    db.out = _dev(out, torch.bfloat16, "out").value
    db.out_cstride, db.out_coff = out.shape[3], 0
    prof = None
    if _launch.PROFILE is not None:
        M = N * H * W
        # algorithmic FLOPs: the first layer has `zbits` (13) real input channels -- the 32 of the packed layout are zero padding
        prof = _Prof("conv3x3_pair_bits_kernel<%s>" % ("true" if tuning.get("STORE_X4") != 0 else "false"), 2.0 * M * 9 * (pa.Cout * zbits + pb.Cout * pb.C0),
                     bits.numel() * 4 + out.numel() * 2 + (pa.weight.numel() + pb.weight.numel()) * 2, pa.name + "+" + pb.name)
    rc = lib.v2x_conv2d_pair(C.byref(da), C.byref(db), _stream())
    if prof is not None:
        prof.done()
    _lib.check(rc, "v2x_conv2d_pair(%s, %s)" % (pa.name, pb.name))
    return out


def tail_eligible(pa, pb, x, split=12):
    """conv_tail.hip covers: conv8_2 as a halo-packed 3x3 s1 32 -> 32 bf16 layer, the fused heads (halo-packed 3x3 32 -> 64 chained with the
    1x1 -> split + (48 - split) without ReLU, fp32, split in {4, 8, 12}), a bf16 NHWC input with H % 8 == 0, W % 32 == 0 and N H W < 2^27."""
    return (pa is not None and pb is not None and split in (4, 8, 12) and pa.w_layout == 1 and pa.ksize == 3 and pa.stride == 1 and pa.C0 == 32 and not pa.C1 and pa.Cout == 32
            and not pa.Cout2 and pa.epilogue == V2X_EPI_BF16 and pb.w_layout == 1 and pb.ksize == 3 and pb.stride == 1 and pb.C0 == 32 and not pb.C1
            and pb.Cout == 64 and pb.Cout2 == 48 and not pb.relu2 and pb.epilogue == V2X_EPI_F32 and x.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[3] == 32
            and x.shape[1] % 8 == 0 and x.shape[2] % 32 == 0 and x.shape[0] * x.shape[1] * x.shape[2] < (1 << 27) and tuning.get("TAIL_FUSE") != 0)


def conv2d_tail(pa, pb, x, split):
    """heads(conv8_2(x)) in one launch (conv_tail.hip through v2x_conv2d_pair's second form): x (N, H, W, 32) bf16 = conv8_1's output ->
    (cls (N, H, W, split), loc (N, H, W, 48 - split)) fp32, bit-identical to conv2d(pa) followed by conv2d(pb, split=split)."""
    lib = _lib.load()
    N, H, W, _ = x.shape
    out = torch.empty((N, H, W, split), dtype=torch.float32, device=x.device)
    out2 = torch.empty((N, H, W, pb.Cout2 - split), dtype=torch.float32, device=x.device)
    da, db = _conv_desc(pa, N, H, W), _conv_desc(pb, N, H, W)
    da.in0 = _dev(x, torch.bfloat16, "x").value
    db.out, db.out_cstride, db.out_coff = out.data_ptr(), split, 0
    db.out2, db.split, db.out2_cstride = out2.data_ptr(), split, out2.shape[3]
    prof = None
    if _launch.PROFILE is not None:
        M = N * H * W
        prof = _Prof("conv3x3_tail_kernel", 2.0 * M * (9 * 32 * 32 + 9 * 32 * 64 + 64 * 48), x.numel() * 2 + (out.numel() + out2.numel()) * 4 +
                     (pa.weight.numel() + pb.weight.numel() + pb.weight2.numel()) * 2, pa.name + "+" + pb.name)
    rc = lib.v2x_conv2d_pair(C.byref(da), C.byref(db), _stream())
    if prof is not None:
        prof.done()
    _lib.check(rc, "v2x_conv2d_pair(%s, %s)" % (pa.name, pb.name))
    return out, out2


def warp_fuse(feat, A, Bt, trans, items, coef, mode, out=None):
    """feat (A*Bt, H, W, C) bf16; trans (Bt, A, A, 4, 4) fp32; items (n_out, 2) int32; coef (n_out, A) fp32."""
    lib = _lib.load()
    n_items, H, W, Cc = feat.shape
    if n_items != A * Bt:
        raise ValueError("feat holds %d maps, expected A*Bt=%d" % (n_items, A * Bt))
    if tuple(trans.shape) != (Bt, A, A, 4, 4):
        raise ValueError("trans must be (Bt, A, A, 4, 4), got %s" % (tuple(trans.shape),))
    n_out = items.shape[0]
    if tuple(coef.shape) != (n_out, A):
        raise ValueError("coef must be (n_out, A)")
    if out is None:
        out = torch.empty((n_out, H, W, Cc), dtype=torch.bfloat16, device=feat.device)
    lds = H % 8 == 0 and W % 8 == 0 and Cc % 128 == 0 and tuning.get("WARP_LDS") != 0
    prof = _Prof(("warp_fuse_lds2_kernel<%d>" % mode if tuning.get("WARP_LDS") >= 2 else "warp_fuse_lds_kernel") if lds else "warp_fuse_kernel", 0,
                 (n_out * (A - 1) + n_out) * H * W * Cc * 2)
    order = _warp_frame_order(items, A, Bt) if (lds and tuning.get("WARP_XCD") != 0) else None
    if order is not None:
        rc = lib.v2x_warp_fuse_ordered(_dev(feat, torch.bfloat16, "feat"), A, Bt, H, W, Cc, _dev(trans, torch.float32, "trans"),
                                       _dev(items, torch.int32, "items"), n_out, _dev(coef, torch.float32, "coef"), mode,
                                       _dev(out, torch.bfloat16, "out"), _dev(order, torch.int32, "order"), A, order.numel(), _stream())
    else:
        rc = lib.v2x_warp_fuse(_dev(feat, torch.bfloat16, "feat"), A, Bt, H, W, Cc, _dev(trans, torch.float32, "trans"),
                               _dev(items, torch.int32, "items"), n_out, _dev(coef, torch.float32, "coef"), mode,
                               _dev(out, torch.bfloat16, "out"), _stream())
    prof.done()
    _lib.check(rc, "v2x_warp_fuse")
    return out


def channel_degrade(items, A, Bt, coef0, coef, coef2, link, trans, trans_out, p_outage, pose_sigma, seed, step):
    """This step's fusion plan and poses from the static plan and the clean poses, one launch: items (n_out, 2) int32;
    coef0 -> coef (n_out, A) fp32 (both None: pose noise alone); coef2 (n_out*A, A) fp32 or None; link (Bt, A, A) uint8 or None; trans ->
    trans_out (Bt, A, A, 4, 4) fp32 (trans_out None if and only if pose_sigma == 0); step: a one-element int64 / uint64 device tensor, read as the
    step s and left as s + 1.  Nothing synchronises with the host."""
    n_out = items.shape[0]
    if coef0 is not None and (tuple(coef0.shape) != (n_out, A) or tuple(coef.shape) != (n_out, A)):
        raise ValueError("coef0 and coef must be (n_out, A)")
    if coef2 is not None and tuple(coef2.shape) != (n_out * A, A):
        raise ValueError("coef2 must be (n_out * A, A)")
    if link is not None and tuple(link.shape) != (Bt, A, A):
        raise ValueError("link must be (Bt, A, A)")
    if trans_out is not None and (trans is None or tuple(trans.shape) != (Bt, A, A, 4, 4) or tuple(trans_out.shape) != (Bt, A, A, 4, 4)):
        raise ValueError("trans and trans_out must be (Bt, A, A, 4, 4)")
    if step.numel() != 1 or step.dtype not in (torch.int64, torch.uint64):
        raise ValueError("step must be one 64-bit integer in device memory")
    prof = _Prof("channel_degrade_kernel", 0, (2 * n_out * A + (n_out * A * A if coef2 is not None else 0)) * 4 + (2 * Bt * A * A * 64 if trans_out is not None else 0))
    rc = _lib.load().v2x_channel_degrade(_dev(items, torch.int32, "items"), n_out, A, Bt, _dev_opt(coef0, torch.float32, "coef0"), _dev_opt(coef, torch.float32, "coef"),
                                         _dev_opt(coef2, torch.float32, "coef2"), _dev_opt(link, torch.uint8, "link"),
                                         _dev_opt(trans if trans_out is not None else None, torch.float32, "trans"), _dev_opt(trans_out, torch.float32, "trans_out"),
                                         C.c_float(p_outage), C.c_float(pose_sigma), C.c_uint64(seed), _dev(step, step.dtype, "step"), _stream())
    prof.done()
    _lib.check(rc, "v2x_channel_degrade")


def items_tensor(items, A, Bt, device):
    """(n_out, 2) int32 device tensor of the (ego, frame) pairs of a fusion plan, with the frame-ordered table v2x_warp_fuse_ordered walks
    attached (built here on the host, where the list is: no device round trip later)."""
    t = torch.tensor(items, dtype=torch.int32, device=device).view(-1, 2)
    order = [-1] * (A * Bt)
    ok = True
    for m, (a, f) in enumerate(items):
        if not (0 <= a < A and 0 <= f < Bt) or order[f * A + a] >= 0:
            ok = False                       # outside the table, or listed twice: the plain grid
            break
        order[f * A + a] = m
    t._v2x_frame_order = (t._version, torch.tensor(order, dtype=torch.int32, device=device).view(Bt, A) if ok and len(items) else False)
    return t


def _warp_frame_order(items, A, Bt):
    """(Bt, A) int32 table: the output map of (frame, ego), -1 where there is none -- what v2x_warp_fuse_ordered walks so that the output maps
    of one frame (which all read the same A source maps) are computed by one XCD and share its L2.  Built once per items tensor (the fusion plan
    keeps it); never inside a hipGraph capture (the table would live in the graph's private pool): the caller then takes the unordered launch."""
    tag = getattr(items, "_v2x_frame_order", None)
    if tag is None or tag[0] != items._version:            # (a table built for other contents of this tensor is not trusted)
        if torch.cuda.is_current_stream_capturing():
            return None
        order = torch.full((Bt, A), -1, dtype=torch.int32, device=items.device)
        order[items[:, 1].long(), items[:, 0].long()] = torch.arange(items.shape[0], dtype=torch.int32, device=items.device)
        if int((order >= 0).sum()) != items.shape[0]:
            order = False                        # an (ego, frame) pair listed twice: the table cannot hold both -> the plain grid, always
        tag = (items._version, order)
        items._v2x_frame_order = tag
    return None if tag[1] is False else tag[1]


# ------------------------------------------------------------------ a5
ATTN_MODES = {"softmax": 0, "activated": 1, "argmax_test": 2}


ATTN_NORMS = {"softmax": 0, "sparsemax": 1}


def attn_handshake(keys, querys, w_lin, b_lin, A, Bt, mode, thres=0.2, norm="softmax"):
    """keys (A*Bt, K) fp32, querys (A*Bt, Q) fp32 -> prob, coef (Bt, A_key, A_query) fp32.  norm: how the scores of a query are
    normalised over the keys -- "softmax", or "sparsemax" (When2com(sparse=True): exact zeros outside the support)."""
    lib = _lib.load()
    K, Q = keys.shape[1], querys.shape[1]
    prob = torch.empty((Bt, A, A), dtype=torch.float32, device=keys.device)
    coef = torch.empty_like(prob)
    if ATTN_NORMS[norm] != 0:
        _lib.check(lib.v2x_attn_handshake_norm(_dev(keys, torch.float32, "keys"), _dev(querys, torch.float32, "querys"),
                                               _dev(w_lin, torch.float32, "w_lin"), _dev(b_lin, torch.float32, "b_lin"), A, Bt,
                                               K, Q, ATTN_MODES[mode], ATTN_NORMS[norm], C.c_float(thres), _dev(prob, torch.float32, "prob"),
                                               _dev(coef, torch.float32, "coef"), _stream()), "v2x_attn_handshake_norm")
        return prob, coef
    _lib.check(lib.v2x_attn_handshake(_dev(keys, torch.float32, "keys"), _dev(querys, torch.float32, "querys"),
                                      _dev(w_lin, torch.float32, "w_lin"), _dev(b_lin, torch.float32, "b_lin"), A, Bt,
                                      K, Q, ATTN_MODES[mode], C.c_float(thres), _dev(prob, torch.float32, "prob"),
                                      _dev(coef, torch.float32, "coef"), _stream()), "v2x_attn_handshake")
    return prob, coef


# ------------------------------------------------------------------ f-4 (DiscoNet)
def pixel_weighted_fuse(scores, valid, maps):
    """scores (n, A, H, W, S) fp32 (channel 0 used), valid (n, A) fp32, maps (n, A, H, W, C) bf16 -> (n, H, W, C) bf16."""
    lib = _lib.load()
    n, A, H, W, Cc = maps.shape
    out = torch.empty((n, H, W, Cc), dtype=torch.bfloat16, device=maps.device)
    _lib.check(lib.v2x_pixel_weighted_fuse(_dev(scores, torch.float32, "scores"), scores.shape[-1],
                                           _dev(valid, torch.float32, "valid"), _dev(maps, torch.bfloat16, "maps"), n, A, H, W,
                                           Cc, _dev(out, torch.bfloat16, "out"), _stream()), "v2x_pixel_weighted_fuse")
    return out


# ------------------------------------------------------------------ a8
def seg_argmax_confusion(logits, label=None, want_pred=True):
    """logits (n, H, W, n_cls) fp32 NHWC; label (n, H, W) uint8 -> (pred uint8, conf int64 [n_cls, n_cls])."""
    lib = _lib.load()
    n, H, W, ncls = logits.shape
    pred = torch.empty((n, H, W), dtype=torch.uint8, device=logits.device) if want_pred else None
    conf = torch.zeros((ncls, ncls), dtype=torch.int64, device=logits.device) if label is not None else None
    _lib.check(lib.v2x_seg_argmax_confusion(
        _dev(logits, torch.float32, "logits"), _dev(label, torch.uint8, "label") if label is not None else None,
        n, H, W, ncls, _dev(pred, torch.uint8, "pred") if pred is not None else None,
        _dev(conf, torch.int64, "conf") if conf is not None else None, _stream()), "v2x_seg_argmax_confusion")
    return pred, conf


# ------------------------------------------------------------------ layer = halo kernel when eligible, else gather kernel(s)
class Layer:
    """One logical layer (possibly a fused pair).  `halo` is the packing of the patch-based kernel family that
    covers the layer (conv_halo.hip, conv_stream*.hip) at the extents it tiles (covers()); `fallback` is the list
    of gather-kernel convs computing the same thing for any other extent.  `split` > 0: two output tensors."""

    __slots__ = ("halo", "fallback", "split", "name", "det", "latency")

    def __init__(self, fallback, halo=None, split=0, name=None, latency=None):
        self.fallback, self.halo, self.split = list(fallback), halo, split
        self.latency = latency   # a 9-tap streamed packing for DECLARED latency launches when `halo` is a form without split-K (the streamed parity-class kernel)
        self.det = None      # det heads only: the packing with the score threshold in the epilogue (packing.pack_heads_det)
        self.name = name or self.fallback[0].name


def _splitk_gate():
    """Launches with at least this many tiles are never split: 200 (measured, one-frame inference), or 5/8 of a latency_dispatch(target=...) block's target."""
    return max(200, (getattr(_latency, "target", 0) or tuning.get("SPLITK_TARGET")) * 5 // 8)


def small_batch_splitk(pc, N, H, W):
    """Latency mode (a declared latency launch: latency_launches() above): how many chunk ranges a streamed stride-1 layer is split into so
    that a launch has about one workgroup per CU.  One collaborative frame is 5 maps: a 32x32 layer with 256 output channels is then 40
    tiles of 256 pixels x 128 channels on 256 CUs, each walking all its chunks (conv5_1: 216 steps) -- 117 us for 18 GFLOP.  With the
    chunks divided over `splitk` workgroups per tile (partial sums added by splitk_reduce_kernel in range order) the same layer runs on
    ~240.  The mode is DECLARED by the caller, never derived from the batch inside a sharded runner: the split changes the fp32 summation
    order (one bf16 rounding of the output), and kernel selection that followed the item count would break the R-rank == 1-rank bitwise
    equality.  Asked of a packing that covers(pc, H, W): select() is the caller."""
    if pc.w_layout != 2 or pc.stride not in (1, 2) or not latency_launches():
        return 0
    rows = _lib.load().v2x_conv_stream_tile_rows(pc.Cout, pc.epilogue)
    if rows not in (64, 96, 128):
        return 0
    if pc.stride == 2:
        # the 1-tap stride-2 kernel (128 output pixels per workgroup): conv4_1 at one frame is 20-40 workgroups walking 8 chunks each (34 us);
        # conv1_1 (one chunk, resident form) and conv2_1 (two chunks) are never split
        if pc.C1 or pc.up0 or pc.Cout2 or pc.epilogue != V2X_EPI_BF16 or pc.w_rows != pc.Cout:
            return 0
        tiles = N * ((H // 2) * (W // 2) // 128) * (pc.Cout // rows)
        chunks, least = pc.C0 // 32, 8                            # (conv3_1, 4 chunks: two ranges + the reduce launch 21 us against 20 unsplit)
    else:
        # Measured (one frame = 5 maps / eight = 40, tools/layer_profile.py): a split pays when the unsplit launch has fewer than ~200 tiles
        # AND every range keeps >= 2 chunks (conv6_2, 4 chunks: 4 ranges of one 35 us vs 32 unsplit); the 4-wave kernel WITHOUT a split is slower
        # than the 8-wave forms even at 160 workgroups (conv5_1 at 40 maps: 163 vs 137 us), so there is no "more, smaller tiles" mode.
        if pc.Cout2:
            return 0
        tiles = N * (H * W // 256) * (pc.w_rows // rows)       # workgroups of the 4-wave form (256-pixel tiles)
        chunks, least = (pc.C0 + pc.C1) // 32, 4
    if tiles >= _splitk_gate() or chunks < least:
        return 0
    want = min(chunks // 2, -(-(getattr(_latency, "target", 0) or tuning.get("SPLITK_TARGET")) // tiles))
    while want > 1 and -(-chunks // want) * (want - 1) >= chunks:     # no empty range
        want -= 1
    return want if want > 1 else 0


def select(layer, N, H, W, bits=False):
    """-> (the packing run_layer launches for N maps of H x W, its splitk), or None: the gather fallback chain.  Which extents a kernel family
    tiles is the library's answer (covers); the policy is Python's: the bit grid (bits) goes only to a halo packing; inside a declared latency
    block `layer.latency` is taken when small_batch_splitk splits it; the streamed stride-1 forms (one 256-pixel tile per workgroup) run from
    256 pixels per map on.  That choice looks at the map extent only, never at the batch: kernel selection must not change with the number of
    items a rank owns, or R-rank results would stop being bitwise equal to 1-rank results."""
    h = layer.halo
    if bits:
        return (h, 0) if h is not None and h.w_layout == 1 and covers(h, H, W, True) else None
    lat = layer.latency
    if lat is not None and latency_launches() and covers(lat, H, W):
        sk = small_batch_splitk(lat, N, H, W)
        if sk > 1:
            return lat, sk
    if h is None or not covers(h, H, W) or (h.w_layout in (2, 4) and h.stride == 1 and H * W < 256):
        return None
    return h, small_batch_splitk(h, N, H, W)


def run_layer(layer, in0, in1=None, zbits=0):
    """zbits > 0: in0 is the voxelizer's int32 bit grid (N, H, W) -- only the first layer's halo packing reads it."""
    src = in0 if in1 is None else in1
    N, H, W = in0.shape[0], src.shape[1], src.shape[2]
    sel = select(layer, N, H, W, in0.dtype == torch.int32)
    if sel is None and in0.dtype == torch.int32:
        in0 = bits_to_nhwc(in0, zbits, layer.fallback[0].C0)  # no kernel reads the bit grid at this extent: expand, then as any bf16 map
        sel = select(layer, N, H, W)
    if sel is not None:
        return conv2d(sel[0], in0, in1, split=layer.split, zbits=zbits, splitk=sel[1])
    y = conv2d(layer.fallback[0], in0, in1, split=layer.split if len(layer.fallback) == 1 else 0)
    for i, pc in enumerate(layer.fallback[1:], 1):
        y = conv2d(pc, y, split=layer.split if i == len(layer.fallback) - 1 else 0)
    return y


# ------------------------------------------------------------------ rows f-1 and f-3 live in their own modules; `ops.<name>` keeps working
from .ops_post import assign_targets, assign_targets_sparse_keys, conv2d_det, det_map, det_nms_candidates, det_postprocess, late_fuse, match_detections, rotated_iou  # noqa: E402,F401
from .ops_seg import median_frequency_weights, pad_box_lists, rasterize_seg, seg_grid  # noqa: E402,F401
from .ops_lidar import box_rows, lidar_cast, ring_table, sensor_rows, visible_boxes  # noqa: E402,F401
from .ops_lidar import az_time_table, lidar_cast_moving, visible_boxes_moving  # noqa: E402,F401
from .ops_vis import freespace_bits, mask_unobserved, vis_maps  # noqa: E402,F401
from .ops_track import assign_iou, hota_sequences, mot_sequences, sort_step  # noqa: E402,F401
from .ops_train import (bn_train_backward, bn_train_forward, cast_pad_chsum, channel_sum, conv3x3_wgrad, det_loss_backward, det_loss_forward,  # noqa: E402,F401
                        det_corner_loss_backward, det_corner_loss_forward, gru_gates, gru_gates_backward, gru_gates_nhwc, gru_gates_nhwc_backward, gru_gates_nhwc_ok, upcat, upcat_backward, v2v_message,
                        seg_loss_backward, seg_loss_backward_packed, seg_loss_forward, seg_loss_shape_ok, v2v_message_backward, warp_affine, zero_insert)


# `ops.PROFILE = []` / `ops.PROFILE` (bench.py, tools/): one list for every wrapper module, kept in _launch
import sys as _sys  # noqa: E402
import types as _types  # noqa: E402


class _OpsModule(_types.ModuleType):
    @property
    def PROFILE(self):
        return _launch.PROFILE

    @PROFILE.setter
    def PROFILE(self, value):
        _launch.PROFILE = value


_sys.modules[__name__].__class__ = _OpsModule

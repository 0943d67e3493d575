"""The plan table of the inference convolutions, a runnable case for every row of it, and float64 references (csrc/conv_stream.hip,
conv_stream_pc.hip, conv_stream_s2.hip, conv_halo.hip, conv1x1.hip, conv_igemm.hip; the fused conv_halo_pair.hip and conv_tail.hip).  A plain
helper module (as tests/train_refs.py): tests/test_conv_plan_cpu.py asks the library for the kernel name of every TABLE row,
tests/test_conv_refs_cpu.py checks the references and the conditions the two input families must satisfy without a GPU,
tests/test_gpu_conv_sweep.py launches every case and holds the kernels to the references.

A layer is a list of STAGES (one for a plain layer, two for a 3x3 chained with a 1x1 or for the bit-grid pair, three for the detection tail).
A stage computes, in torch.float64 on the CPU and on the bf16 operands exactly as the kernel gets them (for w_layout 3 / 4 the packer's
pre-summed, once-rounded class weights): nearest x2 upsample of source 0 where up0, channel concat, k x k conv with zero padding at stride 1 or
2, acc * scale + shift, ReLU where the layer has it.  Between stages the hidden map is rounded ONCE to bf16 (train_refs.bf16r64).

Two input families:
  int   activations in {-1, 0, 1} ({0, 1} for the bit grid), weights k/16 with |k| <= 7, scale in {0.5, 1, 2}, shift a multiple of 1/16: every
        term and every partial sum is a multiple of one power of two and small enough that fp32 addition in ANY order is exact
        (int_exactness), so the kernel's output must equal the reference bit for bit (bf16 outputs: the reference rounded once).
  rand  N(0, 1) activations rounded to bf16, He-scaled weights, scale in [0.5, 1.5], shift N(0, 0.2), as tests/test_gpu_fuzz.py.  The bars are
        those of tests/test_gpu_train_sweep.py (rand_bars)."""
import contextlib
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

from train_refs import SMALL, TINY, bf16r, bf16r64, clear_of_bf16_ties, fp32_bar

F64 = torch.float64
PTR = 0x1000      # every tensor pointer of the table: non-null, 16-byte aligned, never dereferenced
BF16, F32, GRU, DET = 0, 1, 2, 3


def desc(**kw):
    """A v2x_conv_desc: 3x3 stride 1 pad 1, one map, plain bf16 epilogue unless the row says otherwise; w_rows / w_kpad / out_cstride as the packers would set them."""
    from v2x_sim_amd import _lib
    d = _lib.ConvDesc()
    f = dict(N=1, ksize=3, stride=1, pad=1, C1=0, up0=0, epilogue=BF16, relu=1, w_layout=0, Cout2=0)
    f.update(kw)
    lay, cin = f.get("w_layout", 0), f["C0"] + f["C1"]
    if "w_rows" not in f:
        need = 3 * f["Cout"] if f["epilogue"] == GRU else f["Cout"]
        rows = _lib.load().v2x_conv_tile_rows(f["Cout"], f["epilogue"]) if lay == 0 else 1
        f["w_rows"] = (need + rows - 1) // rows * rows
    if "w_kpad" not in f:
        f["w_kpad"] = (16 * f["C0"] + 9 * f["C1"]) if lay in (3, 4) else ((f["ksize"] ** 2 * cin + 63) // 64 * 64 if lay == 0 else 9 * cin)
    f.setdefault("out_cstride", f["Cout2"] or f["Cout"])
    for k in ("in0", "weight", "scale", "shift", "out"):
        f.setdefault(k, PTR)
    if f["C1"]:
        f.setdefault("in1", PTR)
    if f["Cout2"]:
        for k in ("weight2", "scale2", "shift2"):
            f.setdefault(k, PTR)
    if f.get("splitk", 0) > 1:
        f.setdefault("splitk_ws", PTR)
    if f["epilogue"] == DET:
        f.update(out2=PTR, out2_cstride=6, det_counts=PTR, det_cap=4096, det_thr=0.5, out_cstride=4096)
    for k, v in f.items():
        setattr(d, k, v)
    return d


def S(**kw):   # streamed layout
    return dict(w_layout=2, **kw)


def H(**kw):   # halo layout
    return dict(w_layout=1, **kw)


REDUCE, REDUCE_GRU = " + splitk_reduce_kernel<false>", " + splitk_reduce_kernel<true>"
# (expected name, switches, descriptor).  Rows marked DRIFT are the cases the retired Python copy of this dispatch got wrong.
TABLE = [
    # ---- conv_stream.hip: v2x_conv_stream_dispatch ------------------------------------------------------------------------------
    ("conv3x3_stream8q_kernel", {}, dict(w_layout=4, C0=128, C1=64, up0=1, Cout=64, H=16, W=64)),
    ("conv3x3_stream8p_kernel", {}, dict(w_layout=4, C0=256, C1=128, up0=1, Cout=128, H=16, W=32)),
    ("conv3x3_stream_kernel<96, 16, 16, 0, true>" + REDUCE_GRU, {}, S(C0=64, Cout=32, epilogue=GRU, H=16, W=16, splitk=2)),        # DRIFT (split-K labels)
    ("conv3x3_stream_kernel<96, 8, 32, 0, true>" + REDUCE_GRU, {}, S(C0=32, C1=32, Cout=64, epilogue=GRU, H=8, W=32, splitk=2)),
    ("conv3x3_stream_kernel<128, 16, 16, 0, true>" + REDUCE, {}, S(C0=128, Cout=128, H=16, W=16, splitk=4)),
    ("conv3x3_stream_kernel<128, 8, 32, 0, true>" + REDUCE, {}, S(C0=64, Cout=256, H=16, W=32, splitk=2)),
    ("conv3x3_stream_kernel<64, 16, 16, 0, true>" + REDUCE, {}, S(C0=64, Cout=64, H=16, W=16, splitk=2)),
    ("conv3x3_stream_kernel<64, 8, 32, 0, true>" + REDUCE, {}, S(C0=96, Cout=64, H=16, W=32, splitk=3)),
    ("conv3x3_stream8g_kernel<128, 0, true>", {}, S(C0=256, Cout=256, H=32, W=32, N=3)),
    ("conv3x3_stream8g_kernel<96, 2, true>", {"STREAM_WT": 2}, S(C0=256, C1=256, Cout=256, epilogue=GRU, H=32, W=32)),
    ("conv3x3_stream8g_kernel<96, 2, false>", {}, S(C0=256, C1=256, Cout=256, epilogue=GRU, H=32, W=32)),
    ("conv3x3_stream8_kernel<96, 2>", {"STREAM_G": 0}, S(C0=256, C1=256, Cout=256, epilogue=GRU, H=32, W=32)),
    ("conv3x3_stream8_kernel<96, 2>", {}, S(C0=32, Cout=32 * 257, epilogue=GRU, H=16, W=32)),          # DRIFT: three taps need n_co_tiles <= CUs
    ("conv3x3_stream8_kernel<128, 1>", {}, S(C0=128, Cout=128, Cout2=128, H=64, W=64, N=24)),            # chained, 192 tiles: a full launch
    ("conv3x3_stream_kernel<128, 8, 32, 1, false>", {}, S(C0=128, Cout=128, Cout2=128, H=64, W=64, N=5)),  # DRIFT: few_chain_tiles (160 x 4 < 3 x 256)
    ("conv3x3_stream8g_kernel<128, 0, false>", {"STREAM_WT": 0}, S(C0=128, Cout=128, H=16, W=32)),
    ("conv3x3_stream8_kernel<128, 0>", {"STREAM_G": 0}, S(C0=128, Cout=128, H=16, W=32)),
    ("conv3x3_stream8_kernel<128, 0>", {}, S(C0=32, Cout=128 * 257, H=16, W=32)),                        # DRIFT: n_co_tiles > CUs
    ("conv3x3_wide3_kernel<64>", {}, S(C0=128, C1=64, up0=1, Cout=64, H=32, W=64)),
    ("conv3x3_wide_kernel<64, 1>", {}, S(C0=64, Cout=64, Cout2=64, H=32, W=32)),
    ("conv3x3_wide_kernel<64, 0>", {}, S(C0=64, Cout=64, H=16, W=32)),
    ("conv3x3_wide_kernel<64, 0>", {"WIDE3": 0}, S(C0=128, C1=64, up0=1, Cout=64, H=32, W=64)),
    ("conv3x3_stream_kernel<128, 16, 16, 1, false>", {}, S(C0=128, Cout=128, Cout2=128, H=16, W=16)),
    ("conv3x3_stream_kernel<128, 8, 32, 1, false>", {}, S(C0=128, Cout=128, Cout2=128, H=8, W=32)),
    ("conv3x3_stream_kernel<64, 16, 16, 1, false>", {}, S(C0=64, Cout=64, Cout2=64, H=16, W=16)),
    ("conv3x3_stream_kernel<64, 8, 32, 1, false>", {}, S(C0=64, Cout=64, Cout2=64, H=8, W=32)),
    ("conv3x3_stream_kernel<96, 16, 16, 2, false>", {}, S(C0=256, C1=256, Cout=256, epilogue=GRU, H=16, W=16)),
    ("conv3x3_stream_kernel<96, 8, 32, 2, false>", {}, S(C0=256, C1=256, Cout=256, epilogue=GRU, H=8, W=32)),
    ("conv3x3_stream_kernel<128, 16, 16, 0, false>", {}, S(C0=512, Cout=512, H=16, W=16, N=2)),
    ("conv3x3_stream_kernel<128, 8, 32, 0, false>", {"STREAM_WAVES": 4}, S(C0=128, Cout=128, H=16, W=32)),
    ("conv3x3_stream_kernel<64, 16, 16, 0, false>", {}, S(C0=64, Cout=64, H=16, W=16)),
    ("conv3x3_stream_kernel<64, 8, 32, 0, false>", {"STREAM_WIDE": 0}, S(C0=128, C1=64, up0=1, Cout=64, H=16, W=32)),
    # ---- conv_stream_s2.hip: v2x_conv_stream_s2_dispatch ------------------------------------------------------------------------
    ("conv3x3_s2_stream_kernel<128, 8, 16, true>" + REDUCE, {}, S(stride=2, C0=256, Cout=512, H=32, W=32, splitk=4)),               # DRIFT (split-K labels)
    ("conv3x3_s2_stream_kernel<64, 8, 16, true>" + REDUCE, {}, S(stride=2, C0=64, Cout=64, H=16, W=32, splitk=2)),
    ("conv3x3_s2_stream_kernel<128, 4, 32, true>" + REDUCE, {}, S(stride=2, C0=64, Cout=128, H=24, W=128, splitk=2)),
    ("conv3x3_s2_stream_kernel<64, 4, 32, true>" + REDUCE, {}, S(stride=2, C0=64, Cout=64, H=8, W=64, splitk=2)),
    ("conv3x3_s2g_kernel<8, 32>", {}, S(stride=2, C0=64, Cout=128, H=32, W=128, N=2)),
    ("conv3x3_s2g_kernel<16, 16>", {}, S(stride=2, C0=256, Cout=512, H=32, W=32, N=2)),
    ("conv3x3_s2_stream_kernel<128, 4, 32, false>", {}, S(stride=2, C0=64, Cout=128, H=128, W=128, N=8, small_batch=1)),  # DRIFT: the fourth template argument
    ("conv3x3_s2_stream_kernel<128, 4, 32, false>", {"S2_G": 0}, S(stride=2, C0=64, Cout=128, H=32, W=128)),
    ("conv3x3_s2_stream_kernel<128, 8, 16, false>", {}, S(stride=2, C0=128, Cout=128, H=16, W=32)),
    ("conv3x3_s2_stream_kernel<64, 8, 16, false>", {}, S(stride=2, C0=32, Cout=64, H=32, W=32)),       # DRIFT: the 16 x 16 test comes before the resident-weights test
    ("conv3x3_s2_resident_kernel<64>", {}, S(stride=2, C0=32, Cout=64, H=16, W=64, N=3)),
    ("conv3x3_s2_stream_kernel<128, 4, 32, false>", {}, S(stride=2, C0=32, Cout=128, H=8, W=64)),
    ("conv3x3_s2_stream_kernel<64, 4, 32, false>", {}, S(stride=2, C0=64, Cout=64, H=8, W=64)),
    # ---- conv_halo.hip: v2x_conv_halo_dispatch ----------------------------------------------------------------------------------
    ("conv3x3_halo_sb_kernel<0, 32, 32, 0, 0, true>", {}, H(C0=32, Cout=32, H=8, W=32, in_format=1, in_zbits=13)),
    ("conv3x3_halo_sb_kernel<0, 32, 32, 0, 0, false>", {}, H(C0=32, Cout=32, H=8, W=32)),
    ("conv3x3_halo_ppc_kernel<64, 32, 32>", {}, dict(w_layout=3, C0=64, C1=32, up0=1, Cout=32, H=24, W=32, N=3)),
    ("conv3x3_halo_pp_kernel<64, 32, 32, 0>", {}, H(C0=64, C1=32, up0=1, Cout=32, H=16, W=32)),
    ("conv3x3_halo_kernel<64, 32, 32, 0, 0>", {}, H(C0=64, C1=32, up0=1, Cout=32, H=24, W=32, N=3)),   # DRIFT: conv8_1, odd tile count
    ("conv3x3_halo_kernel<64, 32, 32, 0, 0>", {"HALO_PP": 0}, H(C0=64, C1=32, up0=1, Cout=32, H=16, W=32)),
    ("conv3x3_halo_pp_kernel<0, 64, 64, 0>", {}, H(C0=64, Cout=64, H=16, W=32)),
    ("conv3x3_halo_kernel<0, 64, 64, 0, 0>", {}, H(C0=64, Cout=64, H=40, W=96, N=3)),                   # DRIFT: conv7_2, odd tile count
    ("conv3x3_halo_pp_kernel<0, 64, 64, 64>", {}, H(C0=64, Cout=64, Cout2=64, H=24, W=32, N=4)),
    ("conv3x3_halo_kernel<0, 64, 64, 64, 1>", {}, H(C0=64, Cout=64, Cout2=64, H=24, W=32, N=3)),        # DRIFT: the chained layer, odd tile count
    ("conv3x3_halo_kernel<0, 64, 32, 0, 0>", {}, H(C0=64, Cout=32, H=8, W=32)),
    ("conv3x3_halo_kernel<0, 32, 64, 0, 0>", {}, H(C0=32, Cout=64, H=8, W=32)),
    ("conv3x3_halo_kernel<0, 32, 64, 48, 2>", {}, H(C0=32, Cout=64, Cout2=48, epilogue=F32, H=8, W=32)),
    ("conv3x3_halo_kernel<0, 32, 32, 16, 2>", {}, H(C0=32, Cout=32, Cout2=8, epilogue=F32, H=8, W=32)),
    ("conv3x3_halo_kernel<0, 32, 64, 64, 3>", {}, H(C0=32, Cout=64, Cout2=64, epilogue=DET, H=8, W=32)),   # DRIFT: the DET epilogue
    # ---- conv1x1.hip: v2x_conv1x1_dispatch (every channel-tile count, every chunk count, both epilogues) --------------------------
    ("conv1x1_stream_kernel<1, 1, false, 4>", {}, dict(ksize=1, pad=0, C0=32, Cout=16, H=8, W=8)),
    ("conv1x1_stream_kernel<2, 2, true, 4>", {}, dict(ksize=1, pad=0, C0=64, Cout=32, epilogue=F32, H=8, W=8)),
    ("conv1x1_stream_kernel<4, 3, false, 4>", {}, dict(ksize=1, pad=0, C0=128, Cout=48, H=8, W=8)),
    ("conv1x1_stream_kernel<1, 4, true, 4>", {}, dict(ksize=1, pad=0, C0=32, Cout=64, epilogue=F32, H=8, W=8)),
    ("conv1x1_stream_kernel<2, 6, false, 4>", {}, dict(ksize=1, pad=0, C0=64, Cout=96, H=8, W=8)),
    ("conv1x1_stream_kernel<4, 8, false, 2>", {}, dict(ksize=1, pad=0, C0=128, Cout=128, H=8, W=8)),
    ("conv1x1_stream_kernel<2, 8, true, 2>", {}, dict(ksize=1, pad=0, C0=64, Cout=128, epilogue=F32, H=8, W=8)),
    ("conv1x1_stream_kernel<1, 1, true, 4>", {}, dict(ksize=1, pad=0, C0=32, Cout=4, epilogue=F32, H=8, W=8)),
    ("conv1x1_stream_kernel<4, 4, true, 2>", {}, dict(ksize=1, pad=0, C0=128, Cout=64, epilogue=F32, H=8, W=8)),
    # ---- conv_igemm.hip: the gather tail of v2x_conv2d --------------------------------------------------------------------------
    ("conv_igemm_kernel<96, 128, 2, 2, 2>", {}, dict(C0=64, C1=64, Cout=64, epilogue=GRU, H=8, W=8)),
    ("conv_igemm_kernel<32, 256, 1, 4, 1>", {}, dict(C0=32, Cout=12, epilogue=F32, H=8, W=8)),
    ("conv_igemm_kernel<48, 256, 1, 4, 1>", {}, dict(C0=32, Cout=48, epilogue=F32, H=8, W=8)),
    ("conv_igemm_kernel<64, 128, 2, 2, 1>", {}, dict(C0=32, Cout=64, epilogue=F32, H=8, W=8)),
    ("conv_igemm_kernel<128, 128, 2, 2, 1>", {}, dict(C0=32, Cout=96, epilogue=F32, H=8, W=8)),
    ("conv_igemm_kernel<32, 256, 1, 4, 0>", {}, dict(C0=16, Cout=32, stride=2, H=9, W=7)),
    ("conv_igemm_kernel<48, 256, 1, 4, 0>", {}, dict(C0=32, Cout=40, H=8, W=8)),
    ("conv_igemm_kernel<64, 128, 2, 2, 0>", {}, dict(C0=64, C1=32, up0=1, Cout=64, H=8, W=8)),
    ("conv_igemm_kernel<128, 128, 2, 2, 0>", {}, dict(C0=32, Cout=256, H=8, W=8)),
    ("conv_igemm_kernel<64, 128, 2, 2, 0>", {"CONV1X1": 0}, dict(ksize=1, pad=0, C0=64, Cout=64, H=8, W=8)),
    ("conv_igemm_kernel<128, 128, 2, 2, 0>", {}, dict(ksize=1, pad=0, C0=96, Cout=128, H=8, W=8)),      # three chunks: not a shape of the streaming 1x1 kernel
]

# shapes v2x_conv2d refuses: by its validation, and by each dispatch function's "not mine"
REJECTED = [
    S(C0=128, Cout=128, H=7, W=32),                          # not tileable
    S(C0=128, Cout=128, H=16, W=32, splitk=8),               # more splits than chunks
    S(C0=48, Cout=128, H=16, W=32),                          # C0 % 32
    S(C0=128, Cout=96, H=16, W=32),                          # no row tile for this Cout
    S(stride=2, C0=64, Cout=128, H=8, W=48),                 # stride 2: no tiling
    S(stride=2, C0=64, C1=64, Cout=128, H=8, W=64),          # stride 2: one source only
    H(C0=96, Cout=32, H=8, W=32),                            # no halo instantiation
    H(C0=32, Cout=32, H=12, W=32),                           # H % 8
    H(C0=64, Cout=64, H=8, W=32, in_format=1, in_zbits=13),  # bit-grid input exists for 32 -> 32 only
    dict(w_layout=3, C0=128, C1=32, up0=1, Cout=32, H=8, W=32),
    dict(w_layout=4, C0=128, C1=64, up0=1, Cout=64, H=16, W=32),
    dict(C0=12, Cout=32, H=8, W=8),                          # gather: C0 % 8
    dict(C0=32, Cout=32, H=8, W=8, w_kpad=100),
    dict(C0=32, Cout=32, H=4096, W=4096),                    # 24-bit row arithmetic
    dict(C0=32, Cout=32, H=8, W=8, epilogue=DET),
]


# ====================================================================================================== the runnable cases
# One ConvCase per TABLE row.  `fields` / `switches` are the row's own unless the packers cannot build it: then they are the replacement, and
# `note` says what was replaced and why.  `same_as`: the replacement is exactly another row's case (it is run once, under that row).
ConvCase = namedtuple("ConvCase", "row name switches fields same_as note")

# kernel forms the sweep does not launch (name -> reason); at most the DET form and three others
NOT_RUN = {
    "conv3x3_halo_kernel<0, 32, 64, 64, 3>": "V2X_EPI_DET: the thresholded candidate epilogue, held bit for bit to the logits path by tests/test_gpu_postprocess.py",
}


def _cases():
    out, first = [], {}
    for row, (name, switches, fields) in enumerate(TABLE):
        f, sw, note = dict(fields), dict(switches), ""
        if name in NOT_RUN:
            out.append(ConvCase(row, name, sw, f, None, "not run: " + NOT_RUN[name]))
            continue
        if f.get("epilogue") == GRU and f["Cout"] == 32 * 257:
            # 257 channel tiles of a GRU with 8 224 hidden channels: the float64 oracle cell would hold a 8 224 -> 24 672 channel 3x3 W_hh
            # (1.8e9 weights).  The same kernel form is reached with STREAM_G = 0 on the network's own GRU shape.
            note = "replaces S(C0=32, Cout=32 * 257, GRU, 16 x 32): the oracle cell of that width cannot be built; same name through STREAM_G = 0"
            sw, f = {"STREAM_G": 0}, S(C0=256, C1=256, Cout=256, epilogue=GRU, H=32, W=32)
        key = (name, tuple(sorted(sw.items())), tuple(sorted(f.items())))
        out.append(ConvCase(row, name, sw, f, first.get(key), note))
        first.setdefault(key, row)
    return out


CONV_CASES = _cases()
RUN_CASES = [c for c in CONV_CASES if c.name not in NOT_RUN and c.same_as is None]
# the two fused launches (ops.conv2d_pair on the bit grid: conv_halo_pair.hip; ops.conv2d_tail: conv_tail.hip) at the smallest shapes of their own tests
FUSED_CASES = [("pair", 1, 8, 32), ("pair", 2, 40, 96), ("tail", 1, 8, 32), ("tail", 2, 40, 96)]
ZBITS = 13
TAIL_SPLIT = 12


def case_id(c):
    f = c.fields
    sw = "".join("-%s%d" % kv for kv in sorted(c.switches.items()))
    return "r%02d-%s%s" % (c.row, c.name.split(" + ")[0].replace("conv3x3_", "").replace("_kernel", "").replace(" ", ""), sw) + \
        "-%dx%dx%d" % (f.get("N", 1), f["H"], f["W"])


def is_gru(c):
    return c.fields.get("epilogue") == GRU


def families(c):
    """GRU rows have no int family: their gates are transcendental."""
    return ("rand",) if is_gru(c) else ("int", "rand")


# ====================================================================================================== stages and their float64 evaluation
class Stage:
    """One conv + scale / shift (+ ReLU).  w [Cout][Cin][k][k] fp32 holding bf16 values; for the parity-class layouts `wc` holds the pre-summed,
    once-rounded class weights [4][4][Cout][C0] of the upsampled source and w only the skip source's [Cout][C1][3][3]."""

    def __init__(self, w, scale, shift, relu, stride=1, pad=1, up0=0, C0=None, wc=None):
        self.w, self.scale, self.shift, self.relu, self.stride, self.pad, self.up0, self.wc = w, scale, shift, bool(relu), stride, pad, up0, wc
        self.C0 = C0


def stage_lin(st, x0, x1, dt, absolute=False):
    """The linear part of a stage in dtype dt: x0 (N, C0, H >> up0, W >> up0), x1 (N, C1, H, W) or None -> acc (N, Cout, Ho, Wo).
    absolute: sum of |term| instead (the int family's exactness condition)."""
    prep = (lambda t: t.to(dt).abs()) if absolute else (lambda t: t.to(dt))
    if st.wc is not None:
        cout, c0 = st.wc.shape[2], st.wc.shape[3]
        y = F.conv2d(prep(x1), prep(st.w), None, 1, 1)
        n, _, hs, ws = x0.shape
        xp = F.pad(prep(x0), (1, 1, 1, 1))
        wc = prep(st.wc)
        for py in range(2):
            for px in range(2):
                k = wc[py * 2 + px].view(2, 2, cout, c0).permute(2, 3, 0, 1).contiguous()      # [Cout][C0][a][b]
                full = F.conv2d(xp, k)                                                         # (hs + 1) x (ws + 1) positions
                y[:, :, py::2, px::2] += full[:, :, py:py + hs, px:px + ws]
        return y
    x = prep(x0)
    if st.up0:
        x = F.interpolate(x, scale_factor=(2, 2))
    if x1 is not None:
        x = torch.cat((x, prep(x1)), 1)
    return F.conv2d(x, prep(st.w), None, st.stride, st.pad)


def stage_pre(st, x0, x1, dt):
    """acc * scale + shift, before the ReLU."""
    return stage_lin(st, x0, x1, dt) * st.scale.to(dt).view(1, -1, 1, 1) + st.shift.to(dt).view(1, -1, 1, 1)


def layer_ref(stages, x0, x1, dt=F64):
    """The whole layer in dtype dt (float64: the reference; float32: torch's own evaluation): -> the last stage's output, unrounded.  The hidden
    maps between stages are rounded once to bf16."""
    h0, h1 = x0, x1
    for i, st in enumerate(stages):
        y = stage_pre(st, h0, h1, dt)
        if st.relu:
            y = F.relu(y)
        if i + 1 < len(stages):
            h0, h1 = bf16r64(y).to(dt), None
    return y


def bits_to_channels(bits, zbits):
    """(N, H, W) int32 bit words -> (N, zbits, H, W) fp32 of 0 / 1: channel z is bit z."""
    z = torch.arange(zbits, dtype=torch.int32).view(1, -1, 1, 1)
    return ((bits.unsqueeze(1) >> z) & 1).float()


# ====================================================================================================== operands
def int_weight(cout, cin, k, salt=0):
    """k/16 with integer |k| <= 7, a fixed function of (output channel, input channel, tap) that differs between neighbours in every dimension."""
    o = torch.arange(cout).view(-1, 1, 1)
    c = torch.arange(cin).view(1, -1, 1)
    t = torch.arange(k * k).view(1, 1, -1)
    return (((131 * o + 31 * c + 7 * t + 5 * salt) % 15 - 7).float() / 16).view(cout, cin, k, k)


def int_scale_shift(cout, salt=0):
    o = torch.arange(cout)
    return torch.tensor([0.5, 1.0, 2.0])[(o + salt) % 3], ((o * 37 + 11 + 7 * salt) % 65 - 32).float() / 16


INT_DENSITY = 0.5      # share of non-zero activations of the int family (and of set bits of the bit grid); tests/test_conv_refs_cpu.py checks
                       # int_exactness for every case at its density
TAIL_INT_DENSITY = 0.125   # the three-stage tail: the third stage's terms are multiples of 2^-14, so its sums have to stay smaller (at 0.5 the
                           # epilogue of the 1x1 reaches 1.7 x 2^24 quanta)


def _acts(g, shape, family, density=INT_DENSITY):
    if family == "int":
        return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float() * (torch.rand(shape, generator=g) < density).float()
    return bf16r(torch.randn(shape, generator=g))


def _bits(g, shape, family):
    p = INT_DENSITY if family == "int" else 0.3
    word = torch.zeros(shape, dtype=torch.int32)
    for z in range(ZBITS):
        word |= (torch.rand(shape, generator=g) < p).to(torch.int32) << z
    return word


def _params(g, cout, cin, k, family, salt=0):
    if family == "int":
        return (int_weight(cout, cin, k, salt),) + int_scale_shift(cout, salt)
    w = bf16r(torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5)
    return w, torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2


class Built:
    """One case with operands: x0, x1 (NCHW fp32 holding bf16 values; x0 the expanded 0 / 1 channels for a bit grid), bits, stages, `pack(device)`
    -> the PackedConv(s), and for GRU rows `cell` (the oracle cell in float64 on the bf16 weights)."""
    x1 = bits = cell = None
    splitk = 0
    small_batch = False


def _single_stage(f, g, family):
    from v2x_sim_amd import packing
    lay, C0, C1, cout, k = f.get("w_layout", 0), f["C0"], f.get("C1", 0), f["Cout"], f.get("ksize", 3)
    stride, pad, up0, epi, cout2 = f.get("stride", 1), f.get("pad", 1), f.get("up0", 0), f.get("epilogue", BF16), f.get("Cout2", 0)
    bits = f.get("in_format", 0) == 1
    cin = ZBITS if bits else C0 + C1
    w, s, t = _params(g, cout, cin, k, family)
    chain, st2 = None, None
    if cout2:
        relu2 = epi != F32                     # the fp32 chained forms are the heads: no ReLU behind the 1x1
        w2, s2, t2 = _params(g, cout2, cout, 1, family, salt=1)
        chain, st2 = (w2, s2, t2, relu2), Stage(w2, s2, t2, relu2, 1, 0)
    if lay in (3, 4):
        wc = bf16r(packing.parity_class_weights(w[:, :C0]))
        st = Stage(w[:, C0:].contiguous(), s, t, True, 1, 1, 1, C0, wc)
    else:
        st = Stage(w, s, t, True, stride, pad, up0, C0)

    def pack(device):
        if lay == 0:
            return packing.pack_conv("t", w, s, t, stride=stride, pad=pad, C0=C0, C1=C1, up0=up0, relu=True, epilogue=epi, device=device)
        if lay == 1:
            return packing.pack_conv_halo("t", w, s, t, C0=C0, C1=C1, relu=True, cin_pad=32 if bits else None, chain=chain, epilogue=epi, device=device)
        if lay == 2:
            return packing.pack_conv_stream("t", w, s, t, C0=C0, C1=C1, up0=up0, relu=True, chain=chain, stride=stride, device=device)
        if lay == 3:
            return packing.pack_conv_halo_parity("t", w, s, t, C0=C0, C1=C1, device=device)
        return packing.pack_conv_stream_parity("t", w, s, t, C0=C0, C1=C1, device=device)
    return [st] + ([st2] if st2 else []), pack


def _draw(c, family, attempt):
    from oracle import coperception_ref as R
    from v2x_sim_amd import packing
    f = c.fields
    g = torch.Generator().manual_seed(1000 * c.row + (17 if family == "int" else 29) + 7919 * attempt)
    b = Built()
    N, Hh, Ww, C0, C1, up0 = f.get("N", 1), f["H"], f["W"], f["C0"], f.get("C1", 0), f.get("up0", 0)
    b.N, b.H, b.W, b.splitk, b.small_batch = N, Hh, Ww, f.get("splitk", 0), bool(f.get("small_batch", 0))
    b.f32 = f.get("epilogue", BF16) == F32
    if f.get("in_format", 0) == 1:
        b.bits = _bits(g, (N, Hh, Ww), family)
        b.x0 = bits_to_channels(b.bits, ZBITS)
    else:
        b.x0 = _acts(g, (N, C0, Hh >> up0, Ww >> up0), family)
        if C1:
            b.x1 = _acts(g, (N, C1, Hh, Ww), family)
    if is_gru(c):
        cell = R.Conv2dGRUCell(C0 + C1, f["Cout"], 3)
        with torch.no_grad():
            for p in cell.parameters():
                lim = 1.0 / f["Cout"] ** 0.5
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * lim)
            cell.weight_ih_l0.copy_(bf16r(cell.weight_ih_l0))
        packer = packing.pack_gru_stream if f.get("w_layout", 0) == 2 else packing.pack_gru
        b.pack = lambda device: packer("gru", cell.weight_ih_l0, cell.bias_ih_l0, cell.bias_hh_l0, C0=C0, C1=C1, device=device)
        b.cell, b.stages = cell.double(), []
    else:
        b.stages, b.pack = _single_stage(f, g, family)
    return b


def _draw_fused(kind, N, Hh, Ww, family, attempt):
    from v2x_sim_amd import packing
    g = torch.Generator().manual_seed(N * 100 + Hh + (3 if kind == "pair" else 5) + (17 if family == "int" else 29) + 7919 * attempt)
    b = Built()
    b.N, b.H, b.W = N, Hh, Ww
    b.f32 = kind == "tail"
    if kind == "pair":
        b.bits = _bits(g, (N, Hh, Ww), family)
        b.x0 = bits_to_channels(b.bits, ZBITS)
        wa, sa, ta = _params(g, 32, ZBITS, 3, family)
        wb, sb, tb = _params(g, 32, 32, 3, family, salt=1)
        b.stages = [Stage(wa, sa, ta, True), Stage(wb, sb, tb, True)]
        b.pack = lambda device: (packing.pack_conv_halo("a", wa, sa, ta, C0=32, cin_pad=32, device=device),
                                 packing.pack_conv_halo("b", wb, sb, tb, C0=32, device=device))
    else:
        b.x0 = F.relu(_acts(g, (N, 32, Hh, Ww), family)) if family == "rand" else _acts(g, (N, 32, Hh, Ww), family, TAIL_INT_DENSITY)
        wa, sa, ta = _params(g, 32, 32, 3, family)
        wb, sb, tb = _params(g, 64, 32, 3, family, salt=1)
        w2, s2, t2 = _params(g, 48, 64, 1, family, salt=2)
        b.stages = [Stage(wa, sa, ta, True), Stage(wb, sb, tb, True), Stage(w2, s2, t2, False, 1, 0)]
        b.pack = lambda device: (packing.pack_conv_halo("a", wa, sa, ta, C0=32, device=device),
                                 packing.pack_conv_halo("b", wb, sb, tb, C0=32, chain=(w2, s2, t2, False), epilogue=F32, device=device))
    return b


def ref_maps(b):
    """The maps the rand family checks against float64: all of them, or the first and the last of a case with many large maps."""
    return list(range(b.N)) if b.N * b.H * b.W <= 5 * 64 * 64 else [0, b.N - 1]


def _sub(b, maps):
    return b.x0[maps], (None if b.x1 is None else b.x1[maps])


def gru_ref(b, maps):
    """The oracle's Conv2dGRUCell in float64 (emulation off) on the bf16 input and the bf16 W_ih."""
    x0, x1 = _sub(b, maps)
    x = x0 if x1 is None else torch.cat((x0, x1), 1)
    with torch.no_grad():
        return b.cell(x.to(F64), None, emulate=False)


def _finish_rand(b):
    """float64 reference and bars of a rand case on ref_maps(b); -> False when a small case has to be drawn again (TINY: a bf16 tie, SMALL: the kink)."""
    b.maps = ref_maps(b)
    if b.cell is not None:
        b.ref = gru_ref(b, b.maps)
        return True
    x0, x1 = _sub(b, b.maps)
    b.bars = rand_bars(b.stages, x0, x1)
    b.ref = b.bars["ref"]
    n = b.ref.numel()
    if n < SMALL and b.stages[-1].relu and bool(b.bars["kink"].any()):
        return False
    if n < TINY and not b.f32 and not clear_of_bf16_ties(b.ref):
        return False
    if len(b.stages) > 1 and not b.f32 and b.bars["kept_pixels"] < KEPT_MIN:
        return False
    return True


@functools.lru_cache(maxsize=2)
def build(row, family):
    """The case of TABLE row `row` with operands of `family`; rand cases also carry the float64 reference (`ref`, on `maps`) and the bars."""
    c = CONV_CASES[row]
    for attempt in range(200):
        b = _draw(c, family, attempt)
        if family == "int" or _finish_rand(b):
            b.attempt = attempt
            return b
    raise AssertionError("no clear draw for row %d" % row)


@functools.lru_cache(maxsize=2)
def build_fused(kind, N, Hh, Ww, family):
    for attempt in range(200):
        b = _draw_fused(kind, N, Hh, Ww, family, attempt)
        if family == "int" or _finish_rand(b):
            b.attempt = attempt
            return b
    raise AssertionError("no clear draw")


def int_ref(b, big=1 << 31):
    """The exact answer of an int case over every map.  Evaluated in float64, or -- for a case of more than `big` multiply-adds -- in fp32, which
    tests/test_conv_refs_cpu.py shows equal bit for bit there (int_exactness)."""
    st = b.stages[0]
    cin_taps = (st.w.shape[1] * st.w.shape[2] * st.w.shape[3]) + (16 * st.wc.shape[3] if st.wc is not None else 0)
    macs = b.N * b.H * b.W // (st.stride ** 2) * st.w.shape[0] * cin_taps
    return layer_ref(b.stages, b.x0, b.x1, torch.float32 if macs > big else F64).to(F64)


# ====================================================================================================== the int family's exactness condition
def quantum(v):
    """The largest power of two (<= 1) that divides every element of v."""
    v = v.to(F64)
    q = 1.0
    while not bool((v / q == torch.round(v / q)).all()):
        q /= 2
        assert q > 2.0 ** -40
    return q


def int_exactness(b, dt=F64):
    """Per stage: (worst sum of |term| / quantum of the terms, worst (sum of |term| * |scale| + |shift|) / quantum of the result, worst sum of
    |term|).  Every partial sum of a stage is a multiple of its quantum and at most the sum of |term|: while the first two stay below 2^24, fp32
    addition in any order, the multiplication by a power-of-two scale and the addition of the shift (fused or not) are all exact.
    dt = torch.float32 evaluates the sums of a large case in fp32: sums of non-negative multiples of one quantum, exact themselves while they stay
    below 2^24 quanta and never smaller than half the true sum otherwise."""
    out, h0, h1 = [], b.x0, b.x1
    for i, st in enumerate(b.stages):
        wq = min(quantum(st.w), quantum(st.wc) if st.wc is not None else 1.0)
        xq = min(quantum(h0), quantum(h1) if h1 is not None else 1.0)
        sabs = stage_lin(st, h0, h1, dt, absolute=True).to(F64)
        qacc = wq * xq
        qpre = min(qacc * quantum(st.scale), quantum(st.shift))
        pre_abs = sabs * st.scale.abs().double().view(1, -1, 1, 1) + st.shift.abs().double().view(1, -1, 1, 1)
        out.append((float(sabs.max()) / qacc, float(pre_abs.max()) / qpre, float(sabs.max())))
        y = stage_pre(st, h0, h1, dt).to(F64)
        if st.relu:
            y = F.relu(y)
        if i + 1 < len(b.stages):
            h0, h1 = bf16r64(y), None
    return out


# ====================================================================================================== the rand family's bars
FLIP_MAX, KINK_MAX = 1e-3, 1e-4          # per case, as tests/test_gpu_train_sweep.py; tests/test_conv_refs_cpu.py keeps the reference alone at half of each
KEPT_MIN = 0.5                           # a chained case with a bf16 output is drawn until at least this share of its pixels reads no hidden value that may
                                         # round the other way (float64 and torch's fp32 only: nothing of the kernel enters the choice of the draw)
KINK = 1e-5                              # |acc * scale + shift| below which a ReLU output is exempt from the flip count


def bf16_step(x):
    """One bf16 step at each element's magnitude (float64)."""
    a = x.to(F64).abs()
    _, e = torch.frexp(a)
    return torch.where(a == 0, torch.zeros_like(a), torch.ldexp(torch.ones_like(a), e - 8))


def tie_distance(x):
    """Distance of each element to the nearest midpoint between two bf16 neighbours."""
    a = x.to(F64).abs()
    q = bf16_step(a)
    t = torch.where(q > 0, a / torch.where(q > 0, q, torch.ones_like(q)), torch.zeros_like(a))
    return torch.where(q > 0, ((t - torch.floor(t)) - 0.5).abs() * q, torch.full_like(a, float("inf")))


def rand_bars(stages, x0, x1):
    """float64 reference of a rand case and what its bars need.  Stage by stage, on the float64 path's own (rounded) hidden map:
      alone_i  the worst error of torch's fp32 evaluation of stage i against float64 (the reference-alone error);
      P_i      a bound of the error of the kernel's hidden value BEFORE its rounding: 4 alone_i + sum |w_i scale_i| R_(i-1);
      R_i      how far the ROUNDED hidden value may legitimately differ: 0 where the float64 value lies farther than P_i from every bf16 tie and from
               the ReLU kink (no midpoint inside [h - P_i, h + P_i]: both round to the same value); elsewhere P_i + one bf16 step at |h| + P_i
               (|round(h') - round(h)| <= |h' - h| + two half steps).  For a hidden value of ordinary size P_i is far below its step and this is the
               one step of the first-order rule; a hidden value close to zero has steps BELOW P_i, and there the P_i term is the larger one.
    The last stage's bar is widened by `widen` = sum |w scale| R of the hidden values it reads (zero for a plain layer), and rounding flips are
    counted only over outputs that read no such value (`clean`).
    -> dict(ref, ref32, bar32, alone [per stage], widen, clean, kink, kept_pixels)"""
    h0, h1, R = x0, x1, None
    alone, out = [], {}
    for i, st in enumerate(stages):
        pre = stage_pre(st, h0, h1, F64)
        pre32 = stage_pre(st, h0, h1, torch.float32).to(F64)
        act, act32 = (F.relu(pre), F.relu(pre32)) if st.relu else (pre, pre32)
        alone.append(float((act32 - act).abs().max()))
        sw = (st.w.double().abs() * st.scale.double().abs().view(-1, 1, 1, 1))
        widen = F.conv2d(R, sw, None, st.stride, st.pad) if R is not None else torch.zeros_like(pre)
        if i + 1 == len(stages):
            bar32, _ = fp32_bar(act, act32)
            out.update(ref=act, ref32=act32, bar32=bar32, widen=widen, clean=widen == 0,
                       kink=(pre.abs() < KINK) if st.relu else torch.zeros_like(pre, dtype=torch.bool))
            break
        P = 4 * alone[-1] + widen
        near_tie = tie_distance(act) < P
        near_kink = (pre.abs() < P) if st.relu else torch.zeros_like(near_tie)
        R = (near_tie | near_kink).double() * (P + bf16_step(act.abs() + P))
        h0, h1 = bf16r64(act), None
    out["alone"] = alone
    out["kept_pixels"] = float(out["clean"].all(1).double().mean())
    return out


def bf16_bar(bars):
    """Per element: half a bf16 step + 4 x the reference-alone fp32 error of the case (floor one fp32 ulp) + the widening.  The half step is the one
    at the magnitude of the value the kernel ROUNDS, which may lie bar32 + widen above the reference: past a power of two the step doubles (for a
    plain layer that slack is a few 1e-6 and moves the half step only for a reference within that of a power of two)."""
    slack = bars["bar32"] + bars["widen"]
    return bf16_step(bars["ref"].abs() + slack) / 2 + slack


def bf16_excess(got64, bars):
    """Worst (error - half a bf16 step - widening) / fp32 bar: the part of the 4 x reference-alone allowance a bf16 output uses (<= 0: none)."""
    slack = bars["bar32"] + bars["widen"]
    return float((((got64 - bars["ref"]).abs() - bf16_step(bars["ref"].abs() + slack) / 2 - bars["widen"]) / bars["bar32"]).max())


def flip_kink_shares(got64, bars):
    """-> (share of the clean, off-kink elements whose bf16 value differs from the float64 reference rounded once; share of exempted kink elements)."""
    count = bars["clean"] & ~bars["kink"]
    flips = ((got64 != bf16r64(bars["ref"])) & count).double().sum() / max(int(count.sum()), 1)
    return float(flips), float(bars["kink"].double().mean())


def gru_bar(ref):
    """The expression of tests/test_gpu_stream.py::test_gru_gate_arithmetic_over_its_whole_range, per element."""
    return 2 ** -7 * max(float(ref.abs().max()), 1e-6) + 2 ** -7 * ref.abs()


def latency(b):
    from v2x_sim_amd import ops
    return ops.latency_dispatch() if b.small_batch else contextlib.nullcontext()

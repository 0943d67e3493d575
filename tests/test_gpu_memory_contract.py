"""Every kernel-launching wrapper held to the memory half of its contract (include/v2x_amd.h): it writes all of its outputs, writes only
its outputs, and reads nothing it was not given.  tests/guarded_alloc.py serves the wrappers' torch.empty / empty_like / zeros / full from
poisoned buffers with 4096 guard bytes on either side; every input and in/out operand is copied into such a buffer too.

One table (ROWS), one row per wrapper; tests/test_guarded_alloc_cpu.py checks that every public function of the six wrapper modules is a row
here or launches nothing.  The cases are the first, smallest entries of the case lists the reference modules export plus the first entry
that is no multiple of the kernel's tile or block; no reference arithmetic is evaluated here.  Each case runs the call with identical inputs
plain (twice: an entry must repeat its own bits), under poison 0xFF and under poison 0x4B, and asserts
  1. every guard byte of every allocation, operand and caller-supplied output still holds the poison;
  2. inside the region the header defines (rows below a count, ...: the row's `region`; by default the whole output) the three runs agree
     bit for bit;
  3. no NaN inside the region that the plain run does not have;
  4. where the header says "untouched" / "not written", the elements outside the region still hold what the wrapper put there -- the poison
     for torch.empty, the fill for torch.zeros;
  5. an input that is not also an output still holds the bits it was given;
  6. a workspace is allocated by the wrapper at exactly the size the entry's *_workspace_size reports: its guards prove that size enough.
Rows whose result is an unordered set by the header's wording (the fused detection heads' candidate slots) are compared through the row's
`canon`, which is the comparison their own test makes."""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

import guarded_alloc as G

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")

# name: the id; covers: the public functions ("module.function") the row runs; cases: [(id, case)]; call(case, dev, h) -> {name: tensor} with
# h.guarded() around every input, h.empty() for every output the caller supplies; region(case, plain) -> {name: (mask of the defined elements,
# untouched)} for the outputs that are not defined everywhere -- untouched True: everything outside the mask must keep its pre-call content, a
# boolean tensor: those elements must, False: the header calls the rest scratch; switches(case) -> {tuning switch: value};
# canon(case, outs) -> outs in a form that two correct runs share.
Row = namedtuple("Row", "name covers cases call region switches canon", defaults=(None, None, None))
ROWS = []


def row(name, covers, cases, region=None, switches=None, canon=None):
    def add(call):
        ROWS.append(Row(name, tuple(covers), list(cases), call, region, switches, canon))
        return call
    return add


def _t(a, dev):
    return (torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a).to(dev)


def _below(count, cap, shape_tail=()):
    """Mask (n, cap) + tail: entry k of row i is defined iff k < count[i] (a negative count: none)."""
    m = torch.arange(cap, device=count.device)[None, :] < count.clamp(min=0)[:, None].long()
    for _ in shape_tail:
        m = m.unsqueeze(-1)
    return m.expand(m.shape[:2] + tuple(shape_tail)) if shape_tail else m


def _first(cases, pred):
    return next(i for i, c in enumerate(cases) if pred(c))


# ================================================================================================================== bit grid
def _clouds(case):
    pts = np.load(os.path.join(GOLD, "voxel_2048.npz"))["points"].astype(np.float32)
    counts = {"golden2048": (pts.shape[0],), "two_clouds_2048_0": (pts.shape[0], 0)}[case]
    buf = np.zeros((len(counts), pts.shape[0], 4), np.float32)
    buf[:, :, :pts.shape[1]] = pts[None]
    return buf, np.asarray(counts, np.int32)


CLOUDS = [("golden2048", "golden2048"), ("two_clouds_2048_0", "two_clouds_2048_0")]


def _bits(case, dev, h):
    from v2x_sim_amd import ops
    buf, cnt = _clouds(case)
    return h.guarded(ops.voxelize_bits(_t(buf, dev), _t(cnt, dev), ops.VoxelGrid()))


@row("voxelize_bits", ["ops.voxelize_bits"], CLOUDS)
def _voxelize_bits(case, dev, h):
    from v2x_sim_amd import ops
    buf, cnt = _clouds(case)
    return {"bits": ops.voxelize_bits(h.guarded(_t(buf, dev)), h.guarded(_t(cnt, dev)), ops.VoxelGrid())}


@row("voxelize_fused_bits", ["ops.voxelize_fused_bits"], CLOUDS)
def _voxelize_fused_bits(case, dev, h):
    from v2x_sim_amd import ops
    buf, cnt = _clouds(case)
    n = len(cnt)
    xf = torch.eye(4)[:3].repeat(n, 1, 1).contiguous()
    ar = torch.arange(n, dtype=torch.int32)
    # n + 1 grids: the last one is nobody's destination and must come back cleared
    return {"bits": ops.voxelize_fused_bits(h.guarded(_t(buf, dev)), h.guarded(_t(cnt, dev)), h.guarded(_t(xf, dev)), h.guarded(_t(ar, dev)),
                                            h.guarded(_t(ar.clone(), dev)), n + 1, ops.VoxelGrid())}


@row("bits_to_dense", ["ops.bits_to_dense"], CLOUDS)
def _bits_to_dense(case, dev, h):
    from v2x_sim_amd import ops
    return {"dense": ops.bits_to_dense(_bits(case, dev, h), 13)}


@row("bits_to_nhwc", ["ops.bits_to_nhwc"], [("%s-cpad%d" % (n, p), (c, p)) for n, c in CLOUDS for p in (16, 32)])
def _bits_to_nhwc(case, dev, h):
    from v2x_sim_amd import ops
    return {"nhwc": ops.bits_to_nhwc(_bits(case[0], dev, h), 13, case[1])}


@row("dense_to_nhwc", ["ops.dense_to_nhwc"], [("%s-cpad%d" % (n, p), (c, p)) for n, c in CLOUDS for p in (16, 32)])
def _dense_to_nhwc(case, dev, h):
    from v2x_sim_amd import ops
    dense = h.guarded(ops.bits_to_dense(_bits(case[0], dev, h), 13))
    return {"nhwc": ops.dense_to_nhwc(dense, case[1])}


def _occupancy():
    return int(np.load(os.path.join(GOLD, "voxel_2048.npz"))["indices"].shape[0])


IDX_CASES = [("%s-cap-%s" % (n, k), (c, k)) for n, c in CLOUDS for k in ("below", "above")]


def _idx_cap(kind):
    return _occupancy() - 5 if kind == "below" else _occupancy() + 59


def _idx_region(case, plain):
    cap = plain["idx"].shape[1]
    # "only `cap` are written": rows below min(count, cap); the wrapper clears the rest, and it stays cleared
    return {"idx": (_below(plain["counts"].clamp(max=cap), cap, (3,)), True)}


@row("bits_to_indices", ["ops.bits_to_indices"], IDX_CASES, region=_idx_region)
def _bits_to_indices(case, dev, h):
    from v2x_sim_amd import ops
    idx, counts = ops.bits_to_indices(_bits(case[0], dev, h), 13, _idx_cap(case[1]))
    return {"idx": idx, "counts": counts}


@row("indices_to_bits", ["ops.indices_to_bits"], CLOUDS)
def _indices_to_bits(case, dev, h):
    from v2x_sim_amd import ops
    idx, counts = ops.bits_to_indices(_bits(case, dev, h), 13, _idx_cap("above"))
    return {"bits": ops.indices_to_bits(h.guarded(idx), h.guarded(counts), ops.VoxelGrid())}


# ================================================================================================================== convolutions
def _guard_pc(pc, h):
    """The packed layer with its parameter tensors between guards too."""
    from v2x_sim_amd import ops
    q = ops.PackedConv(**{k: getattr(pc, k) for k in ops.PackedConv.__slots__ if k != "covered"})
    for k in ("weight", "scale", "shift", "weight2", "scale2", "shift2"):
        setattr(q, k, h.guarded(getattr(pc, k)))
    return q


def _nhwc(x, dev):
    return None if x is None else x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(dev)


def _conv_cases():
    """One RUN_CASES row per w_layout (the smallest), the smallest split-K row of either stride (their workspace) and of the GRU epilogue, and the
    gather kernel's 9 x 7 stride-2 row (no multiple of any tile)."""
    import conv_refs as R
    picks = {}
    for c in R.RUN_CASES:
        f = c.fields
        size = f.get("N", 1) * f["H"] * f["W"] * (f["C0"] + f.get("C1", 0)) * f["Cout"]
        if R.is_gru(c):
            key = "gru-splitk" if f.get("splitk") else None
        elif f.get("splitk"):
            key = "splitk-stride%d" % f.get("stride", 1)
        elif f["H"] % 8:
            key = "layout0-ragged"
        else:
            key = "layout%d" % f.get("w_layout", 0)
        if key and (key not in picks or size < picks[key][0]):
            picks[key] = (size, c)
    return [("%s-%s" % (k, R.case_id(c)), c) for k, (_, c) in sorted(picks.items())]


def _conv_built(c):
    import conv_refs as R
    return R._draw(c, "rand", 0) if R.is_gru(c) else R.build(c.row, "int")


@row("conv2d", ["ops.conv2d"], _conv_cases(), switches=lambda c: c.switches)
def _conv2d(c, dev, h):
    import conv_refs as R
    from v2x_sim_amd import ops
    b = _conv_built(c)
    pc = _guard_pc(b.pack(dev), h)
    in0 = h.guarded(b.bits.to(dev)) if b.bits is not None else h.guarded(_nhwc(b.x0, dev))
    with R.latency(b):
        return {"out": ops.conv2d(pc, in0, h.guarded(_nhwc(b.x1, dev)), zbits=c.fields.get("in_zbits", 0), splitk=b.splitk)}


def _gather_case():
    import conv_refs as R
    return next(c for c in R.RUN_CASES if c.name == "conv_igemm_kernel<48, 256, 1, 4, 0>")


@row("run_layer", ["ops.run_layer"], [("bits-to-gather-fallback", None)])
def _run_layer(case, dev, h):
    """A layer without a halo packing on the bit grid: run_layer expands the bits (bits_to_nhwc) and takes the gather kernel."""
    import conv_refs as R
    from v2x_sim_amd import ops
    b = R.build(_gather_case().row, "int")
    g = torch.Generator().manual_seed(5)
    bits = torch.randint(0, 1 << R.ZBITS, (2, b.H, b.W), generator=g, dtype=torch.int32)
    return {"out": ops.run_layer(ops.Layer([_guard_pc(b.pack(dev), h)]), h.guarded(bits.to(dev)), zbits=R.ZBITS)}


def _fused(kind):
    import conv_refs as R
    return [("%s-%dx%dx%d" % c, c) for c in R.FUSED_CASES if c[0] == kind and c[1:] == (1, 8, 32)]


@row("conv2d_pair", ["ops.conv2d_pair"], _fused("pair"))
def _conv2d_pair(c, dev, h):
    import conv_refs as R
    from v2x_sim_amd import ops
    b = R.build_fused(*c, "int")
    pa, pb = (_guard_pc(p, h) for p in b.pack(dev))
    return {"out": ops.conv2d_pair(pa, pb, h.guarded(b.bits.to(dev)), R.ZBITS)}


@row("conv2d_tail", ["ops.conv2d_tail"], _fused("tail"))
def _conv2d_tail(c, dev, h):
    import conv_refs as R
    from v2x_sim_amd import ops
    b = R.build_fused(*c, "int")
    pa, pb = (_guard_pc(p, h) for p in b.pack(dev))
    cls, loc = ops.conv2d_tail(pa, pb, h.guarded(_nhwc(b.x0, dev)), R.TAIL_SPLIT)
    return {"cls": cls, "loc": loc}


_HEADS = {}


def _det_heads(dev):
    if "pc" not in _HEADS:
        from test_gpu_postprocess import _heads_model
        _HEADS["pc"] = _heads_model(dev).packed(dev)["heads"].det
    return _HEADS["pc"]


def _det_canon(case, outs):
    """The header's wording: a candidate's slot is the order of arrival ("~score bits << 32 | anchor index << 12 | slot"), so two runs agree on the
    SET.  Per map: the candidates without their slot in ascending order, each with the codes its slot holds; a map with more candidates than slots
    keeps whichever arrived first -- only its count is comparable."""
    keys, codes, counts = outs["keys"], outs["codes"], outs["counts"]
    cap = keys.shape[1]
    res = {"counts": counts}
    for i in range(keys.shape[0]):
        k = int(counts[i])
        if k > cap:
            continue
        slot = (keys[i, :k] & 0xfff).long()
        assert sorted(slot.tolist()) == list(range(k)), "the slots of map %d are no permutation of its count" % i
        order = torch.argsort(keys[i, :k] >> 12)
        res["cand%d" % i] = (keys[i, :k] >> 12)[order]
        res["codes%d" % i] = codes[i][slot[order]]
    return res


@row("conv2d_det", ["ops_post.conv2d_det"], [("5x8x32-thr0.7-cap4096", (0.7, 4096)), ("5x8x32-thr0-cap64-overflow", (0.0, 64))], canon=_det_canon)
def _conv2d_det(case, dev, h):
    from v2x_sim_amd import ops
    g = torch.Generator().manual_seed(13)
    x = (torch.randn(5, 8, 32, 32, generator=g) * 0.7).relu().to(torch.bfloat16)
    keys, codes, counts = ops.conv2d_det(_guard_pc(_det_heads(dev), h), h.guarded(x.to(dev)), case[0], case[1])
    return {"keys": keys, "codes": codes, "counts": counts}


_CODECS = {}


def _codec(C, Cc, dev, h):
    from v2x_sim_amd import ops
    if (C, Cc) not in _CODECS:
        from test_gpu_codec import _packed
        _CODECS[(C, Cc)] = _packed(C, Cc, dev, seed=C + Cc)[0]
    pc = _CODECS[(C, Cc)]
    return ops.PackedCodec(pc.name, pc.C, pc.Cc, h.guarded(pc.weight), h.guarded(pc.ss))


CODEC_CASES = [("C%d-Cc%d-M%d" % c, c) for c in ((128, 1, 1), (128, 1, 37), (256, 64, 37), (256, 64, 257))]


def _codec_x(c, dev):
    g = torch.Generator().manual_seed(sum(c))
    return torch.randn(c[2], c[0], generator=g).to(torch.bfloat16).to(dev)


@row("codec", ["ops.codec"], CODEC_CASES)
def _codec_fused(c, dev, h):
    from v2x_sim_amd import ops
    pc, x = _codec(c[0], c[1], dev, h), h.guarded(_codec_x(c, dev))
    y, msg = ops.codec(pc, x, want_msg=True)
    return {"y": y, "msg": msg, "y_alone": ops.codec(pc, x)}


@row("codec_compress", ["ops.codec_compress"], CODEC_CASES)
def _codec_compress(c, dev, h):
    from v2x_sim_amd import ops
    return {"msg": ops.codec_compress(_codec(c[0], c[1], dev, h), h.guarded(_codec_x(c, dev)))}


@row("codec_decompress", ["ops.codec_decompress"], CODEC_CASES)
def _codec_decompress(c, dev, h):
    from v2x_sim_amd import ops
    g = torch.Generator().manual_seed(sum(c) + 1)
    msg = torch.randn(c[2], c[1], generator=g).relu().to(torch.bfloat16).to(dev)
    return {"y": ops.codec_decompress(_codec(c[0], c[1], dev, h), h.guarded(msg))}


# ================================================================================================================== fusion
def _warp_cases():
    import fusion_refs as FR
    picks = [0, _first(FR.WARP_CASES, lambda c: c.items == "ragged"), _first(FR.WARP_CASES, lambda c: c.form == "direct<1>"),
             _first(FR.WARP_CASES, lambda c: c.form == "direct<1>" and c.items == "ragged")]
    return [("%s-%s" % (FR.warp_case_id(FR.WARP_CASES[i]), FR.MODE_NAMES[m]), (i, m)) for i in picks for m in (FR.WSUM, FR.MEAN, FR.MAX)]


@row("warp_fuse", ["ops.warp_fuse"], _warp_cases())
def _warp_fuse(case, dev, h):
    """Without out= (the wrapper allocates) and with it (the caller's buffer), on an items tensor whose frame-order table the wrapper builds."""
    import fusion_refs as FR
    from v2x_sim_amd import ops
    c = FR.WARP_CASES[case[0]]
    feat, T, items, coef, _ = FR.make_warp_case(c)
    x, Td, cd = h.guarded(_nhwc(feat, dev)), h.guarded(T.to(dev)), h.guarded(coef.to(dev))
    it = h.guarded(torch.tensor(items, dtype=torch.int32, device=dev).view(-1, 2))
    given = h.empty((len(items), c.H, c.W, c.C), torch.bfloat16, dev)
    ops.warp_fuse(x, c.A, c.Bt, Td, it, cd, case[1], out=given)
    return {"allocated": ops.warp_fuse(x, c.A, c.Bt, Td, it, cd, case[1]), "given": given}


def _attn_cases():
    import fusion_refs as FR
    picks = [_first(FR.ATTN_CASES, lambda c, a=a: c.A == a) for a in (1, 5, 9)]
    return [("%s-%s" % (FR.attn_case_id(FR.ATTN_CASES[i]), norm), (i, norm)) for i in picks for norm in ("softmax", "sparsemax")]


@row("attn_handshake", ["ops.attn_handshake"], _attn_cases())
def _attn_handshake(case, dev, h):
    import fusion_refs as FR
    from v2x_sim_amd import ops
    c = FR.ATTN_CASES[case[0]]
    keys, querys, w, b = (h.guarded(t.to(dev)) for t in FR.make_attn_case(c, case[0]))
    outs = {}
    for mode in ("softmax", "activated", "argmax_test"):
        outs["prob_" + mode], outs["coef_" + mode] = ops.attn_handshake(keys, querys, w, b, c.A, c.Bt, mode, norm=case[1])
    return outs


def _pixel_cases():
    import fusion_refs as FR
    picks = [0, _first(FR.PIXEL_CASES, lambda c: c.C % 16), _first(FR.PIXEL_CASES, lambda c: c.n == 70)]
    return [(FR.pixel_case_id(FR.PIXEL_CASES[i]), i) for i in picks]


@row("pixel_weighted_fuse", ["ops.pixel_weighted_fuse"], _pixel_cases())
def _pixel_weighted_fuse(i, dev, h):
    import fusion_refs as FR
    from v2x_sim_amd import ops
    scores, valid, maps = FR.make_pixel_case(FR.PIXEL_CASES[i], i)
    return {"out": ops.pixel_weighted_fuse(h.guarded(scores.to(dev)), h.guarded(valid.to(dev)), h.guarded(maps.to(torch.bfloat16).to(dev)))}


def _seg_cases():
    import fusion_refs as FR
    small = [i for i, c in enumerate(FR.SEG_CASES) if c.n * c.H * c.W <= 3 * 64 * 64 and c.offset is None]      # never a workload-sized case
    picks = [_first(FR.SEG_CASES, lambda c: c.n_cls == 8 and c.n * c.H * c.W % 4 == 0 and c.n * c.H * c.W <= 3 * 64 * 64 and c.offset is None),
             _first(FR.SEG_CASES, lambda c: c.n * c.H * c.W % 4 != 0)]
    picks += [i for i in small if FR.SEG_CASES[i].n_cls == 64][:1]
    return [(FR.seg_case_id(FR.SEG_CASES[i]), i) for i in picks]


@row("seg_argmax_confusion", ["ops.seg_argmax_confusion"], _seg_cases())
def _seg_argmax_confusion(i, dev, h):
    import fusion_refs as FR
    from v2x_sim_amd import ops
    logits, label = FR.make_seg_case(FR.SEG_CASES[i], i)
    lg, lb = h.guarded(logits.to(dev)), h.guarded(label.to(dev))
    pred, conf = ops.seg_argmax_confusion(lg, lb)
    pred_alone, _ = ops.seg_argmax_confusion(lg, None)
    _, conf_alone = ops.seg_argmax_confusion(lg, lb, want_pred=False)
    return {"pred": pred, "conf": conf, "pred_alone": pred_alone, "conf_alone": conf_alone}


def _channel_cases():
    import channel_refs as CR
    picks = [0, 1, _first(CR.CASES, lambda c: len(set(c["counts"])) > 1), _first(CR.CASES, lambda c: c["sigma"] == 0),
             _first(CR.CASES, lambda c: c["outputs"] == "bare")]
    return [(CR.CASES[i]["name"], i) for i in picks]


@row("channel_degrade", ["ops.channel_degrade"], _channel_cases())
def _channel_degrade(i, dev, h):
    """Allocates nothing: every output is the caller's (h.empty), the step counter an in/out operand."""
    import channel_refs as CR
    from v2x_sim_amd import ops
    case = CR.CASES[i]
    Ag, Bt, bare, sigma = case["A"], case["Bt"], case["outputs"] == "bare", case["sigma"]
    items, coef0 = CR.static_plan(case["counts"], Ag, case["kind"], case["only_v2i"])
    n = len(items)
    it = h.guarded(torch.tensor(items, dtype=torch.int32).view(-1, 2).to(dev))
    outs = {"coef": h.empty((n, Ag), torch.float32, dev)}
    if not bare:
        outs["coef2"], outs["link"] = h.empty((n * Ag, Ag), torch.float32, dev), h.empty((Bt, Ag, Ag), torch.uint8, dev)
    T = h.guarded(_t(CR.synthetic_trans(Bt, Ag, seed=Bt * 100 + Ag), dev)) if sigma > 0 else None
    if sigma > 0:
        outs["trans_out"] = h.empty((Bt, Ag, Ag, 4, 4), torch.float32, dev)
    outs["step"] = h.guarded(torch.tensor([case["step"]], dtype=torch.int64, device=dev))
    ops.channel_degrade(it, Ag, Bt, h.guarded(_t(coef0, dev)), outs["coef"], outs.get("coef2"), outs.get("link"), T, outs.get("trans_out"), case["p"], sigma,
                        case["seed"], outs["step"])
    return outs


# ================================================================================================================== post-processing
def _nms_cases():
    import post_refs as P
    mixed = _first(P.NMS_CASES, lambda c: {0, 37, 513} <= set(c.counts) and not c.rotated)
    rot = _first(P.NMS_CASES, lambda c: c.rotated and 513 in c.counts)
    return [(P.NMS_CASES[i].name, i) for i in (mixed, rot)]


def _nms_launch(i, dev, h):
    import post_refs as P
    d = P.make_nms_case(i)
    case = d["case"]
    t = {k: h.guarded(_t(v, dev)) for k, v in P.launch_arrays(d["maps"], d["anchors"], d["codes"], case.cap).items()}
    t["anchors"] = h.guarded(_t(d["anchors"], dev))
    return case, t


def _nms_region(case, plain):
    """out_count >= 0: the detections below it, scores and anchor indices beyond it are not written, box rows beyond it are the call's scratch;
    negative ("more than cap candidates"): "nothing else is written for that map"."""
    cap = plain["scores"].shape[1]
    over = (plain["count"] < 0)[:, None, None].expand(-1, cap, 5)
    return {"boxes": (_below(plain["count"], cap, (5,)), over), "scores": (_below(plain["count"], cap), True), "index": (_below(plain["count"], cap), True)}


def _nms_outs(res):
    return dict(zip(("boxes", "scores", "index", "count"), res))


@row("det_postprocess", ["ops_post.det_postprocess"], _nms_cases(), region=_nms_region)
def _det_postprocess(i, dev, h):
    import post_refs as P
    from v2x_sim_amd import ops
    case, t = _nms_launch(i, dev, h)
    return _nms_outs(ops.det_postprocess(t["cls"], t["loc"], t["anchors"], P.SCORE_THR, case.nms_thr, case.cap, rotated=case.rotated))


@row("det_nms_candidates", ["ops_post.det_nms_candidates"], _nms_cases(), region=_nms_region)
def _det_nms_candidates(i, dev, h):
    from v2x_sim_amd import ops
    case, t = _nms_launch(i, dev, h)
    return _nms_outs(ops.det_nms_candidates(t["keys"], t["slot_codes"], t["counts"], t["anchors"], case.nms_thr, rotated=case.rotated))


def _late_region(i, plain):
    """As v2x_det_postprocess: rows below out_count; scores and sources beyond it are not written, box rows beyond it are scratch."""
    cap = plain["scores"].shape[1]
    return {"boxes": (_below(plain["count"], cap, (5,)), False), "scores": (_below(plain["count"], cap), True), "src": (_below(plain["count"], cap), True)}


def _late_cases():
    import late_refs as LR
    return [(LR.LATE_CASES[i].name, i) for i in (0, 1)]


@row("late_fuse", ["ops_post.late_fuse"], _late_cases(), region=_late_region)
def _late_fuse(i, dev, h):
    import late_refs as LR
    from v2x_sim_amd import ops
    d = LR.make_late_case(i)
    c = d["case"]
    g = lambda a: h.guarded(_t(a, dev))      # noqa: E731
    res = ops.late_fuse(g(d["boxes"]), g(d["scores"]), g(d["counts"].astype(np.int32)), g(d["rigid"]), g(d["link"].astype(np.uint8)), c.extents,
                        nms_thr=c.nms_thr, rotated=c.rotated, cap_out=c.cap_out)
    return dict(zip(("boxes", "scores", "src", "count"), res))


def _assign_cases():
    import assign_refs as AR
    picks = [0, 1, _first(AR.ASSIGN_CASES, lambda c: c.X % 16 and len(c.items) == 1)]
    wants = ((), ("assoc",), ("anchor_iou",), ("assoc", "anchor_iou"))
    return [("%s-want-%s" % (AR.ASSIGN_CASES[i].name, "+".join(w) or "none"), (i, w)) for i in picks for w in wants]


@row("assign_targets", ["ops_post.assign_targets"], _assign_cases())
def _assign_targets(case, dev, h):
    import assign_refs as AR
    from v2x_sim_amd import ops
    d = AR.make_case(case[0])
    c = d["case"]
    return ops.assign_targets(h.guarded(_t(d["gt_boxes"], dev)), h.guarded(_t(d["gt_count"], dev)), h.guarded(_t(d["anchors"], dev)), pos_thr=c.pos_thr,
                              neg_thr=c.neg_thr, force_match=bool(c.force), want=case[1])


@row("rotated_iou", ["ops_post.rotated_iou"], [("explicit-pairs", 0), ("one-by-pairs", 1)])
def _rotated_iou(case, dev, h):
    import post_refs as P
    from v2x_sim_amd import ops
    a, b = P.iou_pair_arrays()
    return {"iou": ops.rotated_iou(h.guarded(_t(a[:1] if case else a, dev)), h.guarded(_t(b, dev)))}


def _match_region(want_iou, plain):
    """"entries >= det_count untouched": they keep the wrapper's fill."""
    m = _below(plain["det_count"], plain["tp"].shape[1])
    return {k: (m, True) for k in ("tp", "best_iou") if k in plain}


@row("match_detections", ["ops_post.match_detections"], [("match0-tp", False), ("match0-tp-and-iou", True)], region=_match_region)
def _match_detections(want_iou, dev, h):
    import post_refs as P
    from v2x_sim_amd import ops
    det, dc, gt, gc, thr, _ = P.make_match_case(0)
    dcd = h.guarded(_t(dc, dev))
    res = ops.match_detections(h.guarded(_t(det, dev)), dcd, h.guarded(_t(gt, dev)), h.guarded(_t(gc, dev)), thr, want_iou=want_iou)
    outs = {"tp": res[0], "best_iou": res[1]} if want_iou else {"tp": res}
    outs["det_count"] = dcd.clamp(max=det.shape[1])
    return outs


DET_MAP_CASES = ("degenerate", "taken-0.5-0.7", "length-65")


@row("det_map", ["ops_post.det_map"], [("%s-%s" % (n, "flags" if f else "ap"), (n, f)) for n in DET_MAP_CASES for f in (False, True)])
def _det_map(case, dev, h):
    import det_map_refs as DR
    from v2x_sim_amd import ops
    c = DR.make_case(case[0])
    t = {k: h.guarded(_t(np.array(c[k]), dev)) for k in ("det", "scores", "det_count", "gt", "gt_count", "group")}
    res = ops.det_map(t["det"], t["scores"], t["det_count"], t["gt"], t["gt_count"], t["group"], c["thrs"], c["n_groups"], want_flags=case[1])
    return dict(zip(("ap", "num_gt", "num_det", "num_tp", "tp", "rank"), res))


# ================================================================================================================== tracking
@row("assign_iou", ["ops_track.assign_iou"], [("%dx%d-%s" % (r, c, "direct" if d else "optimal"), (r, c, d)) for r, c in ((1, 5), (13, 9), (64, 64)) for d in (1, 0)])
def _assign_iou(case, dev, h):
    from v2x_sim_amd import ops
    r, c, direct = case
    rng = np.random.default_rng(100 * r + c)
    iou = rng.uniform(0.0, 1.0, (3, r, c)).astype(np.float32)
    iou[1] *= (rng.uniform(size=(r, c)) < 0.2)                       # sparse: the direct shortcut's side
    nr, nc = np.asarray([r, r, max(r - 1, 0)], np.int32), np.asarray([c, max(c - 2, 0), c], np.int32)
    return {"row_to_col": ops.assign_iou(h.guarded(_t(iou, dev)), h.guarded(_t(nr, dev)), h.guarded(_t(nc, dev)), thr=0.3, direct=bool(direct))}


def _sort_region(case, plain):
    """"Entries >= out_count are not written": they keep the poison of the wrapper's torch.empty."""
    res = {}
    for f in range(4):
        cnt, cap = plain["count%d" % f], plain["ids%d" % f].shape[1]
        res.update({"boxes%d" % f: (_below(cnt, cap, (4,)), True), "ids%d" % f: (_below(cnt, cap), True), "det%d" % f: (_below(cnt, cap), True)})
    return res


@row("sort_step", ["ops_track.sort_step"], [("4frames-3streams-tcap%d" % t, t) for t in (64, 5)], region=_sort_region)
def _sort_step(t_cap, dev, h):
    """Four frames, three streams of different detection counts (12 objects, 5, none); the state tensors are in/out operands."""
    import track_refs as TR
    from test_gpu_track import _pack
    from v2x_sim_amd import ops
    dets = [TR.make_case(0)[0], [d[:5] for d in TR.make_case(1)[0]], [np.zeros((0, 4), np.float32)] * TR.N_FRAMES]
    st = tuple(h.guarded(torch.zeros(s, dtype=dt, device=dev)) for s, dt in (((3, t_cap, 17), torch.float32), ((3, t_cap, 5), torch.int32), ((3, 4), torch.int32)))
    outs = {"trk_f": st[0], "trk_i": st[1], "stream_i": st[2]}
    for f in range(4):
        buf, cnt = _pack([dets[s][f] for s in range(3)], 64)
        res = ops.sort_step(h.guarded(_t(buf, dev)), h.guarded(_t(cnt, dev)), *st, min_hits=1)
        outs.update({"boxes%d" % f: res[0], "ids%d" % f: res[1], "det%d" % f: res[2], "count%d" % f: res[3]})
    return outs


def _seq_args(a, dev, h):
    return [h.guarded(_t(a[k], dev)) for k in ("gb", "gi", "gc", "tb", "ti", "tc")]


@row("hota_sequences", ["ops_track.hota_sequences"], [("hota-case0", 0), ("hota-case0-and-one-frame", 1)])
def _hota_sequences(case, dev, h):
    import hota_refs as H
    from test_gpu_hota import _pad
    from v2x_sim_amd import ops
    frames = H.make_frames(*H.CASES[0])
    a = _pad([frames, frames[:1]] if case else [frames])
    out_i, out_f = ops.hota_sequences(*_seq_args(a, dev, h), a["NG"], a["NT"])
    return {"out_i": out_i, "out_f": out_f}


@row("mot_sequences", ["ops_track.mot_sequences"], [("mot-stress0", 0), ("mot-stress0-and-one-frame", 1)])
def _mot_sequences(case, dev, h):
    import mot_refs as M
    from test_gpu_mot import _pad
    from v2x_sim_amd import ops
    n_gt, n_trk, n_frames = M.STRESS[0]
    frames = M.group_frames(0, n_gt, n_trk, n_frames)
    a = _pad([frames, frames[:1]] if case else [frames])
    out_i, out_f = ops.mot_sequences(*_seq_args(a, dev, h), a["NG"], a["NT"])
    return {"out_i": out_i, "out_f": out_f}


# ================================================================================================================== segmentation targets, LiDAR
def _raster_cases():
    import seg_raster_refs as SR
    return [("%s-%s" % (SR.NAMES[i], "+".join(w) or "labels"), (i, w)) for i in (0, 1) for w in (("owner", "hist"), ())]


@row("rasterize_seg", ["ops_seg.rasterize_seg"], _raster_cases())
def _rasterize_seg(case, dev, h):
    import seg_raster_refs as SR
    from v2x_sim_amd import ops
    c = SR.RASTER_CASES[case[0]]
    rng = np.random.default_rng(1000 + case[0])
    grid = SR.grid_of(c.X, c.Y, c.cell)
    items = c.build(rng, grid, c.cap, c.n_cls)
    boxes = np.zeros((len(items), c.cap, 5), np.float32)
    boxes[:, :, 2:4] = 1000.0
    cls = np.full((len(items), c.cap), min(7, c.n_cls - 1), np.uint8)
    count = np.zeros((len(items),), np.int32)
    for m, (b, k, n) in enumerate(items):
        boxes[m, :b.shape[0]], cls[m, :b.shape[0]], count[m] = b, k, n
    rank = None if c.rank is None else h.guarded(_t(np.asarray(c.rank, np.uint8), dev))
    return ops.rasterize_seg(h.guarded(_t(boxes, dev)), h.guarded(_t(cls, dev)), h.guarded(_t(count, dev)), grid, n_classes=c.n_cls, rank=rank, want=case[1])


def _lidar_cases():
    import lidar_refs as LR
    picks = [0, 1, _first(LR.CASES, lambda c: "max_pts_below" in c[0])]
    return [(LR.NAMES[i], i) for i in picks]


def _lidar_scene(build):
    """The scene of a case builder without its reference; a symbolic max_pts ("above" / "equal" / "below" the returns) becomes a fixed small number."""
    sc = dict(build())
    if isinstance(sc["max_pts"], str):
        sc["max_pts"] = {"above": 1024, "equal": 96, "below": 40}[sc["max_pts"]]
    return sc


def _cast_kw(sc):
    return dict(ground_z=sc["ground_z"], r_min=sc["r_min"], r_max=sc["r_max"], sigma_r=sc["sigma_r"], p_drop=sc["p_drop"], seed=sc["seed"], step=sc["step"])


def _scene_on(sc, keys, dev, h):
    return {k: h.guarded(_t(np.array(sc[k]), dev)) for k in keys}


@row("lidar_cast", ["ops_lidar.lidar_cast"], _lidar_cases())
def _lidar_cast(i, dev, h):
    import lidar_refs as LR
    from v2x_sim_amd import ops
    sc = _lidar_scene(LR.CASES[i][1])
    d = _scene_on(sc, ("sensors", "frame_of", "boxes", "box_count", "beam", "az"), dev, h)
    res = dict(ops.lidar_cast(d["sensors"], d["frame_of"], d["boxes"], d["box_count"], d["beam"], d["az"], sc["max_pts"], **_cast_kw(sc)))
    bare = ops.lidar_cast(d["sensors"], d["frame_of"], d["boxes"], d["box_count"], d["beam"], d["az"], sc["max_pts"], want=(), **_cast_kw(sc))
    res.update({"points_bare": bare["points"], "n_pts_bare": bare["n_pts"]})
    return res


@row("visible_boxes", ["ops_lidar.visible_boxes"], [("%s-%s" % (n, "any" if a else "own"), (i, a)) for n, i in _lidar_cases() for a in (False, True)])
def _visible_boxes(case, dev, h):
    import lidar_refs as LR
    from v2x_sim_amd import ops
    sc = _lidar_scene(LR.CASES[case[0]][1])
    d = _scene_on(sc, ("sensors", "frame_of", "boxes", "box_count", "beam", "az"), dev, h)
    hits = h.guarded(ops.lidar_cast(d["sensors"], d["frame_of"], d["boxes"], d["box_count"], d["beam"], d["az"], sc["max_pts"], **_cast_kw(sc))["box_hits"])
    gt, cnt = ops.visible_boxes(hits, d["sensors"], d["frame_of"], d["boxes"], d["box_count"], min_hits=sc["min_hits"], any_agent=case[1], x_lim=sc["x_lim"],
                                y_lim=sc["y_lim"])
    return {"gt_boxes": gt, "gt_count": cnt}


MOTION_KEYS = ("sensors", "sensor_vel", "time_of", "frame_of", "boxes", "box_vel", "box_count", "beam", "az", "az_time")


def _motion_cases():
    import lidar_motion_refs as MR
    picks = [0, 1, 2 * MR.N_STATIC, _first(MR.CASES, lambda c: "max_pts_below" in c[0] and not c[0].startswith("zero_"))]
    return [(MR.NAMES[i], i) for i in picks]


def _moving_cast(sc, d, **kw):
    from v2x_sim_amd import ops
    return ops.lidar_cast_moving(d["sensors"], d["sensor_vel"], d["time_of"], d["frame_of"], d["boxes"], d["box_vel"], d["box_count"], d["beam"], d["az"],
                                 d["az_time"], sc["max_pts"], **kw, **_cast_kw(sc))


@row("lidar_cast_moving", ["ops_lidar.lidar_cast_moving"], _motion_cases())
def _lidar_cast_moving(i, dev, h):
    import lidar_motion_refs as MR
    sc = _lidar_scene(MR.CASES[i][1])
    d = _scene_on(sc, MOTION_KEYS, dev, h)
    res = dict(_moving_cast(sc, d))
    bare = _moving_cast(sc, d, want=())
    res.update({"points_bare": bare["points"], "n_pts_bare": bare["n_pts"]})
    return res


@row("visible_boxes_moving", ["ops_lidar.visible_boxes_moving"],
     [("%s-%s" % (n, "any" if a else "own-no-vel"), (i, a)) for n, i in _motion_cases() for a in (False, True)])
def _visible_boxes_moving(case, dev, h):
    import lidar_motion_refs as MR
    from v2x_sim_amd import ops
    sc = _lidar_scene(MR.CASES[case[0]][1])
    d = _scene_on(sc, MOTION_KEYS, dev, h)
    hits = h.guarded(_moving_cast(sc, d)["box_hits"])
    return ops.visible_boxes_moving(hits, d["sensors"], d["sensor_vel"], d["time_of"], d["frame_of"], d["boxes"], d["box_vel"], d["box_count"], t_ref=sc["t_ref"],
                                    min_hits=sc["min_hits"], any_agent=case[1], x_lim=sc["x_lim"], y_lim=sc["y_lim"], want=("gt_vel",) if case[1] else ())


# ================================================================================================================== training
def _train_cases(cases, ident, off=None):
    """The first case and the first off-block case (by default: the first whose row count is no multiple of 8)."""
    picks = [0, _first(cases, off)] if off else [0]
    return [(ident(cases[i]) if callable(ident) else ident % tuple(cases[i])[:ident.count("%")], i) for i in dict.fromkeys(picks)]


def _tr():
    import train_refs
    return train_refs


@row("conv3x3_wgrad", ["ops_train.conv3x3_wgrad"], _train_cases(_tr().WGRAD_CASES, _tr().wgrad_case_id, lambda c: c.cin_out) +
     _train_cases(_tr().WGRAD_CASES, _tr().wgrad_case_id, lambda c: c.N == 3 and c.H == 8)[1:])
def _conv3x3_wgrad(i, dev, h):
    from v2x_sim_amd import ops
    c = _tr().WGRAD_CASES[i]
    x, dy = _tr().make_wgrad_case(c)
    return {"dw": ops.conv3x3_wgrad(h.guarded(x.to(dev)), h.guarded(dy.to(dev)), cin_out=c.cin_out)}


def _bn_call(i, dev, h):
    from v2x_sim_amd import ops
    R = _tr()
    c = R.BN_CASES[i]
    x, dy, gamma, beta, rm0, rv0 = (h.guarded(t.to(dev)) for t in R.make_bn_case(c))
    y, mean, invstd = ops.bn_train_forward(x, gamma, beta, rm0, rv0, R.bn_eps(c), R.BN_MOMENTUM, c.relu)
    return c, x, dy, gamma, beta, {"y": y, "mean": mean, "invstd": invstd, "running_mean": rm0, "running_var": rv0}


BN_PICKS = _train_cases(_tr().BN_CASES, _tr().c8_case_id, lambda c: c.reach == "rpp+") + _train_cases(_tr().BN_CASES, _tr().c8_case_id, lambda c: c.reach == "rpp-")[1:]
_bn_switch = lambda i: {"BN_PARTIAL_T": _tr().BN_CASES[i].layout}      # noqa: E731


@row("bn_train_forward", ["ops_train.bn_train_forward"], BN_PICKS, switches=_bn_switch)
def _bn_train_forward(i, dev, h):
    return _bn_call(i, dev, h)[5]


@row("bn_train_backward", ["ops_train.bn_train_backward"], BN_PICKS, switches=_bn_switch)
def _bn_train_backward(i, dev, h):
    from v2x_sim_amd import ops
    c, x, dy, gamma, beta, fwd = _bn_call(i, dev, h)
    mean, invstd = h.guarded(fwd["mean"]), h.guarded(fwd["invstd"])
    dx, dgamma, dbeta = ops.bn_train_backward(x, dy, gamma, beta, mean, invstd, c.relu)
    dx1, dgamma1, dbeta1, dsum = ops.bn_train_backward(x, dy, gamma, beta, mean, invstd, c.relu, dx_sum=True)
    return {"dx": dx, "dgamma": dgamma, "dbeta": dbeta, "dx_s": dx1, "dgamma_s": dgamma1, "dbeta_s": dbeta1, "dx_sum": dsum,
            "running_mean": fwd["running_mean"], "running_var": fwd["running_var"]}         # (the forward's in/out operands)


@row("channel_sum", ["ops_train.channel_sum"], _train_cases(_tr().CS_CASES, _tr().c8_case_id, lambda c: c.reach == "rpp+"))
def _channel_sum(i, dev, h):
    from v2x_sim_amd import _lib, ops
    c = _tr().CS_CASES[i]
    assert _lib.load().v2x_channel_sum_workspace_size(c.M, c.C) > 0                # the kernel, not the wrapper's torch path
    return {"sums": ops.channel_sum(h.guarded(_tr().make_cs_case(c).to(dev)))}


@row("cast_pad_chsum", ["ops_train.cast_pad_chsum"], _train_cases(_tr().CP_CASES, _tr().cp_case_id, lambda c: c.reach == "rpp+"))
def _cast_pad_chsum(i, dev, h):
    from v2x_sim_amd import ops
    c = _tr().CP_CASES[i]
    res = ops.cast_pad_chsum(h.guarded(_tr().make_cp_case(c).to(dev)), c.Cp)
    assert res is not None, "the kernel refused a shape of its table"
    return {"out": res[0], "sums": res[1]}


GATES_PICKS = _train_cases(_tr().GATES_NHWC_CASES, _tr().c8_case_id, lambda c: c.reach == "rpp+")


@row("gru_gates_nhwc", ["ops_train.gru_gates_nhwc"], GATES_PICKS)
def _gru_gates_nhwc(i, dev, h):
    from v2x_sim_amd import ops
    gi, bhh, _ = _tr().make_gates_nhwc_case(_tr().GATES_NHWC_CASES[i])
    return {"h": ops.gru_gates_nhwc(h.guarded(gi.to(dev)), h.guarded(bhh.to(dev)))}


@row("gru_gates_nhwc_backward", ["ops_train.gru_gates_nhwc_backward"], GATES_PICKS)
def _gru_gates_nhwc_backward(i, dev, h):
    from v2x_sim_amd import ops
    gi, bhh, dh = (h.guarded(t.to(dev)) for t in _tr().make_gates_nhwc_case(_tr().GATES_NHWC_CASES[i]))
    dgi, sums = ops.gru_gates_nhwc_backward(gi, bhh, dh)
    return {"dgi": dgi, "sums": sums}


GATES_F32_PICKS = _train_cases(_tr().GATES_F32_CASES, "%dx%dx%dx%d", lambda c: (c.H * c.W) % 8)


@row("gru_gates", ["ops_train.gru_gates"], GATES_F32_PICKS)
def _gru_gates(i, dev, h):
    from v2x_sim_amd import ops
    gi, bhh, _ = _tr().make_gates_f32_case(_tr().GATES_F32_CASES[i])
    return {"h": ops.gru_gates(h.guarded(gi.to(dev)), h.guarded(bhh.to(dev)))}


@row("gru_gates_backward", ["ops_train.gru_gates_backward"], GATES_F32_PICKS)
def _gru_gates_backward(i, dev, h):
    from v2x_sim_amd import ops
    gi, bhh, dh = (h.guarded(t.to(dev)) for t in _tr().make_gates_f32_case(_tr().GATES_F32_CASES[i]))
    dgi, dn_r = ops.gru_gates_backward(gi, bhh, dh)
    return {"dgi": dgi, "dn_r": dn_r}


@row("warp_affine", ["ops_train.warp_affine"], [("C%d-%dx%d-%s" % (*_tr().WARP_TRAIN_CASES[i][:3], "transpose" if b else "forward"), (i, b))
                                                for i in (0, _first(_tr().WARP_TRAIN_CASES, lambda c: c.H % 8)) for b in (False, True)])
def _warp_affine(case, dev, h):
    from v2x_sim_amd import ops
    x, d, th = _tr().make_warp_train_case(_tr().WARP_TRAIN_CASES[case[0]])
    return {"out": ops.warp_affine(h.guarded((d if case[1] else x).to(dev)), h.guarded(th.to(dev)), backward=case[1])}


def _v2v_setup(i, dev, h):
    from v2x_sim_amd.models.det.base import IntermediateModelBase
    from v2x_sim_amd.train import hip_graph
    R = _tr()
    c = R.V2V_CASES[i]
    cur, base, T, d = R.make_v2v_case(c)
    counts, items, rows = IntermediateModelBase.frame_plan(torch.full((c.B, c.A), c.A), c.B, c.A)

    class _M:
        pass
    plan = hip_graph._v2v_plan(_M(), counts, items, rows, c.B, c.A, T, c.A * c.B, dev)
    plan = {k: (h.guarded(v) if torch.is_tensor(v) and v.dtype == torch.int32 else v) for k, v in plan.items()}
    return c, cur, base, h.guarded(T.to(dev)), d, plan


V2V_PICKS = _train_cases(_tr().V2V_CASES, _tr().v2v_case_id, lambda c: c.two) + _train_cases(_tr().V2V_CASES, _tr().v2v_case_id, lambda c: c.form == "irregular")[1:]


@row("v2v_message", ["ops_train.v2v_message"], V2V_PICKS)
def _v2v_message(i, dev, h):
    from v2x_sim_amd import ops
    c, cur, base, T, _, plan = _v2v_setup(i, dev, h)
    return {"conv_in": ops.v2v_message(h.guarded(cur.to(dev)), h.guarded(base.to(dev)) if c.two else None, T, plan)}


@row("v2v_message_backward", ["ops_train.v2v_message_backward"], V2V_PICKS)
def _v2v_message_backward(i, dev, h):
    from v2x_sim_amd import ops
    c, _, _, T, d, plan = _v2v_setup(i, dev, h)
    dbase, dcur = ops.v2v_message_backward(h.guarded(d.to(dev)), T, plan, c.A * c.B, c.two)
    return {"dbase": dbase, **({"dcur": dcur} if c.two else {})}


UPCAT_PICKS = [("%dx%dx%dx%d+%d" % c, c) for c in _tr().UPCAT_CASES[:2] + [next(c for c in _tr().UPCAT_CASES if c[3] % 16)]]


@row("upcat", ["ops_train.upcat"], UPCAT_PICKS)
def _upcat(c, dev, h):
    from v2x_sim_amd import ops
    N, H, W, C0, C1 = c
    g = torch.Generator().manual_seed(N * H + C0 + C1)
    lo, skip = _tr().grid_values((N, H, W, C0), g), _tr().grid_values((N, 2 * H, 2 * W, C1), g)
    return {"cat": ops.upcat(h.guarded(lo.to(dev)), h.guarded(skip.to(dev)))}


@row("upcat_backward", ["ops_train.upcat_backward"], UPCAT_PICKS)
def _upcat_backward(c, dev, h):
    from v2x_sim_amd import ops
    N, H, W, C0, C1 = c
    dcat = _tr().grid_values((N, 2 * H, 2 * W, C0 + C1), torch.Generator().manual_seed(N * H + C0))
    d_lo, d_skip = ops.upcat_backward(h.guarded(dcat.to(dev)), C0)
    return {"d_lo": d_lo, "d_skip": d_skip}


@row("zero_insert", ["ops_train.zero_insert"], [("%dx%dx%dx%d" % s, s) for s in _tr().ZERO_INSERT_CASES[:2]])
def _zero_insert(shape, dev, h):
    from v2x_sim_amd import ops
    dy = torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape))).to(torch.bfloat16)
    return {"out": ops.zero_insert(h.guarded(dy.to(dev)))}


DET_PICKS = _train_cases(_tr().DET_CASES, _tr().det_case_id, lambda c: c.n == 255 and c.mask == "sparse") + \
    _train_cases(_tr().DET_CASES, _tr().det_case_id, lambda c: c.n == 257 and c.mask == "sparse")[1:]


def _grads(ws, dev, h):
    return [None if w is None else h.guarded(torch.tensor(w, dtype=torch.float32, device=dev)) for w in ws]


@row("det_loss_forward", ["ops_train.det_loss_forward"], DET_PICKS)
def _det_loss_forward(i, dev, h):
    from v2x_sim_amd import ops
    R = _tr()
    cls, lab, loc, tgt, mask = (h.guarded(t.to(dev)) for t in R.make_det_case(R.DET_CASES[i]))
    return {"out4": ops.det_loss_forward(cls, lab, loc, tgt, mask, R.DET_ALPHA, R.DET_BETA)}


@row("det_loss_backward", ["ops_train.det_loss_backward"], DET_PICKS)
def _det_loss_backward(i, dev, h):
    from v2x_sim_amd import ops
    R = _tr()
    c = R.DET_CASES[i]
    cls, lab, loc, tgt, mask = (h.guarded(t.to(dev)) for t in R.make_det_case(c))
    out4 = h.guarded(ops.det_loss_forward(cls, lab, loc, tgt, mask, R.DET_ALPHA, R.DET_BETA))
    dcls, dloc = ops.det_loss_backward(cls, lab, loc, tgt, mask, R.DET_ALPHA, R.DET_BETA, out4, *_grads(c.grads, dev, h))
    return {"dcls": dcls, "dloc": dloc}


def _corner_picks():
    import corner_loss_refs as CL
    picks = [0, _first(CL.CORNER_CASES, lambda c: c[0] == 255 and c[1] == 3), _first(CL.CORNER_CASES, lambda c: c[0] == 257)]
    return [(CL.corner_case_id(CL.CORNER_CASES[i]), i) for i in picks]


def _corner_operands(i, dev, h):
    import corner_loss_refs as CL
    c = CL.CORNER_CASES[i]
    return c, [h.guarded(t.to(dev)) for t in CL.make_corner_case(c)], c[2] == CL.H


@row("det_corner_loss_forward", ["ops_train.det_corner_loss_forward"], _corner_picks())
def _det_corner_loss_forward(i, dev, h):
    import corner_loss_refs as CL
    from v2x_sim_amd import ops
    c, t, swap = _corner_operands(i, dev, h)
    return {"out4": ops.det_corner_loss_forward(*t, swap, CL.ALPHA)}


@row("det_corner_loss_backward", ["ops_train.det_corner_loss_backward"], _corner_picks())
def _det_corner_loss_backward(i, dev, h):
    import corner_loss_refs as CL
    from v2x_sim_amd import ops
    c, t, swap = _corner_operands(i, dev, h)
    out4 = h.guarded(ops.det_corner_loss_forward(*t, swap, CL.ALPHA))
    dcls, dloc = ops.det_corner_loss_backward(*t, swap, CL.ALPHA, out4, *_grads(c.grads, dev, h))
    return {"dcls": dcls, "dloc": dloc}


def _seg_loss_picks():
    import seg_loss_refs as S
    picks = [0, _first(S.SEG_CASES, lambda c: c.M == 257), _first(S.SEG_CASES, lambda c: c.M > 4096 and c.M % 8)]
    return [(S.case_id(S.SEG_CASES[i]), i) for i in picks]


def _seg_loss_operands(i, dev, h):
    import seg_loss_refs as S
    c = S.SEG_CASES[i]
    x, lab, w = S.make_case(c)
    return c, h.guarded(x.to(dev)), h.guarded(lab.to(dev)), None if w is None else h.guarded(w.to(dev))


@row("seg_loss_forward", ["ops_train.seg_loss_forward"], _seg_loss_picks())
def _seg_loss_forward(i, dev, h):
    from v2x_sim_amd import ops
    c, x, lab, w = _seg_loss_operands(i, dev, h)
    out3 = ops.seg_loss_forward(x, lab, w)
    assert out3 is not None, "the kernels refused a shape of their table"
    return {"out3": out3}


@row("seg_loss_backward", ["ops_train.seg_loss_backward"], _seg_loss_picks())
def _seg_loss_backward(i, dev, h):
    from v2x_sim_amd import ops
    c, x, lab, w = _seg_loss_operands(i, dev, h)
    out3 = h.guarded(ops.seg_loss_forward(x, lab, w))
    g = h.guarded(torch.tensor(0.75, dtype=torch.float32, device=dev))
    return {"dlogits": ops.seg_loss_backward(x, lab, w, out3, g), "dlogits_g1": ops.seg_loss_backward(x, lab, w, out3, None)}


@row("seg_loss_backward_packed", ["ops_train.seg_loss_backward_packed"], _seg_loss_picks())
def _seg_loss_backward_packed(i, dev, h):
    from v2x_sim_amd import ops
    c, x, lab, w = _seg_loss_operands(i, dev, h)
    out3 = h.guarded(ops.seg_loss_forward(x, lab, w))
    dy, sums = ops.seg_loss_backward_packed(x, lab, w, out3, h.guarded(torch.tensor(0.75, dtype=torch.float32, device=dev)), c.Cp)
    return {"dy": dy, "sums": sums}


@row("HipAdam.step", ["train.optim.HipAdam.step"], [(_tr().adam_case_id(_tr().ADAM_CASES[i]), i) for i in (0, 1)], switches=lambda i: {"TRAIN_ADAM_HIP": 1})
def _adam_step(i, dev, h):
    """One fused step over tensors of ADAM_SIZES (4095, 4096, 4097, 1, 0, ...): parameters, gradients and both moments between guards."""
    from v2x_sim_amd.train.optim import HipAdam, use_hip_adam
    R = _tr()
    c = R.ADAM_CASES[i]
    tensors = R.make_adam_case(c)
    ps = [torch.nn.Parameter(h.guarded(p.to(dev))) for p, _, _, _ in tensors]
    kw = dict(betas=R.ADAM_BETAS, eps=R.ADAM_EPS, weight_decay=c.wd)
    if c.device_lr:
        opt = torch.optim.Adam(ps, lr=h.guarded(torch.tensor(R.ADAM_LR, dtype=torch.float32, device=dev)), capturable=True, **kw)
    else:
        opt = torch.optim.Adam(ps, lr=R.ADAM_LR, **kw)
    opt = use_hip_adam(opt)
    assert isinstance(opt, HipAdam)
    outs = {}
    for k, (q, (_, g, m, v)) in enumerate(zip(ps, tensors)):
        q.grad = h.guarded(g.to(dev))
        opt.state[q] = {"step": torch.tensor(float(c.step - 1), dtype=torch.float32, device=dev if c.device_lr else "cpu"),
                        "exp_avg": h.guarded(m.to(dev)), "exp_avg_sq": h.guarded(v.to(dev))}
        outs.update({"p%d" % k: q.data, "g%d" % k: q.grad, "m%d" % k: opt.state[q]["exp_avg"], "v%d" % k: opt.state[q]["exp_avg_sq"]})
    opt.step()
    return outs


# ================================================================================================================== the test
ROW_BY_NAME = {r.name: r for r in ROWS}
assert len(ROW_BY_NAME) == len(ROWS)
PARAMS = [pytest.param(r.name, k, id="%s-%s" % (r.name, cid)) for r in ROWS for k, (cid, _) in enumerate(r.cases)]


def _outputs(r, case, dev, h):
    outs = {k: v for k, v in r.call(case, dev, h).items() if v is not None}
    torch.cuda.synchronize()
    return outs


def compare_runs(what, plain, got, region, harness, canon=None):
    """Assertions 2 - 4 of the module docstring for one poisoned run `got` against the plain run."""
    assert set(got) == set(plain), (what, sorted(got), sorted(plain))
    if harness is not None:
        for name, (mask, untouched) in region.items():
            if untouched is False:
                continue
            rest = ~mask if untouched is True else untouched           # True: everything outside the region; a mask: those elements
            rec = harness.record_of(got[name])
            if rec.poisoned:
                assert G.holds_poison(got[name], harness.poison, rest), "%s: %s was written where its header says it is not" % (what, name)
            else:
                assert bool((got[name][rest] == rec.fill).all()), "%s: %s lost the wrapper's fill where its header says it is not written" % (what, name)
    a, b = (plain, got) if canon is None else (canon(plain), canon(got))
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for name in a:
        mask = region[name][0] if name in region and canon is None else None
        assert a[name].shape == b[name].shape and a[name].dtype == b[name].dtype, (what, name)
        nans = G.new_nans(b[name], a[name], mask)
        assert nans == 0, "%s: %s holds %d NaN(s) the plain run does not" % (what, name, nans)
        if not G.same_bits(a[name], b[name], mask):
            ia, ib = G.as_int(a[name]), G.as_int(b[name])
            diff = (ia != ib) if mask is None else ((ia != ib) & mask)
            at = diff.nonzero()
            raise AssertionError("%s: %s differs from the plain run in %d of %d elements, first at %s" % (what, name, int(diff.sum()), diff.numel(), at[0].tolist()))


@pytest.mark.parametrize("name,k", PARAMS)
def test_memory_contract(device, tune, name, k):
    r = ROW_BY_NAME[name]
    case = r.cases[k][1]
    for sw, v in ((r.switches(case) if r.switches else {}) or {}).items():
        tune(sw, v)
    plain = _outputs(r, case, device, G.PlainAlloc())
    region = (r.region(case, plain) if r.region else None) or {}
    canon = (lambda o: r.canon(case, o)) if r.canon else None
    compare_runs("%s, a second plain run" % name, plain, _outputs(r, case, device, G.PlainAlloc()), region, None, canon)
    for poison in G.POISONS:
        with G.GuardedAlloc(poison) as h:
            got = _outputs(r, case, device, h)
            assert h.records, "nothing of %s went through the harness" % name
            h.check_guards()
            h.check_operands_unchanged(written=got.values())        # (an in/out operand is one of the row's outputs)
            compare_runs("%s under poison 0x%02X" % (name, poison), plain, got, region, h, canon)


# ================================================================================================================== the harness on the device
def test_harness_notices_on_the_device(device):
    """No kernel involved: the test itself overwrites one guard byte through the recorded buffer, and skips an element of a view."""
    from v2x_sim_amd import ops

    def entry(h, skip):
        with h:
            out = ops.torch.empty((5, 7), dtype=torch.float32, device=device)
            assert out.data_ptr() % 256 == 0 and out.is_contiguous()
            val = torch.arange(35.0, device=device).view(5, 7)
            if skip:
                out[:4] = val[:4]
                out[4, :6] = val[4, :6]
            else:
                out.copy_(val)
        return out

    plain = entry(G.PlainAlloc(), False)
    runs = [(G.GuardedAlloc(p), False) for p in G.POISONS]
    outs = [entry(h, s) for h, s in runs]
    for (h, _), out in zip(runs, outs):
        h.check_guards()
        assert h.record_of(out).kind == "empty" and "test_gpu_memory_contract.py" in h.record_of(out).call
        compare_runs("complete", {"out": plain}, {"out": out}, {}, h)
    # one guard byte, just behind the view
    h, out = runs[0][0], outs[0]
    rec = h.record_of(out)
    rec.buffer[rec.front + rec.nbytes] = 0
    with pytest.raises(AssertionError, match=r"1 guard byte\(s\) behind the empty \(5, 7\) float32 made by test_gpu_memory_contract.py.*0 bytes past its end"):
        h.check_guards()
    rec.buffer[rec.front + rec.nbytes] = h.poison
    rec.buffer[rec.front - 1] = 0
    with pytest.raises(AssertionError, match="in front of the empty.*1 bytes before its start"):
        h.check_guards()
    # a skipped element: the guards are intact, the two-pattern comparison reports it
    skipped = []
    for p in G.POISONS:
        h = G.GuardedAlloc(p)
        skipped.append(entry(h, True))
        h.check_guards()
        with pytest.raises(AssertionError, match="out (holds 1 NaN|differs from the plain run in 1 of 35 elements, first at \\[4, 6\\])"):
            compare_runs("skipped", {"out": plain}, {"out": skipped[-1]}, {}, h)
    assert not G.same_bits(skipped[0], skipped[1])
    mask = torch.ones(5, 7, dtype=torch.bool, device=device)
    mask[4, 6] = False
    assert G.same_bits(skipped[0], skipped[1], mask) and G.holds_poison(skipped[1], 0x4B, ~mask)
    assert ops.torch is torch


# ================================================================================================================== end to end
def _forward(kind, dev):
    from test_gpu_models import make_inputs
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models import det
    from v2x_sim_amd.utils.synthetic import init_synthetic_weights
    A = {"FaFNet": 2, "V2VNet": 2, "When2com": 5}[kind]
    pm = init_synthetic_weights(getattr(det, kind)(Config("train"), **({} if kind == "FaFNet" else {"num_agent": A})), seed=4).to(dev)
    _, bev, T = make_inputs(A, 1, n_pts=4000, seed=9)
    bev, T, nat = bev.to(dev), T.to(dev), torch.full((1, A), A)

    def run():
        with torch.no_grad():
            if kind == "FaFNet":
                res = pm(bev)
            elif kind == "V2VNet":
                res = pm(bev, T, nat, batch_size=1)
            else:
                res = pm(bev, T, nat, training=False, inference="activated", batch_size=1)
        torch.cuda.synchronize()
        return {k: v for k, v in res.items() if torch.is_tensor(v)}
    return run


def _train_step(dev, tune):
    import copy
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.det import FaFNet
    from v2x_sim_amd.train import detection_loss, train_forward
    from v2x_sim_amd.train.loop import synthetic_batch_on_device
    from v2x_sim_amd.utils.synthetic import init_synthetic_weights
    tune("TRAIN_HIP", 1)
    tune("TRAIN_GRAPH", 0)
    cfg = Config("train")
    base = init_synthetic_weights(FaFNet(cfg, kd_flag=0, num_agent=2), seed=3).to(dev)
    data = synthetic_batch_on_device(cfg, 1, 2, seed=5, device=dev)

    def run():
        model = copy.deepcopy(base)
        model.train()
        res = train_forward(model, data["bev_seq"], data["trans_matrices"], data["num_agent"], 1)
        loss = detection_loss(res, data["labels"], data["reg_targets"], data["reg_loss_mask"])
        loss[0].backward()
        torch.cuda.synchronize()
        outs = {"loss%d" % k: v.detach() for k, v in enumerate(loss)}
        outs.update({"cls": res["cls"].detach(), "loc": res["loc"].detach()})
        outs.update({"grad." + k: p.grad.detach() for k, p in model.named_parameters() if p.grad is not None})
        outs.update({"buffer." + k: b.detach() for k, b in model.named_buffers() if "running" in k})
        return outs
    return run


@pytest.mark.parametrize("kind", ["FaFNet", "V2VNet", "When2com", "FaFNet-train-step"])
def test_end_to_end_under_the_harness(device, tune, kind):
    """A forward of each family and one eager HIP training step of FaFNet with the wrapper modules (only) proxied: guards intact; logits, loss,
    gradients and running statistics bit-identical to the plain run under both poison bytes."""
    run = _train_step(device, tune) if kind == "FaFNet-train-step" else _forward(kind, device)
    plain = run()
    assert any(k in plain for k in ("cls", "loss0")) and all(bool(torch.isfinite(v.float()).all()) for v in plain.values())
    compare_runs("%s, a second plain run" % kind, plain, run(), {}, None)
    for poison in G.POISONS:
        with G.GuardedAlloc(poison) as h:
            got = run()
            assert len(h.records) > 10, "the model's launches did not go through the proxied wrappers"
            h.check_guards()
        compare_runs("%s under poison 0x%02X" % (kind, poison), plain, got, {}, h)

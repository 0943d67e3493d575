"""Detection losses of upstream coperception/utils/loss.py + CoDetModule.FaFModule.loss_calculator (absent from
/root/reference; README.md:101 names the training scripts that use them).  Build-owned restatement:

  classification: softmax focal loss (alpha = 0.25 on the foreground class, gamma = 2) over every anchor,
  localisation:   smooth-L1 (sigma = 3  ->  beta = 1/9) over the anchors selected by reg_loss_mask,
  both summed and divided by the number of positive anchors (at least 1);  loss = cls + loc.
  normalizer="batch" (oracle/ASSUMPTIONS.md row 49, the second reading; configs.Config.loss_normalizer): divided by the number of maps instead.

Segmentation loss of upstream coperception/utils/SegModule.py::SegModule.step (nn.CrossEntropyLoss; absent from /root/reference as well), restated as
segmentation_loss: pixel-wise softmax cross entropy with optional class weights and ignored labels, the weighted mean over the pixels that count.
"""
import torch
import torch.nn.functional as F

ALPHA, GAMMA, SIGMA = 0.25, 2.0, 3.0


def focal_loss(cls_logits, label_one_hot):
    """cls_logits (N, M, 2) fp32, label_one_hot (N, M, 2) -> per-anchor loss (N, M)."""
    logp = F.log_softmax(cls_logits, dim=-1)
    p_t = (logp.exp() * label_one_hot).sum(-1)
    alpha_t = label_one_hot[..., 1] * ALPHA + label_one_hot[..., 0] * (1.0 - ALPHA)
    return -alpha_t * (1.0 - p_t).pow(GAMMA) * (logp * label_one_hot).sum(-1)


class _DetLossHip(torch.autograd.Function):
    """The whole loss on the hand-written kernels (csrc/det_loss.hip): forward = one pass over the five tensors + a finish launch, backward = one
    pass writing both gradients; as PyTorch ops the same arithmetic is ~45 launches over 31 + 94 MB tensors per 10-map step (0.6 ms of 5.8)."""

    @staticmethod
    def forward(ctx, cls, loc, lab, tgt, mask):
        from .. import ops
        ctx.set_materialize_grads(False)      # the gradients of unused outputs arrive as None, not as zero tensors (a fill launch each)
        out = ops.det_loss_forward(cls, lab, loc, tgt, mask, ALPHA, 1.0 / (SIGMA * SIGMA))
        ctx.save_for_backward(cls, loc, lab, tgt, mask, out)
        n_pos = out[3]
        ctx.mark_non_differentiable(n_pos)
        return out[0], out[1], out[2], n_pos

    @staticmethod
    def backward(ctx, g_loss, g_cls, g_loc, _g_npos=None):
        from .. import ops
        cls, loc, lab, tgt, mask, out = ctx.saved_tensors
        gs = [None if g is None else g.to(torch.float32).contiguous() for g in (g_loss, g_cls, g_loc)]
        dcls, dloc = ops.det_loss_backward(cls, lab, loc, tgt, mask, ALPHA, 1.0 / (SIGMA * SIGMA), out, *gs)
        return dcls, dloc, None, None, None


def _hip_loss_ok(cls, loc, labels, reg_targets, reg_loss_mask):
    from .. import tuning
    if not (cls.is_cuda and tuning.get("TRAIN_HIP") != 0 and tuning.get("TRAIN_LOSS_HIP") != 0):
        return False
    if not (cls.dtype == loc.dtype == labels.dtype == reg_targets.dtype == torch.float32 and reg_loss_mask.dtype in (torch.bool, torch.uint8)):
        return False
    n = cls.numel() // 2
    return (cls.shape[-1] == 2 and labels.numel() == 2 * n and loc.numel() == 6 * n and reg_targets.numel() == 6 * n and reg_loss_mask.numel() == n
            and loc.shape[-1] == 6)


LOSS_TYPES = ("faf_loss", "corner_loss")
WH_AXES = ("w_along_heading", "h_along_heading")


class _DetCornerLossHip(torch.autograd.Function):
    """The loss with the corner localisation term on the hand-written kernels (csrc/det_corner_loss.hip): the launches, the outputs and the handling of
    the incoming gradients are _DetLossHip's; anchors (M, 6) fp32 on the device, wh_swap a python bool."""

    @staticmethod
    def forward(ctx, cls, loc, lab, tgt, mask, anchors, wh_swap):
        from .. import ops
        ctx.set_materialize_grads(False)
        out = ops.det_corner_loss_forward(cls, lab, loc, tgt, mask, anchors, wh_swap, ALPHA)
        ctx.save_for_backward(cls, loc, lab, tgt, mask, anchors, out)
        ctx.wh_swap = wh_swap
        n_pos = out[3]
        ctx.mark_non_differentiable(n_pos)
        return out[0], out[1], out[2], n_pos

    @staticmethod
    def backward(ctx, g_loss, g_cls, g_loc, _g_npos=None):
        from .. import ops
        cls, loc, lab, tgt, mask, anchors, out = ctx.saved_tensors
        gs = [None if g is None else g.to(torch.float32).contiguous() for g in (g_loss, g_cls, g_loc)]
        dcls, dloc = ops.det_corner_loss_backward(cls, lab, loc, tgt, mask, anchors, ctx.wh_swap, ALPHA, out, *gs)
        return dcls, dloc, None, None, None, None, None


def corner_anchor_table(anchors, device, dtype=torch.float32):
    """The anchors of one map as the corner loss reads them: (X, Y, A, 6) or (M, 6), tensor or numpy -> (M, 6) contiguous on `device`."""
    a = anchors if isinstance(anchors, torch.Tensor) else torch.as_tensor(anchors)
    if a.dim() < 2 or a.shape[-1] != 6:
        raise ValueError("anchors must be (X, Y, A, 6) or (M, 6) [x, y, w, h, sin, cos], got %s" % (tuple(a.shape),))
    return a.reshape(-1, 6).to(device=device, dtype=dtype).contiguous()


def decode_corners(codes, anchors, wh_axis="w_along_heading"):
    """codes (..., M, 6), anchors (M, 6) -> (..., M, 4, 2): the 'faf' decode of utils/postprocess.py::decode_boxes followed by box_corners' four corners
    (same order, same reading of wh_axis), in differentiable PyTorch ops.  atan2(ds, dc) at ds = dc = 0 has value 0 and gradient 0 (torch's own backward
    divides 0 by 0 there): such a pair is replaced by the constants (0, 1) before the call."""
    ds, dc = codes[..., 4], codes[..., 5]
    z = (ds == 0) & (dc == 0)
    dyaw = torch.atan2(torch.where(z, torch.zeros_like(ds), ds), torch.where(z, torch.ones_like(dc), dc))
    x = anchors[:, 0] + codes[..., 0]
    y = anchors[:, 1] + codes[..., 1]
    w = anchors[:, 2] * torch.exp(torch.clamp(codes[..., 2], -4.0, 4.0))
    h = anchors[:, 3] * torch.exp(torch.clamp(codes[..., 3], -4.0, 4.0))
    yaw = torch.atan2(anchors[:, 4], anchors[:, 5]) + dyaw
    if wh_axis == "h_along_heading":
        w, h = h, w
    c, s = torch.cos(yaw)[..., None], torch.sin(yaw)[..., None]
    ox = w[..., None] * torch.tensor([0.5, -0.5, -0.5, 0.5], dtype=codes.dtype, device=codes.device)
    oy = h[..., None] * torch.tensor([0.5, 0.5, -0.5, -0.5], dtype=codes.dtype, device=codes.device)
    return torch.stack([x[..., None] + ox * c - oy * s, y[..., None] + ox * s + oy * c], -1)


def corner_distance_sum(loc, reg_targets, reg_loss_mask, anchors, wh_axis="w_along_heading"):
    """The corner localisation term before its normaliser: loc, reg_targets (N, M, 6), reg_loss_mask (N, M, 1) bool, anchors (M, 6)
    -> sum over the selected anchors of the four distances between the corners of the decoded prediction and of the decoded target.
    The codes of an unselected anchor are replaced by zeros BEFORE the decode (torch.where, not a masked sum: inf or NaN there would give inf * 0): such an
    anchor decodes to the same box twice, contributes exactly 0 and receives exactly zero gradient.  |D| at D = 0 has gradient 0 (torch's sqrt has none):
    a zero squared length is replaced by the constant 1 under the root.  No data-dependent shape, no host synchronisation: capturable."""
    x = torch.where(reg_loss_mask, loc, torch.zeros_like(loc))
    t = torch.where(reg_loss_mask, reg_targets, torch.zeros_like(reg_targets))
    d = decode_corners(x, anchors, wh_axis) - decode_corners(t, anchors, wh_axis)
    q = (d * d).sum(-1)
    zero = q == 0
    return torch.where(zero, torch.zeros_like(q), torch.sqrt(torch.where(zero, torch.ones_like(q), q))).sum()


def detection_loss(result, labels, reg_targets, reg_loss_mask, normalizer="positives", loss_type="faf_loss", anchors=None, wh_axis="w_along_heading"):
    """result: {'cls' (N, X*Y*A, 2), 'loc' (N, X, Y, A, 1, 6)};  labels (N, X, Y, A, 2);  reg_targets (N, X, Y, A, 1, 6);
    reg_loss_mask (N, X, Y, A, 1) bool  ->  (loss, cls_loss, loc_loss) scalars.  On the MI355X with the HIP training engine (TRAIN_HIP, and
    TRAIN_LOSS_HIP != 0) and fp32 operands: three launches of csrc/det_loss.hip; otherwise the PyTorch ops below (the specification).
    loss_type (configs.Config.loss_type, upstream's switch): "faf_loss" = the smooth-L1 term above; "corner_loss" = the distance between the four
    corners of the decoded prediction and of the decoded target (corner_distance_sum), same classification term, same
    normaliser.  It needs `anchors` -- (X, Y, A, 6) or (M, 6), tensor or numpy, the anchors of ONE map -- and reads `wh_axis` (Config.box_wh_axis);
    under the same switches it runs as three launches of csrc/det_corner_loss.hip."""
    if normalizer not in ("positives", "batch"):
        raise ValueError("normalizer must be 'positives' or 'batch'")
    if loss_type not in LOSS_TYPES:
        raise ValueError("loss_type must be one of %s, got %r" % (LOSS_TYPES, loss_type))
    n = result["cls"].shape[0]
    if loss_type == "corner_loss":
        if anchors is None:
            raise ValueError("loss_type='corner_loss' decodes the boxes: it needs the anchors of one map")
        if wh_axis not in WH_AXES:
            raise ValueError("wh_axis must be one of %s" % (WH_AXES,))
        loc = result["loc"]
        table = corner_anchor_table(anchors, loc.device, loc.dtype)
        if loc.numel() != n * table.shape[0] * 6:
            raise ValueError("corner_loss: loc %s does not hold %d maps of %d anchors" % (tuple(loc.shape), n, table.shape[0]))
        if _hip_loss_ok(result["cls"], loc, labels, reg_targets, reg_loss_mask):
            loss, cls_loss, loc_loss, n_pos = _DetCornerLossHip.apply(result["cls"].contiguous(), loc.contiguous(), labels.contiguous(), reg_targets.contiguous(),
                                                                      reg_loss_mask.contiguous(), table, wh_axis == "h_along_heading")
            if normalizer == "batch":
                k = n_pos / float(n)
                return loss * k, cls_loss * k, loc_loss * k
            return loss, cls_loss, loc_loss
        lab = labels.reshape(n, -1, 2).to(result["cls"].dtype)
        n_pos = lab[..., 1].sum().clamp(min=1.0) if normalizer == "positives" else torch.tensor(float(n), dtype=result["cls"].dtype, device=result["cls"].device)
        cls_loss = focal_loss(result["cls"], lab).sum() / n_pos
        loc_loss = corner_distance_sum(loc.reshape(n, -1, 6), reg_targets.reshape(n, -1, 6).to(loc.dtype), reg_loss_mask.reshape(n, -1, 1).to(torch.bool),
                                       table, wh_axis) / n_pos
        return cls_loss + loc_loss, cls_loss, loc_loss
    if _hip_loss_ok(result["cls"], result["loc"], labels, reg_targets, reg_loss_mask):
        loss, cls_loss, loc_loss, n_pos = _DetLossHip.apply(result["cls"].contiguous(), result["loc"].contiguous(), labels.contiguous(),
                                                            reg_targets.contiguous(), reg_loss_mask.contiguous())
        if normalizer == "batch":     # the kernels divide by the positives: rescale by n_pos / n (a device scalar: no synchronisation, capturable)
            k = n_pos / float(n)
            return loss * k, cls_loss * k, loc_loss * k
        return loss, cls_loss, loc_loss
    lab = labels.reshape(n, -1, 2).to(result["cls"].dtype)
    n_pos = lab[..., 1].sum().clamp(min=1.0) if normalizer == "positives" else torch.tensor(float(n), dtype=result["cls"].dtype, device=result["cls"].device)
    cls_loss = focal_loss(result["cls"], lab).sum() / n_pos
    # masked SUM instead of boolean indexing: the same terms, but no data-dependent shape -- no host synchronisation, and the step can be
    # captured in a hipGraph (train/graph_step.py).  Unselected anchors contribute exactly 0 (their terms are finite: targets are 0 there).
    m = reg_loss_mask.reshape(n, -1, 1).to(result["loc"].dtype)
    per = F.smooth_l1_loss(result["loc"].reshape(n, -1, 6), reg_targets.reshape(n, -1, 6).to(result["loc"].dtype), reduction="none",
                           beta=1.0 / (SIGMA * SIGMA))
    loc_loss = (per * m).sum() / n_pos
    return cls_loss + loc_loss, cls_loss, loc_loss


class _SegLossHip(torch.autograd.Function):
    """segmentation_loss on the hand-written kernels (csrc/seg_loss.hip): forward = one pass over logits and labels + a finish launch, backward = one pass
    writing the fp32 logit gradients (form (a); the class head fused with the loss takes form (b): train/hip_graph.py::_SegHeadLoss)."""

    @staticmethod
    def forward(ctx, logits, labels, weight):
        from .. import ops
        ctx.set_materialize_grads(False)
        out = ops.seg_loss_forward(logits, labels, weight)
        ctx.save_for_backward(logits, labels, out, *(() if weight is None else (weight,)))
        return out[0]

    @staticmethod
    def backward(ctx, g_loss):
        from .. import ops
        if g_loss is None:
            return None, None, None
        logits, labels, out = ctx.saved_tensors[:3]
        weight = ctx.saved_tensors[3] if len(ctx.saved_tensors) > 3 else None
        return ops.seg_loss_backward(logits, labels, weight, out, g_loss.to(torch.float32).contiguous()), None, None


def seg_loss_weight(weight, logits):
    """The class weights as the kernels take them: None, or an fp32 contiguous (C,) tensor on the logits' device."""
    if weight is None:
        return None
    return torch.as_tensor(weight, dtype=torch.float32, device=logits.device).contiguous()


def _hip_seg_loss_ok(logits, labels, weight):
    from .. import tuning
    if not (logits.is_cuda and tuning.get("TRAIN_HIP") != 0 and tuning.get("TRAIN_SEG_LOSS_HIP") != 0):
        return False
    if logits.dtype != torch.float32 or labels.dtype != torch.uint8 or labels.device != logits.device:
        return False
    return seg_kernels_take(logits, labels, weight)


def seg_kernels_take(logits, labels, weight, c_pad=0):
    """Whether csrc/seg_loss.hip takes these operands (contiguous forms of them): C % 4 == 0, 4 <= C <= 32, one label per pixel."""
    from .. import ops_train
    return ops_train._seg_loss_operands(logits.contiguous(), labels.contiguous(), weight, c_pad) is not None


def segmentation_loss(logits, labels, weight=None, ignore_index=255):
    """logits (..., C) fp32 NHWC, labels (...) uint8 (or any integer type on the PyTorch-op path), weight (C,) or None  ->  the scalar loss

        valid_i = label_i < C                 (every label >= C is ignored; ignore_index, 255 by convention, must be one of them)
        w_i     = valid_i * (weight[label_i] or 1),   nll_i = logsumexp(logits_i) - logits_i[label_i]
        loss    = sum w_i nll_i / (sum w_i if sum w_i > 0 else 1)

    which is F.cross_entropy(weight=, ignore_index=, reduction="mean") wherever a pixel counts, and 0 with zero gradients (not NaN) where none does.
    On the MI355X with TRAIN_HIP and TRAIN_SEG_LOSS_HIP != 0, fp32 logits and uint8 labels: three launches of csrc/seg_loss.hip; otherwise the PyTorch ops
    below (the specification): masked sums, no data-dependent shape -- no host synchronisation, capturable in a hipGraph (train/graph_step.py)."""
    Cn = logits.shape[-1]
    if not (ignore_index >= Cn or ignore_index < 0):
        raise ValueError("segmentation_loss: ignore_index %d names a class of the %d-class head" % (ignore_index, Cn))
    if tuple(labels.shape) != tuple(logits.shape[:-1]):
        raise ValueError("segmentation_loss: labels %s do not match logits %s" % (tuple(labels.shape), tuple(logits.shape)))
    w = None if weight is None else torch.as_tensor(weight, device=logits.device)
    if _hip_seg_loss_ok(logits, labels, None if w is None else w.to(torch.float32).contiguous()):
        return _SegLossHip.apply(logits.contiguous(), labels.contiguous(), seg_loss_weight(w, logits))
    lab = labels.reshape(-1).long()
    x = logits.reshape(-1, Cn)
    valid = (lab >= 0) & (lab < Cn)
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    wi = valid.to(x.dtype)
    if w is not None:
        wi = wi * w.to(x.dtype)[safe]
    nll = torch.logsumexp(x, dim=-1) - x.gather(1, safe[:, None])[:, 0]
    num, den = (wi * nll).sum(), wi.sum()
    return num / torch.where(den > 0, den, torch.ones_like(den))

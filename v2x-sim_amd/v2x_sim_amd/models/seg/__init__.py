"""BEV semantic segmentation variants (BASELINE.json config 5).

Upstream coperception/models/seg/* is not in /root/reference and its backbone widths are
unverified, so the build-owned spec reuses the detection backbone (rows a2/a6)
and replaces the det heads by a 1x1 conv 32 -> n_classes producing NHWC fp32 logits
(DESIGN.md section 3.6).  n_classes = 8 as recollected for V2X-Sim.

Every --com of detection except `late` has its class here, and every one is `class XSeg(SegHeadMixin, X)`: the detection twin (its FAMILY, its
backbone(), its forward_nhwc) with `outc` added and head() -- what forward_nhwc ends in -- answering decoder + class head instead of the detection heads.
"""
import torch
import torch.nn as nn

from ... import ops, packing, tuning
from ..._lib import V2X_EPI_F32
from ..det.base import LidarDecoder, _ParamsOnly
from ..det.FaFNet import FaFNet
from ..det.fusion import CatFusion, DiscoNet, MaxFusion, MeanFusion, SumFusion
from ..det.V2VNet import V2VNet
from ..det.When2com import When2com


class OutConv(_ParamsOnly):
    def __init__(self, cin, n_classes):
        super().__init__()
        self.conv = nn.Conv2d(cin, n_classes, kernel_size=1)


class SegHeadMixin(object):
    """The class head on a detection twin: `class XSeg(SegHeadMixin, X)`.  The twin's constructor, then `outc`; the twin's packing plus `seg` /
    `seg_fused`; the twin's forward_nhwc itself, which ends in self.head -- here decoder + 1x1 class head -> logits (N, X, Y, n_classes) fp32 NHWC
    (upstream returns NCHW; argmax / CE are layout-agnostic, and ops.seg_argmax_confusion consumes NHWC directly).  Link masks, compress_level
    and the bit-grid input (zbits) are whatever the twin takes."""

    def __init__(self, config, n_classes=8, **kw):
        super().__init__(config, **kw)
        self.n_classes = n_classes
        self.outc = OutConv(32, n_classes)

    def _pack(self, device):
        pk = super()._pack(device)
        conv = self.outc.conv
        scale, shift = packing.fold_bn(conv.bias, None, conv.out_channels)
        pk["seg"] = packing.pack_conv("outc", conv.weight, scale, shift, stride=1, pad=0, relu=False, epilogue=V2X_EPI_F32, device=device)
        pk["seg_fused"] = self._pack_fused(self.backbone()[1], device)
        return pk

    def _pack_fused(self, decoder, device):
        """conv8_2 (3x3 32 -> 32, BN, ReLU) chained with the 1x1 class head in ONE halo launch (conv_halo.hip: <0, 32, 32, 16, 2>): the 32-channel
        map is rounded to bf16 exactly as the stand-alone layer stores it but never reaches HBM (-1.3 GB written and read back per 320 maps, and the
        gather kernel's two launches for the head).  None when the head has more than 16 classes (one padded channel tile) or a class count that
        is not a multiple of 4 (the chained fp32 epilogue stores whole float4s per k-slot quarter; v2x_conv2d(halo) requires Cout2 % 4 == 0): such
        heads keep the two-layer path."""
        conv = self.outc.conv
        n_cls = conv.out_channels
        if n_cls > 16 or n_cls % 4 != 0 or decoder.conv8_2.out_channels != 32 or decoder.conv8_2.in_channels != 32:
            return None
        s1, t1 = packing.fold_bn(decoder.conv8_2.bias, decoder.bn8_2, 32)
        w2 = conv.weight.detach().float().cpu()
        b2 = conv.bias.detach().float().cpu() if conv.bias is not None else torch.zeros(n_cls)
        return packing.pack_conv_halo("decoder.conv8_2+outc", decoder.conv8_2.weight, s1, t1, relu=True, chain=(w2, torch.ones(n_cls), b2, False),
                                      epilogue=V2X_EPI_F32, device=device)

    def head(self, pk, feats):
        """Decoder + class head -> fp32 NHWC logits; conv8_2 and the head as one launch where the map tiles (tuning switch SEG_FUSE)."""
        fused = pk.get("seg_fused")
        x0 = feats[0]
        if fused is not None and tuning.get("SEG_FUSE") != 0 and ops.covers(fused, x0.shape[1], x0.shape[2]):
            return ops.conv2d(fused, LidarDecoder.run(pk["dec"], *feats, last=False))
        return ops.conv2d(pk["seg"], LidarDecoder.run(pk["dec"], *feats))


class FaFNetSeg(SegHeadMixin, FaFNet):
    pass


class V2VNetSeg(SegHeadMixin, V2VNet):
    pass


class When2comSeg(SegHeadMixin, When2com):
    """when2com / who2com with the class head: the handshake and the weighted warp-sum of the detection model (When2com.fused_feats), then
    decoder + 1x1 head.  Every constructor switch of When2com, `sparse` (sparsemax) included; a link mask raises as there.  What differs from the
    twin: forward_nhwc returns the logits (not a dict), the handshake on request, and forward has no maps / vis / MO_flag."""

    @ops.latency_entry
    def forward_nhwc(self, x0, trans_matrices, num_agent_tensor, training=True, inference="activated", batch_size=1, plan=None,
                     return_handshake=False):
        """-> logits (A*B, X, Y, n_classes) fp32 NHWC; return_handshake=True: (logits, prob, coef), the two (B, A_key, A_query)."""
        pk = self.packed(x0.device)
        feats, prob, coef = self.fused_feats(pk, x0, trans_matrices, num_agent_tensor, training, inference, batch_size, plan)
        logits = self.head(pk, feats)
        return (logits, prob, coef) if return_handshake else logits

    def forward(self, bevs, trans_matrices, num_agent_tensor, training=True, inference="activated", batch_size=1):
        return self.forward_nhwc(self._input_nhwc(bevs), trans_matrices, num_agent_tensor, training, inference, batch_size)

    def run_batch(self, data, batch_size=1, inference=None):
        logits, _, coef = self.forward_nhwc(self._input_nhwc(data["bev_seq"]), data["trans_matrices"], data["num_agent"], False,
                                            inference or "activated", batch_size, return_handshake=True)
        self.last_num_connect = self.num_connect(coef, self.agent_num)
        return logits


class SumFusionSeg(SegHeadMixin, SumFusion):
    pass


class MeanFusionSeg(SegHeadMixin, MeanFusion):
    pass


class MaxFusionSeg(SegHeadMixin, MaxFusion):
    pass


class CatFusionSeg(SegHeadMixin, CatFusion):
    pass


class DiscoNetSeg(SegHeadMixin, DiscoNet):
    pass


# --com of tools/seg/train_seg.py and eval_seg.py -> the class (who2com is a When2comSeg evaluated with inference 'argmax_test', as in tools/det/test_codet.py)
COM_CLASSES = {"lowerbound": FaFNetSeg, "upperbound": FaFNetSeg, "v2v": V2VNetSeg, "when2com": When2comSeg, "who2com": When2comSeg,
               "sum": SumFusionSeg, "mean": MeanFusionSeg, "max": MaxFusionSeg, "cat": CatFusionSeg, "disco": DiscoNetSeg}


def default_inference(com):
    return "argmax_test" if com == "who2com" else "activated"

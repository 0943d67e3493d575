"""Simple intermediate-fusion baselines -- mirrors of upstream coperception/models/det/
{SumFusion,MeanFusion,MaxFusion,CatFusion}.py on base/FusionBase.py (absent from /root/reference; README.md:101 lists
the benchmark family).  Per ego agent: the ego map and every neighbour's map warped into the ego frame are reduced by
sum / mean / max; CatFusion concatenates the ego map with that mean and applies a 1x1 conv + BN + ReLU
(ModulationLayer3).  From recollection upstream's list STARTS with the ego map; frozen here.

MI355X mapping: the whole reduction is ONE warp_fuse launch (modes WSUM with unit coefficients / MEAN / MAX; the ego
term is read unwarped), and CatFusion's concat is the two-source loader of the 1x1 implicit-GEMM layer.
"""
import torch
import torch.nn as nn

from ... import ops, packing
from ..._lib import V2X_FUSE_MAX, V2X_FUSE_MEAN, V2X_FUSE_WSUM
from .base import IntermediateModelBase, LidarDecoder, LidarEncoder, _ParamsOnly  # noqa: F401


class FusionBase(IntermediateModelBase):
    FUSE_MODE = None

    def __init__(self, config, layer=3, in_channels=13, kd_flag=0, num_agent=5, compress_level=0, only_v2i=False):
        super().__init__(config, layer, in_channels, kd_flag=kd_flag, num_agent=num_agent,
                         compress_level=compress_level, only_v2i=only_v2i)

    def _pack(self, device):
        return {"enc": self.u_encoder.pack("u_encoder.", device), "dec": self.decoder.pack("decoder.", device),
                "heads": self._pack_heads(device)}

    def make_plan(self, num_agent_tensor, batch_size, device):
        A = self.agent_num
        counts, items, rows = self.frame_plan(num_agent_tensor, batch_size, A)
        coef = torch.zeros((len(items), A), dtype=torch.float32)
        L = self.links(batch_size)
        for m, (a, f) in enumerate(items):
            coef[m, :counts[f]] = 1.0        # ego included
            if L is not None:                # link mask: the fusion list is the ego and the linked neighbours (mean divides by its length)
                for j in range(counts[f]):
                    if j != a and not L[f][a][j]:
                        coef[m, j] = 0.0
        full = len(items) == A * batch_size
        plan = {"items": ops.items_tensor(items, A, batch_size, device), "coef": coef.to(device),
                "rows": None if full else torch.tensor(rows, device=device)}
        return self._finish_plan(plan, batch_size, device)

    def _finish_plan(self, plan, batch_size, device):
        return self.channel_plan(plan, batch_size, device)

    def post_fusion(self, ego, fused, pk):
        return fused

    def fuse(self, feat, trans_matrices, plan, batch_size, pk):
        fused = ops.warp_fuse(feat, self.agent_num, batch_size, trans_matrices.to(torch.float32).contiguous(),
                              plan["items"], plan["coef"], self.FUSE_MODE)
        rows = plan["rows"]
        ego = feat if rows is None else feat.index_select(0, rows)
        out = self.post_fusion(ego, fused, pk)
        if rows is None:
            return out
        cur = feat.clone()
        cur.index_copy_(0, rows, out)
        return cur

    @ops.latency_entry
    def forward_nhwc(self, x0, trans_matrices, num_agent_tensor, batch_size=1, plan=None):
        pk = self.packed(x0.device)
        feats = LidarEncoder.run(pk["enc"], x0)
        if plan is None:
            plan = self.make_plan(num_agent_tensor, batch_size, x0.device)
        plan, trans_matrices = self.degrade(plan, trans_matrices)
        feats[self.layer] = self.fuse(feats[self.layer], trans_matrices, plan, batch_size, pk)
        return self.head(pk, feats)

    def forward(self, bevs, trans_matrices, num_agent_tensor, batch_size=1):
        return self.forward_nhwc(self._input_nhwc(bevs), trans_matrices, num_agent_tensor, batch_size)


class SumFusion(FusionBase):
    FAMILY, FUSE_MODE = "fusion", V2X_FUSE_WSUM


class MeanFusion(FusionBase):
    FAMILY, FUSE_MODE = "fusion", V2X_FUSE_MEAN


class MaxFusion(FusionBase):
    FAMILY, FUSE_MODE = "fusion", V2X_FUSE_MAX


class ModulationLayer3(_ParamsOnly):
    def __init__(self, channel=256):
        super().__init__()
        self.conv1_1 = nn.Conv2d(2 * channel, channel, kernel_size=1, stride=1, padding=0)
        self.bn1_1 = nn.BatchNorm2d(channel)


class CatFusion(FusionBase):
    FAMILY, FUSE_MODE = "fusion", V2X_FUSE_MEAN

    def __init__(self, config, layer=3, in_channels=13, kd_flag=0, num_agent=5, compress_level=0, only_v2i=False):
        super().__init__(config, layer, in_channels, kd_flag, num_agent, compress_level, only_v2i)
        self.modulation_layer_3 = ModulationLayer3(self.fusion_shape()[0])

    def _pack(self, device):
        pk = super()._pack(device)
        c = self.fusion_shape()[0]
        m = self.modulation_layer_3
        pk["mod"] = packing.pack_conv_bn("modulation_layer_3.conv1_1", m.conv1_1, m.bn1_1, C0=c, C1=c, device=device)
        return pk

    def post_fusion(self, ego, fused, pk):
        return ops.conv2d(pk["mod"], ego, fused)     # cat(ego, mean) never exists: two-source 1x1 conv


class PixelWeightedFusionSoftmax(_ParamsOnly):
    def __init__(self, channel=256):
        super().__init__()
        self.conv1_1 = nn.Conv2d(channel * 2, 128, 1)
        self.bn1_1 = nn.BatchNorm2d(128)
        self.conv1_2 = nn.Conv2d(128, 32, 1)
        self.bn1_2 = nn.BatchNorm2d(32)
        self.conv1_3 = nn.Conv2d(32, 8, 1)
        self.bn1_3 = nn.BatchNorm2d(8)
        self.conv1_4 = nn.Conv2d(8, 1, 1)


class DiscoNet(FusionBase):
    """DiscoNet's pixel-wise weighted fusion (upstream coperception/models/det/DiscoNet.py) without the distillation teacher
    (kd_flag must be 0: the teacher / KD loss is out of scope).

    MI355X mapping: one warp_fuse launch materialises every (ego, source) map (one-hot coefficients; the ego's own map is
    copied unwarped), the four 1x1 convs run as implicit-GEMM layers over the (item x source) batch with the concat as the
    two-source loader, and v2x_pixel_weighted_fuse does exp / normalise / weighted sum per pixel."""
    FAMILY, FUSE_MODE = "disco", V2X_FUSE_WSUM

    def __init__(self, config, layer=3, in_channels=13, kd_flag=0, num_agent=5, compress_level=0, only_v2i=False):
        super().__init__(config, layer, in_channels, kd_flag, num_agent, compress_level, only_v2i)
        self.pixel_weighted_fusion = PixelWeightedFusionSoftmax(self.fusion_shape()[0])

    def _pack(self, device):
        pk = super()._pack(device)
        c = self.fusion_shape()[0]
        m = self.pixel_weighted_fusion
        w4 = torch.zeros((4, 8, 1, 1))                       # the 1-channel score padded to the kernel's 4-channel store quantum
        w4[0] = m.conv1_4.weight.detach().float().cpu()[0]
        b4 = torch.zeros(4)
        b4[0] = float(m.conv1_4.bias.detach()[0])
        pk["pw"] = [packing.pack_conv_bn("pixel_weighted_fusion.conv1_1", m.conv1_1, m.bn1_1, C0=c, C1=c, device=device),
                    packing.pack_conv_bn("pixel_weighted_fusion.conv1_2", m.conv1_2, m.bn1_2, device=device),
                    packing.pack_conv_bn("pixel_weighted_fusion.conv1_3", m.conv1_3, m.bn1_3, device=device),
                    packing.pack_conv("pixel_weighted_fusion.conv1_4", w4, torch.ones(4), b4, stride=1, pad=0, relu=True,
                                      epilogue=packing.V2X_EPI_F32, device=device)]
        return pk

    def make_plan(self, num_agent_tensor, batch_size, device):
        plan = super().make_plan(num_agent_tensor, batch_size, device)
        A = self.agent_num
        n = plan["items"].shape[0]
        # virtual items (m, k): the map of source k in the frame of ego item m  ->  one-hot coefficient rows
        plan["items2"] = plan["items"].repeat_interleave(A, 0).contiguous()
        valid = plan["coef"]                                               # (n, A): 1 for real agents
        plan["coef2"] = (torch.eye(A, device=device).repeat(n, 1) * valid.repeat_interleave(A, 0)).contiguous()
        plan["valid"] = valid.contiguous()
        return self.channel_plan(plan, batch_size, device, coef2="coef2", also=("valid",))

    def _finish_plan(self, plan, batch_size, device):
        return plan                      # the condition is attached once the one-hot rows exist (make_plan above)

    def fuse(self, feat, trans_matrices, plan, batch_size, pk):
        A = self.agent_num
        maps = ops.warp_fuse(feat, A, batch_size, trans_matrices.to(torch.float32).contiguous(), plan["items2"], plan["coef2"],
                             V2X_FUSE_WSUM)                                 # (n*A, H, W, C): source k in ego m's frame
        rows = plan["rows"]
        ego = feat if rows is None else feat.index_select(0, rows)
        x = ops.conv2d(pk["pw"][0], ego.repeat_interleave(A, 0).contiguous(), maps)
        x = ops.conv2d(pk["pw"][1], x)
        x = ops.conv2d(pk["pw"][2], x)
        scores = ops.conv2d(pk["pw"][3], x)                                # (n*A, H, W, 4) fp32, channel 0 = the score
        n, H, W, C = ego.shape
        out = ops.pixel_weighted_fuse(scores.view(n, A, H, W, 4), plan["valid"], maps.view(n, A, H, W, C))
        if rows is None:
            return out
        cur = feat.clone()
        cur.index_copy_(0, rows, out)
        return cur

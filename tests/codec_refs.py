"""References for the communication limits (compress_level, only_v2i, link masks): the oracle's OWN operations, composed here because
oracle/ is frozen.

* CodecEncoder: oracle LidarEncoder + the four upstream modules; forward = the parent's sequence, then two R.cbr calls on x_3 (x_4 has been
  computed from the uncompressed x_3 by then).
* apply_links: FusionBase.forward / V2VNet.fuse of the oracle with the neighbour loops taking L[b][i][j] ("ego i of frame b receives from j").
* codec_fp64 / unpack_codec: the kernel's arithmetic in float64 and the documented K-slot map of its packed weights.
"""
import numpy as np
import torch
import torch.nn as nn

from oracle import coperception_ref as R


class CodecEncoder(R.LidarEncoder):
    def __init__(self, height_feat_size=13, compress_level=0):
        super().__init__(height_feat_size)
        self.compress_level = compress_level
        if compress_level > 0:
            cc = 256 >> compress_level
            self.com_compresser = nn.Conv2d(256, cc, 1)
            self.bn_compress = nn.BatchNorm2d(cc)
            self.com_decompresser = nn.Conv2d(cc, 256, 1)
            self.bn_decompress = nn.BatchNorm2d(256)

    def forward(self, x, emulate=False):
        feats = super().forward(x, emulate)
        if self.compress_level > 0:
            m = R.cbr(feats[3], self.com_compresser, self.bn_compress, emulate)
            feats[3] = R.cbr(m, self.com_decompresser, self.bn_decompress, emulate)
        return feats


def with_codec(om, compress_level, in_channels=13):
    """Replace the reference model's u_encoder by the codec subclass (before load_state_dict)."""
    om.u_encoder = CodecEncoder(in_channels, compress_level)
    return om


def only_v2i_mask(B, A):
    L = torch.zeros((B, A, A), dtype=torch.bool)
    L[:, 0, :] = True
    L[:, :, 0] = True
    return L


def _fusion_forward(self, L, bevs, trans_matrices, num_agent_tensor, batch_size=1):
    """R.FusionBase.forward with the link test in the neighbour loop."""
    e = self.emulate_bf16
    bevs = bevs.permute(0, 1, 4, 2, 3)
    enc = self.u_encoder(bevs, e)
    lcm = self.local_com_mat(enc[self.layer], batch_size)
    size = (1,) + tuple(lcm.shape[2:])
    update = lcm.clone()
    for b in range(batch_size):
        n = int(num_agent_tensor[b, 0])
        for i in range(n):
            feats = [lcm[b, i]]
            for j in range(n):
                if j != i and bool(L[b][i][j]):
                    feats.append(R.feature_transformation(lcm[b, j], trans_matrices[b, i][j], size))
            update[b, i] = self.fusion(feats)
    x = self.decode_heads(enc, self.agents_to_batch(update))
    return self.get_cls_loc_result(x)


def _v2v_fuse(self, L, local_com_mat, trans_matrices, num_agent_tensor, batch_size):
    """R.V2VNet.fuse with the link test in the neighbour loop (an ego without a link: torch.stack of an empty list raises)."""
    e = self.emulate_bf16
    size = (1,) + tuple(local_com_mat.shape[2:])
    update = local_com_mat.clone()
    for b in range(batch_size):
        n = int(num_agent_tensor[b, 0])
        feats = [local_com_mat[b, k] for k in range(self.agent_num)]
        for _ in range(self.gnn_iter_num):
            updated = []
            for i in range(n):
                all_warp = trans_matrices[b, i]
                nb_list = []
                for j in range(n):
                    if j != i and bool(L[b][i][j]):
                        src = feats[j] if self.neighbor_source == "updated" else local_com_mat[b, j]
                        nb_list.append(R.feature_transformation(src, all_warp[j], size))
                mean_feat = R._q(torch.mean(torch.stack(nb_list), dim=0), e)
                ego = local_com_mat[b, i] if self.neighbor_source == "frozen" else feats[i]
                cat_feat = torch.cat([ego, mean_feat], dim=0).unsqueeze(0)
                updated.append(self.convgru(cat_feat, None, e).squeeze(0))
            feats = updated + feats[n:]
        for k in range(n):
            update[b, k] = feats[k]
    return update


def apply_links(om, L):
    """L (B, A, A) bool: the reference model `om` (an R.FusionBase family member or an R.V2VNet / V2VNetSeg) honours it from now on."""
    if isinstance(om, R.V2VNet):
        om.fuse = lambda *a, **k: _v2v_fuse(om, L, *a, **k)
    elif isinstance(om, R.FusionBase):
        om.forward = lambda *a, **k: _fusion_forward(om, L, *a, **k)
    else:
        raise TypeError("no masked reference for %s" % type(om).__name__)
    return om


# ---- the kernel's arithmetic ------------------------------------------------------------------------------------------------------------
def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def codec_stage_fp64(x_bf16, w, scale, shift):
    """relu((x . w^T) * scale + shift) in float64 on bf16 operands (x given as bf16, w rounded to bf16 here), not rounded."""
    y = x_bf16.double() @ w.to(torch.bfloat16).double().t()
    return torch.relu(y * scale.double() + shift.double())


def unpack_codec(wpack, C, Cc):
    """The packed fragments (uint16 / bf16 viewed as a flat tensor) -> (Wc [Cc, C], Wd [C, Cc]) through the documented map
    (include/v2x_amd.h): stage one fragment (i, ks), lane 16 q + j, element e = Wc[16 i + j][32 ks + 8 q + e]; stage two fragment (i, c),
    element e = 4 h + r = Wd[16 i + j][32 c + 16 h + 4 q + r].  Padding entries must be zero (asserted)."""
    w = wpack.view(torch.bfloat16).float().reshape(-1, 64, 8)
    ks1, ct1, ks2, ct2 = C // 32, max(Cc // 16, 1), max(Cc // 32, 1), C // 16
    assert w.shape[0] == ct1 * ks1 + ct2 * ks2
    wc = torch.zeros((16 * ct1, C))
    wd = torch.zeros((C, 32 * ks2))
    for i in range(ct1):
        for ks in range(ks1):
            fr = w[i * ks1 + ks]
            for lane in range(64):
                q, j = lane >> 4, lane & 15
                wc[16 * i + j, 32 * ks + 8 * q:32 * ks + 8 * q + 8] = fr[lane]
    for i in range(ct2):
        for c in range(ks2):
            fr = w[ct1 * ks1 + i * ks2 + c]
            for lane in range(64):
                q, j = lane >> 4, lane & 15
                for e in range(8):
                    wd[16 * i + j, 32 * c + 16 * (e >> 2) + 4 * q + (e & 3)] = fr[lane, e]
    assert float(wc[Cc:].abs().max() if wc.shape[0] > Cc else 0.0) == 0.0
    assert float(wd[:, Cc:].abs().max() if wd.shape[1] > Cc else 0.0) == 0.0
    return wc[:Cc], wd[:, :Cc]


def codec_modules(C, Cc, seed):
    """Seeded conv / BN pairs for kernel tests: weights He-normal, BN non-trivial, both pre-activations take both signs."""
    g = torch.Generator().manual_seed(seed)
    conv_c, bn_c, conv_d, bn_d = nn.Conv2d(C, Cc, 1), nn.BatchNorm2d(Cc), nn.Conv2d(Cc, C, 1), nn.BatchNorm2d(C)
    with torch.no_grad():
        for conv in (conv_c, conv_d):
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * float(np.sqrt(2.0 / conv.in_channels)))
            conv.bias.copy_(torch.randn(conv.bias.shape, generator=g) * 0.05)
        for bn in (bn_c, bn_d):
            bn.weight.copy_(torch.rand(bn.weight.shape, generator=g) * 0.5 + 0.75)
            bn.bias.copy_(torch.randn(bn.bias.shape, generator=g) * 0.1)
            bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=g) * 0.1)
            bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=g) * 0.5 + 0.75)
    for m in (conv_c, bn_c, conv_d, bn_d):
        m.eval()
    return conv_c, bn_c, conv_d, bn_d


def e2e_noise(om, bev, T, nat, B, keys=("cls", "loc")):
    """The reference's own bf16 noise: emulate=True against emulate=False, (max, mean) of |diff| relative to max|fp32 ref| per key."""
    out = {}
    with torch.no_grad():
        om.emulate_bf16 = True
        a = om(bev, T, nat, batch_size=B)
        om.emulate_bf16 = False
        b = om(bev, T, nat, batch_size=B)
    if not isinstance(a, dict):
        a, b, keys = {"logits": a}, {"logits": b}, ("logits",)
    for k in keys:
        scale = float(b[k].abs().max())
        d = (a[k].float() - b[k].float()).abs()
        out[k] = (float(d.max()) / scale, float(d.mean()) / scale)
    return out


def emulate_codec_lanes(wpack, ss, x_bf16, C, Cc):
    """The kernel's data path for ONE 16-pixel fragment, lane by lane, on the packed buffers: v_mfma_f32_16x16x32_bf16 takes A[m = j][k = 8 q + e]
    and B[k = 8 q + e][n = j] from lane 16 q + j and leaves D[m = 4 q + r][n = j] in it.  Stage two's B fragment of chunk c is BUILT FROM THE
    LANE'S OWN stage-one results (tiles 2 c and 2 c + 1), with no exchange between lanes -- which is only right if the packed decompress
    weights are in that slot order.  x_bf16 (16, C) -> (msg (16, Cc), y (16, C)) float64, un-rounded y / rounded msg."""
    w = wpack.view(torch.bfloat16).double().reshape(-1, 64, 8)
    ss = ss.double()
    ks1, ct1, ks2, ct2 = C // 32, max(Cc // 16, 1), max(Cc // 32, 1), C // 16
    sc1, sf1, sc2, sf2 = ss[:16 * ct1], ss[16 * ct1:32 * ct1], ss[32 * ct1:32 * ct1 + C], ss[32 * ct1 + C:]
    x = x_bf16.double()

    def mfma(afrag, bfrag):                        # [lane][8] each -> D as [lane][4]
        A = torch.zeros(16, 32, dtype=torch.float64)
        B = torch.zeros(32, 16, dtype=torch.float64)
        for lane in range(64):
            q, j = lane >> 4, lane & 15
            A[j, 8 * q:8 * q + 8] = afrag[lane]
            B[8 * q:8 * q + 8, j] = bfrag[lane]
        D = A @ B
        return torch.stack([torch.stack([D[4 * (lane >> 4) + r, lane & 15] for r in range(4)]) for lane in range(64)])

    lanes = torch.arange(64)
    q, j = lanes >> 4, lanes & 15
    own = torch.zeros(ct1, 64, 4, dtype=torch.float64)             # stage-one results a lane holds: tile i, channels 16 i + 4 q + r
    for i in range(ct1):
        acc = torch.zeros(64, 4, dtype=torch.float64)
        for ks in range(ks1):
            bfrag = torch.stack([x[j[l], 32 * ks + 8 * q[l]:32 * ks + 8 * q[l] + 8] for l in range(64)])
            acc += mfma(w[i * ks1 + ks], bfrag)
        ch = (16 * i + 4 * q)[:, None] + torch.arange(4)[None]
        own[i] = bf16_round(torch.relu(acc * sc1[ch] + sf1[ch]).float()).double()
    msg = torch.zeros(16, 16 * ct1, dtype=torch.float64)
    for i in range(ct1):
        for l in range(64):
            msg[j[l], 16 * i + 4 * q[l]:16 * i + 4 * q[l] + 4] = own[i, l]
    y = torch.zeros(16, C, dtype=torch.float64)
    for i in range(ct2):
        acc = torch.zeros(64, 4, dtype=torch.float64)
        for c in range(ks2):
            hi = own[2 * c + 1] if 2 * c + 1 < ct1 else torch.zeros(64, 4, dtype=torch.float64)
            acc += mfma(w[ct1 * ks1 + i * ks2 + c], torch.cat([own[2 * c], hi], 1))      # the lane's own registers, nothing else
        ch = (16 * i + 4 * q)[:, None] + torch.arange(4)[None]
        out = torch.relu(acc * sc2[ch] + sf2[ch])
        for l in range(64):
            y[j[l], 16 * i + 4 * q[l]:16 * i + 4 * q[l] + 4] = out[l]
    return msg[:, :Cc], y

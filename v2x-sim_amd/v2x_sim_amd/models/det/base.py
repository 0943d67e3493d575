"""Host-side mirror of upstream coperception/models/det/backbone/Backbone.py and
coperception/models/det/base/{DetModelBase,IntermediateModelBase,NonIntermediateModelBase}.py
(not present in /root/reference; README.md:101 names the benchmarks they implement).

The nn.Module tree below exists to hold parameters under the upstream attribute names
(`u_encoder.conv1_1.weight`, `decoder.bn5_1.running_var`, `classification.conv1.weight`,
`regression.box_prediction.0.weight`, ...) so upstream-style checkpoints / optimizers see the
same state_dict.  None of these torch modules is ever *called*: forward() packs the
parameters once (packing.py) and runs the hand-written HIP kernels through ops.py.  On a
machine without the MI355X library the forward raises -- there is no eager fallback.
"""
import torch
import torch.nn as nn

from ... import ops, packing
from ...ops import V2X_EPI_BF16, V2X_EPI_F32  # noqa: F401

INPUT_C_PAD = 32  # BEV height bins (13) zero-padded to one MFMA k-step of channels
LAYER_SHAPES = {0: (32, 256, 256), 1: (64, 128, 128), 2: (128, 64, 64), 3: (256, 32, 32), 4: (512, 16, 16)}


class _ParamsOnly(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover - guard
        raise RuntimeError("%s is a parameter container; the compute path is the HIP engine of the owning model"
                           % type(self).__name__)


class Conv3D(_ParamsOnly):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv3d = nn.Conv3d(cin, cout, kernel_size=(1, 1, 1), stride=1, padding=(0, 0, 0))
        self.bn3d = nn.BatchNorm3d(cout)


class LidarEncoder(_ParamsOnly):
    """13 -> 32,32 @256^2 -> 64,64 (+1x1) @128^2 -> 128,128 (+1x1) @64^2 -> 256,256 @32^2 -> 512,512 @16^2."""

    def __init__(self, height_feat_size=13, compress_level=0):
        super().__init__()
        try:
            import operator
            level = operator.index(compress_level)          # python and numpy integers
        except TypeError:
            level = -1
        if isinstance(compress_level, bool) or not 0 <= level <= 8:
            raise ValueError("compress_level must be an integer in 0..8, got %r" % (compress_level,))
        compress_level = level
        self.height_feat_size = height_feat_size
        self.compress_level = compress_level
        self.conv_pre_1 = nn.Conv2d(height_feat_size, 32, 3, 1, 1)
        self.conv_pre_2 = nn.Conv2d(32, 32, 3, 1, 1)
        self.bn_pre_1 = nn.BatchNorm2d(32)
        self.bn_pre_2 = nn.BatchNorm2d(32)
        self.conv3d_1 = Conv3D(64, 64)
        self.conv3d_2 = Conv3D(128, 128)
        self.conv1_1 = nn.Conv2d(32, 64, 3, 2, 1)
        self.conv1_2 = nn.Conv2d(64, 64, 3, 1, 1)
        self.conv2_1 = nn.Conv2d(64, 128, 3, 2, 1)
        self.conv2_2 = nn.Conv2d(128, 128, 3, 1, 1)
        self.conv3_1 = nn.Conv2d(128, 256, 3, 2, 1)
        self.conv3_2 = nn.Conv2d(256, 256, 3, 1, 1)
        self.conv4_1 = nn.Conv2d(256, 512, 3, 2, 1)
        self.conv4_2 = nn.Conv2d(512, 512, 3, 1, 1)
        for n, c in (("1_1", 64), ("1_2", 64), ("2_1", 128), ("2_2", 128),
                     ("3_1", 256), ("3_2", 256), ("4_1", 512), ("4_2", 512)):
            setattr(self, "bn" + n, nn.BatchNorm2d(c))
        if compress_level > 0:
            # upstream's communication codec on x_3: the MESSAGE is the (256 >> k)-channel map between the two
            cc = 256 >> compress_level
            self.com_compresser = nn.Conv2d(256, cc, kernel_size=1, stride=1)
            self.bn_compress = nn.BatchNorm2d(cc)
            self.com_decompresser = nn.Conv2d(cc, 256, kernel_size=1, stride=1)
            self.bn_decompress = nn.BatchNorm2d(256)

    def pack(self, prefix, device):
        """-> list of ops.Layer.  Full-resolution layers carry a halo-kernel packing next to the
        gather-kernel one; conv1_2 + the 1x1x1 conv3d_1 are one fused layer when the halo kernel runs."""
        L = packing.layer_conv_bn
        cin_pad = INPUT_C_PAD
        plan = [L(prefix + "conv_pre_1", self.conv_pre_1, self.bn_pre_1, cin_pad=cin_pad, device=device),
                L(prefix + "conv_pre_2", self.conv_pre_2, self.bn_pre_2, device=device)]
        levels = [plan]
        for lvl in ("1", "2", "3", "4"):
            c1, b1 = getattr(self, "conv%s_1" % lvl), getattr(self, "bn%s_1" % lvl)
            c2, b2 = getattr(self, "conv%s_2" % lvl), getattr(self, "bn%s_2" % lvl)
            stage = [L(prefix + "conv%s_1" % lvl, c1, b1, device=device)]
            if lvl == "1":
                # 64 -> 64 3x3, then the 1x1x1 "Conv3D" 64 -> 64: chained in the streamed kernel's epilogue
                c3 = self.conv3d_1
                fb = [packing.pack_conv_bn(prefix + "conv1_2", c2, b2, device=device),
                      packing.pack_conv_bn(prefix + "conv3d_1", c3.conv3d, c3.bn3d, device=device)]
                s1, t1 = packing.fold_bn(c2.bias, b2, c2.out_channels)
                s2, t2 = packing.fold_bn(c3.conv3d.bias, c3.bn3d, c3.conv3d.out_channels)
                # resident-weights 8-wave ping-pong halo kernel, 1x1 chained in its store phase
                halo = packing.pack_conv_halo(prefix + "conv1_2+conv3d_1", c2.weight, s1, t1, relu=True,
                                              chain=(c3.conv3d.weight[:, :, 0], s2, t2, True), device=device)
                stage.append(ops.Layer(fb, halo, name=prefix + "conv1_2+conv3d_1"))
            elif lvl == "2" and packing.CHAIN_STREAM and packing.STREAM_KERNEL:
                # 128 -> 128 3x3, then the 1x1x1 "Conv3D" 128 -> 128: chained in the streamed kernel's epilogue (the
                # intermediate map never reaches HBM: -2 x 1 MB per map and one launch less)
                c3 = self.conv3d_2
                fb = [packing.pack_conv_bn(prefix + "conv2_2", c2, b2, device=device),
                      packing.pack_conv_bn(prefix + "conv3d_2", c3.conv3d, c3.bn3d, device=device)]
                s1, t1 = packing.fold_bn(c2.bias, b2, c2.out_channels)
                s2, t2 = packing.fold_bn(c3.conv3d.bias, c3.bn3d, c3.conv3d.out_channels)
                halo = packing.pack_conv_stream(prefix + "conv2_2+conv3d_2", c2.weight, s1, t1, relu=True,
                                                chain=(c3.conv3d.weight[:, :, 0], s2, t2, True), device=device)
                stage.append(ops.Layer(fb, halo, name=prefix + "conv2_2+conv3d_2"))
            else:
                stage.append(L(prefix + "conv%s_2" % lvl, c2, b2, device=device))
                if lvl == "2":
                    c3 = self.conv3d_2
                    stage.append(ops.Layer([packing.pack_conv_bn(prefix + "conv3d_2", c3.conv3d, c3.bn3d, device=device)]))
            levels.append(stage)
        if self.compress_level > 0:
            # after the five stages: the codec of x_3 (run() applies it once x_4 has been computed from the uncompressed x_3)
            levels.append(packing.pack_codec(prefix + "codec", self.com_compresser, self.bn_compress, self.com_decompresser,
                                             self.bn_decompress, device=device))
        return levels

    @staticmethod
    def run(levels, x, zbits=0):
        """x: (N, X, Y, INPUT_C_PAD) bf16 NHWC, or the voxelizer's int32 bit grid (N, X, Y) with zbits height bins
        (conv_pre_1 then expands the bits while filling its LDS patch) -> [x, x_1, x_2, x_3, x_4].  compress_level > 0: x_3 is the
        map after compress / decompress (every agent's, the ego's included), x_4 comes from the uncompressed one."""
        feats = []
        codec = levels[5] if len(levels) > 5 else None
        for stage in levels[:5]:
            k = 0
            if stage is levels[0] and len(stage) == 2 and ops.pair_eligible(stage[0].halo, stage[1].halo, x, zbits):
                # conv_pre_1 -> conv_pre_2 in one launch, the 32-channel intermediate stays in LDS (conv_halo_pair.hip)
                x = ops.conv2d_pair(stage[0].halo, stage[1].halo, x, zbits)
                k = 2
            for layer in stage[k:]:
                x = ops.run_layer(layer, x, zbits=zbits if x.dtype == torch.int32 else 0)
            feats.append(x)
        if codec is not None:
            feats[3] = ops.codec(codec, feats[3])
        return feats


class LidarDecoder(_ParamsOnly):
    """4 x [nearest x2 upsample, concat skip, conv+BN+ReLU x2]; the upsample+concat never exists
    in memory -- the first conv of each level reads both sources directly."""

    def __init__(self, height_feat_size=13):
        super().__init__()
        self.conv5_1 = nn.Conv2d(512 + 256, 256, 3, 1, 1)
        self.conv5_2 = nn.Conv2d(256, 256, 3, 1, 1)
        self.conv6_1 = nn.Conv2d(256 + 128, 128, 3, 1, 1)
        self.conv6_2 = nn.Conv2d(128, 128, 3, 1, 1)
        self.conv7_1 = nn.Conv2d(128 + 64, 64, 3, 1, 1)
        self.conv7_2 = nn.Conv2d(64, 64, 3, 1, 1)
        self.conv8_1 = nn.Conv2d(64 + 32, 32, 3, 1, 1)
        self.conv8_2 = nn.Conv2d(32, 32, 3, 1, 1)
        for n, c in (("5_1", 256), ("5_2", 256), ("6_1", 128), ("6_2", 128),
                     ("7_1", 64), ("7_2", 64), ("8_1", 32), ("8_2", 32)):
            setattr(self, "bn" + n, nn.BatchNorm2d(c))

    def pack(self, prefix, device):
        L = packing.layer_conv_bn
        plan = []
        for lvl, (cup, cskip) in (("5", (512, 256)), ("6", (256, 128)), ("7", (128, 64)), ("8", (64, 32))):
            plan.append(L(prefix + "conv%s_1" % lvl, getattr(self, "conv%s_1" % lvl), getattr(self, "bn%s_1" % lvl),
                          C0=cup, C1=cskip, up0=1, device=device))
            plan.append(L(prefix + "conv%s_2" % lvl, getattr(self, "conv%s_2" % lvl), getattr(self, "bn%s_2" % lvl),
                          device=device))
        return plan

    @staticmethod
    def run(plan, x, x_1, x_2, x_3, x_4, last=True):
        """last=False stops before conv8_2 (DetModelBase.decode_heads then runs conv8_2 + the heads as one launch)."""
        it = iter(plan)
        y = x_4
        for skip in (x_3, x_2, x_1, x):
            y = ops.run_layer(next(it), y, skip)
            if skip is x and not last:
                return y
            y = ops.run_layer(next(it), y)
        return y


class ClassificationHead(_ParamsOnly):
    def __init__(self, config):
        super().__init__()
        channel = 32
        self.conv1 = nn.Conv2d(channel, channel, kernel_size=3, stride=1, padding=1)
        self.conv2 = nn.Conv2d(channel, config.category_num * len(config.anchor_size), kernel_size=1, stride=1,
                               padding=0)
        self.bn1 = nn.BatchNorm2d(channel)


class SingleRegressionHead(_ParamsOnly):
    def __init__(self, config):
        super().__init__()
        channel = 32
        out_seq_len = 1 if config.only_det else config.pred_len
        self.box_prediction = nn.Sequential(
            nn.Conv2d(channel, channel, kernel_size=3, stride=1, padding=1), nn.BatchNorm2d(channel), nn.ReLU(),
            nn.Conv2d(channel, len(config.anchor_size) * config.box_code_size * out_seq_len, kernel_size=1,
                      stride=1, padding=0))


class DetModelBase(nn.Module):
    """Abstract detection model (upstream DetModelBase): heads + agent<->batch helpers + the
    packed-parameter cache shared by every concrete model."""
    # what a model says about itself ONCE; the training engines (train/graph.py, train/hip_graph.py) and the step modules (utils/) ask it instead
    # of probing attributes.  "faf" | "v2v" | "when2com" | "fusion" | "disco" on the concrete classes, None on the abstract bases
    FAMILY = None
    last_num_connect = None        # when2com segmentation variants: the communication rate of the last run_batch()

    def __init__(self, config, layer=3, in_channels=13, kd_flag=True, p_com_outage=0.0, num_agent=5,
                 only_v2i=False):
        super().__init__()
        if kd_flag not in (0, False):
            raise NotImplementedError("knowledge distillation (DiscoNet teacher) is out of scope (DESIGN.md s8)")
        self.motion_state = config.motion_state
        self.out_seq_len = 1 if config.only_det else config.pred_len
        self.box_code_size = config.box_code_size
        self.category_num = config.category_num
        self.use_map = config.use_map
        self.anchor_num_per_loc = len(config.anchor_size)
        self.classification = ClassificationHead(config)
        self.regression = SingleRegressionHead(config)
        self.agent_num = num_agent
        self.kd_flag = kd_flag
        self.layer = layer
        self.in_channels = in_channels
        self._packed = None
        self._packed_key = None

    # ---- packed-parameter cache -----------------------------------------------------------
    def _pack(self, device):  # pragma: no cover - overridden
        raise NotImplementedError

    def packed(self, device=None):
        if device is None:
            device = next(self.parameters()).device
        if torch.device(device).type != "cuda":
            raise RuntimeError("v2x_sim_amd models run on the MI355X only: move the model to 'cuda' "
                               "(no CPU fallback exists in the product path)")
        key = (str(device), sum(t._version + getattr(t, "_v2x_epoch", 0) for t in self.parameters())
               + sum(t._version + getattr(t, "_v2x_epoch", 0) for t in self.buffers()))   # _v2x_epoch: packing.watch_optimizer (fused optimizers do not bump _version)
        if self._packed is None or self._packed_key != key:
            with torch.no_grad():
                self._packed = self._pack(device)
            self._packed_key = key
        return self._packed

    def repack(self):
        self._packed = None

    # ---- what every family answers ---------------------------------------------------------
    def backbone(self):  # pragma: no cover - overridden
        """-> (encoder, decoder): the two parameter containers, wherever the family keeps them."""
        raise NotImplementedError

    def head(self, pk, feats):
        """What every forward_nhwc ends in: the detection heads here, the class head in models/seg."""
        return self.decode_heads(pk, feats)

    def run_batch(self, data, batch_size=1, inference=None):
        """forward() on a batch dict ('bev_seq', 'trans_matrices', 'num_agent'): the one call of the step modules' inference paths.
        `inference` is when2com's; the other families take no such argument."""
        return self(data["bev_seq"], data["trans_matrices"], data["num_agent"], batch_size=batch_size)

    # ---- shared pieces --------------------------------------------------------------------
    def _pack_heads(self, device):
        """cls | reg hidden 3x3 (32 -> 64) chained with the block-diagonal 1x1 (64 -> 12 + 36): one halo
        launch writes both fp32 logit tensors; the gather-kernel pair is the fallback for odd extents."""
        bp = self.regression.box_prediction
        c = self.classification
        hidden, final, ncls = packing.pack_heads("heads", c.conv1, c.bn1, c.conv2, bp[0], bp[1], bp[3], device=device)
        s1, t1 = packing.fold_bn(c.conv1.bias, c.bn1, c.conv1.out_channels)
        s2, t2 = packing.fold_bn(bp[0].bias, bp[1], bp[0].out_channels)
        w1 = torch.cat([c.conv1.weight.detach().float().cpu(), bp[0].weight.detach().float().cpu()], 0)
        hc, hr = c.conv1.out_channels, bp[0].out_channels
        nreg = bp[3].out_channels
        w2 = torch.zeros((ncls + nreg, hc + hr, 1, 1), dtype=torch.float32)
        w2[:ncls, :hc] = c.conv2.weight.detach().float().cpu()
        w2[ncls:, hc:] = bp[3].weight.detach().float().cpu()
        b2 = torch.cat([c.conv2.bias.detach().float().cpu(), bp[3].bias.detach().float().cpu()])
        halo = None
        if (hc + hr, ncls + nreg) == (64, 48):
            halo = packing.pack_conv_halo("heads.fused", w1, torch.cat([s1, s2]), torch.cat([t1, t2]), relu=True,
                                          chain=(w2, torch.ones(ncls + nreg), b2, False), epilogue=V2X_EPI_F32,
                                          device=device)
        layer = ops.Layer([hidden, final], halo, split=ncls, name="heads")
        # the same heads with the score threshold in the epilogue (detections without the logits round trip): DetModelBase.detections()
        layer.det = packing.pack_heads_det("heads.det", c.conv1, c.bn1, c.conv2, bp[0], bp[1], bp[3], device=device) if halo is not None else None
        return layer

    def _input_nhwc(self, bevs):
        """(N, 1, X, Y, Z) fp32 dense BEV (the reference Dataset format) -> (N, X, Y, c_pad) bf16."""
        if bevs.dim() != 5 or bevs.shape[1] != 1:
            raise ValueError("bevs must be (batch*agents, 1, X, Y, Z); got %s" % (tuple(bevs.shape),))
        return ops.dense_to_nhwc(bevs[:, 0].to(torch.float32).contiguous(), INPUT_C_PAD)

    def decode_heads(self, pk, feats):
        """Decoder + heads on the (possibly fused) pyramid `feats` -> {'loc', 'cls'}; inside `with model.detections(thr, cap)` and when
        the extent allows -> {'det': (keys, codes, counts)}: the candidates of apply_nms_det's threshold step straight from the heads'
        epilogue (ops.conv2d_det), the logits never written."""
        req = getattr(self, "_det_request", None)
        heads, last = pk["heads"], pk["dec"][-1]
        if req is None and heads.halo is not None and last.halo is not None:
            # logits: conv8_2 and the heads as ONE launch when the extent allows (conv_tail.hip; bit-identical to the two launches)
            x = LidarDecoder.run(pk["dec"], *feats, last=False)
            if ops.tail_eligible(last.halo, heads.halo, x, heads.split):
                cls, loc = ops.conv2d_tail(last.halo, heads.halo, x, heads.split)
                return self._shape_cls_loc(cls, loc)
            x = ops.run_layer(last, x)
        else:
            x = LidarDecoder.run(pk["dec"], *feats)
        det = getattr(pk["heads"], "det", None)
        if (req is not None and det is not None and ops.covers(det, x.shape[1], x.shape[2])
                and (self.anchor_num_per_loc, self.category_num, self.box_code_size, self.out_seq_len) == (6, 2, 6, 1)):
            return {"det": ops.conv2d_det(det, x, req[0], req[1])}
        return self.get_cls_loc_result(x, pk["heads"])

    def detections(self, score_thr, cap=4096):
        """Context manager: forward() calls inside return candidates instead of logits (see decode_heads)."""
        import contextlib

        @contextlib.contextmanager
        def _cm():
            prev = getattr(self, "_det_request", None)
            self._det_request = (float(score_thr), int(cap))
            try:
                yield self
            finally:
                self._det_request = prev
        return _cm()

    def _shape_cls_loc(self, cls, loc):
        n = cls.shape[0]
        return {"loc": loc.view(-1, loc.size(1), loc.size(2), self.anchor_num_per_loc, self.out_seq_len, self.box_code_size),
                "cls": cls.view(n, -1, self.category_num)}

    def get_cls_loc_result(self, x, heads):
        cls, loc = ops.run_layer(heads, x)  # fp32 NHWC == upstream's permute(0, 2, 3, 1)
        n = cls.shape[0]
        cls_preds = cls.view(n, -1, self.category_num)
        loc_preds = loc.view(-1, loc.size(1), loc.size(2), self.anchor_num_per_loc, self.out_seq_len,
                             self.box_code_size)
        return {"loc": loc_preds, "cls": cls_preds}

    @staticmethod
    def agents_to_batch(feats):
        return torch.cat([feats[:, i] for i in range(feats.shape[1])], 0)


class NonIntermediateModelBase(DetModelBase):
    pass


class IntermediateModelBase(DetModelBase):
    """Models that exchange an intermediate feature map (upstream IntermediateModelBase/FusionBase)."""

    def __init__(self, config, layer=3, in_channels=13, kd_flag=True, p_com_outage=0.0, num_agent=5,
                 compress_level=0, only_v2i=False):
        super().__init__(config, layer, in_channels, kd_flag, p_com_outage, num_agent, only_v2i)
        from ...utils import comm
        flags = comm.current_model_flags()      # inside `with comm.model_flags(...)`: what a constructor call that leaves the two at their defaults takes
        pose_noise, channel_seed = 0.0, 0
        if flags is not None:
            if compress_level == 0:
                compress_level = flags["compress_level"]
            only_v2i = only_v2i or flags["only_v2i"]
            if p_com_outage == 0.0:
                p_com_outage = flags.get("p_com_outage", 0.0)
            pose_noise, channel_seed = flags.get("pose_noise", 0.0), flags.get("channel_seed", 0)
        self.compress_level = compress_level
        self.only_v2i = bool(only_v2i)
        self._link_mask = None
        # the degraded-link condition: what the next make_plan() takes, the step counter (device memory once a plan exists) and the last draw
        self._channel = None
        self._channel_step0, self._channel_step, self._last_links, self._channel_stats = 0, None, None, None
        self.set_channel(p_com_outage, pose_noise, channel_seed)
        if flags is not None and "channel_models" in flags and self._channel is not None:
            flags["channel_models"].append(self)       # the evaluation tools print the realised share of links up (comm.run_eval_driver)
            self._channel_stats = [None, None]
        self.u_encoder = LidarEncoder(in_channels, compress_level=compress_level)
        self.decoder = LidarDecoder(in_channels)

    def backbone(self):
        return self.u_encoder, self.decoder

    # ---- who may talk to whom -------------------------------------------------------------
    def set_link_mask(self, mask):
        """mask[b, i, j] (bool, (B, A, A) or (A, A) for every frame): ego i of frame b receives from agent j.  The diagonal and the rows /
        columns of absent agents are ignored.  None removes it.  only_v2i=True (agent 0 is the road-side unit: a link j -> i exists only if
        i == 0 or j == 0) is ANDed with it.  Takes effect in the next make_plan(): a plan built before keeps its links."""
        if mask is not None:
            mask = torch.as_tensor(mask).detach().to("cpu")
            A = self.agent_num
            if mask.dim() not in (2, 3) or tuple(mask.shape[-2:]) != (A, A):
                raise ValueError("link mask must be (B, %d, %d) or (%d, %d), got %s" % (A, A, A, A, tuple(mask.shape)))
            mask = mask != 0
        self._link_mask = mask

    def links(self, batch_size):
        """-> None when every link is allowed, else nested lists L[b][i][j] of python bools (only_v2i AND the user mask)."""
        A = self.agent_num
        m = self._link_mask
        if m is None and not self.only_v2i:
            return None
        if m is not None and m.dim() == 3 and m.shape[0] != batch_size:
            raise ValueError("link mask holds %d frames, the batch %d" % (m.shape[0], batch_size))
        out = []
        for b in range(batch_size):
            mb = None if m is None else (m if m.dim() == 2 else m[b]).tolist()
            out.append([[(mb is None or bool(mb[i][j])) and (not self.only_v2i or i == 0 or j == 0) for j in range(A)] for i in range(A)])
        return out

    # ---- degraded links: p_com_outage and pose noise drawn on the device --------------------------------
    CHANNEL_OUTAGE = True          # False: the family takes pose noise only (when2com: its attention has no agreed reading under a link mask)

    def set_channel(self, p_com_outage=0.0, pose_noise=0.0, seed=0):
        """Every directed link j -> i is down with probability p_com_outage at every step, independently; pose_noise is the sigma in metres of Gaussian
        noise on the translation of every agent-to-agent transform; seed (64 bits) keys the counter-based generator, so a host predicts every draw
        from (seed, step).  Like set_link_mask it takes effect in the next make_plan(): a plan built before keeps its condition."""
        import math
        p, sigma = float(p_com_outage), float(pose_noise)
        if not 0.0 <= p <= 1.0:
            raise ValueError("p_com_outage must lie in [0, 1], got %r" % (p_com_outage,))
        if not (sigma >= 0.0 and math.isfinite(sigma)):
            raise ValueError("pose_noise must be finite and >= 0, got %r" % (pose_noise,))
        seed = int(seed)
        if not 0 <= seed < (1 << 64):
            raise ValueError("the channel seed must lie in [0, 2^64), got %r" % (seed,))
        if p > 0.0 and not self.CHANNEL_OUTAGE:
            raise NotImplementedError("when2com under link outage is out of scope: its attention has no agreed reading under a link mask "
                                      "(DESIGN.md section 9); pose noise alone is accepted")
        self._channel = None if (p == 0.0 and sigma == 0.0) else (p, sigma, seed)

    @property
    def p_com_outage(self):
        return 0.0 if self._channel is None else self._channel[0]

    @property
    def pose_noise(self):
        return 0.0 if self._channel is None else self._channel[1]

    def reset_channel(self, step=0):
        """The step counter := step (stream-ordered, no synchronisation): the next degraded forward draws the links and the noise of that step."""
        step = int(step)
        if not 0 <= step < (1 << 63):
            raise ValueError("the channel step must lie in [0, 2^63), got %r" % (step,))
        self._channel_step0 = step
        if self._channel_step is not None:
            self._channel_step.fill_(step)

    def channel_step(self):
        """The step the next degraded forward will draw.  The ONLY call of the feature that synchronises with the host."""
        return self._channel_step0 if self._channel_step is None else int(self._channel_step.item())

    def last_links(self):
        """(B, A, A) uint8 device tensor of the last draw: [f][i][j] = 1 iff ego i of frame f fused source j != i; None before the first one and
        under pose noise alone."""
        return self._last_links

    def _channel_counter(self, device):
        if self._channel_step is None or self._channel_step.device != torch.device(device):
            self._channel_step = torch.tensor([self._channel_step0], dtype=torch.int64, device=device)    # the kernel reads it as a uint64
        return self._channel_step

    def channel_plan(self, plan, batch_size, device, coef="coef", coef2=None, also=()):
        """What every family's make_plan() ends in.  Undegraded: the plan as it is.  Degraded: one more entry, "channel" -- the static rows, the live
        buffers of this step's rows (and DiscoNet's one-hot rows), the link table and the pose buffer: allocated ONCE here, so their addresses are
        stable under capture.  Every other entry of the plan stays what the family built."""
        if self._channel is None:
            return plan
        p, sigma, seed = self._channel
        A = self.agent_num
        ch = {"p": p, "sigma": sigma, "seed": seed, "Bt": batch_size, "coef0": None, "coef": None, "coef2": None, "links": None,
              "trans": torch.empty((batch_size, A, A, 4, 4), dtype=torch.float32, device=device) if sigma > 0.0 else None}
        live = dict(plan)
        if coef is not None:
            c0 = plan[coef].contiguous()
            ch["coef0"], ch["coef"] = c0, torch.empty_like(c0)
            ch["links"] = torch.zeros((batch_size, A, A), dtype=torch.uint8, device=device)
            live[coef] = ch["coef"]
            for k in also:                       # DiscoNet's `valid` = coef
                live[k] = ch["coef"]
            if coef2 is not None:
                ch["coef2"] = torch.empty_like(plan[coef2])
                live[coef2] = ch["coef2"]
            eye = torch.eye(A, device=c0.device).index_select(0, plan["items"][:, 0].long().to(c0.device))
            ch["possible"] = ((c0 != 0) & (eye == 0)).sum()          # the static plan's links: what the realised share is measured against
        ch["live"] = live
        self._channel_counter(plan["items"].device)
        plan = dict(plan)
        plan["channel"] = ch
        return plan

    def degrade(self, plan, trans_matrices):
        """-> (this step's plan, this step's poses): ONE ops.channel_degrade launch on a degraded plan, the arguments themselves otherwise."""
        ch = plan.get("channel")
        if ch is None:
            return plan, trans_matrices
        trans = trans_matrices.to(torch.float32).contiguous() if ch["trans"] is not None else None
        ops.channel_degrade(plan["items"], self.agent_num, ch["Bt"], ch["coef0"], ch["coef"], ch["coef2"], ch["links"], trans, ch["trans"],
                            ch["p"], ch["sigma"], ch["seed"], self._channel_counter(plan["items"].device))
        self._last_links = ch["links"]
        if self._channel_stats is not None and ch["links"] is not None:       # built by an evaluation tool: device-side sums, read once at the end
            up, possible = ch["links"].sum(), ch["possible"]
            self._channel_stats = [up if self._channel_stats[0] is None else self._channel_stats[0] + up,
                                   possible if self._channel_stats[1] is None else self._channel_stats[1] + possible]
        return ch["live"], (ch["trans"] if ch["trans"] is not None else trans_matrices)

    def channel_link_stats(self):
        """-> (links up, links the static plans allowed) summed over the degraded forwards so far (synchronises); (0, 0) where nothing was counted."""
        if not self._channel_stats or self._channel_stats[0] is None:
            return 0, 0
        return int(self._channel_stats[0].item()), int(self._channel_stats[1].item())

    def fusion_shape(self):
        return LAYER_SHAPES[self.layer]

    @staticmethod
    def frame_plan(num_agent_tensor, batch_size, agent_num):
        """Host-side bookkeeping shared by the fusion models.

        num_agent_tensor (B, A) -- [b, 0] is the number of real agents of frame b (upstream
        convention).  Returns python lists: items [(agent, frame)] in agent-major order for every
        real agent, and the flat row of each item in the (A*B) agent-major batch."""
        nat = num_agent_tensor.detach().to("cpu") if isinstance(num_agent_tensor, torch.Tensor) else num_agent_tensor
        counts = [int(nat[b][0]) for b in range(batch_size)]
        for c in counts:
            if c < 1 or c > agent_num:
                raise ValueError("num_agent_tensor[b, 0]=%d outside [1, %d]" % (c, agent_num))
        items = [(a, f) for a in range(agent_num) for f in range(batch_size) if a < counts[f]]
        rows = [a * batch_size + f for a, f in items]
        return counts, items, rows

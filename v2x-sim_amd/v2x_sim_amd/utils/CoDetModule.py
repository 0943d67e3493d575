"""Mirror of upstream coperception/utils/CoDetModule.py::FaFModule (absent from /root/reference; README.md:101
points at tools/det/{train,test}_codet.py which drive it).

`predict_all` keeps the upstream call shape: run the model (HIP engine) on the agent-major batch, then per
agent apply the 'faf' decode + NMS (utils/postprocess.py) unless that agent's BEV is empty.
`step` is the training step: PyTorch-ROCm autograd graph (train/graph.py) over the same
parameter tree, focal + smooth-L1 losses (train/loss.py), optimizer step; the HIP engine re-packs lazily afterwards.
"""
import numpy as np
import torch

from . import postprocess


class FaFModule(object):
    def __init__(self, model, teacher, config, optimizer, kd_flag):
        if kd_flag:
            raise NotImplementedError("knowledge distillation is out of scope (DESIGN.md section 8)")
        self.model = model
        self.config = config
        self.optimizer = optimizer
        from .. import packing
        packing.watch_optimizer(optimizer)   # fused optimizers update the parameters without bumping their version counters
        self.anchors = postprocess.build_anchor_map(config)
        self.score_thr = 0.7
        self.nms_thr = 0.01
        self.device_postprocess = True    # False: upstream's host-side numpy path (utils/postprocess.apply_nms_det)
        self.fused_detection = True       # with device_postprocess: score threshold in the heads' epilogue, logits never stored
        self.cap = 4096                   # candidate capacity per map of the device path
        self._anchors_dev = None
        # late fusion (upstream --com late): the agents exchange their detections, every ego suppresses the union in its own frame (one more
        # launch behind the per-agent NMS, ops.late_fuse).  Who hears whom: set_link_mask / late_only_v2i, the agent table and the empty sweeps.
        self.late_fusion = False
        self.late_only_v2i = False        # vehicles hear the road-side unit (agent 0) only, agent 0 hears everybody
        self.late_cap = None              # merged capacity per ego of the device path (None: self.cap)
        self._late_link = None
        self.late_stats = {"egos": 0, "kept": 0, "from_neighbours": 0}    # counted by predict_all under late_fusion
        from . import comm
        flags = comm.current_model_flags() or {}
        if flags.get("late"):             # built inside comm.model_flags(late=True): tools/det/eval_codet.py --com late
            self.late_fusion, self.late_only_v2i, self.late_stats = True, bool(flags.get("only_v2i")), flags["late_stats"]
        # oracle/ASSUMPTIONS.md rows 48 / 49 as switches (configs.Config): which box extent runs along the heading, the loss normaliser
        self.wh_axis = getattr(config, "box_wh_axis", "w_along_heading")
        self.loss_normalizer = getattr(config, "loss_normalizer", "positives")
        if self.wh_axis not in postprocess.WH_AXES:
            raise ValueError("config.box_wh_axis must be one of %s" % (postprocess.WH_AXES,))
        # upstream's loss_calculator switch (train/loss.py::detection_loss): "faf_loss" = smooth-L1 on the codes, "corner_loss" = the corner distance
        self.loss_type = getattr(config, "loss_type", "faf_loss")
        from ..train.loss import LOSS_TYPES
        if self.loss_type not in LOSS_TYPES:
            raise ValueError("config.loss_type must be one of %s, got %r" % (LOSS_TYPES, self.loss_type))
        if self.loss_type == "corner_loss" and not (getattr(config, "only_det", True) and getattr(config, "code_type", "faf") == "faf"
                                                    and getattr(config, "pred_len", 1) == 1):
            raise NotImplementedError("loss_type='corner_loss' covers only_det=True, code_type='faf', pred_len=1 (DESIGN.md section 3.10)")
        self._loss_anchors = None         # the anchors of one map on the device, (M, 6): what the corner loss decodes through
        self._graphed = None              # (batch-shape key, GraphedTrainStep) when V2X_TRAIN_GRAPH=1

    def step(self, data, batch_size, num_agent=5):
        """One optimisation step.  data: 'bev_seq' (A*B, 1, X, Y, Z), 'labels' (A*B, X, Y, A', 2), 'reg_targets'
        (A*B, X, Y, A', 1, 6), 'reg_loss_mask' (A*B, X, Y, A', 1), 'trans_matrices' (B, A, A, 4, 4), 'num_agent' (B, A)
        -> (loss, cls_loss, loc_loss) python floats, as upstream."""
        from .. import packing
        from ..train import detection_loss, train_forward
        if self.optimizer is None:
            raise RuntimeError("FaFModule.step needs an optimizer")
        bev = data["bev_seq"]
        if not bev.is_cuda or next(self.model.parameters()).device != bev.device:
            raise RuntimeError("FaFModule.step trains on the MI355X: move the model and the batch to 'cuda'")
        self.model.train()
        if self._graph_ok(data, batch_size):
            # V2X_TRAIN_HIP=1 V2X_TRAIN_GRAPH=1: the whole step as one hipGraph (train/graph_step.py), rebuilt when the batch shape changes
            from ..train.graph_step import GraphedTrainStep, cached_step
            key = self._graph_key(data, batch_size)
            step = cached_step(self.optimizer, key, lambda: GraphedTrainStep(self.model, self.optimizer, data, batch_size, normalizer=self.loss_normalizer,
                                                                             **self._loss_kwargs(bev.device)))
            self._graphed = (key, step)
            loss, cls_loss, loc_loss = step(data)
            return loss.item(), cls_loss.item(), loc_loss.item()
        result = train_forward(self.model, bev, data.get("trans_matrices"), data.get("num_agent"), batch_size)
        loss, cls_loss, loc_loss = detection_loss(result, data["labels"], data["reg_targets"], data["reg_loss_mask"], normalizer=self.loss_normalizer,
                                                  **self._loss_kwargs(bev.device))
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer.step()
        packing.stepped(self.optimizer)       # (an optimizer without step hooks: stamp the parameters here)
        return loss.item(), cls_loss.item(), loc_loss.item()

    def _loss_kwargs(self, device):
        """detection_loss's loss_type / anchors / wh_axis; the anchor table goes to the device once (as _anchors_dev does for post-processing)."""
        if self.loss_type != "corner_loss":
            return {"loss_type": self.loss_type}
        if self._loss_anchors is None or self._loss_anchors.device != device:
            from ..train.loss import corner_anchor_table
            self._loss_anchors = corner_anchor_table(self.anchors, device)
        return {"loss_type": self.loss_type, "anchors": self._loss_anchors, "wh_axis": self.wh_axis}

    def _graph_key(self, data, batch_size):
        return (id(self.model),) + tuple(tuple(data[k].shape) for k in ("bev_seq", "labels", "reg_targets", "reg_loss_mask")) + (batch_size, self.loss_normalizer,
                                                                                                                                self.loss_type)

    def _graph_ok(self, data, batch_size):
        from .. import tuning
        if tuning.get("TRAIN_HIP") != 1 or tuning.get("TRAIN_GRAPH") != 1:
            return False
        if hasattr(self.model, "outc"):             # a segmentation variant: SegModule's step
            return False
        from ..train.graph_step import cached_step, capture_ok
        return capture_ok(self.model, self.optimizer, data, cached_step(self.optimizer, self._graph_key(data, batch_size)))

    def set_link_mask(self, mask):
        """Late fusion's "who hears whom": (B, A, A) bool, entry [b, i, j] = ego i of frame b receives agent j's boxes; a false diagonal entry
        takes agent i out of the frame.  None: everybody hears everybody.  late_only_v2i and the agent table are applied on top."""
        self._late_link = None if mask is None else np.asarray(mask.cpu().numpy() if hasattr(mask, "cpu") else mask).astype(bool)

    def late_links(self, data, batch_size, num_agent):
        """-> (B, A, A) bool on the host: the user's mask, only_v2i and the agent table ('num_agent' (B, A): the agents of frame b are 0 .. n_b - 1)
        folded; the empty sweeps are not in it (predict_all folds them on the device and through its None slots)."""
        A, B = num_agent, batch_size
        L = np.ones((B, A, A), bool) if self._late_link is None else self._late_link.copy()
        if L.shape != (B, A, A):
            raise ValueError("late fusion: the link mask is %s, the batch needs %s" % (L.shape, (B, A, A)))
        if self.late_only_v2i:
            v = np.eye(A, dtype=bool)
            v[:, 0] = True
            v[0, :] = True
            L &= v
        nat = data.get("num_agent")
        if nat is not None:
            n = np.asarray(nat.cpu().numpy() if hasattr(nat, "cpu") else nat).reshape(B, -1)[:, 0]
            here = np.arange(A)[None, :] < n[:, None]
            L &= here[:, :, None] & here[:, None, :]
        return L

    def _late_counted(self, seq_results):
        for k, row in enumerate(seq_results):
            for det in row:
                if det is not None:
                    self.late_stats["egos"] += 1
                    self.late_stats["kept"] += len(det["src_agent"])
                    self.late_stats["from_neighbours"] += int((det["src_agent"] != k).sum())
        return seq_results

    def _late_fused(self, boxes, scores, count, late):
        """The fused launch behind the per-agent NMS, before the extents are un-swapped.  -> (per-agent count on the host, fused lists or None when
        an ego was not computed: the caller takes the numpy path).  Copies: the two count vectors as one, then boxes and scores | sources."""
        from .. import ops
        rigid, link = late
        fb, fs, fsrc, fcount = ops.late_fuse(boxes.contiguous(), scores, count, rigid, link, self.config.area_extents, self.nms_thr,
                                             cap_out=self.late_cap or boxes.shape[1])
        both = torch.stack([count, fcount]).cpu().numpy()
        count_h, fcount_h = both[0], both[1]
        if (count_h < 0).any() or (fcount_h < 0).any():
            return count_h, None
        kmax = int(max(1, fcount_h.max()))
        swap = self.wh_axis == "h_along_heading"
        fb = (fb[:, :kmax][..., [0, 1, 3, 2, 4]] if swap else fb[:, :kmax]).cpu().numpy()
        ss = torch.cat([fs[:, :kmax], fsrc[:, :kmax].view(torch.float32)], 1).cpu().numpy()
        fs_h, src_h = ss[:, :kmax], np.ascontiguousarray(ss[:, kmax:]).view(np.int32)
        cap_in = boxes.shape[1]
        return count_h, [{"boxes": fb[r, :fcount_h[r]], "scores": fs_h[r, :fcount_h[r]], "src_agent": (src_h[r, :fcount_h[r]] // cap_in).astype(np.int64),
                          "corners": postprocess.box_corners(fb[r, :fcount_h[r]], self.wh_axis) if fcount_h[r] else np.zeros((0, 4, 2), np.float32)}
                         for r in range(boxes.shape[0])]

    def postprocess(self, result, late=None):
        """Device-side score / threshold / decode / NMS (v2x_det_postprocess) for every map of `result` -> list of
        dict(boxes, corners, scores) like postprocess.apply_nms_det; maps with more than `cap` candidates fall back to the
        host function (with random weights tens of thousands of anchors can pass the threshold).
        result = {'det': ...} (the heads already thresholded, DetModelBase.detections): only sort + decode + NMS are left;
        -> None if a map overflowed `cap` there (the caller re-runs the logits path: no logits exist to fall back on).
        late = (rigid (B, A, A, 8), link (B, A, A) uint8) on the device: the late-fusion launch is chained behind the NMS and the return value is
        the pair (per-agent lists or None, fused lists or None) -- the fused lists when every ego was computed, the per-agent ones otherwise."""
        from .. import ops
        dev = (result["det"][0] if "det" in result else result["cls"]).device
        # "h_along_heading": the kernels lay w along the heading; a box with the extents exchanged is what they compute from anchors with
        # (w, h) exchanged and codes with (dw, dh) exchanged -- w' = a_h exp(dh) = h, h' = a_w exp(dw) = w -- so the second reading costs one
        # channel permutation of the codes and a column swap of the result, no second kernel (the corners below follow self.wh_axis)
        swap = self.wh_axis == "h_along_heading"
        perm = [0, 1, 3, 2, 4, 5]
        if self._anchors_dev is None or self._anchors_dev.device != dev:
            a = np.ascontiguousarray(self.anchors.reshape(-1, 6))
            self._anchors_dev = torch.from_numpy(np.ascontiguousarray(a[:, perm]) if swap else a).to(dev)

        def unswap(b):
            return b[..., [0, 1, 3, 2, 4]] if swap else b
        if "det" in result:
            keys, codes, counts = result["det"]
            boxes, scores, _, count = ops.det_nms_candidates(keys, codes[..., perm].contiguous() if swap else codes, counts, self._anchors_dev, self.nms_thr)
            fused = None
            if late is not None:
                count, fused = self._late_fused(boxes, scores, count, late)
                if fused is not None:
                    return None, fused
            boxes = unswap(boxes)
            count = count.cpu().numpy() if late is None else count
            if (count < 0).any():
                return None
            kmax = int(max(1, count.max()))
            boxes, scores = boxes[:, :kmax].cpu().numpy(), scores[:, :kmax].cpu().numpy()
            out = [{"boxes": boxes[i, :count[i]], "scores": scores[i, :count[i]],
                    "corners": postprocess.box_corners(boxes[i, :count[i]], self.wh_axis) if count[i] else np.zeros((0, 4, 2), np.float32)}
                   for i in range(keys.shape[0])]
            return out if late is None else (out, None)
        cls, loc = result["cls"], result["loc"]
        boxes, scores, _, count = ops.det_postprocess(cls.contiguous(), (loc.reshape(cls.shape[0], -1, 6)[..., perm] if swap else loc).contiguous(), self._anchors_dev,
                                                      self.score_thr, self.nms_thr, self.cap)
        if late is not None:
            count, fused = self._late_fused(boxes, scores, count, late)
            if fused is not None:
                return None, fused
        boxes = unswap(boxes)
        count = count.cpu().numpy() if late is None else count
        kmax = int(max(1, count.max()))
        boxes, scores = boxes[:, :kmax].cpu().numpy(), scores[:, :kmax].cpu().numpy()
        out = []
        for i in range(cls.shape[0]):
            if count[i] < 0:
                out.append(postprocess.apply_nms_det(loc[i].float().cpu().numpy(), cls[i].float().cpu().numpy(), self.anchors,
                                                     self.score_thr, self.nms_thr, wh_axis=self.wh_axis))
                continue
            b = boxes[i, :count[i]]
            out.append({"boxes": b, "corners": postprocess.box_corners(b, self.wh_axis) if count[i] else np.zeros((0, 4, 2), np.float32),
                        "scores": scores[i, :count[i]]})
        return out if late is None else (out, None)

    def predict_all(self, data, batch_size, validation=True, num_agent=5, inference="activated"):
        """data: dict with 'bev_seq' (A*B, 1, X, Y, Z), 'trans_matrices' (B, A, A, 4, 4),
        'num_agent' (B, A).  -> (loss, cls_loss, loc_loss, seq_results) with the losses None
        (no labels are consumed at inference) and seq_results[k][b] = detections of agent k in frame b, or None when
        that agent's BEV is empty (upstream skips such agents; the slot is kept so that callers pair detections with
        ground truth BY FRAME, never by list position).  when2com / who2com models run in `inference` mode."""
        bev_seq = data["bev_seq"]

        def run():
            with torch.no_grad():
                return self.model.run_batch(data, batch_size, inference)
        dets = None
        late = links = fused = None
        post = self.postprocess
        if self.late_fusion:
            # who hears whom: the host's table (mask, only_v2i, agent table) and, folded in ON THE DEVICE, the empty sweeps -- no copy waits here
            links = self.late_links(data, batch_size, num_agent)
            if self.device_postprocess:
                occ = (bev_seq.reshape(bev_seq.shape[0], -1) != 0).any(dim=1).reshape(num_agent, batch_size).t()          # (B, A)
                link_dev = torch.from_numpy(links).to(bev_seq.device) & occ[:, :, None] & occ[:, None, :]
                T = data["trans_matrices"]
                if isinstance(T, torch.Tensor) and T.is_cuda:      # the same derivation where the matrices are: no device-to-host copy is added
                    rigid = postprocess.late_rigid_from_trans_torch(T)
                else:
                    rigid = torch.from_numpy(postprocess.late_rigid_from_trans(T)).to(bev_seq.device)
                late = (rigid.contiguous(), link_dev.to(torch.uint8).contiguous())
                post = lambda r: self.postprocess(r, late)      # noqa: E731
        if self.device_postprocess and self.fused_detection and hasattr(self.model, "detections"):
            # detections without the logits round trip: the heads' epilogue thresholds the scores (DetModelBase.detections)
            with self.model.detections(self.score_thr, self.cap):
                result = run()
            dets = post(result) if "det" in result else None
            if dets is None and "det" in result:
                result = run()              # a map overflowed the candidate capacity: the logits path and its host fallback
        else:
            result = run()
        occupied = (bev_seq.reshape(bev_seq.shape[0], -1) != 0).any(dim=1).cpu().numpy()
        seq_results = [[] for _ in range(num_agent)]
        if dets is None:
            dets = post(result) if self.device_postprocess else None
        if late is not None:
            dets, fused = dets
        if fused is not None:
            # every ego came out of the fused launch; a slot is None where the agent is absent (mask, agent table) or its sweep empty
            self.last_result = result
            return None, None, None, self._late_counted([[fused[k * batch_size + b] if occupied[k * batch_size + b] and links[b, k, k] else None
                                                          for b in range(batch_size)] for k in range(num_agent)])
        if dets is None:
            cls = result["cls"].float().cpu().numpy()
            loc = result["loc"].float().cpu().numpy()
        for k in range(num_agent):
            for b in range(batch_size):
                row = k * batch_size + b
                if not occupied[row]:
                    seq_results[k].append(None)
                    continue
                seq_results[k].append(dets[row] if dets is not None else
                                      postprocess.apply_nms_det(loc[row], cls[row], self.anchors, self.score_thr, self.nms_thr))
        self.last_result = result
        if self.late_fusion:
            # the numpy mirror: device_postprocess off, or an ego the fused launch did not compute (a map or the merged list beyond its capacity)
            seq_results = postprocess.late_fusion(seq_results, data["trans_matrices"], num_agent, self.config.area_extents, link=links,
                                                  nms_thr=self.nms_thr, wh_axis=self.wh_axis)
            self._late_counted(seq_results)
        return None, None, None, seq_results

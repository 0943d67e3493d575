"""Mirror of upstream coperception/utils/SegModule.py (absent from /root/reference; README.md:101 points at tools/seg/
{train,test}_seg.py which drive it): `step` = one optimisation step with pixel-wise cross entropy (PyTorch-ROCm autograd
graph over the engine's parameter tree, train/graph.py), `predict` = HIP inference + argmax / confusion matrix on the device
(v2x_seg_argmax_confusion).  With the switches of tuning.py on (all default 0) `step` runs the loss on csrc/seg_loss.hip (TRAIN_SEG_LOSS_HIP: class weights,
ignored labels), the class head fused with it (TRAIN_SEG_HEAD_FUSE) and the whole step as one hipGraph (TRAIN_SEG_GRAPH: train/graph_step.py)."""
import torch
import torch.nn.functional as F


class SegModule(object):
    def __init__(self, model, teacher, config, optimizer, kd_flag=0, class_weight=None, ignore_index=255):
        if kd_flag:
            raise NotImplementedError("knowledge distillation is out of scope (DESIGN.md section 8)")
        self.model, self.config, self.optimizer = model, config, optimizer
        self.class_weight, self.ignore_index = class_weight, ignore_index     # train/loss.py::segmentation_loss (the switched-on paths of step)
        self.last_num_connect = None      # when2com variants: the communication rate of the last predict()
        self._graphed = None            # (batch-shape key, GraphedSegTrainStep) when TRAIN_SEG_GRAPH = 1
        from .. import packing
        packing.watch_optimizer(optimizer)   # fused optimizers update the parameters without bumping their version counters

    def step(self, data, num_agent=5, batch_size=1):
        """data: 'bev_seq' (A*B, 1, X, Y, Z), 'labels' (A*B, X, Y) uint8/int64, 'trans_matrices', 'num_agent' -> loss (float)."""
        from ..train import train_forward
        bev = data["bev_seq"]
        if not bev.is_cuda:
            raise RuntimeError("SegModule.step trains on the MI355X: move the model and the batch to 'cuda'")
        self.model.train()
        from .. import tuning
        if self._graph_ok(data, batch_size):
            # TRAIN_SEG_GRAPH = 1 (with TRAIN_HIP): the whole step as one hipGraph (train/graph_step.py::GraphedSegTrainStep), under FaFModule.step's
            # conditions and caching rule -- the captured steps live on the optimizer, one per batch shape
            from ..train.graph_step import GraphedSegTrainStep, cached_step
            key = self._graph_key(data, batch_size)
            step = cached_step(self.optimizer, key, lambda: GraphedSegTrainStep(self.model, self.optimizer, data, batch_size, class_weight=self.class_weight,
                                                                                ignore_index=self.ignore_index))
            self._graphed = (key, step)
            return step(data).item()
        if tuning.get("TRAIN_HIP") == 1 and tuning.get("TRAIN_SEG_LOSS_HIP") != 0:
            # the eager step with the loss on csrc/seg_loss.hip (and, TRAIN_SEG_HEAD_FUSE, the class head fused with it)
            from ..train.hip_graph import seg_train_loss
            labels = data["labels"] if data["labels"].dtype == torch.uint8 else data["labels"].to(torch.uint8)
            loss = seg_train_loss(self.model, bev, labels, data.get("trans_matrices"), data.get("num_agent"), batch_size, weight=self.class_weight,
                                  ignore_index=self.ignore_index)
        else:
            logits = train_forward(self.model, bev, data.get("trans_matrices"), data.get("num_agent"), batch_size)
            # (ignore_index: a rasterized map may hold the ignore label; without it a 255 is an out-of-range target.  Maps without one: the same bits)
            loss = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), data["labels"].reshape(-1).long(), ignore_index=self.ignore_index)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer.step()
        from .. import packing
        packing.stepped(self.optimizer)       # (an optimizer without step hooks: stamp the parameters here)
        return loss.item()

    def _graph_key(self, data, batch_size):
        cw = None if self.class_weight is None else tuple(float(v) for v in torch.as_tensor(self.class_weight).reshape(-1).tolist())
        return (id(self.model), "seg") + tuple(tuple(data[k].shape) for k in ("bev_seq", "labels")) + (batch_size, cw, self.ignore_index)

    def _graph_ok(self, data, batch_size):
        from .. import tuning
        if tuning.get("TRAIN_HIP") != 1 or tuning.get("TRAIN_SEG_GRAPH") != 1 or self.optimizer is None or not hasattr(self.model, "outc"):
            return False
        # (When2comSeg and the fusion family: no captured step exists for them -- their steps run eager, the kernel loss paths of step() still apply)
        from ..train.graph_step import cached_step, capture_ok
        return capture_ok(self.model, self.optimizer, data, cached_step(self.optimizer, self._graph_key(data, batch_size)))

    def predict(self, data, batch_size=1, label=None, inference=None):
        """-> (pred (A*B, X, Y) uint8, confusion matrix int64 [n_cls, n_cls] or None) on the HIP path.  when2com variants: `inference`
        ('softmax' | 'activated' | 'argmax_test', default 'activated') selects the links, and self.last_num_connect keeps the communication
        rate of this batch (When2com.num_connect)."""
        from .. import ops
        self.model.eval()
        with torch.no_grad():
            logits = self.model.run_batch(data, batch_size, inference)
        self.last_num_connect = self.model.last_num_connect
        return ops.seg_argmax_confusion(logits, label)


def iou_from_confusion(conf):
    """rows = label, cols = prediction -> per-class IoU (nan where the class is absent)."""
    conf = conf.double()
    tp = conf.diag()
    denom = conf.sum(0) + conf.sum(1) - tp
    return torch.where(denom > 0, tp / denom, torch.full_like(tp, float("nan")))

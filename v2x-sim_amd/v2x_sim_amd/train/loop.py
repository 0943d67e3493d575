"""Training loops shared by tools/det/train_codet.py and the trained-detector parity test.

Input side stays on the HIP path: sweeps are voxelised on the GPU (ops.voxelize_bits -> ops.bits_to_dense) into the
dense (A*B, 1, X, Y, Z) occupancy the reference Dataset yields; targets arrive sparse and are scattered on the device.
"""
import torch

from .. import ops, packing, tuning
from ..utils import postprocess, synthetic_scene
from ..utils.CoDetModule import FaFModule


def init_for_training(model, fg_prior=0.01, seed=0):
    """Kaiming-normal conv weights, identity BN, and a classification bias that starts every anchor at
    p(foreground) = fg_prior (the usual focal-loss initialisation)."""
    import math
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.Conv3d)):
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / fan_in))
                m.bias.zero_()
            elif isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm3d)):
                m.reset_parameters()
                m.reset_running_stats()
        b = model.classification.conv2.bias.view(-1, model.category_num)
        half = 0.5 * math.log((1.0 - fg_prior) / fg_prior)
        b[:, 0], b[:, 1] = half, -half
        model.classification.conv2.weight.mul_(0.1)
        model.regression.box_prediction[3].weight.mul_(0.1)
    return model


TARGET_RULES = ("radius", "iou")
_ANCHORS_ON_DEVICE = {}


def iou_targets_on_device(gt_lists, anchors, device, **assign_kw):
    """The training targets of DESIGN.md section 3.7's IoU rule for a batch: gt_lists = one (G_m, 5) array of boxes per item, in the models' batch
    order; padded to the longest list, uploaded once and assigned in ONE call (ops.assign_targets) -- no per-item work on the host.
    -> (labels, reg_targets, reg_loss_mask bool) as dense_targets_on_device returns them."""
    import numpy as np
    cap = max(1, max(np.asarray(g).reshape(-1, 5).shape[0] for g in gt_lists))
    boxes = np.zeros((len(gt_lists), cap, 5), np.float32)
    count = np.zeros((len(gt_lists),), np.int32)
    for m, g in enumerate(gt_lists):
        g = np.asarray(g, np.float32).reshape(-1, 5)
        boxes[m, :g.shape[0]], count[m] = g, g.shape[0]
    return iou_targets_from_device(torch.from_numpy(boxes).to(device), torch.from_numpy(count).to(device), anchors, device, **assign_kw)


def iou_targets_from_device(gt_boxes, gt_count, anchors, device, **assign_kw):
    """iou_targets_on_device for ground truth that is already on the device in the padded form: gt_boxes (n, cap, 5) fp32, gt_count (n,) int32 (what
    ops.visible_boxes leaves there) -- no host list, no upload."""
    import numpy as np
    key = (id(anchors), str(device))
    if key not in _ANCHORS_ON_DEVICE or _ANCHORS_ON_DEVICE[key][0] is not anchors:
        _ANCHORS_ON_DEVICE[key] = (anchors, torch.from_numpy(np.ascontiguousarray(anchors, np.float32)).to(device))
    res = ops.assign_targets(gt_boxes, gt_count, _ANCHORS_ON_DEVICE[key][1], want=(), **assign_kw)
    return res["labels"], res["reg_targets"], res["reg_loss_mask"].view(torch.bool)


def seg_targets_on_device(box_lists, class_lists, config, device, n_classes=8, rank=None, want=(), out=None):
    """The segmentation labels of DESIGN.md section 3.8's rule for a batch, the twin of iou_targets_on_device: box_lists = one (G_m, 5) array of boxes
    per item, in the models' batch order, class_lists = one (G_m,) array of class ids per item (None: every box is class 1); padded to the longest
    list, uploaded once and rasterized in ONE call (ops.rasterize_seg) on config's grid -- no per-item work on the host.  rank: a host sequence of
    n_classes ranks or None.  -> ops.rasterize_seg's dict: labels (n, X, Y) uint8 on the device and whatever `want` names (owner, hist)."""
    import numpy as np
    boxes, cls, count = ops.pad_box_lists(box_lists, class_lists)
    d_rank = None if rank is None else torch.from_numpy(np.asarray(rank, np.uint8).reshape(-1)).to(device)
    return ops.rasterize_seg(torch.from_numpy(boxes).to(device), torch.from_numpy(cls).to(device), torch.from_numpy(count).to(device), config,
                             n_classes=n_classes, rank=d_rank, want=want, out=out)


SCENES = ("sampled", "raycast", "raycast-moving")


def synthetic_batch_on_device(config, frames, agents, seed, device, grid=None, anchors=None, with_targets=True, targets="radius", scene="sampled",
                              **scene_kw):
    """-> data dict in FaFModule.step / predict_all's format (+ 'gt_boxes'[agent][frame] host arrays).
    targets: the assignment rule -- "radius": positives built per item on the host and scattered on the device; "iou": the
    padded boxes uploaded and assigned by rotated IoU in one call on the device (iou_targets_on_device).
    scene: "sampled": utils/synthetic_scene.make_scene's points on every car in range; "raycast": a world of boxes swept on the device with occlusion
    (utils/raycast_scene.raycast_batch_on_device), always with the IoU targets; "raycast-moving": ONE such world in motion,
    the `frames` items being consecutive steps of it (utils/raycast_scene.raycast_sequence_on_device; make_moving_world's keywords and the sequence's
    are both taken from scene_kw); scene_kw goes to whichever it is."""
    if targets not in TARGET_RULES:
        raise ValueError("targets must be one of %s" % (TARGET_RULES,))
    if scene not in SCENES:
        raise ValueError("scene must be one of %s" % (SCENES,))
    if scene == "raycast":
        from ..utils import raycast_scene
        return raycast_scene.raycast_batch_on_device(config, frames, agents, seed, device, grid, anchors, with_targets, **scene_kw)
    if scene == "raycast-moving":
        from ..utils import raycast_scene
        world_kw = {k: scene_kw.pop(k) for k in ("n_cars", "n_walls", "p_parked", "speed", "extent", "agent_extent") if k in scene_kw}
        world = scene_kw.pop("world", None) or raycast_scene.make_moving_world(1, agents, seed, **world_kw)
        return raycast_scene.raycast_sequence_on_device(config, world, frames, device=device, grid=grid, anchors=anchors, with_targets=with_targets,
                                                        seed=seed, **scene_kw)
    anchors = postprocess.build_anchor_map(config) if anchors is None else anchors
    grid = grid or ops.VoxelGrid(config.voxel_size, config.area_extents)
    b = synthetic_scene.make_batch(frames, agents, seed=seed, anchors=anchors if with_targets and targets == "radius" else None, targets="sparse",
                                   **scene_kw)
    pts = torch.from_numpy(b["points"]).to(device)
    bits = ops.voxelize_bits(pts, torch.from_numpy(b["n_pts"]).to(device), grid)
    data = {"bev_seq": ops.bits_to_dense(bits, grid.dims[2])[:, None],
            "trans_matrices": torch.from_numpy(b["trans"]).to(device), "num_agent": torch.from_numpy(b["num_agent"]),
            "gt_boxes": b["gt_boxes"]}
    if with_targets and targets == "iou":
        data["labels"], data["reg_targets"], data["reg_loss_mask"] = iou_targets_on_device(
            [b["gt_boxes"][a][f] for a in range(agents) for f in range(frames)], anchors, device)
    elif with_targets:
        data["labels"], data["reg_targets"], data["reg_loss_mask"] = synthetic_scene.dense_targets_on_device(
            b["pos"], b["pos_reg"], frames * agents, anchors.shape, device)
    return data


def make_optimizer(model, lr, total_steps):
    """Adam + the step-wise MultiStepLR (x0.3 at 60 % and 85 % of `total_steps`) every loop here uses.  Drivers that
    train for several epochs create the pair ONCE over the whole run and hand it to the loops, so that Adam's moments and
    the decay schedule survive epoch boundaries (and checkpoints)."""
    if tuning.get("TRAIN_GRAPH") == 1 and next(model.parameters()).is_cuda:
        # hipGraph-captured steps (train/graph_step.py): step counter and learning rate live on the device; the scheduler updates the
        # lr tensor in place, so the captured optimizer step sees every decay
        dev = next(model.parameters()).device
        opt = torch.optim.Adam(model.parameters(), lr=torch.tensor(float(lr), device=dev), capturable=True, fused=True)
    else:
        # fused: ONE multi-tensor kernel per step on the device (the default per-parameter form issues two tiny elementwise launches per
        # parameter: 184 of them = 0.47 ms of a 10-map FaFNet step)
        opt = torch.optim.Adam(model.parameters(), lr=lr, fused=next(model.parameters()).is_cuda)
    packing.watch_optimizer(opt)     # a fused step does not bump the parameters' version counters: the packed-weight caches need the hook
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[int(total_steps * 0.6), int(total_steps * 0.85)], gamma=0.3)
    return opt, sched


def train_synthetic(model, config, steps, frames_per_step=2, lr=1e-3, seed=0, device="cuda:0", log=None, agents=None,
                    opt=None, sched=None, targets="radius", scene="sampled", **scene_kw):
    """Adam on freshly generated synthetic scenes (never the same scene twice).  -> list of (loss, cls, loc).
    opt / sched: the run's optimizer and scheduler (make_optimizer); created here for a single self-contained run.
    targets: "radius" | "iou", scene: "sampled" | "raycast" | "raycast-moving", see synthetic_batch_on_device."""
    agents = agents or model.agent_num
    device = torch.device(device)
    model.to(device)
    if opt is None:
        opt, sched = make_optimizer(model, lr, steps)
    module = FaFModule(model, None, config, opt, 0)
    grid = ops.VoxelGrid(config.voxel_size, config.area_extents)
    hist = []
    for it in range(steps):
        data = synthetic_batch_on_device(config, frames_per_step, agents, seed * 1000003 + it, device, grid, module.anchors,
                                         targets=targets, scene=scene, **scene_kw)
        hist.append(module.step(data, frames_per_step, agents))
        if sched is not None:
            sched.step()
        if log and (it % log == 0 or it == steps - 1):
            print("step %4d  loss %.4f  cls %.4f  loc %.4f" % ((it,) + hist[-1]), flush=True)
    model.eval()
    return hist


def dataset_batch_on_device(samples, grid, anchors, device, targets="radius"):
    """Parsed-dataset samples (datasets.V2XSimDet with densify='none': sparse voxel indices + poses + gt boxes) -> the
    data dict of FaFModule.step.  The sweep is densified on the GPU (v2x_indices_to_bits -> v2x_bits_to_dense_f32); the
    anchor targets upstream's Dataset would return (label_one_hot, reg_target, reg_loss_mask) are built from the stored
    ground-truth boxes (synthetic_scene.anchor_targets_sparse, the radius rule of DESIGN.md section 3.7) and scattered
    on the device; targets="iou": assigned by rotated IoU on the device in one call (iou_targets_on_device)."""
    import numpy as np
    if targets not in TARGET_RULES:
        raise ValueError("targets must be one of %s" % (TARGET_RULES,))
    B, A = len(samples), len(samples[0])
    items = [(a, b) for a in range(A) for b in range(B)]                       # agent-major, as the models batch
    cap = max(1, max(samples[b][a][0].shape[0] for a, b in items))
    idx = np.zeros((len(items), cap, 3), np.int32)
    cnt = np.zeros((len(items),), np.int32)
    pos, reg = [], []
    for m, (a, b) in enumerate(items):
        it = samples[b][a][0]
        idx[m, :it.shape[0]] = it
        cnt[m] = it.shape[0]
        if targets == "radius":
            p, r = synthetic_scene.anchor_targets_sparse(samples[b][a][12], anchors)
            pos.append(np.concatenate([np.full((p.shape[0], 1), m, np.int64), p], 1))
            reg.append(r)
    bits = ops.indices_to_bits(torch.from_numpy(idx).to(device), torch.from_numpy(cnt).to(device), grid)
    data = {"bev_seq": ops.bits_to_dense(bits, grid.dims[2])[:, None],
            "trans_matrices": torch.from_numpy(np.stack([np.stack([samples[b][a][11] for a in range(A)])
                                                         for b in range(B)])).to(device),
            "num_agent": torch.tensor([[samples[b][a][10] for a in range(A)] for b in range(B)]),
            "gt_boxes": [[samples[b][a][12] for b in range(B)] for a in range(A)]}
    if targets == "iou":
        data["labels"], data["reg_targets"], data["reg_loss_mask"] = iou_targets_on_device([samples[b][a][12] for a, b in items], anchors, device)
    else:
        data["labels"], data["reg_targets"], data["reg_loss_mask"] = synthetic_scene.dense_targets_on_device(
            np.concatenate(pos), np.concatenate(reg), len(items), anchors.shape, device)
    return data


def train_dataset(model, config, dataset, epochs=1, batch=2, lr=1e-3, seed=0, device="cuda:0", log=None, num_workers=0,
                  opt=None, sched=None, targets="radius"):
    """Adam over a parsed dataset (datasets.V2XSimDet, densify='none'), shuffled per epoch; upstream's
    train_codet.py loop with the densify and the target scatter moved to the GPU.  -> list of (loss, cls, loc) per step.
    opt / sched as in train_synthetic."""
    from torch.utils.data import DataLoader
    device = torch.device(device)
    model.to(device)
    own = opt is None
    if own:
        opt = torch.optim.Adam(model.parameters(), lr=lr)
    module = FaFModule(model, None, config, opt, 0)
    grid = ops.VoxelGrid(config.voxel_size, config.area_extents)
    loader = DataLoader(dataset, batch_size=batch, shuffle=True, drop_last=False, num_workers=num_workers,
                        collate_fn=lambda x: x, generator=torch.Generator().manual_seed(seed))
    steps = epochs * len(loader)
    if own:
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[int(steps * 0.6), int(steps * 0.85)], gamma=0.3)
    hist = []
    for ep in range(epochs):
        for samples in loader:
            data = dataset_batch_on_device(samples, grid, module.anchors, device, targets=targets)
            hist.append(module.step(data, len(samples), len(samples[0])))
            if sched is not None:
                sched.step()
            if log and (len(hist) % log == 1 or len(hist) == steps):
                print("epoch %d step %4d  loss %.4f  cls %.4f  loc %.4f" % ((ep + 1, len(hist)) + hist[-1]), flush=True)
    model.eval()
    return hist

#!/usr/bin/env python3
"""Segmentation training driver -- the flag surface of upstream coperception/tools/seg/train_seg.py
(/root/reference/README.md:101 points at it; the script itself is not in the reference tree).

    python tools/seg/train_seg.py --data synthetic --com v2v --steps 300 --batch 2 --logpath out/
    python tools/seg/train_seg.py --data /path/V2X-Sim-seg/train --com v2v --nepoch 5 --batch 2 --logpath out/
    python tools/seg/train_seg.py --data synthetic --com when2com --steps 20 --batch 1        (--com: every detection baseline but `late`)
    python tools/seg/train_seg.py --data synthetic --targets boxes --class_weight balanced    (labels rasterized on the GPU, median-frequency weights)
    python tools/seg/train_seg.py --data synthetic --scene raycast --observed any            (ray-cast world; cells no agent observed are ignored)

Synthetic scenes (utils/synthetic_scene.py: vehicle footprints as class 1), PyTorch-ROCm autograd over the HIP engine's
parameter tree, checkpoint with upstream's 'model_state_dict' key for tools/seg/test_seg.py / eval_seg.py --resume."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, "v2x-sim_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


TARGETS = ("map", "boxes")
SCENES = ("sampled", "raycast")
OBSERVED = ("own", "any", "all")


def seg_batch(config, frames, agents, seed, device, grid, targets="map", n_classes=8, scene="sampled", observed="own"):
    """targets="map": the label maps painted per item on the host (synthetic_scene.seg_labels) and uploaded; "boxes": the padded boxes uploaded and
    rasterized for the whole batch in one call on the device (train/loop.py::seg_targets_on_device).
    scene="raycast": a world of cars (class 1) and walls (class 2) swept on the device, its boxes rasterized there and the cells no ray observed --
    the sweep's own rays (observed="own"), any agent's of the frame ("any"), or no masking ("all") -- set to the ignore class 255
    (utils/raycast_scene.raycast_seg_batch_on_device); `targets` does not apply."""
    from v2x_sim_amd import ops
    from v2x_sim_amd.utils import synthetic_scene
    if scene == "raycast":
        from v2x_sim_amd.utils import raycast_scene
        return raycast_scene.raycast_seg_batch_on_device(config, frames, agents, seed, device, observed=observed, n_classes=n_classes, grid=grid)
    b = synthetic_scene.make_batch(frames, agents, seed=seed)
    bits = ops.voxelize_bits(torch.from_numpy(b["points"]).to(device), torch.from_numpy(b["n_pts"]).to(device), grid)
    if targets == "boxes":
        from v2x_sim_amd.train.loop import seg_targets_on_device
        labels = seg_targets_on_device([b["gt_boxes"][a][f] for a in range(agents) for f in range(frames)], None, config, device, n_classes=n_classes)["labels"]
    else:
        labels = torch.from_numpy(np.stack([synthetic_scene.seg_labels(b["gt_boxes"][a][f], config) for a in range(agents) for f in range(frames)])).to(device)
    return {"bev_seq": ops.bits_to_dense(bits, grid.dims[2])[:, None], "trans_matrices": torch.from_numpy(b["trans"]).to(device),
            "num_agent": torch.from_numpy(b["num_agent"]), "labels": labels}


BALANCE_BATCHES = 32     # synthetic data: the class frequencies come from the first 32 batches


def synthetic_label_hist(config, frames, agents, first_seed, device, n_classes, scene="sampled"):
    """Cells per class over the first BALANCE_BATCHES synthetic batches of a run, from the rasterizer's histogram (only the boxes are uploaded).
    scene="raycast": the histogram the rasteriser gives for the painted world of each batch, before the unobserved cells are masked."""
    from v2x_sim_amd.train.loop import seg_targets_on_device
    from v2x_sim_amd.utils import synthetic_scene
    total = torch.zeros((n_classes + 1,), dtype=torch.int64, device=device)
    if scene == "raycast":
        from v2x_sim_amd.utils import raycast_scene
        for it in range(BALANCE_BATCHES):
            total += raycast_scene.raycast_seg_batch_on_device(config, frames, agents, first_seed + it, device, observed="all", n_classes=n_classes,
                                                               want_hist=True)["hist"].sum(0)
        return total.cpu().numpy()
    for it in range(BALANCE_BATCHES):
        b = synthetic_scene.make_batch(frames, agents, seed=first_seed + it)
        res = seg_targets_on_device([b["gt_boxes"][a][f] for a in range(agents) for f in range(frames)], None, config, device, n_classes=n_classes,
                                    want=("hist",))
        total += res["hist"].sum(0)
    return total.cpu().numpy()


def dataset_label_hist(dataset, grid, device, n_classes):
    """Cells per class over ONE pass of a parsed set: bev_seg maps are counted with torch.bincount on the device, boxes samples through the
    rasterizer's histogram, a frame's agents in one call."""
    from v2x_sim_amd import ops
    total = torch.zeros((n_classes + 1,), dtype=torch.int64, device=device)
    for k in range(len(dataset)):
        labels = [t[1] for t in dataset[k]]
        kinds = [isinstance(lab, tuple) for lab in labels]
        if any(kinds) and not all(kinds):
            raise ValueError("frame %d mixes bev_seg samples and gt_boxes samples" % k)
        if kinds[0]:
            boxes, cls, count = ops.pad_box_lists([lab[0] for lab in labels], [lab[1] for lab in labels])
            res = ops.rasterize_seg(torch.from_numpy(boxes).to(device), torch.from_numpy(cls).to(device), torch.from_numpy(count).to(device), grid,
                                    n_classes=n_classes, want=("hist",))
            total += res["hist"].sum(0)
        else:
            seen = torch.bincount(torch.from_numpy(np.stack(labels)).to(device).reshape(-1).long(), minlength=256)
            total[:n_classes] += seen[:n_classes]
            total[n_classes] += seen[n_classes:].sum()
    return total.cpu().numpy()


def class_weight_arg(text):
    """--class_weight: '' (none), 'balanced', or a comma list of floats (kept as text; main() parses it)."""
    if text in ("", "balanced"):
        return text
    try:
        [float(v) for v in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("expected `balanced` or a comma list of numbers, got %r" % text)
    return text


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("-d", "--data", default="synthetic", type=str)
    ap.add_argument("--com", default="v2v", choices=["lowerbound", "upperbound", "v2v", "when2com", "who2com", "sum", "mean", "max", "cat", "disco"])
    ap.add_argument("--inference", default=None, choices=["softmax", "activated", "argmax_test"],
                    help="when2com / who2com: the selection of the communication rate printed after each epoch (training itself uses the soft scores)")
    ap.add_argument("--batch", default=2, type=int)
    ap.add_argument("--steps", default=300, type=int)
    ap.add_argument("--nepoch", default=1, type=int)
    ap.add_argument("--lr", default=1e-3, type=float)
    ap.add_argument("--num_agent", default=5, type=int)
    ap.add_argument("--logpath", default="", type=str)
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--log", action="store_true")
    ap.add_argument("--rsu", default=1, type=int, help="parsed dataset: 1 = agent0 (the RSU) takes part, 0 = vehicles only")
    ap.add_argument("--resume", default="", type=str)
    from v2x_sim_amd.utils import comm
    comm.add_arguments(ap)
    ap.add_argument("--engine", default="", choices=["", "torch", "hip", "hip-graph"],
                    help="training graph: torch = PyTorch-ROCm ops (fp32, MIOpen); hip = bf16 NHWC graph on the hand-written kernels (V2X_TRAIN_HIP=1), the loss "
                         "as PyTorch ops; hip-graph = the same with the loss kernels, the class head fused with the loss and every step replayed as one hipGraph "
                         "(V2X_TRAIN_SEG_LOSS_HIP / _HEAD_FUSE / _GRAPH = 1; a capturable Adam with a device-tensor learning rate).  Default: whatever the "
                         "environment variables say")
    ap.add_argument("--class_weight", default="", type=class_weight_arg,
                    help="comma list of per-class loss weights (the kernel loss paths; default: none), or `balanced`: median-frequency weights "
                         "w_c = median(f) / f_c over the classes that occur (0 for the absent ones), computed before training -- synthetic data: from the "
                         "first 32 batches; a parsed set: from one pass over it")
    ap.add_argument("--targets", default="map", choices=list(TARGETS),
                    help="synthetic data: map = label maps painted per item on the host and uploaded; boxes = the boxes uploaded and rasterized for the whole "
                         "batch in one call on the GPU (v2x_seg_rasterize).  A parsed set decides per sample: bev_seg maps or gt_boxes + gt_classes")
    ap.add_argument("--scene", default="sampled", choices=list(SCENES),
                    help="synthetic data: sampled = points on every car in range (utils/synthetic_scene.py); raycast = a world of cars and walls swept "
                         "on the GPU with occlusion, labels rasterized there (cars 1, walls 2) and masked by what the rays observed (--observed)")
    ap.add_argument("--observed", default="own", choices=list(OBSERVED),
                    help="--scene raycast: a cell is the ignore class 255 unless a ray of the sweep itself (own) or of any agent of the frame (any) "
                         "crossed or hit it; all = no masking")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.engine:
        from v2x_sim_amd import tuning
        tuning.set("TRAIN_HIP", int("0" if args.engine == "torch" else "1"))
        for name in ("TRAIN_SEG_LOSS_HIP", "TRAIN_SEG_HEAD_FUSE", "TRAIN_SEG_GRAPH"):
            tuning.set(name, int("1" if args.engine == "hip-graph" else "0"))
    class_weight = [float(v) for v in args.class_weight.split(",")] if args.class_weight not in ("", "balanced") else None
    from v2x_sim_amd import ops
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.seg import COM_CLASSES, When2comSeg, default_inference
    from v2x_sim_amd.train.loop import init_for_training
    from v2x_sim_amd.utils import comm
    from v2x_sim_amd.utils.SegModule import SegModule
    if not torch.cuda.is_available():
        raise SystemExit("train_seg.py needs the MI355X")
    device = torch.device("cuda:0")
    config = Config("train", binary=True, only_det=True)
    A = args.num_agent
    comm.refuse_channel_in_training(args)
    ckw = comm.model_kwargs(args, intermediate=args.com not in ("lowerbound", "upperbound"))
    model = COM_CLASSES[args.com](config, num_agent=A, **ckw)
    if args.engine == "hip-graph" and args.com not in ("lowerbound", "upperbound", "v2v"):
        print("--engine hip-graph: no captured step exists for --com %s, its steps run eager (the kernel loss paths stay on)" % args.com, file=sys.stderr)
    ckpt = None
    if args.resume:
        ckpt = torch.load(args.resume, map_location="cpu")
        comm.check_checkpoint(ckpt, args)
        model.load_state_dict(ckpt.get("model_state_dict", ckpt), strict=True)
    else:
        init_for_training(model, seed=args.seed)
    model.to(device)
    loader = None
    if args.data != "synthetic":
        # parsed dataset in the README.md:66-79 layout: <data>/agent{k}/{scene}_{frame}/0.npy with 'bev_seg' (agent0 = RSU)
        from torch.utils.data import DataLoader
        from v2x_sim_amd.datasets import V2XSimSeg, seg_batch_on_device
        first = 0 if args.rsu else 1
        roots = [os.path.join(args.data, "agent%d" % k) for k in range(first, first + A)]
        dataset = V2XSimSeg(dataset_roots=roots, config=config, split="train", densify="none")
        loader = DataLoader(dataset, batch_size=args.batch, shuffle=True, collate_fn=lambda x: x,
                            generator=torch.Generator().manual_seed(args.seed))
        print("training on %d frames x %d agents from %s" % (len(dataset), A, args.data))
    # one optimizer for the whole run, kept in the checkpoint (same rule as tools/det/train_codet.py)
    if args.engine == "hip-graph":       # the captured step needs the step counters and the learning rate on the device
        opt = torch.optim.Adam(model.parameters(), lr=torch.tensor(args.lr, dtype=torch.float32, device=device), capturable=True)
    else:
        opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    start = 1
    if ckpt is not None and "optimizer_state_dict" in ckpt:
        opt.load_state_dict(ckpt["optimizer_state_dict"])
    if ckpt is not None and "epoch" in ckpt:
        start = int(ckpt["epoch"]) + 1
    if class_weight is not None and len(class_weight) != model.n_classes:
        raise SystemExit("--class_weight needs %d values" % model.n_classes)
    grid = ops.VoxelGrid(config.voxel_size, config.area_extents)
    if args.class_weight == "balanced":
        if loader is not None:
            hist = dataset_label_hist(dataset, grid, device, model.n_classes)
        else:
            hist = synthetic_label_hist(config, args.batch, A, (args.seed + start) * 1000003, device, model.n_classes, args.scene)
        class_weight = ops.median_frequency_weights(hist, model.n_classes)
        print("class weights (median frequency): %s" % ", ".join("%.4g" % w for w in class_weight))
    module = SegModule(model, None, config, opt, 0, class_weight=class_weight)
    for epoch in range(start, args.nepoch + 1):
        losses, last = [], None
        if loader is not None:
            for samples in loader:
                last = (seg_batch_on_device(samples, grid, device, n_classes=model.n_classes), len(samples))
                losses.append(module.step(last[0], len(samples[0]), len(samples)))
        else:
            for it in range(args.steps):
                last = (seg_batch(config, args.batch, A, (args.seed + epoch) * 1000003 + it, device, grid, args.targets, model.n_classes, args.scene, args.observed),
                        args.batch)
                losses.append(module.step(last[0], A, args.batch))
                if args.log and it % 20 == 0:
                    print("step %4d  loss %.4f" % (it, losses[-1]), flush=True)
        print("epoch %d: mean loss of the last 20 steps %.4f" % (epoch, float(np.mean(losses[-20:]))))
        if isinstance(model, When2comSeg) and last is not None:
            # the communication rate of the current weights on the epoch's last batch, synthetic or parsed (off-diagonal non-zero links per agent and frame)
            module.predict(last[0], batch_size=last[1], inference=args.inference or default_inference(args.com))
            print("epoch %d: communication rate %.3f" % (epoch, module.last_num_connect))
        if args.logpath:
            os.makedirs(args.logpath, exist_ok=True)
            torch.save({"epoch": epoch, "model_state_dict": model.state_dict(), "optimizer_state_dict": opt.state_dict(),
                        **comm.checkpoint_fields(args)}, os.path.join(args.logpath, "epoch_%d.pth" % epoch))
    model.eval()
    return model


if __name__ == "__main__":
    main()

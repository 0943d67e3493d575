"""The batched box rasterizer on the MI355X: v2x_seg_rasterize (csrc/seg_raster.hip) against the float64 reference and the case table of
tests/seg_raster_refs.py under its comparison rule (labels and owner equal wherever a cell's margin is >= 1e-9 m, at most 0.01 % of a case's cells
below it, none in the exact tie case; hist = the bincount of the device's own labels), the empty call, buffer reuse, reproducibility, capture and
replay, and the labels as the training loop, the dataset reader, SegModule.step and the driver read them."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import seg_raster_refs as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _garbage(d, device):
    """Output buffers no result looks like: label 0x5b, owner -77, hist -77."""
    n, case = d["boxes"].shape[0], d["case"]
    return {"labels": torch.full((n, case.X, case.Y), 0x5b, dtype=torch.uint8, device=device),
            "owner": torch.full((n, case.X, case.Y), -77, dtype=torch.int32, device=device),
            "hist": torch.full((n, case.n_cls + 1), -77, dtype=torch.int64, device=device)}


def _inputs(d, device):
    rank = None if d["rank"] is None else torch.from_numpy(d["rank"].copy()).to(device)
    return (torch.from_numpy(d["boxes"].copy()).to(device), torch.from_numpy(d["cls"].copy()).to(device), torch.from_numpy(d["count"].copy()).to(device)), rank


def _run(device, d, want=("owner", "hist"), out=None):
    from v2x_sim_amd import ops
    args, rank = _inputs(d, device)
    res = ops.rasterize_seg(*args, d["grid"], n_classes=d["case"].n_cls, rank=rank, want=want, out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("index", range(len(SR.RASTER_CASES)), ids=SR.NAMES)
def test_sweep_against_reference(device, index):
    """Every case of the table into buffers pre-filled with garbage: every element comes back written and equal to the reference."""
    d = SR.make_case(index)
    got = _run(device, d, out=_garbage(d, device))
    SR.assert_matches(d, got["labels"], got["owner"], got["hist"])


def test_optional_outputs_may_be_null(device):
    d = SR.make_case(SR.NAMES.index("random_40x48"))
    full, bare = _run(device, d), _run(device, d, want=())
    assert set(bare) == {"labels"} and np.array_equal(bare["labels"], full["labels"])
    only_hist = _run(device, d, want=("hist",))
    assert set(only_hist) == {"labels", "hist"} and np.array_equal(only_hist["hist"], full["hist"]) and np.array_equal(only_hist["labels"], full["labels"])
    only_owner = _run(device, d, want=("owner",))
    assert set(only_owner) == {"labels", "owner"} and np.array_equal(only_owner["owner"], full["owner"])


def test_zero_items(device):
    from v2x_sim_amd import ops
    res = ops.rasterize_seg(torch.zeros((0, 8, 5), device=device), torch.zeros((0, 8), dtype=torch.uint8, device=device),
                            torch.zeros((0,), dtype=torch.int32, device=device), SR.grid_of(17, 40, 0.25), want=("owner", "hist"))
    assert res["labels"].shape == (0, 17, 40) and res["owner"].shape == (0, 17, 40) and res["hist"].shape == (0, 9)


def test_out_reuse_leaves_no_stale_element(device):
    """A dense case, then a call with every count 0 into the same buffers: all background, no owner, the histogram all in column 0."""
    from v2x_sim_amd import ops
    d = SR.make_case(SR.NAMES.index("counts_0_over_full_cap256"))
    case = d["case"]
    args, rank = _inputs(d, device)
    out = _garbage(d, device)
    res = ops.rasterize_seg(*args, d["grid"], n_classes=case.n_cls, rank=rank, out=out)
    assert all(res[k] is out[k] for k in out) and int((res["labels"] != 0).sum()) > 1000
    res = ops.rasterize_seg(args[0], args[1], torch.zeros_like(args[2]), d["grid"], n_classes=case.n_cls, rank=rank, out=out)
    torch.cuda.synchronize()
    assert int(res["labels"].count_nonzero()) == 0 and bool((res["owner"] == -1).all())
    assert res["hist"].cpu().tolist() == [[case.X * case.Y] + [0] * case.n_cls] * 3
    with pytest.raises(ValueError, match="out"):
        ops.rasterize_seg(*args, d["grid"], n_classes=case.n_cls, out={"labels": out["labels"][:, :-1].contiguous()})


def test_two_calls_give_the_same_bits(device):
    d = SR.make_case(SR.NAMES.index("random_32_classes_ranked"))
    a, b = _run(device, d, out=_garbage(d, device)), _run(device, d)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_capture_and_replay(device):
    """The call under torch.cuda.graph; the boxes, classes and counts are then changed in place and the graph replayed: the other case's reference."""
    from v2x_sim_amd import ops
    d1, d2 = SR.make_case(SR.NAMES.index("overlaps_null_rank")), SR.make_case(SR.NAMES.index("overlaps_permuted_rank"))
    (boxes, cls, count), _ = _inputs(d1, device)
    rank = torch.arange(8, dtype=torch.uint8, device=device)               # the NULL rank spelled out: the replay swaps the table's contents
    kw = dict(n_classes=8, rank=rank, want=("owner", "hist"))
    ops.rasterize_seg(boxes, cls, count, d1["grid"], **kw)                 # library loaded, allocator warm
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.rasterize_seg(boxes, cls, count, d1["grid"], **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = ops.rasterize_seg(boxes, cls, count, d1["grid"], **kw)
    graph.replay()
    torch.cuda.synchronize()
    SR.assert_matches(d1, res["labels"].cpu().numpy(), res["owner"].cpu().numpy(), res["hist"].cpu().numpy(), "captured")
    boxes.copy_(torch.from_numpy(d2["boxes"].copy()).flip(1))              # other contents, same shapes: the boxes in reverse order ...
    cls.copy_(torch.from_numpy(d2["cls"].copy()).flip(1))
    count.fill_(d2["case"].cap)                                            # ... which puts the padding rows (1000 m, class 7) first: every row is read
    rank.copy_(torch.from_numpy(d2["rank"].copy()))
    graph.replay()
    torch.cuda.synchronize()
    flipped = dict(d2, boxes=d2["boxes"][:, ::-1], cls=d2["cls"][:, ::-1], count=np.full_like(d2["count"], d2["case"].cap))
    flipped["refs"] = [SR.raster_item_ref(flipped["boxes"][m], flipped["cls"][m], flipped["count"][m], d2["grid"], 8, d2["rank"]) for m in range(6)]
    SR.assert_matches(flipped, res["labels"].cpu().numpy(), res["owner"].cpu().numpy(), res["hist"].cpu().numpy(), "replayed")
    assert not np.array_equal(flipped["refs"][0]["labels"], d1["refs"][0]["labels"])


def test_seg_targets_on_device_equals_the_host_loop(device):
    """train/loop.py::seg_targets_on_device on a synthetic batch (2 frames x 3 agents, Config's 256 x 256 grid, every box class 1) == the stacked
    utils/synthetic_scene.seg_labels maps, bit for bit; with classes, the ignore label and the histogram come through."""
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.train.loop import seg_targets_on_device
    from v2x_sim_amd.utils import synthetic_scene
    cfg = Config("train", binary=True, only_det=True)
    b = synthetic_scene.make_batch(2, 3, seed=11, ground_pts=10, clutter_pts=10, pts_per_car=4)
    lists = [b["gt_boxes"][a][f] for a in range(3) for f in range(2)]
    want = np.stack([synthetic_scene.seg_labels(g, cfg) for g in lists])
    res = seg_targets_on_device(lists, None, cfg, device, want=("hist",))
    assert res["labels"].dtype == torch.uint8 and res["labels"].is_cuda and np.array_equal(res["labels"].cpu().numpy(), want)
    assert int(want.sum()) > 500 and res["hist"].cpu()[:, 1].tolist() == want.reshape(6, -1).sum(1).tolist()
    classes = [np.where(np.arange(g.shape[0]) % 3 == 0, 200, 1 + np.arange(g.shape[0]) % 7) for g in lists]
    res = seg_targets_on_device(lists, classes, cfg, device, want=("hist", "owner"))
    lab, own = res["labels"].cpu().numpy(), res["owner"].cpu().numpy()
    assert np.array_equal(lab != 0, want == 1) and int((lab == 255).sum()) > 0      # the cars never overlap: the footprints are the same cells
    for m, c in enumerate(classes):
        hit = own[m] >= 0
        assert np.array_equal(lab[m][hit], np.where(c[own[m][hit]] >= 8, 255, c[own[m][hit]]).astype(np.uint8))
        assert np.array_equal(res["hist"][m].cpu().numpy(), SR.hist_of(lab[m], 8))


def _driver():
    spec = importlib.util.spec_from_file_location("train_seg_cli", os.path.join(ROOT, "tools", "seg", "train_seg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_seg_batch_on_device_rasterizes_a_boxes_dataset(device, tmp_path):
    """The same two frames of two agents written twice -- once with the bev_seg maps the reference paints, once with the boxes and classes -- read back
    through V2XSimSeg and seg_batch_on_device: the same labels, the same sweeps; the driver's one-pass histogram counts both kinds alike."""
    from v2x_sim_amd import ops
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.datasets import V2XSimSeg, seg_batch_on_device, write_seg_sample
    cfg = Config("train", binary=True, only_det=True)
    grid = ops.VoxelGrid(cfg.voxel_size, cfg.area_extents)
    g6 = SR.config_grid(cfg)
    rng = np.random.default_rng(4)
    T = np.stack([np.eye(4, dtype=np.float32)] * 2)
    for f in range(2):
        for a in range(2):
            k = 5 + 3 * a + f
            boxes = np.concatenate([rng.uniform(-30, 30, (k, 2)), rng.uniform(1, 9, (k, 2)), rng.uniform(-3, 3, (k, 1))], 1).astype(np.float32)
            classes = rng.choice([0, 1, 2, 3, 5, 7, 200], k).astype(np.uint8)
            idx = rng.integers(0, (256, 256, 13), (200, 3)).astype(np.int32)
            ref = SR.raster_item_ref(boxes, classes, k, g6, 8)
            assert float(ref["margin"].min()) >= SR.RASTER_MARGIN
            write_seg_sample(os.path.join(str(tmp_path), "maps"), "train", a, 2, f, idx, T, 2, ref["labels"])
            write_seg_sample(os.path.join(str(tmp_path), "boxes"), "train", a, 2, f, idx, T, 2, None, gt_boxes=boxes, gt_classes=classes)
    sets = {kind: V2XSimSeg(dataset_roots=[os.path.join(str(tmp_path), kind, "train", "agent%d" % a) for a in range(2)], config=cfg, split="train",
                            densify="none") for kind in ("maps", "boxes")}
    data = {kind: seg_batch_on_device([ds[0], ds[1]], grid, device, want=("hist",)) for kind, ds in sets.items()}
    assert data["boxes"]["labels"].dtype == torch.uint8 and data["boxes"]["labels"].shape == (4, 256, 256)
    assert torch.equal(data["boxes"]["labels"], data["maps"]["labels"]) and torch.equal(data["boxes"]["bev_seq"], data["maps"]["bev_seq"])
    assert int((data["boxes"]["labels"] == 255).sum()) > 0 and "label_hist" in data["boxes"] and "label_hist" not in data["maps"]
    mod = _driver()
    h_maps, h_boxes = (mod.dataset_label_hist(sets[kind], grid, device, 8) for kind in ("maps", "boxes"))
    assert np.array_equal(h_maps, h_boxes) and int(h_boxes.sum()) == 4 * 256 * 256 and h_boxes[8] > 0
    assert np.array_equal(h_boxes, data["boxes"]["label_hist"].sum(0).cpu().numpy())


@pytest.mark.parametrize("engine", ["hip", "hip-graph"])
def test_segmodule_step_on_rasterized_labels_with_ignore(device, tune, engine):
    """One SegModule.step on labels from the rasterizer that contain 255 (an ignore box per item) and class weights: a finite loss on both engines
    whose loss runs on csrc/seg_loss.hip -- the eager step and the step captured as one hipGraph (tools/seg/train_seg.py --engine hip-graph)."""
    from v2x_sim_amd import ops
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.seg import FaFNetSeg
    from v2x_sim_amd.train.loop import init_for_training, seg_targets_on_device
    from v2x_sim_amd.utils import synthetic_scene
    from v2x_sim_amd.utils.SegModule import SegModule
    graph = int(engine == "hip-graph")
    tune("TRAIN_HIP", 1)
    tune("TRAIN_SEG_LOSS_HIP", 1)
    tune("TRAIN_SEG_HEAD_FUSE", 1)
    tune("TRAIN_SEG_GRAPH", graph)
    cfg = Config("train", binary=True, only_det=True)
    grid = ops.VoxelGrid(cfg.voxel_size, cfg.area_extents)
    b = synthetic_scene.make_batch(1, 2, seed=21)
    lists = [np.concatenate([b["gt_boxes"][a][0], np.asarray([[3.0, -4.0, 9.0, 6.0, 0.4]], np.float32)]) for a in range(2)]
    classes = [np.asarray([1 + i % 7 for i in range(g.shape[0] - 1)] + [255]) for g in lists]
    res = seg_targets_on_device(lists, classes, cfg, device, want=("hist",))
    assert int(res["hist"][:, 8].min()) > 100 and int(res["hist"][:, 1:8].sum()) > 100
    bits = ops.voxelize_bits(torch.from_numpy(b["points"]).to(device), torch.from_numpy(b["n_pts"]).to(device), grid)
    data = {"bev_seq": ops.bits_to_dense(bits, grid.dims[2])[:, None], "trans_matrices": torch.from_numpy(b["trans"]).to(device),
            "num_agent": torch.from_numpy(b["num_agent"]), "labels": res["labels"]}
    model = init_for_training(FaFNetSeg(cfg, num_agent=2), seed=3).to(device)
    weights = ops.median_frequency_weights(res["hist"].cpu().numpy(), 8)
    opt = torch.optim.Adam(model.parameters(), lr=torch.tensor(1e-3, device=device), capturable=True) if graph else torch.optim.Adam(model.parameters(), lr=1e-3)
    module = SegModule(model, None, cfg, opt, 0, class_weight=weights)
    loss = module.step(data, 2, 1)
    assert np.isfinite(loss) and loss > 0
    assert (module._graphed is not None) == bool(graph)


def test_segmodule_pytorch_loss_path_skips_the_ignore_label(device, tune, monkeypatch):
    """SegModule.step with the kernel loss off (F.cross_entropy): a map that holds 255 gives the mean over the other cells, not an out-of-range target.
    The network is replaced by one bias vector, so the loss has a closed form: log(8) at zero logits, whatever the labels are."""
    import v2x_sim_amd.train as train_pkg
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.utils.SegModule import SegModule
    for name in ("TRAIN_HIP", "TRAIN_SEG_LOSS_HIP", "TRAIN_SEG_HEAD_FUSE", "TRAIN_SEG_GRAPH"):
        tune(name, 0)
    d = SR.make_case(SR.NAMES.index("overlaps_null_rank"))
    labels = torch.from_numpy(_run(device, d, want=())["labels"]).to(device)
    assert int((labels == 255).sum()) > 0 and int((labels == 7).sum()) > 0

    class Bias(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.b = torch.nn.Parameter(torch.zeros(8))

    monkeypatch.setattr(train_pkg, "train_forward", lambda model, bev, trans, num_agent, batch_size: model.b.expand(tuple(labels.shape) + (8,)))
    model = Bias().to(device)
    module = SegModule(model, None, Config("train"), torch.optim.SGD(model.parameters(), lr=0.1), 0)
    loss = module.step({"bev_seq": torch.zeros((6, 1, 48, 40, 13), device=device), "labels": labels}, 6, 1)
    assert abs(loss - float(np.log(8.0))) < 1e-5
    grad_sign = model.b.detach().cpu().numpy()
    assert np.isfinite(grad_sign).all() and grad_sign[0] > 0 > grad_sign[2]          # background (most cells) gains, a class that does not occur loses


def test_driver_runs_on_boxes_targets_and_balanced_weights(device, capsys, tune):
    """tools/seg/train_seg.py --targets boxes --steps 3, and a --class_weight balanced run: both complete; the balanced run prints its weights -- the
    synthetic scenes hold background and vehicles, so two classes carry a weight and the rarer one the greater."""
    for name in ("TRAIN_HIP", "TRAIN_SEG_LOSS_HIP", "TRAIN_SEG_HEAD_FUSE", "TRAIN_SEG_GRAPH"):
        tune(name, 0)                                                       # the driver's --engine sets them; restored at teardown
    mod = _driver()
    common = ["--com", "lowerbound", "--steps", "3", "--batch", "1", "--num_agent", "2", "--engine", "hip"]
    model = mod.main(common + ["--targets", "boxes"])
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert "mean loss" in capsys.readouterr().out
    mod.main(common + ["--targets", "boxes", "--class_weight", "balanced"])
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if ln.startswith("class weights (median frequency):")]
    assert len(line) == 1 and "mean loss" in out, out
    w = [float(v) for v in line[0].split(":")[1].split(",")]
    assert len(w) == 8 and w[0] > 0 and w[1] > w[0] and w[2:] == [0.0] * 6
    assert abs(1.0 / w[0] + 1.0 / w[1] - 2.0) < 1e-2                      # two classes: median = (f0 + f1) / 2 = 0.5, w = 0.5 / f (printed to 4 digits)

"""The IoU anchor assignment on the MI355X: v2x_det_assign_targets (csrc/det_assign.hip) against the float64 reference and the case table of
tests/assign_refs.py -- labels, regression mask, assoc and gt_best equal, IoUs and codes within one fp32 ulp of the rounded reference, nothing
excluded (no case of the table has an undecided element: tests/test_assign_refs_cpu.py) --, its optional outputs, the empty call, reproducibility,
capture and replay, and the targets as the detection loss and the training loop read them."""
import numpy as np
import pytest
import torch

import assign_refs as AR

pytestmark = pytest.mark.gpu
NAMES = [c.name for c in AR.ASSIGN_CASES]


def _garbage(shape, dtype, device):
    """A buffer no output value looks like: NaN floats, 0x5b bytes, -77 ints."""
    if dtype == torch.float32:
        return torch.full(shape, float("nan"), dtype=dtype, device=device)
    return torch.full(shape, 0x5b if dtype == torch.uint8 else -77, dtype=dtype, device=device)


def _run(device, d, want=("assoc", "anchor_iou"), garbage=True, **kw):
    from v2x_sim_amd import ops
    from v2x_sim_amd.ops_post import ASSIGN_OUTPUTS
    case = d["case"]
    n, shape = d["gt_boxes"].shape[0], d["anchors"].shape[:3]
    out = None
    if garbage:
        out = {k: _garbage((n,) + tuple(shape) + tail, dt, device) for k, (dt, tail) in ASSIGN_OUTPUTS.items() if k in want or k not in ("assoc", "anchor_iou")}
        out["gt_max_iou"] = _garbage((n, case.gt_cap), torch.float32, device)
        out["gt_best"] = _garbage((n, case.gt_cap), torch.int32, device)
    args = dict(pos_thr=case.pos_thr, neg_thr=case.neg_thr, force_match=bool(case.force))
    args.update(kw)
    res = ops.assign_targets(torch.from_numpy(d["gt_boxes"]).to(device), torch.from_numpy(d["gt_count"]).to(device), torch.from_numpy(d["anchors"]).to(device),
                             want=want, out=out, **args)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _within_one_ulp(got, ref64, what):
    ref32 = ref64.astype(np.float32)
    err = np.abs(got.astype(np.float64) - ref32.astype(np.float64))
    bad = ~(err <= AR.ulp32(ref32))                                         # NaN fails
    assert not bad.any(), (what, int(bad.sum()), got[bad][:4], ref32[bad][:4])


def _assert_item(got, m, ref, what):
    Q = ref["mask"].size
    assert np.array_equal(got["labels"][m].reshape(Q, 2), ref["labels"].astype(np.float32)), what
    assert np.array_equal(got["reg_loss_mask"][m].reshape(Q), ref["mask"].astype(np.uint8)), what
    assert np.array_equal(got["gt_best"][m], ref["gt_best"].astype(np.int32)), (what, got["gt_best"][m][:8], ref["gt_best"][:8])
    _within_one_ulp(got["gt_max_iou"][m], ref["gt_max_iou"], (what, "gt_max_iou"))
    _within_one_ulp(got["reg_targets"][m].reshape(Q, 6), ref["code"], (what, "code"))
    if "assoc" in got:
        assert np.array_equal(got["assoc"][m].reshape(Q), ref["assoc"].astype(np.int32)), what
    if "anchor_iou" in got:
        _within_one_ulp(got["anchor_iou"][m].reshape(Q), ref["anchor_iou"], (what, "anchor_iou"))


@pytest.mark.parametrize("index", range(len(AR.ASSIGN_CASES)), ids=NAMES)
def test_sweep_against_reference(device, index):
    """Every case of the table -- grids of one cell, one tile, ragged tiles, a second tile row and the workload's 256 x 256 x 6; 1 and 3 items with counts
    0, 1, gt_cap and gt_cap + 3; gt_cap 1, 8 and 256; the edge rows -- into buffers pre-filled with garbage: every element comes back written."""
    d = AR.make_case(index)
    got = _run(device, d)
    for m, ref in enumerate(d["refs"]):
        _assert_item(got, m, ref, (d["case"].name, m))


def test_optional_outputs_may_be_null(device):
    d = AR.make_case(NAMES.index("two_rows"))
    full, bare = _run(device, d), _run(device, d, want=())
    assert "assoc" not in bare and "anchor_iou" not in bare
    for k, v in bare.items():
        assert np.array_equal(v.view(np.uint8), full[k].view(np.uint8)), k
    only_iou = _run(device, d, want=("anchor_iou",), garbage=False)
    assert "assoc" not in only_iou and np.array_equal(only_iou["anchor_iou"].view(np.uint32), full["anchor_iou"].view(np.uint32))


def test_zero_items(device):
    from v2x_sim_amd import ops
    anchors = torch.from_numpy(AR.anchor_map(16, 16, 6)).to(device)
    res = ops.assign_targets(torch.zeros((0, 8, 5), device=device), torch.zeros((0,), dtype=torch.int32, device=device), anchors)
    assert res["labels"].shape == (0, 16, 16, 6, 2) and res["reg_loss_mask"].shape == (0, 16, 16, 6, 1) and res["gt_best"].shape == (0, 8)


def test_two_calls_give_the_same_bits(device):
    d = AR.make_case(NAMES.index("tile_cap256"))
    a, b = _run(device, d), _run(device, d, garbage=False)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def test_force_match_switch_and_thresholds(device):
    """force_match = 0 on a forced-match case: the threshold step alone (the reference with the switch off), gt_max_iou / gt_best still reported;
    neg_thr == pos_thr leaves no ignored row."""
    d = AR.make_case(NAMES.index("claims"))
    got = _run(device, d, force_match=False)
    for m in range(len(d["refs"])):
        ref = AR.assign_item_ref(d["gt_boxes"][m], d["gt_count"][m], d["anchors"], d["case"].pos_thr, d["case"].neg_thr, force_match=False)
        assert AR.n_undecided(ref) == 0
        _assert_item(got, m, ref, ("claims, no force", m))
        assert np.array_equal(ref["gt_best"], d["refs"][m]["gt_best"])
    got = _run(device, AR.make_case(NAMES.index("ragged_no_ignore")))
    assert np.all(got["labels"].sum(-1) == 1.0)


def test_capture_and_replay(device):
    """The call under torch.cuda.graph on a 16 x 16 x 6 grid; the boxes are then changed in place and the graph replayed: equal to the eager result."""
    from v2x_sim_amd import ops
    d1, d2 = AR.make_case(NAMES.index("tile_cars")), AR.make_case(NAMES.index("tile_items3"))
    anchors = torch.from_numpy(d1["anchors"]).to(device)
    boxes, count = torch.from_numpy(d1["gt_boxes"]).to(device), torch.from_numpy(d1["gt_count"]).to(device)
    ops.assign_targets(boxes, count, anchors)                               # library loaded, allocator warm
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.assign_targets(boxes, count, anchors)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = ops.assign_targets(boxes, count, anchors)
    graph.replay()
    torch.cuda.synchronize()
    eager = _run(device, d1, garbage=False)
    for k, v in res.items():
        assert np.array_equal(v.cpu().numpy().view(np.uint8), eager[k].view(np.uint8)), k
    boxes.copy_(torch.from_numpy(d2["gt_boxes"][2:3]))                      # another item's boxes, same shapes
    count.fill_(int(d2["gt_count"][2]))
    graph.replay()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in res.items()}
    _assert_item(got, 0, d2["refs"][2], "replayed")


def test_targets_feed_the_detection_loss(device):
    """32 x 32 x 6: labels / reg_targets / reg_loss_mask go into v2x_det_loss_forward as they are; the loss is finite, and an ignored row contributes
    nothing: the loss over the rows that are not ignored alone is the same."""
    from v2x_sim_amd import ops, ops_train
    anchors = AR.anchor_map(32, 32, 6)
    rng = np.random.default_rng(3)
    boxes = np.asarray([[AR._car(rng, 3.0, 3.0, yaw) for yaw in (0.0, np.pi / 8, np.pi / 4, np.pi / 2)]], np.float32)
    res = ops.assign_targets(torch.from_numpy(boxes).to(device), torch.tensor([4], dtype=torch.int32, device=device), torch.from_numpy(anchors).to(device))
    labels, reg, mask = res["labels"].reshape(-1, 2), res["reg_targets"].reshape(-1, 6), res["reg_loss_mask"].reshape(-1)
    ignored = labels.sum(1) == 0
    assert int(ignored.sum()) > 0 and int(mask.sum()) > 0 and int((labels[:, 0] == 1).sum()) > 0
    g = torch.Generator().manual_seed(1)
    cls = torch.randn((labels.shape[0], 2), generator=g).to(device)
    loc = torch.randn((labels.shape[0], 6), generator=g).to(device)
    full = ops_train.det_loss_forward(cls, labels, loc, reg, mask, 0.25, 1.0 / 9.0).cpu().numpy()
    keep = ~ignored
    part = ops_train.det_loss_forward(cls[keep].contiguous(), labels[keep].contiguous(), loc[keep].contiguous(), reg[keep].contiguous(),
                                      mask[keep].contiguous(), 0.25, 1.0 / 9.0).cpu().numpy()
    assert np.isfinite(full).all() and full[3] == float(mask.sum()) == part[3]
    # two fp32 sums of the same ~6000 terms in different partial orders: relative 6000 * 2^-24 at the very most
    assert np.allclose(full[:3], part[:3], rtol=4e-4, atol=0), (full, part)
    # and with the ignored rows' logits replaced, nothing moves at all: same rows, same order, bit for bit
    cls2 = cls.clone()
    cls2[ignored] = 37.0
    again = ops_train.det_loss_forward(cls2, labels, loc, reg, mask, 0.25, 1.0 / 9.0).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), full.view(np.uint32))


def test_training_loop_on_iou_targets(device):
    """train/loop.py with targets="iou": the batch's targets equal a direct assign_targets call on the padded boxes, and a training step runs on them."""
    from v2x_sim_amd import ops
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.det import FaFNet
    from v2x_sim_amd.train.loop import init_for_training, synthetic_batch_on_device, train_synthetic
    cfg = Config("train")
    a = synthetic_batch_on_device(cfg, 1, 2, 5, device, targets="iou")
    r = synthetic_batch_on_device(cfg, 1, 2, 5, device)
    assert a["labels"].shape == r["labels"].shape and a["reg_targets"].shape == r["reg_targets"].shape and a["reg_loss_mask"].dtype == r["reg_loss_mask"].dtype
    assert a["reg_loss_mask"].shape == r["reg_loss_mask"].shape and torch.equal(a["bev_seq"], r["bev_seq"])
    lists = [np.asarray(a["gt_boxes"][k][0], np.float32).reshape(-1, 5) for k in range(2)]
    cap = max(1, max(g.shape[0] for g in lists))
    boxes = np.zeros((2, cap, 5), np.float32)
    for m, g in enumerate(lists):
        boxes[m, :g.shape[0]] = g
    res = ops.assign_targets(torch.from_numpy(boxes).to(device), torch.tensor([g.shape[0] for g in lists], dtype=torch.int32, device=device),
                             torch.from_numpy(__import__("v2x_sim_amd.utils.postprocess", fromlist=["x"]).build_anchor_map(cfg)).to(device))
    assert torch.equal(res["labels"], a["labels"]) and torch.equal(res["reg_targets"], a["reg_targets"])
    assert torch.equal(res["reg_loss_mask"].view(torch.bool), a["reg_loss_mask"])
    n_boxes = sum(g.shape[0] for g in lists)
    assert 0 < int((res["gt_best"] >= 0).sum()) <= n_boxes                  # the cars within reach of the grid have their anchor
    model = init_for_training(FaFNet(cfg, layer=3, kd_flag=0, num_agent=2), seed=0)
    hist = train_synthetic(model, cfg, 2, frames_per_step=1, lr=1e-3, seed=3, device=device, agents=2, targets="iou")
    assert len(hist) == 2 and all(np.isfinite(h).all() for h in hist)

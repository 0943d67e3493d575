"""Segmentation training on the HIP path: the class head fused with the loss (train/hip_graph.py::_SegHeadLoss over csrc/seg_loss.hip form (b)), the step captured as
one hipGraph (train/graph_step.py::GraphedSegTrainStep) and SegModule.step with the three switches on.  The structure and the bars are those of
tests/test_gpu_train_kernels.py::test_graphed_training_step_equals_eager: a step on these kernels has no atomics and no library-chosen algorithm in it."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _seg_batch(cfg, frames, agents, seed, device):
    """tools/seg/train_seg.py::seg_batch: synthetic scenes, vehicle footprints as class 1."""
    from v2x_sim_amd import ops
    from v2x_sim_amd.utils import synthetic_scene
    grid = ops.VoxelGrid(cfg.voxel_size, cfg.area_extents)
    b = synthetic_scene.make_batch(frames, agents, seed=seed)
    bits = ops.voxelize_bits(torch.from_numpy(b["points"]).to(device), torch.from_numpy(b["n_pts"]).to(device), grid)
    labels = np.stack([synthetic_scene.seg_labels(b["gt_boxes"][a][f], cfg) for a in range(agents) for f in range(frames)])
    return {"bev_seq": ops.bits_to_dense(bits, grid.dims[2])[:, None], "trans_matrices": torch.from_numpy(b["trans"]).to(device),
            "num_agent": torch.from_numpy(b["num_agent"]), "labels": torch.from_numpy(labels).to(device).to(torch.uint8)}


def _switches(tune, loss=1, fuse=1, graph=0):
    tune("TRAIN_HIP", 1)
    tune("TRAIN_SEG_LOSS_HIP", loss)
    tune("TRAIN_SEG_HEAD_FUSE", fuse)
    tune("TRAIN_SEG_GRAPH", graph)


def test_fused_head_and_loss_equal_the_two_nodes(device, tune):
    """_SegHeadLoss against conv1x1 + segmentation_loss (both on the kernels) on one decoder-shaped map (2, 32, 64, 32), 8 classes, class weights and ignored
    labels: the same loss bits; dx and dW bit-equal (form (b) IS the cast of form (a): the data- and weight-gradient kernels read identical operands); db -- the
    packed kernel's channel sums against v2x_cast_pad_chsum_f32's, two fixed summation orders over the same 4 096 fp32 terms per channel.  A term passes through at
    most `depth` fp32 additions, each within 2^-24 of a partial sum bounded by sum |d|: the packed kernel 4 (a thread's run) + 6 (butterfly) + 2 (waves) = 12, then
    fp64; cast_pad_chsum 16 (a thread's rows) + 64 (the row sets of a workgroup, added in order) = 80, then fp64; one rounding to fp32 each: the two differ by at
    most (12 + 80 + 2) 2^-24 sum |d| per channel."""
    from v2x_sim_amd import ops
    from v2x_sim_amd.train import hip_graph
    from v2x_sim_amd.train.loss import segmentation_loss
    g = torch.Generator().manual_seed(5)
    y = torch.randn(2, 32, 64, 32, generator=g).to(torch.bfloat16).to(device)
    w = (torch.randn(8, 32, 1, 1, generator=g) * 0.3).to(device)
    b = torch.randn(8, generator=g).to(device)
    lab = torch.randint(0, 8, (2, 32, 64), generator=g)
    lab[torch.rand(2, 32, 64, generator=g) < 0.2] = 255
    lab = lab.to(torch.uint8).to(device)
    cw = (torch.rand(8, generator=g) * 3.9 + 0.1).to(device)

    def grads(fuse):
        _switches(tune, 1, fuse)
        yy, ww, bb = y.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        loss = hip_graph.seg_head_loss(yy, ww, bb, lab, cw, 255)
        name = type(loss.grad_fn).__name__
        assert ("_SegHeadLoss" in name) == bool(fuse) and ("_SegLossHip" in name) == (not fuse), name
        loss.backward()
        return loss.detach(), yy.grad, ww.grad, bb.grad

    lf, dxf, dwf, dbf = grads(1)
    l2, dx2, dw2, db2 = grads(0)
    assert torch.equal(lf, l2)
    assert torch.equal(dxf.view(torch.int16), dx2.view(torch.int16)), "dx differs"
    assert torch.equal(dwf, dw2), "dW differs"
    logits = hip_graph.conv1x1(y, w, b, f32_out=True)
    out3 = ops.seg_loss_forward(logits, lab, cw)
    d = ops.seg_loss_backward(logits, lab, cw, out3, None).reshape(-1, 8)
    bar = (12 + 80 + 2) * 2.0 ** -24 * d.abs().double().sum(0)
    err = (dbf.double() - db2.double()).abs()
    print("db: worst |fused - two nodes| / bar = %.3g" % float((err / bar).max()))
    assert bool((err <= bar).all())
    assert float((dbf.double() - d.double().sum(0)).abs().max()) <= float(bar.max())
    # a shape the fused node does not take (W % 32 != 0) falls back to the two nodes and still differentiates
    y2 = y[:, :, :48].contiguous().requires_grad_(True)
    loss = hip_graph.seg_head_loss(y2, w.clone().requires_grad_(True), b, lab[:, :, :48].contiguous(), cw, 255)
    assert "_SegHeadLoss" not in type(loss.grad_fn).__name__
    loss.backward()
    assert bool(torch.isfinite(y2.grad.float()).all())


def _eager_steps(model, opt, batches, weight=None):
    from v2x_sim_amd.train.hip_graph import seg_train_loss
    losses = []
    for d in batches:
        loss = seg_train_loss(model, d["bev_seq"], d["labels"], d["trans_matrices"], d["num_agent"], 1, weight=weight)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def _same_state(eager, graphed, steps):
    for (k, pe), (_, pg) in zip(eager.state_dict().items(), graphed.state_dict().items()):
        if "num_batches_tracked" in k:
            # (the segmentation variants inherit the detection heads and never run them: their BatchNorm layers count nothing on either path)
            assert int(pe) == int(pg) == (0 if k.startswith(("classification.", "regression.")) else steps), k
            continue
        assert float((pe.float() - pg.float()).abs().max()) <= 1e-6 * max(float(pe.float().abs().max()), 1e-3), k


def test_graphed_seg_step_equals_eager_fafnetseg(device, tune):
    """FaFNetSeg, 2 maps: five replays of the captured step on five batches == five eager steps from the same start (losses to rtol 1e-6, parameters to 1e-6 of
    each tensor's scale, num_batches_tracked == 5); after five more replays the captured loss has decreased."""
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.seg import FaFNetSeg
    from v2x_sim_amd.train.graph_step import GraphedSegTrainStep
    from v2x_sim_amd.train.loop import init_for_training
    _switches(tune)
    cfg = Config("train", binary=True, only_det=True)
    base = init_for_training(FaFNetSeg(cfg, num_agent=2), seed=1).to(device)
    batches = [_seg_batch(cfg, 1, 2, 10 + i, device) for i in range(5)]
    cw = [0.5, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    eager = copy.deepcopy(base).train()
    losses_e = _eager_steps(eager, torch.optim.SGD(eager.parameters(), lr=1e-2), batches, weight=cw)
    graphed = copy.deepcopy(base).train()
    step = GraphedSegTrainStep(graphed, torch.optim.SGD(graphed.parameters(), lr=1e-2), batches[0], 1, class_weight=cw)
    losses_g = [float(step(d)) for d in batches]
    print("eager  ", ["%.5f" % v for v in losses_e])
    print("graphed", ["%.5f" % v for v in losses_g])
    assert np.allclose(losses_g, losses_e, rtol=1e-6)
    _same_state(eager, graphed, 5)
    for i in range(5):
        last = float(step(batches[i]))
    print("captured loss after five more replays: %.5f (first %.5f)" % (last, losses_g[0]))
    assert np.isfinite(last) and last < losses_g[0]
    with pytest.raises(ValueError):
        step(dict(batches[0], labels=batches[0]["labels"][:1]))


def test_graphed_seg_step_equals_eager_v2vnetseg(device, tune):
    """V2VNetSeg, one frame of 2 agents, SGD: the same check over three batches; a batch with another num_agent table is refused."""
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.seg import V2VNetSeg
    from v2x_sim_amd.train.graph_step import GraphedSegTrainStep
    from v2x_sim_amd.train.loop import init_for_training
    _switches(tune)
    cfg = Config("train", binary=True, only_det=True)
    base = init_for_training(V2VNetSeg(cfg, num_agent=2), seed=2).to(device)
    batches = [_seg_batch(cfg, 1, 2, 20 + i, device) for i in range(3)]
    eager = copy.deepcopy(base).train()
    losses_e = _eager_steps(eager, torch.optim.SGD(eager.parameters(), lr=1e-2), batches)
    graphed = copy.deepcopy(base).train()
    step = GraphedSegTrainStep(graphed, torch.optim.SGD(graphed.parameters(), lr=1e-2), batches[0], 1)
    losses_g = [float(step(d)) for d in batches]
    print("eager  ", ["%.5f" % v for v in losses_e])
    print("graphed", ["%.5f" % v for v in losses_g])
    assert np.allclose(losses_g, losses_e, rtol=1e-6)
    _same_state(eager, graphed, 3)
    other = dict(batches[0], num_agent=torch.ones_like(batches[0]["num_agent"]))
    with pytest.raises(ValueError):
        step(other)


def test_segmodule_step_with_the_switches_on(device, tune):
    """SegModule.step with TRAIN_SEG_LOSS_HIP / _HEAD_FUSE / _GRAPH = 1 and a capturable Adam: takes the captured path (one step cached on the optimizer, reused);
    with TRAIN_SEG_GRAPH = 0 an eager step afterwards sees the replayed weights (its loss continues the run, far below the start); predict() still runs and
    answers like a fresh copy holding the same state_dict."""
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.seg import FaFNetSeg
    from v2x_sim_amd.train.graph_step import GraphedSegTrainStep
    from v2x_sim_amd.train.loop import init_for_training
    from v2x_sim_amd.utils.SegModule import SegModule
    _switches(tune, graph=1)
    cfg = Config("train", binary=True, only_det=True)
    model = init_for_training(FaFNetSeg(cfg, num_agent=2), seed=3).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=torch.tensor(1e-3, device=device), capturable=True)
    module = SegModule(model, None, cfg, opt, 0, class_weight=[1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    batches = [_seg_batch(cfg, 1, 2, 40 + i, device) for i in range(4)]
    with torch.no_grad():
        model.eval()
        module.predict(batches[0])                       # packs the initial weights for inference
    losses = [module.step(batches[i % 4], 2, 1) for i in range(12)]
    cache = opt.__dict__["_v2x_graphed_steps"]
    assert len(cache) == 1 and isinstance(next(iter(cache.values())), GraphedSegTrainStep) and module._graphed[1] is next(iter(cache.values()))
    assert float(opt.state[next(iter(opt.state))]["step"]) == 12
    print("SegModule.step, captured: loss %.4f -> %.4f in 12 steps" % (losses[0], losses[-1]))
    assert np.isfinite(losses[-1]) and losses[-1] < losses[0]
    # a second module around the same optimizer reuses the captured step
    module2 = SegModule(model, None, cfg, opt, 0, class_weight=[1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    module2.step(batches[0], 2, 1)
    assert len(cache) == 1
    # an eager step after replays sees the replayed weights: its loss is the loss of a fresh copy holding the same state_dict (stale packed weights -- the
    # replays do not bump the parameters' version counters -- would give the loss of an earlier step's weights)
    from v2x_sim_amd.train.hip_graph import seg_train_loss
    twin = FaFNetSeg(cfg, num_agent=2).to(device)
    twin.load_state_dict(model.state_dict())
    twin.train()
    d = batches[1]
    with torch.no_grad():
        want = float(seg_train_loss(twin, d["bev_seq"], d["labels"], d["trans_matrices"], d["num_agent"], 1, weight=module.class_weight))
    tune("TRAIN_SEG_GRAPH", 0)
    eager_loss = module.step(d, 2, 1)
    print("eager step after 13 replays: loss %.5f, a fresh copy of the replayed weights: %.5f (the first step's: %.5f)" % (eager_loss, want, losses[0]))
    assert abs(eager_loss - want) <= 1e-6 * abs(want) and float(opt.state[next(iter(opt.state))]["step"]) == 14
    # predict() after training: the inference engine serves the trained weights
    pred, conf = module.predict(batches[2], label=batches[2]["labels"])
    fresh = FaFNetSeg(cfg, num_agent=2).to(device)
    fresh.load_state_dict(model.state_dict())
    pred2, conf2 = SegModule(fresh, None, cfg, None, 0).predict(batches[2], label=batches[2]["labels"])
    assert torch.equal(pred, pred2) and torch.equal(conf, conf2)
    assert int(conf.sum()) == batches[2]["labels"].numel()

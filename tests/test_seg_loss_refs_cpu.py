"""CPU checks of the segmentation loss' specification and references (tests/seg_loss_refs.py), of the case table the GPU sweep runs
(tests/test_gpu_seg_loss.py), and of the switches' defaults: a plain SegModule.step takes neither new path."""
import pytest
import torch
import torch.nn.functional as F

import seg_loss_refs as S

F64 = torch.float64


def _spec64(x, lab, w):
    from v2x_sim_amd.train.loss import segmentation_loss
    return segmentation_loss(x, lab, None if w is None else w.to(F64))


SMALL = [i for i, c in enumerate(S.SEG_CASES) if c.M <= 6000]


@pytest.mark.parametrize("index", SMALL, ids=[S.case_id(S.SEG_CASES[i]) for i in SMALL])
def test_spec_equals_cross_entropy_and_the_written_out_gradient_equals_autograd(index):
    """train/loss.py::segmentation_loss in float64 == F.cross_entropy(weight=, ignore_index=, reduction="mean") wherever a pixel counts (both ignore values of
    the table: 255 and C -- the latter mapped to 255 for torch, which knows one); == the float64 reference; its autograd gradient == the written-out formula;
    nothing counts: 0 with zero gradients."""
    c = S.SEG_CASES[index]
    x32, lab, w = S.make_case(c)
    x = x32.to(F64).requires_grad_(True)
    loss = _spec64(x, lab, w)
    ref = S.seg_loss_ref64(x32, lab, w)
    assert torch.isfinite(loss)
    assert abs(float(loss) - float(ref["loss"])) <= 1e-12 * max(1.0, abs(float(ref["loss"])))
    g = 0.75
    (loss * g).backward()
    grad = S.seg_loss_grad_ref64(x32, lab, w, g, ref)
    assert torch.isfinite(x.grad).all()
    assert float((x.grad - grad).abs().max()) <= 1e-12 * max(1e-30, float(grad.abs().max())) + 1e-300
    if float(ref["den"]) > 0:
        lab_t = torch.where(lab.long() >= c.C, torch.full_like(lab.long(), 255), lab.long())
        ce = F.cross_entropy(x32.to(F64), lab_t, weight=None if w is None else w.to(F64), ignore_index=255, reduction="mean")
        assert abs(float(ce) - float(loss)) <= 1e-12 * max(1.0, abs(float(ce)))
    else:
        assert float(loss) == 0.0 and float(x.grad.abs().max()) == 0.0
    if c.labels == "all_ignored":
        assert float(ref["den"]) == 0.0 and float(loss) == 0.0 and float(x.grad.abs().max()) == 0.0


def test_spec_accepts_long_labels_and_refuses_an_ignore_index_that_is_a_class():
    from v2x_sim_amd.train.loss import segmentation_loss
    x = torch.randn(2, 3, 5, 8, dtype=F64)
    lab = torch.randint(0, 8, (2, 3, 5))
    lab[0, 0, 0] = 255
    a = segmentation_loss(x, lab.to(torch.uint8))
    b = segmentation_loss(x, lab)
    assert float(a) == float(b) == pytest.approx(float(F.cross_entropy(x.reshape(-1, 8), lab.reshape(-1), ignore_index=255)), rel=1e-12)
    with pytest.raises(ValueError):
        segmentation_loss(x, lab, ignore_index=3)
    with pytest.raises(ValueError):
        segmentation_loss(x, lab[:1])


def test_packed_reference_is_one_rounding_with_zero_padding():
    c = next(k for k in S.SEG_CASES if k.C == 12 and k.M < 6000 and k.labels != "all_ignored")
    x, lab, w = S.make_case(c)
    grad = S.seg_loss_grad_ref64(x, lab, w, 1.0)
    out, sums = S.packed_ref64(grad, 16)
    assert out.shape == (c.M, 16) and float(out[:, 12:].abs().max()) == 0.0
    big = grad.abs() >= 2.0 ** -100
    assert float(((out[:, :12] - grad).abs()[big] / grad.abs()[big]).max()) <= 2.0 ** -8
    assert torch.equal(out[:, :12].to(torch.bfloat16).to(F64)[big], out[:, :12][big])          # representable in bf16
    assert float((sums - grad.sum(0)).abs().max()) == 0.0


def test_integer_cases_have_integer_gradients():
    """logits "int" with g = den: every gradient is -w, 0 or +w exactly (the softmax is one-hot in float64 to 1e-76)."""
    for c in (k for k in S.SEG_CASES if k.logits == "int" and k.M < 100000):
        x, lab, w = S.make_case(c)
        ref = S.seg_loss_ref64(x, lab, w)
        assert float(ref["den"]) > 0 and float(ref["den"]) == round(float(ref["den"])) < 2 ** 24
        grad = S.seg_loss_grad_ref64(x, lab, w, float(ref["den"]), ref)
        assert float((grad - grad.round()).abs().max()) < 1e-60
        assert float(grad.abs().sum(0).max()) < 2 ** 24          # every partial sum is an exact fp32 integer


def test_case_table_reaches_what_it_claims():
    cs = S.SEG_CASES
    assert {c.M for c in cs} >= set(S.SMALL_M) and {c.C for c in cs} == set(S.CLASSES)
    for C in S.CLASSES:
        assert {c.Cp for c in cs if c.C == C} >= {S.r8(C), 32}
    assert {c.labels for c in cs} == set(S.LABEL_KINDS) and {c.weight for c in cs} >= set(S.WEIGHT_KINDS)
    # both sides of every cap, and the mirrors' arithmetic at them
    assert S.sl_fwd_blocks(S.FWD_CAP_M) == (S.SL_FWD_MAX_BLOCKS, S.SL_FWD_MAX_BLOCKS) and S.sl_fwd_blocks(S.FWD_CAP_M + 1) == (S.SL_FWD_MAX_BLOCKS, S.SL_FWD_MAX_BLOCKS + 1)
    assert S.sl_bwd_blocks(S.FWD_CAP_M) == (S.SL_BWD_MAX_BLOCKS, S.SL_BWD_MAX_BLOCKS) and S.sl_bwd_blocks(S.FWD_CAP_M + 1) == (S.SL_BWD_MAX_BLOCKS, S.SL_BWD_MAX_BLOCKS + 1)
    assert S.sl_pk_blocks(S.PK_CAP_M) == (S.SL_PK_MAX_BLOCKS, S.SL_PK_MAX_BLOCKS) and S.sl_pk_blocks(S.PK_CAP_M + 1) == (S.SL_PK_MAX_BLOCKS, S.SL_PK_MAX_BLOCKS + 1)
    for name, fn in (("forward", S.sl_fwd_blocks), ("backward", S.sl_bwd_blocks), ("packed", S.sl_pk_blocks)):
        sides = {fn(c.M)[1] > fn(c.M)[0] for c in cs}
        assert sides == {False, True}, name
        assert any(fn(c.M)[1] == fn(c.M)[0] == fn(10 ** 9)[0] for c in cs), name          # exactly at the cap
        assert any(fn(c.M)[0] > 1 and fn(c.M)[1] == fn(c.M)[0] for c in cs), name          # more than one workgroup below it
    assert max(c.M * c.C for c in cs) <= (S.FWD_CAP_M + 1) * 8
    # the saturated rows are there and every input is finite; every label kind counts pixels somewhere except "all_ignored"
    for c in (k for k in cs if k.M in (257, 5000)):
        x, lab, w = S.make_case(c)
        assert torch.isfinite(x).all()
        if c.logits == "sat":
            assert float(x.abs().max()) == 88.0 and bool((x.abs() == 60.0).any())
    for kind in S.LABEL_KINDS:
        dens = [float(S.seg_loss_ref64(*S.make_case(c))["den"]) for c in cs if c.labels == kind and c.M <= 6000]
        assert (max(dens) == 0.0) if kind == "all_ignored" else (max(dens) > 0.0)
    c = next(k for k in cs if k.labels == "ignored30" and k.M >= 5000 and k.M < 6000)
    lab = S.make_case(c)[1]
    share = float((lab >= c.C).double().mean())
    assert 0.25 < share < 0.35 and bool((lab == 255).any()) and bool((lab == c.C).any())


def test_workspace_mirror_against_the_library():
    from v2x_sim_amd import _lib
    lib = _lib.load()
    for (M, C, Cp) in [(1, 4, 0), (1, 4, 8), (5000, 12, 16), (5000, 12, 24), (5000, 12, 8), (S.PK_CAP_M + 1, 32, 32), (S.FWD_CAP_M + 1, 8, 8), (7, 6, 8), (7, 36, 64),
                       (0, 8, 8), (100, 8, 64)]:
        assert lib.v2x_seg_loss_workspace_size(M, C, Cp) == S.workspace_bytes(M, C, Cp), (M, C, Cp)
    # argument validation happens before any HIP call
    assert lib.v2x_seg_loss_forward(None, None, None, 4, 8, None, None, None) == -22
    assert lib.v2x_seg_loss_backward(None, None, None, 4, 8, None, None, None, None) == -22
    assert lib.v2x_seg_loss_backward_packed(None, None, None, 4, 8, None, None, 8, None, None, None, None) == -22


def test_switches_default_off_and_a_plain_step_takes_neither_new_path(monkeypatch):
    """TRAIN_SEG_LOSS_HIP / TRAIN_SEG_HEAD_FUSE / TRAIN_SEG_GRAPH default to 0, and SegModule.step with the defaults reaches neither the captured step nor
    hip_graph.seg_train_loss (both replaced by functions that raise): it runs train_forward + F.cross_entropy as before.  No GPU: train_forward is replaced by a
    small differentiable stand-in and the batch claims to be on the device."""
    import os
    from v2x_sim_amd import tuning
    from v2x_sim_amd.train import graph_step, hip_graph
    from v2x_sim_amd.utils import SegModule as SM
    for name in ("TRAIN_SEG_LOSS_HIP", "TRAIN_SEG_HEAD_FUSE", "TRAIN_SEG_GRAPH"):
        assert tuning._HOST_DEFAULTS[name] == 0
        if os.environ.get("V2X_" + name, "") == "":
            assert tuning.get(name) == 0

    def boom(*a, **k):
        raise AssertionError("a plain SegModule.step reached a new path")
    monkeypatch.setattr(hip_graph, "seg_train_loss", boom)
    monkeypatch.setattr(graph_step, "GraphedSegTrainStep", boom)
    for name in ("TRAIN_SEG_LOSS_HIP", "TRAIN_SEG_HEAD_FUSE", "TRAIN_SEG_GRAPH"):
        monkeypatch.setitem(tuning._host, name, 0)

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.outc = torch.nn.Linear(3, 8)
            self.stpn = torch.nn.Identity()

    class OnDevice(torch.Tensor):
        is_cuda = True

    model = Tiny()
    seen = []

    def fake_forward(m, bev, trans, num_agent, batch_size):
        seen.append(1)
        return m.outc(torch.Tensor(bev)[:, 0, :, :, :3])
    import v2x_sim_amd.train as T
    monkeypatch.setattr(T, "train_forward", fake_forward)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    mod = SM.SegModule(model, None, None, opt)
    assert mod.class_weight is None and mod.ignore_index == 255
    bev = torch.randn(2, 1, 4, 4, 3).as_subclass(OnDevice)
    lab = torch.randint(0, 8, (2, 4, 4), dtype=torch.uint8)
    before, before_b = model.outc.weight.detach().clone(), model.outc.bias.detach().clone()
    loss = mod.step({"bev_seq": bev, "labels": lab}, batch_size=1)
    want = float(F.cross_entropy(torch.nn.functional.linear(torch.Tensor(bev)[:, 0, :, :, :3], before, before_b).reshape(-1, 8), lab.reshape(-1).long()))
    assert seen == [1] and loss == pytest.approx(want, rel=1e-5)
    assert not torch.equal(model.outc.weight.detach(), before)
    assert "_v2x_graphed_steps" not in opt.__dict__ and mod._graphed is None

"""The corner localisation loss without a GPU: the references and the case table of tests/corner_loss_refs.py, the PyTorch-op
statement in train/loss.py::detection_loss(loss_type="corner_loss"), and the switch's way from the command line to the loss --
tools/det/train_codet.py --loss_type -> Config.loss_type -> FaFModule -> detection_loss / GraphedTrainStep."""
import math
import os

import numpy as np
import pytest
import torch

import corner_loss_refs as CR
import train_refs as R

F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [CR.corner_case_id(c) for c in CR.CORNER_CASES]


def _one(codes_p, codes_t, anchor, wh_axis="w_along_heading", dtype=torch.float64):
    """The loc term of ONE selected anchor through detection_loss (normaliser 1: the label is positive)."""
    from v2x_sim_amd.train.loss import detection_loss
    x = torch.tensor([[codes_p]], dtype=dtype, requires_grad=True)
    out = detection_loss({"cls": torch.zeros(1, 1, 2, dtype=dtype), "loc": x}, torch.tensor([[[0.0, 1.0]]], dtype=dtype), torch.tensor([[codes_t]], dtype=dtype),
                         torch.ones(1, 1, 1, dtype=torch.bool), loss_type="corner_loss", anchors=torch.tensor([anchor], dtype=dtype), wh_axis=wh_axis)
    return out[2], x


def _val(t):
    return float(t.detach())


def test_hand_cases():
    anchor = [10.0, -5.0, 4.0, 2.0, 0.0, 1.0]
    same = [0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    # pure translation by (3, 4): every corner moves by 5
    v, _ = _one([3.0, 4.0, 0.0, 0.0, 0.0, 1.0], same, anchor)
    assert abs(_val(v) - 20.0) < 1e-12
    # a square of side 2 turned by pi / 2 about its centre: every corner (distance sqrt 2 from the centre) moves to its neighbour's place, a side away
    sq = [0.0, 0.0, 2.0, 2.0, 0.0, 1.0]
    v, _ = _one([0.0, 0.0, 0.0, 0.0, 1.0, 0.0], same, sq)
    assert abs(_val(v) - 4 * 2.0) < 1e-12
    # ... and by pi: across the diagonal, 2 sqrt 2 each
    v, _ = _one([0.0, 0.0, 0.0, 0.0, 0.0, -1.0], same, sq)
    assert abs(_val(v) - 4 * 2.0 * math.sqrt(2.0)) < 1e-12
    # h_along_heading == the same case with (w, h) and (dw, dh) exchanged
    p, t = [0.3, -0.2, 0.4, -0.1, 0.5, 0.8], [0.1, 0.1, -0.2, 0.3, -0.1, 1.0]
    swap = lambda c: [c[0], c[1], c[3], c[2], c[4], c[5]]          # noqa: E731
    a = [1.0, 2.0, 4.5, 2.0, math.sin(0.4), math.cos(0.4)]
    vh, xh = _one(p, t, a, "h_along_heading")
    vw, xw = _one(swap(p), swap(t), swap(a), "w_along_heading")
    assert abs(_val(vh) - _val(vw)) < 1e-12 and abs(_val(vh) - _val(_one(p, t, a)[0])) > 1e-3
    vh.backward()
    vw.backward()
    assert torch.allclose(xh.grad[0, 0], xw.grad[0, 0][[0, 1, 3, 2, 4, 5]], rtol=0, atol=1e-12)
    # the kinks: prediction == target, (ds, dc) = (0, 0), the clip -- value and gradient finite, the gradient 0 where the spec says so
    v, x = _one(p, p, a)
    v.backward()
    assert _val(v) == 0.0 and float(x.grad.abs().max()) == 0.0
    v, x = _one([0.3, -0.2, 0.4, -0.1, 0.0, 0.0], t, a)
    v.backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad[0, 0, 4:].abs().max()) == 0.0
    assert abs(_val(v) - _val(_one([0.3, -0.2, 0.4, -0.1, 0.0, 1.0], t, a)[0])) < 1e-12            # value of atan2 at (0, 0): 0
    for dw, passes in ((4.0, True), (-4.0, True), (4.5, False), (-5.0, False)):
        v, x = _one([0.3, -0.2, dw, -0.1, 0.5, 0.8], t, a)
        v.backward()
        assert (float(x.grad[0, 0, 2]) != 0.0) == passes, dw
        assert abs(_val(v) - _val(_one([0.3, -0.2, max(-4.0, min(4.0, dw)), -0.1, 0.5, 0.8], t, a)[0])) < 1e-12


def test_the_table_covers_what_it_claims():
    counts = {c.n for c in CR.CORNER_CASES}
    assert counts >= {1, 255, 256, 257, 2048, 2049} and any(20000 <= n <= 99999 for n in counts)
    assert R.dl_blocks(2048)[0] == 1 and R.dl_blocks(2049)[0] == 2 and max(R.dl_blocks(n)[0] for n in counts) > 8
    for n in counts - {1, 257}:
        maps = {c.n_maps for c in CR.CORNER_CASES if c.n == n}
        assert 1 in maps or n == 514, n
        assert any(m > 1 for m in maps), n
    for axis in (CR.W, CR.H):
        for norm in ("positives", "batch"):
            mine = [c for c in CR.CORNER_CASES if c.wh_axis == axis and c.normalizer == norm and c.n == 514]
            assert {(c.mask, c.fill) for c in mine} == {("none", "draw"), ("all", "draw"), ("sparse", "zero"), ("sparse", "junk")}
    assert {c.grads for c in CR.CORNER_CASES} == {c.grads for c in R.DET_CASES}
    assert all(c.n % c.n_maps == 0 for c in CR.CORNER_CASES)
    twins = [(a, b) for a in CR.CORNER_CASES for b in CR.CORNER_CASES if a.fill == "zero" and b == a._replace(fill="junk")]
    assert len(twins) == 4
    for a, b in twins:
        ta, tb = CR.make_corner_case(a), CR.make_corner_case(b)
        mask = ta[4]
        assert torch.equal(mask, tb[4]) and not bool(mask.all())
        for k in (2, 3):
            assert torch.equal(ta[k][mask], tb[k][mask]) and float(ta[k][~mask].abs().max()) == 0.0
            bad = tb[k][~mask]
            assert bool(torch.isinf(bad).any()) and bool(torch.isnan(bad).any()) and bool((bad == 1e30).any())
    # the edge rows are where the docstring of make_corner_case puts them
    c = next(c for c in CR.CORNER_CASES if c.n == 514 and c.mask == "all")
    _, _, loc, tgt, mask, anchors = CR.make_corner_case(c)
    inside = float(torch.nextafter(torch.tensor(4.0), torch.tensor(0.0)))
    assert torch.equal(loc[0], tgt[0]) and [float(loc[k, 2]) for k in (1, 2, 3, 4)] == [4.0, -4.0, inside, 4.5] and float(loc[5, 3]) == -5.0
    assert float(tgt[6, 2]) == 4.0 and float(tgt[7, 3]) == -4.5 and float(tgt[8, 2]) == -inside
    assert float(loc[9, 4:].abs().max()) == 0.0 and float(tgt[10, 4:].abs().max()) == 0.0 and math.copysign(1.0, float(loc[12, 4])) == -1.0
    yaw_a = torch.atan2(anchors[:, 4], anchors[:, 5]).double()
    for row in (13, 14):          # the two headings lie on the two sides of the cut, less than pi / 2 apart through it
        yp = float(yaw_a[row % anchors.shape[0]] + torch.atan2(loc[row, 4], loc[row, 5]).double())
        yt = float(yaw_a[row % anchors.shape[0]] + torch.atan2(tgt[row, 4], tgt[row, 5]).double())
        assert abs(abs(yp - yt) - 6.0) < 1e-6
    assert len({(float(a[2]), float(a[3]), float(a[4])) for a in anchors}) >= 6


@pytest.mark.parametrize("index", range(len(CR.CORNER_CASES)), ids=IDS)
def test_references_on_the_table(index):
    """Per case: the floor holds; the float64 reference == detection_loss's PyTorch-op statement evaluated in float64; the written-out gradients == its
    float64 autograd; the fp32 evaluation alone stays within ALONE_REL (gradients) and 1e-5 (losses, relative); mask none: exactly 0."""
    c = CR.CORNER_CASES[index]
    cls, lab, loc, tgt, mask, anchors = CR.make_corner_case(c)
    assert CR.min_selected_distance(c, loc, tgt, mask, anchors) >= CR.FLOOR
    alpha = R.f32c(CR.ALPHA)
    ref = CR.corner_loss_ref64(cls, lab, loc, tgt, mask, anchors, c.wh_axis, alpha, c.n_maps if c.normalizer == "batch" else None)
    dc, dl = CR.corner_grads_ref64(cls, lab, loc, tgt, mask, anchors, c.wh_axis, ref["norm"], *c.grads, alpha=alpha)
    out64, dc64, dl64 = CR.corner_loss_f32(cls, lab, loc, tgt, mask, anchors, c.wh_axis, c.n_maps, c.normalizer, c.grads, dtype=F64)
    assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(dl64).all())
    for k, name in enumerate(("loss", "cls_loss", "loc_loss")):
        # (detection_loss holds alpha = 0.25 as a python float; 0.25 is exact in fp32, so the two agree)
        assert abs(float(out64[k]) - float(ref[name])) <= 1e-12 * max(1.0, abs(float(ref[name]))), name
    gs = max(float(dl.abs().max()), 1e-30)
    assert float((dl64 - dl).abs().max()) <= 1e-11 * gs and float((dc64 - dc).abs().max()) <= 1e-12 * max(float(dc.abs().max()), 1e-30)
    assert float(dl[~mask].abs().max() if bool((~mask).any()) else 0.0) == 0.0
    ex = CR.exact_rows(c, mask)
    assert float(dl[ex].abs().sum()) == 0.0
    out32, dc32, dl32 = CR.corner_loss_f32(cls, lab, loc, tgt, mask, anchors, c.wh_axis, c.n_maps, c.normalizer, c.grads)
    assert bool(torch.isfinite(dl32).all()) and float(dl32[ex].abs().sum()) == 0.0 and float(dl32[~mask].abs().sum()) == 0.0
    assert float((dl32.double() - dl).abs().max()) <= CR.ALONE_REL * gs
    for k, name in enumerate(("loss", "cls_loss", "loc_loss")):
        assert abs(float(out32[k]) - float(ref[name])) <= 1e-5 * abs(float(ref[name])) + 1e-30, name
    if c.mask == "none":
        assert float(ref["loc_loss"]) == 0.0 and float(out32[2]) == 0.0


def test_detection_loss_switch_and_errors():
    from v2x_sim_amd.train.loss import detection_loss
    c = CR.CORNER_CASES[2]
    cls, lab, loc, tgt, mask, anchors = CR.make_corner_case(c)
    m = c.n // c.n_maps
    res = {"cls": cls.view(c.n_maps, m, 2), "loc": loc.view(c.n_maps, m, 1, 6)}
    args = (lab.view(c.n_maps, m, 2), tgt.view(c.n_maps, m, 1, 6), mask.view(c.n_maps, m, 1))
    base = detection_loss(res, *args)
    # the default call is the function as it stood: smooth-L1, anchors not needed, not read
    again = detection_loss(res, *args, loss_type="faf_loss", anchors=None)
    assert all(torch.equal(a, b) for a, b in zip(base, again))
    ref = R.det_loss_ref64(cls, lab, loc, tgt, mask, 0.25, 1.0 / 9.0)
    assert abs(float(base[2]) - float(ref["loc_loss"])) <= 1e-5 * float(ref["loc_loss"])
    # corner_loss: tensor or numpy anchors, (M, 6) or (X, Y, A, 6); uint8 masks
    cor = detection_loss(res, *args, loss_type="corner_loss", anchors=anchors)
    a4 = anchors.numpy().reshape(5, 17, 1, 6)
    cor4 = detection_loss(res, args[0], args[1], args[2].to(torch.uint8), loss_type="corner_loss", anchors=a4)
    assert all(torch.equal(a, b) for a, b in zip(cor, cor4))
    assert torch.equal(cor[1], base[1]) and float(cor[2]) != float(base[2])
    r = CR.corner_loss_ref64(cls, lab, loc, tgt, mask, anchors, CR.W)
    assert abs(float(cor[2]) - float(r["loc_loss"])) <= 1e-5 * float(r["loc_loss"])
    with pytest.raises(ValueError):
        detection_loss(res, *args, loss_type="corner_loss")
    with pytest.raises(ValueError):
        detection_loss(res, *args, loss_type="iou_loss", anchors=anchors)
    with pytest.raises(ValueError):
        detection_loss(res, *args, loss_type="corner_loss", anchors=anchors, wh_axis="diagonal")
    with pytest.raises(ValueError):
        detection_loss(res, *args, loss_type="corner_loss", anchors=anchors[:7])
    with pytest.raises(ValueError):
        detection_loss(res, *args, loss_type="corner_loss", anchors=anchors[:, :5])


def test_fafmodule_reads_loss_type():
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.utils.CoDetModule import FaFModule
    data = {k: torch.zeros(2, 3) for k in ("bev_seq", "labels", "reg_targets", "reg_loss_mask")}
    keys, net = [], torch.nn.Linear(1, 1)
    for name in ("faf_loss", "corner_loss"):
        cfg = Config("train", loss_type=name)
        cfg.box_wh_axis = "h_along_heading"
        mod = FaFModule(net, None, cfg, None, 0)
        assert mod.loss_type == name
        kw = mod._loss_kwargs(torch.device("cpu"))
        keys.append(mod._graph_key(data, 1))
        if name == "faf_loss":
            assert kw == {"loss_type": "faf_loss"}
            continue
        assert kw["loss_type"] == "corner_loss" and kw["wh_axis"] == "h_along_heading"
        M = int(np.prod(mod.anchors.shape[:-1]))
        assert tuple(kw["anchors"].shape) == (M, 6) and kw["anchors"].dtype == torch.float32
        assert torch.equal(kw["anchors"], torch.from_numpy(np.ascontiguousarray(mod.anchors.reshape(-1, 6))).float())
        assert mod._loss_kwargs(torch.device("cpu"))["anchors"] is kw["anchors"]          # kept, not rebuilt per step
    assert keys[0] != keys[1] and keys[0][:-1] == keys[1][:-1]
    with pytest.raises(ValueError):
        FaFModule(torch.nn.Linear(1, 1), None, Config("train", loss_type="giou_loss"), None, 0)


def test_train_codet_hands_loss_type_to_config(monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location("train_codet_cli_corner", os.path.join(ROOT, "tools", "det", "train_codet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    assert ap.parse_args([]).loss_type == "faf_loss" and ap.parse_args(["--loss_type", "corner_loss"]).loss_type == "corner_loss"
    with pytest.raises(SystemExit):
        ap.parse_args(["--loss_type", "iou_loss"])
    # main() builds its Config from the flag: stop it right there
    import v2x_sim_amd.configs as configs
    seen = {}

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.update(kw)
        raise Stop()
    monkeypatch.setattr(configs, "Config", fake)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    with pytest.raises(Stop):
        mod.main(["--com", "lowerbound", "--loss_type", "corner_loss"])
    assert seen.get("loss_type") == "corner_loss"

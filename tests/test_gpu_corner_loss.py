"""csrc/det_corner_loss.hip (v2x_det_corner_loss_forward / _backward behind train/loss.py::detection_loss(loss_type="corner_loss")) on the MI355X, against
the float64 reference and over the case table of tests/corner_loss_refs.py (tests/test_corner_loss_refs_cpu.py checks both without a GPU), and one
end-to-end case through FaFModule.step on both engines and as the captured step.  DESIGN.md section 3.10 is the specification.

Bars.  Gradients: train_refs.fp32_bar -- per element 4 x the error of torch's own fp32 evaluation of that case against float64 (the PyTorch-op
statement, absolute corners then the difference), floor one fp32 ulp.  The three scalar losses: the bound tests/test_gpu_train_sweep.py uses for
det_loss's scalars, (run + 12) 2^-24 of the loss, not widened; the ratio against the plain 4 x bar is printed beside it as `.../4x`.
Every launch runs twice (identical bits); the outputs of the direct calls sit between NaN guard regions that must come back untouched; a case whose
unselected codes hold inf / NaN / 1e30 gives the bits of its zero-filled twin; mask none: loc_loss and dloc exactly 0; prediction == target: that row
of dloc exactly 0.

Measured on 1x MI355X (29 cases + 2 tests, 18 s of wall time with the float64 references; no case above 2 s).  Worst over the table:
  reference alone (absolute)   loss 7.5e-4, cls_loss 1.6e-3, loc_loss 2.1e-3, dcls 2.3e-7, dloc 1.6e-4
  kernel error / bar           loss 0.85, cls_loss 0.85, loc_loss 0.14, n_pos 0.89, dcls 0.40, dloc 0.41
  kernel error / plain 4 x bar loss 1.07, cls_loss 0.97, loc_loss 1.16 (one number's reference-alone error is one draw of a rounding, not a scale)
End to end (FaFNet, 2 maps, SGD 1e-3, four steps on one batch): eager HIP engine 17.0857 -> 10.1995 -> 6.4972 -> 5.0056, the captured step the same
digits bit for bit; fp32 engine's first step 17.0973 (6.8e-4 apart; loc 15.9446 against 15.9329); faf_loss on the same batch: loc 2.2140, cls equal."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import corner_loss_refs as CR
import train_refs as R

pytestmark = pytest.mark.gpu
F64 = torch.float64
U32 = 2.0 ** -24
GUARD = 64          # floats of NaN on each side of an output
IDS = [CR.corner_case_id(c) for c in CR.CORNER_CASES]


def _fp32_check(name, got, ref64, ref32, slack=None):
    """test_gpu_train_sweep.py::fp32_check: -> (worst error / bar, the reference-alone error)."""
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == ref64.shape, (name, got.dtype, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), "%s: an element is not finite" % name
    bar, alone = R.fp32_bar(ref64, ref32)
    if slack is not None:
        bar = torch.maximum(bar, torch.as_tensor(slack, dtype=F64).expand_as(bar))
    return R.worst_over_bar(got, ref64, bar), alone


def _from_corner_hip(t):
    """Whether t's autograd graph contains train/loss.py::_DetCornerLossHip's backward node."""
    todo, seen = [t.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if "_DetCornerLossHip" in type(f).__name__:
            return True
        todo += [nf for nf, _ in f.next_functions]
    return False


class _Guarded:
    """A float32 output of `numel` elements between two NaN regions of GUARD floats (8-byte aligned: GUARD is even)."""

    def __init__(self, numel, device):
        self.buf = torch.full((numel + 2 * GUARD,), float("nan"), dtype=torch.float32, device=device)
        self.view = self.buf[GUARD:GUARD + numel]

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[GUARD + self.view.numel():]).all())


def _p(t):
    return C.c_void_p(t.data_ptr())


def _direct(dev_ops, n, M, swap, grads, device):
    """The two entry points themselves, through ctypes, into guarded outputs.  -> (losses (3,), n_pos, dcls, dloc)."""
    from v2x_sim_amd import _lib
    lib = _lib.load()
    cd, ld, xd, td, md, ad = dev_ops
    out4, dcls, dloc = _Guarded(4, device), _Guarded(2 * n, device), _Guarded(6 * n, device)
    ws = _Guarded(lib.v2x_det_loss_workspace_size(n) // 4, device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    m8 = md.view(torch.uint8)
    _lib.check(lib.v2x_det_corner_loss_forward(_p(cd), _p(ld), _p(xd), _p(td), _p(m8), _p(ad), n, M, swap, CR.ALPHA, out4.ptr(), ws.ptr(), stream), "forward")
    gs = [None if w is None else torch.tensor(w, dtype=torch.float32, device=device) for w in grads]
    _lib.check(lib.v2x_det_corner_loss_backward(_p(cd), _p(ld), _p(xd), _p(td), _p(m8), _p(ad), n, M, swap, CR.ALPHA, out4.ptr(),
                                                *[None if g is None else _p(g) for g in gs], dcls.ptr(), dloc.ptr(), stream), "backward")
    torch.cuda.synchronize()
    for name, g in (("out4", out4), ("workspace", ws), ("dcls", dcls), ("dloc", dloc)):
        assert g.intact(), "%s: a guard region was written" % name
        assert not bool(torch.isnan(g.view).any()), "%s: an element was not written (or is NaN)" % name
    return out4.view[:3].clone(), out4.view[3].clone(), dcls.view.clone().view(n, 2), dloc.view.clone().view(n, 6)


def _through_detection_loss(dev_ops, c, tune, normalizer):
    from v2x_sim_amd.train.loss import detection_loss
    cd, ld, xd, td, md, ad = dev_ops
    tune("TRAIN_HIP", 1)
    tune("TRAIN_LOSS_HIP", 1)
    m = c.n // c.n_maps
    cg, xg = cd.view(c.n_maps, m, 2).clone().requires_grad_(True), xd.view(c.n_maps, m, 6).clone().requires_grad_(True)
    out = detection_loss({"cls": cg, "loc": xg}, ld.view(c.n_maps, m, 2), td.view(c.n_maps, m, 6), md.view(c.n_maps, m, 1), normalizer=normalizer,
                         loss_type="corner_loss", anchors=ad, wh_axis=c.wh_axis)
    # the kernels, not the PyTorch ops detection_loss would otherwise run: every loss hangs on the corner Function's node
    assert all(_from_corner_hip(o) for o in out), "detection_loss(loss_type='corner_loss') took its PyTorch-op path"
    sum(o * w for o, w in zip(out, c.grads) if w is not None).backward()
    return torch.stack([o.detach() for o in out]), None, cg.grad.view(-1, 2), xg.grad.view(-1, 6)


@pytest.mark.parametrize("index", range(len(CR.CORNER_CASES)), ids=IDS)
def test_corner_loss_sweep(device, tune, index):
    """normalizer "positives": the entry points themselves (incoming gradients as device scalars or null pointers, guarded outputs); "batch": through
    detection_loss, whose Function hands the gradients of unused outputs over as None.  See the module docstring for the bars."""
    c = CR.CORNER_CASES[index]
    cls, lab, loc, tgt, mask, anchors = CR.make_corner_case(c)
    n, M = c.n, c.n // c.n_maps
    alpha = R.f32c(CR.ALPHA)
    batch = c.normalizer == "batch"
    ref = CR.corner_loss_ref64(cls, lab, loc, tgt, mask, anchors, c.wh_axis, alpha, c.n_maps if batch else None)
    ref_dc, ref_dl = CR.corner_grads_ref64(cls, lab, loc, tgt, mask, anchors, c.wh_axis, ref["norm"], *c.grads, alpha=alpha)
    out32, dc32, dl32 = CR.corner_loss_f32(cls, lab, loc, tgt, mask, anchors, c.wh_axis, c.n_maps, c.normalizer, c.grads)
    swap = int(c.wh_axis == CR.H)

    def run(loc_t, tgt_t):
        dev_ops = tuple(t.to(device).contiguous() for t in (cls, lab, loc_t, tgt_t, mask, anchors))
        if batch:
            return _through_detection_loss(dev_ops, c, tune, "batch")
        return _direct(dev_ops, n, M, swap, c.grads, device)

    losses, n_pos, dcls, dloc = run(loc, tgt)
    losses2, _, dcls2, dloc2 = run(loc, tgt)
    assert torch.equal(losses, losses2) and torch.equal(dcls, dcls2) and torch.equal(dloc, dloc2), "a second launch gave other bits"
    if c.fill == "junk":
        # inf / NaN / 1e30 in the codes of unselected anchors: the bits of the same case with zeros there
        keep = mask[:, None]
        z = torch.zeros(())
        l0, _, dc0, dl0 = run(torch.where(keep, loc, z), torch.where(keep, tgt, z))
        assert torch.equal(losses, l0) and torch.equal(dcls, dc0) and torch.equal(dloc, dl0), "junk in unselected anchors changed the result"
    figs = []
    depth = -(-n // (R.DL_THREADS * R.dl_blocks(n)[0])) + 12
    for k, name in enumerate(("loss", "cls_loss", "loc_loss")):
        # test_det_loss_sweep's bound for the scalars: a thread's run of terms, six butterfly levels, two levels over the waves, 4 ulps for a term
        ratio, alone = _fp32_check(name, losses[k], ref[name], out32[k], depth * U32 * ref[name].abs())
        figs += [(name + "_alone", alone), (name + "/bar", ratio), (name + "/4x", _fp32_check(name, losses[k], ref[name], out32[k])[0])]
    if n_pos is not None:
        ratio, _ = _fp32_check("n_pos", n_pos, ref["n_pos"], lab[:, 1].sum().clamp(min=1.0))
        figs.append(("n_pos/bar", ratio))
    for name, got, r64, r32 in (("dcls", dcls, ref_dc, dc32), ("dloc", dloc, ref_dl, dl32)):
        ratio, alone = _fp32_check(name, got, r64, r32)
        figs += [(name + "_alone", alone), (name + "/bar", ratio)]
    print("corner_loss    %-52s %s" % (CR.corner_case_id(c), "  ".join("%s %.3g" % kv for kv in figs)))
    assert all(v <= 1.0 for k, v in figs if k.endswith("/bar")), figs
    dl = dloc.cpu()
    assert float(dl[~mask].abs().sum()) == 0.0, "an unselected anchor has a gradient"
    assert float(dl[CR.exact_rows(c, mask)].abs().sum()) == 0.0, "prediction == target bit for bit, yet its gradient is not 0"
    if c.mask == "none":
        assert float(losses[2]) == 0.0


def test_corner_loss_refuses_bad_operands(device):
    """n_anchors not a multiple of anchors_per_map: an error code and v2x_last_error from the C entry, ValueError from the wrappers; nothing is launched."""
    from v2x_sim_amd import _lib, ops
    lib = _lib.load()
    n = 10
    cls, lab, loc, tgt = (torch.zeros(n, k, device=device) for k in (2, 2, 6, 6))
    mask = torch.zeros(n, dtype=torch.uint8, device=device)
    anchors = torch.ones(3, 6, device=device)
    out4, ws = torch.zeros(4, device=device), torch.zeros(64, device=device)
    rc = lib.v2x_det_corner_loss_forward(_p(cls), _p(lab), _p(loc), _p(tgt), _p(mask), _p(anchors), n, 3, 0, 0.25, _p(out4), _p(ws), None)
    assert rc != 0 and b"multiple" in lib.v2x_last_error()
    rc = lib.v2x_det_corner_loss_backward(_p(cls), _p(lab), _p(loc), _p(tgt), _p(mask), _p(anchors), n, 3, 0, 0.25, _p(out4), None, None, None, _p(cls), _p(loc), None)
    assert rc != 0 and b"multiple" in lib.v2x_last_error()
    with pytest.raises(ValueError):
        ops.det_corner_loss_forward(cls, lab, loc, tgt, mask, anchors, False, 0.25)
    with pytest.raises(ValueError):
        ops.det_corner_loss_forward(cls, lab, loc, tgt, mask, anchors[:2, :5].contiguous(), False, 0.25)
    with pytest.raises(RuntimeError):
        ops.det_corner_loss_forward(cls, lab, loc, tgt, mask, torch.ones(5, 6), False, 0.25)           # anchors on the host


def test_corner_loss_trains_on_both_engines_and_captured(device, tune):
    """FaFNet, 2 agents, one frame of the default map: four FaFModule.step's on one batch with Config(loss_type="corner_loss") -- eager on the HIP engine,
    eager on V2X_TRAIN_HIP=0, and as the captured step -- and one faf_loss step for contrast.
    First-step losses of the two engines: within 2e-2, the bound tests/test_gpu_train_kernels.py puts on the first-step loss of the bf16 HIP engine
    against the fp32 engine for the smooth-L1 step (tests/test_gpu_train.py's own engine-against-engine bound, 25 % of the final loss, follows from
    it); captured == eager HIP bit for bit, every step; the fourth loss is below the first; the first loc_loss is not the smooth-L1 one."""
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.det import FaFNet
    from v2x_sim_amd.train.loop import init_for_training, synthetic_batch_on_device
    from v2x_sim_amd.utils.CoDetModule import FaFModule
    cfg = Config("train", loss_type="corner_loss")
    base = init_for_training(FaFNet(cfg, kd_flag=0, num_agent=2), seed=1).to(device)
    data = synthetic_batch_on_device(cfg, 1, 2, seed=10, device=device)
    assert int(data["reg_loss_mask"].sum()) > 0

    def steps(config, hip, graph, count=4):
        tune("TRAIN_HIP", hip)
        tune("TRAIN_GRAPH", graph)
        model = copy.deepcopy(base).train()
        module = FaFModule(model, None, config, torch.optim.SGD(model.parameters(), lr=1e-3), 0)
        out = [module.step(data, 1, 2) for _ in range(count)]
        assert (module._graphed is not None) == bool(graph)
        return out

    eager = steps(cfg, 1, 0)
    fp32 = steps(cfg, 0, 0, count=1)
    graphed = steps(cfg, 1, 1)
    faf = steps(Config("train"), 1, 0, count=1)
    print("corner_loss, eager HIP engine :", ["%.6f %.6f %.6f" % h for h in eager])
    print("corner_loss, captured step    :", ["%.6f %.6f %.6f" % h for h in graphed])
    print("corner_loss, fp32 engine      : %.6f %.6f %.6f   faf_loss, HIP engine: %.6f %.6f %.6f" % (fp32[0] + faf[0]))
    assert np.isfinite(np.asarray(eager)).all()
    for a, b in zip(eager[0], fp32[0]):
        assert abs(a - b) <= 2e-2 * abs(b), (eager[0], fp32[0])
    assert graphed == eager, "the captured corner-loss step is not the eager one bit for bit"
    assert eager[-1][0] < eager[0][0]
    assert abs(eager[0][1] - faf[0][1]) <= 1e-6 * abs(faf[0][1]) and abs(eager[0][2] - faf[0][2]) > 1e-3 * abs(faf[0][2])

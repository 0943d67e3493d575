"""csrc/seg_loss.hip (v2x_seg_loss_forward / _backward / _backward_packed) swept over the case table of tests/seg_loss_refs.py against its float64 references --
seeded, the same cases every run; tests/test_seg_loss_refs_cpu.py checks the references and that the table reaches both sides of every block cap.

Bars (the rules of tests/test_gpu_train_sweep.py).  fp32 outputs: per element 4 x the error of torch's own fp32 evaluation of that case against float64, with a
floor of one fp32 ulp of the element's reference (train_refs.fp32_bar).  Integer-valued cases: equal.  Every case launches twice and demands identical bits;
each test prints its worst figure as a fraction of its bar (pytest -s), the un-widened ratio beside a widened one as `.../4x`.

Widened bars, each derived where it is applied from the number formats and the kernels' summation runs alone (U = 2^-24, one rounding):
  loss, num, den -- single numbers: the reference-alone figure of ONE number is one draw of a rounding error, not a scale (test_gpu_train_sweep.py, "losses").
    _scalar_slack: the det-loss rule (run + 12) U of the sum, with the run of THIS kernel's threads, plus the C-term softmax of every pixel.
  gradient elements -- on the smallest cases (M = 1: C elements) the reference-alone figure is again a handful of draws, and the kernel reads den as the forward
    kernel SUMMED it in fp32, which torch's evaluation of a few terms does not pay.  _grad_slack: a first-order bound per element.
  channel sums -- _sums_slack: the packed kernel's own summation run over elements that carry _grad_slack each.

Measured on 1x MI355X (39 cases; the module: 7 s of wall time, float64 references included; the slowest case -- 2 097 153 pixels x 8 classes -- 1.7 s).  Worst error / bar, and
against the plain 4 x bar: loss 0.06 (0.44), num 0.10 (0.88), den 0.09 (0.25), gradient elements 0.10 (1.11 on ONE case, M = 1 with four elements, at most 0.14 on
the others), channel sums 0.06 (1.11 on the same case, at most 0.36 on the others); integer cases exact; form (b) bit-equal to the cast of form (a) everywhere;
at most 4.9e-5 of a case's bf16 elements differ from the float64 gradient rounded once (cap 1e-3)."""
import pytest
import torch

import seg_loss_refs as S
import train_refs as R

pytestmark = pytest.mark.gpu
F64 = torch.float64
U32 = 2.0 ** -24
FLIP_MAX = 1e-3            # share of a case's bf16 elements that may differ from the float64 gradient rounded once (test_gpu_train_sweep.py's cap)
FLIP_MIN_ELEMS = 20000     # ... asserted on cases with at least this many elements (a share of a few elements is a draw); printed for every case


def show(family, case, figs):
    print("%-14s %-44s %s" % (family, case, "  ".join("%s %.3g" % kv for kv in figs)))


def fp32_check(name, got, ref64, ref32, slack=None):
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == ref64.shape, (name, got.dtype, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), "%s: an element is not finite" % name
    bar, alone = R.fp32_bar(ref64, ref32)
    plain = R.worst_over_bar(got, ref64, bar)
    if slack is not None:
        bar = torch.maximum(bar, torch.as_tensor(slack, dtype=F64).expand_as(bar))
    return R.worst_over_bar(got, ref64, bar), alone, plain


def _scalar_slack(c, ref):
    """First-order bounds of the forward kernels' three numbers.
    One pixel: e_j = expf(x_j - max) carries 2 U relative (libm) and |x_j - max| U from the rounded argument, at most 0.37 U of s >= 1 absolute per term; the sum of
    C terms C - 1 roundings: s within (1.4 C + 2) U relative, log(s) within that absolutely plus 2 U log(s); (max - x_label) one rounding; their sum one more:
    |d nll_i| <= U (2 C + 8 + 2 nll_i) for C >= 4.  Times w_i: one rounding.
    The sums (terms >= 0): a thread's run of fwd_run(M) terms, six butterfly levels, two levels over the waves, then fp64: (run + 8) U of the sum.
      num within U [(run + 11) num + (2 C + 8) den];   den within U (run + 8) den;
      loss = (float)(num / den) in fp64, one rounding: U [(2 run + 20) loss + (2 C + 8)].   -> {name: bound}"""
    run = S.fwd_run(c.M)
    num, den, loss = (abs(float(ref[k])) for k in ("num", "den", "loss"))
    per_pixel = 2 * c.C + 8
    return {"num": U32 * ((run + 11) * num + per_pixel * den), "den": U32 * (run + 8) * den,
            "loss": U32 * ((2 * run + 20) * loss + (per_pixel if den > 0 else 0.0))}


def _grad_slack(c, ref, g, lab):
    """First-order bound per gradient element d_ij = k w_i (p_ij - [j == l_i]), k = g / den.
    p_ij = e_j * (1 / s): e_j as above (2 U relative, 0.37 U of s absolute), s within (1.4 C + 2) U, the reciprocal and the product one rounding each:
    |d p_ij| <= U [p_ij (1.4 C + 6) + 0.4]; the label's element -(sum of the others) / s the same with one sum more.  k = g / den: one rounding, and den itself
    within (run + 8) U (its own slack); times w_i, times the difference: two roundings.  So
      |d d_ij| <= U k w_i [ |p_ij - [j == l_i]| (1.4 C + run + 18) + 0.4 ]."""
    den = float(ref["den"])
    k = abs(float(g)) / (den if den > 0 else 1.0)
    _, safe, valid = S.pixel_weights64(lab, c.C, None)
    onehot = torch.zeros_like(ref["p"]).scatter_(1, safe[:, None], 1.0) * valid.to(F64)[:, None]
    return U32 * k * ref["w"][:, None] * ((ref["p"] - onehot).abs() * (1.4 * c.C + S.fwd_run(c.M) + 18) + 0.4)


def _sums_slack(c, grad64, gslack):
    """sums[c] = sum over the pixels of the fp32 gradients: every element carries its _grad_slack; the additions of terms of both signs are bounded on the sum of
    the magnitudes: a thread's run of pk_run(M) terms, six butterfly levels, two over the waves, then fp64 and one rounding: (run + 9) U sum |d_ij|."""
    return gslack.sum(0) + U32 * (S.pk_run(c.M) + 9) * grad64.abs().sum(0)


@pytest.mark.parametrize("index", range(len(S.SEG_CASES)), ids=[S.case_id(c) for c in S.SEG_CASES])
def test_seg_loss_sweep(device, index):
    from v2x_sim_amd import _lib, ops
    c = S.SEG_CASES[index]
    x, lab, w = S.make_case(c)
    ref = S.seg_loss_ref64(x, lab, w)
    integer = c.logits == "int"
    g = float(ref["den"]) if integer else 0.75
    grad64 = S.seg_loss_grad_ref64(x, lab, w, g, ref)
    loss32, num32, den32, grad32 = S.spec_f32(x, lab, w, g)
    assert _lib.load().v2x_seg_loss_workspace_size(c.M, c.C, c.Cp) == S.workspace_bytes(c.M, c.C, c.Cp) > 0
    xd, ld, wd = x.to(device), lab.to(device), None if w is None else w.to(device)
    gd = torch.tensor(g, dtype=torch.float32, device=device)

    def run():
        out3 = ops.seg_loss_forward(xd, ld, wd)
        assert out3 is not None, "the kernels refused a shape of their table"
        da = ops.seg_loss_backward(xd, ld, wd, out3, gd)
        dyp, sums = ops.seg_loss_backward_packed(xd, ld, wd, out3, gd, c.Cp)
        return out3, da, dyp, sums

    out3, da, dyp, sums = run()
    again = run()
    assert all(torch.equal(a, b) for a, b in zip((out3, da, dyp, sums), again)), "a second launch gave other bits"
    figs = []
    # ---- forward: loss, num, den
    sl = _scalar_slack(c, ref)
    for k, (name, r32) in enumerate((("loss", loss32), ("num", num32), ("den", den32))):
        ratio, alone, plain = fp32_check(name, out3[k], ref[name], r32, sl[name])
        figs += [(name + "_alone", alone), (name + "/bar", ratio), (name + "/4x", plain)]
    if w is None or integer:
        assert float(out3[2]) == float(ref["den"]), "the count of the pixels that count is not the exact integer"
    if float(ref["den"]) == 0.0:
        assert float(out3[0]) == 0.0 and float(out3[1]) == 0.0 and float(da.abs().max()) == 0.0 and float(sums.abs().max()) == 0.0
    # ---- form (a)
    assert da.shape == x.shape and dyp.shape == (c.M, c.Cp) and dyp.dtype == torch.bfloat16 and sums.shape == (c.C,)
    if integer:
        assert torch.equal(da.cpu(), grad64.float()), "%d elements differ from the exact integers" % int((da.cpu() != grad64.float()).sum())
        assert torch.equal(sums.cpu(), grad64.sum(0).float()), "the channel sums are not the exact integers"
    else:
        gslack = _grad_slack(c, ref, g, lab)
        ratio, alone, plain = fp32_check("dlogits", da, grad64, grad32, gslack)
        figs += [("d_alone", alone), ("d/bar", ratio), ("d/4x", plain)]
        ratio, alone, plain = fp32_check("sums", sums, grad64.sum(0), grad32.sum(0), _sums_slack(c, grad64, gslack))
        figs += [("sums_alone", alone), ("sums/bar", ratio), ("sums/4x", plain)]
    # ---- form (b): what cast_pad_chsum makes of form (a), bit for bit; padding exactly zero
    packed = ops.cast_pad_chsum(da, c.Cp)
    assert packed is not None
    assert torch.equal(dyp.view(torch.int16), packed[0].view(torch.int16)), "form (b) is not the bf16 cast of form (a)"
    if c.Cp > c.C:
        assert int((dyp[:, c.C:].view(torch.int16) != 0).sum()) == 0, "a padding channel is not exactly zero"
    ref_b, _ = S.packed_ref64(grad64, c.Cp)
    normal = grad64.abs() >= 2.0 ** -120          # below, bf16 is denormal: bf16r64 does not model it
    flips = float((dyp[:, :c.C].cpu().to(F64)[normal] != ref_b[:, :c.C][normal]).double().mean()) if bool(normal.any()) else 0.0
    figs.append(("flips", flips))
    show("seg_loss", S.case_id(c), figs)
    assert all(v <= 1.0 for k, v in figs if k.endswith("/bar")), figs
    if grad64.numel() >= FLIP_MIN_ELEMS:
        assert flips <= FLIP_MAX, flips


def test_wrappers_refuse_what_the_kernels_do_not_take(device):
    """None -- the caller's PyTorch-op path -- for class counts, label types and weights outside the kernels' table; never a launch."""
    from v2x_sim_amd import ops
    x = torch.randn(64, 8, device=device)
    lab = torch.zeros(64, dtype=torch.uint8, device=device)
    out3 = ops.seg_loss_forward(x, lab)
    assert out3 is not None
    assert ops.seg_loss_forward(x[:, :6].contiguous(), lab) is None
    assert ops.seg_loss_forward(torch.randn(64, 36, device=device), lab) is None
    assert ops.seg_loss_forward(x, lab.long()) is None
    assert ops.seg_loss_forward(x, lab[:63]) is None
    assert ops.seg_loss_forward(x, lab, torch.ones(7, device=device)) is None
    assert ops.seg_loss_backward_packed(x, lab, None, out3, None, 24) is None
    assert ops.seg_loss_backward_packed(x, lab, None, out3, None, 4) is None


def test_segmentation_loss_takes_the_kernels_when_switched_on(device, tune):
    """train/loss.py::segmentation_loss with TRAIN_SEG_LOSS_HIP = 1: the autograd Function (loss and gradient equal to the entry points' bits); = 0: the PyTorch ops."""
    from v2x_sim_amd import ops
    from v2x_sim_amd.train.loss import segmentation_loss
    c = next(k for k in S.SEG_CASES if k.M > 5000 and k.C == 8 and k.logits == "sat" and k.M < 6000)
    x, lab, w = S.make_case(c)
    xd, ld = x.to(device).view(1, -1, 1, c.C), lab.to(device).view(1, -1, 1)
    wd = None if w is None else w.to(device)
    tune("TRAIN_HIP", 1)
    tune("TRAIN_SEG_LOSS_HIP", 0)
    xs = xd.clone().requires_grad_(True)
    spec = segmentation_loss(xs, ld, wd)
    assert "_SegLossHip" not in type(spec.grad_fn).__name__
    spec.backward()
    tune("TRAIN_SEG_LOSS_HIP", 1)
    xk = xd.clone().requires_grad_(True)
    loss = segmentation_loss(xk, ld, wd)
    assert "_SegLossHip" in type(loss.grad_fn).__name__
    (loss * 0.75).backward()
    out3 = ops.seg_loss_forward(xd.reshape(-1, c.C), ld.reshape(-1), wd)
    da = ops.seg_loss_backward(xd.reshape(-1, c.C), ld.reshape(-1), wd, out3, torch.tensor(0.75, device=device))
    assert torch.equal(loss.detach(), out3[0]) and torch.equal(xk.grad.reshape(-1, c.C), da)
    assert float((loss.detach() - spec.detach()).abs()) <= 1e-5 * float(spec.detach().abs())
    assert float((xk.grad / 0.75 - xs.grad).abs().max()) <= 1e-5 * float(xs.grad.abs().max())

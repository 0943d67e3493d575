"""The training kernels (csrc/conv_wgrad.hip, bn_train.hip, gru_train.hip, v2v_train.hip, warp_train.hip, upcat_train.hip, det_loss.hip, adam.hip
and the train_math.h they share) swept over shapes, block caps and edge values against the float64 references of tests/train_refs.py --
seeded, the same cases every run; tests/test_train_refs_cpu.py checks the references, that every table reaches the form or the side of the
cap it claims, and the conditions the assertions below rest on.  tests/test_gpu_train_kernels.py holds the same entry points against torch
fp32 at a handful of shapes; this module is where shapes and edges live.

Bars.  Exact-integer cases: torch.equal with the float64 reference.  bf16-stored outputs: the expressions of the existing tests, named where
they are applied, plus two share caps -- at most 1e-3 of a case's elements may differ at all from the float64 reference rounded once to bf16,
and at most 1e-4 may be exempted as within 1e-5 of the ReLU kink.  fp32 outputs: per element 4 x the error of torch's own fp32 evaluation of
that case against float64 (`alone` below), with a floor of one fp32 ulp of the element's reference (train_refs.fp32_bar).  Every test prints
its worst figure as a fraction of its bar (pytest -s), launches twice and demands identical bits.

Widened bars (each for its family alone; the derivation stands where it is applied, the un-widened ratio is printed beside it as `.../4x`):
  BN dgamma -- alone of the BN outputs.  The backward recomputes xhat from the saved fp32 mean and invstd, three roundings per term that torch's evaluation
    does not pay (_bn_dgamma_slack).  Against the plain 4 x bar, on the kernels as they stand (fp64 workgroup sum): 1.13 on ONE case, (M, C) = (2, 16) -- two
    terms per channel, where the reference-alone figure is the largest of 16 draws of a handful of roundings -- and at most 0.43 on the other 64.  The other BN
    outputs hold the plain bar: invstd 0.67, running_var 0.49, dbeta 1.00 (one fp32 ulp where torch's own sum is exact), mean 0.25, running_mean 0.40.
  losses -- the three scalar losses of det_loss.  The reference-alone figure of ONE number is one draw of a rounding error, not a scale (it was 2.9e-6 of
    154.4, 0.12 ulp, on the case that measured 1.19 x the plain bar with a kernel error of 1.5 ulps).  Bound: (run + 12) 2^-24 of the loss.
  fp32 gates -- floor 10 ulps instead of 1: a product of six rounded factors; 1.11 x the plain bar on the 24-element case (C = 1, H W = 4), at most 0.39 on the others.

Measured on 1x MI355X (294 cases; the module: 80 s of wall time, float64 references included; no case above 2 s).  Per family: the reference-alone fp32 error (worst case,
absolute), the kernel's worst error / bar, the worst share of bf16 roundings that differ from float64 (cap 1e-3) and of ReLU-kink exemptions (cap 1e-4):
  family            reference alone   worst error / bar                                              flips      kink
  wgrad             1.1e-3 (dW)       0.53; integers exact; WGRAD_TR / WGRAD_REDUCE4 forms bit-equal  -          -
  bn                8.8e-7 (invstd)   mean 0.25, invstd 0.67, rm 0.40, rv 0.49, dgamma 0.43,        y 9.7e-5   1.2e-5
                    5.2e-2 (dgamma)   dbeta 1.00, dx-sum 0.67; y 0.99 and dx 0.48 of one bf16 step   dx 4.8e-4
  channel_sum       9.1e-2            1.00 (one fp32 ulp, where torch's own sum is exact); ints exact -          -
  cast_pad_chsum    2.3e-6            0.54; integers exact; the bf16 map bit-equal                    -          -
  gates (NHWC)      1.1e-5 (sums)     h 0.99, dgi 1.00 of one bf16 step; sums 0.50 / 0.87            h 5.0e-4   -
                                                                                                      dgi 5.4e-4
  gates (fp32)      2.6e-7            h 0.24, dgi 0.39, dpre_n r 0.39                                 -          -
  warp_affine       1.6e-5 / 1.3e-4   forward 0.59, transpose 0.75, <d, F x> = <F^T d, x> 0.03        -          -
  v2v_message       -                 forward 0.97, backward 0.97 of the existing bars                1.3e-4     -
                                                                                                      bwd 1.7e-4
  upcat, zero_insert                  bit-equal
  det_loss          1.9e-1 (loss)     losses 0.16, n_pos 0.53, dcls 0.41, dloc 0.42                   -          -
  adam              1.6e-5 (p)        p 0.25, m 0.25, v 0.25                                          -          -
Before the two changes to bn_train.hip that this sweep led to (HISTORY.md): invstd 17.9 x the plain bar at C = 8, dx flips 1.5e-3 at C = 16, y flips 6.2e-3 on the
ill-conditioned case."""
import functools

import pytest
import torch

import train_refs as R

pytestmark = pytest.mark.gpu
F64 = torch.float64
FLIP_MAX, KINK_MAX = 1e-3, 1e-4          # per case; tests/test_train_refs_cpu.py keeps the inputs at half of each


def fp32_check(name, got, ref64, ref32, slack=None):
    """-> (worst error / bar, the reference-alone error).  got: the kernel's fp32 output (device or host).  slack: a family's written-down
    widening of the bar (a float64 tensor or number: the bar is at least this), see the module docstring."""
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == ref64.shape, (name, got.dtype, got.shape, ref64.shape)
    assert bool(torch.isfinite(got).all()), "%s: an element is not finite" % name
    bar, alone = R.fp32_bar(ref64, ref32)
    if slack is not None:
        bar = torch.maximum(bar, torch.as_tensor(slack, dtype=F64).expand_as(bar))
    return R.worst_over_bar(got, ref64, bar), alone


U32 = 2.0 ** -24          # half an fp32 ulp, relative: the bound of one rounding


def show(family, case, figs):
    print("%-14s %-44s %s" % (family, case, "  ".join("%s %.3g" % kv for kv in figs)))


def finite(*tensors):
    for t in tensors:
        assert bool(torch.isfinite(t.float()).all()), "an output element is not finite"


# ------------------------------------------------------------------------------------------------------------------ 3x3 weight gradient
@pytest.mark.parametrize("index", range(len(R.WGRAD_CASES)), ids=[R.wgrad_case_id(c) for c in R.WGRAD_CASES])
def test_wgrad_sweep(device, tune, index):
    """v2x_conv3x3_wgrad + _reduce: the library's split count is the mirror's; dW against float64 (integers: equal; random: the fp32 bar against
    autograd of F.conv2d); WGRAD_TR = 0 and WGRAD_REDUCE4 = 0 give the default form's bits."""
    from v2x_sim_amd import _lib, ops
    c = R.WGRAD_CASES[index]
    plan = R.wgrad_plan(c.N, c.H, c.W, c.Cin, c.Cout)
    assert _lib.load().v2x_conv3x3_wgrad_splits(c.N, c.H, c.W, c.Cin, c.Cout) == plan["slots"]
    x, dy = R.make_wgrad_case(c)
    xd, dyd = x.to(device), dy.to(device)
    got = ops.conv3x3_wgrad(xd, dyd, cin_out=c.cin_out)
    cin = c.cin_out or c.Cin
    ref = R.wgrad_ref64(x, dy)[:, :cin]
    assert got.shape == (c.Cout, cin, 3, 3)
    finite(got)
    if c.exact:
        assert torch.equal(got.cpu(), ref.float()), "%d of %d elements differ from the exact integers" % (int((got.cpu() != ref.float()).sum()), ref.numel())
        show("wgrad", R.wgrad_case_id(c), [("max|dW|", float(ref.abs().max()))])
    else:
        ratio, alone = fp32_check("dW", got, ref, R.wgrad_f32(x, dy)[:, :cin])
        show("wgrad", R.wgrad_case_id(c), [("alone", alone), ("worst/bar", ratio)])
        assert ratio <= 1.0, ratio
    assert torch.equal(ops.conv3x3_wgrad(xd, dyd, cin_out=c.cin_out), got), "a second launch gave other bits"
    tune("WGRAD_TR", 0)
    assert torch.equal(ops.conv3x3_wgrad(xd, dyd, cin_out=c.cin_out), got), "WGRAD_TR = 0 differs"
    tune.reset("WGRAD_TR")
    tune("WGRAD_REDUCE4", 0)
    assert torch.equal(ops.conv3x3_wgrad(xd, dyd, cin_out=c.cin_out), got), "WGRAD_REDUCE4 = 0 differs"
    tune.reset("WGRAD_REDUCE4")


# ------------------------------------------------------------------------------------------------------------------ batch-statistics BN
def _bn_dgamma_slack(c, ref, dy):
    """The one widened bar of the BN family (module docstring, "BN dgamma"): a first-order bound, from the number formats alone, of what the
    kernels' xhat costs.  bn_partial_kernel<1> recomputes xhat = (x - mean) * invstd per term from the SAVED fp32 mean and invstd: three roundings
    per term (bounded on the sum of |g xhat|), invstd's own rounding to fp32 (half an ulp of dgamma), and half an fp32 ulp of the saved mean times
    invstd |dbeta|.  torch's evaluation keeps the two statistics in its accumulation type.  Nothing here grows with the workgroup's run."""
    g = torch.where(ref["y0"] > 0, dy.double(), torch.zeros((), dtype=F64)) if c.relu else dy.double()
    # sum |g xhat| <= sqrt(sum g^2 sum xhat^2) (Cauchy-Schwarz), sum xhat^2 = M var / (var + eps) <= M
    abs_gx = torch.sqrt((g * g).sum(0) * c.M)
    return 3 * U32 * abs_gx + U32 * ref["dgamma"].abs() + U32 * ref["mean"].abs() * ref["invstd"] * ref["dbeta"].abs()


@pytest.mark.parametrize("index", range(len(R.BN_CASES)), ids=[R.c8_case_id(c) for c in R.BN_CASES])
def test_bn_train_sweep(device, tune, index):
    """v2x_bn_train_forward / _backward / _backward_dxsum in the case's BN_PARTIAL_T layout.  Statistics, running statistics, dgamma, dbeta and the
    sum of dx as stored: the fp32 bar against F.batch_norm autograd.  y and dx: the expressions of test_bn_train_kernels_vs_autograd (one bf16
    step of the value; dx exempt within 1e-5 of the ReLU kink) on the float64 reference, plus the two share caps.  Integer inputs: the mean
    (sum x / M) and dbeta (sum dy) equal the float64 values bit for bit."""
    from v2x_sim_amd import ops
    c = R.BN_CASES[index]
    tune("BN_PARTIAL_T", c.layout)
    x, dy, gamma, beta, rm0, rv0 = R.make_bn_case(c)
    eps, mom = R.bn_eps(c), R.BN_MOMENTUM
    ref = R.bn_ref64(x, dy, gamma, beta, R.f32c(eps), R.f32c(mom), rm0, rv0, c.relu)
    f32 = R.bn_f32(x, dy, gamma, beta, eps, mom, rm0, rv0, c.relu)
    xd, dyd, gd, bd = x.to(device), dy.to(device), gamma.to(device), beta.to(device)

    def run():
        rmd, rvd = rm0.to(device), rv0.to(device)
        y, mean, invstd = ops.bn_train_forward(xd, gd, bd, rmd, rvd, eps, mom, c.relu)
        dx, dgamma, dbeta = ops.bn_train_backward(xd, dyd, gd, bd, mean, invstd, c.relu)
        dx1, dgamma1, dbeta1, dsum = ops.bn_train_backward(xd, dyd, gd, bd, mean, invstd, c.relu, dx_sum=True)
        assert torch.equal(dx1, dx) and torch.equal(dgamma1, dgamma) and torch.equal(dbeta1, dbeta), "the dx-sum form changed dx, dgamma or dbeta"
        return dict(y=y, mean=mean, invstd=invstd, rm=rmd, rv=rvd, dx=dx, dgamma=dgamma, dbeta=dbeta, dsum=dsum)

    got = run()
    again = run()
    for k in got:
        assert torch.equal(got[k], again[k]), "a second launch gave other bits in %s" % k
    finite(*got.values())
    slack = {"dgamma": _bn_dgamma_slack(c, ref, dy)}
    figs = []
    plain = []           # the widened output against the un-widened 4 x bar: printed, not asserted
    for k in ("mean", "invstd", "rm", "rv", "dgamma", "dbeta"):
        ratio, alone = fp32_check(k, got[k], ref[k], f32[k], slack.get(k))
        figs.append((k, ratio))
        if k in slack:
            plain.append((k + "/4x", fp32_check(k, got[k], ref[k], f32[k])[0]))
    stored = got["dx"].cpu()
    ratio, _ = fp32_check("dsum", got["dsum"], R.bn_dxsum_ref64(stored), stored.float().sum(0))
    figs.append(("dsum", ratio))
    # y: test_bn_train_kernels_vs_autograd's expression (tol_y = 2^-7 |ybf| clamped at 2^-6) on the float64 reference rounded once
    y = got["y"].cpu().double()
    ybf = R.bf16r64(ref["y"])
    tol_y = 2.0 ** -7 * ybf.abs().clamp(min=2.0 ** -6)
    ry = float(((y - ybf).abs() / tol_y).max())
    # dx: the same test's tol_dx, its exemption within 1e-5 of the kink, on the float64 reference
    dxr = ref["dx"]
    err = (stored.double() - dxr).abs()
    kink = (ref["y0"].abs() < 1e-5) if c.relu else torch.zeros_like(err, dtype=torch.bool)
    tol_dx = 2.0 ** -7 * dxr.abs() + 2.0 ** -8 * float(dxr.abs().max()) * 2.0 ** -4 + 1e-6
    rdx = float(torch.where(kink, torch.zeros_like(err), err / tol_dx).max())
    flips_y = R.flip_share(y, ref["y"])
    flips_dx = float(((stored.double() != R.bf16r64(dxr)) & ~kink).double().mean())
    kink_share = float(kink.double().mean())
    show("bn", R.c8_case_id(c), figs + [("y/bar", ry), ("dx/bar", rdx), ("flips_y", flips_y), ("flips_dx", flips_dx), ("kink", kink_share)] + plain)
    assert all(v <= 1.0 for _, v in figs), figs
    if c.kind == "ill":      # the case exists to keep test_bn_train_kernels_vs_autograd's bar on invstd (rtol 2e-5) holding at mean / std ~ 125
        rel = float(((got["invstd"].cpu().double() - ref["invstd"]).abs() / ref["invstd"]).max())
        print("bn             %-44s invstd relative error %.3g (bar 2e-5)" % (R.c8_case_id(c), rel))
        assert rel <= 2e-5, rel
    if c.kind == "int":
        assert torch.equal(got["mean"].cpu(), ref["mean"].float()), "sum x / M is not the exact value"
        assert torch.equal(got["dbeta"].cpu(), ref["dbeta"].float()), "sum dy is not the exact integer"
    assert ry <= 1.0 and rdx <= 1.0, (ry, rdx)
    assert flips_y <= FLIP_MAX and flips_dx <= FLIP_MAX and kink_share <= KINK_MAX, (flips_y, flips_dx, kink_share)


# ------------------------------------------------------------------------------------------------------------------ channel sums
@pytest.mark.parametrize("index", range(len(R.CS_CASES)), ids=[R.c8_case_id(c) for c in R.CS_CASES])
def test_channel_sum_sweep(device, index):
    """v2x_channel_sum_bf16: integers equal the float64 sums bit for bit; random values meet the fp32 bar against torch's fp32 sum."""
    from v2x_sim_amd import _lib, ops
    c = R.CS_CASES[index]
    assert _lib.load().v2x_channel_sum_workspace_size(c.M, c.C) == R.cs_blocks(c.M, c.C)[0] * c.C * 4       # the kernel, not ops.channel_sum's torch path
    x = R.make_cs_case(c)
    xd = x.to(device)
    got = ops.channel_sum(xd)
    ref = R.channel_sum_ref64(x)
    finite(got)
    if c.kind == "int":
        assert torch.equal(got.cpu(), ref.float()), (got.cpu() - ref.float()).abs().max()
        show("channel_sum", R.c8_case_id(c), [("max|sum|", float(ref.abs().max()))])
    else:
        ratio, alone = fp32_check("sums", got, ref, x.float().sum(0))
        show("channel_sum", R.c8_case_id(c), [("alone", alone), ("worst/bar", ratio)])
        assert ratio <= 1.0, ratio
    assert torch.equal(ops.channel_sum(xd), got)


@pytest.mark.parametrize("index", range(len(R.CP_CASES)), ids=[R.cp_case_id(c) for c in R.CP_CASES])
def test_cast_pad_chsum_sweep(device, index):
    """v2x_cast_pad_chsum_f32: the bf16 map equals F.pad + one rounding; the sums as above."""
    from v2x_sim_amd import ops
    c = R.CP_CASES[index]
    x = R.make_cp_case(c)
    xd = x.to(device)
    res = ops.cast_pad_chsum(xd, c.Cp)
    assert res is not None, "the kernel refused a shape of its table"
    out, sums = res
    ref_out, ref = R.cast_pad_chsum_ref64(x, c.Cp)
    assert torch.equal(out.cpu(), ref_out)
    assert sums.shape == (c.C,)
    if c.kind == "int":
        assert torch.equal(sums.cpu(), ref.float())
        show("cast_pad_chsum", R.cp_case_id(c), [("max|sum|", float(ref.abs().max()))])
    else:
        ratio, alone = fp32_check("sums", sums, ref, x.sum(0))
        show("cast_pad_chsum", R.cp_case_id(c), [("alone", alone), ("worst/bar", ratio)])
        assert ratio <= 1.0, ratio
    out2, sums2 = ops.cast_pad_chsum(xd, c.Cp)
    assert torch.equal(out2, out) and torch.equal(sums2, sums)


# ------------------------------------------------------------------------------------------------------------------ ConvGRU gates
def _gates_nhwc_check(got_h, got_dgi, ref):
    """test_gru_gates_nhwc_vs_torch's expressions on the float64 reference rounded once: h within 2^-7 |hb| + 1e-6, dgi within
    2^-7 |gb| + 1e-6 max |gb|.  -> (h / bar, dgi / bar, flips h, flips dgi)."""
    h, dgi = got_h.cpu().double(), got_dgi.cpu().double()
    hb, gb = R.bf16r64(ref["h"]), R.bf16r64(ref["dgi"])
    rh = float(((h - hb).abs() / (2.0 ** -7 * hb.abs() + 1e-6)).max())
    rg = float(((dgi - gb).abs() / (2.0 ** -7 * gb.abs() + 1e-6 * float(gb.abs().max()))).max())
    return rh, rg, R.flip_share(h, ref["h"]), R.flip_share(dgi, ref["dgi"])


@pytest.mark.parametrize("index", range(len(R.GATES_NHWC_CASES)), ids=[R.c8_case_id(c) for c in R.GATES_NHWC_CASES])
def test_gru_gates_nhwc_sweep(device, index):
    """v2x_gru_gates_nhwc_bf16 / _bwd_bf16: h and dgi as above plus the flip cap; the six sum vectors -- dgi as stored (fp32 bar against torch's
    fp32 sum of the stored values), the r, z copies identical, dpre_n * r against float64 (fp32 bar against autograd's d bias_hh)."""
    from v2x_sim_amd import ops
    c = R.GATES_NHWC_CASES[index]
    C = c.C
    gi, bhh, dh = R.make_gates_nhwc_case(c)
    ref = R.gru_gates_ref64(gi, bhh, dh)
    f32 = R.gru_gates_f32(gi, bhh, dh)
    gid, bd, dhd = gi.to(device), bhh.to(device), dh.to(device)
    h = ops.gru_gates_nhwc(gid, bd)
    dgi, sums = ops.gru_gates_nhwc_backward(gid, bd, dhd)
    h2 = ops.gru_gates_nhwc(gid, bd)
    dgi2, sums2 = ops.gru_gates_nhwc_backward(gid, bd, dhd)
    assert torch.equal(h, h2) and torch.equal(dgi, dgi2) and torch.equal(sums, sums2), "a second launch gave other bits"
    finite(h, dgi, sums)
    rh, rg, fh, fg = _gates_nhwc_check(h, dgi, ref)
    stored = dgi.cpu()
    r1, _ = fp32_check("sums[:3C]", sums[:3 * C], stored.double().sum(0), stored.float().sum(0))
    assert torch.equal(sums[3 * C:5 * C], sums[:2 * C])
    r2, alone = fp32_check("sums[5C:]", sums[5 * C:], ref["dbhh"][2 * C:], f32["dbhh"][2 * C:])
    show("gates_nhwc", R.c8_case_id(c), [("h/bar", rh), ("dgi/bar", rg), ("flips_h", fh), ("flips_dgi", fg), ("sums_stored", r1), ("sums_dbhh_n", r2), ("alone", alone)])
    assert rh <= 1.0 and rg <= 1.0 and r1 <= 1.0 and r2 <= 1.0, (rh, rg, r1, r2)
    assert fh <= FLIP_MAX and fg <= FLIP_MAX, (fh, fg)


@pytest.mark.parametrize("index", range(len(R.GATES_F32_CASES)), ids=["%dx%dx%dx%d" % c[:4] for c in R.GATES_F32_CASES])
def test_gru_gates_f32_sweep(device, index):
    """v2x_gru_gates_f32 / _bwd_f32 on pre-activations to +-90, exact zeros and gi + b = 0: finite, and h, dgi, dpre_n * r at the fp32 bar."""
    from v2x_sim_amd import ops
    c = R.GATES_F32_CASES[index]
    gi, bhh, dh = R.make_gates_f32_case(c)
    ref = R.gru_gates_ref64(gi, bhh, dh, 1)
    f32 = R.gru_gates_f32(gi, bhh, dh, 1)
    gid, bd, dhd = gi.to(device), bhh.to(device), dh.to(device)
    h = ops.gru_gates(gid, bd)
    dgi, dn_r = ops.gru_gates_backward(gid, bd, dhd)
    dgi2, dn_r2 = ops.gru_gates_backward(gid, bd, dhd)
    assert torch.equal(ops.gru_gates(gid, bd), h) and torch.equal(dgi, dgi2) and torch.equal(dn_r, dn_r2)
    figs = []
    # Widened for this family alone (module docstring, "fp32 gates"): the floor of an element's bar is 10 fp32 ulps of its reference instead of 1.
    # d gi_r = dh (1 - z) (1 - n^2) b_n r (1 - r) is a product of six factors: six roundings of 1/2 ulp, r, z and n each within ~2 ulps (expf 1 ulp,
    # tanhf 2 ulps, the division), their complements likewise away from saturation -- ~10 ulps at first order in ANY fp32 evaluation; a case of 24
    # elements (C = 1, H W = 4) samples torch's own error too thinly for 4 x its maximum to cover that.
    for name, got, r64, r32 in (("h", h, ref["h"], f32["h"]), ("dgi", dgi, ref["dgi"], f32["dgi"]), ("dpn_r", dn_r, ref["dpn_r"], f32["dpn_r"])):
        ratio, alone = fp32_check(name, got, r64, r32, 10 * R.ulp32(r64))
        figs += [(name + "_alone", alone), (name + "/bar", ratio), (name + "/4x", fp32_check(name, got, r64, r32)[0])]
    show("gates_f32", "%dx%dx%dx%d" % c[:4], figs)
    assert all(v <= 1.0 for k, v in figs if k.endswith("/bar")), figs


def _ulps(got, ref64):
    e = (got.double() - ref64).abs() / R.ulp32(ref64)
    return float(e.max()), float(e.mean())


@pytest.mark.parametrize("P,C", R.GRU_COPY_SHAPES)
def test_gru_backward_copies_against_float64(device, P, C):
    """The two copies of the GRU backward formulas (train_math.h::tm_gru_gates_bwd in the fp32 NCHW kernel, the in-place copy in
    gru_gates_nhwc_kernel<true>) on the SAME bf16 pre-activations, each against float64: the fp32 copy in fp32 ulps (its output is fp32), the
    NHWC copy after its bf16 store (in bf16 steps and as flips of the once-rounded reference), and the number of elements on which the two
    disagree once the fp32 copy's result is rounded to bf16 too.  Both meet their bars; the figures stand in train_math.h."""
    from v2x_sim_amd import ops
    g = torch.Generator().manual_seed(P + C)
    gi = (torch.randn(P, 3 * C, generator=g) * 1.5).to(torch.bfloat16)
    bhh = torch.randn(3 * C, generator=g) * 0.5
    dh = torch.randn(P, C, generator=g).to(torch.bfloat16)
    ref = R.gru_gates_ref64(gi, bhh, dh)
    f32 = R.gru_gates_f32(gi, bhh, dh)
    # the fp32 kernel reads [maps][3C][H W] with H W % 4 == 0: one map whose pixels are the rows (padded with copies of row 0 to a multiple of 4)
    pad = (-P) % 4
    rows = torch.cat([torch.arange(P), torch.zeros(pad, dtype=torch.long)])
    gi4 = gi.float()[rows].t().contiguous().view(1, 3 * C, -1, 1).to(device)
    dh4 = dh.float()[rows].t().contiguous().view(1, C, -1, 1).to(device)
    dgi_f, _ = ops.gru_gates_backward(gi4, bhh.to(device), dh4)
    dgi_f = dgi_f.view(3 * C, -1).t()[:P].cpu()
    dgi_n, _ = ops.gru_gates_nhwc_backward(gi.to(device), bhh.to(device), dh.to(device))
    dgi_n = dgi_n.cpu()
    ratio, alone = fp32_check("dgi fp32 copy", dgi_f, ref["dgi"], f32["dgi"])
    mx, mean = _ulps(dgi_f, ref["dgi"])
    tmx, tmean = _ulps(f32["dgi"], ref["dgi"])
    _, rg, _, flips = _gates_nhwc_check(torch.zeros(1), dgi_n, dict(h=torch.zeros(1, dtype=F64), dgi=ref["dgi"]))
    flips_f = R.flip_share(R.bf16r(dgi_f), ref["dgi"])
    differ = int((R.bf16r(dgi_f) != dgi_n.float()).sum())
    print("gru copies (%d, %d): fp32 copy max %.2f / mean %.3f fp32 ulps (torch fp32: %.2f / %.3f), worst/bar %.3f;  NHWC copy worst/bar %.3f, %d of %d stored "
          "elements differ from bf16(float64) (the fp32 copy rounded to bf16: %d);  the two copies disagree on %d elements after the bf16 store"
          % (P, C, mx, mean, tmx, tmean, ratio, rg, round(flips * ref["dgi"].numel()), ref["dgi"].numel(), round(flips_f * ref["dgi"].numel()), differ))
    assert ratio <= 1.0 and rg <= 1.0 and flips <= FLIP_MAX, (ratio, rg, flips)


# ------------------------------------------------------------------------------------------------------------------ affine warp
@pytest.mark.parametrize("index", range(len(R.WARP_TRAIN_CASES)), ids=["C%d-%dx%d" % c[:3] for c in R.WARP_TRAIN_CASES])
def test_warp_affine_sweep(device, index):
    """v2x_warp_affine_f32 / _bwd_f32, one pose per map and every map judged on its own (its own torch-fp32 figure, its own bar): forward against
    F.grid_sample in float64, backward against the explicit transpose, and <d, F x> = <F^T d, x> per pose in float64 at the tolerance of
    test_warp_affine_forward_and_transpose_vs_grid_sample (1e-4 max(1, |lhs|))."""
    from v2x_sim_amd import ops
    c = R.WARP_TRAIN_CASES[index]
    x, d, th = R.make_warp_train_case(c)
    ref = R.warp_affine_ref64(x, th)
    reft = R.warp_affine_transpose_ref64(d, th)
    y32, g32 = R.warp_affine_f32(x, th, d)
    xd, dd, thd = x.to(device), d.to(device), th.to(device)
    got = ops.warp_affine(xd, thd)
    gott = ops.warp_affine(dd, thd, backward=True)
    assert torch.equal(ops.warp_affine(xd, thd), got) and torch.equal(ops.warp_affine(dd, thd, backward=True), gott)
    got, gott = got.cpu(), gott.cpu()
    bad = []
    for p, name in enumerate(R.WARP_POSE_NAMES):
        rf, af = fp32_check(name, got[p], ref[p], y32[p])
        rb, ab = fp32_check(name + "^T", gott[p], reft[p], g32[p])
        lhs = float((d[p].double() * got[p].double()).sum())
        rhs = float((gott[p].double() * x[p].double()).sum())
        rt = abs(lhs - rhs) / (1e-4 * max(1.0, abs(lhs)))
        show("warp_affine", "C%d-%dx%d %s" % (c.C, c.H, c.W, name), [("alone", af), ("fwd/bar", rf), ("alone^T", ab), ("bwd/bar", rb), ("transpose/bar", rt)])
        if rf > 1.0 or rb > 1.0 or rt > 1.0:
            bad.append((name, rf, rb, rt))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------ V2VNet's message
@functools.lru_cache(maxsize=2)
def _v2v_refs(index):
    c = R.V2V_CASES[index]
    cur, base, T, d = R.make_v2v_case(c)
    return cur, base, T, d, R.v2v_message_ref64(cur, base, T, c.A, c.B), R.v2v_message_bwd_ref64(d, T, c.A, c.B, c.two)


@pytest.mark.parametrize("index", range(len(R.V2V_CASES)), ids=[R.v2v_case_id(c) for c in R.V2V_CASES])
def test_v2v_message_sweep(device, index):
    """v2x_v2v_message_bf16 / _bwd_bf16 on the plan hip_graph._v2v_plan builds: the expressions of test_v2v_message_forward_and_backward_vs_torch on
    the float64 reference (forward 2^-8 |ref| + 2e-5 max |ref|, backward 2^-8 |ref| + 5e-5 max |ref|), the flip cap on the message half and on
    dbase, the ego half (and dcur) copied bit for bit."""
    from v2x_sim_amd import ops
    from v2x_sim_amd.models.det.base import IntermediateModelBase
    from v2x_sim_amd.train import hip_graph
    c = R.V2V_CASES[index]
    cur, base, T, d, ref, (ref_dbase, ref_dcur) = _v2v_refs(index)
    A, B, C = c.A, c.B, c.C
    N = A * B
    counts, items, rows = IntermediateModelBase.frame_plan(torch.full((B, A), A), B, A)

    class _M:
        pass
    plan = hip_graph._v2v_plan(_M(), counts, items, rows, B, A, T, N, device)
    assert plan is not None and plan["K"] == A - 1 and plan["src"].tolist() == [p[1] for p in R.v2v_pairs(A, B)[2]]
    Td = T.to(device)
    curd = cur.to(device)
    based = base.to(device) if c.two else None
    got = ops.v2v_message(curd, based, Td, plan)
    assert torch.equal(ops.v2v_message(curd, based, Td, plan), got), "a second launch gave other bits"
    got = got.cpu()
    finite(got)
    assert torch.equal(got[..., :C], cur), "the ego half is not a copy"
    msg, rmsg = got[..., C:].double(), ref[..., C:]
    rf = float(((msg - rmsg).abs() / (2.0 ** -8 * rmsg.abs() + 2e-5 * float(ref.abs().max()))).max())
    ff = R.flip_share(msg, rmsg)
    dn = d.to(device)
    dbase, dcur = ops.v2v_message_backward(dn, Td, plan, N, c.two)
    dbase2, dcur2 = ops.v2v_message_backward(dn, Td, plan, N, c.two)
    assert torch.equal(dbase, dbase2) and (dcur is None or torch.equal(dcur, dcur2))
    dbase = dbase.cpu()
    finite(dbase)
    rb = float(((dbase.double() - ref_dbase).abs() / (2.0 ** -8 * ref_dbase.abs() + 5e-5 * float(ref_dbase.abs().max()))).max())
    fb = R.flip_share(dbase, ref_dbase)
    if c.two:
        assert torch.equal(dcur.cpu().double(), ref_dcur), "dcur is not the ego half of the gradient"
    show("v2v_message", R.v2v_case_id(c), [("fwd/bar", rf), ("flips", ff), ("bwd/bar", rb), ("flips_bwd", fb)])
    assert rf <= 1.0 and rb <= 1.0, (rf, rb)
    if not c.signed:         # signed maps: cancelling sums are outside the double-rounding condition; the existing bar alone
        assert ff <= FLIP_MAX and fb <= FLIP_MAX, (ff, fb)


# ------------------------------------------------------------------------------------------------------------------ upsample + concat, zero insertion
@pytest.mark.parametrize("N,H,W,C0,C1", R.UPCAT_CASES)
def test_upcat_sweep(device, N, H, W, C0, C1):
    """v2x_upcat_bf16 / _bwd_bf16 on values whose 2 x 2 sums are exact in fp32 (train_refs.grid_values): equality with the references."""
    from v2x_sim_amd import ops
    g = torch.Generator().manual_seed(N * H + C0 + C1)
    lo, skip = R.grid_values((N, H, W, C0), g), R.grid_values((N, 2 * H, 2 * W, C1), g)
    lod, skipd = lo.to(device), skip.to(device)
    cat = ops.upcat(lod, skipd)
    assert torch.equal(cat.cpu(), R.upcat_ref(lo, skip))
    assert torch.equal(ops.upcat(lod, skipd), cat), "a second launch gave other bits"
    dcat = R.grid_values((N, 2 * H, 2 * W, C0 + C1), g)
    dcatd = dcat.to(device)
    dlo, dskip = ops.upcat_backward(dcatd, C0)
    rlo, rskip = R.upcat_backward_ref(dcat, C0)
    assert torch.equal(dlo.cpu(), rlo) and torch.equal(dskip.cpu(), rskip)
    dlo2, dskip2 = ops.upcat_backward(dcatd, C0)
    assert torch.equal(dlo2, dlo) and torch.equal(dskip2, dskip), "a second launch gave other bits"


@pytest.mark.parametrize("shape", R.ZERO_INSERT_CASES)
def test_zero_insert_sweep(device, shape):
    from v2x_sim_amd import ops
    g = torch.Generator().manual_seed(sum(shape))
    dy = torch.randn(*shape, generator=g).to(torch.bfloat16)
    dyd = dy.to(device)
    out = ops.zero_insert(dyd)
    assert torch.equal(out.cpu(), R.zero_insert_ref(dy))
    assert torch.equal(ops.zero_insert(dyd), out), "a second launch gave other bits"


# ------------------------------------------------------------------------------------------------------------------ detection loss
def _from_det_loss_hip(t):
    """Whether t's autograd graph contains train/loss.py::_DetLossHip's backward node."""
    todo, seen = [t.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if "_DetLossHip" in type(f).__name__:
            return True
        todo += [nf for nf, _ in f.next_functions]
    return False


@pytest.mark.parametrize("index", range(len(R.DET_CASES)), ids=[R.det_case_id(c) for c in R.DET_CASES])
def test_det_loss_sweep(device, tune, index):
    """csrc/det_loss.hip against the formulas at its head in float64.  normalizer "positives": the entry points themselves (the incoming gradients
    as device scalars or null pointers); "batch": through train/loss.py::detection_loss, whose autograd Function hands unused outputs' gradients
    over as None.  Losses, n_pos and both gradients at the fp32 bar against the PyTorch-op specification in fp32; one-hot labels: the positive
    count is the exact integer."""
    from v2x_sim_amd import ops
    from v2x_sim_amd.train.loss import detection_loss
    c = R.DET_CASES[index]
    cls, lab, loc, tgt, mask = R.make_det_case(c)
    alpha, beta = R.f32c(R.DET_ALPHA), R.f32c(R.DET_BETA)
    batch = c.normalizer == "batch"
    ref = R.det_loss_ref64(cls, lab, loc, tgt, mask, alpha, beta, c.n_maps if batch else None)
    ref_dc, ref_dl = R.det_loss_grads_ref64(cls, lab, loc, tgt, mask, alpha, beta, ref["norm"], *c.grads)
    out32, dc32, dl32 = R.det_loss_f32(cls, lab, loc, tgt, mask, c.n_maps, c.normalizer, c.grads)
    d = lambda t: t.to(device)          # noqa: E731
    cd, ld, xd, td, md = d(cls), d(lab), d(loc), d(tgt), d(mask)

    def run():
        if not batch:
            out4 = ops.det_loss_forward(cd, ld, xd, td, md, R.DET_ALPHA, R.DET_BETA)
            gs = [None if w is None else torch.tensor(w, dtype=torch.float32, device=device) for w in c.grads]
            dcls, dloc = ops.det_loss_backward(cd, ld, xd, td, md, R.DET_ALPHA, R.DET_BETA, out4, *gs)
            return out4[:3].clone(), out4[3].clone(), dcls, dloc
        tune("TRAIN_HIP", 1)
        tune("TRAIN_LOSS_HIP", 1)
        n = c.n // c.n_maps
        cg, xg = cd.view(c.n_maps, n, 2).clone().requires_grad_(True), xd.view(c.n_maps, n, 6).clone().requires_grad_(True)
        out = detection_loss({"cls": cg, "loc": xg}, ld.view(c.n_maps, n, 2), td.view(c.n_maps, n, 6), md.view(c.n_maps, n, 1), normalizer="batch")
        # the kernels, not the PyTorch ops detection_loss falls back to: every loss hangs (through the batch rescaling) on the Function's node
        assert all(_from_det_loss_hip(o) for o in out), "detection_loss took its PyTorch-op path"
        sum(o * w for o, w in zip(out, c.grads) if w is not None).backward()
        return torch.stack([o.detach() for o in out]), None, cg.grad.view(-1, 2), xg.grad.view(-1, 6)

    losses, n_pos, dcls, dloc = run()
    losses2, _, dcls2, dloc2 = run()
    assert torch.equal(losses, losses2) and torch.equal(dcls, dcls2) and torch.equal(dloc, dloc2), "a second launch gave other bits"
    figs = []
    # The three losses are single numbers: the reference-alone figure of ONE number is one draw of a rounding error (it is 0 now and then), not a
    # scale, so 4 x it is no bar.  Widened for these three alone (module docstring, "losses") to the first-order bound of the kernel's own sum of
    # non-negative terms: a thread's run of ceil(n / (256 blocks)) terms, six butterfly levels, two levels over the waves (then fp64), plus 4 ulps
    # for a term's own expf / logf -- (run + 12) 2^-24 of the loss.
    depth = -(-c.n // (R.DL_THREADS * R.dl_blocks(c.n)[0])) + 12
    for k, name in enumerate(("loss", "cls_loss", "loc_loss")):
        ratio, alone = fp32_check(name, losses[k], ref[name], out32[k], depth * U32 * ref[name].abs())
        figs += [(name + "_alone", alone), (name + "/bar", ratio), (name + "/4x", fp32_check(name, losses[k], ref[name], out32[k])[0])]
    if n_pos is not None:
        ratio, _ = fp32_check("n_pos", n_pos, ref["n_pos"], lab[:, 1].sum().clamp(min=1.0))
        figs.append(("n_pos/bar", ratio))
        if "one-hot" in c.reach:
            assert float(n_pos) == float(ref["n_pos"]), "the positive count is not the exact integer"
    for name, got, r64, r32 in (("dcls", dcls, ref_dc, dc32), ("dloc", dloc, ref_dl, dl32)):
        ratio, alone = fp32_check(name, got, r64, r32)
        figs += [(name + "_alone", alone), (name + "/bar", ratio)]
    show("det_loss", R.det_case_id(c), figs)
    assert all(v <= 1.0 for k, v in figs if k.endswith("/bar")), figs
    if c.mask == "none":
        assert float(losses[2]) == 0.0 and float(dloc.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------ Adam
@pytest.mark.parametrize("index", range(len(R.ADAM_CASES)), ids=[R.adam_case_id(c) for c in R.ADAM_CASES])
def test_adam_sweep(device, tune, index):
    """v2x_adam_step_f32 behind train/optim.py::HipAdam, ONE step from a given state (sizes around ADAM_BLOCK_ELEMS, a zero-element tensor, host or
    device learning rate and step counters): p, m, v at the fp32 bar against torch.optim.Adam's fp32 step on the CPU; g = 0 from a zero state
    without weight decay leaves p untouched (no NaN at eps > 0)."""
    from v2x_sim_amd.train.optim import HipAdam, use_hip_adam
    c = R.ADAM_CASES[index]
    tune("TRAIN_ADAM_HIP", 1)
    tensors = R.make_adam_case(c)
    kw = dict(betas=R.ADAM_BETAS, eps=R.ADAM_EPS, weight_decay=c.wd)

    lr32 = R.f32c(R.ADAM_LR) if c.device_lr else R.ADAM_LR       # a device learning rate is an fp32 tensor

    def stepped(dev, hip):
        ps = [torch.nn.Parameter(p.clone().to(dev)) for p, _, _, _ in tensors]
        if hip and c.device_lr:      # capturable: learning rate and step counters live on the device
            opt = torch.optim.Adam(ps, lr=torch.tensor(R.ADAM_LR, dtype=torch.float32, device=dev), capturable=True, **kw)
        else:                        # (torch's capturable form needs a GPU: the CPU reference takes the same fp32 learning rate as a float)
            opt = torch.optim.Adam(ps, lr=lr32, **({} if hip else {"foreach": False}), **kw)
        if hip:
            opt = use_hip_adam(opt)
            assert isinstance(opt, HipAdam)
        for q, (_, g, m, v) in zip(ps, tensors):
            q.grad = g.clone().to(dev)
            opt.state[q] = {"step": torch.tensor(float(c.step - 1), dtype=torch.float32, device=dev if hip and c.device_lr else "cpu"),
                            "exp_avg": m.clone().to(dev), "exp_avg_sq": v.clone().to(dev)}
        opt.step()
        return [(q.detach().cpu(), opt.state[q]["exp_avg"].cpu(), opt.state[q]["exp_avg_sq"].cpu(), float(opt.state[q]["step"])) for q in ps]

    got, again, f32 = stepped(device, True), stepped(device, True), stepped("cpu", False)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    alone = {"p": 0.0, "m": 0.0, "v": 0.0}
    for (p, g, m, v), o, o2, t in zip(tensors, got, again, f32):
        assert all(torch.equal(a, b) for a, b in zip(o[:3], o2[:3])), "a second launch gave other bits"
        assert o[3] == float(c.step) == t[3]
        ref = R.adam_ref64(p, g, m, v, c.step, lr32, R.ADAM_BETAS[0], R.ADAM_BETAS[1], R.ADAM_EPS, c.wd)
        for k, name in enumerate(("p", "m", "v")):
            ratio, al = fp32_check(name, o[k], ref[k], t[k])
            worst[name], alone[name] = max(worst[name], ratio), max(alone[name], al)
        if c.zero_grad and c.step == 1 and c.wd == 0:
            assert torch.equal(o[0], p) and float(o[1].abs().sum()) == 0 and float(o[2].abs().sum()) == 0
    show("adam", R.adam_case_id(c), [(k + "_alone", alone[k]) for k in alone] + [(k + "/bar", worst[k]) for k in worst])
    assert max(worst.values()) <= 1.0, worst

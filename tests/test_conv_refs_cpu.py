"""tests/conv_refs.py checked without a GPU: the float64 references agree with torch's own fp32 convolution, the int family's sums are exact in
fp32 whatever the order, the rand family's inputs keep the reference alone at half of the sweep's share caps, and every case -- packed by the
project's own packers, on the CPU -- plans to the kernel name of its TABLE row."""
import pytest
import torch
import torch.nn.functional as F

import conv_refs as R
from train_refs import bf16r, fp32_flips, worst_over_bar

F64 = torch.float64
CPU_MACS = 3 << 30          # cases above this many multiply-adds are compared with float64 on their first and last map only


def _macs(c):
    f = c.fields
    k2 = f.get("ksize", 3) ** 2
    return f.get("N", 1) * f["H"] * f["W"] // f.get("stride", 1) ** 2 * f["Cout"] * (f["C0"] + f.get("C1", 0)) * k2


def _smallest_of_each_kind():
    """The smallest case of each (layout, epilogue, stride, ksize)."""
    best = {}
    for c in R.RUN_CASES:
        if R.is_gru(c):
            continue
        f = c.fields
        key = (f.get("w_layout", 0), f.get("epilogue", 0), f.get("stride", 1), f.get("ksize", 3), bool(f.get("Cout2")), f.get("in_format", 0))
        if key not in best or _macs(c) < _macs(best[key]):
            best[key] = c
    return sorted(best.values(), key=lambda c: c.row)


def _independent_f32(b):
    """F.conv2d in fp32 on the same operands, written without conv_refs' stage functions: the 9-tap layer on the upsampled, concatenated input.
    (Parity-class layers: the packer's pre-summed weights are what the kernel multiplies, so the 9-tap form with the ORIGINAL weights is no
    reference of it; those cases are compared in the int family, where the class sums are exact -- test_parity_class_sums_are_the_nine_taps.)"""
    h = b.x0
    for i, st in enumerate(b.stages):
        if st.up0:
            h = F.interpolate(h, scale_factor=(2, 2))
        if i == 0 and b.x1 is not None:
            h = torch.cat((h, b.x1), 1)
        y = F.conv2d(h, st.w, None, st.stride, st.pad) * st.scale.view(1, -1, 1, 1) + st.shift.view(1, -1, 1, 1)
        y = F.relu(y) if st.relu else y
        h = bf16r(y)
    return y


@pytest.mark.parametrize("c", [c for c in R.RUN_CASES if not R.is_gru(c) and c.fields.get("w_layout", 0) not in (3, 4) and _macs(c) <= 1 << 29] , ids=R.case_id)
def test_float64_reference_agrees_with_torch_fp32(c):
    """Plain rows: fp32_bar of the case (4 x the error of conv_refs' own fp32 evaluation, floor one ulp).  Chained rows: the independent chain
    rounds its hidden map from fp32, so an element near a tie may differ by a step there -- the chain's own bar (rand_bars' widening) covers it."""
    b = R.build(c.row, "rand")
    ind = _independent_f32(b)[b.maps].to(F64)
    bars = b.bars
    assert ind.shape == b.ref.shape
    ratio = float(((ind - b.ref).abs() / (bars["bar32"] + bars["widen"])).max())
    assert ratio <= 1.0, (R.case_id(c), ratio)


def test_the_smallest_case_of_each_kind_is_in_the_agreement_test():
    ran = {c.row for c in R.RUN_CASES if not R.is_gru(c) and c.fields.get("w_layout", 0) not in (3, 4) and _macs(c) <= 1 << 29}
    assert all(c.row in ran for c in _smallest_of_each_kind() if c.fields.get("w_layout", 0) not in (3, 4))


@pytest.mark.parametrize("lay", [3, 4])
def test_parity_class_sums_are_the_nine_taps(lay):
    """w_layout 3 / 4 on int weights: the class sums are exact in bf16 (|k| <= 28 sixteenths), so the parity-class reference must EQUAL the 9-tap layer
    on the nearest-upsampled input."""
    c = next(c for c in R.RUN_CASES if c.fields.get("w_layout", 0) == lay)
    b = R.build(c.row, "int")
    st = b.stages[0]
    w_up = R.int_weight(c.fields["Cout"], c.fields["C0"] + c.fields["C1"], 3)[:, :c.fields["C0"]]
    x = torch.cat((F.interpolate(b.x0, scale_factor=(2, 2)), b.x1), 1).double()
    nine = F.relu(F.conv2d(x, torch.cat((w_up, st.w), 1).double(), None, 1, 1) * st.scale.double().view(1, -1, 1, 1) + st.shift.double().view(1, -1, 1, 1))
    assert torch.equal(nine, R.layer_ref(b.stages, b.x0, b.x1))


def _fused(what):
    return not isinstance(what, R.ConvCase)


def _wid(what):
    return "%s-%dx%dx%d" % what if _fused(what) else R.case_id(what)


def _first_last(b):
    if b.N > 2:
        b.x0 = b.x0[[0, b.N - 1]]
        b.x1 = None if b.x1 is None else b.x1[[0, b.N - 1]]
    return b


def _int_built(what):
    return R._draw_fused(*what, "int", 0) if _fused(what) else R._draw(what, "int", 0)


INT_THINGS = [c for c in R.RUN_CASES if not R.is_gru(c)] + R.FUSED_CASES


@pytest.mark.parametrize("what", INT_THINGS, ids=_wid)
def test_int_family_is_exact(what):
    b = _int_built(what)
    # the operands are what the family says
    assert set(b.x0.unique().tolist()) <= ({0.0, 1.0} if b.bits is not None else {-1.0, 0.0, 1.0})
    for st in b.stages:
        for w in (st.w,) + ((st.wc,) if st.wc is not None else ()):
            k = w * 16
            assert torch.equal(k, k.round()) and float(k.abs().max()) <= (28 if w is st.wc else 7) and torch.equal(bf16r(w), w)
        assert set(st.scale.tolist()) <= {0.5, 1.0, 2.0} and torch.equal(st.shift * 16, (st.shift * 16).round()) and float(st.shift.abs().max()) <= 2
        w = st.w                          # neighbouring indices differ in every dimension
        assert bool((w[1:] != w[:-1]).all()) and bool((w[:, 1:] != w[:, :-1]).all())
        if w.shape[2] == 3:
            assert bool((w[:, :, 1:] != w[:, :, :-1]).all()) and bool((w[:, :, :, 1:] != w[:, :, :, :-1]).all())
    # exactness: per stage, sum |term| and the epilogue stay below 2^24 quanta, and the issue's own condition sum |term| x 256 < 2^24
    # (over EVERY map; a large case sums in fp32 there and is then compared with float64 on its first and last map)
    large = not _fused(what) and _macs(what) > CPU_MACS
    for i, (acc_q, pre_q, sabs) in enumerate(R.int_exactness(b, torch.float32 if large else F64)):
        cap = 2 ** 23 if large else 2 ** 24          # (fp32 sums: half the bound, see int_exactness)
        assert acc_q < cap and pre_q < cap and sabs * 256 < 2 ** 24, (i, acc_q, pre_q, sabs)
    if large:
        b = _first_last(b)
    ref64 = R.layer_ref(b.stages, b.x0, b.x1, F64)
    ref32 = R.layer_ref(b.stages, b.x0, b.x1, torch.float32)
    assert torch.equal(ref32.to(F64), ref64)                                       # fp32 evaluation == float64, bit for bit
    assert float((ref64 != 0).double().mean()) >= 0.25                             # the answer is not mostly zeros
    # every 32-channel chunk of every source and every tap reaches some output: non-zero activations where the tap reads, non-zero weights
    st = b.stages[0]
    k = st.w.shape[2]
    srcs = [(b.x0, st.wc.abs().sum((0, 1)).t() if st.wc is not None else st.w[:, :b.x0.shape[1]].abs().sum((2, 3)).t())]
    if b.x1 is not None:
        srcs.append((b.x1, (st.w if st.wc is not None else st.w[:, b.x0.shape[1]:]).abs().sum((2, 3)).t()))
    for x, wsum in srcs:
        for c0 in range(0, x.shape[1], 32):
            assert float(x[:, c0:c0 + 32, 1:-1, 1:-1].abs().sum()) > 0 and float(wsum[c0:c0 + 32].sum()) > 0
    taps = st.w.abs().sum((0, 1))
    assert bool((taps > 0).all()) and taps.shape == (k, k)
    if st.wc is not None:
        assert bool((st.wc.abs().sum((2, 3)) > 0).all())


RAND_THINGS = [c for c in R.RUN_CASES if not R.is_gru(c)] + R.FUSED_CASES


@pytest.mark.parametrize("what", RAND_THINGS, ids=_wid)
def test_rand_family_keeps_the_reference_alone_at_half_the_caps(what):
    """torch's own fp32 result, rounded to bf16, differs from bf16r64(ref64) on at most FLIP_MAX / 2 of the elements the sweep counts; at most
    KINK_MAX / 2 are exempted at the ReLU kink; torch's fp32 result is inside the sweep's own bar; a chained case whose output is bf16 keeps half
    of its pixels in the flip count (an fp32 output has no flip count)."""
    b = R.build_fused(*what, "rand") if _fused(what) else R.build(what.row, "rand")
    bars = b.bars
    flips, kink = R.flip_kink_shares(bf16r(bars["ref32"].float()).to(F64), bars)
    print("%s: alone %s flips %.1e kink %.1e kept pixels %.2f draw %d" % (what, ["%.1e" % a for a in bars["alone"]], flips, kink, bars["kept_pixels"], b.attempt))
    assert flips <= R.FLIP_MAX / 2 and kink <= R.KINK_MAX / 2, (flips, kink)
    assert worst_over_bar(bars["ref32"], bars["ref"], bars["bar32"]) <= 0.25 + 1e-12
    if len(b.stages) > 1 and not b.f32:
        assert bars["kept_pixels"] >= 0.5, bars["kept_pixels"]
    elif len(b.stages) == 1:
        assert bars["kept_pixels"] == 1.0 and float(bars["widen"].abs().max()) == 0.0


def test_reference_alone_flip_share_over_the_layer_shapes():
    """The figure the caps rest on: fp32-then-bf16 against float64-then-bf16 over K = 288 ... 6912 (measured 1.2e-4 ... 2.9e-4)."""
    for cin in (32, 128, 768):
        g = torch.Generator().manual_seed(cin)
        x = bf16r(torch.randn(2, cin, 32, 32, generator=g))
        w = bf16r(torch.randn(64, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5)
        y64 = F.conv2d(x.double(), w.double(), None, 1, 1)
        share = fp32_flips(F.conv2d(x, w, None, 1, 1), y64)
        print("K = %d: reference-alone flip share %.1e" % (9 * cin, share))
        assert share <= R.FLIP_MAX / 2


def test_gru_reference_is_the_oracle_cell_in_float64():
    c = next(c for c in R.RUN_CASES if R.is_gru(c) and c.fields.get("w_layout", 0) == 0)
    b = R.build(c.row, "rand")
    x = torch.cat((b.x0, b.x1), 1)
    with torch.no_grad():
        gi = F.conv2d(x.double(), b.cell.weight_ih_l0, b.cell.bias_ih_l0, 1, 1)
        bh = b.cell.bias_hh_l0.view(1, -1, 1, 1)
        (ir, iz, inn), (hr, hz, hn) = gi.chunk(3, 1), bh.chunk(3, 1)
        n = torch.tanh(inn + torch.sigmoid(ir + hr) * hn)
        want = n - torch.sigmoid(iz + hz) * n
    assert b.ref.dtype == F64 and torch.allclose(b.ref, want, rtol=0, atol=1e-14)
    assert torch.equal(bf16r(b.cell.weight_ih_l0.float()).double(), b.cell.weight_ih_l0)


# ------------------------------------------------------------------------------------------------------ the plan name of every case
def plan_name(c, pc):
    """v2x_conv2d_plan of the PACKED layer (w_rows, w_kpad, layout as the packer set them) with placeholder tensors."""
    from v2x_sim_amd import _lib, ops, tuning
    f = c.fields
    d = ops._conv_desc(pc, f.get("N", 1), f["H"], f["W"])
    d.in0, d.in1, d.out = R.PTR, (R.PTR if pc.C1 else None), R.PTR
    for k in ("weight", "scale", "shift") + (("weight2", "scale2", "shift2") if pc.Cout2 else ()):
        setattr(d, k, R.PTR)
    d.in_format, d.in_zbits = f.get("in_format", 0), f.get("in_zbits", 0)
    d.out_cstride = pc.Cout2 or pc.Cout
    d.small_batch = f.get("small_batch", 0)
    if f.get("splitk", 0) > 1:
        d.splitk, d.splitk_ws = f["splitk"], R.PTR
    old = {k: tuning.set(k, v) for k, v in c.switches.items()}
    try:
        return _lib.conv_plan(d)
    finally:
        for k, v in old.items():
            tuning.set(k, v)


@pytest.mark.parametrize("c", R.RUN_CASES, ids=R.case_id)
def test_every_case_plans_to_its_rows_name(c):
    b = R._draw(c, "int" if not R.is_gru(c) else "rand", 0)
    pc = b.pack("cpu")
    assert plan_name(c, pc) == c.name
    d = R.desc(**c.fields)                    # and the packer's geometry is the table's
    assert (pc.w_rows, pc.w_kpad, pc.w_layout or 0) == (d.w_rows, d.w_kpad, d.w_layout) or c.note


def test_the_sweep_runs_every_name_of_the_table_but_not_run():
    table = {name for name, _, _ in R.TABLE}
    ran = {c.name for c in R.RUN_CASES}
    assert ran | set(R.NOT_RUN) == table and not (ran & set(R.NOT_RUN))
    assert len(R.CONV_CASES) == len(R.TABLE) and [c.row for c in R.CONV_CASES] == list(range(len(R.TABLE)))
    others = [n for n in R.NOT_RUN if not n.endswith(", 3>")]
    assert len(others) <= 3 and len(R.NOT_RUN) <= 4
    for c in R.CONV_CASES:
        if c.same_as is not None:
            twin = R.CONV_CASES[c.same_as]
            assert (twin.name, twin.switches, twin.fields) == (c.name, c.switches, c.fields) and twin in R.RUN_CASES and c.note
        elif not c.note:
            assert (c.name, c.switches, c.fields) == R.TABLE[c.row]

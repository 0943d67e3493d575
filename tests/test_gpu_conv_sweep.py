"""Every dispatch form of the inference convolutions against float64 (tests/conv_refs.py), with exact-integer cases.

One test per row of the plan table (tests/conv_refs.py::TABLE, the table tests/test_conv_plan_cpu.py names) and input family, plus the two fused
launches (ops.conv2d_pair on the bit grid, ops.conv2d_tail).  Each case
  * sets the row's switches, packs the layer with the project's own packer and asserts that the library names the row's kernel -- before the
    launch (ops.conv_kernel_name) and for the descriptor actually launched (the instrumented launch's record, which also covers split-K);
  * gives every input as the inner maps of a buffer whose first and last map are NaN (all-ones words for the bit grid) and the output as the
    inner maps of a buffer filled with a sentinel: afterwards the outer output maps still hold the sentinel and no output element is NaN -- a halo
    read or a store that leaves its own map without leaving the allocation shows, and nothing faults (ops.conv2d_tail allocates its own outputs:
    its inputs are guarded, its outputs are not);
  * launches twice and demands identical bits;
  * int family: torch.equal with the exact answer (fp32 outputs) or with the exact answer rounded once to bf16.  No tolerance, no flips;
  * rand family: fp32 outputs within fp32_bar (4 x the error of torch's own fp32 evaluation of the case, floor one ulp); bf16 outputs within
    half a bf16 step of the float64 reference + that bar, at most FLIP_MAX = 1e-3 of the elements rounded differently from float64 and at most
    KINK_MAX = 1e-4 exempted at the ReLU kink; chained layers with the widening and the flip population of conv_refs.rand_bars; GRU rows with
    the expression of test_gpu_stream.py::test_gru_gate_arithmetic_over_its_whole_range against the oracle cell in float64 (the v_exp_f32 /
    v_rcp_f32 gates dominate there; this sweep does not tighten them).
Every test prints worst error / bar and the flip share (-s shows them).

Measured on one MI355X run (156 tests, module wall time 8.3 s, the float64 references included; slowest case 2.1 s: row 17's 32 896 output
channels).  Every int case -- 72 table rows and the four fused launches, 42 M output elements -- equals its exact answer bit for bit: the MFMA paths,
split-K with its reduce kernel, the chained 1x1 and both fused launches reproduce exact sums whatever their order of accumulation, and round a
bf16 output to nearest-even exactly once.  Per kernel family (worst over its cases): `alone` = the reference-alone fp32 error; `fp32 used` = the
share of the 4 x alone allowance a bf16 output uses beyond its half step; `err/plain` = worst error / the bar WITHOUT the chained layers'
widening (above 1 only on chained forms, where a hidden value legitimately rounds the other way; with the widening every case is <= 1.0);
flips (cap 1e-3) and kink exemptions (cap 1e-4); `gru/bar` = the GRU rows against their looser expression:
  family                       int/rand  int elements alone      fp32 used  err/plain  flips     kink      gru/bar 
  conv3x3_stream8q_kernel        1 / 1          65500 9.9e-07    0.041      1          7.6e-05   0.0e+00   -       
  conv3x3_stream8p_kernel        1 / 1          65500 1e-06      0.12       1          1.5e-04   0.0e+00   -       
  conv3x3_stream_kernel         13 / 17       3308100 2.2e-06    0.13       3.5e+02    3.0e-04   3.0e-05   0.17    
  conv3x3_stream8g_kernel        2 / 4         851500 1.7e-06    0.12       1          3.7e-04   8.9e-06   0.17    
  conv3x3_stream8_kernel         3 / 4       29465500 1.8e-06    0.057      54         3.2e-04   6.8e-06   0.17    
  conv3x3_wide3_kernel           1 / 1         131000 1.4e-06    0.029      1          3.8e-05   1.5e-05   -       
  conv3x3_wide_kernel            3 / 3         229300 1.4e-06    0.22       1          1.2e-04   1.5e-05   -       
  conv3x3_s2_stream_kernel      10 / 10       4624070 1.7e-06    0.07       1          1.8e-04   1.0e-05   -       
  conv3x3_s2g_kernel             2 / 2         524000 1.6e-06    0.1        1          8.0e-05   3.8e-06   -       
  conv3x3_s2_resident_kernel     1 / 1          49200 1e-06      0.0024     1          4.1e-05   0.0e+00   -       
  conv3x3_halo_sb_kernel         2 / 2          16380 8.8e-07    0.02       1          1.2e-04   0.0e+00   -       
  conv3x3_halo_ppc_kernel        1 / 1          73700 8e-07      0.0074     1          2.7e-05   1.4e-05   -       
  conv3x3_halo_pp_kernel         3 / 3         246200 1.1e-06    0.036      15         6.1e-05   0.0e+00   -       
  conv3x3_halo_kernel            8 / 8        1013040 1.3e-06    0.055      82         3.7e-04   4.1e-06   -       
  conv1x1_stream_kernel          9 / 9          37116 9.6e-07    0.027      1          3.7e-04   0.0e+00   -       
  conv_igemm_kernel             10 / 11         50068 1e-06      0.013      1          6.1e-05   0.0e+00   0.16    
  conv3x3_pair_bits_kernel       2 / 2         254190 5.3e-07    0.014      27         1.3e-05   4.1e-06   -       
  conv3x3_tail_kernel            2 / 2         381300 1.2e-06    -          2.6e+03    -         -         -       
Mutation check (scratch builds, not part of the tree): with the (ky 2, kx 1) tap of the last 32-channel chunk zeroed at column 31 of every tile in
conv3x3_halo_body, all ten conv3x3_halo_kernel / conv3x3_halo_sb_kernel rows fail in both families (int: 45 of 8 192 elements on row 45, all at
x = 31, odd rows) and no other row does; with one of the last tap's MFMAs left out of conv3x3_halo_pp_kernel, exactly its three rows fail."""
import pytest
import torch

import conv_refs as R
from train_refs import bf16r64, worst_over_bar

pytestmark = pytest.mark.gpu
F64 = torch.float64
SENTINEL = -768.0            # exact in bf16 and fp32; no case produces it over a whole map


def _nhwc(x, device):
    return x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(device)


def _guarded(inner, fill):
    """inner (N, ...) on the device -> the same values as maps [1 : N + 1] of a buffer of N + 2 maps whose outer two hold `fill`."""
    buf = torch.full((inner.shape[0] + 2,) + tuple(inner.shape[1:]), fill, dtype=inner.dtype, device=inner.device)
    buf[1:-1] = inner
    return buf


def _inputs(b, device):
    """-> (in0, in1, the buffers that own them)."""
    if b.bits is not None:
        g0 = _guarded(b.bits.to(device), -1)
    else:
        g0 = _guarded(_nhwc(b.x0, device), float("nan"))
    g1 = _guarded(_nhwc(b.x1, device), float("nan")) if b.x1 is not None else None
    return g0[1:-1], (g1[1:-1] if g1 is not None else None), (g0, g1)


def _check_guards(outbuf):
    assert bool((outbuf[0] == SENTINEL).all()) and bool((outbuf[-1] == SENTINEL).all()), "a store left its own map"
    assert not bool(torch.isnan(outbuf[1:-1].float()).any()), "a read left its own map (NaN guard) or the kernel produced NaN"
    assert not bool((outbuf[1:-1] == SENTINEL).all(dim=-1).any()), "a pixel was never written"


def _nchw64(y):
    return y.to(F64).cpu().permute(0, 3, 1, 2).contiguous()


def _launch_row(ops, c, b, pc, device):
    """The row's launch into a guarded output; -> (output NCHW float64, the kernel name(s) the library recorded for the launched descriptor)."""
    in0, in1, _keep = _inputs(b, device)
    f = c.fields
    Ho, Wo = ops.conv_out_hw(pc, b.H, b.W)
    odt = torch.float32 if b.f32 else torch.bfloat16
    outs = []
    for _ in range(2):
        outbuf = torch.full((b.N + 2, Ho, Wo, pc.Cout2 or pc.Cout), SENTINEL, dtype=odt, device=device)
        ops.PROFILE = []
        try:
            with R.latency(b):
                ops.conv2d(pc, in0, in1, out=outbuf[1:-1], zbits=f.get("in_zbits", 0), splitk=b.splitk)
            torch.cuda.synchronize()
            names = [r[0] for r in ops.PROFILE]
        finally:
            ops.PROFILE = None
        _check_guards(outbuf)
        outs.append(outbuf[1:-1])
    assert torch.equal(outs[0].view(torch.int32 if b.f32 else torch.int16), outs[1].view(torch.int32 if b.f32 else torch.int16)), "two launches differ"
    return _nchw64(outs[0]), names


def _show(what, family, figs):
    print("\nconv-sweep %-62s %-4s " % (what, family) + "  ".join("%s %.3g" % kv for kv in figs))


def _steps_off(got, want_b):
    """Worst difference in bf16 steps of the expected value (reporting of an int mismatch)."""
    step = torch.maximum(R.bf16_step(want_b), R.bf16_step(got))          # (an expected 0 has no step of its own: the step of what came back)
    d = (got - want_b).abs()
    return float(torch.where(step > 0, d / torch.where(step > 0, step, torch.ones_like(step)), torch.zeros_like(d)).max())


def _hold_int(what, b, got):
    want = R.int_ref(b)
    assert got.shape == want.shape
    if not b.f32:
        want = bf16r64(want)
    bad = got != want
    n_bad = int(bad.sum())
    _show(what, "int", [("mismatches", n_bad), ("of", got.numel()), ("nonzero", float((want != 0).double().mean()))])
    if n_bad:
        idx = bad.nonzero()
        where = ["(n %d, c %d, y %d, x %d): got %r want %r" % (*i.tolist(), float(got[tuple(i)]), float(want[tuple(i)])) for i in idx[:8]]
        chans = sorted(set(idx[:, 1].tolist()))
        raise AssertionError("%s: %d of %d elements differ from the exact answer, worst by %.3g bf16 steps; channels %s%s; rows %d..%d, columns %d..%d; first: %s"
                             % (what, n_bad, got.numel(), _steps_off(got, want), chans[:16], "..." if len(chans) > 16 else "",
                                int(idx[:, 2].min()), int(idx[:, 2].max()), int(idx[:, 3].min()), int(idx[:, 3].max()), "; ".join(where)))


def _hold_rand(what, b, got_all):
    got = got_all[b.maps]
    assert got.shape == b.ref.shape
    if b.cell is not None:
        ratio = float(((got - b.ref).abs() / R.gru_bar(b.ref)).max())
        _show(what, "rand", [("gru err/bar", ratio), ("flips", float((got != bf16r64(b.ref)).double().mean()))])
        assert ratio <= 1.0, (what, ratio)
        return
    bars = b.bars
    if b.f32:
        ratio = float(((got - bars["ref"]).abs() / (bars["bar32"] + bars["widen"])).max())
        _show(what, "rand", [("err/bar", ratio), ("unwidened", worst_over_bar(got, bars["ref"], bars["bar32"])), ("alone", max(bars["alone"]))])
        assert ratio <= 1.0, (what, ratio)
        return
    err, bar = (got - bars["ref"]).abs(), R.bf16_bar(bars)
    ratio = float((err / bar).max())
    flips, kink = R.flip_kink_shares(got, bars)
    plain = bars["bar32"] + R.bf16_step(bars["ref"]) / 2           # the bar without the chained layers' widening, printed beside it
    _show(what, "rand", [("err/bar", ratio), ("unwidened", float((err / plain).max())), ("fp32 part used", R.bf16_excess(got, bars)), ("flips", flips), ("kink", kink),
                         ("alone", max(bars["alone"])), ("kept", bars["kept_pixels"])])
    assert ratio <= 1.0 and flips <= R.FLIP_MAX and kink <= R.KINK_MAX, (what, ratio, flips, kink)


@pytest.mark.parametrize("c,family", [(c, fam) for c in R.RUN_CASES for fam in R.families(c)], ids=lambda v: v if isinstance(v, str) else R.case_id(v))
def test_conv_form(device, tune, c, family):
    from v2x_sim_amd import ops
    for k, v in c.switches.items():
        tune(k, v)
    b = R.build(c.row, family)
    pc = b.pack(device)
    if not b.splitk:                       # (ops.conv_kernel_name has no split-K argument: those rows are named by the launch record alone)
        with R.latency(b):
            assert ops.conv_kernel_name(pc, b.H, b.W, b.bits is not None, b.N) == c.name
    got, names = _launch_row(ops, c, b, pc, device)
    assert names == [c.name], (names, c.name)
    (_hold_int if family == "int" else _hold_rand)(R.case_id(c), b, got)


@pytest.mark.parametrize("family", ["int", "rand"])
@pytest.mark.parametrize("kind,N,Hh,Ww", R.FUSED_CASES)
def test_fused_launch(device, kind, N, Hh, Ww, family):
    """ops.conv2d_pair (conv_halo_pair.hip: two 3x3 32 -> 32 layers on the bit grid) and ops.conv2d_tail (conv_tail.hip: conv8_2 + the chained
    heads) against the exact answer and against float64, the hidden maps rounded once to bf16."""
    from v2x_sim_amd import ops
    b = R.build_fused(kind, N, Hh, Ww, family)
    pa, pb = b.pack(device)
    in0, _, _keep = _inputs(b, device)
    outs = []
    for _ in range(2):
        if kind == "pair":
            assert ops.pair_eligible(pa, pb, in0, R.ZBITS)
            outbuf = torch.full((N + 2, Hh, Ww, 32), SENTINEL, dtype=torch.bfloat16, device=device)
            ops.conv2d_pair(pa, pb, in0, R.ZBITS, out=outbuf[1:-1])
            torch.cuda.synchronize()
            _check_guards(outbuf)
            outs.append(outbuf[1:-1])
        else:
            assert ops.tail_eligible(pa, pb, in0, R.TAIL_SPLIT)
            cls, loc = ops.conv2d_tail(pa, pb, in0, R.TAIL_SPLIT)
            torch.cuda.synchronize()
            outs.append(torch.cat((cls, loc), 3))
            assert not bool(torch.isnan(outs[-1]).any())
    assert torch.equal(outs[0].view(torch.int32 if b.f32 else torch.int16), outs[1].view(torch.int32 if b.f32 else torch.int16)), "two launches differ"
    (_hold_int if family == "int" else _hold_rand)("%s-%dx%dx%d" % (kind, N, Hh, Ww), b, _nchw64(outs[0]))

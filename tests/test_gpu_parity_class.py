"""Parity-class form of the decoder's upsample -> concat -> 3x3 layers (conv_halo.hip: conv3x3_halo_ppc_kernel, w_layout 3; row a6).

Two kinds of test, kept apart on purpose (guardrails):
  * PARITY tests compare the kernel with the UNMODIFIED fp32 oracle layer (oracle/coperception_ref.py::cbr on
    cat(F.interpolate(x_up), x_skip) -- 9 taps on the nearest-upsampled operand, fp32 weights).  The tolerance is the bf16 rounding of the
    weights and of the output, the same bound the 9-tap kernel is held to in the same test (tools/parity_class_study.py: rms error 2.2-2.4e-3
    of the rms output for either form).
  * KERNEL tests compare it with a torch fp32 evaluation of the SAME bf16 operands -- the pre-summed, once-rounded 2x2-tap weights -- to one
    bf16 ulp of the output; they check the kernel's arithmetic, not the parity with the reference."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import coperception_ref as R

pytestmark = pytest.mark.gpu


def bf16r(x):
    return x.to(torch.bfloat16).to(torch.float32)


def to_nhwc_bf16(x_nchw, dev):
    return x_nchw.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(dev)


def from_nhwc(y):
    return y.float().cpu().permute(0, 3, 1, 2).contiguous()


def _layer(C0, C1, Cout, seed):
    """an oracle conv + BN pair with the statistics of a trained layer (He-scaled weights, non-trivial BN)"""
    g = torch.Generator().manual_seed(seed)
    conv = nn.Conv2d(C0 + C1, Cout, 3, 1, 1)
    bn = nn.BatchNorm2d(Cout).eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / ((C0 + C1) * 9)) ** 0.5)
        conv.bias.copy_(torch.randn(Cout, generator=g) * 0.1)
        bn.weight.copy_(torch.rand(Cout, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(Cout, generator=g) * 0.1)
        bn.running_mean.copy_(torch.randn(Cout, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(Cout, generator=g) + 0.5)
    return conv, bn


def _inputs(N, C0, C1, H, W, seed):
    g = torch.Generator().manual_seed(seed + 1)
    x_up = bf16r(F.relu(torch.randn(N, C0, H // 2, W // 2, generator=g)))    # post-ReLU maps, as in the network
    x_sk = bf16r(F.relu(torch.randn(N, C1, H, W, generator=g)))
    return x_up, x_sk


def _oracle_fp32(conv, bn, x_up, x_sk):
    """the unmodified reference layer: F.relu(bn(conv(cat(up(x), skip)))) in fp32 (LidarDecoder.forward, emulate=False)"""
    with torch.no_grad():
        return R.cbr(torch.cat((F.interpolate(x_up, scale_factor=(2, 2)), x_sk), dim=1), conv, bn, emulate=False)


def _same_operands_ref(packing, conv, bn, x_up, x_sk, C0):
    """torch fp32 evaluation of what the kernel multiplies: bf16 pre-summed class weights on the half-resolution map + bf16 3x3 weights on the
    skip map, fp32 sums, folded BN, ReLU (no output rounding)."""
    with torch.no_grad():
        w = conv.weight.detach().float()
        scale, shift = packing.fold_bn(conv.bias, bn, conv.out_channels)
        wc = bf16r(packing.parity_class_weights(w[:, :C0]))                 # [4][4][Cout][C0]
        y = F.conv2d(x_sk, bf16r(w[:, C0:]), None, 1, 1)
        N, _, hs, ws = x_up.shape
        xp = F.pad(x_up, (1, 1, 1, 1))
        for py in range(2):
            for px in range(2):
                k = wc[py * 2 + px].view(2, 2, conv.out_channels, C0).permute(2, 3, 0, 1).contiguous()   # [Cout][C0][a][b]
                full = F.conv2d(xp, k)                                     # (hs + 1) x (ws + 1) positions
                y[:, :, py::2, px::2] += full[:, :, py:py + hs, px:px + ws]
        return F.relu(y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))


def _run(ops, pc, x_up, x_sk, device):
    return ops.conv2d(pc, to_nhwc_bf16(x_up, device), to_nhwc_bf16(x_sk, device))


CASES = [(2, 16, 32), (3, 64, 96), (1, 8, 32), (3, 24, 32), (5, 256, 256)]   # one pair; ragged walk; a single tile (group 1 idle); odd tile count; full size


@pytest.mark.parametrize("N,H,W", CASES)
def test_parity_class_kernel_against_the_same_bf16_operands(device, N, H, W):
    """KERNEL test: one bf16 ulp of the output against torch on the pre-summed bf16 weights (image borders, odd tile counts, full size)."""
    from v2x_sim_amd import ops, packing
    conv, bn = _layer(64, 32, 32, seed=N * 100 + H)
    x_up, x_sk = _inputs(N, 64, 32, H, W, seed=H + W)
    scale, shift = packing.fold_bn(conv.bias, bn, 32)
    pc = packing.pack_conv_halo_parity("conv8_1", conv.weight, scale, shift, C0=64, C1=32, device=device)
    assert ops.conv_kernel_name(pc, H, W, False, N) == "conv3x3_halo_ppc_kernel<64, 32, 32>"
    got = from_nhwc(_run(ops, pc, x_up, x_sk, device))
    ref = _same_operands_ref(packing, conv, bn, x_up, x_sk, 64)
    assert got.shape == ref.shape
    assert torch.allclose(got, ref, atol=2e-3, rtol=2 ** -7), float((got - ref).abs().max())


@pytest.mark.parametrize("N,H,W", [(3, 64, 96), (5, 256, 256)])
def test_parity_class_layer_against_the_unmodified_fp32_oracle(device, N, H, W, tune):
    """PARITY test: the kernel against the oracle's fp32 layer (9 taps on the nearest-upsampled operand, fp32 weights, no rounding anywhere).
    Tolerance = bf16 rounding of weights and output: rms error <= 4e-3 of the rms output, max error <= 3e-2 max|ref| -- and the 9-tap kernel
    (V2X_PARITY_CLASS = 0 packing) is held to the SAME bounds on the same data: the pre-summed form is not allowed to be a worse restatement."""
    from v2x_sim_amd import ops, packing
    conv, bn = _layer(64, 32, 32, seed=7 + H)
    x_up, x_sk = _inputs(N, 64, 32, H, W, seed=11 + W)
    ref = _oracle_fp32(conv, bn, x_up, x_sk)
    scale, shift = packing.fold_bn(conv.bias, bn, 32)
    forms = {
        "parity-class": packing.pack_conv_halo_parity("conv8_1", conv.weight, scale, shift, C0=64, C1=32, device=device),
        "9-tap": packing.pack_conv_halo("conv8_1", conv.weight, scale, shift, C0=64, C1=32, device=device),
    }
    err = {}
    for name, pc in forms.items():
        got = from_nhwc(_run(ops, pc, x_up, x_sk, device))
        d = got - ref
        err[name] = (float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()), float(d.abs().max() / ref.abs().max()))
        assert err[name][0] <= 4e-3 and err[name][1] <= 3e-2, (name, err[name])
    # neither form is systematically closer to the reference: their rms errors agree to 25 %
    assert abs(err["parity-class"][0] - err["9-tap"][0]) <= 0.25 * err["9-tap"][0], err


def test_parity_class_packing_is_selected_by_shape_and_switch(device, tune):
    """layer_conv_bn packs conv8_1's shape (cat(up(64), 32) -> 32) for the parity-class kernel by default and for the 9-tap halo kernel with
    PARITY_CLASS = 0; other decoder shapes keep their kernels."""
    from v2x_sim_amd import packing
    conv, bn = _layer(64, 32, 32, seed=3)
    lay = packing.layer_conv_bn("conv8_1", conv, bn, device=device, C0=64, C1=32, up0=1)
    assert lay.halo.w_layout == 3 and lay.halo.w_kpad == 16 * 64 + 9 * 32
    tune("PARITY_CLASS", 0)
    lay = packing.layer_conv_bn("conv8_1", conv, bn, device=device, C0=64, C1=32, up0=1)
    assert lay.halo.w_layout == 1
    tune.reset("PARITY_CLASS")
    conv7, bn7 = _layer(128, 64, 64, seed=4)   # conv7_1's shape: the two-tiles-per-workgroup streamed kernel at PARITY_CLASS = 3 (default)
    lay = packing.layer_conv_bn("conv7_1", conv7, bn7, device=device, C0=128, C1=64, up0=1)
    assert lay.halo.w_layout == 4 and lay.halo.w_rows == 64 and lay.latency is not None and lay.latency.w_layout == 2
    tune("PARITY_CLASS", 2)
    assert packing.layer_conv_bn("conv7_1", conv7, bn7, device=device, C0=128, C1=64, up0=1).halo.w_layout == 2
    # conv6_1's shape: the streamed parity-class kernel at PARITY_CLASS >= 2, with a 9-tap streamed packing for declared latency launches
    conv6, bn6 = _layer(256, 128, 128, seed=5)
    lay = packing.layer_conv_bn("conv6_1", conv6, bn6, device=device, C0=256, C1=128, up0=1)
    assert lay.halo.w_layout == 4 and lay.latency is not None and lay.latency.w_layout == 2
    tune("PARITY_CLASS", 1)
    lay = packing.layer_conv_bn("conv6_1", conv6, bn6, device=device, C0=256, C1=128, up0=1)
    assert lay.halo.w_layout == 2 and lay.latency is None


def test_parity_class_store_forms_walks_and_repeats_are_bit_identical(device, tune):
    """16-byte and 8-byte store forms, the XCD-contiguous and the round-robin tile walk, and repeated launches give the same bits (no race
    between the two wave groups' phases; ragged persistent walk: 3 x 64 x 96 = 72 tiles on up to 36 workgroups)."""
    from v2x_sim_amd import ops, packing
    conv, bn = _layer(64, 32, 32, seed=21)
    x_up, x_sk = _inputs(40, 64, 32, 128, 128, seed=5)                  # 2 560 tiles: 5 pairs per workgroup
    scale, shift = packing.fold_bn(conv.bias, bn, 32)
    pc = packing.pack_conv_halo_parity("conv8_1", conv.weight, scale, shift, C0=64, C1=32, device=device)
    xu, xs = to_nhwc_bf16(x_up, device), to_nhwc_bf16(x_sk, device)
    base = ops.conv2d(pc, xu, xs).clone()
    for _ in range(3):
        assert torch.equal(base.view(torch.int16), ops.conv2d(pc, xu, xs).view(torch.int16))
    for name in ("STORE_X4", "HALO_XCD"):
        tune(name, 0)
        assert torch.equal(base.view(torch.int16), ops.conv2d(pc, xu, xs).view(torch.int16)), name
        tune.reset(name)
    # a view with a channel offset that is not 16-byte aligned takes the 8-byte stores by itself
    out = torch.zeros((40, 128, 128, 36), dtype=torch.bfloat16, device=device)
    ops.conv2d(pc, xu, xs, out=out, out_coff=4)
    assert torch.equal(out[..., 4:].contiguous().view(torch.int16), base.view(torch.int16)) and float(out[..., :4].abs().max()) == 0.0


def test_parity_class_transpose_detecting(device):
    """Asymmetric check: a single hot half-resolution pixel / channel and a single hot skip pixel -> every output pixel they reach carries
    exactly the (pre-summed, bf16) weight the class decomposition assigns, at the right place."""
    from v2x_sim_amd import ops, packing
    C0, C1, Cout, H, W = 64, 32, 32, 16, 32
    w = (torch.arange(Cout * (C0 + C1) * 9, dtype=torch.float32).view(Cout, C0 + C1, 3, 3) % 61) / 16.0
    x_up = torch.zeros(1, C0, H // 2, W // 2)
    x_up[0, 5, 3, 7] = 1.0
    x_sk = torch.zeros(1, C1, H, W)
    x_sk[0, 9, 12, 30] = 2.0
    pc = packing.pack_conv_halo_parity("t", w, torch.ones(Cout), torch.zeros(Cout), C0=C0, C1=C1, relu=False, device=device)
    got = from_nhwc(_run(ops, pc, x_up, x_sk, device))
    # reference: the 9-tap layer with every product exact (integers / 16) -- the sums of up to four taps are exact in bf16 here (< 2^8 steps of 1/16)
    ref = F.conv2d(torch.cat((F.interpolate(x_up, scale_factor=(2, 2)), x_sk), 1), w, None, 1, 1)
    assert torch.equal(got, bf16r(ref)), float((got - ref).abs().max())
    assert np.count_nonzero(got.numpy()) > 0


# ---- the streamed parity-class kernel (conv_stream_pc.hip: conv5_1, conv6_1; w_layout 4) ----------------------------------------------------
STREAMED = [  # (C0, C1, Cout, N, H, W)
    (512, 256, 256, 2, 32, 32),     # conv5_1: whole maps = two tiles x two channel tiles
    (256, 128, 128, 2, 64, 64),     # conv6_1
    (256, 128, 128, 1, 16, 32),     # a single tile: every border is zero padding
    (64, 32, 128, 3, 48, 96),       # short K (two up chunks, one skip chunk), ragged persistent walk
    (512, 256, 256, 40, 32, 32),    # 160 tiles on <= 256 workgroups ... and
    (256, 128, 128, 80, 64, 64),    # 640 tiles: 2.5 tiles per workgroup (the persistent loop, the next tile's prologue under the stores)
    (128, 64, 64, 2, 128, 128),     # conv7_1: the two-tiles-per-workgroup kernel (conv3x3_stream8q_kernel)
    (128, 64, 64, 1, 16, 64),       # ... a single region: every border is zero padding
    (32, 32, 64, 3, 48, 192),       # ... one up chunk, one skip chunk; ragged walk
    (128, 64, 64, 40, 128, 128),    # ... 640 regions: 2.5 per workgroup
]
STREAMED_ORACLE = STREAMED[:2] + STREAMED[6:7]


@pytest.mark.parametrize("C0,C1,Cout,N,H,W", STREAMED)
def test_streamed_parity_class_kernel_against_the_same_bf16_operands(device, C0, C1, Cout, N, H, W):
    """KERNEL test of conv3x3_stream8p_kernel: one bf16 ulp of the output against torch on the pre-summed bf16 weights; repeated launches are
    bit-identical (no race between the wave groups, the phases and the tiles of the persistent loop)."""
    from v2x_sim_amd import ops, packing
    conv, bn = _layer(C0, C1, Cout, seed=C0 + N)
    x_up, x_sk = _inputs(N, C0, C1, H, W, seed=H + W + N)
    scale, shift = packing.fold_bn(conv.bias, bn, Cout)
    pc = packing.pack_conv_stream_parity("conv5_1", conv.weight, scale, shift, C0=C0, C1=C1, device=device)
    assert ops.conv_kernel_name(pc, H, W, False, N) == ("conv3x3_stream8q_kernel" if Cout == 64 else "conv3x3_stream8p_kernel") and pc.w_kpad == 16 * C0 + 9 * C1
    xu, xs = to_nhwc_bf16(x_up, device), to_nhwc_bf16(x_sk, device)
    y = ops.conv2d(pc, xu, xs)
    again = [ops.conv2d(pc, xu, xs) for _ in range(2)]
    assert all(torch.equal(y.view(torch.int16), z.view(torch.int16)) for z in again)
    if N <= 3:
        ref = _same_operands_ref(packing, conv, bn, x_up, x_sk, C0)
        got = from_nhwc(y)
        assert got.shape == ref.shape
        assert torch.allclose(got, ref, atol=2e-3, rtol=2 ** -7), float((got - ref).abs().max())
    else:   # many maps: every map against the first occurrence of the same input (the inputs repeat with period 2)
        xu2, xs2 = xu.clone(), xs.clone()
        xu2[2:] = xu[:2].repeat((N - 2) // 2, 1, 1, 1)
        xs2[2:] = xs[:2].repeat((N - 2) // 2, 1, 1, 1)
        y2 = ops.conv2d(pc, xu2, xs2)
        assert torch.equal(y2[2:].view(torch.int16), y2[:2].repeat((N - 2) // 2, 1, 1, 1).view(torch.int16))   # a map's bits do not depend on its place in the walk
        assert torch.equal(y2[:2].view(torch.int16), y[:2].view(torch.int16))


@pytest.mark.parametrize("C0,C1,Cout,N,H,W", STREAMED_ORACLE)
def test_streamed_parity_class_layer_against_the_unmodified_fp32_oracle(device, C0, C1, Cout, N, H, W):
    """PARITY test (same bounds as conv8_1's above): the streamed parity-class kernel and the 9-tap streamed kernel against the oracle's fp32
    9-tap layer on the nearest-upsampled operand."""
    from v2x_sim_amd import ops, packing
    conv, bn = _layer(C0, C1, Cout, seed=5 + H)
    x_up, x_sk = _inputs(N, C0, C1, H, W, seed=9 + W)
    ref = _oracle_fp32(conv, bn, x_up, x_sk)
    scale, shift = packing.fold_bn(conv.bias, bn, Cout)
    forms = {"parity-class": packing.pack_conv_stream_parity("l", conv.weight, scale, shift, C0=C0, C1=C1, device=device),
             "9-tap": packing.pack_conv_stream("l", conv.weight, scale, shift, C0=C0, C1=C1, up0=1, device=device)}
    err = {}
    for name, pc in forms.items():
        got = from_nhwc(_run(ops, pc, x_up, x_sk, device))
        d = got - ref
        err[name] = (float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()), float(d.abs().max() / ref.abs().max()))
        assert err[name][0] <= 4e-3 and err[name][1] <= 3e-2, (name, err[name])
    assert abs(err["parity-class"][0] - err["9-tap"][0]) <= 0.25 * err["9-tap"][0], err


# ---- seeded random-shape sweeps (every eligible combination the dispatch accepts, not only the network's shapes) ---------------------------------------
def _sweep_cases(seed, n):
    rng = np.random.default_rng(seed)
    cases = []
    while len(cases) < n:
        kind = int(rng.integers(0, 3))
        if kind == 0:      # resident parity-class kernel: the one compiled shape, any extent
            C0, C1, Cout = 64, 32, 32
            H, W = 8 * int(rng.integers(1, 7)), 32 * int(rng.integers(1, 4))
        elif kind == 1:    # streamed, 128-row tiles
            C0, C1, Cout = 32 * int(rng.integers(1, 5)), 32 * int(rng.integers(1, 4)), 128 * int(rng.integers(1, 3))
            H, W = 16 * int(rng.integers(1, 4)), 32 * int(rng.integers(1, 3))
        else:              # streamed, 64 rows: two tiles per workgroup
            C0, C1, Cout = 32 * int(rng.integers(1, 5)), 32 * int(rng.integers(1, 3)), 64
            H, W = 16 * int(rng.integers(1, 4)), 64 * int(rng.integers(1, 3))
        cases.append((C0, C1, Cout, int(rng.integers(1, 4)), H, W))
    return cases


@pytest.mark.parametrize("C0,C1,Cout,N,H,W", _sweep_cases(2025, 18))
def test_parity_class_kernels_random_shapes(device, C0, C1, Cout, N, H, W):
    """One bf16 ulp against torch on the same pre-summed operands, for shapes drawn at random from what the dispatch accepts (channel counts, tile
    counts, odd numbers of tiles, extents of a single tile); and the layer stays inside the fp32 oracle's bounds."""
    from v2x_sim_amd import ops, packing
    conv, bn = _layer(C0, C1, Cout, seed=C0 + 3 * C1 + Cout + N)
    x_up, x_sk = _inputs(N, C0, C1, H, W, seed=H * 7 + W + N)
    scale, shift = packing.fold_bn(conv.bias, bn, Cout)
    if (C0, C1, Cout) == (64, 32, 32):
        pc = packing.pack_conv_halo_parity("sweep", conv.weight, scale, shift, C0=C0, C1=C1, device=device)
    else:
        pc = packing.pack_conv_stream_parity("sweep", conv.weight, scale, shift, C0=C0, C1=C1, device=device)
    assert pc.w_layout in (3, 4) and ops.covers(pc, H, W)
    got = from_nhwc(_run(ops, pc, x_up, x_sk, device))
    ref = _same_operands_ref(packing, conv, bn, x_up, x_sk, C0)
    assert got.shape == ref.shape
    assert torch.allclose(got, ref, atol=2e-3, rtol=2 ** -7), float((got - ref).abs().max())
    orc = _oracle_fp32(conv, bn, x_up, x_sk)
    d = got - orc
    assert float(d.pow(2).mean().sqrt() / orc.pow(2).mean().sqrt()) <= 4e-3 and float(d.abs().max() / orc.abs().max()) <= 3e-2

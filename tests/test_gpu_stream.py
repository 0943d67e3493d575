"""GPU parity of the streamed-weights halo kernel (conv_stream.hip, w_layout 2) against torch-CPU on the
same bf16 operands, and against the gather kernel.  Tolerance: bf16 output = one rounding (rel 2^-7)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import coperception_ref as R

pytestmark = pytest.mark.gpu


def bf16r(x):
    return x.to(torch.bfloat16).to(torch.float32)


def nhwc(x, dev):
    return x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(dev)


def back(y):
    return y.float().cpu().permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("cfg", [
    # (C_up, C, Cout, N, H, W)
    (0, 128, 128, 2, 16, 32),     # conv2_2 / conv6_2 class, 8x32 tiles, 128-row channel tile
    (0, 256, 256, 1, 32, 32),     # conv3_2 class: two channel tiles, 4 pixel tiles
    (0, 512, 512, 2, 16, 16),     # conv4_2 class: 16x16 tiles (W = 16)
    (256, 128, 128, 1, 16, 64),   # conv6_1: x2-upsampled source + skip
    (128, 64, 64, 2, 8, 32),      # conv7_1: 64-row channel tile (1 weight DMA per wave)
    (512, 256, 256, 1, 16, 16),   # conv5_1 on a 16x16 map: upsampled source with 16x16 tiles
])
def test_stream_conv_vs_torch(device, cfg):
    from v2x_sim_amd import ops, packing
    cup, c, cout, N, H, W = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x = bf16r(torch.randn(N, c, H, W, generator=g))
    x_up = bf16r(torch.randn(N, cup, H // 2, W // 2, generator=g)) if cup else None
    w = torch.randn(cout, cup + c, 3, 3, generator=g) * (2.0 / ((cup + c) * 9)) ** 0.5
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    xin = torch.cat((F.interpolate(x_up, scale_factor=(2, 2)), x), 1) if cup else x
    ref = F.relu(F.conv2d(xin, bf16r(w), None, 1, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    pc = packing.pack_conv_stream("t", w, scale, shift, C0=cup if cup else c, C1=c if cup else 0, up0=1 if cup else 0,
                                  device=device)
    y = ops.conv2d(pc, nhwc(x_up, device), nhwc(x, device)) if cup else ops.conv2d(pc, nhwc(x, device))
    got = back(y)
    assert got.shape == ref.shape
    assert torch.allclose(got, ref, atol=2e-3, rtol=2 ** -7), float((got - ref).abs().max())
    # repeatability (the kernel's counted-vmcnt pipeline must not race): 5 more launches, identical bits
    for _ in range(5):
        y2 = ops.conv2d(pc, nhwc(x_up, device), nhwc(x, device)) if cup else ops.conv2d(pc, nhwc(x, device))
        assert torch.equal(y2, y)


def test_stream_two_plain_sources(device):
    """GRU-style concat without upsampling, plain BN/ReLU epilogue."""
    from v2x_sim_amd import ops, packing
    g = torch.Generator().manual_seed(3)
    a, b = bf16r(torch.randn(2, 64, 16, 32, generator=g)), bf16r(torch.randn(2, 64, 16, 32, generator=g))
    w = torch.randn(64, 128, 3, 3, generator=g) * 0.04
    scale, shift = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2
    ref = F.relu(F.conv2d(torch.cat((a, b), 1), bf16r(w), None, 1, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    pc = packing.pack_conv_stream("t", w, scale, shift, C0=64, C1=64, up0=0, device=device)
    got = back(ops.conv2d(pc, nhwc(a, device), nhwc(b, device)))
    assert torch.allclose(got, ref, atol=2e-3, rtol=2 ** -7)


@pytest.mark.parametrize("hw", [(32, 32), (16, 16)])
def test_stream_gru_vs_oracle(device, hw):
    from v2x_sim_amd import ops, packing
    H, W = hw
    torch.manual_seed(5)
    cell = R.Conv2dGRUCell(512, 256, 3)
    gen = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for p in cell.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.02)
        xx = bf16r(torch.randn(3, 512, H, W, generator=gen))
        ref = cell(xx, None, emulate=True)
    pc = packing.pack_gru_stream("gru", cell.weight_ih_l0, cell.bias_ih_l0, cell.bias_hh_l0, C0=256, C1=256, device=device)
    h = back(ops.conv2d(pc, nhwc(xx[:, :256], device), nhwc(xx[:, 256:], device)))
    assert torch.allclose(h, ref, atol=2 ** -7, rtol=2 ** -7), float((h - ref).abs().max())
    pg = packing.pack_gru("gru", cell.weight_ih_l0, cell.bias_ih_l0, cell.bias_hh_l0, C0=256, C1=256, device=device)
    h2 = back(ops.conv2d(pg, nhwc(xx[:, :256], device), nhwc(xx[:, 256:], device)))
    assert torch.allclose(h, h2, atol=2 ** -7, rtol=2 ** -7)


def test_stream_chain_8wave_form_on_a_full_launch(device, tune):
    """The chained 128 -> 128 -> 128 layer takes the 8-wave kernel only when its launch fills 3/4 of a round of the CUs (a handful of maps takes
    the 4-wave kernel's smaller tiles: same K order, same epilogue).  24 maps of 64 x 64 = 192 tiles is such a launch: bit-identical to the
    4-wave kernel on the same input (so the choice may follow the batch), and right against torch on the first two maps."""
    from v2x_sim_amd import ops, packing
    ch, N, H, W = 128, 24, 64, 64
    g = torch.Generator().manual_seed(77)
    x = bf16r(torch.randn(N, ch, H, W, generator=g))
    w1 = torch.randn(ch, ch, 3, 3, generator=g) * (2.0 / (ch * 9)) ** 0.5
    s1, t1 = torch.rand(ch, generator=g) + 0.5, torch.randn(ch, generator=g) * 0.2
    w2 = torch.randn(ch, ch, 1, 1, generator=g) * (2.0 / ch) ** 0.5
    s2, t2 = torch.rand(ch, generator=g) + 0.5, torch.randn(ch, generator=g) * 0.2
    pc = packing.pack_conv_stream("c", w1, s1, t1, relu=True, chain=(w2, s2, t2, True), device=device)
    xd = nhwc(x, device)
    y8 = ops.conv2d(pc, xd).clone()
    tune("STREAM_WAVES", 4)
    y4 = ops.conv2d(pc, xd).clone()
    assert torch.equal(y8.view(torch.int16), y4.view(torch.int16))
    small = ops.conv2d(pc, xd[:2].contiguous())        # two maps alone: the 4-wave kernel by the launch-size rule -- the same bits again
    tune.reset("STREAM_WAVES")
    small_default = ops.conv2d(pc, xd[:2].contiguous())
    assert torch.equal(small.view(torch.int16), y8[:2].view(torch.int16)) and torch.equal(small_default.view(torch.int16), y8[:2].view(torch.int16))
    hid = bf16r(F.relu(F.conv2d(x[:2], bf16r(w1), None, 1, 1) * s1.view(1, -1, 1, 1) + t1.view(1, -1, 1, 1)))
    ref = F.relu(F.conv2d(hid, bf16r(w2)) * s2.view(1, -1, 1, 1) + t2.view(1, -1, 1, 1))
    got = back(y8[:2])
    assert torch.allclose(got, ref, atol=3e-2, rtol=2 ** -6), float((got - ref).abs().max())


@pytest.mark.parametrize("gain", [1e-3, 0.3, 3.0, 40.0])
def test_gru_gate_arithmetic_over_its_whole_range(device, gain):
    """common.h: v2x_gru_h0 -- sigmoid / tanh on v_exp_f32 / v_rcp_f32 with the series below |x| = 2^-6.  Weight gain 1e-3 puts every
    pre-activation in the series branch, 0.3 straddles its switch at 2^-6, 40 saturates the gates (exp overflows to inf -> rcp 0 -> exactly
    0 / 1 / +-1).  All three kernels that emit GRU output (streamed 8-wave, streamed 4-wave, gather) against torch's fp32 gates."""
    from v2x_sim_amd import ops, packing
    torch.manual_seed(11)
    cell = R.Conv2dGRUCell(512, 256, 3)
    gen = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for name, p in cell.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.02 * gain * (0.05 if (gain < 1 and "bias" in name) else 1.0))
        xx = bf16r(torch.randn(2, 512, 16, 32, generator=gen))
        ref = cell(xx, None, emulate=True)
    assert torch.isfinite(ref).all()
    pc = packing.pack_gru_stream("gru", cell.weight_ih_l0, cell.bias_ih_l0, cell.bias_hh_l0, C0=256, C1=256, device=device)
    pg = packing.pack_gru("gru", cell.weight_ih_l0, cell.bias_ih_l0, cell.bias_hh_l0, C0=256, C1=256, device=device)
    x0, x1 = nhwc(xx[:, :256], device), nhwc(xx[:, 256:], device)
    outs = [back(ops.conv2d(pc, x0, x1)), back(ops.conv2d(pg, x0, x1))]
    for h in outs:
        assert torch.isfinite(h).all()
        # one bf16 rounding of the result + the fp32 sums' order: relative 2^-7, absolute a bf16 ulp of the smallest normal scale met here
        assert torch.allclose(h, ref, atol=2 ** -7 * max(float(ref.abs().max()), 1e-6), rtol=2 ** -7), float((h - ref).abs().max())
    if gain >= 40.0:
        assert float((ref.abs() > 0.99).float().mean()) > 0.2     # the saturated branch really is exercised
    if gain <= 1e-3:
        assert float(ref.abs().max()) < 2 ** -6


@pytest.mark.parametrize("hw", [(16, 32), (16, 16), (8, 32)])
@pytest.mark.parametrize("ch", [64, 128])
def test_stream_chain_conv1x1(device, hw, ch, tune):
    """conv1_2 -> conv3d_1 (64 ch) and conv2_2 -> conv3d_2 (128 ch) in the streamed kernel: 3x3 C->C +BN+ReLU (bf16 hidden,
    never stored) then 1x1 C->C +BN+ReLU.  16x32 maps take the 8-wave kernel at 128 channels, 8x32 / 16x16 the 4-wave one."""
    from v2x_sim_amd import ops, packing
    H, W = hw
    g = torch.Generator().manual_seed(15 + ch)
    x = bf16r(torch.randn(2, ch, H, W, generator=g))
    w1 = torch.randn(ch, ch, 3, 3, generator=g) * (2.0 / (ch * 9)) ** 0.5
    s1, t1 = torch.rand(ch, generator=g) + 0.5, torch.randn(ch, generator=g) * 0.2
    w2 = torch.randn(ch, ch, 1, 1, generator=g) * (2.0 / ch) ** 0.5
    s2, t2 = torch.rand(ch, generator=g) + 0.5, torch.randn(ch, generator=g) * 0.2
    hid = bf16r(F.relu(F.conv2d(x, bf16r(w1), None, 1, 1) * s1.view(1, -1, 1, 1) + t1.view(1, -1, 1, 1)))
    ref = F.relu(F.conv2d(hid, bf16r(w2)) * s2.view(1, -1, 1, 1) + t2.view(1, -1, 1, 1))
    pc = packing.pack_conv_stream("c", w1, s1, t1, relu=True, chain=(w2, s2, t2, True), device=device)
    got = back(ops.conv2d(pc, nhwc(x, device)))
    assert torch.allclose(got, ref, atol=3e-2, rtol=2 ** -6), float((got - ref).abs().max())
    assert float((got - ref).abs().mean()) < 2e-3
    if ch == 128 and H % 16 == 0 and W % 32 == 0:   # 8-wave and 4-wave kernels: same K order, same epilogue -> same bits
        # (two maps are below the few_chain_tiles bound of the dispatch: the launch above already was the 4-wave kernel's)
        assert ops.conv_kernel_name(pc, H, W, False, 2) == "conv3x3_stream_kernel<128, 8, 32, 1, false>"
        tune("STREAM_WAVES", 4)
        y4 = back(ops.conv2d(pc, nhwc(x, device)))
        assert torch.equal(got, y4)


@pytest.mark.parametrize("cfg", [
    # (C_up, C, Cout, N, H, W, gru)
    (0, 256, 256, 3, 32, 32, False),    # conv3_2 class
    (512, 256, 256, 2, 32, 32, False),  # conv5_1: half-resolution source + skip
    (256, 128, 128, 1, 64, 64, False),  # conv6_1
    (0, 128, 128, 2, 16, 32, False),    # a single 16x32 tile per map
    (256, 256, 256, 2, 32, 32, True),   # ConvGRU (two plain sources)
])
def test_stream8_equals_stream4_bitwise(device, cfg, tune):
    """The 8-wave ping-pong kernel walks K in the same order with the same fragment mapping as the 4-wave kernel:
    outputs must be identical bit for bit (and stable over repeated launches: its barrier/vmcnt protocol is new)."""
    from v2x_sim_amd import ops, packing
    cup, c, cout, N, H, W, gru = cfg
    g = torch.Generator().manual_seed(sum(cfg[:6]))
    x = nhwc(bf16r(torch.randn(N, c, H, W, generator=g)), device)
    if gru:
        x0 = nhwc(bf16r(torch.randn(N, cup, H, W, generator=g)), device)
        w = torch.randn(3 * cout, cup + c, 3, 3, generator=g) * 0.02
        b1, b2 = torch.randn(3 * cout, generator=g) * 0.1, torch.randn(3 * cout, generator=g) * 0.1
        pc = packing.pack_gru_stream("g", w, b1, b2, C0=cup, C1=c, device=device)
        run = lambda: ops.conv2d(pc, x0, x)
    else:
        w = torch.randn(cout, cup + c, 3, 3, generator=g) * (2.0 / ((cup + c) * 9)) ** 0.5
        scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
        pc = packing.pack_conv_stream("t", w, scale, shift, C0=cup if cup else c, C1=c if cup else 0,
                                      up0=1 if cup else 0, device=device)
        if cup:
            x0 = nhwc(bf16r(torch.randn(N, cup, H // 2, W // 2, generator=g)), device)
            run = lambda: ops.conv2d(pc, x0, x)
        else:
            run = lambda: ops.conv2d(pc, x)
    tune("STREAM_G", 0)          # the 1-tap 8-wave kernel (the 3-tap form has its own test below)
    tune("STREAM_WAVES", 4)
    y4 = run()
    tune.reset("STREAM_WAVES")
    y8 = run()
    assert torch.equal(y4, y8)
    for _ in range(10):
        assert torch.equal(run(), y8)
    # the default: three taps per synchronisation (stream8g).  K order (chunk, kx, ky) instead of (chunk, ky, kx): the same
    # products summed in another order -> at most one bf16 rounding apart, and bit-stable over launches
    tune.reset("STREAM_G")
    yg = run()
    assert ops.conv_kernel_name(pc, H, W, False, N).startswith("conv3x3_stream8g_kernel<")
    d = (yg.float() - y8.float()).abs()
    assert torch.allclose(yg.float(), y8.float(), atol=2e-3 if not gru else 2 ** -7, rtol=2 ** -7), float(d.max())
    assert float((yg != y8).float().mean()) < 0.02
    for _ in range(10):
        assert torch.equal(run(), yg)
    # the two wave tilings of stream8g (all channels x 64 pixels per wave / half the channels x 128 pixels) walk K in the same order:
    # bit-identical, for the plain layers (default: new tiling) and the ConvGRU (default: old tiling)
    tune("STREAM_WT", 0)
    assert ops.conv_kernel_name(pc, H, W, False, N) == "conv3x3_stream8g_kernel<%d, %d, false>" % ((96, 2) if gru else (128, 0))
    y_old = run()
    tune("STREAM_WT", 2)
    assert ops.conv_kernel_name(pc, H, W, False, N) == "conv3x3_stream8g_kernel<%d, %d, true>" % ((96, 2) if gru else (128, 0))
    y_new = run()
    tune.reset("STREAM_WT")
    assert torch.equal(y_old, yg) and torch.equal(y_new, yg)
    # (the 32x32x16-MFMA form of this kernel -- round 3, measured 9-20 % slower, removed from the source in round 4 -- was verified BIT-IDENTICAL
    # to this one on these five cases and on the bench layers: profiles/r03_m32_rejected.txt)


@pytest.mark.parametrize("cfg", [
    # (C_up, C, Cout, N, H, W, gru): enough tiles (> 256 workgroups) for the persistent form to take several tiles each
    (0, 256, 256, 160, 32, 32, False),   # conv3_2 at the bench batch: 640 tiles, 2.5 per workgroup (uneven tail)
    (256, 128, 128, 40, 64, 64, False),  # conv6_1: half-resolution source first -> descriptor tables switch resolution
    (256, 256, 256, 40, 32, 32, True),   # ConvGRU: 8 channel tiles
    (0, 128, 128, 33, 64, 64, False),    # 264 tiles: 8 workgroups take a second tile, 248 do not
])
def test_stream8_persistent_equals_one_tile_per_workgroup_bitwise(device, cfg, tune):
    """The persistent 8-wave kernel (tiles bid, bid + grid, ...; next tile's patch and weight slices prefetched across the
    tile boundary, relaxed vmcnt after the epilogue) must produce exactly the bits of the one-tile-per-workgroup launch."""
    from v2x_sim_amd import ops, packing
    cup, c, cout, N, H, W, gru = cfg
    g = torch.Generator().manual_seed(sum(cfg[:6]))
    x = torch.randn(N, H, W, c, generator=g).to(torch.bfloat16).to(device)
    if gru:
        x0 = torch.randn(N, H, W, cup, generator=g).to(torch.bfloat16).to(device)
        w = torch.randn(3 * cout, cup + c, 3, 3, generator=g) * 0.02
        pc = packing.pack_gru_stream("g", w, torch.randn(3 * cout, generator=g) * 0.1, torch.randn(3 * cout, generator=g) * 0.1,
                                     C0=cup, C1=c, device=device)
        run = lambda: ops.conv2d(pc, x0, x)
    else:
        w = torch.randn(cout, cup + c, 3, 3, generator=g) * (2.0 / ((cup + c) * 9)) ** 0.5
        pc = packing.pack_conv_stream("t", w, torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2,
                                      C0=cup if cup else c, C1=c if cup else 0, up0=1 if cup else 0, device=device)
        if cup:
            x0 = torch.randn(N, H // 2, W // 2, cup, generator=g).to(torch.bfloat16).to(device)
            run = lambda: ops.conv2d(pc, x0, x)
        else:
            run = lambda: ops.conv2d(pc, x)
    tune("STREAM_G", 0)
    tune("STREAM_PERSIST", 0)
    ref = run()
    tune.reset("STREAM_PERSIST")
    for _ in range(5):
        assert torch.equal(run(), ref)
    # the 3-tap form is always persistent: its multi-tile walk (ring and patch fill wrapping into the next tile) against the
    # 1-tap kernel at one bf16 rounding, bit-stable over launches
    tune.reset("STREAM_G")
    yg = run()
    assert torch.allclose(yg.float(), ref.float(), atol=2e-3 if not gru else 2 ** -7, rtol=2 ** -7), float((yg.float() - ref.float()).abs().max())
    assert float((yg != ref).float().mean()) < 0.02
    for _ in range(5):
        assert torch.equal(run(), yg)



@pytest.mark.parametrize("cfg", [
    # (C, Cout, N, H, W): H % 8 == 0, W % 64 == 0 (4 x 32 output tiles) or H % 16 == 0, W % 32 == 0 (8 x 16)
    (32, 64, 3, 16, 64),      # conv1_1 class (one chunk, BCO = 64)
    (64, 128, 2, 24, 128),    # conv2_1 class (two chunks, BCO = 128)
    (128, 256, 2, 8, 64),     # conv3_1 class (two channel tiles)
    (256, 512, 3, 32, 32),    # conv4_1: 16 x 16 outputs -> the 8 x 16 output-tile form (four channel tiles, 8 chunks)
    (64, 64, 2, 16, 32),      # 8 x 16 form with BCO = 64, one tile per map, every border is padding
    (128, 128, 1, 48, 96),    # 8 x 16 form, 3 x 3 tiles per map (interior + border tiles)
])
def test_stride2_stream_conv_vs_torch_and_gather(device, cfg):
    """Stride-2 streamed kernel (conv_stream_s2.hip: parity-de-interleaved patch) vs torch fp32 on the same bf16 operands
    (one bf16 ulp) and vs the gather kernel on the same layer."""
    from v2x_sim_amd import ops, packing
    C, Cout, N, H, W = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x = bf16r(torch.randn(N, C, H, W, generator=g))
    w = torch.randn(Cout, C, 3, 3, generator=g) * (2.0 / (C * 9)) ** 0.5
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.2
    ref = F.relu(F.conv2d(x, bf16r(w), None, 2, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    pc = packing.pack_conv_stream("s2", w, scale, shift, C0=C, stride=2, device=device)
    got = back(ops.conv2d(pc, nhwc(x, device)))
    assert got.shape == ref.shape == (N, Cout, H // 2, W // 2)
    assert torch.allclose(got, ref, atol=2e-3, rtol=2 ** -7), float((got - ref).abs().max())
    pg = packing.pack_conv("g", w, scale, shift, stride=2, pad=1, relu=True, device=device)
    alt = back(ops.conv2d(pg, nhwc(x, device)))
    assert torch.allclose(got, alt, atol=2e-3, rtol=2 ** -7)


@pytest.mark.parametrize("cfg", [
    # (C, Cout, N, H, W): output maps tile by 8 x 32, or by 16 x 16
    (64, 128, 2, 32, 128),     # conv2_1 class: two chunks, 8 x 32 tiles, 2 x 2 tiles per map
    (128, 256, 3, 16, 64),     # conv3_1 class: two channel tiles, one tile per map (every border is padding)
    (256, 512, 2, 32, 32),     # conv4_1: 16 x 16 outputs -> the 16 x 16 tile form, four channel tiles, 8 chunks
    (96, 128, 5, 64, 96),      # three chunks, 16 x 16 tiles, 2 x 3 tiles per map
    (64, 128, 40, 48, 64),     # persistent walk: more tiles than workgroups (3 x 1 tiles x 40 maps on <= 256 CUs needs > 256: see N)
])
def test_stride2_three_tap_kernel_vs_torch_and_one_tap(device, cfg, tune):
    """conv3x3_s2g_kernel (8 waves, three taps per synchronisation, parity-split patch refilled in place) vs torch fp32 on the same bf16
    operands and vs the 1-tap stride-2 kernel: K order (chunk, kx in {0, 2, 1}, ky) differs, so one bf16 rounding, not bits.  S2_G = 2
    forces the form for launches that would not fill the chip; repeated launches are bit-stable."""
    from v2x_sim_amd import ops, packing
    C, Cout, N, H, W = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    if N == 40:
        N = 2 * torch.cuda.get_device_properties(0).multi_processor_count // 3 + 7     # > 2 tiles per workgroup, ragged tail
    x = bf16r(torch.randn(N, C, H, W, generator=g))
    w = torch.randn(Cout, C, 3, 3, generator=g) * (2.0 / (C * 9)) ** 0.5
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.2
    ref = F.relu(F.conv2d(x, bf16r(w), None, 2, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    pc = packing.pack_conv_stream("s2", w, scale, shift, C0=C, stride=2, device=device)
    xd = nhwc(x, device)
    tune("S2_G", 2)
    assert ops.conv_kernel_name(pc, H, W, False, N) == "conv3x3_s2g_kernel<%s>" % ("8, 32" if (W // 2) % 32 == 0 else "16, 16")
    got = ops.conv2d(pc, xd)
    for _ in range(3):
        assert torch.equal(ops.conv2d(pc, xd), got)
    tune("S2_G", 0)
    assert ops.conv_kernel_name(pc, H, W, False, N) == "conv3x3_s2_stream_kernel<128, %s, false>" % ("4, 32" if W % 64 == 0 else "8, 16")
    one = ops.conv2d(pc, xd)
    got, one = back(got), back(one)
    assert got.shape == ref.shape == (N, Cout, H // 2, W // 2)
    assert torch.allclose(got, ref, atol=2e-3, rtol=2 ** -7), float((got - ref).abs().max())
    assert torch.allclose(got, one, atol=2e-3, rtol=2 ** -7)
    assert float((got != one).float().mean()) < 0.02


@pytest.mark.parametrize("cfg", [
    # (C_up, C, N, H, W, chain)
    (128, 64, 2, 32, 64, False),   # conv7_1 class: half-resolution source + skip
    (0, 64, 3, 16, 32, False),     # conv7_2 class (one 16x32 tile per map)
    (0, 64, 2, 32, 32, True),      # conv1_2 -> conv3d_1 chain
])
def test_wide_kernel_equals_256_pixel_kernel_bitwise(device, cfg, tune):
    """The wide 4-wave form (128 pixels per wave, single-buffered patch) walks K in the same order with the same
    fragments as the 256-pixel kernel and shares its epilogue: identical bits, also over repeated launches."""
    from v2x_sim_amd import ops, packing
    cup, c, N, H, W, chain = cfg
    g = torch.Generator().manual_seed(sum(cfg[:5]))
    x = torch.randn(N, H, W, c, generator=g).to(torch.bfloat16).to(device)
    w = torch.randn(64, cup + c, 3, 3, generator=g) * (2.0 / ((cup + c) * 9)) ** 0.5
    ch = (torch.randn(64, 64, 1, 1, generator=g) * 0.2, torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2, True) if chain else None
    pc = packing.pack_conv_stream("t", w, torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2,
                                  C0=cup if cup else c, C1=c if cup else 0, up0=1 if cup else 0, chain=ch, device=device)
    if cup:
        x0 = torch.randn(N, H // 2, W // 2, cup, generator=g).to(torch.bfloat16).to(device)
        run = lambda: ops.conv2d(pc, x0, x)
    else:
        run = lambda: ops.conv2d(pc, x)
    tune("STREAM_WIDE", 0)
    ref = run()
    tune.reset("STREAM_WIDE")
    tune("WIDE3", 0)            # the 1-tap wide form (the 3-tap form walks K in another order: below)
    for _ in range(5):
        assert torch.equal(run(), ref)
    tune.reset("WIDE3")
    # default for the plain epilogue: three taps per synchronisation (conv3x3_wide3_kernel), K order (chunk, kx, ky): the same products
    # summed in another order -> at most one bf16 rounding apart, and bit-stable over launches
    y3 = run()
    name = ops.conv_kernel_name(pc, H, W, False, N)
    three = not chain and cup + c >= 96
    assert name == ("conv3x3_wide3_kernel<64>" if three else "conv3x3_wide_kernel<64, %d>" % (1 if chain else 0)), name
    if not three:
        assert torch.equal(y3, ref)
    else:
        assert torch.allclose(y3.float(), ref.float(), atol=2e-3, rtol=2 ** -7), float((y3.float() - ref.float()).abs().max())
        assert float((y3 != ref).float().mean()) < 0.02
    for _ in range(5):
        assert torch.equal(run(), y3)


@pytest.mark.parametrize("layer", ["conv5_1", "conv6_1", "conv7_1", "convgru", "conv2_1"])
def test_full_size_properties_batch_equivariance_and_scaling(device, layer):
    """Size-independent properties at the BENCH size (one half-batch = 320 maps; the oracle cannot follow there):
    (a) the batch is a set -- permuting the maps permutes the outputs, bit for bit (the persistent kernels walk tiles of many maps per
        workgroup: nothing may leak across maps or depend on a map's position in the launch);
    (b) exact homogeneity under power-of-two scaling for the plain layers -- y(4 x) == 4 y(x) bitwise with shift = 0 (fp32 accumulation and
        bf16 rounding commute with a power of two, ReLU is positively homogeneous), which pins every tap's weight to ITS pixel: a dropped or
        doubled tap at some tile border would survive (a) but not the comparison with torch on the small cases above -- this ties the two."""
    from v2x_sim_amd import ops, packing
    g = torch.Generator().manual_seed(len(layer) * 7)
    N = 320
    if layer == "convgru":
        w = torch.randn(768, 512, 3, 3, generator=g) * 0.02
        pc = packing.pack_gru_stream("g", w, torch.randn(768, generator=g) * 0.1, torch.randn(768, generator=g) * 0.1, C0=256, C1=256, device=device)
        xs = [torch.relu(torch.randn(N, 32, 32, 256, generator=g)).to(torch.bfloat16).to(device) for _ in range(2)]
        plain = False
    else:
        c0, c1, cout, hw, up, stride = {"conv5_1": (512, 256, 256, 32, 1, 1), "conv6_1": (256, 128, 128, 64, 1, 1), "conv7_1": (128, 64, 64, 128, 1, 1),
                                        "conv2_1": (64, 0, 128, 128, 0, 2)}[layer]
        if hw == 128:
            N = 160
        w = torch.randn(cout, c0 + c1, 3, 3, generator=g) * (2.0 / ((c0 + c1) * 9)) ** 0.5
        pc = packing.pack_conv_stream(layer, w, torch.rand(cout, generator=g) + 0.5, torch.zeros(cout), C0=c0 if c1 else c0 + c1, C1=c1, up0=up, relu=True,
                                      stride=stride, device=device)
        h0 = hw // 2 if up else hw
        xs = [torch.relu(torch.randn(N, h0, h0, c0, generator=g)).to(torch.bfloat16).to(device)]
        if c1:
            xs.append(torch.relu(torch.randn(N, hw, hw, c1, generator=g)).to(torch.bfloat16).to(device))
        plain = True
    run = lambda t: ops.conv2d(pc, *t)
    y = run(xs)
    perm = torch.randperm(N, generator=g).to(device)
    yp = run([t[perm].contiguous() for t in xs])
    assert torch.equal(yp, y[perm]), "%s: outputs depend on the position of a map in the batch" % layer
    if plain:
        y4 = run([(t.float() * 4).to(torch.bfloat16) for t in xs])
        assert torch.equal(y4.float(), y.float() * 4), "%s: y(4x) != 4 y(x)" % layer
        assert float(y.float().abs().max()) > 0.1


@pytest.mark.parametrize("cfg", [
    # (C_up, C, Cout, N, H, W, gru, splitk)
    (512, 256, 256, 5, 32, 32, False, 6),    # conv5_1 at ONE collaborative frame: 24 chunks in 6 ranges, half-resolution source first
    (0, 256, 256, 5, 32, 32, False, 4),      # conv3_2 / conv5_2: 8 chunks
    (0, 512, 512, 5, 16, 16, False, 8),      # conv4_2: 16x16 tiles
    (256, 128, 128, 5, 64, 64, False, 3),    # conv6_1
    (0, 128, 128, 2, 16, 32, False, 3),      # 4 chunks in 3 ranges (2, 2) -> refused (an empty range): falls to 2
    (256, 256, 256, 5, 32, 32, True, 2),     # ConvGRU: gate epilogue in the reduce kernel
    (256, 256, 256, 3, 32, 32, True, 5),     # 16 chunks in 5 ranges of 4, 4, 4, 4 (the last one would be empty): refused -> 4
    (128, 64, 64, 5, 128, 128, False, 2),    # conv7_1: 64-row tiles
])
def test_small_batch_splitk(device, cfg, tune):
    """Latency mode: the chunk range of a streamed layer divided over `splitk` workgroups per tile + splitk_reduce_kernel (fixed-order sum,
    epilogue).  Against torch fp32 on the same bf16 operands (one bf16 ulp), against the default kernel (fp32 summation order: one bf16
    rounding on few entries), bit-stable over launches; a split with an empty range is refused by the library."""
    from v2x_sim_amd import ops, packing
    cup, c, cout, N, H, W, gru, splitk = cfg
    g = torch.Generator().manual_seed(sum(cfg[:6]) + splitk)
    x = bf16r(torch.randn(N, c, H, W, generator=g))
    if gru:
        x0 = bf16r(torch.randn(N, cup, H, W, generator=g))
        cell = R.Conv2dGRUCell(cup + c, cout, 3)
        with torch.no_grad():
            for p in cell.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            ref = cell(torch.cat((x0, x), 1), None, emulate=True)
        pc = packing.pack_gru_stream("g", cell.weight_ih_l0, cell.bias_ih_l0, cell.bias_hh_l0, C0=cup, C1=c, device=device)
        a0, a1 = nhwc(x0, device), nhwc(x, device)
        tol = dict(atol=2 ** -7, rtol=2 ** -7)
    else:
        w = torch.randn(cout, cup + c, 3, 3, generator=g) * (2.0 / ((cup + c) * 9)) ** 0.5
        scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
        pc = packing.pack_conv_stream("t", w, scale, shift, C0=cup if cup else c, C1=c if cup else 0, up0=1 if cup else 0, device=device)
        if cup:
            xu = bf16r(torch.randn(N, cup, H // 2, W // 2, generator=g))
            xin = torch.cat((F.interpolate(xu, scale_factor=(2, 2)), x), 1)
            a0, a1 = nhwc(xu, device), nhwc(x, device)
        else:
            xin, a0, a1 = x, nhwc(x, device), None
        ref = F.relu(F.conv2d(xin, bf16r(w), None, 1, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
        tol = dict(atol=2e-3, rtol=2 ** -7)
    base = ops.conv2d(pc, a0, a1)
    chunks = (cup + c) // 32
    if -(-chunks // splitk) * (splitk - 1) >= chunks:
        with pytest.raises(Exception, match="not tileable|v2x_conv2d"):
            ops.conv2d(pc, a0, a1, splitk=splitk)
        splitk -= 1
    y = ops.conv2d(pc, a0, a1, splitk=splitk)
    assert torch.allclose(back(y), ref, **tol), float((back(y) - ref).abs().max())
    assert torch.allclose(y.float(), base.float(), **tol) and float((y != base).float().mean()) < 0.03
    for _ in range(4):
        assert torch.equal(ops.conv2d(pc, a0, a1, splitk=splitk), y)
    # the switch: off -> run_layer launches the default kernel; on -> small_batch_splitk picks a split that fills the chip
    assert ops.small_batch_splitk(pc, N, H, W) == 0
    tune("SMALL_BATCH", 1)
    s_auto = ops.small_batch_splitk(pc, N, H, W)
    tiles = N * (H * W // 256) * (pc.w_rows // ops._lib.load().v2x_conv_stream_tile_rows(pc.Cout, pc.epilogue))
    assert s_auto == 0 or (2 <= s_auto <= chunks // 2 and tiles < 200 and tiles * s_auto <= 520), (s_auto, tiles, chunks)
    if s_auto:
        assert torch.allclose(back(ops.conv2d(pc, a0, a1, splitk=s_auto)), ref, **tol)


def test_gru_xcd_walk_is_a_pure_reordering(device, tune):
    """GRU_XCD_WALK only permutes which workgroup computes which (pixel tile, channel tile) of the ConvGRU's persistent grid (8 x 4 tiles per XCD
    and round instead of 4 x 8: -16 % fabric reads): identical bits, also when the tile count is not a multiple of the grid."""
    from v2x_sim_amd import ops, packing
    g = torch.Generator().manual_seed(11)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    for N in (ncu // 16 + 3, 2 * ncu // 16 + 1):          # 2 pixel tiles x 8 channel tiles per map: more tiles than workgroups, ragged tail
        w = torch.randn(768, 512, 3, 3, generator=g) * 0.02
        pc = packing.pack_gru_stream("gru", w, torch.randn(768, generator=g) * 0.1, torch.randn(768, generator=g) * 0.1, C0=256, C1=256, device=device)
        x0 = torch.randn(N, 32, 32, 256, generator=g).to(torch.bfloat16).to(device)
        x1 = torch.randn(N, 32, 32, 256, generator=g).to(torch.bfloat16).to(device)
        tune("GRU_XCD_WALK", 0)
        ref = ops.conv2d(pc, x0, x1)
        tune("GRU_XCD_WALK", 1)
        assert torch.equal(ops.conv2d(pc, x0, x1), ref)


@pytest.mark.parametrize("cfg", [(256, 512, 5, 32, 32), (128, 256, 5, 64, 64), (256, 128, 3, 16, 64), (128, 64, 2, 32, 32)])
def test_stride2_split_k_form_vs_torch_and_unsplit(device, cfg, tune):
    """Latency mode for the stride-2 layers (conv4_1 / conv3_1 at one frame): the 1-tap stride-2 kernel with the chunk range divided over
    blockIdx.y + splitk_reduce_kernel.  Every legal split agrees with torch fp32 on the same bf16 operands and with the unsplit kernel to one bf16
    rounding (fp32 summation order), is bit-stable, and ops.small_batch_splitk picks a split only with SMALL_BATCH = 1."""
    from v2x_sim_amd import ops, packing
    C, Cout, N, H, W = cfg
    g = torch.Generator().manual_seed(sum(cfg))
    x = bf16r(torch.randn(N, C, H, W, generator=g))
    w = torch.randn(Cout, C, 3, 3, generator=g) * (2.0 / (C * 9)) ** 0.5
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.2
    ref = F.relu(F.conv2d(x, bf16r(w), None, 2, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    pc = packing.pack_conv_stream("s2", w, scale, shift, C0=C, stride=2, device=device)
    xd = nhwc(x, device)
    tune("S2_G", 0)
    base = ops.conv2d(pc, xd)
    chunks = C // 32
    for sk in range(2, chunks + 1):
        if -(-chunks // sk) * (sk - 1) >= chunks:
            continue                                   # an empty range: the library refuses it
        y = ops.conv2d(pc, xd, splitk=sk)
        assert torch.equal(ops.conv2d(pc, xd, splitk=sk), y)
        got = back(y)
        assert torch.allclose(got, ref, atol=2e-3, rtol=2 ** -7), (sk, float((got - ref).abs().max()))
        assert torch.allclose(got, back(base), atol=2e-3, rtol=2 ** -7) and float((y != base).float().mean()) < 0.02
    tune("SMALL_BATCH", 0)
    assert ops.small_batch_splitk(pc, N, H, W) == 0
    tune("SMALL_BATCH", 1)
    sk = ops.small_batch_splitk(pc, N, H, W)
    assert sk == 0 or (2 <= sk <= chunks // 2)
    if C == 256 and Cout == 512:
        assert sk == 4                                  # conv4_1 at one frame: 40 tiles, 8 chunks


def test_plan_call_leaves_the_lds_opt_in_to_the_first_launch():
    """ops.conv_kernel_name asks the library which kernel a layer takes (v2x_conv2d_plan: the dispatch with the launch helper recording instead of launching).
    Such a call must not use up the helper's once-per-device state: in a FRESH process (a child; nothing has launched the kernel there) the name of a
    32 -> 128 layer on one 16 x 32 map -- stream8g, 153 KiB of LDS, impossible without the opt-in -- is asked first, then the layer is launched and compared
    with torch fp32 on the same bf16 operands at test_stream_conv_vs_torch's tolerance.  A consumed flag shows as a launch error."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = """
import sys
sys.path[:0] = [%r, %r]
import torch
import torch.nn.functional as F
from v2x_sim_amd import ops, packing
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(32 + 128)
r = lambda t: t.to(torch.bfloat16).to(torch.float32)
x = r(torch.randn(1, 32, 16, 32, generator=g))
w = torch.randn(128, 32, 3, 3, generator=g) * (2.0 / (32 * 9)) ** 0.5
scale, shift = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g) * 0.2
ref = F.relu(F.conv2d(x, r(w), None, 1, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
pc = packing.pack_conv_stream("t", w, scale, shift, C0=32, device=dev)
print("NAME", ops.conv_kernel_name(pc, 16, 32))
y = ops.conv2d(pc, x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(dev))
got = y.float().cpu().permute(0, 3, 1, 2)
print("MAXERR", float((got - ref).abs().max()))
print("CLOSE", bool(torch.allclose(got, ref, atol=2e-3, rtol=2 ** -7)))
""" % (root, os.path.join(root, "v2x-sim_amd"))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "NAME conv3x3_stream8g_kernel<128, 0, true>\n" in p.stdout and "CLOSE True" in p.stdout, p.stdout + p.stderr

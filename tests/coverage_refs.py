"""Which extents the convolution kernel families tile, written out over plain integers: the rules ops.run_layer and train/hip_graph.py carried
in Python before they asked the library (ops.covers / ops.select: v2x_conv2d_plan, v2x_conv3x3_wgrad_splits).  An independent statement for
tests/test_coverage_cpu.py to hold the library's answers to; a plain helper module (as tests/conv_refs.py), nothing here calls the library."""
BF16, F32, GRU = 0, 1, 2

# 18 extents from 2 to 256 -- below a tile, odd, every tile size and multiples that are none of another's -- and, as widths only, six wide maps
# around the halo kernels' DMA-table bound (10 W + 34) cmax < 2^20: W < 1635 at 64 channels, W < 3274 at 32
EXTENTS = (2, 4, 7, 8, 12, 16, 24, 32, 40, 48, 56, 64, 80, 96, 128, 160, 192, 256)
WIDE = (1600, 1632, 1664, 3264, 3296, 6560)

# the eight packed forms of the sweep: the descriptor fields a packer sets (tests/conv_refs.py::desc fills in w_rows / w_kpad the same way)
FORMS = {
    "halo 32->32": dict(w_layout=1, C0=32, Cout=32),
    "halo 64->64": dict(w_layout=1, C0=64, Cout=64),
    "halo parity 64+32->32": dict(w_layout=3, C0=64, C1=32, up0=1, Cout=32),
    "stream 128->128": dict(w_layout=2, C0=128, Cout=128),
    "stream 64->64": dict(w_layout=2, C0=64, Cout=64),
    "stream parity 256+128->128": dict(w_layout=4, C0=256, C1=128, up0=1, Cout=128),
    "stream parity 128+64->64": dict(w_layout=4, C0=128, C1=64, up0=1, Cout=64),
    "stride-2 64->128": dict(w_layout=2, stride=2, C0=64, Cout=128),
}
# five more for the switch-independence table: the other halo instantiations, a chained fp32 head and the ConvGRU
MORE_FORMS = {
    "halo 64->32": dict(w_layout=1, C0=64, Cout=32),
    "halo 32->64": dict(w_layout=1, C0=32, Cout=64),
    "halo 64+32->32": dict(w_layout=1, C0=64, C1=32, up0=1, Cout=32),
    "halo heads 32->64->48": dict(w_layout=1, C0=32, Cout=64, Cout2=48, epilogue=F32),
    "stream gru 256+256->256": dict(w_layout=2, C0=256, C1=256, Cout=256, epilogue=GRU),
}


def halo_eligible(H, W, w_layout=1, cmax=0, cout=0):
    """cmax: the widest source's channel count -- the halo kernel's packed DMA tables hold a lane's element offset inside the patch rows
    in 20 bits ((10 W + 34) cmax < 2^20)."""
    if w_layout in (1, 3) and (10 * W + 34) * cmax >= (1 << 20):
        return False
    if w_layout == 4:
        return H % 16 == 0 and W % (64 if cout == 64 else 32) == 0      # the streamed parity-class kernels: 16 x 32 tiles (pairs of them at 64 rows)
    if H % 8 == 0 and W % 32 == 0:
        return True
    return w_layout == 2 and H % 16 == 0 and W % 16 == 0  # the streamed kernel also has 16x16 tiles


def stride2_eligible(H, W):
    """The stride-2 streamed kernel: 4 x 32 output tiles, or 8 x 16 ones for narrow maps."""
    return (H % 8 == 0 and W % 64 == 0) or (H % 16 == 0 and W % 32 == 0)


def covered(form, H, W):
    """The library has a kernel for this packed form on maps of H x W."""
    if form.get("stride", 1) == 2:
        return stride2_eligible(H, W)
    return halo_eligible(H, W, form["w_layout"], max(form["C0"], form.get("C1", 0)), form["Cout"])


def selected(form, H, W):
    """run_layer launches the form's packing (not the gather fallback chain): covered, and the streamed stride-1 forms from 256 pixels on."""
    return covered(form, H, W) and (form.get("stride", 1) == 2 or form["w_layout"] not in (2, 4) or H * W >= 256)


def selected_from_bits(form, H, W):
    """run_layer hands the bit grid itself to the layer: a halo packing (the 32 -> 32 first layer) on a map that tiles by 8 x 32 (no
    DMA-table bound was asked: on a bit grid wider than 3273 the launch was refused)."""
    return form["w_layout"] == 1 and halo_eligible(H, W, 1)


# ---- the training graph (train/hip_graph.py::hip_eligible as it was): channel pairs (cin, cout, cin_pad), both strides, 12 x 12 extents
TRAIN_CHANNELS = ((13, 32, 32), (32, 32, None), (32, 64, None), (64, 64, None), (64, 32, None), (64, 128, None), (128, 128, None), (128, 256, None),
                  (256, 256, None), (256, 512, None), (512, 512, None), (96, 32, None), (32, 96, None), (192, 64, None), (384, 128, None))
TRAIN_EXTENTS = (4, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256)


def train_layout(cin_p, cout, stride):
    """packing.train_layout with every packing switch at its default: 1 = halo kernel, 2 = streamed kernels, 0 = gather kernel."""
    if stride == 1 and (cin_p, cout) in ((32, 32), (64, 64), (64, 32)):
        return 1
    if stride == 1 and cin_p >= 64 and cin_p % 32 == 0 and cout % 64 == 0:
        return 2
    if stride == 2 and cin_p % 32 == 0 and cout % 64 == 0:
        return 2
    return 0


def layer_runs(cin_p, cout, stride, H, W):
    layout = train_layout(cin_p, cout, stride)
    if layout == 0:
        return True                                    # the gather kernel takes any extent
    if stride == 2:
        return stride2_eligible(H, W)
    return halo_eligible(H, W, layout, cin_p) and (layout != 2 or H * W >= 256)


def hip_eligible(cout, cin, stride, H, W, cin_pad=None, k=3):
    if not (k == 3 and stride in (1, 2) and cout % 32 == 0 and H % 8 == 0 and W % 32 == 0):
        return False
    cin_p = cin_pad if cin_pad is not None else (cin + 31) // 32 * 32
    if cin_p % 32:
        return False
    return layer_runs(cin_p, cout, stride, H, W) and layer_runs(cout, cin_p, 1, H, W)


def upcat_conv_rule_was(H, W):
    """What upcat_conv3x3 asked of its full-resolution extent before it asked the library: the tile sizes, without the DMA-table bound."""
    return H % 8 == 0 and W % 32 == 0

"""Which extents a conv kernel family tiles is the library's answer: ops.covers / ops.select / ops.wgrad_covers ask v2x_conv2d_plan and
v2x_conv3x3_wgrad_splits, memoise the boolean, and Python keeps no copy of the tile sizes or table bounds.  No GPU: nothing is launched.
  * the answers are the ones the retired Python rules gave (tests/coverage_refs.py holds those rules over plain integers), with no disagreement;
  * the covered set follows no library switch, so a memoised boolean needs no invalidation;
  * a second question for the same key makes no library call, a refusal included;
  * the training graph's fused full-resolution layer gives way to the unfused one where the map is too wide for the halo kernels' tables;
  * the functions that select kernels hold no extent arithmetic of their own."""
import inspect

import pytest
import torch

import coverage_refs as R
from conv_refs import desc


def packed(**form):
    """A PackedConv without tensors for a coverage_refs form: w_rows / w_kpad / out_cstride as tests/conv_refs.py::desc sets them."""
    from v2x_sim_amd import ops
    d = desc(H=8, W=32, **form)
    return ops.PackedConv(name="t", C0=d.C0, C1=d.C1, up0=d.up0, Cout=d.Cout, ksize=d.ksize, stride=d.stride, pad=d.pad, epilogue=d.epilogue,
                          relu=True, w_rows=d.w_rows, w_kpad=d.w_kpad, w_layout=d.w_layout or None, Cout2=d.Cout2, relu2=False)


def layer_of(pc):
    """pc as the patch-based packing of a layer whose gather fallback is never launched here."""
    from v2x_sim_amd import ops
    return ops.Layer([packed(C0=pc.C0, C1=pc.C1, up0=pc.up0, Cout=pc.Cout, stride=pc.stride)], pc)


SWEEP = [(H, W) for H in R.EXTENTS for W in R.EXTENTS + R.WIDE]


def test_covers_and_select_give_the_retired_rules_answers():
    from v2x_sim_amd import ops
    assert len(R.FORMS) * len(SWEEP) == 3456
    wrong = []
    for name, form in R.FORMS.items():
        pc = packed(**form)
        layer = layer_of(pc)
        for H, W in SWEEP:
            if ops.covers(pc, H, W) != R.covered(form, H, W):
                wrong.append(("covers", name, H, W))
            sel = ops.select(layer, 1, H, W)
            if (sel is not None) != R.selected(form, H, W) or (sel is not None and sel != (pc, 0)):
                wrong.append(("select", name, H, W))
    assert not wrong, wrong[:20]


def test_select_hands_the_bit_grid_to_the_first_layers_halo_packing_only():
    from v2x_sim_amd import ops
    wrong = []
    for name, form in R.FORMS.items():
        pc = packed(**form)
        layer = layer_of(pc)
        for H in R.EXTENTS:
            for W in R.EXTENTS:
                want = name == "halo 32->32" and R.selected_from_bits(form, H, W)
                sel = ops.select(layer, 1, H, W, bits=True)
                if (sel == (pc, 0)) != want or (sel is not None) != want:
                    wrong.append((name, H, W))
    assert not wrong, wrong[:20]
    assert ops.select(ops.Layer([packed(C0=32, Cout=32)]), 1, 8, 32, bits=True) is None        # no patch-based packing at all: the fallback chain


def test_select_prefers_the_latency_packing_only_where_it_is_declared_covered_and_split(tune):
    from v2x_sim_amd import ops
    form = R.FORMS["stream parity 256+128->128"]
    pc, lat = packed(**form), packed(**dict(form, w_layout=2))
    layer = layer_of(pc)
    layer.latency = lat
    tune("SMALL_BATCH", 2)
    assert ops.select(layer, 5, 32, 32) == (pc, 0)                     # no declaration: the throughput form
    with ops.latency_dispatch():
        sk = ops.small_batch_splitk(lat, 5, 32, 32)
        assert sk > 1 and ops.select(layer, 5, 32, 32) == (lat, sk)   # conv5_1 at one frame: 20 tiles, 12 chunks
        assert ops.select(layer, 320, 32, 32) == (pc, 0)              # a full launch is not split
        assert ops.select(layer, 5, 24, 48) is None                   # neither form tiles 24 x 48: the fallback chain, no split asked of it


def test_hip_eligible_gives_the_retired_rules_answers():
    from v2x_sim_amd.train import hip_graph
    n, wrong = 0, []
    for cin, cout, cin_pad in R.TRAIN_CHANNELS:
        w = torch.empty((cout, cin, 3, 3), device="meta")
        for stride in (1, 2):
            for H in R.TRAIN_EXTENTS:
                for W in R.TRAIN_EXTENTS:
                    n += 1
                    if hip_graph.hip_eligible(w, stride, H, W, cin_pad) != R.hip_eligible(cout, cin, stride, H, W, cin_pad):
                        wrong.append((cin, cout, stride, H, W))
    assert n == 4320 and not wrong, wrong[:20]
    assert not hip_graph.hip_eligible(torch.empty((64, 64, 1, 1), device="meta"), 1, 32, 32)
    assert not hip_graph.hip_eligible(torch.empty((64, 64, 3, 3), device="meta"), 3, 32, 32)
    assert not hip_graph.hip_eligible(torch.empty((64, 64, 3, 3), device="meta"), 1, 32, 32, 40)      # a stored channel count that is no whole tile
    assert not hip_graph.hip_eligible(torch.empty((48, 64, 3, 3), device="meta"), 1, 32, 32)


def test_wgrad_covers_is_the_weight_gradient_kernels_requirement():
    from v2x_sim_amd import ops
    for H in R.TRAIN_EXTENTS + (1664,):
        for W in R.TRAIN_EXTENTS + (1664,):
            for cin, cout in ((32, 32), (96, 32), (64, 48), (40, 64), (256, 512), (0, 32)):
                want = H % 8 == 0 and W % 32 == 0 and cin > 0 and cin % 32 == 0 and cout % 32 == 0
                assert ops.wgrad_covers(H, W, cin, cout) == want, (H, W, cin, cout)
    before = ops.wgrad_covers.cache_info()
    assert ops.wgrad_covers(8, 32, 32, 32) and not ops.wgrad_covers(8, 48, 32, 32)
    after = ops.wgrad_covers.cache_info()
    assert (after.hits, after.misses) == (before.hits + 2, before.misses)              # asked once per key, a refusal included


def test_the_covered_set_follows_no_library_switch(tune):
    """Why covers keeps a boolean without an invalidation hook: every library switch at 0, 1, 2 and 4 leaves the covered set of 13 forms x 81
    extents as it is at the defaults (the switches choose AMONG the kernels of a family; which extents the family tiles is not theirs)."""
    from v2x_sim_amd import ops, tuning
    forms = dict(R.FORMS, **R.MORE_FORMS)
    extents = R.EXTENTS[::2]
    pcs = [packed(**f) for f in forms.values()]
    assert len(pcs) == 13 and len(extents) == 9

    def table():
        for pc in pcs:
            pc.covered.clear()
        return [ops.covers(pc, H, W) for pc in pcs for H in extents for W in extents]

    base = table()
    assert any(base) and not all(base)
    for pc, form in zip(pcs, forms.values()):
        assert any(ops.covers(pc, H, W) for H in extents for W in extents), form       # every form of the table is one the library knows
    for name in tuning.LIBRARY_SWITCHES:
        for v in (0, 1, 2, 4):
            tune(name, v)
            assert table() == base, (name, v)
        tune.reset(name)


def test_covers_asks_the_library_once_per_key(monkeypatch):
    from v2x_sim_amd import _lib, ops
    lib = _lib.load()
    calls, real = [], lib.v2x_conv2d_plan

    def counted(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(lib, "v2x_conv2d_plan", counted)
    pc = packed(**R.FORMS["halo 64->64"])
    assert ops.covers(pc, 16, 32) and len(calls) == 1
    assert ops.covers(pc, 16, 32) and len(calls) == 1
    assert not ops.covers(pc, 16, 1664) and len(calls) == 2                 # refused (the DMA tables): memoised all the same
    assert not ops.covers(pc, 16, 1664) and len(calls) == 2
    assert not ops.covers(pc, 16, 32, bits=True) and len(calls) == 3        # `bits` is part of the key (the bit grid is the 32 -> 32 layer's)
    assert ops.covers(pc, 16, 32) and len(calls) == 3
    assert pc.covered == {(16, 32, False): True, (16, 1664, False): False, (16, 32, True): False}
    other = packed(**R.FORMS["halo 64->64"])
    assert ops.covers(other, 16, 32) and len(calls) == 4                    # the memo is the packing's own


def test_a_refusal_is_not_the_next_failures_text():
    """covers' refused question leaves its text in v2x_last_error; a later failing call reports its own."""
    from v2x_sim_amd import _lib, ops
    assert not ops.covers(packed(**R.FORMS["halo 64->64"]), 16, 1664)
    with pytest.raises(_lib.V2XLibraryError, match="not tileable"):
        ops.conv_kernel_name(packed(**R.FORMS["stream 128->128"]), 7, 32)


def test_the_wide_fused_training_layer_gives_way():
    """upcat_conv3x3's fused form (forward 64 + 32 -> 32, data gradients 32 -> 64 and 32 -> 32 on the halo kernels) at the full-resolution extent:
    covered to W = 1632, refused from 1664 (the forward form's 64-channel source) -- where the retired rule said yes and the launch was refused."""
    from v2x_sim_amd.train import hip_graph
    assert hip_graph.upcat_conv_covered(8, 1600) and hip_graph.upcat_conv_covered(8, 1632) and hip_graph.upcat_conv_covered(256, 256)
    assert not hip_graph.upcat_conv_covered(8, 1664) and not hip_graph.upcat_conv_covered(8, 3296)
    assert R.upcat_conv_rule_was(8, 1664) and R.upcat_conv_rule_was(8, 3296)
    assert not hip_graph.upcat_conv_covered(12, 64) and not hip_graph.upcat_conv_covered(8, 48)
    from v2x_sim_amd import ops, packing
    fwd, d_a, d_b = (packing.halo_conv_shape("t", 32, 96, c_up, rows)[0] for c_up, rows in ((64, None), (0, (0, 64)), (0, (64, 32))))
    assert (fwd.C0, fwd.C1, fwd.up0, fwd.Cout) == (64, 32, 1, 32) and (d_a.C0, d_a.C1, d_a.Cout) == (32, 0, 64) and (d_b.C0, d_b.C1, d_b.Cout) == (32, 0, 32)
    assert ops.covers(fwd, 8, 1632) and not ops.covers(fwd, 8, 1664)
    assert ops.covers(d_a, 8, 3264) and not ops.covers(d_a, 8, 3296) and not ops.covers(d_b, 8, 3296)     # the 32-channel data-gradient forms


def test_no_second_copy_of_the_extent_rules_is_left():
    from v2x_sim_amd import ops
    from v2x_sim_amd.train import hip_graph
    for fn in (ops.select, ops.run_layer, hip_graph.hip_eligible, hip_graph.upcat_conv3x3):
        src = inspect.getsource(fn)
        for rule in ("% 8", "% 16", "% 32", "% 64"):
            assert rule not in src, (fn.__name__, rule)
    assert "covers(" in inspect.getsource(ops.select) and "select(" in inspect.getsource(ops.run_layer)
    assert not hasattr(ops, "halo_eligible") and not hasattr(hip_graph, "_layer_runs")
    # conv_kernel_name and covers fill ONE descriptor: the same helper, and no field assignment of their own but the latency declaration
    for fn in (ops.conv_kernel_name, ops.covers):
        assert "_plan_desc(" in inspect.getsource(fn) and "ConvDesc" not in inspect.getsource(fn)

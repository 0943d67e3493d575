"""The ConvGRU's streamed kernel (csrc/conv_stream.hip: conv3x3_stream8g_kernel<96, 2, *>) after its load phase was rewritten for the 96-row
form (unrolled tap columns, hoisted lane constants, scalar weight addresses): the same DMAs, the same reads, the same K order, so every
output BIT is what the previous kernel produced.

tests/golden/gru_stream_bits.json holds the SHA-256 of the bf16 output bytes of every case, recorded once on the GPU from a build of the commit
before the rewrite (names and hashes only; the operands are drawn by tests/conv_refs.py::_draw from the case's seed).  Each case is also held
to the float64 oracle cell (conv_refs.gru_ref) with the tolerance tests/test_gpu_stream.py uses for the ConvGRU (atol = rtol = 2**-7), so a
wrong golden cannot hide.  Every case runs through the public entry (packing.pack_gru_stream + ops.run_layer) with operands, parameters and
the output between poisoned guard regions (tests/guarded_alloc.py), as tests/test_gpu_memory_contract.py does.

Cases, the smallest that reach each path of the kernel:
  a  32 + 32 -> 3 x 32 channels, N = 1, 32 x 32   two chunks, six steps per tile: the weight stream wraps into the next tile inside its first two steps
  b  256 + 256 -> 3 x 256, N = 2, 32 x 32         the bench's channel counts, 8 channel tiles (the GRU_XCD_WALK branch is off at this grid)
  c  32 + 32 -> 3 x 32, N = 130, 32 x 32          260 tiles on a 256-workgroup grid: four workgroups take a second tile, the rest stop
                                                  (has_next both ways, the relaxed wait after an epilogue)
  d  32 + 32 -> 3 x 32, N = 1, 48 x 64            tiles away from and on every image border: the zero page of the patch descriptors
  e  STREAM_WT = 2 on (a) and (b)                 the wave-tiled instantiation: the same bits as the plain one"""
import functools
import hashlib
import json
import os

import pytest
import torch

import conv_refs as R
import guarded_alloc as G

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "gru_stream_bits.json")

# name -> (C0, C1, hidden, N, H, W, maps held to the float64 reference)
CASES = {
    "a": (32, 32, 32, 1, 32, 32, [0]),
    "b": (256, 256, 256, 2, 32, 32, [0, 1]),
    "c": (32, 32, 32, 130, 32, 32, [0, 127, 128, 129]),      # maps 128 and 129 are the four second tiles (two 16 x 32 tiles per map)
    "d": (32, 32, 32, 1, 48, 64, [0]),
}
RUNS = [("a", 0), ("b", 0), ("c", 0), ("d", 0), ("a", 2), ("b", 2)]     # (case, STREAM_WT); 0 = the library's default tiling for the ConvGRU


@functools.lru_cache(maxsize=None)
def built(name):
    """Operands and the float64 reference of a case, drawn once and shared by the runs that use it (never modified)."""
    C0, C1, hid, N, H, W, maps = CASES[name]
    c = R.ConvCase(9000 + sorted(CASES).index(name), "gru_load_phase_" + name, {}, dict(w_layout=2, C0=C0, C1=C1, Cout=hid, epilogue=R.GRU, N=N, H=H, W=W), None, "")
    b = R._draw(c, "rand", 0)
    b.ref = R.gru_ref(b, maps)
    return b


def nhwc(x, dev):
    return x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(dev)


def guard_pc(pc, h):
    """The packed layer with its parameter tensors between guards (as tests/test_gpu_memory_contract.py::_guard_pc)."""
    from v2x_sim_amd import ops
    q = ops.PackedConv(**{k: getattr(pc, k) for k in ops.PackedConv.__slots__ if k != "covered"})
    for k in ("weight", "scale", "shift", "weight2", "scale2", "shift2"):
        setattr(q, k, h.guarded(getattr(pc, k)))
    return q


def run_case(name, dev, h):
    """-> the ConvGRU's output (N, H, W, hidden) bf16 through packing.pack_gru_stream + ops.run_layer, everything the kernel touches guarded by h."""
    from v2x_sim_amd import ops
    b = built(name)
    pc = guard_pc(b.pack(dev), h)
    out = ops.run_layer(ops.Layer([pc], halo=pc), h.guarded(nhwc(b.x0, dev)), h.guarded(nhwc(b.x1, dev)))
    torch.cuda.synchronize()
    return out


def sha(t):
    return hashlib.sha256(t.contiguous().view(torch.int16).cpu().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("name,wt", RUNS, ids=["%s-wt%d" % r for r in RUNS])
def test_gru_stream_bits_are_the_previous_kernels(device, tune, name, wt):
    from v2x_sim_amd import ops
    C0, C1, hid, N, H, W, maps = CASES[name]
    b = built(name)
    if wt:
        tune("STREAM_WT", wt)
    assert ops.conv_kernel_name(b.pack(device), H, W, False, N) == "conv3x3_stream8g_kernel<96, 2, %s>" % ("true" if wt else "false")
    plain = run_case(name, device, G.PlainAlloc())
    assert plain.shape == (N, H, W, hid) and plain.dtype == torch.bfloat16
    # the float64 oracle, with the ConvGRU's tolerance of tests/test_gpu_stream.py
    got = plain[maps].float().permute(0, 3, 1, 2).cpu().double()
    err = float((got - b.ref).abs().max())
    print("case %s wt %d: max |out - float64 reference| = %.3g" % (name, wt, err))
    assert torch.allclose(got, b.ref, atol=2 ** -7, rtol=2 ** -7), err
    # bit for bit the previous kernel (the wave-tiled form: the same golden as the plain one)
    want = json.load(open(GOLDEN))["cases"][name]
    assert sha(plain) == want, "case %s: the output bits differ from the recorded ones" % name
    # between guard regions: nothing outside is written, no input is written, and the bits do not depend on what lies around the buffers
    for poison in G.POISONS:
        with G.GuardedAlloc(poison) as h:
            out = run_case(name, device, h)
            assert h.records
            h.check_guards()
            h.check_operands_unchanged(written=[out])
            assert G.same_bits(out, plain), "case %s under poison 0x%02X differs from the plain run" % (name, poison)

"""v2x_conv2d_plan: the library names the kernel(s) v2x_conv2d would launch for a descriptor, from the code path that launches them (csrc/common.h:
v2x_launch in plan mode records the kernel's own symbol instead of launching).  No GPU: nothing is launched and no tensor pointer is read.
  * a table of descriptors that reaches every `return launch_...` of the four dispatch functions (conv_halo / conv_stream / conv_stream_s2 / conv1x1) and of
    v2x_conv2d's gather tail, each with the name it must produce written out;
  * a rejected shape gets the same code and the same v2x_last_error text from the plan entry as from v2x_conv2d;
  * every name the table produces is a kernel of the library's gfx950 code object;
  * the kernel names bench.py's tables are keyed by (FETCH_FACTOR, the stream-ceiling mixes) are names the library produces."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/llvm/bin"
PTR = 0x1000      # every tensor pointer of the table: non-null, 16-byte aligned, never dereferenced
BF16, F32, GRU, DET = 0, 1, 2, 3


def desc(**kw):
    """A v2x_conv_desc: 3x3 stride 1 pad 1, one map, plain bf16 epilogue unless the row says otherwise; w_rows / w_kpad / out_cstride as the packers would set them."""
    from v2x_sim_amd import _lib
    d = _lib.ConvDesc()
    f = dict(N=1, ksize=3, stride=1, pad=1, C1=0, up0=0, epilogue=BF16, relu=1, w_layout=0, Cout2=0)
    f.update(kw)
    lay, cin = f["w_layout"], f["C0"] + f["C1"]
    if "w_rows" not in f:
        need = 3 * f["Cout"] if f["epilogue"] == GRU else f["Cout"]
        rows = _lib.load().v2x_conv_tile_rows(f["Cout"], f["epilogue"]) if lay == 0 else 1
        f["w_rows"] = (need + rows - 1) // rows * rows
    if "w_kpad" not in f:
        f["w_kpad"] = (16 * f["C0"] + 9 * f["C1"]) if lay in (3, 4) else ((f["ksize"] ** 2 * cin + 63) // 64 * 64 if lay == 0 else 9 * cin)
    f.setdefault("out_cstride", f["Cout2"] or f["Cout"])
    for k in ("in0", "weight", "scale", "shift", "out"):
        f.setdefault(k, PTR)
    if f["C1"]:
        f.setdefault("in1", PTR)
    if f["Cout2"]:
        for k in ("weight2", "scale2", "shift2"):
            f.setdefault(k, PTR)
    if f.get("splitk", 0) > 1:
        f.setdefault("splitk_ws", PTR)
    if f["epilogue"] == DET:
        f.update(out2=PTR, out2_cstride=6, det_counts=PTR, det_cap=4096, det_thr=0.5, out_cstride=4096)
    for k, v in f.items():
        setattr(d, k, v)
    return d


def S(**kw):   # streamed layout
    return dict(w_layout=2, **kw)


def H(**kw):   # halo layout
    return dict(w_layout=1, **kw)


REDUCE, REDUCE_GRU = " + splitk_reduce_kernel<false>", " + splitk_reduce_kernel<true>"
# (expected name, switches, descriptor).  Rows marked DRIFT are the cases the retired Python copy of this dispatch got wrong.
TABLE = [
    # ---- conv_stream.hip: v2x_conv_stream_dispatch ------------------------------------------------------------------------------
    ("conv3x3_stream8q_kernel", {}, dict(w_layout=4, C0=128, C1=64, up0=1, Cout=64, H=16, W=64)),
    ("conv3x3_stream8p_kernel", {}, dict(w_layout=4, C0=256, C1=128, up0=1, Cout=128, H=16, W=32)),
    ("conv3x3_stream_kernel<96, 16, 16, 0, true>" + REDUCE_GRU, {}, S(C0=64, Cout=32, epilogue=GRU, H=16, W=16, splitk=2)),        # DRIFT (split-K labels)
    ("conv3x3_stream_kernel<96, 8, 32, 0, true>" + REDUCE_GRU, {}, S(C0=32, C1=32, Cout=64, epilogue=GRU, H=8, W=32, splitk=2)),
    ("conv3x3_stream_kernel<128, 16, 16, 0, true>" + REDUCE, {}, S(C0=128, Cout=128, H=16, W=16, splitk=4)),
    ("conv3x3_stream_kernel<128, 8, 32, 0, true>" + REDUCE, {}, S(C0=64, Cout=256, H=16, W=32, splitk=2)),
    ("conv3x3_stream_kernel<64, 16, 16, 0, true>" + REDUCE, {}, S(C0=64, Cout=64, H=16, W=16, splitk=2)),
    ("conv3x3_stream_kernel<64, 8, 32, 0, true>" + REDUCE, {}, S(C0=96, Cout=64, H=16, W=32, splitk=3)),
    ("conv3x3_stream8g_kernel<128, 0, true>", {}, S(C0=256, Cout=256, H=32, W=32, N=3)),
    ("conv3x3_stream8g_kernel<96, 2, true>", {"STREAM_WT": 2}, S(C0=256, C1=256, Cout=256, epilogue=GRU, H=32, W=32)),
    ("conv3x3_stream8g_kernel<96, 2, false>", {}, S(C0=256, C1=256, Cout=256, epilogue=GRU, H=32, W=32)),
    ("conv3x3_stream8_kernel<96, 2>", {"STREAM_G": 0}, S(C0=256, C1=256, Cout=256, epilogue=GRU, H=32, W=32)),
    ("conv3x3_stream8_kernel<96, 2>", {}, S(C0=32, Cout=32 * 257, epilogue=GRU, H=16, W=32)),          # DRIFT: three taps need n_co_tiles <= CUs
    ("conv3x3_stream8_kernel<128, 1>", {}, S(C0=128, Cout=128, Cout2=128, H=64, W=64, N=24)),            # chained, 192 tiles: a full launch
    ("conv3x3_stream_kernel<128, 8, 32, 1, false>", {}, S(C0=128, Cout=128, Cout2=128, H=64, W=64, N=5)),  # DRIFT: few_chain_tiles (160 x 4 < 3 x 256)
    ("conv3x3_stream8g_kernel<128, 0, false>", {"STREAM_WT": 0}, S(C0=128, Cout=128, H=16, W=32)),
    ("conv3x3_stream8_kernel<128, 0>", {"STREAM_G": 0}, S(C0=128, Cout=128, H=16, W=32)),
    ("conv3x3_stream8_kernel<128, 0>", {}, S(C0=32, Cout=128 * 257, H=16, W=32)),                        # DRIFT: n_co_tiles > CUs
    ("conv3x3_wide3_kernel<64>", {}, S(C0=128, C1=64, up0=1, Cout=64, H=32, W=64)),
    ("conv3x3_wide_kernel<64, 1>", {}, S(C0=64, Cout=64, Cout2=64, H=32, W=32)),
    ("conv3x3_wide_kernel<64, 0>", {}, S(C0=64, Cout=64, H=16, W=32)),
    ("conv3x3_wide_kernel<64, 0>", {"WIDE3": 0}, S(C0=128, C1=64, up0=1, Cout=64, H=32, W=64)),
    ("conv3x3_stream_kernel<128, 16, 16, 1, false>", {}, S(C0=128, Cout=128, Cout2=128, H=16, W=16)),
    ("conv3x3_stream_kernel<128, 8, 32, 1, false>", {}, S(C0=128, Cout=128, Cout2=128, H=8, W=32)),
    ("conv3x3_stream_kernel<64, 16, 16, 1, false>", {}, S(C0=64, Cout=64, Cout2=64, H=16, W=16)),
    ("conv3x3_stream_kernel<64, 8, 32, 1, false>", {}, S(C0=64, Cout=64, Cout2=64, H=8, W=32)),
    ("conv3x3_stream_kernel<96, 16, 16, 2, false>", {}, S(C0=256, C1=256, Cout=256, epilogue=GRU, H=16, W=16)),
    ("conv3x3_stream_kernel<96, 8, 32, 2, false>", {}, S(C0=256, C1=256, Cout=256, epilogue=GRU, H=8, W=32)),
    ("conv3x3_stream_kernel<128, 16, 16, 0, false>", {}, S(C0=512, Cout=512, H=16, W=16, N=2)),
    ("conv3x3_stream_kernel<128, 8, 32, 0, false>", {"STREAM_WAVES": 4}, S(C0=128, Cout=128, H=16, W=32)),
    ("conv3x3_stream_kernel<64, 16, 16, 0, false>", {}, S(C0=64, Cout=64, H=16, W=16)),
    ("conv3x3_stream_kernel<64, 8, 32, 0, false>", {"STREAM_WIDE": 0}, S(C0=128, C1=64, up0=1, Cout=64, H=16, W=32)),
    # ---- conv_stream_s2.hip: v2x_conv_stream_s2_dispatch ------------------------------------------------------------------------
    ("conv3x3_s2_stream_kernel<128, 8, 16, true>" + REDUCE, {}, S(stride=2, C0=256, Cout=512, H=32, W=32, splitk=4)),               # DRIFT (split-K labels)
    ("conv3x3_s2_stream_kernel<64, 8, 16, true>" + REDUCE, {}, S(stride=2, C0=64, Cout=64, H=16, W=32, splitk=2)),
    ("conv3x3_s2_stream_kernel<128, 4, 32, true>" + REDUCE, {}, S(stride=2, C0=64, Cout=128, H=24, W=128, splitk=2)),
    ("conv3x3_s2_stream_kernel<64, 4, 32, true>" + REDUCE, {}, S(stride=2, C0=64, Cout=64, H=8, W=64, splitk=2)),
    ("conv3x3_s2g_kernel<8, 32>", {}, S(stride=2, C0=64, Cout=128, H=32, W=128, N=2)),
    ("conv3x3_s2g_kernel<16, 16>", {}, S(stride=2, C0=256, Cout=512, H=32, W=32, N=2)),
    ("conv3x3_s2_stream_kernel<128, 4, 32, false>", {}, S(stride=2, C0=64, Cout=128, H=128, W=128, N=8, small_batch=1)),  # DRIFT: the fourth template argument
    ("conv3x3_s2_stream_kernel<128, 4, 32, false>", {"S2_G": 0}, S(stride=2, C0=64, Cout=128, H=32, W=128)),
    ("conv3x3_s2_stream_kernel<128, 8, 16, false>", {}, S(stride=2, C0=128, Cout=128, H=16, W=32)),
    ("conv3x3_s2_stream_kernel<64, 8, 16, false>", {}, S(stride=2, C0=32, Cout=64, H=32, W=32)),       # DRIFT: the 16 x 16 test comes before the resident-weights test
    ("conv3x3_s2_resident_kernel<64>", {}, S(stride=2, C0=32, Cout=64, H=16, W=64, N=3)),
    ("conv3x3_s2_stream_kernel<128, 4, 32, false>", {}, S(stride=2, C0=32, Cout=128, H=8, W=64)),
    ("conv3x3_s2_stream_kernel<64, 4, 32, false>", {}, S(stride=2, C0=64, Cout=64, H=8, W=64)),
    # ---- conv_halo.hip: v2x_conv_halo_dispatch ----------------------------------------------------------------------------------
    ("conv3x3_halo_sb_kernel<0, 32, 32, 0, 0, true>", {}, H(C0=32, Cout=32, H=8, W=32, in_format=1, in_zbits=13)),
    ("conv3x3_halo_sb_kernel<0, 32, 32, 0, 0, false>", {}, H(C0=32, Cout=32, H=8, W=32)),
    ("conv3x3_halo_ppc_kernel<64, 32, 32>", {}, dict(w_layout=3, C0=64, C1=32, up0=1, Cout=32, H=24, W=32, N=3)),
    ("conv3x3_halo_pp_kernel<64, 32, 32, 0>", {}, H(C0=64, C1=32, up0=1, Cout=32, H=16, W=32)),
    ("conv3x3_halo_kernel<64, 32, 32, 0, 0>", {}, H(C0=64, C1=32, up0=1, Cout=32, H=24, W=32, N=3)),   # DRIFT: conv8_1, odd tile count
    ("conv3x3_halo_kernel<64, 32, 32, 0, 0>", {"HALO_PP": 0}, H(C0=64, C1=32, up0=1, Cout=32, H=16, W=32)),
    ("conv3x3_halo_pp_kernel<0, 64, 64, 0>", {}, H(C0=64, Cout=64, H=16, W=32)),
    ("conv3x3_halo_kernel<0, 64, 64, 0, 0>", {}, H(C0=64, Cout=64, H=40, W=96, N=3)),                   # DRIFT: conv7_2, odd tile count
    ("conv3x3_halo_pp_kernel<0, 64, 64, 64>", {}, H(C0=64, Cout=64, Cout2=64, H=24, W=32, N=4)),
    ("conv3x3_halo_kernel<0, 64, 64, 64, 1>", {}, H(C0=64, Cout=64, Cout2=64, H=24, W=32, N=3)),        # DRIFT: the chained layer, odd tile count
    ("conv3x3_halo_kernel<0, 64, 32, 0, 0>", {}, H(C0=64, Cout=32, H=8, W=32)),
    ("conv3x3_halo_kernel<0, 32, 64, 0, 0>", {}, H(C0=32, Cout=64, H=8, W=32)),
    ("conv3x3_halo_kernel<0, 32, 64, 48, 2>", {}, H(C0=32, Cout=64, Cout2=48, epilogue=F32, H=8, W=32)),
    ("conv3x3_halo_kernel<0, 32, 32, 16, 2>", {}, H(C0=32, Cout=32, Cout2=8, epilogue=F32, H=8, W=32)),
    ("conv3x3_halo_kernel<0, 32, 64, 64, 3>", {}, H(C0=32, Cout=64, Cout2=64, epilogue=DET, H=8, W=32)),   # DRIFT: the DET epilogue
    # ---- conv1x1.hip: v2x_conv1x1_dispatch (every channel-tile count, every chunk count, both epilogues) --------------------------
    ("conv1x1_stream_kernel<1, 1, false, 4>", {}, dict(ksize=1, pad=0, C0=32, Cout=16, H=8, W=8)),
    ("conv1x1_stream_kernel<2, 2, true, 4>", {}, dict(ksize=1, pad=0, C0=64, Cout=32, epilogue=F32, H=8, W=8)),
    ("conv1x1_stream_kernel<4, 3, false, 4>", {}, dict(ksize=1, pad=0, C0=128, Cout=48, H=8, W=8)),
    ("conv1x1_stream_kernel<1, 4, true, 4>", {}, dict(ksize=1, pad=0, C0=32, Cout=64, epilogue=F32, H=8, W=8)),
    ("conv1x1_stream_kernel<2, 6, false, 4>", {}, dict(ksize=1, pad=0, C0=64, Cout=96, H=8, W=8)),
    ("conv1x1_stream_kernel<4, 8, false, 2>", {}, dict(ksize=1, pad=0, C0=128, Cout=128, H=8, W=8)),
    ("conv1x1_stream_kernel<2, 8, true, 2>", {}, dict(ksize=1, pad=0, C0=64, Cout=128, epilogue=F32, H=8, W=8)),
    ("conv1x1_stream_kernel<1, 1, true, 4>", {}, dict(ksize=1, pad=0, C0=32, Cout=4, epilogue=F32, H=8, W=8)),
    ("conv1x1_stream_kernel<4, 4, true, 2>", {}, dict(ksize=1, pad=0, C0=128, Cout=64, epilogue=F32, H=8, W=8)),
    # ---- conv_igemm.hip: the gather tail of v2x_conv2d --------------------------------------------------------------------------
    ("conv_igemm_kernel<96, 128, 2, 2, 2>", {}, dict(C0=64, C1=64, Cout=64, epilogue=GRU, H=8, W=8)),
    ("conv_igemm_kernel<32, 256, 1, 4, 1>", {}, dict(C0=32, Cout=12, epilogue=F32, H=8, W=8)),
    ("conv_igemm_kernel<48, 256, 1, 4, 1>", {}, dict(C0=32, Cout=48, epilogue=F32, H=8, W=8)),
    ("conv_igemm_kernel<64, 128, 2, 2, 1>", {}, dict(C0=32, Cout=64, epilogue=F32, H=8, W=8)),
    ("conv_igemm_kernel<128, 128, 2, 2, 1>", {}, dict(C0=32, Cout=96, epilogue=F32, H=8, W=8)),
    ("conv_igemm_kernel<32, 256, 1, 4, 0>", {}, dict(C0=16, Cout=32, stride=2, H=9, W=7)),
    ("conv_igemm_kernel<48, 256, 1, 4, 0>", {}, dict(C0=32, Cout=40, H=8, W=8)),
    ("conv_igemm_kernel<64, 128, 2, 2, 0>", {}, dict(C0=64, C1=32, up0=1, Cout=64, H=8, W=8)),
    ("conv_igemm_kernel<128, 128, 2, 2, 0>", {}, dict(C0=32, Cout=256, H=8, W=8)),
    ("conv_igemm_kernel<64, 128, 2, 2, 0>", {"CONV1X1": 0}, dict(ksize=1, pad=0, C0=64, Cout=64, H=8, W=8)),
    ("conv_igemm_kernel<128, 128, 2, 2, 0>", {}, dict(ksize=1, pad=0, C0=96, Cout=128, H=8, W=8)),      # three chunks: not a shape of the streaming 1x1 kernel
]

# shapes v2x_conv2d refuses: by its validation, and by each dispatch function's "not mine"
REJECTED = [
    S(C0=128, Cout=128, H=7, W=32),                          # not tileable
    S(C0=128, Cout=128, H=16, W=32, splitk=8),               # more splits than chunks
    S(C0=48, Cout=128, H=16, W=32),                          # C0 % 32
    S(C0=128, Cout=96, H=16, W=32),                          # no row tile for this Cout
    S(stride=2, C0=64, Cout=128, H=8, W=48),                 # stride 2: no tiling
    S(stride=2, C0=64, C1=64, Cout=128, H=8, W=64),          # stride 2: one source only
    H(C0=96, Cout=32, H=8, W=32),                            # no halo instantiation
    H(C0=32, Cout=32, H=12, W=32),                           # H % 8
    H(C0=64, Cout=64, H=8, W=32, in_format=1, in_zbits=13),  # bit-grid input exists for 32 -> 32 only
    dict(w_layout=3, C0=128, C1=32, up0=1, Cout=32, H=8, W=32),
    dict(w_layout=4, C0=128, C1=64, up0=1, Cout=64, H=16, W=32),
    dict(C0=12, Cout=32, H=8, W=8),                          # gather: C0 % 8
    dict(C0=32, Cout=32, H=8, W=8, w_kpad=100),
    dict(C0=32, Cout=32, H=4096, W=4096),                    # 24-bit row arithmetic
    dict(C0=32, Cout=32, H=8, W=8, epilogue=DET),
]


def _plan(lib, d, cap=512):
    buf = C.create_string_buffer(cap)
    rc = lib.v2x_conv2d_plan(C.byref(d), buf, cap)
    return rc, buf.value.decode(), lib.v2x_last_error().decode()


@pytest.fixture(scope="module")
def planned():
    """The table run once: [(expected, got rc, got name)]; switches set per row and put back."""
    from v2x_sim_amd import _lib, tuning
    lib = _lib.load()
    out = []
    for expected, switches, fields in TABLE:
        old = {k: tuning.set(k, v) for k, v in switches.items()}
        try:
            rc, name, err = _plan(lib, desc(**fields))
        finally:
            for k, v in old.items():
                tuning.set(k, v)
        out.append((expected, rc, name, err))
    return out


def test_every_dispatch_return_names_its_kernel(planned):
    wrong = [(e, rc, n, err) for e, rc, n, err in planned if rc != 0 or n != e]
    assert not wrong, wrong
    # the table reaches every launch function of the five files: each kernel family and each template form of it appears
    families = {n.split("<")[0] for _, _, name, _ in planned for n in name.split(" + ")}
    assert families == {"conv3x3_stream8q_kernel", "conv3x3_stream8p_kernel", "conv3x3_stream_kernel", "splitk_reduce_kernel", "conv3x3_stream8g_kernel",
                        "conv3x3_stream8_kernel", "conv3x3_wide3_kernel", "conv3x3_wide_kernel", "conv3x3_s2_stream_kernel", "conv3x3_s2g_kernel",
                        "conv3x3_s2_resident_kernel", "conv3x3_halo_sb_kernel", "conv3x3_halo_ppc_kernel", "conv3x3_halo_pp_kernel", "conv3x3_halo_kernel",
                        "conv1x1_stream_kernel", "conv_igemm_kernel"}


def test_plan_mode_is_per_call_and_bounded():
    from v2x_sim_amd import _lib
    lib = _lib.load()
    d = desc(**S(C0=64, Cout=256, H=16, W=32, splitk=2))
    full = "conv3x3_stream_kernel<128, 8, 32, 0, true>" + REDUCE
    assert _plan(lib, d)[:2] == (0, full)
    assert _plan(lib, d, len(full) + 1)[:2] == (0, full)                       # the terminating NUL is the last byte
    rc, _, err = _plan(lib, d, len(full))
    assert rc == -22 and "do not fit" in err
    assert lib.v2x_conv2d_plan(C.byref(d), None, 0) == -22
    assert lib.v2x_conv2d_plan(None, C.create_string_buffer(8), 8) == -22 and b"null descriptor" in lib.v2x_last_error()
    assert _plan(lib, d)[:2] == (0, full)                                      # a failed call leaves no sink behind


@pytest.mark.parametrize("i", range(len(REJECTED)))
def test_rejected_shapes_get_the_launch_entrys_code_and_text(i):
    from v2x_sim_amd import _lib
    lib = _lib.load()
    d = desc(**REJECTED[i])
    rc, name, err = _plan(lib, d)
    # (only a descriptor the plan refused BEFORE any kernel was chosen goes to the launching entry: it stops at the same line)
    assert rc == -22 and name == "" and err, (rc, name, err)
    assert lib.v2x_conv2d(C.byref(d), None) == rc
    assert lib.v2x_last_error().decode() == err


def _device_kernels(tmp_path):
    """Demangled names (argument list cut) of the function symbols of the gfx950 code objects inside the built library."""
    from v2x_sim_amd import _lib
    import bench
    os.symlink(_lib.LIB_PATH, str(tmp_path / "lib.so"))
    subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=str(tmp_path), stdout=subprocess.DEVNULL)
    objs = sorted(f for f in os.listdir(str(tmp_path)) if f.endswith("gfx950"))
    assert objs
    syms = set()
    for f in objs:
        for ln in subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-s", "--wide", f], cwd=str(tmp_path), capture_output=True, text=True, check=True).stdout.splitlines():
            p = ln.split()
            if len(p) == 8 and p[3] == "FUNC":
                syms.add(p[7])
    dem = subprocess.run(["c++filt"], input="\n".join(sorted(syms)), capture_output=True, text=True, check=True).stdout.splitlines()
    return {bench.strip_kernel_args(n) for n in dem}


def test_every_planned_name_is_a_kernel_of_the_device_code(planned, tmp_path):
    kernels = _device_kernels(tmp_path)
    assert len(kernels) > 100
    names = {n for _, _, name, _ in planned for n in name.split(" + ")}
    assert names and not (names - kernels), sorted(names - kernels)


def test_the_benchmarks_tables_are_keyed_by_names_the_library_produces(planned):
    import bench

    class Asked(dict):     # stream_ceiling_fractions asks `k in kernels` for every key of its mixes table (if it ever iterates another way, this harvest --
                           # and the len() guard below -- fails and must follow it)
        def __contains__(self, k):
            self[k] = None
            return False

    asked = Asked()
    bench.stream_ceiling_fractions(asked, {})
    mixes = set(dict.keys(asked)) - {"conv3x3_tail_kernel"}           # (the fused tail is v2x_conv2d_pair's kernel)
    assert len(mixes) >= 4
    names = {n for _, _, name, _ in planned for n in name.split(" + ")}
    assert set(bench.FETCH_FACTOR) <= names, set(bench.FETCH_FACTOR) - names
    assert mixes <= names, mixes - names


def test_conv_kernel_name_is_the_librarys_answer():
    """ops.conv_kernel_name fills a descriptor from the packed layer (placeholders for the activations) and asks the library: no second dispatch in
    Python, and a declared latency launch reaches the descriptor."""
    import inspect
    import torch
    from v2x_sim_amd import ops
    src = inspect.getsource(ops.conv_kernel_name)
    assert "conv_plan" in src and "tuning.get" not in src
    w, ss = torch.zeros(64, dtype=torch.bfloat16), torch.zeros(128)
    pc = ops.PackedConv(name="t", weight=w, scale=ss, shift=ss, C0=64, C1=0, up0=0, Cout=128, ksize=3, stride=2, pad=1, epilogue=BF16, relu=True, w_rows=128,
                        w_kpad=576, w_layout=2)
    assert ops.conv_kernel_name(pc, 128, 128, N=8) == "conv3x3_s2g_kernel<8, 32>"
    with ops.latency_dispatch():
        assert ops.conv_kernel_name(pc, 128, 128, N=8) == "conv3x3_s2_stream_kernel<128, 4, 32, false>"
        assert ops.conv_kernel_name(pc, 128, 128, N=64) == "conv3x3_s2g_kernel<8, 32>"
    pc.stride, pc.Cout2, pc.weight2, pc.scale2, pc.shift2, pc.relu2, pc.C0 = 1, 128, w, ss, ss, True, 128
    assert ops.conv_kernel_name(pc, 64, 64, N=24) == "conv3x3_stream8_kernel<128, 1>"
    with pytest.raises(Exception, match="not tileable"):
        ops.conv_kernel_name(pc, 7, 32)

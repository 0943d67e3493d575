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

from conv_refs import BF16, REDUCE, REJECTED, TABLE, S, desc     # the table lives in tests/conv_refs.py: the GPU sweep runs every row of it

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/llvm/bin"


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

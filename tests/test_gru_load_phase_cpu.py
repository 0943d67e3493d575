"""The 96-row instantiations of conv3x3_stream8g_kernel (the ConvGRU) unroll their tap-column loop and hoist lane constants into the registers the
96-row form has spare.  A spill would put scratch traffic into the kernel's counted vmcnt protocol, so the resources are held here, on the CPU:
csrc/conv_stream.hip is cross-compiled for gfx950 as tools/isa_stats.py does, and the code object's metadata (nothing else) must say, for
<96, 2, false> and <96, 2, true>:
  * a private segment of 0 bytes (no scratch) and no spilled VGPR;
  * at most 256 VGPRs (two waves per SIMD: __launch_bounds__(512), amdgpu_waves_per_eu(2, 2));
  * no static LDS: the whole group segment is the dynamic size the launcher passes, launch_stream8g's 3 x 3 x 96 x 64 (ring) + 2 x 40 KiB
    (patches) + 1 KiB (epilogue parameters) = 135 KiB of the 160 KiB, which the metadata cannot hold and which is therefore recomputed here."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "v2x-sim_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ["_Z23conv3x3_stream8g_kernelILi96ELi2ELb0EEv10StreamArgs", "_Z23conv3x3_stream8g_kernelILi96ELi2ELb1EEv10StreamArgs"]


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """{mangled kernel name: {metadata key: int}} of conv_stream.hip's gfx950 code object."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("gru_lp") / "conv_stream.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", os.path.join(CSRC, "conv_stream.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    notes = text[text.index("amdhsa.kernels:"):]
    md = {}
    for entry in re.split(r"\n  - ", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry)
        if name:
            md[name.group(1)] = {k: int(v) for k, v in re.findall(r"^\s*\.(\w+):\s+(\d+)\s*$", entry, flags=re.M)}
    return md


@pytest.mark.parametrize("kernel", KERNELS)
def test_96_row_stream8g_resources(metadata, kernel):
    assert kernel in metadata, sorted(k for k in metadata if "stream8g" in k)
    m = metadata[kernel]
    print(kernel, {k: m[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")})
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0
    assert m["vgpr_count"] + m.get("agpr_count", 0) <= 256 and m["vgpr_count"] <= 256
    assert m["max_flat_workgroup_size"] == 512
    assert m["group_segment_fixed_size"] == 0                       # all of its LDS is the launcher's dynamic size:
    assert 3 * 3 * 96 * 64 + 2 * 40 * 1024 + 1024 == 135 * 1024     # ring of 3 steps x 3 taps, two 40-KiB patch buffers, 1 KiB of epilogue parameters

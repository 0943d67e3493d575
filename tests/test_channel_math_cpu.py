"""The degraded-link draw's arithmetic (v2x-sim_amd/csrc/channel_math.h: Philox4x32-10, the counter layout, the two uniforms, the normals), checked
on the host -- the check that runs without a GPU.

tests/channel_driver.cpp is compiled with the host compiler against the SAME header the kernel compiles and prints words, uniforms, link decisions
and normals of every directed pair of a few (seed, step, Bt, A, p); they are compared with tests/channel_refs.py, which is written from the
definitions: words, uniforms (as fp32 bit patterns) and link decisions exactly, normals within 1e-5 (fp32 libm against float64: |n| <= 5.77, the
angle's fp32 rounding <= 5e-7, a few ulp from libm -- about 3.5e-6 in all)."""
import os
import shutil
import struct
import subprocess

import pytest

import channel_refs as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "v2x-sim_amd", "csrc")

# (seed, step, Bt, A, p): a small table, a seed >= 2^32, both sides of the step's carry, A = 32 (the agent fields' top values), p at both ends
DRAWS = [(7, 0, 3, 5, 0.3), (CR.BIG_SEED, 17, 2, 5, 0.3), (21, CR.CARRY_STEP, 1, 32, 0.3), (21, CR.CARRY_STEP + 1, 1, 32, 0.3),
         ((1 << 64) - 1, (1 << 63) + 5, 2, 3, 0.5), (5, 2, 2, 4, 0.0), (5, 2, 2, 4, 1.0)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/bin/hipcc") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("channel") / "channel_driver")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "channel_driver.cpp"), "-o", exe, "-lm"]
    if cxx.endswith("hipcc"):
        cmd[1:1] = ["-x", "c++"]
    subprocess.check_call(cmd)
    return lambda *args: subprocess.run([exe] + list(args), capture_output=True, text=True, check=True).stdout.splitlines()


def _f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def test_known_answer_vectors(driver):
    out = driver("kat")
    assert [tuple(int(x, 16) for x in line.split()) for line in out] == [k[2] for k in CR.KATS]


@pytest.mark.parametrize("draw", DRAWS, ids=lambda d: "seed%x-step%x-b%d-a%d-p%g" % d)
def test_words_uniforms_links_and_normals(driver, draw):
    seed, step, Bt, A, p = draw
    lines = driver("%d,%d,%d,%d,%r" % (seed, step, Bt, A, p))
    assert len(lines) == Bt * A * (A - 1)
    it = iter(lines)
    worst = 0.0
    for f in range(Bt):
        for i in range(A):
            for j in range(A):
                if j == i:
                    continue
                t = next(it).split()
                assert (int(t[0]), int(t[1]), int(t[2])) == (f, i, j)
                wo = CR.words(seed, step, f, CR.DOMAIN_OUTAGE, i, j)
                wp = CR.words(seed, step, f, CR.DOMAIN_POSE, i, j)
                assert tuple(int(x, 16) for x in t[3:7]) == wo, (f, i, j)
                assert int(t[7], 16) == _f32_bits(CR.outage_uniform(wo[0]))                  # exact in fp32: the pack rounds nothing
                assert int(t[8]) == int(CR.link_down(seed, step, f, i, j, p))
                assert tuple(int(x, 16) for x in t[9:13]) == wp, (f, i, j)
                assert tuple(int(x, 16) for x in t[13:17]) == tuple(_f32_bits(u) for u in CR.pose_uniforms(wp))
                for got, want in zip(t[17:20], CR.normals(seed, step, f, i, j)):
                    worst = max(worst, abs(float(got) - want))
    print("normals: max |fp32 - float64| = %.3g" % worst)
    assert worst <= 1e-5

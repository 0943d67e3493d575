"""The streamed 3x3 kernels' patch geometry (v2x-sim_amd/csrc/stream_geom.h: patch_desc, patch_col, patch_slot_off), checked on the host.

tests/stream_geom_driver.cpp is compiled with the host compiler and prints, for a tile of an image, the LDS-DMA source descriptor of every 16-byte
slot of the patch and the fragment-read offset of every (output column, tap column kx, k-slot quarter fq).  The model below is written from the data
layout, not from the helper (activations are NHWC bf16 [item][y][x][c]; csrc/conv_stream.hip: the patch of a chunk is pixel-major,
64 bytes = four 16-byte channel slots per pixel, slot s of patch column pc at physical slot s ^ ((pc >> shift) & 3)): it fills an image with one id
per (pixel, channel slot), plays the DMA the descriptors describe into an LDS image, and compares
  * the LDS image with the patch the convolution needs -- every patch pixel inside the image holds exactly its source pixel's four slots (a
    permutation of them, by the swizzle), every pixel outside the image and every slot behind the patch is the zero page (-1);
  * what the column table makes a lane read, in every patch row, with the operand of that tap: source column x0 + col + kx - 1 (zero padding outside
    the image; at half resolution the x2 nearest-upsampled map, i.e. source column >> 1 of the half-size map), the lane's own slot fq."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "v2x-sim_amd", "csrc")

# (TH, TW), image (H, W), tiles (y0, x0): one tile that meets all four borders at once, and the four corner tiles (+ an interior one where there is one)
IMAGES = {
    (16, 32): [((16, 32), [(0, 0)]), ((32, 64), [(0, 0), (0, 32), (16, 0), (16, 32)]), ((48, 96), [(16, 32)])],
    (8, 32): [((8, 32), [(0, 0)]), ((32, 64), [(0, 0), (0, 32), (24, 0), (24, 32), (8, 32)])],
    (16, 16): [((16, 16), [(0, 0)]), ((32, 64), [(0, 0), (0, 48), (16, 0), (16, 48), (16, 16)])],
}
CASES = [(th, tw, psh, h, w, n, y0, x0, hf) for (th, tw), images in IMAGES.items() for (h, w), tiles in images for (y0, x0) in tiles
         for psh in (1, 2) for n in (0, 2) for hf in (0, 1)]


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/bin/hipcc") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("geom") / "stream_geom_driver")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "stream_geom_driver.cpp"), "-o", exe]
    if cxx.endswith("hipcc"):
        cmd[1:1] = ["-x", "c++"]
    subprocess.check_call(cmd)
    out = subprocess.run([exe] + [",".join(map(str, c)) for c in CASES], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == 2 * len(CASES)
    return {c: (np.array(out[2 * i].split()[1:], dtype=np.int64), np.array(out[2 * i + 1].split()[1:], dtype=np.int64)) for i, c in enumerate(CASES)}


def _model(th, tw, psh, h, w, n, y0, x0, hf):
    """-> (ids of the source map [N][Hs][Ws][4 slots], the patch the tile needs as [PH][PW] source pixels (y, x) or None)"""
    hs, ws = (h // 2, w // 2) if hf else (h, w)
    ph, pw = (th // 2 + 2, tw // 2 + 2) if hf else (th + 2, tw + 2)
    yt, xt = (y0 // 2 - 1, x0 // 2 - 1) if hf else (y0 - 1, x0 - 1)
    ids = np.arange(3 * hs * ws * 4, dtype=np.int64).reshape(3, hs, ws, 4) + 1        # 0 = the zero page
    need = [[(yt + r, xt + c) if 0 <= yt + r < hs and 0 <= xt + c < ws else None for c in range(pw)] for r in range(ph)]
    return ids, need, (hs, ws, ph, pw, yt)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "t%dx%d-swz%d-%dx%d-n%d-y%d-x%d-%s" % (c[:8] + ("half" if c[8] else "full",)))
def test_patch_descriptor_and_column_table(case, driver_output):
    th, tw, psh, h, w, n, y0, x0, hf = case
    desc, ctab = driver_output[case]
    ids, need, (hs, ws, ph, pw, yt) = _model(*case)
    flat = ids.reshape(-1, 4)                                   # [pixel index (n * Hs + y) * Ws + x][slot]

    # ---- play the DMA: LDS slot L <- 16 bytes at element offset (d >> 5) * C + (d & 31) of a 32-channel chunk, or the zero page
    assert len(desc) >= ph * pw * 4 + 64 and len(desc) % 64 == 0
    lds = np.zeros(len(desc), dtype=np.int64)
    for L, d in enumerate(desc):
        if d == -1:
            continue
        assert d >= 0 and (d & 31) % 8 == 0, (L, d)
        lds[L] = flat[d >> 5, (d & 31) // 8]
    # ---- the patch: pixel-major, slot s of patch column pc at physical slot s ^ ((pc >> psh) & 3)
    for r in range(ph):
        for c in range(pw):
            got = lds[(r * pw + c) * 4:(r * pw + c) * 4 + 4]
            if need[r][c] is None:
                assert (desc[(r * pw + c) * 4:(r * pw + c) * 4 + 4] == -1).all(), (r, c)
                continue
            y, x = need[r][c]
            want = ids[n, y, x]
            assert sorted(got) == sorted(want), (r, c, got, want)                  # the pixel's own four slots, each once
            for s in range(4):
                assert got[s ^ ((c >> psh) & 3)] == want[s], (r, c, s)
    assert (desc[ph * pw * 4:] == -1).all()                                        # behind the patch: the zero page

    # ---- the column table: lane (fq) of output column col under tap column kx reads, in patch row r, the operand of that tap
    ctab = ctab.reshape(tw, 3, 4)
    for col in range(tw):
        for kx in range(3):
            X = x0 + col + kx - 1                               # the tap's column of the (upsampled) input; outside [0, W): zero padding
            for fq in range(4):
                off = int(ctab[col, kx, fq])
                assert off % 16 == 0 and 0 <= off < pw * 64, (col, kx, fq, off)
                for r in range(ph):
                    y, xs = yt + r, (X >> 1) if hf else X       # the patch row's source row; the tap's source column
                    want = ids[n, y, xs, fq] if (0 <= y < hs and 0 <= X < w) else 0
                    assert lds[r * pw * 4 + off // 16] == want, (col, kx, fq, r)

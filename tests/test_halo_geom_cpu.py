"""The resident-weight "halo" kernels' patch geometry (v2x-sim_amd/csrc/halo_geom.h), checked on the host: no GPU, a few seconds.

tests/halo_geom_driver.cpp is compiled with the host compiler, once per swizzle build (-DV2X_HALO_PSWZ_BUILD=1 / 2), and prints the DMA table word of
every LDS slot (with its fields as the header takes them apart) and the fragment read offset of every (patch row, patch column, k-slot).  The model
below is written from the data layout, not from the helpers (the header's first comment: NHWC bf16 maps; a patch is pixel-major, SPP 16-byte slots per
pixel, logical slot s of patch column x at physical slot s ^ swizzle(x); table word = offset | row << 20 | column << 24, -1 behind the patch): it fills
a source map with one id per (pixel, 16-byte channel slot), plays the DMAs the table words describe for a tile the way the kernels' fill loops do
(image-bounds test on the word's row and column; base of the patch's first source pixel + the word's offset; else the zero page) and checks
  * every patch pixel inside the image holds exactly its source pixel's slots, slot s at s ^ swizzle; every pixel outside the image and every slot
    behind the patch is the zero page;
  * the fragment read offset of every (output row, output column, tap row, tap column, k-slot) lands on the operand of that tap: zero padding outside
    the image, source pixel >> 1 for the x2 nearest-upsampled half-resolution source, the column-parity plane for the parity-class form;
  * the table form and the direct form (halo_slot_src) give the same DMA source for every slot of the full- and the half-resolution patch, and that
    source is the one the model played;
  * the tail's window: the tile-invariant lane offset of every window slot reads its pixel's slot at in_coff of an in_cstride-channel map.
(The tail's border-tile window fill and the fill loops' own bounds test are written in the kernels: tests/test_gpu_conv_sweep.py and
tests/test_gpu_tail.py cover them on the device.)"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "v2x-sim_amd", "csrc")
TH, TW = 8, 32
# image (H, W) -> tiles (y0, x0): one tile touching all four borders; the four corner tiles; an interior tile
IMAGES = [((8, 32), [(0, 0)]), ((16, 64), [(0, 0), (0, 32), (8, 0), (8, 32)]), ((24, 96), [(8, 32)])]
FULL, HALF, PLANES, WINDOW = 0, 1, 2, 3
# (kind, SPP, in_cstride, in_coff): 32, 64 and 96 channels; the planes at the widths the parity-class form is built for and one more; the tail's window
FORMS = ([(FULL, s, 0, 0) for s in (4, 8, 12)] + [(HALF, s, 0, 0) for s in (4, 8, 12)] + [(PLANES, s, 0, 0) for s in (4, 8)] +
         [(WINDOW, 4, 32, 0), (WINDOW, 4, 96, 40)])
CASES = [(b, k, s, cs, co, h, w, n, y0, x0) for b in (1, 2) for (k, s, cs, co) in FORMS for (h, w), tiles in IMAGES for (y0, x0) in tiles for n in (0, 2)]


def _swz(build, spp, x):
    if build == 1:
        return (x & 7) if spp == 8 else ((x >> 1) & 3)
    return ((((x >> 1) & 1) << 2) ^ ((x >> 2) & 3)) if spp == 8 else ((x >> 2) & 3)


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/bin/hipcc") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    out = {}
    keys = sorted({(k, s, w, cs) for (_, k, s, cs, _, _, w, _, _, _) in CASES})
    for build in (1, 2):
        exe = str(tmp_path_factory.mktemp("halo_geom") / ("halo_geom_driver%d" % build))
        cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-DV2X_HALO_PSWZ_BUILD=%d" % build, "-I", CSRC, os.path.join(ROOT, "tests", "halo_geom_driver.cpp"), "-o", exe]
        if cxx.endswith("hipcc"):
            cmd[1:1] = ["-x", "c++"]
        subprocess.check_call(cmd)
        tiles = sorted({(k, s, h, w, n, y0, x0) for (_, k, s, _, _, h, w, n, y0, x0) in CASES if k in (FULL, HALF)})
        lines = subprocess.run([exe] + ["%d,%d,%d,%d" % k for k in keys] + ["%d,%d,%d,%d,%d,%d,%d" % t for t in tiles],
                               capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(lines) == 3 * len(keys) + len(tiles)
        for i, k in enumerate(keys):
            out[(build,) + k] = tuple(np.array(lines[3 * i + j].split()[1:], dtype=np.int64) for j in range(3))
        for i, t in enumerate(tiles):
            out[(build, "forms") + t] = np.array(lines[3 * len(keys) + i].split()[1:], dtype=np.int64).reshape(-1, 2)
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "swz%d-kind%d-spp%d-cs%d+%d-%dx%d-n%d-y%d-x%d" % c)
def test_patch_fill_and_fragment_reads(case, driver_output):
    build, kind, spp, cs, coff, H, W, n, y0, x0 = case
    E, F, G = driver_output[(build, kind, spp, W, cs)]
    if kind == WINDOW:
        return _check_window(build, cs, coff, H, W, n, y0, x0, E, F)
    C = spp * 8
    hs, ws = (H // 2, W // 2) if kind == HALF else (H, W)
    ph, pw = (TH // 2 + 2, TW // 2 + 2) if kind == HALF else (TH + 2, TW + 2)
    yt, xt = (y0 // 2 - 1, x0 // 2 - 1) if kind == HALF else (y0 - 1, x0 - 1)
    ids = np.arange(3 * hs * ws * spp, dtype=np.int64).reshape(3, hs, ws, spp) + 1          # 0 = the zero page
    flat = ids.reshape(-1)

    # ---- play the DMAs as the kernels' fill loops do
    E = E.reshape(-1, 4)
    assert len(E) % 64 == 0 and len(E) >= ph * pw * spp
    base = ((n * hs + yt) * ws + xt) * C
    lds = np.zeros(len(E), dtype=np.int64)
    src = np.full(len(E), -1, dtype=np.int64)                                                # the element offset each slot's DMA reads, -1 = zero page
    for L, (e, row, col, off) in enumerate(E):
        if e < 0:
            assert e == -1
            continue
        assert (row, col, off) == ((e >> 20) & 15, (e >> 24) & 63, e & 0xfffff) and off % 8 == 0, (L, e)
        y, x = yt + row, xt + col
        if 0 <= y < hs and 0 <= x < ws:
            elem = base + off
            assert elem % 8 == 0 and (elem % C) // 8 < spp
            lds[L] = flat[(elem // C) * spp + (elem % C) // 8]
            src[L] = elem
    assert (E[ph * pw * spp:, 0] == -1).all()                                                # behind the patch: the zero page

    # ---- the patch the layout promises; lds_pix(pr, pc) = first LDS slot of the pixel, swizzled on column sx
    def lds_pix(pr, pc):
        if kind == PLANES:
            return (((pc & 1) * ph + pr) * (pw // 2) + (pc >> 1)) * spp, pc >> 1
        return (pr * pw + pc) * spp, pc
    for pr in range(ph):
        for pc in range(pw):
            p0, sx = lds_pix(pr, pc)
            y, x = yt + pr, xt + pc
            inside = 0 <= y < hs and 0 <= x < ws
            for s in range(spp):
                assert lds[p0 + (s ^ _swz(build, spp, sx))] == (ids[n, y, x, s] if inside else 0), (pr, pc, s)

    # ---- the two fill forms: the table form as the driver (like the kernels' loops) evaluates it, and the direct form, against what was played
    if kind in (FULL, HALF):
        forms = driver_output[(build, "forms", kind, spp, H, W, n, y0, x0)]
        assert len(forms) == len(E)
        assert (forms[:, 0] == src).all() and (forms[:, 1] == src).all(), np.nonzero((forms[:, 0] != src) | (forms[:, 1] != src))[0][:8]
    if kind == HALF:                                                                         # the header's own column rule for the upsampled source
        Gh = G.reshape(ph, TW, 3, spp)
        for col in range(TW):
            for kx in range(3):
                assert (Gh[:, col, kx, :] == F.reshape(ph, pw, spp)[:, ((col + kx - 1) >> 1) + 1, :]).all(), (col, kx)

    # ---- fragment reads: output pixel (r, col) under tap (ky, kx), k-slot k
    if kind == PLANES:
        Fo = F.reshape(2, ph, pw // 2, spp)
    else:
        Fo = F.reshape(ph, pw, spp)
    for r in range(TH):
        for ky in range(3):
            Y = y0 + r + ky - 1
            for col in range(TW):
                for kx in range(3):
                    X = x0 + col + kx - 1
                    if kind == HALF:
                        pr, pc, ys, xs = ((r + ky - 1) >> 1) + 1, ((col + kx - 1) >> 1) + 1, Y >> 1, X >> 1
                    else:
                        pr, pc, ys, xs = r + ky, col + kx, Y, X
                    inside = 0 <= Y < H and 0 <= X < W
                    for k in range(spp):
                        off = int(Fo[pc & 1, pr, pc >> 1, k] if kind == PLANES else Fo[pr, pc, k])
                        assert off % 16 == 0
                        assert lds[off // 16] == (ids[n, ys, xs, k] if inside else 0), (r, ky, col, kx, k)


def _check_window(build, cs, coff, H, W, n, y0, x0, rel, F):
    ih, iw, sps = TH + 4, TW + 4, cs // 8
    ids = np.arange(3 * H * W * sps, dtype=np.int64).reshape(3, H, W, sps) + 1
    flat = ids.reshape(-1)
    assert len(rel) == ih * iw * 4
    base = ((n * H + y0 - 2) * W + x0 - 2) * cs + coff
    F = F.reshape(ih, iw, 4)
    for pr in range(ih):
        for pc in range(iw):
            y, x = y0 - 2 + pr, x0 - 2 + pc
            if not (0 <= y < H and 0 <= x < W):
                continue                                  # a border tile's out-of-image pixels: the kernel's own bounds test, the zero page
            for k in range(4):
                off = int(F[pr, pc, k])
                assert off % 16 == 0 and off // 16 == (pr * iw + pc) * 4 + (k ^ _swz(build, 4, pc)), (pr, pc, k)
                elem = base + int(rel[off // 16])
                assert elem % 8 == 0
                assert flat[(elem // cs) * sps + (elem % cs) // 8] == ids[n, y, x, coff // 8 + k], (pr, pc, k)

// Tile and patch geometry of the streamed 3x3 kernels (conv_stream.hip, conv_stream_pc.hip, conv_stream_s2.hip; the workgroup remap also conv_igemm.hip):
// ONE definition of the integer arithmetic every kernel form used to carry a copy of.  Plain integers in, plain integers out -- no HIP type -- so a
// host compiler can build it too: tests/test_stream_geom_cpu.py checks the patch descriptor and the column table against a model of DESIGN.md section 5.
#pragma once

#if defined(__HIPCC__)
#define V2X_GEOM_FN __host__ __device__ __forceinline__
#else
#define V2X_GEOM_FN static inline
#endif

// XCD-major workgroup order (guide T1): the hardware deals consecutive workgroup ids to the 8 XCDs round-robin (workgroup b runs on XCD b % 8); this
// gives every XCD a CONTIGUOUS run of tiles, so that the channel tiles of one pixel tile (same activations) and neighbouring pixel tiles (shared
// halos) meet in one L2.  Bijective for any grid size.
V2X_GEOM_FN int xcd_major_bid(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, i = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + i;
}

// Pixel-tile id -> image n and the tile's first output pixel (y0, x0).  Pixel tiles run along tiles_x, then tiles_y, then the images;
// txy = tiles_x * tiles_y.
template <int TH, int TW>
V2X_GEOM_FN void px_tile_coords(int tiles_x, int txy, int px_tile, int &n, int &y0, int &x0) {
    n = px_tile / txy;
    const int trem = px_tile - n * txy;
    const int ty = trem / tiles_x;
    y0 = ty * TH;
    x0 = (trem - ty * tiles_x) * TW;
}
// Tile id (channel tile fastest, then the pixel tiles) -> (n, y0, x0): the persistent kernels, which decode many tiles of ONE channel tile and
// keep txy
template <int TH, int TW>
V2X_GEOM_FN void stream_tile_coords(int tiles_x, int n_co_tiles, int txy, int tile, int &n, int &y0, int &x0) {
    px_tile_coords<TH, TW>(tiles_x, txy, tile / n_co_tiles, n, y0, x0);
}
// ... -> (channel tile, n, y0, x0): the kernels that own one tile per workgroup.  (Statement order is the kernels' own -- channel split, then
// txy: the compiled kernels are instruction for instruction what they were with this written out in each of them.)
template <int TH, int TW>
V2X_GEOM_FN void stream_tile_coords(int tiles_x, int tiles_y, int n_co_tiles, int tile, int &co_tile, int &n, int &y0, int &x0) {
    co_tile = tile % n_co_tiles;
    const int px_tile = tile / n_co_tiles;
    px_tile_coords<TH, TW>(tiles_x, tiles_x * tiles_y, px_tile, n, y0, x0);
}

// Patch swizzle: patch column pc's channel slot s (16 bytes) lives at physical slot s ^ patch_swz<PSH>(pc) of the pixel's 64 bytes.
// PSH = 1 is the production swizzle everywhere; 2 is the other candidate of conv_stream.hip (V2X_STREAM_PSWZ_BUILD).
template <int PSH>
V2X_GEOM_FN int patch_swz(int pc) { return (pc >> PSH) & 3; }

// DMA source descriptor of 16-byte slot L of a PH x PW patch (pixel-major, 4 slots per pixel) whose first pixel is source pixel (yt, xt) of image n
// of an H x W map:  (source pixel index << 5) | (logical slot * 8 elements),  -1 = zero page (outside the image, or the padding behind the patch).
template <int PH, int PW, int PSH>
V2X_GEOM_FN int patch_desc_at(int H, int W, int n, int yt, int xt, int L) {
    const int pix = L >> 2, phys = L & 3;
    const int pr = pix / PW, pc = pix - pr * PW;
    const int y = yt + pr, x = xt + pc;
    const bool ok = pix < PH * PW && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
    return ok ? ((((n * H + y) * W + x) << 5) | ((phys ^ patch_swz<PSH>(pc)) << 3)) : -1;
}
// The patch of a TH x TW output tile at (y0, x0) of an H x W output: (TH + 2) x (TW + 2) pixels from (y0 - 1, x0 - 1) of a full-resolution source, or
// (hf: the x2 nearest-upsampled decoder operand) the (TH/2 + 2) x (TW/2 + 2) pixels from (y0/2 - 1, x0/2 - 1) of the H/2 x W/2 map.
template <int TH, int TW, int PSH>
V2X_GEOM_FN int patch_desc(int H, int W, int n, int y0, int x0, int L, bool hf) {
    if (!hf) return patch_desc_at<TH + 2, TW + 2, PSH>(H, W, n, y0 - 1, x0 - 1, L);
    return patch_desc_at<TH / 2 + 2, TW / 2 + 2, PSH>(H >> 1, W >> 1, n, (y0 >> 1) - 1, (x0 >> 1) - 1, L);
}

// Patch column of output column `col` under tap column kx: col + kx at full resolution, floor((col + kx - 1) / 2) + 1 at half resolution
V2X_GEOM_FN int patch_col(int col, int kx, bool hf) { return hf ? (((col + kx - 1) >> 1) + 1) : (col + kx); }
// Byte offset inside a patch row of the B fragment read of lane (pixel at patch column pc, k-slot quarter fq): the pixel's 64 bytes, the lane's
// logical slot fq at its swizzled place
template <int PSH>
V2X_GEOM_FN int patch_slot_off(int pc, int fq) { return ((pc << 2) + (fq ^ patch_swz<PSH>(pc))) * 16; }

// Tile and patch geometry of the resident-weight "halo" 3x3 kernels (conv_halo.hip, conv_halo_pair.hip, conv_tail.hip): ONE definition of the integer
// arithmetic every kernel form used to carry a copy of.  Plain integers in, plain integers out -- no HIP type -- so a host compiler can build it too:
// tests/test_halo_geom_cpu.py plays the DMAs these descriptors describe and holds the result against a model of the layout below.  The tile decode and
// the workgroup order are stream_geom.h's (px_tile_coords, xcd_major_bid).
//
// THE LAYOUT.  Activations are NHWC bf16; a 16-byte SLOT is 8 channels of one pixel, SPP = C / 8 slots per pixel.  A PH x PW patch lies in LDS
// pixel-major: pixel (pr, pc) at slots [(pr * PW + pc) * SPP, + SPP), its logical slot s at physical slot halo_swz<SPP>(s, pc) of those -- the XOR rule
// that keeps the 16-lane ds_read_b128 groups of a fragment (16 consecutive pixels of one patch row, one k-slot) off each other's banks.  The patch is
// filled by LDS-DMA, 64 slots (1 KiB) per wave instruction, so its slot count is rounded up to whole waves (round64); the slots behind the patch and
// the pixels outside the image read the zero page.
// TABLE WORD of LDS slot L (computed once per lane and piece, tile-invariant):  bits 0-19 = element offset of the lane's 16 bytes from the patch's
// first source pixel, bits 20-23 = patch row, bits 24-29 = patch column (for the image-bounds test), -1 = a slot behind the patch.  The dispatch
// bounds W so that the offset fits its 20 bits.
// (Statement order inside the helpers is the kernels' own: they compile to the instruction streams they had with this written out in each of them.)
#pragma once
#include "stream_geom.h"

namespace halo {
constexpr int TH = 8, TW = 32;              // output tile
constexpr int PH = TH + 2, PW = TW + 2;     // its full-resolution patch (= the region the fused pairs compute their first layer on: MH x MW)
constexpr int PH0 = TH / 2 + 2, PW0 = TW / 2 + 2;   // ... of the half-resolution (x2 nearest-upsampled) source
constexpr int PWH = PW / 2;                 // columns per column-parity plane of the full-resolution patch (parity-class form)
constexpr int MH = PH, MW = PW;
constexpr int IH = TH + 4, IW = TW + 4;     // input window of the fused pairs (two 3x3 layers deep)

constexpr int round64(int v) { return (v + 63) / 64 * 64; }
constexpr int ns1(int c1) { return round64(PH * PW * (c1 / 8)); }             // 16-B slots of the full-resolution patch, padded to whole waves
constexpr int ns0(int c0) { return round64(PH0 * PW0 * (c0 / 8)); }           // ... of the half-resolution patch (0 without one)
constexpr int ns1_planes(int c1) { return round64(2 * PH * PWH * (c1 / 8)); } // ... of the two column-parity planes
}  // namespace halo

// Patch swizzle (slot permutation per pixel x).  Chosen by TIMING the fragment reads (tools/lds_conflict_probe.hip: lane (fj, fq) reads
// 16 bytes of pixel x0 + fj -- or ((c + fj) >> 1) + 1 for a half-resolution source -- at slot 4*kc + fq; 8 reads in flight per wave):
//   4 slots per pixel:  (x >> 2) & 3             17.5 ns per read at every alignment of both forms;  the round-1 choice (x >> 1) & 3:
//                                                22.9 ns for EVERY full-resolution read, 22.6 for two of three half-resolution alignments
//   8 slots per pixel:  ((x >> 1) & 1) * 4 ^ ((x >> 2) & 3)   17.2-17.5 ns;  round 1's x & 7: 22.7 / 19.2 ns
// SQ_LDS_BANK_CONFLICT reads 0 for the slow full-resolution patterns: the counter does not see whatever pairing rule ds_read_b128
// applies, which is how round 1's search (driven by that counter) settled on them.  INSIDE the kernels the faster reads change nothing
// (same-box A/B, two runs each: heads 1 132-1 154 vs 1 133-1 139 us, conv8_1 967-974 vs 975-977, pair kernel 687-713 vs 723-727 (worse: its
// layer-A epilogue WRITES this layout), conv7_2 365-367 vs 364-369; the tail kernel +3 %): the fragment reads are not what these kernels wait
// for.  Default stays the round-1 swizzle (V2X_HALO_PSWZ_BUILD=1); =2 builds the timing-derived one, in all three files.
#ifndef V2X_HALO_PSWZ_BUILD
#define V2X_HALO_PSWZ_BUILD 1
#endif
template <int SPP>
V2X_GEOM_FN int halo_swz(int slot, int x) {
    if constexpr (V2X_HALO_PSWZ_BUILD == 1) {
        if constexpr (SPP == 8) return slot ^ (x & 7);
        else return slot ^ ((x >> 1) & 3);
    } else {
        if constexpr (SPP == 8) return slot ^ ((((x >> 1) & 1) << 2) ^ ((x >> 2) & 3));
        else return slot ^ ((x >> 2) & 3);  // SPP 4 or 12: permute inside each aligned group of 4 slots
    }
}

// Tile id -> image n and the tile's INDICES (ty, tx) instead of its first pixel: the kernels that test for border tiles
V2X_GEOM_FN void halo_tile_index(int tiles_x, int txy, int tile, int &n, int &ty, int &tx) { px_tile_coords<1, 1>(tiles_x, txy, tile, n, ty, tx); }

// ---- fragment reads ----------------------------------------------------------------------------------------------------------------------
// Byte offset of logical slot `kslot` of the patch pixel with linear index pix in patch column pc
template <int SPP>
V2X_GEOM_FN int halo_pix_off(int pix, int pc, int kslot) { return (pix * SPP + halo_swz<SPP>(kslot, pc)) * 16; }
// ... of patch pixel (pr, pc) of a patch PW_ columns wide
template <int PW_, int SPP>
V2X_GEOM_FN int halo_frag_off(int pr, int pc, int kslot) { return ((pr * PW_ + pc) * SPP + halo_swz<SPP>(kslot, pc)) * 16; }
// ... of the operand of output column `col` under tap column kx in patch row pr of a full-resolution PH x PW patch
template <int SPP>
V2X_GEOM_FN int halo_frag_off_full(int pr, int col, int kx, int kslot) { return halo_frag_off<halo::PW, SPP>(pr, col + kx, kslot); }
// ... the same for the x2 nearest-upsampled half-resolution source, patch row pr of its PH0 x PW0 patch: patch column ((col + kx - 1) >> 1) + 1
// (stream_geom.h: patch_col)
template <int SPP>
V2X_GEOM_FN int halo_frag_off_half(int pr, int col, int kx, int kslot) { return halo_frag_off<halo::PW0, SPP>(pr, patch_col(col, kx, true), kslot); }
// ... of plane column cc, row pr of column-parity plane q (patch column 2 cc + q): the swizzle is the dense form's on the plane column
template <int SPP>
V2X_GEOM_FN int halo_frag_off_plane(int q, int pr, int cc, int kslot) { return halo_pix_off<SPP>((q * halo::PH + pr) * halo::PWH + cc, cc, kslot); }

// ---- patch fill --------------------------------------------------------------------------------------------------------------------------
// A slot's DMA source is (does it read the image -- else the zero page --, element offset of its 16 bytes in the source map).  Two forms give it:
// the TABLE form -- halo_entry once per lane and piece, then per tile its fields against the tile's origin (the fill loops of the kernels: bounds test
// on row and column, halo_patch_base + offset) -- and the DIRECT form halo_slot_src, per piece and tile, of the kernels on a tight register budget.
// tests/test_halo_geom_cpu.py holds the two against each other for every slot.  (conv_halo.hip's own fill loops and read sites carry this text written out,
// on halo_swz and the table-word functions: through halo_slot_src / halo_frag_off* two of its kernels measured slower -- HISTORY.md.)
//
// Direct form: slot L of a PH_ x PW_ patch whose first pixel is source pixel (yt, xt) of image n of an [N][H][W][C] map
template <int PH_, int PW_, int SPP>
V2X_GEOM_FN bool halo_slot_src(int H, int W, int C, int n, int yt, int xt, int L, unsigned &off) {
    const int pix = L / SPP, phys = L - pix * SPP;
    const int pr = pix / PW_, pc = pix - pr * PW_;
    const int y = yt + pr, x = xt + pc;
    const bool ok = pix < PH_ * PW_ && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
    off = ((unsigned)(n * H + y) * (unsigned)W + (unsigned)x) * (unsigned)C + halo_swz<SPP>(phys, pc) * 8;   // may wrap outside the image: used where ok
    return ok;
}
// Table form: element offset of the patch's first source pixel (y0 - 1, x0 - 1) of the tile at (y0, x0), once per tile
V2X_GEOM_FN unsigned halo_patch_base(int H, int W, int C, int n, int y0, int x0) {
    return ((unsigned)(n * H + y0 - 1) * (unsigned)W + (unsigned)(x0 - 1)) * (unsigned)C;
}
// Table word of LDS slot L of a PH_ x PW_ patch with SPP slots per pixel; the source has C channels per pixel and a row stride of W >> WSH pixels
// (WSH = 1: the half-resolution source of a W-wide output)
template <int PH_, int PW_, int SPP, int WSH = 0>
V2X_GEOM_FN int halo_entry(int W, int C, int L) {
    const int pix = L / SPP, phys = L - pix * SPP;
    const int pr = pix / PW_, pc = pix - pr * PW_;
    return pix < PH_ * PW_ ? (((pr * (W >> WSH) + pc) * C + halo_swz<SPP>(phys, pc) * 8) | (pr << 20) | (pc << 24)) : -1;
}
// ... its fields: patch row and column (for the image-bounds test), element offset
V2X_GEOM_FN int halo_entry_row(int e) { return (e >> 20) & 15; }
V2X_GEOM_FN int halo_entry_col(int e) { return (e >> 24) & 63; }
V2X_GEOM_FN unsigned halo_entry_off(int e) { return (unsigned)(e & 0xfffff); }
// ... of the full-resolution patch stored as two column-parity planes [q][PH][PWH]: slot L -> (plane q, row pr, plane column cc, physical slot);
// the pixel it holds is patch column pc = 2 cc + q (the DMA permutes the pixels on their way in)
template <int SPP>
V2X_GEOM_FN int halo_entry_planes(int W, int C, int L) {
    const int pix = L / SPP, phys = L - pix * SPP;
    const int q = pix / (halo::PH * halo::PWH), rem = pix - q * (halo::PH * halo::PWH);
    const int pr = rem / halo::PWH, cc = rem - pr * halo::PWH;
    const int pc = 2 * cc + q;
    return pix < 2 * halo::PH * halo::PWH ? (((pr * W + pc) * C + halo_swz<SPP>(phys, cc) * 8) | (pr << 20) | (pc << 24)) : -1;
}

// The fused tail's IH x IW input window (4 slots per pixel: 32 channels of a map with cs channels per pixel), tile-invariant part of window slot sidx:
// element offset from the window's first pixel (a tile away from the image border needs no bounds test)
V2X_GEOM_FN unsigned halo_window_rel(int W, int cs, int sidx) {
    const int pix = sidx >> 2, phys = sidx & 3;
    const int pr = pix / halo::IW, pcx = pix - pr * halo::IW;
    return (unsigned)(pr * W + pcx) * (unsigned)cs + (unsigned)(halo_swz<4>(phys, pcx) * 8);
}

#if defined(__HIPCC__)
// 64 B of zeros: the LDS-DMA source of out-of-image patch pixels and of the slots behind a patch (the one device-side declaration here; one copy per
// translation unit: no relocatable device code needed)
static __device__ __attribute__((aligned(64))) unsigned int g_halo_zero_page[16];
#endif

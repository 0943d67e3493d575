// Host driver of tests/test_halo_geom_cpu.py: prints what v2x-sim_amd/csrc/halo_geom.h computes, so that the test can hold it against its own model of
// the data layout.  Plain C++ (the header needs no HIP type); built once per swizzle build (-DV2X_HALO_PSWZ_BUILD=1 / 2).
//   halo_geom_driver kind,SPP,W,cs ...        kind 0 = full-resolution patch, 1 = half-resolution patch, 2 = parity planes, 3 = the tail's window
// per argument three lines:
//   "E": per LDS slot L = 0 .. NS-1 the table word and its fields as the header takes them apart: e row col off  (kind 3: halo_window_rel, one number)
//   "F": the fragment read offset of every (patch row, patch column, k-slot) -- kind 2: (plane, row, plane column, k-slot)
//   "G": kind 1: halo_frag_off_half of every (patch row, output column, tap column, k-slot); empty otherwise
//   halo_geom_driver kind,SPP,H,W,n,y0,x0 ...  (kind 0 or 1) one line
//   "S": per LDS slot the DMA source in the TABLE form (halo_entry, its fields against the tile origin, halo_patch_base) and in the DIRECT form
//        (halo_slot_src), each as the element offset or -1 for the zero page
#include <cstdio>
#include <cstdlib>

#include "halo_geom.h"

using namespace halo;

template <int SPP>
static void dump(int kind, int W, int cs) {
    const int C = SPP * 8;
    printf("E");
    if (kind == 3) {
        for (int s = 0; s < IH * IW * 4; ++s) printf(" %u", halo_window_rel(W, cs, s));
    } else {
        const int NS = kind == 0 ? ns1(C) : (kind == 1 ? ns0(C) : ns1_planes(C));
        for (int L = 0; L < NS; ++L) {
            const int e = kind == 0 ? halo_entry<PH, PW, SPP>(W, C, L) : (kind == 1 ? halo_entry<PH0, PW0, SPP, 1>(W, C, L) : halo_entry_planes<SPP>(W, C, L));
            printf(" %d %d %d %u", e, halo_entry_row(e), halo_entry_col(e), halo_entry_off(e));
        }
    }
    printf("\nF");
    if (kind == 0) {
        for (int pr = 0; pr < PH; ++pr)
            for (int pc = 0; pc < PW; ++pc)
                for (int k = 0; k < SPP; ++k) printf(" %d", pc < 2 ? halo_frag_off<PW, SPP>(pr, pc, k) : halo_frag_off_full<SPP>(pr, pc - 2, 2, k));
    } else if (kind == 1) {
        for (int pr = 0; pr < PH0; ++pr)
            for (int pc = 0; pc < PW0; ++pc)
                for (int k = 0; k < SPP; ++k) printf(" %d", halo_frag_off<PW0, SPP>(pr, pc, k));
    } else if (kind == 2) {
        for (int q = 0; q < 2; ++q)
            for (int pr = 0; pr < PH; ++pr)
                for (int cc = 0; cc < PWH; ++cc)
                    for (int k = 0; k < SPP; ++k) printf(" %d", halo_frag_off_plane<SPP>(q, pr, cc, k));
    } else {
        for (int pr = 0; pr < IH; ++pr)
            for (int pc = 0; pc < IW; ++pc)
                for (int k = 0; k < 4; ++k) printf(" %d", halo_frag_off<IW, 4>(pr, pc, k));
    }
    printf("\nG");
    if (kind == 1)
        for (int pr = 0; pr < PH0; ++pr)
            for (int col = 0; col < TW; ++col)
                for (int kx = 0; kx < 3; ++kx)
                    for (int k = 0; k < SPP; ++k) printf(" %d", halo_frag_off_half<SPP>(pr, col, kx, k));
    printf("\n");
}

// the two fill forms for one tile: as the kernels' table loops do it, and halo_slot_src
template <int PH_, int PW_, int SPP, int WSH>
static void forms(int H, int W, int n, int y0, int x0) {
    const int C = SPP * 8, Hs = H >> WSH, Ws = W >> WSH, ys = y0 >> WSH, xs = x0 >> WSH;
    const unsigned base = halo_patch_base(Hs, Ws, C, n, ys, xs);
    printf("S");
    for (int L = 0; L < round64(PH_ * PW_ * SPP); ++L) {
        const int e = halo_entry<PH_, PW_, SPP, WSH>(W, C, L);
        const int y = ys - 1 + halo_entry_row(e), x = xs - 1 + halo_entry_col(e);
        const bool ok = e >= 0 && (unsigned)y < (unsigned)Hs && (unsigned)x < (unsigned)Ws;
        unsigned off;
        const bool okd = halo_slot_src<PH_, PW_, SPP>(Hs, Ws, C, n, ys - 1, xs - 1, L, off);
        printf(" %lld %lld", ok ? (long long)(base + halo_entry_off(e)) : -1ll, okd ? (long long)off : -1ll);
    }
    printf("\n");
}
template <int SPP>
static void forms(int kind, int H, int W, int n, int y0, int x0) {
    if (kind == 0) forms<PH, PW, SPP, 0>(H, W, n, y0, x0);
    else forms<PH0, PW0, SPP, 1>(H, W, n, y0, x0);
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        int kind, spp, W, cs, H, n, y0, x0;
        if (sscanf(argv[i], "%d,%d,%d,%d,%d,%d,%d", &kind, &spp, &H, &W, &n, &y0, &x0) == 7) {
            if (kind > 1) return 5;
            if (spp == 4) forms<4>(kind, H, W, n, y0, x0);
            else if (spp == 8) forms<8>(kind, H, W, n, y0, x0);
            else if (spp == 12) forms<12>(kind, H, W, n, y0, x0);
            else return 3;
            continue;
        }
        if (sscanf(argv[i], "%d,%d,%d,%d", &kind, &spp, &W, &cs) != 4) return 2;
        if (spp == 4) dump<4>(kind, W, cs);
        else if (spp == 8) dump<8>(kind, W, cs);
        else if (spp == 12) dump<12>(kind, W, cs);
        else return 3;
    }
    // the tile decode the kernels share with the streamed family: tile -> (n, ty, tx) of a 2 x 3-tile map
    int n, ty, tx;
    halo_tile_index(3, 6, 2 * 6 + 1 * 3 + 2, n, ty, tx);
    return (n == 2 && ty == 1 && tx == 2) ? 0 : 4;
}

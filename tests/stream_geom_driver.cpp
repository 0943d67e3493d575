// Host driver of tests/test_stream_geom_cpu.py: prints what v2x-sim_amd/csrc/stream_geom.h computes, so that the test can hold it against its own
// model of the data layout.  Plain C++ (the header needs no HIP type).
//   stream_geom_driver TH,TW,PSH,H,W,n,y0,x0,hf ...
// per argument one line "D <descriptor of slot L, L = 0 .. NL-1>" (NL = the patch's 1-KiB pieces rounded up, plus one piece of padding) and one line
// "C <byte offset for (col, kx, fq)>", col-major over TW x 3 x 4.
#include <cstdio>
#include <cstdlib>

#include "stream_geom.h"

template <int TH, int TW, int PSH>
static void dump(int H, int W, int n, int y0, int x0, bool hf) {
    const int slots = hf ? (TH / 2 + 2) * (TW / 2 + 2) * 4 : (TH + 2) * (TW + 2) * 4;
    const int NL = ((slots + 63) / 64 + 1) * 64;
    printf("D");
    for (int L = 0; L < NL; ++L) printf(" %d", patch_desc<TH, TW, PSH>(H, W, n, y0, x0, L, hf));
    printf("\nC");
    for (int col = 0; col < TW; ++col)
        for (int kx = 0; kx < 3; ++kx)
            for (int fq = 0; fq < 4; ++fq) printf(" %d", patch_slot_off<PSH>(patch_col(col, kx, hf), fq));
    printf("\n");
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        int TH, TW, PSH, H, W, n, y0, x0, hf;
        if (sscanf(argv[i], "%d,%d,%d,%d,%d,%d,%d,%d,%d", &TH, &TW, &PSH, &H, &W, &n, &y0, &x0, &hf) != 9) return 2;
        const int key = TH * 1000 + TW * 10 + PSH;
        switch (key) {
            case 16321: dump<16, 32, 1>(H, W, n, y0, x0, hf != 0); break;
            case 16322: dump<16, 32, 2>(H, W, n, y0, x0, hf != 0); break;
            case 8321: dump<8, 32, 1>(H, W, n, y0, x0, hf != 0); break;
            case 8322: dump<8, 32, 2>(H, W, n, y0, x0, hf != 0); break;
            case 16161: dump<16, 16, 1>(H, W, n, y0, x0, hf != 0); break;
            case 16162: dump<16, 16, 2>(H, W, n, y0, x0, hf != 0); break;
            default: return 3;
        }
    }
    return 0;
}

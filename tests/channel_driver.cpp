// Host driver of tests/test_channel_math_cpu.py: prints what v2x-sim_amd/csrc/channel_math.h computes, so that the test can hold it against the
// reference of tests/channel_refs.py.  Plain C++ (the header needs no HIP type).
//   channel_driver kat                         the three known-answer vectors of Philox4x32-10: one line of four hex words each
//   channel_driver seed,step,Bt,A,p ...        per argument and directed pair (f, i, j), j != i, one line
//       "f i j  w0 w1 w2 w3 (outage domain, hex)  bits(u)  down  w0 w1 w2 w3 (pose domain, hex)  bits(ua) bits(ub) bits(uc) bits(ud)  nx ny nz (%.9g)"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "channel_math.h"

static uint32_t bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "kat")) {
            const uint32_t kat[3][6] = {{0, 0, 0, 0, 0, 0},
                                        {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                                        {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
            for (const auto &k : kat) {
                const ChanWords w = chan_philox4x32_10(k[0], k[1], k[2], k[3], k[4], k[5]);
                printf("%08x %08x %08x %08x\n", w.w[0], w.w[1], w.w[2], w.w[3]);
            }
            continue;
        }
        uint64_t seed, step;
        int Bt, A;
        float p;
        if (sscanf(argv[a], "%" SCNu64 ",%" SCNu64 ",%d,%d,%f", &seed, &step, &Bt, &A, &p) != 5 || A > CHAN_MAX_AGENTS) return 2;
        for (int f = 0; f < Bt; ++f)
            for (int i = 0; i < A; ++i)
                for (int j = 0; j < A; ++j) {
                    if (j == i) continue;
                    const ChanWords o = chan_words(seed, step, (uint32_t)f, CHAN_DOMAIN_OUTAGE, (uint32_t)i, (uint32_t)j);
                    const ChanWords q = chan_words(seed, step, (uint32_t)f, CHAN_DOMAIN_POSE, (uint32_t)i, (uint32_t)j);
                    float n[3];
                    chan_normals(q, n);
                    printf("%d %d %d %08x %08x %08x %08x %08x %d %08x %08x %08x %08x %08x %08x %08x %08x %.9g %.9g %.9g\n", f, i, j, o.w[0], o.w[1], o.w[2],
                           o.w[3], bits(chan_uniform24(o.w[0])), chan_link_down(o, p) ? 1 : 0, q.w[0], q.w[1], q.w[2], q.w[3], bits(chan_uniform23(q.w[0])),
                           bits(chan_uniform23(q.w[1])), bits(chan_uniform23(q.w[2])), bits(chan_uniform23(q.w[3])), (double)n[0], (double)n[1], (double)n[2]);
                }
    }
    return 0;
}

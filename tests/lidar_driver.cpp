// Host driver of tests/test_lidar_refs_cpu.py: prints what v2x-sim_amd/csrc/lidar_math.h computes, so that the test can hold it against the reference
// of tests/lidar_refs.py.  Plain C++ (the header needs no HIP type).
//   lidar_driver seed,step,n_sweeps,n_rays,p ...      per argument, sweep s and ray r one line
//       "s r  w0 w1 w2 w3 (hex)  bits(uniform24(w0))  dropped  bits(uniform23(w1)) bits(uniform23(w2))  bits(intensity)  normal (%.9g)"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lidar_math.h"

static uint32_t bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; ++a) {
        uint64_t seed, step;
        int n_sweeps, n_rays;
        float p;
        if (sscanf(argv[a], "%" SCNu64 ",%" SCNu64 ",%d,%d,%f", &seed, &step, &n_sweeps, &n_rays, &p) != 5) return 2;
        for (int s = 0; s < n_sweeps; ++s)
            for (int r = 0; r < n_rays; ++r) {
                const ChanWords d = lidar_words(seed, step, (uint32_t)s, (uint32_t)r);
                printf("%d %d %08x %08x %08x %08x %08x %d %08x %08x %08x %.9g\n", s, r, d.w[0], d.w[1], d.w[2], d.w[3], bits(chan_uniform24(d.w[0])),
                       lidar_dropped(d, p) ? 1 : 0, bits(chan_uniform23(d.w[1])), bits(chan_uniform23(d.w[2])), bits(lidar_intensity(d)),
                       (double)lidar_normal(d));
            }
    }
    return 0;
}

// Host driver of tests/test_lidar_motion_refs_cpu.py: prints what the moving-scene functions of v2x-sim_amd/csrc/lidar_math.h compute, so that the test
// can hold them against tests/lidar_motion_refs.py bit for bit.  Plain C++ (the header needs no HIP type), built with -ffp-contract=off as the kernel is.
//   lidar_motion_driver FILE      per line of FILE, all fields hexadecimal bit patterns:
//       "time_of az_time (fp32)  lx0 dlx ly0 dly (fp64)  cx ox vgx vsx (fp32)  t_ref (fp32)"
//   -> "T lx ly (fp64 bits)  T_ref (fp64 bits)  ex (fp64 bits: the relative centre's x at T_ref)"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lidar_math.h"

static float f32(uint32_t u) {
    float v;
    memcpy(&v, &u, 4);
    return v;
}
static double f64(uint64_t u) {
    double v;
    memcpy(&v, &u, 8);
    return v;
}
static uint64_t bits(double v) {
    uint64_t u;
    memcpy(&u, &v, 8);
    return u;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *fh = fopen(argv[1], "r");
    if (!fh) return 2;
    uint32_t t0, ta, cx, ox, vg, vs, tr;
    uint64_t lx0, dlx, ly0, dly;
    int n;
    while ((n = fscanf(fh, "%" SCNx32 " %" SCNx32 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32,
                       &t0, &ta, &lx0, &dlx, &ly0, &dly, &cx, &ox, &vg, &vs, &tr)) == 11) {
        const double T = lidar_ray_time(f32(t0), f32(ta)), T_ref = lidar_ray_time(f32(t0), f32(tr));
        printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits(T), bits(lidar_moved(f64(lx0), f64(dlx), T)),
               bits(lidar_moved(f64(ly0), f64(dly), T)), bits(T_ref), bits(lidar_rel_centre((double)f32(cx), (double)f32(ox), (double)f32(vg), (double)f32(vs), T_ref)));
    }
    fclose(fh);
    return n == EOF ? 0 : 3;
}

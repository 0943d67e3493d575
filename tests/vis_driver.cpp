// Host driver of tests/test_vis_refs_cpu.py: runs the free-space walk of v2x-sim_amd/csrc/vis_math.h -- the code both kernels of lidar_vis.hip run -- on a
// case file and writes the grids, so that the test can hold them against the reference of tests/vis_refs.py byte for byte.  Plain C++ (the header needs
// no HIP type); built with -ffp-contract=off like the device object.
//   vis_driver in out [in out ...]
//   in:  int32  n_clouds, max_pts, stride, n_jobs, n_grids, has_origin, has_xform, has_idx
//        double voxel[3], extent_lo[3];  int32 dims[3], pad
//        float  pts[n_clouds][max_pts][stride];  int32 n_pts[n_clouds]
//        float  origin[n_jobs][3] (if has_origin);  float xform[n_jobs][12] (if has_xform);  int32 src[n_jobs], dst[n_jobs] (if has_idx)
//   out: uint32 trav_bits[n_grids][X][Y]
// Every ray is also walked band by band of 16 rows, as the LDS kernel does; a difference from the whole walk is error 7.
// The job loop restates v2x_lidar_freespace_bits' (a job naming a cloud or grid that does not exist is skipped; rays past min(n_pts, max_pts) are not read).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vis_math.h"

template <class T>
static bool rd(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static int run(const char *in, const char *out) {
    FILE *f = fopen(in, "rb");
    if (!f) return 2;
    int32_t h[8], dims[4];
    double vox[3], lo[3];
    if (fread(h, 4, 8, f) != 8 || fread(vox, 8, 3, f) != 3 || fread(lo, 8, 3, f) != 3 || fread(dims, 4, 4, f) != 4) return 3;
    const int n_clouds = h[0], max_pts = h[1], stride = h[2], n_jobs = h[3], n_grids = h[4];
    std::vector<float> pts, origin, xform;
    std::vector<int32_t> n_pts, src, dst;
    if (!rd(f, pts, (size_t)n_clouds * max_pts * stride) || !rd(f, n_pts, n_clouds) || !rd(f, origin, h[5] ? (size_t)n_jobs * 3 : 0) ||
        !rd(f, xform, h[6] ? (size_t)n_jobs * 12 : 0) || !rd(f, src, h[7] ? n_jobs : 0) || !rd(f, dst, h[7] ? n_jobs : 0))
        return 4;
    fclose(f);
    VisGrid g;
    for (int a = 0; a < 3; ++a) vis_grid_axis(g, a, vox[a], lo[a]);
    g.X = dims[0];
    g.Y = dims[1];
    g.Z = dims[2];
    std::vector<uint32_t> bits((size_t)n_grids * g.X * g.Y, 0u), banded(bits.size(), 0u);
    for (int j = 0; j < n_jobs; ++j) {
        const int cloud = h[7] ? src[j] : j, grid = h[7] ? dst[j] : j;
        if ((unsigned)cloud >= (unsigned)n_clouds || (unsigned)grid >= (unsigned)n_grids) continue;
        const int n = n_pts[cloud] < max_pts ? n_pts[cloud] : max_pts;
        uint32_t *b = bits.data() + (size_t)grid * g.X * g.Y;
        for (int i = 0; i < n; ++i) {
            double qo[3], qp[3];
            vis_ray(g, pts.data() + ((size_t)cloud * max_pts + i) * stride, h[5] ? origin.data() + (size_t)j * 3 : nullptr,
                    h[6] ? xform.data() + (size_t)j * 12 : nullptr, qo, qp);
            vis_walk(g.X, g.Y, g.Z, qo, qp, 0, g.X, [&](int ix, int iy, uint32_t mask) { b[(size_t)ix * g.Y + iy] |= mask; });
            // the LDS kernel's way: band by band of 16 rows, each band asking for its own rows only -- must be the same columns and masks
            uint32_t *b2 = banded.data() + (size_t)grid * g.X * g.Y;
            for (int r0 = 0; r0 < g.X; r0 += 16) {
                const int r1 = r0 + 16 < g.X ? r0 + 16 : g.X;
                vis_walk(g.X, g.Y, g.Z, qo, qp, r0, r1, [&](int ix, int iy, uint32_t mask) {
                    if (ix < r0 || ix >= r1) mask = 0xffffffffu;      // a row outside the band asked for: poison the grid, the comparison fails
                    b2[(size_t)ix * g.Y + iy] |= mask;
                });
            }
        }
    }
    if (bits != banded) return 7;
    FILE *o = fopen(out, "wb");
    if (!o) return 5;
    const bool ok = bits.empty() || fwrite(bits.data(), 4, bits.size(), o) == bits.size();
    return fclose(o) == 0 && ok ? 0 : 6;
}

int main(int argc, char **argv) {
    if (argc < 3 || (argc - 1) % 2) return 1;
    for (int a = 1; a + 1 < argc; a += 2) {
        const int rc = run(argv[a], argv[a + 1]);
        if (rc) {
            fprintf(stderr, "vis_driver: %s: error %d\n", argv[a], rc);
            return rc;
        }
    }
    return 0;
}

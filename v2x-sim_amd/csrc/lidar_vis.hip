// Row f-2 "visibility maps": the free-space half of a LiDAR sweep.  The voxeliser (a1) keeps where a sweep's returns END; this file walks every ray
// from the sensor origin to its return and sets the voxels it crossed (upstream's data preparation keeps them as `vis_maps`: occupied / free / unknown).
// The rule is DESIGN.md section 3.13 and lives in vis_math.h, shared with the host driver of tests/test_vis_refs_cpu.py.
//
//   v2x_lidar_freespace_bits   trav_bits [n_grids][X][Y] uint32, bit z = some ray of some job passed through voxel (x, y, z).  Jobs as in
//                              v2x_voxelize_fused_bits.  OR is idempotent: the result does not depend on the order, two calls give the same bytes.
//       general form           one ray per thread, one device-scope atomicOr per column into the cleared grid.
//       LDS form               the grid in LDS as 16-bit pixels, cut into bands of VIS_BAND_ROWS x rows: one workgroup per (grid, band) walks, of every
//                              ray of every job of its grid, the rows of its band only (a row of the walk depends on nothing but the ray and its
//                              index: the same columns, the same masks), with ds_or, and stores the band once as 16-byte words -- no memset pass.
//   v2x_vis_bits_to_dense_f32  occ / trav bits -> upstream's vis_maps layout [n][X][Y][Z] fp32 with three values.
//   v2x_vis_mask_labels        segmentation labels with the cells no ray observed set to the ignore class.
#include "common.h"
#include "vis_math.h"

struct VisJobs {
    const float *pts;
    const int32_t *n_pts;
    const float *origin, *xform;
    const int32_t *src, *dst;
    int n_clouds, max_pts, pt_stride, n_jobs, n_grids;
};

// the cloud and grid of job j, or false where either does not exist (src / dst are device data the host cannot inspect: such a job is skipped)
__device__ __forceinline__ bool vis_job(const VisJobs &J, int j, int &cloud, int &grid) {
    cloud = J.src ? J.src[j] : j;
    grid = J.dst ? J.dst[j] : j;
    return (unsigned)cloud < (unsigned)J.n_clouds && (unsigned)grid < (unsigned)J.n_grids;
}

__global__ __launch_bounds__(256) void freespace_scatter_kernel(VisJobs J, VisGrid vg, uint32_t *__restrict__ bits) {
    const int job = blockIdx.y;
    int cloud, g;
    if (!vis_job(J, job, cloud, g)) return;
    const int n = min(J.n_pts[cloud], J.max_pts);
    const float *base = J.pts + (size_t)cloud * J.max_pts * J.pt_stride;
    const float *m = J.xform ? J.xform + (size_t)job * 12 : nullptr;
    const float *org = J.origin ? J.origin + (size_t)job * 3 : nullptr;
    uint32_t *grid = bits + (size_t)g * vg.X * vg.Y;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        double qo[3], qp[3];
        vis_ray(vg, base + (size_t)i * J.pt_stride, org, m, qo, qp);
        vis_walk(vg.X, vg.Y, vg.Z, qo, qp, 0, vg.X, [&](int ix, int iy, uint32_t mask) { atomicOr(&grid[(size_t)ix * vg.Y + iy], mask); });
    }
}

constexpr int VIS_BAND_ROWS = 16;
constexpr int VIS_LDS_THREADS = 256;

__global__ __launch_bounds__(VIS_LDS_THREADS) void freespace_lds_kernel(VisJobs J, VisGrid vg, int n_bands, uint32_t *__restrict__ bits) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sband[];   // [rows * Y / 2]: two 16-bit pixels per word
    const int g = blockIdx.x / n_bands, band = blockIdx.x - g * n_bands;
    const int tid = threadIdx.x;
    const int row0 = band * VIS_BAND_ROWS, row1 = min(row0 + VIS_BAND_ROWS, vg.X);
    const int n_words = ((row1 - row0) * vg.Y) >> 1;                   // a multiple of 4 (the host checked X * Y % 8 == 0; row0 * Y is a multiple of 16)
    for (int i = tid * 4; i < n_words; i += VIS_LDS_THREADS * 4) *reinterpret_cast<uint4 *>(&sband[i]) = make_uint4(0, 0, 0, 0);
    __syncthreads();
    for (int job = 0; job < J.n_jobs; ++job) {
        int cloud, jg;
        if (!vis_job(J, job, cloud, jg) || jg != g) continue;         // workgroup-uniform
        const int n = min(J.n_pts[cloud], J.max_pts);
        const float *base = J.pts + (size_t)cloud * J.max_pts * J.pt_stride;
        const float *m = J.xform ? J.xform + (size_t)job * 12 : nullptr;
        const float *org = J.origin ? J.origin + (size_t)job * 3 : nullptr;
        for (int i = tid; i < n; i += VIS_LDS_THREADS) {
            double qo[3], qp[3];
            vis_ray(vg, base + (size_t)i * J.pt_stride, org, m, qo, qp);
            vis_walk(vg.X, vg.Y, vg.Z, qo, qp, row0, row1, [&](int ix, int iy, uint32_t mask) {
                const int pix = (ix - row0) * vg.Y + iy;
                atomicOr(&sband[pix >> 1], mask << ((pix & 1) * 16));
            });
        }
    }
    __syncthreads();
    uint32_t *out = bits + ((size_t)g * vg.X + row0) * vg.Y;
    for (int k = tid; k < (n_words >> 1); k += VIS_LDS_THREADS) {
        const uint2 w = *reinterpret_cast<const uint2 *>(&sband[2 * k]);
        *reinterpret_cast<uint4 *>(&out[4 * k]) = make_uint4(w.x & 0xffffu, w.x >> 16, w.y & 0xffffu, w.y >> 16);
    }
}

__global__ __launch_bounds__(256) void vis_bits_to_dense_f32_kernel(const uint32_t *__restrict__ occ, const uint32_t *__restrict__ trav, size_t n_pix, int Z,
                                                                    float v_occ, float v_free, float v_unknown, float *__restrict__ out) {
    const size_t total = n_pix * (size_t)Z;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t pix = i / Z;
        const int z = (int)(i - pix * Z);
        const uint32_t o = (occ[pix] >> z) & 1u, t = (trav[pix] >> z) & 1u;
        out[i] = o ? v_occ : (t ? v_free : v_unknown);
    }
}

// labels_out may be labels_in: every thread reads and writes its own element only
__global__ __launch_bounds__(256) void vis_mask_labels_kernel(const uint8_t *labels_in, const uint32_t *__restrict__ occ, const uint32_t *__restrict__ trav,
                                                              size_t n_pix, uint32_t z_mask, uint8_t ignore, uint8_t *labels_out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += (size_t)gridDim.x * blockDim.x)
        labels_out[i] = ((occ[i] | trav[i]) & z_mask) == 0 ? ignore : labels_in[i];
}

static inline int vis_grid_for(size_t total, int block) {
    size_t g = (total + block - 1) / block;
    if (g > 256 * 8) g = 256 * 8;
    if (g < 1) g = 1;
    return (int)g;
}

// Does the SHAPE take the LDS form?  The fused voxeliser's condition on the grid (16-bit pixels: Z <= 16; the whole grid within its 128 KiB LDS budget; 16-byte
// pieces) -- and nothing else: no switch, no count.
static inline bool vis_lds_shape(int X, int Y, int Z) { return Z <= 16 && (size_t)X * Y * 2 <= 128 * 1024 && ((size_t)X * Y) % 8 == 0; }

extern "C" int v2x_lidar_freespace_bits(const float *pts, const int32_t *n_pts, int n_clouds, int max_pts, int pt_stride, const float *origin,
                                        const float *xform, const int32_t *src_cloud, const int32_t *dst_grid, int n_jobs, int n_grids,
                                        const double *extents, const double *voxel, const int32_t *dims_xyz, uint32_t *trav_bits, v2x_stream_t stream) {
    V2X_REQUIRE(extents && voxel && dims_xyz && (trav_bits || n_grids == 0), "v2x_lidar_freespace_bits: null pointer");
    V2X_REQUIRE(n_clouds >= 0 && max_pts >= 0 && pt_stride >= 3 && n_jobs >= 0 && n_grids >= 0 && n_jobs <= 65535,
                "v2x_lidar_freespace_bits: bad sizes (stride >= 3, n_jobs <= 65535)");
    V2X_REQUIRE((src_cloud == nullptr) == (dst_grid == nullptr), "v2x_lidar_freespace_bits: src_cloud and dst_grid come together or not at all");
    V2X_REQUIRE(dims_xyz[2] >= 1 && dims_xyz[2] <= 32, "v2x_lidar_freespace_bits: Z=%d must be in [1,32]", dims_xyz[2]);
    V2X_REQUIRE(dims_xyz[0] >= 1 && dims_xyz[1] >= 1 && (long long)dims_xyz[0] * dims_xyz[1] <= (1ll << 30), "v2x_lidar_freespace_bits: bad grid dims");
    if (n_grids == 0) return V2X_OK;
    const bool work = n_jobs > 0 && max_pts > 0 && n_clouds > 0;
    V2X_REQUIRE(!work || (pts && n_pts), "v2x_lidar_freespace_bits: null pointer");
    hipStream_t s = (hipStream_t)stream;
    VisGrid vg;
    for (int a = 0; a < 3; ++a) {
        V2X_REQUIRE(voxel[a] > 0.0, "v2x_lidar_freespace_bits: voxel size must be > 0");
        vis_grid_axis(vg, a, voxel[a], extents[2 * a]);
    }
    vg.X = dims_xyz[0];
    vg.Y = dims_xyz[1];
    vg.Z = dims_xyz[2];
    const VisJobs J = {pts, n_pts, origin, xform, src_cloud, dst_grid, n_clouds, max_pts, pt_stride, n_jobs, n_grids};
    const int n_bands = (vg.X + VIS_BAND_ROWS - 1) / VIS_BAND_ROWS;
    if (work && vis_lds_shape(vg.X, vg.Y, vg.Z) && (reinterpret_cast<uintptr_t>(trav_bits) & 15) == 0 && (long long)n_grids * n_bands <= 0x7fffffffll) {
        const int rows = vg.X < VIS_BAND_ROWS ? vg.X : VIS_BAND_ROWS;
        const int lds_bytes = rows * vg.Y * 2;          // <= 128 KiB by vis_lds_shape
        return v2x_launch<freespace_lds_kernel, 128 * 1024>("freespace_lds_kernel", dim3((unsigned)(n_grids * n_bands)), dim3(VIS_LDS_THREADS), lds_bytes, s, J, vg,
                                                             n_bands, trav_bits);
    }
    if (hipMemsetAsync(trav_bits, 0, (size_t)n_grids * vg.X * vg.Y * sizeof(uint32_t), s) != hipSuccess) {
        v2x_set_error("v2x_lidar_freespace_bits: memset failed");
        return V2X_EIO;
    }
    if (!work) return V2X_OK;
    dim3 grid((max_pts + 255) / 256, n_jobs);
    if (grid.x > 256) grid.x = 256;
    return v2x_launch<freespace_scatter_kernel, 0>("freespace_scatter_kernel", grid, dim3(256), 0, s, J, vg, trav_bits);
}

extern "C" int v2x_vis_bits_to_dense_f32(const uint32_t *occ_bits, const uint32_t *trav_bits, int n, int X, int Y, int Z, float v_occ, float v_free,
                                         float v_unknown, float *out, v2x_stream_t stream) {
    V2X_REQUIRE(n >= 0 && X > 0 && Y > 0 && Z > 0 && Z <= 32, "v2x_vis_bits_to_dense_f32: bad dims");
    if (n == 0) return V2X_OK;
    V2X_REQUIRE(occ_bits && trav_bits && out, "v2x_vis_bits_to_dense_f32: null pointer");
    const size_t n_pix = (size_t)n * X * Y;
    return v2x_launch<vis_bits_to_dense_f32_kernel, 0>("vis_bits_to_dense_f32_kernel", dim3(vis_grid_for(n_pix * Z, 256)), dim3(256), 0, (hipStream_t)stream,
                                                       occ_bits, trav_bits, n_pix, Z, v_occ, v_free, v_unknown, out);
}

extern "C" int v2x_vis_mask_labels(const uint8_t *labels_in, const uint32_t *occ_bits, const uint32_t *trav_bits, int n, int X, int Y, uint32_t z_mask,
                                   int ignore, uint8_t *labels_out, v2x_stream_t stream) {
    V2X_REQUIRE(n >= 0 && X > 0 && Y > 0, "v2x_vis_mask_labels: bad dims");
    V2X_REQUIRE(ignore >= 0 && ignore <= 255, "v2x_vis_mask_labels: ignore=%d must be in [0,255]", ignore);
    if (n == 0) return V2X_OK;
    V2X_REQUIRE(labels_in && occ_bits && trav_bits && labels_out, "v2x_vis_mask_labels: null pointer");
    const size_t n_pix = (size_t)n * X * Y;
    return v2x_launch<vis_mask_labels_kernel, 0>("vis_mask_labels_kernel", dim3(vis_grid_for(n_pix, 256)), dim3(256), 0, (hipStream_t)stream, labels_in,
                                                 occ_bits, trav_bits, n_pix, z_mask, (uint8_t)ignore, labels_out);
}

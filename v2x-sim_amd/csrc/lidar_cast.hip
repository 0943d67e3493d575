// f-2 / f-3 -- synthetic scenes with occlusion: the sweeps of all agents of all frames of a step ray-cast against a scene of boxes, compacted into the
// (points, n_pts) form the voxeliser reads, with per-box return counts; and the ground truth those counts imply ("the cars this agent -- or any agent --
// got returns from", the num_lidar_pts rule of the real data preparation).  Build-owned spec: DESIGN.md section 3.12 ("LiDAR ray cast").  Two launches
// for all sweeps of a call (one more for the ground truth), no allocation, no host synchronisation; every output element is written.
//   THE RULE, in short (fp64 from the fp32 inputs, every product and sum rounded on its own; the host passes every angle as its cos / sin pair, no
//   trigonometric function is called for the geometry).  Ray r = b * NA + a: d = (ce*ca, ce*sa, se) in the sensor frame, w = (c*dx - s*dy, s*dx + c*dy,
//   dz) in the world, from o = (x, y, z).  Box g by slabs in its own frame: lx = px*cg + py*sg, ly = -px*sg + py*cg (p = o - centre), ux, uy alike from
//   w; x in [-w/2, w/2], y in [-h/2, h/2], z in [z0, z1]; an axis with u == 0 misses when l lies outside the closed slab and constrains nothing
//   otherwise; a hit iff t_near <= t_far and t_near > 0, at t_near.  Ground for dz < 0 at t = (ground_z - oz)/dz > 0.  The smallest t wins, the lowest
//   box index on ties, a box over the ground.  A return iff r_min <= t <= r_max and the draw (lidar_math.h) does not drop it; the point is t' * d with
//   t' = fmaf(sigma_r, normal, (float)t), in the sensor frame.
//   lidar_cast_kernel     one 256-thread workgroup per 256-ray chunk of a sweep.  Thread g reads box g of the sweep's frame, drops the invalid ones
//                         and puts the rest into LDS in box order (wave ballots + a prefix over the four waves), already relative to the sensor: (lx, ly,
//                         cg, sg, w/2, h/2, z0, z1, index).  Then a thread owns one ray and walks the boxes (LDS broadcast reads).  Per ray a record
//                         (t' bits, hit id or -1 without a return) and per chunk the number of returns go to the workspace.
//   lidar_compact_kernel  the same grid.  A workgroup sums the chunk counts of its sweep before its own (integer sums of a fixed table: the position of a
//                         return depends on nothing else), places its returns by ballot + prefix in ascending r, rebuilds the point from the record
//                         (direction and intensity are functions of (r, sweep) alone), and counts the kept returns per box (LDS counters, then integer
//                         atomics on box_hits, which the first kernel cleared).  The rows from n_pts on are zeroed by the sweep's workgroups together.
//   lidar_visible_kernel  one workgroup per sweep, thread g = box g: the three conditions, rows compacted in box order.
#include "common.h"
#include "lidar_math.h"

// the geometry is compared bit for bit with a host reference that rounds every operation (this file is also compiled with -ffp-contract=off: Makefile)
#pragma clang fp contract(off)

constexpr int LIDAR_MAX_BOX = 256;       // one box per thread in the load
constexpr int LIDAR_CHUNK = 256;         // rays per workgroup
constexpr int LIDAR_MAX_RAYS = 1 << 24;  // per sweep

struct lidar_args {
    const float *sensors;        // [n][6]
    const int32_t *frame_of;     // [n]
    const float *boxes;          // [F][cap][9]
    const int32_t *box_count;    // [F]
    int n_frames, cap;
    const float *beam, *az;      // [NB][2], [NA][2]
    int n_az, n_rays, n_chunks;
    float ground_z, r_min, r_max, sigma_r, p_drop;
    uint64_t seed, step;
    float *points;               // [n][max_pts][4]
    int32_t *n_pts;              // [n]
    int max_pts;
    int32_t *hit;                // [n][max_pts] or null
    int32_t *box_hits;           // [n][cap] or null
    uint2 *rec;                  // workspace [n][n_rays]: (bits of t', hit id or -1)
    int32_t *chunk_n;            // workspace [n][n_chunks]
};

__device__ __forceinline__ bool lidar_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ int lidar_count(const int32_t *box_count, int n_frames, int cap, int f) {
    if ((unsigned)f >= (unsigned)n_frames) return 0;           // a sweep of no frame sees an empty scene
    const int c = box_count[f];
    return c < 0 ? 0 : (c > cap ? cap : c);
}
__device__ __forceinline__ bool lidar_box_valid(const float (&b)[9]) {
    bool ok = b[2] >= 0.0f && b[3] >= 0.0f && b[8] >= b[7];
#pragma unroll
    for (int e = 0; e < 9; ++e) ok = ok && lidar_finite(b[e]);
    return ok;
}
// one axis of the slab test; false = the ray misses the box on this axis alone
__device__ __forceinline__ bool lidar_slab(double l, double u, double lo, double hi, double &t_near, double &t_far) {
    if (u == 0.0) return l >= lo && l <= hi;
    const double ta = (lo - l) / u, tb = (hi - l) / u;
    t_near = fmax(t_near, fmin(ta, tb));
    t_far = fmin(t_far, fmax(ta, tb));
    return true;
}
// sensor-frame direction of ray r
__device__ __forceinline__ void lidar_direction(const lidar_args &p, int r, double &dx, double &dy, double &dz) {
    const int bi = r / p.n_az, ai = r - bi * p.n_az;
    const double ce = (double)p.beam[2 * bi], se = (double)p.beam[2 * bi + 1], ca = (double)p.az[2 * ai], sa = (double)p.az[2 * ai + 1];
    dx = ce * ca;
    dy = ce * sa;
    dz = se;
}

__global__ __launch_bounds__(256) void lidar_cast_kernel(lidar_args p) {
    __shared__ double s_box[LIDAR_MAX_BOX][8];        // lx, ly, cg, sg, w/2, h/2, z0, z1
    __shared__ int s_index[LIDAR_MAX_BOX];
    __shared__ int s_wave_n[4], s_wave_ret[4];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int s = blockIdx.x / p.n_chunks, chunk = blockIdx.x - s * p.n_chunks;
    const float *sen = p.sensors + (size_t)s * 6;
    const double ox = (double)sen[0], oy = (double)sen[1], oz = (double)sen[2], cs = (double)sen[4], sn = (double)sen[5];
    const int f = p.frame_of[s];
    const int count = lidar_count(p.box_count, p.n_frames, p.cap, f);

    if (chunk == 0 && p.box_hits && tid < p.cap) p.box_hits[(size_t)s * p.cap + tid] = 0;     // the compaction launch adds to it

    // thread g = box g (count <= cap <= 256): the valid ones into LDS in box order, relative to this sensor
    bool live = false;
    float b[9];
    if (tid < count) {
        const float *src = p.boxes + ((size_t)f * p.cap + tid) * 9;
#pragma unroll
        for (int e = 0; e < 9; ++e) b[e] = src[e];
        live = lidar_box_valid(b);
    }
    const unsigned long long mask = __ballot(live);
    if (lane == 0) s_wave_n[wave] = __popcll(mask);
    __syncthreads();
    int base = 0, n_live = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) base += s_wave_n[w];
        n_live += s_wave_n[w];
    }
    if (live) {
        const int k = base + __popcll(mask & ((1ull << lane) - 1ull));
        const double px = ox - (double)b[0], py = oy - (double)b[1], cg = (double)b[5], sg = (double)b[6];
        s_box[k][0] = px * cg + py * sg;
        s_box[k][1] = -px * sg + py * cg;
        s_box[k][2] = cg;
        s_box[k][3] = sg;
        s_box[k][4] = (double)b[2] / 2.0;
        s_box[k][5] = (double)b[3] / 2.0;
        s_box[k][6] = (double)b[7];
        s_box[k][7] = (double)b[8];
        s_index[k] = tid;
    }
    __syncthreads();

    const int r = chunk * LIDAR_CHUNK + tid;
    bool ret = false;
    int id = -1;
    float t_rep = 0.0f;
    if (r < p.n_rays) {
        double dx, dy, dz;
        lidar_direction(p, r, dx, dy, dz);
        const double wx = cs * dx - sn * dy, wy = sn * dx + cs * dy;
        double best = __builtin_inf();
        for (int k = 0; k < n_live; ++k) {                // workgroup-uniform bound, LDS broadcast reads, ascending box index
            const double cg = s_box[k][2], sg = s_box[k][3], hw = s_box[k][4], hh = s_box[k][5];
            const double ux = wx * cg + wy * sg, uy = -wx * sg + wy * cg;
            double t_near = -__builtin_inf(), t_far = __builtin_inf();
            if (!lidar_slab(s_box[k][0], ux, -hw, hw, t_near, t_far)) continue;
            if (!lidar_slab(s_box[k][1], uy, -hh, hh, t_near, t_far)) continue;
            if (!(t_near <= t_far)) continue;             // the z slab can only narrow the interval
            if (!lidar_slab(oz, dz, s_box[k][6], s_box[k][7], t_near, t_far)) continue;
            if (t_near <= t_far && t_near > 0.0 && t_near < best) {
                best = t_near;
                id = 1 + s_index[k];
            }
        }
        if (dz < 0.0) {
            const double t = ((double)p.ground_z - oz) / dz;
            if (t > 0.0 && t < best) {                    // strictly: a box at the same t keeps the ray
                best = t;
                id = 0;
            }
        }
        if (id >= 0 && best >= (double)p.r_min && best <= (double)p.r_max) {
            const ChanWords d = lidar_words(p.seed, p.step, (uint32_t)s, (uint32_t)r);
            if (!lidar_dropped(d, p.p_drop)) {
                ret = true;
                t_rep = lidar_noisy_range(best, p.sigma_r, p.sigma_r != 0.0f ? lidar_normal(d) : 0.0f);
            }
        }
        p.rec[(size_t)s * p.n_rays + r] = make_uint2(__float_as_uint(t_rep), (uint32_t)(ret ? id : -1));
    }
    const unsigned long long rmask = __ballot(ret);
    if (lane == 0) s_wave_ret[wave] = __popcll(rmask);
    __syncthreads();
    if (tid == 0) p.chunk_n[blockIdx.x] = s_wave_ret[0] + s_wave_ret[1] + s_wave_ret[2] + s_wave_ret[3];
}

__global__ __launch_bounds__(256) void lidar_compact_kernel(lidar_args p) {
    __shared__ int s_before[4], s_total[4], s_wave_ret[4];
    __shared__ int s_hist[LIDAR_MAX_BOX];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int s = blockIdx.x / p.n_chunks, chunk = blockIdx.x - s * p.n_chunks;
    s_hist[tid] = 0;

    // returns of this sweep before this chunk, and in all of it
    int before = 0, total = 0;
    for (int c = tid; c < p.n_chunks; c += 256) {
        const int v = p.chunk_n[(size_t)s * p.n_chunks + c];
        total += v;
        if (c < chunk) before += v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        before += __shfl_xor(before, off);
        total += __shfl_xor(total, off);
    }
    const int r = chunk * LIDAR_CHUNK + tid;
    uint2 rec = make_uint2(0u, 0xffffffffu);
    if (r < p.n_rays) rec = p.rec[(size_t)s * p.n_rays + r];
    const int code = (int)rec.y;
    const bool ret = code >= 0;
    const unsigned long long rmask = __ballot(ret);
    if (lane == 0) {
        s_before[wave] = before;
        s_total[wave] = total;
        s_wave_ret[wave] = __popcll(rmask);
    }
    __syncthreads();
    before = s_before[0] + s_before[1] + s_before[2] + s_before[3];
    total = s_total[0] + s_total[1] + s_total[2] + s_total[3];
    const int n_keep = total < p.max_pts ? total : p.max_pts;
    int pos = before + __popcll(rmask & ((1ull << lane) - 1ull));
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (w < wave) pos += s_wave_ret[w];

    if (ret && pos < p.max_pts) {
        double dx, dy, dz;
        lidar_direction(p, r, dx, dy, dz);
        const double t = (double)__uint_as_float(rec.x);
        const ChanWords d = lidar_words(p.seed, p.step, (uint32_t)s, (uint32_t)r);
        float *out = p.points + ((size_t)s * p.max_pts + pos) * 4;
        out[0] = (float)(t * dx);
        out[1] = (float)(t * dy);
        out[2] = (float)(t * dz);
        out[3] = lidar_intensity(d);
        if (p.hit) p.hit[(size_t)s * p.max_pts + pos] = code;
        if (code >= 1) atomicAdd(&s_hist[code - 1], 1);       // code <= 256: the index of a box that sat in a 256-entry table
    }
    // the rows past the kept returns, shared among the sweep's workgroups
    for (long long j = (long long)n_keep + (long long)chunk * LIDAR_CHUNK + tid; j < p.max_pts; j += (long long)p.n_chunks * LIDAR_CHUNK) {
        float *out = p.points + ((size_t)s * p.max_pts + (size_t)j) * 4;
        out[0] = 0.0f;
        out[1] = 0.0f;
        out[2] = 0.0f;
        out[3] = 0.0f;
        if (p.hit) p.hit[(size_t)s * p.max_pts + (size_t)j] = -1;
    }
    if (chunk == 0 && tid == 0) p.n_pts[s] = n_keep;
    if (p.box_hits) {
        __syncthreads();
        if (tid < p.cap && s_hist[tid] != 0) atomicAdd(&p.box_hits[(size_t)s * p.cap + tid], s_hist[tid]);
    }
}

struct lidar_visible_args {
    const int32_t *box_hits;     // [n][cap]
    const float *sensors;        // [n][6]
    const int32_t *frame_of;     // [n]
    int n_sweeps;
    const float *boxes;          // [F][cap][9]
    const int32_t *box_count;    // [F]
    int n_frames, cap, min_hits, any_agent;
    float x_lim, y_lim;
    float *gt_boxes;             // [n][cap][5]
    int32_t *gt_count;           // [n]
};

__global__ __launch_bounds__(256) void lidar_visible_kernel(lidar_visible_args p) {
    __shared__ int s_wave_n[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, s = blockIdx.x;
    const float *sen = p.sensors + (size_t)s * 6;
    const int f = p.frame_of[s];
    const int count = lidar_count(p.box_count, p.n_frames, p.cap, f);

    bool keep = false;
    float row[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (tid < count) {
        float b[9];
        const float *src = p.boxes + ((size_t)f * p.cap + tid) * 9;
#pragma unroll
        for (int e = 0; e < 9; ++e) b[e] = src[e];
        int hits = p.box_hits[(size_t)s * p.cap + tid];
        if (p.any_agent)
            for (int q = 0; q < p.n_sweeps; ++q)
                if (p.frame_of[q] == f) hits = max(hits, p.box_hits[(size_t)q * p.cap + tid]);
        if (lidar_box_valid(b) && hits >= p.min_hits) {
            const double ox = (double)sen[0], oy = (double)sen[1], oz = (double)sen[2], cs = (double)sen[4], sn = (double)sen[5];
            const double ex = (double)b[0] - ox, ey = (double)b[1] - oy;
            const double x = ex * cs + ey * sn, y = -ex * sn + ey * cs;                      // R_s^T (c - o)
            const double px = ox - (double)b[0], py = oy - (double)b[1], cg = (double)b[5], sg = (double)b[6];
            const double lx = px * cg + py * sg, ly = -px * sg + py * cg;                    // the sensor origin in the box's frame, as the cast has it
            const bool inside = fabs(lx) <= (double)b[2] / 2.0 && fabs(ly) <= (double)b[3] / 2.0 && oz >= (double)b[7] && oz <= (double)b[8];
            if (fabs(x) < (double)p.x_lim && fabs(y) < (double)p.y_lim && !inside) {
                keep = true;
                row[0] = (float)x;
                row[1] = (float)y;
                row[2] = b[2];
                row[3] = b[3];
                row[4] = b[4] - sen[3];
            }
        }
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) s_wave_n[wave] = __popcll(mask);
    __syncthreads();
    int base = 0, n_keep = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) base += s_wave_n[w];
        n_keep += s_wave_n[w];
    }
    float *out = p.gt_boxes + (size_t)s * p.cap * 5;
    if (keep) {
        const int k = base + __popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
        for (int e = 0; e < 5; ++e) out[k * 5 + e] = row[e];
    }
    if (tid >= n_keep && tid < p.cap) {
#pragma unroll
        for (int e = 0; e < 5; ++e) out[tid * 5 + e] = 0.0f;
    }
    if (tid == 0) p.gt_count[s] = n_keep;
}

static bool lidar_aligned(const void *ptr, uintptr_t a) { return (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) == 0; }
static long long lidar_chunks(long long n_rays) { return (n_rays + LIDAR_CHUNK - 1) / LIDAR_CHUNK; }
static bool lidar_shape_ok(long long n_sweeps, int n_beams, int n_az, int box_cap) {
    if (n_sweeps < 0 || n_beams < 1 || n_az < 1 || box_cap < 1 || box_cap > LIDAR_MAX_BOX) return false;
    const long long n_rays = (long long)n_beams * n_az;
    return n_rays <= LIDAR_MAX_RAYS && (n_sweeps == 0 || lidar_chunks(n_rays) <= 0x7fffffffLL / n_sweeps);
}

extern "C" long long v2x_lidar_cast_workspace_size(long long n_sweeps, int n_beams, int n_az, int box_cap) {
    if (!lidar_shape_ok(n_sweeps, n_beams, n_az, box_cap)) return -1;
    const long long n_rays = (long long)n_beams * n_az;
    return n_sweeps * n_rays * (long long)sizeof(uint2) + n_sweeps * lidar_chunks(n_rays) * (long long)sizeof(int32_t);
}

extern "C" int v2x_lidar_cast(const float *sensors, const int32_t *frame_of, long long n_sweeps, const float *boxes, const int32_t *box_count, int n_frames,
                              int box_cap, const float *beam, int n_beams, const float *az, int n_az, float ground_z, float r_min, float r_max, float sigma_r,
                              float p_drop, uint64_t seed, uint64_t step, float *points, int32_t *n_pts, int max_pts, int32_t *hit, int32_t *box_hits,
                              void *workspace, long long workspace_bytes, v2x_stream_t stream) {
    if (n_sweeps == 0) return V2X_OK;
    V2X_REQUIRE(n_sweeps > 0, "v2x_lidar_cast: negative n_sweeps (%lld)", n_sweeps);
    V2X_REQUIRE(box_cap >= 1 && box_cap <= LIDAR_MAX_BOX, "v2x_lidar_cast: box_cap=%d must lie in [1, %d]", box_cap, LIDAR_MAX_BOX);
    V2X_REQUIRE(n_frames >= 1, "v2x_lidar_cast: n_frames=%d must be >= 1", n_frames);
    V2X_REQUIRE(max_pts > 0, "v2x_lidar_cast: max_pts=%d must be > 0", max_pts);
    V2X_REQUIRE(lidar_shape_ok(n_sweeps, n_beams, n_az, box_cap),
                "v2x_lidar_cast: n_sweeps=%lld, n_beams=%d, n_az=%d: sizes must be >= 1, n_beams*n_az <= 2^24 and n_sweeps*chunks < 2^31", n_sweeps, n_beams, n_az);
    V2X_REQUIRE(p_drop >= 0.0f && p_drop <= 1.0f, "v2x_lidar_cast: p_drop=%g must lie in [0, 1]", (double)p_drop);
    V2X_REQUIRE(sigma_r >= 0.0f && sigma_r <= 3.0e38f, "v2x_lidar_cast: sigma_r=%g must be finite and >= 0", (double)sigma_r);
    V2X_REQUIRE(r_min <= r_max, "v2x_lidar_cast: r_min (%g) <= r_max (%g) needed", (double)r_min, (double)r_max);
    V2X_REQUIRE(ground_z >= -3.0e38f && ground_z <= 3.0e38f, "v2x_lidar_cast: ground_z=%g must be finite", (double)ground_z);
    V2X_REQUIRE(sensors && frame_of && boxes && box_count && beam && az && points && n_pts,
                "v2x_lidar_cast: null pointer (only hit and box_hits may be null)");
    const long long need = v2x_lidar_cast_workspace_size(n_sweeps, n_beams, n_az, box_cap);
    V2X_REQUIRE(workspace && workspace_bytes >= need, "v2x_lidar_cast: workspace of %lld bytes, %lld needed", workspace ? workspace_bytes : 0LL, need);
    V2X_REQUIRE(lidar_aligned(workspace, 8), "v2x_lidar_cast: workspace must be 8-byte aligned");
    V2X_REQUIRE(lidar_aligned(sensors, 4) && lidar_aligned(frame_of, 4) && lidar_aligned(boxes, 4) && lidar_aligned(box_count, 4) && lidar_aligned(beam, 4) &&
                    lidar_aligned(az, 4) && lidar_aligned(points, 4) && lidar_aligned(n_pts, 4) && lidar_aligned(hit, 4) && lidar_aligned(box_hits, 4),
                "v2x_lidar_cast: int32 / fp32 arrays must be 4-byte aligned");
    const int n_rays = n_beams * n_az, n_chunks = (int)lidar_chunks(n_rays);
    uint2 *rec = static_cast<uint2 *>(workspace);
    const lidar_args p = {sensors, frame_of, boxes, box_count, n_frames, box_cap, beam, az, n_az, n_rays, n_chunks, ground_z, r_min, r_max, sigma_r, p_drop,
                          seed, step, points, n_pts, max_pts, hit, box_hits, rec, reinterpret_cast<int32_t *>(rec + (size_t)n_sweeps * n_rays)};
    const dim3 grid((unsigned)(n_sweeps * n_chunks));
    const int rc = v2x_launch<lidar_cast_kernel, 0>("lidar_cast_kernel", grid, dim3(256), 0, (hipStream_t)stream, p);
    if (rc != V2X_OK) return rc;
    return v2x_launch<lidar_compact_kernel, 0>("lidar_compact_kernel", grid, dim3(256), 0, (hipStream_t)stream, p);
}

extern "C" int v2x_lidar_visible_boxes(const int32_t *box_hits, const float *sensors, const int32_t *frame_of, long long n_sweeps, const float *boxes,
                                       const int32_t *box_count, int n_frames, int box_cap, int min_hits, int any_agent, float x_lim, float y_lim,
                                       float *gt_boxes, int32_t *gt_count, v2x_stream_t stream) {
    if (n_sweeps == 0) return V2X_OK;
    V2X_REQUIRE(n_sweeps > 0 && n_sweeps <= 0x7fffffffLL, "v2x_lidar_visible_boxes: n_sweeps=%lld must lie in [0, 2^31)", n_sweeps);
    V2X_REQUIRE(box_cap >= 1 && box_cap <= LIDAR_MAX_BOX, "v2x_lidar_visible_boxes: box_cap=%d must lie in [1, %d]", box_cap, LIDAR_MAX_BOX);
    V2X_REQUIRE(n_frames >= 1, "v2x_lidar_visible_boxes: n_frames=%d must be >= 1", n_frames);
    V2X_REQUIRE(x_lim > 0.0f && y_lim > 0.0f, "v2x_lidar_visible_boxes: x_lim (%g) and y_lim (%g) must be > 0", (double)x_lim, (double)y_lim);
    V2X_REQUIRE(box_hits && sensors && frame_of && boxes && box_count && gt_boxes && gt_count, "v2x_lidar_visible_boxes: null pointer");
    V2X_REQUIRE(lidar_aligned(box_hits, 4) && lidar_aligned(sensors, 4) && lidar_aligned(frame_of, 4) && lidar_aligned(boxes, 4) && lidar_aligned(box_count, 4) &&
                    lidar_aligned(gt_boxes, 4) && lidar_aligned(gt_count, 4),
                "v2x_lidar_visible_boxes: int32 / fp32 arrays must be 4-byte aligned");
    const lidar_visible_args p = {box_hits, sensors, frame_of, (int)n_sweeps, boxes, box_count, n_frames, box_cap, min_hits, any_agent, x_lim, y_lim, gt_boxes,
                                  gt_count};
    return v2x_launch<lidar_visible_kernel, 0>("lidar_visible_kernel", dim3((unsigned)n_sweeps), dim3(256), 0, (hipStream_t)stream, p);
}

// ---- moving scenes (DESIGN.md section 3.12 "moving scenes") ---------------------------------------------------------------------------------------
// Every box and every sensor moves in a straight line at constant velocity with a fixed yaw; sensors / boxes give the poses at time 0.  A sweep takes
// time: ray r = b * NA + a of sweep s is cast at T = (double)time_of[s] + (double)az_time[a] (lidar_math.h), against the boxes where they are THEN.
//   THE RULE.  For box g with q = (vsx - vgx, vsy - vgy) (sensor minus box, fp64 from the fp32 velocities): lx0 = px*cg + py*sg, ly0 = -px*sg + py*cg
//   with p = o0 - c0 exactly as the static rule has them; dlx = qx*cg + qy*sg, dly = -qx*sg + qy*cg; lx = lx0 + dlx*T, ly = ly0 + dly*T, every product
//   and sum rounded on its own.  Everything else is the static rule at the ray's own time: w, ux, uy, the z slab with lz = oz (no vertical motion),
//   the ground, the winner and its ties, r_min / r_max, the draw on (seed, step, sweep, ray), the point t' * d in the SENSOR frame at the ray's time
//   (a raw sweep: no ego-motion compensation).  A box whose velocity equals the sensor's has q = 0 exactly and is met as if both stood still.
//   A box with a non-finite velocity is dropped, keeping its index.  A sweep whose time_of or sensor_vel is not finite meets no box and has no ground
//   truth; a ray whose az_time is not finite meets no box; the ground, which does not move, still answers both.
//   lidar_cast_moving_kernel     lidar_cast_kernel's grid, box load, ballot and prefix; an LDS row carries dlx, dly after the static eight.  It writes
//                                the same per-ray record and per-chunk counts, so lidar_compact_kernel follows it unchanged.
//   lidar_visible_moving_kernel  one workgroup per sweep, thread g = box g, at T_ref = (double)time_of[s] + (double)t_ref.
struct lidar_moving_args {
    lidar_args base;
    const float *box_vel;        // [F][cap][2]
    const float *sensor_vel;     // [n][2]
    const float *time_of;        // [n]
    const float *az_time;        // [NA]
};

__global__ __launch_bounds__(256) void lidar_cast_moving_kernel(lidar_moving_args m) {
    __shared__ double s_box[LIDAR_MAX_BOX][10];       // lx0, ly0, cg, sg, w/2, h/2, z0, z1, dlx, dly
    __shared__ int s_index[LIDAR_MAX_BOX];
    __shared__ int s_wave_n[4], s_wave_ret[4];

    const lidar_args &p = m.base;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int s = blockIdx.x / p.n_chunks, chunk = blockIdx.x - s * p.n_chunks;
    const float *sen = p.sensors + (size_t)s * 6;
    const double ox = (double)sen[0], oy = (double)sen[1], oz = (double)sen[2], cs = (double)sen[4], sn = (double)sen[5];
    const float vsx = m.sensor_vel[(size_t)s * 2], vsy = m.sensor_vel[(size_t)s * 2 + 1], t0 = m.time_of[s];
    const bool sweep_ok = lidar_finite(vsx) && lidar_finite(vsy) && lidar_finite(t0);
    const int f = p.frame_of[s];
    const int count = lidar_count(p.box_count, p.n_frames, p.cap, f);

    if (chunk == 0 && p.box_hits && tid < p.cap) p.box_hits[(size_t)s * p.cap + tid] = 0;     // the compaction launch adds to it

    bool live = false;
    float b[9], vgx = 0.0f, vgy = 0.0f;
    if (tid < count) {
        const float *src = p.boxes + ((size_t)f * p.cap + tid) * 9;
#pragma unroll
        for (int e = 0; e < 9; ++e) b[e] = src[e];
        vgx = m.box_vel[((size_t)f * p.cap + tid) * 2];
        vgy = m.box_vel[((size_t)f * p.cap + tid) * 2 + 1];
        live = sweep_ok && lidar_box_valid(b) && lidar_finite(vgx) && lidar_finite(vgy);
    }
    const unsigned long long mask = __ballot(live);
    if (lane == 0) s_wave_n[wave] = __popcll(mask);
    __syncthreads();
    int base = 0, n_live = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) base += s_wave_n[w];
        n_live += s_wave_n[w];
    }
    if (live) {
        const int k = base + __popcll(mask & ((1ull << lane) - 1ull));
        const double px = ox - (double)b[0], py = oy - (double)b[1], cg = (double)b[5], sg = (double)b[6];
        const double qx = (double)vsx - (double)vgx, qy = (double)vsy - (double)vgy;
        s_box[k][0] = px * cg + py * sg;
        s_box[k][1] = -px * sg + py * cg;
        s_box[k][2] = cg;
        s_box[k][3] = sg;
        s_box[k][4] = (double)b[2] / 2.0;
        s_box[k][5] = (double)b[3] / 2.0;
        s_box[k][6] = (double)b[7];
        s_box[k][7] = (double)b[8];
        s_box[k][8] = qx * cg + qy * sg;
        s_box[k][9] = -qx * sg + qy * cg;
        s_index[k] = tid;
    }
    __syncthreads();

    const int r = chunk * LIDAR_CHUNK + tid;
    bool ret = false;
    int id = -1;
    float t_rep = 0.0f;
    if (r < p.n_rays) {
        double dx, dy, dz;
        lidar_direction(p, r, dx, dy, dz);
        const float ta = m.az_time[r % p.n_az];
        const double T = lidar_ray_time(t0, ta);
        const int n_box = lidar_finite(ta) ? n_live : 0;      // a ray without a time meets the ground alone
        const double wx = cs * dx - sn * dy, wy = sn * dx + cs * dy;
        double best = __builtin_inf();
        for (int k = 0; k < n_box; ++k) {                     // LDS broadcast reads, ascending box index
            const double cg = s_box[k][2], sg = s_box[k][3], hw = s_box[k][4], hh = s_box[k][5];
            const double ux = wx * cg + wy * sg, uy = -wx * sg + wy * cg;
            const double lx = lidar_moved(s_box[k][0], s_box[k][8], T), ly = lidar_moved(s_box[k][1], s_box[k][9], T);
            double t_near = -__builtin_inf(), t_far = __builtin_inf();
            if (!lidar_slab(lx, ux, -hw, hw, t_near, t_far)) continue;
            if (!lidar_slab(ly, uy, -hh, hh, t_near, t_far)) continue;
            if (!(t_near <= t_far)) continue;                 // the z slab can only narrow the interval
            if (!lidar_slab(oz, dz, s_box[k][6], s_box[k][7], t_near, t_far)) continue;
            if (t_near <= t_far && t_near > 0.0 && t_near < best) {
                best = t_near;
                id = 1 + s_index[k];
            }
        }
        if (dz < 0.0) {
            const double t = ((double)p.ground_z - oz) / dz;
            if (t > 0.0 && t < best) {                        // strictly: a box at the same t keeps the ray
                best = t;
                id = 0;
            }
        }
        if (id >= 0 && best >= (double)p.r_min && best <= (double)p.r_max) {
            const ChanWords d = lidar_words(p.seed, p.step, (uint32_t)s, (uint32_t)r);
            if (!lidar_dropped(d, p.p_drop)) {
                ret = true;
                t_rep = lidar_noisy_range(best, p.sigma_r, p.sigma_r != 0.0f ? lidar_normal(d) : 0.0f);
            }
        }
        p.rec[(size_t)s * p.n_rays + r] = make_uint2(__float_as_uint(t_rep), (uint32_t)(ret ? id : -1));
    }
    const unsigned long long rmask = __ballot(ret);
    if (lane == 0) s_wave_ret[wave] = __popcll(rmask);
    __syncthreads();
    if (tid == 0) p.chunk_n[blockIdx.x] = s_wave_ret[0] + s_wave_ret[1] + s_wave_ret[2] + s_wave_ret[3];
}

struct lidar_visible_moving_args {
    lidar_visible_args base;
    const float *box_vel;        // [F][cap][2]
    const float *sensor_vel;     // [n][2]
    const float *time_of;        // [n]
    float t_ref;
    int32_t *gt_ids;             // [n][cap]
    float *gt_vel;               // [n][cap][2] or null
};

__global__ __launch_bounds__(256) void lidar_visible_moving_kernel(lidar_visible_moving_args m) {
    __shared__ int s_wave_n[4];
    const lidar_visible_args &p = m.base;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, s = blockIdx.x;
    const float *sen = p.sensors + (size_t)s * 6;
    const float vsx = m.sensor_vel[(size_t)s * 2], vsy = m.sensor_vel[(size_t)s * 2 + 1], t0 = m.time_of[s];
    const bool sweep_ok = lidar_finite(vsx) && lidar_finite(vsy) && lidar_finite(t0);
    const int f = p.frame_of[s];
    const int count = lidar_count(p.box_count, p.n_frames, p.cap, f);

    bool keep = false;
    float row[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, vel[2] = {0.0f, 0.0f};
    if (tid < count && sweep_ok) {
        float b[9];
        const float *src = p.boxes + ((size_t)f * p.cap + tid) * 9;
#pragma unroll
        for (int e = 0; e < 9; ++e) b[e] = src[e];
        const float vgx = m.box_vel[((size_t)f * p.cap + tid) * 2], vgy = m.box_vel[((size_t)f * p.cap + tid) * 2 + 1];
        int hits = p.box_hits[(size_t)s * p.cap + tid];
        if (p.any_agent)                                      // the sweeps of the same world AT THE SAME TIME (fp32 equality of time_of)
            for (int q = 0; q < p.n_sweeps; ++q)
                if (p.frame_of[q] == f && m.time_of[q] == t0) hits = max(hits, p.box_hits[(size_t)q * p.cap + tid]);
        if (lidar_box_valid(b) && lidar_finite(vgx) && lidar_finite(vgy) && hits >= p.min_hits) {
            const double ox = (double)sen[0], oy = (double)sen[1], oz = (double)sen[2], cs = (double)sen[4], sn = (double)sen[5];
            const double T = lidar_ray_time(t0, m.t_ref);
            const double ex = lidar_rel_centre((double)b[0], ox, (double)vgx, (double)vsx, T);
            const double ey = lidar_rel_centre((double)b[1], oy, (double)vgy, (double)vsy, T);
            const double x = ex * cs + ey * sn, y = -ex * sn + ey * cs;                      // R_s^T (c - o) at T_ref
            const double px = ox - (double)b[0], py = oy - (double)b[1], cg = (double)b[5], sg = (double)b[6];
            const double qx = (double)vsx - (double)vgx, qy = (double)vsy - (double)vgy;
            const double lx = lidar_moved(px * cg + py * sg, qx * cg + qy * sg, T), ly = lidar_moved(-px * sg + py * cg, -qx * sg + qy * cg, T);
            const bool inside = fabs(lx) <= (double)b[2] / 2.0 && fabs(ly) <= (double)b[3] / 2.0 && oz >= (double)b[7] && oz <= (double)b[8];
            if (fabs(x) < (double)p.x_lim && fabs(y) < (double)p.y_lim && !inside) {
                const double rvx = (double)vgx - (double)vsx, rvy = (double)vgy - (double)vsy;
                keep = true;
                row[0] = (float)x;
                row[1] = (float)y;
                row[2] = b[2];
                row[3] = b[3];
                row[4] = b[4] - sen[3];
                vel[0] = (float)(rvx * cs + rvy * sn);
                vel[1] = (float)(-rvx * sn + rvy * cs);
            }
        }
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) s_wave_n[wave] = __popcll(mask);
    __syncthreads();
    int base = 0, n_keep = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) base += s_wave_n[w];
        n_keep += s_wave_n[w];
    }
    float *out = p.gt_boxes + (size_t)s * p.cap * 5;
    int32_t *ids = m.gt_ids + (size_t)s * p.cap;
    float *ov = m.gt_vel ? m.gt_vel + (size_t)s * p.cap * 2 : nullptr;
    if (keep) {                                               // k <= tid < cap
        const int k = base + __popcll(mask & ((1ull << lane) - 1ull));
#pragma unroll
        for (int e = 0; e < 5; ++e) out[k * 5 + e] = row[e];
        ids[k] = tid;
        if (ov) {
            ov[k * 2] = vel[0];
            ov[k * 2 + 1] = vel[1];
        }
    }
    if (tid >= n_keep && tid < p.cap) {
#pragma unroll
        for (int e = 0; e < 5; ++e) out[tid * 5 + e] = 0.0f;
        ids[tid] = -1;
        if (ov) {
            ov[tid * 2] = 0.0f;
            ov[tid * 2 + 1] = 0.0f;
        }
    }
    if (tid == 0) p.gt_count[s] = n_keep;
}

extern "C" int v2x_lidar_cast_moving(const float *sensors, const float *sensor_vel, const float *time_of, const int32_t *frame_of, long long n_sweeps,
                                     const float *boxes, const float *box_vel, const int32_t *box_count, int n_frames, int box_cap, const float *beam,
                                     int n_beams, const float *az, const float *az_time, int n_az, float ground_z, float r_min, float r_max, float sigma_r,
                                     float p_drop, uint64_t seed, uint64_t step, float *points, int32_t *n_pts, int max_pts, int32_t *hit,
                                     int32_t *box_hits, void *workspace, long long workspace_bytes, v2x_stream_t stream) {
    if (n_sweeps == 0) return V2X_OK;
    V2X_REQUIRE(n_sweeps > 0, "v2x_lidar_cast_moving: negative n_sweeps (%lld)", n_sweeps);
    V2X_REQUIRE(box_cap >= 1 && box_cap <= LIDAR_MAX_BOX, "v2x_lidar_cast_moving: box_cap=%d must lie in [1, %d]", box_cap, LIDAR_MAX_BOX);
    V2X_REQUIRE(n_frames >= 1, "v2x_lidar_cast_moving: n_frames=%d must be >= 1", n_frames);
    V2X_REQUIRE(max_pts > 0, "v2x_lidar_cast_moving: max_pts=%d must be > 0", max_pts);
    V2X_REQUIRE(lidar_shape_ok(n_sweeps, n_beams, n_az, box_cap),
                "v2x_lidar_cast_moving: n_sweeps=%lld, n_beams=%d, n_az=%d: sizes must be >= 1, n_beams*n_az <= 2^24 and n_sweeps*chunks < 2^31", n_sweeps,
                n_beams, n_az);
    V2X_REQUIRE(p_drop >= 0.0f && p_drop <= 1.0f, "v2x_lidar_cast_moving: p_drop=%g must lie in [0, 1]", (double)p_drop);
    V2X_REQUIRE(sigma_r >= 0.0f && sigma_r <= 3.0e38f, "v2x_lidar_cast_moving: sigma_r=%g must be finite and >= 0", (double)sigma_r);
    V2X_REQUIRE(r_min <= r_max, "v2x_lidar_cast_moving: r_min (%g) <= r_max (%g) needed", (double)r_min, (double)r_max);
    V2X_REQUIRE(ground_z >= -3.0e38f && ground_z <= 3.0e38f, "v2x_lidar_cast_moving: ground_z=%g must be finite", (double)ground_z);
    V2X_REQUIRE(sensors && sensor_vel && time_of && frame_of && boxes && box_vel && box_count && beam && az && az_time && points && n_pts,
                "v2x_lidar_cast_moving: null pointer (only hit and box_hits may be null)");
    const long long need = v2x_lidar_cast_workspace_size(n_sweeps, n_beams, n_az, box_cap);
    V2X_REQUIRE(workspace && workspace_bytes >= need, "v2x_lidar_cast_moving: workspace of %lld bytes, %lld needed", workspace ? workspace_bytes : 0LL, need);
    V2X_REQUIRE(lidar_aligned(workspace, 8), "v2x_lidar_cast_moving: workspace must be 8-byte aligned");
    V2X_REQUIRE(lidar_aligned(sensors, 4) && lidar_aligned(sensor_vel, 4) && lidar_aligned(time_of, 4) && lidar_aligned(frame_of, 4) && lidar_aligned(boxes, 4) &&
                    lidar_aligned(box_vel, 4) && lidar_aligned(box_count, 4) && lidar_aligned(beam, 4) && lidar_aligned(az, 4) && lidar_aligned(az_time, 4) &&
                    lidar_aligned(points, 4) && lidar_aligned(n_pts, 4) && lidar_aligned(hit, 4) && lidar_aligned(box_hits, 4),
                "v2x_lidar_cast_moving: int32 / fp32 arrays must be 4-byte aligned");
    const int n_rays = n_beams * n_az, n_chunks = (int)lidar_chunks(n_rays);
    uint2 *rec = static_cast<uint2 *>(workspace);
    const lidar_moving_args m = {{sensors, frame_of, boxes, box_count, n_frames, box_cap, beam, az, n_az, n_rays, n_chunks, ground_z, r_min, r_max, sigma_r,
                                  p_drop, seed, step, points, n_pts, max_pts, hit, box_hits, rec, reinterpret_cast<int32_t *>(rec + (size_t)n_sweeps * n_rays)},
                                 box_vel, sensor_vel, time_of, az_time};
    const dim3 grid((unsigned)(n_sweeps * n_chunks));
    const int rc = v2x_launch<lidar_cast_moving_kernel, 0>("lidar_cast_moving_kernel", grid, dim3(256), 0, (hipStream_t)stream, m);
    if (rc != V2X_OK) return rc;
    return v2x_launch<lidar_compact_kernel, 0>("lidar_compact_kernel", grid, dim3(256), 0, (hipStream_t)stream, m.base);
}

extern "C" int v2x_lidar_visible_boxes_moving(const int32_t *box_hits, const float *sensors, const float *sensor_vel, const float *time_of, float t_ref,
                                              const int32_t *frame_of, long long n_sweeps, const float *boxes, const float *box_vel, const int32_t *box_count,
                                              int n_frames, int box_cap, int min_hits, int any_agent, float x_lim, float y_lim, float *gt_boxes,
                                              int32_t *gt_count, int32_t *gt_ids, float *gt_vel, v2x_stream_t stream) {
    if (n_sweeps == 0) return V2X_OK;
    V2X_REQUIRE(n_sweeps > 0 && n_sweeps <= 0x7fffffffLL, "v2x_lidar_visible_boxes_moving: n_sweeps=%lld must lie in [0, 2^31)", n_sweeps);
    V2X_REQUIRE(box_cap >= 1 && box_cap <= LIDAR_MAX_BOX, "v2x_lidar_visible_boxes_moving: box_cap=%d must lie in [1, %d]", box_cap, LIDAR_MAX_BOX);
    V2X_REQUIRE(n_frames >= 1, "v2x_lidar_visible_boxes_moving: n_frames=%d must be >= 1", n_frames);
    V2X_REQUIRE(x_lim > 0.0f && y_lim > 0.0f, "v2x_lidar_visible_boxes_moving: x_lim (%g) and y_lim (%g) must be > 0", (double)x_lim, (double)y_lim);
    V2X_REQUIRE(t_ref >= -3.0e38f && t_ref <= 3.0e38f, "v2x_lidar_visible_boxes_moving: t_ref=%g must be finite", (double)t_ref);
    V2X_REQUIRE(box_hits && sensors && sensor_vel && time_of && frame_of && boxes && box_vel && box_count && gt_boxes && gt_count && gt_ids,
                "v2x_lidar_visible_boxes_moving: null pointer (only gt_vel may be null)");
    V2X_REQUIRE(lidar_aligned(box_hits, 4) && lidar_aligned(sensors, 4) && lidar_aligned(sensor_vel, 4) && lidar_aligned(time_of, 4) && lidar_aligned(frame_of, 4) &&
                    lidar_aligned(boxes, 4) && lidar_aligned(box_vel, 4) && lidar_aligned(box_count, 4) && lidar_aligned(gt_boxes, 4) &&
                    lidar_aligned(gt_count, 4) && lidar_aligned(gt_ids, 4) && lidar_aligned(gt_vel, 4),
                "v2x_lidar_visible_boxes_moving: int32 / fp32 arrays must be 4-byte aligned");
    const lidar_visible_moving_args m = {{box_hits, sensors, frame_of, (int)n_sweeps, boxes, box_count, n_frames, box_cap, min_hits, any_agent, x_lim, y_lim,
                                          gt_boxes, gt_count},
                                         box_vel, sensor_vel, time_of, t_ref, gt_ids, gt_vel};
    return v2x_launch<lidar_visible_moving_kernel, 0>("lidar_visible_moving_kernel", dim3((unsigned)n_sweeps), dim3(256), 0, (hipStream_t)stream, m);
}

// a8 / f-3 -- segmentation training targets: the annotated boxes of every item of a batch painted into the per-cell class map bev_seg (upstream does
// this once, when the data is created: create_data_seg.py; utils/synthetic_scene.seg_labels is the one-class host loop it replaces).  Build-owned
// spec: DESIGN.md section 3.8 ("Box rasterization").  At most two launches for all items of a call, no global atomics, no allocation, no host
// synchronisation; every output element is written.
//   THE RULE.  Cell (i, j) has the centre px = x0 + (i + 0.5) * vx, py = y0 + (j + 0.5) * vy.  Box g = (x, y, w, h, yaw) covers it iff |lx| <= w/2
//   and |ly| <= h/2 with lx = (px-x)*c + (py-y)*s, ly = -(px-x)*s + (py-y)*c, c = cos(yaw), s = sin(yaw): fp64 from the fp32 inputs, every product
//   and sum rounded on its own (no fused multiply-add), borders closed.  A box with a non-finite field or a negative extent is dropped; a zero extent
//   is valid.  Among the boxes that cover a cell the greatest rank wins, the lowest box index on ties: class 0 never paints, class c in [1, n_cls)
//   has rank[c] (c itself without a table) and paints c, a class >= n_cls paints the ignore label 255 and outranks every class.  Uncovered: 0.
//   raster_tile_kernel    one 256-thread workgroup per 16 x 16 tile of cells and item.  Thread g reads box g and culls it against the tile: the box's
//                         bounding circle against the rectangle of the tile's cell centres, with slack on the safe side.  The survivors go into LDS in
//                         box order (wave ballots + a prefix over the four waves) as (x, y, c, s, w/2, h/2, rank, label, index) -- the trigonometry is
//                         done once per box and tile.  Then a thread owns one cell (iy along the lanes: 16-byte runs of labels) and walks the
//                         survivors.  With a histogram: LDS integer counters per workgroup, copied to workspace slot [item][tile][n_cls + 1].
//   raster_hist_kernel    one workgroup per item: a wave per label folds the tile slots into hist (integer sums: order-free).
#include "common.h"

// the coverage arithmetic is compared bit for bit with a host reference that rounds every operation
#pragma clang fp contract(off)

constexpr int RASTER_MAX_BOX = 256;     // one box per thread in the cull
constexpr int RASTER_TILE = 16;
constexpr int RASTER_MAX_CLS = 32;
constexpr int RASTER_IGNORE = 255;
// The cull compares squared fp64 distances; the slack keeps it on the safe side of their rounding (a box it lets through is decided per cell).
constexpr double RASTER_CULL_SLACK = 1.0 + 1e-9;

struct raster_args {
    const float *boxes;         // [n][cap][5]
    const uint8_t *cls;         // [n][cap]
    const int32_t *count;       // [n]
    const uint8_t *rank;        // [n_cls] or null
    int cap, X, Y, n_cls, tiles_y, tiles;
    float x0, y0, vx, vy;
    uint8_t *labels;            // [n][X][Y]
    int32_t *owner;             // [n][X][Y] or null
    int32_t *ws;                // [n][tiles][n_cls + 1] or null (no histogram)
};

__device__ __forceinline__ bool raster_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ int raster_count(const raster_args &p, int item) {
    const int c = p.count[item];
    return c < 0 ? 0 : (c > p.cap ? p.cap : c);
}
__device__ __forceinline__ double raster_centre(float origin, int i, float step) { return (double)origin + ((double)i + 0.5) * (double)step; }

__global__ __launch_bounds__(256) void raster_tile_kernel(raster_args p) {
    __shared__ double s_geo[RASTER_MAX_BOX][6];       // x, y, cos, sin, w/2, h/2
    __shared__ int s_rank[RASTER_MAX_BOX], s_index[RASTER_MAX_BOX];
    __shared__ uint8_t s_label[RASTER_MAX_BOX];
    __shared__ int s_wave_n[4];
    __shared__ int s_hist[RASTER_MAX_CLS + 1];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int item = blockIdx.x / p.tiles, tile = blockIdx.x - item * p.tiles;
    const int tx = tile / p.tiles_y, ty = tile - tx * p.tiles_y;
    const int ix = tx * RASTER_TILE + (tid >> 4), iy = ty * RASTER_TILE + (tid & 15);
    const bool active = ix < p.X && iy < p.Y;
    const int count = raster_count(p, item);
    if (tid <= RASTER_MAX_CLS) s_hist[tid] = 0;

    // the cull: thread g = box g (count <= cap <= 256) against the rectangle the tile's cell centres span
    bool live = false;
    float b[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    int rank = 0, label = 0;
    if (tid < count) {
        const float *src = p.boxes + ((size_t)item * p.cap + tid) * 5;
#pragma unroll
        for (int e = 0; e < 5; ++e) b[e] = src[e];
        const int c = p.cls[(size_t)item * p.cap + tid];
        const bool valid = raster_finite(b[0]) && raster_finite(b[1]) && raster_finite(b[2]) && raster_finite(b[3]) && raster_finite(b[4]) &&
                           b[2] >= 0.0f && b[3] >= 0.0f;
        if (valid && c != 0) {                            // class 0 never paints
            if (c >= p.n_cls) {
                rank = 256;                               // above every uint8 rank
                label = RASTER_IGNORE;
            } else {
                rank = p.rank ? (int)p.rank[c] : c;
                label = c;
            }
            const int ix1 = min(tx * RASTER_TILE + RASTER_TILE - 1, p.X - 1), iy1 = min(ty * RASTER_TILE + RASTER_TILE - 1, p.Y - 1);
            const double rx0 = raster_centre(p.x0, tx * RASTER_TILE, p.vx), rx1 = raster_centre(p.x0, ix1, p.vx);
            const double ry0 = raster_centre(p.y0, ty * RASTER_TILE, p.vy), ry1 = raster_centre(p.y0, iy1, p.vy);
            const double dx = fmax(fmax(rx0 - (double)b[0], (double)b[0] - rx1), 0.0), dy = fmax(fmax(ry0 - (double)b[1], (double)b[1] - ry1), 0.0);
            const double r2 = 0.25 * ((double)b[2] * (double)b[2] + (double)b[3] * (double)b[3]);
            live = !(dx * dx + dy * dy > r2 * RASTER_CULL_SLACK);
        }
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
        const double yaw = (double)b[4];
        s_geo[k][0] = (double)b[0];
        s_geo[k][1] = (double)b[1];
        s_geo[k][2] = cos(yaw);
        s_geo[k][3] = sin(yaw);
        s_geo[k][4] = (double)b[2] / 2.0;
        s_geo[k][5] = (double)b[3] / 2.0;
        s_rank[k] = rank;
        s_label[k] = (uint8_t)label;
        s_index[k] = tid;
    }
    __syncthreads();

    // a thread's cell against the survivors, in box order: a later box takes the cell only with a greater rank
    const double px = raster_centre(p.x0, ix, p.vx), py = raster_centre(p.y0, iy, p.vy);
    int best_rank = -1, best_index = -1, best_label = 0;
    for (int k = 0; k < n_live; ++k) {                    // workgroup-uniform, LDS broadcast reads
        const double ex = px - s_geo[k][0], ey = py - s_geo[k][1], c = s_geo[k][2], s = s_geo[k][3];
        const double lx = ex * c + ey * s, ly = -ex * s + ey * c;
        if (fabs(lx) <= s_geo[k][4] && fabs(ly) <= s_geo[k][5] && s_rank[k] > best_rank) {
            best_rank = s_rank[k];
            best_index = s_index[k];
            best_label = s_label[k];
        }
    }
    if (active) {
        const size_t cell = ((size_t)item * p.X + ix) * p.Y + iy;
        p.labels[cell] = (uint8_t)best_label;
        if (p.owner) p.owner[cell] = best_index;
        if (p.ws) atomicAdd(&s_hist[best_label == RASTER_IGNORE ? p.n_cls : best_label], 1);
    }
    if (p.ws) {
        __syncthreads();
        if (tid <= p.n_cls) p.ws[(size_t)blockIdx.x * (p.n_cls + 1) + tid] = s_hist[tid];
    }
}

__global__ __launch_bounds__(256) void raster_hist_kernel(const int32_t *__restrict__ ws, int tiles, int n_cls, long long *__restrict__ hist) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, item = blockIdx.x;
    const int bins = n_cls + 1;
    for (int bin = wave; bin < bins; bin += 4) {
        long long sum = 0;
        for (int t = lane; t < tiles; t += 64) sum += ws[((size_t)item * tiles + t) * bins + bin];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0) hist[(size_t)item * bins + bin] = sum;
    }
}

static long long raster_tiles(int X, int Y) { return (long long)((X + RASTER_TILE - 1) / RASTER_TILE) * ((Y + RASTER_TILE - 1) / RASTER_TILE); }
static bool raster_shape_ok(long long n, int X, int Y) { return n >= 0 && X >= 1 && Y >= 1 && (n == 0 || raster_tiles(X, Y) <= 0x7fffffffLL / n); }

extern "C" long long v2x_seg_rasterize_workspace_size(long long n, int X, int Y, int n_cls) {
    if (!raster_shape_ok(n, X, Y) || n_cls < 2 || n_cls > RASTER_MAX_CLS) return -1;
    return n * raster_tiles(X, Y) * (n_cls + 1) * (long long)sizeof(int32_t);
}

extern "C" int v2x_seg_rasterize(const float *boxes, const uint8_t *cls, const int32_t *count, long long n, int cap, float x0, float y0, float vx, float vy,
                                 int X, int Y, int n_cls, const uint8_t *rank, uint8_t *labels, int32_t *owner, long long *hist, void *workspace,
                                 long long workspace_bytes, v2x_stream_t stream) {
    if (n == 0) return V2X_OK;
    V2X_REQUIRE(n > 0, "v2x_seg_rasterize: negative n (%lld)", n);
    V2X_REQUIRE(cap >= 1 && cap <= RASTER_MAX_BOX, "v2x_seg_rasterize: cap=%d must lie in [1, %d]", cap, RASTER_MAX_BOX);
    V2X_REQUIRE(n_cls >= 2 && n_cls <= RASTER_MAX_CLS, "v2x_seg_rasterize: n_cls=%d must lie in [2, %d]", n_cls, RASTER_MAX_CLS);
    V2X_REQUIRE(vx > 0.0f && vy > 0.0f && vx <= 3.0e38f && vy <= 3.0e38f && x0 >= -3.0e38f && x0 <= 3.0e38f && y0 >= -3.0e38f && y0 <= 3.0e38f,
                "v2x_seg_rasterize: grid needs finite x0 (%g), y0 (%g) and finite cell sizes vx (%g), vy (%g) > 0", (double)x0, (double)y0, (double)vx,
                (double)vy);
    V2X_REQUIRE(raster_shape_ok(n, X, Y), "v2x_seg_rasterize: n=%lld, X=%d, Y=%d: sizes must be >= 1 and n*tiles < 2^31", n, X, Y);
    V2X_REQUIRE(boxes && cls && count && labels, "v2x_seg_rasterize: null pointer (only rank, owner, hist and, without hist, workspace may be null)");
    const int tiles_y = (Y + RASTER_TILE - 1) / RASTER_TILE, tiles = (int)raster_tiles(X, Y);
    if (hist) {
        const long long need = v2x_seg_rasterize_workspace_size(n, X, Y, n_cls);
        V2X_REQUIRE(workspace && workspace_bytes >= need, "v2x_seg_rasterize: workspace of %lld bytes, %lld needed for hist", workspace ? workspace_bytes : 0LL,
                    need);
        V2X_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0 && (reinterpret_cast<uintptr_t>(hist) & 7) == 0,
                    "v2x_seg_rasterize: workspace must be 4-byte and hist 8-byte aligned");
    }
    V2X_REQUIRE(!owner || (reinterpret_cast<uintptr_t>(owner) & 3) == 0, "v2x_seg_rasterize: owner must be 4-byte aligned");
    const raster_args p = {boxes, cls, count, rank, cap, X, Y, n_cls, tiles_y, tiles, x0, y0, vx, vy, labels, owner, hist ? static_cast<int32_t *>(workspace) : nullptr};
    const int rc = v2x_launch<raster_tile_kernel, 0>("raster_tile_kernel", dim3((unsigned)(n * tiles)), dim3(256), 0, (hipStream_t)stream, p);
    if (rc != V2X_OK || !hist) return rc;
    return v2x_launch<raster_hist_kernel, 0>("raster_hist_kernel", dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream,
                                             static_cast<const int32_t *>(workspace), tiles, n_cls, hist);
}

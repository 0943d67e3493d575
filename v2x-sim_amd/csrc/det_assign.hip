// f-3 -- detection training targets: anchors assigned to ground-truth boxes by rotated IoU with thresholds (upstream does this once, when the data is
// created, and stores gt_max_iou; the radius rule of utils/synthetic_scene.anchor_targets_sparse is the stand-in it replaces).  Build-owned spec:
// DESIGN.md section 3.7 ("IoU assignment").  Two launches for all items of a call, no atomics, no allocation, no host synchronisation; every output
// element is written.
//   assign_tile_kernel    one 256-thread workgroup per 16 x 16 tile of cells and item, a thread owns one cell with its A anchors.  The item's boxes
//                         are staged in LDS; a box whose centre lies further from the tile's anchor centres than the two circumradii reach is dead
//                         for the tile (IoU is exactly 0), the same test per cell precedes every rotated_iou_d (det_geom.h).  Per anchor: the box of
//                         largest IoU (lowest index on ties), the threshold step, the dense outputs.  Per live box: the tile's best (IoU, flat anchor
//                         index) -- a wave reduction per (anchor slot, box), lane 0 folds it into the wave's LDS row, the four rows are combined at
//                         the end -- into workspace slot [item][box][tile].  max with "lowest index on ties" is order-free: bit-reproducible.
//   assign_finish_kernel  one workgroup per item: a wave per box folds the tile slots, then one thread per box resolves the claims on the same anchor
//                         (largest IoU, lowest box on ties) and the winners patch their anchor's outputs.
#include "common.h"
#include "det_geom.h"

constexpr int ASSIGN_MAX_GT = 256;      // one staged box per thread
constexpr int ASSIGN_TILE = 16;
// The circumradius reject compares squared fp64 distances; the slack keeps it on the safe side of their rounding (a pair it lets through is decided by
// rotated_iou_d, which returns 0 for disjoint boxes anyway).
constexpr double ASSIGN_REJECT_SLACK = 1.0 + 1e-9;

struct assign_slot { double iou; int idx, pad; };   // a box's best anchor within one tile; idx = -1: none (iou = 0)

struct assign_args {
    const float *gt_boxes;      // [n][gt_cap][5]
    const int32_t *gt_count;    // [n]
    const float *anchors;       // [X][Y][A][6]
    int X, Y, A, gt_cap, tiles_y, tiles;
    float pos_thr, neg_thr;
    int force_match;
    float *labels, *reg;        // [n][X][Y][A][2], [n][X][Y][A][1][6]
    uint8_t *mask;              // [n][X][Y][A][1]
    int32_t *assoc;             // [n][X][Y][A] or null
    float *anchor_iou;          // [n][X][Y][A] or null
};

__device__ __forceinline__ bool assign_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ int assign_count(const assign_args &p, int item) {
    const int c = p.gt_count[item];
    return c < 0 ? 0 : (c > p.gt_cap ? p.gt_cap : c);
}
// Can the box overlap anything?  Finite fields, extents >= 0 (the spec's valid box) and an area: a valid box without one has IoU 0 with everything.
__device__ __forceinline__ bool assign_box_live(const float *b) {
    return assign_finite(b[0]) && assign_finite(b[1]) && assign_finite(b[2]) && assign_finite(b[3]) && assign_finite(b[4]) && b[2] >= 0.0f && b[3] >= 0.0f &&
           (double)b[2] * b[3] != 0.0;
}
// The anchor's box (x, y, w, h, yaw_a): yaw_a = the fp32 rounding of atan2(sin, cos) in fp64.
__device__ __forceinline__ void assign_anchor_box(const float *a, float (&box)[5]) {
    box[0] = a[0];
    box[1] = a[1];
    box[2] = a[2];
    box[3] = a[3];
    box[4] = (float)atan2((double)a[4], (double)a[5]);
}
__device__ __forceinline__ double assign_radius(float w, float h) { return 0.5 * sqrt((double)w * w + (double)h * h); }

// Anchor q (flat index within the item) becomes positive for box g: label (0, 1), mask 1, assoc g, the code of (q, g) -- the inverse of decode_boxes, in
// fp64 from the fp32 inputs, rounded once.
__device__ __forceinline__ void assign_write_positive(const assign_args &p, size_t row, const float (&ab)[5], const float *g, int gi) {
    const double kPi = 3.14159265358979323846;
    double d = fmod(((double)g[4] - (double)ab[4]) + 0.5 * kPi, kPi);
    if (d < 0.0) d += kPi;
    d -= 0.5 * kPi;                                       // folded to [-pi/2, pi/2)
    *reinterpret_cast<float2 *>(p.labels + row * 2) = make_float2(0.0f, 1.0f);
    float *r = p.reg + row * 6;
    r[0] = (float)((double)g[0] - (double)ab[0]);
    r[1] = (float)((double)g[1] - (double)ab[1]);
    r[2] = (float)log((double)g[2] / (double)ab[2]);
    r[3] = (float)log((double)g[3] / (double)ab[3]);
    r[4] = (float)sin(d);
    r[5] = (float)cos(d);
    p.mask[row] = 1;
    if (p.assoc) p.assoc[row] = gi;
}

// the better of two (IoU, index) candidates: larger IoU, lower index on ties; idx = -1 goes with iou = 0 and loses to everything
__device__ __forceinline__ void assign_better(double &iou, int &idx, double o_iou, int o_idx) {
    if (o_iou > iou || (o_iou == iou && o_idx >= 0 && (idx < 0 || o_idx < idx))) {
        iou = o_iou;
        idx = o_idx;
    }
}
__device__ __forceinline__ void assign_wave_best(double &iou, int &idx) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o_iou = __shfl_xor(iou, off);
        const int o_idx = __shfl_xor(idx, off);
        assign_better(iou, idx, o_iou, o_idx);
    }
}

__global__ __launch_bounds__(256) void assign_tile_kernel(assign_args p, assign_slot *__restrict__ ws) {
    __shared__ float s_box[ASSIGN_MAX_GT * 5];
    __shared__ double s_rad[ASSIGN_MAX_GT];
    __shared__ uint8_t s_live[ASSIGN_MAX_GT];
    __shared__ double s_wiou[4][ASSIGN_MAX_GT];
    __shared__ int s_widx[4][ASSIGN_MAX_GT];
    __shared__ double s_bound[4][5];          // per wave: min x, max x, min y, max y, max circumradius of its anchors

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int item = blockIdx.x / p.tiles, tile = blockIdx.x - item * p.tiles;
    const int tx = tile / p.tiles_y, ty = tile - tx * p.tiles_y;
    const int ix = tx * ASSIGN_TILE + (tid >> 4), iy = ty * ASSIGN_TILE + (tid & 15);     // iy, the fast dimension of the outputs, along the lanes
    const bool active = ix < p.X && iy < p.Y;
    const int A = p.A, count = assign_count(p, item);
    const size_t cell = active ? (size_t)ix * p.Y + iy : 0;

    // the tile's anchors: where their centres lie and how far they reach
    double bx0 = 1e300, bx1 = -1e300, by0 = 1e300, by1 = -1e300, br = 0.0;
    if (active) {
        for (int a = 0; a < A; ++a) {
            const float *an = p.anchors + (cell * A + a) * 6;
            bx0 = fmin(bx0, (double)an[0]);
            bx1 = fmax(bx1, (double)an[0]);
            by0 = fmin(by0, (double)an[1]);
            by1 = fmax(by1, (double)an[1]);
            br = fmax(br, assign_radius(an[2], an[3]));
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        bx0 = fmin(bx0, __shfl_xor(bx0, off));
        bx1 = fmax(bx1, __shfl_xor(bx1, off));
        by0 = fmin(by0, __shfl_xor(by0, off));
        by1 = fmax(by1, __shfl_xor(by1, off));
        br = fmax(br, __shfl_xor(br, off));
    }
    if (lane == 0) {
        s_bound[wave][0] = bx0;
        s_bound[wave][1] = bx1;
        s_bound[wave][2] = by0;
        s_bound[wave][3] = by1;
        s_bound[wave][4] = br;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        bx0 = fmin(bx0, s_bound[w][0]);
        bx1 = fmax(bx1, s_bound[w][1]);
        by0 = fmin(by0, s_bound[w][2]);
        by1 = fmax(by1, s_bound[w][3]);
        br = fmax(br, s_bound[w][4]);
    }
    // stage the item's boxes (thread g = box g; count <= gt_cap <= 256); dead for the tile: not live at all, or out of every anchor's reach
    if (tid < count) {
        const float *b = p.gt_boxes + ((size_t)item * p.gt_cap + tid) * 5;
        float v[5];
#pragma unroll
        for (int e = 0; e < 5; ++e) s_box[tid * 5 + e] = v[e] = b[e];
        bool live = assign_box_live(v);
        double rad = 0.0;
        if (live) {
            rad = assign_radius(v[2], v[3]);
            const double dx = fmax(fmax(bx0 - (double)v[0], (double)v[0] - bx1), 0.0), dy = fmax(fmax(by0 - (double)v[1], (double)v[1] - by1), 0.0);
            const double reach = rad + br;
            live = !(dx * dx + dy * dy > reach * reach * ASSIGN_REJECT_SLACK);
        }
        s_rad[tid] = rad;
        s_live[tid] = live ? 1 : 0;
    }
    for (int g = lane; g < count; g += 64) {
        s_wiou[wave][g] = 0.0;
        s_widx[wave][g] = -1;
    }
    __syncthreads();

    const size_t row0 = ((size_t)item * p.X * p.Y + cell) * A;
    for (int a = 0; a < A; ++a) {
        float ab[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        double ra = 0.0;
        if (active) {
            assign_anchor_box(p.anchors + (cell * A + a) * 6, ab);
            ra = assign_radius(ab[2], ab[3]);
        }
        const int flat = active ? (int)(cell * A + a) : -1;
        double best = 0.0;
        int best_g = -1;
        for (int g = 0; g < count; ++g) {
            if (!s_live[g]) continue;                      // workgroup-uniform
            double iou = 0.0;
            if (active) {
                const double dx = (double)ab[0] - (double)s_box[g * 5], dy = (double)ab[1] - (double)s_box[g * 5 + 1], reach = ra + s_rad[g];
                // the BOX is the polygon that is clipped, by the anchor's edges: a box that lies inside the anchor comes back vertex for vertex, so every
                // anchor of one size that contains it gets the same IoU bits (a small box ties over many anchors; the lowest index must win, not a rounding)
                if (!(dx * dx + dy * dy > reach * reach * ASSIGN_REJECT_SLACK)) iou = rotated_iou_d(s_box + g * 5, ab);
            }
            if (iou > best) {                              // ascending g: the lowest index wins a tie
                best = iou;
                best_g = g;
            }
            if (__ballot(iou > 0.0) != 0ull) {             // wave-uniform
                double w_iou = iou;
                int w_idx = iou > 0.0 ? flat : -1;
                assign_wave_best(w_iou, w_idx);
                if (lane == 0) {
                    double c_iou = s_wiou[wave][g];
                    int c_idx = s_widx[wave][g];
                    assign_better(c_iou, c_idx, w_iou, w_idx);
                    s_wiou[wave][g] = c_iou;
                    s_widx[wave][g] = c_idx;
                }
            }
        }
        if (active) {
            const size_t row = row0 + a;
            if (p.anchor_iou) p.anchor_iou[row] = (float)best;
            if (best_g >= 0 && best >= (double)p.pos_thr) {
                assign_write_positive(p, row, ab, s_box + best_g * 5, best_g);
            } else {
                // background below neg_thr, otherwise ignored: (0, 0) contributes to neither loss term
                *reinterpret_cast<float2 *>(p.labels + row * 2) = make_float2(best < (double)p.neg_thr ? 1.0f : 0.0f, 0.0f);
                float *r = p.reg + row * 6;
#pragma unroll
                for (int e = 0; e < 6; ++e) r[e] = 0.0f;
                p.mask[row] = 0;
                if (p.assoc) p.assoc[row] = -1;
            }
        }
    }
    __syncthreads();
    // the tile's slot of every box of the item, dead ones included (the finish kernel reads count * tiles slots without a validity map)
    for (int g = tid; g < count; g += 256) {
        double iou = 0.0;
        int idx = -1;
#pragma unroll
        for (int w = 0; w < 4; ++w) assign_better(iou, idx, s_wiou[w][g], s_widx[w][g]);
        ws[((size_t)item * p.gt_cap + g) * p.tiles + tile] = {iou, idx, 0};
    }
}

__global__ __launch_bounds__(256) void assign_finish_kernel(assign_args p, const assign_slot *__restrict__ ws, float *__restrict__ gt_max_iou,
                                                             int32_t *__restrict__ gt_best) {
    __shared__ double s_iou[ASSIGN_MAX_GT];
    __shared__ int s_idx[ASSIGN_MAX_GT];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, item = blockIdx.x;
    const int count = assign_count(p, item);
    for (int g = wave; g < count; g += 4) {
        const assign_slot *s = ws + ((size_t)item * p.gt_cap + g) * p.tiles;
        double iou = 0.0;
        int idx = -1;
        for (int t = lane; t < p.tiles; t += 64) assign_better(iou, idx, s[t].iou, s[t].idx);
        assign_wave_best(iou, idx);
        if (lane == 0) {
            s_iou[g] = iou;
            s_idx[g] = idx;
        }
    }
    __syncthreads();
    for (int g = tid; g < p.gt_cap; g += 256) {
        const bool has = g < count && s_idx[g] >= 0;       // gmax > 0
        gt_max_iou[(size_t)item * p.gt_cap + g] = has ? (float)s_iou[g] : 0.0f;
        gt_best[(size_t)item * p.gt_cap + g] = has ? s_idx[g] : -1;
        if (!has || !p.force_match) continue;
        // several boxes on one anchor: the largest IoU keeps it, the lowest box on ties
        const int q = s_idx[g];
        bool wins = true;
        for (int o = 0; o < count; ++o)
            if (o != g && s_idx[o] == q && (s_iou[o] > s_iou[g] || (s_iou[o] == s_iou[g] && o < g))) wins = false;
        if (!wins) continue;
        float ab[5];
        assign_anchor_box(p.anchors + (size_t)q * 6, ab);
        assign_write_positive(p, (size_t)item * p.X * p.Y * p.A + q, ab, p.gt_boxes + ((size_t)item * p.gt_cap + g) * 5, g);
    }
}

static bool assign_shape_ok(long long n_items, int X, int Y, int A, int gt_cap) {
    if (n_items < 0 || X < 1 || Y < 1 || A < 1 || gt_cap < 1 || gt_cap > ASSIGN_MAX_GT) return false;
    if ((long long)X * Y > 0x7fffffffLL / A) return false;                                          // the flat anchor index is an int
    const long long tiles = (long long)((X + ASSIGN_TILE - 1) / ASSIGN_TILE) * ((Y + ASSIGN_TILE - 1) / ASSIGN_TILE);
    return n_items == 0 || tiles <= 0x7fffffffLL / n_items;                                         // one workgroup per (item, tile)
}

extern "C" long long v2x_det_assign_workspace_size(long long n_items, int X, int Y, int A, int gt_cap) {
    if (!assign_shape_ok(n_items, X, Y, A, gt_cap)) return -1;
    const long long tiles = (long long)((X + ASSIGN_TILE - 1) / ASSIGN_TILE) * ((Y + ASSIGN_TILE - 1) / ASSIGN_TILE);
    return n_items * gt_cap * tiles * (long long)sizeof(assign_slot);
}

extern "C" int v2x_det_assign_targets(const float *gt_boxes, const int32_t *gt_count, long long n_items, int gt_cap, const float *anchors, int X, int Y,
                                      int A, float pos_thr, float neg_thr, int force_match, float *labels, float *reg_targets, uint8_t *reg_loss_mask,
                                      int32_t *assoc, float *anchor_iou, float *gt_max_iou, int32_t *gt_best, void *workspace, long long workspace_bytes,
                                      v2x_stream_t stream) {
    V2X_REQUIRE(n_items >= 0, "v2x_det_assign_targets: negative n_items (%lld)", n_items);
    if (n_items == 0) return V2X_OK;
    V2X_REQUIRE(gt_cap >= 1 && gt_cap <= ASSIGN_MAX_GT, "v2x_det_assign_targets: gt_cap=%d must lie in [1, %d]", gt_cap, ASSIGN_MAX_GT);
    V2X_REQUIRE(neg_thr > 0.0f && neg_thr <= pos_thr && pos_thr <= 1.0f, "v2x_det_assign_targets: thresholds need 0 < neg_thr (%g) <= pos_thr (%g) <= 1",
                (double)neg_thr, (double)pos_thr);
    V2X_REQUIRE(assign_shape_ok(n_items, X, Y, A, gt_cap), "v2x_det_assign_targets: n_items=%lld, X=%d, Y=%d, A=%d: sizes must be >= 1, X*Y*A and n_items*tiles < 2^31",
                n_items, X, Y, A);
    V2X_REQUIRE(gt_boxes && gt_count && anchors && labels && reg_targets && reg_loss_mask && gt_max_iou && gt_best && workspace,
                "v2x_det_assign_targets: null pointer (only assoc and anchor_iou may be null)");
    V2X_REQUIRE(workspace_bytes >= v2x_det_assign_workspace_size(n_items, X, Y, A, gt_cap), "v2x_det_assign_targets: workspace of %lld bytes, %lld needed",
                workspace_bytes, v2x_det_assign_workspace_size(n_items, X, Y, A, gt_cap));
    V2X_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(labels) & 7) == 0,
                "v2x_det_assign_targets: workspace and labels must be 8-byte aligned");
    const int tiles_y = (Y + ASSIGN_TILE - 1) / ASSIGN_TILE, tiles = ((X + ASSIGN_TILE - 1) / ASSIGN_TILE) * tiles_y;
    const assign_args p = {gt_boxes, gt_count, anchors, X, Y, A, gt_cap, tiles_y, tiles, pos_thr, neg_thr, force_match != 0,
                           labels, reg_targets, reg_loss_mask, assoc, anchor_iou};
    assign_slot *ws = static_cast<assign_slot *>(workspace);
    const int rc = v2x_launch<assign_tile_kernel, 0>("assign_tile_kernel", dim3((unsigned)(n_items * tiles)), dim3(256), 0, (hipStream_t)stream, p, ws);
    if (rc != V2X_OK) return rc;
    return v2x_launch<assign_finish_kernel, 0>("assign_finish_kernel", dim3((unsigned)n_items), dim3(256), 0, (hipStream_t)stream, p,
                                               static_cast<const assign_slot *>(ws), gt_max_iou, gt_best);
}

// Box geometry of row f-1, shared by postprocess.hip (det_nms_kernel, rotated_iou_kernel, match_detections_kernel) and late_fuse.hip
// (late_fuse_kernel): the rotated-box IoU in fp64, the stand-up box of a decoded box and the overlap test of greedy suppression.  ONE definition:
// a box suppressed by the per-agent NMS and by the cross-agent NMS is suppressed by the same arithmetic.
#pragma once
#include "common.h"

constexpr int DET_MAX_CAP = 4096;
// Two launches per batch: the bit-matrix form handles the maps with at most NMS_FAST_CAP candidates, the others are marked NMS_PENDING in
// their out_count and taken by the second launch (the serial scan), which returns at once for every other map.
constexpr int NMS_PENDING = (int)0x80000000;
constexpr int NMS_FAST_CAP = 512;

// ---- rotated-box IoU (row f-1: upstream's eval_map intersects shapely polygons; here: convex clipping in fp64) ----------
// Corners of (x, y, w, h, yaw), counter-clockwise, first = (+w/2, +h/2) rotated (the order of utils/postprocess.box_corners).
__device__ __forceinline__ void box_corners_d(const float *b, double (&cx)[4], double (&cy)[4]) {
    const double x = b[0], y = b[1], w = b[2], h = b[3], yaw = b[4];
    const double c = cos(yaw), s = sin(yaw);
    const double dx[4] = {0.5 * w, -0.5 * w, -0.5 * w, 0.5 * w}, dy[4] = {0.5 * h, 0.5 * h, -0.5 * h, -0.5 * h};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        cx[q] = x + dx[q] * c - dy[q] * s;
        cy[q] = y + dx[q] * s + dy[q] * c;
    }
}

// Area of (quad 1) intersected with (quad 2): Sutherland-Hodgman, quad 1 clipped by the four edges of quad 2.  A convex
// polygon gains at most one vertex per clip: 4 + 4 = 8.
static __device__ double quad_intersection_area(const double (&ax)[4], const double (&ay)[4], const double (&bx)[4], const double (&by)[4]) {
    double px[10], py[10], qx[10], qy[10];
    int n = 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        px[i] = ax[i];
        py[i] = ay[i];
    }
    for (int e = 0; e < 4 && n > 0; ++e) {
        const double ex0 = bx[e], ey0 = by[e], ex1 = bx[(e + 1) & 3], ey1 = by[(e + 1) & 3];
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const int j = (i + 1 == n) ? 0 : i + 1;
            const double sp = (ex1 - ex0) * (py[i] - ey0) - (ey1 - ey0) * (px[i] - ex0);
            const double sq = (ex1 - ex0) * (py[j] - ey0) - (ey1 - ey0) * (px[j] - ex0);
            if (sp >= 0.0) {
                qx[m] = px[i];
                qy[m] = py[i];
                ++m;
            }
            if ((sp >= 0.0) != (sq >= 0.0)) {
                const double t = sp / (sp - sq);
                qx[m] = px[i] + t * (px[j] - px[i]);
                qy[m] = py[i] + t * (py[j] - py[i]);
                ++m;
            }
        }
        n = m;
        for (int i = 0; i < n; ++i) {
            px[i] = qx[i];
            py[i] = qy[i];
        }
    }
    if (n < 3) return 0.0;
    double a2 = 0.0;
    for (int i = 0; i < n; ++i) {
        const int j = (i + 1 == n) ? 0 : i + 1;
        a2 += px[i] * py[j] - px[j] * py[i];
    }
    return 0.5 * fabs(a2);
}

static __device__ double rotated_iou_d(const float *a, const float *b) {
    // A rectangle without area shares none with anything.  Not only a shortcut: all four edges of a POINT rectangle (w = h = 0) have
    // zero length, every sp below is 0 and "inside", so clipping against it returned the whole of `a` -- inter = area(a) up to its
    // rounding, uni = a rounding error, IoU = 0 or ~1e16 as the rounding fell.
    if ((double)a[2] * a[3] == 0.0 || (double)b[2] * b[3] == 0.0) return 0.0;
    double ax[4], ay[4], bx[4], by[4];
    box_corners_d(a, ax, ay);
    box_corners_d(b, bx, by);
    // stand-up boxes first: disjoint -> 0 without clipping
    double a0 = ax[0], a1 = ax[0], a2 = ay[0], a3 = ay[0], b0 = bx[0], b1 = bx[0], b2 = by[0], b3 = by[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) {
        a0 = fmin(a0, ax[q]); a1 = fmax(a1, ax[q]); a2 = fmin(a2, ay[q]); a3 = fmax(a3, ay[q]);
        b0 = fmin(b0, bx[q]); b1 = fmax(b1, bx[q]); b2 = fmin(b2, by[q]); b3 = fmax(b3, by[q]);
    }
    if (a1 < b0 || b1 < a0 || a3 < b2 || b3 < a2) return 0.0;
    const double inter = quad_intersection_area(ax, ay, bx, by);
    const double uni = (double)a[2] * a[3] + (double)b[2] * b[3] - inter;   // |w*h| of each rectangle
    return uni > 0.0 ? inter / uni : 0.0;
}

// ---- greedy suppression -----------------------------------------------------------------------------------------------
// Stand-up box (x1, y1, x2, y2) of a decoded box: the corners (+-w/2, +-h/2) rotated; x extents = |w/2*c| + |h/2*s| in exact arithmetic; numpy
// takes min/max of the four corners -- do the same so that the roundings agree
__device__ __forceinline__ float4 det_standup_box(float x, float y, float w, float h, float yaw) {
    const float c = cosf(yaw), s = sinf(yaw);
    const float dx[4] = {w / 2, -w / 2, -w / 2, w / 2}, dy[4] = {h / 2, h / 2, -h / 2, -h / 2};
    float x1 = 3.0e38f, y1 = 3.0e38f, x2 = -3.0e38f, y2 = -3.0e38f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        // separately rounded products and sums, in numpy's order (the intent: the builtins do not bind the backend's contraction -- HISTORY.md, late_fuse.hip;
        // the suppression tests decide with a margin on the IoU, and the arithmetic stays as it has always been compiled)
        const float cx = __fsub_rn(__fadd_rn(x, __fmul_rn(dx[q], c)), __fmul_rn(dy[q], s));
        const float cy = __fadd_rn(__fadd_rn(y, __fmul_rn(dx[q], s)), __fmul_rn(dy[q], c));
        x1 = fminf(x1, cx);
        x2 = fmaxf(x2, cx);
        y1 = fminf(y1, cy);
        y2 = fmaxf(y2, cy);
    }
    return make_float4(x1, y1, x2, y2);
}

// Does the KEPT box k suppress candidate i?  bk, bi: their stand-up boxes; box_k, box_i: the boxes themselves (x, y, w, h, yaw), read only in
// rotated mode, where the stand-up overlap is only the cheap reject and the decision is the polygon IoU.
template <bool ROTATED>
__device__ __forceinline__ bool det_suppresses(const float4 &bk, const float4 &bi, const float *box_k, const float *box_i, float nms_thr) {
    const float iw = fmaxf(0.0f, fminf(bk.z, bi.z) - fmaxf(bk.x, bi.x));
    const float ih = fmaxf(0.0f, fminf(bk.w, bi.w) - fmaxf(bk.y, bi.y));
    const float inter = iw * ih;
    if constexpr (ROTATED) {
        return inter > 0.0f && (float)rotated_iou_d(box_k, box_i) > nms_thr;
    } else {
        const float area_k = (bk.z - bk.x) * (bk.w - bk.y);
        const float area_i = (bi.z - bi.x) * (bi.w - bi.y);
        return inter / (area_k + area_i - inter + 1e-12f) > nms_thr;
    }
}

// The per-detection step of eval_map's matching (mmdet tpfp_default), shared by postprocess.hip (match_detections_kernel: one threshold) and
// det_map.hip (det_map_match_kernel: up to eight thresholds from ONE search): which ground truth does a detection take?  The one of highest
// rotated IoU (fp64 clip, det_geom.h), the lowest index on ties; an IoU of 0 (or NaN) takes none.  The choice does not depend on the threshold.
// ONE definition: the sweep of tests/test_gpu_post_sweep.py over the strided scan and the tree reduction guards both kernels.
#pragma once
#include "det_geom.h"

constexpr int DET_MATCH_THREADS = 256;
constexpr int DET_MATCH_MAX_GT = 8192;

// Called by ALL DET_MATCH_THREADS threads of the workgroup.  d: the detection (x, y, w, h, yaw); gt_row: the image's ground truths [ng][5];
// s_best / s_arg: LDS, DET_MATCH_THREADS entries each.  On return (after the tree's last barrier) s_best[0] = the best IoU (0.0 without a
// match) and s_arg[0] = its ground truth's index (-1 without one).  The caller synchronises before the next call overwrites them.
__device__ __forceinline__ void det_best_gt(const float *d, const float *gt_row, int ng, int tid, double *s_best, int *s_arg) {
    double best = 0.0;
    int arg = -1;
    for (int g = tid; g < ng; g += DET_MATCH_THREADS) {
        const double v = rotated_iou_d(d, gt_row + (size_t)g * 5);
        if (v > best) {
            best = v;
            arg = g;
        }
    }
    s_best[tid] = best;
    s_arg[tid] = arg;
    __syncthreads();
    for (int st = DET_MATCH_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) {
            const double o = s_best[tid + st];
            const int oa = s_arg[tid + st];
            // larger IoU wins; equal IoU: the lower ground-truth index (a sequential scan keeps the first maximum)
            if (o > s_best[tid] || (o == s_best[tid] && oa >= 0 && (s_arg[tid] < 0 || oa < s_arg[tid]))) {
                s_best[tid] = o;
                s_arg[tid] = oa;
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int det_clamp_count(int n, int cap) { return n < 0 ? 0 : (n > cap ? cap : n); }

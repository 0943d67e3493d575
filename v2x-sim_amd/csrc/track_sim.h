// The frame reading the tracking metrics of row f-5 share: hota.hip (the HOTA family) and mot_seq.hip (CLEAR MOT and the Identity family) compact a
// frame's valid boxes, compute the fp64 IoU and read non-finite values in ONE way.  Moved here verbatim from hota.hip; the rules are stated at the head of
// that file and in include/v2x_amd.h.
#pragma once
#include "track_assign.h"
#include <float.h>

__device__ __forceinline__ double hota_finite0(double v) { return fabs(v) <= DBL_MAX ? v : 0.0; }   // NaN and +-inf read as 0

// ClearMot._iou64 on one pair: fp64 on the fp32 coordinates, operation by operation (no contraction: the host statement rounds every product)
__device__ __forceinline__ double hota_iou(const float4 a, const float4 b) {
#pragma clang fp contract(off)
    const double w = fmax(0.0, fmin((double)a.z, (double)b.z) - fmax((double)a.x, (double)b.x));
    const double h = fmax(0.0, fmin((double)a.w, (double)b.w) - fmax((double)a.y, (double)b.y));
    const double wh = w * h;
    const double aa = ((double)a.z - (double)a.x) * ((double)a.w - (double)a.y);
    const double ab = ((double)b.z - (double)b.x) * ((double)b.w - (double)b.y);
    return hota_finite0(wh / (aa + ab - wh));
}

__device__ __forceinline__ double hota_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ long long hota_wave_sum(long long v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the slot of id g among the frame's ng compacted ground-truth ids (lowest slot if the caller repeated it), or -1; wave-uniform
__device__ __forceinline__ int hota_slot_of(const int32_t *ids, int ng, int g, int lane) {
    const int id = lane < ng ? ids[lane] : -1;
    const unsigned long long b = __ballot(id == g);
    return b ? __ffsll(b) - 1 : -1;
}

// compaction of one side of a frame: -> the number of valid boxes; boxes to LDS, ids to the workspace, both in slot order
__device__ __forceinline__ int hota_compact(const float *boxes, const int32_t *ids, int count, int cap, int n_ids, float4 *box_lds, int32_t *ids_out, int lane) {
    const int n = min(max(count, 0), cap);
    const int id = lane < n ? ids[lane] : -1;
    const bool ok = id >= 0 && id < n_ids;
    const unsigned long long b = __ballot(ok);
    if (ok) {
        const int pos = __popcll(b & trk_lt_mask(lane));
        box_lds[pos] = *reinterpret_cast<const float4 *>(boxes + (size_t)lane * 4);
        ids_out[pos] = id;
    }
    return __popcll(b);
}

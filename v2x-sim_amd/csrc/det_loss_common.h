// What the two detection-loss kernel files share (det_loss.hip: focal + smooth-L1; det_corner_loss.hip: focal + corner distance): the argument block,
// the focal-loss terms of one anchor, the fixed-order workgroup sum, the forward grid and the fp64 finish launch.  One definition, so that the
// classification term, the partial layout ([n_blocks][3]: sum l_1, cls sum, loc sum) and the workspace size are the same for both localisation forms.
#pragma once
#include "common.h"

constexpr int DL_THREADS = 256;
constexpr int DL_MAX_BLOCKS = 1024;

struct DetLossArgs {
    const float *cls, *lab, *loc, *tgt;   // [n][2], [n][2], [n][6], [n][6]
    const uint8_t *mask;                  // [n] (bool)
    long long n;                          // anchors
    float alpha, beta;
    float *part;                          // [n_blocks][3]: sum l_1, cls sum, loc sum
    float *out;                           // [4]: loss, cls_loss, loc_loss, n (clamped)
    const float *g_loss, *g_cls, *g_loc;  // incoming gradients (device scalars; null = 0)
    float *dcls, *dloc;
    int n_blocks;
    // the corner form only (det_corner_loss.hip)
    const float *anchors;                 // [m][6]: x, y, w, h, sin, cos
    long long m;                          // anchors per map: anchor i decodes through row i mod m
    int wh_swap;                          // != 0: h runs along the heading (Config.box_wh_axis = "h_along_heading")
};

struct FocalTerms {
    float p0, p1, pt, s, alpha_t;
};

__device__ __forceinline__ FocalTerms focal_terms(float c0, float c1, float l0, float l1, float alpha) {
    FocalTerms f;
    const float m = fmaxf(c0, c1);
    const float e0 = __expf(c0 - m), e1 = __expf(c1 - m);
    const float lse = m + __logf(e0 + e1);
    const float lp0 = c0 - lse, lp1 = c1 - lse;
    const float inv = 1.0f / (e0 + e1);
    f.p0 = e0 * inv;
    f.p1 = e1 * inv;
    f.pt = f.p0 * l0 + f.p1 * l1;
    f.s = lp0 * l0 + lp1 * l1;
    f.alpha_t = l1 * alpha + l0 * (1.0f - alpha);
    return f;
}

// fixed-order sum of one value per thread over the workgroup (wave butterfly, then the four waves in wave order)
__device__ __forceinline__ float block_sum(float v, float *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup: thread t adds partials t, t + 256, ... in fp64, then a fixed tree
static __global__ __launch_bounds__(DL_THREADS) void det_loss_finish_kernel(const DetLossArgs a) {
    __shared__ double r[3][DL_THREADS];
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < a.n_blocks; b += DL_THREADS)
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += (double)a.part[b * 3 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int w = DL_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
#pragma unroll
            for (int k = 0; k < 3; ++k) r[k][threadIdx.x] += r[k][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float n = fmaxf((float)r[0][0], 1.0f);
        const float cl = (float)r[1][0] / n, ll = (float)r[2][0] / n;
        a.out[0] = cl + ll;
        a.out[1] = cl;
        a.out[2] = ll;
        a.out[3] = n;
    }
}

static inline int dl_blocks(long long n) {
    long long b = (n + DL_THREADS * 8 - 1) / (DL_THREADS * 8);      // >= 8 anchors per thread
    if (b < 1) b = 1;
    return (int)(b < DL_MAX_BLOCKS ? b : DL_MAX_BLOCKS);
}

static inline unsigned dl_bwd_blocks(long long n) {
    long long b = (n + DL_THREADS * 4 - 1) / (DL_THREADS * 4);
    return (unsigned)(b > 4096 ? 4096 : b);
}

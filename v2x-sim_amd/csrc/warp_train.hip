// Affine bilinear resampling of fp32 NCHW maps and its EXACT transpose -- the cross-agent warp of the training graph (row f-3).
// Upstream: coperception/models/det/base/IntermediateModelBase.py::feature_transformation = F.affine_grid + F.grid_sample
// (bilinear, zeros padding, align_corners=False), applied twice (rotation about the map centre, then translation); code absent from
// /root/reference, see include/v2x_amd.h.  In the PyTorch graph the BACKWARD of grid_sample is a scatter with fp32 atomics
// (grid_sampler_2d_backward_kernel: 0.9 ms per call on 40 x 256 x 32 x 32 maps = 17 % of a V2VNet training step, and not
// bit-reproducible).  Here the data gradient is a GATHER: for an affine map the output pixels q whose sample point falls within one pixel
// of an input pixel p lie in a small parallelogram around M^-1 (p - t) (<= 3 x 3 for a rotation, 2 x 2 for a translation); every thread
// owns one input pixel, walks those candidates in a fixed order, recomputes each candidate's sample position with the SAME device function
// as the forward kernel and adds w(q, p) * dout[q] -- the exact transpose of the forward operator, deterministic, no atomics.  The geometry
// (taps, candidate box, recomputed weight) is train_math.h's, shared with v2v_train.hip's two-pass message kernels.
// A singular or strongly shrinking map (|det M| small: many output pixels per input pixel) widens the candidate box up to the whole map --
// still exact, only slower.
#include "train_math.h"

namespace {
constexpr int WT_CCH = 16;   // channels per thread (the taps / candidates of a pixel are computed once per chunk)

struct WarpTrainArgs {
    const float *src;    // forward: input maps; backward: output gradient   [P][C][H][W]
    const float *theta;  // [P][2][3]
    float *dst;          // forward: output maps; backward: input gradient   [P][C][H][W]
    int P, C, H, W;
};

__global__ __launch_bounds__(256) void warp_affine_fwd_kernel(const WarpTrainArgs a) {
    const int p = blockIdx.z, c0 = blockIdx.y * WT_CCH;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int HW = a.H * a.W;
    if (pix >= HW) return;
    float th[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) th[k] = a.theta[p * 6 + k];
    const int i = pix / a.W, j = pix - i * a.W;
    const TmWarpTaps t = tm_warp_taps(th, j, i, a.H, a.W);
    const int nc = min(WT_CCH, a.C - c0);
    for (int c = 0; c < nc; ++c) {
        const float *s = a.src + ((size_t)p * a.C + c0 + c) * HW;
        // the same order of additions as at::native's grid_sampler_2d kernel: nw, ne, sw, se
        float v = s[t.o[0]] * t.w[0];
        v += s[t.o[1]] * t.w[1];
        v += s[t.o[2]] * t.w[2];
        v += s[t.o[3]] * t.w[3];
        a.dst[((size_t)p * a.C + c0 + c) * HW + pix] = v;
    }
}

__global__ __launch_bounds__(256) void warp_affine_bwd_kernel(const WarpTrainArgs a) {
    const int p = blockIdx.z, c0 = blockIdx.y * WT_CCH;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    const int HW = a.H * a.W;
    if (pix >= HW) return;
    float th[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) th[k] = a.theta[p * 6 + k];
    const int y = pix / a.W, x = pix - y * a.W;
    const TmWarpBox b = tm_warp_candidates(th, x, y, a.H, a.W);
    const int nc = min(WT_CCH, a.C - c0);
    float acc[WT_CCH];
#pragma unroll
    for (int c = 0; c < WT_CCH; ++c) acc[c] = 0.f;
    const float *s = a.src + ((size_t)p * a.C + c0) * HW;
    for (int i = b.ilo; i <= b.ihi; ++i)
        for (int j = b.jlo; j <= b.jhi; ++j) {
            const float w = tm_warp_weight(th, j, i, x, y, a.H, a.W);
            if (w == 0.f) continue;
            const int q = i * a.W + j;
#pragma unroll
            for (int c = 0; c < WT_CCH; ++c)
                if (c < nc) acc[c] += w * s[(size_t)c * HW + q];
        }
    for (int c = 0; c < nc; ++c) a.dst[((size_t)p * a.C + c0 + c) * HW + pix] = acc[c];
}

int warp_train_launch(bool bwd, const float *src, const float *theta, float *dst, int P, int C, int H, int W, hipStream_t s, const char *who) {
    V2X_REQUIRE(src && theta && dst, "%s: null pointer", who);
    V2X_REQUIRE(P >= 0 && C > 0 && H > 0 && W > 0 && (long long)H * W <= (1 << 24) && (long long)P * C * H * W < (1ll << 40), "%s: bad extent", who);
    if (P == 0) return V2X_OK;
    V2X_REQUIRE(P <= 65535 && (C + WT_CCH - 1) / WT_CCH <= 65535, "%s: more than 65535 maps or channel chunks per launch", who);
    WarpTrainArgs a{src, theta, dst, P, C, H, W};
    const dim3 grid((H * W + 255) / 256, (C + WT_CCH - 1) / WT_CCH, P);
    if (bwd) hipLaunchKernelGGL(warp_affine_bwd_kernel, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(warp_affine_fwd_kernel, grid, dim3(256), 0, s, a);
    V2X_CHECK_LAUNCH(who);
    return V2X_OK;
}
}  // namespace

extern "C" int v2x_warp_affine_f32(const float *in, const float *theta, int P, int C, int H, int W, float *out, v2x_stream_t stream) {
    return warp_train_launch(false, in, theta, out, P, C, H, W, (hipStream_t)stream, "v2x_warp_affine_f32");
}

extern "C" int v2x_warp_affine_bwd_f32(const float *dout, const float *theta, int P, int C, int H, int W, float *din, v2x_stream_t stream) {
    return warp_train_launch(true, dout, theta, din, P, C, H, W, (hipStream_t)stream, "v2x_warp_affine_bwd_f32");
}

// Arithmetic shared by the TRAINING kernels (warp_train, v2v_train, gru_train, bn_train, upcat_train): ONE definition of everything two of them must agree on
// bit for bit.  Device helpers (and one host predicate) only; no inference file includes this, so the inference objects do not depend on it.
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------------- eight bf16 (16 bytes) <-> fp32
__device__ __forceinline__ void tm_unpack8(const uint4 v, float f[8]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = __uint_as_float(w[i] << 16);
        f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
}
__device__ __forceinline__ uint4 tm_pack8(const float f[8]) {
    return make_uint4(pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7]));
}
// s += v
__device__ __forceinline__ void tm_acc8(float s[8], const uint4 v) {
    float f[8];
    tm_unpack8(v, f);
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] += f[i];
}

// ---------------------------------------------------------------------------------------------- affine bilinear resampling
// F.affine_grid + F.grid_sample (bilinear, zeros padding, align_corners = False) under theta [2][3].  The forward kernels (warp_affine_fwd_kernel on fp32 NCHW,
// v2v_message_kernel on bf16 NHWC) take their taps from tm_warp_taps; the backward kernels are gathers over tm_warp_candidates with the weight recomputed by
// tm_warp_weight from the SAME sample position -- which is what makes them the exact transposes of the forward operators.

// sample position, in input pixel units, of output pixel (j = column, i = row): affine_grid + grid_sample's unnormalisation
__device__ __forceinline__ void tm_warp_sample_pos(const float th[6], int j, int i, int H, int W, float &ix, float &iy) {
    const float xn = (2.0f * (float)j + 1.0f) / (float)W - 1.0f;
    const float yn = (2.0f * (float)i + 1.0f) / (float)H - 1.0f;
    const float gx = th[0] * xn + th[1] * yn + th[2];
    const float gy = th[3] * xn + th[4] * yn + th[5];
    ix = ((gx + 1.0f) * (float)W - 1.0f) * 0.5f;
    iy = ((gy + 1.0f) * (float)H - 1.0f) * 0.5f;
}

struct TmWarpTaps {
    float w[4];   // nw, ne, sw, se (at::native grid_sampler_2d's order of additions); 0 for a tap outside the map
    int o[4];     // pixel index of the tap (0 where the weight is 0)
};

__device__ __forceinline__ TmWarpTaps tm_warp_taps(const float th[6], int j, int i, int H, int W) {
    float ix, iy;
    tm_warp_sample_pos(th, j, i, H, W, ix, iy);
    const float fx = floorf(ix), fy = floorf(iy);
    // out-of-range sample positions (also inf / nan) contribute nothing: compare in float before converting
    const bool any = fx >= -1.0f && fx < (float)W && fy >= -1.0f && fy < (float)H;
    const int x0 = any ? (int)fx : 0, y0 = any ? (int)fy : 0;
    const float wx1 = ix - fx, wy1 = iy - fy, wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;
    const bool vx0 = any && x0 >= 0, vx1 = any && x0 + 1 < W, vy0 = any && y0 >= 0, vy1 = any && y0 + 1 < H;
    TmWarpTaps t;
    t.w[0] = (vx0 && vy0) ? wx0 * wy0 : 0.f;
    t.w[1] = (vx1 && vy0) ? wx1 * wy0 : 0.f;
    t.w[2] = (vx0 && vy1) ? wx0 * wy1 : 0.f;
    t.w[3] = (vx1 && vy1) ? wx1 * wy1 : 0.f;
    t.o[0] = (vx0 && vy0) ? y0 * W + x0 : 0;
    t.o[1] = (vx1 && vy0) ? y0 * W + x0 + 1 : 0;
    t.o[2] = (vx0 && vy1) ? (y0 + 1) * W + x0 : 0;
    t.o[3] = (vx1 && vy1) ? (y0 + 1) * W + x0 + 1 : 0;
    return t;
}

struct TmWarpBox {
    int jlo, jhi, ilo, ihi;
};

// The output pixels whose sample point can fall within one pixel of input pixel (x, y).  The sample position is an affine function of the output pixel,
// (ix, iy) = M (j, i) + t, so they lie in a parallelogram around M^-1 (p - t) (<= 3 x 3 for a rotation, 2 x 2 for a translation); a singular or non-finite theta
// gives the whole map -- still exact, only slower.
__device__ __forceinline__ TmWarpBox tm_warp_candidates(const float th[6], int x, int y, int H, int W) {
    const float fw = (float)W, fh = (float)H;
    const float m00 = th[0], m01 = th[1] * fw / fh, m10 = th[3] * fh / fw, m11 = th[4];
    float t0, t1;
    tm_warp_sample_pos(th, 0, 0, H, W, t0, t1);
    const float det = m00 * m11 - m01 * m10;
    TmWarpBox b = {0, W - 1, 0, H - 1};
    if (fabsf(det) > 1e-6f && isfinite(det) && isfinite(t0) && isfinite(t1)) {
        const float r00 = m11 / det, r01 = -m01 / det, r10 = -m10 / det, r11 = m00 / det;
        const float qj = r00 * ((float)x - t0) + r01 * ((float)y - t1), qi = r10 * ((float)x - t0) + r11 * ((float)y - t1);
        // |ix - x| < 1 and |iy - y| < 1  <=>  q in q0 + M^-1 (-1, 1)^2; the slack covers the rounding of the two evaluations
        const float ej = fabsf(r00) + fabsf(r01) + 1e-2f, ei = fabsf(r10) + fabsf(r11) + 1e-2f;
        b.jlo = (int)fmaxf(ceilf(qj - ej), 0.f);
        b.jhi = (int)fminf(floorf(qj + ej), fw - 1.f);
        b.ilo = (int)fmaxf(ceilf(qi - ei), 0.f);
        b.ihi = (int)fminf(floorf(qi + ei), fh - 1.f);
    }
    return b;
}

// the forward weight (tm_warp_taps) of output pixel (j, i) on input pixel (x, y)
__device__ __forceinline__ float tm_warp_weight(const float th[6], int j, int i, int x, int y, int H, int W) {
    float ix, iy;
    tm_warp_sample_pos(th, j, i, H, W, ix, iy);
    const float fx = floorf(ix), fy = floorf(iy);
    const float wx = ((float)x == fx) ? 1.0f - (ix - fx) : (((float)x == fx + 1.0f) ? ix - fx : 0.f);
    const float wy = ((float)y == fy) ? 1.0f - (iy - fy) : (((float)y == fy + 1.0f) ? iy - fy : 0.f);
    return wx * wy;
}

// ---------------------------------------------------------------------------------------------- ConvGRU gates of the training graph (h0 = 0)
//     r = sigmoid(gi_r + b_r),  z = sigmoid(gi_z + b_z),  n = tanh(gi_n + r b_n),  h = n - z n          (b = bias_hh)
// libm expf / tanhf, not common.h's v2x_sigmoid / v2x_tanh: the training graph is compared with torch's own sigmoid / tanh to 1e-6.  The FORWARD function is
// the one definition for the fp32 NCHW and the bf16 NHWC kernel (gru_train.hip).  The backward function serves the fp32 kernel alone: the NHWC backward keeps
// its own copy of these expressions (see there: calling this one changed its stored bits), and the two backwards do NOT agree bit for bit (about one dgi_n in 10^4).
__device__ __forceinline__ float tm_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float tm_gru_gates_fwd(float gi_r, float gi_z, float gi_n, float b_r, float b_z, float b_n) {
    const float r = tm_sigmoid(gi_r + b_r), z = tm_sigmoid(gi_z + b_z);
    const float n = tanhf(gi_n + r * b_n);
    return n - z * n;
}

// dh -> d gi_r, d gi_z, d gi_n and dpre_n * r (whose channel sums are d bias_hh's n part).  gru_gates_nhwc_kernel<true> repeats these expressions in place:
// edit the two together.
// Both copies against float64 on the same bf16 pre-activations (tests/test_gpu_train_sweep.py::test_gru_backward_copies_against_float64, 1x MI355X),
// at (P, C) = (1001, 32) | (1536, 64):
//   this function (fp32 out):   mean error 14.4 | 14.2 fp32 ulps of the element, max 2.2e4 | 2.3e5 -- the maximum sits on saturated gates, where 1 - z and 1 - n^2 cancel and
//                               ANY fp32 evaluation loses the element's low bits: torch's own fp32 ops measure 14.5 | 14.4 mean and the same maxima to the unit; 0.30 | 0.35 of
//                               the sweep's bar (4 x torch's fp32 error).  Rounded to bf16, 26 of 96 096 | 53 of 294 912 elements differ from the float64 result rounded once.
//   the NHWC copy (bf16 out):   27 of 96 096 | 56 of 294 912 stored elements differ from the float64 result rounded once (2.8e-4 | 1.9e-4; the sweep allows 1e-3), none by more
//                               than 0.76 | 0.93 of one bf16 step.
//   the two copies disagree on 7 | 21 elements after the bf16 store ("about one dgi_n in 10^4"): each is within fp32 rounding of float64, neither is the closer one -- the
//   disagreement is where an fp32 difference of a few ulps straddles a bf16 rounding boundary.
__device__ __forceinline__ void tm_gru_gates_bwd(float gi_r, float gi_z, float gi_n, float b_r, float b_z, float b_n, float dh, float &dgi_r, float &dgi_z,
                                                 float &dgi_n, float &dpn_r) {
    const float r = tm_sigmoid(gi_r + b_r), z = tm_sigmoid(gi_z + b_z);
    const float n = tanhf(gi_n + r * b_n);
    const float dn = dh * (1.0f - z), dz = -dh * n;
    const float dpn = dn * (1.0f - n * n);
    const float dr = dpn * b_n;
    dgi_r = dr * r * (1.0f - r);
    dgi_z = dz * z * (1.0f - z);
    dgi_n = dpn;
    dpn_r = dpn * r;
}

// ---------------------------------------------------------------------------------------------- per-channel sums over the pixels of a [M][C] map
// The maps these kernels reduce: a thread owns one group of 8 channels (16 bytes of bf16), 256 threads cover 256 / (C / 8) rows per pass.
static inline bool tm_chan8_shape_ok(long long M, int C) { return M > 0 && C >= 8 && C % 8 == 0 && 256 % (C / 8) == 0; }

// Fixed-order channel partials of a 256-thread workgroup: thread r0 * groups + cg (groups = C / 8, r0 < rpp = 256 / groups) holds the sums acc[8] of channel
// group cg over its rows; thread (r0 == 0, cg) adds the rpp row sets in order and writes part[blockIdx.x][C].  Every thread of the workgroup must call it, once per kernel and as the
// kernel's last use of LDS: red is function-local and no barrier follows the reads.
__device__ __forceinline__ void tm_channel_partials(const float acc[8], int groups, int rpp, int cg, int r0, int C, float *__restrict__ part) {
    __shared__ float red[256][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) red[threadIdx.x][j] = acc[j];
    __syncthreads();
    if (r0 == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float s = 0.f;
            for (int k = 0; k < rpp; ++k) s += red[k * groups + cg][j];
            part[(size_t)blockIdx.x * C + cg * 8 + j] = s;
        }
    }
}

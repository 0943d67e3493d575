// ConvGRU gate arithmetic of the TRAINING graph, forward and backward, as one launch each.
//
// Upstream: convolutional_rnn.Conv2dGRU (V2VNet.py calls convgru(x, None): h0 = 0, so the hidden-to-hidden convolution contributes its bias
// only) -- restated in v2x_sim_amd/train/graph.py::_gru_step:
//     r = sigmoid(gi_r + bh_r),  z = sigmoid(gi_z + bh_z),  n = tanh(gi_n + r bh_n),  h = n - z n
// on the fp32 NCHW pre-activations gi (P, 3C, H, W) of the input convolution (bias_ih included) and bias_hh (3C).  As PyTorch ops that is 8
// elementwise launches forward and ~14 backward; here one each, the backward also producing the tensor whose channel sums are d bias_hh's
// n part (d bias_hh's r and z parts are the channel sums of dgi itself).  Forward arithmetic = expf / tanhf in fp32 (this is the training graph:
// it is compared with torch's own sigmoid / tanh to 1e-6).
//
// Two layouts.  The forward arithmetic is one function (train_math.h: tm_gru_gates_fwd); the fp32 backward calls tm_gru_gates_bwd, the NHWC backward keeps
// the same expressions in place (through the shared function its stored bits change; see the kernel):
//   gru_gates_kernel          fp32 NCHW: gi [P][3C][HW] -> h [P][C][HW]; <true>: dh -> dgi, dpre_n * r               (v2x_gru_gates_f32 / _bwd_f32)
//   gru_gates_nhwc_kernel     bf16 NHWC: gi [P][3C] -> h [P][C]; <true>: dh -> dgi + per-workgroup channel sums      (v2x_gru_gates_nhwc_bf16 / _bwd_bf16)
//   vt_sum_finish_kernel      those sums -> d bias_ih | d bias_hh [6C], fixed order
// The NHWC form serves V2VNet's message-passing rounds between v2v_train.hip's message kernels and the input convolution.
#include "train_math.h"

struct GruGateArgs {
    const float *gi;      // [P][3C][HW]
    const float *bhh;     // [3C]
    const float *dh;      // [P][C][HW] (backward)
    float *h;             // [P][C][HW] (forward)
    float *dgi;           // [P][3C][HW] (backward)
    float *dn_r;          // [P][C][HW] (backward): dpre_n * r, whose channel sums are d bias_hh[2C + c]
    long long P;
    int C, HW4;           // HW / 4
};

template <bool BWD>
__global__ __launch_bounds__(256) void gru_gates_kernel(const GruGateArgs a) {
    const long long total = a.P * a.C * a.HW4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int q = (int)(i % a.HW4);
        const long long pc = i / a.HW4;
        const int c = (int)(pc % a.C);
        const long long p = pc / a.C;
        const size_t base3 = ((size_t)p * 3 * a.C + c) * a.HW4 + q;       // float4 index of the r plane
        const size_t plane = (size_t)a.C * a.HW4;
        const float4 gr = reinterpret_cast<const float4 *>(a.gi)[base3];
        const float4 gz = reinterpret_cast<const float4 *>(a.gi)[base3 + plane];
        const float4 gn = reinterpret_cast<const float4 *>(a.gi)[base3 + 2 * plane];
        const float br = a.bhh[c], bz = a.bhh[a.C + c], bn = a.bhh[2 * a.C + c];
        const float vr[4] = {gr.x, gr.y, gr.z, gr.w}, vz[4] = {gz.x, gz.y, gz.z, gz.w}, vn[4] = {gn.x, gn.y, gn.z, gn.w};
        float o0[4], o1[4], o2[4], o3[4];
        float dh[4] = {0.f, 0.f, 0.f, 0.f};
        if (BWD) {
            const float4 d = reinterpret_cast<const float4 *>(a.dh)[(size_t)pc * a.HW4 + q];
            dh[0] = d.x; dh[1] = d.y; dh[2] = d.z; dh[3] = d.w;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!BWD) o0[k] = tm_gru_gates_fwd(vr[k], vz[k], vn[k], br, bz, bn);
            else tm_gru_gates_bwd(vr[k], vz[k], vn[k], br, bz, bn, dh[k], o0[k], o1[k], o2[k], o3[k]);      // d gi_r, d gi_z, d gi_n, d bias_hh's n part
        }
        if (!BWD) {
            reinterpret_cast<float4 *>(a.h)[(size_t)pc * a.HW4 + q] = make_float4(o0[0], o0[1], o0[2], o0[3]);
        } else {
            reinterpret_cast<float4 *>(a.dgi)[base3] = make_float4(o0[0], o0[1], o0[2], o0[3]);
            reinterpret_cast<float4 *>(a.dgi)[base3 + plane] = make_float4(o1[0], o1[1], o1[2], o1[3]);
            reinterpret_cast<float4 *>(a.dgi)[base3 + 2 * plane] = make_float4(o2[0], o2[1], o2[2], o2[3]);
            reinterpret_cast<float4 *>(a.dn_r)[(size_t)pc * a.HW4 + q] = make_float4(o3[0], o3[1], o3[2], o3[3]);
        }
    }
}

static unsigned gg_grid(long long total) {
    long long b = (total + 255) / 256;
    return (unsigned)(b < 8192 ? (b < 1 ? 1 : b) : 8192);
}

extern "C" int v2x_gru_gates_f32(const float *gi, const float *bias_hh, long long P, int C, int HW, float *h, v2x_stream_t stream) {
    V2X_REQUIRE(gi && bias_hh && h, "v2x_gru_gates_f32: null pointer");
    V2X_REQUIRE(P > 0 && C > 0 && HW > 0 && HW % 4 == 0, "v2x_gru_gates_f32: needs P, C > 0 and H * W %% 4 == 0");
    GruGateArgs a = {};
    a.gi = gi;
    a.bhh = bias_hh;
    a.h = h;
    a.P = P;
    a.C = C;
    a.HW4 = HW / 4;
    hipLaunchKernelGGL(gru_gates_kernel<false>, dim3(gg_grid(P * C * a.HW4)), dim3(256), 0, (hipStream_t)stream, a);
    V2X_CHECK_LAUNCH("gru_gates_kernel");
    return V2X_OK;
}

extern "C" int v2x_gru_gates_bwd_f32(const float *gi, const float *bias_hh, const float *dh, long long P, int C, int HW, float *dgi, float *dn_r,
                                     v2x_stream_t stream) {
    V2X_REQUIRE(gi && bias_hh && dh && dgi && dn_r, "v2x_gru_gates_bwd_f32: null pointer");
    V2X_REQUIRE(P > 0 && C > 0 && HW > 0 && HW % 4 == 0, "v2x_gru_gates_bwd_f32: needs P, C > 0 and H * W %% 4 == 0");
    GruGateArgs a = {};
    a.gi = gi;
    a.bhh = bias_hh;
    a.dh = dh;
    a.dgi = dgi;
    a.dn_r = dn_r;
    a.P = P;
    a.C = C;
    a.HW4 = HW / 4;
    hipLaunchKernelGGL(gru_gates_kernel<true>, dim3(gg_grid(P * C * a.HW4)), dim3(256), 0, (hipStream_t)stream, a);
    V2X_CHECK_LAUNCH("gru_gates_kernel<bwd>");
    return V2X_OK;
}

// ---------------------------------------------------------------------------------------------- the same gates on bf16 NHWC maps (V2VNet's message-passing rounds, v2v_train.hip)
namespace {
struct GatesNhwcArgs {
    const uint16_t *gi;    // [P][3C]  P = maps x pixels
    const float *bhh;      // [3C]
    const uint16_t *dh;    // [P][C]   (backward)
    uint16_t *h;           // [P][C]   (forward)
    uint16_t *dgi;         // [P][3C]  (backward)
    float *partial;        // [blocks][6C] (backward): sums of dgi AS STORED (r, z, n: d bias_ih) | the same r, z | sums of dpre_n * r (d bias_hh)
    long long P;
    int C, rows_per_block;
};

template <bool BWD>
__global__ __launch_bounds__(256) void gru_gates_nhwc_kernel(const GatesNhwcArgs a) {
    __shared__ float red[BWD ? 256 : 1][BWD ? 33 : 1];
    const int G = a.C >> 3;
    const int t = threadIdx.x, g = t % G, sub = t / G, nsub = 256 / G;
    float br[8], bz[8], bn[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        br[c] = a.bhh[g * 8 + c];
        bz[c] = a.bhh[a.C + g * 8 + c];
        bn[c] = a.bhh[2 * a.C + g * 8 + c];
    }
    float s[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) s[c] = 0.f;
    const long long p0 = (long long)blockIdx.x * a.rows_per_block;
    long long p1 = p0 + a.rows_per_block;
    if (p1 > a.P) p1 = a.P;
    const uint4 *gi = reinterpret_cast<const uint4 *>(a.gi);
    for (long long p = p0 + sub; p < p1; p += nsub) {
        float vr[8], vz[8], vn[8];
        tm_unpack8(gi[(size_t)p * 3 * G + g], vr);
        tm_unpack8(gi[(size_t)p * 3 * G + G + g], vz);
        tm_unpack8(gi[(size_t)p * 3 * G + 2 * G + g], vn);
        float dh[8];
        if (BWD) tm_unpack8(reinterpret_cast<const uint4 *>(a.dh)[(size_t)p * G + g], dh);
        float o0[8], o1[8], o2[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (!BWD) {
                o0[c] = tm_gru_gates_fwd(vr[c], vz[c], vn[c], br[c], bz[c], bn[c]);
            } else {
                // tm_gru_gates_bwd's expressions, kept in place: calling the shared function here changed stored bits when it was tried (7 of 96 096 dgi
                // elements at (P, C) = (1001, 32), 21 of 294 912 at (1536, 64), and the sums with them; the compiler contracts the expressions differently).
                // This kernel and the fp32 one already differ in the last bit of a few dgi_n.  A second copy of the formulas -- edit it together with tm_gru_gates_bwd.
                const float r = tm_sigmoid(vr[c] + br[c]), z = tm_sigmoid(vz[c] + bz[c]);
                const float n = tanhf(vn[c] + r * bn[c]);
                const float dn = dh[c] * (1.0f - z), dz = -dh[c] * n;
                const float dpn = dn * (1.0f - n * n);
                const float dr = dpn * bn[c];
                o0[c] = dr * r * (1.0f - r);
                o1[c] = dz * z * (1.0f - z);
                o2[c] = dpn;
                s[24 + c] += dpn * r;
            }
        }
        if (!BWD) {
            reinterpret_cast<uint4 *>(a.h)[(size_t)p * G + g] = tm_pack8(o0);
        } else {
            const uint4 q0 = tm_pack8(o0), q1 = tm_pack8(o1), q2 = tm_pack8(o2);
            uint4 *dg = reinterpret_cast<uint4 *>(a.dgi);
            dg[(size_t)p * 3 * G + g] = q0;
            dg[(size_t)p * 3 * G + G + g] = q1;
            dg[(size_t)p * 3 * G + 2 * G + g] = q2;
            float f0[8], f1[8], f2[8];       // the sums are over the values AS STORED: what the convolution's own gradients see
            tm_unpack8(q0, f0);
            tm_unpack8(q1, f1);
            tm_unpack8(q2, f2);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                s[c] += f0[c];
                s[8 + c] += f1[c];
                s[16 + c] += f2[c];
            }
        }
    }
    if (BWD) {
#pragma unroll
        for (int c = 0; c < 32; ++c) red[t][c] = s[c];
        __syncthreads();
        // thread (g, c) adds the nsub rows of its channel in row order
        for (int o = t; o < G * 32; o += 256) {
            const int gg = o >> 5, c = o & 31;
            float v = 0.f;
            for (int rr = 0; rr < nsub; ++rr) v += red[rr * G + gg][c];
            const int kind = c >> 3, ch = gg * 8 + (c & 7);
            float *row = a.partial + (size_t)blockIdx.x * 6 * a.C;
            if (kind < 3) row[kind * a.C + ch] = v;
            if (kind < 2) row[(3 + kind) * a.C + ch] = v;
            if (kind == 3) row[5 * a.C + ch] = v;
        }
    }
}

// out[c] = sum over the blocks' partials in block order (fp64).  A workgroup owns 32 columns: thread (rg, col) adds rows rg, rg + 8, ... (eight loads in flight,
// 128 contiguous bytes per row), then the eight row groups are added in order -- the same association every run.
__global__ __launch_bounds__(256) void vt_sum_finish_kernel(const float *partial, int n_blocks, int n_cols, float *out) {
    __shared__ double red[8][33];
    const int col = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + col;
    double s = 0.0;
    if (c < n_cols) {
        for (int b0 = rg; b0 < n_blocks; b0 += 64) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = b0 + 8 * k < n_blocks ? partial[(size_t)(b0 + 8 * k) * n_cols + c] : 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) s += (double)v[k];
        }
    }
    red[rg][col] = s;
    __syncthreads();
    if (rg == 0 && c < n_cols) {
        double t = red[0][col];
#pragma unroll
        for (int k = 1; k < 8; ++k) t += red[k][col];
        out[c] = (float)t;
    }
}

constexpr int GATES_MAX_BLOCKS = 256;

int gates_plan(long long P, int C, int &rows_per_block) {
    const int nsub = 256 / (C / 8);
    long long rpb = (P + GATES_MAX_BLOCKS - 1) / GATES_MAX_BLOCKS;
    rpb = (rpb + nsub - 1) / nsub * nsub;
    rows_per_block = (int)rpb;
    return (int)((P + rpb - 1) / rpb);
}
}  // namespace

extern "C" int v2x_gru_gates_nhwc_bf16(const uint16_t *gi, const float *bias_hh, long long P, int C, uint16_t *h, v2x_stream_t stream) {
    V2X_REQUIRE(gi && bias_hh && h, "v2x_gru_gates_nhwc_bf16: null pointer");
    V2X_REQUIRE(tm_chan8_shape_ok(P, C), "v2x_gru_gates_nhwc_bf16: needs P > 0 and C in {8, 16, 32, ..., 2048} (C / 8 divides 256), got P=%lld C=%d", P, C);
    GatesNhwcArgs a = {};
    a.gi = gi;
    a.bhh = bias_hh;
    a.h = h;
    a.P = P;
    a.C = C;
    // forward: plenty of small workgroups (no partials to keep few)
    const int nsub = 256 / (C / 8);
    a.rows_per_block = nsub * 4;
    const long long blocks = (P + a.rows_per_block - 1) / a.rows_per_block;
    hipLaunchKernelGGL(gru_gates_nhwc_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    V2X_CHECK_LAUNCH("gru_gates_nhwc_kernel");
    return V2X_OK;
}

extern "C" long long v2x_gru_gates_nhwc_workspace_size(long long P, int C) {
    if (!tm_chan8_shape_ok(P, C)) return 0;
    int rpb;
    return (long long)gates_plan(P, C, rpb) * 6 * C * (long long)sizeof(float);
}

extern "C" int v2x_gru_gates_nhwc_bwd_bf16(const uint16_t *gi, const float *bias_hh, const uint16_t *dh, long long P, int C, uint16_t *dgi, float *sums6c,
                                           float *workspace, v2x_stream_t stream) {
    V2X_REQUIRE(gi && bias_hh && dh && dgi && sums6c && workspace, "v2x_gru_gates_nhwc_bwd_bf16: null pointer");
    V2X_REQUIRE(tm_chan8_shape_ok(P, C), "v2x_gru_gates_nhwc_bwd_bf16: needs P > 0 and C in {8, 16, 32, ..., 2048} (C / 8 divides 256), got P=%lld C=%d", P, C);
    GatesNhwcArgs a = {};
    a.gi = gi;
    a.bhh = bias_hh;
    a.dh = dh;
    a.dgi = dgi;
    a.partial = workspace;
    a.P = P;
    a.C = C;
    const int nblk = gates_plan(P, C, a.rows_per_block);
    hipLaunchKernelGGL(gru_gates_nhwc_kernel<true>, dim3(nblk), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(vt_sum_finish_kernel, dim3((6 * C + 31) / 32), dim3(256), 0, (hipStream_t)stream, workspace, nblk, 6 * C, sums6c);
    V2X_CHECK_LAUNCH("gru_gates_nhwc_kernel<bwd>");
    return V2X_OK;
}

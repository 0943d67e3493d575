// Segmentation loss of the training step -- pixel-wise softmax cross entropy with class weights and ignored labels -- forward and backward
// (SURVEY.md section 8 rows a8 / f-3).
//
// Upstream: coperception/utils/SegModule.py::SegModule.step's nn.CrossEntropyLoss (absent from /root/reference; README.md:101 names the training
// scripts that use it); this build's restatement is v2x_sim_amd/train/loss.py::segmentation_loss:
//     valid_i = label_i < C          (any label >= C is ignored; 255 is the conventional value)
//     w_i     = valid_i * (weight[label_i] or 1)
//     nll_i   = logsumexp(logits_i) - logits_i[label_i]
//     num = sum w_i nll_i,   den = sum w_i,   loss = num / (den > 0 ? den : 1)
//     d loss / d logit_ij = g w_i (softmax_ij - [j == label_i]) / den
// As PyTorch ops (log_softmax, nll_loss and their backward kernels, then the head's pad / cast / sum) that is ~10 launches and seven passes over the
// logits or their gradients per step.  Here: one pass for (num, den) (per-workgroup partials, added in workgroup order in fp64: bit-reproducible, no
// atomics), one tiny finish launch, and ONE pass for the gradients that reads g and den from device memory (nothing returns to the host: the step
// stays capturable).  The gradient pass has two output forms over the SAME per-pixel function (sl_pixel_grad): (a) fp32 [M][C]; (b) what
// v2x_cast_pad_chsum_f32 would make of (a) -- bf16 [M][Cp] with zero padding channels plus the fp32 per-channel sums (the class head's bias
// gradient; fixed-order workgroup partials + a finish launch) -- so the fp32 gradient never reaches HBM on the way into the head's kernels.
//
// A thread owns a pixel: its C = 4 NQ logits are NQ 16-byte loads into registers (NQ is a template parameter: every index is static, nothing goes
// to scratch), the row's arithmetic needs no exchange between lanes.  Accuracy: libm expf / logf; the label's own term is formed without
// cancellation -- nll = log(s) + (max - x_label), softmax_label - 1 = -(sum of the OTHER terms) / s.
#include "train_math.h"

constexpr int SL_THREADS = 256;
constexpr int SL_FWD_PIX = 2048, SL_FWD_MAX_BLOCKS = 1024;     // forward: >= 8 pixels per thread
constexpr int SL_BWD_PIX = 1024, SL_BWD_MAX_BLOCKS = 2048;     // backward (a): >= 4 pixels per thread
constexpr int SL_PK_PIX = 1024, SL_PK_MAX_BLOCKS = 1024;       // backward (b): one row of channel partials per workgroup

struct SegLossArgs {
    const float *logits;        // [M][C]
    const uint8_t *lab;         // [M]
    const float *weight;        // [C] or null
    long long M;
    int C, Cp;
    float *part;                // forward: [n_blocks][2] (num, den); packed backward: [n_blocks][C]
    float *out;                 // [3]: loss, num, den
    const float *g_loss;        // incoming gradient of the loss (device scalar; null = 1)
    float *dlogits;             // form (a)
    uint16_t *dy;               // form (b)
    int n_blocks;
};

template <int NQ>
__device__ __forceinline__ void sl_load_row(const float *__restrict__ logits, long long i, float x[4 * NQ]) {
    const float4 *p = reinterpret_cast<const float4 *>(logits) + i * NQ;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const float4 t = p[q];
        x[4 * q] = t.x;
        x[4 * q + 1] = t.y;
        x[4 * q + 2] = t.z;
        x[4 * q + 3] = t.w;
    }
}

// x -> e_j = exp(x_j - max) in place;  -> s = sum e_j, m = max, xl = x_label, so = the sum of the terms other than the label's.  The label's place is tested in
// two levels -- its quad (l >> 2 against q) and its place in the quad (l & 3 against t): 4 + NQ predicates instead of 4 NQ (at C = 32 the per-channel
// predicates alone outran the scalar registers).  Both sums go quad by quad: s = sum_q (e_4q + e_4q+1 + e_4q+2 + e_4q+3).
template <int NQ>
__device__ __forceinline__ void sl_softmax_terms(float x[4 * NQ], int l, float &s, float &m, float &xl, float &so) {
    const int lq = l >> 2, lt = l & 3;
    m = x[0];
    xl = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        float c = x[4 * q];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            m = fmaxf(m, x[4 * q + t]);
            c = (lt == t) ? x[4 * q + t] : c;
        }
        xl = (lq == q) ? c : xl;
    }
    s = 0.f;
    so = 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        float full = 0.f, excl = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float e = expf(x[4 * q + t] - m);
            x[4 * q + t] = e;
            full += e;
            excl += (lt == t) ? 0.f : e;
        }
        s += full;
        so += (lq == q) ? excl : full;
    }
}

// THE per-pixel gradient of both backward forms: d[j] = kw (softmax_j - [j == l]), kw = g w_i / den.  An ignored pixel is exactly zero (its logits are not read).
template <int NQ>
__device__ __forceinline__ void sl_pixel_grad(const float *__restrict__ logits, long long i, int l, float kw, float d[4 * NQ]) {
    if (l >= 4 * NQ) {
#pragma unroll
        for (int j = 0; j < 4 * NQ; ++j) d[j] = 0.f;
        return;
    }
    float s, m, xl, so;
    sl_load_row<NQ>(logits, i, d);
    sl_softmax_terms<NQ>(d, l, s, m, xl, so);
    const int lq = l >> 2, lt = l & 3;
    const float inv = 1.0f / s, pl = -(so * inv);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float p = d[4 * q + t] * inv;
            const float in_quad = (lt == t) ? pl : p;
            d[4 * q + t] = kw * ((lq == q) ? in_quad : p);
        }
    }
}

// g / den as the backward kernels read it (den = 0: every w_i is 0 and so is every gradient)
__device__ __forceinline__ float sl_scale(const SegLossArgs &a) {
    const float den = a.out[2];
    return (a.g_loss ? *a.g_loss : 1.0f) / (den > 0.f ? den : 1.0f);
}

__device__ __forceinline__ float sl_weight(const SegLossArgs &a, int l) { return l < a.C ? (a.weight ? a.weight[l] : 1.0f) : 0.f; }

// fixed-order sum of one value per thread over the workgroup (wave butterfly, then the four waves in wave order)
__device__ __forceinline__ float sl_block_sum(float v, float *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

template <int NQ>
__global__ __launch_bounds__(SL_THREADS) void seg_loss_partial_kernel(const SegLossArgs a) {
    __shared__ float red[4];
    float num = 0.f, den = 0.f;
    for (long long i = (long long)blockIdx.x * SL_THREADS + threadIdx.x; i < a.M; i += (long long)gridDim.x * SL_THREADS) {
        const int l = a.lab[i];
        if (l >= 4 * NQ) continue;
        const float w = sl_weight(a, l);
        float x[4 * NQ], s, m, xl, so;
        sl_load_row<NQ>(a.logits, i, x);
        sl_softmax_terms<NQ>(x, l, s, m, xl, so);
        num += w * (logf(s) + (m - xl));
        den += w;
    }
    const float s0 = sl_block_sum(num, red), s1 = sl_block_sum(den, red);
    if (threadIdx.x == 0) {
        a.part[blockIdx.x * 2 + 0] = s0;
        a.part[blockIdx.x * 2 + 1] = s1;
    }
}

// one workgroup: thread t adds partials t, t + 256, ... in fp64, then a fixed tree
__global__ __launch_bounds__(SL_THREADS) void seg_loss_finish_kernel(const SegLossArgs a) {
    __shared__ double r[2][SL_THREADS];
    double s[2] = {0.0, 0.0};
    for (int b = threadIdx.x; b < a.n_blocks; b += SL_THREADS) {
        s[0] += (double)a.part[b * 2 + 0];
        s[1] += (double)a.part[b * 2 + 1];
    }
    r[0][threadIdx.x] = s[0];
    r[1][threadIdx.x] = s[1];
    __syncthreads();
    for (int w = SL_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            r[0][threadIdx.x] += r[0][threadIdx.x + w];
            r[1][threadIdx.x] += r[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double num = r[0][0], den = r[1][0];
        a.out[0] = (float)(num / (den > 0.0 ? den : 1.0));
        a.out[1] = (float)num;
        a.out[2] = (float)den;
    }
}

// form (a): fp32 [M][C]
template <int NQ>
__global__ __launch_bounds__(SL_THREADS) void seg_loss_backward_kernel(const SegLossArgs a) {
    const float k = sl_scale(a);
    for (long long i = (long long)blockIdx.x * SL_THREADS + threadIdx.x; i < a.M; i += (long long)gridDim.x * SL_THREADS) {
        const int l = a.lab[i];
        float d[4 * NQ];
        sl_pixel_grad<NQ>(a.logits, i, l, k * sl_weight(a, l), d);
        float4 *o = reinterpret_cast<float4 *>(a.dlogits) + i * NQ;
#pragma unroll
        for (int q = 0; q < NQ; ++q) o[q] = make_float4(d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]);
    }
}

// form (b): bf16 [M][Cp], channels C.. zero, + per-workgroup partial channel sums of the fp32 values part[blockIdx.x][C]
template <int NQ>
__global__ __launch_bounds__(SL_THREADS) void seg_loss_backward_packed_kernel(const SegLossArgs a) {
    constexpr int C = 4 * NQ, G = (C + 7) / 8;      // G: the 8-channel groups that hold data
    __shared__ float red[4][C];
    const float k = sl_scale(a);
    const int groups = a.Cp / 8;
    float acc[C];
#pragma unroll
    for (int j = 0; j < C; ++j) acc[j] = 0.f;
    for (long long i = (long long)blockIdx.x * SL_THREADS + threadIdx.x; i < a.M; i += (long long)gridDim.x * SL_THREADS) {
        const int l = a.lab[i];
        float d[C];
        sl_pixel_grad<NQ>(a.logits, i, l, k * sl_weight(a, l), d);
#pragma unroll
        for (int j = 0; j < C; ++j) acc[j] += d[j];
        uint4 *o = reinterpret_cast<uint4 *>(a.dy + i * a.Cp);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float f[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = (8 * g + j < C) ? d[(8 * g + j < C) ? 8 * g + j : 0] : 0.f;
            o[g] = tm_pack8(f);
        }
        for (int g = G; g < groups; ++g) o[g] = make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int j = 0; j < C; ++j) {
        float v = acc[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < C) a.part[(size_t)blockIdx.x * C + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// sums[c] = the workgroups' partials of channel c: one wave per channel, lane l adds partials l, l + 64, ... in order (fp64), then a fixed butterfly
__global__ __launch_bounds__(256) void seg_loss_sums_finish_kernel(const float *__restrict__ part, int nblk, int C, float *__restrict__ sums) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= C) return;
    double s = 0.0;
    for (int b = lane; b < nblk; b += 64) s += (double)part[(size_t)b * C + c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) sums[c] = (float)s;
}

// ---- grids: one small function each (tests/seg_loss_refs.py mirrors them)
static int sl_grid(long long M, int pix, int cap) {
    long long b = (M + pix - 1) / pix;
    if (b < 1) b = 1;
    return (int)(b < cap ? b : cap);
}
static int sl_fwd_blocks(long long M) { return sl_grid(M, SL_FWD_PIX, SL_FWD_MAX_BLOCKS); }
static int sl_bwd_blocks(long long M) { return sl_grid(M, SL_BWD_PIX, SL_BWD_MAX_BLOCKS); }
static int sl_pk_blocks(long long M) { return sl_grid(M, SL_PK_PIX, SL_PK_MAX_BLOCKS); }

#define SL_LAUNCH(KERNEL, C, ...)                                                        \
    switch ((C) / 4) {                                                                   \
        case 1: hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__); break;                       \
        case 2: hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__); break;                       \
        case 3: hipLaunchKernelGGL(KERNEL<3>, __VA_ARGS__); break;                       \
        case 4: hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__); break;                       \
        case 5: hipLaunchKernelGGL(KERNEL<5>, __VA_ARGS__); break;                       \
        case 6: hipLaunchKernelGGL(KERNEL<6>, __VA_ARGS__); break;                       \
        case 7: hipLaunchKernelGGL(KERNEL<7>, __VA_ARGS__); break;                       \
        default: hipLaunchKernelGGL(KERNEL<8>, __VA_ARGS__); break;                      \
    }

extern "C" long long v2x_seg_loss_workspace_size(long long M, int C, int Cp) {
    if (M <= 0 || C < 4 || C > 32 || C % 4) return 0;
    long long floats = (long long)sl_fwd_blocks(M) * 2;
    if (Cp != 0) {
        if (Cp < C || !tm_chan8_shape_ok(M, Cp)) return 0;
        const long long pk = (long long)sl_pk_blocks(M) * C;
        if (pk > floats) floats = pk;
    }
    return floats * (long long)sizeof(float);
}

static int sl_check(const char *what, const float *logits, const uint8_t *labels, long long M, int C) {
    V2X_REQUIRE(logits && labels, "%s: null pointer", what);
    V2X_REQUIRE(M > 0 && C >= 4 && C <= 32 && C % 4 == 0, "%s: needs M > 0, C %% 4 == 0 and 4 <= C <= 32, got M=%lld C=%d", what, M, C);
    V2X_REQUIRE((reinterpret_cast<uintptr_t>(logits) & 15) == 0, "%s: logits must be 16-byte aligned", what);
    return V2X_OK;
}

extern "C" int v2x_seg_loss_forward(const float *logits, const uint8_t *labels, const float *weight, long long M, int C, float *out3, float *workspace,
                                    v2x_stream_t stream) {
    if (int rc = sl_check("v2x_seg_loss_forward", logits, labels, M, C)) return rc;
    V2X_REQUIRE(out3 && workspace, "v2x_seg_loss_forward: null pointer");
    SegLossArgs a = {};
    a.logits = logits;
    a.lab = labels;
    a.weight = weight;
    a.M = M;
    a.C = C;
    a.part = workspace;
    a.out = out3;
    a.n_blocks = sl_fwd_blocks(M);
    hipStream_t s = (hipStream_t)stream;
    SL_LAUNCH(seg_loss_partial_kernel, C, dim3(a.n_blocks), dim3(SL_THREADS), 0, s, a);
    hipLaunchKernelGGL(seg_loss_finish_kernel, dim3(1), dim3(SL_THREADS), 0, s, a);
    V2X_CHECK_LAUNCH("seg_loss_forward");
    return V2X_OK;
}

extern "C" int v2x_seg_loss_backward(const float *logits, const uint8_t *labels, const float *weight, long long M, int C, const float *out3,
                                     const float *g_loss, float *dlogits, v2x_stream_t stream) {
    if (int rc = sl_check("v2x_seg_loss_backward", logits, labels, M, C)) return rc;
    V2X_REQUIRE(out3 && dlogits, "v2x_seg_loss_backward: null pointer");
    V2X_REQUIRE((reinterpret_cast<uintptr_t>(dlogits) & 15) == 0, "v2x_seg_loss_backward: dlogits must be 16-byte aligned");
    SegLossArgs a = {};
    a.logits = logits;
    a.lab = labels;
    a.weight = weight;
    a.M = M;
    a.C = C;
    a.out = const_cast<float *>(out3);
    a.g_loss = g_loss;
    a.dlogits = dlogits;
    a.n_blocks = sl_bwd_blocks(M);
    SL_LAUNCH(seg_loss_backward_kernel, C, dim3(a.n_blocks), dim3(SL_THREADS), 0, (hipStream_t)stream, a);
    V2X_CHECK_LAUNCH("seg_loss_backward_kernel");
    return V2X_OK;
}

extern "C" int v2x_seg_loss_backward_packed(const float *logits, const uint8_t *labels, const float *weight, long long M, int C, const float *out3,
                                            const float *g_loss, int Cp, uint16_t *dy, float *sums, float *workspace, v2x_stream_t stream) {
    if (int rc = sl_check("v2x_seg_loss_backward_packed", logits, labels, M, C)) return rc;
    V2X_REQUIRE(out3 && dy && sums && workspace, "v2x_seg_loss_backward_packed: null pointer");
    V2X_REQUIRE(Cp >= C && tm_chan8_shape_ok(M, Cp), "v2x_seg_loss_backward_packed: needs Cp >= C, Cp in {8, 16, 32, ...} (Cp / 8 divides 256), got C=%d Cp=%d", C, Cp);
    V2X_REQUIRE((reinterpret_cast<uintptr_t>(dy) & 15) == 0, "v2x_seg_loss_backward_packed: dy must be 16-byte aligned");
    SegLossArgs a = {};
    a.logits = logits;
    a.lab = labels;
    a.weight = weight;
    a.M = M;
    a.C = C;
    a.Cp = Cp;
    a.out = const_cast<float *>(out3);
    a.g_loss = g_loss;
    a.dy = dy;
    a.part = workspace;
    a.n_blocks = sl_pk_blocks(M);
    hipStream_t s = (hipStream_t)stream;
    SL_LAUNCH(seg_loss_backward_packed_kernel, C, dim3(a.n_blocks), dim3(SL_THREADS), 0, s, a);
    hipLaunchKernelGGL(seg_loss_sums_finish_kernel, dim3((C + 3) / 4), dim3(256), 0, s, workspace, a.n_blocks, C, sums);
    V2X_CHECK_LAUNCH("seg_loss_backward_packed");
    return V2X_OK;
}

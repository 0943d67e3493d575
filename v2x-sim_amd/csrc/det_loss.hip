// Detection loss of the training step, forward and backward, as three launches.
//
// Upstream: coperception/utils/loss.py (SoftmaxFocalClassificationLoss, WeightedSmoothL1LocalizationLoss) combined in
// coperception/utils/CoDetModule.py::FaFModule.loss_calculator (absent from /root/reference; README.md:101 names the training scripts that use
// them); this build's restatement is v2x_sim_amd/train/loss.py::detection_loss:
//     cls  = sum over anchors of  -alpha_t (1 - p_t)^2 sum_k l_k log p_k,   p = softmax(logits), p_t = sum_k l_k p_k, alpha_t = 0.25 l_1 + 0.75 l_0
//     loc  = sum over anchors with mask of smooth_l1(x - t; beta = 1/9) over the 6 box codes
//     n    = max(sum l_1, 1);   loss = cls / n + loc / n
// As PyTorch ops that is ~45 elementwise / reduction launches over 31 + 94 MB tensors per 10-map step (0.6 ms of a 5.8-ms step, forward + backward).
// Here: one pass for the three sums (per-workgroup partials, added in workgroup order in fp64: bit-reproducible, no atomics), one tiny finish
// launch, and one pass for both gradients that reads the incoming scalar gradients from device memory (nothing returns to the host: the step
// stays capturable).  The gradient formulas are the derivatives autograd forms for the expressions above, for ANY label pair (l_0, l_1):
//     d cls / d c_j = -alpha_t [ -2 (1 - p_t) p_j (l_j - p_t) s + (1 - p_t)^2 (l_j - p_j (l_0 + l_1)) ],   s = sum_k l_k log p_k
//     d loc / d x   = mask * (|d| < beta ? d / beta : sign(d)),   d = x - t
// The corner form of the localisation term (loss_type = "corner_loss") lives in det_corner_loss.hip; det_loss_common.h holds what the two files share.
#include "det_loss_common.h"

__global__ __launch_bounds__(DL_THREADS) void det_loss_partial_kernel(const DetLossArgs a) {
    __shared__ float red[4];
    float npos = 0.f, cs = 0.f, ls = 0.f;
    const float inv_beta = 1.0f / a.beta, half_beta = 0.5f * a.beta;
    for (long long i = (long long)blockIdx.x * DL_THREADS + threadIdx.x; i < a.n; i += (long long)gridDim.x * DL_THREADS) {
        const float2 c = reinterpret_cast<const float2 *>(a.cls)[i];
        const float2 l = reinterpret_cast<const float2 *>(a.lab)[i];
        const FocalTerms f = focal_terms(c.x, c.y, l.x, l.y, a.alpha);
        const float om = 1.0f - f.pt;
        cs += -f.alpha_t * (om * om) * f.s;
        npos += l.y;
        if (a.mask[i]) {
            const float2 *x = reinterpret_cast<const float2 *>(a.loc) + 3 * i;
            const float2 *t = reinterpret_cast<const float2 *>(a.tgt) + 3 * i;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float2 xv = x[k], tv = t[k];
                const float d0 = fabsf(xv.x - tv.x), d1 = fabsf(xv.y - tv.y);
                acc += d0 < a.beta ? 0.5f * d0 * d0 * inv_beta : d0 - half_beta;
                acc += d1 < a.beta ? 0.5f * d1 * d1 * inv_beta : d1 - half_beta;
            }
            ls += acc;
        }
    }
    const float s0 = block_sum(npos, red), s1 = block_sum(cs, red), s2 = block_sum(ls, red);
    if (threadIdx.x == 0) {
        a.part[blockIdx.x * 3 + 0] = s0;
        a.part[blockIdx.x * 3 + 1] = s1;
        a.part[blockIdx.x * 3 + 2] = s2;
    }
}

__global__ __launch_bounds__(DL_THREADS) void det_loss_backward_kernel(const DetLossArgs a) {
    const float n = a.out[3];
    const float g0 = a.g_loss ? *a.g_loss : 0.f;
    const float gc = (g0 + (a.g_cls ? *a.g_cls : 0.f)) / n;
    const float gl = (g0 + (a.g_loc ? *a.g_loc : 0.f)) / n;
    const float inv_beta = 1.0f / a.beta;
    for (long long i = (long long)blockIdx.x * DL_THREADS + threadIdx.x; i < a.n; i += (long long)gridDim.x * DL_THREADS) {
        const float2 c = reinterpret_cast<const float2 *>(a.cls)[i];
        const float2 l = reinterpret_cast<const float2 *>(a.lab)[i];
        const FocalTerms f = focal_terms(c.x, c.y, l.x, l.y, a.alpha);
        const float om = 1.0f - f.pt, L = l.x + l.y;
        const float k1 = 2.0f * om * f.s, k2 = om * om;
        float2 dc;
        dc.x = gc * (-f.alpha_t) * (-k1 * f.p0 * (l.x - f.pt) + k2 * (l.x - f.p0 * L));
        dc.y = gc * (-f.alpha_t) * (-k1 * f.p1 * (l.y - f.pt) + k2 * (l.y - f.p1 * L));
        reinterpret_cast<float2 *>(a.dcls)[i] = dc;
        float2 *dx = reinterpret_cast<float2 *>(a.dloc) + 3 * i;
        if (a.mask[i]) {
            const float2 *x = reinterpret_cast<const float2 *>(a.loc) + 3 * i;
            const float2 *t = reinterpret_cast<const float2 *>(a.tgt) + 3 * i;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float2 xv = x[k], tv = t[k];
                const float d0 = xv.x - tv.x, d1 = xv.y - tv.y;
                float2 o;
                o.x = gl * (fabsf(d0) < a.beta ? d0 * inv_beta : (d0 > 0.f ? 1.f : (d0 < 0.f ? -1.f : 0.f)));
                o.y = gl * (fabsf(d1) < a.beta ? d1 * inv_beta : (d1 > 0.f ? 1.f : (d1 < 0.f ? -1.f : 0.f)));
                dx[k] = o;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) dx[k] = make_float2(0.f, 0.f);
        }
    }
}

extern "C" long long v2x_det_loss_workspace_size(long long n_anchors) {
    if (n_anchors <= 0) return 0;
    return (long long)dl_blocks(n_anchors) * 3 * (long long)sizeof(float);
}

extern "C" int v2x_det_loss_forward(const float *cls, const float *labels, const float *loc, const float *targets, const uint8_t *mask,
                                    long long n_anchors, float alpha, float beta, float *out4, float *workspace, v2x_stream_t stream) {
    V2X_REQUIRE(cls && labels && loc && targets && mask && out4 && workspace, "v2x_det_loss_forward: null pointer");
    V2X_REQUIRE(n_anchors > 0 && beta > 0.f, "v2x_det_loss_forward: needs n_anchors > 0 and beta > 0");
    DetLossArgs a = {};
    a.cls = cls;
    a.lab = labels;
    a.loc = loc;
    a.tgt = targets;
    a.mask = mask;
    a.n = n_anchors;
    a.alpha = alpha;
    a.beta = beta;
    a.part = workspace;
    a.out = out4;
    a.n_blocks = dl_blocks(n_anchors);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(det_loss_partial_kernel, dim3(a.n_blocks), dim3(DL_THREADS), 0, s, a);
    hipLaunchKernelGGL(det_loss_finish_kernel, dim3(1), dim3(DL_THREADS), 0, s, a);
    V2X_CHECK_LAUNCH("det_loss_forward");
    return V2X_OK;
}

extern "C" int v2x_det_loss_backward(const float *cls, const float *labels, const float *loc, const float *targets, const uint8_t *mask,
                                     long long n_anchors, float alpha, float beta, const float *out4, const float *g_loss, const float *g_cls,
                                     const float *g_loc, float *dcls, float *dloc, v2x_stream_t stream) {
    V2X_REQUIRE(cls && labels && loc && targets && mask && out4 && dcls && dloc, "v2x_det_loss_backward: null pointer");
    V2X_REQUIRE(n_anchors > 0 && beta > 0.f, "v2x_det_loss_backward: needs n_anchors > 0 and beta > 0");
    DetLossArgs a = {};
    a.cls = cls;
    a.lab = labels;
    a.loc = loc;
    a.tgt = targets;
    a.mask = mask;
    a.n = n_anchors;
    a.alpha = alpha;
    a.beta = beta;
    a.out = const_cast<float *>(out4);
    a.g_loss = g_loss;
    a.g_cls = g_cls;
    a.g_loc = g_loc;
    a.dcls = dcls;
    a.dloc = dloc;
    long long b = (n_anchors + DL_THREADS * 4 - 1) / (DL_THREADS * 4);
    if (b > 4096) b = 4096;
    hipLaunchKernelGGL(det_loss_backward_kernel, dim3((unsigned)b), dim3(DL_THREADS), 0, (hipStream_t)stream, a);
    V2X_CHECK_LAUNCH("det_loss_backward_kernel");
    return V2X_OK;
}

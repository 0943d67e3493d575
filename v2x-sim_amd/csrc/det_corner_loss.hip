// Detection loss with the corner form of the localisation term (Config.loss_type = "corner_loss"), forward and backward, as three launches
// (DESIGN.md section 3.10 is the specification, restated here).
//
// Upstream: coperception/utils/CoDetModule.py::FaFModule.loss_calculator switches on config.loss_type; its corner_loss is absent from
// /root/reference, so the statement is build-owned: v2x_sim_amd/train/loss.py::detection_loss(loss_type="corner_loss") in PyTorch ops.
//   For every anchor i with mask_i, the predicted codes x_i and the target codes t_i are decoded through the SAME anchor row a = anchors[i mod m]
//   (utils/postprocess.py::decode_boxes, postprocess.hip's decode):
//       x = xa + dx,  y = ya + dy,  w = wa exp(clip(dw, -4, 4)),  h = ha exp(clip(dh, -4, 4)),  yaw = atan2(sa, ca) + atan2(ds, dc)
//       atan2(ds, dc) at ds = dc = 0 (either sign of zero): value 0, gradient 0
//   corners as utils/postprocess.py::box_corners lays them: with L the extent along the heading (w; h under wh_swap) and P the other one,
//       u = L/2 (cos yaw, sin yaw),  v = P/2 (-sin yaw, cos yaw),  corner_k = (x, y) + sx_k u + sy_k v,  (sx, sy) = (+,+), (-,+), (-,-), (+,-)
//       loc = sum_i mask_i sum_k |corner_k(x_i) - corner_k(t_i)|_2
//   cls = the focal term of det_loss.hip, unchanged;  n = max(sum l_1, 1);  out4 = {cls / n + loc / n, cls / n, loc / n, n}.
//   The anchor centre cancels in the difference and is cancelled here (more accurate; only (wa, ha, sa, ca) are read):
//       D_k = (dx_x - dx_t, dy_x - dy_t) + sx_k U + sy_k V,   U = u_x - u_t,  V = v_x - v_t
//   The codes of an unselected anchor are NOT READ (they may be inf or NaN): it adds exactly 0 and its dloc row is exactly 0.
// Backward, written out (recomputed from the inputs, nothing saved per anchor).  With n_k = D_k / |D_k| (0 where |D_k| = 0):
//       G_D = sum n_k,  G_U = sum sx_k n_k,  G_V = sum sy_k n_k
//       d/d dx = G_D.x,  d/d dy = G_D.y
//       d/dL = (G_U . (c, s)) / 2,  d/dP = (G_V . (-s, c)) / 2,  d/dyaw = L/2 (G_U . (-s, c)) - P/2 (G_V . (c, s))
//       d/d dw = d/dw * w * [-4 <= dw <= 4]  (w = L, or P under wh_swap),  d/d dh likewise  (torch.clamp's gradient: passes at the bounds)
//       d/d ds = d/dyaw * dc / (ds^2 + dc^2),  d/d dc = -d/dyaw * ds / (ds^2 + dc^2);  both 0 at ds = dc = 0
//   times (g_loss + g_loc) / n.  dcls: det_loss.hip's formula.
// The decode uses expf / atan2f / sincosf at library accuracy (the test bar is tied to torch's fp32 evaluation).  The products that form u and v
// are __fmul_rn and the two functions that form D_k are compiled with fp contract(off): the compiler must not contract a product into the
// subtraction U = u_x - u_t, or bit-equal codes would leave a rounding residue instead of the exact 0 whose gradient is defined as 0.
// No atomics, fixed summation order (det_loss_common.h): bit-reproducible; nothing returns to the host: capturable.
#include "det_loss_common.h"

struct CornerBox {
    float w, h;          // decoded extents
    float hl, hp;        // half extent along the heading / across it
    float c, s;          // cos yaw, sin yaw
    float ux, uy, vx, vy;
};

// codes x[0] = (dx, dy), x[1] = (dw, dh), x[2] = (ds, dc); the anchor's (wa, ha) and yaw_a = atan2f(sa, ca)
__device__ __forceinline__ CornerBox corner_decode(float2 wh_code, float2 sc_code, float wa, float ha, float yaw_a, int swap) {
#pragma clang fp contract(off)
    CornerBox b;
    b.w = wa * expf(fminf(fmaxf(wh_code.x, -4.0f), 4.0f));
    b.h = ha * expf(fminf(fmaxf(wh_code.y, -4.0f), 4.0f));
    const float dyaw = (sc_code.x == 0.0f && sc_code.y == 0.0f) ? 0.0f : atan2f(sc_code.x, sc_code.y);
    sincosf(yaw_a + dyaw, &b.s, &b.c);
    b.hl = 0.5f * (swap ? b.h : b.w);
    b.hp = 0.5f * (swap ? b.w : b.h);
    b.ux = __fmul_rn(b.hl, b.c);
    b.uy = __fmul_rn(b.hl, b.s);
    b.vx = -__fmul_rn(b.hp, b.s);
    b.vy = __fmul_rn(b.hp, b.c);
    return b;
}

struct CornerDiff {
    float x[4], y[4];    // D_k in corner order (+,+), (-,+), (-,-), (+,-)
};

__device__ __forceinline__ CornerDiff corner_diff(float2 dxy_x, float2 dxy_t, const CornerBox &p, const CornerBox &t) {
#pragma clang fp contract(off)
    const float Dx = dxy_x.x - dxy_t.x, Dy = dxy_x.y - dxy_t.y;
    const float Ux = p.ux - t.ux, Uy = p.uy - t.uy, Vx = p.vx - t.vx, Vy = p.vy - t.vy;
    const float Ax = Dx + Ux, Ay = Dy + Uy, Bx = Dx - Ux, By = Dy - Uy;
    CornerDiff d;
    d.x[0] = Ax + Vx; d.y[0] = Ay + Vy;
    d.x[1] = Bx + Vx; d.y[1] = By + Vy;
    d.x[2] = Bx - Vx; d.y[2] = By - Vy;
    d.x[3] = Ax - Vx; d.y[3] = Ay - Vy;
    return d;
}

__global__ __launch_bounds__(DL_THREADS) void det_corner_loss_partial_kernel(const DetLossArgs a) {
    __shared__ float red[4];
    float npos = 0.f, cs = 0.f, ls = 0.f;
    const long long stride = (long long)gridDim.x * DL_THREADS;
    const long long rstep = stride % a.m;
    long long i = (long long)blockIdx.x * DL_THREADS + threadIdx.x;
    long long r = i % a.m;                                          // the anchor row of i, stepped with i (no division in the loop)
    for (; i < a.n; i += stride, r = (r + rstep >= a.m ? r + rstep - a.m : r + rstep)) {
        const float2 c = reinterpret_cast<const float2 *>(a.cls)[i];
        const float2 l = reinterpret_cast<const float2 *>(a.lab)[i];
        const FocalTerms f = focal_terms(c.x, c.y, l.x, l.y, a.alpha);
        const float om = 1.0f - f.pt;
        cs += -f.alpha_t * (om * om) * f.s;
        npos += l.y;
        if (a.mask[i]) {
            const float2 *x = reinterpret_cast<const float2 *>(a.loc) + 3 * i;
            const float2 *t = reinterpret_cast<const float2 *>(a.tgt) + 3 * i;
            const float2 *an = reinterpret_cast<const float2 *>(a.anchors) + 3 * r;
            const float2 awh = an[1], asc = an[2];
            const float yaw_a = atan2f(asc.x, asc.y);
            const CornerBox p = corner_decode(x[1], x[2], awh.x, awh.y, yaw_a, a.wh_swap);
            const CornerBox q = corner_decode(t[1], t[2], awh.x, awh.y, yaw_a, a.wh_swap);
            const CornerDiff d = corner_diff(x[0], t[0], p, q);
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc += sqrtf(d.x[k] * d.x[k] + d.y[k] * d.y[k]);
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

__global__ __launch_bounds__(DL_THREADS) void det_corner_loss_backward_kernel(const DetLossArgs a) {
    const float n = a.out[3];
    const float g0 = a.g_loss ? *a.g_loss : 0.f;
    const float gc = (g0 + (a.g_cls ? *a.g_cls : 0.f)) / n;
    const float gl = (g0 + (a.g_loc ? *a.g_loc : 0.f)) / n;
    const long long stride = (long long)gridDim.x * DL_THREADS;
    const long long rstep = stride % a.m;
    long long i = (long long)blockIdx.x * DL_THREADS + threadIdx.x;
    long long r = i % a.m;
    for (; i < a.n; i += stride, r = (r + rstep >= a.m ? r + rstep - a.m : r + rstep)) {
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
            const float2 *an = reinterpret_cast<const float2 *>(a.anchors) + 3 * r;
            const float2 awh = an[1], asc = an[2];
            const float yaw_a = atan2f(asc.x, asc.y);
            const float2 xwh = x[1], xsc = x[2];
            const CornerBox p = corner_decode(xwh, xsc, awh.x, awh.y, yaw_a, a.wh_swap);
            const CornerBox q = corner_decode(t[1], t[2], awh.x, awh.y, yaw_a, a.wh_swap);
            const CornerDiff d = corner_diff(x[0], t[0], p, q);
            float nx[4], ny[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float len = sqrtf(d.x[k] * d.x[k] + d.y[k] * d.y[k]);
                const float inv = len > 0.f ? 1.0f / len : 0.f;
                nx[k] = d.x[k] * inv;
                ny[k] = d.y[k] * inv;
            }
            const float GDx = (nx[0] + nx[1]) + (nx[2] + nx[3]), GDy = (ny[0] + ny[1]) + (ny[2] + ny[3]);
            const float GUx = (nx[0] - nx[1]) + (nx[3] - nx[2]), GUy = (ny[0] - ny[1]) + (ny[3] - ny[2]);
            const float GVx = (nx[0] + nx[1]) - (nx[2] + nx[3]), GVy = (ny[0] + ny[1]) - (ny[2] + ny[3]);
            const float dL = 0.5f * (GUx * p.c + GUy * p.s);
            const float dP = 0.5f * (GVy * p.c - GVx * p.s);
            const float dyaw = p.hl * (GUy * p.c - GUx * p.s) - p.hp * (GVx * p.c + GVy * p.s);
            const float dw = a.wh_swap ? dP : dL, dh = a.wh_swap ? dL : dP;
            const float r2 = xsc.x * xsc.x + xsc.y * xsc.y;
            const float ir2 = r2 > 0.f ? 1.0f / r2 : 0.f;
            dx[0] = make_float2(gl * GDx, gl * GDy);
            dx[1] = make_float2((xwh.x >= -4.0f && xwh.x <= 4.0f) ? gl * dw * p.w : 0.f, (xwh.y >= -4.0f && xwh.y <= 4.0f) ? gl * dh * p.h : 0.f);
            dx[2] = make_float2(gl * dyaw * (xsc.y * ir2), -(gl * dyaw) * (xsc.x * ir2));
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) dx[k] = make_float2(0.f, 0.f);
        }
    }
}

static int corner_args_ok(long long n_anchors, long long anchors_per_map, const char *who) {
    V2X_REQUIRE(n_anchors > 0 && anchors_per_map > 0, "%s: needs n_anchors > 0 and anchors_per_map > 0", who);
    V2X_REQUIRE(n_anchors % anchors_per_map == 0, "%s: n_anchors (%lld) is not a multiple of anchors_per_map (%lld)", who, n_anchors, anchors_per_map);
    return V2X_OK;
}

extern "C" int v2x_det_corner_loss_forward(const float *cls, const float *labels, const float *loc, const float *targets, const uint8_t *mask,
                                           const float *anchors, long long n_anchors, long long anchors_per_map, int wh_swap, float alpha,
                                           float *out4, float *workspace, v2x_stream_t stream) {
    V2X_REQUIRE(cls && labels && loc && targets && mask && anchors && out4 && workspace, "v2x_det_corner_loss_forward: null pointer");
    if (int rc = corner_args_ok(n_anchors, anchors_per_map, "v2x_det_corner_loss_forward")) return rc;
    DetLossArgs a = {};
    a.cls = cls;
    a.lab = labels;
    a.loc = loc;
    a.tgt = targets;
    a.mask = mask;
    a.n = n_anchors;
    a.alpha = alpha;
    a.part = workspace;
    a.out = out4;
    a.n_blocks = dl_blocks(n_anchors);
    a.anchors = anchors;
    a.m = anchors_per_map;
    a.wh_swap = wh_swap != 0;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(det_corner_loss_partial_kernel, dim3(a.n_blocks), dim3(DL_THREADS), 0, s, a);
    hipLaunchKernelGGL(det_loss_finish_kernel, dim3(1), dim3(DL_THREADS), 0, s, a);
    V2X_CHECK_LAUNCH("det_corner_loss_forward");
    return V2X_OK;
}

extern "C" int v2x_det_corner_loss_backward(const float *cls, const float *labels, const float *loc, const float *targets, const uint8_t *mask,
                                            const float *anchors, long long n_anchors, long long anchors_per_map, int wh_swap, float alpha,
                                            const float *out4, const float *g_loss, const float *g_cls, const float *g_loc, float *dcls, float *dloc,
                                            v2x_stream_t stream) {
    V2X_REQUIRE(cls && labels && loc && targets && mask && anchors && out4 && dcls && dloc, "v2x_det_corner_loss_backward: null pointer");
    if (int rc = corner_args_ok(n_anchors, anchors_per_map, "v2x_det_corner_loss_backward")) return rc;
    DetLossArgs a = {};
    a.cls = cls;
    a.lab = labels;
    a.loc = loc;
    a.tgt = targets;
    a.mask = mask;
    a.n = n_anchors;
    a.alpha = alpha;
    a.out = const_cast<float *>(out4);
    a.g_loss = g_loss;
    a.g_cls = g_cls;
    a.g_loc = g_loc;
    a.dcls = dcls;
    a.dloc = dloc;
    a.anchors = anchors;
    a.m = anchors_per_map;
    a.wh_swap = wh_swap != 0;
    hipLaunchKernelGGL(det_corner_loss_backward_kernel, dim3(dl_bwd_blocks(n_anchors)), dim3(DL_THREADS), 0, (hipStream_t)stream, a);
    V2X_CHECK_LAUNCH("det_corner_loss_backward_kernel");
    return V2X_OK;
}

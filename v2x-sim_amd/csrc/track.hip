// Row f-5: tracking.  SORT (Kalman constant-velocity box filter + IoU association by optimal assignment + track birth / death; upstream
// coperception/tools/track/sort.py = abewley's sort.py -- code absent from the reference tree, frozen in DESIGN.md section 3) for ALL streams of a
// step in ONE launch, and the association step alone on caller-supplied matrices (the CLEAR MOT metric uses it).
//   * one wave of 64 per stream (a workgroup = a wave: the barriers below order LDS traffic of that wave only).  lane = track for predict / update / output /
//     deaths, lane = detection for the measurement and the births, lane = COLUMN of the assignment;
//   * the IoU matrix sits in LDS as fp64 [64][64] (32 KiB), stored [small index][large index] whichever of detections / tracks is the larger set, so that
//     the lanes always walk the larger dimension (stride-1, conflict-free) and the assignment always has rows <= columns: rectangular both ways;
//   * assignment = shortest augmenting paths with potentials (Jonker-Volgenant / the O(n^3) Hungarian) in fp64: a row's column scan is one LDS read per
//     lane, the minimum a 6-step butterfly over (value, lane) -- ties go to the lowest lane, so the result is deterministic.  With IoUs that are multiples
//     of 2^-k every potential is one too and the optimum is exact;
//   * births, outputs and deaths are placed by wave ballots + prefix counts: stable order, no atomics;
//   * the filter: with SORT's F, H, Q, R the covariance never leaves the pattern "2x2 blocks (u,u'), (v,v'), (s,s') + the scalar r" (the innovation
//     covariance is diagonal), so a track is three 2-state filters and one scalar filter in fp32, Joseph-form update written out per block.
// Every loop is bounded by construction: an augmentation visits at most cols + 1 columns, there are at most `rows` augmentations, a NaN / infinite IoU is
// read as 0 and every count is clamped to its capacity -- no input can spin a wave.
#include "track_assign.h"
#include <float.h>

#define TRK_SCR 28               // words per track in the compaction scratch (17 + 5 + 4, padded)

// abewley's shortcut: every row and every column with at most one entry > thr -> those entries.  Returns the lane's row (or -1); ok is wave-uniform.
__device__ int trk_direct(const double *M, int ns, int nb, double thr, int lane, bool &ok) {
    int cnt = 0, mine = -1;
    bool bad = false;
    for (int i = 0; i < ns; ++i) {
        const bool hit = lane < nb && M[i * TRK_N + lane] > thr;
        if (__popcll(__ballot(hit)) > 1) bad = true;
        if (hit) {
            ++cnt;
            mine = i;
        }
    }
    if (__ballot(cnt > 1)) bad = true;
    ok = !bad;
    return mine;
}

// The association rule of both entry points.  M [small][large] sanitised, ns <= nb.  Returns the lane's (large index's) small index or -1.
__device__ int trk_associate(const double *M, double *u, int ns, int nb, float thr_f, int direct, int lane) {
    if (ns <= 0 || nb <= 0) return -1;
    const double thr = (double)thr_f;
    if (direct) {
        bool ok;
        const int m = trk_direct(M, ns, nb, thr, lane, ok);
        if (ok) return m;
    }
    int p = trk_assign(M, u, ns, nb, lane);
    if (p >= 0 && M[p * TRK_N + lane] < thr) p = -1;
    return p;
}

__device__ __forceinline__ float trk_finite0(float v) { return fabsf(v) <= FLT_MAX ? v : 0.0f; }   // NaN and +-inf read as 0

// abewley's iou_batch on one pair, fp32
__device__ __forceinline__ float trk_iou(const float4 d, const float4 t) {
    const float w = fmaxf(0.0f, fminf(d.z, t.z) - fmaxf(d.x, t.x));
    const float h = fmaxf(0.0f, fminf(d.w, t.w) - fmaxf(d.y, t.y));
    const float wh = w * h;
    return trk_finite0(wh / ((d.z - d.x) * (d.w - d.y) + (t.z - t.x) * (t.w - t.y) - wh));
}

__global__ __launch_bounds__(TRK_N) void assign_kernel(const float *iou, const int32_t *n_rows, const int32_t *n_cols, int cap_r, int cap_c, float thr,
                                                       int direct, int32_t *row_to_col) {
    __shared__ TrkLds L;
    const int s = blockIdx.x, lane = threadIdx.x;
    const int nr = min(max(n_rows[s], 0), cap_r), nc = min(max(n_cols[s], 0), cap_c);
    const bool tr = nr > nc;                          // lanes walk the larger dimension
    const int ns = tr ? nc : nr, nb = tr ? nr : nc;
    const float *m = iou + (size_t)s * cap_r * cap_c;
    for (int i = 0; i < ns; ++i)
        if (lane < nb) L.M[i * TRK_N + lane] = (double)trk_finite0(tr ? m[(size_t)lane * cap_c + i] : m[(size_t)i * cap_c + lane]);
    L.d2t[lane] = -1;
    __syncthreads();
    const int p = trk_associate(L.M, L.u, ns, nb, thr, direct, lane);
    if (lane < nb) {
        if (tr) L.d2t[lane] = p;
        else if (p >= 0) L.d2t[p] = lane;
    }
    __syncthreads();
    if (lane < cap_r) row_to_col[(size_t)s * cap_r + lane] = L.d2t[lane];
}

struct SortArgs {
    const float *det;
    const int32_t *det_count;
    float *trk_f;
    int32_t *trk_i, *stream_i;
    float *out_boxes;
    int32_t *out_ids, *out_det, *out_count;
    int det_cap, box_format, t_cap, max_age, min_hits, direct;
    float thr;
};

// [x1, y1, x2, y2] of the updated / predicted state
__device__ __forceinline__ float4 trk_state_box(const float *x) {
    const float w = sqrtf(x[2] * x[3]);
    const float h = x[2] / w;
    return make_float4(x[0] - w * 0.5f, x[1] - h * 0.5f, x[0] + w * 0.5f, x[1] + h * 0.5f);
}

// one (position, rate) block: predict P = F P F' + Q
__device__ __forceinline__ void trk_predict2(float *P, float qp, float qv) {
    P[0] = P[0] + (P[1] + P[1]) + P[2] + qp;
    P[1] = P[1] + P[2];
    P[2] = P[2] + qv;
}

// one (position, rate) block: measurement zm of the position with noise r, Joseph form P = (I - KH) P (I - KH)' + K R K'
__device__ __forceinline__ void trk_update2(float &xp, float &xv, float *P, float zm, float r) {
    const float a = P[0], b = P[1], c = P[2];
    const float y = zm - xp, S = a + r;
    const float k0 = a / S, k1 = b / S, g = 1.0f - k0;
    xp += k0 * y;
    xv += k1 * y;
    P[0] = g * g * a + k0 * k0 * r;
    P[1] = g * (b - k1 * a) + k0 * k1 * r;
    P[2] = (k1 * k1 * a - 2.0f * k1 * b + c) + k1 * k1 * r;
}

__global__ __launch_bounds__(TRK_N) void sort_step_kernel(const SortArgs a) {
    __shared__ TrkLds L;
    const int s = blockIdx.x, lane = threadIdx.x;
    const unsigned long long lt = trk_lt_mask(lane);
    int32_t *si = a.stream_i + (size_t)s * 4;
    int T = min(max(si[0], 0), a.t_cap);
    int next_id = si[1], status = si[3];
    const int frame = si[2] + 1;

    // ---- detections: lane = detection ---------------------------------------------------------------------------------------------------
    const int dc = a.det_count[s];
    int D = 0;
    if (dc < 0) status |= 4;
    else {
        D = min(dc, min(TRK_N, a.det_cap));
        if (dc > D) status |= 1;
    }
    float4 db = make_float4(0.f, 0.f, 0.f, 0.f), zd = db;
    if (lane < D) {
        if (a.box_format == 0) {
            db = *reinterpret_cast<const float4 *>(a.det + ((size_t)s * a.det_cap + lane) * 4);
        } else {
            const float *b = a.det + ((size_t)s * a.det_cap + lane) * 5;
            float w = b[2], h = b[3];
            if (a.box_format == 2) {
                const float t = w;
                w = h;
                h = t;
            }
            const float c = cosf(b[4]), sn = sinf(b[4]);
            float x1 = FLT_MAX, y1 = FLT_MAX, x2 = -FLT_MAX, y2 = -FLT_MAX;
#pragma unroll
            for (int k = 0; k < 4; ++k) {             // utils/postprocess.py::box_corners, then standup
                const float dx = (k == 0 || k == 3) ? w * 0.5f : -w * 0.5f, dy = k < 2 ? h * 0.5f : -h * 0.5f;
                const float cx = b[0] + dx * c - dy * sn, cy = b[1] + dx * sn + dy * c;
                x1 = fminf(x1, cx);
                y1 = fminf(y1, cy);
                x2 = fmaxf(x2, cx);
                y2 = fmaxf(y2, cy);
            }
            db = make_float4(x1, y1, x2, y2);
        }
        const float w = db.z - db.x, h = db.w - db.y;
        zd = make_float4(db.x + w * 0.5f, db.y + h * 0.5f, w * h, w / h);
    }
    L.dbox[lane] = db;
    L.z[lane] = zd;

    // ---- predict: lane = track ----------------------------------------------------------------------------------------------------------
    float x[7], P[10];
    int32_t ti[5];
#pragma unroll
    for (int k = 0; k < 7; ++k) x[k] = 0.f;
#pragma unroll
    for (int k = 0; k < 10; ++k) P[k] = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) ti[k] = 0;
    float *tf = a.trk_f + (size_t)s * a.t_cap * 17;
    int32_t *tg = a.trk_i + (size_t)s * a.t_cap * 5;
    float4 pb = make_float4(0.f, 0.f, 0.f, 0.f);
    bool live = lane < T;
    if (live) {
#pragma unroll
        for (int k = 0; k < 7; ++k) x[k] = tf[lane * 17 + k];
#pragma unroll
        for (int k = 0; k < 10; ++k) P[k] = tf[lane * 17 + 7 + k];
#pragma unroll
        for (int k = 0; k < 5; ++k) ti[k] = tg[lane * 5 + k];
        if (x[6] + x[2] <= 0.f) x[6] = 0.f;
        x[0] += x[4];
        x[1] += x[5];
        x[2] += x[6];
        trk_predict2(P + 0, 1.0f, 0.01f);
        trk_predict2(P + 3, 1.0f, 0.01f);
        trk_predict2(P + 6, 1.0f, 1.0e-4f);
        P[9] += 1.0f;
        ti[4] += 1;
        if (ti[1] > 0) ti[3] = 0;
        ti[1] += 1;
        pb = trk_state_box(x);
    }
    const bool valid = live && fabsf(pb.x) <= FLT_MAX && fabsf(pb.y) <= FLT_MAX && fabsf(pb.z) <= FLT_MAX && fabsf(pb.w) <= FLT_MAX;
    const unsigned long long vb = __ballot(valid);
    if (__popcll(vb) != T) {                          // wave-uniform: a track with a non-finite predicted box leaves; stable compaction through LDS
        float *scr = reinterpret_cast<float *>(L.M);
        const int pos = __popcll(vb & lt);
        if (valid) {
            float *q = scr + pos * TRK_SCR;
#pragma unroll
            for (int k = 0; k < 7; ++k) q[k] = x[k];
#pragma unroll
            for (int k = 0; k < 10; ++k) q[7 + k] = P[k];
#pragma unroll
            for (int k = 0; k < 5; ++k) q[17 + k] = __int_as_float(ti[k]);
            q[22] = pb.x, q[23] = pb.y, q[24] = pb.z, q[25] = pb.w;
        }
        __syncthreads();
        T = __popcll(vb);
        live = lane < T;
        if (live) {
            const float *q = scr + lane * TRK_SCR;
#pragma unroll
            for (int k = 0; k < 7; ++k) x[k] = q[k];
#pragma unroll
            for (int k = 0; k < 10; ++k) P[k] = q[7 + k];
#pragma unroll
            for (int k = 0; k < 5; ++k) ti[k] = __float_as_int(q[17 + k]);
            pb = make_float4(q[22], q[23], q[24], q[25]);
        }
        __syncthreads();
    }
    L.pbox[lane] = pb;
    L.d2t[lane] = -1;
    L.t2d[lane] = -1;
    __syncthreads();

    // ---- associate: lane = the larger of (detections, tracks) ----------------------------------------------------------------------------
    const bool tr = D > T;
    const int ns = tr ? T : D, nb = tr ? D : T;
    for (int i = 0; i < ns; ++i)
        if (lane < nb) L.M[i * TRK_N + lane] = (double)(tr ? trk_iou(db, L.pbox[i]) : trk_iou(L.dbox[i], pb));
    __syncthreads();
    const int p = trk_associate(L.M, L.u, ns, nb, a.thr, a.direct, lane);
    if (lane < nb) {
        if (tr) {
            L.d2t[lane] = p;
            if (p >= 0) L.t2d[p] = lane;
        } else {
            L.t2d[lane] = p;
            if (p >= 0) L.d2t[p] = lane;
        }
    }
    __syncthreads();

    // ---- update the matched tracks: lane = track -----------------------------------------------------------------------------------------
    int mdet = live ? L.t2d[lane] : -1;
    if (mdet >= 0) {
        const float4 zm = L.z[mdet];
        ti[1] = 0;
        ti[2] += 1;
        ti[3] += 1;
        trk_update2(x[0], x[4], P + 0, zm.x, 1.0f);
        trk_update2(x[1], x[5], P + 3, zm.y, 1.0f);
        trk_update2(x[2], x[6], P + 6, zm.z, 10.0f);
        const float pr = P[9], k = pr / (pr + 10.0f), g = 1.0f - k;
        x[3] += k * (zm.w - x[3]);
        P[9] = g * g * pr + k * k * 10.0f;
    }

    // ---- births: lane = detection -> the slots behind the live tracks, in detection order -------------------------------------------------
    const bool unmatched = lane < D && L.d2t[lane] < 0;
    const unsigned long long ub = __ballot(unmatched);
    const int n_unm = __popcll(ub), kept = min(n_unm, a.t_cap - T);
    if (n_unm > kept) status |= 2;
    const int rank = __popcll(ub & lt);
    if (unmatched && rank < kept) L.birth[rank] = lane;
    __syncthreads();
    if (lane >= T && lane < T + kept) {
        mdet = L.birth[lane - T];
        const float4 zm = L.z[mdet];
        x[0] = zm.x, x[1] = zm.y, x[2] = zm.z, x[3] = zm.w, x[4] = x[5] = x[6] = 0.f;
        P[0] = P[3] = P[6] = P[9] = 10.f;
        P[2] = P[5] = P[8] = 1.0e4f;
        P[1] = P[4] = P[7] = 0.f;
        ti[0] = next_id + (lane - T) + 1;
        ti[1] = ti[2] = ti[3] = ti[4] = 0;
    }
    next_id += kept;
    T += kept;
    live = lane < T;

    // ---- output (ascending id = storage order), then deaths ------------------------------------------------------------------------------
    const bool rep = live && ti[1] == 0 && (ti[3] >= a.min_hits || frame <= a.min_hits);
    const unsigned long long rb = __ballot(rep);
    if (rep) {
        const size_t o = (size_t)s * a.t_cap + __popcll(rb & lt);
        *reinterpret_cast<float4 *>(a.out_boxes + o * 4) = trk_state_box(x);
        a.out_ids[o] = ti[0];
        a.out_det[o] = mdet;
    }
    const bool keep = live && ti[1] <= a.max_age;
    const unsigned long long kb = __ballot(keep);
    if (keep) {                                       // every lane's track is in registers: the in-place compaction has no hazard
        const int pos = __popcll(kb & lt);
#pragma unroll
        for (int k = 0; k < 7; ++k) tf[pos * 17 + k] = x[k];
#pragma unroll
        for (int k = 0; k < 10; ++k) tf[pos * 17 + 7 + k] = P[k];
#pragma unroll
        for (int k = 0; k < 5; ++k) tg[pos * 5 + k] = ti[k];
    }
    if (lane == 0) {
        si[0] = __popcll(kb);
        si[1] = next_id;
        si[2] = frame;
        si[3] = status;
        a.out_count[s] = __popcll(rb);
    }
}

extern "C" int v2x_assign_iou(const float *iou, const int32_t *n_rows, const int32_t *n_cols, int n, int cap_r, int cap_c, float thr, int direct,
                              int32_t *row_to_col, v2x_stream_t stream) {
    V2X_REQUIRE(iou && n_rows && n_cols && row_to_col, "v2x_assign_iou: null pointer");
    V2X_REQUIRE(n >= 0, "v2x_assign_iou: n = %d", n);
    V2X_REQUIRE(cap_r >= 1 && cap_r <= TRK_N && cap_c >= 1 && cap_c <= TRK_N, "v2x_assign_iou: cap_r = %d, cap_c = %d outside [1, 64] (one wave per matrix)", cap_r,
                cap_c);
    if (n == 0) return V2X_OK;
    hipLaunchKernelGGL(assign_kernel, dim3(n), dim3(TRK_N), 0, reinterpret_cast<hipStream_t>(stream), iou, n_rows, n_cols, cap_r, cap_c, thr, direct, row_to_col);
    V2X_CHECK_LAUNCH("assign_kernel");
    return V2X_OK;
}

extern "C" int v2x_sort_step(const float *det_boxes, const int32_t *det_count, int n, int det_cap, int box_format, float *trk_f, int32_t *trk_i,
                             int32_t *stream_i, int t_cap, float iou_thr, int max_age, int min_hits, int direct, float *out_boxes, int32_t *out_ids,
                             int32_t *out_det, int32_t *out_count, v2x_stream_t stream) {
    V2X_REQUIRE(det_boxes && det_count && trk_f && trk_i && stream_i && out_boxes && out_ids && out_det && out_count, "v2x_sort_step: null pointer");
    V2X_REQUIRE(n >= 0 && det_cap >= 1, "v2x_sort_step: n = %d, det_cap = %d", n, det_cap);
    V2X_REQUIRE(box_format >= 0 && box_format <= 2, "v2x_sort_step: box_format = %d (0: xyxy, 1 / 2: x, y, w, h, yaw with w / h along the heading)", box_format);
    V2X_REQUIRE(t_cap >= 1 && t_cap <= TRK_N, "v2x_sort_step: t_cap = %d outside [1, 64] (one wave per stream)", t_cap);
    V2X_REQUIRE(max_age >= 0 && min_hits >= 0, "v2x_sort_step: max_age = %d, min_hits = %d must not be negative", max_age, min_hits);
    V2X_REQUIRE(box_format != 0 || (reinterpret_cast<uintptr_t>(det_boxes) & 15) == 0, "v2x_sort_step: xyxy det_boxes must be 16-byte aligned");
    V2X_REQUIRE((reinterpret_cast<uintptr_t>(out_boxes) & 15) == 0, "v2x_sort_step: out_boxes must be 16-byte aligned");
    if (n == 0) return V2X_OK;
    const SortArgs a = {det_boxes, det_count, trk_f, trk_i, stream_i, out_boxes, out_ids, out_det, out_count, det_cap, box_format, t_cap, max_age, min_hits,
                        direct, iou_thr};
    hipLaunchKernelGGL(sort_step_kernel, dim3(n), dim3(TRK_N), 0, reinterpret_cast<hipStream_t>(stream), a);
    V2X_CHECK_LAUNCH("sort_step_kernel");
    return V2X_OK;
}

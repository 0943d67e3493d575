// f-1 -- the detection metric of a whole split in one call: mmdet "area" AP per agent (group) and IoU threshold, from the NMS'd boxes that
// v2x_det_postprocess left on the device.  Replaces utils/postprocess.py::eval_map (a Python loop over every detection of every map with
// polygon clipping on the host, once per agent and threshold) and the host half of eval_map_device (the sort and the cumulative sums).
// The frozen rule is DESIGN.md section 3.11.
//
// Four launches, no atomics, no allocation, no host synchronisation (capturable); cross-workgroup order comes from the kernel boundaries only:
//   1. det_map_match_kernel   grid n_img            one workgroup per map walks its detections in score order (match_detections_kernel's walk).
//                                                   The ground truth a detection takes (det_match.h) does not depend on the threshold: ONE search
//                                                   per detection, then one "taken" bit per ground truth AND threshold (a byte per ground truth in
//                                                   LDS: 8192 x 8 bits = 8 KiB).  The n_thr flags of a detection leave as one byte.
//   2. det_map_count_kernel   grid n_groups         ground truths and detections per group (integer sums: any order gives the same bits).
//   3. det_map_rank_kernel    grid n_img            every map's list is sorted already, so the position of a detection in its group's ranked list
//                                                   is a sum of binary searches, one per map of the group: entries >= its score in the maps before
//                                                   its own, its position in its own, entries > its score in the maps after.  That is numpy's
//                                                   stable argsort(-scores) over the image-major concatenation -- exact, no scatter passes, no
//                                                   arrival order.  Scores compare as fp32 VALUES (-0.0 == +0.0).  The flag byte is scattered to
//                                                   its rank: one contiguous ranked list per group.  COST: every workgroup walks ALL n_img maps
//                                                   and filters by group (scalar loads), and searches each map of its group: n_img^2 scalar
//                                                   steps whatever n_groups is, and (detections x maps per group) searches -- quadratic in the
//                                                   maps per group (5.6 ms at 5 000 maps, 161 ms at 50 000: profiles/det_map_bench.txt).  A
//                                                   per-group list of map indices from the count kernel (4 B per map of workspace) would remove
//                                                   the filter's share; a stable radix sort the rest.  Neither is built.
//   4. det_map_ap_kernel      grid (n_groups, n_thr) one workgroup walks its ranked list BACKWARDS in chunks of DET_MAP_CHUNK: with the number of true
//                                                   positives known (a counting pass), the cumulative count at a position is the count at the
//                                                   chunk's end minus a suffix, so one walk yields precision, its suffix maximum (the envelope)
//                                                   and the area sum, in a fixed order -- float64, bit-reproducible.
#include "common.h"
#include "det_match.h"

constexpr int DET_MAP_MAX_THR = 8;
constexpr int DET_MAP_MAX_GROUPS = 64;
constexpr int DET_MAP_ITEMS = 4;                                    // consecutive list positions per thread of the AP walk
constexpr int DET_MAP_CHUNK = DET_MATCH_THREADS * DET_MAP_ITEMS;    // 1024 positions per step of the AP walk

struct det_map_args {
    const float *det_boxes, *det_scores, *gt_boxes, *iou_thr;
    const int32_t *det_count, *gt_count, *group;
    int det_cap, gt_cap, n_groups, n_thr;
    long long n_img;
    double *ap;
    long long *num_gt, *num_det, *num_tp;
    uint8_t *tp;          // optional
    int32_t *rank;        // optional
    uint8_t *flags;       // workspace [n_img][det_cap]: bit t = true positive at threshold t
    uint8_t *ranked;      // workspace [n_img * det_cap]: the flag bytes in ranked order, group after group
};

__device__ __forceinline__ int det_map_group_of(const det_map_args &p, long long img) {
    const int g = p.group[img];
    return g >= 0 && g < p.n_groups ? g : -1;
}

__global__ __launch_bounds__(DET_MATCH_THREADS) void det_map_match_kernel(const det_map_args p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint8_t *taken = reinterpret_cast<uint8_t *>(smem);        // [gt_cap]: bit t = taken at threshold t
    __shared__ double s_best[DET_MATCH_THREADS];
    __shared__ int s_arg[DET_MATCH_THREADS];
    const long long img = blockIdx.x;
    const int tid = threadIdx.x;
    const int nd = det_clamp_count(p.det_count[img], p.det_cap), ng = det_clamp_count(p.gt_count[img], p.gt_cap);
    double thr[DET_MAP_MAX_THR];
#pragma unroll
    for (int t = 0; t < DET_MAP_MAX_THR; ++t) thr[t] = t < p.n_thr ? (double)p.iou_thr[t] : 2.0;
    for (int g = tid; g < ng; g += DET_MATCH_THREADS) taken[g] = 0;
    __syncthreads();
    uint8_t *flags = p.flags + (size_t)img * p.det_cap;
    for (int j = 0; j < nd; ++j) {
        det_best_gt(p.det_boxes + ((size_t)img * p.det_cap + j) * 5, p.gt_boxes + (size_t)img * p.gt_cap * 5, ng, tid, s_best, s_arg);
        if (tid == 0) {
            const int a0 = s_arg[0];
            unsigned bits = 0;
            if (a0 >= 0) {
                const double best = s_best[0];
                const unsigned was = taken[a0];
#pragma unroll
                for (int t = 0; t < DET_MAP_MAX_THR; ++t)
                    if (best >= thr[t] && !((was >> t) & 1u)) bits |= 1u << t;       // unused thresholds are 2.0: never reached
                taken[a0] = (uint8_t)(was | bits);
            }
            flags[j] = (uint8_t)bits;
        }
        __syncthreads();
    }
    // (the last barrier of the walk orders thread 0's global stores before these reads: workgroup scope)
    for (int j = tid; j < p.det_cap; j += DET_MATCH_THREADS) {
        const unsigned bits = j < nd ? flags[j] : 0u;
        if (j >= nd) flags[j] = 0;
        if (p.tp)
            for (int t = 0; t < p.n_thr; ++t) p.tp[((size_t)t * p.n_img + img) * p.det_cap + j] = (uint8_t)((bits >> t) & 1u);
    }
}

__global__ __launch_bounds__(DET_MATCH_THREADS) void det_map_count_kernel(const det_map_args p) {
    __shared__ long long s_gt[DET_MATCH_THREADS], s_det[DET_MATCH_THREADS];
    const int g = blockIdx.x, tid = threadIdx.x;
    long long ngt = 0, ndet = 0;
    for (long long img = tid; img < p.n_img; img += DET_MATCH_THREADS) {
        if (det_map_group_of(p, img) != g) continue;
        ngt += det_clamp_count(p.gt_count[img], p.gt_cap);
        ndet += det_clamp_count(p.det_count[img], p.det_cap);
    }
    s_gt[tid] = ngt;
    s_det[tid] = ndet;
    __syncthreads();
    for (int st = DET_MATCH_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) {
            s_gt[tid] += s_gt[tid + st];
            s_det[tid] += s_det[tid + st];
        }
        __syncthreads();
    }
    if (tid == 0) {
        p.num_gt[g] = s_gt[0];
        p.num_det[g] = s_det[0];
    }
}

// entries of the descending list s[0, n) that are > x (STRICT) or >= x
template <bool STRICT>
__device__ __forceinline__ int det_map_count_before(const float *__restrict__ s, int n, float x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const float v = s[mid];
        if (STRICT ? v > x : v >= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(64) void det_map_rank_kernel(const det_map_args p) {
    const long long img = blockIdx.x;
    const int tid = threadIdx.x;
    const int g = det_map_group_of(p, img);
    const int nd = g < 0 ? 0 : det_clamp_count(p.det_count[img], p.det_cap);
    if (p.rank)
        for (int j = nd + tid; j < p.det_cap; j += 64) p.rank[(size_t)img * p.det_cap + j] = -1;
    if (nd == 0) return;
    long long base = 0;                        // where the group's ranked list starts: the groups before it, in order
    for (int k = 0; k < g; ++k) base += p.num_det[k];
    for (int j0 = 0; j0 < nd; j0 += 64) {
        const int j = j0 + tid;
        const bool live = j < nd;
        const float x = live ? p.det_scores[(size_t)img * p.det_cap + j] : 0.0f;
        int r = live ? j : 0;
        for (long long m = 0; m < p.n_img; ++m) {          // wave-uniform: the group and the count of map m are scalar loads
            if (m == img || det_map_group_of(p, m) != g) continue;
            const int nm = det_clamp_count(p.det_count[m], p.det_cap);
            if (nm == 0 || !live) continue;
            const float *s = p.det_scores + (size_t)m * p.det_cap;
            r += m < img ? det_map_count_before<false>(s, nm, x) : det_map_count_before<true>(s, nm, x);
        }
        if (live) {
            // r < the group's num_det: every term is at most its map's count and the own term is j < nd
            if (p.rank) p.rank[(size_t)img * p.det_cap + j] = r;
            p.ranked[base + r] = p.flags[(size_t)img * p.det_cap + j];
        }
    }
}

__global__ __launch_bounds__(DET_MATCH_THREADS) void det_map_ap_kernel(const det_map_args p) {
    __shared__ long long s_cnt[DET_MATCH_THREADS];
    __shared__ int s_wsum[4];
    __shared__ double s_max[DET_MATCH_THREADS + 1];
    __shared__ double s_wmax[4], s_warea[4];
    const int g = blockIdx.x, t = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n = p.num_det[g], G = p.num_gt[g];
    long long base = 0;
    for (int k = 0; k < g; ++k) base += p.num_det[k];
    const uint8_t *list = p.ranked + base;
    // the number of true positives: the cumulative count at the list's end
    long long c = 0;
    for (long long i = tid; i < n; i += DET_MATCH_THREADS) c += (list[i] >> t) & 1;
    s_cnt[tid] = c;
    __syncthreads();
    for (int st = DET_MATCH_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) s_cnt[tid] += s_cnt[tid + st];
        __syncthreads();
    }
    const long long total_tp = s_cnt[0];
    if (tid == 0) p.num_tp[(size_t)g * p.n_thr + t] = total_tp;
    if (G == 0 || n == 0 || total_tp == 0) {       // no true positive: every term of the area sum is absent
        if (tid == 0) p.ap[(size_t)g * p.n_thr + t] = 0.0;
        return;
    }
    const double dG = (double)G;
    long long tp_end = total_tp;                   // cumulative true positives at the end of the current chunk
    double env_next = 0.0;                         // suffix maximum of the precision over everything after the current chunk
    double area = 0.0;                             // thread 0's: the chunks' sums, last chunk first
    const long long n_chunks = (n + DET_MAP_CHUNK - 1) / DET_MAP_CHUNK;
    for (long long ch = n_chunks - 1; ch >= 0; --ch) {
        const long long i0 = ch * DET_MAP_CHUNK + (long long)tid * DET_MAP_ITEMS;
        int f[DET_MAP_ITEMS], incl[DET_MAP_ITEMS];
        int mine = 0;
#pragma unroll
        for (int e = 0; e < DET_MAP_ITEMS; ++e) {
            f[e] = i0 + e < n ? (list[i0 + e] >> t) & 1 : 0;
            mine += f[e];
            incl[e] = mine;
        }
        // inclusive scan of the threads' counts: within the wave by shuffles, across the four waves through LDS
        int scan = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(scan, off);
            if (lane >= off) scan += o;
        }
        if (lane == 63) s_wsum[wave] = scan;
        __syncthreads();
        int before = 0, chunk_tp = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += s_wsum[w];
            chunk_tp += s_wsum[w];
        }
        const long long tp_first = tp_end - chunk_tp + before + scan - mine;      // cumulative count BEFORE this thread's first position
        double prec[DET_MAP_ITEMS];
        double pmax = 0.0;
#pragma unroll
        for (int e = 0; e < DET_MAP_ITEMS; ++e) {
            // precision = tp / (tp + fp) = tp / (position + 1); positions past the list's end: 0, neutral under the maximum
            prec[e] = i0 + e < n ? (double)(tp_first + incl[e]) / (double)(i0 + e + 1) : 0.0;
            pmax = fmax(pmax, prec[e]);
        }
        // inclusive suffix maximum over the threads
        double smax = pmax;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double o = __shfl_down(smax, off);
            if (lane + off < 64) smax = fmax(smax, o);
        }
        if (lane == 0) s_wmax[wave] = smax;
        __syncthreads();
        double later = env_next;
#pragma unroll
        for (int w = 3; w >= 0; --w)
            if (w > wave) later = fmax(later, s_wmax[w]);
        s_max[tid] = fmax(smax, later);
        if (tid == 0) s_max[DET_MATCH_THREADS] = env_next;
        __syncthreads();
        double env = s_max[tid + 1];               // the envelope just after this thread's last position
        double term = 0.0;
#pragma unroll
        for (int e = DET_MAP_ITEMS - 1; e >= 0; --e) {
            env = fmax(env, prec[e]);
            if (f[e]) {
                const long long k = tp_first + incl[e];
                term += ((double)k / dG - (double)(k - 1) / dG) * env;      // recall's step times the envelope
            }
        }
        env_next = s_max[0];
        tp_end -= chunk_tp;
        // the chunk's sum in a fixed order: butterfly within the wave, then the four waves in order
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) term += __shfl_xor(term, off);
        if (lane == 0) s_warea[wave] = term;
        __syncthreads();
        if (tid == 0) area += ((s_warea[3] + s_warea[2]) + s_warea[1]) + s_warea[0];
        // (the next chunk's first LDS write, s_wsum, is read only after ITS barrier; s_max / s_warea are rewritten two barriers from here)
    }
    if (tid == 0) p.ap[(size_t)g * p.n_thr + t] = area;
}

static bool det_map_dims_ok(long long n_img, int det_cap, int gt_cap, int n_groups, int n_thr) {
    return n_img >= 0 && n_img < (1LL << 31) && det_cap >= 1 && det_cap <= DET_MAX_CAP && gt_cap >= 1 && gt_cap <= DET_MATCH_MAX_GT && n_groups >= 1 &&
           n_groups <= DET_MAP_MAX_GROUPS && n_thr >= 1 && n_thr <= DET_MAP_MAX_THR && n_img * det_cap < (1LL << 31);
}

extern "C" long long v2x_det_map_workspace_size(long long n_img, int det_cap, int gt_cap, int n_groups, int n_thr) {
    if (!det_map_dims_ok(n_img, det_cap, gt_cap, n_groups, n_thr)) return -1;
    return 2 * n_img * det_cap;       // the flag bytes in map order and in ranked order
}

extern "C" int v2x_det_map(const float *det_boxes, const float *det_scores, const int32_t *det_count, int det_cap, const float *gt_boxes,
                           const int32_t *gt_count, int gt_cap, const int32_t *group, long long n_img, int n_groups, const float *iou_thr, int n_thr,
                           double *ap, long long *num_gt, long long *num_det, long long *num_tp, uint8_t *tp, int32_t *rank, void *workspace,
                           long long workspace_bytes, v2x_stream_t stream) {
    if (n_img == 0) return V2X_OK;
    V2X_REQUIRE(det_map_dims_ok(n_img, det_cap, gt_cap, n_groups, n_thr),
                "v2x_det_map: n_img=%lld, det_cap=%d (1..%d), gt_cap=%d (1..%d), n_groups=%d (1..%d), n_thr=%d (1..%d); n_img*det_cap < 2^31", n_img, det_cap,
                DET_MAX_CAP, gt_cap, DET_MATCH_MAX_GT, n_groups, DET_MAP_MAX_GROUPS, n_thr, DET_MAP_MAX_THR);
    V2X_REQUIRE(det_boxes && det_scores && det_count && gt_boxes && gt_count && group && iou_thr && ap && num_gt && num_det && num_tp,
                "v2x_det_map: null pointer (only tp and rank may be null)");
    const long long need = v2x_det_map_workspace_size(n_img, det_cap, gt_cap, n_groups, n_thr);
    V2X_REQUIRE(workspace && workspace_bytes >= need, "v2x_det_map: workspace of %lld bytes, %lld needed", workspace ? workspace_bytes : 0LL, need);
    V2X_REQUIRE((reinterpret_cast<uintptr_t>(ap) & 7) == 0 && (reinterpret_cast<uintptr_t>(num_gt) & 7) == 0 && (reinterpret_cast<uintptr_t>(num_det) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(num_tp) & 7) == 0 && (reinterpret_cast<uintptr_t>(rank) & 3) == 0,
                "v2x_det_map: ap, num_gt, num_det, num_tp must be 8-byte and rank 4-byte aligned");
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    const det_map_args p = {det_boxes, det_scores, gt_boxes, iou_thr, det_count, gt_count, group, det_cap, gt_cap, n_groups, n_thr, n_img,
                            ap, num_gt, num_det, num_tp, tp, rank, ws, ws + n_img * det_cap};
    hipStream_t s = (hipStream_t)stream;
    int rc = v2x_launch<det_map_match_kernel, 0>("det_map_match_kernel", dim3((unsigned)n_img), dim3(DET_MATCH_THREADS), (gt_cap + 15) & ~15, s, p);
    if (rc != V2X_OK) return rc;
    rc = v2x_launch<det_map_count_kernel, 0>("det_map_count_kernel", dim3(n_groups), dim3(DET_MATCH_THREADS), 0, s, p);
    if (rc != V2X_OK) return rc;
    rc = v2x_launch<det_map_rank_kernel, 0>("det_map_rank_kernel", dim3((unsigned)n_img), dim3(64), 0, s, p);
    if (rc != V2X_OK) return rc;
    return v2x_launch<det_map_ap_kernel, 0>("det_map_ap_kernel", dim3(n_groups, n_thr), dim3(DET_MATCH_THREADS), 0, s, p);
}

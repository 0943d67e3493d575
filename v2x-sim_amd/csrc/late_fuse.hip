// f-1 -- late fusion (the V2X-Sim table's "Co-lower-bound", upstream test_codet.py --com late): every agent detects on its own sweep, the
// agents exchange BOXES, and each ego suppresses the union of its own detections and its neighbours', moved into its frame.
//
// On the host this is a Python loop over the egos with a numpy NMS each (utils/postprocess.late_fusion) behind a detector that needs 0.5 ms per
// frame.  Here: one 256-thread workgroup per ego (agent i of frame b, row i*B + b of the agent-major batch), all egos of a call in one launch.
// Build-owned spec: DESIGN.md section 3 ("late fusion").
//   gather    the ego's detections as they are; for every j != i with link[b][i][j] the detections of row j*B + b, moved by rigid[b][i][j]
//             = (r00, r01, tx, r10, r11, ty, dyaw, 0) in fp32 with separately rounded products and sums:
//                 x' = (r00*x + r01*y) + tx,  y' = (r10*x + r11*y) + ty,  yaw' = yaw + dyaw,
//             kept iff x_lo <= x' < x_hi and y_lo <= y' < y_hi.  A candidate with a non-finite field or a score that is not >= 0 is dropped.
//   sort      bitonic in LDS on the key (~score bits << 32 | tie), tie = (0 for the ego, j + 1 for neighbour j) * cap_in + rank in the
//             source list: score descending, then the ego's own boxes, then neighbours by agent index, then by rank.  The key is unique, so
//             the LDS slot a candidate was gathered into (an atomic counter) never reaches the output.
//   suppress  det_nms_kernel's arithmetic (det_geom.h) in det_nms_kernel's two forms: the bit matrix for at most NMS_FAST_CAP (512) merged
//             candidates -- the normal case: 46 KiB of LDS, three workgroups per CU --, the serial scan with 28 bytes of LDS per candidate
//             (112 KiB at cap_out = 4096) for the egos the first launch marked NMS_PENDING; that launch returns at once for every other ego.
//   compact   kept boxes, scores (the source's bits), source = j*cap_in + rank, count.
#include "common.h"
#include "det_geom.h"

struct late_args {
    const float *boxes;        // [A*B][cap_in][5]
    const float *scores;       // [A*B][cap_in]
    const int32_t *counts;     // [A*B]
    const float *rigid;        // [B][A][A][8]
    const uint8_t *link;       // [B][A][A]
    int A, B, cap_in, cap_out;
    float x_lo, x_hi, y_lo, y_hi, nms_thr;
};

__device__ __forceinline__ bool late_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
// A value the optimiser cannot look through: the product that went in is a finished, rounded fp32 (no instruction is emitted).
__device__ __forceinline__ float late_rounded(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

// Candidate `rank` of agent j as ego i of frame b sees it: false = dropped.  Evaluated twice per candidate (gather: the key; after the sort:
// the box) -- 8 flops against an LDS record of 20 more bytes per candidate.
__device__ __forceinline__ bool late_candidate(const late_args &p, int i, int j, int b, int rank, float (&box)[5], float &score) {
    const size_t row = (size_t)j * p.B + b;
    const float *s = p.boxes + (row * p.cap_in + rank) * 5;
    score = p.scores[row * p.cap_in + rank];
    const float x = s[0], y = s[1];
    box[2] = s[2];
    box[3] = s[3];
    if (j == i) {   // the ego's own: bit for bit, never cropped
        box[0] = x;
        box[1] = y;
        box[4] = s[4];
    } else {
        // Every product and sum rounded on its own, as numpy's float32 operations are.  __fmul_rn / __fadd_rn name the intent, but they are plain
        // `*` and `+` to the compiler, and under hipcc's default -ffp-contract=fast the BACKEND fuses them whatever the source says (measured: y' =
        // fma(r10, x, r11*y), one ulp off; `#pragma clang fp contract(off)` did not change it).  late_rounded makes each product opaque.
        const float *r = p.rigid + (((size_t)b * p.A + i) * p.A + j) * 8;
        box[0] = __fadd_rn(__fadd_rn(late_rounded(__fmul_rn(r[0], x)), late_rounded(__fmul_rn(r[1], y))), r[2]);
        box[1] = __fadd_rn(__fadd_rn(late_rounded(__fmul_rn(r[3], x)), late_rounded(__fmul_rn(r[4], y))), r[5]);
        box[4] = __fadd_rn(s[4], r[6]);
        if (!(box[0] >= p.x_lo && box[0] < p.x_hi && box[1] >= p.y_lo && box[1] < p.y_hi)) return false;
    }
    // finite fields (the source's x, y too: an ego box is not transformed), a score >= 0 (NaN fails both)
    return late_finite(x) && late_finite(y) && late_finite(s[4]) && late_finite(box[0]) && late_finite(box[1]) && late_finite(box[2]) && late_finite(box[3]) &&
           late_finite(box[4]) && late_finite(score) && score >= 0.0f;
}

template <bool ROTATED, bool FAST>
__global__ __launch_bounds__(256) void late_fuse_kernel(late_args p, float *__restrict__ out_boxes, float *__restrict__ out_scores,
                                                        int32_t *__restrict__ out_src, int32_t *__restrict__ out_count, int lcap,
                                                        int pending_only) {
    // lcap = candidates this launch's LDS holds (FAST: NMS_FAST_CAP, else cap_out); the layout is det_nms_kernel's
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long *skey = reinterpret_cast<unsigned long long *>(smem);          // [lcap]
    float4 *sbox = reinterpret_cast<float4 *>(smem + (size_t)lcap * 8);                 // [lcap] stand-up x1,y1,x2,y2
    int *skept = reinterpret_cast<int *>(smem + (size_t)lcap * 24);                     // [lcap] sorted positions kept
    unsigned long long *smask = reinterpret_cast<unsigned long long *>(smem + (size_t)lcap * 28);   // FAST: [lcap][lcap / 64]
    __shared__ int s_nkept, s_cnt, s_bad;

    const int ego = blockIdx.x, tid = threadIdx.x;
    const int A = p.A, B = p.B, cap_in = p.cap_in, cap_out = p.cap_out;
    const int i = ego / B, b = ego - i * B;
    if (pending_only && out_count[ego] != NMS_PENDING) return;
    const uint8_t *lk = p.link + ((size_t)b * A + i) * A;
    if (lk[i] == 0) {           // the ego itself is absent
        if (tid == 0) out_count[ego] = 0;
        return;
    }
    if (tid == 0) {
        s_cnt = 0;
        s_nkept = 0;
        s_bad = 0;
    }
    __syncthreads();
    // a linked source (the ego included) without a result of its own: the post-processor's negative count
    for (int j = tid; j < A; j += 256)
        if ((j == i || lk[j] != 0) && p.counts[(size_t)j * B + b] < 0) s_bad = 1;
    __syncthreads();
    if (s_bad) {
        if (tid == 0) out_count[ego] = -(cap_out + 1);
        return;
    }
    // gather: slot = an LDS counter (any order -- the sort key is unique); the count runs on past lcap, the keys do not
    for (int j = 0; j < A; ++j) {
        if (j != i && lk[j] == 0) continue;
        int cj = p.counts[(size_t)j * B + b];
        cj = cj > cap_in ? cap_in : cj;
        const unsigned tie0 = (j == i ? 0u : (unsigned)(j + 1)) * (unsigned)cap_in;
        for (int r = tid; r < cj; r += 256) {
            float box[5], score;
            if (!late_candidate(p, i, j, b, r, box, score)) continue;
            const int pos = atomicAdd(&s_cnt, 1);
            // -0.0f == 0.0f: one key for both, so that the order is the comparison's (the OUTPUT score is read from the source)
            const unsigned sbits = score == 0.0f ? 0u : __float_as_uint(score);
            if (pos < lcap) skey[pos] = ((unsigned long long)(~sbits) << 32) | (tie0 + (unsigned)r);
        }
    }
    __syncthreads();
    const int cnt = s_cnt;
    if (cnt > cap_out) {        // overflow: report -count, the caller decides (host path / larger cap_out)
        if (tid == 0) out_count[ego] = -cnt;
        return;
    }
    if (FAST && cnt > lcap) {   // more candidates than the fast form holds: the second launch takes this ego
        if (tid == 0) out_count[ego] = NMS_PENDING;
        return;
    }
    int np2 = 1;
    while (np2 < cnt) np2 <<= 1;
    for (int q = cnt + tid; q < np2; q += 256) skey[q] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= np2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int q = tid; q < np2; q += 256) {
                const int l = q ^ j;
                if (l > q) {
                    const unsigned long long a = skey[q], c = skey[l];
                    const bool up = (q & k) == 0;
                    if ((a > c) == up) {
                        skey[q] = c;
                        skey[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    // the sorted candidates again: stand-up boxes to LDS, (x, y, w, h, yaw) to the output staging area (global, sorted order; compacted below)
    float *stage = out_boxes + (size_t)ego * cap_out * 5;
    for (int q = tid; q < cnt; q += 256) {
        const unsigned tie = (unsigned)(skey[q] & 0xffffffffu);
        const int g = (int)(tie / (unsigned)cap_in), r = (int)(tie - (unsigned)g * (unsigned)cap_in);
        float box[5], score;
        (void)late_candidate(p, i, g == 0 ? i : g - 1, b, r, box, score);
        sbox[q] = det_standup_box(box[0], box[1], box[2], box[3], box[4]);
        float *o = stage + (size_t)q * 5;
#pragma unroll
        for (int e = 0; e < 5; ++e) o[e] = box[e];
    }
    __syncthreads();
    if constexpr (FAST) {
        // suppression bit matrix: word (q, w) = the candidates j in [64 w, 64 w + 64), j > q, that candidate q suppresses if it is kept
        const int W = (cnt + 63) >> 6;
        for (int idx = tid; idx < cnt * W; idx += 256) {
            const int q = idx / W, w = idx - q * W;
            unsigned long long bits = 0;
            const int j0 = w << 6;
            if (j0 + 63 > q) {
                const float4 bq = sbox[q];
                for (int t = 0; t < 64; ++t) {
                    const int j = j0 + t;
                    if (j <= q || j >= cnt) continue;
                    if (det_suppresses<ROTATED>(bq, sbox[j], stage + (size_t)q * 5, stage + (size_t)j * 5, p.nms_thr)) bits |= 1ull << t;
                }
            }
            smask[idx] = bits;
        }
        __syncthreads();
        if (tid < 64) {   // one wave: lane w owns word w of the "removed" set (W <= 8)
            unsigned long long removed = 0;
            int nk = 0;
            for (int q = 0; q < cnt; ++q) {
                const unsigned long long word = __shfl(removed, q >> 6);
                if (!((word >> (q & 63)) & 1ull)) {        // wave-uniform
                    if (tid == 0) skept[nk] = q;
                    ++nk;
                    if (tid < W) removed |= smask[q * W + tid];
                }
            }
            if (tid == 0) s_nkept = nk;
        }
        __syncthreads();
    } else {
        // greedy scan: candidate q against the kept list by all threads in parallel
        for (int q = 0; q < cnt; ++q) {
            const float4 bq = sbox[q];
            const int nk = s_nkept;
            int sup = 0;
            for (int k = tid; k < nk; k += 256)
                if (det_suppresses<ROTATED>(sbox[skept[k]], bq, stage + (size_t)skept[k] * 5, stage + (size_t)q * 5, p.nms_thr)) sup = 1;
            sup = __syncthreads_or(sup);
            if (!sup && tid == 0) {
                skept[nk] = q;
                s_nkept = nk + 1;
            }
            __syncthreads();
        }
    }
    // compact the kept detections to the front (sorted positions are increasing: position k <- skept[k] >= k, reads of a batch before its writes)
    const int nk = s_nkept;
    for (int k0 = 0; k0 < nk; k0 += 256) {
        const int k = k0 + tid;
        float v[5];
        unsigned tie = 0;
        if (k < nk) {
            const int src = skept[k];
            for (int e = 0; e < 5; ++e) v[e] = stage[(size_t)src * 5 + e];
            tie = (unsigned)(skey[src] & 0xffffffffu);
        }
        __syncthreads();
        if (k < nk) {
            const int g = (int)(tie / (unsigned)cap_in), r = (int)(tie - (unsigned)g * (unsigned)cap_in);
            const int j = g == 0 ? i : g - 1;
            for (int e = 0; e < 5; ++e) stage[(size_t)k * 5 + e] = v[e];
            out_scores[(size_t)ego * cap_out + k] = p.scores[((size_t)j * B + b) * cap_in + r];
            out_src[(size_t)ego * cap_out + k] = j * cap_in + r;
        }
        __syncthreads();
    }
    if (tid == 0) out_count[ego] = nk;
}

template <bool ROTATED>
static int late_fuse_launch(const late_args &p, float *out_boxes, float *out_scores, int32_t *out_src, int32_t *out_count, hipStream_t s) {
    const int n = p.A * p.B;
    const int smem_fast = NMS_FAST_CAP * 28 + NMS_FAST_CAP * (NMS_FAST_CAP / 64) * 8;   // 46 KiB: no LDS opt-in, three workgroups per CU
    const int rc = v2x_launch<late_fuse_kernel<ROTATED, true>, 0>("late_fuse_kernel", dim3(n), dim3(256), smem_fast, s, p, out_boxes, out_scores, out_src,
                                                                  out_count, NMS_FAST_CAP, 0);
    if (rc != V2X_OK || p.cap_out <= NMS_FAST_CAP) return rc;   // no ego can be pending: one launch
    return v2x_launch<late_fuse_kernel<ROTATED, false>, DET_MAX_CAP * 28>("late_fuse_kernel", dim3(n), dim3(256), p.cap_out * 28, s, p, out_boxes, out_scores,
                                                                          out_src, out_count, p.cap_out, 1);
}

extern "C" int v2x_det_late_fuse(const float *boxes, const float *scores, const int32_t *counts, int A, int B, int cap_in,
                                 const float *rigid, const uint8_t *link, float x_lo, float x_hi, float y_lo, float y_hi,
                                 float nms_thr, int rotated, int cap_out, float *out_boxes, float *out_scores,
                                 int32_t *out_src, int32_t *out_count, v2x_stream_t stream) {
    V2X_REQUIRE(A >= 0 && B >= 0, "v2x_det_late_fuse: negative size (A=%d, B=%d)", A, B);
    if (A == 0 || B == 0) return V2X_OK;
    V2X_REQUIRE(A <= 65536 && (long long)A * B <= 0x7fffffffLL / DET_MAX_CAP, "v2x_det_late_fuse: A=%d, B=%d: at most 65536 agents and 2^19 egos", A, B);
    V2X_REQUIRE(cap_in >= 64 && cap_in <= DET_MAX_CAP && (cap_in & (cap_in - 1)) == 0, "v2x_det_late_fuse: cap_in=%d must be a power of two in [64, %d]", cap_in,
                DET_MAX_CAP);
    V2X_REQUIRE(cap_out >= 64 && cap_out <= DET_MAX_CAP && (cap_out & (cap_out - 1)) == 0, "v2x_det_late_fuse: cap_out=%d must be a power of two in [64, %d]",
                cap_out, DET_MAX_CAP);
    V2X_REQUIRE(boxes && scores && counts && rigid && link && out_boxes && out_scores && out_src && out_count, "v2x_det_late_fuse: null pointer");
    const late_args p = {boxes, scores, counts, rigid, link, A, B, cap_in, cap_out, x_lo, x_hi, y_lo, y_hi, nms_thr};
    return rotated ? late_fuse_launch<true>(p, out_boxes, out_scores, out_src, out_count, (hipStream_t)stream)
                   : late_fuse_launch<false>(p, out_boxes, out_scores, out_src, out_count, (hipStream_t)stream);
}

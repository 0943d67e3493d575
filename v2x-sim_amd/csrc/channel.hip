// Degraded links: this step's fusion plan and poses from the static plan and the clean poses -- p_com_outage (every directed
// link down with probability p, independently) and pose noise (Gaussian, sigma metres, on the translation of every agent-to-agent transform).  The draw
// is counter-based (channel_math.h: Philox4x32-10 on (step, frame, domain, ego, source) under the seed), so it depends on nothing but those: not on the
// launch geometry, the item order or which agents are present, and a host predicts it bit for bit.
//   channel_degrade_kernel   ONE workgroup of 256 threads; the problem is 128 frames x 25 pairs.  The step counter lives in device memory: every thread
//                            reads it first, the last statement -- behind a workgroup barrier that every read precedes -- is thread 0 leaving step + 1.
//                            A replayed hipGraph therefore draws fresh links and noise at every replay, and nothing synchronises with the host.
//     pass 1, a thread per directed pair (f, i, j) of [Bt][A][A]: link[f][i][j] = 0, and with pose noise the 16 floats of trans[f][i][j] copied to
//             trans_out with sigma * (nx, ny, nz) added to entries [0][3], [1][3], [2][3] where j != i.
//     pass 2, behind a barrier, a thread per (item m, source j): coef[m][j] = coef0[m][j], or 0 where j is not the ego and the link is down; row
//             m * A + j of coef2 (DiscoNet's one-hot rows) = coef[m][j] on its own column, 0 elsewhere; link[f][ego][j] = (coef[m][j] != 0), j != ego.
// Every output element is written by every launch; the static rows coef0 and the clean poses are only read.
#include "common.h"
#include "channel_math.h"

struct channel_args {
    const int32_t *items;      // [n_out][2] (ego, frame)
    int n_out, A, Bt;
    const float *coef0;        // [n_out][A] or null (pose noise alone)
    float *coef;               // [n_out][A] or null, with coef0
    float *coef2;              // [n_out * A][A] or null
    uint8_t *link;             // [Bt][A][A] or null
    const float *trans;        // [Bt][A][A][16] or null (no pose noise)
    float *trans_out;          // [Bt][A][A][16], with trans
    float p_outage, pose_sigma;
    uint64_t seed;
    uint64_t *step;
};

__global__ __launch_bounds__(256) void channel_degrade_kernel(channel_args p) {
    const int tid = threadIdx.x, A = p.A, AA = A * A;
    const uint64_t step = *p.step;

    if (p.link || p.trans_out) {
        const long long pairs = (long long)p.Bt * AA;
        for (long long q = tid; q < pairs; q += 256) {
            if (p.link) p.link[q] = 0;
            if (!p.trans_out) continue;
            const int f = (int)(q / AA), r = (int)(q - (long long)f * AA), i = r / A, j = r - i * A;
            float t[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) t[e] = p.trans[q * 16 + e];
            if (j != i) {
                float n[3];
                chan_normals(chan_words(p.seed, step, (uint32_t)f, CHAN_DOMAIN_POSE, (uint32_t)i, (uint32_t)j), n);
                t[3] += p.pose_sigma * n[0];
                t[7] += p.pose_sigma * n[1];
                t[11] += p.pose_sigma * n[2];
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) p.trans_out[q * 16 + e] = t[e];
        }
    }
    __syncthreads();     // the cleared link table before the entries of the present egos

    if (p.coef) {
        const long long entries = (long long)p.n_out * A;
        for (long long e = tid; e < entries; e += 256) {
            const long long m = e / A;
            const int j = (int)(e - m * A), i = p.items[2 * m], f = p.items[2 * m + 1];
            const bool inside = (unsigned)i < (unsigned)A && (unsigned)f < (unsigned)p.Bt;     // an item outside the tables keeps its static row and draws nothing
            float c = p.coef0[e];
            if (inside && j != i && p.p_outage > 0.0f &&
                chan_link_down(chan_words(p.seed, step, (uint32_t)f, CHAN_DOMAIN_OUTAGE, (uint32_t)i, (uint32_t)j), p.p_outage))
                c = 0.0f;
            p.coef[e] = c;
            if (p.coef2)
                for (int k = 0; k < A; ++k) p.coef2[e * A + k] = (k == j) ? c : 0.0f;
            if (p.link && inside && j != i) p.link[((long long)f * A + i) * A + j] = c != 0.0f ? 1 : 0;
        }
    }

    __syncthreads();     // every thread has read the step
    if (tid == 0) *p.step = step + 1;
}

static bool chan_aligned(const void *ptr, uintptr_t a) { return (reinterpret_cast<uintptr_t>(ptr) & (a - 1)) == 0; }

extern "C" int v2x_channel_degrade(const int32_t *items, int n_out, int A, int Bt, const float *coef0, float *coef, float *coef2, uint8_t *link,
                                   const float *trans, float *trans_out, float p_outage, float pose_sigma, uint64_t seed, uint64_t *step_dev,
                                   v2x_stream_t stream) {
    if (n_out == 0) return V2X_OK;
    V2X_REQUIRE(n_out > 0, "v2x_channel_degrade: negative n_out (%d)", n_out);
    V2X_REQUIRE(A >= 1 && A <= CHAN_MAX_AGENTS, "v2x_channel_degrade: A=%d must lie in [1, %d]", A, CHAN_MAX_AGENTS);
    V2X_REQUIRE(Bt >= 1, "v2x_channel_degrade: Bt=%d must be >= 1", Bt);
    V2X_REQUIRE(p_outage >= 0.0f && p_outage <= 1.0f, "v2x_channel_degrade: p_outage=%g must lie in [0, 1]", (double)p_outage);
    V2X_REQUIRE(pose_sigma >= 0.0f && pose_sigma <= 3.0e38f, "v2x_channel_degrade: pose_sigma=%g must be finite and >= 0", (double)pose_sigma);
    V2X_REQUIRE(items && step_dev, "v2x_channel_degrade: null pointer (items, step_dev)");
    V2X_REQUIRE((coef0 != nullptr) == (coef != nullptr), "v2x_channel_degrade: coef0 and coef come together (both NULL: pose noise alone)");
    V2X_REQUIRE(coef || (!coef2 && !link && p_outage == 0.0f), "v2x_channel_degrade: p_outage > 0, coef2 and link need coef0 and coef");
    V2X_REQUIRE(coef != coef0 || !coef, "v2x_channel_degrade: coef must not be the static rows coef0");
    V2X_REQUIRE((trans_out == nullptr) == (pose_sigma == 0.0f), "v2x_channel_degrade: trans_out is NULL if and only if pose_sigma == 0");
    V2X_REQUIRE(!trans_out || (trans && trans != trans_out), "v2x_channel_degrade: pose noise reads trans and writes trans_out, never in place");
    V2X_REQUIRE(chan_aligned(items, 4) && chan_aligned(coef0, 4) && chan_aligned(coef, 4) && chan_aligned(coef2, 4) && chan_aligned(trans, 4) &&
                    chan_aligned(trans_out, 4) && chan_aligned(step_dev, 8),
                "v2x_channel_degrade: int32 / fp32 arrays must be 4-byte aligned, step_dev 8-byte aligned");
    const channel_args p = {items, n_out, A, Bt, coef0, coef, coef2, link, trans_out ? trans : nullptr, trans_out, p_outage, pose_sigma, seed, step_dev};
    return v2x_launch<channel_degrade_kernel, 0>("channel_degrade_kernel", dim3(1), dim3(256), 0, (hipStream_t)stream, p);
}

// Row f-5: the HOTA family of tracking metrics (TrackEval's hota.py, frozen in DESIGN.md section 3) for ALL sequences of a test split in one call: five
// launches whatever the number of sequences and frames, no device-to-host synchronisation between them, no atomics.
//   1. hota_sim_kernel    grid S F        a frame's valid boxes are compacted (count clamped to [0, cap], an id outside [0, n_ids) makes its box absent), the
//                                         similarity S = IoU in fp64 (lane = track, loop = ground truth) and J = S / (colsum + rowsum - S) go to the workspace;
//   2. hota_pot_kernel    grid S NG tiles a wave owns (sequence, ground-truth id, tile of 64 track ids): it walks the frames IN ORDER, finds the id's slot by
//                                         ballot, the slot of each of its 64 track ids through an LDS table, and adds that entry of J to a REGISTER (lane =
//                                         track id): pot[g][k], gt_cnt[g], trk_cnt[k] -- a fixed summation order by construction;
//   3. hota_match_kernel  grid S F        gas[g][k] S = pot / (gt_cnt + trk_cnt - pot) S into LDS [small][large] (rows <= columns both ways, like assign_kernel), the
//                                         maximum-sum assignment (trk_assign, track_assign.h), then each ground-truth slot's matched track id and similarity;
//   4. hota_count_kernel  grid S NG tiles the same walk with lane = alpha: per-id TP and sum of matched S in registers, the match counts mc[alpha][g][k] of the
//                                         tile in LDS; at the end the lane sums its row of mc^2 / max(1, .) in track-id order -- mc never reaches memory;
//   5. hota_reduce_kernel grid S n_alpha  lane-strided sums over the ground-truth ids and the frames, one butterfly: TP, FN, FP, AssA, AssRe, AssPr, loc.
// A workgroup = one wave of 64; the barriers order that wave's LDS traffic.  Every loop is bounded by cap, F, an id count or 64; every index is
// formed from clamped counts and validated ids, so no input writes outside its buffers; a non-finite similarity or score reads as 0, so the assignment sees
// finite numbers only (its termination: track_assign.h).  Duplicate ids within a frame (a caller error) make one of the two boxes win: unspecified, memory-safe.
// Padding does not change a bit of a sequence's result: a padded frame, ground-truth id, track id or tile adds an exact 0.0 in the same place of the same order.
#include "track_sim.h"

#define HOTA_MAX_ALPHA 32
#define HOTA_NBUF 14

struct HotaDims {
    int S, F, cap, NG, NT, tiles, n_alpha;
};

struct HotaWs {
    double *sim, *jm;            // [S][F][cap][cap]  (ground-truth slot, track slot) of the compacted frame
    double *pot;                 // [S][NG][NT]
    double *msim;                // [S][F][cap]       the similarity of a ground-truth slot's match
    double *part;                // [S][n_alpha][NG][tiles][3]
    double *locg;                // [S][n_alpha][NG]
    int32_t *gt_cnt, *trk_cnt;   // [S][NG], [S][NT]
    int32_t *cgid, *ctid, *mtrk; // [S][F][cap]       compacted ids; the track id a ground-truth slot matched, or -1
    int32_t *nvg, *nvt;          // [S][F]            valid boxes of the frame
    int32_t *tpg;                // [S][n_alpha][NG]
};

__global__ __launch_bounds__(TRK_N) void hota_sim_kernel(const float *gt_boxes, const int32_t *gt_ids, const int32_t *gt_count, const float *trk_boxes,
                                                         const int32_t *trk_ids, const int32_t *trk_count, const HotaDims d, const HotaWs w) {
    __shared__ TrkLds L;
    const size_t sf = blockIdx.x, row0 = sf * d.cap;
    const int lane = threadIdx.x;
    const int ng = hota_compact(gt_boxes + row0 * 4, gt_ids + row0, gt_count[sf], d.cap, d.NG, L.dbox, w.cgid + row0, lane);
    const int nt = hota_compact(trk_boxes + row0 * 4, trk_ids + row0, trk_count[sf], d.cap, d.NT, L.pbox, w.ctid + row0, lane);
    if (lane == 0) {
        w.nvg[sf] = ng;
        w.nvt[sf] = nt;
    }
    __syncthreads();
    const float4 tb = lane < nt ? L.pbox[lane] : make_float4(0.f, 0.f, 0.f, 0.f);
    double col = 0.0;                                 // the column sum: ground-truth slots in order
    for (int i = 0; i < ng; ++i) {
        const double s = lane < nt ? hota_iou(L.dbox[i], tb) : 0.0;
        L.M[i * TRK_N + lane] = s;                    // read back by this lane only
        col += s;
        const double r = hota_wave_sum(s);
        if (lane == 0) L.u[i] = r;
    }
    __syncthreads();
    if (lane < nt)
        for (int i = 0; i < ng; ++i) {
            const double s = L.M[i * TRK_N + lane];
            const double den = col + L.u[i] - s;
            const size_t o = (row0 + i) * d.cap + lane;
            w.sim[o] = s;
            w.jm[o] = den > DBL_EPSILON ? hota_finite0(s / den) : 0.0;
        }
}

__global__ __launch_bounds__(TRK_N) void hota_pot_kernel(const HotaDims d, const HotaWs w) {
    __shared__ int slot_of[TRK_N];                    // track id of the tile -> its slot in the frame, or -1
    const int lane = threadIdx.x;
    const int tile = blockIdx.x % d.tiles, g = (blockIdx.x / d.tiles) % d.NG, s = blockIdx.x / d.tiles / d.NG;
    const int k0 = tile * TRK_N;
    double acc = 0.0;
    int gcnt = 0, tcnt = 0;
    for (int f = 0; f < d.F; ++f) {
        const size_t sf = (size_t)s * d.F + f, row0 = sf * d.cap;
        const int ng = w.nvg[sf], nt = w.nvt[sf];
        const int slot = hota_slot_of(w.cgid + row0, ng, g, lane);
        gcnt += slot >= 0;
        if (nt == 0) continue;                        // wave-uniform
        slot_of[lane] = -1;
        __syncthreads();
        if (lane < nt) {
            const int r = w.ctid[row0 + lane] - k0;
            if (r >= 0 && r < TRK_N) slot_of[r] = lane;
        }
        __syncthreads();
        const int so = slot_of[lane];                 // the next frame's clear of this entry is this lane's own, behind this read
        tcnt += so >= 0;
        if (slot >= 0 && so >= 0) acc += w.jm[(row0 + slot) * d.cap + so];
    }
    const int k = k0 + lane;
    if (k < d.NT) {
        w.pot[((size_t)s * d.NG + g) * d.NT + k] = acc;
        if (g == 0) w.trk_cnt[(size_t)s * d.NT + k] = tcnt;
    }
    if (tile == 0 && lane == 0) w.gt_cnt[(size_t)s * d.NG + g] = gcnt;
}

__global__ __launch_bounds__(TRK_N) void hota_match_kernel(const HotaDims d, const HotaWs w) {
    __shared__ TrkLds L;
    int *gid = L.t2d, *tid = L.birth;                 // the frame's ids by slot
    const size_t sf = blockIdx.x, row0 = sf * d.cap;
    const int lane = threadIdx.x, s = blockIdx.x / d.F;
    const int ng = w.nvg[sf], nt = w.nvt[sf];
    if (ng == 0) return;
    if (nt == 0) {
        if (lane < ng) {
            w.mtrk[row0 + lane] = -1;
            w.msim[row0 + lane] = 0.0;
        }
        return;
    }
    gid[lane] = lane < ng ? w.cgid[row0 + lane] : 0;
    tid[lane] = lane < nt ? w.ctid[row0 + lane] : 0;
    L.d2t[lane] = -1;
    __syncthreads();
    const bool tr = ng > nt;                          // lanes walk the larger dimension
    const int ns = tr ? nt : ng, nb = tr ? ng : nt;
    const double *pot = w.pot + (size_t)s * d.NG * d.NT;
    const int32_t *gcnt = w.gt_cnt + (size_t)s * d.NG, *tcnt = w.trk_cnt + (size_t)s * d.NT;
    if (lane < nb)
        for (int i = 0; i < ns; ++i) {
            const int gi = tr ? lane : i, tj = tr ? i : lane;
            const int g = gid[gi], k = tid[tj];
            const double p = pot[(size_t)g * d.NT + k];
            const double gas = p / ((double)(gcnt[g] + tcnt[k]) - p);
            L.M[i * TRK_N + lane] = hota_finite0(gas * w.sim[(row0 + gi) * d.cap + tj]);
        }
    __syncthreads();
    const int p = trk_assign(L.M, L.u, ns, nb, lane);
    if (lane < nb) {
        if (tr) L.d2t[lane] = p;
        else if (p >= 0) L.d2t[p] = lane;
    }
    __syncthreads();
    if (lane < ng) {
        const int c = L.d2t[lane];
        w.mtrk[row0 + lane] = c >= 0 ? tid[c] : -1;
        w.msim[row0 + lane] = c >= 0 ? w.sim[(row0 + lane) * d.cap + c] : 0.0;
    }
}

__global__ __launch_bounds__(TRK_N) void hota_count_kernel(const double *alpha, const HotaDims d, const HotaWs w) {
    __shared__ int mc[HOTA_MAX_ALPHA][TRK_N + 1];     // [alpha][track id of the tile]; a row is touched by its own lane only (+ 1: the lanes hit one column)
    const int lane = threadIdx.x;
    const int tile = blockIdx.x % d.tiles, g = (blockIdx.x / d.tiles) % d.NG, s = blockIdx.x / d.tiles / d.NG;
    const int k0 = tile * TRK_N;
    const bool act = lane < d.n_alpha;
    const double thr = act ? alpha[lane] - DBL_EPSILON : 0.0;
    if (act)
        for (int r = 0; r < TRK_N; ++r) mc[lane][r] = 0;
    int tp = 0;
    double loc = 0.0;
    for (int f = 0; f < d.F; ++f) {
        const size_t sf = (size_t)s * d.F + f, row0 = sf * d.cap;
        const int slot = hota_slot_of(w.cgid + row0, w.nvg[sf], g, lane);
        if (slot < 0 || w.nvt[sf] == 0) continue;     // wave-uniform
        const int mk = w.mtrk[row0 + slot];
        if (mk < 0) continue;
        const double ms = w.msim[row0 + slot];
        if (act && ms >= thr) {
            ++tp;
            loc += ms;
            const int r = mk - k0;
            if (r >= 0 && r < TRK_N) mc[lane][r] += 1;
        }
    }
    if (!act) return;
    const int gc = w.gt_cnt[(size_t)s * d.NG + g];
    double a = 0.0, re = 0.0, pr = 0.0;
    for (int r = 0; r < TRK_N && k0 + r < d.NT; ++r) {
        const int c = mc[lane][r];
        if (c == 0) continue;
        const int tc = w.trk_cnt[(size_t)s * d.NT + k0 + r];
        const double cc = (double)c * (double)c;
        a += cc / (double)max(1, gc + tc - c);
        re += cc / (double)max(1, gc);
        pr += cc / (double)max(1, tc);
    }
    const size_t o = ((size_t)s * d.n_alpha + lane) * d.NG + g;
    double *pt = w.part + (o * d.tiles + tile) * 3;
    pt[0] = a;
    pt[1] = re;
    pt[2] = pr;
    if (tile == 0) {
        w.tpg[o] = tp;
        w.locg[o] = loc;
    }
}

__global__ __launch_bounds__(TRK_N) void hota_reduce_kernel(const HotaDims d, const HotaWs w, int32_t *out_i, double *out_f) {
    const int lane = threadIdx.x;
    const int s = blockIdx.x / d.n_alpha;
    const size_t o0 = (size_t)blockIdx.x * d.NG;      // blockIdx.x = s n_alpha + alpha
    double a = 0.0, re = 0.0, pr = 0.0, loc = 0.0;
    long long tp = 0, n_gt = 0, n_trk = 0;
    if (d.NT > 0)                                     // without track ids kernels 2-4 did not run: every term is 0
        for (int g = lane; g < d.NG; g += TRK_N) {
            for (int t = 0; t < d.tiles; ++t) {
                const double *pt = w.part + ((o0 + g) * d.tiles + t) * 3;
                a += pt[0];
                re += pt[1];
                pr += pt[2];
            }
            tp += w.tpg[o0 + g];
            loc += w.locg[o0 + g];
        }
    for (int f = lane; f < d.F; f += TRK_N) {
        n_gt += w.nvg[(size_t)s * d.F + f];
        n_trk += w.nvt[(size_t)s * d.F + f];
    }
    a = hota_wave_sum(a);
    re = hota_wave_sum(re);
    pr = hota_wave_sum(pr);
    loc = hota_wave_sum(loc);
    tp = hota_wave_sum(tp);
    n_gt = hota_wave_sum(n_gt);
    n_trk = hota_wave_sum(n_trk);
    if (lane == 0) {
        const double den = (double)(tp > 1 ? tp : 1);
        int32_t *oi = out_i + (size_t)blockIdx.x * 3;
        double *of = out_f + (size_t)blockIdx.x * 4;
        oi[0] = (int32_t)tp;
        oi[1] = (int32_t)(n_gt - tp);
        oi[2] = (int32_t)(n_trk - tp);
        of[0] = a / den;
        of[1] = re / den;
        of[2] = pr / den;
        of[3] = loc;
    }
}

// the workspace: byte offset of each buffer (16-byte aligned) and the total; false on a size out of range or an overflow
static bool hota_layout(int S, int F, int cap, int NG, int NT, int n_alpha, size_t off[HOTA_NBUF], size_t *total) {
    if (S < 0 || F < 1 || cap < 1 || cap > TRK_N || NG < 0 || NT < 0 || n_alpha < 1 || n_alpha > HOTA_MAX_ALPHA) return false;
    const size_t tiles = ((size_t)NT + TRK_N - 1) / TRK_N;
    const size_t dims[HOTA_NBUF][6] = {
        {8, (size_t)S, (size_t)F, (size_t)cap, (size_t)cap, 1},       {8, (size_t)S, (size_t)F, (size_t)cap, (size_t)cap, 1},
        {8, (size_t)S, (size_t)NG, (size_t)NT, 1, 1},                 {8, (size_t)S, (size_t)F, (size_t)cap, 1, 1},
        {8, (size_t)S, (size_t)n_alpha, (size_t)NG, tiles, 3},        {8, (size_t)S, (size_t)n_alpha, (size_t)NG, 1, 1},
        {4, (size_t)S, (size_t)NG, 1, 1, 1},                          {4, (size_t)S, (size_t)NT, 1, 1, 1},
        {4, (size_t)S, (size_t)F, (size_t)cap, 1, 1},                 {4, (size_t)S, (size_t)F, (size_t)cap, 1, 1},
        {4, (size_t)S, (size_t)F, (size_t)cap, 1, 1},                 {4, (size_t)S, (size_t)F, 1, 1, 1},
        {4, (size_t)S, (size_t)F, 1, 1, 1},                           {4, (size_t)S, (size_t)n_alpha, (size_t)NG, 1, 1},
    };
    size_t at = 0;
    for (int b = 0; b < HOTA_NBUF; ++b) {
        size_t bytes = 1;
        for (int k = 0; k < 6; ++k)
            if (__builtin_mul_overflow(bytes, dims[b][k], &bytes)) return false;
        off[b] = at;
        if (__builtin_add_overflow(bytes, (size_t)15, &bytes)) return false;
        if (__builtin_add_overflow(at, bytes & ~(size_t)15, &at)) return false;
    }
    *total = at > 16 ? at : 16;
    return true;
}

extern "C" size_t v2x_hota_workspace_size(int n_seq, int n_frames, int cap, int n_gt_ids, int n_trk_ids, int n_alpha) {
    size_t off[HOTA_NBUF], total = 0;
    return hota_layout(n_seq, n_frames, cap, n_gt_ids, n_trk_ids, n_alpha, off, &total) ? total : 0;
}

extern "C" int v2x_hota_sequences(const float *gt_boxes, const int32_t *gt_ids, const int32_t *gt_count, const float *trk_boxes, const int32_t *trk_ids,
                                  const int32_t *trk_count, int n_seq, int n_frames, int cap, int n_gt_ids, int n_trk_ids, const double *alpha, int n_alpha,
                                  void *workspace, size_t workspace_bytes, int32_t *out_i, double *out_f, v2x_stream_t stream) {
    V2X_REQUIRE(gt_boxes && gt_ids && gt_count && trk_boxes && trk_ids && trk_count && alpha && workspace && out_i && out_f, "v2x_hota_sequences: null pointer");
    V2X_REQUIRE(n_seq >= 0 && n_frames >= 1, "v2x_hota_sequences: n_seq = %d, n_frames = %d", n_seq, n_frames);
    V2X_REQUIRE(cap >= 1 && cap <= TRK_N, "v2x_hota_sequences: cap = %d outside [1, 64] (one wave per frame)", cap);
    V2X_REQUIRE(n_gt_ids >= 0 && n_trk_ids >= 0, "v2x_hota_sequences: n_gt_ids = %d, n_trk_ids = %d must not be negative", n_gt_ids, n_trk_ids);
    V2X_REQUIRE(n_alpha >= 1 && n_alpha <= HOTA_MAX_ALPHA, "v2x_hota_sequences: n_alpha = %d outside [1, %d]", n_alpha, HOTA_MAX_ALPHA);
    size_t off[HOTA_NBUF], total = 0;
    V2X_REQUIRE(hota_layout(n_seq, n_frames, cap, n_gt_ids, n_trk_ids, n_alpha, off, &total), "v2x_hota_sequences: the workspace size overflows");
    V2X_REQUIRE(workspace_bytes >= total, "v2x_hota_sequences: workspace of %zu bytes, v2x_hota_workspace_size asks for %zu", workspace_bytes, total);
    const long long tiles = ((long long)n_trk_ids + TRK_N - 1) / TRK_N, grid_max = 1ll << 24;    // grids stay far below 2^32 threads
    V2X_REQUIRE((long long)n_seq * n_frames <= grid_max && (long long)n_seq * n_gt_ids <= grid_max && (long long)n_seq * n_gt_ids * tiles <= grid_max,
                "v2x_hota_sequences: n_seq x n_frames and n_seq x n_gt_ids x ceil(n_trk_ids / 64) must not exceed 2^24");
    V2X_REQUIRE(((reinterpret_cast<uintptr_t>(gt_boxes) | reinterpret_cast<uintptr_t>(trk_boxes) | reinterpret_cast<uintptr_t>(workspace)) & 15) == 0,
                "v2x_hota_sequences: gt_boxes, trk_boxes and workspace must be 16-byte aligned");
    if (n_seq == 0) return V2X_OK;
    char *base = static_cast<char *>(workspace);
    HotaWs w;
    w.sim = reinterpret_cast<double *>(base + off[0]);
    w.jm = reinterpret_cast<double *>(base + off[1]);
    w.pot = reinterpret_cast<double *>(base + off[2]);
    w.msim = reinterpret_cast<double *>(base + off[3]);
    w.part = reinterpret_cast<double *>(base + off[4]);
    w.locg = reinterpret_cast<double *>(base + off[5]);
    w.gt_cnt = reinterpret_cast<int32_t *>(base + off[6]);
    w.trk_cnt = reinterpret_cast<int32_t *>(base + off[7]);
    w.cgid = reinterpret_cast<int32_t *>(base + off[8]);
    w.ctid = reinterpret_cast<int32_t *>(base + off[9]);
    w.mtrk = reinterpret_cast<int32_t *>(base + off[10]);
    w.nvg = reinterpret_cast<int32_t *>(base + off[11]);
    w.nvt = reinterpret_cast<int32_t *>(base + off[12]);
    w.tpg = reinterpret_cast<int32_t *>(base + off[13]);
    const HotaDims d = {n_seq, n_frames, cap, n_gt_ids, n_trk_ids, (int)tiles, n_alpha};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 frames(n_seq * n_frames), ids(n_seq * n_gt_ids * (int)tiles), wave(TRK_N);
    hipLaunchKernelGGL(hota_sim_kernel, frames, wave, 0, st, gt_boxes, gt_ids, gt_count, trk_boxes, trk_ids, trk_count, d, w);
    V2X_CHECK_LAUNCH("hota_sim_kernel");
    if (ids.x > 0) {                                  // no ground-truth id or no track id: nothing can match, kernel 5 reads the frame counts only
        hipLaunchKernelGGL(hota_pot_kernel, ids, wave, 0, st, d, w);
        V2X_CHECK_LAUNCH("hota_pot_kernel");
        hipLaunchKernelGGL(hota_match_kernel, frames, wave, 0, st, d, w);
        V2X_CHECK_LAUNCH("hota_match_kernel");
        hipLaunchKernelGGL(hota_count_kernel, ids, wave, 0, st, alpha, d, w);
        V2X_CHECK_LAUNCH("hota_count_kernel");
    }
    hipLaunchKernelGGL(hota_reduce_kernel, dim3(n_seq * n_alpha), wave, 0, st, d, w, out_i, out_f);
    V2X_CHECK_LAUNCH("hota_reduce_kernel");
    return V2X_OK;
}

// Row f-5: the CLEAR MOT family (TP, FN, FP, IDSW, MOTP, MT / PT / ML, Frag) and the Identity family (IDTP, IDFN, IDFP) of ALL sequences of a test split
// in one call (TrackEval's clear.py and identity.py as DESIGN.md section 3 freezes them): five launches whatever the number of sequences and frames, no
// device-to-host synchronisation between them, no atomics.
//   1. mot_sim_kernel     grid S F        hota.hip's frame reading (track_sim.h): the valid boxes compacted, S = IoU in fp64 (lane = track, loop = ground
//                                         truth) to the workspace;
//   2. mot_clear_kernel   grid S          ONE wave walks a sequence's frames IN ORDER.  Per frame: the continuity pairs first (a ground-truth id whose match of
//                                         the previous frame is present with S >= thr - 2^-52: utils/mot_metrics.py gives the argument why every optimum of
//                                         1000 [continuity] + S contains them), their rows and columns removed, trk_assign in fp64 on the thresholded rest,
//                                         matched = entry > 0.  Per-id state in the workspace: prev (the last matched track id), lastf (the frame of that match:
//                                         "in the previous frame's matches" = lastf == f - 1, so a frame without matches clears the term by itself), present,
//                                         matched, starts.  The matched similarities are added by lane 0 in slot order: frame order, then slot order;
//   3. mot_pmc_kernel     grid S NG tiles hota_pot_kernel's walk with an integer register: pmc[g][k] = frames in which both are present with S >= thr (plain),
//                                         stored [small id side][large id side] so that a row of kernel 4's scan is contiguous;
//   4. mot_wide_kernel    grid S          one workgroup of 256 per sequence: the maximum-weight assignment of the small id side to the large one -- shortest
//                                         augmenting paths on -pmc with 64-bit INTEGER potentials, lanes stride over the columns, the (value, column) minimum of the
//                                         workgroup goes through LDS, ties to the lowest column.  <= small augmentations of <= large + 1 steps; an all-zero row is left out.  IDTP = its value:
//                                         the weights are integers >= 0, so the value is unique (whatever the matching) and equals the optimum over PARTIAL matchings;
//   5. mot_reduce_kernel  grid S          MT / PT / ML / Frag in integers over the ids with present > 0, the box totals of the frames, the eleven outputs.
// Every loop is bounded by cap, F, an id count or the workgroup size; every index is formed from clamped counts and validated ids.  Duplicate ids within a
// frame (a caller error) make lanes write the same per-id word or claim the same column: unspecified numbers, memory-safe, terminating.  Padding (frames,
// ids, the other sequences) does not change a bit of a sequence's outputs: the integers are schedule-free and MOTP_sum has one order.
#include "track_sim.h"

#define MOT_MAX_IDS 2048         // ids per side of one sequence: u, v, minv (8 bytes), way, row (2 bytes) and used (1 byte) per id = 29 bytes x 2048 = 58 KiB of
                                 // the 64 KiB a workgroup's static LDS may take (the CU holds 160 KiB)
#define MOT_WG 256
#define MOT_NBUF 13
#define MOT_HUGE (1ll << 62)

struct MotDims {
    int S, F, cap, NG, NT, tiles;
    int tr;                      // NG > NT: the rows of the wide assignment are the track ids
};

struct MotWs {
    double *sim;                 // [S][F][cap][cap]  (ground-truth slot, track slot) of the compacted frame
    double *seq_f;               // [S]               MOTP_sum
    int32_t *pmc;                // [S][small][large]
    int32_t *cgid, *ctid;        // [S][F][cap]
    int32_t *nvg, *nvt;          // [S][F]
    int32_t *prev, *lastf, *present, *matched, *starts;   // [S][NG]
    int32_t *seq_i;              // [S][8]            TP, FN, FP, IDSW (kernel 2), IDTP (kernel 4)
};

__global__ __launch_bounds__(TRK_N) void mot_sim_kernel(const float *gt_boxes, const int32_t *gt_ids, const int32_t *gt_count, const float *trk_boxes,
                                                        const int32_t *trk_ids, const int32_t *trk_count, const MotDims d, const MotWs w) {
    __shared__ float4 gbox[TRK_N], tbox[TRK_N];
    const size_t sf = blockIdx.x, row0 = sf * d.cap;
    const int lane = threadIdx.x;
    const int ng = hota_compact(gt_boxes + row0 * 4, gt_ids + row0, gt_count[sf], d.cap, d.NG, gbox, w.cgid + row0, lane);
    const int nt = hota_compact(trk_boxes + row0 * 4, trk_ids + row0, trk_count[sf], d.cap, d.NT, tbox, w.ctid + row0, lane);
    if (lane == 0) {
        w.nvg[sf] = ng;
        w.nvt[sf] = nt;
    }
    __syncthreads();
    if (lane < nt) {
        const float4 tb = tbox[lane];
        for (int i = 0; i < ng; ++i) w.sim[(row0 + i) * d.cap + lane] = hota_iou(gbox[i], tb);
    }
}

__global__ __launch_bounds__(TRK_N) void mot_clear_kernel(const double thr, const MotDims d, const MotWs w) {
    __shared__ TrkLds L;
    __shared__ double ms[TRK_N];                      // the matched similarity of a ground-truth slot
    __shared__ int rmap[TRK_N], cmap[TRK_N];          // the ground-truth slots and the track slots no continuity pair took, in slot order
    int *tid = L.birth, *colfix = L.t2d;              // the frame's track ids by slot; columns a continuity pair took
    const int lane = threadIdx.x, s = blockIdx.x;
    const size_t id0 = (size_t)s * d.NG;
    int32_t *prev = w.prev + id0, *lastf = w.lastf + id0, *present = w.present + id0, *matched = w.matched + id0, *starts = w.starts + id0;
    for (int g = lane; g < d.NG; g += TRK_N) {
        prev[g] = -1;
        lastf[g] = -2;
        present[g] = matched[g] = starts[g] = 0;
    }
    __syncthreads();
    const double lo = thr - DBL_EPSILON;
    int tp = 0, fn = 0, fp = 0, idsw = 0;
    double motp = 0.0;                                // lane 0's
    for (int f = 0; f < d.F; ++f) {
        const size_t sf = (size_t)s * d.F + f, row0 = sf * d.cap;
        const int ng = w.nvg[sf], nt = w.nvt[sf];
        const int g = lane < ng ? w.cgid[row0 + lane] : -1;
        int pv = -1, lf = -2;
        if (g >= 0) {
            present[g] += 1;
            pv = prev[g];
            lf = lastf[g];
        }
        __syncthreads();                              // the per-id words change lanes from frame to frame; the previous frame's reads of L are over
        if (ng == 0 || nt == 0) {                     // wave-uniform; no match, so lastf keeps the continuity term of the next frame off
            fn += ng;
            fp += nt;
            continue;
        }
        tid[lane] = lane < nt ? w.ctid[row0 + lane] : -1;
        colfix[lane] = 0;
        L.d2t[lane] = -1;
        __syncthreads();
        int c = -1;                                   // the continuity pair of this ground-truth slot
        double sc = 0.0;
        if (g >= 0 && pv >= 0 && lf == f - 1)
            for (int j = 0; j < nt; ++j)
                if (tid[j] == pv) {
                    c = j;
                    break;
                }
        if (c >= 0) {
            sc = w.sim[(row0 + lane) * d.cap + c];
            if (!(sc >= lo && sc > 0.0)) c = -1;
        }
        if (c >= 0) colfix[c] = 1;
        const unsigned long long rowfree = __ballot(g >= 0 && c < 0);
        __syncthreads();
        const unsigned long long colfree = __ballot(lane < nt && !colfix[lane]);
        const int nr = __popcll(rowfree), nc = __popcll(colfree);
        const int rpos = __popcll(rowfree & trk_lt_mask(lane));      // this slot's row of the rest, when it is free
        if ((rowfree >> lane) & 1ull) rmap[rpos] = lane;
        if ((colfree >> lane) & 1ull) cmap[__popcll(colfree & trk_lt_mask(lane))] = lane;
        __syncthreads();
        const bool tr = nr > nc;                      // lanes walk the larger dimension of the rest
        const int ns = tr ? nc : nr, nb = tr ? nr : nc;
        int cc = c, t = -1;
        double sv = sc;
        if (ns > 0) {                                 // wave-uniform
            if (lane < nb)
                for (int i = 0; i < ns; ++i) {
                    const int gi = rmap[tr ? lane : i], tj = cmap[tr ? i : lane];
                    const double v = w.sim[(row0 + gi) * d.cap + tj];
                    L.M[i * TRK_N + lane] = v < lo ? 0.0 : v;
                }
            __syncthreads();
            const int p = trk_assign(L.M, L.u, ns, nb, lane);
            if (lane < nb) {
                if (tr) L.d2t[lane] = p;
                else if (p >= 0) L.d2t[p] = lane;
            }
            __syncthreads();
            if ((rowfree >> lane) & 1ull) {
                const int q = L.d2t[rpos];
                if (q >= 0) {
                    sv = tr ? L.M[q * TRK_N + rpos] : L.M[rpos * TRK_N + q];
                    if (sv > 0.0) cc = cmap[q];
                }
            }
        }
        const bool m = g >= 0 && cc >= 0;
        if (m) t = tid[cc];
        const unsigned long long mm = __ballot(m);
        idsw += __popcll(__ballot(m && pv >= 0 && pv != t));
        if (m) {
            starts[g] += lf != f - 1;
            matched[g] += 1;
            prev[g] = t;
            lastf[g] = f;
        }
        ms[lane] = m ? sv : 0.0;
        __syncthreads();
        if (lane == 0)
            for (int i = 0; i < ng; ++i)
                if ((mm >> i) & 1ull) motp += ms[i];
        const int nm = __popcll(mm);
        tp += nm;
        fn += ng - nm;
        fp += nt - nm;
    }
    if (lane == 0) {
        int32_t *o = w.seq_i + (size_t)s * 8;
        o[0] = tp;
        o[1] = fn;
        o[2] = fp;
        o[3] = idsw;
        w.seq_f[s] = motp;
    }
}

__global__ __launch_bounds__(TRK_N) void mot_pmc_kernel(const double thr, const MotDims d, const MotWs w) {
    __shared__ int slot_of[TRK_N];                    // track id of the tile -> its slot in the frame, or -1
    const int lane = threadIdx.x;
    const int tile = blockIdx.x % d.tiles, g = (blockIdx.x / d.tiles) % d.NG, s = blockIdx.x / d.tiles / d.NG;
    const int k0 = tile * TRK_N;
    int acc = 0;
    for (int f = 0; f < d.F; ++f) {
        const size_t sf = (size_t)s * d.F + f, row0 = sf * d.cap;
        const int ng = w.nvg[sf], nt = w.nvt[sf];
        const int slot = hota_slot_of(w.cgid + row0, ng, g, lane);
        if (slot < 0 || nt == 0) continue;            // wave-uniform
        slot_of[lane] = -1;
        __syncthreads();
        if (lane < nt) {
            const int r = w.ctid[row0 + lane] - k0;
            if (r >= 0 && r < TRK_N) slot_of[r] = lane;
        }
        __syncthreads();
        const int so = slot_of[lane];                 // the next frame's clear of this entry is this lane's own, behind this read
        if (so >= 0 && w.sim[(row0 + slot) * d.cap + so] >= thr) ++acc;
    }
    const int k = k0 + lane;
    if (k < d.NT) w.pmc[(size_t)s * d.NG * d.NT + (d.tr ? (size_t)k * d.NG + g : (size_t)g * d.NT + k)] = acc;
}

struct MotWideLds {
    long long u[MOT_MAX_IDS], v[MOT_MAX_IDS], minv[MOT_MAX_IDS];   // row and column potentials; the column's distance on this augmentation
    short way[MOT_MAX_IDS], row[MOT_MAX_IDS];        // the column before this one on the path (-1: the virtual start column); the row assigned to the column
    unsigned char used[MOT_MAX_IDS];
    long long red_v[MOT_WG / TRK_N];
    int red_j[MOT_WG / TRK_N];
};

// (v, j) -> the workgroup's lexicographic minimum, in every thread; red_* may be written again after the caller's next barrier
__device__ __forceinline__ void mot_wg_argmin(long long &v, int &j, MotWideLds &L, int t) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const long long ov = __shfl_xor(v, off);
        const int oj = __shfl_xor(j, off);
        if (ov < v || (ov == v && oj < j)) {
            v = ov;
            j = oj;
        }
    }
    if ((t & (TRK_N - 1)) == 0) {
        L.red_v[t / TRK_N] = v;
        L.red_j[t / TRK_N] = j;
    }
    __syncthreads();
    v = L.red_v[0];
    j = L.red_j[0];
#pragma unroll
    for (int k = 1; k < MOT_WG / TRK_N; ++k) {
        const long long ov = L.red_v[k];
        const int oj = L.red_j[k];
        if (ov < v || (ov == v && oj < j)) {
            v = ov;
            j = oj;
        }
    }
}

__global__ __launch_bounds__(MOT_WG) void mot_wide_kernel(const MotDims d, const MotWs w) {
    __shared__ MotWideLds L;
    const int t = threadIdx.x, s = blockIdx.x;
    const int ns = d.tr ? d.NT : d.NG, nb = d.tr ? d.NG : d.NT;     // ns <= nb <= MOT_MAX_IDS (checked by the host)
    const int32_t *W = w.pmc + (size_t)s * d.NG * d.NT;              // [ns][nb]
    for (int j = t; j < nb; j += MOT_WG) {
        L.v[j] = 0;
        L.row[j] = -1;
    }
    for (int i = t; i < ns; i += MOT_WG) L.u[i] = 0;
    __syncthreads();
    for (int i = 0; i < ns; ++i) {                    // <= rows augmentations
        int any = 0;                                  // a row without a positive entry (an id of the padding, an id that never met the other side) adds 0
        for (int j = t; j < nb; j += MOT_WG) any |= W[(size_t)i * nb + j] > 0;     // wherever it goes: it stays unassigned, the matching is partial
        if (!__syncthreads_or(any)) continue;         // workgroup-uniform
        for (int j = t; j < nb; j += MOT_WG) {
            L.minv[j] = MOT_HUGE;
            L.way[j] = -1;
            L.used[j] = 0;
        }
        __syncthreads();
        int j0 = -1, i0 = i;
        bool found = false;
        for (int it = 0; it <= nb; ++it) {            // <= cols + 1 columns are visited
            const long long ui0 = L.u[i0];
            const int32_t *Wr = W + (size_t)i0 * nb;
            long long best = MOT_HUGE;
            int j1 = nb;
            for (int j = t; j < nb; j += MOT_WG) {    // a thread's columns ascend: < keeps its lowest
                if (j == j0) L.used[j] = 1;
                if (L.used[j]) continue;
                const long long cur = -(long long)Wr[j] - ui0 - L.v[j];
                long long mv = L.minv[j];
                if (cur < mv) {
                    mv = cur;
                    L.minv[j] = cur;
                    L.way[j] = (short)j0;
                }
                if (mv < best) {
                    best = mv;
                    j1 = j;
                }
            }
            mot_wg_argmin(best, j1, L, t);
            if (j1 >= nb) break;                      // no open column: cannot happen with rows <= columns
            const long long delta = best;
            for (int j = t; j < nb; j += MOT_WG) {
                if (L.used[j]) {
                    const int r = L.row[j];           // a used column holds a row; distinct columns hold distinct rows, none of them row i
                    if (r >= 0) L.u[r] += delta;
                    L.v[j] -= delta;
                } else {
                    L.minv[j] -= delta;
                }
            }
            if (t == 0) L.u[i] += delta;              // the virtual column's row
            __syncthreads();
            j0 = j1;
            const int pj = L.row[j0];
            if (pj < 0) {
                found = true;
                break;
            }
            i0 = pj;
        }
        if (found && t == 0)
            for (int it = 0; it <= nb && j0 >= 0; ++it) {   // flip the path back to the virtual column
                const int jp = L.way[j0];
                L.row[j0] = jp >= 0 ? L.row[jp] : (short)i;
                j0 = jp;
            }
        __syncthreads();
    }
    long long sum = 0;
    for (int j = t; j < nb; j += MOT_WG) {
        const int r = L.row[j];
        if (r >= 0) sum += W[(size_t)r * nb + j];
    }
    sum = hota_wave_sum(sum);
    __syncthreads();
    if ((t & (TRK_N - 1)) == 0) L.red_v[t / TRK_N] = sum;
    __syncthreads();
    if (t == 0) {
        long long all = 0;
        for (int k = 0; k < MOT_WG / TRK_N; ++k) all += L.red_v[k];
        w.seq_i[(size_t)s * 8 + 4] = (int32_t)all;
    }
}

__global__ __launch_bounds__(TRK_N) void mot_reduce_kernel(const MotDims d, const MotWs w, int32_t *out_i, double *out_f) {
    const int lane = threadIdx.x, s = blockIdx.x;
    const size_t id0 = (size_t)s * d.NG;
    long long mt = 0, ptp = 0, seen = 0, frag = 0, n_gt = 0, n_trk = 0;
    for (int g = lane; g < d.NG; g += TRK_N) {
        const long long pr = w.present[id0 + g], ma = w.matched[id0 + g], st = w.starts[id0 + g];
        if (pr <= 0) continue;                        // an id of the padding, or one that never occurs
        seen += 1;
        mt += 5 * ma > 4 * pr;
        ptp += 5 * ma >= pr;
        frag += st > 1 ? st - 1 : 0;
    }
    for (int f = lane; f < d.F; f += TRK_N) {
        n_gt += w.nvg[(size_t)s * d.F + f];
        n_trk += w.nvt[(size_t)s * d.F + f];
    }
    mt = hota_wave_sum(mt);
    ptp = hota_wave_sum(ptp);
    seen = hota_wave_sum(seen);
    frag = hota_wave_sum(frag);
    n_gt = hota_wave_sum(n_gt);
    n_trk = hota_wave_sum(n_trk);
    if (lane == 0) {
        const int32_t *q = w.seq_i + (size_t)s * 8;
        const long long idtp = d.NG > 0 && d.NT > 0 ? q[4] : 0;      // without ids on one side kernels 3 and 4 did not run
        int32_t *o = out_i + (size_t)s * 11;
        o[0] = q[0];
        o[1] = q[1];
        o[2] = q[2];
        o[3] = q[3];
        o[4] = (int32_t)mt;
        o[5] = (int32_t)(ptp - mt);
        o[6] = (int32_t)(seen - ptp);
        o[7] = (int32_t)frag;
        o[8] = (int32_t)idtp;
        o[9] = (int32_t)(n_gt - idtp);
        o[10] = (int32_t)(n_trk - idtp);
        out_f[s] = w.seq_f[s];
    }
}

// the workspace: byte offset of each buffer (16-byte aligned) and the total; false on a size out of range, an id space beyond the cap or an overflow
static bool mot_layout(int S, int F, int cap, int NG, int NT, size_t off[MOT_NBUF], size_t *total) {
    if (S < 0 || F < 1 || cap < 1 || cap > TRK_N || NG < 0 || NT < 0 || NG > MOT_MAX_IDS || NT > MOT_MAX_IDS) return false;
    const size_t dims[MOT_NBUF][5] = {
        {8, (size_t)S, (size_t)F, (size_t)cap, (size_t)cap}, {8, (size_t)S, 1, 1, 1},
        {4, (size_t)S, (size_t)NG, (size_t)NT, 1},           {4, (size_t)S, (size_t)F, (size_t)cap, 1},
        {4, (size_t)S, (size_t)F, (size_t)cap, 1},           {4, (size_t)S, (size_t)F, 1, 1},
        {4, (size_t)S, (size_t)F, 1, 1},                     {4, (size_t)S, (size_t)NG, 1, 1},
        {4, (size_t)S, (size_t)NG, 1, 1},                    {4, (size_t)S, (size_t)NG, 1, 1},
        {4, (size_t)S, (size_t)NG, 1, 1},                    {4, (size_t)S, (size_t)NG, 1, 1},
        {4, (size_t)S, 8, 1, 1},
    };
    size_t at = 0;
    for (int b = 0; b < MOT_NBUF; ++b) {
        size_t bytes = 1;
        for (int k = 0; k < 5; ++k)
            if (__builtin_mul_overflow(bytes, dims[b][k], &bytes)) return false;
        off[b] = at;
        if (__builtin_add_overflow(bytes, (size_t)15, &bytes)) return false;
        if (__builtin_add_overflow(at, bytes & ~(size_t)15, &at)) return false;
    }
    *total = at > 16 ? at : 16;
    return true;
}

extern "C" size_t v2x_mot_workspace_size(int n_seq, int n_frames, int cap, int n_gt_ids, int n_trk_ids) {
    size_t off[MOT_NBUF], total = 0;
    return mot_layout(n_seq, n_frames, cap, n_gt_ids, n_trk_ids, off, &total) ? total : 0;
}

extern "C" int v2x_mot_sequences(const float *gt_boxes, const int32_t *gt_ids, const int32_t *gt_count, const float *trk_boxes, const int32_t *trk_ids,
                                 const int32_t *trk_count, int n_seq, int n_frames, int cap, int n_gt_ids, int n_trk_ids, double thr, void *workspace,
                                 size_t workspace_bytes, int32_t *out_i, double *out_f, v2x_stream_t stream) {
    V2X_REQUIRE(gt_boxes && gt_ids && gt_count && trk_boxes && trk_ids && trk_count && workspace && out_i && out_f, "v2x_mot_sequences: null pointer");
    V2X_REQUIRE(n_seq >= 0 && n_frames >= 1, "v2x_mot_sequences: n_seq = %d, n_frames = %d", n_seq, n_frames);
    V2X_REQUIRE(cap >= 1 && cap <= TRK_N, "v2x_mot_sequences: cap = %d outside [1, 64] (one wave per frame)", cap);
    V2X_REQUIRE(n_gt_ids >= 0 && n_trk_ids >= 0, "v2x_mot_sequences: n_gt_ids = %d, n_trk_ids = %d must not be negative", n_gt_ids, n_trk_ids);
    V2X_REQUIRE(n_gt_ids <= MOT_MAX_IDS && n_trk_ids <= MOT_MAX_IDS, "v2x_mot_sequences: n_gt_ids = %d, n_trk_ids = %d beyond the id cap %d", n_gt_ids, n_trk_ids,
                MOT_MAX_IDS);
    V2X_REQUIRE(fabs(thr) <= DBL_MAX, "v2x_mot_sequences: thr is not finite");
    size_t off[MOT_NBUF], total = 0;
    V2X_REQUIRE(mot_layout(n_seq, n_frames, cap, n_gt_ids, n_trk_ids, off, &total), "v2x_mot_sequences: the workspace size overflows");
    V2X_REQUIRE(workspace_bytes >= total, "v2x_mot_sequences: workspace of %zu bytes, v2x_mot_workspace_size asks for %zu", workspace_bytes, total);
    const long long tiles = ((long long)n_trk_ids + TRK_N - 1) / TRK_N, grid_max = 1ll << 24;    // grids stay far below 2^32 threads
    V2X_REQUIRE((long long)n_seq * n_frames <= grid_max && (long long)n_seq * n_gt_ids * tiles <= grid_max,
                "v2x_mot_sequences: n_seq x n_frames and n_seq x n_gt_ids x ceil(n_trk_ids / 64) must not exceed 2^24");
    V2X_REQUIRE(((reinterpret_cast<uintptr_t>(gt_boxes) | reinterpret_cast<uintptr_t>(trk_boxes) | reinterpret_cast<uintptr_t>(workspace)) & 15) == 0,
                "v2x_mot_sequences: gt_boxes, trk_boxes and workspace must be 16-byte aligned");
    if (n_seq == 0) return V2X_OK;
    char *base = static_cast<char *>(workspace);
    MotWs w;
    w.sim = reinterpret_cast<double *>(base + off[0]);
    w.seq_f = reinterpret_cast<double *>(base + off[1]);
    w.pmc = reinterpret_cast<int32_t *>(base + off[2]);
    w.cgid = reinterpret_cast<int32_t *>(base + off[3]);
    w.ctid = reinterpret_cast<int32_t *>(base + off[4]);
    w.nvg = reinterpret_cast<int32_t *>(base + off[5]);
    w.nvt = reinterpret_cast<int32_t *>(base + off[6]);
    w.prev = reinterpret_cast<int32_t *>(base + off[7]);
    w.lastf = reinterpret_cast<int32_t *>(base + off[8]);
    w.present = reinterpret_cast<int32_t *>(base + off[9]);
    w.matched = reinterpret_cast<int32_t *>(base + off[10]);
    w.starts = reinterpret_cast<int32_t *>(base + off[11]);
    w.seq_i = reinterpret_cast<int32_t *>(base + off[12]);
    const MotDims d = {n_seq, n_frames, cap, n_gt_ids, n_trk_ids, (int)tiles, n_gt_ids > n_trk_ids ? 1 : 0};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 frames(n_seq * n_frames), seqs(n_seq), ids(n_seq * n_gt_ids * (int)tiles), wave(TRK_N);
    hipLaunchKernelGGL(mot_sim_kernel, frames, wave, 0, st, gt_boxes, gt_ids, gt_count, trk_boxes, trk_ids, trk_count, d, w);
    V2X_CHECK_LAUNCH("mot_sim_kernel");
    hipLaunchKernelGGL(mot_clear_kernel, seqs, wave, 0, st, thr, d, w);
    V2X_CHECK_LAUNCH("mot_clear_kernel");
    if (ids.x > 0) {                                  // no ground-truth id or no track id: IDTP = 0, kernel 5 does not read it
        hipLaunchKernelGGL(mot_pmc_kernel, ids, wave, 0, st, thr, d, w);
        V2X_CHECK_LAUNCH("mot_pmc_kernel");
        hipLaunchKernelGGL(mot_wide_kernel, seqs, dim3(MOT_WG), 0, st, d, w);
        V2X_CHECK_LAUNCH("mot_wide_kernel");
    }
    hipLaunchKernelGGL(mot_reduce_kernel, seqs, wave, 0, st, d, w, out_i, out_f);
    V2X_CHECK_LAUNCH("mot_reduce_kernel");
    return V2X_OK;
}

// The one-wave optimal assignment of row f-5, shared by track.hip (SORT's association, v2x_assign_iou) and hota.hip (the HOTA metric's per-frame
// matching): the LDS block of a wave, the wave-wide lexicographic minimum and the shortest-augmenting-path assignment in fp64.  Moved here
// verbatim from track.hip; the description of the method is at the head of that file.
#pragma once
#include "common.h"

#define TRK_N 64                 // wave width = the capacity of tracks, detections, rows and columns
#define TRK_HUGE 1.0e300

struct TrkLds {
    double M[TRK_N * TRK_N];     // [small][large] IoU (also the compaction scratch of the predict phase, before the matrix exists)
    double u[TRK_N];             // row potentials
    float4 dbox[TRK_N], pbox[TRK_N], z[TRK_N];
    int d2t[TRK_N], t2d[TRK_N], birth[TRK_N];
};

__device__ __forceinline__ unsigned long long trk_lt_mask(int lane) { return (1ull << lane) - 1ull; }

// (v, idx) -> the wave's lexicographic minimum, in every lane
__device__ __forceinline__ void trk_wave_argmin(double &v, int &idx) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(idx, off);
        if (ov < v || (ov == v && oi < idx)) {
            v = ov;
            idx = oi;
        }
    }
}

// max-sum assignment of ns rows to nb >= ns columns (lane = column): min-cost on -M.  Returns the row assigned to the lane's column, or -1.
__device__ int trk_assign(const double *M, double *u, int ns, int nb, int lane) {
    double v = 0.0;              // the column's potential
    int p = -1;                  // the row assigned to the column
    u[lane] = 0.0;
    __syncthreads();
    for (int i = 0; i < ns; ++i) {                    // <= rows augmentations
        double minv = TRK_HUGE;
        int way = -1;            // the column before this one on the path (-1: the virtual start column, which holds row i)
        bool used = false;
        int j0 = -1, i0 = i;
        bool found = false;
        for (int it = 0; it <= nb; ++it) {            // <= cols + 1 columns are visited
            if (lane == j0) used = true;
            const bool open = lane < nb && !used;
            const double ui0 = u[i0];
            double key = TRK_HUGE;
            if (open) {
                const double cur = -M[i0 * TRK_N + lane] - ui0 - v;
                if (cur < minv) {
                    minv = cur;
                    way = j0;
                }
                key = minv;
            }
            int j1 = open ? lane : TRK_N;
            double delta = key;
            trk_wave_argmin(delta, j1);
            if (j1 >= nb) break;                      // no open column: cannot happen with rows <= columns
            __syncthreads();
            if (used && p >= 0) {
                u[p] += delta;                        // distinct rows: the used columns hold distinct rows, none of them row i
                v -= delta;
            } else if (lane < nb) {
                minv -= delta;
            }
            if (lane == 0) u[i] += delta;             // the virtual column's row
            __syncthreads();
            j0 = j1;
            const int pj = __shfl(p, j0);
            if (pj < 0) {
                found = true;
                break;
            }
            i0 = pj;
        }
        if (!found) continue;
        for (int it = 0; it <= nb && j0 >= 0; ++it) { // flip the path back to the virtual column
            const int j1 = __shfl(way, j0);
            const int pprev = __shfl(p, j1 & (TRK_N - 1));
            if (lane == j0) p = j1 >= 0 ? pprev : i;
            j0 = j1;
        }
    }
    return p;
}

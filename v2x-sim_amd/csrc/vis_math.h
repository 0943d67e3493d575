// The free-space ray walk of DESIGN.md section 3.13 (row f-2 "visibility maps"): ONE definition, compiled for the device by lidar_vis.hip (both of its
// kernel forms) and for the host by tests/vis_driver.cpp, which tests/test_vis_refs_cpu.py holds against the float64 reference of tests/vis_refs.py
// byte for byte.  Plain C++ outside hipcc (no HIP type).  Every fp64 operation below is rounded on its own: the including object is built with
// -ffp-contract=off, and nothing here may be rewritten as an fma.
//
// The ray is the pair of fp64 grid coordinates q_o, q_p (voxel faces are the integers, the grid is the box [0,X] x [0,Y] x [0,Z]); with d = q_p - q_o
// a point of it is q_o + t d, t in [0, 1].  The walk is three nested, independent steps:
//   clip     [t0, t1] = [0, 1] cut by the three slabs: per axis with d != 0 the pair (0 - o) / d, (D - o) / d, the smaller one raising t0, the larger one
//            lowering t1; an axis with d == 0 only asks 0 <= o <= D.  t0 > t1: the ray never meets the box.
//   rows     x(t0), x(t1) (each o.x + t * d.x: one product, one sum) give the x rows floor(min) .. floor(max), clamped to [0, X-1].  Row i owns the
//            parameter range [max(t0, t_in), min(t1, t_out)], t_in / t_out = (face - o.x) / d.x for its two faces i, i + 1 in the ray's direction --
//            each computed from its lattice index, never from the previous one.  d.x == 0: the one row keeps [t0, t1].  An empty range skips the row.
//   columns  inside a row the same with y; the column's range [u_a, u_b] gives z(u_a), z(u_b), and the z bits floor(min) .. floor(max), clamped to
//            [0, Z-1], are the column's mask: one OR.
// Ties follow from that without a special case: voxels are CLOSED -- a ray that touches a face, an edge or a corner (in exact arithmetic: a coordinate
// that is an integer) sets the voxels on both sides of it where they exist in the grid; a ray inside a face plane sets the side floor() names (the
// upper one; on the grid's last face the clamp gives the last voxel).  A row depends on nothing but (q_o, q_p, i): a caller that owns only the rows
// [row0, row1) walks exactly the columns the whole walk has there (the banded LDS kernel).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define V2X_VIS_FN __host__ __device__ __forceinline__
#else
#define V2X_VIS_FN static inline
#endif

struct VisGrid {
    double vs[3], inv[3], mn[3];   // voxel size, its exact reciprocal where pow2, floor(lo / vs): a1's quotient (voxelize.hip: vox_quot)
    int pow2[3];
    int X, Y, Z;
};

// host side: the fields of one axis from the voxel size and the lower extent, as v2x_voxelize_bits sets them
static inline void vis_grid_axis(VisGrid &g, int a, double vs, double lo) {
    int e = 0;
    const double m = frexp(vs, &e);
    g.vs[a] = vs;
    g.pow2[a] = (m == 0.5 && e > -1000 && e < 1000) ? 1 : 0;
    g.inv[a] = g.pow2[a] ? 1.0 / vs : 0.0;
    g.mn[a] = floor(lo / vs);
}

// ((x*m0 + y*m1) + z*m2) + m3 in fp32, every operation rounded on its own (the fused voxeliser's arithmetic)
V2X_VIS_FN float vis_move_row(float x, float y, float z, const float *m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(x, m[0]), __fmul_rn(y, m[1])), __fmul_rn(z, m[2])), m[3]);
#else
    volatile float a = x * m[0], b = y * m[1], c = z * m[2];
    volatile float s = a + b;
    volatile float u = s + c;
    return u + m[3];
#endif
}

// moved fp32 coordinate -> fp64 grid coordinate on axis k
V2X_VIS_FN double vis_quot(float c, const VisGrid &g, int k) {
    const double p = (double)c;
    return (g.pow2[k] ? p * g.inv[k] : p / g.vs[k]) - g.mn[k];
}

V2X_VIS_FN bool vis_finite(double v) { return v - v == 0.0; }

// one slab of the clip; false: the ray misses the box on this axis alone
V2X_VIS_FN bool vis_slab(double o, double d, double D, double &t0, double &t1) {
    if (d == 0.0) return o >= 0.0 && o <= D;
    double ta = (0.0 - o) / d, tb = (D - o) / d;
    if (d < 0.0) {
        const double s = ta;
        ta = tb;
        tb = s;
    }
    if (ta > t0) t0 = ta;
    if (tb < t1) t1 = tb;
    return true;
}

V2X_VIS_FN int vis_cell(double v, int D) {
    const double f = floor(v);
    if (!(f > 0.0)) return 0;
    if (f > (double)(D - 1)) return D - 1;
    return (int)f;
}

// the parameter range of lattice cell i on one axis, cut into [ta, tb]
V2X_VIS_FN void vis_cell_range(double o, double d, int i, double &ta, double &tb) {
    if (d == 0.0) return;
    const double lo = ((double)i - o) / d, hi = ((double)(i + 1) - o) / d;
    const double t_in = d > 0.0 ? lo : hi, t_out = d > 0.0 ? hi : lo;
    if (t_in > ta) ta = t_in;
    if (t_out < tb) tb = t_out;
}

// Walks the ray q_o -> q_p over the rows [row0, row1) of an X x Y x Z grid; emit(ix, iy, mask) once per column it crosses there.
template <class Emit>
V2X_VIS_FN void vis_walk(int X, int Y, int Z, const double *o, const double *p, int row0, int row1, Emit &&emit) {
    if (!(vis_finite(o[0]) && vis_finite(o[1]) && vis_finite(o[2]) && vis_finite(p[0]) && vis_finite(p[1]) && vis_finite(p[2]))) return;
    const double dx = p[0] - o[0], dy = p[1] - o[1], dz = p[2] - o[2];
    if (dx == 0.0 && dy == 0.0 && dz == 0.0) return;
    double t0 = 0.0, t1 = 1.0;
    if (!vis_slab(o[0], dx, (double)X, t0, t1) || !vis_slab(o[1], dy, (double)Y, t0, t1) || !vis_slab(o[2], dz, (double)Z, t0, t1)) return;
    if (t0 > t1) return;
    const double xa = o[0] + t0 * dx, xb = o[0] + t1 * dx;
    int ix_lo = vis_cell(xa < xb ? xa : xb, X), ix_hi = vis_cell(xa < xb ? xb : xa, X);
    if (ix_lo < row0) ix_lo = row0;
    if (ix_hi > row1 - 1) ix_hi = row1 - 1;
    for (int ix = ix_lo; ix <= ix_hi; ++ix) {
        double ta = t0, tb = t1;
        vis_cell_range(o[0], dx, ix, ta, tb);
        if (ta > tb) continue;
        const double ya = o[1] + ta * dy, yb = o[1] + tb * dy;
        const int iy_lo = vis_cell(ya < yb ? ya : yb, Y), iy_hi = vis_cell(ya < yb ? yb : ya, Y);
        for (int iy = iy_lo; iy <= iy_hi; ++iy) {
            double ua = ta, ub = tb;
            vis_cell_range(o[1], dy, iy, ua, ub);
            if (ua > ub) continue;
            const double za = o[2] + ua * dz, zb = o[2] + ub * dz;
            const int k_lo = vis_cell(za < zb ? za : zb, Z), k_hi = vis_cell(za < zb ? zb : za, Z);
            emit(ix, iy, (2u << k_hi) - (1u << k_lo));
        }
    }
}

// A job's ray r: the moved origin and endpoint as grid coordinates.  m: the job's 3x4 transform or NULL (identity); org: its origin or NULL (zero).
V2X_VIS_FN void vis_ray(const VisGrid &g, const float *pt, const float *org, const float *m, double *qo, double *qp) {
    const float ox = org ? org[0] : 0.f, oy = org ? org[1] : 0.f, oz = org ? org[2] : 0.f;
    for (int k = 0; k < 3; ++k) {
        const float a = m ? vis_move_row(ox, oy, oz, m + 4 * k) : (k == 0 ? ox : k == 1 ? oy : oz);
        const float b = m ? vis_move_row(pt[0], pt[1], pt[2], m + 4 * k) : pt[k];
        qo[k] = vis_quot(a, g, k);
        qp[k] = vis_quot(b, g, k);
    }
}

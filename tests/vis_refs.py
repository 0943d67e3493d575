"""References of the free-space ray walk (v2x-sim_amd/csrc/vis_math.h) and the case table its tests share.

  freespace_ref(case)   the frozen rule in float64 numpy, vectorised over rays, the same operations in the same order: the bytes every form must give.
  exact_sets(...)       the exact statement in fractions.Fraction with DELTA = 2^-30 grid units: per ray, the voxels it MUST set (the closed segment
                        meets the closed cube shrunk by DELTA on every side) and the voxels it MAY set (it meets the cube grown by DELTA).
  CASES                 the table; cases(), by name.

DELTA is derived, not tuned: |q| stays below 2^10, so an fp64 ulp is at most 2^-43; a crossing computed directly from its lattice index costs about
ten operations, which puts the error below 2^-39; DELTA leaves a factor of 2^9 over that."""
import math
from fractions import Fraction

import numpy as np

DELTA = Fraction(1, 1 << 30)


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
class Grid:
    """voxel sizes, extents -> dims (ops.VoxelGrid's formula), a1's quotient per axis."""

    def __init__(self, voxel, extents):
        self.voxel = tuple(float(v) for v in voxel)
        self.extents = tuple((float(lo), float(hi)) for lo, hi in extents)
        self.dims = tuple(int(math.ceil(hi / v) - 1 - math.floor(lo / v) + 1) for (lo, hi), v in zip(self.extents, self.voxel))
        self.mn = tuple(float(math.floor(lo / v)) for (lo, _), v in zip(self.extents, self.voxel))
        self.pow2 = tuple(math.frexp(v)[0] == 0.5 for v in self.voxel)

    def raw_quot(self, c, k):
        """a1's quotient of fp32 coordinates (array) on axis k: the product with the exact reciprocal of a power-of-two voxel size, else the division"""
        p = np.asarray(c, np.float32).astype(np.float64)
        with np.errstate(all="ignore"):
            return p * (1.0 / self.voxel[k]) if self.pow2[k] else p / self.voxel[k]

    def quot(self, c, k):
        """moved fp32 coordinates (array) of axis k -> fp64 grid coordinates"""
        with np.errstate(all="ignore"):
            return self.raw_quot(c, k) - self.mn[k]

    def world(self, q):
        """grid coordinates -> the fp32 world coordinates the case stores (exact for the power-of-two grids the tie cases use)"""
        q = np.asarray(q, np.float64)
        return ((q + np.asarray(self.mn)) * np.asarray(self.voxel)).astype(np.float32)


def move_f32(m, v):
    """((x*m0 + y*m1) + z*m2) + m3 per row of the 3x4 m, fp32, every operation rounded on its own.  v: (n, 3) -> (n, 3)"""
    m = np.asarray(m, np.float32).reshape(3, 4)
    v = np.asarray(v, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.stack([((v[:, 0] * m[r, 0] + v[:, 1] * m[r, 1]) + v[:, 2] * m[r, 2]) + m[r, 3] for r in range(3)], 1).astype(np.float32)


class Case:
    """One call of v2x_lidar_freespace_bits.  origin / xform / (src, dst) may be None as in the C ABI."""

    def __init__(self, name, grid, pts, n_pts, origin=None, xform=None, src=None, dst=None, n_grids=None, ties=None, exact=False):
        self.name, self.grid = name, grid
        self.pts = np.ascontiguousarray(pts, np.float32)
        assert self.pts.ndim == 3 and self.pts.shape[2] >= 3
        self.n_pts = np.ascontiguousarray(n_pts, np.int32)
        self.n_jobs = self.pts.shape[0] if src is None else len(src)
        self.origin = None if origin is None else np.ascontiguousarray(origin, np.float32).reshape(self.n_jobs, 3)
        self.xform = None if xform is None else np.ascontiguousarray(xform, np.float32).reshape(self.n_jobs, 3, 4)
        self.src = None if src is None else np.ascontiguousarray(src, np.int32)
        self.dst = None if dst is None else np.ascontiguousarray(dst, np.int32)
        self.n_grids = int(self.pts.shape[0] if n_grids is None else n_grids)
        self.ties = ties          # tie cases: one bool per job, True where the exact statement must leave a choice (allowed != required)
        self.exact = exact        # seeded random cases on the small grids: required == allowed is asserted

    def jobs(self):
        """-> [(grid index, q_o (n, 3), q_p (n, 3))] of the jobs that are not skipped, rays past min(n_pts, max_pts) left out"""
        out = []
        n_clouds, max_pts = self.pts.shape[:2]
        for j in range(self.n_jobs):
            c = j if self.src is None else int(self.src[j])
            g = j if self.dst is None else int(self.dst[j])
            if not (0 <= c < n_clouds and 0 <= g < self.n_grids):
                continue
            n = max(min(int(self.n_pts[c]), max_pts), 0)
            p = self.pts[c, :n, :3]
            o = np.zeros((1, 3), np.float32) if self.origin is None else self.origin[j:j + 1]
            if self.xform is not None:
                p, o = move_f32(self.xform[j], p), move_f32(self.xform[j], o)
            qp = np.stack([self.grid.quot(p[:, k], k) for k in range(3)], 1)
            qo = np.stack([self.grid.quot(np.broadcast_to(o[:, k], (n,)), k) for k in range(3)], 1)
            out.append((g, qo, qp))
        return out


# ---- the frozen rule in float64 ------------------------------------------------------------------------------------------------------------
def _cell(v, D):
    f = np.floor(v)
    return np.where(~(f > 0.0), 0.0, np.where(f > D - 1, D - 1.0, f)).astype(np.int64)


def _cell_range(o, d, i, ta, tb):
    nz = d != 0.0
    with np.errstate(all="ignore"):
        lo, hi = (i.astype(np.float64) - o) / d, ((i + 1).astype(np.float64) - o) / d
    t_in, t_out = np.where(d > 0.0, lo, hi), np.where(d > 0.0, hi, lo)
    return np.where(nz & (t_in > ta), t_in, ta), np.where(nz & (t_out < tb), t_out, tb)


def walk_ref(dims, qo, qp, bits):
    """ORs the voxels of the rays q_o -> q_p ((n, 3) float64 each) into bits (X, Y) uint32."""
    X, Y, Z = dims
    qo, qp = np.asarray(qo, np.float64).reshape(-1, 3), np.asarray(qp, np.float64).reshape(-1, 3)
    keep = np.isfinite(qo).all(1) & np.isfinite(qp).all(1)
    qo, qp = qo[keep], qp[keep]
    d = qp - qo
    keep = (d != 0.0).any(1)
    qo, d = qo[keep], d[keep]
    t0, t1, ok = np.zeros(len(d)), np.ones(len(d)), np.ones(len(d), bool)
    for k, D in enumerate((X, Y, Z)):
        o, dk = qo[:, k], d[:, k]
        z = dk == 0.0
        ok &= np.where(z, (o >= 0.0) & (o <= D), True)
        with np.errstate(all="ignore"):
            ta, tb = (0.0 - o) / dk, (float(D) - o) / dk
        ta, tb = np.where(dk < 0.0, tb, ta), np.where(dk < 0.0, ta, tb)
        t0, t1 = np.where(~z & (ta > t0), ta, t0), np.where(~z & (tb < t1), tb, t1)
    ok &= ~(t0 > t1)
    qo, d, t0, t1 = qo[ok], d[ok], t0[ok], t1[ok]
    if not len(d):
        return bits
    xa, xb = qo[:, 0] + t0 * d[:, 0], qo[:, 0] + t1 * d[:, 0]
    ix_lo, ix_hi = _cell(np.where(xa < xb, xa, xb), X), _cell(np.where(xa < xb, xb, xa), X)
    for r in range(int((ix_hi - ix_lo).max()) + 1):
        a = np.nonzero(ix_lo + r <= ix_hi)[0]
        ix = ix_lo[a] + r
        ta, tb = _cell_range(qo[a, 0], d[a, 0], ix, t0[a], t1[a])
        s = ~(ta > tb)
        a, ix, ta, tb = a[s], ix[s], ta[s], tb[s]
        if not len(a):
            continue
        ya, yb = qo[a, 1] + ta * d[a, 1], qo[a, 1] + tb * d[a, 1]
        iy_lo, iy_hi = _cell(np.where(ya < yb, ya, yb), Y), _cell(np.where(ya < yb, yb, ya), Y)
        for c in range(int((iy_hi - iy_lo).max()) + 1):
            b = np.nonzero(iy_lo + c <= iy_hi)[0]
            iy = iy_lo[b] + c
            ua, ub = _cell_range(qo[a[b], 1], d[a[b], 1], iy, ta[b], tb[b])
            s = ~(ua > ub)
            b, iy, ua, ub = b[s], iy[s], ua[s], ub[s]
            if not len(b):
                continue
            za, zb = qo[a[b], 2] + ua * d[a[b], 2], qo[a[b], 2] + ub * d[a[b], 2]
            k_lo, k_hi = _cell(np.where(za < zb, za, zb), Z), _cell(np.where(za < zb, zb, za), Z)
            mask = (((np.uint64(2) << k_hi.astype(np.uint64)) - (np.uint64(1) << k_lo.astype(np.uint64))) & np.uint64(0xffffffff)).astype(np.uint32)
            np.bitwise_or.at(bits, (ix[b], iy), mask)
    return bits


def freespace_ref(case):
    """-> trav_bits (n_grids, X, Y) uint32: the bytes v2x_lidar_freespace_bits must give"""
    X, Y, Z = case.grid.dims
    out = np.zeros((case.n_grids, X, Y), np.uint32)
    for g, qo, qp in case.jobs():
        walk_ref(case.grid.dims, qo, qp, out[g])
    return out


def occ_ref(case):
    """a1's occupancy of the same clouds and jobs (strict lo < p < hi on the moved fp32 coordinate, index floor(quot) - mn) -> (n_grids, X, Y) uint32"""
    X, Y, Z = case.grid.dims
    out = np.zeros((case.n_grids, X, Y), np.uint32)
    n_clouds, max_pts = case.pts.shape[:2]
    for j in range(case.n_jobs):
        c = j if case.src is None else int(case.src[j])
        g = j if case.dst is None else int(case.dst[j])
        if not (0 <= c < n_clouds and 0 <= g < case.n_grids):
            continue
        p = case.pts[c, :max(min(int(case.n_pts[c]), max_pts), 0), :3]
        if case.xform is not None:
            p = move_f32(case.xform[j], p)
        p64 = p.astype(np.float64)
        with np.errstate(all="ignore"):
            keep = np.ones(len(p), bool)
            idx = []
            for k in range(3):
                lo, hi = case.grid.extents[k]
                keep &= (lo < p64[:, k]) & (p64[:, k] < hi)
                idx.append(np.floor(case.grid.raw_quot(p[:, k], k)) - case.grid.mn[k])
        idx = np.stack(idx, 1)[keep].astype(np.int64)
        inb = ((idx >= 0) & (idx < np.asarray(case.grid.dims))).all(1)
        idx = idx[inb]
        np.bitwise_or.at(out[g], (idx[:, 0], idx[:, 1]), (np.uint32(1) << idx[:, 2].astype(np.uint32)))
    return out


def vis_maps_ref(occ, trav, Z, p_occ=0.7, p_free=0.4):
    z = np.arange(Z, dtype=np.uint32)
    o, t = (occ[..., None] >> z) & 1, (trav[..., None] >> z) & 1
    v_occ, v_free = np.float32(math.log(p_occ / (1.0 - p_occ))), np.float32(math.log(p_free / (1.0 - p_free)))
    return np.where(o == 1, v_occ, np.where(t == 1, v_free, np.float32(0.0))).astype(np.float32)


def mask_labels_ref(labels, occ, trav, z_mask=0xffffffff, ignore=255):
    return np.where(((occ | trav) & np.uint32(z_mask)) == 0, np.uint8(ignore), labels).astype(np.uint8)


# ---- the exact statement -------------------------------------------------------------------------------------------------------------------
def _meets(o, d, lo, hi):
    """does the closed segment o + t d, t in [0, 1], meet the closed box [lo, hi] (per-axis Fractions)?"""
    t0, t1 = Fraction(0), Fraction(1)
    for k in range(3):
        if d[k] == 0:
            if not lo[k] <= o[k] <= hi[k]:
                return False
            continue
        ta, tb = (lo[k] - o[k]) / d[k], (hi[k] - o[k]) / d[k]
        if ta > tb:
            ta, tb = tb, ta
        t0, t1 = max(t0, ta), min(t1, tb)
        if t0 > t1:
            return False
    return True


def exact_sets(dims, qo, qp):
    """-> (required, allowed), each (X, Y) uint32, of the rays q_o -> q_p taken as rationals.  A skipped ray (non-finite, zero length) sets nothing."""
    X, Y, Z = dims
    req, alw = np.zeros((X, Y), np.uint32), np.zeros((X, Y), np.uint32)
    for a, b in zip(np.asarray(qo, np.float64).reshape(-1, 3), np.asarray(qp, np.float64).reshape(-1, 3)):
        if not (np.isfinite(a).all() and np.isfinite(b).all()) or (a == b).all():
            continue
        o = [Fraction(float(v)) for v in a]
        d = [Fraction(float(v)) - w for v, w in zip(b, o)]
        rng = [range(max(int(math.floor(min(a[k], b[k]))) - 1, 0), min(int(math.floor(max(a[k], b[k]))) + 2, D)) for k, D in enumerate(dims)]
        for i in rng[0]:
            for j in rng[1]:
                for k in rng[2]:
                    c = (i, j, k)
                    if _meets(o, d, [Fraction(v) - DELTA for v in c], [Fraction(v + 1) + DELTA for v in c]):
                        alw[i, j] |= np.uint32(1 << k)
                        if _meets(o, d, [Fraction(v) + DELTA for v in c], [Fraction(v + 1) - DELTA for v in c]):
                            req[i, j] |= np.uint32(1 << k)
    return req, alw


def exact_grids(case):
    """-> (required, allowed) (n_grids, X, Y) uint32: the unions over every job's rays"""
    X, Y, Z = case.grid.dims
    req, alw = np.zeros((case.n_grids, X, Y), np.uint32), np.zeros((case.n_grids, X, Y), np.uint32)
    for g, qo, qp in case.jobs():
        r, a = exact_sets(case.grid.dims, qo, qp)
        req[g] |= r
        alw[g] |= a
    return req, alw


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
PRODUCT_VOXEL = (0.25, 0.25, 0.4)
G_UNIT = Grid((1.0, 1.0, 1.0), ((-2.0, 2.0), (-2.0, 2.0), (-1.0, 1.0)))                  # 4 x 4 x 2, faces on integers: ties are exact
G_SMALL = Grid(PRODUCT_VOXEL, ((-1.1, 0.7), (-1.1, 0.7), (-0.9, 0.3)))                    # 8 x 8 x 4, the product's voxel, extents off the faces
G_MID = Grid(PRODUCT_VOXEL, ((-2.1, 1.7), (-2.1, 1.7), (-3.1, 1.9)))                      # 16 x 16 x 13
G_BAND = Grid((0.25, 0.25, 0.25), ((-4.0, 4.0), (-2.5, 2.5), (-2.0, 2.0)))                # 32 x 20 x 16: two row bands of the LDS form
G_TALL = Grid((0.25, 0.25, 0.25), ((-4.0, 4.0), (-4.0, 4.0), (-2.0, 2.25)))               # 32 x 32 x 17: general form, by Z
G_WIDE = Grid(PRODUCT_VOXEL, ((-32.5, 32.5), (-32.0, 32.0), (-3.0, 2.0)))                 # 260 x 256 x 13: general form, by size
G_PRODUCT = Grid(PRODUCT_VOXEL, ((-32.0, 32.0), (-32.0, 32.0), (-3.0, 2.0)))              # 256 x 256 x 13
for _g, _d in ((G_UNIT, (4, 4, 2)), (G_SMALL, (8, 8, 4)), (G_MID, (16, 16, 13)), (G_BAND, (32, 20, 16)), (G_TALL, (32, 32, 17)), (G_WIDE, (260, 256, 13)),
               (G_PRODUCT, (256, 256, 13))):
    assert _g.dims == _d, (_g.dims, _d)

E40 = 2.0 ** -40

# (name, tie, q_o, q_p) in grid coordinates of a power-of-two grid: one ray per job, each into its own grid.  tie: the exact statement leaves a choice.
_UNIT_RAYS = [
    ("along +x", False, (0.5, 1.5, 0.5), (3.5, 1.5, 0.5)),
    ("along -y", False, (1.5, 3.5, 1.5), (1.5, 0.5, 1.5)),
    ("vertical +z", False, (1.5, 1.5, 0.25), (1.5, 1.5, 1.75)),
    ("vertical -z from above the grid", False, (2.5, 0.5, 3.75), (2.5, 0.5, 0.25)),
    ("xy plane", False, (0.25, 0.5, 0.5), (3.75, 2.25, 0.5)),
    ("xz plane", False, (0.25, 1.5, 0.125), (3.75, 1.5, 1.875)),
    ("yz plane", False, (1.5, 3.75, 1.875), (1.5, 0.25, 0.125)),
    ("in the face plane y = 2", True, (0.5, 2.0, 0.5), (3.5, 2.0, 0.5)),
    ("along the edge y = 2, z = 1", True, (0.5, 2.0, 1.0), (3.5, 2.0, 1.0)),
    ("vertical along the edge x = 2, y = 2", True, (2.0, 2.0, 0.25), (2.0, 2.0, 1.75)),
    ("xy diagonal through the corners", True, (0.5, 0.5, 0.5), (3.5, 3.5, 0.5)),
    ("space diagonal corner to corner", True, (0.0, 0.0, 0.0), (4.0, 4.0, 2.0)),
    ("anti-diagonal through (2, 2, 1)", True, (3.5, 0.5, 1.75), (0.5, 3.5, 0.25)),
    ("nearly axis-parallel, off the faces", False, (0.5, 2.0 + 2.0 ** -20, 0.5), (3.5, 2.0 + 2.0 ** -20 + E40, 0.5)),
    ("nearly axis-parallel, across the face y = 2", True, (0.5, 2.0 - E40 / 2, 0.5), (3.5, 2.0 + E40 / 2, 0.5)),
    ("origin on a face", True, (0.0, 1.5, 0.5), (2.5, 2.75, 1.5)),
    ("origin on a corner of the grid", True, (0.0, 0.0, 0.0), (2.25, 1.75, 1.125)),
    ("origin on an inner corner", True, (2.0, 2.0, 1.0), (3.75, 0.25, 0.25)),
    ("origin outside", False, (-1.5, 1.25, 0.5), (2.5, 2.75, 1.5)),
    ("origin above", False, (1.25, 1.75, 3.5), (2.75, 0.5, 0.5)),
    ("endpoint equal to the origin", False, (1.5, 1.5, 0.5), (1.5, 1.5, 0.5)),
    ("endpoint outside", False, (1.5, 1.5, 0.5), (6.5, 3.25, 1.75)),
    ("both outside, through the grid", False, (-1.5, 0.75, 0.25), (5.5, 3.25, 1.75)),
    ("misses the box", False, (-1.5, 0.5, 0.5), (0.5, -1.5, 0.5)),
    ("misses the box above", False, (0.5, 0.5, 2.5), (3.5, 3.5, 2.25)),
    ("grazes an edge of the box", True, (-1.0, 1.0, 0.5), (1.0, -1.0, 0.5)),
    ("grazes a corner of the box", True, (-1.0, 1.0, -0.5), (1.0, -1.0, 0.5)),
    ("in the grid's last face x = 4", True, (4.0, 0.5, 0.5), (4.0, 3.5, 1.5)),
    ("NaN in the point", False, (0.5, 0.5, 0.5), (float("nan"), 1.5, 0.5)),
    ("inf in the point", False, (0.5, 0.5, 0.5), (2.5, float("inf"), 0.5)),
    ("NaN in the origin", False, (0.5, float("nan"), 0.5), (2.5, 1.5, 0.5)),
    ("inf in the origin", False, (float("-inf"), 0.5, 0.5), (2.5, 1.5, 0.5)),
]

_BAND_RAYS = [   # 32 x 20 x 16, the LDS form's band boundary is the face x = 16
    ("shallow across x = 16", False, (15.875, 0.25, 3.5), (16.125, 19.75, 12.5)),
    ("shallow across x = 16, backwards", False, (16.0625, 19.5, 9.25), (15.9375, 0.5, 2.75)),
    ("exactly along x = 16", True, (16.0, 0.5, 4.5), (16.0, 19.5, 11.5)),
    ("along the edge x = 16, z = 8", True, (16.0, 19.5, 8.0), (16.0, 0.5, 8.0)),
    ("through the corner (16, 10)", True, (12.5, 6.5, 7.5), (19.5, 13.5, 7.5)),
    ("from band 0 to band 1, steep", False, (0.5, 9.25, 0.5), (31.5, 10.75, 15.5)),
    ("nearly parallel to x = 16, across it", True, (16.0 - E40 / 2, 0.5, 4.5), (16.0 + E40 / 2, 19.5, 4.5)),
    ("ends on x = 16", True, (3.5, 3.5, 3.5), (16.0, 12.25, 9.5)),
]


def _ray_case(name, grid, rays, stride):
    """one cloud of one point, one origin and one grid per ray"""
    n = len(rays)
    pts = np.full((n, 1, stride), 7.0, np.float32)
    org = np.zeros((n, 3), np.float32)
    for i, (_, _, qo, qp) in enumerate(rays):
        pts[i, 0, :3], org[i] = grid.world(qp), grid.world(qo)
    return Case(name, grid, pts, np.ones(n, np.int32), origin=org, ties=[r[1] for r in rays])


def _yaw_xform(rng, n, shift, tilt=0.0):
    m = np.zeros((n, 3, 4), np.float64)
    for j in range(n):
        a, b = rng.uniform(-math.pi, math.pi), rng.uniform(-tilt, tilt)
        rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
        rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
        m[j, :, :3] = rz @ rx
        m[j, :, 3] = rng.uniform(-1, 1, 3) * np.asarray(shift)
    return m.astype(np.float32)


def _random_case(name, grid, seed, n_clouds, max_pts, stride, n_pts=None, jobs=None, n_grids=None, origin=True, xform=True, spread=1.3, exact=False):
    """points and origins uniform in the grid's box scaled by `spread` about its centre; jobs: (src, dst) lists or None"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(grid.extents).T
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * spread
    pts = np.full((n_clouds, max_pts, stride), 3.0, np.float32)
    pts[..., :3] = rng.uniform(mid - half, mid + half, (n_clouds, max_pts, 3))
    n_jobs = n_clouds if jobs is None else len(jobs[0])
    return Case(name, grid, pts, np.full(n_clouds, max_pts, np.int32) if n_pts is None else n_pts,
                origin=rng.uniform(mid - half, mid + half, (n_jobs, 3)) if origin else None,
                xform=_yaw_xform(rng, n_jobs, half * 0.3, 0.2) if xform else None,
                src=None if jobs is None else jobs[0], dst=None if jobs is None else jobs[1], n_grids=n_grids, exact=exact)


def _ring_case(name, grid, beams, steps, sensor_z=0.0, seed=5):
    """a sweep as the cast gives it: origin None (the zero vector), returns on a ground plane, on walls and at the range limit"""
    rng = np.random.default_rng(seed)
    elev = np.deg2rad(np.linspace(-30.67, 10.67, beams))[:, None]
    az = (np.arange(steps) * (2 * math.pi / steps))[None, :]
    rng_m = np.where(np.sin(elev) < 0, np.minimum((1.8 + sensor_z) / np.maximum(-np.sin(elev), 1e-9), 70.0), 70.0) * np.ones_like(az)
    rng_m = np.minimum(rng_m, rng.uniform(4.0, 90.0, (1, steps)))            # walls at random ranges: occlusion
    p = np.stack([rng_m * np.cos(elev) * np.cos(az), rng_m * np.cos(elev) * np.sin(az), rng_m * np.sin(elev) + sensor_z, np.zeros_like(rng_m)], -1)
    return Case(name, grid, p.reshape(1, beams * steps, 4), np.array([beams * steps], np.int32))


def _build_cases():
    c = [
        _ray_case("unit_ties_stride3", G_UNIT, _UNIT_RAYS, 3),
        _ray_case("band_boundary_stride4", G_BAND, _BAND_RAYS, 4),
        _random_case("unit_random_stride3", G_UNIT, 11, 3, 12, 3, exact=True),
        _random_case("small_random_stride5_n_pts", G_SMALL, 12, 4, 10, 5, n_pts=np.array([10, 0, 15, 7], np.int32), exact=True),
        _random_case("small_five_jobs_one_target", G_SMALL, 13, 3, 6, 4, jobs=([0, 1, 2, 0, 1, 2, 7, -1, 1], [1, 1, 1, 1, 1, 0, 0, 1, 9]), n_grids=2, exact=True),
        # the zero origin is the lattice corner (5, 5, 3) of this grid, as a cast sweep's sensor is a corner of the product grid: every ray starts on a tie
        _random_case("small_no_origin_no_xform", G_SMALL, 14, 3, 8, 4, origin=False, xform=False, n_grids=2),
        _random_case("small_origin_zero_moved", G_SMALL, 15, 2, 8, 4, origin=False, exact=True),
        _random_case("small_no_jobs", G_SMALL, 16, 2, 4, 4, jobs=([], []), n_grids=2, origin=False, xform=False),
        _random_case("small_no_points", G_SMALL, 17, 2, 5, 4, n_pts=np.zeros(2, np.int32)),
        _random_case("mid_two_jobs_one_target", G_MID, 18, 3, 40, 4, jobs=([0, 1, 2], [0, 0, 1]), n_grids=2),
        _random_case("band_random_stride3", G_BAND, 19, 2, 64, 3, spread=1.1),
        _random_case("tall_general_by_z", G_TALL, 20, 2, 64, 4),
        _random_case("wide_general_by_size", G_WIDE, 21, 2, 96, 4, spread=1.05),
        _ring_case("product_ring_8192", G_PRODUCT, 4, 2048),
    ]
    return {k.name: k for k in c}


CASES = _build_cases()
_REF_CACHE = {}


def cases():
    return list(CASES.values())


def reference(name):
    """freespace_ref of a case, computed once and shared; the returned array must not be written"""
    if name not in _REF_CACHE:
        _REF_CACHE[name] = freespace_ref(CASES[name])
        _REF_CACHE[name].setflags(write=False)
    return _REF_CACHE[name]

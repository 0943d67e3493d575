"""Float64 reference, case table and comparison rule for the batched box rasterizer (csrc/seg_raster.hip, DESIGN.md section 3.8 "Box rasterization").

Written independently of the kernel: no tiles, no cull -- every box of an item is evaluated over the whole grid with numpy, in the order of operations the
rule freezes (utils/synthetic_scene.seg_labels' arithmetic), and the boxes are painted in index order under "greatest rank, lowest index on ties".

The reference also returns, per cell, how close its decision is to flipping: `margin` = the smallest of | |lx| - w/2 | and | |ly| - h/2 | over the item's
valid boxes (metres).  Both sides evaluate the same fp64 expressions on the same fp32 inputs; the device's sin / cos may differ from numpy's in the last
place, nothing else may.  A cell whose margin is below RASTER_MARGIN may therefore be left out of a comparison -- in at most MAX_EXCLUDED of a case's
cells, a condition on the case table (tests/test_seg_raster_refs_cpu.py), not a measurement.  The `exact` cases (yaw = 0, coordinates exact in fp32: cos =
1, sin = 0, every product and sum exact) allow no exclusion at all although their margins are 0 by design: the closed border must hold bit for bit.
"""
import functools
import math
from collections import namedtuple

import numpy as np

RASTER_MARGIN = 1e-9         # metres
MAX_EXCLUDED = 1e-4          # of a case's cells
MAX_BOXES = 256
IGNORE = 255


def grid_of(X, Y, cell):
    """(x0, y0, vx, vy, X, Y) of an X x Y grid of `cell`-sized cells centred on the origin; the four reals as the fp32 values the C ABI takes."""
    f = lambda v: float(np.float32(v))
    return (f(-X * cell / 2), f(-Y * cell / 2), f(cell), f(cell), X, Y)


def config_grid(config):
    return (float(np.float32(config.area_extents[0][0])), float(np.float32(config.area_extents[1][0])), float(np.float32(config.voxel_size[0])),
            float(np.float32(config.voxel_size[1])), int(config.map_dims[0]), int(config.map_dims[1]))


def raster_item_ref(boxes, cls, count, grid, n_cls, rank=None):
    """One item.  boxes (cap, 5) fp32, cls (cap,) uint8, count int -> dict(labels (X, Y) uint8, owner (X, Y) int32, hist (n_cls + 1,) int64,
    margin (X, Y) float64; inf where the item has no valid box)."""
    x0, y0, vx, vy, X, Y = grid
    boxes = np.asarray(boxes, np.float32).reshape(-1, 5)
    cls = np.asarray(cls, np.uint8).reshape(-1)
    px = np.float64(x0) + (np.arange(X, dtype=np.float64) + 0.5) * np.float64(vx)
    py = np.float64(y0) + (np.arange(Y, dtype=np.float64) + 0.5) * np.float64(vy)
    labels = np.zeros((X, Y), np.uint8)
    owner = np.full((X, Y), -1, np.int32)
    best = np.full((X, Y), -1, np.int64)
    margin = np.full((X, Y), np.inf, np.float64)
    for g in range(min(max(int(count), 0), boxes.shape[0])):
        b = boxes[g].astype(np.float64)
        if not np.isfinite(b).all() or b[2] < 0 or b[3] < 0:
            continue
        ex, ey = (px - b[0])[:, None], (py - b[1])[None, :]
        c, s = math.cos(b[4]), math.sin(b[4])
        lx = ex * c + ey * s
        ly = -ex * s + ey * c
        hw, hh = b[2] / 2, b[3] / 2
        margin = np.minimum(margin, np.minimum(np.abs(np.abs(lx) - hw), np.abs(np.abs(ly) - hh)))
        k = int(cls[g])
        if k == 0:
            continue
        r, lab = (256, IGNORE) if k >= n_cls else (int(rank[k]) if rank is not None else k, k)
        take = (np.abs(lx) <= hw) & (np.abs(ly) <= hh) & (r > best)
        labels[take], owner[take], best[take] = lab, g, r
    return {"labels": labels, "owner": owner, "hist": hist_of(labels, n_cls), "margin": margin}


def hist_of(labels, n_cls):
    """Cells per label of one map, the last column counting 255 (a label in [n_cls, 255) cannot occur)."""
    seen = np.bincount(np.asarray(labels, np.uint8).reshape(-1), minlength=256).astype(np.int64)
    assert seen[n_cls:IGNORE].sum() == 0, "label outside [0, n_cls) and not 255"
    return np.concatenate([seen[:n_cls], seen[IGNORE:]])


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
# name, X, Y, cell, n_cls, rank (None or a tuple of n_cls ranks), cap, build(rng, grid, cap, n_cls) -> [(boxes (k, 5), cls (k,), count)] with k <= cap, exact
RasterCase = namedtuple("RasterCase", "name X Y cell n_cls rank cap build exact")


def _random_boxes(rng, grid, k, n_cls):
    """k boxes: extents 0.3-12 m, centres up to 2 m outside the grid, yaw in +-4 rad; classes over [0, n_cls) with a few ignore ids."""
    x0, y0, vx, vy, X, Y = grid
    b = np.stack([rng.uniform(x0 - 2.0, x0 + X * vx + 2.0, k), rng.uniform(y0 - 2.0, y0 + Y * vy + 2.0, k), rng.uniform(0.3, 12.0, k),
                  rng.uniform(0.3, 12.0, k), rng.uniform(-4.0, 4.0, k)], 1).astype(np.float32)
    c = rng.integers(0, n_cls, k)
    c = np.where(rng.random(k) < 0.08, rng.choice([n_cls, 200, 255], k), c)
    return b, c.astype(np.uint8)


def _random_items(counts):
    def build(rng, grid, cap, n_cls):
        out = []
        for k in counts:
            b, c = _random_boxes(rng, grid, max(0, min(k, cap)), n_cls)
            out.append((b, c, k))
        return out
    return build


def _big_and_outside(rng, grid, cap, n_cls):
    x0, y0, vx, vy, X, Y = grid
    big = [0.3, -0.2, 3.0 * X * vx, 3.0 * Y * vy, 0.7]
    out1 = [x0 - 9.0, y0 - 9.0, 4.0, 2.0, 0.4]                    # wholly outside, beyond the 2 m band
    out2 = [x0 + X * vx + 30.0, 0.0, 6.0, 6.0, -1.1]
    small = [1.1, 0.9, 2.0, 4.4, 2.2]
    return [(np.asarray([big], np.float32), np.asarray([3], np.uint8), 1),
            (np.asarray([out1, out2], np.float32), np.asarray([2, 5], np.uint8), 2),
            (np.asarray([out1, big, small, out2], np.float32), np.asarray([2, 3, 5, 200], np.uint8), 4)]


def _corner_straddle(rng, grid, cap, n_cls):
    """Boxes centred on the corner shared by tiles (0,0), (0,1), (1,0), (1,1) -- the cell boundary 16 | 15 in both axes -- and on the ragged corner."""
    x0, y0, vx, vy, X, Y = grid
    cx, cy = x0 + 16 * vx, y0 + 16 * vy
    items = []
    for yaw in (0.3, -1.2):
        items.append((np.asarray([[cx, cy, 9 * vx, 5 * vy, yaw], [x0 + 32 * vx + 0.01, y0 + 32 * vy - 0.02, 7 * vx, 7 * vy, yaw + 0.5]], np.float32),
                      np.asarray([2, 4], np.uint8), 2))
    return items


def _overlaps(rng, grid, cap, n_cls):
    """Stacks of overlapping boxes around the origin: different classes (both index orders), the same class twice, a class-0 box on top, an ignore box
    over classes; the table runs them under the NULL rank and under a permuted one."""
    hi = n_cls - 1
    lo = 1
    mid = min(3, hi)
    a = [0.2, 0.1, 6.0, 3.0, 0.4]
    b = [1.0, -0.5, 3.0, 6.0, -0.3]
    c = [-0.8, 0.6, 4.0, 4.0, 1.9]
    z = [0.0, 0.0, 5.0, 5.0, 0.1]
    ig = [0.5, 0.5, 2.0, 7.0, 0.9]
    return [(np.asarray([a, b, c], np.float32), np.asarray([lo, hi, mid], np.uint8), 3),
            (np.asarray([b, a, c], np.float32), np.asarray([hi, lo, mid], np.uint8), 3),
            (np.asarray([a, b, c], np.float32), np.asarray([mid, mid, mid], np.uint8), 3),           # same class: owner = the lowest index
            (np.asarray([a, z, b], np.float32), np.asarray([lo, 0, hi], np.uint8), 3),               # a class-0 box is a no-op
            (np.asarray([ig, a, b, c], np.float32), np.asarray([200, lo, hi, mid], np.uint8), 4),     # ignore first, still wins
            (np.asarray([a, b, ig, z], np.float32), np.asarray([hi, lo, n_cls, 0], np.uint8), 4)]     # the smallest ignore id


def _dropped(rng, grid, cap, n_cls):
    nan, inf = float("nan"), float("inf")
    ok1 = [0.4, 0.3, 3.0, 2.0, 0.5]
    ok2 = [-1.0, 1.0, 2.0, 4.4, -0.7]
    ok3 = [1.5, -1.2, 2.5, 2.5, 2.9]
    bad = [[nan, 0.0, 3.0, 3.0, 0.0], [0.0, inf, 3.0, 3.0, 0.0], [0.0, 0.0, -inf, 3.0, 0.0], [0.0, 0.0, 3.0, nan, 0.0], [0.0, 0.0, 3.0, 3.0, inf],
           [0.0, 0.0, -1.0, 3.0, 0.2], [0.0, 0.0, 3.0, -0.5, 0.2]]
    rows = [bad[0], ok1, bad[1], bad[2], ok2, bad[3], bad[4], bad[5], ok3, bad[6]]
    cls = [7, 1, 7, 7, 2, 7, 200, 7, 1, 7]
    return [(np.asarray(rows, np.float32), np.asarray(cls, np.uint8), len(rows)),
            (np.asarray(bad, np.float32), np.asarray([5] * len(bad), np.uint8), len(bad))]


def _ties_yaw0(rng, grid, cap, n_cls):
    """yaw = 0 and every coordinate a multiple of cell / 2 = 0.125 m: the edges pass exactly through cell centres, the fp64 arithmetic is exact."""
    x0, y0, vx, vy, X, Y = grid
    ctr = lambda i, j: (x0 + (i + 0.5) * vx, y0 + (j + 0.5) * vy)
    (ax, ay), (bx, by), (zx, zy), (ox, oy) = ctr(5, 7), ctr(20, 18), ctr(30, 3), ctr(33, 9)
    eps = 2.0 ** -20
    item0 = [[ax, ay, 6 * vx, 4 * vy, 0.0],                  # edges on the centres of rows 2 and 8, columns 5 and 9
             [bx, by, 10 * vx, 2 * vy, 0.0],                 # crosses the tile border at 16
             [bx + 5 * vx, by, 0.0, 2 * vy, 0.0],            # zero width: one column segment of cells, on the previous box's edge
             [zx, zy, 0.0, 0.0, 0.0],                        # zero extent exactly on a centre: that cell
             [ox + eps, oy, 0.0, 0.0, 0.0],                  # just off: nothing
             [ctr(36, 30)[0], ctr(36, 30)[1], 0.0, 0.0, 0.0]]
    item1 = [[ax + vx / 2, ay + vy / 2, 5 * vx, 3 * vy, 0.0],   # centre on a cell corner, odd extents: edges on centres again
             [ax + vx / 2, ay + vy / 2, 5 * vx, 3 * vy, 0.0],   # the same box again under a greater class
             [x0 + X * vx - vx / 2, y0 + vy / 2, 2 * vx, 2 * vy, 0.0]]  # on the grid's corner cell
    return [(np.asarray(item0, np.float32), np.asarray([1, 2, 3, 4, 5, 200], np.uint8), len(item0)),
            (np.asarray(item1, np.float32), np.asarray([2, 5, 1], np.uint8), len(item1))]


def _perm_rank(n_cls, seed):
    return tuple(int(v) for v in np.random.default_rng(seed).permutation(n_cls))


RASTER_CASES = [
    RasterCase("random_40x48", 40, 48, 0.25, 8, None, 64, _random_items([1, 7, 64, 33, 64, 12]), False),
    RasterCase("random_17x40_coarse", 17, 40, 1.6, 8, None, 64, _random_items([64, 5, 40, 64]), False),
    RasterCase("random_one_tile", 16, 16, 0.25, 8, None, 16, _random_items([16, 3]), False),
    RasterCase("random_48x17_two_classes", 48, 17, 0.25, 2, None, 32, _random_items([32, 9, 1]), False),
    RasterCase("random_32_classes_ranked", 40, 40, 1.6, 32, _perm_rank(32, 5), 64, _random_items([64, 64, 20]), False),
    RasterCase("counts_0_over_full_cap256", 40, 48, 1.6, 8, None, 256, _random_items([0, 259, 256]), False),
    RasterCase("count_over_small_cap", 17, 17, 0.25, 8, None, 4, _random_items([7, 0, 4, -3]), False),
    RasterCase("big_and_outside", 40, 17, 0.25, 8, None, 4, _big_and_outside, False),
    RasterCase("corner_straddle", 40, 48, 0.25, 8, None, 2, _corner_straddle, False),
    RasterCase("overlaps_null_rank", 48, 40, 0.25, 8, None, 4, _overlaps, False),
    RasterCase("overlaps_permuted_rank", 48, 40, 0.25, 8, (0, 6, 5, 1, 4, 3, 2, 0), 4, _overlaps, False),
    RasterCase("overlaps_two_classes", 16, 17, 0.25, 2, None, 4, _overlaps, False),
    RasterCase("overlaps_32_classes", 17, 16, 1.6, 32, _perm_rank(32, 9), 4, _overlaps, False),
    RasterCase("dropped_between_valid", 40, 40, 0.25, 8, None, 10, _dropped, False),
    RasterCase("ties_yaw0", 40, 48, 0.25, 8, None, 8, _ties_yaw0, True),
]
NAMES = [c.name for c in RASTER_CASES]


@functools.lru_cache(maxsize=None)
def make_case(index):
    """-> dict(case, grid, boxes (n, cap, 5) fp32, cls (n, cap) uint8, count (n,) int32, rank (n_cls,) uint8 or None, refs [per item]).  Computed once
    per process and shared: the arrays are read-only.  The rows beyond an item's count hold a 1000 m box of a painting class: reading one paints the
    whole map.  (A count above cap comes with all cap rows filled with real boxes: the clamp reaches every one of them.)"""
    case = RASTER_CASES[index]
    grid = grid_of(case.X, case.Y, case.cell)
    rng = np.random.default_rng(1000 + index)
    items = case.build(rng, grid, case.cap, case.n_cls)
    n = len(items)
    boxes = np.zeros((n, case.cap, 5), np.float32)
    boxes[:, :, 2:4] = 1000.0                                  # a padding row that was read would cover everything ...
    cls = np.full((n, case.cap), min(7, case.n_cls - 1), np.uint8)     # ... with a painting class
    count = np.zeros((n,), np.int32)
    for m, (b, c, k) in enumerate(items):
        assert b.shape[0] <= case.cap and b.shape[0] == c.shape[0] and (k <= b.shape[0] or b.shape[0] == case.cap)
        boxes[m, :b.shape[0]], cls[m, :b.shape[0]], count[m] = b, c, k
    rank = None if case.rank is None else np.asarray(case.rank, np.uint8)
    refs = [raster_item_ref(boxes[m], cls[m], count[m], grid, case.n_cls, rank) for m in range(n)]
    for a in [boxes, cls, count] + ([rank] if rank is not None else []) + [v for r in refs for v in r.values()]:
        a.setflags(write=False)
    return {"case": case, "grid": grid, "boxes": boxes, "cls": cls, "count": count, "rank": rank, "refs": refs}


def excluded_mask(d):
    """(n, X, Y) bool: the cells a comparison of this case may leave out -- none for an exact case."""
    margin = np.stack([r["margin"] for r in d["refs"]])
    return np.zeros(margin.shape, bool) if d["case"].exact else margin < RASTER_MARGIN


def max_excluded_cells(d):
    return int(math.floor(MAX_EXCLUDED * d["count"].shape[0] * d["case"].X * d["case"].Y))


def assert_matches(d, labels, owner=None, hist=None, what=""):
    """The comparison rule: labels and owner equal wherever the cell is not excluded, at most max_excluded_cells excluded; hist equals the bincount
    of the device's own labels exactly, and the reference's hist whenever no cell was left out."""
    case = d["case"]
    what = what or case.name
    ref_l = np.stack([r["labels"] for r in d["refs"]])
    ref_o = np.stack([r["owner"] for r in d["refs"]])
    out = excluded_mask(d)
    assert int(out.sum()) <= max_excluded_cells(d), (what, int(out.sum()), max_excluded_cells(d))
    assert labels.dtype == np.uint8 and labels.shape == ref_l.shape, (what, labels.dtype, labels.shape)
    bad = (labels != ref_l) & ~out
    assert not bad.any(), (what, "labels", int(bad.sum()), np.argwhere(bad)[:4].tolist(), labels[bad][:4], ref_l[bad][:4])
    if owner is not None:
        assert owner.dtype == np.int32 and owner.shape == ref_o.shape
        bad = (owner != ref_o) & ~out
        assert not bad.any(), (what, "owner", int(bad.sum()), np.argwhere(bad)[:4].tolist(), owner[bad][:4], ref_o[bad][:4])
    if hist is not None:
        assert hist.dtype == np.int64 and hist.shape == (ref_l.shape[0], case.n_cls + 1)
        own = np.stack([hist_of(labels[m], case.n_cls) for m in range(labels.shape[0])])
        assert np.array_equal(hist, own), (what, "hist against the device's own labels", hist, own)
        if not out.any():
            assert np.array_equal(hist, np.stack([r["hist"] for r in d["refs"]])), (what, "hist against the reference")

"""Float64 reference, case table and case generator for the IoU anchor assignment (csrc/det_assign.hip, DESIGN.md section 3.7 "IoU assignment").

Written independently of the kernel: the intersection of two rectangles is not a Sutherland-Hodgman clip but the hull of (vertices of one inside the
other) + (edge crossings), ordered by angle about their centroid, vectorised over the anchors of one box.  Disjoint rectangles have no such point: their
IoU is exactly 0.  A box that lies inside an anchor with clearance has IoU area(box) / area(anchor), evaluated as that quotient: the same float64 for every
anchor of one size that contains it (in exact arithmetic the tie is real; the kernel clips the box by the anchor's edges, gets the box back vertex for vertex
and so ties bitwise as well -- the lowest flat index wins on both sides).

The reference also returns what it cannot decide (`undecided`): both sides evaluate fp64 expressions on the same fp32 inputs and differ by contraction
and libm rounding, parts in 1e13; a decision closer than ASSIGN_MARGIN to its alternative could fall either way.
  anchor   miou within the margin of pos_thr or neg_thr;
  anchor   its two largest IoUs within the margin of each other -- "no box", IoU 0, is the last competitor, so a miou in (0, margin) counts --, unless the
           runner-up's row is bitwise the winner's (duplicate boxes: the lower index, on both sides);
  box      its two largest anchor IoUs within the margin (0 again the last competitor), unless both are containment ties as above;
  positive its heading difference d within the margin of the fold at +-pi/2.
make_case() jitters centres and headings and redraws while anything is undecided; it raises after 20 draws.
"""
import math
from collections import namedtuple

import numpy as np

ASSIGN_MARGIN = 1e-9
CELL = 0.25
MAX_GT = 256
_TOL = 1e-12                 # geometric slack of the inside / crossing tests (metres, resp. edge parameter): 1e3 below the margin
_CLEAR = 1e-6                # clearance (metres) from which a box counts as contained


class GridConfig(object):
    """What utils/postprocess.build_anchor_map reads, for an X x Y grid of 0.25 m cells centred on the origin with the first A configured anchors."""

    def __init__(self, X, Y, A):
        from v2x_sim_amd.configs.Config import Config
        self.map_dims = [X, Y, 13]
        self.voxel_size = (CELL, CELL, 0.4)
        self.area_extents = np.asarray([[-X * CELL / 2, X * CELL / 2], [-Y * CELL / 2, Y * CELL / 2], [-3.0, 2.0]])
        self.anchor_size = Config("train").anchor_size[:A]


def anchor_map(X, Y, A):
    from v2x_sim_amd.utils.postprocess import build_anchor_map
    return build_anchor_map(GridConfig(X, Y, A))


def anchor_boxes64(anchors):
    """(X, Y, A, 6) fp32 -> (X*Y*A, 5) float64 (x, y, w, h, yaw_a), yaw_a = the fp32 rounding of atan2(sin, cos) in float64."""
    a = np.asarray(anchors, np.float32).reshape(-1, 6).astype(np.float64)
    yaw = np.arctan2(a[:, 4], a[:, 5]).astype(np.float32).astype(np.float64)
    return np.concatenate([a[:, :4], yaw[:, None]], 1)


def corners64(b):
    """(N, 5) float64 -> (N, 4, 2), counter-clockwise."""
    c, s = np.cos(b[:, 4]), np.sin(b[:, 4])
    dx = 0.5 * b[:, 2:3] * np.asarray([1.0, -1.0, -1.0, 1.0])
    dy = 0.5 * b[:, 3:4] * np.asarray([1.0, 1.0, -1.0, -1.0])
    return np.stack([b[:, 0:1] + dx * c[:, None] - dy * s[:, None], b[:, 1:2] + dx * s[:, None] + dy * c[:, None]], -1)


def _clearance(pts, poly):
    """pts (N, K, 2), poly (N, 4, 2) counter-clockwise -> (N, K) signed distance of each point to the polygon's nearest edge line (>= 0: inside)."""
    v0, v1 = poly, np.roll(poly, -1, axis=1)
    e = v1 - v0                                                            # (N, 4, 2)
    ln = np.maximum(np.hypot(e[..., 0], e[..., 1]), 1e-300)
    rel = pts[:, :, None, :] - v0[:, None, :, :]                           # (N, K, 4, 2)
    cr = e[:, None, :, 0] * rel[..., 1] - e[:, None, :, 1] * rel[..., 0]
    return (cr / ln[:, None, :]).min(-1)


def iou_box_anchors64(box, anc):
    """box (5,) float64, anc (N, 5) float64 -> (iou (N,), contained (N,) bool: the box lies inside that anchor with clearance)."""
    N = anc.shape[0]
    iou, contained = np.zeros(N), np.zeros(N, bool)
    area_b, area_a = box[2] * box[3], anc[:, 2] * anc[:, 3]
    if N == 0 or area_b == 0.0:
        return iou, contained
    near = np.nonzero((np.hypot(anc[:, 0] - box[0], anc[:, 1] - box[1]) <= 0.5 * (np.hypot(anc[:, 2], anc[:, 3]) + math.hypot(box[2], box[3])) + 1e-3)
                      & (area_a != 0.0))[0]
    if near.size == 0:
        return iou, contained
    Q = corners64(anc[near])                                               # (M, 4, 2)
    M = near.size
    P = np.broadcast_to(corners64(box[None]), (M, 4, 2))
    cp, cq = _clearance(P, Q), _clearance(Q, P)
    pts = [P, Q]
    ok = [cp >= -_TOL, cq >= -_TOL]
    P1, Q1 = np.roll(P, -1, axis=1), np.roll(Q, -1, axis=1)
    for i in range(4):
        r = P1[:, i] - P[:, i]                                             # (M, 2)
        for j in range(4):
            s = Q1[:, j] - Q[:, j]
            den = r[:, 0] * s[:, 1] - r[:, 1] * s[:, 0]
            w = Q[:, j] - P[:, i]
            good = np.abs(den) > 1e-12 * np.hypot(r[:, 0], r[:, 1]) * np.hypot(s[:, 0], s[:, 1])
            dsafe = np.where(good, den, 1.0)
            t = (w[:, 0] * s[:, 1] - w[:, 1] * s[:, 0]) / dsafe
            u = (w[:, 0] * r[:, 1] - w[:, 1] * r[:, 0]) / dsafe
            pts.append((P[:, i] + t[:, None] * r)[:, None, :])
            ok.append((good & (t >= -_TOL) & (t <= 1 + _TOL) & (u >= -_TOL) & (u <= 1 + _TOL))[:, None])
    pts, ok = np.concatenate(pts, 1), np.concatenate(ok, 1)                # (M, 24, 2), (M, 24)
    k = ok.sum(1)
    cen = (pts * ok[..., None]).sum(1) / np.maximum(k, 1)[:, None]
    rel = pts - cen[:, None, :]
    ang = np.where(ok, np.arctan2(rel[..., 1], rel[..., 0]), np.inf)
    order = np.argsort(ang, axis=1, kind="stable")
    rel = np.take_along_axis(rel, order[..., None], 1)
    oks = np.take_along_axis(ok, order, 1)
    rel = np.where(oks[..., None], rel, rel[:, :1, :])                     # the unused slots repeat the first vertex: no area
    nxt = np.roll(rel, -1, axis=1)
    inter = 0.5 * np.abs((rel[..., 0] * nxt[..., 1] - nxt[..., 0] * rel[..., 1]).sum(1))
    inter = np.where(k >= 3, inter, 0.0)
    uni = area_a[near] + area_b - inter
    val = np.where(uni > 0, inter / np.where(uni > 0, uni, 1.0), 0.0)
    inside = cp.min(1) > _CLEAR
    val = np.where(inside, area_b / area_a[near], val)
    iou[near], contained[near] = val, inside
    return iou, contained


def iou_brute64(a, b):
    """Two boxes (5,) -> IoU by a plain Python Sutherland-Hodgman clip (the test of the vectorised form; one pair per call)."""
    if a[2] * a[3] == 0 or b[2] * b[3] == 0:
        return 0.0
    pa, pb = corners64(np.asarray(a, np.float64)[None])[0].tolist(), corners64(np.asarray(b, np.float64)[None])[0].tolist()
    poly = pa
    for e in range(4):
        (x0, y0), (x1, y1) = pb[e], pb[(e + 1) % 4]
        side = lambda p: (x1 - x0) * (p[1] - y0) - (y1 - y0) * (p[0] - x0)
        new = []
        for i in range(len(poly)):
            p, q = poly[i], poly[(i + 1) % len(poly)]
            sp, sq = side(p), side(q)
            if sp >= 0:
                new.append(p)
            if (sp >= 0) != (sq >= 0):
                t = sp / (sp - sq)
                new.append([p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])])
        poly = new
        if not poly:
            return 0.0
    inter = 0.5 * abs(sum(poly[i][0] * poly[(i + 1) % len(poly)][1] - poly[(i + 1) % len(poly)][0] * poly[i][1] for i in range(len(poly))))
    return inter / (a[2] * a[3] + b[2] * b[3] - inter)


def valid_boxes(boxes):
    """(G, 5) fp32 -> (G,) bool: finite fields and extents >= 0."""
    b = np.asarray(boxes, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(b).all(1) & (b[:, 2] >= 0) & (b[:, 3] >= 0)


def fold(d):
    """Heading difference folded to [-pi/2, pi/2)."""
    return np.mod(d + 0.5 * math.pi, math.pi) - 0.5 * math.pi


def codes64(gt, anc):
    """gt (N, 5), anc (N, 5) float64 -> (code (N, 6) float64, d (N,) unfolded heading difference)."""
    d = gt[:, 4] - anc[:, 4]
    f = fold(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([gt[:, 0] - anc[:, 0], gt[:, 1] - anc[:, 1], np.log(gt[:, 2] / anc[:, 2]), np.log(gt[:, 3] / anc[:, 3]), np.sin(f), np.cos(f)], 1), d


def assign_item_ref(boxes, count, anchors, pos_thr=0.6, neg_thr=0.45, force_match=True):
    """One item.  boxes (gt_cap, 5) fp32, anchors (X, Y, A, 6) fp32 -> dict: labels (Q, 2), code (Q, 6) float64, mask (Q,) bool, assoc (Q,), anchor_iou
    (Q,) float64, gt_max_iou (gt_cap,) float64, gt_best (gt_cap,), iou (gt_cap, Q) float64, and `undecided`: dict of index arrays (see the module
    docstring).  The thresholds are compared as their fp32 values, as the C entry receives them."""
    boxes = np.asarray(boxes, np.float32)
    gt_cap = boxes.shape[0]
    count = int(min(max(int(count), 0), gt_cap))
    pos, neg = float(np.float32(pos_thr)), float(np.float32(neg_thr))
    anc = anchor_boxes64(anchors)
    Q = anc.shape[0]
    valid = np.zeros(gt_cap, bool)
    valid[:count] = valid_boxes(boxes[:count])
    b64 = boxes.astype(np.float64)
    iou, cont = np.zeros((gt_cap, Q)), np.zeros((gt_cap, Q), bool)
    for g in np.nonzero(valid)[0]:
        iou[g], cont[g] = iou_box_anchors64(b64[g], anc)
    # per anchor
    miou = iou.max(0) if gt_cap else np.zeros(Q)
    gstar = np.where(miou > 0, iou.argmax(0), -1)
    und_anchor = (np.abs(miou - pos) < ASSIGN_MARGIN) | (np.abs(miou - neg) < ASSIGN_MARGIN)
    first = {}
    group = np.asarray([first.setdefault(boxes[g].tobytes(), g) for g in range(gt_cap)])      # rows that are bitwise equal share their lowest index
    for g in np.unique(gstar[gstar >= 0]):
        sel = np.nonzero(gstar == g)[0]
        others = np.nonzero(valid & (group != group[g]))[0]
        second = iou[np.ix_(others, sel)].max(0) if others.size else np.zeros(sel.size)
        und_anchor[sel[miou[sel] - np.maximum(second, 0.0) < ASSIGN_MARGIN]] = True
    positive = miou >= pos
    labels = np.zeros((Q, 2))
    labels[positive, 1] = 1.0
    labels[miou < neg, 0] = 1.0
    assoc = np.where(positive, gstar, -1)
    # per box
    gmax, gbest = np.zeros(gt_cap), np.full(gt_cap, -1, np.int64)
    und_box = np.zeros(gt_cap, bool)
    for g in np.nonzero(valid)[0]:
        q = int(iou[g].argmax())
        if iou[g, q] <= 0:
            continue
        gmax[g], gbest[g] = iou[g, q], q
        rest = iou[g].copy()
        rest[q] = 0.0
        r = int(rest.argmax())
        tie_by_containment = cont[g, q] and cont[g, r] and anc[q, 2] == anc[r, 2] and anc[q, 3] == anc[r, 3]
        if gmax[g] - rest[r] < ASSIGN_MARGIN and not tie_by_containment:
            und_box[g] = True
    if force_match:
        for g in np.nonzero(gbest >= 0)[0]:
            rivals = [o for o in np.nonzero(gbest == gbest[g])[0] if o != g and (gmax[o] > gmax[g] or (gmax[o] == gmax[g] and o < g))]
            if any(abs(gmax[o] - gmax[g]) < ASSIGN_MARGIN and group[o] != group[g] for o in np.nonzero(gbest == gbest[g])[0] if o != g):
                und_box[g] = True
            if not rivals:
                assoc[gbest[g]] = g
                labels[gbest[g]] = (0.0, 1.0)
    mask = assoc >= 0
    code = np.zeros((Q, 6))
    qs = np.nonzero(mask)[0]
    d = np.zeros(0)
    if qs.size:
        code[qs], d = codes64(b64[assoc[qs]], anc[qs])
    near_fold = np.abs(np.abs(fold(d)) - 0.5 * math.pi) < ASSIGN_MARGIN
    return {"labels": labels, "code": code, "mask": mask, "assoc": assoc, "anchor_iou": miou, "gt_max_iou": gmax, "gt_best": gbest, "iou": iou,
            "undecided": {"anchor": np.nonzero(und_anchor)[0], "box": np.nonzero(und_box)[0], "fold": qs[near_fold]}}


def n_undecided(ref):
    return sum(int(v.size) for v in ref["undecided"].values())


# ---- the case table ----------------------------------------------------------------------------------------------------------------------------
# A case: grid (X, Y, A), gt_cap, thresholds, force_match, and per item (count, kinds): `kinds` names how each of the gt_cap rows is drawn (the last
# kind repeats to fill the rows), `count` is what gt_count says (it may exceed gt_cap, or leave drawn rows unread).
#   car      2.0 x 4.4 m (+-5 %) within the grid, heading = a configured anchor yaw + up to 0.05 rad          -> threshold positives
#   car8/4   the same, heading pi/8 resp. pi/4 off the yaw-0 anchor                                           -> ignored rows / forced match only
#   any      1.7..2.3 x 3.6..4.8 m, any heading, anywhere within the grid
#   small    0.6 x 0.6 m: no threshold positive, many anchors contain it (containment tie: lowest index)
#   zero_w   zero width (valid, IoU 0);  nan: a NaN field;  neg: a negative extent  (dropped);  far: 60 m outside;  edge: centre on the grid's border
#   dup      the previous row again, bit for bit
#   onto     a car ON the forced anchor of the previous row (a `small`): both claim that anchor, the car wins
#   beside   a car one cell beside the forced anchor of the previous row: the anchor is the car's threshold positive, the small box's claim overrides it
Case = namedtuple("Case", "name X Y A gt_cap pos_thr neg_thr force items")
_I = lambda count, *kinds: (count, kinds)
ASSIGN_CASES = (
    Case("one_cell", 1, 1, 1, 1, 0.6, 0.45, 1, (_I(1, "any"),)),
    Case("one_cell_count0", 1, 1, 1, 8, 0.6, 0.45, 1, (_I(0, "car"),)),
    Case("tile_cars", 16, 16, 6, 8, 0.6, 0.45, 1, (_I(3, "car", "car8", "car4", "car"),)),
    Case("tile_items3", 16, 16, 6, 8, 0.6, 0.45, 1, (_I(0, "car"), _I(1, "car"), _I(11, "car", "any"))),
    Case("tile_cap1", 16, 16, 6, 1, 0.6, 0.45, 1, (_I(1, "car"), _I(4, "car4"), _I(0, "car"))),
    Case("tile_cap256", 16, 16, 6, 256, 0.6, 0.45, 1, (_I(1, "car"), _I(259, "any", "car4", "car8", "car"), _I(0, "car"))),
    Case("ragged_edges", 17, 19, 3, 8, 0.6, 0.45, 1, (_I(8, "zero_w", "nan", "neg", "far", "edge", "small", "car", "dup"),)),
    Case("ragged_noforce", 17, 19, 3, 8, 0.6, 0.45, 0, (_I(5, "car4", "small", "car", "edge", "any"),)),
    Case("ragged_no_ignore", 17, 19, 3, 8, 0.5, 0.5, 1, (_I(4, "car", "car8", "car4", "any"), _I(8, "any"))),
    Case("two_rows", 33, 16, 6, 8, 0.6, 0.45, 1, (_I(6, "car", "car8", "edge", "dup", "small", "any"), _I(2, "far", "car"), _I(8, "any"))),
    Case("claims", 40, 40, 6, 8, 0.6, 0.45, 1, (_I(2, "small", "onto"), _I(2, "small", "beside"), _I(4, "car", "dup", "small", "dup"))),
    Case("full_grid", 256, 256, 6, 8, 0.6, 0.45, 1, (_I(8, "car", "car8", "car4", "car", "any", "small", "edge", "car"),)),
)
ANCHOR_YAWS = (0.0, math.pi / 2, -math.pi / 4)


def _car(rng, hx, hy, yaw, at=None):
    c = (rng.uniform(-hx, hx), rng.uniform(-hy, hy)) if at is None else at
    # never aligned to better than 0.025 rad and never wider than the anchor: an aligned car that contains the 2 x 4 m anchor, or crosses it as one strip
    # crosses another, has the same IoU with the neighbouring anchor in exact arithmetic, and the best anchor is then a matter of rounding
    return [c[0], c[1], 2.0 * rng.uniform(0.96, 1.0), 4.4 * rng.uniform(0.97, 1.05), yaw + rng.uniform(0.025, 0.06) * rng.choice([-1.0, 1.0])]


def _draw_item(case, count, kinds, anchors, rng):
    hx, hy = case.X * CELL / 2, case.Y * CELL / 2
    rows = np.zeros((case.gt_cap, 5), np.float32)
    anc = anchor_boxes64(anchors)
    for g in range(case.gt_cap):
        kind = kinds[min(g, len(kinds) - 1)]
        if kind == "car":
            b = _car(rng, hx, hy, ANCHOR_YAWS[rng.integers(min(case.A, 3))])
        elif kind in ("car8", "car4"):
            b = _car(rng, hx, hy, math.pi / (8 if kind == "car8" else 4))
        elif kind == "any":
            b = [rng.uniform(-hx, hx), rng.uniform(-hy, hy), rng.uniform(1.7, 2.3), rng.uniform(3.6, 4.8), rng.uniform(-math.pi, math.pi)]
        elif kind == "small":
            b = [rng.uniform(-hx / 2, hx / 2), rng.uniform(-hy / 2, hy / 2), 0.6, 0.6, rng.uniform(-0.3, 0.3)]
        elif kind == "zero_w":
            b = [rng.uniform(-hx, hx), rng.uniform(-hy, hy), 0.0, 4.0, rng.uniform(-1, 1)]
        elif kind == "nan":
            b = [rng.uniform(-hx, hx), float("nan"), 2.0, 4.0, 0.0]
        elif kind == "neg":
            b = [rng.uniform(-hx, hx), rng.uniform(-hy, hy), -2.0, 4.0, 0.0]
        elif kind == "far":
            b = [hx + 60.0 + rng.uniform(0, 1), rng.uniform(-hy, hy), 2.0, 4.4, rng.uniform(-1, 1)]
        elif kind == "edge":
            b = [hx + rng.uniform(-0.05, 0.05), rng.uniform(-hy, hy), 2.0, 4.4, rng.uniform(-1, 1)]
        elif kind == "dup":
            rows[g] = rows[g - 1]
            continue
        elif kind in ("onto", "beside"):
            iou, _ = iou_box_anchors64(rows[g - 1].astype(np.float64), anc)
            q = anc[int(iou.argmax())]                                      # the previous row's forced anchor
            off = 0.0 if kind == "onto" else CELL
            at = (q[0] + off * math.cos(q[4]) + rng.uniform(-0.03, 0.03), q[1] + off * math.sin(q[4]) + rng.uniform(-0.03, 0.03))
            b = _car(rng, hx, hy, q[4], at)
            b[4] = q[4] + rng.uniform(-0.02, 0.02)
        else:
            raise ValueError(kind)
        rows[g] = np.asarray(b, np.float32)
    return rows


_CASE_CACHE = {}


def make_case(index):
    """-> dict: case, anchors (X, Y, A, 6) fp32, gt_boxes (n, gt_cap, 5) fp32, gt_count (n,) int32, refs [item] (assign_item_ref).  Drawn once per process;
    redrawn (new jitter) while any item has an undecided element, AssertionError after 20 draws."""
    if index in _CASE_CACHE:
        return _CASE_CACHE[index]
    case = ASSIGN_CASES[index]
    anchors = anchor_map(case.X, case.Y, case.A)
    for draw in range(20):
        rng = np.random.default_rng(7919 * index + 101 * draw + 3)
        boxes = np.stack([_draw_item(case, c, k, anchors, rng) for c, k in case.items])
        counts = np.asarray([c for c, _ in case.items], np.int32)
        refs = [assign_item_ref(boxes[m], counts[m], anchors, case.pos_thr, case.neg_thr, bool(case.force)) for m in range(len(case.items))]
        if all(n_undecided(r) == 0 for r in refs):
            out = {"case": case, "anchors": anchors, "gt_boxes": boxes, "gt_count": counts, "refs": refs, "draws": draw + 1}
            _CASE_CACHE[index] = out
            return out
    raise AssertionError("%s: undecided elements remain after 20 draws" % case.name)


def ulp32(x):
    """Spacing of fp32 at |x| (the subnormal spacing at 0)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)

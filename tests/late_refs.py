"""float64 reference and the seeded case table for late fusion (csrc/late_fuse.hip: v2x_det_late_fuse; DESIGN.md section 3 "late fusion").  A plain
helper module as tests/post_refs.py, whose greedy NMS (nms_ref64) it composes: tests/test_late_refs_cpu.py checks the reference against brute force
and every condition of the case table without a GPU, tests/test_gpu_late_fuse.py holds the kernel to it.  numpy only; every case is seeded.

The reference is fed the operands the kernel gets.  The box transform is evaluated in numpy float32 -- separate float32 multiplications and additions
are the kernel's arithmetic (__fmul_rn / __fadd_rn), bit for bit --, the crop compares those fp32 values, the suppression runs in float64 on them."""
import functools
import math
from collections import namedtuple

import numpy as np

from post_refs import IOU_MARGIN, SCORE_STEP, nms_ref64

AREA = ((-32.0, 32.0), (-32.0, 32.0))          # Config.area_extents' x and y
WIDE = ((-1.0e4, 1.0e4), (-1.0e4, 1.0e4))      # nothing is cropped: the merged count is the sum of the linked counts


# ------------------------------------------------------------------------------------------------------------------ poses
def pose(yaw, x, y):
    M = np.eye(4)
    M[0, 0], M[0, 1], M[1, 0], M[1, 1] = math.cos(yaw), -math.sin(yaw), math.sin(yaw), math.cos(yaw)
    M[0, 3], M[1, 3] = x, y
    return M


def trans_from_poses(poses):
    """World poses of the A agents -> (trans (A, A, 4, 4) fp32 in the WARP's convention, as the dataset's trans_matrices and
    synthetic_scene.make_scene's "trans": T03 = -t_y, T13 = t_x of the geometric inv(P_i) @ P_j; trans_geo (A, A, 4, 4) float64)."""
    A = len(poses)
    T, G = np.zeros((A, A, 4, 4), np.float32), np.zeros((A, A, 4, 4))
    for i in range(A):
        for j in range(A):
            G[i, j] = np.linalg.inv(poses[i]) @ poses[j]
            T[i, j] = G[i, j].astype(np.float32)
            T[i, j, 0, 3], T[i, j, 1, 3] = np.float32(-G[i, j, 1, 3]), np.float32(G[i, j, 0, 3])
    return T, G


def rigid_ref(trans):
    """The spec's derivation, written out: (..., 4, 4) -> (..., 8) fp32 (r00, r01, tx, r10, r11, ty, dyaw, 0), float64 rounded once."""
    T = np.asarray(trans, np.float64)
    r = np.zeros(T.shape[:-2] + (8,))
    r[..., 0], r[..., 1], r[..., 3], r[..., 4] = T[..., 0, 0], T[..., 0, 1], T[..., 1, 0], T[..., 1, 1]
    r[..., 2], r[..., 5] = T[..., 1, 3], -T[..., 0, 3]
    r[..., 6] = np.arctan2(T[..., 1, 0], T[..., 0, 0])
    return r.astype(np.float32)


def transform32(boxes, r):
    """(N, 5) fp32, (8,) fp32 -> (N, 5) fp32: x' = (r00*x + r01*y) + tx, y' = (r10*x + r11*y) + ty, yaw' = yaw + dyaw, each operation rounded."""
    b = np.asarray(boxes, np.float32).reshape(-1, 5)
    r = np.asarray(r, np.float32)
    assert b.dtype == np.float32 and r.dtype == np.float32
    out = b.copy()
    with np.errstate(all="ignore"):
        out[:, 0] = np.float32(r[0] * b[:, 0]) + np.float32(r[1] * b[:, 1]) + r[2]
        out[:, 1] = np.float32(r[3] * b[:, 0]) + np.float32(r[4] * b[:, 1]) + r[5]
        out[:, 4] = b[:, 4] + r[6]
    assert out.dtype == np.float32
    return out


# ------------------------------------------------------------------------------------------------------------------ the reference
def ego_candidates(boxes, scores, counts, rigid, link, A, B, cap_in, extents, i, b):
    """The candidates of ego (i, b): -> boxes (N, 5) fp32 in the ego's frame, scores (N,) fp32, tie key (N,), src (N,) = j*cap_in + rank."""
    (x_lo, x_hi), (y_lo, y_hi) = [tuple(np.float32(v) for v in e) for e in extents[:2]]
    bs, ss, tie, src = [], [], [], []
    for j in range(A):
        if j != i and not link[b, i, j]:
            continue
        c = min(max(int(counts[j * B + b]), 0), cap_in)
        raw = boxes[j * B + b, :c]
        sc = scores[j * B + b, :c]
        with np.errstate(all="ignore"):
            bx = raw.copy() if j == i else transform32(raw, rigid[b, i, j])
            ok = np.isfinite(raw).all(1) & np.isfinite(bx).all(1) & np.isfinite(sc) & (sc >= 0)
            if j != i:
                ok &= (bx[:, 0] >= x_lo) & (bx[:, 0] < x_hi) & (bx[:, 1] >= y_lo) & (bx[:, 1] < y_hi)
        w = np.nonzero(ok)[0]
        bs.append(bx[w]), ss.append(sc[w]), src.append(j * cap_in + w)
        tie.append((0 if j == i else j + 1) * cap_in + w)
    if not bs:
        return np.zeros((0, 5), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(bs), np.concatenate(ss), np.concatenate(tie).astype(np.int64), np.concatenate(src).astype(np.int64)


def ego_reference(boxes, scores, counts, rigid, link, A, B, cap_in, cap_out, extents, nms_thr, rotated, i, b):
    """The documented answer for ego (i, b): dict(count[, src, boxes (fp32, the bits expected), score_bits, consulted, cand])."""
    if not link[b, i, i]:
        return {"count": 0, "src": np.zeros(0, np.int64)}
    if any(counts[j * B + b] < 0 for j in range(A) if j == i or link[b, i, j]):
        return {"count": -(cap_out + 1)}
    bx, sc, tie, src = ego_candidates(boxes, scores, counts, rigid, link, A, B, cap_in, extents, i, b)
    if len(sc) > cap_out:
        return {"count": -len(sc)}
    kept, con = nms_ref64(sc.astype(np.float64), bx.astype(np.float64), nms_thr, rotated, index=tie)
    return {"count": len(kept), "src": src[kept], "boxes": bx[kept], "score_bits": sc[kept].view(np.uint32), "consulted": con, "n_cand": len(sc),
            "cand_scores": sc, "cand_tie": tie}


def brute_force(boxes5, scores, tie, nms_thr, iou):
    """Greedy NMS by the definition, pair by pair with the given IoU function: the order by sorting python tuples."""
    order = sorted(range(len(scores)), key=lambda q: (-float(scores[q]), int(tie[q])))
    kept = []
    for q in order:
        if all(not iou(boxes5[k], boxes5[q]) > nms_thr for k in kept):
            kept.append(q)
    return kept


# ------------------------------------------------------------------------------------------------------------------ cases
# One case = one call.  counts[b][j]: detections of agent j in frame b (negative: the post-processor's "not computed"; above cap_in: hostile, reads
# as cap_in).  link: "all", "none", "v2i" (vehicles hear agent 0 only, agent 0 hears everybody), "asym" (a seeded irregular mask, not symmetric),
# "absent" (agents 1 and A-1 absent from frame 0: rows, columns and diagonal off).  scores: "distinct" or "ties" (groups of bit-equal scores
# across agents).  extents: AREA (the crop is active) or WIDE.
LateCase = namedtuple("LateCase", "name A B cap_in cap_out nms_thr rotated link extents counts scores seed")

_c100 = (100, 100, 100, 100, 100)
LATE_CASES = (
    LateCase("a2-small", 2, 1, 64, 64, 0.01, False, "all", AREA, ((20, 30),), "distinct", 1),
    LateCase("a5-b3-rot", 5, 3, 64, 1024, 0.3, True, "all", AREA, ((64, 0, 37, 1, 63), (5, 64, 64, 64, 64), (0, 0, 0, 0, 9)), "distinct", 2),
    LateCase("a6-fast-edge", 6, 3, 256, 1024, 0.2, False, "all", WIDE, (_c100 + (11,), _c100 + (12,), _c100 + (13,)), "distinct", 3),
    LateCase("a2-capout64-edge", 2, 3, 64, 64, 0.01, False, "all", WIDE, ((32, 31), (32, 32), (33, 32)), "distinct", 4),
    LateCase("a5-capout1024-edge", 5, 3, 256, 1024, 0.2, False, "all", WIDE, ((256, 256, 256, 256, 0), (256, 256, 256, 256, 1), (256, 255, 256, 256, 0)), "ties", 5),
    LateCase("a6-serial-rot", 6, 1, 256, 1024, 0.2, True, "all", WIDE, ((100, 100, 100, 100, 100, 100),), "distinct", 6),
    LateCase("a5-v2i", 5, 3, 64, 64, 0.01, False, "v2i", AREA, ((12, 10, 9, 11, 8), (10, 0, 12, 9, 7), (3, 12, 12, 12, 12)), "ties", 7),
    LateCase("a5-asym", 5, 3, 64, 1024, 0.01, False, "asym", AREA, ((40, 35, 0, 64, 20), (1, 2, 3, 4, 5), (64, 64, 64, 64, 64)), "distinct", 8),
    LateCase("a6-absent", 6, 3, 64, 64, 0.3, False, "absent", AREA, ((10, 9, 8, 7, 6, 5), (10, 9, 8, 7, 6, 5), (4, 4, 4, 4, 4, 4)), "distinct", 9),
    LateCase("a5-negative-source", 5, 3, 64, 64, 0.01, False, "asym", AREA, ((10, -70, 9, 8, 7), (6, 6, -1, 6, 6), (5, 5, 5, 5, -4096)), "distinct", 10),
    LateCase("a1", 1, 3, 64, 64, 0.01, True, "all", AREA, ((64,), (0,), (17,)), "distinct", 11),
    LateCase("a5-hostile-counts", 5, 1, 64, 1024, 0.01, False, "all", WIDE, ((65, 4096, 2 ** 31 - 1, 64, 1),), "distinct", 12),
)
PITCH = 8.0          # metres between world objects: with sizes <= 4.5 m (diagonal 6.4 m) and 0.4 m of jitter, the stand-up boxes of two DIFFERENT objects
                     # never overlap -- every consulted IoU is 0 or that of two detections of the same object


def make_link(kind, A, B, rng):
    L = np.ones((B, A, A), np.uint8)
    if kind == "none":
        L[:] = np.eye(A, dtype=np.uint8)
    elif kind == "v2i":
        L[:] = 0
        L[:, :, 0] = 1
        L[:, 0, :] = 1
        L[:, np.arange(A), np.arange(A)] = 1
    elif kind == "asym":
        L = (rng.random((B, A, A)) < 0.5).astype(np.uint8)
        L[:, np.arange(A), np.arange(A)] = 1
        L[:, 0, 1], L[:, 1, 0] = 1, 0                  # not symmetric, whatever the draw
    elif kind == "absent":
        for j in (1, A - 1):
            L[0, j, :] = 0
            L[0, :, j] = 0
    else:
        assert kind == "all"
    return L


def _world(n, rng):
    nx = int(math.ceil(math.sqrt(n)))
    k = np.arange(n)
    w = np.zeros((n, 5))
    w[:, 0] = ((k % nx) - (nx - 1) / 2.0) * PITCH + rng.uniform(-0.4, 0.4, n)
    w[:, 1] = ((k // nx) - (nx - 1) / 2.0) * PITCH + rng.uniform(-0.4, 0.4, n)
    w[:, 2:4] = rng.uniform(1.2, 4.2, (n, 2))
    w[:, 4] = rng.uniform(-math.pi, math.pi, n)
    return w


def _tie_levels(n, rng):
    lv = np.empty(n, np.int64)
    at = g = 0
    while at < n:
        size = int(rng.integers(2, 9))
        lv[at:at + size] = g
        at += size
        g += 1
    return lv[rng.permutation(n)]


@functools.lru_cache(maxsize=None)
def make_late_case(index):
    """-> dict(case, boxes (A*B, cap_in, 5), scores (A*B, cap_in), counts (A*B,), trans (B, A, A, 4, 4), rigid (B, A, A, 8), link (B, A, A), refs[i][b]).
    Per frame: a world of objects on a lattice, A agents at seeded poses; agent j detects counts[b][j] distinct objects, each a little off its true
    place (0.15 m, 3 % of its size, 0.05 rad) and expressed in j's frame; its list is in descending score order.  Rows past a count hold boxes that
    WOULD enter (a detection at the ego's origin with the top score) if the kernel read them."""
    case = LATE_CASES[index]
    A, B, cap_in = case.A, case.B, case.cap_in
    rng = np.random.default_rng(7000 + case.seed)
    boxes = np.zeros((A * B, cap_in, 5), np.float32)
    boxes[:, :, 2:4] = 2.0
    scores = np.full((A * B, cap_in), 0.999, np.float32)
    counts = np.zeros(A * B, np.int32)
    trans = np.zeros((B, A, A, 4, 4), np.float32)
    for b in range(B):
        held = [min(max(c, 0), cap_in) for c in case.counts[b]]
        total = sum(held)
        world = _world(max(max(held), int(0.6 * total), 1), rng)
        span = 10.0 if case.extents is AREA else 30.0
        poses = [pose(rng.uniform(-math.pi, math.pi), *rng.uniform(-span, span, 2)) for _ in range(A)]
        trans[b] = trans_from_poses(poses)[0]
        level = _tie_levels(total, rng) if case.scores == "ties" else rng.permutation(total)
        at = 0
        for j in range(A):
            c = held[j]
            counts[j * B + b] = case.counts[b][j]
            pick = rng.choice(world.shape[0], c, replace=False)
            d = world[pick].copy()
            d[:, 0:2] += rng.uniform(-0.15, 0.15, (c, 2))
            d[:, 2:4] *= rng.uniform(0.97, 1.03, (c, 2))
            d[:, 4] += rng.uniform(-0.05, 0.05, c)
            inv = np.linalg.inv(poses[j])
            local = d.copy()
            local[:, 0:2] = d[:, 0:2] @ inv[:2, :2].T + inv[:2, 3]
            local[:, 4] = d[:, 4] - math.atan2(poses[j][1, 0], poses[j][0, 0])
            s = (0.97 - SCORE_STEP * level[at:at + c]).astype(np.float32)
            at += c
            order = np.argsort(-s, kind="stable")
            boxes[j * B + b, :c] = local[order].astype(np.float32)
            scores[j * B + b, :c] = s[order]
    rigid = rigid_ref(trans)
    link = make_link(case.link, A, B, rng)
    refs = [[ego_reference(boxes, scores, counts, rigid, link, A, B, cap_in, case.cap_out, case.extents, case.nms_thr, case.rotated, i, b)
             for b in range(B)] for i in range(A)]
    return {"case": case, "boxes": boxes, "scores": scores, "counts": counts, "trans": trans, "rigid": rigid, "link": link, "refs": refs}


# ------------------------------------------------------------------------------------------------------------------ the scene test
SCENE_SEEDS = tuple(range(12))
SCENE_CROP = ((-29.0, 29.0), (-29.0, 29.0))


def scene_inputs(seed, cap_in=64):
    """make_scene(sensor_range=18, n_cars=40): every agent's detections ARE its own ground truth (scores distinct, descending).
    -> boxes (A, cap_in, 5), scores (A, cap_in), counts (A,), trans (1, A, A, 4, 4), gt_any: per agent the (G, 5) cars in range of ANY agent."""
    from v2x_sim_amd.utils.synthetic_scene import make_scene
    own = make_scene(sensor_range=18.0, n_cars=40, seed=seed, ground_pts=10, clutter_pts=10, pts_per_car=4, max_pts=512)
    anyone = make_scene(sensor_range=18.0, n_cars=40, seed=seed, ground_pts=10, clutter_pts=10, pts_per_car=4, max_pts=512, gt="any")
    A = len(own["gt_boxes"])
    boxes = np.zeros((A, cap_in, 5), np.float32)
    scores = np.zeros((A, cap_in), np.float32)
    counts = np.zeros(A, np.int32)
    for j, g in enumerate(own["gt_boxes"]):
        counts[j] = len(g)
        boxes[j, :len(g)] = g
        scores[j, :len(g)] = (0.95 - 1e-3 * j - 1e-5 * np.arange(len(g))).astype(np.float32)
    return boxes, scores, counts, own["trans"][None], anyone["gt_boxes"], own["trans_geo"]


def rigid_equality_inputs():
    """Matrices on which the numpy and the torch derivation of `rigid` must agree bit for bit: the scenes' poses, the case table's, atan2's quadrant edges."""
    from v2x_sim_amd.utils.synthetic_scene import make_scene
    out = [make_scene(agents=5, n_cars=4, seed=s, ground_pts=10, clutter_pts=10, pts_per_car=4, max_pts=256)["trans"] for s in range(12)]
    out += [make_late_case(k)["trans"] for k in range(len(LATE_CASES))]
    yaws = [0.0, math.pi / 2, math.pi, -math.pi / 2, -math.pi, math.pi / 4, 3 * math.pi / 4, 1e-8, -1e-8, math.pi - 1e-7]
    out.append(trans_from_poses([pose(y, 3.0 * k, -2.0 * k) for k, y in enumerate(yaws)])[0])
    return out

"""float64 references and the seeded case tables for the detection post-processing kernels of csrc/postprocess.hip (det_candidates_kernel,
det_nms_kernel in its FAST and serial forms, rotated_iou_kernel, match_detections_kernel).  A plain helper module (as tests/fusion_refs.py):
tests/test_post_refs_cpu.py checks the references against oracle/postprocess_ref.py and every condition the case tables must satisfy
without a GPU, tests/test_gpu_post_sweep.py holds the kernels to them.  numpy and math only; every case is seeded.

The references are fed the operands the kernels get (fp32 logits, codes, anchors and boxes, widened exactly) and compute in float64."""
import functools
import math
from collections import namedtuple

import numpy as np

from oracle import postprocess_ref as PR

NMS_FAST_CAP = 512          # csrc/postprocess.hip: at most this many candidates take the FAST (bit matrix) form
WORD = 64                   # candidates per word of the FAST form's `removed` set
BLOCK = 256                 # keys one pass of the workgroup's bitonic sort handles (threads per workgroup)
SCORE_THR = 0.7             # the sweep's score threshold on the logits path
IOU_MARGIN = 1e-3           # every consulted pair IoU is further than this from its case's nms_thr
SCORE_STEP = 6e-5           # distance of neighbouring score levels (the condition asserted is >= 1e-5)


# ------------------------------------------------------------------------------------------------------------------ decode, geometry
def score64(c0, c1):
    """postprocess_ref.fg_score on arrays of fp32 logits, in float64."""
    c0, c1 = np.asarray(c0, np.float64), np.asarray(c1, np.float64)
    m = np.maximum(c0, c1)
    e0, e1 = np.exp(c0 - m), np.exp(c1 - m)
    return e1 / (e0 + e1)


def decode64(codes, anchors):
    """postprocess_ref.decode_faf on arrays: codes (N, 6), anchors (N, 6) -> (N, 5) float64 (x, y, w, h, yaw)."""
    c = np.asarray(codes, np.float64).reshape(-1, 6)
    a = np.asarray(anchors, np.float64).reshape(-1, 6)
    dw = np.clip(c[:, 2], -PR.DECODE_CLIP, PR.DECODE_CLIP)
    dh = np.clip(c[:, 3], -PR.DECODE_CLIP, PR.DECODE_CLIP)
    return np.stack([a[:, 0] + c[:, 0], a[:, 1] + c[:, 1], a[:, 2] * np.exp(dw), a[:, 3] * np.exp(dh),
                     np.arctan2(a[:, 4], a[:, 5]) + np.arctan2(c[:, 4], c[:, 5])], 1)


def corners64(boxes5):
    """postprocess_ref.corners_of on arrays: (N, 5) -> (N, 4, 2), counter-clockwise, first = (+w/2, +h/2) rotated."""
    b = np.asarray(boxes5, np.float64).reshape(-1, 5)
    c, s = np.cos(b[:, 4]), np.sin(b[:, 4])
    out = np.empty((b.shape[0], 4, 2))
    for q, (sx, sy) in enumerate(((0.5, 0.5), (-0.5, 0.5), (-0.5, -0.5), (0.5, -0.5))):
        lx, ly = sx * b[:, 2], sy * b[:, 3]
        out[:, q, 0] = b[:, 0] + lx * c - ly * s
        out[:, q, 1] = b[:, 1] + lx * s + ly * c
    return out


def standup64(corners):
    return np.stack([corners[..., 0].min(-1), corners[..., 1].min(-1), corners[..., 0].max(-1), corners[..., 1].max(-1)], -1)


_IOU_CACHE = {}


def rotated_iou64(ca, cb):
    """postprocess_ref.rotated_iou of two (4, 2) corner arrays, remembered per pair of operands (the case generators ask again and again)."""
    key = (ca.tobytes(), cb.tobytes())
    v = _IOU_CACHE.get(key)
    if v is None:
        v = _IOU_CACHE[key] = PR.rotated_iou(ca.tolist(), cb.tolist())
    return v


def iou_ref64(a, b):
    """(na, 5), (nb, 5) fp32 boxes -> (na, nb) float64 IoU by the oracle, one call per pair.  A rectangle of zero width or height has no
    area, so its intersection with anything has none: IoU 0 by definition (also 0 / 0, both empty -- the kernel's convention) -- stated
    here because the oracle's point-in-polygon test takes EVERY point for inside a polygon whose edges all have zero length."""
    a, b = np.asarray(a, np.float32).reshape(-1, 5), np.asarray(b, np.float32).reshape(-1, 5)
    ca, cb = corners64(a), corners64(b)
    ea, eb = (a[:, 2] == 0) | (a[:, 3] == 0), (b[:, 2] == 0) | (b[:, 3] == 0)
    return np.array([[0.0 if ea[i] or eb[j] else rotated_iou64(ca[i], cb[j]) for j in range(len(cb))] for i in range(len(ca))]).reshape(len(ca), len(cb))


# ------------------------------------------------------------------------------------------------------------------ NMS reference
Consulted = namedtuple("Consulted", "iou kept cand")     # per consulted pair: its IoU and the positions of the kept box and the candidate


def nms_ref64(scores, boxes5, nms_thr, rotated, index=None):
    """Greedy NMS in float64 on decoded candidates: order = score descending, ties by `index` (default: position) ascending; a candidate is
    dropped iff its IoU with an already KEPT one exceeds nms_thr -- the stand-up boxes' IoU, or (rotated) the polygon IoU of the boxes
    themselves, which is evaluated (postprocess_ref.rotated_iou) only where the stand-up boxes overlap.
    -> (kept positions in the order kept, Consulted): every pair (kept, candidate) the scan looked at, each candidate against the whole kept
    list of its moment, as both forms of det_nms_kernel do (rotated: the pairs whose stand-up boxes overlap)."""
    scores = np.asarray(scores, np.float64)
    n = scores.shape[0]
    index = np.arange(n) if index is None else np.asarray(index)
    order = np.lexsort((index, -scores))
    cor = corners64(np.asarray(boxes5, np.float64).reshape(-1, 5)[order])
    su = standup64(cor)
    area = (su[:, 2] - su[:, 0]) * (su[:, 3] - su[:, 1])
    kept = np.empty(n, np.int64)
    nk = 0
    c_iou, c_k, c_i = [], [], []
    for i in range(n):
        k = kept[:nk]
        iw = np.minimum(su[k, 2], su[i, 2]) - np.maximum(su[k, 0], su[i, 0])
        ih = np.minimum(su[k, 3], su[i, 3]) - np.maximum(su[k, 1], su[i, 1])
        ov = (iw > 0.0) & (ih > 0.0)
        if rotated:
            k = k[ov]
            iou = np.array([rotated_iou64(cor[i], cor[q]) for q in k], np.float64)
        else:
            inter = np.where(ov, iw * ih, 0.0)
            iou = inter / (area[k] + area[i] - inter)
        c_iou.append(iou)
        c_k.append(k)
        c_i.append(np.full(k.shape, i, np.int64))
        if not (iou > nms_thr).any():
            kept[nk] = i
            nk += 1
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros((0,), dt)
    return order[kept[:nk]], Consulted(cat(c_iou, np.float64), order[cat(c_k, np.int64)], order[cat(c_i, np.int64)])


# ------------------------------------------------------------------------------------------------------------------ NMS cases
# One case = the maps of ONE launch.  counts: candidates per map (> cap: only the -count answer is asserted).  geom: "chains" (unit squares on
# a line at pitch 0.5, yaw exactly 0: every IoU is 0 or 1/3, exact in fp32) or "lattice" (2-D lattice, seeded jitter, sizes 1 - 5 m, seeded
# yaws).  order (chains): how the scores run along the line.  scores: "distinct", "equal" or "ties" (groups of 2 - 16 bit-equal scores).
NmsCase = namedtuple("NmsCase", "name cap nms_thr rotated geom order scores counts seed")

NMS_CASES = (
    NmsCase("cap64-chains-desc", 64, 0.2, False, "chains", "desc", "distinct", (0, 1, 2, 63, 64, 65), 1),
    NmsCase("cap64-lattice-ties-rot", 64, 0.3, True, "lattice", None, "ties", (63, 64, 65, 2, 1, 0), 2),
    NmsCase("cap256-chains-asc", 256, 0.2, False, "chains", "asc", "distinct", (255, 256, 257, 65, 64, 63), 3),
    NmsCase("cap256-lattice-equal", 256, 0.01, False, "lattice", None, "equal", (256, 255, 257, 37), 4),
    NmsCase("cap1024-chains-perm-ties", 1024, 0.2, False, "chains", "perm", "ties", (511, 512, 513, 1023, 1024, 1025), 5),
    NmsCase("cap1024-chains-perm-rot", 1024, 0.2, True, "chains", "perm", "distinct", (512, 513, 257, 2), 6),
    NmsCase("cap1024-lattice-mixed", 1024, 0.01, False, "lattice", None, "distinct", (0, 37, 512, 513, 1025, 1024, 1), 7),
    NmsCase("cap1024-lattice-mixed-permuted", 1024, 0.3, False, "lattice", None, "ties", (513, 1, 1024, 0, 1025, 37, 512), 8),
    NmsCase("cap1024-lattice-rot", 1024, 0.1, True, "lattice", None, "distinct", (1023, 511, 512, 65), 9),
    NmsCase("cap4096-chains-perm", 4096, 0.2, False, "chains", "perm", "distinct", (4095, 4096, 4097, 1025, 513), 10),
    NmsCase("cap4096-chains-desc-equal", 4096, 0.2, False, "chains", "desc", "equal", (4096, 512), 11),
    NmsCase("cap4096-lattice-ties", 4096, 0.01, False, "lattice", None, "ties", (4096, 1023), 12),
    NmsCase("cap4096-lattice-rot", 4096, 0.3, True, "lattice", None, "distinct", (4096, 4097, 257), 13),
)
MIXED_COUNTS = lambda cap: (0, 37, 512, 513, cap + 1, cap, 1)
EXTRA_ANCHORS = 16          # anchors per case beyond cap: M = cap + 16, so that cap + 1 candidates exist and a map is a proper subset


def level_margin(rank):
    """fp32 logit margin c1 - c0 of score level `rank` (0 = the highest): levels are SCORE_STEP apart, all above SCORE_THR + 0.02."""
    s = 0.97 - SCORE_STEP * np.asarray(rank, np.float64)
    return np.log(s / (1.0 - s)).astype(np.float32)


def _nms_geometry(case, rng):
    """-> anchors (M, 6), codes (M, 6) fp32: the geometry of every anchor of the case (its maps pick runs of them)."""
    M = case.cap + EXTRA_ANCHORS
    anchors = np.zeros((M, 6), np.float32)
    codes = np.zeros((M, 6), np.float32)
    if case.geom == "chains":
        anchors[:, 0] = 0.5 * np.arange(M)              # exact in fp32; unit squares, yaw atan2(0, 1) + atan2(0, 1) = 0 exactly
        anchors[:, 2:4] = 1.0
        anchors[:, 5] = 1.0
        codes[:, 5] = 1.0
        return anchors, codes
    nx = int(math.ceil(math.sqrt(M)))
    pitch = 1.9                                           # 65 sites: +-60.8 m, with the jitter inside |x|, |y| <= 64 m
    site = np.arange(M)
    anchors[:, 0] = ((site % nx) - (nx - 1) / 2.0) * pitch
    anchors[:, 1] = ((site // nx) - (nx - 1) / 2.0) * pitch
    anchors[:, 2:4] = rng.uniform(1.2, 4.5, (M, 2))
    ya = rng.uniform(-math.pi, math.pi, M)
    anchors[:, 4], anchors[:, 5] = np.sin(ya), np.cos(ya)
    _jitter(codes, np.arange(M), rng)
    return anchors, codes


def _jitter(codes, which, rng):
    n = len(which)
    codes[which, 0:2] = rng.uniform(-0.4, 0.4, (n, 2))
    codes[which, 2:4] = rng.uniform(-0.1, 0.1, (n, 2))    # sizes stay within 1.08 .. 4.98 m
    yc = rng.uniform(-0.3, 0.3, n)
    r = rng.uniform(0.5, 2.0, n)                          # the code's (sin, cos) need not be normalised
    codes[which, 4], codes[which, 5] = r * np.sin(yc), r * np.cos(yc)


def _tie_groups(c, rng):
    """Group id per ordinal: groups of 2 - 16 members (the last takes what is left), members scattered by a seeded permutation."""
    gid = np.empty(c, np.int64)
    at = g = 0
    while at < c:
        size = int(rng.integers(2, 17))
        gid[at:at + size] = g
        at += size
        g += 1
    return gid[rng.permutation(c)] if c else gid


def _nms_map(case, c, rng):
    """One map: a run of c anchors, their score levels and the slot each candidate's key sits in."""
    M = case.cap + EXTRA_ANCHORS
    off = int(rng.integers(0, M - c + 1))
    aid = np.arange(off, off + c, dtype=np.int64)
    if case.scores == "equal":
        rank = np.zeros(c, np.int64)
    elif case.scores == "ties":
        rank = _tie_groups(c, rng)
    elif case.order == "desc":
        rank = np.arange(c)
    elif case.order == "asc":
        rank = np.arange(c)[::-1].copy()
    else:
        rank = rng.permutation(c)
    return {"aid": aid, "margin": level_margin(rank), "slot": rng.permutation(c)}


def map_reference(m, anchors, codes, cap, nms_thr, rotated):
    """The float64 answer for one map {"aid", "margin", ...}: count (-c when c > cap), kept anchor indices in order, their fp32 score bits and
    float64 boxes, and the consulted pairs (as anchor indices)."""
    aid = m["aid"]
    c = len(aid)
    if c > cap:
        return {"count": -c}
    sc = score64(np.zeros(c, np.float32), m["margin"])
    boxes = decode64(codes[aid], anchors[aid])
    kept, con = nms_ref64(sc, boxes, nms_thr, rotated, index=aid)
    return {"count": len(kept), "index": aid[kept], "score_bits": sc[kept].astype(np.float32).view(np.uint32), "scores": sc[kept],
            "boxes": boxes[kept], "consulted": Consulted(con.iou, aid[con.kept], aid[con.cand]), "all_scores": sc}


@functools.lru_cache(maxsize=None)
def make_nms_case(index):
    """-> dict(anchors, codes, maps, refs).  Lattice cases: a candidate of a consulted pair whose IoU lies within IOU_MARGIN of nms_thr is
    given another jitter until no such pair is left, so that no decision of the case rests on a rounding."""
    case = NMS_CASES[index]
    rng = np.random.default_rng(1000 + case.seed)
    anchors, codes = _nms_geometry(case, rng)
    maps = [_nms_map(case, c, rng) for c in case.counts]
    for _ in range(40):
        refs = [map_reference(m, anchors, codes, case.cap, case.nms_thr, case.rotated) for m in maps]
        if case.geom == "chains":
            break
        bad = set()
        for r in refs:
            if r["count"] >= 0:
                near = np.abs(r["consulted"].iou - case.nms_thr) <= 1.5 * IOU_MARGIN
                bad.update(r["consulted"].cand[near].tolist())
        if not bad:
            break
        _jitter(codes, np.array(sorted(bad)), rng)
    else:
        raise AssertionError("%s: pairs near the threshold remain" % case.name)
    return {"case": case, "anchors": anchors, "codes": codes, "maps": maps, "refs": refs}


def launch_arrays(maps, anchors, codes, cap):
    """numpy operands of one launch for both entries.  Logits path: cls (n, M, 2), loc (n, M, 6) -- an anchor outside the map scores 0.007.
    Slotted path: keys (n, cap) int64 = ~score bits << 32 | anchor << 12 | slot, slot_codes (n, cap, 6), counts (n,) -- score bits = the fp32
    rounding of the float64 score; unused slots hold a key that would sort FIRST (score 1.0, anchor 0) and NaN codes, and a map with more
    than cap candidates holds the first cap of them, as the fused heads leave it."""
    n, M = len(maps), anchors.shape[0]
    cls = np.zeros((n, M, 2), np.float32)
    cls[:, :, 1] = -5.0
    loc = np.broadcast_to(codes, (n, M, 6)).copy()
    poison = np.uint64(~np.float32(1.0).view(np.uint32) & 0xffffffff) << np.uint64(32) | np.uint64(cap - 1)
    keys = np.full((n, cap), poison, np.uint64)
    slot_codes = np.full((n, cap, 6), np.nan, np.float32)
    counts = np.zeros((n,), np.int32)
    for i, m in enumerate(maps):
        aid, slot = m["aid"], m["slot"]
        cls[i, aid, 1] = m["margin"]
        counts[i] = len(aid)
        bits = score64(np.zeros(len(aid), np.float32), m["margin"]).astype(np.float32).view(np.uint32)
        fit = slot < cap
        keys[i, slot[fit]] = ((~bits[fit]).astype(np.uint64) & np.uint64(0xffffffff)) << np.uint64(32) | (aid[fit].astype(np.uint64) << np.uint64(12)) | slot[fit].astype(np.uint64)
        slot_codes[i, slot[fit]] = codes[aid[fit]]
    return {"cls": cls, "loc": loc, "keys": keys.view(np.int64), "slot_codes": slot_codes, "counts": counts}


def pad_to_serial(m, anchors, codes, rng):
    """A map with at most NMS_FAST_CAP candidates -> (map, anchors, codes) with isolated candidates appended until the count exceeds
    NMS_FAST_CAP: each scores below every original and lies 10 m from the next, far from everything.  The padded map takes the serial form;
    its first k detections must be the unpadded map's."""
    c = len(m["aid"])
    assert c <= NMS_FAST_CAP
    extra = NMS_FAST_CAP + 1 - c + int(rng.integers(0, 40))
    M = anchors.shape[0]
    a2 = np.zeros((M + extra, 6), np.float32)
    a2[:M] = anchors
    a2[M:, 0] = 5000.0 + 10.0 * np.arange(extra)
    a2[M:, 1] = 5000.0
    a2[M:, 2:4] = 1.0
    a2[M:, 5] = 1.0
    c2 = np.zeros((M + extra, 6), np.float32)
    c2[:M] = codes
    c2[M:, 5] = 1.0
    s = 0.7195 - 2e-5 * rng.permutation(extra)             # 0.7195 .. 0.708: below the lowest level (0.72), above SCORE_THR
    pm = {"aid": np.concatenate([m["aid"], M + np.arange(extra)]),
          "margin": np.concatenate([m["margin"], np.log(s / (1.0 - s)).astype(np.float32)]),
          "slot": rng.permutation(c + extra)}
    return pm, a2, c2


# ------------------------------------------------------------------------------------------------------------------ decode cases
def make_decode_case():
    """-> codes (N, 6), anchors (N, 6) fp32, one row per edge: every (dw, dh) of the list (the +-4 clip from both sides), the (ds, dc) that
    meet atan2f(0, 0) and its neighbours, yaw sums beyond +-pi, boxes at |x| = 1e4 m (anchor and offset chosen so that the fp32 sum is exact:
    the spacing of fp32 at 1e4 is 9.8e-4 m, above the 1e-4 m bar)."""
    dwh = (-5.0, -4.0, -4.0 + 2.0 ** -20, 0.0, 4.0, 4.001, 50.0)
    dsc = ((0.0, 0.0), (0.0, -1.0), (1e-30, 1.0), (-1.0, 0.0))
    rows = []
    for i, dw in enumerate(dwh):
        for j, dh in enumerate(dwh):
            ds, dc = dsc[(i + j) % 4]
            rows.append(((0.25, -0.125, dw, dh, ds, dc), (3.0 * i, 2.0 * j, 2.0, 4.0, 0.0, 1.0)))
    for ds, dc in dsc:
        for ya in (0.0, math.pi / 2, -math.pi / 4, 3.0):
            rows.append(((0.5, 0.5, 0.1, -0.1, ds, dc), (1.0, 1.0, 3.0, 12.0, math.sin(ya), math.cos(ya))))
    for ya, yc in ((3.0, 2.0), (-3.0, -2.5), (math.pi, math.pi), (2.5, 0.7), (-math.pi / 2, -math.pi)):
        rows.append(((0.0, 0.0, 0.0, 0.0, math.sin(yc), math.cos(yc)), (0.0, 0.0, 2.0, 4.0, math.sin(ya), math.cos(ya))))
    for xa, dx, y_a, dy in ((9984.0, 16.0, 0.0, 0.0), (-9000.0, -1000.0, 8192.0, 1808.0), (10000.0, 0.0, -10000.0, 0.0)):
        rows.append(((dx, dy, 0.3, -0.2, 0.1, 0.9), (xa, y_a, 2.0, 4.0, 0.6, 0.8)))
    codes = np.array([r[0] for r in rows], np.float32)
    anchors = np.array([r[1] for r in rows], np.float32)
    return codes, anchors


DECODE_CASES = make_decode_case()


# ------------------------------------------------------------------------------------------------------------------ candidate cases
CAND_THRS = (0.0, 0.5, 0.7, 1.0)
CAND_MS = (1, 255, 257, 16384, 16385)
CAND_CAP = 4096
CAND_CASES = tuple((thr, M) for thr in CAND_THRS for M in CAND_MS)
CAND_MARGIN = 1e-5


def thr32(thr):
    """The threshold as the kernel gets it: a C float."""
    return float(np.float32(thr))


def _cand_special_rows(thr):
    """(c0, c1, why) rows whose score sits exactly AT a threshold by construction, or at the edge of the candidate margin around `thr`."""
    rows = [(0.0, 0.0, "equal"), (3.5, 3.5, "equal"), (-7.0, -7.0, "equal"),
            (-80.0, 80.0, "saturated"), (80.0, -80.0, "saturated"), (-1e4, 1e4, "saturated"), (1e4, -1e4, "saturated")]
    t = thr32(thr)
    if 0.0 < t < 1.0 and t != 0.5:
        # log(thr / (1 - thr)) itself, rounded to fp32 either way, gives a score 1e-8 from thr -- below the 6e-8 resolution of the fp32 score,
        # so no reference decides it; the rows sit where the candidate margin starts instead: the score CAND_MARGIN (and a little) away
        for sign in (-1.0, 1.0):
            s = t + sign * 1.02 * CAND_MARGIN
            rows.append((1.0, float(np.float32(1.0 + math.log(s / (1.0 - s)))), "margin-edge"))
    # thr = 0.5: the margin log(1) = 0 IS the equal-logits row, whichever way it is rounded; thr = 0 and 1: the margin is -+inf, the saturated rows
    return rows


@functools.lru_cache(maxsize=None)
def make_cand_case(thr, M):
    """-> cls (M, 2) fp32, expected passing anchor indices (float64 rule: score64 >= thr as a C float), expected count (-n when n > CAND_CAP).
    The special rows cycle through the first anchors, the rest is seeded with ~10 % above 0.7; the LAST anchor always passes a threshold
    below 1 by a wide margin and saturates for a threshold of 1 (M = 16385: the one anchor of the second grid pass)."""
    rng = np.random.default_rng(int(thr * 100) * 100003 + M)
    special = _cand_special_rows(thr)
    cls = np.empty((M, 2), np.float32)
    cls[:, 0] = rng.normal(0.0, 1.0, M)
    cls[:, 1] = cls[:, 0] + rng.uniform(-8.0, 1.5, M).astype(np.float32)
    ns = min(M, 3 * len(special))
    for i in range(ns):
        cls[i] = special[i % len(special)][:2]
    cls[M - 1] = (-80.0, 80.0) if thr >= 1.0 else (-1.0, 4.0)
    t = thr32(thr)
    for _ in range(20):                                     # the seeded rest keeps the candidate margin
        s = score64(cls[:, 0], cls[:, 1])
        near = (np.abs(s - t) < 2 * CAND_MARGIN) & (s != t) & (np.arange(M) >= ns) & (np.arange(M) < M - 1)
        if not near.any() or t == 0.0:
            break
        cls[near, 1] = cls[near, 0] + rng.uniform(-8.0, 1.5, int(near.sum())).astype(np.float32)
    s = score64(cls[:, 0], cls[:, 1])
    passing = np.nonzero(s >= t)[0]
    count = len(passing) if len(passing) <= CAND_CAP else -len(passing)
    return cls, passing, count


# ------------------------------------------------------------------------------------------------------------------ rotated IoU cases
PI32 = float(np.float32(math.pi))
_THIN = float(np.float32(1e-3))
_R2 = math.sqrt(2.0)
# (name, box a, box b, closed-form IoU or None, degenerate?)  Closed forms use the fp32 values the kernel receives.
IOU_PAIRS = (
    ("identical", (1, 2, 2, 4, 0.3), (1, 2, 2, 4, 0.3), 1.0, False),
    ("contained", (0, 0, 2, 4, 0.3), (0, 0, 1, 2, 0.3), 0.25, False),
    ("generic", (0, 0, 2, 4, 0.3), (0.5, 0.25, 3, 2, -0.4), None, False),
    ("generic-2", (-3, 1, 4.5, 1.5, 2.0), (-2.5, 0.5, 2, 5, -1.1), None, False),
    ("quarter-turn-same-extents", (0, 0, 2, 4, 0.0), (0, 0, 2, 4, PI32 / 2), 1.0 / 3.0, False),
    ("quarter-turn-swapped-extents", (0, 0, 2, 4, 0.3), (0, 0, 4, 2, 0.3 + PI32 / 2), 1.0, False),
    ("half-turn", (0, 0, 2, 4, 0.3), (0, 0, 2, 4, 0.3 + PI32), 1.0, False),
    ("full-turn", (0, 0, 2, 4, 0.3), (0, 0, 2, 4, 0.3 + 2 * PI32), 1.0, False),
    ("minus-half-turn", (0, 0, 2, 4, -0.3), (0, 0, 2, 4, -0.3 - PI32), 1.0, False),
    ("zero-width", (0, 0, 0, 4, 0.3), (0, 0, 2, 4, 0.3), 0.0, True),
    ("zero-width-second", (0, 0, 2, 4, 0.3), (0.5, 0, 3, 0, 1.0), 0.0, True),
    ("zero-width-both-crossing", (0, 0, 0, 4, 0.0), (0, 0, 4, 0, 0.0), 0.0, True),
    ("both-empty", (1, 1, 0, 0, 0.0), (1, 1, 0, 0, 0.0), 0.0, True),
    ("both-empty-apart", (1, 1, 0, 0, 0.7), (3, 1, 0, 0, 0.0), 0.0, True),
    ("empty-inside-box", (0, 0, 0, 0, 0.0), (0, 0, 2, 4, 0.3), 0.0, True),
    ("box-around-empty", (0, 0, 2, 4, PI32 / 2), (1, 1, 0, 0, 0.0), 0.0, True),      # the clip window is a point: every edge has zero length
    ("box-around-empty-2", (-2.5, 0.5, 2, 5, -1.1), (0, 0, 0, 0, 0.0), 0.0, True),
    ("needles-crossing", (0, 0, _THIN, 5, 0.2), (0, 0, 5, _THIN, 0.2), _THIN * _THIN / (10 * _THIN - _THIN * _THIN), True),
    ("needle-in-box", (0, 0, _THIN, 5, 0.0), (0, 0, 2, 4, 0.0), 4 * _THIN / (5 * _THIN + 8 - 4 * _THIN), True),
    ("needle-on-itself", (0, 0, _THIN, 5, 1.0), (0, 0, _THIN, 5, 1.0), 1.0, True),
    ("shared-edge", (0, 0, 2, 4, 0.0), (2, 0, 2, 4, 0.0), 0.0, True),
    ("shared-edge-partial", (0, 0, 2, 4, 0.0), (2, 1, 2, 4, 0.0), 0.0, True),
    ("shared-edge-turned", (0, 0, 2, 4, PI32 / 2), (0, 2, 2, 4, PI32 / 2), 0.0, True),
    ("corner-contact", (0, 0, 2, 2, 0.0), (2, 2, 2, 2, 0.0), 0.0, True),
    ("corner-on-edge", (0, 0, 2, 2, 0.0), (1 + _R2, 0, 2, 2, PI32 / 4), 0.0, True),
    ("far-1e4", (1e4, -1e4, 2, 4, 0.3), (1e4 + 0.5, -1e4 + 0.25, 3, 2, -0.4), None, False),
    ("far-1e4-identical", (-1e4, 1e4, 2, 4, 0.3), (-1e4, 1e4, 2, 4, 0.3), 1.0, False),
    ("far-1e4-disjoint", (1e4, 1e4, 2, 4, 0.3), (-1e4, 1e4, 2, 4, 0.3), 0.0, False),
)
IOU_TILE_A, IOU_TILE_B, IOU_NA, IOU_NB = 41, 40, 1025, 1024
IOU_GRID_PASS = 4096 * 256            # v2x_rotated_iou's grid: outputs from this flat index on belong to the grid-stride loop


IOU_CASES = IOU_PAIRS                  # ... and the size case of make_iou_size_case()


def iou_pair_arrays():
    a = np.array([p[1] for p in IOU_PAIRS], np.float32)
    b = np.array([p[2] for p in IOU_PAIRS], np.float32)
    return a, b


def rand_boxes(rng, n, spread=3.0, lo=0.5):
    return np.stack([rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n), rng.uniform(lo, 5.0, n), rng.uniform(lo, 5.0, n),
                     rng.uniform(-math.pi, math.pi, n)], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def make_iou_size_case():
    """na = 1025, nb = 1024 from 41 x 40 distinct boxes tiled: -> a, b, the float64 reference of the distinct pairs gathered to (na, nb)."""
    rng = np.random.default_rng(77)
    ta, tb = rand_boxes(rng, IOU_TILE_A), rand_boxes(rng, IOU_TILE_B)
    ia, ib = np.arange(IOU_NA) % IOU_TILE_A, np.arange(IOU_NB) % IOU_TILE_B
    ref = iou_ref64(ta, tb)
    return ta[ia], tb[ib], ref[np.ix_(ia, ib)], (ta, tb, ref)


# ------------------------------------------------------------------------------------------------------------------ matching
def match_ref64(det, nd, gt, ng, thr):
    """mmdet's tpfp_default as match_detections_kernel's header states it: the detections (rows of det, in descending-score order) each take the
    ground truth of HIGHEST rotated IoU (lowest index on ties; an IoU of 0 takes none) and are true positives iff that IoU >= thr and the
    ground truth is still free -- no second choice.  nd, ng are clamped to [0, rows].  -> tp (nd,), best_iou (nd,), runner-up IoU (nd,)
    (the second largest of the row, equal to the best on a tie; 0 with fewer than two ground truths)."""
    det = np.asarray(det, np.float32).reshape(-1, 5)
    gt = np.asarray(gt, np.float32).reshape(-1, 5)
    nd = min(max(int(nd), 0), det.shape[0])
    ng = min(max(int(ng), 0), gt.shape[0])
    cd, cg = corners64(det[:nd]), corners64(gt[:ng])
    sd, sg = standup64(cd), standup64(cg)
    free = np.ones(ng, bool)
    tp, best, second = np.zeros(nd, np.int32), np.zeros(nd), np.zeros(nd)
    for j in range(nd):
        ov = np.nonzero((np.minimum(sd[j, 2], sg[:, 2]) >= np.maximum(sd[j, 0], sg[:, 0])) & (np.minimum(sd[j, 3], sg[:, 3]) >= np.maximum(sd[j, 1], sg[:, 1])))[0]
        b, arg, vals = 0.0, -1, []
        for g in ov:                                         # ascending index: the first maximum is kept
            v = rotated_iou64(cd[j], cg[g])
            vals.append(v)
            if v > b:
                b, arg = v, int(g)
        vals.sort()
        best[j] = b
        second[j] = vals[-2] if len(vals) >= 2 else 0.0
        if arg >= 0 and b >= thr and free[arg]:
            free[arg] = False
            tp[j] = 1
    return tp, best, second


MATCH_MARGIN = 1e-6
# (name, gt_cap, det_cap, thr, images); an image = dict(ng, nd, and optionally dup=(p, q), det_count, gt_count, hand)
MATCH_CASES = (
    ("small", 8, 12, 0.5, (dict(ng=0, nd=5), dict(ng=1, nd=4), dict(ng=2, nd=6), dict(ng=8, nd=12, det_count=12 + 9),
                           dict(ng=8, nd=0, det_count=-3), dict(ng=0, nd=7, gt_count=-1), dict(ng=8, nd=9, gt_count=8 + 1, next_bait=True),
                           dict(ng=5, nd=8))),
    ("threshold-one", 4, 4, 1.0, (dict(hand="identical"), dict(ng=3, nd=4))),
    ("threshold-quarter", 4, 4, 0.25, (dict(hand="contained"), dict(ng=4, nd=4))),
    ("strided", 600, 16, 0.5, (dict(ng=255, nd=14), dict(ng=256, nd=14, dup=(254, 255)), dict(ng=257, nd=14, dup=(255, 256)), dict(ng=513, nd=16, dup=(5, 300)),
                               dict(ng=513, nd=16, dup=(7, 263)), dict(ng=600, nd=12, gt_count=600 + 1, next_bait=True), dict(ng=2, nd=5),
                               dict(ng=513, nd=12, mirror=(5, 300)), dict(ng=257, nd=10, mirror=(255, 256)), dict(ng=513, nd=9, mirror=(7, 263)))),
    ("gt-cap-8192", 8192, 16, 0.5, (dict(ng=8192, nd=16, dup=(5, 300)), dict(ng=8192, nd=8, gt_count=8192 + 1, next_bait=True, dup=(255, 256)), dict(ng=1, nd=3),
                                    dict(ng=8192, nd=8, mirror=(77, 8000)))),
    ("strided-thr075", 600, 16, 0.75, (dict(ng=513, nd=16, dup=(255, 256)), dict(ng=257, nd=10))),
)


def _gt_field(rng, n):
    """n ground truths on a lattice of pitch 7 m (jitter 1 m, sizes 1 - 5 m, any yaw): neighbours may touch, most pairs are far apart."""
    nx = max(1, int(math.ceil(math.sqrt(max(n, 1)))))
    i = np.arange(n)
    g = rand_boxes(rng, n, spread=1.0, lo=1.0)
    g[:, 0] += ((i % nx) * 7.0).astype(np.float32)
    g[:, 1] += ((i // nx) * 7.0).astype(np.float32)
    return g


def _perturbed(rng, box):
    d = box.astype(np.float64).copy()
    d[:2] += rng.normal(0, 0.35, 2)
    d[2:4] *= rng.uniform(0.85, 1.2, 2)
    d[4] += rng.normal(0, 0.12)
    return d.astype(np.float32)


def _match_image(rng, spec, gt_cap, det_cap, thr, gt0=None):
    det = np.zeros((det_cap, 5), np.float32)
    gt = np.zeros((gt_cap, 5), np.float32)
    if "hand" in spec:
        gt[:2] = [[0, 0, 2, 4, 0.0], [9, 0, 2, 4, 0.0]]
        if spec["hand"] == "identical":       # identical boxes: IoU exactly 1 = thr; the second detection on it finds it taken
            det[:3] = [[0, 0, 2, 4, 0.0], [0, 0, 2, 4, 0.0], [9, 0.5, 2, 4, 0.0]]
        else:                                 # a 1 x 2 inside a 2 x 4, both at yaw 0: 2 / 8 = 0.25 exactly
            det[:3] = [[0.25, -0.5, 1, 2, 0.0], [9, 0, 1, 1, 0.0], [9.25, 0.5, 1, 2, 0.0]]
        return det, gt, 3, 2
    ng, nd = spec["ng"], spec["nd"]
    gt[:ng] = _gt_field(rng, ng)
    if gt0 is not None:
        gt[0] = gt0
    ext = 7.0 * math.ceil(math.sqrt(max(ng, 1)))
    dup = spec.get("dup")
    forced = {}
    if dup:                                   # two detections ON the duplicated pair: the first takes the lower index, the second has no second choice
        gt[dup[1]] = gt[dup[0]]
        at = sorted(rng.choice(nd - 1, 2, replace=False).tolist())
        forced = {at[0]: gt[dup[0]].copy(), at[1]: gt[dup[0]].copy()}
    mirror = spec.get("mirror")
    if mirror:
        # Identical duplicates cannot show WHICH of them a detection took (every later detection ties on them again and follows the first).
        # Two DIFFERENT ground truths, mirror images about a detection, can: 2 x 4 boxes at yaw 0, 0.5 m left and right of it, dyadic
        # coordinates -- both IoUs are 6 / 10 to the bit.  The detection takes the lower index p; one sitting on q then finds q free (true
        # positive) and one sitting on p finds it taken -- with the higher index taken first, those two flags swap.
        p_, q_ = mirror
        gt[p_], gt[q_] = (MIRROR_AT[0] - 0.5, MIRROR_AT[1], 2, 4, 0), (MIRROR_AT[0] + 0.5, MIRROR_AT[1], 2, 4, 0)
        at = sorted(rng.choice(nd - 1, 3, replace=False).tolist())
        forced.update({at[0]: np.array((MIRROR_AT[0], MIRROR_AT[1], 2, 4, 0), np.float32), at[1]: gt[q_].copy(), at[2]: gt[p_].copy()})
    if spec.get("next_bait"):                 # the last detection is far from every ground truth of its own image
        forced[nd - 1] = np.array(BAIT, np.float32)
    for j in range(nd):
        for _ in range(50):
            if j in forced:
                d = forced[j]
                break
            if ng and rng.random() < 0.8:
                d = _perturbed(rng, gt[int(rng.integers(0, ng))])      # several detections may pick the same ground truth
            else:
                d = rand_boxes(rng, 1, spread=1.0, lo=1.0)[0]
                d[:2] = rng.uniform(0.0, ext, 2)
            _, b, s = match_ref64(d[None], 1, gt, ng, thr)
            if (b[0] - s[0] >= 10 * MATCH_MARGIN or b[0] == s[0]) and abs(b[0] - thr) >= 10 * MATCH_MARGIN:
                break
        else:
            raise AssertionError("no detection with a margin found")
        det[j] = d
    # rows past the counts: boxes that WOULD match if the kernel read them
    if ng < gt_cap and nd:
        gt[ng:] = det[0]
    if nd < det_cap and ng:
        det[nd:] = gt[0]
    return det, gt, spec.get("det_count", nd), spec.get("gt_count", ng)


BAIT = (-500.0, -500.0, 2.0, 4.0, 0.5)
MIRROR_AT = (-100.0, -100.0)


@functools.lru_cache(maxsize=None)
def make_match_case(index):
    """-> det (n, det_cap, 5), det_count (n,), gt (n, gt_cap, 5), gt_count (n,), thr, refs [(tp, best, second)] per image.  The counts are
    the RAW ones handed to the kernel (negative and beyond the capacity included).  next_bait: the image whose gt_count is gt_cap + 1 ends
    with a detection far from all its ground truths, and the NEXT image's first ground truth -- the row an unclamped count would reach --
    is that very box."""
    name, gt_cap, det_cap, thr, images = MATCH_CASES[index]
    rng = np.random.default_rng(4000 + index)
    dets, gts, dcs, gcs = [], [], [], []
    for i, spec in enumerate(images):
        bait = np.array(BAIT, np.float32) if i and images[i - 1].get("next_bait") else None
        d, g, dc, gc = _match_image(rng, spec, gt_cap, det_cap, thr, gt0=bait)
        dets.append(d), gts.append(g), dcs.append(dc), gcs.append(gc)
    det, gt = np.stack(dets), np.stack(gts)
    dc, gc = np.array(dcs, np.int32), np.array(gcs, np.int32)
    refs = [match_ref64(det[i], dc[i], gt[i], gc[i], thr) for i in range(len(images))]
    return det, dc, gt, gc, thr, refs

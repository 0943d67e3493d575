"""float64 reference and the seeded case table for v2x_det_map (csrc/det_map.hip): the AP table of a split -- all maps, all agents (groups), all IoU
thresholds -- in one call.  A plain helper module (as tests/post_refs.py): tests/test_det_map_refs_cpu.py checks the reference against
oracle/postprocess_ref.py::eval_map and utils/postprocess.py::eval_map and the condition below without a GPU, tests/test_gpu_det_map.py holds the
kernels to it.  numpy and math only; every case is seeded.

The reference, from the definition: the true-positive flags of every map are post_refs.match_ref64's, per threshold (the
greedy walk restarts per threshold: one "taken" set each); the ranked list of a group is numpy's stable argsort of the negated scores over the
image-major concatenation of its maps; AP is mmdet's "area" mode with the sum taken exactly (math.fsum).

CONDITION (asserted by make_case, never a measurement): every detection's reference best IoU is at least post_refs.MATCH_MARGIN away from every
threshold of its case and from its runner-up.  The designed exact ties are the only exceptions and are declared per map (`exact`): identical
duplicate ground truths, the dyadic "mirror" pair, and the "identical" / "contained" hand images of post_refs, where best == runner-up or
best == threshold TO THE BIT."""
import functools
import math

import numpy as np

import post_refs as PR

NAN = float("nan")
CHUNK = 1024          # csrc/det_map.hip: DET_MAP_CHUNK, the positions one step of the AP walk takes (256 threads x 4)
WAVE, BLOCK = 64, 256  # ... the shuffle scans' width and the threads of the walk
LIST_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097)
BOUNDARIES = (64, 256, 1024, 2048, 4096)


# ------------------------------------------------------------------------------------------------------------------ reference
def ap_ref64(scores, tps, num_gt):
    """mmdet 'area' AP of one group: scores, tps image-major (per map in ranked order), from the definition.  -> (ap, order)."""
    scores = np.asarray(scores, np.float64)
    order = np.argsort(-scores, kind="stable")
    if num_gt == 0 or scores.size == 0:
        return 0.0, order
    f = np.asarray(tps, np.int64)[order]
    tp = np.cumsum(f)
    prec = tp / np.arange(1, f.size + 1)
    env = np.maximum.accumulate(prec[::-1])[::-1]
    terms = [(int(tp[i]) / num_gt - (int(tp[i]) - 1) / num_gt) * float(env[i]) for i in np.nonzero(f)[0]]
    return math.fsum(terms), order


def reference(det, scores, det_count, gt, gt_count, group, thrs, n_groups):
    n, det_cap = scores.shape
    T = len(thrs)
    nd = np.clip(det_count, 0, det_cap).astype(np.int64)
    ng = np.clip(gt_count, 0, gt.shape[1]).astype(np.int64)
    tp = np.zeros((T, n, det_cap), np.uint8)
    best, second = np.zeros((n, det_cap)), np.zeros((n, det_cap))
    for i in range(n):
        for t, thr in enumerate(thrs):
            f, b, s = PR.match_ref64(det[i], det_count[i], gt[i], gt_count[i], float(np.float32(thr)))
            tp[t, i, :nd[i]] = f
            best[i, :nd[i]], second[i, :nd[i]] = b, s
    rank = np.full((n, det_cap), -1, np.int32)
    ap, num_tp = np.zeros((n_groups, T)), np.zeros((n_groups, T), np.int64)
    num_gt, num_det = np.zeros(n_groups, np.int64), np.zeros(n_groups, np.int64)
    for g in range(n_groups):
        maps = [i for i in range(n) if group[i] == g]
        where = [(i, j) for i in maps for j in range(nd[i])]
        num_gt[g], num_det[g] = int(sum(ng[i] for i in maps)), len(where)
        sc = np.array([scores[i, j] for i, j in where], np.float64)
        for t in range(T):
            flags = np.array([tp[t, i, j] for i, j in where], np.int64)
            ap[g, t], order = ap_ref64(sc, flags, int(num_gt[g]))
            num_tp[g, t] = int(flags.sum())
        for pos, k in enumerate(np.argsort(-sc, kind="stable")):
            rank[where[k]] = pos
    return {"tp": tp, "rank": rank, "ap": ap, "num_gt": num_gt, "num_det": num_det, "num_tp": num_tp, "best": best, "second": second}


# ------------------------------------------------------------------------------------------------------------------ assembling a case
def _assemble(maps, thrs, n_groups, det_cap, gt_cap):
    """maps: dict(det (m, 5), scores (m,), gt (k, 5), group[, det_count, gt_count (the RAW counts handed over), exact, garbage]).  Every map is put
    in stable descending score order (the entry's contract); rows past the counts are NaN sentinels."""
    n = len(maps)
    det, sc = np.full((n, det_cap, 5), NAN, np.float32), np.full((n, det_cap), NAN, np.float32)
    gt = np.full((n, gt_cap, 5), NAN, np.float32)
    dc, gc, gr = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i, m in enumerate(maps):
        d, s, g = np.asarray(m["det"], np.float32).reshape(-1, 5), np.asarray(m["scores"], np.float32).reshape(-1), np.asarray(m["gt"], np.float32).reshape(-1, 5)
        assert len(d) == len(s) <= det_cap and len(g) <= gt_cap
        if not m.get("garbage"):
            order = np.argsort(-s, kind="stable")
            d, s = d[order], s[order]
        det[i, :len(s)], sc[i, :len(s)], gt[i, :len(g)] = d, s, g
        dc[i], gc[i], gr[i] = m.get("det_count", len(s)), m.get("gt_count", len(g)), m["group"]
        assert dc[i] == len(s) or (len(s) == det_cap and dc[i] > det_cap) or (len(s) == 0 and dc[i] < 0)
        assert gc[i] == len(g) or (len(g) == gt_cap and gc[i] > gt_cap) or (len(g) == 0 and gc[i] < 0)
    case = {"det": det, "scores": sc, "det_count": dc, "gt": gt, "gt_count": gc, "group": gr, "thrs": tuple(thrs), "n_groups": n_groups,
            "det_cap": det_cap, "gt_cap": gt_cap, "exact": np.array([bool(m.get("exact")) for m in maps], bool)}
    case["ref"] = reference(det, sc, dc, gt, gc, gr, thrs, n_groups) if n else {
        "tp": np.zeros((len(thrs), 0, det_cap), np.uint8), "rank": np.zeros((0, det_cap), np.int32), "ap": np.zeros((n_groups, len(thrs))),
        "num_gt": np.zeros(n_groups, np.int64), "num_det": np.zeros(n_groups, np.int64), "num_tp": np.zeros((n_groups, len(thrs)), np.int64),
        "best": np.zeros((0, det_cap)), "second": np.zeros((0, det_cap))}
    check_condition(case)
    return case


def check_condition(case):
    """The module's CONDITION; raises AssertionError naming the detection that misses it.  -> the smallest distances met (threshold, runner-up)."""
    ref, worst_thr, worst_second = case["ref"], math.inf, math.inf
    nd = np.clip(case["det_count"], 0, case["det_cap"])
    for i in range(len(nd)):
        live = 0 <= case["group"][i] < case["n_groups"]
        if live:
            assert np.isfinite(case["scores"][i, :nd[i]]).all(), "map %d: a counted score is not finite" % i
            assert (np.diff(case["scores"][i, :nd[i]].astype(np.float64)) <= 0).all(), "map %d is not in descending score order" % i
        for j in range(nd[i]):
            b, s = ref["best"][i, j], ref["second"][i, j]
            for thr in case["thrs"]:
                thr = float(np.float32(thr))
                if not (case["exact"][i] and b == thr):
                    assert abs(b - thr) >= PR.MATCH_MARGIN, "map %d detection %d: best IoU %.9f against threshold %g" % (i, j, b, thr)
                    worst_thr = min(worst_thr, abs(b - thr))
            if not (case["exact"][i] and b == s) and b > 0:
                assert b - s >= PR.MATCH_MARGIN, "map %d detection %d: best IoU %.9f, runner-up %.9f" % (i, j, b, s)
                worst_second = min(worst_second, b - s)
    return worst_thr, worst_second


# ------------------------------------------------------------------------------------------------------------------ box builders
def _gt_row(rng, k):
    """k ground truths 12 m apart on a line (sizes 2 - 5 m, any yaw): no two of them, and no detection built on one, reach another."""
    g = PR.rand_boxes(rng, k, spread=0.5, lo=2.0)
    g[:, 0] += 12.0 * np.arange(k, dtype=np.float32)
    return g


def _on(gt_box, f):
    """A detection inside gt_box with the width scaled by f < 1: IoU = f up to the rounding of the product."""
    d = np.array(gt_box, np.float32)
    d[2] = np.float32(d[2] * f)
    return d


FAR = np.array((-300.0, 40.0, 2.0, 4.0, 0.3), np.float32)       # a false positive at every threshold: reaches no ground truth


def _far(k):
    d = FAR.copy()
    d[1] += 9.0 * k
    return d


def _pattern_group(rng, flags, group, per_map, fmid=False):
    """Maps of one group whose RANKED list carries flags[pos] (1: true positive at every threshold of (0.5, 0.7), 0: false positive, 2 with fmid: IoU
    ~0.6, true positive at 0.5 only): position pos goes to map pos % n_maps with score 1 - pos * 2^-14 (exact in fp32, strictly descending)."""
    L = len(flags)
    n_maps = max(1, -(-L // per_map))
    maps = [{"det": [], "scores": [], "gt": None, "group": group} for _ in range(n_maps)]
    for pos, f in enumerate(flags):
        maps[pos % n_maps]["scores"].append(1.0 - pos * 2.0 ** -14)
        maps[pos % n_maps]["det"].append(f)
    for m in maps:
        kinds = m["det"]
        g = _gt_row(rng, sum(1 for f in kinds if f) + 1)             # one ground truth stays unmatched
        det, k = [], 0
        for q, f in enumerate(kinds):
            if f:
                det.append(_on(g[k], rng.uniform(0.55, 0.65) if f == 2 else rng.uniform(0.76, 0.95)))
                k += 1
            else:
                det.append(_far(q))
        m["det"], m["gt"] = np.array(det, np.float32).reshape(-1, 5), g
    return maps


def _length_flags(rng, L):
    """A ranked list of L flags: random, and across every boundary b < L + 3 a run of false positives [b - 6, b - 2) followed by a run of true
    positives [b - 2, b + 3): the suffix maximum of the precision and the recall's steps both cross b."""
    f = (rng.random(L) < 0.45).astype(np.int64)
    f[rng.random(L) < 0.1] = 2
    for b in BOUNDARIES:
        for pos in range(b - 6, b + 3):
            if 0 <= pos < L:
                f[pos] = 0 if pos < b - 2 else 1
    return f.tolist()


def _interleave(a, b):
    out = []
    for k in range(max(len(a), len(b))):
        out += a[k:k + 1] + b[k:k + 1]
    return out


def _garbage(det_cap, gt_cap, boxes_too):
    """A map outside every group (group = -1) whose scores are NaN: never read.  boxes_too: its boxes are NaN as well (it matches nothing)."""
    rng = np.random.default_rng(99)
    g = _gt_row(rng, min(2, gt_cap))
    d = np.array([_on(g[0], 0.9), _far(0)][:min(2, det_cap)], np.float32)
    if boxes_too:
        d[:] = NAN
    return {"det": d, "scores": np.full(len(d), NAN, np.float32), "gt": g, "group": -1, "garbage": True}


# ------------------------------------------------------------------------------------------------------------------ the cases
def _case_empty():
    return _assemble([], (0.5, 0.7), 2, 4, 4)


def _case_degenerate():
    rng = np.random.default_rng(7001)
    g = _gt_row(rng, 3)
    none = np.zeros((0, 5), np.float32)
    maps = [{"det": none, "scores": [], "gt": g, "group": 0},                                                   # ground truths, no detections
            {"det": [_far(0), _far(1), _on(g[0], 0.9)], "scores": [0.9, 0.8, 0.7], "gt": none, "group": 1},      # detections, num_gt = 0
            # group 2: no maps at all
            {"det": [_on(g[1], 0.9)], "scores": [0.6], "gt": g[1:2], "group": 3},                                # one on one: a hit ...
            {"det": [_far(0)], "scores": [0.6], "gt": g[1:2], "group": 4}]                                       # ... and a miss
    return _assemble(maps, (0.5, 0.7), 5, 4, 4)


def _case_taken(thrs):
    """A (IoU ~0.6) and then B (IoU ~0.8) on the same ground truth: at 0.5 A takes it and B is a false positive, at 0.7 A falls short and B is the
    true positive.  ONE taken set shared by the thresholds gets B wrong at 0.7 (or at 0.5, with the thresholds the other way round)."""
    rng = np.random.default_rng(7002)
    g = _gt_row(rng, 3)
    maps = [{"det": [_on(g[0], 0.61), _on(g[0], 0.83), _on(g[1], 0.9), _far(0), _on(g[2], 0.58), _on(g[2], 0.62)],
             "scores": [0.95, 0.9, 0.85, 0.8, 0.75, 0.7], "gt": g, "group": 0},
            {"det": [_on(g[1], 0.6), _on(g[1], 0.9), _on(g[1], 0.8)], "scores": [0.93, 0.88, 0.5], "gt": g[:2], "group": 0}]
    return _assemble(maps, thrs, 1, 8, 4)


def _case_hand(hand, thr):
    rng = np.random.default_rng(7003)
    det, gt, nd, ng = PR._match_image(rng, {"hand": hand}, 4, 4, thr)
    g = _gt_row(rng, 2)
    maps = [{"det": det[:nd], "scores": [0.9, 0.8, 0.7], "gt": gt[:ng], "group": 0, "exact": True},
            {"det": [_on(g[0], 0.9), _far(0), _on(g[1], 0.12)], "scores": [0.85, 0.8, 0.75], "gt": g, "group": 0}]
    return _assemble(maps, (thr,), 1, 4, 4)


def _case_eight():
    rng = np.random.default_rng(7004)
    thrs = (0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85)
    fs = (0.52, 0.58, 0.62, 0.68, 0.72, 0.78, 0.82, 0.9, 0.3)
    maps = []
    for i in range(3):
        g = _gt_row(rng, 5)
        picks = rng.permutation(len(fs))
        det = [_on(g[k % 4], fs[p]) for k, p in enumerate(picks)]          # several per ground truth, weakest and strongest in any order
        maps.append({"det": det, "scores": rng.permutation(len(det)) * 0.1 + 0.05 * i, "gt": g, "group": i % 2})
    return _assemble(maps, thrs, 2, 16, 8)


def _tie_maps(rng, scores_per_map, groups):
    maps = []
    for sc, grp in zip(scores_per_map, groups):
        g = _gt_row(rng, 3)
        det = [(_on(g[k % 3], rng.uniform(0.76, 0.95)) if rng.random() < 0.6 else _far(k)) for k in range(len(sc))]
        maps.append({"det": det, "scores": sc, "gt": g, "group": grp})
    return maps


def _case_ties():
    rng = np.random.default_rng(7005)
    sc = [[0.9, 0.5, 0.5, 0.5, 0.2], [0.5, 0.5, 0.4], [0.9, 0.9, 0.5, 0.2, 0.2], [0.5, 0.2], [0.5], [0.9, 0.5, 0.5]]
    return _assemble(_tie_maps(rng, sc, [0, 1, 0, 1, 0, 1]), (0.5, 0.7), 2, 8, 4)


def _case_all_equal():
    rng = np.random.default_rng(7006)
    sc = [[0.5] * k for k in (3, 1, 5, 0, 2, 4, 7)]
    return _assemble(_tie_maps(rng, sc, [0, 1, 0, 0, 1, 0, 1]), (0.5, 0.7), 2, 8, 4)


def _case_signed_zero():
    rng = np.random.default_rng(7007)
    sc = [[0.25, -0.0, 0.0, -0.5], [0.0, -0.0, -0.25], [-0.0], [0.0, 0.0, -0.0, -0.0], [0.5, -0.0, -1.0]]
    return _assemble(_tie_maps(rng, sc, [0, 0, 0, 1, 0]), (0.5, 0.7), 2, 4, 4)


def _case_interleaved(frame_major):
    rng = np.random.default_rng(7008)
    sc = [np.round(rng.uniform(0.1, 0.9, int(k)), 1) for k in rng.integers(1, 7, 12)]       # one decimal: ties across maps and groups
    groups = [k % 3 for k in range(12)] if frame_major else [k // 4 for k in range(12)]
    maps = _tie_maps(rng, sc, groups)
    maps.insert(5, _garbage(8, 4, True))
    maps.insert(0, _garbage(8, 4, False))
    maps.append(_garbage(8, 4, True))
    return _assemble(maps, (0.5, 0.7), 3, 8, 4)


def _case_padding():
    """NaN sentinels past every count (all cases have them), det_count > det_cap, negative counts, gt_count > gt_cap."""
    rng = np.random.default_rng(7009)
    det_cap, gt_cap = 6, 3
    g = _gt_row(rng, 3)
    full = [_on(g[0], 0.9), _on(g[1], 0.6), _far(0), _on(g[2], 0.8), _far(1), _on(g[0], 0.85)]
    none = np.zeros((0, 5), np.float32)
    maps = [{"det": full, "scores": [0.9, 0.8, 0.7, 0.6, 0.5, 0.4], "gt": g, "group": 0, "det_count": det_cap + 5, "gt_count": gt_cap + 2},
            {"det": none, "scores": [], "gt": g[:2], "group": 0, "det_count": -3},
            {"det": full[:3], "scores": [0.85, 0.8, 0.3], "gt": none, "group": 1, "gt_count": -1},
            {"det": full[:4], "scores": [0.75, 0.7, 0.6, 0.6], "gt": g[:2], "group": 1},
            {"det": none, "scores": [], "gt": none, "group": 0, "det_count": -1, "gt_count": -7}]
    return _assemble(maps, (0.5, 0.7), 2, det_cap, gt_cap)


def _case_length(L):
    """A group whose ranked list has L detections (the chunk, block and wave widths of the AP walk and one past each), its maps interleaved with a
    second, short group's; per_map = 61 detections (odd: the searches end at every depth)."""
    rng = np.random.default_rng(7100 + L)
    a = _pattern_group(rng, _length_flags(rng, L), 0, 61, fmid=True)
    b = _pattern_group(rng, _length_flags(rng, 7), 1, 3, fmid=True)
    return _assemble(_interleave(a, b), (0.5, 0.7), 2, 64, 64)


def _case_wide_maps():
    """Maps with MORE detections than the 64 lanes that rank a map (195: three full passes and a partial one) beside short ones, det_cap 200."""
    rng = np.random.default_rng(7400)
    a = _pattern_group(rng, _length_flags(rng, 390), 0, 195, fmid=True)
    b = _pattern_group(rng, _length_flags(rng, 131), 1, 66, fmid=True)
    return _assemble(_interleave(a, b), (0.5, 0.7), 2, 200, 160)


def _field_map(rng, ng, nd, group, thrs):
    """A map from post_refs-style fields: ng ground truths on the 7 m lattice, detections perturbed from them or dropped anywhere, each drawn again
    (seeded: part of the case's definition) until it keeps ten margins from every threshold and from its runner-up."""
    gt = PR._gt_field(rng, ng)
    ext = 7.0 * math.ceil(math.sqrt(max(ng, 1)))
    det = []
    for _ in range(nd):
        for _ in range(50):
            if ng and rng.random() < 0.8:
                d = PR._perturbed(rng, gt[int(rng.integers(0, ng))])
            else:
                d = PR.rand_boxes(rng, 1, spread=1.0, lo=1.0)[0]
                d[:2] = rng.uniform(0.0, ext, 2)
            _, b, s = PR.match_ref64(d[None], 1, gt, ng, 0.5)
            if (b[0] - s[0] >= 10 * PR.MATCH_MARGIN or b[0] == 0.0) and all(abs(b[0] - float(np.float32(t))) >= 10 * PR.MATCH_MARGIN for t in thrs):
                break
        else:
            raise AssertionError("no detection with a margin found")
        det.append(d)
    scores = np.round(rng.uniform(0.7, 1.0, nd), 3)           # three decimals: a few ties across the maps of a group
    return {"det": np.array(det, np.float32).reshape(-1, 5), "scores": scores, "gt": gt, "group": group}


SCALE_GROUPS, SCALE_MAPS = 5, 40


def _case_scale():
    """5 groups x 40 maps x about 30 detections on about 20 ground truths, frame-major (the tool's order)."""
    rng = np.random.default_rng(7200)
    maps = [_field_map(rng, int(rng.integers(15, 26)), int(rng.integers(22, 39)), g, (0.5, 0.7)) for _ in range(SCALE_MAPS) for g in range(SCALE_GROUPS)]
    return _assemble(maps, (0.5, 0.7), SCALE_GROUPS, 64, 64)


def _case_gt_cap():
    """gt_cap = 8192, 3 maps: the strided search with every row in use, a duplicated pair (exact tie: the lower index) and the dyadic mirror pair."""
    maps = []
    for i, spec in enumerate((dict(ng=8192, nd=6, dup=(5, 300)), dict(ng=8192, nd=5, mirror=(77, 8000)), dict(ng=3, nd=4))):
        rng = np.random.default_rng(7300 + i)
        det, gt, nd, ng = PR._match_image(rng, spec, 8192, 8, 0.5)
        # _match_image keeps its margins from 0.5 only: the thresholds of this case are chosen away from the IoUs it drew (checked by _assemble)
        maps.append({"det": det[:nd], "scores": np.linspace(0.9, 0.4, nd) + 0.01 * i, "gt": gt[:ng], "group": i % 2, "exact": "dup" in spec or "mirror" in spec})
    return _assemble(maps, (0.5, 0.7), 2, 8, 8192)


CASES = {
    "empty": _case_empty,
    "degenerate": _case_degenerate,
    "taken-0.5-0.7": lambda: _case_taken((0.5, 0.7)),
    "taken-0.7-0.5": lambda: _case_taken((0.7, 0.5)),
    "taken-0.5-0.5-0.7": lambda: _case_taken((0.5, 0.5, 0.7)),
    "threshold-one": lambda: _case_hand("identical", 1.0),
    "threshold-quarter": lambda: _case_hand("contained", 0.25),
    "eight-thresholds": _case_eight,
    "ties": _case_ties,
    "all-equal": _case_all_equal,
    "signed-zero": _case_signed_zero,
    "interleaved-agent-major": lambda: _case_interleaved(False),
    "interleaved-frame-major": lambda: _case_interleaved(True),
    "padding": _case_padding,
    "wide-maps": _case_wide_maps,
    "scale": _case_scale,
    "gt-cap-8192": _case_gt_cap,
}
CASES.update({"length-%d" % L: (lambda L=L: _case_length(L)) for L in LIST_LENGTHS})
CASE_NAMES = tuple(CASES)
HOST_MAX_DET = 700          # cases with at most this many detections are also scored by the two host implementations of eval_map


@functools.lru_cache(maxsize=None)
def make_case(name):
    """-> dict(det, scores, det_count, gt, gt_count, group (the RAW arrays handed to the entry), thrs, n_groups, det_cap, gt_cap, exact, ref).
    Raises AssertionError when the module's CONDITION does not hold.  Cached: the arrays are shared, nobody writes to them."""
    case = CASES[name]()
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def host_lists(case, g):
    """Group g of a case as the host implementations take it: per map dict(boxes, corners, scores) and the (G, 4, 2) ground-truth corners."""
    nd, ng = np.clip(case["det_count"], 0, case["det_cap"]), np.clip(case["gt_count"], 0, case["gt_cap"])
    dets, gts = [], []
    for i in np.nonzero(case["group"] == g)[0]:
        b = case["det"][i, :nd[i]]
        dets.append({"boxes": b, "corners": PR.corners64(b), "scores": case["scores"][i, :nd[i]]})
        gts.append(PR.corners64(case["gt"][i, :ng[i]]))
    return dets, gts

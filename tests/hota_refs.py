"""Float64 reference of the HOTA family (row f-5; TrackEval's hota.py as DESIGN.md section 3 freezes it) and the seeded cases the tests share.  A plain
numpy statement that shares no code with the product; its assignment is track_refs.assign_max, its similarity track_refs.iou_xyxy.

* A frame is (gt_boxes [n][4], gt_ids [n], trk_boxes [m][4], trk_ids [m]); boxes are rounded to float32 first (what the product is given), everything
  after that is float64.  Ids may be any integers: they are renumbered per sequence in order of first appearance.
* `score_sequence` -> the per-alpha counts and sums of one sequence, `finalize` the derived fields, `combine` the rule for several sequences,
  `summary` the means over alpha.
* `make_frames(seed, n_obj, n_frames)`: track_refs.make_case tracked by track_refs.SortRef on the CPU (no GPU tracker in the loop); ground-truth id =
  object index, track ids renumbered in order of first appearance.
* A case is KEPT iff (a) the pairs of every frame's assignment that carry a positive score are the same under three reruns with every similarity
  perturbed by a relative U(-1e-9, 1e-9), and (b) no such pair's similarity lies within 1e-7 of a threshold: a correct fp64 implementation with another
  summation order cannot decide such a case differently.  At most one case in eight may be dropped (`kept_cases` asserts it).
"""
import functools

import numpy as np

import track_refs as R

ALPHAS = np.arange(0.05, 0.99, 0.05)
EPS = np.finfo(np.float64).eps
PERTURB = 1e-9
MARGIN = 1e-7
FIELDS = ("HOTA", "DetA", "AssA", "DetRe", "DetPr", "AssRe", "AssPr", "LocA")
CASES = [(s, 12, 24) for s in range(8)] + [(s, 40, 30) for s in range(4)] + [(s, 60, 12) for s in range(4)]


def similarity(gt_boxes, trk_boxes):
    s = R.iou_xyxy(np.asarray(gt_boxes, dtype=np.float32).reshape(-1, 4), np.asarray(trk_boxes, dtype=np.float32).reshape(-1, 4))
    s[~np.isfinite(s)] = 0.0
    return s


def score_sequence(frames, alphas=ALPHAS, perturb_rng=None):
    """-> {"TP", "FN", "FP": int64 [A]; "AssA", "AssRe", "AssPr", "loc": float64 [A]; "matches": per frame [(gt id, track id, S, score)]; "n_gt_ids",
    "n_trk_ids"}."""
    gmap, tmap, fr = {}, {}, []
    for gb, gi, tb, ti in frames:
        g = np.array([gmap.setdefault(int(i), len(gmap)) for i in gi], dtype=np.int64)
        t = np.array([tmap.setdefault(int(i), len(tmap)) for i in ti], dtype=np.int64)
        assert len(set(g.tolist())) == len(g) and len(set(t.tolist())) == len(t), "an id twice in one frame"
        S = similarity(gb, tb)
        if perturb_rng is not None:
            S = S * (1.0 + perturb_rng.uniform(-PERTURB, PERTURB, S.shape))
        fr.append((g, t, S))
    NG, NT, A = len(gmap), len(tmap), len(alphas)
    # pass 1: the global alignment score
    pot = np.zeros((NG, NT))
    gt_cnt = np.zeros(NG)
    trk_cnt = np.zeros(NT)
    for g, t, S in fr:
        gt_cnt[g] += 1
        trk_cnt[t] += 1
        if len(g) and len(t):
            den = S.sum(0)[None, :] + S.sum(1)[:, None] - S
            J = np.zeros_like(S)
            m = den > EPS
            J[m] = S[m] / den[m]
            pot[g[:, None], t[None, :]] += J
    gas = pot / (gt_cnt[:, None] + trk_cnt[None, :] - pot)             # every id occurs: the denominator is >= 1
    # pass 2: the frames, independent of each other
    TP, FN, FP = (np.zeros(A, dtype=np.int64) for _ in range(3))
    loc = np.zeros(A)
    mc = np.zeros((A, NG, NT))
    matches = []
    for g, t, S in fr:
        if len(g) == 0:
            FP += len(t)
            matches.append([])
            continue
        if len(t) == 0:
            FN += len(g)
            matches.append([])
            continue
        score = gas[g[:, None], t[None, :]] * S
        pairs = R.assign_max(score)
        assert len(pairs) == min(len(g), len(t))
        rows = np.array([r for r, _ in pairs], dtype=np.int64)
        cols = np.array([c for _, c in pairs], dtype=np.int64)
        ms = S[rows, cols]
        matches.append([(int(g[r]), int(t[c]), float(S[r, c]), float(score[r, c])) for r, c in pairs])
        for a, alpha in enumerate(alphas):
            ok = ms >= alpha - EPS
            m = int(ok.sum())
            TP[a] += m
            FN[a] += len(g) - m
            FP[a] += len(t) - m
            loc[a] += ms[ok].sum()
            mc[a, g[rows[ok]], t[cols[ok]]] += 1
    tp1 = np.maximum(1, TP)
    sq = mc * mc
    return {"TP": TP, "FN": FN, "FP": FP, "loc": loc, "matches": matches, "n_gt_ids": NG, "n_trk_ids": NT,
            "AssA": (sq / np.maximum(1, gt_cnt[None, :, None] + trk_cnt[None, None, :] - mc)).sum((1, 2)) / tp1,
            "AssRe": (sq / np.maximum(1, gt_cnt)[None, :, None]).sum((1, 2)) / tp1,
            "AssPr": (sq / np.maximum(1, trk_cnt)[None, None, :]).sum((1, 2)) / tp1}


def finalize(r):
    """The derived per-alpha fields of a sequence or of a combination."""
    TP, FN, FP = (r[k].astype(np.float64) for k in ("TP", "FN", "FP"))
    out = {k: r[k] for k in ("TP", "FN", "FP", "loc", "AssA", "AssRe", "AssPr")}
    out["LocA"] = np.maximum(1e-10, r["loc"]) / np.maximum(1e-10, TP)
    out["DetRe"] = TP / np.maximum(1, TP + FN)
    out["DetPr"] = TP / np.maximum(1, TP + FP)
    out["DetA"] = TP / np.maximum(1, TP + FN + FP)
    out["HOTA"] = np.sqrt(out["DetA"] * out["AssA"])
    return out


def combine(seqs):
    """Integer fields add, the association fields are TP-weighted means, loc adds; the rest is recomputed."""
    TP = sum(s["TP"] for s in seqs)
    out = {"TP": TP, "FN": sum(s["FN"] for s in seqs), "FP": sum(s["FP"] for s in seqs), "loc": sum(s["loc"] for s in seqs)}
    for k in ("AssA", "AssRe", "AssPr"):
        out[k] = sum(s[k] * s["TP"] for s in seqs) / np.maximum(1, TP)
    return finalize(out)


def summary(r):
    return {k: float(np.mean(r[k])) for k in FIELDS}


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
def make_frames(seed, n_obj=R.N_OBJ, n_frames=R.N_FRAMES):
    dets, gt = R.make_case(seed, n_obj, n_frames)
    _, recs = R.run_case(dets)
    first = {}
    frames = []
    for f, rec in enumerate(recs):
        ids = [first.setdefault(int(i), len(first)) for i in rec["ids"]]
        frames.append((gt[f].astype(np.float32), list(range(n_obj)), rec["boxes"].astype(np.float32), ids))
    return frames


def _decided(r):
    return [sorted((g, k) for g, k, _, sc in fr if sc > 0) for fr in r["matches"]]


def closest_to_a_threshold(r, alphas=ALPHAS):
    s = np.array([s for fr in r["matches"] for _, _, s, sc in fr if sc > 0])
    return float(np.abs(s[:, None] - np.asarray(alphas)[None, :]).min()) if s.size else float("inf")


def is_kept(frames, base=None):
    base = score_sequence(frames) if base is None else base
    if closest_to_a_threshold(base) < MARGIN:
        return False
    return all(_decided(score_sequence(frames, perturb_rng=np.random.default_rng(9000 + k))) == _decided(base) for k in range(3))


@functools.lru_cache(maxsize=None)
def case(seed, n_obj=R.N_OBJ, n_frames=R.N_FRAMES):
    """-> (frames, score_sequence's result, kept).  Cached and never modified: the CPU tests and the GPU tests share it."""
    frames = make_frames(seed, n_obj, n_frames)
    base = score_sequence(frames)
    return frames, base, is_kept(frames, base)


def kept_cases(cases=None):
    cases = CASES if cases is None else list(cases)
    out = [c for c in cases if case(*c)[2]]
    assert 8 * (len(cases) - len(out)) <= len(cases), "more than one case in eight dropped: %d of %d kept" % (len(out), len(cases))
    return out

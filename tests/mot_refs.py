"""Float64 reference of the batched CLEAR MOT family and the Identity family (row f-5; TrackEval's clear.py and identity.py as DESIGN.md section 3
freezes them) and the seeded cases the tests share.  A plain numpy statement that shares no code with the product; its similarity is
track_refs.iou_xyxy (through hota_refs.similarity: boxes rounded to float32 first), its assignment track_refs.assign_max.

* `score_sequence(frames)` -> the eleven counts, MOTP_sum, the per-frame match sets, pmc and the closest similarity to the threshold.
* `identity_reduced` / `identity_full` / `identity_brute` / `identity_greedy`: IDTP as the maximum-weight partial matching on pmc, through TrackEval's
  (G + T) x (G + T) fn_mat + fp_mat problem, by exhaustive search, and what largest-entry-first greedy reaches (a LOWER bound the tests show to be strict).
* `finalize` / `combine`: the host arithmetic.
* Sequence cases = hota_refs.CASES (the same frames).  A case is KEPT iff no similarity of any pair in any frame lies within 1e-7 of the threshold and
  the per-frame CLEAR match sets are the same under three reruns with every similarity perturbed by a relative U(-1e-9, 1e-9).  At most one case in
  eight may be dropped (`kept_cases` asserts it).
* Identity stress cases (`STRESS`, `group_frames`): tracked scenes give an almost diagonal pmc, so these deal random ids into groups of identical boxes:
  S is exactly 1 inside a group and 0 across, pmc is dense with small integers, and the ID counts and TP / FN / FP do not depend on how ties break
  (IDSW, MT / PT / ML and Frag do: not compared on these).
"""
import functools
import itertools

import numpy as np

import hota_refs as H
import track_refs as R

THR = 0.5
EPS = np.finfo(np.float64).eps
PERTURB = 1e-9
MARGIN = 1e-7
COUNTS = ("TP", "FN", "FP", "IDSW", "MT", "PT", "ML", "Frag", "IDTP", "IDFN", "IDFP")
RATIOS = ("MOTA", "MOTP", "MODA", "sMOTA", "CLR_Re", "CLR_Pr", "IDF1", "IDR", "IDP")
CASES = list(H.CASES)
STRESS = [(5, 6, 6), (40, 70, 20), (70, 40, 20), (64, 65, 30), (130, 150, 40), (150, 130, 40)]


# ---- identity -----------------------------------------------------------------------------------------------------------------------------
def identity_reduced(pmc):
    """max over partial one-to-one matchings of sum pmc: the entries are >= 0, so a complete assignment of the smaller side reaches it."""
    pmc = np.asarray(pmc, dtype=np.float64)
    return int(round(sum(pmc[r, c] for r, c in R.assign_max(pmc))))


def identity_full(pmc, gt_cnt, trk_cnt, solver=None):
    """TrackEval's identity.py: the (G + T) x (G + T) problem on fn_mat + fp_mat.  -> (IDTP, IDFN, IDFP)."""
    pmc = np.asarray(pmc, dtype=np.float64)
    G, T = pmc.shape
    fn = np.zeros((G + T, G + T))
    fp = np.zeros((G + T, G + T))
    fp[G:, :T] = 1e10
    fn[:G, T:] = 1e10
    for g in range(G):
        fn[g, :T] = gt_cnt[g]
        fn[g, T + g] = gt_cnt[g]
    for t in range(T):
        fp[:G, t] = trk_cnt[t]
        fp[G + t, t] = trk_cnt[t]
    fn[:G, :T] -= pmc
    fp[:G, :T] -= pmc
    pairs = (solver or (lambda c: R.assign_max(-c)))(fn + fp)
    idfn = int(round(sum(fn[r, c] for r, c in pairs)))
    idfp = int(round(sum(fp[r, c] for r, c in pairs)))
    return int(np.sum(gt_cnt)) - idfn, idfn, idfp


def identity_brute(pmc):
    """Exhaustive search over ALL partial matchings (each row takes a free column or none)."""
    pmc = np.asarray(pmc)
    G, T = pmc.shape
    best = 0
    for cols in itertools.product(range(-1, T), repeat=G):
        used = [c for c in cols if c >= 0]
        if len(set(used)) == len(used):
            best = max(best, int(sum(pmc[r, c] for r, c in enumerate(cols) if c >= 0)))
    return best


def identity_greedy(pmc):
    """Largest entry first (ties: lowest row, then lowest column), rows and columns removed as they are taken."""
    m = np.array(pmc, dtype=np.int64)
    total = 0
    while m.size and m.max() > 0:
        r, c = np.unravel_index(int(np.argmax(m)), m.shape)
        total += int(m[r, c])
        m[r, :] = 0
        m[:, c] = 0
    return total


# ---- the reference --------------------------------------------------------------------------------------------------------------------------
def score_sequence(frames, thr=THR, perturb_rng=None):
    """-> {the eleven COUNTS: int; "MOTP_sum": float; "matches": per frame the sorted [(gt id, track id)]; "pmc" int64 [NG][NT]; "gt_cnt", "trk_cnt",
    "present", "matched", "starts"; "n_gt_ids", "n_trk_ids"; "closest": the smallest |S - thr| of any pair of any frame}.  Ids are renumbered in order
    of first appearance."""
    gmap, tmap, fr = {}, {}, []
    for gb, gi, tb, ti in frames:
        g = [gmap.setdefault(int(i), len(gmap)) for i in gi]
        t = [tmap.setdefault(int(i), len(tmap)) for i in ti]
        assert len(set(g)) == len(g) and len(set(t)) == len(t), "an id twice in one frame"
        S = H.similarity(gb, tb)
        if perturb_rng is not None:
            S = S * (1.0 + perturb_rng.uniform(-PERTURB, PERTURB, S.shape))
        fr.append((g, t, S))
    NG, NT = len(gmap), len(tmap)
    pmc = np.zeros((NG, NT), dtype=np.int64)
    gt_cnt, trk_cnt = np.zeros(NG, dtype=np.int64), np.zeros(NT, dtype=np.int64)
    present, matched, starts = (np.zeros(NG, dtype=np.int64) for _ in range(3))
    tp = fn = fp = idsw = 0
    motp = 0.0
    closest = float("inf")
    prev, prev_step, matches = {}, {}, []
    for g, t, S in fr:
        for i in g:
            gt_cnt[i] += 1
            present[i] += 1
        for k in t:
            trk_cnt[k] += 1
        if not g or not t:
            fn += len(g)
            fp += len(t)
            prev_step = {}
            matches.append([])
            continue
        closest = min(closest, float(np.abs(S - thr).min()))
        pmc[np.array(g)[:, None], np.array(t)[None, :]] += S >= thr
        score = np.array([[1000.0 * (prev_step.get(i) == k) for k in t] for i in g]) + S
        score[S < thr - EPS] = 0
        step = {}
        for r, c in R.assign_max(score):
            if score[r, c] > 0:
                i, k = g[r], t[c]
                idsw += i in prev and prev[i] != k
                starts[i] += i not in prev_step
                matched[i] += 1
                step[i] = k
                motp += float(S[r, c])
        prev.update(step)
        prev_step = step
        matches.append(sorted(step.items()))
        tp += len(step)
        fn += len(g) - len(step)
        fp += len(t) - len(step)
    seen = present > 0
    mt = int(np.sum(seen & (5 * matched > 4 * present)))
    pt = int(np.sum(seen & (5 * matched >= present))) - mt
    idtp = identity_reduced(pmc) if NG and NT else 0
    return {"TP": tp, "FN": fn, "FP": fp, "IDSW": int(idsw), "MT": mt, "PT": pt, "ML": int(seen.sum()) - mt - pt, "Frag": int(np.maximum(0, starts - 1).sum()),
            "IDTP": idtp, "IDFN": int(gt_cnt.sum()) - idtp, "IDFP": int(trk_cnt.sum()) - idtp, "MOTP_sum": motp, "matches": matches, "pmc": pmc,
            "gt_cnt": gt_cnt, "trk_cnt": trk_cnt, "present": present, "matched": matched, "starts": starts, "n_gt_ids": NG, "n_trk_ids": NT,
            "closest": closest}


def finalize(c):
    """The host arithmetic on the counts of a sequence or of a combination."""
    gt = max(1, c["TP"] + c["FN"])
    out = {k: c[k] for k in COUNTS + ("MOTP_sum",)}
    out["MOTA"] = (c["TP"] - c["FP"] - c["IDSW"]) / gt
    out["MOTP"] = c["MOTP_sum"] / max(1, c["TP"])
    out["MODA"] = (c["TP"] - c["FP"]) / gt
    out["sMOTA"] = (c["MOTP_sum"] - c["FP"] - c["IDSW"]) / gt
    out["CLR_Re"] = c["TP"] / gt
    out["CLR_Pr"] = c["TP"] / max(1, c["TP"] + c["FP"])
    out["IDR"] = c["IDTP"] / max(1, c["IDTP"] + c["IDFN"])
    out["IDP"] = c["IDTP"] / max(1, c["IDTP"] + c["IDFP"])
    out["IDF1"] = c["IDTP"] / max(1, c["IDTP"] + 0.5 * c["IDFP"] + 0.5 * c["IDFN"])
    return out


def combine(seqs):
    """Every count and MOTP_sum add; the ratios are recomputed."""
    return finalize({k: sum(s[k] for s in seqs) for k in COUNTS + ("MOTP_sum",)})


def motp_bound(ref):
    """|MOTP_sum - reference| allowed: two fp64 sums of at most TP non-negative terms in different orders, plus one ulp on each term."""
    return (ref["TP"] + 2) * 2.0 ** -52 * ref["MOTP_sum"]


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
def is_kept(frames, base=None, thr=THR):
    base = score_sequence(frames, thr) if base is None else base
    if base["closest"] < MARGIN:
        return False
    return all(score_sequence(frames, thr, perturb_rng=np.random.default_rng(9100 + k))["matches"] == base["matches"] for k in range(3))


@functools.lru_cache(maxsize=None)
def case(seed, n_obj=R.N_OBJ, n_frames=R.N_FRAMES):
    """-> (frames, score_sequence's result, kept) on hota_refs' frames.  Cached and never modified: the CPU tests and the GPU tests share it."""
    frames = H.case(seed, n_obj, n_frames)[0]
    base = score_sequence(frames)
    return frames, base, is_kept(frames, base)


def kept_cases(cases=None):
    cases = CASES if cases is None else list(cases)
    out = [c for c in cases if case(*c)[2]]
    assert 8 * (len(cases) - len(out)) <= len(cases), "more than one case in eight dropped: %d of %d kept" % (len(out), len(cases))
    return out


def group_frames(seed, n_gt, n_trk, n_frames):
    """Each frame takes up to 48 random ids per side and deals them into groups of 0-4 ground truths and 0-4 tracks; all boxes of a group are the same
    4 x 2 box, groups sit on cells 10 apart."""
    rng = np.random.default_rng(5000 + seed)
    frames = []
    for _ in range(n_frames):
        gs = rng.permutation(n_gt)[:int(rng.integers(1, min(48, n_gt) + 1))].tolist()
        ts = rng.permutation(n_trk)[:int(rng.integers(1, min(48, n_trk) + 1))].tolist()
        gb, gi, tb, ti = [], [], [], []
        cell = 0
        while gs or ts:
            a, b = int(rng.integers(0, 5)), int(rng.integers(0, 5))
            box = [10.0 * (cell % 12), 10.0 * (cell // 12), 10.0 * (cell % 12) + 4.0, 10.0 * (cell // 12) + 2.0]
            cell += 1
            for _ in range(min(a, len(gs))):
                gi.append(gs.pop())
                gb.append(box)
            for _ in range(min(b, len(ts))):
                ti.append(ts.pop())
                tb.append(box)
        frames.append((np.array(gb, np.float32).reshape(-1, 4), gi, np.array(tb, np.float32).reshape(-1, 4), ti))
    return frames


@functools.lru_cache(maxsize=None)
def stress_case(k):
    """-> (frames, score_sequence's result) of STRESS[k].  Cached and never modified."""
    n_gt, n_trk, n_frames = STRESS[k]
    frames = group_frames(k, n_gt, n_trk, n_frames)
    return frames, score_sequence(frames)

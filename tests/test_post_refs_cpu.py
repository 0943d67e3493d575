"""The float64 references of tests/post_refs.py, checked without a GPU against the scalar oracle (oracle/postprocess_ref.py), and every
CONDITION the GPU sweep (tests/test_gpu_post_sweep.py) relies on, asserted on the case tables alone: the sweep demands exact kept sets, exact
orders and exact true-positive flags and forgives nothing, so a case whose answer rests on a rounding must fail HERE, before it reaches a GPU."""
import math

import numpy as np
import pytest

import post_refs as P
from oracle import postprocess_ref as PR

_NMS_IDS = [c.name for c in P.NMS_CASES]


# ------------------------------------------------------------------------------------------------------------------ conditions, as functions
def iou_margin_violations(consulted_iou, nms_thr, margin=P.IOU_MARGIN):
    """Pair IoU margin: boxes have sides >= 1 m and |x|, |y| <= 64 m, so a few fp32 roundings of a coordinate are <= 2e-5 m and move an IoU by at
    most perimeter / area x 2 x 2e-5 ~ 1.6e-4; every consulted pair keeps 1e-3 from the threshold."""
    return int((np.abs(np.asarray(consulted_iou) - nms_thr) <= margin).sum())


def score_separation_violations(scores, margins):
    """Score separation: two candidates of a map either have bit-identical logits (a built tie) or float64 scores >= 1e-5 apart (the fp32
    softmax is good to ~1e-7, the project's score bar is 1e-6)."""
    order = np.argsort(scores, kind="stable")
    s, m = np.asarray(scores)[order], np.asarray(margins)[order]
    gap = np.diff(s)
    same = m[1:].view(np.uint32) == m[:-1].view(np.uint32)
    return int(((gap < 1e-5) & ~same).sum())


def match_margin_violations(best, second, thr, exact_ok):
    """Match margin: best and runner-up IoU are bit-equal (a built tie) or >= 1e-6 apart; the best IoU is exactly at thr (allowed only where the
    case is built so) or >= 1e-6 from it."""
    best, second = np.asarray(best), np.asarray(second)
    bad = ((best - second < P.MATCH_MARGIN) & (best != second)).sum()
    at = best == thr
    bad += ((np.abs(best - thr) < P.MATCH_MARGIN) & ~at).sum() + (0 if exact_ok else at.sum())
    return int(bad)


def cand_margin_violations(scores, thr):
    """Candidate margin: every score is exactly at the threshold (equal logits: 0.5; saturated: 1.0 and 0.0) or >= 1e-5 from it.  A threshold of
    0 is met by every score whatever its rounding (scores are never negative), so nothing can rest on one there."""
    t = P.thr32(thr)
    if t == 0.0:
        return 0
    s = np.asarray(scores)
    return int(((np.abs(s - t) < P.CAND_MARGIN) & (s != t)).sum())


# ------------------------------------------------------------------------------------------------------------------ references vs the oracle
def test_array_helpers_are_the_oracles_scalars():
    rng = np.random.default_rng(0)
    codes, anchors = P.make_decode_case()
    got = P.decode64(codes, anchors)
    for i in range(len(codes)):
        assert tuple(got[i]) == PR.decode_faf(codes[i], anchors[i]), i
    boxes = P.rand_boxes(rng, 20)
    cor = P.corners64(boxes)
    for i in range(20):
        want = PR.corners_of(tuple(float(v) for v in boxes[i]))
        assert np.abs(cor[i] - np.asarray(want)).max() < 1e-15
        assert np.allclose(P.standup64(cor[i]), PR.standup_of(want), atol=1e-15)
    c = rng.normal(0, 3, (50, 2)).astype(np.float32)
    s = P.score64(c[:, 0], c[:, 1])
    for i in range(50):
        assert abs(s[i] - PR.fg_score(float(c[i, 0]), float(c[i, 1]))) < 1e-16


@pytest.mark.parametrize("index", range(len(P.NMS_CASES)), ids=_NMS_IDS)
def test_nms_ref64_equals_oracle_detect(index):
    """Every map with <= 300 candidates: the same kept anchors in the same order as postprocess_ref.detect on the logits the sweep launches."""
    d = P.make_nms_case(index)
    case = d["case"]
    arr = P.launch_arrays(d["maps"], d["anchors"], d["codes"], case.cap)
    n_checked = 0
    for i, (m, r) in enumerate(zip(d["maps"], d["refs"])):
        if len(m["aid"]) > 300 or r["count"] < 0:
            continue
        det = PR.detect(arr["cls"][i].tolist(), arr["loc"][i].tolist(), d["anchors"].tolist(), P.SCORE_THR, case.nms_thr, rotated=case.rotated)
        assert [k["index"] for k in det] == r["index"].tolist(), (case.name, i)
        assert np.allclose([k["score"] for k in det], r["scores"], atol=0, rtol=1e-15)
        assert np.allclose(np.asarray([k["box"] for k in det]).reshape(-1, 5), r["boxes"], atol=1e-12)
        n_checked += 1
    assert n_checked or min(case.counts) > 300


def test_match_ref64_equals_oracle_eval_map_flags():
    """match_ref64's flags against postprocess_ref.eval_map on the small cases.  eval_map returns the AP, not the flags, but on ONE image the AP
    of the first j + 1 detections exceeds the AP of the first j exactly when detection j is a true positive (a true positive adds a recall
    step of positive precision, a false positive adds none and leaves the earlier steps' precision alone), and a greedy matching of a prefix
    is the prefix of the matching."""
    n_img = n_tp = 0
    for index, (name, gt_cap, det_cap, thr, images) in enumerate(P.MATCH_CASES):
        if gt_cap > 8:
            continue
        det, dc, gt, gc, thr, refs = P.make_match_case(index)
        for i in range(det.shape[0]):
            tp = refs[i][0]
            ng = min(max(int(gc[i]), 0), gt_cap)
            gts = [PR.corners_of(tuple(float(v) for v in g)) for g in gt[i, :ng]]
            dets = [(1.0 - 1e-3 * j, PR.corners_of(tuple(float(v) for v in det[i, j]))) for j in range(len(tp))]
            ap = [0.0] + [PR.eval_map([dets[:j + 1]], [gts], thr)[0] for j in range(len(tp))]
            assert [int(ap[j + 1] > ap[j] + 1e-12) for j in range(len(tp))] == tp.tolist(), (name, i)
            n_img += 1
            n_tp += int(tp.sum())
    assert n_img >= 10 and n_tp >= 10


def test_iou_reference_against_closed_forms_and_raster():
    """The explicit pairs: the oracle's vertex-collection IoU meets the hand-computed answers (5e-7: the fp32 rounding of pi turns a box by
    1e-7 rad), nothing is NaN; the non-degenerate ones and a sample of the size case agree with the raster referee to its resolution."""
    a, b = P.iou_pair_arrays()
    ref = P.iou_ref64(a, b)
    assert np.isfinite(ref).all()
    for i, (name, _, _, closed, degenerate) in enumerate(P.IOU_PAIRS):
        if closed is not None:
            assert abs(ref[i, i] - closed) < 5e-7, (name, ref[i, i], closed)
        assert abs(ref[i, i] - P.iou_ref64(b[i:i + 1], a[i:i + 1])[0, 0]) < 1e-9, name
        if not degenerate and not name.startswith("far"):
            r = PR.raster_iou(tuple(float(v) for v in a[i]), tuple(float(v) for v in b[i]))
            assert abs(ref[i, i] - r) < 0.02, (name, ref[i, i], r)
    # 1e4 m: the same pair as "generic", moved (the fp32 sums are exact)
    i, j = [p[0] for p in P.IOU_PAIRS].index("far-1e4"), [p[0] for p in P.IOU_PAIRS].index("generic")
    assert abs(ref[i, i] - ref[j, j]) < 1e-9 and ref[j, j] > 0.1
    ta, tb, tref = P.make_iou_size_case()[3]
    rng = np.random.default_rng(5)
    for _ in range(40):
        i, j = int(rng.integers(0, len(ta))), int(rng.integers(0, len(tb)))
        r = PR.raster_iou(tuple(float(v) for v in ta[i]), tuple(float(v) for v in tb[j]))
        assert abs(tref[i, j] - r) < 0.02, (i, j, tref[i, j], r)
    assert (tref > 0).mean() > 0.3
    A, B, full, _ = P.make_iou_size_case()
    assert A.shape == (P.IOU_NA, 5) and B.shape == (P.IOU_NB, 5) and full.shape == (P.IOU_NA, P.IOU_NB)
    assert full.size > P.IOU_GRID_PASS and (full.reshape(-1)[P.IOU_GRID_PASS:] > 0).any()          # the grid-stride tail holds non-trivial answers


# ------------------------------------------------------------------------------------------------------------------ no case rests on a rounding
@pytest.mark.parametrize("index", range(len(P.NMS_CASES)), ids=_NMS_IDS)
def test_nms_cases_keep_their_margins(index):
    d = P.make_nms_case(index)
    case = d["case"]
    assert case.cap in (64, 256, 1024, 4096) and d["anchors"].shape == (case.cap + P.EXTRA_ANCHORS, 6)
    assert d["anchors"].dtype == np.float32 and d["codes"].dtype == np.float32
    boxes = P.decode64(d["codes"], d["anchors"])
    assert boxes[:, 2:4].min() >= 1.0
    if case.geom == "lattice":
        assert np.abs(boxes[:, :2]).max() <= 64.0
    else:
        assert (boxes[:, 4] == 0).all() and (boxes[:, 2:4] == 1).all()
    for m, r in zip(d["maps"], d["refs"]):
        c = len(m["aid"])
        assert len(set(m["aid"].tolist())) == c and sorted(m["slot"].tolist()) == list(range(c))
        if c > case.cap:
            assert r["count"] == -c
            continue
        assert score_separation_violations(r["all_scores"], m["margin"]) == 0
        assert c == 0 or r["all_scores"].min() > P.SCORE_THR + 1e-3
        if case.geom == "chains":          # exact: every consulted IoU is 0, 1/3 or 1 up to the last bit of float64
            iou = r["consulted"].iou
            assert ((iou == 0) | (np.abs(iou - 1.0 / 3.0) < 1e-15) | (iou == 1)).all()
        assert iou_margin_violations(r["consulted"].iou, case.nms_thr) == 0, case.name
        assert 0 < r["count"] or c == 0
        if c > 2:
            assert r["count"] < c, "nothing suppressed: the map tests no suppression"


def test_margin_checks_reject_a_violating_case():
    """The four conditions refuse what they must: a pair 5e-4 from the threshold, two levels 5e-6 apart, a runner-up 5e-7 below the best, a
    score 5e-6 above the threshold."""
    assert iou_margin_violations([0.0, 0.3005, 0.9], 0.3) == 1 and iou_margin_violations([0.0, 0.302, 0.9], 0.3) == 0
    m = np.array([1.0, 1.00003, 2.0], np.float32)
    assert score_separation_violations(P.score64(np.zeros(3), m), m) == 1
    m = np.array([1.0, 1.0, 2.0], np.float32)
    assert score_separation_violations(P.score64(np.zeros(3), m), m) == 0
    assert match_margin_violations([0.8], [0.8 - 5e-7], 0.5, False) == 1 and match_margin_violations([0.8], [0.8], 0.5, False) == 0
    assert match_margin_violations([0.5 + 5e-7], [0.1], 0.5, False) == 1 and match_margin_violations([0.5], [0.1], 0.5, False) == 1
    assert match_margin_violations([0.5], [0.1], 0.5, True) == 0
    assert cand_margin_violations([0.7 + 5e-6], 0.7) == 1 and cand_margin_violations([P.thr32(0.7), 0.72], 0.7) == 0


def test_match_cases_keep_their_margins_and_hold_every_required_item():
    ngs, dups, mirrors, raw_d, raw_g = set(), set(), set(), set(), set()
    for index, (name, gt_cap, det_cap, thr, images) in enumerate(P.MATCH_CASES):
        det, dc, gt, gc, thr, refs = P.make_match_case(index)
        assert det.shape == (len(images), det_cap, 5) and gt.shape == (len(images), gt_cap, 5) and gt_cap <= 8192
        assert float(np.float32(thr)) == thr                                     # the kernel gets the very threshold
        for i, spec in enumerate(images):
            tp, best, second = refs[i]
            assert match_margin_violations(best, second, thr, exact_ok="hand" in spec) == 0, (name, i)
            ng = min(max(int(gc[i]), 0), gt_cap)
            ngs.add(ng)
            raw_d.add(int(dc[i]) - det_cap if dc[i] > det_cap else int(dc[i]) if dc[i] < 0 else 0)
            raw_g.add(int(gc[i]) - gt_cap if gc[i] > gt_cap else int(gc[i]) if gc[i] < 0 else 0)
            if "hand" in spec:
                assert best[0] == thr and tp[0] == 1 and (tp.tolist() == [1, 0, 0] if spec["hand"] == "identical" else tp.tolist() == [1, 0, 1])
            if spec.get("dup"):
                p, q = spec["dup"]
                dups.add((p, q))
                assert p < q < ng and np.array_equal(gt[i, p], gt[i, q])
                on = [j for j in range(len(tp)) if np.array_equal(det[i, j], gt[i, p])]
                assert len(on) == 2 and best[on[0]] == second[on[0]] and abs(best[on[0]] - 1.0) < 1e-9
                assert tp[on[0]] == 1 and tp[on[1]] == 0, "the first takes the lower index, the second has no second choice"
            if spec.get("mirror"):
                p, q = spec["mirror"]
                mirrors.add((p, q))
                on_q = [j for j in range(len(tp)) if np.array_equal(det[i, j], gt[i, q])][0]
                on_p = [j for j in range(len(tp)) if np.array_equal(det[i, j], gt[i, p])][0]
                mid = [j for j in range(len(tp)) if tuple(det[i, j, :2]) == P.MIRROR_AT][0]
                assert p < q < ng and mid < on_q < on_p and best[mid] == second[mid] == 0.6 and thr <= 0.5
                assert (tp[mid], tp[on_q], tp[on_p]) == (1, 1, 0), "the tie goes to the lower index: q stays free, p is taken"
            if spec.get("next_bait"):
                assert gc[i] == gt_cap + 1 and np.array_equal(gt[i + 1, 0], det[i, spec["nd"] - 1]) and tp[spec["nd"] - 1] == 0
                assert best[spec["nd"] - 1] == 0.0
            if len(tp) >= 8:
                assert 0 < tp.sum() < len(tp)
    assert {0, 1, 2, 255, 256, 257, 513, 8192} <= ngs
    assert {(5, 300), (7, 263), (255, 256)} <= dups              # different threads; one thread (7 = 263 - 256); neighbours across the stride
    # mirrored pairs: in different threads whose partial results meet late in the tree (5 | 300, 77 | 8000), thread 255 against thread 0, one thread
    assert {(5, 300), (255, 256), (7, 263), (77, 8000)} <= mirrors
    assert {-3, 9} <= raw_d and {-1, 1} <= raw_g


@pytest.mark.parametrize("thr,M", P.CAND_CASES)
def test_cand_cases_keep_their_margin(thr, M):
    cls, passing, count = P.make_cand_case(thr, M)
    assert cls.shape == (M, 2) and cls.dtype == np.float32
    s = P.score64(cls[:, 0], cls[:, 1])
    assert cand_margin_violations(s, thr) == 0
    assert M - 1 in passing
    if thr == 0.0:
        assert len(passing) == M and count == (M if M <= P.CAND_CAP else -M)
    else:
        assert 0 < len(passing) <= P.CAND_CAP and count == len(passing)
    if M >= 255:
        t = P.thr32(thr)
        kinds = {why for _, _, why in P._cand_special_rows(thr)}
        assert {"equal", "saturated"} <= kinds and (("margin-edge" in kinds) == (thr == 0.7))
        assert (s == 0.5).sum() >= 3 and (s == 1.0).sum() >= 2 and (s == 0.0).sum() >= 1
        if thr == 0.7:
            edge = np.abs(s - t)
            assert ((edge >= P.CAND_MARGIN) & (edge < 1.1 * P.CAND_MARGIN) & (s > t)).any() and ((edge >= P.CAND_MARGIN) & (edge < 1.1 * P.CAND_MARGIN) & (s < t)).any()
        if 0 < thr < 1:
            assert len(passing) < M


def test_decode_case_holds_every_edge():
    codes, anchors = P.make_decode_case()
    assert {-5.0, -4.0, -4.0 + 2.0 ** -20, 0.0, 4.0, float(np.float32(4.001)), 50.0} <= set(codes[:, 2].astype(np.float64).tolist())
    assert set(codes[:49, 2].tolist()) == set(codes[:49, 3].tolist())
    assert np.float32(-4.0 + 2.0 ** -20) != np.float32(-4.0)
    pairs = {(float(a), float(b)) for a, b in codes[:, 4:6]}
    assert {(0.0, 0.0), (0.0, -1.0), (float(np.float32(1e-30)), 1.0), (-1.0, 0.0)} <= pairs and np.float32(1e-30) > 0
    box = P.decode64(codes, anchors)
    assert (box[:, 4] > math.pi).any() and (box[:, 4] < -math.pi).any()
    assert (np.abs(box[:, 0]) == 1e4).sum() >= 3 and (np.abs(box[:, 1]) == 1e4).sum() >= 2
    # the sums at 1e4 m are exact in fp32, so the 1e-4 m bar asks nothing of fp32's spacing there
    x32 = anchors[:, 0] + codes[:, 0]
    assert np.array_equal(x32.astype(np.float64), box[:, 0]) or np.abs(x32.astype(np.float64) - box[:, 0])[np.abs(box[:, 0]) > 100].max() == 0
    assert box[:, 2].max() == 2.0 * math.exp(4.0) and box[:, 2].min() == 2.0 * math.exp(-4.0)


# ------------------------------------------------------------------------------------------------------------------ coverage
def _sorted_view(d, i):
    """Map i of an NMS case in sorted order: stand-up IoU matrix, kept flags."""
    case, m, r = d["case"], d["maps"][i], d["refs"][i]
    aid = m["aid"]
    order = np.lexsort((aid, -r["all_scores"]))
    su = P.standup64(P.corners64(P.decode64(d["codes"][aid], d["anchors"][aid])))[order]
    iw = np.clip(np.minimum(su[:, None, 2], su[None, :, 2]) - np.maximum(su[:, None, 0], su[None, :, 0]), 0, None)
    ih = np.clip(np.minimum(su[:, None, 3], su[None, :, 3]) - np.maximum(su[:, None, 1], su[None, :, 1]), 0, None)
    area = (su[:, 2] - su[:, 0]) * (su[:, 3] - su[:, 1])
    iou = iw * ih / (area[:, None] + area[None, :] - iw * ih)
    kept = np.isin(aid[order], r["index"])
    return iou > case.nms_thr, kept, m["slot"][order], m["margin"][order]


def test_nms_case_table_reaches_every_form_and_edge():
    """An edit of the table must not silently stop reaching a branch of det_nms_kernel: counts on both sides of 64 (the bit-matrix word), of 512
    (FAST / serial) and of every cap; the mixed batch in the stated order and in a permuted one; every geometry, score kind and mode; in a
    512-candidate chains map every 64-bit word holds a candidate that a KEPT one suppresses; a chain A suppresses B, B would have suppressed
    C, C kept, that crosses a word; a tie group whose keys sit in two 256-key blocks of the sort."""
    counts = {c for case in P.NMS_CASES for c in case.counts}
    assert {0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025} <= counts
    assert {case.cap for case in P.NMS_CASES} == {64, 256, 1024, 4096}
    for cap in (64, 256, 1024, 4096):
        assert {cap - 1, cap, cap + 1} <= {c for case in P.NMS_CASES if case.cap == cap for c in case.counts}, cap
    mixed = [case for case in P.NMS_CASES if sorted(case.counts) == sorted(P.MIXED_COUNTS(case.cap))]
    assert any(case.counts == P.MIXED_COUNTS(case.cap) for case in mixed) and any(case.counts != P.MIXED_COUNTS(case.cap) for case in mixed)
    assert {(c.geom, c.order) for c in P.NMS_CASES} >= {("chains", "desc"), ("chains", "asc"), ("chains", "perm"), ("lattice", None)}
    assert {c.scores for c in P.NMS_CASES} == {"distinct", "equal", "ties"}
    assert {(c.geom, c.rotated) for c in P.NMS_CASES} == {("chains", False), ("chains", True), ("lattice", False), ("lattice", True)}
    assert {c.nms_thr for c in P.NMS_CASES if c.geom == "lattice" and not c.rotated} == {0.01, 0.3}
    assert all(c.nms_thr == 0.2 for c in P.NMS_CASES if c.geom == "chains")
    assert any(c.rotated and max(x for x in c.counts if x <= c.cap) > P.NMS_FAST_CAP for c in P.NMS_CASES)      # the serial form, rotated
    words_ok = chain_ok = tie_ok = False
    for index, case in enumerate(P.NMS_CASES):
        d = P.make_nms_case(index)
        for i, c in enumerate(case.counts):
            if c > case.cap:
                continue
            if case.scores == "ties" and c > P.BLOCK:
                m = d["maps"][i]
                for bits in np.unique(m["margin"].view(np.uint32)):
                    members = np.nonzero(m["margin"].view(np.uint32) == bits)[0]
                    blocks = set((m["slot"][members] // P.BLOCK).tolist())
                    order_by_anchor = m["slot"][members]                         # members ascend in anchor index
                    if len(blocks) >= 2 and len(members) >= 2 and (np.diff(order_by_anchor) < 0).any():
                        tie_ok = True
            if case.geom != "chains" or c != 512:
                continue
            sup, kept, _, _ = _sorted_view(d, i)
            by_kept = np.triu(sup & kept[:, None], 1)                            # row i kept, column j > i suppressed by it
            hit_words = {int(j) // P.WORD for j in np.nonzero(by_kept.any(0))[0]}
            words_ok |= hit_words == set(range(512 // P.WORD))
            for a in np.nonzero(kept)[0]:
                for b in np.nonzero(by_kept[a])[0]:
                    for cc in np.nonzero(np.triu(sup, 1)[b] & kept)[0]:         # b (dropped) overlaps the later, KEPT cc
                        if len({int(a) // P.WORD, int(b) // P.WORD, int(cc) // P.WORD}) >= 2:
                            chain_ok = True
    assert words_ok and chain_ok and tie_ok, (words_ok, chain_ok, tie_ok)

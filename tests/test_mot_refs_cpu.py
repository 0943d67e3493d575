"""CPU tests of the CLEAR / Identity reference (tests/mot_refs.py) the GPU tests compare with: agreement with track_refs.ClearMotRef, hand-counted
MT / PT / ML / Frag, the Identity optimum three ways (reduced, TrackEval's (G + T) x (G + T) problem, brute force; scipy where present), the kept-case
cap, optimum against greedy on the stress cases, the combination rule, `hota_extras`, and the two C ABI entries as far as they go without a GPU."""
import ctypes

import numpy as np
import pytest

import hota_refs as H
import mot_refs as M
import track_refs as R

NONE = np.zeros((0, 4), dtype=np.float32)


def _box(cx, cy, w=4.0, h=2.0):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]


def _one_object(matched_frames, n_frames=10, extra_gt=()):
    """One ground-truth object (id 7) over n_frames; its track (id 3) sits on it in matched_frames and 50 m away otherwise."""
    frames = []
    for f in range(n_frames):
        gb = np.array([_box(0, 0)] + [_box(100, 100)] * len(extra_gt), np.float32)
        tb = np.array([_box(0, 0) if f in matched_frames else _box(50, 50)], np.float32)
        frames.append((gb, [7] + list(extra_gt), tb, [3]))
    return frames


def test_clear_counts_equal_clearmotref_on_every_case():
    for c in M.CASES:
        frames, ref, _ = M.case(*c)
        cm = R.ClearMotRef()
        for gb, gi, tb, ti in frames:
            cm.update(gb, gi, tb, ti)
        assert (ref["TP"], ref["FN"], ref["FP"], ref["IDSW"]) == (cm.tp, cm.fn, cm.fp, cm.idsw), c
        assert abs(ref["MOTP_sum"] - cm.iou_sum) <= 1e-12 * max(1.0, cm.iou_sum), c
        assert ref["TP"] + ref["FN"] == ref["IDTP"] + ref["IDFN"] and ref["TP"] + ref["FP"] == ref["IDTP"] + ref["IDFP"]
        assert ref["MT"] + ref["PT"] + ref["ML"] == ref["n_gt_ids"]


def test_mt_pt_ml_frag_hand_counted():
    r = M.score_sequence(_one_object({0, 1, 2, 5, 6, 7, 8, 9}))                         # 8 of 10: ratio 0.8 is PT, not MT; two runs: Frag 1
    assert (r["MT"], r["PT"], r["ML"], r["Frag"], r["TP"], r["FN"], r["FP"], r["IDSW"]) == (0, 1, 0, 1, 8, 2, 2, 0)
    assert r["matched"].tolist() == [8] and r["present"].tolist() == [10] and r["starts"].tolist() == [2]
    r = M.score_sequence(_one_object(set(range(9))))                                    # 9 of 10: MT
    assert (r["MT"], r["PT"], r["ML"], r["Frag"]) == (1, 0, 0, 0)
    r = M.score_sequence(_one_object({4}))                                              # 1 of 10: below 0.2, ML
    assert (r["MT"], r["PT"], r["ML"], r["Frag"]) == (0, 0, 1, 0)
    r = M.score_sequence(_one_object({3, 4}))                                           # 2 of 10: 0.2 is PT
    assert (r["MT"], r["PT"], r["ML"]) == (0, 1, 0)
    r = M.score_sequence(_one_object(set(range(9)), extra_gt=(9,)))                     # a second, never matched object: ML
    assert (r["MT"], r["PT"], r["ML"]) == (1, 0, 1)
    assert M.score_sequence([]) ["ML"] == 0                                             # an id absent from the sequence counts nowhere


def test_empty_frames_clear_the_continuity_term():
    """Two tracks on one object; track 1 matched in frame 0.  With an empty frame between, frame 2 is decided on similarity alone (track 2 is closer);
    without it, continuity keeps track 1."""
    gb = np.array([_box(0, 0)], np.float32)
    first = (gb, [0], np.array([_box(0, 0)], np.float32), [1])
    both = (gb, [0], np.array([_box(0.5, 0), _box(0.1, 0)], np.float32), [1, 2])
    kept = M.score_sequence([first, both])
    assert kept["matches"] == [[(0, 0)], [(0, 0)]] and kept["IDSW"] == 0 and kept["Frag"] == 0
    for gap, k in (((gb, [0], NONE, []), 1), ((NONE, [], NONE, []), 1), ((NONE, [], gb, [9]), 2)):     # k: track 2's number by first appearance
        cut = M.score_sequence([first, gap, both])
        assert cut["matches"][2] == [(0, k)] and cut["IDSW"] == 1 and cut["Frag"] == 1, gap


def test_swap_case_by_hand():
    """Two objects over 10 frames whose two tracks exchange them after frame 5."""
    a, b = _box(0, 0), _box(20, 0)
    frames = [(np.array([a, b], np.float32), [0, 1], np.array([a, b] if f < 5 else [b, a], np.float32), [10, 11]) for f in range(10)]
    r = M.finalize(M.score_sequence(frames))
    assert (r["IDTP"], r["IDFN"], r["IDFP"]) == (10, 10, 10) and r["IDF1"] == 0.5 and r["IDR"] == 0.5 and r["IDP"] == 0.5
    assert (r["TP"], r["FN"], r["FP"], r["IDSW"]) == (20, 0, 0, 2) and r["MOTA"] == 0.9 and r["MOTP"] == 1.0 and r["Frag"] == 0 and r["MT"] == 2


def test_identity_three_formulations_agree():
    rng = np.random.default_rng(11)
    for _ in range(40):
        G, T = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        pmc = rng.integers(0, 5, (G, T)) * (rng.random((G, T)) < 0.7)
        gt_cnt = pmc.sum(1) + rng.integers(0, 3, G)
        trk_cnt = pmc.sum(0) + rng.integers(0, 3, T)
        best = M.identity_brute(pmc)
        assert M.identity_reduced(pmc) == best
        assert M.identity_full(pmc, gt_cnt, trk_cnt) == (best, int(gt_cnt.sum()) - best, int(trk_cnt.sum()) - best)
        assert M.identity_greedy(pmc) <= best
    for c in M.CASES[:2] + M.CASES[8:9]:
        ref = M.case(*c)[1]
        assert M.identity_full(ref["pmc"], ref["gt_cnt"], ref["trk_cnt"]) == (ref["IDTP"], ref["IDFN"], ref["IDFP"]), c


def test_identity_agrees_with_scipy():
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment

    def solver(cost):
        r, c = lsa(cost)
        return list(zip(r.tolist(), c.tolist()))

    for ref in [M.case(*c)[1] for c in M.CASES] + [M.stress_case(k)[1] for k in range(len(M.STRESS))]:
        r, c = lsa(-ref["pmc"])
        assert int(ref["pmc"][r, c].sum()) == ref["IDTP"]
        assert M.identity_full(ref["pmc"], ref["gt_cnt"], ref["trk_cnt"], solver) == (ref["IDTP"], ref["IDFN"], ref["IDFP"])


def test_at_most_one_case_in_eight_is_dropped():
    kept = M.kept_cases()
    assert len(kept) >= 14 and {c[1:] for c in kept} == {(12, 24), (40, 30), (60, 12)}
    closest = min(M.case(*c)[1]["closest"] for c in kept)
    print("kept %d of %d; closest similarity to the threshold %.3g" % (len(kept), len(M.CASES), closest))
    assert closest >= M.MARGIN
    refs = [M.case(*c)[1] for c in kept]
    assert sum(r["IDSW"] for r in refs) > 0 and sum(r["Frag"] for r in refs) > 0 and sum(r["MT"] for r in refs) > 0 and sum(r["ML"] + r["PT"] for r in refs) > 0
    assert any(r["n_trk_ids"] > 64 for r in refs)


def test_optimum_beats_greedy_on_the_stress_cases():
    wins = 0
    for k, (n_gt, n_trk, _) in enumerate(M.STRESS):
        frames, ref = M.stress_case(k)
        greedy = M.identity_greedy(ref["pmc"])
        print("stress %s: optimum %d, greedy %d, pmc max %d, ids %d x %d" % (M.STRESS[k], ref["IDTP"], greedy, ref["pmc"].max(), ref["n_gt_ids"], ref["n_trk_ids"]))
        assert greedy <= ref["IDTP"] and max(len(fr[1]) for fr in frames) <= 48 and max(len(fr[3]) for fr in frames) <= 48
        assert ref["closest"] == 0.5                                                     # S is exactly 0 or 1
        wins += greedy < ref["IDTP"]
    assert wins >= 4
    big = M.stress_case(4)[1]
    assert big["n_gt_ids"] > 128 and big["n_trk_ids"] > 128                              # beyond two waves
    assert M.stress_case(3)[1]["n_gt_ids"] == 64 and M.stress_case(3)[1]["n_trk_ids"] == 65   # the one-wave boundary


def test_combination_rule_against_a_hand_sum():
    one = M.score_sequence(_one_object({0, 1, 2, 5, 6, 7, 8, 9}))                       # TP 8, FN 2, FP 2, IDTP 8
    b = np.array([_box(0, 0)], np.float32)
    two = M.score_sequence([(b, [0], np.array([[-1.5, -1, 2.5, 1]], np.float32), [5 if f < 2 else 9]) for f in range(4)])   # IoU 3.5 / 4.5; IDSW 1
    assert (two["TP"], two["IDSW"], two["IDTP"], two["IDFN"], two["IDFP"]) == (4, 1, 2, 2, 2) and abs(two["MOTP_sum"] - 4 * 3.5 / 4.5) <= 4e-15
    r = M.combine([one, two])
    s = 8 + 4 * 3.5 / 4.5
    assert (r["TP"], r["FN"], r["FP"], r["IDSW"], r["IDTP"], r["IDFN"], r["IDFP"], r["Frag"], r["PT"], r["MT"]) == (12, 2, 2, 1, 10, 4, 4, 1, 1, 1)
    for k, want in (("MOTA", 9 / 14), ("MOTP", s / 12), ("MODA", 10 / 14), ("sMOTA", (s - 3) / 14), ("CLR_Re", 12 / 14), ("CLR_Pr", 12 / 14), ("IDR", 10 / 14),
                    ("IDP", 10 / 14), ("IDF1", 10 / 14)):
        assert abs(r[k] - want) <= 4e-15, (k, r[k], want)                               # a few ulps of MOTP_sum = 11.1
    empty = M.combine([])
    assert all(empty[k] == 0 for k in M.COUNTS + M.RATIOS)


def test_hota_extras_against_closed_forms():
    from v2x_sim_amd.utils.mot_metrics import hota_extras
    b = np.array([_box(0, 0)], np.float32)
    per = H.finalize(H.score_sequence([(b, [0], b, [5 if f < 2 else 9]) for f in range(4)]))      # DetRe 1, AssA 0.5, LocA 1 at every alpha
    x = hota_extras({"per_alpha": per})
    assert set(x) == {"OWTA", "HOTA(0)", "LocA(0)", "HOTALocA(0)"}
    assert abs(x["OWTA"] - np.sqrt(0.5)) <= 1e-15 and abs(x["HOTA(0)"] - np.sqrt(0.5)) <= 1e-15 and x["LocA(0)"] == 1.0 and abs(x["HOTALocA(0)"] - np.sqrt(0.5)) <= 1e-15
    per = H.finalize(H.case(0)[1])
    x = hota_extras({"per_alpha": per})
    assert abs(x["OWTA"] - float(np.mean(np.sqrt(per["DetRe"] * per["AssA"])))) <= 1e-15
    assert x["HOTA(0)"] == per["HOTA"][0] and x["LocA(0)"] == per["LocA"][0] and x["HOTALocA(0)"] == per["HOTA"][0] * per["LocA"][0]
    assert x["OWTA"] >= float(np.mean(per["HOTA"]))                                     # DetRe >= DetA


def test_c_abi_entries_validate_without_a_gpu():
    """v2x_mot_workspace_size / v2x_mot_sequences exist in the library and in the binding; sizes out of range or beyond the id cap give 0 / -22 with a
    message before any HIP call; the workspace size is the sum of its buffers and guards against overflow."""
    from v2x_sim_amd import _lib, ops_track
    lib = _lib.load()
    size = lib.v2x_mot_workspace_size
    cap_ids = ops_track.MOT_MAX_IDS
    assert cap_ids >= 1024
    S, F, cap, NG, NT = 50, 100, 40, 40, 120
    want = 0
    for elem, n in ((8, S * F * cap * cap), (8, S), (4, S * NG * NT), (4, S * F * cap), (4, S * F * cap), (4, S * F), (4, S * F)) + ((4, S * NG),) * 5 + ((4, S * 8),):
        want += (elem * n + 15) // 16 * 16
    assert size(S, F, cap, NG, NT) == want
    assert size(0, 1, 1, 0, 0) == 16 and size(1, 1, 1, 0, 0) > 0 and size(1, 1, 64, cap_ids, cap_ids) > 0
    for bad in ((-1, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 65, 1, 1), (1, 1, 1, -1, 1), (1, 1, 1, 1, -1), (1, 1, 1, cap_ids + 1, 1),
                (1, 1, 1, 1, cap_ids + 1)):
        assert size(*bad) == 0, bad
    big = 2 ** 31 - 1
    assert size(big, big, 64, cap_ids, cap_ids) == 0                                  # overflows 64 bits: refused, not wrapped
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(S=1, F=1, cap=1, NG=1, NT=1, thr=0.5, ws=1 << 20, ptr=p):
        return lib.v2x_mot_sequences(ptr, p, p, p, p, p, S, F, cap, NG, NT, thr, p, ws, p, p, None)

    for kw, text in ((dict(ptr=None), b"null pointer"), (dict(S=-1), b"n_seq"), (dict(F=0), b"n_frames"), (dict(cap=65), b"cap = 65"), (dict(cap=0), b"cap = 0"),
                     (dict(NG=-1), b"n_gt_ids"), (dict(NT=cap_ids + 1), b"id cap"), (dict(NG=cap_ids + 1), b"id cap"), (dict(thr=float("nan")), b"thr"),
                     (dict(thr=float("inf")), b"thr"), (dict(ws=8), b"workspace of 8 bytes"), (dict(S=1 << 20, F=1 << 10, ws=2 ** 62), b"2^24"),
                     (dict(S=big, F=big, cap=64, NG=cap_ids, NT=cap_ids), b"overflows")):
        assert call(**kw) == -22, kw
        assert text in lib.v2x_last_error(), (kw, lib.v2x_last_error())

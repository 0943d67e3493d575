"""CPU tests of the HOTA reference (tests/hota_refs.py) the GPU tests compare with: closed forms, agreement with scipy's assignment on the kept cases, the
kept-case cap, the combination rule against a hand sum; the parser of tools/track/eval_track.py; and the two C ABI entries as far as they go without
a GPU."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import hota_refs as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = len(H.ALPHAS)


def _box(cx, cy, w=4.0, h=2.0):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]


def _score(frames):
    return H.finalize(H.score_sequence(frames))


def test_the_thresholds_are_numpys_nineteen():
    assert A == 19 and H.ALPHAS[0] == 0.05 and H.ALPHAS[5] == 0.05 + 5 * 0.05 and H.ALPHAS[-1] < 0.951 and H.EPS == 2.0 ** -52


def test_tracks_equal_to_the_ground_truth_score_one():
    rng = np.random.default_rng(1)
    frames = []
    for f in range(5):
        b = np.array([_box(10 * k + f, rng.uniform(-5, 5)) for k in range(4)])
        frames.append((b, [7, 3, 1000, 0], b.copy(), [7, 3, 1000, 0]))
    r = _score(frames)
    assert r["TP"].tolist() == [20] * A and r["FN"].tolist() == [0] * A and r["FP"].tolist() == [0] * A
    for k in H.FIELDS:
        assert np.array_equal(r[k], np.ones(A)), k


@pytest.mark.parametrize("k", [1, 3])
def test_one_object_whose_track_id_changes_half_way(k):
    b = np.array([_box(0, 0)])
    frames = [(b, [0], b, [5 if f < k else 9]) for f in range(2 * k)]
    r = _score(frames)
    assert r["TP"].tolist() == [2 * k] * A
    for name, want in (("DetA", 1.0), ("DetRe", 1.0), ("DetPr", 1.0), ("AssA", 0.5), ("AssRe", 0.5), ("AssPr", 1.0), ("LocA", 1.0), ("HOTA", np.sqrt(0.5))):
        assert np.allclose(r[name], want, rtol=0, atol=1e-15), (name, r[name])


def test_one_pair_of_iou_one_third():
    r = _score([(np.array([[0, 0, 2, 1]]), [0], np.array([[1, 0, 3, 1]]), [0])])
    assert r["TP"].tolist() == [1] * 6 + [0] * 13                                     # the six alpha <= 0.30
    assert r["FN"].tolist() == [0] * 6 + [1] * 13 and r["FP"].tolist() == [0] * 6 + [1] * 13
    assert np.allclose(r["LocA"][:6], 1.0 / 3.0, rtol=0, atol=1e-15) and np.array_equal(r["LocA"][6:], np.ones(13))
    assert np.array_equal(r["AssA"], np.array([1.0] * 6 + [0.0] * 13)) and np.array_equal(r["HOTA"][6:], np.zeros(13))


def test_the_two_empty_sequence_rules():
    b = np.array([_box(0, 0), _box(10, 0)])
    none = np.zeros((0, 4))
    r = _score([(b, [0, 1], none, []), (b[:1], [0], none, [])])                      # no tracker boxes at all
    assert r["FN"].tolist() == [3] * A and r["TP"].tolist() == [0] * A and r["FP"].tolist() == [0] * A
    assert np.array_equal(r["LocA"], np.ones(A)) and all(np.array_equal(r[k], np.zeros(A)) for k in H.FIELDS if k != "LocA")
    r = _score([(none, [], b, [4, 2]), (none, [], b[:1], [2])])                      # no ground truth
    assert r["FP"].tolist() == [3] * A and r["TP"].tolist() == [0] * A and r["FN"].tolist() == [0] * A
    assert np.array_equal(r["LocA"], np.ones(A)) and all(np.array_equal(r[k], np.zeros(A)) for k in H.FIELDS if k != "LocA")
    r = _score([])
    assert r["TP"].tolist() == [0] * A and np.array_equal(r["LocA"], np.ones(A))


def test_mixed_frames_count_the_unmatched_side():
    """A frame with ground truth only, a frame with tracks only, a frame with both: FN and FP per the frame rules, counts of the ids include the lone frames."""
    b = np.array([_box(0, 0)])
    none = np.zeros((0, 4))
    r = _score([(b, [0], none, []), (none, [], b, [0]), (b, [0], b, [0])])
    assert r["TP"].tolist() == [1] * A and r["FN"].tolist() == [1] * A and r["FP"].tolist() == [1] * A
    assert np.allclose(r["AssA"], 1.0 / 3.0, rtol=0, atol=1e-15)                      # 1 x 1 / (2 + 2 - 1)
    assert np.allclose(r["AssRe"], 0.5, rtol=0, atol=1e-15) and np.allclose(r["AssPr"], 0.5, rtol=0, atol=1e-15)


def test_combination_rule_against_a_hand_sum():
    b = np.array([_box(0, 0)])
    one = H.score_sequence([(b, [0], b, [5 if f < 2 else 9]) for f in range(4)])      # TP 4, AssA 0.5, loc 4
    two = H.score_sequence([(np.array([[0, 0, 2, 1]]), [0], np.array([[1, 0, 3, 1], [50, 50, 52, 51]]), [0, 1])])   # IoU 1/3 and a stray track
    r = H.combine([one, two])
    lo, hi = 0, 9                                                                      # alpha = 0.05 and alpha = 0.5
    assert (r["TP"][lo], r["FN"][lo], r["FP"][lo]) == (5, 0, 1) and (r["TP"][hi], r["FN"][hi], r["FP"][hi]) == (4, 1, 2)
    assert abs(r["AssA"][lo] - (0.5 * 4 + 1.0 * 1) / 5) <= 1e-15 and abs(r["AssA"][hi] - 0.5) <= 1e-15
    assert abs(r["AssPr"][lo] - (1.0 * 4 + 1.0 * 1) / 5) <= 1e-15 and abs(r["AssRe"][lo] - (0.5 * 4 + 1.0) / 5) <= 1e-15
    assert abs(r["DetA"][lo] - 5 / 6) <= 1e-15 and abs(r["DetA"][hi] - 4 / 7) <= 1e-15
    assert abs(r["DetRe"][hi] - 4 / 5) <= 1e-15 and abs(r["DetPr"][hi] - 4 / 6) <= 1e-15
    assert abs(r["HOTA"][lo] - np.sqrt(5 / 6 * 0.6)) <= 1e-15 and abs(r["HOTA"][hi] - np.sqrt(4 / 7 * 0.5)) <= 1e-15
    assert abs(r["LocA"][lo] - (4 + 1 / 3) / 5) <= 1e-15 and r["LocA"][hi] == 1.0
    s = H.summary(r)
    assert set(s) == set(H.FIELDS) and abs(s["DetA"] - float(np.mean(r["DetA"]))) == 0


def test_at_most_one_case_in_eight_is_dropped():
    kept = H.kept_cases()
    assert len(kept) >= 14 and {c[1:] for c in kept} == {(12, 24), (40, 30), (60, 12)}
    closest = min(H.closest_to_a_threshold(H.case(*c)[1]) for c in kept)
    hota = [H.summary(H.finalize(H.case(*c)[1]))["HOTA"] for c in kept]
    print("kept %d of %d; closest similarity to a threshold %.3g; mean HOTA %.4f (%.4f .. %.4f)" % (len(kept), len(H.CASES), closest, np.mean(hota), min(hota),
                                                                                             max(hota)))
    assert closest >= H.MARGIN and 0.3 < np.mean(hota) < 0.8                           # neither trivial nor hopeless: every field is exercised
    big = [H.case(*c) for c in kept if c[1] == 40]
    assert big and all(b[1]["n_trk_ids"] > 64 for b in big)                            # an id space beyond one wave
    full = [H.case(*c) for c in kept if c[1] == 60]
    assert full and max(len(fr[3]) for b in full for fr in b[0]) > 48                  # near-full frames


def test_reference_agrees_with_scipy_on_the_kept_cases(monkeypatch):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment

    def scipy_max(M):
        M = np.asarray(M, dtype=np.float64)
        r, c = lsa(-M)
        return sorted((int(a), int(b)) for a, b in zip(r, c))

    for c in H.kept_cases():
        frames, base, _ = H.case(*c)
        monkeypatch.setattr(H.R, "assign_max", scipy_max)
        other = H.score_sequence(frames)
        monkeypatch.undo()
        assert H._decided(other) == H._decided(base), c
        assert np.array_equal(other["TP"], base["TP"])
        assert np.abs(H.finalize(other)["HOTA"] - H.finalize(base)["HOTA"]).max() <= 1e-12, c


def _tool():
    spec = importlib.util.spec_from_file_location("eval_track", os.path.join(ROOT, "tools", "track", "eval_track.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_eval_track_parser(tmp_path):
    mod = _tool()
    p = tmp_path / "a.txt"
    p.write_text("1,3,10.5,20,4,2,0.9,-1,-1,-1\n\n2,3,11.5,20,4,2,0.8,-1,-1,-1\n1,7,-3,-1,2.5,1,0.7,-1,-1,-1\n")
    rec = mod.read_mot(str(p))
    assert sorted(rec) == [1, 2] and rec[1][0] == [3, 7] and rec[2][0] == [3]
    assert rec[1][1].dtype == np.float32 and rec[1][1].tolist() == [[10.5, 20.0, 14.5, 22.0], [-3.0, -1.0, -0.5, 0.0]]
    assert rec[2][1].tolist() == [[11.5, 20.0, 15.5, 22.0]]
    frames = mod.sequence_frames({4: rec[1]}, {2: rec[2]})                             # frames 2, 3, 4: the middle one is empty on both sides
    assert [(f[0], len(f[1]), f[2], len(f[3])) for f in frames] == [([], 0, [3], 1), ([], 0, [], 0), ([3, 7], 2, [], 0)]
    (tmp_path / "bad.txt").write_text("1,2,3\n")
    with pytest.raises(ValueError):
        mod.read_mot(str(tmp_path / "bad.txt"))
    os.makedirs(str(tmp_path / "agent0"))
    (tmp_path / "agent0" / "5.txt").write_text("")
    assert mod.list_files(str(tmp_path)) == ["a.txt", os.path.join("agent0", "5.txt"), "bad.txt"]


def test_c_abi_entries_validate_without_a_gpu():
    """v2x_hota_workspace_size / v2x_hota_sequences exist in the library and in the binding; sizes out of range give 0 / -22 with a message before any HIP
    call; the workspace size is the sum the header describes and guards against overflow."""
    from v2x_sim_amd import _lib
    lib = _lib.load()
    size = lib.v2x_hota_workspace_size
    S, F, cap, NG, NT, na = 50, 100, 40, 40, 80, 19
    tiles = (NT + 63) // 64
    want = 0
    for elem, n in ((8, S * F * cap * cap), (8, S * F * cap * cap), (8, S * NG * NT), (8, S * F * cap), (8, S * na * NG * tiles * 3), (8, S * na * NG),
                    (4, S * NG), (4, S * NT), (4, S * F * cap), (4, S * F * cap), (4, S * F * cap), (4, S * F), (4, S * F), (4, S * na * NG)):
        want += (elem * n + 15) // 16 * 16
    assert size(S, F, cap, NG, NT, na) == want
    assert size(0, 1, 1, 0, 0, 1) == 16 and size(1, 1, 1, 0, 0, 1) > 0
    for bad in ((-1, 1, 1, 1, 1, 1), (1, 0, 1, 1, 1, 1), (1, 1, 0, 1, 1, 1), (1, 1, 65, 1, 1, 1), (1, 1, 1, -1, 1, 1), (1, 1, 1, 1, -1, 1), (1, 1, 1, 1, 1, 0),
                (1, 1, 1, 1, 1, 33)):
        assert size(*bad) == 0, bad
    big = 2 ** 31 - 1
    assert size(big, big, 64, big, big, 32) == 0                                      # overflows 64 bits: refused, not wrapped
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(S=1, F=1, cap=1, NG=1, NT=1, na=1, ws=1 << 20, ptr=p):
        return lib.v2x_hota_sequences(ptr, p, p, p, p, p, S, F, cap, NG, NT, p, na, p, ws, p, p, None)

    for kw, text in ((dict(ptr=None), b"null pointer"), (dict(S=-1), b"n_seq"), (dict(F=0), b"n_frames"), (dict(cap=65), b"cap = 65"), (dict(cap=0), b"cap = 0"),
                     (dict(NG=-1), b"n_gt_ids"), (dict(na=33), b"n_alpha = 33"), (dict(na=0), b"n_alpha = 0"), (dict(ws=8), b"workspace of 8 bytes"),
                     (dict(S=1 << 20, F=1 << 10, ws=2 ** 62), b"2^24"), (dict(S=big, F=big, cap=64, NG=big, NT=big, na=32), b"overflows")):
        assert call(**kw) == -22, kw
        assert text in lib.v2x_last_error(), (kw, lib.v2x_last_error())

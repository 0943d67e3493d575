"""CPU tests of row f-5 (tracking): the float64 references of tests/track_refs.py against independent statements (brute force, scipy, hand-counted
sequences), the conditions the GPU tests rest on (enough generated cases survive the coin-flip filter; the two association readings really
differ; the covariance pattern the kernel stores is the whole covariance), and the C ABI's two entries as far as they go without a GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import track_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _total(M, pairs):
    return sum(M[r, c] for r, c in pairs)


def test_assignment_equals_brute_force():
    """200 random matrices with min(rows, cols) <= 7, both orientations, some with ties (quantised) and zeros."""
    rng = np.random.default_rng(11)
    for k in range(200):
        nr, nc = int(rng.integers(1, 8)), int(rng.integers(1, 8))
        M = rng.random((nr, nc))
        if k % 3 == 0:
            M = np.round(M * 8) / 8
        if k % 5 == 0:
            M[rng.random((nr, nc)) < 0.4] = 0
        pairs = R.assign_max(M)
        assert len(pairs) == min(nr, nc)
        assert len({r for r, _ in pairs}) == len(pairs) == len({c for _, c in pairs})
        assert abs(_total(M, pairs) - R.assign_brute(M)) <= 1e-12, (k, M)


def test_assignment_equals_scipy():
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(12)
    for k in range(60):
        nr, nc = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        M = rng.random((nr, nc))
        r, c = lsa(-M)
        assert abs(M[r, c].sum() - _total(M, R.assign_max(M))) <= 1e-10


def test_direct_reading_on_a_built_matrix():
    """One entry above the threshold per row and column: direct takes it; the optimal assignment prefers two sub-threshold entries of larger sum."""
    M = np.array([[0.35, 0.29], [0.29, 0.0]])
    assert R.associate(M, 0.3, True).tolist() == [0, -1]
    assert R.associate(M, 0.3, False).tolist() == [-1, -1]
    M2 = np.array([[0.5, 0.4], [0.45, 0.0]])          # two entries above the threshold in row 0: both readings assign
    assert R.associate(M2, 0.3, True).tolist() == R.associate(M2, 0.3, False).tolist() == [1, 0]
    bad = np.array([[np.nan, 0.6], [np.inf, 0.1]])
    assert R.associate(bad, 0.3, False).tolist() == [1, -1]


def test_enough_generated_cases_are_kept():
    """The filter's cap is a CONDITION: of seeds 0..39 at least 36 survive, for either reading (otherwise the generator is wrong, not the cap)."""
    for direct in (False, True):
        n = sum(R.kept(s, direct) for s in range(40))
        print("direct=%d: %d of 40 kept" % (direct, n))
        assert n >= 36, (direct, n)


def test_the_two_readings_differ_and_the_covariance_keeps_its_pattern_and_fp32_decides_alike():
    differ, off = 0, 0.0
    for s in range(40):
        dets, _ = R.make_case(s)
        trk, fr = R.run_case(dets, True)
        differ += trk.readings_differ
        off = max(off, trk.offpattern)
        if s < 12:
            _, fr32 = R.run_case(dets, True, dtype=np.float32)
            assert R.decisions(fr32) == R.decisions(fr), s
    print("frames on which direct = 0 / 1 decide differently: %d of %d; largest off-pattern |P|: %.3g" % (differ, 40 * R.N_FRAMES, off))
    assert differ >= 1
    assert off < 1e-9


def _seq(mot, frames):
    for gt, gid, tb, tid in frames:
        mot.update(np.array(gt, dtype=np.float64).reshape(-1, 4), gid, np.array(tb, dtype=np.float64).reshape(-1, 4), tid)
    return mot.result()


A, B = [0, 0, 10, 10], [20, 0, 30, 10]
HAND_SEQUENCES = {
    "perfect": ([([A, B], [0, 1], [A, B], [5, 6])] * 4, dict(TP=8, FP=0, FN=0, IDSW=0, MOTA=1.0, MOTP=1.0)),
    "one_switch": ([([A, B], [0, 1], [A, B], [5, 6])] * 2 + [([A, B], [0, 1], [A, B], [5, 7])] * 2,
                   dict(TP=8, FP=0, FN=0, IDSW=1, MOTA=7 / 8, MOTP=1.0)),
    "miss_and_fp": ([([A, B], [0, 1], [A, B], [5, 6]), ([A, B], [0, 1], [A, [50, 50, 60, 60]], [5, 6]), ([A, B], [0, 1], [A, B], [5, 6])],
                    dict(TP=5, FP=1, FN=1, IDSW=0, MOTA=(5 - 1) / 6, MOTP=1.0)),
}


@pytest.mark.parametrize("name", sorted(HAND_SEQUENCES))
def test_clear_mot_reference_on_hand_written_sequences(name):
    frames, want = HAND_SEQUENCES[name]
    got = _seq(R.ClearMotRef(), frames)
    for k, v in want.items():
        assert got[k] == pytest.approx(v, abs=1e-12), (name, k, got)


def test_clear_mot_continuity_beats_the_better_iou():
    """TrackEval's +1000: a GT stays with its previous tracker while that pair passes the threshold, even when another tracker overlaps it more."""
    g = [0, 0, 10, 10]
    frames = [([g], [0], [g], [1]), ([g], [0], [[1, 0, 11, 10], g], [1, 2])]
    got = _seq(R.ClearMotRef(), frames)
    assert (got["TP"], got["FP"], got["IDSW"]) == (2, 1, 0)
    assert got["MOTP"] == pytest.approx((1 + 9 / 11) / 2)


def test_library_exports_and_validates_the_tracking_entries():
    """v2x_sort_step / v2x_assign_iou exist in the library and in the binding; bad arguments return -22 with a message before any HIP call."""
    from v2x_sim_amd import _lib
    lib = _lib.load()
    for name in ("v2x_sort_step", "v2x_assign_iou"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    p = ctypes.c_void_p(64)           # never dereferenced: validation comes first
    f = ctypes.c_float(0.3)

    def assign(iou=p, nr=p, nc=p, n=1, cap_r=8, cap_c=8, out=p):
        return lib.v2x_assign_iou(iou, nr, nc, n, cap_r, cap_c, f, 1, out, None)

    def sort(det=p, cnt=p, n=1, det_cap=64, fmt=0, tf=p, ti=p, si=p, t_cap=64, ob=p, oi=p, od=p, oc=p):
        return lib.v2x_sort_step(det, cnt, n, det_cap, fmt, tf, ti, si, t_cap, f, 1, 3, 1, ob, oi, od, oc, None)

    cases = ((assign, dict(iou=None), b"null"), (assign, dict(out=None), b"null"), (assign, dict(cap_c=65), b"cap_c"), (assign, dict(cap_r=0), b"cap_r"),
             (sort, dict(det=None), b"null"), (sort, dict(si=None), b"null"), (sort, dict(oc=None), b"null"), (sort, dict(t_cap=65), b"t_cap"),
             (sort, dict(t_cap=0), b"t_cap"), (sort, dict(fmt=3), b"box_format"), (sort, dict(fmt=-1), b"box_format"))
    for fn, kw, word in cases:
        assert fn(**kw) == -22, kw
        assert word in lib.v2x_last_error(), (kw, lib.v2x_last_error())
    assert assign(n=0) == 0 and sort(n=0) == 0      # nothing to do: no launch


def test_tracker_wrappers_refuse_host_tensors():
    import torch
    from v2x_sim_amd import ops
    from v2x_sim_amd.utils.mot_metrics import ClearMot
    from v2x_sim_amd.utils.tracking import SortTracker
    with pytest.raises(RuntimeError):
        SortTracker(2, device="cpu")
    z = torch.zeros
    with pytest.raises(RuntimeError):
        ops.sort_step(z(1, 8, 4), z(1, dtype=torch.int32), z(1, 8, 17), z(1, 8, 5, dtype=torch.int32), z(1, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        ops.assign_iou(z(1, 4, 4), z(1, dtype=torch.int32), z(1, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        ClearMot().update(z(1, 4), [0], z(1, 4), [1])


def test_track_kernels_have_no_scratch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_stats.py"), "track.hip"], capture_output=True, text=True, check=True).stdout
    kernels = re.findall(r"(sort_step_kernel|assign_kernel)\(.*\n\s+vgpr (\d+) agpr \S+ sgpr \d+ scratch (\d+)", out)
    assert sorted(k[0] for k in kernels) == ["assign_kernel", "sort_step_kernel"], out
    for name, vgpr, scratch in kernels:
        assert int(scratch) == 0 and int(vgpr) <= 128, (name, vgpr, scratch)

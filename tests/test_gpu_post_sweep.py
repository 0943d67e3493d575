"""The detection post-processing kernels (csrc/postprocess.hip: det_candidates_kernel, det_nms_kernel FAST and serial, rotated_iou_kernel,
match_detections_kernel) swept over candidate counts, ties, suppression chains and edges against the float64 references of tests/post_refs.py
-- seeded, the same cases every run; tests/test_post_refs_cpu.py checks the references and the conditions the assertions below rest on (every
consulted pair IoU 1e-3 from its threshold, score levels 1e-5 apart or bit-equal, match IoUs 1e-6 apart or bit-equal), so nothing here is
excluded or forgiven: kept anchors and their ORDER, true-positive flags and candidate sets are demanded exactly.  The bars are those of
tests/test_gpu_postprocess.py: boxes 1e-4 m and 1e-5 rad (modulo 2 pi), scores 1e-6, IoU 1e-6.

Each test prints its worst figure as a fraction of its bar (pytest -s shows them).  First run on 1x MI355X (the module: 43 tests, 4.7 s wall,
float64 references included; the slowest, the rotated 4096-candidate map, 0.95 s), worst error / bar: det_nms boxes 0.019 (1.9e-6 m), yaw 0.037,
scores 0.081 (8.1e-8: one fp32 rounding), counts / kept anchors / order exact in all 13 launches; FAST = serial bit for bit on 13 stand-up and 7
rotated maps (2146 + 1080 suppressions); decode x, y 0.000, w, h 0.047 (rtol 4.7e-8), yaw 0.032; candidate sets exact; rotated_iou 0.029 over
1025 x 1024 pairs, 0.014 in the grid-stride tail, iou(a, b) = iou(b, a) to the bit; best_iou 0.030, true-positive flags exact.
That first run FAILED test_rotated_iou_sweep: a rectangle against a POINT rectangle (w = h = 0) inside its stand-up box gave IoU 9.0e15
(pairs "box-around-empty" of post_refs.IOU_PAIRS; fixed in rotated_iou_d, csrc/HISTORY.md)."""
import ctypes as C

import numpy as np
import pytest
import torch

import post_refs as P
from oracle import postprocess_ref as PR

pytestmark = pytest.mark.gpu

BOX_BAR, YAW_BAR, SCORE_BAR, IOU_BAR = 1e-4, 1e-5, 1e-6, 1e-6

def _yaw_diff(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a, np.float64) - np.asarray(b, np.float64)))))


def _dev_launch(arr, anchors, device):
    t = {k: torch.from_numpy(v).to(device) for k, v in arr.items()}
    t["anchors"] = torch.from_numpy(anchors).to(device)
    return t


def _run_both(t, cap, nms_thr, rotated, score_thr=P.SCORE_THR):
    """-> {"slotted": outputs of det_nms_candidates on the built keys, "logits": outputs of det_postprocess on the logits}, as numpy."""
    from v2x_sim_amd import ops
    out = {"slotted": ops.det_nms_candidates(t["keys"], t["slot_codes"], t["counts"], t["anchors"], nms_thr, rotated=rotated),
           "logits": ops.det_postprocess(t["cls"], t["loc"], t["anchors"], score_thr, nms_thr, cap, rotated=rotated)}
    return {k: tuple(x.cpu().numpy() for x in v) for k, v in out.items()}


def _check_map(tag, got, i, r, exact_scores):
    """Map i of a launch against its reference r; -> (worst box error, worst yaw error, worst score error)."""
    boxes, scores, index, count = got
    assert int(count[i]) == r["count"], "%s: count %d, reference %d" % (tag, int(count[i]), r["count"])
    k = r["count"]
    if k <= 0:
        return 0.0, 0.0, 0.0
    assert np.array_equal(index[i, :k].astype(np.int64), r["index"]), "%s: kept anchors or their order differ from the reference" % tag
    bits = scores[i, :k].view(np.uint32)
    if exact_scores:
        assert np.array_equal(bits, r["score_bits"]), "%s: score bits" % tag
    else:           # equal logits give equal bits: the tie groups of the reference are tie groups of the kernel's scores
        assert np.array_equal(np.diff(bits) == 0, np.diff(r["score_bits"].astype(np.int64)) == 0), "%s: ties are not bit-equal" % tag
    es = float(np.abs(scores[i, :k].astype(np.float64) - r["scores"]).max())
    eb = float(np.abs(boxes[i, :k, :4].astype(np.float64) - r["boxes"][:, :4]).max())
    ey = float(_yaw_diff(boxes[i, :k, 4], r["boxes"][:, 4]).max())
    assert es < SCORE_BAR and eb < BOX_BAR and ey < YAW_BAR, (tag, es, eb, ey)
    return eb, ey, es


def _same_bits(tag, a, b):
    """Two launches: identical counts and, for every map, identical bits in everything it reports."""
    assert np.array_equal(a[3], b[3]), "%s: counts differ between two launches" % tag
    for i, k in enumerate(a[3]):
        k = max(int(k), 0)
        assert np.array_equal(a[0][i, :k].view(np.uint32), b[0][i, :k].view(np.uint32)) and np.array_equal(a[1][i, :k].view(np.uint32), b[1][i, :k].view(np.uint32)) \
            and np.array_equal(a[2][i, :k], b[2][i, :k]), "%s: map %d differs between two launches" % (tag, i)


# ------------------------------------------------------------------------------------------------------------------ NMS
@pytest.mark.parametrize("index", range(len(P.NMS_CASES)), ids=[c.name for c in P.NMS_CASES])
def test_nms_candidates_sweep(device, index):
    """Every map of the case in ONE launch, through both entries: v2x_det_nms_candidates on keys built from fp32 score bits (the slotted path:
    slots in seeded disorder, unused slots poisoned) and v2x_det_postprocess on logits that give the same candidates.  Both: the reference's
    count (-count for a map beyond cap, its neighbours unaffected), the kept anchors in the exact order, the score bits (slotted) or scores
    at 1e-6 with bit-equal ties (logits), boxes at 1e-4 m / 1e-5 rad of the float64 decode; a second launch gives identical bits."""
    d = P.make_nms_case(index)
    case = d["case"]
    t = _dev_launch(P.launch_arrays(d["maps"], d["anchors"], d["codes"], case.cap), d["anchors"], device)
    first = _run_both(t, case.cap, case.nms_thr, case.rotated)
    second = _run_both(t, case.cap, case.nms_thr, case.rotated)
    worst = [0.0, 0.0, 0.0]
    for path in ("slotted", "logits"):
        for i, (m, r) in enumerate(zip(d["maps"], d["refs"])):
            e = _check_map("%s %s map %d (%d candidates)" % (case.name, path, i, len(m["aid"])), first[path], i, r, path == "slotted")
            worst = [max(a, b) for a, b in zip(worst, e)]
        _same_bits("%s %s" % (case.name, path), first[path], second[path])
    print("det_nms %-32s counts %s -> %s  worst/bar: box %.3f yaw %.3f score %.3f" % (
        case.name, list(case.counts), [r["count"] for r in d["refs"]], worst[0] / BOX_BAR, worst[1] / YAW_BAR, worst[2] / SCORE_BAR))


def _serial_sources(rotated):
    """(case index, map index) of maps with 1 .. 512 candidates, at most two per case: the FAST form's side of the comparison."""
    out = []
    for ci, case in enumerate(P.NMS_CASES):
        if case.rotated != rotated:
            continue
        fit = sorted((i for i, c in enumerate(case.counts) if 0 < c <= min(P.NMS_FAST_CAP, case.cap)), key=lambda i: -case.counts[i])
        out += [(ci, i) for i in fit[:2]]
    return out


@pytest.mark.parametrize("rotated", [False, True], ids=["standup", "rotated"])
def test_fast_form_equals_serial_form_bitwise(device, rotated):
    """det_nms_kernel's header: "Same order, same overlap arithmetic, same decisions: identical detections".  No switch forces the serial form,
    so a map with <= 512 candidates (FAST) is run again with isolated candidates appended until it exceeds 512 (serial): they score below every
    original and overlap nothing, so they are kept and follow the originals -- whose k boxes, scores and indices must be bit for bit the
    unpadded map's, through both entries."""
    rng = np.random.default_rng(99)
    sources = _serial_sources(rotated)
    assert len(sources) >= 4 and any(P.NMS_CASES[ci].counts[i] == P.NMS_FAST_CAP for ci, i in sources)
    n_sup = 0
    for ci, i in sources:
        d = P.make_nms_case(ci)
        case, m, r = d["case"], d["maps"][i], d["refs"][i]
        c = len(m["aid"])
        pm, a2, c2 = P.pad_to_serial(m, d["anchors"], d["codes"], rng)
        extra = len(pm["aid"]) - c
        assert c <= P.NMS_FAST_CAP < c + extra <= 1024
        fast = _run_both(_dev_launch(P.launch_arrays([m], d["anchors"], d["codes"], case.cap), d["anchors"], device), case.cap, case.nms_thr, rotated)
        serial = _run_both(_dev_launch(P.launch_arrays([pm], a2, c2, 1024), a2, device), 1024, case.nms_thr, rotated)
        for path in ("slotted", "logits"):
            f, s = fast[path], serial[path]
            k = int(f[3][0])
            tag = "%s map %d (%d + %d candidates) %s" % (case.name, i, c, extra, path)
            assert k == r["count"] and int(s[3][0]) == k + extra, (tag, k, r["count"], int(s[3][0]))
            assert np.array_equal(f[2][0, :k], s[2][0, :k]), "%s: the two forms keep different anchors" % tag
            assert np.array_equal(f[1][0, :k].view(np.uint32), s[1][0, :k].view(np.uint32)), "%s: score bits" % tag
            assert np.array_equal(f[0][0, :k].view(np.uint32), s[0][0, :k].view(np.uint32)), "%s: box bits" % tag
            assert (s[2][0, k:k + extra] >= d["anchors"].shape[0]).all()
        n_sup += c - r["count"]
    assert n_sup > 100                                          # the compared maps did suppress
    print("fast = serial (%s): %d maps, %d suppressions, identical bits" % ("rotated" if rotated else "stand-up", len(sources), n_sup))


def test_decode_edges(device):
    """DECODE_CASES through an NMS threshold of 1.0 (nothing is suppressed), both entries, against postprocess_ref.decode_faf: x, y at 1e-4 m, yaw
    at 1e-5 rad modulo 2 pi, w and h at rtol 1e-6 (up to 4 exp(4) = 218 m an absolute bar means nothing)."""
    codes, anchors = P.DECODE_CASES
    n = len(codes)
    m = {"aid": np.arange(n), "margin": P.level_margin(np.arange(n)), "slot": np.random.default_rng(3).permutation(n)}
    got = _run_both(_dev_launch(P.launch_arrays([m], anchors, codes, 256), anchors, device), 256, 1.0, False)
    want = np.array([PR.decode_faf(codes[i], anchors[i]) for i in range(n)])
    for path in ("slotted", "logits"):
        boxes, scores, index, count = got[path]
        assert int(count[0]) == n and np.array_equal(index[0, :n], np.arange(n))
        b = boxes[0, :n].astype(np.float64)
        assert np.isfinite(b).all()
        exy = float(np.abs(b[:, :2] - want[:, :2]).max())
        ewh = float((np.abs(b[:, 2:4] - want[:, 2:4]) / want[:, 2:4]).max())
        ey = float(_yaw_diff(b[:, 4], want[:, 4]).max())
        print("decode %-8s worst/bar: xy %.3f  wh %.3f  yaw %.3f" % (path, exy / BOX_BAR, ewh / 1e-6, ey / YAW_BAR))
        assert exy < BOX_BAR and ewh < 1e-6 and ey < YAW_BAR, (path, exy, ewh, ey)


@pytest.mark.parametrize("thr,M", P.CAND_CASES)
def test_candidates_edges(device, thr, M):
    """det_candidates_kernel at the saturated ends of the softmax and at the thresholds 0, 0.5, 0.7, 1: the count (-count beyond cap) and the
    candidate SET equal the float64 rule exactly (NMS threshold 1.0 and boxes 3 m apart: every candidate is reported)."""
    from v2x_sim_amd import ops
    cls, passing, count = P.make_cand_case(thr, M)
    anchors = np.zeros((M, 6), np.float32)
    anchors[:, 0] = 3.0 * np.arange(M)
    anchors[:, 2:4] = 1.0
    anchors[:, 5] = 1.0
    loc = np.zeros((1, M, 6), np.float32)
    loc[..., 5] = 1.0
    _, _, index, cnt = ops.det_postprocess(torch.from_numpy(cls)[None].to(device), torch.from_numpy(loc).to(device), torch.from_numpy(anchors).to(device),
                                           thr, 1.0, P.CAND_CAP)
    assert int(cnt[0]) == count, (int(cnt[0]), count)
    if count >= 0:
        got = np.sort(index[0, :count].cpu().numpy())
        assert np.array_equal(got, passing), "candidate set differs: %s" % sorted(set(got.tolist()) ^ set(passing.tolist()))[:10]


# ------------------------------------------------------------------------------------------------------------------ rotated IoU
def test_rotated_iou_sweep(device):
    """The degenerate poses (zero width, both empty, needles, turns by pi, pi / 2, 2 pi, shared edges, corner contact, 1e4 m) pair by pair, and
    1025 x 1024 pairs -- beyond the 4096 x 256 threads of one grid pass -- against float64 at 1e-6; iou(a, b) and iou(b, a) agree at the same
    bar; nothing is NaN, in the full matrix of the degenerate boxes either."""
    from v2x_sim_amd import ops
    a, b = P.iou_pair_arrays()
    ref = np.array([P.iou_ref64(a[i:i + 1], b[i:i + 1])[0, 0] for i in range(len(a))])
    ad, bd = torch.from_numpy(a).to(device), torch.from_numpy(b).to(device)
    ab, ba = ops.rotated_iou(ad, bd).cpu().numpy().astype(np.float64), ops.rotated_iou(bd, ad).cpu().numpy().astype(np.float64)
    assert np.isfinite(ab).all() and np.isfinite(ba).all(), "NaN / inf for a degenerate rectangle"
    assert (ab >= 0).all() and (ab <= 1 + IOU_BAR).all()
    err = np.abs(np.diag(ab) - ref)
    for i, p in enumerate(P.IOU_PAIRS):
        assert err[i] < IOU_BAR, (p[0], float(np.diag(ab)[i]), float(ref[i]))
    sym = float(np.abs(ab - ba.T).max())
    assert sym < IOU_BAR, sym
    A, B, full, _ = P.make_iou_size_case()
    Ad, Bd = torch.from_numpy(A).to(device), torch.from_numpy(B).to(device)
    got = ops.rotated_iou(Ad, Bd).cpu().numpy().astype(np.float64)
    assert got.shape == full.shape and got.size > P.IOU_GRID_PASS and np.isfinite(got).all()
    e_all = np.abs(got - full)
    tail = float(e_all.reshape(-1)[P.IOU_GRID_PASS:].max())
    sym2 = float(np.abs(got - ops.rotated_iou(Bd, Ad).cpu().numpy().astype(np.float64).T).max())
    print("rotated_iou worst/bar: explicit pairs %.3f, symmetry %.3f; %d x %d: all %.3f, grid-stride tail %.3f, symmetry %.3f" % (
        float(err.max()) / IOU_BAR, sym / IOU_BAR, A.shape[0], B.shape[0], float(e_all.max()) / IOU_BAR, tail / IOU_BAR, sym2 / IOU_BAR))
    assert float(e_all.max()) < IOU_BAR and sym2 < IOU_BAR, (float(e_all.max()), sym2)


# ------------------------------------------------------------------------------------------------------------------ matching
@pytest.mark.parametrize("index", range(len(P.MATCH_CASES)), ids=[c[0] for c in P.MATCH_CASES])
def test_match_detections_sweep(device, index):
    """match_detections_kernel with up to 8192 ground truths per image (the strided scan, the tree reduction's lower-index rule across and
    within threads, no second choice), counts below 0 and beyond the capacities: tp equals the reference exactly, best_iou at 1e-6, with and
    without best_iou requested; rows past det_count keep what the buffers held."""
    from v2x_sim_amd import _lib, ops
    from v2x_sim_amd.ops_post import _dev, _stream
    det, dc, gt, gc, thr, refs = P.make_match_case(index)
    n, det_cap, gt_cap = det.shape[0], det.shape[1], gt.shape[1]
    d = lambda x: torch.from_numpy(x).to(device)
    detd, dcd, gtd, gcd = d(det), d(dc), d(gt), d(gc)
    tp_only = ops.match_detections(detd, dcd, gtd, gcd, thr).cpu().numpy()
    tp = torch.full((n, det_cap), -7, dtype=torch.int32, device=device)           # sentinels: an untouched row still holds them
    best = torch.full((n, det_cap), -7.0, dtype=torch.float32, device=device)
    _lib.check(_lib.load().v2x_match_detections(_dev(detd, torch.float32, "det"), _dev(dcd, torch.int32, "det_count"), det_cap, _dev(gtd, torch.float32, "gt"),
                                                _dev(gcd, torch.int32, "gt_count"), gt_cap, n, C.c_float(thr), _dev(tp, torch.int32, "tp"),
                                                _dev(best, torch.float32, "best"), _stream()), "v2x_match_detections")
    tp, best = tp.cpu().numpy(), best.cpu().numpy()
    worst = 0.0
    for i in range(n):
        rtp, rbest, _ = refs[i]
        nd = len(rtp)
        assert nd == min(max(int(dc[i]), 0), det_cap)
        assert np.array_equal(tp[i, :nd], rtp), (P.MATCH_CASES[index][0], i, tp[i, :nd].tolist(), rtp.tolist())
        assert np.array_equal(tp_only[i, :nd], rtp) and (tp_only[i, nd:] == 0).all()
        assert (tp[i, nd:] == -7).all() and (best[i, nd:] == -7.0).all(), "rows past det_count were written"
        if nd:
            worst = max(worst, float(np.abs(best[i, :nd].astype(np.float64) - rbest).max()))
    print("match_detections %-18s gt_cap %d: %d true positives of %d, best_iou worst/bar %.3f" % (
        P.MATCH_CASES[index][0], gt_cap, int(sum(r[0].sum() for r in refs)), int(sum(len(r[0]) for r in refs)), worst / IOU_BAR))
    assert worst < IOU_BAR, worst

"""Late fusion without a GPU: the float64 reference of tests/late_refs.py against brute force, every condition its case table must satisfy (nothing
is skipped at run time: a condition that does not hold fails), the pose convention against synthetic scenes' trans_geo, the numpy path
(utils/postprocess.late_fusion) against the reference, the scene property the GPU test asserts (here through the numpy path), and the drivers' flag."""
import importlib.util
import math
import os

import numpy as np
import pytest

import late_refs as LR
import post_refs as PR
from v2x_sim_amd.utils import postprocess as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _iou_standup(a, b):
    ca, cb = PR.standup64(PR.corners64(a[None]))[0], PR.standup64(PR.corners64(b[None]))[0]
    iw, ih = min(ca[2], cb[2]) - max(ca[0], cb[0]), min(ca[3], cb[3]) - max(ca[1], cb[1])
    inter = iw * ih if iw > 0 and ih > 0 else 0.0
    return inter / ((ca[2] - ca[0]) * (ca[3] - ca[1]) + (cb[2] - cb[0]) * (cb[3] - cb[1]) - inter)


def test_reference_on_hand_countable_cases():
    """Two agents, 3 m apart along x, the neighbour turned a quarter: unit-free numbers one can check by hand."""
    A, B, cap = 2, 1, 64
    poses = [LR.pose(0.0, 0.0, 0.0), LR.pose(math.pi / 2, 3.0, 0.0)]
    trans, geo = LR.trans_from_poses(poses)
    rigid = LR.rigid_ref(trans[None])
    boxes = np.zeros((2, cap, 5), np.float32)
    scores = np.zeros((2, cap), np.float32)
    # ego 0: a car at (5, 1) and one at (-10, 0).  Agent 1 sees the first at its own (1, -2) [= world (3 + 2, 0 + 1)] with a HIGHER score, one new car
    # at its (0, 20) [world (-17, 0)] and one at its (0, -40) [world (43, 0): outside +-32 for ego 0]
    boxes[0, :2] = [[5, 1, 2, 4, 0.0], [-10, 0, 2, 4, 0.0]]
    scores[0, :2] = [0.9, 0.8]
    boxes[1, :3] = [[1, -2, 2, 4, -math.pi / 2], [0, 20, 2, 4, 0.3], [0, -40, 2, 4, 0.0]]
    scores[1, :3] = [0.95, 0.85, 0.75]
    counts = np.array([2, 3], np.int32)
    link = np.ones((1, 2, 2), np.uint8)
    r = LR.ego_reference(boxes, scores, counts, rigid, link, A, B, cap, 64, LR.AREA, 0.01, False, 0, 0)
    assert r["count"] == 3 and r["src"].tolist() == [cap + 0, cap + 1, 1] and r["n_cand"] == 4        # the neighbour's copy of the first car wins
    np.testing.assert_allclose(r["boxes"][:, :2], [[5, 1], [-17, 0], [-10, 0]], atol=1e-5)
    np.testing.assert_allclose(r["boxes"][0, 4], 0.0, atol=1e-6)
    # the other way round: ego 1 gets ego 0's cars at its (1, -2) (suppressed by its own, better one) and (0, 13)
    r1 = LR.ego_reference(boxes, scores, counts, rigid, link, A, B, cap, 64, LR.AREA, 0.01, False, 1, 0)
    assert r1["src"].tolist() == [cap + 0, cap + 1, 1, cap + 2]
    np.testing.assert_allclose(r1["boxes"][2, :2], [0, 13], atol=1e-5)
    # links off: the ego's own list; ego absent: nothing; a negative linked count: not computed
    off = np.eye(2, dtype=np.uint8)[None]
    assert LR.ego_reference(boxes, scores, counts, rigid, off, A, B, cap, 64, LR.AREA, 0.01, False, 0, 0)["src"].tolist() == [0, 1]
    gone = np.array([[[0, 1], [1, 1]]], np.uint8)
    assert LR.ego_reference(boxes, scores, counts, rigid, gone, A, B, cap, 64, LR.AREA, 0.01, False, 0, 0)["count"] == 0
    neg = np.array([2, -5], np.int32)
    assert LR.ego_reference(boxes, scores, neg, rigid, link, A, B, cap, 64, LR.AREA, 0.01, False, 0, 0)["count"] == -65
    assert LR.ego_reference(boxes, scores, neg, rigid, off, A, B, cap, 64, LR.AREA, 0.01, False, 0, 0)["count"] == 2


@pytest.mark.parametrize("index", [0, 6, 8])
def test_reference_agrees_with_brute_force(index):
    d = LR.make_late_case(index)
    c = d["case"]
    for i in range(c.A):
        for b in range(c.B):
            r = d["refs"][i][b]
            if r["count"] <= 0:
                continue
            bx, sc, tie, src = LR.ego_candidates(d["boxes"], d["scores"], d["counts"], d["rigid"], d["link"], c.A, c.B, c.cap_in, c.extents, i, b)
            kept = LR.brute_force(bx.astype(np.float64), sc, tie, c.nms_thr, _iou_standup)
            assert src[kept].tolist() == r["src"].tolist()


# Egos per case with a positive count / count 0 / a negative count, worked out from the case definitions: cap_out + 1 merged candidates take a whole
# frame's egos out (a2-capout64-edge frame 2, a5-capout1024-edge frame 1); an absent agent or an ego without any candidate gives 0 (a6-absent: agents 1
# and 5 of frame 0; a1: the frame with no detection); a negative source takes out every ego that hears it (a5-negative-source: under its seeded mask
# only ego 4 of frame 0 and ego 0 of frame 2 do not hear the frame's negative agent).
EGOS_BY_SIGN = {"a2-small": (2, 0, 0), "a5-b3-rot": (15, 0, 0), "a6-fast-edge": (18, 0, 0), "a2-capout64-edge": (4, 0, 2), "a5-capout1024-edge": (10, 0, 5),
                "a6-serial-rot": (6, 0, 0), "a5-v2i": (15, 0, 0), "a5-asym": (15, 0, 0), "a6-absent": (16, 2, 0), "a5-negative-source": (2, 0, 13),
                "a1": (2, 1, 0), "a5-hostile-counts": (5, 0, 0)}


@pytest.mark.parametrize("index", range(len(LR.LATE_CASES)))
def test_case_table_conditions(index):
    d = LR.make_late_case(index)
    c = d["case"]
    counts = [d["refs"][i][b]["count"] for i in range(c.A) for b in range(c.B)]
    assert (sum(v > 0 for v in counts), sum(v == 0 for v in counts), sum(v < 0 for v in counts)) == EGOS_BY_SIGN[c.name]
    assert c.A in (1, 2, 5, 6) and c.B in (1, 3) and c.cap_in in (64, 256) and c.cap_out in (64, 1024)
    for i in range(c.A):
        for b in range(c.B):
            r = d["refs"][i][b]
            if r["count"] <= 0:                        # no suppression ran: nothing to hold (their number is asserted above)
                continue
            con = r["consulted"]
            assert (np.abs(con.iou - c.nms_thr) > PR.IOU_MARGIN).all(), (c.name, i, b, float(np.abs(con.iou - c.nms_thr).min()))
            s = np.sort(r["cand_scores"].astype(np.float64))
            gaps = np.diff(s)
            if c.scores == "distinct":
                assert (gaps >= 1e-5).all(), (c.name, i, b)
            else:
                assert ((gaps == 0) | (gaps >= 1e-5)).all() and (gaps == 0).any(), (c.name, i, b)
            assert len(set(r["cand_tie"].tolist())) == len(r["cand_tie"])
    for row in range(c.A * c.B):                       # every list is in descending score order, as the post-processor emits it
        n = min(max(int(d["counts"][row]), 0), c.cap_in)
        assert (np.diff(d["scores"][row, :n]) <= 0).all()


def test_case_table_covers_what_it_claims():
    """Merged counts 511 / 512 / 513 and cap_out / cap_out + 1, both suppression forms in both modes, suppressed AND surviving neighbours."""
    merged = {}
    for k, c in enumerate(LR.LATE_CASES):
        d = LR.make_late_case(k)
        merged[c.name] = [[d["refs"][i][b].get("n_cand", d["refs"][i][b]["count"]) for b in range(c.B)] for i in range(c.A)]
    assert merged["a6-fast-edge"][0] == [511, 512, 513]
    assert merged["a2-capout64-edge"][1] == [63, 64, -65]
    assert merged["a5-capout1024-edge"][2] == [1024, -1025, 1023]
    assert merged["a6-serial-rot"][0] == [600]
    d = LR.make_late_case(0)
    r = d["refs"][0][0]
    from_nb = int((r["src"] >= d["case"].cap_in).sum())
    assert 0 < from_nb and r["count"] < r["n_cand"]                       # neighbours contribute, and duplicates are suppressed
    neg = LR.make_late_case([c.name for c in LR.LATE_CASES].index("a5-negative-source"))
    counts = [[neg["refs"][i][b]["count"] for b in range(3)] for i in range(5)]
    assert any(v == -65 for row in counts for v in row) and any(v > 0 for row in counts for v in row)


def test_rigid_from_trans_agrees_with_trans_geo():
    """late_rigid_from_trans on the warp-convention `trans` of synthetic scenes reproduces the geometric trans_geo: the rotation block, the
    translation and the heading -- with zero error (both are fp32 roundings of the same float64 numbers)."""
    from v2x_sim_amd.utils.synthetic_scene import make_scene
    for seed in range(12):
        sc = make_scene(agents=5, n_cars=4, seed=seed, ground_pts=10, clutter_pts=10, pts_per_car=4, max_pts=256)
        r = P.late_rigid_from_trans(sc["trans"])
        assert r.dtype == np.float32 and r.shape == (5, 5, 8)
        assert np.array_equal(r, LR.rigid_ref(sc["trans"]))
        G = sc["trans_geo"]
        assert np.array_equal(r[..., [0, 1, 3, 4]], G[..., :2, :2].reshape(5, 5, 4))
        assert np.array_equal(r[..., 2], G[..., 0, 3]) and np.array_equal(r[..., 5], G[..., 1, 3])
        assert np.array_equal(r[..., 6], np.arctan2(G[..., 1, 0].astype(np.float64), G[..., 0, 0].astype(np.float64)).astype(np.float32))
        assert (r[..., 7] == 0).all()
    t = __import__("torch").from_numpy(sc["trans"])
    assert np.array_equal(P.late_rigid_from_trans(t), r)


def test_rigid_torch_derivation_equals_numpy():
    """late_rigid_from_trans_torch (what predict_all uses where the matrices already are) against late_rigid_from_trans, bit for bit, on the
    scenes' poses, the case table's and the quadrant edges of atan2 (CPU tensors here; tests/test_gpu_late_fuse.py repeats it on the device)."""
    import torch
    for T in LR.rigid_equality_inputs():
        got = P.late_rigid_from_trans_torch(torch.from_numpy(T))
        assert got.dtype == torch.float32
        assert np.array_equal(got.numpy().view(np.uint32), P.late_rigid_from_trans(T).view(np.uint32))


def _seq_from_arrays(boxes, scores, counts, A, B, cap_in):
    return [[None if counts[j * B + b] < 0 else {"boxes": boxes[j * B + b, :min(counts[j * B + b], cap_in)], "scores": scores[j * B + b, :min(counts[j * B + b], cap_in)]}
             for b in range(B)] for j in range(A)]


@pytest.mark.parametrize("index", [k for k, c in enumerate(LR.LATE_CASES) if not c.rotated and c.name != "a5-negative-source"])
def test_numpy_path_agrees_with_reference(index):
    """utils/postprocess.late_fusion (fp32 numpy, the host path) gives the reference's kept set, order and boxes; it has no capacity, so the cases
    that overflow cap_out are compared with the reference at a capacity that holds them."""
    d = LR.make_late_case(index)
    c = d["case"]
    seq = _seq_from_arrays(d["boxes"], d["scores"], d["counts"], c.A, c.B, c.cap_in)
    got = P.late_fusion(seq, d["trans"], c.A, c.extents, link=d["link"], nms_thr=c.nms_thr)
    for i in range(c.A):
        for b in range(c.B):
            r = d["refs"][i][b]
            if r["count"] < 0:
                r = LR.ego_reference(d["boxes"], d["scores"], d["counts"], d["rigid"], d["link"], c.A, c.B, c.cap_in, 1 << 20, c.extents, c.nms_thr, False, i, b)
            if not d["link"][b, i, i]:
                assert got[i][b] is None
                continue
            g = got[i][b]
            assert len(g["scores"]) == r["count"], (c.name, i, b)
            if r["count"]:
                assert np.array_equal(g["boxes"].view(np.uint32), r["boxes"].view(np.uint32))
                assert np.array_equal(g["scores"].view(np.uint32), r["score_bits"])
                assert g["src_agent"].tolist() == (r["src"] // c.cap_in).tolist()
                assert g["corners"].shape == (r["count"], 4, 2)


def test_numpy_path_h_along_heading_and_absent_agents():
    d = LR.make_late_case(0)
    c = d["case"]
    seq = _seq_from_arrays(d["boxes"], d["scores"], d["counts"], c.A, c.B, c.cap_in)
    ref = P.late_fusion(seq, d["trans"], c.A, c.extents)
    swapped = [[{"boxes": s["boxes"][:, [0, 1, 3, 2, 4]], "scores": s["scores"]} for s in row] for row in seq]
    got = P.late_fusion(swapped, d["trans"], c.A, c.extents, wh_axis="h_along_heading")
    for i in range(c.A):
        assert np.array_equal(got[i][0]["boxes"][:, [0, 1, 3, 2, 4]], ref[i][0]["boxes"])
        assert np.allclose(got[i][0]["corners"], ref[i][0]["corners"])
    seq[1][0] = None                                   # an absent agent sends nothing and gets nothing
    alone = P.late_fusion(seq, d["trans"], c.A, c.extents)
    assert alone[1][0] is None and np.array_equal(alone[0][0]["boxes"], seq[0][0]["boxes"])


def scene_maps(seed, fuse):
    """The scene property: with each agent's own ground truth as its detections, the late-fused lists are EXACTLY the cars in range of any agent.
    fuse(boxes, scores, counts, rigid, link) -> per ego (boxes (n, 5), scores (n,)).  -> (fused aps, ego-only aps, consulted IoUs)."""
    boxes, scores, counts, trans, gt_any, _ = LR.scene_inputs(seed)
    A = boxes.shape[0]
    rigid = P.late_rigid_from_trans(trans)
    link = np.ones((1, A, A), np.uint8)
    fused = fuse(boxes, scores, counts, rigid, link)
    ious = []
    for i in range(A):
        r = LR.ego_reference(boxes, scores, counts, rigid, link, A, 1, boxes.shape[1], 1024, LR.SCENE_CROP, 0.01, False, i, 0)
        ious.append(r["consulted"].iou)
        assert np.array_equal(fused[i][0].view(np.uint32), r["boxes"].view(np.uint32)), (seed, i)
    ann = [P.box_corners(g.astype(np.float64)) for g in gt_any]
    late = [{"corners": P.box_corners(fused[i][0].astype(np.float64)), "scores": fused[i][1]} for i in range(A)]
    ego = [{"corners": P.box_corners(boxes[i, :counts[i]].astype(np.float64)), "scores": scores[i, :counts[i]]} for i in range(A)]
    aps = {t: (P.eval_map(late, ann, t)[0], P.eval_map(ego, ann, t)[0]) for t in (0.5, 0.7)}
    return aps, np.concatenate(ious)


@pytest.mark.parametrize("seed", LR.SCENE_SEEDS)
def test_scene_property_through_the_numpy_path(seed):
    boxes, scores, counts, trans, _, _ = LR.scene_inputs(seed)
    A = boxes.shape[0]

    def fuse(bx, sc, cn, rigid, link):
        out = P.late_fusion(_seq_from_arrays(bx, sc, cn, A, 1, bx.shape[1]), trans, A, LR.SCENE_CROP, link=link)
        return [(out[i][0]["boxes"], out[i][0]["scores"]) for i in range(A)]
    aps, ious = scene_maps(seed, fuse)
    assert (np.abs(ious - 0.01) > 1e-3).all()
    for t in (0.5, 0.7):
        assert aps[t][0] == 1.0, (seed, t, aps[t])
        assert aps[t][1] <= 0.66, (seed, t, aps[t])


def test_scene_property_fails_under_a_wrong_convention():
    """The plain (t_x, t_y) reading of the translation, or the inverse direction, cannot reach mAP 1."""
    boxes, scores, counts, trans, gt_any, geo = LR.scene_inputs(0)
    A = boxes.shape[0]
    seq = _seq_from_arrays(boxes, scores, counts, A, 1, boxes.shape[1])
    ann = [P.box_corners(g.astype(np.float64)) for g in gt_any]
    for wrong in (geo[None], np.swapaxes(trans, 1, 2)):       # trans_geo read as if it were the warp's; trans[j, i] for trans[i, j]
        out = P.late_fusion(seq, wrong, A, LR.SCENE_CROP)
        late = [{"corners": P.box_corners(out[i][0]["boxes"].astype(np.float64)), "scores": out[i][0]["scores"]} for i in range(A)]
        assert P.eval_map(late, ann, 0.5)[0] < 0.9


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_both_drivers_take_com_late():
    """The detection driver's own file is part of the test surface and stays as it is: --com late goes through tools/det/eval_codet.py
    (comm.run_eval_driver), which runs the driver as --com lowerbound with late fusion switched on for the FaFModule it builds, --only_v2i as the
    link mask of the exchanged boxes.  The tracking driver has the flag itself."""
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.det import FaFNet
    from v2x_sim_amd.utils import comm
    from v2x_sim_amd.utils.CoDetModule import FaFModule
    det = _load(os.path.join(ROOT, "tools", "det", "test_codet.py"), "late_test_codet")
    seen = {}

    def driver(argv):
        args = det.build_parser().parse_args(argv)             # what reaches the driver parses with ITS parser
        m = FaFModule(FaFNet(Config("test"), kd_flag=0, num_agent=2), None, Config("test"), None, 0)
        seen.update(com=args.com, batch=args.batch, late=m.late_fusion, v2i=m.late_only_v2i)
        m.late_stats["egos"] += 2
        m.late_stats["kept"] += 7
        m.late_stats["from_neighbours"] += 3
        return {0.5: 0.25}
    res = comm.run_eval_driver(driver, ["--data", "d", "--com", "late", "--only_v2i", "1", "--batch", "2"])
    assert seen == {"com": "lowerbound", "batch": 2, "late": True, "v2i": True}
    assert res == {0.5: 0.25, "late_kept": 7, "late_from_neighbours": 3}
    comm.run_eval_driver(driver, ["--data", "d", "--com", "late"])
    assert seen["late"] and not seen["v2i"]
    comm.run_eval_driver(driver, ["--data", "d", "--com", "lowerbound"])
    assert seen == {"com": "lowerbound", "batch": 1, "late": False, "v2i": False}          # nothing leaks out of the block
    with pytest.raises(SystemExit):
        comm.run_eval_driver(driver, ["--data", "d", "--com", "late", "--compress_level", "2"])
    trk = _load(os.path.join(ROOT, "tools", "track", "track_codet.py"), "late_track_codet")
    assert trk.build_parser().parse_args(["--data", "d", "--out", "o", "--com", "late"]).com == "late"
    with pytest.raises(SystemExit):
        trk.build_parser().parse_args(["--data", "d", "--out", "o", "--com", "later"])


def test_abi_argument_checks_without_gpu():
    """v2x_det_late_fuse: A*B == 0 returns before the null-pointer checks; bad capacities and null pointers give -22 with the error text."""
    from v2x_sim_amd import _lib
    lib = _lib.load()
    f = lib.v2x_det_late_fuse
    z = (0.0, 0.0, 0.0, 0.0, 0.01)
    assert f(None, None, None, 0, 3, 64, None, None, *z, 0, 64, None, None, None, None, None) == 0
    assert f(None, None, None, 5, 0, 7, None, None, *z, 0, 9, None, None, None, None, None) == 0
    assert f(None, None, None, 5, 1, 64, None, None, *z, 0, 64, None, None, None, None, None) == -22 and b"null pointer" in lib.v2x_last_error()
    for cap_in, cap_out in ((63, 64), (64, 96), (8192, 64), (64, 32), (64, 8192)):
        assert f(None, None, None, 5, 1, cap_in, None, None, *z, 0, cap_out, None, None, None, None, None) == -22
        assert b"power of two" in lib.v2x_last_error()
    assert f(None, None, None, -1, 1, 64, None, None, *z, 0, 64, None, None, None, None, None) == -22

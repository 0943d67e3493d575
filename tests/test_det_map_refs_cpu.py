"""CPU checks of the detection-mAP work (no GPU): the float64 reference of tests/det_map_refs.py against the two host implementations of eval_map,
the condition every case must satisfy, the argument validation of v2x_det_map / v2x_det_map_workspace_size before any HIP call, the binding, the
tool's flag and DetMap's input checks."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import det_map_refs as R
import post_refs as PR


def _small(case):
    return int(case["ref"]["num_det"].sum()) <= R.HOST_MAX_DET and case["gt_cap"] <= 64


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_condition_holds_and_reference_equals_host_eval_map(name):
    """make_case raises when a detection's best IoU comes within post_refs.MATCH_MARGIN of a threshold or of its runner-up (designed exact ties
    excepted); on every case small enough for them, the reference AP equals oracle/postprocess_ref.py::eval_map and utils/postprocess.py::eval_map
    per group and threshold to 1e-12, and the counts agree."""
    from oracle import postprocess_ref as O
    from v2x_sim_amd.utils import postprocess as P
    case = R.make_case(name)
    worst = R.check_condition(case)
    print("%-26s maps %4d  detections %5d  margins: threshold %.3g, runner-up %.3g" % (name, len(case["group"]), int(case["ref"]["num_det"].sum()), worst[0], worst[1]))
    assert min(worst) >= PR.MATCH_MARGIN
    ref = case["ref"]
    assert ref["ap"].shape == (case["n_groups"], len(case["thrs"])) and (ref["ap"] >= 0).all() and (ref["ap"] <= 1 + 1e-15).all()
    if not _small(case):
        return
    for g in range(case["n_groups"]):
        dets, gts = R.host_lists(case, g)
        for t, thr in enumerate(case["thrs"]):
            thr = float(np.float32(thr))
            ap_o, num_gt, num_det = O.eval_map([[(float(s), c.tolist()) for s, c in zip(d["scores"], d["corners"])] for d in dets],
                                               [c.tolist() for c in gts], thr)
            ap_p, info = P.eval_map(dets, gts, thr)
            assert (num_gt, num_det) == (ref["num_gt"][g], ref["num_det"][g]) == (info["num_gt"], info["num_det"])
            assert abs(ref["ap"][g, t] - ap_o) <= 1e-12 and abs(ref["ap"][g, t] - ap_p) <= 1e-12, (name, g, thr, ref["ap"][g, t], ap_o, ap_p)


def test_case_table_covers_what_it_must():
    """The designed properties of the cases, read off the reference: the per-threshold taken sets matter, the ties tie, the lists have their lengths."""
    c = R.make_case("taken-0.5-0.7")
    assert c["ref"]["tp"][0, 0, :2].tolist() == [1, 0] and c["ref"]["tp"][1, 0, :2].tolist() == [0, 1]       # A then B on one ground truth
    c = R.make_case("taken-0.7-0.5")
    assert c["ref"]["tp"][1, 0, :2].tolist() == [1, 0] and c["ref"]["tp"][0, 0, :2].tolist() == [0, 1]
    c = R.make_case("taken-0.5-0.5-0.7")
    assert np.array_equal(c["ref"]["tp"][0], c["ref"]["tp"][1]) and not np.array_equal(c["ref"]["tp"][0], c["ref"]["tp"][2])
    c = R.make_case("all-equal")                    # the rank is the image-major order within each group
    for g in range(2):
        ranks = [c["ref"]["rank"][i, j] for i in np.nonzero(c["group"] == g)[0] for j in range(c["det_count"][i])]
        assert ranks == list(range(len(ranks)))
    c = R.make_case("signed-zero")                  # map 0's -0.0 ranks before map 1's +0.0: the VALUES tie, the map index decides
    assert np.signbit(c["scores"][0, 1]) and c["scores"][1, 0] == 0 and not np.signbit(c["scores"][1, 0])
    assert c["ref"]["rank"][0, 1] < c["ref"]["rank"][1, 0] and c["ref"]["rank"][0, 2] < c["ref"]["rank"][1, 0]
    for L in R.LIST_LENGTHS:
        c = R.make_case("length-%d" % L)
        assert c["ref"]["num_det"].tolist() == [L, 7]
        assert 0 < c["ref"]["num_tp"][0, 1] <= c["ref"]["num_tp"][0, 0] or L == 1
    c = R.make_case("scale")
    assert len(c["group"]) == 200 and c["gt_cap"] == 64 and 25 <= c["ref"]["num_det"].sum() / 200 <= 35
    assert (c["ref"]["ap"] > 0.05).all() and (c["ref"]["ap"][:, 0] > c["ref"]["ap"][:, 1]).all()
    c = R.make_case("gt-cap-8192")
    assert c["gt_cap"] == 8192 and len(c["group"]) == 3
    c = R.make_case("padding")
    assert c["det_count"][0] > c["det_cap"] and c["gt_count"][0] > c["gt_cap"] and (c["det_count"] < 0).any() and (c["gt_count"] < 0).any()
    assert np.isnan(c["det"][2, 3:]).all() and np.isnan(c["scores"][3, 4:]).all()
    for name in ("interleaved-agent-major", "interleaved-frame-major"):
        c = R.make_case(name)
        assert (c["group"] == -1).sum() == 3 and np.isnan(c["scores"][c["group"] == -1][:, :2]).all()


def test_entry_points_validate_without_a_device():
    """Both entries exist in the library and in the binding (ABI 18: additive); every bad-dimension class gives -1 / -22 with a message before any
    HIP call; n_img == 0 is V2X_OK with null pointers."""
    from v2x_sim_amd import _lib
    lib = _lib.load()
    assert lib.v2x_abi_version() == _lib.ABI_VERSION == 18
    assert "v2x_det_map" in _lib.SIGNATURES and "v2x_det_map_workspace_size" in _lib.SIGNATURES
    assert _lib.SIGNATURES["v2x_det_map_workspace_size"] == (C.c_longlong, [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int])
    assert len(_lib.SIGNATURES["v2x_det_map"][1]) == 21
    size = lib.v2x_det_map_workspace_size
    assert size(0, 64, 64, 1, 1) == 0 and size(10, 64, 8192, 64, 8) == 2 * 10 * 64 and size(1, 4096, 1, 1, 1) == 2 * 4096
    bad = [(-1, 64, 64, 1, 1), (4, 0, 64, 1, 1), (4, 4097, 64, 1, 1), (4, 64, 0, 1, 1), (4, 64, 8193, 1, 1), (4, 64, 64, 0, 1), (4, 64, 64, 65, 1),
           (4, 64, 64, 1, 0), (4, 64, 64, 1, 9), ((1 << 31) // 64, 64, 64, 1, 1), (1 << 40, 1, 1, 1, 1), (1 << 62, 4096, 1, 1, 1)]
    p = C.c_void_p(64)          # never dereferenced: every call below fails (or returns) before a launch

    def call(n, det_cap, gt_cap, ng, nt, ptr=p, ws=p, ws_bytes=1 << 40, req=None):
        a = [ptr] * 11 if req is None else req
        return lib.v2x_det_map(a[0], a[1], a[2], det_cap, a[3], a[4], gt_cap, a[5], n, ng, a[6], nt, a[7], a[8], a[9], a[10], None, None, ws, ws_bytes, None)
    for dims in bad:
        assert size(*dims) == -1, dims
        assert call(*dims) == -22 and b"v2x_det_map" in lib.v2x_last_error(), dims
    assert size((1 << 31) // 64 - 1, 64, 64, 1, 1) > 0
    for k in range(11):          # each required pointer
        req = [p] * 11
        req[k] = None
        assert call(4, 64, 64, 1, 2, req=req) == -22 and b"null pointer" in lib.v2x_last_error(), k
    assert call(4, 64, 64, 1, 2, ws=None) == -22 and b"workspace" in lib.v2x_last_error()
    assert call(4, 64, 64, 1, 2, ws_bytes=2 * 4 * 64 - 1) == -22 and b"workspace" in lib.v2x_last_error()
    assert call(0, 64, 64, 1, 2, ptr=None, ws=None, ws_bytes=0) == 0          # torch's empty tensors have null data pointers
    assert call(0, -5, 0, 0, 0, ptr=None, ws=None, ws_bytes=0) == 0           # ... whatever the other arguments are


def test_tool_takes_map_engine():
    """build_parser() of tools/det/map_codet.py -- tools/det/test_codet.py's own parser plus --map_engine host|device, default host, other values
    refused -- and tools/det/eval_codet.py drives that file."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("map_codet", os.path.join(root, "tools", "det", "map_codet.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ap = tool.build_parser()
    assert ap.parse_args(["--data", "x"]).map_engine == "host"
    assert ap.parse_args(["--data", "x", "--map_engine", "device"]).map_engine == "device"
    assert ap.parse_args(["--data", "x", "--map_engine", "host", "--com", "disco", "--score_thr", "0.6"]).com == "disco"
    with pytest.raises(SystemExit):
        ap.parse_args(["--data", "x", "--map_engine", "numpy"])
    assert tool._without_flag(["--data", "x", "--map_engine", "host", "--log", "--map_engine=host"]) == ["--data", "x", "--log"]
    assert "map_codet.main" in open(os.path.join(root, "tools", "det", "eval_codet.py")).read()


def test_detmap_input_checks():
    from v2x_sim_amd import ops
    from v2x_sim_amd.utils.det_metrics import DetMap
    assert callable(ops.det_map)
    m = DetMap(iou_thrs=(0.5, 0.7), n_groups=2)
    box = np.array([[0, 0, 2, 4, 0.1]], np.float32)
    with pytest.raises(ValueError):
        m.update({"boxes": box, "scores": np.array([np.nan], np.float32)}, box)
    with pytest.raises(ValueError):
        m.update({"boxes": box, "scores": np.array([np.inf], np.float32)}, box)
    with pytest.raises(ValueError):
        m.update({"boxes": box, "scores": np.array([0.5], np.float32)}, box, group=2)
    with pytest.raises(ValueError):
        DetMap(iou_thrs=(0.0,))
    with pytest.raises(ValueError):
        DetMap(iou_thrs=(0.5,) * 9)
    with pytest.raises(ValueError):
        DetMap(n_groups=65)
    with pytest.raises(ValueError):
        DetMap(wh_axis="sideways")
    # update sorts stably by descending score and exchanges the extents of both sides for h_along_heading
    m = DetMap(wh_axis="h_along_heading")
    two = np.array([[0, 0, 2, 4, 0.1], [5, 5, 1, 3, 0.2]], np.float32)
    m.update({"boxes": two, "scores": np.array([0.2, 0.9], np.float32)}, box)
    boxes, scores, gt, group = m._maps[0]
    assert scores.tolist() == [np.float32(0.9), np.float32(0.2)] and boxes[0].tolist() == [5, 5, 3, 1, np.float32(0.2)] and gt[0, 2:4].tolist() == [4, 2] and group == 0
    r = DetMap(n_groups=3).result()          # nothing collected: zeros, no device needed
    assert r["ap"].shape == (3, 2) and not r["ap"].any() and r["mean_ap"].tolist() == [0, 0] and r["num_gt"].tolist() == [0, 0, 0]

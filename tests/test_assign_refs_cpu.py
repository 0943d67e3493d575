"""CPU tests of the IoU anchor assignment's float64 reference (tests/assign_refs.py) and of the feature's host-side plumbing: the vectorised IoU against
a brute-force clip, hand-made cases of the rule, the zero-undecided condition of the committed case table, the sparse-key round trip through the
dataset loader, the C entries and the driver switch."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest
import torch

import assign_refs as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = math.pi


def _anchor5(anchors, ix, iy, a):
    return AR.anchor_boxes64(anchors[ix:ix + 1, iy:iy + 1, a:a + 1])[0]


def _flat(anchors, ix, iy, a):
    return (ix * anchors.shape[1] + iy) * anchors.shape[2] + a


def test_vectorised_iou_matches_brute_force():
    """The hull-of-points intersection, vectorised over anchors, against a Python Sutherland-Hodgman clip pair by pair: random boxes, and the special
    positions (equal, contained, containing, touching, disjoint, zero extent)."""
    anc = AR.anchor_boxes64(AR.anchor_map(16, 16, 6))
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(25):
        b = np.asarray([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(0.3, 6), rng.uniform(0.3, 6), rng.uniform(-4, 4)], np.float32).astype(np.float64)
        iou, _ = AR.iou_box_anchors64(b, anc)
        for q in rng.integers(0, anc.shape[0], 50):
            worst = max(worst, abs(iou[q] - AR.iou_brute64(b, anc[q])))
    assert worst < 1e-13, worst
    q = 16 * 8 * 6 + 8 * 6 + 2
    iou, cont = AR.iou_box_anchors64(anc[q], anc)
    assert abs(iou[q] - 1.0) < 1e-13 and not cont[q]                       # an anchor equal to a box
    small = np.asarray([anc[q, 0], anc[q, 1], 0.6, 0.6, 0.2])
    iou, cont = AR.iou_box_anchors64(small, anc)
    assert cont[q] and iou[q] == 0.36 / 8.0 and abs(AR.iou_brute64(small, anc[q]) - 0.045) < 1e-15
    same = np.nonzero(cont & (anc[:, 2] == 2.0))[0]
    assert same.size > 10 and np.all(iou[same] == iou[q])                  # the containment tie is exact
    far = np.asarray([40.0, 0.0, 2.0, 4.0, 0.3])
    assert not AR.iou_box_anchors64(far, anc)[0].any()
    assert not AR.iou_box_anchors64(np.asarray([0.0, 0.0, 0.0, 4.0, 0.3]), anc)[0].any()


def test_aligned_pi8_pi4_cars_land_on_the_three_label_kinds():
    """A 2.0 x 4.4 m car on an anchor's centre: aligned IoU 0.91, pi/8 off 0.66, pi/4 off 0.48 (the worst heading the three anchor yaws leave open).
    With thresholds 0.7 / 0.5 and no forced match the cell's yaw-0 anchor is positive, ignored, background; the forced match makes the last positive."""
    anchors = AR.anchor_map(24, 24, 3)
    ix = iy = 12
    a0 = _anchor5(anchors, ix, iy, 0)
    q = _flat(anchors, ix, iy, 0)
    want = {0.0: (0.9091, (0.0, 1.0)), PI / 8: (0.66, (0.0, 0.0)), PI / 4: (0.48, (1.0, 0.0))}
    for yaw, (iou, label) in want.items():
        box = np.asarray([[a0[0], a0[1], 2.0, 4.4, yaw]], np.float32)
        r = AR.assign_item_ref(box, 1, anchors, 0.7, 0.5, force_match=False)
        assert abs(r["iou"][0, q] - iou) < 6e-3, (yaw, r["iou"][0, q])
        assert abs(r["iou"][0, q] - AR.iou_brute64(box[0].astype(np.float64), a0)) < 1e-13
        assert tuple(r["labels"][q]) == label and r["mask"][q] == (label == (0.0, 1.0)) and r["assoc"][q] == (0 if label == (0.0, 1.0) else -1)
        assert not r["code"][~r["mask"]].any()
    box = np.asarray([[a0[0] + 0.01, a0[1] - 0.02, 2.0, 4.4, PI / 4 + 0.01]], np.float32)
    r = AR.assign_item_ref(box, 1, anchors, 0.7, 0.5, force_match=True)
    assert AR.n_undecided(r) == 0 and r["mask"].sum() == 1 and r["gt_best"][0] >= 0 and r["assoc"][r["gt_best"][0]] == 0
    assert r["gt_max_iou"][0] == r["iou"][0].max() < 0.5
    b = r["gt_best"][0]
    g, a = box[0].astype(np.float64), AR.anchor_boxes64(anchors)[b]
    d = g[4] - a[4]
    d = d - PI * math.floor((d + PI / 2) / PI)                              # folded to [-pi/2, pi/2)
    want_code = [g[0] - a[0], g[1] - a[1], math.log(g[2] / a[2]), math.log(g[3] / a[3]), math.sin(d), math.cos(d)]
    assert np.allclose(r["code"][b], want_code, rtol=0, atol=1e-14) and -PI / 2 <= d < PI / 2
    # the code inverts utils/postprocess.decode_boxes
    from v2x_sim_amd.utils.postprocess import decode_boxes
    dec = decode_boxes(r["code"][b][None], anchors.reshape(-1, 6)[b][None].astype(np.float64))[0]
    assert np.allclose(dec[:4], g[:4], atol=1e-12) and abs(math.remainder(dec[4] - g[4], PI)) < 1e-7


def test_duplicates_invalid_rows_and_competing_claims():
    anchors = AR.anchor_map(40, 40, 6)
    anc = AR.anchor_boxes64(anchors)
    car = [0.13, -0.21, 1.96, 4.4, 0.04]
    # duplicate boxes: the lower index takes every anchor and the forced match; the copy gets the same gt_best and no anchor
    r = AR.assign_item_ref(np.asarray([car, car, [np.nan, 0, 2, 4, 0], [0, 0, -2, 4, 0], [0, 0, 0, 4, 0], car], np.float32), 5, anchors)
    assert AR.n_undecided(r) == 0
    assert set(r["assoc"][r["mask"]].tolist()) == {0} and r["gt_best"][0] == r["gt_best"][1] >= 0 and r["gt_max_iou"][0] == r["gt_max_iou"][1]
    assert r["gt_best"][2:].tolist() == [-1] * 4 and not r["gt_max_iou"][2:].any()      # NaN, negative extent, zero width, beyond the count
    assert not r["iou"][2:].any()
    # brute force over every anchor for the car: argmax and the threshold sets
    brute = np.asarray([AR.iou_brute64(np.asarray(car, np.float32).astype(np.float64), anc[q]) if abs(anc[q, 0]) < 5 and abs(anc[q, 1]) < 5 else 0.0
                        for q in range(anc.shape[0])])
    assert np.abs(brute - r["iou"][0]).max() < 1e-13 and int(brute.argmax()) == r["gt_best"][0]
    assert np.array_equal(np.nonzero(brute >= np.float32(0.6))[0], np.nonzero(r["mask"])[0])
    assert np.array_equal(brute < np.float32(0.45), r["labels"][:, 0] == 1.0)
    # two boxes claim one anchor (the table's "claims" case, items 0 and 1): the larger IoU keeps it; one cell beside it the small box's claim overrides
    d = AR.make_case([c.name for c in AR.ASSIGN_CASES].index("claims"))
    r0, r1 = d["refs"][0], d["refs"][1]
    assert r0["gt_best"][0] == r0["gt_best"][1] and r0["gt_max_iou"][1] > r0["gt_max_iou"][0] and r0["assoc"][r0["gt_best"][0]] == 1
    assert not (r0["assoc"] == 0).any()
    q = r1["gt_best"][0]
    assert q != r1["gt_best"][1] and r1["assoc"][q] == 0 and r1["anchor_iou"][q] >= 0.6 and r1["iou"][1, q] == r1["anchor_iou"][q]
    assert (r1["assoc"] == 0).sum() == 1 and tuple(r1["labels"][q]) == (0.0, 1.0)
    assert np.allclose(r1["code"][q][:2], d["gt_boxes"][1, 0, :2].astype(np.float64) - AR.anchor_boxes64(d["anchors"])[q, :2], atol=1e-14)


def test_no_case_of_the_table_has_an_undecided_element():
    """The condition the GPU sweep rests on: it may exclude nothing.  Also: the table holds what it claims (every label kind, forced-only boxes,
    dropped rows, counts beyond gt_cap)."""
    kinds = set()
    for i, case in enumerate(AR.ASSIGN_CASES):
        d = AR.make_case(i)
        assert d["draws"] <= 20
        for m, r in enumerate(d["refs"]):
            assert AR.n_undecided(r) == 0, (case.name, m, {k: v.size for k, v in r["undecided"].items()})
            lab = r["labels"]
            kinds |= {tuple(v) for v in np.unique(lab, axis=0).tolist()}
            assert np.array_equal(r["mask"], lab[:, 1] == 1.0) and np.array_equal(r["mask"], r["assoc"] >= 0)
            if case.neg_thr == case.pos_thr:
                assert np.all(lab.sum(1) == 1.0)                           # no ignored rows
            if not case.force:
                assert np.all(r["anchor_iou"][r["mask"]] >= np.float32(case.pos_thr))
    assert kinds == {(0.0, 0.0), (0.0, 1.0), (1.0, 0.0)}
    edges = AR.make_case([c.name for c in AR.ASSIGN_CASES].index("ragged_edges"))
    r = edges["refs"][0]
    assert r["gt_best"][:4].tolist() == [-1] * 4 and r["gt_best"][4] >= 0 and 0 < r["gt_max_iou"][5] < 0.1      # zero_w, nan, neg, far | edge | small
    assert (r["assoc"] == 5).sum() == 1 and r["gt_best"][6] == r["gt_best"][7]
    assert max(c for case in AR.ASSIGN_CASES for c, _ in case.items) > AR.MAX_GT


def test_sparse_keys_round_trip_through_the_dataset_loader(tmp_path):
    """ops.assign_targets_sparse_keys on a dense result -> a 0.npy with upstream's sparse training keys -> datasets.V2XSimDet(targets=True), unchanged
    loader: positives, codes, regression mask and gt_max_iou come back; the format has no ignore state, an ignored anchor reads back as background."""
    from v2x_sim_amd import ops
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.datasets import V2XSimDet
    from v2x_sim_amd.datasets.V2XSimDet import UPSTREAM_TARGET_KEYS
    d = AR.make_case([c.name for c in AR.ASSIGN_CASES].index("full_grid"))
    r, case = d["refs"][0], d["case"]
    cfg = Config("train")
    shape = (case.X, case.Y, case.A)
    assert list(shape[:2]) == cfg.map_dims[:2] and np.array_equal(d["anchors"], __import__("v2x_sim_amd.utils.postprocess", fromlist=["x"]).build_anchor_map(cfg))
    res = {"labels": torch.from_numpy(r["labels"].astype(np.float32).reshape((1,) + shape + (2,))),
           "reg_targets": torch.from_numpy(r["code"].astype(np.float32).reshape((1,) + shape + (1, 6))),
           "reg_loss_mask": torch.from_numpy(r["mask"].astype(np.uint8).reshape((1,) + shape + (1,))),
           "gt_max_iou": torch.from_numpy(r["gt_max_iou"].astype(np.float32)[None])}
    keys = ops.assign_targets_sparse_keys(res, 0)
    assert set(keys) == set(UPSTREAM_TARGET_KEYS) | {"gt_max_iou"}
    sample = dict(keys, voxel_indices_0=np.zeros((1, 3), np.int32), trans_matrices=np.eye(4, dtype=np.float32)[None], num_sensor=1, target_agent_id=0,
                  gt_boxes=d["gt_boxes"][0])
    path = os.path.join(str(tmp_path), "train", "agent0", "1_0")
    os.makedirs(path)
    np.save(os.path.join(path, "0.npy"), sample, allow_pickle=True)
    t = V2XSimDet(dataset_roots=[os.path.join(str(tmp_path), "train", "agent0")], config=cfg, split="train", densify="none", targets=True)[0][0]
    label, reg, mask = t[2], t[3], t[4]
    want = res["labels"][0].numpy().copy()
    ignored = want.sum(-1) == 0
    assert ignored.sum() > 0 and r["mask"].sum() > 0
    want[ignored] = (1.0, 0.0)
    assert np.array_equal(label, want) and np.array_equal(reg, res["reg_targets"][0].numpy()) and np.array_equal(mask[..., 0], r["mask"].reshape(shape))
    assert np.array_equal(t[7], res["gt_max_iou"][0].numpy())


def test_header_ctypes_rows_and_argument_errors():
    """The two C entries are declared, bound and refuse bad arguments before any HIP call; n_items == 0 returns at once."""
    import ctypes as C
    from v2x_sim_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "v2x_amd.h")).read(), flags=re.S)
    assert re.search(r"long long\s+v2x_det_assign_workspace_size\s*\(", src) and re.search(r"int\s+v2x_det_assign_targets\s*\(", src)
    assert _lib.SIGNATURES["v2x_det_assign_workspace_size"][0] is C.c_longlong and len(_lib.SIGNATURES["v2x_det_assign_targets"][1]) == 21
    lib = _lib.load()
    assert lib.v2x_abi_version() == 18
    assert lib.v2x_det_assign_workspace_size(10, 256, 256, 6, 8) == 10 * 8 * 256 * 16
    assert lib.v2x_det_assign_workspace_size(3, 17, 19, 3, 256) == 3 * 256 * 4 * 16
    assert lib.v2x_det_assign_workspace_size(1, 16, 16, 6, 257) == -1 and lib.v2x_det_assign_workspace_size(1, 16, 16, 6, 0) == -1
    assert lib.v2x_det_assign_workspace_size(1, 65536, 65536, 6, 8) == -1 and lib.v2x_det_assign_workspace_size(0, 16, 16, 6, 8) == 0

    def call(n=1, gt_cap=8, pos=0.6, neg=0.45, X=16, Y=16, A=6):
        return lib.v2x_det_assign_targets(None, None, n, gt_cap, None, X, Y, A, C.c_float(pos), C.c_float(neg), 1, None, None, None, None, None, None, None,
                                          None, 0, None)
    assert call(n=0) == 0 and call(n=0, gt_cap=0, pos=7.0) == 0            # nothing to do: before every other check
    for kw, text in (({"gt_cap": 0}, b"gt_cap"), ({"gt_cap": 257}, b"gt_cap"), ({"neg": 0.0}, b"thresholds"), ({"neg": 0.7}, b"thresholds"),
                     ({"pos": 1.5}, b"thresholds"), ({"pos": float("nan")}, b"thresholds"), ({"X": 0}, b"sizes"), ({"n": -1}, b"n_items"), ({}, b"null")):
        assert call(**kw) == -22 and text in lib.v2x_last_error(), (kw, lib.v2x_last_error())


def test_driver_takes_the_targets_switch():
    spec = importlib.util.spec_from_file_location("train_codet_cli", os.path.join(ROOT, "tools", "det", "train_codet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ap = mod.build_parser()
    assert ap.parse_args([]).targets == "radius" and ap.parse_args(["--targets", "iou"]).targets == "iou"
    with pytest.raises(SystemExit):
        ap.parse_args(["--targets", "nearest"])
    import inspect
    from v2x_sim_amd.train import loop
    for fn in (loop.synthetic_batch_on_device, loop.dataset_batch_on_device, loop.train_synthetic, loop.train_dataset):
        assert inspect.signature(fn).parameters["targets"].default == "radius"

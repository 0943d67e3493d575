"""CPU tests of the box rasterizer's float64 reference (tests/seg_raster_refs.py) and of the feature's host-side plumbing: the reference against
utils/synthetic_scene.seg_labels, the exclusion condition of the committed case table, hand-made cases of the rule, the C entries' prototypes and
argument errors, the boxes samples of the seg dataset, the driver's switches and the median-frequency weights."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import seg_raster_refs as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_equals_seg_labels_on_synthetic_scenes():
    """Class 1 on Config's 256 x 256 grid: the reference and the host loop it restates give the same map, bit for bit, for every agent of two scenes."""
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.utils import synthetic_scene
    cfg = Config("train", binary=True, only_det=True)
    grid = SR.config_grid(cfg)
    assert grid == (-32.0, -32.0, 0.25, 0.25, 256, 256)
    painted = 0
    for seed in (0, 7):
        scene = synthetic_scene.make_scene(agents=3, seed=seed, ground_pts=10, clutter_pts=10, pts_per_car=4)
        for g in scene["gt_boxes"]:
            ref = SR.raster_item_ref(g, np.ones((g.shape[0],), np.uint8), g.shape[0], grid, 8)
            want = synthetic_scene.seg_labels(g, cfg)
            assert np.array_equal(ref["labels"], want)
            assert np.array_equal(ref["owner"] >= 0, want == 1) and ref["hist"][1] == int(want.sum()) and ref["hist"][2:].sum() == 0
            painted += int(want.sum())
    assert painted > 1000


@pytest.mark.parametrize("index", range(len(SR.RASTER_CASES)), ids=SR.NAMES)
def test_case_table_keeps_the_exclusion_cap(index):
    """A condition on the table, not a measurement: at most 0.01 % of a case's cells lie within 1e-9 m of a box border; an exact case excludes
    nothing, holds real ties (margin 0) and nothing between 0 and the margin (its arithmetic is exact)."""
    d = SR.make_case(index)
    case = d["case"]
    out = SR.excluded_mask(d)
    assert int(out.sum()) <= SR.max_excluded_cells(d)
    assert d["boxes"].shape[0] <= 6 and case.X in (16, 17, 40, 48) and case.Y in (16, 17, 40, 48) and case.cell in (0.25, 1.6)
    assert 1 <= case.cap <= SR.MAX_BOXES and 2 <= case.n_cls <= 32
    if case.exact:
        margin = np.stack([r["margin"] for r in d["refs"]])
        assert not out.any() and (margin == 0).sum() >= 20 and not ((margin > 0) & (margin < SR.RASTER_MARGIN)).any()
        assert np.all(d["boxes"][..., 4] == 0)


def test_table_covers_the_edges_the_rule_names():
    by = {c.name: SR.make_case(i) for i, c in enumerate(SR.RASTER_CASES)}
    d = by["counts_0_over_full_cap256"]
    assert d["count"].tolist() == [0, 259, 256] and d["boxes"].shape[1] == 256 and (d["refs"][0]["labels"] == 0).all() and (d["refs"][0]["owner"] == -1).all()
    assert by["count_over_small_cap"]["count"].tolist() == [7, 0, 4, -3] and (by["count_over_small_cap"]["refs"][3]["labels"] == 0).all()
    big = by["big_and_outside"]["refs"]
    assert (big[0]["labels"] == 3).all() and (big[1]["labels"] == 0).all() and set(np.unique(big[2]["labels"])) == {3, 5}
    st = by["corner_straddle"]["refs"][0]["owner"]
    assert all((st[a, b] == 0).any() for a in (slice(0, 16), slice(16, 32)) for b in (slice(0, 16), slice(16, 32)))       # all four tiles round the corner
    # overlaps: the greater class id wins under the NULL rank in either index order; under the permuted rank class 1 (rank 6) beats 7 (rank 0) and 3 (rank 1)
    nul, per = by["overlaps_null_rank"]["refs"], by["overlaps_permuted_rank"]["refs"]
    assert np.array_equal(nul[0]["labels"], nul[1]["labels"]) and not np.array_equal(nul[0]["owner"], nul[1]["owner"])
    assert nul[0]["hist"][7] > per[0]["hist"][7] > 0 and per[0]["hist"][1] > nul[0]["hist"][1] > 0
    # same class three times: a cell belongs to the FIRST box that covers it -- where box 0 owns the cell among different classes too, it still does
    assert set(np.unique(nul[2]["owner"])) == {-1, 0, 1, 2} and (nul[2]["owner"][nul[0]["owner"] == 0] == 0).all()
    assert ((nul[2]["owner"] == 0) & (nul[0]["owner"] == 1)).any()                         # ... and it keeps cells the higher class took from it there
    assert 1 not in np.unique(nul[3]["owner"]) and set(np.unique(nul[3]["labels"])) == {0, 1, 7}          # the class-0 box painted nothing, hid nothing
    assert nul[4]["hist"][8] > 0 and (nul[4]["owner"][nul[4]["labels"] == 255] == 0).all()
    assert nul[5]["hist"][8] > 0 and (nul[5]["owner"][nul[5]["labels"] == 255] == 2).all() and 3 not in np.unique(nul[5]["owner"])
    dr = by["dropped_between_valid"]["refs"]
    assert set(np.unique(dr[0]["owner"])) == {-1, 1, 4, 8} and 255 not in dr[0]["labels"] and (dr[1]["labels"] == 0).all() and np.isinf(dr[1]["margin"]).all()
    t0, t1 = by["ties_yaw0"]["refs"]
    assert (t0["owner"] == 0).sum() == 7 * 5 and (t0["owner"] == 1).sum() == 11 * 3 - 3 and (t0["owner"] == 2).sum() == 3        # closed borders
    assert (t0["owner"] == 3).sum() == 1 and (t0["owner"] == 4).sum() == 0 and t0["labels"][36, 30] == 255
    assert (t1["owner"] == 1).sum() == 6 * 4 and (t1["owner"] == 0).sum() == 0 and (t1["owner"] == 2).sum() == 2 * 2 and t1["owner"][39, 0] == 2


def test_header_ctypes_rows_and_argument_errors():
    """The two C entries are declared, bound and refuse bad arguments before any HIP call; n == 0 returns at once, before every other check."""
    from v2x_sim_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "v2x_amd.h")).read(), flags=re.S)
    m = re.search(r"int\s+v2x_seg_rasterize\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m and re.search(r"long long\s+v2x_seg_rasterize_workspace_size\s*\(", src)
    params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
    res, args = _lib.SIGNATURES["v2x_seg_rasterize"]
    assert res is C.c_int and len(args) == len(params) == 19
    for p, a in zip(params, args):
        want = C.c_void_p if ("*" in p or p.startswith("v2x_stream_t")) else C.c_float if p.startswith("float") else C.c_longlong if p.startswith("long long") else C.c_int
        assert a is want, (p, a)
    assert _lib.SIGNATURES["v2x_seg_rasterize_workspace_size"] == (C.c_longlong, [C.c_longlong, C.c_int, C.c_int, C.c_int])
    lib = _lib.load()
    assert lib.v2x_abi_version() == 18                                                   # additive: the version stays
    assert lib.v2x_seg_rasterize_workspace_size(10, 256, 256, 8) == 10 * 256 * 9 * 4
    assert lib.v2x_seg_rasterize_workspace_size(3, 17, 40, 32) == 3 * 6 * 33 * 4 and lib.v2x_seg_rasterize_workspace_size(0, 16, 16, 8) == 0
    assert lib.v2x_seg_rasterize_workspace_size(1, 16, 16, 1) == -1 and lib.v2x_seg_rasterize_workspace_size(1, 16, 16, 33) == -1
    assert lib.v2x_seg_rasterize_workspace_size(1, 0, 16, 8) == -1 and lib.v2x_seg_rasterize_workspace_size(2 ** 31, 16, 16, 8) == -1

    def call(n=1, cap=8, vx=0.25, vy=0.25, X=16, Y=16, n_cls=8, x0=-2.0):
        return lib.v2x_seg_rasterize(None, None, None, n, cap, C.c_float(x0), C.c_float(-2.0), C.c_float(vx), C.c_float(vy), X, Y, n_cls, None, None, None,
                                     None, None, 0, None)
    assert call(n=0) == 0 and call(n=0, cap=0, n_cls=99, vx=-1.0, X=0) == 0               # nothing to do: before every range and pointer check
    for kw, text in (({"cap": 0}, b"cap"), ({"cap": 257}, b"cap"), ({"n_cls": 1}, b"n_cls"), ({"n_cls": 33}, b"n_cls"), ({"vx": 0.0}, b"cell sizes"),
                     ({"vy": -0.25}, b"cell sizes"), ({"vx": float("nan")}, b"cell sizes"), ({"vy": float("inf")}, b"cell sizes"),
                     ({"x0": float("nan")}, b"finite"), ({"X": 0}, b"sizes"), ({"n": 2 ** 31, "X": 17}, b"2^31"), ({"n": 2 ** 23, "X": 256, "Y": 256}, b"2^31"),
                     ({"n": -1}, b"negative n"), ({}, b"null")):
        assert call(**kw) == -22 and text in lib.v2x_last_error(), (kw, lib.v2x_last_error())


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_coverage_arithmetic_is_not_contracted(tmp_path):
    """The rule rounds every product and sum of the cull, the cell centres and the coverage test on its own; a fused multiply-add there would move a
    decision by less than the tests' margin, so the ISA is read instead: raster_tile_kernel has three barriers, and the only fp64 FMAs of the kernel
    sit between the first two, where the survivors' cos / sin are computed (libm's polynomials)."""
    import subprocess
    out = os.path.join(str(tmp_path), "seg_raster.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only",
                           os.path.join(ROOT, "v2x-sim_amd", "csrc", "seg_raster.hip"), "-o", out], stderr=subprocess.DEVNULL)
    m = re.search(r"^_Z18raster_tile_kernel\w*:.*?s_endpgm", open(out).read(), flags=re.S | re.M)
    assert m
    lines = [ln.strip() for ln in m.group(0).splitlines() if ln.strip() and not ln.strip().startswith(";")]
    bars = [i for i, ln in enumerate(lines) if ln.startswith("s_barrier")]
    assert len(bars) == 3, bars
    count = lambda seg, op: sum(ln.startswith(op) for ln in seg)
    cull, trig, cells = lines[:bars[0]], lines[bars[0]:bars[1]], lines[bars[1]:bars[2]]
    assert count(cull, "v_fma_f64") == 0 and count(cull, "v_mul_f64") >= 8            # four cell centres, the squared distance and radius
    assert count(trig, "v_fma_f64") > 0
    assert count(cells, "v_fma_f64") == 0 and count(cells, "v_mul_f64") >= 6 and count(cells, "v_cmp_le_f64") >= 2
    assert "scratch_" not in m.group(0)


def test_wrapper_refuses_host_tensors_and_bad_shapes():
    from v2x_sim_amd import ops
    grid = SR.grid_of(16, 16, 0.25)
    boxes, cls, count = torch.zeros((1, 4, 5)), torch.zeros((1, 4), dtype=torch.uint8), torch.zeros((1,), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rasterize_seg(boxes, cls, count, grid)
    with pytest.raises(ValueError, match="rasterize_seg"):
        ops.rasterize_seg(boxes, cls[:, :3], count, grid)
    with pytest.raises(ValueError, match="unknown output"):
        ops.rasterize_seg(boxes, cls, count, grid, want=("margin",))
    with pytest.raises(ValueError, match="rank"):
        ops.rasterize_seg(boxes, cls, count, grid, rank=torch.zeros((7,), dtype=torch.uint8))
    assert ops.seg_grid(ops.VoxelGrid()) == (-32.0, -32.0, 0.25, 0.25, 256, 256)
    b, c, k = ops.pad_box_lists([np.zeros((0, 5)), np.ones((3, 5)), np.ones((1, 5))])
    assert b.shape == (3, 3, 5) and b.dtype == np.float32 and c.tolist() == [[0, 0, 0], [1, 1, 1], [1, 0, 0]] and k.tolist() == [0, 3, 1]
    b, c, k = ops.pad_box_lists([np.ones((2, 5))], [[4, 200]])
    assert c.dtype == np.uint8 and c.tolist() == [[4, 200]]
    with pytest.raises(ValueError):
        ops.pad_box_lists([np.ones((2, 5))], [[4]])
    with pytest.raises(ValueError, match="256"):
        ops.pad_box_lists([np.ones((257, 5))])


def _write_frame(root, split, frame, kinds, rng):
    """One frame of two agents; kinds[a] in {"map", "boxes", "neither"}."""
    from v2x_sim_amd.datasets import write_sample, write_seg_sample
    out = []
    for a, kind in enumerate(kinds):
        idx = rng.integers(0, (256, 256, 13), (50, 3)).astype(np.int32)
        T = np.stack([np.eye(4, dtype=np.float32)] * 2)
        boxes = np.concatenate([rng.uniform(-20, 20, (4, 2)), rng.uniform(1, 5, (4, 2)), rng.uniform(-3, 3, (4, 1))], 1)
        classes = np.asarray([1, 2, 7, 200])
        if kind == "map":
            write_seg_sample(root, split, a, 3, frame, idx, T, 2, rng.integers(0, 8, (256, 256)))
        elif kind == "boxes":
            write_seg_sample(root, split, a, 3, frame, idx, T, 2, None, gt_boxes=boxes, gt_classes=classes)
        else:
            write_sample(root, split, a, 3, frame, idx, T, 2, gt_boxes=boxes)
        out.append((boxes, classes))
    return out


def test_boxes_samples_round_trip_and_the_refusals(tmp_path):
    """write_seg_sample(gt_boxes=, gt_classes=) -> V2XSimSeg: the pair comes back in the label slot as fp32 (G, 5) and uint8 (G,); a sample with neither
    kind still raises the KeyError that names bev_seg; a batch that mixes the kinds is refused before any device work (this machine has no device)."""
    from v2x_sim_amd import ops
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.datasets import V2XSimSeg, seg_batch_on_device, write_seg_sample
    rng = np.random.default_rng(2)
    root = str(tmp_path)
    wrote = _write_frame(root, "train", 0, ("boxes", "boxes"), rng)
    _write_frame(root, "train", 1, ("map", "map"), rng)
    _write_frame(root, "val", 0, ("boxes", "map"), rng)
    _write_frame(root, "test", 0, ("neither", "boxes"), rng)
    cfg = Config("train")
    roots = lambda split: [os.path.join(root, split, "agent%d" % a) for a in range(2)]
    ds = V2XSimSeg(dataset_roots=roots("train"), config=cfg, split="train", densify="none")
    assert len(ds) == 2
    for a, t in enumerate(ds[0]):
        boxes, classes = t[1]
        assert boxes.dtype == np.float32 and classes.dtype == np.uint8
        assert np.array_equal(boxes, wrote[a][0].astype(np.float32)) and np.array_equal(classes, wrote[a][1].astype(np.uint8))
        stored = np.load(os.path.join(t[2], "0.npy"), allow_pickle=True).item()
        assert "bev_seg" not in stored and stored["gt_boxes"].dtype == np.float32 and stored["gt_classes"].dtype == np.uint8
    assert isinstance(ds[1][0][1], np.ndarray) and ds[1][0][1].shape == (256, 256)
    with pytest.raises(KeyError, match="bev_seg"):
        V2XSimSeg(dataset_roots=roots("test"), config=cfg, split="test", densify="none")[0]
    grid = ops.VoxelGrid(cfg.voxel_size, cfg.area_extents)
    mixed = V2XSimSeg(dataset_roots=roots("val"), config=cfg, split="val", densify="none")[0]
    with pytest.raises(ValueError, match="mixes"):
        seg_batch_on_device([mixed], grid, torch.device("cuda:0"))
    with pytest.raises(ValueError, match="mixes"):
        seg_batch_on_device([ds[0], ds[1]], grid, torch.device("cuda:0"))
    T = np.stack([np.eye(4, dtype=np.float32)] * 2)
    with pytest.raises(ValueError):
        write_seg_sample(root, "val", 0, 1, 1, np.zeros((1, 3), np.int32), T, 1, None)
    with pytest.raises(ValueError):
        write_seg_sample(root, "val", 0, 1, 1, np.zeros((1, 3), np.int32), T, 1, None, gt_boxes=np.zeros((2, 5)), gt_classes=[1])
    with pytest.raises(ValueError):
        write_seg_sample(root, "val", 0, 1, 1, np.zeros((1, 3), np.int32), T, 1, None, gt_boxes=np.zeros((1, 5)), gt_classes=[300])


def _driver():
    spec = importlib.util.spec_from_file_location("train_seg_cli", os.path.join(ROOT, "tools", "seg", "train_seg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_driver_takes_the_targets_and_class_weight_switches():
    ap = _driver().build_parser()
    a = ap.parse_args([])
    assert a.targets == "map" and a.class_weight == ""
    assert ap.parse_args(["--targets", "boxes"]).targets == "boxes" and ap.parse_args(["--class_weight", "balanced"]).class_weight == "balanced"
    assert ap.parse_args(["--class_weight", "1,2,0.5,1,1,1,1,1"]).class_weight == "1,2,0.5,1,1,1,1,1"       # the comma list keeps working
    for bad in (["--targets", "polygons"], ["--class_weight", "heavy"], ["--class_weight", "1,two"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    import inspect
    from v2x_sim_amd.train import loop
    sig = inspect.signature(loop.seg_targets_on_device)
    assert list(sig.parameters)[:4] == ["box_lists", "class_lists", "config", "device"]


def test_median_frequency_weights_on_a_hand_made_histogram():
    """f = (0.5, 0.25, 0, 0.125, 0.125): median over the four classes that occur = 0.1875 -> w = (0.375, 0.75, 0, 1.5, 1.5); the ignore column and
    the leading axes do not count."""
    from v2x_sim_amd import ops
    w = ops.median_frequency_weights(np.asarray([[300, 100, 0, 50, 100, 999], [100, 100, 0, 50, 0, 1]]), 5)
    assert w == [0.375, 0.75, 0.0, 1.5, 1.5]
    assert ops.median_frequency_weights([8, 0, 0], 2) == [1.0, 0.0] and ops.median_frequency_weights([0, 0, 5], 2) == [0.0, 0.0]
    assert ops.median_frequency_weights([64, 32, 16, 16], 4) == [0.375, 0.75, 1.5, 1.5]

"""Late fusion on the MI355X: v2x_det_late_fuse (csrc/late_fuse.hip) against the float64 reference and the case table of tests/late_refs.py -- kept
set, order and sources equal, boxes bit-equal to the numpy-float32 evaluation of the transform, scores bit-equal to the inputs --, its identities,
edges and hostile inputs, the scene property (late-fused ground truth = the cars in range of any agent), FaFModule.late_fusion and the driver."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import late_refs as LR
from v2x_sim_amd.utils import postprocess as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(device, boxes, scores, counts, rigid, link, extents, nms_thr, rotated, cap_out):
    from v2x_sim_amd import ops
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    ob, osc, osrc, ocnt = ops.late_fuse(t(boxes), t(scores), t(counts.astype(np.int32)), t(rigid), t(link.astype(np.uint8)), extents, nms_thr=nms_thr,
                                        rotated=rotated, cap_out=cap_out)
    torch.cuda.synchronize()
    return ob.cpu().numpy(), osc.cpu().numpy(), osrc.cpu().numpy(), ocnt.cpu().numpy()


def _assert_ego(got, row, ref, what):
    ob, osc, osrc, ocnt = got
    assert ocnt[row] == ref["count"], (what, int(ocnt[row]), ref["count"])
    n = ref["count"]
    if n > 0:
        assert osrc[row, :n].tolist() == ref["src"].tolist(), what
        assert np.array_equal(ob[row, :n].view(np.uint32), ref["boxes"].view(np.uint32)), what
        assert np.array_equal(osc[row, :n].view(np.uint32), ref["score_bits"]), what


@pytest.mark.parametrize("index", range(len(LR.LATE_CASES)), ids=[c.name for c in LR.LATE_CASES])
def test_sweep_against_reference(device, index):
    """Every case of the table (stand-up and rotated suppression, the bit-matrix and the serial form, 511 / 512 / 513 and cap_out / cap_out + 1
    merged candidates, only_v2i / asymmetric / absent links, negative and oversized source counts): count, order, sources, box and score bits."""
    d = LR.make_late_case(index)
    c = d["case"]
    got = _run(device, d["boxes"], d["scores"], d["counts"], d["rigid"], d["link"], c.extents, c.nms_thr, c.rotated, c.cap_out)
    for i in range(c.A):
        for b in range(c.B):
            _assert_ego(got, i * c.B + b, d["refs"][i][b], (c.name, i, b))


def _stable_list(rng, n, cap_in):
    """n boxes no NMS removes (10 m apart), descending distinct scores; the rows past n hold a box that would be kept."""
    boxes = np.zeros((cap_in, 5), np.float32)
    boxes[:, 0] = 1.0e3
    boxes[:, 2:4] = 2.0
    scores = np.full(cap_in, 0.999, np.float32)
    k = np.arange(n)
    boxes[:n] = np.stack([(k % 16) * 10.0 - 75.0 + rng.uniform(-1, 1, n), (k // 16) * 10.0 - 75.0 + rng.uniform(-1, 1, n), rng.uniform(1.5, 4.5, n),
                          rng.uniform(1.5, 4.5, n), rng.uniform(-math.pi, math.pi, n)], 1).astype(np.float32)
    scores[:n] = (0.99 - 1e-4 * k).astype(np.float32)
    return boxes, scores


@pytest.mark.parametrize("A,links_off", [(1, False), (5, True)])
@pytest.mark.parametrize("cap_in,cap_out,rotated", [(64, 64, False), (256, 1024, True)])
def test_identity(device, A, links_off, cap_in, cap_out, rotated):
    """One agent, and five with every link off: the output is the input, bit for bit, for 0, 1, 63, 64 and cap_in detections -- inside AND outside
    the crop (the ego's own boxes are never cropped), the other agents' lists untouched."""
    rng = np.random.default_rng(5)
    ns = sorted({0, 1, 63, 64, cap_in})
    B = len(ns)
    boxes = np.zeros((A * B, cap_in, 5), np.float32)
    scores = np.zeros((A * B, cap_in), np.float32)
    counts = np.zeros(A * B, np.int32)
    for j in range(A):
        for b in range(B):
            n = ns[(b + j) % B]
            boxes[j * B + b], scores[j * B + b] = _stable_list(rng, n, cap_in)
            counts[j * B + b] = n
    rigid = LR.rigid_ref(np.stack([LR.trans_from_poses([LR.pose(rng.uniform(-3, 3), *rng.uniform(-5, 5, 2)) for _ in range(A)])[0] for _ in range(B)]))
    link = np.tile(np.eye(A, dtype=np.uint8), (B, 1, 1)) if links_off else np.ones((B, A, A), np.uint8)
    ob, osc, osrc, ocnt = _run(device, boxes, scores, counts, rigid, link, LR.AREA, 0.01, rotated, cap_out)
    assert ocnt.tolist() == counts.tolist()
    for j in range(A):
        for b in range(B):
            r, n = j * B + b, counts[j * B + b]
            assert np.array_equal(ob[r, :n].view(np.uint32), boxes[r, :n].view(np.uint32))
            assert np.array_equal(osc[r, :n].view(np.uint32), scores[r, :n].view(np.uint32))
            assert osrc[r, :n].tolist() == (j * cap_in + np.arange(n)).tolist()


def _coincident(A, cap_in, with_ego, yaw=0.4):
    """Agents 0 (the ego), 2 and 3 of five all report ONE box at the same place of the ego's frame with the same score bits; poses = pure
    translations by whole metres, so that the transform is exact."""
    poses = [LR.pose(0.0, 4.0 * j, -3.0 * j) for j in range(A)]
    trans, _ = LR.trans_from_poses(poses)
    boxes = np.zeros((A, cap_in, 5), np.float32)
    scores = np.zeros((A, cap_in), np.float32)
    counts = np.zeros(A, np.int32)
    for j in ((0, 2, 3) if with_ego else (2, 3)):
        boxes[j, 0] = [10.0 - 4.0 * j, 6.0 + 3.0 * j, 2.0, 4.5, yaw]
        scores[j, 0] = 0.8125
        counts[j] = 1
    # a better box elsewhere from agent 3, a worse one elsewhere from agent 1: the tie is neither first nor last
    boxes[3, 0], boxes[3, 1] = [-20.0 - 12.0, 0.0 + 9.0, 2.0, 4.0, 0.0], boxes[3, 0].copy()
    scores[3, 0], scores[3, 1] = 0.9, scores[3, 0]
    counts[3] = 2
    boxes[1, 0], scores[1, 0], counts[1] = [20.0 - 4.0, 20.0 + 3.0, 2.0, 4.0, 1.0], 0.5, 1
    return boxes, scores, counts, LR.rigid_ref(trans[None]), np.ones((1, A, A), np.uint8)


@pytest.mark.parametrize("rotated", [False, True])
def test_ties(device, rotated):
    """Bit-equal scores on coincident boxes from the ego and two neighbours: the ego's box survives; without the ego's, the lower agent's."""
    cap = 64
    for with_ego, want in ((True, [3 * cap + 0, 0 * cap + 0, 1 * cap + 0]), (False, [3 * cap + 0, 2 * cap + 0, 1 * cap + 0])):
        boxes, scores, counts, rigid, link = _coincident(5, cap, with_ego)
        ob, osc, osrc, ocnt = _run(device, boxes, scores, counts, rigid, link, LR.AREA, 0.01, rotated, 64)
        assert ocnt[0] == 3 and osrc[0, :3].tolist() == want, (with_ego, ocnt[0], osrc[0, :4])
        ref = LR.ego_reference(boxes, scores, counts, rigid, link, 5, 1, cap, 64, LR.AREA, 0.01, rotated, 0, 0)
        assert ref["src"].tolist() == want
        assert np.array_equal(ob[0, 1], np.array([10.0, 6.0, 2.0, 4.5, 0.4], np.float32)) and osc[0, 1] == np.float32(0.8125)


def test_crop_edges(device):
    """Neighbour centres exactly at x_lo (kept), at nextafter(x_hi, -inf) (kept) and at x_hi (dropped), the same in y; the ego's own box AT x_hi
    stays.  The neighbour's frame is the ego's shifted by whole metres: the transformed centre is exact."""
    cap, A = 64, 2
    x_lo, x_hi, y_lo, y_hi = -32.0, 32.0, -24.0, 24.0
    f = np.float32
    below = lambda v: float(np.nextafter(f(v), f(-np.inf)))
    trans, _ = LR.trans_from_poses([LR.pose(0.0, 0.0, 0.0), LR.pose(0.0, 8.0, -8.0)])
    cx = [(x_lo, 0.0, True), (below(x_lo), 4.0, False), (below(x_hi), 8.0, True), (x_hi, 12.0, False),
          (0.0, y_lo, True), (4.0, below(y_lo), False), (8.0, below(y_hi), True), (12.0, y_hi, False), (x_lo, y_lo, True), (x_hi, y_hi, False)]
    boxes = np.zeros((A, cap, 5), np.float32)
    scores = np.zeros((A, cap), np.float32)
    for k, (x, y, _) in enumerate(cx):
        # subtracting the offset must be exact too: the edges and their neighbours are, 8 being a multiple of their spacing's power of two
        boxes[1, k] = [f(x) - f(8.0), f(y) + f(8.0), 0.5, 0.5, 0.0]
        assert f(boxes[1, k, 0] + f(8.0)) == f(x) and f(boxes[1, k, 1] - f(8.0)) == f(y)
        scores[1, k] = 0.9 - 0.01 * k
    boxes[0, 0], scores[0, 0] = [x_hi, y_hi, 0.5, 0.5, 0.0], 0.95
    boxes[0, 1], scores[0, 1] = [100.0, -100.0, 0.5, 0.5, 0.0], 0.94
    counts = np.array([2, len(cx)], np.int32)
    got = _run(device, boxes, scores, counts, LR.rigid_ref(trans[None]), np.ones((1, A, A), np.uint8), ((x_lo, x_hi), (y_lo, y_hi)), 0.01, False, 64)
    want = [0, 1] + [cap + k for k, (_, _, keep) in enumerate(cx) if keep]
    assert got[3][0] == len(want) and got[2][0, :len(want)].tolist() == want
    kept = [k for k, (_, _, keep) in enumerate(cx) if keep]
    assert np.array_equal(got[0][0, 2:len(want), 0], np.array([cx[k][0] for k in kept], np.float32))
    assert np.array_equal(got[0][0, 2:len(want), 1], np.array([cx[k][1] for k in kept], np.float32))
    ref = LR.ego_reference(boxes, scores, counts, LR.rigid_ref(trans[None]), np.ones((1, A, A), np.uint8), A, 1, cap, 64, ((x_lo, x_hi), (y_lo, y_hi)), 0.01, False, 0, 0)
    _assert_ego(got, 0, ref, "crop")


def test_hostile_input(device):
    """NaN / inf fields, negative and NaN scores, counts beyond cap_in and A*B = 0: no fault, and the documented answer -- such candidates are
    dropped, wherever they sit, and drop nothing else."""
    from v2x_sim_amd import ops
    d = LR.make_late_case(0)
    c = d["case"]
    boxes, scores, counts = d["boxes"].copy(), d["scores"].copy(), d["counts"].copy()
    boxes[0, 0, 0] = np.nan          # the ego's best box
    boxes[0, 3, 4] = np.inf
    boxes[1, 1, 2] = -np.inf
    boxes[1, 2, 1] = np.nan
    scores[1, 4] = np.nan
    scores[0, 5] = -0.25
    scores[1, 6] = np.inf
    rigid = d["rigid"].copy()
    got = _run(device, boxes, scores, counts, rigid, d["link"], c.extents, c.nms_thr, False, c.cap_out)
    for i in range(2):
        ref = LR.ego_reference(boxes, scores, counts, rigid, d["link"], 2, 1, c.cap_in, c.cap_out, c.extents, c.nms_thr, False, i, 0)
        assert ref["count"] > 0 and ref["n_cand"] < d["refs"][i][0]["n_cand"]
        _assert_ego(got, i, ref, ("hostile", i))
    # a transform that is not finite drops that neighbour's boxes, nothing else
    rigid[0, 0, 1, 2] = np.nan
    got = _run(device, d["boxes"], d["scores"], d["counts"], rigid, d["link"], c.extents, c.nms_thr, False, c.cap_out)
    assert got[3][0] == counts[0] and (got[2][0, :counts[0]] < c.cap_in).all()
    # counts beyond cap_in: LATE_CASES "a5-hostile-counts" (the sweep).  A*B = 0: nothing is touched, nothing is launched
    e = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=device)
    for A, B in ((0, 3), (5, 0)):
        out = ops.late_fuse(e(A * B, 64, 5), e(A * B, 64), e(A * B, dt=torch.int32), e(B, A, A, 8), e(B, A, A, dt=torch.uint8), LR.AREA)
        assert out[3].numel() == 0
    with pytest.raises(Exception, match="power of two"):
        ops.late_fuse(e(2, 64, 5), e(2, 64), e(2, dt=torch.int32), e(1, 2, 2, 8), e(1, 2, 2, dt=torch.uint8), LR.AREA, cap_out=96)
    torch.cuda.synchronize()


@pytest.mark.parametrize("index", [1, 2])
def test_batch_independence(device, index):
    """An ego alone (B = 1, its own frame only) and inside the batch: identical bits -- in the bit-matrix form and, for the 513-candidate frame, the
    serial one, which then runs in a launch where it is the only pending ego."""
    d = LR.make_late_case(index)
    c = d["case"]
    full = _run(device, d["boxes"], d["scores"], d["counts"], d["rigid"], d["link"], c.extents, c.nms_thr, c.rotated, c.cap_out)
    b = c.B - 1
    rows = [j * c.B + b for j in range(c.A)]
    alone = _run(device, d["boxes"][rows], d["scores"][rows], d["counts"][rows], d["rigid"][b:b + 1], d["link"][b:b + 1], c.extents, c.nms_thr, c.rotated, c.cap_out)
    for i in range(c.A):
        n = full[3][i * c.B + b]
        assert alone[3][i] == n and n > 0
        for q in range(3):
            assert np.array_equal(alone[q][i, :n].view(np.uint32), full[q][i * c.B + b, :n].view(np.uint32))


def test_scene_property(device):
    """12 seeded scenes (sensor range 18 m, 40 cars), every agent's detections = its own ground truth, crop +-29 m: late-fused mAP@0.5 and @0.7
    against the cars in range of ANY agent are exactly 1.0, the ego-only lists reach at most 0.66; no consulted IoU within 1e-3 of the threshold.
    All scenes in ONE call (B = 12).  A wrong pose convention or direction cannot pass (tests/test_late_refs_cpu.py shows both fail)."""
    ins = [LR.scene_inputs(s) for s in LR.SCENE_SEEDS]
    A, B, cap = ins[0][0].shape[0], len(ins), ins[0][0].shape[1]
    boxes = np.stack([ins[b][0][j] for j in range(A) for b in range(B)])
    scores = np.stack([ins[b][1][j] for j in range(A) for b in range(B)])
    counts = np.array([ins[b][2][j] for j in range(A) for b in range(B)], np.int32)
    rigid = P.late_rigid_from_trans(np.concatenate([ins[b][3] for b in range(B)]))
    link = np.ones((B, A, A), np.uint8)
    ob, osc, osrc, ocnt = _run(device, boxes, scores, counts, rigid, link, LR.SCENE_CROP, 0.01, False, 1024)
    assert (ocnt > 0).all()
    for b in range(B):
        gt_any = ins[b][4]
        ann = [P.box_corners(g.astype(np.float64)) for g in gt_any]
        late = [{"corners": P.box_corners(ob[i * B + b, :ocnt[i * B + b]].astype(np.float64)), "scores": osc[i * B + b, :ocnt[i * B + b]]} for i in range(A)]
        ego = [{"corners": P.box_corners(boxes[i * B + b, :counts[i * B + b]].astype(np.float64)), "scores": scores[i * B + b, :counts[i * B + b]]} for i in range(A)]
        for i in range(A):
            ref = LR.ego_reference(boxes, scores, counts, rigid, link, A, B, cap, 1024, LR.SCENE_CROP, 0.01, False, i, b)
            assert (np.abs(ref["consulted"].iou - 0.01) > 1e-3).all()
            _assert_ego((ob, osc, osrc, ocnt), i * B + b, ref, ("scene", b, i))
        for thr in (0.5, 0.7):
            assert P.eval_map(late, ann, thr)[0] == 1.0, (b, thr)
            assert P.eval_map(ego, ann, thr)[0] <= 0.66, (b, thr)


def test_rigid_device_derivation_equals_host(device):
    """predict_all derives `rigid` where trans_matrices already is (late_rigid_from_trans_torch: torch float64 on the device, rounded once): bit-equal
    to the host derivation on the scenes' poses, the case table's and the quadrant edges of atan2."""
    for T in LR.rigid_equality_inputs():
        got = P.late_rigid_from_trans_torch(torch.from_numpy(T).to(device))
        assert got.is_cuda and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy().view(np.uint32), P.late_rigid_from_trans(T).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ module and driver
def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lowerbound_ckpt(device, tmp_path_factory):
    """A short-trained lowerbound detector (tools/det/train_codet.py on synthetic scenes, as tests/test_gpu_dataset.py trains its own)."""
    logdir = str(tmp_path_factory.mktemp("late_ckpt"))
    _load(os.path.join(ROOT, "tools", "det", "train_codet.py"), "late_train_codet").main(
        ["--data", "synthetic", "--com", "lowerbound", "--steps", "120", "--batch", "2", "--logpath", logdir])
    return os.path.join(logdir, "epoch_1.pth")


@pytest.mark.parametrize("mask", ["all", "only_v2i", "user"])
def test_module_late_fusion(device, lowerbound_ckpt, mask):
    """FaFModule.late_fusion on the trained detector, two frames of five agents with one empty sweep: for every ego the fused list equals the
    reference applied to the SAME module's per-agent detections (late_fusion off); absent and empty agents keep None."""
    from v2x_sim_amd import ops
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.det import FaFNet
    from v2x_sim_amd.utils import synthetic_scene
    from v2x_sim_amd.utils.CoDetModule import FaFModule
    A, B = 5, 2
    config = Config("test")
    model = FaFNet(config, layer=3, kd_flag=0, num_agent=A)
    model.load_state_dict(torch.load(lowerbound_ckpt, map_location="cpu")["model_state_dict"], strict=True)
    model = model.eval().to(device)
    batch = synthetic_scene.make_batch(B, A, seed=77)
    grid = ops.VoxelGrid()
    n_pts = batch["n_pts"].copy()
    n_pts[3 * B + 1] = 0                                   # agent 3 of frame 1: an empty sweep
    bits = ops.voxelize_bits(torch.from_numpy(batch["points"]).to(device), torch.from_numpy(n_pts).to(device), grid)
    bev = ops.bits_to_dense(bits, grid.dims[2]).unsqueeze(1)
    data = {"bev_seq": bev, "trans_matrices": torch.from_numpy(batch["trans"]).to(device), "num_agent": torch.from_numpy(batch["num_agent"])}
    module = FaFModule(model, None, config, None, 0)
    module.score_thr = 0.5
    plain = module.predict_all(data, B, validation=False, num_agent=A)[3]
    assert plain[3][1] is None and sum(len(d["scores"]) for row in plain for d in row if d is not None) > 10
    module.late_fusion = True
    link = np.ones((B, A, A), bool)
    if mask == "only_v2i":
        module.late_only_v2i = True
        link[:] = np.eye(A, dtype=bool)
        link[:, :, 0] = link[:, 0, :] = True
    elif mask == "user":
        link = np.random.default_rng(3).random((B, A, A)) < 0.5
        link[:, np.arange(A), np.arange(A)] = True
        link[0, 2, :] = link[0, :, 2] = False                  # agent 2 is taken out of frame 0
        module.set_link_mask(torch.from_numpy(link))
    fused = module.predict_all(data, B, validation=False, num_agent=A)[3]
    cap = 64
    while cap < max(len(d["scores"]) for row in plain for d in row if d is not None):
        cap *= 2
    boxes = np.zeros((A * B, cap, 5), np.float32)
    scores = np.zeros((A * B, cap), np.float32)
    counts = np.zeros(A * B, np.int32)
    for j in range(A):
        for b in range(B):
            if plain[j][b] is not None:
                n = len(plain[j][b]["scores"])
                boxes[j * B + b, :n], scores[j * B + b, :n], counts[j * B + b] = plain[j][b]["boxes"], plain[j][b]["scores"], n
    present = np.array([[plain[j][b] is not None and link[b, j, j] for j in range(A)] for b in range(B)])
    L = (link & present[:, :, None] & present[:, None, :]).astype(np.uint8)
    rigid = P.late_rigid_from_trans(batch["trans"])
    from_nb = 0
    for i in range(A):
        for b in range(B):
            if not present[b, i]:
                assert fused[i][b] is None
                continue
            ref = LR.ego_reference(boxes, scores, counts, rigid, L, A, B, cap, 4096, config.area_extents, module.nms_thr, False, i, b)
            g = fused[i][b]
            assert len(g["scores"]) == ref["count"], (i, b)
            if ref["count"]:
                assert np.array_equal(g["boxes"].view(np.uint32), ref["boxes"].view(np.uint32))
                assert np.array_equal(g["scores"].view(np.uint32), ref["score_bits"])
                assert g["src_agent"].tolist() == (ref["src"] // cap).tolist()
                from_nb += int((g["src_agent"] != i).sum())
    assert from_nb > 0
    # the numpy path (device_postprocess off) gives the same lists
    module.device_postprocess = False
    host = module.predict_all(data, B, validation=False, num_agent=A)[3]
    for i in range(A):
        for b in range(B):
            assert (host[i][b] is None) == (fused[i][b] is None)
            if fused[i][b] is not None:
                assert host[i][b]["src_agent"].tolist() == fused[i][b]["src_agent"].tolist()
                np.testing.assert_allclose(host[i][b]["boxes"], fused[i][b]["boxes"], rtol=0, atol=1e-3)


def test_driver_com_late(device, lowerbound_ckpt, tmp_path, capsys):
    """tools/det/test_codet.py under --com late on a parsed tree (through tools/det/eval_codet.py: the driver's own file stays as it is) accepts the
    lowerbound checkpoint, runs, and reports the neighbours' share; tools/track/track_codet.py --com late on the same tree."""
    from v2x_sim_amd import ops
    from v2x_sim_amd.datasets import write_sample
    from v2x_sim_amd.utils import synthetic_scene
    A, frames = 5, 2
    grid = ops.VoxelGrid()
    root = os.path.join(str(tmp_path), "V2X-Sim-det")
    for f in range(frames):
        sc = synthetic_scene.make_scene(A, seed=9100 + f)
        bits = ops.voxelize_bits(torch.from_numpy(sc["points"]).to(device), torch.from_numpy(sc["n_pts"]).to(device), grid)
        idx, cnt = ops.bits_to_indices(bits, grid.dims[2], 32768)
        idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
        for a in range(A):
            write_sample(root, "test", a, 7, f, idx[a, :cnt[a]], sc["trans"][a], A, gt_boxes=sc["gt_boxes"][a])
    mod = _load(os.path.join(ROOT, "tools", "det", "eval_codet.py"), "late_eval_codet_gpu")
    res = mod.main(["--data", os.path.join(root, "test"), "--com", "late", "--resume", lowerbound_ckpt, "--batch", "2", "--score_thr", "0.5"])
    out = capsys.readouterr().out
    assert "average local mAP@0.5" in out and "late fusion:" in out and "came from neighbours" in out
    assert 0.0 <= res[0.5] <= 1.0 and res["late_kept"] > 0 and 0 <= res["late_from_neighbours"] <= res["late_kept"]
    # the tracking driver on the same tree: one MOT-challenge file per agent for the one scene, and the same report
    trk = _load(os.path.join(ROOT, "tools", "track", "track_codet.py"), "late_track_codet_gpu")
    out_dir = os.path.join(str(tmp_path), "tracks")
    tres = trk.main(["--data", os.path.join(root, "test"), "--out", out_dir, "--com", "late", "--resume", lowerbound_ckpt, "--score_thr", "0.5", "--min_hits", "1"])
    out = capsys.readouterr().out
    assert "late fusion:" in out and "came from neighbours" in out
    assert sorted(tres["files"]) == sorted(os.path.join(out_dir, "agent%d" % a, "7.txt") for a in range(A)) and tres["lines"] > 0

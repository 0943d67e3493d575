"""The LiDAR ray cast on the MI355X: v2x_lidar_cast and v2x_lidar_visible_boxes (csrc/lidar_cast.hip) against the float64 reference and the case table
of tests/lidar_refs.py.  At sigma_r = 0 every output equals the reference BIT FOR BIT -- no tolerance, no excluded ray --, the guard regions around
every output stay untouched and a second call gives identical bytes.  At sigma_r > 0 hits, counts and intensities stay exact and the coordinates lie
within sigma_r * 1e-5 + 2^-23 |coordinate| of the float64 evaluation of the same draw (tests/test_gpu_channel.py's bound for the same Box-Muller on the
same libm: the normal to 1e-5 absolute, one fp32 rounding of the sum; here the product with a direction component of magnitude <= 1 and the store add
half an ulp each, which the two 2^-24 terms of 2^-23 hold).  Then the occlusion case end to end through raycast_batch_on_device, and one training step."""
import numpy as np
import pytest
import torch

import lidar_refs as LR

pytestmark = pytest.mark.gpu
GUARD = 64
SENTINEL_I = -77777


def _guarded(shape, dtype, device):
    """A tensor of `shape` inside a larger buffer: NaN (fp32) or a sentinel (int32) on both sides and, before the call, in the tensor itself."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * GUARD,), float("nan") if dtype == torch.float32 else SENTINEL_I, dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + numel].view(shape)


def _guards_intact(buf):
    h = buf.cpu()
    edge = torch.cat([h[:GUARD], h[-GUARD:]])
    return bool(torch.isnan(edge).all()) if h.dtype == torch.float32 else bool((edge == SENTINEL_I).all())


def _scene_on(sc, device):
    return {k: torch.from_numpy(np.array(sc[k])).to(device) for k in ("sensors", "frame_of", "boxes", "box_count", "beam", "az")}


def _cast(sc, device, want=("hit", "box_hits"), guarded=True):
    from v2x_sim_amd import ops
    d = _scene_on(sc, device)
    n, cap, mp = sc["sensors"].shape[0], sc["boxes"].shape[1], sc["max_pts"]
    shapes = {"points": ((n, mp, 4), torch.float32), "n_pts": ((n,), torch.int32), "hit": ((n, mp), torch.int32), "box_hits": ((n, cap), torch.int32)}
    bufs, out = {}, None
    if guarded:
        out = {}
        for k, (shape, dtype) in shapes.items():
            if k in ("points", "n_pts") or k in want:
                bufs[k], out[k] = _guarded(shape, dtype, device)
    res = ops.lidar_cast(d["sensors"], d["frame_of"], d["boxes"], d["box_count"], d["beam"], d["az"], mp, ground_z=sc["ground_z"], r_min=sc["r_min"],
                         r_max=sc["r_max"], sigma_r=sc["sigma_r"], p_drop=sc["p_drop"], seed=sc["seed"], step=sc["step"], want=want, out=out)
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert _guards_intact(b), (k, "guard region written")
    return d, res


def _visible(sc, d, box_hits, any_agent, device):
    from v2x_sim_amd import ops
    n, cap = sc["sensors"].shape[0], sc["boxes"].shape[1]
    (bg, gt), (bc, cnt) = _guarded((n, cap, 5), torch.float32, device), _guarded((n,), torch.int32, device)
    ops.visible_boxes(box_hits, d["sensors"], d["frame_of"], d["boxes"], d["box_count"], min_hits=sc["min_hits"], any_agent=any_agent, x_lim=sc["x_lim"],
                      y_lim=sc["y_lim"], out=(gt, cnt))
    torch.cuda.synchronize()
    assert _guards_intact(bg) and _guards_intact(bc)
    return gt.cpu().numpy(), cnt.cpu().numpy()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


@pytest.mark.parametrize("index", range(len(LR.CASES)), ids=LR.NAMES)
def test_case_equals_the_reference_bit_for_bit(device, index):
    sc = LR.make_case(index)
    ref = sc["ref"]
    d, res = _cast(sc, device)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    for k in ("n_pts", "hit", "box_hits", "points"):
        bad = np.argwhere(got[k].view(np.uint32) != ref[k].view(np.uint32)) if got[k].dtype == np.float32 else np.argwhere(got[k] != ref[k])
        assert _same_bits(got[k], ref[k]), (LR.NAMES[index], k, len(bad), bad[:4].tolist(), got[k][tuple(bad[0])], ref[k][tuple(bad[0])])
    for any_agent, key in ((False, "gt_own"), (True, "gt_any")):
        gt, cnt = _visible(sc, d, res["box_hits"], any_agent, device)
        assert np.array_equal(cnt, ref[key][1]), (LR.NAMES[index], key, cnt, ref[key][1])
        assert _same_bits(gt, ref[key][0]), (LR.NAMES[index], key)
    _, again = _cast(sc, device)
    for k in got:
        assert _same_bits(again[k].cpu().numpy(), got[k]), (LR.NAMES[index], k, "second call")


@pytest.mark.parametrize("index", range(len(LR.NOISE_CASES)), ids=[n for n, _ in LR.NOISE_CASES])
def test_range_noise(device, index):
    sc = LR.make_noise_case(index)
    ref, sigma = sc["ref"], float(np.float32(sc["sigma_r"]))
    _, res = _cast(sc, device)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    for k in ("n_pts", "hit", "box_hits"):
        assert np.array_equal(got[k], ref[k]), k
    assert _same_bits(np.ascontiguousarray(got["points"][..., 3]), np.ascontiguousarray(ref["points"][..., 3]))           # the intensities: exact
    err = np.abs(got["points"][..., :3].astype(np.float64) - ref["points64"][..., :3])
    bound = sigma * 1e-5 + 2.0 ** -23 * np.abs(ref["points64"][..., :3])
    moved = np.abs(got["points"][..., :3].astype(np.float64) - LR.cast_ref(dict(sc, sigma_r=0.0))["points64"][..., :3]).max()
    print("%s: worst coordinate error %.3g (bound there %.3g); the noise moves a coordinate by up to %.3g" % (
        LR.NOISE_CASES[index][0], err.max(), bound.reshape(-1)[err.argmax()], moved))
    assert (err <= bound).all(), float((err - bound).max())
    assert moved > sigma                                                                                                  # the noise is there
    _, again = _cast(sc, device)
    assert _same_bits(again["points"].cpu().numpy(), got["points"])


def test_optional_outputs_in_both_orders(device):
    sc = LR.make_case(LR.NAMES.index("seven_sweeps_three_frames_shuffled"))
    _, full = _cast(sc, device)
    for want in ((), ("hit",), ("box_hits",)):
        _, part = _cast(sc, device, want=want)
        assert set(part) == {"points", "n_pts"} | set(want)
        for k in part:
            assert torch.equal(part[k], full[k]), (want, k)
    _, plain = _cast(sc, device, guarded=False)                         # outputs the wrapper allocates itself
    assert all(torch.equal(plain[k], full[k]) for k in full)


def test_zero_sweeps(device):
    from v2x_sim_amd import ops
    sc = LR.make_case(0)
    d = _scene_on(sc, device)
    res = ops.lidar_cast(d["sensors"][:0], d["frame_of"][:0], d["boxes"], d["box_count"], d["beam"], d["az"], 8)
    assert res["points"].shape == (0, 8, 4) and res["box_hits"].shape == (0, 1)
    gt, cnt = ops.visible_boxes(res["box_hits"], d["sensors"][:0], d["frame_of"][:0], d["boxes"], d["box_count"])
    assert gt.shape == (0, 1, 5) and cnt.shape == (0,)


def _occlusion_world():
    """tests/lidar_refs.py's occlusion scene as a make_world dict: the car first (the only label), the wall after it; two sensors, one frame."""
    from v2x_sim_amd.utils import synthetic_scene
    car, wall = (12.0, 0.5, 4.4, 2.0, 0.0, -1.8, -0.25), (6.0, 0.0, 0.5, 12.0, 0.0, -1.8, 2.0)
    sensors = np.asarray([[0, 0, 0, 0.0], [18.0, -1.0, 0.0, 3.0]], np.float32)
    T, T_geo = synthetic_scene.warp_transforms([synthetic_scene._pose(float(s[3]), float(s[0]), float(s[1])) for s in sensors])
    return {"sensors": sensors, "frame_of": np.zeros((2,), np.int32), "boxes": np.asarray([[car, wall]], np.float32), "box_count": np.asarray([2], np.int32),
            "car_count": np.asarray([1], np.int32), "trans": T[None], "trans_geo": T_geo[None], "num_agent": np.full((1, 2), 2, np.int64)}, car


def test_occlusion_end_to_end(device):
    """raycast_batch_on_device on the wall scene: the dict of the sampled path; A's occupancy is empty inside the hidden car's footprint, B's is not;
    A's labels hold a positive for the car under gt="any" and none under gt="own"."""
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.train.loop import synthetic_batch_on_device
    from v2x_sim_amd.utils import postprocess
    cfg = Config("train", binary=True, only_det=True)
    anchors = postprocess.build_anchor_map(cfg)
    world, car = _occlusion_world()
    data = {gt: synthetic_batch_on_device(cfg, 1, 2, 3, device, anchors=anchors, scene="raycast", gt=gt, gt_lists=True, sigma_r=0.0, world=world)
            for gt in ("own", "any")}
    sampled = synthetic_batch_on_device(cfg, 1, 2, 3, device, anchors=anchors, targets="iou", ground_pts=50, clutter_pts=10, pts_per_car=20)
    for gt, dd in data.items():
        assert set(dd) == set(sampled)
        for k, v in sampled.items():
            if isinstance(v, torch.Tensor):
                assert (dd[k].shape, dd[k].dtype, dd[k].device) == (v.shape, v.dtype, v.device), (gt, k)
        assert len(dd["gt_boxes"]) == 2 and all(len(row) == 1 and row[0].dtype == np.float32 and row[0].shape[1] == 5 for row in dd["gt_boxes"])
    assert torch.equal(data["own"]["bev_seq"], data["any"]["bev_seq"])
    # occupied cells in the world frame, against the car's footprint shrunk by 0.3 m (more than a cell)
    x0, y0, vx, vy = float(cfg.area_extents[0][0]), float(cfg.area_extents[1][0]), float(cfg.voxel_size[0]), float(cfg.voxel_size[1])
    inside = []
    for m, s in enumerate(world["sensors"]):
        ij = data["own"]["bev_seq"][m, 0].any(-1).nonzero().cpu().numpy()
        assert ij.shape[0] > 1000
        x, y = x0 + (ij[:, 0] + 0.5) * vx, y0 + (ij[:, 1] + 0.5) * vy
        wx, wy = s[0] + np.cos(s[3]) * x - np.sin(s[3]) * y, s[1] + np.sin(s[3]) * x + np.cos(s[3]) * y
        inside.append(int(((np.abs(wx - car[0]) < car[2] / 2 - 0.3) & (np.abs(wy - car[1]) < car[3] / 2 - 0.3)).sum()))
    print("occupied cells inside the car's footprint: A %d, B %d" % tuple(inside))
    assert inside[0] == 0 and inside[1] >= 5
    assert [len(data["own"]["gt_boxes"][a][0]) for a in range(2)] == [0, 1] and [len(data["any"]["gt_boxes"][a][0]) for a in range(2)] == [1, 1]
    assert np.allclose(data["any"]["gt_boxes"][0][0][0], [12.0, 0.5, 4.4, 2.0, 0.0])
    pos_own, pos_any = data["own"]["labels"][0, ..., 1], data["any"]["labels"][0, ..., 1]
    assert int(pos_own.sum()) == 0 and int(pos_any.sum()) >= 1
    ij = pos_any.nonzero()[:, :2].cpu().numpy()
    assert (np.hypot(anchors[ij[:, 0], ij[:, 1], 0, 0] - 12.0, anchors[ij[:, 0], ij[:, 1], 0, 1] - 0.5) < 3.0).all()       # the positives sit on the car
    assert int(data["own"]["labels"][1, ..., 1].sum()) >= 1 and torch.equal(data["own"]["labels"][1], data["any"]["labels"][1])


def test_one_training_step_on_a_raycast_batch(device):
    """One FaFModule.step on a 1-frame x 2-agent ray-cast batch (make_world's scene, the default engine): a finite loss, with positives to learn from."""
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.det import FaFNet
    from v2x_sim_amd.train.loop import init_for_training, synthetic_batch_on_device
    from v2x_sim_amd.utils.CoDetModule import FaFModule
    cfg = Config("train", binary=True, only_det=True)
    data = synthetic_batch_on_device(cfg, 1, 2, seed=10, device=device, scene="raycast")
    assert "gt_boxes" not in data and int(data["reg_loss_mask"].sum()) > 0 and data["bev_seq"].shape[0] == 2
    model = init_for_training(FaFNet(cfg, kd_flag=0, num_agent=2), seed=1).to(device).train()
    module = FaFModule(model, None, cfg, torch.optim.SGD(model.parameters(), lr=1e-3), 0)
    out = module.step(data, 1, 2)
    assert all(np.isfinite(v) for v in out) and out[0] > 0

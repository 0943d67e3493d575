"""The MOVING LiDAR ray cast on the MI355X: v2x_lidar_cast_moving and v2x_lidar_visible_boxes_moving (csrc/lidar_cast.hip) against the float64 reference
and the case table of tests/lidar_motion_refs.py.  At sigma_r = 0 every output -- points, n_pts, hit, box_hits, gt_boxes, gt_count, gt_ids, gt_vel --
equals the reference BIT FOR BIT, the guard regions around every output stay untouched and a second call gives identical bytes; at sigma_r > 0 the
comparison is tests/test_gpu_lidar.py::test_range_noise's, with its bound.  With nothing moving the bytes are ops.lidar_cast's from the same process.
Then the sequences end to end: tools/track/synth_tracks.py on two hand-made worlds against the reference pipeline (float64 SORT on the reference's
ground truth), and one training step on a moving batch."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import lidar_motion_refs as MR
import lidar_refs as LR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
SENTINEL_I = -77777
SCENE_KEYS = ("sensors", "sensor_vel", "time_of", "frame_of", "boxes", "box_vel", "box_count", "beam", "az", "az_time")


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
    return {k: torch.from_numpy(np.array(sc[k])).to(device) for k in SCENE_KEYS}


def _cast_args(sc, d):
    return (d["sensors"], d["sensor_vel"], d["time_of"], d["frame_of"], d["boxes"], d["box_vel"], d["box_count"], d["beam"], d["az"], d["az_time"], sc["max_pts"])


def _cast_kw(sc):
    return dict(ground_z=sc["ground_z"], r_min=sc["r_min"], r_max=sc["r_max"], sigma_r=sc["sigma_r"], p_drop=sc["p_drop"], seed=sc["seed"], step=sc["step"])


def _cast(sc, device, want=("hit", "box_hits"), guarded=True, d=None):
    from v2x_sim_amd import ops
    d = d or _scene_on(sc, device)
    n, cap, mp = sc["sensors"].shape[0], sc["boxes"].shape[1], sc["max_pts"]
    shapes = {"points": ((n, mp, 4), torch.float32), "n_pts": ((n,), torch.int32), "hit": ((n, mp), torch.int32), "box_hits": ((n, cap), torch.int32)}
    bufs, out = {}, None
    if guarded:
        out = {}
        for k, (shape, dtype) in shapes.items():
            if k in ("points", "n_pts") or k in want:
                bufs[k], out[k] = _guarded(shape, dtype, device)
    res = ops.lidar_cast_moving(*_cast_args(sc, d), want=want, out=out, **_cast_kw(sc))
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert _guards_intact(b), (k, "guard region written")
    return d, res


def _visible(sc, d, box_hits, any_agent, device, want=("gt_vel",), guarded=True):
    from v2x_sim_amd import ops
    n, cap = sc["sensors"].shape[0], sc["boxes"].shape[1]
    shapes = {"gt_boxes": ((n, cap, 5), torch.float32), "gt_count": ((n,), torch.int32), "gt_ids": ((n, cap), torch.int32), "gt_vel": ((n, cap, 2), torch.float32)}
    bufs, out = {}, None
    if guarded:
        out = {}
        for k, (shape, dtype) in shapes.items():
            if k != "gt_vel" or k in want:
                bufs[k], out[k] = _guarded(shape, dtype, device)
    res = ops.visible_boxes_moving(box_hits, d["sensors"], d["sensor_vel"], d["time_of"], d["frame_of"], d["boxes"], d["box_vel"], d["box_count"],
                                   t_ref=sc["t_ref"], min_hits=sc["min_hits"], any_agent=any_agent, x_lim=sc["x_lim"], y_lim=sc["y_lim"], want=want, out=out)
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert _guards_intact(b), (k, "guard region written")
    return {k: v.cpu().numpy() for k, v in res.items()}


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_gt(name, sc, d, box_hits, device):
    for any_agent, key in ((False, "gt_own"), (True, "gt_any")):
        got = _visible(sc, d, box_hits, any_agent, device)
        for k, want in zip(("gt_boxes", "gt_count", "gt_ids", "gt_vel"), sc["ref"][key]):
            assert _same_bits(got[k], want), (name, key, k, got[k][:1], want[:1])


@pytest.mark.parametrize("index", range(len(MR.CASES)), ids=MR.NAMES)
def test_case_equals_the_reference_bit_for_bit(device, index):
    sc = MR.make_case(index)
    ref, name = sc["ref"], MR.NAMES[index]
    d, res = _cast(sc, device)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    for k in ("n_pts", "hit", "box_hits", "points"):
        bad = np.argwhere(got[k].view(np.uint32) != ref[k].view(np.uint32)) if got[k].dtype == np.float32 else np.argwhere(got[k] != ref[k])
        assert _same_bits(got[k], ref[k]), (name, k, len(bad), bad[:4].tolist(), got[k][tuple(bad[0])], ref[k][tuple(bad[0])])
    _check_gt(name, sc, d, res["box_hits"], device)
    _, again = _cast(sc, device, d=d)
    for k in got:
        assert _same_bits(again[k].cpu().numpy(), got[k]), (name, k, "second call")


@pytest.mark.parametrize("index", range(len(MR.NOISE_CASES)), ids=[n for n, _ in MR.NOISE_CASES])
def test_range_noise(device, index):
    """tests/test_gpu_lidar.py::test_range_noise's comparison and bound: hits, counts and intensities exact, the coordinates within sigma_r * 1e-5 +
    2^-23 |coordinate| of the float64 evaluation of the same draw."""
    sc = MR.make_noise_case(index)
    ref, sigma = sc["ref"], float(np.float32(sc["sigma_r"]))
    d, res = _cast(sc, device)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    for k in ("n_pts", "hit", "box_hits"):
        assert np.array_equal(got[k], ref[k]), k
    assert _same_bits(np.ascontiguousarray(got["points"][..., 3]), np.ascontiguousarray(ref["points"][..., 3]))
    err = np.abs(got["points"][..., :3].astype(np.float64) - ref["points64"][..., :3])
    bound = sigma * 1e-5 + 2.0 ** -23 * np.abs(ref["points64"][..., :3])
    moved = np.abs(got["points"][..., :3].astype(np.float64) - MR.cast_moving_ref(dict(sc, sigma_r=0.0))["points64"][..., :3]).max()
    print("%s: worst coordinate error %.3g (bound there %.3g); the noise moves a coordinate by up to %.3g" % (
        MR.NOISE_CASES[index][0], err.max(), bound.reshape(-1)[err.argmax()], moved))
    assert (err <= bound).all(), float((err - bound).max())
    assert moved > sigma
    _check_gt(MR.NOISE_CASES[index][0], sc, d, res["box_hits"], device)
    _, again = _cast(sc, device, d=d)
    assert _same_bits(again["points"].cpu().numpy(), got["points"])


@pytest.mark.parametrize("name", ["seven_sweeps_three_frames_shuffled", "cap256_full_3x87", "occlusion_wall", "p_drop_half"])
def test_nothing_moving_gives_the_static_entries_bytes(device, name):
    """Zero velocities and zero times: ops.lidar_cast / ops.visible_boxes on the same scene, from the same process."""
    from v2x_sim_amd import ops
    sc = dict(MR.moving(LR.make_case(LR.NAMES.index(name)), az_time=np.zeros(LR.make_case(LR.NAMES.index(name))["az"].shape[0]), t_ref=0.0))
    d, res = _cast(sc, device)
    static = ops.lidar_cast(d["sensors"], d["frame_of"], d["boxes"], d["box_count"], d["beam"], d["az"], sc["max_pts"], **_cast_kw(sc))
    for k in ("points", "n_pts", "hit", "box_hits"):
        assert torch.equal(res[k].view(torch.int32), static[k].view(torch.int32)), (name, k)
    for any_agent in (False, True):
        gt, cnt = ops.visible_boxes(static["box_hits"], d["sensors"], d["frame_of"], d["boxes"], d["box_count"], min_hits=sc["min_hits"], any_agent=any_agent,
                                    x_lim=sc["x_lim"], y_lim=sc["y_lim"])
        got = _visible(sc, d, res["box_hits"], any_agent, device)
        assert _same_bits(got["gt_boxes"], gt.cpu().numpy()) and _same_bits(got["gt_count"], cnt.cpu().numpy()) and not got["gt_vel"].any()


def test_optional_outputs_in_both_orders(device):
    sc = MR.make_case(MR.NAMES.index("negative_time_of"))
    d, full = _cast(sc, device)
    for want in ((), ("hit",), ("box_hits",)):
        _, part = _cast(sc, device, want=want, d=d)
        assert set(part) == {"points", "n_pts"} | set(want)
        for k in part:
            assert torch.equal(part[k], full[k]), (want, k)
    _, plain = _cast(sc, device, guarded=False, d=d)                    # outputs the wrapper allocates itself
    assert all(torch.equal(plain[k], full[k]) for k in full)
    with_vel = _visible(sc, d, full["box_hits"], False, device)
    for kw in (dict(want=()), dict(want=(), guarded=False), dict(guarded=False)):
        part = _visible(sc, d, full["box_hits"], False, device, **kw)
        assert set(part) == {"gt_boxes", "gt_count", "gt_ids"} | set(kw.get("want", ("gt_vel",)))
        assert all(_same_bits(part[k], with_vel[k]) for k in part), kw
    assert with_vel["gt_vel"].any()


def test_zero_sweeps(device):
    from v2x_sim_amd import ops
    sc = MR.make_case(MR.NAMES.index("negative_time_of"))
    d = _scene_on(sc, device)
    res = ops.lidar_cast_moving(d["sensors"][:0], d["sensor_vel"][:0], d["time_of"][:0], d["frame_of"][:0], d["boxes"], d["box_vel"], d["box_count"], d["beam"],
                                d["az"], d["az_time"], 8)
    assert res["points"].shape == (0, 8, 4) and res["box_hits"].shape == (0, 16)
    vis = ops.visible_boxes_moving(res["box_hits"], d["sensors"][:0], d["sensor_vel"][:0], d["time_of"][:0], d["frame_of"][:0], d["boxes"], d["box_vel"],
                                   d["box_count"])
    assert vis["gt_boxes"].shape == (0, 16, 5) and vis["gt_count"].shape == (0,) and vis["gt_ids"].shape == (0, 16) and vis["gt_vel"].shape == (0, 16, 2)


def test_captured_in_a_graph_and_replayed(device):
    """The cast's two launches and the ground truth's one, in sequence on one stream (no parallel branch), captured once and replayed twice into
    poisoned outputs: the reference's bytes both times."""
    from v2x_sim_amd import ops
    sc = MR.make_case(MR.NAMES.index("max_pts_below_moving"))
    ref = sc["ref"]
    d = _scene_on(sc, device)
    n, cap, mp = sc["sensors"].shape[0], sc["boxes"].shape[1], sc["max_pts"]
    out = {"points": torch.empty((n, mp, 4), device=device), "n_pts": torch.empty((n,), dtype=torch.int32, device=device),
           "hit": torch.empty((n, mp), dtype=torch.int32, device=device), "box_hits": torch.empty((n, cap), dtype=torch.int32, device=device)}
    vout = {"gt_boxes": torch.empty((n, cap, 5), device=device), "gt_count": torch.empty((n,), dtype=torch.int32, device=device),
            "gt_ids": torch.empty((n, cap), dtype=torch.int32, device=device), "gt_vel": torch.empty((n, cap, 2), device=device)}

    def run():
        ops.lidar_cast_moving(*_cast_args(sc, d), out=out, **_cast_kw(sc))
        ops.visible_boxes_moving(out["box_hits"], d["sensors"], d["sensor_vel"], d["time_of"], d["frame_of"], d["boxes"], d["box_vel"], d["box_count"],
                                 t_ref=sc["t_ref"], min_hits=sc["min_hits"], x_lim=sc["x_lim"], y_lim=sc["y_lim"], out=vout)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                                               # warm-up outside the capture: allocations settle
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    first = None
    for _ in range(2):
        for t in list(out.values()) + list(vout.values()):
            t.fill_(float("nan") if t.dtype == torch.float32 else SENTINEL_I)
        graph.replay()
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in list(out.items()) + list(vout.items())}
        for k in ("points", "n_pts", "hit", "box_hits"):
            assert _same_bits(got[k], ref[k]), k
        for k, want in zip(("gt_boxes", "gt_count", "gt_ids", "gt_vel"), ref["gt_own"]):
            assert _same_bits(got[k], want), k
        if first is not None:
            assert all(_same_bits(got[k], first[k]) for k in got)
        first = got


# ---- sequences end to end -------------------------------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("synth_tracks_cli", os.path.join(ROOT, "tools", "track", "synth_tracks.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _frame_ids(path):
    out = set()
    with open(path) as fh:
        for line in fh:
            v = line.split(",")
            out.add((int(v[0]), int(v[1])))
    return out


STEPS = 8


@pytest.fixture(scope="module")
def sequences(tmp_path_factory):
    """synth_tracks.py --detections gt --score on the two hand-made worlds (scene0: open road, scene1: wall), under --gt own and --gt any, and the
    reference pipeline's answers for the same worlds, computed once."""
    scenes = [MR.open_road(STEPS), MR.wall_road(STEPS)]
    world = MR.world_of(scenes)
    tool, runs = _tool(), {}
    for gt in ("own", "any"):
        out = str(tmp_path_factory.mktemp("seq_" + gt))
        runs[gt] = tool.main(["--out", out, "--scenes", "2", "--steps", str(STEPS), "--num_agent", "2", "--gt", gt, "--detections", "gt", "--score",
                              "--beams", "8", "--az_steps", "256", "--elev_deg", "-12", "0", "--sigma_r", "0"], world=world)
    refs = {gt: [MR.reference_pipeline(sc, gt, STEPS) for sc in scenes] for gt in ("own", "any")}
    return runs, refs


def _row(run, a, w):
    return next(r for r in run["score"]["files"] if r["name"] == os.path.join("agent%d" % a, "scene%d.txt" % w))


def test_sequence_text_equals_the_reference_pipeline(device, sequences):
    """Ground-truth text and track text as (frame, id) sets, per agent and scene, against cast_moving_ref -> visible_moving_ref -> float64 SORT."""
    runs, refs = sequences
    for gt in ("own", "any"):
        for w in range(2):
            for a in range(2):
                gts, trks = refs[gt][w][a]
                want_gt = {(f, i) for f in gts for i in gts[f][0]}
                want_trk = {(f, int(i)) for f in trks for i in trks[f][0]}
                assert _frame_ids(os.path.join(runs[gt]["gt"], "agent%d" % a, "scene%d.txt" % w)) == want_gt, (gt, w, a)
                assert _frame_ids(os.path.join(runs[gt]["trk"], "agent%d" % a, "scene%d.txt" % w)) == want_trk, (gt, w, a)
                assert want_gt and want_trk


def test_open_road_has_no_identity_switch(device, sequences):
    runs, _ = sequences
    for gt in ("own", "any"):
        for a in range(2):
            row = _row(runs[gt], a, 0)
            assert row["IDSW"] == 0 and row["Frag"] == 0 and row["TP"] == 3 * STEPS and row["FN"] == 0, (gt, a, row)


def test_wall_breaks_the_hidden_cars_track_under_own_ground_truth_only(device, sequences):
    """Sensor A (agent 0) loses car 0 (ground-truth id 1) behind the wall for two steps, longer than max_age = 1: under --gt own the car's track is
    fragmented or switches identity -- car 1 (id 2) stands in the open, present and tracked under one id in every frame, so the event is car 0's --,
    under --gt any its ground truth is continuous (B sees it throughout)."""
    runs, _ = sequences
    own, anyb = _row(runs["own"], 0, 1), _row(runs["any"], 0, 1)
    assert own["Frag"] + own["IDSW"] >= 1, own
    gt_own = _frame_ids(os.path.join(runs["own"]["gt"], "agent0", "scene1.txt"))
    gt_any = _frame_ids(os.path.join(runs["any"]["gt"], "agent0", "scene1.txt"))
    assert {f for f, i in gt_own if i == 1} == {1, 2, 5, 6, 7, 8} and {f for f, i in gt_own if i == 2} == set(range(1, STEPS + 1))
    assert {f for f, i in gt_any if i == 1} == set(range(1, STEPS + 1))
    trk = _frame_ids(os.path.join(runs["own"]["trk"], "agent0", "scene1.txt"))
    assert len({i for _, i in trk}) == 3                                  # car 1 under one id, car 0 under two
    assert anyb["IDSW"] == 0, anyb


def test_one_training_step_on_a_moving_batch(device):
    """The twin of tests/test_gpu_lidar.py::test_one_training_step_on_a_raycast_batch: one FaFModule.step on a raycast_sequence_on_device batch (one
    world, two agents, two steps): a finite loss, a finite gradient for every parameter, positives to learn from."""
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.det import FaFNet
    from v2x_sim_amd.train.loop import init_for_training, synthetic_batch_on_device
    from v2x_sim_amd.utils.CoDetModule import FaFModule
    cfg = Config("train", binary=True, only_det=True)
    data = synthetic_batch_on_device(cfg, 2, 2, seed=10, device=device, scene="raycast-moving")
    assert int(data["reg_loss_mask"].sum()) > 0 and data["bev_seq"].shape[0] == 4 and data["gt_ids"].shape[0] == 4 and data["trans_matrices"].shape[:3] == (2, 2, 2)
    ids, cnt = data["gt_ids"].cpu().numpy(), data["gt_count"].cpu().numpy()
    assert all((ids[m, :cnt[m]] >= 0).all() and (ids[m, cnt[m]:] == -1).all() for m in range(4)) and cnt.sum() > 0
    model = init_for_training(FaFNet(cfg, kd_flag=0, num_agent=2), seed=1).to(device).train()
    module = FaFModule(model, None, cfg, torch.optim.SGD(model.parameters(), lr=1e-3), 0)
    out = module.step(data, 2, 2)
    assert all(np.isfinite(v) for v in out) and out[0] > 0
    grads = [p.grad for p in model.parameters() if p.requires_grad]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)

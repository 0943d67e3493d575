"""v2x_det_map (csrc/det_map.hip) on the MI355X against the float64 reference of tests/det_map_refs.py: the true-positive flags of every threshold,
the rank of every detection and the counts EXACTLY, AP within (num_tp + 1) * 2^-50; bit-reproducible; guard regions intact; the flags equal
v2x_match_detections' per threshold; DetMap against eval_map / eval_map_device on the scale case; tools/det/map_codet.py --map_engine device
against tools/det/test_codet.py on a parsed dataset.

The AP bound is derived, not measured: each true positive contributes one term (two divisions and a subtraction give the recall step, one product:
the step k/G - (k-1)/G carries at most 2 ulp of its operands ~ 2^-52 absolute since both are <= 1, the product with the envelope <= 1 one more
rounding), the partial sums are <= 1, so each of the num_tp additions adds at most 2^-53; the reference sums exactly (math.fsum)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import det_map_refs as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64          # sentinel elements on both sides of every output


def ap_bound(num_tp):
    return (np.asarray(num_tp, np.float64) + 1.0) * 2.0 ** -50


class _Guarded(object):
    """A device buffer of `shape` with GUARD sentinel elements before and after it, all pre-filled with the sentinel."""

    def __init__(self, shape, dtype, sentinel, device):
        self.numel, self.shape, self.sentinel = int(np.prod(shape)), shape, sentinel
        self.buf = torch.full((self.numel + 2 * GUARD,), sentinel, dtype=dtype, device=device)
        self.view = self.buf[GUARD:GUARD + self.numel]

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def guards_intact(self):
        g = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.numel:]]).cpu().numpy()
        return bool(np.isnan(g).all()) if isinstance(self.sentinel, float) else bool((g == self.sentinel).all())

    def numpy(self):
        return self.view.cpu().numpy().reshape(self.shape)


def _upload(case, device):
    return {k: torch.from_numpy(np.array(case[k])).to(device) for k in ("det", "scores", "det_count", "gt", "gt_count", "group")}


def call_entry(case, dev_in, device, want_flags):
    """ONE v2x_det_map call through the C ABI on guarded, sentinel-filled outputs and an exactly sized, guarded workspace."""
    from v2x_sim_amd import _lib
    lib = _lib.load()
    n, det_cap, gt_cap, G, T = len(case["group"]), case["det_cap"], case["gt_cap"], case["n_groups"], len(case["thrs"])
    out = {"ap": _Guarded((G, T), torch.float64, float("nan"), device), "num_gt": _Guarded((G,), torch.int64, -7777, device),
           "num_det": _Guarded((G,), torch.int64, -7777, device), "num_tp": _Guarded((G, T), torch.int64, -7777, device)}
    if want_flags:
        out["tp"] = _Guarded((T, n, det_cap), torch.uint8, 0xAB, device)
        out["rank"] = _Guarded((n, det_cap), torch.int32, -7777, device)
    nbytes = lib.v2x_det_map_workspace_size(n, det_cap, gt_cap, G, T)
    assert nbytes == 2 * n * det_cap
    ws = _Guarded((nbytes,), torch.uint8, 0xCD, device)
    thr = torch.tensor(case["thrs"], dtype=torch.float32, device=device)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.v2x_det_map(ptr(dev_in["det"]), ptr(dev_in["scores"]), ptr(dev_in["det_count"]), det_cap, ptr(dev_in["gt"]), ptr(dev_in["gt_count"]), gt_cap,
                         ptr(dev_in["group"]), n, G, ptr(thr), T, out["ap"].ptr(), out["num_gt"].ptr(), out["num_det"].ptr(), out["num_tp"].ptr(),
                         out["tp"].ptr() if want_flags else None, out["rank"].ptr() if want_flags else None, ws.ptr(), nbytes,
                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "v2x_det_map")
    torch.cuda.synchronize()
    for k, o in list(out.items()) + [("workspace", ws)]:
        assert o.guards_intact(), "%s: a guard element around the buffer was overwritten" % k
    return {k: o.numpy() for k, o in out.items()}


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_det_map_against_float64(device, name):
    from v2x_sim_amd import ops
    case = R.make_case(name)
    ref = case["ref"]
    n, T = len(case["group"]), len(case["thrs"])
    dev_in = _upload(case, device)
    got = call_entry(case, dev_in, device, True)
    if n == 0:
        # the entry returns V2X_OK before the pointer checks and touches nothing; the wrapper returns zeros itself
        assert np.isnan(got["ap"]).all() and (got["num_gt"] == -7777).all() and (got["num_tp"] == -7777).all()
        ap, num_gt, num_det, num_tp, tp, rank = ops.det_map(dev_in["det"], dev_in["scores"], dev_in["det_count"], dev_in["gt"], dev_in["gt_count"], dev_in["group"],
                                                            case["thrs"], case["n_groups"], want_flags=True)
        assert ap.shape == (case["n_groups"], T) and not ap.any() and not num_gt.any() and not num_det.any() and not num_tp.any() and tp.shape == (T, 0, case["det_cap"])
        return
    err = np.abs(got["ap"] - ref["ap"])
    print("%-26s AP error worst / bound %.3g (worst %.3g), %d detections, %d true positives" % (
        name, float((err / ap_bound(ref["num_tp"])).max()), float(err.max()), int(ref["num_det"].sum()), int(ref["num_tp"].sum())))
    for k in ("tp", "rank", "num_gt", "num_det", "num_tp"):           # every element written (no sentinel left) and equal to the reference
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (name, k, np.argwhere(got[k] != ref[k])[:8])
    assert not np.isnan(got["ap"]).any() and (err <= ap_bound(ref["num_tp"])).all(), (name, got["ap"], ref["ap"])
    # a second call: identical bits; without the optional outputs: the same table
    again = call_entry(case, dev_in, device, True)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), (name, k)
    bare = call_entry(case, dev_in, device, False)
    for k in ("ap", "num_gt", "num_det", "num_tp"):
        assert got[k].tobytes() == bare[k].tobytes(), (name, k)
    # the flags of each threshold are v2x_match_detections' at that threshold, bit for bit (rows below the count: the others are not written there)
    nd = np.clip(case["det_count"], 0, case["det_cap"])
    live = np.arange(case["det_cap"])[None, :] < nd[:, None]
    for t, thr in enumerate(case["thrs"]):
        single = ops.match_detections(dev_in["det"], dev_in["det_count"], dev_in["gt"], dev_in["gt_count"], float(thr)).cpu().numpy()
        assert np.array_equal(single[live], got["tp"][t][live].astype(np.int32)), (name, thr)
    # the wrapper: same bits as the raw entry
    ap, num_gt, num_det, num_tp = ops.det_map(dev_in["det"], dev_in["scores"], dev_in["det_count"], dev_in["gt"], dev_in["gt_count"], dev_in["group"],
                                              case["thrs"], case["n_groups"])
    assert ap.cpu().numpy().tobytes() == got["ap"].tobytes() and np.array_equal(num_tp.cpu().numpy(), got["num_tp"])
    assert np.array_equal(num_gt.cpu().numpy(), got["num_gt"]) and np.array_equal(num_det.cpu().numpy(), got["num_det"])


def test_detmap_class_on_the_scale_case(device):
    """DetMap (update per map in a SHUFFLED detection order: it sorts) = utils/postprocess.py::eval_map per agent and threshold within the bound, and
    matches eval_map_device; update_batch on the padded device tensors gives the same bits."""
    from v2x_sim_amd.utils import postprocess as P
    from v2x_sim_amd.utils.det_metrics import DetMap
    case = R.make_case("scale")
    ref = case["ref"]
    G, thrs = case["n_groups"], case["thrs"]
    rng = np.random.default_rng(5)
    m = DetMap(iou_thrs=thrs, n_groups=G)
    for i in range(len(case["group"])):
        nd, ng = case["det_count"][i], case["gt_count"][i]
        # a permutation that keeps equal scores in their order (eval_map's stable sort must see the same ties)
        perm = rng.permutation(nd)
        sc = case["scores"][i, :nd]
        for v in np.unique(sc):
            pos = np.nonzero(sc[perm] == v)[0]
            perm[pos] = np.sort(perm[pos])
        m.update({"boxes": case["det"][i, perm], "scores": sc[perm]}, case["gt"][i, :ng], group=int(case["group"][i]))
    res = m.result(device)
    assert res["ap"].dtype == np.float64 and res["ap"].shape == (G, len(thrs)) and np.array_equal(res["mean_ap"], res["ap"].mean(0))
    assert np.array_equal(res["num_gt"], ref["num_gt"]) and np.array_equal(res["num_det"], ref["num_det"]) and np.array_equal(res["num_tp"], ref["num_tp"])
    dev_in = _upload(case, device)
    for g in range(G):
        dets, gts = R.host_lists(case, g)
        sel = torch.from_numpy(np.nonzero(case["group"] == g)[0]).to(device)
        gt_list = [case["gt"][i, :case["gt_count"][i]] for i in np.nonzero(case["group"] == g)[0]]
        for t, thr in enumerate(thrs):
            ap_host, info = P.eval_map(dets, gts, thr)
            ap_dev, _ = P.eval_map_device(dev_in["det"][sel], dev_in["scores"][sel], dev_in["det_count"][sel], gt_list, thr)
            print("agent %d  mAP@%.1f  DetMap %.17g  eval_map %.17g  eval_map_device %.17g" % (g, thr, res["ap"][g, t], ap_host, ap_dev))
            assert info["num_gt"] == res["num_gt"][g]
            assert abs(res["ap"][g, t] - ap_host) <= ap_bound(res["num_tp"][g, t]) and abs(res["ap"][g, t] - ap_dev) <= ap_bound(res["num_tp"][g, t])
    b = DetMap(iou_thrs=thrs, n_groups=G)
    b.update_batch(dev_in["det"], dev_in["scores"], dev_in["det_count"], dev_in["gt"], dev_in["gt_count"], dev_in["group"])
    assert b.result()["ap"].tobytes() == res["ap"].tobytes()
    with pytest.raises(ValueError):
        b.update_batch(dev_in["det"], dev_in["scores"], dev_in["det_count"] - 100, dev_in["gt"], dev_in["gt_count"], dev_in["group"])
    with pytest.raises(ValueError):
        b.update_batch(dev_in["det"], dev_in["scores"].flip(1), dev_in["det_count"] * 0 + case["det_cap"], dev_in["gt"], dev_in["gt_count"], dev_in["group"])
    with pytest.raises(ValueError):
        b.update_batch(dev_in["det"], dev_in["scores"] * float("nan"), dev_in["det_count"], dev_in["gt"], dev_in["gt_count"], dev_in["group"])


def test_map_codet_device_engine_equals_the_default(device, tmp_path, capsys):
    """tools/det/map_codet.py (and tools/det/eval_codet.py, which drives it) on a small synthetic parsed dataset, built as
    tests/test_gpu_dataset.py builds its own: without the flag and with --map_engine host the output IS tools/det/test_codet.py's;
    --map_engine device returns the same two means within the bound and prints the same lines.  The ground truth is written from the
    model's own detections (shrunk copies: IoU 0.9 and 0.6, and one box far away) so that the APs are not trivially zero."""
    from oracle import voxelize_ref as VR
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.datasets import write_sample
    from v2x_sim_amd.models.det import V2VNet
    from v2x_sim_amd.utils import postprocess as P
    from v2x_sim_amd.utils.synthetic import init_synthetic_weights, synthetic_points, synthetic_poses
    A, frames = 3, 2
    pts = synthetic_points(A * frames, 15000, seed=31)
    T = synthetic_poses(frames, A, seed=32)
    rng = np.random.default_rng(1)
    far = np.array([[40.0, 40.0, 2.0, 4.0, 0.3]])

    def write(gt_of):
        for f in range(frames):
            for a in range(A):
                _, idx = VR.voxelize_occupy(pts[a * frames + f], return_indices=True)
                write_sample(str(tmp_path), "test", a, 3, f, idx, T[f, a], A, gt_boxes=gt_of(a, f))
    write(lambda a, f: np.concatenate([rng.uniform(-25, 25, (6, 2)), np.tile([2.0, 4.0], (6, 1)), rng.uniform(-1, 1, (6, 1))], 1))
    ckpt = os.path.join(str(tmp_path), "ckpt.pth")
    torch.save({"epoch": 1, "model_state_dict": init_synthetic_weights(V2VNet(Config("test"), num_agent=A), seed=4).state_dict()}, ckpt)
    spec = importlib.util.spec_from_file_location("test_codet", os.path.join(ROOT, "tools", "det", "test_codet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    argv = ["--data", os.path.join(str(tmp_path), "test"), "--com", "v2v", "--resume", ckpt, "--num_agent", str(A), "--batch", "2", "--score_thr", "0.55"]
    # first pass (default engine): record what eval_map is given, per agent the detections of its frames in order
    seen, orig = [], P.eval_map
    P.eval_map = lambda dets, anns, thr: (seen.append(dets), orig(dets, anns, thr))[1]
    try:
        mod.main(argv)
    finally:
        P.eval_map = orig
    per_agent = seen[0::2]          # two thresholds per agent
    assert len(per_agent) == A and all(len(d) == frames for d in per_agent)

    def from_detections(a, f):
        b = np.asarray(per_agent[a][f]["boxes"], np.float32).reshape(-1, 5)[:6].copy()
        b[0::2, 2] *= np.float32(0.9)
        b[1::2, 2] *= np.float32(0.6)
        return np.concatenate([b.astype(np.float64), far], 0)
    write(from_detections)
    capsys.readouterr()

    def load(name):
        sp = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", "det", name + ".py"))
        m = importlib.util.module_from_spec(sp)
        sp.loader.exec_module(m)
        return m
    tool, wrapper = load("map_codet"), load("eval_codet")
    ref = mod.main(argv)                                   # test_codet.py itself
    out_ref = capsys.readouterr().out
    runs = {}
    for name, fn, extra in (("default", tool.main, []), ("host", tool.main, ["--map_engine", "host"]), ("device", tool.main, ["--map_engine", "device"]),
                            ("wrapper-device", wrapper.main, ["--map_engine=device"])):
        runs[name] = (fn(argv + extra), capsys.readouterr().out)
    print(runs["device"][1])
    n_tp = sum(min(6, len(per_agent[a][f]["scores"])) for a in range(A) for f in range(frames))
    assert set(ref) == {0.5, 0.7} and "average local mAP@0.5" in out_ref and out_ref.count("agent") >= A
    for name in ("default", "host"):
        assert runs[name] == (ref, out_ref), name
    for name in ("device", "wrapper-device"):
        res, out = runs[name]
        assert set(res) == {0.5, 0.7}
        for iou in (0.5, 0.7):
            assert abs(res[iou] - ref[iou]) <= ap_bound(n_tp), (name, iou, res[iou], ref[iou])
        assert out == out_ref, (name, out, out_ref)
    assert n_tp == 0 or ref[0.5] > ref[0.7] > 0.0

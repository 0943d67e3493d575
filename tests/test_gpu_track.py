"""GPU tests of row f-5 (csrc/track.hip: assign_kernel, sort_step_kernel; utils/tracking.py, utils/mot_metrics.py) against the float64 references of
tests/track_refs.py.

Decisions (ids, matched detections, the counters of every stream and track) must EQUAL the reference's on generated cases that survive the
coin-flip filter (track_refs.kept).  Values are held to max(8 x d32, 16 ulp): d32 = the deviation of the reference's OWN float32 run from its float64
run on that case and quantity (never taken from the kernel), x 8 for a different but equally fp32 operation order (three decoupled 2-state filters and
fused multiply-adds instead of 7 x 7 matrix products), ulp = a float32 step at the quantity's largest magnitude in the case (a floor for quantities
whose float32 reference run happens to be exact).  Quantities: the reported boxes, each of the 7 state components, each of the 10 stored covariance entries.
"""
import functools

import numpy as np
import pytest
import torch

import track_refs as R

pytestmark = pytest.mark.gpu

CAP = 64
NAN = float("nan")


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def _state(n, t_cap, dev):
    return (torch.zeros((n, t_cap, 17), dtype=torch.float32, device=dev), torch.zeros((n, t_cap, 5), dtype=torch.int32, device=dev),
            torch.zeros((n, 4), dtype=torch.int32, device=dev))


def _pack(dets_per_stream, det_cap, width=4):
    """list (stream) of [k][width] arrays -> (n, det_cap, width) float32 with NaN behind each stream's rows (an over-read shows), counts."""
    n = len(dets_per_stream)
    buf = np.full((n, det_cap, width), NAN, dtype=np.float32)
    cnt = np.zeros(n, dtype=np.int32)
    for s, d in enumerate(dets_per_stream):
        d = np.asarray(d, dtype=np.float32).reshape(-1, width)
        k = min(len(d), det_cap)
        buf[s, :k] = d[:k]
        cnt[s] = len(d)
    return buf, cnt


def _run_gpu(seqs, dev, t_cap=CAP, det_cap=CAP, box_format=0, counts=None, hook=None, **kw):
    """seqs: list (stream) of lists (frame) of detection arrays.  One launch per frame for all streams.  -> per stream the list of frame records
    (the layout of track_refs.run_case).  counts[s][f] overrides det_count; hook(f, state) runs before frame f (tests that write states)."""
    from v2x_sim_amd import ops
    n, frames = len(seqs), len(seqs[0])
    width = 4 if box_format == 0 else 5
    st = _state(n, t_cap, dev)
    out = [[] for _ in range(n)]
    for f in range(frames):
        if hook is not None:
            hook(f, st)
        buf, cnt = _pack([seqs[s][f] for s in range(n)], det_cap, width)
        if counts is not None:
            cnt = np.array([counts[s][f] for s in range(n)], dtype=np.int32)
        boxes, ids, det, count = ops.sort_step(torch.from_numpy(buf).to(dev), torch.from_numpy(cnt).to(dev), *st, box_format=box_format, **kw)
        boxes, ids, det, count = boxes.cpu().numpy(), ids.cpu().numpy(), det.cpu().numpy(), count.cpu().numpy()
        tf, ti, si = (t.cpu().numpy() for t in st)
        for s in range(n):
            k, nt = int(count[s]), int(si[s, 0])
            out[s].append({"boxes": boxes[s, :k].astype(np.float64), "ids": ids[s, :k].astype(np.int64), "det": det[s, :k].astype(np.int64),
                           "stream_i": si[s].astype(np.int64), "trk_i": ti[s, :nt].astype(np.int64), "trk_f": tf[s, :nt].astype(np.float64)})
    return out


def _run_ref(seq, counts=None, hook=None, dtype=np.float64, **kw):
    kw = dict(kw)
    if "iou_thr" not in kw:
        kw["iou_thr"] = R.IOU_THR
    trk = R.SortRef(dtype=dtype, **kw)
    frames = []
    for f, d in enumerate(seq):
        if hook is not None:
            hook(f, trk)
        boxes, ids, det = trk.step(d, None if counts is None else counts[f])
        frames.append({"boxes": boxes.astype(np.float64), "ids": ids, "det": det, "stream_i": trk.stream_i(), "trk_i": trk.trk_i(), "trk_f": trk.trk_f()})
    return frames


def _same_decisions(got, want, what=""):
    for f, (g, w) in enumerate(zip(R.decisions(got), R.decisions(want))):
        assert g == w, "%s frame %d:\n kernel    %s\n reference %s" % (what, f, g, w)


def _check(seqs, dev, ref_kw=None, **kw):
    """Run the streams on the kernel and each through the reference; decisions must be equal.  -> (kernel records, reference records)."""
    got = _run_gpu(seqs, dev, **kw)
    ref_kw = dict(ref_kw or {})
    for k in ("max_age", "min_hits", "direct", "iou_thr", "t_cap"):
        if k in kw:
            ref_kw[k] = kw[k]
    counts = kw.get("counts")
    want = [_run_ref(seqs[s], counts=None if counts is None else counts[s], **ref_kw) for s in range(len(seqs))]
    for s in range(len(seqs)):
        _same_decisions(got[s], want[s], "stream %d" % s)
    return got, want


def _box(cx, cy, w=4.0, h=2.0):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]


# ---- the assignment kernel ----------------------------------------------------------------------------------------------------------------
def _quantised(rng, nr, nc):
    return rng.integers(0, 1025, (nr, nc)).astype(np.float64) / 1024.0


def _assign_gpu(mats, dev, thr, direct, cap_r=CAP, cap_c=CAP):
    from v2x_sim_amd import ops
    n = len(mats)
    buf = np.full((n, cap_r, cap_c), 0.75, dtype=np.float32)      # behind the live block: entries a stride slip would pick up
    nr = np.array([m.shape[0] for m in mats], dtype=np.int32)
    nc = np.array([m.shape[1] for m in mats], dtype=np.int32)
    for k, m in enumerate(mats):
        buf[k, :m.shape[0], :m.shape[1]] = m
    r2c = ops.assign_iou(torch.from_numpy(buf).to(dev), torch.from_numpy(nr).to(dev), torch.from_numpy(nc).to(dev), thr=thr, direct=direct)
    return r2c.cpu().numpy()


ASSIGN_LAUNCHES = [
    ((1, 1), (1, 5), (5, 1)),
    ((7, 7), (13, 9), (9, 13)),
    ((64, 64), (64, 3), (3, 64)),
    ((0, 6), (6, 0), (5, 5)),           # n_rows = 0, n_cols = 0; the third is replaced by an all-zero matrix
]


@pytest.mark.parametrize("launch", range(len(ASSIGN_LAUNCHES)))
def test_assign_kernel_reaches_the_optimum_exactly(device, launch):
    """IoUs that are multiples of 2^-10: every sum is exact in fp64, so the total of the kernel's pairs must EQUAL the reference optimum (thr = 0: every
    pair of the assignment is reported); with thr = 0.3 the same assignment comes back with exactly the pairs below the threshold removed."""
    rng = np.random.default_rng(100 + launch)
    mats = [_quantised(rng, nr, nc) for nr, nc in ASSIGN_LAUNCHES[launch]]
    if launch == 3:
        mats[2] = np.zeros((5, 5))
    for cap_r, cap_c in ((CAP, CAP), (max(m.shape[0] for m in mats) or 1, max(m.shape[1] for m in mats) or 1)):
        full = _assign_gpu(mats, device, 0.0, False, cap_r, cap_c)
        cut = _assign_gpu(mats, device, 0.3, False, cap_r, cap_c)
        for k, m in enumerate(mats):
            nr, nc = m.shape
            assert R.is_partial_matching(full[k], nr, nc), (k, full[k])
            assert sum(int(c) >= 0 for c in full[k]) == min(nr, nc)
            want = sum(m[r, c] for r, c in R.assign_max(m))
            assert R.matching_total(m, full[k][:nr]) == want, (launch, k, m.shape)
            expect = [int(c) if c >= 0 and not m[r, c] < 0.3 else -1 for r, c in enumerate(full[k][:nr])]
            assert cut[k][:nr].tolist() == expect and R.is_partial_matching(cut[k], nr, nc)
            assert all(m[r, c] >= 0.3 for r, c in enumerate(cut[k][:nr]) if c >= 0)


def test_assign_kernel_direct_reading_and_bad_entries(device):
    """direct = 1 on a matrix built so that the readings differ gives the direct reading (and direct = 0 the other); NaN / inf entries read as 0 and the
    result is a valid matching; three different sizes per launch."""
    a = np.array([[0.35, 0.29], [0.29, 0.0]])
    b = np.array([[0.5, 0.4, 0.0], [0.45, 0.0, 0.0]])
    c = np.array([[NAN, 0.6, 0.1, 0.2], [np.inf, 0.1, 0.7, -np.inf], [0.2, NAN, NAN, 0.9], [0.1, 0.2, 0.3, 0.4], [0.9, 0.0, 0.0, NAN]])
    for direct in (True, False):
        got = _assign_gpu([a, b, c], device, 0.3, direct)
        for k, m in enumerate((a, b, c)):
            nr, nc = m.shape
            assert R.is_partial_matching(got[k], nr, nc)
            assert got[k][:nr].tolist() == R.associate(m, 0.3, direct).tolist(), (direct, k, got[k][:nr])
    assert _assign_gpu([a], device, 0.3, True)[0][:2].tolist() == [0, -1]
    assert _assign_gpu([a], device, 0.3, False)[0][:2].tolist() == [-1, -1]


# ---- the tracker on generated scenes --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(seed, direct):
    dets, gt = R.make_case(seed)
    _, f64 = R.run_case(dets, direct)
    _, f32 = R.run_case(dets, direct, dtype=np.float32)
    return dets, gt, f64, f32


_GPU_RUNS = {}


def _scene_runs(direct, dev):
    """Six kept seeds, three streams per launch (their detection counts differ frame by frame); run once per reading, shared by the tests."""
    if direct not in _GPU_RUNS:
        seeds = R.kept_seeds(direct, 6)
        assert len(seeds) == 6
        runs = {}
        for group in (seeds[:3], seeds[3:]):
            got = _run_gpu([_reference(s, direct)[0] for s in group], dev, direct=direct)
            runs.update(dict(zip(group, got)))
        _GPU_RUNS[direct] = runs
    return _GPU_RUNS[direct]


@pytest.mark.parametrize("direct", [False, True])
def test_tracker_decisions_equal_the_reference(device, direct):
    for seed, got in _scene_runs(direct, device).items():
        _same_decisions(got, _reference(seed, direct)[2], "seed %d direct %d" % (seed, direct))
        assert any(len(f["ids"]) for f in got) and max(int(f["stream_i"][1]) for f in got) > R.N_OBJ      # tracks were reported, born and replaced


QUANTITIES = [("boxes", "boxes", None)] + [("x%d" % k, "trk_f", k) for k in range(7)] + [("P%d" % k, "trk_f", 7 + k) for k in range(10)]


@pytest.mark.parametrize("direct", [False, True])
def test_tracker_values_within_the_fp32_reference_deviation(device, direct):
    worst = 0.0
    for seed, got in _scene_runs(direct, device).items():
        _, _, f64, f32 = _reference(seed, direct)
        assert R.decisions(f32) == R.decisions(f64), seed             # d32 is a deviation between two runs that decided alike
        _same_decisions(got, f64, "seed %d" % seed)
        for name, key, col in QUANTITIES:
            pick = (lambda fr: fr[key]) if col is None else (lambda fr: fr[key][:, col])
            d32 = max([float(np.abs(pick(a) - pick(b)).max()) for a, b in zip(f32, f64) if pick(a).size] or [0.0])
            err = max([float(np.abs(pick(a) - pick(b)).max()) for a, b in zip(got, f64) if pick(a).size] or [0.0])
            mag = max([float(np.abs(pick(b)).max()) for b in f64 if pick(b).size] or [0.0])
            tol = max(8 * d32, 16 * float(np.spacing(np.float32(mag))))
            ratio = err / d32 if d32 > 0 else 0.0
            worst = max(worst, ratio)
            print("seed %2d direct %d %-5s |ref| %.3g  d32 %.3g  kernel %.3g  tol %.3g  kernel/d32 %.2f" % (seed, direct, name, mag, d32, err, tol, ratio))
            assert err <= tol, (seed, name, err, tol, d32)
    print("direct %d: largest kernel / d32 = %.2f" % (direct, worst))


# ---- edges, each at its smallest shape ------------------------------------------------------------------------------------------------------
def test_empty_first_frame_and_a_stream_without_detections(device):
    seqs = [[[], [_box(0, 0)], [_box(0.2, 0)], [_box(0.4, 0)]], [[], [], [], []]]
    got, _ = _check(seqs, device)
    assert got[0][0]["stream_i"].tolist() == [0, 0, 1, 0] and len(got[0][0]["ids"]) == 0
    assert [f["stream_i"].tolist() for f in got[1]] == [[0, 0, k, 0] for k in (1, 2, 3, 4)]
    assert got[0][2]["ids"].tolist() == [1] and got[0][3]["trk_i"].tolist() == [[1, 0, 2, 2, 2]]


def test_death_then_birth_never_reuses_an_id_and_keeps_ascending_order(device):
    a, b, c = _box(0, 0), _box(20, 0), _box(-20, 5)
    seq = [[a, b], [a, b], [a, b], [b], [b], [b], [c, b], [b, c]]
    got, _ = _check([seq], device, min_hits=1)
    g = got[0]
    assert g[2]["trk_i"][:, 0].tolist() == [1, 2]
    assert g[5]["trk_i"][:, 0].tolist() == [2]                         # id 1 died (max_age = 1)
    assert g[6]["trk_i"][:, 0].tolist() == [2, 3] and g[7]["trk_i"][:, 0].tolist() == [2, 3]
    assert g[7]["ids"].tolist() == [2, 3] and g[7]["det"].tolist() == [0, 1]


def test_min_hits_warm_up(device):
    a, b = _box(0, 0), _box(20, 0)
    seq = [[a], [a], [a, b], [a, b], [a, b], [a, b]]
    got, _ = _check([seq], device, min_hits=3)
    assert [f["ids"].tolist() for f in got[0]] == [[1], [1], [1, 2], [1], [1], [1, 2]]


def test_max_age_bridges_a_gap_of_two_frames(device):
    a = _box(0, 0)
    seq = [[a], [a], [a], [], [], [a], [a]]
    got, _ = _check([seq], device, max_age=3, min_hits=1)
    assert [f["trk_i"][:, 0].tolist() for f in got[0]] == [[1]] * 7
    assert got[0][5]["ids"].tolist() == [1] and got[0][4]["trk_i"][0, 1] == 2
    got1, _ = _check([seq], device, max_age=1, min_hits=1)             # the default loses it
    assert got1[0][5]["trk_i"][:, 0].tolist() == [2]


def test_track_capacity_drops_the_later_births(device):
    boxes = [_box(6 * k, 0) for k in range(11)]
    got, _ = _check([[boxes, boxes]], device, t_cap=8)
    f = got[0][0]
    assert f["stream_i"].tolist() == [8, 8, 1, 2] and f["ids"].tolist() == list(range(1, 9)) and f["det"].tolist() == list(range(8))
    assert got[0][1]["stream_i"].tolist() == [8, 8, 2, 2] and got[0][1]["det"].tolist() == list(range(8))


def test_seventy_detections_read_sixty_four(device):
    boxes = [_box(6 * (k % 10), 4 * (k // 10)) for k in range(70)]
    got, _ = _check([[boxes, boxes]], device, det_cap=80)
    assert got[0][0]["stream_i"].tolist() == [64, 64, 1, 1]
    assert got[0][1]["ids"].tolist() == list(range(1, 65)) and got[0][1]["det"].tolist() == list(range(64))


def test_negative_count_is_an_empty_frame(device):
    a = _box(0, 0)
    got, _ = _check([[[a], [a], [a]]], device, counts=[[1, -5, 1]], max_age=2)
    assert [f["stream_i"].tolist() for f in got[0]] == [[1, 1, 1, 0], [1, 1, 2, 4], [1, 1, 3, 4]]
    assert len(got[0][1]["ids"]) == 0 and got[0][2]["ids"].tolist() == [1]


def test_non_finite_prediction_removes_that_track_only(device):
    boxes = [_box(0, 0), _box(20, 0), _box(40, 0)]

    def gpu_hook(f, st):
        if f == 2:
            st[0][0, 1, 2] = -1.0                                      # s < 0: sqrt(s r) is NaN

    def ref_hook(f, trk):
        if f == 2:
            trk.tracks[1].x[2] = -1.0

    got = _run_gpu([[boxes] * 4], device, hook=gpu_hook)
    want = _run_ref([boxes] * 4, hook=ref_hook)
    _same_decisions(got[0], want)
    assert got[0][2]["trk_i"][:, 0].tolist() == [1, 3, 4]              # 2 left before the association, its detection started id 4
    assert got[0][2]["trk_i"][:2, 2].tolist() == [2, 2]                # the others matched as before
    plain = _run_gpu([[boxes] * 4], device)[0]                         # the same frames without the damage: tracks 1 and 3 carry the same bits
    for f in range(4):
        for tid in (1, 3):
            a = got[0][f]["trk_f"][got[0][f]["trk_i"][:, 0] == tid]
            b = plain[f]["trk_f"][plain[f]["trk_i"][:, 0] == tid]
            assert a.shape == (1, 17) and np.array_equal(a, b), (f, tid)


@pytest.mark.parametrize("wh_axis,fmt", [("w_along_heading", 1), ("h_along_heading", 2)])
def test_rotated_box_formats_measure_the_stand_up_box(device, wh_axis, fmt):
    """(x, y, w, h, yaw) through box_format 1 / 2 against box_format 0 on utils/postprocess.py's box_corners + standup of the same boxes: the same
    decisions, boxes within 1e-4 m (the device's sinf / cosf against numpy's on extents of a few metres)."""
    from v2x_sim_amd.utils import postprocess
    rng = np.random.default_rng(5)
    c0 = rng.uniform(-20, 20, (6, 2))
    v = rng.uniform(-1, 1, (6, 2))
    wh = np.stack([rng.uniform(3.5, 5.5, 6), rng.uniform(1.7, 2.4, 6)], 1)
    yaw = rng.uniform(-np.pi, np.pi, 6)
    rot, std = [], []
    for f in range(5):
        b = np.concatenate([c0 + v * f, wh, (yaw + 0.02 * f)[:, None]], 1).astype(np.float32)
        rot.append(b)
        std.append(postprocess.standup(postprocess.box_corners(b.astype(np.float64), wh_axis)).astype(np.float32))
    got_r = _run_gpu([rot], device, box_format=fmt)[0]
    got_s = _run_gpu([std], device)[0]
    _same_decisions(got_r, got_s)
    for a, b in zip(got_r, got_s):
        np.testing.assert_allclose(a["boxes"], b["boxes"], atol=1e-4, rtol=0)
    if fmt == 2:                                                        # and the two readings do measure different boxes
        other = _run_gpu([rot], device, box_format=1)[0]
        assert np.abs(other[0]["boxes"] - got_r[0]["boxes"]).max() > 0.1


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------------
def _rotated_frames(seed, n, frames):
    rng = np.random.default_rng(seed)
    k = [int(rng.integers(2, 7)) for _ in range(n)]
    c0 = [rng.uniform(-20, 20, (kk, 2)) for kk in k]
    out = []
    for f in range(frames):
        boxes = np.full((n, CAP, 5), NAN, dtype=np.float32)
        for s in range(n):
            boxes[s, :k[s], :2] = c0[s] + 0.3 * f
            boxes[s, :k[s], 2:] = (4.5, 2.0, 0.3 * s)
        out.append((boxes, np.array(k, dtype=np.int32)))
    return out


def test_sort_tracker_reproduces_the_kernel_call_resets_and_round_trips(device):
    from v2x_sim_amd import ops
    from v2x_sim_amd.utils.tracking import SortTracker
    frames = [(torch.from_numpy(b).to(device), torch.from_numpy(c).to(device)) for b, c in _rotated_frames(3, 3, 6)]
    trk = SortTracker(3, device=device)
    st = _state(3, CAP, device)
    for b, c in frames[:3]:
        got = trk.update(b, c)
        want = ops.sort_step(b, c, *st, box_format=1)
        n = got[3].cpu()
        assert torch.equal(n, want[3].cpu()) and int(n.min()) >= 2
        for s in range(3):
            for g, w in zip(got[:3], want[:3]):
                assert torch.equal(g[s, :n[s]], w[s, :n[s]])
        for g, w in zip((trk.trk_f, trk.trk_i, trk.stream_i), st):
            assert torch.equal(g, w)
    # state_dict round trip: a second tracker continues the sequence bit-identically
    sd = trk.state_dict()
    twin = SortTracker(3, device=device)
    twin.load_state_dict(sd)
    a, b = trk.update(*frames[3]), twin.update(*frames[3])
    n = a[3].cpu()
    assert torch.equal(n, b[3].cpu()) and all(torch.equal(x[s, :n[s]], y[s, :n[s]]) for x, y in zip(a[:3], b[:3]) for s in range(3))
    assert all(torch.equal(getattr(trk, k), getattr(twin, k)) for k in ("trk_f", "trk_i", "stream_i"))
    assert torch.equal(sd["stream_i"][:, 2].cpu(), torch.full((3,), 3, dtype=torch.int32))          # the dict is a copy
    # reset(streams=[1]) empties stream 1 only
    before = trk.stream_i.cpu().clone()
    trk.reset(streams=[1])
    assert trk.stream_i[1].tolist() == [0, 0, 0, 0] and torch.equal(trk.stream_i[[0, 2]].cpu(), before[[0, 2]])
    out = trk.update(*frames[4])
    k = int(frames[4][1][1])
    assert out[1][1, :k].tolist() == list(range(1, k + 1)) and trk.stream_i[1].tolist() == [k, k, 1, 0]
    assert int(trk.stream_i[0, 2]) == 5
    assert trk.status() == [[], [], []]
    with pytest.raises(RuntimeError):
        trk.update(frames[0][0].cpu(), frames[0][1].cpu())


def test_four_steps_replay_as_one_graph(device):
    """One stream, four steps captured into one graph on the capture's current stream (a chain: no parallel branches) and replayed over fresh input:
    the states and outputs equal four eager steps bit for bit."""
    from v2x_sim_amd import ops
    dets, _ = R.make_case(R.kept_seeds(True, 1)[0])
    warm = [_pack([d], CAP) for d in dets[:4]]
    fresh = [_pack([d], CAP) for d in dets[4:8]]
    det_buf = [torch.from_numpy(b).to(device) for b, _ in warm]
    cnt_buf = [torch.from_numpy(c).to(device) for _, c in warm]
    st = _state(1, CAP, device)
    outs = [(torch.zeros((1, CAP, 4), device=device), torch.zeros((1, CAP), dtype=torch.int32, device=device),
             torch.zeros((1, CAP), dtype=torch.int32, device=device), torch.zeros((1,), dtype=torch.int32, device=device)) for _ in range(4)]
    ops.sort_step(det_buf[0], cnt_buf[0], *st, out=outs[0])            # the library is loaded before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in range(4):
            ops.sort_step(det_buf[k], cnt_buf[k], *st, out=outs[k])
    for t in st:
        t.zero_()
    for k, (b, c) in enumerate(fresh):
        det_buf[k].copy_(torch.from_numpy(b))
        cnt_buf[k].copy_(torch.from_numpy(c))
    g.replay()
    torch.cuda.synchronize()
    st2 = _state(1, CAP, device)
    for k, (b, c) in enumerate(fresh):
        want = ops.sort_step(torch.from_numpy(b).to(device), torch.from_numpy(c).to(device), *st2)
        n = int(want[3])
        assert n == int(outs[k][3]) and n > 0
        assert all(torch.equal(w[0, :n], o[0, :n]) for w, o in zip(want[:3], outs[k][:3]))
    nt = int(st2[2][0, 0])
    assert nt > 0 and torch.equal(st[2], st2[2]) and torch.equal(st[0][0, :nt], st2[0][0, :nt]) and torch.equal(st[1][0, :nt], st2[1][0, :nt])


# ---- the metric -----------------------------------------------------------------------------------------------------------------------------
def test_clear_mot_equals_the_reference_on_tracked_scenes(device):
    """GT = the generator's objects (index = id), tracks = the kernel's output: integer counts equal the reference's, MOTP within 1e-6."""
    from v2x_sim_amd.utils.mot_metrics import ClearMot
    runs = _scene_runs(True, device)
    for seed in list(runs)[:2]:
        gt = _reference(seed, True)[1]
        mot, ref = ClearMot(), R.ClearMotRef()
        gid = list(range(gt.shape[1]))
        for f, rec in enumerate(runs[seed]):
            mot.update(torch.from_numpy(gt[f]).to(device), gid, torch.from_numpy(rec["boxes"]).to(device), rec["ids"].tolist())
            ref.update(gt[f], gid, rec["boxes"], rec["ids"])
        got, want = mot.result(), ref.result()
        print(seed, got)
        for k in ("TP", "FP", "FN", "IDSW"):
            assert got[k] == want[k], (seed, k, got, want)
        assert want["TP"] > 100 and abs(got["MOTP"] - want["MOTP"]) <= 1e-6 and abs(got["MOTA"] - want["MOTA"]) <= 1e-12


# ---- the tool -------------------------------------------------------------------------------------------------------------------------------
def test_track_codet_writes_mot_challenge_text(device, tmp_path, capsys):
    """tools/track/track_codet.py on a parsed synthetic tree (two scenes of three frames, three agents, seeded weights): one file per agent and scene,
    every line `frame,id,x1,y1,w,h,score,-1,-1,-1` with frames counted from 1 within the scene and ids from 1 in every file."""
    import importlib.util
    import os
    from oracle import voxelize_ref as VR
    from v2x_sim_amd.datasets import write_sample
    from v2x_sim_amd.utils.synthetic import synthetic_points, synthetic_poses
    A, scenes, frames = 3, (3, 11), 3
    pts = synthetic_points(A * len(scenes) * frames, 15000, seed=41)
    T = synthetic_poses(len(scenes) * frames, A, seed=42)
    rng = np.random.default_rng(2)
    for si, scene in enumerate(scenes):
        for f in range(frames):
            for a in range(A):
                k = si * frames + f
                _, idx = VR.voxelize_occupy(pts[a * len(scenes) * frames + k], return_indices=True)
                gt = np.concatenate([rng.uniform(-25, 25, (6, 2)), np.tile([2.0, 4.0], (6, 1)), rng.uniform(-1, 1, (6, 1))], 1)
                write_sample(str(tmp_path), "test", a, scene, f, idx, T[k, a], A, gt_boxes=gt)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("track_codet", os.path.join(root, "tools", "track", "track_codet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out_dir = os.path.join(str(tmp_path), "tracks")
    res = mod.main(["--data", os.path.join(str(tmp_path), "test"), "--out", out_dir, "--com", "lowerbound", "--num_agent", str(A), "--batch", "2",
                    "--score_thr", "0.55", "--direct", "0"])
    assert "files" in capsys.readouterr().out
    want = sorted(os.path.join(out_dir, "agent%d" % a, "%d.txt" % s) for a in range(A) for s in scenes)
    assert sorted(res["files"]) == want and all(os.path.isfile(p) for p in want)
    n_lines = 0
    for p in want:
        ids = set()
        for line in open(p):
            v = line.strip().split(",")
            assert len(v) == 10 and v[7:] == ["-1", "-1", "-1"]
            assert 1 <= int(v[0]) <= frames and int(v[1]) >= 1 and float(v[4]) > 0 and float(v[5]) > 0 and 0.55 <= float(v[6]) <= 1.0
            ids.add(int(v[1]))
            n_lines += 1
        assert not ids or min(ids) == 1
    assert n_lines == res["lines"] and n_lines > 0

"""GPU tests of the HOTA family (csrc/hota.hip through ops.hota_sequences; utils/mot_metrics.py::Hota; tools/track/eval_track.py) against the float64
reference of tests/hota_refs.py on cases that survive its coin-flip filter (hota_refs.is_kept).

TP, FN and FP must be EQUAL for every threshold.  AssA, AssRe, AssPr and loc / max(1, TP) are held to 1e-9 absolute: both sides are fp64 and a sum
has at most F x 64 terms in [0, 1], so the derived bound is near 1e-12; 1e-9 leaves room for another summation order.  Every comparison prints its
largest deviation.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import hota_refs as H
import track_refs as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
TOL = 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = np.zeros((0, 4), dtype=np.float32)


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def _pad(seqs, F=None, cap=None):
    """list (sequence) of hota_refs frames -> the padded arrays of one call, ids renumbered per sequence in order of first appearance (the reference's
    numbering).  Behind a frame's boxes: NaN coordinates and id 0 (a VALID id: an over-read of the count shows)."""
    S = len(seqs)
    F = F or max([len(q) for q in seqs] + [1])
    cap = cap or max([max(len(fr[1]), len(fr[3])) for q in seqs for fr in q] + [1])
    a = {"gb": np.full((S, F, cap, 4), NAN, np.float32), "gi": np.zeros((S, F, cap), np.int32), "gc": np.zeros((S, F), np.int32),
         "tb": np.full((S, F, cap, 4), NAN, np.float32), "ti": np.zeros((S, F, cap), np.int32), "tc": np.zeros((S, F), np.int32), "NG": 0, "NT": 0}
    for s, q in enumerate(seqs):
        gmap, tmap = {}, {}
        for f, (gb, gi, tb, ti) in enumerate(q):
            a["gb"][s, f, :len(gi)] = np.asarray(gb, np.float32).reshape(-1, 4)
            a["tb"][s, f, :len(ti)] = np.asarray(tb, np.float32).reshape(-1, 4)
            a["gi"][s, f, :len(gi)] = [gmap.setdefault(int(i), len(gmap)) for i in gi]
            a["ti"][s, f, :len(ti)] = [tmap.setdefault(int(i), len(tmap)) for i in ti]
            a["gc"][s, f], a["tc"][s, f] = len(gi), len(ti)
        a["NG"], a["NT"] = max(a["NG"], len(gmap)), max(a["NT"], len(tmap))
    return a


def _call(a, dev):
    from v2x_sim_amd import ops
    t = [torch.from_numpy(a[k]).to(dev) for k in ("gb", "gi", "gc", "tb", "ti", "tc")]
    return ops.hota_sequences(*t, a["NG"], a["NT"])


def _run(seqs, dev, **kw):
    out_i, out_f = _call(_pad(seqs, **kw), dev)
    return out_i.cpu().numpy(), out_f.cpu().numpy()


def _same(out_i, out_f, s, ref, what=""):
    """Row s of a call against score_sequence's record.  -> the largest deviation of the four float fields."""
    for k, name in enumerate(("TP", "FN", "FP")):
        assert out_i[s, :, k].tolist() == ref[name].tolist(), "%s sequence %d %s:\n kernel    %s\n reference %s" % (what, s, name, out_i[s, :, k], ref[name])
    dev = 0.0
    for k, name in enumerate(("AssA", "AssRe", "AssPr")):
        dev = max(dev, float(np.abs(out_f[s, :, k] - ref[name]).max()))
    tp1 = np.maximum(1, ref["TP"])
    dev = max(dev, float(np.abs(out_f[s, :, 3] / tp1 - ref["loc"] / tp1).max()))
    print("%s sequence %d: TP %d .. %d, largest deviation %.3g" % (what, s, ref["TP"].min(), ref["TP"].max(), dev))
    assert dev <= TOL, (what, s, dev)
    return dev


def _kept(frames):
    ref = H.score_sequence(frames)
    assert H.is_kept(frames, ref), "the case is a coin flip: choose another"
    return ref


def _box(cx, cy, w=4.0, h=2.0):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]


def _scene(seed, present_gt, present_trk, n_obj=6, jitter=0.3):
    """Objects on a 10 m grid drifting slowly; frame f holds the ground truth of the objects in present_gt[f] and jittered tracks (id = 100 + object) of
    those in present_trk[f]."""
    rng = np.random.default_rng(seed)
    c0 = np.stack([10.0 * np.arange(n_obj), rng.uniform(-3, 3, n_obj)], 1)
    frames = []
    for f, (pg, pt) in enumerate(zip(present_gt, present_trk)):
        c = c0 + 0.2 * f
        gb = np.array([_box(*c[o]) for o in pg], np.float32).reshape(-1, 4)
        tb = np.array([_box(*(c[o] + rng.uniform(-jitter, jitter, 2))) for o in pt], np.float32).reshape(-1, 4)
        frames.append((gb, list(pg), tb, [100 + o for o in pt]))
    return frames


# ---- batches against the reference ----------------------------------------------------------------------------------------------------------
def _batch(which):
    if which == "ragged":
        cut = H.case(2)[0][:1]                           # one frame: lengths 24, 24, 1 under one F
        return [H.case(0)[0], H.case(1)[0], cut], [H.case(0)[1], H.case(1)[1], _kept(cut)]
    n_obj, n_frames = (40, 30) if which == "wide" else (60, 12)
    frames, ref, kept = H.case(0, n_obj, n_frames)
    assert kept
    return [frames], [ref]


@pytest.mark.parametrize("which", ["ragged", "wide", "full"])
def test_batch_equals_the_reference(device, which):
    """ragged: S = 3, two 12 x 24 cases and one cut to a single frame.  wide: a 40 x 30 case, 71 track ids -- an id space beyond one wave, the id-indexed
    kernels tile it.  full: a 60 x 12 case, up to 57 tracks against 60 ground-truth boxes per frame.
    Measured on the MI355X: largest deviation 2.2e-16 in each of the three against the 1e-9 bound."""
    assert H.case(0)[2] and H.case(1)[2]
    seqs, refs = _batch(which)
    if which == "wide":
        assert refs[0]["n_trk_ids"] > 64
    out_i, out_f = _run(seqs, device)
    for s, ref in enumerate(refs):
        _same(out_i, out_f, s, ref, which)
        assert ref["TP"][0] > 0 and 0 < ref["AssA"][0] <= 1


def test_rectangular_both_ways_in_one_sequence(device):
    """Frames with more ground truth than tracks and frames with more tracks than ground truth: the matrix is stored [small][large] either way."""
    pg = [(0, 1, 2, 3, 4), (0, 1), (0, 1, 2, 3, 4, 5), (2,), (0, 1, 2)]
    pt = [(0, 2), (0, 1, 2, 3, 5), (1, 2, 3), (0, 1, 2, 3), (0, 1, 2)]
    frames = _scene(3, pg, pt)
    ref = _kept(frames)
    out_i, out_f = _run([frames], device)
    _same(out_i, out_f, 0, ref, "rectangular")
    assert ref["TP"][0] == 11 and ref["FN"][0] == 6 and ref["FP"][0] == 6


def test_exact_capacity_sixty_four_by_sixty_four(device):
    """One frame of exactly 64 x 64: 64 disjoint boxes on a grid, the tracks are the same boxes with small offsets under shuffled ids."""
    rng = np.random.default_rng(8)
    c = np.stack(np.meshgrid(np.arange(8), np.arange(8)), -1).reshape(-1, 2) * 10.0
    gb = np.array([_box(*p) for p in c], np.float32)
    order = rng.permutation(64)
    tb = np.array([_box(*(c[o] + rng.uniform(-0.5, 0.5, 2))) for o in order], np.float32)
    frames = [(gb, list(range(64)), tb, [int(o) + 500 for o in order])]
    ref = _kept(frames)
    out_i, out_f = _run([frames], device)
    assert out_i.shape == (1, 19, 3) and out_f.shape == (1, 19, 4)
    _same(out_i, out_f, 0, ref, "64 x 64")
    assert ref["TP"][0] == 64 and ref["TP"][-1] < 64


def test_empty_frames_and_sequences_leave_the_others_untouched(device):
    """A frame with ground truth only, a frame with tracks only, an all-empty sequence and a sequence without any track inside one batch: the FN / FP rules,
    and the ordinary sequence of the batch is bit-identical to itself scored alone."""
    lone = _scene(4, [(0, 1, 2), (0, 1), ()], [(), (0, 1), (0, 1, 2, 3)])      # ground truth only; both; tracks only
    no_trk = [(fr[0], fr[1], NONE, []) for fr in H.case(3)[0][:4]]
    plain = H.case(0)[0][:6]
    seqs = [lone, [], no_trk, plain]
    out_i, out_f = _run(seqs, device)
    refs = [_kept(lone), H.score_sequence([]), H.score_sequence(no_trk), _kept(plain)]
    for s, ref in enumerate(refs):
        _same(out_i, out_f, s, ref, "empties")
    assert out_i[0, 0].tolist() == [2, 3, 4] and out_i[0, -1, 1] == 5 - out_i[0, -1, 0]
    assert out_i[1].tolist() == [[0, 0, 0]] * 19 and not out_f[1].any()
    assert out_i[2].tolist() == [[0, 48, 0]] * 19 and not out_f[2].any()                # 4 frames x 12 objects missed
    alone_i, alone_f = _run([plain], device)
    assert np.array_equal(alone_i[0], out_i[3]) and np.array_equal(alone_f[0], out_f[3])
    only_gt = [(fr[0], fr[1], NONE, []) for fr in plain]                                # a call without any track id: kernels 2-4 have nothing to do
    oi, of = _run([only_gt], device)
    assert oi[0].tolist() == [[0, 72, 0]] * 19 and not of.any()
    only_trk = [(NONE, [], fr[2], fr[3]) for fr in plain]
    oi, of = _run([only_trk], device)
    n = sum(len(fr[3]) for fr in plain)
    assert oi[0].tolist() == [[0, 0, n]] * 19 and not of.any()


def test_determinism_and_independence_of_the_batch(device):
    """The same call twice gives identical outputs; a sequence scored alone (another F, cap and id-space padding) equals its rows in the batch bit for bit."""
    seqs, _ = _batch("ragged")
    wide = H.case(0, 40, 30)[0]
    a = _pad(seqs + [wide])
    i1, f1 = _call(a, device)
    i2, f2 = _call(a, device)
    assert torch.equal(i1, i2) and torch.equal(f1, f2)
    for s, q in enumerate(seqs + [wide]):
        ai, af = _call(_pad([q]), device)
        assert torch.equal(ai[0], i1[s]) and torch.equal(af[0], f1[s]), s


def test_hostile_values(device):
    """NaN and +-inf boxes read as similarity 0 and change nothing else; negative and oversized counts clamp; an id out of range makes that box absent.
    Value checks on results: every expectation is the reference on the input with the same boxes removed."""
    base = H.case(0)[0][:6]
    ref = _kept(base)
    # a ground-truth box and a track with non-finite coordinates in every frame: present (one more miss, one more false positive), similar to nothing
    bad_g = np.array([[NAN, 0, 4, 2], [0, 0, np.inf, 2], [-np.inf, -np.inf, np.inf, np.inf]], np.float32)
    bad_t = np.array([[0, NAN, 4, 2], [-np.inf, 0, 4, 2], [np.inf, np.inf, np.inf, np.inf]], np.float32)
    spiked = [(np.concatenate([fr[0], bad_g[f % 3][None]]), fr[1] + [900], np.concatenate([fr[2], bad_t[f % 3][None]]), fr[3] + [901]) for f, fr in enumerate(base)]
    out_i, out_f = _run([spiked], device)
    with np.errstate(invalid="ignore"):
        spiked_ref = H.score_sequence(spiked)
    _same(out_i, out_f, 0, spiked_ref, "non-finite boxes")
    assert np.array_equal(out_i[0, :, 0], ref["TP"]) and np.array_equal(out_i[0, :, 1], ref["FN"] + 6) and np.array_equal(out_i[0, :, 2], ref["FP"] + 6)
    assert np.abs(out_f[0, :, 0] - ref["AssA"]).max() <= TOL
    # counts: negative = an empty side; beyond cap = cap
    other = H.case(1)[0][:6]                              # at most 12 tracks per frame and exactly 12 ground-truth boxes: count = cap
    a = _pad([other])
    assert a["gb"].shape[2] == 12 and int(a["gc"].min()) == 12
    a["gc"][0, 1] = -7
    a["gc"][0, 2] = 1000
    a["tc"][0, 3] = -(2 ** 31)
    want = list(other)
    want[1] = (NONE, [], other[1][2], other[1][3])
    want[3] = (other[3][0], other[3][1], NONE, [])
    out_i, out_f = (t.cpu().numpy() for t in _call(a, device))
    _same(out_i, out_f, 0, _kept(want), "clamped counts")
    # ids out of range: the box is absent everywhere
    a = _pad([base])
    a["gi"][0, 0, 2] = a["NG"]
    a["gi"][0, 4, 5] = -1
    a["ti"][0, 2, 0] = a["NT"] + 1000
    a["ti"][0, 5, 1] = -(2 ** 31)
    want = [list(fr) for fr in base]
    for f, side, k in ((0, 0, 2), (4, 0, 5), (2, 2, 0), (5, 2, 1)):
        want[f][side] = np.delete(want[f][side], k, 0)
        want[f][side + 1] = [v for j, v in enumerate(want[f][side + 1]) if j != k]
    out_i, out_f = (t.cpu().numpy() for t in _call(a, device))
    _same(out_i, out_f, 0, _kept([tuple(fr) for fr in want]), "ids out of range")
    assert out_i[0, 0, 0] + out_i[0, 0, 1] == ref["TP"][0] + ref["FN"][0] - 2 and out_i[0, 0, 0] + out_i[0, 0, 2] == ref["TP"][0] + ref["FP"][0] - 2


def test_wrapper_refuses_bad_shapes(device):
    from v2x_sim_amd import ops
    a = _pad([H.case(0)[0][:2]])
    t = {k: torch.from_numpy(a[k]).to(device) for k in ("gb", "gi", "gc", "tb", "ti", "tc")}
    with pytest.raises(ValueError):
        ops.hota_sequences(t["gb"], t["gi"], t["gc"], t["tb"][:, :1], t["ti"], t["tc"], a["NG"], a["NT"])
    with pytest.raises(ValueError):
        ops.hota_sequences(t["gb"], t["gi"], t["gc"], t["tb"], t["ti"], t["tc"], a["NG"], a["NT"], alpha=torch.zeros(33, dtype=torch.float64, device=device))
    with pytest.raises(ValueError):
        ops.hota_sequences(t["gb"], t["gi"], t["gc"], t["tb"], t["ti"], t["tc"], -1, a["NT"])
    with pytest.raises(RuntimeError):
        ops.hota_sequences(t["gb"].cpu(), t["gi"], t["gc"], t["tb"], t["ti"], t["tc"], a["NG"], a["NT"])


# ---- the class ------------------------------------------------------------------------------------------------------------------------------
def _feed(metric, frames, dev):
    for gb, gi, tb, ti in frames:
        metric.update(torch.from_numpy(np.asarray(gb, np.float32).reshape(-1, 4)).to(dev), gi, torch.from_numpy(np.asarray(tb, np.float32).reshape(-1, 4)).to(dev), ti)


def _same_record(got, want, what):
    dev = 0.0
    for k in ("TP", "FN", "FP"):
        assert got["per_alpha"][k].tolist() == want[k].tolist(), (what, k)
    for k in H.FIELDS:
        dev = max(dev, float(np.abs(got["per_alpha"][k] - want[k]).max()))
        assert abs(got[k] - float(np.mean(want[k]))) <= TOL, (what, k)
    print("%s: largest deviation of the eight fields %.3g" % (what, dev))
    assert dev <= TOL, (what, dev)


def test_hota_class_sequences_ids_and_errors(device):
    from v2x_sim_amd.utils.mot_metrics import Hota
    b = np.array([_box(0, 0), _box(10, 0)], np.float32)
    odd = [(b, [1000, 7], b + np.float32(0.25), [7, 1000]), (b[:1], [1000], b[::-1].copy(), [-5, 7]), (b, [7, 1000], b[:1] + np.float32(0.5), [1000])]
    seqs = [H.case(0)[0], odd, H.case(1)[0][:5]]
    refs = [H.case(0)[1], _kept(odd), _kept(seqs[2])]
    m = Hota()
    for q in seqs[:-1]:
        _feed(m, q, device)
        m.new_sequence()
    _feed(m, seqs[2], device)                             # the open sequence counts without new_sequence()
    got = m.result()
    assert len(got["sequences"]) == 3 and np.array_equal(got["alphas"], H.ALPHAS)
    for s, ref in enumerate(refs):
        _same_record(got["sequences"][s], H.finalize(ref), "sequence %d" % s)
    _same_record(got, H.combine(refs), "combined")
    again = m.result()                                    # result() does not consume
    assert all(np.array_equal(again["per_alpha"][k], got["per_alpha"][k]) for k in got["per_alpha"])
    one = Hota()
    _feed(one, odd, device)
    _same_record(one.result(), H.finalize(refs[1]), "alone")
    empty = Hota().result()
    assert empty["sequences"] == [] and empty["LocA"] == 1.0 and empty["HOTA"] == 0.0 and empty["TP"] == 0.0
    dev_b = torch.from_numpy(b).to(device)
    with pytest.raises(ValueError):
        Hota().update(torch.zeros((65, 4), device=device), list(range(65)), dev_b, [0, 1])
    with pytest.raises(ValueError):
        Hota().update(dev_b, [3, 3], dev_b, [0, 1])
    with pytest.raises(ValueError):
        Hota().update(dev_b, [0, 1], dev_b, [4, 4])
    with pytest.raises(RuntimeError):
        Hota().update(torch.from_numpy(b), [0, 1], dev_b, [0, 1])
    with pytest.raises(RuntimeError):
        Hota().update(dev_b, [0, 1], torch.from_numpy(b), [0, 1])


# ---- the tool -------------------------------------------------------------------------------------------------------------------------------
def _write(path, frames, side):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        for f, fr in enumerate(frames):
            for (x1, y1, x2, y2), i in zip(np.asarray(fr[2 * side], np.float64).reshape(-1, 4), fr[2 * side + 1]):
                fh.write("%d,%d,%.9g,%.9g,%.9g,%.9g,1,-1,-1,-1\n" % (f + 1, i + 1, x1, y1, x2 - x1, y2 - y1))


def test_eval_track_end_to_end(device, tmp_path, capsys):
    """Text files written from two kept cases' ground truth and tracks, plus a ground-truth file without a tracker file: the combined row equals the
    references on what the tool's own parser reads -- hota_refs within 1e-9, track_refs.ClearMotRef's counts exactly and its MOTP within 1e-6 (the
    tolerance test_gpu_track.py uses for the same class)."""
    spec = importlib.util.spec_from_file_location("eval_track", os.path.join(ROOT, "tools", "track", "eval_track.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    gt_dir, trk_dir = str(tmp_path / "gt"), str(tmp_path / "trk")
    names = [os.path.join("agent0", "3.txt"), os.path.join("agent1", "3.txt"), os.path.join("agent1", "9.txt")]
    cases = [H.case(0)[0], H.case(1)[0], H.case(2)[0][:3]]
    for name, frames in zip(names, cases):
        _write(os.path.join(gt_dir, name), frames, 0)
    for name, frames in zip(names[:2], cases[:2]):
        _write(os.path.join(trk_dir, name), frames, 1)
    out_json = str(tmp_path / "scores.json")
    rec = mod.main(["--gt", gt_dir, "--trk", trk_dir, "--out", out_json])
    text = capsys.readouterr().out
    assert "no tracker file" in text and "COMBINED" in text and all(c in text for c in mod.COLUMNS)
    import json
    assert json.load(open(out_json)) == rec
    assert [r["name"] for r in rec["files"]] == sorted(names) and rec["files"][2]["note"].startswith("no tracker file")
    refs, clear = [], []
    for name in sorted(names):
        trk_path = os.path.join(trk_dir, name)
        parsed = mod.sequence_frames(mod.read_mot(os.path.join(gt_dir, name)), mod.read_mot(trk_path) if os.path.exists(trk_path) else {})
        frames = [(gb, gi, tb, ti) for gi, gb, ti, tb in parsed]
        ref = H.score_sequence(frames)
        assert H.is_kept(frames, ref), name
        refs.append(ref)
        c = R.ClearMotRef()
        for gb, gi, tb, ti in frames:
            c.update(gb, gi, tb, ti)
        clear.append(c)
    for row, ref, c in zip(rec["files"], refs, clear):
        want, cw = H.summary(H.finalize(ref)), c.result()
        assert all(abs(row[k] - want[k]) <= TOL for k in H.FIELDS), (row, want)
        assert row["IDSW"] == cw["IDSW"] and abs(row["MOTA"] - cw["MOTA"]) <= 1e-12 and abs(row["MOTP"] - cw["MOTP"]) <= 1e-6
    want = H.summary(H.combine(refs))
    got = rec["combined"]
    print({k: (got[k], want[k]) for k in H.FIELDS})
    assert all(abs(got[k] - want[k]) <= TOL for k in H.FIELDS)
    tp, fp, fn, idsw = (sum(getattr(c, k) for c in clear) for k in ("tp", "fp", "fn", "idsw"))
    assert tp > 250 and got["IDSW"] == idsw and abs(got["MOTA"] - (tp - fp - idsw) / (tp + fn)) <= 1e-12
    assert abs(got["MOTP"] - sum(c.iou_sum for c in clear) / tp) <= 1e-6
    assert 0.3 < got["HOTA"] < 0.8 and rec["files"][2]["HOTA"] == 0.0 and rec["files"][2]["LocA"] == 1.0

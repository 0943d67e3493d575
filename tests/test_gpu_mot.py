"""GPU tests of the batched CLEAR MOT and Identity families (csrc/mot_seq.hip through ops.mot_sequences; utils/mot_metrics.py::ClearIdentity and
hota_extras; tools/track/eval_track.py) against the float64 reference of tests/mot_refs.py.

On cases that survive the reference's coin-flip filter (mot_refs.is_kept) the eleven integers must be EQUAL and
|MOTP_sum - reference| <= (TP + 2) 2^-52 MOTP_sum: two fp64 sums of at most TP non-negative terms in different orders, plus one ulp on each term.
On the identity stress cases (groups of identical boxes) the ID counts and TP / FN / FP do not depend on how ties break and must be equal; IDSW,
MT / PT / ML and Frag do depend on it there and are not compared.  Every comparison prints its largest deviation.
"""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import hota_refs as H
import mot_refs as M

pytestmark = pytest.mark.gpu

NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = np.zeros((0, 4), dtype=np.float32)
ID_COLS = (0, 1, 2, 8, 9, 10)                           # TP, FN, FP, IDTP, IDFN, IDFP: tie-independent on the stress cases


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def _pad(seqs, NG=None, NT=None):
    """list (sequence) of frames -> the padded arrays of one call, ids renumbered per sequence in order of first appearance (the reference's numbering).
    Behind a frame's boxes: NaN coordinates and id 0 (a VALID id: an over-read of the count shows)."""
    S = len(seqs)
    F = max([len(q) for q in seqs] + [1])
    cap = max([max(len(fr[1]), len(fr[3])) for q in seqs for fr in q] + [1])
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
    if NG is not None:
        a["NG"], a["NT"] = NG, NT
    return a


def _call(a, dev, thr=0.5):
    from v2x_sim_amd import ops
    t = [torch.from_numpy(a[k]).to(dev) for k in ("gb", "gi", "gc", "tb", "ti", "tc")]
    return ops.mot_sequences(*t, a["NG"], a["NT"], thr=thr)


def _run(seqs, dev, **kw):
    out_i, out_f = _call(_pad(seqs, **kw), dev)
    assert out_i.shape == (len(seqs), 11) and out_i.dtype == torch.int32 and out_f.shape == (len(seqs), 1) and out_f.dtype == torch.float64
    return out_i.cpu().numpy(), out_f.cpu().numpy()


def _same(out_i, out_f, s, ref, what="", cols=range(11)):
    """Row s of a call against score_sequence's record.  -> |MOTP_sum - reference| / its bound."""
    got, want = [int(out_i[s, k]) for k in cols], [ref[M.COUNTS[k]] for k in cols]
    assert got == want, "%s sequence %d %s:\n kernel    %s\n reference %s" % (what, s, [M.COUNTS[k] for k in cols], got, want)
    dev, bound = abs(float(out_f[s, 0]) - ref["MOTP_sum"]), M.motp_bound(ref)
    print("%s sequence %d: %s, |MOTP_sum - reference| %.3g (bound %.3g)" % (what, s, dict(zip(M.COUNTS, out_i[s].tolist())), dev, bound))
    assert dev <= bound, (what, s, dev, bound)
    return dev / bound if bound else 0.0


def _kept(frames):
    ref = M.score_sequence(frames)
    assert M.is_kept(frames, ref), "the case is a coin flip: choose another"
    return ref


def _box(cx, cy, w=4.0, h=2.0):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]


def _feed(metric, frames, dev):
    for gb, gi, tb, ti in frames:
        metric.update(torch.from_numpy(np.asarray(gb, np.float32).reshape(-1, 4)).to(dev), gi, torch.from_numpy(np.asarray(tb, np.float32).reshape(-1, 4)).to(dev), ti)


def _hand_gap_case(gap):
    """test_mot_refs_cpu's hand case: track 1 matched in frame 0; after the gap frame the closer track 2 wins, without it continuity keeps track 1."""
    gb = np.array([_box(0, 0)], np.float32)
    first = (gb, [0], np.array([_box(0, 0)], np.float32), [1])
    both = (gb, [0], np.array([_box(0.5, 0), _box(0.1, 0)], np.float32), [1, 2])
    return [first] + ([gap] if gap is not None else []) + [both]


# ---- batches against the reference ----------------------------------------------------------------------------------------------------------
def test_all_kept_cases_in_one_ragged_batch(device):
    """The sixteen hota_refs cases (12 x 24, 40 x 30 with more than 64 track ids, 60 x 12 with near-full frames) under one F, cap and id space.
    Measured on the MI355X: every integer equal; |MOTP_sum - reference| = 0 on all sixteen (both sides add the matched similarities in frame order, then
    slot order), against bounds of 4.1e-12 .. 8.9e-11."""
    kept = M.kept_cases()
    seqs, refs = [M.case(*c)[0] for c in kept], [M.case(*c)[1] for c in kept]
    out_i, out_f = _run(seqs, device)
    worst = max(_same(out_i, out_f, s, ref, "kept") for s, ref in enumerate(refs))
    print("largest |MOTP_sum - reference| / bound over %d sequences: %.3g" % (len(kept), worst))
    assert sum(r["IDSW"] for r in refs) > 0 and sum(r["Frag"] for r in refs) > 0 and min(r["TP"] for r in refs) > 0


def test_per_frame_clearmot_is_a_second_witness(device):
    """The same cases through the online class (one assignment launch per frame): TP, FP, FN and IDSW agree with the batched call."""
    from v2x_sim_amd.utils.mot_metrics import ClearMot
    kept = M.kept_cases()
    out_i, _ = _run([M.case(*c)[0] for c in kept], device)
    for s, c in enumerate(kept):
        cm = ClearMot()
        _feed(cm, M.case(*c)[0], device)
        assert (cm.tp, cm.fn, cm.fp, cm.idsw) == tuple(out_i[s, :4].tolist()), c


def test_a_sequence_alone_and_in_the_batch_is_bit_identical(device):
    """Another F, cap, id-space padding and orientation of the id matrix around the same sequence: the same bits; and the same call twice."""
    seqs = [M.case(0)[0], M.case(0, 40, 30)[0], M.stress_case(2)[0], M.case(0, 60, 12)[0], M.stress_case(1)[0]]
    a = _pad(seqs)
    i1, f1 = _call(a, device)
    i2, f2 = _call(a, device)
    assert torch.equal(i1, i2) and torch.equal(f1, f2)
    for s, q in enumerate(seqs):
        ai, af = _call(_pad([q]), device)
        assert torch.equal(ai[0], i1[s]) and torch.equal(af[0], f1[s]), s


def test_identity_stress_cases_in_one_batch(device):
    """Dense pmc with small integers, both orientations, the one-wave boundary (64 x 65) and an id space beyond two waves: the optimum, which
    largest-entry-first greedy misses on every case (test_mot_refs_cpu.py)."""
    cases = [M.stress_case(k) for k in range(len(M.STRESS))]
    out_i, out_f = _run([c[0] for c in cases], device)
    for s, (_, ref) in enumerate(cases):
        _same(out_i, out_f, s, ref, "stress %s" % (M.STRESS[s],), cols=ID_COLS)
        assert M.identity_greedy(ref["pmc"]) < ref["IDTP"]
    tall = [M.stress_case(k) for k in (2, 5)]                                           # alone: more ground-truth ids than track ids in the CALL
    out_i, out_f = _run([c[0] for c in tall], device)
    for s, (_, ref) in enumerate(tall):
        _same(out_i, out_f, s, ref, "tall", cols=ID_COLS)


def test_exact_capacity_sixty_four_by_sixty_four(device):
    """Frames of exactly 64 x 64: 64 disjoint boxes on a grid, the tracks are the same boxes with small offsets under shuffled ids; in the second frame
    eight tracks moved on to the next object's box."""
    rng = np.random.default_rng(8)
    c = np.stack(np.meshgrid(np.arange(8), np.arange(8)), -1).reshape(-1, 2) * 10.0
    gb = np.array([_box(*p) for p in c], np.float32)
    frames = []
    for f in range(2):
        order = rng.permutation(64)
        at = c[(order + (f == 1) * (order < 8)) % 64]
        tb = np.array([_box(*(p + rng.uniform(-0.3, 0.3, 2))) for p in at], np.float32)
        frames.append((gb, list(range(64)), tb, [int(o) + 500 for o in order]))
    ref = _kept(frames)
    out_i, out_f = _run([frames], device)
    _same(out_i, out_f, 0, ref, "64 x 64")
    assert ref["TP"] > 100 and ref["IDSW"] > 0


def test_id_space_padded_to_the_cap(device):
    """70 ground-truth ids and 56 track ids over 8 frames, scored under n_gt_ids = n_trk_ids = the cap: the reference's numbers; the ids of the padding
    (and the 14 objects no track follows are ML, nothing else is) do not count."""
    from v2x_sim_amd import ops_track
    rng = np.random.default_rng(21)
    c0 = np.stack([10.0 * (np.arange(70) % 10), 10.0 * (np.arange(70) // 10)], 1)
    frames = []
    for f in range(8):
        show = [o for o in range(70) if (o + f) % 7 != 0]                               # 60 of the 70 per frame
        trk = [o for o in show if o % 5 != 0]
        gb = np.array([_box(*(c0[o] + 0.2 * f)) for o in show], np.float32)
        tb = np.array([_box(*(c0[o] + 0.2 * f + rng.uniform(-0.3, 0.3, 2))) for o in trk], np.float32)
        frames.append((gb, show, tb, [100 + o for o in trk]))
    ref = _kept(frames)
    assert ref["n_gt_ids"] == 70 and ref["n_trk_ids"] == 56 and ref["ML"] == 14 and ref["MT"] == 56
    out_i, out_f = _run([frames], device, NG=ops_track.MOT_MAX_IDS, NT=ops_track.MOT_MAX_IDS)
    _same(out_i, out_f, 0, ref, "id cap")


def test_empties(device):
    plain = M.case(0)[0][:6]
    n_g, n_t = sum(len(fr[1]) for fr in plain), sum(len(fr[3]) for fr in plain)
    only_gt = [(fr[0], fr[1], NONE, []) for fr in plain]
    only_trk = [(NONE, [], fr[2], fr[3]) for fr in plain]
    gaps = [_hand_gap_case(None), _hand_gap_case((np.array([_box(0, 0)], np.float32), [0], NONE, [])), _hand_gap_case((NONE, [], NONE, [])),
            _hand_gap_case((NONE, [], np.array([_box(0, 0)], np.float32), [9]))]
    seqs = [only_gt, only_trk, [], plain] + gaps
    refs = [M.score_sequence(q) if s < 3 else _kept(q) for s, q in enumerate(seqs)]
    out_i, out_f = _run(seqs, device)
    for s, ref in enumerate(refs):
        _same(out_i, out_f, s, ref, "empties")
    assert out_i[0].tolist() == [0, n_g, 0, 0, 0, 0, 12, 0, 0, n_g, 0] and out_f[0, 0] == 0                # FN = IDFN = the boxes, ML = the 12 ids
    assert out_i[1].tolist() == [0, 0, n_t, 0, 0, 0, 0, 0, 0, 0, n_t] and out_f[1, 0] == 0                 # FP = IDFP
    assert not out_i[2].any() and out_f[2, 0] == 0
    assert out_i[4, 3] == 0 and out_i[4, 7] == 0 and [out_i[s, 3] for s in (5, 6, 7)] == [1, 1, 1] and [out_i[s, 7] for s in (5, 6, 7)] == [1, 1, 1]
    for q, want in ((only_gt, out_i[0]), (only_trk, out_i[1])):                          # a call without any id on one side: kernels 3 and 4 do not run
        oi, of = _run([q], device)
        assert np.array_equal(oi[0], want) and of[0, 0] == 0


def test_hostile_values(device):
    """NaN and +-inf boxes are present and similar to nothing; negative and oversized counts clamp; an id out of range makes that box absent.
    Every expectation is the reference on the input with the same boxes removed (non-finite: on the same input, its similarity reads as 0)."""
    base = M.case(0)[0][:6]
    ref = _kept(base)
    bad_g = np.array([[NAN, 0, 4, 2], [0, 0, np.inf, 2], [-np.inf, -np.inf, np.inf, np.inf]], np.float32)
    bad_t = np.array([[0, NAN, 4, 2], [-np.inf, 0, 4, 2], [np.inf, np.inf, np.inf, np.inf]], np.float32)
    spiked = [(np.concatenate([fr[0], bad_g[f % 3][None]]), fr[1] + [900], np.concatenate([fr[2], bad_t[f % 3][None]]), fr[3] + [901]) for f, fr in enumerate(base)]
    out_i, out_f = _run([spiked], device)
    with np.errstate(invalid="ignore"):
        spiked_ref = M.score_sequence(spiked)
    _same(out_i, out_f, 0, spiked_ref, "non-finite boxes")
    assert out_i[0, :4].tolist() == [ref["TP"], ref["FN"] + 6, ref["FP"] + 6, ref["IDSW"]] and out_i[0, 8] == ref["IDTP"] and out_i[0, 6] == ref["ML"] + 1
    # counts: negative = an empty side; beyond cap = cap
    other = M.case(1)[0][:6]
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
    assert out_i[0, 0] + out_i[0, 1] == ref["TP"] + ref["FN"] - 2 and out_i[0, 8] + out_i[0, 10] == ref["IDTP"] + ref["IDFP"] - 2


def test_wrapper_refuses_bad_arguments_before_any_launch(device):
    from v2x_sim_amd import ops, ops_track
    a = _pad([M.case(0)[0][:2]])
    t = {k: torch.from_numpy(a[k]).to(device) for k in ("gb", "gi", "gc", "tb", "ti", "tc")}
    args = (t["gb"], t["gi"], t["gc"], t["tb"], t["ti"], t["tc"])
    for ng, nt in ((ops_track.MOT_MAX_IDS + 1, a["NT"]), (a["NG"], ops_track.MOT_MAX_IDS + 1), (-1, a["NT"])):
        with pytest.raises(ValueError):
            ops.mot_sequences(*args, ng, nt)
    with pytest.raises(ValueError):
        ops.mot_sequences(t["gb"], t["gi"], t["gc"], t["tb"][:, :1], t["ti"], t["tc"], a["NG"], a["NT"])
    with pytest.raises(ValueError):
        ops.mot_sequences(*args, a["NG"], a["NT"], thr=NAN)
    with pytest.raises(RuntimeError):
        ops.mot_sequences(t["gb"].cpu(), t["gi"], t["gc"], t["tb"], t["ti"], t["tc"], a["NG"], a["NT"])
    out_i, _ = ops.mot_sequences(*args, ops_track.MOT_MAX_IDS, ops_track.MOT_MAX_IDS)    # the cap itself is served
    assert out_i[0, 0] > 0


# ---- the class ------------------------------------------------------------------------------------------------------------------------------
def _same_record(got, want, what):
    for k in M.COUNTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert abs(got["MOTP_sum"] - want["MOTP_sum"]) <= (want["TP"] + 2) * 2.0 ** -52 * want["MOTP_sum"], what
    for k in M.RATIOS:                                   # integer ratios are the same division; the two with MOTP_sum inherit its bound
        tol = (want["TP"] + 2) * 2.0 ** -52 * max(1.0, abs(want[k])) if k in ("MOTP", "sMOTA") else 0.0
        assert abs(got[k] - want[k]) <= tol, (what, k, got[k], want[k])


def test_clear_identity_class_sequences_ids_and_errors(device):
    from v2x_sim_amd.utils.mot_metrics import ClearIdentity, Hota
    b = np.array([_box(0, 0), _box(10, 0)], np.float32)
    odd = [(b, [1000, 7], b + np.float32(0.25), [7, 1000]), (b[:1], [1000], b[::-1].copy(), [-5, 7]), (b, [7, 1000], b[:1] + np.float32(0.5), [1000])]
    seqs = [M.case(0)[0], odd, M.case(1)[0][:5]]
    refs = [M.case(0)[1], _kept(odd), _kept(seqs[2])]
    m, h = ClearIdentity(), Hota()
    for q in seqs[:-1]:
        _feed(m, q, device)
        _feed(h, q, device)
        m.new_sequence()
        h.new_sequence()
    _feed(m, seqs[2], device)                             # the open sequence counts without new_sequence()
    _feed(h, seqs[2], device)
    got = m.result()
    assert len(got["sequences"]) == 3
    for s, ref in enumerate(refs):
        _same_record(got["sequences"][s], M.finalize(ref), "sequence %d" % s)
    _same_record(got, M.combine(refs), "combined")
    assert m.result() == got                              # result() does not consume
    assert all(torch.equal(x, y) if torch.is_tensor(x) else x == y for x, y in zip(m.padded(), h.padded()))      # one padding
    empty = ClearIdentity().result()
    assert empty["sequences"] == [] and all(empty[k] == 0 for k in M.COUNTS + M.RATIOS)
    dev_b = torch.from_numpy(b).to(device)
    with pytest.raises(ValueError):
        ClearIdentity().update(torch.zeros((65, 4), device=device), list(range(65)), dev_b, [0, 1])
    with pytest.raises(ValueError):
        ClearIdentity().update(dev_b, [3, 3], dev_b, [0, 1])
    with pytest.raises(RuntimeError):
        ClearIdentity().update(torch.from_numpy(b), [0, 1], dev_b, [0, 1])


# ---- the tool -------------------------------------------------------------------------------------------------------------------------------
def _write(path, frames, side):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        for f, fr in enumerate(frames):
            for (x1, y1, x2, y2), i in zip(np.asarray(fr[2 * side], np.float64).reshape(-1, 4), fr[2 * side + 1]):
                fh.write("%d,%d,%.9g,%.9g,%.9g,%.9g,1,-1,-1,-1\n" % (f + 1, i + 1, x1, y1, x2 - x1, y2 - y1))


def test_eval_track_new_columns_end_to_end(device, tmp_path, capsys):
    """Text files written from two kept cases plus a ground-truth-only file: every column the batched scorer adds, per file and combined, against
    mot_refs on what the tool's own parser reads; the hota_extras fields against hota_refs; the JSON equals the returned record."""
    spec = importlib.util.spec_from_file_location("eval_track", os.path.join(ROOT, "tools", "track", "eval_track.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    gt_dir, trk_dir = str(tmp_path / "gt"), str(tmp_path / "trk")
    names = [os.path.join("agent0", "3.txt"), os.path.join("agent1", "3.txt"), os.path.join("agent1", "9.txt")]
    cases = [M.case(0)[0], M.case(1)[0], M.case(2)[0][:3]]
    for name, frames in zip(names, cases):
        _write(os.path.join(gt_dir, name), frames, 0)
    for name, frames in zip(names[:2], cases[:2]):
        _write(os.path.join(trk_dir, name), frames, 1)
    out_json = str(tmp_path / "scores.json")
    rec = mod.main(["--gt", gt_dir, "--trk", trk_dir, "--out", out_json])
    text = capsys.readouterr().out
    assert all(c in text for c in mod.COLUMNS) and all(c in mod.COLUMNS for c in ("IDF1", "IDR", "IDP", "MT", "ML", "Frag", "MOTA", "MOTP", "IDSW", "HOTA"))
    assert json.load(open(out_json)) == rec
    refs, hrefs = [], []
    for name in sorted(names):
        trk_path = os.path.join(trk_dir, name)
        parsed = mod.sequence_frames(mod.read_mot(os.path.join(gt_dir, name)), mod.read_mot(trk_path) if os.path.exists(trk_path) else {})
        frames = [(gb, gi, tb, ti) for gi, gb, ti, tb in parsed]
        ref = M.score_sequence(frames)
        assert M.is_kept(frames, ref), name
        refs.append(ref)
        hrefs.append(H.score_sequence(frames))
    for row, ref, href in zip(rec["files"], refs, hrefs):
        _same_record(row, M.finalize(ref), row["name"])
        per = H.finalize(href)
        assert abs(row["OWTA"] - float(np.mean(np.sqrt(per["DetRe"] * per["AssA"])))) <= 1e-9 and abs(row["HOTA(0)"] - per["HOTA"][0]) <= 1e-9
        assert abs(row["LocA(0)"] - per["LocA"][0]) <= 1e-9 and abs(row["HOTALocA(0)"] - per["HOTA"][0] * per["LocA"][0]) <= 1e-9
    _same_record(rec["combined"], M.combine(refs), "combined")
    per = H.combine(hrefs)
    assert abs(rec["combined"]["OWTA"] - float(np.mean(np.sqrt(per["DetRe"] * per["AssA"])))) <= 1e-9
    lone = rec["files"][2]
    assert lone["IDFN"] == lone["FN"] == refs[2]["FN"] > 0 and lone["ML"] == 12 and lone["IDF1"] == 0.0 and lone["MOTA"] == 0.0
    assert rec["combined"]["IDTP"] > 250 and 0.3 < rec["combined"]["IDF1"] < 1.0

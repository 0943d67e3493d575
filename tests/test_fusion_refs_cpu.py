"""The float64 references of tests/fusion_refs.py, checked without a GPU -- against the fp32 oracle (oracle/coperception_ref.py) and the
committed golden vectors -- and every CONDITION the GPU sweep (tests/test_gpu_fusion_sweep.py) relies on, asserted on the reference alone
for every generated case: a case list that would make a GPU assertion vacuous fails here first."""
import os

import numpy as np
import pytest
import torch

import fusion_refs as FR
from oracle import coperception_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")
bf16r = FR.bf16r


# ------------------------------------------------------------------------------------------------------------------ warp + fuse
def test_warp_case_list_holds_every_required_item():
    """What the sweep must contain (extents, channel counts, agent counts, frame counts, forms, item lists, poses), ticked off here so that
    an edit of the list cannot silently drop one; every case's stated form is the one its shape is eligible for."""
    cs = FR.WARP_CASES
    assert len(cs) == len(set(cs)) and len(cs) - len(FR._WARP_EDGE_CASES) >= 20
    ext = {(c.H, c.W) for c in cs}
    assert {(8, 8), (8, 24), (40, 16), (24, 56), (64, 64), (16, 16), (128, 128), (12, 20), (32, 32)} <= ext
    assert any(c.H % 8 or c.W % 8 for c in cs)
    assert {8, 24, 48, 128, 256, 384, 512} <= {c.C for c in cs}
    assert {(64, 64, 128), (16, 16, 512)} <= {(c.H, c.W, c.C) for c in cs}
    assert {1, 2, 3, 6, 7, 32} <= {c.A for c in cs}
    assert 1 in {c.Bt for c in cs} and any(c.Bt % 8 for c in cs if c.Bt > 1)
    assert {"all", "ragged"} <= {c.items for c in cs}
    for c in cs:
        assert c.form == FR.warp_form_of(c.H, c.W, c.C), c
        # the conditions of csrc/warp_fuse.hip, spelled out: LDS forms H % 8 == W % 8 == 0 and C % 128 == 0; else C % 16 == 0 picks <2>
        lds = c.H % 8 == 0 and c.W % 8 == 0 and c.C % 128 == 0
        assert (c.form == "lds") == lds and (c.form == "direct<2>") == (not lds and c.C % 16 == 0) and (c.form == "direct<1>") == (not lds and c.C % 16 != 0)
        assert c.C % 8 == 0 and 1 <= c.A <= 32
    for form in ("direct<1>", "direct<2>", "lds"):
        assert sum(c.form == form for c in cs) >= 3, form
        assert sum(c.form == form for c in FR._WARP_EDGE_CASES) >= 3, form


def test_warp_cases_cover_every_hand_pose_and_special_row():
    """Every hand-made pose is met by an LDS case and by a direct case; every case with three or more outputs has the three special
    coefficient rows (ego coefficient 0, a single neighbour, all zeros), and the random part leaves zeros and non-zeros."""
    names = [n for n, _ in FR.hand_poses(32, 32)]
    assert len(names) == FR.N_HAND_POSES == 18
    seen = {"lds": set(), "direct": set()}
    for c in FR.WARP_CASES:
        feat, T, items, coef, used = FR.make_warp_case(c)
        seen["lds" if c.form == "lds" else "direct"].update(used)
        assert feat.shape == (c.A * c.Bt, c.C, c.H, c.W) and torch.equal(feat, bf16r(feat))
        assert T.shape == (c.Bt, c.A, c.A, 4, 4) and T.dtype == torch.float32 and bool(torch.isfinite(T).all())
        assert len(set(items)) == len(items) and all(0 <= a < c.A and 0 <= f < c.Bt for a, f in items)
        assert (len(items) == c.A * c.Bt) == (c.items == "all")
        if c.items == "ragged":
            assert items != sorted(items)
        assert coef.shape == (len(items), c.A) and bool((coef >= 0).all())
        if len(items) >= 3:
            assert int((coef[2] != 0).sum()) == 0                                      # count == 0
            if c.A > 1:
                assert coef[0, items[0][0]] == 0 and int((coef[0] != 0).sum()) >= 1   # the ego left out
                nz = torch.nonzero(coef[1]).flatten().tolist()
                assert len(nz) == 1 and nz[0] != items[1][0]                            # count == 1 on the warped branch
    assert seen["lds"] == set(names) and seen["direct"] == set(names)


def _warp_ref32_modes(feat, T, items, coef, A, Bt):
    """tests/test_gpu_stages.py::_warp_ref (the fp32 oracle's warp, fp32 accumulation) for the three modes in one pass."""
    C, H, W = feat.shape[1:]
    return FR.fuse_modes(feat, T, items, coef, A, Bt, lambda m, p: R.feature_transformation(m, p, (1, C, H, W)), torch.float32)


def test_fuse_modes_is_warp_ref():
    """The one-pass loop is the loop of test_gpu_stages._warp_ref, mode by mode, bit for bit (same warp, same accumulation order)."""
    c = FR.WarpCase("direct<2>", 12, 20, 16, 4, 2, "ragged", 7)
    feat, T, items, coef, _ = FR.make_warp_case(c)
    got = _warp_ref32_modes(feat, T, items, coef, c.A, c.Bt)
    for mode in (0, 1, 2):
        n_out = len(items)
        out = torch.zeros(n_out, c.C, c.H, c.W)
        for m, (ego, f) in enumerate(items):
            acc, cnt = torch.zeros(c.C, c.H, c.W), 0
            for j in range(c.A):
                cj = float(coef[m, j])
                if cj == 0:
                    continue
                cnt += 1
                v = feat[j * c.Bt + f] if j == ego else R.feature_transformation(feat[j * c.Bt + f], T[f, ego, j], (1, c.C, c.H, c.W))
                if mode == 2:
                    acc = v if cnt == 1 else torch.maximum(acc, v)
                else:
                    acc = acc + (v if mode == 1 else cj * v)
            out[m] = acc / cnt if (mode == 1 and cnt) else acc
        assert torch.allclose(got[mode], out, atol=1e-6, rtol=1e-6), mode
    assert torch.equal(FR.warp_fuse_ref64(feat, T, items, coef, c.A, c.Bt, 1), FR.warp_fuse_ref64_modes(feat, T, items, coef, c.A, c.Bt)[1])


@pytest.mark.parametrize("case", FR.WARP_CASES, ids=FR.warp_case_id)
def test_warp_ref64_vs_fp32_oracle(case):
    """After bf16 rounding the float64 reference and the fp32 oracle agree within the project's stage bar (atol 4e-3, rtol 2^-7:
    tests/test_gpu_stages.py::test_warp_fuse_vs_oracle) on every case of the sweep, in every mode; before rounding they are ~1e-4 apart
    at most, so the bar has room for the kernel's own fp32 rounding on top."""
    c = case
    feat, T, items, coef, _ = FR.make_warp_case(c)
    r64 = FR.warp_fuse_ref64_modes(feat, T, items, coef, c.A, c.Bt)
    r32 = _warp_ref32_modes(feat, T, items, coef, c.A, c.Bt)
    for mode in (0, 1, 2):
        a, b = r64[mode], r32[mode]
        assert bool(torch.isfinite(a).all())
        gap = float((a - b.double()).abs().max()) if a.numel() else 0.0
        # before rounding: measured <= 7.0e-5 over the list (128 x 128, MEAN / MAX).  The bound is the fp32 side's own error: sample positions
        # up to 128 px carry a few ulp (~3e-5 px) in each of the two resampling steps, times a map slope of up to ~8 per pixel (the difference
        # of two unit normals) -> ~5e-4 per source; a weighted sum of A sources grows with A.
        assert gap <= 1e-3 * max(1.0, c.A / 4.0), (FR.MODE_NAMES[mode], gap)
        assert torch.allclose(bf16r(b), bf16r(a.float()), atol=4e-3, rtol=2 ** -7), (FR.MODE_NAMES[mode], gap)
    if len(items) >= 3:
        assert float(r64[0][2].abs().max()) == 0 and float(r64[1][2].abs().max()) == 0 and float(r64[2][2].abs().max()) == 0   # the row of zeros


def test_warp_ref64_golden():
    g = np.load(os.path.join(GOLD, "warp_2agent.npz"))
    feat = torch.from_numpy(g["feat"])
    assert torch.equal(feat, bf16r(feat))
    got = FR.warp64(feat[1], torch.from_numpy(g["T"]))
    assert torch.allclose(got.float(), torch.from_numpy(g["warped"]), atol=1e-4, rtol=0)
    assert torch.allclose(bf16r(got.float()), bf16r(torch.from_numpy(g["warped"])), atol=4e-3, rtol=2 ** -7)
    assert torch.equal(FR.warp64(feat[0], torch.eye(4)).float(), feat[0])          # the identity pose: weights exactly 1 / 0


def test_warp_ref64_known_shifts():
    """Arithmetic anchors: a whole-pixel shift moves the image by exactly that many pixels (zeros shifted in), a quarter turn permutes it."""
    H, W = 8, 24
    img = bf16r(torch.randn(2, H, W, generator=torch.Generator().manual_seed(1)))
    hp = dict(FR.hand_poses(H, W))
    got = FR.warp64(img, hp["whole-pixel"])           # T = (+3 px, -2 px): the output pixel (x, y) samples (x + 3, y + 2) (the y translation is negated)
    want = torch.zeros(2, H, W, dtype=torch.float64)
    want[:, :H - 2, :W - 3] = img[:, 2:, 3:].double()
    assert torch.allclose(got, want, atol=1e-12)
    assert float(FR.warp64(img, hp["off-map"]).abs().max()) == 0 and float(FR.warp64(img, hp["1e6"]).abs().max()) == 0
    sq = bf16r(torch.randn(2, 16, 16, generator=torch.Generator().manual_seed(2)))
    quarter = FR.warp64(sq, dict(FR.hand_poses(16, 16))["yaw+pi/2"])
    assert torch.allclose(quarter, torch.rot90(sq.double(), 1, (1, 2)), atol=1e-9) or torch.allclose(quarter, torch.rot90(sq.double(), -1, (1, 2)), atol=1e-9)


def test_warp_fuse_entry_accepts_an_empty_item_list():
    """n_out = 0 returns before anything is launched -- also when the (empty) items / coef / out tensors of the caller have null data pointers,
    as torch's empty tensors do (found by this sweep: the null-pointer check used to come first and refused the call)."""
    import ctypes
    from v2x_sim_amd import _lib
    lib = _lib.load()
    some = ctypes.create_string_buffer(64)            # never read: the call returns before a launch
    p = ctypes.cast(some, ctypes.c_void_p)
    assert lib.v2x_warp_fuse(p, 3, 2, 16, 16, 128, p, None, 0, None, 1, None, None) == 0
    assert lib.v2x_warp_fuse(p, 3, 2, 16, 16, 128, p, None, 1, None, 1, None, None) == -22 and b"null pointer" in lib.v2x_last_error()
    assert lib.v2x_warp_fuse(None, 3, 2, 16, 16, 128, p, None, 0, None, 1, None, None) == -22


# ------------------------------------------------------------------------------------------------------------------ handshake
def _oracle_prob(keys, querys, w, b, A, Bt):
    attn = R.MIMOGeneralDotProductAttention(querys.shape[1], keys.shape[1])
    with torch.no_grad():
        attn.linear.weight.copy_(w)
        attn.linear.bias.copy_(b)
        key_mat = torch.stack([keys[Bt * i: Bt * (i + 1)] for i in range(A)], 1)
        query_mat = torch.stack([querys[Bt * i: Bt * (i + 1)] for i in range(A)], 1)
        return attn.scores(query_mat, key_mat)


def test_attn_case_list_holds_every_required_item():
    shapes = {(c.A, c.Bt, c.K, c.Q) for c in FR.ATTN_CASES if c.scale == 1 and not c.tie}
    assert {(5, 2, 1024, 32), (1, 3, 1024, 32), (6, 3, 1024, 32), (8, 2, 1024, 32), (9, 2, 1024, 32), (32, 1, 256, 32), (5, 2, 1000, 24),
            (7, 2, 100, 48), (2, 4, 64, 8)} <= shapes
    assert {30.0, 300.0} <= {c.scale for c in FR.ATTN_CASES if (c.A, c.Bt, c.K, c.Q) == (5, 2, 1024, 32)}
    assert any(c.thres == 0.05 for c in FR.ATTN_CASES)
    ties = [c for c in FR.ATTN_CASES if c.tie]
    assert len(ties) >= 2 and all(c.tie[0] < c.tie[1] for c in ties)
    assert any(c.Q == 32 and c.A <= 8 for c in ties) and any(c.Q != 32 or c.A > 8 for c in ties)     # both projection paths
    assert len({FR.attn_case_id(c) for c in FR.ATTN_CASES}) == len(FR.ATTN_CASES)


@pytest.mark.parametrize("index", range(len(FR.ATTN_CASES)), ids=[FR.attn_case_id(c) for c in FR.ATTN_CASES])
def test_attn_ref64_and_conditions(index):
    c = FR.ATTN_CASES[index]
    keys, querys, w, b = FR.make_attn_case(c, index)
    assert keys.shape == (c.A * c.Bt, c.K) and querys.shape == (c.A * c.Bt, c.Q) and w.shape == (c.K, c.Q) and b.shape == (c.K,)
    scores, prob, soft = FR.attn_handshake_ref64(keys, querys, w, b, c.A, c.Bt, "softmax")
    assert scores.dtype == torch.float64 and prob.shape == (c.Bt, c.A, c.A) and torch.equal(soft, prob)
    assert bool(torch.isfinite(prob).all()) and torch.allclose(prob.sum(1), torch.ones(c.Bt, c.A, dtype=torch.float64), atol=1e-12)
    # the conditions the GPU assertions rest on
    margin, gap, tie_ok = FR.attn_conditions(c, scores, prob)
    assert margin >= FR.ATTN_THRES_MARGIN, margin            # no probability within 1e-3 of the threshold: the selection is compared whole
    assert gap >= FR.ATTN_GAP, gap                            # the arg-max is decided by more than rounding
    assert tie_ok
    smax = float(scores.abs().max())
    if c.scale == 30.0:
        assert smax > 89.0                                    # expf overflows (fp32: x > 88.7) without the max subtraction
    if c.scale == 300.0:
        assert smax > 1000.0
    # against the fp32 oracle at the golden's bar, scaled as the GPU test scales it
    tol = 1e-5 * max(1.0, smax / 8.0)
    ref32 = _oracle_prob(keys, querys, w, b, c.A, c.Bt)
    assert float((ref32.double() - prob).abs().max()) <= tol / 3
    # the selections
    _, _, act = FR.attn_handshake_ref64(keys, querys, w, b, c.A, c.Bt, "activated", c.thres)
    assert torch.equal(act != 0, prob > c.thres) and torch.equal(act[act != 0], prob[act != 0])
    _, _, arg = FR.attn_handshake_ref64(keys, querys, w, b, c.A, c.Bt, "argmax_test")
    assert torch.equal(arg.sum(1), torch.ones(c.Bt, c.A, dtype=torch.float64)) and bool(((arg == 0) | (arg == 1)).all())
    m = R.When2com.__new__(R.When2com)
    m.agent_num = c.A
    if c.tie:
        k1, k2 = c.tie
        assert bool((arg[:, k1] == 1).all()) and bool((arg[:, k2] == 0).all())         # the first of the tied pair, for every query
        assert torch.equal(keys.view(c.A, c.Bt, -1)[k1], keys.view(c.A, c.Bt, -1)[k2])
    else:
        want, _ = R.When2com.coefficients(m, ref32, "argmax_test", False)
        assert torch.equal(arg.float(), want)
    want, _ = R.When2com.coefficients(m, ref32, "activated", False, thres=c.thres)
    assert torch.equal(act != 0, want != 0)


def test_attn_ref64_golden():
    g = np.load(os.path.join(GOLD, "attn_5x5.npz"))
    d = lambda k: torch.from_numpy(g[k])
    _, prob, act = FR.attn_handshake_ref64(d("keys"), d("querys"), d("w"), d("b"), 5, 2, "activated")
    assert torch.allclose(prob.float(), d("prob"), atol=1e-5)
    assert torch.allclose(act.float(), d("coef_activated"), atol=1e-5)
    _, _, arg = FR.attn_handshake_ref64(d("keys"), d("querys"), d("w"), d("b"), 5, 2, "argmax_test")
    assert torch.equal(arg.float(), d("coef_argmax"))


# ------------------------------------------------------------------------------------------------------------------ pixel-weighted fuse
def test_pixel_cases_and_ref64():
    cs = FR.PIXEL_CASES
    assert {(3, 5, 8, 16, 64, 4), (2, 6, 64, 64, 128, 1), (1, 32, 8, 8, 8, 2), (2, 3, 128, 128, 256, 1), (70, 2, 8, 8, 16, 1)} <= {tuple(c[:6]) for c in cs}
    assert any(c.smax == 20.0 for c in cs) and any(c.H * c.W * c.C // 8 > 65536 for c in cs) and any(c.S == 1 for c in cs)
    patterns = set()
    for i, c in enumerate(cs):
        if c.H * c.W * c.C * c.n * c.A > (1 << 24):
            scores, valid, maps = FR.make_pixel_case(c._replace(H=8, W=8), i)       # (the large cases: the generator's pattern on a small map)
        else:
            scores, valid, maps = FR.make_pixel_case(c, i)
        assert bool((valid[:, 0] == 1).all())                                        # the ego is always valid
        for row in valid:
            patterns.add("all" if bool(row.all()) else "ego" if int(row.sum()) == 1 else "middle")
        ref = FR.pixel_weighted_fuse_ref64(scores, valid, maps)
        e = torch.exp(scores[..., 0]) * valid.view(c.n, c.A, 1, 1)                   # test_pixel_weighted_fuse_vs_torch's fp32 statement
        r32 = ((e / e.sum(1, keepdim=True)).unsqueeze(-1) * maps).sum(1)
        assert bool(torch.isfinite(ref).all()) and torch.allclose(bf16r(r32), bf16r(ref.float()), atol=2e-3, rtol=2 ** -7)
        ego_only = [m for m in range(c.n) if int(valid[m].sum()) == 1]
        for m in ego_only:
            assert torch.equal(ref[m], maps[m, 0].double())
    assert patterns == {"all", "ego", "middle"}


# ------------------------------------------------------------------------------------------------------------------ seg argmax + confusion
def test_seg_cases_and_ref():
    cs = FR.SEG_CASES
    assert any(c.n_cls == 8 and c.n * c.H * c.W > 4096 * 256 * 4 and not c.offset for c in cs)        # the 8-class kernel loops
    assert any(c.n_cls != 8 and c.n * c.H * c.W > 2048 * 256 for c in cs)                              # the generic kernel loops
    assert {1, 64} <= {c.n_cls for c in cs} and any(c.n_cls == 8 and (c.n * c.H * c.W) % 4 for c in cs)
    assert {"logits", "label"} <= {c.offset for c in cs if c.n_cls == 8 and (c.n * c.H * c.W) % 4 == 0}
    for i, c in enumerate(cs):
        small = c if c.n * c.H * c.W <= (1 << 18) else c._replace(n=1, H=128, W=128)                  # the generator's statistics on a smaller map
        logits, label = FR.make_seg_case(small, i)
        pred, conf = FR.argmax_confusion_ref(logits, label, c.n_cls)
        assert torch.equal(pred, logits.argmax(-1))                                                     # torch.argmax: the first maximum as well
        keep = label < c.n_cls
        assert torch.equal(conf, R.confusion_matrix(pred[keep], label[keep], c.n_cls)) and int(conf.sum()) == int(keep.sum())
        assert 0 < int(keep.sum()) < label.numel()                                                      # ignore labels are present
        if c.n_cls > 1 and small.n * small.H * small.W >= 1024:
            top = logits.topk(2, dim=-1).values
            assert int((top[..., 0] == top[..., 1]).sum()) > 0                                          # exact ties at the maximum exist
        assert FR.argmax_confusion_ref(logits, None, c.n_cls)[1] is None
    # first maximum wins, by hand
    lg = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 0.0, -1.0]])
    pred, conf = FR.argmax_confusion_ref(lg, torch.tensor([1, 7, 2], dtype=torch.uint8), 4)
    assert pred.tolist() == [1, 0, 0] and int(conf[1, 1]) == 1 and int(conf[2, 0]) == 1 and int(conf.sum()) == 2

"""tests/train_refs.py without a GPU: (1) every backward reference equals torch.autograd of its float64 forward, (2) every case table
reaches the kernel form / the side of the block cap it claims -- the plans are recomputed from the constants of the sources, each mirror names
the lines it restates -- (3) the exact-integer cases are exact in fp32 whatever the order of the sums, (4) the conditions the assertions of
tests/test_gpu_train_sweep.py rest on: rounding an fp32 evaluation to bf16 instead of the float64 one changes at most 5e-4 of a case's
elements, and at most 5e-5 of a BN case's elements sit within 1e-5 of the ReLU kink."""
import functools

import pytest
import torch
import torch.nn.functional as F

import train_refs as R

F64 = torch.float64


def rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# ------------------------------------------------------------------------------------------------------------------ references against autograd
def test_wgrad_ref_equals_autograd():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 8, 32, 32, generator=g, dtype=F64)
    dy = torch.randn(2, 8, 32, 64, generator=g, dtype=F64)
    w = torch.zeros(64, 32, 3, 3, dtype=F64, requires_grad=True)
    F.conv2d(x.permute(0, 3, 1, 2), w, None, 1, 1).backward(dy.permute(0, 3, 1, 2))
    assert rel(R.wgrad_ref64(x, dy), w.grad) < 1e-12
    # a delta image and a delta gradient pick single taps out (the orientation of ky, kx)
    x0, d0 = torch.zeros(1, 8, 32, 32), torch.zeros(1, 8, 32, 64)
    x0[0, 0, 0, 3] = d0[0, 1, 1, 6] = 1.0
    want = torch.zeros(64, 32, 3, 3, dtype=F64)
    want[6, 3, 0, 0] = 1.0
    assert torch.equal(R.wgrad_ref64(x0, d0), want)


@pytest.mark.parametrize("relu", [False, True])
def test_bn_ref_equals_autograd(relu):
    g = torch.Generator().manual_seed(2)
    M, C = 333, 16
    x = (torch.randn(M, C, generator=g, dtype=F64) * 0.7 + 0.2).requires_grad_(True)
    dy = torch.randn(M, C, generator=g, dtype=F64)
    gamma = (0.5 + torch.rand(C, generator=g, dtype=F64)).requires_grad_(True)
    beta = (0.3 * torch.randn(C, generator=g, dtype=F64)).requires_grad_(True)
    rm, rv = torch.randn(C, generator=g, dtype=F64), 0.5 + torch.rand(C, generator=g, dtype=F64)
    ref = R.bn_ref64(x.detach(), dy, gamma.detach(), beta.detach(), 1e-5, 0.1, rm, rv, relu)
    y = F.batch_norm(x, rm, rv, gamma, beta, True, 0.1, 1e-5)            # updates rm, rv in place
    if relu:
        assert float(y.detach().abs().min()) > 1e-9                      # away from the kink the formulas are exact
        y = F.relu(y)
    y.backward(dy)
    for name, want in (("y", y.detach()), ("dx", x.grad), ("dgamma", gamma.grad), ("dbeta", beta.grad), ("rm", rm), ("rv", rv),
                       ("mean", x.detach().mean(0)), ("invstd", 1 / torch.sqrt(x.detach().var(0, unbiased=False) + 1e-5))):
        assert rel(ref[name], want) < 1e-12, name


@pytest.mark.parametrize("dim", [1, -1])
def test_gru_gates_ref_equals_autograd(dim):
    g = torch.Generator().manual_seed(3)
    shape = (3, 15, 4, 6) if dim == 1 else (40, 15)
    gi = (torch.randn(shape, generator=g, dtype=F64) * 2).requires_grad_(True)
    bhh = (torch.randn(15, generator=g, dtype=F64) * 0.5).requires_grad_(True)
    dshape = list(shape)
    dshape[dim] = 5
    dh = torch.randn(dshape, generator=g, dtype=F64)
    ref = R.gru_gates_ref64(gi.detach(), bhh.detach(), dh, dim)
    bs = [1] * len(shape)
    bs[dim] = -1
    i_r, i_z, i_n = gi.chunk(3, dim)
    h_r, h_z, h_n = (t.reshape(bs) for t in bhh.chunk(3))
    r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
    n = torch.tanh(i_n + r * h_n)
    h = n - z * n
    h.backward(dh)
    assert rel(ref["h"], h.detach()) < 1e-12 and rel(ref["dgi"], gi.grad) < 1e-12 and rel(ref["dbhh"], bhh.grad) < 1e-12


@pytest.mark.parametrize("H,W", [(16, 48), (5, 7)])
def test_warp_matrix_is_grid_sample_and_its_transpose_is_autograd(H, W):
    """Per pose: the dense operator reproduces F.grid_sample in float64, and the explicit gather over its weights is autograd's backward."""
    g = torch.Generator().manual_seed(4)
    poses = R.warp_poses(H, W)
    th = torch.stack([t for _, t in poses])
    P, C = len(poses), 3
    x = torch.randn(P, C, H, W, generator=g, dtype=F64).requires_grad_(True)
    d = torch.randn(P, C, H, W, generator=g, dtype=F64)
    y = R.warp_affine_ref64(x, th)
    gx, = torch.autograd.grad(y, x, d)
    gt = R.warp_affine_transpose_ref64(d, th)
    for p, (name, t) in enumerate(poses):
        S = R.warp_matrix64(t, H, W)
        fwd = (S @ x.detach()[p].reshape(C, -1).t()).t().reshape(C, H, W)
        scale = max(float(y.detach()[p].abs().max()), 1.0)
        assert float((fwd - y.detach()[p]).abs().max()) <= 1e-12 * scale, name
        assert float((gt[p] - gx[p]).abs().max()) <= 1e-12 * max(float(gx[p].abs().max()), 1.0), name
    names = [n for n, _ in poses]
    assert float(y.detach()[names.index("one-width-out")].abs().max()) == 0.0
    col = y.detach()[names.index("one-column-left")]
    assert float(col[:, :, 1:].abs().max()) == 0.0 and float(col[:, :, 0].abs().min()) > 0.0           # one column in range
    half = R.warp_matrix64(poses[names.index("half-pixel")][1], H, W)
    assert float((half[half != 0] - 0.25).abs().max()) < 1e-6                                              # all four weights 1/4 (to the fp32 theta)
    assert R.warp_det(poses[names.index("reflect")][1], H, W) < 0
    assert 1e-6 < abs(R.warp_det(poses[names.index("det>1e-6")][1], H, W)) < 1e-5
    assert 0 < abs(R.warp_det(poses[names.index("det<1e-6")][1], H, W)) < 1e-6
    assert abs(R.warp_det(poses[names.index("rank1")][1], H, W)) < 1e-9 and R.warp_det(poses[names.index("zero")][1], H, W) == 0.0
    assert abs(R.warp_det(poses[names.index("rot90")][1], H, W) - 1.0) < 1e-6 and abs(R.warp_det(poses[names.index("rot45")][1], H, W) - 1.0) < 1e-6


@pytest.mark.parametrize("index", [1, 3, 10])
def test_v2v_message_refs_equal_autograd(index):
    c = R.V2V_CASES[index]
    cur, base, T, d = R.make_v2v_case(c)
    b64 = base.to(F64).requires_grad_(True)
    c64 = cur.to(F64).requires_grad_(True) if c.two else b64
    out = R.v2v_message_ref64(c64, b64, T, c.A, c.B)
    out.backward(d.to(F64))
    dbase, dcur = R.v2v_message_bwd_ref64(d, T, c.A, c.B, c.two)
    assert rel(dbase, b64.grad) < 1e-12
    if c.two:
        assert rel(dcur, c64.grad) < 1e-12


@pytest.mark.parametrize("normalizer", ["positives", "batch"])
def test_det_loss_refs_equal_the_specification_and_autograd(normalizer):
    """det_loss_ref64 == train/loss.py::detection_loss evaluated in float64, and the written-out gradients == its autograd (inputs away from
    the smooth-L1 switch)."""
    from v2x_sim_amd.train.loss import detection_loss
    g = torch.Generator().manual_seed(5)
    n, maps = 600, 3
    cls = (torch.randn(n, 2, generator=g, dtype=F64) * 3).requires_grad_(True)
    loc = (torch.randn(n, 6, generator=g, dtype=F64) * 0.5).requires_grad_(True)
    tgt = torch.randn(n, 6, generator=g, dtype=F64) * 0.4
    lab = torch.zeros(n, 2, dtype=F64)
    lab[:, 1] = (torch.rand(n, generator=g) < 0.1).double()
    lab[:, 0] = 1 - lab[:, 1]
    lab[:20] = 0.0
    lab[20:40] = torch.tensor([0.3, 0.7], dtype=F64)
    mask = torch.rand(n, generator=g) < 0.3
    beta = 1.0 / 9.0
    assert float(((loc.detach() - tgt).abs() - beta).abs().min()) > 1e-9
    out = detection_loss({"cls": cls.view(maps, -1, 2), "loc": loc.view(maps, -1, 6)}, lab.view(maps, -1, 2), tgt.view(maps, -1, 6), mask.view(maps, -1, 1),
                         normalizer=normalizer)
    ref = R.det_loss_ref64(cls.detach(), lab, loc.detach(), tgt, mask, 0.25, beta, maps if normalizer == "batch" else None)
    for k, name in enumerate(("loss", "cls_loss", "loc_loss")):
        assert abs(float(out[k]) - float(ref[name])) <= 1e-12 * abs(float(ref[name])), name
    w = (1.0, 0.25, -0.5)
    (out[0] * w[0] + out[1] * w[1] + out[2] * w[2]).backward()
    dcls, dloc = R.det_loss_grads_ref64(cls.detach(), lab, loc.detach(), tgt, mask, 0.25, beta, ref["norm"], *w)
    assert rel(dcls, cls.grad) < 1e-12 and rel(dloc, loc.grad) < 1e-12
    dcls0, dloc0 = R.det_loss_grads_ref64(cls.detach(), lab, loc.detach(), tgt, mask, 0.25, beta, ref["norm"], None, 0.25, None)
    assert float(dloc0.abs().max()) == 0.0 and rel(dcls0 * (1.25 / 0.25), dcls) < 1e-12


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_ref_equals_torch_adam(wd):
    g = torch.Generator().manual_seed(6)
    p = torch.nn.Parameter(torch.randn(100, generator=g, dtype=F64))
    opt = torch.optim.Adam([p], lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    q, m, v = p.detach().clone(), torch.zeros(100, dtype=F64), torch.zeros(100, dtype=F64)
    for step in range(1, 5):
        gr = torch.randn(100, generator=g, dtype=F64)
        p.grad = gr.clone()
        opt.step()
        q, m, v = R.adam_ref64(q, gr, m, v, step, 3e-3, 0.9, 0.999, 1e-8, wd)
        assert rel(q, p.detach()) < 1e-12 and rel(m, opt.state[p]["exp_avg"]) < 1e-12 and rel(v, opt.state[p]["exp_avg_sq"]) < 1e-12


def test_exact_references_and_bf16_rounding():
    g = torch.Generator().manual_seed(7)
    lo, skip = R.grid_values((2, 3, 5, 8), g), R.grid_values((2, 6, 10, 16), g)
    lo_r, skip_r = lo.float().requires_grad_(True), skip.float().requires_grad_(True)
    cat = R.upcat_ref(lo_r, skip_r)
    assert torch.equal(cat.detach().to(torch.bfloat16), R.upcat_ref(lo, skip))
    d = R.grid_values(tuple(cat.shape), g)
    glo, gskip = torch.autograd.grad(cat, (lo_r, skip_r), d.float())
    dlo, dskip = R.upcat_backward_ref(d, 8)
    assert torch.equal(dlo, glo.to(torch.bfloat16)) and torch.equal(dskip.float(), gskip)       # the grid values make the four-term sums exact in fp32: one rounding
    z = R.zero_insert_ref(lo)
    assert torch.equal(z[:, ::2, ::2], lo) and float(z.float().abs().sum()) == float(lo.float().abs().sum())
    # one rounding float64 -> bf16: equals torch's cast wherever the value is an fp32 (no second rounding to hide)
    x = torch.randn(10000, generator=g)
    assert torch.equal(R.bf16r64(x.double()).float(), R.bf16r(x))
    tie = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=F64)      # above a tie, a tie (to even), a tie (to even: up)
    assert R.bf16r64(tie).tolist() == [1.0 + 2.0 ** -7, 1.0, 1.0 + 2.0 ** -6]
    assert R.ulp32(torch.tensor([1.0, 1.5, 0.75, 0.0], dtype=F64)).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -24, 2.0 ** -149]


# ------------------------------------------------------------------------------------------------------------------ the tables reach what they claim
def test_plan_mirrors_on_known_values():
    """Hand-computed values of the mirrors (so a typo in one cannot make a table 'reach' a form): bn_plan = bn_train.hip::bn_plan, the
    dx-sum grid = the `blocks` of v2x_bn_train_backward_dxsum and its workspace size, cs_blocks = bn_train.hip::cs_blocks, gates_plan =
    gru_train.hip::gates_plan, dl_blocks = det_loss.hip::dl_blocks, the backward grid = the launch in v2x_det_loss_backward, the wgrad splits =
    conv_wgrad.hip::v2x_conv3x3_wgrad_splits and the launch in v2x_conv3x3_wgrad."""
    assert R.bn_plan(7, 8) == (256, 1) and R.bn_plan(2048 * 256, 8) == (256, 2048) and R.bn_plan(2048 * 256 + 1, 8) == (512, 1025)
    assert R.bn_dxsum_blocks(2048 * 256 + 1, 8) == (2048, 2049) and R.bn_dxsum_blocks(2048, 2048) == (2048, 2048)
    assert R.cs_blocks(1, 8) == (1, 1) and R.cs_blocks(512 * 16 * 256, 8) == (512, 512) and R.cs_blocks(512 * 16 + 1, 2048) == (512, 513)
    assert R.gates_plan(256 * 32, 64) == (32, 256) and R.gates_plan(256 * 32 + 1, 64) == (64, 129) and R.gates_plan(1, 2048) == (1, 1)
    assert R.dl_blocks(1) == (1, 1) and R.dl_blocks(1024 * 2048) == (1024, 1024) and R.dl_blocks(1024 * 2048 + 1) == (1024, 1025)
    assert R.dl_bwd_blocks(4096 * 1024) == (4096, 4096) and R.dl_bwd_blocks(4096 * 1024 + 1) == (4096, 4097)
    p = R.wgrad_plan(10, 128, 128, 64, 64)            # FaFNet's conv1: pairs 2 -> 192 splits over 640 tiles
    assert (p["pairs"], p["tiles"], p["n_split"], p["slots"], p["rows32"]) == (2, 640, 192, 192, False)
    p = R.wgrad_plan(3, 8, 32, 64, 96)
    assert (p["pairs"], p["tiles"], p["n_split"], p["slots"], p["rows32"]) == (6, 3, 3, 6, True)
    assert R.wgrad_plan(1, 8, 16, 32, 32) is None and R.wgrad_plan(1, 8, 32, 16, 32) is None
    assert [R.v2v_bwd_form(k) for k in (1, 4, 5, 8, 9)] == ["kmax4", "kmax4", "kmax8", "kmax8", "irregular"]
    assert all(R.chan8_ok(1, c) for c in R.C8_CHANNELS) and not R.chan8_ok(1, 24) and not R.chan8_ok(1, 4096) and not R.chan8_ok(0, 8)


def _count(pairs):
    n = {}
    for k in pairs:
        n[k] = n.get(k, 0) + 1
    return n


def test_wgrad_table_reaches_every_form():
    """conv_wgrad.hip::v2x_conv3x3_wgrad_splits: each case's tags are exactly what its plan says, and both row forms, one
    tile, the 256 clamp, ragged tile shares, a two-dimensional tile grid, cin_out < Cin and the exact-integer operands are each met twice;
    the reduce takes its vectorised form (cin_out % 4 == 0, v2x_conv3x3_wgrad_reduce) and its scalar form."""
    n = {}
    for c in R.WGRAD_CASES:
        p = R.wgrad_plan(c.N, c.H, c.W, c.Cin, c.Cout)
        assert p is not None, c
        tags = set()
        if p["tiles"] == 1:
            tags.add("tiles1")
        if p["pairs"] == 1 and p["want"] > 256 and p["tiles"] >= 256:
            assert p["n_split"] == 256
            tags.add("clamp256")
        if p["tiles"] % p["n_split"]:
            tags.add("ragged")
        if c.H // R.WG_TH > 1 and c.W // R.WG_TW > 1:
            tags.add("grid2d")
        if c.cin_out is not None and c.cin_out < c.Cin:
            tags.add("cin_out")
        assert tags == set(c.reach), (c, tags)
        for t in tags | {"rows32" if p["rows32"] else "rows64", "int" if c.exact else "randn",
                         "reduce4" if (c.cin_out or c.Cin) % 4 == 0 else "reduce1"}:
            n[t] = n.get(t, 0) + 1
        if c.exact:      # every partial sum is an integer below 2^24: exact in fp32 in any order
            assert 4 * c.N * c.H * c.W < 2 ** 24
    for t in ("tiles1", "clamp256", "ragged", "grid2d", "cin_out", "rows32", "rows64", "int", "randn", "reduce4", "reduce1"):
        assert n.get(t, 0) >= 2, (t, n)
    assert len({R.wgrad_case_id(c) for c in R.WGRAD_CASES}) == len(R.WGRAD_CASES)


def test_c8_tables_reach_both_sides_of_every_cap():
    """The BN, channel-sum and gates tables share tm_chan8_shape_ok's channel counts (train_math.h::tm_chan8_shape_ok).  For EVERY C: the rows 2, 7,
    rpp - 1 (where it exists), rpp + 1 and 1000, and one row count on each side of the family's cap:
      bn_plan (bn_train.hip::bn_plan): below, vec_per_block = 256 and >= 2045 workgroups; above, vec_per_block = 512 -- and the dx-sum grid
        (v2x_bn_train_backward_dxsum) uncapped below, capped at BN_DXSUM_MAX_BLOCKS above;
      cs_blocks (bn_train.hip::cs_blocks): uncapped below (<= 512 workgroups of >= 16 passes), capped above (a 17th pass begins);
      gates_plan (gru_train.hip::gates_plan): 256 workgroups of nsub rows below, rows_per_block = 2 nsub above."""
    for C in R.C8_CHANNELS:
        r = R.rpp(C)
        want = {2, 7, r + 1, 1000} | ({r - 1} if r > 1 else set())
        for name, table in (("bn", R.BN_CASES), ("cs", R.CS_CASES), ("gates", R.GATES_NHWC_CASES)):
            rows = {c.M: c for c in table if c.C == C and c.kind == "randn" or c.C == C and name == "cs"}
            assert want <= set(rows), (name, C, want - set(rows))
            if r > 1:
                assert rows[r - 1].reach == "rpp-"
            assert rows[r + 1].reach == "rpp+"
            lo = [c for c in rows.values() if c.reach == "cap-"]
            hi = [c for c in rows.values() if c.reach == "cap+"]
            assert len(lo) >= 1 and len(hi) >= 1, (name, C)
            for c in lo + hi:
                assert R.chan8_ok(c.M, c.C)
                below = c.reach == "cap-"
                if name == "bn":
                    per, nb = R.bn_plan(c.M, C)
                    capped, raw = R.bn_dxsum_blocks(c.M, C)
                    assert (per == 256 and nb >= 2045 and raw == capped) if below else (per == 512 and raw > capped == R.BN_DXSUM_MAX_BLOCKS), c
                    assert abs(c.M * (C // 8) - R.BN_MAX_BLOCKS * R.BN_THREADS) <= 3 * (C // 8)
                elif name == "cs":
                    capped, raw = R.cs_blocks(c.M, C)
                    assert (raw == capped == R.CS_MAX_BLOCKS) if below else (raw == capped + 1), c
                    assert abs(c.M - R.CS_MAX_BLOCKS * 16 * r) == 3
                else:
                    rpb, nb = R.gates_plan(c.M, C)
                    assert (rpb == r and nb == -(-c.M // r) >= R.GATES_MAX_BLOCKS - 1) if below else (rpb == 2 * r and nb == R.GATES_MAX_BLOCKS // 2 + 1), c
    # BN: both layouts of the partials and relu on / off on each side of the cap, at least twice each; the G >= 64 lane mapping of
    # bn_bwd_apply_kernel<true> (bn_train.hip, the `if (SUM)` block after the pixel loop) at G = 64, 128 and 256, each with row counts on both sides of one pass
    n = _count((c.reach, c.layout) for c in R.BN_CASES)
    assert all(n.get((s, t), 0) >= 2 for s in ("cap-", "cap+") for t in (0, 1)), n
    n = _count((c.reach, c.relu) for c in R.BN_CASES)
    assert all(n.get((s, t), 0) >= 2 for s in ("cap-", "cap+") for t in (False, True)), n
    n = _count((c.C, c.layout, c.relu) for c in R.BN_CASES)
    assert all(sum(v for k, v in n.items() if k[0] == C and k[1] == t) >= 2 and sum(v for k, v in n.items() if k[0] == C and k[2] == u) >= 2
               for C in R.C8_CHANNELS for t in (0, 1) for u in (False, True)), n
    assert {c.C // 8 for c in R.BN_CASES if c.C // 8 >= 64} == {64, 128, 256}
    ill = [c for c in R.BN_CASES if c.kind == "ill"]
    assert len(ill) >= 2
    for c in ill:
        x = R.make_bn_case(c)[0].double()
        ratio = (x.mean(0).abs() / x.std(0)).min()
        assert float(ratio) > 100, float(ratio)                       # mean / std ~ 125
    assert len({R.c8_case_id(c) for c in R.BN_CASES}) == len(R.BN_CASES)
    # cast_pad_chsum: every padded channel count, both sides of the cap at three of them, C < Cp with the last group half or wholly padding
    assert {c.Cp for c in R.CP_CASES} == set(R.C8_CHANNELS)
    n = _count(c.reach for c in R.CP_CASES)
    assert n.get("cap-", 0) >= 2 and n.get("cap+", 0) >= 2
    for c in R.CP_CASES:
        assert c.C % 4 == 0 and 0 < c.C <= c.Cp and R.chan8_ok(c.M, c.Cp)
        capped, raw = R.cs_blocks(c.M, c.Cp)
        if c.reach == "cap-":
            assert raw == capped == R.CS_MAX_BLOCKS
        if c.reach == "cap+":
            assert raw == capped + 1
    assert sum(1 for c in R.CP_CASES if c.C % 8 == 4) >= 2 and sum(1 for c in R.CP_CASES if c.C == c.Cp) >= 2 and sum(1 for c in R.CP_CASES if c.Cp - c.C >= 8) >= 2


def test_exact_integer_cases_are_exact():
    """Operands in -2 .. 2: the sum of the absolute values of the terms of any output element stays below 2^24, so every partial sum in every
    order is an integer fp32 holds exactly -- the kernel must equal the float64 reference bit for bit."""
    ints = [c for c in R.CS_CASES if c.kind == "int"]
    assert len(ints) >= 2 and {"cap-", "cap+"} <= {c.reach for c in ints}
    for c in ints:
        x = R.make_cs_case(c).float()
        assert torch.equal(x, x.round()) and float(x.abs().max()) <= 2 and float(x.abs().sum(0).max()) < 2 ** 24
    ints = [c for c in R.CP_CASES if c.kind == "int"]
    assert len(ints) >= 2 and {"cap-", "cap+"} <= {c.reach for c in ints}
    for c in ints:
        x = R.make_cp_case(c)
        assert torch.equal(x, x.round()) and float(x.abs().sum(0).max()) < 2 ** 24
    ints = [c for c in R.BN_CASES if c.kind == "int"]
    assert len(ints) >= 2 and {"cap-", "cap+"} <= {c.reach for c in ints}
    for c in ints:
        x = R.make_bn_case(c)[0].float()
        assert torch.equal(x, x.round()) and float(x.abs().sum(0).max()) < 2 ** 24 and float((x * x).sum(0).max()) < 2 ** 24
    ints = [c for c in R.WGRAD_CASES if c.exact]
    for c in ints:
        x, dy = R.make_wgrad_case(c)
        assert float(x.float().abs().max()) <= 2 and float(dy.float().abs().max()) <= 2 and torch.equal(x.float(), x.float().round())
    one_hot = [c for c in R.DET_CASES if "one-hot" in c.reach]
    assert len(one_hot) >= 2
    for c in one_hot:
        lab = R.make_det_case(c)[1]
        assert bool(((lab == 0) | (lab == 1)).all()) and c.n < 2 ** 24


def test_gates_f32_table():
    """v2x_gru_gates_f32 (gru_train.hip, its two kernels: one thread per float4 of a plane): H W = 4, H W = 4 x odd, C = 1, and the values the issue
    names -- pre-activations to +-90, exact zeros, gi + b = 0."""
    hw = [c.H * c.W for c in R.GATES_F32_CASES]
    assert all(v % 4 == 0 for v in hw) and hw.count(4) >= 2 and sum(1 for v in hw if v > 4 and (v // 4) % 2 == 1) >= 2
    assert sum(1 for c in R.GATES_F32_CASES if c.C == 1) >= 2
    for c in R.GATES_F32_CASES:
        gi, bhh, dh = R.make_gates_f32_case(c)
        assert float(gi.max()) == 90.0 and float(gi.min()) == -90.0
        assert bool((gi.view(c.P, 3 * c.C, -1)[:, :, 0] + bhh[None, :] == 0).all())
        assert int((gi == 0).sum()) >= 3 * c.C or c.H * c.W == 4 and c.P == 1
        ref = R.gru_gates_ref64(gi, bhh, dh, 1)
        assert all(bool(torch.isfinite(v).all()) for v in ref.values())


@functools.lru_cache(maxsize=None)
def _v2v_extent(index):
    """Largest candidate-box extent (train_math.h::tm_warp_candidates) over every pair and pixel of a case, both passes."""
    c = R.V2V_CASES[index]
    T = R.make_v2v_case(c)[2]
    worst = 0
    for (_, _, f, a, j) in R.v2v_pairs(c.A, c.B)[2]:
        for th in R.v2v_thetas(T[f, a, j]):
            worst = max(worst, *R.warp_box_extent(th.float(), c.H, c.W))
    return worst


def test_v2v_table_reaches_every_backward_form():
    """v2x_v2v_message_bwd_bf16 (v2v_train.hip lines 320-321: K <= 4 -> KMAX 4, else KMAX 8; line 152: K > KMAX -> irregular; lines 186 / 192:
    a candidate box wider than three -> irregular).  Neighbour counts 1, 4, 5, 8, 9; for each table form at least two cases in which EVERY
    workgroup walks the tables (no box wider than three anywhere) on a map whose pixel count is no multiple of VB_PIX, so the last, partial chunk
    runs it; K > 8 twice; a shrinking pose that overflows the tables with K <= 8 twice; C = 8 and 24, shared and separate cur / base, Bt > 1."""
    assert {c.A - 1 for c in R.V2V_CASES} >= {1, 4, 5, 8, 9}
    n = {}
    for i, c in enumerate(R.V2V_CASES):
        ext = _v2v_extent(i)
        form = R.v2v_bwd_form(c.A - 1)
        if c.shrink:
            assert c.A - 1 <= 8 and ext > 2 and c.form == "irregular", (c, ext)
            key = "overflow"
        elif form == "irregular":
            assert c.form == "irregular"
            key = "K>8"
        else:
            assert c.form == form
            key = form + ("-all-regular-partial-chunk" if ext <= 2 and (c.H * c.W) % R.VB_PIX else "")
        n[key] = n.get(key, 0) + 1
    for key in ("kmax4-all-regular-partial-chunk", "kmax8-all-regular-partial-chunk", "K>8", "overflow"):
        assert n.get(key, 0) >= 2, (key, n)
    assert {c.C for c in R.V2V_CASES} == {8, 24} and {c.two for c in R.V2V_CASES} == {False, True}
    assert sum(1 for c in R.V2V_CASES if c.B > 1) >= 2 and {(c.H, c.W) for c in R.V2V_CASES} >= {(5, 7), (9, 9)}


def test_v2v_plan_refuses_ragged_frames():
    """The message kernels take ONE neighbour count K for every item (v2v_train.hip: V2vMsgArgs.K), so a batch whose frames hold different
    numbers of agents has no plan: hip_graph._v2v_plan answers None and the stage runs on the fp32 graph.  The sweep therefore covers uniform
    plans (Bt > 1 included); this asserts the refusal, and that a uniform plan tabulates train_refs.v2v_pairs' enumeration."""
    from v2x_sim_amd.models.det.base import IntermediateModelBase
    from v2x_sim_amd.train import hip_graph

    class _M:
        pass
    A, B = 4, 2
    T = torch.zeros(B, A, A, 4, 4)
    counts, items, rows = IntermediateModelBase.frame_plan(torch.tensor([[4] * A, [3] * A]), B, A)
    assert hip_graph._v2v_plan(_M(), counts, items, rows, B, A, T, A * B, "cpu") is None
    counts, items, rows = IntermediateModelBase.frame_plan(torch.full((B, A), A), B, A)
    plan = hip_graph._v2v_plan(_M(), counts, items, rows, B, A, T, A * B, "cpu")
    ritems, rrows, pairs = R.v2v_pairs(A, B)
    assert plan["K"] == A - 1 and plan["M"] == len(ritems) and items == ritems and rows == rrows and plan["identity"]
    assert plan["src"].tolist() == [p[1] for p in pairs]
    assert plan["tsel"].tolist() == [(f * A + a) * A + j for (_, _, f, a, j) in pairs]


def test_det_and_adam_tables():
    """det_loss.hip::dl_blocks (lines 156-160) and the backward grid (lines 210-211): n = 1, 255, 257, both sides of the forward cap, the
    backward wrap, each at least twice; masks none / all / sparse; every incoming gradient present and absent.  adam.hip (line 14:
    ADAM_BLOCK_ELEMS = 4096; lines 58 / 81: whole blocks vectorised, the tail scalar): sizes around one block, steps 1 and 10^5, g = 0, both
    weight decays, host and device learning rates."""
    n = _count(t for c in R.DET_CASES for t in c.reach)
    for c in R.DET_CASES:
        capped, raw = R.dl_blocks(c.n)
        bcap, braw = R.dl_bwd_blocks(c.n)
        tags = set()
        if raw == capped == R.DL_MAX_BLOCKS and c.n == R.DL_MAX_BLOCKS * 2048 - 1:
            tags.add("fwd-")
        if raw > capped:
            tags.add("fwd+")
        if braw > bcap:
            tags.add("bwd+")
        assert tags == set(c.reach) - {"one-hot"}, (c, tags)
        assert c.n % c.n_maps == 0
    assert all(n.get(t, 0) >= 2 for t in ("fwd-", "fwd+", "bwd+", "one-hot")), n
    assert {c.n for c in R.DET_CASES} >= {1, 255, 257} and {c.mask for c in R.DET_CASES} == {"none", "all", "sparse"}
    assert {c.normalizer for c in R.DET_CASES} == {"positives", "batch"}
    for k in range(3):
        assert sum(1 for c in R.DET_CASES if c.grads[k] is None) >= 2 and sum(1 for c in R.DET_CASES if c.grads[k] is not None) >= 2
    c = R.DET_CASES[2]
    cls, lab, loc, tgt, mask = R.make_det_case(c)
    assert float(cls.max()) == 80.0 and float(cls.min()) == -80.0 and bool((cls[:, 0] == cls[:, 1]).any())
    pairs = {tuple(round(float(v), 4) for v in row) for row in lab}
    assert pairs == {(1.0, 0.0), (0.0, 1.0), (0.0, 0.0), (0.3, 0.7)}
    d = (loc - tgt)[0]
    b = torch.tensor(R.DET_BETA, dtype=torch.float32)
    assert float(d[0]) == float(b) and float(d[1]) < float(b) < float(d[2]) and float(d[3]) == 0.0 and float(d[2]) - float(d[1]) < 2e-8 and bool(mask[0])
    assert set(R.ADAM_SIZES) >= {4095, 4096, 4097, 1, 0} and R.ADAM_BLOCK_ELEMS == 4096
    assert {c.step for c in R.ADAM_CASES} >= {1, 100000} and {c.wd for c in R.ADAM_CASES} == {0.0, 0.01}
    assert {c.device_lr for c in R.ADAM_CASES} == {False, True} and sum(1 for c in R.ADAM_CASES if c.zero_grad) >= 2
    assert 1 - 0.999 ** 100000 == 1.0 and 1 - 0.9 ** 100000 == 1.0                   # bias corrections "near 1": exactly 1 in float64
    for c in R.ADAM_CASES:
        if c.zero_grad:
            for p, g, m, v in R.make_adam_case(c):
                q = R.adam_ref64(p, g, m, v, c.step, R.ADAM_LR, *R.ADAM_BETAS, R.ADAM_EPS, c.wd)[0]
                assert bool(torch.isfinite(q).all())
                if c.step == 1 and c.wd == 0:
                    assert torch.equal(q, p.double())                                 # update 0, no NaN at eps > 0


def test_warp_train_table():
    """warp_train.hip (line 16: WT_CCH = 16 channels per thread, lines 35 / 57: the tail chunk): C = 1, 16 and 20 on 16 x 48 and 5 x 7 maps
    (H != W, H W no multiple of the 256-thread block), one map per named pose."""
    assert {(c.C, c.H, c.W) for c in R.WARP_TRAIN_CASES} == {(C, H, W) for C in (1, 16, 20) for (H, W) in ((16, 48), (5, 7))}
    assert 20 % R.WT_CCH and 16 % R.WT_CCH == 0
    assert set(R.WARP_POSE_NAMES) >= {"identity", "whole-pixel", "half-pixel", "one-width-out", "one-column-left", "rot90", "rot45", "reflect", "shear-aniso",
                                      "zoom-in-8", "zoom-out-4", "rank1", "zero", "det>1e-6", "det<1e-6"}


# ------------------------------------------------------------------------------------------------------------------ conditions of the GPU assertions
FLIP_CAP = R.FLIP_CAP     # 5e-4; the GPU sweep tolerates 1e-3 per case
assert FLIP_CAP == 5e-4
KINK_CAP = 5e-5          # the GPU sweep tolerates 1e-4 per case


_flips = R.fp32_flips      # share of elements on which fp32-then-bf16 differs from float64-then-bf16


def test_bn_cases_double_rounding_and_kink_conditions():
    """(fp32 evaluation: train_refs.bn_f32_ops -- elementwise fp32 ops around torch.sum's reductions; see there why not F.batch_norm.)"""
    worst = {"y": 0.0, "dx": 0.0, "kink": 0.0}
    bad = []
    for c in R.BN_CASES:
        x, dy, gamma, beta, rm0, rv0 = R.make_bn_case(c)
        eps, mom = R.f32c(R.bn_eps(c)), R.f32c(R.BN_MOMENTUM)
        ref = R.bn_ref64(x, dy, gamma, beta, eps, mom, rm0, rv0, c.relu)
        y32, dx32 = R.bn_f32_ops(x, dy, gamma, beta, R.bn_eps(c), c.relu)
        kink = (ref["y0"].abs() < 1e-5) if c.relu else torch.zeros_like(ref["y0"], dtype=torch.bool)
        fy = _flips(y32, ref["y"])
        keep = ~kink
        fdx = float((R.bf16r(dx32).double()[keep] != R.bf16r64(ref["dx"])[keep]).double().sum()) / x.numel()
        ks = float(kink.double().mean())
        for k, v in (("y", fy), ("dx", fdx), ("kink", ks)):
            worst[k] = max(worst[k], v)
        if fy > FLIP_CAP or fdx > FLIP_CAP or ks >= KINK_CAP:
            bad.append((R.c8_case_id(c), fy, fdx, ks))
    print("BN: worst flip share y %.1e, dx %.1e; worst kink share %.1e" % (worst["y"], worst["dx"], worst["kink"]))
    assert not bad, bad


def test_gates_cases_double_rounding_condition():
    worst = {"h": 0.0, "dgi": 0.0}
    bad = []
    for c in R.GATES_NHWC_CASES:
        gi, bhh, dh = R.make_gates_nhwc_case(c)
        ref = R.gru_gates_ref64(gi, bhh, dh)
        f32 = R.gru_gates_f32(gi, bhh, dh)
        fh, fd = _flips(f32["h"], ref["h"]), _flips(f32["dgi"], ref["dgi"])
        worst["h"], worst["dgi"] = max(worst["h"], fh), max(worst["dgi"], fd)
        if fh > FLIP_CAP or fd > FLIP_CAP:
            bad.append((R.c8_case_id(c), fh, fd))
    print("gates: worst flip share h %.1e, dgi %.1e" % (worst["h"], worst["dgi"]))
    assert not bad, bad


def test_v2v_cases_double_rounding_condition():
    worst = {"msg": 0.0, "dbase": 0.0}
    bad = []
    assert sum(1 for c in R.V2V_CASES if c.signed) >= 3 and {c.form for c in R.V2V_CASES if c.signed} == {"kmax4", "kmax8", "irregular"}
    for c in R.V2V_CASES:
        if c.signed:         # judged with the existing test's bar alone, without the flip cap (train_refs.make_v2v_case)
            continue
        cur, base, T, d = R.make_v2v_case(c)
        ref = R.v2v_message_ref64(cur, base, T, c.A, c.B)
        dbase, _ = R.v2v_message_bwd_ref64(d, T, c.A, c.B, c.two)
        out32, gb32, gc32 = R.v2v_f32(cur, base, T, c.A, c.B, d)
        if not c.two:
            gb32 = gb32 + gc32
        fm, fb = _flips(out32[..., c.C:], ref[..., c.C:]), _flips(gb32, dbase)
        worst["msg"], worst["dbase"] = max(worst["msg"], fm), max(worst["dbase"], fb)
        if fm > FLIP_CAP or fb > FLIP_CAP:
            bad.append((R.v2v_case_id(c), fm, fb))
    print("v2v: worst flip share message %.1e, dbase %.1e" % (worst["msg"], worst["dbase"]))
    assert not bad, bad

"""float64 references and the seeded case lists for the fusion-stage kernels (v2x_warp_fuse, v2x_attn_handshake,
v2x_pixel_weighted_fuse, v2x_seg_argmax_confusion).  A plain helper module (as tests/iou_kats.py): tests/test_fusion_refs_cpu.py checks the
references and every condition the case lists must satisfy without a GPU, tests/test_gpu_fusion_sweep.py holds the kernels to them.

Every reference is the plain statement of the operation in torch.float64 on the CPU, fed the operands the kernel gets (bf16-rounded maps,
fp32 poses / keys / weights widened exactly)."""
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

WSUM, MEAN, MAX = 0, 1, 2                       # ops.V2X_FUSE_* (include/v2x_amd.h)
MODE_NAMES = {WSUM: "WSUM", MEAN: "MEAN", MAX: "MAX"}


def bf16r(x):
    return x.to(torch.bfloat16).to(torch.float32)


# ------------------------------------------------------------------------------------------------------------------ warp + fuse
def warp64(feat, pose):
    """oracle/coperception_ref.py::feature_transformation in float64: feat (C, H, W), pose (4, 4).  Rotate about the map centre, then
    translate by (4 T[0,3] / 128, -4 T[1,3] / 128) in normalised coordinates; align_corners=False, zeros padding, the intermediate image
    materialised (its zero padding and its smoothing are part of the operation)."""
    nb = feat.to(torch.float64).unsqueeze(0)
    p = pose.to(torch.float64)
    tx = (4 * p[0, 3]) / 128
    ty = -(4 * p[1, 3]) / 128
    z, o = torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64)
    theta_rot = torch.stack([torch.stack([p[0, 0], p[0, 1], z]), torch.stack([p[1, 0], p[1, 1], z])]).unsqueeze(0)
    theta_trans = torch.stack([torch.stack([o, z, tx]), torch.stack([z, o, ty])]).unsqueeze(0)
    grid_rot = F.affine_grid(theta_rot, size=nb.shape, align_corners=False)
    grid_trans = F.affine_grid(theta_trans, size=nb.shape, align_corners=False)
    rot = F.grid_sample(nb, grid_rot, mode="bilinear", padding_mode="zeros", align_corners=False)
    return F.grid_sample(rot, grid_trans, mode="bilinear", padding_mode="zeros", align_corners=False).squeeze(0)


def fuse_modes(feat, T, items, coef, A, Bt, warp, dtype):
    """The loop of tests/test_gpu_stages.py::_warp_ref for the three modes in one pass (each warped map is needed by all of them):
    the ego map unwarped, sources with coef == 0 skipped, WSUM = sum of coef * map, MEAN = sum / number of non-zero coefficients (no source:
    zeros), MAX = running maximum that the first source initialises.  `warp(map, pose)` is the resampler, `dtype` the accumulator's."""
    C, H, W = feat.shape[1:]
    out = {m: torch.zeros(len(items), C, H, W, dtype=dtype) for m in (WSUM, MEAN, MAX)}
    for m, (ego, f) in enumerate(items):
        acc_w = torch.zeros(C, H, W, dtype=dtype)
        acc_m = torch.zeros(C, H, W, dtype=dtype)
        acc_x = torch.zeros(C, H, W, dtype=dtype)
        cnt = 0
        for j in range(A):
            c = float(coef[m, j])
            if c == 0:
                continue
            cnt += 1
            v = feat[j * Bt + f].to(dtype) if j == ego else warp(feat[j * Bt + f], T[f, ego, j]).to(dtype)
            acc_w = acc_w + coef[m, j].to(dtype) * v
            acc_m = acc_m + v
            acc_x = v if cnt == 1 else torch.maximum(acc_x, v)
        out[WSUM][m] = acc_w
        out[MEAN][m] = acc_m / cnt if cnt else acc_m
        out[MAX][m] = acc_x
    return out


def warp_fuse_ref64_modes(feat, T, items, coef, A, Bt):
    return fuse_modes(feat, T, items, coef, A, Bt, warp64, torch.float64)


def warp_fuse_ref64(feat, T, items, coef, A, Bt, mode):
    """feat (A*Bt, C, H, W) the bf16-rounded maps, agent-major; T (Bt, A, A, 4, 4) fp32; items [(ego, frame)]; coef (n_out, A)
    -> (n_out, C, H, W) float64."""
    return warp_fuse_ref64_modes(feat, T, items, coef, A, Bt)[mode]


def pose(yaw, tx, ty):
    M = torch.eye(4)
    M[0, 0], M[0, 1], M[1, 0], M[1, 1] = math.cos(yaw), -math.sin(yaw), math.sin(yaw), math.cos(yaw)
    M[0, 3], M[1, 3] = tx, ty
    return M


def hand_poses(H, W):
    """The hand-made poses of a map of H x W pixels.  The translate step moves the image T[0,3] * W / 64 pixels in x and -T[1,3] * H / 64
    pixels in y, so a shift of (px, py) pixels is pose(0, 64 px / W, 64 py / H)."""
    def shift(px, py, yaw=0.0):
        return pose(yaw, 64.0 * px / W, 64.0 * py / H)
    made = [("identity", pose(0.0, 0.0, 0.0)),
            ("whole-pixel", shift(3, -2)),
            ("half-pixel", shift(0.5, 1.5)),
            ("+1e-3px", shift(1e-3, 1e-3)),
            ("-1e-3px", shift(-1e-3, -1e-3)),
            ("off-map", shift(2 * W + 1, -(2 * H + 1))),
            ("1e6", pose(0.0, 1e6, -1e6)),                       # the clamp in bilin_setup
            ("yaw+pi/2", pose(math.pi / 2, 0.0, 0.0)),
            ("yaw-pi/2", pose(-math.pi / 2, 0.0, 0.0)),
            ("yaw-pi", pose(math.pi, 0.0, 0.0)),
            ("yaw0.7", pose(0.7, 0.0, 0.0))]
    # the `special` list of tests/test_gpu_stages.py::test_warp_fuse_lds_form_bitwise_and_oracle (written for a 32 x 32 map; taken as it is)
    special = [pose(0.0, 2.0, -4.0), pose(0.0, 1e-3, -1e-3), pose(0.7, 0.0, 0.0), pose(0.0, 80.0, 3.0), pose(3.1, -31.0, 62.0),
               pose(0.0, 6.0, 6.0), pose(-1.2, 15.9999, -16.0001)]
    return made + [("special%d" % i, p) for i, p in enumerate(special)]


N_HAND_POSES = len(hand_poses(32, 32))

# form: the kernel the default dispatch takes ("direct<1>" = warp_fuse_kernel<1>, "direct<2>" = warp_fuse_kernel<2>, "lds" = the LDS-staged
# forms); items: "all" = every (ego, frame) pair, "ragged" = a shuffled subset
WarpCase = namedtuple("WarpCase", "form H W C A Bt items seed")


def warp_form_of(H, W, C):
    """The eligibility conditions of ops.warp_fuse / warp_fuse_impl (csrc/warp_fuse.hip) with the default WARP_LDS."""
    if H % 8 == 0 and W % 8 == 0 and C % 128 == 0:
        return "lds"
    return "direct<2>" if C % 16 == 0 else "direct<1>"


def warp_case_id(c):
    return "%s-%dx%dx%d-A%d-Bt%d-%s" % (c.form, c.H, c.W, c.C, c.A, c.Bt, c.items)


_WARP_EDGE_CASES = [
    WarpCase("direct<2>", 32, 32, 64, 5, 2, "all", 100),        # the anchor: test_warp_fuse_vs_oracle's shape
    WarpCase("lds", 32, 32, 256, 5, 3, "ragged", 101),          # the anchor of the LDS form
    WarpCase("lds", 8, 8, 128, 3, 1, "all", 102),               # one tile: every window hangs over two borders
    WarpCase("lds", 8, 24, 128, 2, 3, "all", 103),
    WarpCase("lds", 40, 16, 256, 3, 2, "all", 104),
    WarpCase("lds", 24, 56, 128, 6, 1, "all", 105),
    WarpCase("lds", 64, 64, 128, 6, 2, "ragged", 106),          # the layer-2 shape, six agents
    WarpCase("lds", 16, 16, 512, 5, 3, "all", 107),             # the layer-4 shape (blockIdx.z up to 3)
    WarpCase("lds", 128, 128, 128, 3, 1, "all", 108),
    WarpCase("lds", 16, 16, 384, 7, 1, "all", 109),
    WarpCase("lds", 8, 8, 128, 32, 1, "all", 110),              # 32 agents on a small map
    WarpCase("lds", 8, 24, 512, 3, 11, "ragged", 111),          # 11 frames: not a multiple of the 8 XCDs of the ordered launch
    WarpCase("lds", 32, 32, 256, 1, 3, "all", 112),             # a single agent: the ego copy alone
    WarpCase("direct<1>", 12, 20, 24, 3, 2, "all", 113),        # extents that are no multiple of 8
    WarpCase("direct<1>", 8, 8, 8, 7, 3, "ragged", 114),
    WarpCase("direct<1>", 24, 56, 24, 6, 2, "all", 115),
    WarpCase("direct<1>", 16, 16, 8, 1, 2, "all", 116),
    WarpCase("direct<2>", 40, 16, 48, 2, 5, "all", 117),
    WarpCase("direct<2>", 12, 20, 128, 3, 2, "all", 118),       # 128 channels, but the extents rule the LDS form out
    WarpCase("direct<2>", 64, 64, 48, 2, 1, "all", 119),
    WarpCase("direct<2>", 8, 8, 16, 32, 1, "all", 120),
]


def _random_warp_cases(n=21, seed=2024):
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        form = ("lds", "direct<1>", "direct<2>")[i % 3]
        if form == "lds":
            H, W, C = 8 * int(rng.integers(1, 7)), 8 * int(rng.integers(1, 7)), int(rng.choice([128, 256, 384]))
        elif form == "direct<1>":
            H, W, C = int(rng.integers(5, 41)), int(rng.integers(5, 41)), int(rng.choice([8, 24, 40, 56]))
        elif rng.integers(0, 2):
            H, W, C = int(rng.integers(5, 41)), int(rng.integers(5, 41)), int(rng.choice([16, 48, 64, 96]))
        else:                                            # LDS-sized channels on extents the LDS form does not take
            H, W, C = 8 * int(rng.integers(1, 6)) + int(rng.integers(1, 8)), int(rng.integers(5, 41)), int(rng.choice([128, 256]))
        A, Bt = int(rng.integers(1, 9)), int(rng.integers(1, 6))
        cases.append(WarpCase(form, H, W, C, A, Bt, "ragged" if (i % 2 and A * Bt >= 4) else "all", 1000 + i))
    return cases


WARP_CASES = _WARP_EDGE_CASES + _random_warp_cases()


def make_warp_case(c):
    """-> feat (A*Bt, C, H, W) fp32 holding bf16 values, T (Bt, A, A, 4, 4) fp32, items [(ego, frame)], coef (n_out, A) fp32, and the
    names of the hand-made poses the case uses.  The LAST frame carries the hand-made poses (walked from an offset that depends on the
    case, so that small agent counts do not all meet the same few), every other frame synthetic_poses.  One coefficient table serves
    the three modes (MEAN and MAX read only which entries are non-zero): random in [0.3, 1) with about a quarter zeros, then
    row 0: the ego coefficient 0;  row 1: exactly one non-zero entry, a neighbour's;  row 2: all zeros."""
    from v2x_sim_amd.utils.synthetic import synthetic_poses
    g = torch.Generator().manual_seed(c.seed)
    feat = bf16r(torch.randn(c.A * c.Bt, c.C, c.H, c.W, generator=g))
    T = torch.from_numpy(synthetic_poses(c.Bt, c.A, seed=c.seed))
    hand = hand_poses(c.H, c.W)
    used, k = [], (c.seed * 5) % len(hand)
    for i in range(c.A):
        for j in range(c.A):
            if i != j:
                T[c.Bt - 1, i, j] = hand[k % len(hand)][1]
                used.append(hand[k % len(hand)][0])
                k += 1
    items = [(a, f) for a in range(c.A) for f in range(c.Bt)]
    if c.items == "ragged":
        keep = [it for n, it in enumerate(items) if n % 3 != 1]
        perm = torch.randperm(len(keep), generator=g).tolist()
        items = [keep[p] for p in perm]
    coef = torch.rand(len(items), c.A, generator=g) * 0.7 + 0.3
    coef[torch.rand(len(items), c.A, generator=g) < 0.25] = 0
    if len(items) >= 3:
        if c.A > 1:
            coef[0, items[0][0]] = 0
            if not bool((coef[0] != 0).any()):
                coef[0, (items[0][0] + 1) % c.A] = 0.5
            coef[1] = 0
            coef[1, (items[1][0] + 1) % c.A] = 0.75
        coef[2] = 0
    return feat, T, items, coef, used


# ------------------------------------------------------------------------------------------------------------------ handshake
def attn_handshake_ref64(keys, querys, w, b, A, Bt, mode, thres=0.2):
    """keys (A*Bt, K), querys (A*Bt, Q) agent-major, w (K, Q), b (K,) -> scores, prob, coef, each (Bt, A_key, A_query) float64:
    scores[f][k][q] = key_{k,f} . (w query_{q,f} + b), prob = softmax over the keys, coef = prob ("softmax"), prob where prob > thres else 0
    ("activated"), or the one-hot of the FIRST maximal key ("argmax_test")."""
    k64 = keys.to(torch.float64).view(A, Bt, -1).transpose(0, 1)             # (Bt, A, K)
    q64 = querys.to(torch.float64).view(A, Bt, -1).transpose(0, 1)           # (Bt, A, Q)
    qp = q64 @ w.to(torch.float64).T + b.to(torch.float64)                    # (Bt, A, K)
    scores = k64 @ qp.transpose(1, 2)                                         # (Bt, k, q)
    prob = torch.softmax(scores, dim=1)
    if mode == "softmax":
        coef = prob.clone()
    elif mode == "activated":
        coef = prob * (prob > thres).to(torch.float64)
    elif mode == "argmax_test":
        arg = np.argmax(scores.numpy(), axis=1)                               # numpy: the first maximum
        coef = torch.zeros_like(prob)
        coef.scatter_(1, torch.from_numpy(arg).unsqueeze(1), 1.0)
    else:
        raise ValueError(mode)
    return scores, prob, coef


# scale: factor on the keys; tie: (k1, k2) two agents given bit-identical key vectors that win every query; thres: the 'activated' threshold
AttnCase = namedtuple("AttnCase", "A Bt K Q scale tie thres")
ATTN_CASES = [
    AttnCase(5, 2, 1024, 32, 1.0, None, 0.2),          # the anchor (tests/golden/attn_5x5.npz's shape)
    AttnCase(1, 3, 1024, 32, 1.0, None, 0.2),
    AttnCase(6, 3, 1024, 32, 1.0, None, 0.2),
    AttnCase(8, 2, 1024, 32, 1.0, None, 0.2),          # the two sides of the A <= 8 gate of the unrolled projection
    AttnCase(9, 2, 1024, 32, 1.0, None, 0.2),
    AttnCase(32, 1, 256, 32, 1.0, None, 0.2),
    AttnCase(5, 2, 1000, 24, 1.0, None, 0.2),          # the generic projection; K no multiple of 64
    AttnCase(7, 2, 100, 48, 1.0, None, 0.2),
    AttnCase(2, 4, 64, 8, 1.0, None, 0.2),
    AttnCase(5, 2, 1024, 32, 30.0, None, 0.2),         # max |score| ~ 2e2 and ~ 2.6e3: expf of an unshifted score overflows
    AttnCase(5, 2, 1024, 32, 300.0, None, 0.2),
    AttnCase(5, 2, 1024, 32, 1.0, None, 0.05),         # thres passed explicitly
    AttnCase(5, 2, 1024, 32, 1.0, (1, 3), 0.2),        # designed ties
    AttnCase(9, 2, 1024, 32, 1.0, (0, 8), 0.2),
    AttnCase(6, 3, 1000, 24, 1.0, (2, 5), 0.2),
]
ATTN_THRES_MARGIN = 1e-3       # every reference probability is at least this far from thres
ATTN_GAP = 1e-3                # top-two reference score gap per query >= ATTN_GAP * max(1, max |score|)  (except the designed tie itself)


def attn_case_id(c):
    return "A%d-Bt%d-K%d-Q%d%s%s%s" % (c.A, c.Bt, c.K, c.Q, "-x%g" % c.scale if c.scale != 1 else "", "-tie%d=%d" % c.tie if c.tie else "",
                                        "-thres%g" % c.thres if c.thres != 0.2 else "")


def attn_conditions(c, scores, prob):
    """-> (smallest |prob - thres|, smallest top-two score gap relative to max(1, max |score|), the designed tie holds).  In a tie case the
    second of the tied keys is left out of the gap (the pair is equal by design) and the tied pair must win every query."""
    margin = float((prob - c.thres).abs().min())
    s = scores.clone()
    tie_ok = True
    if c.tie:
        k1, k2 = c.tie
        tie_ok = bool(torch.equal(s[:, k1], s[:, k2])) and bool((s.max(1).values == s[:, k1]).all())
        s = torch.cat([s[:, :k2], s[:, k2 + 1:]], 1)
    if s.shape[1] < 2:
        gap = float("inf")
    else:
        top = s.topk(2, dim=1).values
        gap = float((top[:, 0] - top[:, 1]).min()) / max(1.0, float(scores.abs().max()))
    return margin, gap, tie_ok


def make_attn_case(c, index):
    """Input scale as tests/golden/make_golden.py::g_attn.  The case is drawn again (next seed) until every reference probability keeps
    ATTN_THRES_MARGIN from the threshold and every query's top-two gap is at least ATTN_GAP (tests/test_fusion_refs_cpu.py asserts both
    on what is returned)."""
    for attempt in range(64):
        g = torch.Generator().manual_seed(5000 + 100 * index + attempt)
        keys = torch.randn(c.A * c.Bt, c.K, generator=g) * 0.3 * c.scale
        querys = torch.randn(c.A * c.Bt, c.Q, generator=g)
        w = torch.randn(c.K, c.Q, generator=g) * 0.05
        b = torch.randn(c.K, generator=g) * 0.05
        if c.tie:
            # one key vector per frame whose score is the same for EVERY query and above every other key's: the minimum-norm solution of
            # x . qp_q = top (A equations, K unknowns), solved in float64, rounded to fp32 and given to both agents bit for bit
            k1, k2 = c.tie
            s0 = attn_handshake_ref64(keys, querys, w, b, c.A, c.Bt, "softmax")[0]
            q64 = querys.double().view(c.A, c.Bt, -1).transpose(0, 1)
            qp = q64 @ w.double().T + b.double()                                   # (Bt, A, K)
            for f in range(c.Bt):
                top = 2.0 * float(s0[f].abs().max()) + 1.0
                x = torch.linalg.pinv(qp[f]) @ torch.full((c.A,), top, dtype=torch.float64)
                keys[k1 * c.Bt + f] = x.float()
                keys[k2 * c.Bt + f] = keys[k1 * c.Bt + f]
        scores, prob, _ = attn_handshake_ref64(keys, querys, w, b, c.A, c.Bt, "softmax")
        margin, gap, tie_ok = attn_conditions(c, scores, prob)
        if margin >= ATTN_THRES_MARGIN and gap >= ATTN_GAP and tie_ok:
            return keys, querys, w, b
    raise AssertionError("no draw of %s satisfies the conditions" % (c,))


# ------------------------------------------------------------------------------------------------------------------ pixel-weighted fuse
def pixel_weighted_fuse_ref64(scores, valid, maps):
    """scores (n, A, H, W, S) (channel 0 is read), valid (n, A) (0 = source absent), maps (n, A, H, W, C) -> (n, H, W, C) float64:
    per pixel w_k = exp(s_k) / sum_j exp(s_j) over the valid sources -- exp WITHOUT a shift, as upstream -- and the weighted sum of the maps."""
    n, A = valid.shape
    e = torch.exp(scores[..., 0].to(torch.float64)) * (valid != 0).to(torch.float64).view(n, A, 1, 1)
    w = e / e.sum(1, keepdim=True)
    return (w.unsqueeze(-1) * maps.to(torch.float64)).sum(1)


PixelCase = namedtuple("PixelCase", "n A H W C S smax")
PIXEL_CASES = [
    PixelCase(3, 5, 8, 16, 64, 4, 3.0),                # the anchor (test_pixel_weighted_fuse_vs_torch)
    PixelCase(2, 6, 64, 64, 128, 1, 3.0),
    PixelCase(1, 32, 8, 8, 8, 2, 3.0),
    PixelCase(2, 3, 128, 128, 256, 1, 3.0),            # H W C / 8 = 524 288 > 65 536: the grid-stride loop runs 8 passes
    PixelCase(70, 2, 8, 8, 16, 1, 3.0),
    PixelCase(3, 5, 8, 16, 64, 4, 20.0),               # exp(20) = 4.9e8, unshifted on both sides
]


def pixel_case_id(c):
    return "n%d-A%d-%dx%dx%d-S%d-smax%g" % (c.n, c.A, c.H, c.W, c.C, c.S, c.smax)


def make_pixel_case(c, index):
    """valid rows walk: all sources / the ego (source 0) only / a middle source missing.  (An all-invalid row is left out on purpose:
    upstream divides 0 by 0 there and the ego is always valid.)"""
    g = torch.Generator().manual_seed(7000 + index)
    maps = bf16r(torch.randn(c.n, c.A, c.H, c.W, c.C, generator=g))
    scores = torch.rand(c.n, c.A, c.H, c.W, c.S, generator=g) * c.smax
    valid = torch.ones(c.n, c.A)
    for m in range(c.n):
        if m % 3 == 1:
            valid[m, 1:] = 0
        elif m % 3 == 2 and c.A >= 3:
            valid[m, c.A // 2] = 0
    if c.n < 3 and c.A >= 3:                             # fewer rows than patterns: the last row takes the missing middle source
        valid[c.n - 1] = 1
        valid[c.n - 1, c.A // 2] = 0
    return scores, valid, maps


# ------------------------------------------------------------------------------------------------------------------ seg argmax + confusion
def argmax_confusion_ref(logits, label, n_cls):
    """logits (..., n_cls) fp32, label (...) uint8 or None -> (pred int64, conf int64 [n_cls, n_cls] or None): the FIRST maximal class wins;
    conf[label][pred] counts the pixels whose label is < n_cls (anything else is 'ignore')."""
    lg = logits.numpy() if isinstance(logits, torch.Tensor) else np.asarray(logits)
    pred = np.argmax(lg.reshape(-1, n_cls), axis=1).astype(np.int64)           # numpy: the first maximum
    conf = None
    if label is not None:
        lb = (label.numpy() if isinstance(label, torch.Tensor) else np.asarray(label)).reshape(-1).astype(np.int64)
        keep = lb < n_cls
        conf = torch.from_numpy(np.bincount(lb[keep] * n_cls + pred[keep], minlength=n_cls * n_cls).reshape(n_cls, n_cls))
    return torch.from_numpy(pred.reshape(lg.shape[:-1])), conf


# offset: which tensor is a view into a larger buffer ("logits": 4 bytes in, "label": 1 byte in) so that the 8-class form's alignment
# conditions fail.  About 2 % of the pixels have their logits quantised to halves (exact ties); labels are drawn from 0 .. n_cls + 1 (>= n_cls = ignore)
SegCase = namedtuple("SegCase", "n H W n_cls offset")
SEG_CASES = [
    SegCase(80, 256, 256, 8, None),         # 5 242 880 px > 4 096 * 256 * 4: the 8-class kernel's grid-stride loop runs a second pass
    SegCase(3, 512, 512, 5, None),          # 786 432 px > 2 048 * 256: the generic kernel's loop runs a second pass
    SegCase(2, 16, 24, 1, None),
    SegCase(2, 16, 24, 64, None),
    SegCase(1, 3, 5, 8, None),              # n H W % 4 != 0: the generic kernel
    SegCase(2, 32, 32, 8, "logits"),
    SegCase(2, 32, 32, 8, "label"),
    SegCase(3, 64, 64, 8, None),            # the anchor (test_seg_argmax_confusion_exact)
]


def seg_case_id(c):
    return "%dx%dx%d-cls%d%s" % (c.n, c.H, c.W, c.n_cls, "-%s_offset" % c.offset if c.offset else "")


def make_seg_case(c, index):
    g = torch.Generator().manual_seed(9000 + index)
    logits = torch.randn(c.n, c.H, c.W, c.n_cls, generator=g)
    q = torch.rand(c.n, c.H, c.W, 1, generator=g) < 0.02                       # whole pixels quantised to halves: exact ties among their classes
    logits = torch.where(q, torch.round(logits * 2) / 2, logits)
    label = torch.randint(0, c.n_cls + 2, (c.n, c.H, c.W), generator=g).to(torch.uint8)
    return logits, label

"""float64 references, plan mirrors and the seeded case tables for the TRAINING kernels (csrc/conv_wgrad.hip, bn_train.hip, gru_train.hip,
v2v_train.hip, warp_train.hip, upcat_train.hip, det_loss.hip, adam.hip and the train_math.h they share).  A plain helper module (as
tests/fusion_refs.py): tests/test_train_refs_cpu.py checks the references against float64 autograd and every condition the tables must
satisfy without a GPU, tests/test_gpu_train_sweep.py holds the kernels to them.

Every reference is the plain statement of the operation in torch.float64 on the CPU, fed the operands the kernel gets (bf16 maps and fp32
parameters widened exactly).  The backward references are written out as formulas; autograd checks them in the CPU test.  The `*_f32`
functions beside them are torch's own fp32 evaluation of the same operation -- the reference tests/test_gpu_train_kernels.py compares with --
whose error against float64 sets the bar of the fp32 outputs (fp32_bar)."""
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

BF16 = torch.bfloat16
F64 = torch.float64


def bf16r(x):
    return x.to(BF16).to(torch.float32)


def f32c(v):
    """A python float as the kernel receives it through a `float` argument, widened exactly."""
    return float(np.float32(v))


def ulp32(ref64):
    """One fp32 ulp of each element's reference value (2^-149 at 0 and for denormals)."""
    a = ref64.to(F64).abs()
    _, e = torch.frexp(a)
    e = torch.where(a == 0, torch.full_like(e, -125), e)
    return torch.ldexp(torch.ones_like(a), (e - 24).clamp(min=-149))


def fp32_bar(ref64, ref32, factor=4.0):
    """The bar of an fp32 output: per element `factor` x the worst error of torch's own fp32 evaluation of this case against float64, with a
    floor of one fp32 ulp of the element's reference value.  -> (bar tensor, the reference-alone error)."""
    ref64 = ref64.to(F64)
    alone = float((ref32.to(F64) - ref64).abs().max()) if ref64.numel() else 0.0
    return torch.clamp(ulp32(ref64), min=factor * alone), alone


def worst_over_bar(got, ref64, bar):
    if ref64.numel() == 0:
        return 0.0
    return float(((got.to(F64) - ref64.to(F64)).abs() / bar).max())


def bf16r64(x):
    """float64 -> the nearest bf16 value (ties to even), ONE rounding, returned as float64 (torch's own float64 -> bfloat16 cast goes through
    fp32: two roundings).  Normal range only."""
    x = x.to(F64)
    _, e = torch.frexp(x)
    q = torch.ldexp(torch.ones_like(x), e - 8)
    return torch.round(x / q) * q


def flip_share(got, ref64):
    """Share of the elements of a bf16-stored output that differ AT ALL from the float64 reference rounded once to bf16."""
    if ref64.numel() == 0:
        return 0.0
    return float((got.to(F64) != bf16r64(ref64)).double().mean())


TINY, SMALL = 1000, 20000      # element counts below which a case's inputs are drawn until they are clear of bf16 ties / of the ReLU kink


def clear_of_bf16_ties(ref64, margin=2e-6, floor=0.12):
    """True when no element of the float64 reference lies within margin x max(|element|, floor x max |reference|) of the midpoint between two
    bf16 neighbours: no evaluation whose error is ~16 fp32 ulps of the element (or, for an element that is a difference of larger terms, ~2 fp32
    ulps of the largest element) can then round to the other neighbour.  The sweep's cap on rounding flips is a SHARE (1e-3 of a case); on a case of a few hundred elements it demands zero flips,
    which for random inputs would be luck (an fp32 evaluation flips ~2e-4 of the elements) -- so the inputs of such a case are drawn until
    this holds, and the demand is one on the kernel."""
    x = ref64.to(F64).abs().reshape(-1)
    x = x[x > 0]
    if x.numel() == 0:
        return True
    _, e = torch.frexp(x)
    q = torch.ldexp(torch.ones_like(x), e - 8)                 # one bf16 step of the element
    t = x / q
    return bool(((((t - torch.floor(t)) - 0.5).abs() * q) > margin * torch.clamp(x, min=floor * float(x.max()))).all())


def fp32_flips(ref32, ref64):
    """Share of elements on which fp32-then-bf16 differs from float64-then-bf16."""
    return flip_share(bf16r(ref32), ref64)


FLIP_CAP = 5e-4          # the double-rounding condition of tests/test_train_refs_cpu.py (the GPU sweep tolerates 1e-3 per case)


# ====================================================================================================== plan mirrors (constants of the sources)
C8_CHANNELS = (8, 16, 32, 64, 128, 256, 512, 1024, 2048)      # train_math.h::tm_chan8_shape_ok: C % 8 == 0 and 256 % (C / 8) == 0
BN_THREADS, BN_MAX_BLOCKS, BN_DXSUM_MAX_BLOCKS = 256, 2048, 2048
CS_MAX_BLOCKS = 512
GATES_MAX_BLOCKS = 256
DL_THREADS, DL_MAX_BLOCKS, DL_BWD_MAX_BLOCKS = 256, 1024, 4096
WG_TH, WG_TW, WG_CI, WG_CO = 8, 32, 32, 64
VB_PIX = 8
WT_CCH = 16
ADAM_BLOCK_ELEMS = 4096


def chan8_ok(M, C):
    return M > 0 and C >= 8 and C % 8 == 0 and 256 % (C // 8) == 0


def rpp(C):
    """Rows a 256-thread workgroup covers per pass (train_math.h: 256 / (C / 8)); gru_train.hip calls it nsub."""
    return 256 // (C // 8)


def bn_plan(M, C):
    """bn_train.hip::bn_plan -> (vec_per_block, n_blocks)."""
    total = M * (C // 8)
    per = -(-total // BN_MAX_BLOCKS)
    per = -(-per // BN_THREADS) * BN_THREADS
    per = max(per, BN_THREADS)
    return per, -(-total // per)


def bn_dxsum_blocks(M, C):
    """bn_train.hip::bn_train_backward_impl / v2x_bn_dxsum_workspace_size -> (blocks, uncapped blocks)."""
    b = -(-(M * (C // 8)) // BN_THREADS)
    return min(b, BN_DXSUM_MAX_BLOCKS), b


def cs_blocks(M, C):
    """bn_train.hip::cs_blocks -> (blocks, uncapped blocks)."""
    b = max(-(-M // (rpp(C) * 16)), 1)
    return min(b, CS_MAX_BLOCKS), b


def gates_plan(P, C):
    """gru_train.hip::gates_plan -> (rows_per_block, blocks)."""
    nsub = rpp(C)
    rpb = -(-P // GATES_MAX_BLOCKS)
    rpb = -(-rpb // nsub) * nsub
    return rpb, -(-P // rpb)


def dl_blocks(n):
    """det_loss.hip::dl_blocks -> (blocks, uncapped blocks)."""
    b = max(-(-n // (DL_THREADS * 8)), 1)
    return min(b, DL_MAX_BLOCKS), b


def dl_bwd_blocks(n):
    """det_loss.hip::v2x_det_loss_backward -> (blocks, uncapped blocks)."""
    b = -(-n // (DL_THREADS * 4))
    return min(b, DL_BWD_MAX_BLOCKS), b


def wgrad_plan(N, H, W, Cin, Cout):
    """conv_wgrad.hip::v2x_conv3x3_wgrad_splits + v2x_conv3x3_wgrad -> dict(rows32, tiles, pairs, want = ceil(384 / pairs), n_split = the blocks
    that share one (co tile, ci tile) pair, slots = the value the ABI returns); None for a shape the kernel refuses."""
    if N <= 0 or H <= 0 or W <= 0 or H % WG_TH or W % WG_TW or Cin <= 0 or Cin % WG_CI or Cout <= 0 or Cout % 32:
        return None
    rows32 = Cout % WG_CO != 0
    tiles = N * (H // WG_TH) * (W // WG_TW)
    pairs = (Cout // (32 if rows32 else WG_CO)) * (Cin // WG_CI)
    want = -(-384 // pairs)
    n = max(min(want, 256, tiles), 1)
    return dict(rows32=rows32, tiles=tiles, pairs=pairs, want=want, n_split=n, slots=2 * n if rows32 else n)


def v2v_bwd_form(K):
    """v2v_train.hip::v2x_v2v_message_bwd_bf16's launch (K <= 4: KMAX 4, else KMAX 8) and the kernel's `irregular = K > KMAX`."""
    return "kmax4" if K <= 4 else "kmax8" if K <= 8 else "irregular"


# ====================================================================================================== 3x3 weight gradient
def wgrad_ref64(x, dy):
    """x (N, H, W, Cin), dy (N, H, W, Cout) NHWC -> dW (Cout, Cin, 3, 3) float64: dW[co][ci][ky][kx] = sum over n, i, j of
    dy[n][i][j][co] * x[n][i + ky - 1][j + kx - 1][ci], zero padding."""
    x, dy = x.to(F64), dy.to(F64)
    N, H, W, Cin = x.shape
    Cout = dy.shape[3]
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    d2 = dy.reshape(-1, Cout)
    dw = torch.empty(Cout, Cin, 3, 3, dtype=F64)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = d2.t() @ xp[:, ky:ky + H, kx:kx + W].reshape(-1, Cin)
    return dw


def wgrad_f32(x, dy):
    """torch's fp32 evaluation (autograd of F.conv2d on the CPU), as tests/test_gpu_train_kernels.py::test_wgrad_kernel_vs_autograd."""
    w = torch.zeros(dy.shape[3], x.shape[3], 3, 3, requires_grad=True)
    F.conv2d(x.float().permute(0, 3, 1, 2), w, None, 1, 1).backward(dy.float().permute(0, 3, 1, 2))
    return w.grad


# reach: what the case is in the table for (checked against wgrad_plan by the CPU test)
#   tiles1   one pixel tile: n_split = 1                     clamp256  pairs = 1 and >= 256 tiles: the 256-split clamp binds
#   ragged   n_split does not divide the tile count           grid2d    H / 8 > 1 and W / 32 > 1
#   cin_out  the reduce writes fewer input channels than stored
WgradCase = namedtuple("WgradCase", "N H W Cin Cout cin_out exact reach seed")
WGRAD_CASES = [
    WgradCase(1, 8, 32, 32, 64, None, False, ("tiles1",), 1),
    WgradCase(1, 8, 32, 32, 64, None, True, ("tiles1",), 2),
    WgradCase(1, 8, 32, 32, 32, 13, False, ("tiles1", "cin_out"), 3),             # the 32-row form, one tile, the 13-channel first layer
    WgradCase(2, 16, 64, 32, 64, 13, True, ("cin_out", "grid2d"), 4),
    WgradCase(3, 24, 256, 96, 128, None, False, ("ragged", "grid2d"), 5),         # pairs 6 -> 64 splits over 72 tiles
    WgradCase(5, 16, 96, 256, 128, None, True, ("ragged", "grid2d"), 6),          # pairs 16 -> 24 splits over 30 tiles
    WgradCase(3, 8, 32, 32, 96, None, False, (), 7),                              # 32-row form: 3 tiles, 6 workspace slots
    WgradCase(7, 40, 192, 64, 32, None, True, ("ragged", "grid2d"), 8),           # 32-row form: pairs 2 -> 192 splits over 210 tiles
    WgradCase(3, 80, 320, 32, 64, None, False, ("clamp256", "ragged", "grid2d"), 9),   # pairs 1: 384 wanted, 256 taken, 300 tiles
    WgradCase(2, 128, 256, 32, 64, None, True, ("clamp256", "grid2d"), 10),       # pairs 1, exactly 256 tiles: one tile per split
    WgradCase(5, 64, 224, 32, 64, None, True, ("clamp256", "ragged", "grid2d"), 11),   # pairs 1, 280 tiles
]


def wgrad_case_id(c):
    return "%dx%dx%dx%d-%d%s%s" % (c.N, c.H, c.W, c.Cin, c.Cout, "" if c.cin_out is None else "-cin%d" % c.cin_out, "-int" if c.exact else "")


def small_ints(shape, g, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float32)


def make_wgrad_case(c):
    """-> x, dy as bf16 NHWC tensors (random normal, or integers in -2 .. 2 for an exact case)."""
    g = torch.Generator().manual_seed(1000 + c.seed)
    if c.exact:
        return small_ints((c.N, c.H, c.W, c.Cin), g).to(BF16), small_ints((c.N, c.H, c.W, c.Cout), g).to(BF16)
    return torch.randn(c.N, c.H, c.W, c.Cin, generator=g).to(BF16), torch.randn(c.N, c.H, c.W, c.Cout, generator=g).to(BF16)


# ====================================================================================================== batch-statistics BN
def bn_ref64(x, dy, gamma, beta, eps, momentum, rm, rv, relu):
    """x, dy (M, C); gamma, beta, rm, rv (C,).  -> dict of float64 tensors: mean, invstd, rm, rv (updated, unbiased variance), y, dx,
    dgamma, dbeta.  The per-channel sum of dx AS STORED is bn_dxsum_ref64 of the kernel's own dx."""
    x, dy, gamma, beta = x.to(F64), dy.to(F64), gamma.to(F64), beta.to(F64)
    M = x.shape[0]
    mean = x.sum(0) / M
    var = ((x - mean) ** 2).sum(0) / M
    invstd = 1.0 / torch.sqrt(var + eps)
    unbiased = var * M / (M - 1) if M > 1 else var
    xh = (x - mean) * invstd
    y0 = xh * gamma + beta
    g = torch.where(y0 > 0, dy, torch.zeros_like(dy)) if relu else dy
    dbeta = g.sum(0)
    dgamma = (g * xh).sum(0)
    dx = gamma * invstd * (g - dbeta / M - xh * dgamma / M)
    return dict(mean=mean, invstd=invstd, rm=(1 - momentum) * rm.to(F64) + momentum * mean, rv=(1 - momentum) * rv.to(F64) + momentum * unbiased,
                y0=y0, y=y0.clamp(min=0) if relu else y0, dx=dx, dgamma=dgamma, dbeta=dbeta)


def bn_dxsum_ref64(dx_stored):
    return dx_stored.to(F64).sum(0)


def bn_f32(x, dy, gamma, beta, eps, momentum, rm, rv, relu):
    """torch's fp32 evaluation: F.batch_norm(training=True) (+ relu) and its autograd, as test_bn_train_kernels_vs_autograd."""
    xr = x.float().requires_grad_(True)
    ga, be = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = rm.clone(), rv.clone()
    if x.shape[0] == 1:      # F.batch_norm refuses one value per channel (the kernels do not): the same expressions as fp32 ops
        mean, var = xr.mean(0), xr.var(0, unbiased=False)
        yr = (xr - mean) / torch.sqrt(var + eps) * ga + be
        with torch.no_grad():
            rm.mul_(1 - momentum).add_(momentum * mean)
            rv.mul_(1 - momentum).add_(momentum * var)
    else:
        yr = F.batch_norm(xr, rm, rv, ga, be, True, momentum, eps)
    if relu:
        yr = F.relu(yr)
    yr.backward(dy.float())
    var = x.float().var(0, unbiased=False)
    return dict(mean=x.float().mean(0), invstd=1.0 / torch.sqrt(var + eps), rm=rm, rv=rv, y=yr.detach(), dx=xr.grad, dgamma=ga.grad, dbeta=be.grad)


def bn_f32_ops(x, dy, gamma, beta, eps, relu):
    """The same operation as elementwise fp32 torch ops around torch.sum's cascade reductions -> (y, dx).  F.batch_norm's CPU kernel adds a
    channel's values one by one: at 5e5 rows its statistics are off by 1e-5, a property of that evaluation and not of the inputs, so the
    double-rounding CONDITION of the CPU test uses this form (the fp32 BARS keep F.batch_norm, the reference of the existing test)."""
    xr = x.float().requires_grad_(True)
    mean, var = xr.mean(0), xr.var(0, unbiased=False)
    y = (xr - mean) * torch.rsqrt(var + eps) * gamma + beta
    if relu:
        y = F.relu(y)
    y.backward(dy.float())
    return y.detach(), xr.grad


# reach: "cap-" / "cap+" = the row count just below / above the block cap of the kernel family (bn: M C / 8 = 2048 x 256, channel sum:
# M = 512 x 16 x rpp, gates backward: P = 256 x nsub), "rpp-" / "rpp+" = one row fewer / more than a workgroup covers per pass
C8Case = namedtuple("C8Case", "M C relu layout kind reach seed")      # kind: "randn", "int" (exact sums), "ill" (mean / std ~ 125)
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
BN_EPS_FEW_ROWS = 0.25
# With two or three rows and eps = 1e-5, dx is a difference of O(1) terms that cancel to O(eps / var): every fp32 evaluation (torch's own
# included) then lands on the other side of a bf16 rounding boundary on a large share of the elements, and the CPU test's double-rounding
# condition rejects the inputs.  eps = 0.25 keeps the same code paths with a well-conditioned dx.


def bn_eps(c):
    return BN_EPS_FEW_ROWS if c.M <= 3 else BN_EPS


def _c8_rows(C, cap_lo, cap_hi):
    """The row counts of one channel count: 2, 7, one fewer / more than a pass covers, 1000, the two sides of the cap; a count that appears
    twice keeps its tag (C = 2048: rpp - 1 = 0 is dropped, rpp + 1 = 2)."""
    r = rpp(C)
    rows = {}
    for M, reach in ((2, ""), (7, ""), (r - 1, "rpp-"), (r + 1, "rpp+"), (1000, ""), (cap_lo, "cap-"), (cap_hi, "cap+")):
        if M >= 1 and not rows.get(M):
            rows[M] = reach
    return list(rows.items())


def _bn_table():
    cases, k = [], 0
    for C in C8_CHANNELS:
        G = C // 8
        cap = BN_MAX_BLOCKS * BN_THREADS // G              # rows at which M * G = 2048 * 256 (BN_DXSUM_MAX_BLOCKS caps at the same count)
        for M, reach in _c8_rows(C, cap - 3, cap + 3):
            k += 1
            cases.append(C8Case(M, C, bool(k & 1), (k >> 1) & 1, "randn", reach, k))
    # relu and layout alternate down the table; the cap rows of one C get both layouts because they are neighbours in it
    cases.append(C8Case(3072, 64, True, 1, "ill", "", 901))
    cases.append(C8Case(3072, 64, False, 0, "ill", "", 902))
    cases.append(C8Case(1001, 32, False, 1, "int", "", 903))
    cases.append(C8Case(2048 * 256 // 128 + 3, 1024, False, 0, "int", "cap+", 904))
    cases.append(C8Case(2048 * 256 // 2 - 3, 16, False, 1, "int", "cap-", 905))
    return cases


BN_CASES = _bn_table()


def c8_case_id(c):
    return "M%d-C%d%s%s%s%s" % (c.M, c.C, "" if c.relu is None else "-relu" if c.relu else "-lin", "" if c.layout is None else "-T%d" % c.layout,
                                "" if c.kind == "randn" else "-" + c.kind, "-" + c.reach if c.reach else "")


def _draw_bn_case(c, seed):
    g = torch.Generator().manual_seed(seed)
    M, C = c.M, c.C
    if c.kind == "int":
        x, dy = small_ints((M, C), g), small_ints((M, C), g)
    elif c.kind == "ill":
        # bf16 steps of 0.125 around 16: mean / std ~ 125.  The rows come in pairs 16 + a, 16 - a, so every channel's mean is exactly 16: an fp32
        # mean of arbitrary values at 16 is off by up to 1e-6 = 8e-6 standard deviations, which moves 3e-3 of the bf16 roundings of y in ANY fp32
        # evaluation.  What the case is for stays: var = E[x^2] - mean^2 is 256.0156 - 256.
        half = 0.125 * torch.round(torch.randn(M // 2, C, generator=g))      # whole bf16 steps: 16 + a and 16 - a are both bf16 values
        x = torch.cat([16.0 + half, 16.0 - half] + ([torch.full((1, C), 16.0)] if M % 2 else []))
        dy = torch.randn(M, C, generator=g)
    elif M <= 16:
        # few rows: a ladder of rows about one standard deviation apart, so that no channel's variance is an accident of two close samples
        step = 0.75 + 0.5 * torch.rand(C, generator=g)
        x = torch.randn(C, generator=g) + (torch.arange(M, dtype=torch.float32)[:, None] - (M - 1) / 2) * step + 0.05 * torch.randn(M, C, generator=g)
        dy = torch.randn(M, C, generator=g)
    else:
        x = torch.randn(M, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
        dy = torch.randn(M, C, generator=g)
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    return x.to(BF16), dy.to(BF16), gamma, beta, rm0, rv0


BN_FIRST_DRAW = {5: 1, 37: 1}           # case seed -> first draw (make_bn_case); every other case starts at draw 0


def make_bn_case(c):
    """-> x, dy (M, C) bf16; gamma, beta, rm0, rv0 (C,) fp32.  A case of fewer than SMALL elements is drawn until no element of y sits within
    1e-5 of the ReLU kink, one of fewer than TINY until y and dx are also clear of bf16 ties (clear_of_bf16_ties): their share caps mean zero.
    Both criteria are float64 only, so every host draws the same inputs.  From TINY to SMALL elements the cap allows one to nine flips and a draw
    can sit on too many near-ties for ANY fp32 evaluation: BN_FIRST_DRAW names the first draw to try for those cases, fixed here once;
    tests/test_train_refs_cpu.py then measures the double-rounding condition on the inputs as drawn."""
    n = c.M * c.C
    for attempt in range(BN_FIRST_DRAW.get(c.seed, 0) if TINY <= n < SMALL else 0, 200):
        case = _draw_bn_case(c, 2000 + c.seed + 1000 * attempt)
        if n >= SMALL or c.kind == "int":
            return case
        x, dy, gamma, beta, rm0, rv0 = case
        ref = bn_ref64(x, dy, gamma, beta, f32c(bn_eps(c)), f32c(BN_MOMENTUM), rm0, rv0, c.relu)
        if c.relu and bool((ref["y0"].abs() < 1e-5).any()):
            continue
        if n < TINY and not (clear_of_bf16_ties(ref["y"]) and clear_of_bf16_ties(ref["dx"])):
            continue
        return case
    raise AssertionError("no well-conditioned draw for %s" % (c,))


# ====================================================================================================== channel sums
def channel_sum_ref64(x):
    return x.to(F64).reshape(-1, x.shape[-1]).sum(0)


def cast_pad_chsum_ref64(x, c_pad):
    """x (..., C) fp32 -> (the bf16 map zero-padded to c_pad channels, the float64 channel sums of x)."""
    return F.pad(x, (0, c_pad - x.shape[-1])).to(BF16), channel_sum_ref64(x)


def _cs_table():
    cases, k = [], 0
    for C in C8_CHANNELS:
        cap = CS_MAX_BLOCKS * 16 * rpp(C)
        for M, reach in _c8_rows(C, cap - 3, cap + 3):
            k += 1
            cases.append(C8Case(M, C, None, None, "int" if reach.startswith("cap") and (k & 1) else "randn", reach, k))
    cases.append(C8Case(1001, 16, None, None, "int", "", 950))
    return cases


CS_CASES = _cs_table()


def make_cs_case(c):
    g = torch.Generator().manual_seed(3000 + c.seed)
    if c.kind == "int":
        return small_ints((c.M, c.C), g).to(BF16)
    return (torch.randn(c.M, c.C, generator=g) + 0.3).to(BF16)


CpCase = namedtuple("CpCase", "M C Cp kind reach seed")


def _cp_table():
    cases, k = [], 0
    for Cp in C8_CHANNELS:
        r = rpp(Cp)
        rows = [(7, ""), (r + 1, "rpp+"), (1000, "")]
        if Cp in (8, 64, 2048):
            cap = CS_MAX_BLOCKS * 16 * r
            rows += [(cap - 3, "cap-"), (cap + 3, "cap+")]
        for M, reach in rows:
            k += 1
            C = Cp if k % 3 == 0 else Cp - 4              # C % 4 == 0; the last group's second float4 (or the whole row) is padding
            cases.append(CpCase(M, C, Cp, "int" if reach.startswith("cap") or k % 5 == 0 else "randn", reach, k))
    cases.append(CpCase(1000, 12, 32, "randn", "", 960))      # the heads' shapes
    cases.append(CpCase(1000, 36, 64, "int", "", 961))
    return cases


CP_CASES = _cp_table()


def cp_case_id(c):
    return "M%d-C%d-Cp%d%s%s" % (c.M, c.C, c.Cp, "" if c.kind == "randn" else "-" + c.kind, "-" + c.reach if c.reach else "")


def make_cp_case(c):
    g = torch.Generator().manual_seed(4000 + c.seed)
    if c.kind == "int":
        return small_ints((c.M, c.C), g)
    return torch.randn(c.M, c.C, generator=g) * 0.1 + 0.01


# ====================================================================================================== ConvGRU gates (h0 = 0)
def gru_gates_ref64(gi, bhh, dh, dim=-1):
    """gi (.., 3C, ..) with the r | z | n thirds along `dim`, bhh (3C,), dh like a third of gi.  -> dict of float64: h, dgi (like gi), dpn_r
    (dpre_n * r), dbhh (3C) = the channel sums (d gi_r, d gi_z, dpre_n * r) -- csrc/train_math.h::tm_gru_gates_fwd / _bwd written out."""
    gi, bhh = gi.to(F64), bhh.to(F64)
    shape = [1] * gi.dim()
    shape[dim] = -1
    gr, gz, gn = gi.chunk(3, dim)
    br, bz, bn = (b.reshape(shape) for b in bhh.chunk(3))
    r, z = torch.sigmoid(gr + br), torch.sigmoid(gz + bz)
    n = torch.tanh(gn + r * bn)
    out = dict(h=n - z * n)
    if dh is not None:
        dh = dh.to(F64)
        dn, dz = dh * (1 - z), -dh * n
        dpn = dn * (1 - n * n)
        dr = dpn * bn
        out["dgi"] = torch.cat([dr * r * (1 - r), dz * z * (1 - z), dpn], dim)
        out["dpn_r"] = dpn * r
        red = [d for d in range(gi.dim()) if d != (dim % gi.dim())]
        out["dbhh"] = torch.cat([out["dgi"].sum(red)[:2 * bz.numel()], out["dpn_r"].sum(red)])
    return out


def gates_sums6_ref64(dgi_stored, dpn_r64):
    """The six channel-sum vectors of v2x_gru_gates_nhwc_bwd_bf16: sums of dgi AS STORED (r, z, n: d bias_ih), the same r, z again, sums of
    the unrounded dpre_n * r (d bias_hh's n part)."""
    s = dgi_stored.to(F64).reshape(-1, dgi_stored.shape[-1]).sum(0)
    C = s.numel() // 3
    return torch.cat([s, s[:2 * C], dpn_r64.reshape(-1, C).sum(0)])


def gru_gates_f32(gi, bhh, dh, dim=-1):
    """torch's fp32 evaluation: the ops of train/graph.py::_gru_step and their autograd (test_gru_gates_nhwc_vs_torch)."""
    x = gi.float().clone().requires_grad_(True)
    b = bhh.float().clone().requires_grad_(True)
    shape = [1] * x.dim()
    shape[dim] = -1
    i_r, i_z, i_n = x.chunk(3, dim)
    h_r, h_z, h_n = (t.reshape(shape) for t in b.chunk(3))
    r = torch.sigmoid(i_r + h_r)
    z = torch.sigmoid(i_z + h_z)
    n = torch.tanh(i_n + r * h_n)
    h = n - z * n
    h.backward(dh.float())
    return dict(h=h.detach(), dgi=x.grad, dbhh=b.grad, dpn_r=x.grad.chunk(3, dim)[2] * r.detach())


def _gates_table():
    cases, k = [], 0
    for C in C8_CHANNELS:
        cap = GATES_MAX_BLOCKS * rpp(C)
        for P, reach in _c8_rows(C, cap - 1, cap + 1):
            k += 1
            cases.append(C8Case(P, C, None, None, "randn", reach, k))
    cases.append(C8Case(1001, 32, None, None, "randn", "", 970))      # the two shapes of the shared-arithmetic commit
    cases.append(C8Case(1536, 64, None, None, "randn", "", 971))
    return cases


GATES_NHWC_CASES = _gates_table()
GRU_COPY_SHAPES = ((1001, 32), (1536, 64))


GATES_FIRST_DRAW = {4: 1, 23: 1, 42: 1, 49: 1}


def make_gates_nhwc_case(c):
    """-> gi (P, 3C) bf16, bhh (3C,) fp32, dh (P, C) bf16; a case whose dgi has fewer than TINY elements is drawn until h and dgi are clear of
    bf16 ties (clear_of_bf16_ties: float64 only); one of TINY to SMALL elements is the draw GATES_FIRST_DRAW names (as BN_FIRST_DRAW)."""
    mid = TINY <= c.M * 3 * c.C < SMALL
    for attempt in range(GATES_FIRST_DRAW.get(c.seed, 0) if mid else 0, 200):
        g = torch.Generator().manual_seed(5100 + c.seed + 1000 * attempt)
        gi = (torch.randn(c.M, 3 * c.C, generator=g) * 1.5).to(BF16)
        bhh = torch.randn(3 * c.C, generator=g) * 0.5
        dh = torch.randn(c.M, c.C, generator=g).to(BF16)
        if gi.numel() >= TINY:
            return gi, bhh, dh
        ref = gru_gates_ref64(gi, bhh, dh)
        if clear_of_bf16_ties(ref["h"]) and clear_of_bf16_ties(ref["dgi"], floor=0.0):      # dgi is a product: relative errors only
            return gi, bhh, dh
    raise AssertionError("no draw clear of bf16 ties for %s" % (c,))


GatesF32Case = namedtuple("GatesF32Case", "P C H W seed")
GATES_F32_CASES = [GatesF32Case(3, 5, 2, 2, 1), GatesF32Case(2, 1, 2, 2, 2), GatesF32Case(2, 1, 3, 4, 3), GatesF32Case(4, 16, 4, 5, 4),
                   GatesF32Case(7, 3, 6, 6, 5), GatesF32Case(1, 64, 4, 7, 6), GatesF32Case(5, 32, 16, 16, 7)]


def make_gates_f32_case(c):
    """-> gi (P, 3C, H, W), bhh (3C,), dh (P, C, H, W) fp32: pre-activations spanning +-90 (saturated gates, expf overflow), exact zeros,
    and gi + b = 0 exactly on the first pixel of every map."""
    g = torch.Generator().manual_seed(6000 + c.seed)
    gi = torch.randn(c.P, 3 * c.C, c.H, c.W, generator=g) * 2.0
    bhh = torch.randn(3 * c.C, generator=g) * 0.5
    flat = gi.view(c.P, 3 * c.C, -1)
    hw = c.H * c.W
    span = torch.linspace(-90.0, 90.0, hw)
    flat[0] = span[None, :] * (1 - 2 * (torch.arange(3 * c.C) % 2))[:, None]      # map 0: every channel sweeps -90 .. 90 (odd channels 90 .. -90)
    flat[-1, :, 1] = 0.0                                                           # exact zeros
    flat[:, :, 0] = -bhh[None, :]                                                  # gi + b = 0 (r = z = 1/2 exactly)
    dh = torch.randn(c.P, c.C, c.H, c.W, generator=g)
    return gi.contiguous(), bhh, dh


# ====================================================================================================== affine warp and its transpose
def warp_affine_ref64(x, theta):
    """x (P, C, H, W), theta (P, 2, 3): F.affine_grid + F.grid_sample (bilinear, zeros, align_corners=False) in float64."""
    x, theta = x.to(F64), theta.to(F64)
    return F.grid_sample(x, F.affine_grid(theta, list(x.shape), align_corners=False), mode="bilinear", padding_mode="zeros", align_corners=False)


def warp_matrix64(theta, H, W):
    """The same operator of ONE pose as a dense (H W) x (H W) float64 matrix S: out[q] = sum over p of S[q][p] in[p], the four bilinear
    weights of output pixel q on its in-range neighbours.  Sample position: affine_grid + grid_sample's unnormalisation, written out."""
    th = theta.to(F64)
    j = torch.arange(W, dtype=F64)
    i = torch.arange(H, dtype=F64)
    xn = ((2 * j + 1) / W - 1)[None, :].expand(H, W)
    yn = ((2 * i + 1) / H - 1)[:, None].expand(H, W)
    gx = th[0, 0] * xn + th[0, 1] * yn + th[0, 2]
    gy = th[1, 0] * xn + th[1, 1] * yn + th[1, 2]
    ix = (((gx + 1) * W - 1) / 2).reshape(-1)
    iy = (((gy + 1) * H - 1) / 2).reshape(-1)
    fx, fy = torch.floor(ix), torch.floor(iy)
    S = torch.zeros(H * W, H * W, dtype=F64)
    q = torch.arange(H * W)
    for dx_, dy_ in ((0, 0), (1, 0), (0, 1), (1, 1)):
        px, py = fx + dx_, fy + dy_
        w = (1 - (ix - px).abs()) * (1 - (iy - py).abs())
        ok = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        S.index_put_((q[ok], (py[ok] * W + px[ok]).long()), w[ok], accumulate=True)
    return S


def warp_affine_transpose_ref64(d, theta):
    """The transpose of warp_affine_ref64 applied to an output gradient d (P, C, H, W): the explicit gather din[p] = sum over q of S[q][p] d[q]
    over the same weights."""
    P, C, H, W = d.shape
    d = d.to(F64)
    return torch.stack([(warp_matrix64(theta[p], H, W).t() @ d[p].reshape(C, -1).t()).t().reshape(C, H, W) for p in range(P)])


def warp_affine_f32(x, theta, d):
    """torch's fp32 evaluation: grid_sample and autograd's grid_sampler backward (test_warp_affine_forward_and_transpose_vs_grid_sample)."""
    xr = x.float().clone().requires_grad_(True)
    y = F.grid_sample(xr, F.affine_grid(theta.float(), list(x.shape), align_corners=False), mode="bilinear", padding_mode="zeros", align_corners=False)
    g, = torch.autograd.grad(y, xr, d.float())
    return y.detach(), g


def warp_poses(H, W):
    """One theta (2, 3) per named pose, for a map of H x W pixels.  A translation of (px, py) pixels is theta[:, 2] = (2 px / W, 2 py / H)."""
    def T(a, b, c, d, e, f):
        return torch.tensor([[a, b, c], [d, e, f]], dtype=torch.float32)
    c45 = math.cos(math.pi / 4)
    r = H / W                                           # a rotation of the PIXEL grid: theta = [[c, -s H / W], [s W / H, c]]
    poses = [("identity", T(1, 0, 0, 0, 1, 0)),
             ("whole-pixel", T(1, 0, 2 * 3 / W, 0, 1, -2 * 2 / H)),
             ("half-pixel", T(1, 0, 2 * 0.5 / W, 0, 1, 2 * 1.5 / H)),           # all four weights 1/4
             ("one-width-out", T(1, 0, 2.0, 0, 1, 0)),                           # exactly one map width: every sample is out of range
             ("one-column-left", T(1, 0, 2.0 * (W - 1) / W, 0, 1, 0)),           # W - 1 pixels: only output column 0 reads a pixel (input column W - 1)
             ("rot90", T(0, -r, 0, 1 / r, 0, 0)),
             ("rot45", T(c45, -c45 * r, 0, c45 / r, c45, 0)),
             ("reflect", T(-1, 0, 0.1, 0, 1, 0)),                                # det < 0
             ("shear-aniso", T(0.7, 0.45, 0.1, -0.3, 1.4, -0.2)),
             ("zoom-in-8", T(0.125, 0, 0, 0, 0.125, 0)),
             ("zoom-out-4", T(4, 0, 0, 0, 4, 0)),
             ("rank1", T(0.5, 0.25, 0.1, 1.0, 0.5, -0.2)),
             ("zero", T(0, 0, 0.1, 0, 0, -0.2)),
             ("det>1e-6", T(1.0, 0.0, 0.05, 0.0, 2e-6, 0.1)),                    # the inverse is used: candidate boxes a whole column high
             ("det<1e-6", T(1.0, 0.0, 0.05, 0.0, 5e-7, 0.1))]                    # |det| below the switch of tm_warp_candidates: the whole map
    return poses


def warp_det(theta, H, W):
    """det of the pixel-space matrix of tm_warp_candidates (train_math.h), in float64 from the fp32 theta."""
    th = theta.to(F64)
    return float(th[0, 0] * th[1, 1] - (th[0, 1] * W / H) * (th[1, 0] * H / W))


WarpTrainCase = namedtuple("WarpTrainCase", "C H W seed")
WARP_TRAIN_CASES = [WarpTrainCase(1, 16, 48, 1), WarpTrainCase(16, 16, 48, 2), WarpTrainCase(20, 16, 48, 3),
                    WarpTrainCase(1, 5, 7, 4), WarpTrainCase(16, 5, 7, 5), WarpTrainCase(20, 5, 7, 6)]
WARP_POSE_NAMES = [n for n, _ in warp_poses(16, 48)]


def make_warp_train_case(c):
    """-> x, d (P, C, H, W) fp32 and theta (P, 2, 3): one map per pose."""
    g = torch.Generator().manual_seed(7000 + c.seed)
    th = torch.stack([t for _, t in warp_poses(c.H, c.W)])
    P = th.shape[0]
    return torch.randn(P, c.C, c.H, c.W, generator=g), torch.randn(P, c.C, c.H, c.W, generator=g), th


# ====================================================================================================== V2VNet's message (two-pass warp, mean, concat)
def v2v_thetas(T):
    """v2v_train.hip::vt_thetas / graph.py::warp_batch: pose (4, 4) -> (rotation theta, translation theta)."""
    T = T.to(F64)
    z, o = torch.zeros((), dtype=F64), torch.ones((), dtype=F64)
    rot = torch.stack([torch.stack([T[0, 0], T[0, 1], z]), torch.stack([T[1, 0], T[1, 1], z])])
    tr = torch.stack([torch.stack([o, z, 4 * T[0, 3] / 128]), torch.stack([z, o, -4 * T[1, 3] / 128])])
    return rot, tr


def v2v_pairs(A, B):
    """graph.py::v2v_fuse's pair enumeration for B frames of A agents each (what hip_graph._v2v_plan tabulates): items (agent, frame) agent-major,
    rows, and per item its K = A - 1 pairs (item, source row, frame, ego, neighbour) in agent order."""
    items = [(a, f) for a in range(A) for f in range(B)]
    rows = [a * B + f for a, f in items]
    pairs = [(m, j * B + f, f, a, j) for m, (a, f) in enumerate(items) for j in range(A) if j != a]
    return items, rows, pairs


def v2v_message_ref64(cur, base, T, A, B):
    """cur, base (N, H, W, C) NHWC, T (B, A, A, 4, 4) -> conv_in (M, H, W, 2C) float64 = [cur[rows[m]] | mean over the K neighbours of
    grid_sample(grid_sample(base[src], rotation), translation)] -- tests/test_gpu_train_kernels.py::_v2v_reference in float64."""
    items, rows, pairs = v2v_pairs(A, B)
    N, H, W, C = base.shape
    b = base.to(F64).permute(0, 3, 1, 2)
    src = torch.tensor([p[1] for p in pairs])
    th = [v2v_thetas(T[f, a, j]) for (_, _, f, a, j) in pairs]
    rot, tr = torch.stack([t[0] for t in th]), torch.stack([t[1] for t in th])
    warped = warp_affine_ref64(warp_affine_ref64(b.index_select(0, src), rot), tr)
    mean = warped.view(len(items), A - 1, C, H, W).mean(1)
    return torch.cat([cur.to(F64)[torch.tensor(rows)], mean.permute(0, 2, 3, 1)], 3)


def v2v_message_bwd_ref64(d, T, A, B, separate_cur):
    """d (M, H, W, 2C) the gradient of conv_in -> (dbase (N, H, W, C), dcur or None) float64: the explicit transposes
    dbase[src] += S_rot^T S_tr^T d_msg[m] / K over every pair, the ego half added to its own row (or returned beside it)."""
    items, rows, pairs = v2v_pairs(A, B)
    M, H, W, C2 = d.shape
    C, K = C2 // 2, A - 1
    d = d.to(F64)
    dbase = torch.zeros(A * B, H * W, C, dtype=F64)
    for (m, s, f, a, j) in pairs:
        rot, tr = v2v_thetas(T[f, a, j])
        S1, S2 = warp_matrix64(rot, H, W), warp_matrix64(tr, H, W)
        dbase[s] += S1.t() @ (S2.t() @ d[m, :, :, C:].reshape(H * W, C)) / K
    dbase = dbase.view(A * B, H, W, C)
    dcur = torch.zeros(A * B, H, W, C, dtype=F64)
    dcur[torch.tensor(rows)] = d[..., :C]
    return (dbase, dcur) if separate_cur else (dbase + dcur, None)


def v2v_f32(cur, base, T, A, B, d):
    """torch's fp32 evaluation (grid_sample twice, mean, cat and autograd): the reference of test_v2v_message_forward_and_backward_vs_torch.
    Only used by the CPU test's double-rounding condition."""
    items, rows, pairs = v2v_pairs(A, B)
    N, H, W, C = base.shape
    x = base.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    c = cur.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    src = torch.tensor([p[1] for p in pairs])
    th = [v2v_thetas(T[f, a, j]) for (_, _, f, a, j) in pairs]
    rot, tr = torch.stack([t[0] for t in th]).float(), torch.stack([t[1] for t in th]).float()
    xs = x.index_select(0, src)
    w1 = F.grid_sample(xs, F.affine_grid(rot, list(xs.shape), align_corners=False), mode="bilinear", padding_mode="zeros", align_corners=False)
    w2 = F.grid_sample(w1, F.affine_grid(tr, list(xs.shape), align_corners=False), mode="bilinear", padding_mode="zeros", align_corners=False)
    out = torch.cat([c[torch.tensor(rows)], w2.view(len(items), A - 1, C, H, W).mean(1)], 1)
    out.backward(d.float().permute(0, 3, 1, 2))
    return out.detach().permute(0, 2, 3, 1), x.grad.permute(0, 2, 3, 1), c.grad.permute(0, 2, 3, 1)


# form: the backward form the case reaches -- "kmax4" (K <= 4), "kmax8" (5 <= K <= 8), "irregular" (K > 8, or a candidate box wider than the
# 9 x 12 tables: `shrink`).  two: separate cur and base maps.  signed: maps and gradients of both signs (make_v2v_case), judged with the existing
# test's bar alone.
V2vCase = namedtuple("V2vCase", "A B C H W two shrink form seed signed", defaults=(False,))
V2V_CASES = [
    V2vCase(2, 3, 8, 9, 9, False, False, "kmax4", 1),       # K = 1, Bt = 3, H W % 8 = 1: the last chunk holds one pixel
    V2vCase(2, 1, 24, 5, 7, True, False, "kmax4", 2),       # H W % 8 = 3
    V2vCase(5, 2, 24, 9, 9, True, False, "kmax4", 3),       # K = 4
    V2vCase(5, 1, 8, 5, 7, False, False, "kmax4", 4),
    V2vCase(6, 1, 8, 9, 9, False, False, "kmax8", 5),       # K = 5
    V2vCase(6, 2, 24, 5, 7, True, False, "kmax8", 6),
    V2vCase(9, 1, 8, 9, 9, True, False, "kmax8", 7),        # K = 8
    V2vCase(9, 1, 24, 5, 7, False, False, "kmax8", 8),
    V2vCase(10, 1, 8, 5, 7, False, False, "irregular", 9),  # K = 9
    V2vCase(10, 1, 24, 9, 9, True, False, "irregular", 10),
    V2vCase(3, 1, 8, 9, 9, False, True, "irregular", 11),   # a shrinking pose: more candidates than the tables hold
    V2vCase(6, 2, 24, 8, 32, True, True, "irregular", 12),
    V2vCase(5, 2, 8, 9, 9, True, False, "kmax4", 13, True),         # one signed case per form: cancelling sums, the sign of every weight
    V2vCase(6, 1, 24, 5, 7, False, False, "kmax8", 14, True),
    V2vCase(10, 1, 8, 9, 9, False, False, "irregular", 15, True),
]


def v2v_case_id(c):
    return "A%d-B%d-C%d-%dx%d-%s%s-%s" % (c.A, c.B, c.C, c.H, c.W, "two" if c.two else "one", "-shrink" if c.shrink else "", c.form + ("-signed" if c.signed else ""))


def make_v2v_case(c):
    """-> cur, base (N, H, W, C) bf16 (the same tensor unless c.two), T (B, A, A, 4, 4) fp32, d (M, H, W, 2C) bf16.  Poses as
    tests/test_gpu_train_kernels.py::_v2v_case: small rotations, translations of a few cells, one neighbour pushed almost off the map."""
    g = torch.Generator().manual_seed(8000 + c.seed)
    A, B = c.A, c.B
    N = A * B
    # Positive maps and gradients (0.5 + |normal|): with signed values an element of the message is a cancelling sum of up to 16 K products whose
    # weights carry the fp32 coordinate arithmetic's 1e-6, and torch's own fp32 evaluation then rounds 5e-4 .. 1.5e-3 of the elements to the other
    # bf16 neighbour -- above the double-rounding condition of the CPU test.  A dropped, doubled or mis-weighted tap still moves an element by
    # O(1 / (4 K)) of its value.  The signed cases (plain normal values, as the existing test's) keep cancelling sums and the sign of every weight
    # covered: they are outside the double-rounding condition, so the sweep judges them with the existing bar and without the flip cap.
    draw = (lambda *shape: torch.randn(*shape, generator=g)) if c.signed else (lambda *shape: 0.5 + torch.randn(*shape, generator=g).abs())
    base = draw(N, c.H, c.W, c.C).to(BF16)
    cur = draw(N, c.H, c.W, c.C).to(BF16) if c.two else base
    ang = (torch.rand(B, A, A, generator=g) - 0.5) * 1.2
    T = torch.zeros(B, A, A, 4, 4)
    T[..., 0, 0], T[..., 0, 1], T[..., 1, 0], T[..., 1, 1] = torch.cos(ang), -torch.sin(ang), torch.sin(ang), torch.cos(ang)
    T[..., 0, 3] = (torch.rand(B, A, A, generator=g) - 0.5) * 12.0
    T[..., 1, 3] = (torch.rand(B, A, A, generator=g) - 0.5) * 12.0
    T[0, 0, 1, 0, 3] = 40.0
    T[..., 2, 2] = T[..., 3, 3] = 1.0
    if c.shrink:
        T[0, 1, 0, :2, :2] *= 0.3
    d = draw(N, c.H, c.W, 2 * c.C).to(BF16)
    return cur, base, T, d


def warp_box_extent(theta, H, W):
    """tm_warp_candidates (train_math.h) in float64: the largest (jhi - jlo, ihi - ilo) over the pixels of the map, (W - 1, H - 1) when the
    pose takes the whole-map branch.  The tables of v2v_message_bwd_kernel hold boxes of extent <= 2."""
    th = theta.to(F64)
    m00, m01, m10, m11 = float(th[0, 0]), float(th[0, 1]) * W / H, float(th[1, 0]) * H / W, float(th[1, 1])
    det = m00 * m11 - m01 * m10
    if not abs(det) > 1e-6:
        return W - 1, H - 1
    xn0, yn0 = 1.0 / W - 1, 1.0 / H - 1
    t0 = ((float(th[0, 0]) * xn0 + float(th[0, 1]) * yn0 + float(th[0, 2]) + 1) * W - 1) / 2
    t1 = ((float(th[1, 0]) * xn0 + float(th[1, 1]) * yn0 + float(th[1, 2]) + 1) * H - 1) / 2
    r00, r01, r10, r11 = m11 / det, -m01 / det, -m10 / det, m00 / det
    ej, ei = abs(r00) + abs(r01) + 1e-2, abs(r10) + abs(r11) + 1e-2
    wj = wi = 0
    for y in range(H):
        for x in range(W):
            qj, qi = r00 * (x - t0) + r01 * (y - t1), r10 * (x - t0) + r11 * (y - t1)
            jlo, jhi = max(math.ceil(qj - ej), 0), min(math.floor(qj + ej), W - 1)
            ilo, ihi = max(math.ceil(qi - ei), 0), min(math.floor(qi + ei), H - 1)
            if jhi >= jlo and ihi >= ilo:
                wj, wi = max(wj, jhi - jlo), max(wi, ihi - ilo)
    return wj, wi


# ====================================================================================================== upsample + concat, zero insertion (exact)
def upcat_ref(lo, skip):
    N, H, W, C0 = lo.shape
    return torch.cat((lo[:, :, None, :, None, :].expand(N, H, 2, W, 2, C0).reshape(N, 2 * H, 2 * W, C0), skip), 3)


def upcat_backward_ref(dcat, C0):
    """-> (d_lo = the 2 x 2 sums in float64 rounded ONCE to bf16, d_skip = the slice)."""
    N, H2, W2, _ = dcat.shape
    s = dcat[..., :C0].to(F64).reshape(N, H2 // 2, 2, W2 // 2, 2, C0).sum((2, 4))
    return s.to(BF16), dcat[..., C0:].contiguous()


def zero_insert_ref(dy):
    N, Ho, Wo, C = dy.shape
    out = torch.zeros((N, 2 * Ho, 2 * Wo, C), dtype=dy.dtype)
    out[:, ::2, ::2] = dy
    return out


UPCAT_CASES = [(1, 1, 1, 8, 8), (2, 3, 5, 8, 24), (3, 8, 24, 64, 32), (1, 5, 7, 136, 8), (2, 16, 16, 512, 256), (1, 7, 9, 24, 2048)]      # N, H, W, C0, C1
ZERO_INSERT_CASES = [(1, 1, 1, 8), (2, 5, 7, 136), (3, 16, 32, 64), (1, 3, 3, 2048)]


def grid_values(shape, g):
    """bf16 values k / 64, |k| <= 2^14: any sum of four is exact in fp32 and in float64, so the 2 x 2 sums round once whatever the order."""
    return (torch.randint(-(1 << 14), (1 << 14) + 1, shape, generator=g).to(torch.float32) / 64.0).to(BF16).to(torch.float32).to(BF16)


# ====================================================================================================== detection loss
def det_loss_ref64(cls, lab, loc, tgt, mask, alpha, beta, n_maps=None):
    """The formulas at the head of csrc/det_loss.hip in float64.  cls, lab (n, 2); loc, tgt (n, 6); mask (n,) bool.  The normaliser is
    max(sum l_1, 1) (train/loss.py "positives") or, with n_maps, the number of maps ("batch").  -> dict: loss, cls_loss, loc_loss, n_pos
    (clamped), norm, and the pieces the gradients need."""
    c, l, x, t = cls.to(F64), lab.to(F64), loc.to(F64), tgt.to(F64)
    logp = c - torch.logsumexp(c, 1, keepdim=True)
    p = logp.exp()
    pt = (p * l).sum(1)
    s = (logp * l).sum(1)
    alpha_t = l[:, 1] * alpha + l[:, 0] * (1 - alpha)
    cls_sum = (-alpha_t * (1 - pt) ** 2 * s).sum()
    d = (x - t).abs()
    per = torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta)
    loc_sum = (per.sum(1) * mask.to(F64)).sum()
    n_pos = l[:, 1].sum().clamp(min=1.0)
    norm = n_pos if n_maps is None else torch.tensor(float(n_maps), dtype=F64)
    return dict(loss=cls_sum / norm + loc_sum / norm, cls_loss=cls_sum / norm, loc_loss=loc_sum / norm, n_pos=n_pos, norm=norm)


def det_loss_grads_ref64(cls, lab, loc, tgt, mask, alpha, beta, norm, g_loss, g_cls, g_loc):
    """d (g_loss loss + g_cls cls_loss + g_loc loc_loss) / d cls and / d loc, written out (None gradient = 0):
        d cls_sum / d c_j = -alpha_t [ -2 (1 - p_t) p_j (l_j - p_t) s + (1 - p_t)^2 (l_j - p_j (l_0 + l_1)) ]
        d loc_sum / d x   = mask (|d| < beta ? d / beta : sign(d)),  d = x - t"""
    c, l, x, t = cls.to(F64), lab.to(F64), loc.to(F64), tgt.to(F64)
    g0 = 0.0 if g_loss is None else float(g_loss)
    gc = (g0 + (0.0 if g_cls is None else float(g_cls))) / float(norm)
    gl = (g0 + (0.0 if g_loc is None else float(g_loc))) / float(norm)
    logp = c - torch.logsumexp(c, 1, keepdim=True)
    p = logp.exp()
    pt = (p * l).sum(1, keepdim=True)
    s = (logp * l).sum(1, keepdim=True)
    alpha_t = (l[:, 1] * alpha + l[:, 0] * (1 - alpha))[:, None]
    L = l.sum(1, keepdim=True)
    dcls = gc * (-alpha_t) * (-2 * (1 - pt) * s * p * (l - pt) + (1 - pt) ** 2 * (l - p * L))
    d = x - t
    dloc = gl * mask.to(F64)[:, None] * torch.where(d.abs() < beta, d / beta, torch.sign(d))
    return dcls, dloc


def det_loss_f32(cls, lab, loc, tgt, mask, n_maps, normalizer, weights):
    """torch's fp32 evaluation: the PyTorch ops of train/loss.py::detection_loss (the specification the kernels are compared with in
    test_fused_detection_loss_equals_the_torch_ops) and their autograd; weights: the three incoming gradients (None = output unused)."""
    from v2x_sim_amd.train.loss import detection_loss
    n = cls.shape[0] // n_maps
    c = cls.float().view(n_maps, n, 2).clone().requires_grad_(True)
    x = loc.float().view(n_maps, n, 6).clone().requires_grad_(True)
    out = detection_loss({"cls": c, "loc": x}, lab.float().view(n_maps, n, 2), tgt.float().view(n_maps, n, 6), mask.view(n_maps, n, 1), normalizer=normalizer)
    total = sum(o * w for o, w in zip(out, weights) if w is not None)
    total.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad          # noqa: E731  (an output that is not used sends no gradient)
    return [o.detach() for o in out], zero(c).view(-1, 2), zero(x).view(-1, 6)


# mask: "none" / "all" / "sparse".  grads: the incoming gradients of (loss, cls_loss, loc_loss); None = that output is unused.
# reach: "fwd-" / "fwd+" = just below / above DL_MAX_BLOCKS x 2048 anchors (the forward's grid-stride loop wraps once more), "bwd+" = more than
# 4096 x 1024 anchors (the backward's grid wraps), "one-hot" = labels (1, 0) / (0, 1) only: the positive count is an exact integer.
DetCase = namedtuple("DetCase", "n n_maps normalizer mask grads reach seed")
DET_CASES = [
    DetCase(1, 1, "positives", "all", (1.0, 0.25, -0.5), ("one-hot",), 1),
    DetCase(1, 1, "batch", "none", (1.0, None, None), (), 2),
    DetCase(255, 3, "batch", "sparse", (1.0, 0.25, -0.5), (), 3),
    DetCase(255, 1, "positives", "all", (None, 1.0, None), ("one-hot",), 4),
    DetCase(257, 1, "positives", "sparse", (None, None, 1.0), (), 5),
    DetCase(257, 1, "batch", "none", (None, 0.5, 2.0), ("one-hot",), 6),
    DetCase(DL_MAX_BLOCKS * 2048 - 1, 1, "positives", "sparse", (1.0, None, None), ("fwd-", "one-hot"), 7),
    DetCase(DL_MAX_BLOCKS * 2048 + 1, 1, "positives", "sparse", (1.0, 0.25, -0.5), ("fwd+",), 8),
    DetCase(DL_MAX_BLOCKS * 2048 - 1, 1, "batch", "all", (1.0, None, -0.5), ("fwd-",), 9),
    DetCase(DL_MAX_BLOCKS * 2048 + 1, 1, "batch", "none", (1.0, 0.25, None), ("fwd+", "one-hot"), 10),
    DetCase(DL_BWD_MAX_BLOCKS * 1024 + 257, 1, "positives", "sparse", (1.0, 0.25, -0.5), ("fwd+", "bwd+", "one-hot"), 11),
    DetCase(DL_BWD_MAX_BLOCKS * 1024 + 257, 1, "batch", "sparse", (1.0, None, None), ("fwd+", "bwd+"), 12),
]
DET_ALPHA, DET_BETA = 0.25, 1.0 / 9.0


def det_case_id(c):
    return "n%d-maps%d-%s-%s-g%s" % (c.n, c.n_maps, c.normalizer, c.mask, "".join("0" if w is None else "1" for w in c.grads))


def make_det_case(c):
    """-> cls, lab (n, 2), loc, tgt (n, 6) fp32, mask (n,) bool.  Logits to +-80 and tied logits in the first anchors; label pairs (1, 0),
    (0, 1) and -- unless the case is "one-hot" -- (0, 0), (0.3, 0.7); |x - t| exactly beta (as the kernel receives it), one ulp below and
    above, and exactly 0 on the first selected anchors."""
    g = torch.Generator().manual_seed(9000 + c.seed)
    n = c.n
    cls = torch.randn(n, 2, generator=g) * 3.0
    special = torch.tensor([[80.0, -80.0], [-80.0, 80.0], [2.5, 2.5], [0.0, 0.0], [-80.0, -80.0], [80.0, 80.0], [40.0, -37.0], [-1.0, 1.0]])
    k = min(n, len(special))
    cls[:k] = special[:k]
    lab = torch.zeros(n, 2)
    pos = torch.rand(n, generator=g) < 0.05
    pos[:k] = torch.arange(k) % 2 == 0
    lab[:, 1] = pos.float()
    lab[:, 0] = 1.0 - lab[:, 1]
    if "one-hot" not in c.reach:
        kinds = torch.randint(0, 20, (n,), generator=g)
        lab[kinds == 0] = 0.0
        lab[kinds == 1] = torch.tensor([0.3, 0.7])
    loc = torch.randn(n, 6, generator=g) * 0.5
    tgt = torch.randn(n, 6, generator=g) * 0.4
    mask = {"none": torch.zeros(n, dtype=torch.bool), "all": torch.ones(n, dtype=torch.bool), "sparse": pos.clone()}[c.mask]
    if c.mask != "none":
        mask[:k] = True
    # the smooth-L1 switch: x - t must come out of the fp32 subtraction as exactly beta, its neighbours, and 0
    b = np.float32(DET_BETA)
    edge = torch.tensor([float(b), float(np.nextafter(b, np.float32(0))), float(np.nextafter(b, np.float32(1))), 0.0, -float(b), 1.0])
    tgt[:k] = 0.0
    loc[:k] = edge[None, :]
    return cls, lab, loc, tgt, mask


# ====================================================================================================== Adam
def adam_ref64(p, g, m, v, step, lr, beta1, beta2, eps, wd):
    """One step of torch.optim.Adam's documented arithmetic in float64: -> (p, m, v)."""
    p, g, m, v = p.to(F64), g.to(F64), m.to(F64), v.to(F64)
    if wd != 0:
        g = g + wd * p
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    return p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps), m, v


ADAM_SIZES = (4095, 4096, 4097, 1, 0, 3 * 4096 + 5)
# step: the step this call performs (1: the moments start at zero; 10^5: both bias corrections within 1e-43 of 1).  zero_grad: g = 0 everywhere.
AdamCase = namedtuple("AdamCase", "step wd device_lr zero_grad seed")
ADAM_CASES = [AdamCase(1, 0.0, False, False, 1), AdamCase(1, 0.01, True, False, 2), AdamCase(100000, 0.0, True, False, 3),
              AdamCase(100000, 0.01, False, False, 4), AdamCase(1, 0.0, True, True, 5), AdamCase(100000, 0.0, False, True, 6),
              AdamCase(7, 0.01, False, False, 7), AdamCase(7, 0.0, True, False, 8)]
ADAM_LR, ADAM_BETAS, ADAM_EPS = 3e-3, (0.9, 0.999), 1e-8


def adam_case_id(c):
    return "step%d-wd%g-%slr%s" % (c.step, c.wd, "dev" if c.device_lr else "host", "-g0" if c.zero_grad else "")


def make_adam_case(c):
    """-> per tensor (p, g, m, v) fp32; at step 1 the moments are zero (as torch initialises them), later they are a plausible state."""
    gen = torch.Generator().manual_seed(10000 + c.seed)
    out = []
    for n in ADAM_SIZES:
        p = torch.randn(n, generator=gen)
        g = torch.zeros(n) if c.zero_grad else torch.randn(n, generator=gen) * 0.1
        if c.step == 1:
            m, v = torch.zeros(n), torch.zeros(n)
        else:
            m, v = torch.randn(n, generator=gen) * 0.05, torch.rand(n, generator=gen) * 0.01
        out.append((p, g, m, v))
    return out

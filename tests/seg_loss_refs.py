"""float64 references, grid mirrors and the seeded case table of the segmentation-loss kernels (csrc/seg_loss.hip).  A plain helper module in the manner
of tests/train_refs.py: tests/test_seg_loss_refs_cpu.py checks the references against F.cross_entropy and autograd and that the table reaches what it
claims, without a GPU; tests/test_gpu_seg_loss.py holds the kernels to them.

The operation (train/loss.py::segmentation_loss):  valid_i = label_i < C,  w_i = valid_i (weight[label_i] or 1),  nll_i = logsumexp(x_i) - x_i[label_i],
num = sum w_i nll_i,  den = sum w_i,  loss = num / (den > 0 ? den : 1),  d loss / d x_ij = g w_i (softmax_ij - [j == label_i]) / den."""
from collections import namedtuple

import torch

import train_refs as R

F64 = torch.float64

# ====================================================================================================== grid mirrors (constants of csrc/seg_loss.hip)
SL_THREADS = 256
SL_FWD_PIX, SL_FWD_MAX_BLOCKS = 2048, 1024
SL_BWD_PIX, SL_BWD_MAX_BLOCKS = 1024, 2048
SL_PK_PIX, SL_PK_MAX_BLOCKS = 1024, 1024


def _grid(M, pix, cap):
    b = max(-(-M // pix), 1)
    return min(b, cap), b


def sl_fwd_blocks(M):
    """seg_loss.hip::sl_fwd_blocks -> (blocks, uncapped blocks)."""
    return _grid(M, SL_FWD_PIX, SL_FWD_MAX_BLOCKS)


def sl_bwd_blocks(M):
    """seg_loss.hip::sl_bwd_blocks -> (blocks, uncapped blocks)."""
    return _grid(M, SL_BWD_PIX, SL_BWD_MAX_BLOCKS)


def sl_pk_blocks(M):
    """seg_loss.hip::sl_pk_blocks -> (blocks, uncapped blocks)."""
    return _grid(M, SL_PK_PIX, SL_PK_MAX_BLOCKS)


def workspace_bytes(M, C, Cp):
    """v2x_seg_loss_workspace_size."""
    if M <= 0 or C < 4 or C > 32 or C % 4:
        return 0
    floats = sl_fwd_blocks(M)[0] * 2
    if Cp:
        if Cp < C or not R.chan8_ok(M, Cp):
            return 0
        floats = max(floats, sl_pk_blocks(M)[0] * C)
    return floats * 4


def fwd_run(M):
    """The longest run of terms one thread of the forward kernel adds."""
    return -(-M // (SL_THREADS * sl_fwd_blocks(M)[0]))


def pk_run(M):
    return -(-M // (SL_THREADS * sl_pk_blocks(M)[0]))


# ====================================================================================================== references
def pixel_weights64(labels, C, weight):
    lab = labels.long()
    valid = lab < C
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    w = valid.to(F64)
    if weight is not None:
        w = w * weight.to(F64)[safe]
    return w, safe, valid


def seg_loss_ref64(logits, labels, weight=None):
    """-> dict(loss, num, den, nll (M,), w (M,), p (M, C)) in float64.  logits (M, C) fp32, labels (M,) uint8, weight (C,) fp32 or None."""
    x = logits.to(F64)
    C = x.shape[1]
    w, safe, _ = pixel_weights64(labels, C, weight)
    lse = torch.logsumexp(x, dim=1)
    nll = lse - x.gather(1, safe[:, None])[:, 0]
    num, den = (w * nll).sum(), w.sum()
    return dict(loss=num / (den if float(den) > 0 else 1.0), num=num, den=den, nll=nll, w=w, p=torch.exp(x - lse[:, None]))


def seg_loss_grad_ref64(logits, labels, weight, g, ref=None):
    """The gradient formula written out: g w_i (softmax_ij - [j == label_i]) / den (den = 0: zeros).  -> (M, C) float64."""
    ref = ref or seg_loss_ref64(logits, labels, weight)
    C = logits.shape[1]
    _, safe, valid = pixel_weights64(labels, C, weight)
    onehot = torch.zeros_like(ref["p"]).scatter_(1, safe[:, None], 1.0) * valid.to(F64)[:, None]
    den = float(ref["den"])
    return (float(g) / (den if den > 0 else 1.0)) * ref["w"][:, None] * (ref["p"] - onehot)


def packed_ref64(grad64, Cp):
    """Form (b) of the float64 gradient: (the gradient rounded ONCE to bf16, channels C..Cp-1 zero -> (M, Cp) float64; per-channel sums (C,) float64)."""
    M, C = grad64.shape
    out = torch.zeros((M, Cp), dtype=F64)
    out[:, :C] = R.bf16r64(grad64)
    return out, grad64.sum(0)


def spec_f32(logits, labels, weight, g):
    """torch's own fp32 evaluation of the same operation (the written-out masked sums + autograd): -> (loss, num, den, gradient), fp32."""
    x = logits.clone().requires_grad_(True)
    C = x.shape[1]
    lab = labels.long()
    valid = lab < C
    safe = torch.where(valid, lab, torch.zeros_like(lab))
    w = valid.to(torch.float32)
    if weight is not None:
        w = w * weight[safe]
    nll = torch.logsumexp(x, dim=1) - x.gather(1, safe[:, None])[:, 0]
    num, den = (w * nll).sum(), w.sum()
    loss = num / torch.where(den > 0, den, torch.ones_like(den))
    (loss * float(g)).backward()
    return loss.detach(), num.detach(), den.detach(), x.grad


# ====================================================================================================== the case table
SegCase = namedtuple("SegCase", "M C Cp logits labels weight seed")
# logits: "sat" = N(0, 3^2) with about one row in 16 at +-60 and one in 16 at +-88 (saturated softmax: no NaN, no inf); "int" = every row one +88 among -88s
#         (softmax exactly one-hot: with g = den and integer weights every gradient is an integer)
# labels: "uniform" | "one_class" | "ignored30" (about 30 % ignored, half 255 and half C) | "all_ignored"
# weight: "none" | "random" (uniform in [0.1, 4]) | "zero_class" (ones, one class 0) | "int" (integers 0..3, for the "int" logits)
LABEL_KINDS = ("uniform", "one_class", "ignored30", "all_ignored")
WEIGHT_KINDS = ("none", "random", "zero_class")
SMALL_M = (1, 63, 64, 255, 257)
CLASSES = (4, 8, 12, 16, 32)
FWD_CAP_M = SL_FWD_PIX * SL_FWD_MAX_BLOCKS          # the largest M below the forward (and form (a)) cap: 2^21
PK_CAP_M = SL_PK_PIX * SL_PK_MAX_BLOCKS             # ... the packed backward's: 2^20


def r8(C):
    return (C + 7) // 8 * 8


def _cases():
    out = []
    for i, M in enumerate(SMALL_M):
        for ci, C in enumerate(CLASSES):
            out.append(SegCase(M, C, 32 if (i + ci) % 2 else r8(C), "sat", LABEL_KINDS[(i + ci) % 4], WEIGHT_KINDS[(2 * i + ci) % 3], 100 * i + ci))
    # more than one workgroup in every kernel, every class count, every label / weight kind once more
    for ci, C in enumerate(CLASSES):
        out.append(SegCase(5000 + 37 * ci, C, r8(C) if ci % 2 else 32, "sat", LABEL_KINDS[ci % 3], WEIGHT_KINDS[(ci + 1) % 3], 700 + ci))
    out.append(SegCase(4099, 8, 8, "sat", "all_ignored", "random", 720))
    # both sides of the three block caps (forward and form (a) share M = 2^21; the packed backward's is 2^20)
    # (the float64 reference of 2^21 pixels is most of such a case's time: four classes except for the largest case, uniform labels)
    out.append(SegCase(PK_CAP_M, 4, 8, "sat", "ignored30", "random", 801))
    out.append(SegCase(PK_CAP_M + 1, 4, 32, "sat", "uniform", "none", 802))
    out.append(SegCase(FWD_CAP_M, 4, 8, "sat", "uniform", "zero_class", 803))
    out.append(SegCase(FWD_CAP_M + 1, 8, 8, "sat", "uniform", "random", 804))
    # integer-valued gradients
    out.append(SegCase(257, 8, 8, "int", "uniform", "int", 901))
    out.append(SegCase(5003, 12, 16, "int", "ignored30", "none", 902))
    out.append(SegCase(70001, 32, 32, "int", "uniform", "int", 903))
    out.append(SegCase(PK_CAP_M + 1, 4, 8, "int", "ignored30", "int", 904))
    return out


SEG_CASES = _cases()


def case_id(c):
    return "M%d-C%d-Cp%d-%s-%s-%s" % (c.M, c.C, c.Cp, c.logits, c.labels, c.weight)


def make_case(c):
    """-> (logits (M, C) fp32, labels (M,) uint8, weight (C,) fp32 or None), seeded."""
    g = torch.Generator().manual_seed(1000 + c.seed)
    M, C = c.M, c.C
    if c.logits == "int":
        hot = torch.randint(0, C, (M,), generator=g)
        x = torch.full((M, C), -88.0).scatter_(1, hot[:, None], 88.0)
    else:
        x = torch.randn(M, C, generator=g) * 3.0
        sel = torch.randint(0, 16, (M,), generator=g)
        signs = torch.randint(0, 2, (M, C), generator=g).float() * 2 - 1
        x = torch.where((sel == 0)[:, None], signs * 60.0, x)
        x = torch.where((sel == 1)[:, None], signs * 88.0, x)
    if c.labels == "one_class":
        lab = torch.full((M,), int(torch.randint(0, C, (1,), generator=g)))
    else:
        lab = torch.randint(0, C, (M,), generator=g)
    if c.labels == "ignored30":
        u = torch.rand(M, generator=g)
        lab = torch.where(u < 0.15, torch.full_like(lab, 255), lab)
        lab = torch.where((u >= 0.15) & (u < 0.30), torch.full_like(lab, C), lab)
    elif c.labels == "all_ignored":
        lab = torch.where(torch.rand(M, generator=g) < 0.5, torch.full_like(lab, 255), torch.full_like(lab, C))
    if c.weight == "none":
        w = None
    elif c.weight == "random":
        w = torch.rand(C, generator=g) * 3.9 + 0.1
    elif c.weight == "zero_class":
        w = torch.ones(C)
        w[int(torch.randint(0, C, (1,), generator=g))] = 0.0
    else:
        w = torch.randint(0, 4, (C,), generator=g).float()
    return x.contiguous(), lab.to(torch.uint8), w

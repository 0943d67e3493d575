"""float64 reference and the seeded case list for the sparsemax form of the handshake (v2x_attn_handshake_norm, norm = 1).  A plain helper
module in the style of tests/fusion_refs.py, whose score reference it imports: tests/test_attn_sparse_refs_cpu.py checks the reference and
every condition the case list must satisfy without a GPU, tests/test_gpu_attn_sparse.py holds the kernel to them.

Sparsemax of a score column z over the A keys: sorted descending z_(1) >= ... >= z_(A),
k* = max{ j : 1 + j z_(j) > sum_{i<=j} z_(i) }, tau = (sum_{i<=k*} z_(i) - 1) / k*, p_k = max(z_k - tau, 0)."""
import itertools
from collections import namedtuple

import torch

import fusion_refs as FR

ATTN_THRES_MARGIN, ATTN_GAP = FR.ATTN_THRES_MARGIN, FR.ATTN_GAP


def prob_bar(scores):
    """The GPU bar on prob: 4 x the softmax bar of test_attn_handshake_sweep (1e-5 * max(1, max |score| / 8)): a row of sparsemax's Jacobian has
    l1-norm below 2 (inside the support dp_k / dz_l = [k = l] - 1 / k*), a row of softmax's at most 1/2."""
    return 4e-5 * max(1.0, float(scores.abs().max()) / 8.0)


TAU_MARGIN_BARS = 8            # every reference |z_k - tau| is at least this many bars: a score error of the bar's size cannot move a key in or out


def sparsemax_ref64(scores):
    """scores (Bt, A_key, A_query) float64 -> (prob, tau (Bt, 1, A_query), support size (Bt, A_query)), column by column as the definition reads."""
    Bt, A, _ = scores.shape
    prob = torch.zeros_like(scores)
    tau = torch.zeros((Bt, 1, A), dtype=torch.float64)
    size = torch.zeros((Bt, A), dtype=torch.int64)
    for f in range(Bt):
        for q in range(A):
            z = scores[f, :, q]
            srt = sorted(z.tolist(), reverse=True)
            kstar, cum, csum = 0, 0.0, 0.0
            for j in range(1, A + 1):
                cum += srt[j - 1]
                if 1.0 + j * srt[j - 1] > cum:
                    kstar, csum = j, cum
            t = (csum - 1.0) / kstar
            tau[f, 0, q] = t
            size[f, q] = kstar
            prob[f, :, q] = (z - t).clamp(min=0)
    return prob, tau, size


def sparsemax_handshake_ref64(keys, querys, w, b, A, Bt, mode, thres=0.2):
    """As fusion_refs.attn_handshake_ref64 with sparsemax over the keys -> scores, prob, coef (each (Bt, A_key, A_query) float64), tau, support
    size.  The selections act on prob as there; 'argmax_test' is the one-hot of the FIRST maximal probability."""
    scores = FR.attn_handshake_ref64(keys, querys, w, b, A, Bt, "softmax")[0]
    prob, tau, size = sparsemax_ref64(scores)
    if mode == "softmax":
        coef = prob.clone()
    elif mode == "activated":
        coef = prob * (prob > thres).to(torch.float64)
    elif mode == "argmax_test":
        coef = torch.zeros_like(prob)
        for f in range(Bt):
            for q in range(A):
                col = prob[f, :, q].tolist()
                coef[f, col.index(max(col)), q] = 1.0
    else:
        raise ValueError(mode)
    return scores, prob, coef, tau, size


def simplex_projection_brute(z):
    """The Euclidean projection of the vector z (float64, at most a handful of entries) onto the probability simplex by enumeration: for every
    non-empty support S the point p_S = z_S - (sum z_S - 1) / |S| (zero outside S) is the projection onto the face's affine hull; the
    projection onto the simplex is the feasible one (p_S >= 0) nearest to z."""
    A = z.numel()
    best, best_d = None, float("inf")
    for n in range(1, A + 1):
        for S in itertools.combinations(range(A), n):
            idx = torch.tensor(S)
            p = torch.zeros_like(z)
            p[idx] = z[idx] - (z[idx].sum() - 1.0) / n
            if float(p.min()) < 0:
                continue
            d = float((p - z).square().sum())
            if d < best_d:
                best, best_d = p, d
    return best


SparseCase = FR.AttnCase       # A Bt K Q scale tie thres
SPARSE_CASES = [c for c in FR.ATTN_CASES if c.scale == 1.0 and c.tie is None and c.thres == 0.2] + [      # the shapes: A = 1, 5, 8, 9, 32, ...
    SparseCase(5, 2, 1024, 32, 0.3, None, 0.2),        # key scales 0.3 .. 0.03: the score gaps shrink below 1 and the supports grow to A
    SparseCase(5, 2, 1024, 32, 0.1, None, 0.2),
    SparseCase(5, 2, 1024, 32, 0.03, None, 0.2),
    SparseCase(9, 2, 1024, 32, 0.3, None, 0.2),
    SparseCase(9, 2, 1024, 32, 0.1, None, 0.2),
    SparseCase(9, 2, 1024, 32, 0.03, None, 0.2),
    SparseCase(5, 2, 1024, 32, 30.0, None, 0.2),       # max |score| ~ 2e2 and ~ 2.6e3: the sums must be taken after the shift
    SparseCase(5, 2, 1024, 32, 300.0, None, 0.2),
    SparseCase(5, 2, 1024, 32, 1.0, (1, 3), 0.2),      # a designed tie: both keys get 0.5, the first wins 'argmax_test'
    SparseCase(5, 2, 1024, 32, 0.3, None, 0.05),       # thres passed explicitly
]
sparse_case_id = FR.attn_case_id


def sparse_conditions(c, scores, prob, tau):
    """-> (smallest |z_k - tau| in bars of prob_bar, smallest |p - thres| over the non-zero p, relative top-two gap, the designed tie holds)."""
    tau_margin = float((scores - tau).abs().min()) / prob_bar(scores)
    nz = prob[prob > 0]
    thres_margin = float((nz - c.thres).abs().min())
    _, gap, tie_ok = FR.attn_conditions(c, scores, prob)
    return tau_margin, thres_margin, gap, tie_ok


def make_sparse_case(c, index):
    """Inputs drawn as fusion_refs.make_attn_case draws them (the designed tie included), redrawn (next seed) until the conditions of
    sparse_conditions hold: |z - tau| >= TAU_MARGIN_BARS bars everywhere, non-zero probabilities ATTN_THRES_MARGIN from the threshold, the
    top-two gap rule of ATTN_GAP.  tests/test_attn_sparse_refs_cpu.py asserts them on what is returned."""
    for attempt in range(64):
        g = torch.Generator().manual_seed(7000 + 100 * index + attempt)
        keys = torch.randn(c.A * c.Bt, c.K, generator=g) * 0.3 * c.scale
        querys = torch.randn(c.A * c.Bt, c.Q, generator=g)
        w = torch.randn(c.K, c.Q, generator=g) * 0.05
        b = torch.randn(c.K, generator=g) * 0.05
        if c.tie:
            k1, k2 = c.tie
            s0 = FR.attn_handshake_ref64(keys, querys, w, b, c.A, c.Bt, "softmax")[0]
            q64 = querys.double().view(c.A, c.Bt, -1).transpose(0, 1)
            qp = q64 @ w.double().T + b.double()                                   # (Bt, A, K)
            for f in range(c.Bt):
                top = 2.0 * float(s0[f].abs().max()) + 1.0
                x = torch.linalg.pinv(qp[f]) @ torch.full((c.A,), top, dtype=torch.float64)
                keys[k1 * c.Bt + f] = x.float()
                keys[k2 * c.Bt + f] = keys[k1 * c.Bt + f]
        scores, prob, _, tau, _ = sparsemax_handshake_ref64(keys, querys, w, b, c.A, c.Bt, "softmax")
        tau_margin, thres_margin, gap, tie_ok = sparse_conditions(c, scores, prob, tau)
        if tau_margin >= TAU_MARGIN_BARS and thres_margin >= ATTN_THRES_MARGIN and gap >= ATTN_GAP and tie_ok:
            return keys, querys, w, b
    raise AssertionError("no draw of %s satisfies the conditions" % (c,))

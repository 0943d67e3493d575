"""The sparsemax form of the handshake kernel (csrc/attention.hip, v2x_attn_handshake_norm with norm = 1) swept over the case list of
tests/attn_sparse_refs.py against its float64 reference -- seeded, the same cases every run; tests/test_attn_sparse_refs_cpu.py checks the
reference and the conditions the equalities below rest on (every |z - tau| at least 8 bars, non-zero probabilities 1e-3 from the threshold,
top-two gaps above rounding).

prob is held at 4e-5 * max(1, max |score| / 8): the softmax bar of test_attn_handshake_sweep times 4 (a row of sparsemax's Jacobian has l1-norm
below 2, a row of softmax's at most 1/2).  Each case prints its worst error as a fraction of the bar (pytest -s shows them).

First run on 1x MI355X (the module: 2.6 s wall, float64 references included), worst error / bar: 0.024 (A = 6, |prob - fp64| 9.7e-7, max |score|
6.6); 0.013 - 0.014 at A = 5 .. 9 and key scale 1; 0.001 - 0.007 at key scales 0.3 .. 0.03 (supports of up to 9 keys); exact (0) where the support
is one key -- A = 1, the 30x and 300x scales (max |score| 2.4e3) -- and in the designed tie (0.5 | 0.5)."""
import ctypes as C
import functools

import pytest
import torch

import attn_sparse_refs as SR
import fusion_refs as FR

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(index):
    c = SR.SPARSE_CASES[index]
    keys, querys, w, b = SR.make_sparse_case(c, index)
    return keys, querys, w, b, SR.sparsemax_handshake_ref64(keys, querys, w, b, c.A, c.Bt, "softmax")


@pytest.mark.parametrize("index", range(len(SR.SPARSE_CASES)), ids=[SR.sparse_case_id(c) for c in SR.SPARSE_CASES])
def test_attn_handshake_sparsemax_sweep(device, index):
    from v2x_sim_amd import ops
    c = SR.SPARSE_CASES[index]
    keys, querys, w, b, (scores, prob, _, tau, size) = _case(index)
    tol = SR.prob_bar(scores)
    d = lambda t: t.to(device)                                                     # noqa: E731
    kw = {} if c.thres == 0.2 else {"thres": c.thres}
    p0, c0 = ops.attn_handshake(d(keys), d(querys), d(w), d(b), c.A, c.Bt, "softmax", norm="sparsemax")
    assert torch.equal(p0, c0)                                                     # 'softmax' selection: coef is prob, bit for bit
    p0 = p0.cpu()
    assert bool(torch.isfinite(p0).all()) and bool((p0 >= 0).all())
    err = float((p0.double() - prob).abs().max())
    print("attn_handshake sparsemax %-30s max|score| %.3e  support %d..%d  max|prob - fp64| %.3e  worst/bar %.3f"
          % (SR.sparse_case_id(c), float(scores.abs().max()), int(size.min()), int(size.max()), err, err / tol))
    assert err <= tol, (err, tol)
    assert torch.equal(p0 > 0, prob > 0), "the support differs from the reference's"
    assert float((p0.double().sum(1) - 1).abs().max()) <= 1e-5                     # every column (query) sums to 1
    p1, c1 = ops.attn_handshake(d(keys), d(querys), d(w), d(b), c.A, c.Bt, "activated", norm="sparsemax", **kw)
    p1, c1 = p1.cpu(), c1.cpu()
    ref_sel = prob > c.thres
    assert torch.equal(p1, p0)
    assert torch.equal(c1 != 0, ref_sel), "the 'activated' selection differs from the reference's"
    assert torch.equal(c1[ref_sel], p1[ref_sel]) and float(c1[~ref_sel].abs().sum()) == 0
    p2, c2 = ops.attn_handshake(d(keys), d(querys), d(w), d(b), c.A, c.Bt, "argmax_test", norm="sparsemax")
    ref_arg = SR.sparsemax_handshake_ref64(keys, querys, w, b, c.A, c.Bt, "argmax_test")[2]
    assert torch.equal(p2.cpu(), p0)
    assert torch.equal(c2.cpu().double(), ref_arg), "the arg-max key differs from the reference's (ties: the first maximum wins)"
    if c.tie:
        k1, k2 = c.tie
        assert bool((p0[:, k1] == 0.5).all()) and bool((p0[:, k2] == 0.5).all())   # the tied pair shares the column
        assert bool((c2.cpu()[:, k1] == 1).all())
    # a second launch gives the same bits
    assert torch.equal(ops.attn_handshake(d(keys), d(querys), d(w), d(b), c.A, c.Bt, "softmax", norm="sparsemax")[0].cpu(), p0)


def _norm_entry(keys, querys, w, b, A, Bt, mode, norm, thres=0.2):
    """v2x_attn_handshake_norm called directly (ops.attn_handshake sends "softmax" to the old entry)."""
    from v2x_sim_amd import _lib, ops
    lib = _lib.load()
    prob = torch.full((Bt, A, A), float("nan"), dtype=torch.float32, device=keys.device)
    coef = torch.full_like(prob, float("nan"))
    rc = lib.v2x_attn_handshake_norm(ops._dev(keys, torch.float32, "keys"), ops._dev(querys, torch.float32, "querys"), ops._dev(w, torch.float32, "w"),
                                     ops._dev(b, torch.float32, "b"), A, Bt, keys.shape[1], querys.shape[1], ops.ATTN_MODES[mode], norm, C.c_float(thres),
                                     ops._dev(prob, torch.float32, "prob"), ops._dev(coef, torch.float32, "coef"), ops._stream())
    return rc, prob, coef


@pytest.mark.parametrize("index", range(len(FR.ATTN_CASES)), ids=[FR.attn_case_id(c) for c in FR.ATTN_CASES])
def test_norm_entry_with_norm_0_is_the_old_entry(device, index):
    """On the inputs of test_attn_handshake_sweep the new entry with norm = 0 returns the bits of v2x_attn_handshake, in every mode."""
    from v2x_sim_amd import ops
    c = FR.ATTN_CASES[index]
    keys, querys, w, b = (t.to(device) for t in FR.make_attn_case(c, index))
    for mode in ("softmax", "activated", "argmax_test"):
        p_old, c_old = ops.attn_handshake(keys, querys, w, b, c.A, c.Bt, mode, thres=c.thres)
        rc, p_new, c_new = _norm_entry(keys, querys, w, b, c.A, c.Bt, mode, 0, c.thres)
        assert rc == 0
        assert torch.equal(p_new, p_old) and torch.equal(c_new, c_old), mode


def test_norm_entry_argument_errors(device):
    from v2x_sim_amd import _lib
    c = FR.ATTN_CASES[0]
    keys, querys, w, b = (t.to(device) for t in FR.make_attn_case(c, 0))
    for norm in (-1, 2):
        rc, prob, _ = _norm_entry(keys, querys, w, b, c.A, c.Bt, "softmax", norm)
        assert rc == -22 and bool(torch.isnan(prob).all())                          # refused before any launch
    # A = 32 with K = 1024: the staging (and norm = 1's sorted copy) exceeds the 64 KiB check -> the argument error, no launch
    big = torch.zeros(32, 1024, device=device)
    rc, _, _ = _norm_entry(big, torch.zeros(32, 32, device=device), w, b, 32, 1, "softmax", 1)
    assert rc == -22
    # the sorted copy is counted: A = 32, Q = 32, K = 447 stages (32 * 447 + 1024 + 1024) * 4 = 65 408 bytes -- under the 65 536 of the check, and
    # norm = 0 launches; norm = 1 adds A * A floats (69 504 bytes) and is refused, nothing written
    g = torch.Generator().manual_seed(447)
    k447, q32 = (torch.randn(32, 447, generator=g) * 0.3).to(device), torch.randn(32, 32, generator=g).to(device)
    w447, b447 = (torch.randn(447, 32, generator=g) * 0.05).to(device), (torch.randn(447, generator=g) * 0.05).to(device)
    rc, prob, _ = _norm_entry(k447, q32, w447, b447, 32, 1, "softmax", 0)
    assert rc == 0 and float((prob.sum(1) - 1).abs().max()) <= 1e-5
    rc, prob, _ = _norm_entry(k447, q32, w447, b447, 32, 1, "softmax", 1)
    assert rc == -22 and bool(torch.isnan(prob).all())
    assert _lib.load().v2x_abi_version() == 18

"""The sparsemax handshake reference of tests/attn_sparse_refs.py, the conditions its case list must satisfy (tests/test_gpu_attn_sparse.py rests
its equalities on them) and the differentiable torch sparsemax of train/graph.py -- all on the CPU."""
import functools

import pytest
import torch

import attn_sparse_refs as SR

_IDS = [SR.sparse_case_id(c) for c in SR.SPARSE_CASES]


@functools.lru_cache(maxsize=None)
def _case(index):
    c = SR.SPARSE_CASES[index]
    keys, querys, w, b = SR.make_sparse_case(c, index)
    return (keys, querys, w, b) + SR.sparsemax_handshake_ref64(keys, querys, w, b, c.A, c.Bt, "softmax")


def test_case_table_covers_the_shapes_and_scales():
    cs = SR.SPARSE_CASES
    assert {1, 5, 8, 9, 32} <= {c.A for c in cs}
    assert any(c.Q != 32 for c in cs) and any(c.K % 64 != 0 for c in cs)               # the generic projection; K no multiple of 64
    for A in (5, 9):
        assert {1.0, 0.3, 0.1, 0.03} <= {c.scale for c in cs if c.A == A}
    assert {30.0, 300.0} <= {c.scale for c in cs}
    assert any(c.tie for c in cs) and any(c.thres != 0.2 for c in cs)


@pytest.mark.parametrize("index", range(len(SR.SPARSE_CASES)), ids=_IDS)
def test_case_conditions(index):
    c = SR.SPARSE_CASES[index]
    keys, querys, w, b, scores, prob, coef, tau, size = _case(index)
    tau_margin, thres_margin, gap, tie_ok = SR.sparse_conditions(c, scores, prob, tau)
    assert tau_margin >= SR.TAU_MARGIN_BARS, tau_margin
    assert thres_margin >= SR.ATTN_THRES_MARGIN and gap >= SR.ATTN_GAP and tie_ok
    assert float((prob.sum(1) - 1).abs().max()) <= 1e-12                              # every column sums to 1
    assert torch.equal((prob > 0).sum(1), size) and bool((prob >= 0).all())
    assert torch.equal(coef, prob)
    if c.tie:
        k1, k2 = c.tie
        assert bool((prob[:, k1] == 0.5).all()) and bool((prob[:, k2] == 0.5).all())
        arg = SR.sparsemax_handshake_ref64(keys, querys, w, b, c.A, c.Bt, "argmax_test")[2]
        assert bool((arg[:, k1] == 1).all())                                          # the first of the tied keys
    act = SR.sparsemax_handshake_ref64(keys, querys, w, b, c.A, c.Bt, "activated", c.thres)[2]
    assert torch.equal(act != 0, prob > c.thres) and torch.equal(act[act != 0], prob[act != 0])


def test_support_sizes_across_the_table():
    sizes, full, onehot = set(), False, False
    for i, c in enumerate(SR.SPARSE_CASES):
        size = _case(i)[8]
        sizes |= set(size.flatten().tolist())
        if c.A > 1:
            full = full or bool((size == c.A).any())
            onehot = onehot or bool((size == 1).any())
    assert {1, 2, 3, 4, 5} <= sizes, sorted(sizes)
    assert full and onehot


@pytest.mark.parametrize("index", [i for i, c in enumerate(SR.SPARSE_CASES) if c.A <= 5],
                         ids=[SR.sparse_case_id(c) for c in SR.SPARSE_CASES if c.A <= 5])
def test_reference_is_the_projection_onto_the_simplex(index):
    c = SR.SPARSE_CASES[index]
    scores, prob = _case(index)[4:6]
    for f in range(c.Bt):
        for q in range(c.A):
            brute = SR.simplex_projection_brute(scores[f, :, q])
            assert float((brute - prob[f, :, q]).abs().max()) <= 1e-12 * max(1.0, float(scores.abs().max()))


@pytest.mark.parametrize("index", range(len(SR.SPARSE_CASES)), ids=_IDS)
def test_graph_sparsemax_equals_reference(index):
    from v2x_sim_amd.train.graph import sparsemax
    scores, prob = _case(index)[4:6]
    got = sparsemax(scores, 1)
    assert got.dtype == torch.float64
    assert float((got - prob).abs().max()) <= 1e-12 * max(1.0, float(scores.abs().max()))
    assert torch.equal(got > 0, prob > 0)


def test_graph_sparsemax_gradcheck():
    from v2x_sim_amd.train.graph import sparsemax
    index = next(i for i, c in enumerate(SR.SPARSE_CASES) if c.A == 5 and c.scale == 0.3 and c.thres == 0.2)   # supports of several sizes
    scores = _case(index)[4].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda z: sparsemax(z, 1), (scores,), eps=1e-6, atol=1e-6)
    lead = torch.randn(3, 5, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(1))                # another dim, other extents
    assert float((sparsemax(lead, 1).sum(1) - 1).abs().max()) <= 1e-12
    assert float((sparsemax(lead, 2).sum(2) - 1).abs().max()) <= 1e-12

"""tests/channel_refs.py checked on its own, without a GPU: the generator against its published vectors, and the draws' elementary properties."""
import math

import numpy as np

import channel_refs as CR


def test_philox_known_answer_vectors():
    for counter, key, want in CR.KATS:
        assert CR.philox4x32_10(counter, key) == want


def test_counter_layout():
    seed, step = CR.BIG_SEED, (5 << 32) | 9
    assert CR.words(seed, step, 3, 1, 2, 4) == CR.philox4x32_10((9, 5, 3, (1 << 16) | (2 << 8) | 4), (seed & CR.M32, seed >> 32))


def test_p0_and_p1():
    items, coef0 = CR.static_plan([5, 3], 5)
    coef, coef2, link = CR.rewrite_plan(items, coef0, 5, 2, 3, 0, 0.0)
    assert np.array_equal(coef, coef0)
    assert int(link.sum()) == 5 * 4 + 3 * 2 and not link[1, 3:].any() and not link[1, :, 3:].any()
    coef, coef2, link = CR.rewrite_plan(items, coef0, 5, 2, 3, 0, 1.0)
    assert not link.any()
    for m, (a, f) in enumerate(items):
        assert coef[m].tolist() == [1.0 if j == a else 0.0 for j in range(5)]           # every ego fuses its own map only
    assert np.array_equal(coef2.reshape(len(items), 5, 5).sum(1), coef) and np.array_equal(coef2.reshape(len(items), 5, 5).sum(2), coef)
    # u < 1 always, u >= 0 always
    assert all(CR.link_down(1, s, 0, 0, 1, 1.0) and not CR.link_down(1, s, 0, 0, 1, 0.0) for s in range(64))


def test_deterministic_and_steps_differ():
    a = CR.links_up(8, 5, 42, 6, 0.3)
    assert np.array_equal(a, CR.links_up(8, 5, 42, 6, 0.3))
    assert not np.array_equal(a, CR.links_up(8, 5, 42, 7, 0.3))
    assert not np.array_equal(a, CR.links_up(8, 5, 43, 6, 0.3))
    assert CR.normals(42, 6, 0, 1, 2) == CR.normals(42, 6, 0, 1, 2) != CR.normals(42, 7, 0, 1, 2)
    # the carry: step 2^32 is not step 0
    assert CR.words(1, 1 << 32, 0, 0, 0, 1) != CR.words(1, 0, 0, 0, 0, 1)
    # outage and pose are drawn apart
    assert CR.words(1, 0, 0, 0, 0, 1) != CR.words(1, 0, 0, 1, 0, 1)


def test_directions_are_drawn_apart():
    L = CR.links_up(128, 5, 9, 0, 0.3)
    assert any(L[f, i, j] != L[f, j, i] for f in range(128) for i in range(5) for j in range(i))
    assert CR.words(9, 0, 0, 0, 1, 2) != CR.words(9, 0, 0, 0, 2, 1)


def test_realised_outage_rate():
    """128 frames x 5 agents, p = 0.3, steps 0..3: 2 560 directed pairs per step, 768 +- 4 sigma (sigma = sqrt(2560 * 0.3 * 0.7) = 23.2)."""
    got = []
    for s in range(4):
        down = int((~CR.links_up(128, 5, 2024, s, 0.3)).sum())
        got.append(down)
        assert abs(down - 768) <= 93, (s, down)
    print("links down of 2560 at steps 0..3:", got)
    assert len(set(got)) > 1


def test_normals_mean_and_variance():
    """The same pairs: n = 2 560 samples per component and step.  Mean within 4 / sqrt(n), variance within 4 sqrt(2 / n) of 1."""
    for s in range(4):
        t = CR.noise_table(128, 5, 2024, s)
        off = ~np.eye(5, dtype=bool)
        for c in range(3):
            v = t[:, off, c].reshape(-1)
            assert v.size == 2560
            assert abs(v.mean()) <= 4.0 / math.sqrt(v.size), (s, c, v.mean())
            assert abs(v.var() - 1.0) <= 4.0 * math.sqrt(2.0 / v.size), (s, c, v.var())
            assert np.abs(v).max() <= 5.77
        assert not t[:, np.eye(5, dtype=bool)].any()


def test_uniform_ranges():
    assert CR.outage_uniform(0) == 0.0 and CR.outage_uniform(CR.M32) == 1.0 - 2.0 ** -24
    assert CR.pose_uniforms((0, CR.M32, 0, 0))[:2] == (2.0 ** -24, 1.0 - 2.0 ** -24)
    assert math.sqrt(-2.0 * math.log(2.0 ** -24)) < 5.77


def test_find_isolated_and_case_table():
    s = CR.find_isolated([3, 2], 3, 0.5, 77, ego=(0, 0))
    L = CR.links_up(2, 3, 77, s, 0.5)
    assert not L[0, 0, 1] and not L[0, 0, 2] and (L[0, 1, 0] or L[0, 1, 2]) and L[1, 0, 1] and L[1, 1, 0]
    names = [c["name"] for c in CR.CASES]
    assert len(set(names)) == len(names)
    assert {c["A"] for c in CR.CASES} == {1, 2, 5, 32} and {c["Bt"] for c in CR.CASES} == {1, 3, 130}
    assert {c["p"] for c in CR.CASES} == {0.0, 0.3, 1.0} and {c["sigma"] for c in CR.CASES} == {0.0, 0.5}
    assert any(c["seed"] >= 1 << 32 for c in CR.CASES) and any(c["step"] == (1 << 32) - 1 for c in CR.CASES)
    assert any(c["only_v2i"] for c in CR.CASES) and any(c["outputs"] == "bare" for c in CR.CASES)
    assert any(min(c["counts"]) < c["A"] for c in CR.CASES)

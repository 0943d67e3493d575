"""Reference for the degraded-link draw (csrc/channel.hip, csrc/channel_math.h), written from the definitions in plain
Python integers and float64 -- not derived from the header.

* philox4x32_10: Salmon et al. 2011, ten rounds; KATS are the three published known-answer vectors.
* words(seed, step, f, domain, i, j): counter (step & 0xffffffff, step >> 32, f, (domain << 16) | (i << 8) | j), key (seed & 0xffffffff, seed >> 32).
* Outage (domain 0): u = (w[0] >> 8) * 2^-24; link j -> i is down iff u < float32(p).
* Pose (domain 1): u_k = ((w[k] >> 9) + 0.5) * 2^-23; nx = sqrt(-2 ln u_0) cos(2 pi u_1), ny = ... sin(2 pi u_1), nz = sqrt(-2 ln u_2) cos(2 pi u_3).
* static_plan / rewrite_plan: the plan tensors of the fusion family, DiscoNet and V2VNet, and this step's rows of them.
* CASES: the shapes, agent tables and conditions the kernel is held to (tests/test_gpu_channel.py) and the host driver prints
  (tests/test_channel_math_cpu.py).
* v2v_zero_message: the oracle's OWN V2VNet operations composed with a zero message for an ego without a live link (oracle/ is frozen; the
  pattern of tests/codec_refs.py).
"""
import math

import numpy as np

M32 = 0xFFFFFFFF
DOMAIN_OUTAGE, DOMAIN_POSE = 0, 1

KATS = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((M32, M32, M32, M32), (M32, M32), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return (c0, c1, c2, c3)


def words(seed, step, f, domain, i, j):
    assert 0 <= seed < 1 << 64 and 0 <= step < 1 << 64 and 0 <= i < 32 and 0 <= j < 32
    return philox4x32_10((step & M32, step >> 32, f, (domain << 16) | (i << 8) | j), (seed & M32, seed >> 32))


def outage_uniform(w0):
    return (w0 >> 8) / float(1 << 24)            # exact: 24 bits


def link_down(seed, step, f, i, j, p):
    return outage_uniform(words(seed, step, f, DOMAIN_OUTAGE, i, j)[0]) < float(np.float32(p))


def pose_uniforms(w):
    return tuple(((x >> 9) + 0.5) / float(1 << 23) for x in w)        # exact: 24 bits, in (0, 1)


def normals(seed, step, f, i, j):
    ua, ub, uc, ud = pose_uniforms(words(seed, step, f, DOMAIN_POSE, i, j))
    ra, rc = math.sqrt(-2.0 * math.log(ua)), math.sqrt(-2.0 * math.log(uc))
    return (ra * math.cos(2.0 * math.pi * ub), ra * math.sin(2.0 * math.pi * ub), rc * math.cos(2.0 * math.pi * ud))


# ---- plans ---------------------------------------------------------------------------------------------------------------------------------
def items_of(counts, A):
    """Agent-major (ego, frame) pairs of the present agents: IntermediateModelBase.frame_plan's order."""
    return [(a, f) for a in range(A) for f in range(len(counts)) if a < counts[f]]


def static_plan(counts, A, kind="fusion", only_v2i=False):
    """-> (items, coef0 float32 (n, A)).  kind 'fusion': the ego and its linked neighbours (sum / mean / max / cat / DiscoNet); 'v2v': the linked
    neighbours only."""
    items = items_of(counts, A)
    coef = np.zeros((len(items), A), np.float32)
    for m, (a, f) in enumerate(items):
        for j in range(counts[f]):
            if j == a:
                coef[m, j] = 1.0 if kind == "fusion" else 0.0
            elif not only_v2i or a == 0 or j == 0:
                coef[m, j] = 1.0
    return items, coef


def rewrite_plan(items, coef0, A, Bt, seed, step, p):
    """-> (coef (n, A), coef2 (n * A, A), link uint8 (Bt, A, A)) of this step."""
    coef = coef0.copy()
    link = np.zeros((Bt, A, A), np.uint8)
    for m, (i, f) in enumerate(items):
        for j in range(A):
            if j != i and p > 0 and link_down(seed, step, f, i, j, p):
                coef[m, j] = 0.0
            if j != i and coef[m, j] != 0:
                link[f, i, j] = 1
    coef2 = np.zeros((len(items) * A, A), np.float32)
    for m in range(len(items)):
        for k in range(A):
            coef2[m * A + k, k] = coef[m, k]
    return coef, coef2, link


def links_up(Bt, A, seed, step, p):
    """bool (Bt, A, A): [f][i][j] = the link j -> i is NOT down at this step (diagonal True) -- what set_link_mask takes."""
    L = np.ones((Bt, A, A), bool)
    for f in range(Bt):
        for i in range(A):
            for j in range(A):
                if j != i and p > 0 and link_down(seed, step, f, i, j, p):
                    L[f, i, j] = False
    return L


def noise_table(Bt, A, seed, step):
    """float64 (Bt, A, A, 3): the normals of every directed pair, 0 on the diagonal."""
    n = np.zeros((Bt, A, A, 3))
    for f in range(Bt):
        for i in range(A):
            for j in range(A):
                if j != i:
                    n[f, i, j] = normals(seed, step, f, i, j)
    return n


def noised_poses(trans, sigma, seed, step):
    """trans float32 (Bt, A, A, 4, 4) -> float64 copy with sigma * n added to [0][3], [1][3], [2][3] of every pair j != i."""
    Bt, A = trans.shape[:2]
    out = trans.astype(np.float64)
    out[..., :3, 3] += sigma * noise_table(Bt, A, seed, step)
    return out


def find_isolated(counts, A, p, seed, ego=(0, 0), steps=range(4096)):
    """The first step at which every link into ego = (agent, frame) is down while every other ego of the batch keeps >= 1 link."""
    for s in steps:
        L = links_up(len(counts), A, seed, s, p)
        alone = {(i, f) for f, c in enumerate(counts) for i in range(c) if not any(L[f, i, j] for j in range(c) if j != i)}
        if alone == {ego}:
            return s
    raise AssertionError("no such step")


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
def _case(name, A, counts, p, sigma, seed, step, kind="fusion", only_v2i=False, outputs="all"):
    return dict(name=name, A=A, counts=list(counts), Bt=len(counts), p=p, sigma=sigma, seed=seed, step=step, kind=kind, only_v2i=only_v2i, outputs=outputs)


BIG_SEED = (0x9E3779B9 << 32) | 0x7F4A7C15          # >= 2^32: the key's second word is live
CARRY_STEP = (1 << 32) - 1                          # launched twice: the second launch carries into the counter's second word

CASES = [
    _case("a1-b1", 1, [1], 0.3, 0.5, 7, 0),                                        # one agent: no pair, nothing drawn
    _case("a2-b3", 2, [2, 2, 2], 0.3, 0.5, 7, 3),
    _case("a5-b1-p0", 5, [5], 0.0, 0.5, 11, 1),                                    # p = 0: rows copied, noise only
    _case("a5-b3-p1", 5, [5, 5, 5], 1.0, 0.0, 11, 2),                              # p = 1: egos alone; sigma = 0: no pose buffer
    _case("a5-b3-absent", 5, [5, 3, 1], 0.3, 0.5, BIG_SEED, 5),                    # absent agents, a one-agent frame
    _case("a5-b3-v2i", 5, [5, 4, 5], 0.3, 0.0, 13, 9, only_v2i=True),              # an only_v2i static plan
    _case("a5-b3-v2v", 5, [5, 2, 4], 0.3, 0.5, 13, 9, kind="v2v"),
    _case("a5-b130", 5, [5, 4, 3, 5, 2] * 26, 0.3, 0.5, BIG_SEED, 17),             # 3 250 pairs: more than one pass of the workgroup
    _case("a32-b3", 32, [32, 17, 32], 0.3, 0.5, 21, CARRY_STEP),                   # the agent fields' top values; the carry
    _case("a5-b3-bare", 5, [5, 5, 4], 0.3, 0.5, 5, CARRY_STEP, outputs="bare"),    # coef2 and link both NULL
    _case("a32-b1-p1", 32, [32], 1.0, 0.5, BIG_SEED, 0, kind="v2v"),
]


def synthetic_trans(Bt, A, seed):
    """float32 (Bt, A, A, 4, 4): rigid transforms with translations of a few tens of metres (the magnitude of the dataset's)."""
    rng = np.random.default_rng(seed)
    T = np.zeros((Bt, A, A, 4, 4), np.float32)
    yaw = rng.uniform(-np.pi, np.pi, (Bt, A, A))
    T[..., 0, 0], T[..., 0, 1], T[..., 1, 0], T[..., 1, 1] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw)
    T[..., 2, 2] = T[..., 3, 3] = 1.0
    T[..., :3, 3] = rng.uniform(-40.0, 40.0, (Bt, A, A, 3))
    return T


# ---- V2VNet: the oracle's operations with a zero message -------------------------------------------------------------------------------------
def v2v_zero_message(om, L):
    """The reference V2VNet `om` honours the links L (B, A, A) from now on; an ego without a live link gets the ZERO map as its mean message and
    the ConvGRU runs on it -- where tests/codec_refs.py's static-mask reading raises."""
    import torch
    from oracle import coperception_ref as R

    def fuse(local_com_mat, trans_matrices, num_agent_tensor, batch_size):
        e = om.emulate_bf16
        size = (1,) + tuple(local_com_mat.shape[2:])
        update = local_com_mat.clone()
        for b in range(batch_size):
            n = int(num_agent_tensor[b, 0])
            feats = [local_com_mat[b, k] for k in range(om.agent_num)]
            for _ in range(om.gnn_iter_num):
                updated = []
                for i in range(n):
                    nb = [R.feature_transformation(feats[j] if om.neighbor_source == "updated" else local_com_mat[b, j], trans_matrices[b, i][j], size)
                          for j in range(n) if j != i and bool(L[b][i][j])]
                    mean_feat = R._q(torch.mean(torch.stack(nb), dim=0), e) if nb else torch.zeros_like(local_com_mat[b, i])
                    ego = local_com_mat[b, i] if om.neighbor_source == "frozen" else feats[i]
                    updated.append(om.convgru(torch.cat([ego, mean_feat], dim=0).unsqueeze(0), None, e).squeeze(0))
                feats = updated + feats[n:]
            for k in range(n):
                update[b, k] = feats[k]
        return update
    om.fuse = fuse
    return om

"""Degraded links on the MI355X (csrc/channel.hip): the degrade kernel against the reference and case table of
tests/channel_refs.py (checked without a GPU by tests/test_channel_refs_cpu.py and, for the shared header, tests/test_channel_math_cpu.py),
every model family's degraded forward against the existing link-mask path, V2VNet's zero message, and a captured forward that draws fresh
links at every replay.

Bounds.  coef, coef2, link and the step are exact.  Normals: |n| <= 5.77, the fp32 rounding of the angle 2 pi u <= 5e-7, libm a few ulp: about
3.5e-6 in all, held to 1e-5 absolute against float64.  A translation t + sigma * n adds one fp32 rounding of the sum: sigma * 1e-5 + 2^-23 |t|."""
import numpy as np
import pytest
import torch

import channel_refs as CR
from oracle import coperception_ref as R
from test_gpu_models import TOL_EMU, TOL_FP32, check, make_inputs

pytestmark = pytest.mark.gpu

A, B, COUNTS = 3, 2, [3, 2]
FUSION = ["SumFusion", "MeanFusion", "MaxFusion", "CatFusion", "DiscoNet"]


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------------
def _launch(device, case, launches=1, trans=None, sigma=None):
    """-> per launch (coef, coef2, link, trans_out) as numpy (None where not asked for), the step after the last launch, and the inputs."""
    from v2x_sim_amd import ops
    Ag, Bt, bare = case["A"], case["Bt"], case["outputs"] == "bare"
    sigma = case["sigma"] if sigma is None else sigma
    items, coef0 = CR.static_plan(case["counts"], Ag, case["kind"], case["only_v2i"])
    it = torch.tensor(items, dtype=torch.int32).view(-1, 2).to(device)
    c0 = torch.from_numpy(coef0).to(device)
    n = len(items)
    nan = float("nan")                                               # every output starts as garbage: the kernel writes every element
    coef = torch.full((n, Ag), nan, device=device)
    coef2 = None if bare else torch.full((n * Ag, Ag), nan, device=device)
    link = None if bare else torch.full((Bt, Ag, Ag), 255, dtype=torch.uint8, device=device)
    T = CR.synthetic_trans(Bt, Ag, seed=Bt * 100 + Ag) if trans is None else trans
    Td = torch.from_numpy(T).to(device)
    out_T = torch.full((Bt, Ag, Ag, 4, 4), nan, device=device) if sigma > 0 else None
    step = torch.tensor([case["step"]], dtype=torch.int64, device=device)
    outs = []
    for _ in range(launches):
        ops.channel_degrade(it, Ag, Bt, c0, coef, coef2, link, Td if sigma > 0 else None, out_T, case["p"], sigma, case["seed"], step)
        outs.append(tuple(None if t is None else t.cpu().numpy().copy() for t in (coef, coef2, link, out_T)))
    torch.cuda.synchronize()
    assert np.array_equal(c0.cpu().numpy().view(np.uint32), coef0.view(np.uint32)), "the static rows were written"
    assert np.array_equal(Td.cpu().numpy().view(np.uint32), T.view(np.uint32)), "the clean poses were written"
    return outs, int(step.item()), (items, coef0, T)


@pytest.mark.parametrize("case", CR.CASES, ids=lambda c: c["name"])
def test_kernel_against_reference(device, case):
    launches = 2 if case["step"] == CR.CARRY_STEP else 1
    outs, step_after, (items, coef0, T) = _launch(device, case, launches)
    assert step_after == case["step"] + launches
    Ag, Bt = case["A"], case["Bt"]
    for k, (coef, coef2, link, out_T) in enumerate(outs):
        s = case["step"] + k
        rc, rc2, rl = CR.rewrite_plan(items, coef0, Ag, Bt, case["seed"], s, case["p"])
        assert np.array_equal(coef.view(np.uint32), rc.view(np.uint32)), (case["name"], s, "coef")
        if case["outputs"] == "bare":
            assert coef2 is None and link is None
        else:
            assert np.array_equal(coef2.view(np.uint32), rc2.view(np.uint32)), (case["name"], s, "coef2")
            assert np.array_equal(link, rl), (case["name"], s, "link")
        if case["p"] == 0.0:
            assert np.array_equal(coef, coef0)
        if case["p"] == 1.0:
            assert all(coef[m].tolist() == [coef0[m, j] if j == a else 0.0 for j in range(Ag)] for m, (a, f) in enumerate(items))
        if case["sigma"] == 0.0:
            assert out_T is None
            continue
        ref = CR.noised_poses(T, case["sigma"], case["seed"], s)
        same = np.ones((4, 4), bool)
        same[:3, 3] = False
        assert np.array_equal(out_T[..., same].view(np.uint32), T[..., same].view(np.uint32)), "an entry outside the translation changed"
        eye = np.eye(Ag, dtype=bool)
        assert np.array_equal(out_T[:, eye].view(np.uint32), T[:, eye].view(np.uint32)), "a diagonal pair changed"
        err = np.abs(out_T.astype(np.float64) - ref)
        bound = case["sigma"] * 1e-5 + 2.0 ** -23 * np.abs(T.astype(np.float64))
        print("%s step %d: worst translation error %.3g (bound there %.3g)" % (case["name"], s, err.max(), bound.reshape(-1)[err.argmax()]))
        assert (err <= bound).all(), (case["name"], s, float((err - bound).max()))
        if Ag > 1:
            assert np.abs(out_T[:, ~eye][..., :3, 3] - T[:, ~eye][..., :3, 3]).max() > 0.1           # noise was added
    if launches == 2 and case["outputs"] != "bare":
        assert not np.array_equal(outs[0][2], outs[1][2])                                        # the carry: a new step, new links


@pytest.mark.parametrize("name", ["a5-b130", "a32-b3"])
def test_normals_against_float64(device, name):
    """Clean translations of zero and sigma = 1: the pose buffer's translations ARE the fp32 normals (0 + 1 * n is exact)."""
    case = next(c for c in CR.CASES if c["name"] == name)
    Ag, Bt = case["A"], case["Bt"]
    T = CR.synthetic_trans(Bt, Ag, seed=3)
    T[..., :3, 3] = 0.0
    outs, _, _ = _launch(device, case, 1, trans=T, sigma=1.0)
    got = outs[0][3][..., :3, 3].astype(np.float64)
    ref = CR.noise_table(Bt, Ag, case["seed"], case["step"])
    err = np.abs(got - ref)
    print("%s: %d normals, max |fp32 - float64| = %.3g, max |n| = %.3f" % (name, ref.size, err.max(), np.abs(ref).max()))
    assert err.max() <= 1e-5


def test_draw_does_not_depend_on_items_or_presence(device):
    """The same (seed, step): the rows of frame 1 drawn in a 3-frame plan with absent agents == the rows of that frame alone at frame index 1."""
    full = dict(CR.CASES[0], A=5, counts=[5, 5, 5], Bt=3, p=0.3, sigma=0.0, seed=99, step=4, name="full")
    part = dict(full, counts=[2, 5, 1], name="part")
    (fo,), _, (fi, _, _) = _launch(device, full)
    (po,), _, (pi, _, _) = _launch(device, part)
    for m, (a, f) in enumerate(pi):
        if f == 1:
            assert np.array_equal(po[0][m], fo[0][fi.index((a, f))])
    assert np.array_equal(po[2][1], fo[2][1]) and not po[2][2].any() and int(po[2][0].sum()) <= 2


def test_zero_items_and_argument_errors(device):
    from v2x_sim_amd import _lib, ops
    step = torch.tensor([3], dtype=torch.int64, device=device)
    ops.channel_degrade(torch.zeros((0, 2), dtype=torch.int32, device=device), 5, 1, None, None, None, None, None, None, 0.3, 0.0, 1, step)
    assert int(step.item()) == 3                                      # nothing launched
    it = torch.zeros((1, 2), dtype=torch.int32, device=device)
    c = torch.ones((1, 5), device=device)
    with pytest.raises(_lib.V2XLibraryError, match="p_outage"):
        ops.channel_degrade(it, 5, 1, c, c.clone(), None, None, None, None, 1.5, 0.0, 1, step)
    with pytest.raises(_lib.V2XLibraryError, match="must not be the static rows"):
        ops.channel_degrade(it, 5, 1, c, c, None, None, None, None, 0.5, 0.0, 1, step)
    assert int(step.item()) == 3


@pytest.mark.parametrize("form", [0, 1, 2])
def test_warp_kernels_write_zeros_for_an_empty_neighbour_list(device, tune, form):
    """Every form of the warp kernel, every mode: an output item whose coefficient row is all zero is the zero map (what a V2VNet ego whose
    links are all down by outage reads as its mean message)."""
    from v2x_sim_amd import ops
    from v2x_sim_amd._lib import V2X_FUSE_MAX, V2X_FUSE_MEAN, V2X_FUSE_WSUM
    tune("WARP_LDS", form)
    g = torch.Generator().manual_seed(form)
    feat = torch.randn((3, 16, 16, 128), generator=g).to(torch.bfloat16).to(device)
    T = torch.from_numpy(CR.synthetic_trans(1, 3, seed=1)).to(device)
    T[..., :3, 3] *= 0.1
    items = ops.items_tensor([(0, 0), (1, 0), (2, 0)], 3, 1, device)
    coef = torch.tensor([[0, 1, 1], [0, 0, 0], [1, 1, 0]], dtype=torch.float32, device=device)
    for mode in (V2X_FUSE_MEAN, V2X_FUSE_WSUM, V2X_FUSE_MAX):
        out = torch.full((3, 16, 16, 128), 7.0, dtype=torch.bfloat16, device=device)
        ops.warp_fuse(feat, 3, 1, T, items, coef, mode, out=out)
        assert not bool(out[1].any()), (form, mode)
        assert bool(out[0].any()) and bool(out[2].any())


# ---- the models --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs():
    _, bev, T = make_inputs(A, B, n_pts=6000, seed=5)
    return bev, T, torch.tensor([[3] * A, [2] * A])


def _model(P, device, seed=3, **kw):
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.utils.synthetic import init_synthetic_weights
    return init_synthetic_weights(P(Config("train"), num_agent=A, **kw), seed=seed).to(device)


def _same(a, b, what):
    if isinstance(a, dict):
        for k in ("cls", "loc"):
            assert torch.equal(a[k], b[k]), (what, k)
    else:
        assert torch.equal(a, b), what


def _launch_names(fn):
    from v2x_sim_amd import ops
    ops.PROFILE = []
    try:
        out = fn()
        return out, [r[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None


@pytest.mark.parametrize("name", FUSION)
def test_degraded_forward_equals_the_link_mask_path(device, inputs, name):
    from v2x_sim_amd.models import det
    bev, T, nat = inputs
    pm = _model(getattr(det, name), device)
    x0, Td = pm._input_nhwc(bev.to(device)), T.to(device)
    seed, step, p, sigma = CR.BIG_SEED, 6, 0.3, 0.5
    with torch.no_grad():
        pm.set_channel(p_com_outage=p, pose_noise=sigma, seed=seed)
        pm.reset_channel(step)
        plan = pm.make_plan(nat, B, device)
        got, names = _launch_names(lambda: pm.forward_nhwc(x0, Td, nat, B, plan=plan))
        assert names.count("channel_degrade_kernel") == 1
        L = CR.links_up(B, A, seed, step, p)
        _, _, link = CR.rewrite_plan(*CR.static_plan(COUNTS, A), A, B, seed, step, p)
        assert np.array_equal(pm.last_links().cpu().numpy(), link) and 0 < int(link.sum()) < 3 * 2 + 2 * 1
        assert pm.channel_step() == step + 1
        noised = plan["channel"]["trans"].clone()
        ref_T = CR.noised_poses(T.numpy(), sigma, seed, step)
        assert (np.abs(noised.cpu().numpy() - ref_T) <= sigma * 1e-5 + 2.0 ** -23 * np.abs(T.numpy())).all()
        assert torch.equal(Td.cpu(), T)                                            # the caller's tensor is never written
        # the existing path: a static link mask of that step's links, the device's own noised poses passed in
        pm.set_channel()
        pm.set_link_mask(torch.from_numpy(L))
        want, names = _launch_names(lambda: pm.forward_nhwc(x0, noised, nat, B))
        assert "channel_degrade_kernel" not in names
        _same(got, want, name)
        # p = 1 == the all-false mask
        pm.set_link_mask(None)
        pm.set_channel(p_com_outage=1.0, seed=seed)
        alone = pm.forward_nhwc(x0, Td, nat, B)
        assert not bool(pm.last_links().any())
        pm.set_channel()
        pm.set_link_mask(torch.zeros((A, A), dtype=torch.bool))
        _same(alone, pm.forward_nhwc(x0, Td, nat, B), name + " p=1")
        assert not torch.equal(alone["cls"], got["cls"])


@pytest.mark.parametrize("name", ["MeanFusion", "DiscoNet", "V2VNet", "When2com"])
def test_undegraded_model_is_the_parent(device, inputs, name, monkeypatch):
    """p = 0, sigma = 0: the launches and the bits of a model that never heard of the feature; ops.channel_degrade is not called."""
    from v2x_sim_amd import ops
    from v2x_sim_amd.models import det
    bev, T, nat = inputs
    nat = torch.full((B, A), A) if name == "V2VNet" else nat
    plain, pm = _model(getattr(det, name), device), _model(getattr(det, name), device)
    pm.set_channel(pose_noise=0.5, seed=4)
    pm.set_channel(p_com_outage=0.0, pose_noise=0.0)
    monkeypatch.setattr(ops, "channel_degrade", lambda *a, **k: pytest.fail("channel_degrade called by an undegraded model"))
    kw = dict(training=False, inference="activated") if name == "When2com" else {}
    with torch.no_grad():
        a, na = _launch_names(lambda: plain(bev.to(device), T.to(device), nat, batch_size=B, **kw))
        b, nb = _launch_names(lambda: pm(bev.to(device), T.to(device), nat, batch_size=B, **kw))
    assert na == nb and "channel_degrade_kernel" not in nb
    _same(a, b, name)
    assert pm.channel_step() == 0 and pm.last_links() is None


def test_v2vnet_ego_down_by_outage_gets_the_zero_message(device, inputs):
    """A (seed, step) at which ego 0 of frame 0 loses both links and every other ego keeps one: bit-equal to the run on a hand-built plan with
    that ego's row zeroed, and within the end-to-end bar of the oracle's operations composed with a zero message."""
    from v2x_sim_amd.models.det import V2VNet
    bev, T, nat = inputs
    seed, p = 77, 0.5
    step = CR.find_isolated(COUNTS, A, p, seed, ego=(0, 0))
    pm = _model(V2VNet, device)
    om = R.V2VNet(num_agent=A).eval()
    om.load_state_dict(pm.state_dict())
    x0, Td = pm._input_nhwc(bev.to(device)), T.to(device)
    with torch.no_grad():
        static = pm.make_plan(nat, B, device)
        pm.set_channel(p_com_outage=p, seed=seed)
        pm.reset_channel(step)
        got = pm.forward_nhwc(x0, Td, nat, B)
        links = pm.last_links().cpu().numpy()
        assert not links[0, 0].any() and links[0, 1].any() and links[0, 2].any() and links[1, 0, 1] and links[1, 1, 0]
        items, coef0 = CR.static_plan(COUNTS, A, "v2v")
        coef, _, rl = CR.rewrite_plan(items, coef0, A, B, seed, step, p)
        assert np.array_equal(links, rl) and not coef[items.index((0, 0))].any()
        hand = dict(static)
        hand["coef"] = torch.from_numpy(coef).to(device)
        pm.set_channel()
        _same(got, pm.forward_nhwc(x0, Td, nat, B, plan=hand), "hand-built plan")
        CR.v2v_zero_message(om, CR.links_up(B, A, seed, step, p))
        for emu, tol in ((True, TOL_EMU), (False, TOL_FP32)):
            om.emulate_bf16 = emu
            ref = om(bev, T, nat, batch_size=B)
            check(got["cls"], ref["cls"], tol, "V2VNet zero message cls emu=%s" % emu)
            check(got["loc"], ref["loc"], tol, "V2VNet zero message loc emu=%s" % emu)


@pytest.mark.parametrize("name", ["MeanFusionSeg", "When2com", "When2comSeg"])
def test_pose_noise_equals_noised_poses_passed_in(device, inputs, name):
    from v2x_sim_amd.models import det, seg
    bev, T, nat = inputs
    pm = _model(getattr(seg, name) if name.endswith("Seg") else getattr(det, name), device)
    x0, Td = pm._input_nhwc(bev.to(device)), T.to(device)
    # (softmax inference: dense attention weights, so that every neighbour's pose takes part whatever the synthetic scores are)
    kw = dict(training=False, inference="softmax", batch_size=B) if name.startswith("When2com") else dict(batch_size=B)
    with torch.no_grad():
        pm.set_channel(pose_noise=0.5, seed=8)
        pm.reset_channel(2)
        plan = pm.make_plan(nat, B, device)
        got, names = _launch_names(lambda: pm.forward_nhwc(x0, Td, nat, plan=plan, **kw))
        assert names.count("channel_degrade_kernel") == 1 and pm.channel_step() == 3
        noised = plan["channel"]["trans"].clone()
        ref_T = CR.noised_poses(T.numpy(), 0.5, 8, 2)
        assert (np.abs(noised.cpu().numpy() - ref_T) <= 0.5 * 1e-5 + 2.0 ** -23 * np.abs(T.numpy())).all()
        pm.set_channel()
        want = pm.forward_nhwc(x0, noised, nat, **kw)
        clean = pm.forward_nhwc(x0, Td, nat, **kw)
    _same(got, want, name)
    g, c = (got["cls"], clean["cls"]) if isinstance(got, dict) else (got, clean)
    assert not torch.equal(g, c)


# ---- capture -----------------------------------------------------------------------------------------------------------------------------------
def test_captured_forward_draws_fresh_links_at_every_replay(device, inputs):
    from v2x_sim_amd.models.det import MeanFusion
    bev, T, nat = inputs
    pm = _model(MeanFusion, device)
    seed, p, sigma, first = 31, 0.3, 0.5, 5
    x0, Td = pm._input_nhwc(bev.to(device)), T.to(device)
    pm.set_channel(p_com_outage=p, pose_noise=sigma, seed=seed)
    plan = pm.make_plan(nat, B, device)
    with torch.no_grad():
        pm.forward_nhwc(x0, Td, nat, B, plan=plan)                       # library loaded, parameters packed, allocator warm
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            pm.forward_nhwc(x0, Td, nat, B, plan=plan)
        torch.cuda.current_stream().wait_stream(side)
        pm.reset_channel(first)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = pm.forward_nhwc(x0, Td, nat, B, plan=plan)
        replays = []
        for k in range(3):
            graph.replay()
            torch.cuda.synchronize()
            replays.append((pm.last_links().cpu().numpy().copy(), out["cls"].clone(), out["loc"].clone()))
        assert pm.channel_step() == first + 3
        items, coef0 = CR.static_plan(COUNTS, A)
        for k, (links, cls, loc) in enumerate(replays):
            assert np.array_equal(links, CR.rewrite_plan(items, coef0, A, B, seed, first + k, p)[2]), k
            pm.reset_channel(first + k)
            eager = pm.forward_nhwc(x0, Td, nat, B, plan=plan)
            assert torch.equal(eager["cls"], cls) and torch.equal(eager["loc"], loc), k
        assert len({r[0].tobytes() for r in replays}) > 1                # the replays did not see the same links

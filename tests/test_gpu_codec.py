"""Communication limits on the MI355X: the fused codec kernel against float64, its sender / receiver split, compressed and link-masked models
end to end against the reference composed in tests/codec_refs.py, sharded == unsharded, training on the kernels, and the evaluation driver.

End-to-end cases: compress_level in {2, 6} with weights seed 0 and inputs seed 1 -- the levels at which the reference alone (bf16-emulating
against fp32) is no noisier than the uncompressed case the suite already holds to (3e-2, 3e-3) of max|ref|; tests/test_codec_cpu.py recomputes
that condition.  When2com was priced the same way with the designed attention scores of tests/test_gpu_models.py ('activated', in 1e-3 of
max|ref|, cls max / mean, loc max / mean): k = 0: 19.8 / 2.98, 17.0 / 1.89;  k = 2: 15.9 / 1.70, 15.5 / 1.78;  k = 6: 15.1 / 1.51, 9.4 / 1.03
-- both levels qualify and are tested against the emulating reference."""
import os

import numpy as np
import pytest
import torch

import codec_refs as CR
from oracle import coperception_ref as R
from test_gpu_models import TOL_EMU, TOL_FP32, _separate_attention_scores, check, make_inputs

pytestmark = pytest.mark.gpu

E2E_LEVELS = (2, 6)
KERNEL_M = (1, 15, 16, 1000, 5 * 1024, 40 * 1024 + 7)
KERNEL_CASES = [(C, C >> k) for C in (256, 128) for k in range(1, 9) if (C >> k) >= 1]


def _kernel_input(M, C, seed):
    """bf16 pixels with exact zeros (a fifth of the entries), both signs, and one channel of magnitude ~100."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, C, generator=g)
    x[torch.rand(M, C, generator=g) < 0.2] = 0.0
    x[:, 3] = 100.0 * torch.randn(M, generator=g)
    return x.to(torch.bfloat16)


def _packed(C, Cc, device, seed):
    from v2x_sim_amd import packing
    mods = CR.codec_modules(C, Cc, seed)
    pc = packing.pack_codec("codec", *mods, device=device)
    s1, t1 = packing.fold_bn(mods[0].bias, mods[1], Cc)
    s2, t2 = packing.fold_bn(mods[2].bias, mods[3], C)
    return pc, (mods[0].weight.detach().reshape(Cc, C), s1, t1), (mods[2].weight.detach().reshape(C, Cc), s2, t2)


@pytest.mark.parametrize("C,Cc", KERNEL_CASES)
def test_codec_kernel_against_float64(device, C, Cc):
    """Message against float64 of the same bf16 operands; output against float64 FED THE KERNEL'S OWN MESSAGE; each within one bf16 ulp
    (atol 2^-8, rtol 2^-7: bf16 x bf16 products are exact in fp32 and a 256-term fp32 sum is far inside half a bf16 ulp, so only the final
    rounding can differ).  Every M, and on each: fused == compress-then-decompress bitwise, and the fused launch without the message output
    gives the same y."""
    from v2x_sim_amd import ops
    pc, (wc, s1, t1), (wd, s2, t2) = _packed(C, Cc, device, seed=C + Cc)
    for M in KERNEL_M:
        x = _kernel_input(M, C, seed=M + Cc)
        xd = x.to(device)
        y, msg = ops.codec(pc, xd, want_msg=True)
        y_only = ops.codec(pc, xd)
        msg2 = ops.codec_compress(pc, xd)
        y2 = ops.codec_decompress(pc, msg2)
        assert y.shape == (M, C) and msg.shape == (M, Cc) and y.dtype == msg.dtype == torch.bfloat16
        assert torch.equal(msg.view(torch.int16), msg2.view(torch.int16)), (C, Cc, M, "message: fused != compress")
        assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), (C, Cc, M, "y: fused != decompress(compress)")
        assert torch.equal(y.view(torch.int16), y_only.view(torch.int16)), (C, Cc, M, "y depends on the message output")
        ref_m = CR.codec_stage_fp64(x, wc, s1, t1)
        ref_y = CR.codec_stage_fp64(msg.cpu(), wd, s2, t2)
        pre_m = (x.double() @ wc.to(torch.bfloat16).double().t()) * s1.double() + t1.double()
        pre_y = (msg.cpu().double() @ wd.to(torch.bfloat16).double().t()) * s2.double() + t2.double()
        if M >= 1000:                                            # the inputs exercise what they claim to
            assert bool((x == 0).any()) and bool((pre_m < 0).any()) and bool((pre_m > 0).any())
            assert bool((pre_y < 0).any()) and bool((pre_y > 0).any()) and float(x[:, 3].abs().max()) > 100
        for what, got, ref in (("msg", msg, ref_m), ("y", y, ref_y)):
            got = got.cpu().double()
            err = (got - ref).abs() - (2.0 ** -8 + 2.0 ** -7 * ref.abs())
            print("C %d Cc %d M %d %s: max |ref| %.2f, worst margin %.3e" % (C, Cc, M, what, float(ref.abs().max()), float(err.max())))
            assert float(err.max()) <= 0, (C, Cc, M, what, float(err.max()))


@pytest.mark.parametrize("C,Cc", [(256, 128), (256, 64), (256, 4), (128, 64), (128, 1)])
def test_codec_map_bits_do_not_depend_on_the_batch(device, C, Cc):
    """A 32 x 32 map inside M = 40 * 1024 + 7 pixels == the same map alone, bitwise (message and output), wherever it sits."""
    from v2x_sim_amd import ops
    pc, _, _ = _packed(C, Cc, device, seed=7 + Cc)
    M = 40 * 1024 + 7
    x = _kernel_input(M, C, seed=99).to(device)
    y, msg = ops.codec(pc, x, want_msg=True)
    for start in (0, 1024 * 17, M - 1024, 13):                   # (13: not fragment-aligned; M - 1024: includes the partial last fragment)
        one = x[start:start + 1024].contiguous()
        y1, m1 = ops.codec(pc, one.view(1, 32, 32, C), want_msg=True)
        assert torch.equal(y1.view(-1, C).view(torch.int16), y[start:start + 1024].view(torch.int16)), (C, Cc, start)
        assert torch.equal(m1.view(-1, Cc).view(torch.int16), msg[start:start + 1024].view(torch.int16)), (C, Cc, start)


def _build(P, O, device, k=0, pkw=None, okw=None, seed=0):
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.utils.synthetic import init_synthetic_weights
    pm = init_synthetic_weights(P(Config("train"), compress_level=k, **(pkw or {})), seed=seed)
    om = CR.with_codec(O(**(okw or {})), k).eval()
    om.load_state_dict(pm.state_dict())
    return pm.to(device), om


@pytest.mark.parametrize("k", E2E_LEVELS)
@pytest.mark.parametrize("name", ["V2VNet", "MeanFusion", "MaxFusion", "CatFusion", "DiscoNet"])
def test_compressed_models_end_to_end(device, name, k):
    from v2x_sim_amd.models import det
    A, B = 5, 1
    pm, om = _build(getattr(det, name), getattr(R, name), device, k)
    _, bev, T = make_inputs(A, B, 20000, seed=1)
    nat = torch.full((B, A), A)
    with torch.no_grad():
        got = pm(bev.to(device), T.to(device), nat, batch_size=B)
        for emu, tol in ((True, TOL_EMU), (False, TOL_FP32)):
            om.emulate_bf16 = emu
            ref = om(bev, T, nat, batch_size=B)
            check(got["cls"], ref["cls"], tol, "%s k=%d cls emu=%s" % (name, k, emu))
            check(got["loc"], ref["loc"], tol, "%s k=%d loc emu=%s" % (name, k, emu))
        # the flag matters: the uncompressed reference (same other weights) is far outside the bar
        plain = getattr(R, name)().eval()
        plain.load_state_dict({n: v for n, v in pm.state_dict().items() if "compress" not in n}, strict=True)
        plain.emulate_bf16 = True
        far = plain(bev, T, nat, batch_size=B)
    assert float((far["cls"] - ref["cls"]).abs().max()) > 3 * TOL_EMU[0] * float(ref["cls"].abs().max())


@pytest.mark.parametrize("k", E2E_LEVELS)
def test_compressed_v2vnet_seg_end_to_end(device, k):
    from v2x_sim_amd.models.seg import V2VNetSeg
    A, B = 5, 1
    pm, om = _build(V2VNetSeg, R.V2VNetSeg, device, k)
    _, bev, T = make_inputs(A, B, 20000, seed=1)
    nat = torch.full((B, A), A)
    om.emulate_bf16 = True
    with torch.no_grad():
        got = pm.forward_nhwc(pm._input_nhwc(bev.to(device)), T.to(device), nat, batch_size=B)
        ref = om(bev, T, nat, batch_size=B).permute(0, 2, 3, 1).contiguous()
    check(got, ref, TOL_EMU, "seg logits k=%d" % k)


@pytest.mark.parametrize("k", E2E_LEVELS)
def test_compressed_when2com_end_to_end(device, k):
    from v2x_sim_amd.models.det import When2com
    A, B = 5, 1
    pm, om = _build(When2com, R.When2com, device, k)
    _, bev, T = make_inputs(A, B, 20000, seed=1)
    nat = torch.full((B, A), A)
    _separate_attention_scores(pm, om, bev, B)
    om.emulate_bf16 = True
    with torch.no_grad():
        got = pm(bev.to(device), T.to(device), nat, training=False, inference="activated", batch_size=B)
        ref = om(bev, T, nat, training=False, inference="activated", batch_size=B)
    assert torch.equal(got["coef"].cpu() != 0, ref["coef"] != 0), "HIP and oracle selected different links"
    check(got["cls"], ref["cls"], TOL_EMU, "when2com k=%d cls" % k)
    check(got["loc"], ref["loc"], TOL_EMU, "when2com k=%d loc" % k)


def _irregular_mask(B, A):
    g = torch.Generator().manual_seed(77)
    L = torch.rand(B, A, A, generator=g) < 0.5
    L[:, torch.arange(A), (torch.arange(A) + 1) % A] = True     # every ego keeps one neighbour (agent 3 of the 4-agent frame: agent 0 below)
    L[:, :, 0] = True
    return L


@pytest.mark.parametrize("mask", ["only_v2i", "irregular"])
@pytest.mark.parametrize("name", ["SumFusion", "MeanFusion", "MaxFusion", "CatFusion", "DiscoNet", "V2VNet"])
def test_link_masks_end_to_end(device, name, mask):
    """The [5, 4]-agent batch of test_simple_fusion_baselines under only_v2i and under an irregular user mask, against the masked reference at
    the unchanged bar (a mask adds no rounding site, it only shortens sums this batch is already held to the bar on); and the mask matters:
    the unmasked reference is far outside it."""
    from v2x_sim_amd.models import det
    A, B = 5, 2
    v2i = mask == "only_v2i"
    pm, om = _build(getattr(det, name), getattr(R, name), device, 0, pkw=dict(only_v2i=v2i), seed=4)
    L = CR.only_v2i_mask(B, A) if v2i else _irregular_mask(B, A)
    if not v2i:
        pm.set_link_mask(L)
    _, bev, T = make_inputs(A, B, n_pts=8000, seed=9)
    nat = torch.tensor([[5] * A, [4] * A])
    with torch.no_grad():
        got = pm(bev.to(device), T.to(device), nat, batch_size=B)
        om.emulate_bf16 = True
        unmasked = om(bev, T, nat, batch_size=B)
        CR.apply_links(om, L)
        for emu, tol in ((True, TOL_EMU), (False, TOL_FP32)):
            om.emulate_bf16 = emu
            ref = om(bev, T, nat, batch_size=B)
            check(got["cls"], ref["cls"], tol, "%s %s cls emu=%s" % (name, mask, emu))
            check(got["loc"], ref["loc"], tol, "%s %s loc emu=%s" % (name, mask, emu))
    om.emulate_bf16 = True
    with torch.no_grad():
        ref = om(bev, T, nat, batch_size=B)
    assert float((unmasked["cls"] - ref["cls"]).abs().max()) > 3 * TOL_EMU[0] * float(ref["cls"].abs().max())


def test_v2vnet_ego_without_links_raises(device):
    from v2x_sim_amd.models.det import V2VNet
    A, B = 5, 1
    pm, _ = _build(V2VNet, R.V2VNet, device, 0, pkw=dict(only_v2i=True))
    L = torch.ones(B, A, A, dtype=torch.bool)
    L[0, 2, 0] = False
    pm.set_link_mask(L)
    _, bev, T = make_inputs(A, B, n_pts=2000, seed=3)
    with pytest.raises(RuntimeError, match="non-empty TensorList"):
        pm(bev.to(device), T.to(device), torch.full((B, A), A), batch_size=B)


@pytest.mark.parametrize("name", ["V2VNet", "MeanFusion", "DiscoNet", "When2com"])
def test_level_zero_is_the_model_of_today(device, name):
    """compress_level=0, only_v2i=False: the logits of a model built without the arguments, bit for bit, through the same launches."""
    from v2x_sim_amd import ops
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models import det
    from v2x_sim_amd.utils.synthetic import init_synthetic_weights
    A, B = 5, 1
    P = getattr(det, name)
    a = init_synthetic_weights(P(Config("train")), seed=6).to(device)
    b = init_synthetic_weights(P(Config("train"), compress_level=0, only_v2i=False), seed=6).to(device)
    _, bev, T = make_inputs(A, B, n_pts=8000, seed=2)
    nat = torch.full((B, A), A)
    kw = dict(training=False, inference="activated") if name == "When2com" else {}
    outs, launches = [], []
    with torch.no_grad():
        for m in (a, b):
            ops.PROFILE = []
            outs.append(m(bev.to(device), T.to(device), nat, batch_size=B, **kw))
            launches.append([r[0] for r in ops.PROFILE])
            ops.PROFILE = None
    assert launches[0] == launches[1] and not any("codec" in n for n in launches[0])
    assert torch.equal(outs[0]["cls"], outs[1]["cls"]) and torch.equal(outs[0]["loc"], outs[1]["loc"])


@pytest.mark.parametrize("world", [2, 5])
def test_sharded_equals_unsharded_bitwise_compressed_v2i(device, world):
    """The method of test_gpu_models.py::test_sharded_equals_unsharded_bitwise for a compressed, only_v2i V2VNet: one GPU plays every rank in
    turn, the all-gather is the concatenation of the ranks' (decompressed) encoder maps."""
    from v2x_sim_amd.models.det import V2VNet
    from v2x_sim_amd.models.det.base import LidarDecoder
    from v2x_sim_amd.parallel import AgentShard, ShardedV2VNet
    from v2x_sim_amd.utils.synthetic import synthetic_points, synthetic_poses
    A, Bt = 5, 2
    pm, _ = _build(V2VNet, R.V2VNet, device, 2, pkw=dict(only_v2i=True))
    pts = torch.from_numpy(synthetic_points(A * Bt, 16384, seed=11)).to(device)
    cnt = torch.full((A * Bt,), 16384, dtype=torch.int32, device=device)
    trans = torch.from_numpy(synthetic_poses(Bt, A, seed=12)).to(device)
    nat = torch.tensor([[5] * A, [4] * A])
    links = pm.links(Bt)
    with torch.no_grad():
        one = AgentShard(A, Bt, 0, 1)
        ref = ShardedV2VNet(pm, one).forward_points(pts, cnt, trans, one.fusion_plan(nat, device, links=links))
        # the sharded runner and the plain model agree on the plan: same coefficients as V2VNet.make_plan
        assert torch.equal(one.fusion_plan(nat, device, links=links)["coef"], pm.make_plan(nat, Bt, device)["coef"])
        shards = [AgentShard(A, Bt, r, world) for r in range(world)]
        pk = pm.packed(device)
        runners = [ShardedV2VNet(pm, s, exchange=None) for s in shards]
        enc = [rn.encode_points(pts[s.lo:s.hi], cnt[s.lo:s.hi], pk) for rn, s in zip(runners, shards)]
        gathered = torch.cat([e[pm.layer] for e in enc])
        outs = []
        for rn, s, e in zip(runners, shards, enc):
            rn.exchange = lambda t, g=gathered: g
            cur = rn.fuse_local(list(e), trans, s.fusion_plan(nat, device, links=links), pk)
            feats = list(e)
            feats[pm.layer] = cur
            outs.append(pm.get_cls_loc_result(LidarDecoder.run(pk["dec"], *feats), pk["heads"]))
    assert torch.equal(torch.cat([o["cls"] for o in outs]), ref["cls"])
    assert torch.equal(torch.cat([o["loc"] for o in outs]), ref["loc"])


def test_compressed_train_graph_loss_and_grads_match_reference(device, tune):
    """The method and tolerance of tests/test_gpu_train.py::test_train_graph_loss_and_grads_match_oracle for a compressed V2VNet, the four
    new modules' parameters included."""
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.det import V2VNet
    from v2x_sim_amd.train import detection_loss, train_forward
    from v2x_sim_amd.train.loop import synthetic_batch_on_device
    from v2x_sim_amd.utils.synthetic import init_synthetic_weights
    A = 2
    tune("TRAIN_HIP", 0)
    cfg = Config("train")
    pm = init_synthetic_weights(V2VNet(cfg, num_agent=A, compress_level=2), seed=3)
    om = CR.with_codec(R.V2VNet(num_agent=A), 2)
    om.load_state_dict(pm.state_dict())
    pm = pm.to(device)
    data = synthetic_batch_on_device(cfg, 1, A, seed=5, device=device)
    cpu = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in data.items()}
    for mode, gtol in (("eval", 2e-2), ("train", None)):
        getattr(pm, mode)()
        getattr(om, mode)()
        pm.zero_grad()
        om.zero_grad()
        res = train_forward(pm, data["bev_seq"], data["trans_matrices"], data["num_agent"], 1)
        loss = detection_loss(res, data["labels"], data["reg_targets"], data["reg_loss_mask"])
        loss[0].backward()
        ref = om(cpu["bev_seq"], cpu["trans_matrices"], cpu["num_agent"], batch_size=1)
        rloss = detection_loss(ref, cpu["labels"], cpu["reg_targets"], cpu["reg_loss_mask"])
        rloss[0].backward()
        for a, b in zip(loss, rloss):
            assert abs(float(a.detach()) - float(b.detach())) <= 1e-3 * abs(float(b.detach())) + 1e-5, mode
        og = dict(om.named_parameters())
        pg = dict(pm.named_parameters())
        for key in ("u_encoder.com_compresser.weight", "u_encoder.bn_compress.weight", "u_encoder.com_decompresser.weight", "u_encoder.bn_decompress.bias"):
            assert pg[key].grad is not None and float(pg[key].grad.abs().max()) > 0, key
        gmax = max(float(g.grad.abs().max()) for g in og.values() if g.grad is not None)
        worst, worst_k = 0.0, ""
        for k, p in pg.items():
            if p.grad is None:
                assert k == "convgru.weight_hh_l0" and (og[k].grad is None or float(og[k].grad.abs().max()) == 0.0), k
                continue
            d = float((p.grad.cpu() - og[k].grad).abs().max()) / max(float(og[k].grad.abs().max()), 1e-3 * gmax)
            if d >= worst:
                worst, worst_k = d, k
        print("%s-mode BN: loss %.5f (reference %.5f), worst relative gradient difference %.2e (%s)" % (
            mode, float(loss[0].detach()), float(rloss[0].detach()), worst, worst_k))
        if gtol is not None:
            assert worst < gtol, (mode, worst, worst_k)


def test_graphed_compressed_v2vnet_step(device, tune):
    """A compressed V2VNet step on the kernels (both codec layers: _Conv1x1 + the BatchNorm kernels) captures as ONE GraphedTrainStep graph
    and tracks the eager steps, as tests/test_gpu_train_kernels.py::test_graphed_v2vnet_step compares them."""
    import copy
    import warnings
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.det import V2VNet
    from v2x_sim_amd.train import detection_loss, train_forward
    from v2x_sim_amd.train.graph_step import GraphedTrainStep
    from v2x_sim_amd.train.loop import init_for_training, synthetic_batch_on_device
    tune("TRAIN_HIP", 1)
    cfg = Config("train")
    base = init_for_training(V2VNet(cfg, num_agent=3, compress_level=2), seed=1).to(device)
    batches = [synthetic_batch_on_device(cfg, 1, 3, seed=20 + i, device=device) for i in range(5)]
    eager = copy.deepcopy(base).train()
    opt_e = torch.optim.SGD(eager.parameters(), lr=1e-3)
    losses_e = []
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*codec.*")   # k = 2: both layers on the kernels, no library-path warning
        for d in batches:
            res = train_forward(eager, d["bev_seq"], d["trans_matrices"], d["num_agent"], 1)
            loss = detection_loss(res, d["labels"], d["reg_targets"], d["reg_loss_mask"])[0]
            opt_e.zero_grad(set_to_none=True)
            loss.backward()
            opt_e.step()
            losses_e.append(float(loss.detach()))
    w0 = base.u_encoder.com_compresser.weight
    assert not torch.equal(eager.u_encoder.com_compresser.weight, w0)         # the codec trains
    graphed = copy.deepcopy(base).train()
    step = GraphedTrainStep(graphed, torch.optim.SGD(graphed.parameters(), lr=1e-3), batches[0], 1)
    losses_g = [float(step(d)[0]) for d in batches]
    print("eager  ", ["%.5f" % v for v in losses_e])
    print("graphed", ["%.5f" % v for v in losses_g])
    assert np.allclose(losses_g, losses_e, rtol=2e-3)


def test_small_message_trains_on_the_library_path_and_says_so(device, tune):
    """k = 5 (8 channels): the 1x1 kernels want a multiple of 32 input channels, so the codec's layers take the library path -- with a warning,
    once per shape -- and the step still produces gradients for them."""
    import warnings
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.det import MeanFusion
    from v2x_sim_amd.train import detection_loss, train_forward
    from v2x_sim_amd.train import hip_graph
    from v2x_sim_amd.train.loop import init_for_training, synthetic_batch_on_device
    tune("TRAIN_HIP", 1)
    cfg = Config("train")
    m = init_for_training(MeanFusion(cfg, num_agent=2, compress_level=5, only_v2i=True), seed=1).to(device).train()
    d = synthetic_batch_on_device(cfg, 1, 2, seed=3, device=device)
    hip_graph._CODEC_WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        for _ in range(2):
            res = train_forward(m, d["bev_seq"], d["trans_matrices"], d["num_agent"], 1)
    assert sum("codec" in str(w.message) for w in rec) == 1
    detection_loss(res, d["labels"], d["reg_targets"], d["reg_loss_mask"])[0].backward()
    assert float(m.u_encoder.com_decompresser.weight.grad.abs().max()) > 0 and float(m.u_encoder.com_compresser.weight.grad.abs().max()) > 0


def test_test_codet_driver_with_communication_flags(device, tmp_path, capsys):
    """tools/det/test_codet.py's evaluation with --com mean --compress_level 2 --only_v2i 1 (through tools/det/eval_codet.py, which hands the two
    flags to the model and everything else to test_codet.py) on the parsed synthetic tree of tests/test_gpu_dataset.py; a checkpoint that
    records other flags is refused, and the flags do not outlive the call."""
    import importlib.util
    from oracle import voxelize_ref as VR
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.datasets import write_sample
    from v2x_sim_amd.models.det import MeanFusion
    from v2x_sim_amd.utils.synthetic import init_synthetic_weights, synthetic_points, synthetic_poses
    A, frames = 3, 2
    pts = synthetic_points(A * frames, 15000, seed=31)
    T = synthetic_poses(frames, A, seed=32)
    rng = np.random.default_rng(1)
    for f in range(frames):
        for a in range(A):
            _, idx = VR.voxelize_occupy(pts[a * frames + f], return_indices=True)
            gt = np.concatenate([rng.uniform(-25, 25, (6, 2)), np.tile([2.0, 4.0], (6, 1)), rng.uniform(-1, 1, (6, 1))], 1)
            write_sample(str(tmp_path), "test", a, 3, f, idx, T[f, a], A, gt_boxes=gt)
    ckpt = os.path.join(str(tmp_path), "ckpt.pth")
    model = init_synthetic_weights(MeanFusion(Config("test"), num_agent=A, compress_level=2, only_v2i=True), seed=4)
    torch.save({"epoch": 1, "model_state_dict": model.state_dict(), "compress_level": 2, "only_v2i": True}, ckpt)
    spec = importlib.util.spec_from_file_location("eval_codet", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "det", "eval_codet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    common = ["--data", os.path.join(str(tmp_path), "test"), "--com", "mean", "--resume", ckpt, "--num_agent", str(A), "--batch", "2", "--score_thr", "0.55"]
    res = mod.main(common + ["--compress_level", "2", "--only_v2i", "1"])
    out = capsys.readouterr().out
    assert "average local mAP@0.5" in out and out.count("agent") >= A
    assert 0.0 <= res[0.5] <= 1.0 and 0.0 <= res[0.7] <= 1.0
    with pytest.raises(SystemExit):
        mod.main(common + ["--compress_level", "2", "--only_v2i", "0"])
    with pytest.raises(SystemExit):
        mod.main(common + ["--compress_level", "3", "--only_v2i", "1"])
    from v2x_sim_amd.utils import comm
    assert comm.current_model_flags() is None and MeanFusion(Config("test"), num_agent=A).compress_level == 0


def test_test_seg_driver_with_communication_flags(device, capsys):
    """tools/seg/test_seg.py's evaluation (synthetic scenes, seeded weights) with --compress_level 2 --only_v2i 1 through tools/seg/eval_seg.py: runs,
    reports, and the model it built carries the codec (its launches show in the profile list)."""
    import importlib.util
    from v2x_sim_amd import ops
    spec = importlib.util.spec_from_file_location("eval_seg", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "seg", "eval_seg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ops.PROFILE = []
    try:
        res = mod.main(["--com", "v2v", "--num_agent", "3", "--frames", "2", "--batch", "2", "--compress_level", "2", "--only_v2i", "1"])
        names = [r[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert "mIoU" in capsys.readouterr().out and 0.0 <= res["miou"] <= 1.0
    assert any("codec_kernel<256, 64" in n for n in names)
    with pytest.raises(SystemExit):
        mod.main(["--com", "lowerbound", "--compress_level", "2"])


def test_hip_training_graph_with_codec_vs_fp32_graph(device, tune):
    """The bf16 HIP training graph with the codec (k = 2: both layers on the kernels; k = 5: the library path) against the fp32 graph, which
    tests/test_codec_cpu.py and the test above hold to the reference -- by the method and tolerances of
    tests/test_gpu_train_kernels.py::test_hip_graph_training_step_vs_fp32_graph for the uncompressed graph: loss within 2 %, the running
    statistics of EVERY BatchNorm (bn_compress / bn_decompress, and bn4_* / bn5_*, which see a codec applied in the wrong place) within 2 % of
    their scale, gradient cosine over all parameters > 0.95 and no worse than 0.02 below the control (the fp32 graph on bf16-rounded weights),
    gradient norm within 10 %."""
    import copy
    import warnings
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.det import V2VNet
    from v2x_sim_amd.train import detection_loss, train_forward
    from v2x_sim_amd.train.loop import synthetic_batch_on_device
    from v2x_sim_amd.utils.synthetic import init_synthetic_weights
    cfg = Config("train")
    data = synthetic_batch_on_device(cfg, 1, 2, seed=5, device=device)
    for k in (2, 5):
        base = init_synthetic_weights(V2VNet(cfg, num_agent=2, compress_level=k), seed=3).to(device)
        out = {}
        for flag in ("0", "1", "0r"):
            tune("TRAIN_HIP", int(flag[0]))
            model = copy.deepcopy(base)
            model.train()
            if flag == "0r":
                with torch.no_grad():
                    for p in model.parameters():
                        p.copy_(p.to(torch.bfloat16).float())
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res = train_forward(model, data["bev_seq"], data["trans_matrices"], data["num_agent"], 1)
            loss = detection_loss(res, data["labels"], data["reg_targets"], data["reg_loss_mask"])[0]
            loss.backward()
            out[flag] = (float(loss.detach()), {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None},
                         {n: b.detach().float().clone() for n, b in model.named_buffers() if "running" in n})
        tune.reset("TRAIN_HIP")
        l0, g0, b0 = out["0"]
        l1, g1, b1 = out["1"]
        print("k=%d loss: fp32 graph %.5f, HIP graph %.5f, control %.5f" % (k, l0, l1, out["0r"][0]))
        assert abs(l1 - l0) <= 2e-2 * abs(l0), k
        assert set(g0) == set(g1) and "u_encoder.com_decompresser.weight" in g1
        assert "u_encoder.bn_compress.running_mean" in b0
        for n in b0:
            assert float((b1[n] - b0[n]).abs().max()) <= 2e-2 * max(float(b0[n].abs().max()), 1e-3), (k, n)

        def cosine(ga, gb):
            dot = sum(float((ga[n] * gb[n]).sum()) for n in ga)
            na = sum(float((ga[n] ** 2).sum()) for n in ga) ** 0.5
            nb = sum(float((gb[n] ** 2).sum()) for n in ga) ** 0.5
            return dot / (na * nb), na, nb
        c_hip, n0, n1 = cosine(g0, g1)
        c_ctl, _, _ = cosine(g0, out["0r"][1])
        print("k=%d gradient cosine vs the fp32 graph: HIP graph %.4f, control %.4f; norms %.4e / %.4e" % (k, c_hip, c_ctl, n0, n1))
        assert c_hip > 0.95 and c_hip >= c_ctl - 0.02 and abs(n1 - n0) <= 0.1 * n0, k

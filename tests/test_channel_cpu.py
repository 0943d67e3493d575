"""Degraded links without a GPU: construction, set_channel, the plans a degraded model builds, the C ABI's argument
checks, the tools' flags, and the refusals (when2com, training, the sharded runners, the baselines)."""
import pytest
import torch

import channel_refs as CR


def _cfg():
    from v2x_sim_amd.configs import Config
    return Config("train")


def test_base_accepts_p_com_outage_and_has_set_channel():
    from v2x_sim_amd.models.det.base import IntermediateModelBase
    m = IntermediateModelBase(_cfg(), kd_flag=0, p_com_outage=0.3)
    assert m.p_com_outage == 0.3 and m.pose_noise == 0.0
    m.set_channel(p_com_outage=0.5, pose_noise=0.25, seed=(1 << 40) + 3)
    assert (m.p_com_outage, m.pose_noise) == (0.5, 0.25) and m._channel[2] == (1 << 40) + 3
    m.set_channel()
    assert m._channel is None and m.p_com_outage == 0.0
    assert IntermediateModelBase(_cfg(), kd_flag=0)._channel is None
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            IntermediateModelBase(_cfg(), kd_flag=0, p_com_outage=bad)
        with pytest.raises(ValueError):
            m.set_channel(p_com_outage=bad)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            m.set_channel(pose_noise=bad)
    with pytest.raises(ValueError):
        m.set_channel(p_com_outage=0.1, seed=-1)
    with pytest.raises(ValueError):
        m.set_channel(p_com_outage=0.1, seed=1 << 64)


def test_step_counter_on_the_host_side():
    from v2x_sim_amd.models.det import MeanFusion
    m = MeanFusion(_cfg())
    assert m.channel_step() == 0 and m.last_links() is None
    m.reset_channel(41)
    assert m.channel_step() == 41
    m.set_channel(p_com_outage=0.3)
    m.make_plan(torch.full((2, 5), 5), 2, "cpu")
    assert m.channel_step() == 41                       # the counter a plan allocates starts where reset_channel left it
    m.reset_channel((1 << 32) - 1)
    assert m.channel_step() == (1 << 32) - 1
    with pytest.raises(ValueError):
        m.reset_channel(-1)


def test_when2com_refuses_outage_and_takes_pose_noise():
    from v2x_sim_amd.models.det import When2com
    from v2x_sim_amd.models.seg import When2comSeg
    for cls in (When2com, When2comSeg):
        m = cls(_cfg()) if cls is When2com else cls(_cfg(), num_agent=5)
        with pytest.raises(NotImplementedError):
            m.set_channel(p_com_outage=0.3)
        with pytest.raises(NotImplementedError):
            m.set_channel(p_com_outage=0.3, pose_noise=0.5)
        assert m._channel is None
        m.set_channel(pose_noise=0.5, seed=3)
        assert m.pose_noise == 0.5 and m.p_com_outage == 0.0
        plan = m.make_plan(torch.tensor([[3] * 5, [5] * 5]), 2, "cpu")
        ch = plan["channel"]
        assert ch["coef0"] is None and ch["links"] is None and tuple(ch["trans"].shape) == (2, 5, 5, 4, 4) and ch["sigma"] == 0.5
        with pytest.raises(ValueError):
            m.set_channel(p_com_outage=2.0)             # outside [0, 1] is a ValueError everywhere


@pytest.mark.parametrize("name", ["SumFusion", "MeanFusion", "MaxFusion", "CatFusion", "DiscoNet", "V2VNet"])
def test_degraded_plans_keep_their_static_rows(name):
    """set_channel follows set_link_mask's rule: the next make_plan() takes it, a plan built before keeps its condition; an undegraded plan is
    the parent's dict; a degraded one carries the static rows, the live buffers and the pose buffer next to the family's own entries."""
    from v2x_sim_amd.models import det
    m = getattr(det, name)(_cfg())
    nat = torch.tensor([[5] * 5, [3] * 5])
    plain = m.make_plan(nat, 2, "cpu")
    assert "channel" not in plain
    m.set_channel(p_com_outage=0.3, pose_noise=0.5, seed=9)
    plan = m.make_plan(nat, 2, "cpu")
    assert set(plan) == set(plain) | {"channel"}
    for k, v in plain.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(plan[k], v), k           # the family's own entries stay the static plan's, bit for bit
    ch = plan["channel"]
    items, coef0 = CR.static_plan([5, 3], 5, "v2v" if name == "V2VNet" else "fusion")
    assert plan["items"].tolist() == [list(t) for t in items] and torch.equal(ch["coef0"], torch.from_numpy(coef0))
    assert (ch["p"], ch["sigma"], ch["seed"], ch["Bt"]) == (0.3, 0.5, 9, 2)
    assert ch["coef"].shape == ch["coef0"].shape and ch["coef"].data_ptr() != ch["coef0"].data_ptr()
    assert tuple(ch["links"].shape) == (2, 5, 5) and ch["links"].dtype == torch.uint8 and tuple(ch["trans"].shape) == (2, 5, 5, 4, 4)
    assert int(ch["possible"]) == 5 * 4 + 3 * 2
    live = ch["live"]
    assert live["coef"] is ch["coef"] and live["items"] is plan["items"]
    if name == "DiscoNet":
        assert live["valid"] is ch["coef"] and live["coef2"] is ch["coef2"] and ch["coef2"].shape == plain["coef2"].shape
    else:
        assert ch["coef2"] is None
    m.set_channel(pose_noise=0.5)
    assert plan["channel"]["p"] == 0.3                  # a plan built before keeps its condition
    only_pose = m.make_plan(nat, 2, "cpu")["channel"]
    assert only_pose["p"] == 0.0 and only_pose["trans"] is not None
    m.set_channel(p_com_outage=1.0)
    assert m.make_plan(nat, 2, "cpu")["channel"]["trans"] is None        # sigma = 0: no pose buffer, the caller's tensor is used
    m.set_channel()
    assert "channel" not in m.make_plan(nat, 2, "cpu")


def test_v2vnet_static_rule_stays():
    from v2x_sim_amd.models.det import V2VNet
    m = V2VNet(_cfg())
    m.set_channel(p_com_outage=1.0)
    with pytest.raises(RuntimeError):
        m.make_plan(torch.tensor([[5] * 5, [1] * 5]), 2, "cpu")         # a one-agent frame: the static rule, as without outage
    m.set_link_mask(torch.eye(5, dtype=torch.bool))
    with pytest.raises(RuntimeError):
        m.make_plan(torch.full((2, 5), 5), 2, "cpu")                    # an ego without a STATIC link
    m.set_link_mask(None)
    assert "channel" in m.make_plan(torch.full((2, 5), 5), 2, "cpu")    # p = 1 itself is accepted: the zero message


def test_abi_argument_checks_without_gpu():
    import ctypes as C
    from v2x_sim_amd import _lib
    lib = _lib.load()
    f, u = C.c_float, C.c_uint64
    one = C.c_void_p(64)            # non-null, aligned, never dereferenced: every call below returns before a launch
    assert lib.v2x_channel_degrade(None, 0, 99, 0, None, None, None, None, None, None, f(7.0), f(-1.0), u(0), None, None) == 0     # empty: before any check
    call = lambda A=5, p=0.3, s=0.0, items=one, c0=one, c=C.c_void_p(128), tr=None, tro=None, step=one: lib.v2x_channel_degrade(   # noqa: E731
        items, 4, A, 1, c0, c, None, None, tr, tro, f(p), f(s), u(1), step, None)
    for kw, text in ((dict(A=33), b"A=33"), (dict(A=0), b"A=0"), (dict(p=1.5), b"p_outage"), (dict(p=-0.1), b"p_outage"), (dict(p=float("nan")), b"p_outage"),
                     (dict(s=-1.0), b"pose_sigma"), (dict(s=float("inf")), b"pose_sigma"), (dict(s=float("nan")), b"pose_sigma"), (dict(items=None), b"null"),
                     (dict(step=None), b"null"), (dict(c0=None), b"coef0"), (dict(c0=None, c=None), b"need coef0"), (dict(s=0.5), b"trans_out"),
                     (dict(tro=one), b"trans_out"), (dict(s=0.5, tro=one), b"never in place"), (dict(step=C.c_void_p(68)), b"aligned")):
        assert call(**kw) == -22, kw
        assert text in lib.v2x_last_error(), (kw, lib.v2x_last_error())


def test_comm_flags_reach_the_constructors_and_are_refused_for_the_baselines():
    from v2x_sim_amd.models.det import MeanFusion, V2VNet, When2com
    from v2x_sim_amd.utils import comm
    import argparse
    ap = argparse.ArgumentParser()
    comm.add_arguments(ap)
    a = ap.parse_args(["--p_com_outage", "0.25", "--pose_noise", "0.4", "--channel_seed", "12"])
    assert (a.p_com_outage, a.pose_noise, a.channel_seed) == (0.25, 0.4, 12)
    assert (ap.parse_args([]).p_com_outage, ap.parse_args([]).pose_noise, ap.parse_args([]).channel_seed) == (0.0, 0.0, 0)
    with comm.model_flags(p_com_outage=0.25, pose_noise=0.4, channel_seed=12) as flags:
        m = MeanFusion(_cfg())
        assert m._channel == (0.25, 0.4, 12) and flags.value["channel_models"] == [m]
        with pytest.raises(NotImplementedError):
            When2com(_cfg())
    with comm.model_flags(pose_noise=0.4):
        assert When2com(_cfg())._channel == (0.0, 0.4, 0)
    with comm.model_flags(compress_level=1):
        assert MeanFusion(_cfg())._channel is None
    assert MeanFusion(_cfg())._channel is None
    seen = {}

    def driver(argv):
        seen["argv"], seen["channel"] = argv, V2VNet(_cfg())._channel
        return {}
    res = comm.run_eval_driver(driver, ["--data", "d", "--com", "v2v", "--p_com_outage", "0.3", "--pose_noise", "0.5", "--channel_seed", "7"])
    assert seen == {"argv": ["--data", "d", "--com", "v2v"], "channel": (0.3, 0.5, 7)}
    assert (res["links_up"], res["links_possible"]) == (0, 0)                # nothing ran: nothing counted
    comm.run_eval_driver(driver, ["--com", "v2v"])
    assert seen["channel"] is None
    for com in ("lowerbound", "upperbound", "late"):
        for flag in ("--p_com_outage", "--pose_noise"):
            with pytest.raises(SystemExit):
                comm.run_eval_driver(driver, ["--com", com, flag, "0.3"])
    with pytest.raises(SystemExit):
        comm.run_eval_driver(driver, ["--com", "v2v", "--p_com_outage", "1.5"])
    with pytest.raises(SystemExit):
        comm.run_eval_driver(driver, ["--com", "v2v", "--pose_noise", "-1"])
    # an evaluation condition: no checkpoint records it, none is checked against it
    assert set(comm.checkpoint_fields(a)) == {"compress_level", "only_v2i"}
    comm.check_checkpoint({"compress_level": 0, "only_v2i": False, "p_com_outage": 0.9}, a)
    with pytest.raises(SystemExit):
        comm.refuse_channel_in_training(a)
    comm.refuse_channel_in_training(ap.parse_args([]))
    assert "0.7500" in comm.channel_report(3, 4, {"p_com_outage": 0.3, "pose_noise": 0.0, "channel_seed": 1})


def test_training_refuses_outage_on_either_engine():
    from v2x_sim_amd.models.det import MeanFusion
    from v2x_sim_amd.train import graph, hip_graph
    m = MeanFusion(_cfg(), num_agent=2)
    m.set_channel(p_com_outage=0.3)
    bev = torch.zeros((2, 1, 32, 32, 13))
    for engine in (graph, hip_graph):
        with pytest.raises(NotImplementedError, match="outage"):
            engine.train_forward(m, bev, torch.eye(4).expand(1, 2, 2, 4, 4), torch.full((1, 2), 2), batch_size=1)


def test_sharded_runners_refuse_a_degraded_model():
    from v2x_sim_amd.models.det import V2VNet, When2com
    from v2x_sim_amd.parallel import AgentShard, ShardedV2VNet, ShardedWhen2com
    shard = AgentShard(5, 2)
    v = V2VNet(_cfg())
    ShardedV2VNet(v, shard)
    for kw in (dict(p_com_outage=0.3), dict(pose_noise=0.5)):
        v.set_channel(**kw)
        with pytest.raises(NotImplementedError, match="sharded"):
            ShardedV2VNet(v, shard)
    w = When2com(_cfg())
    ShardedWhen2com(w, shard)
    w.set_channel(pose_noise=0.5)
    with pytest.raises(NotImplementedError, match="sharded"):
        ShardedWhen2com(w, shard)

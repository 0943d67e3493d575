"""What every model says about itself -- FAMILY, backbone(), head() -- and what asks it: the fusion-stage tables of the two training engines
(train/graph.py, train/hip_graph.py) and the capture rule of the step modules (train/graph_step.py).  Host side: construction only."""
import types

import pytest
import torch

A = 2


@pytest.fixture(scope="module")
def cfg():
    from v2x_sim_amd.configs import Config
    return Config("train", binary=True, only_det=True)


def _det_classes():
    from v2x_sim_amd.models import det
    return [getattr(det, n) for n in ("FaFNet", "V2VNet", "When2com", "SumFusion", "MeanFusion", "MaxFusion", "CatFusion", "DiscoNet")]


def _twins():
    from v2x_sim_amd.models import det, seg
    return [(getattr(seg, d.__name__ + "Seg"), d) for d in _det_classes()]


def test_every_class_names_a_family_both_engines_know():
    from v2x_sim_amd.models import det, seg
    from v2x_sim_amd.models.det import base, fusion
    from v2x_sim_amd.train import graph, hip_graph
    abstract = (base.DetModelBase, base.NonIntermediateModelBase, base.IntermediateModelBase, fusion.FusionBase)
    exported = [v for v in vars(det).values() if isinstance(v, type) and issubclass(v, base.DetModelBase) and v not in abstract]
    assert set(exported) == set(_det_classes())              # every model class the package exports, none forgotten here
    want = {"FaFNet": "faf", "V2VNet": "v2v", "When2com": "when2com", "SumFusion": "fusion", "MeanFusion": "fusion", "MaxFusion": "fusion",
            "CatFusion": "fusion", "DiscoNet": "disco"}
    for cls in set(exported) | set(seg.COM_CLASSES.values()):
        assert cls.FAMILY is not None, cls.__name__
        for table in (graph.FUSION_STAGES, hip_graph.FUSION_STAGES):
            assert cls.FAMILY in table, cls.__name__
            assert (table[cls.FAMILY] is None) == (cls.FAMILY == "faf"), cls.__name__          # "faf" is known as "no stage"; every other has one
    for d in _det_classes():
        assert d.FAMILY == want[d.__name__]
    assert all(cls.FAMILY is None for cls in abstract)
    assert sorted(graph.FUSION_STAGES) == sorted(hip_graph.FUSION_STAGES) == sorted(set(want.values()))


def test_segmentation_classes_are_their_twins_with_one_mixin(cfg):
    from v2x_sim_amd.models import seg
    assert {s for s, _ in _twins()} == set(seg.COM_CLASSES.values())
    for s_cls, d_cls in _twins():
        assert s_cls.__bases__ == (seg.SegHeadMixin, d_cls) and s_cls.FAMILY == d_cls.FAMILY
        kw = {"image_size": 128} if d_cls.__name__ == "When2com" else {}
        s, d = s_cls(cfg, num_agent=A, **kw), d_cls(cfg, num_agent=A, **kw)
        enc, dec = s.backbone()
        twin = d.stpn if d.FAMILY == "faf" else d
        names = ("encoder", "decoder") if d.FAMILY == "faf" else ("u_encoder", "decoder")
        own = s.stpn if d.FAMILY == "faf" else s
        assert enc is getattr(own, names[0]) and dec is getattr(own, names[1])
        assert d.backbone() == (getattr(twin, names[0]), getattr(twin, names[1]))
        assert type(enc).__name__ == "LidarEncoder" and type(dec).__name__ == "LidarDecoder"
        assert s_cls.head is seg.SegHeadMixin.head and d_cls.head is not s_cls.head
        if d_cls.__name__ not in ("FaFNet", "When2com"):
            assert s_cls.forward_nhwc is d_cls.forward_nhwc, s_cls.__name__               # no copy has come back
    assert seg.FaFNetSeg.forward_nhwc is seg.FaFNet.forward_nhwc
    assert "forward_nhwc" in vars(seg.When2comSeg) and list(vars(seg.FaFNetSeg)) == list(vars(seg.V2VNetSeg))     # only When2comSeg has a body


def test_unknown_family_has_no_training_graph(cfg):
    from v2x_sim_amd.models.det.base import IntermediateModelBase
    from v2x_sim_amd.train import graph, hip_graph

    class Odd(IntermediateModelBase):
        FAMILY = "odd"
    m = Odd(cfg, kd_flag=0, num_agent=A)
    for table in (graph.FUSION_STAGES, hip_graph.FUSION_STAGES):
        with pytest.raises(NotImplementedError):
            graph.fusion_stage_of(table, m)
    with pytest.raises(NotImplementedError):
        graph.train_forward(m.train(), torch.zeros((A, 1, 64, 64, 13)), torch.eye(4).repeat(1, A, A, 1, 1), torch.full((1, A), A), batch_size=1)


def _graph_ok_of_the_parent(model, optimizer, data, cached):
    """utils/CoDetModule.py::FaFModule._graph_ok as it stood before the rule moved (past the switches and the class-head check)."""
    if hasattr(model, "convgru"):
        if cached is not None and not torch.equal(data["num_agent"].cpu(), cached.num_agent):
            return False
    elif not hasattr(model, "stpn"):
        return False
    return all(g.get("capturable", True) for g in optimizer.param_groups)


def _batch(nat):
    return {"bev_seq": torch.zeros(A, 1, 8, 8, 13), "labels": torch.zeros(A, 8, 8), "reg_targets": torch.zeros(A, 8, 8, 6, 1, 6),
            "reg_loss_mask": torch.zeros(A, 8, 8, 6, 1), "num_agent": nat}


@pytest.mark.parametrize("capturable", [True, False])
@pytest.mark.parametrize("name", ["FaFNet", "V2VNet", "When2com", "SumFusion", "DiscoNet"])
def test_capture_rule_by_family(cfg, tune, name, capturable):
    """capture_ok gives what _graph_ok gave for a model of each family, detection and segmentation; the two modules' _graph_ok are that rule
    behind their switches, with the cached step looked up -- not created -- on the optimizer."""
    from v2x_sim_amd.models import det, seg
    from v2x_sim_amd.train.graph_step import cached_step, capture_ok
    from v2x_sim_amd.utils.CoDetModule import FaFModule
    from v2x_sim_amd.utils.SegModule import SegModule
    same, other = torch.full((1, A), A), torch.tensor([[A, A - 1]])
    stub = types.SimpleNamespace(num_agent=same.clone())
    captures = name in ("FaFNet", "V2VNet")
    kw = {"image_size": 128} if name == "When2com" else {}
    for mod, cls in ((det, getattr(det, name)), (seg, getattr(seg, name + "Seg"))):
        model = cls(cfg, num_agent=A, **kw)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=capturable)
        for nat, cached in ([(same, None), (same, stub), (other, stub)] if name == "V2VNet" else [(same, None)]):
            got = capture_ok(model, opt, {"num_agent": nat}, cached)
            assert got is _graph_ok_of_the_parent(model, opt, {"num_agent": nat}, cached)
            assert got is (captures and capturable and nat is not other), (name, capturable)
        module = SegModule(model, None, cfg, opt) if mod is seg else FaFModule(model, None, cfg, opt, 0)
        for k in ("TRAIN_HIP", "TRAIN_GRAPH", "TRAIN_SEG_GRAPH"):
            tune(k, 1)
        data = _batch(same)
        key = module._graph_key(data, 1)
        assert module._graph_ok(data, 1) is (captures and capturable)
        assert "_v2x_graphed_steps" not in opt.__dict__ and cached_step(opt, key) is None
        if name == "V2VNet":
            assert cached_step(opt, key, lambda: stub) is stub and opt.__dict__["_v2x_graphed_steps"] == {key: stub}
            assert cached_step(opt, key, lambda: None) is stub                       # built once per key
            assert module._graph_ok(data, 1) is capturable and module._graph_ok(_batch(other), 1) is False
        tune("TRAIN_GRAPH", 0)
        tune("TRAIN_SEG_GRAPH", 0)
        assert module._graph_ok(data, 1) is False


def test_each_step_module_refuses_the_other_tasks_models(cfg, tune):
    from v2x_sim_amd.models import det, seg
    from v2x_sim_amd.utils.CoDetModule import FaFModule
    from v2x_sim_amd.utils.SegModule import SegModule
    for k in ("TRAIN_HIP", "TRAIN_GRAPH", "TRAIN_SEG_GRAPH"):
        tune(k, 1)
    faf, fafseg = det.FaFNet(cfg, num_agent=A), seg.FaFNetSeg(cfg, num_agent=A)
    sgd = lambda m: torch.optim.SGD(m.parameters(), lr=0.1)  # noqa: E731
    data = _batch(torch.full((1, A), A))
    assert FaFModule(faf, None, cfg, sgd(faf), 0)._graph_ok(data, 1) is True and FaFModule(fafseg, None, cfg, sgd(fafseg), 0)._graph_ok(data, 1) is False
    assert SegModule(fafseg, None, cfg, sgd(fafseg))._graph_ok(data, 1) is True and SegModule(faf, None, cfg, sgd(faf))._graph_ok(data, 1) is False


def test_run_batch_is_the_forward_of_each_family(cfg, monkeypatch):
    """run_batch hands each family's forward() what it takes: FaFNet the sweeps alone, when2com the inference mode, the others the exchange."""
    from v2x_sim_amd.models import det
    data = {"bev_seq": "bev", "trans_matrices": "T", "num_agent": "nat"}
    seen = []
    for cls in (det.FaFNet, det.V2VNet, det.When2com, det.SumFusion):
        monkeypatch.setattr(cls, "forward", lambda self, *a, **k: seen.append((type(self).__name__, a, k)))
    for cls in (det.FaFNet, det.V2VNet, det.When2com, det.SumFusion):
        cls(cfg, num_agent=A, **({"image_size": 128} if cls is det.When2com else {})).run_batch(data, 3, "argmax_test")
    assert seen == [("FaFNet", ("bev",), {}), ("V2VNet", ("bev", "T", "nat"), {"batch_size": 3}),
                    ("When2com", ("bev", "T", "nat"), {"training": False, "inference": "argmax_test", "batch_size": 3}),
                    ("SumFusion", ("bev", "T", "nat"), {"batch_size": 3})]

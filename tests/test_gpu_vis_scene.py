"""Ray-cast segmentation batches (utils/raycast_scene.raycast_seg_batch_on_device): occlusion shows in the labels -- a car behind
a wall is the ignore class for the agent in front of the wall and class 1 for the agent behind it, and for both once any agent's rays count --, the
detection batch keeps its keys and bytes without vis_maps, a FaFNetSeg trains on such a batch on both engines and the training tool takes the flags."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAYS = dict(beams=32, steps=256)


def _two_agent_world():
    """Agent 0 at the origin looking along +x, a wall across x = 6, a car at (10, 0) behind it, agent 1 at (16, 0) looking back along -x: the car lies in
    the wall's shadow for agent 0 (the wall subtends +-46 degrees, the car +-7) and 4 to 8 m in front of agent 1, where 256 azimuths are at most
    0.2 m apart -- less than a cell."""
    from v2x_sim_amd.utils import raycast_scene as RS
    from v2x_sim_amd.utils import synthetic_scene
    boxes = np.zeros((1, 4, 7), np.float32)
    boxes[0, 0] = (0.0, 0.0, 4.4, 2.0, 0.0, RS.GROUND_Z, RS.AGENT_TOP)
    boxes[0, 1] = (16.0, 0.0, 4.4, 2.0, math.pi, RS.GROUND_Z, RS.AGENT_TOP)
    boxes[0, 2] = (10.0, 0.0, 4.0, 2.0, 0.0, RS.GROUND_Z, RS.CAR_TOP)
    boxes[0, 3] = (6.0, 0.0, 0.5, 12.0, 0.0, RS.GROUND_Z, RS.WALL_TOP)
    sensors = np.array([[0.0, 0.0, 0.0, 0.0], [16.0, 0.0, 0.0, math.pi]], np.float32)
    P = [synthetic_scene._pose(float(boxes[0, a, 4]), float(boxes[0, a, 0]), float(boxes[0, a, 1])) for a in range(2)]
    T, T_geo = synthetic_scene.warp_transforms(P)
    return {"sensors": sensors, "frame_of": np.zeros(2, np.int32), "boxes": boxes, "box_count": np.array([4], np.int32),
            "car_count": np.array([3], np.int32), "trans": T[None], "trans_geo": T_geo[None], "num_agent": np.full((1, 2), 2, np.int64)}


def _cells(x0, x1, y0, y1):
    """cell-index slices of the window [x0, x1] x [y0, y1] metres on the product grid (0.25 m cells, -32 m at index 0), one cell inside its border"""
    return (slice(int(x0 / 0.25) + 128 + 1, int(x1 / 0.25) + 128 - 1), slice(int(y0 / 0.25) + 128 + 1, int(y1 / 0.25) + 128 - 1))


@pytest.fixture(scope="module")
def labels(device):
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.utils import raycast_scene as RS
    cfg = Config("train", binary=True, only_det=True)
    out = {}
    for observed in ("own", "any", "all"):
        d = RS.raycast_seg_batch_on_device(cfg, 1, 2, 3, device, observed=observed, world=_two_agent_world(), sigma_r=0.0, **RAYS)
        assert set(d) == {"bev_seq", "trans_matrices", "num_agent", "labels"}
        assert d["labels"].dtype == torch.uint8 and tuple(d["labels"].shape) == (2, 256, 256) and tuple(d["bev_seq"].shape) == (2, 1, 256, 256, 13)
        out[observed] = d["labels"].cpu().numpy()
    return out


def test_occlusion_shows_in_the_labels(labels):
    car0 = _cells(8.0, 12.0, -1.0, 1.0)          # the car in agent 0's frame (= the world's)
    car1 = _cells(4.0, 8.0, -1.0, 1.0)           # ... in agent 1's: 6 m ahead
    painted = labels["all"]
    assert not (painted == 255).any()
    assert (painted[0][car0] == 1).all() and (painted[1][car1] == 1).all()
    assert (painted[0][151:153, _cells(0.0, 1.0, -6.0, 6.0)[1]] == 2).all()         # the wall: the two cell columns x in [5.75, 6.25]
    assert (painted[0][_cells(-2.2, 2.2, -1.0, 1.0)] == 1).all() and (painted[1][_cells(-2.2, 2.2, -1.0, 1.0)] == 1).all()      # the ego cars
    assert set(np.unique(painted)) == {0, 1, 2}
    own = labels["own"]
    assert (own[0][car0] == 255).all(), "agent 0 saw the car through the wall"
    assert (own[1][car1] == 1).all(), "agent 1 did not observe the car in front of it"
    assert (own[0][_cells(-2.2, 2.2, -1.0, 1.0)] == 1).all()                        # its own car: every ray starts there
    assert (own[0][_cells(7.0, 30.0, -1.0, 1.0)] == 255).all()                      # the whole shadow
    anyone = labels["any"]
    assert (anyone[0][car0] == 1).all() and (anyone[1][car1] == 1).all()
    for a in range(2):
        seen_own, seen_any = own[a] != 255, anyone[a] != 255
        assert not (seen_own & ~seen_any).any() and (seen_any & ~seen_own).any()     # a neighbour only adds
        assert np.array_equal(own[a][seen_own], painted[a][seen_own]) and np.array_equal(anyone[a][seen_any], painted[a][seen_any])


def test_detection_batch_is_unchanged_without_vis_maps(device):
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.utils import raycast_scene as RS
    cfg = Config("train", binary=True, only_det=True)
    kw = dict(world=_two_agent_world(), **RAYS)
    base = RS.raycast_batch_on_device(cfg, 1, 2, 3, device, **kw)
    off = RS.raycast_batch_on_device(cfg, 1, 2, 3, device, vis_maps=False, **kw)
    on = RS.raycast_batch_on_device(cfg, 1, 2, 3, device, vis_maps=True, **kw)
    assert set(base) == set(off) == {"bev_seq", "trans_matrices", "num_agent", "labels", "reg_targets", "reg_loss_mask"}
    assert set(on) == set(base) | {"vis_maps"}
    for k in base:
        assert torch.equal(base[k], off[k]) and torch.equal(base[k], on[k]), k
    m = on["vis_maps"]
    assert tuple(m.shape) == (2, 256, 256, 13) and m.dtype == torch.float32
    v_occ, v_free = float(np.float32(math.log(0.7 / 0.3))), float(np.float32(math.log(0.4 / 0.6)))
    assert sorted(float(v) for v in torch.unique(m)) == sorted([v_free, 0.0, v_occ])
    assert torch.equal(m == v_occ, base["bev_seq"][:, 0] == 1.0)                    # occupied is the voxeliser's result


@pytest.mark.parametrize("engine", ["torch", "hip"])
def test_fafnetseg_trains_on_a_raycast_batch(device, tune, engine):
    from v2x_sim_amd.configs import Config
    from v2x_sim_amd.models.seg import FaFNetSeg
    from v2x_sim_amd.train.loop import init_for_training
    from v2x_sim_amd.utils import raycast_scene as RS
    from v2x_sim_amd.utils.SegModule import SegModule
    tune("TRAIN_HIP", int(engine == "hip"))
    for name in ("TRAIN_SEG_LOSS_HIP", "TRAIN_SEG_HEAD_FUSE", "TRAIN_SEG_GRAPH"):
        tune(name, 0)
    cfg = Config("train", binary=True, only_det=True)
    data = RS.raycast_seg_batch_on_device(cfg, 1, 2, 3, device, observed="own", world=_two_agent_world(), **RAYS)
    assert bool((data["labels"] == 255).any())
    model = init_for_training(FaFNetSeg(cfg, num_agent=2), seed=2).to(device)
    module = SegModule(model, None, cfg, torch.optim.Adam(model.parameters(), lr=1e-3), 0)
    losses = [module.step(data, 2, 1) for _ in range(3)]
    assert all(np.isfinite(v) for v in losses), losses


def test_train_seg_takes_the_raycast_flags(device, capsys):
    spec = importlib.util.spec_from_file_location("train_seg_cli_vis", os.path.join(ROOT, "tools", "seg", "train_seg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.BALANCE_BATCHES = 2                                                          # the histogram of two batches is a histogram
    mod.main(["--com", "lowerbound", "--scene", "raycast", "--observed", "any", "--class_weight", "balanced", "--steps", "2", "--batch", "1", "--num_agent", "2"])
    out = capsys.readouterr().out
    assert "class weights (median frequency)" in out and "mean loss of the last 20 steps" in out
    loss = float(out.rsplit("mean loss of the last 20 steps", 1)[1].split()[0])
    assert np.isfinite(loss)

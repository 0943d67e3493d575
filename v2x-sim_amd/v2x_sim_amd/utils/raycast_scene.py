"""Seeded synthetic collaborative scenes WITH OCCLUSION: a world of boxes -- cars and walls -- swept by every agent's
32-beam LiDAR on the device (ops.lidar_cast), with the ground truth "the cars this agent (or any agent) actually got returns from" (ops.visible_boxes),
the num_lidar_pts rule of the real data preparation.  The host makes poses and boxes only, a few hundred floats (`make_world`); points, occupancy,
ground truth and anchor targets never leave the device (`raycast_batch_on_device`).

utils/synthetic_scene.make_scene is the sampled twin: 400 random points on every car in range whether or not anything stands in between.  Here a car
behind a wall returns nothing to the agent in front of it, and collaboration helps because a neighbour sees it from the other side.

The world, in the z range make_scene uses: ground at -1.8, car roofs at -0.25, walls up to +2.0.  Agents ARE cars, with the sensor at the origin of
their frame (z = 0): an agent's own box reaches up to the sensor (z1 = 0, the mast), so it CONTAINS the sensor origin and by the rule returns nothing to
its own sweep and is never its own ground truth -- no special case.  Cars come first in the box table, walls after them: the ground truth reads the
table with the car count, so a wall is never a label."""
import math

import numpy as np

from . import synthetic_scene
from .synthetic_scene import CAR_H, CAR_W

GROUND_Z, CAR_TOP, AGENT_TOP, WALL_TOP = -1.8, -0.25, 0.0, 2.0


def _radius(w, h):
    return 0.5 * math.hypot(w, h)


def make_world(frames, agents=5, seed=0, n_cars=24, n_walls=8, extent=40.0, agent_extent=12.0):
    """`frames` worlds of `n_cars` cars (the first `agents` of them carry the sensors) and `n_walls` walls, none overlapping (bounding circles apart).
    Agent-major sweeps, the models' batch order: sweep m = a * frames + b belongs to frame b.
    -> dict(sensors (A*B, 4) f32 x, y, z, yaw; frame_of (A*B,) i32; boxes (B, cap, 7) f32 x, y, w, h, yaw, z0, z1 with cap = n_cars + n_walls, cars
    first; box_count (B,) i32 = cars + walls placed; car_count (B,) i32; trans / trans_geo (B, A, A, 4, 4) f32 as synthetic_scene.make_scene gives
    them (synthetic_scene.warp_transforms); num_agent (B, A) i64)."""
    if agents > n_cars:
        raise ValueError("make_world: %d agents among %d cars" % (agents, n_cars))
    cap = max(1, n_cars + n_walls)
    boxes = np.zeros((frames, cap, 7), np.float32)
    box_count, car_count = np.zeros((frames,), np.int32), np.zeros((frames,), np.int32)
    sensors = np.zeros((agents * frames, 4), np.float32)
    trans, trans_geo = [], []
    for b in range(frames):
        rng = np.random.default_rng(seed * 100003 + b)
        placed = []                                                   # (x, y, bounding radius)

        def place(lim, w, h):
            for _ in range(400):
                c = rng.uniform(-lim, lim, 2)
                r = _radius(w, h)
                if all(math.hypot(c[0] - x, c[1] - y) > r + q + 0.5 for x, y, q in placed):
                    placed.append((c[0], c[1], r))
                    return c
            return None

        rows = []
        for k in range(n_cars):
            w, h = CAR_W + rng.uniform(-0.15, 0.15), CAR_H + rng.uniform(-0.4, 0.4)
            c = place(agent_extent if k < agents else extent, w, h)
            if c is None:
                if k < agents:
                    raise RuntimeError("make_world: no room for agent %d" % k)
                continue
            rows.append((c[0], c[1], w, h, rng.uniform(-math.pi, math.pi), GROUND_Z, AGENT_TOP if k < agents else CAR_TOP))
        car_count[b] = len(rows)
        for _ in range(n_walls):
            w, h = rng.uniform(0.4, 0.6), rng.uniform(6.0, 14.0)
            c = place(extent, w, h)
            if c is not None:
                rows.append((c[0], c[1], w, h, rng.uniform(-math.pi, math.pi), GROUND_Z, WALL_TOP))
        boxes[b, :len(rows)], box_count[b] = np.asarray(rows, np.float32), len(rows)
        P = []
        for a in range(agents):
            x, y, yaw = (float(v) for v in boxes[b, a, [0, 1, 4]])      # the fp32 values the cast reads: the transforms describe the same poses
            sensors[a * frames + b] = (x, y, 0.0, yaw)
            P.append(synthetic_scene._pose(yaw, x, y))
        T, T_geo = synthetic_scene.warp_transforms(P)
        trans.append(T)
        trans_geo.append(T_geo)
    return {"sensors": sensors, "frame_of": np.tile(np.arange(frames, dtype=np.int32), agents), "boxes": boxes, "box_count": box_count,
            "car_count": car_count, "trans": np.stack(trans), "trans_geo": np.stack(trans_geo), "num_agent": np.full((frames, agents), agents, np.int64)}


def world_on_device(world, device):
    """make_world's tables in the form the kernels read -> dict of device tensors: sensors (n, 6), frame_of, boxes (F, cap, 9), box_count, car_count."""
    import torch
    from .. import ops
    F, cap = world["boxes"].shape[:2]
    rows = ops.box_rows(world["boxes"][..., :5].reshape(-1, 5), world["boxes"][..., 5].reshape(-1), world["boxes"][..., 6].reshape(-1)).reshape(F, cap, 9)
    host = {"sensors": ops.sensor_rows(world["sensors"]), "frame_of": world["frame_of"], "boxes": rows, "box_count": world["box_count"],
            "car_count": world["car_count"]}
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in host.items()}


_RINGS = {}


def _ring_on(device, beams, steps):
    import torch
    from .. import ops
    key = (str(device), beams, steps)
    if key not in _RINGS:
        _RINGS[key] = tuple(torch.from_numpy(t).to(device) for t in ops.ring_table(beams, steps))
    return _RINGS[key]


def raycast_batch_on_device(config, frames, agents, seed, device, grid=None, anchors=None, with_targets=True, gt="own", min_hits=5, gt_lists=False,
                            beams=32, steps=2048, max_pts=None, sigma_r=0.02, p_drop=0.0, r_min=1.0, r_max=70.0, step=0, world=None, **world_kw):
    """-> the data dict of train.loop.synthetic_batch_on_device (FaFModule.step / predict_all's format) from a ray-cast world, by this chain on the
    device: ops.lidar_cast, ops.visible_boxes, ops.voxelize_bits, ops.bits_to_dense, v2x_det_assign_targets (the IoU rule) --
    straight from the device's padded ground truth; nothing is synchronised.
    gt: "own": an agent's ground truth = the cars inside its BEV extents it got >= min_hits returns from; "any": ... that ANY agent of the frame got
    >= min_hits returns from (the cars the ego cannot see but a neighbour can: where collaboration must help).
    gt_lists: also data["gt_boxes"][agent][frame], host arrays (the one read-back; evaluation wants them).  world: a make_world dict to use instead
    of make_world(frames, agents, seed, **world_kw)."""
    import torch
    from .. import ops
    from ..train import loop
    from . import postprocess
    if gt not in ("own", "any"):
        raise ValueError("gt must be 'own' or 'any'")
    world = make_world(frames, agents, seed, **world_kw) if world is None else world
    grid = grid or ops.VoxelGrid(config.voxel_size, config.area_extents)
    d = world_on_device(world, device)
    beam, az = _ring_on(device, beams, steps)
    cast = ops.lidar_cast(d["sensors"], d["frame_of"], d["boxes"], d["box_count"], beam, az, max_pts or beams * steps, ground_z=GROUND_Z, r_min=r_min,
                          r_max=r_max, sigma_r=sigma_r, p_drop=p_drop, seed=seed, step=step, want=("box_hits",))
    x_lim = min(abs(float(config.area_extents[0][0])), abs(float(config.area_extents[0][1]))) - 3.0      # make_scene's 29 m inside +-32 m extents
    y_lim = min(abs(float(config.area_extents[1][0])), abs(float(config.area_extents[1][1]))) - 3.0
    gt_boxes, gt_count = ops.visible_boxes(cast["box_hits"], d["sensors"], d["frame_of"], d["boxes"], d["car_count"], min_hits=min_hits,
                                           any_agent=gt == "any", x_lim=x_lim, y_lim=y_lim)
    bits = ops.voxelize_bits(cast["points"], cast["n_pts"], grid)
    data = {"bev_seq": ops.bits_to_dense(bits, grid.dims[2])[:, None], "trans_matrices": torch.from_numpy(world["trans"]).to(device),
            "num_agent": torch.from_numpy(world["num_agent"])}
    if gt_lists:
        hb, hc = gt_boxes.cpu().numpy(), gt_count.cpu().numpy()
        data["gt_boxes"] = [[hb[a * frames + f, :hc[a * frames + f]].copy() for f in range(frames)] for a in range(agents)]
    if with_targets:
        anchors = postprocess.build_anchor_map(config) if anchors is None else anchors
        data["labels"], data["reg_targets"], data["reg_loss_mask"] = loop.iou_targets_from_device(gt_boxes, gt_count, anchors, device)
    return data

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


def _ring_on(device, beams, steps, elev_deg=None):
    import torch
    from .. import ops
    key = (str(device), beams, steps) + (() if elev_deg is None else (float(elev_deg[0]), float(elev_deg[1])))
    if key not in _RINGS:
        _RINGS[key] = tuple(torch.from_numpy(t).to(device) for t in (ops.ring_table(beams, steps) if elev_deg is None else
                                                                      ops.ring_table(beams, steps, elev_deg)))
    return _RINGS[key]


def raycast_batch_on_device(config, frames, agents, seed, device, grid=None, anchors=None, with_targets=True, gt="own", min_hits=5, gt_lists=False,
                            beams=32, steps=2048, max_pts=None, sigma_r=0.02, p_drop=0.0, r_min=1.0, r_max=70.0, step=0, world=None, vis_maps=False,
                            **world_kw):
    """-> the data dict of train.loop.synthetic_batch_on_device (FaFModule.step / predict_all's format) from a ray-cast world, by this chain on the
    device: ops.lidar_cast, ops.visible_boxes, ops.voxelize_bits, ops.bits_to_dense, v2x_det_assign_targets (the IoU rule) --
    straight from the device's padded ground truth; nothing is synchronised.
    gt: "own": an agent's ground truth = the cars inside its BEV extents it got >= min_hits returns from; "any": ... that ANY agent of the frame got
    >= min_hits returns from (the cars the ego cannot see but a neighbour can: where collaboration must help).
    gt_lists: also data["gt_boxes"][agent][frame], host arrays (the one read-back; evaluation wants them).  world: a make_world dict to use instead
    of make_world(frames, agents, seed, **world_kw).  vis_maps: also data["vis_maps"] (A * frames, X, Y, Z) fp32, upstream's three-state visibility
    map of each sweep's own rays (ops.freespace_bits, ops.vis_maps); without it keys and bytes are what they were."""
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
    if vis_maps:
        data["vis_maps"] = ops.vis_maps(bits, ops.freespace_bits(cast["points"], cast["n_pts"], grid), grid.dims[2])
    if gt_lists:
        hb, hc = gt_boxes.cpu().numpy(), gt_count.cpu().numpy()
        data["gt_boxes"] = [[hb[a * frames + f, :hc[a * frames + f]].copy() for f in range(frames)] for a in range(agents)]
    if with_targets:
        anchors = postprocess.build_anchor_map(config) if anchors is None else anchors
        data["labels"], data["reg_targets"], data["reg_loss_mask"] = loop.iou_targets_from_device(gt_boxes, gt_count, anchors, device)
    return data


# ---- segmentation batches -------------------------------------------------------------------------------------------------
SEG_CAR, SEG_WALL = 1, 2
OBSERVED = ("own", "any", "all")


def fused_jobs(world, frames, agents):
    """The early-fusion jobs of a frame-major world, as tools/bench_configs.py builds the upperbound's: for every frame f and ego i, one job per agent j
    moving sweep j * frames + f into grid i * frames + f.  The transform moves POINTS, so it is the geometric one, world["trans_geo"][f, i, j] =
    inv(P_i) P_j (world["trans"] holds the same poses in the feature warp's axis convention, translation swapped).  -> (xform (n_jobs, 3, 4) f32,
    src (n_jobs,) i32, dst (n_jobs,) i32) host arrays."""
    xf, src, dst = [], [], []
    for f in range(frames):
        for i in range(agents):
            for j in range(agents):
                xf.append(world["trans_geo"][f, i, j][:3])
                src.append(j * frames + f)
                dst.append(i * frames + f)
    return np.ascontiguousarray(np.stack(xf), np.float32), np.asarray(src, np.int32), np.asarray(dst, np.int32)


def raycast_seg_batch_on_device(config, frames, agents, seed, device, observed="own", n_classes=8, grid=None, beams=32, steps=2048, max_pts=None,
                                sigma_r=0.02, p_drop=0.0, r_min=1.0, r_max=70.0, step=0, world=None, want_hist=False, **world_kw):
    """-> the segmentation batch dict SegModule.step takes (bev_seq, trans_matrices, num_agent, labels (A * frames, X, Y) uint8) from a ray-cast world,
    by this chain on the device with nothing synchronised: ops.lidar_cast, ops.voxelize_bits, the world's boxes in each agent's frame
    (ops.visible_boxes_moving with zero velocities, min_hits = 0 and no limits: every box, with its index), ops.rasterize_seg, ops.mask_unobserved.
    Classes: cars 1 (the ego car too: the box that contains the sensor is dropped by the visibility rule, so it is painted from the world table, at
    the origin of its own frame), walls 2, everything else 0.  A cell no ray observed -- behind a wall, under a car's far side -- is the ignore class
    255, the right label for what nobody saw.
    observed: "own": observed by the sweep's own rays; "any": by the rays of any agent of the frame, walked into the ego grid as fused jobs
    (fused_jobs; the occupancy that goes with them is ops.voxelize_fused_bits'); "all": no masking -- the painted world.
    want_hist: also data["hist"] (A * frames, n_classes + 1) int64, the rasteriser's cells per label (before masking)."""
    import torch
    from .. import ops
    if observed not in OBSERVED:
        raise ValueError("observed must be one of %s" % (OBSERVED,))
    world = make_world(frames, agents, seed, **world_kw) if world is None else world
    grid = grid or ops.VoxelGrid(config.voxel_size, config.area_extents)
    d = world_on_device(world, device)
    n, cap = agents * frames, world["boxes"].shape[1]
    beam, az = _ring_on(device, beams, steps)
    cast = ops.lidar_cast(d["sensors"], d["frame_of"], d["boxes"], d["box_count"], beam, az, max_pts or beams * steps, ground_z=GROUND_Z, r_min=r_min,
                          r_max=r_max, sigma_r=sigma_r, p_drop=p_drop, seed=seed, step=step, want=("box_hits",))
    bits = ops.voxelize_bits(cast["points"], cast["n_pts"], grid)
    # every box of the world -- cars and walls -- in each sweep's frame, with its index
    zero2 = torch.zeros((n, 2), dtype=torch.float32, device=device)
    vis = ops.visible_boxes_moving(cast["box_hits"], d["sensors"], zero2, torch.zeros((n,), dtype=torch.float32, device=device), d["frame_of"], d["boxes"],
                                   torch.zeros((frames, cap, 2), dtype=torch.float32, device=device), d["box_count"], t_ref=0.0, min_hits=0,
                                   x_lim=1e9, y_lim=1e9, want=())
    cars = d["car_count"][d["frame_of"].long()][:, None]
    cls = torch.where(vis["gt_ids"] < cars, SEG_CAR, SEG_WALL).to(torch.uint8)
    # row 0: the ego car, (0, 0, w, h, 0) in its own frame; sweep m = a * frames + b carries box a of frame b
    ego = np.zeros((n, 1, 5), np.float32)
    for a in range(agents):
        ego[a * frames:(a + 1) * frames, 0, 2:4] = world["boxes"][:, a, 2:4]
    boxes = torch.cat([torch.from_numpy(ego).to(device), vis["gt_boxes"]], 1)
    cls = torch.cat([torch.full((n, 1), SEG_CAR, dtype=torch.uint8, device=device), cls], 1)
    res = ops.rasterize_seg(boxes, cls, vis["gt_count"] + 1, grid, n_classes=n_classes, want=("hist",) if want_hist else ())
    labels = res["labels"]
    if observed == "own":
        ops.mask_unobserved(labels, bits, ops.freespace_bits(cast["points"], cast["n_pts"], grid), out=labels)
    elif observed == "any":
        xf, src, dst = (torch.from_numpy(t).to(device) for t in fused_jobs(world, frames, agents))
        occ = ops.voxelize_fused_bits(cast["points"], cast["n_pts"], xf, src, dst, n, grid)
        trav = ops.freespace_bits(cast["points"], cast["n_pts"], grid, xform=xf, src_cloud=src, dst_grid=dst, n_grids=n)
        ops.mask_unobserved(labels, occ, trav, out=labels)
    data = {"bev_seq": ops.bits_to_dense(bits, grid.dims[2])[:, None], "trans_matrices": torch.from_numpy(world["trans"]).to(device),
            "num_agent": torch.from_numpy(world["num_agent"]), "labels": labels}
    if want_hist:
        data["hist"] = res["hist"]
    return data


# ---- moving scenes (DESIGN.md section 3.12 "moving scenes") ---------------------------------------------------------------------------------------
# Straight lines at constant velocity with a fixed yaw.  The lane pitch, the speeds, the step and the sweep duration below are this build's choices:
# nothing here is taken from V2X-Sim's recording set-up.
LANE_PITCH = 6.0          # lanes run along the world's x axis at y = k * LANE_PITCH; a car is at most CAR_H + 0.4 = 4.8 m across its lane
DT, SWEEP_TIME = 0.2, 0.1


def make_moving_world(scenes, agents=5, seed=0, n_cars=24, n_walls=8, p_parked=0.25, speed=(3.0, 12.0), extent=40.0, agent_extent=12.0):
    """`scenes` worlds like make_world's, with motion: make_world's dict (sensors, trans, trans_geo at time 0; agent-major sweeps m = a * scenes + w)
    plus box_vel (scenes, cap, 2) f32 and sensor_vel (A * scenes, 2) f32, world-frame (vx, vy) in m/s.  Seeded like make_world.
    Cars stand in lanes along the world's x axis, LANE_PITCH apart, yaw 0 in one lane and pi in the next, and drive along their heading -- the axis
    of yaw, along which a box has its extent w (synthetic_scene's boxes, the default Config.box_wh_axis).  A lane has ONE speed, drawn from
    `speed` (lo, hi), or is a parking lane (probability p_parked; its cars have exactly zero velocity): two cars of a lane keep their distance, two
    cars of different lanes never meet, so no two car boxes overlap at any time.  The first `agents` cars carry the sensors (lanes within
    agent_extent of the origin); sensor_vel is their box's velocity.  Walls stand still, on the lines between two lanes, long side along the lanes."""
    if agents > n_cars:
        raise ValueError("make_moving_world: %d agents among %d cars" % (agents, n_cars))
    cap = max(1, n_cars + n_walls)
    boxes, box_vel = np.zeros((scenes, cap, 7), np.float32), np.zeros((scenes, cap, 2), np.float32)
    box_count, car_count = np.zeros((scenes,), np.int32), np.zeros((scenes,), np.int32)
    sensors, sensor_vel = np.zeros((agents * scenes, 4), np.float32), np.zeros((agents * scenes, 2), np.float32)
    trans, trans_geo = [], []
    k_max, k_agent = int(extent // LANE_PITCH), int(agent_extent // LANE_PITCH)
    for b in range(scenes):
        rng = np.random.default_rng(seed * 100003 + b)
        lanes = {}
        for k in range(-k_max, k_max + 1):
            parked = rng.random() < p_parked
            lanes[k] = {"speed": 0.0 if parked else float(rng.uniform(speed[0], speed[1])), "yaw": 0.0 if k % 2 == 0 else math.pi, "cars": []}
        rows, vels = [], []
        for c in range(n_cars):
            w, h = CAR_W + rng.uniform(-0.15, 0.15), CAR_H + rng.uniform(-0.4, 0.4)
            for _ in range(400):
                k = int(rng.integers(-k_agent, k_agent + 1)) if c < agents else int(rng.integers(-k_max, k_max + 1))
                x = float(rng.uniform(-agent_extent, agent_extent) if c < agents else rng.uniform(-extent, extent))
                lane = lanes[k]
                if all(abs(x - x2) > 0.5 * (w + w2) + 1.0 for x2, w2 in lane["cars"]):
                    lane["cars"].append((x, w))
                    break
            else:
                if c < agents:
                    raise RuntimeError("make_moving_world: no room for agent %d" % c)
                continue
            rows.append((x, k * LANE_PITCH, w, h, lane["yaw"], GROUND_Z, AGENT_TOP if c < agents else CAR_TOP))
            vels.append((lane["speed"] * (1.0 if lane["yaw"] == 0.0 else -1.0), 0.0))          # along the heading: (cos yaw, sin yaw) of yaw 0 or pi, exactly
        car_count[b] = len(rows)
        placed = []
        for _ in range(n_walls):
            w, h = rng.uniform(0.4, 0.6), rng.uniform(6.0, 14.0)
            for _ in range(400):
                k, x = int(rng.integers(-k_max, k_max)), float(rng.uniform(-extent, extent))
                if all(k != k2 or abs(x - x2) > 0.5 * (h + h2) + 0.5 for k2, x2, h2 in placed):
                    placed.append((k, x, h))
                    rows.append((x, (k + 0.5) * LANE_PITCH, w, h, math.pi / 2, GROUND_Z, WALL_TOP))
                    vels.append((0.0, 0.0))
                    break
        boxes[b, :len(rows)], box_vel[b, :len(rows)], box_count[b] = np.asarray(rows, np.float32), np.asarray(vels, np.float32), len(rows)
        P = []
        for a in range(agents):
            x, y, yaw = (float(v) for v in boxes[b, a, [0, 1, 4]])
            sensors[a * scenes + b], sensor_vel[a * scenes + b] = (x, y, 0.0, yaw), box_vel[b, a]
            P.append(synthetic_scene._pose(yaw, x, y))
        T, T_geo = synthetic_scene.warp_transforms(P)
        trans.append(T)
        trans_geo.append(T_geo)
    return {"sensors": sensors, "frame_of": np.tile(np.arange(scenes, dtype=np.int32), agents), "boxes": boxes, "box_count": box_count,
            "car_count": car_count, "trans": np.stack(trans), "trans_geo": np.stack(trans_geo), "num_agent": np.full((scenes, agents), agents, np.int64),
            "box_vel": box_vel, "sensor_vel": sensor_vel}


def sequence_tables(world, steps, dt=DT, t_ref=SWEEP_TIME / 2):
    """The host tables of a sequence: every sweep of every step of every world of `world` (make_moving_world's dict, or a hand-made one of its form).
    Agent-major, the models' batch order over the scenes * steps items: sweep m = a * (scenes * steps) + (w * steps + k) has frame_of[m] = w and
    time_of[m] = k * dt.  -> dict(sensors (n, 4), sensor_vel (n, 2), frame_of (n,), time_of (n,) f32, trans (scenes * steps, A, A, 4, 4) f32,
    num_agent (scenes * steps, A)).
    trans of item (w, k) are built HERE from the poses at k * dt + t_ref -- position = x0 + v * (k * dt + t_ref) in float64 from the fp32 tables,
    rounded to fp32 by warp_transforms -- while the device moves the same poses in its own fp64 arithmetic (relative, per ray): the two agree up to
    rounding, not to the bit."""
    W = world["boxes"].shape[0]
    A = world["sensors"].shape[0] // W
    B = W * steps
    sensors, sensor_vel = np.zeros((A * B, 4), np.float32), np.zeros((A * B, 2), np.float32)
    frame_of, time_of = np.zeros((A * B,), np.int32), np.zeros((A * B,), np.float32)
    trans = np.zeros((B, A, A, 4, 4), np.float32)
    for w in range(W):
        for k in range(steps):
            P = []
            for a in range(A):
                m, src = a * B + w * steps + k, a * W + w
                sensors[m], sensor_vel[m], frame_of[m], time_of[m] = world["sensors"][src], world["sensor_vel"][src], w, k * dt
                x, y, _, yaw = (float(v) for v in world["sensors"][src])
                vx, vy = (float(v) for v in world["sensor_vel"][src])
                T = k * dt + t_ref
                P.append(synthetic_scene._pose(yaw, x + vx * T, y + vy * T))
            trans[w * steps + k] = synthetic_scene.warp_transforms(P)[0]
    return {"sensors": sensors, "sensor_vel": sensor_vel, "frame_of": frame_of, "time_of": time_of, "trans": trans,
            "num_agent": np.full((B, A), A, np.int64)}


_AZ_TIMES = {}


def raycast_sequence_on_device(config, world, steps, dt=DT, sweep_time=SWEEP_TIME, device="cuda:0", grid=None, anchors=None, with_targets=True, gt="own",
                               min_hits=5, gt_lists=False, beams=32, az_steps=2048, max_pts=None, sigma_r=0.02, p_drop=0.0, r_min=1.0, r_max=70.0, seed=0,
                               step=0, elev_deg=None, vis_maps=False):
    """A sequence of `steps` sweeps, dt apart, of every agent of every world of `world` (make_moving_world), all scenes * steps batch items at once:
    ONE ops.lidar_cast_moving call and ONE ops.visible_boxes_moving call (ground truth at half the sweep duration), then raycast_batch_on_device's
    chain -- voxelise, densify, assign -- with nothing synchronised.  A sweep takes sweep_time; a moving car is met where it is when the beam passes.
    -> the data dict FaFModule.step / predict_all read (bev_seq, trans_matrices, num_agent and, with_targets, the IoU targets), plus gt_ids
    (A * scenes * steps, cap) int32 on the device: the box index of each ground-truth row, the car's identity within its world (-1 past the count),
    and gt_boxes_dev / gt_count, the padded rows themselves.  gt_lists: also gt_boxes[agent][item] and gt_id_lists[agent][item], host arrays (the one
    read-back), item = w * steps + k.  elev_deg: (lo, hi) elevations of the ring instead of ops.ring_table's.  vis_maps: also data["vis_maps"]
    (A * scenes * steps, X, Y, Z) fp32 as raycast_batch_on_device gives it -- every ray of a raw moving sweep starts at the origin of its own sensor
    frame, which is what the rule assumes (no de-skewing); without it keys and bytes are what they were."""
    import torch
    from .. import ops
    from ..train import loop
    from . import postprocess
    if gt not in ("own", "any"):
        raise ValueError("gt must be 'own' or 'any'")
    device = torch.device(device)
    grid = grid or ops.VoxelGrid(config.voxel_size, config.area_extents)
    t_ref = sweep_time / 2
    seq = sequence_tables(world, steps, dt, t_ref)
    W, cap = world["boxes"].shape[:2]
    A = world["sensors"].shape[0] // W
    B = W * steps
    rows = ops.box_rows(world["boxes"][..., :5].reshape(-1, 5), world["boxes"][..., 5].reshape(-1), world["boxes"][..., 6].reshape(-1)).reshape(W, cap, 9)
    host = {"sensors": ops.sensor_rows(seq["sensors"]), "sensor_vel": seq["sensor_vel"], "frame_of": seq["frame_of"], "time_of": seq["time_of"],
            "boxes": rows, "box_vel": world["box_vel"], "box_count": world["box_count"], "car_count": world["car_count"]}
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in host.items()}
    beam, az = _ring_on(device, beams, az_steps, elev_deg)
    key = (str(device), az_steps, float(sweep_time))
    if key not in _AZ_TIMES:
        _AZ_TIMES[key] = torch.from_numpy(ops.az_time_table(az_steps, sweep_time)).to(device)
    cast = ops.lidar_cast_moving(d["sensors"], d["sensor_vel"], d["time_of"], d["frame_of"], d["boxes"], d["box_vel"], d["box_count"], beam, az,
                                 _AZ_TIMES[key], max_pts or beams * az_steps, ground_z=GROUND_Z, r_min=r_min, r_max=r_max, sigma_r=sigma_r, p_drop=p_drop,
                                 seed=seed, step=step, want=("box_hits",))
    x_lim = min(abs(float(config.area_extents[0][0])), abs(float(config.area_extents[0][1]))) - 3.0
    y_lim = min(abs(float(config.area_extents[1][0])), abs(float(config.area_extents[1][1]))) - 3.0
    vis = ops.visible_boxes_moving(cast["box_hits"], d["sensors"], d["sensor_vel"], d["time_of"], d["frame_of"], d["boxes"], d["box_vel"], d["car_count"],
                                   t_ref=t_ref, min_hits=min_hits, any_agent=gt == "any", x_lim=x_lim, y_lim=y_lim, want=())
    bits = ops.voxelize_bits(cast["points"], cast["n_pts"], grid)
    data = {"bev_seq": ops.bits_to_dense(bits, grid.dims[2])[:, None], "trans_matrices": torch.from_numpy(seq["trans"]).to(device),
            "num_agent": torch.from_numpy(seq["num_agent"]), "gt_ids": vis["gt_ids"], "gt_boxes_dev": vis["gt_boxes"], "gt_count": vis["gt_count"]}
    if vis_maps:
        data["vis_maps"] = ops.vis_maps(bits, ops.freespace_bits(cast["points"], cast["n_pts"], grid), grid.dims[2])
    if gt_lists:
        hb, hc, hi = vis["gt_boxes"].cpu().numpy(), vis["gt_count"].cpu().numpy(), vis["gt_ids"].cpu().numpy()
        data["gt_boxes"] = [[hb[a * B + j, :hc[a * B + j]].copy() for j in range(B)] for a in range(A)]
        data["gt_id_lists"] = [[hi[a * B + j, :hc[a * B + j]].copy() for j in range(B)] for a in range(A)]
    if with_targets:
        anchors = postprocess.build_anchor_map(config) if anchors is None else anchors
        data["labels"], data["reg_targets"], data["reg_loss_mask"] = loop.iou_targets_from_device(vis["gt_boxes"], vis["gt_count"], anchors, device)
    return data

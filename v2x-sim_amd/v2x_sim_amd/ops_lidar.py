"""Rows f-2 / f-3 (synthetic scenes with occlusion): the python wrappers over v2x_lidar_cast and v2x_lidar_visible_boxes -- the sweeps of all agents
of all frames of a step ray-cast against a scene of boxes on the device, and the ground truth the per-box return counts imply -- and the host tables
they read (beam / azimuth cos-sin pairs, sensor rows, box rows); and their moving twins over v2x_lidar_cast_moving and v2x_lidar_visible_boxes_moving
(constant velocities, sweeps that take time, ground truth with identities).  The rule: DESIGN.md section 3.12.  Re-exported by ops.py (`ops.lidar_cast` ...)."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._launch import _dev, _dev_opt, _stream

LIDAR_MAX_BOXES = 256


def ring_table(beams=32, steps=2048, elev_deg=(-30.67, 10.67), az_offset=0.0):
    """The angles of utils/synthetic.synthetic_ring_sweep as the cos / sin pairs the cast reads: -> (beam (beams, 2), az (steps, 2)) fp32 host arrays.
    `beams` elevations from elev_deg[0] to elev_deg[1] degrees, `steps` azimuths (k + az_offset) * 2 pi / steps.  Ray r = b * steps + a."""
    elev = np.deg2rad(np.linspace(elev_deg[0], elev_deg[1], int(beams)))
    az = (np.arange(int(steps), dtype=np.float64) + float(az_offset)) * (2.0 * math.pi / int(steps))
    return (np.stack([np.cos(elev), np.sin(elev)], 1).astype(np.float32), np.stack([np.cos(az), np.sin(az)], 1).astype(np.float32))


def sensor_rows(xyz_yaw):
    """(n, 4) x, y, z, yaw -> (n, 6) fp32 x, y, z, yaw, cos yaw, sin yaw: the trigonometry is the host's, in float64 from the fp32 yaw."""
    p = np.asarray(xyz_yaw, np.float32).reshape(-1, 4)
    yaw = p[:, 3].astype(np.float64)
    return np.concatenate([p, np.cos(yaw)[:, None].astype(np.float32), np.sin(yaw)[:, None].astype(np.float32)], 1)


def box_rows(boxes, z0, z1):
    """(k, 5) x, y, w, h, yaw with the scalars or (k,) arrays z0, z1 -> (k, 9) fp32 cx, cy, w, h, yaw, cos yaw, sin yaw, z0, z1."""
    b = np.asarray(boxes, np.float32).reshape(-1, 5)
    yaw = b[:, 4].astype(np.float64)
    z = np.stack([np.broadcast_to(np.asarray(z0, np.float32), (b.shape[0],)), np.broadcast_to(np.asarray(z1, np.float32), (b.shape[0],))], 1)
    return np.concatenate([b, np.cos(yaw)[:, None].astype(np.float32), np.sin(yaw)[:, None].astype(np.float32), z], 1)


def _out(res, name, dtype, shape, dev, what):
    t = res.get(name)
    if t is None:
        t = res[name] = torch.empty(shape, dtype=dtype, device=dev)
    elif tuple(t.shape) != tuple(shape) or t.dtype != dtype:
        raise ValueError("%s: out[%r] is %s %s, needs %s %s" % (what, name, t.dtype, tuple(t.shape), dtype, tuple(shape)))
    return t


def _scene_shapes(what, sensors, frame_of, boxes, box_count):
    if sensors.dim() != 2 or sensors.shape[1] != 6 or frame_of.numel() != sensors.shape[0] or boxes.dim() != 3 or boxes.shape[2] != 9 or \
            box_count.numel() != boxes.shape[0] or boxes.shape[0] < 1:
        raise ValueError("%s: sensors %s, frame_of %s, boxes %s, box_count %s" % (what, tuple(sensors.shape), tuple(frame_of.shape), tuple(boxes.shape),
                                                                                 tuple(box_count.shape)))
    return int(sensors.shape[0]), int(boxes.shape[0]), int(boxes.shape[1])


def lidar_cast(sensors, frame_of, boxes, box_count, beam, az, max_pts, ground_z=-1.8, r_min=1.0, r_max=70.0, sigma_r=0.0, p_drop=0.0, seed=0, step=0,
               want=("hit", "box_hits"), out=None):
    """All sweeps of a step against their frames' boxes (v2x_lidar_cast; the rule: DESIGN.md section 3.12 "LiDAR ray cast").
    sensors (n, 6) fp32 (sensor_rows), frame_of (n,) int32, boxes (F, cap, 9) fp32 (box_rows), box_count (F,) int32, beam (NB, 2) and az (NA, 2) fp32
    (ring_table), all on the device ->
    dict: points (n, max_pts, 4) fp32 in the sensor frame, n_pts (n,) int32 (what ops.voxelize_bits reads) and the optional outputs named in `want`:
    hit (n, max_pts) int32 = 1 + box index, 0 ground, -1 past n_pts; box_hits (n, cap) int32 = kept returns per box.  out: a dict of existing tensors
    to write into (an optional output present in `out` is written too).  Every element of every output is written."""
    lib = _lib.load()
    n, F, cap = _scene_shapes("lidar_cast", sensors, frame_of, boxes, box_count)
    if beam.dim() != 2 or beam.shape[1] != 2 or az.dim() != 2 or az.shape[1] != 2:
        raise ValueError("lidar_cast: beam %s, az %s: (N, 2) cos / sin pairs needed" % (tuple(beam.shape), tuple(az.shape)))
    unknown = (set(want) - {"hit", "box_hits"}) | (set(out or ()) - {"points", "n_pts", "hit", "box_hits"})
    if unknown:
        raise ValueError("lidar_cast: unknown output %s" % sorted(unknown))
    seed, step, max_pts = int(seed), int(step), int(max_pts)
    if not (0 <= seed < 1 << 64 and 0 <= step < 1 << 64):
        raise ValueError("lidar_cast: seed and step must lie in [0, 2^64)")
    dev = sensors.device
    res = dict(out) if out is not None else {}
    shapes = {"points": (torch.float32, (n, max_pts, 4)), "n_pts": (torch.int32, (n,)), "hit": (torch.int32, (n, max_pts)), "box_hits": (torch.int32, (n, cap))}
    ptr = {}
    for name, (dtype, shape) in shapes.items():
        if name in ("hit", "box_hits") and name not in want and name not in res:
            ptr[name] = None
            continue
        t = _out(res, name, dtype, shape, dev, "lidar_cast")
        ptr[name] = _dev(t, dtype, name) if n else None
    nbytes = lib.v2x_lidar_cast_workspace_size(n, int(beam.shape[0]), int(az.shape[0]), cap)
    if nbytes < 0:
        raise ValueError("lidar_cast: sizes out of range (n=%d, beams=%d, azimuths=%d, cap=%d in [1, 256])" % (n, beam.shape[0], az.shape[0], cap))
    ws = torch.empty(((max(nbytes, 8) + 7) // 8,), dtype=torch.int64, device=dev)     # rounded UP: the size is a multiple of 4, not of 8 (an odd n * chunks)
    _lib.check(lib.v2x_lidar_cast(_dev(sensors, torch.float32, "sensors") if n else None, _dev(frame_of, torch.int32, "frame_of") if n else None, n,
                                  _dev(boxes, torch.float32, "boxes"), _dev(box_count, torch.int32, "box_count"), F, cap, _dev(beam, torch.float32, "beam"),
                                  int(beam.shape[0]), _dev(az, torch.float32, "az"), int(az.shape[0]), C.c_float(ground_z), C.c_float(r_min), C.c_float(r_max),
                                  C.c_float(sigma_r), C.c_float(p_drop), C.c_uint64(seed), C.c_uint64(step), ptr["points"], ptr["n_pts"], max_pts, ptr["hit"],
                                  ptr["box_hits"], _dev(ws, torch.int64, "workspace"), nbytes, _stream()), "v2x_lidar_cast")
    return res


def visible_boxes(box_hits, sensors, frame_of, boxes, box_count, min_hits=5, any_agent=False, x_lim=29.0, y_lim=29.0, out=None):
    """Each sweep's ground truth from the cast's per-box return counts (v2x_lidar_visible_boxes): the boxes with at least
    `min_hits` kept returns in this sweep (any_agent: in any sweep of the same frame), centre within |x| < x_lim, |y| < y_lim of the sensor frame, not
    containing the sensor ->  (gt_boxes (n, cap, 5) fp32 rows (x, y, w, h, yaw) in the sensor frame, zero past the count; gt_count (n,) int32): the
    padded device form ops.assign_targets reads.  out: (gt_boxes, gt_count) to write into."""
    lib = _lib.load()
    n, F, cap = _scene_shapes("visible_boxes", sensors, frame_of, boxes, box_count)
    if tuple(box_hits.shape) != (n, cap):
        raise ValueError("visible_boxes: box_hits %s, needs %s" % (tuple(box_hits.shape), (n, cap)))
    res = {} if out is None else {"gt_boxes": out[0], "gt_count": out[1]}
    gt = _out(res, "gt_boxes", torch.float32, (n, cap, 5), sensors.device, "visible_boxes")
    cnt = _out(res, "gt_count", torch.int32, (n,), sensors.device, "visible_boxes")
    _lib.check(lib.v2x_lidar_visible_boxes(_dev(box_hits, torch.int32, "box_hits") if n else None, _dev(sensors, torch.float32, "sensors") if n else None,
                                           _dev(frame_of, torch.int32, "frame_of") if n else None, n, _dev(boxes, torch.float32, "boxes"),
                                           _dev(box_count, torch.int32, "box_count"), F, cap, int(min_hits), int(bool(any_agent)), C.c_float(x_lim),
                                           C.c_float(y_lim), _dev_opt(gt if n else None, torch.float32, "gt_boxes"),
                                           _dev_opt(cnt if n else None, torch.int32, "gt_count"), _stream()), "v2x_lidar_visible_boxes")
    return gt, cnt


# ---- moving scenes (DESIGN.md section 3.12 "moving scenes") ---------------------------------------------------------------------------------------
def az_time_table(steps=2048, sweep_time=0.1):
    """The time offset of each azimuth step within a sweep: a * sweep_time / steps, computed in float64 and rounded once -> (steps,) fp32 host array."""
    return (np.arange(int(steps), dtype=np.float64) * float(sweep_time) / int(steps)).astype(np.float32)


def _motion_shapes(what, n, F, cap, sensor_vel, time_of, box_vel):
    if tuple(sensor_vel.shape) != (n, 2) or time_of.numel() != n or tuple(box_vel.shape) != (F, cap, 2):
        raise ValueError("%s: sensor_vel %s, time_of %s, box_vel %s: needs (%d, 2), (%d,), (%d, %d, 2)" % (
            what, tuple(sensor_vel.shape), tuple(time_of.shape), tuple(box_vel.shape), n, n, F, cap))


def lidar_cast_moving(sensors, sensor_vel, time_of, frame_of, boxes, box_vel, box_count, beam, az, az_time, max_pts, ground_z=-1.8, r_min=1.0, r_max=70.0,
                      sigma_r=0.0, p_drop=0.0, seed=0, step=0, want=("hit", "box_hits"), out=None):
    """lidar_cast with time (v2x_lidar_cast_moving; the rule: DESIGN.md section 3.12 "moving scenes"): every box and sensor moves at constant velocity
    from its pose at time 0, and ray r = b * NA + a of sweep s is cast at time_of[s] + az_time[a].  Beyond lidar_cast's arguments: sensor_vel (n, 2)
    fp32, time_of (n,) fp32, box_vel (F, cap, 2) fp32, az_time (NA,) fp32 (az_time_table), on the device.  Many sweeps at different times may share
    one world (frame_of).  -> lidar_cast's dict; with zero velocities or zero times, its bytes."""
    lib = _lib.load()
    n, F, cap = _scene_shapes("lidar_cast_moving", sensors, frame_of, boxes, box_count)
    _motion_shapes("lidar_cast_moving", n, F, cap, sensor_vel, time_of, box_vel)
    if beam.dim() != 2 or beam.shape[1] != 2 or az.dim() != 2 or az.shape[1] != 2 or az_time.dim() != 1 or az_time.shape[0] != az.shape[0]:
        raise ValueError("lidar_cast_moving: beam %s, az %s, az_time %s: (N, 2) cos / sin pairs and one time per azimuth needed" % (
            tuple(beam.shape), tuple(az.shape), tuple(az_time.shape)))
    unknown = (set(want) - {"hit", "box_hits"}) | (set(out or ()) - {"points", "n_pts", "hit", "box_hits"})
    if unknown:
        raise ValueError("lidar_cast_moving: unknown output %s" % sorted(unknown))
    seed, step, max_pts = int(seed), int(step), int(max_pts)
    if not (0 <= seed < 1 << 64 and 0 <= step < 1 << 64):
        raise ValueError("lidar_cast_moving: seed and step must lie in [0, 2^64)")
    dev = sensors.device
    res = dict(out) if out is not None else {}
    shapes = {"points": (torch.float32, (n, max_pts, 4)), "n_pts": (torch.int32, (n,)), "hit": (torch.int32, (n, max_pts)), "box_hits": (torch.int32, (n, cap))}
    ptr = {}
    for name, (dtype, shape) in shapes.items():
        if name in ("hit", "box_hits") and name not in want and name not in res:
            ptr[name] = None
            continue
        t = _out(res, name, dtype, shape, dev, "lidar_cast_moving")
        ptr[name] = _dev(t, dtype, name) if n else None
    nbytes = lib.v2x_lidar_cast_workspace_size(n, int(beam.shape[0]), int(az.shape[0]), cap)
    if nbytes < 0:
        raise ValueError("lidar_cast_moving: sizes out of range (n=%d, beams=%d, azimuths=%d, cap=%d in [1, 256])" % (n, beam.shape[0], az.shape[0], cap))
    ws = torch.empty(((max(nbytes, 8) + 7) // 8,), dtype=torch.int64, device=dev)     # rounded UP: the size is a multiple of 4, not of 8 (an odd n * chunks)
    _lib.check(lib.v2x_lidar_cast_moving(
        _dev(sensors, torch.float32, "sensors") if n else None, _dev(sensor_vel, torch.float32, "sensor_vel") if n else None,
        _dev(time_of, torch.float32, "time_of") if n else None, _dev(frame_of, torch.int32, "frame_of") if n else None, n,
        _dev(boxes, torch.float32, "boxes"), _dev(box_vel, torch.float32, "box_vel"), _dev(box_count, torch.int32, "box_count"), F, cap,
        _dev(beam, torch.float32, "beam"), int(beam.shape[0]), _dev(az, torch.float32, "az"), _dev(az_time, torch.float32, "az_time"), int(az.shape[0]),
        C.c_float(ground_z), C.c_float(r_min), C.c_float(r_max), C.c_float(sigma_r), C.c_float(p_drop), C.c_uint64(seed), C.c_uint64(step), ptr["points"],
        ptr["n_pts"], max_pts, ptr["hit"], ptr["box_hits"], _dev(ws, torch.int64, "workspace"), nbytes, _stream()), "v2x_lidar_cast_moving")
    return res


def visible_boxes_moving(box_hits, sensors, sensor_vel, time_of, frame_of, boxes, box_vel, box_count, t_ref=0.05, min_hits=5, any_agent=False, x_lim=29.0,
                         y_lim=29.0, want=("gt_vel",), out=None):
    """Each sweep's ground truth at time_of + t_ref (v2x_lidar_visible_boxes_moving; DESIGN.md section 3.12 "moving scenes"): visible_boxes' three
    conditions with the poses at that time; any_agent reads the sweeps of the same world that start at the same time.  -> dict: gt_boxes (n, cap, 5)
    fp32, gt_count (n,) int32, gt_ids (n, cap) int32 = the box index of each row (-1 past the count) and, if "gt_vel" is in `want` or in `out`, gt_vel
    (n, cap, 2) fp32 = the box's velocity relative to the sensor, in the sensor frame.  out: a dict of existing tensors to write into."""
    lib = _lib.load()
    n, F, cap = _scene_shapes("visible_boxes_moving", sensors, frame_of, boxes, box_count)
    _motion_shapes("visible_boxes_moving", n, F, cap, sensor_vel, time_of, box_vel)
    if tuple(box_hits.shape) != (n, cap):
        raise ValueError("visible_boxes_moving: box_hits %s, needs %s" % (tuple(box_hits.shape), (n, cap)))
    unknown = (set(want) - {"gt_vel"}) | (set(out or ()) - {"gt_boxes", "gt_count", "gt_ids", "gt_vel"})
    if unknown:
        raise ValueError("visible_boxes_moving: unknown output %s" % sorted(unknown))
    res = dict(out) if out is not None else {}
    dev = sensors.device
    gt = _out(res, "gt_boxes", torch.float32, (n, cap, 5), dev, "visible_boxes_moving")
    cnt = _out(res, "gt_count", torch.int32, (n,), dev, "visible_boxes_moving")
    ids = _out(res, "gt_ids", torch.int32, (n, cap), dev, "visible_boxes_moving")
    vel = _out(res, "gt_vel", torch.float32, (n, cap, 2), dev, "visible_boxes_moving") if ("gt_vel" in want or "gt_vel" in res) else None
    _lib.check(lib.v2x_lidar_visible_boxes_moving(
        _dev(box_hits, torch.int32, "box_hits") if n else None, _dev(sensors, torch.float32, "sensors") if n else None,
        _dev(sensor_vel, torch.float32, "sensor_vel") if n else None, _dev(time_of, torch.float32, "time_of") if n else None, C.c_float(t_ref),
        _dev(frame_of, torch.int32, "frame_of") if n else None, n, _dev(boxes, torch.float32, "boxes"), _dev(box_vel, torch.float32, "box_vel"),
        _dev(box_count, torch.int32, "box_count"), F, cap, int(min_hits), int(bool(any_agent)), C.c_float(x_lim), C.c_float(y_lim),
        _dev_opt(gt if n else None, torch.float32, "gt_boxes"), _dev_opt(cnt if n else None, torch.int32, "gt_count"),
        _dev_opt(ids if n else None, torch.int32, "gt_ids"), _dev_opt(vel if n else None, torch.float32, "gt_vel"), _stream()),
        "v2x_lidar_visible_boxes_moving")
    return res

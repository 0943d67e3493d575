"""Float64 reference, a second exact statement and the case table of the LiDAR ray cast (csrc/lidar_cast.hip).

`cast_ref` states the frozen rule in numpy float64: the operations in the rule's order, each product and sum rounded on its own (numpy fuses
nothing), one array over the rays of a sweep, a python loop over the boxes.  No chunks, no LDS table, no compaction by ballots.  At sigma_r = 0 the
device must return its bytes: points, n_pts, hit, box_hits; `visible_ref` states the ground-truth rule the same way.  At sigma_r > 0 the point
coordinates are given in float64 (`points64`: the same draw, the normal from math.log / math.cos).

`exact_sweep` is the second, independent statement: the ray is clipped against the six half-spaces of each box, evaluated with fractions.Fraction
on the fp32 inputs -- no rounding anywhere, no slabs, no min / max of quotient pairs.  tests/test_lidar_refs_cpu.py holds the two against each other.
"""
import functools
import math
from fractions import Fraction

import numpy as np

import channel_refs as CR

LIDAR_DOMAIN = 0x4C440000
MAX_BOXES = 256


# ---- the draw --------------------------------------------------------------------------------------------------------------------------------
def words(seed, step, sweep, ray):
    assert 0 <= seed < 1 << 64 and 0 <= step < 1 << 64
    return CR.philox4x32_10((ray, sweep, step & CR.M32, LIDAR_DOMAIN | ((step >> 32) & 0xffff)), (seed & CR.M32, seed >> 32))


def uniform24(w):
    return (w >> 8) / float(1 << 24)             # exact: 24 bits, [0, 1)


def uniform23(w):
    return ((w >> 9) + 0.5) / float(1 << 23)     # exact: 24 bits, (0, 1)


def dropped(w, p_drop):
    return uniform24(w[0]) < float(np.float32(p_drop))


def normal64(w):
    return math.sqrt(-2.0 * math.log(uniform23(w[1]))) * math.cos(2.0 * math.pi * uniform23(w[2]))


# ---- the float64 statement of the rule -------------------------------------------------------------------------------------------------------
def box_valid(b):
    return bool(np.isfinite(b).all() and b[2] >= 0 and b[3] >= 0 and b[8] >= b[7])


def clamp_count(box_count, f, cap):
    if not 0 <= f < len(box_count):
        return 0
    return min(max(int(box_count[f]), 0), cap)


def directions(beam, az):
    """-> dx, dy, dz float64 (NB * NA,), ray r = b * NA + a."""
    ce, se = beam[:, 0].astype(np.float64)[:, None], beam[:, 1].astype(np.float64)[:, None]
    ca, sa = az[:, 0].astype(np.float64)[None, :], az[:, 1].astype(np.float64)[None, :]
    return (ce * ca).reshape(-1), (ce * sa).reshape(-1), np.broadcast_to(se, (beam.shape[0], az.shape[0])).reshape(-1).copy()


def _slab(l, u, lo, hi, t_near, t_far, miss):
    zero = u == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (lo - l) / u, (hi - l) / u
    miss = miss | (zero & ((l < lo) | (l > hi)))
    t_near = np.where(zero, t_near, np.maximum(t_near, np.minimum(ta, tb)))
    t_far = np.where(zero, t_far, np.minimum(t_far, np.maximum(ta, tb)))
    return t_near, t_far, miss


def sweep_ref(sen, boxes, count, beam, az, ground_z):
    """One sweep: -> (t (R,) float64, inf without a candidate; id (R,) int: 1 + g, 0 ground, -1 nothing)."""
    dx, dy, dz = directions(beam, az)
    ox, oy, oz, c, s = (np.float64(sen[k]) for k in (0, 1, 2, 4, 5))
    wx, wy = c * dx - s * dy, s * dx + c * dy
    best = np.full(dx.shape, np.inf)
    idx = np.full(dx.shape, -1, np.int64)
    for g in range(count):
        b = boxes[g].astype(np.float64)
        if not box_valid(b):
            continue
        px, py, cg, sg = ox - b[0], oy - b[1], b[5], b[6]
        lx, ly = px * cg + py * sg, -px * sg + py * cg
        ux, uy = wx * cg + wy * sg, -wx * sg + wy * cg
        tn, tf, miss = np.full(dx.shape, -np.inf), np.full(dx.shape, np.inf), np.zeros(dx.shape, bool)
        hw, hh = b[2] / 2, b[3] / 2
        for l, u, lo, hi in ((lx, ux, -hw, hw), (ly, uy, -hh, hh), (oz, dz, b[7], b[8])):
            tn, tf, miss = _slab(np.broadcast_to(l, dx.shape), u, lo, hi, tn, tf, miss)
        take = ~miss & (tn <= tf) & (tn > 0) & (tn < best)
        best, idx = np.where(take, tn, best), np.where(take, 1 + g, idx)
    with np.errstate(divide="ignore", invalid="ignore"):
        tg = (np.float64(np.float32(ground_z)) - oz) / dz
    take = (dz < 0) & (tg > 0) & (tg < best)
    return np.where(take, tg, best), np.where(take, 0, idx)


def cast_ref(sc, max_pts=None):
    """The whole call.  -> dict(points (n, max_pts, 4) fp32 -- exact at sigma_r = 0, the fp32 rounding of points64 otherwise --, points64 float64,
    n_pts, hit (n, max_pts), box_hits (n, cap) int32, returns (n,) = the returns before the cut at max_pts, ray_t / ray_id (n, R): every ray's
    winner)."""
    n, cap = sc["sensors"].shape[0], sc["boxes"].shape[1]
    max_pts = sc["max_pts"] if max_pts is None else max_pts
    dx, dy, dz = directions(sc["beam"], sc["az"])
    sigma = float(np.float32(sc["sigma_r"]))
    out = {"points": np.zeros((n, max_pts, 4), np.float32), "points64": np.zeros((n, max_pts, 4)), "n_pts": np.zeros((n,), np.int32),
           "hit": np.full((n, max_pts), -1, np.int32), "box_hits": np.zeros((n, cap), np.int32), "returns": np.zeros((n,), np.int64),
           "ray_t": np.zeros((n, dx.shape[0])), "ray_id": np.zeros((n, dx.shape[0]), np.int64)}
    r_min, r_max = np.float64(np.float32(sc["r_min"])), np.float64(np.float32(sc["r_max"]))
    for s in range(n):
        f = int(sc["frame_of"][s])
        count = clamp_count(sc["box_count"], f, cap)
        t, idx = sweep_ref(sc["sensors"][s], sc["boxes"][f] if count else None, count, sc["beam"], sc["az"], sc["ground_z"])
        out["ray_t"][s], out["ray_id"][s] = t, idx
        k = 0
        for r in np.nonzero((idx >= 0) & (t >= r_min) & (t <= r_max))[0]:
            w = words(sc["seed"], sc["step"], s, int(r))
            if dropped(w, sc["p_drop"]):
                continue
            out["returns"][s] += 1
            if k >= max_pts:
                continue
            t32 = np.float32(t[r])
            tp = np.float64(t32) + (sigma * normal64(w) if sigma else 0.0)
            if not sigma:
                tp = np.float64(np.float32(tp))
            row = np.array([tp * dx[r], tp * dy[r], tp * dz[r], uniform24(w[3])])
            out["points64"][s, k], out["points"][s, k], out["hit"][s, k] = row, row.astype(np.float32), idx[r]
            if idx[r] >= 1:
                out["box_hits"][s, idx[r] - 1] += 1
            k += 1
        out["n_pts"][s] = k
    return out


def visible_ref(sc, box_hits, any_agent, min_hits=None):
    """-> (gt_boxes (n, cap, 5) fp32, gt_count (n,) int32)."""
    n, cap = sc["sensors"].shape[0], sc["boxes"].shape[1]
    min_hits = sc["min_hits"] if min_hits is None else min_hits
    gt, cnt = np.zeros((n, cap, 5), np.float32), np.zeros((n,), np.int32)
    for s in range(n):
        sen, f = sc["sensors"][s], int(sc["frame_of"][s])
        ox, oy, oz, c, sn = (np.float64(sen[k]) for k in (0, 1, 2, 4, 5))
        for g in range(clamp_count(sc["box_count"], f, cap)):
            b32 = sc["boxes"][f, g]
            b = b32.astype(np.float64)
            hits = int(box_hits[s, g])
            if any_agent:
                hits = max(int(box_hits[q, g]) for q in range(n) if int(sc["frame_of"][q]) == f)
            if not box_valid(b) or hits < min_hits:
                continue
            ex, ey = b[0] - ox, b[1] - oy
            x, y = ex * c + ey * sn, -ex * sn + ey * c
            px, py = ox - b[0], oy - b[1]
            lx, ly = px * b[5] + py * b[6], -px * b[6] + py * b[5]
            inside = abs(lx) <= b[2] / 2 and abs(ly) <= b[3] / 2 and b[7] <= oz <= b[8]
            if abs(x) < np.float64(np.float32(sc["x_lim"])) and abs(y) < np.float64(np.float32(sc["y_lim"])) and not inside:
                gt[s, cnt[s]] = (np.float32(x), np.float32(y), b32[2], b32[3], np.float32(b32[4]) - np.float32(sen[3]))
                cnt[s] += 1
    return gt, cnt


# ---- the exact statement: half-space clipping in rationals -----------------------------------------------------------------------------------
def _fr(v):
    return Fraction(float(v))


def exact_sweep(sen, boxes, count, beam, az, ground_z):
    """Per ray the candidates [(t, id)] sorted by (t, boxes in index order before the ground), every t an exact Fraction, and `shaky`: True when some
    decision of the ray is within SHAKY of flipping (a grazing hit, t_near at 0) -- a float64 evaluation may then differ legitimately."""
    ox, oy, oz, c, s = (_fr(sen[k]) for k in (0, 1, 2, 4, 5))
    gz = _fr(np.float32(ground_z))
    live = []
    for g in range(count):
        if not box_valid(boxes[g].astype(np.float64)):
            continue
        b = [_fr(v) for v in boxes[g]]
        px, py, cg, sg = ox - b[0], oy - b[1], b[5], b[6]
        live.append((g, px * cg + py * sg, -px * sg + py * cg, cg, sg, b[2] / 2, b[3] / 2, b[7], b[8]))
    rays = []
    for bi in range(beam.shape[0]):
        ce, se = _fr(beam[bi, 0]), _fr(beam[bi, 1])
        for ai in range(az.shape[0]):
            ca, sa = _fr(az[ai, 0]), _fr(az[ai, 1])
            dx, dy, dz = ce * ca, ce * sa, se
            wx, wy = c * dx - s * dy, s * dx + c * dy
            cand, shaky = [], False
            for g, lx, ly, cg, sg, hw, hh, z0, z1 in live:
                ux, uy = wx * cg + wy * sg, -wx * sg + wy * cg
                lo, hi, empty = None, None, False
                # the six half-spaces  n . (l + t u) <= e:  (+x, hw), (-x, hw), (+y, hh), (-y, hh), (+z, z1), (-z, -z0)
                for a, e in ((ux, hw - lx), (-ux, hw + lx), (uy, hh - ly), (-uy, hh + ly), (dz, z1 - oz), (-dz, oz - z0)):
                    if a == 0:
                        if e < 0:
                            empty = True
                            break
                    elif a > 0:
                        hi = e / a if hi is None else min(hi, e / a)
                    else:
                        lo = e / a if lo is None else max(lo, e / a)
                    if lo is not None and hi is not None and lo > hi + 1:
                        empty = True                      # far from grazing: stop early
                        break
                if empty or lo is None or hi is None:
                    continue
                scale = max(1, abs(lo))
                if abs(hi - lo) <= SHAKY * scale or abs(lo) <= SHAKY:
                    shaky = True
                if lo <= hi and lo > 0:
                    cand.append((lo, 0, g, 1 + g))
            if dz < 0:
                t = (gz - oz) / dz
                if t > 0:
                    cand.append((t, 1, 0, 0))
            cand.sort()
            rays.append(([(t, i) for t, _, _, i in cand], shaky))
    return rays


SHAKY = Fraction(1, 10 ** 9)


# ---- tables ----------------------------------------------------------------------------------------------------------------------------------
def ring(nb, na, elev_deg, az_offset=0.0):
    elev = np.deg2rad(np.linspace(elev_deg[0], elev_deg[1], nb))
    az = (np.arange(na) + az_offset) * (2.0 * math.pi / na)
    return np.stack([np.cos(elev), np.sin(elev)], 1).astype(np.float32), np.stack([np.cos(az), np.sin(az)], 1).astype(np.float32)


def sensor_rows(rows):
    p = np.asarray(rows, np.float32).reshape(-1, 4)
    yaw = p[:, 3].astype(np.float64)
    return np.concatenate([p, np.cos(yaw)[:, None].astype(np.float32), np.sin(yaw)[:, None].astype(np.float32)], 1)


def box_rows(rows):
    """rows of (cx, cy, w, h, yaw, z0, z1) -> (k, 9)."""
    b = np.asarray(rows, np.float32).reshape(-1, 7)
    yaw = b[:, 4].astype(np.float64)
    with np.errstate(invalid="ignore"):                        # a dropped box may carry an infinite yaw
        return np.concatenate([b[:, :5], np.cos(yaw)[:, None].astype(np.float32), np.sin(yaw)[:, None].astype(np.float32), b[:, 5:7]], 1)


def _ring_boxes(rng, k, r_lo=5.0, r_hi=28.0, top=(-0.4, 2.0)):
    """k car- and wall-sized boxes scattered around the origin, none closer than r_lo to it."""
    rad, ang = rng.uniform(r_lo, r_hi, k), rng.uniform(-math.pi, math.pi, k)
    return np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(1.5, 6.0, k), rng.uniform(1.5, 5.0, k), rng.uniform(-math.pi, math.pi, k),
                     np.full(k, -1.8), rng.uniform(top[0], top[1], k)], 1)


def _scene(sensors, frames, beam, az, frame_of=None, cap=None, counts=None, **kw):
    """frames: one list of 7-tuples per frame.  cap: the table's width (default: the longest list, at least 1).  counts: box_count override."""
    cap = cap or max([1] + [len(f) for f in frames])
    boxes = np.zeros((len(frames), cap, 9), np.float32)
    boxes[:, :, 2:4] = 500.0                                   # a padding row that was read would swallow every ray: a 500 m box around the origin ...
    boxes[:, :, 5], boxes[:, :, 7], boxes[:, :, 8] = 1.0, -100.0, 100.0
    boxes[:, :, 0] = 300.0                                     # ... whose near face lies 50 m out (the sensors sit within a few metres of the origin)
    for f, rows in enumerate(frames):
        if len(rows):
            boxes[f, :len(rows)] = box_rows(rows)
    sen = sensor_rows(sensors)
    sc = dict(sensors=sen, frame_of=np.asarray(frame_of if frame_of is not None else [0] * sen.shape[0], np.int32), boxes=boxes,
              box_count=np.asarray(counts if counts is not None else [len(f) for f in frames], np.int32), beam=beam, az=az, ground_z=-1.8, r_min=1.0,
              r_max=70.0, sigma_r=0.0, p_drop=0.0, seed=7, step=0, max_pts="above", min_hits=5, x_lim=29.0, y_lim=29.0)
    sc.update(kw)
    return sc


def _c_no_boxes():
    return _scene([[0, 0, 0, 0.3]], [[]], *ring(4, 64, (-25, -2)))


def _c_one_box():
    return _scene([[1.0, -2.0, 0.0, -0.7]], [[(9.0, 1.5, 4.4, 2.0, 0.4, -1.8, -0.25)]], *ring(3, 87, (-20, 3), 0.37), max_pts="equal", min_hits=3)


def _c_cap16():
    rng = np.random.default_rng(16)
    return _scene([[0.5, 0.25, 0.0, 2.1]], [_ring_boxes(rng, 16)], *ring(4, 64, (-25, 6), 0.5), max_pts="below", min_hits=2)


def _c_cap256():
    rng = np.random.default_rng(256)
    return _scene([[0.0, 0.0, 0.0, 0.9]], [_ring_boxes(rng, 256, 4.0, 45.0)], *ring(3, 87, (-18, 4), 0.11), min_hits=1)


def _c_seven_sweeps():
    rng = np.random.default_rng(73)
    frames = [_ring_boxes(rng, 5), _ring_boxes(rng, 12), _ring_boxes(rng, 12)]
    sensors = [[rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-0.2, 0.2), rng.uniform(-3, 3)] for _ in range(7)]
    # frame 1 is read with a negative count (empty), frame 2 with one beyond the table (clamped to cap): the 12 rows there are real boxes
    return _scene(sensors, frames, *ring(3, 87, (-22, 5), 0.73), frame_of=[2, 0, 1, 2, 0, 2, 1], counts=[5, -3, 40], cap=12, min_hits=2)


def _c_max_pts_1():
    rng = np.random.default_rng(5)
    return _scene([[0, 0, 0, 0.0], [2.0, 1.0, 0.0, 1.0]], [_ring_boxes(rng, 6)], *ring(4, 64, (-25, 6), 0.25), max_pts=1)


def _c_one_ray():
    beam, az = ring(1, 1, (-5, -5), 0.0)
    # sweep 0 looks at the box, sweep 1 (turned away, its ground return beyond r_max) gets nothing
    return _scene([[0, 0, 0, 0.0], [0, 0, 0, 2.0]], [[(6.0, 0.0, 2.0, 2.0, 0.2, -1.8, 0.5)]], beam, az, r_max=15.0, min_hits=1)


def _c_sensor_inside():
    return _scene([[0.3, -0.2, -1.0, 0.5]], [[(0.0, 0.0, 2.0, 4.4, 0.3, -1.8, -0.25), (8.0, 2.0, 2.0, 4.4, 1.2, -1.8, -0.25)]],
                  *ring(4, 64, (-25, 6), 0.5), min_hits=1)


def _c_axis_aligned():
    """Identity yaw, sensor at the origin, elevation exactly 0 and azimuth entries of exactly (1, 0) and (0, 1): u == 0 on the y, x and z axes."""
    beam = np.asarray([[1.0, 0.0], [0.96875, -0.25]], np.float32)
    az = np.asarray([[1, 0], [0.75, 0.5], [0, 1], [-0.5, 0.75], [-1, 0], [0, -1], [0.5, -0.75], [0.25, 0.25]], np.float32)
    boxes = [(5.0, 0.0, 2.0, 2.0, 0.0, -1.0, 1.0),       # A: +x ray, uy == 0 with ly = 0 inside: t = 4
             (0.0, 5.0, 2.0, 2.0, 0.0, -1.0, 1.0),       # B: +y ray, ux == 0 with lx = 0 inside: t = 4
             (-10.0, 3.0, 2.0, 2.0, 0.0, -1.0, 1.0),     # C: -x ray, uy == 0 with ly = -3 outside: a miss
             (0.0, -6.0, 2.0, 2.0, 0.0, 0.5, 1.0)]       # D: -y ray at elevation 0, dz == 0 with oz = 0 below z0: a miss
    return _scene([[0, 0, 0, 0.0]], [boxes], beam, az, min_hits=1)


def _c_identical():
    b = (7.0, 1.0, 2.0, 4.4, 0.6, -1.8, -0.25)
    return _scene([[0, 0, 0, 0.1]], [[b, b, (-6.0, 2.0, 2.0, 4.4, 0.2, -1.8, -0.25)]], *ring(4, 64, (-20, 2), 0.5), min_hits=1)


def _c_box_on_ground():
    """Direction (1, 0, -1/2) (the tables need no unit vectors): the box's front face x = 4 and the ground z = -2 are both met at t = 4 exactly."""
    beam = np.asarray([[1.0, -0.5], [1.0, -0.25]], np.float32)
    az = np.asarray([[1, 0]], np.float32)
    return _scene([[0, 0, 0, 0.0]], [[(5.0, 0.0, 2.0, 2.0, 0.0, -2.0, 0.0)]], beam, az, ground_z=-2.0, min_hits=1)


def _c_upward():
    rng = np.random.default_rng(12)
    return _scene([[0, 0, 0, -1.0]], [_ring_boxes(rng, 10, 4.0, 20.0, top=(1.0, 6.0))], *ring(4, 64, (1, 12), 0.5), min_hits=1)


def _c_range_exact():
    """One ray along +x, elevation 0 (no ground).  Faces at 3.5, 4 (= r_min), 8 (= r_max) and 8.5 m: only the middle two return."""
    beam, az = np.asarray([[1.0, 0.0]], np.float32), np.asarray([[1.0, 0.0]], np.float32)
    frames = [[(face + 1.0, 0.0, 2.0, 2.0, 0.0, -1.0, 1.0)] for face in (3.5, 4.0, 8.0, 8.5)]
    return _scene([[0, 0, 0, 0.0]] * 4, frames, beam, az, frame_of=[0, 1, 2, 3], r_min=4.0, r_max=8.0, min_hits=1)


def _c_dropped():
    nan = float("nan")
    rows = [(8.0, 0.0, 2.0, 4.4, 0.3, -1.8, -0.25), (4.0, 0.0, nan, 4.4, 0.3, -1.8, 1.0), (0.0, 8.0, 2.0, 4.4, 1.3, -1.8, -0.25),
            (0.0, 4.0, -2.0, 4.4, 0.0, -1.8, 1.0), (-4.0, 0.0, 3.0, 3.0, 0.0, 1.0, -1.8), (-8.0, 0.0, 2.0, 4.4, 2.3, -1.8, -0.25),
            (0.0, -4.0, 3.0, 3.0, float("inf"), -1.8, 1.0)]
    return _scene([[0, 0, 0, 0.2]], [rows], *ring(4, 64, (-20, 2), 0.5), min_hits=1)


def _c_drop(p, **kw):
    def build():
        rng = np.random.default_rng(31)
        return _scene([[0, 0, 0, 0.4], [1.0, 1.0, 0.1, -2.0]], [_ring_boxes(rng, 8)], *ring(3, 87, (-22, 4), 0.2), p_drop=p, min_hits=2, **kw)
    return build


def _c_occlusion():
    """A (at the origin) looks along +x at a wall; the car stands behind it; B stands beyond the car and looks back.  The wall is as tall as the
    sensor's highest beam reaches at the car, so nothing of A's passes over it."""
    wall = (6.0, 0.0, 0.5, 12.0, 0.0, -1.8, 2.0)
    car = (12.0, 0.5, 4.4, 2.0, 0.0, -1.8, -0.25)
    return _scene([[0, 0, 0, 0.0], [18.0, -1.0, 0.0, 3.0]], [[wall, car]], *ring(8, 128, (-25, 5), 0.5), min_hits=5)


CASES = [("no_boxes_4x64", _c_no_boxes), ("one_box_3x87_max_pts_equal", _c_one_box), ("cap16_full_4x64_max_pts_below", _c_cap16),
         ("cap256_full_3x87", _c_cap256), ("seven_sweeps_three_frames_shuffled", _c_seven_sweeps), ("max_pts_1", _c_max_pts_1),
         ("one_ray", _c_one_ray), ("sensor_inside_a_box", _c_sensor_inside), ("axis_aligned_u_zero", _c_axis_aligned),
         ("identical_boxes_tie", _c_identical), ("box_on_ground_tie", _c_box_on_ground), ("upward_beams_only", _c_upward),
         ("range_exactly_r_min_r_max", _c_range_exact), ("dropped_between_live", _c_dropped), ("p_drop_0", _c_drop(0.0)), ("p_drop_1", _c_drop(1.0)),
         ("p_drop_half", _c_drop(0.5)), ("step_2p48m1_seed_high_bits", _c_drop(0.5, step=(1 << 48) - 1, seed=(0xF00DFACE << 32) | 0x80000001)),
         ("occlusion_wall", _c_occlusion)]
NAMES = [n for n, _ in CASES]
EXACT_TIES = ("identical_boxes_tie", "box_on_ground_tie", "axis_aligned_u_zero", "range_exactly_r_min_r_max")     # checked by hand-written expectations too
NOISE_CASES = [("noise_3x87", _c_drop(0.0, sigma_r=0.05)), ("noise_and_drop_3x87", _c_drop(0.5, sigma_r=0.02, step=1 << 33))]


def _finish(sc):
    sc = dict(sc)
    if isinstance(sc["max_pts"], str):
        returns = int(cast_ref(sc, max_pts=1)["returns"].max())
        sc["max_pts"] = {"above": returns + 9, "equal": max(returns, 1), "below": max(returns - 7, 1)}[sc["max_pts"]]
    ref = cast_ref(sc)
    ref["gt_own"], ref["gt_any"] = visible_ref(sc, ref["box_hits"], False), visible_ref(sc, ref["box_hits"], True)
    for v in list(sc.values()) + list(ref.values()):
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    sc["ref"] = ref
    return sc


@functools.lru_cache(maxsize=None)
def make_case(index):
    """The scene of CASES[index] with its reference under "ref".  Computed once per process and shared: the arrays are read-only."""
    return _finish(CASES[index][1]())


@functools.lru_cache(maxsize=None)
def make_noise_case(index):
    return _finish(NOISE_CASES[index][1]())

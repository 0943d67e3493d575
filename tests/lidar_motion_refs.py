"""Float64 reference, a second exact statement and the case table of the MOVING LiDAR ray cast (csrc/lidar_cast.hip: v2x_lidar_cast_moving,
v2x_lidar_visible_boxes_moving; DESIGN.md section 3.12 "moving scenes").  It builds on tests/lidar_refs.py (the static rule, the draw, the tables) and
changes nothing in it.

`cast_moving_ref` / `visible_moving_ref` state the rule in numpy float64, one operation per statement: every box and sensor moves at constant
velocity from its pose at time 0, ray r = b * NA + a of sweep s is cast at T = time_of[s] + az_time[a], and the sensor origin in box g's frame is
l = l0 + dl * T with dl the relative velocity (sensor minus box) rotated into the box's frame.  Everything else is lidar_refs' rule.

`exact_moving_sweep` is the independent statement: fractions.Fraction in WORLD coordinates -- origin o0 + vs*T, centre c0 + vg*T, the ray clipped
against the six half-spaces of the box where it is at T.  No box-frame relative velocity, no rounding.  It carries lidar_refs' SHAKY margin.

What is not finite (the rule's choice, tested as case "non_finite_times"): a box with a non-finite velocity is dropped, keeping its index; a sweep
whose time_of or sensor_vel is not finite meets no box and has no ground truth; a ray whose az_time is not finite meets no box.  The ground answers.
"""
import functools
import math
from fractions import Fraction

import numpy as np

import lidar_refs as LR


def az_times(na, sweep_time=0.1):
    return (np.arange(na, dtype=np.float64) * sweep_time / na).astype(np.float32)


def _finite(*v):
    return bool(np.isfinite(np.asarray(v, np.float64)).all())


def _fma(a, b, c):
    """round(a * b + c), one rounding (float(Fraction) rounds to nearest even)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _moved(l0, dl, T, fused):
    if fused:
        return np.array([_fma(dl, t, l0) for t in T])
    step = dl * T
    return l0 + step


# ---- the float64 statement of the rule -------------------------------------------------------------------------------------------------------
def sweep_moving_ref(sen, svel, t0, boxes, bvel, count, beam, az, az_time, ground_z, fused=False):
    """One sweep: -> (t (R,) float64, inf without a candidate; id (R,) int: 1 + g, 0 ground, -1 nothing).  fused: l0 + dl*T with ONE rounding (what a
    fused multiply-add would give) instead of the rule's two -- for the case that shows the difference."""
    dx, dy, dz = LR.directions(beam, az)
    nb = beam.shape[0]
    ox, oy, oz, c, s = (np.float64(sen[k]) for k in (0, 1, 2, 4, 5))
    vsx, vsy = np.float64(svel[0]), np.float64(svel[1])
    ta = np.tile(az_time.astype(np.float64), nb)                  # ray r = b * NA + a
    ray_ok = np.isfinite(ta)
    with np.errstate(invalid="ignore"):
        T = np.float64(np.float32(t0)) + ta
    T = np.where(ray_ok, T, 0.0)
    sweep_ok = _finite(svel[0], svel[1], t0)
    wx, wy = c * dx - s * dy, s * dx + c * dy
    best = np.full(dx.shape, np.inf)
    idx = np.full(dx.shape, -1, np.int64)
    for g in range(count if sweep_ok else 0):
        b = boxes[g].astype(np.float64)
        if not LR.box_valid(b) or not _finite(bvel[g, 0], bvel[g, 1]):
            continue
        vgx, vgy = np.float64(bvel[g, 0]), np.float64(bvel[g, 1])
        px, py, cg, sg = ox - b[0], oy - b[1], b[5], b[6]
        qx, qy = vsx - vgx, vsy - vgy
        lx0, ly0 = px * cg + py * sg, -px * sg + py * cg
        dlx, dly = qx * cg + qy * sg, -qx * sg + qy * cg
        lx, ly = _moved(lx0, dlx, T, fused), _moved(ly0, dly, T, fused)
        ux, uy = wx * cg + wy * sg, -wx * sg + wy * cg
        tn, tf, miss = np.full(dx.shape, -np.inf), np.full(dx.shape, np.inf), np.zeros(dx.shape, bool)
        hw, hh = b[2] / 2, b[3] / 2
        for l, u, lo, hi in ((lx, ux, -hw, hw), (ly, uy, -hh, hh), (oz, dz, b[7], b[8])):
            tn, tf, miss = LR._slab(np.broadcast_to(l, dx.shape), u, lo, hi, tn, tf, miss)
        take = ray_ok & ~miss & (tn <= tf) & (tn > 0) & (tn < best)
        best, idx = np.where(take, tn, best), np.where(take, 1 + g, idx)
    with np.errstate(divide="ignore", invalid="ignore"):
        tg = (np.float64(np.float32(ground_z)) - oz) / dz
    take = (dz < 0) & (tg > 0) & (tg < best)
    return np.where(take, tg, best), np.where(take, 0, idx)


def cast_moving_ref(sc, max_pts=None, fused=False):
    """The whole call, in lidar_refs.cast_ref's output form."""
    n, cap = sc["sensors"].shape[0], sc["boxes"].shape[1]
    max_pts = sc["max_pts"] if max_pts is None else max_pts
    dx, dy, dz = LR.directions(sc["beam"], sc["az"])
    sigma = float(np.float32(sc["sigma_r"]))
    out = {"points": np.zeros((n, max_pts, 4), np.float32), "points64": np.zeros((n, max_pts, 4)), "n_pts": np.zeros((n,), np.int32),
           "hit": np.full((n, max_pts), -1, np.int32), "box_hits": np.zeros((n, cap), np.int32), "returns": np.zeros((n,), np.int64),
           "ray_t": np.zeros((n, dx.shape[0])), "ray_id": np.zeros((n, dx.shape[0]), np.int64)}
    r_min, r_max = np.float64(np.float32(sc["r_min"])), np.float64(np.float32(sc["r_max"]))
    for s in range(n):
        f = int(sc["frame_of"][s])
        count = LR.clamp_count(sc["box_count"], f, cap)
        t, idx = sweep_moving_ref(sc["sensors"][s], sc["sensor_vel"][s], sc["time_of"][s], sc["boxes"][f] if count else None,
                                  sc["box_vel"][f] if count else None, count, sc["beam"], sc["az"], sc["az_time"], sc["ground_z"], fused)
        out["ray_t"][s], out["ray_id"][s] = t, idx
        k = 0
        for r in np.nonzero((idx >= 0) & (t >= r_min) & (t <= r_max))[0]:
            w = LR.words(sc["seed"], sc["step"], s, int(r))
            if LR.dropped(w, sc["p_drop"]):
                continue
            out["returns"][s] += 1
            if k >= max_pts:
                continue
            t32 = np.float32(t[r])
            tp = np.float64(t32) + (sigma * LR.normal64(w) if sigma else 0.0)
            if not sigma:
                tp = np.float64(np.float32(tp))
            row = np.array([tp * dx[r], tp * dy[r], tp * dz[r], LR.uniform24(w[3])])
            out["points64"][s, k], out["points"][s, k], out["hit"][s, k] = row, row.astype(np.float32), idx[r]
            if idx[r] >= 1:
                out["box_hits"][s, idx[r] - 1] += 1
            k += 1
        out["n_pts"][s] = k
    return out


def ray_time(t0, ta):
    return np.float64(np.float32(t0)) + np.float64(np.float32(ta))


def rel_centre(c0, o0, vg, vs, T):
    """One world-frame component of the box centre relative to the sensor at T: (c0 - o0) + (vg - vs) * T, every operation rounded."""
    e0 = np.float64(c0) - np.float64(o0)
    dv = np.float64(vg) - np.float64(vs)
    step = dv * np.float64(T)
    return e0 + step


def origin_in_box_frame(sen, svel, b, bv, T):
    """(lx, ly) of the sensor origin in the frame of box row b (9 floats) at time T: the cast's two lines."""
    ox, oy = np.float64(sen[0]), np.float64(sen[1])
    b = np.asarray(b).astype(np.float64)
    px, py, cg, sg = ox - b[0], oy - b[1], b[5], b[6]
    qx, qy = np.float64(svel[0]) - np.float64(bv[0]), np.float64(svel[1]) - np.float64(bv[1])
    lx0, ly0 = px * cg + py * sg, -px * sg + py * cg
    dlx, dly = qx * cg + qy * sg, -qx * sg + qy * cg
    sx, sy = dlx * np.float64(T), dly * np.float64(T)
    return lx0 + sx, ly0 + sy


def visible_moving_ref(sc, box_hits, any_agent, min_hits=None, t_ref=None):
    """-> (gt_boxes (n, cap, 5) fp32, gt_count (n,) int32, gt_ids (n, cap) int32, gt_vel (n, cap, 2) fp32)."""
    n, cap = sc["sensors"].shape[0], sc["boxes"].shape[1]
    min_hits = sc["min_hits"] if min_hits is None else min_hits
    t_ref = sc["t_ref"] if t_ref is None else t_ref
    gt, cnt = np.zeros((n, cap, 5), np.float32), np.zeros((n,), np.int32)
    ids, vel = np.full((n, cap), -1, np.int32), np.zeros((n, cap, 2), np.float32)
    x_lim, y_lim = np.float64(np.float32(sc["x_lim"])), np.float64(np.float32(sc["y_lim"]))
    for s in range(n):
        sen, sv, t0, f = sc["sensors"][s], sc["sensor_vel"][s], np.float32(sc["time_of"][s]), int(sc["frame_of"][s])
        if not _finite(sv[0], sv[1], t0):
            continue
        T = ray_time(t0, t_ref)
        ox, oy, oz, c, sn = (np.float64(sen[k]) for k in (0, 1, 2, 4, 5))
        for g in range(LR.clamp_count(sc["box_count"], f, cap)):
            b32, bv = sc["boxes"][f, g], sc["box_vel"][f, g]
            b = b32.astype(np.float64)
            hits = int(box_hits[s, g])
            if any_agent:
                hits = max(int(box_hits[q, g]) for q in range(n) if int(sc["frame_of"][q]) == f and np.float32(sc["time_of"][q]) == t0)
            if not LR.box_valid(b) or not _finite(bv[0], bv[1]) or hits < min_hits:
                continue
            ex, ey = rel_centre(b32[0], sen[0], bv[0], sv[0], T), rel_centre(b32[1], sen[1], bv[1], sv[1], T)
            x, y = ex * c + ey * sn, -ex * sn + ey * c
            lx, ly = origin_in_box_frame(sen, sv, b32, bv, T)
            inside = abs(lx) <= b[2] / 2 and abs(ly) <= b[3] / 2 and b[7] <= oz <= b[8]
            if abs(x) < x_lim and abs(y) < y_lim and not inside:
                rvx, rvy = np.float64(bv[0]) - np.float64(sv[0]), np.float64(bv[1]) - np.float64(sv[1])
                k = cnt[s]
                gt[s, k] = (np.float32(x), np.float32(y), b32[2], b32[3], np.float32(b32[4]) - np.float32(sen[3]))
                ids[s, k] = g
                vel[s, k] = (np.float32(rvx * c + rvy * sn), np.float32(-rvx * sn + rvy * c))
                cnt[s] += 1
    return gt, cnt, ids, vel


# ---- the exact statement: world coordinates, half-space clipping in rationals ---------------------------------------------------------------
def _fr(v):
    return Fraction(float(v))


def exact_moving_sweep(sen, svel, t0, boxes, bvel, count, beam, az, az_time, ground_z):
    """Per ray ([(t, id)] sorted by (t, boxes in index order before the ground), shaky) as lidar_refs.exact_sweep gives them.  The sensor stands at
    o0 + vs*T, box g's centre at c0 + vg*T; the ray o + t*w is clipped against n . (P - c) <= e for the box's four side planes (n = +-the box's axes
    in the world) and its two z planes.  shaky also when a ray parallel to a plane lies within SHAKY of it."""
    SH = LR.SHAKY
    o0 = (_fr(sen[0]), _fr(sen[1]))
    oz, c, s = _fr(sen[2]), _fr(sen[4]), _fr(sen[5])
    gz = _fr(np.float32(ground_z))
    sweep_ok = _finite(svel[0], svel[1], t0)
    live = []
    for g in range(count if sweep_ok else 0):
        if not LR.box_valid(boxes[g].astype(np.float64)) or not _finite(bvel[g, 0], bvel[g, 1]):
            continue
        b = [_fr(v) for v in boxes[g]]
        live.append((g, b[0], b[1], _fr(bvel[g, 0]), _fr(bvel[g, 1]), b[5], b[6], b[2] / 2, b[3] / 2, b[7], b[8]))
    vs = (_fr(svel[0]), _fr(svel[1])) if sweep_ok else (Fraction(0), Fraction(0))
    rays = []
    for bi in range(beam.shape[0]):
        ce, se = _fr(beam[bi, 0]), _fr(beam[bi, 1])
        for ai in range(az.shape[0]):
            ca, sa = _fr(az[ai, 0]), _fr(az[ai, 1])
            dx, dy, dz = ce * ca, ce * sa, se
            wx, wy = c * dx - s * dy, s * dx + c * dy
            cand, shaky = [], False
            ray_ok = _finite(az_time[ai])
            if ray_ok and live:
                T = _fr(np.float32(t0)) + _fr(az_time[ai])
                sx, sy = o0[0] + vs[0] * T, o0[1] + vs[1] * T             # the sensor in the world at T
            for g, cx0, cy0, vgx, vgy, cg, sg, hw, hh, z0, z1 in (live if ray_ok else ()):
                rx, ry = sx - (cx0 + vgx * T), sy - (cy0 + vgy * T)       # sensor minus the centre where it is at T
                ax_w, ay_w = wx * cg + wy * sg, -wx * sg + wy * cg        # the direction along the box's two axes
                ax_r, ay_r = rx * cg + ry * sg, -rx * sg + ry * cg
                lo, hi, empty = None, None, False
                for a, e in ((ax_w, hw - ax_r), (-ax_w, hw + ax_r), (ay_w, hh - ay_r), (-ay_w, hh + ay_r), (dz, z1 - oz), (-dz, oz - z0)):
                    if a == 0:
                        if abs(e) <= SH:
                            shaky = True
                        if e < 0:
                            empty = True
                            break
                    elif a > 0:
                        hi = e / a if hi is None else min(hi, e / a)
                    else:
                        lo = e / a if lo is None else max(lo, e / a)
                    if lo is not None and hi is not None and lo > hi + 1:
                        empty = True
                        break
                if empty or lo is None or hi is None:
                    continue
                scale = max(1, abs(lo))
                if abs(hi - lo) <= SH * scale or abs(lo) <= SH:
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


# ---- the case table --------------------------------------------------------------------------------------------------------------------------
def moving(sc, box_vel=None, sensor_vel=None, time_of=None, az_time=None, t_ref=0.05, **kw):
    """A lidar_refs scene with motion; what is not given is zero (az_time: the table of a 0.1 s sweep)."""
    sc = dict(sc)
    n, (F, cap) = sc["sensors"].shape[0], sc["boxes"].shape[:2]
    bv = np.zeros((F, cap, 2), np.float32)
    if box_vel is not None:
        for f, rows in enumerate(box_vel):
            if len(rows):
                bv[f, :len(rows)] = np.asarray(rows, np.float32).reshape(-1, 2)
    sc["box_vel"] = bv
    sc["sensor_vel"] = np.zeros((n, 2), np.float32) if sensor_vel is None else np.asarray(sensor_vel, np.float32).reshape(n, 2)
    sc["time_of"] = np.zeros((n,), np.float32) if time_of is None else np.asarray(time_of, np.float32).reshape(n)
    sc["az_time"] = az_times(sc["az"].shape[0]) if az_time is None else np.asarray(az_time, np.float32).reshape(sc["az"].shape[0])
    sc["t_ref"] = t_ref
    sc.update(kw)
    return sc


def _static_zero_vel(build):
    def make():
        sc = build()
        return moving(sc, time_of=[0.7] * sc["sensors"].shape[0])           # one time for all: any_agent then reads what the static rule reads
    return make


def _static_zero_time(build, seed):
    def make():
        sc = build()
        rng = np.random.default_rng(900 + seed)
        n, (F, cap) = sc["sensors"].shape[0], sc["boxes"].shape[:2]
        return moving(sc, box_vel=rng.uniform(-15, 15, (F, cap, 2)), sensor_vel=rng.uniform(-15, 15, (n, 2)), az_time=np.zeros(sc["az"].shape[0]), t_ref=0.0)
    return make


def _cap16_scene(seed=16, **kw):
    rng = np.random.default_rng(seed)
    return LR._scene([[0.5, 0.25, 0.0, 2.1], [-1.0, 2.0, 0.1, -0.4]], [LR._ring_boxes(rng, 16)], *LR.ring(3, 87, (-22, 5), 0.5), min_hits=2, **kw), rng


def _c_common_velocity():
    sc, _ = _cap16_scene()
    v = (3.25, -1.5)
    return moving(sc, box_vel=[[v] * 16], sensor_vel=[v, v], time_of=[1e4, 1e4])


def _drive_out(vy):
    beam, az = LR.ring(3, 87, (-10, 2), 0.0)
    sc = LR._scene([[0, 0, 0, 0.0]], [[(8.0, 0.0, 2.0, 4.0, 0.0, -1.8, 0.5)]], beam, az, min_hits=1)
    return moving(sc, box_vel=[[(0.0, vy)]], az_time=az_times(87, 1.0), t_ref=0.5)


def _c_drives_out():
    """A box 7 m ahead, 4 m wide, drives sideways (+y) at 10 m/s during a sweep of one second: the first azimuth steps (0..4, towards +y) meet it, the
    last ones (83..86, which look where it stood at the start) do not."""
    return _drive_out(10.0)


def _drive_over(time_of):
    beam, az = LR.ring(3, 87, (-10, 2), 0.0)
    sc = LR._scene([[0, 0, 0, 0.0]] * len(time_of), [[(-3.0, 0.0, 2.0, 2.0, 0.0, -1.8, 0.5)]], beam, az, min_hits=1, r_min=0.05)
    return moving(sc, box_vel=[[(6.0, 0.0)]], time_of=time_of, az_time=az_times(87, 1.0), t_ref=0.5)


def _c_drives_over():
    """A 2 m box drives along +x at 6 m/s over a sensor at the origin; the sweep takes one second.  Its centre is at -3 + 6 T: it contains the origin
    for T in [1/3, 2/3], the azimuth steps 29..58, which therefore never return from it.  The second sweep starts at T = 1 with the box ahead."""
    return _drive_over([0.0, 1.0])


def _c_negative_time():
    sc, rng = _cap16_scene(17)
    return moving(sc, box_vel=[rng.uniform(-8, 8, (16, 2))], sensor_vel=rng.uniform(-8, 8, (2, 2)), time_of=[-2.5, -0.375])


def _c_cap256_half_invalid():
    rng = np.random.default_rng(257)
    sc = LR._scene([[0.0, 0.0, 0.0, 0.9]], [LR._ring_boxes(rng, 256, 4.0, 45.0)], *LR.ring(3, 87, (-18, 4), 0.11), min_hits=1)
    vel = rng.uniform(-6, 6, (256, 2))
    vel[0::4, 0] = np.nan
    vel[2::4, 1] = np.inf
    vel[6::8, 0] = -np.inf
    return moving(sc, box_vel=[vel], sensor_vel=[(1.5, -2.0)], time_of=[0.4])


def _c_wall_then_clear():
    """lidar_refs' occlusion scene with one sensor and a car that drives sideways (+y, 10 m/s): hidden behind the wall in the sweep at T = 0, beside
    it in the sweep at T = 1.5."""
    wall, car = (6.0, 0.0, 0.5, 12.0, 0.0, -1.8, 2.0), (12.0, 0.5, 4.4, 2.0, 0.0, -1.8, -0.25)
    sc = LR._scene([[0, 0, 0, 0.0]] * 2, [[wall, car]], *LR.ring(3, 87, (-5, -1), 0.0), min_hits=2)
    return moving(sc, box_vel=[[(0.0, 0.0), (0.0, 10.0)]], time_of=[0.0, 1.5])


def _c_one_ray():
    beam, az = LR.ring(1, 1, (-5, -5), 0.0)
    sc = LR._scene([[0, 0, 0, 0.0]] * 2, [[(6.0, 0.0, 2.0, 2.0, 0.0, -1.8, 0.5)]], beam, az, r_max=15.0, min_hits=1)
    return moving(sc, box_vel=[[(0.0, 4.0)]], time_of=[0.0, 1.0], az_time=[0.0])          # at T = 1 the box has left the ray; the ground lies beyond r_max


def _c_max_pts_below():
    sc, rng = _cap16_scene(18, max_pts="below")
    return moving(sc, box_vel=[rng.uniform(-8, 8, (16, 2))], sensor_vel=rng.uniform(-3, 3, (2, 2)), time_of=[0.2, 0.4])


FMA_A = 2.0 ** -27


def _c_fma():
    """Ray a = 0 looks along +x exactly (uy == 0), so the y slab is the closed test |ly| <= h/2 on ly = ly0 + dly*T alone.  With dly = T = 1 + 2^-27 the
    product is 1 + 2^-26 + 2^-54, which rounds to 1 + 2^-26; ly0 = 2^-41 - (1 + 2^-26) and h/2 = 2^-41: two roundings give ly = 2^-41, ON the slab's
    edge (a hit), one rounding gives 2^-41 + 2^-54, outside it (a miss).  A second, ordinary moving box gives the other rays something to meet."""
    beam, az = LR.ring(3, 87, (-10, 2), 0.0)
    thin = (6.0, 1.0, 2.0, 2.0 ** -40, 0.0, -1.8, 0.5)
    other = (-7.0, 3.0, 4.4, 2.0, 0.7, -1.8, 0.5)
    sc = LR._scene([[0.0, -(2.0 ** -26 - 2.0 ** -41), 0.0, 0.0]], [[thin, other]], beam, az, min_hits=1)
    at = az_times(87)
    at[0] = FMA_A
    return moving(sc, box_vel=[[(0.0, -FMA_A), (2.0, -1.0)]], sensor_vel=[(0.0, 1.0)], time_of=[1.0], az_time=at)


def _c_non_finite():
    sc, rng = _cap16_scene(19)
    sc = dict(sc)
    sc["sensors"] = np.concatenate([sc["sensors"], sc["sensors"]])
    sc["frame_of"] = np.zeros((4,), np.int32)
    at = az_times(87)
    at[5], at[40], at[41] = np.nan, np.inf, -np.inf
    return moving(sc, box_vel=[rng.uniform(-8, 8, (16, 2))], sensor_vel=[(1.0, 2.0), (np.inf, 0.0), (0.0, np.nan), (-1.0, 0.5)],
                  time_of=[0.3, 0.3, 0.3, np.nan], az_time=at)


STATIC_ZERO_VEL = [("zero_vel_" + n, _static_zero_vel(b)) for n, b in LR.CASES]
STATIC_ZERO_TIME = [("zero_time_" + n, _static_zero_time(b, k)) for k, (n, b) in enumerate(LR.CASES)]
CASES = STATIC_ZERO_VEL + STATIC_ZERO_TIME + [
    ("common_velocity_t1e4", _c_common_velocity), ("drives_out_of_the_beam", _c_drives_out), ("drives_over_the_sensor", _c_drives_over),
    ("negative_time_of", _c_negative_time), ("cap256_half_invalid_velocity", _c_cap256_half_invalid), ("wall_then_clear_two_times", _c_wall_then_clear),
    ("one_ray_1x1", _c_one_ray), ("max_pts_below_moving", _c_max_pts_below), ("fma_differs", _c_fma), ("non_finite_times", _c_non_finite)]
NAMES = [n for n, _ in CASES]
N_STATIC = len(LR.CASES)
# the copies of lidar_refs scenes in which every ray meets a box (one ray per sweep looking at a face; two rays at one box): no ray can miss
NO_MISS = ("range_exactly_r_min_r_max", "box_on_ground_tie")


def _noise():
    sc, rng = _cap16_scene(20, sigma_r=0.05, p_drop=0.5, step=1 << 33)
    return moving(sc, box_vel=[rng.uniform(-8, 8, (16, 2))], sensor_vel=rng.uniform(-3, 3, (2, 2)), time_of=[0.2, 0.2])


NOISE_CASES = [("noise_and_drop_moving_3x87", _noise)]


def _finish(sc):
    sc = dict(sc)
    if isinstance(sc["max_pts"], str):
        returns = int(cast_moving_ref(sc, max_pts=1)["returns"].max())
        sc["max_pts"] = {"above": returns + 9, "equal": max(returns, 1), "below": max(returns - 7, 1)}[sc["max_pts"]]
    ref = cast_moving_ref(sc)
    ref["gt_own"], ref["gt_any"] = visible_moving_ref(sc, ref["box_hits"], False), visible_moving_ref(sc, ref["box_hits"], True)
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


def static_twin(sc):
    """lidar_refs' reference of the same scene with nothing moving (its max_pts resolved as the moving case resolved it)."""
    st = {k: v for k, v in sc.items() if k != "ref"}
    ref = LR.cast_ref(st)
    ref["gt_own"], ref["gt_any"] = LR.visible_ref(st, ref["box_hits"], False), LR.visible_ref(st, ref["box_hits"], True)
    return ref


# ---- hand-made sequences for the tracking pipeline -------------------------------------------------------------------------------------------
def sequence_scene(sensors, cars, car_vel, walls, steps, dt, ring, sensor_vel=None, sweep_time=0.1, **kw):
    """One world, `steps` sweeps per sensor at k * dt, agent-major (m = a * steps + k): cars first (box_count for the ground truth = the cars), walls
    after them.  -> a scene dict for cast_moving_ref with "car_count"."""
    beam, az = ring
    A = len(sensors)
    rows = [s for s in sensors for _ in range(steps)]
    sc = LR._scene(rows, [list(cars) + list(walls)], beam, az, **kw)
    sv = [(0.0, 0.0)] * A if sensor_vel is None else sensor_vel
    sc = moving(sc, box_vel=[list(car_vel) + [(0.0, 0.0)] * len(walls)], sensor_vel=[v for v in sv for _ in range(steps)],
                time_of=[k * dt for _ in range(A) for k in range(steps)], az_time=az_times(az.shape[0], sweep_time), t_ref=sweep_time / 2)
    sc["car_count"] = np.asarray([len(cars)], np.int32)
    sc["world7"] = {"sensors": np.asarray(sensors, np.float32), "sensor_vel": np.asarray(sv, np.float32), "boxes": np.asarray(list(cars) + list(walls), np.float32),
                    "box_vel": np.asarray(list(car_vel) + [(0.0, 0.0)] * len(walls), np.float32), "cars": len(cars)}
    sc["max_pts"] = beam.shape[0] * az.shape[0]
    return sc


def open_road(steps=8, dt=0.2, ring=None):
    """Three cars at speeds of at most 6 m/s, at least 8 m apart, no walls; two standing sensors."""
    cars = [(10.0, 4.0, 4.4, 2.0, 0.0, -1.8, -0.25), (-8.0, -6.0, 4.4, 2.0, math.pi / 2, -1.8, -0.25), (2.0, 14.0, 4.4, 2.0, math.pi, -1.8, -0.25)]
    vel = [(5.0, 0.0), (0.0, 6.0), (-4.0, 0.0)]
    return sequence_scene([[0, 0, 0, 0.0], [4.0, -14.0, 0.0, 1.2]], cars, vel, [], steps, dt, ring or LR.ring(8, 256, (-12, 0), 0.0), min_hits=5)


def wall_road(steps=8, dt=0.2, ring=None):
    """Car 0 drives along +y at 8 m/s behind a wall as sensor A (at the origin) sees it: visible in steps 0..1, hidden in steps 2..3 (longer than
    max_age = 1), visible again in steps 4..7.  A is turned so that it looks at the car early in its sweep.  Sensor B stands on the other side and
    sees the car throughout.  Car 1 stands in the open."""
    cars = [(12.0, -4.0, 2.0, 4.4, 0.0, -1.8, -0.25), (-9.0, 5.0, 4.4, 2.0, 0.3, -1.8, -0.25)]
    vel = [(0.0, 8.0), (0.0, 0.0)]
    walls = [(6.0, 0.0, 0.5, 3.9, 0.0, -1.8, 2.0)]
    return sequence_scene([[0, 0, 0, -0.6], [24.0, 0.0, 0.0, 3.0]], cars, vel, walls, steps, dt, ring or LR.ring(8, 256, (-12, 0), 0.0), min_hits=5)


def reference_pipeline(sc, gt_mode, steps, max_age=1, min_hits=3):
    """cast_moving_ref -> visible_moving_ref (read with the car count) -> tests/track_refs.SortRef in float64 on the stand-up boxes, per agent of the
    one world of `sc` (sequence_scene's order).  -> per agent (gts {frame: (ids = 1 + box index, stand-up boxes)}, trks {frame: (track ids, boxes)}),
    frames from 1."""
    import post_refs
    import track_refs as TR
    ref = cast_moving_ref(sc)
    gt, cnt, ids, _ = visible_moving_ref(dict(sc, box_count=sc["car_count"]), ref["box_hits"], gt_mode == "any")
    out = []
    for a in range(sc["sensors"].shape[0] // steps):
        trk, gts, trks = TR.SortRef(max_age=max_age, min_hits=min_hits), {}, {}
        for k in range(steps):
            m = a * steps + k
            su = post_refs.standup64(post_refs.corners64(gt[m, :cnt[m]]))
            gts[k + 1] = ([1 + int(i) for i in ids[m, :cnt[m]]], su)
            boxes, tid, _ = trk.step(su.astype(np.float32))
            trks[k + 1] = (tid.tolist(), boxes)
        out.append((gts, trks))
    return out


def world_of(scenes):
    """sequence_scene dicts -> one dict in utils/raycast_scene.make_moving_world's form (what the sequence builder and synth_tracks.py read): a world
    per scene, agent-major sensors m = a * scenes + w."""
    W, A = len(scenes), len(scenes[0]["world7"]["sensors"])
    cap = max(len(sc["world7"]["boxes"]) for sc in scenes)
    out = {"boxes": np.zeros((W, cap, 7), np.float32), "box_vel": np.zeros((W, cap, 2), np.float32), "box_count": np.zeros((W,), np.int32),
           "car_count": np.zeros((W,), np.int32), "sensors": np.zeros((A * W, 4), np.float32), "sensor_vel": np.zeros((A * W, 2), np.float32),
           "frame_of": np.tile(np.arange(W, dtype=np.int32), A), "num_agent": np.full((W, A), A, np.int64)}
    for w, sc in enumerate(scenes):
        w7 = sc["world7"]
        n = len(w7["boxes"])
        out["boxes"][w, :n], out["box_vel"][w, :n], out["box_count"][w], out["car_count"][w] = w7["boxes"], w7["box_vel"], n, w7["cars"]
        for a in range(A):
            out["sensors"][a * W + w], out["sensor_vel"][a * W + w] = w7["sensors"][a], w7["sensor_vel"][a]
    return out

"""The MOVING LiDAR ray cast (csrc/lidar_cast.hip: v2x_lidar_cast_moving / v2x_lidar_visible_boxes_moving; DESIGN.md section 3.12 "moving scenes")
without a GPU: the float64 reference of tests/lidar_motion_refs.py against the static reference where nothing can move, against hand-written
expectations where something does, and against its second, exact statement (rationals, world coordinates) on every case of the table; the one case
where a fused multiply-add would show; csrc/lidar_math.h's three new expressions through a host driver bit for bit; make_moving_world; the C ABI's
argument checks; synth_tracks.py's parser and ground-truth lines; and the whole reference pipeline sweep -> ground truth -> float64 SORT -> CLEAR MOT on
the two hand-made sequences.

The exact statement sets a ray aside when a decision of it lies within lidar_refs.SHAKY of flipping, or when its two best candidates differ by less
than that without being EQUAL (an exact tie is decided by the rule: lowest index, a box over the ground).  At most 2 % of a case's rays may be set
aside and every case needs a decided box hit and a decided ray without one -- except `no_boxes` and the copies of the two lidar_refs scenes named in
lidar_motion_refs.NO_MISS, which have four and two rays, every one of them aimed at a box face (one of the two a deliberate three-way tie)."""
import ctypes as C
import importlib.util
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import lidar_motion_refs as MR
import lidar_refs as LR
import post_refs
import track_refs as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "v2x-sim_amd", "csrc")


def _case(name):
    return MR.make_case(MR.NAMES.index(name))


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _az_hits(sc, s, box):
    """Per beam, the azimuth indices whose ray returns from `box` in sweep s."""
    nb = sc["beam"].shape[0]
    rid, t = sc["ref"]["ray_id"][s].reshape(nb, -1), sc["ref"]["ray_t"][s].reshape(nb, -1)
    ok = (rid == 1 + box) & (t >= np.float32(sc["r_min"])) & (t <= np.float32(sc["r_max"]))
    return [np.nonzero(row)[0].tolist() for row in ok]


# ---- where nothing can move, the static reference's bytes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", list(range(2 * MR.N_STATIC)) + [MR.NAMES.index("common_velocity_t1e4")],
                         ids=MR.NAMES[:2 * MR.N_STATIC] + ["common_velocity_t1e4"])
def test_static_bytes(index):
    """Zero velocities at non-zero times, non-zero velocities at zero times, one common velocity at T = 1e4 s: lidar_refs' reference, byte for byte."""
    sc = MR.make_case(index)
    ref, st = sc["ref"], MR.static_twin(sc)
    if index < MR.N_STATIC:
        assert not sc["box_vel"].any() and not sc["sensor_vel"].any() and sc["time_of"].all() and sc["az_time"][1:].all()
    elif index < 2 * MR.N_STATIC:
        assert not sc["time_of"].any() and not sc["az_time"].any() and sc["sensor_vel"].all() and sc["box_vel"].all()
    else:
        assert (sc["time_of"] == 1e4).all() and (sc["box_vel"][0, :16] == sc["sensor_vel"][0]).all() and sc["sensor_vel"].all()
    for k in ("points", "n_pts", "hit", "box_hits", "ray_t", "ray_id"):
        assert _bits(ref[k], st[k]), (MR.NAMES[index], k)
    for key in ("gt_own", "gt_any"):
        assert _bits(ref[key][0], st[key][0]) and _bits(ref[key][1], st[key][1]), (MR.NAMES[index], key)
        gt, cnt, ids, vel = ref[key]
        for s in range(len(cnt)):
            assert (ids[s, cnt[s]:] == -1).all() and (np.diff(ids[s, :cnt[s]]) > 0).all() and not vel[s, cnt[s]:].any()
            if index != MR.NAMES.index("common_velocity_t1e4") and index < MR.N_STATIC:
                assert not vel[s].any()
    if index == MR.NAMES.index("common_velocity_t1e4"):
        assert not ref["gt_own"][3].any() and ref["gt_own"][1].sum() > 4                   # relative velocity exactly zero


# ---- where something moves: expectations written by hand ----------------------------------------------------------------------------------------
def test_box_drives_out_of_the_beam():
    """The box stands 7 m ahead across azimuths -4..4 (of 87) at T = 0 and drives towards +y at 10 m/s during a one-second sweep: steps 0..4 meet it
    (at step 4, 16.6 degrees, the ray passes x = 7 at y = 2.08 with the box reaching up to 2.46; at step 5 at 2.64 against 2.57), steps 83..86,
    which look where it stood, do not.  With the box standing still the sweep is symmetric."""
    sc = _case("drives_out_of_the_beam")
    assert _az_hits(sc, 0, 0) == [[0, 1, 2, 3, 4]] * 3
    assert sc["ref"]["box_hits"].tolist() == [[15]]
    still = MR.cast_moving_ref(MR._drive_out(0.0), max_pts=300)
    assert [np.nonzero(r)[0].tolist() for r in (still["ray_id"][0].reshape(3, 87) == 1)] == [[0, 1, 2, 3, 84, 85, 86]] * 3
    gt, cnt, ids, vel = sc["ref"]["gt_own"]
    assert cnt.tolist() == [1] and ids.tolist() == [[0]] and gt[0, 0].tolist() == [8.0, 5.0, 2.0, 4.0, 0.0] and vel[0, 0].tolist() == [0.0, 10.0]


def test_box_drives_over_the_sensor():
    """Centre at -3 + 6 T, half width 1: the box contains the origin for T in [1/3, 2/3], azimuth steps 29..58 of the one-second sweep -- none of
    them returns from it, while steps before (the box still behind, seen by the rays looking back) and after (the box ahead) do.  The ground truth
    of the first sweep is taken at T = 0.5, the box around the sensor: no label; the second sweep's at T = 1.5, the box 6 m ahead."""
    sc = _case("drives_over_the_sensor")
    for row in _az_hits(sc, 0, 0):
        assert row == [26, 27, 28] + list(range(79, 87))
        assert not set(row) & set(range(29, 59))
    assert _az_hits(sc, 1, 0) == [[0, 1, 2, 3, 4, 5, 86]] * 3
    frozen = MR.cast_moving_ref(_frozen_over(), max_pts=300)                                   # the box standing around the sensor: never a return
    assert (frozen["ray_id"] != 1).all()
    for key in ("gt_own", "gt_any"):
        gt, cnt, ids, vel = sc["ref"][key]
        assert cnt.tolist() == [0, 1] and ids.tolist() == [[-1], [0]] and gt[1, 0].tolist() == [6.0, 0.0, 2.0, 2.0, 0.0] and vel[1, 0].tolist() == [6.0, 0.0]


def _frozen_over():
    sc = MR._drive_over([0.5])
    return dict(sc, box_vel=np.zeros_like(sc["box_vel"]), boxes=np.concatenate([np.zeros((1, 1, 1), np.float32), sc["boxes"][..., 1:]], -1))


def test_wall_hides_the_car_at_the_first_time_only():
    """Sweep 0 at T = 0: the car stands behind the wall, no return.  Sweep 1 at T = 1.5: it has driven 15 m sideways and stands beside the wall, at
    azimuth atan2(15.5 .. 16.5, 12) = 52 .. 54 degrees: steps 12..14 of 87."""
    sc = _case("wall_then_clear_two_times")
    assert _az_hits(sc, 0, 1) == [[]] * 3 and _az_hits(sc, 1, 1) == [[12, 13, 14]] * 3
    assert _az_hits(sc, 0, 0) == _az_hits(sc, 1, 0) and sc["ref"]["box_hits"].tolist() == [[69, 0], [69, 9]]
    gt, cnt, ids, vel = sc["ref"]["gt_own"]
    assert cnt.tolist() == [1, 2] and ids.tolist() == [[0, -1], [0, 1]] and gt[1, 1, :2].tolist() == [12.0, 16.0] and vel[1, 1].tolist() == [0.0, 10.0]
    assert sc["ref"]["gt_any"][1].tolist() == [1, 2]                  # any_agent reads the sweeps of the SAME time: sweep 1's hits do not help sweep 0


def test_one_ray_negative_time_invalid_velocities_and_max_pts():
    sc = _case("one_ray_1x1")
    assert sc["ref"]["n_pts"].tolist() == [1, 0] and sc["ref"]["hit"][:, 0].tolist() == [1, -1] and sc["ref"]["gt_own"][1].tolist() == [1, 0]
    sc = _case("negative_time_of")
    assert (sc["time_of"] < 0).all() and not _bits(sc["ref"]["points"], MR.static_twin(sc)["points"])
    sc = _case("cap256_half_invalid_velocity")
    bad = ~np.isfinite(sc["box_vel"][0]).all(1)
    assert sc["box_count"][0] == 256 and bad.sum() == 128 and not sc["ref"]["box_hits"][0, bad].any() and (sc["ref"]["box_hits"][0, ~bad] > 0).sum() > 5
    ids, cnt = sc["ref"]["gt_own"][2], sc["ref"]["gt_own"][1]
    assert cnt[0] > 3 and not bad[ids[0, :cnt[0]]].any()                                      # a dropped box keeps its index: the survivors keep theirs
    sc = _case("max_pts_below_moving")
    assert int(sc["ref"]["returns"].max()) > sc["max_pts"] and sc["ref"]["n_pts"].tolist() == [min(int(v), sc["max_pts"]) for v in sc["ref"]["returns"]]


def test_what_is_not_finite():
    """The rule's choice: a sweep with a non-finite time_of or sensor_vel meets no box and has no ground truth, a ray with a non-finite az_time meets
    no box; the ground answers all of them."""
    sc = _case("non_finite_times")
    ref = sc["ref"]
    assert ref["box_hits"][0].sum() > 20 and not ref["box_hits"][1:].any() and ref["gt_own"][1].tolist()[1:] == [0, 0, 0] and ref["gt_any"][1][0] > 0
    assert (ref["ray_id"][1:] <= 0).all() and (ref["n_pts"][1:] > 100).all()
    rid = ref["ray_id"][0].reshape(3, 87)
    assert (rid[:, [5, 40, 41]] <= 0).all() and (rid[:, [5, 40, 41]] == 0).any()


# ---- the two statements of the rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(MR.CASES)), ids=MR.NAMES)
def test_reference_equals_the_exact_statement(index):
    sc = MR.make_case(index)
    name, ref, cap = MR.NAMES[index], sc["ref"], sc["boxes"].shape[1]
    total = aside = hits = misses = 0
    for s in range(sc["sensors"].shape[0]):
        f = int(sc["frame_of"][s])
        count = LR.clamp_count(sc["box_count"], f, cap)
        rays = MR.exact_moving_sweep(sc["sensors"][s], sc["sensor_vel"][s], sc["time_of"][s], sc["boxes"][f], sc["box_vel"][f], count, sc["beam"], sc["az"],
                                     sc["az_time"], sc["ground_z"])
        for r, (cand, shaky) in enumerate(rays):
            total += 1
            if shaky or (len(cand) > 1 and 0 < cand[1][0] - cand[0][0] <= LR.SHAKY * max(1, cand[0][0])):
                aside += 1
                continue
            if not cand:
                assert ref["ray_id"][s, r] == -1 and ref["ray_t"][s, r] == np.inf, (s, r)
                misses += 1
            else:
                t = float(cand[0][0])
                assert ref["ray_id"][s, r] == cand[0][1], (s, r, cand[:2], ref["ray_id"][s, r], ref["ray_t"][s, r])
                assert abs(ref["ray_t"][s, r] - t) <= 1e-12 * max(1.0, t), (s, r)
                hits += cand[0][1] >= 1
                misses += cand[0][1] < 1
    print("%s: %d of %d rays set aside, %d decided box hits, %d decided rays without one" % (name, aside, total, hits, misses))
    small = any(name.endswith(n) for n in MR.NO_MISS)
    if not small:
        assert aside <= 0.02 * total, (aside, total)
        assert misses >= 1 and (hits >= 1 or name.endswith("no_boxes_4x64"))
    else:
        assert hits >= 1 and total <= 4


def test_a_fused_multiply_add_would_show():
    """Case fma_differs: the rule's two roundings put ly ON the edge of the thin box's y slab for the rays of azimuth step 0 (a hit, in every beam
    that reaches the box); one rounding puts it 2^-54 outside (a miss).  The reference computes both."""
    sc = _case("fma_differs")
    two, one = sc["ref"], MR.cast_moving_ref(sc, fused=True)
    assert two["ray_id"][0].reshape(3, 87)[:, 0].tolist() == [1, 1, 1] and (one["ray_id"][0].reshape(3, 87)[:, 0] != 1).all()
    assert np.array_equal(two["ray_id"][0].reshape(3, 87)[:, 1:], one["ray_id"][0].reshape(3, 87)[:, 1:])
    assert two["box_hits"][0, 0] == 3 and one["box_hits"][0, 0] == 0 and not _bits(two["points"], one["points"]) and not _bits(two["hit"], one["hit"])
    # the arithmetic, written out
    a = MR.FMA_A
    T = np.float64(np.float32(1.0)) + np.float64(np.float32(a))
    dly = np.float64(1.0) - np.float64(np.float32(-a))
    ly0 = np.float64(np.float32(-(2.0 ** -26 - 2.0 ** -41))) - 1.0
    assert dly * T == 1 + 2.0 ** -26 and ly0 + dly * T == 2.0 ** -41 and MR._fma(dly, T, ly0) == 2.0 ** -41 + 2.0 ** -54


# ---- lidar_math.h through a host driver ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/bin/hipcc") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("lidar_motion") / "lidar_motion_driver")
    cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "lidar_motion_driver.cpp"), "-o", exe, "-lm"]
    if cxx.endswith("hipcc"):
        cmd[1:1] = ["-x", "c++"]
    subprocess.check_call(cmd)
    return lambda path: subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout.splitlines()


def _h32(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", np.float32(v)))[0]


def _h64(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def test_header_arithmetic_bit_for_bit(driver, tmp_path):
    """T, lx, ly and the relative centre as csrc/lidar_math.h computes them (host compiler, no contraction) against the reference's, on the inputs of
    the moving cases: every sweep, up to 16 boxes, 9 azimuth steps each."""
    rows, want = [], []
    for index in range(2 * MR.N_STATIC, len(MR.CASES)):
        sc = MR.make_case(index)
        na = sc["az"].shape[0]
        for s in range(sc["sensors"].shape[0]):
            sen, sv, t0, f = sc["sensors"][s], sc["sensor_vel"][s], sc["time_of"][s], int(sc["frame_of"][s])
            if not np.isfinite([t0, sv[0], sv[1]]).all():
                continue
            for g in range(min(16, LR.clamp_count(sc["box_count"], f, sc["boxes"].shape[1]))):
                b, bv = sc["boxes"][f, g], sc["box_vel"][f, g]
                if not np.isfinite(bv).all() or not np.isfinite(b).all():
                    continue
                lx0, ly0 = MR.origin_in_box_frame(sen, sv, b, bv, 0.0)
                dl = MR.origin_in_box_frame(np.zeros(6, np.float32), sv, np.concatenate([[0, 0], b[2:]]).astype(np.float32), bv, 1.0)
                for a in sorted(set(np.linspace(0, na - 1, 9).astype(int).tolist())):
                    ta = sc["az_time"][a]
                    if not np.isfinite(ta):
                        continue
                    T, T_ref = MR.ray_time(t0, ta), MR.ray_time(t0, sc["t_ref"])
                    lx, ly = MR.origin_in_box_frame(sen, sv, b, bv, T)
                    rows.append(" ".join([_h32(t0), _h32(ta), _h64(lx0), _h64(dl[0]), _h64(ly0), _h64(dl[1]), _h32(b[0]), _h32(sen[0]), _h32(bv[0]), _h32(sv[0]),
                                          _h32(sc["t_ref"])]))
                    want.append(" ".join(_h64(v) for v in (T, lx, ly, T_ref, MR.rel_centre(b[0], sen[0], bv[0], sv[0], T_ref))))
    path = tmp_path / "rows.txt"
    path.write_text("\n".join(rows) + "\n")
    got = driver(str(path))
    assert len(got) == len(want) > 1000
    bad = [k for k, (x, y) in enumerate(zip(got, want)) if x != y]
    assert not bad, (len(bad), rows[bad[0]], got[bad[0]], want[bad[0]])
    assert any(r.split()[3] != _h64(0.0) for r in rows)


# ---- make_moving_world ------------------------------------------------------------------------------------------------------------------------
def test_make_moving_world():
    from v2x_sim_amd.utils import raycast_scene, synthetic_scene
    w1, w2, w3 = (raycast_scene.make_moving_world(2, 3, seed=s) for s in (4, 4, 5))
    assert set(w1) == set(raycast_scene.make_world(1, 3)) | {"box_vel", "sensor_vel"}
    assert all(np.array_equal(w1[k], w2[k]) for k in w1) and not np.array_equal(w1["boxes"], w3["boxes"]) and not np.array_equal(w1["box_vel"], w3["box_vel"])
    assert w1["boxes"].shape == (2, 32, 7) and w1["box_vel"].shape == (2, 32, 2) and w1["sensor_vel"].shape == (6, 2) and w1["frame_of"].tolist() == [0, 1] * 3
    parked = moving = 0
    for seed in (4, 5, 6):
        world = raycast_scene.make_moving_world(2, 3, seed=seed)
        for b in range(2):
            n, cars = int(world["box_count"][b]), int(world["car_count"][b])
            rows, vel = world["boxes"][b, :n].astype(np.float64), world["box_vel"][b, :n].astype(np.float64)
            assert cars >= 20 and n - cars >= 4 and not vel[cars:].any()                                   # walls stand still
            assert rows[:3, 6].tolist() == [0.0] * 3 and (rows[3:cars, 6] == -0.25).all() and (rows[cars:, 6] == 2.0).all()
            for a in range(3):                                                                             # agents come first and carry the sensors
                assert world["sensors"][a * 2 + b].tolist() == [rows[a, 0], rows[a, 1], 0.0, rows[a, 4]]
                assert world["sensor_vel"][a * 2 + b].tolist() == vel[a].tolist()
            speed = np.hypot(vel[:cars, 0], vel[:cars, 1])
            parked, moving = parked + int((speed == 0).sum()), moving + int((speed > 0).sum())
            assert ((speed == 0) | ((speed >= 3.0) & (speed <= 12.0))).all()
            head = np.stack([np.cos(rows[:cars, 4]), np.sin(rows[:cars, 4])], 1)                           # along the heading
            assert np.allclose(vel[:cars], speed[:, None] * head, atol=1e-5)
            for k in range(20):
                now = rows[:cars, :5].copy()
                now[:, :2] += vel[:cars] * (k * 0.2)
                near = [(i, j) for i in range(cars) for j in range(i) if math.hypot(*(now[i, :2] - now[j, :2])) < 6.0]   # farther apart than two diagonals: no overlap
                for i, j in near:
                    assert post_refs.iou_ref64(now[i:i + 1].astype(np.float32), now[j:j + 1].astype(np.float32))[0, 0] == 0.0, (seed, b, k, i, j)
        P = [synthetic_scene._pose(*(float(v) for v in world["sensors"][a * 2][[3, 0, 1]])) for a in range(3)]
        assert np.array_equal(world["trans"][0], synthetic_scene.warp_transforms(P)[0])
    assert parked >= 10 and moving >= 60
    with pytest.raises(ValueError):
        raycast_scene.make_moving_world(1, 5, n_cars=3)


def test_sequence_tables_order_and_poses():
    from v2x_sim_amd import ops
    from v2x_sim_amd.utils import raycast_scene
    world = raycast_scene.make_moving_world(2, 3, seed=1)
    seq = raycast_scene.sequence_tables(world, 4, dt=0.2, t_ref=0.05)
    assert seq["sensors"].shape == (24, 4) and seq["trans"].shape == (8, 3, 3, 4, 4) and seq["num_agent"].tolist() == [[3] * 3] * 8
    for a in range(3):
        for w in range(2):
            for k in range(4):
                m = a * 8 + w * 4 + k
                assert seq["frame_of"][m] == w and seq["time_of"][m] == np.float32(k * 0.2)
                assert np.array_equal(seq["sensors"][m], world["sensors"][a * 2 + w]) and np.array_equal(seq["sensor_vel"][m], world["sensor_vel"][a * 2 + w])
    assert np.allclose(seq["trans"][0], world["trans"][0], atol=1.0) and np.array_equal(seq["trans"][0][..., :2, :2], world["trans"][0][..., :2, :2])
    t = ops.az_time_table(2048, 0.1)
    assert t.dtype == np.float32 and t[0] == 0 and t[1024] == np.float32(0.05) and np.array_equal(t, (np.arange(2048) * 0.1 / 2048).astype(np.float32))
    assert np.array_equal(ops.az_time_table(87, 0.1), MR.az_times(87))


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------------------------------
def test_abi_argument_checks_without_gpu():
    from v2x_sim_amd import _lib
    lib = _lib.load()
    assert "v2x_lidar_cast_moving" in _lib.SIGNATURES and "v2x_lidar_visible_boxes_moving" in _lib.SIGNATURES and lib.v2x_abi_version() == 18
    f, u = C.c_float, C.c_uint64
    one = C.c_void_p(64)            # non-null, aligned, never dereferenced: every call below returns before a launch
    assert lib.v2x_lidar_cast_moving(None, None, None, None, 0, None, None, None, 0, 999, None, 0, None, None, 0, f(0), f(9), f(1), f(-1), f(7), u(0), u(0), None,
                                     None, -5, None, None, None, -1, None) == 0                     # empty: before any check
    assert lib.v2x_lidar_visible_boxes_moving(None, None, None, None, f(float("nan")), None, 0, None, None, None, 0, 999, 1, 0, f(-1), f(-1), None, None, None,
                                              None, None) == 0
    need = lib.v2x_lidar_cast_workspace_size(4, 3, 87, 8)

    def cast(sensors=one, svel=one, time_of=one, frame_of=one, boxes=one, bvel=one, count=one, cap=8, beam=one, az=one, az_time=one, r_min=1.0, r_max=70.0,
             sigma=0.0, p=0.0, points=one, n_pts=one, max_pts=100, hit=None, box_hits=None, ws=one, ws_bytes=need, n_frames=2, nb=3, na=87, n=4):
        return lib.v2x_lidar_cast_moving(sensors, svel, time_of, frame_of, n, boxes, bvel, count, n_frames, cap, beam, nb, az, az_time, na, f(-1.8), f(r_min),
                                         f(r_max), f(sigma), f(p), u(1), u(2), points, n_pts, max_pts, hit, box_hits, ws, ws_bytes, None)

    nan, inf = float("nan"), float("inf")
    for kw, text in ((dict(sensors=None), b"null"), (dict(svel=None), b"null"), (dict(time_of=None), b"null"), (dict(frame_of=None), b"null"),
                     (dict(boxes=None), b"null"), (dict(bvel=None), b"null"), (dict(count=None), b"null"), (dict(beam=None), b"null"), (dict(az=None), b"null"),
                     (dict(az_time=None), b"null"), (dict(points=None), b"null"), (dict(n_pts=None), b"null"), (dict(cap=0), b"box_cap=0"),
                     (dict(cap=257), b"box_cap=257"), (dict(max_pts=0), b"max_pts=0"), (dict(p=1.5), b"p_drop"), (dict(p=nan), b"p_drop"),
                     (dict(sigma=-1.0), b"sigma_r"), (dict(sigma=inf), b"sigma_r"), (dict(r_min=5.0, r_max=4.0), b"r_min"), (dict(ws=None), b"workspace"),
                     (dict(ws_bytes=need - 1), b"workspace"), (dict(ws=C.c_void_p(68)), b"8-byte aligned"), (dict(az_time=C.c_void_p(66)), b"4-byte aligned"),
                     (dict(bvel=C.c_void_p(66)), b"4-byte aligned"), (dict(n_frames=0), b"n_frames"), (dict(nb=0), b"n_beams=0"), (dict(n=-1), b"negative"),
                     (dict(nb=1 << 13, na=1 << 12), b"2^24")):
        assert cast(**kw) == -22, kw
        assert text in lib.v2x_last_error() and b"v2x_lidar_cast_moving" in lib.v2x_last_error(), (kw, lib.v2x_last_error())

    def visible(hits=one, sensors=one, svel=one, time_of=one, t_ref=0.05, frame_of=one, boxes=one, bvel=one, count=one, cap=8, x_lim=29.0, y_lim=29.0, gt=one,
                gt_count=one, ids=one, vel=None, n_frames=2):
        return lib.v2x_lidar_visible_boxes_moving(hits, sensors, svel, time_of, f(t_ref), frame_of, 4, boxes, bvel, count, n_frames, cap, 5, 0, f(x_lim),
                                                  f(y_lim), gt, gt_count, ids, vel, None)

    for kw, text in ((dict(hits=None), b"null"), (dict(sensors=None), b"null"), (dict(svel=None), b"null"), (dict(time_of=None), b"null"),
                     (dict(frame_of=None), b"null"), (dict(boxes=None), b"null"), (dict(bvel=None), b"null"), (dict(count=None), b"null"), (dict(gt=None), b"null"),
                     (dict(gt_count=None), b"null"), (dict(ids=None), b"null"), (dict(cap=0), b"box_cap=0"), (dict(cap=257), b"box_cap=257"),
                     (dict(x_lim=0.0), b"x_lim"), (dict(y_lim=nan), b"y_lim"), (dict(t_ref=nan), b"t_ref"), (dict(t_ref=inf), b"t_ref"),
                     (dict(n_frames=0), b"n_frames"), (dict(vel=C.c_void_p(66)), b"aligned")):
        assert visible(**kw) == -22, kw
        assert text in lib.v2x_last_error() and b"v2x_lidar_visible_boxes_moving" in lib.v2x_last_error(), (kw, lib.v2x_last_error())


# ---- synth_tracks.py and the reference pipeline ----------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("synth_tracks_cli", os.path.join(ROOT, "tools", "track", "synth_tracks.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_synth_tracks_parser_and_ground_truth_lines():
    mod = _tool()
    ap = mod.build_parser()
    a = ap.parse_args(["--out", "d"])
    assert (a.scenes, a.steps, a.num_agent, a.seed, a.gt, a.detections, a.score, a.dt, a.sweep_time) == (2, 20, 5, 0, "own", "gt", False, 0.2, 0.1)
    a = ap.parse_args(["--out", "d", "--scenes", "3", "--steps", "8", "--num_agent", "2", "--seed", "7", "--gt", "any", "--detections", "model", "--com", "v2v",
                       "--resume", "x.pth", "--score"])
    assert (a.scenes, a.steps, a.num_agent, a.seed, a.gt, a.detections, a.com, a.resume, a.score) == (3, 8, 2, 7, "any", "model", "v2v", "x.pth", True)
    for bad in (["--out", "d", "--gt", "all"], ["--out", "d", "--detections", "oracle"], []):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    # a two-step hand-made table: box 4 axis-aligned, box 0 turned by 90 degrees (its stand-up box has the extents exchanged)
    steps = [(np.asarray([[10.0, 2.0, 2.0, 4.0, 0.0], [0.0, -5.0, 2.0, 4.0, math.pi / 2]], np.float32), [4, 0]), (np.asarray([[11.0, 2.0, 2.0, 4.0, 0.0]], np.float32), [4])]
    lines = [ln for k, (b, i) in enumerate(steps) for ln in mod.gt_lines(b, i, k + 1)]
    assert lines[0] == "1,5,9.0000,0.0000,2.0000,4.0000,1,-1,-1,-1\n" and lines[2] == "2,5,10.0000,0.0000,2.0000,4.0000,1,-1,-1,-1\n"
    v = lines[1].strip().split(",")
    assert v[:2] == ["1", "1"] and np.allclose([float(t) for t in v[2:6]], [-2.0, -6.0, 4.0, 2.0], atol=1e-4) and v[6:] == ["1", "-1", "-1", "-1"]
    assert mod.gt_lines(np.zeros((0, 5), np.float32), [], 3) == []
    assert np.allclose([float(t) for t in mod.gt_lines(steps[0][0][:1], [4], 1, "h_along_heading")[0].split(",")[2:6]], [8.0, 1.0, 4.0, 2.0], atol=1e-4)


def _clear_mot(gts, track_boxes):
    mot = TR.ClearMotRef()
    for f in sorted(gts):
        mot.update(gts[f][1], gts[f][0], track_boxes[f][1], track_boxes[f][0])
    return mot.result()


def _run(sc, gt_mode, steps):
    return MR.reference_pipeline(sc, gt_mode, steps)


def test_reference_pipeline_open_road_and_wall():
    """Open road: three cars in view of both sensors throughout, every one tracked under one id: IDSW = 0, no miss.  Wall: car 0 (ground-truth id 1)
    is hidden from sensor A in steps 2..3 -- longer than max_age = 1 --, so its track dies and a second one is born: two tracker ids, and a gap in
    A's own ground truth that gt = "any" closes (B sees the car throughout)."""
    for gts, trks in _run(MR.open_road(), "own", 8):
        assert all(sorted(gts[f][0]) == [1, 2, 3] for f in gts)
        res = _clear_mot(gts, trks)
        assert res["IDSW"] == 0 and res["FN"] == 0 and res["FP"] == 0 and res["TP"] == 24, res
    sc = MR.wall_road()
    own, anyb = _run(sc, "own", 8), _run(sc, "any", 8)
    gts, trks = own[0]
    assert [1 in gts[f][0] for f in range(1, 9)] == [True, True, False, False, True, True, True, True] and all(2 in gts[f][0] for f in gts)
    car0 = set()
    for f in gts:
        if 1 in gts[f][0]:
            g = gts[f][1][gts[f][0].index(1)]
            iou = TR.iou_xyxy(g[None], trks[f][1])[0] if len(trks[f][0]) else np.zeros(0)
            car0 |= {trks[f][0][j] for j in np.nonzero(iou > 0.5)[0]}
    assert len(car0) == 2, car0
    assert all(1 in anyb[0][0][f][0] for f in range(1, 9))                                                 # continuous under gt = "any"
    assert all(anyb[1][0][f][0] == own[1][0][f][0] == [1] for f in range(1, 9))                            # B: the car throughout, never the other one

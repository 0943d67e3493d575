"""CPU tests of the free-space ray walk: the float64 reference of tests/vis_refs.py against the exact statement in
fractions.Fraction, the library's own walk (v2x-sim_amd/csrc/vis_math.h through tests/vis_driver.cpp) against the reference byte for byte, the three
states of vis_maps, the wrappers' argument checks and the new signatures.  No GPU."""
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "v2x-sim_amd", "csrc")

import vis_refs as V  # noqa: E402

SMALL = [c for c in V.cases() if max(c.grid.dims[0], c.grid.dims[1]) <= 8 and c.grid.dims[2] <= 4]      # the Fraction check stays at or below 8 x 8 x 4


def _sandwich(req, got, alw):
    return bool(((req & ~got) == 0).all() and ((got & ~alw) == 0).all())


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_reference_lies_between_required_and_allowed(case):
    req, alw = V.exact_grids(case)
    got = V.reference(case.name)
    assert _sandwich(req, got, alw), case.name
    if case.exact:      # a seeded random case: the exact statement fixes every bit, the reference must equal it
        assert np.array_equal(req, alw), "%s: a random ray ties; the case must leave no choice" % case.name
        assert np.array_equal(got, req)


def test_tie_cases_leave_a_choice_and_hold_per_ray():
    """Each named ray on its own: the sandwich, and for the rays named as ties allowed != required -- or they would test nothing.  The band-boundary
    rays live on a 32 x 20 x 16 grid; exact_sets only visits the voxels around each ray."""
    n_ties = 0
    for name in ("unit_ties_stride3", "band_boundary_stride4"):
        case = V.CASES[name]
        got = V.reference(name)
        jobs = case.jobs()
        assert len(jobs) == len(case.ties)
        for (g, qo, qp), tie in zip(jobs, case.ties):
            req, alw = V.exact_sets(case.grid.dims, qo, qp)
            assert _sandwich(req, got[g], alw), (name, g)
            if tie:
                assert not np.array_equal(req, alw), (name, g)
                n_ties += 1
    assert n_ties == sum(sum(V.CASES[n].ties) for n in ("unit_ties_stride3", "band_boundary_stride4")) >= 15


def test_skipped_rays_set_nothing():
    case = V.CASES["unit_ties_stride3"]
    got = V.reference(case.name)
    names = [r[0] for r in V._UNIT_RAYS]
    for n in ("endpoint equal to the origin", "misses the box", "misses the box above", "NaN in the point", "inf in the point", "NaN in the origin",
              "inf in the origin"):
        assert not got[names.index(n)].any(), n
    for n in ("along +x", "origin outside", "endpoint outside", "vertical +z"):
        assert got[names.index(n)].any(), n
    col = got[names.index("vertical +z")]
    assert np.count_nonzero(col) == 1 and col[1, 1] == 0b11                       # a single column, both z bins
    assert not V.reference("small_no_jobs").any() and not V.reference("small_no_points").any()


# ---- the library's own walk ------------------------------------------------------------------------------------------------------------------
def _write_case(case, path):
    n_clouds, max_pts, stride = case.pts.shape
    with open(path, "wb") as f:
        f.write(struct.pack("<8i", n_clouds, max_pts, stride, case.n_jobs, case.n_grids, case.origin is not None, case.xform is not None,
                            case.src is not None))
        f.write(struct.pack("<6d", *case.grid.voxel, *[lo for lo, _ in case.grid.extents]))
        f.write(struct.pack("<4i", *case.grid.dims, 0))
        for a in (case.pts, case.n_pts, case.origin, case.xform, case.src, case.dst):
            if a is not None:
                f.write(a.tobytes())


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/bin/hipcc") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler")
    tmp = tmp_path_factory.mktemp("vis")
    exe = str(tmp / "vis_driver")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "vis_driver.cpp"), "-o", exe, "-lm"]
    if cxx.endswith("hipcc"):
        cmd[1:1] = ["-x", "c++"]
    subprocess.check_call(cmd)
    args = []
    for c in V.cases():
        _write_case(c, str(tmp / (c.name + ".in")))
        args += [str(tmp / (c.name + ".in")), str(tmp / (c.name + ".out"))]
    subprocess.run([exe] + args, check=True)                                       # one process for the whole table
    return lambda name: np.fromfile(str(tmp / (name + ".out")), np.uint32)


@pytest.mark.parametrize("case", V.cases(), ids=lambda c: c.name)
def test_library_walk_gives_the_reference_bytes(driver, case):
    ref = V.reference(case.name)
    got = driver(case.name).reshape(ref.shape)
    assert np.array_equal(got, ref), "%s: %d words differ" % (case.name, int((got != ref).sum()))


# ---- vis_maps' three states ------------------------------------------------------------------------------------------------------------------
def test_one_ray_gives_three_states():
    g = V.G_UNIT
    pts = np.zeros((1, 1, 3), np.float32)
    pts[0, 0] = g.world((3.5, 1.5, 0.5))
    case = V.Case("one_ray", g, pts, np.ones(1, np.int32), origin=g.world((0.5, 1.5, 0.5))[None])
    occ, trav = V.occ_ref(case), V.freespace_ref(case)
    assert occ[0, 3, 1] == 1 and np.count_nonzero(occ) == 1
    assert [int(v) for v in trav[0, :, 1]] == [1, 1, 1, 1] and np.count_nonzero(trav) == 4
    m = V.vis_maps_ref(occ, trav, 2)
    assert m.shape == (1, 4, 4, 2) and m.dtype == np.float32
    v_occ, v_free = np.float32(np.log(0.7 / 0.3)), np.float32(np.log(0.4 / 0.6))
    assert m[0, 3, 1, 0] == v_occ                                                  # the return's voxel: traversed AND occupied reads occupied
    assert (m[0, :3, 1, 0] == v_free).all()                                        # crossed on the way
    m[0, :, 1, 0] = 0
    assert not m.any()                                                             # everything else unknown: 0 = log-odds of 0.5
    lab = np.full((1, 4, 4), 3, np.uint8)
    out = V.mask_labels_ref(lab, occ, trav)
    assert (out[0, :, 1] == 3).all() and np.count_nonzero(out == 255) == 12
    assert (V.mask_labels_ref(lab, occ, trav, z_mask=0b10) == 255).all()


def test_sliver_return_reads_free():
    """The documented consequence: a return between the index lattice and a1's open extents is not occupied, so its voxel may read as free.  On the
    product grid z in [-3.2, -3.0) is such a sliver (floor(-3.0 / 0.4) = -8: the lattice starts at -3.2)."""
    g = V.G_PRODUCT
    pts = np.zeros((1, 1, 4), np.float32)
    pts[0, 0, :3] = (4.1, 0.1, -3.1)
    case = V.Case("sliver", g, pts, np.ones(1, np.int32))
    occ, trav = V.occ_ref(case), V.freespace_ref(case)
    assert not occ.any()
    ix, iy = int(np.floor(4.1 / 0.25)) + 128, 128
    assert trav[0, ix, iy] & 1


# ---- the wrappers' checks and the ABI --------------------------------------------------------------------------------------------------------
def test_ops_vis_argument_checks_raise_before_any_launch():
    import torch
    from v2x_sim_amd import ops, ops_vis
    assert ops.freespace_bits is ops_vis.freespace_bits and ops.vis_maps is ops_vis.vis_maps and ops.mask_unobserved is ops_vis.mask_unobserved
    grid = ops.VoxelGrid()
    pts, cnt = torch.zeros(2, 8, 4), torch.zeros(2, dtype=torch.int32)
    idx = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="points must be"):
        ops_vis.freespace_bits(torch.zeros(8, 4), cnt, grid)
    with pytest.raises(ValueError, match="one count per cloud"):
        ops_vis.freespace_bits(pts, torch.zeros(3, dtype=torch.int32), grid)
    with pytest.raises(ValueError, match="come together"):
        ops_vis.freespace_bits(pts, cnt, grid, src_cloud=idx)
    with pytest.raises(ValueError, match="n_grids is needed"):
        ops_vis.freespace_bits(pts, cnt, grid, src_cloud=idx, dst_grid=idx)
    with pytest.raises(ValueError, match="xform"):
        ops_vis.freespace_bits(pts, cnt, grid, xform=torch.zeros(2, 4, 4))
    with pytest.raises(ValueError, match="origin"):
        ops_vis.freespace_bits(pts, cnt, grid, origin=torch.zeros(3, 3), src_cloud=idx[:2], dst_grid=idx[:2], n_grids=1)
    with pytest.raises(ValueError, match="Z=40"):
        ops_vis.freespace_bits(pts, cnt, ops.VoxelGrid(voxel_size=(0.25, 0.25, 0.125)))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops_vis.freespace_bits(pts, cnt, grid)                                     # a missing device is an error, never a fall-back
    bits = torch.zeros(2, 4, 4, dtype=torch.int32)
    with pytest.raises(ValueError, match="must both be"):
        ops_vis.vis_maps(bits, bits[:1], 2)
    with pytest.raises(ValueError, match="Z=33"):
        ops_vis.vis_maps(bits, bits, 33)
    with pytest.raises(ValueError, match="p_occ"):
        ops_vis.vis_maps(bits, bits, 2, p_occ=1.0)
    with pytest.raises(ValueError, match="labels"):
        ops_vis.mask_unobserved(torch.zeros(2, 4, 5, dtype=torch.uint8), bits, bits)
    with pytest.raises(ValueError, match="ignore"):
        ops_vis.mask_unobserved(torch.zeros(2, 4, 4, dtype=torch.uint8), bits, bits, ignore=256)


def test_new_signatures_match_the_header():
    import ctypes as C
    from v2x_sim_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "v2x_amd.h")).read(), flags=re.S)
    want = {"v2x_lidar_freespace_bits": 16, "v2x_vis_bits_to_dense_f32": 11, "v2x_vis_mask_labels": 10}
    for name, n_args in want.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(params) == len(args) == n_args, name
        for p, a in zip(params, args):
            if "*" in p or p.startswith("v2x_stream_t"):
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p)
            elif p.startswith("float"):
                assert a is C.c_float, (name, p)
            else:
                assert a in (C.c_int, C.c_uint32), (name, p)
    lib = _lib.load()
    assert lib.v2x_abi_version() == _lib.ABI_VERSION == 18                         # entries were added, nothing changed
    # argument validation happens before any HIP call
    assert lib.v2x_lidar_freespace_bits(None, None, 1, 1, 4, None, None, None, None, 1, 1, None, None, None, None, None) == -22
    assert b"v2x_lidar_freespace_bits: null pointer" in lib.v2x_last_error()
    ext, vox = (C.c_double * 6)(-1, 1, -1, 1, -1, 1), (C.c_double * 3)(0.25, 0.25, 0.05)
    assert lib.v2x_lidar_freespace_bits(None, None, 1, 1, 4, None, None, None, None, 1, 1, ext, vox, (C.c_int32 * 3)(8, 8, 40), C.c_void_p(16), None) == -22
    assert b"Z=40 must be in [1,32]" in lib.v2x_last_error()
    assert lib.v2x_vis_bits_to_dense_f32(None, None, 1, 4, 4, 2, 1.0, 0.5, 0.0, None, None) == -22
    assert lib.v2x_vis_mask_labels(None, None, None, 1, 4, 4, 1, 300, None, None) == -22 and b"ignore=300" in lib.v2x_last_error()

"""v2x_lidar_freespace_bits, v2x_vis_bits_to_dense_f32 and v2x_vis_mask_labels on the MI355X against the float64 reference of tests/vis_refs.py
(DESIGN.md section 3.13): every case of the table byte for byte in whichever form its shape selects, the two forms against each other, repeatability,
the dense and the label kernels against numpy, a cast sweep against the voxeliser, and graph capture."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vis_refs as V  # noqa: E402

pytestmark = pytest.mark.gpu


def _grid(g):
    from v2x_sim_amd import ops
    vg = ops.VoxelGrid(g.voxel, g.extents)
    assert vg.dims == g.dims
    return vg


def _t(a, dev):
    return None if a is None else torch.from_numpy(a).to(dev)


def _call(case, dev, out=None):
    from v2x_sim_amd import ops_vis
    return ops_vis.freespace_bits(_t(case.pts, dev), _t(case.n_pts, dev), _grid(case.grid), origin=_t(case.origin, dev), xform=_t(case.xform, dev),
                                  src_cloud=_t(case.src, dev), dst_grid=_t(case.dst, dev), n_grids=case.n_grids, out=out)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _misaligned(case, dev, fill):
    """An output 4 bytes off a 16-byte boundary: the LDS form needs aligned 16-byte stores, so the shape rule hands such a call to the general form --
    the way to run a grid that fits the LDS through the device-scope atomics without any switch."""
    X, Y, _ = case.grid.dims
    buf = torch.full((case.n_grids * X * Y + 4,), fill, dtype=torch.int32, device=dev)
    off = next(o for o in range(1, 5) if (buf.data_ptr() + 4 * o) % 16 == 4)
    return buf, buf[off:off + case.n_grids * X * Y].view(case.n_grids, X, Y), off


@pytest.mark.parametrize("case", V.cases(), ids=lambda c: c.name)
def test_every_case_gives_the_reference_bytes(case, device):
    got = _u32(_call(case, device))
    ref = V.reference(case.name)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), "%s: %d words differ" % (case.name, int((got != ref).sum()))


@pytest.mark.parametrize("name", ["mid_two_jobs_one_target", "product_ring_8192", "band_boundary_stride4"])
def test_both_forms_give_the_same_bytes(name, device):
    case = V.CASES[name]
    X, Y, Z = case.grid.dims
    assert Z <= 16 and X * Y * 2 <= 128 * 1024 and (X * Y) % 8 == 0                 # the shape takes the LDS form ...
    lds = _call(case, device)
    assert lds.data_ptr() % 16 == 0
    buf, view, off = _misaligned(case, device, 0x5a5a5a5a)                          # ... unless the output cannot take 16-byte stores
    general = _call(case, device, out=view)
    assert general.data_ptr() == view.data_ptr() and view.data_ptr() % 16 == 4
    assert torch.equal(lds, general)
    assert np.array_equal(_u32(lds), V.reference(name))
    assert bool((buf[:off] == 0x5a5a5a5a).all()) and bool((buf[off + view.numel():] == 0x5a5a5a5a).all())     # nothing written around the grid


@pytest.mark.parametrize("name", ["mid_two_jobs_one_target", "wide_general_by_size"])
def test_two_calls_give_identical_bytes(name, device):
    case = V.CASES[name]
    X, Y, _ = case.grid.dims
    a = _call(case, device, out=torch.full((case.n_grids, X, Y), -1, dtype=torch.int32, device=device))
    b = _call(case, device, out=torch.full((case.n_grids, X, Y), 0x4b4b4b4b, dtype=torch.int32, device=device))
    assert torch.equal(a, b)                                                        # cleared by the call: whatever the buffer held before


def test_vis_maps_and_mask_equal_numpy(device):
    from v2x_sim_amd import ops, ops_vis
    case = V.CASES["mid_two_jobs_one_target"]
    X, Y, Z = case.grid.dims
    trav = _call(case, device)
    occ = ops.voxelize_fused_bits(_t(case.pts, device), _t(case.n_pts, device), _t(case.xform, device), _t(case.src, device), _t(case.dst, device),
                                  case.n_grids, _grid(case.grid))
    occ_h, trav_h = _u32(occ), _u32(trav)
    assert np.array_equal(occ_h, V.occ_ref(case))
    assert (occ_h & ~trav_h).any() == 0 and (trav_h & ~occ_h).any()                 # every return's voxel was crossed; most crossed voxels are free
    dense = ops_vis.vis_maps(occ, trav, Z).cpu().numpy()
    assert dense.shape == (case.n_grids, X, Y, Z)
    assert np.array_equal(dense.view(np.uint32), V.vis_maps_ref(occ_h, trav_h, Z).view(np.uint32))
    assert len(np.unique(dense)) == 3
    other = ops_vis.vis_maps(occ, trav, Z, p_occ=0.9, p_free=0.2).cpu().numpy()
    assert np.array_equal(other.view(np.uint32), V.vis_maps_ref(occ_h, trav_h, Z, 0.9, 0.2).view(np.uint32))
    rng = np.random.default_rng(3)
    lab_h = rng.integers(0, 8, (case.n_grids, X, Y)).astype(np.uint8)
    for z_mask, ignore in ((None, 255), (0b111100, 7), (0, 200)):
        lab = torch.from_numpy(lab_h).to(device)
        want = V.mask_labels_ref(lab_h, occ_h, trav_h, 0xffffffff if z_mask is None else z_mask, ignore)
        got = ops_vis.mask_unobserved(lab, occ, trav, z_mask=z_mask, ignore=ignore)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(lab.cpu().numpy(), lab_h)
        same = ops_vis.mask_unobserved(lab, occ, trav, z_mask=z_mask, ignore=ignore, out=lab)              # in place
        assert same.data_ptr() == lab.data_ptr() and np.array_equal(lab.cpu().numpy(), want)
    assert (want == 200).all()


def test_cast_sweep_occupied_is_the_voxelisers_and_was_crossed(device):
    """On a ray-cast sweep (origin None: the sensor is the zero vector of its own frame): occupied is v2x_voxelize_bits' result, every occupied voxel was
    crossed by the ray that returned from it, and a return in the sliver z in [-3.2, -3.0) -- below a1's open extent, inside the index lattice -- is not
    occupied while its voxel reads as traversed: free."""
    from v2x_sim_amd import ops, ops_vis
    from v2x_sim_amd.utils import raycast_scene as RS
    world = RS.make_world(1, agents=2, seed=4, n_cars=8, n_walls=4)
    d = RS.world_on_device(world, device)
    beam, az = (torch.from_numpy(t).to(device) for t in ops.ring_table(8, 256))
    cast = ops.lidar_cast(d["sensors"], d["frame_of"], d["boxes"], d["box_count"], beam, az, 8 * 256, ground_z=RS.GROUND_Z, sigma_r=0.02, seed=4, want=())
    pts, cnt = cast["points"], cast["n_pts"]
    pts[0, 0, :3] = torch.tensor([4.1, 0.1, -3.1], device=device)                   # one return into the sliver
    grid = ops.VoxelGrid()
    occ, trav = ops.voxelize_bits(pts, cnt, grid), ops_vis.freespace_bits(pts, cnt, grid)
    case = V.Case("cast", V.G_PRODUCT, pts.cpu().numpy(), cnt.cpu().numpy())
    occ_h, trav_h = _u32(occ), _u32(trav)
    assert np.array_equal(occ_h, V.occ_ref(case)) and np.array_equal(trav_h, V.freespace_ref(case))
    assert occ_h.any() and not (occ_h & ~trav_h).any()
    ix, iy = int(np.floor(4.1 / 0.25)) + 128, 128
    assert trav_h[0, ix, iy] & 1
    m = ops_vis.vis_maps(occ, trav, 13)
    if not occ_h[0, ix, iy] & 1:
        assert float(m[0, ix, iy, 0]) == float(np.float32(np.log(0.4 / 0.6)))


def test_capture_and_replay(device):
    case = V.CASES["band_random_stride3"]
    wide = V.CASES["tall_general_by_z"]
    args = [(c, {k: _t(getattr(c, k), device) for k in ("pts", "n_pts", "origin", "xform")}, _grid(c.grid)) for c in (case, wide)]
    outs = [torch.full((c.n_grids,) + c.grid.dims[:2], -1, dtype=torch.int32, device=device) for c in (case, wide)]
    from v2x_sim_amd import ops_vis
    ops_vis.freespace_bits(args[0][1]["pts"], args[0][1]["n_pts"], args[0][2])      # library loaded, LDS opt-in made before the capture
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for (c, t, vg), o in zip(args, outs):
                ops_vis.freespace_bits(t["pts"], t["n_pts"], vg, origin=t["origin"], xform=t["xform"], out=o)
    for o in outs:
        o.fill_(0x33333333)
    g.replay()
    torch.cuda.synchronize()
    for c, o in zip((case, wide), outs):
        assert np.array_equal(_u32(o), V.reference(c.name)), c.name
    g.replay()
    torch.cuda.synchronize()
    for c, o in zip((case, wide), outs):
        assert np.array_equal(_u32(o), V.reference(c.name)), c.name

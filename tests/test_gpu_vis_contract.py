"""The three wrappers of v2x_sim_amd/ops_vis.py held to the memory half of their contract (include/v2x_amd.h), the way tests/test_gpu_memory_contract.py
holds the other wrapper modules: tests/guarded_alloc.py serves their torch.empty calls from poisoned buffers between guards, every input is copied
into such a buffer, and each call runs plain, under poison 0xFF and under poison 0x4B.  Asserted: every guard byte intact, every output element
written (no poison left where the result is defined: the three runs agree bit for bit), the inputs unchanged."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_alloc as G  # noqa: E402
import vis_refs as V  # noqa: E402

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return None if a is None else torch.from_numpy(a).to(dev)


def _freespace(case, dev, h):
    from v2x_sim_amd import ops, ops_vis
    vg = ops.VoxelGrid(case.grid.voxel, case.grid.extents)
    a = {k: h.guarded(_t(getattr(case, k), dev)) for k in ("pts", "n_pts", "origin", "xform", "src", "dst")}
    return {"trav_bits": ops_vis.freespace_bits(a["pts"], a["n_pts"], vg, origin=a["origin"], xform=a["xform"], src_cloud=a["src"], dst_grid=a["dst"],
                                                n_grids=case.n_grids)}


def _bits_pair(case, dev):
    """occ / trav of a case as plain device tensors (computed outside the harness: inputs of the two conversions)"""
    from v2x_sim_amd import ops, ops_vis
    vg = ops.VoxelGrid(case.grid.voxel, case.grid.extents)
    pts, cnt = _t(case.pts, dev), _t(case.n_pts, dev)
    return ops.voxelize_bits(pts, cnt, vg), ops_vis.freespace_bits(pts, cnt, vg, origin=_t(case.origin, dev), xform=_t(case.xform, dev))


def _vis_maps(case, dev, h):
    from v2x_sim_amd import ops_vis
    occ, trav = (h.guarded(t) for t in _bits_pair(case, dev))
    return {"vis_maps": ops_vis.vis_maps(occ, trav, case.grid.dims[2])}


def _labels(bits):
    return (torch.arange(bits.numel(), device=bits.device) % 7).to(torch.uint8).view(bits.shape)


def _mask(case, dev, h):
    from v2x_sim_amd import ops_vis
    occ, trav = (h.guarded(t) for t in _bits_pair(case, dev))
    return {"labels": ops_vis.mask_unobserved(h.guarded(_labels(occ)), occ, trav, z_mask=0x1ffe)}


def _mask_in_place(case, dev, h):
    from v2x_sim_amd import ops_vis
    occ, trav = (h.guarded(t) for t in _bits_pair(case, dev))
    lab = h.guarded(_labels(occ))
    out = ops_vis.mask_unobserved(lab, occ, trav, out=lab)
    assert out.data_ptr() == lab.data_ptr()
    return {"labels": out}, (lab,)


# the LDS form with two bands, the general form by Z, by size, jobs with indices out of range, no jobs at all: the grids must be cleared in full
FREESPACE_CASES = ["band_random_stride3", "tall_general_by_z", "wide_general_by_size", "small_five_jobs_one_target", "small_no_jobs", "unit_ties_stride3"]
ROWS = [("freespace_bits", _freespace, n) for n in FREESPACE_CASES] + \
       [(f.__name__.strip("_"), f, n) for f in (_vis_maps, _mask, _mask_in_place) for n in ("mid_two_jobs_one_target", "small_random_stride5_n_pts")]


@pytest.mark.parametrize("what,call,name", ROWS, ids=["%s-%s" % (r[0], r[2]) for r in ROWS])
def test_wrapper_keeps_its_memory_contract(what, call, name, device):
    from v2x_sim_amd import ops_vis
    case = V.CASES[name]
    runs = []
    for poison in (None,) + G.POISONS:
        with (G.PlainAlloc() if poison is None else G.GuardedAlloc(poison, modules=[ops_vis])) as h:
            res = call(case, device, h)
            outs, written = res if isinstance(res, tuple) else (res, ())
            torch.cuda.synchronize()
            h.check_guards()
            h.check_operands_unchanged(written=written)
            if poison is not None:
                assert len(h.records) >= 2                                          # the operands, and the wrapper's own output unless in place
            runs.append({k: v.clone() for k, v in outs.items()})
    plain, ff, x4b = runs
    for k in plain:
        # an element the kernel never wrote would hold 0xFF.. in one run and 0x4B.. in the other
        assert G.same_bits(plain[k], ff[k]) and G.same_bits(plain[k], x4b[k]), "%s: output %r differs between the plain and the poisoned runs" % (what, k)
        assert G.new_nans(ff[k], plain[k]) == 0

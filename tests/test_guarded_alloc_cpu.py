"""tests/guarded_alloc.py proved on the CPU: the views it hands out, the restore on exit, four faulty stand-in "entries" of plain torch ops that
must each be caught and a correct one that must pass -- and the completeness cap of tests/test_gpu_memory_contract.py: every public function of
the six wrapper modules is a row of its table or is listed in EXEMPT below because it launches no kernel."""
import types

import pytest
import torch

import guarded_alloc as G

# A stand-in wrapper module: its functions allocate through the module's global `torch`, as ops.py and its siblings do.
_STANDIN_SRC = '''
import torch


def scale2(x):                       # correct: writes every output element, reads its workspace only after writing it
    ws = torch.empty((x.numel(),), dtype=torch.float32, device=x.device)
    out = torch.empty_like(x)
    ws.copy_(x.reshape(-1))
    out.copy_((ws * 2).view(x.shape))
    return out


def writes_before(x):
    out = scale2(x)
    torch.as_strided(out._base.view(out.dtype), (1,), (1,), out.storage_offset() - 1).fill_(7.0)
    return out


def writes_after(x):
    out = scale2(x)
    torch.as_strided(out._base.view(out.dtype), (1,), (1,), out.storage_offset() + out.numel()).fill_(7.0)
    return out


def skips_one(x):
    out = torch.empty_like(x)
    out.reshape(-1)[:-1].copy_(x.reshape(-1)[:-1] * 2)
    return out


def reads_workspace_early(x):
    ws = torch.empty((x.numel(),), dtype=torch.float32, device=x.device)
    out = torch.empty_like(x)
    out.copy_(x * 2)
    out.reshape(-1)[3] += ws[3]      # folded in before anything wrote it
    ws.copy_(x.reshape(-1))
    return out


def cleared(n):
    return torch.zeros((n, 3), dtype=torch.int32), torch.full((n,), -1, dtype=torch.int64), torch.zeros(n)


def raises(x):
    torch.empty_like(x)
    raise KeyError("from the body")
'''


@pytest.fixture()
def standin():
    m = types.ModuleType("guarded_alloc_standin")
    exec(compile(_STANDIN_SRC, "guarded_alloc_standin.py", "exec"), m.__dict__)
    return m


def _three_runs(fn, x, standin):
    """The protocol of tests/test_gpu_memory_contract.py on a stand-in: plain, 0xFF, 0x4B.  -> (plain, [(harness, result)] per poison)."""
    plain = fn(x)
    runs = []
    for poison in G.POISONS:
        with G.GuardedAlloc(poison, modules=[standin], guard_cpu=True) as h:
            runs.append((h, fn(h.guarded(x))))
    return plain, runs


@pytest.mark.parametrize("dtype,shape", [(torch.float32, (3, 5)), (torch.bfloat16, (7,)), (torch.int64, (2, 1, 3)), (torch.uint8, (13,)),
                                         (torch.float64, ()), (torch.int32, (0, 4))])
@pytest.mark.parametrize("poison", G.POISONS)
def test_views_have_shape_dtype_alignment_and_poison(standin, dtype, shape, poison):
    with G.GuardedAlloc(poison, modules=[standin], guard_cpu=True) as h:
        t = standin.torch.empty(shape, dtype=dtype)
        like = standin.torch.empty_like(t)
        z = standin.torch.zeros(shape, dtype=dtype)
        f = standin.torch.full(shape, 3, dtype=dtype)
        for v in (t, like, z, f):
            assert tuple(v.shape) == shape and v.dtype == dtype and v.is_contiguous() and v.data_ptr() % 256 == 0
            r = h.record_of(v)
            assert r.front >= G.GUARD and r.buffer.numel() - r.front - r.nbytes >= G.GUARD and r.nbytes == v.numel() * v.element_size()
        assert G.holds_poison(t, poison) and G.holds_poison(like, poison)
        assert h.record_of(t).poisoned and h.record_of(like).poisoned and not h.record_of(z).poisoned and not h.record_of(f).poisoned
        assert bool((z == 0).all()) and bool((f == 3).all())
        assert [r.kind for r in h.records] == ["empty", "empty_like", "zeros", "full"]
        assert all("test_guarded_alloc_cpu.py" in r.call for r in h.records), h.records[0].call
        h.check_guards()
    assert G.GUARD % 256 == 0 and G.GUARD == 4096 and G.POISONS == (0xFF, 0x4B)


def test_poison_reads_as_documented():
    ff, kb = torch.full((8,), 0xFF, dtype=torch.uint8), torch.full((8,), 0x4B, dtype=torch.uint8)
    for dt in (torch.bfloat16, torch.float32, torch.float64):
        assert bool(torch.isnan(ff.view(dt)).all()) and bool(torch.isfinite(kb.view(dt)).all())
    assert abs(float(kb.view(torch.float32)[0]) - 1.3e7) < 1e6
    assert int(ff.view(torch.int32)[0]) == -1 and int(ff[0]) == 255 and int(kb.view(torch.int32)[0]) > 1 << 30


def test_size_spellings_and_fills(standin):
    with G.GuardedAlloc(0x4B, modules=[standin], guard_cpu=True) as h:
        a, b, c = standin.cleared(4)
        assert a.shape == (4, 3) and a.dtype == torch.int32 and b.dtype == torch.int64 and c.dtype == torch.float32 and c.shape == (4,)
        assert int(a.abs().sum()) == 0 and bool((b == -1).all()) and float(c.abs().sum()) == 0
        assert standin.torch.empty(2, 3, dtype=torch.float32).shape == (2, 3) and standin.torch.empty(5, dtype=torch.uint8).shape == (5,)
        assert standin.torch.float32 is torch.float32 and standin.torch.arange(3).tolist() == [0, 1, 2]          # everything else forwards
        assert "cleared" in h.records[0].call
        h.check_guards()


def test_cpu_allocations_pass_through_without_the_flag(standin):
    with G.GuardedAlloc(0xFF, modules=[standin]) as h:
        x = torch.arange(6.0).view(2, 3)
        assert h.guarded(x) is x and h.guarded(None) is None
        out = standin.scale2(x)
        assert torch.equal(out, x * 2) and h.records == []


def test_torch_is_restored_also_when_the_body_raises(standin):
    mods = G.wrapper_modules()
    assert [m.__name__.rsplit(".", 1)[1] for m in mods] == list(G.WRAPPER_MODULES) and len(mods) == 6
    with G.GuardedAlloc(0xFF, guard_cpu=True) as h:
        assert all(m.torch is h.proxy for m in mods)
        with pytest.raises(RuntimeError):
            G.GuardedAlloc(0x4B).__enter__()                    # a second harness on the same modules
        assert all(m.torch is h.proxy for m in mods)            # ... leaves the first one's proxy in place
    assert all(m.torch is torch for m in mods)
    with pytest.raises(KeyError):
        with G.GuardedAlloc(0xFF, modules=[standin], guard_cpu=True):
            assert standin.torch is not torch
            standin.raises(torch.zeros(3))
    assert standin.torch is torch
    from v2x_sim_amd import _launch
    assert _launch.torch is torch


def test_correct_entry_passes(standin):
    x = torch.arange(12.0).view(3, 4) - 5
    plain, runs = _three_runs(standin.scale2, x, standin)
    for h, got in runs:
        h.check_guards()
        assert G.same_bits(got, plain) and G.new_nans(got, plain) == 0
        assert [r.kind for r in h.records] == ["operand", "empty", "empty_like"]


@pytest.mark.parametrize("name,side", [("writes_before", "in front of"), ("writes_after", "behind")])
def test_a_store_outside_the_output_is_caught(standin, name, side):
    x = torch.arange(12.0).view(3, 4)
    for poison in G.POISONS:
        with G.GuardedAlloc(poison, modules=[standin], guard_cpu=True) as h:
            out = getattr(standin, name)(h.guarded(x))
            assert torch.equal(out, x * 2)                       # the values are right: only the guards can tell
            with pytest.raises(AssertionError) as e:
                h.check_guards()
        msg = str(e.value)
        assert "4 guard byte(s) %s the empty_like (3, 4) float32 made by guarded_alloc_standin.py" % side in msg and "(scale2)" in msg, msg
        assert ("1 bytes before its start" in msg) if side == "in front of" else ("0 bytes past its end" in msg), msg


def test_an_unwritten_element_is_caught(standin):
    x = torch.arange(12.0).view(3, 4) + 1
    plain, runs = _three_runs(standin.skips_one, x, standin)
    (h0, ff), (h1, kb) = runs
    h0.check_guards()
    h1.check_guards()                                            # nothing was written outside
    assert not G.same_bits(ff, kb)                               # (the plain run proves nothing here: its element is whatever the allocator recycled)
    assert G.new_nans(ff, x * 2) == 1
    mask = torch.ones(3, 4, dtype=torch.bool)
    mask[2, 3] = False                                           # ... and exactly that element still holds the poison
    assert G.same_bits(ff, kb, mask) and G.holds_poison(ff, 0xFF, ~mask) and G.holds_poison(kb, 0x4B, ~mask) and not G.holds_poison(kb, 0x4B)


def test_a_workspace_slot_read_before_it_is_written_is_caught(standin):
    x = torch.arange(12.0).view(3, 4) + 1
    plain, runs = _three_runs(standin.reads_workspace_early, x, standin)
    (h0, ff), (h1, kb) = runs
    h0.check_guards()
    h1.check_guards()
    assert not G.same_bits(ff, kb)
    assert G.new_nans(ff, x * 2) == 1 and G.new_nans(kb, x * 2) == 0 and bool(torch.isfinite(kb).all())


def test_an_entry_that_writes_into_its_input_is_caught(standin):
    x = torch.arange(12.0).view(3, 4)
    with G.GuardedAlloc(0xFF, modules=[standin], guard_cpu=True) as h:
        gx, gy = h.guarded(x), h.guarded(x + 1)
        out = standin.scale2(gx)
        h.check_operands_unchanged()
        gy[1, 1] = float("nan")                                  # an in/out operand may change ...
        h.check_operands_unchanged(written=[gy, out])
        with pytest.raises(AssertionError, match=r"wrote into its input: operand \(3, 4\) float32 made by test_guarded_alloc_cpu.py"):
            h.check_operands_unchanged()                         # ... an input may not
        h.check_guards()


def test_same_bits_tells_nans_apart_and_respects_the_region():
    a = torch.tensor([1.0, float("nan"), 3.0])
    assert G.same_bits(a, a.clone()) and not torch.equal(a, a.clone())
    b = a.clone()
    b[2] = 4.0
    assert not G.same_bits(a, b) and G.same_bits(a, b, torch.tensor([True, True, False]))
    assert not G.same_bits(a, a.double()) and not G.same_bits(a, a[:2])
    assert G.same_bits(torch.tensor(2.5, dtype=torch.float64), torch.tensor(2.5, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------------------------ completeness
# Public functions of the wrapper modules that are NOT rows of tests/test_gpu_memory_contract.py.  The only admissible reason: the function
# launches no kernel.  A wrapper that launches one is never exempt.
_HOST = "launches no kernel: host arithmetic on python / numpy values"
_ASK = "launches no kernel: asks the library's dispatch or a *_workspace_size / shape predicate"
EXEMPT = {
    "ops.latency_entry": "launches no kernel: a decorator",
    "ops.latency_launches": "launches no kernel: reads a switch",
    "ops.conv_kernel_name": _ASK,
    "ops.covers": _ASK,
    "ops.wgrad_covers": _ASK,
    "ops.conv_out_hw": _HOST,
    "ops.pair_eligible": _ASK,
    "ops.tail_eligible": _ASK,
    "ops.small_batch_splitk": _ASK,
    "ops.select": _ASK,
    "ops.items_tensor": "launches no kernel: builds two small index tensors from a python list",
    "ops_train.gru_gates_nhwc_ok": _ASK,
    "ops_train.seg_loss_shape_ok": _ASK,
    "ops_post.assign_targets_sparse_keys": "launches no kernel: copies a result to the host and reshapes it",
    "ops_seg.seg_grid": _HOST,
    "ops_seg.pad_box_lists": _HOST,
    "ops_seg.median_frequency_weights": _HOST,
    "ops_lidar.ring_table": _HOST,
    "ops_lidar.sensor_rows": _HOST,
    "ops_lidar.box_rows": _HOST,
    "ops_lidar.az_time_table": _HOST,
}


def public_functions():
    """'module.function' of every public function DEFINED in one of the six wrapper modules (re-exports are counted where they are defined)."""
    names = []
    for m in G.wrapper_modules():
        short = m.__name__.rsplit(".", 1)[1]
        for k, v in sorted(vars(m).items()):
            if k.startswith("_") or isinstance(v, type) or not callable(v):
                continue
            if getattr(v, "__module__", None) == m.__name__:
                names.append("%s.%s" % (short, k))
    return names


def test_every_wrapper_is_a_row_or_exempt():
    import test_gpu_memory_contract as T                         # imports without a GPU
    public = public_functions()
    assert len(public) >= 70 and "ops.conv2d" in public and "ops_track.sort_step" in public and "ops.wgrad_covers" in public, public
    covered = set()
    for row in T.ROWS:
        assert row.covers and row.cases, row.name
        covered.update(row.covers)
    assert not covered & set(EXEMPT), "both a row and exempt: %s" % sorted(covered & set(EXEMPT))
    assert all(reason.startswith("launches no kernel") for reason in EXEMPT.values())
    unknown = (covered - {"train.optim.HipAdam.step"} | set(EXEMPT)) - set(public)
    assert not unknown, "names that are not public functions of the wrapper modules: %s" % sorted(unknown)
    missing = [f for f in public if f not in covered and f not in EXEMPT]
    assert not missing, "neither a row of the memory-contract table nor exempt: %s" % missing
    assert "train.optim.HipAdam.step" in covered
    # the wrappers that already have partial guards elsewhere are rows all the same
    for f in ("ops_lidar.lidar_cast", "ops_lidar.lidar_cast_moving", "ops_post.det_map", "ops.conv2d", "ops.run_layer"):
        assert f in covered, f
    print("memory contract: %d of the %d public functions of the wrapper modules launch kernels and are rows; %d launch nothing" % (
        len(covered & set(public)), len(public), len(EXEMPT)))

"""Poisoned, guarded allocations for the wrapper modules (ops.py, ops_train.py, ops_post.py, ops_seg.py, ops_track.py, ops_lidar.py).

    with GuardedAlloc(0xFF) as h:
        x = h.guarded(x)                    # an input or in/out operand: copied between two guards
        out = ops.some_entry(x)             # its torch.empty / empty_like / zeros / full calls are served from poisoned, guarded buffers
        h.check_guards()                    # no byte before or behind any of those tensors changed

While the block is active the name `torch` inside the wrapper modules is a forwarding proxy: everything but the four allocation calls goes
to the real module, nothing is changed in torch itself or in _launch.py.  A device allocation is a contiguous view of the requested shape
and dtype in the middle of a larger uint8 buffer with at least GUARD bytes in front and behind; buffer and view are filled with ONE poison
byte first, zeros / full then write their fill into the view (what the wrapper clears for the kernel is part of what is tested), empty /
empty_like leave the poison.  The two poison bytes: 0xFF reads as NaN in bf16 / fp32 / fp64 and as -1 / 255 in the integer types, 0x4B as
a large finite float (fp32: 1.3e7) and a large positive integer -- an element a kernel never wrote differs between the two runs, a
workspace slot read before it was written makes the outputs differ or NaN.  No knowledge of any kernel is needed.

tests/test_guarded_alloc_cpu.py proves the harness on CPU stand-ins (guard_cpu=True, for that file only); tests/test_gpu_memory_contract.py
runs every kernel-launching wrapper through it."""
import importlib
import sys

import torch as _torch

GUARD = 4096                      # a multiple of 256: the view keeps the alignment the kernels assume
ALIGN = 256
POISONS = (0xFF, 0x4B)
WRAPPER_MODULES = ("ops", "ops_train", "ops_post", "ops_seg", "ops_track", "ops_lidar")


def wrapper_modules():
    """The six wrapper modules, imported (no GPU needed)."""
    return [importlib.import_module("v2x_sim_amd." + m) for m in WRAPPER_MODULES]


class Record:
    """One guarded allocation: `buffer` (uint8, poison in front of and behind `view`), who made it, and whether the view was left poisoned."""

    __slots__ = ("buffer", "view", "front", "nbytes", "call", "kind", "poisoned", "fill", "before")

    def __init__(self, buffer, view, front, nbytes, call, kind, poisoned, fill=None):
        self.buffer, self.view, self.front, self.nbytes, self.call, self.kind, self.poisoned, self.fill = buffer, view, front, nbytes, call, kind, poisoned, fill
        self.before = None          # operands: a copy of what guarded() put there

    def describe(self):
        return "%s %s %s made by %s" % (self.kind, tuple(self.view.shape), str(self.view.dtype).replace("torch.", ""), self.call)


def _shape_of(size):
    if len(size) == 1 and not isinstance(size[0], int):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


def _caller(depth):
    f = sys._getframe(depth)
    return "%s:%d (%s)" % (f.f_code.co_filename.replace("\\", "/").rsplit("/", 1)[-1], f.f_lineno, f.f_code.co_name)


class _TorchProxy:
    """Stands where a wrapper module's global `torch` stood: empty / empty_like / zeros / full are the harness's, the rest is torch's."""

    def __init__(self, harness):
        object.__setattr__(self, "_h", harness)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("the guarded-allocation proxy is read-only")

    def empty(self, *size, **kw):
        return self._h._alloc("empty", _torch.empty, size, kw, None, False)

    def zeros(self, *size, **kw):
        return self._h._alloc("zeros", _torch.zeros, size, kw, 0, False)

    def full(self, size, fill_value, **kw):
        return self._h._alloc("full", _torch.full, (size, fill_value), kw, fill_value, True)

    def empty_like(self, t, **kw):
        kw2 = {"dtype": kw.get("dtype") or t.dtype, "device": kw.get("device") or t.device}
        if set(kw) - {"dtype", "device"} or not self._h._guards(kw2["device"]):
            return _torch.empty_like(t, **kw)           # a CPU tensor, or a layout / memory_format request (none of the wrappers makes one)
        return self._h._alloc("empty_like", None, (tuple(t.shape),), kw2, None, False)


class GuardedAlloc:
    """Context manager: see the module docstring.  poison: the byte; modules: the modules whose `torch` is replaced (default: the six wrapper
    modules); guard_cpu: guard CPU allocations too (tests/test_guarded_alloc_cpu.py only -- CPU allocations otherwise pass through)."""

    def __init__(self, poison, modules=None, guard_cpu=False):
        if not 0 <= int(poison) <= 255:
            raise ValueError("the poison is one byte")
        self.poison, self.guard_cpu = int(poison), bool(guard_cpu)
        self.modules = list(modules) if modules is not None else None
        self.records = []
        self.proxy = _TorchProxy(self)
        self._saved = None

    # ---- installing / restoring -------------------------------------------------------------------------------------------------------
    def __enter__(self):
        if self._saved is not None:
            raise RuntimeError("GuardedAlloc is not re-entrant")
        mods = self.modules if self.modules is not None else wrapper_modules()
        saved = []
        try:
            for m in mods:
                real = m.__dict__["torch"]
                if real is not _torch:
                    raise RuntimeError("%s.torch is already replaced" % m.__name__)
                saved.append((m, real))
                setattr(m, "torch", self.proxy)
        except BaseException:
            for m, real in saved:
                setattr(m, "torch", real)
            raise
        self._saved = saved
        return self

    def __exit__(self, *exc):
        for m, real in self._saved:
            setattr(m, "torch", real)
        self._saved = None
        return False

    # ---- allocating -------------------------------------------------------------------------------------------------------------------
    def _guards(self, device):
        dev = _torch.device(device) if device is not None else _torch.device("cpu")
        return dev.type != "cpu" or self.guard_cpu

    def _place(self, shape, dtype, device, call, kind, poisoned):
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * _torch.empty((), dtype=dtype).element_size()
        buf = _torch.full((GUARD + ALIGN + nbytes + GUARD,), self.poison, dtype=_torch.uint8, device=device)
        front = GUARD + (-(buf.data_ptr() + GUARD)) % ALIGN
        view = buf[front:front + nbytes].view(dtype).view(shape)
        rec = Record(buf, view, front, nbytes, call, kind, poisoned)
        self.records.append(rec)
        return rec

    def _alloc(self, kind, real, args, kw, fill, full):
        device, dtype = kw.get("device"), kw.get("dtype")
        if not self._guards(device) or set(kw) - {"device", "dtype"}:
            return real(*args, **kw)
        shape = _shape_of((args[0],) if full else args)
        if dtype is None:
            dtype = _torch.get_default_dtype() if not full else _torch.full((), fill).dtype
        rec = self._place(shape, dtype, device, _caller(3), kind, fill is None)
        if fill is not None:
            rec.fill = fill
            rec.view.fill_(fill)
        return rec.view

    def empty(self, shape, dtype, device):
        """A poisoned, guarded tensor for an output the CALLER hands to an entry (out=...): what torch.empty is in a plain run."""
        return self._place(tuple(shape), dtype, device, _caller(2), "caller's empty", True).view

    def guarded(self, t):
        """A copy of the input or in/out operand t between two guards (None stays None): an over-read picks up poison, a store outside is seen."""
        if t is None:
            return None
        if not self._guards(t.device):
            return t
        rec = self._place(tuple(t.shape), t.dtype, t.device, _caller(2), "operand", False)
        rec.view.copy_(t.detach())
        rec.before = rec.view.clone()
        return rec.view

    # ---- checking ---------------------------------------------------------------------------------------------------------------------
    def record_of(self, view):
        """The record whose view starts where `view` starts."""
        for r in self.records:
            if r.view is view:
                return r
        for r in self.records:
            if view.numel() and r.view.data_ptr() == view.data_ptr() and r.view.shape == view.shape and r.view.dtype == view.dtype:
                return r
        raise KeyError("no guarded allocation holds this tensor")

    def check_operands_unchanged(self, written=()):
        """Every operand placed with guarded() still holds the bits it was given -- except the in/out operands listed in `written`."""
        skip = {t.data_ptr() for t in written if t.numel()}
        bad = [r.describe() for r in self.records if r.before is not None and r.view.data_ptr() not in skip and not same_bits(r.view, r.before)]
        assert not bad, "an entry wrote into its input: " + "; ".join(bad)

    def check_guards(self):
        """Every guard byte of every record still holds the poison byte; the failure names the allocation."""
        bad = []
        for r in self.records:
            for side, g in (("in front of", r.buffer[:r.front]), ("behind", r.buffer[r.front + r.nbytes:])):
                wrong = g != self.poison
                if bool(wrong.any()):
                    at = wrong.nonzero().flatten()
                    where = "%d bytes before its start" % (r.front - int(at[-1])) if side == "in front of" else "%d bytes past its end" % int(at[0])
                    bad.append("%d guard byte(s) %s the %s were overwritten (the nearest %s)" % (int(at.numel()), side, r.describe(), where))
        assert not bad, "; ".join(bad)


class PlainAlloc:
    """GuardedAlloc's interface with today's allocations: the plain run of a three-run comparison."""
    poison, records = None, ()

    def guarded(self, t):
        return t

    def empty(self, shape, dtype, device):
        return _torch.empty(tuple(shape), dtype=dtype, device=device)

    def check_operands_unchanged(self, written=()):
        """Every operand placed with guarded() still holds the bits it was given -- except the in/out operands listed in `written`."""
        skip = {t.data_ptr() for t in written if t.numel()}
        bad = [r.describe() for r in self.records if r.before is not None and r.view.data_ptr() not in skip and not same_bits(r.view, r.before)]
        assert not bad, "an entry wrote into its input: " + "; ".join(bad)

    def check_guards(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


# ---- bit-level comparisons (NaN-proof) ------------------------------------------------------------------------------------------------
_INT_OF_SIZE = {1: _torch.uint8, 2: _torch.int16, 4: _torch.int32, 8: _torch.int64}


def as_int(t):
    """t's elements as integers of the same width: equality of bits, also where the value is a NaN."""
    t = t.contiguous()
    if t.dtype in (_torch.uint8, _torch.int16, _torch.int32, _torch.int64):
        return t
    return t.view(_INT_OF_SIZE[t.element_size()])


def same_bits(a, b, mask=None):
    """a and b (same shape, same dtype) agree bit for bit -- where mask (a boolean tensor of their shape) is True, or everywhere."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    ia, ib = as_int(a), as_int(b)
    if mask is not None:
        ia, ib = ia[mask], ib[mask]
    return bool(_torch.equal(ia, ib))


def holds_poison(t, poison, mask=None):
    """Every byte of t's elements (of those where mask is True) is the poison byte."""
    by = t.contiguous().reshape(-1).view(_torch.uint8).reshape(t.numel(), t.element_size())
    if mask is not None:
        by = by[mask.reshape(-1)]
    return bool((by == poison).all())


def new_nans(got, plain, mask=None):
    """How many elements of `got` are NaN where `plain` is not (floating types; 0 for the others)."""
    if not got.is_floating_point():
        return 0
    n = _torch.isnan(got) & ~_torch.isnan(plain)
    if mask is not None:
        n = n & mask
    return int(n.sum())

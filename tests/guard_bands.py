"""Guard bands: a call's result must not depend on memory outside its operands, and the call must leave that memory alone.

A banded tensor sits in the middle of ONE larger allocation; the two margins (the bands, 1 MiB each - more than one tile of any kernel
here: 256 positions x 512 channels x 4 bytes = 512 KiB) are filled bytewise and compared bytewise afterwards.  A kernel that strays by up
to a tile therefore lands in a band of the same allocation, never in a foreign one: nothing here can fault that cannot fault without
the bands.  The view starts 1 MiB (a multiple of 4 KiB) into the allocation, so it keeps the alignment the caching allocator gives, which
is all a kernel may assume.

Fill values.  POISON (byte 0xFF) is a NaN in fp32, bf16 and f16 and "active" in a u8 site mask: a read past an operand that reaches a
result shows in the result.  ZERO (byte 0x00) is the second fill: a result that differs between the two runs depends on memory outside
its operands.  Tensors a kernel uses as INDICES (int32 / int64: row lists, tokens, labels, pooling maps, Adam's segment table) always get
zero bands, whatever fill was asked for - a stray read there must never become a wild address.  For those tensors the write check
therefore only catches NON-ZERO stray writes.

`guarded_ops(fill)` extends the bands to what tricolo_amd.ops allocates itself: inside the context the name `torch` in the namespace of
tricolo_amd.ops is a thin proxy whose device-tensor allocators (empty / zeros / full / empty_like / zeros_like) return banded views and
enter them in a ledger; ops._workspace and WgradBatch.slab hand out banded buffers of exactly the byte count asked for (the library's
max(nbytes, 1 MiB) and its 16 MiB arenas would hide a kernel that uses more than the planner granted); the library handle records the
tri_* entry points launched.  On exit: torch.cuda.synchronize(), then every band of the ledger and every band the test registered is
checked; damage raises GuardBandError."""
import contextlib
import functools
import os
import re

import torch

BAND = 1 << 20
ALIGN = 4096
POISON, ZERO = 0xFF, 0x00
INDEX_DTYPES = (torch.int32, torch.int64)
ALLOCATORS = ("empty", "zeros", "full", "empty_like", "zeros_like")
assert BAND % ALIGN == 0


class Band:
    """One banded allocation: parent (u8, BAND + nbytes + BAND), the fill its bands hold, and what the view looks like."""
    __slots__ = ("parent", "nbytes", "fill", "shape", "dtype", "origin")

    def __init__(self, parent, nbytes, fill, shape, dtype, origin):
        self.parent, self.nbytes, self.fill, self.shape, self.dtype, self.origin = parent, nbytes, fill, tuple(shape), dtype, origin

    def damage(self):
        """[(side, offset)]: first damaged byte of each band; offset counts bytes from the START of the view (negative: in front)."""
        out = []
        for side, lo, hi in (("before", 0, BAND), ("after", BAND + self.nbytes, 2 * BAND + self.nbytes)):
            bad = self.parent[lo:hi] != self.fill
            if bool(bad.any()):
                out.append((side, lo + int(bad.nonzero()[0, 0]) - BAND))
        return out


class GuardBandError(AssertionError):
    def __init__(self, records):
        self.records = records                       # [dict(shape, dtype, side, offset, origin, launched)]
        lines = [f"{r['origin']} {r['shape']} {r['dtype']}: band {r['side']} the tensor damaged, first at byte offset {r['offset']} "
                 f"from its start; entry points launched: {', '.join(r['launched']) or '(none)'}" for r in records]
        super().__init__("guard band damaged\n  " + "\n  ".join(lines))


def band_fill(dtype, fill):
    """The byte a tensor of `dtype` gets in its bands when `fill` was asked for: index tensors always zeros (module docstring)."""
    return ZERO if dtype in INDEX_DTYPES else fill


def _alloc(shape, dtype, device, fill, origin, real=torch):
    if isinstance(shape, int):
        shape = (shape,)
    shape = tuple(int(s) for s in shape)
    n = 1
    for s in shape:
        n *= s
    nbytes = n * real.empty((), dtype=dtype).element_size()
    fill = band_fill(dtype, fill)
    parent = real.empty((2 * BAND + nbytes,), dtype=real.uint8, device=device)
    parent.fill_(fill)                               # the interior too: what a kernel leaves unwritten differs between the two fills
    view = parent[BAND:BAND + nbytes].view(dtype).view(shape)
    view._band = Band(parent, nbytes, fill, shape, dtype, origin)
    return view


def banded(t, fill, device=None, origin="input"):
    """A contiguous copy of t (on `device`, default t's) in the middle of one larger allocation whose margins hold `fill` bytes."""
    view = _alloc(t.shape, t.dtype, t.device if device is None else device, fill, origin)
    view.copy_(t)
    return view


@functools.lru_cache(maxsize=1)
def stream_entry_points():
    """Names of the entry points include/tricolo_hip.h declares with `void* stream` as their last parameter: the ones that put work on
    the GPU.  Size and plan queries take no stream (and no device memory)."""
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tricolo_hip.h")
    with open(header) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    decls = re.findall(r"\b(tri_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    return frozenset(name for name, params in decls if re.search(r"void\s*\*\s*stream\s*$", params.strip()))


class RecordingLib:
    """Stands in for the ctypes library handle (tricolo_amd._C._lib, as _C._TimedLib does): notes every tri_* entry point that takes
    arguments - launches and size / plan queries alike; `launches()` keeps the ones declared with a stream (stream_entry_points).
    The one render entry point serves every mode, so of each tri_raster_render call `raster_calls` keeps (fields, samples): the groups
    its descriptor declared (_C.TRI_MESH_*) and its sample count."""

    def __init__(self, real, signatures):
        self._real, self._sig, self.calls, self.raster_calls = real, signatures, [], []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        sig = self._sig.get(name)
        if sig is None or not name.startswith("tri_") or not sig[1]:
            return fn

        def recorded(*a):
            self.calls.append(name)
            if name == "tri_raster_render":                # (batch, cam, sumF, views, H, W, yfov, znear, samples, ...)
                self.raster_calls.append((int(a[0].fields), int(a[8])))
            return fn(*a)
        return recorded

    @staticmethod
    def is_query(name):
        return name not in stream_entry_points()

    def launches(self):
        seen = []
        for n in self.calls:
            if not self.is_query(n) and n not in seen:
                seen.append(n)
        return seen


@contextlib.contextmanager
def recording():
    """Install a RecordingLib as the library handle; yields it.  The real handle is back on exit, whatever happened inside."""
    from tricolo_amd import _C
    real = _C.lib()
    rec = RecordingLib(real, _C.SIGNATURES)
    _C._lib = rec
    try:
        yield rec
    finally:
        _C._lib = real


class TorchProxy:
    """`torch` as tricolo_amd.ops sees it inside guarded_ops: every attribute is the real module's, except the allocators of device
    tensors.  Host and pinned allocations pass through untouched."""

    def __init__(self, real, guard):
        self.__dict__["_real"], self.__dict__["_guard"] = real, guard

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _device(self, kw, like=None):
        dev = kw.get("device", like.device if like is not None else None)
        return None if dev is None else self._real.device(dev)

    def _passes(self, kw, dev):
        return dev is None or dev.type not in self._guard.device_types or kw.get("pin_memory") or kw.get("out") is not None

    @staticmethod
    def _size(size):
        return tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)

    def empty(self, *size, **kw):
        dev = self._device(kw)
        if self._passes(kw, dev):
            return self._real.empty(*size, **kw)
        return self._guard.alloc(self._size(size), kw.get("dtype") or self._real.get_default_dtype(), dev, "ops torch.empty")

    def zeros(self, *size, **kw):
        dev = self._device(kw)
        if self._passes(kw, dev):
            return self._real.zeros(*size, **kw)
        return self._guard.alloc(self._size(size), kw.get("dtype") or self._real.get_default_dtype(), dev, "ops torch.zeros").zero_()

    def full(self, size, fill_value, **kw):
        dev = self._device(kw)
        if self._passes(kw, dev):
            return self._real.full(size, fill_value, **kw)
        dtype = kw.get("dtype") or self._real.full((), fill_value).dtype
        return self._guard.alloc(self._size((size,)), dtype, dev, "ops torch.full").fill_(fill_value)

    def empty_like(self, t, **kw):
        dev = self._device(kw, like=t)
        if self._passes(kw, dev):
            return self._real.empty_like(t, **kw)
        return self._guard.alloc(t.shape, kw.get("dtype") or t.dtype, dev, "ops torch.empty_like")

    def zeros_like(self, t, **kw):
        dev = self._device(kw, like=t)
        if self._passes(kw, dev):
            return self._real.zeros_like(t, **kw)
        return self._guard.alloc(t.shape, kw.get("dtype") or t.dtype, dev, "ops torch.zeros_like").zero_()


class Guard:
    """What guarded_ops yields: the ledger, the fill, put() for the test's own operands, and the recorded entry points."""

    def __init__(self, fill, device, device_types):
        self.fill, self.device, self.device_types = fill, device, tuple(device_types)
        self.ledger, self.lib = [], None

    def alloc(self, shape, dtype, device, origin):
        view = _alloc(shape, dtype, device, self.fill, origin)
        self.ledger.append(view._band)
        return view

    def register(self, view):
        """Enter a tensor made by banded() in the ledger; returns it."""
        self.ledger.append(view._band)
        return view

    def put(self, t, origin="input"):
        """banded copy of t on the guard's device, registered (None stays None)."""
        return None if t is None else self.register(banded(t, self.fill, device=self.device, origin=origin))

    @property
    def launched(self):
        return self.lib.launches() if self.lib is not None else []

    @property
    def raster_calls(self):
        """[(fields, samples)] of the tri_raster_render calls made so far (RecordingLib)."""
        return list(self.lib.raster_calls) if self.lib is not None else []

    def check(self):
        bad = []
        for b in self.ledger:
            for side, off in b.damage():
                bad.append(dict(shape=b.shape, dtype=b.dtype, side=side, offset=off, origin=b.origin, launched=self.launched))
        if bad:
            raise GuardBandError(bad)


@contextlib.contextmanager
def guarded_ops(fill, device="cuda", device_types=("cuda",), record=True):
    """See the module docstring.  device: where put() places operands; device_types: which device types the proxy bands (the CPU
    self-tests pass "cpu")."""
    from tricolo_amd import ops
    guard = Guard(fill, device, device_types)
    real_torch, real_ws, real_slab = ops.torch, ops._workspace, ops.WgradBatch.slab
    on_gpu = "cuda" in guard.device_types and real_torch.cuda.is_available()

    def workspace(nbytes, device):
        return guard.alloc((int(nbytes),), real_torch.uint8, device, "ops._workspace")

    def slab(self, nbytes):
        return guard.alloc(((int(nbytes) + 255) // 256 * 256,), real_torch.uint8, self.device, "WgradBatch.slab")

    def drop_caches():
        ops._wgrad_ws.clear()
        ops.WgradBatch.release()

    rec = recording() if record else contextlib.nullcontext()
    drop_caches()
    ops.torch, ops._workspace, ops.WgradBatch.slab = TorchProxy(real_torch, guard), workspace, slab
    try:
        with rec as lib:
            guard.lib = lib
            yield guard
            if on_gpu:
                real_torch.cuda.synchronize()
    finally:
        ops.torch, ops._workspace, ops.WgradBatch.slab = real_torch, real_ws, real_slab
        drop_caches()
    guard.check()


def same_bytes(a, b):
    """Bit identity of two tensors (NaN != NaN, so values cannot be compared)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))

"""A guarded arena: device buffers of EXACTLY the documented size, with guard words around them (test helper only).

Every GPU test reaches the kernels through ``fused.py`` / ``ops.py``, which size each buffer by the header's size functions and
allocate it with ``torch.empty`` / ``torch.zeros``.  The caching allocator rounds every request up to 512 bytes and packs small
buffers side by side, so a tile that stores its tail rows past ``logits[B]``, or a size function a few hundred bytes short of
what a kernel writes, lands in slack or in a neighbour and no value test notices.  Here the same requests are carved out of one
``uint8`` tensor filled with a guard pattern:

* ``GuardedArena.take(shape, dtype)`` returns a tensor of exactly ``prod(shape) * itemsize`` bytes whose body starts at an
  offset that is 256 mod 512 - 256 is what include/pcgnn.h promises for workspaces, 512 is what torch gives and would hide any
  reliance on more - with a band of at least 4 KiB and at least 16 rows of the buffer's own row pitch (one dense tile's worth,
  rounded up to 256) before and after it.  Neighbouring bodies share the band between them (the wider of the two).
* ``GuardedArena.check(what)`` asserts that every byte of the WHOLE arena outside the bodies handed out still holds the
  pattern, and names the buffer the damage is nearest to, the side, and the first and last damaged byte relative to that
  buffer's END (0 = the first byte behind it; negative values below ``-nbytes`` lie in front of it).
* ``guarded_allocations(arena)`` patches ``torch.empty / zeros / full / empty_like / zeros_like`` for the duration of a ``with``
  block so that allocations on the arena's device come from the arena; everything else (other devices, ``requires_grad``,
  ``out=``, pinned or non-strided layouts, empty tensors) goes to the real function.  It logs every take.

The pattern is the 32-bit word 0x00000003: read as an int32 it is a small valid row index or count, as a float a denormal, so a
stray READ of a band cannot turn into a wild address.  The body of every take starts as ZERO, ``torch.empty`` included: the
arena never hands a body out twice, and pre-filling ``empty`` bodies with the pattern - which would also find reliance on
accidentally zero memory - is left out on purpose: a look-back or ticket word a kernel spins on would then start at 3.
(That is tests/dirty.py's job: ``torch.empty`` bodies and cached workspaces pre-filled, region by region as the header allows.)

A returned tensor has ``storage_offset() == 0`` and a storage of exactly its own bytes (it is re-imported through DLPack):
``fused.py`` takes parameter offsets from ``view.storage_offset()`` relative to ``theta``'s own storage.
"""
import contextlib
import math
import sys
from unittest import mock

import numpy as np
import torch

GUARD_WORD = 0x00000003
BAND_MIN, BAND_ROWS, BAND_ROUND = 4096, 16, 256
BODY_MOD, BODY_REM = 512, 256
_PATCHED = ("empty", "zeros", "full", "empty_like", "zeros_like")
_REAL = {name: getattr(torch, name) for name in _PATCHED}        # (the arena itself never goes through a patched name)


def _itemsize(dtype) -> int:
    return _REAL["empty"]((), dtype=dtype).element_size()


def _shape(size) -> tuple:
    if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


def band_bytes(shape, itemsize: int) -> int:
    """width of the guard band of a buffer: >= 4 KiB and >= 16 rows of its own row pitch (its last dimension), a multiple of 256"""
    pitch = (shape[-1] if len(shape) >= 2 else 1) * itemsize
    return -(-max(BAND_MIN, BAND_ROWS * pitch) // BAND_ROUND) * BAND_ROUND


class GuardedArena:
    def __init__(self, nbytes: int, device):
        self.device = torch.device(device)
        nbytes = -(-int(nbytes) // BODY_MOD) * BODY_MOD
        self.nbytes = nbytes
        word = np.array([GUARD_WORD], dtype="<u4").view(np.uint8)
        self.buf = _REAL["empty"](nbytes, dtype=torch.uint8, device=self.device)
        self.buf.view(-1, 4).copy_(torch.from_numpy(word.copy()).to(self.device))
        self._expect = self.buf.clone()
        if self.buf.data_ptr() % BODY_MOD:             # (torch gives 512 on the device, 64 on the host: offsets are then relative)
            self._skew = BODY_MOD - self.buf.data_ptr() % BODY_MOD
        else:
            self._skew = 0
        self.bodies = []                               # dicts: name, start, end, band, shape, dtype
        self.log = []                                  # (caller file:line, shape, dtype, bytes) of every take
        self._keep = []                                # the tensors handed out (a body is never reused)

    # ------------------------------------------------------------------
    def take(self, shape, dtype=torch.float32, zero: bool = False, name: str = None, fill=None) -> torch.Tensor:
        """A tensor of exactly prod(shape) * itemsize bytes inside the arena.  zero=True is ``torch.zeros``; a body starts as
        zero either way (see the module's docstring).  fill: ``torch.full``'s value."""
        shape = _shape((shape,) if isinstance(shape, int) else (tuple(shape),))
        size = _itemsize(dtype)
        nbytes = int(math.prod(shape)) * size
        if nbytes <= 0:
            raise ValueError("GuardedArena.take: an empty tensor has nothing to guard")
        band = band_bytes(shape, size)
        if self.bodies:
            lo = self.bodies[-1]["end"] + max(self.bodies[-1]["band"], band)
        else:
            lo = band
        # the first offset >= lo whose ADDRESS is 256 mod 512
        start = lo + (BODY_REM - (lo - self._skew)) % BODY_MOD
        end = start + nbytes
        if end + band > self.nbytes:
            raise MemoryError(f"GuardedArena of {self.nbytes} bytes is full: {nbytes} more bytes (+ {band} of band) asked at offset {start}")
        name = name or f"{_caller()} {list(shape)} {str(dtype).replace('torch.', '')}"
        self.bodies.append(dict(name=name, start=start, end=end, band=band, shape=shape, dtype=dtype))
        self.log.append((_caller(), shape, dtype, nbytes))
        body = self.buf[start:end]
        if fill is None:
            body.zero_()
        flat = body.view(dtype)
        if fill is not None:
            flat.fill_(fill)
        out = torch.from_dlpack(flat.view(shape).__dlpack__(stream=-1))        # aliases the arena: storage offset 0, nbytes of storage
        self._keep.append(out)
        return out

    def offset_of(self, t: torch.Tensor) -> int:
        """byte offset of a tensor's first byte inside the arena"""
        return t.data_ptr() - self.buf.data_ptr()

    # ------------------------------------------------------------------
    def damage(self):
        """[] if every byte outside the bodies holds the pattern; else one dict per (buffer, side) with damage nearest to it:
        name, side ("before" / "after"), first, last (byte offsets relative to the buffer's end), count"""
        bad = self.buf != self._expect
        for b in self.bodies:
            bad[b["start"]:b["end"]] = False
        if not bool(bad.any()):
            return []
        idx = bad.nonzero().flatten().cpu().numpy().astype(np.int64)
        if not self.bodies:
            return [dict(name="<the empty arena>", side="after", first=int(idx[0]), last=int(idx[-1]), count=int(idx.size))]
        starts = np.array([b["start"] for b in self.bodies], dtype=np.int64)
        ends = np.array([b["end"] for b in self.bodies], dtype=np.int64)
        mids = (ends[:-1] + starts[1:] + 1) // 2        # damage in [mid, ...) is nearer to the next buffer
        owner = np.searchsorted(mids, idx, side="right")
        out = []
        for o in np.unique(owner):
            mine = idx[owner == o]
            for side, sel in (("before", mine < starts[o]), ("after", mine >= ends[o])):
                if sel.any():
                    hit = mine[sel] - ends[o]
                    out.append(dict(name=self.bodies[o]["name"], side=side, first=int(hit[0]), last=int(hit[-1]), count=int(hit.size)))
        return out

    def check(self, what: str = ""):
        """assert that the whole arena outside the bodies handed out still holds the guard pattern"""
        found = self.damage()
        if found:
            lines = [f"{d['count']} damaged byte(s) {d['side']} {d['name']}: first at end{d['first']:+d}, last at end{d['last']:+d}"
                     for d in found]
            raise AssertionError(f"guard words overwritten{' after ' + what if what else ''}:\n  " + "\n  ".join(lines))

    def table(self):
        """the log as text lines: bytes, shape, dtype, caller"""
        return [f"{n:>12d}  {str(list(s)):<22s} {str(d).replace('torch.', ''):<8s} {c}" for c, s, d, n in self.log]


def _caller() -> str:
    """file:line of the nearest frame outside this module and unittest.mock"""
    f = sys._getframe(1)
    while f is not None and (f.f_code.co_filename == __file__ or "unittest" in f.f_code.co_filename):
        f = f.f_back
    if f is None:
        return "?"
    name = f.f_code.co_filename.replace("\\", "/").split("/")[-1]
    return f"{name}:{f.f_lineno}"


def _on_arena(arena: GuardedArena, device) -> bool:
    if device is None:
        dev = torch.get_default_device() if hasattr(torch, "get_default_device") else torch.device("cpu")
    else:
        dev = torch.device(device)
    if dev.type != arena.device.type:
        return False
    if dev.type == "cpu":
        return True
    if torch.cuda.is_current_stream_capturing():        # (a take zeroes its body: not a launch to record into somebody's graph)
        return False
    want = arena.device.index if arena.device.index is not None else torch.cuda.current_device()
    have = dev.index if dev.index is not None else torch.cuda.current_device()
    return want == have


_PLAIN = {"dtype", "device", "requires_grad", "layout", "pin_memory", "memory_format"}


# (tests/dirty.py imports _plain: what goes to the real function here goes to it there too - keep the two in step)
def _plain(kw: dict, contiguous_input: bool = True) -> bool:
    """only what a plain dense allocation says: anything else (out=, names=, requires_grad, pinned, sparse, channels-last) goes
    to the real function"""
    if set(kw) - _PLAIN or kw.get("requires_grad") or kw.get("pin_memory"):
        return False
    if kw.get("layout") not in (None, torch.strided):
        return False
    fmt = kw.get("memory_format")
    return fmt in (None, torch.contiguous_format) or (fmt == torch.preserve_format and contiguous_input)


@contextlib.contextmanager
def guarded_allocations(arena: GuardedArena):
    """While active, torch.empty / zeros / full / empty_like / zeros_like on the arena's device return ``arena.take(...)``
    (``zeros``: a zeroed body; ``empty``: the body as the arena holds it - zero, see above).  Yields ``arena.log``.  The
    originals are back on exit, also on an exception.  Patch inside a test, never at import time."""

    def sized(name, zero):
        def fn(*size, **kw):
            if not size or not _plain(kw) or not _on_arena(arena, kw.get("device")):
                return _REAL[name](*size, **kw)
            shape = _shape(size)
            dtype = kw.get("dtype") or torch.get_default_dtype()
            if math.prod(shape) == 0:
                return _REAL[name](*size, **kw)
            return arena.take(shape, dtype, zero=zero)
        return fn

    def full(size, fill_value, **kw):
        if not _plain(kw) or not _on_arena(arena, kw.get("device")) or isinstance(fill_value, (complex, torch.Tensor)):
            return _REAL["full"](size, fill_value, **kw)
        shape = _shape((size,))
        dtype = kw.get("dtype")
        if dtype is None:
            dtype = torch.bool if isinstance(fill_value, bool) else torch.int64 if isinstance(fill_value, int) else torch.get_default_dtype()
        if math.prod(shape) == 0:
            return _REAL["full"](size, fill_value, **kw)
        return arena.take(shape, dtype, fill=fill_value)

    def like(name, zero):
        def fn(inp, **kw):
            dev = kw.get("device") or inp.device
            if (not _plain(kw, inp.is_contiguous()) or not _on_arena(arena, dev) or inp.numel() == 0 or inp.layout != torch.strided
                    or not inp.is_contiguous()):
                return _REAL[name](inp, **kw)
            return arena.take(tuple(inp.shape), kw.get("dtype") or inp.dtype, zero=zero)
        return fn

    new = dict(empty=sized("empty", False), zeros=sized("zeros", True), full=full,
               empty_like=like("empty_like", False), zeros_like=like("zeros_like", True))
    with contextlib.ExitStack() as stack:
        for name in _PATCHED:
            stack.enter_context(mock.patch.object(torch, name, new[name]))
        yield arena.log

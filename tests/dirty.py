"""Dirty memory: ``torch.empty`` bodies and cached workspaces that start from a chosen bit pattern (test helper only).

A sibling of ``tests/guarded.py``.  That arena controls WHERE a buffer lies and hands every body out as zero; this module
controls WHAT a buffer holds when a call begins.  ``fused._alloc``, ``wholeset.py``, ``baseline.py`` and ``ops.py`` take their
workspaces and outputs from ``torch.empty``: in a test those are mostly fresh pages that read as zero, in a long-lived process
they are recycled blocks holding another call's plans, look-back tags, tickets and partial sums.  include/pcgnn.h promises "no
initial contents required" for them; ``test_gpu_dirty_memory.py`` runs the calls on such memory (its docstring says which part
of that promise a test can see and which it cannot).

* ``dirty_allocations(fill, int_fill=None, device="cuda")`` patches ``torch.empty`` and ``torch.empty_like`` inside a ``with``
  block: a plain allocation on ``device`` comes back pre-filled, and ``(caller, shape, dtype, bytes)`` is appended to the log
  the block yields.  ``torch.zeros`` and ``torch.full`` are left alone.  What ``guarded_allocations`` passes through to the
  real function is passed through here too (``out=``, pinned memory, ``requires_grad``, non-strided layouts, empty tensors,
  other devices, a stream that is capturing); a pass-through that did produce bytes on ``device`` is listed in
  ``log.unfilled`` so that a test can assert that there was none.
* ``dirty_(tensor, fill)`` overwrites every byte of an existing contiguous buffer, whatever its dtype: for the cached
  workspaces (``engine._inf["ws"]``, the baseline engine's ``inf["ws"]`` / ``inf["train_ws"]``, ``ops._eval_cache``).

A fill is four bytes, repeated from the buffer's first byte:

* ``WORD3``  the 32-bit word 0x00000003, ``guarded``'s pattern: a valid small index, a denormal float, and a value a look-back
  tag or a ticket really takes.
* ``A5``     bytes 0xA5: a large negative int32, a float of about -2.9e-16.
* ``NAN``    the float32 quiet NaN 0x7FC00000.  ONLY for buffers that hold nothing but floats; never for a region a kernel
  reads an index or a count from (as an int32 it is 2143289344).

``int_fill`` is what buffers of an integer or bool dtype get instead of ``fill``: another four-byte fill, or a Python int
stored by VALUE in the buffer's own dtype (-7 in the output tests: no valid id, count or label).
"""
import contextlib
import sys
from unittest import mock

import numpy as np
import torch

from tests.guarded import _plain

WORD3 = bytes((0x03, 0x00, 0x00, 0x00))
A5 = bytes((0xA5,) * 4)
NAN = bytes((0x00, 0x00, 0xC0, 0x7F))
FILLS = {"WORD3": WORD3, "A5": A5, "NAN": NAN}

_PATCHED = ("empty", "empty_like")
_REAL = {name: getattr(torch, name) for name in _PATCHED}


def _caller() -> str:
    """file:line of the nearest frame outside this module and unittest.mock"""
    f = sys._getframe(1)
    while f is not None and (f.f_code.co_filename == __file__ or "unittest" in f.f_code.co_filename):
        f = f.f_back
    if f is None:
        return "?"
    return f"{f.f_code.co_filename.replace(chr(92), '/').split('/')[-1]}:{f.f_lineno}"


def _pattern(fill) -> bytes:
    fill = bytes(fill)
    if len(fill) != 4:
        raise ValueError("a fill is four bytes")
    return fill


def dirty_(t: torch.Tensor, fill) -> torch.Tensor:
    """Overwrite EVERY byte of ``t`` (contiguous, any dtype) with the four-byte ``fill`` repeated from its first byte; a
    Python int is stored by value instead (integer dtypes).  Returns ``t``: same object, same storage."""
    if not t.is_contiguous():
        raise ValueError("dirty_: the buffer must be contiguous")
    if t.numel() == 0:
        return t
    if isinstance(fill, int) and not isinstance(fill, bool):
        if t.dtype.is_floating_point:
            raise ValueError("dirty_: an int fill is for integer buffers")
        t.fill_(fill % 256 if t.dtype == torch.uint8 else fill)          # (uint8 takes the value's low byte)
        return t
    pat = _pattern(fill)
    flat = t.view(-1).view(torch.uint8)                  # (a 0-d tensor has no last dimension to re-view)
    n = flat.numel()
    src = torch.from_numpy(np.frombuffer(pat, dtype=np.uint8).copy()).to(t.device)
    whole = n // 4 * 4
    if whole:
        flat[:whole].view(-1, 4).copy_(src)
    if n - whole:
        flat[whole:].copy_(src[:n - whole])
    return t


def holds(t: torch.Tensor, fill) -> torch.Tensor:
    """bool tensor of ``t``'s shape: which ELEMENTS still hold the fill in every byte (the buffer's first byte is phase 0)"""
    want = dirty_(_REAL["empty_like"](t.contiguous()), fill)
    size = t.element_size()
    same = t.contiguous().view(-1).view(torch.uint8) == want.view(-1).view(torch.uint8)
    return same.view(-1, size).all(dim=1).view(t.shape)


class DirtyLog(list):
    """(caller, shape, dtype, bytes) of every allocation filled; ``unfilled``: the same for allocations on the device that
    went to the real function with bytes in them"""

    def __init__(self):
        super().__init__()
        self.unfilled = []

    def table(self):
        return [f"{n:>12d}  {str(list(s)):<22s} {str(d).replace('torch.', ''):<8s} {c}" for c, s, d, n in self]


def _on_device(device: torch.device, asked) -> bool:
    if asked is None:
        dev = torch.get_default_device() if hasattr(torch, "get_default_device") else torch.device("cpu")
    else:
        dev = torch.device(asked)
    if dev.type != device.type:
        return False
    if dev.type != "cuda" or device.index is None:
        return True
    return (dev.index if dev.index is not None else torch.cuda.current_device()) == device.index


@contextlib.contextmanager
def dirty_allocations(fill, int_fill=None, device="cuda"):
    """While active, plain ``torch.empty`` / ``torch.empty_like`` allocations on ``device`` come back filled: with ``fill``,
    or with ``int_fill`` (if given) where the dtype is an integer or bool one.  Yields the ``DirtyLog``.  The originals are
    back on exit, also on an exception.  Patch inside a test, never at import time."""
    device = torch.device(device)
    log = DirtyLog()
    _pattern(fill)

    def finish(t, plain):
        if t.numel() == 0 or t.layout != torch.strided or not _on_device(device, t.device):
            return t
        entry = (_caller(), tuple(t.shape), t.dtype, t.numel() * t.element_size())
        if not plain or not t.is_contiguous() or (t.device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            log.unfilled.append(entry)                   # (a fill is a launch: not one to record into somebody's graph)
            return t
        use = fill if int_fill is None or t.dtype.is_floating_point or t.dtype.is_complex else int_fill
        dirty_(t, use)
        log.append(entry)
        return t

    def empty(*size, **kw):
        t = _REAL["empty"](*size, **kw)
        if "out" in kw:                                  # (the caller's own tensor, not an allocation)
            return t
        return finish(t, bool(size) and _plain(kw))

    def empty_like(inp, **kw):
        t = _REAL["empty_like"](inp, **kw)
        return finish(t, _plain(kw, inp.is_contiguous()))

    new = dict(empty=empty, empty_like=empty_like)
    with contextlib.ExitStack() as stack:
        for name in _PATCHED:
            stack.enter_context(mock.patch.object(torch, name, new[name]))
        yield log

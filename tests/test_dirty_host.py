"""tests/dirty.py on CPU tensors: the patch fills and logs, ``zeros`` / ``full`` stay what they are, what is no plain allocation
goes to the real function, torch's own functions come back on exit and on an exception, and ``dirty_`` writes every byte."""
import numpy as np
import pytest
import torch

from tests.dirty import A5, FILLS, NAN, WORD3, dirty_, dirty_allocations, holds


def _bytes(t):
    return t.contiguous().view(-1).view(torch.uint8).numpy().tobytes()


def test_the_fills_are_what_their_names_say():
    assert np.frombuffer(WORD3, "<u4")[0] == 0x00000003 and np.frombuffer(WORD3, "<f4")[0] > 0     # a denormal
    assert A5 == b"\xa5\xa5\xa5\xa5" and np.frombuffer(A5, "<i4")[0] < 0
    assert np.frombuffer(NAN, "<u4")[0] == 0x7FC00000 and np.isnan(np.frombuffer(NAN, "<f4")[0])
    assert set(FILLS) == {"WORD3", "A5", "NAN"}


@pytest.mark.parametrize("fill", [WORD3, A5, NAN], ids=["WORD3", "A5", "NAN"])
@pytest.mark.parametrize("shape,dtype", [((17, 3), torch.float32), ((5,), torch.int64), ((7,), torch.uint8), ((2, 3), torch.int32),
                                          ((9,), torch.int16), ((), torch.float32), ((1,), torch.uint8), ((3,), torch.bool)])
def test_dirty_writes_every_byte(fill, shape, dtype):
    t = torch.zeros(shape, dtype=dtype)
    ptr = t.data_ptr()
    assert dirty_(t, fill) is t and t.data_ptr() == ptr
    n = t.numel() * t.element_size()
    assert _bytes(t) == (fill * (n // 4 + 1))[:n]
    assert bool(holds(t, fill).all())
    if dtype == torch.float32 and fill is NAN:
        assert bool(torch.isnan(t).all())
    if dtype == torch.int32 and fill is WORD3:
        assert bool((t == 3).all())


def test_dirty_by_value_refuses_floats_and_strided_views():
    t = torch.zeros(6, dtype=torch.int64)
    dirty_(t, -7)
    assert bool((t == -7).all()) and bool(holds(t, -7).all())
    t[2] = 0
    assert holds(t, -7).tolist() == [True, True, False, True, True, True]
    with pytest.raises(ValueError):
        dirty_(torch.zeros(3), -7)
    with pytest.raises(ValueError):
        dirty_(torch.zeros(4, 4).t(), WORD3)
    with pytest.raises(ValueError):
        dirty_(torch.zeros(4), b"\x01\x02")
    assert dirty_(torch.empty(0), A5).numel() == 0


def test_patch_fills_and_logs_and_leaves_zeros_and_full_alone():
    real = {n: getattr(torch, n) for n in ("empty", "zeros", "full", "empty_like", "zeros_like")}
    with dirty_allocations(NAN, int_fill=WORD3, device="cpu") as log:
        assert torch.empty is not real["empty"] and torch.empty_like is not real["empty_like"]
        assert torch.zeros is real["zeros"] and torch.full is real["full"] and torch.zeros_like is real["zeros_like"]
        e = torch.empty(17, 2, dtype=torch.float32, device="cpu")
        et = torch.empty((3, 5), dtype=torch.int32)
        e8 = torch.empty(6, dtype=torch.uint8)
        el = torch.empty_like(e)
        eli = torch.empty_like(e, dtype=torch.int64)
        z = torch.zeros(4, 4)
        f = torch.full((6,), 2.5)
        # what guarded_allocations passes through is passed through
        dest = torch.zeros(5)
        out = torch.empty(5, out=dest)
        nothing = torch.empty(0, dtype=torch.int32)
        meta = torch.empty(4, device="meta")
        rg = torch.empty(4, requires_grad=True)
        like_t = torch.empty_like(torch.ones(4, 6).t())
    assert all(getattr(torch, n) is fn for n, fn in real.items())
    assert bool(torch.isnan(e).all()) and bool(torch.isnan(el).all())
    assert bool((et == 3).all()) and _bytes(e8) == b"\x03\x00\x00\x00\x03\x00" and bool((eli == 3 + (3 << 32)).all())
    assert not z.any() and bool((f == 2.5).all())
    assert out is dest and not dest.any() and nothing.numel() == 0 and meta.device.type == "meta" and rg.requires_grad
    assert [(s, d, n) for _, s, d, n in log] == [((17, 2), torch.float32, 136), ((3, 5), torch.int32, 60), ((6,), torch.uint8, 6),
                                                  ((17, 2), torch.float32, 136), ((17, 2), torch.int64, 272)]
    assert all(c.startswith("test_dirty_host.py:") for c, _, _, _ in log)
    # a pass-through that made bytes on the device is listed, so that a test can demand that there is none
    assert [(s, d) for _, s, d, _ in log.unfilled] == [((4,), torch.float32), ((6, 4), torch.float32)]
    assert len(log.table()) == 5 and "test_dirty_host.py" in log.table()[0]


def test_patch_fills_by_value_and_one_fill_serves_every_dtype():
    with dirty_allocations(NAN, int_fill=-7, device="cpu") as log:
        a, b = torch.empty(5), torch.empty(5, dtype=torch.int64)
    assert bool(torch.isnan(a).all()) and bool((b == -7).all()) and len(log) == 2 and not log.unfilled
    with dirty_allocations(A5, device="cpu") as log:
        a, b = torch.empty(5), torch.empty(5, dtype=torch.int32)
    assert _bytes(a) == A5 * 5 and _bytes(b) == A5 * 5 and len(log) == 2
    with dirty_allocations(A5, device="cuda") as log:               # another device's allocations are not touched, nor logged
        torch.empty(5)
    assert not log and not log.unfilled


def test_patch_restores_torch_after_an_exception():
    real = {n: getattr(torch, n) for n in ("empty", "empty_like")}
    with pytest.raises(RuntimeError, match="boom"):
        with dirty_allocations(WORD3, device="cpu"):
            torch.empty(4)
            raise RuntimeError("boom")
    assert all(getattr(torch, n) is fn for n, fn in real.items())
    with pytest.raises(ValueError):
        with dirty_allocations(b"\x01", device="cpu"):
            pass
    assert all(getattr(torch, n) is fn for n, fn in real.items())

"""tests/guarded.py on a CPU tensor: exact body sizes, placement, storage offset 0, what a damaged byte is reported as, and
the patcher putting torch's own functions back."""
import pytest
import torch

from tests.guarded import BAND_MIN, GUARD_WORD, GuardedArena, band_bytes, guarded_allocations


def arena(nbytes=1 << 20):
    return GuardedArena(nbytes, "cpu")


def test_bodies_are_exact_placed_at_256_mod_512_with_storage_offset_zero():
    a = arena()
    shapes = [((17, 2), torch.float32), ((3,), torch.uint8), ((5, 100), torch.float32), ((7,), torch.int64), ((1,), torch.int32)]
    got = [a.take(s, d) for s, d in shapes]
    for t, (s, d) in zip(got, shapes):
        n = t.numel() * t.element_size()
        assert tuple(t.shape) == s and t.dtype == d and t.is_contiguous()
        assert t.storage_offset() == 0 and t.untyped_storage().nbytes() == n
        assert t.data_ptr() % 512 == 256
        off = a.offset_of(t)
        assert a.buf.data_ptr() + off == t.data_ptr() and 0 < off and off + n < a.nbytes
        assert not t.any()                              # a body starts as zero, torch.empty's included
    # bands: >= 4 KiB, >= 16 rows of the buffer's own pitch, between neighbours the wider of the two
    for prev, cur in zip(a.bodies, a.bodies[1:]):
        assert cur["start"] - prev["end"] >= max(prev["band"], cur["band"]) >= BAND_MIN
    assert a.bodies[0]["start"] >= a.bodies[0]["band"] and a.nbytes - a.bodies[-1]["end"] >= a.bodies[-1]["band"]
    assert band_bytes((17, 2), 4) == 4096 and band_bytes((5, 100), 4) == 6400 and band_bytes((4, 1001), 4) == 64256
    assert band_bytes((9,), 8) == 4096
    # a write through the tensor is a write into the arena, and nothing else changed
    got[2].fill_(7.0)
    off = a.offset_of(got[2])
    assert torch.equal(a.buf[off:off + 2000].view(torch.float32), torch.full((500,), 7.0))
    a.check("writes inside bodies")
    words = a.buf[:a.bodies[0]["start"] // 4 * 4].view(torch.int32)
    assert bool((words == GUARD_WORD).all())


def test_a_full_arena_says_so():
    a = arena(16384)
    a.take((256,), torch.float32)
    with pytest.raises(MemoryError, match="is full"):
        a.take((4096,), torch.float32)
    a.check()


@pytest.mark.parametrize("where", ["end", "start_minus_1", "far_band_last", "inside"])
def test_one_damaged_byte_is_reported_with_buffer_side_and_offset(where):
    a = arena()
    a.take((40, 3), torch.float32, name="first")
    t = a.take((17, 2), torch.float32, name="logits")
    off, n = a.offset_of(t), 17 * 2 * 4
    body = next(b for b in a.bodies if b["name"] == "logits")
    assert (body["start"], body["end"]) == (off, off + n)
    at = dict(end=off + n, start_minus_1=off - 1, far_band_last=off + n + body["band"] - 1, inside=off + n - 1)[where]
    a.buf[at] = 0xA5
    found = a.damage()
    if where == "inside":
        assert found == []
        a.check()
        return
    want = dict(end=("after", 0), start_minus_1=("before", -n - 1), far_band_last=("after", body["band"] - 1))[where]
    assert found == [dict(name="logits", side=want[0], first=want[1], last=want[1], count=1)]
    with pytest.raises(AssertionError) as err:
        a.check("the call")
    assert f"1 damaged byte(s) {want[0]} logits: first at end{want[1]:+d}, last at end{want[1]:+d}" in str(err.value)
    assert "after the call" in str(err.value)


def test_damage_is_assigned_to_the_nearest_buffer_and_a_run_has_first_and_last():
    a = arena()
    t0 = a.take((8,), torch.float32, name="a")
    t1 = a.take((8,), torch.float32, name="b")
    e0, s1 = a.offset_of(t0) + 32, a.offset_of(t1)
    a.buf[e0:e0 + 24] = 1                              # a tail overrun of "a": every byte differs from 03 00 00 00 ...
    a.buf[s1 - 4:s1] = 0                               # ... and a zero word in front of "b": its first byte does
    found = a.damage()
    assert found == [dict(name="a", side="after", first=0, last=23, count=24),
                     dict(name="b", side="before", first=-36, last=-36, count=1)]
    # the whole arena is checked, not only the bands: the very last byte
    b = arena()
    b.take((8,), torch.float32, name="only")
    b.buf[-1] = 9
    assert [(d["name"], d["side"]) for d in b.damage()] == [("only", "after")]


def test_patcher_takes_device_allocations_and_logs_them():
    a = arena()
    real = {n: getattr(torch, n) for n in ("empty", "zeros", "full", "empty_like", "zeros_like")}
    with guarded_allocations(a) as log:
        assert torch.empty is not real["empty"]
        e = torch.empty(17, 2, dtype=torch.float32, device="cpu")
        z = torch.zeros((3, 5), dtype=torch.int32)
        f = torch.full((6,), 2.5)
        fi = torch.full((6,), 4, device="cpu")
        el, zl = torch.empty_like(e), torch.zeros_like(z, dtype=torch.float32)
        # what is not a plain allocation on the arena's device goes to the real function
        rg = torch.zeros(4, requires_grad=True)
        nothing = torch.empty(0, dtype=torch.int32)
        meta = torch.empty(4, device="meta")
        like_t = torch.empty_like(torch.ones(4, 6).t())
    assert all(getattr(torch, n) is fn for n, fn in real.items())
    for t, shape, dtype in ((e, (17, 2), torch.float32), (z, (3, 5), torch.int32), (f, (6,), torch.float32), (fi, (6,), torch.int64),
                            (el, (17, 2), torch.float32), (zl, (3, 5), torch.float32)):
        assert tuple(t.shape) == shape and t.dtype == dtype and 0 < a.offset_of(t) < a.nbytes and t.storage_offset() == 0
    assert not z.any() and not zl.any() and not e.any() and bool((f == 2.5).all()) and bool((fi == 4).all())
    for t in (rg, nothing, meta, like_t):
        assert t.device.type == "meta" or not 0 <= a.offset_of(t) < a.nbytes
    assert len(log) == 6 and log is a.log
    assert [(s, d, n) for _, s, d, n in log[:3]] == [((17, 2), torch.float32, 136), ((3, 5), torch.int32, 60), ((6,), torch.float32, 24)]
    assert all(c.startswith("test_guarded_host.py:") for c, _, _, _ in log)
    assert len(a.table()) == 6 and "test_guarded_host.py" in a.table()[0]
    a.check("the patched allocations")                  # a zeros body is zero and the bands around it are intact


def test_patcher_restores_torch_after_an_exception():
    a = arena()
    real = {n: getattr(torch, n) for n in ("empty", "zeros", "full", "empty_like", "zeros_like")}
    with pytest.raises(RuntimeError, match="boom"):
        with guarded_allocations(a):
            torch.zeros(4)
            raise RuntimeError("boom")
    assert all(getattr(torch, n) is fn for n, fn in real.items())
    assert not 0 <= a.offset_of(torch.empty(4)) < a.nbytes

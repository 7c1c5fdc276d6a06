"""tests/guard.py on the CPU: the banded allocator reports what it must and nothing else."""
import struct

import pytest
import torch

from guard import BAND, GuardArena, GuardError, WORD_FLOAT, WORD_HALF, WORD_INT_IN, WORD_INT_OUT

NAN = float("nan")
SHAPES = [((5,), torch.float32), ((3, 7), torch.float32), ((129, 96), torch.float32), ((9,), torch.float64),
          ((4, 3), torch.float64), ((7,), torch.bfloat16), ((5, 3), torch.float16), ((11,), torch.int32),
          ((3,), torch.uint8), ((2, 5), torch.int64), ((0, 4), torch.float32), ((2, 3, 4, 5), torch.float32)]


def _bytes(arena, i=-1):
    s = arena.slots[i]
    return s, s.raw.view(torch.uint8)


def _band_sizes(slot):
    return slot.start, slot.raw.numel() * 4 - slot.end


@pytest.mark.parametrize("shape,dtype", SHAPES, ids=[f"{str(d)[6:]}{list(s)}" for s, d in SHAPES])
def test_layout_alignment_band_sizes_and_an_untouched_arena_passes(shape, dtype):
    a = GuardArena("cpu")
    t = a.nan(*shape, dtype=dtype)
    u = a.full(shape, 3, dtype, name="threes")
    v = a.place(torch.ones(shape, dtype=dtype), name="ones")
    itemsize = t.element_size()
    row_bytes = itemsize
    for s in shape[1:]:
        row_bytes *= s
    for i, p in enumerate((t, u, v)):
        assert p.shape == shape and p.dtype == dtype and p.is_contiguous()
        slot, by = _bytes(a, i)
        before, after = _band_sizes(slot)
        assert before >= BAND
        assert after >= (BAND if len(shape) == 1 else max(BAND, 128 * row_bytes))
        if p.numel():
            assert p.data_ptr() % 32 == 16
            assert p.data_ptr() == by.data_ptr() + slot.start and slot.end - slot.start == p.numel() * itemsize
    if dtype.is_floating_point:
        assert bool(torch.isnan(t).all())
    else:
        assert bool((t == -7).all())
    assert bool((u == 3).all()) and bool((v == 1).all())
    assert "threes" in a.slots[1].name and "ones" in a.slots[2].name
    assert "test_layout_alignment" in a.slots[0].name          # unnamed buffers carry their call site
    a.check("untouched")


@pytest.mark.parametrize("align", [32, 64, 256, 512])
def test_align_argument(align):
    a = GuardArena("cpu")
    for t in (a.nan(13, 5, align=align), a.full((7,), 0, torch.float64, align=align), a.place(torch.ones(3), align=align)):
        assert t.data_ptr() % align == 0
    a.check()
    with pytest.raises(AssertionError):
        a.nan(4, align=16)


def test_bands_read_as_nan_in_the_buffers_own_type():
    """the words themselves, and the elements on the payload's own grid on either side of it"""
    assert struct.unpack("<f", struct.pack("<I", WORD_FLOAT))[0] != struct.unpack("<f", struct.pack("<I", WORD_FLOAT))[0]
    d = struct.unpack("<d", struct.pack("<II", WORD_FLOAT, WORD_FLOAT))[0]
    assert d != d
    for dt in (torch.float16, torch.bfloat16):
        assert bool(torch.isnan(torch.tensor([WORD_HALF & 0xFFFF], dtype=torch.int32).to(torch.int16).view(dt)).all())
    a = GuardArena("cpu")
    for dtype, shape in ((torch.float32, (5, 3)), (torch.float64, (3,)), (torch.bfloat16, (7,)), (torch.float16, (3, 3)),
                         (torch.bfloat16, (4, 4))):
        for t in (a.full(shape, 1.0, dtype), a.place(torch.ones(shape, dtype=dtype))):
            slot, by = _bytes(a)
            item = t.element_size()
            before = by[slot.start % item:slot.start].view(dtype)
            tail = (by.numel() - slot.end) // item * item
            after = by[slot.end:slot.end + tail].view(dtype)
            assert before.numel() >= BAND // item and after.numel() >= BAND // item
            assert bool(torch.isnan(before).all()) and bool(torch.isnan(after).all())
            assert bool((t == 1).all())


def test_integer_bands():
    a = GuardArena("cpu")
    out = a.full((5,), 9, torch.int32, name="out")
    inp = a.place(torch.arange(5, dtype=torch.int32), name="in")
    s_out, s_in = a.slots
    assert s_out.word == WORD_INT_OUT and s_in.word == WORD_INT_IN == 0
    assert bool((s_out.raw[:s_out.start // 4] == -8531).all()) and bool((s_out.raw[s_out.end // 4:] == -8531).all())
    assert bool((s_in.raw[:s_in.start // 4] == 0).all()) and bool((s_in.raw[s_in.end // 4:] == 0).all())
    assert out.tolist() == [9] * 5 and inp.tolist() == list(range(5))
    a.check()


CASES = [((129, 96), torch.float32), ((5,), torch.float64), ((7,), torch.bfloat16), ((3,), torch.uint8),
         ((11,), torch.int32)]


@pytest.mark.parametrize("shape,dtype", CASES, ids=[f"{str(d)[6:]}{list(s)}" for s, d in CASES])
@pytest.mark.parametrize("where", ["just_before", "just_after", "first_byte_of_the_arena", "last_byte_of_the_arena"])
def test_one_changed_byte_is_reported_with_name_side_and_offset(shape, dtype, where):
    a = GuardArena("cpu")
    a.nan(4, 4, name="bystander")
    a.full(shape, 0, dtype, name="victim")
    a.place(torch.ones(3), name="other")
    slot, by = _bytes(a, 1)
    before, after = _band_sizes(slot)
    index, side, offset = {"just_before": (slot.start - 1, "before", -1),
                           "just_after": (slot.end, "after", 0),
                           "first_byte_of_the_arena": (0, "before", -before),
                           "last_byte_of_the_arena": (by.numel() - 1, "after", after - 1)}[where]
    by[index] ^= 0x01
    with pytest.raises(GuardError) as e:
        a.check("case 7")
    assert len(e.value.findings) == 1
    name, got_side, got_offset, count = e.value.findings[0]
    assert name.startswith("victim") and (got_side, got_offset, count) == (side, offset, 1)
    msg = str(e.value)
    assert "case 7" in msg and "victim" in msg and f"band {side}" in msg and f"offset {offset} " in msg and "1 byte(s)" in msg
    assert "bystander" not in msg and "other" not in msg
    by[index] ^= 0x01
    a.check("restored")


def test_several_changed_bytes_count_and_nearest_offset():
    a = GuardArena("cpu")
    t = a.nan(10, 4, name="rows")
    slot, by = _bytes(a)
    by[slot.end + 16:slot.end + 32] = 0           # one float4 row stored one row too far
    by[slot.start - 8:slot.start - 4] = 0
    with pytest.raises(GuardError) as e:
        a.check()
    assert sorted(e.value.findings) == [(slot.name, "after", 16, 16), (slot.name, "before", -5, 4)]   # bytes -8 .. -5
    assert bool(torch.isnan(t).all())


def test_writes_inside_the_payload_are_not_reported():
    a = GuardArena("cpu")
    for dtype in (torch.float32, torch.float64, torch.bfloat16, torch.int32, torch.uint8):
        t = a.full((7, 3), 0, dtype)
        t.fill_(1)
        t.view(-1)[0], t.view(-1)[-1] = 2, 2
        slot, by = _bytes(a)
        by[slot.start:slot.end] = 0xFF           # every payload byte, first and last included
    e = a.full((0, 4), None, torch.float32)
    assert e.numel() == 0
    a.check()


def test_full_without_a_fill_leaves_the_payload_and_writes_the_bands():
    a = GuardArena("cpu")
    t = a.full((6,), None, torch.float32, name="workspace")
    assert t.shape == (6,)
    t.zero_()
    a.check()


def test_place_preserves_bit_patterns():
    a = GuardArena("cpu")
    bits = torch.tensor([0x7FC00000, 0x7FC00001, 0xFFC12345 - (1 << 32), 0x7F800001, 0x80000000 - (1 << 32), 0, 1,
                         0x7F800000, 0xFF800000 - (1 << 32), 0x3F800000], dtype=torch.int32)
    x = bits.view(torch.float32)
    p = a.place(x, name="f32")
    assert torch.equal(p.view(torch.int32), bits)
    assert p[4].item() == 0 and torch.signbit(p[4]).item()          # -0.0 stays -0.0
    assert p.data_ptr() != x.data_ptr()
    b64 = torch.tensor([0x7FF8000000000001, 0x7FF0000000000001, -(1 << 63), 0x3FF0000000000000], dtype=torch.int64)
    assert torch.equal(a.place(b64.view(torch.float64)).view(torch.int64), b64)
    b16 = torch.tensor([0x7FC1, 0x7F81, -0x8000, 0x3F80], dtype=torch.int16)
    assert torch.equal(a.place(b16.view(torch.bfloat16)).view(torch.int16), b16)
    ints = torch.tensor([[-1, 2], [3, -(1 << 31)]], dtype=torch.int32)
    assert torch.equal(a.place(ints), ints)
    nc = torch.arange(12.0).view(3, 4).t()                          # a non-contiguous input arrives contiguous
    q = a.place(nc)
    assert q.is_contiguous() and torch.equal(q, nc)
    one = torch.arange(54.0).view(27, 1, 2).transpose(1, 2)          # contiguous, with a stride of 2 in its size-1 dimension
    assert one.is_contiguous() and one.stride(-1) != 1
    q = a.place(one)
    assert q.shape == one.shape and torch.equal(q, one) and q.stride() == (2, 1, 1)
    assert torch.equal(a.place(torch.tensor(2.5)), torch.tensor(2.5))
    g = a.place(torch.ones(3, requires_grad=True))
    assert not g.requires_grad
    a.check()


def test_reset_forgets_old_buffers():
    a = GuardArena("cpu")
    a.nan(8, name="old")
    slot, by = _bytes(a)
    by[slot.end] ^= 0xFF
    with pytest.raises(GuardError):
        a.check()
    a.reset()
    assert a.slots == []
    a.check("empty")
    a.nan(8, name="new")
    a.check("after reset")

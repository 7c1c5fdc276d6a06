"""A banded allocator for the C-ABI tests: every buffer it hands out lies between two guard bands inside one torch
allocation of its own,

    | band before (>= 4096 B) | payload | band after (>= max(4096 B, 128 rows of the payload)) |

so that a kernel which stores past either end of an output or a workspace changes a band (GuardArena.check finds it
and names the buffer, the side, the byte offset from the payload's edge and the number of changed bytes), and a kernel
whose result depends on a load past the end of a float input reads a NaN, which the finiteness checks the tests
already make then see.  The band after a payload covers one whole padded 128-row tile of that buffer's own rows
(row_bytes = prod(shape[1:]) * itemsize); a one-dimensional buffer gets 4096 bytes on both sides.

Band contents, always one 32-bit word repeated from the start of the allocation and compared as bits:
  - floating-point buffers: 0x7FF8DEAD, a quiet NaN as float32 and, twice, as float64; 16-bit types get 0x7FDE7FDE,
    whose halves are a quiet NaN as bfloat16 and as float16;
  - integer buffers the test hands to a kernel to write (full / nan): the sentinel 0xFFFFDEAD, a small negative
    number as int32, which the kernels that read such a buffer back as indices treat as "missing";
  - integer inputs (place): 0, a valid row, so that a stray index read can never send a later access outside a
    buffer.  NO DETECTION IS CLAIMED for loads past the end of an integer input: a 0 read there is a legal index,
    and what follows from it may or may not show in a result.

Every payload starts on a 16-byte boundary that is no 32-byte boundary (data_ptr() % 32 == 16): the least alignment a
row slice of a [n, C] float tensor with C % 4 == 0 has.  `align=` asks for a stronger one (a power of two >= 32) for
the buffers of an entry point whose header documents it.

This is a helper module, not a conftest: nothing here runs unless a test builds a GuardArena."""
import sys

import torch

BAND = 4096
TILE_ROWS = 128
WORD_FLOAT = 0x7FF8DEAD
WORD_HALF = 0x7FDE7FDE
WORD_INT_OUT = 0xFFFFDEAD
WORD_INT_IN = 0x00000000
_FLOAT16 = (torch.float16, torch.bfloat16)


class GuardError(AssertionError):
    """a band changed; `findings` holds (name, side, offset, count) per changed band.  offset: the changed byte
    nearest to the payload, counted from the payload's edge -- 0 is the first byte after the payload, -1 the last
    byte before it"""

    def __init__(self, message, findings):
        super().__init__(message)
        self.findings = findings


def _signed(word):
    return word - (1 << 32) if word >= 1 << 31 else word


def _caller():
    """function:line of the nearest frame outside this module and outside the allocation hooks of the test modules"""
    f = sys._getframe(1)
    while f is not None and (f.f_globals.get("__name__") == __name__ or f.f_code.co_name in
                             ("_nan", "_fill", "_dev", "<lambda>", "<genexpr>", "<dictcomp>", "<listcomp>")):
        f = f.f_back
    return f"{f.f_code.co_name}:{f.f_lineno}" if f is not None else "?"


class _Slot:
    __slots__ = ("name", "raw", "start", "end", "word")

    def __init__(self, name, raw, start, end, word):
        self.name, self.raw, self.start, self.end, self.word = name, raw, start, end, word

    def bands(self):
        """(side, int32 words of the 4-byte-aligned part, the bytes between the payload and that part, their word
        phase) for the band before and the band after the payload"""
        by = self.raw.view(torch.uint8)
        head_end = (self.end + 3) // 4 * 4
        return (("before", self.raw[:self.start // 4], by[:0], 0),
                ("after", self.raw[head_end // 4:], by[self.end:head_end], self.end % 4))


class GuardArena:
    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.slots = []

    # ---- allocation
    def _slot(self, shape, dtype, name, align, word):
        shape = tuple(int(s) for s in shape)
        itemsize = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        row_bytes = itemsize
        for s in shape[1:]:
            row_bytes *= s
        nbytes = numel * itemsize
        after = BAND if len(shape) <= 1 else max(BAND, TILE_ROWS * row_bytes)
        if align is None:
            step, want = 32, 16
        else:
            assert align >= 32 and align & (align - 1) == 0, "align: a power of two >= 32 (16 is the default)"
            step, want = align, 0
        total = BAND + step + nbytes + after
        total = (total + 3) // 4 * 4
        raw = torch.empty(total // 4, dtype=torch.int32, device=self.device)
        base = raw.data_ptr()
        assert base % 16 == 0, "torch allocation below 16-byte alignment"
        start = BAND + (want - (base + BAND)) % step
        end = start + nbytes
        raw[:start // 4].fill_(_signed(word))
        by = raw.view(torch.uint8)
        head_end = (end + 3) // 4 * 4
        if head_end > end:                 # the bytes between the payload's end and the next whole word
            pat = torch.tensor([(word >> (8 * i)) & 0xFF for i in range(4)], dtype=torch.uint8, device=self.device)
            by[end:head_end] = pat[end % 4:]
        raw[head_end // 4:].fill_(_signed(word))
        payload = by[start:end].view(dtype).view(shape) if numel else by[start:start].view(dtype).reshape(shape)
        assert payload.is_contiguous()
        assert numel == 0 or payload.data_ptr() % step == want
        if name is None:
            name = f"#{len(self.slots)} {_caller()}"
        name = f"{name} {str(dtype).replace('torch.', '')}{list(shape)}"
        self.slots.append(_Slot(name, raw, start, end, word))
        return payload

    @staticmethod
    def _word(dtype, written):
        if dtype.is_floating_point:
            return WORD_HALF if dtype in _FLOAT16 else WORD_FLOAT
        return WORD_INT_OUT if written else WORD_INT_IN

    def full(self, shape, fill, dtype=torch.float32, name=None, align=None):
        """a buffer for a kernel to write: payload filled with `fill` (None: left as torch.empty gives it)"""
        if isinstance(shape, int):
            shape = (shape,)
        t = self._slot(shape, dtype, name, align, self._word(dtype, True))
        if fill is not None:
            t.fill_(fill)
        return t

    def nan(self, *shape, dtype=torch.float32, name=None, align=None):
        """the `_nan` of the test modules: NaN, or for an integer type the impossible -7 test_gpu_pool.py uses"""
        return self.full(shape, float("nan") if dtype.is_floating_point else -7, dtype, name, align)

    def place(self, tensor, name=None, align=None):
        """a copy of an input in a slot of its own, bit for bit (on this arena's device)"""
        src = tensor.detach().contiguous()
        t = self._slot(src.shape, src.dtype, name, align, self._word(src.dtype, False))
        if src.numel():
            # flat: a "contiguous" tensor may carry any stride in a dimension of size 1
            t.reshape(-1).view(torch.uint8).copy_(src.reshape(-1).view(torch.uint8).to(self.device))
        return t

    # ---- the check
    def check(self, what=""):
        """synchronise, then assert that every band of every buffer handed out since the last reset holds its word"""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        counts = []
        for s in self.slots:
            for _, words, head, phase in s.bands():
                c = (words != _signed(s.word)).sum()
                if head.numel():
                    pat = torch.tensor([(s.word >> (8 * i)) & 0xFF for i in range(4)], dtype=torch.uint8,
                                       device=self.device)
                    c = c + (head != pat[phase:]).sum()
                counts.append(c)
        if not counts:
            return
        bad = torch.stack(counts).cpu().view(-1, 2)
        if not bool(bad.any()):
            return
        findings = []
        for s, row in zip(self.slots, bad):
            if not bool(row.any()):
                continue
            by = s.raw.view(torch.uint8).cpu()
            pat = torch.tensor([(s.word >> (8 * i)) & 0xFF for i in range(4)], dtype=torch.uint8)
            for side, lo, hi in (("before", 0, s.start), ("after", s.end, by.numel())):
                want = pat[torch.arange(lo, hi) % 4]
                changed = torch.nonzero(by[lo:hi] != want).view(-1)
                if changed.numel():
                    off = int(changed[0]) if side == "after" else int(changed[-1]) - (hi - lo)
                    findings.append((s.name, side, off, int(changed.numel())))
        lines = [f"buffer '{n}': band {side} the payload changed, first changed byte at offset {off} from the payload's "
                 f"edge, {cnt} byte(s) changed" for n, side, off, cnt in findings]
        raise GuardError(f"{what}: a kernel wrote outside its buffer\n  " + "\n  ".join(lines), findings)

    def reset(self):
        """forget (and free) every buffer handed out so far"""
        self.slots = []

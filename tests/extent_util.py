"""Guarded windows for the buffer-extent tests (tests/test_gpu_extents.py; DESIGN.md, "Buffer extents").

A *window* is a contiguous tensor that lives inside one larger torch allocation, its *arena*.  The bytes of the arena in front of and behind the window
are the *bands*; they hold a poison pattern that no kernel of the library produces:

  float32 / float64   a quiet NaN with a payload (0x7FC5A5A5 / 0x7FF8A5A5A5A5A5A5).  The bands are compared as integers, never as floats, so a kernel that
                      itself writes a NaN -- or the same poison value read from an input band -- into a band position that held another byte is seen;
  everything else     0xA5 bytes.

A fresh window holds the poison too: an output that the header documents as written in full must not contain it afterwards (assert_fully_written), and an
input that a kernel reads past its extent hands the kernel NaNs, which show up in a result.

Every pointer the tests pass to the library points into an arena this process owns, and the arena reaches at least the header's full extent behind the
pointer: a band is never smaller than 4 KiB, and each call sizes it to the largest write the entry point could make beyond the window if it were off by one
unit of its contract (one 128-row slab, one record, one slice).  A violation therefore lands in the arena; the tests observe stray writes in owned memory.

`skew` is the window's address modulo 256.  torch's allocations are aligned to 256 bytes or better, which hides a kernel that needs more alignment than the
header promises: a window is placed 16 bytes past a 256-byte boundary where the header promises 16-byte alignment, and 4 bytes past it (the element's own
size, for 8-byte elements) where the header promises nothing.
"""
import math

import torch

DEV = "cuda:0"
MIN_BAND = 4096
POISON32 = 0x7FC5A5A5
POISON64 = 0x7FF8A5A5A5A5A5A5
_FLOAT = {torch.float32: (torch.int32, POISON32), torch.float64: (torch.int64, POISON64)}


class Arena:
    """One allocation: [front band | window | back band].  `off` / `nbytes`: the window's place in `buf` (uint8)."""

    def __init__(self, buf, off, nbytes, dtype):
        self.buf, self.off, self.nbytes, self.dtype = buf, off, nbytes, dtype
        self.expected = buf.clone()  # the poisoned state of every byte, the window's included


def _poison(buf, dtype):
    """fill the whole arena (uint8, a multiple of 8 bytes, 256-byte aligned) with the dtype's poison"""
    if dtype in _FLOAT:
        idt, val = _FLOAT[dtype]
        buf.view(idt).fill_(val)
    else:
        buf.fill_(0xA5)


def window(shape, dtype=torch.float32, front=MIN_BAND, back=MIN_BAND, skew=16):
    """(view, arena): a poisoned contiguous tensor of `shape` at address = skew (mod 256) with at least `front` / `back` poisoned bytes around it."""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    item = torch.empty(0, dtype=dtype).element_size()
    assert 0 <= skew < 256 and skew % item == 0, (skew, item)
    front, back = max(int(front), MIN_BAND), max(int(back), MIN_BAND)
    nbytes = math.prod(shape) * item
    total = (front + 512 + nbytes + back + 7) // 8 * 8
    buf = torch.empty(total, dtype=torch.uint8, device=DEV)
    base = buf.data_ptr()
    assert base % 16 == 0
    off = front + (skew - (base + front)) % 256  # the first address at or behind `front` bytes that is skew (mod 256)
    assert (base + off) % 256 == skew and off >= front and total - off - nbytes >= back
    _poison(buf, dtype)
    view = buf[off : off + nbytes].view(dtype).view(shape)
    assert view.data_ptr() == base + off and view.is_contiguous()
    return view, Arena(buf, off, nbytes, dtype)


def window_of(t, front=MIN_BAND, back=MIN_BAND, skew=16):
    """an input in a window: (view holding a copy of `t`, arena)"""
    view, arena = window(t.shape, t.dtype, front, back, skew)
    view.copy_(t)
    return view, arena


def padded_window_of(t, rows, fill, front=MIN_BAND, back=MIN_BAND, skew=16):
    """an input whose header extent is `rows` >= t.shape[0] rows: rows [0, t.shape[0]) = t, the pad rows behind them = `fill`"""
    assert t.dim() == 2 and rows >= t.shape[0]
    view, arena = window((rows, t.shape[1]), t.dtype, front, back, skew)
    view[: t.shape[0]].copy_(t)
    view[t.shape[0] :].fill_(fill)
    return view, arena


def assert_bands_untouched(arena, what):
    """both bands bit for bit; names the first byte that changed, relative to the window"""
    bad = arena.buf != arena.expected
    bad[arena.off : arena.off + arena.nbytes] = False
    if bool(bad.any()):
        first = int(bad.nonzero()[0])
        n = int(bad.sum())
        where = f"{arena.off - first} bytes in front of the window" if first < arena.off else f"{first - arena.off - arena.nbytes} bytes behind the window's end"
        raise AssertionError(f"{what}: {n} band bytes changed, the first {where} (window of {arena.nbytes} bytes)")


def assert_fully_written(view, what):
    """no element of an output that the header documents as written in full still holds the poison"""
    if view.dtype in _FLOAT:
        idt, val = _FLOAT[view.dtype]
        left = view.view(idt) == val
    else:
        item = view.element_size()
        left = (view.contiguous().view(torch.uint8).view(-1, item) == 0xA5).all(dim=1)
    n = int(left.sum())
    assert n == 0, f"{what}: {n} of {view.numel()} elements were never written (first at flat index {int(left.reshape(-1).nonzero()[0])})"


def is_poison(view):
    """elementwise: does the element still hold the poison (for outputs of which the header says which part is left alone)"""
    if view.dtype in _FLOAT:
        idt, val = _FLOAT[view.dtype]
        return view.view(idt) == val
    return (view.contiguous().view(torch.uint8).view(-1, view.element_size()) == 0xA5).all(dim=1).view(view.shape)


class Windows:
    """The windows of one case: makes them, remembers their arenas, checks all bands at the end."""

    def __init__(self):
        self.arenas = []

    def _keep(self, name, pair):
        self.arenas.append((name, pair[1]))
        return pair[0]

    def inp(self, name, t, skew=16, band=None):
        if band is None:  # a matrix of rows: one more 128-row slab of it, so that a kernel that reads a slab too far still reads owned memory
            band = max(MIN_BAND, 128 * t.shape[-1] * t.element_size()) if t.dim() == 2 else MIN_BAND
        return self._keep(name, window_of(t, band, band, skew))

    def padded(self, name, t, rows, fill, skew=16, band=MIN_BAND):
        return self._keep(name, padded_window_of(t, rows, fill, band, band, skew))

    def out(self, name, shape, dtype=torch.float32, skew=16, band=MIN_BAND):
        return self._keep(name, window(shape, dtype, band, band, skew))

    def zeros(self, name, shape, dtype=torch.float32, skew=16, band=MIN_BAND):
        v = self.out(name, shape, dtype, skew, band)
        v.zero_()
        return v

    def check(self, what):
        torch.cuda.synchronize()
        for name, arena in self.arenas:
            assert_bands_untouched(arena, f"{what}: {name}")

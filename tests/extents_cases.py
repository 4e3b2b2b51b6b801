"""Guard bands for operator outputs and inputs: a kernel may write its own output and nothing else.

The caching allocator rounds every block up, so a store a few elements past the end of an output - or into the pad columns of
a strided row - lands in memory nobody looks at.  `guarded` puts a tensor in the middle of one byte buffer filled with 0xFF
(NaN in f32, bfloat16 and binary16), so that a stray write is visible as a changed byte and a stray read as a NaN in a result.
Plain module like the other *_cases.py files; used on the CPU by tests/test_cpu_extents.py and on the GPU by
tests/test_gpu_extents.py."""
import math

import torch

GUARD = 4096     # bytes in front of and behind the view
ALIGN = 256      # alignment of the view's first byte (the kernels ask for 16; 256 is what the allocator itself gives)
POISON = 0xFF


def _itemsize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def guarded(shape, dtype, device, guard=GUARD):
    """(view, backing): `view` has the requested shape and dtype, is contiguous, starts `guard` bytes into the uint8 tensor
    `backing` at a 256-byte aligned address and is followed by at least `guard` more bytes; every byte of `backing`,
    the view's included, is 0xFF."""
    assert guard > 0 and guard % ALIGN == 0, "the guard must keep the view's alignment"
    shape = tuple(int(s) for s in shape)
    nbytes = math.prod(shape) * _itemsize(dtype)
    backing = torch.full((guard + nbytes + guard + ALIGN,), POISON, dtype=torch.uint8, device=device)
    skew = (-backing.data_ptr()) % ALIGN
    start = skew + guard
    view = backing[start:start + nbytes].view(dtype).view(shape)
    assert view.data_ptr() % ALIGN == 0 and view.data_ptr() == backing.data_ptr() + start
    return view, backing


def _span(backing, view):
    start = view.data_ptr() - backing.data_ptr()
    nbytes = view.numel() * view.element_size()
    assert view.is_contiguous() and 0 < start and start + nbytes < backing.numel(), "not a view made by guarded()"
    return start, nbytes


def assert_guards_intact(backing, view, what="output"):
    """every byte in front of and behind `view` inside `backing` is still 0xFF; otherwise the first and last touched byte
    offsets, relative to the view's first byte, are reported"""
    start, nbytes = _span(backing, view)
    for name, lo, hi in (("front", 0, start), ("back", start + nbytes, backing.numel())):
        bad = torch.nonzero(backing[lo:hi] != POISON).flatten()
        if bad.numel():
            first, last = int(bad[0]) + lo - start, int(bad[-1]) + lo - start
            raise AssertionError("%s: %d bytes of the %s guard were written: first at byte offset %d, last at %d relative to the "
                                 "view (the view holds bytes 0 .. %d)" % (what, bad.numel(), name, first, last, nbytes - 1))


def assert_columns(view2d, lo, hi, expect, what="output"):
    """the pad columns [lo, hi) of every row of a strided output (any leading dimensions, columns last) are `expect`:
    "untouched" - every byte still 0xFF - or "zero" - every byte 0 (+0.0 in every format)"""
    assert expect in ("untouched", "zero") and 0 <= lo <= hi <= view2d.shape[-1]
    if lo == hi:
        return
    cols = view2d.reshape(-1, view2d.shape[-1])[:, lo:hi].contiguous()
    raw = cols.view(torch.uint8).reshape(cols.shape[0], -1)
    want = POISON if expect == "untouched" else 0
    bad = torch.nonzero(raw != want)
    if bad.numel():
        es = view2d.element_size()
        r, c = int(bad[0, 0]), lo + int(bad[0, 1]) // es
        raise AssertionError("%s: pad columns [%d, %d) must be %s, but %d bytes differ: first in row %d, column %d"
                             % (what, lo, hi, expect, bad.shape[0], r, c))


class Plain:
    """Today's allocation: outputs at exactly their size from the caching allocator, inputs copied to the device as they are.
    The default of the case bodies in tests/test_gpu_ops.py."""
    device = "cuda"

    def out(self, shape, dtype, fill=None):
        if fill is None:
            return torch.empty(tuple(shape), device=self.device, dtype=dtype)
        return torch.full(tuple(shape), fill, device=self.device, dtype=dtype)

    def inout(self, t):
        return t.clone().to(self.device)

    def inp(self, t):
        return t.to(self.device)

    def check(self):
        pass


class Guarded(Plain):
    """Every output and every activation input in a guarded buffer.  out(fill=None) leaves the view at 0xFF (NaN): what the
    kernel does not write stays visible.  check() - after torch.cuda.synchronize() - asserts that all guards are intact."""

    def __init__(self, device="cuda"):
        self.device = device
        self.held = []

    def _new(self, shape, dtype, what):
        view, backing = guarded(shape, dtype, self.device)
        self.held.append((backing, view, "%s %d %s%s" % (what, len(self.held), str(dtype).replace("torch.", ""), list(shape))))
        return view

    def out(self, shape, dtype, fill=None):
        view = self._new(shape, dtype, "output")
        if fill is not None:
            view.fill_(fill)
        return view

    def inout(self, t):
        view = self._new(t.shape, t.dtype, "in/out")
        view.copy_(t)
        return view

    def inp(self, t):
        view = self._new(t.shape, t.dtype, "input")
        view.copy_(t)
        return view

    def check(self):
        assert self.held, "the case allocated nothing through the guarded allocator"
        for backing, view, what in self.held:
            assert_guards_intact(backing, view, what)

"""The guard-band helper of tests/extents_cases.py on the CPU: it must see a single stray byte on either side of a view and a
write into a pad column, and the views it hands out must be aligned as promised - a kernel that declines a misaligned pointer
would quietly move a test to another kernel."""
import pytest
import torch

from extents_cases import ALIGN, GUARD, Guarded, Plain, assert_columns, assert_guards_intact, guarded

DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.uint8, torch.int32, torch.int64, torch.float64]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1,), (3, 5), (2, 7, 9), (1, 1, 1, 24)])
def test_view_is_aligned_poisoned_and_inside_its_guards(dtype, shape):
    view, backing = guarded(shape, dtype, "cpu")
    assert view.shape == shape and view.dtype == dtype and view.is_contiguous()
    assert view.data_ptr() % ALIGN == 0
    start = view.data_ptr() - backing.data_ptr()
    assert start >= GUARD and backing.numel() - (start + view.numel() * view.element_size()) >= GUARD
    assert bool((backing == 0xFF).all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(view.double()).all())          # 0xFF bytes are NaN in every floating format used
    assert_guards_intact(backing, view)
    view.zero_()                                                # writing the whole view is no violation
    assert_guards_intact(backing, view)


def test_other_guard_sizes_keep_the_alignment():
    view, backing = guarded((5,), torch.float32, "cpu", guard=512)
    assert view.data_ptr() % ALIGN == 0 and view.data_ptr() - backing.data_ptr() >= 512
    with pytest.raises(AssertionError):
        guarded((5,), torch.float32, "cpu", guard=100)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_one_stray_byte_in_front_is_reported(dtype):
    view, backing = guarded((4, 6), dtype, "cpu")
    start = view.data_ptr() - backing.data_ptr()
    backing[start - 1] = 0
    with pytest.raises(AssertionError, match=r"front guard.*first at byte offset -1, last at -1 "):
        assert_guards_intact(backing, view)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_one_stray_byte_behind_is_reported(dtype):
    view, backing = guarded((4, 6), dtype, "cpu")
    start = view.data_ptr() - backing.data_ptr()
    nbytes = 24 * view.element_size()
    backing[start + nbytes] = 0x7F
    with pytest.raises(AssertionError, match=r"back guard.*first at byte offset %d, last at %d " % (nbytes, nbytes)):
        assert_guards_intact(backing, view)
    backing[start + nbytes + 15] = 0                            # a 16-byte vector store past the end
    with pytest.raises(AssertionError, match=r"2 bytes of the back guard.*first at byte offset %d, last at %d " % (nbytes, nbytes + 15)):
        assert_guards_intact(backing, view)


def test_far_ends_of_both_guards_are_watched():
    view, backing = guarded((8,), torch.float32, "cpu")
    backing[0] = 1
    with pytest.raises(AssertionError, match="front guard"):
        assert_guards_intact(backing, view)
    backing[0] = 0xFF
    backing[-1] = 1
    with pytest.raises(AssertionError, match="back guard"):
        assert_guards_intact(backing, view)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_write_into_a_pad_column_is_reported(dtype):
    view, backing = guarded((2, 5, 16), dtype, "cpu")          # rows of 16, logical width 9
    view[..., :9] = 1.0
    assert_columns(view, 9, 16, "untouched")
    with pytest.raises(AssertionError, match="must be zero"):
        assert_columns(view, 9, 16, "zero")
    view[1, 3, 12] = 0.0                                        # one element of one pad column
    with pytest.raises(AssertionError, match=r"must be untouched.*first in row 8, column 12"):
        assert_columns(view, 9, 16, "untouched")
    view[..., 9:] = 0.0
    assert_columns(view, 9, 16, "zero")
    view[0, 0, 15] = -0.0 if dtype != torch.float32 else 1e-30  # "zero" means the bit pattern of +0.0
    with pytest.raises(AssertionError, match=r"must be zero.*first in row 0, column 15"):
        assert_columns(view, 9, 16, "zero")
    assert_columns(view, 16, 16, "zero")                        # an empty range holds trivially
    assert_guards_intact(backing, view)


def test_allocators_share_one_interface():
    t = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    for alloc in (Plain(), Guarded("cpu")):
        alloc.device = "cpu"
        o = alloc.out((3, 4), torch.bfloat16, fill=-7.0)
        assert o.shape == (3, 4) and bool((o == -7.0).all())
        assert torch.equal(alloc.inp(t), t) and torch.equal(alloc.inout(t), t)
        assert alloc.inout(t).data_ptr() != t.data_ptr()
        alloc.check()
    g = Guarded("cpu")
    o = g.out((3, 4), torch.float32)
    assert bool(torch.isnan(o).all())                           # unfilled guarded outputs stay poisoned
    backing = g.held[0][0]
    backing[o.data_ptr() - backing.data_ptr() + 48] = 0
    with pytest.raises(AssertionError, match=r"output 0 float32\[3, 4\].*first at byte offset 48"):
        g.check()
    with pytest.raises(AssertionError):
        Guarded("cpu").check()                                  # a case that guarded nothing proves nothing

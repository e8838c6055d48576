"""tests/fences.py on CPU tensors: the detector must fire on a planted write one element before and one element after the
payload, on a planted unwritten output element and on a stored plain NaN in a fence, and must pass a clean write - for every
offset the GPU tests use, for the float, integer and 64-bit layouts and for the byte-addressed scratch layout."""
import pytest
import torch

import fences as F

OFFSETS = (0, 1, 2, 3)


def _poison_as_float():
    return torch.tensor([F.POISON], dtype=torch.int32).view(torch.float32)


def test_the_poison_word_is_a_quiet_nan_with_a_payload():
    p = _poison_as_float()
    assert torch.isnan(p).all()
    plain = torch.tensor([float('nan')]).view(torch.int32)
    assert int(plain) != F.POISON and (F.POISON >> 22) & 1 == 1 and F.POISON & 0x3FFFFF != 0


@pytest.mark.parametrize('offset', OFFSETS)
@pytest.mark.parametrize('dtype', [torch.float32, torch.int32, torch.int64, torch.float64])
def test_layout_and_a_clean_write(dtype, offset):
    n = 37
    view, whole = F.fenced(n, dtype, offset)
    size = whole.element_size()
    fence = F.FENCE_BYTES // size
    assert whole.numel() == 2 * fence + offset + n and view.numel() == n
    assert (view.data_ptr() - offset * size) % 16 == 0 and view.data_ptr() - whole.data_ptr() == (fence + offset) * size
    if dtype == torch.float32:
        assert bool((whole.view(torch.int32) == F.POISON).all())
    with pytest.raises(F.FenceError, match='never written'):       # nothing stored yet: every element is reported
        F.check(whole, offset, n)
    F.check(whole, offset, n, written=False)                       # ... unless the payload is an input
    view.copy_(torch.arange(n).to(dtype))
    F.check(whole, offset, n)
    F.check_view(whole, view)


@pytest.mark.parametrize('offset', OFFSETS)
def test_a_write_one_element_before_the_payload(offset):
    n = 16
    view, whole = F.fenced(n, torch.float32, offset)
    view.fill_(1.0)
    whole[F.fence_elems(torch.float32) + offset - 1] = 2.0
    with pytest.raises(F.FenceError, match=r'BEFORE the payload, nearest first at \[-1\]'):
        F.check(whole, offset, n)


@pytest.mark.parametrize('offset', OFFSETS)
def test_a_write_one_element_after_the_payload(offset):
    n = 16
    view, whole = F.fenced(n, torch.float32, offset)
    view.fill_(1.0)
    whole[F.fence_elems(torch.float32) + offset + n] = 0.0
    with pytest.raises(F.FenceError, match=r'AFTER the payload, first at \[16\]'):
        F.check(whole, offset, n)
    assert len(F.problems(whole, offset, n)) == 1


def test_an_unwritten_element_is_named():
    n = 100
    view, whole = F.fenced(n, torch.float32, 3)
    view.fill_(0.5)
    view.view(torch.int32)[41] = F.POISON
    with pytest.raises(F.FenceError, match=r'1 of 100 output element\(s\) never written, first at \[41\]'):
        F.check(whole, 3, n)


def test_a_stored_plain_nan_in_a_fence_is_a_write():
    n = 8
    view, whole = F.fenced(n, torch.float32, 1)
    view.fill_(0.0)
    whole[5] = float('nan')                          # far from the payload, and NaN like its neighbours
    whole[-1] = float('nan')
    assert torch.isnan(whole[:F.fence_elems(torch.float32)]).all()
    found = F.problems(whole, 1, n)
    assert len(found) == 2 and 'BEFORE' in found[0] and 'AFTER' in found[1]
    # a NaN that a kernel computed from poison and stored INTO the payload is a written element; the finiteness check of
    # the caller reports it, not the fence
    view2, whole2 = F.fenced(n, torch.float32, 0)
    view2.fill_(float('nan'))
    F.check(whole2, 0, n)


def test_an_input_keeps_its_values_and_snapshots_compare_bits():
    x = torch.randn(3, 5, 7)
    view, whole = F.fenced_input(x, 2)
    assert torch.equal(view, x.flatten()) and view.data_ptr() % 16 == 8
    F.check(whole, 2, x.numel(), written=False)
    before = F.snapshot(whole)
    assert F.unchanged(whole, before)
    whole[0] = float('nan')
    assert not F.unchanged(whole, before)


@pytest.mark.parametrize('align, offset_bytes', [(16, 0), (256, 0), (256, 4), (256, 16), (16, 4)])
def test_scratch_layout(align, offset_bytes):
    nbytes = 1000
    view, whole = F.fenced_scratch(nbytes, align, offset_bytes)
    assert view.numel() == nbytes and (view.data_ptr() - offset_bytes) % align == 0
    assert bool((view == F.SCRATCH_FILL).all())
    start = view.data_ptr() - whole.data_ptr()
    assert start >= F.FENCE_BYTES and whole.numel() - start - nbytes >= F.FENCE_BYTES
    F.check_view(whole, view)
    view.fill_(0)                                   # the entry may leave anything in its scratch
    F.check_view(whole, view)
    whole[start + nbytes] ^= 0x10                   # one byte past what the size function promised
    with pytest.raises(F.FenceError, match=r'AFTER the payload, first at \[1000\]'):
        F.check_view(whole, view)
    whole[start + nbytes] ^= 0x10
    whole[start - 1] ^= 0x01
    with pytest.raises(F.FenceError, match=r'BEFORE the payload, nearest first at \[-1\]'):
        F.check_view(whole, view)


def test_an_empty_scratch_is_only_fences():
    view, whole = F.fenced_scratch(0, 256)
    assert view.numel() == 0
    F.check_view(whole, view)

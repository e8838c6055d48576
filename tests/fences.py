"""Fenced, poisoned, deliberately misaligned buffers for tests that own every pointer they hand to the C ABI.

One torch allocation of ``FENCE + offset + n + FENCE`` elements; the payload is the ``n`` elements that start ``offset``
elements past a 16-byte boundary (torch's allocations are at least 16-byte aligned, which ``fenced`` asserts).  The whole
allocation, payload included, is filled with one poison word, a quiet NaN with a recognisable payload, written through an
integer view: an input is then copied into its payload, an output keeps the poison.  After the call under test

  - both fences must still be bit-equal to the poison word, compared as integers - a stored ordinary NaN counts as a write;
  - no element of an output payload may still hold the poison word - that would be an element nobody wrote.

FENCE is 64 KiB on each side, by construction larger than anything one workgroup of this tree stages (a 256-pixel fp32 tile
row is 1 KiB, an 8192-key chunk of 64-bit keys 64 KiB), so a stray tile lands inside the test's own allocation: it is seen,
and it touches nobody else's memory.

A scratch buffer has the same layout, in bytes: the payload is exactly what the entry's size function promises, at the
alignment the header demands, pre-filled with 0xFF - an entry that needs a zeroed ticket has to zero it itself.
"""
import numpy as np
import torch

FENCE_BYTES = 64 * 1024
POISON = 0x7FC5A5A5                 # a quiet NaN, payload 0x45A5A5
SCRATCH_FILL = 0xFF
ALIGN = 16                          # what a 4-wide access needs; `offset` is counted from such a boundary

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _poison_word(itemsize):
    """The poison pattern as one signed integer of `itemsize` bytes (little-endian repetition / truncation of POISON)."""
    raw = np.array([POISON, POISON], dtype=np.uint32).tobytes()[:itemsize]
    if itemsize == 1:
        return int(np.frombuffer(raw, dtype=np.uint8)[0])
    return int(np.frombuffer(raw, dtype={2: np.int16, 4: np.int32, 8: np.int64}[itemsize])[0])


def _ints(t):
    """`t` (1-D, contiguous) reinterpreted as integers of its element size."""
    return t.view(_INT_VIEW[t.element_size()])


def fence_elems(dtype):
    return FENCE_BYTES // torch.empty((), dtype=dtype).element_size()


def fenced(n, dtype=torch.float32, offset=0, device='cpu'):
    """(view, whole): `whole` is one poisoned allocation of FENCE + offset + n + FENCE elements, `view` its n payload
    elements, which start `offset` elements past a 16-byte boundary."""
    n, offset = int(n), int(offset)
    assert n >= 0 and offset >= 0
    fence = fence_elems(dtype)
    whole = torch.empty(fence + offset + n + fence, dtype=dtype, device=device)
    assert whole.data_ptr() % ALIGN == 0 and (fence * whole.element_size()) % 256 == 0
    _ints(whole).fill_(_poison_word(whole.element_size()))
    return whole[fence + offset:fence + offset + n], whole


def fenced_input(t, offset=0, device=None):
    """`t` flattened into a fenced payload (its dtype, `device` or its own): (view, whole)."""
    flat = t.detach().contiguous().reshape(-1)
    view, whole = fenced(flat.numel(), flat.dtype, offset, device if device is not None else flat.device)
    view.copy_(flat)
    return view, whole


def fenced_scratch(nbytes, align=ALIGN, offset_bytes=0, device='cpu'):
    """(view, whole) of uint8: a payload of exactly `nbytes` bytes of 0xFF between two poisoned fences, starting
    `offset_bytes` bytes past an `align`-byte boundary (align a power of two up to 256)."""
    nbytes, offset_bytes = int(nbytes), int(offset_bytes)
    assert align in (4, 8, 16, 32, 64, 128, 256) and nbytes >= 0 and offset_bytes >= 0
    whole = torch.empty(FENCE_BYTES + 256 + offset_bytes + nbytes + FENCE_BYTES, dtype=torch.uint8, device=device)
    _poison_bytes(whole)
    lead = (-(whole.data_ptr() + FENCE_BYTES)) % align + offset_bytes
    start = FENCE_BYTES + lead
    view = whole[start:start + nbytes]
    view.fill_(SCRATCH_FILL)
    assert (view.data_ptr() - offset_bytes) % align == 0 or nbytes == 0
    return view, whole


def _poison_bytes(whole):
    """Fill a uint8 allocation with the poison word's bytes, phased by address so that aligned 4-byte reads see POISON."""
    pattern = np.array([POISON], dtype=np.uint32).view(np.uint8)
    phase = whole.data_ptr() % 4
    reps = np.tile(pattern, whole.numel() // 4 + 2)[phase:phase + whole.numel()]
    whole.copy_(torch.from_numpy(reps.copy()))


def _expected_bytes(whole, lo, hi):
    pattern = np.array([POISON], dtype=np.uint32).view(np.uint8)
    phase = (whole.data_ptr() + lo) % 4
    return torch.from_numpy(np.tile(pattern, (hi - lo) // 4 + 2)[phase:phase + hi - lo].copy())


class FenceError(AssertionError):
    pass


def _first(mask, limit=8):
    return mask.nonzero().flatten()[:limit].tolist()


def _problems(whole, start, n, written, name):
    itemsize = whole.element_size()
    host = whole.detach().cpu()
    if whole.dtype == torch.uint8:
        front = host[:start] != _expected_bytes(whole, 0, start)
        back = host[start + n:] != _expected_bytes(whole, start + n, host.numel())
        still = None                                  # scratch: what the entry leaves in it is its own business
    else:
        word = _poison_word(itemsize)
        bits = _ints(host)
        front = bits[:start] != word
        back = bits[start + n:] != word
        still = (bits[start:start + n] == word) if written else None
    out = []
    if front.any():
        idx = [i - start for i in front.nonzero().flatten()[-8:].flip(0).tolist()]
        out.append(f'{name}: {int(front.sum())} element(s) written BEFORE the payload, nearest first at {idx}')
    if back.any():
        out.append(f'{name}: {int(back.sum())} element(s) written AFTER the payload, first at {[n + i for i in _first(back)]}')
    if still is not None and still.any():
        out.append(f'{name}: {int(still.sum())} of {n} output element(s) never written, first at {_first(still)}')
    return out


def problems(whole, offset, n, written=True, name='buffer'):
    """What is wrong with a buffer of `fenced(n, dtype, offset)` after the call under test, as a list of strings (empty:
    nothing).  `written`: the payload is an output, every element of which must have been stored to.  Indices are
    relative to the payload (negative: the front fence)."""
    return _problems(whole, fence_elems(whole.dtype) + int(offset), int(n), written, name)


def check(whole, offset, n, written=True, name='buffer'):
    """Raise FenceError listing every broken fence and (for an output) every element never written."""
    found = problems(whole, offset, n, written, name)
    if found:
        raise FenceError('; '.join(found))


def check_view(whole, view, written=True, name='buffer'):
    """`check` for a payload given as the view `fenced` / `fenced_scratch` returned (a scratch payload's start depends on
    the allocation's address)."""
    start = view.storage_offset() - whole.storage_offset()
    found = _problems(whole, start, view.numel(), written, name)
    if found:
        raise FenceError('; '.join(found))


def snapshot(whole):
    """The bits of the whole allocation on the host (fences included), for 'nothing changed' comparisons."""
    return _ints(whole.detach().cpu().clone()) if whole.dtype != torch.uint8 else whole.detach().cpu().clone()


def unchanged(whole, before):
    now = snapshot(whole)
    return torch.equal(now, before)

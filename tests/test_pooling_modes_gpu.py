"""Kernel-level parity of the 2x2 / stride-2 pooling the plan runs (csrc/st_pool.hip through st_op_pool2x2 /
st_op_pool2x2_backward: the launcher that picks the 4-wide or the scalar kernels) in all three modes of the reference
(style_transfer.py:21-22,41-46) against plain float64 torch CPU ops:
  max      F.max_pool2d(x, 2)
  average  F.avg_pool2d(x, 2) * 2.0
  l2       F.lp_pool2d(x, 2, 2) * 0.78
The backward reference is autograd through that pool followed by where(x > 0, g, 0): the kernels apply the ReLU mask of
the convolution that produced their input.

Bars: the max forward and backward and the average backward are exact against the float64 result rounded to fp32 (a
selection, or a scaling by a power of two); the average forward and the L2 forward and backward are within 4 ulp of the
float64 value, element by element.  Every output buffer is filled with NaN before the call and carries a NaN guard past
its end: an element the kernel never writes, or one it writes out of place, cannot pass."""
import pytest
import torch
from torch.nn import functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MODES = ('max', 'average', 'l2')
ULP = 2.0 ** -23
APPROX_ULPS = 4
GUARD = 64                     # NaN floats behind every device buffer


def _hip():
    from style_transfer import _hip
    return _hip


def _relu_like(c, h, w, seed):
    """Non-negative, about a third exact zeros; every odd channel drawn from {0, 1/4, 1/2, 3/4, 1} (ties among positive
    values decide most of its max windows); some whole 2x2 windows zero (the L2 backward's 0/0)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand((c, h, w), generator=g) * 2 - 0.6).clamp_min(0)
    q = torch.floor(torch.rand((c, h, w), generator=g) * 5) / 4
    x[1::2] = q[1::2]
    z = torch.rand((c, (h + 1) // 2, (w + 1) // 2), generator=g) < 0.15
    x[z.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :h, :w]] = 0
    return x.contiguous()


def _reference(x, go, pooling):
    xd = x.double().unsqueeze(0).requires_grad_(True)
    if pooling == 'max':
        y = F.max_pool2d(xd, 2)
    elif pooling == 'average':
        y = F.avg_pool2d(xd, 2) * 2.0
    else:
        y = F.lp_pool2d(xd, 2, 2) * 0.78
    y.backward(go.double().unsqueeze(0))
    return y.detach()[0], torch.where(xd > 0, xd.grad, 0.0).detach()[0]


def _buffer(n, offset):
    """NaN-filled device buffer: (the n floats starting `offset` floats in, the whole buffer)."""
    buf = torch.full((offset + n + GUARD,), float('nan'), device=DEV)
    return buf[offset:offset + n], buf


def _run(x, go, pooling, in_offset=0, out_offset=0):
    """Forward and backward through the C ABI; the inputs start `in_offset` floats and the outputs `out_offset` floats
    past a 16-byte boundary (torch's allocations are aligned)."""
    hip = _hip()
    c, h, w = x.shape
    n_in, n_out = c * h * w, c * (h // 2) * (w // 2)
    xin, _ = _buffer(n_in, in_offset)
    xin.copy_(x.flatten())
    gout, _ = _buffer(n_out, in_offset)
    gout.copy_(go.flatten())
    y, ybuf = _buffer(n_out, out_offset)
    gin, gbuf = _buffer(n_in, out_offset)
    hip.op_pool2x2(xin.view(c, h, w), pooling, out=y)
    hip.op_pool2x2_backward(xin.view(c, h, w), gout.view(c, h // 2, w // 2), pooling, grad_in=gin)
    torch.cuda.synchronize()
    for buf, n in ((ybuf, n_out), (gbuf, n_in)):
        assert torch.isnan(buf[:out_offset]).all() and torch.isnan(buf[out_offset + n:]).all(), 'write outside the output'
    return y.view(c, h // 2, w // 2).cpu(), gin.view(c, h, w).cpu()


def _exact(name, got, want):
    bad = got.double() != want.float().double()
    print(f'[parity] {name}: {int(bad.sum())} of {got.numel()} elements differ from float64 rounded to fp32')
    assert not bad.any(), (name, bad.nonzero()[:4].tolist())


def _close(name, got, want):
    err = (got.double() - want).abs()
    ulps = float((err / want.abs().clamp_min(1e-300)).max() / ULP)
    print(f'[parity] {name}: max-abs {float(err.max()):.3e} = {float(err.max() / want.abs().max()):.2e} of max |float64|; '
          f'worst element {ulps:.2f} ulp (bar {APPROX_ULPS})')
    assert (err <= APPROX_ULPS * ULP * want.abs()).all(), (name, ulps)


def _check(name, x, go, pooling, y, gin):
    c, h, w = x.shape
    want_y, want_g = _reference(x, go, pooling)
    assert torch.isfinite(y).all() and torch.isfinite(gin).all(), name
    # the row / column that floor mode drops gets exactly 0 although its inputs are positive (the mask alone keeps
    # nothing out there)
    if h % 2:
        assert (x[:, -1] > 0).any() and (gin[:, -1] == 0).all(), name
    if w % 2:
        assert (x[:, :, -1] > 0).any() and (gin[:, :, -1] == 0).all(), name
    (_exact if pooling == 'max' else _close)(f'{name} forward', y, want_y)
    (_exact if pooling in ('max', 'average') else _close)(f'{name} backward', gin, want_g)


def _inputs(c, h, w, seed):
    x = _relu_like(c, h, w, seed)
    go = torch.randn((c, h // 2, w // 2), generator=torch.Generator().manual_seed(seed + 1))
    return x, go


def _windows(x):
    c, h, w = x.shape
    return x[:, :h // 2 * 2, :w // 2 * 2].reshape(c, h // 2, 2, w // 2, 2).permute(0, 1, 3, 2, 4).reshape(c, h // 2, w // 2, 4)


SHAPES = [  # c, h, w, input offset, output offset (floats): what the launcher runs
    (8, 64, 96, 0, 0),        # W % 4 == 0, even H: the 4-wide forward and backward
    (8, 63, 96, 0, 0),        # odd H: the 4-wide forward, the scalar backward (the dropped row)
    (5, 3, 4, 0, 0),          # ... one pooled row
    (8, 64, 94, 0, 0),        # W % 4 == 2: scalar
    (8, 65, 93, 0, 0),        # odd W and H: scalar, dropped row and column
    (16, 2, 2, 0, 0),         # one window per channel
    (64, 135, 181, 0, 0),     # conv1_2's map at 135 x 181 (pooled 67 x 90)
    (8, 64, 96, 1, 0),        # W % 4 == 0 but the inputs one float past 16 bytes: scalar fallback
    (8, 64, 96, 0, 1),        # ... the outputs one float past
    (8, 64, 96, 2, 3),
]


@pytest.mark.parametrize('c,h,w,in_offset,out_offset', SHAPES)
@pytest.mark.parametrize('pooling', MODES)
def test_pool2x2_against_float64(pooling, c, h, w, in_offset, out_offset):
    x, go = _inputs(c, h, w, seed=c * 131 + h * 7 + w)
    win = _windows(x)
    top = win.max(-1, keepdim=True).values
    ties = int(((win == top).sum(-1) > 1).logical_and(top[..., 0] > 0).sum())
    zero = int((top[..., 0] == 0).sum())
    print(f'[parity] pool {pooling} {c}x{h}x{w}: {ties} windows with a tied positive maximum, {zero} all-zero windows')
    assert ties > 0 and zero > 0
    y, gin = _run(x, go, pooling, in_offset, out_offset)
    _check(f'pool {pooling} {c}x{h}x{w} offsets {in_offset}/{out_offset}', x, go, pooling, y, gin)


@pytest.mark.parametrize('pooling', MODES)
def test_pool2x2_grid_stride_loops(pooling):
    """More windows than either launcher's grid cap (16384 x 256 threads of two windows each for the 4-wide kernels,
    8192 x 256 for the scalar ones): each thread runs its grid-stride loop several times, the last round partly."""
    c, h, w = 40, 1024, 2048
    x, go = _inputs(c, h, w, seed=7)
    assert c * (h // 2) * (w // 2) > 2 * 16384 * 256
    for offset in (0, 1):
        y, gin = _run(x, go, pooling, offset, offset)
        _check(f'pool {pooling} {c}x{h}x{w} offset {offset}', x, go, pooling, y, gin)
        del y, gin


def test_pool2x2_rejects_bad_arguments():
    hip = _hip()
    lib = hip.load_library()
    x = torch.rand((1, 4, 4), device=DEV)
    y = torch.empty((1, 2, 2), device=DEV)
    ptr, s = hip._ptr, hip._stream()
    assert lib.st_op_pool2x2(ptr(x), ptr(y), 1, 4, 4, 3, s) != 0
    assert b'mode' in lib.st_last_error()
    assert lib.st_op_pool2x2(ptr(x), ptr(y), 1, 1, 4, 0, s) != 0
    assert lib.st_op_pool2x2_backward(ptr(x), ptr(y), ptr(x), 1, 4, 4, -1, s) != 0
    assert lib.st_op_pool2x2_backward(ptr(x), ptr(y), ptr(x), 0, 4, 4, 0, s) != 0
    assert lib.st_op_pool2x2(ptr(x), ptr(y), 1, 4, 4, 0, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), F.max_pool2d(x.cpu(), 2))

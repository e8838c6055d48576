"""Every 32-bit offset at the largest map the library accepts, and the refusal one pixel count above it, on a real MI355X.

The library has ONE size limit (include/st_amd.h, "Size limit"; st_max_pixels): a map of at most 2^24 - 1 pixels.  It is what
the fp16x3 3x3 kernels prove - they stage 16 channels through a buffer resource of 64 HW bytes and use the byte offset 2^30 as
"out of range" - and profiles/size_limits.md lists the narrowest 32-bit quantity behind every entry point.  The shapes here:

  VEC   2049 x 8188 = 2^24 - 4   the most pixels a map with W % 4 == 0 can have: the 16-byte epilogues and pool kernels
  ODD   4095 x 4097 = 2^24 - 1   the limit itself, odd width: the scalar epilogues and pool kernels; floor pooling drops a
                                 row and a column
  OVER  4096 x 4096 = 2^24       one above: every entry refuses, and 20 refused calls leave the free device memory alone

with 64 channels wherever the entry takes a channel count, so that a tensor is 4 GiB: byte offsets from its base pass 2^32,
offsets inside a 32-channel output group pass 2^30 and end 128 bytes short of 2^31, and offsets inside a 16-channel input
chunk end 64 bytes short of 2^30, the kernels' out-of-range constant.

Two float64 references for the convolutions, and nothing of image size ever crosses to the host:
  whole tensor  the input is rank 2 per channel, x[c] = a_c r s^T + b_c u v^T, on a dyadic grid so that fp32 holds it exactly;
                its zero-padded 3x3 convolution is then bias + A B_co with A = [r shifted by -1, 0, +1 | u alike] (H x 6) and
                B_co (6 x W) the matching combinations of the shifted s and v: a float64 product per output channel on the
                device, compared element by element.  A dropped store, a misplaced tile, a wrong border or a channel mix-up
                anywhere in the map shows.
  windows       seeded randn operands (tests/test_kernels_gpu.py _pc_operands); 96 x 96 windows with their 1-pixel margin go to
                the host and are compared with F.conv2d in float64: the four corners, the middle of each edge, the centre, the
                last rows, and a window around every row where the byte offset inside a 16-channel input chunk or a 32-channel
                output group crosses 2^30, 2^31 or 2^32 (computed from HW; at these shapes only the output group's 2^30 exists).
Bars: tests/test_kernels_gpu.py PRECISIONS for the convolutions (whole tensor and every window alone), the bars of each other
operator's small-shape test for the rest (named at each test).  Each test prints its peak device memory and time."""
import functools
import time

import pytest
import torch
from torch.nn import functional as F

from conftest import rel_l2
import st_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MAX_PIXELS = (1 << 24) - 1
VEC, ODD, OVER = (2049, 8188), (4095, 4097), (4096, 4096)
SHAPES = [VEC, ODD]
CONV_TOL = {0: 2e-6, 4: 3e-6}          # tests/test_kernels_gpu.py PRECISIONS
WIN = 96
C = 64
LIMIT_MESSAGE = r'2\^24 - 1'


def _hip():
    from style_transfer import _hip
    return _hip


def _sid(shape):
    return f'{shape[0]}x{shape[1]}'


@pytest.fixture(autouse=True)
def _peak_memory_and_time(request):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(DEV)
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print(f'[size] {request.node.name}: peak device memory (torch) {torch.cuda.max_memory_allocated(DEV) / 2**30:.2f} GiB, '
          f'{time.perf_counter() - t0:.2f} s')
    torch.cuda.empty_cache()


def test_the_shapes_sit_where_they_claim():
    hip = _hip()
    assert hip.max_pixels() == MAX_PIXELS
    assert VEC[0] * VEC[1] == MAX_PIXELS // 4 * 4 and VEC[1] % 4 == 0          # no W % 4 == 0 map has more pixels
    assert ODD[0] * ODD[1] == MAX_PIXELS and ODD[1] % 2 == 1
    assert OVER[0] * OVER[1] == MAX_PIXELS + 1


# ---- operands -----------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _rank2(c, h, w, seed, signed):
    """x [1, c, h, w] fp32 with x[c] = a_c r s^T + b_c u v^T EXACTLY: a, b are multiples of 1/16 up to 2, r, s, u, v multiples of
    1/64 below 1, so every element is a multiple of 2^-16 below 4 - 18 bits.  Returns x and the float64 factors."""
    g = _gen(seed)
    lo = -1 if signed else 0
    vec = lambda n: torch.randint(lo * 63, 64, (n,), generator=g, device=DEV).double() / 64            # noqa: E731
    r, s, u, v = vec(h), vec(w), vec(h), vec(w)
    amp = lambda: torch.randint(1, 33, (c,), generator=g, device=DEV).double() / 16                    # noqa: E731
    a, b = amp(), amp()
    if signed:
        a = a * (torch.randint(0, 2, (c,), generator=g, device=DEV).double() * 2 - 1)
    x = a.float().view(c, 1, 1) * torch.outer(r, s).float()
    x.addcmul_(b.float().view(c, 1, 1), torch.outer(u, v).float().unsqueeze(0))
    return x.unsqueeze(0), (a, b, r, s, u, v)


def _weights(cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    wt = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (cin * 9)) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.1
    return wt.to(DEV), b.to(DEV)


def _transposed(wt):
    """The forward weight [co, ci, 3, 3] whose zero-padded cross-correlation is conv_transpose2d(., wt, padding=1)."""
    return wt.transpose(0, 1).flip(2, 3).contiguous()


def _shifted(v):
    """[3, n]: row d holds v[i + d - 1], zero where that index leaves the vector (the convolution's zero padding)."""
    z = torch.zeros(1, dtype=v.dtype, device=v.device)
    return torch.stack([torch.cat([z, v[:-1]]), v, torch.cat([v[1:], z])])


def _closed_form_errors(got, wt, bias, factors, relu):
    """(rel-L2, max-abs) of got [1, co, H, W] against the float64 closed form of the zero-padded 3x3 cross-correlation of the
    rank-2 input with wt [co, ci, 3, 3], every element, one output channel at a time on the device."""
    a, b, r, s, u, v = factors
    w64 = wt.double()
    ca, cb = torch.einsum('ocij,c->oij', w64, a), torch.einsum('ocij,c->oij', w64, b)          # [co, dy, dx]
    left = torch.cat([_shifted(r), _shifted(u)]).t().contiguous()                              # [H, 6]
    right = torch.cat([ca @ _shifted(s), cb @ _shifted(v)], dim=1)                             # [co, 6, W]
    num = torch.zeros((), dtype=torch.float64, device=DEV)
    den, worst = num.clone(), num.clone()
    for co in range(wt.shape[0]):
        ref = left @ right[co]
        if bias is not None:
            ref += bias[co].double()
        if relu:
            ref.clamp_(min=0)
        den += ref.square().sum()
        ref -= got[0, co]
        num += ref.square().sum()
        worst = torch.maximum(worst, ref.abs().max())
    return float((num / den).sqrt()), float(worst)


def _window_origins(h, w):
    """{name: (y0, x0)} of the WIN x WIN windows: see the module docstring."""
    my, mx = (h - WIN) // 2, (w - WIN) // 2
    out = {'top-left': (0, 0), 'top-right': (0, w - WIN), 'bottom-left': (h - WIN, 0), 'bottom-right': (h - WIN, w - WIN),
           'top': (0, mx), 'bottom': (h - WIN, mx), 'left': (my, 0), 'right': (my, w - WIN), 'centre': (my, mx),
           'last rows': (h - WIN, (w - WIN) // 3 | 1)}
    hw = h * w
    for group in (16, 32):                       # channels behind one buffer resource: input chunk / output group
        for bits in (30, 31, 32):
            element = (1 << bits) // 4
            ch, rest = divmod(element, hw)
            if ch >= group:
                continue                             # no such row at this shape
            y, x = divmod(rest, w)
            origin = (min(max(y - WIN // 2, 0), h - WIN), min(max(x - WIN // 2, 0), w - WIN))
            if origin not in out.values():
                out[f'byte 2^{bits} of a {group}-channel block (channel {ch}, row {y})'] = origin
    return out


def _padded_crop(t, y0, x0, margin=1):
    """t[..., y0 - margin : y0 + WIN + margin, x0 - ...] on the host in float64, zeros where that leaves the tensor."""
    (h, w), size = t.shape[-2:], WIN
    ya, yb, xa, xb = y0 - margin, y0 + size + margin, x0 - margin, x0 + size + margin
    crop = t[..., max(ya, 0):min(yb, h), max(xa, 0):min(xb, w)].cpu().double()
    return F.pad(crop, (max(-xa, 0), max(xb - w, 0), max(-ya, 0), max(yb - h, 0)))


def _check_windows(name, got, x, wt, bias, relu, tol, mask=None):
    """Every window of got [1, co, H, W] against F.conv2d in float64 on the host (wt: forward layout; mask: x counts only where
    mask > 0)."""
    h, w = x.shape[-2:]
    w64, b64 = wt.cpu().double(), None if bias is None else bias.cpu().double()
    failures = []
    for wname, (y0, x0) in _window_origins(h, w).items():
        crop = _padded_crop(x, y0, x0)
        if mask is not None:
            crop = crop * (_padded_crop(mask, y0, x0) > 0)
        want = F.conv2d(crop, w64, b64)
        if relu:
            want = want.relu()
        have = got[..., y0:y0 + WIN, x0:x0 + WIN].cpu()
        assert want.shape == have.shape == (1, wt.shape[0], WIN, WIN)
        err = rel_l2(have, want)
        print(f'[size] {name} window {wname} at ({y0}, {x0}): rel_l2={err:.3e} (tol {tol:.1e})')
        if not (torch.isfinite(have).all() and err <= tol):
            failures.append(f'{wname} at ({y0}, {x0}): {err:.3e}')
    assert not failures, f'{name}: windows above {tol:.1e}: ' + '; '.join(failures)


def _check_whole(name, got, wt, bias, factors, relu, tol):
    err, worst = _closed_form_errors(got, wt, bias, factors, relu)
    print(f'[size] {name} whole tensor vs the float64 closed form: rel_l2={err:.3e} max_abs={worst:.3e} (tol {tol:.1e})')
    assert err <= tol, f'{name}: whole tensor rel_l2 {err:.3e} > {tol:.1e} (max_abs {worst:.3e})'


def _pc_like(c, h, w, seed, relu_like):
    """tests/test_kernels_gpu.py _pc_operands on the device: a post-ReLU-like operand with a per-channel spread of scales
    (forward), plain randn (a gradient)."""
    g = _gen(seed)
    x = torch.randn((1, c, h, w), generator=g, device=DEV)
    if relu_like:
        x.relu_().mul_(torch.exp(torch.randn((1, c, 1, 1), generator=g, device=DEV)))
    return x


# ---- the 3x3 convolution ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'linear'])
@pytest.mark.parametrize('precision', [0, 4], ids=['fp32', 'fp16x3'])
@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_conv3x3_forward(shape, precision, relu):
    """st_op_conv3x3, 64 -> 64 channels: precision 0 is conv_mfma_kernel (st_conv.hip), precision 4 the producer / consumer
    kernel (st_conv_pc.hip) with the tile its cost model picks."""
    hip, (h, w), tol = _hip(), shape, CONV_TOL[precision]
    name = f'conv3x3 fwd p{precision} {C}->{C} {h}x{w} relu={relu}'
    wt, b = _weights(C, C, 11 + precision)
    x, factors = _rank2(C, h, w, 100 + h, signed=False)
    got = hip.op_conv3x3(x, wt, b, relu, precision)
    del x
    _check_whole(name, got, wt, b, factors, relu, tol)
    del got
    x = _pc_like(C, h, w, 200 + h, True)
    _check_windows(name, hip.op_conv3x3(x, wt, b, relu, precision), x, wt, b, relu, tol)


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'relu_out'])
@pytest.mark.parametrize('precision', [0, 4], ids=['fp32', 'fp16x3'])
@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_conv3x3_data_gradient(shape, precision, masked):
    """st_op_conv3x3_dgrad, 64 <- 64 channels: without a mask against both references; with relu_out (the ReLU output the
    gradient arrives at: grad_out counts only where relu_out > 0; conv_mfma_kernel's masked form at precision 0, the single-role
    conv_split_kernel at precision 4) in windows."""
    hip, (h, w), tol = _hip(), shape, CONV_TOL[precision]
    name = f'conv3x3 dgrad p{precision} {C}<-{C} {h}x{w} {"relu_out" if masked else "no mask"}'
    wt, _ = _weights(C, C, 13 + precision)
    fwd = _transposed(wt)
    if not masked:
        g, factors = _rank2(C, h, w, 300 + h, signed=True)
        got = hip.op_conv3x3_dgrad(g, None, wt, precision)
        del g
        _check_whole(name, got, fwd, None, factors, False, tol)
        del got
    g = _pc_like(C, h, w, 400 + h, False)
    mask = _pc_like(C, h, w, 500 + h, True) if masked else None          # about half of it exactly 0
    _check_windows(name, hip.op_conv3x3_dgrad(g, mask, wt, precision), g, fwd, None, False, tol, mask=mask)


PC_TILES = [(1, 32)] + [(s, tw) for s in (2, 3) for tw in (32, 16, 8)]     # tests/test_kernels_gpu.py test_conv_pc_forced_tiles


@functools.lru_cache(maxsize=1)
def _forced_tile_operands():
    h, w = VEC
    wt, b = _weights(C, C, 17)
    x, factors = _rank2(C, h, w, 600, signed=False)
    return x, factors, wt, b, {}


@pytest.fixture(scope='module')
def _forced_tile_cache():
    yield
    _forced_tile_operands.cache_clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize('tile', PC_TILES, ids=[f'shape{s}-tw{tw}' for s, tw in PC_TILES])
def test_conv_pc_forced_tiles(tile, _forced_tile_cache):
    """Every tile of conv_pc_kernel - the 512-pixel XL tile, the 256- and 128-pixel tiles in the widths 32 / 16 / 8 - once at
    the largest W % 4 == 0 shape: the float64 closed form over the whole tensor, and bit-identity between the tiles (the tile
    shape never changes the order of a pixel's K sum).  No K split exists at this size: the split's partial sums do not fit
    the convolution scratch, and forcing one is refused."""
    hip, (h, w), (shape, tw) = _hip(), VEC, tile
    x, factors, wt, b, first = _forced_tile_operands()
    with hip.options(ST_CONV_PC=2, ST_CONV_PC_SHAPE=shape, ST_CONV_PC_TW=tw, ST_CONV_PC_KSPLIT=1):
        got = hip.op_conv3x3(x, wt, b, True, 4)
    _check_whole(f'conv_pc forced tile shape {shape} width {tw} {h}x{w}', got, wt, b, factors, True, CONV_TOL[4])
    if first:
        assert torch.equal(got, first['out']), f'tile {tile} differs from tile {first["tile"]}'
    else:
        first.update(out=got, tile=tile)
    if shape == 2 and tw == 32:
        with hip.options(ST_CONV_PC=2, ST_CONV_PC_SHAPE=shape, ST_CONV_PC_TW=tw, ST_CONV_PC_KSPLIT=2):
            with pytest.raises(hip.HipLibraryError, match='does not fit'):
                hip.op_conv3x3(x, wt, b, True, 4)


# ---- pooling ------------------------------------------------------------------------------------------------------------------
ULP = 2.0 ** -23
APPROX_ULPS = 4          # tests/test_pooling_modes_gpu.py


def _exact(name, got, want):
    bad = int((got.double() != want.float().double()).sum())
    print(f'[size] {name}: {bad} of {got.numel()} elements differ from float64 rounded to fp32 (bar 0)')
    assert bad == 0, name


def _close(name, got, want):
    err = (got.double() - want).abs()
    ulps = float((err / want.abs().clamp_min(1e-300)).max() / ULP)
    print(f'[size] {name}: max-abs {float(err.max()):.3e}; worst element {ulps:.2f} ulp (bar {APPROX_ULPS})')
    assert bool((err <= APPROX_ULPS * ULP * want.abs()).all()), (name, ulps)


@pytest.mark.parametrize('pooling', ['max', 'average', 'l2'])
@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_pool2x2_forward_and_backward(shape, pooling):
    """st_op_pool2x2 / _backward on 64 channels (the 4-wide kernels at W % 4 == 0, the scalar ones at the odd width) against
    float64 pooling and its autograd on the device, every element, with the bars of tests/test_pooling_modes_gpu.py: the max
    forward and backward and the average backward exact against float64 rounded to fp32, the others within 4 ulp.  The
    backward carries the producing convolution's ReLU mask, where(x > 0, g, 0)."""
    hip, (h, w) = _hip(), shape
    g = _gen(700 + h)
    x = (torch.rand((C, h, w), generator=g, device=DEV) * 2 - 0.6).clamp_(min=0)          # about a third exact zeros
    x[1::2] = torch.floor(x[1::2] * 2.5) / 4                                               # ties among positive values
    go = torch.randn((C, h // 2, w // 2), generator=g, device=DEV)
    y = hip.op_pool2x2(x, pooling)
    gin = hip.op_pool2x2_backward(x, go, pooling)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(gin).all())
    xd = x.double().unsqueeze(0).requires_grad_(True)
    if pooling == 'max':
        want = F.max_pool2d(xd, 2)
    elif pooling == 'average':
        want = F.avg_pool2d(xd, 2) * 2.0
    else:
        want = (F.avg_pool2d(xd * xd, 2) * 4).sqrt() * 0.78          # F.lp_pool2d(xd, 2, 2) * 0.78 without its pow(): seconds at this size
    (gx,) = torch.autograd.grad(want, xd, go.double().unsqueeze(0))
    want, want_g = want.detach()[0], torch.where(xd.detach()[0] > 0, gx[0], 0.0)
    del xd, gx
    name = f'pool2x2 {pooling} {C} x {h}x{w}'
    if h % 2:
        assert bool((x[:, -1] > 0).any()) and bool((gin[:, -1] == 0).all()), 'the row floor mode drops gets exactly 0'
    if w % 2:
        assert bool((x[:, :, -1] > 0).any()) and bool((gin[:, :, -1] == 0).all()), 'the column floor mode drops gets exactly 0'
    (_exact if pooling == 'max' else _close)(f'{name} forward', y, want)
    (_exact if pooling in ('max', 'average') else _close)(f'{name} backward', gin, want_g)


# ---- the pointwise operators --------------------------------------------------------------------------------------------------
def _smooth(seed, h, w):
    """tests/test_vgg_backward_gpu.py _smooth on the device: a bicubic blow-up of a coarse image plus noise, in [0, 1]."""
    g = _gen(seed)
    low = torch.rand((1, 3, max(h // 16, 2), max(w // 16, 2)), generator=g, device=DEV)
    img = F.interpolate(low, (h, w), mode='bicubic', align_corners=False)
    return (img + (torch.rand((1, 3, h, w), generator=g, device=DEV) - 0.5) * (24 / 255)).clamp_(0, 1).contiguous()


@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_tv_loss_and_gradient(shape):
    """st_op_tv_loss against the oracle's TV loss and its autograd in float64 on the device; bars of
    tests/test_kernels_gpu.py test_tv_loss_and_gradient (value 2e-6 relative, gradient 2e-6 rel-L2)."""
    h, w = shape
    img = torch.rand((1, 3, h, w), generator=_gen(800 + h), device=DEV)
    want_loss, want_grad = O.tv_loss_grad_closed_form(img.double())
    loss, grad = _hip().op_tv_loss(img)
    rel = abs(float(loss) - float(want_loss)) / float(want_loss)
    err = float((grad.double() - want_grad).norm() / want_grad.norm())
    print(f'[size] tv loss {h}x{w}: value rel={rel:.3e} (tol 2.0e-06), gradient rel_l2={err:.3e} (tol 2.0e-06)')
    assert rel < 2e-6 and err <= 2e-6


@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_mse_loss_and_backward(shape):
    """st_op_mse_loss / _backward at count = 64 HW (2^30 elements) against float64 on the device; bars of
    tests/test_native_losses_gpu.py: value 1e-4 relative (TERM_TOL), gradient 1e-4 rel-L2 (bar() at that file's floor)."""
    hip, (h, w) = _hip(), shape
    g = _gen(900 + h)
    x = torch.randn((C, h, w), generator=g, device=DEV).relu_()
    t = torch.randn((C, h, w), generator=g, device=DEV).relu_()
    upstream = torch.tensor(0.37, device=DEV)
    value = hip.op_mse_loss(x, t)
    grad = hip.op_mse_loss_backward(x, t, upstream)
    d = x.double().sub_(t)
    want = float(d.square().mean())
    d.mul_(2 * 0.37 / d.numel())                                            # d loss / d x times the upstream scalar
    norm = float(d.norm())
    rel, err = abs(float(value) - want) / want, float(d.sub_(grad).norm()) / norm
    print(f'[size] mse {C} x {h}x{w}: value rel={rel:.3e} (tol 1.0e-04), gradient rel_l2={err:.3e} (tol 1.0e-04)')
    assert rel <= 1e-4 and err <= 1e-4


@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_channel_moments(shape):
    """st_op_channel_moments on 64 channels against float64 moments on the device; bar of test_moments_of_taps (1e-6)."""
    h, w = shape
    x = _pc_like(C, h, w, 1000 + h, True)[0]
    mean, srm = _hip().op_channel_moments(x)
    xd = x.double().flatten(1)
    em, es = rel_l2(mean.cpu(), xd.mean(1).cpu()), rel_l2(srm.cpu(), xd.square().mean(1).cpu())
    print(f'[size] channel moments {C} x {h}x{w}: mean rel_l2={em:.3e}, second moment rel_l2={es:.3e} (tol 1.0e-06)')
    assert em <= 1e-6 and es <= 1e-6


@pytest.mark.parametrize('pool', [1, 4])
@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_laplacian_kernels(shape, pool):
    """st_op_laplacian_target / _value / _backward on 3 channels against the formula of tests/test_laplacian_cpu.py in float64 on
    the device; bars of tests/test_laplacian_gpu.py test_kernels_alone: max(2e-6, 3 x the fp32 formula's own deviation)."""
    from test_laplacian_cpu import formula_terms, pooled_laplacian
    hip, (h, w) = _hip(), shape
    x, content = _smooth(1100 + h, h, w)[0], _smooth(1200 + h, h, w)[0]

    def formula(dtype):
        xi = x.to(dtype).clone().requires_grad_(True)
        value = formula_terms(xi, content.to(dtype), (pool,))[0]
        (grad,) = torch.autograd.grad(value, xi)
        return float(value), grad, pooled_laplacian(content.to(dtype), pool)

    v32, g32, t32 = formula(torch.float32)
    v64, g64, t64 = formula(torch.float64)
    rel = lambda a, b: float((a.double() - b).norm() / b.norm())          # noqa: E731
    floors = abs(v32 - v64) / abs(v64), rel(g32, g64), rel(t32, t64)
    del g32, t32
    target = hip.op_laplacian_target(content, pool)
    value, residual = hip.op_laplacian_value(x, target, pool)
    grad = hip.op_laplacian_backward(residual, x.shape, pool, torch.tensor(1.0, device=DEV))
    errs = abs(float(value) - v64) / abs(v64), rel(grad, g64), rel(target, t64)
    ok = True
    for what, err, floor in zip(('value', 'gradient', 'target'), errs, floors):
        bar = max(2e-6, 3 * floor)
        ok = ok and err <= bar
        print(f'[size] laplacian {h}x{w} p={pool}: {what} hip-vs-fp64 {err:.2e}  fp32 formula floor {floor:.2e}  bar {bar:.1e}')
    assert bool(torch.isfinite(grad).all()) and ok, (errs, floors)
    assert int(torch.count_nonzero(grad[:, h // pool * pool:, :])) == 0 and int(torch.count_nonzero(grad[:, :, w // pool * pool:])) == 0


@pytest.mark.parametrize('precision', [0, 4], ids=['fp32', 'fp16x3'])
@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_conv1x1(shape, precision):
    """st_op_conv1x1 (the style heads' gradient step), 64 -> 64 channels at npix = HW, against a float64 product on the device;
    operands and bars of tests/test_caller_buffers_gpu.py test_conv1x1: rel-L2 1e-6 (fp32) / 2e-6 (fp16x3)."""
    npix = shape[0] * shape[1]
    g = _gen(1300 + shape[0])
    x = torch.randn((C, npix), generator=g, device=DEV).relu_().mul_(torch.exp(2 * torch.randn((C, 1), generator=g, device=DEV)))
    s = torch.randn((C, C), generator=g, device=DEV) * torch.exp(3 * torch.randn((C, C), generator=g, device=DEV)) * 1e-7
    s = (s + s.t()).contiguous()
    bias = torch.randn((C,), generator=g, device=DEV) * 1e-6
    got = _hip().op_conv1x1(x, s, bias, precision)
    want = torch.addmm(bias.double()[:, None], s.double(), x.double())
    err, tol = float((got.double() - want).norm() / want.norm()), 2e-6 if precision else 1e-6
    print(f'[size] conv1x1 p{precision} {C}->{C} npix {npix}: rel_l2={err:.3e} (tol {tol:.1e})')
    assert err <= tol


# ---- a plan at the limit: conv1_1 (st_conv_first.hip), the trunk's forward and its backward ------------------------------------
CROP = 128
PLAN_TAPS = (1, 6, 11)                       # relu1_1, relu2_1, relu3_1; deeper taps live on maps of at most HW / 16 pixels
TAP_TOL = 5e-6                               # tests/test_kernels_gpu.py test_trunk_forward_taps
ABS_BAR, REL_BAR, CEILING = 1e-4, 1.5, 5e-3  # tests/test_vgg_backward_gpu.py bar()


def _geometry():
    """{tap: (stride, receptive-field radius in image pixels)} from the oracle's layer program: a 3x3 convolution widens the
    field by one pixel of its own resolution on each side, a 2x2 pool by at most one, and doubles the stride."""
    out, stride, radius = {}, 1, 0
    for idx, op, _ in O.layer_program():
        if op == 'conv':
            radius += stride
        elif op == 'pool':
            radius += stride
            stride *= 2
        out[idx] = (stride, radius)
    return out


def _crop_origins(h, w):
    """The nine window positions, origins on multiples of 4 (so that both poolings see the image's own 2x2 windows)."""
    ys = {'top': 0, 'middle': (h - CROP) // 2 // 4 * 4, 'bottom': -(-(h - CROP) // 4) * 4}
    xs = {'left': 0, 'centre': (w - CROP) // 2 // 4 * 4, 'right': -(-(w - CROP) // 4) * 4}
    return {f'{ny}-{nx}': (y, x) for ny, y in ys.items() for nx, x in xs.items()}


@functools.lru_cache(maxsize=None)
def _vgg(dtype):
    from style_transfer import vgg
    return [(a.to(dtype), b.to(dtype)) for a, b in vgg.synthetic_vgg19_weights(0)]


def _judge_crops(h, w, image, maps, cots, grad):
    """The plan's taps `maps` ({every ReLU index up to the deepest tap: map}) and image gradient `grad` for the cotangents
    `cots` ({tap: tensor}), all of the full size, against the oracle on the nine crops; returns the failures."""
    geometry = _geometry()
    margin = -(-max(geometry[t][1] for t in PLAN_TAPS) // 4) * 4
    assert margin == 16 and 4 * margin <= CROP
    torch.set_num_threads(min(16, torch.get_num_threads()))
    failures = []
    for name, (y0, x0) in _crop_origins(h, w).items():
        y1, x1 = min(y0 + CROP, h), min(x0 + CROP, w)

        def cut(t, stride, lo=0, local=False):
            """The crop of a map at `stride`, on the host; lo: image pixels trimmed from every side that is no true border;
            local: t is a map of the crop, not of the image."""
            ya, yb = (y0 + (lo if y0 > 0 else 0)) // stride, (y1 - (lo if y1 < h else 0)) // stride
            xa, xb = (x0 + (lo if x0 > 0 else 0)) // stride, (x1 - (lo if x1 < w else 0)) // stride
            oy, ox = (y0 // stride, x0 // stride) if local else (0, 0)
            return t[..., ya - oy:yb - oy, xa - ox:xb - ox].cpu()

        decisions = O.decisions_from_maps({idx: cut(m, geometry[idx][0]) for idx, m in maps.items()}, 'max')
        vjp = {}
        for dtype in (torch.float64, torch.float32):
            img = cut(image, 1).to(dtype).requires_grad_(True)
            feats = O.vgg_features(img, _vgg(dtype), PLAN_TAPS, 'max', decisions)
            (vjp[dtype],) = torch.autograd.grad([feats[t] for t in PLAN_TAPS], img,
                                                [cut(cots[t], geometry[t][0]).to(dtype) for t in PLAN_TAPS])
            if dtype == torch.float64:
                for t in PLAN_TAPS:
                    stride = geometry[t][0]
                    err = rel_l2(cut(maps[t], stride, margin), cut(feats[t].detach(), stride, margin, local=True))
                    print(f'[size] plan {h}x{w} crop {name} at ({y0}, {x0}): features[{t}] rel_l2={err:.3e} (tol {TAP_TOL:.1e})')
                    if not err <= TAP_TOL:
                        failures.append(f'{name} features[{t}]: {err:.3e}')
        g64, g32 = cut(vjp[torch.float64], 1, 2 * margin, local=True), cut(vjp[torch.float32], 1, 2 * margin, local=True)
        err, floor = rel_l2(cut(grad, 1, 2 * margin), g64), rel_l2(g32, g64)
        bar = min(CEILING, max(ABS_BAR, REL_BAR * floor))
        print(f'[size] plan {h}x{w} crop {name} at ({y0}, {x0}): image gradient hip-vs-fp64 {err:.2e}  ref-fp32 floor {floor:.2e}  '
              f'bar {bar:.1e}')
        if not err <= bar:
            failures.append(f'{name} image gradient: {err:.2e} > {bar:.1e}')
    return failures


@pytest.mark.parametrize('shape', SHAPES, ids=_sid)
def test_plan_forward_and_backward(shape):
    """st_plan_forward and st_plan_backward (seeded cotangents on relu1_1, relu2_1, relu3_1) of an fp16x3 max-pooling plan at
    the largest accepted sizes, in nine 128 x 128 crops against oracle/st_oracle.py in float64 on the branches the plan took
    (the crops of its ReLU maps: tests/test_vgg_backward_gpu.py).  A crop computes a tap pixel rightly when its receptive field
    lies inside the crop or is cut by the true image border, and an image-gradient pixel when that holds for every tap pixel
    that sees it: the margins are once and twice the deepest tap's receptive-field radius (13 -> 16 and 32 pixels), none at a
    true border.  Bars: taps 5e-6 rel-L2 (test_trunk_forward_taps), gradient min(5e-3, max(1e-4, 1.5 x the fp32 oracle's own
    deviation from float64 in the same crop)).  conv1_1's two kernels (st_conv_first.hip: forward with replicate padding, the
    data gradient that writes the image gradient) run here and nowhere else at this size."""
    hip, (h, w) = _hip(), shape
    relus = [idx for idx, op, _ in O.layer_program() if op == 'relu' and idx <= max(PLAN_TAPS)]
    image = _smooth(1400 + h, h, w)
    net = hip.Net(_vgg(torch.float32), 'max', DEV, 'fp16x3')
    t0 = time.perf_counter()
    plan = hip.Plan(net, h, w)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    plan.forward(image, max(PLAN_TAPS))
    maps = {idx: plan.feature(idx) for idx in relus}
    cots = {t: torch.randn(maps[t].shape, generator=_gen(4000 + t), device=DEV) for t in PLAN_TAPS}
    grad = plan.backward(list(PLAN_TAPS), [cots[t] for t in PLAN_TAPS])
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f'[size] plan {h}x{w}: st_plan_device_bytes {plan.device_bytes() / 2**30:.2f} GiB, create {t1 - t0:.2f} s, forward to relu3_1 + '
          f'five tap copies + backward {t2 - t1:.2f} s')
    assert bool(torch.isfinite(grad).all())
    failures = _judge_crops(h, w, image, maps, cots, grad)
    assert not failures, '; '.join(failures)


# ---- one above the limit ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _over_buffers():
    """Three tensors of 64 x 2^24 floats: what the refused entries would have read and written, had they not refused."""
    h, w = OVER
    return torch.zeros((3, C, h, w), device=DEV)


@functools.lru_cache(maxsize=1)
def _net():
    return _hip().Net(_vgg(torch.float32), 'max', DEV, 'fp16x3')


def _refusals():
    """{entry: a call on a 4096 x 4096 map}: every public entry that takes an image, a tap or a pixel count of its own."""
    from style_transfer import sharding
    hip, (h, w) = _hip(), OVER
    a, b, c = _over_buffers()
    wt, bias = _weights(C, C, 19)
    halo = torch.zeros((2, C, w), device=DEV)
    one = torch.tensor(1.0, device=DEV)
    calls = {
        'st_plan_create': lambda: hip.Plan(_net(), h, w),
        'st_plan_create_strip': lambda: sharding.StripPlan(_net(), 2 * h, w, 0, h),
        'st_head_create': lambda: hip.Head('w2', C, h, w, DEV),
        'st_op_conv1x1': lambda: hip.op_conv1x1(a.view(C, h * w), wt[:, :, 0, 0].contiguous(), bias, 4),
        'st_op_pool2x2': lambda: hip.op_pool2x2(a, 'max', out=b.view(-1)[:C * (h // 2) * (w // 2)]),
        'st_op_pool2x2_backward': lambda: hip.op_pool2x2_backward(a, b.view(-1)[:C * (h // 2) * (w // 2)], 'max', grad_in=c),
        'st_op_tv_loss': lambda: hip.op_tv_loss(a[:3].unsqueeze(0)),
        'st_op_tv_value': lambda: hip.op_tv_value(a[:3].unsqueeze(0)),
        'st_op_tv_loss_backward': lambda: hip.op_tv_loss_backward(a[:3].unsqueeze(0), one),
        'st_op_channel_moments': lambda: hip.op_channel_moments(a),
        'st_op_laplacian_target': lambda: hip.op_laplacian_target(a[:3], 1),
        'st_op_laplacian_value': lambda: hip.op_laplacian_value(a[:3], b[:3], 1),
        'st_op_laplacian_backward': lambda: hip.op_laplacian_backward(b[:3], (3, h, w), 1, one),
    }
    for precision in (0, 4):
        calls[f'st_op_conv3x3 p{precision}'] = lambda p=precision: hip.op_conv3x3(a.unsqueeze(0), wt, bias, True, p)
        calls[f'st_op_conv3x3_dgrad p{precision}'] = lambda p=precision: hip.op_conv3x3_dgrad(a.unsqueeze(0), b.unsqueeze(0), wt, p)
        calls[f'st_op_conv3x3_strip p{precision}'] = \
            lambda p=precision: hip.op_conv3x3_strip(a.unsqueeze(0), halo, True, True, wt, bias, True, False, precision=p)
        calls[f'st_op_conv3x3_strip_ex p{precision}'] = \
            lambda p=precision: hip.op_conv3x3_strip_ex(a.unsqueeze(0), None, 0, 0, wt, None, False, True, out=c.unsqueeze(0),
                                                        out_mask=b.unsqueeze(0), precision=p)
    return calls


ENTRIES = ['st_plan_create', 'st_plan_create_strip', 'st_head_create', 'st_op_conv1x1', 'st_op_pool2x2', 'st_op_pool2x2_backward',
           'st_op_tv_loss', 'st_op_tv_value', 'st_op_tv_loss_backward', 'st_op_channel_moments', 'st_op_laplacian_target',
           'st_op_laplacian_value', 'st_op_laplacian_backward'] + \
          [f'{e} p{p}' for e in ('st_op_conv3x3', 'st_op_conv3x3_dgrad', 'st_op_conv3x3_strip', 'st_op_conv3x3_strip_ex') for p in (0, 4)]


@pytest.fixture(scope='module')
def _over_cache():
    yield
    _over_buffers.cache_clear()
    _net.cache_clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize('entry', ENTRIES)
def test_one_above_the_limit_is_refused_and_leaves_no_device_memory_behind(entry, _over_cache):
    """4096 x 4096 = 2^24 pixels: the entry refuses with a message that names the limit, before it allocates anything - the
    free device memory after 20 refused calls is what it was (tests/test_kernels_gpu.py
    test_refused_winograd_calls_leave_no_device_memory_behind; the first call warms torch's cached blocks).  The buffers
    behind the pointers have the full size: a call that were not refused would stay inside them."""
    hip = _hip()
    call = _refusals()[entry]
    if entry.startswith('st_plan'):
        _net()
    refused = (hip.HipLibraryError, ValueError)           # (StripPlan raises ValueError for its shape errors)
    with pytest.raises(refused, match=LIMIT_MESSAGE):
        call()
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(DEV)[0]
    for _ in range(20):
        with pytest.raises(refused, match=LIMIT_MESSAGE):
            call()
    torch.cuda.synchronize()
    free_after = torch.cuda.mem_get_info(DEV)[0]
    print(f'[size] {entry}: 20 refused calls: free device memory {free_before / 2**20:.1f} -> {free_after / 2**20:.1f} MiB')
    assert free_after >= free_before - (4 << 20), (free_before, free_after)


def test_the_python_modules_use_the_same_limit():
    """style_transfer/losses.py decides eligibility for the native path with st_max_pixels, not a number of its own."""
    from style_transfer import losses
    assert losses._max_pixels() == MAX_PIXELS
    at = torch.empty((1, C, 1, MAX_PIXELS), device='meta')
    over = torch.empty((1, C, 1, MAX_PIXELS + 1), device='meta')
    assert losses._pixels_ok(at) and not losses._pixels_ok(over)

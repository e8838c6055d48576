"""The reference's loss modules on the library's standalone style head and pointwise entries (style_transfer/losses.py
"native dispatch"; st_head_*, st_op_mse_loss ... in include/st_amd.h), on a real MI355X.

Yardstick: this package's own module in float64 on the CPU - ``module.double()`` on ``x.double()``, the restatement that
test_module_api.py pins to the reference.  The same module in fp32 on the CPU is the reference's own fp32 floor; on exactly
the inputs below it was measured against float64 at: W2 value <= 8.6e-6, gradient <= 7.1e-6; Gram value <= 1.2e-7, gradient
<= 6.3e-7; MSE / scaled MSE <= 1.5e-7 (FLOOR).  Bars are the project's: a loss value max(1e-4, 3 x floor) (TERM_TOL rule), a
feature gradient rel-L2 min(5e-3, max(1e-4, 1.5 x floor)) (bar() of test_term_gradients_gpu.py), moments 1e-6 against float64
moments of the same input (test_moments_of_taps).  With those floors every bar evaluates to 1e-4.

Inputs: x = randn, t = 1.3 randn + 0.2 from torch.Generator().manual_seed(c * 1000 + h), as they are (signed) and through
relu.  Every module is wrapped as Scale(module, 0.37), so that the upstream gradient reaches the library as a device scalar.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_l2
import st_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ABS_BAR, REL_BAR, CEILING = 1e-4, 1.5, 5e-3      # test_term_gradients_gpu.bar()
TERM_TOL = 1e-4                                   # a loss value against a reference (test_hot_path_gpu)
GRAD_TOL = 1e-3                                   # an image gradient against a reference fixture (test_hot_path_gpu)
MOMENT_TOL = 1e-6                                 # test_moments_of_taps
UPSTREAM = 0.37
# the fp32 CPU modules against float64 on these inputs: (value, gradient)
FLOOR = {'w2': (8.6e-6, 7.1e-6), 'gram': (1.2e-7, 6.3e-7), 'mse': (1.5e-7, 1.5e-7), 'scaled_mse': (1.5e-7, 1.5e-7),
         'tv': (1.5e-7, 1.5e-7)}
SHAPES = [(64, 40, 48), (128, 20, 24), (256, 10, 12),
          (512, 5, 6),        # 30 pixels: rank-deficient covariance, a tap below one 32-pixel tile
          (512, 37, 41),      # > 1024 ragged pixels: the convolution launcher's 1x1 path, K split four ways (exact fp32 MFMA)
          (64, 45, 37),       # odd sizes
          (128, 1, 1)]        # one pixel
# Taps on which the backward's 1x1 step is the fp16x3 kernel (launch_conv1x1_split), the one consumer of the two bounds a head
# makes itself - max |F| measured in the forward and kept in the state, max |u Ssym| from head_scale_kernel.  launch_conv
# reaches it only with ksplit == 1, i.e. with more than 320 workgroups of 64 channels x 128 pixels: ceil(npix / 128) (C / 64)
# = 338 and 360 here.  Every shape of SHAPES is below that (K split on the exact fp32 MFMA, or the small-tap kernel).
BIG_SHAPES = [(64, 208, 208), (512, 72, 80)]
KINDS = ['w2', 'gram', 'mse', 'scaled_mse']
TV_IMAGES = [(40, 48), (45, 37), (1, 1)]          # (1, 1): the smallest image the TV entries accept


def value_bar(kind):
    return max(TERM_TOL, 3 * FLOOR[kind][0])


def grad_bar(kind):
    return min(CEILING, max(ABS_BAR, REL_BAR * FLOOR[kind][1]))


def _inputs(shape, relu):
    c, h, w = shape
    g = torch.Generator().manual_seed(c * 1000 + h)
    x = torch.randn((1, c, h, w), generator=g)
    t = 1.3 * torch.randn((1, c, h, w), generator=g) + 0.2
    return (x.relu(), t.relu()) if relu else (x, t)


def _build(kind, t, eps=None):
    """The fp32 module on the CPU (torch code: CPU tensors are not eligible)."""
    from style_transfer import losses as L
    kw = {} if eps is None else {'eps': eps}
    if kind == 'w2':
        return L.StyleLossW2(L.StyleLossW2.get_target(t), **kw)
    if kind == 'gram':
        return L.StyleLoss(L.StyleLoss.get_target(t), **kw)
    if kind == 'mse':
        return L.ContentLossMSE(t)
    if kind == 'scaled_mse':
        return L.ContentLoss(t, **kw)
    return L.TVLoss()


def _float64(module, x):
    """(value, gradient) of Scale(module.double(), 0.37) on x.double(), CPU."""
    from style_transfer import losses as L
    torch.set_num_threads(min(16, torch.get_num_threads()))
    crit = L.Scale(copy.deepcopy(module).double(), UPSTREAM).double()
    x64 = x.double().clone().requires_grad_(True)
    value = crit(x64)
    value.backward()
    return float(value.detach()), x64.grad.detach()


@functools.lru_cache(maxsize=None)
def _case(kind, shape, relu, eps=None):
    x, t = _inputs(shape, relu)
    module = _build(kind, t, eps)
    return (module, x) + _float64(module, x)


def _native(module, x, no_grad=False):
    """(value, gradient, the module on the device) of Scale(module, 0.37) on the device."""
    from style_transfer import losses as L
    m = copy.deepcopy(module).to(DEV)
    crit = L.Scale(m, UPSTREAM).to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    if no_grad:
        with torch.no_grad():
            return crit(xd), None, m
    value = crit(xd)
    value.backward()
    return value.detach(), xd.grad, m


def _check(tag, kind, value, grad, v64, g64):
    torch.cuda.synchronize()
    assert torch.isfinite(value).all() and torch.isfinite(grad).all(), f'{tag}: non-finite result'
    verr = abs(float(value) - v64) / abs(v64) if v64 != 0 else abs(float(value))
    gerr = rel_l2(grad.cpu(), g64) if float(g64.norm()) > 0 else float(grad.double().norm())
    print(f'[native-losses] {tag:52s} value {float(value):.8g} vs fp64 {v64:.8g} rel {verr:.2e} (bar {value_bar(kind):.0e})  '
          f'gradient rel-L2 {gerr:.2e} (bar {grad_bar(kind):.0e})')
    assert verr <= value_bar(kind), (tag, verr)
    assert gerr <= grad_bar(kind), (tag, gerr)


# ---- 1. value and feature gradient against float64, upstream 0.37 ---------------------------------------------------------
@pytest.mark.parametrize('relu', [False, True], ids=['signed', 'relu'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', KINDS)
def test_value_and_gradient_fp16x3(kind, shape, relu):
    from style_transfer import losses as L
    module, x, v64, g64 = _case(kind, shape, relu)
    before = dict(L.native_calls)
    with L.native(True, precision='fp16x3'):
        value, grad, _ = _native(module, x)
    assert L.native_calls.get(kind, 0) == before.get(kind, 0) + 1
    _check(f'{kind} {shape} {"relu" if relu else "signed"} fp16x3', kind, value, grad, v64, g64)


@pytest.mark.parametrize('inputs', ['signed', 'relu', 'zero'])
@pytest.mark.parametrize('shape', BIG_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', ['w2', 'gram'])
def test_value_and_gradient_on_the_fp16x3_1x1_kernel(kind, shape, inputs):
    """Scale(module, 0.37) at the bars of the small shapes, on taps whose 1x1 step runs in fp16x3 (BIG_SHAPES): signed, relu
    and all-zero features (bound 0: dF is the bias term alone)."""
    from style_transfer import losses as L
    module, x, v64, g64 = _case(kind, shape, inputs == 'relu')
    if inputs == 'zero':
        x = torch.zeros_like(x)
        v64, g64 = _float64(module, x)
    with L.native(True, precision='fp16x3'):
        value, grad, _ = _native(module, x)
    _check(f'{kind} {shape} {inputs} fp16x3 1x1', kind, value, grad, v64, g64)


@pytest.mark.parametrize('kind', ['w2', 'gram'])
def test_the_1x1_step_of_a_large_tap_is_the_fp16x3_kernel(kind):
    """The head's backward alone, from one state, by a fp16x3 head and by a fp32 head (which reads (Ssym, b) of the state and
    no bound): against u (Ssym F + b 1^T) in float64 both are at the gradient bar, and on a BIG shape they differ in bits -
    the fp16x3 head ran another kernel, the one that reads the state's bound on max |F| and head_scale_kernel's on max |u Ssym|
    - while on a small shape, where both split K on the fp32 MFMA, they are the same bits.  Signed features; the upstream is
    0.37 and then 1e-3 x that, so that the bound of u Ssym moves by ten binades between two backwards on one head."""
    from style_transfer import _hip
    for shape, differs in ((BIG_SHAPES[0], True), (BIG_SHAPES[1], True), ((64, 40, 48), False)):
        module, x, _, _ = _case(kind, shape, False)
        m = copy.deepcopy(module).to(DEV)
        targets = (m.mean, m.cov, m.cov_sqrt) if kind == 'w2' else (m.target,)
        eps = float(m.eps if kind == 'w2' else m.loss.eps)
        xd = x.to(DEV)[0].contiguous()
        h16, h32 = _hip.Head(kind, *shape, DEV, 'fp16x3'), _hip.Head(kind, *shape, DEV, 'fp32')
        _, state = h16.forward(xd, targets, eps)
        c = shape[0]
        ssym, b = state[:c * c].view(c, c).double().cpu(), state[c * c:c * c + c].double().cpu()
        for u in (UPSTREAM, UPSTREAM * 1e-3):
            up = torch.tensor(u, device=DEV)
            g16, g32 = h16.backward(xd, state, up), h32.backward(xd, state, up)
            torch.cuda.synchronize()
            want = float(up.double()) * (ssym @ x[0].double().flatten(1) + b[:, None])
            e16, e32 = rel_l2(g16.cpu(), want), rel_l2(g32.cpu(), want)
            print(f'[native-losses] {kind} {shape} backward alone, u = {u:g}: fp16x3 head {e16:.2e}, fp32 head {e32:.2e} '
                  f'(bar {grad_bar(kind):.0e}); same bits: {torch.equal(g16, g32)}')
            assert e16 <= grad_bar(kind) and e32 <= grad_bar(kind)
            assert torch.equal(g16, g32) != differs, (shape, u)


@pytest.mark.parametrize('relu', [False, True], ids=['signed', 'relu'])
@pytest.mark.parametrize('shape', [(512, 5, 6), (64, 40, 48)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', ['w2', 'gram'])
def test_value_and_gradient_exact_fp32(kind, shape, relu):
    from style_transfer import losses as L
    module, x, v64, g64 = _case(kind, shape, relu)
    with L.native(True, precision='fp32'):
        value, grad, m = _native(module, x)
    assert L.head_of(m).precision == 'fp32'
    _check(f'{kind} {shape} {"relu" if relu else "signed"} fp32', kind, value, grad, v64, g64)


@pytest.mark.parametrize('size', TV_IMAGES, ids=lambda s: 'x'.join(map(str, s)))
def test_tv_value_and_gradient(size):
    from style_transfer import losses as L
    g = torch.Generator().manual_seed(3000 + size[0])
    x = torch.rand((1, 3, *size), generator=g)
    module = L.TVLoss()
    v64, g64 = _float64(module, x)
    before = L.native_calls.get('tv', 0)
    with L.native(True):
        value, grad, _ = _native(module, x)
    assert L.native_calls.get('tv', 0) == before + 1
    if size == (1, 1):          # every difference is a pixel minus itself
        torch.cuda.synchronize()
        assert v64 == 0 and float(value) == 0 and not grad.any() and not g64.any()
        return
    _check(f'tv {size}', 'tv', value, grad, v64, g64)


# ---- 2. get_target ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('relu', [False, True], ids=['signed', 'relu'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_get_target_against_float64(shape, relu):
    from style_transfer import losses as L
    x, _ = _inputs(shape, relu)
    with L.native(False):
        mean64, srm64 = L.StyleLossW2.get_target(x.double())
    before = L.native_calls.get('moments', 0)
    with L.native(True):
        mean, srm = L.StyleLossW2.get_target(x.to(DEV))
        gram = L.StyleLoss.get_target(x.to(DEV))
        with_grad = L.StyleLoss.get_target(x.to(DEV).requires_grad_(True))         # differentiable: stays torch
    torch.cuda.synchronize()
    assert L.native_calls.get('moments', 0) == before + 2 and with_grad.grad_fn is not None
    assert mean.shape == mean64.shape and srm.shape == srm64.shape and gram.shape == srm64.shape
    em, es = rel_l2(mean.cpu(), mean64), rel_l2(srm.cpu(), srm64)
    print(f'[native-losses] get_target {shape} {"relu" if relu else "signed"}: mean {em:.2e} srm {es:.2e} (bar {MOMENT_TOL:.0e})')
    assert torch.equal(srm, srm.transpose(-2, -1)), 'srm is not exactly symmetric'
    assert torch.equal(gram, srm)
    assert em <= MOMENT_TOL and es <= MOMENT_TOL


# ---- 3. eps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,eps', [('w2', 1e-2), ('gram', 1e-3), ('scaled_mse', 1e-3)])
def test_eps_is_honoured(kind, eps):
    from style_transfer import losses as L
    shape = (64, 40, 48)
    x, t = _inputs(shape, False)
    if kind == 'scaled_mse':
        # t close to x: sum |d| ~ 0.8e-6 x 122880 ~ 0.1, so eps = 1e-3 moves the value by ~ 1 %
        t = x + 1e-6 * torch.randn(x.shape, generator=torch.Generator().manual_seed(7))
    module, default = _build(kind, t, eps), _build(kind, t)
    v64, g64 = _float64(module, x)
    d64, _ = _float64(default, x)
    change = abs(v64 - d64) / abs(d64)
    print(f'[native-losses] eps {kind}: float64 value {v64:.8g} with eps={eps:g}, {d64:.8g} with the default: change {change:.2e}')
    assert v64 != d64
    if kind == 'scaled_mse':
        assert change > 1e-3
    with L.native(True):
        value, grad, _ = _native(module, x)
        dvalue, _, _ = _native(default, x)
    _check(f'{kind} eps={eps:g}', kind, value, grad, v64, g64)
    assert float(value) != float(dvalue)


# ---- 4. the native path really ran -----------------------------------------------------------------------------------------------
def test_native_indicator():
    from style_transfer import losses as L
    shape = (64, 40, 48)
    bytes_of = {}
    for kind in KINDS:
        module, x, _, _ = _case(kind, shape, False)
        before = dict(L.native_calls)
        with L.native(False):
            _, _, m = _native(module, x)
        assert L.head_of(m) is None and L.native_calls == before, kind
        with L.native(True):
            _, _, m = _native(module, x)
        assert L.native_calls.get(kind, 0) == before.get(kind, 0) + 1, kind
        if kind in ('w2', 'gram'):
            head = L.head_of(m)
            assert head is not None and head.device_bytes() > 0 and head.shape == shape
            bytes_of[kind] = head.device_bytes()
            assert not any('head' in k for k in m.state_dict()), list(m.state_dict())
            # another shape: the head is replaced
            x2, _ = _inputs((64, 45, 37), False)
            with L.native(True):
                m(x2.to(DEV))
            assert L.head_of(m) is not head and L.head_of(m).shape == (64, 45, 37)
        else:
            assert L.head_of(m) is None
    torch.cuda.synchronize()
    assert bytes_of['gram'] < bytes_of['w2']          # no covariance / chain matrices, no Newton-Schulz workspace
    # C = 96 on the device: not eligible, torch as before
    x96 = torch.randn((1, 96, 5, 6), generator=torch.Generator().manual_seed(1)).to(DEV)
    assert not L.eligible(x96, 'moments') and not L.eligible(x96.double(), 'mse', (x96.double(),))
    before = dict(L.native_calls)
    with L.native(True):
        a = L.StyleLossW2.get_target(x96)
    with L.native(False):
        b = L.StyleLossW2.get_target(x96)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert L.native_calls == before


def _same_as_torch(module, x):
    """The module on either side of the switch: the same bits, or the same refusal by torch."""
    from style_transfer import losses as L
    out = []
    for on in (True, False):
        xr = x.clone().requires_grad_(True)
        try:
            with L.native(on):
                v = module(xr)
            v.backward()
            out.append((v.detach(), xr.grad))
        except RuntimeError as exc:
            out.append(type(exc))
    if isinstance(out[0], tuple):
        assert isinstance(out[1], tuple) and torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    else:
        assert out[0] == out[1]
    return out[0]


@pytest.mark.parametrize('kind', KINDS)
def test_ineligible_on_the_device_is_the_torch_code(kind):
    """fp32 features ON the device that the native path still refuses: a batch of 2, and a module whose buffers are float64
    (here the clauses behind `is_cuda` decide).  Value and gradient are torch's, bit for bit; no native call is counted - the
    Gram matrix of a refused StyleLoss does not go through the scaled-MSE entry or the head's moments either."""
    from style_transfer import losses as L
    shape = (64, 5, 6)
    x, t = _inputs(shape, False)
    buffers = {'w2': lambda m: (m.mean, m.cov, m.cov_sqrt)}.get(kind, lambda m: (m.target,))
    # batch 2
    x2, t2 = torch.cat([x, 0.5 * x + 0.1]).to(DEV), torch.cat([t, t.flip(-1)]).to(DEV)
    with L.native(False):
        m2 = _build(kind, t2)
    before = dict(L.native_calls)
    assert not L.eligible(x2, kind, buffers(m2)) and not L.eligible(x2, 'moments')
    assert isinstance(_same_as_torch(m2, x2), tuple)
    # a float64 module beside fp32 features
    m64 = copy.deepcopy(_case(kind, shape, False)[0]).double().to(DEV)
    xd = x.to(DEV)
    assert L.eligible(xd, 'moments') and not L.eligible(xd, kind, buffers(m64))
    _same_as_torch(m64, xd)           # (where torch itself refuses float64 buffers beside fp32 features, it does so on both sides)
    for on in (True, False):          # no gradient wanted: get_target by itself would go native here
        with L.native(on), torch.no_grad():
            try:
                out = m64(xd)
            except RuntimeError:
                out = None
        if on:
            first = out
    assert (first is None and out is None) or torch.equal(first, out)
    assert L.native_calls == before


# ---- 5. determinism and autograd contracts -----------------------------------------------------------------------------------
FIVE = KINDS + ['tv']


def _contract_case(kind):
    if kind == 'tv':
        from style_transfer import losses as L
        x = torch.rand((1, 3, 45, 37), generator=torch.Generator().manual_seed(3045))
        module = L.TVLoss()
        return (module, x) + _float64(module, x)
    return _case(kind, (64, 45, 37), False)


@pytest.mark.parametrize('kind', FIVE)
def test_determinism_and_autograd_contracts(kind):
    from style_transfer import losses as L
    module, x, v64, g64 = _contract_case(kind)
    with L.native(True):
        # twice from scratch: the same bits
        v1, g1, _ = _native(module, x)
        v2, g2, m = _native(module, x)
        assert torch.equal(v1, v2) and torch.equal(g1, g2)
        # no_grad: the same value, bit for bit, from the forward that skips what only the gradient needs - whether or not
        # the input says requires_grad (a head's forward then returns no state: Head.forward is watched)
        from style_transfer import _hip
        states = []
        inner = _hip.Head.forward

        def watched(self, *args, **kwargs):
            out = inner(self, *args, **kwargs)
            states.append(out[1])
            return out
        _hip.Head.forward = watched
        try:
            crit0 = L.Scale(copy.deepcopy(module).to(DEV), UPSTREAM).to(DEV)
            with torch.no_grad():
                v3 = crit0(x.to(DEV).requires_grad_(True))
                v4 = crit0(x.to(DEV))
            v5 = crit0(x.to(DEV))                      # grad mode on, nothing requires grad
            assert states == ([None] * 3 if kind in ('w2', 'gram') else []), states
            v6 = crit0(x.to(DEV).requires_grad_(True))
            assert len(states) == (4 if kind in ('w2', 'gram') else 0) and all(st is not None for st in states[3:])
        finally:
            _hip.Head.forward = inner
        assert v3.grad_fn is None and v5.grad_fn is None and v6.grad_fn is not None
        assert torch.equal(v1, v3) and torch.equal(v1, v4) and torch.equal(v1, v5) and torch.equal(v1, v6.detach())
        # one module on two inputs before one backward
        crit = L.Scale(m, UPSTREAM).to(DEV)
        other = (x.flip(-1) * 0.7 + 0.1).contiguous()
        o64v, o64g = _float64(module, other)
        xa, xb = x.to(DEV).requires_grad_(True), other.to(DEV).requires_grad_(True)
        va, vb = crit(xa), crit(xb)
        (va + vb).backward()
        _check(f'{kind} first of two inputs', kind, va.detach(), xa.grad, v64, g64)
        _check(f'{kind} second of two inputs', kind, vb.detach(), xb.grad, o64v, o64g)
        # backward(retain_graph=True) twice: exactly twice the gradient
        xc = x.to(DEV).requires_grad_(True)
        vc = crit(xc)
        vc.backward(retain_graph=True)
        once = xc.grad.clone()
        vc.backward()
        assert torch.equal(once, g1) and torch.equal(xc.grad, 2 * once)
        # an in-place write to the input between forward and backward
        xd = x.to(DEV).requires_grad_(True)
        y = xd * 1.0
        vd = crit(y)
        y.add_(1.0)
        with pytest.raises(RuntimeError, match='modified by an inplace operation'):
            vd.backward()
        # create_graph=True: the torch code's gradient, as a graph
        xe = x.to(DEV).requires_grad_(True)
        (ge,) = torch.autograd.grad(crit(xe), xe, create_graph=True)
        assert ge.requires_grad and rel_l2(ge.detach().cpu(), g64) <= grad_bar(kind)
    torch.cuda.synchronize()


# ---- 6. edge inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_all_zero_features(kind):
    from style_transfer import losses as L
    shape = (64, 40, 48)
    module, x, _, _ = _case(kind, shape, False)
    zero = torch.zeros_like(x)
    v64, g64 = _float64(module, zero)
    with L.native(True):
        value, grad, _ = _native(module, zero)
    _check(f'{kind} all-zero features', kind, value, grad, v64, g64)


@pytest.mark.parametrize('kind', ['mse', 'scaled_mse'])
def test_input_equal_to_target(kind):
    from style_transfer import losses as L
    x, _ = _inputs((64, 45, 37), False)
    module = _build(kind, x.clone())
    with L.native(True):
        value, grad, _ = _native(module, x)
    torch.cuda.synchronize()
    assert float(value) == 0 and torch.isfinite(grad).all() and not grad.any()


# ---- 7. the whole closure ----------------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _reference_style_graph(content_feat, style_moments, content_weight=0.015, tv_weight=2.0):
    """The module graph of reference stylize(), :376,427-455 (as in test_module_api.py, test_vgg_backward_gpu.py)."""
    from style_transfer.style_transfer import ContentLossMSE, LayerApply, Scale, StyleLossW2, SumLoss, TVLoss
    tv = Scale(LayerApply(TVLoss(), 'input'), tv_weight)
    content = [Scale(LayerApply(ContentLossMSE(content_feat), 22), content_weight)]
    style = [Scale(LayerApply(StyleLossW2(style_moments[layer]), layer), w)
             for layer, w in zip(O.STYLE_LAYERS, O.STYLE_LAYER_WEIGHTS)]
    return SumLoss([*content, *style, tv])


def test_reference_closure_native_and_torch_arms(vgg_weights):
    from style_transfer import losses as L
    from style_transfer.style_transfer import StyleLossW2, VGGFeatures
    g = load_golden('eval_tiny')
    styles = [_t(g[k]) for k in sorted(k for k in g if k.startswith('style') and k[5:].isdigit())]
    model = VGGFeatures(O.STYLE_LAYERS + O.CONTENT_LAYERS, str(g['pooling']), weights=vgg_weights, device=DEV)
    want, t64 = g['terms'], g['terms64']
    grads = {}
    for arm in (True, False):
        with L.native(arm):
            with torch.no_grad():
                cfeat = model(_t(g['content']).to(DEV), layers=[22])[22]
                blended = {}
                for img, w in zip(styles, list(g['style_weights'])):
                    feats = model(img.to(DEV), layers=O.STYLE_LAYERS)
                    for layer in O.STYLE_LAYERS:
                        mean, srm = StyleLossW2.get_target(feats[layer])
                        mean, srm = mean * float(w), srm * float(w)
                        if layer in blended:
                            blended[layer][0] += mean
                            blended[layer][1] += srm
                        else:
                            blended[layer] = [mean, srm]
            crit = _reference_style_graph(cfeat, blended).to(DEV)
            before = dict(L.native_calls)
            image = _t(g['image']).to(DEV).requires_grad_(True)
            feats = model(image)
            terms = [float(member(feats).detach()) for member in crit]
            crit(feats).backward()
            torch.cuda.synchronize()
            ran = {k: L.native_calls.get(k, 0) - before.get(k, 0) for k in ('w2', 'mse', 'tv')}
            assert ran == ({'w2': 10, 'mse': 2, 'tv': 2} if arm else {'w2': 0, 'mse': 0, 'tv': 0}), ran
        name = 'native' if arm else 'torch'
        for k in range(7):
            floor = abs(want[k] - t64[k]) / abs(t64[k])
            tol = max(TERM_TOL, 3 * floor) if 1 <= k <= 5 else TERM_TOL
            rel = abs(terms[k] - want[k]) / abs(want[k])
            print(f'[native-losses] eval_tiny {name} term[{O.TERM_NAMES[k]}]: got {terms[k]:.8g} want {want[k]:.8g} rel={rel:.2e} (tol {tol:.1e})')
            assert rel <= tol, (name, O.TERM_NAMES[k], rel, tol)
        err = rel_l2(image.grad.cpu(), g['grad'])
        print(f'[native-losses] eval_tiny {name} arm: image gradient vs the reference rel-L2 {err:.2e} (bar {GRAD_TOL:.0e})')
        assert err <= GRAD_TOL
        grads[arm] = image.grad.detach().cpu()
    err = rel_l2(grads[True], grads[False])
    print(f'[native-losses] eval_tiny native arm vs torch arm: rel-L2 {err:.2e} (bar {GRAD_TOL:.0e})')
    assert err <= GRAD_TOL


def _smooth(seed, h, w):
    g = torch.Generator().manual_seed(seed)
    low = torch.rand((1, 3, max(h // 16, 2), max(w // 16, 2)), generator=g)
    img = torch.nn.functional.interpolate(low, (h, w), mode='bicubic', align_corners=False)
    return (img + (torch.rand((1, 3, h, w), generator=g) - 0.5) * (24 / 255)).clamp(0, 1).contiguous()


def _mixed_graph(cfeat, moments, grams, dtype, device):
    """A kind per layer, which the fused closure's one-kind-per-list configuration cannot express: StyleLossW2 on relu1_1 /
    relu2_1, StyleLoss(eps=1e-6) on relu3_1 / relu4_1 / relu5_1; ContentLossMSE at relu4_2 and TV as in the reference."""
    from style_transfer.style_transfer import ContentLossMSE, LayerApply, Scale, StyleLoss, StyleLossW2, SumLoss, TVLoss
    members = [Scale(LayerApply(ContentLossMSE(cfeat.to(device, dtype)), 22), 0.015)]
    for layer, w in zip(O.STYLE_LAYERS, O.STYLE_LAYER_WEIGHTS):
        if layer in (1, 6):
            head = StyleLossW2(tuple(m.to(device, dtype) for m in moments[layer]))
        else:
            head = StyleLoss(grams[layer].to(device, dtype), eps=1e-6)
        members.append(Scale(LayerApply(head, layer), w))
    members.append(Scale(LayerApply(TVLoss(), 'input'), 2.0))
    return SumLoss(members).to(device, dtype)


def test_mixed_kinds_per_layer(vgg_weights):
    from style_transfer import losses as L
    from style_transfer.style_transfer import StyleLoss, StyleLossW2, VGGFeatures
    size = (40, 48)
    content, style, image = _smooth(111, *size), _smooth(112, *size), _smooth(113, *size)
    taps = sorted(set(O.STYLE_LAYERS + [22]))
    weights64 = [(a.double(), b.double()) for a, b in vgg_weights]
    with torch.no_grad():
        cfeat = O.vgg_features(content, vgg_weights, [22])[22]
        sfeats = O.vgg_features(style, vgg_weights, O.STYLE_LAYERS)
        moments = {layer: StyleLossW2.get_target(sfeats[layer]) for layer in (1, 6)}
        grams = {layer: StyleLoss.get_target(sfeats[layer]) for layer in (11, 20, 29)}
    model = VGGFeatures(taps, 'max', weights=vgg_weights, device=DEV, precision='fp16x3')
    before = dict(L.native_calls)
    with L.native(True):
        crit = _mixed_graph(cfeat, moments, grams, torch.float32, DEV)
        x = image.to(DEV).requires_grad_(True)
        crit(model(x)).backward()
    torch.cuda.synchronize()
    ran = {k: L.native_calls.get(k, 0) - before.get(k, 0) for k in ('w2', 'gram', 'mse', 'tv')}
    assert ran == {'w2': 2, 'gram': 3, 'mse': 1, 'tv': 1}, ran
    plan = model.plan_for(*size)
    relus = [idx for idx, op, _ in O.layer_program() if op == 'relu']
    decisions = O.decisions_from_maps({idx: plan.feature(idx).cpu() for idx in relus}, 'max')
    refs = {}
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for dtype in (torch.float32, torch.float64):
        img = image.to(dtype).clone().requires_grad_(True)
        feats = O.vgg_features(img, vgg_weights if dtype == torch.float32 else weights64, taps, 'max', decisions)
        _mixed_graph(cfeat, moments, grams, dtype, 'cpu')(feats).backward()
        refs[dtype] = img.grad.detach()
    assert torch.isfinite(x.grad).all()
    err, floor = rel_l2(x.grad.cpu(), refs[torch.float64]), rel_l2(refs[torch.float32], refs[torch.float64])
    b = min(CEILING, max(ABS_BAR, REL_BAR * floor))
    print(f'[native-losses] 40x48 W2 (1, 6) + Gram eps=1e-6 (11, 20, 29) + MSE 22 + TV: hip-vs-fp64 {err:.2e}  ref-fp32 floor '
          f'{floor:.2e}  bar {b:.1e}')
    assert err <= b

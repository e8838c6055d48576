"""The backward of the HIP trunk for gradients that arrive at the taps from outside (st_plan_backward, Plan.backward, and
VGGFeatures as a differentiable module), on a real MI355X.

Yardstick: the one of test_term_gradients_gpu.py.  The vector-Jacobian product of st_oracle.vgg_features in float64, evaluated
on the branches the plan's own forward took (every ReLU map read back with plan.feature, st_oracle.decisions_from_maps): what
is left between the two is arithmetic.  floor = rel-L2 of the fp32 oracle's VJP against the float64 one on the same branches;
a VJP passes when rel-L2(HIP, float64) <= min(5e-3, max(1e-4, 1.5 x floor)) - that file's bar(), same constants.  Cotangents
are seeded torch.randn of the tap's shape, images that file's _smooth, weights synthetic_vgg19_weights(0).

"The seven default taps" are what VGGFeatures returns for the default layers: 'input' (the caller's tensor; its gradient
is autograd's own) and features 1, 6, 11, 20, 22, 29.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_l2
import st_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ABS_BAR, REL_BAR, CEILING = 1e-4, 1.5, 5e-3      # test_term_gradients_gpu.bar()
FOLD_TOL = 1e-5                                   # several seeds at once vs the sum of the single-seed passes (same file)
TERM_TOL = 1e-4                                   # a loss value against a reference fixture (test_hot_path_gpu)
GRAD_TOL = 1e-3                                   # an image gradient against a reference fixture (test_hot_path_gpu)
ALL_LAYERS = [1, 3, 4, 6, 8, 9, 11, 13, 15, 17, 18, 20, 22, 24, 26, 27, 29]     # what st_plan_feature accepts
RELUS = [idx for idx, op, _ in O.layer_program() if op == 'relu']
NINE = ['input', 1, 6, 11, 13, 20, 22, 27, 29]    # the seven default taps + a non-default ReLU (13) + a pool output (27)


def bar(floor):
    return min(CEILING, max(ABS_BAR, REL_BAR * floor))


def _smooth(seed, h, w):
    g = torch.Generator().manual_seed(seed)
    low = torch.rand((1, 3, max(h // 16, 2), max(w // 16, 2)), generator=g)
    img = torch.nn.functional.interpolate(low, (h, w), mode='bicubic', align_corners=False)
    return (img + (torch.rand((1, 3, h, w), generator=g) - 0.5) * (24 / 255)).clamp(0, 1).contiguous()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def _weights():
    from style_transfer import vgg
    return vgg.synthetic_vgg19_weights(0)


@functools.lru_cache(maxsize=None)
def _weights64():
    return [(a.double(), b.double()) for a, b in _weights()]


def _cot(tap, shape):
    g = torch.Generator().manual_seed(4000 + (0 if tap == 'input' else int(tap)))
    return torch.randn(tuple(shape), generator=g)


def _decisions(plan, pooling, last_layer=29):
    """The branches of the plan's current forward (a plain forward writes every ReLU map)."""
    torch.cuda.synchronize()
    return O.decisions_from_maps({idx: plan.feature(idx).cpu() for idx in RELUS if idx <= last_layer}, pooling)


def _oracle_vjps(image, pooling, decisions, cots, groups, dtype):
    """One oracle forward in `dtype` on the given branches; the VJP of each group of taps (cotangents `cots`)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    img = image.to(dtype).clone().requires_grad_(True)
    trunk = sorted({t for group in groups for t in group if t != 'input'})
    feats = O.vgg_features(img, _weights() if dtype == torch.float32 else _weights64(), trunk, pooling, decisions)
    out = []
    for k, group in enumerate(groups):
        (g,) = torch.autograd.grad([feats[t] for t in group], img, [cots[t].to(dtype) for t in group],
                                   retain_graph=k + 1 < len(groups))
        out.append(g.detach())
    return out


def _judge(tag, got, g64, g32, failures):
    assert torch.isfinite(got).all(), f'{tag}: non-finite gradient'
    err, floor = rel_l2(got.cpu(), g64), rel_l2(g32, g64)
    b = bar(floor)
    print(f'[vgg-bwd] {tag:44s} hip-vs-fp64 {err:.2e}  ref-fp32 floor {floor:.2e}  bar {b:.1e}  '
          f'{"PASS" if err <= b else "FAIL"}')
    if not err <= b:
        failures.append(f'{tag}: rel-L2 {err:.2e} > {b:.1e} (floor {floor:.2e})')


def _plan(size, pooling='max', precision='fp16x3'):
    from style_transfer import _hip as hip
    net = hip.Net(_weights(), pooling, DEV, precision)
    return net, hip.Plan(net, *size)


# ---- 1. every tap alone ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny():
    """40 x 48, max pooling, fp16x3: the plan behind a full forward, its branches, a cotangent per tap and the oracle's
    single-seed VJPs of all 17 taps in fp32 and float64."""
    size = (40, 48)
    image = _smooth(91, *size)
    net, plan = _plan(size)
    img = image.to(DEV)
    plan.forward(img, 29)
    decisions = _decisions(plan, 'max')
    cots = {layer: _cot(layer, plan.feature(layer).shape) for layer in ALL_LAYERS}
    groups = [(layer,) for layer in ALL_LAYERS]
    g32 = dict(zip(ALL_LAYERS, _oracle_vjps(image, 'max', decisions, cots, groups, torch.float32)))
    g64 = dict(zip(ALL_LAYERS, _oracle_vjps(image, 'max', decisions, cots, groups, torch.float64)))
    return dict(net=net, plan=plan, img=img, image=image, cots=cots, g32=g32, g64=g64, decisions=decisions)


@pytest.mark.parametrize('layer', ALL_LAYERS)
def test_every_tap_alone(layer):
    """One seed: the top of the pass is this layer (masked there if it is a ReLU, not if it is a pool), and everything below
    it receives a written, not an accumulated, gradient."""
    ref = _tiny()
    plan = ref['plan']
    plan.forward(ref['img'], 29)
    got = plan.backward([layer], [ref['cots'][layer].to(DEV)])
    torch.cuda.synchronize()
    failures = []
    _judge(f'40x48-max-fp16x3 features[{layer}] alone', got, ref['g64'][layer], ref['g32'][layer], failures)
    assert not failures, '; '.join(failures)


# ---- 2. several seeds, shapes and arithmetics --------------------------------------------------------------------------------
CASES = [
    ((21, 16), 'max', 'fp16x3'),          # relu5_1 is 1 x 1
    ((135, 181), 'max', 'fp16x3'),        # odd rows and widths: floor-mode pooling drops a row and a column; scalar tails
    ((135, 181), 'average', 'fp16x3'),
    ((135, 181), 'l2', 'fp16x3'),
    ((135, 181), 'max', 'fp32'),
    ((135, 181), 'max', 'bf16x6'),
    ((128, 128), 'max', 'fp16x3'),        # the default run's first scale; W % 4 == 0 vector paths
]


def _case_id(case):
    (h, w), pooling, precision = case
    return f'{h}x{w}-{pooling}-{precision}'


def _module(size, pooling, precision, layers):
    from style_transfer.style_transfer import VGGFeatures
    return VGGFeatures(layers, pooling, weights=_weights(), device=DEV, precision=precision)


@pytest.mark.parametrize('case', CASES, ids=[_case_id(c) for c in CASES])
def test_nine_seeds_through_the_module(case):
    """VGGFeatures on an image that requires grad: cotangents at the seven default taps, relu3_2 (13) and pool4 (27) at
    once, through torch.autograd - the data gradients accumulate into seeded ReLU nodes and into a seeded pool node, and
    'input' is autograd's own."""
    size, pooling, precision = case
    name = _case_id(case)
    image = _smooth(92, *size)
    model = _module(size, pooling, precision, [t for t in NINE if t != 'input'])
    x = image.to(DEV).requires_grad_(True)
    feats = model(x)
    assert feats['input'] is x and all(feats[t].grad_fn is not None for t in NINE if t != 'input')
    decisions = _decisions(model.plan_for(*size), pooling)
    cots = {t: _cot(t, feats[t].shape) for t in NINE}
    (got,) = torch.autograd.grad([feats[t] for t in NINE], x, [cots[t].to(DEV) for t in NINE])
    torch.cuda.synchronize()
    (g32,) = _oracle_vjps(image, pooling, decisions, cots, [tuple(NINE)], torch.float32)
    (g64,) = _oracle_vjps(image, pooling, decisions, cots, [tuple(NINE)], torch.float64)
    failures = []
    _judge(f'{name} nine seeds', got, g64, g32, failures)
    assert not failures, '; '.join(failures)


POOL_FEEDERS = [3, 4, 8, 9, 17, 18, 26, 29]   # relu1_2, 2_2, 3_4, 4_4 feed a pool; pool1, pool2, pool3 (4, 9, 18) are seeded
                                              # below the top as well: conv2_1's, 3_1's and 4_1's data gradients accumulate into them


@pytest.mark.parametrize('size,pooling', [((40, 48), 'max'), ((135, 181), 'max'), ((135, 181), 'l2')],
                         ids=['40x48-max', '135x181-max', '135x181-l2'])
def test_seeds_at_the_convs_that_feed_a_pool(size, pooling):
    """A pooling backward WRITES its input's gradient, so the seed of a ReLU that feeds a pool is added behind it (the one
    place where the seeding kernel accumulates) - none of the cases above has such a seed below the top of the pass.  At
    40 x 48 the same pass is repeated with cotangents whose pointers are not 16-byte aligned: the kernel's element-wise path
    must give the same bits as its 16-byte one."""
    image = _smooth(99, *size)
    net, plan = _plan(size, pooling)
    plan.forward(image.to(DEV), 29)
    decisions = _decisions(plan, pooling)
    cots = {layer: _cot(layer, plan.feature(layer).shape) for layer in POOL_FEEDERS}
    got = plan.backward(POOL_FEEDERS, [cots[layer].to(DEV) for layer in POOL_FEEDERS]).clone()
    torch.cuda.synchronize()
    (g32,) = _oracle_vjps(image, pooling, decisions, cots, [tuple(POOL_FEEDERS)], torch.float32)
    (g64,) = _oracle_vjps(image, pooling, decisions, cots, [tuple(POOL_FEEDERS)], torch.float64)
    failures = []
    _judge(f'{size[0]}x{size[1]}-{pooling}-fp16x3 seeds {POOL_FEEDERS}', got, g64, g32, failures)
    assert not failures, '; '.join(failures)
    if size == (40, 48):
        shifted = []
        for layer in POOL_FEEDERS:
            buf = torch.empty(cots[layer].numel() + 1, device=DEV)
            buf[1:] = cots[layer].flatten().to(DEV)
            shifted.append(buf[1:].view(cots[layer].shape))
            assert shifted[-1].data_ptr() % 16 == 4 and shifted[-1].is_contiguous()
        again = plan.backward(POOL_FEEDERS, shifted)
        torch.cuda.synchronize()
        assert torch.equal(got, again)


# ---- 3. accumulation ---------------------------------------------------------------------------------------------------------
def test_nine_seeds_equal_the_sum_of_nine_single_seeds():
    """Linearity in the cotangents: all nine at once against the sum of nine passes with one each, over ONE forward."""
    size = (40, 48)
    model = _module(size, 'max', 'fp16x3', [t for t in NINE if t != 'input'])
    x = _smooth(93, *size).to(DEV).requires_grad_(True)
    feats = model(x)
    cots = {t: _cot(t, feats[t].shape).to(DEV) for t in NINE}
    (joint,) = torch.autograd.grad([feats[t] for t in NINE], x, [cots[t] for t in NINE], retain_graph=True)
    singles = [torch.autograd.grad(feats[t], x, cots[t], retain_graph=True)[0] for t in NINE]
    torch.cuda.synchronize()
    fold = rel_l2(sum(g.double() for g in singles).cpu(), joint.cpu())
    print(f'[vgg-bwd] 40x48-max-fp16x3 sum of nine single-seed VJPs vs the nine together: rel-L2 {fold:.2e} (bar {FOLD_TOL:.0e})')
    assert fold <= FOLD_TOL


# ---- 4. truncation -----------------------------------------------------------------------------------------------------------
def test_backward_of_a_truncated_forward():
    from style_transfer import _hip as hip
    size = (40, 48)
    image = _smooth(94, *size)
    net, plan = _plan(size)
    plan.forward(image.to(DEV), 22)
    decisions = _decisions(plan, 'max', 22)
    cots = {layer: _cot(layer, plan.feature(layer).shape) for layer in (11, 22)}
    got = plan.backward([22, 11], [cots[22].to(DEV), cots[11].to(DEV)])
    torch.cuda.synchronize()
    (g32,) = _oracle_vjps(image, 'max', decisions, cots, [(11, 22)], torch.float32)
    (g64,) = _oracle_vjps(image, 'max', decisions, cots, [(11, 22)], torch.float64)
    failures = []
    _judge('40x48-max-fp16x3 forward(22), seeds 22 + 11', got, g64, g32, failures)
    assert not failures, '; '.join(failures)
    with pytest.raises(hip.HipLibraryError, match='beyond'):
        plan.backward([29], [torch.zeros((1, 512, 2, 3), device=DEV)])


# ---- 5. state ----------------------------------------------------------------------------------------------------------------
def _with_targets(plan, img):
    """Targets from the image itself, so that the plan's closure can run."""
    plan.forward(img, 29)
    plan.set_content_target_from_forward()
    for i, layer in enumerate(O.STYLE_LAYERS):
        plan.set_style_target(i, *plan.moments(layer))


def test_two_backwards_over_one_forward_are_bit_identical():
    """The backward re-establishes every gradient bound it reads: the second pass does not see the first one's maxima."""
    size = (40, 48)
    net, plan = _plan(size)
    plan.forward(_smooth(95, *size).to(DEV), 29)
    layers = [1, 6, 11, 13, 20, 22, 27, 29]
    big = [_cot(layer, plan.feature(layer).shape).to(DEV) * 64 for layer in layers]
    small = [g / 4096 for g in big]
    first = plan.backward(layers, small).clone()
    plan.backward(layers, big)                       # larger maxima in between
    again = plan.backward(layers, small)
    torch.cuda.synchronize()
    assert torch.equal(first, again)


def test_backward_refuses_what_it_cannot_differentiate():
    from style_transfer import _hip as hip
    size = (40, 48)
    net, plan = _plan(size)
    img = _smooth(96, *size).to(DEV)
    g22 = torch.zeros((1, 512, 5, 6), device=DEV)
    with pytest.raises(hip.HipLibraryError, match='no st_plan_forward is current'):       # a fresh plan
        plan.backward([22], [g22])
    _with_targets(plan, img)
    plan.forward(img, 29)
    plan.backward([22], [g22])
    plan.loss_and_grad(img)                          # a closure: fused pools leave argmax codes instead of maps
    with pytest.raises(hip.HipLibraryError, match='no st_plan_forward is current'):
        plan.backward([22], [g22])
    plan.forward(img, 29)
    with pytest.raises(hip.HipLibraryError, match='named twice'):
        plan.backward([22, 22], [g22, g22])
    with pytest.raises(hip.HipLibraryError, match='at least one'):
        plan.backward([], [])
    # a conv index (21 = conv4_2) is no tap: the binding's shape check and the entry itself both say so
    with pytest.raises(hip.HipLibraryError, match='not a ReLU or pooling output'):
        plan.backward([21], [g22])
    out = torch.empty((1, 3, *size), device=DEV)
    rc = plan.lib.st_plan_backward(plan.handle, 1, (hip.ctypes.c_int * 1)(21), (hip.ctypes.c_void_p * 1)(g22.data_ptr()),
                                   hip._ptr(out), hip._stream())
    assert rc != 0 and b'st_plan_backward: features[21] is not a ReLU or pooling output' in plan.lib.st_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize('between', ['forward', 'closure'])
def test_module_recomputes_when_the_plan_has_moved_on(between):
    """Between the module's forward and .backward() the same plan runs another image of the same size, or a fused closure:
    the autograd node notices the plan's forward counter, runs the forward again and gives the uninterrupted result."""
    size = (40, 48)
    image, other = _smooth(97, *size), _smooth(98, *size)
    taps = [1, 6, 11, 20, 22, 29]
    model = _module(size, 'max', 'fp16x3', taps)
    plan = model.plan_for(*size)
    _with_targets(plan, other.to(DEV))
    x = image.to(DEV).requires_grad_(True)
    feats = model(x)
    decisions = _decisions(plan, 'max')
    cots = {t: _cot(t, feats[t].shape) for t in taps}
    (straight,) = torch.autograd.grad([feats[t] for t in taps], x, [cots[t].to(DEV) for t in taps], retain_graph=True)
    count = plan.forward_count
    if between == 'forward':
        with torch.no_grad():
            model(other.to(DEV))
    else:
        plan.loss_and_grad(other.to(DEV))
    assert plan.forward_count == count + 1
    (got,) = torch.autograd.grad([feats[t] for t in taps], x, [cots[t].to(DEV) for t in taps])
    torch.cuda.synchronize()
    assert plan.forward_count == count + 2           # exactly one recompute
    (g32,) = _oracle_vjps(image, 'max', decisions, cots, [tuple(taps)], torch.float32)
    (g64,) = _oracle_vjps(image, 'max', decisions, cots, [tuple(taps)], torch.float64)
    print(f'[vgg-bwd] 40x48 recompute after a {between}: against the uninterrupted pass rel-L2 {rel_l2(got.cpu(), straight.cpu()):.2e}')
    failures = []
    _judge(f'40x48-max-fp16x3 backward after another {between}', got, g64, g32, failures)
    assert not failures, '; '.join(failures)


# ---- 6. the reference's closure on the HIP trunk ----------------------------------------------------------------------------
def _reference_style_graph(content_feat, style_moments, content_weight=0.015, tv_weight=2.0):
    """The module graph of reference stylize(), :376,427-455 (as in test_module_api.py)."""
    from style_transfer.style_transfer import ContentLossMSE, LayerApply, Scale, StyleLossW2, SumLoss, TVLoss
    tv = Scale(LayerApply(TVLoss(), 'input'), tv_weight)
    content = [Scale(LayerApply(ContentLossMSE(content_feat), 22), content_weight)]
    style = [Scale(LayerApply(StyleLossW2(style_moments[layer]), layer), w)
             for layer, w in zip(O.STYLE_LAYERS, O.STYLE_LAYER_WEIGHTS)]
    return SumLoss([*content, *style, tv])


def test_reference_closure_on_the_hip_trunk(vgg_weights):
    """feats = model(image); loss = crit(feats); loss.backward() (style_transfer.py:472-476) with this package's VGGFeatures
    and loss modules, against the reference's own terms and gradient (eval_tiny, 40 x 48) and against the fused closure."""
    from style_transfer import _hip as hip
    from style_transfer.style_transfer import StyleLossW2, VGGFeatures
    g = load_golden('eval_tiny')
    styles = [_t(g[k]) for k in sorted(k for k in g if k.startswith('style') and k[5:].isdigit())]
    model = VGGFeatures(O.STYLE_LAYERS + O.CONTENT_LAYERS, str(g['pooling']), weights=vgg_weights, device=DEV)
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
    image = _t(g['image']).to(DEV).requires_grad_(True)
    feats = model(image)
    terms = [float(member(feats).detach()) for member in crit]
    total = crit(feats)
    total.backward()
    torch.cuda.synchronize()
    want, t64 = g['terms'], g['terms64']
    for k in range(7):
        floor = abs(want[k] - t64[k]) / abs(t64[k])
        tol = max(TERM_TOL, 3 * floor) if 1 <= k <= 5 else TERM_TOL
        rel = abs(terms[k] - want[k]) / abs(want[k])
        print(f'[vgg-bwd] eval_tiny term[{O.TERM_NAMES[k]}]: got {terms[k]:.8g} want {want[k]:.8g} rel={rel:.2e} (tol {tol:.1e})')
        assert rel <= tol, (O.TERM_NAMES[k], rel, tol)
    err = rel_l2(image.grad.cpu(), g['grad'])
    print(f'[vgg-bwd] eval_tiny module closure on the HIP trunk: image gradient vs the reference rel-L2 {err:.2e} (bar {GRAD_TOL:.0e})')
    assert err <= GRAD_TOL
    # the fused closure on the same targets
    plan = hip.Plan(model.net, *image.shape[2:])
    plan.set_content_target(cfeat[0])
    for i, layer in enumerate(O.STYLE_LAYERS):
        plan.set_style_target(i, blended[layer][0][0], blended[layer][1][0])
    plan.set_loss_weights(0.015, O.STYLE_LAYER_WEIGHTS, 2.0)
    _, fused = plan.loss_and_grad(image.detach())
    torch.cuda.synchronize()
    err = rel_l2(image.grad.cpu(), fused.cpu())
    print(f'[vgg-bwd] eval_tiny module closure vs plan.loss_and_grad on the same targets: rel-L2 {err:.2e} (bar {GRAD_TOL:.0e})')
    assert err <= GRAD_TOL


# ---- 7. a loss the fused closure cannot express ----------------------------------------------------------------------------
def _gatys_graph(content_feats, grams, dtype, device):
    """Gatys et al.: Gram-matrix StyleLoss at the five style taps, ContentLoss (ScaledMSE) at relu4_2 AND relu5_1, TV."""
    from style_transfer.style_transfer import ContentLoss, LayerApply, Scale, StyleLoss, SumLoss, TVLoss
    members = [Scale(LayerApply(ContentLoss(content_feats[layer].to(device, dtype)), layer), 0.015) for layer in (22, 29)]
    members += [Scale(LayerApply(StyleLoss(grams[layer].to(device, dtype)), layer), w)
                for layer, w in zip(O.STYLE_LAYERS, O.STYLE_LAYER_WEIGHTS)]
    members.append(Scale(LayerApply(TVLoss(), 'input'), 2.0))
    return SumLoss(members).to(device, dtype)


def test_gram_style_and_two_content_layers():
    from style_transfer.style_transfer import StyleLoss
    size = (40, 48)
    content, style, image = _smooth(101, *size), _smooth(102, *size), _smooth(103, *size)
    taps = sorted(set(O.STYLE_LAYERS + [22]))
    with torch.no_grad():
        cfeats = O.vgg_features(content, _weights(), [22, 29])
        sfeats = O.vgg_features(style, _weights(), O.STYLE_LAYERS)
        grams = {layer: StyleLoss.get_target(sfeats[layer]) for layer in O.STYLE_LAYERS}
    model = _module(size, 'max', 'fp16x3', taps)
    crit = _gatys_graph(cfeats, grams, torch.float32, DEV)
    x = image.to(DEV).requires_grad_(True)
    loss = crit(model(x))
    loss.backward()
    decisions = _decisions(model.plan_for(*size), 'max')
    refs = {}
    for dtype in (torch.float32, torch.float64):
        img = image.to(dtype).clone().requires_grad_(True)
        feats = O.vgg_features(img, _weights() if dtype == torch.float32 else _weights64(), taps, 'max', decisions)
        _gatys_graph(cfeats, grams, dtype, 'cpu')(feats).backward()
        refs[dtype] = img.grad.detach()
    failures = []
    _judge('40x48 Gram StyleLoss x 5 + ContentLoss 22, 29 + TV', x.grad, refs[torch.float64], refs[torch.float32], failures)
    assert not failures, '; '.join(failures)
    # a working loop: five Adam steps on the pixels through this closure.  lr = 2e-3: the first-order decrease of a step is
    # lr |g|_1, the curvature terms are O(lr^2) - a step 10 x below the reference's default 0.02 cannot overshoot here
    x.grad = None
    opt = torch.optim.Adam([x], lr=2e-3)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = crit(model(x))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(crit(model(x))))
    print('[vgg-bwd] 40x48 Gatys loss over five Adam steps: ' + ' '.join(f'{v:.6g}' for v in losses))
    assert all(np.isfinite(losses)) and all(b < a for a, b in zip(losses, losses[1:])), losses

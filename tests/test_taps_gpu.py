"""Configurable content / style layers (st_plan_set_taps, the general closure, StyleTransfer.content_layers / style_layers)
on a real MI355X.

Yardstick: oracle/st_oracle.py composed by hand - vgg_features, feature_moments, style_target, style_w2, content_mse, tv_loss
in SumLoss order (content terms, style terms, tv) - in float64 and in float32, on the plan's own branches
(decisions_from_maps on the maps of a plain plan.forward to the deepest configured layer, which is the forward the general
closure runs), as test_vgg_backward_gpu.py does.  The HIP plan and the oracle get the SAME targets: the fp32 oracle's features
of a content image and its moments of a style image.

Bars, the project's own:
  image gradient   rel-L2 against float64 <= min(5e-3, max(1e-4, 1.5 x floor)), floor = the fp32 oracle's own distance from
                   float64 (test_term_gradients_gpu.bar);
  each weighted term  |hip - fp32 oracle| / |fp32 oracle| <= max(1e-4, 3 x the fp32 oracle's deviation of that term from
                   float64) (test_hot_path_gpu._term_tols);
  the 8-float array's total against the float32 sum of the terms: 1e-6 relative (test_bench_contract_gpu).
Images are test_vgg_backward_gpu's _smooth, weights synthetic_vgg19_weights(0).
"""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_l2
import st_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ABS_BAR, REL_BAR, CEILING = 1e-4, 1.5, 5e-3      # test_term_gradients_gpu.bar()
TERM_TOL = 1e-4                                   # test_hot_path_gpu._term_tols
SUM_TOL = 1e-6                                    # test_bench_contract_gpu: [7] against the sum of the terms
DEFAULT = ([22], [1, 6, 11, 20, 29])
RELUS = [idx for idx, op, _ in O.layer_program() if op == 'relu']
CONFIGS = {
    'a': ([20], [1, 6, 11, 20, 29]),             # a shallower content tap
    'b': ([22, 29], [1, 6, 11, 20, 29]),         # two content layers; 29 is in both lists
    'c': ([22], [1, 6, 11, 20]),                 # the backward starts at a content tap; the forward stops at 22
    'd': ([18], [1, 13, 27]),                    # a pool output as content; a non-x_1 ReLU and a pool output as style
    'e': ([22], [3, 8, 17, 26]),                 # Gatys-like relu*_2 / last-of-block style layers: each feeds a pool
    'f': ([], [6]),
    'g': ([11], []),
}
TV_WEIGHT = 2.0


def bar(floor):
    return min(CEILING, max(ABS_BAR, REL_BAR * floor))


def _smooth(seed, h, w):
    g = torch.Generator().manual_seed(seed)
    low = torch.rand((1, 3, max(h // 16, 2), max(w // 16, 2)), generator=g)
    img = torch.nn.functional.interpolate(low, (h, w), mode='bicubic', align_corners=False)
    return (img + (torch.rand((1, 3, h, w), generator=g) - 0.5) * (24 / 255)).clamp(0, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _weights():
    from style_transfer import vgg
    return vgg.synthetic_vgg19_weights(0)


@functools.lru_cache(maxsize=None)
def _weights64():
    return [(a.double(), b.double()) for a, b in _weights()]


def _layer_weights(content_layers, style_layers):
    """content_weight / len(content_layers) per layer (:366); the reference's 4^-k style weights over the layers named."""
    raw = [256, 64, 16, 4, 1][:len(style_layers)]
    return [0.015 / max(len(content_layers), 1)] * len(content_layers), [w / sum(raw) for w in raw]


@functools.lru_cache(maxsize=None)
def _inputs(size, pooling):
    """Image, and the fp32 oracle's features of a content and a style image at all 17 taps (shared by every configuration)."""
    h, w = size
    sh = max(16, h * 200 // 256)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    with torch.no_grad():
        cfeats = O.vgg_features(_smooth(71, h, w), _weights(), list(range(1, 30)), pooling)
        sfeats = O.vgg_features(_smooth(72, sh, w), _weights(), list(range(1, 30)), pooling)
    return dict(image=_smooth(73, h, w), cfeats=cfeats, sfeats=sfeats)


def _targets(size, pooling, content_layers, style_layers):
    inp = _inputs(size, pooling)
    return ({layer: inp['cfeats'][layer] for layer in content_layers},
            {layer: O.feature_moments(inp['sfeats'][layer]) for layer in style_layers})


def _oracle(image, pooling, decisions, content_layers, style_layers, ctargets, moments, weights, dtype):
    """SumLoss (:455) composed from the oracle's parts in `dtype`: (weighted terms, total, image gradient)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cws, sws = weights
    img = image.to(dtype).clone().requires_grad_(True)
    feats = O.vgg_features(img, _weights() if dtype == torch.float32 else _weights64(), content_layers + style_layers,
                           pooling, decisions)
    terms = [O.content_mse(feats[layer], ctargets[layer].to(dtype)) * cw for layer, cw in zip(content_layers, cws)]
    for layer, sw in zip(style_layers, sws):
        mean, srm = moments[layer]
        terms.append(O.style_w2(feats[layer], O.style_target(mean.to(dtype), srm.to(dtype))) * sw)
    terms.append(O.tv_loss(img) * TV_WEIGHT)
    total = sum(terms)
    (grad,) = torch.autograd.grad(total, img)
    return [float(t.detach()) for t in terms], float(total.detach()), grad.detach()


def _configured_plan(size, pooling, precision, content_layers, style_layers, configure=True):
    from style_transfer import _hip as hip
    net = hip.Net(_weights(), pooling, DEV, precision)
    plan = hip.Plan(net, *size)
    if configure:
        plan.set_taps(content_layers, style_layers)
    _set_targets(plan, size, pooling, content_layers, style_layers)
    plan.set_loss_weights(*_layer_weights(content_layers, style_layers), TV_WEIGHT)
    return net, plan


def _set_targets(plan, size, pooling, content_layers, style_layers):
    ctargets, moments = _targets(size, pooling, content_layers, style_layers)
    for i, layer in enumerate(content_layers):
        plan.set_content_target(ctargets[layer].to(DEV), i)
    for i, layer in enumerate(style_layers):
        plan.set_style_target(i, moments[layer][0].to(DEV), moments[layer][1].to(DEV))


def _judge(tag, plan, img, image, pooling, content_layers, style_layers, closure):
    """One closure of `plan` against the oracle on the branches of the plan's plain forward to the deepest layer."""
    deepest = max(content_layers + style_layers)
    plan.forward(img, deepest)
    torch.cuda.synchronize()
    decisions = O.decisions_from_maps({idx: plan.feature(idx).cpu() for idx in RELUS if idx <= deepest}, pooling)
    losses, grad = closure()
    torch.cuda.synchronize()
    terms = plan.term_losses().cpu().double().numpy()
    losses = losses.cpu().numpy()
    weights = _layer_weights(content_layers, style_layers)
    ctargets, moments = _targets(tuple(image.shape[2:]), pooling, content_layers, style_layers)
    t32, _, g32 = _oracle(image, pooling, decisions, content_layers, style_layers, ctargets, moments, weights, torch.float32)
    t64, _, g64 = _oracle(image, pooling, decisions, content_layers, style_layers, ctargets, moments, weights, torch.float64)
    names = [f'content[{layer}]' for layer in content_layers] + [f'style[{layer}]' for layer in style_layers] + ['tv']
    failures = []
    assert len(terms) == len(names), (len(terms), names)
    for k, name in enumerate(names):
        floor = abs(t32[k] - t64[k]) / abs(t64[k])
        tol = max(TERM_TOL, 3 * floor)
        rel = abs(terms[k] - t32[k]) / abs(t32[k])
        print(f'[taps] {tag} term {name:12s} got {terms[k]:.8g} want {t32[k]:.8g} rel {rel:.2e}  floor {floor:.2e}  '
              f'bar {tol:.1e}  {"PASS" if rel <= tol else "FAIL"}')
        if not rel <= tol:
            failures.append(f'{tag}: term {name} rel {rel:.2e} > {tol:.1e}')
    want_total = np.float32(0)
    for t in terms.astype(np.float32):
        want_total = np.float32(want_total + t)
    rel_total = abs(float(losses[7]) - float(want_total)) / abs(float(want_total))
    print(f'[taps] {tag} total {losses[7]:.8g} vs fp32 sum of the terms {want_total:.8g} rel {rel_total:.2e} (bar {SUM_TOL:.0e})')
    if not rel_total <= SUM_TOL:
        failures.append(f'{tag}: total rel {rel_total:.2e} > {SUM_TOL:.0e}')
    assert torch.isfinite(grad).all(), f'{tag}: non-finite gradient'
    err, floor = rel_l2(grad.cpu(), g64), rel_l2(g32, g64)
    b = bar(floor)
    print(f'[taps] {tag} gradient hip-vs-fp64 {err:.2e}  ref-fp32 floor {floor:.2e}  bar {b:.1e}  {"PASS" if err <= b else "FAIL"}')
    if not err <= b:
        failures.append(f'{tag}: gradient rel-L2 {err:.2e} > {b:.1e} (floor {floor:.2e})')
    return terms, losses, grad, failures


def _state(img):
    return img.clone(), torch.zeros_like(img), torch.zeros_like(img), (1 - torch.tensor(0.99)).to(DEV) * img


# ---- 1. the default configuration is the existing closure -------------------------------------------------------------------
def test_configured_with_the_default_layers_is_the_unconfigured_plan_bit_for_bit():
    size = (40, 48)
    img = _inputs(size, 'max')['image'].to(DEV)
    _, plain = _configured_plan(size, 'max', 'fp16x3', *DEFAULT, configure=False)
    la, ga = plain.loss_and_grad(img)
    la, ga = la.clone(), ga.clone()
    xa, ma, va, ea = _state(img)
    steps_a = [plain.step(xa, ma, va, ea, k, 0.02).clone() for k in (1, 2, 3)]
    torch.cuda.synchronize()
    assert torch.isfinite(la).all() and torch.isfinite(ga).all()        # (this half runs without the feature too)
    _, conf = _configured_plan(size, 'max', 'fp16x3', *DEFAULT, configure=True)
    lb, gb = conf.loss_and_grad(img)
    lb, gb, terms_b = lb.clone(), gb.clone(), conf.term_losses()
    xb, mb, vb, eb = _state(img)
    steps_b = [conf.step(xb, mb, vb, eb, k, 0.02).clone() for k in (1, 2, 3)]
    torch.cuda.synchronize()
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    assert all(torch.equal(a, b) for a, b in zip(steps_a, steps_b))
    assert torch.equal(xa, xb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(ea, eb)
    assert torch.equal(terms_b, lb[:7])


# ---- 2. the general closure on the default layers ---------------------------------------------------------------------------
@pytest.mark.parametrize('size', [(40, 48), (72, 88)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_general_closure_on_the_default_layers(size):
    """ST_GENERAL_TAPS=1 sends the default configuration through the general closure: seven terms in SumLoss order and the
    gradient against the oracle; its distance from the fast path is printed."""
    from style_transfer import _hip as hip
    image = _inputs(size, 'max')['image']
    img = image.to(DEV)
    _, plan = _configured_plan(size, 'max', 'fp16x3', *DEFAULT)
    fast_l, fast_g = plan.loss_and_grad(img)
    fast_l, fast_g = fast_l.clone(), fast_g.clone()
    tag = f'{size[0]}x{size[1]}-max-fp16x3 default layers, general closure'
    with hip.options(ST_GENERAL_TAPS=1):
        terms, losses, grad, failures = _judge(tag, plan, img, image, 'max', *DEFAULT, lambda: plan.loss_and_grad(img))
    assert len(terms) == 7
    assert np.array_equal(terms.astype(np.float32), losses[:7])          # the 8-float array keeps its meaning
    print(f'[taps] {tag}: against the fast path: gradient rel-L2 {rel_l2(grad.cpu(), fast_g.cpu()):.2e}, total '
          f'{abs(float(losses[7]) - float(fast_l[7])) / abs(float(fast_l[7])):.2e}')
    assert not failures, '; '.join(failures)


# ---- 3. custom configurations -----------------------------------------------------------------------------------------------
CUSTOM = [(name, 'max', 'fp16x3') for name in CONFIGS] + [('d', 'average', 'fp16x3'), ('d', 'l2', 'fp16x3'), ('b', 'max', 'fp32')]


@pytest.mark.parametrize('name, pooling, precision', CUSTOM, ids=lambda v: str(v))
def test_custom_configuration(name, pooling, precision):
    size = (40, 48)
    content_layers, style_layers = CONFIGS[name]
    image = _inputs(size, pooling)['image']
    img = image.to(DEV)
    _, plan = _configured_plan(size, pooling, precision, content_layers, style_layers)
    tag = f'({name}) content {content_layers} style {style_layers} 40x48-{pooling}-{precision}'
    terms, losses, grad, failures = _judge(tag, plan, img, image, pooling, content_layers, style_layers,
                                           lambda: plan.loss_and_grad(img))
    nc, ns = len(content_layers), len(style_layers)
    # the 8-float array of a non-default configuration: content sum, style sum, zeros, tv, total
    t32 = terms.astype(np.float32)
    assert np.isclose(losses[0], t32[:nc].sum(), rtol=SUM_TOL) and np.isclose(losses[1], t32[nc:nc + ns].sum(), rtol=SUM_TOL)
    assert not losses[2:6].any() and losses[6] == t32[-1]
    assert not failures, '; '.join(failures)


# ---- 4. the step entries ----------------------------------------------------------------------------------------------------
def test_step_is_loss_and_grad_plus_update_bit_for_bit():
    size = (40, 48)
    img = _inputs(size, 'max')['image'].to(DEV)
    _, plan = _configured_plan(size, 'max', 'fp16x3', *CONFIGS['b'])
    xa, ma, va, ea = _state(img)
    xb, mb, vb, eb = _state(img)
    for k in (1, 2, 3):
        la = plan.step(xa, ma, va, ea, k, 0.02).clone()
        lb, g = plan.loss_and_grad(xb)
        lb = lb.clone()
        plan.apply_update(xb, g, mb, vb, eb, k, 0.02)
        torch.cuda.synchronize()
        assert torch.equal(la, lb), (k, la, lb)
        assert torch.equal(xa, xb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(ea, eb), k
    assert not torch.equal(xa, img)


def test_lbfgs_step_is_loss_and_grad_plus_update_bit_for_bit():
    from style_transfer import _hip as hip
    size = (40, 48)
    img = _inputs(size, 'max')['image'].to(DEV)
    _, plan = _configured_plan(size, 'max', 'fp16x3', *CONFIGS['b'])
    xa, _, _, ea = _state(img)
    xb, _, _, eb = _state(img)
    opt_a, opt_b = hip.LBFGS(xa), hip.LBFGS(xb)
    for k in (1, 2, 3):
        la = opt_a.step(plan, xa, ea, 0.99).clone()
        lb, g = plan.loss_and_grad(xb)
        lb = lb.clone()
        opt_b.update(xb, g, eb, 0.99)
        torch.cuda.synchronize()
        assert torch.equal(la, lb), (k, la, lb)
        assert torch.equal(xa, xb) and torch.equal(ea, eb), k
    assert opt_a.info() == opt_b.info() and opt_a.info()['n_iter'] == 3
    assert not torch.equal(xa, img)


# ---- 5. errors --------------------------------------------------------------------------------------------------------------
def test_errors():
    from style_transfer import _hip as hip
    from style_transfer import sharding
    size = (48, 48)
    net = hip.Net(_weights(), 'max', DEV, 'fp16x3')
    strip = sharding.StripPlan(net, 48, 48, 0, 32)
    with pytest.raises(hip.HipLibraryError, match='strip'):
        strip.set_taps([20], [1, 6])
    plan = hip.Plan(net, *size)
    with pytest.raises(hip.HipLibraryError, match='pre-ReLU'):
        plan.set_taps([2], [1, 6])
    with pytest.raises(hip.HipLibraryError, match='twice'):
        plan.set_taps([22], [1, 6, 6])
    with pytest.raises(hip.HipLibraryError, match='0 to 16'):
        plan.set_taps(list(hip.TAPS), [1])
    with pytest.raises(hip.HipLibraryError, match='empty'):
        plan.set_taps([], [])
    # a closure before every configured target is set names the missing one
    img = _smooth(73, *size).to(DEV)
    plan.set_taps([20, 22], [3])
    plan.forward(img, 22)
    plan.set_content_target(plan.feature(20), 0)
    with pytest.raises(hip.HipLibraryError, match=r'content target 1 \(features\[22\]\)'):
        plan.loss_and_grad(img)
    plan.set_content_target(plan.feature(22), 1)
    with pytest.raises(hip.HipLibraryError, match=r'style target 0 \(features\[3\]\)'):
        plan.loss_and_grad(img)
    plan.set_style_target(0, *plan.moments(3))
    losses, grad = plan.loss_and_grad(img)
    assert torch.isfinite(losses).all() and torch.isfinite(grad).all()
    # ... and set_taps drops them again, for the same lists too
    plan.set_taps([20, 22], [3])
    with pytest.raises(hip.HipLibraryError, match='content target 0'):
        plan.loss_and_grad(img)


# ---- 6. one store of heads, targets and weights: what sharing a position between configurations must not change ----------------
SIZE = (40, 48)
SHARED = ([22], [1, 6])         # relu1_1 and relu2_1: heads of the default lists too, here with bound words 48 and 49


def _leg(plan, img, steps):
    """(losses, gradient, terms[, the three steps' losses, the state after them]) of `plan` as it is configured now."""
    losses, grad = plan.loss_and_grad(img)
    out = [losses.clone(), grad.clone(), plan.term_losses().clone()]
    if steps:
        state = _state(img)
        out += [plan.step(*state, k, 0.02).clone() for k in (1, 2, 3)]
        out += list(state)
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in out)
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_head_that_two_configurations_share():
    """Default lists, then SHARED, then the default lists again, on ONE plan: the outer legs are equal bit for bit and the
    middle one is a fresh plan's - no target, bound word or fused Gram of a former configuration is left behind."""
    img = _inputs(SIZE, 'max')['image'].to(DEV)
    _, plan = _configured_plan(SIZE, 'max', 'fp16x3', *DEFAULT, configure=False)
    first = _leg(plan, img, steps=True)
    for lists, name in ((SHARED, 'middle'), (DEFAULT, 'last')):
        plan.set_taps(*lists)
        _set_targets(plan, SIZE, 'max', *lists)
        plan.set_loss_weights(*_layer_weights(*lists), TV_WEIGHT)
        if name == 'middle':
            middle = _leg(plan, img, steps=False)
        else:
            last = _leg(plan, img, steps=True)
    _, fresh = _configured_plan(SIZE, 'max', 'fp16x3', *SHARED)
    want = _leg(fresh, img, steps=False)
    assert len(middle[2]) == 4 and _same(middle, want)
    assert len(first) == 10 and _same(first, last)
    assert not torch.equal(first[6], img)


def test_set_taps_drops_the_targets_of_shared_positions():
    from style_transfer import _hip as hip
    img = _inputs(SIZE, 'max')['image'].to(DEV)
    _, plan = _configured_plan(SIZE, 'max', 'fp16x3', *DEFAULT, configure=False)
    _leg(plan, img, steps=True)
    plan.set_taps(*SHARED)          # relu4_2, relu1_1 and relu2_1 all had a target a moment ago
    with pytest.raises(hip.HipLibraryError, match=r'content target 0 \(features\[22\]\)'):
        plan.loss_and_grad(img)
    ctargets, moments = _targets(SIZE, 'max', *SHARED)
    plan.set_content_target(ctargets[22].to(DEV), 0)
    with pytest.raises(hip.HipLibraryError, match=r'style target 0 \(features\[1\]\)'):
        plan.loss_and_grad(img)
    plan.set_style_target(0, moments[1][0].to(DEV), moments[1][1].to(DEV))
    with pytest.raises(hip.HipLibraryError, match=r'style target 1 \(features\[6\]\)'):
        plan.loss_and_grad(img)


def test_moments_do_not_depend_on_the_configuration():
    from style_transfer import _hip as hip
    img = _inputs(SIZE, 'max')['image'].to(DEV)
    net = hip.Net(_weights(), 'max', DEV, 'fp16x3')
    plans = {name: hip.Plan(net, *SIZE) for name in ('plain', 'default', 'other')}
    plans['default'].set_taps(*DEFAULT)
    plans['other'].set_taps([20], [1, 29])
    layers = (1, 6, 11, 20, 29, 4, 22)

    def all_moments():
        got = {}
        for name, plan in plans.items():
            plan.forward(img, 29)
            got[name] = {layer: [t.clone() for t in plan.moments(layer)] for layer in layers}
        torch.cuda.synchronize()
        return got

    unfused = all_moments()
    for layer in layers:
        assert all(torch.isfinite(t).all() for t in unfused['plain'][layer]), layer
        assert _same(unfused['plain'][layer], unfused['default'][layer]), layer
        assert _same(unfused['plain'][layer], unfused['other'][layer]), layer
    # relu1_1's Gram out of conv1_1's launch: the reference's lists only, and then on both plans that have them
    with hip.options(ST_CONV1_GRAM_IN_FORWARD=1):
        fused = all_moments()
    for layer in layers:
        assert _same(fused['plain'][layer], fused['default'][layer]), layer
        if layer != 1:
            assert _same(fused['plain'][layer], fused['other'][layer]), layer
    assert _same(fused['other'][1], unfused['other'][1])


def test_weights_across_set_taps():
    """The default lists named again keep the plan's weights; every other change of lists resets them to the new lists'
    defaults (the tv weight is not a per-layer weight: set_taps leaves it alone)."""
    img = _inputs(SIZE, 'max')['image'].to(DEV)
    reference = _layer_weights(*DEFAULT)[1]
    _, plan = _configured_plan(SIZE, 'max', 'fp16x3', *DEFAULT, configure=False)
    plan.set_loss_weights(0.03, [2 * w for w in reference], 4.0)
    before = _leg(plan, img, steps=False)
    plan.set_taps(*DEFAULT)
    _set_targets(plan, SIZE, 'max', *DEFAULT)
    assert _same(_leg(plan, img, steps=False), before)
    from style_transfer import _hip as hip
    fresh = hip.Plan(plan.net, *SIZE)            # the weights a plan is created with: 0.015, 4^-k / 341, tv 2
    _set_targets(fresh, SIZE, 'max', *DEFAULT)
    want = _leg(fresh, img, steps=False)
    assert not torch.equal(want[0], before[0])
    _, plan = _configured_plan(SIZE, 'max', 'fp16x3', *DEFAULT, configure=False)
    plan.set_loss_weights(0.03, [2 * w for w in reference], TV_WEIGHT)       # (TV_WEIGHT is a fresh plan's 2.0, so `want` holds)
    plan.set_taps([20, 22], [3])
    plan.set_taps(*DEFAULT)
    _set_targets(plan, SIZE, 'max', *DEFAULT)
    assert _same(_leg(plan, img, steps=False), want)


# ---- 7. stylize() -----------------------------------------------------------------------------------------------------------
def _pil(seed, w, h):
    """A smooth synthetic image with every pixel well inside (0, 1): no clamp engages during the few iterations below."""
    from PIL import Image
    arr = (_smooth(seed, h, w)[0] * 0.5 + 0.25).movedim(0, 2).numpy()
    return Image.fromarray(np.uint8(np.round(arr * 255)))


@pytest.mark.parametrize('optimizer', ['adam', 'lbfgs'])
def test_stylize_reads_the_layer_attributes(optimizer):
    from PIL import Image
    from style_transfer import StyleTransfer
    from style_transfer.style_transfer import size_to_fit, to_tensor
    st = StyleTransfer(devices=[DEV], pooling='max', weights='synthetic')
    st.content_layers, st.style_layers = [20, 22], [1, 6, 11]
    st.style_weights = [w / 21 for w in (16, 4, 1)]
    content_image, style_image = _pil(81, 64, 48), _pil(82, 60, 44)
    decay = 0.99
    seen = []

    def callback(it):
        if it.i == 1:
            # The first callback of a scale fires AFTER its first update, so get_image_tensor() no longer returns the starting
            # image x0 the reported loss belongs to: it returns the EMA (decay x0 + x1) / (1 + decay), and st.image is x1.  x0 is
            # solved from the two.  That costs about two fp32 roundings per pixel (~1e-7 of a value near 0.5, random in sign),
            # three orders below the 1e-4 bar on the loss, and needs get_image_tensor()'s clamp to be a no-op: _pil keeps
            # every pixel in [0.25, 0.75] and 6 Adam steps of 0.02 cannot reach 0 or 1.
            avg, x1 = st.get_image_tensor(), st.image.detach()[0]
            seen.append((it.w, it.h, it.loss, (((1 + decay) * avg - x1) / decay).cpu()[None]))

    out = st.stylize(content_image, [style_image], end_scale=64, min_scale=45, initial_iterations=6, iterations=4,
                     optimizer=optimizer, avg_decay=decay, callback=callback)
    result = st.get_image_tensor()
    assert out is not None and torch.isfinite(result).all() and len(seen) == 2
    cws, sws = [0.015 / 2] * 2, st.style_weights
    for (w, h, loss, start), scale in zip(seen, (45, 64)):
        assert (w, h) == size_to_fit(content_image.size, scale, scale_up=True)
        content = to_tensor(content_image.resize((w, h), Image.BICUBIC))[None]
        sw_, sh_ = size_to_fit(style_image.size, scale)
        style = to_tensor(style_image.resize((sw_, sh_), Image.BICUBIC))[None]
        with torch.no_grad():
            cfeats = O.vgg_features(content, _weights(), st.content_layers, 'max')
            sfeats = O.vgg_features(style, _weights(), st.style_layers, 'max')
        moments = {layer: O.feature_moments(sfeats[layer]) for layer in st.style_layers}
        args = (start, 'max', None, st.content_layers, st.style_layers, cfeats, moments, (cws, sws))
        _, total32, _ = _oracle(*args, torch.float32)
        _, total64, _ = _oracle(*args, torch.float64)
        floor = abs(total32 - total64) / abs(total64)
        tol, rel = max(TERM_TOL, 3 * floor), abs(loss - total32) / abs(total32)
        print(f'[taps] stylize {optimizer} {w}x{h}: first loss {loss:.8g} oracle {total32:.8g} rel {rel:.2e} floor {floor:.2e} '
              f'bar {tol:.1e}')
        assert rel <= tol, f'{optimizer} {w}x{h}: first loss rel {rel:.2e} > {tol:.1e}'
    st.content_layers = [2]
    with pytest.raises(ValueError, match='pre-ReLU'):
        st.stylize(content_image, [style_image], end_scale=64, min_scale=45, initial_iterations=1, iterations=1)

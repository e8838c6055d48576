"""The loss kinds (st_plan_set_loss_kinds, StyleTransfer.content_loss / style_loss) on a real MI355X: the reference's StyleLoss
(a Gram matrix under ScaledMSELoss) and ContentLoss (the features under ScaledMSELoss) in the fused closure.

Inputs and yardstick are tests/test_taps_gpu.py's: its _smooth images 71 (content), 72 (style), 73 (the iterate),
synthetic_vgg19_weights(0), and oracle/st_oracle.py composed by hand in float32 and in float64 on the branches of the plan's
own plain forward (decisions_from_maps).  The two new terms are written out below in torch (_scaled_mse, _gram).  Both sides
get the SAME targets: the fp32 oracle's features of image 71 and its (mean, second raw moment) of image 72 - the second raw
moment is the Gram target.

Bars, the project's own (test_taps_gpu):
  each weighted term  |hip - fp32 oracle| / |fp32 oracle| <= max(1e-4, 3 x the fp32 oracle's deviation from float64);
  the total           within 1e-6 of the fp32 sum of the terms;
  image gradient      rel-L2 against float64 <= min(5e-3, max(1e-4, 1.5 x the fp32 oracle's own rel-L2 from float64)).
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_l2
import st_oracle as O
import test_taps_gpu as T

pytestmark = pytest.mark.gpu
DEV = T.DEV
KINDS = ('scaled_mse', 'gram')
SIZE = (40, 48)      # pooled sizes 20, 10, 5, 2 (an odd one); tap counts that are and are not multiples of 4


def _scaled_mse(x, t):
    d = x - t
    return d.pow(2).sum() / (d.abs().sum() + 1e-8)


def _gram(feat):
    flat = feat.flatten(-2)[0]
    return flat @ flat.T / flat.shape[-1]


def _oracle(image, pooling, decisions, content_layers, style_layers, ctargets, moments, weights, kinds, dtype):
    """SumLoss composed in `dtype` with the given kinds: (weighted terms, total, image gradient)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cws, sws = weights
    img = image.to(dtype).clone().requires_grad_(True)
    terms = []
    feats = O.vgg_features(img, T._weights() if dtype == torch.float32 else T._weights64(), content_layers + style_layers,
                           pooling, decisions)
    for layer, cw in zip(content_layers, cws):
        target = ctargets[layer].to(dtype)
        terms.append((O.content_mse(feats[layer], target) if kinds[0] == 'mse' else _scaled_mse(feats[layer], target)) * cw)
    for layer, sw in zip(style_layers, sws):
        mean, srm = moments[layer]
        if kinds[1] == 'w2':
            terms.append(O.style_w2(feats[layer], O.style_target(mean.to(dtype), srm.to(dtype))) * sw)
        else:
            terms.append(_scaled_mse(_gram(feats[layer]), srm.to(dtype)) * sw)
    terms.append(O.tv_loss(img) * T.TV_WEIGHT)
    total = sum(terms)
    (grad,) = torch.autograd.grad(total, img)
    return [float(t.detach()) for t in terms], float(total.detach()), grad.detach()


def _plan(size, pooling, precision, content_layers, style_layers, kinds, configure=True):
    """A plan on the lists with the kinds, test_taps_gpu's targets and weights.  kinds None: set_loss_kinds is never called."""
    from style_transfer import _hip as hip
    net = hip.Net(T._weights(), pooling, DEV, precision)
    plan = hip.Plan(net, *size)
    if configure:
        plan.set_taps(content_layers, style_layers)
    if kinds is not None:
        plan.set_loss_kinds(*kinds)
    T._set_targets(plan, size, pooling, content_layers, style_layers)
    plan.set_loss_weights(*T._layer_weights(content_layers, style_layers), T.TV_WEIGHT)
    return net, plan


def _judge(tag, plan, img, image, pooling, content_layers, style_layers, kinds, closure):
    """One closure of `plan` against the oracle on the branches of the plan's plain forward to the deepest layer."""
    deepest = max(content_layers + style_layers)
    plan.forward(img, deepest)
    torch.cuda.synchronize()
    decisions = O.decisions_from_maps({idx: plan.feature(idx).cpu() for idx in T.RELUS if idx <= deepest}, pooling)
    losses, grad = closure()
    torch.cuda.synchronize()
    terms = plan.term_losses().cpu().double().numpy()
    losses = losses.cpu().numpy()
    weights = T._layer_weights(content_layers, style_layers)
    ctargets, moments = T._targets(tuple(image.shape[2:]), pooling, content_layers, style_layers)
    args = (image, pooling, decisions, content_layers, style_layers, ctargets, moments, weights, kinds)
    t32, _, g32 = _oracle(*args, torch.float32)
    t64, _, g64 = _oracle(*args, torch.float64)
    names = [f'content[{layer}]' for layer in content_layers] + [f'style[{layer}]' for layer in style_layers] + ['tv']
    failures = []
    assert len(terms) == len(names), (len(terms), names)
    for k, name in enumerate(names):
        floor = abs(t32[k] - t64[k]) / abs(t64[k])
        tol = max(T.TERM_TOL, 3 * floor)
        rel = abs(terms[k] - t32[k]) / abs(t32[k])
        print(f'[kinds] {tag} term {name:12s} got {terms[k]:.8g} want {t32[k]:.8g} rel {rel:.2e}  floor {floor:.2e}  '
              f'bar {tol:.1e}  {"PASS" if rel <= tol else "FAIL"}')
        if not rel <= tol:
            failures.append(f'{tag}: term {name} rel {rel:.2e} > {tol:.1e}')
    want_total = np.float32(0)
    for t in terms.astype(np.float32):
        want_total = np.float32(want_total + t)
    rel_total = abs(float(losses[7]) - float(want_total)) / abs(float(want_total))
    print(f'[kinds] {tag} total {losses[7]:.8g} vs fp32 sum of the terms {want_total:.8g} rel {rel_total:.2e} (bar {T.SUM_TOL:.0e})')
    if not rel_total <= T.SUM_TOL:
        failures.append(f'{tag}: total rel {rel_total:.2e} > {T.SUM_TOL:.0e}')
    assert torch.isfinite(grad).all(), f'{tag}: non-finite gradient'
    err, floor = rel_l2(grad.cpu(), g64), rel_l2(g32, g64)
    b = T.bar(floor)
    print(f'[kinds] {tag} gradient hip-vs-fp64 {err:.2e}  ref-fp32 floor {floor:.2e}  bar {b:.1e}  {"PASS" if err <= b else "FAIL"}')
    if not err <= b:
        failures.append(f'{tag}: gradient rel-L2 {err:.2e} > {b:.1e} (floor {floor:.2e})')
    return terms, losses, grad, failures


def _leg(plan, img, steps):
    losses, grad = plan.loss_and_grad(img)
    out = [losses.clone(), grad.clone(), plan.term_losses().clone()]
    if steps:
        state = T._state(img)
        out += [plan.step(*state, k, 0.02).clone() for k in (1, 2, 3)]
        out += list(state)
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in out)
    return out


# ---- 1. the defaults set explicitly -----------------------------------------------------------------------------------------
def test_default_kinds_set_explicitly_are_the_untouched_plan_bit_for_bit():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    _, plain = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=None, configure=False)
    _, named = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=('mse', 'w2'), configure=False)
    assert (named.content_loss, named.style_loss) == ('mse', 'w2')
    a, b = _leg(plain, img, steps=True), _leg(named, img, steps=True)
    assert len(a) == 10 and T._same(a, b)           # losses, gradient, terms, three steps' losses, image, both moments, EMA
    assert not torch.equal(a[6], img)


# ---- 2. / 3. one non-default kind on the default layers ---------------------------------------------------------------------
def _default_layers_case(size, kinds):
    image = T._inputs(size, 'max')['image']
    img = image.to(DEV)
    _, plan = _plan(size, 'max', 'fp16x3', *T.DEFAULT, kinds=kinds)
    tag = f'{size[0]}x{size[1]}-max-fp16x3 default layers, {kinds[0]} + {kinds[1]}'
    terms, losses, _, failures = _judge(tag, plan, img, image, 'max', *T.DEFAULT, kinds, lambda: plan.loss_and_grad(img))
    assert len(terms) == 7
    assert np.array_equal(terms.astype(np.float32), losses[:7])          # the 8-float array keeps its meaning
    assert not failures, '; '.join(failures)


@pytest.mark.parametrize('size', [(40, 48), (72, 88)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_gram_with_mse_on_the_default_layers(size):
    _default_layers_case(size, ('mse', 'gram'))


def test_w2_with_scaled_mse_on_the_default_layers():
    _default_layers_case(SIZE, ('scaled_mse', 'w2'))


# ---- 4. both non-default kinds on other lists -------------------------------------------------------------------------------
BOTH = [('b', 'max', 'fp16x3'),      # layer 29 is in both lists: the scaled-MSE launch adds onto a Gram head's seed
        ('d', 'max', 'fp16x3'),      # pool outputs
        ('f', 'max', 'fp16x3'), ('g', 'max', 'fp16x3'), ('d', 'average', 'fp16x3'), ('d', 'l2', 'fp16x3'), ('b', 'max', 'fp32')]


@pytest.mark.parametrize('name, pooling, precision', BOTH, ids=lambda v: str(v))
def test_both_kinds_on_a_custom_configuration(name, pooling, precision):
    content_layers, style_layers = T.CONFIGS[name]
    image = T._inputs(SIZE, pooling)['image']
    img = image.to(DEV)
    _, plan = _plan(SIZE, pooling, precision, content_layers, style_layers, KINDS)
    tag = f'({name}) content {content_layers} style {style_layers} 40x48-{pooling}-{precision} scaled_mse + gram'
    terms, losses, _, failures = _judge(tag, plan, img, image, pooling, content_layers, style_layers, KINDS,
                                        lambda: plan.loss_and_grad(img))
    nc, ns = len(content_layers), len(style_layers)
    t32 = terms.astype(np.float32)
    assert np.isclose(losses[0], t32[:nc].sum(), rtol=T.SUM_TOL) and np.isclose(losses[1], t32[nc:nc + ns].sum(), rtol=T.SUM_TOL)
    assert not losses[2:6].any() and losses[6] == t32[-1]
    assert not failures, '; '.join(failures)


# ---- 5. exact zeros ---------------------------------------------------------------------------------------------------------
def test_scaled_mse_of_an_image_against_its_own_features_is_exactly_zero():
    """Every d is exactly zero: S2 = 0, S1 = eps, and nothing may become NaN.  The oracle's gradient is the TV gradient alone."""
    from style_transfer import _hip as hip
    content_layers, style_layers = T.CONFIGS['g']
    image = T._inputs(SIZE, 'max')['image']
    img = image.to(DEV)
    net = hip.Net(T._weights(), 'max', DEV, 'fp16x3')
    plan = hip.Plan(net, *SIZE)
    plan.set_taps(content_layers, style_layers)
    plan.set_loss_kinds('scaled_mse', 'w2')
    plan.forward(img, max(content_layers))
    plan.set_content_target_from_forward()
    plan.set_loss_weights(*T._layer_weights(content_layers, style_layers), T.TV_WEIGHT)
    losses, grad = plan.loss_and_grad(img)
    torch.cuda.synchronize()
    terms = plan.term_losses().cpu()
    assert float(terms[0]) == 0.0 and float(losses[0]) == 0.0
    assert torch.isfinite(losses).all() and torch.isfinite(grad).all()
    want = []
    for dtype in (torch.float32, torch.float64):
        x = image.to(dtype).clone().requires_grad_(True)
        (g,) = torch.autograd.grad(O.tv_loss(x) * T.TV_WEIGHT, x)
        want.append(g)
    err, floor = rel_l2(grad.cpu(), want[1]), rel_l2(want[0], want[1])
    print(f'[kinds] exact zeros: gradient hip-vs-fp64 (TV alone) {err:.2e}  floor {floor:.2e}  bar {T.bar(floor):.1e}')
    assert err <= T.bar(floor)
    assert float(losses[7]) == float(terms[1])


# ---- 6. determinism and the steps -------------------------------------------------------------------------------------------
def test_two_closures_on_one_image_are_equal_and_step_is_closure_plus_update():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    _, plan = _plan(SIZE, 'max', 'fp16x3', *T.CONFIGS['b'], KINDS)
    first = [t.clone() for t in plan.loss_and_grad(img)]
    second = [t.clone() for t in plan.loss_and_grad(img)]
    torch.cuda.synchronize()
    assert T._same(first, second) and all(torch.isfinite(t).all() for t in first)
    xa, ma, va, ea = T._state(img)
    xb, mb, vb, eb = T._state(img)
    for k in (1, 2, 3):
        la = plan.step(xa, ma, va, ea, k, 0.02).clone()
        lb, g = plan.loss_and_grad(xb)
        lb = lb.clone()
        plan.apply_update(xb, g, mb, vb, eb, k, 0.02)
        torch.cuda.synchronize()
        assert torch.equal(la, lb), (k, la, lb)
        assert torch.equal(xa, xb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(ea, eb), k
    assert not torch.equal(xa, img)


def test_lbfgs_step_is_closure_plus_update():
    from style_transfer import _hip as hip
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    _, plan = _plan(SIZE, 'max', 'fp16x3', *T.CONFIGS['b'], KINDS)
    xa, _, _, ea = T._state(img)
    xb, _, _, eb = T._state(img)
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


# ---- 7. kinds and lists -----------------------------------------------------------------------------------------------------
def _library_kinds(plan):
    c, s = ctypes.c_int(-1), ctypes.c_int(-1)
    assert plan.lib.st_plan_loss_kinds(plan.handle, ctypes.byref(c), ctypes.byref(s)) == 0
    return c.value, s.value


def test_kinds_and_lists():
    from style_transfer import _hip as hip
    from style_transfer import sharding
    lists = T.CONFIGS['b']
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    net = hip.Net(T._weights(), 'max', DEV, 'fp16x3')
    # a strip plan refuses a non-default kind and takes the defaults
    strip = sharding.StripPlan(net, 48, 48, 0, 32)
    for kinds in (('mse', 'gram'), ('scaled_mse', 'w2')):
        with pytest.raises(hip.HipLibraryError, match='strip'):
            strip.set_loss_kinds(*kinds)
    strip.set_loss_kinds('mse', 'w2')
    assert (strip.content_loss, strip.style_loss) == ('mse', 'w2')
    # names and codes
    plan = hip.Plan(net, *SIZE)
    assert _library_kinds(plan) == (0, 0)
    with pytest.raises(ValueError, match='scaled_mse'):
        plan.set_loss_kinds('l1', 'w2')
    with pytest.raises(ValueError, match='gram'):
        plan.set_loss_kinds('mse', 'gatys')
    for codes in ((2, 0), (0, 2), (-1, 0), (0, -1)):
        assert plan.lib.st_plan_set_loss_kinds(plan.handle, *codes) != 0
        assert 'unknown' in plan.lib.st_last_error().decode() and 'kind' in plan.lib.st_last_error().decode()
    assert _library_kinds(plan) == (0, 0) and (plan.content_loss, plan.style_loss) == ('mse', 'w2')
    # set_loss_kinds drops the targets: the next closure names the first missing one; the kinds survive set_taps
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    plan.loss_and_grad(img)
    plan.set_loss_kinds(*KINDS)
    assert _library_kinds(plan) == (1, 1) and (plan.content_loss, plan.style_loss) == KINDS
    with pytest.raises(hip.HipLibraryError, match=r'content target 0 \(features\[22\]\)'):
        plan.loss_and_grad(img)
    ctargets, moments = T._targets(SIZE, 'max', *T.DEFAULT)
    plan.set_content_target(ctargets[22].to(DEV), 0)
    with pytest.raises(hip.HipLibraryError, match=r'style target 0 \(features\[1\]\)'):
        plan.loss_and_grad(img)
    plan.set_taps(*lists)
    assert _library_kinds(plan) == (1, 1) and (plan.content_loss, plan.style_loss) == KINDS
    # weights set BEFORE set_loss_kinds stay in force: either order of the two calls gives the same closure
    cws, sws = [0.02, 0.005], [0.4, 0.3, 0.15, 0.1, 0.05]
    legs = []
    for kinds_first in (False, True):
        other = hip.Plan(net, *SIZE)
        other.set_taps(*lists)
        if kinds_first:
            other.set_loss_kinds(*KINDS)
            other.set_loss_weights(cws, sws, 3.0)
        else:
            other.set_loss_weights(cws, sws, 3.0)
            other.set_loss_kinds(*KINDS)
        T._set_targets(other, SIZE, 'max', *lists)
        legs.append(_leg(other, img, steps=False))
    assert T._same(*legs)
    T._set_targets(plan, SIZE, 'max', *lists)            # (default weights of the lists: another closure than the legs')
    assert not torch.equal(_leg(plan, img, steps=False)[0], legs[0][0])
    # the range guard runs the closure of the plan's kinds and leaves it as it was on the unflagged synthetic network
    before = _leg(plan, img, steps=False)
    fwd, bwd = plan.range_guard(img)
    assert not any(fwd) and not any(bwd)
    assert T._same(before, _leg(plan, img, steps=False))
    # back to the defaults on the default lists: the fast closure again, equal to a plan that never left it
    plan.set_taps(*T.DEFAULT)
    plan.set_loss_kinds('mse', 'w2')
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    fresh = hip.Plan(net, *SIZE)
    T._set_targets(fresh, SIZE, 'max', *T.DEFAULT)
    assert T._same(_leg(plan, img, steps=True), _leg(fresh, img, steps=True))


# ---- 8. stylize() -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('optimizer', ['adam', 'lbfgs'])
def test_stylize_reads_the_loss_attributes(optimizer):
    from PIL import Image
    from style_transfer import StyleTransfer
    from style_transfer.style_transfer import size_to_fit, to_tensor
    st = StyleTransfer(devices=[DEV], pooling='max', weights='synthetic')
    assert (st.content_loss, st.style_loss) == ('mse', 'w2')
    st.content_loss, st.style_loss = KINDS
    content_image, style_image = T._pil(81, 64, 48), T._pil(82, 60, 44)
    decay = 0.99
    seen = []

    def callback(it):
        if it.i == 1:
            # (the scale's starting image from the EMA and st.image: test_taps_gpu.test_stylize_reads_the_layer_attributes)
            avg, x1 = st.get_image_tensor(), st.image.detach()[0]
            seen.append((it.w, it.h, it.loss, (((1 + decay) * avg - x1) / decay).cpu()[None]))

    out = st.stylize(content_image, [style_image], end_scale=64, min_scale=45, initial_iterations=6, iterations=4,
                     optimizer=optimizer, avg_decay=decay, callback=callback)
    result = st.get_image_tensor()
    assert out is not None and torch.isfinite(result).all() and len(seen) == 2
    cws, sws = [0.015], st.style_weights
    for (w, h, loss, start), scale in zip(seen, (45, 64)):
        assert (w, h) == size_to_fit(content_image.size, scale, scale_up=True)
        content = to_tensor(content_image.resize((w, h), Image.BICUBIC))[None]
        sw_, sh_ = size_to_fit(style_image.size, scale)
        style = to_tensor(style_image.resize((sw_, sh_), Image.BICUBIC))[None]
        with torch.no_grad():
            cfeats = O.vgg_features(content, T._weights(), st.content_layers, 'max')
            sfeats = O.vgg_features(style, T._weights(), st.style_layers, 'max')
        moments = {layer: O.feature_moments(sfeats[layer]) for layer in st.style_layers}
        args = (start, 'max', None, st.content_layers, st.style_layers, cfeats, moments, (cws, sws), KINDS)
        _, total32, _ = _oracle(*args, torch.float32)
        _, total64, _ = _oracle(*args, torch.float64)
        floor = abs(total32 - total64) / abs(total64)
        tol, rel = max(T.TERM_TOL, 3 * floor), abs(loss - total32) / abs(total32)
        print(f'[kinds] stylize {optimizer} {w}x{h}: first loss {loss:.8g} oracle {total32:.8g} rel {rel:.2e} floor {floor:.2e} '
              f'bar {tol:.1e}')
        assert rel <= tol, f'{optimizer} {w}x{h}: first loss rel {rel:.2e} > {tol:.1e}'
    st.style_loss = 'gatys'
    with pytest.raises(ValueError, match=r"'w2', 'gram'"):
        st.stylize(content_image, [style_image], end_scale=64, min_scale=45, initial_iterations=1, iterations=1)

"""A loss kind and an eps per LAYER in the fused closure (st_plan_set_layer_loss_kinds, st_plan_set_loss_eps, list-valued
StyleTransfer.content_loss / style_loss, content_eps / style_eps) on a real MI355X.

Inputs and yardstick are tests/test_taps_gpu.py's and tests/test_loss_kinds_gpu.py's: _smooth images 71 (content), 72 (style),
73 (the iterate), synthetic_vgg19_weights(0), and oracle/st_oracle.py composed by hand in float32 and in float64 on the
branches of the plan's own plain forward.  A layer's kind picks its term and its eps goes where the reference's module puts
it: O.style_target(mean, srm, eps) and O.style_w2(feat, target, eps) for a W2 layer, sum d^2 / (sum |d| + eps) for a Gram or a
scaled-MSE layer.

Bars, the project's own (test_taps_gpu), unchanged:
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
import test_loss_kinds_gpu as K
import test_taps_gpu as T

pytestmark = pytest.mark.gpu
DEV = T.DEV
SIZE = K.SIZE
W2_GRAM = ['w2', 'gram', 'w2', 'gram', 'w2']
GRAM_W2 = ['gram', 'w2', 'gram', 'w2', 'gram']
EPS_DEFAULT = {'w2': 1e-4, 'gram': 1e-8, 'scaled_mse': 1e-8}


def _scaled_mse(x, t, eps):
    d = x - t
    return d.pow(2).sum() / (d.abs().sum() + eps)


def _eps_of(kinds, eps):
    return [EPS_DEFAULT.get(kind) if e is None else e for kind, e in zip(kinds, eps or [None] * len(kinds))]


def _oracle(image, pooling, decisions, content_layers, style_layers, ctargets, moments, weights, kinds, eps, dtype,
            zero_content=False):
    """SumLoss composed in `dtype`, every layer with its own kind and eps: (weighted terms, total, image gradient, features).
    zero_content: the content terms are left out (their value is reported as 0)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cws, sws = weights
    ceps, seps = _eps_of(kinds[0], eps[0]), _eps_of(kinds[1], eps[1])
    img = image.to(dtype).clone().requires_grad_(True)
    terms = []
    feats = O.vgg_features(img, T._weights() if dtype == torch.float32 else T._weights64(), content_layers + style_layers,
                           pooling, decisions)
    for layer, cw, kind, e in zip(content_layers, cws, kinds[0], ceps):
        target = ctargets[layer].to(dtype)
        if zero_content:
            terms.append(torch.zeros((), dtype=dtype))
        else:
            terms.append((O.content_mse(feats[layer], target) if kind == 'mse' else _scaled_mse(feats[layer], target, e)) * cw)
    for layer, sw, kind, e in zip(style_layers, sws, kinds[1], seps):
        mean, srm = moments[layer]
        if kind == 'w2':
            terms.append(O.style_w2(feats[layer], O.style_target(mean.to(dtype), srm.to(dtype), e), e) * sw)
        else:
            terms.append(_scaled_mse(K._gram(feats[layer]), srm.to(dtype), e) * sw)
    terms.append(O.tv_loss(img) * T.TV_WEIGHT)
    total = sum(terms)
    (grad,) = torch.autograd.grad(total, img)
    return [float(t.detach()) for t in terms], float(total.detach()), grad.detach(), {k: v.detach() for k, v in feats.items()}


def _plan(size, pooling, precision, content_layers, style_layers, kinds, eps=None, configure=True, targets=True):
    """A plan on the lists with a kind (and an eps) per layer, in the documented order: layers, kinds, eps, targets."""
    from style_transfer import _hip as hip
    net = hip.Net(T._weights(), pooling, DEV, precision)
    plan = hip.Plan(net, *size)
    if configure:
        plan.set_taps(content_layers, style_layers)
    if kinds is not None:
        plan.set_layer_loss_kinds(*kinds)
    if eps is not None:
        plan.set_loss_eps(*eps)
    if targets:
        T._set_targets(plan, size, pooling, content_layers, style_layers)
    plan.set_loss_weights(*T._layer_weights(content_layers, style_layers), T.TV_WEIGHT)
    return net, plan


def _decisions(plan, img, pooling, content_layers, style_layers):
    deepest = max(content_layers + style_layers)
    plan.forward(img, deepest)
    torch.cuda.synchronize()
    return O.decisions_from_maps({idx: plan.feature(idx).cpu() for idx in T.RELUS if idx <= deepest}, pooling)


def _judge(tag, plan, img, image, pooling, content_layers, style_layers, kinds, eps, closure, zero_content=False):
    """One closure of `plan` against the oracle on the branches of the plan's plain forward to the deepest layer."""
    decisions = _decisions(plan, img, pooling, content_layers, style_layers)
    losses, grad = closure()
    torch.cuda.synchronize()
    terms = plan.term_losses().cpu().double().numpy()
    losses = losses.cpu().numpy()
    weights = T._layer_weights(content_layers, style_layers)
    ctargets, moments = T._targets(tuple(image.shape[2:]), pooling, content_layers, style_layers)
    args = (image, pooling, decisions, content_layers, style_layers, ctargets, moments, weights, kinds, eps)
    t32, _, g32, _ = _oracle(*args, torch.float32, zero_content)
    t64, _, g64, _ = _oracle(*args, torch.float64, zero_content)
    names = ([f'content[{layer}] {kind}' for layer, kind in zip(content_layers, kinds[0])] +
             [f'style[{layer}] {kind}' for layer, kind in zip(style_layers, kinds[1])] + ['tv'])
    failures = []
    assert len(terms) == len(names), (len(terms), names)
    assert np.isfinite(terms).all() and np.isfinite(losses).all(), f'{tag}: non-finite loss'
    for k, name in enumerate(names):
        if zero_content and k < len(content_layers):
            print(f'[layers] {tag} term {name:22s} got {terms[k]:.8g} want exactly 0')
            if terms[k] != 0.0:
                failures.append(f'{tag}: term {name} is {terms[k]:.3g}, not exactly 0')
            continue
        floor = abs(t32[k] - t64[k]) / abs(t64[k])
        tol = max(T.TERM_TOL, 3 * floor)
        rel = abs(terms[k] - t32[k]) / abs(t32[k])
        print(f'[layers] {tag} term {name:22s} got {terms[k]:.8g} want {t32[k]:.8g} rel {rel:.2e}  floor {floor:.2e}  '
              f'bar {tol:.1e}  {"PASS" if rel <= tol else "FAIL"}')
        if not rel <= tol:
            failures.append(f'{tag}: term {name} rel {rel:.2e} > {tol:.1e}')
    want_total = np.float32(0)
    for t in terms.astype(np.float32):
        want_total = np.float32(want_total + t)
    rel_total = abs(float(losses[7]) - float(want_total)) / abs(float(want_total))
    print(f'[layers] {tag} total {losses[7]:.8g} vs fp32 sum of the terms {want_total:.8g} rel {rel_total:.2e} (bar {T.SUM_TOL:.0e})')
    if not rel_total <= T.SUM_TOL:
        failures.append(f'{tag}: total rel {rel_total:.2e} > {T.SUM_TOL:.0e}')
    assert torch.isfinite(grad).all(), f'{tag}: non-finite gradient'
    err, floor = rel_l2(grad.cpu(), g64), rel_l2(g32, g64)
    b = T.bar(floor)
    print(f'[layers] {tag} gradient hip-vs-fp64 {err:.2e}  ref-fp32 floor {floor:.2e}  bar {b:.1e}  {"PASS" if err <= b else "FAIL"}')
    if not err <= b:
        failures.append(f'{tag}: gradient rel-L2 {err:.2e} > {b:.1e} (floor {floor:.2e})')
    return terms, losses, grad, failures


def _configured_array(terms, losses, nc, ns):
    """The 8-float array of a configured plan: content sum, style sum, zeros, tv, total."""
    t32 = terms.astype(np.float32)
    assert np.isclose(losses[0], t32[:nc].sum(), rtol=T.SUM_TOL) and np.isclose(losses[1], t32[nc:nc + ns].sum(), rtol=T.SUM_TOL)
    assert not losses[2:6].any() and losses[6] == t32[-1]


# ---- 1. uniform lists are the scalar setting, bit for bit -------------------------------------------------------------------
def test_uniform_lists_are_the_scalar_setting_bit_for_bit():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    _, scalar = K._plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=K.KINDS, configure=False)
    _, listed = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, (['scaled_mse'], ['gram'] * 5), configure=False)
    assert (listed.content_loss, listed.style_loss) == K.KINDS and listed.style_losses == ('gram',) * 5
    a, b = K._leg(scalar, img, steps=True), K._leg(listed, img, steps=True)
    assert len(a) == 10 and T._same(a, b)           # losses, gradient, terms, three steps' losses, image, both moments, EMA
    assert not torch.equal(a[6], img)


@pytest.mark.parametrize('eps', [(None, None), (None, [1e-4] * 5)], ids=['none', 'the defaults as numbers'])
def test_default_kinds_and_eps_set_explicitly_are_the_untouched_plan_bit_for_bit(eps):
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    _, plain = K._plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=None, configure=False)
    _, named = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, (['mse'], ['w2'] * 5), eps, configure=False)
    assert (named.content_loss, named.style_loss) == ('mse', 'w2')
    assert named.content_eps == (None,) and named.style_eps == (np.float32(1e-4),) * 5
    a, b = K._leg(plain, img, steps=True), K._leg(named, img, steps=True)
    assert len(a) == 10 and T._same(a, b)
    assert not torch.equal(a[6], img)


# ---- 2. mixed kinds on the default layers -----------------------------------------------------------------------------------
MIXED_DEFAULT = [((40, 48), 'mse', W2_GRAM), ((72, 88), 'mse', W2_GRAM), ((40, 48), 'scaled_mse', GRAM_W2)]


@pytest.mark.parametrize('size, content, style', MIXED_DEFAULT, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else
                         v if isinstance(v, str) else ','.join(v))
def test_mixed_kinds_on_the_default_layers(size, content, style):
    """The deepest head's gradient is what the backward starts from: relu5_1 is tried as a W2 and as a Gram head."""
    kinds = ([content], style)
    image = T._inputs(size, 'max')['image']
    img = image.to(DEV)
    _, plan = _plan(size, 'max', 'fp16x3', *T.DEFAULT, kinds)
    assert plan.style_loss == tuple(style) and plan.content_loss == content
    tag = f'{size[0]}x{size[1]}-max-fp16x3 default layers, {content} + {",".join(style)}'
    terms, losses, _, failures = _judge(tag, plan, img, image, 'max', *T.DEFAULT, kinds, (None, None),
                                        lambda: plan.loss_and_grad(img))
    assert len(terms) == 7
    assert np.array_equal(terms.astype(np.float32), losses[:7])          # the 8-float array keeps its meaning
    assert not failures, '; '.join(failures)


# ---- 3. mixed kinds on other lists ------------------------------------------------------------------------------------------
OTHER = [
    # content [22, 29], style [1, 6, 11, 20, 29]: a scaled-MSE seed is added onto a Gram head's seed ... and onto a W2 head's
    ('b', 'max', 'fp16x3', ['mse', 'scaled_mse'], ['w2', 'w2', 'w2', 'w2', 'gram']),
    ('b', 'max', 'fp16x3', ['mse', 'scaled_mse'], ['w2'] * 5),
    # content [18], style [1, 13, 27]: pool outputs
    ('d', 'max', 'fp16x3', ['mse'], ['gram', 'w2', 'gram']),
    ('d', 'average', 'fp16x3', ['mse'], ['gram', 'w2', 'gram']),
    ('d', 'l2', 'fp16x3', ['mse'], ['gram', 'w2', 'gram']),
    # content [22], style [3, 8, 17, 26]: each of these feeds a pool
    ('e', 'max', 'fp16x3', ['mse'], ['w2', 'gram', 'w2', 'gram']),
    ('b', 'max', 'fp32', ['mse', 'scaled_mse'], ['w2', 'w2', 'w2', 'w2', 'gram']),
]


@pytest.mark.parametrize('name, pooling, precision, content, style', OTHER,
                         ids=lambda v: ','.join(v) if isinstance(v, list) else str(v))
def test_mixed_kinds_on_a_custom_configuration(name, pooling, precision, content, style):
    content_layers, style_layers = T.CONFIGS[name]
    kinds = (content, style)
    image = T._inputs(SIZE, pooling)['image']
    img = image.to(DEV)
    _, plan = _plan(SIZE, pooling, precision, content_layers, style_layers, kinds)
    tag = f'({name}) content {content_layers} {",".join(content)} style {style_layers} {",".join(style)} 40x48-{pooling}-{precision}'
    terms, losses, _, failures = _judge(tag, plan, img, image, pooling, content_layers, style_layers, kinds, (None, None),
                                        lambda: plan.loss_and_grad(img))
    _configured_array(terms, losses, len(content_layers), len(style_layers))
    assert not failures, '; '.join(failures)


# ---- 4. eps is honoured, visibly --------------------------------------------------------------------------------------------
def test_eps_is_honoured_visibly():
    """W2 eps 1e-2 on relu1_1 and relu5_1, relu3_1 a Gram head and the content term a scaled MSE, both with eps = a quarter of
    their sum |d|.  Each of these four terms of the fp32 oracle is first shown to differ from the same term at the default eps
    by at least 50 bars, so a build that ignores any of the four eps cannot pass."""
    from style_transfer import _hip as hip
    content_layers, style_layers = T.DEFAULT
    kinds = (['scaled_mse'], ['w2', 'w2', 'gram', 'w2', 'w2'])
    image = T._inputs(SIZE, 'max')['image']
    img = image.to(DEV)
    _, plan = _plan(SIZE, 'max', 'fp16x3', content_layers, style_layers, kinds, targets=False)
    decisions = _decisions(plan, img, 'max', content_layers, style_layers)
    weights = T._layer_weights(content_layers, style_layers)
    ctargets, moments = T._targets(SIZE, 'max', content_layers, style_layers)
    args = (image, 'max', decisions, content_layers, style_layers, ctargets, moments, weights, kinds)
    base32, _, _, feats = _oracle(*args, (None, None), torch.float32)
    # both sums from the fp32 oracle, as host floats
    content_eps = 0.25 * float((feats[22] - ctargets[22]).abs().sum())
    gram_eps = 0.25 * float((K._gram(feats[11]) - moments[11][1]).abs().sum())
    eps = ([content_eps], [1e-2, None, gram_eps, None, 1e-2])
    t32 = _oracle(*args, eps, torch.float32)[0]
    t64 = _oracle(*args, eps, torch.float64)[0]
    for k, name in ((0, 'content[22] scaled_mse'), (1, 'style[1] w2'), (3, 'style[11] gram'), (5, 'style[29] w2')):
        tol = max(T.TERM_TOL, 3 * abs(t32[k] - t64[k]) / abs(t64[k]))
        moved = abs(t32[k] - base32[k]) / abs(t32[k])
        print(f'[layers] eps moves term {name:22s} by {moved:.2e} = {moved / tol:.0f} bars of {tol:.1e}')
        assert moved >= 50 * tol, (name, moved, tol)
    for k in (2, 4, 6):
        assert t32[k] == base32[k]
    plan.set_loss_eps(*eps)
    assert plan.content_eps == (np.float32(content_eps),)
    assert plan.style_eps == tuple(np.float32(v) for v in (1e-2, 1e-4, gram_eps, 1e-4, 1e-2))
    with pytest.raises(hip.HipLibraryError, match=r'content target 0 \(features\[22\]\)'):
        plan.loss_and_grad(img)
    T._set_targets(plan, SIZE, 'max', content_layers, style_layers)          # the targets come after the eps
    tag = '40x48-max-fp16x3 default layers, custom eps'
    terms, losses, _, failures = _judge(tag, plan, img, image, 'max', content_layers, style_layers, kinds, eps,
                                        lambda: plan.loss_and_grad(img))
    assert np.array_equal(terms.astype(np.float32), losses[:7])
    assert not failures, '; '.join(failures)


def test_a_w2_eps_alone_leaves_the_fast_closure():
    """Every kind at its default and ONE eps not: the general closure, judged like the rest."""
    kinds, eps = (['mse'], ['w2'] * 5), (None, [None, None, None, None, 1e-2])
    image = T._inputs(SIZE, 'max')['image']
    img = image.to(DEV)
    _, plan = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds, eps, configure=False)
    terms, losses, _, failures = _judge('40x48-max-fp16x3 default layers, relu5_1 eps 1e-2', plan, img, image, 'max', *T.DEFAULT,
                                        kinds, eps, lambda: plan.loss_and_grad(img))
    assert np.array_equal(terms.astype(np.float32), losses[:7])
    assert not failures, '; '.join(failures)


# ---- 5. zero difference with a custom eps -----------------------------------------------------------------------------------
def test_zero_difference_with_a_custom_eps():
    """Every d is exactly zero: S2 = 0, S1 = eps = 1e-3, the term is exactly 0 and nothing is NaN; the gradient is the other
    terms' alone."""
    kinds, eps = (['scaled_mse'], W2_GRAM), ([1e-3], None)
    image = T._inputs(SIZE, 'max')['image']
    img = image.to(DEV)
    _, plan = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds, eps)
    plan.forward(img, 29)
    plan.set_content_target_from_forward()
    terms, losses, grad, failures = _judge('40x48 zero difference, eps 1e-3', plan, img, image, 'max', *T.DEFAULT, kinds, eps,
                                           lambda: plan.loss_and_grad(img), zero_content=True)
    assert float(terms[0]) == 0.0 and float(losses[0]) == 0.0
    assert not failures, '; '.join(failures)


# ---- 6. determinism and the steps -------------------------------------------------------------------------------------------
def _mixed_plan():
    return _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, (['mse'], W2_GRAM))[1]


def test_two_closures_on_one_image_are_equal_and_step_is_closure_plus_update():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    plan = _mixed_plan()
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
    # the range guard runs the mixed closure and leaves the plan as it was on the unflagged synthetic network
    before = K._leg(plan, img, steps=False)
    fwd, bwd = plan.range_guard(img)
    assert not any(fwd) and not any(bwd)
    assert T._same(before, K._leg(plan, img, steps=False))


def test_lbfgs_step_is_closure_plus_update():
    from style_transfer import _hip as hip
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    plan = _mixed_plan()
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


# ---- 7. setter semantics ----------------------------------------------------------------------------------------------------
def _ints(*values):
    return (ctypes.c_int * max(len(values), 1))(*values)


def _floats(*values):
    return (ctypes.c_float * max(len(values), 1))(*values)


def test_setter_semantics():
    from style_transfer import _hip as hip
    from style_transfer import sharding
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    net = hip.Net(T._weights(), 'max', DEV, 'fp16x3')
    plan = hip.Plan(net, *SIZE)
    lib = plan.lib
    assert plan.content_losses == ('mse',) and plan.style_losses == ('w2',) * 5
    assert plan.content_eps == (None,) and plan.style_eps == (np.float32(1e-4),) * 5
    # the getters return what was set; a mixed list reports -1 and its tuple
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    plan.loss_and_grad(img)
    plan.set_layer_loss_kinds(['scaled_mse'], W2_GRAM)
    assert K._library_kinds(plan) == (1, -1)
    assert plan.content_loss == 'scaled_mse' and plan.style_loss == tuple(W2_GRAM) == plan.style_losses
    assert plan.style_eps == tuple(np.float32(1e-4 if kind == 'w2' else 1e-8) for kind in W2_GRAM)
    assert plan.content_eps == (np.float32(1e-8),)
    # ... and has dropped the targets, as set_loss_eps does
    with pytest.raises(hip.HipLibraryError, match=r'content target 0 \(features\[22\]\)'):
        plan.loss_and_grad(img)
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    mixed = K._leg(plan, img, steps=False)
    plan.set_loss_eps(0.5, [1e-2, None, 1e-3, 1e-6, None])
    assert plan.content_eps == (0.5,)
    assert plan.style_eps == tuple(np.float32(v) for v in (1e-2, 1e-8, 1e-3, 1e-6, 1e-4))
    with pytest.raises(hip.HipLibraryError, match=r'content target 0 \(features\[22\]\)'):
        plan.loss_and_grad(img)
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    assert not torch.equal(K._leg(plan, img, steps=False)[0], mixed[0])
    # errors carry a message and leave the plan as it was
    kinds, eps = (plan.content_losses, plan.style_losses), (plan.content_eps, plan.style_eps)
    before = K._leg(plan, img, steps=False)
    for codes in (([2], [0] * 5), ([0], [0, 0, -1, 0, 0]), ([0], [0, 0, 0, 0, 2])):
        assert lib.st_plan_set_layer_loss_kinds(plan.handle, _ints(*codes[0]), _ints(*codes[1])) != 0
        assert 'unknown' in lib.st_last_error().decode() and 'kind' in lib.st_last_error().decode()
    assert lib.st_plan_set_loss_eps(plan.handle, _floats(float('nan')), None) != 0
    assert 'not finite' in lib.st_last_error().decode()
    assert lib.st_plan_set_loss_eps(plan.handle, None, _floats(0, 0, float('nan'), 0, 0)) != 0
    assert 'not finite' in lib.st_last_error().decode()
    with pytest.raises(ValueError, match='gram'):
        plan.set_layer_loss_kinds(['mse'], ['w2', 'w2', 'w2', 'w2', 'gatys'])
    with pytest.raises(ValueError, match='one per layer'):
        plan.set_layer_loss_kinds(['mse'], ['w2'] * 4)
    with pytest.raises(ValueError, match='one per layer'):
        plan.set_loss_eps(None, [1e-3] * 4)
    with pytest.raises(ValueError, match='non-negative'):
        plan.set_loss_eps(None, [-1e-3] * 5)
    assert (plan.content_losses, plan.style_losses) == kinds and (plan.content_eps, plan.style_eps) == eps
    assert T._same(before, K._leg(plan, img, steps=False))
    # an eps on an mse content entry
    plan.set_layer_loss_kinds(['mse'], W2_GRAM)
    assert plan.style_eps == tuple(np.float32(1e-4 if kind == 'w2' else 1e-8) for kind in W2_GRAM)     # (the kinds reset every eps)
    with pytest.raises(hip.HipLibraryError, match='mse'):
        plan.set_loss_eps([1e-3], None)
    assert plan.content_eps == (None,)
    plan.set_loss_eps([None], 1e-3)
    assert plan.style_eps == (np.float32(1e-3),) * 5
    # set_loss_kinds after set_loss_eps leaves every eps at the default
    plan.set_loss_kinds('scaled_mse', 'gram')
    assert plan.content_eps == (np.float32(1e-8),) and plan.style_eps == (np.float32(1e-8),) * 5
    # set_taps keeps a uniform list's kind and returns a mixed one to kind 0, and every eps to the default
    plan.set_layer_loss_kinds(['scaled_mse'], GRAM_W2)
    plan.set_loss_eps(1e-3, 1e-3)
    plan.set_taps(*T.CONFIGS['b'])
    assert K._library_kinds(plan) == (1, 0)
    assert plan.content_loss == 'scaled_mse' and plan.content_losses == ('scaled_mse',) * 2
    assert plan.style_loss == 'w2' and plan.style_losses == ('w2',) * 5
    assert plan.content_eps == (np.float32(1e-8),) * 2 and plan.style_eps == (np.float32(1e-4),) * 5
    # back to the defaults on the default lists: the fast closure again, equal to a plan that never left it
    plan.set_taps(*T.DEFAULT)
    plan.set_layer_loss_kinds(['mse'], ['w2'] * 5)
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    fresh = hip.Plan(net, *SIZE)
    T._set_targets(fresh, SIZE, 'max', *T.DEFAULT)
    assert T._same(K._leg(plan, img, steps=True), K._leg(fresh, img, steps=True))
    # a strip plan takes the defaults and refuses everything else
    strip = sharding.StripPlan(net, 48, 48, 0, 32)
    with pytest.raises(hip.HipLibraryError, match='strip'):
        strip.set_layer_loss_kinds(['mse'], W2_GRAM)
    with pytest.raises(hip.HipLibraryError, match='strip'):
        strip.set_layer_loss_kinds(['scaled_mse'], ['w2'] * 5)
    with pytest.raises(hip.HipLibraryError, match='strip'):
        strip.set_loss_eps(None, [None, None, None, None, 1e-2])
    strip.set_layer_loss_kinds(['mse'], ['w2'] * 5)
    strip.set_loss_eps(None, [1e-4] * 5)
    assert (strip.content_loss, strip.style_loss) == ('mse', 'w2') and strip.style_eps == (np.float32(1e-4),) * 5


# ---- 8. memory --------------------------------------------------------------------------------------------------------------
def test_a_head_allocates_what_its_own_kind_needs():
    from style_transfer import _hip as hip
    net = hip.Net(T._weights(), 'max', DEV, 'fp16x3')
    used = {}
    for name, style in (('w2', ['w2'] * 5), ('mixed', ['w2', 'w2', 'w2', 'gram', 'gram']), ('gram', ['gram'] * 5)):
        plan = hip.Plan(net, *SIZE)
        plan.set_layer_loss_kinds(['mse'], style)
        T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
        torch.cuda.synchronize()
        used[name] = plan.device_bytes()
    print(f'[layers] st_plan_device_bytes at 40x48: five W2 heads {used["w2"]}, w2,w2,w2,gram,gram {used["mixed"]}, '
          f'five Gram heads {used["gram"]}')
    assert used['gram'] <= used['mixed'] < used['w2']


# ---- 9. stylize() -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('optimizer', ['adam', 'lbfgs'])
def test_stylize_reads_the_per_layer_attributes(optimizer):
    from PIL import Image
    from style_transfer import StyleTransfer
    from style_transfer.style_transfer import size_to_fit, to_tensor
    st = StyleTransfer(devices=[DEV], pooling='max', weights='synthetic')
    assert (st.content_eps, st.style_eps) == (None, None)
    content_image, style_image = T._pil(81, 64, 48), T._pil(82, 60, 44)
    decay, scale = 0.99, 64
    seen = []

    def callback(it):
        if it.i == 1:
            # (the scale's starting image from the EMA and st.image: test_taps_gpu.test_stylize_reads_the_layer_attributes)
            avg, x1 = st.get_image_tensor(), st.image.detach()[0]
            seen.append((it.w, it.h, it.loss, (((1 + decay) * avg - x1) / decay).cpu()[None]))

    def run():
        del seen[:]
        out = st.stylize(content_image, [style_image], end_scale=scale, min_scale=scale, initial_iterations=4, iterations=4,
                         optimizer=optimizer, avg_decay=decay, callback=callback)
        assert out is not None and torch.isfinite(st.get_image_tensor()).all() and len(seen) == 1
        return seen[0]

    default_loss = run()[2]
    kinds = (['scaled_mse'], ['w2', 'w2', 'w2', 'gram', 'gram'])
    eps = (None, [1e-2, None, None, None, 1e-3])
    st.content_loss, st.style_loss, st.style_eps = kinds[0], kinds[1], eps[1]
    w, h, loss, start = run()
    assert (w, h) == size_to_fit(content_image.size, scale, scale_up=True)
    content = to_tensor(content_image.resize((w, h), Image.BICUBIC))[None]
    sw_, sh_ = size_to_fit(style_image.size, scale)
    style = to_tensor(style_image.resize((sw_, sh_), Image.BICUBIC))[None]
    with torch.no_grad():
        cfeats = O.vgg_features(content, T._weights(), st.content_layers, 'max')
        sfeats = O.vgg_features(style, T._weights(), st.style_layers, 'max')
    moments = {layer: O.feature_moments(sfeats[layer]) for layer in st.style_layers}
    args = (start, 'max', None, st.content_layers, st.style_layers, cfeats, moments, ([0.015], st.style_weights), kinds, eps)
    total32, total64 = _oracle(*args, torch.float32)[1], _oracle(*args, torch.float64)[1]
    floor = abs(total32 - total64) / abs(total64)
    tol, rel = max(T.TERM_TOL, 3 * floor), abs(loss - total32) / abs(total32)
    print(f'[layers] stylize {optimizer} {w}x{h}: first loss {loss:.8g} oracle {total32:.8g} rel {rel:.2e} floor {floor:.2e} '
          f'bar {tol:.1e}; the default run: {default_loss:.8g}')
    assert rel <= tol, f'{optimizer} {w}x{h}: first loss rel {rel:.2e} > {tol:.1e}'
    assert abs(loss - default_loss) / abs(default_loss) > 50 * tol
    # the same object with the attributes back at their defaults: the default run again
    del st.content_loss, st.style_loss, st.style_eps
    assert run()[2] == default_loss
    st.style_loss = ['w2', 'w2', 'gram']
    with pytest.raises(ValueError, match='style_loss'):
        st.stylize(content_image, [style_image], end_scale=64, min_scale=64, initial_iterations=1, iterations=1)

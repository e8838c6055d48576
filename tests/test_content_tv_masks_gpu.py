"""Spatial weight maps for the content and TV terms (st_plan_set_content_mask / st_plan_set_tv_mask, _hip.Plan.set_content_mask /
set_tv_mask, StyleTransfer.content_mask / tv_mask) on a real MI355X.

The reference has neither; the yardstick is the math of include/st_amd.h in float64, written out below on st_oracle's parts.
With w the content map at a tap's level (level k + 1 = avg_pool2d(level k, 2); a tap's level = the pools at or before it),
d = F - T on a [C][h][w] tap and cw the entry's weight:
    mse:         cw sum w d^2 / (C h w)                    scaled_mse:  cw sum w d^2 / (sum w |d| + eps)
and with P, Wp the replicate-padded image and TV map and s1 .. s4 TVLoss' slices (style_transfer.py:184-195):
    q(a, b) = mean(((Wp[a] + Wp[b]) / 2) (P[a] - P[b])^2)
    tv = 2 (q((s1,s2),(s1,s1)) / 3 + q((s2,s1),(s1,s1)) / 3 + q((s4,s4),(s3,s3)) / 12 + q((s4,s3),(s3,s4)) / 12)
The gradient is autograd's on those formulas.  Inputs, targets, weights and bars are test_taps_gpu's / test_loss_kinds_gpu's,
the maps test_style_mask_gpu's, all imported:
  each weighted term  |hip - fp32 oracle| / |fp32 oracle| <= max(1e-4, 3 x the fp32 oracle's deviation from float64);
  the total           within 1e-6 of the fp32 sum of the terms;
  image gradient      rel-L2 against float64 <= min(5e-3, max(1e-4, 1.5 x the fp32 oracle's own rel-L2 from float64));
  the TV kernels alone: test_kernels_gpu.test_tv_loss_and_gradient's 2e-6 on value and gradient against the fp32 formula too.
A map that is ignored cannot pass: on the ramp every weighted float64 term differs from its unweighted value by >= 100 bars.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
import st_oracle as O
import test_loss_kinds_gpu as K
import test_style_mask_gpu as MG
import test_taps_gpu as T
from test_style_mask_gpu import binary_mask, ramp_mask

pytestmark = pytest.mark.gpu
DEV = T.DEV
SIZE = MG.SIZE       # 40 x 48
ODD = MG.ODD         # 45 x 54: tap pixel counts 2430, 594, 143, 30, 6 - the scalar paths of the weighted content kernels
# A custom eps for 'scaled_mse' (its default is 1e-8), of the order of S1 = sum |d| itself (6.5e3 at relu4_2 at 40 x 48, 3e4 - 6e4
# at the shallower taps).  Under a negligible eps the term S2 / S1 is a ratio of two sums that a map scales alike: the ramp then
# moves the float64 term at relu4_2 by 0.5 % only - 51 bars -, and an ignored map could hide there.  With eps ~ S1 the map
# moves it by a third, and the test also sees that eps is added behind the weighted sum.
CONTENT_EPS = 4096.0


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
def weighted_tv(image, wmap):
    """include/st_amd.h's TV term under a map, before tv_weight.  image [1, 3, H, W], wmap [H, W], one dtype."""
    p = F.pad(image, (1, 1, 1, 1), mode='replicate')
    wp = F.pad(wmap[None, None], (1, 1, 1, 1), mode='replicate')
    s1, s2, s3, s4 = slice(1, -1), slice(2, None), slice(None, -1), slice(1, None)

    def q(a, b):
        return (((wp[..., a[0], a[1]] + wp[..., b[0], b[1]]) / 2) * (p[..., a[0], a[1]] - p[..., b[0], b[1]]) ** 2).mean()
    return 2 * (q((s1, s2), (s1, s1)) / 3 + q((s2, s1), (s1, s1)) / 3 + q((s4, s4), (s3, s3)) / 12 + q((s4, s3), (s3, s4)) / 12)


def weighted_content(feat, target, wmap, kind, eps):
    """include/st_amd.h's content term under a level of the map, before the entry's weight (wmap None: the unweighted term)."""
    d = feat - target
    w = torch.ones(feat.shape[2:], dtype=feat.dtype) if wmap is None else wmap
    if kind == 'mse':
        return (w * d ** 2).sum() / d.numel()
    return (w * d ** 2).sum() / ((w * d.abs()).sum() + eps)


def _oracle(image, pooling, decisions, content_layers, style_layers, ctargets, moments, weights, kinds, ceps, clevels, tvmap,
            slevels, dtype):
    """SumLoss with the weighted terms in `dtype`: (weighted terms, total, gradient, the UNWEIGHTED content and tv terms).
    clevels / tvmap / slevels: the content map's levels, the TV map, the style mask's (m, M) levels - None: that term plain."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cws, sws = weights
    img = image.to(dtype).clone().requires_grad_(True)
    taps = content_layers + style_layers
    feats = O.vgg_features(img, T._weights() if dtype == torch.float32 else T._weights64(), taps, pooling, decisions) if taps else {}

    def content(layer, cw, levels):
        wmap = None if levels is None else levels[MG.LEVEL[layer]].to(dtype)
        return weighted_content(feats[layer], ctargets[layer].to(dtype), wmap, kinds[0], ceps) * cw

    def tv(wmap):
        return (O.tv_loss(img) if wmap is None else weighted_tv(img, wmap.to(dtype))) * T.TV_WEIGHT
    terms = [content(layer, cw, clevels) for layer, cw in zip(content_layers, cws)]
    terms += [MG._style_term(feats[layer], layer, moments, slevels, kinds[1], dtype) * sw for layer, sw in zip(style_layers, sws)]
    terms.append(tv(tvmap))
    total = sum(terms)
    (grad,) = torch.autograd.grad(total, img)
    with torch.no_grad():
        plain = [float(content(layer, cw, None)) for layer, cw in zip(content_layers, cws)] + [float(tv(None))]
    return [float(t.detach()) for t in terms], float(total.detach()), grad.detach(), plain


def _content_levels(plan):
    """The plan's own levels of the content map, in float64: what its kernels weigh with."""
    return [plan.content_mask_level(k).cpu().double() for k in range(5)]


def _judge(tag, plan, img, image, pooling, content_layers, style_layers, kinds, ceps, moved_terms=()):
    """One closure of `plan` against the oracle under the plan's OWN maps.  moved_terms: names of the terms that the map must
    move by >= 100 bars.  Returns (terms, losses, gradient, failures)."""
    deepest = max(content_layers + style_layers)
    plan.forward(img, deepest)
    torch.cuda.synchronize()
    decisions = O.decisions_from_maps({idx: plan.feature(idx).cpu() for idx in T.RELUS if idx <= deepest}, pooling)
    from style_transfer import _hip as hip

    def held(read):
        try:
            return read()
        except hip.HipLibraryError:
            return None
    clevels = held(lambda: _content_levels(plan))
    tvmap = held(lambda: plan.tv_mask().cpu().double())
    slevels = held(lambda: MG._plan_levels(plan))
    losses, grad = plan.loss_and_grad(img)
    torch.cuda.synchronize()
    terms = plan.term_losses().cpu().double().numpy()
    losses = losses.cpu().numpy()
    weights = T._layer_weights(content_layers, style_layers)
    ctargets, moments = T._targets(tuple(image.shape[2:]), pooling, content_layers, style_layers)
    args = (image, pooling, decisions, content_layers, style_layers, ctargets, moments, weights, kinds, ceps, clevels, tvmap, slevels)
    t32, _, g32, _ = _oracle(*args, torch.float32)
    t64, _, g64, plain64 = _oracle(*args, torch.float64)
    names = [f'content[{layer}]' for layer in content_layers] + [f'style[{layer}]' for layer in style_layers] + ['tv']
    plain_of = dict(zip(names[:len(content_layers)] + ['tv'], plain64))
    failures = []
    assert len(terms) == len(names), (len(terms), names)
    for k, name in enumerate(names):
        floor = abs(t32[k] - t64[k]) / abs(t64[k])
        tol = max(T.TERM_TOL, 3 * floor)
        rel = abs(terms[k] - t32[k]) / abs(t32[k])
        print(f'[maps] {tag} term {name:12s} got {terms[k]:.8g} want {t32[k]:.8g} rel {rel:.2e}  floor {floor:.2e}  '
              f'bar {tol:.1e}  {"PASS" if rel <= tol else "FAIL"}')
        if not rel <= tol:
            failures.append(f'{tag}: term {name} rel {rel:.2e} > {tol:.1e}')
        if name in moved_terms:
            moved = abs(t64[k] - plain_of[name]) / abs(plain_of[name])
            print(f'[maps] {tag} term {name:12s} weighted float64 {t64[k]:.8g} unweighted {plain_of[name]:.8g}: moved by {moved:.3g} = '
                  f'{moved / tol:.0f} bars')
            assert moved >= 100 * tol, f'{tag}: the map moves term {name} by {moved / tol:.1f} bars only: it could be ignored'
    want_total = np.float32(0)
    for t in terms.astype(np.float32):
        want_total = np.float32(want_total + t)
    rel_total = abs(float(losses[7]) - float(want_total)) / abs(float(want_total))
    print(f'[maps] {tag} total {losses[7]:.8g} vs fp32 sum of the terms {want_total:.8g} rel {rel_total:.2e} (bar {T.SUM_TOL:.0e})')
    if not rel_total <= T.SUM_TOL:
        failures.append(f'{tag}: total rel {rel_total:.2e} > {T.SUM_TOL:.0e}')
    assert torch.isfinite(grad).all(), f'{tag}: non-finite gradient'
    err, floor = rel_l2(grad.cpu(), g64), rel_l2(g32, g64)
    b = T.bar(floor)
    print(f'[maps] {tag} gradient hip-vs-fp64 {err:.2e}  ref-fp32 floor {floor:.2e}  bar {b:.1e}  {"PASS" if err <= b else "FAIL"}')
    if not err <= b:
        failures.append(f'{tag}: gradient rel-L2 {err:.2e} > {b:.1e} (floor {floor:.2e})')
    return terms, losses, grad, failures


# ---- 1. the pyramid ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [SIZE, ODD], ids=lambda s: f'{s[0]}x{s[1]}')
def test_pyramid(size):
    """content_mask_level(k) against the avg_pool2d chain of the fp32 map: max abs error <= 2e-6 (the style mask's pyramid bar:
    values <= 1, at most four levels of three roundings each).  tv_mask() is the input bit for bit.  Two calls give equal bits."""
    _, plan = MG._net_plan(size)
    mask = ramp_mask(*size)
    want = MG.pyramid(mask)
    plan.set_content_mask(mask.to(DEV))
    plan.set_tv_mask(mask.to(DEV))
    first = [plan.content_mask_level(k) for k in range(5)]
    first_tv = plan.tv_mask()
    plan.set_content_mask(mask.to(DEV))
    plan.set_tv_mask(mask.to(DEV))
    second = [plan.content_mask_level(k) for k in range(5)]
    torch.cuda.synchronize()
    for k in range(5):
        assert tuple(first[k].shape) == tuple(want[k].shape) == (size[0] >> k, size[1] >> k)
        err = float((first[k].cpu() - want[k]).abs().max())
        print(f'[maps] pyramid {size} level {k} {tuple(first[k].shape)}: max abs {err:.2e} (bar 2e-6)')
        assert err <= 2e-6
        assert torch.equal(first[k], second[k])
    assert torch.equal(first[0].cpu(), mask), 'level 0 is the map itself'
    assert tuple(first_tv.shape) == size and torch.equal(first_tv.cpu(), mask) and torch.equal(plan.tv_mask(), first_tv)


# ---- 2. the weighted TV kernels alone ---------------------------------------------------------------------------------------
def _tv_only_plan(size):
    """A plan whose only other term is relu1_1's content MSE at weight 0: its gradient is the TV kernels' plus an exact zero."""
    from style_transfer import _hip as hip
    net = hip.Net(T._weights(), 'max', DEV, 'fp32')
    plan = hip.Plan(net, *size)
    plan.set_taps([1], [])
    img = T._smooth(73, *size)
    plan.forward(img.to(DEV), 1)
    plan.set_content_target_from_forward()
    plan.set_loss_weights([0.0], [], T.TV_WEIGHT)
    return plan, img


def _tv_oracle(image, wmap, dtype):
    img = image.to(dtype).clone().requires_grad_(True)
    term = (O.tv_loss(img) if wmap is None else weighted_tv(img, wmap.to(dtype))) * T.TV_WEIGHT
    (grad,) = torch.autograd.grad(term, img)
    return float(term.detach()), grad.detach()


@pytest.mark.parametrize('size', [(40, 48), (45, 54), (16, 16), (32, 1040)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_weighted_tv_alone(size):
    """40 x 48: interior and border kernels; 45 x 54: W % 4 != 0, the border kernel only; 16 x 16: almost all border;
    32 x 1040: a row of more than 256 groups of four."""
    plan, image = _tv_only_plan(size)
    img = image.to(DEV)

    def run():
        losses, grad = plan.loss_and_grad(img)
        torch.cuda.synchronize()
        terms = plan.term_losses().cpu().double().numpy()
        assert len(terms) == 2 and terms[0] == 0
        return float(terms[1]), grad.cpu()
    plain_term, plain_grad = run()
    want_plain, _ = _tv_oracle(image, None, torch.float64)
    for name, make in MG.MASKS.items():
        wmap = make(*size)
        plan.set_tv_mask(wmap.to(DEV))
        assert torch.equal(plan.tv_mask().cpu(), wmap)
        term, grad = run()
        t32, g32 = _tv_oracle(image, wmap, torch.float32)
        t64, g64 = _tv_oracle(image, wmap, torch.float64)
        floor = abs(t32 - t64) / abs(t64)
        tol = max(T.TERM_TOL, 3 * floor)
        rel, rel32 = abs(term - t64) / abs(t64), abs(term - t32) / abs(t32)
        err, gfloor, err32 = rel_l2(grad, g64), rel_l2(g32, g64), rel_l2(grad, g32)
        b = T.bar(gfloor)
        tag = f'tv alone {size[0]}x{size[1]} {name}'
        print(f'[maps] {tag}: term {term:.8g} float64 {t64:.8g} rel {rel:.2e} (bar {tol:.1e}); against the fp32 formula {rel32:.2e} '
              f'(bar 2e-6)')
        print(f'[maps] {tag}: gradient hip-vs-fp64 {err:.2e} floor {gfloor:.2e} (bar {b:.1e}); against the fp32 formula {err32:.2e} '
              f'(bar 2e-6)')
        assert rel <= tol and rel32 <= 2e-6
        assert torch.isfinite(grad).all() and err <= b and err32 <= 2e-6
        moved = abs(t64 - want_plain) / abs(want_plain)
        print(f'[maps] {tag}: weighted float64 {t64:.8g} unweighted {want_plain:.8g}: moved by {moved:.3g} = {moved / tol:.0f} bars')
        if name == 'ramp':
            assert moved >= 100 * tol, f'{tag}: the map moves the term by {moved / tol:.1f} bars only: it could be ignored'
        assert not torch.equal(grad, plain_grad)
    plan.set_tv_mask(torch.ones(size).to(DEV))
    ones_term, ones_grad = run()
    rel = abs(ones_term - plain_term) / abs(plain_term)
    print(f'[maps] tv alone {size[0]}x{size[1]} all-ones: term {ones_term:.8g} unmasked {plain_term:.8g} rel {rel:.2e}; gradient '
          f'rel-L2 {rel_l2(ones_grad, plain_grad):.2e}')
    assert rel <= T.TERM_TOL and rel_l2(ones_grad, plain_grad) <= 2e-6
    plan.set_tv_mask(None)
    again_term, again_grad = run()
    assert again_term == plain_term and torch.equal(again_grad, plain_grad), 'a cleared map must leave the plain kernels, bit for bit'


# ---- 3. the weighted content terms ------------------------------------------------------------------------------------------
CONTENT_LISTS = {
    'c22': ([22], [1, 6, 11, 20, 29]),       # the default lists
    'c4-13': ([4, 13], [1, 6]),              # two levels of the map (1 and 2); a pool output as a content tap
    'c6-acc': ([6], [6]),                    # 6 is a style layer too: the content launch ADDS onto the head's seed
}
CONTENT_CASES = [(kind, name, size, precision) for kind in ('mse', 'scaled_mse') for name in CONTENT_LISTS for size in (SIZE, ODD)
                 for precision in ('fp16x3', 'fp32')]


@pytest.mark.parametrize('kind, name, size, precision', CONTENT_CASES,
                         ids=[f'{c[0]}-{c[1]}-{c[2][0]}x{c[2][1]}-{c[3]}' for c in CONTENT_CASES])
def test_weighted_content_terms(kind, name, size, precision):
    content_layers, style_layers = CONTENT_LISTS[name]
    image = T._inputs(size, 'max')['image']
    img = image.to(DEV)
    _, plan = K._plan(size, 'max', precision, content_layers, style_layers, (kind, 'w2'))
    ceps = 1e-8
    if kind == 'scaled_mse':
        ceps = CONTENT_EPS
        plan.set_loss_eps(CONTENT_EPS, None)
        T._set_targets(plan, size, 'max', content_layers, style_layers)       # (a new eps drops the targets)
    kinds = (kind, 'w2')
    names = [f'content[{layer}]' for layer in content_layers]
    plain_terms = K._leg(plan, img, steps=False)[2].cpu().double().numpy()
    plan.set_content_mask(ramp_mask(*size).to(DEV))
    tag = f'content {content_layers} style {style_layers} {size[0]}x{size[1]}-{precision} {kind}, ramp map'
    _, _, _, failures = _judge(tag, plan, img, image, 'max', content_layers, style_layers, kinds, ceps, moved_terms=names)
    assert not failures, '; '.join(failures)
    plan.set_content_mask(torch.ones(size).to(DEV))
    ones_terms = K._leg(plan, img, steps=False)[2].cpu().double().numpy()
    for k, term_name in enumerate(names):
        rel = abs(ones_terms[k] - plain_terms[k]) / abs(plain_terms[k])
        print(f'[maps] {tag}: all-ones map, term {term_name} {ones_terms[k]:.8g} unmasked {plain_terms[k]:.8g} rel {rel:.2e} '
              f'(bar {T.TERM_TOL:.0e})')
        assert rel <= T.TERM_TOL


# ---- 4. everything together -------------------------------------------------------------------------------------------------
def _three_maps(plan):
    plan.set_content_mask(ramp_mask(*SIZE).to(DEV))
    plan.set_tv_mask(binary_mask(*SIZE).to(DEV))
    plan.set_style_mask(ramp_mask(SIZE[1], SIZE[0]).t().contiguous().to(DEV))


def test_all_three_maps_together_on_the_default_layers():
    content_layers, style_layers = T.DEFAULT
    image = T._inputs(SIZE, 'max')['image']
    img = image.to(DEV)
    _, never = K._plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=None, configure=False)
    _, styled = K._plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=None, configure=False)
    styled.set_style_mask(ramp_mask(SIZE[1], SIZE[0]).t().contiguous().to(DEV))
    _, plan = K._plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=None, configure=False)
    _three_maps(plan)
    tag = f'content + tv + style maps, default layers {SIZE[0]}x{SIZE[1]}'
    _, _, _, failures = _judge(tag, plan, img, image, 'max', content_layers, style_layers, ('mse', 'w2'), 1e-8,
                               moved_terms=['content[22]', 'tv'])
    assert not failures, '; '.join(failures)
    first, second = K._leg(plan, img, steps=False), K._leg(plan, img, steps=False)
    assert T._same(first, second), 'two closures on the same inputs must give the same bits'
    plan.set_content_mask(None)
    plan.set_tv_mask(None)
    a, b = K._leg(styled, img, steps=True), K._leg(plan, img, steps=True)
    assert len(a) == 10 and T._same(a, b), 'cleared maps must leave the plan that only ever had the style mask, bit for bit'
    assert not torch.equal(first[1], a[1])
    plan.set_style_mask(None)
    a, b = K._leg(never, img, steps=True), K._leg(plan, img, steps=True)
    assert T._same(a, b), "all three cleared must leave a fresh plan's default closure, bit for bit"


# ---- 5. through the entries -------------------------------------------------------------------------------------------------
def _mapped_default_plan(maps=True):
    _, plan = K._plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=None, configure=False)
    if maps:
        plan.set_content_mask(ramp_mask(*SIZE).to(DEV))
        plan.set_tv_mask(binary_mask(*SIZE).to(DEV))
    return plan


def test_adam_step_lbfgs_step_and_range_guard_on_a_mapped_plan():
    from style_transfer import _hip as hip
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    plan, plain = _mapped_default_plan(), _mapped_default_plan(maps=False)
    before = K._leg(plan, img, steps=False)
    fwd, bwd = plan.range_guard(img)
    assert not any(fwd) and not any(bwd)
    assert T._same(before, K._leg(plan, img, steps=False)), 'the range guard must leave the closure as it was'
    # one native Adam step: the reported terms are loss_and_grad's on the same image, the result closure + update
    xa, ma, va, ea = T._state(img)
    xb, mb, vb, eb = T._state(img)
    la = plan.step(xa, ma, va, ea, 1, 0.02).clone()
    lb, g = plan.loss_and_grad(xb)
    lb = lb.clone()
    plan.apply_update(xb, g, mb, vb, eb, 1, 0.02)
    xc = T._state(img)
    lc = plain.step(*xc, 1, 0.02).clone()
    torch.cuda.synchronize()
    assert torch.equal(la, lb) and torch.equal(la, before[0]), (la, lb, before[0])
    assert torch.equal(xa, xb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(ea, eb)
    assert not torch.equal(xa, img) and not torch.equal(xa, xc[0]) and not torch.equal(la, lc)
    # one native L-BFGS step
    xa, _, _, ea = T._state(img)
    xb, _, _, eb = T._state(img)
    xc, _, _, ec = T._state(img)
    opt_a, opt_b, opt_c = hip.LBFGS(xa), hip.LBFGS(xb), hip.LBFGS(xc)
    la = opt_a.step(plan, xa, ea, 0.99).clone()
    lb, g = plan.loss_and_grad(xb)
    lb = lb.clone()
    opt_b.update(xb, g, eb, 0.99)
    lc = opt_c.step(plain, xc, ec, 0.99).clone()
    torch.cuda.synchronize()
    assert torch.equal(la, lb) and torch.equal(la, before[0])
    assert torch.equal(xa, xb) and torch.equal(ea, eb) and opt_a.info() == opt_b.info()
    assert not torch.equal(xa, img) and not torch.equal(xa, xc) and not torch.equal(la, lc)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['content', 'tv'])
def test_refusals(which):
    from style_transfer import _hip as hip
    from style_transfer import sharding
    entry = f'st_plan_set_{which}_mask'
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    net, plan = K._plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=None, configure=False)
    setter = getattr(plan, f'set_{which}_mask')

    def reader():
        return plan.content_mask_level(0) if which == 'content' else plan.tv_mask()
    plain = K._leg(plan, img, steps=False)
    strip = sharding.StripPlan(net, 48, 48, 0, 32)
    with pytest.raises(hip.HipLibraryError, match=f'{entry}.*strip'):
        getattr(strip, f'set_{which}_mask')(torch.ones((32, 48)).to(DEV))
    with pytest.raises(hip.HipLibraryError, match=f'st_plan_{which}_mask'):
        reader()
    too_large = ramp_mask(*SIZE)
    too_large[7, 9] = 1.5
    with_nan = ramp_mask(*SIZE)
    with_nan[30, 2] = float('nan')
    for bad, pattern in ((too_large, r'\[0, 1\]'), (with_nan, 'NaN'), (torch.zeros(SIZE), 'zero')):
        with pytest.raises(hip.HipLibraryError, match=f'{entry}.*{pattern}'):
            setter(bad.to(DEV))
        with pytest.raises(hip.HipLibraryError, match=f'st_plan_{which}_mask'):       # a refused map leaves the plan without one
            reader()
        assert T._same(plain, K._leg(plan, img, steps=False)), 'after a refused map the plan runs as one without a map'
    with pytest.raises(ValueError, match='40 x 48'):
        setter(torch.ones(ODD).to(DEV))
    setter(ramp_mask(*SIZE).to(DEV))
    mapped = K._leg(plan, img, steps=False)
    assert not torch.equal(mapped[1], plain[1])
    with pytest.raises(hip.HipLibraryError, match=entry):
        setter(too_large.to(DEV))
    assert T._same(plain, K._leg(plan, img, steps=False))
    if which == 'content':
        setter(ramp_mask(*SIZE).to(DEV))
        with pytest.raises(hip.HipLibraryError, match='level'):
            plan.content_mask_level(5)


# ---- 7. stylize() -----------------------------------------------------------------------------------------------------------
def test_stylize_reads_the_map_attributes(monkeypatch):
    from style_transfer import StyleTransfer
    from style_transfer import _hip as hip
    from style_transfer.style_transfer import size_to_fit
    st = StyleTransfer(devices=[DEV], pooling='max', weights='synthetic')
    assert st.content_mask is None and st.tv_mask is None
    content_image, style_image = T._pil(81, 64, 48), T._pil(82, 60, 44)
    st.content_mask = MG._pil_mask(ramp_mask(48, 64))
    st.tv_mask = binary_mask(48, 64).numpy()
    calls = {'content': [], 'tv': []}
    for which in calls:
        original = getattr(hip.Plan, f'set_{which}_mask')

        def wrapped(self, mask, which=which, original=original):
            calls[which].append((self, None if mask is None else tuple(mask.shape)))
            return original(self, mask)
        monkeypatch.setattr(hip.Plan, f'set_{which}_mask', wrapped)
    sizes = []
    out = st.stylize(content_image, [style_image], end_scale=64, min_scale=45, initial_iterations=3, iterations=2,
                     callback=lambda it: sizes.append((it.h, it.w)) if it.i == 1 else None)
    assert out is not None and torch.isfinite(st.get_image_tensor()).all()
    want = [size_to_fit(content_image.size, scale, scale_up=True)[::-1] for scale in (45, 64)]
    assert sizes == want
    for which in calls:
        # once per scale, on the iterate's plan, with a map of that scale's size; no other plan ever received one
        assert [shape for _, shape in calls[which]] == want, (which, calls[which])
        assert all((plan.height, plan.width) == shape for plan, shape in calls[which])
    assert len({id(plan) for plan, _ in calls['content']}) == 2
    assert [id(plan) for plan, _ in calls['content']] == [id(plan) for plan, _ in calls['tv']]
    assert st._plan is calls['content'][-1][0] and st._plan.content_mask_level(0).shape == want[-1]
    assert tuple(st._plan.tv_mask().shape) == want[-1]

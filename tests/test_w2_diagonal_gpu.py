"""Diagonal-covariance W2 style heads (st_plan_set_w2_diagonal, the st_op_channel_* / st_op_w2_diag_* entries,
StyleTransfer.style_diagonal, losses.StyleLossW2Diag) on a real MI355X.

Inputs, plan helpers and bars are tests/test_taps_gpu.py's and tests/test_layer_losses_gpu.py's (and, for the masks, regions, maps
and the Laplacian, the helpers of the tests that introduced them): _smooth images 71 (content), 72 (style), 73 (the iterate),
synthetic_vgg19_weights(0), sizes 40 x 48 and 45 x 54 - the second makes every level's pixel count a non-multiple of 4, so the
tail paths run; relu5_1 has 6 pixels at the first.  The yardstick is oracle/st_oracle.py composed by hand in float32 and in
float64 on the branches of the plan's own plain forward, with include/st_amd.h's formula written out below (_diag_term) for the
flagged layers.

Bars, the project's own, unchanged:
  each weighted term  |hip - fp32 oracle| / |fp32 oracle| <= max(T.TERM_TOL, 3 x the fp32 composition's deviation from float64);
  the total           within T.SUM_TOL of the fp32 sum of the terms;
  image gradient      rel-L2 against float64 <= T.bar(floor), floor = the fp32 composition's own rel-L2 from float64.
A flag that is ignored cannot pass: for every flagged (region, layer) the float64 term of the FULL W2 on the same tap is shown
to differ from the diagonal term by at least 10 of that term's bars; the smallest ratio is printed.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_l2
import st_oracle as O
import test_content_tv_masks_gpu as CM
import test_laplacian_gpu as LG
import test_layer_losses_gpu as L
import test_loss_kinds_gpu as K
import test_style_mask_gpu as MG
import test_style_regions_gpu as R
import test_taps_gpu as T
from test_laplacian_cpu import formula_terms

pytestmark = pytest.mark.gpu
DEV = T.DEV
SIZE, ODD = MG.SIZE, MG.ODD          # 40 x 48 and 45 x 54
ALL = [True] * 5
DEEP = [False, False, False, True, True]
MSE, W2 = ['mse'], ['w2'] * 5
IGNORED_BARS = 10


def _diag_term(feat, m, total, target, eps):
    """include/st_amd.h's term of a flagged entry before its weight: feat [1, C, h, w], m [h, w] the pixel weights and `total`
    their sum, target = the (mean, srm) the plan's setter is given."""
    mat = feat.reshape(feat.shape[1], -1)
    mw = m.reshape(-1)
    mu = (mat * mw).sum(1) / total
    q = (mat * mat * mw).sum(1) / total
    sigma = ((q - mu * mu).clamp(min=0) + eps).sqrt()
    t_mean, t_srm = target
    sigma_t = ((torch.diagonal(t_srm) - t_mean * t_mean).clamp(min=0) + eps).sqrt()
    return (((mu - t_mean) ** 2).sum() + ((sigma - sigma_t) ** 2).sum()) / mat.shape[0]


def _style_term(feat, layer, target, levels, kind, flag, eps, dtype, full=False):
    """The style term of `layer` under the mask `levels` (None: all pixels at weight 1), by the entry's kind, flag and eps.
    full: the full W2 term whatever the flag says."""
    if levels is None:
        h, w = feat.shape[2:]
        m, total = torch.ones((h, w), dtype=dtype), float(h * w)
    else:
        m, total = levels[MG.LEVEL[layer]][0].to(dtype), levels[MG.LEVEL[layer]][1]
    target = (target[0].to(dtype), target[1].to(dtype))
    if kind == 'gram':
        return K._scaled_mse(MG._masked_moments(feat, m, total)[1], target[1])
    e = 1e-4 if eps is None else eps
    if flag and not full:
        return _diag_term(feat, m, total, target, e)
    mean, srm = MG._masked_moments(feat, m, total)
    return MG._w2(mean, srm, O.style_target(target[0], target[1], e), e)


def _oracle(image, pooling, decisions, content_layers, style_layers, ctargets, regions, weights, kinds, flags, seps, clevels, tvmap,
            lap, dtype, full=False):
    """SumLoss in `dtype` with one style term per (region, layer).  regions: a list of (levels or None, moments, rho); lap: None or
    (content image, pools, weight).  Returns the weighted content terms, the weighted (region, layer) terms, the entries' terms
    (the sum of their regions' in region order), the image-space term (TV and the Laplacian's), the total, the gradient and -
    full - the weighted FULL W2 term of every flagged (region, layer)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cws, sws = weights
    img = image.to(dtype).clone().requires_grad_(True)
    feats = O.vgg_features(img, T._weights() if dtype == torch.float32 else T._weights64(), content_layers + style_layers,
                           pooling, decisions)
    cterms = []
    for layer, cw, kind in zip(content_layers, cws, kinds[0]):
        wmap = None if clevels is None else clevels[MG.LEVEL[layer]].to(dtype)
        cterms.append(CM.weighted_content(feats[layer], ctargets[layer].to(dtype), wmap, kind, 1e-8) * cw)
    seps = seps or [None] * len(style_layers)
    rterms = [[_style_term(feats[layer], layer, moments[layer], levels, kind, flag, e, dtype) * (sw * rho)
               for layer, sw, kind, flag, e in zip(style_layers, sws, kinds[1], flags, seps)] for levels, moments, rho in regions]
    entries = []
    for j in range(len(style_layers)):
        entry = rterms[0][j]
        for r in range(1, len(regions)):
            entry = entry + rterms[r][j]
        entries.append(entry)
    space = (O.tv_loss(img) if tvmap is None else CM.weighted_tv(img, tvmap.to(dtype))) * T.TV_WEIGHT
    if lap is not None:
        for term in formula_terms(img, lap[0].to(dtype), lap[1]):
            space = space + term * lap[2]
    total = sum(cterms) + sum(entries) + space
    (grad,) = torch.autograd.grad(total, img)
    fulls = None
    if full:
        with torch.no_grad():
            fulls = [[float(_style_term(feats[layer], layer, moments[layer], levels, kind, flag, e, dtype, full=True) * (sw * rho))
                      if flag else None for layer, sw, kind, flag, e in zip(style_layers, sws, kinds[1], flags, seps)]
                     for levels, moments, rho in regions]
    def f(t):
        return float(t.detach())
    return ([f(t) for t in cterms], [[f(t) for t in row] for row in rterms], [f(t) for t in entries], f(space), f(total),
            grad.detach(), fulls)


def _plan(size, pooling, precision, content_layers, style_layers, kinds, flags, eps=None, configure=True, targets=True):
    """A plan in the documented order: layers, kinds, eps, diagonal, weights, targets.  kinds None: the kinds setter is never
    called; flags None: neither is set_w2_diagonal."""
    from style_transfer import _hip as hip
    net = hip.Net(T._weights(), pooling, DEV, precision)
    plan = hip.Plan(net, *size)
    if configure:
        plan.set_taps(content_layers, style_layers)
    if kinds is not None:
        plan.set_layer_loss_kinds(*kinds)
    if eps is not None:
        plan.set_loss_eps(None, eps)
    if flags is not None:
        plan.set_w2_diagonal(flags)
        assert plan.w2_diagonal == tuple(bool(v) for v in flags)
    plan.set_loss_weights(*T._layer_weights(content_layers, style_layers), T.TV_WEIGHT)
    if targets:
        T._set_targets(plan, size, pooling, content_layers, style_layers)
    return net, plan


def _judge(tag, plan, img, image, pooling, content_layers, style_layers, kinds, flags, seps=None, rhos=None, lap_pools=None):
    """One closure of `plan` against the oracle under the plan's OWN masks and maps.  rhos: the plan has len(rhos) style regions
    (targets: test_style_regions_gpu._region_moments); lap_pools: the plan has a Laplacian of LG.LAP_WEIGHT on these pools
    against LG._content(size).  Returns (failures, the smallest full-vs-diagonal ratio in bars)."""
    from style_transfer import _hip as hip
    size = tuple(image.shape[2:])
    decisions = L._decisions(plan, img, pooling, content_layers, style_layers)

    def held(read):
        try:
            return read()
        except hip.HipLibraryError:
            return None
    clevels = held(lambda: CM._content_levels(plan))
    tvmap = held(lambda: plan.tv_mask().cpu().double())
    if rhos is None:
        regions = [(held(lambda: MG._plan_levels(plan)), T._targets(size, pooling, [], style_layers)[1], 1.0)]
    else:
        regions = [(R._region_levels(plan, r), R._region_moments(size, pooling, style_layers, r), rho) for r, rho in enumerate(rhos)]
    lap = None if lap_pools is None else (LG._content(size), lap_pools, LG.LAP_WEIGHT)
    losses, grad = plan.loss_and_grad(img)
    torch.cuda.synchronize()
    terms = plan.term_losses().cpu().numpy()
    losses = losses.cpu().numpy()
    nc, ns = len(content_layers), len(style_layers)
    got_regions = plan.region_term_losses().cpu().numpy() if rhos is not None else terms[None, nc:nc + ns]
    weights = T._layer_weights(content_layers, style_layers)
    ctargets = T._targets(size, pooling, content_layers, style_layers)[0]
    args = (image, pooling, decisions, content_layers, style_layers, ctargets, regions, weights, kinds, flags, seps, clevels, tvmap,
            lap)
    c32, r32, _, s32, _, g32, _ = _oracle(*args, torch.float32)
    c64, r64, _, s64, _, g64, full64 = _oracle(*args, torch.float64, full=True)
    assert got_regions.shape == (len(regions), ns) and len(terms) == nc + ns + 1, (got_regions.shape, len(terms))
    assert np.isfinite(terms).all() and np.isfinite(losses).all(), f'{tag}: non-finite loss'
    failures, smallest = [], float('inf')

    def check(name, got, want32, want64):
        floor = abs(want32 - want64) / abs(want64)
        tol = max(T.TERM_TOL, 3 * floor)
        rel = abs(got - want32) / abs(want32)
        print(f'[w2diag] {tag} term {name:28s} got {got:.8g} want {want32:.8g} rel {rel:.2e}  floor {floor:.2e}  bar {tol:.1e}  '
              f'{"PASS" if rel <= tol else "FAIL"}')
        if not rel <= tol:
            failures.append(f'{tag}: term {name} rel {rel:.2e} > {tol:.1e}')
        return tol
    for i, layer in enumerate(content_layers):
        check(f'content[{layer}]', float(terms[i]), c32[i], c64[i])
    for r in range(len(regions)):
        for j, layer in enumerate(style_layers):
            what = 'diagonal w2' if flags[j] else kinds[1][j]
            tol = check(f'region {r} style[{layer}] {what}', float(got_regions[r, j]), r32[r][j], r64[r][j])
            if flags[j]:
                # a flag that is ignored: the plan would have computed the full W2 of the same tap
                ratio = abs(full64[r][j] - r64[r][j]) / abs(r64[r][j]) / tol
                smallest = min(smallest, ratio)
                print(f'[w2diag] {tag} region {r} style[{layer}]: the full W2 term {full64[r][j]:.6g} is {ratio:.0f} bars from the '
                      f'diagonal one {r64[r][j]:.6g}')
                assert ratio >= IGNORED_BARS, f'{tag}: region {r} style[{layer}]: the full W2 term is {ratio:.1f} bars away only'
    for j, layer in enumerate(style_layers):          # an entry's term IS the fp32 sum of its regions' terms, in region order
        want = got_regions[0, j]
        for r in range(1, len(regions)):
            want = np.float32(want + got_regions[r, j])
        if not terms[nc + j] == want:
            failures.append(f'{tag}: term style[{layer}] {terms[nc + j]:.9g} is not the fp32 sum of its region terms {want:.9g}')
    check('image-space (tv, laplacian)', float(terms[-1]), s32, s64)
    want_total = np.float32(0)
    for t in terms.astype(np.float32):
        want_total = np.float32(want_total + t)
    rel_total = abs(float(losses[7]) - float(want_total)) / abs(float(want_total))
    print(f'[w2diag] {tag} total {losses[7]:.8g} vs fp32 sum of the terms {want_total:.8g} rel {rel_total:.2e} (bar {T.SUM_TOL:.0e})')
    if not rel_total <= T.SUM_TOL:
        failures.append(f'{tag}: total rel {rel_total:.2e} > {T.SUM_TOL:.0e}')
    assert torch.isfinite(grad).all(), f'{tag}: non-finite gradient'
    err, floor = rel_l2(grad.cpu(), g64), rel_l2(g32, g64)
    b = T.bar(floor)
    print(f'[w2diag] {tag} gradient hip-vs-fp64 {err:.2e}  ref-fp32 floor {floor:.2e}  bar {b:.1e}  {"PASS" if err <= b else "FAIL"}')
    if not err <= b:
        failures.append(f'{tag}: gradient rel-L2 {err:.2e} > {b:.1e} (floor {floor:.2e})')
    print(f'[w2diag] {tag}: smallest distance of a full W2 term from its diagonal term: {smallest:.0f} bars')
    return failures, smallest


# ---- 1. configurations ------------------------------------------------------------------------------------------------------
POOL_AND_CONTENT = ([6], [1, 6, 27])          # relu2_1 is a content layer too; features[27] is a pool output (6 pixels at 40 x 48)
CASES = [
    # name, size, pooling, precision, (content layers, style layers), style kinds, flags, style eps, configure
    ('all-five', SIZE, 'max', 'fp16x3', T.DEFAULT, W2, ALL, None, False),
    ('all-five-odd-fp32', ODD, 'max', 'fp32', T.DEFAULT, W2, ALL, None, False),
    ('deep-two-odd', ODD, 'max', 'fp16x3', T.DEFAULT, W2, DEEP, None, False),
    ('deep-two-fp32', SIZE, 'max', 'fp32', T.DEFAULT, W2, DEEP, None, False),
    ('pool-and-content-average', SIZE, 'average', 'fp16x3', POOL_AND_CONTENT, ['w2'] * 3, [True, True, True], None, True),
    ('pool-and-content-max', ODD, 'max', 'fp16x3', POOL_AND_CONTENT, ['w2'] * 3, [False, True, True], None, True),
    ('with-gram', SIZE, 'max', 'fp16x3', T.DEFAULT, ['w2', 'gram', 'w2', 'gram', 'w2'], [True, False, False, False, True], None, False),
    ('custom-eps', SIZE, 'max', 'fp16x3', T.DEFAULT, W2, [True, False, True, False, True], [1e-2, None, None, 1e-3, 1e-3], False),
]


@pytest.mark.parametrize('name, size, pooling, precision, lists, style_kinds, flags, seps, configure', CASES, ids=[c[0] for c in CASES])
def test_configurations(name, size, pooling, precision, lists, style_kinds, flags, seps, configure):
    content_layers, style_layers = lists
    kinds = (['mse'] * len(content_layers), style_kinds)
    image = T._inputs(size, pooling)['image']
    img = image.to(DEV)
    _, plan = _plan(size, pooling, precision, content_layers, style_layers, None if style_kinds == W2[:len(style_kinds)] else kinds,
                    flags, seps, configure)
    if seps is not None:
        assert plan.style_eps == tuple(np.float32(1e-4 if e is None else e) for e in seps)
    tag = f'({name}) style {style_layers} flags {[int(f) for f in flags]} {size[0]}x{size[1]}-{pooling}-{precision}'
    failures, _ = _judge(tag, plan, img, image, pooling, content_layers, style_layers, kinds, flags, seps)
    if configure:
        L._configured_array(plan.term_losses().cpu().double().numpy(), plan.loss_and_grad(img)[0].cpu().numpy(), len(content_layers),
                            len(style_layers))
    assert not failures, '; '.join(failures)


# ---- 2. everything in force at once -----------------------------------------------------------------------------------------
def test_a_style_mask_both_maps_and_the_laplacian():
    flags = [True, False, True, False, True]
    image = T._inputs(SIZE, 'max')['image']
    _, plan = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, None, flags, configure=False)
    CM._three_maps(plan)                      # a ramp content map, a binary TV map, the transposed ramp as the style mask
    plan.set_laplacian(LG._content(SIZE).to(DEV), (4, 16), LG.LAP_WEIGHT)
    failures, _ = _judge('style mask + content map + TV map + Laplacian, flags 1,0,1,0,1', plan, image.to(DEV), image, 'max',
                         *T.DEFAULT, (MSE, W2), flags, lap_pools=(4, 16))
    assert not failures, '; '.join(failures)


REGION_CASES = [
    ('two-regions', SIZE, [0.5, 0.5], None, ALL, W2),
    ('two-regions-odd', ODD, [0.5, 0.5], None, DEEP, W2),
    ('three-regions-weights', SIZE, [0.5, 0.3, 0.2], [0.5, 0.3, 0.2], [True, False, False, False, True], ['w2', 'gram', 'w2', 'w2', 'w2']),
]


@pytest.mark.parametrize('name, size, rhos, weights, flags, style_kinds', REGION_CASES, ids=[c[0] for c in REGION_CASES])
def test_regions_maps_and_the_laplacian(name, size, rhos, weights, flags, style_kinds):
    image = T._inputs(size, 'max')['image']
    kinds = (MSE, style_kinds)
    _, plan = _plan(size, 'max', 'fp16x3', *T.DEFAULT, None if style_kinds == W2 else kinds, flags, configure=False)
    masks = [MG.ramp_mask(*size), R.complement(*size), MG.binary_mask(*size)][:len(rhos)]
    R._set_regions(plan, size, 'max', T.DEFAULT[1], masks, weights)
    plan.set_content_mask(MG.ramp_mask(*size).to(DEV))
    plan.set_tv_mask(MG.binary_mask(*size).to(DEV))
    plan.set_laplacian(LG._content(size).to(DEV), (4,), LG.LAP_WEIGHT)
    failures, _ = _judge(f'({name}) {len(rhos)} regions + content map + TV map + Laplacian, flags {[int(f) for f in flags]}', plan,
                         image.to(DEV), image, 'max', *T.DEFAULT, kinds, flags, rhos=[float(np.float32(rho)) for rho in rhos],
                         lap_pools=(4,))
    assert not failures, '; '.join(failures)


# ---- 4. bits ----------------------------------------------------------------------------------------------------------------
def _flagged_plan(flags=(True, False, False, True, True), regions=False, mask=False):
    _, plan = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, None, list(flags), configure=False)
    if regions:
        R._set_regions(plan, SIZE, 'max', T.DEFAULT[1], [MG.ramp_mask(*SIZE), R.complement(*SIZE)])
    if mask:
        plan.set_style_mask(MG.ramp_mask(*SIZE).to(DEV))
    return plan


@pytest.mark.parametrize('regions', [False, True], ids=['plain', 'two regions'])
def test_two_closures_are_equal_and_step_is_closure_plus_update(regions):
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    plan = _flagged_plan(regions=regions)
    first = [t.clone() for t in plan.loss_and_grad(img)] + [plan.term_losses().clone()]
    second = [t.clone() for t in plan.loss_and_grad(img)] + [plan.term_losses().clone()]
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
    # the range guard runs the flagged closure and leaves the plan as it was on the unflagged synthetic network
    before = K._leg(plan, img, steps=False)
    fwd, bwd = plan.range_guard(img)
    assert not any(fwd) and not any(bwd)
    assert T._same(before, K._leg(plan, img, steps=False))


def test_lbfgs_step_is_closure_plus_update():
    from style_transfer import _hip as hip
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    plan = _flagged_plan()
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


def test_flags_all_false_and_set_then_cleared_are_the_untouched_plan():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    _, plain = K._plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=None, configure=False)
    want = K._leg(plain, img, steps=True)
    _, zeros = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, None, [False] * 5, configure=False)
    assert zeros.w2_diagonal == (False,) * 5
    assert len(want) == 10 and T._same(want, K._leg(zeros, img, steps=True))
    cleared = _flagged_plan(ALL)
    flagged = K._leg(cleared, img, steps=False)
    assert not torch.equal(flagged[0], want[0])
    cleared.set_w2_diagonal(None)
    assert cleared.w2_diagonal == (False,) * 5
    T._set_targets(cleared, SIZE, 'max', *T.DEFAULT)
    assert T._same(want, K._leg(cleared, img, steps=True))
    assert not torch.equal(want[6], img)


def test_one_region_of_weight_one_is_the_masked_plan():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    masked = _flagged_plan(ALL, mask=True)
    a = K._leg(masked, img, steps=True)
    for weights in (None, [1.0]):
        _, one = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, None, ALL, configure=False)
        R._set_regions(one, SIZE, 'max', T.DEFAULT[1], [MG.ramp_mask(*SIZE)], weights)
        b = K._leg(one, img, steps=True)
        assert len(a) == 10 and T._same(a, b)
        assert torch.equal(one.region_term_losses()[0], one.term_losses()[1:6])
    # ... and the mask is read: the unmasked flagged plan gives other bits
    assert not torch.equal(K._leg(_flagged_plan(ALL), img, steps=False)[0], a[0])


# ---- 5. setter semantics ----------------------------------------------------------------------------------------------------
def _ints(*values):
    return (ctypes.c_int * max(len(values), 1))(*values)


def test_setter_semantics():
    from style_transfer import _hip as hip
    from style_transfer import sharding
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    net = hip.Net(T._weights(), 'max', DEV, 'fp16x3')
    plan = hip.Plan(net, *SIZE)
    lib = plan.lib
    assert plan.w2_diagonal == (False,) * 5
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    before = K._leg(plan, img, steps=False)
    # refusals carry a message and leave the plan as it was, targets included
    assert lib.st_plan_set_w2_diagonal(plan.handle, _ints(0, 0, 0, 0, 2)) != 0
    assert '0 or 1' in lib.st_last_error().decode() and 'st_plan_set_w2_diagonal' in lib.st_last_error().decode()
    assert lib.st_plan_set_w2_diagonal(plan.handle, _ints(0, -1, 0, 0, 0)) != 0
    assert T._same(before, K._leg(plan, img, steps=False))
    plan.set_layer_loss_kinds(MSE, R.MIX)
    assert lib.st_plan_set_w2_diagonal(plan.handle, _ints(0, 0, 0, 1, 0)) != 0
    assert 'gram' in lib.st_last_error().decode()
    with pytest.raises(hip.HipLibraryError, match='gram'):
        plan.set_w2_diagonal(True)
    with pytest.raises(ValueError, match='one per layer'):
        plan.set_w2_diagonal([True] * 4)
    assert plan.w2_diagonal == (False,) * 5
    plan.set_w2_diagonal([True, False, True, False, False])
    assert plan.w2_diagonal == (True, False, True, False, False) and plan.style_losses == tuple(R.MIX)
    # the targets are dropped: the next closure names the first missing one
    plan.set_layer_loss_kinds(MSE, W2)
    assert plan.w2_diagonal == (False,) * 5                                 # (the kinds setter cleared the flags)
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    plan.loss_and_grad(img)
    plan.set_w2_diagonal(DEEP)
    with pytest.raises(hip.HipLibraryError, match=r'content target 0 \(features\[22\]\)'):
        plan.loss_and_grad(img)
    plan.set_content_target(T._targets(SIZE, 'max', *T.DEFAULT)[0][22].to(DEV), 0)
    with pytest.raises(hip.HipLibraryError, match=r'style target 0 \(features\[1\]\)'):
        plan.loss_and_grad(img)
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    assert torch.isfinite(plan.loss_and_grad(img)[0]).all()
    # either kinds setter and set_taps clear the flags
    plan.set_loss_kinds('mse', 'w2')
    assert plan.w2_diagonal == (False,) * 5
    plan.set_w2_diagonal(ALL)
    plan.set_layer_loss_kinds(MSE, W2)
    assert plan.w2_diagonal == (False,) * 5
    plan.set_w2_diagonal(ALL)
    plan.set_taps(*T.CONFIGS['b'])
    assert plan.w2_diagonal == (False,) * 5
    plan.set_w2_diagonal(ALL)
    plan.set_taps(*T.DEFAULT)
    assert plan.w2_diagonal == (False,) * 5
    # back on the default configuration: the fast closure again, equal to a plan that never left it
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    fresh = hip.Plan(net, *SIZE)
    T._set_targets(fresh, SIZE, 'max', *T.DEFAULT)
    assert T._same(K._leg(plan, img, steps=True), K._leg(fresh, img, steps=True))
    # a strip plan takes cleared flags and refuses a set one
    strip = sharding.StripPlan(net, 48, 48, 0, 32)
    assert lib.st_plan_set_w2_diagonal(strip.handle, _ints(0, 0, 0, 0, 1)) != 0
    assert 'strip' in lib.st_last_error().decode()
    assert lib.st_plan_set_w2_diagonal(strip.handle, _ints(0, 0, 0, 0, 0)) == 0
    assert lib.st_plan_set_w2_diagonal(strip.handle, None) == 0


def test_a_flagged_head_allocates_no_c_by_c_workspace():
    """Default lists, targets set: with relu4_1 and relu5_1 flagged the plan holds at least the chain workspaces of two full
    n = 512 W2 heads less - counted here as the nine 512 x 512 matrices a full head's target and chain occupy (cov_t, root_t, cov,
    tmat, mmat, root, gm, dt, dcov), without its Gram partials or its Newton-Schulz scratch."""
    from style_transfer import _hip as hip
    net = hip.Net(T._weights(), 'max', DEV, 'fp16x3')
    used = {}
    for name, flags in (('full', None), ('deep', DEEP), ('all', ALL)):
        plan = hip.Plan(net, *SIZE)
        if flags is not None:
            plan.set_w2_diagonal(flags)
        T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
        torch.cuda.synchronize()
        used[name] = plan.device_bytes()
    print(f'[w2diag] st_plan_device_bytes at 40x48: five full W2 heads {used["full"]}, relu4_1 and relu5_1 diagonal {used["deep"]}, '
          f'all five diagonal {used["all"]}')
    assert used['full'] - used['deep'] >= 2 * 9 * 512 * 512 * 4
    assert used['all'] < used['deep']


# ---- 6. the st_op_* entries alone -------------------------------------------------------------------------------------------
def _formula64(x, mean_t, std_t, eps):
    """test_w2_diagonal_cpu.formula64: (term, dF) at weight 1 for x [C, N] in float64 numpy."""
    from test_w2_diagonal_cpu import formula64
    return formula64(x, mean_t, std_t, eps)


OP_SHAPES = [('one pixel', 'signed', (3, 1, 1)), ('all zeros', 'zeros', (3, 4, 5)), ('C = 1', 'signed', (1, 5, 7)),
             ('C = 3', 'signed', (3, 5, 7)), ('C = 64, one split', 'relu', (64, 8, 8)), ('C = 513', 'signed', (513, 3, 5)),
             ('C = 64, 16-byte groups and splits', 'relu', (64, 96, 100)), ('64 x 208 x 208', 'relu', (64, 208, 208))]


def _op_input(kind, shape, seed):
    g = torch.Generator().manual_seed(seed)
    c = shape[0]
    x = torch.randn(shape, generator=g) * (0.5 + torch.rand((c, 1, 1), generator=g)) + torch.randn((c, 1, 1), generator=g)
    if kind == 'relu':
        x = x.clamp(min=0)
    if kind == 'zeros':
        x = torch.zeros(shape)
    return x.contiguous()


@pytest.mark.parametrize('name, kind, shape', OP_SHAPES, ids=[s[0] for s in OP_SHAPES])
def test_the_operators_alone(name, kind, shape):
    from style_transfer import _hip as hip
    from style_transfer import losses
    c, h, w = shape
    eps = 1e-4
    x = _op_input(kind, shape, 5)
    t = _op_input('signed' if kind == 'zeros' else kind, (c, h + 1, w + 3), 6)
    x64, t64 = x.double().reshape(c, -1).numpy(), t.double().reshape(c, -1).numpy()
    lib = hip.load_library()
    splits = (int(lib.st_op_channel_stats_scratch_floats(c, h * w)) - 4) // (2 * c)
    assert splits >= 1 and (splits == 1) == (h * w <= 4096) and (shape != (64, 208, 208) or splits > 8)
    # the moments
    mean, srm = hip.op_channel_moments(t.to(DEV))
    mean2, srm2 = hip.op_channel_moments(t.to(DEV))
    want_mean, want_srm = t64.mean(1), (t64 * t64).mean(1)
    em = float(np.abs(mean.cpu().double().numpy() - want_mean).max() / max(np.abs(want_mean).max(), 1e-30))
    es = float(np.abs(srm.cpu().double().numpy() - want_srm).max() / max(np.abs(want_srm).max(), 1e-30))
    assert torch.equal(mean, mean2) and torch.equal(srm, srm2)
    # the value and the gradient against the float64 formula, for the float64 target of the same statistics
    mean_t = want_mean
    std_t = np.sqrt(np.maximum(want_srm - want_mean ** 2, 0) + eps)
    want, want_grad = _formula64(x64, mean_t, std_t, eps)
    xd = x.to(DEV)
    mt, st = torch.from_numpy(mean_t).float().to(DEV), torch.from_numpy(std_t).float().to(DEV)
    loss, coeffs = hip.op_w2_diag_loss(xd, mt, st, eps)
    loss2, coeffs2 = hip.op_w2_diag_loss(xd, mt, st, eps)
    up = torch.tensor(-1.75, device=DEV)
    grad = hip.op_w2_diag_loss_backward(xd, coeffs, torch.ones((), device=DEV))
    grad_up = hip.op_w2_diag_loss_backward(xd, coeffs, up)
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2) and torch.equal(coeffs, coeffs2)
    ev = abs(loss.item() - want) / abs(want)
    eg = float(np.linalg.norm(grad.cpu().double().numpy().reshape(c, -1) - want_grad) / np.linalg.norm(want_grad))
    eu = float(np.linalg.norm(grad_up.cpu().double().numpy().reshape(c, -1) + 1.75 * want_grad) / (1.75 * np.linalg.norm(want_grad)))
    print(f'[w2diag] operators {name} {shape} ({splits} splits): moments mean {em:.2e} srm {es:.2e} (bar 1e-6); value {ev:.2e}, '
          f'gradient {eg:.2e}, gradient under upstream -1.75 {eu:.2e} (bars 1e-4)')
    assert em <= 1e-6 and es <= 1e-6
    assert ev <= 1e-4 and eg <= 1e-4 and eu <= 1e-4
    # the module: the native path is taken, agrees with its torch path, and create_graph goes through torch
    module = losses.StyleLossW2Diag((mt, st * st + mt * mt), eps).to(DEV)
    module.std.copy_(st)                      # (the float64 target's sigma itself, not one taken back out of a rounded srm)
    before = losses.native_calls.get('w2_diag', 0)
    xn = xd.clone().requires_grad_()
    value = module(xn)
    value.backward()
    assert losses.native_calls.get('w2_diag', 0) == before + 1
    with losses.native(False):
        xt = xd.clone().requires_grad_()
        value_t = module(xt)
        value_t.backward()
    assert losses.native_calls.get('w2_diag', 0) == before + 1
    assert abs(value.item() - want) / abs(want) <= 1e-4
    assert abs(value.item() - value_t.item()) / abs(value_t.item()) <= 1e-4
    assert rel_l2(xn.grad.cpu(), xt.grad.cpu()) <= 1e-4
    assert rel_l2(xn.grad.cpu().double(), torch.from_numpy(want_grad).reshape(shape)) <= 1e-4


def test_the_module_on_the_device():
    from style_transfer import losses
    x = _op_input('relu', (64, 12, 10), 7).to(DEV)
    target = losses.StyleLossW2Diag.get_target(_op_input('relu', (64, 9, 11), 8).to(DEV)[None])
    assert target[0].shape == (1, 64) and target[1].shape == (1, 64)
    module = losses.StyleLossW2Diag((target[0][0], target[1][0]))
    before = losses.native_calls.get('w2_diag', 0)
    # a batch, float64 and create_graph are the torch code
    assert torch.isfinite(module(torch.stack([x, x]))) and torch.isfinite(module.double()(x.double()))
    module = module.float()
    xg = x.clone().requires_grad_()
    (g,) = torch.autograd.grad(module(xg), xg, create_graph=True)
    assert losses.native_calls.get('w2_diag', 0) == before + 1 and g.requires_grad
    g.pow(2).sum().backward()
    assert torch.isfinite(xg.grad).all()
    # Scale-like upstream factors reach the kernel as a device scalar
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    (module(xa) * 3.5).backward()
    with losses.native(False):
        (module(xb) * 3.5).backward()
    assert rel_l2(xa.grad.cpu(), xb.grad.cpu()) <= 1e-4
    # its own target: the native arithmetic differs from the target's, so the value is tiny, not exactly 0 - and finite
    own = losses.StyleLossW2Diag(losses.StyleLossW2Diag.get_target(x))
    xs = x.clone().requires_grad_()
    v = own(xs)
    v.backward()
    assert 0 <= v.item() <= 1e-10 and torch.isfinite(xs.grad).all()


# ---- 7. stylize() -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('optimizer', ['adam', 'lbfgs'])
def test_stylize_reads_style_diagonal(optimizer):
    from PIL import Image
    from style_transfer import StyleTransfer
    from style_transfer.style_transfer import size_to_fit, to_tensor
    st = StyleTransfer(devices=[DEV], pooling='max', weights='synthetic')
    assert st.style_diagonal is False
    content_image, style_image = T._pil(81, 64, 48), T._pil(82, 60, 44)
    decay = 0.99
    seen = []

    def callback(it):
        if it.i == 1:
            # (the scale's starting image from the EMA and st.image: test_taps_gpu.test_stylize_reads_the_layer_attributes)
            avg, x1 = st.get_image_tensor(), st.image.detach()[0]
            seen.append((it.w, it.h, it.loss, (((1 + decay) * avg - x1) / decay).cpu()[None]))

    def run(min_scale=64):
        del seen[:]
        out = st.stylize(content_image, [style_image], end_scale=64, min_scale=min_scale, initial_iterations=4, iterations=4,
                         optimizer=optimizer, avg_decay=decay, callback=callback)
        assert out is not None and torch.isfinite(st.get_image_tensor()).all()
        return list(seen)

    default_loss = run()[0][2]
    st.style_diagonal = DEEP
    scales = run(min_scale=45)                       # two small scales: the flags are set per scale, before the targets
    assert len(scales) == 2 and scales[0][:2] != scales[1][:2]
    assert st._plan.w2_diagonal == tuple(DEEP)
    (w, h, loss, start), = run()
    assert (w, h) == size_to_fit(content_image.size, 64, scale_up=True)
    content = to_tensor(content_image.resize((w, h), Image.BICUBIC))[None]
    sw_, sh_ = size_to_fit(style_image.size, 64)
    style = to_tensor(style_image.resize((sw_, sh_), Image.BICUBIC))[None]
    with torch.no_grad():
        cfeats = O.vgg_features(content, T._weights(), st.content_layers, 'max')
        sfeats = O.vgg_features(style, T._weights(), st.style_layers, 'max')
    moments = {layer: O.feature_moments(sfeats[layer]) for layer in st.style_layers}
    totals = {}
    for flags in (DEEP, [False] * 5):
        args = (start, 'max', None, st.content_layers, st.style_layers, cfeats, [(None, moments, 1.0)], ([0.015], st.style_weights),
                (MSE, W2), flags, None, None, None, None)
        totals[tuple(flags)] = (_oracle(*args, torch.float32)[4], _oracle(*args, torch.float64)[4])
    total32, total64 = totals[tuple(DEEP)]
    floor = abs(total32 - total64) / abs(total64)
    tol, rel = max(T.TERM_TOL, 3 * floor), abs(loss - total32) / abs(total32)
    ignored = abs(totals[(False,) * 5][1] - total64) / abs(total64)
    print(f'[w2diag] stylize {optimizer} {w}x{h}: first loss {loss:.8g} oracle {total32:.8g} rel {rel:.2e} floor {floor:.2e} '
          f'bar {tol:.1e}; with full W2 heads the float64 total is {ignored / tol:.0f} bars away; the default run: {default_loss:.8g}')
    assert rel <= tol, f'{optimizer} {w}x{h}: first loss rel {rel:.2e} > {tol:.1e}'
    assert ignored >= IGNORED_BARS * tol
    # True: every w2 layer; the same object with the attribute back at its default: the default run again
    st.style_diagonal = True
    run()
    assert st._plan.w2_diagonal == (True,) * 5
    del st.style_diagonal
    assert run()[0][2] == default_loss and st._plan.w2_diagonal == (False,) * 5
    st.style_diagonal = [True, True]
    with pytest.raises(ValueError, match='style_diagonal'):
        st.stylize(content_image, [style_image], end_scale=64, min_scale=64, initial_iterations=1, iterations=1)

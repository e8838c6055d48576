"""Several style regions, each with its own style (st_plan_set_style_regions, _hip.Plan.set_style_regions,
StyleTransfer.style_regions / style_image_regions / style_region_weights) on a real MI355X.

The reference has no such feature; the yardstick is the math of include/st_amd.h in float64: the style mask's formulas
(test_style_mask_gpu) once per region.  With m_r region r's mask at a tap's level and M_r = sum m_r, the term of (region r,
style entry j) is entry j's module - StyleLossW2 or StyleLoss - on
    mean = sum_p m_r,p f_p / M_r,   srm = sum_p m_r,p f_p f_p^T / M_r
against region r's target, times style_weight[j] rho_r; an entry's term is the fp32 sum of its regions' terms in region order;
the gradient is autograd's.  Inputs, region 0's targets, weights and bars are test_taps_gpu's / test_style_mask_gpu's:
  each region term    |hip - fp32 oracle| / |fp32 oracle| <= max(1e-4, 3 x the fp32 oracle's deviation from float64);
  each entry's term   EQUAL to the fp32 sum of its region terms in region order; content and TV terms under the first bar;
  the total           within 1e-6 of the fp32 sum of the terms;
  image gradient      rel-L2 against float64 <= min(5e-3, max(1e-4, 1.5 x the fp32 oracle's own rel-L2 from float64)).
A region that is ignored or mixed up cannot pass: in float64 every region term differs by >= 100 bars from the same term under
another region's mask and from the same term against another region's target (measured on the CPU at 40 x 48, default layers,
W2: the smallest such move is 1 614 bars - features[29], region 0, other mask -, every other one >= 2 872 bars; the fp32
floors are <= 1.3e-5, so every bar is 1e-4).
"""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_l2
import st_oracle as O
import test_loss_kinds_gpu as K
import test_style_mask_gpu as M
import test_taps_gpu as T

pytestmark = pytest.mark.gpu
DEV = T.DEV
SIZE, ODD = M.SIZE, M.ODD      # ODD: tap pixel counts 2430, 594, 143, 30 and 6 - every tail of the add kernel
MIX = ['w2', 'w2', 'w2', 'gram', 'gram']


def complement(h, w):
    return (1 - M.ramp_mask(h, w)).contiguous()


@functools.lru_cache(maxsize=None)
def _other_moments(pooling, seed=74):
    """Region 1's targets: the moments of the oracle's features of _smooth(74, 36, 44), at all 17 taps."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    with torch.no_grad():
        feats = O.vgg_features(T._smooth(seed, 36, 44), T._weights(), list(range(1, 30)), pooling)
    return {layer: O.feature_moments(feat) for layer, feat in feats.items()}


def _region_moments(size, pooling, style_layers, r):
    """Region 0: test_taps_gpu._targets'; region 1: _other_moments; region 2: the moments of test_taps_gpu's CONTENT features."""
    if r == 0:
        return T._targets(size, pooling, [], style_layers)[1]
    if r == 1:
        return {layer: _other_moments(pooling)[layer] for layer in style_layers}
    return {layer: O.feature_moments(T._inputs(size, pooling)['cfeats'][layer]) for layer in style_layers}


def _set_regions(plan, size, pooling, style_layers, masks, weights=None):
    plan.set_style_regions([m.to(DEV) for m in masks])
    if weights is not None:
        plan.set_region_weights(weights)
    for r in range(len(masks)):
        moments = _region_moments(size, pooling, style_layers, r)
        for j, layer in enumerate(style_layers):
            plan.set_region_style_target(r, j, moments[layer][0].to(DEV), moments[layer][1].to(DEV))


def _region_levels(plan, r):
    """Region r's own levels as (m = s^2 in float64, M): what the plan's kernels weigh with."""
    out = []
    for k in range(5):
        s, total = plan.style_region_level(r, k)
        out.append((s.cpu().double() ** 2, total))
    return out


def _plan(size, pooling, precision, content_layers, style_layers, style_kinds, configure=True):
    """test_loss_kinds_gpu._plan with one style kind per layer (a name: every layer)."""
    uniform = isinstance(style_kinds, str)
    net, plan = K._plan(size, pooling, precision, content_layers, style_layers,
                        None if style_kinds == 'w2' else ('mse', style_kinds) if uniform else None, configure)
    if not uniform:
        plan.set_layer_loss_kinds(['mse'] * len(content_layers), list(style_kinds))
        T._set_targets(plan, size, pooling, content_layers, style_layers)
        plan.set_loss_weights(*T._layer_weights(content_layers, style_layers), T.TV_WEIGHT)
    return net, plan


def _oracle(image, pooling, decisions, content_layers, style_layers, ctargets, regions, weights, kinds, dtype, moves=False):
    """SumLoss with one style term per (region, layer) in `dtype`.  regions: a list of (levels, moments, rho).  Returns the
    weighted terms in SumLoss order (an entry's: the sum of its regions' in region order), the weighted region terms [R][ns],
    the total, the gradient and - moves - every region term under the NEXT region's mask and against the NEXT region's target."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cws, sws = weights
    img = image.to(dtype).clone().requires_grad_(True)
    feats = O.vgg_features(img, T._weights() if dtype == torch.float32 else T._weights64(), content_layers + style_layers,
                           pooling, decisions)
    terms = [O.content_mse(feats[layer], ctargets[layer].to(dtype)) * cw for layer, cw in zip(content_layers, cws)]
    region_terms = [[M._style_term(feats[layer], layer, moments, levels, kind, dtype) * (sw * rho)
                     for layer, sw, kind in zip(style_layers, sws, kinds)] for levels, moments, rho in regions]
    for j in range(len(style_layers)):
        entry = region_terms[0][j]
        for r in range(1, len(regions)):
            entry = entry + region_terms[r][j]
        terms.append(entry)
    terms.append(O.tv_loss(img) * T.TV_WEIGHT)
    total = sum(terms)
    (grad,) = torch.autograd.grad(total, img)
    other_mask = other_target = None
    if moves:
        with torch.no_grad():
            nxt = [regions[(r + 1) % len(regions)] for r in range(len(regions))]
            other_mask = [[float(M._style_term(feats[layer], layer, moments, n[0], kind, dtype) * (sw * rho))
                           for layer, sw, kind in zip(style_layers, sws, kinds)] for (_, moments, rho), n in zip(regions, nxt)]
            other_target = [[float(M._style_term(feats[layer], layer, n[1], levels, kind, dtype) * (sw * rho))
                             for layer, sw, kind in zip(style_layers, sws, kinds)] for (levels, _, rho), n in zip(regions, nxt)]
    return ([float(t.detach()) for t in terms], [[float(t.detach()) for t in row] for row in region_terms], float(total.detach()),
            grad.detach(), other_mask, other_target)


def _judge(tag, plan, img, image, pooling, content_layers, style_layers, kinds, rhos):
    """test_style_mask_gpu._judge per (region, layer), with the plan's own levels as the masks."""
    size = tuple(image.shape[2:])
    deepest = max(content_layers + style_layers)
    plan.forward(img, deepest)
    torch.cuda.synchronize()
    decisions = O.decisions_from_maps({idx: plan.feature(idx).cpu() for idx in T.RELUS if idx <= deepest}, pooling)
    regions = [(_region_levels(plan, r), _region_moments(size, pooling, style_layers, r), rho) for r, rho in enumerate(rhos)]
    losses, grad = plan.loss_and_grad(img)
    torch.cuda.synchronize()
    terms = plan.term_losses().cpu().numpy()
    got = plan.region_term_losses().cpu().numpy()
    losses = losses.cpu().numpy()
    weights = T._layer_weights(content_layers, style_layers)
    ctargets = T._targets(size, pooling, content_layers, style_layers)[0]
    args = (image, pooling, decisions, content_layers, style_layers, ctargets, regions, weights, kinds)
    t32, r32, _, g32, _, _ = _oracle(*args, torch.float32)
    t64, r64, _, g64, mask64, target64 = _oracle(*args, torch.float64, moves=True)
    nc, ns = len(content_layers), len(style_layers)
    failures = []
    assert got.shape == (len(rhos), ns) and len(terms) == nc + ns + 1, (got.shape, len(terms))
    for r in range(len(rhos)):
        for j, layer in enumerate(style_layers):
            floor = abs(r32[r][j] - r64[r][j]) / abs(r64[r][j])
            tol = max(T.TERM_TOL, 3 * floor)
            rel = abs(float(got[r, j]) - r32[r][j]) / abs(r32[r][j])
            moved_mask = abs(r64[r][j] - mask64[r][j]) / abs(r64[r][j])
            moved_target = abs(r64[r][j] - target64[r][j]) / abs(r64[r][j])
            print(f'[regions] {tag} region {r} style[{layer}] got {got[r, j]:.8g} want {r32[r][j]:.8g} rel {rel:.2e}  floor {floor:.2e}  '
                  f'bar {tol:.1e}  {"PASS" if rel <= tol else "FAIL"};  another mask moves it by {moved_mask / tol:.0f} bars, another '
                  f'target by {moved_target / tol:.0f} bars')
            if not rel <= tol:
                failures.append(f'{tag}: region {r} term style[{layer}] rel {rel:.2e} > {tol:.1e}')
            assert moved_mask >= 100 * tol, f'{tag}: region {r} style[{layer}]: another mask moves it by {moved_mask / tol:.1f} bars only'
            assert moved_target >= 100 * tol, f'{tag}: region {r} style[{layer}]: another target moves it by {moved_target / tol:.1f} bars only'
    for j, layer in enumerate(style_layers):          # an entry's term IS the fp32 sum of its regions' terms, in region order
        want = got[0, j]
        for r in range(1, len(rhos)):
            want = np.float32(want + got[r, j])
        if not terms[nc + j] == want:
            failures.append(f'{tag}: term style[{layer}] {terms[nc + j]:.9g} is not the fp32 sum of its region terms {want:.9g}')
    for k, name in [(i, f'content[{layer}]') for i, layer in enumerate(content_layers)] + [(nc + ns, 'tv')]:
        floor = abs(t32[k] - t64[k]) / abs(t64[k])
        tol = max(T.TERM_TOL, 3 * floor)
        rel = abs(float(terms[k]) - t32[k]) / abs(t32[k])
        print(f'[regions] {tag} term {name:12s} got {terms[k]:.8g} want {t32[k]:.8g} rel {rel:.2e}  floor {floor:.2e}  bar {tol:.1e}')
        if not rel <= tol:
            failures.append(f'{tag}: term {name} rel {rel:.2e} > {tol:.1e}')
    want_total = np.float32(0)
    for t in terms.astype(np.float32):
        want_total = np.float32(want_total + t)
    rel_total = abs(float(losses[7]) - float(want_total)) / abs(float(want_total))
    print(f'[regions] {tag} total {losses[7]:.8g} vs fp32 sum of the terms {want_total:.8g} rel {rel_total:.2e} (bar {T.SUM_TOL:.0e})')
    if not rel_total <= T.SUM_TOL:
        failures.append(f'{tag}: total rel {rel_total:.2e} > {T.SUM_TOL:.0e}')
    assert torch.isfinite(grad).all(), f'{tag}: non-finite gradient'
    err, floor = rel_l2(grad.cpu(), g64), rel_l2(g32, g64)
    b = T.bar(floor)
    print(f'[regions] {tag} gradient hip-vs-fp64 {err:.2e}  ref-fp32 floor {floor:.2e}  bar {b:.1e}  {"PASS" if err <= b else "FAIL"}')
    if not err <= b:
        failures.append(f'{tag}: gradient rel-L2 {err:.2e} > {b:.1e} (floor {floor:.2e})')
    return failures


# ---- 1. the pyramids --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [SIZE, ODD], ids=lambda s: f'{s[0]}x{s[1]}')
def test_pyramids(size):
    """Region r's levels and sums are, bit for bit, what set_style_mask gives for the same mask; two calls give equal bits;
    the levels are readable after set_taps (the regions survive it)."""
    _, plan = M._net_plan(size)
    masks = [M.ramp_mask(*size), complement(*size), M.binary_mask(*size)]
    want = []
    for mask in masks:
        plan.set_style_mask(mask.to(DEV))
        want.append([plan.style_mask_level(k) for k in range(5)])
    plan.set_style_mask(None)
    reads = []
    for _ in range(2):
        plan.set_style_regions([m.to(DEV) for m in masks])
        reads.append([[plan.style_region_level(r, k) for k in range(5)] for r in range(3)])
    plan.set_taps([22], [3, 8])
    reads.append([[plan.style_region_level(r, k) for k in range(5)] for r in range(3)])
    torch.cuda.synchronize()
    for read in reads:
        for r in range(3):
            for k in range(5):
                assert tuple(read[r][k][0].shape) == (size[0] >> k, size[1] >> k)
                assert torch.equal(read[r][k][0], want[r][k][0]) and read[r][k][1] == want[r][k][1], (r, k)
    assert not torch.equal(reads[0][0][0][0], reads[0][1][0][0])


# ---- 2. the closure against the oracle --------------------------------------------------------------------------------------
CLOSURES = [
    ('default-w2', T.DEFAULT, 'w2', SIZE, 'max', 'fp16x3'),
    ('default-gram', T.DEFAULT, 'gram', SIZE, 'max', 'fp16x3'),
    ('default-mix', T.DEFAULT, MIX, SIZE, 'max', 'fp16x3'),
    ('b', T.CONFIGS['b'], 'w2', SIZE, 'max', 'fp16x3'),           # 29 in both lists: the content term adds onto the accumulated seed
    ('d-average', T.CONFIGS['d'], 'w2', SIZE, 'average', 'fp16x3'),
    ('default-odd', T.DEFAULT, 'w2', ODD, 'max', 'fp16x3'),
    ('default-fp32', T.DEFAULT, 'w2', SIZE, 'max', 'fp32'),
]


@pytest.mark.parametrize('name, lists, style_kinds, size, pooling, precision', CLOSURES, ids=[c[0] for c in CLOSURES])
def test_two_regions_against_the_oracle(name, lists, style_kinds, size, pooling, precision):
    content_layers, style_layers = lists
    image = T._inputs(size, pooling)['image']
    _, plan = _plan(size, pooling, precision, content_layers, style_layers, style_kinds)
    _set_regions(plan, size, pooling, style_layers, [M.ramp_mask(*size), complement(*size)])
    kinds = [style_kinds] * len(style_layers) if isinstance(style_kinds, str) else style_kinds
    tag = f'({name}) content {content_layers} style {style_layers} {size[0]}x{size[1]}-{pooling}-{precision} {style_kinds}'
    failures = _judge(tag, plan, image.to(DEV), image, pooling, content_layers, style_layers, kinds, [0.5, 0.5])
    assert not failures, '; '.join(failures)


def test_three_overlapping_regions_with_weights():
    content_layers, style_layers = T.DEFAULT
    image = T._inputs(SIZE, 'max')['image']
    _, plan = _plan(SIZE, 'max', 'fp16x3', content_layers, style_layers, 'w2')
    rhos = [0.5, 0.3, 0.2]
    _set_regions(plan, SIZE, 'max', style_layers, [M.ramp_mask(*SIZE), complement(*SIZE), M.binary_mask(*SIZE)], rhos)
    failures = _judge('three regions (ramp, complement, binary), weights 0.5 0.3 0.2', plan, image.to(DEV), image, 'max',
                      content_layers, style_layers, ['w2'] * 5, [float(np.float32(rho)) for rho in rhos])
    assert not failures, '; '.join(failures)


# ---- 3. bits ----------------------------------------------------------------------------------------------------------------
def _default_plan(masks=None, weights=None):
    _, plan = K._plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=None, configure=False)
    if masks is not None:
        _set_regions(plan, SIZE, 'max', T.DEFAULT[1], masks, weights)
    return plan


def _two_masks():
    return [M.ramp_mask(*SIZE), complement(*SIZE)]


def test_one_region_of_weight_one_is_the_masked_plan_bit_for_bit():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    masked = _default_plan()
    masked.set_style_mask(M.ramp_mask(*SIZE).to(DEV))
    for weights in (None, [1.0]):
        one = _default_plan([M.ramp_mask(*SIZE)], weights)
        a, b = K._leg(masked, img, steps=True), K._leg(one, img, steps=True)
        assert len(a) == 10 and T._same(a, b)
        # the one region's terms ARE the entries' terms
        assert torch.equal(one.region_term_losses()[0], one.term_losses()[1:6])


def test_two_closures_are_equal_and_step_is_closure_plus_update():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    plan = _default_plan(_two_masks())
    first = [t.clone() for t in plan.loss_and_grad(img)] + [plan.region_term_losses()]
    second = [t.clone() for t in plan.loss_and_grad(img)] + [plan.region_term_losses()]
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
    plan = _default_plan(_two_masks())
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


def test_cleared_regions_leave_the_plan_that_never_had_any_and_the_range_guard_sees_the_regions():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    never = _default_plan()
    plan = _default_plan(_two_masks())
    with_regions = K._leg(plan, img, steps=False)
    # the range guard runs the regions' closure, flags nothing on the synthetic network and leaves the closure as it was
    fwd, bwd = plan.range_guard(img)
    assert not any(fwd) and not any(bwd)
    assert T._same(with_regions, K._leg(plan, img, steps=False))
    plan.set_style_regions(None)
    a, b = K._leg(never, img, steps=True), K._leg(plan, img, steps=True)
    assert len(a) == 10 and T._same(a, b)
    assert not torch.equal(with_regions[1], a[1])


def test_two_all_ones_regions_with_equal_targets_are_the_all_ones_masked_plan():
    """rho = 1/2, 1/2, the same mask and the same targets: each entry's term is t/2 + t/2 - within 1e-6 relative of the
    all-ones-masked plan's t (one rounding of the weight's product and one of the sum, 2^-24 each)."""
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    ones = torch.ones(SIZE)
    masked = _default_plan()
    masked.set_style_mask(ones.to(DEV))
    want = K._leg(masked, img, steps=False)[2].cpu().double()
    plan = _default_plan()
    plan.set_style_regions([ones.to(DEV), ones.to(DEV)])
    moments = _region_moments(SIZE, 'max', T.DEFAULT[1], 0)
    for j, layer in enumerate(T.DEFAULT[1]):
        plan.set_region_style_target(1, j, moments[layer][0].to(DEV), moments[layer][1].to(DEV))
    got = K._leg(plan, img, steps=False)[2].cpu().double()
    rel = ((got - want).abs() / want.abs())[1:6]
    print(f'[regions] two all-ones regions vs the all-ones mask: terms rel {[f"{v:.1e}" for v in rel.tolist()]} (bar 1e-6)')
    assert float(rel.max()) <= 1e-6


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals():
    from style_transfer import _hip as hip
    from style_transfer import sharding
    net, plan = M._net_plan(ODD)
    ramp = M.ramp_mask(*ODD).to(DEV)

    def none_in_force():
        with pytest.raises(hip.HipLibraryError, match='no style regions'):
            plan.style_region_level(0, 0)
        with pytest.raises(hip.HipLibraryError, match='no style regions'):
            plan.region_term_losses()

    strip = sharding.StripPlan(net, 48, 48, 0, 32)
    with pytest.raises(hip.HipLibraryError, match='strip'):
        strip.set_style_regions([torch.ones((32, 48)).to(DEV)])
    none_in_force()
    plan.set_style_regions([ramp])
    with pytest.raises(hip.HipLibraryError, match='5 regions'):
        plan.set_style_regions([ramp] * 5)
    none_in_force()                                 # a refused call leaves no regions in force
    plan.set_style_regions([ramp, ramp])
    last_row = torch.zeros(ODD)
    last_row[44] = 1                                # the row that the 22-row level drops
    with pytest.raises(hip.HipLibraryError, match=r'region 1.*level 1'):
        plan.set_style_regions([ramp, last_row.to(DEV)])
    none_in_force()
    with pytest.raises(hip.HipLibraryError, match=r'region 2.*level 0'):
        plan.set_style_regions([ramp, ramp, torch.zeros(ODD).to(DEV)])
    with_nan = M.ramp_mask(*ODD)
    with_nan[30, 2] = float('nan')
    with pytest.raises(hip.HipLibraryError, match=r'region 0.*NaN'):
        plan.set_style_regions([with_nan.to(DEV), ramp])
    too_large = M.ramp_mask(*ODD)
    too_large[7, 9] = 1.5
    with pytest.raises(hip.HipLibraryError, match=r'region 1.*\[0, 1\]'):
        plan.set_style_regions([ramp, too_large.to(DEV)])
    none_in_force()
    with pytest.raises(ValueError, match='45 x 54'):
        plan.set_style_regions([ramp, torch.ones(SIZE).to(DEV)])
    # targets and weights of a region that is not there
    mean, srm = _other_moments('max')[1]
    with pytest.raises(hip.HipLibraryError, match='region 1 out of range'):
        plan.set_region_style_target(1, 0, mean.to(DEV), srm.to(DEV))
    plan.set_style_regions([ramp, ramp])
    with pytest.raises(hip.HipLibraryError, match='region 2 out of range'):
        plan.set_region_style_target(2, 0, mean.to(DEV), srm.to(DEV))
    with pytest.raises(ValueError, match='3 region weights for 2'):
        plan.set_region_weights([1, 1, 1])
    with pytest.raises(hip.HipLibraryError, match='region 2 out of range'):
        plan.style_region_level(2, 0)
    # the style mask and the regions exclude each other; either may always be cleared
    with pytest.raises(hip.HipLibraryError, match='st_plan_set_style_regions'):
        plan.set_style_mask(ramp)
    plan.set_style_mask(None)
    assert plan.style_region_level(1, 4)[0].shape == (2, 3)
    plan.set_style_regions(None)
    plan.set_style_mask(ramp)
    with pytest.raises(hip.HipLibraryError, match='st_plan_set_style_mask'):
        plan.set_style_regions([ramp, ramp])
    plan.set_style_regions(None)
    assert plan.style_mask_level(0)[0].shape == ODD
    none_in_force()


def test_a_closure_with_one_region_target_missing_is_refused():
    from style_transfer import _hip as hip
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    plan = _default_plan()
    plan.set_style_regions([m.to(DEV) for m in _two_masks()])
    moments = _region_moments(SIZE, 'max', T.DEFAULT[1], 1)
    for j, layer in enumerate(T.DEFAULT[1]):
        if j != 3:
            plan.set_region_style_target(1, j, moments[layer][0].to(DEV), moments[layer][1].to(DEV))
    with pytest.raises(hip.HipLibraryError, match=r'style target 3 \(features\[20\]\) of region 1 not set'):
        plan.loss_and_grad(img)
    plan.set_region_style_target(1, 3, moments[20][0].to(DEV), moments[20][1].to(DEV))
    losses, _ = plan.loss_and_grad(img)
    assert torch.isfinite(losses).all()
    plan.set_taps(*T.CONFIGS['a'])                  # the regions survive, the targets do not
    T._set_targets(plan, SIZE, 'max', *T.CONFIGS['a'])
    with pytest.raises(hip.HipLibraryError, match=r'style target 0 \(features\[1\]\) of region 1 not set'):
        plan.loss_and_grad(img)


# ---- 5. stylize() -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('optimizer', ['adam', 'lbfgs'])
def test_stylize_reads_the_region_attributes(optimizer):
    from PIL import Image
    from style_transfer import StyleTransfer
    from style_transfer.style_transfer import size_to_fit, to_tensor
    st = StyleTransfer(devices=[DEV], pooling='max', weights='synthetic')
    assert st.style_regions is None and st.style_image_regions is None and st.style_region_weights is None
    content_image, style_images = T._pil(81, 64, 48), [T._pil(82, 60, 44), T._pil(83, 56, 40)]
    st.style_regions = [M._pil_mask(M.ramp_mask(48, 64)), M._pil_mask(complement(48, 64))]
    st.style_image_regions = [1, 0]                 # the first image gives region 1's style
    st.style_image_masks = [M._pil_mask(M.binary_mask(44, 60)), None]
    decay = 0.99
    seen = []

    def callback(it):
        if it.i == 1:
            avg, x1 = st.get_image_tensor(), st.image.detach()[0]
            seen.append((it.w, it.h, it.loss, (((1 + decay) * avg - x1) / decay).cpu()[None]))

    out = st.stylize(content_image, style_images, end_scale=64, min_scale=45, initial_iterations=6, iterations=4,
                     optimizer=optimizer, avg_decay=decay, callback=callback)
    assert out is not None and torch.isfinite(st.get_image_tensor()).all() and len(seen) == 2
    cws, sws = [0.015], st.style_weights
    for (w, h, loss, start), scale in zip(seen, (45, 64)):
        assert (w, h) == size_to_fit(content_image.size, scale, scale_up=True)
        content = to_tensor(content_image.resize((w, h), Image.BICUBIC))[None]
        with torch.no_grad():
            cfeats = O.vgg_features(content, T._weights(), st.content_layers, 'max')
        regions = [None, None]
        for i, style_image in enumerate(style_images):
            sw_, sh_ = size_to_fit(style_image.size, scale)
            style = to_tensor(style_image.resize((sw_, sh_), Image.BICUBIC))[None]
            with torch.no_grad():
                sfeats = O.vgg_features(style, T._weights(), st.style_layers, 'max')
            if st.style_image_masks[i] is None:
                moments = {layer: O.feature_moments(sfeats[layer]) for layer in st.style_layers}
            else:
                lv = M._sized_levels(st.style_image_masks[i], sw_, sh_)
                moments = {layer: M._masked_moments(sfeats[layer], lv[M.LEVEL[layer]][0].float(), lv[M.LEVEL[layer]][1])
                           for layer in st.style_layers}
            r = st.style_image_regions[i]
            regions[r] = (M._sized_levels(st.style_regions[r], w, h), moments, 0.5)
        args = (start, 'max', None, st.content_layers, st.style_layers, cfeats, regions, (cws, sws), ['w2'] * 5)
        total32 = _oracle(*args, torch.float32)[2]
        total64 = _oracle(*args, torch.float64)[2]
        floor = abs(total32 - total64) / abs(total64)
        tol, rel = max(T.TERM_TOL, 3 * floor), abs(loss - total32) / abs(total32)
        print(f'[regions] stylize {optimizer} {w}x{h}: first loss {loss:.8g} oracle {total32:.8g} rel {rel:.2e} floor {floor:.2e} '
              f'bar {tol:.1e}')
        assert rel <= tol, f'{optimizer} {w}x{h}: first loss rel {rel:.2e} > {tol:.1e}'
    if optimizer == 'lbfgs':
        return
    # each refusal of _resolve_style_regions, through stylize()
    kwargs = dict(end_scale=64, min_scale=45, initial_iterations=1, iterations=1)
    for attrs, message in [
            (dict(style_image_regions=[0]), 'style_image_regions'),
            (dict(style_image_regions=None), 'style_image_regions'),
            (dict(style_image_regions=[0, 2]), r'style_image_regions\[1\]'),
            (dict(style_image_regions=[1, 1]), 'region 0 has no style image'),
            (dict(style_regions=[st.style_regions[0]] * 5), '5 regions'),
            (dict(style_mask=st.style_regions[0]), 'style_mask together with style_regions'),
            (dict(style_region_weights=[1.0]), 'style_region_weights'),
            (dict(style_region_weights=[0.0, 0.0]), 'style_region_weights')]:
        saved = {name: getattr(st, name) for name in attrs}
        for name, value in attrs.items():
            setattr(st, name, value)
        with pytest.raises(ValueError, match=message):
            st.stylize(content_image, style_images, **kwargs)
        for name, value in saved.items():
            setattr(st, name, value)
    with pytest.raises(ValueError, match='sum to 0'):
        st.stylize(content_image, style_images, style_weights=[0, 1], **kwargs)

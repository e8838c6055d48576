"""Spatial masks for the style statistics (st_plan_set_style_mask, _hip.Plan.set_style_mask, StyleTransfer.style_mask /
style_image_masks) on a real MI355X.

The reference has no such feature; the yardstick is the math of include/st_amd.h in float64.  With m the mask at a tap's
level (level k + 1 = avg_pool2d(level k, 2); a tap's level = the pools at or before it) and M = sum m:
    mean_m = sum_p m_p f_p / M,   srm_m = sum_p m_p f_p f_p^T / M
replace StyleLossW2.get_target(input) inside StyleLossW2.forward and F F^T / N inside StyleLoss.forward; the gradient is
autograd's on those formulas.  Inputs, targets, weights and bars are test_taps_gpu's / test_loss_kinds_gpu's, unchanged:
  each weighted term  |hip - fp32 oracle| / |fp32 oracle| <= max(1e-4, 3 x the fp32 oracle's deviation from float64);
  the total           within 1e-6 of the fp32 sum of the terms;
  image gradient      rel-L2 against float64 <= min(5e-3, max(1e-4, 1.5 x the fp32 oracle's own rel-L2 from float64));
  moments             1e-6 rel-L2 against float64 on the plan's own tap (test_kernels_gpu.test_moments_of_taps' bar for that).
A mask that is ignored cannot pass: every masked float64 style term differs from its unmasked value by >= 100 bars.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
import st_oracle as O
import test_kernels_gpu as KG
import test_loss_kinds_gpu as K
import test_taps_gpu as T

pytestmark = pytest.mark.gpu
DEV = T.DEV
SIZE = (40, 48)
ODD = (45, 54)       # drops an odd row or column at several levels (22 x 27, 11 x 13, 5 x 6, 2 x 3); tap pixel counts 2430, 594,
                     # 143, 30, 6: the pointwise kernel's tails
LEVEL = {1: 0, 3: 0, 4: 1, 6: 1, 8: 1, 9: 2, 11: 2, 13: 2, 15: 2, 17: 2, 18: 3, 20: 3, 22: 3, 24: 3, 26: 3, 27: 4, 29: 4}


def ramp_mask(h, w):
    """m[y, x] = clamp(2 (x / (W - 1) - 0.25), 0, 1) (0.5 + 0.5 y / (H - 1)): a quarter exact zeros, a band of exact ones."""
    x = torch.arange(w, dtype=torch.float64) / (w - 1)
    y = torch.arange(h, dtype=torch.float64) / (h - 1)
    return ((2 * (x - 0.25)).clamp(0, 1)[None, :] * (0.5 + 0.5 * y)[:, None]).float().contiguous()


def binary_mask(h, w):
    m = torch.zeros((h, w))
    m[:math.ceil(h / 2), :math.ceil(w / 2)] = 1
    return m


MASKS = {'ramp': ramp_mask, 'binary': binary_mask}


def pyramid(mask):
    levels = [mask]
    for _ in range(4):
        levels.append(F.avg_pool2d(levels[-1][None, None], 2)[0, 0])
    return levels


def _net_plan(size, precision='fp16x3', pooling='max'):
    from style_transfer import _hip as hip
    net = hip.Net(T._weights(), pooling, DEV, precision)
    return net, hip.Plan(net, *size)


def _plan_levels(plan):
    """The plan's own levels as (m = s^2 in float64, M): what its kernels weigh with."""
    out = []
    for k in range(5):
        s, total = plan.style_mask_level(k)
        out.append((s.cpu().double() ** 2, total))
    return out


# ---- 1. the pyramid ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [SIZE, ODD], ids=lambda s: f'{s[0]}x{s[1]}')
def test_pyramid(size):
    """level^2 against the avg_pool2d chain of the fp32 mask: max abs error <= 2e-6 (values <= 1; at most four levels of
    three roundings each plus a square root and a square, each <= 2^-24 relative: < 1e-6, doubled).  Sums within 1e-6
    relative of the float64 sums of the returned levels.  Two calls give equal bits."""
    _, plan = _net_plan(size)
    mask = ramp_mask(*size)
    want = pyramid(mask)
    plan.set_style_mask(mask.to(DEV))
    first = [plan.style_mask_level(k) for k in range(5)]
    plan.set_style_mask(mask.to(DEV))
    second = [plan.style_mask_level(k) for k in range(5)]
    torch.cuda.synchronize()
    for k in range(5):
        s, total = first[k]
        assert tuple(s.shape) == tuple(want[k].shape) == (size[0] >> k, size[1] >> k)
        err = float((s.cpu() ** 2 - want[k]).abs().max())
        own = float((s.cpu().double() ** 2).sum())
        rel = abs(total - own) / own
        print(f'[mask] pyramid {size} level {k} {tuple(s.shape)}: max abs {err:.2e} (bar 2e-6)  sum {total:.9g} own {own:.9g} '
              f'rel {rel:.2e} (bar 1e-6)')
        assert err <= 2e-6 and rel <= 1e-6
        assert torch.equal(s, second[k][0]) and total == second[k][1]
    if size == SIZE:        # the issue's table for the ramp at 40 x 48
        for k, want_sum in enumerate([720, 180, 45, 11.25, 2.096]):
            assert abs(first[k][1] - want_sum) <= 1e-3 * want_sum, (k, first[k][1])


# ---- 2. masked moments against float64 on the plan's own tap ----------------------------------------------------------------
MOMENT_LAYERS = [1, 4, 6, 11, 20, 29]
VARIANTS = [('fp32', 1), ('fp16x3', 1), ('fp16x3', 2)]      # the three pass-1 kernels (wide = 2: the 128-tile one at small shapes)


def _own_moments(plan, layer, levels):
    f = plan.feature(layer)[0].cpu().double().flatten(1)
    m, total = levels[LEVEL[layer]]
    fm = f * m.flatten()
    return fm.sum(1) / total, fm @ f.t() / total


@pytest.mark.parametrize('precision, wide', VARIANTS, ids=lambda v: str(v))
@pytest.mark.parametrize('size', [SIZE, (135, 181)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_masked_moments(size, precision, wide):
    from style_transfer import _hip as hip
    _, plan = _net_plan(size, precision)
    g = torch.Generator().manual_seed(size[0] * 3 + size[1])
    img = torch.rand((1, 3, *size), generator=g).to(DEV)
    plan.forward(img, 29)
    with hip.options(ST_GRAM_WIDE=wide):
        plain = {layer: plan.moments(layer) for layer in MOMENT_LAYERS}
        for name, make in MASKS.items():
            plan.set_style_mask(make(*size).to(DEV))
            levels = _plan_levels(plan)
            for layer in MOMENT_LAYERS:          # (layer 1 on the default lists: the position conv1_1's fused Gram serves)
                mean, srm = plan.moments(layer)
                want_mean, want_srm = _own_moments(plan, layer, levels)
                tag = f'{name} features[{layer}] {size[0]}x{size[1]} {precision} wide={wide}'
                KG._report(f'masked srm {tag}', srm, want_srm.float(), 1e-6)
                KG._report(f'masked mean {tag}', mean, want_mean.float(), 1e-6)
                assert torch.equal(srm, srm.t()), 'the masked second raw moment must be exactly symmetric'
                assert rel_l2(srm.cpu(), plain[layer][1].cpu()) > 1e-3, 'the mask was ignored'
        plan.set_style_mask(torch.ones(size).to(DEV))
        for layer in MOMENT_LAYERS:
            mean, srm = plan.moments(layer)
            KG._report(f'all-ones srm features[{layer}]', srm, plain[layer][1].cpu(), 1e-6)
            KG._report(f'all-ones mean features[{layer}]', mean, plain[layer][0].cpu(), 1e-6)
        plan.set_style_mask(None)
        for layer in MOMENT_LAYERS:
            assert T._same(plan.moments(layer), plain[layer]), 'a cleared mask must leave the plain moments, bit for bit'


def test_fused_gram_of_conv1_1_never_serves_a_masked_relu1_1():
    """ST_CONV1_GRAM_IN_FORWARD=1: st_plan_forward leaves relu1_1's plain partial sums in conv1_1's launch.  Neither a mask
    set before that forward nor one set after it may be answered from them."""
    from style_transfer import _hip as hip
    _, plan = _net_plan(SIZE)
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    mask = ramp_mask(*SIZE).to(DEV)
    plan.forward(img, 29)
    plan.moments(1)                              # (the head's workspace exists from here on: the fused launch can apply)
    with hip.options(ST_CONV1_GRAM_IN_FORWARD=1):
        for mask_first in (True, False):
            plan.set_style_mask(None)
            if mask_first:
                plan.set_style_mask(mask)
            plan.forward(img, 29)
            if not mask_first:
                plan.set_style_mask(mask)
            mean, srm = plan.moments(1)
            want_mean, want_srm = _own_moments(plan, 1, _plan_levels(plan))
            KG._report(f'masked srm features[1], mask set {"before" if mask_first else "after"} the forward', srm, want_srm.float(), 1e-6)
            KG._report('masked mean features[1]', mean, want_mean.float(), 1e-6)


# ---- 3. the closure against the oracle --------------------------------------------------------------------------------------
def _masked_moments(feat, m, total):
    mat = feat.reshape(feat.shape[1], -1)
    weighted = mat * m.reshape(-1)
    return weighted.sum(1) / total, weighted @ mat.t() / total


def _w2(mean, srm, target, eps=1e-4):
    """StyleLossW2.forward (:175-181) from the input's (mean, srm)."""
    t_mean, t_cov, t_root = target
    cov = srm - torch.outer(mean, mean) + torch.eye(srm.shape[0], dtype=srm.dtype) * eps
    root = O._NSRoot.apply(t_root @ cov @ t_root)
    return torch.mean((mean - t_mean) ** 2) + torch.diagonal(t_cov + cov - 2 * root).mean()


def _style_term(feat, layer, moments, levels, kind, dtype):
    """The style term of `layer` with the mask `levels` (None: unmasked, all pixels at weight 1)."""
    if levels is None:
        h, w = feat.shape[2:]
        m, total = torch.ones((h, w), dtype=dtype), float(h * w)
    else:
        m, total = levels[LEVEL[layer]][0].to(dtype), levels[LEVEL[layer]][1]
    mean, srm = _masked_moments(feat, m, total)
    t_mean, t_srm = moments[layer]
    if kind == 'gram':
        return K._scaled_mse(srm, t_srm.to(dtype))
    return _w2(mean, srm, O.style_target(t_mean.to(dtype), t_srm.to(dtype)))


def _oracle(image, pooling, decisions, content_layers, style_layers, ctargets, moments, weights, style_kind, levels, dtype):
    """SumLoss with masked style terms in `dtype`: (weighted terms, total, gradient, the UNMASKED weighted style terms)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cws, sws = weights
    img = image.to(dtype).clone().requires_grad_(True)
    feats = O.vgg_features(img, T._weights() if dtype == torch.float32 else T._weights64(), content_layers + style_layers,
                           pooling, decisions)
    terms = [O.content_mse(feats[layer], ctargets[layer].to(dtype)) * cw for layer, cw in zip(content_layers, cws)]
    terms += [_style_term(feats[layer], layer, moments, levels, style_kind, dtype) * sw for layer, sw in zip(style_layers, sws)]
    terms.append(O.tv_loss(img) * T.TV_WEIGHT)
    total = sum(terms)
    (grad,) = torch.autograd.grad(total, img)
    with torch.no_grad():
        plain = [float(_style_term(feats[layer], layer, moments, None, style_kind, dtype) * sw) for layer, sw in zip(style_layers, sws)]
    return [float(t.detach()) for t in terms], float(total.detach()), grad.detach(), plain


def _judge(tag, plan, img, image, pooling, content_layers, style_layers, style_kind):
    """test_loss_kinds_gpu._judge with the masked style terms, the plan's own levels as the mask."""
    deepest = max(content_layers + style_layers)
    plan.forward(img, deepest)
    torch.cuda.synchronize()
    decisions = O.decisions_from_maps({idx: plan.feature(idx).cpu() for idx in T.RELUS if idx <= deepest}, pooling)
    levels = _plan_levels(plan)
    losses, grad = plan.loss_and_grad(img)
    torch.cuda.synchronize()
    terms = plan.term_losses().cpu().double().numpy()
    losses = losses.cpu().numpy()
    weights = T._layer_weights(content_layers, style_layers)
    ctargets, moments = T._targets(tuple(image.shape[2:]), pooling, content_layers, style_layers)
    args = (image, pooling, decisions, content_layers, style_layers, ctargets, moments, weights, style_kind, levels)
    t32, _, g32, _ = _oracle(*args, torch.float32)
    t64, _, g64, plain64 = _oracle(*args, torch.float64)
    names = [f'content[{layer}]' for layer in content_layers] + [f'style[{layer}]' for layer in style_layers] + ['tv']
    failures = []
    assert len(terms) == len(names), (len(terms), names)
    for k, name in enumerate(names):
        floor = abs(t32[k] - t64[k]) / abs(t64[k])
        tol = max(T.TERM_TOL, 3 * floor)
        rel = abs(terms[k] - t32[k]) / abs(t32[k])
        print(f'[mask] {tag} term {name:12s} got {terms[k]:.8g} want {t32[k]:.8g} rel {rel:.2e}  floor {floor:.2e}  '
              f'bar {tol:.1e}  {"PASS" if rel <= tol else "FAIL"}')
        if not rel <= tol:
            failures.append(f'{tag}: term {name} rel {rel:.2e} > {tol:.1e}')
        if name.startswith('style'):
            j = k - len(content_layers)
            moved = abs(t64[k] - plain64[j]) / abs(plain64[j])
            print(f'[mask] {tag} term {name:12s} masked float64 {t64[k]:.8g} unmasked {plain64[j]:.8g}: moved by {moved:.3g} = '
                  f'{moved / tol:.0f} bars')
            assert moved >= 100 * tol, f'{tag}: the mask moves term {name} by {moved / tol:.1f} bars only: it could be ignored'
    want_total = np.float32(0)
    for t in terms.astype(np.float32):
        want_total = np.float32(want_total + t)
    rel_total = abs(float(losses[7]) - float(want_total)) / abs(float(want_total))
    print(f'[mask] {tag} total {losses[7]:.8g} vs fp32 sum of the terms {want_total:.8g} rel {rel_total:.2e} (bar {T.SUM_TOL:.0e})')
    if not rel_total <= T.SUM_TOL:
        failures.append(f'{tag}: total rel {rel_total:.2e} > {T.SUM_TOL:.0e}')
    assert torch.isfinite(grad).all(), f'{tag}: non-finite gradient'
    err, floor = rel_l2(grad.cpu(), g64), rel_l2(g32, g64)
    b = T.bar(floor)
    print(f'[mask] {tag} gradient hip-vs-fp64 {err:.2e}  ref-fp32 floor {floor:.2e}  bar {b:.1e}  {"PASS" if err <= b else "FAIL"}')
    if not err <= b:
        failures.append(f'{tag}: gradient rel-L2 {err:.2e} > {b:.1e} (floor {floor:.2e})')
    return failures


CLOSURES = [
    ('default-w2', T.DEFAULT, 'w2', SIZE, 'max', 'fp16x3'),       # the general closure forced on the default configuration
    ('default-gram', T.DEFAULT, 'gram', SIZE, 'max', 'fp16x3'),
    ('b', T.CONFIGS['b'], 'w2', SIZE, 'max', 'fp16x3'),           # 29 in both lists: the content term adds onto a masked seed
    ('d-average', T.CONFIGS['d'], 'w2', SIZE, 'average', 'fp16x3'),
    ('default-odd', T.DEFAULT, 'w2', ODD, 'max', 'fp16x3'),       # pixel counts 2430, 594, 143, 30, 6
    ('default-fp32', T.DEFAULT, 'w2', SIZE, 'max', 'fp32'),
]


@pytest.mark.parametrize('name, lists, style_kind, size, pooling, precision', CLOSURES, ids=[c[0] for c in CLOSURES])
def test_masked_closure_against_the_oracle(name, lists, style_kind, size, pooling, precision):
    content_layers, style_layers = lists
    image = T._inputs(size, pooling)['image']
    img = image.to(DEV)
    _, plan = K._plan(size, pooling, precision, content_layers, style_layers, ('mse', style_kind))
    plan.set_style_mask(ramp_mask(*size).to(DEV))
    tag = f'({name}) content {content_layers} style {style_layers} {size[0]}x{size[1]}-{pooling}-{precision} {style_kind}, ramp mask'
    failures = _judge(tag, plan, img, image, pooling, content_layers, style_layers, style_kind)
    assert not failures, '; '.join(failures)


# ---- 4. bits ----------------------------------------------------------------------------------------------------------------
def _masked_default_plan():
    _, plan = K._plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=None, configure=False)
    plan.set_style_mask(ramp_mask(*SIZE).to(DEV))
    return plan


def test_two_masked_closures_are_equal_and_step_is_closure_plus_update():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    plan = _masked_default_plan()
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


def test_masked_lbfgs_step_is_closure_plus_update():
    from style_transfer import _hip as hip
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    plan = _masked_default_plan()
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


def test_a_cleared_mask_leaves_the_plan_that_never_had_one_and_the_range_guard_sees_the_mask():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    _, never = K._plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=None, configure=False)
    plan = _masked_default_plan()
    masked = K._leg(plan, img, steps=False)
    # the range guard runs the masked closure, flags nothing on the synthetic network and leaves the closure as it was
    fwd, bwd = plan.range_guard(img)
    assert not any(fwd) and not any(bwd)
    assert T._same(masked, K._leg(plan, img, steps=False))
    plan.set_style_mask(None)
    a, b = K._leg(never, img, steps=True), K._leg(plan, img, steps=True)
    assert len(a) == 10 and T._same(a, b)
    assert not torch.equal(masked[1], a[1])


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals():
    from style_transfer import _hip as hip
    from style_transfer import sharding
    net, plan = _net_plan(ODD)
    strip = sharding.StripPlan(net, 48, 48, 0, 32)
    with pytest.raises(hip.HipLibraryError, match='strip'):
        strip.set_style_mask(torch.ones((32, 48)).to(DEV))
    with pytest.raises(hip.HipLibraryError, match='no style mask'):
        plan.style_mask_level(0)
    with pytest.raises(hip.HipLibraryError, match=r'mask.*level 0'):
        plan.set_style_mask(torch.zeros(ODD).to(DEV))
    last_row = torch.zeros(ODD)
    last_row[44] = 1                              # the row that the 22-row level drops
    with pytest.raises(hip.HipLibraryError, match=r'mask.*level 1'):
        plan.set_style_mask(last_row.to(DEV))
    too_large = ramp_mask(*ODD)
    too_large[7, 9] = 1.5
    with pytest.raises(hip.HipLibraryError, match=r'mask.*\[0, 1\]'):
        plan.set_style_mask(too_large.to(DEV))
    with_nan = ramp_mask(*ODD)
    with_nan[30, 2] = float('nan')
    with pytest.raises(hip.HipLibraryError, match=r'mask.*NaN'):
        plan.set_style_mask(with_nan.to(DEV))
    with pytest.raises(hip.HipLibraryError, match='no style mask'):       # a refused mask leaves the plan without one
        plan.style_mask_level(0)
    with pytest.raises(ValueError, match='45 x 54'):
        plan.set_style_mask(torch.ones(SIZE).to(DEV))
    plan.set_style_mask(ramp_mask(*ODD).to(DEV))
    assert plan.style_mask_level(4)[0].shape == (2, 3)
    with pytest.raises(hip.HipLibraryError, match='level'):
        plan.style_mask_level(5)


# ---- 6. stylize() -----------------------------------------------------------------------------------------------------------
def _pil_mask(mask):
    from PIL import Image
    return Image.fromarray(np.uint8(np.round(mask.numpy() * 255)), 'L')


def _sized_levels(pil_mask, w, h):
    """The mask as stylize() brings it to w x h, and its pyramid, as (m float64, M)."""
    from PIL import Image
    m0 = torch.from_numpy(np.asarray(pil_mask.convert('L').resize((w, h), Image.BILINEAR), dtype=np.float32) / np.float32(255))
    return [(level.double(), float(level.double().sum())) for level in pyramid(m0)]


@pytest.mark.parametrize('optimizer', ['adam', 'lbfgs'])
def test_stylize_reads_the_mask_attributes(optimizer):
    from PIL import Image
    from style_transfer import StyleTransfer
    from style_transfer.style_transfer import size_to_fit, to_tensor
    st = StyleTransfer(devices=[DEV], pooling='max', weights='synthetic')
    assert st.style_mask is None and st.style_image_masks is None
    content_image, style_image = T._pil(81, 64, 48), T._pil(82, 60, 44)
    st.style_mask = _pil_mask(ramp_mask(48, 64))
    st.style_image_masks = [_pil_mask(binary_mask(44, 60))]
    decay = 0.99
    seen = []

    def callback(it):
        if it.i == 1:
            # (the scale's starting image from the EMA and st.image: test_taps_gpu.test_stylize_reads_the_layer_attributes)
            avg, x1 = st.get_image_tensor(), st.image.detach()[0]
            seen.append((it.w, it.h, it.loss, (((1 + decay) * avg - x1) / decay).cpu()[None]))

    out = st.stylize(content_image, [style_image], end_scale=64, min_scale=45, initial_iterations=6, iterations=4,
                     optimizer=optimizer, avg_decay=decay, callback=callback)
    assert out is not None and torch.isfinite(st.get_image_tensor()).all() and len(seen) == 2
    cws, sws = [0.015], st.style_weights
    for (w, h, loss, start), scale in zip(seen, (45, 64)):
        assert (w, h) == size_to_fit(content_image.size, scale, scale_up=True)
        content = to_tensor(content_image.resize((w, h), Image.BICUBIC))[None]
        sw_, sh_ = size_to_fit(style_image.size, scale)
        style = to_tensor(style_image.resize((sw_, sh_), Image.BICUBIC))[None]
        out_levels = _sized_levels(st.style_mask, w, h)
        img_levels = _sized_levels(st.style_image_masks[0], sw_, sh_)
        with torch.no_grad():
            cfeats = O.vgg_features(content, T._weights(), st.content_layers, 'max')
            sfeats = O.vgg_features(style, T._weights(), st.style_layers, 'max')
            # the image mask on the target's moments ...
            moments = {layer: _masked_moments(sfeats[layer], img_levels[LEVEL[layer]][0].float(), img_levels[LEVEL[layer]][1])
                       for layer in st.style_layers}
        # ... and the output mask on the iterate's
        args = (start, 'max', None, st.content_layers, st.style_layers, cfeats, moments, (cws, sws), 'w2', out_levels)
        _, total32, _, _ = _oracle(*args, torch.float32)
        _, total64, _, _ = _oracle(*args, torch.float64)
        floor = abs(total32 - total64) / abs(total64)
        tol, rel = max(T.TERM_TOL, 3 * floor), abs(loss - total32) / abs(total32)
        print(f'[mask] stylize {optimizer} {w}x{h}: first loss {loss:.8g} oracle {total32:.8g} rel {rel:.2e} floor {floor:.2e} '
              f'bar {tol:.1e}')
        assert rel <= tol, f'{optimizer} {w}x{h}: first loss rel {rel:.2e} > {tol:.1e}'
    st.style_image_masks = [None, None]
    with pytest.raises(ValueError, match='style_image_masks'):
        st.stylize(content_image, [style_image], end_scale=64, min_scale=45, initial_iterations=1, iterations=1)

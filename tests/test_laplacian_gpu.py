"""The Laplacian loss on pooled images (st_plan_set_laplacian, st_op_laplacian_*, losses.LaplacianLoss,
StyleTransfer.laplacian_weight / laplacian_pools) on a real MI355X.

The reference has none; the yardstick is include/st_amd.h's formula as tests/test_laplacian_cpu.py writes it out in torch
(`pooled_laplacian`, `formula_terms`), with autograd for the gradient - never losses.LaplacianLoss, which is code under test.
Per pool size p: term_p = weight mean((L(Q_p(x)) - L(Q_p(c))) ** 2), Q_p = avg_pool2d(., p), L the 4-neighbour Laplacian on the
replicate-padded map.  Bars:
  the kernels alone (st_op_*): value (relative) and gradient (rel-L2) against float64 <= max(2e-6, 3 x the fp32 torch formula's
      own deviation from float64 on that input) - 2e-6 is test_kernels_gpu's bar for the TV kernels, 3 x the project's margin;
  in the closure, with test_taps_gpu's inputs, targets, weights and bars: each term within max(1e-4, 3 x floor) of the fp32
      oracle, the total within 1e-6 of the fp32 sum of the terms, the gradient within T.bar(floor) of float64.
The oracle is test_content_tv_masks_gpu._oracle's construction with the Laplacian terms added.  The Laplacian's content image
is test_taps_gpu's content image (_smooth(71)); the iterate is its image (_smooth(73)).

LAP_WEIGHT = 10: on the CPU oracle at 40 x 48 and 45 x 54 the float64 gradient with the term differs from the one without by
0.73 (pools (4,)) to 0.98 (pools (4, 16)) in rel-L2, i.e. >= 146 bars even at the bar's ceiling of 5e-3 - a Laplacian that is
ignored cannot pass; every closure case asserts >= 100 bars and prints the factor.
"""
import numpy as np
import pytest
import torch

from conftest import rel_l2
import st_oracle as O
import test_content_tv_masks_gpu as CM
import test_loss_kinds_gpu as K
import test_style_mask_gpu as MG
import test_taps_gpu as T
from test_laplacian_cpu import formula_terms, pooled_laplacian

pytestmark = pytest.mark.gpu
DEV = T.DEV
SIZE = MG.SIZE       # 40 x 48: W % 4 == 0 - the 16-byte paths; p = 16 leaves 2 x 3
ODD = MG.ODD         # 45 x 54: the scalar paths; p = 4 drops row 44 and columns 52, 53; p = 16 leaves 2 x 3
LAP_WEIGHT = 10.0
KERNEL_FLOOR = 2e-6


def _content(size):
    return T._smooth(71, *size)


def _f32(values):
    """fp32(((v0 + v1) + v2) + ...), the additions in list order."""
    total = np.float32(values[0])
    for v in values[1:]:
        total = np.float32(total + np.float32(v))
    return total


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------------
KERNEL_CASES = [((9, 13), 4)] + [(SIZE, p) for p in (1, 4, 16)] + [(ODD, p) for p in (1, 2, 4)]


def _formula_value_and_grad(x, content, pool, dtype):
    xi = x.to(dtype).clone().requires_grad_(True)
    value = formula_terms(xi, content.to(dtype), (pool,))[0]
    (grad,) = torch.autograd.grad(value, xi)
    return float(value.detach()), grad.detach(), pooled_laplacian(content.to(dtype), pool)


def _kernel_bars(x, content, pool):
    """(float64 value, gradient, target; the value's, the gradient's and the target's bar): max(2e-6, 3 x the fp32 formula's own
    deviation from float64)."""
    v32, g32, t32 = _formula_value_and_grad(x, content, pool, torch.float32)
    v64, g64, t64 = _formula_value_and_grad(x, content, pool, torch.float64)
    floors = abs(v32 - v64) / abs(v64), rel_l2(g32, g64), rel_l2(t32, t64)
    return v64, g64, t64, floors, tuple(max(KERNEL_FLOOR, 3 * f) for f in floors)


@pytest.mark.parametrize('channels', [1, 3], ids=['C1', 'C3'])
@pytest.mark.parametrize('size, pool', KERNEL_CASES, ids=[f'{s[0]}x{s[1]}-p{p}' for s, p in KERNEL_CASES])
def test_kernels_alone(size, pool, channels):
    from style_transfer import _hip as hip
    x, content = T._smooth(73, *size)[0, :channels].contiguous(), _content(size)[0, :channels].contiguous()
    v64, g64, t64, floors, bars = _kernel_bars(x, content, pool)
    xd, cd = x.to(DEV), content.to(DEV)
    target = hip.op_laplacian_target(cd, pool)
    value, residual = hip.op_laplacian_value(xd, target, pool)
    upstream = torch.tensor(1.0, device=DEV)
    grad = hip.op_laplacian_backward(residual, xd.shape, pool, upstream)
    half = hip.op_laplacian_backward(residual, xd.shape, pool, 0.5 * upstream)
    again = hip.op_laplacian_value(xd, target, pool)
    own, own_residual = hip.op_laplacian_value(cd, target, pool)
    torch.cuda.synchronize()
    tag = f'[laplacian] kernels {size[0]}x{size[1]} p={pool} C={channels}'
    h, w = size[0] // pool, size[1] // pool
    assert tuple(target.shape) == tuple(residual.shape) == (channels, h, w) and grad.shape == xd.shape
    errs = abs(float(value) - v64) / abs(v64), rel_l2(grad.cpu(), g64), rel_l2(target.cpu(), t64)
    for what, err, floor, b in zip(('value', 'gradient', 'target'), errs, floors, bars):
        print(f'{tag}: {what} hip-vs-fp64 {err:.2e}  fp32 formula floor {floor:.2e}  bar {b:.1e}  {"PASS" if err <= b else "FAIL"}')
    assert torch.isfinite(grad).all()
    assert all(err <= b for err, b in zip(errs, bars)), (errs, bars)
    # the dropped trailing rows and columns get exactly nothing; everything else something
    assert torch.count_nonzero(grad[:, h * pool:, :]) == 0 and torch.count_nonzero(grad[:, :, w * pool:]) == 0
    assert rel_l2(half.cpu(), 0.5 * grad.cpu()) <= 1e-6, 'the upstream scalar multiplies the gradient'
    assert torch.equal(again[0], value) and torch.equal(again[1], residual), 'two calls give equal bits'
    assert float(own) == 0.0 and torch.count_nonzero(own_residual) == 0, 'the content image against its own target is exactly 0'


# ---- 2. the plan's targets --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size, pools', [(SIZE, (1, 4, 16)), (ODD, (4, 2, 1, 16))], ids=['40x48', '45x54'])
def test_targets(size, pools):
    from style_transfer import _hip as hip
    _, plan = MG._net_plan(size)
    content = _content(size)
    plan.set_laplacian(content.to(DEV), pools, LAP_WEIGHT)
    for k, p in enumerate(pools):
        got = plan.laplacian_target(k)
        alone = hip.op_laplacian_target(content[0].to(DEV), p)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (3, size[0] // p, size[1] // p)
        assert torch.equal(got, alone), f'pool size {p}: the plan and the standalone entry run the same kernels'
        _, _, t64, floors, bars = _kernel_bars(T._smooth(73, *size)[0], content[0], p)
        err = rel_l2(got.cpu(), t64)
        print(f'[laplacian] target {size[0]}x{size[1]} p={p}: hip-vs-fp64 {err:.2e}  fp32 formula floor {floors[2]:.2e}  bar {bars[2]:.1e}')
        assert err <= bars[2]
    with pytest.raises(hip.HipLibraryError, match='st_plan_laplacian.*out of range'):
        plan.laplacian_target(len(pools))


# ---- 3. the closure ---------------------------------------------------------------------------------------------------------
def _oracle(image, content, pooling, decisions, content_layers, style_layers, ctargets, moments, weights, kinds, clevels, tvmap,
            slevels, pools, dtype):
    """test_content_tv_masks_gpu._oracle's construction in `dtype` with the Laplacian terms added: (content and style terms,
    tv, [term_p], total, gradient, gradient WITHOUT the Laplacian terms)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cws, sws = weights
    img = image.to(dtype).clone().requires_grad_(True)
    taps = content_layers + style_layers
    feats = O.vgg_features(img, T._weights() if dtype == torch.float32 else T._weights64(), taps, pooling, decisions)
    terms = []
    for layer, cw in zip(content_layers, cws):
        wmap = None if clevels is None else clevels[MG.LEVEL[layer]].to(dtype)
        terms.append(CM.weighted_content(feats[layer], ctargets[layer].to(dtype), wmap, kinds[0], 1e-8) * cw)
    terms += [MG._style_term(feats[layer], layer, moments, slevels, kinds[1], dtype) * sw for layer, sw in zip(style_layers, sws)]
    tv = (O.tv_loss(img) if tvmap is None else CM.weighted_tv(img, tvmap.to(dtype))) * T.TV_WEIGHT
    laps = [term * LAP_WEIGHT for term in formula_terms(img, content.to(dtype), pools)]
    plain = sum(terms) + tv
    total = plain + sum(laps)
    (grad_plain,) = torch.autograd.grad(plain, img, retain_graph=True)
    (grad,) = torch.autograd.grad(total, img)
    return ([float(t.detach()) for t in terms], float(tv.detach()), [float(t.detach()) for t in laps], float(total.detach()),
            grad.detach(), grad_plain.detach())


def _judge(tag, plan, img, image, size, pooling, content_layers, style_layers, kinds, pools, closure=None):
    """One closure of `plan` - which has NO Laplacian yet - without and one with the Laplacian, the latter against the oracle
    under the plan's own maps.  Returns the failures.  `closure`: the judged closure as a callable returning (losses, gradient)
    (tests/test_caller_buffers_gpu.py runs it on buffers of its own); default plan.loss_and_grad(img)."""
    from style_transfer import _hip as hip
    deepest = max(content_layers + style_layers)
    plan.forward(img, deepest)
    torch.cuda.synchronize()
    decisions = O.decisions_from_maps({idx: plan.feature(idx).cpu() for idx in T.RELUS if idx <= deepest}, pooling)

    def held(read):
        try:
            return read()
        except hip.HipLibraryError:
            return None
    clevels = held(lambda: CM._content_levels(plan))
    tvmap = held(lambda: plan.tv_mask().cpu().double())
    slevels = held(lambda: MG._plan_levels(plan))
    plan.loss_and_grad(img)
    tv_alone = plan.term_losses()[-1].clone()
    content = _content(size)
    plan.set_laplacian(content.to(DEV), pools, LAP_WEIGHT)
    losses, grad = closure() if closure is not None else plan.loss_and_grad(img)
    torch.cuda.synchronize()
    terms = plan.term_losses().cpu().double().numpy()
    lterms = plan.laplacian_terms().cpu().numpy()
    losses = losses.cpu().numpy()
    weights = T._layer_weights(content_layers, style_layers)
    ctargets, moments = T._targets(size, pooling, content_layers, style_layers)
    args = (image, content, pooling, decisions, content_layers, style_layers, ctargets, moments, weights, kinds, clevels, tvmap,
            slevels, pools)
    t32, tv32, l32, _, g32, _ = _oracle(*args, torch.float32)
    t64, tv64, l64, _, g64, plain64 = _oracle(*args, torch.float64)
    names = [f'content[{layer}]' for layer in content_layers] + [f'style[{layer}]' for layer in style_layers]
    want32 = dict(zip(names, t32), **{'image-space': tv32 + sum(l32)})
    want64 = dict(zip(names, t64), **{'image-space': tv64 + sum(l64)})
    got = dict(zip(names + ['image-space'], terms))
    assert len(terms) == len(names) + 1 and len(lterms) == 1 + len(pools)
    for k, name in enumerate(['tv alone'] + [f'laplacian p={p}' for p in pools]):
        want32[name], want64[name], got[name] = ([tv32] + l32)[k], ([tv64] + l64)[k], float(lterms[k])
    failures = []
    for name in got:
        floor = abs(want32[name] - want64[name]) / abs(want64[name])
        tol = max(T.TERM_TOL, 3 * floor)
        rel = abs(got[name] - want32[name]) / abs(want32[name])
        print(f'[laplacian] {tag} term {name:16s} got {got[name]:.8g} want {want32[name]:.8g} rel {rel:.2e}  floor {floor:.2e}  '
              f'bar {tol:.1e}  {"PASS" if rel <= tol else "FAIL"}')
        if not rel <= tol:
            failures.append(f'{tag}: term {name} rel {rel:.2e} > {tol:.1e}')
    # the accounting, bit for bit
    assert np.float32(lterms[0]) == np.float32(tv_alone.cpu().numpy()), 'laplacian_terms()[0] is the TV term of the plan without a Laplacian'
    slot = _f32(list(lterms))
    assert np.float32(terms[-1]) == slot and losses[6] == slot, (terms[-1], losses[6], slot)
    want_total = _f32([np.float32(0)] + list(terms.astype(np.float32)))
    rel_total = abs(float(losses[7]) - float(want_total)) / abs(float(want_total))
    print(f'[laplacian] {tag} total {losses[7]:.8g} vs fp32 sum of the terms {want_total:.8g} rel {rel_total:.2e} (bar {T.SUM_TOL:.0e})')
    if not rel_total <= T.SUM_TOL:
        failures.append(f'{tag}: total rel {rel_total:.2e} > {T.SUM_TOL:.0e}')
    assert torch.isfinite(grad).all(), f'{tag}: non-finite gradient'
    err, floor = rel_l2(grad.cpu(), g64), rel_l2(g32, g64)
    b = T.bar(floor)
    print(f'[laplacian] {tag} gradient hip-vs-fp64 {err:.2e}  ref-fp32 floor {floor:.2e}  bar {b:.1e}  {"PASS" if err <= b else "FAIL"}')
    if not err <= b:
        failures.append(f'{tag}: gradient rel-L2 {err:.2e} > {b:.1e} (floor {floor:.2e})')
    moved = rel_l2(plain64, g64)
    print(f'[laplacian] {tag} float64 gradient without the Laplacian is {moved:.3g} from the one with it = {moved / b:.0f} gradient bars')
    assert moved >= 100 * b, f'{tag}: the Laplacian moves the gradient by {moved / b:.1f} bars only: it could be ignored'
    return failures


DEFAULT_CASES = [(size, pools, precision) for size in (SIZE, ODD) for pools in ((4,), (4, 16)) for precision in ('fp16x3', 'fp32')]


@pytest.mark.parametrize('size, pools, precision', DEFAULT_CASES,
                         ids=[f'{s[0]}x{s[1]}-p{"-".join(map(str, p))}-{prec}' for s, p, prec in DEFAULT_CASES])
def test_closure_on_the_default_layers(size, pools, precision):
    image = T._inputs(size, 'max')['image']
    _, plan = K._plan(size, 'max', precision, *T.DEFAULT, kinds=None, configure=False)
    tag = f'default layers {size[0]}x{size[1]}-{precision} pools {pools}'
    failures = _judge(tag, plan, image.to(DEV), image, size, 'max', *T.DEFAULT, ('mse', 'w2'), pools)
    assert not failures, '; '.join(failures)


def test_closure_on_other_layers_with_gram_heads():
    content_layers, style_layers = CM.CONTENT_LISTS['c4-13']
    image = T._inputs(SIZE, 'max')['image']
    _, plan = K._plan(SIZE, 'max', 'fp16x3', content_layers, style_layers, ('mse', 'gram'))
    tag = f'content {content_layers} style {style_layers} gram {SIZE[0]}x{SIZE[1]}-fp16x3 pools (4, 16)'
    failures = _judge(tag, plan, image.to(DEV), image, SIZE, 'max', content_layers, style_layers, ('mse', 'gram'), (4, 16))
    assert not failures, '; '.join(failures)


def test_closure_with_a_style_mask_a_content_map_and_a_tv_map():
    image = T._inputs(SIZE, 'max')['image']
    _, plan = K._plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=None, configure=False)
    CM._three_maps(plan)
    tag = f'default layers {SIZE[0]}x{SIZE[1]}-fp16x3 pools (4,), style mask + content map + TV map'
    failures = _judge(tag, plan, image.to(DEV), image, SIZE, 'max', *T.DEFAULT, ('mse', 'w2'), (4,))
    assert not failures, '; '.join(failures)


# ---- 4. exactness and bits --------------------------------------------------------------------------------------------------
def _default_plan():
    return K._plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=None, configure=False)[1]


def test_the_content_image_itself_has_terms_of_exactly_zero():
    from style_transfer import _hip as hip
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    plan = _default_plan()
    with hip.options(ST_GENERAL_TAPS=1):          # the closure a Laplacian sends the default configuration to
        plain = K._leg(plan, img, steps=False)
    plan.set_laplacian(img, (1, 4, 16), LAP_WEIGHT)
    with_it = K._leg(plan, img, steps=False)
    lterms = plan.laplacian_terms().cpu().numpy()
    assert len(lterms) == 4 and all(float(t) == 0.0 for t in lterms[1:]), lterms
    assert lterms[0] == plain[0][6].item()
    assert T._same(plain, with_it), 'a residual of exactly 0 adds nothing to the losses, the terms or the gradient'


def test_two_closures_give_equal_bits_and_set_then_clear_leaves_the_fast_path():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    never, plan = _default_plan(), _default_plan()
    plan.set_laplacian(_content(SIZE).to(DEV), (4, 16), LAP_WEIGHT)
    first, second = K._leg(plan, img, steps=False), K._leg(plan, img, steps=False)
    assert T._same(first, second), 'two closures on the same inputs must give the same bits'
    lterms = plan.laplacian_terms().clone()
    K._leg(plan, img, steps=False)
    assert torch.equal(lterms, plan.laplacian_terms())
    plan.set_laplacian(None)
    a, b = K._leg(never, img, steps=True), K._leg(plan, img, steps=True)
    assert len(a) == 10 and T._same(a, b), "a cleared Laplacian must leave a fresh plan's default closure, bit for bit"
    assert not torch.equal(first[1], a[1]) and not torch.equal(first[0], a[0])


# ---- 5. steps ---------------------------------------------------------------------------------------------------------------
def _tail_total(losses):
    return _f32([np.float32(0)] + [losses[k] for k in range(7)])


def test_adam_step_lbfgs_step_and_range_guard_on_a_laplacian_plan():
    from style_transfer import _hip as hip
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    plan, plain = _default_plan(), _default_plan()
    plan.set_laplacian(_content(SIZE).to(DEV), (4, 16), LAP_WEIGHT)
    before = K._leg(plan, img, steps=False)
    fwd, bwd = plan.range_guard(img)
    assert len(fwd) == 13 and len(bwd) == 13 and not any(fwd) and not any(bwd)
    assert T._same(before, K._leg(plan, img, steps=False)), 'the range guard must leave the closure as it was'
    # one native Adam step (the folded tail): the reported terms are loss_and_grad's on the same image, the result closure + update
    xa, ma, va, ea = T._state(img)
    xb, mb, vb, eb = T._state(img)
    la = plan.step(xa, ma, va, ea, 1, 0.02).clone()
    lb, g = plan.loss_and_grad(xb)
    lb = lb.clone()
    plan.apply_update(xb, g, mb, vb, eb, 1, 0.02)
    xc = T._state(img)
    lc = plain.step(*xc, 1, 0.02).clone()
    torch.cuda.synchronize()
    assert la.cpu().numpy()[7] == _tail_total(la.cpu().numpy()), 'losses[7] is 0 + l[0] + ... + l[6]'
    assert torch.equal(la, lb) and torch.equal(la, before[0]), (la, lb, before[0])
    assert torch.equal(xa, xb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(ea, eb)
    assert not torch.equal(xa, img) and not torch.equal(xa, xc[0]) and not torch.equal(la, lc)
    # one native L-BFGS step
    xa, _, _, ea = T._state(img)
    xb, _, _, eb = T._state(img)
    opt_a, opt_b = hip.LBFGS(xa), hip.LBFGS(xb)
    la = opt_a.step(plan, xa, ea, 0.99).clone()
    lb, g = plan.loss_and_grad(xb)
    lb = lb.clone()
    opt_b.update(xb, g, eb, 0.99)
    torch.cuda.synchronize()
    assert la.cpu().numpy()[7] == _tail_total(la.cpu().numpy())
    assert torch.equal(la, lb) and torch.equal(la, before[0])
    assert torch.equal(xa, xb) and torch.equal(ea, eb) and opt_a.info() == opt_b.info()
    assert not torch.equal(xa, img)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals():
    from style_transfer import _hip as hip
    from style_transfer import sharding
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    content = _content(SIZE).to(DEV)
    net, plan = K._plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=None, configure=False)
    plain = K._leg(plan, img, steps=False)
    strip = sharding.StripPlan(net, 48, 48, 0, 32)
    with pytest.raises(hip.HipLibraryError, match='st_plan_set_laplacian.*strip'):
        strip.set_laplacian(torch.rand((3, strip.height, strip.width)).to(DEV), (4,), 1.0)

    def none_set():
        with pytest.raises(hip.HipLibraryError, match='st_plan_laplacian: no Laplacian'):
            plan.laplacian_target(0)
        with pytest.raises(hip.HipLibraryError, match='st_plan_laplacian_terms: no Laplacian'):
            plan.laplacian_terms()
        assert T._same(plain, K._leg(plan, img, steps=False)), 'after a refused call the plan runs as one without a Laplacian'
    none_set()
    refused = [((), 1.0, 'pool sizes'), ((1, 2, 3, 4, 5), 1.0, 'pool sizes'), ((4, 2, 4), 1.0, 'repeated'), ((4, 0), 1.0, 'not positive'),
               ((-3,), 1.0, 'not positive'), ((21,), 1.0, '2 x 2'), ((4, 25), 1.0, '2 x 2'), ((4,), 0.0, 'weight'), ((4,), -1.0, 'weight'),
               ((4,), float('nan'), 'weight'), ((4,), float('inf'), 'weight')]
    for armed in (False, True):
        for pools, weight, pattern in refused:
            if armed:                   # ... and a refused call on a plan that HAS a Laplacian leaves it without one
                plan.set_laplacian(content, (4,), LAP_WEIGHT)
                assert not torch.equal(K._leg(plan, img, steps=False)[1], plain[1])
            with pytest.raises(hip.HipLibraryError, match=f'st_plan_set_laplacian.*{pattern}'):
                plan.set_laplacian(content, pools, weight)
            none_set()
    with pytest.raises(ValueError, match='40 x 48'):
        plan.set_laplacian(_content(ODD).to(DEV), (4,), 1.0)
    plan.set_laplacian(content, (20,), 1.0)        # 40 // 20 = 2, 48 // 20 = 2: the smallest map there is
    assert tuple(plan.laplacian_target(0).shape) == (3, 2, 2)


# ---- 7. the module ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size, pools, batch', [(SIZE, (4, 16), True), (ODD, (1, 4), False)], ids=['40x48-p4-16', '45x54-p1-4'])
def test_module_takes_the_native_path(size, pools, batch):
    from style_transfer import losses
    x, content = T._smooth(73, *size), _content(size)
    if not batch:
        x, content = x[0], content[0]
    module = losses.LaplacianLoss(content.to(DEV), pools)
    reference = losses.LaplacianLoss(content.double(), pools)
    x64 = x.double().requires_grad_(True)
    want = reference(x64)
    (g64,) = torch.autograd.grad(want, x64)
    want = want.detach()
    x32 = x.clone().requires_grad_(True)
    (g32,) = torch.autograd.grad(losses.LaplacianLoss(content, pools)(x32), x32)
    gbar = max(KERNEL_FLOOR, 3 * rel_l2(g32, g64))
    vbar = max(KERNEL_FLOOR, 3 * abs(float(losses.LaplacianLoss(content, pools)(x)) - float(want)) / float(want))
    xd = x.to(DEV).requires_grad_(True)
    before = losses.native_calls.get('laplacian', 0)
    value = module(xd)
    assert losses.native_calls.get('laplacian', 0) == before + 1, 'a dense fp32 HIP image takes the native path'
    (3 * value).backward()
    torch.cuda.synchronize()
    value = value.detach()
    verr, gerr = abs(float(value) - float(want)) / float(want), rel_l2(xd.grad.cpu() / 3, g64)
    print(f'[laplacian] module {size[0]}x{size[1]} pools {pools}: value hip-vs-fp64 {verr:.2e} (bar {vbar:.1e}), gradient {gerr:.2e} '
          f'(bar {gbar:.1e})')
    assert value.shape == () and xd.grad.shape == xd.shape and verr <= vbar and gerr <= gbar
    assert float(module(content.to(DEV))) == 0.0
    with losses.native(False):
        xt = x.to(DEV).requires_grad_(True)
        torch_value = module(xt)
        assert losses.native_calls.get('laplacian', 0) == before + 2
        assert torch.equal(torch_value, module._forward_torch(xt))
        torch_value.backward()
    assert abs(float(torch_value.detach()) - float(value)) <= 1e-5 * float(value) and rel_l2(xt.grad.cpu(), xd.grad.cpu() / 3) <= 1e-5
    # create_graph=True: the torch code's gradient, as a graph
    xg = x.to(DEV).requires_grad_(True)
    (g,) = torch.autograd.grad(module(xg), xg, create_graph=True)
    assert g.requires_grad and rel_l2(g.detach().cpu(), g64) <= 1e-5
    assert not losses.eligible(x.to(DEV).double(), 'laplacian') and not losses.eligible(x, 'laplacian')


# ---- 8. stylize() -----------------------------------------------------------------------------------------------------------
def _stylize(st, content_image, style_image, sizes=None):
    out = st.stylize(content_image, [style_image], end_scale=64, min_scale=45, initial_iterations=3, iterations=2,
                     callback=None if sizes is None else (lambda it: sizes.append((it.h, it.w)) if it.i == 1 else None))
    assert out is not None
    image = st.get_image_tensor().clone()
    assert torch.isfinite(image).all()
    return image


def test_stylize_reads_the_laplacian_attributes(monkeypatch):
    from style_transfer import StyleTransfer
    from style_transfer import _hip as hip
    from style_transfer.style_transfer import size_to_fit, to_tensor
    from PIL import Image
    content_image, style_image = T._pil(81, 64, 48), T._pil(82, 60, 44)
    untouched = StyleTransfer(devices=[DEV], pooling='max', weights='synthetic')
    assert untouched.laplacian_weight == 0. and untouched.laplacian_pools == (4,)
    calls = []
    original = hip.Plan.set_laplacian

    def wrapped(self, content, pools=(4,), weight=1.0):
        calls.append((self, None if content is None else content.detach().cpu().clone(), tuple(pools), weight))
        return original(self, content, pools, weight)
    monkeypatch.setattr(hip.Plan, 'set_laplacian', wrapped)
    plain = _stylize(untouched, content_image, style_image)
    assert not calls, 'without a weight the setter is not called'
    st = StyleTransfer(devices=[DEV], pooling='max', weights='synthetic')
    st.laplacian_weight, st.laplacian_pools = 0., (4, 8)
    zero = _stylize(st, content_image, style_image)
    assert not calls and torch.equal(zero, plain), 'weight 0 is the run of a StyleTransfer whose attributes were never touched'
    st.laplacian_weight = 5.0
    sizes = []
    with_it = _stylize(st, content_image, style_image, sizes)
    want = [size_to_fit(content_image.size, scale, scale_up=True)[::-1] for scale in (45, 64)]
    assert sizes == want
    # once per scale, on the iterate's plan, with that scale's content image
    assert len(calls) == 2 and len({id(plan) for plan, *_ in calls}) == 2 and st._plan is calls[-1][0]
    for (plan, content, pools, weight), (h, w) in zip(calls, want):
        assert (plan.height, plan.width) == (h, w) and pools == (4, 8) and weight == 5.0
        assert torch.equal(content, to_tensor(content_image.resize((w, h), Image.BICUBIC))[None])
    assert tuple(st._plan.laplacian_target(1).shape) == (3, want[-1][0] // 8, want[-1][1] // 8)
    assert len(st._plan.laplacian_terms()) == 3
    assert not torch.equal(with_it, plain), 'the term must move the result'

"""The exact per-channel Wasserstein (sorted) option of a W2 style layer (st_plan_set_w2_marginal, the st_op_channel_sort /
st_op_resample_quantiles / st_op_w2_marginal_* entries, StyleTransfer.style_marginal, losses.StyleLossW2Marginal) on a real MI355X.

The sort is judged exactly: its permutation must be torch.sort(x + 0.0, stable=True)'s on the CPU, element for element.  The
resample, the standalone loss and the module are judged against the float64 formula of tests/test_w2_marginal_cpu.py.

Plans: inputs, helpers and bars are tests/test_w2_diagonal_gpu.py's (and through it test_taps_gpu.py's): _smooth images 71
(content), 72 (style), 73 (the iterate), synthetic_vgg19_weights(0), sizes 40 x 48 and 45 x 54 (odd pixel counts; relu5_1 has 6
pixels at the first).  The oracle is composed in float32 and float64 on the plan's own ReLU and pool decisions, with a free stable
sort in each precision; the targets are the sorted rows of the oracle's style features (31 x 48 or 35 x 54 style images, so
n_q != N everywhere; one case uses a 56 x 44 style image), handed to the plan by set_style_quantiles.
Bars, the project's own, unchanged:
  each weighted term  |hip - fp32 oracle| / |fp32 oracle| <= max(T.TERM_TOL, 3 x the fp32 composition's deviation from float64);
  the total           within T.SUM_TOL of the fp32 sum of the terms;
  image gradient      rel-L2 against float64 <= T.bar(floor), floor = the fp32 composition's own rel-L2 from float64.
A flag that is ignored cannot pass: for every flagged layer the float64 diagonal and full W2 terms on the same tap are shown to
differ from the marginal term by at least 10 of that term's bars; the smallest ratio is printed.
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
import test_taps_gpu as T
import test_w2_diagonal_gpu as D
from test_laplacian_cpu import formula_terms
from test_w2_marginal_cpu import marginal_formula, resample_formula

pytestmark = pytest.mark.gpu
DEV = T.DEV
SIZE, ODD = D.SIZE, D.ODD
ALL, DEEP, MSE, W2 = D.ALL, D.DEEP, D.MSE, D.W2
NONE = [False] * 5
IGNORED_BARS = 10


# ---- 1. the sort, exactly ---------------------------------------------------------------------------------------------------
def _sort_shapes():
    from style_transfer import _hip as hip
    k = hip.sort_chunk()
    return [(1, 1), (3, 2), (3, 1000), (3, k - 1), (2, k), (2, k + 1), (3, 3 * k - 5), (2, 5 * k - 3), (513, 37), (64, 1920)]


KINDS = ['signed', 'relu', 'zeros', 'signed zeros', 'sorted', 'reverse', 'eight values']


def _sort_input(kind, c, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((c, n), generator=g)
    if kind == 'relu':
        x = x.clamp(min=0)
    elif kind == 'zeros':
        x = torch.zeros((c, n))
    elif kind == 'signed zeros':
        x = torch.where(torch.rand((c, n), generator=g) < 0.5, torch.tensor(-0.0), torch.tensor(0.0))
    elif kind == 'sorted':
        x = torch.sort(x, dim=1).values
    elif kind == 'reverse':
        x = torch.sort(x, dim=1, descending=True).values
    elif kind == 'eight values':
        x = torch.tensor([-2.5, -1.0, -0.0, 0.0, 0.5, 1.0, 3.0, 7.0])[torch.arange(c * n).reshape(c, n) % 8]
    return x.contiguous()


@pytest.mark.parametrize('index', range(10))
def test_the_sort_is_the_stable_sort_exactly(index):
    from style_transfer import _hip as hip
    c, n = _sort_shapes()[index]
    runs = -(-n // hip.sort_chunk())
    for k, kind in enumerate(KINDS):
        x = _sort_input(kind, c, n, 100 * index + k)
        want = torch.sort(x + 0.0, dim=1, stable=True)
        xd = x.to(DEV)
        values, perm = hip.op_channel_sort(xd)
        values2, perm2 = hip.op_channel_sort(xd)
        only_values, none = hip.op_channel_sort(xd, indices=False)
        none2, only_perm = hip.op_channel_sort(xd, values=False)
        torch.cuda.synchronize()
        assert none is None and none2 is None
        assert torch.equal(perm.cpu(), want.indices), f'{kind} ({c}, {n}), {runs} runs: the permutation differs'
        assert torch.equal(values.cpu(), want.values), f'{kind} ({c}, {n}): the sorted values differ'
        assert not torch.signbit(values).any() or kind not in ('zeros', 'signed zeros')       # x + 0.0: no -0.0 comes back
        assert torch.equal(values, values2) and torch.equal(perm, perm2)
        assert torch.equal(only_values, values) and torch.equal(only_perm, perm)
        if kind == 'zeros':
            assert torch.equal(perm.cpu(), torch.arange(n).expand(c, n))


def test_the_sort_refuses_what_its_grid_cannot_hold():
    from style_transfer import _hip as hip
    lib = hip.load_library()
    x = torch.zeros(16, device=DEV)
    scratch = torch.zeros(1 << 16, device=DEV)
    for c, n in ((0, 4), (1, 0), (1, 1 << 32), (1 << 30, 1 << 20)):
        assert lib.st_op_channel_sort(hip._ptr(x), c, n, hip._ptr(scratch), None, None, None) != 0
        assert 'launch_channel_sort' in lib.st_last_error().decode()


# ---- 2. the resample --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c, n_in, n_out', [(3, 3, 6), (3, 3, 2), (2, 1, 5), (5, 1488, 1920), (4, 2464, 1920), (3, 30, 6), (2, 5000, 1025),
                                            (3, 1000, 1000)])
def test_the_resample(c, n_in, n_out):
    from style_transfer import _hip as hip
    g = torch.Generator().manual_seed(n_in + n_out)
    q = torch.sort(torch.randn((c, n_in), generator=g).clamp(min=-0.5), dim=1).values.contiguous()
    got = hip.op_resample_quantiles(q.to(DEV), n_out).cpu()
    if n_in == n_out:
        assert torch.equal(got, q)
        return
    want = resample_formula(q.double().numpy(), n_out)
    scale = float(q.abs().max())
    worst = float(np.abs(got.double().numpy() - want).max()) / scale
    err = float(np.linalg.norm(got.double().numpy() - want) / np.linalg.norm(want))
    print(f'[w2marg] resample ({c}, {n_in}) -> {n_out}: worst |difference| / max |q| {worst:.2e}, rel-L2 {err:.2e} (bars 1e-6)')
    assert worst <= 1e-6 and err <= 1e-6
    assert bool((got[:, 1:] >= got[:, :-1]).all())


# ---- 3. the standalone loss, its backward and the module --------------------------------------------------------------------
def _op_shapes():
    return [(c, n) for c, n in _sort_shapes()]


@pytest.mark.parametrize('index', range(10))
def test_the_operators_and_the_module(index):
    from style_transfer import _hip as hip
    from style_transfer import losses
    c, n = _op_shapes()[index]
    n_q = max(1, (n * 3) // 4 + 1)
    x = _sort_input('relu', c, n, 7 + index) * 1.5 - 0.1
    q = torch.sort(_sort_input('relu', c, n_q, 8 + index), dim=1).values.contiguous()
    want, want_grad = marginal_formula(x.double().numpy(), q.double().numpy())
    xd, qd = x.to(DEV), q.to(DEV)
    target = hip.op_resample_quantiles(qd, n)
    loss, unit = hip.op_w2_marginal_loss(xd, target)
    loss2, unit2 = hip.op_w2_marginal_loss(xd, target)
    up = torch.tensor(-1.75, device=DEV)
    grad_up = hip.op_w2_marginal_loss_backward(unit, up)
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2) and torch.equal(unit, unit2)
    norm = np.linalg.norm(want_grad)
    ev = abs(loss.item() - want) / abs(want)
    eg = float(np.linalg.norm(unit.cpu().double().numpy() - want_grad) / norm)
    eu = float(np.linalg.norm(grad_up.cpu().double().numpy() + 1.75 * want_grad) / (1.75 * norm))
    print(f'[w2marg] operators ({c}, {n}) against {n_q} quantiles: value {ev:.2e}, gradient {eg:.2e}, under upstream -1.75 {eu:.2e} '
          f'(bars 1e-4)')
    assert ev <= 1e-4 and eg <= 1e-4 and eu <= 1e-4
    # its own target: exactly 0 with an exactly zero gradient
    own, _ = hip.op_channel_sort(xd, indices=False)
    zero, zero_grad = hip.op_w2_marginal_loss(xd, own)
    assert zero.item() == 0.0 and not zero_grad.any()
    # the module: the native path is counted, agrees with its torch path, and native(False) takes torch
    h = 1 if n < 4 or n % 4 else 4
    shape = (c, h, n // h)
    module = losses.StyleLossW2Marginal(qd)
    before = losses.native_calls.get('w2_marginal', 0)
    xn = xd.reshape(shape).clone().requires_grad_()
    value = module(xn)
    (value * 3.5).backward()
    assert losses.native_calls.get('w2_marginal', 0) == before + 1
    with losses.native(False):
        xt = xd.reshape(shape).clone().requires_grad_()
        value_t = module(xt)
        (value_t * 3.5).backward()
    assert losses.native_calls.get('w2_marginal', 0) == before + 1
    assert abs(value.item() - want) / abs(want) <= 1e-4
    assert abs(value.item() - value_t.item()) / abs(value_t.item()) <= 1e-4
    assert rel_l2(xn.grad.cpu(), xt.grad.cpu()) <= 1e-4
    assert rel_l2(xn.grad.cpu().double().reshape(c, n), 3.5 * torch.from_numpy(want_grad)) <= 1e-4


def test_the_module_on_the_device():
    from style_transfer import losses
    x = (_sort_input('relu', 64, 120, 21)).reshape(64, 12, 10).to(DEV)
    style = _sort_input('relu', 64, 99, 22).reshape(1, 64, 9, 11).to(DEV)
    before = losses.native_calls.get('moments', 0)
    target = losses.StyleLossW2Marginal.get_target(style)
    assert losses.native_calls.get('moments', 0) == before + 1
    assert target.shape == (1, 64, 99) and torch.equal(target.cpu(), torch.sort(style.cpu().flatten(-2) + 0.0, dim=-1, stable=True).values)
    module = losses.StyleLossW2Marginal(target[0])
    before = losses.native_calls.get('w2_marginal', 0)
    # a batch, float64 and create_graph are the torch code
    assert torch.isfinite(module(torch.stack([x, x]))) and torch.isfinite(module.double()(x.double()))
    module = module.float()
    xg = x.clone().requires_grad_()
    (g,) = torch.autograd.grad(module(xg), xg, create_graph=True)
    assert losses.native_calls.get('w2_marginal', 0) == before + 1 and g.requires_grad
    g.pow(2).sum().backward()
    assert torch.isfinite(xg.grad).all()
    # its own target: exactly 0, exactly zero gradient, natively
    own = losses.StyleLossW2Marginal(losses.StyleLossW2Marginal.get_target(x))
    xs = x.clone().requires_grad_()
    v = own(xs)
    v.backward()
    assert losses.native_calls.get('w2_marginal', 0) == before + 2
    assert v.item() == 0.0 and not xs.grad.any()


# ---- 4. plans ---------------------------------------------------------------------------------------------------------------
def _sorted_rows(feat, dtype):
    return torch.sort(feat[0].flatten(1).to(dtype) + 0.0, dim=1, stable=True).values


def _resample(q, n):
    """include/st_amd.h's resample in q's dtype with u in float64 (test_w2_marginal_cpu.resample_formula, vectorised)."""
    n_q = q.shape[-1]
    if n_q == n:
        return q
    u = ((torch.arange(n, dtype=torch.float64) + 0.5) * n_q / n - 0.5).clamp(0, n_q - 1)
    lo = u.floor().long()
    hi = (lo + 1).clamp(max=n_q - 1)
    return q[:, lo] + (u - lo).to(q.dtype) * (q[:, hi] - q[:, lo])


def _marginal_term(feat, q):
    """include/st_amd.h's term of a flagged entry before its weight; autograd's sort gives the gradient the header states."""
    mat = feat[0].flatten(1)
    values = torch.sort(mat + 0.0, dim=1, stable=True).values
    return ((values - _resample(q, mat.shape[1])) ** 2).mean()


def _style_feats(size, pooling, style_size=None):
    if style_size is None:
        return T._inputs(size, pooling)['sfeats']
    with torch.no_grad():
        return O.vgg_features(T._smooth(72, *style_size), T._weights(), list(range(1, 30)), pooling)


def _set_targets(plan, size, pooling, content_layers, style_layers, marg, style_size=None):
    ctargets, moments = T._targets(size, pooling, content_layers, style_layers)
    sfeats = _style_feats(size, pooling, style_size)
    for i, layer in enumerate(content_layers):
        plan.set_content_target(ctargets[layer].to(DEV), i)
    for i, layer in enumerate(style_layers):
        if marg[i]:
            plan.set_style_quantiles(i, _sorted_rows(sfeats[layer], torch.float32).to(DEV))
        else:
            plan.set_style_target(i, moments[layer][0].to(DEV), moments[layer][1].to(DEV))


def _plan(size, pooling, precision, content_layers, style_layers, kinds, diag, marg, configure=True, style_size=None):
    """A plan in the documented order: layers, kinds, diagonal, marginal, weights, targets."""
    from style_transfer import _hip as hip
    net = hip.Net(T._weights(), pooling, DEV, precision)
    plan = hip.Plan(net, *size)
    if configure:
        plan.set_taps(content_layers, style_layers)
    if kinds is not None:
        plan.set_layer_loss_kinds(*kinds)
    if diag is not None and any(diag):
        plan.set_w2_diagonal(diag)
    if marg is not None:
        plan.set_w2_marginal(marg)
        assert plan.w2_marginal == tuple(bool(v) for v in marg)
    plan.set_loss_weights(*T._layer_weights(content_layers, style_layers), T.TV_WEIGHT)
    _set_targets(plan, size, pooling, content_layers, style_layers, marg or [False] * len(style_layers), style_size)
    return net, plan


def _oracle(image, pooling, decisions, content_layers, style_layers, ctargets, moments, sfeats, weights, kinds, diag, marg, clevels,
            tvmap, lap, dtype, others=False):
    """SumLoss in `dtype`: (weighted content terms, weighted style terms, the image-space term, total, gradient and - others -
    per flagged layer the weighted (diagonal, full W2) terms of the same tap)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cws, sws = weights
    img = image.to(dtype).clone().requires_grad_(True)
    feats = O.vgg_features(img, T._weights() if dtype == torch.float32 else T._weights64(), content_layers + style_layers, pooling,
                           decisions)
    cterms = []
    for layer, cw, kind in zip(content_layers, cws, kinds[0]):
        wmap = None if clevels is None else clevels[MG.LEVEL[layer]].to(dtype)
        cterms.append(CM.weighted_content(feats[layer], ctargets[layer].to(dtype), wmap, kind, 1e-8) * cw)
    sterms = []
    for layer, sw, kind, dg, mg in zip(style_layers, sws, kinds[1], diag, marg):
        if mg:
            # the fp32 composition resamples the fp32 quantiles in fp32, the float64 one the same quantiles in float64
            sterms.append(_marginal_term(feats[layer], _sorted_rows(sfeats[layer], torch.float32).to(dtype)) * sw)
        else:
            sterms.append(D._style_term(feats[layer], layer, moments[layer], None, kind, dg, None, dtype) * sw)
    space = (O.tv_loss(img) if tvmap is None else CM.weighted_tv(img, tvmap.to(dtype))) * T.TV_WEIGHT
    if lap is not None:
        for term in formula_terms(img, lap[0].to(dtype), lap[1]):
            space = space + term * lap[2]
    total = sum(cterms) + sum(sterms) + space
    (grad,) = torch.autograd.grad(total, img)
    alt = None
    if others:
        with torch.no_grad():
            alt = [(float(D._style_term(feats[layer], layer, moments[layer], None, 'w2', True, None, dtype) * sw),
                    float(D._style_term(feats[layer], layer, moments[layer], None, 'w2', False, None, dtype) * sw)) if mg else None
                   for layer, sw, mg in zip(style_layers, sws, marg)]

    def f(t):
        return float(t.detach())
    return [f(t) for t in cterms], [f(t) for t in sterms], f(space), f(total), grad.detach(), alt


def _judge(tag, plan, img, image, pooling, content_layers, style_layers, kinds, diag, marg, lap_pools=None, style_size=None):
    """One closure of `plan` against the oracle under the plan's OWN maps.  Returns (failures, the smallest distance in bars of a
    diagonal or full W2 term from its marginal term, (the oracle's float64 gradient, the fp32 composition's rel-L2 from it))."""
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
    lap = None if lap_pools is None else (LG._content(size), lap_pools, LG.LAP_WEIGHT)
    losses, grad = plan.loss_and_grad(img)
    torch.cuda.synchronize()
    terms = plan.term_losses().cpu().numpy()
    losses = losses.cpu().numpy()
    nc, ns = len(content_layers), len(style_layers)
    ctargets, moments = T._targets(size, pooling, content_layers, style_layers)
    args = (image, pooling, decisions, content_layers, style_layers, ctargets, moments, _style_feats(size, pooling, style_size),
            T._layer_weights(content_layers, style_layers), kinds, diag, marg, clevels, tvmap, lap)
    c32, s32, sp32, _, g32, _ = _oracle(*args, torch.float32)
    c64, s64, sp64, _, g64, alt = _oracle(*args, torch.float64, others=True)
    assert len(terms) == nc + ns + 1 and np.isfinite(terms).all() and np.isfinite(losses).all(), f'{tag}: terms {terms}'
    failures, smallest = [], float('inf')

    def check(name, got, want32, want64):
        floor = abs(want32 - want64) / abs(want64)
        tol = max(T.TERM_TOL, 3 * floor)
        rel = abs(got - want32) / abs(want32)
        print(f'[w2marg] {tag} term {name:24s} got {got:.8g} want {want32:.8g} rel {rel:.2e}  floor {floor:.2e}  bar {tol:.1e}  '
              f'{"PASS" if rel <= tol else "FAIL"}')
        if not rel <= tol:
            failures.append(f'{tag}: term {name} rel {rel:.2e} > {tol:.1e}')
        return tol
    for i, layer in enumerate(content_layers):
        check(f'content[{layer}]', float(terms[i]), c32[i], c64[i])
    for j, layer in enumerate(style_layers):
        what = 'marginal w2' if marg[j] else 'diagonal w2' if diag[j] else kinds[1][j]
        tol = check(f'style[{layer}] {what}', float(terms[nc + j]), s32[j], s64[j])
        if marg[j]:
            for name, other in zip(('diagonal', 'full W2'), alt[j]):
                ratio = abs(other - s64[j]) / abs(s64[j]) / tol
                smallest = min(smallest, ratio)
                print(f'[w2marg] {tag} style[{layer}]: the {name} term {other:.6g} is {ratio:.0f} bars from the marginal one {s64[j]:.6g}')
                assert ratio >= IGNORED_BARS, f'{tag}: style[{layer}]: the {name} term is {ratio:.1f} bars away only'
    check('image-space (tv, laplacian)', float(terms[-1]), sp32, sp64)
    want_total = np.float32(0)
    for t in terms.astype(np.float32):
        want_total = np.float32(want_total + t)
    rel_total = abs(float(losses[7]) - float(want_total)) / abs(float(want_total))
    print(f'[w2marg] {tag} total {losses[7]:.8g} vs fp32 sum of the terms {want_total:.8g} rel {rel_total:.2e} (bar {T.SUM_TOL:.0e})')
    if not rel_total <= T.SUM_TOL:
        failures.append(f'{tag}: total rel {rel_total:.2e} > {T.SUM_TOL:.0e}')
    assert torch.isfinite(grad).all(), f'{tag}: non-finite gradient'
    err, floor = rel_l2(grad.cpu(), g64), rel_l2(g32, g64)
    b = T.bar(floor)
    print(f'[w2marg] {tag} gradient hip-vs-fp64 {err:.2e}  ref-fp32 floor {floor:.2e}  bar {b:.1e}  {"PASS" if err <= b else "FAIL"}')
    if not err <= b:
        failures.append(f'{tag}: gradient rel-L2 {err:.2e} > {b:.1e} (floor {floor:.2e})')
    print(f'[w2marg] {tag}: smallest distance of a diagonal or full W2 term from its marginal term: {smallest:.0f} bars')
    return failures, smallest, (g64, floor)


CASES = [
    # name, size, pooling, precision, (content layers, style layers), style kinds, diagonal flags, marginal flags, configure, style size
    ('all-five', SIZE, 'max', 'fp16x3', T.DEFAULT, W2, NONE, ALL, False, None),
    ('all-five-odd-fp32', ODD, 'max', 'fp32', T.DEFAULT, W2, NONE, ALL, False, None),
    ('all-five-average', SIZE, 'average', 'fp16x3', T.DEFAULT, W2, NONE, ALL, False, None),
    ('all-five-style-56x44', SIZE, 'max', 'fp16x3', T.DEFAULT, W2, NONE, ALL, False, (56, 44)),
    ('deep-two-odd', ODD, 'max', 'fp16x3', T.DEFAULT, W2, NONE, DEEP, False, None),
    ('deep-two-fp32-average', SIZE, 'average', 'fp32', T.DEFAULT, W2, NONE, DEEP, False, None),
    ('with-gram-and-diagonal', SIZE, 'max', 'fp16x3', T.DEFAULT, ['w2', 'gram', 'w2', 'w2', 'w2'], [True, False, False, False, False],
     [False, False, True, False, True], False, None),
    ('list-d-average', SIZE, 'average', 'fp16x3', T.CONFIGS['d'], ['w2'] * 3, [False] * 3, [True] * 3, True, None),
    ('list-e-odd', ODD, 'max', 'fp16x3', T.CONFIGS['e'], ['w2'] * 4, [False] * 4, [True, False, True, True], True, None),
    ('a-layer-in-both-lists', SIZE, 'max', 'fp16x3', T.CONFIGS['b'], W2, NONE, DEEP, True, None),
]


@pytest.mark.parametrize('name, size, pooling, precision, lists, style_kinds, diag, marg, configure, style_size', CASES,
                         ids=[c[0] for c in CASES])
def test_configurations(name, size, pooling, precision, lists, style_kinds, diag, marg, configure, style_size):
    content_layers, style_layers = lists
    kinds = (['mse'] * len(content_layers), style_kinds)
    image = T._inputs(size, pooling)['image']
    img = image.to(DEV)
    _, plan = _plan(size, pooling, precision, content_layers, style_layers, None if style_kinds == W2[:len(style_kinds)] else kinds,
                    diag, marg, configure, style_size)
    tag = f'({name}) style {style_layers} flags {[int(f) for f in marg]} {size[0]}x{size[1]}-{pooling}-{precision}'
    failures, _, _ = _judge(tag, plan, img, image, pooling, content_layers, style_layers, kinds, diag, marg, style_size=style_size)
    # the plan's own permutation check: the sorted tap of a forward is torch.sort of the tap, exactly
    plan.forward(img, max(style_layers))
    for j, layer in enumerate(style_layers):
        if marg[j]:
            feat = plan.feature(layer).cpu()
            assert torch.equal(plan.quantiles(layer).cpu(), _sorted_rows(feat, torch.float32)), f'{tag}: quantiles of features[{layer}]'
            # ... and the borrowed target is the resample of what was set
            q = _sorted_rows(_style_feats(size, pooling, style_size)[layer], torch.float32)
            held = plan.style_quantiles(j).cpu()
            want = resample_formula(q.double().numpy(), held.shape[1])
            assert held.shape == (feat.shape[1], feat.shape[2] * feat.shape[3])
            assert np.abs(held.double().numpy() - want).max() <= 1e-6 * float(q.abs().max())
    if configure:
        L._configured_array(plan.term_losses().cpu().double().numpy(), plan.loss_and_grad(img)[0].cpu().numpy(), len(content_layers),
                            len(style_layers))
    assert not failures, '; '.join(failures)


def test_both_maps_and_the_laplacian():
    marg = [True, False, True, False, True]
    image = T._inputs(SIZE, 'max')['image']
    _, plan = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, None, None, marg, configure=False)
    plan.set_content_mask(MG.ramp_mask(*SIZE).to(DEV))
    plan.set_tv_mask(MG.binary_mask(*SIZE).to(DEV))
    plan.set_laplacian(LG._content(SIZE).to(DEV), (4, 16), LG.LAP_WEIGHT)
    failures, _, _ = _judge('content map + TV map + Laplacian, flags 1,0,1,0,1', plan, image.to(DEV), image, 'max', *T.DEFAULT,
                            (MSE, W2), NONE, marg, lap_pools=(4, 16))
    assert not failures, '; '.join(failures)


# ---- 5. bits and steps ------------------------------------------------------------------------------------------------------
def _flagged_plan(marg=(True, False, False, True, True)):
    return _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, None, None, list(marg), configure=False)[1]


def test_two_closures_are_equal_step_is_closure_plus_update_and_the_range_guard_runs():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    plan = _flagged_plan()
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
    before = K._leg(plan, img, steps=False)
    fwd, bwd = plan.range_guard(img)
    assert not any(fwd) and not any(bwd)
    assert T._same(before, K._leg(plan, img, steps=False))


def test_native_steps_move_the_image_as_the_oracle_gradient_does():
    """One native Adam step and one native L-BFGS step against the same update applied to the oracle's float64 gradient.
    Adam's first step is lr g / (|g| + eps), lr sign(g) in effect: pixels whose gradient is ~0 may flip under fp32 rounding, so
    the bulk of the image is judged - fewer than 0.2 % of the pixels off by more than 1e-4 (__graft_entry__.smoke's bar), hence
    a mean difference below 0.2 % of the 2 lr a flip moves, 8e-5 < 1e-4.  L-BFGS's first step is -t g with one scalar t: the
    displacement against t times the float64 gradient is judged in rel-L2 by the gradient's own bar, T.bar(floor)."""
    from style_transfer import _hip as hip
    image = T._inputs(SIZE, 'max')['image']
    img = image.to(DEV)
    plan = _flagged_plan(ALL)
    _, _, (g64, floor) = _judge('steps', plan, img, image, 'max', *T.DEFAULT, (MSE, W2), NONE, ALL)
    xa, ma, va, ea = T._state(img)
    plan.step(xa, ma, va, ea, 1, 0.02)
    want = (image.double() - 0.02 * g64 / (g64.abs() + 1e-8)).clamp(0, 1)
    diff = (xa.cpu().double() - want).abs()
    frac_off = float((diff > 1e-4).double().mean())
    print(f'[w2marg] Adam step: mean |difference| {float(diff.mean()):.2e}, {100 * frac_off:.3f}% of pixels off by > 1e-4')
    assert frac_off < 2e-3 and float(diff.mean()) < 1e-4
    xb, _, _, eb = T._state(img)
    opt = hip.LBFGS(xb)
    opt.step(plan, xb, eb, 0.99)
    moved = (xb.cpu().double() - image.double())
    inside = (xb.cpu() > 0) & (xb.cpu() < 1)                   # (clamped pixels aside)
    # the first L-BFGS step is -t g with one scalar t: the displacement is parallel to the oracle's gradient
    t = float((moved[inside] * g64[inside]).sum() / (g64[inside] ** 2).sum())
    err = float(torch.linalg.norm(moved[inside] - t * g64[inside]) / torch.linalg.norm(t * g64[inside]))
    print(f'[w2marg] L-BFGS step: t {t:.4g}, displacement against t x the float64 gradient rel-L2 {err:.2e} (bar {T.bar(floor):.1e})')
    assert t < 0 and err <= T.bar(floor)


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
    _, zeros = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, None, None, NONE, configure=False)
    assert zeros.w2_marginal == (False,) * 5
    assert len(want) == 10 and T._same(want, K._leg(zeros, img, steps=True))
    cleared = _flagged_plan(ALL)
    flagged = K._leg(cleared, img, steps=False)
    assert not torch.equal(flagged[0], want[0])
    cleared.set_w2_marginal(None)
    assert cleared.w2_marginal == (False,) * 5
    T._set_targets(cleared, SIZE, 'max', *T.DEFAULT)
    assert T._same(want, K._leg(cleared, img, steps=True))


def test_a_flagged_head_allocates_no_c_by_c_workspace():
    from style_transfer import _hip as hip
    net = hip.Net(T._weights(), 'max', DEV, 'fp16x3')
    used = {}
    for name, marg in (('full', NONE), ('deep', DEEP)):
        plan = hip.Plan(net, *SIZE)
        plan.set_w2_marginal(marg)
        _set_targets(plan, SIZE, 'max', *T.DEFAULT, marg)
        torch.cuda.synchronize()
        used[name] = plan.device_bytes()
    print(f'[w2marg] st_plan_device_bytes at 40x48: five full W2 heads {used["full"]}, relu4_1 and relu5_1 marginal {used["deep"]}')
    # (nine 512 x 512 matrices per full head - test_w2_diagonal_gpu - less a marginal head's target and keys: under one such matrix)
    assert used['full'] - used['deep'] >= 2 * 8 * 512 * 512 * 4


# ---- 6. setter semantics ----------------------------------------------------------------------------------------------------
def _ints(*values):
    return (ctypes.c_int * max(len(values), 1))(*values)


def test_setter_semantics():
    from style_transfer import _hip as hip
    from style_transfer import sharding
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    net = hip.Net(T._weights(), 'max', DEV, 'fp16x3')
    plan = hip.Plan(net, *SIZE)
    lib = plan.lib

    def refused(call, *words):
        assert call() != 0
        message = lib.st_last_error().decode()
        for word in words:
            assert word in message, (word, message)
    assert plan.w2_marginal == (False,) * 5
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    before = K._leg(plan, img, steps=False)
    moments = T._targets(SIZE, 'max', *T.DEFAULT)[1]
    q = _sorted_rows(T._inputs(SIZE, 'max')['sfeats'][29], torch.float32).to(DEV)
    # refusals carry a message and leave the plan as it was, targets included
    refused(lambda: lib.st_plan_set_w2_marginal(plan.handle, _ints(0, 0, 0, 0, 2)), '0 or 1', 'st_plan_set_w2_marginal')
    refused(lambda: lib.st_plan_set_w2_marginal(plan.handle, _ints(0, -1, 0, 0, 0)), '0 or 1')
    refused(lambda: lib.st_plan_set_style_quantiles(plan.handle, 4, hip._ptr(q), q.shape[1], None), 'not flagged')
    assert T._same(before, K._leg(plan, img, steps=False))
    plan.set_layer_loss_kinds(MSE, ['w2', 'gram', 'w2', 'gram', 'w2'])
    refused(lambda: lib.st_plan_set_w2_marginal(plan.handle, _ints(0, 0, 0, 1, 0)), 'gram')
    with pytest.raises(hip.HipLibraryError, match='gram'):
        plan.set_w2_marginal(True)
    with pytest.raises(ValueError, match='one per layer'):
        plan.set_w2_marginal([True] * 4)
    plan.set_layer_loss_kinds(MSE, W2)
    # diagonal and marginal exclude each other, both ways
    plan.set_w2_diagonal([True, False, False, False, False])
    refused(lambda: lib.st_plan_set_w2_marginal(plan.handle, _ints(1, 0, 0, 0, 0)), 'diagonal')
    plan.set_w2_marginal(DEEP)
    assert plan.w2_marginal == tuple(DEEP) and plan.w2_diagonal == (True, False, False, False, False)
    refused(lambda: lib.st_plan_set_w2_diagonal(plan.handle, _ints(0, 0, 0, 0, 1)), 'marginal')
    plan.set_w2_diagonal(None)
    # a custom eps, both ways
    refused(lambda: plan.lib.st_plan_set_loss_eps(plan.handle, None, (ctypes.c_float * 5)(-1, -1, -1, -1, 1e-3)), 'marginal')
    plan.set_w2_marginal(None)
    plan.set_loss_eps(None, [None, None, None, None, 1e-3])
    refused(lambda: lib.st_plan_set_w2_marginal(plan.handle, _ints(0, 0, 0, 0, 1)), 'eps')
    plan.set_w2_marginal([False, False, False, True, False])
    plan.set_loss_eps(None, None)
    # masks and regions, both ways
    plan.set_w2_marginal(DEEP)
    mask = MG.ramp_mask(*SIZE).to(DEV)
    refused(lambda: lib.st_plan_set_style_mask(plan.handle, hip._ptr(mask), None), 'marginal')
    masks = (ctypes.c_void_p * 1)(mask.data_ptr())
    refused(lambda: lib.st_plan_set_style_regions(plan.handle, 1, masks, None), 'marginal')
    plan.set_style_mask(None)
    plan.set_style_regions(None)
    plan.set_w2_marginal(None)
    plan.set_style_mask(mask)
    refused(lambda: lib.st_plan_set_w2_marginal(plan.handle, _ints(0, 0, 0, 0, 1)), 'style mask')
    assert lib.st_plan_set_w2_marginal(plan.handle, _ints(0, 0, 0, 0, 0)) == 0
    plan.set_style_mask(None)
    plan.set_style_regions([mask])
    refused(lambda: lib.st_plan_set_w2_marginal(plan.handle, _ints(0, 0, 0, 0, 1)), 'regions')
    plan.set_style_regions(None)
    # the targets: dropped by the setter; the moments' setter refuses a flagged entry and names the other call
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    plan.loss_and_grad(img)
    plan.set_w2_marginal(DEEP)
    with pytest.raises(hip.HipLibraryError, match=r'content target 0 \(features\[22\]\)'):
        plan.loss_and_grad(img)
    with pytest.raises(hip.HipLibraryError, match='st_plan_set_style_quantiles'):
        plan.set_style_target(4, moments[29][0].to(DEV), moments[29][1].to(DEV))
    with pytest.raises(hip.HipLibraryError, match='not flagged'):
        plan.set_style_quantiles(0, q)
    with pytest.raises(hip.HipLibraryError, match='no quantile target'):
        plan.style_quantiles(4)
    _set_targets(plan, SIZE, 'max', *T.DEFAULT, DEEP)
    assert torch.isfinite(plan.loss_and_grad(img)[0]).all()
    assert plan.style_quantiles(4).shape == (512, 6)
    # either kinds setter and set_taps clear the flags
    plan.set_loss_kinds('mse', 'w2')
    assert plan.w2_marginal == (False,) * 5
    plan.set_w2_marginal(ALL)
    plan.set_layer_loss_kinds(MSE, W2)
    assert plan.w2_marginal == (False,) * 5
    plan.set_w2_marginal(ALL)
    plan.set_taps(*T.CONFIGS['b'])
    assert plan.w2_marginal == (False,) * 5
    plan.set_w2_marginal(ALL)
    plan.set_taps(*T.DEFAULT)
    assert plan.w2_marginal == (False,) * 5
    # back on the default configuration: the fast closure again, equal to a plan that never left it
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    fresh = hip.Plan(net, *SIZE)
    T._set_targets(fresh, SIZE, 'max', *T.DEFAULT)
    assert T._same(K._leg(plan, img, steps=True), K._leg(fresh, img, steps=True))
    # a strip plan takes cleared flags and refuses a set one
    strip = sharding.StripPlan(net, 48, 48, 0, 32)
    refused(lambda: lib.st_plan_set_w2_marginal(strip.handle, _ints(0, 0, 0, 0, 1)), 'strip')
    assert lib.st_plan_set_w2_marginal(strip.handle, _ints(0, 0, 0, 0, 0)) == 0
    assert lib.st_plan_set_w2_marginal(strip.handle, None) == 0


# ---- 7. stylize() -----------------------------------------------------------------------------------------------------------
def test_stylize_reads_style_marginal():
    from PIL import Image
    from style_transfer import StyleTransfer
    from style_transfer.style_transfer import size_to_fit, to_tensor
    st = StyleTransfer(devices=[DEV], pooling='max', weights='synthetic')
    assert st.style_marginal is False
    content_image, style_image = T._pil(81, 64, 48), T._pil(82, 60, 44)
    decay = 0.99
    seen = []

    def callback(it):
        if it.i == 1:
            avg, x1 = st.get_image_tensor(), st.image.detach()[0]
            seen.append((it.w, it.h, it.loss, (((1 + decay) * avg - x1) / decay).cpu()[None]))

    def run(min_scale=64):
        del seen[:]
        out = st.stylize(content_image, [style_image], end_scale=64, min_scale=min_scale, initial_iterations=4, iterations=4,
                         avg_decay=decay, callback=callback)
        assert out is not None and torch.isfinite(st.get_image_tensor()).all()
        return list(seen)

    default_loss = run()[0][2]
    st.style_marginal = DEEP
    scales = run(min_scale=45)                       # two scales: the flags are set per scale, before the targets
    assert len(scales) == 2 and scales[0][:2] != scales[1][:2]
    assert st._plan.w2_marginal == tuple(DEEP)
    # the final scale's first closure against the oracle's terms, on the image that scale started from
    w, h, loss, start = scales[1]
    assert (w, h) == size_to_fit(content_image.size, 64, scale_up=True)
    content = to_tensor(content_image.resize((w, h), Image.BICUBIC))[None]
    sw_, sh_ = size_to_fit(style_image.size, 64)
    style = to_tensor(style_image.resize((sw_, sh_), Image.BICUBIC))[None]
    with torch.no_grad():
        cfeats = O.vgg_features(content, T._weights(), st.content_layers, 'max')
        sfeats = O.vgg_features(style, T._weights(), st.style_layers, 'max')
    moments = {layer: O.feature_moments(sfeats[layer]) for layer in st.style_layers}
    totals = {}
    for marg in (DEEP, NONE):
        args = (start, 'max', None, st.content_layers, st.style_layers, cfeats, moments, sfeats, ([0.015], st.style_weights), (MSE, W2),
                NONE, marg, None, None, None)
        totals[tuple(marg)] = (_oracle(*args, torch.float32)[3], _oracle(*args, torch.float64)[3])
    total32, total64 = totals[tuple(DEEP)]
    floor = abs(total32 - total64) / abs(total64)
    tol, rel = max(T.TERM_TOL, 3 * floor), abs(loss - total32) / abs(total32)
    ignored = abs(totals[tuple(NONE)][1] - total64) / abs(total64)
    print(f'[w2marg] stylize {w}x{h}: first loss of the last scale {loss:.8g} oracle {total32:.8g} rel {rel:.2e} floor {floor:.2e} '
          f'bar {tol:.1e}; with full W2 heads the float64 total is {ignored / tol:.0f} bars away; the default run: {default_loss:.8g}')
    assert rel <= tol, f'{w}x{h}: first loss rel {rel:.2e} > {tol:.1e}'
    assert ignored >= IGNORED_BARS * tol
    # ... and its final closure: the plan's terms on the final image against the oracle's
    final = st.image.detach().clone()
    st._plan.loss_and_grad(final)
    torch.cuda.synchronize()
    got = st._plan.term_losses().cpu().numpy()
    args = (final.cpu(), 'max', None, st.content_layers, st.style_layers, cfeats, moments, sfeats, ([0.015], st.style_weights), (MSE, W2),
            NONE, DEEP, None, None, None)
    c32, s32, sp32 = _oracle(*args, torch.float32)[:3]
    c64, s64, sp64 = _oracle(*args, torch.float64)[:3]
    assert len(got) == 7
    for name, value, want32, want64 in zip(['content'] + [f'style[{layer}]' for layer in st.style_layers] + ['tv'], got, c32 + s32 + [sp32],
                                           c64 + s64 + [sp64]):
        bar = max(T.TERM_TOL, 3 * abs(want32 - want64) / abs(want64))
        rel_term = abs(float(value) - want32) / abs(want32)
        print(f'[w2marg] stylize final closure {name}: got {float(value):.8g} want {want32:.8g} rel {rel_term:.2e} bar {bar:.1e}')
        assert rel_term <= bar, f'final closure, {name}: rel {rel_term:.2e} > {bar:.1e}'
    del st.style_marginal
    assert run()[0][2] == default_loss and st._plan.w2_marginal == (False,) * 5
    st.style_marginal = [True, True]
    with pytest.raises(ValueError, match='style_marginal'):
        st.stylize(content_image, [style_image], end_scale=64, min_scale=64, initial_iterations=1, iterations=1)
    st.style_marginal, st.style_diagonal = DEEP, DEEP
    with pytest.raises(ValueError, match='style_marginal'):
        st.stylize(content_image, [style_image], end_scale=64, min_scale=64, initial_iterations=1, iterations=1)

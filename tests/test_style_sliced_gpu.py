"""The sliced Wasserstein option of a W2 style layer (st_plan_set_style_sliced, the st_op_sliced_* entries,
StyleTransfer.style_sliced, losses.StyleLossSliced) on a real MI355X.

Formula (include/st_amd.h), written out in float64 in tests/test_style_sliced_cpu.py:
    Y = R F;  T = sum_i a_i resample_N(sort_rows(R S_i));  term = sum_p,k (sort(Y)_p,k - T_p,k)^2 / (P N);  dF = (2 / (P N)) R^T G.
The directions are judged as what they must be - unit rows, a transpose that is one bit for bit, a function of (seed, entry,
epoch), first and fourth moments of sqrt(C) r that a standard normal direction has - and never against a host generator: every
other test takes the R the device drew (given to the operators, borrowed from the plan), converts it to float64 and evaluates the
formula there.  Bars, the project's own: 1e-4 on a value, 1e-4 rel-L2 on a gradient.

The standalone gradient and near-ties.  The permutation is taken from a projection computed in fp32-class arithmetic, so two pixels
whose float64 projections differ by less than that arithmetic's error can change places against the float64 order.  The value does
not feel it (measured: 1e-8 from float64 everywhere); the gradient does, because the two pixels exchange their residuals, and near
the target - tap and style drawn from one distribution with M = N, the hardest case and the one chosen here - the residuals are
small against the spacing of the target.  Measured, gradient rel-L2 against the float64-ORDER gradient on the cases below:
    fp16x3 projection  2.0e-4 (N = 4095), 6.2e-4 (4096), 3.1e-4 (4097), 5.1e-4 (8197), 5.4e-4 (C = 512), 3.8e-4 (P = 128)
    exact fp32 MFMA    2.6e-4,            1.9e-4,        6.9e-4,        4.8e-4,        6.2e-4,           4.1e-4
with 30 to 124 of 2.6e5 to 5.2e5 ranks exchanged under fp32, and 2.7e-7 to 5.4e-5 where M differs from N or the style is scaled.  The
exact fp32 MFMA was tried once, as the issue lays down, and misses the 1e-4 bar by as much: the cause is the 24-bit projection, not
the fp16x3 split.  So the test does what the issue prescribes for that outcome: the figure against the float64 order is PRINTED,
and the gradient is ASSERTED at 1e-4 against the float64 formula evaluated at the kernels' own permutation - the stable order of
st_op_sliced_project's output, which is bit for bit the projection the loss sorts.  That permutation is itself held to a derived
bound: wherever it leaves the float64 order, the float64 projections it puts in the wrong order differ by at most 2 E,
    E = (C + 1) 2^-21 max|F| max|R| + 3 C 2^-24 max_i |f_i|
(the operand and accumulation errors of tests/test_style_nearest_gpu.py's derivation, with |r_p| = 1).  The value bar is not
loosened, and the value at the kernels' permutation is held to it too.  In plans the image gradient meets 1e-4 against the float64
order on every configuration below.

Plans: inputs and helpers are tests/test_w2_marginal_gpu.py's (and through it test_taps_gpu.py's): sizes 40 x 48 and 45 x 54, the
oracle composed in float64 on the plan's own ReLU and pool decisions with the plan's directions.  Every flagged term within 1e-4 of
float64, every image gradient within 1e-4 rel-L2 of float64; unflagged terms at the bars of their own tests.  A flag that is
ignored cannot pass: the marginal and the full W2 term of the same tap are shown to lie at least 10 bars from the sliced term.
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
import test_w2_marginal_gpu as MQ
from test_laplacian_cpu import formula_terms
from test_style_sliced_cpu import sliced_formula, sliced_target_formula

pytestmark = pytest.mark.gpu
DEV = T.DEV
SIZE, ODD = D.SIZE, D.ODD
ALL, DEEP, MSE, W2 = D.ALL, D.DEEP, D.MSE, D.W2
NONE = [False] * 5
IGNORED_BARS = 10
BAR = 1e-4


# ---- 1. the directions --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('p, c', [(64, 64), (64, 512), (512, 64), (128, 128)])
def test_directions(p, c):
    from style_transfer import _hip as hip
    r, rt = hip.op_sliced_directions(3, 2, 5, p, c, DEV)
    again, again_t = hip.op_sliced_directions(3, 2, 5, p, c, DEV)
    assert r.shape == (p, c) and rt.shape == (c, p) and torch.isfinite(r).all()
    assert torch.equal(r, again) and torch.equal(rt, again_t)                   # the same (seed, entry, epoch): the same bits
    assert torch.equal(rt, r.t().contiguous())                                  # R^T is the transpose, bit for bit
    r64 = r.cpu().double()
    norm_err = float((r64.norm(dim=1) - 1).abs().max())
    for other in ((4, 2, 5), (3, 1, 5), (3, 2, 6)):                             # any one of the three changes every row
        changed = hip.op_sliced_directions(*other, p, c, DEV)[0]
        assert bool((changed != r).any(dim=1).all()), other
    x = (r64 * c ** 0.5).flatten()
    mean, fourth, want = float(x.mean()), float((x ** 4).mean()), 3 * c / (c + 2)
    print(f'[sliced] directions P {p} C {c}: max |norm - 1| {norm_err:.2e} (bar 1e-6); mean {mean:+.4f} (bar {5 / (p * c) ** 0.5:.4f}); '
          f'mean x^4 {fourth:.4f} against 3C / (C + 2) = {want:.4f} (bar 0.8)')
    assert norm_err <= 1e-6
    assert abs(mean) <= 5 / (p * c) ** 0.5
    assert abs(fourth - want) <= 0.8                                            # (a sign vector gives 1, a uniform one 1.8)


def test_the_direction_operator_refuses_what_it_cannot_run():
    from style_transfer import _hip as hip
    for p, c, word in ((32, 64, 'projections'), (576, 64, 'projections'), (96, 64, 'projections'), (64, 48, 'channels'), (64, 16, 'channels')):
        with pytest.raises(hip.HipLibraryError, match=word):
            hip.op_sliced_directions(0, 0, 0, p, c, DEV)


# ---- 2. the operators with given directions -------------------------------------------------------------------------------------
def _data(kind, c, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((c, n), generator=g) * 1.3 + 0.2
    if kind == 'relu':
        x = x.clamp(min=0)                       # about half exact zeros: ties, ordered by pixel index
    elif kind == 'zeros':
        x = torch.zeros((c, n))
    return x


OP_CASES = [
    # name, C, P, N, the style images' M, their weights, the tap's data, the style's data
    ('N = 1', 64, 64, 1, [1], None, 'signed', 'signed'),
    ('N = chunk - 1', 64, 64, 4095, [4095], None, 'signed', 'signed'),
    ('N = chunk', 64, 64, 4096, [4096], None, 'relu', 'relu'),
    ('N = chunk + 1', 64, 64, 4097, [4097], None, 'signed', 'signed'),
    ('N = 2 chunks + 5', 64, 64, 2 * 4096 + 5, [2 * 4096 + 5], None, 'relu', 'relu'),
    ('M = 1', 64, 64, 1000, [1], None, 'signed', 'signed'),
    ('M = 3 N / 2', 64, 64, 1000, [1500], None, 'relu', 'relu'),
    ('M = 4096, N = 1000', 64, 64, 1000, [4096], None, 'signed', 'relu'),
    ('C = 512, P = 64', 512, 64, 900, [1350], None, 'relu', 'relu'),
    ('C = 64, P = 128', 64, 128, 2000, [2000], None, 'signed', 'signed'),
    ('two style images, 0.25 / 0.75', 64, 64, 1000, [700, 1300], [0.25, 0.75], 'relu', 'relu'),
    ('three style images, one of weight 0', 128, 64, 333, [333, 50, 400], [1.0, 0.0, 3.0], 'signed', 'relu'),
    ('an all-zero tap', 64, 64, 4096, [3000], None, 'zeros', 'relu'),
    ('an all-zero tap and style', 64, 64, 500, [500], None, 'zeros', 'zeros'),
]


def gradient_at_order(f, r, t, order):
    """(term, dF) of include/st_amd.h in float64 numpy with the permutation GIVEN: order [P, N], row p the pixel of every rank."""
    p, n = r.shape[0], f.shape[1]
    y = r @ f
    g = np.zeros_like(y)
    g[np.arange(p)[:, None], order] = np.take_along_axis(y, order, axis=1) - t
    return float((g * g).sum() / (p * n)), (2.0 / (p * n)) * (r.T @ g)


def _op_target(hip, styles, weights, r, rt, n):
    """T through st_op_sliced_target, image by image in image order, the weights over their sum."""
    weights = weights or [1.0] * len(styles)
    total, target = float(sum(weights)), None
    for s, w in zip(styles, weights):
        if w != 0:
            target = hip.op_sliced_target(s.to(DEV), r, rt, n, target, w / total)
    return target


@pytest.mark.parametrize('name, c, p, n, ms, weights, kind, style_kind', OP_CASES, ids=[case[0] for case in OP_CASES])
def test_value_gradient_and_determinism(name, c, p, n, ms, weights, kind, style_kind):
    from style_transfer import _hip as hip
    f = _data(kind, c, n, 100 + n)
    styles = [_data(style_kind, c, m, 200 + m + i) * (1.0 + 0.5 * i) for i, m in enumerate(ms)]
    r, rt = hip.op_sliced_directions(11, 0, 0, p, c, DEV)
    target = _op_target(hip, styles, weights, r, rt, n)
    loss, unit = hip.op_sliced_loss(f.to(DEV), r, rt, target)
    loss2, unit2 = hip.op_sliced_loss(f.to(DEV), r, rt, _op_target(hip, styles, weights, r, rt, n))
    torch.cuda.synchronize()
    assert torch.equal(loss, loss2) and torch.equal(unit, unit2), 'two calls must give the same bits'
    r64 = r.cpu().double().numpy()
    t64 = sliced_target_formula(r64, [s.double().numpy() for s in styles], weights or [1.0] * len(styles), n)
    want, want_grad = sliced_formula(f.double().numpy(), r64, t64)
    t_err = float(np.abs(target.cpu().double().numpy() - t64).max() / max(np.abs(t64).max(), 1e-30))
    if want == 0.0:                                  # all zeros against all zeros: exactly nothing
        assert float(loss) == 0.0 and not unit.any() and not target.any()
        return
    rel = abs(float(loss) - want) / abs(want)
    err64 = rel_l2(unit.cpu(), torch.from_numpy(want_grad))
    # the permutation the kernels went through: the stable order of their own projection.  Where it differs from the float64 order
    # the two projections must be near-ties, within twice the bound E of the module docstring
    f64 = f.double().numpy()
    y_gpu = hip.op_sliced_project(f.to(DEV), r, rt).cpu()
    perm = torch.sort(y_gpu + 0.0, dim=1, stable=True).indices.numpy()
    y64 = r64 @ f64
    along = np.take_along_axis(y64, perm, axis=1)
    bound = 2 * ((c + 1) * 2.0 ** -21 * float(f.abs().max()) * float(r.abs().max()) + 3 * c * 2.0 ** -24 * float(f.double().norm(dim=0).max()))
    inversion = float(np.maximum(along[:, :-1] - along[:, 1:], 0).max()) if n > 1 else 0.0
    differ = int((perm != np.argsort(y64 + 0.0, axis=1, kind='stable')).sum())
    own_value, own_grad = gradient_at_order(f64, r64, t64, perm)
    err = rel_l2(unit.cpu(), torch.from_numpy(own_grad))
    print(f'[sliced] {name}: C {c} P {p} N {n} M {ms}: target max err {t_err:.2e}; loss {float(loss):.8g} float64 {want:.8g} rel {rel:.2e} (bar '
          f'{BAR:.0e}); gradient rel-L2 at the kernels\' order {err:.2e} (bar {BAR:.0e}), at the float64 order {err64:.2e} (reported); '
          f'{differ} of {p * n} ranks differ, largest inversion {inversion:.2e} (bound {bound:.2e})')
    assert rel <= BAR and err <= BAR
    assert inversion <= bound, 'the kernels\' order differs from the float64 order by more than near-ties'
    assert abs(own_value - want) <= BAR * want
    # the upstream scalar times the unit gradient
    up = torch.tensor(-2.5, device=DEV)
    assert torch.equal(hip.op_sliced_loss_backward(unit, up), up * unit)


@pytest.mark.parametrize('n, m', [(777, 777), (5000, 1234)])
def test_identity_directions_give_the_marginal_operator(n, m):
    from style_transfer import _hip as hip
    f, s = _data('relu', 64, n, 7).to(DEV), _data('relu', 64, m, 8).to(DEV)
    eye = torch.eye(64, device=DEV)
    target = hip.op_sliced_target(s, eye, eye, n)
    loss, unit = hip.op_sliced_loss(f, eye, eye, target)
    q = hip.op_resample_quantiles(hip.op_channel_sort(s, indices=False)[0], n)
    want, want_unit = hip.op_w2_marginal_loss(f, q)
    t_rel = float((target - q).abs().max() / q.abs().max())
    rel, err = abs(float(loss) - float(want)) / abs(float(want)), rel_l2(unit.cpu(), want_unit.cpu())
    print(f'[sliced] R = I, N {n} M {m}: target rel {t_rel:.2e}, value rel {rel:.2e} (bars 1e-6), gradient rel-L2 {err:.2e} (bar {BAR:.0e}) '
          f'against st_op_w2_marginal_loss')
    # (the projection I F rounds every value to 22 bits of its bound: a near-tie of the tap can change order, which the value does
    # not feel and the gradient does - the module docstring)
    assert t_rel <= 1e-6 and rel <= 1e-6 and err <= BAR


@pytest.mark.parametrize('c, p, n, kind', [(64, 64, 4097, 'signed'), (512, 128, 300, 'relu')])
def test_the_target_own_tap(c, p, n, kind):
    from style_transfer import _hip as hip
    f = _data(kind, c, n, 9).to(DEV)
    r, rt = hip.op_sliced_directions(1, 0, 0, p, c, DEV)
    loss, unit = hip.op_sliced_loss(f, r, rt, hip.op_sliced_target(f, r, rt, n))
    y = r.cpu().double() @ f.cpu().double()
    scale = float((y ** 2).mean())
    g0 = (2.0 / (p * n)) * (r.cpu().double().t() @ y)          # the gradient against a zero target: the level a gradient is judged at
    level = float(unit.cpu().double().norm() / g0.norm())
    print(f'[sliced] own tap C {c} P {p} N {n}: term {float(loss):.3e} against mean(Y^2) {scale:.3e}; |gradient| / |gradient at T = 0| {level:.2e}')
    assert 0.0 <= float(loss) <= 1e-10 * scale and level <= 1e-5


def test_the_loss_operators_refuse_what_they_cannot_run():
    from style_transfer import _hip as hip
    r, rt = hip.op_sliced_directions(0, 0, 0, 64, 64, DEV)
    f = torch.zeros((64, 10), device=DEV)
    with pytest.raises(hip.HipLibraryError, match='channels'):
        hip.op_sliced_loss(torch.zeros((48, 10), device=DEV), r[:, :48].contiguous(), rt[:48].contiguous(), torch.zeros((64, 10), device=DEV))
    with pytest.raises(hip.HipLibraryError, match='projections'):
        hip.op_sliced_target(f, r[:32].contiguous(), rt[:, :32].contiguous(), 10)


def test_the_module_on_the_device():
    from style_transfer import losses
    from style_transfer import _hip as hip
    g = torch.Generator().manual_seed(41)
    x = torch.randn((1, 64, 9, 13), generator=g).clamp(min=-0.3)
    style = torch.randn((64, 7, 11), generator=g).clamp(min=-0.3)
    target = losses.StyleLossSliced.get_target(style).to(DEV)
    module = losses.StyleLossSliced(target, projections=128, seed=3)
    before = losses.native_calls.get('sliced', 0)
    xr = x.to(DEV).requires_grad_()
    value = module(xr)
    value.backward()
    assert losses.native_calls.get('sliced', 0) == before + 1 and module.epoch == 1
    r = hip.op_sliced_directions(3, 0, 0, 128, 64, DEV)[0].cpu().double().numpy()          # what the module drew: (seed, entry 0, epoch 0)
    t64 = sliced_target_formula(r, [target.cpu().double().numpy()], [1.0], 9 * 13)
    want, want_grad = sliced_formula(x[0].flatten(1).double().numpy(), r, t64)
    rel, err = abs(value.item() - want) / want, rel_l2(xr.grad.cpu()[0].flatten(1), torch.from_numpy(want_grad))
    print(f'[sliced] module: value rel {rel:.2e}, gradient rel-L2 {err:.2e}')
    assert rel <= BAR and err <= BAR
    second = module(x.to(DEV))
    assert module.epoch == 2 and second.item() != value.item()                  # the next epoch's directions
    # given directions: the library and the torch formula agree; create_graph goes through torch
    module.directions = torch.from_numpy(r).float().to(DEV)
    xa, xb = x.to(DEV).requires_grad_(), x.to(DEV).requires_grad_()
    a = module(xa)
    with losses.native(False):
        b = module(xb)
    assert abs(a.item() - b.item()) <= BAR * abs(b.item()) and abs(a.item() - value.item()) <= 1e-6 * abs(value.item())
    (ga,) = torch.autograd.grad(a, xa, create_graph=True)
    (gb,) = torch.autograd.grad(b, xb, create_graph=True)
    assert ga.requires_grad and rel_l2(ga.detach().cpu(), gb.detach().cpu()) <= BAR
    # what the library does not take runs in torch: a batch, float64, a channel count that is no multiple of 64
    count = losses.native_calls.get('sliced', 0)
    assert torch.isfinite(module(torch.cat([x, x]).to(DEV)))
    small = losses.StyleLossSliced(target[:48].contiguous())
    assert torch.isfinite(small(x[:, :48].to(DEV)))
    assert losses.native_calls.get('sliced', 0) == count


# ---- 3. plans -----------------------------------------------------------------------------------------------------------------
def _style_vectors(size, pooling, layer, style_size=None, samples=None):
    """One style image's feature vectors of a flagged layer as the plan is given them, [C, M] fp32 on the CPU."""
    from style_transfer.style_transfer import _nearest_sample_columns
    tap = MQ._style_feats(size, pooling, style_size)[layer][0].flatten(1)
    columns = _nearest_sample_columns(tap.shape[1], samples)
    return tap[:, torch.tensor(columns)].contiguous()


def _set_targets(plan, size, pooling, content_layers, style_layers, sliced, marg=None, style_size=None, samples=None):
    ctargets, moments = T._targets(size, pooling, content_layers, style_layers)
    sfeats = MQ._style_feats(size, pooling, None)
    for i, layer in enumerate(content_layers):
        plan.set_content_target(ctargets[layer].to(DEV), i)
    for i, layer in enumerate(style_layers):
        if sliced[i]:
            plan.set_style_sliced_vectors(i, _style_vectors(size, pooling, layer, style_size, samples).to(DEV))
        elif marg and marg[i]:
            plan.set_style_quantiles(i, MQ._sorted_rows(sfeats[layer], torch.float32).to(DEV))
        else:
            plan.set_style_target(i, moments[layer][0].to(DEV), moments[layer][1].to(DEV))


def _plan(size, pooling, precision, content_layers, style_layers, kinds, diag, marg, sliced, configure=True, style_size=None, samples=None,
          projections=None, resample=True, seed=0):
    """A plan in the documented order: layers, kinds, diagonal, marginal, sliced (flags, options, seed), weights, targets."""
    from style_transfer import _hip as hip
    net = hip.Net(T._weights(), pooling, DEV, precision)
    plan = hip.Plan(net, *size)
    if configure:
        plan.set_taps(content_layers, style_layers)
    if kinds is not None:
        plan.set_layer_loss_kinds(*kinds)
    if diag is not None and any(diag):
        plan.set_w2_diagonal(diag)
    if marg is not None and any(marg):
        plan.set_w2_marginal(marg)
    if sliced is not None:
        plan.set_style_sliced(sliced)
        assert plan.style_sliced == tuple(bool(v) for v in sliced)
        for j, flag in enumerate(sliced):
            if flag:
                plan.set_sliced_options(j, projections, resample)
        plan.set_sliced_seed(seed)
    plan.set_loss_weights(*T._layer_weights(content_layers, style_layers), T.TV_WEIGHT)
    _set_targets(plan, size, pooling, content_layers, style_layers, sliced or [False] * len(style_layers), marg, style_size, samples)
    return net, plan


def _sliced_term(feat, r, t):
    """include/st_amd.h's term of a flagged entry before its weight; autograd's sort gives the gradient the header states, the
    directions held constant."""
    y = r @ feat[0].flatten(1)
    values = torch.sort(y + 0.0, dim=1, stable=True).values
    return ((values - t) ** 2).mean()


def _oracle(image, pooling, decisions, content_layers, style_layers, ctargets, moments, sfeats, dirs, tgts, weights, kinds, diag, marg,
            sliced, clevels, tvmap, lap, dtype, others=False):
    """SumLoss in `dtype`: (weighted content terms, weighted style terms, the image-space term, total, gradient and - others - per
    flagged layer the weighted marginal and full W2 terms of the same tap).  dirs / tgts: per style layer the plan's directions
    and the float64 target under them."""
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
    for j, (layer, sw, kind) in enumerate(zip(style_layers, sws, kinds[1])):
        if sliced[j]:
            sterms.append(_sliced_term(feats[layer], dirs[j].to(dtype), tgts[j].to(dtype)) * sw)
        elif marg[j]:
            sterms.append(MQ._marginal_term(feats[layer], MQ._sorted_rows(sfeats[layer], torch.float32).to(dtype)) * sw)
        else:
            sterms.append(D._style_term(feats[layer], layer, moments[layer], None, kind, diag[j], None, dtype) * sw)
    space = (O.tv_loss(img) if tvmap is None else CM.weighted_tv(img, tvmap.to(dtype))) * T.TV_WEIGHT
    if lap is not None:
        for term in formula_terms(img, lap[0].to(dtype), lap[1]):
            space = space + term * lap[2]
    total = sum(cterms) + sum(sterms) + space
    (grad,) = torch.autograd.grad(total, img)
    alt = None
    if others:
        with torch.no_grad():
            alt = [(float(MQ._marginal_term(feats[layer], MQ._sorted_rows(sfeats[layer], torch.float32).to(dtype)) * sw),
                    float(D._style_term(feats[layer], layer, moments[layer], None, 'w2', False, None, dtype) * sw)) if fl else None
                   for layer, sw, fl in zip(style_layers, sws, sliced)]

    def f(t):
        return float(t.detach())
    return [f(t) for t in cterms], [f(t) for t in sterms], f(space), f(total), grad.detach(), alt


def _judge(tag, plan, img, image, pooling, content_layers, style_layers, kinds, diag, marg, sliced, lap_pools=None, style_size=None,
           samples=None):
    """One closure of `plan` against the oracle under the plan's OWN maps and directions.  Returns (failures, (the float64
    gradient, the fp32 composition's rel-L2 from it))."""
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
    grad = grad.clone()
    nc, ns = len(content_layers), len(style_layers)
    # the directions that closure used, and the float64 target under them from the vectors the plan was given
    dirs, tgts = [None] * ns, [None] * ns
    for j, layer in enumerate(style_layers):
        if sliced[j]:
            r = plan.sliced_directions(layer)[0].cpu().double()
            held_t = plan.sliced_target(layer).cpu().double()
            assert float((r.norm(dim=1) - 1).abs().max()) <= 1e-6 and held_t.shape[0] == r.shape[0]
            vectors = _style_vectors(size, pooling, layer, style_size, samples).double().numpy()
            dirs[j], tgts[j] = r, torch.from_numpy(sliced_target_formula(r.numpy(), [vectors], [1.0], held_t.shape[1]))
            assert bool((held_t[:, 1:] >= held_t[:, :-1]).all()), f'{tag}: style[{layer}]: the target rows are not sorted'
    ctargets, moments = T._targets(size, pooling, content_layers, style_layers)
    args = (image, pooling, decisions, content_layers, style_layers, ctargets, moments, MQ._style_feats(size, pooling, None), dirs, tgts,
            T._layer_weights(content_layers, style_layers), kinds, diag, marg, sliced, clevels, tvmap, lap)
    c32, s32, sp32, _, g32, _ = _oracle(*args, torch.float32)
    c64, s64, sp64, _, g64, alt = _oracle(*args, torch.float64, others=True)
    assert len(terms) == nc + ns + 1 and np.isfinite(terms).all() and np.isfinite(losses).all(), f'{tag}: terms {terms}'
    failures = []

    def check(name, got, want32, want64):
        floor = abs(want32 - want64) / abs(want64)
        tol = max(T.TERM_TOL, 3 * floor)
        rel = abs(got - want32) / abs(want32)
        print(f'[sliced] {tag} term {name:24s} got {got:.8g} want {want32:.8g} rel {rel:.2e}  floor {floor:.2e}  bar {tol:.1e}  '
              f'{"PASS" if rel <= tol else "FAIL"}')
        if not rel <= tol:
            failures.append(f'{tag}: term {name} rel {rel:.2e} > {tol:.1e}')
    for i, layer in enumerate(content_layers):
        check(f'content[{layer}]', float(terms[i]), c32[i], c64[i])
    for j, layer in enumerate(style_layers):
        if not sliced[j]:
            check(f'style[{layer}] {"marginal w2" if marg[j] else "diagonal w2" if diag[j] else kinds[1][j]}', float(terms[nc + j]), s32[j], s64[j])
            continue
        rel = abs(float(terms[nc + j]) - s64[j]) / abs(s64[j])
        print(f'[sliced] {tag} term style[{layer}] sliced       got {float(terms[nc + j]):.8g} float64 {s64[j]:.8g} rel {rel:.2e}  bar {BAR:.0e}  '
              f'{"PASS" if rel <= BAR else "FAIL"}')
        if not rel <= BAR:
            failures.append(f'{tag}: term style[{layer}] sliced rel {rel:.2e} > {BAR:.0e}')
        for other, value in zip(('marginal', 'full W2'), alt[j]):
            ratio = abs(value - s64[j]) / abs(s64[j]) / BAR
            print(f'[sliced] {tag} style[{layer}]: the {other} term {value:.6g} is {ratio:.0f} bars from the sliced one {s64[j]:.6g}')
            assert ratio >= IGNORED_BARS, f'{tag}: style[{layer}]: the {other} term is {ratio:.1f} bars away only'
    check('image-space (tv, laplacian)', float(terms[-1]), sp32, sp64)
    want_total = np.float32(0)
    for t in terms.astype(np.float32):
        want_total = np.float32(want_total + t)
    rel_total = abs(float(losses[7]) - float(want_total)) / abs(float(want_total))
    print(f'[sliced] {tag} total {losses[7]:.8g} vs fp32 sum of the terms {want_total:.8g} rel {rel_total:.2e} (bar {T.SUM_TOL:.0e})')
    if not rel_total <= T.SUM_TOL:
        failures.append(f'{tag}: total rel {rel_total:.2e} > {T.SUM_TOL:.0e}')
    assert torch.isfinite(grad).all(), f'{tag}: non-finite gradient'
    err, floor = rel_l2(grad.cpu(), g64), rel_l2(g32, g64)
    print(f'[sliced] {tag} gradient hip-vs-fp64 {err:.2e}  ref-fp32 floor {floor:.2e}  bar {BAR:.0e}  {"PASS" if err <= BAR else "FAIL"}')
    if not err <= BAR:
        failures.append(f'{tag}: gradient rel-L2 {err:.2e} > {BAR:.0e} (fp32 composition: {floor:.2e})')
    return failures, (g64, floor)


CASES = [
    # name, size, pooling, precision, (content layers, style layers), style kinds, diagonal, marginal, sliced, configure, style size, samples, P
    ('all-five', SIZE, 'max', 'fp16x3', T.DEFAULT, W2, NONE, NONE, ALL, False, None, None, None),
    ('all-five-odd-fp32', ODD, 'max', 'fp32', T.DEFAULT, W2, NONE, NONE, ALL, False, None, None, None),
    ('all-five-average', SIZE, 'average', 'fp16x3', T.DEFAULT, W2, NONE, NONE, ALL, False, None, None, None),
    ('all-five-style-56x44', SIZE, 'max', 'fp16x3', T.DEFAULT, W2, NONE, NONE, ALL, False, (56, 44), None, None),
    ('all-five-400-samples-128-directions', SIZE, 'max', 'fp16x3', T.DEFAULT, W2, NONE, NONE, ALL, False, None, 400, 128),
    ('deep-two-odd', ODD, 'max', 'fp16x3', T.DEFAULT, W2, NONE, NONE, DEEP, False, None, None, None),
    ('deep-two-fp32-average-64-directions', SIZE, 'average', 'fp32', T.DEFAULT, W2, NONE, NONE, DEEP, False, None, None, 64),
    ('with-gram-diagonal-and-marginal', SIZE, 'max', 'fp16x3', T.DEFAULT, ['w2', 'gram', 'w2', 'w2', 'w2'], [True, False, False, False, False],
     [False, False, True, False, False], [False, False, False, True, True], False, None, None, None),
    ('a-layer-in-both-lists', SIZE, 'max', 'fp16x3', T.CONFIGS['b'], W2, NONE, NONE, DEEP, True, None, None, None),
]


@pytest.mark.parametrize('name, size, pooling, precision, lists, style_kinds, diag, marg, sliced, configure, style_size, samples, proj', CASES,
                         ids=[c[0] for c in CASES])
def test_configurations(name, size, pooling, precision, lists, style_kinds, diag, marg, sliced, configure, style_size, samples, proj):
    content_layers, style_layers = lists
    kinds = (['mse'] * len(content_layers), style_kinds)
    image = T._inputs(size, pooling)['image']
    img = image.to(DEV)
    _, plan = _plan(size, pooling, precision, content_layers, style_layers, None if style_kinds == W2[:len(style_kinds)] else kinds,
                    diag, marg, sliced, configure, style_size, samples, projections=proj)
    tag = f'({name}) style {style_layers} flags {[int(f) for f in sliced]} {size[0]}x{size[1]}-{pooling}-{precision}'
    failures, _ = _judge(tag, plan, img, image, pooling, content_layers, style_layers, kinds, diag, marg, sliced, style_size=style_size,
                         samples=samples)
    # the next closure, under the next epoch's directions, is judged the same way
    more, _ = _judge(tag + ' second closure', plan, img, image, pooling, content_layers, style_layers, kinds, diag, marg, sliced,
                     style_size=style_size, samples=samples)
    assert not failures + more, '; '.join(failures + more)


def test_both_maps_and_the_laplacian():
    sliced = [True, False, True, False, True]
    image = T._inputs(SIZE, 'max')['image']
    _, plan = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, None, None, None, sliced, configure=False)
    plan.set_content_mask(MG.ramp_mask(*SIZE).to(DEV))
    plan.set_tv_mask(MG.binary_mask(*SIZE).to(DEV))
    plan.set_laplacian(LG._content(SIZE).to(DEV), (4, 16), LG.LAP_WEIGHT)
    failures, _ = _judge('content map + TV map + Laplacian, flags 1,0,1,0,1', plan, image.to(DEV), image, 'max', *T.DEFAULT,
                         (MSE, W2), NONE, NONE, sliced, lap_pools=(4, 16))
    assert not failures, '; '.join(failures)


# ---- 4. epochs, bits and steps ------------------------------------------------------------------------------------------------
def _flagged_plan(sliced=(True, False, False, True, True), **kwargs):
    return _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, None, None, None, list(sliced), configure=False, **kwargs)[1]


def _closure(plan, img, layers=(1, 20, 29)):
    """One closure's outputs with the directions, epochs and targets it used."""
    out = [t.clone() for t in plan.loss_and_grad(img)] + [plan.term_losses().clone()]
    epochs = []
    for layer in layers:
        r, epoch = plan.sliced_directions(layer)
        out += [r, plan.sliced_target(layer)]
        epochs.append(epoch)
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in out)
    return out, epochs


def test_resampling_on_epochs_and_seeds():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    plan, twin, other = _flagged_plan(seed=7), _flagged_plan(seed=7), _flagged_plan(seed=8)
    assert plan.sliced_directions(1)[1] == 0                       # before any closure: what the setter drew, at epoch 0
    runs, twins, others = [], [], []
    for k in range(3):
        out, epochs = _closure(plan, img)
        assert epochs == [k] * 3, (k, epochs)                      # one plan-wide counter, advanced by exactly one per closure
        runs.append(out)
        twins.append(_closure(twin, img)[0])
        others.append(_closure(other, img)[0])
    for k in range(3):
        assert T._same(runs[k], twins[k]), f'closure {k}: the same seed must give the same bits'
        assert not torch.equal(runs[k][3], others[k][3]) and not torch.equal(runs[k][0], others[k][0]), f'closure {k}: another seed'
    for k in range(2):                                             # consecutive closures: other directions, another target, another value
        assert not torch.equal(runs[k][3], runs[k + 1][3]) and not torch.equal(runs[k][4], runs[k + 1][4])
        assert not torch.equal(runs[k][0], runs[k + 1][0])
    # the seed setter returns the epoch to 0 (and drops the flagged targets): the run starts over, bit for bit
    plan.set_sliced_seed(7)
    _set_targets(plan, SIZE, 'max', *T.DEFAULT, plan.style_sliced)
    out, epochs = _closure(plan, img)
    assert epochs == [0] * 3 and T._same(out, runs[0])
    # both native steps and the range guard advance it too
    x, m, v, e = T._state(img)
    plan.step(x, m, v, e, 1, 0.02)
    assert plan.sliced_directions(1)[1] == 1
    fwd, bwd = plan.range_guard(img)
    assert not any(fwd) and not any(bwd) and plan.sliced_directions(1)[1] == 2
    plan.loss_and_grad(img)
    assert plan.sliced_directions(1)[1] == 3


def test_resampling_off_two_closures_are_equal_and_two_style_images_blend():
    from style_transfer import _hip as hip
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    plan = _flagged_plan(resample=False, seed=5)
    first, epochs = _closure(plan, img)
    second, again = _closure(plan, img)
    assert epochs == again == [0] * 3 and T._same(first, second)
    # step = closure + update, and an L-BFGS step runs
    xa, ma, va, ea = T._state(img)
    xb, mb, vb, eb = T._state(img)
    for k in (1, 2):
        la = plan.step(xa, ma, va, ea, k, 0.02).clone()
        lb, g = plan.loss_and_grad(xb)
        lb = lb.clone()
        plan.apply_update(xb, g, mb, vb, eb, k, 0.02)
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and torch.equal(xa, xb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(ea, eb), k
    xc, _, _, ec = T._state(img)
    opt = hip.LBFGS(xc)
    for _ in range(2):
        assert torch.isfinite(opt.step(plan, xc, ec, 0.99)).all()
    assert torch.isfinite(xc).all() and not torch.equal(xc, img) and opt.info()['n_iter'] == 2
    assert T._same(first[3:], _closure(plan, img)[0][3:])          # directions and targets: unchanged throughout
    fwd, bwd = plan.range_guard(img)
    assert not any(fwd) and not any(bwd) and plan.sliced_directions(1)[1] == 0
    # two style images, 0.25 / 0.75, and a third of weight 0: the target is the blend of the resampled quantile functions
    a, b = _style_vectors(SIZE, 'max', 20), _style_vectors(SIZE, 'max', 20, (56, 44))
    plan.set_style_sliced_vectors(3, [a.to(DEV), b.to(DEV), (7 * a).to(DEV)], [0.5, 1.5, 0.0])
    r, epoch = plan.sliced_directions(20)
    held = plan.sliced_target(20).cpu().double()
    want = sliced_target_formula(r.cpu().double().numpy(), [a.double().numpy(), b.double().numpy()], [0.25, 0.75], held.shape[1])
    err = float(np.abs(held.numpy() - want).max() / np.abs(want).max())
    print(f'[sliced] two style images 0.25 / 0.75 ({a.shape[1]} and {b.shape[1]} vectors): target max err {err:.2e}')
    assert epoch == 0 and err <= 1e-5
    assert torch.isfinite(plan.loss_and_grad(img)[0]).all()


def test_native_adam_step_moves_the_image_as_the_oracle_gradient_does():
    """One native Adam step against the same update applied to the oracle's float64 gradient under the directions that step used
    (resampling off, so that the judged closure and the step share them)."""
    image = T._inputs(SIZE, 'max')['image']
    img = image.to(DEV)
    plan = _flagged_plan(ALL, resample=False, seed=2)
    failures, (g64, floor) = _judge('steps', plan, img, image, 'max', *T.DEFAULT, (MSE, W2), NONE, NONE, ALL)
    assert not failures, '; '.join(failures)
    xa, ma, va, ea = T._state(img)
    plan.step(xa, ma, va, ea, 1, 0.02)
    want = (image.double() - 0.02 * g64 / (g64.abs() + 1e-8)).clamp(0, 1)
    diff = (xa.cpu().double() - want).abs()
    frac_off = float((diff > 1e-4).double().mean())
    print(f'[sliced] Adam step: max |difference| {float(diff.max()):.2e}, mean {float(diff.mean()):.2e}, {100 * frac_off:.3f}% of pixels off by '
          f'> 1e-4; smallest |g64| {float(g64.abs().min()):.2e}')
    assert float(diff.max()) <= 1e-4


def test_flags_all_false_and_set_then_cleared_are_the_untouched_plan():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    _, plain = K._plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, kinds=None, configure=False)
    want = K._leg(plain, img, steps=True)
    _, zeros = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, None, None, None, NONE, configure=False)
    assert zeros.style_sliced == (False,) * 5
    assert len(want) == 10 and T._same(want, K._leg(zeros, img, steps=True))
    cleared = _flagged_plan(ALL)
    flagged = K._leg(cleared, img, steps=False)
    assert not torch.equal(flagged[0], want[0])
    cleared.set_style_sliced(None)
    assert cleared.style_sliced == (False,) * 5
    T._set_targets(cleared, SIZE, 'max', *T.DEFAULT)
    assert T._same(want, K._leg(cleared, img, steps=True))


def test_a_flagged_head_allocates_no_c_by_c_workspace():
    from style_transfer import _hip as hip
    net = hip.Net(T._weights(), 'max', DEV, 'fp16x3')
    used = {}
    for name, sliced in (('full', NONE), ('deep', DEEP)):
        plan = hip.Plan(net, *SIZE)
        plan.set_style_sliced(sliced)
        _set_targets(plan, SIZE, 'max', *T.DEFAULT, sliced)
        torch.cuda.synchronize()
        used[name] = plan.device_bytes()
    print(f'[sliced] st_plan_device_bytes at 40x48: five full W2 heads {used["full"]}, relu4_1 and relu5_1 sliced {used["deep"]}')
    # (nine 512 x 512 matrices per full head - test_w2_diagonal_gpu - less a sliced head's R and R^T, 512 x 512 each, and its small rows)
    assert used['full'] - used['deep'] >= 2 * 6 * 512 * 512 * 4


# ---- 5. setter semantics ------------------------------------------------------------------------------------------------------
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
    assert plan.style_sliced == (False,) * 5
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    before = K._leg(plan, img, steps=False)
    moments = T._targets(SIZE, 'max', *T.DEFAULT)[1]
    vectors = _style_vectors(SIZE, 'max', 29).to(DEV)
    q = MQ._sorted_rows(T._inputs(SIZE, 'max')['sfeats'][29], torch.float32).to(DEV)
    # refusals carry a message and leave the plan as it was, targets included
    refused(lambda: lib.st_plan_set_style_sliced(plan.handle, _ints(0, 0, 0, 0, 2)), '0 or 1', 'st_plan_set_style_sliced')
    refused(lambda: lib.st_plan_set_style_sliced(plan.handle, _ints(0, -1, 0, 0, 0)), '0 or 1')
    refused(lambda: lib.st_plan_set_sliced_options(plan.handle, 4, 0, 1), 'not flagged', 'st_plan_set_style_sliced')
    with pytest.raises(hip.HipLibraryError, match='not flagged'):
        plan.set_style_sliced_vectors(4, vectors)
    assert T._same(before, K._leg(plan, img, steps=False))
    plan.set_layer_loss_kinds(MSE, ['w2', 'gram', 'w2', 'gram', 'w2'])
    refused(lambda: lib.st_plan_set_style_sliced(plan.handle, _ints(0, 0, 0, 1, 0)), 'gram')
    with pytest.raises(hip.HipLibraryError, match='gram'):
        plan.set_style_sliced(True)
    with pytest.raises(ValueError, match='one per layer'):
        plan.set_style_sliced([True] * 4)
    plan.set_layer_loss_kinds(MSE, W2)
    # diagonal, marginal, nearest and sliced exclude each other, both ways, and each message names the other setter
    plan.set_w2_diagonal([True, False, False, False, False])
    refused(lambda: lib.st_plan_set_style_sliced(plan.handle, _ints(1, 0, 0, 0, 0)), 'st_plan_set_w2_diagonal')
    plan.set_w2_marginal([False, True, False, False, False])
    refused(lambda: lib.st_plan_set_style_sliced(plan.handle, _ints(0, 1, 0, 0, 0)), 'st_plan_set_w2_marginal')
    plan.set_style_nearest([False, False, True, False, False])
    refused(lambda: lib.st_plan_set_style_sliced(plan.handle, _ints(0, 0, 1, 0, 0)), 'st_plan_set_style_nearest')
    plan.set_style_sliced(DEEP)
    assert plan.style_sliced == tuple(DEEP) and plan.w2_diagonal == (True, False, False, False, False)
    assert plan.w2_marginal == (False, True, False, False, False) and plan.style_nearest == (False, False, True, False, False)
    refused(lambda: lib.st_plan_set_w2_diagonal(plan.handle, _ints(0, 0, 0, 0, 1)), 'st_plan_set_style_sliced')
    refused(lambda: lib.st_plan_set_w2_marginal(plan.handle, _ints(0, 0, 0, 1, 0)), 'st_plan_set_style_sliced')
    refused(lambda: lib.st_plan_set_style_nearest(plan.handle, _ints(0, 0, 0, 1, 0)), 'st_plan_set_style_sliced')
    plan.set_w2_diagonal(None)
    plan.set_w2_marginal(None)
    plan.set_style_nearest(None)
    # a custom eps, both ways
    refused(lambda: plan.lib.st_plan_set_loss_eps(plan.handle, None, (ctypes.c_float * 5)(-1, -1, -1, -1, 1e-3)), 'st_plan_set_style_sliced')
    plan.set_style_sliced(None)
    plan.set_loss_eps(None, [None, None, None, None, 1e-3])
    refused(lambda: lib.st_plan_set_style_sliced(plan.handle, _ints(0, 0, 0, 0, 1)), 'st_plan_set_loss_eps')
    plan.set_style_sliced([False, False, False, True, False])
    plan.set_loss_eps(None, None)
    # masks and regions, both ways
    plan.set_style_sliced(DEEP)
    mask = MG.ramp_mask(*SIZE).to(DEV)
    refused(lambda: lib.st_plan_set_style_mask(plan.handle, hip._ptr(mask), None), 'st_plan_set_style_sliced')
    masks = (ctypes.c_void_p * 1)(mask.data_ptr())
    refused(lambda: lib.st_plan_set_style_regions(plan.handle, 1, masks, None), 'st_plan_set_style_sliced')
    plan.set_style_mask(None)
    plan.set_style_regions(None)
    plan.set_style_sliced(None)
    plan.set_style_mask(mask)
    refused(lambda: lib.st_plan_set_style_sliced(plan.handle, _ints(0, 0, 0, 0, 1)), 'st_plan_set_style_mask')
    assert lib.st_plan_set_style_sliced(plan.handle, _ints(0, 0, 0, 0, 0)) == 0
    plan.set_style_mask(None)
    plan.set_style_regions([mask])
    refused(lambda: lib.st_plan_set_style_sliced(plan.handle, _ints(0, 0, 0, 0, 1)), 'st_plan_set_style_regions')
    plan.set_style_regions(None)
    # the options
    plan.set_style_sliced(DEEP)
    for bad in (32, 96, 576, -64):
        refused(lambda: lib.st_plan_set_sliced_options(plan.handle, 4, bad, 1), 'multiple of 64')
    refused(lambda: lib.st_plan_set_sliced_options(plan.handle, 4, 64, 2), '0 or 1')
    refused(lambda: lib.st_plan_set_sliced_options(plan.handle, 5, 64, 1), 'out of range')
    plan.set_style_sliced(None)
    # the targets: dropped by the setter; the other targets' setters refuse a flagged entry and name the right call
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    plan.loss_and_grad(img)
    plan.set_style_sliced(DEEP)
    with pytest.raises(hip.HipLibraryError, match=r'content target 0 \(features\[22\]\)'):
        plan.loss_and_grad(img)
    with pytest.raises(hip.HipLibraryError, match='st_plan_set_style_sliced_vectors'):
        plan.set_style_target(4, moments[29][0].to(DEV), moments[29][1].to(DEV))
    with pytest.raises(hip.HipLibraryError, match='st_plan_set_style_sliced_vectors'):
        plan.set_style_quantiles(4, q)
    with pytest.raises(hip.HipLibraryError, match='st_plan_set_style_sliced_vectors'):
        plan.set_style_vectors(4, vectors)
    with pytest.raises(hip.HipLibraryError, match='not flagged'):
        plan.set_style_sliced_vectors(0, vectors)
    with pytest.raises(hip.HipLibraryError, match='holds no directions'):
        plan.sliced_directions(29)
    with pytest.raises(hip.HipLibraryError, match='holds no target'):
        plan.sliced_target(29)
    with pytest.raises(ValueError, match='style layers'):
        plan.sliced_directions(22)
    with pytest.raises(hip.HipLibraryError, match='weight 0'):
        plan.set_style_sliced_vectors(4, [vectors], [0.0])
    with pytest.raises(hip.HipLibraryError, match='not negative'):
        plan.set_style_sliced_vectors(4, [vectors], [-1.0])
    _set_targets(plan, SIZE, 'max', *T.DEFAULT, DEEP)
    assert torch.isfinite(plan.loss_and_grad(img)[0]).all()
    r, epoch = plan.sliced_directions(29)
    assert r.shape == (512, 512) and epoch == 0 and plan.sliced_target(29).shape == (512, 6)
    # the options drop that entry's target alone; other numbers of directions; a larger and then a smaller style set
    plan.set_sliced_options(4, 128, True)
    with pytest.raises(hip.HipLibraryError, match=r'style target 4 \(features\[29\]\)'):
        plan.loss_and_grad(img)
    bigger = torch.cat([vectors, vectors.flip(1) * 0.5, vectors * 2.0], dim=1).contiguous()
    plan.set_style_sliced_vectors(4, bigger)
    assert torch.isfinite(plan.loss_and_grad(img)[0]).all()
    assert plan.sliced_directions(29)[0].shape == (128, 512) and plan.sliced_target(29).shape == (128, 6)
    grown = plan.device_bytes()
    plan.set_style_sliced_vectors(4, vectors[:, :5].contiguous())
    first = plan.loss_and_grad(img)[0].clone()
    assert torch.isfinite(first).all() and plan.device_bytes() == grown          # (a smaller set allocates nothing)
    # either kinds setter and set_taps clear the flags
    plan.set_loss_kinds('mse', 'w2')
    assert plan.style_sliced == (False,) * 5
    plan.set_style_sliced(ALL)
    plan.set_layer_loss_kinds(MSE, W2)
    assert plan.style_sliced == (False,) * 5
    plan.set_style_sliced(ALL)
    plan.set_taps(*T.CONFIGS['b'])
    assert plan.style_sliced == (False,) * 5
    plan.set_style_sliced(ALL)
    plan.set_taps(*T.DEFAULT)
    assert plan.style_sliced == (False,) * 5
    # back on the default configuration: the fast closure again, equal to a plan that never left it
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    fresh = hip.Plan(net, *SIZE)
    T._set_targets(fresh, SIZE, 'max', *T.DEFAULT)
    assert T._same(K._leg(plan, img, steps=True), K._leg(fresh, img, steps=True))
    # a strip plan takes cleared flags and refuses a set one
    strip = sharding.StripPlan(net, 48, 48, 0, 32)
    refused(lambda: lib.st_plan_set_style_sliced(strip.handle, _ints(0, 0, 0, 0, 1)), 'strip')
    assert lib.st_plan_set_style_sliced(strip.handle, _ints(0, 0, 0, 0, 0)) == 0
    assert lib.st_plan_set_style_sliced(strip.handle, None) == 0


# ---- 6. stylize() -------------------------------------------------------------------------------------------------------------
def test_stylize_reads_style_sliced_and_is_reproducible():
    from style_transfer import StyleTransfer
    st = StyleTransfer(devices=[DEV], pooling='max', weights='synthetic')
    assert st.style_sliced is False and st.style_sliced_resample is True and st.style_sliced_seed == 0
    content_image, style_images = T._pil(81, 64, 48), [T._pil(82, 60, 44), T._pil(83, 52, 40), T._pil(84, 48, 48)]
    weights = [0.75, 0.25, 0.0]                  # the third image is left out of a flagged layer's target
    seen = []

    def callback(it):
        if it.i == 1:
            seen.append((it.w, it.h, it.loss))

    def run(min_scale=64, **kwargs):
        del seen[:]
        out = st.stylize(content_image, style_images, style_weights=weights, end_scale=64, min_scale=min_scale, initial_iterations=4,
                         iterations=4, callback=callback, **kwargs)
        assert out is not None and torch.isfinite(st.get_image_tensor()).all()
        return list(seen), st.get_image_tensor().clone()

    default_loss = run()[0][0][2]
    st.style_sliced, st.style_sliced_samples, st.style_sliced_projections, st.style_sliced_seed = DEEP, 10, 64, 4
    scales, image = run(min_scale=45)                # two scales: the flags, options and seed are set per scale, before the targets
    assert len(scales) == 2 and scales[0][:2] != scales[1][:2]
    assert st._plan.style_sliced == tuple(DEEP) and scales[1][2] != default_loss
    r, epoch = st._plan.sliced_directions(29)
    assert r.shape == (64, 512) and epoch >= 3       # (one epoch per closure of the last scale)
    assert st._plan.sliced_target(20).shape[0] == 64
    again_scales, again = run(min_scale=45)
    assert again_scales == scales and torch.equal(image, again), 'a fixed seed must reproduce the run'
    st.style_sliced_seed = 5
    assert not torch.equal(run(min_scale=45)[1], image)
    # resampling off: the directions of epoch 0 throughout; L-BFGS runs then, and is refused otherwise
    st.style_sliced_resample = False
    run()
    assert st._plan.sliced_directions(29)[1] == 0
    run(optimizer='lbfgs')
    assert st._plan.sliced_directions(29)[1] == 0
    st.style_sliced_resample = True
    with pytest.raises(ValueError, match='style_sliced_resample'):
        run(optimizer='lbfgs')
    del st.style_sliced, st.style_sliced_samples, st.style_sliced_projections, st.style_sliced_seed
    assert run()[0][0][2] == default_loss and st._plan.style_sliced == (False,) * 5
    st.style_sliced = [True, True]
    with pytest.raises(ValueError, match='style_sliced'):
        st.stylize(content_image, style_images[:1], end_scale=64, min_scale=64, initial_iterations=1, iterations=1)
    st.style_sliced, st.style_marginal = DEEP, DEEP
    with pytest.raises(ValueError, match='style_sliced'):
        st.stylize(content_image, style_images[:1], end_scale=64, min_scale=64, initial_iterations=1, iterations=1)
    st.style_sliced, st.style_marginal, st.style_sliced_projections = DEEP, False, 100
    with pytest.raises(ValueError, match='style_sliced_projections'):
        st.stylize(content_image, style_images[:1], end_scale=64, min_scale=64, initial_iterations=1, iterations=1)

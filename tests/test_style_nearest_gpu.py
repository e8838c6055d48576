"""The nearest-neighbour feature-matching option of a W2 style layer (st_plan_set_style_nearest, the st_op_nearest_* entries,
StyleTransfer.style_nearest, losses.StyleLossNearest) on a real MI355X.

Formula (include/st_amd.h), written out in float64 in tests/test_style_nearest_cpu.py and below:
    k*(i) = argmin_k |f_i - s_k|^2, ties: the lowest k;  term = sum_i |f_i - s_k*(i)|^2 / (C N);  dF = (2 / (C N)) (f - s_k*).

How a match is judged.  Where the best and the second best style vector are far apart (planted matches: the gap is about half of
|f_i| max_k |s_k|) and on unrelated random data the indices must EQUAL the float64 arg-min.  Where the arithmetic may legitimately
pick either of two vectors (near-ties) the DEFICIT of the chosen vector is bounded instead,
    deficit_i = d64(i, k_gpu(i)) - min_k d64(i, k),        d64(i, k) = |f_i - s_k|^2 in float64 on the fp32 inputs,
by a bound derived here from the search's arithmetic, not from what it returns.  Names: aF = max |F_ci| and aS = max |S_ck|
(elements), nf_i = |f_i| and nS = max_k |s_k| (vector norms).  The search compares score(i, k) = <f_i, s_k> - |s_k|^2 / 2, and
d = |f_i|^2 - 2 score, so if E_i bounds |computed score - true score| for every k then the chosen vector's true score is at most
2 E_i below the best one's and deficit_i <= 4 E_i.  E_i has four parts:
  * operands.  Each operand is scaled by a power of two so that its bound B (a power of two, max |T| < B <= 2 max |T|:
    profiles/operand_bounds.md, never under and never loose) maps to 2^14, and split into two fp16 planes x0 = fp16(x),
    x1 = fp16(x - x0).  In scaled units ulp(x0) <= 2^3, so |x - x0| <= 2^2 and |x - x0 - x1| <= 2^-10: the represented value is
    off by at most 2^-24 B <= 2^-23 max |T|, and |x1| <= 2^-12 B <= 2^-11 max |T|.  The product f0 s0 + f0 s1 + f1 s0 drops
    f1 s1 <= 2^-22 aF aS.  Per channel the three errors add to 2^-23 + 2^-23 + 2^-22 = 2^-21 times aF aS (second-order terms are
    below 2^-44 and covered by rounding C up to C + 1): (C + 1) 2^-21 aF aS over the C channels.
  * accumulation.  The 3 C products of fp16 values are exact in fp32; each of the 3 C additions rounds by at most 2^-24 of a
    partial sum that is at most sum_c |f_c s_c| <= nf_i nS: 3 C 2^-24 nf_i nS.
  * the bias -|s_k|^2 / 2 is rounded once from double to fp32: 2^-25 nS^2.
  * the final addition of the bias rounds by 2^-24 |score| <= 2^-24 (nf_i nS + nS^2 / 2).
  E_i = (C + 1) 2^-21 aF aS + (3 C + 1) 2^-24 nf_i nS + 2^-24 nS^2, and the bar is deficit_i <= 4 E_i for EVERY pixel, in this
absolute form so that a pixel with f_i = 0 is judged too.  Divided by nf_i nS (the issue's normalisation) it reads
4 ((C + 1) 2^-21 aF aS / (nf_i nS) + (3 C + 1) 2^-24 + 2^-24 nS / nf_i) - of the order of 4 (3 2^-22 + C 2^-24) on Gaussian data,
where aF aS / (nf_i nS) is about 20 / C.  A wrong match has a normalised deficit of order 0.5.  The measured maxima are printed.

Values and gradients are judged against the float64 formula evaluated WITH THE KERNEL'S INDICES, at the project's bars for
standalone operators: 1e-4 on the value, 1e-4 rel-L2 on the gradient.

Plans: inputs and helpers are tests/test_w2_marginal_gpu.py's (and through it test_taps_gpu.py's): sizes 40 x 48 and 45 x 54, the
oracle composed in float64 on the plan's own ReLU and pool decisions with the plan's matches held constant.  Every flagged term
within 1e-4 of float64, every image gradient within 1e-4 rel-L2 of float64; unflagged terms at the bars of their own tests.  A flag
that is ignored cannot pass: the full W2 term of the same tap is shown to lie at least 10 bars from the nearest term.
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

pytestmark = pytest.mark.gpu
DEV = T.DEV
SIZE, ODD = D.SIZE, D.ODD
ALL, DEEP, MSE, W2 = D.ALL, D.DEEP, D.MSE, D.W2
NONE = [False] * 5
IGNORED_BARS = 10
BAR = 1e-4


# ---- the float64 side ---------------------------------------------------------------------------------------------------------
def _distances(f, s, rows=256):
    """(min_k d64, the lowest arg-min, a function k -> d64(i, k(i))) for f [C, N], s [C, M] fp32 on the CPU, in float64."""
    f64, s64 = f.double(), s.double()
    s2 = (s64 * s64).sum(0)
    best, arg = [], []
    for start in range(0, f64.shape[1], rows):
        block = f64[:, start:start + rows]
        d = ((block * block).sum(0)[:, None] - 2.0 * block.T @ s64 + s2[None, :]).clamp(min=0)
        least = d.min(dim=1, keepdim=True).values
        best.append(least[:, 0])
        arg.append(torch.where(d == least, torch.arange(d.shape[1])[None, :], d.shape[1]).min(dim=1).values)

    def at(k):
        r = f64 - s64[:, k]
        return (r * r).sum(0)
    return torch.cat(best), torch.cat(arg), at


def _deficit_bars(f, s):
    """4 E_i of the header for every pixel, and nf_i nS (the issue's normaliser)."""
    c = f.shape[0]
    f64, s64 = f.double(), s.double()
    a_f, a_s = float(f64.abs().max()), float(s64.abs().max())
    nf, n_s = f64.norm(dim=0), float(s64.norm(dim=0).max())
    e = (c + 1) * 2.0 ** -21 * a_f * a_s + (3 * c + 1) * 2.0 ** -24 * nf * n_s + 2.0 ** -24 * n_s * n_s
    return 4.0 * e, nf * n_s


def _check_deficit(tag, f, s, k):
    """The deficit check of the header on every pixel; returns the largest normalised deficit."""
    assert k.dtype == torch.int64 and k.shape == (f.shape[1],) and int(k.min()) >= 0 and int(k.max()) < s.shape[1], tag
    best, _, at = _distances(f, s)
    deficit = at(k) - best
    bars, norm = _deficit_bars(f, s)
    # (d64 itself is a float64 sum: its own rounding, 1e-15 of |f|^2 + |s|^2, is far below every bar)
    slack = 1e-12 * float((f.double() ** 2).sum(0).max() + (s.double() ** 2).sum(0).max())
    worst = float((deficit / norm.clamp(min=1e-300))[norm > 0].max()) if bool((norm > 0).any()) else 0.0
    worst_bar = float((bars / norm.clamp(min=1e-300))[norm > 0].max()) if bool((norm > 0).any()) else 0.0
    print(f'[nearest] {tag}: largest deficit / (|f_i| max|s_k|) {worst:.3e} (largest bar {worst_bar:.3e}), '
          f'largest deficit / its bar {float((deficit / bars.clamp(min=1e-300)).max()):.3e}')
    assert bool((deficit <= bars + slack).all()), f'{tag}: a deficit above 4 E_i: {float((deficit - bars).max()):.3e}'
    return worst


def _formula(f, s, k):
    """(term, dF) at weight 1 in float64 for the matches k."""
    r = f.double() - s.double()[:, k]
    count = f.shape[0] * f.shape[1]
    return float((r * r).sum() / count), 2.0 * r / count


# ---- 1. the standalone search and loss ----------------------------------------------------------------------------------------
def _shapes():
    from style_transfer import _hip as hip
    chunk, tpx, tk = hip.nearest_geometry()
    split = 4 * tk                      # the k range of one split at these pixel counts (st_op_nearest_splits)
    shapes = [(2 * chunk, 1, 1), (2 * chunk, tpx - 1, tk - 1), (2 * chunk, tpx, tk), (2 * chunk, tpx + 1, tk + 1),
              (2 * chunk, 300, 257), (2 * chunk, 130, split - 1), (2 * chunk, 257, split), (2 * chunk, 70, split + 1),
              (2 * chunk, 100, 2 * split), (2 * chunk, 100, 2 * split + 1), (512, 513, 1025), (128, 257, 4099), (512, 1, 1)]
    assert [hip.nearest_splits(n, m) for _, n, m in shapes] == [1, 1, 1, 1, 1, 1, 1, 2, 2, 3, 3, 9, 1]
    return shapes


N_SHAPES = 13


def _gauss(c, n, seed, relu=False):
    x = torch.randn((c, n), generator=torch.Generator().manual_seed(seed))
    return (x.clamp(min=0) if relu else x).contiguous()


def _search(f, s):
    from style_transfer import _hip as hip
    prepared = hip.op_nearest_prepare(s.to(DEV))
    k, score = hip.op_nearest_search(f.to(DEV), prepared, s.shape[1])
    torch.cuda.synchronize()
    return k.cpu(), score.cpu(), prepared


@pytest.mark.parametrize('index', range(N_SHAPES))
def test_planted_matches_are_found_exactly(index):
    c, n, m = _shapes()[index]
    for relu in (False, True):
        g = torch.Generator().manual_seed(1000 + 2 * index + relu)
        s = _gauss(c, m, 2000 + 2 * index + relu, relu)
        perm = torch.randint(0, m, (n,), generator=g)
        f = (s[:, perm] + 1e-3 * torch.randn((c, n), generator=g)).contiguous()
        if relu:
            f = f.clamp(min=0)
        best, arg, at = _distances(f, s)
        if m > 1:       # the data's own property: the planted vector is the float64 arg-min by a gap far above every bar
            assert torch.equal(arg, perm)
        k, score, _ = _search(f, s)
        assert torch.equal(k, perm), f'({c}, {n}, {m}) relu={relu}: {int((k != perm).sum())} of {n} planted matches missed'
        want = (f.double() * s.double()[:, k]).sum(0) - 0.5 * (s.double()[:, k] ** 2).sum(0)
        assert float((score.double() - want).abs().max()) <= float(_deficit_bars(f, s)[0].max()) / 4
        _check_deficit(f'planted ({c}, {n}, {m}) relu={relu}', f, s, k)


@pytest.mark.parametrize('index', range(N_SHAPES))
def test_unrelated_data_and_the_all_zero_tap(index):
    """Checked on the CPU for these seeds: the smallest gap between the best and the second best distance is 5.9e-6 |f_i| max|s_k|
    over all shapes (far above fp32 rounding, far below the worst-case bar), and an emulation of the search's arithmetic - the
    scaled fp16 planes, three fp32 products, the fp32 bias - returns the float64 arg-min on every pixel."""
    c, n, m = _shapes()[index]
    for relu in (False, True):
        f, s = _gauss(c, n, 3000 + 2 * index + relu, relu), _gauss(c, m, 4000 + 2 * index + relu, relu)
        k, _, _ = _search(f, s)
        _, arg, _ = _distances(f, s)
        _check_deficit(f'unrelated ({c}, {n}, {m}) relu={relu}', f, s, k)
        assert torch.equal(k, arg), f'({c}, {n}, {m}) relu={relu}: {int((k != arg).sum())} of {n} matches differ from the float64 arg-min'
    # an all-zero tap: every pixel takes the style vector of the smallest norm
    f, s = torch.zeros((c, n)), _gauss(c, m, 5000 + index)
    k, score, _ = _search(f, s)
    _check_deficit(f'all-zero tap ({c}, {n}, {m})', f, s, k)
    shortest = int((s.double() ** 2).sum(0).argmin())
    assert torch.equal(k, torch.full((n,), shortest)), f'({c}, {n}, {m}): an all-zero tap'
    assert torch.equal(score, torch.full((n,), float((-0.5 * (s.double()[:, shortest] ** 2).sum()).float())))


def test_ties_go_to_the_lowest_index():
    """Bit-identical duplicate columns in one k tile, in different tiles of one split and in different splits (four splits)."""
    from style_transfer import _hip as hip
    c, m = 64, 1600
    assert hip.nearest_splits(200, m) == 4 and hip.nearest_geometry() == (32, 128, 128)
    s = _gauss(c, m, 61)
    groups = [(3, 77), (5, 300), (9, 700, 1500), (130, 131), (600, 1100), (40, 511, 512, 1599)]
    for group in groups:
        for k in group[1:]:
            s[:, k] = s[:, group[0]]
    g = torch.Generator().manual_seed(62)
    owners = torch.tensor([group[i % len(group)] for i, group in enumerate(groups * 34)][:200])
    want = torch.tensor([group[0] for group in (groups * 34)][:200])
    f = (s[:, owners] + 1e-3 * torch.randn((c, 200), generator=g)).contiguous()
    k, _, _ = _search(f, s)
    assert torch.equal(k, want), (k[k != want], want[k != want])
    # every column the same vector: index 0 everywhere, whatever the split
    same = s[:, :1].expand(c, m).contiguous()
    k, _, _ = _search(f, same)
    assert not k.any()


@pytest.mark.parametrize('c, n, m0', [(64, 300, 257), (512, 257, 600), (128, 129, 1400)])
def test_near_ties_stay_under_the_derived_bound(c, n, m0):
    """Columns s_k (1 + 1e-7), s_k (1 - 1e-7), s_k + 1e-7 noise behind the originals: the search may pick either."""
    g = torch.Generator().manual_seed(70 + c)
    base = _gauss(c, m0, 71 + c)
    s = torch.cat([base, base * (1 + 1e-7), base * (1 - 1e-7), base + 1e-7 * torch.randn((c, m0), generator=g),
                   base * (1 + 2.0 ** -22)], dim=1).contiguous()
    perm = torch.randint(0, m0, (n,), generator=g)
    for noise in (1e-3, 0.3):
        f = (base[:, perm] + noise * torch.randn((c, n), generator=g)).contiguous()
        k, _, _ = _search(f, s)
        assert torch.equal(k % m0, perm) or noise > 1e-3
        _check_deficit(f'near-ties ({c}, {n}, {5 * m0}) noise {noise}', f, s, k)


@pytest.mark.parametrize('index', range(N_SHAPES))
def test_value_gradient_determinism_and_the_module(index):
    from style_transfer import _hip as hip
    from style_transfer import losses
    c, n, m = _shapes()[index]
    f = (_gauss(c, n, 80 + index, relu=True) * 1.5 - 0.1).contiguous()
    s = _gauss(c, m, 90 + index, relu=True)
    fd, sd = f.to(DEV), s.to(DEV)
    prepared = hip.op_nearest_prepare(sd)
    prepared2 = hip.op_nearest_prepare(sd)
    loss, unit, k = hip.op_nearest_loss(fd, prepared, m)
    loss2, unit2, k2 = hip.op_nearest_loss(fd, prepared2, m)
    ks, score = hip.op_nearest_search(fd, prepared, m)
    ks2, score2 = hip.op_nearest_search(fd, prepared, m)
    up = torch.tensor(-1.75, device=DEV)
    grad_up = hip.op_nearest_loss_backward(unit, up)
    torch.cuda.synchronize()
    # two calls are equal in bits, indices included, and the loss entry's matches are the search entry's.  (Of the prepared
    # buffer the bias and S^T are compared: of its bound's 32 slots only the largest exponent is ever read.)
    tail = (m + 127) // 128 * 128 * (c + 1)
    assert torch.equal(prepared[-tail:], prepared2[-tail:])
    assert torch.equal(loss, loss2) and torch.equal(unit, unit2) and torch.equal(k, k2)
    assert torch.equal(ks, ks2) and torch.equal(score, score2) and torch.equal(k, ks)
    _check_deficit(f'loss ({c}, {n}, {m})', f, s, k.cpu())
    want, want_grad = _formula(f, s, k.cpu())
    norm = float(want_grad.norm())
    ev = abs(loss.item() - want) / abs(want)
    eg = float((unit.cpu().double() - want_grad).norm()) / norm
    eu = float((grad_up.cpu().double() + 1.75 * want_grad).norm()) / (1.75 * norm)
    print(f'[nearest] operators ({c}, {n}, {m}): value {ev:.2e}, gradient {eg:.2e}, under upstream -1.75 {eu:.2e} (bars 1e-4)')
    assert ev <= BAR and eg <= BAR and eu <= BAR
    # the module: the native path is counted, agrees with its torch path, and native(False) takes torch
    h = 1 if n < 4 or n % 4 else 4
    shape = (c, h, n // h)
    module = losses.StyleLossNearest(sd)
    before = losses.native_calls.get('nearest', 0)
    xn = fd.reshape(shape).clone().requires_grad_()
    value = module(xn)
    (value * 3.5).backward()
    assert losses.native_calls.get('nearest', 0) == before + 1
    assert abs(value.item() - want) / abs(want) <= BAR
    assert rel_l2(xn.grad.cpu().double().reshape(c, n), 3.5 * want_grad) <= BAR
    if index in (4, 9):
        with losses.native(False):
            xt = fd.reshape(shape).clone().requires_grad_()
            value_t = module(xt)
            (value_t * 3.5).backward()
        assert losses.native_calls.get('nearest', 0) == before + 1
        assert abs(value.item() - value_t.item()) / abs(value_t.item()) <= BAR
        assert rel_l2(xn.grad.cpu(), xt.grad.cpu()) <= BAR


def test_the_module_on_the_device():
    from style_transfer import losses
    x = _gauss(64, 120, 21, relu=True).reshape(64, 12, 10).to(DEV)
    style = _gauss(64, 99, 22, relu=True).reshape(1, 64, 9, 11).to(DEV)
    target = losses.StyleLossNearest.get_target(style)
    assert target.shape == (1, 64, 99) and torch.equal(target[0], style[0].flatten(1))
    module = losses.StyleLossNearest(target[0])
    before = losses.native_calls.get('nearest', 0)
    # a batch, float64, a channel count that is no multiple of the K chunk and create_graph are the torch code
    assert torch.isfinite(module(torch.stack([x, x]))) and torch.isfinite(module.double()(x.double()))
    assert torch.isfinite(losses.StyleLossNearest(target[0, :48])(x[:48]))
    module = module.float()
    assert losses.native_calls.get('nearest', 0) == before
    xg = x.clone().requires_grad_()
    (g,) = torch.autograd.grad(module(xg), xg, create_graph=True)
    assert losses.native_calls.get('nearest', 0) == before + 1 and g.requires_grad
    g.pow(2).sum().backward()
    assert torch.isfinite(xg.grad).all()
    # the prepared style set is kept beside the module, not on it: deepcopy and state_dict carry the target alone
    import copy
    assert not [name for name in module.__dict__ if name.startswith('_prep')] and list(module.state_dict()) == ['target']
    twin = copy.deepcopy(module)
    assert torch.equal(twin(x), module(x)) and losses.native_calls.get('nearest', 0) == before + 3
    # at its own vectors the term is at most the search's tolerance (not promised to be exactly 0)
    own = losses.StyleLossNearest(losses.StyleLossNearest.get_target(x))
    v = own(x.clone().requires_grad_())
    bars, _ = _deficit_bars(x.cpu().flatten(1), x.cpu().flatten(1))
    assert 0.0 <= v.item() <= float(bars.sum()) / x.numel()


def test_the_operators_refuse_what_they_cannot_run():
    from style_transfer import _hip as hip
    lib = hip.load_library()
    x = torch.zeros(1 << 16, device=DEV)
    idx = torch.zeros(64, device=DEV, dtype=torch.int32)
    for c, n, m, word in ((48, 4, 4, 'multiple of 32'), (0, 4, 4, 'multiple of 32'), (64, 0, 4, 'at least one'), (64, 4, 0, 'at least one')):
        assert lib.st_op_nearest_search(hip._ptr(x), c, n, hip._ptr(x), m, hip._ptr(x), ctypes.c_void_p(idx.data_ptr()), None, None) != 0
        assert word in lib.st_last_error().decode() and 'st_op_nearest_search' in lib.st_last_error().decode()
    assert lib.st_op_nearest_prepare(hip._ptr(x), 40, 4, hip._ptr(x), None) != 0 and 'st_op_nearest_prepare' in lib.st_last_error().decode()
    assert lib.st_op_nearest_search(None, 64, 4, hip._ptr(x), 4, hip._ptr(x), ctypes.c_void_p(idx.data_ptr()), None, None) != 0


# ---- 2. plans -----------------------------------------------------------------------------------------------------------------
def _style_vectors(size, pooling, layer, style_size=None, samples=None):
    """The style set of a flagged layer as the plan is given it, [C, M] fp32 on the CPU."""
    from style_transfer.style_transfer import _nearest_sample_columns
    tap = MQ._style_feats(size, pooling, style_size)[layer][0].flatten(1)
    columns = _nearest_sample_columns(tap.shape[1], samples)
    return tap[:, torch.tensor(columns)].contiguous()


def _set_targets(plan, size, pooling, content_layers, style_layers, near, marg=None, style_size=None, samples=None):
    ctargets, moments = T._targets(size, pooling, content_layers, style_layers)
    sfeats = MQ._style_feats(size, pooling, None)
    for i, layer in enumerate(content_layers):
        plan.set_content_target(ctargets[layer].to(DEV), i)
    for i, layer in enumerate(style_layers):
        if near[i]:
            plan.set_style_vectors(i, _style_vectors(size, pooling, layer, style_size, samples).to(DEV))
        elif marg and marg[i]:
            plan.set_style_quantiles(i, MQ._sorted_rows(sfeats[layer], torch.float32).to(DEV))
        else:
            plan.set_style_target(i, moments[layer][0].to(DEV), moments[layer][1].to(DEV))


def _plan(size, pooling, precision, content_layers, style_layers, kinds, diag, marg, near, configure=True, style_size=None, samples=None):
    """A plan in the documented order: layers, kinds, diagonal, marginal, nearest, weights, targets."""
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
    if near is not None:
        plan.set_style_nearest(near)
        assert plan.style_nearest == tuple(bool(v) for v in near)
    plan.set_loss_weights(*T._layer_weights(content_layers, style_layers), T.TV_WEIGHT)
    _set_targets(plan, size, pooling, content_layers, style_layers, near or [False] * len(style_layers), marg, style_size, samples)
    return net, plan


def _nearest_term(feat, vectors, k):
    """include/st_amd.h's term of a flagged entry before its weight, the matches k held constant."""
    mat = feat[0].flatten(1)
    return ((mat - vectors[:, k]) ** 2).mean()


def _oracle(image, pooling, decisions, content_layers, style_layers, ctargets, moments, sfeats, sets, matches, weights, kinds, diag, marg,
            near, clevels, tvmap, lap, dtype, others=False):
    """SumLoss in `dtype`: (weighted content terms, weighted style terms, the image-space term, total, gradient and - others - per
    flagged layer the weighted full W2 term of the same tap).  sets / matches: per style layer the style vectors and the plan's
    matches."""
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
        if near[j]:
            sterms.append(_nearest_term(feats[layer], sets[j].to(dtype), matches[j]) * sw)
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
            alt = [float(D._style_term(feats[layer], layer, moments[layer], None, 'w2', False, None, dtype) * sw) if nr else None
                   for layer, sw, nr in zip(style_layers, sws, near)]

    def f(t):
        return float(t.detach())
    return [f(t) for t in cterms], [f(t) for t in sterms], f(space), f(total), grad.detach(), alt


def _judge(tag, plan, img, image, pooling, content_layers, style_layers, kinds, diag, marg, near, lap_pools=None, style_size=None,
           samples=None):
    """One closure of `plan` against the oracle under the plan's OWN maps and matches.  Returns (failures, (the float64 gradient,
    the fp32 composition's rel-L2 from it))."""
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
    sets = [_style_vectors(size, pooling, layer, style_size, samples) if near[j] else None for j, layer in enumerate(style_layers)]
    matches = [plan.nearest_indices(layer).cpu() if near[j] else None for j, layer in enumerate(style_layers)]
    # the matches on the plan's own tap, read back: the deficit check of the header, every pixel
    plan.forward(img, max(content_layers + style_layers))
    for j, layer in enumerate(style_layers):
        if near[j]:
            tap = plan.feature(layer).cpu()[0].flatten(1)
            assert matches[j].shape == (tap.shape[1],)
            _check_deficit(f'{tag} style[{layer}] {tap.shape[1]} pixels against {sets[j].shape[1]} vectors', tap, sets[j], matches[j])
    ctargets, moments = T._targets(size, pooling, content_layers, style_layers)
    args = (image, pooling, decisions, content_layers, style_layers, ctargets, moments, MQ._style_feats(size, pooling, None), sets, matches,
            T._layer_weights(content_layers, style_layers), kinds, diag, marg, near, clevels, tvmap, lap)
    c32, s32, sp32, _, g32, _ = _oracle(*args, torch.float32)
    c64, s64, sp64, _, g64, alt = _oracle(*args, torch.float64, others=True)
    assert len(terms) == nc + ns + 1 and np.isfinite(terms).all() and np.isfinite(losses).all(), f'{tag}: terms {terms}'
    failures = []

    def check(name, got, want32, want64):
        floor = abs(want32 - want64) / abs(want64)
        tol = max(T.TERM_TOL, 3 * floor)
        rel = abs(got - want32) / abs(want32)
        print(f'[nearest] {tag} term {name:24s} got {got:.8g} want {want32:.8g} rel {rel:.2e}  floor {floor:.2e}  bar {tol:.1e}  '
              f'{"PASS" if rel <= tol else "FAIL"}')
        if not rel <= tol:
            failures.append(f'{tag}: term {name} rel {rel:.2e} > {tol:.1e}')
    for i, layer in enumerate(content_layers):
        check(f'content[{layer}]', float(terms[i]), c32[i], c64[i])
    for j, layer in enumerate(style_layers):
        if not near[j]:
            check(f'style[{layer}] {"marginal w2" if marg[j] else "diagonal w2" if diag[j] else kinds[1][j]}', float(terms[nc + j]), s32[j], s64[j])
            continue
        rel = abs(float(terms[nc + j]) - s64[j]) / abs(s64[j])
        print(f'[nearest] {tag} term style[{layer}] nearest      got {float(terms[nc + j]):.8g} float64 {s64[j]:.8g} rel {rel:.2e}  bar {BAR:.0e}  '
              f'{"PASS" if rel <= BAR else "FAIL"}')
        if not rel <= BAR:
            failures.append(f'{tag}: term style[{layer}] nearest rel {rel:.2e} > {BAR:.0e}')
        ratio = abs(alt[j] - s64[j]) / abs(s64[j]) / BAR
        print(f'[nearest] {tag} style[{layer}]: the full W2 term {alt[j]:.6g} is {ratio:.0f} bars from the nearest one {s64[j]:.6g}')
        assert ratio >= IGNORED_BARS, f'{tag}: style[{layer}]: the full W2 term is {ratio:.1f} bars away only'
    check('image-space (tv, laplacian)', float(terms[-1]), sp32, sp64)
    want_total = np.float32(0)
    for t in terms.astype(np.float32):
        want_total = np.float32(want_total + t)
    rel_total = abs(float(losses[7]) - float(want_total)) / abs(float(want_total))
    print(f'[nearest] {tag} total {losses[7]:.8g} vs fp32 sum of the terms {want_total:.8g} rel {rel_total:.2e} (bar {T.SUM_TOL:.0e})')
    if not rel_total <= T.SUM_TOL:
        failures.append(f'{tag}: total rel {rel_total:.2e} > {T.SUM_TOL:.0e}')
    assert torch.isfinite(grad).all(), f'{tag}: non-finite gradient'
    err, floor = rel_l2(grad.cpu(), g64), rel_l2(g32, g64)
    print(f'[nearest] {tag} gradient hip-vs-fp64 {err:.2e}  ref-fp32 floor {floor:.2e}  bar {BAR:.0e}  {"PASS" if err <= BAR else "FAIL"}')
    if not err <= BAR:
        failures.append(f'{tag}: gradient rel-L2 {err:.2e} > {BAR:.0e} (fp32 composition: {floor:.2e})')
    return failures, (g64, floor)


CASES = [
    # name, size, pooling, precision, (content layers, style layers), style kinds, diagonal, marginal, nearest, configure, style size, samples
    ('all-five', SIZE, 'max', 'fp16x3', T.DEFAULT, W2, NONE, NONE, ALL, False, None, None),
    ('all-five-odd-fp32', ODD, 'max', 'fp32', T.DEFAULT, W2, NONE, NONE, ALL, False, None, None),
    ('all-five-average', SIZE, 'average', 'fp16x3', T.DEFAULT, W2, NONE, NONE, ALL, False, None, None),
    ('all-five-style-56x44', SIZE, 'max', 'fp16x3', T.DEFAULT, W2, NONE, NONE, ALL, False, (56, 44), None),
    ('all-five-400-samples', SIZE, 'max', 'fp16x3', T.DEFAULT, W2, NONE, NONE, ALL, False, None, 400),
    ('deep-two-odd', ODD, 'max', 'fp16x3', T.DEFAULT, W2, NONE, NONE, DEEP, False, None, None),
    ('deep-two-fp32-average', SIZE, 'average', 'fp32', T.DEFAULT, W2, NONE, NONE, DEEP, False, None, None),
    ('with-gram-diagonal-and-marginal', SIZE, 'max', 'fp16x3', T.DEFAULT, ['w2', 'gram', 'w2', 'w2', 'w2'], [True, False, False, False, False],
     [False, False, True, False, False], [False, False, False, True, True], False, None, None),
    ('list-d-average', SIZE, 'average', 'fp16x3', T.CONFIGS['d'], ['w2'] * 3, [False] * 3, [False] * 3, [True] * 3, True, None, None),
    ('list-e-odd', ODD, 'max', 'fp16x3', T.CONFIGS['e'], ['w2'] * 4, [False] * 4, [False] * 4, [True, False, True, True], True, None, None),
    ('a-layer-in-both-lists', SIZE, 'max', 'fp16x3', T.CONFIGS['b'], W2, NONE, NONE, DEEP, True, None, None),
]


@pytest.mark.parametrize('name, size, pooling, precision, lists, style_kinds, diag, marg, near, configure, style_size, samples', CASES,
                         ids=[c[0] for c in CASES])
def test_configurations(name, size, pooling, precision, lists, style_kinds, diag, marg, near, configure, style_size, samples):
    content_layers, style_layers = lists
    kinds = (['mse'] * len(content_layers), style_kinds)
    image = T._inputs(size, pooling)['image']
    img = image.to(DEV)
    _, plan = _plan(size, pooling, precision, content_layers, style_layers, None if style_kinds == W2[:len(style_kinds)] else kinds,
                    diag, marg, near, configure, style_size, samples)
    tag = f'({name}) style {style_layers} flags {[int(f) for f in near]} {size[0]}x{size[1]}-{pooling}-{precision}'
    failures, _ = _judge(tag, plan, img, image, pooling, content_layers, style_layers, kinds, diag, marg, near, style_size=style_size,
                         samples=samples)
    if configure:
        L._configured_array(plan.term_losses().cpu().double().numpy(), plan.loss_and_grad(img)[0].cpu().numpy(), len(content_layers),
                            len(style_layers))
    assert not failures, '; '.join(failures)


def test_both_maps_and_the_laplacian():
    near = [True, False, True, False, True]
    image = T._inputs(SIZE, 'max')['image']
    _, plan = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, None, None, None, near, configure=False)
    plan.set_content_mask(MG.ramp_mask(*SIZE).to(DEV))
    plan.set_tv_mask(MG.binary_mask(*SIZE).to(DEV))
    plan.set_laplacian(LG._content(SIZE).to(DEV), (4, 16), LG.LAP_WEIGHT)
    failures, _ = _judge('content map + TV map + Laplacian, flags 1,0,1,0,1', plan, image.to(DEV), image, 'max', *T.DEFAULT,
                         (MSE, W2), NONE, NONE, near, lap_pools=(4, 16))
    assert not failures, '; '.join(failures)


# ---- 3. bits and steps --------------------------------------------------------------------------------------------------------
def _flagged_plan(near=(True, False, False, True, True)):
    return _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, None, None, None, list(near), configure=False)[1]


def test_two_closures_are_equal_step_is_closure_plus_update_and_the_range_guard_runs():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    plan = _flagged_plan()
    first = [t.clone() for t in plan.loss_and_grad(img)] + [plan.term_losses().clone()] + [plan.nearest_indices(layer) for layer in (1, 20, 29)]
    second = [t.clone() for t in plan.loss_and_grad(img)] + [plan.term_losses().clone()] + [plan.nearest_indices(layer) for layer in (1, 20, 29)]
    torch.cuda.synchronize()
    assert T._same(first, second) and all(torch.isfinite(t).all() for t in first[:3])
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
    """One native Adam step and one native L-BFGS step against the same update applied to the oracle's float64 gradient, held as
    tests/test_w2_marginal_gpu.py holds them: Adam's first step is lr sign(g) in effect, so the bulk of the image is judged - fewer
    than 0.2 % of the pixels off by more than 1e-4, a mean difference below 1e-4; L-BFGS's first step is -t g with one scalar t, and
    the displacement against t times the float64 gradient is judged in rel-L2 at the gradient's own bar."""
    from style_transfer import _hip as hip
    image = T._inputs(SIZE, 'max')['image']
    img = image.to(DEV)
    plan = _flagged_plan(ALL)
    failures, (g64, floor) = _judge('steps', plan, img, image, 'max', *T.DEFAULT, (MSE, W2), NONE, NONE, ALL)
    assert not failures, '; '.join(failures)
    xa, ma, va, ea = T._state(img)
    plan.step(xa, ma, va, ea, 1, 0.02)
    want = (image.double() - 0.02 * g64 / (g64.abs() + 1e-8)).clamp(0, 1)
    diff = (xa.cpu().double() - want).abs()
    frac_off = float((diff > 1e-4).double().mean())
    print(f'[nearest] Adam step: mean |difference| {float(diff.mean()):.2e}, {100 * frac_off:.3f}% of pixels off by > 1e-4')
    assert frac_off < 2e-3 and float(diff.mean()) < 1e-4
    xb, _, _, eb = T._state(img)
    opt = hip.LBFGS(xb)
    opt.step(plan, xb, eb, 0.99)
    moved = (xb.cpu().double() - image.double())
    inside = (xb.cpu() > 0) & (xb.cpu() < 1)                   # (clamped pixels aside)
    t = float((moved[inside] * g64[inside]).sum() / (g64[inside] ** 2).sum())
    err = float(torch.linalg.norm(moved[inside] - t * g64[inside]) / torch.linalg.norm(t * g64[inside]))
    print(f'[nearest] L-BFGS step: t {t:.4g}, displacement against t x the float64 gradient rel-L2 {err:.2e} (bar {T.bar(floor):.1e})')
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
    _, zeros = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, None, None, None, NONE, configure=False)
    assert zeros.style_nearest == (False,) * 5
    assert len(want) == 10 and T._same(want, K._leg(zeros, img, steps=True))
    cleared = _flagged_plan(ALL)
    flagged = K._leg(cleared, img, steps=False)
    assert not torch.equal(flagged[0], want[0])
    cleared.set_style_nearest(None)
    assert cleared.style_nearest == (False,) * 5
    T._set_targets(cleared, SIZE, 'max', *T.DEFAULT)
    assert T._same(want, K._leg(cleared, img, steps=True))


def test_a_flagged_head_allocates_no_c_by_c_workspace():
    from style_transfer import _hip as hip
    net = hip.Net(T._weights(), 'max', DEV, 'fp16x3')
    used = {}
    for name, near in (('full', NONE), ('deep', DEEP)):
        plan = hip.Plan(net, *SIZE)
        plan.set_style_nearest(near)
        _set_targets(plan, SIZE, 'max', *T.DEFAULT, near)
        torch.cuda.synchronize()
        used[name] = plan.device_bytes()
    print(f'[nearest] st_plan_device_bytes at 40x48: five full W2 heads {used["full"]}, relu4_1 and relu5_1 nearest {used["deep"]}')
    # (nine 512 x 512 matrices per full head - test_w2_diagonal_gpu - less a nearest head's S^T of 128 rows and its scratch)
    assert used['full'] - used['deep'] >= 2 * 8 * 512 * 512 * 4


# ---- 4. setter semantics ------------------------------------------------------------------------------------------------------
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
    assert plan.style_nearest == (False,) * 5
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    before = K._leg(plan, img, steps=False)
    moments = T._targets(SIZE, 'max', *T.DEFAULT)[1]
    vectors = _style_vectors(SIZE, 'max', 29).to(DEV)
    q = MQ._sorted_rows(T._inputs(SIZE, 'max')['sfeats'][29], torch.float32).to(DEV)
    # refusals carry a message and leave the plan as it was, targets included
    refused(lambda: lib.st_plan_set_style_nearest(plan.handle, _ints(0, 0, 0, 0, 2)), '0 or 1', 'st_plan_set_style_nearest')
    refused(lambda: lib.st_plan_set_style_nearest(plan.handle, _ints(0, -1, 0, 0, 0)), '0 or 1')
    refused(lambda: lib.st_plan_set_style_vectors(plan.handle, 4, hip._ptr(vectors), vectors.shape[1], None), 'not flagged')
    assert T._same(before, K._leg(plan, img, steps=False))
    plan.set_layer_loss_kinds(MSE, ['w2', 'gram', 'w2', 'gram', 'w2'])
    refused(lambda: lib.st_plan_set_style_nearest(plan.handle, _ints(0, 0, 0, 1, 0)), 'gram')
    with pytest.raises(hip.HipLibraryError, match='gram'):
        plan.set_style_nearest(True)
    with pytest.raises(ValueError, match='one per layer'):
        plan.set_style_nearest([True] * 4)
    plan.set_layer_loss_kinds(MSE, W2)
    # diagonal, marginal and nearest exclude each other, both ways
    plan.set_w2_diagonal([True, False, False, False, False])
    refused(lambda: lib.st_plan_set_style_nearest(plan.handle, _ints(1, 0, 0, 0, 0)), 'diagonal')
    plan.set_w2_marginal([False, True, False, False, False])
    refused(lambda: lib.st_plan_set_style_nearest(plan.handle, _ints(0, 1, 0, 0, 0)), 'marginal')
    plan.set_style_nearest(DEEP)
    assert plan.style_nearest == tuple(DEEP) and plan.w2_diagonal == (True, False, False, False, False)
    assert plan.w2_marginal == (False, True, False, False, False)
    refused(lambda: lib.st_plan_set_w2_diagonal(plan.handle, _ints(0, 0, 0, 0, 1)), 'nearest')
    refused(lambda: lib.st_plan_set_w2_marginal(plan.handle, _ints(0, 0, 0, 1, 0)), 'nearest')
    plan.set_w2_diagonal(None)
    plan.set_w2_marginal(None)
    # a custom eps, both ways
    refused(lambda: plan.lib.st_plan_set_loss_eps(plan.handle, None, (ctypes.c_float * 5)(-1, -1, -1, -1, 1e-3)), 'nearest')
    plan.set_style_nearest(None)
    plan.set_loss_eps(None, [None, None, None, None, 1e-3])
    refused(lambda: lib.st_plan_set_style_nearest(plan.handle, _ints(0, 0, 0, 0, 1)), 'eps')
    plan.set_style_nearest([False, False, False, True, False])
    plan.set_loss_eps(None, None)
    # masks and regions, both ways
    plan.set_style_nearest(DEEP)
    mask = MG.ramp_mask(*SIZE).to(DEV)
    refused(lambda: lib.st_plan_set_style_mask(plan.handle, hip._ptr(mask), None), 'nearest')
    masks = (ctypes.c_void_p * 1)(mask.data_ptr())
    refused(lambda: lib.st_plan_set_style_regions(plan.handle, 1, masks, None), 'nearest')
    plan.set_style_mask(None)
    plan.set_style_regions(None)
    plan.set_style_nearest(None)
    plan.set_style_mask(mask)
    refused(lambda: lib.st_plan_set_style_nearest(plan.handle, _ints(0, 0, 0, 0, 1)), 'style mask')
    assert lib.st_plan_set_style_nearest(plan.handle, _ints(0, 0, 0, 0, 0)) == 0
    plan.set_style_mask(None)
    plan.set_style_regions([mask])
    refused(lambda: lib.st_plan_set_style_nearest(plan.handle, _ints(0, 0, 0, 0, 1)), 'regions')
    plan.set_style_regions(None)
    # the targets: dropped by the setter; the other targets' setters refuse a flagged entry and name the right call
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    plan.loss_and_grad(img)
    plan.set_style_nearest(DEEP)
    with pytest.raises(hip.HipLibraryError, match=r'content target 0 \(features\[22\]\)'):
        plan.loss_and_grad(img)
    with pytest.raises(hip.HipLibraryError, match='st_plan_set_style_vectors'):
        plan.set_style_target(4, moments[29][0].to(DEV), moments[29][1].to(DEV))
    with pytest.raises(hip.HipLibraryError, match='st_plan_set_style_vectors'):
        plan.set_style_quantiles(4, q)
    with pytest.raises(hip.HipLibraryError, match='not flagged'):
        plan.set_style_vectors(0, vectors)
    with pytest.raises(hip.HipLibraryError, match='holds no matches'):
        plan.nearest_indices(29)
    with pytest.raises(ValueError, match='style layers'):
        plan.nearest_indices(22)
    refused(lambda: lib.st_plan_set_style_vectors(plan.handle, 4, hip._ptr(vectors), 0, None), 'at least one')
    _set_targets(plan, SIZE, 'max', *T.DEFAULT, DEEP)
    assert torch.isfinite(plan.loss_and_grad(img)[0]).all()
    k = plan.nearest_indices(29)
    assert k.shape == (6,) and k.dtype == torch.int64 and int(k.min()) >= 0 and int(k.max()) < vectors.shape[1]
    # a larger and then a smaller style set on the same entry
    bigger = torch.cat([vectors, vectors.flip(1) * 0.5, vectors * 2.0], dim=1).contiguous()
    plan.set_style_vectors(4, bigger)
    plan.loss_and_grad(img)
    tap = plan.feature(29).cpu()[0].flatten(1)
    _check_deficit('a larger style set', tap, bigger.cpu(), plan.nearest_indices(29).cpu())
    plan.set_style_vectors(4, vectors[:, :5].contiguous())
    plan.loss_and_grad(img)
    _check_deficit('a smaller style set', tap, vectors[:, :5].cpu(), plan.nearest_indices(29).cpu())
    # a set of 257 k tiles (52 splits at 6 pixels), then one of 256 (64 splits): the smaller set needs the larger scratch
    assert (hip.nearest_splits(6, 257 * 128), hip.nearest_splits(6, 256 * 128)) == (52, 64)
    wide = torch.randn((512, 257 * 128), generator=torch.Generator().manual_seed(5)).clamp(min=0) * float(tap.abs().max())
    for m in (257 * 128, 256 * 128, 257 * 128):
        plan.set_style_vectors(4, wide[:, :m].contiguous().to(DEV))
        first = plan.loss_and_grad(img)[0].clone()
        k_first = plan.nearest_indices(29)
        second = plan.loss_and_grad(img)[0].clone()
        torch.cuda.synchronize()
        assert torch.isfinite(first).all() and torch.equal(first, second) and torch.equal(k_first, plan.nearest_indices(29))
        _check_deficit(f'{m} style vectors, {hip.nearest_splits(6, m)} splits', tap, wide[:, :m].contiguous(), k_first.cpu())
    grown = plan.device_bytes()
    plan.set_style_vectors(4, vectors)
    assert plan.device_bytes() == grown                      # (a smaller set allocates nothing)
    # a refused set leaves the entry as it was: the former set and its count
    refused(lambda: lib.st_plan_set_style_vectors(plan.handle, 4, hip._ptr(vectors), 0, None), 'at least one')
    assert torch.isfinite(plan.loss_and_grad(img)[0]).all()
    # either kinds setter and set_taps clear the flags
    plan.set_loss_kinds('mse', 'w2')
    assert plan.style_nearest == (False,) * 5
    plan.set_style_nearest(ALL)
    plan.set_layer_loss_kinds(MSE, W2)
    assert plan.style_nearest == (False,) * 5
    plan.set_style_nearest(ALL)
    plan.set_taps(*T.CONFIGS['b'])
    assert plan.style_nearest == (False,) * 5
    plan.set_style_nearest(ALL)
    plan.set_taps(*T.DEFAULT)
    assert plan.style_nearest == (False,) * 5
    # back on the default configuration: the fast closure again, equal to a plan that never left it
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    fresh = hip.Plan(net, *SIZE)
    T._set_targets(fresh, SIZE, 'max', *T.DEFAULT)
    assert T._same(K._leg(plan, img, steps=True), K._leg(fresh, img, steps=True))
    # a strip plan takes cleared flags and refuses a set one
    strip = sharding.StripPlan(net, 48, 48, 0, 32)
    refused(lambda: lib.st_plan_set_style_nearest(strip.handle, _ints(0, 0, 0, 0, 1)), 'strip')
    assert lib.st_plan_set_style_nearest(strip.handle, _ints(0, 0, 0, 0, 0)) == 0
    assert lib.st_plan_set_style_nearest(strip.handle, None) == 0


# ---- 5. stylize() -------------------------------------------------------------------------------------------------------------
def test_stylize_reads_style_nearest():
    from PIL import Image
    from style_transfer import StyleTransfer
    from style_transfer.style_transfer import _nearest_sample_columns, size_to_fit, to_tensor
    st = StyleTransfer(devices=[DEV], pooling='max', weights='synthetic')
    assert st.style_nearest is False and st.style_nearest_samples is None
    content_image, style_images = T._pil(81, 64, 48), [T._pil(82, 60, 44), T._pil(83, 52, 40), T._pil(84, 48, 48)]
    weights = [0.75, 0.25, 0.0]                  # the third image is dropped from a flagged layer's set
    seen = []

    def callback(it):
        if it.i == 1:
            seen.append((it.w, it.h, it.loss))

    def run(min_scale=64):
        del seen[:]
        out = st.stylize(content_image, style_images, style_weights=weights, end_scale=64, min_scale=min_scale, initial_iterations=4,
                         iterations=4, callback=callback)
        assert out is not None and torch.isfinite(st.get_image_tensor()).all()
        return list(seen)

    default_loss = run()[0][2]
    st.style_nearest, st.style_nearest_samples = DEEP, 10
    scales = run(min_scale=45)                       # two scales: the flags are set per scale, before the targets
    assert len(scales) == 2 and scales[0][:2] != scales[1][:2]
    assert st._plan.style_nearest == tuple(DEEP)
    assert scales[1][2] != default_loss
    # the final closure: the plan's terms on the final image against the oracle's, on the union of the first two images' sampled
    # vectors in image order and with the plan's matches
    w, h = scales[1][:2]
    assert (w, h) == size_to_fit(content_image.size, 64, scale_up=True)
    content = to_tensor(content_image.resize((w, h), Image.BICUBIC))[None]
    with torch.no_grad():
        cfeats = O.vgg_features(content, T._weights(), st.content_layers, 'max')
        per_image = []
        for image in style_images:
            sw_, sh_ = size_to_fit(image.size, 64)
            per_image.append(O.vgg_features(to_tensor(image.resize((sw_, sh_), Image.BICUBIC))[None], T._weights(), st.style_layers, 'max'))
    moments = {}
    for layer in st.style_layers:
        each = [O.feature_moments(feats[layer]) for feats in per_image]
        moments[layer] = tuple(sum(wt * m[i] for wt, m in zip(weights, each)) for i in (0, 1))
    sets = []
    for j, layer in enumerate(st.style_layers):
        taps = [feats[layer][0].flatten(1) for feats, wt in zip(per_image, weights) if wt != 0]
        sets.append(torch.cat([tap[:, torch.tensor(_nearest_sample_columns(tap.shape[1], 10))] for tap in taps], dim=1) if DEEP[j] else None)
    assert sets[3].shape[1] == 20 and sets[4].shape[1] <= 20
    final = st.image.detach().clone()
    st._plan.loss_and_grad(final)
    torch.cuda.synchronize()
    got = st._plan.term_losses().cpu().numpy()
    matches = [st._plan.nearest_indices(layer).cpu() if DEEP[j] else None for j, layer in enumerate(st.style_layers)]
    for j in (3, 4):
        assert int(matches[j].max()) < sets[j].shape[1]
    args = (final.cpu(), 'max', None, st.content_layers, st.style_layers, cfeats, moments, None, sets, matches, ([0.015], st.style_weights),
            (MSE, W2), NONE, NONE, DEEP, None, None, None)
    c32, s32, sp32 = _oracle(*args, torch.float32)[:3]
    c64, s64, sp64 = _oracle(*args, torch.float64)[:3]
    assert len(got) == 7
    for name, value, want32, want64 in zip(['content'] + [f'style[{layer}]' for layer in st.style_layers] + ['tv'], got, c32 + s32 + [sp32],
                                           c64 + s64 + [sp64]):
        bar = max(T.TERM_TOL, 3 * abs(want32 - want64) / abs(want64))
        rel_term = abs(float(value) - want32) / abs(want32)
        print(f'[nearest] stylize final closure {name}: got {float(value):.8g} want {want32:.8g} rel {rel_term:.2e} bar {bar:.1e}')
        assert rel_term <= bar, f'final closure, {name}: rel {rel_term:.2e} > {bar:.1e}'
    del st.style_nearest, st.style_nearest_samples
    assert run()[0][2] == default_loss and st._plan.style_nearest == (False,) * 5
    st.style_nearest = [True, True]
    with pytest.raises(ValueError, match='style_nearest'):
        st.stylize(content_image, style_images[:1], end_scale=64, min_scale=64, initial_iterations=1, iterations=1)
    st.style_nearest, st.style_marginal = DEEP, DEEP
    with pytest.raises(ValueError, match='style_nearest'):
        st.stylize(content_image, style_images[:1], end_scale=64, min_scale=64, initial_iterations=1, iterations=1)
    st.style_nearest, st.style_marginal, st.style_nearest_samples = DEEP, False, 0
    with pytest.raises(ValueError, match='style_nearest_samples'):
        st.stylize(content_image, style_images[:1], end_scale=64, min_scale=64, initial_iterations=1, iterations=1)

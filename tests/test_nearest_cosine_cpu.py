"""Cosine and centred-cosine matching of a nearest head, the parts that need no GPU: the module's torch formula
(losses.StyleLossNearest(target, metric)) against the formula of include/st_amd.h written out here with an explicit N x M matrix in
float64, gradcheck, the tie rule, the resolver of StyleTransfer.style_nearest_metric, the command line, and the header."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO

EPS = 1e-8
METRICS = ('cosine', 'centered_cosine')


def cosine_formula(f, s, metric):
    """(k*, term, dF, the size of dF's two parts) at weight 1 for f [C, N] and s [C, M], float64, straight from include/st_amd.h:
    the explicit N x M matrix p_i(k) = <f_i - mu, s^_k>, its first maximum per row, and the match and mu constants of the
    gradient.  dF is the difference of two parts of size 1 / (N r_i) each, which cancel where the cosine is near 1: rounding is
    judged against that size."""
    mu = s.mean(1) if metric == 'centered_cosine' else torch.zeros_like(s[:, 0])
    d = s - mu[:, None]
    unit = d / torch.sqrt((d * d).sum(0) + EPS)
    g = f - mu[:, None]
    p = g.T @ unit                                                  # [N, M]
    k = torch.tensor([int(torch.nonzero(row == row.max())[0]) for row in p])
    r = torch.sqrt((g * g).sum(0) + EPS)
    best = p[torch.arange(f.shape[1]), k]
    n = f.shape[1]
    return k, float((1.0 - best / r).sum() / n), (-unit[:, k] / r + best * g / r ** 3) / n, float((1.0 / r).max()) / n


@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('shape, m', [((3, 4, 5), 17), ((3, 4, 5), 1), ((4, 1, 1), 9), ((2, 3, 4, 5), 7), ((1, 1, 1), 1), ((5, 6, 7), 50)])
def test_module_torch_formula_against_the_explicit_matrix(shape, m, metric):
    from style_transfer import losses
    g = torch.Generator().manual_seed(21)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    c = shape[-3]
    x.reshape(-1, c, x.shape[-2] * x.shape[-1])[0, :, 0] = 0        # a zero tap pixel
    target = torch.randn((c, m), generator=g, dtype=torch.float64).clamp(min=-0.3)
    if m > 2:
        target[:, 1] = 0                                            # a zero style vector
    module = losses.StyleLossNearest(target, metric)
    assert module.metric == metric and list(module.state_dict()) == ['target']
    module.chunk = 7                 # several blocks of pixels, the last one short
    xr = x.clone().requires_grad_()
    value = module(xr)
    value.backward()
    batch = x.reshape((-1,) + shape[-3:])
    wants = [cosine_formula(b.reshape(c, -1), target, metric) for b in batch]
    want = sum(w[1] for w in wants) / len(wants)
    want_grad = torch.stack([w[2] for w in wants]).reshape(shape) / len(wants)
    assert abs(value.item() - want) <= 1e-12 * max(abs(want), 1e-30)
    assert float((xr.grad - want_grad).abs().max()) <= 1e-12 * max(w[3] for w in wants) / len(wants)
    assert 0.0 <= value.item() <= 2.0
    mu, unit = module.cosine_parts(torch.float64)
    got_k = losses.StyleLossNearest.match_cosine(x.flatten(-2) - mu[:, None], unit, chunk=7).reshape(len(batch), -1)
    for b, w in enumerate(wants):
        assert torch.equal(got_k[b], w[0])
    if metric == 'cosine':
        assert not mu.any()
        if m > 2:
            assert not unit[:, 1].any()                             # a zero vector stays zero


def test_a_tie_goes_to_the_lowest_index_and_the_zero_pixel():
    from style_transfer import losses
    g = torch.Generator().manual_seed(22)
    s = torch.randn((6, 12), generator=g, dtype=torch.float64)
    s[:, 9] = s[:, 2]
    s[:, 5] = s[:, 2]
    s[:, 11] = s[:, 4]
    for metric in METRICS:
        module = losses.StyleLossNearest(s, metric)
        mu, unit = module.cosine_parts(torch.float64)
        f = torch.stack([mu + 0.05 * (s[:, 9] - mu), mu + 3.0 * (s[:, 11] - mu), mu + 0.5 * (s[:, 0] - mu), mu], dim=1)
        k = losses.StyleLossNearest.match_cosine(f - mu[:, None], unit)
        want = cosine_formula(f, s, metric)[0]
        # a scaled copy matches its own vector whatever its length; every score equal (the pixel that equals mu): the first vector
        assert k.tolist() == [2, 4, 0, 0] and torch.equal(k, want)
        xr = f.reshape(6, 2, 2).clone().requires_grad_()
        value = module(xr)
        value.backward()
        # three pixels of cosine 1 and one of cosine 0; at that one the gradient is -(1 / N) s^_0 / sqrt(eps)
        assert abs(value.item() - 0.25) <= 1e-6
        assert torch.allclose(xr.grad.reshape(6, 4)[:, 3], -unit[:, 0] / (4 * EPS ** 0.5), rtol=1e-12, atol=0)


@pytest.mark.parametrize('metric', METRICS)
def test_gradcheck_on_well_separated_data(metric):
    from style_transfer import losses
    g = torch.Generator().manual_seed(23)
    s = torch.randn((5, 9), generator=g, dtype=torch.float64)
    perm = torch.tensor([0, 3, 8, 8, 2, 5])
    noise = 0.2 * torch.randn((2, 5, 6), generator=g, dtype=torch.float64)
    x = ((s.mean(1)[:, None] + 0.3 * (s[:, perm] - s.mean(1)[:, None]))[None] + noise).reshape(2, 5, 2, 3)
    module = losses.StyleLossNearest(s, metric)
    assert torch.autograd.gradcheck(module, (x.clone().requires_grad_(),), eps=1e-6, atol=1e-7)
    xr = x.clone().requires_grad_()
    (first,) = torch.autograd.grad(module(xr), xr, create_graph=True)
    assert first.requires_grad                                       # create_graph goes through torch


def test_the_module_refuses_and_the_default_is_unchanged():
    from style_transfer import _hip, losses
    assert _hip.NEAREST_METRICS == ('l2', 'cosine', 'centered_cosine')
    target = torch.randn((4, 6), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    for bad in ('cos', 'L2', '', None, 1):
        with pytest.raises(ValueError, match='metric'):
            losses.StyleLossNearest(target, bad)
    with pytest.raises(ValueError, match='columns'):
        losses.StyleLossNearest(torch.zeros(3), 'cosine')
    x = torch.randn((4, 3, 3), generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    plain, named = losses.StyleLossNearest(target), losses.StyleLossNearest(target, metric='l2')
    assert plain.metric == 'l2' and torch.equal(plain(x), named(x))
    k = losses.StyleLossNearest.match(x.flatten(-2), target)
    assert torch.equal(plain(x), ((x.flatten(-2) - target[:, k]) ** 2).mean())
    # float32 and half the channels on the CPU: the torch path serves any dtype
    assert torch.isfinite(losses.StyleLossNearest(target.float(), 'centered_cosine')(x.float()))


def test_resolver_refusals():
    from style_transfer.style_transfer import StyleTransfer, _resolve_style_nearest_metric as resolve
    assert StyleTransfer.style_nearest_metric == 'l2'
    deep = [False, False, False, True, True]
    assert resolve('l2', deep) == ['l2'] * 5 and resolve('l2', [False] * 5, world=4) == ['l2'] * 5
    assert resolve('cosine', deep) == ['l2', 'l2', 'l2', 'cosine', 'cosine']
    assert resolve('centered_cosine', [True] * 2) == ['centered_cosine'] * 2
    assert resolve('cosine', [False] * 3) == ['l2'] * 3                      # nothing flagged: nothing to apply it to
    assert resolve(['l2', 'l2', 'l2', 'l2', 'centered_cosine'], deep) == ['l2', 'l2', 'l2', 'l2', 'centered_cosine']
    assert resolve(('l2', 'cosine'), [True, True]) == ['l2', 'cosine']
    assert resolve(['l2'] * 5, deep, world=2) == ['l2'] * 5
    for bad, flags, kwargs, word in (
            ('cos', deep, {}, "one of ('l2', 'cosine', 'centered_cosine')"),
            ('', deep, {}, 'one of'),
            (None, deep, {}, 'one name per entry'),
            (1, deep, {}, 'one name per entry'),
            (True, deep, {}, 'one name per entry'),
            (['cosine'] * 4, deep, {}, '4 names for 5 layers'),
            (['l2', 'l2', 'l2', 'cosine', 'euclid'], deep, {}, "'euclid'"),
            (['l2', 'l2', 'l2', 'cosine', 2], deep, {}, 'is none of'),
            (['cosine', 'l2', 'l2', 'cosine', 'cosine'], deep, {}, 'layer 0 is not flagged in style_nearest'),
            (['l2', 'l2', 'centered_cosine', 'l2', 'l2'], deep, {}, 'layer 2 is not flagged'),
            ('cosine', deep, dict(world=2), '2 ranks'),
            (['l2', 'l2', 'l2', 'l2', 'centered_cosine'], deep, dict(world=4), '4 ranks')):
        with pytest.raises(ValueError, match='style_nearest_metric') as info:
            resolve(bad, flags, **kwargs)
        assert word in str(info.value), (bad, str(info.value))


def test_cli_parsing():
    from style_transfer import cli
    parser = cli.build_parser()
    base = ['content.jpg', 'style.jpg']
    assert parser.parse_args(base).style_nearest_metric == 'l2'
    assert parser.parse_args(base + ['--style-nearest-metric', 'cosine']).style_nearest_metric == 'cosine'
    assert parser.parse_args(base + ['--style-nearest-metric', 'centered_cosine']).style_nearest_metric == 'centered_cosine'
    assert parser.parse_args(base + ['--style-nearest-metric', 'l2,l2,l2,cosine,centered_cosine']).style_nearest_metric == \
        ['l2', 'l2', 'l2', 'cosine', 'centered_cosine']
    for bad in ('cos', 'cosine,', 'l2,,cosine', '', '1'):
        with pytest.raises(SystemExit):
            parser.parse_args(base + ['--style-nearest-metric', bad])

    class Holder:
        pass
    st = cli.apply_loss_kinds(Holder(), parser.parse_args(base + ['--style-nearest', '0,1', '--style-nearest-metric', 'l2,cosine']))
    assert st.style_nearest == [False, True] and st.style_nearest_metric == ['l2', 'cosine']
    assert cli.apply_loss_kinds(Holder(), parser.parse_args(base)).style_nearest_metric == 'l2'


def test_the_symbols_are_in_the_header_and_the_binding():
    from style_transfer import _hip
    text = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    lib = _hip.load_library(require_gpu=False)
    for name in ('st_plan_set_nearest_metric', 'st_plan_nearest_metric', 'st_op_nearest_cosine_prepared_floats',
                 'st_op_nearest_cosine_scratch_floats', 'st_op_nearest_cosine_prepare', 'st_op_nearest_cosine_loss'):
        assert f'{name}(' in text, name
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for phrase in ('eps = 1e-8', 'k*(i)  = argmax_k p_i(k) = argmax_k (<f_i, s^_k> + b_k),   ties: the lowest k',
                   'term_j = w_j sum_i (1 - p_i(k*(i)) / r_i) / N', 'dF_ci  = (w_j / N) (-s^_c,k*(i) / r_i + p_i(k*(i)) g_ci / r_i^3)',
                   'nearest, nearest metric, sliced (flags, options, seed)', "0 'l2'", "1 'cosine'", "2 'centered_cosine'"):
        assert phrase in text, phrase
    assert 'The matching is L2, not cosine' not in text.replace('\n * ', ' ')
    assert lib.st_abi_version() == 2
    # sizes: the cosine buffers are L2's plus the centre, and the L2 sizes are where they were
    for c, m in ((64, 1), (64, 129), (512, 4099)):
        assert lib.st_op_nearest_cosine_prepared_floats(c, m) == lib.st_op_nearest_prepared_floats(c, m) + (c + 63) // 64 * 64
        assert lib.st_op_nearest_cosine_scratch_floats(c, 300, m) == lib.st_op_nearest_scratch_floats(c, 300, m)
    assert hasattr(_hip.Plan, 'set_nearest_metric') and isinstance(_hip.Plan.nearest_metric, property)
    assert callable(_hip.op_nearest_cosine_prepare) and callable(_hip.op_nearest_cosine_loss)

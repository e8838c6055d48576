"""The exact per-channel Wasserstein (sorted) option of a W2 style layer, the parts that need no GPU: the resolver of
StyleTransfer.style_marginal, the command line, the module's torch formula (losses.StyleLossW2Marginal) against the formula of
include/st_amd.h written out here in float64, the resample's numbers by hand, and the header."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO

W2 = ['w2'] * 5


def resample_formula(q, n):
    """include/st_amd.h: T_i = lerp(Q, u), u = clamp((i + 1/2) n_q / N - 1/2, 0, n_q - 1); q [..., n_q] float64 numpy."""
    n_q = q.shape[-1]
    out = np.empty(q.shape[:-1] + (n,), dtype=np.float64)
    for i in range(n):
        u = min(max((i + 0.5) * n_q / n - 0.5, 0.0), n_q - 1.0)
        lo = int(np.floor(u))
        hi = min(lo + 1, n_q - 1)
        out[..., i] = q[..., lo] + (u - lo) * (q[..., hi] - q[..., lo])
    return out


def marginal_formula(x, q):
    """(term, dF) at weight 1 for x [C, N] and the target's quantile functions q [C, n_q], float64 numpy: the stable ascending
    order of every row, ties by index, and the permutation a constant of the gradient."""
    c, n = x.shape
    target = resample_formula(q, n)
    order = np.argsort(x + 0.0, axis=1, kind='stable')
    d = np.take_along_axis(x, order, 1) - target
    grad = np.zeros_like(x)
    np.put_along_axis(grad, order, 2.0 * d / (c * n), 1)
    return float((d * d).sum() / (c * n)), grad


def test_resample_numbers_by_hand():
    from style_transfer.losses import StyleLossW2Marginal as M
    q = torch.tensor([[0.0, 3.0, 9.0]], dtype=torch.float64)
    # three order statistics sit at 1/6, 1/2, 5/6; six midpoints at 1/12 ... 11/12 -> u = -0.25 (clamped), 0.25, 0.75, 1.25, 1.75, 2.25 (clamped)
    six = M.resample(q, 6)
    assert torch.allclose(six, torch.tensor([[0.0, 0.75, 2.25, 4.5, 7.5, 9.0]], dtype=torch.float64), rtol=0, atol=1e-15)
    # two midpoints at 1/4 and 3/4 -> u = 0.25 and 1.75
    two = M.resample(q, 2)
    assert torch.allclose(two, torch.tensor([[0.75, 7.5]], dtype=torch.float64), rtol=0, atol=1e-15)
    assert M.resample(q, 3) is q
    assert np.array_equal(resample_formula(q.numpy(), 6), six.numpy()) and np.array_equal(resample_formula(q.numpy(), 2), two.numpy())
    assert np.array_equal(resample_formula(q.numpy(), 3), q.numpy())
    g = torch.Generator().manual_seed(3)
    big = torch.sort(torch.randn((4, 37), generator=g, dtype=torch.float64), dim=1).values
    for n in (1, 5, 36, 37, 38, 200):
        got = M.resample(big, n)
        assert np.allclose(got.numpy(), resample_formula(big.numpy(), n), rtol=0, atol=1e-15)
        assert bool((got[:, 1:] >= got[:, :-1]).all())
    # fp32 quantiles: u stays in float64, the lerp is fp32
    got32 = M.resample(big.float(), 200)
    assert got32.dtype == torch.float32
    assert np.abs(got32.double().numpy() - resample_formula(big.float().double().numpy(), 200)).max() <= 1e-6 * float(big.abs().max())


@pytest.mark.parametrize('shape, n_q', [((3, 4, 5), 20), ((3, 4, 5), 33), ((2, 3, 4, 5), 7), ((1, 1, 1), 1), ((5, 6, 7), 42)])
def test_module_torch_formula_against_the_formula_written_out(shape, n_q):
    from style_transfer import losses
    g = torch.Generator().manual_seed(11)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    x = torch.where(torch.rand(shape, generator=g) < 0.4, torch.zeros_like(x), x)       # ties: exact zeros, as behind a ReLU
    c = shape[-3]
    style = torch.randn((c, n_q), generator=g, dtype=torch.float64).clamp(min=-0.3)
    q = losses.StyleLossW2Marginal.get_target(style.reshape(c, 1, n_q))
    assert q.shape == (c, n_q) and torch.equal(q, torch.sort(style, dim=1).values)
    module = losses.StyleLossW2Marginal(q)
    xr = x.clone().requires_grad_()
    value = module(xr)
    value.backward()
    batch = x.reshape((-1,) + shape[-3:])
    wants = [marginal_formula(b.reshape(c, -1).numpy(), q.numpy()) for b in batch]
    want = sum(w[0] for w in wants) / len(wants)
    want_grad = np.stack([w[1] for w in wants]).reshape(shape) / len(wants)
    assert abs(value.item() - want) <= 1e-13 * max(abs(want), 1e-30)
    assert np.abs(xr.grad.numpy() - want_grad).max() <= 1e-13 * np.abs(want_grad).max()


def test_module_is_exactly_zero_at_its_own_target():
    from style_transfer import losses
    g = torch.Generator().manual_seed(12)
    for dtype in (torch.float32, torch.float64):
        x = torch.randn((6, 7, 9), generator=g).clamp(min=0).to(dtype)
        x[0, 0, :3] = -0.0
        module = losses.StyleLossW2Marginal(losses.StyleLossW2Marginal.get_target(x))
        assert 'target' in dict(module.named_buffers())
        xr = x.clone().requires_grad_()
        value = module(xr)
        value.backward()
        assert value.item() == 0.0 and not xr.grad.any()
    with pytest.raises(ValueError, match='sorted'):
        losses.StyleLossW2Marginal(torch.zeros(3))


def test_resolver_refusals():
    from style_transfer.style_transfer import StyleTransfer, _resolve_style_marginal as resolve
    assert StyleTransfer.style_marginal is False
    assert resolve(False, W2) == [False] * 5 and resolve(True, W2) == [True] * 5
    assert resolve(True, ['w2', 'gram', 'w2']) == [True, False, True]
    assert resolve(True, W2, [True, False, False, False, False]) == [False, True, True, True, True]
    assert resolve([False, False, False, True, True], W2) == [False, False, False, True, True]
    assert resolve((0, 1, np.bool_(True)), ['w2'] * 3) == [False, True, True]
    for bad, kinds, kwargs, word in (
            ([True] * 4, W2, {}, '4 flags for 5 layers'),
            ([True, 'yes', False, False, False], W2, {}, 'is not a bool'),
            ([False, 2, False, False, False], W2, {}, 'is not a bool'),
            ('1,1', W2, {}, 'one bool per entry'),
            (1.0, W2, {}, 'one bool per entry'),
            ([False, True, False], ['w2', 'gram', 'w2'], {}, "'gram'"),
            ([True, False, False, False, False], W2, dict(style_diagonal=[True, False, False, False, False]), 'style_diagonal'),
            ([False, False, False, True, False], W2, dict(style_eps=[None, None, None, 1e-3, None]), 'style_eps'),
            (True, W2, dict(style_eps=[None, None, None, 1e-3, None]), 'style_eps'),
            ([False, False, False, False, True], W2, dict(masked=True), 'style_mask'),
            (True, W2, dict(masked=True), 'style_regions'),
            (True, W2, dict(masked=True), 'style_image_masks'),
            (True, W2, dict(world=2), '2 ranks'),
            ([False, False, False, False, True], W2, dict(world=4), '4 ranks')):
        with pytest.raises(ValueError, match='style_marginal') as info:
            resolve(bad, kinds, **kwargs)
        assert word in str(info.value), (bad, str(info.value))
    # no set flag: nothing to refuse
    assert resolve(False, W2, masked=True, world=4, style_eps=[1e-3] * 5) == [False] * 5
    assert resolve([False] * 5, ['gram'] * 5, masked=True) == [False] * 5


def test_cli_parsing():
    from style_transfer import cli
    parser = cli.build_parser()
    base = ['content.jpg', 'style.jpg']
    assert parser.parse_args(base).style_marginal is False
    assert parser.parse_args(base + ['--style-marginal', '1']).style_marginal is True
    assert parser.parse_args(base + ['--style-marginal', '0']).style_marginal is False
    assert parser.parse_args(base + ['--style-marginal', '0,0,0,1,1']).style_marginal == [False, False, False, True, True]
    for bad in ('2', 'yes', '1,,0', ''):
        with pytest.raises(SystemExit):
            parser.parse_args(base + ['--style-marginal', bad])

    class Holder:
        pass
    st = cli.apply_loss_kinds(Holder(), parser.parse_args(base + ['--style-marginal', '0,1', '--style-diagonal', '1,0']))
    assert st.style_marginal == [False, True] and st.style_diagonal == [True, False]


def test_the_symbols_are_in_the_header_and_the_binding():
    from style_transfer import _hip
    text = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    lib = _hip.load_library(require_gpu=False)
    for name in ('st_op_sort_chunk', 'st_op_sort_scratch_bytes', 'st_op_channel_sort', 'st_op_resample_quantiles',
                 'st_op_w2_marginal_loss', 'st_op_w2_marginal_loss_backward', 'st_plan_set_w2_marginal', 'st_plan_w2_marginal',
                 'st_plan_set_style_quantiles', 'st_plan_style_quantiles'):
        assert f'{name}(' in text, name
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for phrase in ('torch.sort(f + 0.0, stable=True)', 'u = clamp((i + 1/2) n_q / N - 1/2, 0, n_q - 1)', 'There is no\n * eps',
                   'Order of configuration: layers, kinds, eps, diagonal, marginal, weights, then the targets'):
        assert phrase in text, phrase
    assert _hip.STYLE_LOSSES == ('w2', 'gram')
    chunk = lib.st_op_sort_chunk()
    assert chunk in (4096, 8192)
    # two buffers of 64-bit keys behind a header, and nothing for an empty shape
    assert lib.st_op_sort_scratch_bytes(3, 1000) >= 2 * 3 * 1000 * 8 and lib.st_op_sort_scratch_bytes(0, 5) == 0
    for attr in ('set_w2_marginal', 'w2_marginal', 'quantiles', 'set_style_quantiles'):
        assert hasattr(_hip.Plan, attr), attr
    for attr in ('op_channel_sort', 'op_resample_quantiles', 'op_w2_marginal_loss', 'op_w2_marginal_loss_backward', 'sort_chunk'):
        assert hasattr(_hip, attr), attr

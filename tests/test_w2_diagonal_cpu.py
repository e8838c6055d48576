"""CPU checks of the diagonal-covariance W2 style heads (st_plan_set_w2_diagonal, the st_op_channel_* / st_op_w2_diag_* entries,
StyleTransfer.style_diagonal, --style-diagonal, losses.StyleLossW2Diag): the header declares the entries and the library
exports them, the up-front validation (`_resolve_style_diagonal`) accepts and refuses what it should, stylize() refuses the
same before any device work, the CLI flag reaches the attribute, and the module's torch path computes the formula that
include/st_amd.h fixes - written out below in float64 - on any dtype and batch.  No GPU needed."""
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import REPO
from test_loss_kinds_cpu import _bare_style_transfer, _lib

NEW_ENTRIES = ['st_plan_set_w2_diagonal', 'st_plan_w2_diagonal', 'st_op_channel_moments', 'st_op_w2_diag_loss',
               'st_op_w2_diag_loss_backward']
W2 = ['w2'] * 5
MIXED = ['w2', 'w2', 'w2', 'gram', 'gram']


def _resolve(style_diagonal, style_loss=W2, world=1):
    from style_transfer.style_transfer import _resolve_style_diagonal
    return _resolve_style_diagonal(style_diagonal, style_loss, world)


def test_header_declares_and_library_exports_the_entries():
    header = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    hip, lib = _lib()
    for name in NEW_ENTRIES:
        assert re.search(r'\bint\s+%s\s*\(' % name, text), f'{name} is not declared in st_amd.h'
        assert hasattr(lib, name), f'{name} is not exported by libst_amd.so'
        assert name in hip.EXPORTED_SYMBOLS, f'{name} is not bound by _hip._declare'
    assert re.search(r'\blong long\s+st_op_channel_stats_scratch_floats\s*\(', text)
    assert 'st_op_channel_stats_scratch_floats' in hip.EXPORTED_SYMBOLS
    # an option of a w2 layer: no third kind name, no kind code 2
    assert hip.STYLE_LOSSES == ('w2', 'gram')
    for name in ('set_w2_diagonal', 'w2_diagonal'):
        assert hasattr(hip.Plan, name), name
    # the scratch: 16 bytes of ticket and two partials per channel and split; the smallest taps take one split
    assert lib.st_op_channel_stats_scratch_floats(512, 6) == 4 + 2 * 512
    assert lib.st_op_channel_stats_scratch_floats(1, 1) == 6
    many = lib.st_op_channel_stats_scratch_floats(64, 208 * 208)
    assert (many - 4) % (2 * 64) == 0 and (many - 4) // (2 * 64) > 4
    assert lib.st_op_channel_stats_scratch_floats(0, 5) == 0


@pytest.mark.parametrize('world', [1, 2, 8])
def test_the_default_passes_for_any_world_size(world):
    assert _resolve(False, world=world) == [False] * 5
    assert _resolve([False] * 5, world=world) == [False] * 5
    assert _resolve((0, 0, 0, 0, 0), world=world) == [False] * 5
    assert _resolve(False, MIXED, world=world) == [False] * 5


def test_bools_lists_and_tuples():
    assert _resolve(True) == [True] * 5
    assert _resolve(True, MIXED) == [True, True, True, False, False]        # a bool: every w2 layer
    assert _resolve(True, ['gram'] * 5) == [False] * 5
    assert _resolve([False, False, False, True, True]) == [False, False, False, True, True]
    assert _resolve((True, False, True, False, False), MIXED) == [True, False, True, False, False]
    assert _resolve([np.bool_(True), 0, 1], ['w2'] * 3) == [True, False, True]
    assert _resolve([], []) == [] and _resolve(True, []) == []


@pytest.mark.parametrize('given, kinds', [
    ([True], W2), ([False] * 6, W2), ([], W2), ((True, True), MIXED), ('1,1,1,1,1', W2), (None, W2), (1.0, W2),
    ([True, 2, False, False, False], W2), ([False, False, False, 'yes', False], W2),
    ([False, False, False, True, False], MIXED), ([True] * 5, MIXED),
])
def test_a_bad_value_is_refused_naming_the_attribute(given, kinds):
    with pytest.raises(ValueError, match='style_diagonal'):
        _resolve(given, kinds)


@pytest.mark.parametrize('given', [True, [False, False, False, False, True]])
def test_a_set_flag_is_refused_on_several_ranks(given):
    assert any(_resolve(given, world=1))
    with pytest.raises(ValueError, match='style_diagonal.*strips'):
        _resolve(given, world=2)


def test_stylize_refuses_before_any_device_work():
    from style_transfer import StyleTransfer
    assert StyleTransfer.style_diagonal is False                          # a class attribute
    st = _bare_style_transfer(['cuda:0', 'cuda:1'])
    assert st.style_diagonal is False
    st.style_diagonal = [False, False, False, True, True]
    with pytest.raises(ValueError, match='style_diagonal.*strips'):
        st.stylize(None, [None])
    st = _bare_style_transfer(['cuda:0'])
    st.style_diagonal = [True, True]
    with pytest.raises(ValueError, match='style_diagonal'):
        st.stylize(None, [None])
    st.style_loss, st.style_diagonal = MIXED, [False, False, False, True, False]
    with pytest.raises(ValueError, match="style_diagonal.*'gram'"):
        st.stylize(None, [None])
    assert 'style_diagonal' not in StyleTransfer.stylize.__kwdefaults__ and len(StyleTransfer.stylize.__kwdefaults__) == 14


def test_cli_flag_parses_and_lands_on_the_attribute():
    from style_transfer import cli
    parser = cli.build_parser()
    st = cli.apply_loss_kinds(types.SimpleNamespace(), parser.parse_args(['content.png', 'style.png']))
    assert st.style_diagonal is False
    args = parser.parse_args(['content.png', 'style.png', '--style-diagonal', '0,0,0,1,1'])
    st = cli.apply_loss_kinds(_bare_style_transfer(['cuda:0']), args)
    assert st.style_diagonal == [False, False, False, True, True]
    assert _resolve(st.style_diagonal) == [False, False, False, True, True]
    assert parser.parse_args(['content.png', 'style.png', '--style-diagonal', '1']).style_diagonal is True
    assert parser.parse_args(['content.png', 'style.png', '--style-diagonal', '0']).style_diagonal is False
    for bad in (['--style-diagonal', 'yes'], ['--style-diagonal', '0,1,'], ['--style-diagonal', '2'], ['--style-diagonal', '0,x']):
        with pytest.raises(SystemExit):
            parser.parse_args(['content.png', 'style.png', *bad])


# ---- the module's torch path against the formula of include/st_amd.h in float64 ------------------------------------------------
def formula64(x, mean_t, std_t, eps):
    """(term, dF) at weight 1 and without a mask for x [C, N], all float64 numpy."""
    c, n = x.shape
    mu = x.sum(1) / n
    q = (x * x).sum(1) / n
    sigma = np.sqrt(np.maximum(q - mu * mu, 0.0) + eps)
    term = (((mu - mean_t) ** 2).sum() + ((sigma - std_t) ** 2).sum()) / c
    g = np.where(sigma > 0, (1.0 - std_t / np.where(sigma > 0, sigma, 1.0)) / c, 0.0)
    grad = ((2.0 / c) * (mu - mean_t)[:, None] + 2.0 * g[:, None] * (x - mu[:, None])) / n
    return term, grad


def target64(t, eps):
    c, n = t.shape
    mu = t.sum(1) / n
    q = (t * t).sum(1) / n
    return mu, np.sqrt(np.maximum(q - mu * mu, 0.0) + eps)


def _inputs(kind, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(c, h, w, generator=g, dtype=torch.float64) * (0.5 + torch.rand(c, 1, 1, generator=g, dtype=torch.float64)) + \
        torch.randn(c, 1, 1, generator=g, dtype=torch.float64)
    if kind == 'relu':
        x = x.clamp(min=0)
        if c > 2:
            x[c // 2] = 0                       # a dead channel
    if kind == 'zeros':
        x = torch.zeros_like(x)
    return x


CASES = [('signed', 1, 5, 7), ('signed', 3, 5, 7), ('signed', 64, 9, 6), ('relu', 3, 4, 4), ('relu', 64, 7, 5), ('zeros', 3, 4, 5),
         ('signed', 3, 1, 1), ('relu', 64, 1, 1), ('zeros', 1, 1, 1)]


@pytest.mark.parametrize('kind, c, h, w', CASES)
@pytest.mark.parametrize('eps', [1e-4, 1e-2])
def test_torch_path_matches_the_formula(kind, c, h, w, eps):
    from style_transfer import losses
    x64 = _inputs(kind, c, h, w, 11 + c)
    t64 = _inputs('signed' if kind == 'zeros' else kind, c, h + 1, w + 2, 97 + c)
    mean_t, std_t = target64(t64.reshape(c, -1).numpy(), eps)
    want, want_grad = formula64(x64.reshape(c, -1).numpy(), mean_t, std_t, eps)
    for dtype, rtol in ((torch.float64, 1e-11), (torch.float32, 2e-5)):
        module = losses.StyleLossW2Diag(losses.StyleLossW2Diag.get_target(t64.to(dtype)), eps)
        assert module.mean.shape == (c,) and module.std.shape == (c,) and module.mean.dtype == dtype
        np.testing.assert_allclose(module.std.double().numpy(), std_t, rtol=rtol * 10, atol=0)
        x = x64.to(dtype).clone().requires_grad_()
        loss = module(x)
        loss.backward()
        assert loss.shape == () and loss.dtype == dtype
        assert abs(loss.item() - want) <= rtol * 10 * abs(want), (dtype, loss.item(), want)
        err = np.linalg.norm(x.grad.double().numpy().reshape(c, -1) - want_grad) / max(np.linalg.norm(want_grad), 1e-300)
        assert err <= rtol * 50, (dtype, err)


def test_a_batch_is_the_mean_over_its_images():
    from style_transfer import losses
    c, eps = 3, 1e-4
    t64 = _inputs('signed', c, 6, 5, 3)
    xs = [_inputs('signed', c, 4, 6, 20 + i) for i in range(3)]
    mean_t, std_t = target64(t64.reshape(c, -1).numpy(), eps)
    module = losses.StyleLossW2Diag(losses.StyleLossW2Diag.get_target(t64), eps)
    x = torch.stack(xs).requires_grad_()
    loss = module(x)
    loss.backward()
    parts = [formula64(v.reshape(c, -1).numpy(), mean_t, std_t, eps) for v in xs]
    assert abs(loss.item() - np.mean([p[0] for p in parts])) <= 1e-12 * loss.item()
    for i, (_, grad) in enumerate(parts):
        np.testing.assert_allclose(x.grad[i].reshape(c, -1).numpy(), grad / 3, rtol=1e-9, atol=1e-15)


def test_a_full_second_moment_serves_as_the_target_and_targets_blend():
    from style_transfer import losses
    a, b = _inputs('relu', 3, 5, 4, 1).float(), _inputs('relu', 3, 6, 7, 2).float()
    full = losses.StyleLossW2._get_target_torch(a)                        # (mean [C], srm [C, C])
    diag = losses.StyleLossW2Diag.get_target(a)                           # (mean [C], srm's diagonal [C])
    assert diag[1].shape == (3,) and full[1].shape == (3, 3)
    x = _inputs('relu', 3, 4, 4, 5).float()
    one, two = losses.StyleLossW2Diag(full)(x), losses.StyleLossW2Diag(diag)(x)
    assert abs(one.item() - two.item()) <= 1e-6 * abs(two.item())
    # linear in the image's statistics: the blend of two targets is the target of the blended statistics
    ta, tb = losses.StyleLossW2Diag.get_target(a.double()), losses.StyleLossW2Diag.get_target(b.double())
    blend = tuple(0.25 * u + 0.75 * v for u, v in zip(ta, tb))
    module = losses.StyleLossW2Diag(blend, eps=1e-3)
    np.testing.assert_allclose(module.std.numpy(), np.sqrt(np.maximum(blend[1].numpy() - blend[0].numpy() ** 2, 0) + 1e-3), rtol=1e-12)
    with pytest.raises(ValueError):
        losses.StyleLossW2Diag((ta[0], torch.zeros(4)))


@pytest.mark.parametrize('kind, c, h, w', CASES)
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_the_targets_own_features_give_exactly_zero(kind, c, h, w, dtype):
    from style_transfer import losses
    x = _inputs(kind, c, h, w, 5).to(dtype).requires_grad_()
    for eps in (1e-4, 0.0):
        module = losses.StyleLossW2Diag(losses.StyleLossW2Diag.get_target(x.detach()), eps)
        x.grad = None
        loss = module(x)
        loss.backward()
        assert loss.item() == 0.0
        assert torch.count_nonzero(x.grad).item() == 0 and torch.isfinite(x.grad).all()


def test_a_zero_sigma_has_a_zero_gradient_through_it():
    from style_transfer import losses
    # eps = 0 and a constant channel: sigma = 0, g = 0; the mean term's gradient stays
    t = _inputs('signed', 2, 3, 3, 9)
    module = losses.StyleLossW2Diag(losses.StyleLossW2Diag.get_target(t), eps=0.0)
    x = torch.ones(2, 3, 3, dtype=torch.float64).requires_grad_()
    module(x).backward()
    want = (2.0 / 2) * (1.0 - module.mean) / 9
    np.testing.assert_allclose(x.grad.numpy(), want[:, None, None].expand(2, 3, 3).numpy(), rtol=1e-12)


def test_equals_style_loss_w2_on_exactly_uncorrelated_channels():
    """The tensor: channel c is  b_c + a_c * (row c + 1 of the 8 x 8 Hadamard matrix)  over N = 8 pixels, a_c and b_c dyadic
    rationals.  The Hadamard rows are +-1, mutually orthogonal and orthogonal to the constant row 0, so every channel's mean is
    b_c exactly and every cross-covariance a_c a_d <row, row> / 8 is exactly 0 in float64: the covariance is diagonal by
    construction, and the full W2 of such Gaussians IS the diagonal one.  The bar is the fp32 floor of the comparison, measured
    here as each module's own deviation from its float64 run."""
    from style_transfer import losses
    had = torch.tensor([[1.0]], dtype=torch.float64)
    for _ in range(3):
        had = torch.cat([torch.cat([had, had], 1), torch.cat([had, -had], 1)], 0)
    c = 7

    def build(amps, offsets):
        a = torch.tensor(amps, dtype=torch.float64)[:, None]
        b = torch.tensor(offsets, dtype=torch.float64)[:, None]
        return (b + a * had[1:]).reshape(c, 2, 4)
    x64 = build([1.0, 1.25, 1.5, 0.75, 1.125, 0.875, 1.375], [0.5, -0.25, 1.0, 0.0, 0.75, -0.5, 0.125])
    t64 = build([1.5, 0.75, 1.0, 1.25, 0.875, 1.375, 1.125], [0.25, 0.5, -0.75, 1.0, 0.0, 0.625, -0.125])
    mean, srm = losses.StyleLossW2._get_target_torch(x64)
    cov = losses.StyleLossW2.srm_to_cov(mean, srm)
    assert torch.count_nonzero(cov - torch.diag(torch.diagonal(cov))).item() == 0        # exactly diagonal
    values = {}
    with losses.native(False):
        for dtype in (torch.float64, torch.float32):
            target = losses.StyleLossW2._get_target_torch(t64.to(dtype))
            x = x64.to(dtype)
            values[dtype] = (losses.StyleLossW2(target)(x).item(), losses.StyleLossW2Diag(target)(x).item())
    full64, diag64 = values[torch.float64]
    full32, diag32 = values[torch.float32]
    assert diag64 > 1e-3
    assert abs(full64 - diag64) <= 1e-9 * diag64, (full64, diag64)         # the same number, up to the Newton-Schulz iteration
    floor = abs(full32 - full64) + abs(diag32 - diag64)
    print(f'full fp32 {full32:.9g} fp64 {full64:.12g}; diagonal fp32 {diag32:.9g} fp64 {diag64:.12g}; floor {floor:.3g}')
    assert abs(full32 - diag32) <= floor + 1e-9 * diag64, (full32, diag32, floor)

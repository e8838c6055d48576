"""The sliced Wasserstein option of a W2 style layer, the parts that need no GPU: the module's torch formula
(losses.StyleLossSliced) against the float64 formula written out here, the resolver of StyleTransfer.style_sliced and its
options, the command line, and the header."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO

W2 = ['w2'] * 5


def resample_formula(q, n):
    """q [P, n_q] (sorted rows) at n midpoints, float64 numpy, straight from include/st_amd.h: order statistic k sits at
    (k + 1/2) / n_q, linear in between, clamped at the ends; n_q == n is the identity."""
    n_q = q.shape[1]
    if n_q == n:
        return q.copy()
    u = np.clip((np.arange(n, dtype=np.float64) + 0.5) * n_q / n - 0.5, 0.0, n_q - 1.0)
    i0 = np.floor(u).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_q - 1)
    t = u - i0
    return q[:, i0] + t * (q[:, i1] - q[:, i0])


def sliced_target_formula(r, styles, weights, n):
    """T [P, n] = sum_i a_i resample_n(sort_rows(R S_i)), a_i = w_i / sum w, images of weight 0 left out; float64 numpy."""
    total = float(sum(weights))
    t = np.zeros((r.shape[0], n))
    for s, w in zip(styles, weights):
        if w != 0:
            t += (w / total) * resample_formula(np.sort(r @ s + 0.0, axis=1, kind='stable'), n)
    return t


def sliced_formula(f, r, t):
    """(term, dF) at weight 1 for f [C, N], r [P, C], t [P, N], float64 numpy, straight from include/st_amd.h: Y = R F, the stable
    ascending order of every row of Y + 0.0 (ties by pixel index), G through the permutation, dF = (2 / (P N)) R^T G."""
    p, n = r.shape[0], f.shape[1]
    y = r @ f
    order = np.argsort(y + 0.0, axis=1, kind='stable')
    g = np.zeros_like(y)
    rows = np.arange(p)[:, None]
    g[rows, order] = np.take_along_axis(y, order, axis=1) - t
    return float((g * g).sum() / (p * n)), (2.0 / (p * n)) * (r.T @ g)


def unit_rows(p, c, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.randn((p, c), generator=g, dtype=torch.float64)
    return r / r.norm(dim=1, keepdim=True)


@pytest.mark.parametrize('shape, m, p', [((3, 4, 5), 20, 7), ((3, 4, 5), 1, 3), ((4, 1, 1), 9, 4), ((2, 3, 4, 5), 31, 5), ((6, 5, 7), 50, 6)])
def test_module_torch_formula_against_float64(shape, m, p):
    from style_transfer import losses
    g = torch.Generator().manual_seed(31)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    c = shape[-3]
    style = torch.randn((c, 1, m), generator=g, dtype=torch.float64).clamp(min=-0.3)
    target = losses.StyleLossSliced.get_target(style)
    assert target.shape == (c, m) and torch.equal(target, style.reshape(c, m))
    module = losses.StyleLossSliced(target, projections=p, seed=5)
    assert 'target' in dict(module.named_buffers()) and module.projections == p and module.epoch == 0
    # the directions the module draws: unit rows, a function of (seed, epoch)
    r = module.draw(0, x.device, x.dtype)
    assert r.shape == (p, c) and float((r.norm(dim=1) - 1).abs().max()) < 1e-6
    assert torch.equal(r, module.draw(0, x.device, x.dtype)) and not torch.equal(r, module.draw(1, x.device, x.dtype))
    xr = x.clone().requires_grad_()
    value = module(xr)
    assert module.epoch == 1                                  # training mode: the epoch advances with every forward
    value.backward()
    batch = x.reshape((-1,) + shape[-3:])
    n = shape[-2] * shape[-1]
    t = sliced_target_formula(r.numpy(), [target.numpy()], [1.0], n)
    wants = [sliced_formula(b.reshape(c, -1).numpy(), r.numpy(), t) for b in batch]
    want = sum(w[0] for w in wants) / len(wants)
    want_grad = np.stack([w[1] for w in wants]).reshape(shape) / len(wants)
    assert abs(value.item() - want) <= 1e-12 * max(abs(want), 1e-30)
    assert np.abs(xr.grad.numpy() - want_grad).max() <= 1e-12 * max(np.abs(want_grad).max(), 1e-30)
    # the next forward uses the next epoch's directions; eval mode and resample=False keep theirs
    assert module(x).item() != value.item() and module.epoch == 2
    module.eval()
    assert module(x).item() == module(x).item() and module.epoch == 2
    fixed = losses.StyleLossSliced(target, projections=p, resample=False, seed=5)
    assert fixed(x).item() == value.item() == fixed(x).item() and fixed.epoch == 0
    with pytest.raises(ValueError, match='columns'):
        losses.StyleLossSliced(torch.zeros(3))
    with pytest.raises(ValueError, match='projections'):
        losses.StyleLossSliced(target, projections=0)


def test_the_target_own_tap_gives_exactly_zero():
    from style_transfer import losses
    g = torch.Generator().manual_seed(32)
    s = torch.randn((6, 3, 4), generator=g, dtype=torch.float64).clamp(min=0)      # ties: exact zeros
    module = losses.StyleLossSliced(losses.StyleLossSliced.get_target(s), projections=9)
    xr = s.clone().requires_grad_()
    value = module(xr)
    value.backward()
    assert value.item() == 0.0 and not xr.grad.any()


def test_identity_directions_give_the_marginal_term():
    from style_transfer import losses
    g = torch.Generator().manual_seed(33)
    x = torch.randn((5, 6, 7), generator=g, dtype=torch.float64).clamp(min=-0.2)
    style = torch.randn((5, 4, 9), generator=g, dtype=torch.float64).clamp(min=-0.2)
    sliced = losses.StyleLossSliced(losses.StyleLossSliced.get_target(style))
    sliced.directions = torch.eye(5, dtype=torch.float64)
    marginal = losses.StyleLossW2Marginal(losses.StyleLossW2Marginal.get_target(style))
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    a, b = sliced(xa), marginal(xb)
    a.backward()
    b.backward()
    assert a.item() == b.item() and torch.equal(xa.grad, xb.grad)
    assert sliced.epoch == 0                                  # given directions: nothing is drawn


def test_resolver_refusals():
    from style_transfer.style_transfer import StyleTransfer, _resolve_style_sliced as resolve
    assert StyleTransfer.style_sliced is False and StyleTransfer.style_sliced_projections is None
    assert StyleTransfer.style_sliced_resample is True and StyleTransfer.style_sliced_seed == 0
    assert StyleTransfer.style_sliced_samples is None
    assert resolve(False, W2) == [False] * 5 and resolve(True, W2) == [True] * 5
    assert resolve(True, ['w2', 'gram', 'w2']) == [True, False, True]
    assert resolve(True, W2, [True, False, False, False, False]) == [False, True, True, True, True]
    assert resolve(True, W2, None, [False, True, False, False, False]) == [True, False, True, True, True]
    assert resolve(True, W2, None, None, [False, False, True, False, False]) == [True, True, False, True, True]
    assert resolve([False, False, False, True, True], W2, samples=4096, projections=128, seed=7) == [False, False, False, True, True]
    assert resolve((0, 1, np.bool_(True)), ['w2'] * 3, samples=np.int64(1), projections=np.int64(512)) == [False, True, True]
    assert resolve(True, W2, resample=False, optimizer='lbfgs') == [True] * 5
    for bad, kinds, kwargs, word in (
            ([True] * 4, W2, {}, '4 flags for 5 layers'),
            ([True, 'yes', False, False, False], W2, {}, 'is not a bool'),
            ([False, 2, False, False, False], W2, {}, 'is not a bool'),
            ('1,1', W2, {}, 'one bool per entry'),
            (1.0, W2, {}, 'one bool per entry'),
            ([False, True, False], ['w2', 'gram', 'w2'], {}, "'gram'"),
            ([True, False, False, False, False], W2, dict(style_diagonal=[True, False, False, False, False]), 'style_diagonal'),
            ([False, True, False, False, False], W2, dict(style_marginal=[False, True, False, False, False]), 'style_marginal'),
            ([False, False, True, False, False], W2, dict(style_nearest=[False, False, True, False, False]), 'style_nearest'),
            ([False, False, False, True, False], W2, dict(style_eps=[None, None, None, 1e-3, None]), 'style_eps'),
            (True, W2, dict(style_eps=[None, None, None, 1e-3, None]), 'style_eps'),
            ([False, False, False, False, True], W2, dict(masked=True), 'style_mask'),
            (True, W2, dict(masked=True), 'style_regions'),
            (True, W2, dict(masked=True), 'style_image_masks'),
            (True, W2, dict(world=2), '2 ranks'),
            ([False, False, False, False, True], W2, dict(world=4), '4 ranks'),
            (False, W2, dict(projections=0), 'style_sliced_projections'),
            (True, W2, dict(projections=96), 'style_sliced_projections'),
            (True, W2, dict(projections=576), 'style_sliced_projections'),
            (True, W2, dict(projections=128.0), 'style_sliced_projections'),
            (True, W2, dict(projections=True), 'style_sliced_projections'),
            (False, W2, dict(samples=0), 'style_sliced_samples'),
            (True, W2, dict(samples=-3), 'style_sliced_samples'),
            (True, W2, dict(samples=2.5), 'style_sliced_samples'),
            (True, W2, dict(samples=True), 'style_sliced_samples'),
            (True, W2, dict(samples='4096'), 'style_sliced_samples'),
            (True, W2, dict(resample=1), 'style_sliced_resample'),
            (True, W2, dict(resample='no'), 'style_sliced_resample'),
            (True, W2, dict(seed=-1), 'style_sliced_seed'),
            (True, W2, dict(seed=1.5), 'style_sliced_seed'),
            (True, W2, dict(optimizer='lbfgs'), 'style_sliced_resample = False'),
            ([False, False, False, False, True], W2, dict(optimizer='lbfgs', resample=True), "optimizer='lbfgs'")):
        with pytest.raises(ValueError, match='style_sliced') as info:
            resolve(bad, kinds, **kwargs)
        assert word in str(info.value), (bad, str(info.value))
    # no set flag: nothing to refuse
    assert resolve(False, W2, masked=True, world=4, style_eps=[1e-3] * 5, optimizer='lbfgs') == [False] * 5
    assert resolve([False] * 5, ['gram'] * 5, masked=True) == [False] * 5


def test_cli_parsing():
    from style_transfer import cli
    parser = cli.build_parser()
    base = ['content.jpg', 'style.jpg']
    args = parser.parse_args(base)
    assert args.style_sliced is False and args.style_sliced_projections is None and args.style_sliced_resample is True
    assert args.style_sliced_seed == 0 and args.style_sliced_samples is None
    assert parser.parse_args(base + ['--style-sliced', '1']).style_sliced is True
    assert parser.parse_args(base + ['--style-sliced', '0']).style_sliced is False
    assert parser.parse_args(base + ['--style-sliced', '0,0,0,1,1']).style_sliced == [False, False, False, True, True]
    assert parser.parse_args(base + ['--style-sliced-projections', '128']).style_sliced_projections == 128
    assert parser.parse_args(base + ['--no-style-sliced-resample']).style_sliced_resample is False
    assert parser.parse_args(base + ['--style-sliced-seed', '12345']).style_sliced_seed == 12345
    assert parser.parse_args(base + ['--style-sliced-samples', '16384']).style_sliced_samples == 16384
    for bad in ('2', 'yes', '1,,0', ''):
        with pytest.raises(SystemExit):
            parser.parse_args(base + ['--style-sliced', bad])
    for flag in ('--style-sliced-samples', '--style-sliced-projections'):
        for bad in ('0', '-1', '1.5', 'many', ''):
            with pytest.raises(SystemExit):
                parser.parse_args(base + [flag, bad])
    for bad in ('-1', '1.5', 'seed', ''):
        with pytest.raises(SystemExit):
            parser.parse_args(base + ['--style-sliced-seed', bad])

    class Holder:
        pass
    st = cli.apply_loss_kinds(Holder(), parser.parse_args(base + ['--style-sliced', '0,1', '--style-marginal', '1,0',
                                                                  '--style-sliced-projections', '64', '--no-style-sliced-resample',
                                                                  '--style-sliced-seed', '3', '--style-sliced-samples', '7']))
    assert st.style_sliced == [False, True] and st.style_marginal == [True, False] and st.style_sliced_projections == 64
    assert st.style_sliced_resample is False and st.style_sliced_seed == 3 and st.style_sliced_samples == 7


def test_the_symbols_are_in_the_header_and_the_binding():
    from style_transfer import _hip, losses
    text = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    lib = _hip.load_library(require_gpu=False)
    for name in ('st_plan_set_style_sliced', 'st_plan_style_sliced', 'st_plan_set_sliced_options', 'st_plan_set_sliced_seed',
                 'st_plan_set_style_sliced_vectors', 'st_plan_sliced_directions', 'st_plan_sliced_target', 'st_op_sliced_directions',
                 'st_op_sliced_scratch_bytes', 'st_op_sliced_target', 'st_op_sliced_project', 'st_op_sliced_loss',
                 'st_op_sliced_loss_backward'):
        assert f'{name}(' in text, name
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for phrase in ('term_j = w_j sum_p sum_k (Y_p,pi_p(k) - T_p,k)^2 / (P N)',
                   'dF     = w_j (2 / (P N)) R^T G,   G_p,pi_p(k) = Y_p,pi_p(k) - T_p,k',
                   'T      = sum_i a_i resample_N(sort_rows(R S_i))',
                   'R and the permutations are constants of the gradient', 'There is no eps',
                   'With R = I and P = C the term is the marginal',
                   'z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9', 'h      = mix(key ^ (p << 32 | c))',
                   'z_pc   = sqrt(-2 ln u1) cos(2 pi u2)', 'It is a HOST counter handed to the direction kernel as an argument',
                   'No floating-point atomics anywhere',
                   'Order of configuration: layers, kinds, eps, diagonal, marginal, nearest, sliced (flags, options, seed), weights, then '
                   'the targets'):
        assert phrase in text, phrase
    assert _hip.STYLE_LOSSES == ('w2', 'gram') and lib.st_abi_version() == 2
    # the scratch: three bound words, Y and G [P][n], two buffers of P n keys with the sort's header; nothing for an empty shape,
    # and nothing of size C x C (it does not grow with C)
    assert lib.st_op_sliced_scratch_bytes(64, 64, 1000) >= 2 * 64 * 1000 * 4 + 2 * 64 * 1000 * 8
    assert lib.st_op_sliced_scratch_bytes(64, 64, 1000) == lib.st_op_sliced_scratch_bytes(512, 64, 1000)
    assert lib.st_op_sliced_scratch_bytes(64, 64, 1000) % 256 == 0 and lib.st_op_sliced_scratch_bytes(64, 0, 5) == 0
    for attr in ('set_style_sliced', 'style_sliced', 'set_sliced_options', 'set_sliced_seed', 'set_style_sliced_vectors',
                 'sliced_directions', 'sliced_target'):
        assert hasattr(_hip.Plan, attr), attr
    for attr in ('op_sliced_directions', 'op_sliced_target', 'op_sliced_project', 'op_sliced_loss', 'op_sliced_loss_backward'):
        assert hasattr(_hip, attr), attr
    assert hasattr(losses, 'StyleLossSliced')

"""The nearest-neighbour feature-matching option of a W2 style layer, the parts that need no GPU: the module's torch formula
(losses.StyleLossNearest) against brute force in float64 written out here, the tie rule, the resolver of
StyleTransfer.style_nearest, the command line, the sample selection of style_nearest_samples, and the header."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO

W2 = ['w2'] * 5


def nearest_formula(f, s):
    """(k*, term, dF) at weight 1 for f [C, N] and s [C, M], float64 numpy, straight from include/st_amd.h: the arg-min of
    |f_i - s_k|^2 by brute force with the lowest k among equal distances, and the match a constant of the gradient."""
    c, n = f.shape
    k = np.empty(n, dtype=np.int64)
    for i in range(n):
        d = ((f[:, i:i + 1] - s) ** 2).sum(0)
        k[i] = int(np.flatnonzero(d == d.min())[0])
    r = f - s[:, k]
    return k, float((r * r).sum() / (c * n)), 2.0 * r / (c * n)


@pytest.mark.parametrize('shape, m', [((3, 4, 5), 17), ((3, 4, 5), 1), ((4, 1, 1), 9), ((2, 3, 4, 5), 7), ((1, 1, 1), 1), ((5, 6, 7), 50)])
def test_module_torch_formula_against_brute_force(shape, m):
    from style_transfer import losses
    g = torch.Generator().manual_seed(21)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    c = shape[-3]
    style = torch.randn((c, 1, m), generator=g, dtype=torch.float64).clamp(min=-0.3)
    target = losses.StyleLossNearest.get_target(style)
    assert target.shape == (c, m) and torch.equal(target, style.reshape(c, m))
    module = losses.StyleLossNearest(target)
    module.chunk = 7                 # several blocks of pixels, the last one short
    assert 'target' in dict(module.named_buffers())
    xr = x.clone().requires_grad_()
    value = module(xr)
    value.backward()
    batch = x.reshape((-1,) + shape[-3:])
    wants = [nearest_formula(b.reshape(c, -1).numpy(), target.numpy()) for b in batch]
    want = sum(w[1] for w in wants) / len(wants)
    want_grad = np.stack([w[2] for w in wants]).reshape(shape) / len(wants)
    assert abs(value.item() - want) <= 1e-13 * max(abs(want), 1e-30)
    assert np.abs(xr.grad.numpy() - want_grad).max() <= 1e-13 * max(np.abs(want_grad).max(), 1e-30)
    got_k = losses.StyleLossNearest.match(x.flatten(-2), target, chunk=7).reshape(len(batch), -1)
    for b, w in enumerate(wants):
        assert np.array_equal(got_k[b].numpy(), w[0])
    with pytest.raises(ValueError, match='columns'):
        losses.StyleLossNearest(torch.zeros(3))


def test_a_tie_goes_to_the_lowest_index():
    from style_transfer import losses
    g = torch.Generator().manual_seed(22)
    s = torch.randn((6, 12), generator=g, dtype=torch.float64)
    s[:, 9] = s[:, 2]
    s[:, 5] = s[:, 2]
    s[:, 11] = s[:, 4]
    f = torch.stack([s[:, 9], s[:, 11], s[:, 0], torch.zeros(6, dtype=torch.float64)], dim=1)
    f[:, :3] += 1e-6
    k = losses.StyleLossNearest.match(f, s)
    want, _, _ = nearest_formula(f.numpy(), s.numpy())
    assert k.tolist()[:3] == [2, 4, 0] and np.array_equal(k.numpy(), want)
    # every distance equal: the first vector
    assert losses.StyleLossNearest.match(torch.zeros((3, 4), dtype=torch.float64), torch.ones((3, 5), dtype=torch.float64)).tolist() == [0] * 4
    # at the target's own vectors the torch term is exactly 0
    module = losses.StyleLossNearest(s)
    xr = s.reshape(6, 3, 4).clone().requires_grad_()
    value = module(xr)
    value.backward()
    assert value.item() == 0.0 and not xr.grad.any()


def test_resolver_refusals():
    from style_transfer.style_transfer import StyleTransfer, _resolve_style_nearest as resolve
    assert StyleTransfer.style_nearest is False and StyleTransfer.style_nearest_samples is None
    assert resolve(False, W2) == [False] * 5 and resolve(True, W2) == [True] * 5
    assert resolve(True, ['w2', 'gram', 'w2']) == [True, False, True]
    assert resolve(True, W2, [True, False, False, False, False]) == [False, True, True, True, True]
    assert resolve(True, W2, None, [False, True, False, False, False]) == [True, False, True, True, True]
    assert resolve([False, False, False, True, True], W2, samples=4096) == [False, False, False, True, True]
    assert resolve((0, 1, np.bool_(True)), ['w2'] * 3, samples=np.int64(1)) == [False, True, True]
    for bad, kinds, kwargs, word in (
            ([True] * 4, W2, {}, '4 flags for 5 layers'),
            ([True, 'yes', False, False, False], W2, {}, 'is not a bool'),
            ([False, 2, False, False, False], W2, {}, 'is not a bool'),
            ('1,1', W2, {}, 'one bool per entry'),
            (1.0, W2, {}, 'one bool per entry'),
            ([False, True, False], ['w2', 'gram', 'w2'], {}, "'gram'"),
            ([True, False, False, False, False], W2, dict(style_diagonal=[True, False, False, False, False]), 'style_diagonal'),
            ([False, True, False, False, False], W2, dict(style_marginal=[False, True, False, False, False]), 'style_marginal'),
            ([False, False, False, True, False], W2, dict(style_eps=[None, None, None, 1e-3, None]), 'style_eps'),
            (True, W2, dict(style_eps=[None, None, None, 1e-3, None]), 'style_eps'),
            ([False, False, False, False, True], W2, dict(masked=True), 'style_mask'),
            (True, W2, dict(masked=True), 'style_regions'),
            (True, W2, dict(masked=True), 'style_image_masks'),
            (True, W2, dict(world=2), '2 ranks'),
            ([False, False, False, False, True], W2, dict(world=4), '4 ranks'),
            (False, W2, dict(samples=0), 'style_nearest_samples'),
            (True, W2, dict(samples=-3), 'style_nearest_samples'),
            (True, W2, dict(samples=2.5), 'style_nearest_samples'),
            (True, W2, dict(samples=True), 'style_nearest_samples'),
            (True, W2, dict(samples='4096'), 'style_nearest_samples')):
        with pytest.raises(ValueError, match='style_nearest') as info:
            resolve(bad, kinds, **kwargs)
        assert word in str(info.value), (bad, str(info.value))
    # no set flag: nothing to refuse
    assert resolve(False, W2, masked=True, world=4, style_eps=[1e-3] * 5) == [False] * 5
    assert resolve([False] * 5, ['gram'] * 5, masked=True) == [False] * 5


def test_sample_selection():
    from style_transfer.style_transfer import _nearest_sample_columns as columns
    assert columns(10, None) == list(range(10))
    assert columns(10, 10) == list(range(10)) and columns(10, 11) == list(range(10)) and columns(1, 1) == [0]
    assert columns(10, 4) == [0, 2, 5, 7]                  # floor(t 10 / 4)
    assert columns(7, 3) == [0, 2, 4] and columns(5, 1) == [0]
    for m, k in ((4096, 1000), (262144, 4096), (99991, 4095), (3, 2)):
        got = columns(m, k)
        assert got == [int(np.floor(t * m / k)) for t in range(k)] == [(t * m) // k for t in range(k)]
        assert len(set(got)) == k and got[0] == 0 and got[-1] < m and got == sorted(got)


def test_cli_parsing():
    from style_transfer import cli
    parser = cli.build_parser()
    base = ['content.jpg', 'style.jpg']
    assert parser.parse_args(base).style_nearest is False and parser.parse_args(base).style_nearest_samples is None
    assert parser.parse_args(base + ['--style-nearest', '1']).style_nearest is True
    assert parser.parse_args(base + ['--style-nearest', '0']).style_nearest is False
    assert parser.parse_args(base + ['--style-nearest', '0,0,0,1,1']).style_nearest == [False, False, False, True, True]
    assert parser.parse_args(base + ['--style-nearest-samples', '4096']).style_nearest_samples == 4096
    for bad in ('2', 'yes', '1,,0', ''):
        with pytest.raises(SystemExit):
            parser.parse_args(base + ['--style-nearest', bad])
    for bad in ('0', '-1', '1.5', 'many', ''):
        with pytest.raises(SystemExit):
            parser.parse_args(base + ['--style-nearest-samples', bad])

    class Holder:
        pass
    st = cli.apply_loss_kinds(Holder(), parser.parse_args(base + ['--style-nearest', '0,1', '--style-marginal', '1,0',
                                                                  '--style-nearest-samples', '7']))
    assert st.style_nearest == [False, True] and st.style_marginal == [True, False] and st.style_nearest_samples == 7


def test_the_symbols_are_in_the_header_and_the_binding():
    from style_transfer import _hip, losses
    text = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    lib = _hip.load_library(require_gpu=False)
    for name in ('st_plan_set_style_nearest', 'st_plan_style_nearest', 'st_plan_set_style_vectors', 'st_plan_nearest_indices',
                 'st_op_nearest_k_chunk', 'st_op_nearest_pixel_tile', 'st_op_nearest_k_tile', 'st_op_nearest_splits',
                 'st_op_nearest_prepared_floats', 'st_op_nearest_scratch_floats', 'st_op_nearest_prepare', 'st_op_nearest_search',
                 'st_op_nearest_loss', 'st_op_nearest_loss_backward'):
        assert f'{name}(' in text, name
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for phrase in ('k*(i)  = argmin_k |f_i - s_k|^2 = argmax_k (<f_i, s_k> - |s_k|^2 / 2),   ties: the lowest k',
                   'term_j = w_j sum_i |f_i - s_k*(i)|^2 / (C N)', 'dF_ci  = w_j (2 / (C N)) (f_ci - s_c,k*(i))',
                   'There is no eps', 'the per-image weights do not enter',
                   'Order of configuration: layers, kinds, eps, diagonal, marginal, nearest, weights, then the targets'):
        assert phrase in text, phrase
    assert _hip.STYLE_LOSSES == ('w2', 'gram') and lib.st_abi_version() == 2
    assert (lib.st_op_nearest_k_chunk(), lib.st_op_nearest_pixel_tile(), lib.st_op_nearest_k_tile()) == (32, 128, 128)
    # the split count is a function of the shape: a split owns at least four k tiles
    assert [lib.st_op_nearest_splits(300, m) for m in (1, 511, 512, 513, 1024, 1025, 4099)] == [1, 1, 1, 2, 2, 3, 9]
    assert lib.st_op_nearest_splits(4096, 4096) == 8 and lib.st_op_nearest_splits(0, 5) == 0
    # ... and it is NOT monotone in M (a split owns whole k tiles): a smaller style set can need more splits and a larger scratch,
    # which is why a plan sizes each buffer by its own function (tests/test_style_nearest_gpu.py crosses this boundary)
    assert (lib.st_op_nearest_splits(6, 257 * 128), lib.st_op_nearest_splits(6, 256 * 128)) == (52, 64)
    assert (lib.st_op_nearest_splits(4096, 129 * 128), lib.st_op_nearest_splits(4096, 128 * 128)) == (26, 32)
    assert lib.st_op_nearest_scratch_floats(512, 4096, 128 * 128) > lib.st_op_nearest_scratch_floats(512, 4096, 129 * 128)
    for n, m in ((6, 256 * 128), (4096, 128 * 128), (300, 1025)):
        assert lib.st_op_nearest_scratch_floats(64, n, m) >= 2 * lib.st_op_nearest_splits(n, m) * n
    # S^T padded to whole k tiles with its bias and bound; one (score, k) per pixel and split; nothing for an empty shape
    assert lib.st_op_nearest_prepared_floats(64, 257) >= 384 * 64 + 384 and lib.st_op_nearest_prepared_floats(0, 5) == 0
    assert lib.st_op_nearest_scratch_floats(64, 300, 1025) >= 2 * 3 * 300 and lib.st_op_nearest_scratch_floats(64, 0, 5) == 0
    # ... and nothing of size N x M: the scratch of relu4_1 at 512^2 is far below the 64 MiB of its score matrix
    assert lib.st_op_nearest_scratch_floats(512, 4096, 4096) * 4 < 1 << 20
    for attr in ('set_style_nearest', 'style_nearest', 'set_style_vectors', 'nearest_indices'):
        assert hasattr(_hip.Plan, attr), attr
    for attr in ('op_nearest_prepare', 'op_nearest_search', 'op_nearest_loss', 'op_nearest_loss_backward', 'nearest_splits',
                 'nearest_geometry'):
        assert hasattr(_hip, attr), attr
    assert hasattr(losses, 'StyleLossNearest')

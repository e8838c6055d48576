"""CPU checks of the Laplacian loss on pooled images (st_plan_set_laplacian / st_plan_laplacian / st_plan_laplacian_terms,
st_op_laplacian_*, losses.LaplacianLoss, StyleTransfer.laplacian_weight / laplacian_pools, --laplacian-weight /
--laplacian-pools) - no GPU needed.

The yardstick is include/st_amd.h's formula, written out here in torch (`formula`) and shared with tests/test_laplacian_gpu.py;
it is NOT losses.LaplacianLoss, which is code under test.  Per pool size p, with Q = avg_pool2d(., p) at floor sizes and L the
4-neighbour Laplacian on the replicate-padded map:
    term_p = mean((L(Q(x)) - L(Q(c))) ** 2),        loss = the sum of the term_p in list order
and the gradient is autograd's on that."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conftest import REPO
from test_loss_kinds_cpu import _bare_style_transfer, _lib

NEW_ENTRIES = ['st_plan_set_laplacian', 'st_plan_laplacian', 'st_plan_laplacian_terms', 'st_op_laplacian_target',
               'st_op_laplacian_value', 'st_op_laplacian_backward']


# ---- the yardstick ----------------------------------------------------------------------------------------------------------
def pooled_laplacian(x, pool):
    """L(Q_p(x)) of a [..., C, H, W] tensor: avg_pool2d with kernel and stride `pool` (trailing rows and columns dropped), then
    4 Q - up - down - left - right on the replicate-padded map."""
    lead = x.shape[:-3]
    q = x.reshape((-1,) + tuple(x.shape[-3:]))
    if pool > 1:
        q = F.avg_pool2d(q, pool)
    p = F.pad(q, (1, 1, 1, 1), mode='replicate')
    lap = 4 * q - p[..., :-2, 1:-1] - p[..., 2:, 1:-1] - p[..., 1:-1, :-2] - p[..., 1:-1, 2:]
    return lap.reshape(lead + tuple(lap.shape[-3:]))


def formula_terms(x, content, pools):
    """[term_p for p in pools] at weight 1: each the mean over the [C][h_p][w_p] map (and any batch)."""
    return [((pooled_laplacian(x, p) - pooled_laplacian(content, p)) ** 2).mean() for p in pools]


def formula(x, content, pools):
    return sum(formula_terms(x, content, pools))


def _pair(shape, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=dtype), torch.rand(shape, generator=g, dtype=dtype)


# ---- the library's surface --------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries():
    header = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    hip, lib = _lib()
    for name in NEW_ENTRIES:
        assert re.search(r'\bint\s+%s\s*\(' % name, text), f'{name} is not declared in st_amd.h'
        assert hasattr(lib, name), f'{name} is not exported by libst_amd.so'
        assert name in hip.EXPORTED_SYMBOLS, f'{name} is not bound by _hip._declare'
    assert lib.st_abi_version() == 2
    for name in ('set_laplacian', 'laplacian_target', 'laplacian_terms'):
        assert callable(getattr(hip.Plan, name, None)), name
    comment = ' '.join(header[:header.index('int st_plan_set_laplacian(')].rsplit('/*', 1)[1].replace('*', ' ').split())
    for phrase in ('avg_pool2d', 'replicate-padded', 'clamped', '3 h_p w_p', 'list order', 'image-space slot', 'exactly 0',
                   'at least 2 x 2', 'equal bits', 'strip plan'):
        assert phrase in comment, f'include/st_amd.h, st_plan_set_laplacian: {phrase!r} is not documented'


# ---- the module's torch path ------------------------------------------------------------------------------------------------
CASES = [((9, 13), (1,)), ((9, 13), (2,)), ((9, 13), (4,)), ((9, 13), (1, 2, 4)), ((40, 48), (4, 16)), ((45, 54), (4, 16))]


@pytest.mark.parametrize('batch', [None, 1, 2], ids=['no-batch', 'batch-1', 'batch-2'])
@pytest.mark.parametrize('size, pools', CASES, ids=[f'{s[0]}x{s[1]}-p{"-".join(map(str, p))}' for s, p in CASES])
def test_module_torch_path_is_the_formula(size, pools, batch):
    from style_transfer import losses
    shape = (3,) + size if batch is None else (batch, 3) + size
    x, content = _pair(shape)
    module = losses.LaplacianLoss(content, pools)
    assert module.pools == tuple(pools)
    buffers = dict(module.named_buffers())
    assert sorted(buffers) == [f'target_{k}' for k in range(len(pools))]
    for k, p in enumerate(pools):
        assert buffers[f'target_{k}'].shape == shape[:-2] + (size[0] // p, size[1] // p)
        assert buffers[f'target_{k}'].dtype == torch.float64 and not buffers[f'target_{k}'].requires_grad
    x = x.requires_grad_(True)
    got = module(x)
    want = formula(x, content, pools)
    assert got.shape == () and got.dtype == torch.float64
    assert abs(float(got.detach()) - float(want.detach())) <= 1e-13 * abs(float(want.detach()))
    (g,) = torch.autograd.grad(got, x)
    (gw,) = torch.autograd.grad(want, x)
    assert float((g - gw).norm()) <= 1e-13 * float(gw.norm())
    assert float(module(content)) == 0.0


def test_module_is_a_sum_in_list_order_and_follows_dtype_and_state_dict():
    from style_transfer import losses
    x, content = _pair((3, 40, 48), seed=3, dtype=torch.float32)
    module = losses.LaplacianLoss(content, (4, 16))
    terms = formula_terms(x, content, (4, 16))
    assert torch.allclose(module(x), terms[0] + terms[1], rtol=1e-5)
    clone = losses.LaplacianLoss(torch.zeros_like(content), (4, 16))
    clone.load_state_dict(module.state_dict())
    assert torch.equal(clone(x), module(x))
    assert module.double()(x.double()).dtype == torch.float64


def test_gradcheck():
    from style_transfer import losses
    x, content = _pair((3, 9, 13), seed=5)
    for pools in ((1,), (2,), (4,), (1, 2, 4)):
        module = losses.LaplacianLoss(content, pools)
        assert torch.autograd.gradcheck(module, (x.clone().requires_grad_(True),), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_dropped_trailing_rows_and_columns_get_exactly_zero_gradient():
    from style_transfer import losses
    x, content = _pair((3, 45, 54), seed=7)
    for make in (lambda: losses.LaplacianLoss(content, (4,)), lambda: (lambda t: formula(t, content, (4,)))):
        xi = x.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(make()(xi), xi)
        assert torch.count_nonzero(g[:, 44, :]) == 0 and torch.count_nonzero(g[:, :, 52:]) == 0
        assert torch.count_nonzero(g[:, :44, :52]) == 3 * 44 * 52


@pytest.mark.parametrize('pools', [(), (1, 2, 3, 4, 5), (4, 4), (0,), (-2,), (2.0,), (True,), 4, ('4',)], ids=str)
def test_module_refuses_bad_pools(pools):
    from style_transfer import losses
    with pytest.raises(ValueError, match='pools'):
        losses.LaplacianLoss(torch.zeros(3, 32, 32), pools)


def test_module_refuses_a_pool_that_leaves_less_than_two_by_two():
    from style_transfer import losses
    with pytest.raises(ValueError, match='2 x 2'):
        losses.LaplacianLoss(torch.zeros(3, 32, 31), (16,))
    losses.LaplacianLoss(torch.zeros(3, 32, 32), (16,))


def test_without_a_hip_tensor_nothing_is_counted_as_native():
    from style_transfer import losses
    x, content = _pair((3, 16, 16), dtype=torch.float32)
    before = losses.native_calls.get('laplacian', 0)
    assert not losses.eligible(x, 'laplacian')
    losses.LaplacianLoss(content, (2,))(x)
    assert losses.native_calls.get('laplacian', 0) == before


# ---- StyleTransfer's attributes ---------------------------------------------------------------------------------------------
def _resolve(weight=1.0, pools=(4,), height=32, width=40, world=1):
    from style_transfer.style_transfer import _resolve_laplacian
    return _resolve_laplacian(weight, pools, height, width, world)


def test_no_term_is_the_default_for_any_world_size():
    from style_transfer import StyleTransfer
    assert StyleTransfer.laplacian_weight == 0. and StyleTransfer.laplacian_pools == (4,)
    for world in (1, 2, 8):
        assert _resolve(0., (4,), world=world) is None
    assert _resolve(2, [4, 16]) == (2.0, (4, 16))
    assert _resolve(0.5, (1,), 2, 2) == (0.5, (1,))


@pytest.mark.parametrize('weight', [-1.0, float('nan'), float('inf'), -float('inf'), 'much', None])
def test_a_bad_weight_names_its_attribute(weight):
    with pytest.raises(ValueError, match='laplacian_weight'):
        _resolve(weight)


@pytest.mark.parametrize('pools', [(), (1, 2, 3, 4, 5), (4, 4), (0,), (-2,), (2.5,), 4, None], ids=str)
def test_bad_pools_name_their_attribute(pools):
    with pytest.raises(ValueError, match='laplacian_pools'):
        _resolve(1.0, pools)
    with pytest.raises(ValueError, match='laplacian_pools'):      # ... whatever the weight
        _resolve(0.0, pools)


def test_a_pool_too_large_for_the_smallest_scale_names_its_attribute():
    assert _resolve(1.0, (16,), 32, 40)
    with pytest.raises(ValueError, match='laplacian_pools.*17.*2 x 2'):
        _resolve(1.0, (4, 17), 32, 40)
    with pytest.raises(ValueError, match='laplacian_pools'):
        _resolve(1.0, (16,), 40, 31)


def test_a_term_is_refused_on_several_ranks():
    with pytest.raises(ValueError, match='laplacian_weight.*strips'):
        _resolve(1.0, (4,), world=2)


def test_stylize_refuses_before_any_device_work():
    from PIL import Image
    image = Image.new('RGB', (64, 48))
    st = _bare_style_transfer(['cuda:0'])
    assert st.laplacian_weight == 0. and st.laplacian_pools == (4,)
    for attribute, bad in (('laplacian_weight', -0.5), ('laplacian_weight', float('nan')), ('laplacian_pools', (4, 4)),
                           ('laplacian_pools', ())):
        st = _bare_style_transfer(['cuda:0'])
        st.laplacian_weight = 1.0
        setattr(st, attribute, bad)
        with pytest.raises(ValueError, match=attribute):
            st.stylize(image, [image])
    st = _bare_style_transfer(['cuda:0'])
    st.laplacian_weight, st.laplacian_pools = 1.0, (32,)          # the smallest scale is 43 x 32 (min_scale 43)
    with pytest.raises(ValueError, match='laplacian_pools.*32'):
        st.stylize(image, [image], min_scale=43, end_scale=64)
    st = _bare_style_transfer(['cuda:0', 'cuda:1'])
    st.laplacian_weight = 1.0
    with pytest.raises(ValueError, match='laplacian_weight.*strips'):
        st.stylize(image, [image])


def test_stylize_keeps_its_signature():
    from style_transfer import StyleTransfer
    assert not {'laplacian_weight', 'laplacian_pools'} & set(StyleTransfer.stylize.__kwdefaults__)
    assert len(StyleTransfer.stylize.__kwdefaults__) == 14


def test_cli_options_parse_and_land_on_the_attributes():
    import types
    from style_transfer import cli
    parser = cli.build_parser()
    args = parser.parse_args(['content.png', 'a.png'])
    assert args.laplacian_weight == 0. and args.laplacian_pools == [4]
    st = cli.apply_laplacian(types.SimpleNamespace(), args)
    assert st.laplacian_weight == 0. and st.laplacian_pools == (4,)
    args = parser.parse_args(['content.png', 'a.png', '--laplacian-weight', '2.5', '--laplacian-pools', '4', '16'])
    st = cli.apply_laplacian(_bare_style_transfer(['cuda:0']), args)
    assert st.laplacian_weight == 2.5 and st.laplacian_pools == (4, 16)
    assert _resolve(st.laplacian_weight, st.laplacian_pools, 64, 64) == (2.5, (4, 16))
    for bad in (['--laplacian-weight'], ['--laplacian-weight', 'x'], ['--laplacian-pools'], ['--laplacian-pools', '2.5']):
        with pytest.raises(SystemExit):
            parser.parse_args(['content.png', 'style.png', *bad])

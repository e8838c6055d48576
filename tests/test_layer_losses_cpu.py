"""CPU checks of a loss kind and an eps per layer (st_plan_set_layer_loss_kinds, st_plan_set_loss_eps, list-valued
StyleTransfer.content_loss / style_loss, content_eps / style_eps, the comma lists of --content-loss / --style-loss and
--content-eps / --style-eps): the header declares the entries and the library exports them, the up-front validation
(`_resolve_layer_losses`) accepts and refuses what it should, stylize() refuses the same before any device work, and the CLI
flags reach the attributes - no GPU needed."""
import os
import re
import types

import pytest

from conftest import REPO
from test_loss_kinds_cpu import _bare_style_transfer, _lib

NEW_ENTRIES = ['st_plan_set_layer_loss_kinds', 'st_plan_layer_loss_kinds', 'st_plan_set_loss_eps', 'st_plan_loss_eps']
W2 = ['w2'] * 5


def _resolve(content_loss='mse', style_loss='w2', content_eps=None, style_eps=None, n_content=1, n_style=5, world=1):
    from style_transfer.style_transfer import _resolve_layer_losses
    return _resolve_layer_losses(content_loss, style_loss, content_eps, style_eps, n_content, n_style, world)


def test_header_declares_and_library_exports_the_entries():
    header = open(os.path.join(REPO, 'include', 'st_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    hip, lib = _lib()
    for name in NEW_ENTRIES:
        assert re.search(r'\bint\s+%s\s*\(' % name, text), f'{name} is not declared in st_amd.h'
        assert hasattr(lib, name), f'{name} is not exported by libst_amd.so'
        assert name in hip.EXPORTED_SYMBOLS, f'{name} is not bound by _hip._declare'
    assert lib.st_abi_version() == 2 and re.search(r'#define\s+ST_AMD_ABI_VERSION\s+2\b', header)
    assert hip.CONTENT_LOSSES == ('mse', 'scaled_mse') and hip.STYLE_LOSSES == ('w2', 'gram')
    assert (hip.Plan.content_loss, hip.Plan.style_loss) == ('mse', 'w2')
    for name in ('set_layer_loss_kinds', 'set_loss_eps', 'content_losses', 'style_losses', 'content_eps', 'style_eps'):
        assert hasattr(hip.Plan, name), name


@pytest.mark.parametrize('world', [1, 2, 8])
def test_the_defaults_pass_for_any_world_size(world):
    want = (['mse'], W2, [None], [None] * 5)
    assert _resolve(world=world) == want
    assert _resolve(['mse'], tuple(W2), None, [None] * 5, world=world) == want
    # an eps that IS its kind's default as a float is the default
    assert _resolve('mse', W2, [None], 1e-4, world=world) == want


def test_strings_lists_and_tuples():
    mixed = ['w2', 'w2', 'w2', 'gram', 'gram']
    assert _resolve('scaled_mse', 'gram') == (['scaled_mse'], ['gram'] * 5, [None], [None] * 5)
    assert _resolve(['scaled_mse'], mixed)[:2] == (['scaled_mse'], mixed)
    assert _resolve(('scaled_mse',), tuple(mixed))[:2] == (['scaled_mse'], mixed)
    assert _resolve(['mse', 'scaled_mse'], [], n_content=2, n_style=0)[:2] == (['mse', 'scaled_mse'], [])
    # eps: None, a number for every layer, or one per layer with None for the default
    assert _resolve('scaled_mse', mixed, 1e-3, 1e-2)[2:] == ([1e-3], [1e-2] * 5)
    assert _resolve('scaled_mse', mixed, [0.5], (1e-2, None, None, None, 1e-3))[2:] == ([0.5], [1e-2, None, None, None, 1e-3])
    assert _resolve('mse', mixed, [None], [None, None, 1e-4, 1e-8, 1e-4])[2:] == ([None], [None, None, None, None, 1e-4])
    assert _resolve('mse', 'w2', None, 0)[3] == [0.0] * 5


@pytest.mark.parametrize('kwargs, attribute', [
    (dict(style_loss=['w2', 'gram']), 'style_loss'),
    (dict(style_loss=W2 + ['w2']), 'style_loss'),
    (dict(content_loss=['mse', 'mse']), 'content_loss'),
    (dict(content_loss=[]), 'content_loss'),
    (dict(style_eps=[1e-2, 1e-2]), 'style_eps'),
    (dict(content_loss='scaled_mse', content_eps=[1e-3, 1e-3]), 'content_eps'),
])
def test_a_wrong_length_is_refused(kwargs, attribute):
    with pytest.raises(ValueError, match=attribute):
        _resolve(**kwargs)


@pytest.mark.parametrize('kwargs, attribute, choices', [
    (dict(style_loss=['w2', 'w2', 'gatys', 'w2', 'w2']), 'style_loss', ['w2', 'gram']),
    (dict(style_loss=['w2', 'w2', 'w2', 'w2', None]), 'style_loss', ['w2', 'gram']),
    (dict(content_loss=['l1']), 'content_loss', ['mse', 'scaled_mse']),
    (dict(content_loss=None), 'content_loss', ['mse', 'scaled_mse']),
    (dict(style_loss='gatys', n_style=0), 'style_loss', ['w2', 'gram']),
])
def test_an_unknown_name_is_refused_with_the_choices(kwargs, attribute, choices):
    with pytest.raises(ValueError, match=attribute) as err:
        _resolve(**kwargs)
    for name in choices:
        assert repr(name) in str(err.value), str(err.value)


@pytest.mark.parametrize('kwargs, attribute', [
    (dict(content_eps=1e-3), 'content_eps'),                                 # ContentLossMSE has no eps
    (dict(content_eps=[1e-8]), 'content_eps'),
    (dict(content_loss=['mse', 'scaled_mse'], content_eps=[1e-3, 1e-3], n_content=2), 'content_eps'),
    (dict(style_eps=-1e-4), 'style_eps'),
    (dict(style_eps=[None, None, -1.0, None, None]), 'style_eps'),
    (dict(style_eps=float('nan')), 'style_eps'),
    (dict(style_eps=[None, None, None, None, float('inf')]), 'style_eps'),
    (dict(content_loss='scaled_mse', content_eps=float('nan')), 'content_eps'),
])
def test_a_bad_eps_is_refused(kwargs, attribute):
    with pytest.raises(ValueError, match=attribute):
        _resolve(**kwargs)


@pytest.mark.parametrize('kwargs', [
    dict(style_loss=['w2', 'w2', 'w2', 'gram', 'gram']),
    dict(content_loss=['scaled_mse']),
    dict(style_eps=[None, None, None, None, 1e-2]),
    dict(style_eps=1e-3),
    dict(content_loss='scaled_mse', content_eps=1e-3),
])
def test_a_non_default_entry_is_refused_on_several_ranks(kwargs):
    assert _resolve(**kwargs, world=1)
    with pytest.raises(ValueError, match='strips'):
        _resolve(**kwargs, world=2)


def test_stylize_refuses_before_any_device_work():
    from style_transfer import StyleTransfer
    assert (StyleTransfer.content_eps, StyleTransfer.style_eps) == (None, None)          # class attributes
    st = _bare_style_transfer(['cuda:0', 'cuda:1'])
    assert (st.content_eps, st.style_eps) == (None, None)
    st.style_loss = ['w2', 'w2', 'w2', 'gram', 'gram']
    with pytest.raises(ValueError, match='strips'):
        st.stylize(None, [None])
    st.style_loss, st.style_eps = 'w2', [1e-2, None, None, None, None]
    with pytest.raises(ValueError, match='strips'):
        st.stylize(None, [None])
    st = _bare_style_transfer(['cuda:0'])
    st.style_loss = ['w2', 'gram']
    with pytest.raises(ValueError, match='style_loss'):
        st.stylize(None, [None])
    st.style_loss = ['w2', 'w2', 'w2', 'gram', 'gatys']
    with pytest.raises(ValueError, match=r"'w2', 'gram'"):
        st.stylize(None, [None])
    st.style_loss, st.content_eps = 'w2', 1e-3
    with pytest.raises(ValueError, match='content_eps'):
        st.stylize(None, [None])
    st.content_eps, st.style_eps = None, [1e-2, None, None, None, float('nan')]
    with pytest.raises(ValueError, match='style_eps'):
        st.stylize(None, [None])


def test_stylize_keeps_its_signature():
    from style_transfer import StyleTransfer
    assert not {'content_loss', 'style_loss', 'content_eps', 'style_eps'} & set(StyleTransfer.stylize.__kwdefaults__)
    assert len(StyleTransfer.stylize.__kwdefaults__) == 14


def test_cli_flags_parse_and_land_on_the_attributes():
    from style_transfer import cli
    parser = cli.build_parser()
    args = parser.parse_args(['content.png', 'style.png'])
    st = cli.apply_loss_kinds(types.SimpleNamespace(), args)
    assert (st.content_loss, st.style_loss, st.content_eps, st.style_eps) == ('mse', 'w2', None, None)
    args = parser.parse_args(['content.png', 'style.png', '--style-loss', 'w2,w2,w2,gram,gram', '--content-loss', 'scaled_mse',
                              '--style-eps', '1e-2,,,,1e-3', '--content-eps', '1e-3'])
    st = cli.apply_loss_kinds(_bare_style_transfer(['cuda:0']), args)
    assert st.style_loss == ['w2', 'w2', 'w2', 'gram', 'gram'] and st.content_loss == 'scaled_mse'
    assert st.style_eps == [0.01, None, None, None, 0.001] and st.content_eps == 1e-3
    from style_transfer.style_transfer import _resolve_layer_losses
    assert _resolve_layer_losses(st.content_loss, st.style_loss, st.content_eps, st.style_eps, 1, 5) == (
        ['scaled_mse'], ['w2', 'w2', 'w2', 'gram', 'gram'], [1e-3], [0.01, None, None, None, 0.001])
    args = parser.parse_args(['content.png', 'style.png', '--style-loss', 'gram'])
    assert args.style_loss == 'gram'                                     # a single name stays the plain string
    for bad in (['--style-loss', 'w2,w2,w2,gram,gatys'], ['--content-loss', 'mse,l1'], ['--style-loss', 'w2,'],
                ['--style-eps', '1e-2,x']):
        with pytest.raises(SystemExit):
            parser.parse_args(['content.png', 'style.png', *bad])
